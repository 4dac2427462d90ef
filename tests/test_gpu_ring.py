"""GPU parity for the Ring-VRF rows a10 / a13 / a9 of SURVEY.md §8 through the C ABI:
SRS load, `ring_proof::index` (ring commitment) and `RingProver::prove` (blinding disabled) must
reproduce the reference's ring vectors byte for byte (src/ring.rs:1529-1571): `ring_pks_com`
(144 B / 96 B) and `ring_proof` (592 B / 480 B), for both suites; the proofs also verify under the
oracle's verifier (BLS12-381)."""
import json
import os

import pytest

from helpers import xy
from oracle import ring_py as R

pytestmark = pytest.mark.gpu
FILES = {0: ("bandersnatch_sha-512_ell2_ring.json", "bls12-381-srs-2-11-uncompressed-zcash.bin"),
         1: ("baby-jubjub_sha-512_tai_ring.json", "bn254-testing-2-9-uncompressed.bin")}


@pytest.fixture(scope="module")
def env(golden_dir):
    from ark_vrf_amd import _native as nat
    from ark_vrf_amd.ring import RingSetup
    out = {}
    for i, (vec, srsf) in FILES.items():
        srs = open(os.path.join(golden_dir, srsf), "rb").read()
        ctx = nat.Context(i)
        out[i] = (ctx, RingSetup(ctx, srs, 8), json.load(open(os.path.join(golden_dir, vec))), srs)
    return out


@pytest.mark.parametrize("suite", [0, 1])
def test_setup_parameters(env, suite):
    ctx, setup, vs, srs = env[suite]
    assert setup.domain_size == 512                                        # src/ring.rs:810-821, TEST_RING_SIZE = 8
    assert setup.max_ring_size == 512 - 4 - (253 if suite == 0 else 251)   # src/ring.rs:298-300
    assert (setup.proof_len, setup.commitment_len) == ((592, 144) if suite == 0 else (480, 96))


@pytest.mark.parametrize("suite", [0, 1])
def test_ring_capacity_exceeded(env, suite):
    """ring_size_exceeded (src/ring.rs:1145-1170): SRS too short / too many keys."""
    from ark_vrf_amd import _native as nat
    from ark_vrf_amd.ring import RingSetup
    ctx, setup, vs, srs = env[suite]
    with pytest.raises(nat.AvrfError, match="-> 3"):
        RingSetup(ctx, srs, 100000)
    pk = xy(suite, bytes.fromhex(vs[0]["pk"]))
    with pytest.raises(nat.AvrfError, match="-> 3"):
        setup.index([pk] * (setup.max_ring_size + 1))


@pytest.mark.parametrize("suite", [0, 1])
def test_reference_ring_vectors(env, suite):
    ctx, setup, vs, srs = env[suite]
    s = R.SUITES[suite]
    for v in vs:
        raw = bytes.fromhex(v["ring_pks"])
        pks = [xy(suite, raw[32 * i: 32 * i + 32]) for i in range(len(raw) // 32)]
        key = setup.index(pks)
        assert key.commitment.hex() == v["ring_pks_com"]                   # RingCommitment, 3 KZG commits
        idx = pks.index(xy(suite, bytes.fromhex(v["pk"])))
        proof = key.prove([idx], [bytes.fromhex(v["blinding"])])[0]
        assert proof.hex() == v["ring_proof"]                              # full deterministic ring proof
        key.close()


def test_gpu_proof_verifies_under_oracle(env):
    """A proof made on the GPU for a ring/prover not in the vectors is accepted by the oracle's
    RingVerifier restatement (pairing check), and rejected for another key commitment."""
    import oracle as orc
    ctx, setup, vs, srs_bytes = env[0]
    s = R.SUITES[0]
    sks = [orc.from_seed(0, bytes([40 + i]) + bytes(31)) for i in range(5)]
    pks = [xy(0, pk) for _, pk in sks]
    key = setup.index(pks)
    h = orc.hash_to_curve(0, b"ring-gpu-test")
    sk, pk = sks[2]
    ped, blinding = orc.pedersen_prove(0, sk, [(h, orc.vrf_output(0, sk, h))], b"ad")
    proof = key.prove([2], [blinding])[0]
    prm = R.Params(s, ring_size=8)
    srs = R.Srs(s, srs_bytes)
    fixed = [R.g1_decode_compressed(s, key.commitment[48 * i: 48 * i + 48]) for i in range(3)]
    inst = R.te_decode(s, ped[:32])                                        # Yb = pk + b*B
    assert R.verify(prm, srs, fixed, proof, inst)
    assert not R.verify(prm, srs, fixed, proof, R.te_add(s, inst, s.blinding_base))
    # and the oracle's own prover gives the same bytes
    cols = R.index(prm, srs, [R.te_decode(s, p) for _, p in sks])
    want, _ = R.prove(prm, srs, cols, 2, int.from_bytes(blinding, "little"))
    assert proof == want


def test_ring_1024_matches_oracle(env, golden_dir):
    """BASELINE configs[3] shape: ring of 1024 keys -> PIOP domain N = 2048, SRS 6145 G1 powers.  No reference
    vector exists at this size (SURVEY.md §8c iii): commitment and proof are pinned to the oracle, which is
    itself pinned at N = 512."""
    import hashlib
    from ark_vrf_amd.ring import RingSetup
    ctx, _, _, srs_bytes = env[0]
    s = R.SUITES[0]
    setup = RingSetup(ctx, srs_bytes, 1024)
    assert setup.domain_size == 2048 and setup.max_ring_size == 2048 - 257
    ks = b"".join((int.from_bytes(hashlib.sha512(b"k%d" % i).digest(), "little") % (s.r >> 3) + 1).to_bytes(32, "little") for i in range(1024))
    pks_xy = ctx.scalar_mul_base(ks)
    pkl = [pks_xy[64 * i: 64 * i + 64] for i in range(1024)]
    key = setup.index(pkl)
    prm = R.Params(s, ring_size=1024)
    srs = R.Srs(s, srs_bytes)
    keys = [(int.from_bytes(p[:32], "little"), int.from_bytes(p[32:], "little")) for p in pkl]
    cols = R.index(prm, srs, keys)
    assert key.commitment == R.commitment_bytes(s, cols)
    b = int.from_bytes(hashlib.sha512(b"blinding").digest(), "little") % (s.r >> 3)
    proof = key.prove([777], [b.to_bytes(32, "little")])[0]
    want, _ = R.prove(prm, srs, cols, 777, b)
    assert proof == want


@pytest.mark.parametrize("suite", [0, 1])
def test_ring_verify_reference_vectors(env, suite):
    """a11 / a12: the reference's ring proofs verify one by one and as ONE multi-ring batch (every vector
    has its own ring: its public key sits at index 3 of an otherwise common ring, src/ring.rs:1475-1478);
    perturbations are rejected (prove_verify_batch, src/ring.rs:1017-1140)."""
    from ark_vrf_amd.ring import ring_batch_verify
    ctx, setup, vs, srs = env[suite]
    coms = [bytes.fromhex(v["ring_pks_com"]) for v in vs]
    insts = [xy(suite, bytes.fromhex(v["proof_pk_com"])) for v in vs]
    proofs = [bytes.fromhex(v["ring_proof"]) for v in vs]
    for i in (0, 4):
        assert ring_batch_verify(setup, [coms[i]], None, [insts[i]], [proofs[i]]) == 0       # single verify
    assert ring_batch_verify(setup, coms, list(range(7)), insts, proofs) == 0                # multi-ring batch
    assert ring_batch_verify(setup, [], None, [], []) == 0
    # wrong ring for one item
    assert ring_batch_verify(setup, coms, [1, 1, 2, 3, 4, 5, 6], insts, proofs) == 1
    # tampered evaluation / tampered commitment point / other key commitment
    fq = 48 if suite == 0 else 32
    bad = bytearray(proofs[2]); bad[4 * fq + 5] ^= 1
    assert ring_batch_verify(setup, coms, list(range(7)), insts, proofs[:2] + [bytes(bad)] + proofs[3:]) == 1
    swapped = proofs[:5] + [proofs[6], proofs[5]]
    assert ring_batch_verify(setup, coms, list(range(7)), insts, swapped) == 1
    assert ring_batch_verify(setup, coms, list(range(7)), insts[1:] + insts[:1], proofs) == 1
    junk = bytearray(proofs[0]); junk[1:fq] = b"\x7f" * (fq - 1)
    assert ring_batch_verify(setup, [coms[0]], None, [insts[0]], [bytes(junk)]) in (1, 2)   # undecodable or wrong


@pytest.mark.parametrize("suite", [0, 1])
def test_ring_verify_each(env, suite):
    """n x ring::Verifier::verify (src/ring.rs:228-247) with per-proof statuses: G1 sums and the 2-pairing checks of all proofs
    on the device for many proofs, on the host pool for <= 16, one lone verification as a batch of one (avrf_ring_verify_each).  The
    reference's vectors verify; exactly the perturbed proofs are reported."""
    from ark_vrf_amd.ring import ring_batch_verify, ring_verify_each
    ctx, setup, vs, srs = env[suite]
    coms = [bytes.fromhex(v["ring_pks_com"]) for v in vs]
    insts = [xy(suite, bytes.fromhex(v["proof_pk_com"])) for v in vs]
    proofs = [bytes.fromhex(v["ring_proof"]) for v in vs]
    assert ring_verify_each(setup, coms, list(range(7)), insts, proofs) == [0] * 7
    assert ring_verify_each(setup, [coms[3]], None, [insts[3]], [proofs[3]]) == [0]
    assert ring_verify_each(setup, [], None, [], []) == []
    fq = 48 if suite == 0 else 32
    bad = list(proofs)
    b2 = bytearray(bad[2]); b2[4 * fq + 5] ^= 1; bad[2] = bytes(b2)                       # an evaluation
    b5 = bytearray(bad[5]); b5[4 * fq + 7 * 32 + fq + 31] = 0xff; bad[5] = bytes(b5)      # a scalar >= r: InvalidData
    assert ring_verify_each(setup, coms, list(range(7)), insts, bad) == [0, 0, 1, 0, 0, 2, 0]
    # one verification per call (the batch-of-one form: MSM engine + host pairing) reports the same statuses
    assert [ring_verify_each(setup, [coms[i]], None, [insts[i]], [bad[i]])[0] for i in range(7)] == [0, 0, 1, 0, 0, 2, 0]
    assert ring_verify_each(setup, coms, [4], [insts[3]], [proofs[3]]) == [1]             # against the wrong ring
    assert ring_batch_verify(setup, coms, list(range(7)), insts, bad) == 2                # the batch verifier only sees "something is wrong"
    assert ring_verify_each(setup, coms, [0, 1, 2, 4, 3, 5, 6], insts, proofs) == [0, 0, 0, 1, 1, 0, 0]      # two proofs against the wrong ring
    assert ring_verify_each(setup, coms, list(range(7)), insts[1:] + insts[:1], proofs) == [1] * 7
    if suite == 0:                                                                        # off-subgroup commitment in one proof
        s = R.SUITES[0]
        x = 0x13c60d23238642ea126a1e48cc11d357c30d8b7628dbd25e63b229f1c4069545de11cc9dea959c212e9c82b1478c281d
        y = 0x173eb497b4648ea412daae1e11fa194e01a1d4bf7376e7bad3ef138322e23c3c5114b8a96c915d51db072395e4ad9649
        off = R.g1_encode(s, (x, y), True)
        bad = list(proofs); bad[4] = off + bad[4][48:]
        assert ring_verify_each(setup, coms, list(range(7)), insts, bad) == [0, 0, 0, 0, 2, 0, 0]
        assert ring_verify_each(setup, [coms[4]], None, [insts[4]], [bad[4]]) == [2]


@pytest.mark.parametrize("suite", [0, 1])
def test_ring_verify_large_batch_device_decompression(env, suite):
    """Batches of >= 128 proofs take the G1 square roots on the device (k_g1_decompress): the reference's seven vectors repeated
    to 140 items must give the verdicts the small-batch (host decode) path gives item by item -- valid, a perturbed
    evaluation, an x with no curve point, a flipped sort flag (the other root: a valid point, wrong equation), the canonical
    and a non-canonical infinity, an x >= p, and (BLS12-381) a point outside the prime-order subgroup."""
    from ark_vrf_amd.ring import ring_batch_verify, ring_verify_each
    ctx, setup, vs, srs = env[suite]
    s = R.SUITES[suite]
    fq = 48 if suite == 0 else 32
    reps = 20
    coms = [bytes.fromhex(v["ring_pks_com"]) for v in vs]
    insts = [xy(suite, bytes.fromhex(v["proof_pk_com"])) for v in vs] * reps
    proofs = [bytes.fromhex(v["ring_proof"]) for v in vs] * reps
    rings = list(range(7)) * reps
    n = len(proofs)
    assert n >= 128
    assert ring_batch_verify(setup, coms, rings, insts, proofs) == 0
    assert ring_verify_each(setup, coms, rings, insts, proofs) == [0] * n

    def x_without_point():
        x = 5
        while R.sqrt_mod((x * x * x + s.g1_b) % s.p, s.p) is not None:
            x += 1
        return x

    def enc_x(x, flags):                                   # the compressed form with the given flag bits
        if suite == 0:
            b = bytearray(x.to_bytes(48, "big")); b[0] |= flags; return bytes(b)
        b = bytearray(x.to_bytes(32, "little")); b[31] |= flags; return bytes(b)

    bad = list(proofs)
    exp = [0] * n
    b = bytearray(bad[9]); b[4 * fq + 5] ^= 1; bad[9] = bytes(b); exp[9] = 1                        # an evaluation
    bad[17] = enc_x(x_without_point(), 0x80 if suite == 0 else 0) + bad[17][fq:]; exp[17] = 2       # not on the curve
    b = bytearray(bad[30]); b[0 if suite == 0 else fq - 1] ^= (0x20 if suite == 0 else 0x80); bad[30] = bytes(b); exp[30] = 1   # -P
    inf = (bytes([0xC0]) + bytes(47)) if suite == 0 else (bytes(31) + bytes([0x40]))
    bad[44] = inf + bad[44][fq:]; exp[44] = 1                                                       # canonical infinity decodes
    bad[51] = (bytes([0xC0]) + bytes(46) + b"\x01" if suite == 0 else b"\x01" + bytes(30) + bytes([0x40])) + bad[51][fq:]; exp[51] = 2
    bad[66] = enc_x(s.p + 1, 0x80 if suite == 0 else 0) + bad[66][fq:]; exp[66] = 2                # x >= p
    if suite == 0:
        x = 0x13c60d23238642ea126a1e48cc11d357c30d8b7628dbd25e63b229f1c4069545de11cc9dea959c212e9c82b1478c281d
        y = 0x173eb497b4648ea412daae1e11fa194e01a1d4bf7376e7bad3ef138322e23c3c5114b8a96c915d51db072395e4ad9649
        bad[100] = bad[100][:-48] + R.g1_encode(s, (x, y), True); exp[100] = 2                     # opening proof outside G1
    got = ring_verify_each(setup, coms, rings, insts, bad)
    assert got == exp
    # the same items through the small-batch path (host decode), seven at a time
    small = []
    for k in range(0, n, 7):
        small += ring_verify_each(setup, coms, rings[k: k + 7], insts[k: k + 7], bad[k: k + 7])
    assert small == exp
    assert ring_batch_verify(setup, coms, rings, insts, bad) in (1, 2)
    only_eq = list(proofs); only_eq[9] = bad[9]
    assert ring_batch_verify(setup, coms, rings, insts, only_eq) == 1
    only_dec = list(proofs); only_dec[17] = bad[17]
    assert ring_batch_verify(setup, coms, rings, insts, only_dec) == 2


@pytest.mark.parametrize("suite", [0, 1])
def test_ring_verify_each_host_decode_device_pairing(env, suite):
    """17 to 127 independent verifications decompress their G1 points on the host pool and run their pairing checks on the device:
    the seven vectors three times (21 items), with a perturbed evaluation, a scalar >= r and an item checked against the wrong ring."""
    from ark_vrf_amd.ring import ring_batch_verify, ring_verify_each
    ctx, setup, vs, srs = env[suite]
    fq = 48 if suite == 0 else 32
    coms = [bytes.fromhex(v["ring_pks_com"]) for v in vs]
    insts = [xy(suite, bytes.fromhex(v["proof_pk_com"])) for v in vs] * 3
    proofs = [bytes.fromhex(v["ring_proof"]) for v in vs] * 3
    rings = list(range(7)) * 3
    assert ring_batch_verify(setup, coms, rings, insts, proofs) == 0
    bad, exp = list(proofs), [0] * 21
    b = bytearray(bad[9]); b[4 * fq + 5] ^= 1; bad[9] = bytes(b); exp[9] = 1                          # an evaluation
    b = bytearray(bad[12]); b[4 * fq + 7 * 32 + fq + 31] = 0xff; bad[12] = bytes(b); exp[12] = 2      # lin_zw >= r: InvalidData
    wrong = list(rings); wrong[17] = (rings[17] + 1) % 7; exp[17] = 1                                 # against the wrong ring
    assert ring_verify_each(setup, coms, wrong, insts, bad) == exp


def test_ring_verify_validates_g1_points(env):
    """Validate::Yes of the deserialised RingProof / RingCommitment points: a BLS12-381 G1 point ON the curve but
    OUTSIDE the prime-order subgroup (cofactor ~2^126) and a non-canonical encoding of infinity are InvalidData, not merely
    a failed equation; the canonical infinity decodes (and then fails the equation)."""
    from ark_vrf_amd.ring import ring_batch_verify
    ctx, setup, vs, srs = env[0]
    s = R.SUITES[0]
    v = vs[0]
    com, inst, proof = bytes.fromhex(v["ring_pks_com"]), xy(0, bytes.fromhex(v["proof_pk_com"])), bytes.fromhex(v["ring_proof"])
    assert ring_batch_verify(setup, [com], None, [inst], [proof]) == 0
    x = 0x13c60d23238642ea126a1e48cc11d357c30d8b7628dbd25e63b229f1c4069545de11cc9dea959c212e9c82b1478c281d
    y = 0x173eb497b4648ea412daae1e11fa194e01a1d4bf7376e7bad3ef138322e23c3c5114b8a96c915d51db072395e4ad9649
    assert (y * y - x * x * x - 4) % s.p == 0 and R.g1_mul(s.p, (x, y, 1), s.r) is not None      # on E(Fp), not in G1
    off = R.g1_encode(s, (x, y), True)
    assert ring_batch_verify(setup, [com], None, [inst], [off + proof[48:]]) == 2                # proof commitment
    assert ring_batch_verify(setup, [com], None, [inst], [proof[:-48] + off]) == 2               # opening proof
    assert ring_batch_verify(setup, [off + com[48:]], None, [inst], [proof]) == 2                # ring commitment
    inf = bytes([0xC0]) + bytes(47)
    assert ring_batch_verify(setup, [com], None, [inst], [inf + proof[48:]]) == 1                # canonical infinity: decodes, fails
    assert ring_batch_verify(setup, [com], None, [inst], [bytes([0xC0]) + bytes(46) + b"\x01" + proof[48:]]) == 2
    assert ring_batch_verify(setup, [com], None, [inst], [bytes([0xE0]) + bytes(47) + proof[48:]]) == 2   # infinity with the sort flag
    # BN254 (cofactor 1): infinity flag with a non-zero x is rejected as well
    ctx1, setup1, vs1, _ = env[1]
    v1 = vs1[0]
    com1, inst1, proof1 = bytes.fromhex(v1["ring_pks_com"]), xy(1, bytes.fromhex(v1["proof_pk_com"])), bytes.fromhex(v1["ring_proof"])
    assert ring_batch_verify(setup1, [com1], None, [inst1], [proof1]) == 0
    assert ring_batch_verify(setup1, [com1], None, [inst1], [b"\x01" + bytes(30) + bytes([0x40]) + proof1[32:]]) == 2
    assert ring_batch_verify(setup1, [com1], None, [inst1], [bytes(31) + bytes([0x40]) + proof1[32:]]) == 1


def test_ring_vrf_end_to_end_gpu(env):
    """ring::Prover::prove + ring::Verifier::verify composed from the ABI pieces (src/ring.rs:211-247): Pedersen
    proof + ring proof for the returned blinding; verify = Pedersen verify + ring verify of Yb."""
    import hashlib
    from ark_vrf_amd._native import Batch
    from ark_vrf_amd.ring import ring_batch_verify
    ctx, setup, vs, srs = env[0]
    r_te = 0x1cfb69d4ca675f520cce760202687600ff8f87007419047174fd06b52876e7e1
    sks = [(int.from_bytes(hashlib.sha512(b"e2e%d" % i).digest(), "little") % r_te).to_bytes(32, "little") for i in range(6)]
    pks = ctx.scalar_mul_base(b"".join(sks))
    pkl = [pks[64 * i: 64 * i + 64] for i in range(6)]
    key = setup.index(pkl)
    inputs = ctx.scalar_mul_base(b"".join((i + 7).to_bytes(32, "little") for i in range(6)))
    outs = ctx.scalar_mul(b"".join(sks), inputs)
    ios = [[(inputs[64 * i: 64 * i + 64], outs[64 * i: 64 * i + 64])] for i in range(6)]
    ads = [b"ad%d" % i for i in range(6)]
    ped, blind = ctx.pedersen_prove(Batch.from_items(ios, ads, sks=sks, pks_xy=pkl))
    pedl = [ped[256 * i: 256 * i + 256] for i in range(6)]
    rproofs = key.prove(list(range(6)), [blind[32 * i: 32 * i + 32] for i in range(6)])
    assert ctx.pedersen_batch_verify(ios, ads, pedl) == 0
    ybs = [p[:64] for p in pedl]
    assert ring_batch_verify(setup, [key.commitment], None, ybs, rproofs) == 0
    # a proof by a key outside the ring: index with a different key set
    key2 = setup.index(pkl[:5] + [pkl[0]])
    assert ring_batch_verify(setup, [key2.commitment], None, ybs, rproofs) == 1


@pytest.mark.parametrize("suite", [0, 1])
def test_hiding_proofs(env, suite):
    """blinding_mode 1 (the reference's default hiding RingContext, src/ring.rs:277-295): the 3 zero-knowledge rows
    of every witness column are random, so two proofs of one statement differ, both verify (GPU verifier for both
    suites, oracle verifier for BLS12-381), and a proof for another instance is rejected."""
    import oracle as orc
    from ark_vrf_amd.ring import ring_batch_verify
    ctx, setup, vs, srs_bytes = env[suite]
    s = R.SUITES[suite]
    sks = [orc.from_seed(suite, bytes([90 + i]) + bytes(31)) for i in range(6)]
    key = setup.index([xy(suite, pk) for _, pk in sks])
    h = orc.hash_to_curve(suite, b"hiding")
    items = []
    for j in (0, 5, 2):
        sk, pk = sks[j]
        ped, blinding = orc.pedersen_prove(suite, sk, [(h, orc.vrf_output(suite, sk, h))], b"ad%d" % j)
        items.append((j, blinding, xy(suite, ped[:32])))
    idx = [j for j, _, _ in items]; bl = [b for _, b, _ in items]; ybs = [y for _, _, y in items]
    p1 = key.prove(idx, bl, blinding_mode=1)
    p2 = key.prove(idx, bl, blinding_mode=1)
    p0 = key.prove(idx, bl, blinding_mode=0)
    assert all(a != b for a, b in zip(p1, p2)) and all(a != b for a, b in zip(p1, p0))
    for proofs in (p0, p1, p2):
        assert ring_batch_verify(setup, [key.commitment], None, ybs, proofs) == 0
    assert ring_batch_verify(setup, [key.commitment], None, ybs[1:] + ybs[:1], p1) == 1
    if suite == 0:
        prm = R.Params(s, ring_size=8)
        srs = R.Srs(s, srs_bytes)
        fixed = [R.g1_decode_compressed(s, key.commitment[48 * i: 48 * i + 48]) for i in range(3)]
        for (j, b, y), proof in zip(items, p1):
            inst = (int.from_bytes(y[:32], "little"), int.from_bytes(y[32:], "little"))
            assert R.verify(prm, srs, fixed, proof, inst)


def test_witness_edge_cases_match_oracle(env):
    """Sparse witness path at its corners: signer in the first / last key slot of a FULL ring, blinding with every
    bit set (253 ones -> 254 accumulator steps) and the zero blinding; bytes equal the oracle prover's."""
    ctx, setup, vs, srs_bytes = env[0]
    s = R.SUITES[0]
    import oracle as orc
    nmax = setup.max_ring_size
    base = [orc.from_seed(0, bytes([i % 251, i // 251]) + bytes(30)) for i in range(4)]
    pks = [base[i % 4][1] for i in range(nmax)]
    pkl = [xy(0, p) for p in pks]
    key = setup.index(pkl)
    prm = R.Params(s, ring_size=8)
    srs = R.Srs(s, srs_bytes)
    cols = R.index(prm, srs, [R.te_decode(s, p) for p in pks])
    assert key.commitment == R.commitment_bytes(s, cols)
    ones = (1 << 253) - 1
    cases = [(0, ones), (nmax - 1, ones), (nmax - 1, 0), (0, 1 << 252), (7, 0x5555555555555555555555555555555555555555555555555555555555555555 >> 3)]
    got = key.prove([c[0] for c in cases], [c[1].to_bytes(32, "little") for c in cases])
    for (k, b), proof in zip(cases, got):
        want, _ = R.prove(prm, srs, cols, k, b)
        assert proof == want, (k, hex(b))


@pytest.mark.parametrize("suite", [0, 1])
def test_srs_generate(env, suite):
    """a13, RingSetup::from_seed / from_rand -> Kzg::setup (src/ring.rs:359-374) with an explicit trapdoor: the generated
    URS has powers tau^i g1 (checked against the oracle's G1 scalar multiplication and, by pairing, against tau g2),
    loads like a file, and a ring proof made over it verifies -- on the GPU (both suites) and under the oracle (BLS)."""
    import oracle as orc
    from oracle import pairing_py as PP
    from ark_vrf_amd.ring import RingSetup, ring_batch_verify, srs_generate
    ctx, _, vs, srs_bytes = env[suite]
    s = R.SUITES[suite]
    fq = s.fp_bytes
    tau = int.from_bytes(b"\x42" * 31 + b"\x05", "little") % s.r
    g1 = srs_bytes[8: 8 + 2 * fq]
    cnt = int.from_bytes(srs_bytes[:8], "little")
    g2 = srs_bytes[8 + cnt * 2 * fq + 8: 8 + cnt * 2 * fq + 8 + 4 * fq]
    gen = srs_generate(ctx, suite, tau, g1, g2, 8)
    srs = R.Srs(s, gen)
    assert len(srs.g1) == 3 * 512 + 1 and len(srs.g2_raw) == 2 and srs.g2_raw[0] == g2
    p = s.p
    G = srs.g1[0] + (1,)
    for i in (1, 2, 7, 1536):
        assert srs.g1[i] == R.g1_affine(p, R.g1_mul(p, G, pow(tau, i, s.r)))
    PP.use_curve("bls12_381" if suite == 0 else "bn254")
    dec = PP.g2_decode_zcash_uncompressed if suite == 0 else PP.g2_decode_arkworks_uncompressed
    neg = lambda P: (P[0], (-P[1]) % p)
    assert PP.pairing_product_is_one([(srs.g1[1], dec(srs.g2_raw[0])), (neg(srs.g1[0]), dec(srs.g2_raw[1]))])
    PP.use_curve("bls12_381")
    setup = RingSetup(ctx, gen, 8)
    sks = [orc.from_seed(suite, bytes([7, i]) + bytes(30)) for i in range(5)]
    key = setup.index([xy(suite, pk) for _, pk in sks])
    h = orc.hash_to_curve(suite, b"generated-srs")
    sk, pk = sks[4]
    ped, blinding = orc.pedersen_prove(suite, sk, [(h, orc.vrf_output(suite, sk, h))], b"")
    proof = key.prove([4], [blinding])[0]
    yb = xy(suite, ped[:32])
    assert ring_batch_verify(setup, [key.commitment], None, [yb], [proof]) == 0
    assert ring_batch_verify(setup, [key.commitment], None, [xy(suite, pk)], [proof]) == 1
    if suite == 0:
        prm = R.Params(s, ring_size=8)
        fixed = [R.g1_decode_compressed(s, key.commitment[48 * i: 48 * i + 48]) for i in range(3)]
        assert R.verify(prm, srs, fixed, proof, R.te_decode(s, ped[:32]))
    with pytest.raises(Exception):
        srs_generate(ctx, suite, s.r, g1, g2, 8)                           # tau must be < r


@pytest.mark.parametrize("suite", [0, 1])
def test_setup_from_seed(env, suite):
    """a13, RingSetup::from_seed (src/ring.rs:359-366) as the reference derives it: Transcript::new(SUITE_ID) | seed -> to_rng ->
    Kzg::setup (tau = Fr::rand, g1 = G1::rand, g2 = G2::rand).  UNPINNED by any reference vector: the device-side
    derivation equals the oracle's independent restatement (oracle/ring_py.py srs_from_seed) byte for byte on both pairing curves,
    a different seed gives a different SRS, the same seed the same, and a ring proof made over the seeded setup verifies."""
    import oracle as orc
    from ark_vrf_amd.ring import RingSetup, ring_batch_verify
    ctx, _, vs, _ = env[suite]
    s = R.SUITES[suite]
    seed = bytes([suite + 1]) + bytes(range(31))
    setup = RingSetup.from_seed(ctx, 8, seed)
    got = setup.serialize(compress=False)
    want = R.srs_from_seed(s, 8, seed, n_g1=40)                            # the first 40 powers of the oracle (Python G1 arithmetic)
    fq = s.fp_bytes
    n_g1 = int.from_bytes(got[:8], "little")
    assert n_g1 == 3 * 512 + 1 and got[8: 8 + 40 * 2 * fq] == want[8: 8 + 40 * 2 * fq]
    assert got[8 + n_g1 * 2 * fq:] == want[8 + 40 * 2 * fq:]              # count 2 | g2 | tau g2
    tau, g1, g2 = R.srs_params_from_seed(s, seed)
    srs = R.Srs(s, got)
    assert srs.g1[1536] == R.g1_affine(s.p, R.g1_mul(s.p, g1 + (1,), pow(tau, 1536, s.r)))
    again = RingSetup.from_seed(ctx, 8, seed)
    assert again.serialize(compress=False) == got
    other = RingSetup.from_seed(ctx, 8, bytes(32))
    assert other.serialize(compress=False)[:8 + 2 * fq] != got[:8 + 2 * fq]
    again.close(); other.close()
    sks = [orc.from_seed(suite, bytes([9, i]) + bytes(30)) for i in range(4)]
    key = setup.index([xy(suite, pk) for _, pk in sks])
    h = orc.hash_to_curve(suite, b"seeded-setup")
    sk, pk = sks[2]
    ped, blinding = orc.pedersen_prove(suite, sk, [(h, orc.vrf_output(suite, sk, h))], b"")
    proof = key.prove([2], [blinding])[0]
    assert ring_batch_verify(setup, [key.commitment], None, [xy(suite, ped[:32])], [proof]) == 0
    key.close(); setup.close()


@pytest.mark.parametrize("suite", [0, 1])
def test_setup_serialisation(env, suite):
    """CanonicalSerialize / Deserialize of RingSetup and RingBuilderPcsParams (src/ring.rs:484-542) in both ark-serialize modes:
    uncompressed == the truncated SRS file; compressed == the oracle's encodings of the same points (G1 form pinned by the
    `ring_pks_com` vectors); either form loads into a setup that reproduces the reference's ring commitment and proof."""
    from oracle import pairing_py as PP
    from ark_vrf_amd.ring import RingSetup
    ctx, setup, vs, srs_bytes = env[suite]
    s = R.SUITES[suite]
    fq = s.fp_bytes
    n = 3 * 512 + 1
    cnt = int.from_bytes(srs_bytes[:8], "little")
    g2off = 8 + cnt * 2 * fq + 8
    unc = setup.serialize(False)
    assert unc == n.to_bytes(8, "little") + srs_bytes[8: 8 + n * 2 * fq] + (2).to_bytes(8, "little") + srs_bytes[g2off: g2off + 8 * fq]
    srs = R.Srs(s, srs_bytes)
    PP.use_curve("bls12_381" if suite == 0 else "bn254")
    try:
        dec = PP.g2_decode_zcash_uncompressed if suite == 0 else PP.g2_decode_arkworks_uncompressed
        g2c = b"".join(PP.g2_encode_compressed(dec(srs.g2_raw[i]), suite == 0) for i in range(2))
    finally:
        PP.use_curve("bls12_381")
    want_c = n.to_bytes(8, "little") + b"".join(R.g1_encode(s, P, True) for P in srs.g1[:n]) + (2).to_bytes(8, "little") + g2c
    comp = setup.serialize(True)
    assert comp == want_c
    v = vs[0]
    raw = bytes.fromhex(v["ring_pks"])
    pks = [xy(suite, raw[32 * i: 32 * i + 32]) for i in range(len(raw) // 32)]
    idx = [raw[32 * i: 32 * i + 32].hex() for i in range(len(pks))].index(v["pk"])
    for blob in (unc, comp):
        su2 = RingSetup(ctx, blob, 8)
        assert su2.serialize(False) == unc
        key = su2.index(pks)
        assert key.commitment.hex() == v["ring_pks_com"]
        assert key.prove([idx], [bytes.fromhex(v["blinding"])])[0].hex() == v["ring_proof"]
        key.close(); su2.close()
    from ark_vrf_amd import _native as nat
    x = srs.g1[0][0]
    while R.sqrt_mod((x ** 3 + s.g1_b) % s.p, s.p) is not None:                     # an x with no point on the curve
        x += 1
    enc = bytearray(R.g1_encode(s, (x, 0), True))
    bad = comp[:8] + bytes(enc) + comp[8 + fq:]
    with pytest.raises(nat.AvrfError, match="-> 2"):
        RingSetup(ctx, bad, 8)
    # RingBuilderPcsParams: the SRS in Lagrangian form, L_i(tau) g1 = commit(iNTT(e_i))
    N = 512
    lag = setup.builder_params(False)
    assert len(lag) == 8 + N * 2 * fq and int.from_bytes(lag[:8], "little") == N
    pts = [R.g1_decode_uncompressed(s, lag[8 + 2 * fq * i: 8 + 2 * fq * (i + 1)]) for i in range(N)]
    prm = R.Params(s, ring_size=8)
    for i in (0, 1, 300, 511):
        e = [0] * N; e[i] = 1
        assert pts[i] == R.g1_affine(s.p, R.g1_msm(s.p, srs.g1[:N], R.ifft(s, e, prm.w)))
    acc = None
    for P in pts:
        acc = R.g1_add(s.p, acc, P + (1,))
    assert R.g1_affine(s.p, acc) == srs.g1[0]                                       # sum_i L_i = 1
    lc = setup.builder_params(True)
    assert lc == N.to_bytes(8, "little") + b"".join(R.g1_encode(s, P, True) for P in pts)


@pytest.mark.parametrize("suite", [0, 1])
def test_verifier_only_setup(env, suite):
    """verifier_key_from_commitment with independently distributed PcsVerifierParams (src/ring.rs:435,466-482): a setup built
    from the serialised (g1, g2, tau g2) alone verifies exactly like the full one and refuses everything that needs the SRS."""
    from ark_vrf_amd import _native as nat
    from ark_vrf_amd.ring import RingSetup, VerifierKeyBuilder, ring_batch_verify, ring_verify_each
    ctx, setup, vs, srs = env[suite]
    s = R.SUITES[suite]
    fq = 48 if suite == 0 else 32
    coms = [bytes.fromhex(v["ring_pks_com"]) for v in vs]
    insts = [xy(suite, bytes.fromhex(v["proof_pk_com"])) for v in vs]
    proofs = [bytes.fromhex(v["ring_proof"]) for v in vs]
    raw, comp = setup.pcs_verifier_params(False), setup.pcs_verifier_params(True)
    assert (len(raw), len(comp)) == (2 * fq + 2 * 4 * fq, fq + 2 * 2 * fq)
    n1 = int.from_bytes(srs[:8], "little")
    assert raw == srs[8: 8 + 2 * fq] + srs[8 + n1 * 2 * fq + 8:]                    # powers_in_g1[0] || powers_in_g2[0..2] of the file
    for blob in (raw, comp):
        vo = RingSetup(ctx, blob, 8, verifier_only=True)
        assert (vo.domain_size, vo.max_ring_size, vo.proof_len) == (setup.domain_size, setup.max_ring_size, setup.proof_len)
        assert vo.pcs_verifier_params(True) == comp
        assert ring_batch_verify(vo, coms, list(range(7)), insts, proofs) == 0
        assert ring_verify_each(vo, coms, list(range(7)), insts, proofs) == [0] * 7
        bad = list(proofs); b = bytearray(bad[3]); b[4 * fq + 9] ^= 2; bad[3] = bytes(b)
        assert ring_batch_verify(vo, coms, list(range(7)), insts, bad) == 1
        assert ring_verify_each(vo, coms, list(range(7)), insts, bad) == [0, 0, 0, 1, 0, 0, 0]
        big = 20
        assert ring_verify_each(vo, coms, list(range(7)) * big, insts * big, proofs * big) == [0] * (7 * big)   # device decompression path
        pk = xy(suite, bytes.fromhex(vs[0]["pk"]))
        for call in (lambda: vo.index([pk]), lambda: VerifierKeyBuilder(vo), lambda: vo.serialize(), lambda: vo.builder_params()):
            with pytest.raises(nat.AvrfError, match="-> 4"):                      # SrsLookupFailed
                call()
        vo.close()
    with pytest.raises(nat.AvrfError, match="-> 2"):
        RingSetup(ctx, raw[:-1], 8, verifier_only=True)
    flipped = bytearray(comp); flipped[1] ^= 1                                    # another x: off the curve or outside the subgroup
    try:
        RingSetup(ctx, bytes(flipped), 8, verifier_only=True).close()
        ok = suite == 1                                                           # BN254 G1 has cofactor 1: every curve point is valid
    except nat.AvrfError:
        ok = True
    assert ok


@pytest.mark.parametrize("suite", [0, 1])
def test_verifier_key_builder(env, suite):
    """VerifierKeyBuilder (src/ring.rs:539-637; reference test `verifier_key_builder`, src/ring.rs:1224-1290): keys appended
    in batches give the commitment of `verifier_key(keys)` -- here the reference vector's `ring_pks_com` and
    avrf_ring_index's -- at every stage; capacity is enforced and a failed append changes nothing."""
    from ark_vrf_amd.ring import VerifierKeyBuilder
    ctx, setup, vs, srs = env[suite]
    v = vs[0]
    raw = bytes.fromhex(v["ring_pks"])
    pks = [xy(suite, raw[32 * i: 32 * i + 32]) for i in range(len(raw) // 32)]
    b = VerifierKeyBuilder(setup)
    assert b.free_slots() == setup.max_ring_size
    assert b.finalize() == setup.index([]).commitment                     # empty ring = all padding
    assert b.append(pks[:3]) == 0 and b.free_slots() == setup.max_ring_size - 3
    assert b.finalize() == setup.index(pks[:3]).commitment
    assert b.append([]) == 0
    assert b.append(pks[3:]) == 0
    assert b.finalize().hex() == v["ring_pks_com"]
    assert b.append(pks * 64) == 3                                         # does not fit: nothing appended
    assert b.finalize().hex() == v["ring_pks_com"]
    fill = [pks[i % len(pks)] for i in range(b.free_slots())]
    assert b.append(fill) == 0 and b.free_slots() == 0
    assert b.finalize() == setup.index(pks + fill).commitment
    assert b.append(pks[:1]) == 3
    bad = bytes([0xff] * 32) + pks[0][32:]
    b2 = VerifierKeyBuilder(setup)
    assert b2.append([bad]) == 2 and b2.free_slots() == setup.max_ring_size


def test_chunked_two_lane_proving(env, monkeypatch):
    """avrf_ring_prove splits a call into lockstep chunks and keeps two of them in flight (second lane: own stream,
    scratch and MSM workspace over the shared SRS tables): the proofs do not depend on the chunking."""
    import oracle as orc
    ctx, setup, vs, srs_bytes = env[0]
    sks = [orc.from_seed(0, bytes([3, i]) + bytes(30)) for i in range(6)]
    key = setup.index([xy(0, pk) for _, pk in sks])
    n = 11
    idx = [(5 * j + 1) % 6 for j in range(n)]
    bl = [(int.from_bytes(bytes([j + 1]) * 32, "little") >> 4).to_bytes(32, "little") for j in range(n)]
    whole = key.prove(idx, bl)
    monkeypatch.setenv("AVRF_RING_CHUNK", "2")
    assert key.prove(idx, bl) == whole                                     # 6 chunks over two lanes
    monkeypatch.setenv("AVRF_RING_LANES", "1")
    assert key.prove(idx, bl) == whole
    monkeypatch.setenv("AVRF_RING_CHUNK", "3")
    monkeypatch.delenv("AVRF_RING_LANES")
    assert key.prove(idx, bl) == whole
    assert [key.prove([i], [b])[0] for i, b in zip(idx[:3], bl[:3])] == whole[:3]


def test_c4_shape_1030_proofs_in_one_call(env, golden_dir):
    """BASELINE configs[3] as it is BENCHMARKED: ring 1024 (N = 2048), many proofs in ONE avrf_ring_prove call -- default
    chunking (lockstep chunks of 512 proofs on two lanes, a 6-proof remainder), mixed key indices with repeats, per-proof
    blindings (src/ring.rs:211-226).  Eleven sampled proofs (first / last of every chunk and of the remainder, some inside)
    equal the pure-Python oracle's byte for byte (tests/golden/ring_c4_oracle.json, made by gen_ring_c4_oracle.py); all 1 030
    verify as one batch, and a swapped pair of instances is rejected."""
    import hashlib
    import oracle as orc
    from ark_vrf_amd.ring import RingSetup, ring_batch_verify
    ctx, _, _, srs_bytes = env[0]
    s = R.SUITES[0]
    fx = json.load(open(os.path.join(golden_dir, "ring_c4_oracle.json")))
    ring, n = fx["ring_size"], fx["n_proofs"]
    assert (ring, n) == (1024, 1030)

    def key_index(j):
        return (0, 1, 777, 1023)[j] if j < 4 else (777 if j % 97 == 0 else (j * 389 + 7) % ring)
    setup = RingSetup(ctx, srs_bytes, ring)
    ks = b"".join((int.from_bytes(hashlib.sha512(b"k%d" % i).digest(), "little") % (s.r >> 3) + 1).to_bytes(32, "little") for i in range(ring))
    pks_xy = ctx.scalar_mul_base(ks)
    pkl = [pks_xy[64 * i: 64 * i + 64] for i in range(ring)]
    key = setup.index(pkl)
    assert key.commitment.hex() == fx["commitment"]
    idx = [key_index(j) for j in range(n)]
    assert all(fx["key_index"][str(j)] == idx[j] for j in map(int, fx["proofs"]))
    bl = [(int.from_bytes(hashlib.sha512(b"c4-blinding%d" % j).digest(), "little") % (s.r >> 3)).to_bytes(32, "little") for j in range(n)]
    proofs = key.prove(idx, bl)                                            # ONE call, default chunk size and lanes
    assert len(proofs) == n
    for j, hx in fx["proofs"].items():
        assert proofs[int(j)].hex() == hx, f"proof {j} (key {idx[int(j)]}) differs from the oracle's"
    # instances pk + b B (pedersen::Proof::key_commitment, src/pedersen.rs:64-70): one 2-term msm_unchecked each
    st, bb = orc.point_decompress(0, orc.suite_point(0, 1))
    assert st == 0 and (int.from_bytes(bb[:32], "little"), int.from_bytes(bb[32:], "little")) == s.blinding_base
    one = (1).to_bytes(32, "little")
    inst = [ctx.msm(pkl[idx[j]] + bb, one + bl[j]) for j in range(n)]
    assert ring_batch_verify(setup, [key.commitment], None, inst, proofs) == 0
    inst[5], inst[6] = inst[6], inst[5]
    assert ring_batch_verify(setup, [key.commitment], None, inst, proofs) == 1
    key.close(); setup.close()
