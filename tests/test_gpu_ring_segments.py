"""GPU: avrf_ring_batch_verify_segments -- n_seg independent ring BatchVerifiers (src/ring.rs:682-735) over consecutive runs of the
items, their G1 sums as ONE segmented MSM chain, one 2-pairing check per segment -- on the reference's seven ring vectors (each with
its own ring), repeated.  status[v] must be what avrf_ring_batch_verify answers for segment v's items alone; a defect marks its own
segment and no other; InvalidData wins over VerificationFailure; refusals write nothing.  The two sums of a segment are compared BY
VALUE with oracle/ring_py.py (verifier_values + big-int G1 arithmetic) under randomisers from hashlib.shake_128 over the segment's
own statement.  Suites 0 (Bandersnatch / BLS12-381) and 1 (Baby-JubJub / BN254)."""
import ctypes as C
import hashlib
import json
import os
import struct

import pytest

from helpers import xy
from oracle import ring_py as R

pytestmark = pytest.mark.gpu
FILES = {0: ("bandersnatch_sha-512_ell2_ring.json", "bls12-381-srs-2-11-uncompressed-zcash.bin"),
         1: ("baby-jubjub_sha-512_tai_ring.json", "bn254-testing-2-9-uncompressed.bin")}
OK, FAIL, INVALID, ERR_BAD_ARG = 0, 1, 2, -2
# a BLS12-381 point on the curve and outside the prime-order subgroup (tests/test_gpu_ring.py checks that it is one)
OFF_X = 0x13c60d23238642ea126a1e48cc11d357c30d8b7628dbd25e63b229f1c4069545de11cc9dea959c212e9c82b1478c281d
OFF_Y = 0x173eb497b4648ea412daae1e11fa194e01a1d4bf7376e7bad3ef138322e23c3c5114b8a96c915d51db072395e4ad9649


class Env:
    def __init__(self, suite, golden_dir):
        from ark_vrf_amd import _native as nat
        from ark_vrf_amd.ring import RingSetup
        vec, srsf = FILES[suite]
        self.suite, self.s = suite, R.SUITES[suite]
        self.raw = open(os.path.join(golden_dir, srsf), "rb").read()
        self.ctx = nat.Context(suite)
        self.setup = RingSetup(self.ctx, self.raw, 8)
        self.vs = json.load(open(os.path.join(golden_dir, vec)))
        self.fq = self.s.fp_bytes
        self.coms = [bytes.fromhex(v["ring_pks_com"]) for v in self.vs]
        self.insts7 = [xy(suite, bytes.fromhex(v["proof_pk_com"])) for v in self.vs]
        self.proofs7 = [bytes.fromhex(v["ring_proof"]) for v in self.vs]
        self._slices = {}

    def items(self, n):
        """n items: vector i % 7 against its own ring"""
        return [i % 7 for i in range(n)], [self.insts7[i % 7] for i in range(n)], [self.proofs7[i % 7] for i in range(n)]

    # the defects, by what they do to a proof's bytes
    def flip_eval(self, p):
        b = bytearray(p); b[4 * self.fq + 5] ^= 1; return bytes(b)

    def big_scalar(self, p):                                             # lin_zw >= r
        b = bytearray(p); b[4 * self.fq + 7 * 32 + self.fq + 31] = 0xff; return bytes(b)

    def infinity_commitment(self, p):                                    # the canonical infinity as the proof's first commitment
        inf = (bytes([0xC0]) + bytes(47)) if self.suite == 0 else (bytes(31) + bytes([0x40]))
        return inf + p[self.fq:]


@pytest.fixture(scope="module")
def envs(golden_dir):
    return {i: Env(i, golden_dir) for i in (0, 1)}


def seg_statuses(e, rings, insts, proofs, segs):
    from ark_vrf_amd.ring import ring_batch_verify_segments
    return ring_batch_verify_segments(e.setup, e.coms, rings, insts, proofs, segs)


def slice_statuses(e, rings, insts, proofs, segs):
    """ring_batch_verify of every segment's items alone, with the same commitments table"""
    from ark_vrf_amd.ring import ring_batch_verify
    out, at = [], 0
    for c in segs:
        out.append(ring_batch_verify(e.setup, e.coms, rings[at: at + c], insts[at: at + c], proofs[at: at + c]))
        at += c
    return out


def expected(item_status, segs):
    """the precedence rule over known per-item defects: InvalidData wins, then VerificationFailure; an empty segment is Ok"""
    out, at = [], 0
    for c in segs:
        st = item_status[at: at + c]
        out.append(INVALID if INVALID in st else FAIL if FAIL in st else OK)
        at += c
    return out


SEGMENTATIONS = [[21], [7, 7, 7], [1] * 21, [0, 1, 0, 13, 7, 0], [2, 19]]


@pytest.mark.parametrize("suite", [0, 1])
@pytest.mark.parametrize("segs", SEGMENTATIONS, ids=lambda s: "x".join(map(str, s)) if len(s) < 8 else "%dx1" % len(s))
def test_valid_proofs(envs, suite, segs):
    e = envs[suite]
    rings, insts, proofs = e.items(21)
    got = seg_statuses(e, rings, insts, proofs, segs)
    assert got == [OK] * len(segs)
    assert got == slice_statuses(e, rings, insts, proofs, segs)


@pytest.mark.parametrize("suite", [0, 1])
def test_defects_mark_their_segment(envs, suite):
    from ark_vrf_amd.ring import ring_verify_each
    e = envs[suite]
    rings, insts, proofs = e.items(21)
    cases = []                                                           # (rings, insts, proofs, per-item status)

    def one(item, status, proof=None, ring=None):
        r, p, st = list(rings), list(proofs), [OK] * 21
        if proof is not None:
            p[item] = proof
        if ring is not None:
            r[item] = ring
        st[item] = status
        cases.append((r, insts, p, st))
    one(9, FAIL, proof=e.flip_eval(proofs[9]))                           # a flipped evaluation bit
    one(12, INVALID, proof=e.big_scalar(proofs[12]))                     # a scalar >= r
    one(17, FAIL, ring=(rings[17] + 1) % 7)                              # an item against the wrong ring
    cases.append((rings, insts[1:] + insts[:1], proofs, [FAIL] * 21))    # rotated instances: every item, so every segment touched
    one(5, FAIL, proof=e.infinity_commitment(proofs[5]))                 # decodes, fails the equation
    if suite == 0:
        off = R.g1_encode(e.s, (OFF_X, OFF_Y), True)
        one(4, INVALID, proof=off + proofs[4][48:])                      # outside the subgroup: a commitment slot of the proof
        one(20, INVALID, proof=proofs[20][:-48] + off)                   # and the last opening
    both = list(proofs); both[8] = e.flip_eval(proofs[8]); both[10] = e.big_scalar(proofs[10])
    st = [OK] * 21; st[8] = FAIL; st[10] = INVALID
    cases.append((rings, insts, both, st))                               # both kinds in one segment of [7, 7, 7]: 2
    for r, i, p, st in cases:
        for segs in ([7, 7, 7], [0, 1, 0, 13, 7, 0], [2, 19]):
            assert seg_statuses(e, r, i, p, segs) == expected(st, segs), (st, segs)
        each = ring_verify_each(e.setup, e.coms, r, i, p)
        assert each == st
        assert seg_statuses(e, r, i, p, [1] * 21) == each


@pytest.fixture(scope="module")
def large(envs):
    """140 items (device decompression) with the defects of test_ring_verify_large_batch_device_decompression at the same items, and
    the statuses of the same items verified seven at a time with ring_batch_verify -- computed once per suite"""
    cache = {}

    def get(suite):
        if suite in cache:
            return cache[suite]
        e = envs[suite]
        s, fq = e.s, e.fq
        rings, insts, proofs = e.items(140)
        x = 5
        while R.sqrt_mod((x * x * x + s.g1_b) % s.p, s.p) is not None:
            x += 1

        def enc_x(x, flags):
            if suite == 0:
                b = bytearray(x.to_bytes(48, "big")); b[0] |= flags; return bytes(b)
            b = bytearray(x.to_bytes(32, "little")); b[31] |= flags; return bytes(b)
        bad, st = list(proofs), [OK] * 140
        bad[9] = e.flip_eval(bad[9]); st[9] = FAIL
        bad[17] = enc_x(x, 0x80 if suite == 0 else 0) + bad[17][fq:]; st[17] = INVALID                  # not on the curve
        b = bytearray(bad[30]); b[0 if suite == 0 else fq - 1] ^= (0x20 if suite == 0 else 0x80); bad[30] = bytes(b); st[30] = FAIL   # -P
        bad[44] = e.infinity_commitment(bad[44]); st[44] = FAIL
        bad[51] = (bytes([0xC0]) + bytes(46) + b"\x01" if suite == 0 else b"\x01" + bytes(30) + bytes([0x40])) + bad[51][fq:]; st[51] = INVALID
        bad[66] = enc_x(s.p + 1, 0x80 if suite == 0 else 0) + bad[66][fq:]; st[66] = INVALID            # x >= p
        if suite == 0:
            bad[100] = bad[100][:-48] + R.g1_encode(s, (OFF_X, OFF_Y), True); st[100] = INVALID         # opening proof outside G1
        sevens = slice_statuses(e, rings, insts, bad, [7] * 20)
        assert sevens == expected(st, [7] * 20)                          # (no slice of seven holds both kinds: ring_batch_verify is deterministic on each)
        cache[suite] = (rings, insts, bad, sevens)
        return cache[suite]
    return get


@pytest.mark.parametrize("suite", [0, 1])
@pytest.mark.parametrize("segs", [[7] * 20, [128, 12]], ids=["20x7-device-pairings", "128+12-host-pairings"])
def test_device_decompression(envs, large, suite, segs):
    e = envs[suite]
    rings, insts, bad, sevens = large(suite)
    want = []                                                            # a segment's status from its slices of seven, InvalidData first
    at = 0
    for c in segs:
        part = sevens[at // 7: -(-(at + c) // 7)]                        # the slices of seven that overlap the segment
        want.append(INVALID if INVALID in part else FAIL if FAIL in part else OK)
        at += c
    if segs == [128, 12]:
        assert want == [INVALID, OK]                                     # (items 126 .. 139 hold no defect, so the cut inside a slice of seven changes nothing)
    assert seg_statuses(e, rings, insts, bad, segs) == want


@pytest.mark.parametrize("suite", [0, 1])
def test_rounds(envs, suite):
    """600 one-item segments: 2 * 600 * windows(11) exceeds MSM_SEG_WINDOWS_MAX, so the call runs two chains; one defect lies in the
    last round"""
    from ark_vrf_amd.ring import ring_segments_layout
    e = envs[suite]
    lay = ring_segments_layout(600, [1] * 600)
    assert lay[0] == 11 and lay[1] >= 2
    per_round = lay[2] // (2 * lay[0])
    rings, insts, proofs = e.items(600)
    st = [OK] * 600
    proofs[10] = e.flip_eval(proofs[10]); st[10] = FAIL
    proofs[300] = e.big_scalar(proofs[300]); st[300] = INVALID
    assert 599 >= per_round
    rings[599] = (rings[599] + 2) % 7; st[599] = FAIL                    # (+ 2: vectors 4 and 5 share one ring, and item 599 is vector 4)
    assert e.coms[rings[599]] != e.coms[599 % 7]
    assert seg_statuses(e, rings, insts, proofs, [1] * 600) == st


def le(s, P):
    n = s.fp_bytes
    return bytes(2 * n) if P is None else P[0].to_bytes(n, "little") + P[1].to_bytes(n, "little")


@pytest.mark.parametrize("suite", [0, 1])
def test_sums_by_value(envs, suite):
    """A = sum [r1 (C_agg - v_agg g1 + zeta pi1) + r2 (C_lin - lin_zw g1 + zeta w pi2)], B = -sum (r1 pi1 + r2 pi2) over a segment's
    items, (r1, r2) the two 128-bit halves of the item's 32 SHAKE128 bytes over the SEGMENT's statement (its item count in the header;
    the byte order of tests/test_host_ring_values.py), r1 = 1 in a one-item segment."""
    from ark_vrf_amd.ring import ring_segment_sums
    e = envs[suite]
    s, n, r, p = e.s, e.fq, e.s.r, e.s.p
    srs = R.Srs(s, e.raw)
    prm = R.Params(s, ring_size=8)
    rings, insts, proofs = e.items(7)
    segs = [1, 2, 4]
    assert seg_statuses(e, rings, insts, proofs, segs) == [OK] * 3
    g1 = srs.g1[0]
    key = g1[0].to_bytes(n, "little") + g1[1].to_bytes(n, "little") + srs.g2_raw[0] + srs.g2_raw[1]
    neg = lambda P: (P[0], (-P[1]) % p)
    at = 0
    for v, cnt in enumerate(segs):
        msg = b"avrf-ring-batch" + struct.pack("<3Q", cnt, 7, prm.N) + key + b"".join(struct.pack("<I", i) for i in rings[at: at + cnt])
        msg += b"".join(e.coms) + b"".join(insts[at: at + cnt]) + b"".join(proofs[at: at + cnt])
        rnd = hashlib.shake_128(msg).digest(32 * cnt)
        pts_a, ks_a, pts_b, ks_b = [], [], [], []
        for j in range(cnt):
            it = at + j
            r1, r2 = int.from_bytes(rnd[32 * j: 32 * j + 16], "little"), int.from_bytes(rnd[32 * j + 16: 32 * j + 32], "little")
            if cnt == 1:
                r1 = 1
            fixed = [R.g1_decode_compressed(s, e.coms[rings[it]][n * k: n * k + n]) for k in range(3)]
            inst = (int.from_bytes(insts[it][:32], "little"), int.from_bytes(insts[it][32:], "little"))
            val = R.verifier_values(prm, srs, fixed, proofs[it], inst)
            Cs, nus, al, nl = val["C"], val["nus"], val["alphas"], val["nl"]
            zeta, zw = val["zeta"], val["zeta"] * prm.w % r
            for nu, Pt in zip(nus, fixed + Cs + [val["Cq"]]):                                          # r1 C_agg
                pts_a.append(Pt); ks_a.append(r1 * nu % r)
            for k, Pt in ((nl * al[0], Cs[1]), (nl * al[1] * val["k1"], Cs[2]), (nl * al[2] * val["k2"], Cs[3])):   # r2 C_lin
                pts_a.append(Pt); ks_a.append(r2 * k % r)
            pts_a += [g1, val["pi1"], val["pi2"]]
            ks_a += [-(r1 * val["v_agg"] + r2 * val["lin_zw"]) % r, r1 * zeta % r, r2 * zw % r]
            pts_b += [neg(val["pi1"]), neg(val["pi2"])]; ks_b += [r1, r2]
        a, b = ring_segment_sums(e.setup, v)
        assert a == le(s, R.g1_affine(p, R.g1_msm(p, pts_a, ks_a))), v
        assert b == le(s, R.g1_affine(p, R.g1_msm(p, pts_b, ks_b))), v
        at += cnt
    from ark_vrf_amd import _native as nat
    with pytest.raises(nat.AvrfError):
        ring_segment_sums(e.setup, 3)


@pytest.mark.parametrize("suite", [0, 1])
def test_refusals_write_nothing(envs, suite):
    from ark_vrf_amd.ring import ring_batch_verify, ring_batch_verify_segments, ring_segment_sums, ring_verify_each
    from ark_vrf_amd import _native as nat
    e = envs[suite]
    rings, insts, proofs = e.items(21)
    before = (ring_batch_verify(e.setup, e.coms, rings, insts, proofs), ring_verify_each(e.setup, e.coms, rings, insts, proofs))
    assert before == (OK, [OK] * 21)
    SENT = 0x5a5a5a5a

    def refused(coms, rr, ii, pp, segs, want):
        buf = (C.c_int32 * (len(segs) + 1))(*([SENT] * (len(segs) + 1)))
        assert ring_batch_verify_segments(e.setup, coms, rr, ii, pp, segs, status_buf=buf) == want
        assert list(buf) == [SENT] * (len(segs) + 1)
    refused(e.coms, rings, insts, proofs, [7, 7, 8], ERR_BAD_ARG)        # counts summing to n + 1
    refused(e.coms, rings, insts, proofs, [7, 7, 6], ERR_BAD_ARG)        # and to n - 1
    wrong = list(rings); wrong[20] = 7
    refused(e.coms, wrong, insts, proofs, [7, 7, 7], ERR_BAD_ARG)        # a ring index = n_rings
    refused(e.coms, None, [b""] * 820, [b""] * 820, [820], ERR_BAD_ARG)  # a segment of 820 items: refused before a byte of them is read
    junk = bytearray(e.coms[3]); junk[1: e.fq] = b"\x7f" * (e.fq - 1)
    refused(e.coms[:3] + [bytes(junk)] + e.coms[4:], rings, insts, proofs, [7, 7, 7], INVALID)          # a commitment that does not decode
    if suite == 0:
        off = R.g1_encode(e.s, (OFF_X, OFF_Y), True)
        refused([off + e.coms[0][48:]] + e.coms[1:], rings, insts, proofs, [7, 7, 7], INVALID)           # or lies outside the subgroup
    with pytest.raises(nat.AvrfError):
        ring_segment_sums(e.setup, 0)                                    # no sums after a call that failed
    assert (ring_batch_verify(e.setup, e.coms, rings, insts, proofs), ring_verify_each(e.setup, e.coms, rings, insts, proofs)) == before
    assert ring_batch_verify_segments(e.setup, e.coms, rings, insts, proofs, [7, 7, 7]) == [OK] * 3
    assert ring_batch_verify_segments(e.setup, e.coms, [], [], [], [0, 0]) == [OK, OK]
    assert ring_batch_verify_segments(e.setup, e.coms, [], [], [], []) == []


@pytest.mark.parametrize("suite", [0, 1])
def test_ring_vrf_segments(envs, suite):
    """complete ring-VRF proofs (Pedersen proof || ring proof, built as tests/test_gpu_wire.py builds them) over [3, 4]: the Pedersen
    half segmented on the context, the ring half on the setup"""
    from ark_vrf_amd import _native as nat
    from ark_vrf_amd.ring import ring_vrf_verify_segments
    e = envs[suite]
    L, rlen = nat.lib(), e.setup.proof_len
    proofs, ios, ads = [], [], []
    for v in e.vs:
        raw = bytes.fromhex(v["ring_pks"])
        pks = [xy(suite, raw[32 * i: 32 * i + 32]) for i in range(len(raw) // 32)]
        key = e.setup.index(pks)
        idx = [raw[32 * i: 32 * i + 32].hex() for i in range(len(pks))].index(v["pk"])
        io_xy = xy(suite, bytes.fromhex(v["h"])) + xy(suite, bytes.fromhex(v["gamma"]))
        ad = bytes.fromhex(v["ad"])
        out = (C.c_uint8 * (160 + rlen))()
        assert L.avrf_ring_vrf_prove(e.ctx._h, key._h, C.c_size_t(rlen), C.c_size_t(1), nat._u8(bytes.fromhex(v["sk"])), nat._u32([idx]), nat._u8(io_xy),
                                     nat._u32([1]), nat._u8(ad), nat._u32([len(ad)]), 0, out) == 0
        assert bytes(out)[160:] == bytes.fromhex(v["ring_proof"])
        proofs.append(bytes(out)); ios.append(bytes.fromhex(v["h"]) + bytes.fromhex(v["gamma"])); ads.append(ad)
        key.close()
    rings = list(range(7))
    verify = lambda prs, validate, ctx=e.ctx: ring_vrf_verify_segments(ctx, e.setup, e.coms, rings, ios, [1] * 7, ads, prs, [3, 4], validate)
    flip = lambda p, at: p[:at] + bytes([p[at] ^ 1]) + p[at + 1:]
    ped = list(proofs); ped[1] = flip(ped[1], 100)                       # the Pedersen response s of an item of segment 0
    rng = list(proofs); rng[5] = flip(rng[5], 160 + 4 * e.fq + 5)         # a ring evaluation of an item of segment 1
    both = list(ped); both[5] = rng[5]
    for validate in (0, 1):
        assert verify(proofs, validate) == [OK, OK]
        assert verify(ped, validate) == [FAIL, OK]
        assert verify(rng, validate) == [OK, FAIL]
        assert verify(both, validate) == [FAIL, FAIL]
    other = nat.Context(1 - suite)
    assert verify(proofs, 1, ctx=other) == ERR_BAD_ARG
    other.close()
