"""GPU parity: thin::BatchVerifier over a table of shared points (include/avrf.h avrf_thin_batch_stage_shared) vs the oracle.

The expectation for a shared batch is always derived from the oracle on the EXPANDED batch (every index replaced by its row):
orc.thin_batch_terms_xy gives the terms of src/thin.rs:282-317 in the order R, pk, (O_i, I_i).., G; `fold` re-lays them into the
shared layout -- (R_j, w_j) at j + io0, (O_ji, w c z_i) behind it, row r at n + tot_io + r, (G, g) last -- and adds the key / input
scalars of every row with Python integers modulo the suite's group order.  Everything is compared bit for bit.

Term comparisons need no verifying proofs (the verdict is then 1, the terms are built all the same), so the index distributions
take their points, response scalars and additional data from one synthetic batch of the oracle."""
import ctypes as C
import json
import os
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import oracle as orc
from helpers import IDENTITY_XY, R_ORDER, nat_batch, xy

pytestmark = pytest.mark.gpu

NAMES = {0: "bandersnatch_sha-512_ell2", 1: "baby-jubjub_sha-512_tai"}
Q0 = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001        # base field of suite 0


@pytest.fixture(scope="module")
def ctxs():
    from ark_vrf_amd import _native as nat
    made = {}

    class Lazy(dict):
        def __missing__(self, suite):
            made[suite] = self[suite] = nat.Context(suite)
            return self[suite]
    yield Lazy()
    for c in made.values():
        c.close()


# ---- a shared batch as a dict: rows (list of 64-byte points), pk_index, input_index, outputs (list), io_counts, ads (list), proofs (list of 96 bytes)

def shared(rows, pk_index, input_index, outputs, io_counts, ads, proofs):
    assert len(pk_index) == len(io_counts) == len(ads) == len(proofs) and len(input_index) == len(outputs) == sum(io_counts)
    return dict(n=len(pk_index), rows=list(rows), pk_index=list(pk_index), input_index=list(input_index), outputs=list(outputs),
                io_counts=list(io_counts), ads=list(ads), proofs=list(proofs))


def nat_shared(sb):
    from ark_vrf_amd._native import SharedBatch
    return SharedBatch(sb["n"], b"".join(sb["rows"]), sb["pk_index"], sb["input_index"], b"".join(sb["outputs"]), sb["io_counts"],
                       b"".join(sb["ads"]), [len(a) for a in sb["ads"]], b"".join(sb["proofs"]))


def expanded(sb):
    """the plain batch a shared one stands for, in the C-ABI layout (a gen_batch-style dict)"""
    rows = sb["rows"]
    return dict(n=sb["n"], pks_xy=b"".join(rows[r] for r in sb["pk_index"]),
                ios_xy=b"".join(rows[r] + o for r, o in zip(sb["input_index"], sb["outputs"])), io_counts=sb["io_counts"],
                ads=b"".join(sb["ads"]), ad_lens=[len(a) for a in sb["ads"]], proofs=b"".join(sb["proofs"]), sks=b"")


def fold(suite, sb, bases, sc):
    """oracle terms of the expanded batch -> (bases, scalars) in the shared layout"""
    n, tot, rows, r_order = sb["n"], sum(sb["io_counts"]), sb["rows"], R_ORDER[suite]
    nt = n + tot + len(rows) + 1
    assert len(sc) == 32 * (2 * n + 2 * tot + 1)
    term = lambda k: (bases[64 * k: 64 * k + 64], sc[32 * k: 32 * k + 32])
    out = [None] * nt
    acc = [0] * len(rows)
    k = io0 = 0
    for j, m in enumerate(sb["io_counts"]):
        out[j + io0] = term(k)                                                    # (R_j, w_j)
        pb, ps = term(k + 1)                                                      # (pk_j, w c z0)
        assert pb == rows[sb["pk_index"][j]]
        acc[sb["pk_index"][j]] += int.from_bytes(ps, "little")
        for i in range(m):
            out[j + io0 + 1 + i] = term(k + 2 + 2 * i)                            # (O_i, w c z_i)
            ib, is_ = term(k + 3 + 2 * i)                                         # (I_i, -w s z_i)
            assert ib == rows[sb["input_index"][io0 + i]]
            acc[sb["input_index"][io0 + i]] += int.from_bytes(is_, "little")
        k += 2 + 2 * m; io0 += m
    for r, row in enumerate(rows):
        out[n + tot + r] = (row, (acc[r] % r_order).to_bytes(32, "little"))
    out[nt - 1] = term(k)                                                         # (G, g)
    return b"".join(t[0] for t in out), b"".join(t[1] for t in out)


def run_and_compare(c, suite, sb):
    """stage shared, run, compare all terms with the folded oracle terms; returns the verdict"""
    from ark_vrf_amd import _native as nat
    assert c.thin_batch_stage_shared(nat_shared(sb)) == 0
    st = c.thin_batch_run()
    st_o, bases, sc = orc.thin_batch_terms_xy(suite, expanded(sb))
    assert st_o == 0
    gb, gs = c.last_terms()
    assert len(gs) // 32 == nat.thin_shared_n_terms(sb["n"], sum(sb["io_counts"]), len(sb["rows"]))
    wb, ws = fold(suite, sb, bases, sc)
    assert gs == ws and gb == wb
    return st


def tampered(sb, j):
    pr = list(sb["proofs"])
    pr[j] = pr[j][:64] + bytes([pr[j][64] ^ 1]) + pr[j][65:]
    return dict(sb, proofs=pr)


def proof_abi(suite, comp):
    L = orc.pt_len(suite)
    return xy(suite, comp[:L]) + comp[L:]


_REAL = {}


def real_batch(suite, counts, n_keys, n_inputs, seed=1):
    """a VERIFYING batch of len(counts) items over n_keys keys and n_inputs inputs: proofs by the oracle's prover"""
    key = (suite, tuple(counts), n_keys, n_inputs, seed)
    if key in _REAL:
        return _REAL[key]
    rng = random.Random(seed)
    keys = [orc.from_seed(suite, bytes([k + 1, seed]) + bytes(30)) for k in range(n_keys)]
    inputs = [orc.hash_to_curve(suite, b"slot-%d" % i) for i in range(n_inputs)]
    outs = {}
    items = []
    for j, m in enumerate(counts):
        k = rng.randrange(n_keys)
        ii = [rng.randrange(n_inputs) for _ in range(m)]
        for i in ii:
            if (k, i) not in outs:
                outs[k, i] = orc.vrf_output(suite, keys[k][0], inputs[i])
        items.append((k, ii, b"ad-%d" % j * (j % 3)))
    with ThreadPoolExecutor(max_workers=8) as ex:
        proofs = list(ex.map(lambda it: orc.thin_prove(suite, keys[it[0]][0], [(inputs[i], outs[it[0], i]) for i in it[1]], it[2]), items))
    out_xy = {ki: xy(suite, o) for ki, o in outs.items()}
    rows = [xy(suite, pk) for _, pk in keys] + [xy(suite, h) for h in inputs]
    sb = shared(rows, [k for k, _, _ in items], [n_keys + i for _, ii, _ in items for i in ii],
                [out_xy[k, i] for k, ii, _ in items for i in ii], counts, [ad for _, _, ad in items], [proof_abi(suite, p) for p in proofs])
    _REAL[key] = sb
    return sb


def prefix(sb, n):
    tot = sum(sb["io_counts"][:n])
    return shared(sb["rows"], sb["pk_index"][:n], sb["input_index"][:tot], sb["outputs"][:tot], sb["io_counts"][:n], sb["ads"][:n], sb["proofs"][:n])


@pytest.fixture(scope="module")
def real3k():
    return real_batch(0, [1] * 3000, 3, 2)


# ---------------------------------------------------------------- reference vectors

@pytest.mark.parametrize("suite", [0, 1])
def test_reference_vectors_shared(ctxs, golden_dir, suite):
    with open(os.path.join(golden_dir, NAMES[suite] + "_thin.json")) as f:
        vs = json.load(f)
    rows = [xy(suite, bytes.fromhex(v["pk"])) for v in vs] + [xy(suite, bytes.fromhex(v["h"])) for v in vs]
    assert len(rows) == 14
    sb = shared(rows, range(7), range(7, 14), [xy(suite, bytes.fromhex(v["gamma"])) for v in vs], [1] * 7,
                [bytes.fromhex(v["ad"]) for v in vs], [proof_abi(suite, bytes.fromhex(v["proof_r"] + v["proof_s"])) for v in vs])
    c = ctxs[suite]
    assert run_and_compare(c, suite, sb) == 0
    bad = tampered(sb, 4)
    assert c.thin_batch_stage_shared(nat_shared(bad)) == 0 and c.thin_batch_run() == 1          # tampered s (src/thin.rs:320-322)
    assert c.thin_batch_stage_shared(nat_shared(dict(sb, ads=[b"x"] + sb["ads"][1:]))) == 0 and c.thin_batch_run() == 1   # wrong ad


# ---------------------------------------------------------------- verifying batches with real sharing

def partial_of(c, suite, n, proofs):
    """avrf_thin_batch_challenges, the true weight seed of the batch, avrf_thin_batch_partial from item 0 -> 64 bytes"""
    from ark_vrf_amd import _native as nat
    cs = (C.c_uint8 * (16 * n))()
    assert nat.lib().avrf_thin_batch_challenges(c._h, cs) == 0
    seed, out = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    assert nat.lib().avrf_batch_weight_seed(suite, 0, C.c_size_t(n), cs, nat._u8(b"".join(p[64:] for p in proofs)), seed) == 0
    assert nat.lib().avrf_thin_batch_partial(c._h, seed, C.c_uint64(0), out) == 0
    return bytes(out)


@pytest.mark.parametrize("n", [130, 3000])
def test_verifying_batches(ctxs, real3k, n):
    """K = 3 keys, M = 2 inputs: n = 130 is 266 terms (the single-launch MSM), n = 3 000 is 6 006 (Pippenger)"""
    c = ctxs[0]
    sb = prefix(real3k, n)
    assert run_and_compare(c, 0, sb) == 0
    assert len(c.last_terms()[1]) // 32 == 2 * n + 5 + 1
    bad = tampered(sb, n // 2)
    assert run_and_compare(c, 0, bad) == 1                                      # one tampered response anywhere
    # the same batch staged plainly: same verdicts; and under one seed the partial point of both stagings is orc.msm of the oracle's terms
    cases = [(sb, 0)] + ([(bad, 1)] if n == 130 else [])
    for b, verdict in cases:
        e = expanded(b)
        _, bases, sc = orc.thin_batch_terms_xy(0, e)
        want = orc.msm(0, bases, sc)
        assert (want == IDENTITY_XY) == (verdict == 0)
        assert c.thin_batch_stage(nat_batch(e)) == 0
        assert partial_of(c, 0, n, b["proofs"]) == want
        assert c.thin_batch_run() == verdict
        assert c.thin_batch_stage_shared(nat_shared(b)) == 0
        assert partial_of(c, 0, n, b["proofs"]) == want
        assert c.thin_batch_run() == verdict


def test_mixed_pair_counts(ctxs):
    """the shape of test_multi_io_items (0 .. 17 pairs per item) over K = 5 keys and M = 4 inputs"""
    sb = real_batch(0, [0, 1, 2, 3, 5, 1, 0, 2, 16, 17], 5, 4)
    assert run_and_compare(ctxs[0], 0, sb) == 0
    assert run_and_compare(ctxs[0], 0, tampered(sb, 8)) == 1


@pytest.mark.parametrize("suite", [1, 2, 3, 4, 5, 6, 7])
def test_other_suites(ctxs, suite):
    """suites 5 and 6 take their weights from the host's stream, suite 7 is the short-Weierstrass curve"""
    sb = real_batch(suite, [1] * 40, 3, 2)
    assert run_and_compare(ctxs[suite], suite, sb) == 0
    assert run_and_compare(ctxs[suite], suite, tampered(sb, 17)) == 1


# ---------------------------------------------------------------- index distributions, terms only

@pytest.fixture(scope="module")
def material():
    """3 000 keys + 3 000 inputs (6 000 distinct points), outputs, proofs (R, s < r) and additional data of one synthetic batch"""
    b = orc.gen_batch(0, 0, 3000)
    n = b["n"]
    pts = [b["pks_xy"][64 * j: 64 * j + 64] for j in range(n)] + [b["ios_xy"][128 * j: 128 * j + 64] for j in range(n)]
    assert len(set(pts)) == 2 * n and IDENTITY_XY not in pts
    outs = [b["ios_xy"][128 * j + 64: 128 * j + 128] for j in range(n)]
    ads, off = [], 0
    for ln in b["ad_lens"]:
        ads.append(b["ads"][off: off + ln]); off += ln
    return dict(pts=pts, outs=outs, ads=ads, proofs=[b["proofs"][96 * j: 96 * j + 96] for j in range(n)])


def distribution(kind, n, pts):
    """-> (rows, pk_index, input_index) for n items with one pair each"""
    rng = random.Random(n * 31 + len(kind))
    if kind == "one_row":                                                        # T = 1: every key and every input the same row
        return pts[:1], [0] * n, [0] * n
    if kind == "all_distinct_reversed":                                          # T = 2 n, indices in reversed order
        return pts[: 2 * n], [2 * n - 1 - j for j in range(n)], [n - 1 - j for j in range(n)]
    if kind == "skew":                                                           # one row takes 90 % of the references, 64 rows the rest
        pick = lambda: 17 if rng.random() < 0.9 else rng.choice([r for r in range(65) if r != 17])
        return pts[:65], [pick() for _ in range(n)], [pick() for _ in range(n)]
    if kind == "key_and_input":                                                  # rows used both as a key and as an input
        return pts[:3], [j % 3 for j in range(n)], [(j + 1) % 3 if j % 2 else j % 3 for j in range(n)]
    if kind == "unreferenced":                                                   # unreferenced rows at the start, in the middle, at the end
        used = [2, 3, 6]
        return pts[:9], [rng.choice(used) for _ in range(n)], [rng.choice(used) for _ in range(n)]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["one_row", "all_distinct_reversed", "skew", "key_and_input", "unreferenced"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 3000])
def test_index_distributions(ctxs, material, n, kind):
    rows, pk_index, input_index = distribution(kind, n, material["pts"])
    sb = shared(rows, pk_index, input_index, material["outs"][:n], [1] * n, material["ads"][:n], material["proofs"][:n])
    assert run_and_compare(ctxs[0], 0, sb) in (0, 1)                             # (the proofs belong to other keys: the terms are what is compared)
    if kind == "unreferenced":
        _, gs = ctxs[0].last_terms()
        for r in (0, 1, 4, 5, 7, 8):
            assert gs[32 * (2 * n + r): 32 * (2 * n + r + 1)] == bytes(32)


# ---------------------------------------------------------------- checks

def test_identity_rows(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 20, 3, 2)
    spare = dict(sb, rows=sb["rows"] + [IDENTITY_XY])                            # an identity point nothing refers to
    assert run_and_compare(c, 0, spare) == 0
    for j, into in [(3, "pk_index"), (7, "input_index")]:                        # ... and referred to, as a key / as an input
        idx = list(sb[into]); idx[j] = len(sb["rows"])
        assert c.thin_batch_stage_shared(nat_shared(dict(spare, **{into: idx}))) == 0
        assert c.thin_batch_run() == 2                                           # src/thin.rs:266-271
    outs = list(sb["outputs"]); outs[5] = IDENTITY_XY
    assert c.thin_batch_stage_shared(nat_shared(dict(sb, outputs=outs))) == 0 and c.thin_batch_run() == 2
    assert run_and_compare(c, 0, sb) == 0


def test_non_canonical_rows(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 20, 3, 2)
    row = sb["rows"][1]
    x = int.from_bytes(row[:32], "little")
    lifted = (x + Q0).to_bytes(32, "little") + row[32:]                          # the same x, not reduced
    assert x + Q0 < 1 << 256
    assert c.thin_batch_stage_shared(nat_shared(dict(sb, rows=sb["rows"] + [lifted]))) == 0 and c.thin_batch_run() == 2     # unreferenced
    assert c.thin_batch_stage_shared(nat_shared(dict(sb, rows=[sb["rows"][0], lifted] + sb["rows"][2:]))) == 0 and c.thin_batch_run() == 2
    assert c.thin_batch_stage_shared(nat_shared(dict(sb, rows=sb["rows"] + [Q0.to_bytes(32, "little") + row[32:]]))) == 0 and c.thin_batch_run() == 2
    assert run_and_compare(c, 0, sb) == 0                                        # (the flag does not outlive its staging)


def test_bad_index_is_refused(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 20, 3, 2)
    plain = nat_batch(expanded(sb))
    t = len(sb["rows"])
    assert c.thin_batch_stage(plain) == 0 and c.thin_batch_run() == 0
    for into, j in [("pk_index", 0), ("pk_index", 19), ("input_index", 11)]:
        idx = list(sb[into]); idx[j] = t
        assert c.thin_batch_stage_shared(nat_shared(dict(sb, **{into: idx}))) == -2
        assert c.thin_batch_run() == 0                                           # nothing was staged: the plain batch is still there
    idx = list(sb["pk_index"]); idx[4] = 0xffffffff
    assert c.thin_batch_stage_shared(nat_shared(dict(sb, pk_index=idx))) == -2
    assert c.thin_batch_stage_shared(nat_shared(dict(sb, rows=[], pk_index=[0] * 20, input_index=[0] * 20))) == -2         # n_shared == 0, n > 0
    e = expanded(sb)
    assert c.thin_batch_verify([e["pks_xy"][64 * j: 64 * j + 64] for j in range(20)],
                               [[(e["ios_xy"][128 * j: 128 * j + 64], e["ios_xy"][128 * j + 64: 128 * j + 128])] for j in range(20)],
                               sb["ads"], sb["proofs"]) == 0
    # the empty batch, with and without a table
    assert c.thin_batch_stage_shared(nat_shared(shared(sb["rows"], [], [], [], [], [], []))) == 0 and c.thin_batch_run() == 0
    assert c.thin_batch_stage_shared(nat_shared(shared([], [], [], [], [], [], []))) == 0 and c.thin_batch_run() == 0


def test_validation_level_2(golden_dir):
    """a point with a torsion component, (x, y) -> (-x, -y) as tests/test_gpu_wire.py builds it: on the curve, outside the subgroup"""
    from ark_vrf_amd import _native as nat
    sb = real_batch(0, [1] * 20, 3, 2)
    tweak = lambda p: ((Q0 - int.from_bytes(p[:32], "little")) % Q0).to_bytes(32, "little") + ((Q0 - int.from_bytes(p[32:], "little")) % Q0).to_bytes(32, "little")
    c = nat.Context(0)
    try:
        for level in (1, 2):
            c.set_validation(level)
            assert c.thin_batch_stage_shared(nat_shared(sb)) == 0 and c.thin_batch_run() == 0
        for r in (0, 4):                                                         # a key row, an input row (both referenced)
            rows = list(sb["rows"]); rows[r] = tweak(rows[r])
            assert c.thin_batch_stage_shared(nat_shared(dict(sb, rows=rows))) == 0 and c.thin_batch_run() == 2
        assert c.thin_batch_stage_shared(nat_shared(dict(sb, rows=sb["rows"] + [tweak(sb["rows"][0])]))) == 0 and c.thin_batch_run() == 2   # every row is validated
        outs = list(sb["outputs"]); outs[9] = tweak(outs[9])
        assert c.thin_batch_stage_shared(nat_shared(dict(sb, outputs=outs))) == 0 and c.thin_batch_run() == 2
        pr = list(sb["proofs"]); pr[2] = tweak(pr[2][:64]) + pr[2][64:]
        assert c.thin_batch_stage_shared(nat_shared(dict(sb, proofs=pr))) == 0 and c.thin_batch_run() == 2
        c.set_validation(1)                                                      # on the curve: level 1 lets the torsion point through to the equation
        rows = list(sb["rows"]); rows[0] = tweak(rows[0])
        assert c.thin_batch_stage_shared(nat_shared(dict(sb, rows=rows))) == 0 and c.thin_batch_run() in (0, 1)
        c.set_validation(0)
        assert c.thin_batch_stage_shared(nat_shared(sb)) == 0 and c.thin_batch_run() == 0
    finally:
        c.close()


# ---------------------------------------------------------------- the other run entry points

def test_three_call_run(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 130, 3, 2)
    for b, verdict in [(sb, 0), (tampered(sb, 77), 1)]:
        assert c.thin_batch_stage_shared(nat_shared(b)) == 0
        assert c.thin_batch_run() == verdict
        one_call = c.last_terms()
        assert c.batch_run_begin() == 0 and c.batch_run_hash() == 0 and c.batch_run_end() == verdict
        assert c.last_terms() == one_call
    assert c.thin_batch_stage(nat_batch(expanded(sb))) == 0 and c.thin_batch_run() == 0                  # plainly afterwards
    assert len(c.last_terms()[1]) // 32 == 4 * 130 + 1
    assert run_and_compare(c, 0, sb) == 0                                                                # and shared again


def test_pool(ctxs):
    from ark_vrf_amd import _native as nat
    sb = real_batch(0, [1] * 130, 3, 2)
    good, bad = nat_shared(sb), nat_shared(tampered(sb, 5))
    pool = nat.Pool(0, device=0, kind=1, slots=2, lanes=1, threads=1)
    try:
        tk = [pool.submit_shared(good), pool.submit_shared(bad)]
        assert [pool.wait(t) for t in tk] == [0, 1]
        for from_host in (False, True):
            tk = [pool.resubmit(t, from_host=from_host) for t in tk]
            assert [pool.wait(t) for t in tk] == [0, 1]
        idx = list(sb["pk_index"]); idx[129] = len(sb["rows"])
        with pytest.raises(nat.AvrfError):                                       # the indices are checked before a ticket exists
            pool.submit_shared(nat_shared(dict(sb, pk_index=idx)))
        tk = [pool.submit(nat_batch(expanded(tampered(sb, 5)))), pool.submit(nat_batch(expanded(sb)))]   # plain batches into the same slots
        assert [pool.wait(t) for t in tk] == [1, 0]
        tk = [pool.submit_shared(good), pool.submit_shared(bad)]
        assert [pool.wait(t) for t in tk] == [0, 1]
    finally:
        pool.close()


def test_repeatability(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 3000, 3, 2)
    assert c.thin_batch_stage_shared(nat_shared(sb)) == 0
    runs = []
    for _ in range(3):
        assert c.thin_batch_run() == 0
        runs.append(c.last_terms())
    assert runs[0] == runs[1] == runs[2]
