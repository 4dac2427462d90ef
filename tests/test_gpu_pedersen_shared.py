"""GPU parity: pedersen::BatchVerifier over a table of shared inputs (include/avrf.h avrf_pedersen_batch_stage_shared) vs the oracle.

The expectation is always the oracle's pedersen_batch_terms_xy of the EXPANDED batch (every index replaced by its row), folded on the
Python side into the shared layout (ped_shared_helpers.check_terms): item terms and the two base terms bit for bit; the row scalars bit
for bit when every item has at most one pair, as a group element otherwise (the oracle has no z_i).

Term comparisons need no verifying proofs (the verdict is then 1, the terms are built all the same), so the index distributions take
their points, responses and additional data from one synthetic batch of the oracle."""
import ctypes as C
import json
import os
import random

import pytest

import oracle as orc
from helpers import IDENTITY_XY, nat_batch, xy
from ped_shared_helpers import (BAD_ARG, Q, check_terms, expanded, nat_shared, prefix, real3k, real_batch, run_and_compare, shared,
                                tampered, torsion)

pytestmark = pytest.mark.gpu

NAMES = {0: "bandersnatch_sha-512_ell2", 1: "baby-jubjub_sha-512_tai"}


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


# ---------------------------------------------------------------- 1. reference vectors

@pytest.mark.parametrize("suite", [0, 1])
def test_reference_vectors_shared(ctxs, golden_dir, suite):
    with open(os.path.join(golden_dir, NAMES[suite] + "_pedersen.json")) as f:
        vs = json.load(f)
    L = orc.pt_len(suite)
    proofs = []
    for v in vs:
        p = bytes.fromhex(v["proof_pk_com"] + v["proof_r"] + v["proof_ok"] + v["proof_s"] + v["proof_sb"])
        proofs.append(b"".join(xy(suite, p[L * k: L * k + L]) for k in range(3)) + p[3 * L:])
    rows = sorted(set(xy(suite, bytes.fromhex(v["h"])) for v in vs))
    sb = shared(rows, [rows.index(xy(suite, bytes.fromhex(v["h"]))) for v in vs], [xy(suite, bytes.fromhex(v["gamma"])) for v in vs],
                [1] * len(vs), [bytes.fromhex(v["ad"]) for v in vs], proofs)
    c = ctxs[suite]
    assert run_and_compare(c, suite, sb) == 0
    assert run_and_compare(c, suite, tampered(sb, 4)) == 1
    assert c.pedersen_batch_stage_shared(nat_shared(dict(sb, ads=[b"x"] + sb["ads"][1:]))) == 0 and c.pedersen_batch_run() == 1   # wrong ad


# ---------------------------------------------------------------- 2. verifying batches

@pytest.mark.parametrize("n", [130, 3000])
def test_verifying_batches(ctxs, n):
    """3 inputs: n = 130 is 525 terms, n = 3 000 is 12 005 (Pippenger)"""
    c = ctxs[0]
    sb = prefix(real3k(), n)
    assert run_and_compare(c, 0, sb) == 0
    assert orc.pedersen_batch_verify_xy(0, expanded(sb)) == 0
    j = n // 2
    assert run_and_compare(c, 0, tampered(sb, j, 192)) == 1                     # one s
    assert run_and_compare(c, 0, tampered(sb, n - 1, 224)) == 1                 # one sb
    ok = list(sb["proofs"]); ok[j] = ok[j][:128] + ok[(j + 1) % n][128:192] + ok[j][192:]
    assert ok[j] != sb["proofs"][j]
    assert run_and_compare(c, 0, dict(sb, proofs=ok)) == 1                      # one Ok (another item's: a valid point)
    outs = list(sb["outputs"]); outs[3] = next(o for o in sb["outputs"] if o != outs[3])
    assert run_and_compare(c, 0, dict(sb, outputs=outs)) == 1                   # one output
    idx = list(sb["input_index"]); idx[7] = (idx[7] + 1) % 3
    assert run_and_compare(c, 0, dict(sb, input_index=idx)) == 1                # one input_index pointed at another row
    assert run_and_compare(c, 0, sb) == 0


# ---------------------------------------------------------------- 3. index distributions, terms only

@pytest.fixture(scope="module")
def material():
    """3 001 distinct inputs, outputs, proofs (points, s, sb < r) and additional data of one synthetic Pedersen batch.  The distributions
    take their rows from pts[1:] on (one_row: the last point), so that item 0 never gets its own input back and even n = 1 does not verify."""
    b = orc.gen_batch(0, 1, 3001)
    n = b["n"]
    pts = [b["ios_xy"][128 * j: 128 * j + 64] for j in range(n)]
    assert len(set(pts)) == n and IDENTITY_XY not in pts
    ads, off = [], 0
    for ln in b["ad_lens"]:
        ads.append(b["ads"][off: off + ln]); off += ln
    return dict(pts=pts, outs=[b["ios_xy"][128 * j + 64: 128 * j + 128] for j in range(n)], ads=ads,
                proofs=[b["proofs"][256 * j: 256 * j + 256] for j in range(n)])


def distribution(kind, n, pts):
    """-> (rows, input_index) for n items with one pair each"""
    rng = random.Random(n * 31 + len(kind))
    if kind == "one_row":                                                        # T = 1: one row takes everything
        return pts[3000:], [0] * n
    if kind == "all_distinct_reversed":                                          # T = n > the shares: k_shared_merge's by-lane branch
        return pts[1: n + 1], [n - 1 - j for j in range(n)]
    if kind == "skew":                                                           # one row takes 90 % of the references, 64 rows the rest
        return pts[1:66], [17 if rng.random() < 0.9 else rng.choice([r for r in range(65) if r != 17]) for _ in range(n)]
    if kind == "unreferenced":                                                   # unreferenced rows at both ends of the table (and inside)
        return pts[1:10], [rng.choice([2, 3, 6]) for _ in range(n)]
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["one_row", "all_distinct_reversed", "skew", "unreferenced"])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 63, 64, 65, 129, 1025, 3000])
def test_index_distributions(ctxs, material, n, kind):
    """7 / 8 / 9 and 63 / 64 / 65 straddle the share of eight slots and the 128-thread blocks"""
    rows, input_index = distribution(kind, n, material["pts"])
    sb = shared(rows, input_index, material["outs"][:n], [1] * n, material["ads"][:n], material["proofs"][:n])
    assert run_and_compare(ctxs[0], 0, sb) == 1                                  # (the proofs belong to other inputs: the terms are what is compared)
    if kind == "unreferenced":
        _, gs = ctxs[0].last_terms()
        for r in (0, 1, 4, 5, 7, 8):
            assert gs[32 * (4 * n + r): 32 * (4 * n + r + 1)] == bytes(32)


# ---------------------------------------------------------------- 4. mixed pair counts

def test_mixed_pair_counts(ctxs):
    """0 .. 17 pairs per item (the >= 16-pair merge among them): the rows as a group element, the rest bit for bit"""
    sb = real_batch(0, [0, 1, 2, 3, 16, 17, 1, 0], 4)
    assert run_and_compare(ctxs[0], 0, sb) == 0
    assert run_and_compare(ctxs[0], 0, tampered(sb, 4)) == 1
    assert run_and_compare(ctxs[0], 0, tampered(sb, 7, 224)) == 1                # sb of an item without pairs


# ---------------------------------------------------------------- 5. other suites

@pytest.mark.parametrize("suite", [1, 2, 3, 4, 5, 6, 7])
def test_other_suites(ctxs, suite):
    """suites 5 and 6 take their weights from the host's stream, suite 4 absorbs the 33-byte forms"""
    sb = real_batch(suite, [1] * 65, 2)
    assert run_and_compare(ctxs[suite], suite, sb) == 0
    assert run_and_compare(ctxs[suite], suite, tampered(sb, 17)) == 1


# ---------------------------------------------------------------- 6. identity and range

def test_identity_rows(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 20, 3)
    spare = dict(sb, rows=sb["rows"] + [IDENTITY_XY])                            # an identity row nothing refers to
    assert run_and_compare(c, 0, spare) == 0
    assert run_and_compare(c, 0, tampered(spare, 3)) == 1                        # ... the batch's normal verdict
    idx = list(sb["input_index"]); idx[7] = len(sb["rows"])
    assert c.pedersen_batch_stage_shared(nat_shared(dict(spare, input_index=idx))) == 0
    assert c.pedersen_batch_run() == 2                                           # referenced: io_identity, src/pedersen.rs:278,348-353
    assert run_and_compare(c, 0, sb) == 0


def test_non_canonical_rows(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 20, 3)
    row = sb["rows"][1]
    x = int.from_bytes(row[:32], "little")
    lifted = (x + Q[0]).to_bytes(32, "little") + row[32:]                        # the same x, not reduced
    assert x + Q[0] < 1 << 256
    assert c.pedersen_batch_stage_shared(nat_shared(dict(sb, rows=sb["rows"] + [lifted]))) == 0 and c.pedersen_batch_run() == 2   # unreferenced
    assert c.pedersen_batch_stage_shared(nat_shared(dict(sb, rows=[sb["rows"][0], lifted, sb["rows"][2]]))) == 0 and c.pedersen_batch_run() == 2
    assert run_and_compare(c, 0, sb) == 0                                        # (the flag does not outlive its staging)


def test_no_pairs_at_all(ctxs):
    """every item a valid, verifying no-pair proof, n_shared = 0: AVRF_OK; with a table nothing refers to: AVRF_OK and 4 n + T + 2 terms"""
    c = ctxs[0]
    sb = real_batch(0, [0] * 9, 3)
    assert orc.pedersen_batch_verify_xy(0, expanded(sb)) == 0
    assert c.pedersen_batch_stage_shared(nat_shared(dict(sb, rows=[]))) == 0 and c.pedersen_batch_run() == 0
    assert c.pedersen_batch_stage_shared(nat_shared(tampered(dict(sb, rows=[]), 4))) == 0 and c.pedersen_batch_run() == 1
    assert run_and_compare(c, 0, sb) == 0
    assert run_and_compare(c, 0, tampered(sb, 4, 224)) == 1
    one = real_batch(0, [1] * 20, 3)
    assert c.pedersen_batch_stage_shared(nat_shared(dict(one, rows=[], input_index=[0] * 20))) == BAD_ARG      # pairs and no table
    assert c.pedersen_batch_run() == 1                                           # the batch staged before it is still there
    # the empty batch, with and without a table
    assert c.pedersen_batch_stage_shared(nat_shared(shared(sb["rows"], [], [], [], [], []))) == 0 and c.pedersen_batch_run() == 0
    assert c.pedersen_batch_stage_shared(nat_shared(shared([], [], [], [], [], []))) == 0 and c.pedersen_batch_run() == 0


# ---------------------------------------------------------------- 7. bad index

def test_bad_index_is_refused(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 20, 3)
    before = tampered(sb, 2)
    assert run_and_compare(c, 0, before) == 1
    want = c.last_terms()
    for j, v in [(0, 3), (19, 3), (11, 0xffffffff)]:
        idx = list(sb["input_index"]); idx[j] = v
        assert c.pedersen_batch_stage_shared(nat_shared(dict(sb, input_index=idx))) == BAD_ARG
        assert c.pedersen_batch_run() == 1 and c.last_terms() == want            # the batch staged before it still runs to its verdict


# ---------------------------------------------------------------- 8. validation level 2

def test_validation_level_2():
    from ark_vrf_amd import _native as nat
    sb = real_batch(0, [1] * 20, 3)
    c = nat.Context(0)
    try:
        for level in (1, 2):
            c.set_validation(level)
            assert c.pedersen_batch_stage_shared(nat_shared(sb)) == 0 and c.pedersen_batch_run() == 0
        rows = list(sb["rows"]); rows[1] = torsion(0, rows[1])
        assert c.pedersen_batch_stage_shared(nat_shared(dict(sb, rows=rows))) == 0 and c.pedersen_batch_run() == 2          # a referenced row
        assert c.pedersen_batch_stage_shared(nat_shared(dict(sb, rows=sb["rows"] + [torsion(0, sb["rows"][0])]))) == 0 and c.pedersen_batch_run() == 2   # every row is validated
        outs = list(sb["outputs"]); outs[9] = torsion(0, outs[9])
        assert c.pedersen_batch_stage_shared(nat_shared(dict(sb, outputs=outs))) == 0 and c.pedersen_batch_run() == 2
        pr = list(sb["proofs"]); pr[2] = pr[2][:64] + torsion(0, pr[2][64:128]) + pr[2][128:]
        assert c.pedersen_batch_stage_shared(nat_shared(dict(sb, proofs=pr))) == 0 and c.pedersen_batch_run() == 2
        c.set_validation(0)
        assert c.pedersen_batch_stage_shared(nat_shared(sb)) == 0 and c.pedersen_batch_run() == 0
    finally:
        c.close()


# ---------------------------------------------------------------- 9. three-call run, challenges + partial

def partial_of(c, suite, n, proofs):
    """avrf_pedersen_batch_challenges, the true weight seed of the batch, avrf_pedersen_batch_partial from item 0 -> 64 bytes"""
    from ark_vrf_amd import _native as nat
    cs = (C.c_uint8 * (16 * n))()
    assert nat.lib().avrf_pedersen_batch_challenges(c._h, cs) == 0
    seed, out = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    assert nat.lib().avrf_batch_weight_seed(suite, 1, C.c_size_t(n), cs, nat._u8(b"".join(p[192:] for p in proofs)), seed) == 0
    assert nat.lib().avrf_pedersen_batch_partial(c._h, seed, C.c_uint64(0), out) == 0
    return bytes(out)


def test_three_call_run(ctxs):
    c = ctxs[0]
    sb = prefix(real3k(), 130)
    for b, verdict in [(sb, 0), (tampered(sb, 77), 1)]:
        assert c.pedersen_batch_stage_shared(nat_shared(b)) == 0
        assert c.pedersen_batch_run() == verdict
        one_call = c.last_terms()
        assert c.batch_run_begin() == 0 and c.batch_run_hash() == 0 and c.batch_run_end() == verdict
        assert c.last_terms() == one_call
        # the host seed reproduces the run's MSM point: the oracle's MSM of the expanded batch's terms
        _, bases, sc = orc.pedersen_batch_terms_xy(0, expanded(b))
        want = orc.msm(0, bases, sc)
        assert (want == IDENTITY_XY) == (verdict == 0)
        assert partial_of(c, 0, 130, b["proofs"]) == want
        assert orc.msm(0, *one_call) == want
        assert c.pedersen_batch_run() == verdict


# ---------------------------------------------------------------- 10. segments, 11. restaging

def test_segments_refuse_a_shared_staging(ctxs):
    c = ctxs[0]
    sb = tampered(prefix(real3k(), 40), 5)
    assert c.pedersen_batch_stage_shared(nat_shared(sb)) == 0
    assert c.pedersen_batch_run_segments([20, 20]) == BAD_ARG
    assert c.pedersen_batch_run() == 1                                           # the plain run afterwards still answers
    check_terms(0, sb, c.last_terms())
    assert c.pedersen_batch_run_segments([20, 20]) == BAD_ARG


def test_restaging_plainly(ctxs):
    c = ctxs[0]
    sb = prefix(real3k(), 130)
    assert run_and_compare(c, 0, sb) == 0
    e = expanded(sb)
    assert c.pedersen_batch_stage(nat_batch(e)) == 0 and c.pedersen_batch_run() == 0
    st_o, bases, sc = orc.pedersen_batch_terms_xy(0, e)
    assert st_o == 0 and len(sc) == 32 * (5 * 130 + 2) and c.last_terms() == (bases, sc)
    assert c.pedersen_batch_run_segments([65, 65]) == [0, 0]
    assert run_and_compare(c, 0, sb) == 0                                        # and shared again


# ---------------------------------------------------------------- 12. the pool

def test_pool():
    from ark_vrf_amd import _native as nat
    sb = prefix(real3k(), 130)
    good, bad = nat_shared(sb), nat_shared(tampered(sb, 5))
    pool = nat.Pool(0, device=0, kind=2, slots=2, lanes=1, threads=1)
    try:
        tk = [pool.submit_pedersen_shared(good), pool.submit_pedersen_shared(bad)]
        assert [pool.wait(t) for t in tk] == [0, 1]
        for from_host in (False, True):
            tk = [pool.resubmit(t, from_host=from_host) for t in tk]
            assert [pool.wait(t) for t in tk] == [0, 1]
        idx = list(sb["input_index"]); idx[129] = len(sb["rows"])
        with pytest.raises(nat.AvrfError):                                       # the indices are checked before a ticket exists
            pool.submit_pedersen_shared(nat_shared(dict(sb, input_index=idx)))
        with pytest.raises(nat.AvrfError):                                       # the Thin call still refuses a Pedersen pool
            pool._submit("avrf_pool_submit_shared", good, C.c_size_t(130), C.c_size_t(3), good.shared_xy, nat._u32([0] * 130), good.input_index,
                         good.outputs_xy, good.io_counts, good.ads, good.ad_lens, good.proofs)
        tk = [pool.submit(nat_batch(expanded(tampered(sb, 5)))), pool.submit(nat_batch(expanded(sb)))]   # plain batches into the same slots
        assert [pool.wait(t) for t in tk] == [1, 0]
        tk = [pool.submit_pedersen_shared(good), pool.submit_pedersen_shared(good)]
        assert [pool.wait(t) for t in tk] == [0, 0]
        done, mism, _ = pool.cycle(steps_block=2, from_host=True, expect=0)
        assert done >= 2 and done % 2 == 0 and mism == 0
    finally:
        pool.close()
    thin = nat.Pool(0, device=0, kind=1, slots=1, lanes=1, threads=1)
    try:
        with pytest.raises(nat.AvrfError):                                       # the Thin pool refuses the new call
            thin.submit_pedersen_shared(good)
    finally:
        thin.close()


# ---------------------------------------------------------------- 13. repeatability

def test_repeatability(ctxs):
    """the order of the atomics inside a row must not show"""
    c = ctxs[0]
    assert c.pedersen_batch_stage_shared(nat_shared(real3k())) == 0
    runs = []
    for _ in range(3):
        assert c.pedersen_batch_run() == 0
        runs.append(c.last_terms())
    assert runs[0] == runs[1] == runs[2]
    assert c.pedersen_batch_stage_shared(nat_shared(real3k())) == 0 and c.pedersen_batch_run() == 0     # another placement of the same references
    assert c.last_terms() == runs[0]
