"""GPU parity: the shared-table Thin batch staged from wire bytes (include/avrf.h avrf_thin_batch_stage_shared_wire).

The expectation is always the x || y shared staging of the SAME batch (avrf_thin_batch_stage_shared), which run_and_compare of
test_gpu_thin_shared pins to the oracle's folded terms: the wire staging must leave, byte for byte, the same terms and the same
verdict.  A batch is the dict of test_gpu_thin_shared (x || y points); `wire` compresses its rows, outputs and R with the oracle."""
import json
import os

import pytest

import oracle as orc
from helpers import IDENTITY_XY, nat_batch, xy
from test_gpu_thin_shared import NAMES, expanded, fold, partial_of, prefix, real_batch, run_and_compare, shared, tampered

pytestmark = pytest.mark.gpu

Q = {0: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
     1: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}


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


_COMP = {}


def comp(suite, pxy):
    """x || y -> the suite's wire point (suite 4: the oracle's 32-byte form re-encoded as the 33-byte short-Weierstrass one)"""
    key = (suite, pxy)
    if key not in _COMP:
        w = orc.point_compress(suite, pxy)
        _COMP[key] = orc.sw_encode(suite, w) if suite == orc.BANDERSNATCH_SW else w
    return _COMP[key]


def point_len(suite):
    return 33 if suite == orc.BANDERSNATCH_SW else orc.pt_len(suite)


def wire(suite, sb):
    """the batch's wire form: rows / outputs as lists of compressed points, proofs as R || s"""
    return dict(sb, rows=[comp(suite, r) for r in sb["rows"]], outputs=[comp(suite, o) for o in sb["outputs"]],
                proofs=[comp(suite, p[:64]) + p[64:] for p in sb["proofs"]])


def nat_wire(suite, wb):
    from ark_vrf_amd._native import SharedWireBatch
    L = point_len(suite)
    assert all(len(r) == L for r in wb["rows"]) and all(len(p) == L + 32 for p in wb["proofs"])
    return SharedWireBatch(wb["n"], b"".join(wb["rows"]), wb["pk_index"], wb["input_index"], b"".join(wb["outputs"]), wb["io_counts"],
                           b"".join(wb["ads"]), [len(a) for a in wb["ads"]], b"".join(wb["proofs"]), L)


def same_as_xy(c, suite, sb, validate):
    """x || y shared staging (terms pinned to the oracle) -> wire staging of the same batch: same terms, same verdict; returns it"""
    st_xy = run_and_compare(c, suite, sb)
    want = c.last_terms()
    assert c.thin_batch_stage_shared_wire(nat_wire(suite, wire(suite, sb)), validate) == 0
    st = c.thin_batch_run()
    assert c.last_terms() == want
    assert st == st_xy
    return st


def bad_point(suite):
    """a y with no x on the curve, as tests/test_gpu_wire.py builds it"""
    return next(k.to_bytes(32, "little") for k in range(2, 300) if orc.point_decompress(suite, k.to_bytes(32, "little"))[0] != 0)


def torsion(suite, pxy):
    """(x, y) -> (-x, -y): on the curve, outside the prime-order subgroup"""
    q = Q[suite]
    return ((q - int.from_bytes(pxy[:32], "little")) % q).to_bytes(32, "little") + ((q - int.from_bytes(pxy[32:], "little")) % q).to_bytes(32, "little")


def placements(wb, pt, last_r=False):
    """the wire batch with `pt` as a referenced row, as an unreferenced last row, as an output, as an item's R"""
    rows = list(wb["rows"]); rows[wb["pk_index"][3]] = pt
    outs = list(wb["outputs"]); outs[5] = pt
    j = wb["n"] - 1 if last_r else 2
    pr = list(wb["proofs"]); pr[j] = pt + pr[j][len(pt):]
    return {"referenced row": dict(wb, rows=rows), "unreferenced row": dict(wb, rows=wb["rows"] + [pt]),
            "output": dict(wb, outputs=outs), "R": dict(wb, proofs=pr)}


# ---------------------------------------------------------------- 1. reference vectors

@pytest.mark.parametrize("validate", [0, 1])
@pytest.mark.parametrize("suite", [0, 1])
def test_reference_vectors(ctxs, golden_dir, suite, validate):
    with open(os.path.join(golden_dir, NAMES[suite] + "_thin.json")) as f:
        vs = json.load(f)
    rows_w = [bytes.fromhex(v["pk"]) for v in vs] + [bytes.fromhex(v["h"]) for v in vs]
    assert len(rows_w) == 14
    wb = shared(rows_w, range(7), range(7, 14), [bytes.fromhex(v["gamma"]) for v in vs], [1] * 7, [bytes.fromhex(v["ad"]) for v in vs],
                [bytes.fromhex(v["proof_r"] + v["proof_s"]) for v in vs])                          # the vectors' own bytes
    sb = dict(wb, rows=[xy(suite, r) for r in wb["rows"]], outputs=[xy(suite, o) for o in wb["outputs"]],
              proofs=[xy(suite, p[:32]) + p[32:] for p in wb["proofs"]])
    c = ctxs[suite]
    assert c.thin_batch_stage_shared_wire(nat_wire(suite, wb), validate) == 0 and c.thin_batch_run() == 0
    got = c.last_terms()
    assert run_and_compare(c, suite, sb) == 0                                                     # x || y staging == fold(oracle terms)
    assert got == c.last_terms()
    _, bases, sc = orc.thin_batch_terms_xy(suite, expanded(sb))
    assert got == fold(suite, sb, bases, sc)
    bad = list(wb["proofs"]); bad[4] = bad[4][:32] + bytes([bad[4][32] ^ 1]) + bad[4][33:]         # tampered s
    assert c.thin_batch_verify_shared_wire(nat_wire(suite, dict(wb, proofs=bad)), validate) == 1


# ---------------------------------------------------------------- 2. segment boundaries of the decoding kernel

@pytest.fixture(scope="module")
def material():
    """258 distinct points, 129 outputs, proofs (R, s < r) and additional data of one synthetic batch"""
    b = orc.gen_batch(0, 0, 129)
    n = b["n"]
    pts = [b["pks_xy"][64 * j: 64 * j + 64] for j in range(n)] + [b["ios_xy"][128 * j: 128 * j + 64] for j in range(n)]
    assert len(set(pts)) == 2 * n and IDENTITY_XY not in pts
    ads, off = [], 0
    for ln in b["ad_lens"]:
        ads.append(b["ads"][off: off + ln]); off += ln
    return dict(pts=pts, outs=[b["ios_xy"][128 * j + 64: 128 * j + 128] for j in range(n)], ads=ads,
                proofs=[b["proofs"][96 * j: 96 * j + 96] for j in range(n)])


SEGMENTS = [(1, [0]), (3, [1, 0, 2, 1, 1]), (5, [0, 1, 2, 3, 5, 1, 0, 2, 16, 17])]
SEGMENTS += [(t, [1] * n) for n in (63, 64, 65, 127, 129) for t in (1, 64, 65, 129)]


@pytest.mark.parametrize("t,counts", SEGMENTS, ids=lambda v: str(v) if isinstance(v, int) else "n%d_io%d" % (len(v), sum(v)))
def test_segment_boundaries(ctxs, material, t, counts):
    """thread g of the kernel is row g, output g - T or proof g - T - sum(m): empty output segment, mixed pair counts, and every
    segment ending just before, on and just after a wave and a block (the proofs belong to other keys: the terms are what is compared)"""
    n, tot = len(counts), sum(counts)
    sb = shared(material["pts"][:t], [(5 * j + 2) % t for j in range(n)], [(7 * k + 3) % t for k in range(tot)], material["outs"][:tot],
                counts, material["ads"][:n], material["proofs"][:n])
    assert same_as_xy(ctxs[0], 0, sb, 1) in (0, 1)


# ---------------------------------------------------------------- 3. verifying batches

@pytest.mark.parametrize("n", [130, 3000])
def test_verifying_batches(ctxs, n):
    """K = 3 keys, M = 2 inputs: n = 130 runs the single-launch MSM, n = 3 000 Pippenger"""
    c = ctxs[0]
    sb = prefix(real_batch(0, [1] * 3000, 3, 2), n)
    bad = tampered(sb, n // 2)
    assert same_as_xy(c, 0, sb, 1) == 0
    assert same_as_xy(c, 0, bad, 1) == 1
    if n != 130:
        return
    for b, verdict in [(sb, 0), (bad, 1)]:
        _, bases, sc = orc.thin_batch_terms_xy(0, expanded(b))
        want = orc.msm(0, bases, sc)
        assert (want == IDENTITY_XY) == (verdict == 0)
        assert c.thin_batch_stage_shared_wire(nat_wire(0, wire(0, b)), 1) == 0
        assert partial_of(c, 0, n, b["proofs"]) == want                                            # avrf_thin_batch_partial under the true seed
        assert c.thin_batch_run() == verdict
        one_call = c.last_terms()
        assert c.batch_run_begin() == 0 and c.batch_run_hash() == 0 and c.batch_run_end() == verdict
        assert c.last_terms() == one_call


# ---------------------------------------------------------------- 4. every other suite

@pytest.mark.parametrize("validate", [0, 1])
@pytest.mark.parametrize("suite", [1, 2, 3, 4, 5, 6, 7])
def test_other_suites(ctxs, suite, validate):
    """suites 4 and 7 have 33-byte points (proofs 65 apart); suites 5 and 6 take their responses for the host's weight stream from the wire proof"""
    sb = real_batch(suite, [1] * 40, 3, 2)
    assert ctxs[suite].point_len == point_len(suite)
    assert same_as_xy(ctxs[suite], suite, sb, validate) == 0
    assert same_as_xy(ctxs[suite], suite, tampered(sb, 17), validate) == 1


# ---------------------------------------------------------------- 5. points that do not decode

@pytest.mark.parametrize("validate", [0, 1])
def test_decoding_failures(ctxs, validate):
    from ark_vrf_amd import _native as nat
    c = ctxs[0]
    sb = real_batch(0, [1] * 20, 3, 2)
    wb = wire(0, sb)
    bad_y = bad_point(0)
    # what a run answers after a failed avrf_thin_batch_stage_wire: the same items, expanded, with the key of item 3 undecodable
    pks = [wb["rows"][r] for r in wb["pk_index"]]; pks[3] = bad_y
    ios = b"".join(wb["rows"][r] + o for r, o in zip(wb["input_index"], wb["outputs"]))
    assert nat.lib().avrf_thin_batch_stage_wire(c._h, nat.C.c_size_t(20), nat._u8(b"".join(pks)), nat._u8(ios), nat._u32([1] * 20), nat._u8(b"".join(wb["ads"])),
                                                nat._u32([len(a) for a in wb["ads"]]), nat._u8(b"".join(wb["proofs"])), validate) == 2
    after_wire = c.thin_batch_run()
    for where, b in placements(wb, bad_y, last_r=True).items():
        assert c.thin_batch_stage_shared_wire(nat_wire(0, b), validate) == 2, where
        assert c.thin_batch_run() == after_wire, where
    assert c.thin_batch_verify_shared_wire(nat_wire(0, wb), validate) == 0                         # a good batch staged afterwards verifies


# ---------------------------------------------------------------- 6. Validate::Yes

@pytest.mark.parametrize("suite", [0, 1])
def test_validate_yes(ctxs, suite):
    c = ctxs[suite]
    sb = real_batch(suite, [1] * 20, 3, 2)
    wb = wire(suite, sb)
    for where, b in placements(wb, comp(suite, torsion(suite, sb["rows"][1]))).items():
        assert c.thin_batch_stage_shared_wire(nat_wire(suite, b), 1) == 2, where
        assert c.thin_batch_stage_shared_wire(nat_wire(suite, b), 0) == 0, where                   # Validate::No: it decodes
    ident = comp(suite, IDENTITY_XY)
    spare = dict(wb, rows=wb["rows"] + [ident])                                                    # an identity row nothing refers to
    assert c.thin_batch_stage_shared_wire(nat_wire(suite, spare), 1) == 2                          # (the x || y flavour lets it pass)
    assert c.thin_batch_stage_shared_wire(nat_wire(suite, spare), 0) == 0 and c.thin_batch_run() == 0
    idx = list(wb["pk_index"]); idx[3] = len(wb["rows"])
    assert c.thin_batch_stage_shared_wire(nat_wire(suite, dict(spare, pk_index=idx)), 0) == 0 and c.thin_batch_run() == 2   # referenced: src/thin.rs:266-271
    assert c.thin_batch_verify_shared_wire(nat_wire(suite, wb), 1) == 0


# ---------------------------------------------------------------- 7. bad indices, the empty batch

def test_bad_index_is_refused(ctxs):
    c = ctxs[0]
    sb = real_batch(0, [1] * 20, 3, 2)
    wb = wire(0, sb)
    t = len(wb["rows"])
    assert c.thin_batch_stage(nat_batch(expanded(sb))) == 0 and c.thin_batch_run() == 0
    for into, j, v in [("pk_index", 0, t), ("pk_index", 19, t), ("input_index", 11, t), ("pk_index", 4, 0xffffffff)]:
        idx = list(wb[into]); idx[j] = v
        assert c.thin_batch_stage_shared_wire(nat_wire(0, dict(wb, **{into: idx})), 1) == -2
        assert c.thin_batch_run() == 0                                                             # nothing was staged: the plain batch is still there
    assert c.thin_batch_stage_shared_wire(nat_wire(0, dict(wb, rows=[], pk_index=[0] * 20, input_index=[0] * 20)), 1) == -2   # n_shared == 0, n > 0
    assert len(c.last_terms()[1]) // 32 == 4 * 20 + 1
    # the empty batch, with and without a table
    assert c.thin_batch_stage_shared_wire(nat_wire(0, shared(wb["rows"], [], [], [], [], [], [])), 1) == 0 and c.thin_batch_run() == 0
    assert c.thin_batch_verify_shared_wire(nat_wire(0, shared([], [], [], [], [], [], [])), 1) == 0


# ---------------------------------------------------------------- 8. the pool

def test_pool(ctxs):
    from ark_vrf_amd import _native as nat
    sb = real_batch(0, [1] * 130, 3, 2)
    wb = wire(0, sb)
    good, bad = nat_wire(0, wb), nat_wire(0, wire(0, tampered(sb, 5)))
    undecodable = nat_wire(0, placements(wb, bad_point(0), last_r=True)["R"])
    pool = nat.Pool(0, device=0, kind=1, slots=2, lanes=1, threads=1)
    try:
        tk = [pool.submit_shared_wire(good), pool.submit_shared_wire(bad)]
        assert [pool.wait(t) for t in tk] == [0, 1]
        for from_host in (False, True):
            tk = [pool.resubmit(t, from_host=from_host) for t in tk]
            assert [pool.wait(t) for t in tk] == [0, 1]
        t = pool.submit_shared_wire(undecodable, validate=0)
        assert pool.wait(t) == 2
        t = pool.resubmit(t, from_host=False)                                                      # the resident state repeats the verdict
        assert pool.wait(t) == 2
        tk = [pool.submit(nat_batch(expanded(sb))), pool.submit(nat_batch(expanded(sb)))]          # plain batches into the same slots
        assert [pool.wait(t) for t in tk] == [0, 0]
        idx = list(wb["pk_index"]); idx[129] = len(wb["rows"])
        with pytest.raises(nat.AvrfError):                                                         # the indices are checked before a ticket exists
            pool.submit_shared_wire(nat_wire(0, dict(wb, pk_index=idx)))
        tk = [pool.submit_shared_wire(good), pool.submit_shared_wire(good, validate=0)]
        assert [pool.wait(t) for t in tk] == [0, 0]
        done, mism, _ = pool.cycle(steps_block=2, from_host=True, expect=0)
        assert done >= 2 and done % 2 == 0 and mism == 0
    finally:
        pool.close()


# ---------------------------------------------------------------- 9. repeatability

def test_repeatability(ctxs):
    c = ctxs[0]
    sb = prefix(real_batch(0, [1] * 3000, 3, 2), 1000)
    assert c.thin_batch_stage_shared_wire(nat_wire(0, wire(0, sb)), 1) == 0
    runs = []
    for _ in range(3):
        assert c.thin_batch_run() == 0
        runs.append(c.last_terms())
    assert runs[0] == runs[1] == runs[2]
