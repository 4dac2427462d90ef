"""GPU parity: thin::BatchVerifier over segments of one staged batch (include/avrf.h avrf_thin_batch_run_segments) and the segmented
MSM under it (avrf_msm_te_segments), against the CPU oracle.

The expectation for a segment is always the oracle on THAT SEGMENT'S ITEMS ALONE: orc.thin_batch_terms_xy gives the terms of
src/thin.rs:282-317 in the order R, pk, (O_i, I_i).., G, compared bit for bit with avrf_thin_segment_terms; a status is compared
with the oracle's verdict and with avrf_thin_batch_verify of the segment on its own.  The oracle's results are computed once per
module and shared."""
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
SEGS9 = [1, 2, 3, 5, 7, 16, 33, 64, 130]
BAD_ARG = -2


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


# ---- a batch as a list of items; an item is a dict of the C-ABI pieces (pk 64, ios m x 128, ad, proof 96) and the wire pieces

def item(suite, pk, ios, ad, proof):
    L = orc.pt_len(suite)
    return dict(pk=xy(suite, pk), ios=[xy(suite, i) + xy(suite, o) for i, o in ios], ad=ad, proof=xy(suite, proof[:L]) + proof[L:],
                w_pk=pk, w_ios=[i + o for i, o in ios], w_proof=proof)


def made_items(suite, counts, seed):
    """VERIFYING items with counts[j] I/O pairs each: keys, inputs, outputs and proofs by the oracle's prover"""
    keys = [orc.from_seed(suite, bytes([k + 1, seed]) + bytes(30)) for k in range(5)]
    inputs = [orc.hash_to_curve(suite, b"seg-slot-%d" % i) for i in range(4)]
    outs = {(k, i): orc.vrf_output(suite, keys[k][0], inputs[i]) for k in range(5) for i in range(4)}
    rng = random.Random(seed)
    plan = [(rng.randrange(5), [rng.randrange(4) for _ in range(m)], b"ad-%d" % j * (j % 3)) for j, m in enumerate(counts)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        proofs = list(ex.map(lambda p: orc.thin_prove(suite, keys[p[0]][0], [(inputs[i], outs[p[0], i]) for i in p[1]], p[2]), plan))
    return [item(suite, keys[k][1], [(inputs[i], outs[k, i]) for i in ii], ad, pr) for (k, ii, ad), pr in zip(plan, proofs)]


def golden_items(suite, golden_dir):
    with open(os.path.join(golden_dir, NAMES[suite] + "_thin.json")) as f:
        vs = json.load(f)
    return [item(suite, bytes.fromhex(v["pk"]), [(bytes.fromhex(v["h"]), bytes.fromhex(v["gamma"]))], bytes.fromhex(v["ad"]),
                 bytes.fromhex(v["proof_r"] + v["proof_s"])) for v in vs]


def gen_items(suite, n):
    """orc.gen_batch's one-pair items as item dicts (C-ABI pieces only)"""
    b = orc.gen_batch(suite, 0, n)
    off = [0]
    for ln in b["ad_lens"]:
        off.append(off[-1] + ln)
    return [dict(pk=b["pks_xy"][64 * j: 64 * j + 64], ios=[b["ios_xy"][128 * j: 128 * j + 128]], ad=b["ads"][off[j]: off[j + 1]],
                 proof=b["proofs"][96 * j: 96 * j + 96]) for j in range(n)]


def batch_dict(items):
    """items -> a gen_batch-style dict in the C-ABI (xy) layout"""
    return dict(n=len(items), pks_xy=b"".join(it["pk"] for it in items), ios_xy=b"".join(p for it in items for p in it["ios"]),
                io_counts=[len(it["ios"]) for it in items], ads=b"".join(it["ad"] for it in items), ad_lens=[len(it["ad"]) for it in items],
                proofs=b"".join(it["proof"] for it in items), sks=b"")


def wire_batch(items):
    from ark_vrf_amd._native import Batch
    return Batch(len(items), b"".join(p for it in items for p in it["w_ios"]), [len(it["ios"]) for it in items], b"".join(it["ad"] for it in items),
                 [len(it["ad"]) for it in items], pks_xy=b"".join(it["w_pk"] for it in items), proofs=b"".join(it["w_proof"] for it in items))


def slices(items, segs):
    out, at = [], 0
    for k in segs:
        out.append(items[at: at + k]); at += k
    assert at == len(items)
    return out


def tamper_s(it):
    return dict(it, proof=it["proof"][:64] + bytes([it["proof"][64] ^ 1]) + it["proof"][65:],
                w_proof=it.get("w_proof", b"")[:-32] + bytes([it["proof"][64] ^ 1]) + it.get("w_proof", b"")[-31:])


def oracle_segment(suite, seg):
    """(status, bases, scalars) of the segment's items as a batch of their own; nothing for an empty segment (src/thin.rs:262-264)"""
    if not seg:
        return 0, b"", b""
    b = batch_dict(seg)
    st, bases, sc = orc.thin_batch_terms_xy(suite, b)
    return (orc.thin_batch_verify_xy(suite, b) if st == 0 else st), bases, sc


def check_run(c, suite, items, segs):
    """stage, run the segments, compare every status and every segment's terms with the oracle on the segment alone; -> statuses"""
    assert c.thin_batch_stage(nat_batch(batch_dict(items))) == 0
    got = c.thin_batch_run_segments(segs)
    assert isinstance(got, list) and len(got) == len(segs), got
    for v, seg in enumerate(slices(items, segs)):
        st, bases, sc = oracle_segment(suite, seg)
        assert got[v] == st, (v, got, st)
        if st != 2:
            gb, gs = c.thin_segment_terms(v)
            assert gs == sc and gb == bases, v
    return got


@pytest.fixture(scope="module")
def nine(golden_dir):
    """261 verifying items of suite 0 in nine segments; the 7-item one is the reference's thin vectors, the others have 0 to 3 pairs"""
    rng = random.Random(3)
    made = made_items(0, [rng.choice([0, 1, 1, 2, 3]) for _ in range(sum(SEGS9) - 7)], 7)
    return made[:11] + golden_items(0, golden_dir) + made[11:]


# ---------------------------------------------------------------- the engine alone

_POINTS = {}


def points(suite):
    if suite not in _POINTS:
        g = orc.suite_point(suite, 0)
        rng = random.Random(40 + suite)
        _POINTS[suite] = [xy(suite, orc.smul(suite, rng.randrange(1, R_ORDER[suite]).to_bytes(32, "little"), g)) for _ in range(48)]
    return _POINTS[suite]


def engine_case(c, suite, n_seg, L, seed):
    """n_seg segments of L terms: random terms, but one segment all zero scalars, one a single base L times with the scalar r - 1 (a heavy
    bucket, the top signed digit), one and a half segments shorter than L (zero scalars behind their real length)"""
    rng, pts, r = random.Random(seed), points(suite), R_ORDER[suite]
    bases, scalars = [], []
    for v in range(n_seg):
        real = L if v % 3 else max(1, L // 2 + 1)
        bs = [rng.choice(pts) for _ in range(L)]
        ss = [rng.randrange(r) if t < real else 0 for t in range(L)]
        if v == 1:
            ss = [0] * L
        if v == 2:
            bs, ss = [pts[0]] * L, [r - 1] * L
        if v == 0 and L > 4:
            ss[0], ss[1], ss[2] = 1, r - 1, r - 2
        bases.append(b"".join(bs)); scalars.append(b"".join(s.to_bytes(32, "little") for s in ss))
    got = c.msm_segments(n_seg, b"".join(bases), b"".join(scalars))
    with ThreadPoolExecutor(max_workers=8) as ex:
        want = list(ex.map(lambda v: orc.msm(suite, bases[v], scalars[v]), range(n_seg)))
    assert got == want
    assert got[1] == (bytes(64) if suite == orc.SECP256R1 else IDENTITY_XY)       # all scalars zero: the suite's identity encoding
    return got


SEG_SHAPES = [(8, 5), (8, 300), (8, 600), (8, 1025), (8, 4100), (9, 2049), (3, 300), (3, 2100)]


@pytest.mark.parametrize("n_seg,L,suite", [(n, L, s) for s in (0, 1) for n, L in SEG_SHAPES] + [(8, 5, orc.SECP256R1), (8, 300, orc.SECP256R1)])
def test_msm_segments(ctxs, suite, n_seg, L):
    """window widths 4 (L = 5), 5 (300), 6 (600), 7 (1 025), 8 (2 049: nine segments) and 9 (4 100: nb = 256, the widest); three segments
    take the looped single-MSM route, through the single-launch form (300 terms) and through the Pippenger chain (2 100).  secp256r1, the
    native short-Weierstrass suite, at widths 4 and 5: the generic device Horner (k_horner) behind k_bits_direct, where the
    twisted-Edwards suites take k_horner_quads"""
    engine_case(ctxs[suite], suite, n_seg, L, 100 * n_seg + L)


def test_msm_segments_refusals(ctxs):
    from ark_vrf_amd import _native as nat
    c, pts = ctxs[0], points(0)
    call = lambda n_seg, L: nat.lib().avrf_msm_te_segments(c._h, C.c_size_t(n_seg), C.c_size_t(L), nat._u8(pts[0] * (n_seg * L)),
                                                           nat._u8(bytes(32 * n_seg * L)), (C.c_uint8 * (64 * n_seg))())
    assert call(2, 8192) == BAD_ARG                       # a segment over AVRF_SEGMENT_TERMS_MAX
    assert call(1009, 5) == BAD_ARG                       # 1 009 x 65 virtual windows
    assert call(8, 5) == 0
    assert c.msm_segments(0, b"", b"") == []


# ---------------------------------------------------------------- verdicts and terms

def test_nine_segments(ctxs, nine):
    c = ctxs[0]
    assert check_run(c, 0, nine, SEGS9) == [0] * 9
    # every status is what avrf_thin_batch_verify answers for the segment on its own
    for seg in slices(nine, SEGS9):
        assert c.thin_batch_stage(nat_batch(batch_dict(seg))) == 0 and c.thin_batch_run() == 0


def test_tampered_and_invalid_segments(ctxs, nine):
    """a tampered s in the 3-item and in the 64-item segment: exactly those two fail; the identity key in the 5-item segment: that one is
    InvalidData and nothing else moves"""
    c = ctxs[0]
    bad = list(nine)
    bad[1 + 2 + 1] = tamper_s(bad[1 + 2 + 1])
    j64 = sum(SEGS9[:7]) + 40
    bad[j64] = tamper_s(bad[j64])
    assert check_run(c, 0, bad, SEGS9) == [0, 0, 1, 0, 0, 0, 0, 1, 0]
    bad[1 + 2 + 3 + 2] = dict(bad[1 + 2 + 3 + 2], pk=IDENTITY_XY)
    got = check_run(c, 0, bad, SEGS9)
    assert got == [0, 0, 1, 2, 0, 0, 0, 1, 0]
    for st, seg in zip(got, slices(bad, SEGS9)):
        assert c.thin_batch_stage(nat_batch(batch_dict(seg))) == 0 and c.thin_batch_run() == st
    # the one-call form
    assert c.thin_batch_verify_segments(nat_batch(batch_dict(bad)), SEGS9) == got
    # a scalar >= r and a non-canonical coordinate mark their own segments too
    r_bytes = R_ORDER[0].to_bytes(32, "little")
    worse = list(nine)
    worse[0] = dict(worse[0], proof=worse[0]["proof"][:64] + r_bytes)
    worse[-1] = dict(worse[-1], proof=Q0.to_bytes(32, "little") + worse[-1]["proof"][32:])
    assert c.thin_batch_stage(nat_batch(batch_dict(worse))) == 0
    got = c.thin_batch_run_segments(SEGS9)
    assert got == [2, 0, 0, 0, 0, 0, 0, 0, 2]
    for st, seg in zip(got, slices(worse, SEGS9)):
        assert c.thin_batch_stage(nat_batch(batch_dict(seg))) == 0 and c.thin_batch_run() == st


@pytest.mark.parametrize("segs", [[11, 7, 243], [1, 2, 3, 5, 0, 7, 16, 33, 64, 130], [0, 261, 0]])
def test_other_segmentations(ctxs, nine, segs):
    """three segments take the route below eight (one MSM per segment); an empty segment in the middle is Ok and has no terms"""
    c = ctxs[0]
    assert check_run(c, 0, nine, segs) == [0] * len(segs)
    bad = list(nine)
    bad[12] = tamper_s(bad[12])
    want = [int(12 in range(sum(segs[:v]), sum(segs[:v + 1]))) for v in range(len(segs))]
    assert check_run(c, 0, bad, segs) == want
    for v, k in enumerate(segs):
        if not k:
            assert c.thin_segment_terms(v) == (b"", b"")


# ---------------------------------------------------------------- locate

def test_locate_in_3000(ctxs):
    from ark_vrf_amd import _native as nat
    c = ctxs[0]
    items = gen_items(0, 3000)
    bad = list(items)
    for j in (777, 2990):
        bad[j] = tamper_s(bad[j])
    b = nat_batch(batch_dict(bad))
    segs = [64] * 46 + [56]
    assert c.thin_batch_stage(b) == 0 and c.thin_batch_run() == 1
    got = c.thin_batch_run_segments(segs)
    assert [v for v, st in enumerate(got) if st] == [777 // 64, 2990 // 64] and set(got) == {0, 1}
    # a plain run on the same staging keeps its verdict and its terms
    assert c.thin_batch_run() == 1
    st_o, bases, sc = orc.thin_batch_terms_xy(0, batch_dict(bad))
    assert st_o == 0 and c.last_terms() == (bases, sc)
    assert c.thin_batch_run_segments(segs) == got
    assert c.thin_batch_run() == 1 and c.last_terms() == (bases, sc)
    # the per-item call's statuses, folded per segment
    each = c.thin_verify(b)
    assert [j for j, st in enumerate(each) if st] == [777, 2990]
    assert [max(s) for s in slices(each, segs)] == got
    # thin_verify left the batch staged: segments of it again
    assert c.thin_batch_run_segments(segs) == got


# ---------------------------------------------------------------- other stagings and suites

@pytest.mark.parametrize("validate", [0, 1])
def test_wire_staging(ctxs, nine, validate):
    from ark_vrf_amd import _native as nat
    c = ctxs[0]
    bad = list(nine)
    bad[30] = tamper_s(bad[30])
    want = [0, 0, 0, 0, 0, 1, 0, 0, 0]
    wb = wire_batch(bad)
    assert nat.lib().avrf_thin_batch_stage_wire(c._h, C.c_size_t(wb.n), wb.pks_xy, wb.ios_xy, wb.io_counts, wb.ads, wb.ad_lens, wb.proofs, validate) == 0
    assert c.thin_batch_run_segments(SEGS9) == want
    for v, seg in enumerate(slices(bad, SEGS9)):
        assert c.thin_segment_terms(v) == oracle_segment(0, seg)[1:], v
    assert c.thin_batch_verify_segments_wire(wire_batch(nine), SEGS9, validate) == [0] * 9
    assert c.thin_batch_verify_segments_wire(wb, SEGS9, validate) == want


@pytest.mark.parametrize("suite", [orc.BABYJUBJUB, orc.BANDERSNATCH_SHAKE128])
def test_other_suites(ctxs, suite):
    """Baby-JubJub, and the SHAKE128 suite, whose weight streams the host squeezes per segment"""
    c = ctxs[suite]
    items = gen_items(suite, 32)
    assert check_run(c, suite, items, [4] * 8) == [0] * 8
    bad = list(items)
    bad[22] = tamper_s(bad[22])
    assert check_run(c, suite, bad, [4] * 8) == [0, 0, 0, 0, 0, 1, 0, 0]
    assert check_run(c, suite, bad, [10, 12, 10]) == [0, 0, 1]


def test_validation_level_2(ctxs):
    """an output with a torsion component, (x, y) -> (-x, -y): on the curve, outside the subgroup -- only its segment is InvalidData"""
    from ark_vrf_amd import _native as nat
    items = gen_items(0, 32)
    o = items[13]["ios"][0][64:]
    tors = ((Q0 - int.from_bytes(o[:32], "little")) % Q0).to_bytes(32, "little") + ((Q0 - int.from_bytes(o[32:], "little")) % Q0).to_bytes(32, "little")
    bad = list(items)
    bad[13] = dict(bad[13], ios=[bad[13]["ios"][0][:64] + tors])
    c = nat.Context(0)
    try:
        c.set_validation(2)
        assert c.thin_batch_stage(nat_batch(batch_dict(bad))) == 0
        assert c.thin_batch_run() == 2
        assert c.thin_batch_run_segments([4] * 8) == [0, 0, 0, 2, 0, 0, 0, 0]
        assert c.thin_batch_run_segments([10, 12, 10]) == [0, 2, 0]
        assert c.thin_batch_stage(nat_batch(batch_dict(items))) == 0 and c.thin_batch_run_segments([4] * 8) == [0] * 8
    finally:
        c.close()


# ---------------------------------------------------------------- refusals

def test_refusals(ctxs):
    from ark_vrf_amd import _native as nat
    c = nat.Context(0)
    try:
        assert c.thin_batch_run_segments([1]) == BAD_ARG                       # nothing staged
        items = gen_items(0, 40)
        bad = list(items)
        bad[5] = tamper_s(bad[5])
        b = batch_dict(bad)
        assert c.thin_batch_stage(nat_batch(b)) == 0 and c.thin_batch_run() == 1
        assert c.thin_batch_run_segments([20, 19]) == BAD_ARG                  # counts that do not sum to n
        assert c.thin_batch_run_segments([20, 21]) == BAD_ARG
        assert c.thin_batch_run_segments([1] * 40) == [0] * 5 + [1] + [0] * 34
        assert c.batch_run_begin() == 0
        assert c.thin_batch_run_segments([20, 20]) == BAD_ARG                  # between avrf_batch_run_begin and _end
        assert c.batch_run_hash() == 0 and c.batch_run_end() == 1              # the run is undisturbed
        assert c.thin_batch_run_segments([20, 20]) == [1, 0] and c.thin_batch_run() == 1
        # a limit exceeded: one segment of 2 048 one-pair items is 8 193 terms
        big = gen_items(0, 2048)
        assert c.thin_batch_stage(nat_batch(batch_dict(big))) == 0
        assert c.thin_batch_run_segments([2048]) == BAD_ARG and c.thin_batch_run() == 0
        assert c.thin_batch_run_segments([1024, 1024]) == [0, 0]
        # a shared-table staging
        rows, pk_index, input_index, outs = nat.dedup_points(b["pks_xy"], b["ios_xy"])
        sb = nat.SharedBatch(40, rows, pk_index, input_index, outs, b["io_counts"], b["ads"], b["ad_lens"], b["proofs"])
        assert c.thin_batch_stage_shared(sb) == 0
        assert c.thin_batch_run_segments([20, 20]) == BAD_ARG and c.thin_batch_run() == 1
        assert c.thin_segment_terms(0) == (b"", b"")                           # no segmented run on this staging
        # a Pedersen batch
        pb = orc.gen_batch(0, 1, 8)
        assert c.pedersen_batch_stage(nat_batch(pb)) == 0
        assert c.thin_batch_run_segments([4, 4]) == BAD_ARG and c.pedersen_batch_run() == 0
        # the empty batch: every (empty) segment is Ok
        assert c.thin_batch_stage(nat_batch(orc.gen_batch(0, 0, 0))) == 0
        assert c.thin_batch_run_segments([0, 0]) == [0, 0] and c.thin_batch_run_segments([]) == [] and c.thin_batch_run_segments([1]) == BAD_ARG
    finally:
        c.close()
