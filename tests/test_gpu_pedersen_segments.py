"""GPU parity: pedersen::BatchVerifier over segments of one staged batch (include/avrf.h avrf_pedersen_batch_run_segments), against
the CPU oracle.

The expectation for a segment is always the oracle on THAT SEGMENT'S ITEMS ALONE: orc.pedersen_batch_terms_xy gives the terms of
src/pedersen.rs:383-418 in the order O, Ok, I, Yb, R per item, then G, then B, compared bit for bit with avrf_pedersen_segment_terms;
a status is compared with the oracle's verdict and with avrf_pedersen_batch_verify of the segment on its own.  The oracle's results
are computed once per module and shared."""
import ctypes as C
import json
import os
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import oracle as orc
from helpers import IDENTITY_XY, R_ORDER, nat_batch, xy

pytestmark = pytest.mark.gpu

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


# ---- a batch as a list of items; an item is a dict of the C-ABI pieces (ios m x 128, ad, proof 256) and the wire pieces

def item(suite, ios, ad, proof):
    L = orc.pt_len(suite)
    return dict(ios=[xy(suite, i) + xy(suite, o) for i, o in ios], ad=ad, proof=b"".join(xy(suite, proof[L * k: L * k + L]) for k in range(3)) + proof[3 * L:],
                w_ios=[i + o for i, o in ios], w_proof=proof)


def made_items(suite, counts, seed):
    """VERIFYING items with counts[j] I/O pairs each: keys, inputs, outputs and proofs by the oracle's prover"""
    keys = [orc.from_seed(suite, bytes([k + 1, seed]) + bytes(30)) for k in range(5)]
    inputs = [orc.hash_to_curve(suite, b"pseg-slot-%d" % i) for i in range(4)]
    outs = {(k, i): orc.vrf_output(suite, keys[k][0], inputs[i]) for k in range(5) for i in range(4)}
    rng = random.Random(seed)
    plan = [(rng.randrange(5), [rng.randrange(4) for _ in range(m)], b"ad-%d" % j * (j % 3)) for j, m in enumerate(counts)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        proofs = list(ex.map(lambda p: orc.pedersen_prove(suite, keys[p[0]][0], [(inputs[i], outs[p[0], i]) for i in p[1]], p[2])[0], plan))
    return [item(suite, [(inputs[i], outs[k, i]) for i in ii], ad, pr) for (k, ii, ad), pr in zip(plan, proofs)]


def golden_items(golden_dir):
    with open(os.path.join(golden_dir, "bandersnatch_sha-512_ell2_pedersen.json")) as f:
        vs = json.load(f)
    return [item(0, [(bytes.fromhex(v["h"]), bytes.fromhex(v["gamma"]))], bytes.fromhex(v["ad"]),
                 bytes.fromhex(v["proof_pk_com"] + v["proof_r"] + v["proof_ok"] + v["proof_s"] + v["proof_sb"])) for v in vs]


_GEN = {}


def gen_items(suite, n):
    """orc.gen_batch's one-pair Pedersen items as item dicts (C-ABI pieces only)"""
    if (suite, n) not in _GEN:
        b = orc.gen_batch(suite, 1, n)
        off = [0]
        for ln in b["ad_lens"]:
            off.append(off[-1] + ln)
        _GEN[suite, n] = [dict(ios=[b["ios_xy"][128 * j: 128 * j + 128]], ad=b["ads"][off[j]: off[j + 1]], proof=b["proofs"][256 * j: 256 * j + 256])
                          for j in range(n)]
    return list(_GEN[suite, n])


def batch_dict(items):
    """items -> a gen_batch-style dict in the C-ABI (xy) layout"""
    return dict(n=len(items), pks_xy=b"", ios_xy=b"".join(p for it in items for p in it["ios"]),
                io_counts=[len(it["ios"]) for it in items], ads=b"".join(it["ad"] for it in items), ad_lens=[len(it["ad"]) for it in items],
                proofs=b"".join(it["proof"] for it in items), sks=b"")


def wire_batch(items):
    from ark_vrf_amd._native import Batch
    return Batch(len(items), b"".join(p for it in items for p in it["w_ios"]), [len(it["ios"]) for it in items], b"".join(it["ad"] for it in items),
                 [len(it["ad"]) for it in items], proofs=b"".join(it["w_proof"] for it in items))


def slices(items, segs):
    out, at = [], 0
    for k in segs:
        out.append(items[at: at + k]); at += k
    assert at == len(items)
    return out


def flip(data, at):
    return data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]


def tamper(it, which):
    """the lowest bit of s (which = 0) or of sb (1), in the x || y proof and in the wire proof (the responses are its last 64 bytes)"""
    w = it.get("w_proof", b"")
    return dict(it, proof=flip(it["proof"], 192 + 32 * which), w_proof=flip(w, len(w) - 64 + 32 * which) if w else w)


def oracle_segment(suite, seg):
    """(status, bases, scalars) of the segment's items as a batch of their own; nothing for an empty segment (src/pedersen.rs:343-345)"""
    if not seg:
        return 0, b"", b""
    b = batch_dict(seg)
    st, bases, sc = orc.pedersen_batch_terms_xy(suite, b)
    return (orc.pedersen_batch_verify_xy(suite, b) if st == 0 else st), bases, sc


def alone(c, seg):
    """avrf_pedersen_batch_verify of the segment on its own"""
    assert c.pedersen_batch_stage(nat_batch(batch_dict(seg))) == 0
    return c.pedersen_batch_run()


def check_run(c, suite, items, segs):
    """stage, run the segments, compare every status and every segment's terms with the oracle on the segment alone; -> statuses"""
    assert c.pedersen_batch_stage(nat_batch(batch_dict(items))) == 0
    got = c.pedersen_batch_run_segments(segs)
    assert isinstance(got, list) and len(got) == len(segs), got
    for v, seg in enumerate(slices(items, segs)):
        st, bases, sc = oracle_segment(suite, seg)
        assert got[v] == st, (v, got, st)
        if st != 2:
            gb, gs = c.pedersen_segment_terms(v)
            assert len(gs) == 32 * (5 * len(seg) + 2 if seg else 0)
            assert gs == sc and gb == bases, v
    return got


@pytest.fixture(scope="module")
def nine(golden_dir):
    """261 verifying items of suite 0 in nine segments; the 7-item one is the reference's Pedersen vectors, the others have 0 to 3 pairs
    (no pair: an identity base under a non-zero scalar; two and more: the merged pair)"""
    rng = random.Random(5)
    counts = [rng.choice([0, 1, 1, 2, 3]) for _ in range(sum(SEGS9) - 7)]
    assert {0, 1, 2, 3} <= set(counts)
    made = made_items(0, counts, 9)
    return made[:11] + golden_items(golden_dir) + made[11:]


# ---------------------------------------------------------------- verdicts and terms

def test_nine_segments(ctxs, nine):
    c = ctxs[0]
    assert check_run(c, 0, nine, SEGS9) == [0] * 9
    assert c.pedersen_segments_layout(261, SEGS9)[0] == 652
    # every status is what avrf_pedersen_batch_verify answers for the segment on its own
    for seg in slices(nine, SEGS9):
        assert alone(c, seg) == 0


def test_tampered_and_invalid_segments(ctxs, nine):
    """a tampered s in the 3-item segment and a tampered sb in the 64-item one: exactly those two fail (sb reaches only the B term: the
    second base term sits in its slot); the identity Yb in the 5-item segment: that one is InvalidData and nothing else moves"""
    c = ctxs[0]
    bad = list(nine)
    bad[1 + 2 + 1] = tamper(bad[1 + 2 + 1], 0)
    j64 = sum(SEGS9[:7]) + 40
    bad[j64] = tamper(bad[j64], 1)
    assert check_run(c, 0, bad, SEGS9) == [0, 0, 1, 0, 0, 0, 0, 1, 0]
    j5 = 1 + 2 + 3 + 2
    bad[j5] = dict(bad[j5], proof=IDENTITY_XY + bad[j5]["proof"][64:])
    got = check_run(c, 0, bad, SEGS9)
    assert got == [0, 0, 1, 2, 0, 0, 0, 1, 0]
    for st, seg in zip(got, slices(bad, SEGS9)):
        assert alone(c, seg) == st
    # the one-call form
    assert c.pedersen_batch_verify_segments(nat_batch(batch_dict(bad)), SEGS9) == got


def one_pair_item(items, lo, hi):
    return next(j for j in range(lo, hi) if len(items[j]["ios"]) == 1)


@pytest.mark.parametrize("what", ["io_identity", "s_ge_r", "sb_ge_r", "r_noncanonical"])
def test_invalid_inputs_mark_their_own_segment(ctxs, nine, what):
    """an identity supplied I/O point, s >= r, sb >= r, a non-canonical R coordinate: each marks ITS segment InvalidData and no other"""
    c = ctxs[0]
    r_bytes = R_ORDER[0].to_bytes(32, "little")
    v = {"io_identity": 5, "s_ge_r": 0, "sb_ge_r": 8, "r_noncanonical": 6}[what]
    lo = sum(SEGS9[:v])
    worse = list(nine)
    if what == "io_identity":
        j = one_pair_item(nine, lo, lo + SEGS9[v])
        worse[j] = dict(worse[j], ios=[IDENTITY_XY + worse[j]["ios"][0][64:]])
    else:
        j = lo + SEGS9[v] - 1
        p = worse[j]["proof"]
        p = {"s_ge_r": p[:192] + r_bytes + p[224:], "sb_ge_r": p[:224] + r_bytes, "r_noncanonical": p[:64] + Q0.to_bytes(32, "little") + p[96:]}[what]
        worse[j] = dict(worse[j], proof=p)
    assert c.pedersen_batch_stage(nat_batch(batch_dict(worse))) == 0
    got = c.pedersen_batch_run_segments(SEGS9)
    assert got == [2 if u == v else 0 for u in range(9)]
    for st, seg in zip(got, slices(worse, SEGS9)):
        assert alone(c, seg) == st
    if what == "io_identity":                                                    # (an encoding the oracle's typed points can hold)
        assert oracle_segment(0, slices(worse, SEGS9)[v])[0] == 2


@pytest.mark.parametrize("segs", [[11, 7, 243], [1, 2, 3, 5, 0, 7, 16, 33, 64, 130], [0, 261, 0]])
def test_other_segmentations(ctxs, nine, segs):
    """three segments take the route below eight (one MSM per segment); an empty segment in the middle is Ok and has no terms"""
    c = ctxs[0]
    assert check_run(c, 0, nine, segs) == [0] * len(segs)
    bad = list(nine)
    bad[12] = tamper(bad[12], 1)
    want = [int(12 in range(sum(segs[:v]), sum(segs[:v + 1]))) for v in range(len(segs))]
    assert check_run(c, 0, bad, segs) == want
    for v, k in enumerate(segs):
        if not k:
            assert c.pedersen_segment_terms(v) == (b"", b"")


# ---------------------------------------------------------------- locate

def test_locate_in_3000(ctxs):
    c = ctxs[0]
    bad = gen_items(0, 3000)
    bad[777] = tamper(bad[777], 0)
    bad[2990] = tamper(bad[2990], 1)
    b = nat_batch(batch_dict(bad))
    segs = [64] * 46 + [56]
    assert c.pedersen_batch_stage(b) == 0 and c.pedersen_batch_run() == 1
    st_o, bases, sc = orc.pedersen_batch_terms_xy(0, batch_dict(bad))
    assert st_o == 0 and c.last_terms() == (bases, sc)
    got = c.pedersen_batch_run_segments(segs)
    assert [v for v, st in enumerate(got) if st] == [777 // 64, 2990 // 64] and set(got) == {0, 1}
    # a plain run on the same staging keeps its verdict and its terms
    assert c.pedersen_batch_run() == 1 and c.last_terms() == (bases, sc)
    assert c.pedersen_batch_run_segments(segs) == got
    assert c.pedersen_batch_run() == 1 and c.last_terms() == (bases, sc)
    # the per-item call's statuses, folded per segment
    each = c.pedersen_verify(b)
    assert [j for j, st in enumerate(each) if st] == [777, 2990]
    assert [max(s) for s in slices(each, segs)] == got


# ---------------------------------------------------------------- other stagings and suites

@pytest.mark.parametrize("validate", [0, 1])
def test_wire_staging(ctxs, nine, validate):
    """validate 1 decodes with Validate::Yes, which refuses the identity at staging (avrf_pedersen_batch_stage_wire, as for a plain
    batch), and the Ok of an item without pairs is the identity: that level runs on the items that have a pair"""
    from ark_vrf_amd import _native as nat
    c = ctxs[0]
    good = list(nine) if validate == 0 else [it for it in nine if it["ios"]]
    segs = SEGS9[:8] + [len(good) - sum(SEGS9[:8])]
    assert segs[8] > 0 and (validate or segs == SEGS9)
    bad = list(good)
    bad[30] = tamper(bad[30], 1)
    want = [0, 0, 0, 0, 0, 1, 0, 0, 0]
    wb = wire_batch(bad)
    assert nat.lib().avrf_pedersen_batch_stage_wire(c._h, C.c_size_t(wb.n), wb.ios_xy, wb.io_counts, wb.ads, wb.ad_lens, wb.proofs, validate) == 0
    assert c.pedersen_batch_run_segments(segs) == want
    for v, seg in enumerate(slices(bad, segs)):
        assert c.pedersen_segment_terms(v) == oracle_segment(0, seg)[1:], v
    assert c.pedersen_batch_verify_segments_wire(wire_batch(good), segs, validate) == [0] * 9
    assert c.pedersen_batch_verify_segments_wire(wb, segs, validate) == want
    assert c.pedersen_batch_verify_segments(nat_batch(batch_dict(bad)), segs) == want


@pytest.mark.parametrize("suite", [orc.BABYJUBJUB, orc.BANDERSNATCH_SHAKE128, orc.BANDERSNATCH_SW])
def test_other_suites(ctxs, suite):
    """Baby-JubJub; the SHAKE128 suite, whose 32-byte weights the host squeezes per segment; Bandersnatch-SW, whose prepare kernel absorbs
    the 33-byte forms"""
    c = ctxs[suite]
    items = gen_items(suite, 32)
    assert check_run(c, suite, items, [4] * 8) == [0] * 8
    bad = list(items)
    bad[22] = tamper(bad[22], 1)
    assert check_run(c, suite, bad, [4] * 8) == [0, 0, 0, 0, 0, 1, 0, 0]
    assert check_run(c, suite, bad, [10, 12, 10]) == [0, 0, 1]
    for st, seg in zip([0, 0, 1], slices(bad, [10, 12, 10])):
        assert alone(c, seg) == st


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
        assert c.pedersen_batch_stage(nat_batch(batch_dict(bad))) == 0
        assert c.pedersen_batch_run() == 2
        assert c.pedersen_batch_run_segments([4] * 8) == [0, 0, 0, 2, 0, 0, 0, 0]
        assert c.pedersen_batch_run_segments([10, 12, 10]) == [0, 2, 0]
        assert c.pedersen_batch_stage(nat_batch(batch_dict(items))) == 0 and c.pedersen_batch_run_segments([4] * 8) == [0] * 8
    finally:
        c.close()


# ---------------------------------------------------------------- refusals

def test_refusals(ctxs):
    from ark_vrf_amd import _native as nat
    c = nat.Context(0)
    try:
        assert c.pedersen_batch_run_segments([1]) == BAD_ARG                   # nothing staged
        bad = gen_items(0, 40)
        bad[5] = tamper(bad[5], 0)
        assert c.pedersen_batch_stage(nat_batch(batch_dict(bad))) == 0 and c.pedersen_batch_run() == 1
        assert c.pedersen_batch_run_segments([20, 19]) == BAD_ARG              # counts that do not sum to n
        assert c.pedersen_batch_run_segments([20, 21]) == BAD_ARG
        assert c.pedersen_batch_run_segments([1] * 40) == [0] * 5 + [1] + [0] * 34
        assert c.batch_run_begin() == 0
        assert c.pedersen_batch_run_segments([20, 20]) == BAD_ARG              # between avrf_batch_run_begin and _end
        assert c.batch_run_hash() == 0 and c.batch_run_end() == 1              # the run is undisturbed
        assert c.pedersen_batch_run_segments([20, 20]) == [1, 0] and c.pedersen_batch_run() == 1
        # with a Pedersen staging the Thin call is still refused, and the staging is untouched
        assert c.thin_batch_run_segments([20, 20]) == BAD_ARG and c.thin_segment_terms(0) == (b"", b"")
        assert c.pedersen_batch_run() == 1
        # a limit exceeded: one segment of 1 638 items is 8 192 terms
        big = gen_items(0, 1638)
        assert c.pedersen_batch_stage(nat_batch(batch_dict(big))) == 0
        assert c.pedersen_batch_run_segments([1638]) == BAD_ARG and c.pedersen_batch_run() == 0
        assert c.pedersen_segment_terms(0) == (b"", b"")                       # no segmented run on this staging
        assert c.pedersen_batch_run_segments([1637, 1]) == [0, 0]              # the longest segment there is: 8 187 terms
        # a Thin batch
        tb = orc.gen_batch(0, 0, 8)
        assert c.thin_batch_stage(nat_batch(tb)) == 0
        assert c.pedersen_batch_run_segments([4, 4]) == BAD_ARG and c.pedersen_segment_terms(0) == (b"", b"") and c.thin_batch_run() == 0
        # the empty batch: every (empty) segment is Ok
        assert c.pedersen_batch_stage(nat_batch(orc.gen_batch(0, 1, 0))) == 0
        assert c.pedersen_batch_run_segments([0, 0]) == [0, 0] and c.pedersen_batch_run_segments([]) == [] and c.pedersen_batch_run_segments([1]) == BAD_ARG
    finally:
        c.close()
