"""GPU parity: one verdict per segment of a Thin batch staged over a table of shared points (include/avrf.h
avrf_thin_batch_run_shared_segments) against the CPU oracle.

Every expectation is the oracle on ONE SEGMENT'S EXPANDED ITEMS ALONE (orc.thin_batch_terms_xy, orc.thin_batch_verify_xy), folded in
Python into the layout the run must have chosen (shared_segments_helpers): the merged layout -- item terms, the T row terms with the
segment's own key and input scalars added mod r, the generator term -- or the plain segmented layout.  Terms are compared bit for bit,
statuses as integers; nothing has a tolerance.  Oracle results are computed once per module and shared."""
import json
import os

import pytest

import oracle as orc
import ped_shared_helpers as ph
import shared_segments_helpers as sh
from helpers import IDENTITY_XY, nat_batch, xy

pytestmark = pytest.mark.gpu

NAMES = {0: "bandersnatch_sha-512_ell2", 1: "baby-jubjub_sha-512_tai"}
Q0 = ph.Q[0]
SEGS9 = [1, 0, 7, 16, 33, 40, 3, 29, 1]            # 130 items: an empty segment, one-item segments, items 100 .. 128 across the 128-lane block boundary
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


@pytest.fixture(scope="module")
def b130():
    """130 verifying items of suite 0 with 1 or 3 pairs over T = 5 rows; item 60 has key 0 and row 0 as its input (segment 5)"""
    counts = [3 if j % 9 == 4 else 1 for j in range(130)]
    sb = sh.thin_real_batch(0, counts)
    assert sb["pk_index"][60] == 0 and 0 in sb["input_index"]
    return sb


@pytest.fixture(scope="module")
def material():
    """3 100 one-pair items of the oracle's synthetic batch: points, outputs, proofs (R, s < r) and additional data for term comparisons"""
    b = orc.gen_batch(0, 0, 3100)
    off = [0]
    for ln in b["ad_lens"]:
        off.append(off[-1] + ln)
    return dict(pts=[b["pks_xy"][64 * j: 64 * j + 64] for j in range(3100)], outs=[b["ios_xy"][128 * j + 64: 128 * j + 128] for j in range(3100)],
                ads=[b["ads"][off[j]: off[j + 1]] for j in range(3100)], proofs=[b["proofs"][96 * j: 96 * j + 96] for j in range(3100)])


def synthetic(material, rows, pk_index, input_index):
    n = len(pk_index)
    return dict(n=n, rows=list(rows), pk_index=list(pk_index), input_index=list(input_index), outputs=material["outs"][:n], io_counts=[1] * n,
                ads=material["ads"][:n], proofs=material["proofs"][:n])


def tampered(sb, j):
    pr = list(sb["proofs"])
    pr[j] = pr[j][:64] + bytes([pr[j][64] ^ 1]) + pr[j][65:]
    return dict(sb, proofs=pr)


# ---------------------------------------------------------------- both layouts against the oracle

def test_nine_segments_merged(ctxs, b130):
    """T = 5 < 40 items + pairs: the merged layout, nine segments in one chain; row 0 is a key and an input inside segment 5, and the
    one-item segments leave three or four rows unreferenced"""
    got = sh.check_segments(ctxs[0], 0, b130, SEGS9, 1, key="b130")
    assert got == [0] * 9
    subs = sh.sub_batches(b130, SEGS9)
    assert 0 in subs[5]["pk_index"] and 0 in subs[5]["input_index"]
    _, gs = ctxs[0].thin_segment_terms(0)                                      # one item, one pair: R, O, five rows, G
    assert len(gs) == 32 * 8 and sum(gs[32 * (2 + r): 32 * (3 + r)] == bytes(32) for r in range(5)) in (3, 4)


def test_three_segments_single_msms(ctxs, b130):
    assert sh.check_segments(ctxs[0], 0, b130, [50, 0, 80], 1, key="b130") == [0, 0, 0]


def test_mode_switch_on_one_staging(ctxs, b130):
    """the same staging: one segment of everything is merged, one segment per item (at most 1 + 3 < T + 1 terms) is expanded"""
    c = ctxs[0]
    assert sh.check_segments(c, 0, b130, [130], 1, key="b130") == [0]
    assert sh.check_segments(c, 0, b130, [1] * 130, 0, key="b130", staged=True) == [0] * 130
    assert sh.check_segments(c, 0, b130, SEGS9, 1, key="b130", staged=True) == [0] * 9


def test_tampered_proof_fails_its_segment_only(ctxs, b130):
    bad = tampered(b130, 30)                                                    # segment 4 holds items 24 .. 56
    assert sh.check_segments(ctxs[0], 0, bad, SEGS9, 1) == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert sh.check_segments(ctxs[0], 0, bad, [1] * 130, 0) == [0] * 30 + [1] + [0] * 99


@pytest.mark.parametrize("T", [2, 12])
def test_run_lengths_around_the_share(ctxs, material, T):
    """(segment, row) runs of 7, 8, 9 and 17 contributions each for the key row 0 and the input row 1 (SHARED_SHARE = 8): runs inside a lane,
    cut at one end and at both; T = 2 is 8 virtual rows for 11 lanes (a unit of k_shared_merge is a row), T = 12 is 48 (a unit is a lane)"""
    segs = [7, 8, 9, 17]
    n = sum(segs)
    sb = synthetic(material, material["pts"][:T], [0] * n, [1] * n)
    assert (len(segs) * T <= (2 * n + 7) // 8) == (T == 2)
    sh.check_segments(ctxs[0], 0, sb, segs, 1)


def test_one_row_of_6200_contributions(ctxs, material):
    """one segment of 3 100 one-pair items whose key and input are the same row: its 6 200 contributions span 775 lanes, the four-loads loop
    of k_shared_merge; the proofs belong to other keys, the status is the oracle's"""
    sb = synthetic(material, material["pts"][:1], [0] * 3100, [0] * 3100)
    got = sh.check_segments(ctxs[0], 0, sb, [3100], 1)
    assert got in ([0], [1])


def test_host_squeezed_suite(ctxs):
    """suite 5 takes its weights from the host's sponge stream, segment by segment"""
    sb = sh.thin_real_batch(5, [1, 3, 1, 1, 1, 3, 1, 1, 1, 1, 1, 3, 1, 1, 1, 1, 1, 1, 1, 1])
    segs = [1, 0, 2, 3, 1, 4, 2, 6, 1]
    assert sh.check_segments(ctxs[5], 5, sb, segs, 1) == [0] * 9               # T = 5 < 6 + 6
    assert sh.check_segments(ctxs[5], 5, tampered(sb, 4), segs, 1) == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert sh.check_segments(ctxs[5], 5, sb, [1] * 20, 0) == [0] * 20


@pytest.mark.parametrize("suite", [0, 1])
def test_reference_vectors(ctxs, golden_dir, suite):
    """the reference's seven Thin vectors as one shared batch over their 14 points, cut into segments"""
    with open(os.path.join(golden_dir, NAMES[suite] + "_thin.json")) as f:
        vs = json.load(f)
    L = orc.pt_len(suite)
    proofs = [bytes.fromhex(v["proof_r"] + v["proof_s"]) for v in vs]
    sb = dict(n=7, rows=[xy(suite, bytes.fromhex(v["pk"])) for v in vs] + [xy(suite, bytes.fromhex(v["h"])) for v in vs], pk_index=list(range(7)),
              input_index=list(range(7, 14)), outputs=[xy(suite, bytes.fromhex(v["gamma"])) for v in vs], io_counts=[1] * 7,
              ads=[bytes.fromhex(v["ad"]) for v in vs], proofs=[xy(suite, p[:L]) + p[L:] for p in proofs])
    assert sh.check_segments(ctxs[suite], suite, sb, [3, 0, 4], 0) == [0, 0, 0]  # 14 rows are no fewer than 4 + 4: expanded
    dup = dict(sb, n=14, pk_index=sb["pk_index"] * 2, input_index=sb["input_index"] * 2, outputs=sb["outputs"] * 2, io_counts=[1] * 14,
               ads=sb["ads"] * 2, proofs=sb["proofs"] * 2)
    assert sh.check_segments(ctxs[suite], suite, dup, [10, 4], 1) == [0, 0]       # every vector twice: 14 < 10 + 10, merged
    assert sh.check_segments(ctxs[suite], suite, tampered(dup, 12), [10, 4], 1) == [0, 1]


# ---------------------------------------------------------------- defects

def expect_marked(sb, segs, r):
    marked = sh.segments_referencing(sb, segs, r)
    return [2 if v in marked else 0 for v in range(len(segs))]


def test_identity_row_marks_the_segments_that_reference_it(ctxs, b130):
    c = ctxs[0]
    segs = [1, 1, 1, 1, 126]
    rows = list(b130["rows"]); rows[4] = IDENTITY_XY
    want = expect_marked(b130, segs, 4)
    assert 0 in want[:4] and 2 in want
    bad = sh.with_rows(b130, rows)
    assert sh.check_segments(c, 0, bad, segs, 1) == want                       # (the oracle refuses exactly these: src/thin.rs:266-271)
    spare = sh.with_rows(b130, b130["rows"] + [IDENTITY_XY])                   # an identity row nothing refers to
    assert sh.check_segments(c, 0, spare, SEGS9, 1) == [0] * 9


def test_non_canonical_row(ctxs, b130):
    c = ctxs[0]
    segs = [1, 1, 1, 1, 126]
    for r in (1, 3):                                                           # a key row, an input row
        row = b130["rows"][r]
        x = int.from_bytes(row[:32], "little")
        assert x + Q0 < 1 << 256
        rows = list(b130["rows"]); rows[r] = (x + Q0).to_bytes(32, "little") + row[32:]
        want = expect_marked(b130, segs, r)
        assert 0 in want[:4] and 2 in want
        assert sh.stage(c, sh.with_rows(b130, rows)) == 0
        assert sh.run(c, b130, segs) == want                                   # unreferenced in v: v's status is left alone
        assert c.thin_batch_run() == 2                                         # (the plain run refuses a non-canonical coordinate in any row)
        assert sh.run(c, b130, [1] * 130) == expect_marked(b130, [1] * 130, r)      # the expanded layout, one segment per item
    lifted = (int.from_bytes(b130["rows"][0][:32], "little") + Q0).to_bytes(32, "little") + b130["rows"][0][32:]
    assert sh.stage(c, sh.with_rows(b130, b130["rows"] + [lifted])) == 0       # a non-canonical row nothing refers to
    assert sh.run(c, b130, SEGS9) == [0] * 9 and c.thin_batch_run() == 2


def test_validation_level_2_torsion_row(b130):
    from ark_vrf_amd import _native as nat
    segs = [1, 1, 1, 1, 126]
    c = nat.Context(0)
    try:
        c.set_validation(2)
        assert sh.check_segments(c, 0, b130, SEGS9, 1, key="b130") == [0] * 9
        for r in (2, 4):
            rows = list(b130["rows"]); rows[r] = ph.torsion(0, rows[r])
            want = expect_marked(b130, segs, r)
            assert 0 in want[:4] and 2 in want
            assert sh.stage(c, sh.with_rows(b130, rows)) == 0 and sh.run(c, b130, segs) == want
        assert sh.stage(c, sh.with_rows(b130, b130["rows"] + [ph.torsion(0, b130["rows"][0])])) == 0    # validated, referenced by nothing
        assert sh.run(c, b130, SEGS9) == [0] * 9
        outs = list(b130["outputs"]); outs[0] = ph.torsion(0, outs[0])
        assert sh.stage(c, dict(b130, outputs=outs)) == 0 and sh.run(c, b130, segs) == [2, 0, 0, 0, 0]
    finally:
        c.close()


# ---------------------------------------------------------------- wire

def nat_wire(suite, sb):
    from ark_vrf_amd._native import SharedWireBatch
    L = ph.point_len(suite)
    return SharedWireBatch(sb["n"], b"".join(ph.comp(suite, r) for r in sb["rows"]), sb["pk_index"], sb["input_index"],
                           b"".join(ph.comp(suite, o) for o in sb["outputs"]), sb["io_counts"], b"".join(sb["ads"]), [len(a) for a in sb["ads"]],
                           b"".join(ph.comp(suite, p[:64]) + p[64:] for p in sb["proofs"]), L)


def test_wire_entry_point(ctxs, b130):
    c = ctxs[0]
    bad = tampered(b130, 30)
    assert c.thin_batch_verify_shared_segments_wire(nat_wire(0, bad), SEGS9, validate=1) == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    sub = sh.sub_batches(bad, SEGS9)[4]
    _, bases, sc = sh.oracle_segment(0, sub)
    assert c.thin_segment_terms(4) == sh.fold_thin(0, sub, bases, sc)           # the same terms as from x || y
    assert c.thin_batch_stage_shared_wire(nat_wire(0, b130), validate=1) == 0
    assert c.thin_batch_run_shared_segments([1] * 130) == [0] * 130
    # a row that does not decode: the call returns INVALID_DATA and writes no status
    wb = nat_wire(0, b130)
    raw = bytearray(bytes(wb.shared_xy))
    for y in range(2, 40):                                                     # a y with no x on the curve
        raw[32: 64] = y.to_bytes(32, "little")
        if orc.point_decompress(0, bytes(raw[32: 64]))[0] != 0:
            break
    else:
        pytest.fail("no undecodable y found")
    import ctypes as C
    wb.shared_xy = (C.c_uint8 * len(raw)).from_buffer_copy(bytes(raw))
    assert c.thin_batch_verify_shared_segments_wire(wb, SEGS9, validate=0) == 2


# ---------------------------------------------------------------- other stagings, other states

def test_plain_staging_equals_the_existing_call(ctxs, b130):
    c = ctxs[0]
    assert c.thin_batch_stage(nat_batch(sh.expanded(tampered(b130, 30)))) == 0
    old = c.thin_batch_run_segments(SEGS9)
    old_terms = [c.thin_segment_terms(v) for v in range(9)]
    assert old == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert c.thin_batch_run_shared_segments(SEGS9) == old
    assert [c.thin_segment_terms(v) for v in range(9)] == old_terms


def test_state_afterwards_and_refusals(ctxs, b130):
    c = ctxs[0]
    assert sh.stage(c, b130) == 0
    assert c.thin_batch_run() == 0
    usual = c.last_terms()
    assert c.thin_batch_run_segments(SEGS9) == BAD_ARG                          # the existing call still refuses a shared staging
    assert c.thin_batch_run_shared_segments(SEGS9) == [0] * 9
    assert c.last_terms() == usual and c.thin_batch_run() == 0 and c.last_terms() == usual
    t = c.last_timing()
    assert c.thin_batch_run_shared_segments(SEGS9) == [0] * 9
    t = c.last_timing()
    assert t[0] > 0 and t[5] == 0 and all(x >= 0 for x in t[1:5])
    # refusals leave the staging usable
    assert c.thin_batch_run_shared_segments([100, 29]) == BAD_ARG and c.thin_batch_run_shared_segments([100, 31]) == BAD_ARG
    assert c.pedersen_batch_run_shared_segments(SEGS9) == BAD_ARG               # a staging of the other kind
    assert c.batch_run_begin() == 0
    assert c.thin_batch_run_shared_segments(SEGS9) == BAD_ARG                   # busy: between avrf_batch_run_begin and _end
    assert c.batch_run_hash() == 0
    assert c.thin_batch_run_shared_segments(SEGS9) == BAD_ARG
    assert c.batch_run_end() == 0
    assert c.thin_batch_run_shared_segments(SEGS9) == [0] * 9
    assert c.thin_segment_terms(9) == (b"", b"")
    from ark_vrf_amd import _native as nat
    fresh = nat.Context(0)
    try:
        assert fresh.thin_batch_run_shared_segments([1]) == BAD_ARG             # nothing staged
    finally:
        fresh.close()


def test_repeatability(ctxs, b130):
    c = ctxs[0]
    assert sh.stage(c, b130) == 0
    runs = []
    for _ in range(2):
        st = c.thin_batch_run_shared_segments(SEGS9)
        runs.append((st, [c.thin_segment_terms(v) for v in range(9)]))
    assert runs[0] == runs[1]                                                   # (the atomics' order may differ: sums in Fr are exact)
