"""GPU parity: one verdict per segment of a Pedersen batch staged over a table of shared inputs (include/avrf.h
avrf_pedersen_batch_run_shared_segments) against the CPU oracle.

Every expectation is the oracle on ONE SEGMENT'S EXPANDED ITEMS ALONE (orc.pedersen_batch_terms_xy, orc.pedersen_batch_verify_xy).  In the
merged layout a segment's terms are the shared layout of a batch of just its items, so ped_shared_helpers.check_terms folds them: the
item terms, the two base terms, the row bases and the row scalars of at-most-one-pair segments bit for bit, the row block of a segment
with a multi-pair item as a group element (the oracle has no z_i).  In the expanded layout the terms are the oracle's as they are.
Statuses are integers; nothing has a tolerance."""
import json
import os

import pytest

import oracle as orc
import ped_shared_helpers as ph
import shared_segments_helpers as sh
from helpers import IDENTITY_XY, nat_batch, xy

pytestmark = pytest.mark.gpu

NAMES = {0: "bandersnatch_sha-512_ell2", 1: "baby-jubjub_sha-512_tai"}
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
    """130 verifying items of suite 0 with 0, 1 or 3 pairs over T = 3 inputs; items 0 .. 7 have one pair each"""
    return ph.real_batch(0, [1] * 8 + [(1, 1, 3, 1, 0, 1, 1)[j % 7] for j in range(122)], 3)


def one_pair_tail(sb):
    """the last 33 + 40 + 3 + 29 + 1 items do have multi-pair items; a batch of one-pair items for the bit-exact row scalars"""
    return ph.real_batch(0, [1] * 130, 3, seed=2)


# ---------------------------------------------------------------- both layouts against the oracle

def test_nine_segments_merged(ctxs, b130):
    """T = 3 < 40 items: the merged layout, nine segments in one chain; the one-item segments leave two rows unreferenced"""
    assert sh.check_segments(ctxs[0], 0, b130, SEGS9, 1, key="b130") == [0] * 9
    _, gs = ctxs[0].pedersen_segment_terms(0)                                   # one item: four terms, three rows, G, B
    assert len(gs) == 32 * 9 and sum(gs[32 * (4 + r): 32 * (5 + r)] == bytes(32) for r in range(3)) == 2


def test_one_pair_items_row_scalars_bit_exact(ctxs):
    sb = one_pair_tail(None)
    assert sh.check_segments(ctxs[0], 0, sb, SEGS9, 1) == [0] * 9
    assert sh.check_segments(ctxs[0], 0, sb, [50, 0, 80], 1, staged=True) == [0, 0, 0]     # fewer than eight segments: single MSMs


def test_mode_switch_on_one_staging(ctxs, b130):
    """the same staging: one segment of everything is merged; segments of at most three items (T = 3) are expanded, which needs the
    merged INPUT the shared prepare does not compute"""
    c = ctxs[0]
    assert sh.check_segments(c, 0, b130, [130], 1, key="b130") == [0]
    small = [3] * 43 + [1]
    assert sh.check_segments(c, 0, b130, small, 0, key="b130", staged=True) == [0] * 44
    assert sh.check_segments(c, 0, b130, SEGS9, 1, key="b130", staged=True) == [0] * 9
    assert c.pedersen_batch_run() == 0                                          # the plain shared run prepares for itself again
    ph.check_terms(0, b130, c.last_terms())


def test_tampered_proof_fails_its_segment_only(ctxs, b130):
    bad = ph.tampered(b130, 30)                                                 # segment 4 holds items 24 .. 56
    assert sh.check_segments(ctxs[0], 0, bad, SEGS9, 1) == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert sh.check_segments(ctxs[0], 0, ph.tampered(b130, 129, at=224), [3] * 43 + [1], 0) == [0] * 43 + [1]


@pytest.mark.parametrize("T", [1, 9])
def test_run_lengths_around_the_share(ctxs, T):
    """(segment, row) runs of 7, 8, 9 and 17 contributions of one-pair items that all name row 0 (SHARED_SHARE = 8): inside a lane, cut at
    one end, cut at both; T = 1 is 4 virtual rows for 6 lanes (a unit of k_shared_merge is a row), T = 9 is 36 (a unit is a lane)"""
    segs = [7, 8, 9, 17]
    base = ph.real_batch(0, [1] * 41, 1, seed=3)
    sb = sh.with_rows(base, base["rows"] + [ph.real_batch(0, [1] * 130, 3, seed=2)["rows"][r % 3] for r in range(T - 1)])
    assert (len(segs) * T <= (41 + 7) // 8) == (T == 1)
    assert sh.check_segments(ctxs[0], 0, sb, segs, 1) == [0] * 4


def test_host_squeezed_suite(ctxs):
    """suite 5 takes its weights (t, u: 32 bytes per item) from the host's sponge stream, segment by segment"""
    sb = ph.real_batch(5, [1, 3, 1, 0, 1, 1, 1, 1, 1, 1, 1, 3, 1, 1, 1, 1, 1, 1, 1, 1], 3)
    segs = [1, 0, 2, 3, 1, 4, 2, 6, 1]
    assert sh.check_segments(ctxs[5], 5, sb, segs, 1) == [0] * 9               # T = 3 < 6
    assert sh.check_segments(ctxs[5], 5, ph.tampered(sb, 4), segs, 1) == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert sh.check_segments(ctxs[5], 5, sb, [2] * 10, 0) == [0] * 10


@pytest.mark.parametrize("suite", [0, 1])
def test_reference_vectors(ctxs, golden_dir, suite):
    """the reference's Pedersen vectors as one shared batch over their inputs, cut into segments"""
    with open(os.path.join(golden_dir, NAMES[suite] + "_pedersen.json")) as f:
        vs = json.load(f)
    L = orc.pt_len(suite)
    proofs = [bytes.fromhex(v["proof_pk_com"] + v["proof_r"] + v["proof_ok"] + v["proof_s"] + v["proof_sb"]) for v in vs]
    n = len(vs)
    sb = ph.shared([xy(suite, bytes.fromhex(v["h"])) for v in vs], range(n), [xy(suite, bytes.fromhex(v["gamma"])) for v in vs], [1] * n,
                   [bytes.fromhex(v["ad"]) for v in vs], [b"".join(xy(suite, p[L * k: L * k + L]) for k in range(3)) + p[3 * L:] for p in proofs])
    assert sh.check_segments(ctxs[suite], suite, sb, [3, 0, n - 3], 0) == [0, 0, 0]          # n rows are no fewer than the items: expanded
    dup = ph.shared(sb["rows"], list(range(n)) * 2, sb["outputs"] * 2, [1] * (2 * n), sb["ads"] * 2, sb["proofs"] * 2)
    assert sh.check_segments(ctxs[suite], suite, dup, [n + 3, n - 3], 1) == [0, 0]           # every vector twice: n < n + 3, merged
    assert sh.check_segments(ctxs[suite], suite, ph.tampered(dup, 2 * n - 1), [n + 3, n - 3], 1) == [0, 1]


# ---------------------------------------------------------------- defects

def expect_marked(sb, segs, r):
    marked = sh.segments_referencing(sb, segs, r)
    return [2 if v in marked else 0 for v in range(len(segs))]


SEGS_FEW = [1, 1, 1, 1, 4, 122]


def test_identity_row_marks_the_segments_that_reference_it(ctxs, b130):
    c = ctxs[0]
    rows = list(b130["rows"]); rows[2] = IDENTITY_XY
    want = expect_marked(b130, SEGS_FEW, 2)
    assert 0 in want and 2 in want
    assert sh.check_segments(c, 0, sh.with_rows(b130, rows), SEGS_FEW, 1) == want           # (the oracle refuses exactly these: src/pedersen.rs:278)
    assert sh.check_segments(c, 0, sh.with_rows(b130, b130["rows"] + [IDENTITY_XY]), SEGS9, 1) == [0] * 9


def test_non_canonical_row(ctxs, b130):
    c = ctxs[0]
    row = b130["rows"][1]
    x = int.from_bytes(row[:32], "little")
    assert x + ph.Q[0] < 1 << 256
    rows = list(b130["rows"]); rows[1] = (x + ph.Q[0]).to_bytes(32, "little") + row[32:]
    want = expect_marked(b130, SEGS_FEW, 1)
    assert 0 in want and 2 in want
    assert sh.stage(c, sh.with_rows(b130, rows)) == 0
    assert sh.run(c, b130, SEGS_FEW) == want                                    # unreferenced in v: v's status is left alone
    assert c.pedersen_batch_run() == 2                                          # (the plain run refuses a non-canonical coordinate in any row)
    small = [3] * 43 + [1]
    assert sh.run(c, b130, small) == expect_marked(b130, small, 1)              # the expanded layout
    assert sh.stage(c, sh.with_rows(b130, b130["rows"] + [rows[1]])) == 0       # a non-canonical row nothing refers to
    assert sh.run(c, b130, SEGS9) == [0] * 9 and c.pedersen_batch_run() == 2


def test_validation_level_2_torsion_row():
    """(one-pair items: the Ok of an item without pairs is the identity, which Validate::Yes refuses whatever the table holds)"""
    from ark_vrf_amd import _native as nat
    sb = one_pair_tail(None)
    c = nat.Context(0)
    try:
        c.set_validation(2)
        assert sh.run(c, sb, SEGS9) == BAD_ARG and sh.stage(c, sb) == 0 and sh.run(c, sb, SEGS9) == [0] * 9
        rows = list(sb["rows"]); rows[0] = ph.torsion(0, rows[0])
        want = expect_marked(sb, SEGS_FEW, 0)
        assert 0 in want and 2 in want
        assert sh.stage(c, sh.with_rows(sb, rows)) == 0 and sh.run(c, sb, SEGS_FEW) == want
        assert sh.stage(c, sh.with_rows(sb, sb["rows"] + [ph.torsion(0, sb["rows"][0])])) == 0        # validated, referenced by nothing
        assert sh.run(c, sb, [1] * 8 + [122]) == [0] * 9
        pr = list(sb["proofs"]); pr[1] = ph.torsion(0, pr[1][:64]) + pr[1][64:]                      # Yb of item 1
        assert sh.stage(c, dict(sb, proofs=pr)) == 0 and sh.run(c, sb, [1] * 8 + [122]) == [0, 2] + [0] * 7
    finally:
        c.close()


# ---------------------------------------------------------------- wire

def test_wire_entry_point(ctxs, b130):
    c = ctxs[0]
    bad = ph.tampered(b130, 30)
    assert c.pedersen_batch_verify_shared_segments_wire(ph.nat_wire(0, ph.wire(0, bad)), SEGS9, validate=0) == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    ph.check_terms(0, sh.sub_batches(bad, SEGS9)[4], c.pedersen_segment_terms(4))                # the same terms as from x || y
    assert c.pedersen_batch_stage_shared_wire(ph.nat_wire(0, ph.wire(0, b130)), validate=0) == 0
    assert c.pedersen_batch_run_shared_segments([3] * 43 + [1]) == [0] * 44
    # a row that does not decode: the call returns INVALID_DATA and writes no status
    wb = ph.wire(0, b130)
    for y in range(2, 40):                                                     # a y with no x on the curve
        if orc.point_decompress(0, y.to_bytes(32, "little"))[0] != 0:
            break
    else:
        pytest.fail("no undecodable y found")
    wb = dict(wb, rows=[wb["rows"][0], y.to_bytes(32, "little"), wb["rows"][2]])
    assert c.pedersen_batch_verify_shared_segments_wire(ph.nat_wire(0, wb), SEGS9, validate=0) == 2


# ---------------------------------------------------------------- other stagings, other states

def test_plain_staging_equals_the_existing_call(ctxs, b130):
    c = ctxs[0]
    assert c.pedersen_batch_stage(nat_batch(ph.expanded(ph.tampered(b130, 30)))) == 0
    old = c.pedersen_batch_run_segments(SEGS9)
    old_terms = [c.pedersen_segment_terms(v) for v in range(9)]
    assert old == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert c.pedersen_batch_run_shared_segments(SEGS9) == old
    assert [c.pedersen_segment_terms(v) for v in range(9)] == old_terms
    # a "shared" staging without any pair and without a table is a plain one
    nopairs = ph.real_batch(0, [0] * 9, 0, seed=4)
    assert c.pedersen_batch_stage_shared(ph.nat_shared(nopairs)) == 0
    assert c.pedersen_batch_run_shared_segments([4, 5]) == c.pedersen_batch_run_segments([4, 5]) == [0, 0]


def test_state_afterwards_and_refusals(ctxs, b130):
    c = ctxs[0]
    assert sh.stage(c, b130) == 0
    assert c.pedersen_batch_run() == 0
    usual = c.last_terms()
    assert c.pedersen_batch_run_segments(SEGS9) == BAD_ARG                      # the existing call still refuses a shared staging
    assert c.pedersen_batch_run_shared_segments(SEGS9) == [0] * 9
    assert c.last_terms() == usual and c.pedersen_batch_run() == 0 and c.last_terms() == usual
    assert c.pedersen_batch_run_shared_segments([3] * 43 + [1]) == [0] * 44     # the expanded layout prepares differently ...
    assert c.pedersen_batch_run() == 0 and c.last_terms() == usual              # ... and the plain run is still its usual self
    t = c.last_timing()
    assert c.pedersen_batch_run_shared_segments(SEGS9) == [0] * 9
    t = c.last_timing()
    assert t[0] > 0 and t[5] == 0 and all(x >= 0 for x in t[1:5])
    assert c.pedersen_batch_run_shared_segments([100, 29]) == BAD_ARG and c.pedersen_batch_run_shared_segments([100, 31]) == BAD_ARG
    assert c.thin_batch_run_shared_segments(SEGS9) == BAD_ARG                   # a staging of the other kind
    assert c.batch_run_begin() == 0
    assert c.pedersen_batch_run_shared_segments(SEGS9) == BAD_ARG               # busy: between avrf_batch_run_begin and _end
    assert c.batch_run_hash() == 0
    assert c.pedersen_batch_run_shared_segments(SEGS9) == BAD_ARG
    assert c.batch_run_end() == 0
    assert c.pedersen_batch_run_shared_segments(SEGS9) == [0] * 9


def test_repeatability(ctxs, b130):
    c = ctxs[0]
    assert sh.stage(c, b130) == 0
    runs = []
    for _ in range(2):
        st = c.pedersen_batch_run_shared_segments(SEGS9)
        runs.append((st, [c.pedersen_segment_terms(v) for v in range(9)]))
    assert runs[0] == runs[1]                                                   # (the atomics' order may differ: sums in Fr are exact)
