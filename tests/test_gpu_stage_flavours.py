"""GPU: the four ways of handing a Thin batch to the device -- x || y, a shared table, wire bytes, a shared table of wire bytes --
staged one after another on ONE context and through ONE pool slot: what one flavour leaves staged must never show in the next.

The batch is five verifying items with 0, 1, 2, 1 and 3 I/O pairs (no pair, one and several take different paths in staging and in
validation), made by the oracle's prover (test_gpu_thin_segments.made_items; orc.gen_batch makes one-pair items only).  Its wire form
comes from Context.points_compress, its shared forms from dedup_points / dedup_points_wire.  Suite 0 has the counter-mode weight
transcript, suite 5 the sponge one, which reads the host copy of the responses that staging keeps.  Expected verdicts are the
oracle's; expected terms are those of a FRESH context that staged and ran that flavour alone, computed once per module."""
import ctypes as C

import pytest

import oracle as orc
from test_gpu_thin_segments import batch_dict, made_items, tamper_s
from test_gpu_thin_shared_wire import bad_point

pytestmark = pytest.mark.gpu

OK, FAILURE, INVALID_DATA, BAD_ARG = 0, 1, 2, -2
COUNTS = [0, 1, 2, 1, 3]
SUITES = [0, 5]
FLAVOURS = ["plain", "shared", "wire", "shared_wire"]
ORDER = ["plain", "shared", "wire", "shared_wire", "plain", "wire", "shared"]
VARIANTS = ["good", "tampered", "empty"]


def sources(nat, c, items):
    """the four forms of one batch, flavour -> batch object (c: any context of the suite, for points_compress)"""
    b = batch_dict(items)
    n, L = b["n"], c.point_len
    proofs = [b["proofs"][96 * j: 96 * j + 96] for j in range(n)]
    w_pks, w_ios = c.points_compress(b["pks_xy"]), c.points_compress(b["ios_xy"])
    w_proofs = b"".join(c.points_compress(p[:64]) + p[64:] for p in proofs)
    rest = (b["io_counts"], b["ads"], b["ad_lens"])
    return dict(plain=nat.Batch(n, b["ios_xy"], *rest, pks_xy=b["pks_xy"], proofs=b["proofs"]),
                wire=nat.Batch(n, w_ios, *rest, pks_xy=w_pks, proofs=w_proofs),
                shared=nat.SharedBatch(n, *nat.dedup_points(b["pks_xy"], b["ios_xy"]), *rest, b["proofs"]),
                shared_wire=nat.SharedWireBatch(n, *nat.dedup_points_wire(w_pks, w_ios, L), *rest, w_proofs, L))


def stage(nat, c, flavour, src):
    if flavour == "plain":
        return c.thin_batch_stage(src)
    if flavour == "shared":
        return c.thin_batch_stage_shared(src)
    if flavour == "shared_wire":
        return c.thin_batch_stage_shared_wire(src, 1)
    return nat.lib().avrf_thin_batch_stage_wire(c._h, C.c_size_t(src.n), src.pks_xy, src.ios_xy, src.io_counts, src.ads, src.ad_lens, src.proofs, 1)


def submit(pool, flavour, src):
    return {"plain": pool.submit, "shared": pool.submit_shared, "wire": pool.submit_wire, "shared_wire": pool.submit_shared_wire}[flavour](src)


def undecodable(nat, suite, sw):
    """the shared-wire batch with the row of item 0's key replaced by a y that has no x on the curve"""
    L, r = len(bytes(sw.shared_xy)) // sw.n_shared, sw.pk_index[0]
    rows = bytes(sw.shared_xy)
    rows = rows[: L * r] + bad_point(suite) + rows[L * r + L:]
    return nat.SharedWireBatch(sw.n, rows, sw.pk_index, sw.input_index, sw.outputs_xy, sw.io_counts, sw.ads, sw.ad_lens, sw.proofs, L)


@pytest.fixture(scope="module")
def material():
    """suite -> variant -> dict(items, verdict: the oracle's, src: the four forms, terms: flavour -> a fresh context's last_terms)"""
    from ark_vrf_amd import _native as nat
    out = {}
    for suite in SUITES:
        good = made_items(suite, COUNTS, seed=7)
        variants = dict(good=good, tampered=good[:3] + [tamper_s(good[3])] + good[4:], empty=[])
        util = nat.Context(suite)
        out[suite] = {}
        for name, items in variants.items():
            verdict = orc.thin_batch_verify_xy(suite, batch_dict(items)) if items else OK
            src = sources(nat, util, items)
            terms = {}
            for flavour in FLAVOURS:
                fresh = nat.Context(suite)
                assert stage(nat, fresh, flavour, src[flavour]) == OK and fresh.thin_batch_run() == verdict, (suite, name, flavour)
                terms[flavour] = fresh.last_terms()
                fresh.close()
            out[suite][name] = dict(items=items, verdict=verdict, src=src, terms=terms)
        util.close()
        assert [out[suite][v]["verdict"] for v in VARIANTS] == [OK, FAILURE, OK]
    return out


@pytest.fixture(scope="module")
def nat():
    from ark_vrf_amd import _native
    return _native


@pytest.mark.parametrize("suite", SUITES)
def test_one_context_every_flavour_in_turn(nat, material, suite):
    c = nat.Context(suite)
    try:
        for variant in VARIANTS:
            m = material[suite][variant]
            for flavour in ORDER:
                assert stage(nat, c, flavour, m["src"][flavour]) == OK, (variant, flavour)
                assert c.thin_batch_run() == m["verdict"], (variant, flavour)
                assert c.last_terms() == m["terms"][flavour], (variant, flavour)
    finally:
        c.close()


@pytest.mark.parametrize("suite", SUITES)
def test_state_after_a_failed_staging(nat, material, suite):
    m = material[suite]["good"]
    src, n, pairs = m["src"], len(COUNTS), sum(COUNTS)
    c = nat.Context(suite)
    try:
        assert c.thin_batch_stage_shared(src["shared"]) == OK and c.thin_batch_run() == m["verdict"]
        # a row that does not decode: refused after the reset, so nothing is staged
        assert c.thin_batch_stage_shared_wire(undecodable(nat, suite, src["shared_wire"]), 1) == INVALID_DATA
        assert c.thin_batch_run() == BAD_ARG
        # the plain staging behind it is a plain one: no table left over
        assert c.thin_batch_stage(src["plain"]) == OK and c.thin_batch_run() == m["verdict"]
        bases, scalars = c.last_terms()
        assert len(scalars) // 32 == len(bases) // 64 == 2 * n + 2 * pairs + 1
        assert (bases, scalars) == m["terms"]["plain"]
        # an index past the table is refused BEFORE the reset: the batch staged before stays runnable, with its verdict and terms
        t = material[suite]["tampered"]
        assert c.thin_batch_stage_shared(t["src"]["shared"]) == OK and c.thin_batch_run() == FAILURE
        sb = src["shared"]
        for pk_index, input_index in (([sb.n_shared] + list(sb.pk_index)[1:], sb.input_index), (sb.pk_index, list(sb.input_index)[:-1] + [sb.n_shared])):
            bad = nat.SharedBatch(sb.n, sb.shared_xy, pk_index, input_index, sb.outputs_xy, sb.io_counts, sb.ads, sb.ad_lens, sb.proofs)
            assert c.thin_batch_stage_shared(bad) == BAD_ARG
            assert c.thin_batch_run() == FAILURE and c.last_terms() == t["terms"]["shared"]
    finally:
        c.close()


@pytest.mark.parametrize("suite", SUITES)
def test_one_slot_pool_every_flavour_in_turn(nat, material, suite):
    pool = nat.Pool(suite, kind=1, slots=1, lanes=1, threads=1)
    try:
        for variant in ("good", "tampered"):
            m = material[suite][variant]
            for flavour in FLAVOURS:
                t = submit(pool, flavour, m["src"][flavour])
                assert pool.wait(t) == m["verdict"], (variant, flavour)
                t = pool.resubmit(t, from_host=False)
                assert pool.wait(t) == m["verdict"], (variant, flavour, "resident")
                t = pool.resubmit(t, from_host=True)
                assert pool.wait(t) == m["verdict"], (variant, flavour, "from host")
        m = material[suite]["good"]
        t = pool.submit_shared_wire(undecodable(nat, suite, m["src"]["shared_wire"]), 1)
        assert pool.wait(t) == INVALID_DATA
        t = pool.resubmit(t, from_host=False)
        assert pool.wait(t) == INVALID_DATA
        assert pool.wait(pool.submit(m["src"]["plain"])) == m["verdict"] == OK
    finally:
        pool.close()


@pytest.mark.parametrize("suite", SUITES)
def test_segment_terms_are_the_plain_batch_terms(nat, material, suite):
    items, segs = material[suite]["good"]["items"], [2, 0, 3]
    c, alone = nat.Context(suite), nat.Context(suite)
    try:
        assert c.thin_batch_stage(material[suite]["good"]["src"]["plain"]) == OK
        assert c.thin_batch_run_segments(segs) == [OK, OK, OK]
        at = 0
        for v, k in enumerate(segs):
            seg = items[at: at + k]; at += k
            if not seg:
                assert c.thin_segment_terms(v) == (b"", b"")
                continue
            b = batch_dict(seg)
            assert alone.thin_batch_stage(nat.Batch(k, b["ios_xy"], b["io_counts"], b["ads"], b["ad_lens"], pks_xy=b["pks_xy"], proofs=b["proofs"])) == OK
            assert alone.thin_batch_run() == OK
            assert c.thin_segment_terms(v) == alone.last_terms(), v
    finally:
        c.close(); alone.close()
