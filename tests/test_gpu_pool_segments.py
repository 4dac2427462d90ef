"""avrf_pool segmented jobs (include/avrf.h avrf_pool_submit_segments / _segments_wire / avrf_pool_wait_segments; csrc/pool.hip):
n_seg independent BatchVerifiers over consecutive runs of one submitted batch, one verdict each, with other jobs in flight.

The expectation for a segment is always the oracle on THAT SEGMENT'S ITEMS ALONE (orc.thin_batch_verify_xy /
orc.pedersen_batch_verify_xy; thin::BatchVerifier src/thin.rs:188-326, pedersen::BatchVerifier src/pedersen.rs:303-426), and the
same batch goes through Context.*_batch_run_segments, which must answer the same.  The pool runs ONE MSM chain whatever n_seg is,
the context loops single MSMs below eight segments: both sides of that threshold are here.  Statuses are integers: no tolerance.
Oracle results are computed once per module and shared."""
import ctypes as C
import random
import threading

import pytest

import oracle as orc
import test_gpu_pedersen_segments as ped
import test_gpu_thin_segments as thin
from helpers import IDENTITY_XY, R_ORDER, nat_batch

pytestmark = pytest.mark.gpu

SEGS9 = [1, 2, 3, 5, 7, 16, 33, 64, 130]
Q0 = thin.Q0
BAD_ARG = -2
MOD = {1: thin, 2: ped}                      # pool kind -> the module with that verifier's item helpers


@pytest.fixture(scope="module")
def nat():
    from ark_vrf_amd import _native as nat
    return nat


@pytest.fixture(scope="module")
def ctxs(nat):
    made = {}

    class Lazy(dict):
        def __missing__(self, suite):
            made[suite] = self[suite] = nat.Context(suite)
            return self[suite]
    yield Lazy()
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def nine(golden_dir):
    """per kind: 261 verifying items of suite 0 with 0 to 3 pairs each, the reference's seven vectors among them"""
    rng = random.Random(11)
    counts = [rng.choice([0, 1, 1, 2, 3]) for _ in range(sum(SEGS9) - 7)]
    t = thin.made_items(0, counts, 21)
    p = ped.made_items(0, counts, 22)
    return {1: t[:11] + thin.golden_items(0, golden_dir) + t[11:], 2: p[:11] + ped.golden_items(golden_dir) + p[11:]}


@pytest.fixture(scope="module")
def wide():
    """per kind: ten items, one of them with sixteen pairs, so that the segments' term counts L differ strongly"""
    counts = [1, 0, 16, 2, 1, 1, 3, 1, 2, 1]
    return {1: thin.made_items(0, counts, 31), 2: ped.made_items(0, counts, 32)}


_ORACLE = {}


def oracle(kind, suite, items, segs):
    """the oracle's verdict on every segment's items alone; an empty segment is Ok"""
    out = []
    for seg in thin.slices(items, segs):
        key = (kind, suite, b"".join(it["proof"] for it in seg), b"".join(it.get("pk", b"") + b"".join(it["ios"]) for it in seg))
        if key not in _ORACLE:
            _ORACLE[key] = MOD[kind].oracle_segment(suite, seg)[0]
        out.append(_ORACLE[key])
    return out


def ctx_run(c, kind, items, segs):
    b = nat_batch(MOD[kind].batch_dict(items))
    if kind == 1:
        assert c.thin_batch_stage(b) == 0
        return c.thin_batch_run_segments(segs)
    assert c.pedersen_batch_stage(b) == 0
    return c.pedersen_batch_run_segments(segs)


def job(kind, items):
    return nat_batch(MOD[kind].batch_dict(items))


def run_jobs(pool, kind, jobs):
    """jobs: (items, segs or None for a plain job); all submitted (more than the pool has slots: the oldest is collected first), then
    collected -> per job (status, statuses) or the plain status"""
    got, tickets = {}, []

    def collect():
        k0, t0, segs = tickets.pop(0)
        got[k0] = pool.wait(t0) if segs is None else pool.wait_segments(t0)
    for k, (items, segs) in enumerate(jobs):
        if len(tickets) == pool.n_slots:
            collect()
        b = job(kind, items)
        tickets.append((k, pool.submit(b) if segs is None else pool.submit_segments(b, segs), segs))
    while tickets:
        collect()
    return [got[k] for k in range(len(jobs))]


def make_pool(nat, suite, kind, slots=5, lanes=2, threads=2, group=8, depth=0):
    pool = nat.Pool(suite, kind=kind, slots=slots, lanes=lanes, threads=threads, hash_group=group, depth=depth)
    pool.n_slots = slots
    return pool


def check_jobs(nat, ctxs, suite, kind, jobs, **pool_args):
    """every segmented job's statuses are the oracle's and the context's; its status is their largest"""
    want = [oracle(kind, suite, items, segs) for items, segs in jobs]
    for (items, segs), w in zip(jobs, want):
        assert ctx_run(ctxs[suite], kind, items, segs) == w, segs
    pool = make_pool(nat, suite, kind, **pool_args)
    try:
        got = run_jobs(pool, kind, jobs)
    finally:
        pool.close()
    assert got == [(max(w, default=0), w) for w in want]
    return want


def tamper(kind, it):
    return thin.tamper_s(it) if kind == 1 else ped.tamper(it, 1)


def partitions(n, k):
    """k segments of nearly equal size over n items"""
    return [n // k + (1 if v < n % k else 0) for v in range(k)]


# ---------------------------------------------------------------- shapes, hash groups, depths

@pytest.mark.parametrize("kind,group,depth", [(1, 1, 1), (1, 8, 0), (1, 16, 0), (2, 1, 1), (2, 8, 0), (2, 16, 1)])
def test_shapes(nat, ctxs, nine, wide, kind, group, depth):
    """the nine segments; empty segments first, in the middle and last; 1, 2, 7, 8 and 9 segments (the context's call loops single
    MSMs below eight, the pool's job is one chain); a sixteen-pair item alone in its segment; one bad segment among them"""
    items = nine[kind]
    bad = list(items)
    bad[40] = tamper(kind, bad[40])
    jobs = [(items, SEGS9), (items, [0, 1, 2, 3, 5, 0, 7, 16, 33, 64, 130, 0]), (bad, SEGS9)]
    jobs += [(bad if k in (2, 8) else items, partitions(261, k)) for k in (1, 2, 7, 8, 9)]
    jobs += [(wide[kind], [2, 1, 3, 4]), (wide[kind], [2, 1, 0, 0, 3, 1, 1, 1, 1])]
    want = check_jobs(nat, ctxs, 0, kind, jobs, group=group, depth=depth)
    assert want[0] == [0] * 9 and want[2] == [0, 0, 0, 0, 0, 0, 1, 0, 0] and want[4] == [1, 0] and want[-1] == [0] * 9


@pytest.mark.parametrize("suite,kind", [(s, k) for s in (orc.BABYJUBJUB, orc.BANDERSNATCH_SHAKE128, orc.SECP256R1) for k in (1, 2)])
def test_other_suites(nat, ctxs, suite, kind):
    """Baby-JubJub; the SHAKE128 suite, whose weight streams the worker squeezes per segment; secp256r1, whose plain chains take no
    slot's record (one chain per lane) and whose segments end in the generic device Horner"""
    items = MOD[kind].gen_items(suite, 32)
    bad = list(items)
    bad[22] = tamper(kind, bad[22])
    jobs = [(items, [4] * 8), (bad, [4] * 8), (bad, [10, 12, 10]), (bad, [32]), (items, [0, 30, 2, 0])]
    want = check_jobs(nat, ctxs, suite, kind, jobs, slots=3, lanes=2, threads=2, group=8)
    assert want[1] == [0, 0, 0, 0, 0, 1, 0, 0] and want[2] == [0, 0, 1] and want[3] == [1]


# ---------------------------------------------------------------- bad items mark their own segment only

def one_pair_item(items, lo, hi):
    return next(j for j in range(lo, hi) if len(items[j]["ios"]) == 1)


@pytest.mark.parametrize("kind", [1, 2])
def test_bad_items_mark_their_segment(nat, ctxs, nine, kind):
    """a tampered response: VerificationFailure; an identity key (Thin), an identity input, an identity key commitment Yb (Pedersen),
    a response >= r: InvalidData -- each for its own segment and no other"""
    items = nine[kind]
    r_bytes = R_ORDER[0].to_bytes(32, "little")
    at = lambda v, k=0: sum(SEGS9[:v]) + k
    j_io = one_pair_item(items, at(5), at(6))
    variants = {"tampered": (2, at(2, 1), lambda it: tamper(kind, it)),
                "io_identity": (5, j_io, lambda it: dict(it, ios=[IDENTITY_XY + it["ios"][0][64:]])),
                "s_ge_r": (0, at(0), lambda it: dict(it, proof=(it["proof"][:64] + r_bytes) if kind == 1 else (it["proof"][:192] + r_bytes + it["proof"][224:])))}
    if kind == 1:
        variants["pk_identity"] = (3, at(3, 2), lambda it: dict(it, pk=IDENTITY_XY))
    else:
        variants["yb_identity"] = (3, at(3, 2), lambda it: dict(it, proof=IDENTITY_XY + it["proof"][64:]))
    jobs, marks = [], []
    for name, (v, j, f) in variants.items():
        worse = list(items)
        worse[j] = f(worse[j])
        jobs.append((worse, SEGS9)); marks.append((name, v))
    both = list(items)                                                     # a failure and invalid data in one batch
    both[at(2, 1)] = tamper(kind, both[at(2, 1)])
    both[at(7, 9)] = variants["s_ge_r"][2](both[at(7, 9)])
    jobs.append((both, SEGS9))
    # a response >= r is an encoding the oracle's typed scalars cannot hold: there the expectation is the context's call, which
    # tests/test_gpu_*_segments.py pin to the one-call verifier on the segment alone
    pool = make_pool(nat, 0, kind)
    try:
        got = run_jobs(pool, kind, jobs)
    finally:
        pool.close()
    for (name, v), (worse, segs), g in zip(marks + [("both", None)], jobs, got):
        want = ctx_run(ctxs[0], kind, worse, segs)
        assert g == (max(want), want), name
        if name not in ("s_ge_r", "both"):
            assert want == oracle(kind, 0, worse, segs), name
        if v is not None:
            assert want == [(1 if name == "tampered" else 2) if u == v else 0 for u in range(9)], name
    assert got[-1][1] == [0, 0, 1, 0, 0, 0, 0, 2, 0]


@pytest.mark.parametrize("kind", [1, 2])
def test_validation_level_2(nat, kind):
    """an output with a torsion component, (x, y) -> (-x, -y): on the curve, outside the subgroup -- under set_validation(2) only its
    segment is InvalidData, as the context's call answers"""
    items = MOD[kind].gen_items(0, 32)
    o = items[13]["ios"][0][64:]
    tors = ((Q0 - int.from_bytes(o[:32], "little")) % Q0).to_bytes(32, "little") + ((Q0 - int.from_bytes(o[32:], "little")) % Q0).to_bytes(32, "little")
    bad = list(items)
    bad[13] = dict(bad[13], ios=[bad[13]["ios"][0][:64] + tors])
    c = nat.Context(0)
    pool = make_pool(nat, 0, kind, slots=3)
    try:
        c.set_validation(2)
        assert pool.set_validation(2) == 0
        jobs = [(bad, [4] * 8), (bad, [10, 12, 10]), (items, [4] * 8)]
        want = [ctx_run(c, kind, it, sg) for it, sg in jobs]
        assert want == [[0, 0, 0, 2, 0, 0, 0, 0], [0, 2, 0], [0] * 8]
        assert run_jobs(pool, kind, jobs) == [(max(w), w) for w in want]
    finally:
        pool.close(); c.close()


# ---------------------------------------------------------------- wire

@pytest.mark.parametrize("kind", [1, 2])
def test_wire_jobs(nat, ctxs, nine, kind):
    """validate 0 and 1 agree with the x || y job; a point that does not decode is the JOB's InvalidData with no per-segment status,
    as avrf_*_batch_verify_segments_wire returns it, and runs from the resident state repeat it"""
    m = MOD[kind]
    good = [it for it in nine[kind] if it["ios"]]        # (Validate::Yes refuses the identity, and a Pedersen item without pairs carries it as Ok)
    segs = SEGS9[:8] + [len(good) - sum(SEGS9[:8])]
    bad = list(good)
    bad[30] = tamper(kind, bad[30])
    want = oracle(kind, 0, bad, segs)
    assert want == [0, 0, 0, 0, 0, 1, 0, 0, 0] and ctx_run(ctxs[0], kind, bad, segs) == want
    bad_y = next(k.to_bytes(32, "little") for k in range(2, 300) if orc.point_decompress(0, k.to_bytes(32, "little"))[0] != 0)
    und = list(bad)
    und[-1] = dict(und[-1], w_proof=bad_y + und[-1]["w_proof"][32:])
    verify_wire = ctxs[0].thin_batch_verify_segments_wire if kind == 1 else ctxs[0].pedersen_batch_verify_segments_wire
    pool = make_pool(nat, 0, kind, slots=6)
    try:
        tk = [pool.submit_segments(job(kind, bad), segs)]
        tk += [pool.submit_segments_wire(m.wire_batch(bad), segs, validate=v) for v in (0, 1)]
        tk += [pool.submit_segments_wire(m.wire_batch(good), segs, validate=1), pool.submit_segments_wire(m.wire_batch(und), segs, validate=1)]
        got = [pool.wait_segments(t) for t in tk]
        assert got[:4] == [(1, want)] * 3 + [(0, [0] * 9)]
        assert got[4] == (2, None) and verify_wire(m.wire_batch(und), segs, 1) == 2
        # resubmission: the undecodable job from its resident state, then staged again from the host, then resident again; a good one both ways
        t = tk[4]
        for from_host in (False, True, False):
            t = pool.resubmit(t, from_host=from_host)
            assert pool.wait_segments(t) == (2, None)
        assert pool.wait(pool.resubmit(t)) == 2
        t = tk[1]
        for from_host in (False, True):
            t = pool.resubmit(t, from_host=from_host)
            assert pool.wait_segments(t) == (1, want)
    finally:
        pool.close()


# ---------------------------------------------------------------- jobs in flight

@pytest.mark.parametrize("kind", [1, 2])
def test_jobs_in_flight(nat, ctxs, nine, wide, kind):
    """six jobs of different shapes, plain and segmented interleaved, on five slots / two lanes / two threads: each gets the verdicts of
    its own one-call run; resubmitted twice from the resident state and once from the host; the cycle mode over them"""
    items = nine[kind]
    bad = list(items)
    bad[100] = tamper(kind, bad[100])
    c = ctxs[0]
    jobs = [(items, SEGS9), (bad[:150], None), (bad, partitions(261, 3)), (items[:64], None), (wide[kind], [2, 1, 3, 4]), (bad, [1] * 200 + [61])]
    want = []
    for it, segs in jobs:
        if segs is None:
            stage, run = (c.thin_batch_stage, c.thin_batch_run) if kind == 1 else (c.pedersen_batch_stage, c.pedersen_batch_run)
            assert stage(job(kind, it)) == 0
            want.append(run())
        else:
            w = ctx_run(c, kind, it, segs)
            assert w == oracle(kind, 0, it, segs)
            want.append((max(w), w))
    assert want[1] == 1 and want[3] == 0 and want[2] == (1, [0, 1, 0]) and want[5][1][100] == 1 and sum(want[5][1]) == 1
    pool = make_pool(nat, 0, kind)
    try:
        keep = [job(kind, it) for it, _ in jobs]
        collect = lambda t, segs: pool.wait(t) if segs is None else pool.wait_segments(t)
        tk = [pool.submit(b) if segs is None else pool.submit_segments(b, segs) for b, (_, segs) in zip(keep[:5], jobs)]
        got = [collect(tk[0], jobs[0][1])]                                    # five slots: the sixth job takes the first one's
        tk.append(pool.submit_segments(keep[5], jobs[5][1]))
        got += [collect(t, segs) for t, (_, segs) in zip(tk[1:], jobs[1:])]
        assert got == want
        # the five resident jobs again (the sixth overwrote the first): twice from the resident state, once from the host
        live = list(zip(tk[1:], jobs[1:], want[1:]))
        for from_host in (False, False, True):
            live = [(pool.resubmit(t, from_host=from_host), j, w) for t, j, w in live]
            assert [collect(t, j[1]) for t, j, w in live] == [w for _, _, w in live]
        # a plain wait on a segmented ticket returns the fold
        t = pool.resubmit(live[1][0])
        assert pool.wait(t) == 1
    finally:
        pool.close()
    # the cycle mode: all-valid jobs, plain and segmented, against expect = 0; one job with a bad segment against expect = 1
    pool = make_pool(nat, 0, kind)
    try:
        tk = [pool.submit_segments(job(kind, items), SEGS9), pool.submit(job(kind, items[:64])), pool.submit_segments(job(kind, wide[kind]), [2, 1, 3, 4]),
              pool.submit_segments(job(kind, items), partitions(261, 8))]
        assert [pool.wait(t) for t in tk] == [0] * 4
        for from_host in (False, True):
            done, mism, _ = pool.cycle(steps_block=8, min_seconds=0.0, from_host=from_host, expect=0)
            assert (done, mism) == (8, 0)
        st = pool.stats()
        assert st["hashed"] >= 2 * (9 + 1 + 4 + 8)                            # every segment's transcript is counted
    finally:
        pool.close()
    pool = make_pool(nat, 0, kind, slots=2, lanes=1, threads=1)
    try:
        assert pool.wait_segments(pool.submit_segments(job(kind, bad), SEGS9)) == (1, [0, 0, 0, 0, 0, 0, 0, 1, 0])
        done, mism, _ = pool.cycle(steps_block=4, min_seconds=0.0, expect=1)
        assert (done, mism) == (4, 0)
    finally:
        pool.close()


# ---------------------------------------------------------------- refusals, lifecycle

def test_refusals(nat, ctxs):
    items = thin.gen_items(0, 40)
    bad = list(items)
    bad[5] = thin.tamper_s(bad[5])
    b = thin.batch_dict(bad)
    nb = nat_batch(b)
    pool = make_pool(nat, 0, 1, slots=3)

    def raw(nb, segs):
        tk = C.c_uint64(0)
        st = nat.lib().avrf_pool_submit_segments(pool._h, C.c_size_t(nb.n), nb.pks_xy, nb.ios_xy, nb.io_counts, nb.ads, nb.ad_lens, nb.proofs,
                                                 C.c_size_t(len(segs)), nat._u32(segs), C.byref(tk))
        return st, tk.value

    def still_runs():
        assert pool.wait_segments(pool.submit_segments(nb, [20, 20])) == (1, [1, 0])
    try:
        assert raw(nb, [20, 19])[0] == BAD_ARG and raw(nb, [20, 21])[0] == BAD_ARG       # counts that do not sum to n: no ticket
        still_runs()
        # a segment over AVRF_SEGMENT_TERMS_MAX: 2 items + 2 x 4 095 pairs + 1 = 8 195 terms.  Refused on the submitting thread from
        # io_counts alone, before any other buffer is looked at.
        fat = nat.Batch(2, b"", [4095, 0], b"", [0, 0], pks_xy=bytes(128), proofs=bytes(192))
        assert raw(fat, [1, 1])[0] == BAD_ARG and raw(fat, [2])[0] == BAD_ARG
        still_runs()
        # 1 009 one-item segments of 65 windows each: over AVRF_SEGMENTS_WINDOWS_MAX
        many = nat.Batch(1009, b"", [1] * 1009, b"", [0] * 1009, pks_xy=bytes(64), proofs=bytes(96))
        assert raw(many, [1] * 1009)[0] == BAD_ARG
        still_runs()
        # cap too small, and a plain ticket: refused, and the ticket is not consumed
        t = pool.submit_segments(nb, [10, 10, 20])
        with pytest.raises(nat.AvrfError):
            pool.wait_segments(t, cap=2)
        assert pool.wait_segments(t) == (1, [1, 0, 0])
        t = pool.submit(nb)
        with pytest.raises(nat.AvrfError):
            pool.wait_segments(t, cap=8)
        assert pool.wait(t) == 1
        with pytest.raises(nat.AvrfError):
            pool.wait_segments(t, cap=8)                                                  # collected: gone
        # a shared-table job in the same pool is unaffected
        rows, pk_index, input_index, outs = nat.dedup_points(b["pks_xy"], b["ios_xy"])
        sb = nat.SharedBatch(40, rows, pk_index, input_index, outs, b["io_counts"], b["ads"], b["ad_lens"], b["proofs"])
        assert pool.wait(pool.submit_shared(sb)) == 1
        still_runs()
        # the empty batch: every (empty) segment is Ok; no segments at all
        e = nat_batch(thin.batch_dict([]))
        assert pool.wait_segments(pool.submit_segments(e, [0, 0])) == (0, [0, 0])
        assert pool.wait_segments(pool.submit_segments(e, [])) == (0, [])
        assert raw(e, [1])[0] == BAD_ARG
        still_runs()
    finally:
        pool.close()
    # a Pedersen pool refuses by its own layout: 1 638 items in one segment are 8 192 terms
    pool = make_pool(nat, 0, 2, slots=2)
    try:
        tk = C.c_uint64(0)
        n = 1638
        st = nat.lib().avrf_pool_submit_segments(pool._h, C.c_size_t(n), None, nat._u8(b""), nat._u32([0] * n), nat._u8(b""), nat._u32([0] * n), nat._u8(bytes(256)),
                                                 C.c_size_t(1), nat._u32([n]), C.byref(tk))
        assert st == BAD_ARG
        pit = ped.gen_items(0, 8)
        assert pool.wait_segments(pool.submit_segments(job(2, pit), [4, 4])) == (0, [0, 0])
    finally:
        pool.close()


def test_destroy_with_segmented_jobs_in_flight(nat):
    """a pool destroyed with segmented jobs submitted and uncollected returns; a new pool works afterwards"""
    items = thin.gen_items(0, 200)
    bad = list(items)
    bad[7] = thin.tamper_s(bad[7])
    pool = make_pool(nat, 0, 1, slots=6, lanes=2, threads=2)
    keep = [nat_batch(thin.batch_dict(items)) for _ in range(6)]
    for k, b in enumerate(keep):
        if k % 2:
            pool.submit(b)
        else:
            pool.submit_segments(b, [25] * 8)
    th = threading.Thread(target=pool.close)
    th.start(); th.join(60)
    assert not th.is_alive()
    pool2 = make_pool(nat, 0, 1, slots=2, lanes=1, threads=1, group=1)
    try:
        assert pool2.wait_segments(pool2.submit_segments(nat_batch(thin.batch_dict(bad)), [100, 100])) == (1, [1, 0])
    finally:
        pool2.close()
