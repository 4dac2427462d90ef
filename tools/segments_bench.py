#!/usr/bin/env python3
"""What a segmented batch verifier (avrf_thin_batch_run_segments; avrf_pedersen_batch_run_segments with --kind=pedersen, whose legs
call the Pedersen twin of every entry point named below) gives against the calls it competes with, on one MI355X in one process:
65 536 one-pair items, the legs run alternately, three runs each; a run is the mean of ten calls after two warm-ups.
    a  thin_batch_run_segments on the resident batch: 256 x 256, 1 024 x 64 and 64 x 1 024 items (and 256 x 256 from the host:
       stage + run, what thin_verify pays too)
    b  thin_verify on the same items: one verdict per item
    c  the same 256 batches of 256 items as separate submissions through an avrf_pool with the headline's slots / lanes / threads
       (from page-locked host buffers; and the pool's resident cycle over 144 such batches)
    d  the plain thin_batch_run: one verdict for everything
    e  SEGMENTED JOBS through an avrf_pool of the same slots / lanes / threads (avrf_pool_submit_segments): the 65 536 items as one job
       of 256 x 256, 24 such jobs in flight, and as sixteen jobs of 16 x 256, 144 in flight; each from the slots' resident state and
       staged again from page-locked host buffers on every run (the pool's cycle mode, no foreign-function call per step)
    f  what a caller could do before: k contexts on k host threads, k = 2, 4, 8, each calling thin_batch_verify_segments (stage from
       the host + 256 x 256) on the whole batch, and the same with the batch resident (thin_batch_run_segments)
    g  SHARED TABLES (avrf_thin_batch_run_shared_segments / avrf_pedersen_batch_run_shared_segments): the n items over 1 024 keys + 3
       inputs staged over the table on one context, against avrf_*_batch_run_segments on the expanded staging of the same items on
       another, alternately: resident, staged from page-locked x || y buffers on every call, and from wire bytes with validate = 1;
       Thin 64 x 1 024 (merged layout) and 256 x 256 (expanded is chosen), Pedersen 256 x 256 and 1 024 x 64 (both merged)
Per leg: items/s, and for the context's legs the k_accumulate milliseconds per call (avrf_kernel_stats) and the host-side stage times
of the segmented call (avrf_last_timing: prepare + wait, transcripts, terms launches, MSM chain + wait).
python tools/segments_bench.py [n] [--quick] [--legs=abcdefg] [--shape=ITEMS] [--kind=thin|pedersen]
    --legs: only these legs; --shape=256: of leg a only the segments of that many items, of leg e only the whole-batch jobs (a kernel
            trace of one leg keeps its kernels apart)
    --kind=pedersen: the same legs over the Pedersen verifier (avrf_pedersen_batch_run_segments, avrf_pedersen_verify, a kind 2 pool)"""
import ctypes as C
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle as orc  # noqa: E402
from ark_vrf_amd import _native as nat  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 65536
QUICK = "--quick" in sys.argv
SLOTS, LANES, THREADS, GROUP, DEPTH = 144, 12, 6, 8, 3
REPS, CALLS, WARM = (1, 3, 1) if QUICK else (3, 10, 2)
LEGS = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--legs=")), "abcdefg")
SHAPE = next((int(a.split("=", 1)[1]) for a in sys.argv[1:] if a.startswith("--shape=")), None)
SHAPES = [(n // k, k) for k in (256, 64, 1024) if SHAPE in (None, k)]             # (segments, items per segment)
KIND = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--kind=")), "thin")
# per kind: the oracle's and the pool's kind ids, the x || y proof size, whether items carry a public key (KIND is also the Context methods' prefix)
ORC_KIND, POOL_KIND, PROOF, HAS_PK = {"thin": (0, 1, 96, True), "pedersen": (1, 2, 256, False)}[KIND]


def accum(ctx, reset):
    ms, cnt = C.c_double(0), C.c_uint64(0)
    nat.lib().avrf_kernel_stats(ctx._h, 1 if reset else 0, C.byref(ms), C.byref(cnt), None)
    return ms.value, cnt.value


def timed(ctx, call):
    """mean seconds of CALLS calls after WARM warm-ups; k_accumulate ms and launches per call"""
    for _ in range(WARM):
        call()
    accum(ctx, True)
    t0 = time.perf_counter()
    for _ in range(CALLS):
        call()
    sec = (time.perf_counter() - t0) / CALLS
    ms, cnt = accum(ctx, True)
    return sec, ms / CALLS, cnt / CALLS


def shared_leg(ctx, record):
    """leg g: the n items over 1 024 keys + 3 inputs (shared_bench.py's table; Pedersen: the 3 inputs) staged over the table on one
    context and in expanded form on another; per shape the new call against the existing one, alternately: resident, staged from
    page-locked x || y buffers on every call, and from page-locked wire bytes with validate = 1"""
    from shared_bench import shared_items                                         # (reads the same n and --kind from the command line)
    b = shared_items(ctx, 1024, 3)
    ped = KIND == "pedersen"
    plen = ctx.point_len
    comp = ctx.points_compress
    w_ios = comp(b["ios_xy"])
    w_proofs = comp(b"".join(b["proofs"][PROOF * j: PROOF * j + PROOF - (64 if ped else 32)] for j in range(n)))
    npts = 3 if ped else 1
    tail = lambda j: b["proofs"][PROOF * j + 64 * npts: PROOF * (j + 1)]
    w_proofs = b"".join(w_proofs[plen * npts * j: plen * npts * (j + 1)] + tail(j) for j in range(n))
    common = (b["io_counts"], b["ads"], b["ad_lens"])
    if ped:
        rows, input_index, outs = nat.dedup_inputs(b["ios_xy"])
        sh_xy = nat.PinnedPedersenSharedBatch(n, rows, input_index, outs, *common, b["proofs"])
        sh_w = nat.PinnedPedersenSharedWireBatch(n, comp(rows), input_index, comp(outs), *common, w_proofs, plen)
        ex_xy = nat.PinnedBatch(n, b["ios_xy"], *common, proofs=b["proofs"])
        ex_w = nat.PinnedBatch(n, w_ios, *common, proofs=w_proofs)
        layout = lambda segs: nat.pedersen_shared_segments_layout(n, segs, sh_xy.n_shared)
        shapes = [(n // 256, 256), (n // 64, 64)]
    else:
        rows, pk_index, input_index, outs = nat.dedup_points(b["pks_xy"], b["ios_xy"])
        sh_xy = nat.PinnedSharedBatch(n, rows, pk_index, input_index, outs, *common, b["proofs"])
        sh_w = nat.PinnedSharedWireBatch(n, comp(rows), pk_index, input_index, comp(outs), *common, w_proofs, plen)
        ex_xy = nat.PinnedBatch(n, b["ios_xy"], *common, pks_xy=b["pks_xy"], proofs=b["proofs"])
        ex_w = nat.PinnedBatch(n, w_ios, *common, pks_xy=comp(b["pks_xy"]), proofs=w_proofs)
        layout = lambda segs: nat.thin_shared_segments_layout(segs, b["io_counts"], sh_xy.n_shared)
        shapes = [(n // 1024, 1024), (n // 256, 256)]
    m = lambda c, name: getattr(c, KIND + "_" + name)
    cs, ce = nat.Context(0), nat.Context(0)                                       # the shared staging and the expanded one, side by side
    try:
        for c in (cs, ce):
            c.set_validation(1)
        for rep in range(REPS):
            for n_seg, k in shapes if SHAPE is None else [(n // SHAPE, SHAPE)]:
                segs = [k] * n_seg
                lay = layout(segs)
                arms = {
                    "resident": (lambda: m(cs, "batch_run_shared_segments")(segs), lambda: m(ce, "batch_run_segments")(segs)),
                    "from pinned x||y": (lambda: (m(cs, "batch_stage_shared")(sh_xy), m(cs, "batch_run_shared_segments")(segs))[1],
                                         lambda: m(ce, "batch_verify_segments")(ex_xy, segs)),
                    "from pinned wire": (lambda: m(cs, "batch_verify_shared_segments_wire")(sh_w, segs, 1),
                                         lambda: m(ce, "batch_verify_segments_wire")(ex_w, segs, 1)),
                }
                assert m(cs, "batch_stage_shared")(sh_xy) == 0 and m(ce, "batch_stage")(ex_xy) == 0
                for mode, (new, old) in arms.items():
                    for arm, c, call in (("shared", cs, new), ("expanded", ce, old)):   # alternately, in this one process
                        assert call() == [0] * n_seg, (mode, arm)
                        sec, ms, cnt = timed(c, call)
                        tm = c.last_timing()
                        record("g %d x %d %s, %s" % (n_seg, k, mode, arm), sec, rep=rep, accumulate_ms=round(ms, 4), L=lay[0] if arm == "shared" else None,
                               merged=lay[4] if arm == "shared" else None,
                               stage_us=dict(prepare=round(tm[1]), transcripts=round(tm[2]), terms=round(tm[3]), msm=round(tm[4])))
    finally:
        cs.close(); ce.close()
        for pb in (sh_xy, sh_w, ex_xy, ex_w):
            pb.close()


def main():
    assert nat.set_blocking_sync(0, True) == 0
    ctx = nat.Context(0)
    b = orc.gen_batch(0, ORC_KIND, n, threads=16)
    pks = (lambda lo, hi: b["pks_xy"][64 * lo: 64 * hi]) if HAS_PK else (lambda lo, hi: None)
    batch = nat.Batch(n, b["ios_xy"], b["io_counts"], b["ads"], b["ad_lens"], pks_xy=pks(0, n), proofs=b["proofs"])
    status = (C.c_int32 * n)()
    stage, run, run_segments, verify_segments, verify_into = (getattr(ctx, KIND + "_" + m) for m in
                                                              ("batch_stage", "batch_run", "batch_run_segments", "batch_verify_segments", "verify_into"))
    out = dict(kind=KIND, n=n, reps=REPS, calls=CALLS, warmups=WARM, pool=dict(slots=SLOTS, lanes=LANES, threads=THREADS, hash_group=GROUP, depth=DEPTH), runs=[])

    def record(leg, sec, items=n, **kw):
        run = dict(leg=leg, items_per_sec=round(items / sec), ms_per_call=round(1e3 * sec, 4), **kw)
        out["runs"].append(run)
        print(json.dumps(run), flush=True)

    # leg c's batches: 256 items each, page-locked; one pool for the separate submissions and the resident cycle
    per = 256
    small = []
    off = [0]
    for ln in b["ad_lens"]:
        off.append(off[-1] + ln)
    for k in range(n // per):
        lo, hi = k * per, (k + 1) * per
        small.append(nat.PinnedBatch(per, b["ios_xy"][128 * lo: 128 * hi], [1] * per, b["ads"][off[lo]: off[hi]], b["ad_lens"][lo: hi],
                                     pks_xy=pks(lo, hi), proofs=b["proofs"][PROOF * lo: PROOF * hi]))
    pool = nat.Pool(0, kind=POOL_KIND, slots=SLOTS, lanes=LANES, threads=THREADS, hash_group=GROUP, depth=DEPTH) if "c" in LEGS else None

    def pool_submissions():
        tk = []
        for i, sb in enumerate(small):
            if i >= SLOTS:
                assert pool.wait(tk[i - SLOTS]) == 0                              # a slot comes free
            tk.append(pool.submit(sb))
        for t in tk[max(0, len(tk) - SLOTS):]:
            assert pool.wait(t) == 0

    # leg e: two pools of the headline's shape; every job of a pool reads the same page-locked buffers
    seg_pools = []
    if "e" in LEGS:
        whole = nat.PinnedBatch(n, b["ios_xy"], b["io_counts"], b["ads"], b["ad_lens"], pks_xy=pks(0, n), proofs=b["proofs"])
        part_n = 16 * per
        part = nat.PinnedBatch(part_n, b["ios_xy"][:128 * part_n], [1] * part_n, b["ads"][:off[part_n]], b["ad_lens"][:part_n], pks_xy=pks(0, part_n),
                               proofs=b["proofs"][:PROOF * part_n])
        shapes_e = (("%d x %d per job, 24 jobs" % (n // per, per), whole, n, 24), ("16 x %d per job, %d jobs" % (per, SLOTS), part, part_n, SLOTS))
        for name, pb, items, jobs in shapes_e[:1] if SHAPE else shapes_e:          # (--shape: the whole-batch jobs only)
            sp = nat.Pool(0, kind=POOL_KIND, slots=SLOTS, lanes=LANES, threads=THREADS, hash_group=GROUP, depth=DEPTH)
            tk = [sp.submit_segments(pb, [per] * (items // per)) for _ in range(jobs)]
            assert all(sp.wait_segments(t) == (0, [0] * (items // per)) for t in tk)
            seg_pools.append((name, sp, pb, items, jobs))
    # leg f: eight contexts, each with the whole batch
    many = [nat.Context(0) for _ in range(8)] if "f" in LEGS else []

    def contexts_leg(k, from_host):
        """k host threads, a context each: CALLS calls after WARM warm-ups, started together -> seconds per call of ONE context"""
        segs = [per] * (n // per)
        gate = threading.Barrier(k + 1)
        bad = []

        def work(c):
            vs, rs = getattr(c, KIND + "_batch_verify_segments"), getattr(c, KIND + "_batch_run_segments")
            call = (lambda: vs(batch, segs)) if from_host else (lambda: rs(segs))
            if not from_host:
                getattr(c, KIND + "_batch_stage")(batch)
            for _ in range(WARM):
                call()
            gate.wait()
            for _ in range(CALLS):
                if call() != [0] * len(segs):
                    bad.append(1)
            gate.wait()
        th = [threading.Thread(target=work, args=(c,)) for c in many[:k]]
        [t.start() for t in th]
        gate.wait()
        t0 = time.perf_counter()
        gate.wait()
        sec = time.perf_counter() - t0
        [t.join() for t in th]
        assert not bad
        return sec / CALLS

    try:
        if "g" in LEGS:
            shared_leg(ctx, record)
        for rep in range(REPS if LEGS != "g" else 0):
            assert stage(batch) == 0
            for n_seg, k in SHAPES if "a" in LEGS else []:                         # a: resident
                segs = [k] * n_seg
                assert run_segments(segs) == [0] * n_seg
                sec, ms, cnt = timed(ctx, lambda: run_segments(segs))
                tm = ctx.last_timing()
                record("a %d x %d" % (n_seg, k), sec, rep=rep, accumulate_ms=round(ms, 4), accumulate_launches=cnt,
                       stage_us=dict(prepare=round(tm[1]), transcripts=round(tm[2]), terms=round(tm[3]), msm=round(tm[4])))
            if "d" in LEGS:
                sec, ms, cnt = timed(ctx, lambda: run())
                record("d plain run", sec, rep=rep, accumulate_ms=round(ms, 4), accumulate_launches=cnt)
            if "a" in LEGS and SHAPE in (None, 256):
                segs = [256] * (n // 256)
                sec, ms, cnt = timed(ctx, lambda: verify_segments(batch, segs))
                record("a 256 x 256 from host", sec, rep=rep, accumulate_ms=round(ms, 4))
            if "b" in LEGS:
                sec, _, _ = timed(ctx, lambda: verify_into(batch, status))
                assert not any(status)
                record("b %s_verify" % KIND, sec, rep=rep)
            for name, sp, pb, items, jobs in seg_pools:                           # e
                for from_host in (False, True):
                    sp.cycle(steps_block=jobs, min_seconds=0.1, from_host=from_host, expect=0)
                    sp.stats(reset=True)
                    done, mism, sec = sp.cycle(steps_block=jobs, min_seconds=0.3 if QUICK else 1.0, from_host=from_host, expect=0)
                    assert mism == 0
                    st = sp.stats()
                    record("e pool segments, %s, %s" % (name, "from pinned host" if from_host else "resident"), sec / done, items=items, rep=rep,
                           accumulate_ms=round(st["accumulate_ms_total"] / done, 4), sleeps_per_job=round(st["sleeps"] / done, 2),
                           host_cpu_us_per_job={k[7:]: round(st[k] / done) for k in ("cpu_us_begin", "cpu_us_collect", "cpu_us_hash", "cpu_us_launch", "cpu_us_end")})
            for k in (2, 4, 8) if "f" in LEGS else []:                              # f
                for from_host in (True, False):
                    sec = contexts_leg(k, from_host)
                    record("f %d contexts, 256 x 256 %s" % (k, "from host" if from_host else "resident"), sec, items=k * n, rep=rep)
            if "c" not in LEGS:
                continue
            for _ in range(WARM):                                                  # c
                pool_submissions()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                pool_submissions()
            record("c pool, %d submissions of %d" % (len(small), per), (time.perf_counter() - t0) / CALLS, rep=rep)
            tk = [pool.submit(sb) for sb in small[:SLOTS]]
            assert all(pool.wait(t) == 0 for t in tk)
            pool.cycle(steps_block=SLOTS, min_seconds=0.1, expect=0)
            done, mism, sec = pool.cycle(steps_block=SLOTS, min_seconds=0.3 if QUICK else 1.0, expect=0)
            assert mism == 0
            record("c pool, resident cycle of %d-item batches" % per, sec / done, items=per, rep=rep)
        legs = {}
        for r in out["runs"]:
            legs.setdefault(r["leg"], []).append(r["items_per_sec"])
        out["ranges"] = {leg: [min(v), max(v)] for leg, v in legs.items()}
    finally:
        if pool:
            pool.close()
        for _, sp, pb, _, _ in seg_pools:
            sp.close()
        for pb in {id(x[2]): x[2] for x in seg_pools}.values():
            pb.close()
        for c in many:
            c.close()
        for sb in small:
            sb.close()
        ctx.close()
    print(json.dumps(out["ranges"], indent=1))


if __name__ == "__main__":
    main()
