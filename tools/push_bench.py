#!/usr/bin/env python3
"""What an OPEN batch (avrf_*_batch_open / _push, include/avrf.h) gives a caller whose items arrive in chunks, against the one-shot
call, on one MI355X with one context and nothing else on the device: suite 0, 65 536 one-pair items in avrf_host_alloc buffers.
Two legs run alternately in one process, five timed runs each after a warm-up:
    a  avrf_thin_batch_verify, one shot: stage + run of all items
    b  avrf_thin_batch_open with exact hints, the items pushed in equal chunks back to back, then avrf_thin_batch_run; two times:
         tail   from the return of the last push to the verdict -- what the feature exists for
         total  from the first push to the verdict -- to be held against (a)
       and where the tail went (avrf_last_timing of the run: wait for the stream, transcript left to absorb, terms launch, MSM + wait)
    c  (b) with PACED arrivals: push i is not made before i x gap microseconds after the first (the host spins meanwhile), the model
       of a gossip handler whose items arrive steadily; only the tail is reported (the total is the arrival span)
for 64 x 1 024, 16 x 4 096 and 512 x 128 items, then the same for Pedersen.  Ranges over the timed runs, not means.
python tools/push_bench.py [n] [--runs=5] [--kind=thin|pedersen|both] [--gap-us=300]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle as orc  # noqa: E402
from ark_vrf_amd import _native as nat  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if args else 65536
RUNS = next((int(a.split("=", 1)[1]) for a in sys.argv[1:] if a.startswith("--runs=")), 5)
KINDS = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--kind=")), "both")
GAP_US = next((float(a.split("=", 1)[1]) for a in sys.argv[1:] if a.startswith("--gap-us=")), 300.0)
CHUNKS = [c for c in (1024, 4096, 128) if N % c == 0]


def at(p, off):
    return C.c_void_p(p.value + off)


def bench(kind_name):
    kind, okind, psz = {"thin": (1, 0, 96), "pedersen": (2, 1, 256)}[kind_name]
    L = nat.lib()
    b = orc.gen_batch(0, okind, N, threads=min(16, os.cpu_count() or 1))
    pin = nat.PinnedBatch(N, b["ios_xy"], b["io_counts"], b["ads"], b["ad_lens"], pks_xy=b["pks_xy"] if kind == 1 else None, proofs=b["proofs"])
    ad_off = [0]
    for ln in b["ad_lens"]:
        ad_off.append(ad_off[-1] + ln)
    ctx = nat.Context(0)
    n = C.c_size_t(N)

    def one_shot():
        t0 = time.perf_counter()
        if kind == 1:
            st = L.avrf_thin_batch_verify(ctx._h, n, pin.pks_xy, pin.ios_xy, pin.io_counts, pin.ads, pin.ad_lens, pin.proofs)
        else:
            st = L.avrf_pedersen_batch_verify(ctx._h, n, pin.ios_xy, pin.io_counts, pin.ads, pin.ad_lens, pin.proofs)
        assert st == 0, st
        return (time.perf_counter() - t0) * 1e3

    def pushed(chunk, gap_us=0.0):
        # (the argument lists are made before the clock starts: what is timed is the calls)
        calls = []
        for lo in range(0, N, chunk):
            tail = [at(pin.ios_xy, 128 * lo), at(pin.io_counts, 4 * lo), at(pin.ads, ad_off[lo]), at(pin.ad_lens, 4 * lo), at(pin.proofs, psz * lo)]
            calls.append([ctx._h, C.c_size_t(chunk)] + ([at(pin.pks_xy, 64 * lo)] if kind == 1 else []) + tail)
        push = L.avrf_thin_batch_push if kind == 1 else L.avrf_pedersen_batch_push
        run = L.avrf_thin_batch_run if kind == 1 else L.avrf_pedersen_batch_run
        assert ctx.batch_open(kind, N, N, ad_off[N]) == 0
        t0 = time.perf_counter()
        for i, a in enumerate(calls):
            while gap_us and (time.perf_counter() - t0) * 1e6 < i * gap_us:
                pass
            st = push(*a)
            assert st == 0, st
        t1 = time.perf_counter()
        st = run(ctx._h)
        t2 = time.perf_counter()
        assert st == 0, st
        return (t2 - t1) * 1e3, (t2 - t0) * 1e3, [x / 1e3 for x in ctx.last_timing()[:6]]

    rng = lambda v: "%.2f .. %.2f" % (min(v), max(v))
    out = {}
    for chunk in CHUNKS:
        one_shot(); pushed(chunk)                                               # warm-up: buffers, code objects, the MSM plan
        a, tail, total, where, paced, paced_where = [], [], [], [], [], []
        for _ in range(RUNS):
            a.append(one_shot())
            t, tt, w = pushed(chunk)
            tail.append(t); total.append(tt); where.append(w)
            t, tt, w = pushed(chunk, GAP_US)
            paced.append(t); paced_where.append(w)
        print(f"{kind_name:8s} n={N} chunks {N // chunk} x {chunk}: one shot {rng(a)} ms | open: tail {rng(tail)} ms, total {rng(total)} ms", flush=True)
        names = ["calls", "wait", "hash left", "terms launch", "msm + wait", "verdict"]
        print("         the tail's run by phase (ms): " + ", ".join(f"{nm} {rng([w[i] for w in where])}" for i, nm in enumerate(names)), flush=True)
        print(f"         paced, a push every {GAP_US:.0f} us: tail {rng(paced)} ms; by phase: " + ", ".join(f"{nm} {rng([w[i] for w in paced_where])}" for i, nm in enumerate(names)), flush=True)
        out[f"{N // chunk}x{chunk}"] = dict(one_shot_ms=[min(a), max(a)], tail_ms=[min(tail), max(tail)], total_ms=[min(total), max(total)],
                                            paced_gap_us=GAP_US, paced_tail_ms=[min(paced), max(paced)])
    ctx.close(); pin.close()
    return out


res = {k: bench(k) for k in (["thin", "pedersen"] if KINDS == "both" else [KINDS])}
print(json.dumps(dict(tool="push_bench", n=N, runs=RUNS, ranges_ms=res)))
