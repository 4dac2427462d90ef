#!/usr/bin/env python3
"""What decoding a shared table once per ROW gives a node that holds its keys and inputs as wire bytes (avrf_pool_submit_shared_wire),
at the headline's shape: 65 536 items with one I/O pair each over 1 024 keys + 3 inputs, one pool of 144 slots / 12 lanes / 6 threads,
hash group 8, depth 3, validate = 1, page-locked buffers, the from-host cycle (every step stages its batch again from the host buffers).
Three arms run alternately in this one process and this one pool, three times each:
    wire         avrf_pool_submit_wire: every point of every item decoded on the device (four per item)
    shared_wire  avrf_pool_submit_shared_wire: the 1 027 rows once, then R and the output of every item (two per item)
    shared       avrf_pool_submit_shared on x || y points, nothing to decode: for context
Prints items/s per run, then per arm the runs and their median, the plain-wire arm's spread (max - min) and the ratios.
python tools/shared_wire_bench.py [n] [--quick] [--only=ARM] [--kind=thin|pedersen]
    --quick: one short run per arm; --only=wire | shared_wire | shared: that arm alone (a kernel trace of one arm)
    --kind=pedersen: the Pedersen verifier in a kind 2 pool over 3 inputs (avrf_pool_submit_pedersen_shared_wire: the 3 rows once, then the
                 output and Yb, R, Ok of every item -- four points per item against the plain wire call's five)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ark_vrf_amd import _native as nat  # noqa: E402
from shared_bench import PED, shared_items  # noqa: E402   (the items of its T = 1027 / T = 3 table; it reads the same [n] and --kind from the command line)

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 65536
QUICK = "--quick" in sys.argv
ONLY = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")), None)
SLOTS, LANES, THREADS, GROUP, DEPTH = 144, 12, 6, 8, 3
REPS, MIN_S = (1, 0.3) if QUICK else (3, 1.0)
VALIDATE = 1
ARMS = ("wire", "shared_wire", "shared")
median = lambda v: sorted(v)[len(v) // 2]


def batches(ctx):
    """the same verifying items three ways -> {arm: (page-locked batch, submit)}"""
    b = shared_items(ctx, 1024, 3)
    L = ctx.point_len
    pks, ios = ctx.points_compress(b["pks_xy"]), ctx.points_compress(b["ios_xy"])
    if PED:
        pts = ctx.points_compress(b"".join(b["proofs"][256 * j: 256 * j + 192] for j in range(n)))
        proofs = b"".join(pts[3 * L * j: 3 * L * (j + 1)] + b["proofs"][256 * j + 192: 256 * j + 256] for j in range(n))
        rows, input_index, outputs = nat.dedup_inputs_wire(ios, L)
        rows_xy, input_index_xy, outputs_xy = nat.dedup_inputs(b["ios_xy"])
        assert len(rows) // L == len(rows_xy) // 64 <= 3
        return {
            "wire": (nat.PinnedBatch(n, ios, b["io_counts"], b["ads"], b["ad_lens"], proofs=proofs), lambda pool, x: pool.submit_wire(x, validate=VALIDATE)),
            "shared_wire": (nat.PinnedPedersenSharedWireBatch(n, rows, input_index, outputs, b["io_counts"], b["ads"], b["ad_lens"], proofs, L),
                            lambda pool, x: pool.submit_pedersen_shared_wire(x, validate=VALIDATE)),
            "shared": (nat.PinnedPedersenSharedBatch(n, rows_xy, input_index_xy, outputs_xy, b["io_counts"], b["ads"], b["ad_lens"], b["proofs"]),
                       lambda pool, x: pool.submit_pedersen_shared(x)),
        }
    r = ctx.points_compress(b"".join(b["proofs"][96 * j: 96 * j + 64] for j in range(n)))
    proofs = b"".join(r[L * j: L * j + L] + b["proofs"][96 * j + 64: 96 * j + 96] for j in range(n))
    rows, pk_index, input_index, outputs = nat.dedup_points_wire(pks, ios, L)
    rows_xy, pk_index_xy, input_index_xy, outputs_xy = nat.dedup_points(b["pks_xy"], b["ios_xy"])
    assert len(rows) // L == len(rows_xy) // 64 <= 1027
    return {
        "wire": (nat.PinnedBatch(n, ios, b["io_counts"], b["ads"], b["ad_lens"], pks_xy=pks, proofs=proofs),
                 lambda pool, x: pool.submit_wire(x, validate=VALIDATE)),
        "shared_wire": (nat.PinnedSharedWireBatch(n, rows, pk_index, input_index, outputs, b["io_counts"], b["ads"], b["ad_lens"], proofs, L),
                        lambda pool, x: pool.submit_shared_wire(x, validate=VALIDATE)),
        "shared": (nat.PinnedSharedBatch(n, rows_xy, pk_index_xy, input_index_xy, outputs_xy, b["io_counts"], b["ads"], b["ad_lens"], b["proofs"]),
                   lambda pool, x: pool.submit_shared(x)),
    }


def main():
    assert ONLY is None or ONLY in ARMS, ONLY
    assert nat.set_blocking_sync(0, True) == 0
    ctx = nat.Context(0)
    arms = batches(ctx)
    ctx.close()
    run_arms = [a for a in ARMS if ONLY in (None, a)]
    out = dict(n=n, kind="pedersen" if PED else "thin", n_shared=arms["shared_wire"][0].n_shared, validate=VALIDATE, pool=dict(slots=SLOTS, lanes=LANES, threads=THREADS, hash_group=GROUP, depth=DEPTH),
               reps=REPS, min_seconds=MIN_S, runs=[])
    pool = nat.Pool(0, kind=2 if PED else 1, slots=SLOTS, lanes=LANES, threads=THREADS, hash_group=GROUP, depth=DEPTH)
    try:
        for rep in range(-1, REPS):                                               # rep -1: warm-up of every arm, not recorded
            for arm in run_arms:                                                  # alternately: every slot takes the arm's batch, then the cycle stages it again and again
                batch, submit = arms[arm]
                tk = [submit(pool, batch) for _ in range(SLOTS)]
                assert all(pool.wait(t) == 0 for t in tk)
                pool.stats(reset=True)
                done, mism, sec = pool.cycle(steps_block=SLOTS, min_seconds=0.2 if rep < 0 else MIN_S, from_host=True, expect=0)
                assert mism == 0
                st = pool.stats(reset=True)
                if rep < 0:
                    continue
                run = dict(arm=arm, mode="from_host", rep=rep, items_per_sec=round(done * n / sec), steps=done,
                           host_us_per_step=round(sum(st[k] for k in ("cpu_us_begin", "cpu_us_collect", "cpu_us_hash", "cpu_us_launch", "cpu_us_end")) / max(1, done), 1),
                           begin_us_per_step=round(st["cpu_us_begin"] / max(1, done), 1))
                out["runs"].append(run)
                print(json.dumps(run), flush=True)
        for arm in run_arms:
            v = [r["items_per_sec"] for r in out["runs"] if r["arm"] == arm]
            out[arm] = dict(items_per_sec=v, median=median(v), spread=max(v) - min(v))
        if ONLY is None:
            w, sw = out["wire"], out["shared_wire"]
            out["wire_spread"] = w["spread"]
            out["shared_wire_over_wire"] = round(sw["median"] / w["median"], 4)
            out["shared_wire_over_shared"] = round(sw["median"] / out["shared"]["median"], 4)
            out["not_below_wire_by_more_than_its_spread"] = sw["median"] >= w["median"] - w["spread"]
            if not PED:
                out["reaches_70M"] = sw["median"] >= 70e6
    finally:
        pool.close()
        for batch, _ in arms.values():
            batch.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
