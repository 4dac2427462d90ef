#!/usr/bin/env python3
"""What the shared-table Thin batch verifier (avrf_thin_batch_stage_shared / avrf_pool_submit_shared) gives at the headline's shape:
one pool of 144 slots / 12 lanes / 6 threads, 65 536 items with one I/O pair each, resident cycle mode and the from-host cycle.
For every table size the plain batch (the EXPANDED form of the same items) and its shared staging run alternately in the same
process, three times each: items/s, and k_accumulate milliseconds and launches per run from avrf_pool_stats.
    T = 1 027    1 024 keys + 3 inputs: what a validator set's block / seal batch looks like
    T = 1        every key and every input the SAME row (the input is the key's own point, the output sk * pk): one row of 131 072
                 references, the segmented sum's worst imbalance -- one block of k_shared_merge adds 16 384 partials, 64 per thread
    T = 131 072  nothing shared: the same term count as the plain call plus the extra pass
python tools/shared_bench.py [n] [--quick] [--only=LABEL] [--kind=thin|pedersen]
    --quick: one short run per arm; --only=T=1027 | T=1 | T=2n: that table alone (a kernel trace per table keeps the tables' kernel times apart)
    --kind=pedersen: the Pedersen verifier over a table of shared INPUTS (avrf_pool_submit_pedersen_shared against avrf_pool_submit in a
                 kind 2 pool of the same shape), tables  T=3  (3 inputs: the ticket workload)  and  T=n  (nothing shared: every input its own row)"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle as orc  # noqa: E402
from ark_vrf_amd import _native as nat  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 65536
QUICK = "--quick" in sys.argv
ONLY = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")), None)
KIND = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--kind=")), "thin")
assert KIND in ("thin", "pedersen"), KIND
PED = KIND == "pedersen"
SLOTS, LANES, THREADS, GROUP, DEPTH = 144, 12, 6, 8, 3
REPS, MIN_S = (1, 0.3) if QUICK else (3, 1.0)


def shared_items(ctx, n_keys, n_inputs):
    """n verifying items over n_keys keys and n_inputs inputs (proofs by the device's prover) as an expanded batch dict;
    n_inputs = 0: the one input is key 0's own point, so that with n_keys = 1 every reference names the same point"""
    rng = random.Random(n_keys)
    keys = [orc.from_seed(0, k.to_bytes(4, "little") + bytes(28)) for k in range(n_keys)]
    inputs = [orc.hash_to_curve(0, b"slot-%d" % i) for i in range(n_inputs)] or [keys[0][1]]
    n_inputs = len(inputs)
    xy = lambda p: orc.point_decompress(0, p)[1]
    kxy, ixy = [xy(pk) for _, pk in keys], [xy(h) for h in inputs]
    oxy = {(k, i): xy(orc.vrf_output(0, keys[k][0], inputs[i])) for k in range(n_keys) for i in range(n_inputs)}
    ks, ii = [rng.randrange(n_keys) for _ in range(n)], [rng.randrange(n_inputs) for _ in range(n)]
    ads = [b"%08d" % j for j in range(n)]
    b = dict(n=n, pks_xy=b"".join(kxy[k] for k in ks), ios_xy=b"".join(ixy[i] + oxy[k, i] for k, i in zip(ks, ii)), io_counts=[1] * n,
             ads=b"".join(ads), ad_lens=[8] * n, sks=b"".join(keys[k][0] for k in ks))
    pb = nat.Batch(n, b["ios_xy"], b["io_counts"], b["ads"], b["ad_lens"], pks_xy=b["pks_xy"], sks=b["sks"])
    b["proofs"] = ctx.pedersen_prove(pb)[0] if PED else ctx.thin_prove(pb)
    return b


def arms(b):
    if PED:
        shared_xy, input_index, outputs_xy = nat.dedup_inputs(b["ios_xy"])
        plain = nat.PinnedBatch(n, b["ios_xy"], b["io_counts"], b["ads"], b["ad_lens"], proofs=b["proofs"])
        shared = nat.PinnedPedersenSharedBatch(n, shared_xy, input_index, outputs_xy, b["io_counts"], b["ads"], b["ad_lens"], b["proofs"])
        return plain, shared
    shared_xy, pk_index, input_index, outputs_xy = nat.dedup_points(b["pks_xy"], b["ios_xy"])
    plain = nat.PinnedBatch(n, b["ios_xy"], b["io_counts"], b["ads"], b["ad_lens"], pks_xy=b["pks_xy"], proofs=b["proofs"])
    shared = nat.PinnedSharedBatch(n, shared_xy, pk_index, input_index, outputs_xy, b["io_counts"], b["ads"], b["ad_lens"], b["proofs"])
    return plain, shared


def measure(label, b, out):
    plain, shared = arms(b)
    pools = {}
    try:
        for arm, batch in (("plain", plain), ("shared", shared)):
            pool = pools[arm] = nat.Pool(0, kind=2 if PED else 1, slots=SLOTS, lanes=LANES, threads=THREADS, hash_group=GROUP, depth=DEPTH)
            submit = pool.submit if arm == "plain" else pool.submit_pedersen_shared if PED else pool.submit_shared
            tk = [submit(batch) for _ in range(SLOTS)]
            assert all(pool.wait(t) == 0 for t in tk)
            pool.cycle(steps_block=SLOTS, min_seconds=0.2, expect=0)              # warm-up
        res = out[label] = dict(n_shared=shared.n_shared, terms_plain=5 * n + 2 if PED else 4 * n + 1,
                                terms_shared=nat.pedersen_shared_n_terms(n, shared.n_shared) if PED else nat.thin_shared_n_terms(n, n, shared.n_shared), runs=[])
        for rep in range(REPS):
            for arm in ("plain", "shared"):                                       # alternately, in this one process
                for from_host in (False, True):
                    pool = pools[arm]
                    pool.stats(reset=True)
                    done, mism, sec = pool.cycle(steps_block=SLOTS, min_seconds=MIN_S, from_host=from_host, expect=0)
                    assert mism == 0
                    st = pool.stats(reset=True)
                    run = dict(arm=arm, mode="from_host" if from_host else "resident", rep=rep, items_per_sec=round(done * n / sec), steps=done,
                               accumulate_ms_per_step=round(st["accumulate_ms_total"] / max(1, done), 4), accumulate_launches_per_step=round(st["accumulate_launches"] / max(1, done), 2),
                               host_us_per_step=round(sum(st[k] for k in ("cpu_us_begin", "cpu_us_collect", "cpu_us_hash", "cpu_us_launch", "cpu_us_end")) / max(1, done), 1))
                    res["runs"].append(run)
                    print(label, json.dumps(run), flush=True)
        for mode in ("resident", "from_host"):
            v = {arm: [r["items_per_sec"] for r in res["runs"] if r["arm"] == arm and r["mode"] == mode] for arm in ("plain", "shared")}
            res[mode] = dict(plain=v["plain"], shared=v["shared"], plain_spread=max(v["plain"]) - min(v["plain"]),
                             shared_over_plain=round(sorted(v["shared"])[len(v["shared"]) // 2] / sorted(v["plain"])[len(v["plain"]) // 2], 4))
    finally:
        for pool in pools.values():
            pool.close()
        plain.close(); shared.close()


def main():
    assert nat.set_blocking_sync(0, True) == 0
    ctx = nat.Context(0)
    out = dict(n=n, kind=KIND, pool=dict(slots=SLOTS, lanes=LANES, threads=THREADS, hash_group=GROUP, depth=DEPTH), reps=REPS, min_seconds=MIN_S)
    tables = {"T=1027": lambda: shared_items(ctx, 1024, 3), "T=1": lambda: shared_items(ctx, 1, 0),
              "T=2n": lambda: orc.gen_batch(0, 0, n, threads=16)}
    if PED:
        tables = {"T=3": lambda: shared_items(ctx, 1024, 3), "T=n": lambda: orc.gen_batch(0, 1, n, threads=16)}
    for label, make in tables.items():
        if ONLY == label or (ONLY is None and not (QUICK and label in ("T=2n", "T=n"))):
            measure(label, make(), out)
    assert ONLY is None or ONLY in out, ONLY
    assert "T=1" not in out or out["T=1"]["n_shared"] == 1
    ctx.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
