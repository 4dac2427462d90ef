"""One fresh process of the MSM plan sweep (tests/test_gpu_msm_plans.py): python msm_plan_child.py CASE_FILE

The MSM engine reads its AVRF_* knobs once per process, so every case of the sweep is a process of its own, started by the test with
the knobs in the environment.  CASE_FILE is JSON, {set name: {"call": "msm" | "g1_msm" | "msm_segments", "suite": id, "bases": hex,
"scalars": hex, "n_seg": segments (msm_segments only)}}; every set is run through that method of Context(suite), and one JSON object
goes to stdout: {set name: {"out": hex, "plan": [c, windows, buckets per window, entries per lane]}}, the plan being what
avrf_kernel_stats reports after the call, or {set name: {"error": status}} when the call refused.  A set {"call": "ring_commit",
"suite": id, "srs": path of the SRS file, "keys": hex of 64-byte keys} indexes the keys with RingSetup(ctx, srs, 8) -- three KZG commits
of 512 terms in ONE avrf G1 MSM call on the setup's own lane -- and reports {"out": the ring commitment} (that lane's plan is not
readable from here).  Not a test: pytest does not collect it, and it knows nothing of the expected results."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def ring_commit(ctx, s):
    from ark_vrf_amd.ring import RingSetup
    with open(s["srs"], "rb") as f:
        setup = RingSetup(ctx, f.read(), 8)
    keys = bytes.fromhex(s["keys"])
    key = setup.index([keys[i: i + 64] for i in range(0, len(keys), 64)])
    try:
        return key.commitment
    finally:
        key.close()
        setup.close()


def main(path):
    from ark_vrf_amd import _native as nat
    with open(path) as f:
        sets = json.load(f)
    ctxs, out = {}, {}
    for name, s in sets.items():
        if s["suite"] not in ctxs:
            ctxs[s["suite"]] = nat.Context(s["suite"])
        ctx = ctxs[s["suite"]]
        if s["call"] == "ring_commit":
            out[name] = {"out": ring_commit(ctx, s).hex()}
            continue
        bases, scalars = bytes.fromhex(s["bases"]), bytes.fromhex(s["scalars"])
        try:
            if s["call"] == "msm_segments":
                got = b"".join(ctx.msm_segments(s["n_seg"], bases, scalars))
            else:
                got = getattr(ctx, s["call"])(bases, scalars)
        except nat.AvrfError as e:                                  # "avrf_msm_te -> -3": the status is all the sweep wants
            out[name] = {"error": int(str(e).rsplit("->", 1)[1])}
            continue
        plan = (C.c_int32 * 4)()
        assert nat.lib().avrf_kernel_stats(ctx._h, 0, None, None, plan) == 0
        out[name] = {"out": got.hex(), "plan": list(plan)}
    for ctx in ctxs.values():
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
