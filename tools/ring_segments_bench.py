#!/usr/bin/env python3
"""What the segmented ring verifier (avrf_ring_batch_verify_segments) gives against the calls it competes with, on one MI355X, in ONE
process on ONE setup: n = 4 096 valid ring proofs over one ring of 1 024 keys (Bandersnatch / BLS12-381), the legs run alternately,
REPS timed repetitions each after one warm-up, ranges printed.
    a  ring_batch_verify_segments as 256 x 16, 64 x 64 and 16 x 256 segments: one verdict per segment
    b  ring_verify_each on the same items: one verdict per ITEM
    c  ring_batch_verify on all of them: one verdict
    d  n_seg separate ring_batch_verify calls, for each shape of leg a: what a caller with groups could do before
Every leg goes through the C ABI with its byte buffers built once (no per-call joins on the Python side).
After the legs one segmented run of every shape is repeated in a child process with AVRF_RING_TRACE set (the laps are read once per
process, and they print on every call), from the same proofs, and its laps are printed: where the time of a call goes.
python tools/ring_segments_bench.py [n] [ring] [--reps=K] [--legs=abcd] [--no-trace] [--proofs=FILE]
    --legs: only these legs (a kernel trace of leg a alone keeps the chain's kernels apart from the other legs' k_g1_lincomb)
    --proofs=FILE: keep the proofs in FILE and take them from there when it exists (a kernel trace then holds no prover kernel)"""
import ctypes as C
import os
import pickle
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ark_vrf_amd import _native as nat  # noqa: E402
from ark_vrf_amd.ring import RingSetup  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
opt = lambda name, default: next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--" + name + "=")), default)
N = int(args[0]) if args else 4096
RING = int(args[1]) if len(args) > 1 else 1024
REPS = int(opt("reps", "5"))
LEGS = opt("legs", "abcd")
TRACE_FROM = opt("trace-from", None)
PROOFS = opt("proofs", None)
SHAPES = [(N // k, k) for k in (16, 64, 256)]                                    # (segments, items per segment)
SRS = os.path.join(ROOT, "tests", "golden", "bls12-381-srs-2-11-uncompressed-zcash.bin")


def make_proofs(ctx, setup):
    import bench
    sks = bench.derive_scalars(b"rsb-sk", 0, RING, bench.R_BANDERSNATCH)
    pks = ctx.scalar_mul_base(sks)
    pkl = [pks[64 * i: 64 * i + 64] for i in range(RING)]
    setup.set_table_budget(0)                                                  # bucket form: no table of all multiples for a one-off proving run
    key = setup.index(pkl)
    idx = [(7 * j + 3) % RING for j in range(N)]
    inputs = ctx.scalar_mul_base(bench.derive_scalars(b"rsb-in", 0, N, bench.R_BANDERSNATCH))
    psk = b"".join(sks[32 * k: 32 * k + 32] for k in idx)
    ppk = b"".join(pkl[k] for k in idx)
    outs = ctx.scalar_mul(psk, inputs)
    ios = b"".join(inputs[64 * j: 64 * j + 64] + outs[64 * j: 64 * j + 64] for j in range(N))
    ads = [b"ad-%d" % j for j in range(N)]
    ped, blind = ctx.pedersen_prove(nat.Batch(N, ios, [1] * N, b"".join(ads), [len(a) for a in ads], pks_xy=ppk, sks=psk))
    proofs = key.prove(idx, [blind[32 * j: 32 * j + 32] for j in range(N)])
    com = key.commitment
    key.close()
    return com, b"".join(ped[256 * j: 256 * j + 64] for j in range(N)), b"".join(proofs)


class Calls:
    """the four calls over prebuilt buffers"""

    def __init__(self, setup, com, ybs, proofs):
        self.L, self.h, self.plen = nat.lib(), setup._h, setup.proof_len
        self.com, self.ybs, self.proofs = nat._u8(com), nat._u8(ybs), nat._u8(proofs)
        self.status = (C.c_int32 * N)()
        self.slices = {}
        for n_seg, k in SHAPES:
            self.slices[k] = [(nat._u8(ybs[64 * v * k: 64 * (v + 1) * k]), nat._u8(proofs[self.plen * v * k: self.plen * (v + 1) * k])) for v in range(n_seg)]

    def segments(self, n_seg, k):
        rc = self.L.avrf_ring_batch_verify_segments(self.h, C.c_size_t(N), self.com, C.c_size_t(1), None, self.ybs, self.proofs, C.c_size_t(n_seg),
                                                    nat._u32([k] * n_seg), self.status)
        assert rc == 0 and not any(self.status[:n_seg]), rc

    def each(self):
        rc = self.L.avrf_ring_verify_each(self.h, C.c_size_t(N), self.com, C.c_size_t(1), None, self.ybs, self.proofs, self.status)
        assert rc == 0 and not any(self.status), rc

    def batch(self):
        assert self.L.avrf_ring_batch_verify(self.h, C.c_size_t(N), self.com, C.c_size_t(1), None, self.ybs, self.proofs) == 0

    def separate(self, k):
        for yb, pr in self.slices[k]:
            assert self.L.avrf_ring_batch_verify(self.h, C.c_size_t(k), self.com, C.c_size_t(1), None, yb, pr) == 0


def main():
    ctx = nat.Context(0)
    setup = RingSetup(ctx, open(SRS, "rb").read(), RING)
    if TRACE_FROM:                                                             # the child: one traced segmented run per shape
        com, ybs, proofs = pickle.load(open(TRACE_FROM, "rb"))
        calls = Calls(setup, com, ybs, proofs)
        for n_seg, k in SHAPES:
            calls.segments(n_seg, k)                                           # warm: workspaces, pairing tables
        for n_seg, k in SHAPES:
            sys.stderr.write("laps of one segmented run, %d x %d:\n" % (n_seg, k)); sys.stderr.flush()
            calls.segments(n_seg, k)
        return
    t0 = time.perf_counter()
    if PROOFS and os.path.exists(PROOFS):
        com, ybs, proofs = pickle.load(open(PROOFS, "rb"))
        assert len(ybs) == 64 * N and len(proofs) == setup.proof_len * N
    else:
        com, ybs, proofs = make_proofs(ctx, setup)
        if PROOFS:
            pickle.dump((com, ybs, proofs), open(PROOFS, "wb"))
    print("ring %d, %d proofs ready in %.1f s; %d timed repetitions per leg after one warm-up" % (RING, N, time.perf_counter() - t0, REPS), flush=True)
    calls = Calls(setup, com, ybs, proofs)
    legs = []
    if "a" in LEGS:
        legs += [("a segments %4d x %-3d" % (n_seg, k), (lambda n_seg=n_seg, k=k: calls.segments(n_seg, k))) for n_seg, k in SHAPES]
    if "b" in LEGS:
        legs.append(("b ring_verify_each     ", calls.each))
    if "c" in LEGS:
        legs.append(("c ring_batch_verify    ", calls.batch))
    if "d" in LEGS:
        legs += [("d %4d separate x %-3d " % (n_seg, k), (lambda k=k: calls.separate(k))) for n_seg, k in SHAPES]
    times = {name: [] for name, _ in legs}
    for name, fn in legs:
        fn()                                                                   # warm-up
    for rep in range(REPS):
        for name, fn in legs:                                                  # alternately: a drift of the box touches every leg alike
            t = time.perf_counter()
            fn()
            times[name].append(1e3 * (time.perf_counter() - t))
    for name, _ in legs:
        v = sorted(times[name])
        print("%s  %8.2f .. %8.2f ms  (median %8.2f)  %8.0f .. %8.0f proofs/s" % (name, v[0], v[-1], v[len(v) // 2], N / v[-1] * 1e3, N / v[0] * 1e3), flush=True)
    if "--no-trace" not in sys.argv and "a" in LEGS:
        with tempfile.NamedTemporaryFile(suffix=".pkl", delete=False) as f:
            pickle.dump((com, ybs, proofs), f)
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), str(RING), "--trace-from=" + f.name], env=dict(os.environ, AVRF_RING_TRACE="1"),
                                 capture_output=True, text=True, timeout=600)
            text = res.stderr[res.stderr.find("laps of one segmented run"):] if "laps of one segmented run" in res.stderr else res.stderr
            print(text if res.returncode == 0 else "trace child failed (%d):\n%s" % (res.returncode, res.stderr), flush=True)
        finally:
            os.unlink(f.name)
    setup.close()
    ctx.close()


if __name__ == "__main__":
    main()
