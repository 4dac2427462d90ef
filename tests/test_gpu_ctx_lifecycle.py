"""Contexts and pools give their device memory back: free memory as the HIP runtime reports it (hipMemGetInfo) does not fall
over repeated create / run / close cycles of a Context and of a Pool.  Nothing in the library lists a context's buffers any
more -- every buffer is freed by the struct that holds it -- so this test is what says that they all come back.

The allowance comes from sizes, not from a run.  The smallest per-item buffer a context that verified a Thin batch holds is
d_pks, n x 64 bytes (more after the staging buffers' rounding): losing even that one per cycle costs K * n * 64 bytes, 52 MB
for n = 4096 and K = 200 -- far above allocator granularity -- and the test allows half of it.  The MSM workspace, the lane's
term arrays and the pool's per-slot records are all larger per cycle than that.

What the test cannot see: a lost buffer of a few hundred bytes (the flag words, the workspace's win_tot / plan words) stays
below allocator granularity at this K."""
import ctypes as C
import random

import pytest

import oracle as orc
from helpers import nat_batch, rand_points_xy, rand_scalar

pytestmark = pytest.mark.gpu
N, K = 4096, 200
ALLOWED = K * N * 64 // 2


def free_bytes():
    from ark_vrf_amd import _native as nat
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert nat.lib().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


@pytest.fixture(scope="module")
def thin():
    b = orc.gen_batch(orc.BANDERSNATCH, 0, N)
    assert all(c == 1 for c in b["io_counts"])
    return b


def test_context_cycles_return_memory(thin):
    from ark_vrf_amd import _native as nat
    assert K * N * 64 >= 32 * 10**6
    want = orc.thin_batch_verify_xy(orc.BANDERSNATCH, thin)
    assert want == 0
    ped = orc.gen_batch(orc.BANDERSNATCH, 1, 256)
    ped["pks_xy"] = b""
    rng = random.Random(7)
    pts = rand_points_xy(rng, orc.BANDERSNATCH, 3)
    sc = [rand_scalar(rng, orc.BANDERSNATCH) for _ in pts]
    b, pb = nat_batch(thin), nat_batch(ped)
    after_first = None
    for i in range(K):
        ctx = nat.Context(orc.BANDERSNATCH)
        assert ctx.thin_batch_stage(b) == 0
        st = ctx.thin_batch_run()
        if i == 0:                                                     # the verdict; then the other staged kind and the single-launch MSM through the same
            assert st == want                                          # context (in the FIRST cycle: what the runtime sets up once per process for a
                                                                       # kernel's first launch -- code objects, queue scratch -- is then part of the baseline)
            assert ctx.pedersen_batch_stage(pb) == 0
            assert ctx.pedersen_batch_run() == orc.pedersen_batch_verify_xy(orc.BANDERSNATCH, ped) == 0
            assert len(ctx.msm(b"".join(pts), b"".join(sc))) == 64
        ctx.close()
        if i == 0:
            after_first = free_bytes()
    after_last = free_bytes()
    print(f"context cycles: free after first {after_first}, after {K} {after_last}, drop {after_first - after_last}, allowed {ALLOWED}")
    assert abs(after_first - after_last) < ALLOWED


def test_pool_cycles_return_memory(thin):
    from ark_vrf_amd import _native as nat
    b = nat_batch(thin)
    after_first = None
    for i in range(K):
        pool = nat.Pool(orc.BANDERSNATCH, kind=1, slots=4, lanes=2, threads=2)
        tickets = [pool.submit(b) for _ in range(4)]                   # one batch per slot
        verdicts = [pool.wait(t) for t in tickets]
        pool.close()
        assert verdicts == [0, 0, 0, 0]
        if i == 0:
            after_first = free_bytes()
    after_last = free_bytes()
    print(f"pool cycles: free after first {after_first}, after {K} {after_last}, drop {after_first - after_last}, allowed {ALLOWED}")
    assert abs(after_first - after_last) < ALLOWED
