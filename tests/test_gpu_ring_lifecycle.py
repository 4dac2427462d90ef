"""Ring handles give their device memory back: free memory as the HIP runtime reports it (hipMemGetInfo) does not fall over
repeated create / close cycles of a VerifierKeyBuilder, of a ring key, and of a whole setup that has proved on both lanes.

The thresholds come from sizes, not from runs.  A ring key holds the ring's cap - 1 points as 96-byte te_pre entries
(cap = N - 3; N = 512 for a ring of 8 over the committed 2^11 SRS: 508 points, 48 768 bytes): the smallest device buffer a
builder or a key owns, so losing even that one per cycle is 34 MB after K = 700 cycles -- far above allocator granularity --
and the test allows half of it.  For whole setups the allowance is half of one setup's footprint."""
import ctypes as C
import json
import os

import pytest

from helpers import xy

pytestmark = pytest.mark.gpu
K = 700
TE_PRE_BYTES = 96


def free_bytes():
    from ark_vrf_amd import _native as nat
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert nat.lib().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


@pytest.fixture(scope="module")
def env(golden_dir):
    from ark_vrf_amd import _native as nat
    ctx = nat.Context(0)
    srs = open(os.path.join(golden_dir, "bls12-381-srs-2-11-uncompressed-zcash.bin"), "rb").read()
    v = json.load(open(os.path.join(golden_dir, "bandersnatch_sha-512_ell2_ring.json")))[0]
    raw = bytes.fromhex(v["ring_pks"])
    pks = [xy(0, raw[32 * i: 32 * i + 32]) for i in range(len(raw) // 32)]
    yield ctx, srs, pks, v
    ctx.close()


def smallest_buffer_total(setup):
    """K times the smallest device buffer of a key: the te_pre points."""
    assert setup.domain_size == 512
    cap = setup.domain_size - 3
    return K * (cap - 1) * TE_PRE_BYTES


def test_builder_cycles_return_memory(env):
    from ark_vrf_amd.ring import RingSetup, VerifierKeyBuilder
    ctx, srs, pks, v = env
    setup = RingSetup(ctx, srs, 8)
    total = smallest_buffer_total(setup)
    assert total >= 32 * 10**6
    after_first = None
    for i in range(K):
        b = VerifierKeyBuilder(setup)
        if i == 0:
            assert b.append(pks) == 0 and b.finalize().hex() == v["ring_pks_com"]
        b.close()
        if i == 0:
            after_first = free_bytes()
    after_last = free_bytes()
    setup.close()
    print(f"builder cycles: free after first {after_first}, after {K} {after_last}, drop {after_first - after_last}, allowed {total // 2}")
    assert abs(after_first - after_last) < total // 2


def test_index_cycles_return_memory(env):
    from ark_vrf_amd.ring import RingSetup
    ctx, srs, pks, v = env
    setup = RingSetup(ctx, srs, 8)
    total = smallest_buffer_total(setup)
    after_first = None
    for i in range(K):
        key = setup.index(pks)
        if i == 0:
            assert key.commitment.hex() == v["ring_pks_com"]
        key.close()
        if i == 0:
            after_first = free_bytes()
    after_last = free_bytes()
    setup.close()
    print(f"index cycles: free after first {after_first}, after {K} {after_last}, drop {after_first - after_last}, allowed {total // 2}")
    assert abs(after_first - after_last) < total // 2


def test_setup_cycles_with_two_lanes_return_memory(env):
    """Whole setups that proved 32 proofs -- two chunks of 16, one per lane, so the second lane's stream, scratch and MSM
    workspace exist -- on the bucket form (budget 0: no table of all multiples, whose registry is another resource)."""
    from ark_vrf_amd.ring import RingSetup
    ctx, srs, pks, v = env
    idx = pks.index(xy(0, bytes.fromhex(v["pk"])))
    cycles, n = 8, 32
    footprint = after_first = None
    for i in range(cycles):
        before = free_bytes()
        setup = RingSetup(ctx, srs, 8)
        setup.set_table_budget(0)
        key = setup.index(pks)
        proofs = key.prove([idx] * n, [bytes.fromhex(v["blinding"])] * n)
        if i == 0:
            assert proofs == [bytes.fromhex(v["ring_proof"])] * n
            footprint = before - free_bytes()
        key.close()
        setup.close()
        if i == 0:
            after_first = free_bytes()
    after_last = free_bytes()
    print(f"setup cycles: footprint {footprint}, free after first {after_first}, after {cycles} {after_last}, drop {after_first - after_last}")
    assert footprint > 0
    assert abs(after_first - after_last) < footprint // 2
