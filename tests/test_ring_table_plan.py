"""The shape of the ring prover's tables of all multiples (include/avrf.h avrf_ring_table_bytes) against an independent
restatement, and the explicit-budget plan rule that tests/test_gpu_ring_tables.py checks on the device.  Host arithmetic only."""
import pytest

# scalar field of the pairing curve: BLS12-381 Fr (255 bits), BN254 Fr (254 bits); affine Montgomery points of 96 / 64 bytes
R_ORDER = {0: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
           1: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
FR_BITS = {0: 255, 1: 254}
POINT_BYTES = {0: 96, 1: 64}
RING_SUITES = (0, 1, 2, 4, 5)


def curve_of(suite):
    return 1 if suite == 1 else 0


def bases(suite, ring_size, kind):
    """3N + 1 SRS powers (kind 0) or 2N + 1 witness bases (kind 1), N the PIOP domain of the ring."""
    from ark_vrf_amd import _native as nat
    import ctypes as C
    f = nat.lib().avrf_ring_pcs_domain_size
    f.restype = C.c_size_t
    pcs = f(int(suite), C.c_size_t(ring_size))
    return pcs if kind == 0 else 2 * ((pcs - 1) // 3) + 1


def table_shape(curve, n, c):
    """(rows, points, bytes): R = ceil(bits / c) digit rows of 2^(c-1) multiples each, the top row cut to the largest digit r - 1
    reaches there, and one carry row (one multiple) when that digit exceeds 2^(c-1)."""
    R = -(-FR_BITS[curve] // c)
    half = 1 << (c - 1)
    top = ((R_ORDER[curve] - 1) >> (c * (R - 1))) + 1
    mult = [half] * (R - 1) + [min(top, half)] + ([1] if top > half else [])
    points = sum(mult) * n
    return len(mult), points, points * POINT_BYTES[curve]


def expected_bytes(suite, ring_size, kind, c):
    if suite not in RING_SUITES or not 8 <= c <= 16:
        return 0
    _, points, nbytes = table_shape(curve_of(suite), bases(suite, ring_size, kind), c)
    return nbytes if points < (1 << 31) - 1 else 0


def bucket_width(suite, ring_size):
    """The setup's fixed-base window (avrf_ring_setup_plan out[0] before any table): floor(log2(3N + 1)), one less on BN254, in [8, 13]."""
    lg = bases(suite, ring_size, 0).bit_length() - 1
    c = lg if curve_of(suite) == 0 else lg - 1
    return min(max(c, 8), 13)


def plan(suite, ring_size, budget, table_bytes):
    """The explicit-budget rule: the SRS table the widest c in [bucket width, 16] that fits the budget, then the witness table the
    widest c in [8, 16] that fits what is left.  Returns ((c, bytes) SRS, (c, bytes) witness), c = 0 for no table."""
    out = []
    for kind, lo in ((0, max(bucket_width(suite, ring_size), 8)), (1, 8)):
        got = (0, 0)
        for c in range(16, lo - 1, -1):
            b = table_bytes(suite, ring_size, kind, c)
            if b and b <= budget:
                got = (c, b)
                budget -= b
                break
        out.append(got)
    return tuple(out)


@pytest.mark.parametrize("suite", RING_SUITES)
def test_table_bytes_matches_restatement(suite):
    from ark_vrf_amd.ring import table_bytes
    for ring in (8, 1024, 4096):
        for kind in (0, 1):
            for c in range(7, 18):
                assert table_bytes(suite, ring, kind, c) == expected_bytes(suite, ring, kind, c), (suite, ring, kind, c)


def test_table_bytes_anchors():
    from ark_vrf_amd.ring import table_bytes
    assert table_bytes(0, 1024, 0, 15) == 164_309_827_680                  # 1.71 G points
    assert table_shape(0, 6145, 15)[1] == 1_711_560_705
    assert table_bytes(1, 4096, 0, 13) == 122_564_122_688
    assert table_bytes(0, 1024, 1, 14) == 57_999_360_768
    assert table_shape(0, 6145, 16)[1] > (1 << 31)                         # 3.2 G points: over the 31-bit entry indices
    assert table_bytes(0, 1024, 0, 16) == 0
    assert table_bytes(1, 4096, 0, 15) == table_bytes(1, 4096, 0, 16) == 0
    for kind in (0, 1):
        for ring in (8, 1024):
            assert table_bytes(3, ring, kind, 12) == 0                     # Ed25519: no ring
            assert table_bytes(0, ring, kind, 7) == table_bytes(0, ring, kind, 17) == 0
    assert table_bytes(0, 8, 2, 12) == 0 and table_bytes(0, 0, 0, 12) == 0


def test_bucket_width_and_plans_of_the_gpu_tests():
    """The budgets tests/test_gpu_ring_tables.py proves with give the widths it expects (ring 8: N = 512)."""
    from ark_vrf_amd.ring import table_bytes
    assert bucket_width(0, 8) == 10 and bucket_width(1, 8) == 9
    assert bucket_width(0, 1024) == 12 and bucket_width(1, 4096) == 13
    pairs = {0: [(10, 8), (12, 11), (14, 14)], 1: [(9, 8), (11, 10), (13, 13)]}
    for suite, ps in pairs.items():
        for cs, cw in ps:
            budget = table_bytes(suite, 8, 0, cs) + table_bytes(suite, 8, 1, cw)
            (pc, pb), (wc, wb) = plan(suite, 8, budget, table_bytes)
            assert (pc, wc) == (cs, cw) and pb + wb == budget, (suite, cs, cw)
    assert table_bytes(0, 8, 0, 10) + table_bytes(0, 8, 1, 8) == 2_294_810_208
    assert plan(0, 8, 10**9, table_bytes) == ((0, 0), (9, table_bytes(0, 8, 1, 9)))   # below the SRS minimum: witness table only
    assert plan(0, 8, 0, table_bytes) == ((0, 0), (0, 0))
    (pc, _), (wc, _) = plan(1, 4096, 130 * 10**9, table_bytes)
    assert (pc, wc) == (13, 8)                                              # the benchmark's BN254 shape
