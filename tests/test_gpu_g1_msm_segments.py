"""GPU parity: avrf_g1_msm_segments -- n_seg independent G1 MSMs as ONE Pippenger chain of virtual windows, finished on the device by
k_g1_horner_wave (a wave per MSM: 64-way Horner over the bit sums, then the affine conversion) -- against the ring oracle's big-int
MSM and against avrf_g1_msm of every segment on its own.  Both pairing curves; bases are the reference's SRS points
(tests/golden/*.bin).  The call runs the chain for every n_seg >= 1, so one segment exercises the new kernel too."""
import os
import random

import pytest

from oracle import ring_py as R

pytestmark = pytest.mark.gpu
SRS = {0: "bls12-381-srs-2-11-uncompressed-zcash.bin", 1: "bn254-testing-2-9-uncompressed.bin"}
OK, INVALID_DATA, ERR_BAD_ARG = 0, 2, -2


@pytest.fixture(scope="module")
def env(golden_dir):
    from ark_vrf_amd import _native as nat
    out = {}
    for i in (0, 1):
        s = R.SUITES[i]
        srs = R.Srs(s, open(os.path.join(golden_dir, SRS[i]), "rb").read())
        out[i] = (s, srs, nat.Context(i))
    return out


def le(s, P):
    n = s.fp_bytes
    return bytes(2 * n) if P is None else P[0].to_bytes(n, "little") + P[1].to_bytes(n, "little")


def want(s, pts, ks):
    return le(s, R.g1_affine(s.p, R.g1_msm(s.p, pts, ks)))


def run(s, ctx, segs, L):
    """segs: list of (points, scalars) per segment, each at most L long; shorter ones are padded with zero scalars over all-zero bases"""
    bases = b"".join(b"".join(le(s, P) for P in pts) + bytes(2 * s.fp_bytes * (L - len(pts))) for pts, _ in segs)
    scal = b"".join(b"".join(k.to_bytes(32, "little") for k in ks) + bytes(32 * (L - len(ks))) for _, ks in segs)
    return ctx.g1_msm_segments(len(segs), L, bases, scal)


def check(s, ctx, segs, L, single=True):
    got = run(s, ctx, segs, L)
    assert isinstance(got, list) and len(got) == len(segs), got
    for v, (pts, ks) in enumerate(segs):
        assert got[v] == want(s, pts, ks), (v, L)
        if single:                                                       # avrf_g1_msm of the same segment
            assert got[v] == ctx.g1_msm(b"".join(le(s, P) for P in pts), b"".join(k.to_bytes(32, "little") for k in ks)), (v, L)
    return got


@pytest.mark.parametrize("suite", [0, 1])
@pytest.mark.parametrize("n_seg,L", [(1, 1), (1, 13), (7, 11), (8, 11), (9, 161), (33, 13)])
def test_shapes(env, suite, n_seg, L):
    """random scalars with 0, 1 and r - 1 among them; every segment over bases of its own (a slice of the SRS that moves with v)"""
    s, srs, ctx = env[suite]
    rng = random.Random(1000 * suite + 10 * n_seg + L)
    segs = []
    for v in range(n_seg):
        pts = [srs.g1[(7 * v + t) % 300] for t in range(L)]
        ks = [rng.randrange(s.r) for _ in range(L)]
        if L >= 3:
            ks[(v + 0) % L], ks[(v + 1) % L], ks[(v + 2) % L] = 0, 1, s.r - 1
        else:
            ks[0] = [s.r - 1, 1, 0][v % 3]
        segs.append((pts, ks))
    check(s, ctx, segs, L)


@pytest.mark.parametrize("suite", [0, 1])
@pytest.mark.parametrize("L", [11, 161, 257])
def test_both_ends_of_the_horner_split(env, suite, L):
    """A segment whose only non-zero scalar is 1 (only bit sum 0, lane 0's last addition), one whose only non-zero scalar is the
    largest power of two below r (only the top lanes' bit sums, shifted by the whole tree) and one with r - 1 (every window).
    The kernel folds m = ceil(nbits / 64) bit sums per lane, nbits = windows x c.  msm_plan gives L = 11 AND L = 161 the same c = 4
    (c = log2 L - 3, floored at 4): nbits = 256 on both curves, a multiple of 64, m = 4, no lane reads beyond nbits.  L = 257 is the
    smallest L with c = 5: nbits = 260 (BLS12-381, 255-bit r) or 255 (BN254, 254-bit r), NOT a multiple of 64 -- lanes whose bit sums
    lie at or beyond nbits count the identity.  The window bits come from the layout call (host arithmetic), not from this text."""
    from ark_vrf_amd import _native as nat
    s, srs, ctx = env[suite]
    lay = nat.thin_segments_layout([1], [(L - 3) // 2])                # a Thin segment of 2 + 2 pairs + 1 = L terms: { L, .., .., c }
    assert lay[0] == L
    c = lay[3]
    nbits = c * -(-(s.r.bit_length() + 1) // c)
    assert (nbits % 64 == 0) == (L != 257), (L, c, nbits)
    top = 1 << (s.r.bit_length() - 1)
    assert top < s.r < 2 * top
    segs = []
    for v, k in enumerate((1, top, s.r - 1)):
        pts = [srs.g1[(5 * v + t) % 300] for t in range(L)]
        ks = [0] * L
        ks[L - 1 - v] = k
        segs.append((pts, ks))
    got = check(s, ctx, segs, L)
    assert got[0] == le(s, segs[0][0][L - 1])                          # 1 * P by value


@pytest.mark.parametrize("suite", [0, 1])
@pytest.mark.parametrize("L", [11, 161])
def test_where_the_xyzz_law_is_incomplete(env, suite, L):
    s, srs, ctx = env[suite]
    rng = random.Random(77 + suite + L)
    P, Q = srs.g1[3], srs.g1[7]
    negP = (P[0], (-P[1]) % s.p)
    k = rng.randrange(1, s.r)
    ordinary = lambda a: ([srs.g1[a + t] for t in range(L)], [rng.randrange(s.r) for _ in range(L)])
    a, b = ordinary(20), ordinary(40)
    segs = [
        ([P] * L, [1] * L),                                              # one base L times: every addition is a doubling
        ([P, negP], [k, k]),                                             # cancels
        ([P, None, Q], [k, 5, 7]),                                       # a base at infinity
        a,
        ([srs.g1[60 + t] for t in range(L)], [0] * L),                   # all-zero scalars between two ordinary segments
        b,
    ]
    got = check(s, ctx, segs, L)
    assert got[0] == le(s, R.g1_affine(s.p, R.g1_mul(s.p, (P[0], P[1], 1), L)))
    assert got[1] == bytes(2 * s.fp_bytes) and got[4] == bytes(2 * s.fp_bytes)
    assert run(s, ctx, [a, b], L) == [got[3], got[5]]                    # the neighbours' results without the empty one between them


@pytest.mark.parametrize("suite", [0, 1])
def test_padding(env, suite):
    """segments shorter than L carry zero scalars over all-zero bases (what the ring verifier's padded vectors look like)"""
    s, srs, ctx = env[suite]
    rng = random.Random(5 + suite)
    segs = [([srs.g1[11 * v + t] for t in range(n)], [rng.randrange(s.r) for _ in range(n)]) for v, n in enumerate([11, 1, 0, 7, 2, 10, 3, 11, 5])]
    got = check(s, ctx, segs, 11)
    assert got[2] == bytes(2 * s.fp_bytes)


def test_no_terms(env):
    s, srs, ctx = env[0]
    assert ctx.g1_msm_segments(3, 0, b"", b"") == [bytes(96)] * 3
    assert ctx.g1_msm_segments(0, 5, b"", b"") == []


@pytest.mark.parametrize("suite", [0, 1])
def test_refusals(env, suite):
    s, srs, ctx = env[suite]
    fq = s.fp_bytes
    assert ctx.g1_msm_segments(1, 8192, bytes(2 * fq * 8192), bytes(32 * 8192)) == ERR_BAD_ARG
    assert ctx.g1_msm_segments(1, 8191, bytes(2 * fq * 8191), bytes(32 * 8191)) == [bytes(2 * fq)]     # the limit itself is served
    pts = [srs.g1[t] for t in range(4)]
    good = b"".join(le(s, P) for P in pts)
    one = (1).to_bytes(32, "little")
    assert ctx.g1_msm_segments(2, 2, good, one * 3 + s.r.to_bytes(32, "little")) == INVALID_DATA       # a scalar = r
    bad = good[: 2 * fq] + s.p.to_bytes(fq, "little") + good[3 * fq:]                                  # a coordinate = p
    assert ctx.g1_msm_segments(2, 2, bad, one * 4) == INVALID_DATA
    assert ctx.g1_msm_segments(2, 2, good, one * 4) == [want(s, pts[:2], [1, 1]), want(s, pts[2:], [1, 1])]   # and the context still serves
