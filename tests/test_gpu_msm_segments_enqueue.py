"""GPU parity: the segmented MSM chain in its two halves (csrc/msm.h msm_te_segments_enqueue / msm_te_segments_finish), which the
pool's segmented jobs run, against the CPU oracle.

Python reaches the halves through the probe avrf_msm_te_segments_chain: ONE chain whatever n_seg is (avrf_msm_te_segments loops
single MSMs below eight segments), reported to the context's own record (finish waits for the stream) or to a record of the
call's own (finish does not wait, as with a pool slot's record).  The expectation is orc.msm on every segment alone; the results
are points, compared byte for byte."""
import random
from concurrent.futures import ThreadPoolExecutor

import pytest

import oracle as orc
from helpers import IDENTITY_XY, R_ORDER, xy

pytestmark = pytest.mark.gpu

_POINTS = {}


def points(suite):
    if suite not in _POINTS:
        g = orc.suite_point(suite, 0)
        rng = random.Random(70 + suite)
        _POINTS[suite] = [xy(suite, orc.smul(suite, rng.randrange(1, R_ORDER[suite]).to_bytes(32, "little"), g)) for _ in range(24)]
    return _POINTS[suite]


@pytest.fixture(scope="module")
def ctxs():
    from ark_vrf_amd import _native as nat
    made = {}

    class Lazy(dict):
        def __missing__(self, suite):
            made[suite] = self[suite] = nat.Context(suite)
            return self[suite]
    yield Lazy()
    for c in made.values():
        c.close()


_CASES = {}


def case(suite, n_seg, L):
    """(bases, scalars, expected points) per segment, computed once.  Segment 1 (or the only one when L > 1: its first half) has
    zero scalars throughout; every third term of the others is a zero scalar or -- twisted Edwards only -- the identity base; one
    segment repeats a single base under r - 1 (a heavy bucket and the top signed digit)."""
    if (suite, n_seg, L) not in _CASES:
        rng, pts, r = random.Random(1000 * n_seg + L + suite), points(suite), R_ORDER[suite]
        ident = None if suite == orc.SECP256R1 else IDENTITY_XY
        bases, scalars = [], []
        for v in range(n_seg):
            bs = [rng.choice(pts) for _ in range(L)]
            ss = [rng.randrange(r) for _ in range(L)]
            for t in range(0, L, 3):
                if (t // 3) % 2 == 0 or ident is None:
                    ss[t] = 0
                else:
                    bs[t] = ident
            if L == 1:
                ss = [rng.randrange(1, r)]
            if v == 1:
                ss = [0] * L                                            # all of this segment's scalars are zero
            if v == 2:
                bs, ss = [pts[0]] * L, [r - 1] * L
            if v == 0 and L > 4:
                ss[1], ss[2], ss[4] = 1, r - 1, r - 2
            bases.append(b"".join(bs)); scalars.append(b"".join(s.to_bytes(32, "little") for s in ss))
        with ThreadPoolExecutor(max_workers=8) as ex:
            want = list(ex.map(lambda v: orc.msm(suite, bases[v], scalars[v]), range(n_seg)))
        _CASES[suite, n_seg, L] = b"".join(bases), b"".join(scalars), want
    return _CASES[suite, n_seg, L]


SHAPES = [(n_seg, L) for n_seg in (1, 7, 8, 40) for L in (1, 5, 257)]


@pytest.mark.parametrize("own_record", [True, False])
@pytest.mark.parametrize("n_seg,L", SHAPES)
def test_chain_halves_match_oracle(ctxs, n_seg, L, own_record):
    """both sides of the eight-segment threshold of the synchronous call, window widths 4 (L = 1, 5) and 5 (257)"""
    bases, scalars, want = case(0, n_seg, L)
    got = ctxs[0].msm_segments_chain(n_seg, bases, scalars, own_record=own_record)
    assert got == want
    if n_seg > 1:
        assert got[1] == IDENTITY_XY                                    # all scalars zero: the identity
    # the synchronous call (which loops single MSMs below eight segments) agrees
    assert ctxs[0].msm_segments(n_seg, bases, scalars) == want


@pytest.mark.parametrize("own_record", [True, False])
@pytest.mark.parametrize("suite,n_seg,L", [(1, 7, 5), (1, 40, 257), (orc.SECP256R1, 1, 5), (orc.SECP256R1, 7, 257), (orc.SECP256R1, 8, 5)])
def test_chain_halves_other_suites(ctxs, suite, n_seg, L, own_record):
    """Baby-JubJub, and secp256r1: the generic device Horner (k_horner), and a suite whose plain chains take no caller's record --
    the segmented chain's finished points fit any record"""
    bases, scalars, want = case(suite, n_seg, L)
    assert ctxs[suite].msm_segments_chain(n_seg, bases, scalars, own_record=own_record) == want


def test_chain_refusals_and_empty(ctxs):
    import ctypes as C
    from ark_vrf_amd import _native as nat
    c, pts = ctxs[0], points(0)

    def call(n_seg, L, own):
        return nat.lib().avrf_msm_te_segments_chain(c._h, C.c_size_t(n_seg), C.c_size_t(L), nat._u8(pts[0] * (n_seg * L)), nat._u8(bytes(32 * n_seg * L)),
                                                   own, (C.c_uint8 * (64 * max(1, n_seg)))())
    for own in (0, 1):
        assert call(2, 8192, own) == -2                                 # a segment over AVRF_SEGMENT_TERMS_MAX: nothing launched
        assert call(1009, 5, own) == -2                                 # 1 009 x 65 virtual windows
        assert call(8, 5, own) == 0
        assert c.msm_segments_chain(0, b"", b"", own_record=bool(own)) == []
    # no terms at all: every segment's sum is the identity
    assert c.msm_segments_chain(3, b"", b"") == [IDENTITY_XY] * 3
    bases, scalars, want = case(0, 7, 5)
    assert c.msm_segments_chain(7, bases, scalars, own_record=False) == want   # the context still works
