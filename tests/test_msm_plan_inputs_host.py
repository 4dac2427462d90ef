"""The inputs of the MSM plan sweep (tests/msm_plan_inputs.py) have what each plan needs, checked on the CPU: k_digits' signed recoding
restated in Python, applied to `mix` for every window width 4 .. 15 and every group order the sweep uses.  These are conditions on
the inputs: when one fails, the inputs change, not the condition."""
import pytest

import msm_plan_inputs as mpi
from helpers import R_ORDER

# the group orders of the five chains: Bandersnatch, Baby-JubJub, secp256r1; G1 of BLS12-381 and of BN254
ORDERS = {"te0": R_ORDER[0], "te1": R_ORDER[1], "te7": R_ORDER[7],
          "g1_0": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
          "g1_1": 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001}
SEED = 4100


@pytest.fixture(scope="module", params=sorted(ORDERS))
def mix(request):
    r = ORDERS[request.param]
    terms, k0, k1 = mpi.mix_terms(r, SEED)
    assert all(0 <= k < r for _, _, k in terms)
    return r, terms, k0, k1


def test_digit_patterns():
    for c in range(3, 16):
        top, neg = mpi.digit_patterns(c)
        nw, nb = 248 // c, 1 << (c - 1)
        assert mpi.recode(top, c, nw + 1) == [(nb, False)] * nw + [(0, False)]
        d = mpi.recode(neg, c, nw + 1)
        assert d[0] == (nb - 1, True) and d[1:nw] == [(nb - 2, True)] * (nw - 1) and d[nw] == (1, False)


def test_recode_is_the_scalar():
    r = ORDERS["te7"]
    for k in (0, 1, r - 1, r - 2, (1 << 248) - 1, 0x1234567890abcdef << 190):
        for c in mpi.WIDTHS:
            d = mpi.recode(k, c, mpi.nwin(r.bit_length(), c))
            assert sum((-b if neg else b) << (c * w) for w, (b, neg) in enumerate(d)) == k
            assert all(b <= 1 << (c - 1) for b, _ in d)


@pytest.mark.parametrize("c", list(mpi.WIDTHS))
def test_mix_conditions(mix, c):
    r, terms, k0, k1 = mix
    bits = r.bit_length()
    nw, nb = mpi.nwin(bits, c), 1 << (c - 1)
    assert 2048 < len(terms) <= 8192                                       # the Pippenger chain, one sort tile
    assert sum(1 for b, _, _ in terms if b == -1) >= 100 and sum(1 for _, _, k in terms if k == 0) >= 100
    assert sum(1 for _, neg, _ in terms if neg) >= 150
    digits = [mpi.recode(k, c, nw) for _, _, k in terms]
    count = [dict() for _ in range(nw)]                                    # entries per bucket, per window
    signs = [set() for _ in range(nw)]
    for d in digits:
        for w, (b, neg) in enumerate(d):
            if b:
                count[w][b] = count[w].get(b, 0) + 1
                signs[w].add(neg)
    # a key in the top bucket b = nb
    assert any(nb in cw for cw in count)
    # keys of both signs in every window; the top window has positive keys only whatever the scalars (recode's assertion: nwin leaves
    # it at most c - 1 bits of the scalar), so there the condition is a key at all
    assert all(signs[w] == {False, True} for w in range(nw - 1)), [w for w in range(nw - 1) if signs[w] != {False, True}]
    assert signs[nw - 1] == {False}
    # a carry into the top window
    assert any(d[nw - 2][1] for d in digits)
    # k0 and k1 land in a bucket of every window
    assert all(b for b, _ in mpi.recode(k0, c, nw)) and all(b for b, _ in mpi.recode(k1, c, nw))
    # a heavy bucket at per = 64, so at every smaller share too -- in every window
    assert all(max(cw.values()) > mpi.HEAVY_PARTIALS * 64 for cw in count)
    # an ordinary multi-partial bucket at per = 8: more than one lane, no more than HEAVY_PARTIALS
    assert any(9 <= v <= 96 for cw in count for v in cw.values())
    # at per = 1, from the width on at which buckets get that small: the last bucket k_bucket_sum merges itself and the first it hands on
    if c >= 8:
        sizes = {v for cw in count for v in cw.values()}
        assert mpi.HEAVY_PARTIALS in sizes and mpi.HEAVY_PARTIALS + 1 in sizes


def empty_runs(buckets, nb):
    """lengths of the runs of empty buckets that have an occupied bucket on either side"""
    occ = sorted(buckets)
    return [b - a - 1 for a, b in zip(occ, occ[1:]) if b - a > 1]


def test_mix_empty_runs_at_13(mix):
    """a lane whose share crosses a run of empty buckets (k_accumulate's do .. while skip): at c = 13 a run of 16 or more inside a window,
    occupied buckets on either side of it"""
    r, terms, _, _ = mix
    nw = mpi.nwin(r.bit_length(), 13)
    occupied = [set() for _ in range(nw)]
    for _, _, k in terms:
        for w, (b, _) in enumerate(mpi.recode(k, 13, nw)):
            if b:
                occupied[w].add(b)
    longest = [max(empty_runs(o, 1 << 12), default=0) for o in occupied]
    assert max(longest[:nw - 1]) >= 16, longest


def test_other_sets():
    r = ORDERS["te0"]
    t3 = mpi.tiles3_terms(r, SEED)
    assert len(t3) == 16391 == 2 * 8192 + 7 and len({b for b, _, _ in t3}) == mpi.TILES3_BASES
    small = mpi.small_terms(r, SEED)
    assert sorted(small) == [1, 2, 5, 64, 300] and all(len(v) == n for n, v in small.items())
    assert all(0 <= k < r and -1 <= b < mpi.MIX_BASES for v in small.values() for b, _, k in v)
    bases, ks = mpi.collapse(["a", "b", "a"], [r - 1, 5, 3], r)
    assert dict(zip(bases, ks)) == {"a": 2, "b": 5}
