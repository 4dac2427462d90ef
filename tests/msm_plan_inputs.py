"""Inputs of the MSM plan sweep (tests/test_gpu_msm_plans.py), as abstract terms: no curve arithmetic happens here.

A term is (base, negated, scalar): `base` is an index into a list of distinct points the caller supplies (-1: the identity),
`negated` asks for the point's inverse.  The sweep turns the terms into the bytes of one chain (a twisted-Edwards suite, the native
short-Weierstrass suite, a pairing curve's G1); tests/test_msm_plan_inputs_host.py checks on the CPU, with a Python restatement of
k_digits' signed recoding (`recode`), that `mix` has what every plan (window width c = 4 .. 15, entries per lane 1 .. 4 096) needs
to be exercised -- see `mix_terms`."""
import random

HEAVY_PARTIALS = 12                      # csrc/msm.hip: a bucket fed by more lanes than this goes to k_heavy_sum
WIDTHS = range(4, 16)                    # the window widths msm_plan may choose
MIX_BASES, TILES3_BASES = 24, 257


def nwin(bits, c):
    """windows of a `bits`-bit scalar (msm_plan: one bit more than the scalar, for the carry of the signed recoding)"""
    return (bits + 1 + c - 1) // c


def recode(k, c, nw):
    """k_digits: [(bucket, negative)] per window; bucket 0 = no entry, digits in [-(2^(c-1) - 1), 2^(c-1)]"""
    nb, mask, carry, out = 1 << (c - 1), (1 << c) - 1, 0, []
    for w in range(nw):
        v = ((k >> (w * c)) & mask) + carry
        if v > nb:
            out.append(((1 << c) - v, True)); carry = 1
        else:
            out.append((v, False)); carry = 0
    assert carry == 0                    # the top window never goes negative: it holds at most c - 1 bits of the scalar
    return out


def digit_patterns(c):
    """two scalars of at most 249 bits (below every group order used: the smallest has 251): every digit of the first is 2^(c-1), the
    top bucket, unsigned; every digit of the second is 2^(c-1) + 1 (+ the carry): negative, with a carry into the next window"""
    nw = 248 // c
    top = sum((1 << (c - 1)) << (c * w) for w in range(nw))
    neg = sum(((1 << (c - 1)) + 1) << (c * w) for w in range(nw))
    assert top.bit_length() <= 249 and neg.bit_length() <= 249
    return top, neg


def full_scalar(rng, r):
    """a scalar below r without a zero digit in any window of any width: its term lands in a bucket of EVERY window"""
    bits = r.bit_length()
    k = rng.randrange(1, r)
    while True:                          # (one random scalar in a million has none: draw again only the bits around a zero digit)
        zero = [(c, w) for c in WIDTHS for w, (b, _) in enumerate(recode(k, c, nwin(bits, c))) if not b]
        if not zero:
            return k
        c, w = rng.choice(zero)
        lo = max(0, (w - 1) * c)         # the window and the one below it, whose sign is the carry
        k2 = (k & ~(((1 << 2 * c) - 1) << lo)) | (rng.getrandbits(2 * c) << lo)
        if 0 < k2 < r:
            k = k2


def mix_terms(r, seed):
    """About 3 200 shuffled terms over MIX_BASES points: above the single-launch size, inside one sort tile.  -> (terms, k0, k1)

      1 000 random scalars below r and 500 of random length up to 192 bits (so the windows above hold few enough entries that, even
            at c = 4, some bucket is fed by a handful of lanes only);
      800 copies of (base 0, k0) and 40 of (base 1, k1), k0 and k1 without a zero digit: a heavy bucket and an ordinary
            multi-partial bucket in every window, both made of P + P + P ...;
      12 and 13 copies of two more such pairs: buckets of exactly HEAVY_PARTIALS entries and of one more;
      150 pairs P, -P with one scalar: runs that pass through the identity;
      100 identity bases with random scalars, 100 zero scalars;
      1, 2, r - 1, r - 2, 2^248 - 1;
      for every c in 3 .. 15 the two digit patterns of `digit_patterns`."""
    rng = random.Random(seed)
    terms = []
    for i in range(1000):
        terms.append((i % MIX_BASES, False, rng.randrange(r)))
    for i in range(500):
        terms.append((i % MIX_BASES, False, rng.getrandbits(rng.randrange(1, 193))))
    k0, k1 = full_scalar(rng, r), full_scalar(rng, r)
    terms += [(0, False, k0)] * 800 + [(1, False, k1)] * 40
    # either side of the heavy threshold when every lane holds one entry: the most partials k_bucket_sum merges, the fewest k_heavy_sum does
    terms += [(2, False, full_scalar(rng, r))] * HEAVY_PARTIALS + [(3, False, full_scalar(rng, r))] * (HEAVY_PARTIALS + 1)
    for i in range(150):
        k = rng.randrange(r)
        terms += [(2 + i % 5, False, k), (2 + i % 5, True, k)]
    for i in range(100):
        terms += [(-1, False, rng.randrange(r)), (7, False, 0)]
    for i, k in enumerate([1, 2, r - 1, r - 2, (1 << 248) - 1]):
        terms.append((8 + i, False, k))
    for c in range(3, 16):
        top, neg = digit_patterns(c)
        terms += [(13 + c % 11, False, top), (13 + (c + 5) % 11, c % 2 == 1, neg)]
    rng.shuffle(terms)
    assert 2048 < len(terms) <= 8192
    return terms, k0, k1


def tiles3_terms(r, seed):
    """16 391 random terms over TILES3_BASES points: three sort tiles of 8 192 keys, the last one partial"""
    rng = random.Random(seed)
    return [(i % TILES3_BASES, False, rng.randrange(r)) for i in range(16391)]


def small_terms(r, seed):
    """{n: terms} for n = 1, 2, 5, 64, 300: MSMs that take the single launch unless AVRF_MSM_TINY=0 sends them down the general chain,
    where most lanes have empty shares and most windows of the short scalars no entries at all"""
    rng = random.Random(seed)
    out = {1: [(0, False, r - 1)], 2: [(0, False, rng.randrange(r)), (1, True, rng.getrandbits(64))],
           5: [(0, False, rng.randrange(r)), (-1, False, rng.randrange(r)), (1, False, 0), (0, True, 5), (2, False, rng.getrandbits(130))]}
    mix = mix_terms(r, seed)[0]
    out[64], out[300] = mix[:64], mix[1000:1300]
    return out


def collapse(bases, scalars, r):
    """the same sum with every distinct base once: its scalars added mod r in Python integers.  -> (bases, scalars)"""
    acc = {}
    for b, k in zip(bases, scalars):
        acc[b] = (acc.get(b, 0) + k) % r
    return list(acc), list(acc.values())
