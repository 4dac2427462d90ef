"""Operands, expected values and file packing for tools/fpu_probe.hip: the unsaturated-limb field and point layer (csrc/fpu.h, fpu_te.h,
fpu_g1.h, fpu_sqrt.h) on operands placed at the ENDS of the intervals the headers document, checked against Python integers.

The reference is arithmetic mod p and the affine group laws written out with pow(x, -1, p) below.  tools/fpu_model.py is imported for two
purposes only: to assert, case by case while generating, that an operand set satisfies the preconditions the headers state (its limb_check /
value-bound / to_packed assertions fire if a construction lands outside them), and for the limb-for-limb expectation of fu_mul / fu_sqr.

jobs() returns the list of Job objects in the order of the probe's main(): one per (type, operation), each with its cases (operand words +
what the checker needs) and a check(case, out_words) that returns None or (got, want) strings.  Every job has a multiple of 64 cases (whole
waves: g1u_madd / g1r_add vote with __any); wave k of a job is cases[64 k : 64 k + 64]."""
import functools
import os
import random
import struct
import sys

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import fpu_model as M  # noqa: E402

FIELDS = ["FqBandersnatch", "FqBabyJubJub", "FqEd25519", "FqBn254", "FqBls12381"]
G1_OF_FIELD = {"FqBn254": "G1Bn254", "FqBls12381": "G1Bls12381"}
SUITES = ["SuiteBandersnatch", "SuiteBabyJubJub", "SuiteJubJub", "SuiteEd25519"]          # a = -5, 1, -1, -1 (p = 2^255 - 19)
CURVES = ["G1Bls12381", "G1Bn254"]
SQRT_FIELDS = ["FqBandersnatch", "FqBabyJubJub", "FqEd25519"]
N_FIELD, N_MUL, N_POINT = 1024, 384, 128         # cases per field-level job (fu_mul / fu_sqr: the model's multiplier runs on each) / at least per point-level job
TE_INV, T4_INV, G1_INV = (15, 17, 24, 13), (16, 18, 25, 19), (46, 26, 15, 15)            # the inductive value bounds, in tenths of p
G1R_VB = 128                                     # |values| < 128 p in g1r_*
GARBAGE = 0xA5A5A5A5


def s32(w):
    return w - (1 << 32) if w >> 31 else w


def fmt(ws):
    return "[" + " ".join("%x" % (w & 0xffffffff) for w in ws) + "]"


class Case:
    def __init__(self, desc, words, ctx):
        self.desc, self.words, self.ctx = desc, words, ctx

    def __getattr__(self, k):
        try:
            return self.__dict__["ctx"][k]
        except KeyError:
            raise AttributeError(k)


class Job:
    def __init__(self, name, in_w, out_w, check):
        self.name, self.in_w, self.out_w, self.check, self.cases = name, in_w, out_w, check, []

    def add(self, desc, words, **ctx):
        assert len(words) == self.in_w and all(-(1 << 31) <= w < (1 << 32) for w in words), (self.name, desc)
        self.cases.append(Case(desc, [w & 0xffffffff for w in words], ctx))

    def fill(self, rand, n):
        while len(self.cases) < n or len(self.cases) % 64:
            rand()
        return self


class Fld:
    """layout of a field in unsaturated limbs (fpu.h UL<F>) and the conversions between integers, limbs and saturated words"""

    def __init__(self, name, C):
        self.name, self.m = name, M.Field(name, C[name])
        self.p, self.N = self.m.p, self.m.N
        self.W, self.L = (29, 9) if self.N == 8 else (28, 14)
        self.SH = self.W * self.L - 32 * self.N
        self.MASK = (1 << self.W) - 1
        self.R, self.Ru = 1 << (32 * self.N), 1 << (self.W * self.L)
        self.top = self.W * (self.L - 1)

    def sl(self, v):
        """limbs 0 .. L-2 in [0, 2^W), the top limb signed and taking the rest: the form a product leaves"""
        return [(v >> (self.W * i)) & self.MASK for i in range(self.L - 1)] + [v >> self.top]

    def val(self, limbs):
        return sum(l << (self.W * i) for i, l in enumerate(limbs))

    def words(self, v):
        assert 0 <= v < self.R
        return [(v >> (32 * i)) & 0xffffffff for i in range(self.N)]

    def unwords(self, ws):
        return sum(w << (32 * i) for i, w in enumerate(ws))

    def signed(self, ws):
        return [s32(w) for w in ws]

    def unique(self, limbs):
        return all(0 <= l <= self.MASK for l in limbs[:-1])

    def prod_form(self, rng, top=1 << 20):
        """what a previous product leaves: limbs 0 .. L-2 in [0, 2^W), a small signed top limb"""
        return [rng.choice([0, self.MASK, rng.randrange(self.MASK + 1), rng.randrange(self.MASK + 1)]) for _ in range(self.L - 1)] + [rng.randrange(-top, top + 1)]

    def neg_form(self, limbs, rng):
        """the same value with 2^W moved between neighbouring limbs at random places: limbs in [-2^W, 2^W]"""
        r = list(limbs)
        for i in range(self.L - 1):
            if rng.getrandbits(1):
                r[i] -= 1 << self.W; r[i + 1] += 1
        assert self.val(r) == self.val(limbs)
        return r


def rep(c, tenths, side, p):
    """the representative c + k p of largest magnitude with |value| < tenths / 10 * p, on the positive (side 0) or negative side of zero"""
    if side == 0:
        v = c + (tenths * p - 1 - 10 * c) // (10 * p) * p
    else:
        v = c - (tenths * p - 1 + 10 * c) // (10 * p) * p
    assert v % p == c % p and 10 * abs(v) < tenths * p and 10 * abs(v + (p if side == 0 else -p)) >= tenths * p
    return v


def sqrt_mod(n, p):
    """Tonelli-Shanks; None for a non-residue"""
    n %= p
    if n == 0:
        return 0
    if pow(n, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2; s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(n, q, p), pow(n, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % p; i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


# ------------------------------------------------------------------------------------------------------------------ field level

def job_slice(f, S, rng):
    def check(c, out):
        want = f.sl(c.v << S)
        return None if out == want else (fmt(out), fmt(want))
    j = Job(f"{f.name}/fu_slice<{S}>", f.N, f.L, check)
    vals = [0, 1, f.p - 1, f.p, f.p + 1, f.R - 1, f.R % f.p] + [1 << k for k in range(32 * f.N)] + [(1 << k) - 1 for k in range(2, 32 * f.N, 7)]
    for v in vals:
        j.add(f"v = {v:#x}", f.words(v), v=v)

    def rand():
        v = rng.randrange(f.R); j.add(f"random v = {v:#x}", f.words(v), v=v)
    return j.fill(rand, N_FIELD)


def job_cneg(f, rng):
    L, ext = f.L, (1 << 31) - 1

    def check(c, out):
        want = [-l if c.s else l for l in c.a]
        return None if f.signed(out) == want else (fmt(out), fmt(want))
    j = Job(f"{f.name}/fu_cneg", L + 1, L, check)

    def add(desc, a, s):
        j.add(f"{desc}, mask {s}", a + [s], a=a, s=s)
    for s in (0, -1):
        for name, a in (("2^31 - 1", [ext] * L), ("-(2^31 - 1)", [-ext] * L), ("0", [0] * L), ("1", [1] * L), ("-1", [-1] * L),
                        ("alternating +-(2^31 - 1)", [ext if i & 1 else -ext for i in range(L)]), ("2^W", [1 << f.W] * L), ("-2^30", [-(1 << 30)] * L)):
            add("limbs " + name, a, s)
    add("limbs -2^31", [-(1 << 31)] * L, 0)                  # the mask 0 passes every int32 through
    return j.fill(lambda: add("random", [rng.choice([ext, -ext, rng.randrange(-ext, ext + 1), rng.randrange(-ext, ext + 1)]) for _ in range(L)], rng.choice((0, -1))), N_FIELD)


def job_carry(f, rng):
    L, W = f.L, f.W
    span = 1 << (31 - W)                                     # a limb of magnitude < 2^31 carries at most this much

    def check(c, out):
        r = f.signed(out)
        ok = f.val(r) == f.val(c.a) and 0 <= r[0] <= f.MASK and all(-span <= l < (1 << W) + span for l in r[1:-1])
        if all(0 <= l < (4 << W) for l in c.a[:-1]):          # the header's range: limbs in [0, 2^W + 4)
            ok = ok and all(0 <= l < (1 << W) + 4 for l in r[:-1])
        return None if ok else (fmt(out) + f" value {f.val(r):#x}", f"value {f.val(c.a):#x}, limbs in range")
    j = Job(f"{f.name}/fu_carry", L, L, check)
    ext = (1 << 31) - 1
    consts = [ext, -ext, 1 << W, (1 << W) - 1, -1, -(1 << W), -(1 << W) - 1, -(1 << 30) - 5, (1 << W) + 3, 1, 1 - (1 << W), (4 << W) - 1, -(3 << (W - 1))]
    tops = [1 << 30, -(1 << 30), 0, 12345, -1]
    for k, c in enumerate(consts):
        j.add(f"limbs 0..L-2 = {c:#x}", [c] * (L - 1) + [tops[k % len(tops)]], a=[c] * (L - 1) + [tops[k % len(tops)]])
        for i in range(L - 1):
            a = [0] * L; a[i] = c; a[L - 1] = tops[(k + i) % len(tops)]
            j.add(f"limb {i} = {c:#x}, others 0", a, a=a)

    def rand():
        a = [rng.choice(consts + [rng.randrange(-ext, ext + 1)] * 6) for _ in range(L - 1)] + [rng.randrange(-(1 << 30), (1 << 30) + 1)]
        j.add("random", a, a=a)
    return j.fill(rand, N_FIELD)


def job_carry_u(f, rng):
    """B + 5 A as teu_madd forms it (unsigned limbs 0 .. L-2, signed top)"""
    L, W = f.L, f.W

    def check(c, out):
        r = f.signed(out)
        cmax = max(b + 5 * a for a, b in zip(c.A[:-1], c.B[:-1])) >> W          # the largest carry the sums can hand on
        want = f.val(c.B) + 5 * f.val(c.A)
        ok = f.val(r) == want and 0 <= r[0] <= f.MASK and all(0 <= l <= f.MASK + cmax for l in r[1:-1])
        return None if ok else (fmt(out) + f" value {f.val(r):#x}", f"value {want:#x}, limbs in [0, 2^W + {cmax}]")
    j = Job(f"{f.name}/fu_carry_u(B + 5 A)", 2 * L, L, check)

    def add(desc, A, B):
        assert all(0 <= b + 5 * a < (1 << 32) for a, b in zip(A[:-1], B[:-1])) and -(1 << 31) <= B[-1] + 5 * A[-1] < (1 << 31)
        j.add(desc, A + B, A=A, B=B)
    M_ = f.MASK
    add("A limbs 2^W + 3, B limbs 2^W - 1 (the sum needs bit 31)", [M_ + 4] * (L - 1) + [3], [M_] * (L - 1) + [-7])
    add("A, B limbs 2^W - 1 (two products' outputs at their largest)", [M_] * (L - 1) + [-(1 << 24)], [M_] * (L - 1) + [1 << 24])
    add("alternating: a carry of 5 into low bits all ones", [M_ if i % 2 == 0 else 0 for i in range(L - 1)] + [1], [M_] * (L - 1) + [0])
    add("zero", [0] * L, [0] * L)
    add("A = 0", [0] * L, [M_] * (L - 1) + [-1])
    add("B = 0", [M_] * (L - 1) + [-1], [0] * L)

    def rand():
        add("random products' outputs", f.prod_form(rng, 1 << 24), f.prod_form(rng, 1 << 24))
    return j.fill(rand, N_FIELD)


def job_times5(f, rng):
    L, W = f.L, f.W

    def check(c, out):
        r = f.signed(out)
        ok = f.val(r) == 5 * f.val(c.a) and 0 <= r[0] <= f.MASK and all(0 <= l <= f.MASK + 5 for l in r[1:-1])
        return None if ok else (fmt(out) + f" value {f.val(r):#x}", f"value {5 * f.val(c.a):#x}, limbs in [0, 2^W + 4]")
    j = Job(f"{f.name}/fu_times5", L, L, check)

    def add(desc, a):
        assert all(0 <= l < (1 << W) + 4 for l in a[:-1]) and abs(a[-1]) < 1 << 28
        j.add(desc, a, a=a)
    ones5 = (f.MASK * pow(5, -1, 1 << W)) & f.MASK                              # 5 * ones5 = all ones in the low W bits
    add("limbs 2^W + 3", [f.MASK + 4] * (L - 1) + [(1 << 28) - 1])
    add("limbs 2^W - 1", [f.MASK] * (L - 1) + [-(1 << 28) + 1])
    add("limbs 0", [0] * L)
    add("alternating 2^W + 3 / low bits all ones after the multiplication", [f.MASK + 4 if i % 2 == 0 else ones5 for i in range(L - 1)] + [5])
    return j.fill(lambda: add("random", [rng.choice([f.MASK + 4, f.MASK + 1, ones5, rng.randrange((1 << W) + 4), rng.randrange((1 << W) + 4)]) for _ in range(L - 1)]
                              + [rng.randrange(-(1 << 28) + 1, 1 << 28)]), N_FIELD)


def mul_operands(f, rng, sqr):
    """[(description, a, b)]: the operand classes of fu_mul (|a_i| <= 2^30, |b_j| <= 2^29 + 4) or fu_sqr (|a_i| <= 2^29 + 2^4; b is a); top limbs 2^28"""
    L, W, p = f.L, f.W, f.p
    A, B, T = ((1 << 29) + 16, (1 << 29) + 16, 1 << 28) if sqr else (1 << 30, (1 << 29) + 4, 1 << 28)
    out = []
    for r in range(8):                                                         # every limb at its extreme, all sign patterns
        sa, sb, st = (1 if r & 1 else -1), (1 if r & 2 else -1), (1 if r & 4 else -1)
        out.append((f"all limbs extreme, signs {sa:+d} {sb:+d}, tops {st:+d}", [sa * A] * (L - 1) + [st * T], [sb * B] * (L - 1) + [st * T]))
    for i in range(L):
        for sa in (1, -1):
            for sb in (1, -1):
                a = [0] * L; a[i] = sa * (T if i == L - 1 else A)
                out.append((f"a = limb {i} at {sa:+d} extreme, b all limbs {sb:+d} extreme", a, [sb * B] * (L - 1) + [sb * T]))
    sp = [("p", p), ("2p", 2 * p), ("p - 1", p - 1), ("0", 0), ("1", 1), ("R mod p", f.R % p)]
    for na, va in sp:
        for nb, vb in sp:
            out.append((f"limbs of {na} x limbs of {nb}", f.sl(va), f.sl(vb)))
    for _ in range(48):
        out.append(("two previous products' outputs", f.prod_form(rng), f.prod_form(rng)))
    for k in range(48):                                                        # how E, F, G reach a product
        r1, r2, r3, r4 = (f.prod_form(rng) for _ in range(4))
        a = [x - y for x, y in zip(r1, r2)] if (sqr or k & 1) else [x + y for x, y in zip(r1, r2)]
        out.append(("sum / difference of two products' outputs x difference of two", a, [x - y for x, y in zip(r3, r4)]))
    return out, (A, B, T)


def job_mul(f, rng, sqr):
    L, W, p = f.L, f.W, f.p

    def check(c, out):
        r = f.signed(out)
        va, vb, vr = f.val(c.a), f.val(c.b), f.val(r)
        ok = (vr * f.Ru - va * vb) % p == 0 and f.unique(r) and abs(vr) < abs(va * vb) // f.Ru + p + 1 and r == c.want
        return None if ok else (fmt(out), fmt(c.want))
    j = Job(f"{f.name}/{'fu_sqr' if sqr else 'fu_mul'}", L if sqr else 2 * L, L, check)
    ops, (A, B, T) = mul_operands(f, rng, sqr)

    def add(desc, a, b):
        if sqr:
            b = a
        assert all(abs(x) <= A for x in a[:-1]) and all(abs(x) <= B for x in b[:-1]) and abs(a[-1]) <= T and abs(b[-1]) <= T, (j.name, desc)
        want = f.m.mul(a, b, sqr=sqr)                                          # asserts that every column stays inside the signed 64-bit range
        j.add(desc, a if sqr else a + b, a=a, b=b, want=want)
    for desc, a, b in ops:
        add(desc, a, b)
    return j.fill(lambda: add("random limbs inside the bounds", M.rand_limbs(f.m, rng, A, T), M.rand_limbs(f.m, rng, B, T)), N_MUL)


def packed_reps(f, v):
    """limb vectors of the value v: the slice (signed top), and 2^W moved between neighbouring limbs either way, at one place or at all of them"""
    base, out = f.sl(v), []
    out.append(("slice", base))
    for i in (0, f.L // 2, f.L - 2):
        for d in (1, -1):
            r = list(base); r[i] += d << f.W; r[i + 1] -= d
            out.append((f"2^W moved {'into' if d > 0 else 'out of'} limb {i}", r))
    r = list(base)
    for i in range(f.L - 1):
        r[i] -= 1 << f.W; r[i + 1] += 1
    out.append(("every low limb negative", r))
    return out


def job_packed(f, KB, rng):
    p, K = f.p, 1 << KB

    def check(c, out):
        want = f.words(c.v % p)
        return None if out == want else (fmt(out), fmt(want))
    j = Job(f"{f.name}/fu_to_packed<{KB}>", f.L, f.N, check)

    def add(desc, v, limbs):
        assert f.val(limbs) == v and f.m.to_packed(limbs, KB) == v % p         # the model asserts |value| < 2^KB p and the int32 ranges
        j.add(desc, limbs, v=v)
    vals = [("0", 0), ("1", 1), ("-1", -1), ("p - 1", p - 1), ("-(p - 1)", 1 - p), ("p + 1", p + 1), ("-(p + 1)", -p - 1), (f"{K} p - 1", K * p - 1), (f"-({K} p - 1)", 1 - K * p)]
    vals += [(f"{k} p", k * p) for k in range(-K + 1, K)]
    for name, v in vals:
        for rn, limbs in packed_reps(f, v):
            add(f"value {name}, {rn}", v, limbs)

    def rand():
        v = rng.randrange(1 - K * p, K * p)
        rn, limbs = rng.choice(packed_reps(f, v))
        add(f"random value {v:#x}, {rn}", v, limbs)
    return j.fill(rand, N_FIELD)


def job_zero(f, rng):
    """flags: fu_is_zero_mod_p, fu_maybe_zero_mod_p, fu_is_zero_mod_p2, fu_maybe_zero_mod_p2.  The exact tests answer for a Montgomery product's
    output: unique representation, value in (-p, 2p) (a square's: (-p, 3p) for the _p2 form)"""
    L, W, p = f.L, f.W, f.p

    def check(c, out):
        v = f.val(c.a)
        want = list(out)
        if -p < v < 2 * p:
            want[0] = int(v % p == 0)
        if -p < v < 3 * p:
            want[2] = int(v % p == 0)
        if out[0] == 1: want[1] = 1
        if out[2] == 1: want[3] = 1
        ok = out == want and all(w in (0, 1) for w in out)
        return None if ok else (fmt(out), fmt(want))
    j = Job(f"{f.name}/zero tests", L, 4, check)

    def add(desc, a):
        v = f.val(a)
        assert not (-p < v < 3 * p and v % p == 0) or f.unique(a), (j.name, desc)
        j.add(desc, a, a=a)
    for name, v in (("all zero", 0), ("p's", p), ("2p's", 2 * p)):
        add("limbs " + name, f.sl(v))
        for i in range(L):
            for d in (1, -1):
                a = f.sl(v); a[i] += d
                add(f"limbs {name}, limb {i} {d:+d}", a)
        for _ in range(8):
            a = f.prod_form(rng, 1 << 10); a[0] = f.sl(v)[0]; a[1] |= 1
            add(f"limb 0 alone equals {name}", a)
    for k in range(-6, 7):                                                     # P = U2 - X a multiple of p: what the accumulator bounds allow
        P = f.sl(k * p)
        add(f"fu_sqr of the slice of {k} p", f.m.mul(P, P, sqr=True))
        for _ in range(3):
            c = rng.randrange(p)
            P = [x - y for x, y in zip(f.sl(k * p + c), f.sl(c))]
            assert f.val(P) == k * p
            add(f"fu_sqr of {k} p as a difference of two slices", f.m.mul(P, P, sqr=True))
    return j.fill(lambda: add("random product output", f.prod_form(rng, 1 << 10)), N_FIELD)


def field_jobs(f, rng):
    return [job_slice(f, 0, rng), job_slice(f, f.SH, rng), job_cneg(f, rng), job_carry(f, rng), job_carry_u(f, rng), job_times5(f, rng),
            job_mul(f, rng, False), job_mul(f, rng, True), job_packed(f, 2, rng), job_zero(f, rng)]


# ------------------------------------------------------------------------------------------------------------------ twisted Edwards

class Chain(M.TEChain):
    """teu4_madd_pre from the model's own assertion primitives (its lim / hsum / check_out and the multiplier's column checks)"""

    def madd_pre(self, P, q):
        f = self.f
        X, Y, T, Z = P
        n29, n30 = (1 << f.W) + 4, 1 << (f.W + 1)
        sl = lambda v: f.slice(v, f.SH)
        A, B, C = f.mul(X, sl(q[0])), f.mul(Y, sl(q[1])), f.mul(T, sl(q[2]))
        XY = [M.i32(a + b) for a, b in zip(X, Y)]
        self.lim(XY, n30, sl(q[0] + q[1]), n29)
        E = f.mul(XY, sl(q[0] + q[1]))
        E = [M.i32(e - a - b) for e, a, b in zip(E, A, B)]
        F = [M.i32(z - c) for z, c in zip(Z, C)]; G = [M.i32(z + c) for z, c in zip(Z, C)]
        H = self.hsum(A, B)
        self.lim(E, n30, F, n29); self.lim(G, n30, H, n29)
        return self.check_out((f.mul(E, F), f.mul(G, H), f.mul(E, H), f.mul(F, G)))


class TEc:
    def __init__(self, name, C, f, rng):
        d = C[name]
        self.name, self.f, self.m = name, f, M.TE(name, d, f.m)
        p, Ri = f.p, pow(f.R, -1, f.p)
        self.a = {0: 1, 1: p - 5, 2: p - 1}[d["A_KIND"]]
        self.d = d["D"] * Ri % p
        self.G = (d["G_X"] * Ri % p, d["G_Y"] * Ri % p)
        assert self.on_curve(self.G)
        G = self.G
        named = [("G", G), ("2 G", self.mulk(2, G)), ("3 G", self.mulk(3, G)), ("7 G", self.mulk(7, G)), ("identity", (0, 1)), ("(0, -1)", (0, p - 1))]
        x4 = sqrt_mod(pow(self.a, -1, p), p)                                    # (+-1/sqrt(a), 0): order 4, where a is a square
        if x4 is not None:
            named += [(f"({x4:#x}, 0)" if x4 != 1 else "(1, 0)", (x4, 0)), ("(-1/sqrt(a), 0)" if x4 != 1 else "(p - 1, 0)", (p - x4, 0))]
        mont = lambda v: v * f.R % p
        k = 11
        while not any(n.startswith("x R + y R >= p") for n, _ in named) or not any(n.startswith("x R + y R < p") for n, _ in named):
            P = self.mulk(k, G)
            tag = "x R + y R >= p" if mont(P[0]) + mont(P[1]) >= p else "x R + y R < p"
            if not any(n.startswith(tag) for n, _ in named):
                named.append((f"{tag}: {k} G", P))
            k += 1
        assert all(self.on_curve(P) for _, P in named)
        self.bases = named
        self.pool = [self.mulk(rng.getrandbits(64) | 1, G) for _ in range(24)]

    def on_curve(self, P):
        x, y = P
        return (self.a * x * x + y * y - 1 - self.d * x * x * y * y) % self.f.p == 0

    def add(self, P, Q):
        p = self.f.p
        (x1, y1), (x2, y2) = P, Q
        k = self.d * x1 * x2 % p * y1 * y2 % p
        return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, p) % p, (y1 * y2 - self.a * x1 * x2) * pow(1 - k, -1, p) % p)

    def neg(self, P):
        return (-P[0] % self.f.p, P[1])

    def mulk(self, k, P):
        r = (0, 1)
        for bit in bin(k)[2:]:
            r = self.add(r, r)
            if bit == "1":
                r = self.add(r, P)
        return r

    def pre(self, P):
        f = self.f
        return (P[0] * f.R % f.p, P[1] * f.R % f.p, self.d * P[0] * P[1] % f.p * f.R % f.p)

    def pre_words(self, P):
        return sum((self.f.words(v) for v in self.pre(P)), [])

    def ext(self, P, mu):
        """an extended point in saturated canonical Montgomery words with the projective scale mu"""
        f = self.f
        return tuple(v * mu % f.p * f.R % f.p for v in (P[0], P[1], P[0] * P[1], 1))

    def acc(self, A, s, sides, form, inv, rng, carried):
        """limbs (X, Y, T, Z) of an accumulator holding A as the point (s X, Y, s T, Z) (s = 0 / -1), each coordinate at the end of its interval on the
        side sides[j] of zero.  form 0: slices as a product leaves them; 1: 2^W moved between limbs of X, Y, T (limbs in [-2^W, 2^W]); 2: Z, the free
        projective scale, chosen limb by limb from the ends of a product's range [0, 2^W) -- of the carried range [0, 2^W + 4] where the operation takes
        carried operands (`carried`) -- and its top limb placed at the bound"""
        f, p = self.f, self.f.p
        if form == 2:
            low = [rng.choice(([f.MASK + 4, f.MASK + 5, f.MASK + 1] if carried else [f.MASK, f.MASK - 1, 1]) + [f.MASK, 0, rng.randrange(f.MASK + 1)]) for _ in range(f.L - 1)]
            lv, lim = f.val(low), (inv[3] * p + 9) // 10
            top = (lim - 1 - lv) >> f.top if sides[3] == 0 else -((lim - 1 + lv) >> f.top)
            Z = low + [top]
            assert 10 * abs(f.val(Z)) < inv[3] * p
            lam = f.val(Z) % p
        else:
            lam = rng.randrange(1, p)
            Z = f.sl(rep(lam, inv[3], sides[3], p))
        sg = -1 if s else 1
        res = [sg * lam * A[0] % p, lam * A[1] % p, sg * lam * A[0] * A[1] % p]
        XYT = [f.sl(rep(c, b, side, p)) for c, b, side in zip(res, inv, sides)]
        if form == 1:
            XYT = [f.neg_form(v, rng) for v in XYT]
        return XYT + [Z]

    def acc_stream(self, rng, inv, n_struct, carried):
        """(description, point, s, limbs): every side pattern on a rotating set of points, forms and signs, then random ones for ever"""
        specials = [("identity", (0, 1)), ("(0, -1)", (0, self.f.p - 1)), ("G", self.G), ("-G", self.neg(self.G))]
        k = 0
        while True:
            pat = k % 16 if k < n_struct else rng.getrandbits(4)
            name, A = specials[(k // 16) % 4] if (k < n_struct and k % 3 == 0) else ("random point", rng.choice(self.pool))
            s, form = -(k >> 1 & 1) if k < n_struct else -rng.getrandbits(1), (k + (k >> 4)) % 3
            sides = [(pat >> j) & 1 for j in range(4)]
            yield f"acc = {name}, sides {pat:04b}, form {form}, neg {s}", A, s, self.acc(A, s, sides, form, inv, rng, carried)
            k += 1

    def point_check(self, inv, signed, c, limbs4, negw=None):
        """None, or why the limbs are not the point c.want: affine value, T Z = X Y, the inductive bounds, products' limb ranges"""
        f, p = self.f, self.f.p
        X, Y, T, Z = (f.val(v) for v in limbs4)
        if signed and negw != (0xffffffff if c.neg else 0):
            return f"neg {negw:#x}"
        if not all(f.unique(v) for v in limbs4):
            return "limbs 0..L-2 outside [0, 2^W)"
        if not all(10 * abs(v) < b * p for v, b in zip((X, Y, T, Z), inv)):
            return "outside the inductive bound: |X|, |Y|, |T|, |Z| / p = " + ", ".join(f"{abs(v) / p:.3f}" for v in (X, Y, T, Z))
        if (T * Z - X * Y) % p or Z % p == 0:
            return "T Z != X Y"
        zi = pow(Z, -1, p)
        got = ((-X if (signed and c.neg) else X) * zi % p, Y * zi % p)
        return None if got == c.want else f"affine ({got[0]:#x}, {got[1]:#x})"


def te_jobs(te, rng):
    f, p, L = te.f, te.f.p, te.f.L
    name = te.name
    want_str = lambda c: f"affine ({c.want[0]:#x}, {c.want[1]:#x})"
    flat = lambda limbs4: sum(limbs4, [])
    split = lambda ws: [f.signed(ws[9 * k: 9 * k + 9]) for k in range(4)]
    chain = Chain(te.m)
    jobs = []

    # teu_from_pre
    def chk_from_pre(c, out):
        x, y, t, z = split(out)
        Q = c.Q
        ok = x == f.sl(Q[0] * f.R % p) and y == f.sl(Q[1] * f.R % p) and z == f.sl(f.R % p) and out[36] == (0xffffffff if c.neg else 0)
        ok = ok and f.val(t) % p == Q[0] * Q[1] * f.R % p and f.unique(t) and abs(f.val(t)) < p * p * (1 << f.SH) // f.Ru + p + 1
        return None if ok else (fmt(out), f"slices of x R, y R, t = x y R, z = R, neg {c.neg}")
    j = Job(f"{name}/teu_from_pre", 25, 37, chk_from_pre)

    def add_from_pre(bn, Q, neg):
        r = te.m.from_pre(te.pre(Q), bool(neg))
        assert te.m.to_affine(r) == (te.neg(Q) if neg else Q)
        j.add(f"base {bn}, neg {neg}", te.pre_words(Q) + [neg], Q=Q, neg=neg)
    for bn, Q in te.bases:
        for neg in (0, 1):
            add_from_pre(bn, Q, neg)
    jobs.append(j.fill(lambda: add_from_pre("random", rng.choice(te.pool), rng.getrandbits(1)), N_POINT))

    # teu_madd
    def chk_madd(c, out):
        why = te.point_check(TE_INV, True, c, split(out), out[36])
        return None if why is None else (fmt(out) + " " + why, want_str(c))
    j = Job(f"{name}/teu_madd", 62, 37, chk_madd)
    accs = te.acc_stream(rng, TE_INV, 16 * len(te.bases), False)

    def add_madd(bn, Q, neg):
        desc, A, s, limbs = next(accs)
        if "random point" in desc and rng.randrange(8) == 0:                   # the accumulator holds the base itself, or its negative
            A = Q if rng.getrandbits(1) else te.neg(Q); desc = desc.replace("random point", "+-base")
            limbs = te.acc(A, s, [rng.getrandbits(1) for _ in range(4)], rng.randrange(3), TE_INV, rng, False)
        want = te.add(A, te.neg(Q) if neg else Q)
        r = te.m.madd(tuple(limbs) + (s,), te.pre(Q), bool(neg))               # the model's limb and value assertions: the case is inside the contract
        j.add(f"{desc}; base {bn}, neg {neg}", flat(limbs) + [s] + te.pre_words(Q) + [neg], want=want, neg=neg, model=te.m.to_affine(r))
    for bi, (bn, Q) in enumerate(te.bases):
        for pat in range(16):
            add_madd(bn, Q, (pat + bi) & 1)                                    # with acc_stream's neg = bit 1 of its counter: all four combinations per base
    jobs.append(j.fill(lambda: add_madd(*rng.choice(te.bases + [("random", P) for P in te.pool]), rng.getrandbits(1)), N_POINT))

    # teu_to_ext, and the partial-sum round trip
    def ext_words(c):
        sg = -1 if c.s else 1
        X, Y, T, Z = (f.val(v) for v in c.limbs)
        return sum((f.words(v % p) for v in (sg * X, Y, sg * T, Z)), [])

    def chk_to_ext(c, out):
        return None if out == ext_words(c) else (fmt(out), fmt(ext_words(c)))

    def chk_part(c, out):
        sg = -1 if c.s else 1
        raw = [[sg * l for l in v] if k % 2 == 0 else list(v) for k, v in enumerate(c.limbs)]
        want = [w & 0xffffffff for w in flat(c.limbs) + [c.s, 0, 0, 0]] + ext_words(c) + ext_words(c) + [w & 0xffffffff for w in flat(raw)]
        return None if out == want else (fmt(out), fmt(want))
    j1, j2 = Job(f"{name}/teu_to_ext", 37, 32, chk_to_ext), Job(f"{name}/teu_store_part -> teu_load_part / _coord / _coord_raw", 37, 140, chk_part)
    for j in (j1, j2):
        accs2 = te.acc_stream(rng, TE_INV, 64, True)

        def add_acc(j=j, accs2=accs2):
            desc, A, s, limbs = next(accs2)
            sg = -1 if s else 1
            for k, v in enumerate(limbs):
                f.m.to_packed([sg * l for l in v] if k % 2 == 0 else v)       # asserts the precondition of fu_to_packed
            j.add(desc, flat(limbs) + [s], limbs=limbs, s=s)
        jobs.append(j.fill(add_acc, N_POINT))

    # teu4_from_ext
    def chk_t4_from_ext(c, out):
        want = flat([f.sl(v) for v in c.e])
        return None if f.signed(out) == want else (fmt(out), fmt(want))
    j = Job(f"{name}/teu4_from_ext", 32, 36, chk_t4_from_ext)

    def add_fe(desc, e):
        j.add(desc, sum((f.words(v) for v in e), []), e=e)
    for v in (0, 1, p - 1, f.R % p):
        add_fe(f"coordinates {v:#x}", (v,) * 4)
    for bn, Q in te.bases:
        add_fe(f"{bn}, Z = 1", te.ext(Q, 1))
    jobs.append(j.fill(lambda: add_fe("random point, random scale", te.ext(rng.choice(te.pool), rng.randrange(1, p))), N_POINT))

    # teu4_dbl / teu4_add_sat / teu4_madd_pre
    def chk_t4(c, out):
        why = te.point_check(T4_INV, False, c, split(out))
        return None if why is None else (fmt(out) + " " + why, want_str(c))
    for op in ("teu4_dbl", "teu4_add_sat", "teu4_madd_pre"):
        j = Job(f"{name}/{op}", {"teu4_dbl": 36, "teu4_add_sat": 68, "teu4_madd_pre": 60}[op], 36, chk_t4)
        accs4 = te.acc_stream(rng, T4_INV, 64, op != "teu4_madd_pre")

        def add_t4(bn=None, Q=None, j=j, op=op, accs4=accs4):
            desc, A, s, limbs = next(accs4)
            if s:
                A = te.neg(A)                                                  # no sign word here: the limbs are the point (X, Y, T, Z) itself
            if Q is None:
                bn, Q = rng.choice(te.bases + [("random", P) for P in te.pool])
            if op == "teu4_dbl":
                r = chain.dbl(tuple(limbs)); want = te.add(A, A); words = flat(limbs)
            elif op == "teu4_add_sat":
                e = te.ext(Q, rng.choice([1, p - 1, rng.randrange(1, p)]))
                r = chain.add_sat(tuple(limbs), e); want = te.add(A, Q); words = flat(limbs) + sum((f.words(v) for v in e), [])
                desc += f"; entry {bn}"
            else:
                r = chain.madd_pre(tuple(limbs), te.pre(Q)); want = te.add(A, Q); words = flat(limbs) + te.pre_words(Q)
                desc += f"; base {bn}"
            j.add(desc, words, want=want, neg=0, model=chain.to_affine(r))
        if op != "teu4_dbl":
            for bn, Q in te.bases:
                for _ in range(4):
                    add_t4(bn, Q)
        jobs.append(j.fill(add_t4, N_POINT))

    # teu4_to_ext
    def chk_t4_to_ext(c, out):
        want = sum((f.words(f.val(v) % p) for v in c.limbs), [])
        return None if out == want else (fmt(out), fmt(want))
    j = Job(f"{name}/teu4_to_ext", 36, 32, chk_t4_to_ext)
    accs5 = te.acc_stream(rng, T4_INV, 64, True)

    def add_t4e():
        desc, A, s, limbs = next(accs5)
        for v in limbs:
            f.m.to_packed(v)
        j.add(desc, flat(limbs), limbs=limbs)
    jobs.append(j.fill(add_t4e, N_POINT))
    # the order of the probe: from_pre, madd, to_ext, part, teu4_from_ext, dbl, add_sat, madd_pre, teu4_to_ext
    return jobs


# ------------------------------------------------------------------------------------------------------------------ G1, XYZZ

class G1c:
    def __init__(self, name, C, f, rng):
        self.name, self.f, self.m = name, f, M.G1(name, C[name], f.m)
        self.red = M.G1Red(self.m)
        p = f.p
        self.b = C[name]["B"] * pow(f.R, -1, p) % p
        self.a, self.bb, self.g, self.d = (4 if f.SH == 8 else 3), 2, 4, 6       # fpu_g1.h G1U<C>: 3a - 2b = SH, g = 2m, d = 3m, m = 2
        self.sx, self.sy, self.kx, self.ky = self.a + f.SH - self.g, self.bb + f.SH - self.d, self.g - self.a, self.d - self.bb
        assert 3 * self.a - 2 * self.bb == f.SH and p % 4 == 3
        self.pool = [self.rand_point(rng) for _ in range(24)]
        x = 1                                                                   # the curve point of smallest x >= 1 (BN254: the generator (1, 2)) and small multiples
        while pow(x ** 3 + self.b, (p - 1) // 2, p) != 1:
            x += 1
        y = pow(x ** 3 + self.b, (p + 1) // 4, p)
        G0 = (x, min(y, p - y))
        self.named = [(f"G0 = ({x}, {G0[1]:#x})", G0)] + [(f"{k} G0", self.mulk(k, G0)) for k in (2, 3, 7)]
        y0 = sqrt_mod(self.b, p)
        if y0 is not None:
            self.named.append(("(0, sqrt b): x = 0, order 3", (0, y0)))
        assert all((P[1] ** 2 - P[0] ** 3 - self.b) % p == 0 for _, P in self.named)
        self.inv_x = 10 * (1 << self.a) if self.kx == 0 else G1_INV[0]          # g1u_load_part: X of an affine point stored as it entered, < 2^a p

    def rand_point(self, rng):
        p = self.f.p
        while True:
            x = rng.randrange(p); r = (x * x * x + self.b) % p
            y = pow(r, (p + 1) // 4, p)
            if y * y % p == r and y:
                return (x, y if rng.getrandbits(1) else p - y)

    def add(self, P, Q):
        p = self.f.p
        if P is None: return Q
        if Q is None: return P
        (x1, y1), (x2, y2) = P, Q
        if x1 == x2:
            if (y1 + y2) % p == 0: return None
            l = 3 * x1 * x1 * pow(2 * y1, -1, p) % p
        else:
            l = (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (l * l - x1 - x2) % p
        return (x3, (l * (x1 - x3) - y1) % p)

    def neg(self, P):
        return None if P is None else (P[0], -P[1] % self.f.p)

    def mulk(self, k, P):
        r = None
        for bit in bin(k)[2:]:
            r = self.add(r, r)
            if bit == "1":
                r = self.add(r, P)
        return r

    def base_words(self, Q):
        f = self.f
        return [0] * (2 * f.N) if Q is None else f.words(Q[0] * f.R % f.p) + f.words(Q[1] * f.R % f.p)

    def acc_res(self, A, l):
        """residues of the accumulator (R 2^a l^2 x, R 2^b l^3 y, R 2^g l^2, R 2^d l^3)"""
        f, p = self.f, self.f.p
        return [(f.R << self.a) * l * l * A[0] % p, (f.R << self.bb) * l ** 3 * A[1] % p, (f.R << self.g) * l * l % p, (f.R << self.d) * l ** 3 % p]

    def red_res(self, A, l):
        """residues of a reduction point: (l^2 x, l^3 y, l^2, l^3) R'"""
        f, p = self.f, self.f.p
        return [f.Ru * l * l * A[0] % p, f.Ru * l ** 3 * A[1] % p, f.Ru * l * l % p, f.Ru * l ** 3 % p]

    def limbs(self, res, inv, sides, form, rng):
        f = self.f
        out = [f.sl(rep(c, b, s, f.p)) for c, b, s in zip(res, inv, sides)]
        return [f.neg_form(v, rng) for v in out] if form else out

    def acc(self, A, rng, sides=None, form=None, inv=G1_INV):
        sides = [rng.getrandbits(1) for _ in range(4)] if sides is None else sides
        return self.limbs(self.acc_res(A, rng.randrange(1, self.f.p)), inv, sides, rng.getrandbits(1) if form is None else form, rng)

    def red_point(self, A, rng, kind=None):
        """a reduction point as the kernels meet it: 0 loaded (the slices g1r_from_sat makes), 1 the largest representative a load can produce
        (just below 2^SH p), 2 / 3 computed (a product's output form / limbs in [-2^W, 2^W]) at the ends of g1u_madd's intervals"""
        f, p = self.f, self.f.p
        kind = rng.randrange(4) if kind is None else kind
        res = self.red_res(A, rng.randrange(1, p))
        if kind == 0:
            return [f.sl((c * pow(1 << f.SH, -1, p) % p) << f.SH) for c in res], kind
        if kind == 1:
            return [f.sl(c + ((1 << f.SH) - 1) * p) for c in res], kind
        return self.limbs(res, G1_INV, [rng.getrandbits(1) for _ in range(4)], kind == 3, rng), kind

    def check_acc(self, c, limbs4, inf, inv, ratio):
        """None, or why the record is not c.want (None: the identity).  ratio: ZZ^3 = ratio ZZZ^2; x = X 2^kx / ZZ, y = Y 2^ky / ZZZ (kx = ky = 0 in the reduction form)"""
        f, p = self.f, self.f.p
        if c.want is None:
            return None if inf == 1 else f"inf {inf:#x} on the identity"
        if inf != 0:
            return f"inf {inf:#x}"
        X, Y, ZZ, ZZZ = (f.val(v) for v in limbs4)
        if not all(10 * abs(v) < b * p for v, b in zip((X, Y, ZZ, ZZZ), inv)):
            return "outside the bound: |X|, |Y|, |ZZ|, |ZZZ| / p = " + ", ".join(f"{abs(v) / p:.3f}" for v in (X, Y, ZZ, ZZZ))
        if ZZ % p == 0 or (ZZ ** 3 - ratio * ZZZ ** 2) % p:
            return "ZZ^3 != ZZZ^2"
        kx, ky = (self.kx, self.ky) if ratio == f.R else (0, 0)
        got = ((X << kx) * pow(ZZ, -1, p) % p, (Y << ky) * pow(ZZZ, -1, p) % p)
        return None if got == c.want else f"affine ({got[0]:#x}, {got[1]:#x})"


def g1_field_jobs(g, rng):
    return [job_slice(g.f, s, rng) for s in (g.a, g.bb, g.sx, g.sy)]


def g1_jobs(g, rng):
    f, p, L, N = g.f, g.f.p, g.f.L, g.f.N
    name, RW, PART = g.name, 4 * g.f.L + 1, (4 * g.f.L + 1 + 3) // 4 * 4
    want_str = lambda c: "identity" if c.want is None else f"affine ({c.want[0]:#x}, {c.want[1]:#x})"
    flat = lambda limbs4: sum(limbs4, [])
    split = lambda ws: [f.signed(ws[L * k: L * k + L]) for k in range(4)]
    words4 = lambda vs: sum((f.words(v) for v in vs), [])
    garbage = [GARBAGE] * (4 * L)
    jobs = []

    # g1u_from_affine: plain slices; (0, 0) is infinity
    def chk_from_affine(c, out):
        y = f.sl(c.y << g.bb)
        want = f.sl(c.x << g.a) + ([-l for l in y] if c.neg else y) + f.sl((f.R << g.g) % p) + f.sl((f.R << g.d) % p) + [int(c.x == 0 and c.y == 0)]
        return None if f.signed(out) == want else (fmt(out), fmt(want))
    j = Job(f"{name}/g1u_from_affine", 2 * N + 1, RW, chk_from_affine)

    def add_fa(desc, x, y, neg):
        j.add(f"{desc}, neg {neg}", f.words(x) + f.words(y) + [neg], x=x, y=y, neg=neg)
    for neg in (0, 1):
        for x, y in ((0, 0), (0, 1), (1, 0), (p - 1, p - 1), (f.R % p, f.R % p)):
            add_fa(f"words ({x:#x}, {y:#x})", x, y, neg)
    for bn, Q in g.named:
        add_fa(bn, Q[0] * f.R % p, Q[1] * f.R % p, 0); add_fa(bn, Q[0] * f.R % p, Q[1] * f.R % p, 1)
    jobs.append(j.fill(lambda: (lambda Q: add_fa("random point", Q[0] * f.R % p, Q[1] * f.R % p, rng.getrandbits(1)))(rng.choice(g.pool)), N_POINT))

    # g1u_from_xyzz: four constant multiplications
    def chk_from_xyzz(c, out):
        r = split(out)
        ok = out[4 * L] == int(c.w[2] == 0) and all(f.unique(v) for v in r)
        for v, w, k in zip(r, c.w, (g.a, g.bb, g.g, g.d)):
            ok = ok and f.val(v) % p == (w << k) % p and abs(f.val(v)) < w * p // f.Ru + p + 1
        return None if ok else (fmt(out), "X 2^a, Y 2^b, ZZ 2^g, ZZZ 2^d mod p, |value| < 1.1 p")
    j = Job(f"{name}/g1u_from_xyzz", 4 * N, RW, chk_from_xyzz)

    def add_fx(desc, w):
        for v, k in zip(w, (g.a, g.bb, g.g, g.d)):
            f.m.mul(f.m.slice(v, 0), f.m.slice((f.Ru << k) % p, 0))
        j.add(desc, words4(w), w=w)
    add_fx("the identity (1, 1, 0, 0)", (f.R % p, f.R % p, 0, 0))
    add_fx("coordinates p - 1", (p - 1,) * 4)

    def rand_fx():
        A, l = rng.choice(g.pool), rng.randrange(1, p)
        add_fx("random point, random scale", tuple(v * f.R % p for v in (l * l * A[0], l ** 3 * A[1], l * l, l ** 3)))
    jobs.append(j.fill(rand_fx, N_POINT))

    # g1u_madd
    def chk_madd(c, out):
        if c.path == "base at infinity":
            return None if out == c.acc_words else (fmt(out), "the accumulator unchanged")
        inv = (10 << g.a, 10 << g.bb, 10, 10) if c.path == "accumulator at infinity" else G1_INV
        why = g.check_acc(c, split(out), out[4 * L], inv, f.R)
        return None if why is None else (fmt(out) + " " + why, want_str(c))
    j = Job(f"{name}/g1u_madd", RW + 2 * N + 1, RW, chk_madd)

    def add_madd(desc, A, limbs, Q, neg):
        """A: the accumulator's point (None: the flag is set and limbs are garbage words)"""
        Qs = g.neg(Q) if neg else Q
        path = "base at infinity" if Q is None else "accumulator at infinity" if A is None else "exceptional" if A[0] == Q[0] else "addition"
        acc_words = [w & 0xffffffff for w in (garbage if A is None else flat(limbs)) + [int(A is None)]]
        model = None
        if path in ("exceptional", "addition"):
            r = g.m.madd(tuple(limbs), (Q[0] * f.R % p, Q[1] * f.R % p), bool(neg))       # the model's limb, column and zero-test-range assertions
            assert (r is None) == (path == "exceptional")
            model = "exceptional" if r is None else g.m.to_affine(r)
        j.add(f"{path}: {desc}, neg {neg}", acc_words + g.base_words(Q) + [neg], want=g.add(A, Qs), path=path, acc_words=acc_words, model=model)

    def normal():
        A, Q = rng.sample(g.pool, 2)
        add_madd("random points", A, g.acc(A, rng), Q, rng.getrandbits(1))

    def exceptional():
        """acc = +-(neg ? -Q : Q), every coordinate at an end of its interval"""
        Q, same, neg = rng.choice(g.pool), rng.getrandbits(1), rng.getrandbits(1)
        Qs = g.neg(Q) if neg else Q
        A = Qs if same else g.neg(Qs)
        add_madd(f"acc = {'' if same else '-'}(base)", A, g.acc(A, rng), Q, neg)
    exceptional()                                                              # wave 0: one exceptional lane, 63 ordinary ones
    for _ in range(63):
        normal()
    normal()                                                                   # wave 1: the reverse
    for _ in range(63):
        exceptional()
    Q0 = g.pool[0]
    for same in (1, 0):                                                        # P = U2 - X = 0, +-p, +-2p, ... as an integer: every representative the bounds allow
        for neg in (0, 1):
            for k in range(-5, 5):
                exceptional_k(g, rng, add_madd, Q0, same, neg, k, None)
            for k in range(-3, 3):
                exceptional_k(g, rng, add_madd, Q0, same, neg, None, k)
    for Q in g.pool[:4]:
        for neg in (0, 1):
            add_madd("accumulator flagged, coordinates 0xA5..", None, None, Q, neg)
            add_madd("base all-zero words", Q, g.acc(Q, rng), None, neg)
    add_madd("both at infinity", None, None, None, 0)
    for bi, (bn, Q) in enumerate(g.named):                                     # every side pattern against each named base; then the named points as accumulators
        for pat in range(16):
            A = rng.choice(g.pool)
            add_madd(f"sides {pat:04b}, base {bn}", A, g.acc(A, rng, [(pat >> k) & 1 for k in range(4)], (pat + bi) & 1), Q, (pat >> 1) & 1)
        for same in (1, 0):
            A = Q if same else g.neg(Q)
            add_madd(f"acc = {'' if same else '-'}base = {bn}", A, g.acc(A, rng), Q, 0)
        add_madd(f"acc = {bn}", Q, g.acc(Q, rng), rng.choice(g.pool), bi & 1)
    jobs.append(j.fill(normal, N_POINT))

    # g1u_store_part -> g1u_load_part
    def chk_part(c, out):
        vals = [f.val(v) for v in c.limbs]
        want = [w & 0xffffffff for w in flat(c.limbs) + [c.inf] + [0] * (PART - RW)]
        want += words4(((vals[0] << g.kx) % p, (vals[1] << g.ky) % p, 0 if c.inf else vals[2] % p, 0 if c.inf else vals[3] % p))
        return None if out == want else (fmt(out), fmt(want))
    j = Job(f"{name}/g1u_store_part -> g1u_load_part", RW, PART + 4 * N, chk_part)

    def add_part(desc, limbs, inf):
        g.m.to_saturated(tuple(limbs))                                         # asserts the preconditions of the reader's fu_to_packed<KB>
        j.add(desc, flat(limbs) + [inf], limbs=limbs, inf=inf)
    add_part("the identity as g1u_identity makes it", [[0] * L] * 4, 1)
    for pat in range(16):
        A = rng.choice(g.pool)
        add_part(f"sides {pat:04b}", g.acc(A, rng, [(pat >> k) & 1 for k in range(4)], pat & 1, (g.inv_x,) + G1_INV[1:]), 0)
    for Q in g.pool[:4]:
        add_part("an affine point as it entered", [f.sl((Q[0] * f.R % p) << g.a), f.sl((Q[1] * f.R % p) << g.bb), f.sl((f.R << g.g) % p), f.sl((f.R << g.d) % p)], 0)
    jobs.append(j.fill(lambda: add_part("random", g.acc(rng.choice(g.pool), rng, inv=(g.inv_x,) + G1_INV[1:]), 0), N_POINT))

    # g1r_from_sat
    def chk_from_sat(c, out):
        want = flat([f.sl(w << f.SH) for w in c.w]) + [int(c.w[2] == 0)]
        return None if f.signed(out) == want else (fmt(out), fmt(want))
    j = Job(f"{name}/g1r_from_sat", 4 * N, RW, chk_from_sat)
    for w in ((f.R % p, f.R % p, 0, 0), (p - 1,) * 4, (0, 0, 1, 1), (1, 1, 0, 1)):
        j.add(f"words {tuple(hex(v) for v in w)}", words4(w), w=w)
    jobs.append(j.fill(lambda: (lambda w: j.add("random words below p", words4(w), w=w))(tuple(rng.randrange(p) for _ in range(4))), N_POINT))

    red_inv = (10 * G1R_VB,) * 4
    rec = lambda P: garbage + [1] if P is None else flat(P) + [0]

    def chk_red(c, out):
        if c.same_as is not None:                                              # an operand handed through (the other one is the identity)
            return None if out == c.same_as else (fmt(out), fmt(c.same_as))
        why = g.check_acc(c, split(out), out[4 * L], red_inv, f.Ru)
        if why is None and c.want is not None and not all(abs(l) <= (1 << f.W) + 16 for v in split(out) for l in v[:-1]):
            why = "limbs beyond 2^W + 16"
        return None if why is None else (fmt(out) + " " + why, want_str(c))

    # g1r_dbl
    j = Job(f"{name}/g1r_dbl", RW, RW, chk_red)

    def add_dbl(kind=None):
        A = rng.choice(g.pool)
        P, kind = g.red_point(A, rng, kind)
        r = g.red.dbl(tuple(P))
        j.add(f"operand kind {kind}", rec(P), want=g.add(A, A), same_as=None, model=g.red.to_affine(r))
    j.add("the identity", rec(None), want=None, same_as=[w & 0xffffffff for w in rec(None)], model=None)
    for kind in range(4):
        for _ in range(8):
            add_dbl(kind)
    jobs.append(j.fill(add_dbl, N_POINT))

    # g1r_add
    j = Job(f"{name}/g1r_add", 2 * RW, RW, chk_red)

    def add_add(desc, A, P, B, Q):
        """A, B: the points (None: flagged, garbage coordinates); P, Q: their limbs"""
        same_as, model = None, None
        if A is None or B is None:
            same_as = [w & 0xffffffff for w in (rec(Q) if A is None else rec(P))]
        else:
            r = g.red.add(tuple(P), tuple(Q))                                 # the model's limb, column and zero-test-range assertions
            model = g.red.to_affine(r)
        j.add(desc, rec(P) + rec(Q), want=g.add(A, B), same_as=same_as, model=model)

    def normal_r():
        A, B = rng.sample(g.pool, 2)
        (P, ka), (Q, kb) = g.red_point(A, rng), g.red_point(B, rng)
        add_add(f"random points, operand kinds {ka} {kb}", A, P, B, Q)

    def exceptional_r(vx=None):
        A = rng.choice(g.pool)
        B = A if rng.getrandbits(1) else g.neg(A)
        (P, ka), (Q, kb) = g.red_point(A, rng), g.red_point(B, rng)
        if vx is not None:                                                     # the second operand computed, its X at every representative the bounds allow
            res = g.red_res(B, rng.randrange(1, p))
            Q = g.limbs(res, G1_INV, [rng.getrandbits(1) for _ in range(4)], 0, rng); kb = 2
            if 10 * abs(res[0] + vx * p) < G1_INV[0] * p:
                Q[0] = f.sl(res[0] + vx * p)
        add_add(f"b = {'' if B == A else '-'}a, operand kinds {ka} {kb}{'' if vx is None else f', X shifted by {vx} p'}", A, P, B, Q)
    exceptional_r()
    for _ in range(63):
        normal_r()
    normal_r()
    for _ in range(63):
        exceptional_r()
    for k in range(-5, 5):
        exceptional_r(k); exceptional_r(k)
    for ka in range(4):                                                        # every pair of operand kinds, both the same point and different ones
        for kb in range(4):
            A, B = rng.sample(g.pool, 2)
            add_add(f"operand kinds {ka} {kb}", A, g.red_point(A, rng, ka)[0], B, g.red_point(B, rng, kb)[0])
            add_add(f"a + a, operand kinds {ka} {kb}", A, g.red_point(A, rng, ka)[0], A, g.red_point(A, rng, kb)[0])
            add_add(f"a - a, operand kinds {ka} {kb}", A, g.red_point(A, rng, ka)[0], g.neg(A), g.red_point(g.neg(A), rng, kb)[0])
    for bn, B in g.named:                                                      # the named points as freshly loaded operands (x = 0 loads as zero limbs)
        A = rng.choice(g.pool)
        add_add(f"b = {bn} loaded", A, g.red_point(A, rng)[0], B, g.red_point(B, rng, 0)[0])
        add_add(f"a = b = {bn} loaded", B, g.red_point(B, rng, 0)[0], B, g.red_point(B, rng, 1)[0])
    A = g.pool[1]
    add_add("a flagged, coordinates 0xA5..", None, None, A, g.red_point(A, rng, 1)[0])
    add_add("b flagged, coordinates 0xA5..", A, g.red_point(A, rng, 1)[0], None, None)
    add_add("both flagged", None, None, None, None)
    jobs.append(j.fill(normal_r, N_POINT))

    # g1r_to_sat
    def chk_to_sat(c, out):
        conv = f.R * pow(f.Ru, -1, p)
        want = words4((f.R % p, f.R % p, 0, 0)) if c.inf else words4(tuple(f.val(v) * conv % p for v in c.limbs))
        return None if out == want else (fmt(out), fmt(want))
    j = Job(f"{name}/g1r_to_sat", RW, 4 * N, chk_to_sat)

    def add_ts(kind=None):
        P, kind = g.red_point(rng.choice(g.pool), rng, kind)
        one = f.m.slice_pos(f.R % p)
        for v in P:
            f.m.to_packed(f.m.mul(v, one))                                     # asserts the preconditions of the product and of fu_to_packed<2>
        j.add(f"operand kind {kind}", rec(P), limbs=P, inf=0)
    j.add("the identity, zero limbs", [0] * (4 * L) + [1], limbs=None, inf=1)
    for kind in range(4):
        for _ in range(8):
            add_ts(kind)
    jobs.append(j.fill(add_ts, N_POINT))

    # g1r_store -> g1r_load
    def chk_store(c, out):
        zz_zero = all(l == 0 for l in c.limbs[2])
        want = [w & 0xffffffff for w in flat(c.limbs) + [c.inf] + [0] * (PART - RW) + flat(c.limbs) + [int(c.inf != 0 or zz_zero)]]
        got = out[:PART + RW]                                                  # (the record is padded to whole 16-byte stores)
        return None if got == want else (fmt(got), fmt(want))
    j = Job(f"{name}/g1r_store -> g1r_load", RW, (PART + RW + 3) // 4 * 4, chk_store)
    j.add("all-zero words: a bucket nothing was written to", [0] * RW, limbs=[[0] * L] * 4, inf=0)
    j.add("flagged", flat([[1] * L] * 4) + [1], limbs=[[1] * L] * 4, inf=1)
    j.add("flag word 0x80000000", flat([[1] * L] * 4) + [1 << 31], limbs=[[1] * L] * 4, inf=1 << 31)

    def add_st():
        P, kind = g.red_point(rng.choice(g.pool), rng)
        j.add(f"operand kind {kind}", rec(P), limbs=P, inf=0)
    jobs.append(j.fill(add_st, N_POINT))
    # the order of the probe: from_affine, from_xyzz, madd, part, g1r_from_sat, g1r_dbl, g1r_add, g1r_to_sat, g1r_store
    return jobs


def exceptional_k(g, rng, add_madd, Q, same, neg, kx, ky):
    """acc = +-(neg ? -Q : Q) with X (or Y) at the representative `residue + k p`, wherever that is inside the bound: P = U2 - X (R = S2 - Y) is then
    a multiple of p that runs over every value the bounds allow, and PP comes out as zero limbs for some and as p's for others"""
    f, p = g.f, g.f.p
    Qs = g.neg(Q) if neg else Q
    A = Qs if same else g.neg(Qs)
    res = g.acc_res(A, rng.randrange(1, p))
    limbs = g.limbs(res, G1_INV, [rng.getrandbits(1) for _ in range(4)], 0, rng)
    what = ""
    if kx is not None and 10 * abs(res[0] + kx * p) < G1_INV[0] * p:
        limbs[0] = f.sl(res[0] + kx * p); what = f", X = residue {kx:+d} p"
    if ky is not None and 10 * abs(res[1] + ky * p) < G1_INV[1] * p:
        limbs[1] = f.sl(res[1] + ky * p); what = f", Y = residue {ky:+d} p"
    add_madd(f"acc = {'' if same else '-'}(base){what}", A, limbs, Q, neg)


# ------------------------------------------------------------------------------------------------------------------ square root

def job_sqrt(f, rng):
    p, Ri = f.p, pow(f.R, -1, f.p)

    def check(c, out):
        flag, x = out[0], f.unwords(out[1:9]) * Ri % p
        ok = out[:9] == out[9:] and flag in (0, 1)                             # fu_sqrt_ratio_nf and fp_sqrt_ratio_nf, bit for bit
        if c.u:                                                                # (u = 0: the root is 0 and the flag is whatever the two agree on)
            ok = ok and flag == int(pow(c.u * pow(c.v, -1, p) % p, (p - 1) // 2, p) == 1)
        if ok and (flag or c.u == 0):
            ok = x * x * c.v % p == c.u
        return None if ok else (fmt(out[:9]) + " / " + fmt(out[9:]), f"flag {int(pow(c.u * pow(c.v, -1, p) % p, (p - 1) // 2, p) == 1) if c.u else 'any'}, x^2 v = u")
    j = Job(f"{f.name}/fu_sqrt_ratio_nf | fp_sqrt_ratio_nf", 16, 18, check)

    def add(desc, u, v):
        u, v = u % p, v % p
        assert v
        j.add(f"{desc}: u = {u:#x}, v = {v:#x}", f.words(u * f.R % p) + f.words(v * f.R % p), u=u, v=v)
    nonsq = next(n for n in range(2, 100) if pow(n, (p - 1) // 2, p) == p - 1)
    sp = [1, p - 1, 2, (p - 1) // 2]
    add("u = 0", 0, 1); add("u = 0", 0, rng.randrange(1, p)); add("u = v", 5, 5); add("u = v", p - 1, p - 1)
    for u in sp:
        for v in sp:
            add("small / extreme", u, v)
    for _ in range(32):
        x, v = rng.randrange(1, p), rng.randrange(1, p)
        add("u / v a square", x * x * v, v)
        add("u / v a non-square", nonsq * x * x * v, v)
    for _ in range(256):
        add("random", rng.randrange(p), rng.randrange(1, p))
    return j.fill(lambda: add("random", rng.randrange(p), rng.randrange(1, p)), 64)


# ------------------------------------------------------------------------------------------------------------------ the file

@functools.lru_cache(maxsize=None)
def jobs(seed=950):
    """every job, in the order of tools/fpu_probe.hip's main()"""
    rng = random.Random(seed)
    C = M.parse()
    flds = {n: Fld(n, C) for n in FIELDS}
    out = []
    for n in FIELDS:
        out += field_jobs(flds[n], rng)
        if n in G1_OF_FIELD:
            out += g1_field_jobs(G1c(G1_OF_FIELD[n], C, flds[n], rng), rng)
    out.append(job_packed(flds["FqBls12381"], 4, rng))
    for n in SUITES:
        out += te_jobs(TEc(n, C, flds[C[n]["Fq"]], rng), rng)
    for n in CURVES:
        out += g1_jobs(G1c(n, C, flds[C[n]["Fq"]], rng), rng)
    out += [job_sqrt(flds[n], rng) for n in SQRT_FIELDS]
    assert all(len(j.cases) % 64 == 0 and j.cases for j in out)
    return out


def jobs_of(variant, seed=950):
    """the jobs a build of the probe runs: all of them, or -- with -DAVRF_NO_FPU_ASM -- all but the square roots at the end of the list (the probe leaves
    them out of that build: fu_sqrt_ratio_nf is an out-of-line function, and with the C++ multipliers inlined into it it is the shape
    tools/lint_device_code.py fences off)"""
    js = jobs(seed)
    return js if variant == "asm" else js[:len(js) - len(SQRT_FIELDS)]


def pack(js):
    b = bytearray()
    for i, j in enumerate(js):
        b += struct.pack("<4I", i, len(j.cases), j.in_w, j.out_w)
        for c in j.cases:
            b += struct.pack(f"<{j.in_w}I", *c.words)
    return bytes(b)


def unpack_input(data):
    """the bytes of an input file -> [(index, in_w, out_w, [words per case])]"""
    out, pos = [], 0
    while pos < len(data):
        i, n, in_w, out_w = struct.unpack_from("<4I", data, pos); pos += 16
        out.append((i, in_w, out_w, [list(struct.unpack_from(f"<{in_w}I", data, pos + 4 * in_w * k)) for k in range(n)]))
        pos += 4 * in_w * n
    assert pos == len(data)
    return out


def unpack(data, js):
    """the bytes of an output file -> per job, per case, the list of its words (lengths checked)"""
    out, pos = [], 0
    for j in js:
        n = len(j.cases)
        assert pos + 4 * j.out_w * n <= len(data), "output file too short"
        out.append([list(struct.unpack_from(f"<{j.out_w}I", data, pos + 4 * j.out_w * k)) for k in range(n)])
        pos += 4 * j.out_w * n
    assert pos == len(data), "output file too long"
    return out


def failures(js, outs, limit=4):
    """[(job, number of bad cases, [(case description, got, want)] for the first `limit`)] over every case of every job"""
    bad = []
    for j, rows in zip(js, outs):
        errs = [(c, e) for c, e in ((c, j.check(c, row)) for c, row in zip(j.cases, rows)) if e is not None]
        if errs:
            bad.append((j.name, len(errs), [(c.desc, "got " + e[0], "want " + e[1]) for c, e in errs[:limit]]))
    return bad
