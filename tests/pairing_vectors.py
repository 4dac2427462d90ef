"""Operands and expected values, from oracle/pairing_py.F12 and Python integers, for the two programs that run the pairing layers on a file of
operands: tools/pairing_probe.hip (pairing_dev.h: Fp12 over sixteen lanes, k_g2_lines, the Miller loop and the final exponentiation; GPU) and
tests/cpp/host_pairing_values.cpp (host_pairing.h: the Fp2/Fp6/Fp12 tower, Granger-Scott squaring, G2Lines, the three Miller products; CPU).
Both read and write the layout documented at the top of tools/pairing_probe.hip; the device program takes an Fp12 element as its twelve
coefficients d_k of w^k in the direct basis Fp[w]/(w^12 - 2 xi0 w^6 + xi0^2 + 1) -- the model of oracle/pairing_py.F12 -- the host program as the
twelve words of its struct F12 (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, each a | b), which by the map documented at f12_frob2 in
host_pairing.h are the Fp2 coefficients A_k = a_k + b_k u of w^0, w^2, w^4, w^1, w^3, w^5 with u = w^6 - xi0: d_k = a_k - xi0 b_k, d_(k+6) = b_k.
Nothing here reads consts_gen.h or any output of the code under test."""
import math
import os
from contextlib import contextmanager

from oracle import pairing_py as PP
from oracle import ring_py as R
from oracle.pairing_py import F12

from conftest import GOLDEN

OPS = {"mul": 1, "sqr": 2, "mul_line": 3, "conj": 4, "frob2": 5, "frob1": 6, "inv": 7, "pow_x": 8, "final_exp": 9, "cyclo_sqr": 10,
       "g2_lines": 11, "miller": 12, "miller_fe": 13}
ARITY = {"mul": 2, "mul_line": 2}                          # every other Fp12 operation takes one element
# curve id -> (name in pairing_py, 32-bit words per Fp value, the curve parameter x, SRS fixture)
CURVES = {0: ("bls12_381", 12, -0xd201000000010000, "bls12-381-srs-2-11-uncompressed-zcash.bin"),
          1: ("bn254", 8, 4965661367192848881, "bn254-testing-2-9-uncompressed.bin")}
LINE_POS = {True: (0, 2, 3, 6, 8), False: (0, 1, 3, 7, 9)}  # non-zero coefficients of a line: M-twist, D-twist
TOWER_K = (0, 2, 4, 1, 3, 5)                               # power of w of c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2


@contextmanager
def curve(cid):
    """pairing_py computes on one global curve: select it for the block, then put the default back."""
    PP.use_curve(CURVES[cid][0])
    try:
        yield
    finally:
        PP.use_curve("bls12_381")


def exponents(cid):
    """(E, H): the exponent the final exponentiation claims, E = (p^6 - 1)(p^2 + 1) H, from p, r and x alone."""
    name, _, x, _ = CURVES[cid]
    p, r = PP.CURVES[name]["P"], PP.CURVES[name]["R"]
    cyc = p ** 4 - p ** 2 + 1
    assert cyc % r == 0
    if cid == 0:
        H = (x - 1) ** 2 * (x + p) * (x * x + p * p - 1) + 3
        assert H == 3 * (cyc // r)
    else:
        H = cyc // r
    return (p ** 6 - 1) * (p ** 2 + 1) * H, H


def conj(a):
    """a^(p^6): w -> -w (w^(p^6) = -w because w^6 = xi is not a square in Fp6).  The conj section checks this map against F12.__pow__."""
    return F12([-c if k & 1 else c for k, c in enumerate(a.c)])


def embed2_at(v, j):
    """the Fp2 value v = (a, b) times w^j, j < 6, as direct coefficients"""
    c = [0] * 12
    c[j], c[j + 6] = (v[0] - PP.XI0 * v[1]) % PP.P, v[1] % PP.P
    return c


# ---------------------------------------------------------------- lines of a fixed G2 argument, by affine Fp2 arithmetic on the twist

def g2_lines(q):
    """[(lam, c)] per step of the ate loop (one per doubling, one more per set bit): slope and c = lam x_T - y_T, T the running point."""
    f2m, f2s, f2a, f2i = PP.f2_mul, PP.f2_sub, PP.f2_add, PP.f2_inv
    (qx, qy), (tx, ty) = q, q
    out = []
    for i in range(PP.ATE_LOOP.bit_length() - 2, -1, -1):
        lam = f2m(f2m((3, 0), f2m(tx, tx)), f2i(f2a(ty, ty)))
        out.append((lam, f2s(f2m(lam, tx), ty)))
        nx = f2s(f2s(f2m(lam, lam), tx), tx)
        tx, ty = nx, f2s(f2m(lam, f2s(tx, nx)), ty)
        if (PP.ATE_LOOP >> i) & 1:
            lam = f2m(f2s(qy, ty), f2i(f2s(qx, tx)))
            out.append((lam, f2s(f2m(lam, tx), ty)))
            nx = f2s(f2s(f2m(lam, lam), tx), qx)
            tx, ty = nx, f2s(f2m(lam, f2s(tx, nx)), ty)
    return out


def line_table(lines):
    """the steps x 36 values k_g2_lines writes for one argument, as plain integers: {T0[12], TX[12], TY[12]} per step with the line at
    P = (xP, yP) being T0 + TX xP + TY yP:  M-twist c at w^0, -lam at w^2, 1 at w^3;  D-twist 1 at w^0, -lam at w^1, c at w^3."""
    out = []
    for lam, c in lines:
        neg = ((-lam[0]) % PP.P, (-lam[1]) % PP.P)
        one = [0] * 12
        if PP.MTWIST:
            one[3] = 1
            out += embed2_at(c, 0) + embed2_at(neg, 2) + one
        else:
            one[0] = 1
            out += embed2_at(c, 3) + embed2_at(neg, 1) + one
    return out


def line_at(lam, c, pt):
    """the line of one step evaluated at the G1 point pt, as an F12"""
    m = ((-lam[0] * pt[0]) % PP.P, (-lam[1] * pt[0]) % PP.P)
    if PP.MTWIST:
        parts = (embed2_at(c, 0), embed2_at(m, 2), embed2_at((pt[1], 0), 3))
    else:
        parts = (embed2_at((pt[1], 0), 0), embed2_at(m, 1), embed2_at(c, 3))
    return F12([sum(v) for v in zip(*parts)])


def miller(tables, pts):
    """f <- f^2, then f <- f l_s(P_q) for every pair q whose G1 point is not at infinity, per step s"""
    f, s = F12.one(), 0
    for i in range(PP.ATE_LOOP.bit_length() - 2, -1, -1):
        f = f * f
        for _ in range(2 if (PP.ATE_LOOP >> i) & 1 else 1):
            for tab, pt in zip(tables, pts):
                if pt is not None:
                    f = f * line_at(tab[s][0], tab[s][1], pt)
            s += 1
    assert all(s == len(t) for t in tables)
    return f


# ---------------------------------------------------------------- the cases

def sections(cid, rng, host=False):
    """The operations of one curve in file order: a list of dicts {op, labels, and either `items` (tuples of F12 operands) or `qs` (G2 points) and,
    for the Miller sections, `pts` (per item the G1 point of each pair, None = infinity)} with `want`: per item the expected F12; for g2_lines
    per G2 point its [(lam, c)].  Call inside `with curve(cid)`.  host adds the cyclotomic squaring, which only the host code has."""
    name, _, x, srs_file = CURVES[cid]
    p, r = PP.P, PP.R_ORDER
    E, _ = exponents(cid)
    rnd = lambda: F12([rng.randrange(p) for _ in range(12)])
    pm1 = F12([p - 1] * 12)
    zero, one = F12.zero(), F12.one()
    mono = lambda i, v=1: F12([v if k == i else 0 for k in range(12)])
    hole = lambda i: F12([0 if k == i else p - 1 for k in range(12)])
    # Values cross the file boundary as Montgomery residues v R mod p, and the lazy accumulators add up products of RESIDUES: the operands at
    # the end of their interval are those whose residue is p - 1 (the value -1/R), not the value p - 1.  Both are run; `near` draws every residue
    # from the top 2^32 values below p, so that the quotient digits of the Montgomery reductions vary from case to case.
    Ri = pow(1 << (32 * CURVES[cid][1]), -1, p)
    res = lambda residues: F12([v * Ri for v in residues])
    top = res([p - 1] * 12)
    near = lambda: res([p - 1 - rng.randrange(1 << 32) for _ in range(12)])
    out = []

    def f12_section(op, cases, fn):
        items, labels = [c[1:] for c in cases], [c[0] for c in cases]
        out.append({"op": op, "items": items, "labels": labels, "want": [fn(*it) for it in items]})

    mul_cases = [("all p-1", pm1, pm1), ("zero zero", zero, zero), ("zero random", zero, rnd()), ("one one", one, one), ("one random", one, rnd())]
    mul_cases += [("(p-1)w^%d (p-1)w^%d" % (i, j), mono(i, p - 1), mono(j, p - 1)) for i in range(12) for j in range(12)]
    mul_cases += [("p-1 but 0 at %d, %d" % (i, (5 * i + 2) % 12), hole(i), hole((5 * i + 2) % 12)) for i in range(12)]
    mul_cases += [("random %d" % i, rnd(), rnd()) for i in range(61)]
    mul_cases += [("all residues p-1", top, top)] + [("residues near p-1, %d" % i, near(), near()) for i in range(24)]
    f12_section("mul", mul_cases, lambda a, b: a * b)

    sqr_cases = [("all p-1", pm1), ("zero", zero), ("one", one), ("all (p-1)/2", F12([(p - 1) // 2] * 12))]
    sqr_cases += [("(p-1)w^%d" % i, mono(i, p - 1)) for i in range(12)] + [("p-1 but 0 at %d" % i, hole(i)) for i in range(12)]
    sqr_cases += [("random %d" % i, rnd()) for i in range(61)]
    sqr_cases += [("all residues p-1", top)] + [("residues near p-1, %d" % i, near()) for i in range(24)]
    f12_section("sqr", sqr_cases, lambda a: a * a)

    pos = LINE_POS[PP.MTWIST]
    sparse = lambda vals: F12([vals[pos.index(k)] if k in pos else 0 for k in range(12)])
    ls = [("all p-1", sparse([p - 1] * 5))] + [("p-1 at %d" % pos[t], sparse([p - 1 if u == t else 0 for u in range(5)])) for t in range(5)]
    ls += [("random %d" % i, sparse([rng.randrange(p) for _ in range(5)])) for i in range(3)] + [("residues p-1", sparse([(p - 1) * Ri] * 5))]
    fs = [("all p-1", pm1)] + [("w^%d" % i, mono(i)) for i in range(12)] + [("random %d" % i, rnd()) for i in range(4)]
    fs += [("all residues p-1", top), ("residues near p-1", near())]
    f12_section("mul_line", [("f %s, l %s" % (fn_, ln), f, l) for fn_, f in fs for ln, l in ls], lambda f, l: f * l)

    frob_in = [("w^%d" % i, mono(i)) for i in range(12)] + [("all p-1", pm1)] + [("random %d" % i, rnd()) for i in range(16)]
    ap = [a ** p for _, a in frob_in]                                          # a^p, a^(p^2) = (a^p)^p, a^(p^6) = (a^(p^2))^(p^4): all by F12.__pow__
    ap2 = [a ** p for a in ap]
    ap6 = [a ** (p ** 4) for a in ap2]
    assert all(conj(a) == w for (_, a), w in zip(frob_in, ap6))
    for op, want in (("conj", ap6), ("frob2", ap2), ("frob1", ap)):
        out.append({"op": op, "items": [(a,) for _, a in frob_in], "labels": [n for n, _ in frob_in], "want": want})

    fp6 = rnd()
    inv_cases = [("one", one)] + [("w^%d" % i, mono(i)) for i in range(12)] + [("all p-1", pm1), ("in Fp", mono(0, rng.randrange(1, p)))]
    inv_cases += [("in Fp2", F12([rng.randrange(p) if k in (0, 6) else 0 for k in range(12)])), ("in Fp6", F12([c if k % 2 == 0 else 0 for k, c in enumerate(fp6.c)]))]
    inv_cases += [("random %d" % i, rnd()) for i in range(16)]
    f12_section("inv", inv_cases, lambda a: a.inv())
    assert all(a * w == one for (a,), w in zip(out[-1]["items"], out[-1]["want"]))

    pow_cases = [("random %d" % i, rnd()) for i in range(8)] + [("all p-1", pm1)]
    if host:                                   # the host squares with f12_cyclo_sqr: its operands are mapped into the cyclotomic subgroup
        pow_cases = [("cyclotomic of " + n, a ** ((p ** 6 - 1) * (p ** 2 + 1))) for n, a in pow_cases]
    f12_section("pow_x", pow_cases, lambda a: conj(a ** -x) if x < 0 else a ** x)

    fe_cases = [("random %d" % i, rnd()) for i in range(6)] + [("one", one), ("in Fp", mono(0, rng.randrange(2, p)))]
    fe_cases += [("in Fp2", F12([rng.randrange(1, p) if k in (0, 6) else 0 for k in range(12)]))]
    f12_section("final_exp", fe_cases, lambda f: f ** E)

    if host:
        ts = [one] + [rnd() ** ((p ** 6 - 1) * (p ** 2 + 1)) for _ in range(5)]
        f12_section("cyclo_sqr", [("t = 1", ts[0])] + [("cyclotomic %d" % i, t) for i, t in enumerate(ts[1:])], lambda t: t * t)

    srs = R.Srs(R.SUITES[cid], open(os.path.join(GOLDEN, srs_file), "rb").read())
    dec = PP.g2_decode_zcash_uncompressed if cid == 0 else PP.g2_decode_arkworks_uncompressed
    enc = PP.g2_encode_zcash_uncompressed if cid == 0 else PP.g2_encode_arkworks_uncompressed
    g2, tau_g2 = dec(srs.g2_raw[0]), dec(srs.g2_raw[1])
    qs = [g2, tau_g2] + [dec(enc(PP.g2_mul(g2, k))) for k in (2, 3, r - 1)]
    qnames = ["g2", "tau g2", "2 g2", "3 g2", "(r-1) g2"]
    tabs = [g2_lines(q) for q in qs]
    out.append({"op": "g2_lines", "qs": qs, "labels": qnames, "want": tabs})

    g = srs.g1
    shapes = {1: [(1,), (0,), (1,), (0,), (0,), (1,)],                                      # which pairs of an item are live: the four groups
              2: [(1, 1), (0, 1), (1, 0), (0, 0), (1, 1), (0, 1)],                          # of the first wave all differ
              3: [(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1)]}
    which = {1: [4], 2: [0, 1], 3: [2, 3, 4]}                                               # the G2 arguments of the np-pair items
    for np_, shape in shapes.items():
        pts = [[g[1 + 3 * i + q] if live else None for q, live in enumerate(item)] for i, item in enumerate(shape)]
        sel = [tabs[j] for j in which[np_]]
        out.append({"op": "miller", "qs": [qs[j] for j in which[np_]], "pts": pts, "want": [miller(sel, item) for item in pts],
                    "labels": ["np %d, live %s" % (np_, item) for item in shape]})

    # Miller loop and final exponentiation together against the oracle's generic pairing: final_exp(prod miller_loop)^(E r / (p^12 - 1)).  The
    # oracle's lines differ from the tabulated ones by factors in proper subfields (a sign; w^3, in Fp4), which the easy part removes.
    full = p ** 12 - 1
    assert (E * r) % full == 0 and math.gcd(E * r // full, r) == 1
    neg = lambda pt: (pt[0], (-pt[1]) % p)
    pts = [[g[1], neg(g[0])], [g[1], neg(g[1])], [g[5], neg(g[4])], [g[2], g[7]], [None, g[3]]]   # true, broken, true, arbitrary, one pair alone
    want = []
    for a, b in pts:
        e = PP.final_exp(PP.miller_loop(g2, a) * PP.miller_loop(tau_g2, b)) ** (E * r // full)
        want.append(e)
    assert want[0] == one and want[2] == one and want[1] != one
    out.append({"op": "miller_fe", "qs": [g2, tau_g2], "pts": pts, "want": want,
                "labels": ["e(tau g1, g2) e(-g1, tau g2)", "e(tau g1, g2) e(-tau g1, tau g2)", "e(tau^5 g1, g2) e(-tau^4 g1, tau g2)",
                           "e(tau^2 g1, g2) e(tau^7 g1, tau g2)", "e(tau^3 g1, tau g2) alone"]})
    return out


# ---------------------------------------------------------------- the files

def to_tower(d, xi0, p):
    """direct coefficients -> the twelve words of the host's struct F12"""
    out = []
    for k in TOWER_K:
        out += [(d[k] + xi0 * d[k + 6]) % p, d[k + 6]]
    return out


def from_tower(t, xi0, p):
    d = [0] * 12
    for i, k in enumerate(TOWER_K):
        a, b = t[2 * i], t[2 * i + 1]
        d[k], d[k + 6] = (a - xi0 * b) % p, b
    return d


class Codec:
    """Montgomery residues of N words, and elements in the basis of the program addressed"""

    def __init__(self, cid, host):
        name, self.nl, _, _ = CURVES[cid]
        self.cid, self.host = cid, host
        self.p, self.xi0 = PP.CURVES[name]["P"], PP.CURVES[name]["XI0"]
        self.Rm = (1 << (32 * self.nl)) % self.p
        self.Ri = pow(self.Rm, -1, self.p)

    def fp(self, v):
        return (v * self.Rm % self.p).to_bytes(4 * self.nl, "little")

    def el(self, a):
        return b"".join(self.fp(v) for v in (to_tower(a.c, self.xi0, self.p) if self.host else a.c))

    def pack(self, secs):
        u32 = lambda v: v.to_bytes(4, "little")
        b = bytearray(u32(self.cid))
        for s in secs:
            if "items" in s:
                assert all(len(it) == ARITY.get(s["op"], 1) for it in s["items"])
                n, np_, body = len(s["items"]), 0, b"".join(self.el(a) for it in s["items"] for a in it)
            else:
                body = b"".join(self.fp(v) for q in s["qs"] for c in q for v in c)
                n, np_ = len(s["qs"]), 0
                if "pts" in s:
                    n, np_ = len(s["pts"]), len(s["qs"])
                    assert all(len(it) == np_ for it in s["pts"])
                    body += b"".join(self.fp(v) for it in s["pts"] for pt in it for v in (pt or (0, 0)))
            if not self.host:                      # the device geometry: four items per 64-lane block
                assert s["op"] == "g2_lines" or (n % 4 != 0 and n > 4), (s["op"], n)
            b += u32(OPS[s["op"]]) + u32(n) + u32(np_) + body
        return bytes(b)

    def expected(self, secs):
        """[(label, integer)] of every value of the output file, in file order (plain integers, out of Montgomery form)"""
        out = []
        for s in secs:
            op = s["op"]
            if op == "g2_lines":
                for qn, lines in zip(s["labels"], s["want"]):
                    if self.host:
                        vals = [v for lam, c in lines for v in lam + c]
                        out += [("%s of %s, step %d, %s" % (op, qn, i // 4, ("lam.a", "lam.b", "c.a", "c.b")[i % 4]), v) for i, v in enumerate(vals)]
                    else:
                        vals = line_table(lines)
                        out += [("%s of %s, step %d, %s[%d]" % (op, qn, i // 36, ("T0", "TX", "TY")[i % 36 // 12], i % 12), v) for i, v in enumerate(vals)]
                out.append((op + " flag", None))
                continue
            forms = ("generic", "lines", "lines_par") if self.host and op in ("miller", "miller_fe") else ("",)
            for form in forms:
                for label, w in zip(s["labels"], s["want"]):
                    out += [("%s %s [%s] coefficient %d" % (op, form, label, k), v) for k, v in enumerate(w.c)]
        return out

    def unpack(self, data, secs):
        """the output file as plain integers in the order of expected(): elements back in the direct basis, the flag word as it is"""
        sz, exp = 4 * self.nl, self.expected(secs)
        assert len(data) == sz * len(exp), "output file has %d bytes, expected %d" % (len(data), sz * len(exp))
        raw = [int.from_bytes(data[sz * i: sz * (i + 1)], "little") for i in range(len(exp))]
        vals, i = [], 0
        while i < len(exp):
            w = 1 if exp[i][1] is None or exp[i][0].startswith("g2_lines") else 12
            chunk = raw[i: i + w]
            if exp[i][1] is None:
                vals += chunk
            elif any(v >= self.p for v in chunk):              # not reduced: never equal to an expected value
                vals += [-v - 1 for v in chunk]
            else:
                el = [v * self.Ri % self.p for v in chunk]
                vals += from_tower(el, self.xi0, self.p) if self.host and w == 12 else el
            i += w
        return vals

    def mismatches(self, data, secs):
        """[(label, got, want)] over every value of the output file; the flag of k_g2_lines / g2_lines must be 0"""
        exp, got = self.expected(secs), self.unpack(data, secs)
        return [(label, hex(g) if g >= 0 else "not reduced: " + hex(-g - 1), hex(w or 0)) for (label, w), g in zip(exp, got) if g != (w or 0)]
