"""Operands and expected values, from Python integers, for the two programs that run the Montgomery field layer on a file of operands:
tests/cpp/host_field_check.cpp (host_te.h HostField, CPU) and tools/field_probe.hip (fpn.h / fp256.h, GPU).  Both read and write the layout
documented at their top; both run the operations of OPS in this order."""
import os
import re
import struct

from conftest import ROOT

OPS = ["add", "sub", "neg", "dbl", "mul", "sqr", "to_mont", "from_mont", "inv", "inv_fermat", "ge_p", "roundtrip"]


def consts_fields():
    """[(name, limbs, p)] of every field struct of consts_gen.h, in file order."""
    text = open(os.path.join(ROOT, "ark_vrf_amd", "csrc", "consts_gen.h")).read()
    out = []
    for m in re.finditer(r"struct (F[qr]\w+) \{\s*static constexpr int N = (\d+);\s*static constexpr uint32_t P\[\d+\] = \{([^}]*)\};", text):
        words = [int(w.strip().rstrip("u"), 16) for w in m.group(3).split(",")]
        assert len(words) == int(m.group(2))
        out.append((m.group(1), len(words), sum(w << (32 * i) for i, w in enumerate(words))))
    return out


def cases(p, nl, rng, n_rand):
    """(pairs, wide): pairs (a, b) with a, b < p -- structured a (0, 1, p-1, p-2, (p-1)/2, 2^k +- 1, values whose top limb equals p's), each
    once against a structured and once against a random b, then n_rand random pairs; wide (a, b) with p <= a < 2^(32 nl), b < p."""
    top = 1 << (32 * nl)
    s = [0, 1, p - 1, p - 2, (p - 1) // 2]
    for k in range(32 * nl + 1):
        s += [v for v in ((1 << k) - 1, (1 << k) + 1) if v < p]
    ptop = p >> (32 * (nl - 1)) << (32 * (nl - 1))
    s += [ptop, ptop + (p - ptop) // 2, ptop + (p - ptop) // 2 + 1]                    # top limb equal to p's, below p
    s += [ptop + rng.randrange(p - ptop) for _ in range(8)]
    s = list(dict.fromkeys(s))
    assert all(0 <= v < p for v in s)
    pairs = [(a, s[(5 * i + 2) % len(s)]) for i, a in enumerate(s)] + [(a, rng.randrange(p)) for a in s]
    pairs += [(rng.randrange(p), rng.randrange(p)) for _ in range(n_rand)]
    w = [p, p + 1, top - 1, top - 2, (p + top) // 2] + [rng.randrange(p, top) for _ in range(59)]
    wide = [(a, b) for a, b in zip(w, [p - 1, 1, p - 1, 0, 2] + [rng.randrange(p) for _ in range(59)])]
    return pairs, wide


def expected(p, nl, pairs, wide):
    """The output blocks of one field, as a list of integers (one per item and block), in file order."""
    R = 1 << (32 * nl)
    Ri = pow(R, -1, p)
    inv = [R * R * pow(a, -1, p) % p if a else 0 for a, _ in pairs]
    f = {"add": [(a + b) % p for a, b in pairs], "sub": [(a - b) % p for a, b in pairs], "neg": [-a % p for a, _ in pairs],
         "dbl": [2 * a % p for a, _ in pairs], "mul": [a * b * Ri % p for a, b in pairs], "sqr": [a * a * Ri % p for a, _ in pairs],
         "to_mont": [a * R % p for a, _ in pairs], "from_mont": [a * Ri % p for a, _ in pairs], "inv": inv, "inv_fermat": inv,
         "ge_p": [0] * len(pairs), "roundtrip": [a for a, _ in pairs]}
    out = [v for op in OPS for v in f[op]] + [1] * len(wide)
    if p.bit_length() < 32 * nl:                          # top bit clear: a Montgomery product takes any first operand below R
        out += [a * b * Ri % p for a, b in wide]
    return out


def pack(fields):
    """fields: [(nl, pairs, wide)] -> the bytes of the input file."""
    b = bytearray()
    for nl, pairs, wide in fields:
        b += struct.pack("<II", len(pairs), len(wide))
        for a, c in pairs + wide:
            b += a.to_bytes(4 * nl, "little") + c.to_bytes(4 * nl, "little")
    return bytes(b)


def unpack(data, fields_expected):
    """data: the bytes of the output file; fields_expected: [(nl, expected list)] -> [list of integers] per field (lengths checked)."""
    out, pos = [], 0
    for nl, exp in fields_expected:
        sz = 4 * nl
        assert pos + sz * len(exp) <= len(data), "output file too short"
        out.append([int.from_bytes(data[pos + sz * i: pos + sz * (i + 1)], "little") for i in range(len(exp))])
        pos += sz * len(exp)
    assert pos == len(data), "output file too long"
    return out


def describe(nl, pairs, wide, idx):
    """which (operation, operands) item idx of a field's output is"""
    n = len(pairs)
    if idx < len(OPS) * n:
        return OPS[idx // n], tuple(hex(v) for v in pairs[idx % n])
    idx -= len(OPS) * n
    return ("ge_p" if idx < len(wide) else "mul") + " (wide)", tuple(hex(v) for v in wide[idx % len(wide)])
