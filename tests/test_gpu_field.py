"""The device field layer (fpn.h: one set of operations for every limb count; fp256.h's out-of-line inversion) against Python integers:
tools/field_probe.hip is compiled with the library's flags and run on the GPU box, one workgroup of 256 lanes per (field, operation).
Fields: FqBandersnatch (asm multiplier), FqEd25519, the two full-width fields of secp256r1, FqBn254 (8 limbs, G1 / pairing call sites) and
FqBls12381 (12 limbs).  Operations: add, sub, neg, dbl, mul, sqr, to_mont, from_mont, the GCD inversion and the fixed power a^(p-2), ge_p and
the 16-byte load / store round trip, on 0, 1, p-1, p-2, (p-1)/2, 2^k +- 1, values whose top limb equals p's and 4096 random pairs; mul also
with first operands in [p, 2^(32 N)) where the modulus leaves its top bit clear.  Every result is compared."""
import os
import random
import subprocess

import pytest

import field_vectors as fv
from conftest import ROOT

pytestmark = pytest.mark.gpu

PROBE_FIELDS = ["FqBandersnatch", "FqEd25519", "FqSecp256r1", "FrSecp256r1", "FqBn254", "FqBls12381"]      # the order of tools/field_probe.hip


def test_field_probe(tmp_path):
    by_name = {name: (nl, p) for name, nl, p in fv.consts_fields()}
    rng = random.Random(355)
    cs = [by_name[name] + fv.cases(by_name[name][1], by_name[name][0], rng, 4096) for name in PROBE_FIELDS]
    want = [(nl, fv.expected(p, nl, pairs, wide)) for nl, p, pairs, wide in cs]
    exe, fin, fout = str(tmp_path / "field_probe"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(fin, "wb").write(fv.pack([(nl, pairs, wide) for nl, _, pairs, wide in cs]))
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-enable-ipra=0", "-Wno-unused-value",
                           "-I", os.path.join(ROOT, "ark_vrf_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "field_probe.hip")])
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "field probe ok" in r.stdout, r.stdout + r.stderr
    got = fv.unpack(open(fout, "rb").read(), want)
    for name, (nl, p, pairs, wide), (_, w), g in zip(PROBE_FIELDS, cs, want, got):
        bad = [i for i in range(len(w)) if w[i] != g[i]]
        assert not bad, (name, len(bad), [fv.describe(nl, pairs, wide, i) + (hex(g[i]), hex(w[i])) for i in bad[:4]])
