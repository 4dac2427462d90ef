"""The host pairing (host_pairing.h: Fp2/Fp6/Fp12 tower, Granger-Scott cyclotomic squaring, G2Lines, the three Miller products, the final
exponentiation) BY VALUE against oracle/pairing_py.F12 and Python integers: tests/cpp/host_pairing_values.cpp, compiled with g++, runs every
operation on the operands of tests/pairing_vectors.py -- the operand sets the device probe gets (tests/test_gpu_pairing_values.py) -- and every
value it writes is compared, exactly.  f12_mul, f12_sqr, f12_mul_line (against the dense product), f12_conj / f12_frob2 / f12_frob1 (against
a^(p^6), a^(p^2), a^p), f12_inv, f12_pow_x and f12_cyclo_sqr (operands mapped into the cyclotomic subgroup by Python), final_exp against f^E
for the exponent E its comment claims, every lam and c of g2_lines, and miller / miller_lines / miller_lines_par against the Miller recurrence
on the Python-computed lines (all three are the same field element: they multiply the same lines in the same order, and a product of Miller
functions is the Miller function of the product), with points at infinity; after final_exp they equal the oracle's generic pairing raised to
E r / (p^12 - 1).  No GPU."""
import os
import random
import subprocess

import pytest

import pairing_vectors as pv
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hpv") / "host_pairing_values")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "host_pairing_values.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("cid", [0, 1], ids=["bls12_381", "bn254"])
def test_host_pairing_values(exe, tmp_path, cid):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    codec = pv.Codec(cid, host=True)
    with pv.curve(cid):
        secs = pv.sections(cid, random.Random(12381 + cid), host=True)
        open(fin, "wb").write(codec.pack(secs))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "host pairing values ok", r.stdout + r.stderr
        bad = codec.mismatches(open(fout, "rb").read(), secs)
    assert {s["op"] for s in secs} == set(pv.OPS)
    assert not bad, (len(bad), bad[:6])
