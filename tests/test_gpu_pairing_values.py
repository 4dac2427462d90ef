"""The device pairing layer (pairing_dev.h) BY VALUE against oracle/pairing_py.F12 and Python integers: tools/pairing_probe.hip is compiled once
with the library's flags and run once per curve (BLS12-381, BN254) as a child process on the operands of tests/pairing_vectors.py; every
coefficient of every result is compared, exactly.  The probe's kernels have the library's geometry (64-lane blocks, sixteen lanes per element);
every operation runs at an item count that is no multiple of four and spans at least two blocks, so the partial last wave is always there.
  f12_mul, f12_sqr       every coefficient p - 1, zero, one, all (p-1) w^i (p-1) w^j (the index schedules against the 144 basis products),
                         p - 1 with one hole, random; and, because the lazy accumulators (four unreduced products per fold, acc < 2 p R) add
                         products of Montgomery RESIDUES, every coefficient with residue p - 1 and 24 cases with residues within 2^32 of it
  f12_mul_line           lines with the five coefficients of the twist type (all p - 1, each alone, random, residues p - 1) against the dense product
  f12_conj/frob2/frob1   against a^(p^6), a^(p^2), a^p by F12.__pow__;  f12_inv against F12.inv (subfield elements included)
  f12_pow_x              a^|x| (conjugated for BLS12-381's negative x) on arbitrary a
  pairing_final_exp      against f^E, E = (p^6 - 1)(p^2 + 1) H, H from p, r and x
  k_g2_lines             every entry of the tables of g2, tau g2, 2 g2, 3 g2, (r-1) g2 against affine Fp2 arithmetic in Python; flag 0
  pairing_miller         1, 2 and 3 pairs with points at infinity placed so that the four groups of a wave skip different pairs, against the
                         recurrence f <- f^2, f <- f l_s(P); and with the final exponentiation against the oracle's generic pairing."""
import os
import random
import subprocess
import sys

import pytest

import pairing_vectors as pv
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEVICE_OPS = [op for op in pv.OPS if op != "cyclo_sqr"]          # f12_cyclo_sqr exists on the host only
IDS = {0: "bls12_381", 1: "bn254"}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairing_probe") / "pairing_probe")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-enable-ipra=0", "-Wno-unused-value",
                           "-Wno-pass-failed", "-I", os.path.join(ROOT, "ark_vrf_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "pairing_probe.hip")])
    return exe


@pytest.fixture(scope="module")
def results(probe, tmp_path_factory):
    """{curve: (sections, mismatches) or an error string}: one child process per curve; after one that did not end well nothing more is started"""
    d, out, broken = tmp_path_factory.mktemp("pairing_values"), {}, None
    for cid in (0, 1):
        if broken:
            out[cid] = "not run: " + broken
            continue
        fin, fout = str(d / ("in%d.bin" % cid)), str(d / ("out%d.bin" % cid))
        codec = pv.Codec(cid, host=False)
        with pv.curve(cid):
            secs = pv.sections(cid, random.Random(12381 + cid))
            open(fin, "wb").write(codec.pack(secs))
            try:
                r = subprocess.run([probe, fin, fout], capture_output=True, text=True, timeout=120)
            except subprocess.TimeoutExpired:
                out[cid] = broken = "the probe of %s did not finish in 120 s" % IDS[cid]
                continue
            if r.returncode != 0 or "pairing probe ok" not in r.stdout:
                out[cid] = broken = "the probe of %s ended with status %d: %s" % (IDS[cid], r.returncode, r.stdout + r.stderr)
                continue
            out[cid] = (secs, codec.mismatches(open(fout, "rb").read(), secs))
    return out


def test_probe_passes_device_lint(probe):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_device_code.py"), probe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("op", DEVICE_OPS)
@pytest.mark.parametrize("cid", [0, 1], ids=[IDS[0], IDS[1]])
def test_pairing_values(results, cid, op):
    assert not isinstance(results[cid], str), results[cid]
    secs, bad = results[cid]
    assert [s["op"] for s in secs if s["op"] == op], "no section for " + op
    mine = [b for b in bad if b[0].split(" ")[0] == op]
    assert not mine, (len(mine), mine[:6])
