"""The unsaturated-limb field and point layer on the device (csrc/fpu.h, fpu_asm_gen.h, fpu_te.h, fpu_g1.h, fpu_sqrt.h) at the ends of its
documented intervals, against Python integers.  tools/fpu_probe.hip is compiled twice with the library's flags -- as it ships, and with
-DAVRF_NO_FPU_ASM (the C++ multipliers in place of the generated asm blocks) -- and each binary runs once on the operands of
tests/fpu_vectors.py (the second build leaves the out-of-line square root out), one workgroup of 256 lanes per (type, operation).  Checked per case:
  fu_mul / fu_sqr            value(r) 2^(W L) = value(a) value(b) mod p, limbs 0..L-2 in [0, 2^W), |value(r)| < |a b| / 2^(W L) + p + 1, the limbs of
                             tools/fpu_model.py's multiplier, and the same limbs from both builds
  fu_slice / fu_cneg / fu_carry / fu_carry_u / fu_times5     the exact value and the limb ranges
  fu_to_packed<KB>           exactly value mod p;   the zero tests: the flags against value mod p == 0
  te / G1 point operations   the affine point of the group law, T Z = X Y (ZZ^3 = ZZZ^2), every coordinate inside its inductive bound, the
                             identity flag, the store / load round trips word for word
  fu_sqrt_ratio_nf           flag and root equal to fp_sqrt_ratio_nf's bit for bit, root^2 v = u, the flag against the Legendre symbol
The vectors are kept honest without a device by test_vectors_are_inside_the_contract_and_agree_with_the_model below."""
import os
import subprocess

import pytest

import fpu_vectors as fv
from conftest import ROOT

HIPCC_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-enable-ipra=0", "-Wno-unused-value", "-I", os.path.join(ROOT, "ark_vrf_amd", "csrc")]
VARIANTS = {"asm": [], "no_asm": ["-DAVRF_NO_FPU_ASM"]}


def test_vectors_are_inside_the_contract_and_agree_with_the_model():
    """No device: the generator runs (it asserts the model's preconditions case by case -- limb magnitudes, int64 columns, value bounds, the range of
    fu_to_packed and of the zero tests -- and fails loudly where a construction lands outside them), the file round-trips, every job fills whole
    waves, and the expected point of every point case is what the model's own addition gives on the same limbs."""
    js = fv.jobs()
    data = fv.pack(js)
    back = fv.unpack_input(data)
    assert len(back) == len(js)
    for k, (j, (i, in_w, out_w, rows)) in enumerate(zip(js, back)):
        assert (i, in_w, out_w) == (k, j.in_w, j.out_w) and rows == [c.words for c in j.cases], j.name
        assert len(j.cases) % 64 == 0 and len(j.cases) >= 64, j.name
    n_model = 0
    for j in js:
        for c in j.cases:
            if "model" not in c.ctx or c.model is None:
                continue
            n_model += 1
            if c.model == "exceptional":                          # the model's zero test fired: the law's exceptional inputs, and only those
                assert c.path == "exceptional", (j.name, c.desc)
            else:
                assert c.model == c.want, (j.name, c.desc, c.model, c.want)
    assert n_model > 3000
    names = [j.name for j in js]
    for must in ("FqBandersnatch/fu_mul", "FqBls12381/fu_sqr", "FqBls12381/fu_to_packed<4>", "FqBn254/zero tests", "SuiteJubJub/teu_madd", "SuiteEd25519/teu4_dbl",
                 "G1Bls12381/g1u_madd", "G1Bn254/g1r_add", "FqBabyJubJub/fu_sqrt_ratio_nf | fp_sqrt_ratio_nf"):
        assert must in names, must
    # the exceptional paths and both directions of the wave vote are there: wave 0 of g1u_madd / g1r_add has one exceptional lane, wave 1 one ordinary lane
    for j in js:
        if j.name.endswith("/g1u_madd"):
            exc = [c.path == "exceptional" for c in j.cases[:128]]
            assert sum(exc[:64]) == 1 and sum(exc[64:]) == 63, j.name
            assert {"exceptional", "addition", "accumulator at infinity", "base at infinity"} <= {c.path for c in j.cases}
            assert any(c.path == "exceptional" and c.want is None for c in j.cases) and any(c.path == "exceptional" and c.want is not None for c in j.cases)
        if j.name.endswith("/g1r_add"):
            exc = [c.desc.startswith("b = ") for c in j.cases[:128]]
            assert sum(exc[:64]) == 1 and sum(exc[64:]) == 63, j.name


@pytest.fixture(scope="module")
def probe_outputs(tmp_path_factory):
    """both variants compiled once and run once on the same input: {variant: per job, per case, the output words}"""
    d = tmp_path_factory.mktemp("fpu_probe")
    fins = {v: str(d / f"in_{v}.bin") for v in VARIANTS}
    for v in VARIANTS:                                             # the same operands; the no_asm build runs all jobs but the square roots (fv.jobs_of)
        open(fins[v], "wb").write(fv.pack(fv.jobs_of(v)))
    exes = {v: str(d / f"fpu_probe_{v}") for v in VARIANTS}
    procs = {v: subprocess.Popen(["/opt/rocm/bin/hipcc"] + HIPCC_FLAGS + extra + ["-o", exes[v], os.path.join(ROOT, "tools", "fpu_probe.hip")])
             for v, extra in VARIANTS.items()}                   # the two compiles side by side: they are the bulk of the wall time
    for v, pr in procs.items():
        assert pr.wait() == 0, f"hipcc failed for the {v} variant"
    outs = {}
    for v in VARIANTS:
        fout = str(d / f"out_{v}.bin")
        r = subprocess.run([exes[v], fins[v], fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "fpu probe ok" in r.stdout, (v, r.stdout + r.stderr)
        outs[v] = fv.unpack(open(fout, "rb").read(), fv.jobs_of(v))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fpu_probe(probe_outputs, variant):
    bad = fv.failures(fv.jobs_of(variant), probe_outputs[variant])
    assert not bad, (variant, len(bad), bad[:6])


@pytest.mark.gpu
def test_asm_and_cpp_multipliers_give_identical_limbs(probe_outputs):
    """fu_mul_asm / fu_sqr_asm against the C++ multipliers of fpu.h: every word of every job (everything else in the two builds is the same source)"""
    outs, bad = probe_outputs, []
    assert len(outs["no_asm"]) == len(fv.jobs_of("no_asm")) > 100
    for j, a, b in zip(fv.jobs_of("no_asm"), outs["asm"], outs["no_asm"]):
        diff = [i for i in range(len(a)) if a[i] != b[i]]
        if diff:
            bad.append((j.name, len(diff), [(j.cases[i].desc, "asm " + fv.fmt(a[i]), "no asm " + fv.fmt(b[i])) for i in diff[:4]]))
    assert not bad, (len(bad), bad[:6])
