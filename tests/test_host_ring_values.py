"""The ring verifier's host arithmetic (host_ring.h: G1 decompression, the Fiat-Shamir schedule, HostRing::reduce, the batch randomisers) BY
VALUE, without a GPU: tests/cpp/host_ring_values.cpp, compiled with g++, runs every case and writes the status, the seven decoded points, the
7 alphas, zeta, the 8 nus and the 10 + 1 + 2 scalars of the two G1 sums; every value is compared, exactly, with oracle/ring_py.py
verifier_values (the function the oracle's own verify runs on) and the scalar formulas of SURVEY.md A.8:
    s[j] = r1 nu_j (j = 0..3, 7)   s4 = r1 nu4 + r2 nl a0   s5 = r1 nu5 + r2 nl a1 k1   s6 = r1 nu6 + r2 nl a2 k2   s8 = r1 zeta   s9 = r2 zeta w
    g = r1 v_agg + r2 lin_zw       second sum (-r1, -r2)
and the randomiser bytes with hashlib.shake_128 over the same concatenation.  Cases: all seven ring vectors of every suite oracle/ring_py.py
models (Bandersnatch and JubJub over BLS12-381, Baby-JubJub over BN254; it does not model the SW and SHAKE128 suites), each with seeded 128-bit
(r1, r2) and with (1, r2) -- the rule of a batch of one; per suite an evaluation >= r, lin_zw >= r and an instance coordinate >= r (InvalidData)
and a proof whose first commitment is the canonical point at infinity (decodes; its values are compared)."""
import hashlib
import json
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT
from oracle import ring_py as R
from test_oracle_ring import FILES

OK, INVALID = 0, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hrv") / "host_ring_values")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "host_ring_values.cpp"), "-o", out])
    return out


def _cases(s, vs, rng):
    """[(commitment, instance bytes, proof, r1, r2, expected status)]"""
    n, r = s.fp_bytes, s.r
    out = []
    for v in vs:
        com, proof = bytes.fromhex(v["ring_pks_com"]), bytes.fromhex(v["ring_proof"])
        x, y = R.te_decode(s, bytes.fromhex(v["proof_pk_com"]))
        inst = x.to_bytes(32, "little") + y.to_bytes(32, "little")
        r2 = rng.getrandbits(128)
        out.append((com, inst, proof, rng.getrandbits(128), r2, OK))
        out.append((com, inst, proof, 1, r2, OK))
    com, inst, proof, r1, r2, _ = out[0]
    ev, lz = 4 * n, 5 * n + 7 * 32
    big = lambda v: (v + r).to_bytes(32, "little")                                  # the same residue, not canonical (r < 2^255)
    out.append((com, inst, proof[:ev + 64] + big(int.from_bytes(proof[ev + 64: ev + 96], "little")) + proof[ev + 96:], r1, r2, INVALID))
    out.append((com, inst, proof[:lz] + big(int.from_bytes(proof[lz: lz + 32], "little")) + proof[lz + 32:], r1, r2, INVALID))
    out.append((com, inst[:32] + big(int.from_bytes(inst[32:], "little")), proof, r1, r2, INVALID))
    out.append((com, inst, R.g1_encode(s, None, True) + proof[n:], r1, r2, OK))
    return out


@pytest.mark.parametrize("suite", sorted(FILES), ids=lambda i: R.SUITES[i].name)
def test_host_ring_values(exe, tmp_path, golden_dir, suite):
    s = R.SUITES[suite]
    vec, srsf = FILES[suite]
    raw = open(os.path.join(golden_dir, srsf), "rb").read()
    srs = R.Srs(s, raw)
    vs = json.load(open(os.path.join(golden_dir, vec)))
    assert len(vs) == 7
    ring_size, n, r = 8, s.fp_bytes, s.r
    prm = R.Params(s, ring_size=ring_size)
    cases = _cases(s, vs, random.Random(20260 + suite))
    g1_raw = raw[8: 8 + 2 * n]
    vk = g1_raw + srs.g2_raw[0] + srs.g2_raw[1]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4I", suite, ring_size, len(cases), 0) + vk)
        for com, inst, proof, r1, r2, _ in cases:
            f.write(com + inst + proof + r1.to_bytes(32, "little") + r2.to_bytes(32, "little"))
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "host ring values ok", res.stdout + res.stderr
    got = open(fout, "rb").read()
    rec = 4 + 7 * 2 * n + 16 * 32 + 13 * 32
    assert len(got) == len(cases) * rec + 32 * len(cases)
    le = lambda v: (v % r).to_bytes(32, "little")
    bad = []
    for i, (com, inst, proof, r1, r2, want) in enumerate(cases):
        o = got[i * rec: (i + 1) * rec]
        status, = struct.unpack_from("<i", o, 0)
        if status != want:
            bad.append((i, "status", status, want))
            continue
        if want != OK:
            continue
        fixed = [R.g1_decode_compressed(s, com[n * j: n * j + n]) for j in range(3)]
        instance = (int.from_bytes(inst[:32], "little"), int.from_bytes(inst[32:], "little"))
        v = R.verifier_values(prm, srs, fixed, proof, instance)
        pts = v["C"] + [v["Cq"], v["pi1"], v["pi2"]]
        al, zeta, nu, nl, k1, k2 = v["alphas"], v["zeta"], v["nus"], v["nl"], v["k1"], v["k2"]
        s1 = [r1 * nu[j] for j in range(4)] + [r1 * nu[4] + r2 * nl * al[0], r1 * nu[5] + r2 * nl * al[1] * k1,
                                               r1 * nu[6] + r2 * nl * al[2] * k2, r1 * nu[7], r1 * zeta, r2 * zeta * prm.w]
        expect = b"".join(R.g1_encode(s, P, False) for P in pts) + b"".join(le(x) for x in al + [zeta] + nu + s1)
        expect += le(r1 * v["v_agg"] + r2 * v["lin_zw"]) + le(-r1) + le(-r2)
        names = ["point%d" % j for j in range(7)] + ["alpha%d" % j for j in range(7)] + ["zeta"] + ["nu%d" % j for j in range(8)] + \
                ["s%d" % j for j in range(10)] + ["g", "t0", "t1"]
        sizes = [2 * n] * 7 + [32] * 29
        assert len(expect) == rec - 4 == sum(sizes)
        at = 0
        for name, sz in zip(names, sizes):
            if o[4 + at: 4 + at + sz] != expect[at: at + sz]:
                bad.append((i, name))
            at += sz
    assert not bad, (len(bad), bad[:8])
    # one batch of all cases, case i against ring i: the bytes SHAKE128 absorbs, in order
    k = len(cases)
    g1 = srs.g1[0]
    msg = b"avrf-ring-batch" + struct.pack("<3Q", k, k, prm.N) + g1[0].to_bytes(n, "little") + g1[1].to_bytes(n, "little") + srs.g2_raw[0] + srs.g2_raw[1]
    msg += b"".join(struct.pack("<I", i) for i in range(k)) + b"".join(c[0] for c in cases) + b"".join(c[1] for c in cases) + b"".join(c[2] for c in cases)
    assert got[k * rec:] == hashlib.shake_128(msg).digest(32 * k)
