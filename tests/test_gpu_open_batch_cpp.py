"""thin::OpenBatchVerifier and pedersen::OpenBatchVerifier of the C++ mirror (include/avrf.hpp) on the reference's golden vectors: push
one by one, push_many, verify, verify_segments, len.  Compiled with g++ against libavrf.so as test_gpu_cpp_mirror.py compiles its client."""
import json
import os
import subprocess

import pytest

from conftest import ROOT
from helpers import proof_xy, xy

pytestmark = pytest.mark.gpu
NAMES = {0: "bandersnatch_sha-512_ell2", 1: "baby-jubjub_sha-512_tai", 5: "bandersnatch_shake128_ell2"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "open_batch_check")
    lib = os.path.join(ROOT, "ark_vrf_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "open_batch_check.cpp"),
                           "-o", out, "-L", lib, "-lavrf", f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("suite", [0, 1, 5])
def test_open_batch_verifiers(exe, golden_dir, tmp_path, suite):
    vt = json.load(open(os.path.join(golden_dir, NAMES[suite] + "_thin.json")))
    vp = json.load(open(os.path.join(golden_dir, NAMES[suite] + "_pedersen.json")))
    p = lambda h: xy(suite, bytes.fromhex(h)).hex()
    lines = []
    for t in vt:
        lines.append(" ".join(["thin", p(t["pk"]), p(t["h"]), p(t["gamma"]), t["ad"] or "-", proof_xy(suite, bytes.fromhex(t["proof_r"] + t["proof_s"]), 0).hex()]))
    for v in vp:
        pr = bytes.fromhex(v["proof_pk_com"] + v["proof_r"] + v["proof_ok"] + v["proof_s"] + v["proof_sb"])
        lines.append(" ".join(["ped", p(v["h"]), p(v["gamma"]), v["ad"] or "-", proof_xy(suite, pr, 1).hex()]))
    items = tmp_path / "items.txt"
    items.write_text("\n".join(lines) + "\n")
    res = subprocess.run([exe, str(suite), str(items)], capture_output=True, text=True, check=True).stdout
    kv = dict(line.split("=", 1) for line in res.strip().splitlines())
    assert len(vt) == len(vp) == 7
    assert kv == {"thin_empty": "0", "thin_one_by_one": "0", "thin_len": "7", "thin_segments": "00", "thin_after_bad": "1", "thin_segments_bad": "01",
                  "thin_len_bad": "8", "thin_many": "0", "thin_staged": "0", "thin_len_closed": "0", "thin_push_closed_throws": "1",
                  "ped_one_by_one": "0", "ped_len": "7", "ped_segments": "00", "ped_after_bad": "1", "ped_segments_bad": "010", "ped_many": "0"}
