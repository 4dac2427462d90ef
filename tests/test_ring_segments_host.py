"""The host side of the segmented ring verifier, without a GPU:
  * avrf_ring_segments_layout through libavrf.so (host arithmetic only): { L, rounds, padded terms of the largest round, window bits };
  * HostRing::segment_randomisers (host_ring.h, compiled with g++ by tests/cpp/host_ring_segments.cpp): the bytes every segment derives
    equal hashlib.shake_128 over the SEGMENT's own statement -- its item count, its slice of the ring indices, ALL the commitments,
    its instances and proofs, in the byte order of tests/test_host_ring_values.py -- and for one segment of everything they equal
    HostRing::batch_randomisers of the whole batch."""
import hashlib
import json
import os
import struct
import subprocess

import pytest

from conftest import ROOT
from oracle import ring_py as R
from test_oracle_ring import FILES

ERR_BAD_ARG = -2


def test_layout():
    """L = 10 (longest segment) + 1.  Window bits: the small-MSM rule of the engine, c = floor(log2 L) - 3, at least 4.  A round holds
    min(65535 // (2 W), 2^20 // (2 L), (2^32 - 2^16 - 1) // (2 W L)) segments, W = ceil(257 / c) windows of a 256-bit scalar: two vectors
    per segment under AVRF_SEGMENTS_WINDOWS_MAX, AVRF_SEGMENTS_PADDED_TERMS_MAX and the 32-bit entry offsets."""
    from ark_vrf_amd.ring import ring_segments_layout
    # 16 items: L = 161, c = 7 - 3 = 4, W = 65, 504 segments per round: one round of 256, 2 * 256 * 161 padded terms
    assert ring_segments_layout(4096, [16] * 256) == (161, 1, 82432, 4)
    # 600 one-item segments: L = 11, c = 4, 2 * 600 * 65 = 78 000 windows > 65 535: rounds of 504 and 96; the larger pads 2 * 504 * 11
    assert ring_segments_layout(600, [1] * 600) == (11, 2, 11088, 4)
    # the longest segment there is: L = 8191, c = 12 - 3 = 9, W = 29; the padded-terms limit holds 2^20 // 16 382 = 64 per round
    assert ring_segments_layout(819, [819]) == (8191, 1, 16382, 9)
    assert ring_segments_layout(5, [0, 0, 5]) == (51, 1, 306, 4)
    assert ring_segments_layout(0, []) == (1, 0, 0, 4)
    assert ring_segments_layout(7, [3, 3]) == ERR_BAD_ARG                      # counts that do not sum to n
    assert ring_segments_layout(5, [3, 3]) == ERR_BAD_ARG
    assert ring_segments_layout(820, [820]) == ERR_BAD_ARG                     # 10 * 820 + 1 > AVRF_SEGMENT_TERMS_MAX
    assert ring_segments_layout(821, [1, 820]) == ERR_BAD_ARG


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hrs") / "host_ring_segments")
    subprocess.check_call(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "host_ring_segments.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("suite", [0, 1], ids=lambda i: R.SUITES[i].name)
@pytest.mark.parametrize("segs", [[1, 2, 4], [7]], ids=str)
def test_segment_randomisers(exe, tmp_path, golden_dir, suite, segs):
    s = R.SUITES[suite]
    vec, srsf = FILES[suite]
    raw = open(os.path.join(golden_dir, srsf), "rb").read()
    srs = R.Srs(s, raw)
    vs = json.load(open(os.path.join(golden_dir, vec)))
    k, n, ring_size = len(vs), s.fp_bytes, 8
    assert k == 7 == sum(segs)
    prm = R.Params(s, ring_size=ring_size)
    coms = [bytes.fromhex(v["ring_pks_com"]) for v in vs]
    insts = []
    for v in vs:
        x, y = R.te_decode(s, bytes.fromhex(v["proof_pk_com"]))
        insts.append(x.to_bytes(32, "little") + y.to_bytes(32, "little"))
    proofs = [bytes.fromhex(v["ring_proof"]) for v in vs]
    vk = raw[8: 8 + 2 * n] + srs.g2_raw[0] + srs.g2_raw[1]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4I", suite, ring_size, k, len(segs)) + vk + struct.pack("<%dI" % len(segs), *segs))
        for i in range(k):
            f.write(coms[i] + insts[i] + proofs[i])
    res = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "host ring segments ok", res.stdout + res.stderr
    got = open(fout, "rb").read()
    assert len(got) == 2 * 32 * k
    g1 = srs.g1[0]
    key = g1[0].to_bytes(n, "little") + g1[1].to_bytes(n, "little") + srs.g2_raw[0] + srs.g2_raw[1]

    def statement(first, cnt):                                                  # what a batch call on these items alone absorbs
        msg = b"avrf-ring-batch" + struct.pack("<3Q", cnt, k, prm.N) + key
        msg += b"".join(struct.pack("<I", i) for i in range(first, first + cnt)) + b"".join(coms)
        return msg + b"".join(insts[first: first + cnt]) + b"".join(proofs[first: first + cnt])
    first = 0
    for cnt in segs:
        assert got[32 * first: 32 * (first + cnt)] == hashlib.shake_128(statement(first, cnt)).digest(32 * cnt), (first, cnt)
        first += cnt
    assert got[32 * k:] == hashlib.shake_128(statement(0, k)).digest(32 * k)  # batch_randomisers of the whole batch
    if segs == [7]:
        assert got[: 32 * k] == got[32 * k:]
