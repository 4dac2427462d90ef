"""Open batches, the parts that need no GPU: the exports of include/avrf.h (avrf_*_batch_open / _push / avrf_batch_flush /
avrf_batch_pushed) and the running weight transcript (ark_vrf_amd/csrc/host_weight_stream.h) -- a stand-alone program built with g++
from that header alone, run once plainly and once built with -fsanitize=address,undefined, whose values are compared with hashlib and
with avrf_batch_weight_seed."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ark_vrf_amd", "csrc")
SUITE_ID = {0: b"Bandersnatch-SHA512-ELL2-v1", 1: b"BabyJubJub-SHA512-TAI-v1"}
# SUITE_ID || 0x50 of suites 0 and 1 (28 and 25 bytes), and lengths that put the 64- and 96-byte records at the other phases of the
# 128-byte SHA-512 block, the 168-byte SHAKE128 rate and the 64-byte SHA-256 block: 1, 64, 111 and a whole block
PREFIXES = [SUITE_ID[0] + b"\x50", SUITE_ID[1] + b"\x50", b"\x50", bytes(range(64)), bytes(range(111)), bytes(range(128))]

NEW_SYMBOLS = ["avrf_thin_batch_open", "avrf_pedersen_batch_open", "avrf_thin_batch_push", "avrf_thin_batch_push_wire",
               "avrf_pedersen_batch_push", "avrf_pedersen_batch_push_wire", "avrf_batch_flush", "avrf_batch_pushed"]


def test_exports():
    """the eight calls are exported by libavrf.so and declared in include/avrf.h"""
    from ark_vrf_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "avrf.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(nat.lib(), name), name
        assert name + "(" in header, name
    # no context: every call refuses (and none dereferences it)
    L = nat.lib()
    z = C.c_size_t(0)
    assert L.avrf_thin_batch_open(None, z, z, z) == nat.ERR_BAD_ARG and L.avrf_pedersen_batch_open(None, z, z, z) == nat.ERR_BAD_ARG
    assert L.avrf_thin_batch_push(None, z, None, None, None, None, None, None) == nat.ERR_BAD_ARG
    assert L.avrf_pedersen_batch_push_wire(None, z, None, None, None, None, None, 1) == nat.ERR_BAD_ARG
    assert L.avrf_batch_flush(None) == nat.ERR_BAD_ARG
    L.avrf_batch_pushed.restype = C.c_size_t
    out = (C.c_size_t * 3)(7, 7, 7)
    assert L.avrf_batch_pushed(None, out) == 0 and list(out) == [0, 0, 0]


def records(n, recsz):
    """tests/cpp/weight_stream.cpp make_records"""
    out = bytearray(n * recsz)
    for j in range(n):
        for i in range(recsz):
            if i < 16 or i >= 32:
                out[j * recsz + i] = (((j * 2654435761) & 0xffffffff) + i * 40503 + 12345 & 0xffffffff) >> 7 & 0xff
    return bytes(out)


def expected(hash_id, msg, out_len):
    if hash_id == 0:
        return hashlib.sha512(msg).digest()
    if hash_id == 1:
        return hashlib.shake_128(msg).digest(out_len)
    seed = hashlib.sha256(msg).digest()          # DigestXof: block_i = H(seed || LE64(i))
    out, i = b"", 0
    while len(out) < out_len:
        out += hashlib.sha256(seed + i.to_bytes(8, "little")).digest()
        i += 1
    return out[:out_len]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("weight_stream")
    src = os.path.join(ROOT, "tests", "cpp", "weight_stream.cpp")
    plain, san = str(d / "weight_stream"), str(d / "weight_stream_san")
    base = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src]
    subprocess.check_call(base + ["-O2", "-o", plain])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san])
    return plain, san


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
def test_weight_stream_chunkings(programs, which):
    """every chunking ends where the whole message ends (checked by the program itself, exit status), a clone finalised mid-way leaves
    the original going on to the right end, and the end values are hashlib's -- and avrf_batch_weight_seed's where that call applies"""
    from ark_vrf_amd import _native as nat
    r = subprocess.run([programs[which]] + [p.hex() for p in PREFIXES], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert len(lines) == 3 * 2 * 4 * len(PREFIXES)
    by_len = {len(p): p for p in PREFIXES}
    seen = set()
    for h, recsz, n, plen, end, mid in lines:
        h, recsz, n, plen = int(h), int(recsz), int(n), int(plen)
        seen.add((h, recsz, n, plen))
        prefix, rec = by_len[plen], records(n, recsz)
        per = 16 if recsz == 64 else 32
        for count, got in ((n, end), (n // 2, mid)):
            want = expected(h, prefix + rec[: count * recsz], count * per)
            assert (bytes.fromhex(got) if got != "-" else b"") == want, (h, recsz, n, plen, count)
        if h == 0 and prefix[:-1] in SUITE_ID.values():            # the library's own whole-batch transcript
            suite = [k for k, v in SUITE_ID.items() if v == prefix[:-1]][0]
            c16 = b"".join(rec[recsz * j: recsz * j + 16] for j in range(n))
            resp = b"".join(rec[recsz * j + 32: recsz * (j + 1)] for j in range(n))
            seed = (C.c_uint8 * 64)()
            assert nat.lib().avrf_batch_weight_seed(suite, 1 if recsz == 96 else 0, C.c_size_t(n), nat._u8(c16), nat._u8(resp), seed) == 0
            assert bytes(seed).hex() == end
    assert seen == {(h, r, n, len(p)) for h in range(3) for r in (64, 96) for n in (1, 2, 129, 600) for p in PREFIXES}
