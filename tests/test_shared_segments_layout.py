"""Host side of the segmented run over a shared-table staging (include/avrf.h avrf_thin_batch_run_shared_segments,
avrf_pedersen_batch_run_shared_segments): avrf_*_shared_segments_layout against the same arithmetic in Python -- which of the two layouts
is chosen, the limits on the chosen L, the refusals -- and the declarations of the C ABI and its C++ mirror.  No GPU needed."""
import os
import random
import re
import subprocess

from conftest import ROOT
from shared_segments_helpers import py_layout

NEW_SYMBOLS = ("avrf_thin_batch_run_shared_segments", "avrf_pedersen_batch_run_shared_segments", "avrf_thin_batch_verify_shared_segments_wire",
               "avrf_pedersen_batch_verify_shared_segments_wire", "avrf_thin_shared_segments_layout", "avrf_pedersen_shared_segments_layout")
BAD_ARG = -2


def thin(segs, counts, T):
    from ark_vrf_amd import _native as nat
    return nat.thin_shared_segments_layout(segs, counts, T)


def ped(segs, T):
    from ark_vrf_amd import _native as nat
    return nat.pedersen_shared_segments_layout(sum(segs), segs, T)


def test_layout_matches_python_arithmetic():
    from ark_vrf_amd import _native as nat
    rng = random.Random(18)
    for _ in range(60):
        segs = [rng.choice([0, 1, 2, 5, 40, 300]) for _ in range(rng.randrange(1, 12))]
        counts = [rng.choice([0, 1, 1, 2, 3]) for _ in range(sum(segs))]
        T = rng.choice([1, 2, 3, 5, 40, 299, 300, 301, 700])
        assert thin(segs, counts, T) == py_layout(True, segs, counts, T), (segs, T)
        assert ped(segs, T) == py_layout(False, segs, counts, T), (segs, T)
        assert nat.Context.thin_shared_segments_layout(segs, counts, T) == py_layout(True, segs, counts, T)
    # no table: the plain segmented layout, mode 0
    assert thin([3, 0, 2], [1] * 5, 0) == nat.thin_segments_layout([3, 0, 2], [1] * 5) + (0,)
    assert ped([3, 5], 0) == nat.pedersen_segments_layout(8, [3, 5]) + (0,) == (27, 54, 44, 4, 0)
    # the shapes of include/avrf.h: padded lengths 1 029 / 1 282, 69 / 82, 3 076 / 4 097; Thin 256 x 256 over 1 027 rows stays expanded
    assert ped([256] * 256, 3) == (1029, 256 * 1029, 256 * 1029, 7, 1) and nat.pedersen_segments_layout(65536, [256] * 256)[0] == 1282
    # 4 096 x 16 would be 69 against 82 terms, but 4 096 segments at 4-bit windows are 4 096 * 65 virtual windows: over
    # AVRF_SEGMENTS_WINDOWS_MAX in EITHER layout, so both calls refuse it; 1 024 x 64 (261 against 322) is the finest of the measured shapes
    assert ped([16] * 4096, 3) == BAD_ARG and nat.pedersen_segments_layout(65536, [16] * 4096) == BAD_ARG
    assert py_layout(False, [16] * 4096, [], 3)[0] == 69 and 4096 * 65 > nat.SEGMENTS_WINDOWS_MAX
    assert ped([64] * 1024, 3) == (261, 1024 * 261, 1024 * 261, 5, 1) and nat.pedersen_segments_layout(65536, [64] * 1024)[0] == 322
    assert thin([1024] * 64, [1] * 65536, 1027) == (3076, 64 * 3076, 64 * 3076, 8, 1)
    assert thin([256] * 256, [1] * 65536, 1027) == (1025, 256 * 1025, 256 * 1025, 7, 0)  # 512 + 1 027 + 1 merged terms would be more


def test_mode_around_the_tie():
    """merged exactly when L_m < L_p: Thin T < max(items + pairs), Pedersen T < max(items); a tie goes to expanded"""
    # Thin, one pair per item: segments of 4 and 3 items, max(items + pairs) = 8
    one = [1] * 7
    assert thin([4, 3], one, 7) == (4 + 4 + 7 + 1, 32, 16 + 14, 4, 1)
    assert thin([4, 3], one, 8) == (17, 34, 17 + 13, 4, 0)                               # L_m = 17 = L_p: expanded
    assert thin([4, 3], one, 9) == (17, 34, 30, 4, 0)
    # Thin, mixed pair counts 0, 3, 1 | 2, 1: the first segment has 3 items + 4 pairs, the second 2 + 3
    mixed = [0, 3, 1, 2, 1]
    assert thin([3, 2], mixed, 6) == (7 + 6 + 1, 28, 14 + 12, 4, 1)
    assert thin([3, 2], mixed, 7) == (15, 30, 15 + 11, 4, 0)
    assert thin([3, 2], mixed, 8) == (15, 30, 26, 4, 0)
    # Pedersen: segments of 5 and 9 items
    assert ped([5, 9], 8) == (36 + 8 + 2, 92, 30 + 46, 4, 1)
    assert ped([5, 9], 9) == (47, 94, 27 + 47, 4, 0)                                     # L_m = 47 = L_p
    assert ped([5, 9], 10) == (47, 94, 74, 4, 0)


def test_empty_segments_and_wrong_counts():
    one = [1] * 12
    for segs in ([0, 5, 7], [5, 0, 7], [5, 7, 0], [0, 0, 12, 0], [0, 0]):
        n = sum(segs)
        assert thin(segs, one[:n], 3) == py_layout(True, segs, one[:n], 3), segs
        assert ped(segs, 3) == py_layout(False, segs, one[:n], 3), segs
    assert thin([0, 5, 7], one, 3) == (7 + 7 + 3 + 1, 54, 14 + 18, 4, 1)                # an empty segment has no terms, not T + 1
    assert ped([0, 0], 3) == (0, 0, 0, 0, 0) and thin([], [], 3) == (0, 0, 0, 0, 0)
    # counts that do not sum to n
    assert thin([5, 6], one, 3) == BAD_ARG and thin([5, 8], one, 3) == BAD_ARG and thin([], one, 3) == BAD_ARG
    from ark_vrf_amd import _native as nat
    assert nat.pedersen_shared_segments_layout(12, [5, 6], 3) == BAD_ARG
    assert nat.pedersen_shared_segments_layout(12, [5, 8], 3) == BAD_ARG
    assert nat.pedersen_shared_segments_layout(1, [], 3) == BAD_ARG


def test_limits_apply_to_the_chosen_length():
    from ark_vrf_amd import _native as nat
    # AVRF_SEGMENT_TERMS_MAX.  2 048 one-pair Thin items over 1 027 rows: 5 124 merged terms, where the plain layout's 8 193 is refused
    one = [1] * 4096
    assert nat.thin_segments_layout([2048], one[:2048]) == BAD_ARG and 2 * 2048 + 2 * 2048 + 1 > nat.SEGMENT_TERMS_MAX
    assert thin([2048], one[:2048], 1027) == (5124, 5124, 5124, 9, 1)
    assert thin([2048], one[:2048], 4094) == (8191, 8191, 8191, 9, 1)
    assert thin([2048], one[:2048], 4095) == BAD_ARG                                     # merged is chosen (8 192 < 8 193) and is over the limit
    assert thin([2048], one[:2048], 4096) == BAD_ARG                                     # a tie: expanded, 8 193
    assert thin([4096], one, 3) == BAD_ARG                                               # 8 196 merged
    assert ped([2046], 5) == (8191, 8191, 8191, 9, 1) and ped([2047], 5) == BAD_ARG      # 4 k + 7; the plain layout stops at 1 637 items
    assert nat.pedersen_segments_layout(1638, [1638]) == BAD_ARG
    # AVRF_SEGMENTS_PADDED_TERMS_MAX on n_seg * L_m: 1 019 segments of 256 items pad to 1 019 * 1 029 terms, 1 020 are over
    assert 1019 * 1029 <= nat.SEGMENTS_PADDED_TERMS_MAX < 1020 * 1029
    assert ped([256] * 1019, 3) == (1029, 1019 * 1029, 1019 * 1029, 7, 1)
    assert ped([256] * 1020, 3) == BAD_ARG
    assert nat.pedersen_segments_layout(256 * 1019, [256] * 1019) == BAD_ARG             # (the expanded layout of the accepted one is over it)
    # AVRF_SEGMENTS_WINDOWS_MAX: two-item segments over one row are 11 merged terms at 4-bit windows, 65 windows each
    assert ped([2] * 1008, 1) == (11, 11 * 1008, 11 * 1008, 4, 1)
    assert ped([2] * 1009, 1) == BAD_ARG and 1009 * 65 > nat.SEGMENTS_WINDOWS_MAX >= 1008 * 65


def test_abi_declares_the_entry_points_and_the_mirror_compiles(tmp_path):
    with open(os.path.join(ROOT, "include", "avrf.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "include", "avrf.hpp")) as f:
        hpp = f.read()
    from ark_vrf_amd import _native as nat
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, h), sym
        assert sym in hpp, sym
        assert hasattr(nat.lib(), sym), sym                                         # exported by the built library
    client = tmp_path / "client.cpp"
    client.write_text('#include "avrf.hpp"\n'
                      "std::vector<avrf::Status> f(const avrf::thin::BatchVerifier &t, const avrf::pedersen::SharedBatchVerifier &p, const std::vector<uint32_t> &s) {\n"
                      "  auto a = t.run_shared_segments(s), b = p.verify_segments(s);\n"
                      "  a.push_back((avrf::Status)(p.segments_layout(s)[4] + avrf::thin::shared_segments_layout(s, s, 3)[4]));\n"
                      "  a.insert(a.end(), b.begin(), b.end()); return a;\n"
                      "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(client)])
