"""Host side of the Pedersen batch verifier over segments (include/avrf.h avrf_pedersen_batch_run_segments): the layout arithmetic of
avrf_pedersen_segments_layout against the same arithmetic in Python (src/pedersen.rs:383-418: five terms per item, G and B per
segment), its limits, and the C ABI's declarations.  No GPU needed."""
import os
import random
import re

from conftest import ROOT

NEW_SYMBOLS = ("avrf_pedersen_batch_run_segments", "avrf_pedersen_batch_verify_segments", "avrf_pedersen_batch_verify_segments_wire",
               "avrf_pedersen_segments_layout", "avrf_pedersen_segment_terms")
BAD_ARG = -2


def window_bits(L):
    """what the engine's plan gives an L-term MSM below 65 536 terms: floor(log2 L) - 3, at least 4"""
    return max(4, L.bit_length() - 1 - 3)


def layout(seg_items):
    """n_seg pedersen::BatchVerifiers over consecutive items: 5 k + 2 terms for k items (src/pedersen.rs:383-418), none for an empty
    segment (:343-345)"""
    counts = [5 * k + 2 if k else 0 for k in seg_items]
    L = max(counts, default=0)
    return (L, len(seg_items) * L, sum(counts), window_bits(L) if L else 0)


def test_layout_matches_python_arithmetic():
    from ark_vrf_amd import _native as nat
    rng = random.Random(12)
    cases = [[1, 2, 3, 5, 7, 16, 33, 64, 130], [4] * 8, [3, 0, 2], [0, 0], [], [256] * 256, [64] * 1024, [1024] * 64, [1], [11, 7, 243],
             [0, 261, 0], [1, 2, 3, 5, 0, 7, 16, 33, 64, 130]]
    for _ in range(30):
        cases.append([rng.choice([0, 1, 2, 5, 40, 300]) for _ in range(rng.randrange(1, 12))])
    for segs in cases:
        assert nat.pedersen_segments_layout(sum(segs), segs) == layout(segs), segs
        assert nat.Context.pedersen_segments_layout(sum(segs), segs) == layout(segs)
    assert nat.pedersen_segments_layout(261, [1, 2, 3, 5, 7, 16, 33, 64, 130])[0] == 652
    # the measured shape: 256 segments of 256 items are 1 282 terms each at 7-bit windows
    assert nat.pedersen_segments_layout(65536, [256] * 256) == (1282, 256 * 1282, 256 * 1282, 7)
    assert nat.pedersen_segments_layout(65536, [64] * 1024) == (322, 1024 * 322, 1024 * 322, 5)
    assert nat.pedersen_segments_layout(65536, [1024] * 64) == (5122, 64 * 5122, 64 * 5122, 9)


def test_layout_limits_and_refusals():
    from ark_vrf_amd import _native as nat
    # the longest segment: 5 k + 2 <= SEGMENT_TERMS_MAX = 8 191 gives k = 1 637 (8 187 terms); 1 638 items are 8 192
    assert 5 * 1637 + 2 == 8187 <= nat.SEGMENT_TERMS_MAX < 5 * 1638 + 2
    assert nat.pedersen_segments_layout(1637, [1637]) == (8187, 8187, 8187, 9)
    assert nat.pedersen_segments_layout(1638, [1638]) == BAD_ARG
    # virtual windows of the chain: n_seg * ceil(257 / c) <= SEGMENTS_WINDOWS_MAX (c = 4 for one-item segments: 65 windows each)
    assert nat.pedersen_segments_layout(1008, [1] * 1008) == (7, 7 * 1008, 7 * 1008, 4)
    assert nat.pedersen_segments_layout(1009, [1] * 1009) == BAD_ARG and 1009 * 65 > nat.SEGMENTS_WINDOWS_MAX >= 1008 * 65
    # the padded layout: n_seg * L <= SEGMENTS_PADDED_TERMS_MAX -- one long segment pads every other one
    assert 129 * 8187 > nat.SEGMENTS_PADDED_TERMS_MAX >= 128 * 8187
    assert nat.pedersen_segments_layout(127 + 1637, [1] * 127 + [1637]) == (8187, 128 * 8187, 127 * 7 + 8187, 9)
    assert nat.pedersen_segments_layout(128 + 1637, [1] * 128 + [1637]) == BAD_ARG
    assert nat.pedersen_segments_layout(128 * 1637, [1637] * 128) == (8187, 128 * 8187, 128 * 8187, 9)
    assert nat.pedersen_segments_layout(129 * 1637, [1637] * 129) == BAD_ARG
    # counts that do not sum to n
    assert nat.pedersen_segments_layout(8, [3, 4]) == BAD_ARG
    assert nat.pedersen_segments_layout(8, [3, 6]) == BAD_ARG
    assert nat.pedersen_segments_layout(1, []) == BAD_ARG
    assert nat.pedersen_segments_layout(8, [3, 5]) == (27, 54, 44, 4)


def test_abi_declares_and_documents_the_entry_points():
    with open(os.path.join(ROOT, "include", "avrf.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "include", "avrf.hpp")) as f:
        hpp = f.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t) %s\(" % sym, h), sym
        assert sym in hpp, sym
    assert h.count("src/pedersen.rs:303-426") >= 3
    from ark_vrf_amd import _native as nat
    for sym in NEW_SYMBOLS:
        assert hasattr(nat.lib(), sym), sym                                         # exported by the built library
