"""Host side of the Thin batch verifier over segments (include/avrf.h avrf_thin_batch_run_segments): the layout arithmetic of
avrf_thin_segments_layout against the same arithmetic in Python, its limits, and the C ABI's declarations.  No GPU needed."""
import os
import random
import re

from conftest import ROOT

NEW_SYMBOLS = ("avrf_thin_batch_run_segments", "avrf_thin_batch_verify_segments", "avrf_thin_batch_verify_segments_wire",
               "avrf_thin_segments_layout", "avrf_thin_segment_terms", "avrf_msm_te_segments")
BAD_ARG = -2


def window_bits(L):
    """what the engine's plan gives an L-term MSM below 65 536 terms: floor(log2 L) - 3, at least 4"""
    return max(4, L.bit_length() - 1 - 3)


def layout(seg_items, io_counts):
    """n_seg thin::BatchVerifiers over consecutive items: 2 terms per item, 2 per I/O pair, the generator (src/thin.rs:282-317);
    none for an empty segment (:262-264)"""
    at, counts = 0, []
    for k in seg_items:
        counts.append(2 * k + 2 * sum(io_counts[at: at + k]) + 1 if k else 0)
        at += k
    assert at == len(io_counts)
    L = max(counts, default=0)
    return (L, len(seg_items) * L, sum(counts), window_bits(L) if L else 0)


def test_layout_matches_python_arithmetic():
    from ark_vrf_amd import _native as nat
    rng = random.Random(11)
    cases = [([1, 2, 3, 5, 7, 16, 33, 64, 130], None), ([4] * 8, [1] * 32), ([3, 0, 2], [0, 1, 3, 3, 0]), ([0, 0], []), ([], []),
             ([256] * 256, [1] * 65536), ([64] * 1024, [1] * 65536), ([1024] * 64, [1] * 65536), ([1], [0]), ([1], [3])]
    for _ in range(30):
        segs = [rng.choice([0, 1, 2, 5, 40, 300]) for _ in range(rng.randrange(1, 12))]
        cases.append((segs, None))
    for segs, io in cases:
        if io is None:
            io = [rng.choice([0, 1, 3]) for _ in range(sum(segs))]                 # mixed pair counts
        assert nat.thin_segments_layout(segs, io) == layout(segs, io), (segs, io)
        assert nat.Context.thin_segments_layout(segs, io) == layout(segs, io)
    # the shapes of the issue's cost estimate: 256 segments of 256 one-pair items are 1 025 terms each at 7-bit windows
    assert nat.thin_segments_layout([256] * 256, [1] * 65536) == (1025, 256 * 1025, 256 * 1025, 7)
    assert nat.thin_segments_layout([1] * 8, [0] * 8)[3] == 4 and nat.thin_segments_layout([1024] * 8, [1] * 8192)[3] == 9


def test_layout_limits_and_refusals():
    from ark_vrf_amd import _native as nat
    # a segment of exactly SEGMENT_TERMS_MAX terms: 2 k + 2 pairs + 1 = 8 191 with k = 2 047 one-pair items and one pair more
    io = [1] * 2047
    io[5] = 2
    assert 2 * 2047 + 2 * sum(io) + 1 == nat.SEGMENT_TERMS_MAX
    assert nat.thin_segments_layout([2047], io) == (8191, 8191, 8191, 9)
    io[6] = 2                                                                       # two terms more: over the limit
    assert nat.thin_segments_layout([2047], io) == BAD_ARG
    assert nat.thin_segments_layout([2048], [1] * 2048) == BAD_ARG                  # 8 193 terms
    # the padded layout: n_seg * L <= SEGMENTS_PADDED_TERMS_MAX -- one long segment pads every other one
    assert 129 * 8189 > nat.SEGMENTS_PADDED_TERMS_MAX >= 128 * 8189
    assert nat.thin_segments_layout([1] * 127 + [2047], [1] * (127 + 2047)) == (8189, 128 * 8189, 127 * 5 + 8189, 9)
    assert nat.thin_segments_layout([1] * 128 + [2047], [1] * (128 + 2047)) == BAD_ARG
    assert nat.thin_segments_layout([2047] * 128, [1] * (128 * 2047)) == (8189, 128 * 8189, 128 * 8189, 9)
    assert nat.thin_segments_layout([2047] * 129, [1] * (129 * 2047)) == BAD_ARG
    # virtual windows of the chain: n_seg * ceil(257 / c) <= SEGMENTS_WINDOWS_MAX (c = 4 for one-item segments: 65 windows each)
    assert nat.thin_segments_layout([1] * 1008, [1] * 1008) == (5, 5040, 5040, 4)
    assert nat.thin_segments_layout([1] * 1009, [1] * 1009) == BAD_ARG and 1009 * 65 > nat.SEGMENTS_WINDOWS_MAX >= 1008 * 65
    # counts that do not sum to n
    assert nat.thin_segments_layout([3, 4], [1] * 8) == BAD_ARG
    assert nat.thin_segments_layout([3, 6], [1] * 8) == BAD_ARG
    assert nat.thin_segments_layout([], [1]) == BAD_ARG
    assert nat.thin_segments_layout([3, 5], [1] * 8) == (21, 42, 34, 4)


def test_abi_declares_and_documents_the_entry_points():
    with open(os.path.join(ROOT, "include", "avrf.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "include", "avrf.hpp")) as f:
        hpp = f.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t) %s\(" % sym, h), sym
    assert h.count("src/thin.rs:188-326") >= 5
    for name, value in (("AVRF_SEGMENT_TERMS_MAX", "8191"), ("AVRF_SEGMENTS_PADDED_TERMS_MAX", "1 << 20"), ("AVRF_SEGMENTS_WINDOWS_MAX", "65535")):
        assert re.search(r"%s = %s\b" % (name, re.escape(value)), h), name
    for sym in ("avrf_thin_batch_run_segments", "avrf_thin_batch_verify_segments", "avrf_thin_segment_terms", "avrf_msm_te_segments", "avrf_thin_segments_layout"):
        assert sym in hpp, sym
    from ark_vrf_amd import _native as nat
    for sym in NEW_SYMBOLS:
        assert hasattr(nat.lib(), sym), sym                                         # exported by the built library
