"""The pool's segmented jobs without a device: the C ABI declares and exports them, and the Python wrapper has the methods."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["avrf_pool_submit_segments", "avrf_pool_submit_segments_wire", "avrf_pool_wait_segments"]


def test_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "avrf.h")).read()
    from ark_vrf_amd import _native as nat
    lib = nat.lib()
    for sym in SYMBOLS + ["avrf_msm_te_segments_chain"]:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
    # the segments follow the arguments of the plain submission, the ticket comes last; statuses come with their capacity
    decl = lambda sym: re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\(([^;]*)\);" % sym, header).group(1))
    assert decl("avrf_pool_submit_segments").endswith("size_t n_seg, const uint32_t *seg_items, uint64_t *ticket")
    assert decl("avrf_pool_submit_segments_wire").endswith("int validate, size_t n_seg, const uint32_t *seg_items, uint64_t *ticket")
    assert decl("avrf_pool_wait_segments") == "avrf_pool *pool, uint64_t ticket, int *status, int32_t *status_out, size_t cap"


def test_python_pool_has_the_methods():
    from ark_vrf_amd import _native as nat
    for name in ("submit_segments", "submit_segments_wire", "wait_segments"):
        assert callable(getattr(nat.Pool, name, None)), name
    assert callable(getattr(nat.Context, "msm_segments_chain", None))
