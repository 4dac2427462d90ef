"""Host side of the Thin batch verifier over a table of shared points (include/avrf.h avrf_thin_batch_stage_shared): the term
count, the helper that turns an expanded batch into a table and indices, and the C ABI's declarations.  No GPU needed."""
import os
import random
import re

from conftest import ROOT

NEW_SYMBOLS = ("avrf_thin_batch_stage_shared", "avrf_pool_submit_shared", "avrf_thin_shared_n_terms")


def test_n_terms_formula():
    from ark_vrf_amd import _native as nat
    rng = random.Random(5)
    cases = [(0, 0, 0), (0, 0, 7), (1, 0, 1), (1, 1, 1), (5, 0, 3), (65536, 65536, 1027), (65536, 65536, 131072), (3, 40, 0)]
    cases += [(rng.randrange(1 << 20), rng.randrange(1 << 20), rng.randrange(1 << 20)) for _ in range(50)]
    for n, tot_io, t in cases:
        assert nat.thin_shared_n_terms(n, tot_io, t) == n + tot_io + t + 1, (n, tot_io, t)
    # one pair per item and a small table: half the plain batch's 2 n + 2 tot_io + 1 terms, plus the table
    assert nat.thin_shared_n_terms(65536, 65536, 1027) == (2 * 65536 + 2 * 65536 + 1 - 1) // 2 + 1027 + 1


def test_dedup_points_round_trip():
    from ark_vrf_amd import _native as nat
    rng = random.Random(11)
    keys = [rng.randbytes(64) for _ in range(5)]
    inputs = [rng.randbytes(64) for _ in range(3)] + [keys[2]]            # one point that is both a key and an input
    counts = [0, 1, 2, 3, 5, 1, 0, 2, 16, 17]
    pk_of = [rng.randrange(5) for _ in counts]
    in_of = [rng.randrange(4) for _ in range(sum(counts))]
    outs = [rng.randbytes(64) for _ in range(sum(counts))]
    pks_xy = b"".join(keys[i] for i in pk_of)
    ios_xy = b"".join(inputs[i] + o for i, o in zip(in_of, outs))
    shared, pk_index, input_index, outputs = nat.dedup_points(pks_xy, ios_xy)
    rows = [shared[64 * r: 64 * r + 64] for r in range(len(shared) // 64)]
    assert len(rows) == len(set(rows)) == len(set(keys[i] for i in pk_of) | set(inputs[i] for i in in_of))
    assert len(pk_index) == len(counts) and len(input_index) == sum(counts)
    assert b"".join(rows[r] for r in pk_index) == pks_xy
    assert b"".join(rows[r] + outs[k] for k, r in enumerate(input_index)) == ios_xy
    assert outputs == b"".join(outs)
    # items without pairs, and nothing at all
    shared, pk_index, input_index, outputs = nat.dedup_points(keys[0] + keys[1] + keys[0], b"")
    assert len(shared) == 128 and pk_index[0] == pk_index[2] != pk_index[1] and input_index == [] and outputs == b""
    assert nat.dedup_points(b"", b"") == (b"", [], [], b"")


def test_new_symbols_declared_and_exported():
    from ark_vrf_amd import _native as nat
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avrf.h")).read(), flags=re.S)
    lib = nat.lib()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", src), s
        assert hasattr(lib, s), s
    # the declared argument lists: table and indices in front of the outputs, the rest as avrf_thin_batch_stage
    m = re.search(r"int\s+avrf_thin_batch_stage_shared\s*\(([^)]*)\)", src)
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["ctx", "n", "n_shared", "shared_xy", "pk_index", "input_index", "outputs_xy", "io_counts", "ads", "ad_lens", "proofs"]
    m = re.search(r"int\s+avrf_pool_submit_shared\s*\(([^)]*)\)", src)
    names = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert names == ["pool", "n", "n_shared", "shared_xy", "pk_index", "input_index", "outputs_xy", "io_counts", "ads", "ad_lens", "proofs", "ticket"]
