"""Host side of the shared-table Thin batch from wire bytes (include/avrf.h avrf_thin_batch_stage_shared_wire): the C ABI's
declarations and exports, and the helper that turns an expanded wire batch into a table of compressed rows and indices.  No GPU needed."""
import os
import random
import re

import pytest

from conftest import ROOT

STAGE_ARGS = ["ctx", "n", "n_shared", "shared", "pk_index", "input_index", "outputs", "io_counts", "ads", "ad_lens", "proofs", "validate"]
DECLARED = {
    "avrf_thin_batch_stage_shared_wire": STAGE_ARGS,
    "avrf_thin_batch_verify_shared_wire": STAGE_ARGS,
    "avrf_pool_submit_shared_wire": ["pool"] + STAGE_ARGS[1:] + ["ticket"],
}


def test_symbols_declared_and_exported():
    from ark_vrf_amd import _native as nat
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avrf.h")).read(), flags=re.S)
    lib = nat.lib()
    for sym, want in DECLARED.items():
        m = re.search(rf"int\s+{sym}\s*\(([^)]*)\)", src)
        assert m, sym
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, sym
        assert hasattr(lib, sym), sym


@pytest.mark.parametrize("L", [32, 33])
def test_dedup_points_wire_round_trip(L):
    from ark_vrf_amd import _native as nat
    rng = random.Random(11 + L)
    keys = [rng.randbytes(L) for _ in range(5)]
    inputs = [rng.randbytes(L) for _ in range(3)] + [keys[2]]             # one point that is both a key and an input
    counts = [0, 1, 2, 3, 5, 1, 0, 2, 16, 17]
    pk_of = [2] + [rng.randrange(5) for _ in counts[1:]]
    in_of = [3] + [rng.randrange(4) for _ in range(sum(counts) - 1)]     # ... and is referred to as both
    outs = [rng.randbytes(L) for _ in range(sum(counts))]
    pks = b"".join(keys[i] for i in pk_of)
    ios = b"".join(inputs[i] + o for i, o in zip(in_of, outs))
    shared, pk_index, input_index, outputs = nat.dedup_points_wire(pks, ios, L)
    assert len(shared) % L == 0
    rows = [shared[L * r: L * r + L] for r in range(len(shared) // L)]
    assert len(rows) == len(set(rows)) == len(set(keys[i] for i in pk_of) | set(inputs[i] for i in in_of))
    assert len(pk_index) == len(counts) and len(input_index) == sum(counts)
    assert pk_index[0] == input_index[0]                                  # the key that is also an input is ONE row
    assert b"".join(rows[r] for r in pk_index) == pks
    assert b"".join(rows[r] + outs[k] for k, r in enumerate(input_index)) == ios
    assert outputs == b"".join(outs)
    # what it returns is what SharedWireBatch takes: n_shared counts L-byte rows
    b = nat.SharedWireBatch(len(counts), shared, pk_index, input_index, outputs, counts, b"", [0] * len(counts), bytes((L + 32) * len(counts)), L)
    assert b.n_shared == len(rows)
    # items without pairs, and nothing at all
    shared, pk_index, input_index, outputs = nat.dedup_points_wire(keys[0] + keys[1] + keys[0], b"", L)
    assert len(shared) == 2 * L and pk_index[0] == pk_index[2] != pk_index[1] and input_index == [] and outputs == b""
    assert nat.dedup_points_wire(b"", b"", L) == (b"", [], [], b"")
