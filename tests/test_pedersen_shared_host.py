"""Host side of the Pedersen batch verifier over a table of shared inputs (include/avrf.h avrf_pedersen_batch_stage_shared): the term
count 4 n + T + 2, the dedup helpers of the Python layer, and the C ABI's declarations.  No GPU needed."""
import os
import random
import re

from conftest import ROOT

STAGE_ARGS = "n, n_shared, shared_xy, input_index, outputs_xy, io_counts, ads, ad_lens, proofs"
WIRE_ARGS = "n, n_shared, shared, input_index, outputs, io_counts, ads, ad_lens, proofs, validate"
# symbol -> the argument names in order (the handle first)
DECLARED = {
    "avrf_pedersen_batch_stage_shared": "ctx, " + STAGE_ARGS,
    "avrf_pedersen_shared_n_terms": "n, n_shared",
    "avrf_pedersen_batch_stage_shared_wire": "ctx, " + WIRE_ARGS,
    "avrf_pedersen_batch_verify_shared_wire": "ctx, " + WIRE_ARGS,
    "avrf_pool_submit_pedersen_shared": "pool, " + STAGE_ARGS + ", ticket",
    "avrf_pool_submit_pedersen_shared_wire": "pool, " + WIRE_ARGS + ", ticket",
}


def test_n_terms_formula():
    from ark_vrf_amd import _native as nat
    assert nat.pedersen_shared_n_terms(0, 0) == 2
    assert nat.pedersen_shared_n_terms(65536, 3) == 262149 < 5 * 65536 + 2 == 327682
    assert nat.pedersen_shared_n_terms(1, 0) == 6 and nat.pedersen_shared_n_terms(0, 7) == 9
    rng = random.Random(4)
    for _ in range(200):
        n, t = rng.randrange(1 << 24), rng.randrange(1 << 20)
        assert nat.pedersen_shared_n_terms(n, t) == 4 * n + t + 2


def rand_point(rng, nbytes):
    return bytes(rng.randrange(256) for _ in range(nbytes))


def test_dedup_round_trips_an_expanded_batch():
    from ark_vrf_amd import _native as nat
    rng = random.Random(9)
    for L, dedup in [(64, nat.dedup_inputs), (32, lambda ios: nat.dedup_inputs_wire(ios, 32)), (33, lambda ios: nat.dedup_inputs_wire(ios, 33))]:
        inputs = [rand_point(rng, L) for _ in range(3)]
        for counts in ([1] * 50, [0, 1, 2, 3, 16, 17, 1, 0], [0, 0, 0], [], [5]):
            pairs = [(rng.choice(inputs), rand_point(rng, L)) for _ in range(sum(counts))]
            ios = b"".join(i + o for i, o in pairs)
            shared, input_index, outputs = dedup(ios)
            rows = [shared[L * r: L * r + L] for r in range(len(shared) // L)]
            assert len(rows) == len(set(rows)) == len(set(i for i, _ in pairs)) <= 3      # distinct rows, every one referenced
            assert len(input_index) == sum(counts) and len(outputs) == L * sum(counts)
            assert b"".join(rows[r] + outputs[L * k: L * k + L] for k, r in enumerate(input_index)) == ios
            if not pairs:
                assert (shared, input_index, outputs) == (b"", [], b"")                   # items without pairs: n_shared = 0
            # the batch classes take the helper's output as it is
            n = len(counts)
            if L == 64:
                b = nat.PedersenSharedBatch(n, shared, input_index, outputs, counts, b"", [0] * n, bytes(256 * n))
            else:
                b = nat.PedersenSharedWireBatch(n, shared, input_index, outputs, counts, b"", [0] * n, bytes((3 * L + 64) * n), L)
            assert b.n_shared == len(rows) and len(b.args()) == 9


def test_abi_declares_and_documents_the_entry_points():
    with open(os.path.join(ROOT, "include", "avrf.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "include", "avrf.hpp")) as f:
        hpp = f.read()
    for sym, names in DECLARED.items():
        m = re.search(r"\b(int|size_t) %s\(([^;]*)\);" % sym, h)
        assert m, sym
        got = [re.split(r"[\s\*]+", a.strip())[-1] for a in m.group(2).split(",")]
        assert got == names.split(", "), (sym, got)                                      # the argument order of the issue
        assert sym in hpp, sym
    assert "4 n + n_shared + 2" in h and "src/pedersen.rs:387-418" in h
    from ark_vrf_amd import _native as nat
    for sym in DECLARED:
        assert hasattr(nat.lib(), sym), sym                                              # exported by the built library
    for name in ("PedersenSharedBatch", "PedersenSharedWireBatch", "PinnedPedersenSharedBatch", "PinnedPedersenSharedWireBatch", "dedup_inputs",
                 "dedup_inputs_wire", "pedersen_shared_n_terms"):
        assert hasattr(nat, name), name
    for name in ("pedersen_batch_stage_shared", "pedersen_batch_stage_shared_wire", "pedersen_batch_verify_shared_wire"):
        assert hasattr(nat.Context, name), name
    assert hasattr(nat.Pool, "submit_pedersen_shared") and hasattr(nat.Pool, "submit_pedersen_shared_wire")
