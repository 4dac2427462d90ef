// proof_kind.h -- the proof kinds of the C ABI and every size the host derives from them, stated once.  Host-only, no HIP includes:
// capi_wire.hip (a pure composition of public entry points) reads the same table as capi.hip and pool.hip.
//   kind      x || y proof (ABI)                          wire proof (`serialize_compressed`, points of L bytes)
//   Thin      R(64) || s(32)                        96    R(L) || s(32)                          64 at L = 32   src/thin.rs:43-48
//   Pedersen  Yb(64) || R(64) || Ok(64) || s || sb  256   Yb(L) || R(L) || Ok(L) || s || sb     160             src/pedersen.rs:69-75
//   Tiny      c(16) || s(32)                        48    c(16) || s(32)                         48             src/tiny.rs:60-78
// The batch verifiers' weight transcript (src/thin.rs:274-279, src/pedersen.rs:361-367) absorbs one record per item,
// c(16) || 0(16) || responses, and yields `weight` bytes per item; Tiny has no batch verifier.
#pragma once
#include <stddef.h>

namespace avrf {
enum ProofKind : int { Thin = 1, Pedersen = 2, Tiny = 3 };   // the values are ABI: avrf_pool_create(kind), avrf_ctx::staged_kind
struct KindFacts {
  bool pk;            // the verifier takes a public key per item (Pedersen proofs carry the key commitment Yb instead)
  size_t points;      // proof points, in front of the scalars
  size_t tail;        // bytes of scalars behind the points
  size_t resp;        // the last `resp` of those: the responses the weight transcript absorbs (s | s, sb)
  size_t weight;      // weight bytes per item
  constexpr size_t xy_proof() const { return 64 * points + tail; }
  constexpr size_t wire_proof(size_t L) const { return L * points + tail; }
  constexpr size_t resp_at_xy() const { return xy_proof() - resp; }
  constexpr size_t resp_at_wire(size_t L) const { return wire_proof(L) - resp; }
  constexpr size_t record() const { return 32 + resp; }
};
constexpr KindFacts KIND_FACTS[4] = {{false, 0, 0, 0, 0}, {true, 1, 32, 32, 16}, {false, 3, 64, 64, 32}, {true, 0, 48, 0, 0}};
constexpr const KindFacts &kind_facts(int kind) { return KIND_FACTS[kind]; }
// terms of the batch verifier's MSM (src/thin.rs:282-317: 2 per item, 2 per I/O pair, G; src/pedersen.rs:369-418: 5 per item, G, B)
constexpr size_t n_terms(int kind, size_t n, size_t tot_io) { return kind == Thin ? 2 * n + 2 * tot_io + 1 : 5 * n + 2; }
// Thin over a table of n_shared points (include/avrf.h avrf_thin_batch_stage_shared): R per item, O per I/O pair, one term per row, G
constexpr size_t thin_shared_n_terms(size_t n, size_t tot_io, size_t n_shared) { return n + tot_io + n_shared + 1; }
// Pedersen over a table of n_shared inputs (avrf_pedersen_batch_stage_shared): O, Ok, Yb, R per item, one term per row, G, BLINDING_BASE
constexpr size_t ped_shared_n_terms(size_t n, size_t n_shared) { return 4 * n + n_shared + 2; }
constexpr size_t shared_n_terms(int kind, size_t n, size_t tot_io, size_t n_shared) { return kind == Thin ? thin_shared_n_terms(n, tot_io, n_shared) : ped_shared_n_terms(n, n_shared); }
// the references of a shared-table batch, one per contribution to a row's scalar: Thin every key and every input, Pedersen the inputs
constexpr size_t shared_n_contrib(int kind, size_t n, size_t tot_io) { return (KIND_FACTS[kind].pk ? n : 0) + tot_io; }
// what the prepare kernel leaves the terms kernel besides the challenges: Thin z_{j,i} (16 bytes per I/O pair), Pedersen the merged pair
// -- over a shared table (k_ped_prepare<S, true>) only its output half, and z_{j,i} (16 bytes per I/O pair) behind the n slots
constexpr size_t z_bytes(int kind, size_t n, size_t tot_io, bool shared = false) { return kind == Thin ? tot_io * 16 + 16 : n * 128 + (shared ? tot_io * 16 + 16 : 0); }

static_assert(kind_facts(Thin).xy_proof() == 96 && kind_facts(Pedersen).xy_proof() == 256 && kind_facts(Tiny).xy_proof() == 48, "x || y proofs");
static_assert(kind_facts(Thin).wire_proof(32) == 64 && kind_facts(Pedersen).wire_proof(32) == 160 && kind_facts(Tiny).wire_proof(32) == 48, "wire proofs");
static_assert(kind_facts(Thin).resp_at_xy() == 64 && kind_facts(Pedersen).resp_at_xy() == 192 && kind_facts(Thin).resp_at_wire(32) == 32 && kind_facts(Pedersen).resp_at_wire(32) == 96, "responses");
static_assert(kind_facts(Thin).record() == 64 && kind_facts(Pedersen).record() == 96, "transcript records");
}  // namespace avrf
