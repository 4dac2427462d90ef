// capi_internal.h -- what the translation units of libavrf.so share about a context (capi.hip, pool.hip): buffers, the
// execution lane (stream + MSM workspace), the record of the run in flight and the ONE family of phases that walks a staged batch
// through BatchVerifier::verify (src/thin.rs:257-325, src/pedersen.rs:341-426), as a whole batch or as n_seg groups of items.
// Not part of the C ABI (include/avrf.h).
#pragma once
#include "../../include/avrf.h"
#include "host_te.h"
#include "msm.h"
#include "proof_kind.h"
#include "host_weight_stream.h"
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <deque>
#include <new>
#include <vector>

#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "avrf: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return AVRF_ERR_NO_DEVICE; } } while (0)

namespace avrf {

// Staging buffers of a context: msm.h's owned storage under another size rule -- rounded up, so that batches of slowly growing
// size do not reallocate -- and with an error code instead of a throw, for HIP_TRY.  Freed with whatever holds them.
template <bool PINNED> struct StageBuf : OwnedMem<PINNED> {
  hipError_t ensure(size_t bytes) {
    if (bytes <= this->cap && this->p) return hipSuccess;
    return this->reset(PINNED ? bytes + 256 : bytes + bytes / 8 + 256);
  }
};
using DevBuf = StageBuf<false>;
using PinBuf = StageBuf<true>;

template <class F> int guarded(F f) {
  try { return f(); }
  catch (const avrf::HipFailure &e) { fprintf(stderr, "avrf: HIP error %s at %s:%d\n", hipGetErrorString(e.err), e.file, e.line); return AVRF_ERR_NO_DEVICE; }
  catch (const std::bad_alloc &) { return AVRF_ERR_NO_DEVICE; }
}

// An execution lane: the stream an MSM chain runs on, its workspace and the term arrays the chain reads.  A context owns one;
// the slots of a pool (pool.hip) borrow the pool's lanes for the MSM phase of their batches, so that many staged batches can
// wait for their weight transcript without each holding a stream and ~150 MB of workspace.  One chain in flight per lane.
// (the stream is a base so that it outlives every member: workspace and term arrays are freed before the stream they ran on goes)
struct LaneStream {
  hipStream_t stream = nullptr;
  LaneStream() = default;
  LaneStream(const LaneStream &) = delete;
  LaneStream &operator=(const LaneStream &) = delete;
  ~LaneStream() { if (stream) (void)hipStreamDestroy(stream); }
};
struct Lane : LaneStream {
  int queued = 0;                 // chains enqueued and not yet collected (pool.hip)
  MsmWorkspace ws;
  DevBuf d_scalars, d_pre, d_gpart;
  DevBuf d_shared;                // a shared-table batch: the row scalars' contributions and partial sums of the chain being built (thin_shared.h)
  // a segmented run (run_launch below): the terms kernel's per-item scratch (Thin w s z0, n x 32 bytes; Pedersen u s and u sb, n x 64),
  // the n_seg + 1 item offsets and the n_seg weight seeds of the chain being built
  DevBuf d_seg_wsz, d_seg_off, d_seg_seeds;
};

// The shape of a run of the staged batch: the whole batch under one verdict, or (segmented) n_seg groups of consecutive items with a
// verdict each (thin_seg.h): group v is the items [off[v], off[v + 1]) and has L of the n_seg L = `padded` term slots.  merged: the
// merged layout of a shared-table staging (thin_shared.h "Segments"), row0[v] the term of group v's row 0.
struct RunShape { bool segmented = false, merged = false; size_t n_seg = 0, L = 0, padded = 0; std::vector<uint32_t> off, row0; };
enum class RunPhase { Idle, Begun, Launched };
// Everything about the run in flight (run_begin .. run_end below); the phase is written by those functions and by run_close alone
struct BatchRun {
  RunPhase phase = RunPhase::Idle;
  RunShape shape;
  std::vector<int32_t> item_status;   // a segmented run's attribution pass: a status per item (empty unless the batch's flag word was set)
  uint8_t digest[64] = {0};           // a whole-batch run: the digest of its weight transcript (counter-mode suites)
  bool unit_weights = false;          // every item's weight is 1 (avrf_thin_verify runs ONE item as its own equation through the MSM path)
  double begin_us = 0, msm_us = 0;    // avrf_last_timing: what enqueueing the prepare step took, and the chain
  // a segmented run: page-locked, so that the copies up never wait for the lane, the item offsets (n_seg + 1 words, padded to 64 bytes),
  // the n_seg weight seeds and, for the merged layout, the n_seg terms row0; and the groups' transcript messages, prefix || records each
  PinBuf h_up; std::vector<uint8_t> h_msg;
};
}  // namespace avrf

struct avrf_ctx {
  int suite = 0, device = 0;
  hipStream_t stream = nullptr;   // where the next piece of work is enqueued: the own lane's stream, or what a pool points it at
  avrf::Lane own; avrf::Lane *L = &own;
  avrf::MsmChain *pend = nullptr;   // pool slots: the record of the slot's MSM chain (several chains queue on one lane); else the lane's own
  avrf::MsmChain &chain() const { return pend ? *pend : L->ws.own; }
  bool lane_owner = true;         // false: a pool slot -- no stream or workspace of its own (L and stream are set by the pool)
  // staged batch
  int validate = 0;               // avrf_ctx_set_validation: 0 unchecked (typed-point callers), 1 on-curve, 2 + subgroup
  bool wire_pending = false;              // staged from wire bytes without waiting: run_collect reads the decode flag (h_flags[2])
  uint64_t stage_gen = 0, chal_gen = 0;   // challenges of *_batch_challenges belong to staging generation chal_gen
  int staged_kind = 0;            // 0 none, else the ProofKind staged (proof_kind.h)
  size_t n = 0, tot_io = 0, n_terms = 0;
  avrf::DevBuf d_pks, d_ios, d_io_off, d_ads, d_ad_off, d_proofs, d_sks;
  // a Thin or Pedersen batch staged over a table of shared points (avrf_thin_batch_stage_shared, avrf_pedersen_batch_stage_shared;
  // thin_shared.h): n_shared rows, 0 for a plain staging; n_contrib references (proof_kind.h shared_n_contrib).
  // d_pks / d_ios hold the gathered rows, so that the prepare kernel runs as on a plain batch; the terms come from the table and the plan.
  size_t n_shared = 0, n_contrib = 0;
  avrf::DevBuf d_table, d_table_idx, d_table_outs, d_table_rows, d_table_plan;
  std::vector<uint8_t> h_resp;    // host copy of the response scalars (s [, sb]) for the weight transcript (sponge transcripts only)
  avrf::DevBuf d_rec; avrf::PinBuf h_msg;     // counter-mode transcripts: the records written by the prepare kernel, and prefix || records on the host
  size_t h_msg_len = 0;
  std::vector<uint8_t> h_weights; avrf::DevBuf d_weights;   // sponge transcripts: the squeezed weight stream of the staged batch
  avrf::DevBuf d_c, d_z, d_flags, d_misc, d_out, d_status;
  avrf::DevBuf d_tabs;                               // per-item window tables of the independent prove / verify kernels
  avrf::DevBuf d_fixed; bool fixed_ready = false;   // fixed-base tables of G and BLINDING_BASE (provers, scalar_mul_base), built on first use
  avrf::PinBuf h_c, h_flags, h_io;
  // The run in flight, and what the last segmented run of the staged batch left for avrf_*_segment_terms: terms of its own, n_seg * L of
  // them in d_seg_scalars / d_seg_pre, so that the plain run's terms stay what they were, described by last_seg.shape while last_seg.gen
  // == stage_gen.  (A pool slot has neither: its segmented terms go to the arrays of the lane it borrows, run_launch.)
  // d_seg_plan: the per-run plan of a run in the merged layout (shared_seg_plan).
  avrf::BatchRun run;
  struct { avrf::RunShape shape; uint64_t gen = 0; } last_seg;
  avrf::DevBuf d_seg_scalars, d_seg_pre, d_seg_plan;
  // An OPEN batch (include/avrf.h avrf_*_batch_open / _push / _flush; BatchVerifier::new / push, src/thin.rs:199-243): staged_kind == kind
  // and gen == stage_gen while it is open, so whatever stages on the context, or drops what is staged, closes it.  n / tot_io / n_terms
  // above are its totals so far; the staged buffers hold `cap_*` and grow with their used prefix kept (capi.hip open_grow).  Each push
  // leaves a chunk: its item range and an event behind the copy back of its records (sponge / SHA-256 suites: its challenges).  `ws` has
  // absorbed the records of items [0, absorbed); a run finalises a clone of it.  `arena`: the page-locked copies of the pushed chunks,
  // in blocks that never move while copies up from them are in flight.  io_off stays in h_io; ad_off has a buffer of its own here
  // (stage_open keeps it behind io_off at n + 1, which an append would have to move).
  struct OpenBatch {
    struct Chunk { size_t n0 = 0, n = 0; avrf::DevEvent done; };
    int kind = 0; uint64_t gen = 0;
    size_t ad_bytes = 0, cap_items = 0, cap_pairs = 0, cap_ad = 0, absorbed = 0;
    std::deque<Chunk> chunks;                 // pushed and not yet absorbed, oldest first
    avrf::WeightStream ws;
    avrf::PinBuf h_ad_off;
    std::vector<avrf::PinBuf> arena; size_t arena_used = 0;   // bytes used of arena.back()
  } open;
  double timing[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // The order a context goes in: its device made current and its own stream drained; then the members, last first -- the staging
  // buffers, then `own`: workspace and term arrays, the stream last.  (A pool slot's context has no stream or workspace of its own; the
  // pool detaches it from the lane it borrowed before it dies, pool.hip ~Slot.)
  ~avrf_ctx() { (void)hipSetDevice(device); if (own.stream) (void)hipStreamSynchronize(own.stream); }
};

namespace avrf {
struct WeightJob;
// Where a batch comes from: the caller's host arrays, named for what they hold.  The x || y flavours read pks / ios / proofs as
// affine coordinates; `wire` ones as serialize_compressed bytes, decoded on the device (validate: + not the identity, + subgroup).
// n_shared != 0: over a table of shared points (include/avrf.h) -- `table` rows, the items' keys (Thin) and inputs as indices into
// it, the `outputs` beside them -- and pks / ios are not read.  A Pedersen source has no pk_index.
struct BatchSource {
  int kind = 0; size_t n = 0;       // a ProofKind (sizes: proof_kind.h)
  bool wire = false; int validate = 0;
  const uint8_t *sks = nullptr, *pks = nullptr, *ios = nullptr; const uint32_t *io_counts = nullptr;
  const uint8_t *ads = nullptr; const uint32_t *ad_lens = nullptr; const uint8_t *proofs = nullptr;   // proofs / pks / sks may be NULL for provers
  size_t n_shared = 0; const uint8_t *table = nullptr; const uint32_t *pk_index = nullptr, *input_index = nullptr; const uint8_t *outputs = nullptr;
  // append: a chunk pushed to an open batch (plain or wire, never over a table) -- its n items go behind the n0 items and a0 pairs that
  // are already there, and the decode flag is the batch's (cleared at open, not per chunk)
  bool append = false; size_t n0 = 0, a0 = 0;
};
// how the entry points fill one from their argument lists: x || y arrays, a table with indices, and either as wire bytes
inline BatchSource plain_source(int kind, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                                const uint32_t *ad_lens, const uint8_t *proofs) {
  BatchSource s;
  s.kind = kind; s.n = n; s.pks = pks; s.ios = ios; s.io_counts = io_counts; s.ads = ads; s.ad_lens = ad_lens; s.proofs = proofs;
  return s;
}
inline BatchSource shared_source(int kind, size_t n, size_t n_shared, const uint8_t *table, const uint32_t *pk_index, const uint32_t *input_index,
                                 const uint8_t *outputs, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs) {
  BatchSource s = plain_source(kind, n, nullptr, nullptr, io_counts, ads, ad_lens, proofs);
  s.n_shared = n_shared; s.table = table; s.pk_index = pk_index; s.input_index = input_index; s.outputs = outputs;
  return s;
}
inline BatchSource wire_source(BatchSource s, int validate) { s.wire = true; s.validate = validate; return s; }
// Staging, then the phases of a staged batch's run, shared by the C ABI's run calls (capi.hip) and the pool's workers (pool.hip).  One
// stager over a source: opening and close are shared, the payload (what is copied, what decodes it) is the flavour's.  wait = false
// (pool.hip): nothing is waited for, and a wire source's decode flag is read by run_collect.
int ctx_create(int suite, int device, bool lane_owner, avrf_ctx **out);
int ctx_stage(avrf_ctx *c, const BatchSource &src, bool wait);
// the host's check of a shared-table source (every index < n_shared; outputs present), which ctx_stage makes itself and the pool makes on
// the submitting thread as well
bool shared_indices_ok(const BatchSource &src);
bool suite_host_weights(int suite);                                   // sponge / SHA-256 transcript: the host squeezes the weight stream itself (no seed)
void sha512_many(WeightJob *const *jobs, int k);                      // k <= 16 transcripts hashed together: scalar, eight or sixteen lanes, as the host CPU allows

// The run of a staged Thin or Pedersen batch in phases, whole or segmented (include/avrf.h avrf_*_batch_run, avrf_*_batch_run_segments).
// Each refuses out of order, an error leaves the context idle, and a run with nothing to do (no items, or no segments) passes through
// every phase without device work.  What a run asks for: the whole batch, or n_seg groups of seg_items[v] consecutive items; a shared-
// table staging runs segmented only with shared_ok (avrf_*_batch_run_shared_segments, a context of its own lane), in the shorter of
// the merged and the expanded layout.
struct RunRequest { bool segmented = false; size_t n_seg = 0; const uint32_t *seg_items = nullptr; bool shared_ok = false, unit_weights = false; };
inline bool ctx_busy(const avrf_ctx *c) { return c->run.phase != RunPhase::Idle; }
//   run_begin     a segmented run's layout (in locals first: a refusal changes nothing) and buffer sizing; then validation + prepare
//                 kernel + copies back on c->stream, once for all groups -- an open batch's pushes have enqueued that already.
//                 Segmented over a shared table the checks are those of the items alone (the table's range flag is not taken over)
//                 and Pedersen's prepare merges the pairs as the run's layout wants them
//   run_collect   (c->stream's work has completed) the decode flag of a wire staging or of an open batch's chunks, then the batch's
//                 flag word: AVRF_INVALID_DATA for a whole-batch run; a segmented run finds the items that raised it in the per-item
//                 attribution pass, which waits for c->stream
//   run_messages  how many counter-mode transcripts a caller that hashes several contexts' together (pool.hip) takes one by one: 0 for a
//                 sponge / SHA-256 suite or a run with nothing to do (run_hash does what there is to do), 1 for a whole-batch run, n_seg
//                 for a segmented one.  run_job describes message v (the whole batch's in place, a group's built at a place of its own:
//                 distinct v may be built from different threads), run_seed stores its digest
//   run_hash      everything on the calling thread (spread: and the process's host pool): counter-mode suites hash prefix || records,
//                 sponge / SHA-256 suites squeeze the weight stream of the batch or of every group, an open batch finalises a clone
//   run_launch    weight stream or seeds up, the terms kernel (segmented: offsets up and padding scalars zeroed first), then ONE MSM
//                 chain on c->stream / c->L with c->chain(), whatever n_seg is -- but none for a segmented run of a context of its own lane
//   run_end       collects the chain (waits for the stream only with the lane's own record); a segmented run of a context of its own lane
//                 runs msm_te_segments here instead, which keeps that call's loop of single MSMs below eight segments.  Then a status
//                 from every sum: status_out[0], or status_out[0 .. n_seg) with the per-item statuses folded in
int run_begin(avrf_ctx *c, int kind, const RunRequest &rq = RunRequest());
int run_collect(avrf_ctx *c, int kind);
size_t run_messages(const avrf_ctx *c);
void run_job(avrf_ctx *c, size_t v, WeightJob *job);
void run_seed(avrf_ctx *c, size_t v, const uint8_t digest[64]);
int run_hash(avrf_ctx *c, int kind, bool spread);
int run_launch(avrf_ctx *c, int kind);
int run_end(avrf_ctx *c, int kind, int32_t *status_out);
inline bool run_chain_enqueued(const avrf_ctx *c) { return c->run.phase == RunPhase::Launched; }   // run_launch came through: a chain may be in flight on c->L
// closes a run from outside its phases (the pool when a slot's run is over or the slot dies; the caller deals with stream and chain record)
inline void run_close(avrf_ctx *c) { c->run.phase = RunPhase::Idle; }
double now_us();
}  // namespace avrf
