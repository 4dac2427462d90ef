// capi_internal.h -- what the translation units of libavrf.so share about a context (capi.hip, pool.hip): buffers, the
// execution lane (stream + MSM workspace) and the phases of BatchVerifier::verify (src/thin.rs:257-325, src/pedersen.rs:341-426).
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
  // a segmented run (seg_launch below): the terms kernel's per-item scratch (Thin w s z0, n x 32 bytes; Pedersen u s and u sb, n x 64),
  // the n_seg + 1 item offsets and the n_seg weight seeds of the chain being built
  DevBuf d_seg_wsz, d_seg_off, d_seg_seeds;
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
  bool wire_pending = false;              // staged from wire bytes without waiting: batch_collect reads the decode flag (h_flags[2])
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
  // the last segmented run of the staged batch (avrf_thin_batch_run_segments, avrf_pedersen_batch_run_segments; thin_seg.h): terms of its
  // own, n_seg * seg_L of them, so that the plain run's terms stay what they were; seg_off (n_seg + 1 item offsets) describes them while
  // seg_gen == stage_gen.  (A pool slot has neither: its segmented terms go to the arrays of the lane it borrows, seg_launch.)
  // seg_row0: non-empty exactly when that run took the merged layout of a shared-table staging (thin_shared.h "Segments"): the term of each
  // segment's row 0.  d_seg_plan: the per-run plan of such a run (shared_seg_plan).
  uint64_t seg_gen = 0; size_t seg_L = 0; std::vector<uint32_t> seg_off, seg_row0;
  avrf::DevBuf d_seg_scalars, d_seg_pre, d_seg_plan;
  std::vector<uint8_t> h_seg_msg;   // the segments' weight-transcript messages, prefix || records each
  // the segmented run in flight (seg_begin .. seg_end, run_phase 3 and 4): its layout, the per-item statuses of the attribution pass
  // (empty unless the batch's flag word was set) and, page-locked so that the copies up never wait for the lane, the item offsets
  // (n_seg + 1 words, padded to 64 bytes) followed by the n_seg weight seeds and, for the merged layout, the n_seg terms row0
  struct SegRun { size_t n_seg = 0, L = 0, padded = 0; bool merged = false; std::vector<uint32_t> off, row0; std::vector<int32_t> item_status; } seg;
  avrf::PinBuf h_seg_up;
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
  int run_phase = 0;             // batch_begin / batch_hash / batch_end: 1, 2; a segmented run (seg_begin .. seg_end): 3, 4
  bool unit_weights = false;      // batch_launch: every item's weight is 1 (avrf_thin_verify runs ONE item as its own equation through the MSM path)
  double run_t0 = 0, run_begin_us = 0, run_msm_us = 0;
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
// Staging, then the phases of a staged batch's run, shared by the three-call ABI (capi.hip) and the pool's workers (pool.hip).  One stager
// over a source: opening and close are shared, the payload (what is copied, what decodes it) is the flavour's.  wait = false (pool.hip):
// nothing is waited for, and a wire source's decode flag is read by batch_collect.
int ctx_create(int suite, int device, bool lane_owner, avrf_ctx **out);
int ctx_stage(avrf_ctx *c, const BatchSource &src, bool wait);
// the host's check of a shared-table source (every index < n_shared; outputs present), which ctx_stage makes itself and the pool makes on
// the submitting thread as well
bool shared_indices_ok(const BatchSource &src);
// validation + prepare kernel + copies back enqueued on c->stream.  segmented (seg_begin): over a shared table the checks are those of the
// items alone -- the table's range flag is not taken over -- and Pedersen's prepare merges the pairs as the run's layout (c->seg) wants them
int batch_begin(avrf_ctx *c, int kind, bool segmented = false);
int batch_collect(avrf_ctx *c, int kind);                             // (c->stream's work has completed) AVRF_INVALID_DATA for a refused item
bool suite_host_weights(int suite);                                   // sponge / SHA-256 transcript: batch_seed squeezes the weight stream itself (no seed)
int batch_seed(avrf_ctx *c, int kind, uint8_t digest[64]);            // the weight transcript on the calling thread
void sha512_many(WeightJob *const *jobs, int k);                      // k <= 16 transcripts hashed together: scalar, eight or sixteen lanes, as the host CPU allows
int batch_launch(avrf_ctx *c, int kind, const uint8_t digest[64]);    // terms kernel + MSM chain enqueued on c->stream / c->L
int batch_end(avrf_ctx *c, int kind);                                 // waits for the chain, folds, verdict
// The segmented run of a staged Thin or Pedersen batch (include/avrf.h avrf_thin_batch_run_segments, avrf_pedersen_batch_run_segments) in
// phases of the same discipline: each refuses out of order, an error leaves the context idle.  run_phase 3 from seg_begin, 4 from seg_launch.
//   seg_begin    layout check (counts, limits), buffer sizing, batch_begin: validation + prepare kernel + copies back on c->stream.
//                A shared-table staging is refused unless shared_ok (avrf_*_batch_run_shared_segments, a context of its own lane): the
//                layout is then the shorter of merged and expanded (include/avrf.h)
//   seg_collect  (c->stream's work has completed) a wire batch's decode flag; only when the batch's flag word is set, the per-item
//                attribution pass, which waits for c->stream
//   seg_hash     the n_seg weight transcripts on the calling thread (spread: and the process's host pool): counter-mode suites hash
//                prefix || the segment's records, sponge / SHA-256 suites squeeze every segment's weight stream.  A caller that hashes
//                several contexts' transcripts together (pool.hip) takes the counter-mode messages one by one instead: seg_job builds
//                message v and describes it, seg_seed stores its digest
//   seg_launch   seeds and offsets up, padding scalars zeroed, terms kernel; a pool slot: ONE chain enqueued on c->stream / c->L with
//                c->chain(), whatever n_seg is
//   seg_end      a pool slot: collects the chain (waits for the stream only with the lane's own record).  A context of its own lane
//                runs msm_te_segments here instead, which keeps that call's loop of single MSMs below eight segments.  Then
//                status_out[0 .. n_seg), the per-item statuses folded in
int seg_begin(avrf_ctx *c, int kind, size_t n_seg, const uint32_t *seg_items, bool shared_ok = false);
int seg_collect(avrf_ctx *c, int kind);
int seg_hash(avrf_ctx *c, int kind, bool spread);
void seg_job(avrf_ctx *c, int kind, size_t v, WeightJob *job);
void seg_seed(avrf_ctx *c, size_t v, const uint8_t digest[64]);
int seg_launch(avrf_ctx *c, int kind);
int seg_end(avrf_ctx *c, int kind, int32_t *status_out);
double now_us();
}  // namespace avrf
