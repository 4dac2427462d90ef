// thin_seg.h -- thin::BatchVerifier over SEGMENTS of one staged batch (avrf_thin_batch_run_segments, include/avrf.h): n_seg
// independent verifiers over consecutive runs of items, each with its own weight transcript and its own verdict (src/thin.rs:188-326),
// built in one pass over the device.
//
// Segment v covers the staged items [seg_off[v], seg_off[v + 1]).  Its MSM terms are those of a plain batch of just these items, in the
// reference's order (src/thin.rs:287-317: R, pk, (O, I).., then (G, g_v) last), at [v L, v L + n_v) of arrays of n_seg * L terms, where
// n_v = 2 items_v + 2 pairs_v + 1 and L is the largest n_v.  The scalars of [v L + n_v, (v + 1) L) are zero -- the engine never gathers
// a zero scalar's base (msm.h msm_te_segments), so the padding bases stay unwritten.  An empty segment has no terms at all.
//
// pedersen::BatchVerifier (avrf_pedersen_batch_run_segments; src/pedersen.rs:303-426) takes the same layout with n_v = 5 items_v + 2:
// per item O, Ok, I, Yb, R (src/pedersen.rs:383-410), then (G, -sum u s) and (BLINDING_BASE, -sum u sb) last (:413-418).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "msm.h"
#include "suite_dispatch.h"

namespace avrf {

struct BatchDev;
struct Seed64;

// the segment of item j: the largest v < n_seg with seg_off[v] <= j (an empty segment shares its offset with the next one, which wins).
// The same search finds the item of I/O pair k in the items' pair offsets (an item without pairs shares its offset likewise).
__device__ __forceinline__ uint32_t segment_of(const uint32_t *__restrict__ seg_off, uint32_t n_seg, uint32_t j) {
  uint32_t lo = 0, hi = n_seg;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (seg_off[mid] <= j) lo = mid; else hi = mid; }
  return lo;
}

// Per-suite launch table (thin_seg.hip, built once per suite like vrf_batch.hip).
template <class S> struct SegOps {
  // d_seg_off: n_seg + 1 item offsets; d_seeds: n_seg weight-transcript digests (counter-mode transcripts; a sponge suite's streams are
  // b.weights, segment v's 16-byte weights from item seg_off[v] on); d_wsz: n x 8 words of scratch (each item's w s z0).  The caller has
  // zeroed d_scalars (n_seg * L x 8 words).
  static void thin_terms(const BatchDev &b, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t L, const Seed64 *d_seeds, const uint32_t *d_c,
                         const uint32_t *d_z, uint32_t *d_wsz, uint32_t *d_scalars, te_pre_raw *d_pre, hipStream_t st);
  // the checks of k_thin_prepare (src/thin.rs:266-271) once more, per item: d_status[j] = 2 for an item that raised the batch's flag word
  static void item_flags(const BatchDev &b, int32_t *d_status, hipStream_t st);
  // Pedersen.  d_seeds / b.weights as above with 32-byte weights; d_merged: k_ped_prepare's merged pairs (n x 128 bytes); d_usb: n x 16
  // words of scratch (each item's u s, then each item's u sb).
  static void ped_terms(const BatchDev &b, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t L, const Seed64 *d_seeds, const uint32_t *d_c,
                        const uint8_t *d_merged, uint32_t *d_usb, uint32_t *d_scalars, te_pre_raw *d_pre, hipStream_t st);
  // the checks of k_ped_prepare (src/pedersen.rs:276-278, 348-353) once more, per item
  static void ped_item_flags(const BatchDev &b, int32_t *d_status, hipStream_t st);
};
#define AVRF_SEG(suite, CALL) with_suite((suite), [&](auto tag_) { return SegOps<typename decltype(tag_)::type>::CALL; })

}  // namespace avrf
