// thin_shared.h -- thin::BatchVerifier over a table of shared points (avrf_thin_batch_stage_shared, include/avrf.h).
//
// The reference merges ONE shared base into a single MSM term: the generator, g -= w s z0 (src/thin.rs:303,316-317).  A batch
// whose public keys and inputs come from a table of T points gets the same treatment for every row: the scalars of all the
// terms that share a base are added in Fr, which leaves sum scalar * base -- the group element the verdict tests -- unchanged
// and the MSM at n + tot_io + T + 1 terms instead of 2 n + 2 tot_io + 1.
//
//   staging (once per staged batch, shared_plan + rows_pre):
//     gather    the table rows into the plain staged layout (d_pks, d_ios with the outputs beside their inputs), so that
//               k_thin_prepare and its per-item checks run as they are; histogram of the references per row
//     scan      row_off[T + 1]: where each row's contributions start in row order
//     place     pos[C]: the slot of contribution t (item j's key: t = j; I/O pair k's input: t = n + k) in row order,
//               slot_row[C]: the row a slot belongs to.  C = n + tot_io.  The order inside a row is whatever the atomics
//               gave: Fr addition is exact, so it cannot change a result.
//     rows_pre  every row once to te_pre (Montgomery x, y, k = d x y); canonical-range check of every row
//   run (thin_terms): k_thin_terms_shared calls thin_item (batch_terms_dev.h), the one statement of an item's arithmetic that
//     k_thin_terms calls too; its sink emits the R and O terms and stores the key / input scalars (Montgomery form) to
//     contrib[pos[.]]; k_shared_lanes sums equal contiguous shares of SHARED_SHARE slots per lane -- rows inside a share are
//     finished there, a row that crosses a share boundary leaves partials; k_shared_merge adds the partials of each such row
//     (min(lanes, T) units, four per block, 256 threads on each cut row) and the generator term.  Three launches whatever the distribution of the references.
//
// Pedersen (avrf_pedersen_batch_stage_shared): an item has no key, so the references are the tot_io inputs alone (C = tot_io, t = k for
// I/O pair k) and the table holds inputs only.  The reference already merges G and BLINDING_BASE (src/pedersen.rs:387-418); an item's
// input term is -t s I_merged = sum_i (-t s z_i) I_i (merge_ios, common.rs:389-419), so each pair adds -t s z_i to its row and the MSM has
// 4 n + T + 2 terms instead of 5 n + 2.  Same plan, same k_shared_lanes; k_ped_terms_shared is the ped_item caller and k_shared_merge<S, 2>
// writes both base terms.
//
// Segments (avrf_thin_batch_run_shared_segments, avrf_pedersen_batch_run_shared_segments): the sum runs per (segment, row) pair instead of
// per row, which gives segment v the reference's treatment of G restricted to its own items.  A per-run plan (shared_seg_plan) sorts the
// contributions by virtual row v T + r; k_shared_lanes / k_shared_merge sum them as they are and place row v T + r at the term
// shared_row_term names; k_shared_seg_base writes each segment's base term(s).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "msm.h"
#include "suite_dispatch.h"

namespace avrf {

struct BatchDev;
struct Seed64;

enum { SHARED_SHARE = 8 };                                            // slots one lane of k_shared_lanes sums
constexpr size_t shared_lanes(size_t n_contrib) { return (n_contrib + SHARED_SHARE - 1) / SHARED_SHARE; }
// per-run scratch of a lane: contrib (8 words per slot), then per lane of k_shared_lanes head and tail partials (16 words) and the tail's row (1)
constexpr size_t shared_scratch_words(size_t n_contrib) { return 8 * n_contrib + 17 * shared_lanes(n_contrib) + 16; }
// the plan of a staging: cursor[T + 1] | row_off[T + 1] | pos[C] | slot_row[C] | range flag of the table
constexpr size_t shared_plan_words(size_t n_shared, size_t n_contrib) { return 2 * (n_shared + 1) + 2 * n_contrib + 4; }

enum : uint32_t { SHARED_NO_ROW = 0xffffffffu };
struct SharedPlan {
  const uint32_t *row_off, *pos, *slot_row;
  const te_pre_raw *rows;          // table_rows precomputed bases
  uint32_t n_shared, n_contrib;    // the plan's rows (a segmented run's: VIRTUAL rows, below) and contributions
  // A segmented run's plan (shared_seg_plan): row v T + r is row r of the table AS SEGMENT v REFERENCES IT, T = table_rows, so that
  // n_shared = n_seg T; seg_row0[v] is the MSM term of segment v's row 0 (SHARED_NO_ROW: an empty segment, which has no terms).
  // A staging's own plan has seg_row0 == NULL and table_rows == n_shared: row r is the term t0 + r the launch names.
  const uint32_t *seg_row0; uint32_t table_rows;
};
// THE map from a plan's row to its MSM term (k_shared_lanes and k_shared_merge both go through it); r: the table row whose base it takes.
// SHARED_NO_ROW: the row has no term.
__device__ __forceinline__ uint32_t shared_row_term(const SharedPlan &p, uint32_t t0, uint32_t row, uint32_t &r) {
  if (!p.seg_row0) { r = row; return t0 + row; }
  const uint32_t v = row / p.table_rows, s0 = p.seg_row0[v];
  r = row - v * p.table_rows;
  return s0 == SHARED_NO_ROW ? (uint32_t)SHARED_NO_ROW : s0 + r;
}

// Gather + counting sort of a staging (suite-independent: shared_stage.hip).  idx: pk_index (n) then input_index (tot_io); plan: shared_plan_words.
// n: the items that reference a KEY row -- 0 for a Pedersen batch, whose references are the tot_io inputs alone (d_pks is then not touched).
// An index >= n_shared is the host's to refuse; the kernels clamp it so that no read leaves the table.
// (a refused memset or launch comes back as its error, so that a failed plan is never reported as a good staging)
hipError_t shared_plan(const uint8_t *d_table, uint32_t n_shared, const uint32_t *d_idx, const uint8_t *d_outputs, uint32_t n, uint32_t tot_io,
                       uint8_t *d_pks, uint8_t *d_ios, uint32_t *d_plan, hipStream_t st);
inline SharedPlan shared_plan_view(const uint32_t *d_plan, const te_pre_raw *d_rows, size_t n_shared, size_t n_contrib) {
  const uint32_t *row_off = d_plan + (n_shared + 1);
  return SharedPlan{row_off, row_off + (n_shared + 1), row_off + (n_shared + 1) + n_contrib, d_rows, (uint32_t)n_shared, (uint32_t)n_contrib, nullptr, (uint32_t)n_shared};
}
inline uint32_t *shared_plan_flag(uint32_t *d_plan, size_t n_shared, size_t n_contrib) { return d_plan + 2 * (n_shared + 1) + 2 * n_contrib; }

// The plan of ONE segmented run over a staging (avrf_thin_batch_run_shared_segments, avrf_pedersen_batch_run_shared_segments; merged
// layout): contribution t belongs to the segment of its item, so it gets the virtual row v(t) T + row(t), and the same counting sort
// (k_shared_scan, k_shared_place, without the gather) puts the contributions in (segment, row) order.  n_seg T < n_seg L <= 2^20 bounds
// the histogram.  d_plan: cursor[R + 1] | row_off[R + 1] | pos[C] | slot_row[C] | vrow[C] | seg_row0[n_seg], R = n_seg T -- the caller has
// copied seg_row0 up.  d_idx as shared_plan; n: the staged items, nk: those that reference a key row (n, or 0 for Pedersen);
// d_io_off: the n + 1 pair offsets; d_seg_off: the n_seg + 1 item offsets.
constexpr size_t shared_seg_plan_words(size_t n_seg, size_t n_shared, size_t n_contrib) { return 2 * (n_seg * n_shared + 1) + 3 * n_contrib + n_seg + 4; }
inline uint32_t *shared_seg_plan_row0(uint32_t *d_plan, size_t n_seg, size_t n_shared, size_t n_contrib) { return d_plan + 2 * (n_seg * n_shared + 1) + 3 * n_contrib; }
hipError_t shared_seg_plan(const uint32_t *d_idx, const uint32_t *d_io_off, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t n_shared, uint32_t n,
                           uint32_t nk, uint32_t tot_io, uint32_t *d_plan, hipStream_t st);
inline SharedPlan shared_seg_plan_view(const uint32_t *d_plan, const te_pre_raw *d_rows, size_t n_seg, size_t n_shared, size_t n_contrib) {
  SharedPlan p = shared_plan_view(d_plan, d_rows, n_seg * n_shared, n_contrib);
  p.seg_row0 = p.slot_row + 2 * n_contrib; p.table_rows = (uint32_t)n_shared;
  return p;
}

// Per-suite launch table (thin_shared.hip, built once per suite like vrf_batch.hip).
template <class S> struct SharedOps {
  static hipError_t rows_pre(const uint8_t *d_table, uint32_t n_shared, te_pre_raw *d_rows, uint32_t *d_flag, hipStream_t st);
  // terms in the layout of include/avrf.h: (R_j, w_j) at j + io_off[j], (O_ji, w c z_i) behind it, row r at n + tot_io + r, (G, g) last
  static void thin_terms(const BatchDev &b, const Seed64 &seed, uint64_t j0, const uint32_t *d_c, const uint32_t *d_z, const SharedPlan &p,
                         uint32_t tot_io, uint32_t *d_scratch, uint32_t *d_scalars, te_pre_raw *d_pre, uint32_t *d_gpart, hipStream_t st);
  // Pedersen: item j's four terms at 4 j, row r at 4 n + r, (G, .) and (BLINDING_BASE, .) last.  d_merged: what k_ped_prepare<S, true> left
  // (merged outputs, then the z_i); d_gpart: 2 x ceil(n / 128) partials as BatchOps::ped_terms.  p.n_contrib = tot_io.
  static void ped_terms(const BatchDev &b, const Seed64 &seed, uint64_t j0, const uint32_t *d_c, const uint8_t *d_merged, const SharedPlan &p,
                        uint32_t *d_scratch, uint32_t *d_scalars, te_pre_raw *d_pre, uint32_t *d_gpart, hipStream_t st);
  // The merged layout of a segmented run (include/avrf.h avrf_thin_batch_run_shared_segments): segment v's item terms from v L on (Thin
  // (R_j, w_j) at (j - first) + (io_off[j] - io_off[first]) with its outputs behind it, Pedersen four terms at 4 (j - first)), its T row
  // terms at seg_row0[v], its base term(s) behind them.  p: shared_seg_plan_view; d_seg_off / d_seeds / L as SegOps (thin_seg.h);
  // d_wsz: each item's w s z0 (Thin, n x 8 words) or u s then u sb (Pedersen, n x 16); the caller has zeroed d_scalars.
  static void thin_seg_terms(const BatchDev &b, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t L, const Seed64 *d_seeds, const uint32_t *d_c,
                             const uint32_t *d_z, const SharedPlan &p, uint32_t *d_scratch, uint32_t *d_wsz, uint32_t *d_scalars, te_pre_raw *d_pre, hipStream_t st);
  static void ped_seg_terms(const BatchDev &b, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t L, const Seed64 *d_seeds, const uint32_t *d_c,
                            const uint8_t *d_merged, const SharedPlan &p, uint32_t *d_scratch, uint32_t *d_wsz, uint32_t *d_scalars, te_pre_raw *d_pre, hipStream_t st);
};
#define AVRF_SHARED(suite, CALL) with_suite((suite), [&](auto tag_) { return SharedOps<typename decltype(tag_)::type>::CALL; })

}  // namespace avrf
