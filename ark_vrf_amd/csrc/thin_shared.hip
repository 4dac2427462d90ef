// thin_shared.hip -- the device side of thin::BatchVerifier over a table of shared points (thin_shared.h).
//
//   k_shared_pre                     : every table row once to te_pre, through the suite's own te_make_pre
//   k_ped_terms_shared               : ped_item (batch_terms_dev.h; src/pedersen.rs:369-410), as k_ped_terms: the four terms on the item's own points;
//                                      the input scalars -t s z_i go to contrib[pos[.]] (thin_shared.h "Pedersen")
//   k_thin_terms_shared              : thin_item (batch_terms_dev.h; src/thin.rs:287-313), as k_thin_terms of vrf_batch.hip: the R and
//                                      output terms; the key and input scalars go to contrib[pos[.]] in Montgomery form
//   k_shared_lanes / k_shared_merge  : the segmented sum of contrib in Fr -> the T row terms; the generator term (src/thin.rs:303,316-317)
//   k_thin_terms_shared_seg, k_ped_terms_shared_seg, k_shared_seg_base : the same over SEGMENTS of the staged batch (thin_shared.h
//                                      "Segments"): the item under its segment's weight stream, the sums per (segment, row) through
//                                      the same k_shared_lanes / k_shared_merge, one block per segment for its base term(s)
// One lane per item / reference / share; scalar-field sums in 8 x u32 Montgomery form (fp256.h).
// (the staging -- k_shared_gather / _scan / _place, shared_plan, shared_seg_plan -- knows no suite: shared_stage.hip)
#include "thin_shared.h"
#include "thin_seg.h"
#include "proto_dev.h"
#include "batch_terms_dev.h"

// Built once per suite (-DAVRF_TU_SUITE=<id>, csrc/Makefile): the suite's kernels and the explicit instantiation of SharedOps<S>,
// which capi.hip reaches through AVRF_SHARED.
#ifndef AVRF_TU_SUITE
#error "thin_shared.hip is built once per suite: -DAVRF_TU_SUITE=<id> (csrc/Makefile)"
#endif
namespace avrf {

// row r -> Montgomery x, y, k = d x y (what emit_term of vrf_batch.hip computes per reference); a coordinate >= q is flagged
template <class S>
__global__ void __launch_bounds__(128)
k_shared_pre(const uint8_t *__restrict__ table, uint32_t n_shared, te_pre *__restrict__ rows, uint32_t *__restrict__ flag) {
  using Fq = typename S::Fq;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_shared) return;
  const uint8_t *xy = table + 64 * (size_t)r;
  fp x = fp_load_le(xy), y = fp_load_le(xy + 32);
  if (ge_p<Fq>(x) || ge_p<Fq>(y)) atomicOr(flag, (uint32_t)FLAG_RANGE);
  store_pre(rows + r, te_make_pre<S>(fp_to_mont<Fq>(x), fp_to_mont<Fq>(y)));
}


// k_thin_terms_shared's sink of thin_item's terms: item j emits (R_j, w_j) at j + io0 and (O_i, w c z_i) at j + io0 + 1 + i; w c (its
// key's row) and -w s z_i (its inputs' rows) go to contrib, in Montgomery form.
// t0: 0 for the plain run; a segmented run's kernel moves the item terms by v L - (first + io_off[first]), first = the segment's first
// item, so that the segment's slice starts with its first item's R (mod 2^32, as SegTerms of thin_seg.hip).
template <class S> struct SharedTerms {
  uint32_t *__restrict__ scalars; te_pre *__restrict__ pre; const uint32_t *__restrict__ pos; uint32_t *__restrict__ contrib; uint32_t n, t0;
  AVRF_DI void r(uint32_t j, uint32_t io0, const fp &w_plain, const uint8_t *xy) const { emit_term<S>(scalars, pre, t0 + j + io0, w_plain, xy); }
  AVRF_DI void key(uint32_t j, uint32_t, const fp &wc) const { fp_store(contrib + 8 * (size_t)pos[j], wc); }
  AVRF_DI void output(uint32_t j, uint32_t io0, uint32_t i, const fp &sc_plain, const uint8_t *xy) const { emit_term<S>(scalars, pre, t0 + j + io0 + 1 + i, sc_plain, xy); }
  AVRF_DI void input(uint32_t, uint32_t io0, uint32_t i, const fp &sc_mont, const uint8_t *) const { fp_store(contrib + 8 * (size_t)pos[n + io0 + i], sc_mont); }
};

template <class S>
__global__ void __launch_bounds__(128)
k_thin_terms_shared(BatchDev b, Seed64 seed, uint64_t j0, const uint32_t *__restrict__ c_in, const uint32_t *__restrict__ z_in,
                    const uint32_t *__restrict__ pos, uint32_t *__restrict__ contrib, uint32_t *__restrict__ scalars,
                    te_pre *__restrict__ pre, uint32_t *__restrict__ gpart) {
  using Fr = typename S::Fr;
  __shared__ fp red[128];
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  fp ws = fp_zero();
  if (j < b.n) ws = thin_item<S>(b, seed, j0, c_in, z_in, j, SharedTerms<S>{scalars, pre, pos, contrib, b.n, 0});
  const fp sum = block_sum<Fr, 128>(ws, red);                                  // of w_j s_j z0 (Montgomery form), thin.rs:303
  if (threadIdx.x == 0) fp_store(gpart + 8 * (size_t)blockIdx.x, sum);
}

// the same per item under its SEGMENT's weight stream, with its index inside the segment (k_thin_terms_seg of thin_seg.hip): the R and
// output terms go to the segment's slice, the key and input scalars to contrib[pos[.]] of the run's plan, w s z0 to wsz
template <class S>
__global__ void __launch_bounds__(128)
k_thin_terms_shared_seg(BatchDev b, const uint32_t *__restrict__ seg_off, uint32_t n_seg, uint32_t L, const Seed64 *__restrict__ seeds,
                        const uint32_t *__restrict__ c_in, const uint32_t *__restrict__ z_in, const uint32_t *__restrict__ pos,
                        uint32_t *__restrict__ contrib, uint32_t *__restrict__ wsz, uint32_t *__restrict__ scalars, te_pre *__restrict__ pre) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b.n) return;
  const uint32_t v = segment_of(seg_off, n_seg, j), first = seg_off[v];
  Seed64 seed = {};
  if (!b.weights) seed = seeds[v];                        // (a sponge suite's stream sits at b.weights + 16 j whatever the segment)
  const uint32_t t0 = v * L - (first + b.io_off[first]);
  // j0 = -first: thin_item takes weight j0 + j = the item's index inside its segment
  const fp ws = thin_item<S>(b, seed, (uint64_t)0 - first, c_in, z_in, j, SharedTerms<S>{scalars, pre, pos, contrib, b.n, t0});
  fp_store(wsz + 8 * (size_t)j, ws);                      // w_j s_j z0 (Montgomery form), thin.rs:303
}

// k_ped_terms_shared's sink of ped_item's terms: item j's (O, t c), (Ok, t), (Yb, u c), (R, u) at 4 j + {0, 1, 2, 3}.  Term 2, (I, -t s),
// is not emitted: the merged input is sum z_i I_i (common.rs:389-419), so -t s z_i goes to the row of pair i's input -- contrib[pos[io0 + i]]
// in Montgomery form, z_0 = 1 and z_i (i >= 1) as k_ped_prepare<S, true> left them behind the merged outputs.
template <class S> struct PedSharedTerms {
  uint32_t *__restrict__ scalars; te_pre *__restrict__ pre; const uint32_t *__restrict__ io_off; const uint32_t *__restrict__ z_in;
  const uint32_t *__restrict__ pos; uint32_t *__restrict__ contrib; uint32_t t0;   // t0: 0, or a segmented run's v L - 4 first
  using Fr = typename S::Fr;
  AVRF_DI void term(uint32_t j, uint32_t k, const fp &sc_plain, const uint8_t *xy) const {
    if (k != 2) { emit_term<S>(scalars, pre, t0 + 4 * j + (k > 2 ? k - 1 : k), sc_plain, xy); return; }
    const uint32_t io0 = io_off[j], m = io_off[j + 1] - io0;
    if (!m) return;                                                     // no pair: the merged input is the identity (pedersen.rs:264-267)
    const fp ts = fp_to_mont<Fr>(sc_plain);
    fp_store(contrib + 8 * (size_t)pos[io0], ts);
    for (uint32_t i = 1; i < m; i++)
      fp_store(contrib + 8 * (size_t)pos[io0 + i], fp_mul<Fr>(ts, fp_to_mont<Fr>(fp_from_u128(z_in + 4 * (size_t)(io0 + i)))));
  }
};

// per-item part of pedersen::BatchVerifier::verify over a table of shared inputs (ped_item, batch_terms_dev.h), as k_ped_terms of vrf_batch.hip
template <class S>
__global__ void __launch_bounds__(128)
k_ped_terms_shared(BatchDev b, Seed64 seed, uint64_t j0, const uint32_t *__restrict__ c_in, const uint8_t *__restrict__ merged_xy,
                   const uint32_t *__restrict__ pos, uint32_t *__restrict__ contrib, uint32_t *__restrict__ scalars, te_pre *__restrict__ pre,
                   uint32_t *__restrict__ gpart, uint32_t *__restrict__ bpart) {
  using Fr = typename S::Fr;
  __shared__ fp red[128];
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  fp us = fp_zero(), usb = fp_zero();
  if (j < b.n)
    us = ped_item<S>(b, seed, j0, c_in, merged_xy, j,
                     PedSharedTerms<S>{scalars, pre, b.io_off, reinterpret_cast<const uint32_t *>(merged_xy + 128 * (size_t)b.n), pos, contrib, 0}, usb);
  const fp gsum = block_sum<Fr, 128>(us, red);
  if (threadIdx.x == 0) fp_store(gpart + 8 * (size_t)blockIdx.x, gsum);
  __syncthreads();
  const fp bsum = block_sum<Fr, 128>(usb, red);
  if (threadIdx.x == 0) fp_store(bpart + 8 * (size_t)blockIdx.x, bsum);
}

// the same per item under its SEGMENT's weight stream (k_ped_terms_seg of thin_seg.hip); usb: two planes, u s at 8 j and u sb at 8 (n + j)
template <class S>
__global__ void __launch_bounds__(128)
k_ped_terms_shared_seg(BatchDev b, const uint32_t *__restrict__ seg_off, uint32_t n_seg, uint32_t L, const Seed64 *__restrict__ seeds,
                       const uint32_t *__restrict__ c_in, const uint8_t *__restrict__ merged_xy, const uint32_t *__restrict__ pos,
                       uint32_t *__restrict__ contrib, uint32_t *__restrict__ usb, uint32_t *__restrict__ scalars, te_pre *__restrict__ pre) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b.n) return;
  const uint32_t v = segment_of(seg_off, n_seg, j), first = seg_off[v];
  Seed64 seed = {};
  if (!b.weights) seed = seeds[v];                        // (a host-squeezed suite's stream sits at b.weights + 32 j whatever the segment)
  // j0 = -first: ped_item takes chunks 2 (j0 + j), 2 (j0 + j) + 1 = those of the item's index inside its segment
  fp u_sb;
  const fp u_s = ped_item<S>(b, seed, (uint64_t)0 - first, c_in, merged_xy, j,
                             PedSharedTerms<S>{scalars, pre, b.io_off, reinterpret_cast<const uint32_t *>(merged_xy + 128 * (size_t)b.n), pos, contrib,
                                               v * L - 4 * first}, u_sb);
  fp_store(usb + 8 * (size_t)j, u_s);                     // u_j s_j, u_j sb_j (Montgomery form), pedersen.rs:409-410
  fp_store(usb + 8 * ((size_t)b.n + j), u_sb);
}

// one block per segment: its base term(s) behind its T row terms -- (G, g_v) from the w s z0 of its items (src/thin.rs:303,316-317);
// NBASE = 2 (Pedersen): (G, -sum u s) and (BLINDING_BASE, -sum u sb) from the two planes of wsz (src/pedersen.rs:413-418)
template <class S, int NBASE>
__global__ void __launch_bounds__(256)
k_shared_seg_base(const uint32_t *__restrict__ seg_off, const uint32_t *__restrict__ seg_row0, uint32_t n_shared, uint32_t n,
                  const uint32_t *__restrict__ wsz, uint32_t *__restrict__ scalars, te_pre *__restrict__ pre) {
  __shared__ fp red[256];
  const uint32_t v = blockIdx.x, first = seg_off[v], items = seg_off[v + 1] - first;
  if (!items) return;                                     // (block-uniform) an empty segment has no terms: src/thin.rs:262-264
  const uint32_t t = seg_row0[v] + n_shared;
  base_term<S>(wsz + 8 * (size_t)first, items, scalars, pre, t, 0, red);
  if constexpr (NBASE == 2) {
    __syncthreads();
    base_term<S>(wsz + 8 * ((size_t)n + first), items, scalars, pre, t + 1, 1, red);
  }
}

// Lane l sums slots [l SHARE, (l + 1) SHARE) in slot order, whatever rows they belong to.  A run of one row's slots that begins
// and ends inside the share IS that row: its scalar is written.  A run cut by the share's start is the lane's head partial, one
// cut by its end only the tail partial (with the row it belongs to): k_shared_merge adds tail(l) + head(l + 1) + ... for that row.
// The same threads copy the precomputed bases into the row terms and zero the scalars of unreferenced rows.
template <class S>
__global__ void __launch_bounds__(256)
k_shared_lanes(SharedPlan p, const uint32_t *__restrict__ contrib, uint32_t *__restrict__ part, uint32_t *__restrict__ tail_row,
               uint32_t *__restrict__ scalars, te_pre *__restrict__ pre, uint32_t t0) {
  using Fr = typename S::Fr;
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  for (uint32_t row = gid; row < p.n_shared; row += nth) {
    uint32_t r;
    const uint32_t t = shared_row_term(p, t0, row, r);
    if (t == SHARED_NO_ROW) continue;                                   // (a segmented run's empty segment: nothing is written)
    store_pre(pre + t, load_pre(reinterpret_cast<const te_pre *>(p.rows) + r));
    if (p.row_off[row] == p.row_off[row + 1]) fp_store(scalars + 8 * (size_t)t, fp_zero());
  }
  const uint32_t a = gid * SHARED_SHARE;
  if (a >= p.n_contrib) return;
  const uint32_t e = a + SHARED_SHARE < p.n_contrib ? a + SHARED_SHARE : p.n_contrib;
  uint32_t r = p.slot_row[a], tail = SHARED_NO_ROW;
  fp acc = fp_zero();
  for (uint32_t q = a; q <= e; q++) {
    const uint32_t rq = q < e ? p.slot_row[q] : SHARED_NO_ROW;
    if (rq != r) {                                                      // the run of row r ends at q
      const bool starts_here = p.row_off[r] >= a, ends_here = p.row_off[r + 1] <= q;
      uint32_t tr;
      if (starts_here && ends_here) fp_store(scalars + 8 * (size_t)shared_row_term(p, t0, r, tr), fp_from_mont<Fr>(acc));
      else if (!starts_here) fp_store(part + 16 * (size_t)gid, acc);
      else { fp_store(part + 16 * (size_t)gid + 8, acc); tail = r; }
      r = rq; acc = fp_zero();
    }
    if (q < e) acc = fp_add<Fr>(acc, fp_load(contrib + 8 * (size_t)q));
  }
  tail_row[gid] = tail;
}

// The rows cut by a share boundary: lane l = row_off[r] / SHARE of k_shared_lanes left the row's tail, its slots run on to lane
// (row_off[r + 1] - 1) / SHARE, and every lane on the way holds a head partial of it.  A block takes four UNITS one after the other and
// all its 256 threads add one cut row's partials (four independent running sums per thread, then a tree in LDS), so that ONE row of
// all 131 072 references -- 16 384 partials -- costs each thread 64 additions.  A unit is a ROW when there are no more rows than
// lanes (the shared case: a cut row is known from row_off alone), else a LANE (tail_row says whether it left a tail): min(lanes, T)
// units.  The last block is the generator term (base_term, as k_g_final); NBASE = 2 (Pedersen): the last two are (G, .) at t0 + T from gpart
// and (BLINDING_BASE, .) at t0 + T + 1 from the nparts partials behind it.
template <class S, int NBASE = 1>
__global__ void __launch_bounds__(256)
k_shared_merge(SharedPlan p, const uint32_t *__restrict__ part, const uint32_t *__restrict__ tail_row, uint32_t n_units, int by_row,
               const uint32_t *__restrict__ gpart, uint32_t nparts, uint32_t *__restrict__ scalars, te_pre *__restrict__ pre, uint32_t t0) {
  using Fr = typename S::Fr;
  __shared__ fp red[256];
  const uint32_t tid = threadIdx.x;
  // NBASE = 0 (a segmented run): no base term here, k_shared_seg_base writes every segment's own
  if constexpr (NBASE == 1) {
  if (blockIdx.x == gridDim.x - 1) { base_term<S, true>(gpart, nparts, scalars, pre, t0 + p.n_shared, 0, red); return; }   // (G, g), rolled as below
  } else if (NBASE && blockIdx.x + NBASE >= gridDim.x) {
    const uint32_t w = blockIdx.x + NBASE - gridDim.x;                  // 0: G, 1: BLINDING_BASE
    base_term<S, true>(gpart + 8 * (size_t)nparts * w, nparts, scalars, pre, t0 + p.n_shared + w, (int)w, red);
    return;
  }
  for (uint32_t i = 0; i < 4; i++) {                                    // (everything that decides control flow below is block-uniform)
    const uint32_t u = blockIdx.x * 4 + i;
    if (u >= n_units) break;
    uint32_t l, r;
    if (by_row) {
      r = u;
      const uint32_t s = p.row_off[r], e = p.row_off[r + 1];
      if (e == s) continue;
      l = s / SHARED_SHARE;
      if ((e - 1) / SHARED_SHARE == l) continue;                        // inside one share: k_shared_lanes finished it
    } else {
      l = u; r = tail_row[l];
      if (r == SHARED_NO_ROW) continue;
    }
    const uint32_t last = (p.row_off[r + 1] - 1) / SHARED_SHARE;        // <= (n_contrib - 1) / SHARE: a lane of k_shared_lanes
    fp acc = tid == 0 ? fp_load(part + 16 * (size_t)l + 8) : fp_zero();
    uint32_t k = l + 1 + tid;
    for (; k + 768 <= last; k += 1024) {                                // four loads in flight, one running sum
      const fp b0 = fp_load(part + 16 * (size_t)k), b1 = fp_load(part + 16 * (size_t)(k + 256)),
               b2 = fp_load(part + 16 * (size_t)(k + 512)), b3 = fp_load(part + 16 * (size_t)(k + 768));
      acc = fp_add<Fr>(fp_add<Fr>(fp_add<Fr>(fp_add<Fr>(acc, b0), b1), b2), b3);
    }
    for (; k <= last; k += 256) acc = fp_add<Fr>(acc, fp_load(part + 16 * (size_t)k));
    const fp sum = block_sum<Fr, 256, true>(acc, red);                  // (rolled: unrolled, the tree's eight masked additions spill SGPRs)
    uint32_t tr;                                                        // (a row with contributions has a term: its segment has items)
    if (tid == 0) fp_store(scalars + 8 * (size_t)shared_row_term(p, t0, r, tr), fp_from_mont<Fr>(sum));
    __syncthreads();                                                   // red is reused by the next unit
  }
}

template <class S> hipError_t SharedOps<S>::rows_pre(const uint8_t *d_table, uint32_t n_shared, te_pre_raw *d_rows, uint32_t *d_flag, hipStream_t st) {
  if (!n_shared) return hipSuccess;
  hipLaunchKernelGGL(k_shared_pre<S>, dim3((n_shared + 127) / 128), dim3(128), 0, st, d_table, n_shared, (te_pre *)d_rows, d_flag);
  return hipGetLastError();
}
template <class S> void SharedOps<S>::thin_terms(const BatchDev &b, const Seed64 &seed, uint64_t j0, const uint32_t *d_c, const uint32_t *d_z, const SharedPlan &p,
                                                 uint32_t tot_io, uint32_t *d_scratch, uint32_t *d_scalars, te_pre_raw *d_pre, uint32_t *d_gpart, hipStream_t st) {
  if (!b.n) return;
  const uint32_t nl = (uint32_t)shared_lanes(p.n_contrib), t0 = b.n + tot_io;
  uint32_t *contrib = d_scratch, *part = contrib + 8 * (size_t)p.n_contrib, *tail_row = part + 16 * (size_t)nl;
  dim3 g((b.n + 127) / 128), blk(128);
  hipLaunchKernelGGL(k_thin_terms_shared<S>, g, blk, 0, st, b, seed, j0, d_c, d_z, p.pos, contrib, d_scalars, (te_pre *)d_pre, d_gpart);
  const uint32_t work = nl > p.n_shared ? nl : p.n_shared;
  hipLaunchKernelGGL(k_shared_lanes<S>, dim3((work + 255) / 256), dim3(256), 0, st, p, contrib, part, tail_row, d_scalars, (te_pre *)d_pre, t0);
  const int by_row = p.n_shared <= nl;
  const uint32_t units = by_row ? p.n_shared : nl;
  hipLaunchKernelGGL(k_shared_merge<S>, dim3((units + 3) / 4 + 1), dim3(256), 0, st, p, part, tail_row, units, by_row, d_gpart, g.x, d_scalars, (te_pre *)d_pre, t0);
}
template <class S> void SharedOps<S>::ped_terms(const BatchDev &b, const Seed64 &seed, uint64_t j0, const uint32_t *d_c, const uint8_t *d_merged, const SharedPlan &p,
                                                uint32_t *d_scratch, uint32_t *d_scalars, te_pre_raw *d_pre, uint32_t *d_gpart, hipStream_t st) {
  if (!b.n) return;
  const uint32_t nl = (uint32_t)shared_lanes(p.n_contrib), t0 = 4 * b.n;
  uint32_t *contrib = d_scratch, *part = contrib + 8 * (size_t)p.n_contrib, *tail_row = part + 16 * (size_t)nl;
  dim3 g((b.n + 127) / 128), blk(128);
  hipLaunchKernelGGL(k_ped_terms_shared<S>, g, blk, 0, st, b, seed, j0, d_c, d_merged, p.pos, contrib, d_scalars, (te_pre *)d_pre, d_gpart, d_gpart + 8 * (size_t)g.x);
  const uint32_t work = nl > p.n_shared ? nl : p.n_shared;
  if (work) hipLaunchKernelGGL(k_shared_lanes<S>, dim3((work + 255) / 256), dim3(256), 0, st, p, contrib, part, tail_row, d_scalars, (te_pre *)d_pre, t0);
  const int by_row = p.n_shared <= nl;
  const uint32_t units = by_row ? p.n_shared : nl;
  hipLaunchKernelGGL((k_shared_merge<S, 2>), dim3((units + 3) / 4 + 2), dim3(256), 0, st, p, part, tail_row, units, by_row, d_gpart, g.x, d_scalars, (te_pre *)d_pre, t0);
}
// what the two segmented launchers share behind their terms kernel: the (segment, row) sums into the segments' row terms (t0 = 0: the
// plan names the terms), then every segment's base term(s)
template <class S, int NBASE>
static void seg_row_sums(const SharedPlan &p, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t n, uint32_t *d_scratch, const uint32_t *d_wsz,
                         uint32_t *d_scalars, te_pre_raw *d_pre, hipStream_t st) {
  const uint32_t nl = (uint32_t)shared_lanes(p.n_contrib);
  uint32_t *contrib = d_scratch, *part = contrib + 8 * (size_t)p.n_contrib, *tail_row = part + 16 * (size_t)nl;
  const uint32_t work = nl > p.n_shared ? nl : p.n_shared;
  hipLaunchKernelGGL(k_shared_lanes<S>, dim3((work + 255) / 256), dim3(256), 0, st, p, contrib, part, tail_row, d_scalars, (te_pre *)d_pre, 0u);
  const int by_row = p.n_shared <= nl;
  const uint32_t units = by_row ? p.n_shared : nl;
  if (units) hipLaunchKernelGGL((k_shared_merge<S, 0>), dim3((units + 3) / 4), dim3(256), 0, st, p, part, tail_row, units, by_row, (const uint32_t *)nullptr, 0u,
                                d_scalars, (te_pre *)d_pre, 0u);
  hipLaunchKernelGGL((k_shared_seg_base<S, NBASE>), dim3(n_seg), dim3(256), 0, st, d_seg_off, p.seg_row0, p.table_rows, n, d_wsz, d_scalars, (te_pre *)d_pre);
}
template <class S> void SharedOps<S>::thin_seg_terms(const BatchDev &b, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t L, const Seed64 *d_seeds, const uint32_t *d_c,
                                                     const uint32_t *d_z, const SharedPlan &p, uint32_t *d_scratch, uint32_t *d_wsz, uint32_t *d_scalars,
                                                     te_pre_raw *d_pre, hipStream_t st) {
  if (!b.n || !n_seg) return;
  hipLaunchKernelGGL(k_thin_terms_shared_seg<S>, dim3((b.n + 127) / 128), dim3(128), 0, st, b, d_seg_off, n_seg, L, d_seeds, d_c, d_z, p.pos, d_scratch, d_wsz,
                     d_scalars, (te_pre *)d_pre);
  seg_row_sums<S, 1>(p, d_seg_off, n_seg, b.n, d_scratch, d_wsz, d_scalars, d_pre, st);
}
template <class S> void SharedOps<S>::ped_seg_terms(const BatchDev &b, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t L, const Seed64 *d_seeds, const uint32_t *d_c,
                                                    const uint8_t *d_merged, const SharedPlan &p, uint32_t *d_scratch, uint32_t *d_wsz, uint32_t *d_scalars,
                                                    te_pre_raw *d_pre, hipStream_t st) {
  if (!b.n || !n_seg) return;
  hipLaunchKernelGGL(k_ped_terms_shared_seg<S>, dim3((b.n + 127) / 128), dim3(128), 0, st, b, d_seg_off, n_seg, L, d_seeds, d_c, d_merged, p.pos, d_scratch, d_wsz,
                     d_scalars, (te_pre *)d_pre);
  seg_row_sums<S, 2>(p, d_seg_off, n_seg, b.n, d_scratch, d_wsz, d_scalars, d_pre, st);
}
template struct SharedOps<suite_by_id<AVRF_TU_SUITE>::type>;

}  // namespace avrf
