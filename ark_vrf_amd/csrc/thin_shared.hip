// thin_shared.hip -- the device side of thin::BatchVerifier over a table of shared points (thin_shared.h).
//
//   k_shared_gather / _scan / _place : staging -- the plain staged layout from the table, and the counting sort of the
//                                      n + tot_io references by row (32-bit integer atomics on counters only)
//   k_shared_pre                     : every table row once to te_pre, through the suite's own te_make_pre
//   k_thin_terms_shared              : k_thin_terms (vrf_batch.hip; src/thin.rs:287-313) without the key and input terms:
//                                      their scalars go to contrib[pos[.]] in Montgomery form
//   k_shared_lanes / k_shared_merge  : the segmented sum of contrib in Fr -> the T row terms; the generator term (src/thin.rs:303,316-317)
// One lane per item / reference / share; scalar-field sums in 8 x u32 Montgomery form (fp256.h).
#include "thin_shared.h"
#include "proto_dev.h"
#include "batch_terms_dev.h"

// Built once per suite (-DAVRF_TU_SUITE=<id>, csrc/Makefile): the suite's kernels and the explicit instantiation of SharedOps<S>,
// which capi.hip reaches through AVRF_SHARED.  The suite-independent staging kernels live in suite 0's unit.
#ifndef AVRF_TU_SUITE
#error "thin_shared.hip is built once per suite: -DAVRF_TU_SUITE=<id> (csrc/Makefile)"
#endif
namespace avrf {

#if AVRF_TU_SUITE == 0
// ---------------------------------------------------------------- staging: gather and plan

// ctr[r] += 1 for every active lane, returning the value each lane's own increment saw.  References crowd on few rows (a handful of
// inputs, one key), and same-address atomics serialise: the lanes of a wave that name the row of the wave's first pending lane are
// counted with ONE atomic, four times over; what is still pending after that (rows that differ lane by lane) goes one by one.
AVRF_DI uint32_t wave_count(uint32_t *ctr, uint32_t r, bool active) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t slot = 0;
  bool todo = active;
  for (int round = 0; round < 4; round++) {
    const unsigned long long pending = __ballot(todo);
    if (!pending) break;                                                // (wave-uniform)
    const int leader = __ffsll(pending) - 1;
    const uint32_t key = __shfl(r, leader);
    const bool mine = todo && r == key;
    const unsigned long long m = __ballot(mine);
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(ctr + key, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    if (mine) { slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1)); todo = false; }
  }
  if (todo) slot = atomicAdd(ctr + r, 1u);
  return slot;
}

// reference t: item t's key (t < n) or the input of I/O pair t - n.  Copies the row (and the pair's output) into the plain staged
// layout and counts the reference of its row.
__global__ void __launch_bounds__(256)
k_shared_gather(const uint8_t *__restrict__ table, uint32_t n_shared, const uint32_t *__restrict__ idx, const uint8_t *__restrict__ outs,
                uint32_t n, uint32_t tot_io, uint8_t *__restrict__ pks, uint8_t *__restrict__ ios, uint32_t *__restrict__ cnt) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n + tot_io;
  uint32_t r = active ? idx[t] : 0;
  if (r >= n_shared) r = n_shared - 1;                                  // (refused on the host; never a read outside the table)
  wave_count(cnt, r, active);
  if (!active) return;
  const uint4 *src = reinterpret_cast<const uint4 *>(table + 64 * (size_t)r);
  uint4 *dst = reinterpret_cast<uint4 *>(t < n ? pks + 64 * (size_t)t : ios + 128 * (size_t)(t - n));
#pragma unroll
  for (int i = 0; i < 4; i++) dst[i] = src[i];
  if (t >= n) {
    const uint4 *o = reinterpret_cast<const uint4 *>(outs + 64 * (size_t)(t - n));
#pragma unroll
    for (int i = 0; i < 4; i++) dst[4 + i] = o[i];
  }
}

// exclusive prefix sums of the counts (one block; every thread a contiguous chunk): row_off[0 .. T], and the counts replaced by
// the same offsets as the placement's cursors
__global__ void __launch_bounds__(1024)
k_shared_scan(uint32_t *__restrict__ cursor, uint32_t *__restrict__ row_off, uint32_t n_shared) {
  __shared__ uint32_t sums[1024];
  const uint32_t tid = threadIdx.x, chunk = (n_shared + 1023) / 1024;
  const uint32_t lo = tid * chunk < n_shared ? tid * chunk : n_shared, hi = lo + chunk < n_shared ? lo + chunk : n_shared;
  uint32_t s = 0;
  for (uint32_t i = lo; i < hi; i++) s += cursor[i];
  sums[tid] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t v = tid >= d ? sums[tid - d] : 0;
    __syncthreads();
    sums[tid] += v;
    __syncthreads();
  }
  uint32_t base = sums[tid] - s;
  for (uint32_t i = lo; i < hi; i++) { const uint32_t c = cursor[i]; row_off[i] = base; cursor[i] = base; base += c; }
  if (tid == 1023) row_off[n_shared] = sums[1023];
}

__global__ void __launch_bounds__(256)
k_shared_place(const uint32_t *__restrict__ idx, uint32_t n_shared, uint32_t n_contrib, uint32_t *__restrict__ cursor,
               uint32_t *__restrict__ pos, uint32_t *__restrict__ slot_row) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = t < n_contrib;
  uint32_t r = active ? idx[t] : 0;
  if (r >= n_shared) r = n_shared - 1;
  const uint32_t s = wave_count(cursor, r, active);                     // < row_off[r + 1] <= n_contrib: the same references were counted
  if (active) { pos[t] = s; slot_row[s] = r; }
}

hipError_t shared_plan(const uint8_t *d_table, uint32_t n_shared, const uint32_t *d_idx, const uint8_t *d_outputs, uint32_t n, uint32_t tot_io,
                       uint8_t *d_pks, uint8_t *d_ios, uint32_t *d_plan, hipStream_t st) {
  const uint32_t nc = n + tot_io;
  if (!nc || !n_shared) return hipSuccess;
  uint32_t *cursor = d_plan, *row_off = d_plan + (n_shared + 1), *pos = row_off + (n_shared + 1), *slot_row = pos + nc;
  if (hipError_t e = hipMemsetAsync(cursor, 0, (size_t)(n_shared + 1) * 4, st)) return e;
  hipLaunchKernelGGL(k_shared_gather, dim3((nc + 255) / 256), dim3(256), 0, st, d_table, n_shared, d_idx, d_outputs, n, tot_io, d_pks, d_ios, cursor);
  hipLaunchKernelGGL(k_shared_scan, dim3(1), dim3(1024), 0, st, cursor, row_off, n_shared);
  hipLaunchKernelGGL(k_shared_place, dim3((nc + 255) / 256), dim3(256), 0, st, d_idx, n_shared, nc, cursor, pos, slot_row);
  return hipGetLastError();                                             // (a launch that was refused)
}
#endif  // AVRF_TU_SUITE == 0

// ---------------------------------------------------------------- per suite

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


// The per-item arithmetic of k_thin_terms: weights from the seed or from b.weights, j0, the block sum of w s into gpart.  Item j
// emits (R_j, w_j) at j + io0 and (O_i, w c z_i) at j + io0 + 1 + i; w c (its key's row) and -w s z_i (its inputs' rows) go to contrib.
template <class S>
__global__ void __launch_bounds__(128)
k_thin_terms_shared(BatchDev b, Seed64 seed, uint64_t j0, const uint32_t *__restrict__ c_in, const uint32_t *__restrict__ z_in,
                    const uint32_t *__restrict__ pos, uint32_t *__restrict__ contrib, uint32_t *__restrict__ scalars,
                    te_pre *__restrict__ pre, uint32_t *__restrict__ gpart) {
  using Fr = typename S::Fr;
  __shared__ fp red[128];
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  fp ws = fp_zero();
  if (j < b.n) {
    uint32_t io0 = b.io_off[j], m = b.io_off[j + 1] - io0;
    uint64_t gj = j0 + j;
    uint32_t ww[4];
    if (b.weights) { const uint4 v = *reinterpret_cast<const uint4 *>(b.weights + 16 * (size_t)j); ww[0] = v.x; ww[1] = v.y; ww[2] = v.z; ww[3] = v.w; }
    else { uint64_t blk[8]; sha512_xof_block(seed.w, gj >> 2, blk); digest_le128(blk, (int)(gj & 3), ww); }
    fp w_plain = fp_zero(); w_plain.v[0] = ww[0]; w_plain.v[1] = ww[1]; w_plain.v[2] = ww[2]; w_plain.v[3] = ww[3];
    fp w = fp_to_mont<Fr>(w_plain);
    fp c = fp_to_mont<Fr>(fp_from_u128(c_in + 4 * (size_t)j));
    const uint8_t *pr = b.proofs + 96 * (size_t)j;
    fp s = fp_to_mont<Fr>(fp_load_le(pr + 64));
    fp wc = fp_mul<Fr>(w, c);                               // thin.rs:291-292
    ws = fp_mul<Fr>(w, s);
    uint32_t t = j + io0;
    emit_term<S>(scalars, pre, t, w_plain, pr);                                           // (R_j, w_j)        :295-296
    fp_store(contrib + 8 * (size_t)pos[j], wc);                                           // (pk_j, w c z0)    :299-300, z0 = 1
    for (uint32_t i = 0; i < m; i++) {                                                    // :306-312
      fp z = fp_to_mont<Fr>(fp_from_u128(z_in + 4 * (size_t)(io0 + i)));
      const uint8_t *p = b.ios_xy + 128 * (size_t)(io0 + i);
      emit_term<S>(scalars, pre, t + 1 + i, fp_from_mont<Fr>(fp_mul<Fr>(wc, z)), p + 64);              // (O_i, w c z_i)
      fp_store(contrib + 8 * (size_t)pos[b.n + io0 + i], fp_neg<Fr>(fp_mul<Fr>(ws, z)));               // (I_i, -w s z_i)
    }
  }
  // block sum of w_j s_j z0 (Montgomery form), thin.rs:303
  red[threadIdx.x] = ws;
  __syncthreads();
  for (int s2 = 64; s2 >= 1; s2 >>= 1) {
    if ((int)threadIdx.x < s2) red[threadIdx.x] = fp_add<Fr>(red[threadIdx.x], red[threadIdx.x + s2]);
    __syncthreads();
  }
  if (threadIdx.x == 0) fp_store(gpart + 8 * (size_t)blockIdx.x, red[0]);
}

enum : uint32_t { SHARED_NO_ROW = 0xffffffffu };

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
  for (uint32_t r = gid; r < p.n_shared; r += nth) {
    store_pre(pre + t0 + r, load_pre(reinterpret_cast<const te_pre *>(p.rows) + r));
    if (p.row_off[r] == p.row_off[r + 1]) fp_store(scalars + 8 * (size_t)(t0 + r), fp_zero());
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
      if (starts_here && ends_here) fp_store(scalars + 8 * (size_t)(t0 + r), fp_from_mont<Fr>(acc));
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
// units.  The last block sums the partials of w s into the generator term, as k_g_final does.
template <class S>
__global__ void __launch_bounds__(256)
k_shared_merge(SharedPlan p, const uint32_t *__restrict__ part, const uint32_t *__restrict__ tail_row, uint32_t n_units, int by_row,
               const uint32_t *__restrict__ gpart, uint32_t nparts, uint32_t *__restrict__ scalars, te_pre *__restrict__ pre, uint32_t t0) {
  using Fr = typename S::Fr; using Fq = typename S::Fq;
  __shared__ fp red[256];
  const uint32_t tid = threadIdx.x;
  if (blockIdx.x == gridDim.x - 1) {                                    // g = -(sum of partials); last term (G, g)
    fp acc = fp_zero();
    for (uint32_t i = tid; i < nparts; i += 256) acc = fp_add<Fr>(acc, fp_load(gpart + 8 * (size_t)i));
    red[tid] = acc;
    __syncthreads();
#pragma unroll 1                                                        // (unrolled, the tree's eight masked additions spill SGPRs)
    for (int s2 = 128; s2 >= 1; s2 >>= 1) {
      if ((int)tid < s2) red[tid] = fp_add<Fr>(red[tid], red[tid + s2]);
      __syncthreads();
    }
    if (tid == 0) {
      const uint32_t t_last = t0 + p.n_shared;
      fp_store(scalars + 8 * (size_t)t_last, fp_from_mont<Fr>(fp_neg<Fr>(red[0])));
      te_pre g; g.x = fp_const<Fq>(S::G_X); g.y = fp_const<Fq>(S::G_Y); g.k = fp_const<Fq>(S::G_K);
      store_pre(pre + t_last, g);
    }
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
    red[tid] = acc;
    __syncthreads();
#pragma unroll 1                                                        // (unrolled, the tree's eight masked additions spill SGPRs)
    for (int s2 = 128; s2 >= 1; s2 >>= 1) {
      if ((int)tid < s2) red[tid] = fp_add<Fr>(red[tid], red[tid + s2]);
      __syncthreads();
    }
    if (tid == 0) fp_store(scalars + 8 * (size_t)(t0 + r), fp_from_mont<Fr>(red[0]));
    __syncthreads();                                                    // red is reused by the next unit
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
template struct SharedOps<suite_by_id<AVRF_TU_SUITE>::type>;

}  // namespace avrf
