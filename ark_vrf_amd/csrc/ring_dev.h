// ring_dev.h -- the device layer of the ring prover (ring.hip holds the host side): the NTT over Fr of the pairing curve, the constraint
// aggregation on the 4N domain, quotient, evaluations, linearisation and opening quotients (k_ring_*), the witness accumulation
// (k_ring_witness_acc) and the small kernels of index and the Lagrange-basis build.  DESIGN.md section 4, section 7.
#pragma once
#include "te.h"
#include "te_quad.h"
#include <string.h>

namespace avrf {

// ------------------------------------------------------------------------------------------------
// device NTT over Fr of the pairing curve (radix-2, stages fused through LDS; batch of equal sizes);
// tw[k] = w^k (Montgomery), k < n/2

template <class F>
__global__ void k_ntt_bitrev(uint32_t *__restrict__ data, uint32_t n, int logn, uint32_t batch) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t b = t / n, i = t - b * n;
  if (b >= batch) return;
  uint32_t j = __brev(i) >> (32 - logn);
  if (i < j) {
    uint32_t *p = data + ((size_t)b * n + i) * 8, *q = data + ((size_t)b * n + j) * 8;
    fp x = fp_load(p), y = fp_load(q);
    fp_store(p, y); fp_store(q, x);
  }
}
template <class F>
__global__ void k_ntt_scale(uint32_t *__restrict__ data, uint32_t total, fp k) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  uint32_t *p = data + (size_t)t * 8;
  fp_store(p, fp_mul<F>(fp_load(p), k));
}

// Up to 8 consecutive butterfly stages [s0, s1) on a tile held in LDS: 2^(s1-s0) rows with row stride 2^s0 elements
// times 2^cols_log adjacent columns (<= 256 elements, whole 128-byte lines when s0 > 0).  A size-2^13 transform is
// 2 passes over HBM instead of 13.  brev_load: the tile is gathered from the bit-reversed positions of `src` (another
// buffer, `src_n` <= n valid elements per vector, the rest read as zero -- zero-extension of a shorter coefficient
// vector costs nothing); otherwise src == dst is read in place.  do_scale: multiply by `scale` on the way out.
template <class F>
__global__ void __launch_bounds__(128)
k_ntt_fused(const uint32_t *__restrict__ src, uint32_t src_n, uint32_t *__restrict__ dst, uint32_t n, int logn, int s0, int s1, uint32_t cols_log,
            const uint32_t *__restrict__ tw, int brev_load, fp scale, int do_scale) {
  __shared__ uint32_t sh[256 * 8];
  const uint32_t cols = 1u << cols_log, tile = (1u << (s1 - s0)) << cols_log;
  const uint32_t tiles_per_vec = n / tile, b = blockIdx.x / tiles_per_vec, t = blockIdx.x - b * tiles_per_vec;
  const uint32_t low_groups = (1u << s0) >> cols_log;
  const uint32_t hi = t / low_groups, lo = t - hi * low_groups;
  const uint32_t base = (hi << s1) + (lo << cols_log);
  for (uint32_t e = threadIdx.x; e < tile; e += blockDim.x) {
    const uint32_t i = base + ((e >> cols_log) << s0) + (e & (cols - 1));
    fp v;
    if (brev_load) { const uint32_t j = __brev(i) >> (32 - logn); v = j < src_n ? fp_load(src + ((size_t)b * src_n + j) * 8) : fp_zero(); }
    else v = fp_load(src + ((size_t)b * n + i) * 8);
    fp_store(sh + e * 8, v);
  }
  __syncthreads();
  // (the twiddles are read from global memory inside the butterflies: preloading the tile - cols <= 255 twiddles of a pass into a
  // second 8 KB of LDS measured slower -- 559 us against 400 us per launch in the 2 048-proof profile, proofs/s unchanged)
  for (int s = s0; s < s1; s++) {
    const int hl = s - s0;                                             // half = 2^hl rows
    for (uint32_t j = threadIdx.x; j < tile / 2; j += blockDim.x) {
      const uint32_t c = j & (cols - 1), jr = j >> cols_log;
      const uint32_t grp = jr >> hl, pos = jr & ((1u << hl) - 1);
      const uint32_t r0 = (grp << (hl + 1)) + pos, r1 = r0 + (1u << hl);
      const uint32_t pg = (pos << s0) + (lo << cols_log) + c;          // position inside the stage's global group
      const fp w = fp_load(tw + ((size_t)pg << (logn - 1 - s)) * 8);
      uint32_t *p = sh + ((r0 << cols_log) + c) * 8, *q = sh + ((r1 << cols_log) + c) * 8;
      const fp u = fp_load(p), v = fp_mul<F>(fp_load(q), w);
      fp_store(p, fp_add<F>(u, v)); fp_store(q, fp_sub<F>(u, v));
    }
    __syncthreads();
  }
  for (uint32_t e = threadIdx.x; e < tile; e += blockDim.x) {
    const uint32_t i = base + ((e >> cols_log) << s0) + (e & (cols - 1));
    fp v = fp_load(sh + e * 8);
    if (do_scale) v = fp_mul<F>(v, scale);
    fp_store(dst + ((size_t)b * n + i) * 8, v);
  }
}

// (i)NTT of `batch` vectors of size n (tw = powers of the root or of its inverse; scale = 1/n for the inverse).
// src == dst: in place (a bit-reversal pass first).  Otherwise dst = NTT(zero-extended src), src vectors of src_n <= n.
template <class F>
static void ntt_launch2(const uint32_t *d_src, uint32_t src_n, uint32_t *d_dst, uint32_t n, const uint32_t *d_tw, uint32_t batch, const fp *scale, hipStream_t st) {
  int logn = 0; while ((1u << logn) < n) logn++;
  const bool inplace = d_src == d_dst;
  if (inplace) hipLaunchKernelGGL(k_ntt_bitrev<F>, dim3(((size_t)n * batch + 255) / 256), dim3(256), 0, st, d_dst, n, logn, batch);
  fp one; memset(&one, 0, sizeof one);
  for (int s0 = 0; s0 < logn;) {
    int s1 = s0 + 8 < logn ? s0 + 8 : logn;
    if (s1 < logn && logn - s1 < 3) s1 = logn - 3 > s0 ? logn - 3 : s1;   // keep the last pass at >= 3 stages
    uint32_t cols_log = 8 - (uint32_t)(s1 - s0); if ((int)cols_log > s0) cols_log = (uint32_t)s0;
    const uint32_t tile = (1u << (s1 - s0)) << cols_log;
    const bool last = s1 == logn;
    hipLaunchKernelGGL(k_ntt_fused<F>, dim3((unsigned)((size_t)(n / tile) * batch)), dim3(tile / 2 < 128 ? (tile / 2 ? tile / 2 : 1) : 128), 0, st,
                       (s0 == 0 && !inplace) ? d_src : (const uint32_t *)d_dst, src_n, d_dst, n, logn, s0, s1, cols_log, d_tw,
                       (s0 == 0 && !inplace) ? 1 : 0, (last && scale) ? *scale : one, (last && scale) ? 1 : 0);
    s0 = s1;
  }
}
template <class F>
static void ntt_launch(uint32_t *d_data, uint32_t n, const uint32_t *d_tw, uint32_t batch, const fp *scale, hipStream_t st) {
  ntt_launch2<F>(d_data, n, d_data, n, d_tw, batch, scale, st);
}

// ------------------------------------------------------------------------------------------------
// PIOP constraint aggregation on the 4N domain: one lane per domain point.
// e4 = evaluations of bits | ip_acc | acc_x | acc_y (4 x M), fixed4 = points.x | points.y | selector
// (3 x M), l4 = L_first | L_last (2 x M), tw4[k] = w4^k (k < M/2; w4^(M/2) = -1).
struct RingConsts { fp alpha[7]; fp w_last, seedx, seedy, resx, resy; };

template <class S>
__global__ void __launch_bounds__(256)
k_ring_constraints(const uint32_t *__restrict__ e4, const uint32_t *__restrict__ fixed4, const uint32_t *__restrict__ l4,
                   const uint32_t *__restrict__ tw4, const RingConsts *__restrict__ consts, uint32_t M, uint32_t *__restrict__ out) {
  using F = typename S::Fq;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const uint32_t proof = blockIdx.y;                                  // one proof per grid row
  e4 += (size_t)proof * 4 * M * 8; out += (size_t)proof * M * 8;
  const RingConsts &c = consts[proof];
  const uint32_t is = (i + 4) & (M - 1);                              // column(wX) on the 4N domain
  auto at = [&](const uint32_t *base, uint32_t col, uint32_t idx) { return fp_load(base + ((size_t)col * M + idx) * 8); };
  const fp one = fp_one<F>();
  const fp b = at(e4, 0, i), ip = at(e4, 1, i), x1 = at(e4, 2, i), y1 = at(e4, 3, i);
  const fp ips = at(e4, 1, is), x3 = at(e4, 2, is), y3 = at(e4, 3, is);
  const fp x2 = at(fixed4, 0, i), y2 = at(fixed4, 1, i), sel = at(fixed4, 2, i);
  const fp lf = at(l4, 0, i), ll = at(l4, 1, i);
  fp xi = fp_load(tw4 + (size_t)(i & (M / 2 - 1)) * 8);
  if (i >= M / 2) xi = fp_neg<F>(xi);
  const fp nl = fp_sub<F>(xi, c.w_last), omb = fp_sub<F>(one, b);
  const fp x1y1 = fp_mul<F>(x1, y1), x2y2 = fp_mul<F>(x2, y2);
  fp c0 = fp_mul<F>(fp_sub<F>(fp_sub<F>(ips, ip), fp_mul<F>(sel, b)), nl);
  fp t1 = fp_add<F>(fp_mul<F>(y1, y2), mul_a<S>(fp_mul<F>(x1, x2)));
  fp c1 = fp_mul<F>(fp_add<F>(fp_mul<F>(b, fp_sub<F>(fp_sub<F>(fp_mul<F>(x3, t1), x1y1), x2y2)), fp_mul<F>(omb, fp_sub<F>(x3, x1))), nl);
  fp t2 = fp_sub<F>(fp_mul<F>(x1, y2), fp_mul<F>(x2, y1));
  fp c2 = fp_mul<F>(fp_add<F>(fp_mul<F>(b, fp_add<F>(fp_sub<F>(fp_mul<F>(y3, t2), x1y1), x2y2)), fp_mul<F>(omb, fp_sub<F>(y3, y1))), nl);
  fp c3 = fp_mul<F>(b, omb);
  fp c4 = fp_add<F>(fp_mul<F>(lf, fp_sub<F>(x1, c.seedx)), fp_mul<F>(ll, fp_sub<F>(x1, c.resx)));
  fp c5 = fp_add<F>(fp_mul<F>(lf, fp_sub<F>(y1, c.seedy)), fp_mul<F>(ll, fp_sub<F>(y1, c.resy)));
  fp c6 = fp_add<F>(fp_mul<F>(lf, ip), fp_mul<F>(ll, fp_sub<F>(ip, one)));
  fp s = fp_mul<F>(c.alpha[0], c0);
  s = fp_add<F>(s, fp_mul<F>(c.alpha[1], c1)); s = fp_add<F>(s, fp_mul<F>(c.alpha[2], c2)); s = fp_add<F>(s, fp_mul<F>(c.alpha[3], c3));
  s = fp_add<F>(s, fp_mul<F>(c.alpha[4], c4)); s = fp_add<F>(s, fp_mul<F>(c.alpha[5], c5)); s = fp_add<F>(s, fp_mul<F>(c.alpha[6], c6));
  fp_store(out + (size_t)i * 8, s);
}


// ------------------------------------------------------------------------------------------------
// per-proof polynomial rounds of the prover on the device; grid.y / blockIdx = proof.
// All vectors are Montgomery Fr, 8 words per element.

struct Fp3 { fp v[3]; };

template <class F> AVRF_DI fp fp_pow_u32(fp a, uint32_t e) {
  fp r = fp_one<F>();
  while (e) { if (e & 1) r = fp_mul<F>(r, a); e >>= 1; if (e) a = fp_sqr<F>(a); }
  return r;
}
// sum over the 256 lanes of a workgroup (sh: 256 x 8 words); result valid in every lane
template <class F> AVRF_DI fp block_sum256(fp v, uint32_t *sh) {
  const uint32_t t = threadIdx.x;
  __syncthreads();
  fp_store(sh + t * 8, v);
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (t < s) fp_store(sh + t * 8, fp_add<F>(fp_load(sh + t * 8), fp_load(sh + (t + s) * 8)));
    __syncthreads();
  }
  return fp_load(sh);
}
// value at x of the length-len polynomial c: lane t takes coefficients [t*L, (t+1)*L)
template <class F> AVRF_DI fp block_eval256(const uint32_t *c, uint32_t len, const fp &x, uint32_t *sh) {
  const uint32_t t = threadIdx.x, L = (len + 255) / 256;
  uint32_t lo = t * L, hi = lo + L; if (hi > len) hi = len;
  fp h = fp_zero();
  for (uint32_t i = hi; i > lo; i--) h = fp_add<F>(fp_mul<F>(h, x), fp_load(c + (size_t)(i - 1) * 8));
  if (lo < hi) h = fp_mul<F>(h, fp_pow_u32<F>(x, lo));
  return block_sum256<F>(h, sh);
}

// quotient: q = agg * Z / (X^N - 1) with Z = X^3 + z2 X^2 + z1 X + z0 (the three zk rows), agg of length M = 4N:
// t[k] = sum_m z[m] agg[k-m];  q[i] = sum_{j >= 1} t[i + jN]   (exact division: the remainder is zero)
template <class F>
__global__ void __launch_bounds__(256)
k_ring_quotient(const uint32_t *__restrict__ agg, uint32_t N, uint32_t qlen, Fp3 z, uint32_t *__restrict__ q) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, M = 4 * N;
  if (i >= qlen) return;
  const uint32_t *a = agg + (size_t)blockIdx.y * M * 8;
  fp acc = fp_zero();
  for (uint32_t k = i + N; k <= M + 2; k += N) {
    if (k < M) acc = fp_add<F>(acc, fp_mul<F>(z.v[0], fp_load(a + (size_t)k * 8)));
    if (k >= 1 && k - 1 < M) acc = fp_add<F>(acc, fp_mul<F>(z.v[1], fp_load(a + (size_t)(k - 1) * 8)));
    if (k >= 2 && k - 2 < M) acc = fp_add<F>(acc, fp_mul<F>(z.v[2], fp_load(a + (size_t)(k - 2) * 8)));
    if (k >= 3 && k - 3 < M) acc = fp_add<F>(acc, fp_load(a + (size_t)(k - 3) * 8));
  }
  fp_store(q + ((size_t)blockIdx.y * qlen + i) * 8, acc);
}

// ev[proof][c] = poly_c(zeta_proof), c: px | py | sel (fixed, shared) | bits | ip | ax | ay (coef: proof x 4 x N)
template <class F>
__global__ void __launch_bounds__(256)
k_ring_evals(const uint32_t *__restrict__ coef, const uint32_t *__restrict__ fixed, const uint32_t *__restrict__ zeta, uint32_t N,
             uint32_t *__restrict__ ev) {
  __shared__ uint32_t sh[256 * 8];
  const uint32_t c = blockIdx.x, p = blockIdx.y;
  const uint32_t *poly = c < 3 ? fixed + (size_t)c * N * 8 : coef + ((size_t)p * 4 + (c - 3)) * N * 8;
  fp v = block_eval256<F>(poly, N, fp_load(zeta + (size_t)p * 8), sh);
  if (threadIdx.x == 0) fp_store(ev + ((size_t)p * 7 + c) * 8, v);
}

// linearisation polynomial lin = f0 ip + f1 ax + f2 ay (f from the evaluations, A.7 step 6) and lin(zeta w)
template <class S>
__global__ void __launch_bounds__(256)
k_ring_lin(const uint32_t *__restrict__ coef, const RingConsts *__restrict__ consts, const uint32_t *__restrict__ zeta,
           const uint32_t *__restrict__ ev, fp w, uint32_t N, uint32_t *__restrict__ lin, uint32_t *__restrict__ lin_zw) {
  using F = typename S::Fq;
  __shared__ uint32_t sh[256 * 8];
  const uint32_t p = blockIdx.x, t = threadIdx.x;
  const RingConsts &c = consts[p];
  const uint32_t *e = ev + (size_t)p * 7 * 8;
  const fp z = fp_load(zeta + (size_t)p * 8), one = fp_one<F>();
  const fp x2 = fp_load(e), y2 = fp_load(e + 8), b = fp_load(e + 24), x1 = fp_load(e + 40), y1 = fp_load(e + 48);
  const fp nlz = fp_sub<F>(z, c.w_last), omb = fp_sub<F>(one, b);
  const fp k1 = fp_add<F>(fp_mul<F>(b, fp_add<F>(fp_mul<F>(y1, y2), mul_a<S>(fp_mul<F>(x1, x2)))), omb);
  const fp k2 = fp_add<F>(fp_mul<F>(b, fp_sub<F>(fp_mul<F>(x1, y2), fp_mul<F>(x2, y1))), omb);
  const fp f0 = fp_mul<F>(nlz, c.alpha[0]), f1 = fp_mul<F>(nlz, fp_mul<F>(c.alpha[1], k1)), f2 = fp_mul<F>(nlz, fp_mul<F>(c.alpha[2], k2));
  const uint32_t *ip = coef + ((size_t)p * 4 + 1) * N * 8, *ax = ip + (size_t)N * 8, *ay = ax + (size_t)N * 8;
  uint32_t *out = lin + (size_t)p * N * 8;
  for (uint32_t i = t; i < N; i += 256)
    fp_store(out + (size_t)i * 8, fp_add<F>(fp_add<F>(fp_mul<F>(f0, fp_load(ip + (size_t)i * 8)), fp_mul<F>(f1, fp_load(ax + (size_t)i * 8))),
                                            fp_mul<F>(f2, fp_load(ay + (size_t)i * 8))));
  __syncthreads();
  fp v = block_eval256<F>(out, N, fp_mul<F>(z, w), sh);
  if (t == 0) fp_store(lin_zw + (size_t)p * 8, v);
}

// aggregated opening polynomial at zeta: sum_c nu_c poly_c + nu_7 q   (length qlen; the 7 columns have length N)
template <class F>
__global__ void __launch_bounds__(256)
k_ring_aggz(const uint32_t *__restrict__ coef, const uint32_t *__restrict__ fixed, const uint32_t *__restrict__ q, const uint32_t *__restrict__ nu,
            uint32_t N, uint32_t qlen, uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
  if (i >= qlen) return;
  const uint32_t *nup = nu + (size_t)p * 8 * 8;
  fp acc = fp_mul<F>(fp_load(nup + 7 * 8), fp_load(q + ((size_t)p * qlen + i) * 8));
  if (i < N) {
    for (int c = 0; c < 3; c++) acc = fp_add<F>(acc, fp_mul<F>(fp_load(nup + c * 8), fp_load(fixed + ((size_t)c * N + i) * 8)));
    for (int c = 0; c < 4; c++) acc = fp_add<F>(acc, fp_mul<F>(fp_load(nup + (3 + c) * 8), fp_load(coef + (((size_t)p * 4 + c) * N + i) * 8)));
  }
  fp_store(out + ((size_t)p * qlen + i) * 8, acc);
}

// out = (c(X) - c(z)) / (X - z), z = zs[proof] * zmul: out[i-1] = A_i = c[i] + z A_{i+1}.  Lane t owns indices
// [t*L, (t+1)*L); the carry into a chunk comes from a suffix scan of the chunk values with multiplier z^L.
template <class F>
__global__ void __launch_bounds__(256)
k_ring_divlin(const uint32_t *__restrict__ in, uint32_t in_stride, uint32_t len, const uint32_t *__restrict__ zs, fp zmul,
              uint32_t *__restrict__ out, uint32_t out_stride) {
  __shared__ uint32_t sh[256 * 8];
  const uint32_t p = blockIdx.x, t = threadIdx.x, L = (len + 255) / 256;
  const uint32_t *c = in + (size_t)p * in_stride * 8;
  uint32_t *o = out + (size_t)p * out_stride * 8;
  const fp z = fp_mul<F>(fp_load(zs + (size_t)p * 8), zmul);
  uint32_t lo = t * L, hi = lo + L; if (hi > len) hi = len; if (lo > len) lo = len;
  fp h = fp_zero();
  for (uint32_t i = hi; i > lo; i--) h = fp_add<F>(fp_mul<F>(h, z), fp_load(c + (size_t)(i - 1) * 8));
  // carry[t] = sum_{t' > t} h_{t'} z^(L (t' - t - 1)):  start from h_{t+1}, then Hillis-Steele with z^(L d)
  fp_store(sh + t * 8, h);
  __syncthreads();
  fp A = t + 1 < 256 ? fp_load(sh + (t + 1) * 8) : fp_zero();
  fp mul = fp_pow_u32<F>(z, L);
  for (uint32_t d = 1; d < 256; d <<= 1) {
    __syncthreads();
    fp_store(sh + t * 8, A);
    __syncthreads();
    if (t + d < 256) A = fp_add<F>(A, fp_mul<F>(mul, fp_load(sh + (t + d) * 8)));
    mul = fp_sqr<F>(mul);
  }
  for (uint32_t i = hi; i > lo; i--) {
    A = fp_add<F>(fp_load(c + (size_t)(i - 1) * 8), fp_mul<F>(A, z));
    if (i >= 2) fp_store(o + (size_t)(i - 2) * 8, A);
  }
}

// Witness columns from their sparse description (A.7 step 1): pos = sorted rows with bit 1 (<= 256 per proof,
// padded), vals = the cnt+1 successive accumulator points (x | y), kidx = the signer's row, zk = the values of the
// last 3 rows of each column (proof x 4 x 3; nullptr: zeros).  cols[proof] = bits | ip | ax | ay (4 x N evaluations).
template <class F>
__global__ void __launch_bounds__(256)
k_ring_witness_cols(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ kidx,
                    const uint32_t *__restrict__ vals, const uint32_t *__restrict__ zk, uint32_t N, uint32_t cap, uint32_t *__restrict__ cols) {
  __shared__ uint32_t sp[256];
  const uint32_t p = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  sp[threadIdx.x] = pos[(size_t)p * 256 + threadIdx.x];
  __syncthreads();
  if (i >= N) return;
  const uint32_t m = cnt[p], ki = kidx[p];
  uint32_t lo = 0, hi = m;                               // r = number of pos < i
  while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (sp[mid] < i) lo = mid + 1; else hi = mid; }
  const bool bit = lo < m && sp[lo] == i;
  const fp one = fp_one<F>(), zero = fp_zero();
  uint32_t *c = cols + (size_t)p * 4 * N * 8;
  if (i >= cap) {                                          // the 3 zero-knowledge rows: random when hiding, else zero
    for (int col = 0; col < 4; col++)
      fp_store(c + ((size_t)col * N + i) * 8, zk ? fp_load(zk + (((size_t)p * 4 + col) * 3 + (i - cap)) * 8) : zero);
    return;
  }
  fp_store(c + (size_t)i * 8, bit ? one : zero);
  fp_store(c + ((size_t)N + i) * 8, i > ki ? one : zero);
  const uint32_t *v = vals + ((size_t)p * 257 + lo) * 16;
  fp_store(c + ((size_t)2 * N + i) * 8, fp_load(v));
  fp_store(c + ((size_t)3 * N + i) * 8, fp_load(v + 8));
}
// RingProver round 0 on the device (A.7 step 1; w3f-ring-proof `PiopProver::build`): the witness in sparse form.  One lane per
// proof.  Rows with bit 1: the signer's key, then the set bits of the blinding (row keyset + i).  The accumulator column only
// changes there: acc_0 = seed, acc_{j+1} = acc_j + point[pos_j] on the suite's twisted-Edwards curve (mixed additions, the ring's
// points tabulated as te_pre at index time), all m + 1 <= 255 partial sums normalised with ONE inversion (Montgomery's trick over
// the lane's own chain; the extended points and prefix products live in `scratch`, 257 x 160 bytes per proof).  Written: the row
// list and count, the affine partial sums (k_ring_witness_cols expands them into the columns), the four sparse vectors of the
// Lagrange-basis commitments (bits | index polynomial | acc_x | acc_y: base index + PLAIN scalar), and per proof the result
// and the instance (= result - seed) for the transcript.  Until round 3 this ran on host threads (<= 254 additions + 2
// inversions per proof): 4 ms of two cores per 128-proof chunk, the largest host item of a rank of an 8-GPU node.
template <class S>
__global__ void __launch_bounds__(64)
k_ring_witness_acc(const te_pre *__restrict__ points, const uint32_t *__restrict__ kidx, const uint8_t *__restrict__ blind, uint32_t n, uint32_t keyset,
                   uint32_t L, uint32_t N, uint32_t cap, fp seedx, fp seedy, const uint32_t *__restrict__ zk, uint32_t *__restrict__ scratch,
                   uint32_t *__restrict__ pos, uint32_t *__restrict__ cnt, uint32_t *__restrict__ vals, uint32_t *__restrict__ sc, uint32_t *__restrict__ bi,
                   uint32_t *__restrict__ out) {
  // FOUR lanes per proof (te_quad.h: lane jc of the quad holds coordinate jc of the accumulator): a mixed addition is two rounds
  // of multiplications instead of eight sequential ones, the backward pass two rounds per row instead of four multiplications.
  using F = typename S::Fq;
  constexpr uint32_t MP = 264;
  const uint32_t lane = threadIdx.x & 63, jc = lane & 3;
  uint32_t p = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  const bool live = p < n;
  if (!live) p = n - 1;                                                        // (whole quads stay in step for the cross-lane moves; they write nothing)
  uint32_t *ppos = pos + (size_t)p * 256;
  const uint32_t ki = kidx[p];
  // the row list (every lane of the quad derives it; lane 0 writes it)
  uint32_t m = 1;
  for (uint32_t i = 0; i < L; i++) if ((blind[32 * (size_t)p + (i >> 3)] >> (i & 7)) & 1) m++;
  if (live && jc == 0) {
    uint32_t w = 0; ppos[w++] = ki;
    for (uint32_t i = 0; i < L; i++) if ((blind[32 * (size_t)p + (i >> 3)] >> (i & 7)) & 1) ppos[w++] = keyset + i;
    for (uint32_t j = w; j < 256; j++) ppos[j] = 0xffffffffu;
    cnt[p] = m;
  }
  // pass 1: the chain.  Scratch entry i of the proof: x | y | z of acc_i | prefix product z_0 .. z_{i-1}; lane jc stores word block jc
  // (lane 2 carries T, which is not kept: it stores the prefix product instead)
  uint32_t *sp = scratch + (size_t)p * 257 * 32;
  fp acc = jc == 0 ? seedx : jc == 1 ? seedy : jc == 2 ? fp_mul<F>(seedx, seedy) : fp_one<F>();
  fp run = fp_one<F>();                                                        // (meaningful on lane 3, mirrored to lane 2 for the store)
  uint32_t next_row = ki, bit = 0;
#pragma unroll 1
  for (uint32_t j = 0; j <= m; j++) {
    const fp z = qperm<3, 3, 3, 3>(acc);
    if (live) fp_store(sp + (size_t)j * 32 + 8 * (jc == 2 ? 3 : jc == 3 ? 2 : jc), jc == 2 ? run : acc);   // x, y, [z at block 2 from lane 3], run at block 3 from lane 2
    run = fp_mul<F>(run, z);
    if (j < m) {
      const te_pre q = points[next_row];
      acc = q_madd<S>(acc, q.x, q.y, q.k, jc);
      while (bit < L && !((blind[32 * (size_t)p + (bit >> 3)] >> (bit & 7)) & 1)) bit++;     // the next set bit of the blinding
      next_row = keyset + bit; bit++;
    }
  }
  fp inv = fp_inv_nf<F>(run);                                                   // (binary GCD, fp256.h: the fixed power was ~30 % of this kernel)
  // pass 2 (backwards): affine coordinates (Montgomery form) and, one row behind, the sparse scalars of the two accumulator columns
  uint32_t *v = vals + (size_t)p * 257 * 16;
  uint32_t *b = bi + (size_t)p * 4 * MP; uint32_t *qv = sc + (size_t)p * 4 * MP * 8;
  fp prev = fp_zero(), res = fp_zero();                                        // lane 0 / 1: x / y of row i + 1; of the last row (the result)
#pragma unroll 1
  for (uint32_t i = m + 1; i-- > 0;) {
    const uint32_t *e = sp + (size_t)i * 32;
    // round 1: lane 3: zi = inv * pre_i; lane 2: inv * z_i (the next inv); lanes 0, 1: from_mont of the previous row's difference
    const fp z = fp_load(e + 16), pre = fp_load(e + 24), xy = fp_load(e + 8 * (jc & 1));
    fp one_plain = fp_zero(); one_plain.v[0] = 1;
    const fp a1 = jc >= 2 ? inv : fp_zero(), b1 = jc == 3 ? pre : z;
    const fp r1 = fp_mul<F>(a1, b1);
    const fp zi = qperm<3, 3, 3, 3>(r1);
    inv = qperm<2, 2, 2, 2>(r1);
    // round 2: lanes 0, 1: x_i zi, y_i zi
    const fp aff = fp_mul<F>(xy, zi);
    if (live && jc < 2) fp_store(v + (size_t)i * 16 + 8 * jc, aff);
    if (i < m) {                                                               // scalar of row i: from_mont(v_i - v_{i+1}), base N + pos_i + 1
      const fp d = fp_from_mont<F>(fp_sub<F>(aff, prev));
      if (live && jc < 2) fp_store(qv + (size_t)((2 + jc) * MP + i) * 8, d);
    }
    if (i == m) res = aff;
    prev = aff;
  }
  // the rest is cheap and done by lane 0 of the quad (result coordinates from the registers of lanes 0 and 1, not through memory)
  const fp resx = qperm<0, 0, 0, 0>(res), resy = qperm<1, 1, 1, 1>(res);
  if (!live || jc != 0) return;
  // instance = result - seed  (-(x, y) = (-x, y))
  te_ext r; r.x = resx; r.y = resy; r.t = fp_mul<F>(resx, resy); r.z = fp_one<F>();
  const te_aff inst = te_to_aff<S>(te_madd<S>(r, te_make_pre<S>(fp_neg<F>(seedx), seedy)));
  uint32_t *o = out + (size_t)p * 32;
  fp_store(o, resx); fp_store(o + 8, resy); fp_store(o + 16, inst.x); fp_store(o + 24, inst.y);
  // sparse vectors: bits | ip | ax | ay   (the host zeroed both arrays: unused entries are scalar 0 at base 0)
  fp one_plain = fp_zero(); one_plain.v[0] = 1;
  const fp minus1 = fp_from_mont<F>(fp_neg<F>(fp_one<F>()));
  for (uint32_t j = 0; j < m; j++) { b[j] = ppos[j]; fp_store(qv + (size_t)j * 8, one_plain); }
  b[MP] = N + cap; fp_store(qv + (size_t)MP * 8, one_plain);
  b[MP + 1] = N + ki + 1; fp_store(qv + (size_t)(MP + 1) * 8, minus1);
  for (uint32_t j = 0; j < m; j++) b[2 * MP + j] = b[3 * MP + j] = N + ppos[j] + 1;
  b[2 * MP + m] = b[3 * MP + m] = N + cap;
  fp_store(qv + (size_t)(2 * MP + m) * 8, fp_from_mont<F>(resx)); fp_store(qv + (size_t)(3 * MP + m) * 8, fp_from_mont<F>(resy));
  if (zk) for (uint32_t col = 0; col < 4; col++) for (uint32_t j = 0; j < 3; j++) {     // + zk_j * L_{cap+j}(tau) G
    b[col * MP + m + 1 + j] = cap + j;
    fp_store(qv + (size_t)(col * MP + m + 1 + j) * 8, fp_from_mont<F>(fp_load(zk + (((size_t)p * 4 + col) * 3 + j) * 8)));
  }
}
template <class S>
__global__ void k_ring_points_pre(const uint32_t *__restrict__ xy_mont, uint32_t n, te_pre *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = te_make_pre<S>(fp_load(xy_mont + (size_t)i * 16), fp_load(xy_mont + (size_t)i * 16 + 8));
}
template <class F>
__global__ void k_set_diag(uint32_t *__restrict__ mat, uint32_t n, uint32_t rows, uint32_t col0) {   // row i of the tile = unit vector e_(col0 + i)
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) fp_store(mat + ((size_t)i * n + col0 + i) * 8, fp_one<F>());
}

}  // namespace avrf
