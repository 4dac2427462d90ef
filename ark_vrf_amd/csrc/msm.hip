// msm.hip -- Pippenger bucket MSM on gfx950 (CDNA4), curve-generic (curves.h): twisted Edwards (Thin / Pedersen batch
// verification) and short-Weierstrass G1 (KZG commitments of the ring SNARK).
//
// Replaces arkworks `VariableBaseMSM::msm_unchecked` (third-party ark-ec 0.6) at the
// reference call sites src/thin.rs:319, src/pedersen.rs:420, src/utils/common.rs:410-411 and inside w3f-pcs KZG.
// Any correct MSM yields the same group element; parity is on the normalised result
// (SURVEY.md A.9), so the decomposition below is designed for the GPU, not copied:
//
//   k_digits     one lane per scalar: signed c-bit digits of every window -> 16-bit keys
//                (bucket | sign<<15), window-major, coalesced
//   k_hist       workgroup (tile, window): LDS histogram of its tile of keys -> H[w][tile][b]
//   k_scan_tiles lane per (window, bucket): prefix over tiles (in place), entry counts;  k_scan_offs  workgroup per window: entry offsets, window total
//   k_plan       one workgroup: entries per lane `per` = ceil(all entries / lanes the chip holds at once) and the first
//                lane of every window
//   k_scatter    workgroup (tile, window): LDS cursors seeded from the scanned histogram; every
//                key gets its slot with an LDS atomic -- no global atomics anywhere in the sort
//   k_accumulate EQUAL SHARES: every lane owns `per` consecutive entries of the sorted array, whatever buckets they fall
//                in, so all lanes of the launch do the same number of mixed additions and the launch is exactly one
//                residency round of the chip (no tail, no load sorting, no cross-lane reduction in the hot kernel).
//                At a bucket boundary the lane writes its partial sum to slot (lane + bucket) -- strictly increasing
//                along the sorted order, so the partials of one bucket are contiguous -- and starts over.
//   k_bucket_sum per bucket: identity for empty buckets, else the sum of its partials (a wave cooperates on buckets
//                that many lanes fed: skewed scalars)
//   k_wsum_blk / k_wsum   weighted bucket sum sum_b b*B_b of one window (or of one fixed-base bucket set) by
//                a workgroup / a group of lanes: 2 additions per bucket + a suffix scan
//   k_rowcol, k_bits, k_bits_direct, k_horner   the bit-decomposition reduction sum_b b*B_b = sum_k 2^k T_k, kept for
//                G1 MSMs without a window table (ring_proof::index, the verifier's MSMs) and for segmented launches
//   host         msm_fold: Horner over what the chain's tail left (window triples, bit sums), or the finished points as they are
//
// Fixed-base mode (G1 only): the bases are a window table T[w][i] = 2^(c w) P_i, so ALL windows of a scalar vector
// share one bucket set; `batch` vectors over the same table run as `batch` bucket sets in one launch chain.
//
// Layout in HBM: points AoS (te_pre x|y|k 96 B; G1 affine x|y 64 / 96 B), gathered whole by one lane with dwordx4
// loads; keys/sorted SoA per window (coalesced); buckets AoS (te_ext 128 B; XYZZ 128 / 192 B).
#include "msm.h"
#include "host_pool.h"
#include "curves.h"
#include "suite_dispatch.h"
#include "te_quad.h"
#include "host_g1.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <vector>

namespace avrf {

// a failed HIP call (out of memory, lost device) unwinds to the C-ABI entry point, which returns AVRF_ERR_NO_DEVICE
#define HIP_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw HipFailure{e_, __FILE__, __LINE__}; } while (0)

// ---------------------------------------------------------------- conversions

// mont_in: the coordinates are ALREADY Montgomery limbs (arkworks' in-memory Fp; the zero-copy flavour of SURVEY.md 8b)
template <class S>
__global__ void __launch_bounds__(256) k_pre_from_affine(const uint8_t *__restrict__ xy, uint32_t n, te_pre *__restrict__ out,
                                  uint32_t *__restrict__ flag, int check_curve, int mont_in) {
  using Fq = typename S::Fq;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp x = fp_load_le(xy + 64 * (size_t)i), y = fp_load_le(xy + 64 * (size_t)i + 32);
  uint32_t f = 0;
  if (ge_p<Fq>(x) || ge_p<Fq>(y)) f |= 1;
  fp xm = mont_in ? x : fp_to_mont<Fq>(x), ym = mont_in ? y : fp_to_mont<Fq>(y);
  if (check_curve && !te_on_curve<S>(xm, ym)) f |= 2;
  store_pre(out + i, te_make_pre<S>(xm, ym));
  if (f) atomicOr(flag, f);
}

void launch_pre_from_affine(int suite, const uint8_t *d_xy, size_t n, te_pre_raw *d_pre, uint32_t *d_flag,
                            int check_curve, hipStream_t stream, int mont_in) {
  if (!n) return;
  dim3 g((unsigned)((n + 255) / 256)), b(256);
  with_suite(suite, [&](auto tag) { using S = typename decltype(tag)::type;
    hipLaunchKernelGGL(k_pre_from_affine<S>, g, b, 0, stream, d_xy, (uint32_t)n, (te_pre *)d_pre, d_flag, check_curve, mont_in); });
}
// scalars held as Montgomery limbs of Fr (arkworks' in-memory ScalarField) -> plain integers, in place; flag |= 4 when >= r
template <class S>
__global__ void __launch_bounds__(256) k_scalars_from_mont(uint32_t *__restrict__ sc, uint32_t n, uint32_t *__restrict__ flag) {
  using Fr = typename S::Fr;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp k = fp_load(sc + 8 * (size_t)i);
  if (ge_p<Fr>(k)) atomicOr(flag, 4u);
  fp_store(sc + 8 * (size_t)i, fp_from_mont<Fr>(k));
}
void launch_scalars_from_mont(int suite, uint32_t *d_scalars, size_t n, uint32_t *d_flag, hipStream_t stream) {
  if (!n) return;
  with_suite(suite, [&](auto tag) { using S = typename decltype(tag)::type;
    hipLaunchKernelGGL(k_scalars_from_mont<S>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_scalars, (uint32_t)n, d_flag); });
}

// ---------------------------------------------------------------- digits

// signed digit of window w with carry chain; digits in [-(2^(c-1)-1), 2^(c-1)];
// key = bucket (1..2^(c-1), 0 = skip) | sign << 15
// blockIdx.y = index of the scalar vector in a batch of MSMs over the same bases ("virtual windows"
// v = batch * nwin + w everywhere downstream)
// (With fixed-base window tables the nwin digit rows of one vector are simply consumed as ONE window of
// n * nwin keys: same layout, different interpretation downstream.)
__global__ void __launch_bounds__(256) k_digits(const uint32_t *__restrict__ scalars, uint32_t n, uint32_t stride, int c, int nwin, uint16_t *__restrict__ keys, int mont) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t bat = blockIdx.y;
  keys += (size_t)bat * nwin * n;
  uint32_t s[9];
  const uint4 *p = reinterpret_cast<const uint4 *>(scalars + 8 * ((size_t)bat * stride + i));
  uint4 a = p[0], b = p[1];
  s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w; s[8] = 0;
  if (mont) {                                                // the vector holds Montgomery limbs (the ring prover's coefficient vectors): 1 = BLS12-381 Fr, 2 = BN254 Fr
    fp v;
#pragma unroll
    for (int k = 0; k < 8; k++) v.v[k] = s[k];
    v = mont == 1 ? fp_from_mont<FqBandersnatch>(v) : fp_from_mont<FqBabyJubJub>(v);
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = v.v[k];
  }
  const uint32_t nb = 1u << (c - 1), mask = (1u << c) - 1;
  uint32_t carry = 0;
  for (int w = 0; w < nwin; w++) {
    int bit = w * c;
    uint32_t v = 0;
    if (bit < 256) {
      int li = bit >> 5, sh = bit & 31;
      uint64_t two = (uint64_t)s[li] | ((uint64_t)s[li + 1] << 32);
      v = (uint32_t)(two >> sh) & mask;
    }
    v += carry;
    uint32_t key;
    if (v > nb) { key = ((1u << c) - v) | 0x8000u; carry = 1; }   // negative digit: bucket 2^c - v
    else { key = v; carry = 0; }
    keys[(size_t)w * n + i] = (uint16_t)key;
  }
}

// ---------------------------------------------------------------- counting sort (LDS only)

// H[(w * ntiles + tile) * nb + (bucket-1)] = number of keys of `tile` in that bucket
__global__ void __launch_bounds__(256)
k_hist(const uint16_t *__restrict__ keys, uint32_t n, uint32_t tile_len, int c, uint32_t *__restrict__ H) {
  extern __shared__ uint32_t lds[];
  const uint32_t nb = 1u << (c - 1), tile = blockIdx.x, w = blockIdx.y, ntiles = gridDim.x;
  for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) lds[b] = 0;
  __syncthreads();
  uint32_t lo = tile * tile_len, hi = lo + tile_len; if (hi > n) hi = n;
  const uint16_t *kw = keys + (size_t)w * n;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    uint32_t b = kw[i] & 0x7fffu;
    if (b) atomicAdd(&lds[b - 1], 1u);
  }
  __syncthreads();
  uint32_t *out = H + ((size_t)w * ntiles + tile) * nb;
  for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) out[b] = lds[b];
}

// Two steps.  k_scan_tiles, one lane per (window, bucket), adjacent lanes on adjacent buckets: in place, H[w][tile][b] becomes the
// exclusive prefix over tiles (loads issued eight tiles at a time: the chain is additions, not memory round trips) and
// cnts[slot] (slot = w*nb + b-1) the entry count.  k_scan_offs, one workgroup (1024 lanes) per window: offs[slot] = entry
// offset (global, w*n based), win_tot[w] = entries of the window.  (One fused workgroup per window took 55 us of a 1.17 ms
// batch: 4 buckets x 33 tiles of dependent, strided read-modify-writes per lane on 20 workgroups.)
__global__ void __launch_bounds__(256)
k_scan_tiles(uint32_t *__restrict__ H, uint32_t ntiles, int c, uint32_t *__restrict__ cnts) {
  const uint32_t nb = 1u << (c - 1), w = blockIdx.y, b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  uint32_t *Hb = H + (size_t)w * ntiles * nb + b;
  uint32_t run = 0, k = 0;
  for (; k + 8 <= ntiles; k += 8) {
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = Hb[(size_t)(k + j) * nb];
#pragma unroll
    for (int j = 0; j < 8; j++) { Hb[(size_t)(k + j) * nb] = run; run += v[j]; }
  }
  for (; k < ntiles; k++) { const uint32_t v = Hb[(size_t)k * nb]; Hb[(size_t)k * nb] = run; run += v; }
  cnts[(size_t)w * nb + b] = run;
}
__global__ void __launch_bounds__(1024)
k_scan_offs(const uint32_t *__restrict__ cnts, uint32_t n, int c, uint32_t *__restrict__ offs, uint32_t *__restrict__ win_tot) {
  __shared__ uint32_t part[1024];
  const uint32_t nb = 1u << (c - 1), w = blockIdx.x, t = threadIdx.x;
  const uint32_t bpt = (nb + 1023) / 1024;
  uint32_t b0 = t * bpt, b1 = b0 + bpt; if (b1 > nb) b1 = nb; if (b0 > nb) b0 = nb;
  uint32_t sum = 0;
  for (uint32_t b = b0; b < b1; b++) sum += cnts[(size_t)w * nb + b];
  part[t] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    uint32_t v = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  if (t == 1023) win_tot[w] = part[1023];
  uint32_t run = part[t] - sum + w * n;
  for (uint32_t b = b0; b < b1; b++) { offs[(size_t)w * nb + b] = run; run += cnts[(size_t)w * nb + b]; }
}

// plan[0] = per (entries per lane), plan[1] = lanes used, plan[2] = 0 (heavy-bucket counter of k_bucket_sum); lane_base[v] = first lane of window v (lane_base[vwin] = plan[1]).
// per = max(per_min, ceil(sum of win_tot / lanes_target)): with lanes_target = what the chip holds in one residency round
// of k_accumulate, the launch is one round of equally loaded lanes.
__global__ void __launch_bounds__(1024)
k_plan(const uint32_t *__restrict__ win_tot, uint32_t vwin, uint32_t lanes_target, uint32_t per_min, uint32_t *__restrict__ lane_base,
       uint32_t *__restrict__ plan) {
  __shared__ uint64_t red[1024];
  __shared__ uint32_t sc[1024];
  __shared__ uint32_t carry_s;
  const uint32_t t = threadIdx.x;
  uint64_t s = 0;
  for (uint32_t v = t; v < vwin; v += 1024) s += win_tot[v];
  red[t] = s;
  __syncthreads();
  for (uint32_t off = 512; off >= 1; off >>= 1) { if (t < off) red[t] += red[t + off]; __syncthreads(); }
  const uint64_t total = red[0];
  // every window rounds its last lane up, so the launch uses up to total / per + vwin lanes: shares are sized for
  // lanes_target - vwin, or those few extra lanes land in a workgroup that is NOT resident in the first round -- it starts when
  // the first workgroup retires and the kernel ends a whole share later (round 5: waves lived 280 us of a 355 us launch)
  if (lanes_target > 8 * vwin) lanes_target -= vwin;
  uint64_t per64 = (total + lanes_target - 1) / lanes_target;
  if (per64 < per_min) per64 = per_min;
  const uint32_t per = (uint32_t)per64;
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t base = 0; base < vwin; base += 1024) {
    const uint32_t v = base + t;
    const uint32_t mine = v < vwin ? (win_tot[v] + per - 1) / per : 0;
    sc[t] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
      uint32_t x = (t >= off) ? sc[t - off] : 0;
      __syncthreads();
      sc[t] += x;
      __syncthreads();
    }
    if (v < vwin) lane_base[v] = carry_s + sc[t] - mine;
    __syncthreads();
    if (t == 1023) carry_s += sc[1023];
    __syncthreads();
  }
  if (t == 0) { lane_base[vwin] = carry_s; plan[0] = per; plan[1] = carry_s; plan[2] = 0; }
}

// remap_n != 0 (fixed-base tables): key position p = dw * remap_n + i refers to table entry dw * remap_stride + i
// (or dw * remap_stride + bidx[v][i] when the vector names its own bases)
// base_stride != 0 (segmented MSMs, msm_te_segments): vector w / nwin multiplies bases of its own, which start at (w / nwin) * base_stride
__global__ void __launch_bounds__(256)
k_scatter(const uint16_t *__restrict__ keys, uint32_t n, uint32_t tile_len, int c, const uint32_t *__restrict__ H,
          const uint32_t *__restrict__ offs, uint32_t *__restrict__ sorted, uint32_t remap_n, uint32_t remap_stride,
          const uint32_t *__restrict__ bidx, uint32_t ntiles, uint32_t vwin, uint32_t nwin, uint32_t base_stride) {
  extern __shared__ uint32_t lds[];
  // XCD-aware placement: workgroups go round-robin over the 8 XCDs by linear id, and every XCD has its own L2.  All tiles of a
  // window run on ONE XCD (window w on XCD w mod 8), so the 4-byte scattered stores into that window's region of sorted[]
  // meet in one L2 and leave it as whole lines (with tiles of a window spread over all XCDs every L2 evicted partial lines:
  // 142 MB written for 21 MB of indices, rounds 1-2).
  const uint32_t nb = 1u << (c - 1);
  const uint32_t xcd = blockIdx.x & 7u, k = blockIdx.x >> 3, tile = k % ntiles, w = xcd + 8u * (k / ntiles);
  if (w >= vwin) return;
  const uint32_t base0 = base_stride ? (w / nwin) * base_stride : 0u;   // (0 for every launch over shared bases: the stored index is i, as ever)
  const uint32_t *Hin = H + ((size_t)w * ntiles + tile) * nb;
  for (uint32_t b = threadIdx.x; b < nb; b += blockDim.x) lds[b] = offs[(size_t)w * nb + b] + Hin[b];
  __syncthreads();
  uint32_t lo = tile * tile_len, hi = lo + tile_len; if (hi > n) hi = n;
  const uint16_t *kw = keys + (size_t)w * n;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    uint32_t key = kw[i], b = key & 0x7fffu;
    if (b) {
      uint32_t pos = atomicAdd(&lds[b - 1], 1u);
      uint32_t idx = i + base0;
      if (remap_n) {                                      // bidx: per-vector base indices (sparse MSMs over a shared table)
        uint32_t j = i % remap_n;
        idx = (i / remap_n) * remap_stride + (bidx ? bidx[(size_t)w * remap_n + j] : j);
      }
      sorted[pos] = idx | ((key & 0x8000u) << 16);
    }
  }
}

// out-of-line point ops for the (cold) reduction kernels: keeps their code size and compile time down
template <class CV> __device__ __noinline__ void cv_add_nf(typename CV::acc_t *r, const typename CV::acc_t *a, const typename CV::acc_t *b) { *r = CV::add(*a, *b); }
template <class CV> __device__ __noinline__ void cv_dbl_nf(typename CV::acc_t *r, const typename CV::acc_t *a) { *r = CV::dbl(*a); }
template <class CV> AVRF_DI typename CV::acc_t cv_add(const typename CV::acc_t &a, const typename CV::acc_t &b) {
  if constexpr (CV::INLINE_REDUCE_OPS) return CV::add(a, b);
  else { typename CV::acc_t r; cv_add_nf<CV>(&r, &a, &b); return r; }
}
template <class CV> AVRF_DI typename CV::acc_t cv_dbl(const typename CV::acc_t &a) {
  if constexpr (CV::INLINE_REDUCE_OPS) return CV::dbl(a);
  else { typename CV::acc_t r; cv_dbl_nf<CV>(&r, &a); return r; }
}


// ---------------------------------------------------------------- bucket accumulation (curve-generic)

// Lane t owns the entries [e0, e0 + per) of window v (lane_base[v] <= t < lane_base[v + 1]; r = t - lane_base[v];
// e0 = v * n + r * per).  Partial sums go to part[(t + v * nb + b) * ACC_WORDS] for every bucket b the range touches.
template <class CV>
__global__ void __launch_bounds__(256, CV::MIN_WAVES)
k_accumulate(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ sorted,
             const uint32_t *__restrict__ offs, const uint32_t *__restrict__ win_tot, const uint32_t *__restrict__ lane_base,
             const uint32_t *__restrict__ plan, uint32_t vwin, uint32_t nb, uint32_t n, uint32_t *__restrict__ part) {
  using AC = typename CV::accum;                              // the register form of the accumulator (curves.h)
  using acc_t = typename AC::acc_t; using base_t = typename CV::base_t;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t per = plan[0];
  if (t >= plan[1]) return;
  uint32_t lo = 0, hi = vwin;                                  // largest v with lane_base[v] <= t
  while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (lane_base[mid] <= t) lo = mid; else hi = mid; }
  const uint32_t v = lo;
  const uint32_t wbeg = v * n, wend = wbeg + win_tot[v];
  const uint32_t e0 = wbeg + (t - lane_base[v]) * per;
  uint32_t e1 = e0 + per; if (e1 > wend) e1 = wend;
  const uint32_t *ow = offs + (size_t)v * nb;
  lo = 0; hi = nb;                                             // largest b with offs[b] <= e0: the bucket of entry e0
  while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (ow[mid] <= e0) lo = mid; else hi = mid; }
  uint32_t b = lo;
  uint32_t nxt = (b + 1 < nb) ? ow[b + 1] : 0xffffffffu;      // first entry of the next bucket
  const size_t slot0 = (size_t)t + (size_t)v * nb;
  acc_t acc;
  {
    // Gather pipeline through LDS: the base of entry k + 1 travels HBM -> LDS by DMA (global_load_lds_dwordx4: lane l's 16-byte
    // chunk c lands at chunk c's row + 16 l of the wave's buffer) while the addition of entry k runs, and costs NO registers until
    // it is read back at the top of its own iteration (the register form of this prefetch held 24 VGPRs across the whole
    // addition: 198 for the twisted-Edwards kernel; the 381-bit kernel had no room for it and waited out every gather).
    // Two buffers per wave; the index of entry k + 2 is in flight as well.
    extern __shared__ uint32_t acc_lds[];
    constexpr int BW = CV::BASE_WORDS, CH = BW / 4;
    uint32_t *wbuf = acc_lds + (threadIdx.x >> 6) * (2 * BW * 64);
    const uint32_t lane = threadIdx.x & 63;
    auto issue = [&](uint32_t ix, uint32_t slot) {
      const uint32_t *src = bases + (size_t)(ix & 0x7fffffffu) * BW;
#pragma unroll
      for (int c = 0; c < CH; c++)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + 4 * c),
                                         (__attribute__((address_space(3))) void *)(wbuf + slot * (BW * 64) + c * 256), 16, 0, 0);
    };
    auto fetch = [&](uint32_t slot) {
      uint32_t w[BW];
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const uint4 v = *reinterpret_cast<const uint4 *>(wbuf + slot * (BW * 64) + c * 256 + lane * 4);
        w[4 * c] = v.x; w[4 * c + 1] = v.y; w[4 * c + 2] = v.z; w[4 * c + 3] = v.w;
      }
      return CV::base_from_words(w);
    };
    const uint32_t cnt = e1 - e0;
    if constexpr (!CV::PREFETCH) acc = AC::identity();
    uint32_t idx = cnt ? sorted[e0] : 0u;                       // (a lane with an empty share reads nothing and gathers nothing)
    uint32_t idx1 = cnt > 1 ? sorted[e0 + 1] : 0u;
    if (cnt) issue(idx, 0);
    for (uint32_t k = 0; k < cnt; k++) {                        // k is the same in every lane of the wave (shares start together)
      const uint32_t i = e0 + k, cidx = idx;
      // the DMA of this buffer was issued one iteration ago: the compiler's own wait insertion does not carry an LDS-DMA across
      // the loop's back edge (it put the ds_reads BEFORE its vmcnt(0)), so the wait is explicit -- and a compiler barrier.
      // lgkmcnt(0): the ds_reads of the OTHER buffer (last iteration's fetch) have returned before the DMA issued below overwrites it.
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      const base_t cur = fetch(k & 1);
      idx = idx1;
      if (k + 1 < cnt) issue(idx, (k + 1) & 1);
      if (k + 2 < cnt) idx1 = sorted[i + 2];
      if constexpr (CV::PREFETCH) {                             // first entry of every lane: no addition, just the base
        if (k == 0) { acc = AC::from_base(cur, (cidx & 0x80000000u) != 0); continue; }
      }                                                          // (the 381-bit policy's madd takes the identity as it comes: one code path, fewer registers)
      if (i >= nxt) {                                          // bucket boundary inside the lane's range
        AC::store_part(part + (slot0 + b) * AC::PART_WORDS, acc);
        acc = AC::identity();
        do { b++; nxt = (b + 1 < nb) ? ow[b + 1] : 0xffffffffu; } while (i >= nxt);
      }
      acc = AC::madd(acc, cur, (cidx & 0x80000000u) != 0);
    }
  }
  AC::store_part(part + (slot0 + b) * AC::PART_WORDS, acc);
}

template <class CV> AVRF_DI typename CV::acc_t wave_sum(typename CV::acc_t acc);

// Bucket `slot` = v * nb + b holds entries [offs, offs + cnt): they were accumulated by lanes lf..ll of window v, whose partials
// sit in part[lf + slot .. ll + slot].  Buckets fed by more than HEAVY lanes (the short top window of a 253-bit scalar; skewed
// scalars) are only listed here (plan[2] = count, heavy[] = slots) and summed by k_heavy_sum, one workgroup each.
constexpr uint32_t HEAVY_PARTIALS = 12;
template <class CV>
__global__ void __launch_bounds__(256, CV::RED_WAVES)
k_bucket_sum(const uint32_t *__restrict__ offs, const uint32_t *__restrict__ cnts, const uint32_t *__restrict__ lane_base,
             uint32_t *__restrict__ plan, uint32_t nslots, uint32_t nb, uint32_t n, const uint32_t *__restrict__ part,
             uint32_t *__restrict__ buckets, uint32_t *__restrict__ heavy) {
  using acc_t = typename CV::acc_t;
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nslots) return;
  const uint32_t per = plan[0];
  const uint32_t cnt = cnts[slot];
  if (!cnt) { if (!CV::ZERO_IS_IDENTITY) CV::store_acc(buckets + (size_t)slot * CV::ACC_WORDS, CV::identity()); return; }
  const uint32_t v = slot / nb, rel = offs[slot] - v * n;
  const uint32_t lf = rel / per, ll = (rel + cnt - 1) / per, np = ll - lf + 1;
  if (np > HEAVY_PARTIALS) { heavy[atomicAdd(&plan[2], 1u)] = slot; return; }
  const size_t p0 = (size_t)lane_base[v] + lf + slot;
  using AC = typename CV::accum;
  acc_t acc = AC::load_part(part + p0 * AC::PART_WORDS);
#pragma unroll 1
  for (uint32_t k = 1; k < np; k++) acc = cv_add<CV>(acc, AC::load_part(part + (p0 + k) * AC::PART_WORDS));
  CV::store_acc(buckets + (size_t)slot * CV::ACC_WORDS, acc);
}

template <class CV>
__global__ void __launch_bounds__(256, CV::RED_WAVES)
k_heavy_sum(const uint32_t *__restrict__ offs, const uint32_t *__restrict__ cnts, const uint32_t *__restrict__ lane_base,
            const uint32_t *__restrict__ plan, uint32_t nb, uint32_t n, const uint32_t *__restrict__ part,
            uint32_t *__restrict__ buckets, const uint32_t *__restrict__ heavy) {
  using acc_t = typename CV::acc_t;
  extern __shared__ uint32_t lds[];                                            // 4 accumulators
  const uint32_t per = plan[0], nheavy = plan[2], t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (uint32_t h = blockIdx.x; h < nheavy; h += gridDim.x) {
    const uint32_t slot = heavy[h], cnt = cnts[slot];
    const uint32_t v = slot / nb, rel = offs[slot] - v * n;
    const uint32_t lf = rel / per, ll = (rel + cnt - 1) / per, np = ll - lf + 1;
    const size_t p0 = (size_t)lane_base[v] + lf + slot;
    if constexpr (CV::QUAD) { q_heavy_sum<typename CV::suite>(part, p0, np, buckets + (size_t)slot * CV::ACC_WORDS, lds); continue; }
    acc_t a = CV::identity();
#pragma unroll 1
    for (uint32_t k = t; k < np; k += 256) a = cv_add<CV>(a, CV::accum::load_part(part + (p0 + k) * CV::accum::PART_WORDS));
    a = wave_sum<CV>(a);                                                        // valid in lane 0
    if (lane == 0) CV::store_acc(lds + wv * CV::ACC_WORDS, a);
    __syncthreads();
    if (t == 0) {
#pragma unroll 1
      for (uint32_t w = 1; w < 4; w++) a = cv_add<CV>(a, CV::load_acc(lds + w * CV::ACC_WORDS));
      CV::store_acc(buckets + (size_t)slot * CV::ACC_WORDS, a);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- bucket reduction by index bits

template <class CV> AVRF_DI typename CV::acc_t wave_sum(typename CV::acc_t acc) {
#pragma unroll 1
  for (int off = 32; off >= 1; off >>= 1) acc = cv_add<CV>(acc, CV::shfl_down(acc, off));
  return acc;                                             // valid in lane 0
}

// Bucket index b in [1, nb-1] (nb = 2^(c-1)) split as b = hi * 2^h + lo; B_0 = identity.
// One wave per task: tasks [0, NR) are row sums R_hi (2^h contiguous buckets), tasks [NR, NR+NC)
// are column sums C_lo (stride 2^h).  rc[w * (NR+NC) + task].
template <class CV>
__global__ void __launch_bounds__(256)
k_rowcol(const uint32_t *__restrict__ buckets, int c, int h, uint32_t total_waves, uint32_t *__restrict__ rc) {
  const uint32_t nb = 1u << (c - 1), NC = 1u << h, NR = nb >> h;
  const uint32_t gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (gw >= total_waves) return;
  const uint32_t tasks = NR + NC, w = gw / tasks, task = gw - w * tasks;
  const uint32_t *B = buckets + (size_t)w * nb * CV::ACC_WORDS;              // B[b-1]
  typename CV::acc_t acc = CV::identity();
  if (task < NR) {
    for (uint32_t lo = lane; lo < NC; lo += 64) { uint32_t b = task * NC + lo; if (b >= 1) acc = CV::add(acc, CV::load_acc(B + (size_t)(b - 1) * CV::ACC_WORDS)); }
  } else {
    uint32_t lo = task - NR;
    for (uint32_t hi = lane; hi < NR; hi += 64) { uint32_t b = hi * NC + lo; if (b >= 1) acc = CV::add(acc, CV::load_acc(B + (size_t)(b - 1) * CV::ACC_WORDS)); }
  }
  acc = wave_sum<CV>(acc);
  if (lane == 0) CV::store_acc(rc + (size_t)gw * CV::ACC_WORDS, acc);
}

// One wave per (window, bit k), k in [0, c): out[w*c + k] = T_k.
template <class CV>
__global__ void __launch_bounds__(256)
k_bits(const uint32_t *__restrict__ buckets, const uint32_t *__restrict__ rc, int c, int h, uint32_t total_waves, uint32_t *__restrict__ out) {
  const uint32_t nb = 1u << (c - 1), NC = 1u << h, NR = nb >> h;
  const uint32_t gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (gw >= total_waves) return;
  const uint32_t w = gw / c, k = gw - w * c;
  const uint32_t *RC = rc + (size_t)w * (NR + NC) * CV::ACC_WORDS;
  typename CV::acc_t acc = CV::identity();
  if ((int)k == c - 1) { if (lane == 0) acc = CV::load_acc(buckets + ((size_t)w * nb + (nb - 1)) * CV::ACC_WORDS); }   // only b = nb
  else if ((int)k < h) { for (uint32_t lo = lane; lo < NC; lo += 64) if ((lo >> k) & 1) acc = CV::add(acc, CV::load_acc(RC + (size_t)(NR + lo) * CV::ACC_WORDS)); }
  else { uint32_t kk = k - h; for (uint32_t hi = lane; hi < NR; hi += 64) if ((hi >> kk) & 1) acc = CV::add(acc, CV::load_acc(RC + (size_t)hi * CV::ACC_WORDS)); }
  acc = wave_sum<CV>(acc);
  if (lane == 0) CV::store_acc(out + (size_t)gw * CV::ACC_WORDS, acc);
}

// Small bucket counts (nb <= 256, the batched KZG-sized MSMs): one LANE per (window, bit k) adds the nb/2
// buckets whose index has bit k set -- the wave-per-task row/column kernels above would spend a whole
// wave (and a 6-step shuffle tree) on a handful of buckets.
template <class CV>
__global__ void __launch_bounds__(128)
k_bits_direct(const uint32_t *__restrict__ buckets, int c, uint32_t total, uint32_t *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const uint32_t nb = 1u << (c - 1), w = t / c, k = t - w * c;
  const uint32_t *B = buckets + (size_t)w * nb * CV::ACC_WORDS;
  typename CV::acc_t acc = CV::identity();
  if ((int)k == c - 1) acc = CV::load_acc(B + (size_t)(nb - 1) * CV::ACC_WORDS);
  else for (uint32_t m = 0; m < (nb >> 1); m++) {
    uint32_t b = ((m >> k) << (k + 1)) | (1u << k) | (m & ((1u << k) - 1));
    acc = CV::add(acc, CV::load_acc(B + (size_t)(b - 1) * CV::ACC_WORDS));
  }
  CV::store_acc(out + (size_t)t * CV::ACC_WORDS, acc);
}

// Window/bit Horner on the device for BATCHED MSMs: one lane per MSM walks its nbits bit sums,
// result = sum_p 2^p T_p.  (A single MSM finishes faster on the host; with hundreds of MSMs per launch
// chain the host Horner would dominate.)
template <class CV>
__global__ void __launch_bounds__(64)
k_horner(const uint32_t *__restrict__ bits, uint32_t nbits, uint32_t batch, uint32_t *__restrict__ out) {
  uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const uint32_t *T = bits + (size_t)b * nbits * CV::ACC_WORDS;
  typename CV::acc_t acc = CV::identity();
  for (int i = (int)nbits - 1; i >= 0; i--) {
    acc = CV::dbl(acc);
    acc = CV::add(acc, CV::load_acc(T + (size_t)i * CV::ACC_WORDS));
  }
  CV::store_acc(out + (size_t)b * CV::ACC_WORDS, acc);
}

// The same Horner for the segmented twisted-Edwards chain (msm_te_segments), a WAVE per MSM with a point spread over the four lanes of
// a quad (te_quad.h).  A lane per MSM walks nbits one-lane doublings and additions one after the other, and a SIMD retires those no
// faster for four waves than for sixty-four: 2.9 ms for 256 MSMs of 259 bit sums, two thirds of the whole segmented call.  Here quad q
// of the wave folds the m = ceil(nbits / 16) bit sums from q m on (m two-round doublings and three-round additions), then a tree over
// the quads shifts the upper half by s m doublings and adds it, s = 1, 2, 4, 8: 15 m doublings in a row -- the 2^252 of the top bits,
// which no arrangement avoids -- but only four more additions.  All 64 lanes stay active throughout (the DPP moves of q_add / q_dbl
// need whole quads); only quad 0's result is kept.
template <class S>
__global__ void __launch_bounds__(64)
k_horner_quads(const uint32_t *__restrict__ bits, uint32_t nbits, uint32_t *__restrict__ out) {
  const uint32_t v = blockIdx.x, q = threadIdx.x >> 2, j = threadIdx.x & 3, m = (nbits + 15) / 16;
  const uint32_t *T = bits + (size_t)v * nbits * 32 + j * 8;          // coordinate j of te_ext x | y | t | z
  fp acc = q_identity<S>(j);
#pragma unroll 1
  for (int i = (int)m - 1; i >= 0; i--) {
    const uint32_t p = q * m + (uint32_t)i;
    acc = q_dbl<S>(acc, j);
    acc = q_add<S>(acc, p < nbits ? fp_load(T + (size_t)p * 32) : q_identity<S>(j), j);
  }
#pragma unroll 1
  for (uint32_t s = 1; s < 16; s <<= 1) {
    fp o = fp_shfl_down(acc, 4 * (int)s);                             // quad q + s (what the quads without such a partner compute is dropped)
#pragma unroll 1
    for (uint32_t d = 0; d < s * m; d++) o = q_dbl<S>(o, j);
    acc = q_add<S>(acc, o, j);
  }
  if (q == 0) fp_store(out + (size_t)v * 32 + j * 8, acc);
}

// The Horner of the segmented G1 chain (msm_g1_segments), a WAVE per MSM, and the affine conversion behind it.  An XYZZ point of the
// 12-limb curve fills 48 registers, so a point stays in its lane (no quad form as te_quad.h has for the 8-limb Edwards points); the
// split is the one of k_horner_quads with lanes for quads.  Lane q folds the m = ceil(nbits / 64) bit sums from q m on (m doublings and
// m additions, all lanes side by side); a tree over the lanes then shifts the upper half by s m doublings and adds it, s = 1, 2, .., 32
// (points move between lanes as in k_g1_lincomb, one shuffle per limb).  In a row: 64 m >= nbits doublings -- the 2^(nbits - m) of the top
// lane, which no arrangement avoids -- but m + 6 additions instead of nbits.  Bit sums at or beyond nbits count as the identity; what the
// lanes without a partner compute is dropped.  The result leaves as a Montgomery AFFINE point ((0, 0) = infinity, fp_inv_gcd as at the
// end of k_g1_lincomb) at out[v]: the layout launch_pairing_check reads, two consecutive vectors being one check's (A, B).
template <class C>
__global__ void __launch_bounds__(64)
k_g1_horner_wave(const uint32_t *__restrict__ bits, uint32_t nbits, uint32_t *__restrict__ out) {
  using CV = G1Curve<C>; using Fq = typename C::Fq; constexpr int N = Fq::N;
  const uint32_t v = blockIdx.x, q = threadIdx.x, m = (nbits + 63) / 64;
  const uint32_t *T = bits + (size_t)v * nbits * CV::ACC_WORDS;
  typename CV::acc_t acc = CV::identity();
#pragma unroll 1
  for (int i = (int)m - 1; i >= 0; i--) {
    const uint32_t p = q * m + (uint32_t)i;
    acc = CV::dbl(acc);
    if (p < nbits) acc = CV::add(acc, CV::load_acc(T + (size_t)p * CV::ACC_WORDS));
  }
#pragma unroll 1
  for (uint32_t s = 1; s < 64; s <<= 1) {
    typename CV::acc_t o = CV::shfl_down(acc, (int)s);                 // lane q + s
#pragma unroll 1
    for (uint32_t d = 0; d < s * m; d++) o = CV::dbl(o);
    acc = CV::add(acc, o);
  }
  if (q == 0) {
    uint32_t *o = out + (size_t)v * 2 * N;
    if (CV::is_identity(acc)) { fp_store<N>(o, fp_zero<N>()); fp_store<N>(o + N, fp_zero<N>()); }
    else {
      const fpn<N> inv = fp_inv_gcd<Fq>(fp_mul<Fq>(acc.zz, acc.zzz));
      fp_store<N>(o, fp_mul<Fq>(acc.x, fp_mul<Fq>(inv, acc.zzz)));       // X / ZZ
      fp_store<N>(o + N, fp_mul<Fq>(acc.y, fp_mul<Fq>(inv, acc.zz)));    // Y / ZZZ
    }
  }
}

// Fixed-base (table) batched MSMs have ONE bucket set per MSM: out[set] = sum_b b * B_b.  A group of 2^lps_log lanes
// (inside one wave) shares a set; lane g owns the m = nb >> lps_log consecutive buckets above g*m (running sums: 2 adds
// per bucket); then sum_g W_g + m * sum_g g * S_g by a group suffix scan and a group reduction.
template <class CV>
__global__ void __launch_bounds__(256, CV::RED_WAVES)
k_wsum(const uint32_t *__restrict__ buckets, uint32_t nb, uint32_t nsets, uint32_t lps_log, uint32_t *__restrict__ out) {
  using acc_t = typename CV::acc_t;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lps = 1u << lps_log, set = t >> lps_log, g = t & (lps - 1), m = nb >> lps_log;
  const bool live = set < nsets;
  acc_t S = CV::identity(), W = CV::identity();
  if (live) {
    const uint32_t *B = buckets + (size_t)set * nb * CV::ACC_WORDS;          // B[b-1]
    const uint32_t lo = g * m + 1;
#pragma unroll 1
    for (uint32_t b = lo + m - 1; b >= lo; b--) {                              // S = sum B_b, W = sum (b - g*m) B_b
      S = CV::add(S, CV::load_acc(B + (size_t)(b - 1) * CV::ACC_WORDS));
      W = CV::add(W, S);
    }
  }
  acc_t A = S;                                                                // suffix sums of S over the group
#pragma unroll 1
  for (uint32_t off = 1; off < lps; off <<= 1) {
    acc_t o = CV::shfl_down(A, off);
    if (g + off < lps) A = cv_add<CV>(A, o);
  }
  acc_t Z = g ? A : CV::identity();                                           // sum_g g * S_g = sum_{g >= 1} A_g
#pragma unroll 1
  for (uint32_t k = m; k > 1; k >>= 1) Z = cv_dbl<CV>(Z);
  acc_t V = cv_add<CV>(W, Z);
#pragma unroll 1
  for (uint32_t off = lps >> 1; off >= 1; off >>= 1) {
    acc_t o = CV::shfl_down(V, off);
    if (g + off < lps) V = cv_add<CV>(V, o);
  }
  if (live && g == 0) CV::store_out(out + (size_t)set * CV::OUT_WORDS, V);
}

// Same weighted sum with a whole workgroup (wps waves) per bucket set, for launches with few sets: lane t of the
// group owns m = nb / (64 wps) consecutive buckets; each wave reduces to (V_w, Y_w) = (sum_l W_l + m l S_l, sum_l S_l)
// as above, and lane 0 finishes sum_w V_w + 64 m sum_w w Y_w over the wps pairs left in LDS.
template <class CV>
__global__ void __launch_bounds__(256, CV::RED_WAVES)
k_wsum_blk(const uint32_t *__restrict__ buckets, uint32_t nb, uint32_t *__restrict__ out) {
  using acc_t = typename CV::acc_t;
  extern __shared__ uint32_t lds[];                                            // wps x {V, Y}
  const uint32_t set = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6, wps = blockDim.x >> 6;
  const uint32_t m = nb / blockDim.x;
  const uint32_t *B = buckets + (size_t)set * nb * CV::ACC_WORDS;              // B[b-1]
  acc_t S = CV::identity(), W = CV::identity();
  {
    const uint32_t lo = t * m + 1;
#pragma unroll 1
    for (uint32_t b = lo + m - 1; b >= lo; b--) {
      S = CV::add(S, CV::load_acc(B + (size_t)(b - 1) * CV::ACC_WORDS));
      W = CV::add(W, S);
    }
  }
  acc_t A = S;
#pragma unroll 1
  for (uint32_t off = 1; off < 64; off <<= 1) {
    acc_t o = CV::shfl_down(A, off);
    if (lane + off < 64) A = cv_add<CV>(A, o);
  }
  acc_t Z = lane ? A : CV::identity();
#pragma unroll 1
  for (uint32_t k = m; k > 1; k >>= 1) Z = cv_dbl<CV>(Z);
  acc_t V = cv_add<CV>(W, Z);
#pragma unroll 1
  for (uint32_t off = 32; off >= 1; off >>= 1) {
    acc_t o = CV::shfl_down(V, off);
    if (lane + off < 64) V = cv_add<CV>(V, o);
  }
  if (lane == 0) { CV::store_acc(lds + (2 * wv) * CV::ACC_WORDS, V); CV::store_acc(lds + (2 * wv + 1) * CV::ACC_WORDS, A); }
  __syncthreads();
  if (t == 0) {
    acc_t r = V, suf = CV::identity(), q = CV::identity();                     // q = sum_{w >= 1} w Y_w = sum of suffix sums
#pragma unroll 1
    for (uint32_t w = wps - 1; w >= 1; w--) {
      suf = cv_add<CV>(suf, CV::load_acc(lds + (2 * w + 1) * CV::ACC_WORDS));
      q = cv_add<CV>(q, suf);
      r = cv_add<CV>(r, CV::load_acc(lds + (2 * w) * CV::ACC_WORDS));
    }
#pragma unroll 1
    for (uint32_t k = 64 * m; k > 1; k >>= 1) q = cv_dbl<CV>(q);
    CV::store_out(out + (size_t)set * CV::OUT_WORDS, cv_add<CV>(r, q));
  }
}

// ---------------------------------------------------------------- host engine

// tuning knobs from the environment, read once per process
struct MsmEnv {
  int c = 0, per_min = 8, wsum_wps = 0, occ = 0, tile = 0; bool window_sums = true, tiny = true;
  size_t wsum_blk_max = 64;          // fixed-base launches of at most this many bucket sets take the workgroup-per-set weighted sum
  MsmEnv() {
    // 4 .. 15, the range of msm_plan's own choices; anything else leaves the choice to msm_plan (below 4 the window-sum form's host fold
    // -- 2^4 between P1 and P2 -- no longer fits a window; above 15 a bucket no longer fits a key)
    if (const char *e = getenv("AVRF_MSM_C")) { int v = atoi(e); if (v >= 4 && v <= 15) c = v; }
    if (const char *e = getenv("AVRF_MSM_OCC")) { int v = atoi(e); if (v >= 1 && v <= 8) occ = v; }   // resident k_accumulate waves per SIMD to fill
    if (const char *e = getenv("AVRF_MSM_TILE")) { int v = atoi(e); if (v >= 1024 && v <= (1 << 22)) tile = v; }       // keys per sort workgroup of a batched launch
    if (const char *e = getenv("AVRF_MSM_PER_MIN")) { int v = atoi(e); if (v >= 1 && v <= 4096) per_min = v; }
    if (const char *e = getenv("AVRF_TE_WSUM_WPS")) { int v = atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) wsum_wps = v; }
    if (const char *e = getenv("AVRF_TE_WINDOW_SUMS")) window_sums = atoi(e) != 0;
    if (const char *e = getenv("AVRF_G1_WSUM_BLK_MAX")) { int v = atoi(e); if (v >= 0 && v <= 65536) wsum_blk_max = (size_t)v; }
    if (const char *e = getenv("AVRF_MSM_TINY")) tiny = atoi(e) != 0;                    // (A/B hook: 0 sends small MSMs through the general chain too)
  }
};
static const MsmEnv &msm_env() { static const MsmEnv e; return e; }
// sort tile: keys per workgroup of k_hist / k_scatter.  2048 / 4096 / 8192 measured the same headline, single-context MSM time and ring
// rate (4096 moves 65 MB instead of 90 in k_scatter but doubles the histogram table); for the batched launches of the ring prover
// (>= 64 bucket sets: parallelism comes from the vectors) AVRF_MSM_TILE = 32 768 / 131 072 / one tile per vector were no faster on
// BLS12-381 and 5 % slower on BN254 (round 4: k_scatter moves 11 x its algorithmic bytes there, but it runs beside the other
// contexts' multiplier-bound k_accumulate, so its memory time is not on the critical path).
static uint32_t tile_len_for(size_t n, size_t vwin) { return vwin >= 64 && msm_env().tile ? (uint32_t)msm_env().tile : 8192u; }

MsmPlan msm_plan(size_t n, int scalar_bits) {
  MsmPlan p;
  int lg = 0; while (((size_t)1 << (lg + 1)) <= n) lg++;
  int c = lg >= 16 ? lg - 5 : lg - 3;                   // small (KZG-sized, batched) MSMs: ~8 entries per bucket
  if (c < 4) c = 4; if (c > 15) c = 15;
  p.c = msm_env().c ? msm_env().c : c; p.lpb = 0;
  p.nb = 1 << (p.c - 1);
  p.nwin = (scalar_bits + 1 + p.c - 1) / p.c;
  return p;
}


// lanes one residency round of k_accumulate<CV> holds on the current device (CUs x resident workgroups x 256), and the
// dynamic LDS bytes that hold the kernel to that many workgroups per CU.  The kernel uses no LDS; asking for a slice of the
// CU's 160 KB is how a launch is kept BELOW what its registers would allow (AVRF_MSM_OCC, or the policy's MAX_WAVES): with
// several contexts in flight the waves of a register-light k_accumulate otherwise take every slot of a SIMD and the other
// contexts' latency-bound kernels (hashing, sort, reductions) no longer overlap with it.
struct AccShape { size_t lanes; unsigned lds; };
template <class CV> static AccShape accumulate_shape() {
  static AccShape cache[64] = {};
  static std::mutex mu;                                                       // contexts call this from their own host threads
  int dev = 0; HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) dev = 0;
  std::lock_guard<std::mutex> lk(mu);
  if (!cache[dev].lanes) {
    int cus = 0, blocks = 0, lds_cu = 0, lds_blk = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_accumulate<CV>, 256, 0));
    if (blocks < 1) blocks = 1;
    // LDS of one CU and the most one workgroup may ask for (160 KB both on gfx950; the slice below is computed from what the
    // device reports, and the cap is skipped where a slice cannot be expressed)
    if (hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess || lds_cu <= 0) { (void)hipGetLastError(); lds_cu = 0; }
    if (hipDeviceGetAttribute(&lds_blk, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || lds_blk <= 0) { (void)hipGetLastError(); lds_blk = 64 * 1024; }
    {  // the runtime may report the 64 KB of older parts for gfx950, whose CUs have 160 KB (MI355X_MICROARCH.md)
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, dev) == hipSuccess && !strncmp(prop.gcnArchName, "gfx950", 6)) {
        if (lds_cu < 160 * 1024) lds_cu = 160 * 1024;
        if (lds_blk < 160 * 1024) lds_blk = 160 * 1024;
      } else (void)hipGetLastError();
    }
    int cap = CV::MAX_WAVES;                                                  // a block of 256 lanes = one wave on each of a CU's 4 SIMDs
    if (msm_env().occ) cap = msm_env().occ;
    unsigned lds = 0;
    if (cap >= 1 && cap < blocks && lds_cu > 0) {
      const unsigned slice = (unsigned)(lds_cu / (cap + 1) + 1024);           // cap + 1 slices do not fit, cap slices do
      if ((size_t)slice * cap <= (size_t)lds_cu && slice <= (unsigned)lds_blk) {
        blocks = cap; lds = slice;
        if (lds > 48 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *)k_accumulate<CV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      }
    }
    {   // the gather pipeline's two buffers per wave (k_accumulate): at least that much dynamic LDS; resident workgroups follow
      const unsigned need = 4u * 2u * CV::BASE_WORDS * 64u * 4u;
      if (lds < need) lds = need;
      if (lds > 48 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *)k_accumulate<CV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      int blk2 = 0;
      HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blk2, k_accumulate<CV>, 256, lds));
      if (blk2 >= 1 && blk2 < blocks) blocks = blk2;
    }
    cache[dev] = AccShape{(size_t)cus * blocks * 256, lds};
  }
  return cache[dev];
}

// AVRF_MSM_POISON=1 (debugging): fresh workspace memory is filled with 0xA5 bytes, so that a kernel that reads what no kernel wrote fails
// every time instead of depending on what the allocator hands back
static bool msm_poison() { static const bool on = getenv("AVRF_MSM_POISON") != nullptr; return on; }
static void poison(void *p, size_t bytes, int which) {
  if (!msm_poison() || !p) return;
  if (const char *e = getenv("AVRF_MSM_POISON_SKIP")) { if (atoi(e) == which) return; }
  HIP_CHECK(hipMemset(p, 0xA5, bytes)); if (!getenv("AVRF_MSM_POISON_NOSYNC")) HIP_CHECK(hipDeviceSynchronize());
}
// one buffer of the workspace: grow-only, exactly `bytes` when it grows; `which` is its number for the poison hook
static void ws_buf(DevMem &m, size_t bytes, int which) {
  if (bytes <= m.cap) return;
  m.ensure(bytes);
  poison(m.p, bytes, which);
}

// (buffers listed together grow together: their sizes rise and fall with the same quantity)
void MsmWorkspace::ensure(size_t n, const MsmPlan &p, size_t acc_bytes, size_t batch, size_t lanes_max, size_t part_bytes) {
  const size_t vwin = (size_t)p.nwin * batch;           // virtual windows
  const size_t nbk = vwin * p.nb, nbits = vwin * p.c;
  const size_t need_n = vwin * n;
  const size_t ntiles = (n + tile_len_for(n, vwin) - 1) / tile_len_for(n, vwin);
  ws_buf(keys, need_n * 2 + 16, 1); ws_buf(sorted, need_n * 4 + 16, 2);
  ws_buf(hist, nbk * ntiles * 4 + 64, 3);
  ws_buf(cnts, nbk * 4, 4); ws_buf(offsets, nbk * 4, 5); ws_buf(heavy, nbk * 4, 6);
  ws_buf(win_tot, (vwin + 64) * 4, 7); ws_buf(lane_base, (vwin + 64) * 4, 8);
  plan_dev.ensure(64);
  ws_buf(buckets, nbk * acc_bytes, 9); ws_buf(rc, nbk * acc_bytes, 10);               // rc: >= nwin * (NR + NC)
  ws_buf(part, (lanes_max + nbk + 64) * (part_bytes ? part_bytes : acc_bytes) + 64, 11);
  ws_buf(bits, nbits * acc_bytes, 12); own.ensure(nbits * acc_bytes);
}

void MsmChain::ensure(size_t bytes) {
  if (!plan_host) { plan_host.ensure(64); plan_host.as()[0] = plan_host.as()[1] = 0; }
  if (!ev0) { HIP_CHECK(ev0.create()); HIP_CHECK(ev1.create()); }
  bits_host.ensure(bytes);
}

// Collects the chain msm_device enqueued on `stream` with `rec` as its record and books its plan / k_accumulate timing on the lane.
// The workspace's own record: waits for the stream.  A caller's record: no wait, the caller has seen an event behind the chain complete.
static void msm_collect(MsmWorkspace &ws, MsmChain &rec, hipStream_t stream) {
  if (ws.owns(rec)) { HIP_CHECK(hipStreamSynchronize(stream)); HIP_CHECK(hipGetLastError()); }
  HIP_CHECK(hipEventElapsedTime(&ws.accum_ms_last, rec.ev0, rec.ev1));
  rec.plan.lpb = (int)rec.plan_host.as()[0];
  ws.accum_ms_total += ws.accum_ms_last; ws.accum_launches++; ws.last_plan = rec.plan;
}

// Small MSMs (a BatchVerifier of up to a few hundred items, ONE independent verification run as its own equation, the verifier's
// two G1 sums of a few ring proofs): the Pippenger chain below is twelve launches of latency there (0.28 ms for five terms) and
// almost no work.  One launch instead: wave (p, v) sums the bases whose scalar of vector v has bit p set -- lane = term, a
// butterfly of ceil(log2 n) additions -- which are exactly the bit sums T_p the general path hands to the host's Horner
// (sum_p 2^p T_p; the sequential doublings run ~10 x faster on a host core than on a lone wave).
// (Up to 2 048 terms with workgroups of up to four waves -- one per SIMD, the whole register file each: a thread takes the terms
// t, t + T, .., the waves' sums meet in LDS --
// the reference's own batch-size sweep, 1 .. 256 items per BatchVerifier, benches/SUMMARY.md:43-61, lives entirely in this range.
// Above it the bit sums cost too much work -- n * bits / 2 additions against n * windows -- and the Pippenger chain takes over.)
constexpr size_t MSM_TINY_TERMS = 2048, MSM_TINY_VECTORS = 32;
template <class CV>
__global__ void __launch_bounds__(256)
k_msm_tiny_bits(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ scalars, uint32_t n, uint32_t stride, uint32_t *__restrict__ out) {
  extern __shared__ uint32_t lds[];                                            // one accumulator per wave
  const uint32_t p = blockIdx.x, v = blockIdx.y, t = threadIdx.x, T = blockDim.x, lane = t & 63, wv = t >> 6, nw = T >> 6;
  typename CV::acc_t acc = CV::identity();
  bool first = true;
#pragma unroll 1
  for (uint32_t k = t; k < n; k += T) {
    if (!((scalars[8 * ((size_t)v * stride + k) + (p >> 5)] >> (p & 31)) & 1u)) continue;
    const typename CV::base_t q = CV::load_base(bases + (size_t)k * CV::BASE_WORDS);
    acc = first ? CV::from_base(q, false) : CV::madd(acc, q, false);
    first = false;
  }
  uint32_t span = 1; while (span < n && span < 64) span <<= 1;
#pragma unroll 1
  for (uint32_t off = span >> 1; off >= 1; off >>= 1) acc = cv_add<CV>(acc, CV::shfl_down(acc, (int)off));
  if (nw > 1) {
    if (lane == 0) CV::store_acc(lds + wv * CV::ACC_WORDS, acc);
    __syncthreads();
    if (wv == 0) {
      acc = lane < nw ? CV::load_acc(lds + lane * CV::ACC_WORDS) : CV::identity();
#pragma unroll 1
      for (uint32_t off = nw >> 1; off >= 1; off >>= 1) acc = cv_add<CV>(acc, CV::shfl_down(acc, (int)off));
    }
  }
  if (t == 0) CV::store_acc(out + ((size_t)v * gridDim.x + p) * CV::ACC_WORDS, acc);
}

// What msm_device is told beyond bases, scalars and the lane.  The defaults: one scalar vector over plain bases, waited for.
struct MsmLaunch {
  size_t batch = 1;                      // scalar vectors of length n over the SAME n bases (d_scalars = batch x n x 8 words): every vector gets its own nwin windows
  // fixed-base mode (table_c != 0): d_bases is a window table T[w * table_stride + i] = 2^(table_c * w) * P_i, so all windows of a
  // vector share ONE bucket set: downstream it is a 1-window MSM over n * nwin (table) bases
  int table_c = 0; size_t table_stride = 0;
  size_t scalar_stride = 0;              // vector b's scalars start at element b * scalar_stride (0: n)
  const uint32_t *d_base_idx = nullptr;  // sparse form (msm.h msm_g1_fixed_device)
  bool defer = false;                    // everything up to the copies back is enqueued, nothing is waited for: the caller collects later (msm_collect)
  int scalars_mont = 0;                  // the scalars are Montgomery limbs (msm.h msm_g1_fixed_device)
  size_t base_stride = 0;                // segmented form (msm.h msm_te_segments): vector v multiplies bases [v * base_stride, v * base_stride + n); 0: shared bases
  uint32_t *d_affine_out = nullptr;      // segmented G1 form (msm.h msm_g1_segments): where the device leaves the finished affine points (nullptr: ws.rc)
};

// The six chains of msm_device, named by what ends them; msm_tail is the one place that decides between them.
enum class MsmTail { SINGLE_LAUNCH, WINDOW_TRIPLES, TABLE_WSUM, DEVICE_HORNER, G1_HORNER_AFFINE, HOST_BITS };
template <class CV> static MsmTail msm_tail(size_t n, const MsmLaunch &o) {
  const bool plain = !o.table_c && !o.d_base_idx && !o.scalars_mont && !o.base_stride;
  if (plain && n <= MSM_TINY_TERMS && o.batch <= MSM_TINY_VECTORS && msm_env().tiny) return MsmTail::SINGLE_LAUNCH;   // k_msm_tiny_bits alone: bit sums
  if (CV::WINDOW_SUMS && o.batch == 1 && msm_env().window_sums) return MsmTail::WINDOW_TRIPLES;                        // three points per window
  if (CV::FIXED_TABLE && o.table_c) return MsmTail::TABLE_WSUM;                       // one weighted sum per bucket set: a finished point per vector
  if (!CV::FIXED_TABLE && o.base_stride) return MsmTail::DEVICE_HORNER;   // segmented (msm_te_segments only: G1 does not build this tail's kernels): device bit sums and Horner
  if (CV::FIXED_TABLE && o.base_stride) return MsmTail::G1_HORNER_AFFINE;  // segmented G1 (msm_g1_segments only): device bit sums, a wave's Horner and affine point per vector
  return MsmTail::HOST_BITS;                                                          // k_rowcol / k_bits: the bit sums of every vector
}
// what the stages of one chain share: the lane, the record, the launch and, for the general chain, the plan with the sizes derived from it
struct MsmRun {
  MsmWorkspace &ws; MsmChain &rec; hipStream_t stream; const MsmLaunch &o;
  MsmPlan p;
  size_t n;                    // keys per virtual window (fixed-base mode: n_in * digit windows)
  uint32_t vwin, nbk;          // virtual windows (nwin per vector) | buckets of all of them
  size_t acc_bytes;            // one accumulator of the reduction kernels
  uint32_t tile_len, ntiles;   // keys per sort workgroup | sort workgroups per virtual window
};
// the one way results leave the device: the copy back and, with it, the description of what the copy carries
static void copy_back(MsmChain &rec, const DevMem &from, const MsmResult &res, hipStream_t stream) {
  rec.res = res;
  HIP_CHECK(hipMemcpyAsync(rec.bits_host.p, from.p, res.vectors * res.stride() * res.words * 4, hipMemcpyDeviceToHost, stream));
}
template <class CV> static void chain_single_launch(const uint32_t *d_bases, const uint32_t *d_scalars, size_t n, int scalar_bits, MsmRun &r) {
  r.p.c = 1; r.p.nwin = scalar_bits; r.p.nb = 1; r.p.lpb = 0;
  const size_t acc_b = (size_t)CV::ACC_WORDS * 4, nbits = (size_t)scalar_bits;
  r.ws.ensure(n, r.p, acc_b, r.o.batch, 256);
  r.rec.ensure(r.o.batch * nbits * acc_b); r.rec.plan_host.as()[0] = 0; r.rec.plan = r.p;
  HIP_CHECK(hipEventRecord(r.rec.ev0, r.stream));
  unsigned threads = 64; while (threads < n && threads < 256) threads <<= 1;           // a power of two of waves: the LDS butterfly halves it
  hipLaunchKernelGGL(k_msm_tiny_bits<CV>, dim3((unsigned)nbits, (unsigned)r.o.batch), dim3(threads), (threads / 64) * acc_b, r.stream, d_bases, d_scalars, (uint32_t)n,
                     (uint32_t)(r.o.scalar_stride ? r.o.scalar_stride : n), r.ws.bits.as());
  HIP_CHECK(hipEventRecord(r.rec.ev1, r.stream));
  copy_back(r.rec, r.ws.bits, MsmResult{MsmResult::BIT_SUMS, r.o.batch, nbits, (size_t)CV::ACC_WORDS}, r.stream);
}
// the sort: digits -> keys, per-tile histograms, offsets, the lanes' plan, entries grouped by (virtual window, bucket) in ws.sorted
static void chain_sort(const uint32_t *d_scalars, size_t n_in, int dig_nwin, size_t lanes_target, const MsmRun &r) {
  MsmWorkspace &ws = r.ws; const MsmLaunch &o = r.o; const MsmPlan &p = r.p; hipStream_t stream = r.stream;
  const dim3 b256(256);
  const size_t lds_bytes = (size_t)p.nb * 4;
  // fixed-base mode: key (window w, term i) gathers table entry w * table_stride + i
  const uint32_t remap_n = o.table_c ? (uint32_t)n_in : 0, remap_stride = o.table_c ? (uint32_t)o.table_stride : 0;
  hipLaunchKernelGGL(k_digits, dim3((unsigned)((n_in + 255) / 256), (unsigned)o.batch), b256, 0, stream, d_scalars, (uint32_t)n_in,
                     (uint32_t)(o.scalar_stride ? o.scalar_stride : n_in), p.c, dig_nwin, ws.keys.as<uint16_t>(), o.scalars_mont);
  hipLaunchKernelGGL(k_hist, dim3(r.ntiles, r.vwin), b256, lds_bytes, stream, ws.keys.as<uint16_t>(), (uint32_t)r.n, r.tile_len, p.c, ws.hist.as());
  hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)((p.nb + 255) / 256), r.vwin), b256, 0, stream, ws.hist.as(), r.ntiles, p.c, ws.cnts.as());
  hipLaunchKernelGGL(k_scan_offs, dim3(r.vwin), dim3(1024), 0, stream, ws.cnts.as(), (uint32_t)r.n, p.c, ws.offsets.as(), ws.win_tot.as());
  hipLaunchKernelGGL(k_plan, dim3(1), dim3(1024), 0, stream, ws.win_tot.as(), r.vwin, (uint32_t)lanes_target, (uint32_t)msm_env().per_min,
                     ws.lane_base.as(), ws.plan_dev.as());
  hipLaunchKernelGGL(k_scatter, dim3(8u * ((r.vwin + 7u) / 8u) * r.ntiles), b256, lds_bytes, stream, ws.keys.as<uint16_t>(), (uint32_t)r.n, r.tile_len, p.c, ws.hist.as(),
                     ws.offsets.as(), ws.sorted.as(), remap_n, remap_stride, o.d_base_idx, r.ntiles, r.vwin, (uint32_t)p.nwin, (uint32_t)o.base_stride);
}
template <class BV> static void bucket_sums(const MsmRun &r) {
  hipLaunchKernelGGL(k_bucket_sum<BV>, dim3((r.nbk + 255) / 256), dim3(256), 0, r.stream, r.ws.offsets.as(), r.ws.cnts.as(), r.ws.lane_base.as(), r.ws.plan_dev.as(), r.nbk,
                     (uint32_t)r.p.nb, (uint32_t)r.n, r.ws.part.as(), r.ws.buckets.as(), r.ws.heavy.as());
  hipLaunchKernelGGL(k_heavy_sum<BV>, dim3(r.nbk < 1024 ? r.nbk : 1024), dim3(256), 4 * r.acc_bytes, r.stream, r.ws.offsets.as(), r.ws.cnts.as(), r.ws.lane_base.as(),
                     r.ws.plan_dev.as(), (uint32_t)r.p.nb, (uint32_t)r.n, r.ws.part.as(), r.ws.buckets.as(), r.ws.heavy.as());
}
// the accumulation (bracketed by the record's events), the bucket sums into ws.buckets and the plan's copy back
// (red: the reduction kernels run over CV::red -- G1 in fixed-base mode: general additions on the unsaturated limbs, buckets in raw limbs)
template <class CV> static void chain_accumulate(const uint32_t *d_bases, size_t lanes_max, bool red, const MsmRun &r) {
  r.rec.ensure((size_t)r.vwin * 3 * r.acc_bytes);   // the window triples, which are all a caller's record is sent (the workspace's own is sized with `bits`)
  if (CV::ZERO_IS_IDENTITY) HIP_CHECK(hipMemsetAsync(r.ws.buckets.p, 0, (size_t)r.nbk * r.acc_bytes, r.stream));   // empty buckets
  HIP_CHECK(hipEventRecord(r.rec.ev0, r.stream));
  hipLaunchKernelGGL(k_accumulate<CV>, dim3((unsigned)((lanes_max + 255) / 256)), dim3(256), accumulate_shape<CV>().lds, r.stream, d_bases, r.ws.sorted.as(),
                     r.ws.offsets.as(), r.ws.win_tot.as(), r.ws.lane_base.as(), r.ws.plan_dev.as(), r.vwin, (uint32_t)r.p.nb, (uint32_t)r.n, r.ws.part.as());
  HIP_CHECK(hipEventRecord(r.rec.ev1, r.stream));
  if (red) bucket_sums<typename CV::red>(r); else bucket_sums<CV>(r);
  HIP_CHECK(hipMemcpyAsync(r.rec.plan_host.p, r.ws.plan_dev.p, 8, hipMemcpyDeviceToHost, r.stream));
  r.rec.plan = r.p;
}
// weighted bucket sum of every window with the four-lanes-per-point kernels (te_quad.h): three points per window come
// back; the host folds them into its window Horner (scales 1, 2^4, 16 m), so the device does no doublings at all
template <class CV> static void tail_window_triples(const MsmRun &r) {
  const uint32_t nb = (uint32_t)r.p.nb;
  const uint32_t wpw = nb >= 256 ? 16u : 1u, m = nb >= 256 ? nb / 256 : (nb >= 16 ? nb / 16 : 1u), nwaves = r.vwin * wpw;
  hipLaunchKernelGGL(k_wsum_q1<typename CV::suite>, dim3((nwaves + 3) / 4), dim3(256), 0, r.stream, r.ws.buckets.as(), nb, m, wpw, nwaves, r.ws.rc.as());
  hipLaunchKernelGGL(k_wsum_q2<typename CV::suite>, dim3(r.vwin), dim3(64), 0, r.stream, r.ws.rc.as(), wpw, r.ws.bits.as());
  int lg = 4; while ((1u << lg) < 16 * m) lg++;
  copy_back(r.rec, r.ws.bits, MsmResult{MsmResult::WINDOW_TRIPLES, 1, r.vwin, (size_t)CV::ACC_WORDS, lg}, r.stream);
}
// one bucket set per MSM: weighted sum in one kernel, no bit sums
template <class CV> static void tail_table_wsum(const MsmRun &r) {
  using RV = typename CV::red;
  const size_t batch = r.o.batch; const uint32_t nb = (uint32_t)r.p.nb;
  uint32_t wps = 1;                                      // waves per bucket set when the launch has few sets
  // (a wave per set does the least work per bucket -- 2.5 adds against 4.4 with four waves -- and measured faster as
  // soon as a few hundred sets are in flight; the workgroup form is for the handful of sets of a single proof)
  // (round 3 re-check with 512-set launches, which fill only half the SIMDs with one wave per set: two waves per set 12.4 k proofs/s,
  // four 11.9 k against 12.6-12.7 k -- with several contexts in flight the idle SIMDs are not idle, total work decides)
  const uint32_t wps_max = batch <= msm_env().wsum_blk_max ? 4 : 1;
  while (wps < wps_max && nb >= 64 * wps * 2) wps *= 2;
  if (wps > 1) {
    hipLaunchKernelGGL(k_wsum_blk<RV>, dim3((unsigned)batch), dim3(64 * wps), (size_t)wps * 2 * r.acc_bytes, r.stream, r.ws.buckets.as(), nb, r.ws.rc.as());
  } else {
    uint32_t lps_log = 6;                                // lanes per bucket set: enough waves to cover the chip, <= nb
    while (lps_log > 2 && (batch << (lps_log - 1)) >= 2048 * 64) lps_log--;
    while ((1u << lps_log) > nb) lps_log--;
    hipLaunchKernelGGL(k_wsum<RV>, dim3((unsigned)(((batch << lps_log) + 255) / 256)), dim3(256), 0, r.stream, r.ws.buckets.as(), nb, (uint32_t)batch, lps_log, r.ws.rc.as());
  }
  copy_back(r.rec, r.ws.rc, MsmResult{MsmResult::POINTS, batch, 1, (size_t)RV::OUT_WORDS}, r.stream);
}
// the bit sums T_k (sum_b b B_b = sum_k 2^k T_k) of every virtual window into ws.bits, rows and columns of the bucket grid first
template <class CV> static void rowcol_bits(const MsmRun &r) {
  const int c = r.p.c, h = (c - 1) / 2;
  const uint32_t tasks = (1u << h) + ((uint32_t)r.p.nb >> h), nbits = r.vwin * (uint32_t)c;
  hipLaunchKernelGGL(k_rowcol<CV>, dim3(((size_t)r.vwin * tasks * 64 + 255) / 256), dim3(256), 0, r.stream, r.ws.buckets.as(), c, h, r.vwin * tasks, r.ws.rc.as());
  hipLaunchKernelGGL(k_bits<CV>, dim3(((size_t)nbits * 64 + 255) / 256), dim3(256), 0, r.stream, r.ws.buckets.as(), r.ws.rc.as(), c, h, nbits, r.ws.bits.as());
}
// segmented launch: the bit sums in one kernel while a window's buckets allow it, the Horner on the device, only `batch` points come back
template <class CV> static void tail_device_horner(const MsmRun &r) {
  const uint32_t nbits = r.vwin * (uint32_t)r.p.c, vbits = (uint32_t)(r.p.nwin * r.p.c), batch = (uint32_t)r.o.batch;
  if (r.p.nb <= 256) hipLaunchKernelGGL(k_bits_direct<CV>, dim3((nbits + 127) / 128), dim3(128), 0, r.stream, r.ws.buckets.as(), r.p.c, nbits, r.ws.bits.as());
  else rowcol_bits<CV>(r);
  if constexpr (CV::QUAD) hipLaunchKernelGGL(k_horner_quads<typename CV::suite>, dim3(batch), dim3(64), 0, r.stream, r.ws.bits.as(), vbits, r.ws.rc.as());   // a wave per MSM (te_quad.h)
  else hipLaunchKernelGGL(k_horner<CV>, dim3((batch + 63) / 64), dim3(64), 0, r.stream, r.ws.bits.as(), vbits, batch, r.ws.rc.as());                      // a lane per MSM
  r.rec.ensure((size_t)batch * r.acc_bytes);   // the `batch` finished points, whoever's record it is (chain_accumulate sized it for the window triples already: no growth here)
  copy_back(r.rec, r.ws.rc, MsmResult{MsmResult::POINTS, batch, 1, (size_t)CV::ACC_WORDS}, r.stream);
}
// segmented G1 launch (msm_g1_segments keeps nb <= 256): the bit sums in one kernel, Horner and affine conversion by a wave per vector;
// the `batch` Montgomery affine points stay on the device (o.d_affine_out, or ws.rc) for a kernel behind this chain and come back as well
template <class CV> static void tail_g1_horner_affine(const MsmRun &r) {
  const uint32_t nbits = r.vwin * (uint32_t)r.p.c, vbits = (uint32_t)(r.p.nwin * r.p.c), batch = (uint32_t)r.o.batch;
  uint32_t *d_out = r.o.d_affine_out ? r.o.d_affine_out : r.ws.rc.as();
  hipLaunchKernelGGL(k_bits_direct<CV>, dim3((nbits + 127) / 128), dim3(128), 0, r.stream, r.ws.buckets.as(), r.p.c, nbits, r.ws.bits.as());
  hipLaunchKernelGGL(k_g1_horner_wave<typename CV::curve>, dim3(batch), dim3(64), 0, r.stream, r.ws.bits.as(), vbits, d_out);
  r.rec.res = MsmResult{MsmResult::AFFINE, batch, 1, (size_t)CV::BASE_WORDS};
  r.rec.ensure((size_t)batch * CV::BASE_WORDS * 4);
  HIP_CHECK(hipMemcpyAsync(r.rec.bits_host.p, d_out, (size_t)batch * CV::BASE_WORDS * 4, hipMemcpyDeviceToHost, r.stream));
}
// Enqueues the device pipeline of o.batch MSMs: the single launch, or sort, accumulation and the tail msm_tail picks; collects it unless
// o.defer.  `rec`: the workspace's own record or a caller's (window-sum form and the segmented chain's device Horner only).  Throws HipFailure when a HIP call fails.
template <class CV>
static void msm_device(const uint32_t *d_bases, const uint32_t *d_scalars, size_t n_in, int scalar_bits, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream,
                       const MsmLaunch &o = MsmLaunch()) {
  const MsmTail tail = msm_tail<CV>(n_in, o);
  MsmRun r{ws, rec, stream, o, msm_plan(n_in, scalar_bits), n_in};
  if (tail == MsmTail::SINGLE_LAUNCH) chain_single_launch<CV>(d_bases, d_scalars, n_in, scalar_bits, r);
  else {
    MsmPlan &p = r.p;
    int dig_nwin = p.nwin;
    if (o.table_c) {
      dig_nwin = (scalar_bits + 1 + o.table_c - 1) / o.table_c;
      p.c = o.table_c; p.nb = 1 << (o.table_c - 1); p.nwin = 1;
      r.n = n_in * (size_t)dig_nwin;                                      // one window of n_in * dig_nwin keys per vector
    }
    const bool red = tail == MsmTail::TABLE_WSUM;
    r.acc_bytes = (size_t)(red ? (int)CV::red::ACC_WORDS : (int)CV::ACC_WORDS) * 4;
    r.vwin = (uint32_t)(p.nwin * o.batch); r.nbk = r.vwin * p.nb;
    const size_t lanes_target = accumulate_shape<CV>().lanes, lanes_max = lanes_target + r.vwin + 256;   // sum_v ceil(tot_v / per) <= total / per + vwin
    if ((size_t)r.vwin * r.n >= 0xffff0000ull) throw HipFailure{hipErrorInvalidValue, __FILE__, __LINE__};   // 32-bit entry offsets
    ws.ensure(r.n, p, r.acc_bytes, o.batch, lanes_max, (size_t)CV::accum::PART_WORDS * 4);
    r.tile_len = tile_len_for(r.n, r.vwin); r.ntiles = (uint32_t)((r.n + r.tile_len - 1) / r.tile_len);
    chain_sort(d_scalars, n_in, dig_nwin, lanes_target, r);
    chain_accumulate<CV>(d_bases, lanes_max, red, r);
    // a caller's record is taken by the tails that size it: the window triples and the finished points of the segmented chain
    if (tail != MsmTail::WINDOW_TRIPLES && tail != MsmTail::DEVICE_HORNER && !ws.owns(rec)) throw HipFailure{hipErrorInvalidValue, __FILE__, __LINE__};
    if constexpr (CV::WINDOW_SUMS) if (tail == MsmTail::WINDOW_TRIPLES) tail_window_triples<CV>(r);
    if constexpr (CV::FIXED_TABLE) if (tail == MsmTail::TABLE_WSUM) tail_table_wsum<CV>(r);
    if constexpr (!CV::FIXED_TABLE) if (tail == MsmTail::DEVICE_HORNER) tail_device_horner<CV>(r);
    if constexpr (CV::FIXED_TABLE) if (tail == MsmTail::G1_HORNER_AFFINE) tail_g1_horner_affine<CV>(r);
    if (tail == MsmTail::HOST_BITS) { rowcol_bits<CV>(r); copy_back(r.rec, ws.bits, MsmResult{MsmResult::BIT_SUMS, o.batch, (size_t)(p.nwin * p.c), (size_t)CV::ACC_WORDS}, r.stream); }
  }
  if (!o.defer) msm_collect(ws, rec, stream);
}
// Vector v of a COLLECTED record as a point of the host group HG (HostTe<S> or HostG1<C>), according to the form the chain's tail left.
template <class HG> static auto msm_fold(const MsmChain &rec, size_t v) {
  const MsmResult &r = rec.res;
  const uint32_t *bh = rec.bits_host.as() + v * r.stride() * r.words;
  auto acc = HG::identity();
  auto step = [&](int dbls, size_t i) { while (dbls-- > 0) acc = HG::dbl(acc); acc = HG::add(acc, HG::from_raw32(bh + i * r.words)); };   // acc = 2^dbls acc + point i
  const int c = rec.plan.c, lg = r.lg;
  if (r.form == MsmResult::POINTS) return HG::from_raw32(bh);
  if (r.form == MsmResult::BIT_SUMS) for (size_t i = r.per; i-- > 0;) step(1, i);                       // bit sums T_p: sum_p 2^p T_p
  else for (size_t w = r.per; w-- > 0;) { step(c - lg, 3 * w + 2); step(lg - 4, 3 * w + 1); step(4, 3 * w); }   // window triples: W_w = P1 + 2^4 P2 + 2^lg P3; sum_w 2^(c w) W_w
  return acc;
}

template <class S>
static int msm_te_enqueue_impl(const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t n, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream) {
  rec.n = n; rec.armed = true;
  MsmLaunch o; o.defer = true;
  if (n) msm_device<TeCurve<S>>((const uint32_t *)d_pre, d_scalars, n, S::Fr::BITS, ws, rec, stream, o);
  return 0;
}
template <class S>
static int msm_te_finish_impl(MsmWorkspace &ws, MsmChain &rec, hipStream_t stream, HostExt *out) {
  *out = HostTe<S>::identity();
  if (!rec.armed) return -1;                              // nothing was enqueued (or another call consumed the chain): an error, never the identity
  rec.disarm();
  if (rec.n == 0) return 0;
  msm_collect(ws, rec, stream);
  *out = msm_fold<HostTe<S>>(rec, 0);
  return 0;
}

template <class F> static int te_call(int suite, F f) { return suite < 0 || suite >= AVRF_N_SUITES ? -1 : with_suite(suite, f); }   // a suite id out of range answers -1
int msm_te_enqueue(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t n, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream) {
  return te_call(suite, [&](auto tag) { using S = typename decltype(tag)::type; return msm_te_enqueue_impl<S>(d_pre, d_scalars, n, ws, rec, stream); });
}
int msm_te_finish(int suite, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream, HostExt *out) {
  return te_call(suite, [&](auto tag) { using S = typename decltype(tag)::type; return msm_te_finish_impl<S>(ws, rec, stream, out); });
}
template <class S>
static int msm_te_small_vectors_impl(const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t n, size_t nv, MsmWorkspace &ws, hipStream_t stream, HostExt *out) {
  if (!n || n > MSM_TINY_TERMS || !nv || nv > MSM_TINY_VECTORS || !msm_env().tiny) return -1;
  MsmLaunch o; o.batch = nv; o.scalar_stride = n;
  msm_device<TeCurve<S>>((const uint32_t *)d_pre, d_scalars, n, S::Fr::BITS, ws, ws.own, stream, o);
  ws.own.disarm();
  parallel_for(nv, [&](size_t v) { out[v] = msm_fold<HostTe<S>>(ws.own, v); });   // the vectors' Horners side by side
  return 0;
}
int msm_te_small_vectors(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t n, size_t n_vectors, MsmWorkspace &ws, hipStream_t stream,
                         HostExt *out) {
  return te_call(suite, [&](auto tag) { using S = typename decltype(tag)::type; return msm_te_small_vectors_impl<S>(d_pre, d_scalars, n, n_vectors, ws, stream, out); });
}
// n_seg independent MSMs of L terms each in ONE chain: vector v over bases of its own (MsmLaunch::base_stride), bucket sums by
// k_bits_direct (L <= 8191 keeps nb <= 256), the Horner on the device, n_seg finished points back.  The chain comes in two halves, as
// msm_te_enqueue / msm_te_finish do: everything launched and `defer`red, then collected and folded.  The enqueue form runs ONE chain
// whatever n_seg >= 1 is; every limit is checked before anything is launched.
template <class S>
static int msm_te_segments_enqueue_impl(const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t L, size_t n_seg, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream) {
  if (L > MSM_SEG_TERMS_MAX || n_seg * L > 0x7fffffffull) return -1;
  const size_t vwin = n_seg * (size_t)msm_plan(L ? L : 1, S::Fr::BITS).nwin;
  // k_hist / k_scan_tiles take the virtual window as blockIdx.y; the sorted array is addressed by 32-bit entry offsets
  if (L && (vwin > MSM_SEG_WINDOWS_MAX || vwin * L >= 0xffff0000ull)) return -1;
  rec.n = n_seg * L; rec.armed = true;
  rec.res = MsmResult{MsmResult::POINTS, n_seg, 1, (size_t)TeCurve<S>::ACC_WORDS};   // what the tail's copy back will say again; all there is to say when no term exists
  MsmLaunch o; o.batch = n_seg; o.scalar_stride = L; o.base_stride = L; o.defer = true;
  if (rec.n) msm_device<TeCurve<S>>((const uint32_t *)d_pre, d_scalars, L, S::Fr::BITS, ws, rec, stream, o);
  return 0;
}
template <class S>
static int msm_te_segments_finish_impl(MsmWorkspace &ws, MsmChain &rec, hipStream_t stream, HostExt *out) {
  if (!rec.armed) return -1;                              // nothing was enqueued (or another call consumed the chain): an error, never identities
  rec.disarm();
  const size_t n_seg = rec.res.vectors;
  if (rec.n == 0) { for (size_t v = 0; v < n_seg; v++) out[v] = HostTe<S>::identity(); return 0; }
  msm_collect(ws, rec, stream);
  for (size_t v = 0; v < n_seg; v++) out[v] = msm_fold<HostTe<S>>(rec, v);
  return 0;
}
int msm_te_segments_enqueue(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t L, size_t n_seg, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream) {
  return te_call(suite, [&](auto tag) { using S = typename decltype(tag)::type; return msm_te_segments_enqueue_impl<S>(d_pre, d_scalars, L, n_seg, ws, rec, stream); });
}
int msm_te_segments_finish(int suite, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream, HostExt *out) {
  return te_call(suite, [&](auto tag) { using S = typename decltype(tag)::type; return msm_te_segments_finish_impl<S>(ws, rec, stream, out); });
}
// The synchronous call.  Fewer than MSM_SEG_CHAIN_MIN vectors loop the single-MSM path instead of the chain; the threshold has not
// been measured, and this is the one place it is written.
constexpr size_t MSM_SEG_CHAIN_MIN = 8;
template <class S>
static int msm_te_segments_impl(const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t L, size_t n_seg, MsmWorkspace &ws, hipStream_t stream, HostExt *out) {
  using HT = HostTe<S>;
  for (size_t v = 0; v < n_seg; v++) out[v] = HT::identity();
  if (!L || !n_seg) return 0;
  if (L > MSM_SEG_TERMS_MAX || n_seg * L > 0x7fffffffull) return -1;
  if (n_seg < MSM_SEG_CHAIN_MIN) {
    for (size_t v = 0; v < n_seg; v++) {
      if (int e = msm_te_enqueue_impl<S>(d_pre + v * L, d_scalars + 8 * v * L, L, ws, ws.own, stream)) return e;
      if (int e = msm_te_finish_impl<S>(ws, ws.own, stream, out + v)) return e;
    }
    return 0;
  }
  if (int e = msm_te_segments_enqueue_impl<S>(d_pre, d_scalars, L, n_seg, ws, ws.own, stream)) return e;
  return msm_te_segments_finish_impl<S>(ws, ws.own, stream, out);
}
int msm_te_segments(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t L, size_t n_seg, MsmWorkspace &ws, hipStream_t stream, HostExt *out) {
  return te_call(suite, [&](auto tag) { using S = typename decltype(tag)::type; return msm_te_segments_impl<S>(d_pre, d_scalars, L, n_seg, ws, stream, out); });
}
int msm_segments_window_bits(size_t L) { return msm_plan(L, 256).c; }
bool msm_te_pending_supported(int suite) {
  if (suite < 0 || suite >= AVRF_N_SUITES || !msm_env().window_sums) return false;
  return with_suite(suite, [&](auto tag) { using S = typename decltype(tag)::type; return (bool)TeCurve<S>::WINDOW_SUMS; });
}
int msm_te_device(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t n,
                  MsmWorkspace &ws, hipStream_t stream, HostExt *out) {
  if (int e = msm_te_enqueue(suite, d_pre, d_scalars, n, ws, ws.own, stream)) return e;
  return msm_te_finish(suite, ws, ws.own, stream, out);
}

// ---------------------------------------------------------------- G1 (KZG) MSM

// canonical affine coordinates (x || y, FQ_BYTES little-endian each; (0,0) = infinity) -> Montgomery bases
template <class C>
__global__ void __launch_bounds__(256) k_g1_bases(const uint8_t *__restrict__ xy, uint32_t n, uint32_t *__restrict__ out, uint32_t *__restrict__ flag) {
  using Fq = typename C::Fq; constexpr int N = Fq::N;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t *src = reinterpret_cast<const uint32_t *>(xy + (size_t)i * N * 8);
  fpn<N> x = fp_load<N>(src), y = fp_load<N>(src + N);
  if (ge_p<Fq>(x) || ge_p<Fq>(y)) atomicOr(flag, 1u);
  fp_store<N>(out + (size_t)i * 2 * N, fp_to_mont<Fq>(x)); fp_store<N>(out + (size_t)i * 2 * N + N, fp_to_mont<Fq>(y));
}

// CanonicalDeserialize of compressed G1 points (ark-serialize; the zcash big-endian form for BLS12-381, little-endian with the
// flags in the last byte for BN254 -- SURVEY.md A.1), one lane per point: x from the bytes, y = (x^3 + b)^((p + 1) / 4)
// (p = 3 mod 4 for both fields), sign by the "lexicographically largest" flag.  out_xy = x || y canonical little-endian
// ((0, 0) for the point at infinity), ok[i] = 0 undecodable / not on the curve, 1 a point, 2 infinity.  The ring verifiers
// need the y coordinates on the HOST too (their transcript absorbs uncompressed points), so the result goes back; a 381-bit
// square root is ~570 field multiplications, 60 us on a host core.
template <class C>
__global__ void __launch_bounds__(64) k_g1_decompress(const uint8_t *__restrict__ comp, uint32_t n, uint8_t *__restrict__ out_xy, uint8_t *__restrict__ ok) {
  using Fq = typename C::Fq; constexpr int N = Fq::N, FQB = 4 * N;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t *b = comp + (size_t)i * FQB;
  uint8_t le[FQB]; bool big, inf;
  if (FQB == 48) {
    inf = b[0] & 0x40; big = b[0] & 0x20;
    if (!(b[0] & 0x80)) { ok[i] = 0; return; }
    for (int k = 0; k < FQB; k++) le[k] = b[FQB - 1 - k];
    le[FQB - 1] &= 0x1f;
  } else {
    inf = b[FQB - 1] & 0x40; big = b[FQB - 1] & 0x80;
    for (int k = 0; k < FQB; k++) le[k] = b[k];
    le[FQB - 1] &= 0x3f;
  }
  fpn<N> x;
  for (int k = 0; k < N; k++) x.v[k] = (uint32_t)le[4 * k] | ((uint32_t)le[4 * k + 1] << 8) | ((uint32_t)le[4 * k + 2] << 16) | ((uint32_t)le[4 * k + 3] << 24);
  uint32_t *o = reinterpret_cast<uint32_t *>(out_xy + (size_t)i * 2 * FQB);
  if (inf) {                                                          // canonical encoding only: no sort flag, every other bit zero
    const bool good = !big && fp_is_zero(x);
    fp_store<N>(o, fp_zero<N>()); fp_store<N>(o + N, fp_zero<N>());
    ok[i] = good ? 2 : 0; return;
  }
  if (ge_p<Fq>(x)) { ok[i] = 0; return; }
  const fpn<N> xm = fp_to_mont<Fq>(x);
  const fpn<N> rhs = fp_add<Fq>(fp_mul<Fq>(fp_sqr<Fq>(xm), xm), fp_const<Fq>(C::B));
  uint32_t e[N];                                                      // (p + 1) / 4 = ((p - 1) / 2 + 1) / 2
  { uint64_t c = 1; for (int k = 0; k < N; k++) { c += Fq::HALF[k]; e[k] = (uint32_t)c; c >>= 32; } }
  for (int k = 0; k < N; k++) e[k] = (e[k] >> 1) | (k + 1 < N ? e[k + 1] << 31 : 0u);
  fpn<N> y = fp_one<Fq>();
#pragma unroll 1
  for (int k = 32 * N - 1; k >= 0; k--) {
    y = fp_sqr<Fq>(y);
    if ((e[k >> 5] >> (k & 31)) & 1) y = fp_mul<Fq>(y, rhs);
  }
  if (!fp_eq(fp_sqr<Fq>(y), rhs)) { ok[i] = 0; return; }             // not on the curve
  fpn<N> yp = fp_from_mont<Fq>(y);
  bool is_big = false;                                                // yp > (p - 1) / 2 ?
  for (int k = N - 1; k >= 0; k--) if (yp.v[k] != Fq::HALF[k]) { is_big = yp.v[k] > Fq::HALF[k]; break; }
  if (is_big != big) yp = fp_from_mont<Fq>(fp_neg<Fq>(y));
  fp_store<N>(o, x); fp_store<N>(o + N, yp);
  ok[i] = 1;
}

// Fixed-base window table over `n` affine bases: table[w * n + i] = 2^(c w) * P_i, w < nwin, affine Montgomery.
// One lane per base walks its nwin rows twice: forwards it leaves X, Y in the table slot and ZZ, ZZZ and the running product of
// the ZZ ZZZ before the row in `tmp` (3 N words per entry); ONE inversion of the lane's total; backwards it peels 1 / (ZZ ZZZ)
// off row by row (Montgomery's trick) and normalises.  (Two inversions per entry -- 1 140 of the ~1 230 multiplications an
// entry cost -- made the two tables of a ring setup 84 ms of a 2 048-proof profile.)
template <class C>
__global__ void __launch_bounds__(64)
k_g1_table(const uint32_t *__restrict__ bases, uint32_t n, int c, int nwin, uint32_t *__restrict__ table, uint32_t *__restrict__ tmp) {
  using CV = G1Curve<C>; using Fq = typename C::Fq; constexpr int N = Fq::N;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typename CV::base_t b = CV::load_base(bases + (size_t)i * 2 * N);
  typename CV::acc_t acc = CV::from_affine(b);
  fpn<N> run = fp_one<Fq>();
#pragma unroll 1
  for (int w = 0; w < nwin; w++) {
    const size_t e = (size_t)w * n + i;
    fp_store<N>(table + e * 2 * N, acc.x); fp_store<N>(table + e * 2 * N + N, acc.y);
    fp_store<N>(tmp + e * 3 * N, acc.zz); fp_store<N>(tmp + e * 3 * N + N, acc.zzz); fp_store<N>(tmp + e * 3 * N + 2 * N, run);
    if (!CV::is_identity(acc)) run = fp_mul<Fq>(run, fp_mul<Fq>(acc.zz, acc.zzz));
    if (w + 1 < nwin) for (int k = 0; k < c; k++) acc = CV::dbl(acc);
  }
  fpn<N> inv = fp_inv_gcd<Fq>(run);
#pragma unroll 1
  for (int w = nwin - 1; w >= 0; w--) {
    const size_t e = (size_t)w * n + i;
    uint32_t *o = table + e * 2 * N;
    const fpn<N> zz = fp_load<N>(tmp + e * 3 * N), zzz = fp_load<N>(tmp + e * 3 * N + N);
    if (fp_is_zero(zz)) { fp_store<N>(o, fp_zero<N>()); fp_store<N>(o + N, fp_zero<N>()); continue; }
    const fpn<N> dinv = fp_mul<Fq>(inv, fp_load<N>(tmp + e * 3 * N + 2 * N));     // 1 / (ZZ ZZZ) of this row
    inv = fp_mul<Fq>(inv, fp_mul<Fq>(zz, zzz));
    fp_store<N>(o, fp_mul<Fq>(fp_load<N>(o), fp_mul<Fq>(dinv, zzz)));             // X / ZZ
    fp_store<N>(o + N, fp_mul<Fq>(fp_load<N>(o + N), fp_mul<Fq>(dinv, zz)));      // Y / ZZZ
  }
}

void build_g1_table(int curve, const uint32_t *d_bases, size_t n, int c, int nwin, uint32_t *d_table, hipStream_t stream) {
  if (!n) return;
  const size_t fqn = curve == 0 ? G1Bls12381::Fq::N : G1Bn254::Fq::N;
  // Plain scratch, the stream waited for, then freed: setup-time work.  (Until round 6 the scratch came from the stream-ordered pool --
  // hipMallocAsync / hipFreeAsync -- so that the build stayed asynchronous.  Next to the synchronous hipMalloc / hipFree of the MSM
  // workspaces that was a race: after two setups on two streams the first batched commitment of avrf_ring_srs_generate returned the
  // point at infinity for its first vector, every time, and not with HIP_LAUNCH_BLOCKING=1 or a device synchronisation in between
  // (tests/test_gpu_ring.py::test_srs_generate caught it once an unrelated null-stream hipMemset, which had been hiding it, went away).)
  // (owned: a throw between the allocation and the free -- a launch or the wait failing -- does not leak it)
  DevMem tmp((size_t)nwin * n * 3 * fqn * 4);
  dim3 g((unsigned)((n + 63) / 64)), b(64);
  if (curve == 0) hipLaunchKernelGGL(k_g1_table<G1Bls12381>, g, b, 0, stream, d_bases, (uint32_t)n, c, nwin, d_table, tmp.as());
  else hipLaunchKernelGGL(k_g1_table<G1Bn254>, g, b, 0, stream, d_bases, (uint32_t)n, c, nwin, d_table, tmp.as());
  HIP_CHECK(hipStreamSynchronize(stream));
  HIP_CHECK(tmp.release());
}

// The G1 tail: every vector of the collected record to a point, all of them to affine bytes.
template <class C> static void g1_results(const MsmChain &rec, size_t batch, uint8_t *out_xy) {
  using HG = HostG1<C>;
  std::vector<typename HG::Pt> res(batch);
  auto fold = [&](size_t b) { res[b] = msm_fold<HG>(rec, b); };
  // (a few vectors of bit sums: their Horners -- as many doublings and additions as a vector has bit sums -- run side by side)
  if (rec.res.form == MsmResult::BIT_SUMS && batch >= 2) parallel_for(batch, fold);
  else for (size_t b = 0; b < batch; b++) fold(b);
  HG::to_affine_bytes_batch(res.data(), batch, out_xy);
}
template <class C>
static int msm_g1_impl(const uint32_t *d_bases, const uint32_t *d_scalars, size_t n, MsmWorkspace &ws, hipStream_t stream, uint8_t *out_xy, const MsmLaunch &o) {
  if (!n) { memset(out_xy, 0, o.batch * 8 * C::Fq::N); return 0; }   // no terms: the point at infinity (all-zero x || y) for every vector
  msm_device<G1Curve<C>>(d_bases, d_scalars, n, C::Fr::BITS, ws, ws.own, stream, o);
  g1_results<C>(ws.own, o.batch, out_xy);
  return 0;
}

// Prime-order-subgroup test of BLS12-381 G1 points (cofactor ~2^126, so curve membership is not enough; the reference gets
// it from ark-serialize's Validate::Yes when it deserialises a RingProof / RingCommitment, src/ring.rs:97-150):
//   P in G1  <=>  phi(P) = [-z^2] P,  phi(x, y) = (beta x, y),  z = 0xd201000000010000  (Scott 2021, "A note on group
// membership tests for G1, G2 and GT on BLS pairing-friendly curves"): two 64-bit double-and-add ladders instead of a
// 255-bit one.  One lane per point; (0, 0) = infinity passes.  BN254 G1 has cofactor 1: nothing to test.
__device__ static const uint32_t BLS12_381_BETA_MONT[12] = {0x798a64e8, 0x30f1361b, 0x7ece5a2a, 0xf3b8ddab, 0xc61577f7, 0x16a8ca3a,
                                                            0x74fd029b, 0xc26a2ff8, 0x60701c6e, 0x3636b766, 0x241b6160, 0x051ba4ab};
// (0, 0) = infinity passes
AVRF_DI bool g1_bls_in_subgroup(const G1Curve<G1Bls12381>::base_t &P) {
  using CV = G1Curve<G1Bls12381>; using Fq = G1Bls12381::Fq; constexpr int N = Fq::N;
  if (fp_is_zero(P.x) && fp_is_zero(P.y)) return true;
  const uint64_t z = 0xd201000000010000ull;
  CV::acc_t a = CV::from_affine(P);
#pragma unroll 1
  for (int b = 62; b >= 0; b--) { a = CV::dbl(a); if ((z >> b) & 1) a = CV::madd(a, P, false); }
  const CV::acc_t q1 = a;                                                   // [z] P
#pragma unroll 1
  for (int b = 62; b >= 0; b--) { a = CV::dbl(a); if ((z >> b) & 1) a = CV::add(a, q1); }      // [z^2] P
  fpn<N> beta; for (int k = 0; k < N; k++) beta.v[k] = BLS12_381_BETA_MONT[k];
  // [z^2] P == (beta x, -y)  in XYZZ:  X = beta x ZZ,  Y = -y ZZZ,  ZZ != 0
  bool ok = !fp_is_zero(a.zz);
  ok = ok && fp_eq(a.x, fp_mul<Fq>(fp_mul<Fq>(beta, P.x), a.zz));
  ok = ok && fp_eq(a.y, fp_neg<Fq>(fp_mul<Fq>(P.y, a.zzz)));
  return ok;
}
__global__ void __launch_bounds__(64)
k_g1_subgroup_bls(const uint32_t *__restrict__ bases, uint32_t n, uint32_t *__restrict__ flag, int32_t *__restrict__ rec_status, uint32_t ppr) {
  using CV = G1Curve<G1Bls12381>; constexpr int N = G1Bls12381::Fq::N;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!g1_bls_in_subgroup(CV::load_base(bases + (size_t)i * 2 * N))) { atomicOr(flag, 2u); if (rec_status) rec_status[i / ppr] = 2; }
}
// the same test for a LIST of points of records of unequal length: entry i tests base point[i] and pins a failure on record rec_of[i]
__global__ void __launch_bounds__(64)
k_g1_subgroup_bls_list(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ point, const uint32_t *__restrict__ rec_of, uint32_t n,
                       uint32_t *__restrict__ flag, int32_t *__restrict__ rec_status) {
  using CV = G1Curve<G1Bls12381>; constexpr int N = G1Bls12381::Fq::N;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!g1_bls_in_subgroup(CV::load_base(bases + (size_t)point[i] * 2 * N))) { atomicOr(flag, 2u); rec_status[rec_of[i]] = 2; }
}
void launch_g1_subgroup_check(int curve, const uint32_t *d_bases, size_t n, uint32_t *d_flag, hipStream_t stream, int32_t *d_rec_status, uint32_t ppr) {
  if (!n || curve != 0) return;
  hipLaunchKernelGGL(k_g1_subgroup_bls, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d_bases, (uint32_t)n, d_flag, d_rec_status, ppr ? ppr : 1u);
}
void launch_g1_subgroup_check_list(int curve, const uint32_t *d_bases, const uint32_t *d_point, const uint32_t *d_rec_of, size_t n, uint32_t *d_flag,
                                   int32_t *d_rec_status, hipStream_t stream) {
  if (!n || curve != 0) return;
  hipLaunchKernelGGL(k_g1_subgroup_bls_list, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, d_bases, d_point, d_rec_of, (uint32_t)n, d_flag, d_rec_status);
}

// Small linear combinations, one 16-lane group per item: lane t < tpi computes scalar_t * P_t, lanes [0, split) are summed into
// point 0, lanes [split, tpi) into point 1; both leave as Montgomery affine x | y ((0, 0) = infinity) at
// out[(2 item + q) * 2N] -- the two G1 arguments of an independent KZG pairing check (RingVerifier::verify, src/ring.rs:242),
// whose bases differ per item so that no bucket method applies.
// GLV (BLS12-381): phi(x, y) = (beta x, y) multiplies by -z^2 on G1 (the relation k_g1_subgroup_bls tests), so with
// k = k1 + k2 z^2 (k1 = k mod z^2, k2 = k div z^2, both < 2^128; the caller splits, scalars arrive as k1 | k2 << 128)
// k P = k1 P + k2 (-phi(P)): one chain of 128 doublings over the joint 2-bit table {i P + j (beta x, -y)} instead of 255
// doublings with a wave-divergent addition behind each.  Without GLV: 255-bit double-and-add.
template <class C, bool GLV>
__global__ void __launch_bounds__(64)
k_g1_lincomb(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ scalars, uint32_t n_items, uint32_t tpi, uint32_t split,
             uint32_t *__restrict__ out) {
  using CV = G1Curve<C>; using Fq = typename C::Fq; constexpr int N = Fq::N;
  const uint32_t lane = threadIdx.x & 63, k = lane & 15;
  uint32_t item = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const bool live = item < n_items;
  if (!live) item = n_items - 1;
  typename CV::acc_t acc = CV::identity();
  if (k < tpi) {
    const size_t t = (size_t)item * tpi + k;
    const typename CV::base_t P = CV::load_base(bases + t * 2 * N);
    uint32_t sc[8];
    { const uint4 *sp = reinterpret_cast<const uint4 *>(scalars + t * 8); uint4 a = sp[0], b = sp[1];
      sc[0] = a.x; sc[1] = a.y; sc[2] = a.z; sc[3] = a.w; sc[4] = b.x; sc[5] = b.y; sc[6] = b.z; sc[7] = b.w; }
    if constexpr (GLV && N == 12) {
      typename CV::base_t Q;                                           // -phi(P)
      { fpn<N> beta;
#pragma unroll
        for (int i = 0; i < N; i++) beta.v[i] = BLS12_381_BETA_MONT[i];
        Q.x = fp_mul<Fq>(beta, P.x); Q.y = fp_neg<Fq>(P.y);
        if (fp_is_zero(P.x) && fp_is_zero(P.y)) Q = P; }               // infinity stays infinity
      typename CV::acc_t tab[16];                                      // tab[4 j + i] = i P + j Q (per-lane scratch)
      tab[0] = CV::identity(); tab[4] = CV::from_affine(Q);
      tab[8] = CV::madd(tab[4], Q, false); tab[12] = CV::madd(tab[8], Q, false);
#pragma unroll 1
      for (int j = 0; j < 4; j++)
#pragma unroll 1
        for (int i = 1; i < 4; i++) tab[4 * j + i] = CV::madd(tab[4 * j + i - 1], P, false);
#pragma unroll 1
      for (int w = 63; w >= 0; w--) {
        acc = CV::dbl(CV::dbl(acc));
        const uint32_t d1 = (sc[w >> 4] >> (2 * (w & 15))) & 3u, d2 = (sc[4 + (w >> 4)] >> (2 * (w & 15))) & 3u;
        if (d1 | d2) acc = CV::add(acc, tab[4 * d2 + d1]);
      }
    } else {
#pragma unroll 1
      for (int bit = 255; bit >= 0; bit--) {
        acc = CV::dbl(acc);
        if ((sc[bit >> 5] >> (bit & 31)) & 1) acc = CV::madd(acc, P, false);
      }
    }
  }
  // lanes 0 and `split` gather their segment (the other lanes add along and are ignored)
#pragma unroll 1
  for (uint32_t t = 1; t < 16; t++) {
    uint32_t src = k < split ? t : split + t;
    const bool inside = k < split ? src < split : src < tpi;
    if (src > 15) src = 15;
    typename CV::acc_t o;
#pragma unroll
    for (int i = 0; i < N; i++) {
      o.x.v[i] = __shfl(acc.x.v[i], src, 16); o.y.v[i] = __shfl(acc.y.v[i], src, 16);
      o.zz.v[i] = __shfl(acc.zz.v[i], src, 16); o.zzz.v[i] = __shfl(acc.zzz.v[i], src, 16);
    }
    if ((k == 0 || k == split) && inside) acc = CV::add(acc, o);
  }
  if (live && (k == 0 || k == split)) {
    uint32_t *o = out + ((size_t)item * 2 + (k == 0 ? 0 : 1)) * 2 * N;
    if (CV::is_identity(acc)) { fp_store<N>(o, fp_zero<N>()); fp_store<N>(o + N, fp_zero<N>()); }
    else {
      const fpn<N> inv = fp_inv_gcd<Fq>(fp_mul<Fq>(acc.zz, acc.zzz));
      fp_store<N>(o, fp_mul<Fq>(acc.x, fp_mul<Fq>(inv, acc.zzz)));       // X / ZZ
      fp_store<N>(o + N, fp_mul<Fq>(acc.y, fp_mul<Fq>(inv, acc.zz)));    // Y / ZZZ
    }
  }
}
void launch_g1_lincomb(int curve, const uint32_t *d_bases, const uint32_t *d_scalars, size_t n_items, uint32_t tpi, uint32_t split, uint32_t *d_out,
                       hipStream_t stream, bool glv_split_scalars) {
  if (!n_items) return;
  const dim3 grid((unsigned)((n_items * 16 + 63) / 64)), block(64);
  if (curve == 0 && glv_split_scalars) hipLaunchKernelGGL((k_g1_lincomb<G1Bls12381, true>), grid, block, 0, stream, d_bases, d_scalars, (uint32_t)n_items, tpi, split, d_out);
  else if (curve == 0) hipLaunchKernelGGL((k_g1_lincomb<G1Bls12381, false>), grid, block, 0, stream, d_bases, d_scalars, (uint32_t)n_items, tpi, split, d_out);
  else hipLaunchKernelGGL((k_g1_lincomb<G1Bn254, false>), grid, block, 0, stream, d_bases, d_scalars, (uint32_t)n_items, tpi, split, d_out);
}

void g1_glv_split_bls(uint64_t k[4]) {
  const uint64_t z = 0xd201000000010000ull;
  uint64_t q1[4], q2[4];                                            // q1 = k div z, q2 = q1 div z; floor(floor(k / z) / z) = floor(k / z^2)
  unsigned __int128 rem = 0;
  for (int i = 3; i >= 0; i--) { unsigned __int128 cur = (rem << 64) | k[i]; q1[i] = (uint64_t)(cur / z); rem = cur % z; }
  rem = 0;
  for (int i = 3; i >= 0; i--) { unsigned __int128 cur = (rem << 64) | q1[i]; q2[i] = (uint64_t)(cur / z); rem = cur % z; }
  // k1 = k - q2 z^2 (fits 128 bits): low 128 bits of the difference
  const unsigned __int128 z2 = (unsigned __int128)z * z, q = ((unsigned __int128)q2[1] << 64) | q2[0];
  const unsigned __int128 klo = ((unsigned __int128)k[1] << 64) | k[0];
  const unsigned __int128 k1 = klo - q * z2;                         // mod 2^128; exact because k1 < z^2 < 2^128
  k[0] = (uint64_t)k1; k[1] = (uint64_t)(k1 >> 64); k[2] = q2[0]; k[3] = q2[1];
}

void launch_g1_decompress(int curve, const uint8_t *d_comp, size_t n, uint8_t *d_out_xy, uint8_t *d_ok, hipStream_t stream) {
  if (!n) return;
  dim3 g((unsigned)((n + 63) / 64)), b(64);
  if (curve == 0) hipLaunchKernelGGL(k_g1_decompress<G1Bls12381>, g, b, 0, stream, d_comp, (uint32_t)n, d_out_xy, d_ok);
  else hipLaunchKernelGGL(k_g1_decompress<G1Bn254>, g, b, 0, stream, d_comp, (uint32_t)n, d_out_xy, d_ok);
}

void launch_g1_bases(int curve, const uint8_t *d_xy, size_t n, uint32_t *d_out, uint32_t *d_flag, hipStream_t stream) {
  if (!n) return;
  dim3 g((unsigned)((n + 255) / 256)), b(256);
  if (curve == 0) hipLaunchKernelGGL(k_g1_bases<G1Bls12381>, g, b, 0, stream, d_xy, (uint32_t)n, d_out, d_flag);
  else hipLaunchKernelGGL(k_g1_bases<G1Bn254>, g, b, 0, stream, d_xy, (uint32_t)n, d_out, d_flag);
}

int msm_g1_device(int curve, const uint32_t *d_bases, const uint32_t *d_scalars, size_t n, MsmWorkspace &ws, hipStream_t stream, uint8_t *out_xy,
                  size_t batch, size_t scalar_stride) {
  MsmLaunch o; o.batch = batch; o.scalar_stride = scalar_stride;
  if (curve == 0) return msm_g1_impl<G1Bls12381>(d_bases, d_scalars, n, ws, stream, out_xy, o);
  if (curve == 1) return msm_g1_impl<G1Bn254>(d_bases, d_scalars, n, ws, stream, out_xy, o);
  return -1;
}
// n_seg independent G1 MSMs of L terms each in ONE chain, beside msm_te_segments and under its limits (all checked before anything is
// launched): vector v over bases of its own (MsmLaunch::base_stride), the sort, k_accumulate<G1Curve<C>> and the bucket sums of every G1
// chain, bit sums by k_bits_direct, then k_g1_horner_wave.  Always the chain, whatever n_seg >= 1 is.  Collects (synchronises the stream).
template <class C>
static int msm_g1_segments_impl(const uint32_t *d_bases, const uint32_t *d_scalars, size_t L, size_t n_seg, MsmWorkspace &ws, hipStream_t stream, uint8_t *out_xy,
                                uint32_t *d_out) {
  using Fq = HostField<typename C::Fq>; constexpr size_t B = 4 * C::Fq::N;
  if (L > MSM_SEG_TERMS_MAX || n_seg * L > 0x7fffffffull) return -1;
  const size_t vwin = n_seg * (size_t)msm_plan(L ? L : 1, C::Fr::BITS).nwin;
  if (L && (vwin > MSM_SEG_WINDOWS_MAX || vwin * L >= 0xffff0000ull)) return -1;
  if (!L || !n_seg) {                                    // no terms: the point at infinity for every vector
    if (out_xy) memset(out_xy, 0, n_seg * 2 * B);
    if (d_out && n_seg) HIP_CHECK(hipMemsetAsync(d_out, 0, n_seg * 2 * B, stream));
    return 0;
  }
  MsmLaunch o; o.batch = n_seg; o.scalar_stride = L; o.base_stride = L; o.d_affine_out = d_out;
  msm_device<G1Curve<C>>(d_bases, d_scalars, L, C::Fr::BITS, ws, ws.own, stream, o);
  ws.own.disarm();
  for (size_t v = 0; out_xy && v < n_seg; v++) {         // Montgomery affine -> canonical bytes; (0, 0) stays all-zero
    typename Fq::El x, y; memcpy(x.l, ws.own.bits_host.as<uint8_t>() + v * 2 * B, B); memcpy(y.l, ws.own.bits_host.as<uint8_t>() + v * 2 * B + B, B);
    x = Fq::from_mont(x); y = Fq::from_mont(y);
    memcpy(out_xy + v * 2 * B, x.l, B); memcpy(out_xy + v * 2 * B + B, y.l, B);
  }
  return 0;
}
int msm_g1_segments(int curve, const uint32_t *d_bases, const uint32_t *d_scalars, size_t L, size_t n_seg, MsmWorkspace &ws, hipStream_t stream, uint8_t *out_xy,
                    uint32_t *d_out) {
  if (curve == 0) return msm_g1_segments_impl<G1Bls12381>(d_bases, d_scalars, L, n_seg, ws, stream, out_xy, d_out);
  if (curve == 1) return msm_g1_segments_impl<G1Bn254>(d_bases, d_scalars, L, n_seg, ws, stream, out_xy, d_out);
  return -1;
}
int msm_g1_segments_windows(int curve, size_t L) { return msm_plan(L ? L : 1, curve == 0 ? G1Bls12381::Fr::BITS : G1Bn254::Fr::BITS).nwin; }
// ---------------------------------------------------------------- fixed-base MSM over a table of ALL multiples (no buckets, no sort)
//
// A KZG commitment is an MSM over ONE fixed base set (the SRS), and an MI355X has 288 GB of HBM.  G1DirectTable holds, for every
// window row w and base i, every multiple m 2^(c w) P_i a signed c-bit digit can ask for (m = 1 .. 2^(c-1)): a commitment is then the
// plain SUM of one table point per (coefficient, row) -- n * rows mixed additions into per-lane accumulators and a tree over the lanes'
// partial sums.  No digit sort, no bucket sums, no weighted bucket reduction (the latter two were a quarter of the ring prover's device
// time), and the window can be as wide as memory allows: c = 15 for the 6 145 powers of a ring-1024 setup = 17 rows instead of the 22 of
// the 12-bit bucket form (1.71 G points, 164 GB).  The gathers are random 96-byte reads over the whole table: 12.7 G/s measured on a
// 200 GB table (tools/gather_probe.hip, profiles/r6_gather_probe.txt), four times what 24 k proofs/s ask for, 8 us each -- covered by
// the LDS-DMA prefetch of k_accumulate, whose addition takes longer than that.
//   layout: point (w, m, i) = (m + 1) 2^(c w) P_i at t.off[w] + m * n + i (affine Montgomery, (0, 0) = infinity): a build step writes
//   whole rows of bases at a time.  Rows: R = ceil(bits / c) digit rows; the top one holds only the multiples its digits can reach, and a
//   carry row (one multiple) follows when the signed recoding can carry out of it.
template <class C> static void direct_shape(size_t n, int c, G1DirectTable *t) {
  constexpr int BITS = C::Fr::BITS;
  const int R = (BITS + c - 1) / c;
  const uint32_t nb = 1u << (c - 1);
  // largest digit of the top row: (r - 1) >> (c (R - 1)), plus the carry coming in
  uint32_t top = 0;
  { const int bit = c * (R - 1); uint64_t w[9] = {}; for (int k = 0; k < 8; k++) w[k] = C::Fr::P[k];
    uint64_t borrow = 1; for (int k = 0; k < 8; k++) { const uint64_t d = w[k] - borrow; borrow = w[k] < borrow; w[k] = d & 0xffffffffu; }     // r - 1
    const int li = bit >> 5, sh = bit & 31; const uint64_t two = w[li] | (w[li + 1] << 32); top = (uint32_t)((two >> sh) & ((1ull << c) - 1)) + 1u; }
  t->c = c; t->n = n; t->rows = R;
  uint64_t off = 0;
  for (int w = 0; w < R; w++) { t->mult[w] = (w + 1 < R) ? nb : (top <= nb ? top : nb); t->off[w] = off; off += (uint64_t)t->mult[w] * n; }
  if (top > nb) { t->mult[R] = 1; t->off[R] = off; off += n; t->rows = R + 1; }
  t->points = off; t->bytes = off * 2 * C::Fq::N * 4;
}
size_t g1_direct_table_shape(int curve, size_t n, int c, G1DirectTable *t) {
  G1DirectTable tmp; if (!t) t = &tmp;
  t->curve = curve;
  if (curve == 0) direct_shape<G1Bls12381>(n, c, t); else direct_shape<G1Bn254>(n, c, t);
  return t->bytes;
}

// One lane per (row, base): the multiples m0 + 1 .. m0 + K of its base, as k_g1_table normalises a lane's rows -- X, Y into the table
// slot, ZZ, ZZZ and the running product into tmp, ONE inversion per lane and chunk, Montgomery's trick backwards.
template <class C>
__global__ void __launch_bounds__(64)
k_g1_multiples(const uint32_t *__restrict__ rowbase, uint32_t n, uint32_t rows, G1DirectTable t, uint32_t m0, uint32_t K, uint32_t *__restrict__ table,
               uint32_t *__restrict__ tmp, uint32_t lanes) {
  using CV = G1Curve<C>; using Fq = typename C::Fq; constexpr int N = Fq::N;
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= lanes) return;
  const uint32_t w = lane / n, i = lane - w * n;
  if (m0 >= t.mult[w]) return;
  const uint32_t kend = m0 + K < t.mult[w] ? m0 + K : t.mult[w];
  const typename CV::base_t B = CV::load_base(rowbase + ((size_t)w * n + i) * 2 * N);
  typename CV::acc_t acc = CV::from_affine(B);
  if (m0) acc = CV::madd(CV::from_affine(CV::load_base(table + (t.off[w] + (uint64_t)(m0 - 1) * n + i) * 2 * N)), B, false);
  fpn<N> run = fp_one<Fq>();
#pragma unroll 1
  for (uint32_t m = m0; m < kend; m++) {
    uint32_t *o = table + (t.off[w] + (uint64_t)m * n + i) * 2 * N;
    uint32_t *q = tmp + ((size_t)(m - m0) * lanes + lane) * 3 * N;
    fp_store<N>(o, acc.x); fp_store<N>(o + N, acc.y);
    fp_store<N>(q, acc.zz); fp_store<N>(q + N, acc.zzz); fp_store<N>(q + 2 * N, run);
    if (!CV::is_identity(acc)) run = fp_mul<Fq>(run, fp_mul<Fq>(acc.zz, acc.zzz));
    if (m + 1 < kend) acc = m == 0 ? CV::dbl(acc) : CV::madd(acc, B, false);
  }
  fpn<N> inv = fp_inv_gcd<Fq>(run);
#pragma unroll 1
  for (uint32_t m = kend; m-- > m0;) {
    uint32_t *o = table + (t.off[w] + (uint64_t)m * n + i) * 2 * N;
    const uint32_t *q = tmp + ((size_t)(m - m0) * lanes + lane) * 3 * N;
    const fpn<N> zz = fp_load<N>(q), zzz = fp_load<N>(q + N);
    if (fp_is_zero(zz)) { fp_store<N>(o, fp_zero<N>()); fp_store<N>(o + N, fp_zero<N>()); continue; }
    const fpn<N> dinv = fp_mul<Fq>(inv, fp_load<N>(q + 2 * N));              // 1 / (ZZ ZZZ) of this multiple
    inv = fp_mul<Fq>(inv, fp_mul<Fq>(zz, zzz));
    fp_store<N>(o, fp_mul<Fq>(fp_load<N>(o), fp_mul<Fq>(dinv, zzz)));        // X / ZZ
    fp_store<N>(o + N, fp_mul<Fq>(fp_load<N>(o + N), fp_mul<Fq>(dinv, zz)));  // Y / ZZZ
  }
}
template <class C> static void build_direct_impl(const uint32_t *d_bases, G1DirectTable *t, hipStream_t stream) {
  constexpr int N = C::Fq::N;
  const size_t n = t->n; const uint32_t rows = (uint32_t)t->rows;
  if (t->points >= 0x7fffffffull) throw HipFailure{hipErrorInvalidValue, __FILE__, __LINE__};     // 31-bit entry indices
  HIP_CHECK(hipMalloc(&t->d, t->bytes));
  // transient scratch (include/avrf.h, resource contract): the window rows of the bases (2 Fq per lane), then K multiples' ZZ / ZZZ /
  // running products per lane (3 Fq each) -- 386 Fq per (row, base) at the peak; build_g1_table's own scratch is gone by then
  DevMem rowbase((size_t)rows * n * 2 * N * 4);
  build_g1_table(t->curve, d_bases, n, t->c, (int)rows, rowbase.as(), stream);
  const uint32_t lanes = (uint32_t)(rows * n), K = 128;
  DevMem tmp((size_t)K * lanes * 3 * N * 4);
  uint32_t mmax = 0; for (uint32_t w = 0; w < rows; w++) mmax = t->mult[w] > mmax ? t->mult[w] : mmax;
  for (uint32_t m0 = 0; m0 < mmax; m0 += K)
    hipLaunchKernelGGL(k_g1_multiples<C>, dim3((lanes + 63) / 64), dim3(64), 0, stream, (const uint32_t *)rowbase.as(), (uint32_t)n, rows, *t, m0, K, t->d, tmp.as(), lanes);
  HIP_CHECK(hipStreamSynchronize(stream));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(tmp.release()); HIP_CHECK(rowbase.release());
}
void build_g1_direct_table(int curve, const uint32_t *d_bases, size_t n, int c, G1DirectTable *t, hipStream_t stream) {
  free_g1_direct_table(t);                           // (a table this struct held before is not leaked by a rebuild into it)
  g1_direct_table_shape(curve, n, c, t);
  if (curve == 0) build_direct_impl<G1Bls12381>(d_bases, t, stream); else build_direct_impl<G1Bn254>(d_bases, t, stream);
}
void free_g1_direct_table(G1DirectTable *t) { if (t->d) (void)hipFree(t->d); t->d = nullptr; }

constexpr uint32_t DIRECT_ZERO = 0xffffffffu;
// entry (vector, coefficient i, row w) -> table index | sign << 31 (DIRECT_ZERO for a zero digit); the digits are k_digits' signed recoding
// (base_idx != nullptr: the sparse form -- entry i of vector b multiplies table base base_idx[b * n + i])
__global__ void __launch_bounds__(256) k_direct_index(const uint32_t *__restrict__ scalars, uint32_t n, uint32_t stride, G1DirectTable t, uint32_t *__restrict__ idx, int mont,
                                                      const uint32_t *__restrict__ base_idx) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t bat = blockIdx.y, rows = (uint32_t)t.rows, tn = (uint32_t)t.n;
  const int c = t.c;
  uint32_t s[9];
  const uint4 *p = reinterpret_cast<const uint4 *>(scalars + 8 * ((size_t)bat * stride + i));
  const uint4 a = p[0], b = p[1];
  s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w; s[8] = 0;
  if (mont) {
    fp v;
#pragma unroll
    for (int k = 0; k < 8; k++) v.v[k] = s[k];
    v = mont == 1 ? fp_from_mont<FqBandersnatch>(v) : fp_from_mont<FqBabyJubJub>(v);
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = v.v[k];
  }
  uint32_t *o = idx + ((size_t)bat * n + i) * rows;
  const uint32_t ib = base_idx ? base_idx[(size_t)bat * n + i] : i;
  const uint32_t nb = 1u << (c - 1), mask = (1u << c) - 1;
  uint32_t carry = 0;
  for (uint32_t w = 0; w < rows; w++) {
    const int bit = (int)w * c;
    uint32_t v = 0;
    if (bit < 256) {
      const int li = bit >> 5, sh = bit & 31;
      const uint64_t two = (uint64_t)s[li] | ((uint64_t)(li + 1 < 9 ? s[li + 1] : 0u) << 32);
      v = (uint32_t)(two >> sh) & mask;
    }
    v += carry;
    uint32_t m, sign = 0;
    if (v > nb) { m = (1u << c) - v; sign = 0x80000000u; carry = 1; } else { m = v; carry = 0; }
    // (a scalar below r never asks a row for more than it holds: direct_shape sized the top row and the carry row from r - 1)
    o[w] = (m == 0 || m > t.mult[w] || ib >= tn) ? DIRECT_ZERO : (uint32_t)(t.off[w] + (uint64_t)(m - 1) * tn + ib) | sign;
  }
}

// Lane t sums the table points of the entries [e0, e1) of ONE vector (t / lpv); its partial sum goes to part[t].  The gather
// pipeline is k_accumulate's: the point of entry k + 1 travels HBM -> LDS by DMA while the addition of entry k runs.
template <class CV>
__global__ void __launch_bounds__(256, CV::MIN_WAVES)
k_accumulate_direct(const uint32_t *__restrict__ table, const uint32_t *__restrict__ idx, uint32_t E, uint32_t lpv, uint32_t per, uint32_t batch,
                    uint32_t *__restrict__ part) {
  using AC = typename CV::accum; using acc_t = typename AC::acc_t; using base_t = typename CV::base_t;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t vec = t / lpv, r = t - vec * lpv;
  extern __shared__ uint32_t acc_lds[];
  constexpr int BW = CV::BASE_WORDS, CH = BW / 4;
  uint32_t *wbuf = acc_lds + (threadIdx.x >> 6) * (2 * BW * 64);
  const uint32_t lane = threadIdx.x & 63;
  const bool live = vec < batch;
  const size_t v0 = (size_t)(live ? vec : 0) * E;
  uint32_t cnt = 0; size_t e0 = v0;
  if (live && (uint64_t)r * per < E) { e0 = v0 + (size_t)r * per; cnt = (uint64_t)r * per + per <= E ? per : (uint32_t)(E - (uint64_t)r * per); }
  auto issue = [&](uint32_t ix, uint32_t slot) {
    const uint32_t *src = table + (size_t)(ix == DIRECT_ZERO ? 0u : (ix & 0x7fffffffu)) * BW;
#pragma unroll
    for (int c = 0; c < CH; c++)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + 4 * c),
                                       (__attribute__((address_space(3))) void *)(wbuf + slot * (BW * 64) + c * 256), 16, 0, 0);
  };
  auto fetch = [&](uint32_t slot) {
    uint32_t w[BW];
#pragma unroll
    for (int c = 0; c < CH; c++) {
      const uint4 v = *reinterpret_cast<const uint4 *>(wbuf + slot * (BW * 64) + c * 256 + lane * 4);
      w[4 * c] = v.x; w[4 * c + 1] = v.y; w[4 * c + 2] = v.z; w[4 * c + 3] = v.w;
    }
    return CV::base_from_words(w);
  };
  acc_t acc = AC::identity();
  uint32_t ix = cnt ? idx[e0] : DIRECT_ZERO;
  uint32_t ix1 = cnt > 1 ? idx[e0 + 1] : DIRECT_ZERO;
  if (cnt) issue(ix, 0);
  for (uint32_t k = 0; k < cnt; k++) {
    const uint32_t cix = ix;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");            // the DMA of this buffer, and the reads of the other one before it is overwritten
    const base_t cur = fetch(k & 1);
    ix = ix1;
    if (k + 1 < cnt) issue(ix, (k + 1) & 1);
    if (k + 2 < cnt) ix1 = idx[e0 + k + 2];
    if (cix != DIRECT_ZERO) acc = AC::madd(acc, cur, (cix & 0x80000000u) != 0);
  }
  if (t < batch * lpv) AC::store_part(part + (size_t)t * AC::PART_WORDS, acc);
}
// one WAVE per vector: lane t sums the partials t, t + 64, .. of its vector one after the other, then the wave's butterfly -- 64 (lpv / 64 + 5)
// lane-additions per vector instead of the 7 lpv of a lane per partial (the kernel is latency-bound either way; what it does not issue, the
// other contexts' accumulations do) -> one point (canonical XYZZ for the host, as the bucket form's k_wsum leaves it)
template <class RV>
__global__ void __launch_bounds__(64, RV::RED_WAVES)
k_direct_reduce(const uint32_t *__restrict__ part, uint32_t lpv, uint32_t *__restrict__ out) {
  using acc_t = typename RV::acc_t;
  const uint32_t vec = blockIdx.x, t = threadIdx.x;
  acc_t a = RV::identity();
#pragma unroll 1
  for (uint32_t k = t; k < lpv; k += 64) a = cv_add<RV>(a, RV::accum::load_part(part + ((size_t)vec * lpv + k) * RV::accum::PART_WORDS));
  a = wave_sum<RV>(a);
  if (t == 0) RV::store_out(out + (size_t)vec * RV::OUT_WORDS, a);
}
template <class C>
static int msm_g1_direct_impl(const G1DirectTable &t, const uint32_t *d_scalars, size_t n, size_t scalar_stride, MsmWorkspace &ws, hipStream_t stream,
                              uint8_t *out_xy, size_t batch, int scalars_mont, const uint32_t *d_base_idx) {
  using CV = G1Curve<C>; using RV = typename CV::red;
  if (!n || !batch) return -1;
  const size_t rows = (size_t)t.rows, E = n * rows;
  if (E * batch >= 0xffff0000ull || (!d_base_idx && n > t.n)) throw HipFailure{hipErrorInvalidValue, __FILE__, __LINE__};
  const AccShape shape = accumulate_shape<CV>();
  size_t lpv = shape.lanes / batch; if (lpv > 1024) lpv = 1024; if (lpv < 1) lpv = 1;
  const size_t per = (E + lpv - 1) / lpv, lanes = batch * lpv;
  // workspace: the entry indices take `sorted`, the partial sums `part`, the results `rc`; the chain reports to the workspace's own record
  MsmChain &rec = ws.own;
  MsmPlan p; p.c = t.c; p.nwin = 1; p.nb = 1; p.lpb = (int)per;
  ws.ensure(E, p, (size_t)RV::OUT_WORDS * 4 > (size_t)RV::ACC_WORDS * 4 ? (size_t)RV::OUT_WORDS * 4 : (size_t)RV::ACC_WORDS * 4, batch, lanes + 256,
            (size_t)CV::accum::PART_WORDS * 4);
  static std::once_flag once[2];
  std::call_once(once[t.curve ? 1 : 0], [&]() {
    if (shape.lds > 48 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *)k_accumulate_direct<CV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.lds));
  });
  hipLaunchKernelGGL(k_direct_index, dim3((unsigned)((n + 255) / 256), (unsigned)batch), dim3(256), 0, stream, d_scalars, (uint32_t)n, (uint32_t)(scalar_stride ? scalar_stride : n),
                     t, ws.sorted.as(), scalars_mont, d_base_idx);
  HIP_CHECK(hipEventRecord(rec.ev0, stream));
  hipLaunchKernelGGL(k_accumulate_direct<CV>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), shape.lds, stream, (const uint32_t *)t.d, ws.sorted.as(),
                     (uint32_t)E, (uint32_t)lpv, (uint32_t)per, (uint32_t)batch, ws.part.as());
  HIP_CHECK(hipEventRecord(rec.ev1, stream));
  hipLaunchKernelGGL(k_direct_reduce<RV>, dim3((unsigned)batch), dim3(64), 0, stream, ws.part.as(), (uint32_t)lpv, ws.rc.as());
  copy_back(rec, ws.rc, MsmResult{MsmResult::POINTS, batch, 1, (size_t)RV::OUT_WORDS}, stream);
  rec.plan_host.as()[0] = (uint32_t)per;
  rec.plan = p;
  msm_collect(ws, rec, stream);
  g1_results<C>(rec, batch, out_xy);
  return 0;
}
int msm_g1_direct_device(const G1DirectTable &t, const uint32_t *d_scalars, size_t n, size_t scalar_stride, MsmWorkspace &ws, hipStream_t stream,
                         uint8_t *out_xy, size_t batch, int scalars_mont, const uint32_t *d_base_idx) {
  if (t.curve == 0) return msm_g1_direct_impl<G1Bls12381>(t, d_scalars, n, scalar_stride, ws, stream, out_xy, batch, scalars_mont, d_base_idx);
  return msm_g1_direct_impl<G1Bn254>(t, d_scalars, n, scalar_stride, ws, stream, out_xy, batch, scalars_mont, d_base_idx);
}

int msm_g1_fixed_device(int curve, const uint32_t *d_table, int table_c, size_t table_stride, const uint32_t *d_scalars, size_t n,
                        size_t scalar_stride, MsmWorkspace &ws, hipStream_t stream, uint8_t *out_xy, size_t batch, const uint32_t *d_base_idx,
                        int scalars_mont) {
  MsmLaunch o; o.batch = batch; o.table_c = table_c; o.table_stride = table_stride; o.scalar_stride = scalar_stride; o.d_base_idx = d_base_idx; o.scalars_mont = scalars_mont;
  if (curve == 0) return msm_g1_impl<G1Bls12381>(d_table, d_scalars, n, ws, stream, out_xy, o);
  if (curve == 1) return msm_g1_impl<G1Bn254>(d_table, d_scalars, n, ws, stream, out_xy, o);
  return -1;
}

}  // namespace avrf
