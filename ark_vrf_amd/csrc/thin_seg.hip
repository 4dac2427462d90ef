// thin_seg.hip -- the device side of thin::BatchVerifier and pedersen::BatchVerifier over segments of one staged batch (thin_seg.h).
//
//   k_thin_terms_seg : thin_item (batch_terms_dev.h; src/thin.rs:287-313) for every staged item, under its SEGMENT's weight stream
//                      and with its index inside the segment; the terms go to the segment's slice of the padded arrays
//   k_seg_base       : one block per segment: the generator term (src/thin.rs:303,316-317) from the segment's w s z0 values (base_term)
//   k_seg_item_flags : the input checks of k_thin_prepare (src/thin.rs:266-271) per item, run only after the batch's flag word came back set
//   k_ped_terms_seg, k_ped_seg_base, k_ped_seg_item_flags : the same three for Pedersen -- ped_item (src/pedersen.rs:369-410), the two
//                      base terms of a segment (:413-418), the checks of k_ped_prepare (:276-278, 348-353)
// One lane per item; scalar-field products in 8 x u32 Montgomery form (fp256.h).
#include "thin_seg.h"
#include "proto_dev.h"
#include "batch_terms_dev.h"

// Built once per suite (-DAVRF_TU_SUITE=<id>, csrc/Makefile): the suite's kernels and the explicit instantiation of SegOps<S>,
// which capi.hip reaches through AVRF_SEG.
#ifndef AVRF_TU_SUITE
#error "thin_seg.hip is built once per suite: -DAVRF_TU_SUITE=<id> (csrc/Makefile)"
#endif
namespace avrf {

// k_thin_terms_seg's sink of thin_item's terms: the plain batch's positions (k_thin_terms: item j's four kinds at 2 j + 2 io0 ..) moved by
// t0 = v L - (2 first + 2 io_off[first]), first = the segment's first item -- so the segment's slice starts with its first item's R
template <class S> struct SegTerms {
  uint32_t *__restrict__ scalars; te_pre *__restrict__ pre; const uint8_t *__restrict__ pks_xy; uint32_t t0;
  using Fr = typename S::Fr;
  AVRF_DI void r(uint32_t j, uint32_t io0, const fp &w_plain, const uint8_t *xy) const { emit_term<S>(scalars, pre, t0 + 2 * j + 2 * io0, w_plain, xy); }
  AVRF_DI void key(uint32_t j, uint32_t io0, const fp &wc) const { emit_term<S>(scalars, pre, t0 + 2 * j + 2 * io0 + 1, fp_from_mont<Fr>(wc), pks_xy + 64 * (size_t)j); }
  AVRF_DI void output(uint32_t j, uint32_t io0, uint32_t i, const fp &sc_plain, const uint8_t *xy) const { emit_term<S>(scalars, pre, t0 + 2 * j + 2 * io0 + 2 + 2 * i, sc_plain, xy); }
  AVRF_DI void input(uint32_t j, uint32_t io0, uint32_t i, const fp &sc_mont, const uint8_t *xy) const { emit_term<S>(scalars, pre, t0 + 2 * j + 2 * io0 + 3 + 2 * i, fp_from_mont<Fr>(sc_mont), xy); }
};

template <class S>
__global__ void __launch_bounds__(128)
k_thin_terms_seg(BatchDev b, const uint32_t *__restrict__ seg_off, uint32_t n_seg, uint32_t L, const Seed64 *__restrict__ seeds,
                 const uint32_t *__restrict__ c_in, const uint32_t *__restrict__ z_in, uint32_t *__restrict__ wsz,
                 uint32_t *__restrict__ scalars, te_pre *__restrict__ pre) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b.n) return;
  const uint32_t v = segment_of(seg_off, n_seg, j), first = seg_off[v];
  Seed64 seed = {};
  if (!b.weights) seed = seeds[v];                        // (a sponge suite's stream sits at b.weights + 16 j whatever the segment)
  const uint32_t t0 = v * L - (2 * first + 2 * b.io_off[first]);
  // j0 = -first: thin_item takes weight j0 + j = the item's index inside its segment
  const fp ws = thin_item<S>(b, seed, (uint64_t)0 - first, c_in, z_in, j, SegTerms<S>{scalars, pre, b.pks_xy, t0});
  fp_store(wsz + 8 * (size_t)j, ws);                      // w_j s_j z0 (Montgomery form), thin.rs:303
}

template <class S>
__global__ void __launch_bounds__(256)
k_seg_base(const uint32_t *__restrict__ io_off, const uint32_t *__restrict__ seg_off, uint32_t L, const uint32_t *__restrict__ wsz,
           uint32_t *__restrict__ scalars, te_pre *__restrict__ pre) {
  __shared__ fp red[256];
  const uint32_t v = blockIdx.x, first = seg_off[v], items = seg_off[v + 1] - first;
  if (!items) return;                                     // (block-uniform) an empty segment has no terms: src/thin.rs:262-264
  const uint32_t n_v = 2 * items + 2 * (io_off[first + items] - io_off[first]) + 1;
  base_term<S>(wsz + 8 * (size_t)first, items, scalars, pre, v * L + n_v - 1, 0, red);
}

template <class S>
__global__ void __launch_bounds__(128)
k_seg_item_flags(BatchDev b, int32_t *__restrict__ status) {
  using Fr = typename S::Fr;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b.n) return;
  uint32_t f = point_flags<S>(fp_load_le(b.pks_xy + 64 * (size_t)j), fp_load_le(b.pks_xy + 64 * (size_t)j + 32));
  for (uint32_t k = b.io_off[j]; k < b.io_off[j + 1]; k++) {
    const uint8_t *p = b.ios_xy + 128 * (size_t)k;
    f |= point_flags<S>(fp_load_le(p), fp_load_le(p + 32)) | point_flags<S>(fp_load_le(p + 64), fp_load_le(p + 96));
  }
  const uint8_t *pr = b.proofs + 96 * (size_t)j;
  f |= point_flags<S>(fp_load_le(pr), fp_load_le(pr + 32)) & FLAG_RANGE;       // R may be the identity (thin.rs:95-99)
  if (ge_p<Fr>(fp_load_le(pr + 64))) f |= FLAG_SCALAR;
  if (f) status[j] = 2;
}

// ---------------------------------------------------------------- Pedersen (src/pedersen.rs:303-426)

// k_ped_terms_seg's sink of ped_item's terms: the plain batch's positions (k_ped_terms: 5 j + k) moved by t0 = v L - 5 first
template <class S> struct SegPedTerms {
  uint32_t *__restrict__ scalars; te_pre *__restrict__ pre; uint32_t t0;
  AVRF_DI void term(uint32_t j, uint32_t k, const fp &sc_plain, const uint8_t *xy) const { emit_term<S>(scalars, pre, t0 + 5 * j + k, sc_plain, xy); }
};

// usb: n x 2 field elements of scratch as two planes, item j's u s at 8 j and its u sb at 8 (n + j) -- base_term reads a segment's run of either
template <class S>
__global__ void __launch_bounds__(128)
k_ped_terms_seg(BatchDev b, const uint32_t *__restrict__ seg_off, uint32_t n_seg, uint32_t L, const Seed64 *__restrict__ seeds,
                const uint32_t *__restrict__ c_in, const uint8_t *__restrict__ merged_xy, uint32_t *__restrict__ usb,
                uint32_t *__restrict__ scalars, te_pre *__restrict__ pre) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b.n) return;
  const uint32_t v = segment_of(seg_off, n_seg, j), first = seg_off[v];
  Seed64 seed = {};
  if (!b.weights) seed = seeds[v];                        // (a host-squeezed suite's stream sits at b.weights + 32 j whatever the segment)
  // j0 = -first: ped_item takes chunks 2 (j0 + j), 2 (j0 + j) + 1 = those of the item's index inside its segment
  fp u_sb;
  const fp u_s = ped_item<S>(b, seed, (uint64_t)0 - first, c_in, merged_xy, j, SegPedTerms<S>{scalars, pre, v * L - 5 * first}, u_sb);
  fp_store(usb + 8 * (size_t)j, u_s);                     // u_j s_j, u_j sb_j (Montgomery form), pedersen.rs:409-410
  fp_store(usb + 8 * ((size_t)b.n + j), u_sb);
}

// one block per segment: (G, -sum u s) at v L + 5 items and (BLINDING_BASE, -sum u sb) behind it (src/pedersen.rs:413-418)
template <class S>
__global__ void __launch_bounds__(256)
k_ped_seg_base(const uint32_t *__restrict__ seg_off, uint32_t n, uint32_t L, const uint32_t *__restrict__ usb,
               uint32_t *__restrict__ scalars, te_pre *__restrict__ pre) {
  __shared__ fp red[256];
  const uint32_t v = blockIdx.x, first = seg_off[v], items = seg_off[v + 1] - first;
  if (!items) return;                                     // (block-uniform) an empty segment has no terms: src/pedersen.rs:343-345
  base_term<S>(usb + 8 * (size_t)first, items, scalars, pre, v * L + 5 * items, 0, red);
  __syncthreads();
  base_term<S>(usb + 8 * ((size_t)n + first), items, scalars, pre, v * L + 5 * items + 1, 1, red);
}

// the checks of k_ped_prepare (src/pedersen.rs:276-278, 348-353) per item.  The merged pair is not among them: an item without pairs
// merges to the identity legitimately (src/pedersen.rs:264-267).
template <class S>
__global__ void __launch_bounds__(128)
k_ped_seg_item_flags(BatchDev b, int32_t *__restrict__ status) {
  using Fr = typename S::Fr;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= b.n) return;
  uint32_t f = 0;
  for (uint32_t k = b.io_off[j]; k < b.io_off[j + 1]; k++) {
    const uint8_t *p = b.ios_xy + 128 * (size_t)k;
    f |= point_flags<S>(fp_load_le(p), fp_load_le(p + 32)) | point_flags<S>(fp_load_le(p + 64), fp_load_le(p + 96));
  }
  const uint8_t *pr = b.proofs + 256 * (size_t)j;
  f |= point_flags<S>(fp_load_le(pr), fp_load_le(pr + 32));                                    // Yb: pk_com.is_zero() (:348-353)
  f |= (point_flags<S>(fp_load_le(pr + 64), fp_load_le(pr + 96)) | point_flags<S>(fp_load_le(pr + 128), fp_load_le(pr + 160))) & FLAG_RANGE;   // R, Ok
  if (ge_p<Fr>(fp_load_le(pr + 192)) || ge_p<Fr>(fp_load_le(pr + 224))) f |= FLAG_SCALAR;
  if (f) status[j] = 2;
}

template <class S> void SegOps<S>::thin_terms(const BatchDev &b, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t L, const Seed64 *d_seeds, const uint32_t *d_c,
                                              const uint32_t *d_z, uint32_t *d_wsz, uint32_t *d_scalars, te_pre_raw *d_pre, hipStream_t st) {
  if (!b.n || !n_seg) return;
  hipLaunchKernelGGL(k_thin_terms_seg<S>, dim3((b.n + 127) / 128), dim3(128), 0, st, b, d_seg_off, n_seg, L, d_seeds, d_c, d_z, d_wsz, d_scalars, (te_pre *)d_pre);
  hipLaunchKernelGGL(k_seg_base<S>, dim3(n_seg), dim3(256), 0, st, b.io_off, d_seg_off, L, d_wsz, d_scalars, (te_pre *)d_pre);
}
template <class S> void SegOps<S>::item_flags(const BatchDev &b, int32_t *d_status, hipStream_t st) {
  if (!b.n) return;
  hipLaunchKernelGGL(k_seg_item_flags<S>, dim3((b.n + 127) / 128), dim3(128), 0, st, b, d_status);
}
template <class S> void SegOps<S>::ped_terms(const BatchDev &b, const uint32_t *d_seg_off, uint32_t n_seg, uint32_t L, const Seed64 *d_seeds, const uint32_t *d_c,
                                             const uint8_t *d_merged, uint32_t *d_usb, uint32_t *d_scalars, te_pre_raw *d_pre, hipStream_t st) {
  if (!b.n || !n_seg) return;
  hipLaunchKernelGGL(k_ped_terms_seg<S>, dim3((b.n + 127) / 128), dim3(128), 0, st, b, d_seg_off, n_seg, L, d_seeds, d_c, d_merged, d_usb, d_scalars, (te_pre *)d_pre);
  hipLaunchKernelGGL(k_ped_seg_base<S>, dim3(n_seg), dim3(256), 0, st, d_seg_off, b.n, L, d_usb, d_scalars, (te_pre *)d_pre);
}
template <class S> void SegOps<S>::ped_item_flags(const BatchDev &b, int32_t *d_status, hipStream_t st) {
  if (!b.n) return;
  hipLaunchKernelGGL(k_ped_seg_item_flags<S>, dim3((b.n + 127) / 128), dim3(128), 0, st, b, d_status);
}
template struct SegOps<suite_by_id<AVRF_TU_SUITE>::type>;

}  // namespace avrf
