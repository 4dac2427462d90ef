// batch_terms_dev.h -- what the terms kernels of the batch verifiers share (vrf_batch.hip k_thin_terms / k_ped_terms / k_g_final,
// thin_shared.hip k_thin_terms_shared / k_ped_terms_shared / k_shared_merge, thin_seg.hip's segmented kernels of both kinds), each stated once:
//   fp_from_u128, emit_term : a 128-bit little-endian value as a field element; one MSM term (plain scalar + precomputed base)
//   block_sum               : the sum of an Fr value over a block, in LDS
//   thin_item               : the per-item arithmetic of thin::BatchVerifier::verify, src/thin.rs:287-313, over a sink for its terms
//   ped_item                : the per-item arithmetic of pedersen::BatchVerifier::verify, src/pedersen.rs:369-410, over a sink likewise
//   base_term               : the shared-base term (G or BLINDING_BASE, -(sum of the blocks' partials)), src/thin.rs:303,316-317
#pragma once
#include "proto_dev.h"

namespace avrf {

AVRF_DI fp fp_from_u128(const uint32_t *w) {
  fp a = fp_zero(); uint4 v = *reinterpret_cast<const uint4 *>(w);
  a.v[0] = v.x; a.v[1] = v.y; a.v[2] = v.z; a.v[3] = v.w; return a;
}
template <class S> AVRF_DI void emit_term(uint32_t *scalars, te_pre *pre, uint32_t t, const fp &scalar_plain, const uint8_t *xy) {
  using Fq = typename S::Fq;
  fp_store(scalars + 8 * (size_t)t, scalar_plain);
  fp x = fp_to_mont<Fq>(fp_load_le(xy)), y = fp_to_mont<Fq>(fp_load_le(xy + 32));
  store_pre(pre + t, te_make_pre<S>(x, y));
}

// The sum of v over the block's NT threads (a power of two; red: NT elements of LDS), valid on thread 0.  Every thread of the block
// calls it; a caller that uses red again puts a __syncthreads() in between.  ROLLED keeps the tree a loop: a kernel that has no
// registers to spare for the unrolled tree's masked additions says so (k_shared_merge).
template <class F, int NT, bool ROLLED = false>
AVRF_DI fp block_sum(const fp &v, fp *red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll ROLLED ? 1 : NT
  for (int s2 = NT / 2; s2 >= 1; s2 >>= 1) {
    if ((int)threadIdx.x < s2) red[threadIdx.x] = fp_add<F>(red[threadIdx.x], red[threadIdx.x + s2]);
    __syncthreads();
  }
  return red[0];
}

// Item j of thin::BatchVerifier::verify (src/thin.rs:287-313): its four kinds of term go to `out`, a struct of inline functions
//   r(j, io0, w_plain, xy)   key(j, io0, wc_mont)   output(j, io0, i, scalar_plain, xy)   input(j, io0, i, scalar_mont, xy)
// (plain / mont: the scalar's form); what the item adds to the generator's scalar, w_j s_j z0 in Montgomery form (:303), is returned.
template <class S, class Out>
AVRF_DI fp thin_item(const BatchDev &b, const Seed64 &seed, uint64_t j0, const uint32_t *__restrict__ c_in, const uint32_t *__restrict__ z_in,
                     uint32_t j, const Out &out) {
  using Fr = typename S::Fr;
  uint32_t io0 = b.io_off[j], m = b.io_off[j + 1] - io0;
  // w_j = challenge_scalar(&mut t): 16 bytes of the weight stream (thin.rs:289, common.rs:72-76)
  // (j0 = global index of this shard's first item when one batch is split over several GPUs)
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
  fp ws = fp_mul<Fr>(w, s);
  out.r(j, io0, w_plain, pr);                                                           // (R_j, w_j)        :295-296
  out.key(j, io0, wc);                                                                  // (pk_j, w c z0)    :299-300, z0 = 1
  for (uint32_t i = 0; i < m; i++) {                                                    // :306-312
    fp z = fp_to_mont<Fr>(fp_from_u128(z_in + 4 * (size_t)(io0 + i)));
    const uint8_t *p = b.ios_xy + 128 * (size_t)(io0 + i);
    out.output(j, io0, i, fp_from_mont<Fr>(fp_mul<Fr>(wc, z)), p + 64);                 // (O_i, w c z_i)
    out.input(j, io0, i, fp_neg<Fr>(fp_mul<Fr>(ws, z)), p);                             // (I_i, -w s z_i)
  }
  return ws;
}

// Item j of pedersen::BatchVerifier::verify (src/pedersen.rs:369-410): its five terms go to `out`, a struct with one inline function
//   term(j, k, scalar_plain, xy)      k = 0 (O, t c)   1 (Ok, t)   2 (I, -t s)   3 (Yb, u c)   4 (R, u)
// (O, I: the item's merged pair, merged_xy + 128 j, k_ped_prepare); what the item adds to the scalars of G and BLINDING_BASE, u s
// (returned) and u sb (usb), comes back in Montgomery form (:409-410).
template <class S, class Out>
AVRF_DI fp ped_item(const BatchDev &b, const Seed64 &seed, uint64_t j0, const uint32_t *__restrict__ c_in, const uint8_t *__restrict__ merged_xy,
                    uint32_t j, const Out &out, fp &usb) {
  using Fr = typename S::Fr;
  // 32 squeezed bytes per item: t = bytes[0..16], u = bytes[16..32]   (:373-381)
  // (j0: global index of the shard's first item when one batch is split over several GPUs)
  fp t_plain, u_plain;
  if (b.weights) { t_plain = fp_from_u128(reinterpret_cast<const uint32_t *>(b.weights + 32 * (size_t)j)); u_plain = fp_from_u128(reinterpret_cast<const uint32_t *>(b.weights + 32 * (size_t)j + 16)); }
  else {
    ShaReader rd; for (int i = 0; i < 8; i++) rd.seed[i] = seed.w[i]; rd.have = 0;
    t_plain = xof128(rd, (uint32_t)(2 * (j0 + j))); u_plain = xof128(rd, (uint32_t)(2 * (j0 + j) + 1));
  }
  fp tt = fp_to_mont<Fr>(t_plain), uu = fp_to_mont<Fr>(u_plain);
  fp c = fp_to_mont<Fr>(fp_from_u128(c_in + 4 * (size_t)j));
  const uint8_t *pr = b.proofs + 256 * (size_t)j, *mo = merged_xy + 128 * (size_t)j;
  fp s = fp_to_mont<Fr>(fp_load_le(pr + 192)), sb = fp_to_mont<Fr>(fp_load_le(pr + 224));
  out.term(j, 0, fp_from_mont<Fr>(fp_mul<Fr>(tt, c)), mo + 64);                    // (O, t c)      :392-393
  out.term(j, 1, t_plain, pr + 128);                                               // (Ok, t)       :395-396
  out.term(j, 2, fp_from_mont<Fr>(fp_neg<Fr>(fp_mul<Fr>(tt, s))), mo);             // (I, -t s)     :398-399
  out.term(j, 3, fp_from_mont<Fr>(fp_mul<Fr>(uu, c)), pr);                         // (Yb, u c)     :402-403
  out.term(j, 4, u_plain, pr + 64);                                                // (R, u)        :405-406
  const fp us = fp_mul<Fr>(uu, s); usb = fp_mul<Fr>(uu, sb);                       // :409-410
  return us;
}

// g = -(sum of the nparts partials); term t_last = (G, g), or (BLINDING_BASE, g) for which_base 1   (thin.rs:303,316-317).
// One block of 256 threads; red: 256 elements of LDS; ROLLED as in block_sum.
template <class S, bool ROLLED = false>
AVRF_DI void base_term(const uint32_t *__restrict__ gpart, uint32_t nparts, uint32_t *__restrict__ scalars, te_pre *__restrict__ pre,
                       uint32_t t_last, int which_base, fp *red) {
  using Fr = typename S::Fr; using Fq = typename S::Fq;
  fp acc = fp_zero();
  for (uint32_t i = threadIdx.x; i < nparts; i += 256) acc = fp_add<Fr>(acc, fp_load(gpart + 8 * (size_t)i));
  const fp sum = block_sum<Fr, 256, ROLLED>(acc, red);
  if (threadIdx.x == 0) {
    fp_store(scalars + 8 * (size_t)t_last, fp_from_mont<Fr>(fp_neg<Fr>(sum)));
    te_pre g;
    if (which_base == 0) { g.x = fp_const<Fq>(S::G_X); g.y = fp_const<Fq>(S::G_Y); g.k = fp_const<Fq>(S::G_K); }
    else { g.x = fp_const<Fq>(S::B_X); g.y = fp_const<Fq>(S::B_Y); g.k = fp_const<Fq>(S::B_K); }
    store_pre(pre + t_last, g);
  }
}

}  // namespace avrf
