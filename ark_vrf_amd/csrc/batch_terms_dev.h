// batch_terms_dev.h -- what the terms kernels of the batch verifiers share (vrf_batch.hip k_thin_terms / k_ped_terms / k_g_final,
// thin_shared.hip k_thin_terms_shared / k_ped_terms_shared / k_shared_merge, thin_seg.hip's segmented kernels of both kinds), each stated once:
//   fp_from_u128, emit_term : a 128-bit little-endian value as a field element; one MSM term (plain scalar + precomputed base)
//   block_sum               : the sum of an Fr value over a block, in LDS
//   WeightBlocks            : the blocks of the counter-mode weight stream that a workgroup's items read, hashed once, in LDS
//   thin_item               : the per-item arithmetic of thin::BatchVerifier::verify, src/thin.rs:287-313, over a sink for its terms
//   thin_item_plain         : the same for a sink that takes every scalar in plain form, in eight Fr products instead of eleven
//   ped_item, ped_item_w    : the per-item arithmetic of pedersen::BatchVerifier::verify, src/pedersen.rs:369-410, over a sink likewise
//                             (ped_item_w: with the item's weights given), ten Fr products
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

// The weight stream of a counter-mode transcript, block i = H(seed || LE64(i)) of 64 bytes, shared by a workgroup.  Item g (a GLOBAL
// index, j0 + j) reads bytes [BYTES g, BYTES g + BYTES) of it: BYTES = 16 (thin: w) or 32 (Pedersen: t, u), so 4 or 2 items read one
// block and every lane hashing its own repeats the compression 4 or 2 times.  Here the blocks that cover the workgroup's items
// [g_first, g_first + count), count in 1..NT, are hashed once, one lane per block (the first wave or two of the workgroup), and left
// in LDS word-major (word i of block k at lds[i * MAXB + k]: the lanes of a wave write consecutive addresses).  Any g_first: a
// first block shared with the previous workgroup is hashed by both (j0 % 4 != 0 in avrf_thin_batch_partial).
// fill is called by EVERY thread of the workgroup (it ends in a barrier); chunk16 then reads chunk c (16 bytes) of
// item g as four little-endian words.
template <int NT, int BYTES> struct WeightBlocks {
  static_assert(BYTES == 16 || BYTES == 32, "16 bytes per item (thin) or 32 (Pedersen)");
  static constexpr int MAXB = NT * BYTES / 64 + 1;                             // + 1: g_first need not start a block
  static constexpr int WORDS = 8 * MAXB;                                       // uint64_t elements of LDS
  static AVRF_DI void fill(const Seed64 &seed, uint64_t g_first, uint32_t count, uint64_t *lds) {
    const uint64_t fb = g_first * BYTES / 64, lb = ((g_first + count) * BYTES - 1) / 64;
    uint32_t nb = count ? (uint32_t)(lb - fb) + 1 : 0;                         // <= MAXB for count <= NT
    nb = nb < (uint32_t)MAXB ? nb : (uint32_t)MAXB;
    for (uint32_t k = threadIdx.x; k < nb; k += NT) {
      uint64_t blk[8]; sha512_xof_block(seed.w, fb + k, blk);
#pragma unroll
      for (int i = 0; i < 8; i++) lds[i * MAXB + k] = blk[i];
    }
    __syncthreads();
  }
  static AVRF_DI void chunk16(const uint64_t *lds, uint64_t g_first, uint64_t g, int c, uint32_t (&w)[4]) {
    const uint64_t byte = g * BYTES + 16 * (uint64_t)c;
    const uint32_t k = (uint32_t)(byte / 64 - g_first * BYTES / 64), q = (uint32_t)(byte % 64) / 16;
    be128_le(lds[(2 * q) * MAXB + k], lds[(2 * q + 1) * MAXB + k], w);
  }
};

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

// thin_item for a sink that takes EVERY scalar in plain form,
//   r(j, io0, w_plain, xy)   key(j, io0, wc_plain)   output(j, io0, i, scalar_plain, xy)   input(j, io0, i, scalar_plain, xy)
// with the item's weight w_j given (four little-endian words: the caller read it from the stream or from WeightBlocks).  Nothing
// is converted to Montgomery form: the plain values are multiplied as they are, mm(a, b) = a b / R, and ONE product by a power of R
// restores the form that is wanted,
//   w c   = mm(mm(w, c), R^2)            w c z  = mm(mm(mm(w, c), z), R^3)
//   w s R = mm(mm(s, w), R^3)            w s z  = mm(mm(mm(s, w), z), R^3)
// eight products for one pair where thin_item spends eleven (four to_mont, four products, three from_mont).  The same canonical
// values come out: every product is a fully reduced residue.  (s, the only operand that can exceed r -- such a proof is flagged
// by k_thin_prepare -- goes first: the multiplier takes any first operand below 2^256, fp256.h.)
template <class S, class Out>
AVRF_DI fp thin_item_plain(const BatchDev &b, const uint32_t (&ww)[4], const uint32_t *__restrict__ c_in, const uint32_t *__restrict__ z_in,
                           uint32_t j, const Out &out) {
  using Fr = typename S::Fr;
  uint32_t io0 = b.io_off[j], m = b.io_off[j + 1] - io0;
  fp w_plain = fp_zero(); w_plain.v[0] = ww[0]; w_plain.v[1] = ww[1]; w_plain.v[2] = ww[2]; w_plain.v[3] = ww[3];
  const fp r2 = fp_const<Fr>(Fr::R2), r3 = fp_const<Fr>(Fr::R3);
  const uint8_t *pr = b.proofs + 96 * (size_t)j;
  const fp wc = fp_mul<Fr>(fp_from_u128(c_in + 4 * (size_t)j), w_plain);       // w c / R     thin.rs:291-292
  const fp ws = fp_mul<Fr>(fp_load_le(pr + 64), w_plain);                      // w s / R
  out.r(j, io0, w_plain, pr);                                                           // (R_j, w_j)        :295-296
  out.key(j, io0, fp_mul<Fr>(wc, r2));                                                  // (pk_j, w c z0)    :299-300, z0 = 1
  for (uint32_t i = 0; i < m; i++) {                                                    // :306-312
    const fp z = fp_from_u128(z_in + 4 * (size_t)(io0 + i));
    const uint8_t *p = b.ios_xy + 128 * (size_t)(io0 + i);
    out.output(j, io0, i, fp_mul<Fr>(fp_mul<Fr>(wc, z), r3), p + 64);                   // (O_i, w c z_i)
    out.input(j, io0, i, fp_neg<Fr>(fp_mul<Fr>(fp_mul<Fr>(ws, z), r3)), p);             // (I_i, -w s z_i)
  }
  return fp_mul<Fr>(ws, r3);                                                            // w s z0 in Montgomery form, :303
}

template <class S, class Out>
AVRF_DI fp ped_item_w(const BatchDev &b, const fp &t_plain, const fp &u_plain, const uint32_t *__restrict__ c_in,
                      const uint8_t *__restrict__ merged_xy, uint32_t j, const Out &out, fp &usb);

// Item j of pedersen::BatchVerifier::verify (src/pedersen.rs:369-410): its five terms go to `out`, a struct with one inline function
//   term(j, k, scalar_plain, xy)      k = 0 (O, t c)   1 (Ok, t)   2 (I, -t s)   3 (Yb, u c)   4 (R, u)
// (O, I: the item's merged pair, merged_xy + 128 j, k_ped_prepare); what the item adds to the scalars of G and BLINDING_BASE, u s
// (returned) and u sb (usb), comes back in Montgomery form (:409-410).
template <class S, class Out>
AVRF_DI fp ped_item(const BatchDev &b, const Seed64 &seed, uint64_t j0, const uint32_t *__restrict__ c_in, const uint8_t *__restrict__ merged_xy,
                    uint32_t j, const Out &out, fp &usb) {
  // 32 squeezed bytes per item: t = bytes[0..16], u = bytes[16..32]   (:373-381)
  // (j0: global index of the shard's first item when one batch is split over several GPUs)
  fp t_plain, u_plain;
  if (b.weights) { t_plain = fp_from_u128(reinterpret_cast<const uint32_t *>(b.weights + 32 * (size_t)j)); u_plain = fp_from_u128(reinterpret_cast<const uint32_t *>(b.weights + 32 * (size_t)j + 16)); }
  else {
    ShaReader rd; for (int i = 0; i < 8; i++) rd.seed[i] = seed.w[i]; rd.have = 0;
    t_plain = xof128(rd, (uint32_t)(2 * (j0 + j))); u_plain = xof128(rd, (uint32_t)(2 * (j0 + j) + 1));
  }
  return ped_item_w<S>(b, t_plain, u_plain, c_in, merged_xy, j, out, usb);
}
// ped_item with the item's weights t, u given (plain; the caller read them from the stream or from WeightBlocks).  As in
// thin_item_plain nothing is converted to Montgomery form first: ten Fr products instead of thirteen,
//   t c = mm(mm(c, t), R^2)   t s = mm(mm(s, t), R^2)   u c = mm(mm(c, u), R^2)   u s R = mm(mm(s, u), R^3)   u sb R = mm(mm(sb, u), R^3)
// (s and sb, which can exceed r in a proof that k_ped_prepare flags, go first: fp256.h).
template <class S, class Out>
AVRF_DI fp ped_item_w(const BatchDev &b, const fp &t_plain, const fp &u_plain, const uint32_t *__restrict__ c_in,
                      const uint8_t *__restrict__ merged_xy, uint32_t j, const Out &out, fp &usb) {
  using Fr = typename S::Fr;
  const fp r2 = fp_const<Fr>(Fr::R2), r3 = fp_const<Fr>(Fr::R3);
  const fp c = fp_from_u128(c_in + 4 * (size_t)j);
  const uint8_t *pr = b.proofs + 256 * (size_t)j, *mo = merged_xy + 128 * (size_t)j;
  const fp s = fp_load_le(pr + 192), sb = fp_load_le(pr + 224);
  out.term(j, 0, fp_mul<Fr>(fp_mul<Fr>(c, t_plain), r2), mo + 64);                 // (O, t c)      :392-393
  out.term(j, 1, t_plain, pr + 128);                                               // (Ok, t)       :395-396
  out.term(j, 2, fp_neg<Fr>(fp_mul<Fr>(fp_mul<Fr>(s, t_plain), r2)), mo);          // (I, -t s)     :398-399
  out.term(j, 3, fp_mul<Fr>(fp_mul<Fr>(c, u_plain), r2), pr);                      // (Yb, u c)     :402-403
  out.term(j, 4, u_plain, pr + 64);                                                // (R, u)        :405-406
  usb = fp_mul<Fr>(fp_mul<Fr>(sb, u_plain), r3);                                   // :409-410, Montgomery form
  return fp_mul<Fr>(fp_mul<Fr>(s, u_plain), r3);
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
