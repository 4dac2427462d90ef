// vrf_batch.hip -- per-item Fiat-Shamir hashing and MSM term construction on the device.
//
//   k_thin_prepare : thin::BatchVerifier::prepare, src/thin.rs:209-226
//                    (vrf_transcript_scalars_with_schnorr src/utils/common.rs:251-258,
//                     vrf_transcript_base :159-173, DelinearizeScalars :335-369, challenge :270-280)
//   k_thin_terms   : the per-item part of thin::BatchVerifier::verify, src/thin.rs:287-313 (thin_item_plain, batch_terms_dev.h)
//   k_g_final      : the shared-generator term, src/thin.rs:303,316-317 (base_term, batch_terms_dev.h)
//   k_ped_prepare  : pedersen::BatchItem::new, src/pedersen.rs:276-293
//   k_ped_terms    : the per-item part of pedersen::BatchVerifier::verify, src/pedersen.rs:369-410 (ped_item_w, batch_terms_dev.h)
// One lane per batch item; SHA-512 state in VGPRs (sha512_dev.h); scalar-field products in
// 8 x u32 Montgomery form (fp256.h).  The terms kernels hash the weight stream's blocks once per workgroup (WeightBlocks).
#include "vrf_batch.h"
#include "proto_dev.h"
#include "batch_terms_dev.h"
#include "suite_dispatch.h"

// Built once per suite (-DAVRF_TU_SUITE=<id>: the kernels of that suite and the explicit instantiation of BatchOps<S>, which
// capi.hip reaches through AVRF_BATCH); csrc/Makefile.
#ifndef AVRF_TU_SUITE
#error "vrf_batch.hip is built once per suite: -DAVRF_TU_SUITE=<id> (csrc/Makefile)"
#endif
namespace avrf {

// k_thin_prepare for an item with ONE pair where ThinLayout1<S>::OK (proto_dev.h): the same bytes hashed, placed differently.  The
// 172 (Bandersnatch) bytes before the additional data go into the block at compile-time offsets, 68 of them as literal block words;
// the additional data, the two tags and R follow at a run-time position eight bytes to a step (sha512_dev.h, Sha512Tail).  Five
// compressions for a short `ad`: block 1, and the final and first squeeze block of the delinearisation and challenge forks.
template <class S>
AVRF_DI uint32_t thin_prepare_one(const BatchDev &b, uint32_t j, uint32_t io0, uint32_t ad0, uint32_t adl,
                                  uint32_t *__restrict__ c_out, uint32_t *__restrict__ z_out) {
  using Fr = typename S::Fr; using L = ThinLayout1<S>;
  constexpr ShaLit lit = L::prefix();
  const uint8_t *pk = b.pks_xy + 64 * (size_t)j, *p = b.ios_xy + 128 * (size_t)io0, *pr = b.proofs + 96 * (size_t)j;
  uint32_t f = 0, v[8];
  Sha512 h; sha512_init(h);
  sha512_lit<L::PK>(h, lit);
  fp x = fp_load_le(pk), y = fp_load_le(pk + 32);
  f |= point_flags<S>(x, y); point_words<S>(x, y, v); sha512_words_at<L::PK>(h, v);                // thin.rs:266-271
  x = fp_load_le(p); y = fp_load_le(p + 32);
  f |= point_flags<S>(x, y); point_words<S>(x, y, v); sha512_words_at<L::IN>(h, v);
  x = fp_load_le(p + 64); y = fp_load_le(p + 96);
  f |= point_flags<S>(x, y); point_words<S>(x, y, v); sha512_words_at<L::OUT>(h, v);
  sha512_u32le_at<L::ADL>(h, adl); sha512_u32le_at<L::ADL + 4>(h, 0);                               // common.rs:169-170
  sha512_static_end<L::END>(h);
  Sha512Tail t = sha512_tail_begin(h);
  sha512_tail_bytes(t, b.ads + ad0, adl);
  uint64_t seed[8], blk[8]; uint32_t w[4];
  {                                                                            // DelinearizeScalars :345-363
    Sha512Tail td = t;
    sha512_tail_absorb(td, (uint64_t)DS_DELINEARIZE << 56, 1);
    sha512_tail_final(td, seed); sha512_xof_block(seed, 0, blk); be128_le(blk[0], blk[1], w);
    *reinterpret_cast<uint4 *>(z_out + 4 * (size_t)io0) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  x = fp_load_le(pr); y = fp_load_le(pr + 32);                                 // challenge :270-280
  const fp s = fp_load_le(pr + 64);
  if (point_flags<S>(x, y) & FLAG_RANGE) f |= FLAG_RANGE;                      // R may be the identity (thin.rs:95-99)
  if (ge_p<Fr>(s)) f |= FLAG_SCALAR;
  sha512_tail_absorb(t, (uint64_t)DS_CHALLENGE << 56, 1);
  point_words<S>(x, y, v); sha512_tail_words(t, v);
  sha512_tail_final(t, seed); sha512_xof_block(seed, 0, blk); be128_le(blk[0], blk[1], w);
  *reinterpret_cast<uint4 *>(c_out + 4 * (size_t)j) = make_uint4(w[0], w[1], w[2], w[3]);
  if (b.records) {                                                             // LE32(c) || LE32(s) of the weight transcript, thin.rs:274-279
    uint4 *r = reinterpret_cast<uint4 *>(b.records + 64 * (size_t)j);
    const uint4 *sp = reinterpret_cast<const uint4 *>(pr + 64);
    r[0] = make_uint4(w[0], w[1], w[2], w[3]); r[1] = make_uint4(0, 0, 0, 0); r[2] = sp[0]; r[3] = sp[1];
  }
  return f;
}

template <class S>
__global__ void __launch_bounds__(128)
k_thin_prepare(BatchDev b, uint32_t *__restrict__ c_out, uint32_t *__restrict__ z_out, uint32_t *__restrict__ flags) {
  using Fr = typename S::Fr;
  uint32_t j = b.first + blockIdx.x * blockDim.x + threadIdx.x;                // the range [b.first, b.n): a whole batch, or one pushed chunk of an open one
  if (j >= b.n) return;
  uint32_t io0 = b.io_off[j], io1 = b.io_off[j + 1], m = io1 - io0;
  uint32_t ad0 = b.ad_off[j], adl = b.ad_off[j + 1] - ad0;
  uint32_t f = 0;
  if constexpr (ThinLayout1<S>::OK) if (m == 1) {                              // every other item, also of the same wave: the general path below
    f = thin_prepare_one<S>(b, j, io0, ad0, adl, c_out, z_out);
    if (f) atomicOr(flags, f);
    return;
  }
  suite_tr<S> h; tr_init(h);
  for (int i = 0; i < S::SUITE_ID_LEN; i++) tr_byte(h, S::SUITE_ID[i]);       // Transcript::new(SUITE_ID)
  tr_byte(h, DS_THIN);                                                         // common.rs:166
  tr_u64le(h, (uint64_t)m + 1);                                                // absorb_ios :377-383, Schnorr pair first
  absorb_generator<S>(h);                                                    // chain_ios :231-240: (G, pk)
  // short-Weierstrass presentation, one pair (the common shape): the 33-byte forms of pk, I, O and R with ONE inversion
  sw_enc enc[4]; bool have_enc = false;
  if constexpr (S::SW_CODEC) if (m == 1) {
    const uint8_t *p = b.ios_xy + 128 * (size_t)io0, *pr = b.proofs + 96 * (size_t)j, *pk = b.pks_xy + 64 * (size_t)j;
    const fp xs[4] = {fp_load_le(pk), fp_load_le(p), fp_load_le(p + 64), fp_load_le(pr)};
    const fp ys[4] = {fp_load_le(pk + 32), fp_load_le(p + 32), fp_load_le(p + 96), fp_load_le(pr + 32)};
    sw_encode_te_many<S, 4>(xs, ys, enc); have_enc = true;
  }
  {
    fp x = fp_load_le(b.pks_xy + 64 * (size_t)j), y = fp_load_le(b.pks_xy + 64 * (size_t)j + 32);
    f |= point_flags<S>(x, y);                                                 // thin.rs:266-271
    if (have_enc) absorb_sw_enc(h, enc[0]); else absorb_point_xy<S>(h, x, y);
  }
  for (uint32_t i = 0; i < m; i++) {
    const uint8_t *p = b.ios_xy + 128 * (size_t)(io0 + i);
    fp x = fp_load_le(p), y = fp_load_le(p + 32);
    f |= point_flags<S>(x, y); if (have_enc) absorb_sw_enc(h, enc[1]); else absorb_point_xy<S>(h, x, y);
    x = fp_load_le(p + 64); y = fp_load_le(p + 96);
    f |= point_flags<S>(x, y); if (have_enc) absorb_sw_enc(h, enc[2]); else absorb_point_xy<S>(h, x, y);
  }
  tr_u64le(h, (uint64_t)adl);                                                  // common.rs:169-170
  tr_bytes(h, b.ads + ad0, adl);
  if (m) {                                                                     // DelinearizeScalars :345-363
    auto rd = delin_seed(h);
    for (uint32_t i = 0; i < m; i++) {
      uint32_t w[4]; rd_chunk16(rd, i, w);
      uint4 *o = reinterpret_cast<uint4 *>(z_out + 4 * (size_t)(io0 + i));
      *o = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  {                                                                            // challenge :270-280
    const uint8_t *pr = b.proofs + 96 * (size_t)j;
    fp x = fp_load_le(pr), y = fp_load_le(pr + 32), s = fp_load_le(pr + 64);
    if (point_flags<S>(x, y) & FLAG_RANGE) f |= FLAG_RANGE;                    // R may be the identity (thin.rs:95-99)
    if (ge_p<Fr>(s)) f |= FLAG_SCALAR;
    tr_byte(h, DS_CHALLENGE);
    if (have_enc) absorb_sw_enc(h, enc[3]); else absorb_point_xy<S>(h, x, y);
    auto rd = tr_reader(h);
    uint32_t w[4]; rd_chunk16(rd, 0, w);
    uint4 *o = reinterpret_cast<uint4 *>(c_out + 4 * (size_t)j);
    *o = make_uint4(w[0], w[1], w[2], w[3]);
    if (b.records) {                                                           // LE32(c) || LE32(s) of the weight transcript, thin.rs:274-279
      uint4 *r = reinterpret_cast<uint4 *>(b.records + 64 * (size_t)j);
      const uint4 *sp = reinterpret_cast<const uint4 *>(pr + 64);
      r[0] = make_uint4(w[0], w[1], w[2], w[3]); r[1] = make_uint4(0, 0, 0, 0); r[2] = sp[0]; r[3] = sp[1];
    }
  }
  if (f) atomicOr(flags, f);
}

// k_thin_terms' sink of thin_item's terms: item j's four kinds at 2 j + 2 io0 (+1, +2 + 2 i, +3 + 2 i), every scalar in plain form
template <class S> struct PlainTerms {
  uint32_t *__restrict__ scalars; te_pre *__restrict__ pre; const uint8_t *__restrict__ pks_xy;
  using Fr = typename S::Fr;
  AVRF_DI void r(uint32_t j, uint32_t io0, const fp &w_plain, const uint8_t *xy) const { emit_term<S>(scalars, pre, 2 * j + 2 * io0, w_plain, xy); }
  AVRF_DI void key(uint32_t j, uint32_t io0, const fp &wc_plain) const { emit_term<S>(scalars, pre, 2 * j + 2 * io0 + 1, wc_plain, pks_xy + 64 * (size_t)j); }
  AVRF_DI void output(uint32_t j, uint32_t io0, uint32_t i, const fp &sc_plain, const uint8_t *xy) const { emit_term<S>(scalars, pre, 2 * j + 2 * io0 + 2 + 2 * i, sc_plain, xy); }
  AVRF_DI void input(uint32_t j, uint32_t io0, uint32_t i, const fp &sc_plain, const uint8_t *xy) const { emit_term<S>(scalars, pre, 2 * j + 2 * io0 + 3 + 2 * i, sc_plain, xy); }
};

// Workgroups of TERMS_NT items: the first wave hashes the (up to 65) blocks of the weight stream for all four (WeightBlocks,
// batch_terms_dev.h); a host-made stream (b.weights, the sponge suites) is read as before.  One partial per workgroup goes to gpart.
enum { TERMS_NT = 256 };
template <class S>
__global__ void __launch_bounds__(TERMS_NT)
k_thin_terms(BatchDev b, Seed64 seed, uint64_t j0, const uint32_t *__restrict__ c_in, const uint32_t *__restrict__ z_in,
             uint32_t *__restrict__ scalars, te_pre *__restrict__ pre, uint32_t *__restrict__ gpart) {
  using Fr = typename S::Fr; using WB = WeightBlocks<TERMS_NT, 16>;
  __shared__ fp red[TERMS_NT];
  __shared__ uint64_t wblk[WB::WORDS];
  const uint32_t jb = blockIdx.x * TERMS_NT, j = jb + threadIdx.x;
  if (!b.weights) WB::fill(seed, j0 + jb, b.n - jb < TERMS_NT ? b.n - jb : TERMS_NT, wblk);     // (uniform: every thread takes it)
  fp ws = fp_zero();
  if (j < b.n) {
    // w_j = challenge_scalar(&mut t): 16 bytes of the weight stream (thin.rs:289, common.rs:72-76)
    uint32_t ww[4];
    if (b.weights) { const uint4 v = *reinterpret_cast<const uint4 *>(b.weights + 16 * (size_t)j); ww[0] = v.x; ww[1] = v.y; ww[2] = v.z; ww[3] = v.w; }
    else WB::chunk16(wblk, j0 + jb, j0 + j, 0, ww);
    ws = thin_item_plain<S>(b, ww, c_in, z_in, j, PlainTerms<S>{scalars, pre, b.pks_xy});
  }
  const fp sum = block_sum<Fr, TERMS_NT>(ws, red);                             // of w_j s_j z0 (Montgomery form), thin.rs:303
  if (threadIdx.x == 0) fp_store(gpart + 8 * (size_t)blockIdx.x, sum);
}

// last term (G, g) -- for Pedersen the last two, on G and BLINDING_BASE
template <class S>
__global__ void __launch_bounds__(256)
k_g_final(const uint32_t *__restrict__ gpart, uint32_t nparts, uint32_t *__restrict__ scalars, te_pre *__restrict__ pre,
          uint32_t t_last, int which_base) {
  __shared__ fp red[256];
  base_term<S>(gpart, nparts, scalars, pre, t_last, which_base, red);
}


// ---------------------------------------------------------------- Pedersen batch

// pedersen::BatchItem::new (src/pedersen.rs:276-293): challenge c_j and the merged I/O pair
// (written as canonical xy to merged_xy[j], 128 bytes) for every item.
// SHARED (a batch over a table of shared inputs, thin_shared.h): the inputs stay rows of the table, so the merged INPUT is never
// computed or written -- only the merged output (merged_xy + 128 j + 64, where ped_item reads it) and, behind the n slots, the
// delinearisation scalars z_i, i >= 1, of every multi-pair item (16 bytes at merged_xy + 128 n + 16 (io0 + i); z_0 = 1 is not stored).
template <class S, bool SHARED>
__global__ void __launch_bounds__(128)
k_ped_prepare(BatchDev b, uint32_t *__restrict__ c_out, uint8_t *__restrict__ merged_xy, uint32_t *__restrict__ flags) {
  using Fr = typename S::Fr;
  uint32_t j = b.first + blockIdx.x * blockDim.x + threadIdx.x;                // the range [b.first, b.n): a whole batch, or one pushed chunk of an open one
  if (j >= b.n) return;
  uint32_t io0 = b.io_off[j], m = b.io_off[j + 1] - io0, ad0 = b.ad_off[j], adl = b.ad_off[j + 1] - ad0;
  const uint8_t *ios = b.ios_xy + 128 * (size_t)io0, *pr = b.proofs + 256 * (size_t)j;
  suite_tr<S> t; uint32_t f = 0;
  tr_base<S>(t, DS_PEDERSEN, false, nullptr, ios, m, b.ads + ad0, adl, &f);   // io identity -> io_identity flag (:278)
  uint8_t *mo = merged_xy + 128 * (size_t)j;
  if constexpr (SHARED) {
    if (m == 1) {
      const uint4 *src = reinterpret_cast<const uint4 *>(ios + 64); uint4 *dst = reinterpret_cast<uint4 *>(mo + 64);
#pragma unroll
      for (int i = 0; i < 4; i++) dst[i] = src[i];
    } else if (m == 0) {
      fp zero = fp_zero(), one = fp_zero(); one.v[0] = S::SW_NATIVE ? 0 : 1;
      fp_store_le(mo + 64, zero); fp_store_le(mo + 96, one);
    } else {                                                                   // merge_ios' output half; the z_i go to the terms kernel
      auto dseed = delin_seed(t);
      uint32_t *z_out = reinterpret_cast<uint32_t *>(merged_xy + 128 * (size_t)b.n);
      te_ext om = te_identity<S>();
      for (uint32_t i = 0; i < m; i++) {
        te_pre po = pre_from_xy<S>(ios + 128 * (size_t)i + 64);
        if (i == 0) om = te_madd<S>(om, po);
        else {
          fp z = xof128(dseed, i - 1);
          *reinterpret_cast<uint4 *>(z_out + 4 * (size_t)(io0 + i)) = make_uint4(z.v[0], z.v[1], z.v[2], z.v[3]);
          om = te_add<S>(om, te_smul<S>(po, z, 128));
        }
      }
      store_xy<S>(mo + 64, te_to_aff<S>(om));
    }
  } else if (m == 1) {
    const uint4 *src = reinterpret_cast<const uint4 *>(ios); uint4 *dst = reinterpret_cast<uint4 *>(mo);
#pragma unroll
    for (int i = 0; i < 8; i++) dst[i] = src[i];
  } else if (m == 0) {
    fp zero = fp_zero(), one = fp_zero(); one.v[0] = S::SW_NATIVE ? 0 : 1;      // identity: (0, 1), or (0, 0) for a short-Weierstrass suite
    fp_store_le(mo, zero); fp_store_le(mo + 32, one); fp_store_le(mo + 64, zero); fp_store_le(mo + 96, one);
  } else {                                                                     // merge_ios, common.rs:389-419
    auto dseed = delin_seed(t);
    te_ext im = te_identity<S>(), om = te_identity<S>();
    for (uint32_t i = 0; i < m; i++) {
      te_pre pi = pre_from_xy<S>(ios + 128 * (size_t)i), po = pre_from_xy<S>(ios + 128 * (size_t)i + 64);
      if (i == 0) { im = te_madd<S>(im, pi); om = te_madd<S>(om, po); }
      else { fp z = xof128(dseed, i - 1); im = te_add<S>(im, te_smul<S>(pi, z, 128)); om = te_add<S>(om, te_smul<S>(po, z, 128)); }
    }
    te_aff ia = te_to_aff<S>(im), oa = te_to_aff<S>(om);
    store_xy<S>(mo, ia); store_xy<S>(mo + 64, oa);
  }
  fp ybx = fp_load_le(pr), yby = fp_load_le(pr + 32), rx = fp_load_le(pr + 64), ry = fp_load_le(pr + 96);
  fp okx = fp_load_le(pr + 128), oky = fp_load_le(pr + 160);
  f |= point_flags<S>(ybx, yby);                                               // pk_com.is_zero() (:348-353)
  f |= (point_flags<S>(rx, ry) | point_flags<S>(okx, oky)) & FLAG_RANGE;
  if (ge_p<Fr>(fp_load_le(pr + 192)) || ge_p<Fr>(fp_load_le(pr + 224))) f |= FLAG_SCALAR;
  if constexpr (S::SW_CODEC) {                                                 // the three proof points' 33-byte forms, one inversion
    const fp xs[3] = {ybx, rx, okx}, ys[3] = {yby, ry, oky};
    sw_enc enc[3]; sw_encode_te_many<S, 3>(xs, ys, enc);
    absorb_sw_enc(t, enc[0]); tr_byte(t, DS_CHALLENGE); absorb_sw_enc(t, enc[1]); absorb_sw_enc(t, enc[2]);
  } else {
    absorb_point_xy<S>(t, ybx, yby);                                           // :280
    tr_byte(t, DS_CHALLENGE); absorb_point_xy<S>(t, rx, ry); absorb_point_xy<S>(t, okx, oky);
  }
  fp c = challenge_finish(t);                                                  // :281
  *reinterpret_cast<uint4 *>(c_out + 4 * (size_t)j) = make_uint4(c.v[0], c.v[1], c.v[2], c.v[3]);
  if (b.records) {                                                             // LE32(c) || LE32(s) || LE32(sb), pedersen.rs:361-367
    uint4 *r = reinterpret_cast<uint4 *>(b.records + 96 * (size_t)j);
    const uint4 *sp = reinterpret_cast<const uint4 *>(pr + 192);
    r[0] = make_uint4(c.v[0], c.v[1], c.v[2], c.v[3]); r[1] = make_uint4(0, 0, 0, 0); r[2] = sp[0]; r[3] = sp[1]; r[4] = sp[2]; r[5] = sp[3];
  }
  if (f) atomicOr(flags, f);
}

// k_ped_terms' sink of ped_item's terms: item j's five at 5 j + k
template <class S> struct PlainPedTerms {
  uint32_t *__restrict__ scalars; te_pre *__restrict__ pre;
  AVRF_DI void term(uint32_t j, uint32_t k, const fp &sc_plain, const uint8_t *xy) const { emit_term<S>(scalars, pre, 5 * j + k, sc_plain, xy); }
};

// per-item part of pedersen::BatchVerifier::verify, src/pedersen.rs:369-410 (ped_item_w, batch_terms_dev.h)
template <class S>
__global__ void __launch_bounds__(TERMS_NT)
k_ped_terms(BatchDev b, Seed64 seed, uint64_t j0, const uint32_t *__restrict__ c_in, const uint8_t *__restrict__ merged_xy,
            uint32_t *__restrict__ scalars, te_pre *__restrict__ pre, uint32_t *__restrict__ gpart, uint32_t *__restrict__ bpart) {
  using Fr = typename S::Fr; using WB = WeightBlocks<TERMS_NT, 32>;
  __shared__ fp red[TERMS_NT];
  __shared__ uint64_t wblk[WB::WORDS];
  const uint32_t jb = blockIdx.x * TERMS_NT, j = jb + threadIdx.x;
  if (!b.weights) WB::fill(seed, j0 + jb, b.n - jb < TERMS_NT ? b.n - jb : TERMS_NT, wblk);     // (uniform: every thread takes it)
  fp us = fp_zero(), usb = fp_zero();
  if (j < b.n) {
    // 32 squeezed bytes per item: t = bytes[0..16], u = bytes[16..32]   (pedersen.rs:373-381)
    fp t_plain, u_plain;
    if (b.weights) { t_plain = fp_from_u128(reinterpret_cast<const uint32_t *>(b.weights + 32 * (size_t)j)); u_plain = fp_from_u128(reinterpret_cast<const uint32_t *>(b.weights + 32 * (size_t)j + 16)); }
    else {
      uint32_t w[4];
      WB::chunk16(wblk, j0 + jb, j0 + j, 0, w); t_plain = fp_zero(); t_plain.v[0] = w[0]; t_plain.v[1] = w[1]; t_plain.v[2] = w[2]; t_plain.v[3] = w[3];
      WB::chunk16(wblk, j0 + jb, j0 + j, 1, w); u_plain = fp_zero(); u_plain.v[0] = w[0]; u_plain.v[1] = w[1]; u_plain.v[2] = w[2]; u_plain.v[3] = w[3];
    }
    us = ped_item_w<S>(b, t_plain, u_plain, c_in, merged_xy, j, PlainPedTerms<S>{scalars, pre}, usb);
  }
  const fp gsum = block_sum<Fr, TERMS_NT>(us, red);
  if (threadIdx.x == 0) fp_store(gpart + 8 * (size_t)blockIdx.x, gsum);
  __syncthreads();
  const fp bsum = block_sum<Fr, TERMS_NT>(usb, red);
  if (threadIdx.x == 0) fp_store(bpart + 8 * (size_t)blockIdx.x, bsum);
}

template <class S> void BatchOps<S>::ped_prepare(const BatchDev &b, uint32_t *d_c, uint8_t *d_merged, uint32_t *d_flags, bool shared, hipStream_t st) {
  if (b.n <= b.first) return;
  dim3 g((b.n - b.first + 127) / 128), blk(128);                                // every output is indexed by the absolute item / pair: a range writes what the whole would
  if (shared) hipLaunchKernelGGL((k_ped_prepare<S, true>), g, blk, 0, st, b, d_c, d_merged, d_flags);
  else hipLaunchKernelGGL((k_ped_prepare<S, false>), g, blk, 0, st, b, d_c, d_merged, d_flags);
}
template <class S> void BatchOps<S>::ped_terms(const BatchDev &b, const Seed64 &seed, uint64_t j0, const uint32_t *d_c, const uint8_t *d_merged,
                                               uint32_t *d_scalars, te_pre_raw *d_pre, uint32_t *d_gpart, uint32_t n_terms, hipStream_t st) {
  if (!b.n) return;
  dim3 g((b.n + TERMS_NT - 1) / TERMS_NT), blk(TERMS_NT);
  uint32_t *bp = d_gpart + 8 * (size_t)g.x;
  hipLaunchKernelGGL(k_ped_terms<S>, g, blk, 0, st, b, seed, j0, d_c, d_merged, d_scalars, (te_pre *)d_pre, d_gpart, bp);
  hipLaunchKernelGGL(k_g_final<S>, dim3(1), dim3(256), 0, st, d_gpart, g.x, d_scalars, (te_pre *)d_pre, n_terms - 2, 0);
  hipLaunchKernelGGL(k_g_final<S>, dim3(1), dim3(256), 0, st, bp, g.x, d_scalars, (te_pre *)d_pre, n_terms - 1, 1);
}
template <class S> void BatchOps<S>::thin_prepare(const BatchDev &b, uint32_t *d_c, uint32_t *d_z, uint32_t *d_flags, hipStream_t st) {
  if (b.n <= b.first) return;
  dim3 g((b.n - b.first + 127) / 128), blk(128);                                // every output is indexed by the absolute item / pair: a range writes what the whole would
  hipLaunchKernelGGL(k_thin_prepare<S>, g, blk, 0, st, b, d_c, d_z, d_flags);
}
template <class S> void BatchOps<S>::thin_terms(const BatchDev &b, const Seed64 &seed, uint64_t j0, const uint32_t *d_c, const uint32_t *d_z,
                                                uint32_t *d_scalars, te_pre_raw *d_pre, uint32_t *d_gpart, uint32_t n_terms, hipStream_t st) {
  if (!b.n) return;
  dim3 g((b.n + TERMS_NT - 1) / TERMS_NT), blk(TERMS_NT);
  hipLaunchKernelGGL(k_thin_terms<S>, g, blk, 0, st, b, seed, j0, d_c, d_z, d_scalars, (te_pre *)d_pre, d_gpart);
  hipLaunchKernelGGL(k_g_final<S>, dim3(1), dim3(256), 0, st, d_gpart, g.x, d_scalars, (te_pre *)d_pre, n_terms - 1, 0);
}
template struct BatchOps<suite_by_id<AVRF_TU_SUITE>::type>;

}  // namespace avrf
