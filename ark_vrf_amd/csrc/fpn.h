// fpn.h -- prime-field arithmetic for gfx950 VALU: N saturated u32 limbs, Montgomery R = 2^(32 N).  The one field layer of the
// device code: N = 8 for the 256-bit fields of the VRF suites and BN254's base field, N = 12 for the BLS12-381 base field
// (381 bits); fp256.h adds what exists for eight limbs only.
//
// Device counterpart of what the reference gets from arkworks `Fp<MontBackend<_, 4>>` / `<_, 6>` (third-party ark-ff 0.6;
// reached from src/thin.rs:289-311, src/pedersen.rs:373-410 for the scalar field, from every group operation for the base
// field, and from the KZG commit/open MSMs of the ring SNARK, w3f-ring-proof, src/ring.rs:220,404,416,731).  One field element
// per lane, limbs in VGPRs; products through v_mad_u64_u32 (mac96.h).  Most moduli leave the top bit of their top limb clear,
// which admits the carry-free forms; the two 256-bit fields of secp256r1 (F::FULL) keep bit 32 N of a sum or a Montgomery
// product and fold it into the conditional subtraction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "consts_gen.h"
#include "mac96.h"

namespace avrf {

#define AVRF_DI __device__ __forceinline__
#define AVRF_DN __device__ __noinline__ static

template <int N> struct fpn { uint32_t v[N]; };
template <class F> using fe = fpn<F::N>;
using fp = fpn<8>;

template <int N = 8> AVRF_DI fpn<N> fp_zero() { fpn<N> r;
#pragma unroll
  for (int i = 0; i < N; i++) r.v[i] = 0;
  return r; }
template <class F> AVRF_DI fe<F> fp_const(const uint32_t (&c)[F::N]) { fe<F> r;
#pragma unroll
  for (int i = 0; i < F::N; i++) r.v[i] = c[i];
  return r; }
template <class F> AVRF_DI fe<F> fp_one() { return fp_const<F>(F::ONE); }
template <int N> AVRF_DI bool fp_is_zero(const fpn<N> &a) { uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < N; i++) o |= a.v[i];
  return o == 0; }
template <int N> AVRF_DI bool fp_eq(const fpn<N> &a, const fpn<N> &b) { uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < N; i++) o |= a.v[i] ^ b.v[i];
  return o == 0; }

// r = a + b on the plain integers, returns the carry
// (carry chains through __builtin_addc / __builtin_subc: one v_addc_co_u32 / v_subb_co_u32 per limb.  The uint64_t / int64_t
// accumulator idiom compiled to ~90 instructions per field addition -- 64-bit adds, arithmetic shifts and the moves that build
// their register pairs -- against ~30 in this form; a mixed addition has eleven of them.)
template <int N> AVRF_DI uint32_t fp_addc(fpn<N> &r, const fpn<N> &a, const fpn<N> &b) {
  unsigned c = 0;
#pragma unroll
  for (int i = 0; i < N; i++) r.v[i] = __builtin_addc(a.v[i], b.v[i], c, &c);
  return c;
}
// r = a - b, returns the borrow (0/1)
template <int N> AVRF_DI uint32_t fp_subb(fpn<N> &r, const fpn<N> &a, const fpn<N> &b) {
  unsigned br = 0;
#pragma unroll
  for (int i = 0; i < N; i++) r.v[i] = __builtin_subc(a.v[i], b.v[i], br, &br);
  return br;
}
template <class F> AVRF_DI uint32_t sub_p(fe<F> &r, const fe<F> &a) {
  unsigned br = 0;
#pragma unroll
  for (int i = 0; i < F::N; i++) r.v[i] = __builtin_subc(a.v[i], (unsigned)F::P[i], br, &br);
  return br;
}
// a >= p ?  (plain integer compare)
template <class F> AVRF_DI bool ge_p(const fe<F> &a) { fe<F> t; return sub_p<F>(t, a) == 0; }
// the conditional subtraction that closes an addition or a Montgomery product: t + c 2^(32 N) < 2p  ->  [0, p)
template <class F> AVRF_DI fe<F> fp_reduce_once(fe<F> t, uint32_t c) {
  fe<F> u;
  uint32_t br = sub_p<F>(u, t);
  if constexpr (F::FULL) br = br && !c; else (void)c;   // a carry out only when the top bit of p is set
#pragma unroll
  for (int i = 0; i < F::N; i++) t.v[i] = br ? t.v[i] : u.v[i];
  return t;
}

template <class F> AVRF_DI fe<F> fp_add(const fe<F> &a, const fe<F> &b) {
  fe<F> t; const uint32_t c = fp_addc(t, a, b);
  return fp_reduce_once<F>(t, c);
}
template <class F> AVRF_DI fe<F> fp_sub(const fe<F> &a, const fe<F> &b) {
  fe<F> t; const uint32_t m = 0u - fp_subb(t, a, b);     // borrow: add p back
  unsigned c = 0;
#pragma unroll
  for (int i = 0; i < F::N; i++) t.v[i] = __builtin_addc(t.v[i], (unsigned)(F::P[i] & m), c, &c);
  return t;
}
template <class F> AVRF_DI fe<F> fp_neg(const fe<F> &a) {
  fe<F> t; unsigned br = 0; const bool z = fp_is_zero(a);
#pragma unroll
  for (int i = 0; i < F::N; i++) { const unsigned d = __builtin_subc((unsigned)F::P[i], a.v[i], br, &br); t.v[i] = z ? 0u : d; }
  return t;
}
template <class F> AVRF_DI fe<F> fp_dbl(const fe<F> &a) { return fp_add<F>(a, a); }

// Montgomery product a*b/R mod p, product scanning (mac96.h)
template <class F> AVRF_DI fe<F> fp_mul(const fe<F> &a, const fe<F> &b) {
  fe<F> r; const uint32_t c = mont_mul_ps<F::N, F>(r.v, a.v, b.v);
  return fp_reduce_once<F>(r, c);
}
template <class F> AVRF_DI fe<F> fp_sqr(const fe<F> &a) {
  fe<F> r; const uint32_t c = mont_sqr_ps<F::N, F>(r.v, a.v);
  return fp_reduce_once<F>(r, c);
}
// the operand-scanning (carry-free CIOS) form, kept as the cross-check in tools/ubench.hip (top bit of p clear)
template <class F> AVRF_DI fe<F> fp_mul_cios(const fe<F> &a, const fe<F> &b) {
  constexpr int N = F::N;
  uint32_t t[N];
#pragma unroll
  for (int i = 0; i < N; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    uint64_t A = (uint64_t)a.v[0] * b.v[i] + t[0];
    uint32_t m = (uint32_t)A * F::NINV;
    uint64_t C = (uint64_t)m * F::P[0] + (uint32_t)A;
    A >>= 32; C >>= 32;
#pragma unroll
    for (int j = 1; j < N; j++) {
      A += (uint64_t)a.v[j] * b.v[i] + t[j];
      C += (uint64_t)m * F::P[j] + (uint32_t)A;
      t[j - 1] = (uint32_t)C;
      A >>= 32; C >>= 32;
    }
    t[N - 1] = (uint32_t)(A + C);
  }
  fe<F> r;
#pragma unroll
  for (int i = 0; i < N; i++) r.v[i] = t[i];
  return fp_reduce_once<F>(r, 0);
}

template <class F> AVRF_DI fe<F> fp_to_mont(const fe<F> &a) { return fp_mul<F>(a, fp_const<F>(F::R2)); }
template <class F> AVRF_DI fe<F> fp_from_mont(const fe<F> &a) { fe<F> one = fp_zero<F::N>(); one.v[0] = 1; return fp_mul<F>(a, one); }

// the out-of-line multiplier of the per-item protocol kernels (code size / compile time, and the fence of DESIGN.md section 7-5);
// the MSM hot loops keep the force-inlined form
template <class F> AVRF_DN fe<F> fp_mul_nf(fe<F> a, fe<F> b) { return fp_mul<F>(a, b); }

// a^e for a constant exponent (plain integer of N limbs), square-and-multiply MSB first; NF: through the out-of-line multiplier
template <class F, bool NF = false> AVRF_DI fe<F> fp_pow_const(const fe<F> &a, const uint32_t (&e)[F::N]) {
  fe<F> r = fp_one<F>();
  bool started = false;
  for (int i = 32 * F::N - 1; i >= 0; i--) {
    if (started) { if constexpr (NF) r = fp_mul_nf<F>(r, r); else r = fp_sqr<F>(r); }
    if ((e[i >> 5] >> (i & 31)) & 1) {
      if (!started) r = a; else if constexpr (NF) r = fp_mul_nf<F>(r, a); else r = fp_mul<F>(r, a);
      started = true;
    }
  }
  return r;
}
// a^(p-2): the fixed-length inversion, and the cross-check of the Euclidean forms
template <class F> AVRF_DI fe<F> fp_inv(const fe<F> &a) { return fp_pow_const<F>(a, F::PM2); }

// a^-1 (0 -> 0) by the binary GCD with ONE fused step per iteration, written without branches so that the 64 different values of a wave walk the same
// instruction stream (only the trip count differs, ~1.4 x BITS +- a few):
//   u even:          u <- u / 2,        x1 <- x1 / 2
//   u odd, u >= v:   u <- (u - v) / 2,  x1 <- (x1 - x2) / 2
//   u odd, u <  v:   (u, v) <- ((v - u) / 2, u),  (x1, x2) <- ((x2 - x1) / 2, x1)
// with x1 a = u, x2 a = v (mod p), v odd throughout; u = 0 leaves v = 1, x2 = a^-1.  ~15 N carry / select instructions per step:
// ~45 k per 256-bit inversion against ~110 k (two thirds multiply-adds) for the fixed power a^(p-2): 0.23 -> ~0.1 ms of a prover
// kernel's single wave per SIMD; ~95 k against ~330 k for the 381-bit field (1.4 ms of a lone wave in k_g1_lincomb and in the
// pairing kernel).
// NF: the rescaling products go through the out-of-line multiplier (the 256-bit per-item kernels: fp_inv_nf of fp256.h) instead of being
// inlined (G1 and pairing kernels).
template <class F, bool NF = false> AVRF_DN fe<F> fp_inv_gcd(fe<F> a) {
  constexpr int N = F::N;
  const fe<F> P = fp_const<F>(F::P);
  fe<F> u = a, v = P, x1 = fp_zero<N>(), x2 = fp_zero<N>();
  x1.v[0] = 1;
#pragma unroll 1
  while (!fp_is_zero(u)) {
    const bool odd = (u.v[0] & 1u) != 0;
    fe<F> d1, d2;
    const bool lt = fp_subb(d1, u, v) != 0;                // d1 = u - v, d2 = v - u
    fp_subb(d2, v, u);
    const bool sw = odd && lt;
    fe<F> xa, xb;                                          // minuend / subtrahend of the x update
#pragma unroll
    for (int i = 0; i < N; i++) {
      const uint32_t un = odd ? (lt ? d2.v[i] : d1.v[i]) : u.v[i];
      v.v[i] = sw ? u.v[i] : v.v[i];
      u.v[i] = un;
      xa.v[i] = sw ? x2.v[i] : x1.v[i];
      xb.v[i] = odd ? (sw ? x1.v[i] : x2.v[i]) : 0u;
    }
#pragma unroll
    for (int i = 0; i < N - 1; i++) u.v[i] = (u.v[i] >> 1) | (u.v[i + 1] << 31);
    u.v[N - 1] >>= 1;
#pragma unroll
    for (int i = 0; i < N; i++) x2.v[i] = sw ? x1.v[i] : x2.v[i];
    fe<F> t = fp_sub<F>(xa, xb);                           // in [0, p)
    uint32_t c = 0;
    { const uint32_t m = 0u - (t.v[0] & 1u); fe<F> pm;     // t / 2 mod p: (t + p) / 2 when t is odd
#pragma unroll
      for (int i = 0; i < N; i++) pm.v[i] = F::P[i] & m;
      c = fp_addc(t, t, pm); }
#pragma unroll
    for (int i = 0; i < N - 1; i++) x1.v[i] = (t.v[i] >> 1) | (t.v[i + 1] << 31);
    x1.v[N - 1] = (t.v[N - 1] >> 1) | (c << 31);
  }
  const fe<F> r2 = fp_const<F>(F::R2);                    // x2 = (a' R)^-1 for a = a' R; times R^3 / R gives a'^-1 R
  if constexpr (NF) return fp_mul_nf<F>(x2, fp_mul_nf<F>(r2, r2));
  else return fp_mul<F>(x2, fp_mul<F>(r2, r2));
}

// 16-byte vectorised loads / stores of the N words of an element (N is a multiple of 4; 16-byte aligned)
template <int N = 8> AVRF_DI fpn<N> fp_load(const uint32_t *s) {
  fpn<N> r; const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
#pragma unroll
  for (int i = 0; i < N / 4; i++) { uint4 q = s4[i]; r.v[4 * i] = q.x; r.v[4 * i + 1] = q.y; r.v[4 * i + 2] = q.z; r.v[4 * i + 3] = q.w; }
  return r;
}
template <int N> AVRF_DI void fp_store(uint32_t *d, const fpn<N> &a) {
  uint4 *d4 = reinterpret_cast<uint4 *>(d);
#pragma unroll
  for (int i = 0; i < N / 4; i++) d4[i] = make_uint4(a.v[4 * i], a.v[4 * i + 1], a.v[4 * i + 2], a.v[4 * i + 3]);
}
template <int N> AVRF_DI fpn<N> fp_shfl_down(const fpn<N> &a, int delta) {
  fpn<N> r;
#pragma unroll
  for (int i = 0; i < N; i++) r.v[i] = __shfl_down(a.v[i], delta);
  return r;
}

}  // namespace avrf
