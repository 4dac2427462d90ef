// host_te.h -- host-side (CPU) finishing arithmetic of the product: the Montgomery field on 64-bit
// limbs (any width: host_g1.h and host_pairing.h build on it) and twisted-Edwards point ops, used for the O(256) tail of an MSM (window Horner), for
// combining per-GPU partial points, and for normalising results.  This is product code (it is
// NOT the oracle and shares no source with oracle/); the heavy lifting is in the HIP kernels.
#pragma once
#include <stdint.h>
#include <string.h>
#include "consts_gen.h"

namespace avrf {

// An element: L 64-bit limbs, the device's 2 L 32-bit words read as they lie in memory.
template <int L> struct HostEl { uint64_t l[L]; };
using H256 = HostEl<4>;

// The host field: saturated Montgomery arithmetic (R = 2^(64 L)) on any field struct of consts_gen.h -- four limbs for the 256-bit
// fields (secp256r1's included: the carry out of a sum or a product joins the conditional subtraction), six for BLS12-381's base field.
template <class F> struct HostField {
  static constexpr int L = F::N / 2;                       // 64-bit limbs
  using El = HostEl<L>;
  static El from32(const uint32_t (&c)[F::N]) { El r; for (int i = 0; i < L; i++) r.l[i] = (uint64_t)c[2 * i] | ((uint64_t)c[2 * i + 1] << 32); return r; }
  static El P() { return from32(F::P); }
  static El one() { return from32(F::ONE); }
  static El r2() { return from32(F::R2); }
  static El zero() { El r; memset(&r, 0, sizeof r); return r; }
  static constexpr uint64_t p_limb(int i) { return (uint64_t)F::P[2 * i] | ((uint64_t)F::P[2 * i + 1] << 32); }
  static constexpr uint64_t ninv64() {  // -p^-1 mod 2^64 from p
    uint64_t p0 = p_limb(0), inv = 1;
    for (int i = 0; i < 7; i++) inv *= 2 - p0 * inv;
    return (uint64_t)0 - inv;
  }
  static bool is_zero(const El &a) { uint64_t o = 0; for (int i = 0; i < L; i++) o |= a.l[i]; return o == 0; }
  static bool eq(const El &a, const El &b) { uint64_t o = 0; for (int i = 0; i < L; i++) o |= a.l[i] ^ b.l[i]; return o == 0; }
  static uint64_t addc(El &o, const El &a, const El &b) {
    unsigned __int128 c = 0;
    for (int i = 0; i < L; i++) { c += (unsigned __int128)a.l[i] + b.l[i]; o.l[i] = (uint64_t)c; c >>= 64; }
    return (uint64_t)c;
  }
  static uint64_t subb(El &o, const El &a, const El &b) {
    uint64_t br = 0;
    for (int i = 0; i < L; i++) { unsigned __int128 t = (unsigned __int128)a.l[i] - b.l[i] - br; o.l[i] = (uint64_t)t; br = (uint64_t)(t >> 64) & 1; }
    return br;
  }
  static bool geq(const El &a, const El &b) { for (int i = L - 1; i >= 0; i--) if (a.l[i] != b.l[i]) return a.l[i] > b.l[i]; return true; }
  static bool geq_p(const El &a) { El t; return subb(t, a, P()) == 0; }
  static El add(const El &a, const El &b) { El t, u; uint64_t c = addc(t, a, b); uint64_t br = subb(u, t, P()); return (c || !br) ? u : t; }
  static El sub(const El &a, const El &b) { El t; if (subb(t, a, b)) addc(t, t, P()); return t; }
  static El neg(const El &a) { if (is_zero(a)) return a; El t; subb(t, P(), a); return t; }
  static El dbl(const El &a) { return add(a, a); }
  // Montgomery product, operand scanning with the reduction interleaved (CIOS); constants folded at compile time.
  // Any a < 2^(64 L) with b < p comes out reduced.
  static El mul(const El &a, const El &b) {
    constexpr uint64_t ninv = ninv64();
    uint64_t t[L + 2];
#pragma GCC unroll 16
    for (int i = 0; i < L + 2; i++) t[i] = 0;
#pragma GCC unroll 16
    for (int i = 0; i < L; i++) {
      unsigned __int128 c = 0;
#pragma GCC unroll 16
      for (int j = 0; j < L; j++) { c += (unsigned __int128)a.l[j] * b.l[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
      c += t[L]; t[L] = (uint64_t)c; t[L + 1] = (uint64_t)(c >> 64);
      const uint64_t q = t[0] * ninv;
      c = (unsigned __int128)q * p_limb(0) + t[0]; c >>= 64;
#pragma GCC unroll 16
      for (int j = 1; j < L; j++) { c += (unsigned __int128)q * p_limb(j) + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
      c += t[L]; t[L - 1] = (uint64_t)c; t[L] = t[L + 1] + (uint64_t)(c >> 64);
    }
    El r, u; for (int i = 0; i < L; i++) r.l[i] = t[i];
    uint64_t br = subb(u, r, P());
    return (t[L] || !br) ? u : r;
  }
  static El sqr(const El &a) { return mul(a, a); }
  static El to_mont(const El &a) { return mul(a, r2()); }
  static El from_mont(const El &a) { El o = zero(); o.l[0] = 1; return mul(a, o); }
  // a^(p-2): the fixed-length inversion of the 256-bit call sites (HostTe, the ring prover and verifier), and the cross-check of inv()
  static El inv_fermat(const El &a) {
    El e = from32(F::PM2), r = one();
    for (int i = 64 * L - 1; i >= 0; i--) { r = sqr(r); if ((e.l[i / 64] >> (i % 64)) & 1) r = mul(r, a); }
    return r;
  }
  // halve modulo p (p odd): x/2 if even, (x + p)/2 otherwise
  static void half_mod(El &x, const El &p) {
    uint64_t carry = 0;
    if (x.l[0] & 1) carry = addc(x, x, p);
    for (int i = 0; i < L - 1; i++) x.l[i] = (x.l[i] >> 1) | (x.l[i + 1] << 63);
    x.l[L - 1] = (x.l[L - 1] >> 1) | (carry << 63);
  }
  static void shr1(El &x) { for (int i = 0; i < L - 1; i++) x.l[i] = (x.l[i] >> 1) | (x.l[i + 1] << 63); x.l[L - 1] >>= 1; }
  // Montgomery inverse by the binary extended Euclid (about 2 * bits shift/subtract steps; ~5x faster than a^(p-2)).
  // Not constant time: public data only (G1 and pairing call sites: verifier, proof normalisation).
  static El inv(const El &a_mont) {
    const El p = P();
    El u = from_mont(a_mont), v = p, x1 = zero(), x2 = zero();
    if (is_zero(u)) return u;
    x1.l[0] = 1;
    El onep = zero(); onep.l[0] = 1;
    while (!eq(u, onep) && !eq(v, onep)) {
      while (!(u.l[0] & 1)) { shr1(u); half_mod(x1, p); }
      while (!(v.l[0] & 1)) { shr1(v); half_mod(x2, p); }
      if (geq(u, v)) { subb(u, u, v); if (subb(x1, x1, x2)) addc(x1, x1, p); }
      else { subb(v, v, u); if (subb(x2, x2, x1)) addc(x2, x2, p); }
    }
    const El r = eq(u, onep) ? x1 : x2;                       // plain inverse of the plain value
    return mul(r, r2());                                      // back to Montgomery form
  }
  static El load_le(const uint8_t *b) { El r; memcpy(r.l, b, 8 * L); return r; }
  static void store_le(uint8_t *b, const El &a) { memcpy(b, a.l, 8 * L); }
};

struct HostExt { H256 x, y, t, z; };

template <class S> struct HostTe {
  using Fq = HostField<typename S::Fq>;
  static H256 mul_a(const H256 &v) {
    if (S::A_KIND == 1) { H256 t = Fq::add(v, v); t = Fq::add(t, t); t = Fq::add(t, v); return Fq::neg(t); }
    if (S::A_KIND == 2) return Fq::neg(v);
    return v;
  }
  // S::SW_NATIVE (secp256r1): the same struct holds XYZZ coordinates (X, Y, ZZ = t, ZZZ = z), identity ZZ = 0 -- te.h
  static HostExt identity() {
    HostExt r; memset(&r, 0, sizeof r); r.y = Fq::one();
    if constexpr (S::SW_NATIVE) r.x = Fq::one(); else r.z = Fq::one();
    return r;
  }
  static bool is_identity(const HostExt &p) {
    if constexpr (S::SW_NATIVE) return Fq::is_zero(p.t);
    return Fq::is_zero(p.x) && Fq::eq(p.y, p.z);
  }
  static HostExt sw_dbl(const HostExt &a) {            // dbl-2008-s-1, a = -3
    H256 U = Fq::add(a.y, a.y), V = Fq::sqr(U), W = Fq::mul(U, V), Sx = Fq::mul(a.x, V);
    H256 M = Fq::mul(Fq::sub(a.x, a.t), Fq::add(a.x, a.t)); M = Fq::add(Fq::add(M, M), M);
    HostExt r;
    r.x = Fq::sub(Fq::sqr(M), Fq::add(Sx, Sx));
    r.y = Fq::sub(Fq::mul(M, Fq::sub(Sx, r.x)), Fq::mul(W, a.y));
    r.t = Fq::mul(V, a.t); r.z = Fq::mul(W, a.z);
    return r;
  }
  static HostExt sw_add(const HostExt &a, const HostExt &b) {   // add-2008-s with its exceptional cases
    if (Fq::is_zero(a.t)) return b;
    if (Fq::is_zero(b.t)) return a;
    H256 U1 = Fq::mul(a.x, b.t), P = Fq::sub(Fq::mul(b.x, a.t), U1);
    H256 S1 = Fq::mul(a.y, b.z), R = Fq::sub(Fq::mul(b.y, a.z), S1);
    if (Fq::is_zero(P)) return Fq::is_zero(R) ? sw_dbl(a) : identity();
    H256 PP = Fq::sqr(P), Q = Fq::mul(U1, PP), PPP = Fq::mul(P, PP), T = Fq::mul(S1, PPP);
    HostExt r;
    r.t = Fq::mul(Fq::mul(a.t, b.t), PP); r.z = Fq::mul(Fq::mul(a.z, b.z), PPP);
    r.x = Fq::sub(Fq::sub(Fq::sqr(R), PPP), Fq::add(Q, Q));
    r.y = Fq::sub(Fq::mul(R, Fq::sub(Q, r.x)), T);
    return r;
  }
  static HostExt add(const HostExt &p, const HostExt &q) {
    if constexpr (S::SW_NATIVE) return sw_add(p, q);
    static const H256 d = Fq::from32(S::D);
    H256 A = Fq::mul(p.x, q.x), B = Fq::mul(p.y, q.y), C = Fq::mul(Fq::mul(p.t, q.t), d), D = Fq::mul(p.z, q.z);
    H256 E = Fq::sub(Fq::sub(Fq::mul(Fq::add(p.x, p.y), Fq::add(q.x, q.y)), A), B);
    H256 F = Fq::sub(D, C), G = Fq::add(D, C), H = Fq::sub(B, mul_a(A));
    HostExt r; r.x = Fq::mul(E, F); r.y = Fq::mul(G, H); r.t = Fq::mul(E, H); r.z = Fq::mul(F, G); return r;
  }
  static HostExt dbl(const HostExt &p) {
    if constexpr (S::SW_NATIVE) return sw_dbl(p);
    H256 A = Fq::sqr(p.x), B = Fq::sqr(p.y), C = Fq::sqr(p.z); C = Fq::add(C, C);
    H256 D = mul_a(A), E = Fq::sub(Fq::sub(Fq::sqr(Fq::add(p.x, p.y)), A), B);
    H256 G = Fq::add(D, B), F = Fq::sub(G, C), H = Fq::sub(D, B);
    HostExt r; r.x = Fq::mul(E, F); r.y = Fq::mul(G, H); r.t = Fq::mul(E, H); r.z = Fq::mul(F, G); return r;
  }
  // canonical affine bytes x||y (LE32 each)
  static void to_affine_bytes(const HostExt &p, uint8_t out[64]) {
    if constexpr (S::SW_NATIVE) {                       // the identity: all-zero bytes
      H256 i = Fq::inv_fermat(Fq::mul(p.t, p.z));
      H256 x = Fq::from_mont(Fq::mul(p.x, Fq::mul(i, p.z))), y = Fq::from_mont(Fq::mul(p.y, Fq::mul(i, p.t)));
      Fq::store_le(out, x); Fq::store_le(out + 32, y); return;
    }
    H256 zi = Fq::inv_fermat(p.z);
    H256 x = Fq::from_mont(Fq::mul(p.x, zi)), y = Fq::from_mont(Fq::mul(p.y, zi));
    Fq::store_le(out, x); Fq::store_le(out + 32, y);
  }
  static bool from_affine_bytes(const uint8_t in[64], HostExt *o) {
    H256 x = Fq::load_le(in), y = Fq::load_le(in + 32);
    if (Fq::geq_p(x) || Fq::geq_p(y)) return false;
    if constexpr (S::SW_NATIVE) {
      if (Fq::is_zero(x) && Fq::is_zero(y)) { *o = identity(); return true; }
      o->x = Fq::to_mont(x); o->y = Fq::to_mont(y); o->t = Fq::one(); o->z = Fq::one(); return true;
    }
    o->x = Fq::to_mont(x); o->y = Fq::to_mont(y); o->t = Fq::mul(o->x, o->y); o->z = Fq::one();
    return true;
  }
  static HostExt from_raw32(const uint32_t *w) {  // device te_ext_raw -> host
    HostExt r; memcpy(&r, w, 128); return r;      // identical little-endian limb layout
  }
};

}  // namespace avrf
