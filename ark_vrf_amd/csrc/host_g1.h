// host_g1.h -- host-side finishing arithmetic for G1 (short Weierstrass, a = 0): XYZZ point ops
// over the host field of host_te.h, used for the O(256)-step window Horner of a
// KZG MSM and for normalising its result.  Product code (not the oracle).
#pragma once
#include <stdint.h>
#include <string.h>
#include "host_te.h"

namespace avrf {

// XYZZ points on y^2 = x^3 + b; identity <=> zz = 0.  Same limb layout as the device accumulators.
template <class C> struct HostG1 {
  using Fq = HostField<typename C::Fq>;
  using El = typename Fq::El;
  struct Pt { El x, y, zz, zzz; };
  static Pt identity() { Pt r; r.x = Fq::one(); r.y = Fq::one(); r.zz = Fq::zero(); r.zzz = Fq::zero(); return r; }
  static bool is_identity(const Pt &a) { return Fq::is_zero(a.zz); }
  static Pt from_raw32(const uint32_t *w) { Pt r; memcpy(&r, w, sizeof r); return r; }
  static Pt dbl(const Pt &a) {
    if (is_identity(a)) return a;
    El U = Fq::dbl(a.y), V = Fq::sqr(U), W = Fq::mul(U, V), S = Fq::mul(a.x, V);
    El X2 = Fq::sqr(a.x), M = Fq::add(Fq::dbl(X2), X2);
    Pt r;
    r.x = Fq::sub(Fq::sqr(M), Fq::dbl(S));
    r.y = Fq::sub(Fq::mul(M, Fq::sub(S, r.x)), Fq::mul(W, a.y));
    r.zz = Fq::mul(V, a.zz); r.zzz = Fq::mul(W, a.zzz);
    return r;
  }
  static Pt add(const Pt &a, const Pt &b) {
    if (is_identity(a)) return b;
    if (is_identity(b)) return a;
    El U1 = Fq::mul(a.x, b.zz), U2 = Fq::mul(b.x, a.zz), S1 = Fq::mul(a.y, b.zzz), S2 = Fq::mul(b.y, a.zzz);
    El P = Fq::sub(U2, U1), R = Fq::sub(S2, S1);
    if (Fq::is_zero(P)) return Fq::is_zero(R) ? dbl(a) : identity();
    El PP = Fq::sqr(P), PPP = Fq::mul(P, PP), Q = Fq::mul(U1, PP);
    Pt r;
    r.x = Fq::sub(Fq::sub(Fq::sqr(R), PPP), Fq::dbl(Q));
    r.y = Fq::sub(Fq::mul(R, Fq::sub(Q, r.x)), Fq::mul(S1, PPP));
    r.zz = Fq::mul(Fq::mul(a.zz, b.zz), PP); r.zzz = Fq::mul(Fq::mul(a.zzz, b.zzz), PPP);
    return r;
  }
  // canonical affine x || y, little-endian, 8*L bytes each; all zero for the identity
  static void to_affine_bytes(const Pt &a, uint8_t *out) {
    constexpr int B = 8 * Fq::L;
    if (is_identity(a)) { memset(out, 0, 2 * B); return; }
    El zi = Fq::inv(a.zz), zzzi = Fq::inv(a.zzz);
    El x = Fq::from_mont(Fq::mul(a.x, zi)), y = Fq::from_mont(Fq::mul(a.y, zzzi));
    memcpy(out, x.l, B); memcpy(out + B, y.l, B);
  }
  // same for many points with one field inversion (Montgomery's trick over all zz and zzz)
  static void to_affine_bytes_batch(const Pt *pts, size_t n, uint8_t *out) {
    constexpr int B = 8 * Fq::L;
    if (n == 1) { to_affine_bytes(pts[0], out); return; }
    El *pre = new El[2 * n + 1];
    El run = Fq::one();
    for (size_t i = 0; i < n; i++) {
      const bool id = is_identity(pts[i]);
      pre[2 * i] = run; if (!id) run = Fq::mul(run, pts[i].zz);
      pre[2 * i + 1] = run; if (!id) run = Fq::mul(run, pts[i].zzz);
    }
    El inv = Fq::inv(run);
    for (size_t i = n; i-- > 0;) {
      uint8_t *o = out + 2 * B * i;
      if (is_identity(pts[i])) { memset(o, 0, 2 * B); continue; }
      El zzzi = Fq::mul(inv, pre[2 * i + 1]); inv = Fq::mul(inv, pts[i].zzz);
      El zzi = Fq::mul(inv, pre[2 * i]); inv = Fq::mul(inv, pts[i].zz);
      El x = Fq::from_mont(Fq::mul(pts[i].x, zzi)), y = Fq::from_mont(Fq::mul(pts[i].y, zzzi));
      memcpy(o, x.l, B); memcpy(o + B, y.l, B);
    }
    delete[] pre;
  }
};

}  // namespace avrf
