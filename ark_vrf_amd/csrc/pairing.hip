// pairing.hip -- batched pairing-product checks on gfx950: Miller loop + final exponentiation of BLS12-381 and BN254 for
//   e(A_i, Q_0) * e(B_i, Q_1) * ... == 1,   i < n   (G2 arguments fixed per setup: the KZG verifier key g2, tau g2)
//
// Device counterpart of arkworks `Pairing::multi_pairing` + `final_exponentiation` as reached from
// `RingVerifier::verify` (src/ring.rs:242) when many ring proofs are verified INDEPENDENTLY (one 2-pairing check
// each; SURVEY.md 8 a11, config C4 "4 096 independent verifies => 8 192 pairings").  The batch verifier
// (src/ring.rs:731) needs two pairings per batch and keeps using the host (host_pairing.h).
//
// The device layer -- Fp12 over sixteen lanes, the Miller loop and the final exponentiation, k_pairing_check, k_g2_lines -- is
// pairing_dev.h (its layout is described there); this unit is the host side: building the per-setup tables and launching the check.
//
// Miller loop: the G2 arguments are fixed, so the line coefficients (slope lam and c = lam x_T - y_T per doubling /
// addition step, in Fp2) are tabulated once per setup -- by k_g2_lines, ON THE DEVICE (affine G2 arithmetic over
// Fp2) -- and lane k evaluates its coefficient of the line at P = (xP, yP) as T0[k] + TX[k] xP + TY[k] yP.
// Final exponentiation: easy part with ONE Fp inversion (norm Fp12 -> Fp6 -> Fp2 -> Fp by Frobenius maps), hard part by the
// x-chain (BLS12: (x-1)^2 (x+p) (x^2+p^2-1) + 3) or plain square-and-multiply (BN254).  Only "== 1" is returned.
#include "../../include/avrf.h"
#include "fpn.h"
#include "host_pairing.h"
#include "msm.h"
#include "pairing.h"
#include "pairing_dev.h"
#include <vector>

namespace avrf {

#define HIP_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw HipFailure{e_, __FILE__, __LINE__}; } while (0)

// ---------------------------------------------------------------- host side

template <class C> static void build_impl(PairingTables &pt, const uint8_t *g2_raw, size_t nq, hipStream_t stream) {
  using HP = HostPairing<C>; constexpr int N = C::Fq::N;
  const std::vector<uint32_t> csw = pairing_consts<C>();       // constants (Montgomery form)
  // G2 arguments (Montgomery x.a | x.b | y.a | y.b)
  const size_t g2len = C::Fq::N * 4 * 4;
  std::vector<uint32_t> qw(nq * 4 * N);
  for (size_t i = 0; i < nq; i++) {
    typename HP::G2 q; HP::g2_decode(g2_raw + i * g2len, &q);
    if (q.inf) throw HipFailure{hipErrorInvalidValue, __FILE__, __LINE__};
    memcpy(&qw[(i * 4 + 0) * N], q.x.a.l, 4 * N); memcpy(&qw[(i * 4 + 1) * N], q.x.b.l, 4 * N);
    memcpy(&qw[(i * 4 + 2) * N], q.y.a.l, 4 * N); memcpy(&qw[(i * 4 + 3) * N], q.y.b.l, 4 * N);
  }
  pt.steps = (uint32_t)ate_steps<C>(); pt.nq = (uint32_t)nq; pt.words = N;
  pt.d_cst.ensure(csw.size() * 4); pt.d_tab.ensure((size_t)nq * pt.steps * 36 * N * 4);
  DevMem d_q(qw.size() * 4), d_flag(4);
  HIP_CHECK(hipMemcpyAsync(pt.d_cst.p, csw.data(), csw.size() * 4, hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipMemcpyAsync(d_q.p, qw.data(), qw.size() * 4, hipMemcpyHostToDevice, stream));
  HIP_CHECK(hipMemsetAsync(d_flag.p, 0, 4, stream));
  hipLaunchKernelGGL(k_g2_lines<C>, dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, stream, (const uint32_t *)d_q.as(), (uint32_t)nq, pt.steps,
                     (const uint32_t *)pt.d_cst.as(), pt.d_tab.as(), d_flag.as());
  uint32_t flag = 0;
  HIP_CHECK(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, stream));
  HIP_CHECK(hipStreamSynchronize(stream)); HIP_CHECK(hipGetLastError());
  if (flag) throw HipFailure{hipErrorInvalidValue, __FILE__, __LINE__};
}

void PairingTables::build(int curve, const uint8_t *g2_raw, size_t nq, hipStream_t stream) {
  release();
  if (curve == 0) build_impl<G1Bls12381>(*this, g2_raw, nq, stream); else build_impl<G1Bn254>(*this, g2_raw, nq, stream);
  this->curve = curve;
}
void PairingTables::release() { (void)d_cst.release(); (void)d_tab.release(); steps = nq = 0; }

void launch_pairing_check(const PairingTables &pt, const uint32_t *d_pts, size_t n, int32_t *d_ok, hipStream_t stream) {
  if (!n) return;
  const dim3 grid((unsigned)((n * 16 + 63) / 64)), block(64);
  if (pt.curve == 0) hipLaunchKernelGGL(k_pairing_check<G1Bls12381>, grid, block, 0, stream, d_pts, (const uint32_t *)pt.d_tab.as(), (const uint32_t *)pt.d_cst.as(),
                                        (uint32_t)n, pt.nq, pt.steps, d_ok);
  else hipLaunchKernelGGL(k_pairing_check<G1Bn254>, grid, block, 0, stream, d_pts, (const uint32_t *)pt.d_tab.as(), (const uint32_t *)pt.d_cst.as(), (uint32_t)n,
                          pt.nq, pt.steps, d_ok);
}

}  // namespace avrf
