// host_ring.h -- the host arithmetic of the ring proof (ring.hip holds the handles, the device rounds and the stream work): the
// ark-transcript and its schedule, the G1 wire codec, the proof layout, the batch randomisers and the verifier's reduction of one
// item to the scalars of its two G1 sums.  Stated ONCE for the prover and the verifier, and host-only: no HIP, no thread pool, so
// tests/cpp/host_ring_values.cpp compiles it with g++ and tests/test_host_ring_values.py compares every challenge and every scalar
// with oracle/ring_py.py, without a GPU.  Product code (not the oracle).
#pragma once
#include "../../include/avrf.h"
#include "consts_gen.h"
#include "host_g1.h"
#include "host_shake128.h"
#include "host_te.h"
#include <stdint.h>
#include <string.h>
#include <vector>

namespace avrf {

// ------------------------------------------------------------------------------------------------
// SHAKE128 + ark-transcript

struct ArkTranscript {
  HostShake128 h; bool has_len = false; uint32_t len = 0;
  void write(const void *d, size_t n) { h.update(d, n); len = (has_len ? len : 0) + (uint32_t)n; has_len = true; }
  void separate() { if (has_len) { uint8_t b[4] = {(uint8_t)(len >> 24), (uint8_t)(len >> 16), (uint8_t)(len >> 8), (uint8_t)len}; h.update(b, 4); has_len = false; } }
  void label(const char *l) { separate(); write(l, strlen(l)); separate(); }
  void label(const uint8_t *l, size_t n) { separate(); write(l, n); separate(); }
  void append(const uint8_t *d, size_t n) { separate(); write(d, n); separate(); }
  void challenge48(const char *l, uint8_t out[48]) { label(l); write("challenge", 9); h.squeeze_copy(out, 48); separate(); }
};

// ------------------------------------------------------------------------------------------------
// suite-generic host helpers

template <class S, class G> struct RingTypes {
  using Fr = HostField<typename S::Fq>;              // Fr(pairing curve) = Fq(TE curve)
  using Te = HostTe<S>;
  using HG = HostG1<G>;
  using FqN = HostField<typename G::Fq>;
  static constexpr int FQB = G::Fq::N * 4;            // bytes of a G1 coordinate
};

// int_BE(48 bytes) mod r, Montgomery form
// (hi 2^256 + lo) R = (hi R) R^2 / R + lo R: three Montgomery products -- sixteen challenges per proof on the prover AND the verifier;
// the byte-by-byte Horner form this replaces cost 96 products, 3.8 us, i.e. 60 us of a core per proof of the ~80 a proof took)
template <class F> static H256 fr_from_be48(const uint8_t b[48]) {
  using Fr = HostField<F>;
  H256 hi = {{0, 0, 0, 0}}, lo;
  for (int i = 0; i < 2; i++) { uint64_t v; memcpy(&v, b + 8 * i, 8); hi.l[1 - i] = __builtin_bswap64(v); }
  for (int i = 0; i < 4; i++) { uint64_t v; memcpy(&v, b + 16 + 8 * i, 8); lo.l[3 - i] = __builtin_bswap64(v); }
  static const H256 r2 = Fr::r2();
  return Fr::add(Fr::mul(Fr::mul(hi, r2), r2), Fr::mul(lo, r2));    // (mul reduces any 256-bit left operand: its result is below 2 p before the final subtraction)
}
template <class F> static H256 fr_pow(H256 a, uint64_t e) {
  using Fr = HostField<F>; H256 r = Fr::one();
  while (e) { if (e & 1) r = Fr::mul(r, a); a = Fr::sqr(a); e >>= 1; }
  return r;
}
template <class F> static H256 fr_small(uint64_t v) { return HostField<F>::to_mont(H256{{v, 0, 0, 0}}); }
// canonical LE32 of a Montgomery residue
template <class F> static void fr_store_le32(uint8_t *o, const H256 &mont) { const H256 p = HostField<F>::from_mont(mont); memcpy(o, p.l, 32); }

struct G1Aff { uint8_t xy[96]; bool inf; };           // canonical LE x || y (FQB bytes each)
// a result of the MSM engine or of HostG1::to_affine_bytes (x || y, fqb bytes each): the point at infinity iff all zero
static inline G1Aff g1_from_xy(const uint8_t *xy, int fqb) {
  G1Aff r; memset(&r, 0, sizeof r); memcpy(r.xy, xy, 2 * fqb);
  r.inf = true; for (int i = 0; i < 2 * fqb; i++) if (r.xy[i]) r.inf = false;
  return r;
}
// PIOP domain size of a ring (src/ring.rs:810-821): the keys, 4 more rows and the bits of the blinding, up to a power of two
static inline size_t ring_domain_size(size_t ring_size, size_t scalar_bits) {
  size_t need = ring_size + 4 + scalar_bits, N = 1; while (N < need) N <<= 1;
  return N;
}
// x || y (FQB bytes each, little-endian limbs as they lie) as two field elements, zero-extended: THE conversion of every G1 point the
// host computes with, whether canonical bytes (G1Aff::xy) or the Montgomery words the device wrote
template <class G> static void g1_coords(const uint8_t *xy, typename HostField<typename G::Fq>::El *x, typename HostField<typename G::Fq>::El *y) {
  constexpr int B = G::Fq::N * 4;
  memset(x, 0, sizeof *x); memset(y, 0, sizeof *y); memcpy(x->l, xy, B); memcpy(y->l, xy + B, B);
}

// ark-serialize G1 encodings: BLS12-381 zcash big-endian; BN254 arkworks little-endian
// (o: B bytes compressed, 2 B uncompressed, all zero on entry)
template <class G> static void g1_encode_to(const G1Aff &p, bool compressed, uint8_t *o) {
  constexpr int B = G::Fq::N * 4;
  using FqN = HostField<typename G::Fq>;
  const int len = compressed ? B : 2 * B;
  typename FqN::El y, half = FqN::from32(G::Fq::HALF), t;
  memcpy(y.l, p.xy + B, B);
  bool big = !p.inf && FqN::subb(t, half, y) != 0;    // y > (p-1)/2
  if (B == 48) {                                      // zcash
    if (p.inf) { o[0] = compressed ? 0xC0 : 0x40; return; }
    for (int i = 0; i < B; i++) o[i] = p.xy[B - 1 - i];
    if (compressed) { o[0] |= 0x80; if (big) o[0] |= 0x20; }
    else for (int i = 0; i < B; i++) o[B + i] = p.xy[2 * B - 1 - i];
  } else {
    if (p.inf) { o[len - 1] |= 0x40; return; }
    memcpy(o, p.xy, len);
    if (big) o[len - 1] |= 0x80;
  }
}
template <class G> static void g1_encode(const G1Aff &p, bool compressed, std::vector<uint8_t> &out) {
  constexpr int B = G::Fq::N * 4;
  const size_t o = out.size();
  out.resize(o + (compressed ? B : 2 * B), 0);
  g1_encode_to<G>(p, compressed, &out[o]);
}

// ---- G1 decompression (ark-serialize compressed forms); p = 3 mod 4 for both curves
template <class G> static bool g1_decompress(const uint8_t *b, G1Aff *out) {
  using FqN = HostField<typename G::Fq>; using QEl = typename FqN::El;
  constexpr int FQB = G::Fq::N * 4;
  memset(out, 0, sizeof *out);
  uint8_t le[48]; bool big, inf;
  if (FQB == 48) { inf = b[0] & 0x40; big = b[0] & 0x20; if (!(b[0] & 0x80)) return false; for (int i = 0; i < FQB; i++) le[i] = b[FQB - 1 - i]; le[FQB - 1] &= 0x1f; }
  else { inf = b[FQB - 1] & 0x40; big = b[FQB - 1] & 0x80; memcpy(le, b, FQB); le[FQB - 1] &= 0x3f; }
  if (inf) {                                                          // canonical encoding only: no sort flag, every other bit zero
    if (big) return false;
    for (int i = 0; i < FQB; i++) if (le[i]) return false;
    out->inf = true; return true;
  }
  QEl x; memcpy(x.l, le, FQB);
  QEl t; if (FqN::subb(t, x, FqN::P()) == 0) return false;           // x >= p
  QEl xm = FqN::to_mont(x);
  QEl rhs = FqN::add(FqN::mul(FqN::sqr(xm), xm), FqN::from32(G::B));
  static const QEl e = [] { QEl v = FqN::P(), one = FqN::zero(); one.l[0] = 1; FqN::addc(v, v, one);   // (p + 1) / 4
                            for (int k = 0; k < 2; k++) for (int i = 0; i < FqN::L; i++) v.l[i] = (v.l[i] >> 1) | (i + 1 < FqN::L ? v.l[i + 1] << 63 : 0);
                            return v; }();
  QEl y = FqN::one();
  for (int i = 64 * FqN::L - 1; i >= 0; i--) { y = FqN::sqr(y); if ((e.l[i / 64] >> (i % 64)) & 1) y = FqN::mul(y, rhs); }
  if (!FqN::eq(FqN::sqr(y), rhs)) return false;                       // not on the curve
  QEl yp = FqN::from_mont(y), half = FqN::from32(G::Fq::HALF);
  bool is_big = FqN::subb(t, half, yp) != 0;
  if (is_big != big) { y = FqN::neg(y); yp = FqN::from_mont(y); }
  memcpy(out->xy, x.l, FQB); memcpy(out->xy + FQB, yp.l, FQB);
  return true;
}
template <class G> static G1Aff g1_from_raw(const uint8_t *p) {       // one serialize_uncompressed G1 entry
  constexpr int FQB = G::Fq::N * 4;
  G1Aff a; memset(&a, 0, sizeof a);
  if (FQB == 48) { a.inf = p[0] & 0x40; if (!a.inf) for (int k = 0; k < FQB; k++) { a.xy[k] = p[FQB - 1 - k]; a.xy[FQB + k] = p[2 * FQB - 1 - k]; } }
  else { a.inf = p[2 * FQB - 1] & 0x40; if (!a.inf) { memcpy(a.xy, p, 2 * FQB); a.xy[2 * FQB - 1] &= 0x3f; } }
  return a;
}
// host coordinates of an affine point (HostG1's XYZZ form)
template <class G> static typename HostG1<G>::Pt g1_lift(const G1Aff &p) {
  using HG = HostG1<G>; using FqN = HostField<typename G::Fq>;
  typename HG::Pt q = HG::identity();
  if (!p.inf) { typename FqN::El x, y; g1_coords<G>(p.xy, &x, &y); q.x = FqN::to_mont(x); q.y = FqN::to_mont(y); q.zz = FqN::one(); q.zzz = FqN::one(); }
  return q;
}
// The same subgroup test as k_g1_subgroup_bls (phi(P) = [-z^2] P) on the host, for small batches: one lane of the device
// needs 2.8 ms for the two 64-bit ladders however few points there are; a host core does them in ~0.1 ms per point.
template <class G> static bool g1_in_subgroup_host(const G1Aff &a) {
  using HG = HostG1<G>; using FqN = HostField<typename G::Fq>; using QEl = typename FqN::El;
  if (G::Fq::N * 4 != 48 || a.inf) return true;                       // BN254 G1 has cofactor 1
  static const uint32_t BETA[12] = {0x798a64e8, 0x30f1361b, 0x7ece5a2a, 0xf3b8ddab, 0xc61577f7, 0x16a8ca3a,
                                    0x74fd029b, 0xc26a2ff8, 0x60701c6e, 0x3636b766, 0x241b6160, 0x051ba4ab};
  QEl beta; memcpy(beta.l, BETA, sizeof BETA > sizeof beta.l ? sizeof beta.l : sizeof BETA);
  const typename HG::Pt p = g1_lift<G>(a);
  const uint64_t z = 0xd201000000010000ull;
  typename HG::Pt q = p;
  for (int b = 62; b >= 0; b--) { q = HG::dbl(q); if ((z >> b) & 1) q = HG::add(q, p); }
  const typename HG::Pt q1 = q;
  for (int b = 62; b >= 0; b--) { q = HG::dbl(q); if ((z >> b) & 1) q = HG::add(q, q1); }
  if (HG::is_identity(q)) return false;
  return FqN::eq(q.x, FqN::mul(FqN::mul(beta, p.x), q.zz)) && FqN::eq(q.y, FqN::neg(FqN::mul(p.y, q.zzz)));
}
// coordinates < p and y^2 = x^3 + b (the point at infinity passes): the check of an UNCOMPRESSED G1 entry that ark-serialize's
// Validate::Yes makes before the subgroup test (a decompressed point is on the curve by construction)
template <class G> static bool g1_on_curve_host(const G1Aff &a) {
  using FqN = HostField<typename G::Fq>; using QEl = typename FqN::El;
  if (a.inf) return true;
  QEl x, y; g1_coords<G>(a.xy, &x, &y);
  if (FqN::geq(x, FqN::P()) || FqN::geq(y, FqN::P())) return false;
  const QEl xm = FqN::to_mont(x), ym = FqN::to_mont(y);
  return FqN::eq(FqN::sqr(ym), FqN::add(FqN::mul(FqN::sqr(xm), xm), FqN::from32(G::B)));
}

// ------------------------------------------------------------------------------------------------
// the ring proof on the wire (src/ring.rs:220): 4 G1 (witness columns) || 7 Fr (evaluations at zeta) || G1 (quotient)
// || Fr (linearisation at zeta w) || G1 || G1 (the two openings); G1 compressed, Fr canonical LE32.  The ONE statement of it: the
// prover's serialisation, the verifier and the C ABI's lengths read these.
template <class G> struct RingProofLayout {
  static constexpr size_t FQB = G::Fq::N * 4;
  static constexpr size_t EVALS = 4 * FQB, CQ = EVALS + 7 * 32, LIN_ZW = CQ + FQB, PI1 = LIN_ZW + 32, PI2 = PI1 + FQB, LEN = PI2 + FQB;
  static constexpr size_t G1_OFF[7] = {0, FQB, 2 * FQB, 3 * FQB, CQ, PI1, PI2};   // C[0..3], C_q, pi_1, pi_2: the order of every "seven points" below
  static constexpr size_t COMMITMENT_LEN = 3 * FQB;                   // the compressed RingCommitment
};
static_assert(RingProofLayout<G1Bls12381>::LEN == 592 && RingProofLayout<G1Bn254>::LEN == 480, "ring proof lengths of the reference's vectors");
static_assert(RingProofLayout<G1Bls12381>::COMMITMENT_LEN == 144 && RingProofLayout<G1Bn254>::COMMITMENT_LEN == 96, "ring commitment lengths");
static inline size_t ring_proof_len(int curve) { return curve == 0 ? RingProofLayout<G1Bls12381>::LEN : RingProofLayout<G1Bn254>::LEN; }   // curve: 0 BLS12-381, 1 BN254
static inline size_t ring_commitment_len(int curve) { return curve == 0 ? RingProofLayout<G1Bls12381>::COMMITMENT_LEN : RingProofLayout<G1Bn254>::COMMITMENT_LEN; }

template <class S, class G> struct HostRing {
  using T = RingTypes<S, G>;
  using Fr = typename T::Fr; using Te = typename T::Te;
  using F = typename S::Fq;
  using PL = RingProofLayout<G>;
  static constexpr int FQB = T::FQB;

  // generator of the evaluation domain of size n (a power of two)
  static H256 domain_root(size_t n) {
    H256 w = Fr::from32(G::ROOT_OF_UNITY);
    int lg = 0; while (((size_t)1 << lg) < n) lg++;
    for (int i = 0; i < G::TWO_ADICITY - lg; i++) w = Fr::sqr(w);
    return w;
  }
  // pts: the seven points in G1_OFF order; ev, lin_zw: Montgomery
  static void proof_serialize(const G1Aff *const pts[7], const H256 ev[7], const H256 &lin_zw, uint8_t *out) {
    memset(out, 0, PL::LEN);
    for (int j = 0; j < 7; j++) g1_encode_to<G>(*pts[j], true, out + PL::G1_OFF[j]);
    for (int i = 0; i < 7; i++) fr_store_le32<F>(out + PL::EVALS + 32 * i, ev[i]);
    fr_store_le32<F>(out + PL::LIN_ZW, lin_zw);
  }

  // ---- the Fiat-Shamir schedule, label by label.  The prover calls these between its device rounds, the
  // verifier in sequence.
  static H256 challenge(ArkTranscript &t, const char *l) { uint8_t b[48]; t.challenge48(l, b); return fr_from_be48<F>(b); }
  // suite id, "vk", the verifier key: g1_0 || g2_raw || the ring's three commitments (uncompressed) -- the same for every proof over one ring
  static ArkTranscript prelude(const G1Aff &g1_0, const std::vector<uint8_t> &g2_raw, const G1Aff C[3]) {
    ArkTranscript t;
    t.label(S::SUITE_ID, S::SUITE_ID_LEN);
    t.label("vk");
    std::vector<uint8_t> vk; g1_encode<G>(g1_0, false, vk);
    vk.insert(vk.end(), g2_raw.begin(), g2_raw.end());
    for (int i = 0; i < 3; i++) g1_encode<G>(C[i], false, vk);
    t.append(vk.data(), vk.size());
    return t;
  }
  // the instance (x || y, canonical LE32 each) and the four witness commitments -> the 7 constraint aggregation coefficients
  static void alphas(ArkTranscript &t, const uint8_t inst[64], const G1Aff C[4], H256 al[7]) {
    t.label("instance"); t.append(inst, 64);
    uint8_t b[4 * 2 * FQB] = {0}; for (int i = 0; i < 4; i++) g1_encode_to<G>(C[i], false, b + i * 2 * FQB);
    t.label("committed_cols"); t.append(b, sizeof b);
    for (int i = 0; i < 7; i++) al[i] = challenge(t, "constraints_aggregation");
  }
  // the quotient commitment -> the evaluation point
  static H256 zeta(ArkTranscript &t, const G1Aff &Cq) {
    uint8_t b[2 * FQB] = {0}; g1_encode_to<G>(Cq, false, b);
    t.label("quotient"); t.append(b, sizeof b);
    return challenge(t, "evaluation_point");
  }
  // the 7 evaluations and the linearisation's (canonical LE32, as in the proof) -> the 8 KZG aggregation coefficients
  static void nus(ArkTranscript &t, const uint8_t ev[7 * 32], const uint8_t lin_zw[32], H256 nu[8]) {
    t.label("register_evaluations"); t.append(ev, 7 * 32);
    t.label("shifted_linearization_evaluation"); t.append(lin_zw, 32);
    for (int i = 0; i < 8; i++) nu[i] = challenge(t, "kzg_aggregation");
  }

  // ---- batch randomisers: SHAKE128 over everything the batch contains, 32 bytes (r1 || r2, 128 bits each) per item
  // (the statement is bound in full: sizes, the verifier key, which ring every proof is checked against)
  static std::vector<uint8_t> batch_randomisers(size_t n, size_t n_rings, size_t N, const G1Aff &g1_0, const std::vector<uint8_t> &g2_raw,
                                                const uint32_t *ring_of_item, const uint8_t *commitments, const uint8_t *instances_xy, const uint8_t *proofs) {
    HostShake128 rh; rh.update("avrf-ring-batch", 15);
    { uint64_t hdr[3] = {(uint64_t)n, (uint64_t)n_rings, (uint64_t)N}; rh.update(hdr, sizeof hdr); }
    rh.update(g1_0.xy, 2 * FQB); rh.update(g2_raw.data(), g2_raw.size());
    for (size_t i = 0; i < n; i++) { uint32_t ri = ring_of_item ? ring_of_item[i] : 0; rh.update(&ri, 4); }
    rh.update(commitments, PL::COMMITMENT_LEN * n_rings); rh.update(instances_xy, 64 * n); rh.update(proofs, PL::LEN * n);
    std::vector<uint8_t> rnd(32 * n); rh.squeeze_copy(rnd.data(), rnd.size());
    return rnd;
  }
  // the randomisers of ONE segment of a segmented call (avrf_ring_batch_verify_segments): the items [first, first + count) of the
  // call's arrays, derived exactly as a batch call on those items alone derives them -- its own item count, its slice of
  // ring_of_item, ALL the call's commitments, its instances and proofs.  32 bytes per item of the segment into out.
  static void segment_randomisers(size_t first, size_t count, size_t n_rings, size_t N, const G1Aff &g1_0, const std::vector<uint8_t> &g2_raw,
                                  const uint32_t *ring_of_item, const uint8_t *commitments, const uint8_t *instances_xy, const uint8_t *proofs, uint8_t *out) {
    if (!count) return;
    const std::vector<uint8_t> rnd = batch_randomisers(count, n_rings, N, g1_0, g2_raw, ring_of_item ? ring_of_item + first : nullptr, commitments,
                                                       instances_xy + 64 * first, proofs + PL::LEN * first);
    memcpy(out, rnd.data(), rnd.size());
  }
  // an item's r1, r2 (Montgomery) from its 32 bytes
  static void randomiser_pair(const uint8_t rnd[32], H256 *r1, H256 *r2) {
    H256 a = {{0, 0, 0, 0}}, c = {{0, 0, 0, 0}}; memcpy(a.l, rnd, 16); memcpy(c.l, rnd + 16, 16); *r1 = Fr::to_mont(a); *r2 = Fr::to_mont(c);
  }

  // ---- RingVerifier::verify up to the group arithmetic (src/ring.rs:242): one item -> the scalars of
  //   e(sum r (C - v g1 + z pi), g2) * e(-sum r pi, tau g2) == 1
  // what depends on the setup alone, built once per call
  struct VerifierConsts {
    size_t N; H256 w, w_last, ninv, wz[3], seedx, seedy;            // w_last = w^(cap-1), cap = N - 3; wz[j] = w^(N-3+j); the accumulator seed
    VerifierConsts(size_t N_, const H256 &w_, const H256 &ninv_) : N(N_), w(w_), w_last(fr_pow<F>(w_, N_ - 4)), ninv(ninv_) {
      for (int j = 0; j < 3; j++) wz[j] = fr_pow<F>(w, N - 3 + j);
      seedx = Fr::from32(S::ACC_X); seedy = Fr::from32(S::ACC_Y);
    }
  };
  // First sum over [the ring's three commitments, the proof's seven points, g1] with s1[0..9] and -gsc; second over [pi_1, pi_2] with s2.
  struct Item {
    H256 al[7], zeta, nu[8];                                          // the challenges (Montgomery)
    H256 s1[10], s2[2];                                               // plain, as the MSM engine takes them
    H256 gsc;                                                         // Montgomery: the batch subtracts the sum of these once
  };
  // t_ring: the ring's transcript after the prelude; proof: PL::LEN bytes whose seven points decoded to pts (G1_OFF order); inst: x || y;
  // r1, r2 Montgomery (the caller's rule for a batch of one, r1 = 1, included).  AVRF_OK, or AVRF_INVALID_DATA for a scalar >= r,
  // or AVRF_VERIFICATION_FAILURE for zeta^N = 1; `o` is complete only on AVRF_OK.
  static int reduce(const VerifierConsts &vc, const ArkTranscript &t_ring, const G1Aff pts[7], const uint8_t *proof, const uint8_t inst[64],
                    const H256 &r1, const H256 &r2, Item &o) {
    const H256 one = Fr::one();
    const size_t N = vc.N; const H256 &w_last = vc.w_last, &seedx = vc.seedx, &seedy = vc.seedy;
    H256 ev[7], lin_zw;
    for (int i = 0; i < 7; i++) { H256 v = Fr::load_le(proof + PL::EVALS + 32 * i); if (Fr::geq_p(v)) return AVRF_INVALID_DATA; ev[i] = Fr::to_mont(v); }
    { H256 v = Fr::load_le(proof + PL::LIN_ZW); if (Fr::geq_p(v)) return AVRF_INVALID_DATA; lin_zw = Fr::to_mont(v); }
    H256 ix = Fr::load_le(inst), iy = Fr::load_le(inst + 32);
    if (Fr::geq_p(ix) || Fr::geq_p(iy)) return AVRF_INVALID_DATA;
    H256 ixm = Fr::to_mont(ix), iym = Fr::to_mont(iy);
    // transcript replay
    ArkTranscript t = t_ring;
    H256 *al = o.al, *nu = o.nu;
    alphas(t, inst, pts, al);
    const H256 zeta = o.zeta = HostRing::zeta(t, pts[4]);
    nus(t, proof + PL::EVALS, proof + PL::LIN_ZW, nu);
    // q(zeta) from the evaluations (A.8)
    const H256 x2 = ev[0], y2 = ev[1], sel = ev[2], b = ev[3], ip = ev[4], x1 = ev[5], y1 = ev[6];
    const H256 nl = Fr::sub(zeta, w_last), omb = Fr::sub(one, b);
    H256 zn = zeta; for (size_t k = 1; k < N; k <<= 1) zn = Fr::sqr(zn);
    const H256 zn1 = Fr::sub(zn, one);
    if (Fr::is_zero(zn1)) return AVRF_VERIFICATION_FAILURE;
    HostExt sd; sd.x = seedx; sd.y = seedy; sd.t = Fr::mul(seedx, seedy); sd.z = one;
    HostExt in; in.x = ixm; in.y = iym; in.t = Fr::mul(ixm, iym); in.z = one;
    HostExt rs = Te::add(sd, in);
    // the item's four inversions -- 1 / (zeta - 1), 1 / (zeta - w^(cap-1)) of the two Lagrange values, 1 / z of seed + instance,
    // 1 / (zeta^N - 1) -- as ONE (Montgomery's trick; a fixed-exponent inversion is 380 products, 13 us).  zeta^N != 1 was checked, so
    // the first, second and fourth are non-zero; z = 0 (an instance off the curve) keeps the old meaning: 1 / 0 = 0
    const bool z_zero = Fr::is_zero(rs.z);
    const H256 v0 = Fr::sub(zeta, one), v1 = nl, v2 = z_zero ? one : rs.z, v3 = zn1;
    const H256 p01 = Fr::mul(v0, v1), p012 = Fr::mul(p01, v2);
    H256 tinv = Fr::inv_fermat(Fr::mul(p012, v3));
    const H256 i3 = Fr::mul(tinv, p012); tinv = Fr::mul(tinv, v3);
    const H256 i2 = Fr::mul(tinv, p01); tinv = Fr::mul(tinv, v2);
    const H256 i1 = Fr::mul(tinv, v0), i0 = Fr::mul(tinv, v1);
    const H256 zn1n = Fr::mul(zn1, vc.ninv);
    const H256 lf = Fr::mul(zn1n, i0), ll = Fr::mul(Fr::mul(w_last, zn1n), i1);      // L_i(zeta) = w^i (zeta^N - 1) / (N (zeta - w^i))
    const H256 rzi = z_zero ? H256{{0, 0, 0, 0}} : i2; const H256 resx = Fr::mul(rs.x, rzi), resy = Fr::mul(rs.y, rzi);
    const H256 x1y1 = Fr::mul(x1, y1), x2y2 = Fr::mul(x2, y2);
    H256 rest[7];
    rest[0] = Fr::mul(Fr::neg(Fr::add(ip, Fr::mul(sel, b))), nl);
    rest[1] = Fr::mul(Fr::sub(Fr::mul(b, Fr::neg(Fr::add(x1y1, x2y2))), Fr::mul(omb, x1)), nl);
    rest[2] = Fr::mul(Fr::sub(Fr::mul(b, Fr::sub(x2y2, x1y1)), Fr::mul(omb, y1)), nl);
    rest[3] = Fr::mul(b, omb);
    rest[4] = Fr::add(Fr::mul(lf, Fr::sub(x1, seedx)), Fr::mul(ll, Fr::sub(x1, resx)));
    rest[5] = Fr::add(Fr::mul(lf, Fr::sub(y1, seedy)), Fr::mul(ll, Fr::sub(y1, resy)));
    rest[6] = Fr::add(Fr::mul(lf, ip), Fr::mul(ll, Fr::sub(ip, one)));
    H256 aggz = lin_zw; for (int i = 0; i < 7; i++) aggz = Fr::add(aggz, Fr::mul(al[i], rest[i]));
    H256 zk = one; for (int j = 0; j < 3; j++) zk = Fr::mul(zk, Fr::sub(zeta, vc.wz[j]));
    const H256 qz = Fr::mul(Fr::mul(aggz, zk), i3);
    H256 vagg = Fr::mul(nu[7], qz); for (int i = 0; i < 7; i++) vagg = Fr::add(vagg, Fr::mul(nu[i], ev[i]));
    const H256 a_coef = S::A_KIND == 1 ? Fr::neg(fr_small<F>(5)) : S::A_KIND == 2 ? Fr::neg(one) : one;
    const H256 k1 = Fr::add(Fr::mul(b, Fr::add(Fr::mul(y1, y2), Fr::mul(a_coef, Fr::mul(x1, x2)))), omb);
    const H256 k2 = Fr::add(Fr::mul(b, Fr::sub(Fr::mul(x1, y2), Fr::mul(x2, y1))), omb);
    const H256 zw = Fr::mul(zeta, vc.w);
    // per item: 10 terms of the first MSM (3 fixed + 4 witness + C_q + pi1 + pi2) and 2 of the second
    H256 s[10];
    for (int j = 0; j < 4; j++) s[j] = Fr::mul(r1, nu[j]);
    s[4] = Fr::add(Fr::mul(r1, nu[4]), Fr::mul(r2, Fr::mul(nl, al[0])));
    s[5] = Fr::add(Fr::mul(r1, nu[5]), Fr::mul(r2, Fr::mul(nl, Fr::mul(al[1], k1))));
    s[6] = Fr::add(Fr::mul(r1, nu[6]), Fr::mul(r2, Fr::mul(nl, Fr::mul(al[2], k2))));
    s[7] = Fr::mul(r1, nu[7]);
    s[8] = Fr::mul(r1, zeta); s[9] = Fr::mul(r2, zw);
    for (int j = 0; j < 10; j++) o.s1[j] = Fr::from_mont(s[j]);
    o.gsc = Fr::add(Fr::mul(r1, vagg), Fr::mul(r2, lin_zw));
    o.s2[0] = Fr::from_mont(Fr::neg(r1)); o.s2[1] = Fr::from_mont(Fr::neg(r2));
    return AVRF_OK;
  }
};

}  // namespace avrf
