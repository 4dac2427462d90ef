// ring.hip -- Ring-VRF membership SNARK: setup (SRS), ring indexing (`ring_proof::index`,
// src/ring.rs:404,416) and the ring prover (`RingProver::prove`, src/ring.rs:220), following the
// byte-exact specification in SURVEY.md Appendix A.5 / A.7 (w3f-ring-proof 0.0.10, un-vendored).
//
// Split of the work: proofs are proved in lockstep chunks.  On the device: the witness columns
// (expanded from their sparse description), all NTTs, the constraint aggregation on the 4N domain, quotient,
// evaluations, linearisation and opening quotients (k_ring_* / k_ntt_*, ring_dev.h) and every KZG commitment as a batched
// fixed-base MSM (msm.hip) over window tables of the SRS -- the four witness columns in the Lagrange basis, where
// they are sparse -- and (round 4) the <= 254 twisted-Edwards additions of every proof's witness accumulator with their
// batch normalisation (k_ring_witness_acc).  On host threads between the device rounds: only the Fiat-Shamir transcript
// (SHAKE128).  Verification: transcript replay and scalars on the
// host pool, two G1 MSMs on the device, one 2-pairing check on the host (host_pairing.h).
// The host arithmetic of both -- transcript schedule, G1 codec, proof layout, the verifier's reduction of an item to scalars -- is
// host_ring.h; this file keeps the handles, the table registry, setup, key, the prover's rounds, the verifier's stages and the exports.
#include "../../include/avrf.h"
#include "ring_dev.h"
#include "host_g1.h"
#include "host_pairing.h"
#include "host_ring.h"
#include "host_te.h"
#include "msm.h"
#include "pairing.h"
#include "suite_dispatch.h"
#include "host_shake128.h"
#include "host_sha512.h"
#include "host_sha256.h"
#include "host_pool.h"
#include "capi_internal.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <sys/random.h>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

namespace avrf {

// a failed HIP call unwinds to the extern "C" entry point (guarded(), capi_internal.h), which returns AVRF_ERR_NO_DEVICE
#define HIP_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw avrf::HipFailure{e_, __FILE__, __LINE__}; } while (0)

// AVRF_RING_TRACE: the phases of a prove or verify call on stderr, one line per lap(): wall time since the last lap and, for the
// prover, the PROCESS's CPU time of the phase, workers included.  `RingTrace lap(...); lap("phase");`
struct RingTrace {
  static bool on() { static const bool t = getenv("AVRF_RING_TRACE") != nullptr; return t; }
  static double now(clockid_t c) { struct timespec ts; clock_gettime(c, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }
  const char *who; size_t n; bool cpu; double t_prev, c_prev;
  RingTrace(const char *who_, size_t n_, bool cpu_) : who(who_), n(n_), cpu(cpu_) { restart(); }
  void restart() { t_prev = now(CLOCK_MONOTONIC); c_prev = cpu ? now(CLOCK_PROCESS_CPUTIME_ID) : 0; }
  double wall_ms() const { return now(CLOCK_MONOTONIC) - t_prev; }
  void operator()(const char *what) {
    if (!on()) return;
    const double t = now(CLOCK_MONOTONIC), c = cpu ? now(CLOCK_PROCESS_CPUTIME_ID) : 0;
    if (cpu) fprintf(stderr, "  %s[%zu] %-32s %8.3f ms wall %8.3f ms cpu\n", who, n, what, t - t_prev, c - c_prev);
    else fprintf(stderr, "  %s[%zu] %-28s %8.3f ms\n", who, n, what, t - t_prev);
    t_prev = t; c_prev = c;
  }
};

}  // namespace avrf

using namespace avrf;

// ------------------------------------------------------------------------------------------------
// handles

// The table of all multiples of an SRS (msm.h G1DirectTable: 164 GB for the 6 145 powers of a ring-1024 setup at c = 15) is a property
// of (device, SRS): every setup over the same SRS on a device -- the four contexts bench.py proves with, their second lanes --
// shares ONE through this registry; the last setup to go frees it.
struct DirectEntry {
  G1DirectTable t; int device = 0, kind = 0; std::vector<uint8_t> srs_key;   // kind 0: the SRS powers, 1: the witness bases derived from them
  ~DirectEntry() { if (t.d) { (void)hipSetDevice(device); free_g1_direct_table(&t); } }
};
static std::mutex g_direct_mu;
static std::vector<std::weak_ptr<DirectEntry>> g_direct;

// What ONE chunk of proofs in flight mutates: a stream, staging, the per-chunk scratch and an MSM workspace.  A setup has two, so
// that two chunks are in flight and one hides the other's host rounds.  Lane 0 runs on the context's stream and serves every
// other call on the setup; lane 1 gets a non-blocking stream of its own on the first two-lane prove call and allocates nothing
// before it is used.
struct RingLane {
  hipStream_t stream = nullptr; bool owns_stream = false;
  DevMem buf;                                         // staging for NTT batches / MSM scalars
  // per-chunk scratch: 0 witness evaluations (4 x 4N; later the opening quotients), 1 aggregated constraints (4N; later
  // the aggregated opening polynomial), 2 coefficients (4 x N), 3 parameter block, 4 quotient, 5 linearisation
  DevMem scr[6];
  MsmWorkspace ws;
  uint32_t *scratch(int which, size_t bytes) { scr[which].ensure(bytes); return scr[which].as(); }
  // A scratch slot cut into typed fields: carve().take(p, count) ... .into(which).  Every field's size and its pointer come from the
  // ONE request that names it; each field starts on a 256-byte boundary, in the order taken; into() is the slot's one scratch() call.
  struct Carve {
    static constexpr int MAX_FIELDS = 12;
    RingLane &ln; size_t total = 0; int nf = 0; struct { void *ptr; size_t off; void (*set)(void *, uint8_t *); } f[MAX_FIELDS];
    template <class T> Carve &take(T *&p, size_t count) {
      if (nf == MAX_FIELDS) throw HipFailure{hipErrorInvalidValue, __FILE__, __LINE__};
      f[nf++] = {&p, total, [](void *ptr, uint8_t *at) { *(T **)ptr = (T *)at; }}; total += (count * sizeof(T) + 255) / 256 * 256;
      return *this;
    }
    void into(int which) { uint8_t *base = (uint8_t *)ln.scratch(which, total); for (int i = 0; i < nf; i++) f[i].set(f[i].ptr, base + f[i].off); }
  };
  Carve carve() { return Carve{*this}; }
  RingLane() = default;
  RingLane(const RingLane &) = delete;
  RingLane &operator=(const RingLane &) = delete;
  ~RingLane() { ws.release(); if (owns_stream) (void)hipStreamDestroy(stream); }   // (the workspace before the stream it ran on)
};

// Everything outside the two lanes is SHARED by the chunks in flight and read-only while they are: whatever a chunk needs built on
// first use (the witness table, the tables of all multiples) is built by avrf_ring_prove before its threads start, on lane 0.
// `delete` releases everything but the registry references, which avrf_ring_setup_free drops under g_direct_mu first.
struct avrf_ring_setup {
  avrf_ctx *ctx; int suite; int curve; int device;    // curve: pairing curve of the suite (0 BLS12-381, 1 BN254)
  size_t N, cap, keyset, L, n_srs;                    // n_srs = 0: verifier-only setup (PcsVerifierParams), no SRS on the device
  DevMem d_srs;                                       // n_srs Montgomery affine points
  DevMem d_srs_table; int table_c = 0, table_nwin = 0;   // fixed-base window table over the SRS (batched commits)
  std::shared_ptr<DirectEntry> direct, direct_wit; bool direct_tried = false;   // the tables of all multiples (SRS powers; witness bases), built on first use
  uint64_t table_budget = UINT64_MAX;                 // HBM the two tables may take (avrf_ring_setup_set_table_budget; UINT64_MAX: the process default)
  uint64_t planned_budget = UINT64_MAX;               // the budget the tables held now were planned under
  bool table_missed = false;                          // a planned table was not built (did not fit, allocation or build failed): bucket form for it
  std::atomic<uint64_t> table_batches{0};             // commitment batches served from the tables (both lanes count)
  DevMem d_wit_bases;                                 // the 2N + 1 witness bases the tables are built over
  int wit_c = 0, wit_nwin = 0;                        // window width of the witness table (sparse MSMs: few entries, small buckets)
  DevMem d_wit_table;                                 // same over [L_i(tau) G, i < N | prefix sums PS_k = sum_{i<k} L_i(tau) G, k <= N] (witness commits)
  std::unique_ptr<void, void (*)(void *)> host_lines{nullptr, nullptr};   // host Miller-loop line tables of (g2, tau g2), built on first use
  G1Aff g1_0;                                         // powers_in_g1[0]
  std::vector<uint8_t> g2_raw;                        // powers_in_g2[0..2] exactly as in the SRS file
  std::vector<uint8_t> g1_raw;                        // the n_srs powers_in_g1 this setup keeps, serialize_uncompressed encoding
  std::vector<uint8_t> lag_raw;                       // L_i(tau) G, i < N (RingBuilderPcsParams), same encoding; filled by ensure_lagrange
  H256 w, w4;                                         // domain generators (Montgomery)
  DevMem d_tw_n, d_tw_n_inv, d_tw_4n, d_tw_4n_inv;
  H256 ninv, n4inv;
  std::vector<std::pair<H256, H256>> h_pows;          // 2^i * BLINDING_BASE, affine Montgomery
  DevMem d_l4;                                        // L_first | L_last evaluated on the 4N domain (2 x 4N)
  PairingTables ptab; bool ptab_ready = false;        // line tables of (g2, tau g2) for the device pairing checks (built on first use)
  std::vector<uint8_t> seg_sums; size_t seg_sums_n = 0;   // the last segmented verification's two G1 sums per segment (avrf_ring_segment_sums); n = 0: none
  RingLane lane[2];
};
static_assert(!std::is_copy_constructible<avrf_ring_setup>::value && !std::is_copy_assignable<avrf_ring_setup>::value,
              "a setup owns device memory and its lanes: a lane is a member, never a copy");
struct avrf_ring_key {
  avrf_ring_setup *setup;
  size_t n_keys;
  std::vector<std::pair<H256, H256>> points;          // cap-1 points, affine Montgomery
  std::vector<H256> px, py, sel;                      // evaluations (N each, Montgomery)
  std::vector<H256> px_poly, py_poly, sel_poly;       // coefficients
  std::vector<H256> px4, py4, sel4;                   // evaluations on the 4N domain
  G1Aff C[3];
  DevMem d_fixed4;                                    // px4 | py4 | sel4 on the device (3 x 4N)
  DevMem d_fixed_coef;                                // px | py | sel coefficients on the device (3 x N)
  DevMem d_points_pre;                                // the ring's points (keys, padding, blinding-base powers) as te_pre {x, y, d x y}: k_ring_witness_acc
};

// VerifierKeyBuilder (src/ring.rs:539-637): the ring commitment under construction
struct avrf_ring_vk_builder {
  avrf_ring_setup *setup;
  size_t curr = 0;                                    // keys appended so far
  G1Aff C[3];                                         // commitments to the x, y and selector columns of the partial ring
};

extern "C" hipStream_t avrf_ctx_stream_(avrf_ctx *c);
extern "C" int avrf_ctx_busy_(avrf_ctx *c);     // a three-call batch run is open on the context (capi.hip): its stream is taken
extern "C" int avrf_ctx_suite_(avrf_ctx *c);
extern "C" int avrf_ctx_device_(avrf_ctx *c);

namespace {

// The layout of a segmented verification (include/avrf.h avrf_ring_segments_layout; host arithmetic only): every segment is two
// vectors of L = 10 (longest segment) + 1 terms, and a round is as many consecutive segments as ONE segmented chain takes: its virtual
// windows (2 per_round windows(L) <= AVRF_SEGMENTS_WINDOWS_MAX, with the windows of a 256-bit scalar: no curve's are more), its
// padded terms (2 per_round L <= AVRF_SEGMENTS_PADDED_TERMS_MAX) and its 32-bit entry offsets.
constexpr size_t RING_SEGMENT_ITEMS_MAX = ((size_t)AVRF_SEGMENT_TERMS_MAX - 1) / 10;   // 10 items + 1 terms in the longer vector: 819
struct RingSegLayout {
  uint64_t L = 1, rounds = 0, padded = 0, c = 0; size_t per_round = 1;
  std::vector<uint32_t> off;                          // n_seg + 1 item offsets
};
static int ring_segments_layout(size_t n, size_t n_seg, const uint32_t *seg_items, RingSegLayout &o) {
  if ((n_seg && !seg_items) || n_seg > 0x0fffffffULL || n > 0xffffffffULL) return AVRF_ERR_BAD_ARG;
  o.off.assign(n_seg + 1, (uint32_t)n);
  uint64_t at = 0, longest = 0;
  for (size_t v = 0; v < n_seg; v++) {
    const uint64_t items = seg_items[v];
    if (items > RING_SEGMENT_ITEMS_MAX || at + items > n) return AVRF_ERR_BAD_ARG;
    o.off[v] = (uint32_t)at; at += items;
    if (items > longest) longest = items;
  }
  if (at != n) return AVRF_ERR_BAD_ARG;
  o.L = 10 * longest + 1; o.c = (uint64_t)msm_segments_window_bits((size_t)o.L);
  const uint64_t nwin = (257 + o.c - 1) / o.c;
  uint64_t per = (uint64_t)AVRF_SEGMENTS_WINDOWS_MAX / (2 * nwin);
  if (per > (uint64_t)AVRF_SEGMENTS_PADDED_TERMS_MAX / (2 * o.L)) per = (uint64_t)AVRF_SEGMENTS_PADDED_TERMS_MAX / (2 * o.L);
  if (per > 0xfffeffffull / (2 * nwin * o.L)) per = 0xfffeffffull / (2 * nwin * o.L);
  o.per_round = (size_t)per;                          // >= 64: L <= AVRF_SEGMENT_TERMS_MAX
  o.rounds = (n_seg + per - 1) / per;
  o.padded = 2 * (n_seg < per ? n_seg : per) * o.L;
  return AVRF_OK;
}

template <class S, class G> struct Ring {
  using T = RingTypes<S, G>;
  using Fr = typename T::Fr; using Te = typename T::Te;
  using F = typename S::Fq;
  using HR = HostRing<S, G>;                          // the host arithmetic (host_ring.h)
  using PL = RingProofLayout<G>;
  static constexpr int FQB = T::FQB;

  static DevMem make_twiddles(H256 w, size_t n) {
    std::vector<H256> tw(n / 2);
    H256 x = Fr::one();
    for (size_t i = 0; i < n / 2; i++) { tw[i] = x; x = Fr::mul(x, w); }
    DevMem d((n / 2) * 32); HIP_CHECK(hipMemcpy(d.p, tw.data(), (n / 2) * 32, hipMemcpyHostToDevice));
    return d;
  }
  static void g1_from_xy_batch(const std::vector<uint8_t> &xy, size_t batch, G1Aff *out) {
    for (size_t b = 0; b < batch; b++) out[b] = g1_from_xy(&xy[b * 2 * FQB], FQB);
  }
  // in-place (i)NTT of `batch` vectors of size n held on the host, via the device
  static void ntt(avrf_ring_setup *su, RingLane &ln, std::vector<H256> &v, size_t n, size_t batch, bool inverse) {
    ln.buf.ensure(n * batch * 32);
    HIP_CHECK(hipMemcpyAsync(ln.buf.p, v.data(), n * batch * 32, hipMemcpyHostToDevice, ln.stream));
    const DevMem &tw = n == su->N ? (inverse ? su->d_tw_n_inv : su->d_tw_n) : (inverse ? su->d_tw_4n_inv : su->d_tw_4n);
    fp sc; H256 k = n == su->N ? su->ninv : su->n4inv; memcpy(sc.v, k.l, 32);
    ntt_launch<F>(ln.buf.as(), (uint32_t)n, tw.as(), (uint32_t)batch, inverse ? &sc : nullptr, ln.stream);
    HIP_CHECK(hipMemcpyAsync(v.data(), ln.buf.p, n * batch * 32, hipMemcpyDeviceToHost, ln.stream));
    HIP_CHECK(hipStreamSynchronize(ln.stream));
  }
  // `batch` KZG commits in one launch chain: coeffs = batch vectors of length n (Montgomery; pad with zeros)
  static void commit_batch(avrf_ring_setup *su, RingLane &ln, const H256 *coeffs_mont, size_t n, size_t batch, G1Aff *out) {
    std::vector<H256> plain(n * batch);
    for (size_t i = 0; i < n * batch; i++) plain[i] = Fr::from_mont(coeffs_mont[i]);
    ln.buf.ensure(n * batch * 32);
    HIP_CHECK(hipMemcpyAsync(ln.buf.p, plain.data(), n * batch * 32, hipMemcpyHostToDevice, ln.stream));
    std::vector<uint8_t> xy(batch * 2 * FQB);
    msm_g1_device(su->curve, su->d_srs.as(), ln.buf.as(), n, ln.ws, ln.stream, xy.data(), batch);
    g1_from_xy_batch(xy, batch, out);
  }

  // a handle with what both loaders fill alike: identity, lane 0 on the context's stream, sizes and the domain constants
  static std::unique_ptr<avrf_ring_setup> new_setup(avrf_ctx *ctx, size_t N, size_t n_srs) {
    auto su = std::make_unique<avrf_ring_setup>();
    su->ctx = ctx; su->suite = S::ID; su->curve = pairing_curve_of(S::ID); su->lane[0].stream = avrf_ctx_stream_(ctx); su->device = avrf_ctx_device_(ctx);
    su->N = N; su->cap = N - 3; su->L = S::Fr::BITS; su->keyset = su->cap - su->L - 1; su->n_srs = n_srs;
    su->w4 = HR::domain_root(4 * N); su->w = Fr::sqr(Fr::sqr(su->w4));
    su->ninv = Fr::inv_fermat(fr_small<F>(N)); su->n4inv = Fr::inv_fermat(fr_small<F>(4 * N));
    return su;
  }

  // ---- setup: parse `URS { powers_in_g1, powers_in_g2 }` (serialize_uncompressed), src/ring.rs:380-393,1412-1421
  static int setup_load(avrf_ctx *ctx, const uint8_t *srs, size_t len, size_t ring_size, avrf_ring_setup **out) {
    const size_t L = S::Fr::BITS, N = ring_domain_size(ring_size, L), pcs = 3 * N + 1;
    if (len < 8) return AVRF_INVALID_DATA;
    uint64_t cnt; memcpy(&cnt, srs, 8);
    const size_t e1 = 2 * FQB, e2 = 4 * FQB;
    // serialize_compressed form of the same object (RingSetup / PcsParams, src/ring.rs:484-521): decompress on the host pool
    // and continue with the equivalent uncompressed bytes
    std::vector<uint8_t> unc;
    if (cnt <= (len - 8) / FQB && len >= 8 + cnt * FQB + 8) {
      uint64_t c2; memcpy(&c2, srs + 8 + cnt * FQB, 8);
      if (len == 8 + cnt * FQB + 8 + c2 * 2 * FQB && len != 8 + cnt * e1 + 8 + c2 * e2) {
        if (cnt < pcs || c2 < 2) return AVRF_RING_CAPACITY_EXCEEDED;
        using HP = HostPairing<G>;
        std::vector<G1Aff> pts(pcs);
        std::atomic<int> bad{0};
        parallel_for(pcs, [&](size_t i) { if (!g1_decompress<G>(srs + 8 + i * FQB, &pts[i])) bad = 1; });
        if (bad) return AVRF_INVALID_DATA;
        unc.resize(8);
        { uint64_t v = pcs; memcpy(unc.data(), &v, 8); }
        for (size_t i = 0; i < pcs; i++) g1_encode<G>(pts[i], false, unc);
        { uint64_t v = 2; size_t o = unc.size(); unc.resize(o + 8); memcpy(&unc[o], &v, 8); }
        for (int i = 0; i < 2; i++) {
          typename HP::G2 q;
          if (!HP::g2_decode_compressed(srs + 8 + cnt * FQB + 8 + (size_t)i * 2 * FQB, &q)) return AVRF_INVALID_DATA;
          size_t o = unc.size(); unc.resize(o + e2); HP::g2_encode(q, &unc[o]);
        }
        srs = unc.data(); len = unc.size(); memcpy(&cnt, srs, 8);
      }
    }
    if (len < 8 + cnt * e1 + 8) return AVRF_INVALID_DATA;
    uint64_t cnt2; memcpy(&cnt2, srs + 8 + cnt * e1, 8);
    if (len != 8 + cnt * e1 + 8 + cnt2 * e2) return AVRF_INVALID_DATA;
    if (cnt < pcs || cnt2 < 2) return AVRF_RING_CAPACITY_EXCEEDED;      // src/ring.rs:382-384
    std::unique_ptr<avrf_ring_setup> owner = new_setup(ctx, N, pcs);
    avrf_ring_setup *su = owner.get(); RingLane &ln = su->lane[0];
    std::vector<uint8_t> le(pcs * e1);
    for (size_t i = 0; i < pcs; i++) { const G1Aff a = g1_from_raw<G>(srs + 8 + i * e1); memcpy(&le[i * e1], a.xy, e1); }   // (infinity: all zero)
    memcpy(su->g1_0.xy, le.data(), e1); su->g1_0.inf = false;
    su->g2_raw.assign(srs + 8 + cnt * e1 + 8, srs + 8 + cnt * e1 + 8 + 2 * e2);
    su->g1_raw.assign(srs + 8, srs + 8 + pcs * e1);
    HIP_CHECK(hipSetDevice(su->device));
    {
      DevMem d_le(le.size()), d_flag(4); uint32_t flag = 0;
      su->d_srs.ensure(pcs * e1);
      HIP_CHECK(hipMemcpy(d_le.p, le.data(), le.size(), hipMemcpyHostToDevice)); HIP_CHECK(hipMemsetAsync(d_flag.p, 0, 4, ln.stream));   // (the flag reset in stream order with the kernel: the null stream does not order with a non-blocking one)
      launch_g1_bases(su->curve, d_le.as<uint8_t>(), pcs, su->d_srs.as(), d_flag.as(), ln.stream);
      HIP_CHECK(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, ln.stream)); HIP_CHECK(hipStreamSynchronize(ln.stream));
      if (flag) return AVRF_INVALID_DATA;
    }
    {  // fixed-base window table: T[w][i] = 2^(c w) * tau^i G, all windows of a commit then share one bucket set
      // window width from the size of the commitments (3N + 1 coefficients): wider windows save bucket additions (k_accumulate:
      // one per table row and coefficient), narrower ones save bucket REDUCTION (k_bucket_sum + k_wsum: 2^(c-1) buckets per set).
      // Which wins depends on what else runs: ONE context alone prefers narrow windows (ring 1024, N = 2048, BLS12-381:
      // c = 12 / 11 / 10 / 9 -> 11.1 / 11.4 / 11.6 / 10.8 k proofs/s -- its latency-bound reductions sit on the critical path),
      // FOUR contexts sharing the chip, as bench.py and a loaded server run it, hide each other's reductions and pay for
      // additions only: c = 11 / 12 / 13 -> 13.8 / 14.4 / 13.8 k; BN254 ring 4096 (N = 8192): c = 12 / 13 -> 7.39 / 7.56 k
      // (tools/ring4_bench.py with AVRF_RING_TABLE_C swept).  The loaded regime decides: c = log2(3N + 1) rounded down
      // (381-bit curve), one less on the 254-bit curve whose additions are cheaper relative to its reductions.
      { int lg = 0; while (((size_t)2 << lg) <= pcs) lg++;                    // floor(log2(3N + 1)) = log2(N) + 1
        su->table_c = G::Fq::N > 8 ? lg : lg - 1;
        if (su->table_c < 8) su->table_c = 8; if (su->table_c > 13) su->table_c = 13; }
      if (const char *e = getenv("AVRF_RING_TABLE_C")) { int v = atoi(e); if (v >= 4 && v <= 14) su->table_c = v; }
      {
        su->table_nwin = (G::Fr::BITS + 1 + su->table_c - 1) / su->table_c;
        su->d_srs_table.ensure((size_t)su->table_nwin * pcs * e1);
        build_g1_table(su->curve, su->d_srs.as(), pcs, su->table_c, su->table_nwin, su->d_srs_table.as(), ln.stream);
        HIP_CHECK(hipStreamSynchronize(ln.stream));
      }
    }
    su->d_tw_n = make_twiddles(su->w, N); su->d_tw_n_inv = make_twiddles(Fr::inv_fermat(su->w), N);
    su->d_tw_4n = make_twiddles(su->w4, 4 * N); su->d_tw_4n_inv = make_twiddles(Fr::inv_fermat(su->w4), 4 * N);
    {  // Lagrange basis polynomials of rows 0 and cap-1, evaluated on the 4N domain (shared by every proof)
      const H256 zero = {{0, 0, 0, 0}};
      std::vector<H256> lfl(2 * N, zero); lfl[0] = Fr::one(); lfl[N + su->cap - 1] = Fr::one();
      ntt(su, ln, lfl, N, 2, true);
      std::vector<H256> l4(2 * 4 * N, zero);
      for (size_t i = 0; i < N; i++) { l4[i] = lfl[i]; l4[4 * N + i] = lfl[N + i]; }
      ntt(su, ln, l4, 4 * N, 2, false);
      su->d_l4.ensure(l4.size() * 32); HIP_CHECK(hipMemcpy(su->d_l4.p, l4.data(), l4.size() * 32, hipMemcpyHostToDevice));
    }
    // 2^i * H  (A.5)
    HostExt h; h.x = Fr::from32(S::B_X); h.y = Fr::from32(S::B_Y); h.t = Fr::mul(h.x, h.y); h.z = Fr::one();
    for (size_t i = 0; i < L; i++) {
      H256 zi = Fr::inv_fermat(h.z); su->h_pows.push_back({Fr::mul(h.x, zi), Fr::mul(h.y, zi)});
      h = Te::dbl(h);
    }
    *out = owner.release();
    return AVRF_OK;
  }

  // ---- verifier-only setup (src/ring.rs:466-482 verifier_key_from_commitment: "verifier-only users: no SRS required"):
  // built from PcsVerifierParams = RawKzgVerifierKey { g1, g2, tau_in_g2 } (RingSetup::pcs_verifier_params, src/ring.rs:435)
  // in either ark-serialize mode.  Carries what the verifiers use -- domain, g1, (g2, tau g2) -- and no SRS: index / prove /
  // builder / serialisation of the full setup answer AVRF_SRS_LOOKUP_FAILED on such a handle.
  static int verifier_setup_load(avrf_ctx *ctx, const uint8_t *vp, size_t len, size_t ring_size, avrf_ring_setup **out) {
    using HP = HostPairing<G>;
    const size_t e1 = 2 * FQB, e2 = 4 * FQB;
    G1Aff g1; std::vector<uint8_t> g2(2 * e2);
    if (len == e1 + 2 * e2) {
      g1 = g1_from_raw<G>(vp);
      memcpy(g2.data(), vp + e1, 2 * e2);
      typename HP::G2 q;
      for (int i = 0; i < 2; i++) if (!HP::g2_decode(g2.data() + (size_t)i * e2, &q) || q.inf || !HP::g2_on_twist(q)) return AVRF_INVALID_DATA;
    } else if (len == FQB + 2 * 2 * FQB) {
      if (!g1_decompress<G>(vp, &g1)) return AVRF_INVALID_DATA;
      for (int i = 0; i < 2; i++) {
        typename HP::G2 q;
        if (!HP::g2_decode_compressed(vp + FQB + (size_t)i * 2 * FQB, &q)) return AVRF_INVALID_DATA;
        HP::g2_encode(q, g2.data() + (size_t)i * e2);
      }
    } else return AVRF_INVALID_DATA;
    // g1: in range, on the curve, in the prime-order subgroup, not the point at infinity (the uncompressed form carries both
    // coordinates, so the curve equation is checked here; BN254 G1 has cofactor 1).  The two G2 points are decoded and checked to
    // lie on the twist; like the reference's RingSetup deserialisation they get no G2 subgroup test -- PcsVerifierParams are
    // trusted-setup material published with the ring parameters, not per-proof input (src/ring.rs:466-474).
    if (g1.inf || !g1_on_curve_host<G>(g1) || !g1_in_subgroup_host<G>(g1)) return AVRF_INVALID_DATA;
    std::unique_ptr<avrf_ring_setup> su = new_setup(ctx, ring_domain_size(ring_size, S::Fr::BITS), 0);
    su->g1_0 = g1; su->g2_raw = g2;
    *out = su.release();
    return AVRF_OK;
  }
  static int verifier_params_serialize(avrf_ring_setup *su, bool compress, std::vector<uint8_t> &o) {
    using HP = HostPairing<G>;
    g1_encode<G>(su->g1_0, compress, o);
    if (!compress) { o.insert(o.end(), su->g2_raw.begin(), su->g2_raw.end()); return AVRF_OK; }
    for (int i = 0; i < 2; i++) {
      typename HP::G2 q; HP::g2_decode(su->g2_raw.data() + (size_t)i * 4 * FQB, &q);
      size_t at = o.size(); o.resize(at + 2 * FQB); HP::g2_encode_compressed(q, &o[at]);
    }
    return AVRF_OK;
  }

  // ---- RingSetup::from_seed (src/ring.rs:359-366) as the reference derives it: S::Transcript::new(SUITE_ID), absorb_raw(seed),
  // to_rng() (src/utils/transcript.rs:61-92: every draw is the next bytes of the squeeze stream), then Kzg::setup(pcs_domain_size - 1,
  // rng) = w3f-pcs URS::generate: tau = Fr::rand, g1 = G1::rand, g2 = G2::rand, powers tau^i g1 / g2.  **UNPINNED**: the reference holds
  // no vector of a seeded setup; the draw order and the samplers are restated from the published code of ark-ff
  // (Fp::rand: N x next_u64 limbs, top limb masked to the modulus' bits, taken AS the Montgomery representation, rejected if >= p;
  // Fp2: c0 then c1), ark-ec (Projective::rand: x = BaseField::rand, greatest = next_u32's top bit, the larger / smaller root by the
  // field's Ord, times the cofactor) and rand 0.8, and checked against oracle/ring_py.py srs_from_seed, which restates the same.
  struct SeedStream {
    std::vector<uint8_t> buf; size_t pos = 0; uint8_t dig[64]; uint64_t blk = 0;
    const uint8_t *absorbed; size_t absorbed_len;
    void more(size_t n) {
      if constexpr (S::XOF_SHAKE) { HostShake128 h; h.update(absorbed, absorbed_len); buf.resize(pos + n + 4096); h.squeeze_copy(buf.data(), buf.size()); }
      else if constexpr (S::TR_SHA256) { HostSha256 h; h.update(absorbed, absorbed_len); buf.resize(pos + n + 4096); h.squeeze_copy(buf.data(), buf.size()); }
      else {                                                           // DigestXof over SHA-512: d = H(absorbed), block_i = H(d || LE64(i))
        if (!blk && buf.empty()) { HostSha512 h; h.update(absorbed, absorbed_len); h.final(dig); }
        while (buf.size() < pos + n) { HostSha512 h; h.update(dig, 64); uint8_t c[8]; for (int i = 0; i < 8; i++) c[i] = (uint8_t)(blk >> (8 * i)); h.update(c, 8);
          uint8_t o[64]; h.final(o); buf.insert(buf.end(), o, o + 64); blk++; }
      }
    }
    void take(uint8_t *out, size_t n) { if (pos + n > buf.size()) more(n); memcpy(out, buf.data() + pos, n); pos += n; }
    bool boolean() { uint8_t b[4]; take(b, 4); return (b[3] & 0x80) != 0; }                     // (rng.next_u32() as i32) < 0
    template <int L, int BITS> void field(uint64_t *v, const uint64_t *p) {                     // ark-ff Fp::rand: the limbs ARE the Montgomery form
      for (;;) {
        uint8_t b[8 * L]; take(b, sizeof b); memcpy(v, b, sizeof b);
        constexpr int shave = 64 * L - BITS;
        if (shave) v[L - 1] &= ~(uint64_t)0 >> shave;
        bool less = false;
        for (int i = L - 1; i >= 0; i--) if (v[i] != p[i]) { less = v[i] < p[i]; break; }
        if (less) return;
      }
    }
  };
  static int setup_from_seed(avrf_ctx *ctx, const uint8_t seed[32], size_t ring_size, avrf_ring_setup **out) {
    using HP = HostPairing<G>; using HG = typename T::HG;
    std::vector<uint8_t> ab(S::SUITE_ID, S::SUITE_ID + S::SUITE_ID_LEN); ab.insert(ab.end(), seed, seed + 32);
    SeedStream st; st.absorbed = ab.data(); st.absorbed_len = ab.size();
    // tau = Fr::rand: the drawn limbs are tau's Montgomery form
    H256 tau_m; { const H256 pr = Fr::P(); st.template field<4, G::Fr::BITS>(tau_m.l, pr.l); }
    const H256 tau = Fr::from_mont(tau_m);
    uint8_t tau_le[32]; memcpy(tau_le, tau.l, 32);
    // g1 = G1::rand: first x with x^3 + b a square, the root picked by `greatest`, times the cofactor
    std::vector<uint8_t> g1_urs, g2_urs(4 * FQB);
    for (;;) {
      const QEl pq = FqN::P(); QEl xm; st.template field<FqN::L, G::Fq::BITS>(xm.l, pq.l);
      const bool greatest = st.boolean();
      const QEl rhs = FqN::add(FqN::mul(FqN::sqr(xm), xm), FqN::from32(G::B));
      static const QEl e = [] { QEl v = FqN::P(), one = FqN::zero(); one.l[0] = 1; FqN::addc(v, v, one);   // (p + 1) / 4
                                for (int k = 0; k < 2; k++) for (int i = 0; i < FqN::L; i++) v.l[i] = (v.l[i] >> 1) | (i + 1 < FqN::L ? v.l[i + 1] << 63 : 0);
                                return v; }();
      QEl y = FqN::one();
      for (int i = 64 * FqN::L - 1; i >= 0; i--) { y = FqN::sqr(y); if ((e.l[i / 64] >> (i % 64)) & 1) y = FqN::mul(y, rhs); }
      if (!FqN::eq(FqN::sqr(y), rhs)) continue;
      QEl t; const QEl yp = FqN::from_mont(y), half = FqN::from32(G::Fq::HALF);
      const bool is_larger = FqN::subb(t, half, yp) != 0;                                       // y > (p - 1) / 2  <=>  y > -y
      if (is_larger != greatest) y = FqN::neg(y);
      typename HG::Pt pt; pt.x = xm; pt.y = y; pt.zz = FqN::one(); pt.zzz = FqN::one();
      static const uint64_t COF_BLS[2] = {0x8c00aaab0000aaabULL, 0x396c8c005555e156ULL};
      typename HG::Pt acc = HG::identity();
      if (FQB == 48) { for (int i = 127; i >= 0; i--) { acc = HG::dbl(acc); if ((COF_BLS[i / 64] >> (i % 64)) & 1) acc = HG::add(acc, pt); } }
      else acc = pt;                                                                            // BN254: cofactor 1
      G1Aff a; memset(&a, 0, sizeof a); HG::to_affine_bytes(acc, a.xy); a.inf = false;
      g1_encode<G>(a, false, g1_urs);
      break;
    }
    // g2 = G2::rand on the twist: x = (c0, c1), the root by the (c1, c0) order, times the cofactor
    for (;;) {
      const QEl pq = FqN::P(); typename HP::F2 x; st.template field<FqN::L, G::Fq::BITS>(x.a.l, pq.l); st.template field<FqN::L, G::Fq::BITS>(x.b.l, pq.l);
      const bool greatest = st.boolean();
      typename HP::F2 y;
      if (!HP::f2_sqrt(HP::f2_add(HP::f2_mul(HP::f2_sqr(x), x), HP::twist_b()), &y)) continue;
      if (HP::f2_is_largest(y) != greatest) y = HP::f2_neg(y);
      typename HP::G2 q; q.x = x; q.y = y; q.inf = false;
      static const uint64_t COF2_BLS[8] = {0xcf1c38e31c7238e5ULL, 0x1616ec6e786f0c70ULL, 0x21537e293a6691aeULL, 0xa628f1cb4d9e82efULL,
                                           0xa68a205b2e5a7ddfULL, 0xcd91de4547085abaULL, 0x091d50792876a202ULL, 0x05d543a95414e7f1ULL};
      static const uint64_t COF2_BN[4] = {0x345f2299c0f9fa8dULL, 0x06ceecda572a2489ULL, 0xb85045b68181585eULL, 0x30644e72e131a029ULL};
      const uint64_t *cof = FQB == 48 ? COF2_BLS : COF2_BN; const int cbits = FQB == 48 ? 512 : 256;
      typename HP::G2 acc; acc.inf = true; acc.x = HP::f2_zero(); acc.y = HP::f2_zero();
      for (int i = cbits - 1; i >= 0; i--) { acc = HP::g2_dbl(acc); if ((cof[i / 64] >> (i % 64)) & 1) acc = HP::g2_add(acc, q); }
      HP::g2_encode(acc, g2_urs.data());
      break;
    }
    const size_t n_g1 = avrf_ring_pcs_domain_size(S::ID, ring_size);
    std::vector<uint8_t> srs(8 + n_g1 * 2 * FQB + 8 + 2 * 4 * FQB);
    size_t len = 0;
    if (int e = srs_generate(ctx, tau_le, g1_urs.data(), g2_urs.data(), n_g1, srs.data(), srs.size(), &len)) return e;
    return setup_load(ctx, srs.data(), len, ring_size, out);
  }

  // ---- Kzg::setup (reached from RingSetup::from_rand / from_seed, src/ring.rs:359-374) with the trapdoor and the two
  // generators given explicitly: writes `URS { powers_in_g1: tau^i g1 (i < n_g1), powers_in_g2: [g2, tau g2] }` in the
  // serialize_uncompressed layout that setup_load reads.  The n_g1 fixed-base multiplications are ONE batched table MSM.
  static int srs_generate(avrf_ctx *ctx, const uint8_t tau_le[32], const uint8_t *g1_urs, const uint8_t *g2_urs, size_t n_g1,
                          uint8_t *out, size_t out_cap, size_t *out_len) {
    const size_t e1 = 2 * FQB, e2 = 4 * FQB, need = 8 + n_g1 * e1 + 8 + 2 * e2;
    if (out_len) *out_len = need;
    if (!out || out_cap < need) return AVRF_ERR_BAD_ARG;
    H256 tau = Fr::load_le(tau_le);
    if (Fr::geq_p(tau) || !n_g1) return AVRF_INVALID_DATA;
    hipStream_t stream = avrf_ctx_stream_(ctx);
    HIP_CHECK(hipSetDevice(avrf_ctx_device_(ctx)));
    // g1: URS entry -> canonical little-endian x || y
    uint8_t le[2 * 48];
    if (FQB == 48) { if (g1_urs[0] & 0xC0) return AVRF_INVALID_DATA; for (int k = 0; k < FQB; k++) { le[k] = g1_urs[FQB - 1 - k]; le[FQB + k] = g1_urs[2 * FQB - 1 - k]; } }
    else { if (g1_urs[e1 - 1] & 0x40) return AVRF_INVALID_DATA; memcpy(le, g1_urs, e1); le[e1 - 1] &= 0x3f; }   // 0x80: arkworks' sign-of-y flag
    std::vector<H256> pw(n_g1);                                        // tau^i, plain
    { H256 tm = Fr::to_mont(tau), run = Fr::one(); for (size_t i = 0; i < n_g1; i++) { pw[i] = Fr::from_mont(run); run = Fr::mul(run, tm); } }
    const int c = 4, nwin = (G::Fr::BITS + 1 + c - 1) / c;
    std::vector<uint8_t> xy(n_g1 * e1);
    {
      MsmWorkspace ws;
      DevMem d_le(e1), d_flag(4), d_base(e1), d_table((size_t)nwin * e1), d_sc(n_g1 * 32); uint32_t flag = 0;
      HIP_CHECK(hipMemcpy(d_le.p, le, e1, hipMemcpyHostToDevice)); HIP_CHECK(hipMemsetAsync(d_flag.p, 0, 4, stream));   // (the flag reset in stream order with the kernel that sets it)
      HIP_CHECK(hipMemcpy(d_sc.p, pw.data(), n_g1 * 32, hipMemcpyHostToDevice));
      launch_g1_bases(pairing_curve_of(S::ID), d_le.as<uint8_t>(), 1, d_base.as(), d_flag.as(), stream);
      HIP_CHECK(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, stream)); HIP_CHECK(hipStreamSynchronize(stream));
      if (flag) return AVRF_INVALID_DATA;
      build_g1_table(pairing_curve_of(S::ID), d_base.as(), 1, c, nwin, d_table.as(), stream);
      msm_g1_fixed_device(pairing_curve_of(S::ID), d_table.as(), c, 1, d_sc.as(), 1, 1, ws, stream, xy.data(), n_g1);
    }
    uint64_t cnt = n_g1; memcpy(out, &cnt, 8);
    {
      std::vector<uint8_t> enc; enc.reserve(n_g1 * e1);
      for (size_t i = 0; i < n_g1; i++) g1_encode<G>(g1_from_xy(&xy[i * e1], FQB), false, enc);   // serialize_uncompressed (with arkworks' y flag on BN254)
      memcpy(out + 8, enc.data(), n_g1 * e1);
    }
    using HP = HostPairing<G>;
    typename HP::G2 g2; HP::g2_decode(g2_urs, &g2);
    typename HP::G2 tg2 = HP::g2_mul(g2, tau.l);
    uint8_t *o2 = out + 8 + n_g1 * e1; cnt = 2; memcpy(o2, &cnt, 8);
    memcpy(o2 + 8, g2_urs, e2); HP::g2_encode(tg2, o2 + 8 + e2);
    return AVRF_OK;
  }

  // ---- ring_proof::index (A.5): fixed columns and their commitments
  static int index(avrf_ring_setup *su, const uint8_t *pks_xy, size_t n_keys, std::unique_ptr<avrf_ring_key> &out) {
    if (n_keys > su->keyset) return AVRF_RING_CAPACITY_EXCEEDED;       // src/ring.rs:400-402
    const size_t N = su->N; RingLane &ln = su->lane[0];
    auto k = std::make_unique<avrf_ring_key>(); k->setup = su; k->n_keys = n_keys;
    H256 padx = Fr::from32(S::PAD_X), pady = Fr::from32(S::PAD_Y);
    for (size_t i = 0; i < n_keys; i++) {
      H256 x = Fr::load_le(pks_xy + 64 * i), y = Fr::load_le(pks_xy + 64 * i + 32);
      if (Fr::geq_p(x) || Fr::geq_p(y)) return AVRF_INVALID_DATA;
      k->points.push_back({Fr::to_mont(x), Fr::to_mont(y)});
    }
    for (size_t i = n_keys; i < su->keyset; i++) k->points.push_back({padx, pady});
    for (auto &p : su->h_pows) k->points.push_back(p);
    H256 zero = {{0, 0, 0, 0}};
    std::vector<H256> cols(3 * N, zero);
    for (size_t i = 0; i < k->points.size(); i++) { cols[i] = k->points[i].first; cols[N + i] = k->points[i].second; }
    for (size_t i = 0; i < su->keyset; i++) cols[2 * N + i] = Fr::one();
    k->px.assign(cols.begin(), cols.begin() + N); k->py.assign(cols.begin() + N, cols.begin() + 2 * N); k->sel.assign(cols.begin() + 2 * N, cols.end());
    ntt(su, ln, cols, N, 3, true);
    k->px_poly.assign(cols.begin(), cols.begin() + N); k->py_poly.assign(cols.begin() + N, cols.begin() + 2 * N); k->sel_poly.assign(cols.begin() + 2 * N, cols.end());
    commit_batch(su, ln, cols.data(), N, 3, k->C);
    k->d_fixed_coef.ensure(3 * N * 32); HIP_CHECK(hipMemcpy(k->d_fixed_coef.p, cols.data(), 3 * N * 32, hipMemcpyHostToDevice));
    // evaluations of the fixed columns on the 4N domain (shared by every proof over this ring)
    std::vector<H256> e4(3 * 4 * N, zero);
    for (size_t i = 0; i < N; i++) { e4[i] = k->px_poly[i]; e4[4 * N + i] = k->py_poly[i]; e4[8 * N + i] = k->sel_poly[i]; }
    ntt(su, ln, e4, 4 * N, 3, false);
    k->px4.assign(e4.begin(), e4.begin() + 4 * N); k->py4.assign(e4.begin() + 4 * N, e4.begin() + 8 * N); k->sel4.assign(e4.begin() + 8 * N, e4.end());
    k->d_fixed4.ensure(e4.size() * 32); HIP_CHECK(hipMemcpy(k->d_fixed4.p, e4.data(), e4.size() * 32, hipMemcpyHostToDevice));
    {  // the same points as te_pre for the device witness accumulation (k_ring_witness_acc)
      const size_t np = k->points.size();
      std::vector<H256> xy(2 * np);
      for (size_t i = 0; i < np; i++) { xy[2 * i] = k->points[i].first; xy[2 * i + 1] = k->points[i].second; }
      ln.buf.ensure(np * 64);
      k->d_points_pre.ensure(np * sizeof(te_pre));
      HIP_CHECK(hipMemcpyAsync(ln.buf.p, xy.data(), np * 64, hipMemcpyHostToDevice, ln.stream));
      hipLaunchKernelGGL(k_ring_points_pre<S>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ln.stream, (const uint32_t *)ln.buf.as(), (uint32_t)np, k->d_points_pre.as<te_pre>());
      HIP_CHECK(hipStreamSynchronize(ln.stream));
    }
    out = std::move(k);
    return AVRF_OK;
  }

  // ---- VerifierKeyBuilder (src/ring.rs:539-637): start from the all-padding ring, then every appended key replaces a
  // padding point: C_x += (x - x_pad) L_i(tau) G, C_y likewise -- two sparse MSMs over the Lagrange-basis table per append
  static G1Aff g1_add_aff(const G1Aff &a, const G1Aff &b) {
    using HG = typename T::HG;
    uint8_t xy[2 * FQB]; HG::to_affine_bytes(HG::add(g1_lift<G>(a), g1_lift<G>(b)), xy);
    return g1_from_xy(xy, FQB);
  }
  static int builder_new(avrf_ring_setup *su, avrf_ring_vk_builder **out) {
    std::unique_ptr<avrf_ring_key> k;
    if (int st = index(su, nullptr, 0, k)) return st;                  // the ring of padding points only
    auto b = std::make_unique<avrf_ring_vk_builder>(); b->setup = su;
    for (int i = 0; i < 3; i++) b->C[i] = k->C[i];
    ensure_lagrange(su);
    *out = b.release();
    return AVRF_OK;
  }
  static int builder_append(avrf_ring_vk_builder *b, const uint8_t *pks_xy, size_t n) {
    avrf_ring_setup *su = b->setup; RingLane &ln = su->lane[0];
    if (n > su->keyset - b->curr) return AVRF_RING_CAPACITY_EXCEEDED;   // src/ring.rs:606-608; nothing appended
    if (!n) return AVRF_OK;
    const H256 padx = Fr::from32(S::PAD_X), pady = Fr::from32(S::PAD_Y);
    std::vector<H256> sc(2 * n); std::vector<uint32_t> bi(2 * n);
    for (size_t i = 0; i < n; i++) {
      H256 x = Fr::load_le(pks_xy + 64 * i), y = Fr::load_le(pks_xy + 64 * i + 32);
      if (Fr::geq_p(x) || Fr::geq_p(y)) return AVRF_INVALID_DATA;
      sc[i] = Fr::from_mont(Fr::sub(Fr::to_mont(x), padx)); sc[n + i] = Fr::from_mont(Fr::sub(Fr::to_mont(y), pady));
      bi[i] = bi[n + i] = (uint32_t)(b->curr + i);
    }
    uint32_t *d_sc, *d_bi;
    ln.carve().take(d_sc, 2 * n * 8).take(d_bi, 2 * n).into(1);
    HIP_CHECK(hipMemcpyAsync(d_sc, sc.data(), 2 * n * 32, hipMemcpyHostToDevice, ln.stream));
    HIP_CHECK(hipMemcpyAsync(d_bi, bi.data(), 2 * n * 4, hipMemcpyHostToDevice, ln.stream));
    std::vector<G1Aff> D; commit_sparse(su, ln, d_sc, d_bi, n, 2, D);
    b->C[0] = g1_add_aff(b->C[0], D[0]); b->C[1] = g1_add_aff(b->C[1], D[1]);
    b->curr += n;
    return AVRF_OK;
  }

  // ---- RingProver::prove with blinding disabled (A.7) for a batch of proofs over one ring, in lockstep:
  // every device stage (iNTT, KZG commits, NTT(4N) + constraint aggregation + iNTT(4N), openings) runs ONCE for
  // the whole chunk -- batched NTTs and one batched MSM launch chain over the shared SRS per round of the
  // Fiat-Shamir transcript -- while the O(N) per-proof bookkeeping runs on the host between the rounds.
  // out: per proof 4*G1 || 7*Fr || G1 || Fr || G1 || G1.
  struct ProofState {
    H256 seedx, seedy, resx, resy, instx, insty, al[7], zeta, ev[7], lin_zw, nu[8];
    G1Aff C[4], Cq, pi[2];
    ArkTranscript t;
  };
  // batched commit of `batch` coefficient vectors on the device in Montgomery form: vector b starts at
  // d_coeffs_mont + b * stride elements, its first n coefficients are committed (the source is left untouched)
  static void commit_device(avrf_ring_setup *su, RingLane &ln, const uint32_t *d_coeffs_mont, size_t stride, size_t n, size_t batch, std::vector<G1Aff> &out) {
    // (the digit kernel of the MSM takes the Montgomery limbs as they are: no plain copy of the coefficient vectors)
    constexpr int mont_id = std::is_same<F, FqBandersnatch>::value ? 1 : 2;
    static_assert(std::is_same<F, FqBandersnatch>::value || std::is_same<F, FqBabyJubJub>::value, "scalar field of the KZG commitments");
    std::vector<uint8_t> xy(batch * 2 * FQB);
    RingTrace trace("commit", batch, false);
    if (trace.on()) { HIP_CHECK(hipStreamSynchronize(ln.stream)); trace.restart(); }
    // many vectors at once and the table of all multiples is there: one gathered point per (coefficient, row), no buckets (msm.hip)
    if (su->direct && batch >= 32) { msm_g1_direct_device(su->direct->t, d_coeffs_mont, n, stride, ln.ws, ln.stream, xy.data(), batch, mont_id); ++su->table_batches; }
    else msm_g1_fixed_device(su->curve, su->d_srs_table.as(), su->table_c, su->n_srs, d_coeffs_mont, n, stride, ln.ws, ln.stream, xy.data(), batch, nullptr, mont_id);
    if (trace.on()) fprintf(stderr, "    commit n=%zu batch=%zu: %.3f ms wall, accumulate %.3f ms (c=%d seg=%d)\n", n, batch,
                            trace.wall_ms(), ln.ws.accum_ms_last, ln.ws.last_plan.c, ln.ws.last_plan.lpb);
    out.resize(batch); g1_from_xy_batch(xy, batch, out.data());
  }
  // Lagrange-basis SRS for the witness columns, built on first use: L_i(tau) G = commit(iNTT(e_i)) (N commits in one
  // batched MSM), then the prefix sums PS_k on the host and a window table over [L_0 .. L_{N-1} | PS_0 .. PS_N].
  // (lane 0, and never with a chunk in flight: the chunks read what this writes)
  static void ensure_lagrange(avrf_ring_setup *su) {
    if (su->d_wit_table) return;
    const size_t N = su->N, nb = 2 * N + 1; RingLane &ln = su->lane[0];
    // in tiles of 256 unit vectors: scratch is O(256 N) instead of the N x N matrix (2 GiB at N = 8192, 137 GB at 2^16)
    const size_t TILE = N < 256 ? N : 256;
    uint32_t *d_mat = ln.scratch(0, TILE * N * 32);
    std::vector<G1Aff> lag; lag.reserve(N);
    for (size_t i0 = 0; i0 < N; i0 += TILE) {
      const size_t rows = N - i0 < TILE ? N - i0 : TILE;
      HIP_CHECK(hipMemsetAsync(d_mat, 0, rows * N * 32, ln.stream));
      hipLaunchKernelGGL(k_set_diag<F>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ln.stream, d_mat, (uint32_t)N, (uint32_t)rows, (uint32_t)i0);
      { fp sc; memcpy(sc.v, su->ninv.l, 32); ntt_launch<F>(d_mat, (uint32_t)N, su->d_tw_n_inv.as(), (uint32_t)rows, &sc, ln.stream); }
      std::vector<G1Aff> part; commit_device(su, ln, d_mat, N, N, rows, part);
      lag.insert(lag.end(), part.begin(), part.end());
    }
    su->lag_raw.clear();
    for (size_t i = 0; i < N; i++) g1_encode<G>(lag[i], false, su->lag_raw);
    using HG = typename T::HG;
    std::vector<typename HG::Pt> ps(N + 1);
    ps[0] = HG::identity();
    for (size_t i = 0; i < N; i++) ps[i + 1] = HG::add(ps[i], g1_lift<G>(lag[i]));
    std::vector<uint8_t> le(nb * 2 * FQB);
    for (size_t i = 0; i < N; i++) memcpy(&le[i * 2 * FQB], lag[i].xy, 2 * FQB);
    HG::to_affine_bytes_batch(ps.data(), N + 1, &le[N * 2 * FQB]);
    DevMem d_le(le.size()), d_flag(4), d_bases(nb * 2 * FQB);
    HIP_CHECK(hipMemcpy(d_le.p, le.data(), le.size(), hipMemcpyHostToDevice)); HIP_CHECK(hipMemsetAsync(d_flag.p, 0, 4, ln.stream));
    launch_g1_bases(su->curve, d_le.as<uint8_t>(), nb, d_bases.as(), d_flag.as(), ln.stream);
    su->wit_c = 7;
    if (const char *e = getenv("AVRF_RING_WIT_C")) { int v = atoi(e); if (v >= 4 && v <= 14) su->wit_c = v; }
    su->wit_nwin = (G::Fr::BITS + 1 + su->wit_c - 1) / su->wit_c;
    DevMem d_table((size_t)su->wit_nwin * nb * 2 * FQB);
    build_g1_table(su->curve, d_bases.as(), nb, su->wit_c, su->wit_nwin, d_table.as(), ln.stream);
    HIP_CHECK(hipStreamSynchronize(ln.stream));
    su->d_wit_bases = std::move(d_bases); su->d_wit_table = std::move(d_table);   // (only a finished table is seen)
  }
  // `batch` sparse commits over the witness table: vector b = m (base index, plain scalar) pairs
  static void commit_sparse(avrf_ring_setup *su, RingLane &ln, const uint32_t *d_scalars_plain, const uint32_t *d_base_idx, size_t m, size_t batch, std::vector<G1Aff> &out) {
    std::vector<uint8_t> xy(batch * 2 * FQB);
    if (su->direct_wit && batch >= 32) { msm_g1_direct_device(su->direct_wit->t, d_scalars_plain, m, m, ln.ws, ln.stream, xy.data(), batch, 0, d_base_idx); ++su->table_batches; }
    else msm_g1_fixed_device(su->curve, su->d_wit_table.as(), su->wit_c, 2 * su->N + 1, d_scalars_plain, m, m, ln.ws, ln.stream, xy.data(), batch, d_base_idx);
    out.resize(batch); g1_from_xy_batch(xy, batch, out.data());
  }

  // (the witness table is there: avrf_ring_prove builds it before the first chunk -- two chunks run this at once)
  static int prove_chunk(avrf_ring_key *k, RingLane &ln, size_t n, const uint32_t *key_index, const uint8_t *blindings, bool hiding, uint8_t *out) {
    avrf_ring_setup *su = k->setup;
    const size_t N = su->N, cap = su->cap, M = 4 * N;
    const H256 one = Fr::one();
    RingTrace lap("ring_prove", n, true);                              // (wall time and the PROCESS's CPU time of every phase, workers included)
    std::vector<ProofState> st(n);
    const H256 w_last = fr_pow<F>(su->w, cap - 1);
    // ---- round 0: the witness in sparse form (A.7 step 1).  Rows with bit 1: the signer's key and the set bits
    // of the blinding; the accumulator column only changes there, so it is cnt+1 points; the four KZG commits are
    // sparse MSMs over the Lagrange-basis SRS and its prefix sums (same group elements as the coefficient-form commits).
    constexpr size_t MP = 264;                                         // padded entries per sparse vector (L + 2 + 3 zk rows <= 264)
    // hiding (RingContext with blinding, src/ring.rs:277-295): the last 3 rows of every witness column are uniformly
    // random field elements (w3f-ring-proof `private_column`); they only add 3 sparse terms to each commitment
    std::vector<H256> zk;
    if (hiding) {
      std::vector<uint8_t> rnd(n * 12 * 48);
      for (size_t o = 0; o < rnd.size();) { ssize_t g = getrandom(&rnd[o], rnd.size() - o, 0); if (g <= 0) return AVRF_ERR_BAD_ARG; o += (size_t)g; }
      zk.resize(n * 12);
      for (size_t i = 0; i < n * 12; i++) zk[i] = fr_from_be48<F>(&rnd[i * 48]);
    }
    // ---- round 0 + 1 (device): witness accumulation (k_ring_witness_acc), columns, coefficients, their 4N evaluations, 4n sparse
    // commits in one MSM chain.  Back to the host: result and instance of every proof (for the transcript and the constraints).
    uint32_t *d_coef = ln.scratch(2, n * 4 * N * 32), *d_e4 = ln.scratch(0, std::max(n * 4 * M * 32, n * 257 * 128));
    std::vector<H256> wout(n * 4);
    {
      const size_t b_cnt = n * 4, b_sc = n * 4 * MP * 32, b_bi = n * 4 * MP * 4, b_zk = n * 12 * 32, b_bl = n * 32, b_out = n * 128;
      uint32_t *d_sc, *d_val, *d_zk, *d_pos, *d_bi, *d_cnt, *d_ki, *d_bl, *d_out;
      ln.carve().take(d_sc, b_sc / 4).take(d_val, n * 257 * 16).take(d_zk, b_zk / 4).take(d_pos, n * 256).take(d_bi, b_bi / 4).take(d_cnt, n).take(d_ki, n)
          .take(d_bl, b_bl / 4).take(d_out, b_out / 4).into(1);
      if (hiding) HIP_CHECK(hipMemcpyAsync(d_zk, zk.data(), b_zk, hipMemcpyHostToDevice, ln.stream));
      HIP_CHECK(hipMemcpyAsync(d_ki, key_index, b_cnt, hipMemcpyHostToDevice, ln.stream));
      HIP_CHECK(hipMemcpyAsync(d_bl, blindings, b_bl, hipMemcpyHostToDevice, ln.stream));
      HIP_CHECK(hipMemsetAsync(d_sc, 0, b_sc, ln.stream));
      HIP_CHECK(hipMemsetAsync(d_bi, 0, b_bi, ln.stream));
      fp sx, sy; { const H256 ax = Fr::from32(S::ACC_X), ay = Fr::from32(S::ACC_Y); memcpy(sx.v, ax.l, 32); memcpy(sy.v, ay.l, 32); }
      hipLaunchKernelGGL(k_ring_witness_acc<S>, dim3((unsigned)((4 * n + 63) / 64)), dim3(64), 0, ln.stream, k->d_points_pre.as<const te_pre>(), (const uint32_t *)d_ki,
                         (const uint8_t *)d_bl, (uint32_t)n, (uint32_t)su->keyset, (uint32_t)su->L, (uint32_t)N, (uint32_t)cap, sx, sy,
                         hiding ? (const uint32_t *)d_zk : nullptr, d_e4, d_pos, d_cnt, d_val, d_sc, d_bi, d_out);
      HIP_CHECK(hipMemcpyAsync(wout.data(), d_out, b_out, hipMemcpyDeviceToHost, ln.stream));
      hipLaunchKernelGGL(k_ring_witness_cols<F>, dim3((unsigned)((N + 255) / 256), (unsigned)n), dim3(256), 0, ln.stream, (const uint32_t *)d_pos,
                         (const uint32_t *)d_cnt, (const uint32_t *)d_ki, (const uint32_t *)d_val, hiding ? (const uint32_t *)d_zk : nullptr, (uint32_t)N, (uint32_t)cap, d_coef);
      { fp sc; memcpy(sc.v, su->ninv.l, 32); ntt_launch<F>(d_coef, (uint32_t)N, su->d_tw_n_inv.as(), (uint32_t)(4 * n), &sc, ln.stream); }
      ntt_launch2<F>(d_coef, (uint32_t)N, d_e4, (uint32_t)M, su->d_tw_4n.as(), (uint32_t)(4 * n), nullptr, ln.stream);   // zero-extended to 4N
      std::vector<G1Aff> C; commit_sparse(su, ln, d_sc, d_bi, MP, 4 * n, C);                                         // (waits for the stream)
      const H256 ax = Fr::from32(S::ACC_X), ay = Fr::from32(S::ACC_Y);
      for (size_t p = 0; p < n; p++) {
        for (int i = 0; i < 4; i++) st[p].C[i] = C[4 * p + i];
        st[p].seedx = ax; st[p].seedy = ay; st[p].resx = wout[4 * p]; st[p].resy = wout[4 * p + 1]; st[p].instx = wout[4 * p + 2]; st[p].insty = wout[4 * p + 3];
      }
    }
    lap("intt + ntt4n + 4n commits");
    const ArkTranscript t0 = HR::prelude(su->g1_0, su->g2_raw, k->C);   // shared by every proof over this ring
    parallel_for(n, [&](size_t p) {
      ProofState &ps = st[p];
      ps.t = t0;
      uint8_t inst[64]; fr_store_le32<F>(inst, ps.instx); fr_store_le32<F>(inst + 32, ps.insty);
      HR::alphas(ps.t, inst, ps.C, ps.al);
    }, 64);                                                            // (3 us per proof on one thread: a worker is worth waking for ~200 us)
    lap("transcript: alphas");
    // per-chunk parameter block on the device: RingConsts[n] | zeta[n] | nu[8n] | ev[7n] | lin_zw[n]
    const size_t qlen = 3 * N + 1, olen = 3 * N;
    RingConsts *d_rc; uint32_t *d_zeta, *d_nu, *d_ev;
    ln.carve().take(d_rc, n).take(d_zeta, n * 8).take(d_nu, n * 64).take(d_ev, n * 64).into(3);   // (ev and lin_zw one field: they come back in one copy)
    uint32_t *d_linzw = d_ev + n * 56;
    // ---- round 2 (device): constraint aggregation on the 4N domain, iNTT(4N), * Z_zk / (X^N - 1), n quotient commits
    uint32_t *d_agg = ln.scratch(1, n * M * 32), *d_q = ln.scratch(4, n * qlen * 32);
    {
      std::vector<RingConsts> rc(n);
      auto setfp = [](fp &d, const H256 &v) { memcpy(d.v, v.l, 32); };
      for (size_t p = 0; p < n; p++) {
        for (int i = 0; i < 7; i++) setfp(rc[p].alpha[i], st[p].al[i]);
        setfp(rc[p].w_last, w_last); setfp(rc[p].seedx, st[p].seedx); setfp(rc[p].seedy, st[p].seedy); setfp(rc[p].resx, st[p].resx); setfp(rc[p].resy, st[p].resy);
      }
      HIP_CHECK(hipMemcpyAsync(d_rc, rc.data(), n * sizeof(RingConsts), hipMemcpyHostToDevice, ln.stream));
      hipLaunchKernelGGL(k_ring_constraints<S>, dim3((M + 255) / 256, (unsigned)n), dim3(256), 0, ln.stream, d_e4, k->d_fixed4.as(), su->d_l4.as(), su->d_tw_4n.as(),
                         (const RingConsts *)d_rc, (uint32_t)M, d_agg);
      fp sc; memcpy(sc.v, su->n4inv.l, 32);
      ntt_launch<F>(d_agg, (uint32_t)M, su->d_tw_4n_inv.as(), (uint32_t)n, &sc, ln.stream);
      Fp3 z;                                                           // Z(X) = prod_j (X - w^(N-3+j)) = X^3 + z2 X^2 + z1 X + z0
      { H256 r0 = fr_pow<F>(su->w, N - 3), r1 = Fr::mul(r0, su->w), r2 = Fr::mul(r1, su->w);
        H256 z2 = Fr::neg(Fr::add(Fr::add(r0, r1), r2)), z1 = Fr::add(Fr::add(Fr::mul(r0, r1), Fr::mul(r0, r2)), Fr::mul(r1, r2)), z0 = Fr::neg(Fr::mul(Fr::mul(r0, r1), r2));
        setfp(z.v[0], z0); setfp(z.v[1], z1); setfp(z.v[2], z2); }
      hipLaunchKernelGGL(k_ring_quotient<F>, dim3((unsigned)((qlen + 255) / 256), (unsigned)n), dim3(256), 0, ln.stream, (const uint32_t *)d_agg, (uint32_t)N,
                         (uint32_t)qlen, z, d_q);
      lap("constraints + quotient (launch)");
      std::vector<G1Aff> C; commit_device(su, ln, d_q, qlen, qlen, n, C);
      for (size_t p = 0; p < n; p++) st[p].Cq = C[p];
    }
    lap("n quotient commits");
    // ---- round 3: evaluation point (host transcript), evaluations + linearisation (device)
    std::vector<H256> zs(n);
    {
      parallel_for(n, [&](size_t p) {
        ProofState &ps = st[p];
        ps.zeta = HR::zeta(ps.t, ps.Cq); zs[p] = ps.zeta;
      }, 256);
      HIP_CHECK(hipMemcpyAsync(d_zeta, zs.data(), n * 32, hipMemcpyHostToDevice, ln.stream));
    }
    uint32_t *d_lin = ln.scratch(5, n * N * 32);
    fp w_dev; memcpy(w_dev.v, su->w.l, 32);
    hipLaunchKernelGGL(k_ring_evals<F>, dim3(7, (unsigned)n), dim3(256), 0, ln.stream, (const uint32_t *)d_coef, (const uint32_t *)k->d_fixed_coef.as(),
                       (const uint32_t *)d_zeta, (uint32_t)N, d_ev);
    hipLaunchKernelGGL(k_ring_lin<S>, dim3((unsigned)n), dim3(256), 0, ln.stream, (const uint32_t *)d_coef, (const RingConsts *)d_rc, (const uint32_t *)d_zeta,
                       (const uint32_t *)d_ev, w_dev, (uint32_t)N, d_lin, d_linzw);
    {
      std::vector<H256> evh(n * 8);                                    // ev[7n] | lin_zw[n] are contiguous on the device
      HIP_CHECK(hipMemcpyAsync(evh.data(), d_ev, n * 8 * 32, hipMemcpyDeviceToHost, ln.stream));
      HIP_CHECK(hipStreamSynchronize(ln.stream));
      std::vector<H256> nus(n * 8);
      parallel_for(n, [&](size_t p) {
        ProofState &ps = st[p];
        for (int i = 0; i < 7; i++) ps.ev[i] = evh[p * 7 + i];
        ps.lin_zw = evh[n * 7 + p];
        uint8_t evb[8 * 32]; for (int i = 0; i < 7; i++) fr_store_le32<F>(evb + 32 * i, ps.ev[i]);
        fr_store_le32<F>(evb + 7 * 32, ps.lin_zw);
        HR::nus(ps.t, evb, evb + 7 * 32, ps.nu);
        for (int i = 0; i < 8; i++) nus[p * 8 + i] = ps.nu[i];
      }, 64);
      HIP_CHECK(hipMemcpyAsync(d_nu, nus.data(), n * 8 * 32, hipMemcpyHostToDevice, ln.stream));
      HIP_CHECK(hipStreamSynchronize(ln.stream));                     // nus goes out of scope
    }
    lap("evals + linearisation");
    // ---- round 4 (device): aggregated opening at zeta, opening of lin at zeta*w, 2n opening commits
    {
      uint32_t *d_aggz = d_agg;                                        // the 4N aggregate is dead: reuse (qlen <= 4N)
      uint32_t *d_open = ln.scratch(0, n * 4 * M * 32);           // = d_e4 (dead): q1 (n x olen) | q2 (n x N)
      uint32_t *d_q1 = d_open, *d_q2 = d_open + n * olen * 8;
      hipLaunchKernelGGL(k_ring_aggz<F>, dim3((unsigned)((qlen + 255) / 256), (unsigned)n), dim3(256), 0, ln.stream, (const uint32_t *)d_coef,
                         (const uint32_t *)k->d_fixed_coef.as(), (const uint32_t *)d_q, (const uint32_t *)d_nu, (uint32_t)N, (uint32_t)qlen, d_aggz);
      fp one_m; memcpy(one_m.v, one.l, 32);
      hipLaunchKernelGGL(k_ring_divlin<F>, dim3((unsigned)n), dim3(256), 0, ln.stream, (const uint32_t *)d_aggz, (uint32_t)qlen, (uint32_t)qlen,
                         (const uint32_t *)d_zeta, one_m, d_q1, (uint32_t)olen);
      // small chunks: BOTH openings in one MSM chain (2n vectors of stride 3N, the short one zero-padded: zero digits are dropped
      // by the sort) -- a chain of 32-128 proofs is latency-bound (k_wsum_blk: ~50 sequential G1 additions per bucket set, 0.85 ms
      // whatever the number of sets), so the second chain cost as much as the first; large chunks keep two exact-length chains
      const bool merged = n <= 128;
      const size_t q2_stride = merged ? olen : N;
      if (merged) HIP_CHECK(hipMemsetAsync(d_q2, 0, n * olen * 32, ln.stream));
      hipLaunchKernelGGL(k_ring_divlin<F>, dim3((unsigned)n), dim3(256), 0, ln.stream, (const uint32_t *)d_lin, (uint32_t)N, (uint32_t)N,
                         (const uint32_t *)d_zeta, w_dev, d_q2, (uint32_t)q2_stride);
      std::vector<G1Aff> C1, C2;
      if (merged) {
        commit_device(su, ln, d_q1, olen, olen, 2 * n, C1);
        for (size_t p = 0; p < n; p++) { st[p].pi[0] = C1[p]; st[p].pi[1] = C1[n + p]; }
      } else {
        commit_device(su, ln, d_q1, olen, olen, n, C1);
        commit_device(su, ln, d_q2, N, N - 1, n, C2);
        for (size_t p = 0; p < n; p++) { st[p].pi[0] = C1[p]; st[p].pi[1] = C2[p]; }
      }
    }
    lap("2n opening commits");
    for (size_t p = 0; p < n; p++) {
      const ProofState &ps = st[p];
      const G1Aff *const pts[7] = {&ps.C[0], &ps.C[1], &ps.C[2], &ps.C[3], &ps.Cq, &ps.pi[0], &ps.pi[1]};
      HR::proof_serialize(pts, ps.ev, ps.lin_zw, out + PL::LEN * p);
    }
    lap("proof bytes");
    return AVRF_OK;
  }

  using FqN = typename T::FqN; using QEl = typename FqN::El;

  // the verifier's two sums over one launch chain: vector 0 = scalars_a over bases_a, vector 1 = scalars_b over bases_b, as two
  // scalar vectors over the concatenated bases (a zero scalar has no digits and costs nothing downstream).  One chain instead
  // of two is 0.25 ms of launch latency less per verification call, and the host's two bit-sum Horners run side by side.
  static void g1_msm2(avrf_ring_setup *su, RingLane &ln, const std::vector<uint8_t> &bases_a, const std::vector<H256> &scalars_a,
                      const std::vector<uint8_t> &bases_b, const std::vector<H256> &scalars_b, bool check_subgroup_a, bool *bad_points,
                      G1Aff *out_a, G1Aff *out_b) {
    const size_t na = scalars_a.size(), nbv = scalars_b.size(), n = na + nbv;
    uint8_t *d_xy; uint32_t *d_b, *d_s, *d_flag;
    ln.carve().take(d_xy, n * 2 * FQB).take(d_b, n * 2 * FQB / 4).take(d_s, 2 * n * 8).take(d_flag, 1).into(1);
    HIP_CHECK(hipMemcpyAsync(d_xy, bases_a.data(), na * 2 * FQB, hipMemcpyHostToDevice, ln.stream));
    HIP_CHECK(hipMemcpyAsync(d_xy + na * 2 * FQB, bases_b.data(), nbv * 2 * FQB, hipMemcpyHostToDevice, ln.stream));
    HIP_CHECK(hipMemsetAsync(d_s, 0, 2 * n * 32, ln.stream));
    HIP_CHECK(hipMemcpyAsync(d_s, scalars_a.data(), na * 32, hipMemcpyHostToDevice, ln.stream));
    HIP_CHECK(hipMemcpyAsync(d_s + (n + na) * 8, scalars_b.data(), nbv * 32, hipMemcpyHostToDevice, ln.stream));
    HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, ln.stream));
    launch_g1_bases(su->curve, d_xy, n, d_b, d_flag, ln.stream);
    if (check_subgroup_a) launch_g1_subgroup_check(su->curve, d_b, na, d_flag, ln.stream);   // Validate::Yes of the deserialised points
    uint8_t xy[2][2 * FQB];
    msm_g1_device(su->curve, d_b, d_s, n, ln.ws, ln.stream, &xy[0][0], 2, n);            // (synchronises the stream)
    if (bad_points) { uint32_t f = 0; HIP_CHECK(hipMemcpy(&f, d_flag, 4, hipMemcpyDeviceToHost)); *bad_points = f != 0; }
    *out_a = g1_from_xy(xy[0], FQB); *out_b = g1_from_xy(xy[1], FQB);
  }

  // ---- CanonicalSerialize of the setup objects (src/ring.rs:484-542): RingSetup = its PcsParams (URS { powers_in_g1,
  // powers_in_g2 }), RingBuilderPcsParams = Vec<G1Affine> (the SRS in Lagrangian form); both in either ark-serialize mode
  static void put_points(const std::vector<uint8_t> &raw, size_t n, bool compress, std::vector<uint8_t> &o) {
    { uint64_t v = n; size_t at = o.size(); o.resize(at + 8); memcpy(&o[at], &v, 8); }
    if (!compress) { o.insert(o.end(), raw.begin(), raw.begin() + n * 2 * FQB); return; }
    for (size_t i = 0; i < n; i++) g1_encode<G>(g1_from_raw<G>(&raw[i * 2 * FQB]), true, o);
  }
  static int setup_serialize(avrf_ring_setup *su, bool compress, std::vector<uint8_t> &o) {
    using HP = HostPairing<G>;
    put_points(su->g1_raw, su->n_srs, compress, o);
    { uint64_t v = 2; size_t at = o.size(); o.resize(at + 8); memcpy(&o[at], &v, 8); }
    if (!compress) { o.insert(o.end(), su->g2_raw.begin(), su->g2_raw.end()); return AVRF_OK; }
    for (int i = 0; i < 2; i++) {
      typename HP::G2 q; HP::g2_decode(su->g2_raw.data() + (size_t)i * 4 * FQB, &q);
      size_t at = o.size(); o.resize(at + 2 * FQB); HP::g2_encode_compressed(q, &o[at]);
    }
    return AVRF_OK;
  }
  static int builder_params_serialize(avrf_ring_setup *su, bool compress, std::vector<uint8_t> &o) {
    ensure_lagrange(su);
    put_points(su->lag_raw, su->N, compress, o);
    return AVRF_OK;
  }

  // ---- n independent KZG pairing checks on the device: ok[i] = [ e(A_i, g2) * e(B_i, tau g2) == 1 ]   (pairing.hip)
  static void ensure_pairing(avrf_ring_setup *su) {
    if (su->ptab_ready) return;
    su->ptab.build(su->curve, su->g2_raw.data(), 2, su->lane[0].stream);
    su->ptab_ready = true;
  }
  // the Miller-loop lines of the setup's two fixed G2 arguments, tabulated once for the host pairing (host_pairing.h G2Lines)
  using HP = HostPairing<G>;
  static const typename HP::G2Lines *host_lines(avrf_ring_setup *su) {
    static std::mutex lines_mu;
    std::lock_guard<std::mutex> lk(lines_mu);
    if (!su->host_lines) {
      typename HP::G2 q[2];
      const size_t g2len = su->g2_raw.size() / 2;
      HP::g2_decode(su->g2_raw.data(), &q[0]); HP::g2_decode(su->g2_raw.data() + g2len, &q[1]);
      std::unique_ptr<typename HP::G2Lines[]> t(new typename HP::G2Lines[2]);
      t[0] = HP::g2_lines(q[0]); t[1] = HP::g2_lines(q[1]);
      // (published only when both tables are complete: a throw above leaves host_lines null and the next call builds again)
      su->host_lines = std::unique_ptr<void, void (*)(void *)>(t.release(), [](void *p) { delete[] static_cast<typename HP::G2Lines *>(p); });
    }
    return static_cast<const typename HP::G2Lines *>(su->host_lines.get());
  }
  // Few independent checks: ONE wave of the device pairing kernel needs 11.7 ms whatever it carries, a host core 1.0 ms per check
  // (line tables), so up to two checks per pool thread (at most 16) are finished on the host pool from the device's G1 sums.
  static bool few_checks(size_t n) { size_t t = HostPool::get().size(); if (t > 8) t = 8; return n <= 2 * t; }
  // pts: n x {A, B} Montgomery affine points as launch_g1_bases / launch_g1_lincomb write them ((0, 0) = infinity)
  static void host_pair_checks(avrf_ring_setup *su, const uint32_t *pts, size_t n, int32_t *ok) {
    const typename HP::G2Lines *lines = host_lines(su);
    constexpr size_t FW = FQB / 4;
    parallel_for(n, [&](size_t it) {
      QEl px[2], py[2]; bool pinf[2];
      for (int i = 0; i < 2; i++) {
        const uint32_t *w = pts + (2 * it + i) * 2 * FW;
        g1_coords<G>((const uint8_t *)w, &px[i], &py[i]);
        bool z = true; for (size_t k = 0; k < 2 * FW; k++) z = z && w[k] == 0;
        pinf[i] = z;
      }
      ok[it] = HP::product_is_one_lines(px, py, pinf, lines, 2) ? 1 : 0;
    });
  }
  static int pairing_check(avrf_ring_setup *su, size_t n, const uint8_t *a_xy, const uint8_t *b_xy, int32_t *ok_out) {
    if (!n) return AVRF_OK;
    const size_t e1 = 2 * FQB; RingLane &ln = su->lane[0];
    std::vector<uint8_t> le(2 * n * e1);
    for (size_t i = 0; i < n; i++) { memcpy(&le[(2 * i) * e1], a_xy + i * e1, e1); memcpy(&le[(2 * i + 1) * e1], b_xy + i * e1, e1); }
    uint8_t *d_le; uint32_t *d_pts, *d_flag; int32_t *d_ok;
    ln.carve().take(d_le, 2 * n * e1).take(d_pts, 2 * n * e1 / 4).take(d_ok, n).take(d_flag, 1).into(1);
    HIP_CHECK(hipMemcpyAsync(d_le, le.data(), 2 * n * e1, hipMemcpyHostToDevice, ln.stream));
    HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, ln.stream));
    launch_g1_bases(su->curve, d_le, 2 * n, d_pts, d_flag, ln.stream);
    uint32_t flag = 0;
    if (few_checks(n)) {
      std::vector<uint32_t> pts(2 * n * e1 / 4);
      HIP_CHECK(hipMemcpyAsync(pts.data(), d_pts, 2 * n * e1, hipMemcpyDeviceToHost, ln.stream));
      HIP_CHECK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ln.stream));
      HIP_CHECK(hipStreamSynchronize(ln.stream)); HIP_CHECK(hipGetLastError());
      if (flag) return AVRF_INVALID_DATA;
      host_pair_checks(su, pts.data(), n, ok_out);
      return AVRF_OK;
    }
    ensure_pairing(su);
    launch_pairing_check(su->ptab, d_pts, n, d_ok, ln.stream);
    HIP_CHECK(hipMemcpyAsync(ok_out, d_ok, n * 4, hipMemcpyDeviceToHost, ln.stream));
    HIP_CHECK(hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, ln.stream));
    HIP_CHECK(hipStreamSynchronize(ln.stream)); HIP_CHECK(hipGetLastError());
    return flag ? AVRF_INVALID_DATA : AVRF_OK;
  }

  // ---- RingVerifier::verify / multi-ring batch verifier (src/ring.rs:242,693-735).
  // Every item's two KZG openings are folded with 128-bit randomisers into
  //   e(sum r (C - v g1 + z pi), g2) * e(-sum r pi, tau g2) == 1 :
  // two G1 MSMs on the GPU (10 n + 1 and 2 n terms) and one 2-pairing check on the host.
  // each_status != nullptr: the n items are verified INDEPENDENTLY (n x RingVerifier::verify): per-item status, one 2-pairing
  // check per item on the device (k_g1_lincomb + pairing.hip) instead of one randomised check for the whole batch.
  // The call is a sequence of stages over one record (verify_batch, below, is the sequence); the arithmetic of an item is HR::reduce.
  static constexpr size_t DEVICE_DECOMPRESS_MIN = 128;   // items; below, the pool's cores finish sooner than a device round trip
  struct VerifyRun {
    avrf_ring_setup *su; RingLane &ln; size_t n, n_rings;
    const uint8_t *commitments; const uint32_t *ring_of_item; const uint8_t *instances_xy, *proofs; int32_t *each_status;
    RingTrace lap;
    bool host_subgroup;                                // Validate::Yes (subgroup) of the deserialised G1 points: on the host pool for small batches, on the device otherwise
    std::vector<G1Aff> fixed;                          // verify_commitments: the three commitments of every ring
    std::vector<uint8_t> rnd;                          // HR::batch_randomisers: 32 bytes per item
    std::vector<G1Aff> dec; std::vector<uint8_t> dec_ok;   // verify_points: the 7 G1 points of every proof (RingProofLayout order) | 0: did not decode
    std::vector<ArkTranscript> t_ring;                 // verify_transcripts: per ring
    // verify_reduce.  per item: 10 terms of the first MSM (3 fixed + 4 witness + C_q + pi1 + pi2) and 2 of the second
    std::vector<uint8_t> b1, b2; std::vector<H256> s1, s2, gsc;
    std::vector<int32_t> item_st;                      // (each_status, segments) what the host part found wrong with an item
    // verify_segments: segment v is the items [seg_off[v], seg_off[v + 1]); empty for the two unsegmented sequences
    std::vector<uint32_t> seg_off;
    std::vector<uint8_t> lone;                         // (segments) the item is the only one of its segment: r1 = 1, the rule of a batch of one
    bool per_item() const { return each_status || !seg_off.empty(); }   // a failing item is booked on the item, not on the call
  };
  static int verify_commitments(VerifyRun &r) {
    r.fixed.resize(3 * r.n_rings);
    for (size_t i = 0; i < 3 * r.n_rings; i++) if (!g1_decompress<G>(r.commitments + FQB * i, &r.fixed[i])) return AVRF_INVALID_DATA;
    if (r.host_subgroup) {
      std::atomic<int> badc{0};
      parallel_for(3 * r.n_rings, [&](size_t i) { if (!g1_in_subgroup_host<G>(r.fixed[i])) badc = 1; });
      if (badc) return AVRF_INVALID_DATA;
    }
    return AVRF_OK;
  }
  // the 7 G1 points of every proof: decompression (a 381-bit square root each) and, for small batches, the subgroup test,
  // one host task per POINT so that a single verification spreads over the pool
  static void verify_points(VerifyRun &r) {
    const size_t n = r.n, np = 7 * n; RingLane &ln = r.ln;
    r.dec.resize(np); r.dec_ok.assign(np, 0);
    if (n >= DEVICE_DECOMPRESS_MIN) {
      // large batches: the square roots on the device (k_g1_decompress), one lane per point; the y coordinates come back
      // because the transcript replay below absorbs the uncompressed points
      std::vector<uint8_t> comp(np * FQB), xy(np * 2 * FQB);
      for (size_t k = 0; k < np; k++) memcpy(&comp[k * FQB], r.proofs + PL::LEN * (k / 7) + PL::G1_OFF[k % 7], FQB);
      uint8_t *d_comp, *d_xy, *d_ok;
      ln.carve().take(d_comp, np * FQB).take(d_xy, np * 2 * FQB).take(d_ok, np).into(1);
      HIP_CHECK(hipMemcpyAsync(d_comp, comp.data(), np * FQB, hipMemcpyHostToDevice, ln.stream));
      launch_g1_decompress(r.su->curve, d_comp, np, d_xy, d_ok, ln.stream);
      HIP_CHECK(hipMemcpyAsync(xy.data(), d_xy, np * 2 * FQB, hipMemcpyDeviceToHost, ln.stream));
      HIP_CHECK(hipMemcpyAsync(r.dec_ok.data(), d_ok, np, hipMemcpyDeviceToHost, ln.stream));
      HIP_CHECK(hipStreamSynchronize(ln.stream)); HIP_CHECK(hipGetLastError());
      for (size_t k = 0; k < np; k++) {
        memset(&r.dec[k], 0, sizeof r.dec[k]);
        if (r.dec_ok[k] == 2) r.dec[k].inf = true; else memcpy(r.dec[k].xy, &xy[k * 2 * FQB], 2 * FQB);
      }
      r.lap("G1 decompression (device)");
    } else
    parallel_for(np, [&](size_t k) {
      bool ok = g1_decompress<G>(r.proofs + PL::LEN * (k / 7) + PL::G1_OFF[k % 7], &r.dec[k]);
      if (ok && r.host_subgroup) ok = g1_in_subgroup_host<G>(r.dec[k]);
      r.dec_ok[k] = ok;
    });
  }
  // the transcript up to the verifier key is the same for every proof checked against one ring: absorbed once per ring
  static void verify_transcripts(VerifyRun &r) {
    r.t_ring.resize(r.n_rings);
    for (size_t k = 0; k < r.n_rings; k++) r.t_ring[k] = HR::prelude(r.su->g1_0, r.su->g2_raw, &r.fixed[3 * k]);
  }
  // every item to its bases and scalars; the items are independent until the MSMs, so the host part runs on the thread pool
  static int verify_reduce(VerifyRun &r) {
    const size_t n = r.n, e1 = 2 * FQB;
    r.b1.resize((10 * n + 1) * e1); r.b2.resize(2 * n * e1); r.s1.resize(10 * n + 1); r.s2.resize(2 * n); r.gsc.resize(n);
    r.item_st.assign(r.per_item() ? n : 0, 0);
    std::atomic<int> status{AVRF_OK};
    auto fail = [&](size_t it, int st) { if (r.per_item()) r.item_st[it] = st; else status = st; };
    const typename HR::VerifierConsts vc(r.su->N, r.su->w, r.su->ninv);
    parallel_for(n, [&](size_t it) {
      const uint32_t ring = r.ring_of_item ? r.ring_of_item[it] : 0;
      if (ring >= r.n_rings) { status = AVRF_ERR_BAD_ARG; return; }
      const G1Aff *fx = &r.fixed[3 * ring], *pts = &r.dec[7 * it];
      for (int j = 0; j < 7; j++) if (!r.dec_ok[7 * it + j]) { fail(it, AVRF_INVALID_DATA); return; }
      // randomisers r1, r2 (128 bits each)
      H256 r1, r2; HR::randomiser_pair(&r.rnd[32 * it], &r1, &r2);
      if (r.lone.empty() ? n == 1 : r.lone[it] != 0) r1 = Fr::one();
      typename HR::Item o;
      if (int st = HR::reduce(vc, r.t_ring[ring], pts, r.proofs + PL::LEN * it, r.instances_xy + 64 * it, r1, r2, o)) { fail(it, st); return; }
      uint8_t *b = &r.b1[10 * it * e1];
      for (int j = 0; j < 3; j++) memcpy(b + j * e1, fx[j].xy, e1);
      for (int j = 0; j < 7; j++) memcpy(b + (3 + j) * e1, pts[j].xy, e1);
      memcpy(&r.s1[10 * it], o.s1, sizeof o.s1);
      r.gsc[it] = o.gsc;
      memcpy(&r.b2[2 * it * e1], pts[5].xy, e1); memcpy(&r.b2[(2 * it + 1) * e1], pts[6].xy, e1);
      r.s2[2 * it] = o.s2[0]; r.s2[2 * it + 1] = o.s2[1];
    }, 4);
    return status;
  }
  // n > 1 independent verifications: per-item sums on the device, then the pairing checks on the device or, when few, on the host pool
  static int verify_tail_each(VerifyRun &r) {
    avrf_ring_setup *su = r.su; RingLane &ln = r.ln; const size_t n = r.n;
    // 13 (base, scalar) pairs per item: its 10 terms of the first argument, the g1 term, its 2 terms of the second
    const size_t e1 = 2 * FQB, TPI = 13;
    std::vector<uint8_t> bb(n * TPI * e1); std::vector<H256> ss(n * TPI);
    for (size_t it = 0; it < n; it++) {
      memcpy(&bb[(it * TPI) * e1], &r.b1[(10 * it) * e1], 10 * e1);
      for (int j = 0; j < 10; j++) ss[it * TPI + j] = r.s1[10 * it + j];
      memcpy(&bb[(it * TPI + 10) * e1], su->g1_0.xy, e1); ss[it * TPI + 10] = Fr::from_mont(Fr::neg(r.gsc[it]));
      memcpy(&bb[(it * TPI + 11) * e1], &r.b2[(2 * it) * e1], 2 * e1);
      ss[it * TPI + 11] = r.s2[2 * it]; ss[it * TPI + 12] = r.s2[2 * it + 1];
    }
    const bool host_pair = few_checks(n);
    if (!host_pair) ensure_pairing(su);
    const size_t nb = n * TPI;
    uint8_t *d_xy; uint32_t *d_b, *d_s, *d_pts, *d_flag; int32_t *d_ok, *d_rec;
    ln.carve().take(d_xy, nb * e1).take(d_b, nb * e1 / 4).take(d_s, nb * 8).take(d_pts, n * 2 * e1 / 4).take(d_ok, n).take(d_rec, n).take(d_flag, 1).into(1);
    HIP_CHECK(hipMemcpyAsync(d_xy, bb.data(), nb * e1, hipMemcpyHostToDevice, ln.stream));
    if (su->curve == 0) parallel_for(n, [&](size_t it) { for (size_t j = 0; j < TPI; j++) g1_glv_split_bls(ss[it * TPI + j].l); });   // k -> (k mod z^2, k div z^2)
    HIP_CHECK(hipMemcpyAsync(d_s, ss.data(), nb * 32, hipMemcpyHostToDevice, ln.stream));
    HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, ln.stream)); HIP_CHECK(hipMemsetAsync(d_rec, 0, n * 4, ln.stream));
    launch_g1_bases(su->curve, d_xy, nb, d_b, d_flag, ln.stream);
    if (!r.host_subgroup) launch_g1_subgroup_check(su->curve, d_b, nb, d_flag, ln.stream, d_rec, (uint32_t)TPI);
    launch_g1_lincomb(su->curve, d_b, d_s, n, (uint32_t)TPI, 11, d_pts, ln.stream, su->curve == 0);
    std::vector<int32_t> okv(n), rec(n); uint32_t range_flag = 0;
    std::vector<uint32_t> pts(host_pair ? n * 2 * e1 / 4 : 0);
    if (host_pair) HIP_CHECK(hipMemcpyAsync(pts.data(), d_pts, n * 2 * e1, hipMemcpyDeviceToHost, ln.stream));
    else {
      launch_pairing_check(su->ptab, d_pts, n, d_ok, ln.stream);
      HIP_CHECK(hipMemcpyAsync(okv.data(), d_ok, n * 4, hipMemcpyDeviceToHost, ln.stream));
    }
    HIP_CHECK(hipMemcpyAsync(rec.data(), d_rec, n * 4, hipMemcpyDeviceToHost, ln.stream));
    HIP_CHECK(hipMemcpyAsync(&range_flag, d_flag, 4, hipMemcpyDeviceToHost, ln.stream));
    HIP_CHECK(hipStreamSynchronize(ln.stream)); HIP_CHECK(hipGetLastError());
    r.lap(host_pair ? "per-item G1 sums (device)" : "per-item G1 sums + pairing checks (device)");
    if (range_flag & 1) return AVRF_INVALID_DATA;      // a base with a coordinate >= p (launch_g1_bases): no item to pin it on
    if (host_pair) { host_pair_checks(su, pts.data(), n, okv.data()); r.lap("pairing checks (host pool)"); }
    for (size_t it = 0; it < n; it++)
      r.each_status[it] = r.item_st[it] ? r.item_st[it] : rec[it] ? AVRF_INVALID_DATA : okv[it] ? AVRF_OK : AVRF_VERIFICATION_FAILURE;
    return AVRF_OK;
  }
  // the batch folded into two sums: one MSM chain on the device, one 2-pairing check on the host.  The verdict of the batch.
  // (sums_out: the two sums, for the probe of the segmented call)
  static int verify_tail_folded(VerifyRun &r, G1Aff *sums_out = nullptr) {
    avrf_ring_setup *su = r.su; const size_t n = r.n;
    H256 g1_scalar = {{0, 0, 0, 0}};
    for (size_t it = 0; it < n; it++) g1_scalar = Fr::sub(g1_scalar, r.gsc[it]);
    memcpy(&r.b1[10 * n * 2 * FQB], su->g1_0.xy, 2 * FQB); r.s1[10 * n] = Fr::from_mont(g1_scalar);
    // b1 holds every deserialised G1 point of the batch (ring commitments, proof commitments, opening proofs): its bases are
    // subgroup-checked on the device before they are used (ark-serialize Validate::Yes; BLS12-381 G1 has a large cofactor)
    bool bad = false;
    G1Aff acc1, acc2;
    g1_msm2(su, r.ln, r.b1, r.s1, r.b2, r.s2, !r.host_subgroup, &bad, &acc1, &acc2);
    if (bad) return AVRF_INVALID_DATA;
    if (sums_out) { sums_out[0] = acc1; sums_out[1] = acc2; }
    r.lap("two G1 MSMs (device, one chain)");
    const typename HP::G2Lines *lines = host_lines(su);
    QEl px[2], py[2]; bool pinf[2] = {acc1.inf, acc2.inf};
    const G1Aff *accs[2] = {&acc1, &acc2};
    for (int i = 0; i < 2; i++) { QEl x, y; g1_coords<G>(accs[i]->xy, &x, &y); px[i] = FqN::to_mont(x); py[i] = FqN::to_mont(y); }
    const bool ok = HP::product_is_one_lines_par(px, py, pinf, lines, 2, [](size_t k, auto fn) { parallel_for(k, fn); });   // the two Miller loops side by side
    r.lap("2-pairing check (host)");
    return ok ? AVRF_OK : AVRF_VERIFICATION_FAILURE;
  }
  static int verify_batch(avrf_ring_setup *su, size_t n, const uint8_t *commitments, const uint32_t *ring_of_item, size_t n_rings,
                          const uint8_t *instances_xy, const uint8_t *proofs, int32_t *each_status = nullptr) {
    if (n == 0) return AVRF_OK;
    VerifyRun r{su, su->lane[0], n, n_rings, commitments, ring_of_item, instances_xy, proofs, each_status, RingTrace("ring_verify", n, false),
                FQB == 48 && 10 * n + 3 * n_rings <= 512};
    if (int st = verify_commitments(r)) return st;
    r.rnd = HR::batch_randomisers(n, n_rings, su->N, su->g1_0, su->g2_raw, ring_of_item, commitments, instances_xy, proofs);
    verify_points(r);
    verify_transcripts(r);
    if (int st = verify_reduce(r)) return st;
    r.lap("decode + transcripts (host)");
    // ONE independent verification is a batch of one: its two 11- / 2-term sums go through the MSM engine and the pairing
    // check runs on the host (2.4 ms; the per-item device form is paced by lone 381-bit double-and-add chains: 5 ms)
    if (each_status && n == 1 && r.item_st[0]) { each_status[0] = r.item_st[0]; return AVRF_OK; }
    if (each_status && n > 1) return verify_tail_each(r);
    const int verdict = verify_tail_folded(r);
    if (each_status) { each_status[0] = verdict; return AVRF_OK; }
    return verdict;
  }

  // ---- n_seg independent BatchVerifiers (src/ring.rs:682-735, one per segment) over consecutive runs of the items: DESIGN.md 4.17.
  // The stages of verify_batch with the segment boundaries in the record, then a third tail.  Segment v's randomisers are those of a
  // batch call on its items alone (HR::segment_randomisers), so its two sums are the sums avrf_ring_batch_verify forms for them.
  //
  // verify_tail_segments: every segment is two vectors of ONE segmented G1 chain (msm.h msm_g1_segments), A_v = its items' 10 terms each
  // and the g1 term with -sum gsc, B_v = its items' 2 terms each, both padded with zero scalars to L = 10 (longest segment) + 1; the
  // finishing kernel leaves (A_v, B_v) side by side as one pairing check's two points, which the device pairing kernel reads where they
  // lie -- or, for few segments (few_checks), the host pool from the copy back.  A segment the host part condemned contributes zero
  // scalars and keeps the host's status; so does an empty one (AVRF_OK).  More segments than one chain's limits hold run as several
  // chains over consecutive runs of segments (RingSegLayout::per_round).
  // st: n_seg statuses, the host's verdicts on entry; sums: 2 n_seg canonical points for avrf_ring_segment_sums.
  static int verify_tail_segments(VerifyRun &r, const RingSegLayout &lay, std::vector<int32_t> &st, std::vector<uint8_t> &sums) {
    avrf_ring_setup *su = r.su; RingLane &ln = r.ln;
    const size_t n_seg = r.seg_off.size() - 1, e1 = 2 * FQB, L = (size_t)lay.L;
    const bool host_pair = few_checks(n_seg), dev_subgroup = !r.host_subgroup && su->curve == 0;
    if (!host_pair) ensure_pairing(su);
    for (size_t s0 = 0; s0 < n_seg; s0 += lay.per_round) {
      const size_t ns = n_seg - s0 < lay.per_round ? n_seg - s0 : lay.per_round, nv = 2 * ns, np = nv * L;
      std::vector<uint8_t> bb(np * e1, 0); std::vector<H256> ss(np, H256{{0, 0, 0, 0}});
      std::vector<uint32_t> pt, rec_of;                // the proofs' G1 points still to be subgroup-tested | the segment (of this round) each belongs to
      for (size_t j = 0; j < ns; j++) {
        const size_t v = s0 + j, first = r.seg_off[v], cnt = r.seg_off[v + 1] - first;
        if (!cnt || st[v]) continue;
        const size_t a0 = 2 * j * L, b0 = (2 * j + 1) * L;
        memcpy(&bb[a0 * e1], &r.b1[10 * first * e1], 10 * cnt * e1);
        for (size_t k = 0; k < 10 * cnt; k++) ss[a0 + k] = r.s1[10 * first + k];
        H256 g = {{0, 0, 0, 0}};
        for (size_t it = first; it < first + cnt; it++) g = Fr::sub(g, r.gsc[it]);
        memcpy(&bb[(a0 + 10 * cnt) * e1], su->g1_0.xy, e1); ss[a0 + 10 * cnt] = Fr::from_mont(g);
        memcpy(&bb[b0 * e1], &r.b2[2 * first * e1], 2 * cnt * e1);
        for (size_t k = 0; k < 2 * cnt; k++) ss[b0 + k] = r.s2[2 * first + k];
        // (the ring commitments, terms 0 .. 2 of an item, were tested once per call; pi_1 and pi_2 of B_v are terms 8 and 9 of A_v)
        if (dev_subgroup) for (size_t it = 0; it < cnt; it++) for (size_t p = 3; p < 10; p++) { pt.push_back((uint32_t)(a0 + 10 * it + p)); rec_of.push_back((uint32_t)j); }
      }
      uint8_t *d_xy; uint32_t *d_b, *d_s, *d_pts, *d_flag, *d_pt, *d_rec_of; int32_t *d_ok, *d_rec;
      ln.carve().take(d_xy, np * e1).take(d_b, np * e1 / 4).take(d_s, np * 8).take(d_pts, nv * e1 / 4).take(d_ok, ns).take(d_rec, ns).take(d_flag, 1)
          .take(d_pt, pt.size()).take(d_rec_of, pt.size()).into(1);
      HIP_CHECK(hipMemcpyAsync(d_xy, bb.data(), np * e1, hipMemcpyHostToDevice, ln.stream));
      HIP_CHECK(hipMemcpyAsync(d_s, ss.data(), np * 32, hipMemcpyHostToDevice, ln.stream));
      HIP_CHECK(hipMemsetAsync(d_flag, 0, 4, ln.stream)); HIP_CHECK(hipMemsetAsync(d_rec, 0, ns * 4, ln.stream));
      launch_g1_bases(su->curve, d_xy, np, d_b, d_flag, ln.stream);
      if (!pt.empty()) {
        HIP_CHECK(hipMemcpyAsync(d_pt, pt.data(), pt.size() * 4, hipMemcpyHostToDevice, ln.stream));
        HIP_CHECK(hipMemcpyAsync(d_rec_of, rec_of.data(), pt.size() * 4, hipMemcpyHostToDevice, ln.stream));
        launch_g1_subgroup_check_list(su->curve, d_b, d_pt, d_rec_of, pt.size(), d_flag, d_rec, ln.stream);
      }
      std::vector<uint8_t> xy(nv * e1);
      // (the layout keeps every round inside the engine's limits: a refusal here is a defect, not an input)
      if (msm_g1_segments(su->curve, d_b, d_s, L, nv, ln.ws, ln.stream, xy.data(), d_pts)) throw HipFailure{hipErrorInvalidValue, __FILE__, __LINE__};   // (synchronises the stream)
      r.lap("segment sums (device, one chain)");
      std::vector<int32_t> okv(ns), rec(ns); uint32_t range_flag = 0;
      if (!host_pair) {
        launch_pairing_check(su->ptab, d_pts, ns, d_ok, ln.stream);
        HIP_CHECK(hipMemcpyAsync(okv.data(), d_ok, ns * 4, hipMemcpyDeviceToHost, ln.stream));
      }
      HIP_CHECK(hipMemcpyAsync(rec.data(), d_rec, ns * 4, hipMemcpyDeviceToHost, ln.stream));
      HIP_CHECK(hipMemcpyAsync(&range_flag, d_flag, 4, hipMemcpyDeviceToHost, ln.stream));
      HIP_CHECK(hipStreamSynchronize(ln.stream)); HIP_CHECK(hipGetLastError());
      if (range_flag & 1) return AVRF_INVALID_DATA;      // a base with a coordinate >= p (launch_g1_bases): no segment to pin it on
      // the chain's record holds the Montgomery affine points the finishing kernel wrote: what the host pairing reads
      if (host_pair) { host_pair_checks(su, ln.ws.own.bits_host.template as<uint32_t>(), ns, okv.data()); r.lap("pairing checks (host pool)"); }
      else r.lap("pairing checks (device)");
      for (size_t j = 0; j < ns; j++) {
        const size_t v = s0 + j;
        if (r.seg_off[v + 1] == r.seg_off[v] || st[v]) continue;
        st[v] = rec[j] ? AVRF_INVALID_DATA : okv[j] ? AVRF_OK : AVRF_VERIFICATION_FAILURE;
        memcpy(&sums[2 * v * e1], &xy[2 * j * e1], 2 * e1);
      }
    }
    return AVRF_OK;
  }
  // one segment through the folded tail: the batch of its items alone
  static int verify_segment_folded(VerifyRun &r, size_t v, uint8_t *sums_xy) {
    const size_t first = r.seg_off[v], cnt = r.seg_off[v + 1] - first, e1 = 2 * FQB;
    VerifyRun q{r.su, r.ln, cnt, r.n_rings, r.commitments, r.ring_of_item, r.instances_xy, r.proofs, nullptr, RingTrace("ring_verify_segment", cnt, false), r.host_subgroup};
    q.b1.assign(r.b1.begin() + 10 * first * e1, r.b1.begin() + 10 * (first + cnt) * e1); q.b1.resize((10 * cnt + 1) * e1);
    q.s1.assign(r.s1.begin() + 10 * first, r.s1.begin() + 10 * (first + cnt)); q.s1.resize(10 * cnt + 1);
    q.b2.assign(r.b2.begin() + 2 * first * e1, r.b2.begin() + 2 * (first + cnt) * e1);
    q.s2.assign(r.s2.begin() + 2 * first, r.s2.begin() + 2 * (first + cnt));
    q.gsc.assign(r.gsc.begin() + first, r.gsc.begin() + first + cnt);
    G1Aff acc[2];
    const int verdict = verify_tail_folded(q, acc);
    if (verdict != AVRF_INVALID_DATA) { memcpy(sums_xy, acc[0].xy, e1); memcpy(sums_xy + e1, acc[1].xy, e1); }
    return verdict;
  }
  // Fewer segments than this run the folded tail once per segment instead of the chain: one segment IS the folded batch, and two
  // folded tails are two launch chains, two host Horners and two host pairings against one chain.  The threshold has not been
  // measured (tools/ring_segments_bench.py times 16 segments and more); this is the one place it is written.
  static constexpr size_t RING_SEG_CHAIN_MIN = 2;
  static int verify_segments(avrf_ring_setup *su, size_t n, const uint8_t *commitments, const uint32_t *ring_of_item, size_t n_rings,
                             const uint8_t *instances_xy, const uint8_t *proofs, const RingSegLayout &lay, int32_t *status_out) {
    const size_t n_seg = lay.off.size() - 1, e1 = 2 * FQB;
    std::vector<int32_t> st(n_seg, AVRF_OK);
    std::vector<uint8_t> sums(2 * n_seg * e1, 0);
    su->seg_sums_n = 0;
    if (n) {
      VerifyRun r{su, su->lane[0], n, n_rings, commitments, ring_of_item, instances_xy, proofs, nullptr, RingTrace("ring_verify_segments", n, false),
                  FQB == 48 && 10 * n + 3 * n_rings <= 512};
      r.seg_off = lay.off; r.lone.assign(n, 0);
      for (size_t v = 0; v < n_seg; v++) if (lay.off[v + 1] - lay.off[v] == 1) r.lone[lay.off[v]] = 1;
      // all 3 n_rings commitments before any segment: decoded, and in the subgroup whichever side tests the proofs' points
      if (int s = verify_commitments(r)) return s;
      if (!r.host_subgroup) {
        std::atomic<int> badc{0};
        parallel_for(3 * n_rings, [&](size_t i) { if (!g1_in_subgroup_host<G>(r.fixed[i])) badc = 1; });
        if (badc) return AVRF_INVALID_DATA;
      }
      r.rnd.resize(32 * n);
      parallel_for(n_seg, [&](size_t v) {
        HR::segment_randomisers(lay.off[v], lay.off[v + 1] - lay.off[v], n_rings, su->N, su->g1_0, su->g2_raw, ring_of_item, commitments, instances_xy, proofs, &r.rnd[32 * lay.off[v]]);
      });
      verify_points(r);
      verify_transcripts(r);
      if (int s = verify_reduce(r)) return s;
      r.lap("decode + transcripts (host)");
      // the host's verdict on a segment: AVRF_INVALID_DATA wins over AVRF_VERIFICATION_FAILURE, whatever the order of its items
      for (size_t v = 0; v < n_seg; v++)
        for (size_t it = lay.off[v]; it < lay.off[v + 1]; it++)
          if (r.item_st[it] == AVRF_INVALID_DATA || (r.item_st[it] && !st[v])) st[v] = r.item_st[it];
      if (n_seg < RING_SEG_CHAIN_MIN) {
        for (size_t v = 0; v < n_seg; v++) if (lay.off[v + 1] != lay.off[v] && !st[v]) st[v] = verify_segment_folded(r, v, &sums[2 * v * e1]);
      } else if (int s = verify_tail_segments(r, lay, st, sums)) return s;
    }
    for (size_t v = 0; v < n_seg; v++) status_out[v] = st[v];
    su->seg_sums = std::move(sums); su->seg_sums_n = n_seg;
    return AVRF_OK;
  }
};

using RingB = Ring<SuiteBandersnatch, G1Bls12381>;
using RingJ = Ring<SuiteBabyJubJub, G1Bn254>;
using RingK = Ring<SuiteJubJub, G1Bls12381>;        // JubJub-SHA512-TAI over BLS12-381 (src/suites/jubjub.rs:76-95)
using RingX = Ring<SuiteBandersnatchShake, G1Bls12381>;   // Bandersnatch with the SHAKE128 transcript (src/suites/bandersnatch_shake128.rs)
using RingW = Ring<SuiteBandersnatchSW, G1Bls12381>;   // Bandersnatch-SW: the ring proof runs on the TEMapping of the keys (src/ring.rs:75-81)
// f(r) with r a value of the suite's Ring: it has only static members, so r.f(...) names them
template <class F> static auto with_ring(int suite, F &&f) {
  switch (suite) { case 1: return f(RingJ{}); case 2: return f(RingK{}); case 4: return f(RingW{}); case 5: return f(RingX{}); default: return f(RingB{}); }
}
// the compressed RingCommitment: the three column commitments in the pairing curve's encoding
static void encode_commitment(int curve, const G1Aff C[3], uint8_t *out) {
  std::vector<uint8_t> b;
  for (int i = 0; i < 3; i++) { if (curve == 0) g1_encode<G1Bls12381>(C[i], true, b); else g1_encode<G1Bn254>(C[i], true, b); }
  memcpy(out, b.data(), b.size());
}

}  // namespace

// The tables of all multiples of this setup's SRS powers (kind 0) and witness bases (kind 1): found in the registry or built (once
// per device and SRS, ~2 s).
//  - no explicit budget (the process default): sized to the HBM that is free -- the widest window c <= 16 whose table fits
//    min(what is left of AVRF_RING_TABLE_GB (default 232, both tables together), free - 40 GB), any registry table of the SRS adopted;
//    no table when even the bucket form's own width does not fit, when AVRF_RING_DIRECT=0, or when the allocation fails (the bucket form
//    then runs as before).
//  - an explicit budget (avrf_ring_setup_set_table_budget): the widths are a pure function of it (plan_direct); free memory only
//    decides whether a planned table is built, and a registry table is adopted only at exactly the planned width.
// Either way table_missed records a planned table that is not held.  Called under no lock; takes g_direct_mu.
static bool direct_env_off() { const char *e = getenv("AVRF_RING_DIRECT"); return e && atoi(e) == 0; }
static double direct_env_budget_gb() { const char *e = getenv("AVRF_RING_TABLE_GB"); return e ? atof(e) : 232.0; }
static bool tables_disabled(const avrf_ring_setup *su) { return su->table_budget != UINT64_MAX ? su->table_budget == 0 : direct_env_off(); }
static size_t direct_bases(const avrf_ring_setup *su, int kind) { return kind ? 2 * su->N + 1 : su->n_srs; }
// bytes of the table of `nb` bases at width c, 0 when it would hold 2^31 - 1 points or more (31-bit entry indices of k_direct_index)
static uint64_t direct_bytes(int curve, size_t nb, int c) {
  G1DirectTable shape;
  const uint64_t b = g1_direct_table_shape(curve, nb, c, &shape);
  return shape.points < 0x7fffffffull ? b : 0;
}
// the explicit-budget plan: the SRS table the widest c in [bucket width, 16] that fits the budget, then the witness table the widest
// c in [8, 16] that fits what is left (c = 0: no table of that kind)
static void plan_direct(const avrf_ring_setup *su, uint64_t budget, int c_out[2], uint64_t bytes_out[2]) {
  for (int kind = 0; kind < 2; kind++) {
    c_out[kind] = 0; bytes_out[kind] = 0;
    const int c_lo = kind ? 8 : std::max(su->table_c, 8);
    for (int c = 16; c >= c_lo; c--) {
      const uint64_t b = direct_bytes(su->curve, direct_bases(su, kind), c);
      if (b && b <= budget) { c_out[kind] = c; bytes_out[kind] = b; budget -= b; break; }
    }
  }
}
static void drop_tables_locked(avrf_ring_setup *su) {                 // (g_direct_mu held: the registry frees a table with its last holder)
  su->direct.reset(); su->direct_wit.reset();
}
static std::shared_ptr<DirectEntry> find_direct_locked(const avrf_ring_setup *su, int kind, int c_exact) {
  const size_t nb = direct_bases(su, kind);
  for (auto it = g_direct.begin(); it != g_direct.end();) {
    std::shared_ptr<DirectEntry> e = it->lock();
    if (!e) { it = g_direct.erase(it); continue; }
    if (e->device == su->device && e->kind == kind && e->t.curve == su->curve && e->t.n == nb && e->srs_key == su->g1_raw && (!c_exact || e->t.c == c_exact)) return e;
    ++it;
  }
  return nullptr;
}
static uint64_t held_bytes_locked(int device) {
  uint64_t sum = 0;
  for (auto &w : g_direct) if (std::shared_ptr<DirectEntry> e = w.lock()) if (e->device == device && e->t.d) sum += e->t.bytes;
  return sum;
}
static void ensure_direct(avrf_ring_setup *su) {
  if (su->direct_tried || !su->n_srs) return;
  su->direct_tried = true;
  su->table_missed = false;
  su->planned_budget = su->table_budget;
  const bool expl = su->table_budget != UINT64_MAX;
  if (tables_disabled(su)) { std::lock_guard<std::mutex> lk(g_direct_mu); drop_tables_locked(su); return; }
  with_ring(su->suite, [&](auto r) { r.ensure_lagrange(su); return 0; });   // the witness bases
  std::lock_guard<std::mutex> lk(g_direct_mu);
  double budget_gb = direct_env_budget_gb();
  int plan_c[2] = {0, 0}; uint64_t plan_b[2] = {0, 0};
  if (expl) plan_direct(su, su->table_budget, plan_c, plan_b);
  // kind 0 over the SRS powers, then kind 1 over the witness bases with what is left of the budget
  for (int kind = 0; kind < 2; kind++) {
    std::shared_ptr<DirectEntry> &slot = kind ? su->direct_wit : su->direct;
    const size_t nb = direct_bases(su, kind);
    const uint32_t *bases = (kind ? su->d_wit_bases : su->d_srs).as();
    if (!bases) continue;
    int c = 0;
    if (expl) {
      if (slot && slot->t.c != plan_c[kind]) slot.reset();               // (held at another width: released before anything is built)
      if (!plan_c[kind] || slot) continue;                               // nothing planned, or held at the planned width already
      if ((slot = find_direct_locked(su, kind, plan_c[kind]))) continue;
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); su->table_missed = true; continue; }
      if ((double)plan_b[kind] > (double)free_b - 40e9) { su->table_missed = true; continue; }
      c = plan_c[kind];
    } else {
      const int c_min = kind ? su->wit_c : su->table_c;
      if (kind) if (const char *e = getenv("AVRF_RING_DIRECT_WIT")) if (atoi(e) == 0) continue;   // (A/B knob: the witness commits stay on the bucket form)
      if (!slot) slot = find_direct_locked(su, kind, 0);
      if (slot) { budget_gb -= slot->t.bytes * 1e-9; continue; }
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); break; }
      double usable = (double)free_b - 40e9; if (usable > budget_gb * 1e9) usable = budget_gb * 1e9;
      for (int cc = 16; cc >= c_min && cc >= 8; cc--) {
        const uint64_t b = direct_bytes(su->curve, nb, cc);
        if (b && (double)b <= usable) { c = cc; break; }
      }
      if (!c) continue;
    }
    auto e = std::make_shared<DirectEntry>();
    e->device = su->device; e->kind = kind; e->srs_key = su->g1_raw;
    try { build_g1_direct_table(su->curve, bases, nb, c, &e->t, su->lane[0].stream); }
    catch (const HipFailure &) { (void)hipGetLastError(); su->table_missed = true; continue; }   // (the entry's destructor frees what was allocated)
    g_direct.push_back(e);
    slot = e;
    budget_gb -= e->t.bytes * 1e-9;
  }
}

extern "C" {

int avrf_ring_setup_load(avrf_ctx *ctx, const uint8_t *srs, size_t srs_len, size_t ring_size, avrf_ring_setup **out) {
  if (!ctx || !srs || !out || ring_size == 0) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(ctx)) return AVRF_ERR_BAD_ARG;
  *out = nullptr;
  if (!ring_suite(avrf_ctx_suite_(ctx))) return AVRF_ERR_BAD_ARG;      // not a RingSuite (Ed25519)
  return guarded([&] { return with_ring(avrf_ctx_suite_(ctx), [&](auto r) { return r.setup_load(ctx, srs, srs_len, ring_size, out); }); });
}
int avrf_ring_srs_generate(avrf_ctx *ctx, const uint8_t *tau, const uint8_t *g1, const uint8_t *g2, size_t n_g1, uint8_t *out, size_t out_cap, size_t *out_len) {
  if (!ctx || !tau || !g1 || !g2 || !ring_suite(avrf_ctx_suite_(ctx))) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(ctx)) return AVRF_ERR_BAD_ARG;
  return guarded([&] { return with_ring(avrf_ctx_suite_(ctx), [&](auto r) { return r.srs_generate(ctx, tau, g1, g2, n_g1, out, out_cap, out_len); }); });
}
int avrf_ring_setup_from_seed(avrf_ctx *ctx, const uint8_t *seed, size_t ring_size, avrf_ring_setup **out) {
  if (!ctx || !seed || !out || !ring_suite(avrf_ctx_suite_(ctx))) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(ctx)) return AVRF_ERR_BAD_ARG;
  *out = nullptr;
  return guarded([&] { return with_ring(avrf_ctx_suite_(ctx), [&](auto r) { return r.setup_from_seed(ctx, seed, ring_size, out); }); });
}
size_t avrf_ring_pcs_domain_size(int suite, size_t ring_size) {       /* pcs_domain_size, src/ring.rs:810-817: 3 * piop_domain + 1 */
  const size_t L = with_suite(suite, [&](auto tag) { using S = typename decltype(tag)::type; return (size_t)S::Fr::BITS; });
  return 3 * ring_domain_size(ring_size, L) + 1;
}
void avrf_ring_setup_free(avrf_ring_setup *su) {
  if (!su) return;
  (void)hipSetDevice(su->device);
  { std::lock_guard<std::mutex> lk(g_direct_mu); drop_tables_locked(su); }
  delete su;
}
size_t avrf_ring_max_ring_size(const avrf_ring_setup *su) { return su ? su->keyset : 0; }
size_t avrf_ring_domain_size(const avrf_ring_setup *su) { return su ? su->N : 0; }
size_t avrf_ring_proof_len(const avrf_ring_setup *su) { return su ? ring_proof_len(su->curve) : 0; }
size_t avrf_ring_commitment_len(const avrf_ring_setup *su) { return su ? ring_commitment_len(su->curve) : 0; }
int avrf_ring_setup_suite(const avrf_ring_setup *su) { return su ? su->suite : -1; }
avrf_ring_setup *avrf_ring_key_setup(const avrf_ring_key *key) { return key ? key->setup : nullptr; }
int avrf_ring_setup_plan(const avrf_ring_setup *su, int32_t out[4]) {
  if (!su || !out) return AVRF_ERR_BAD_ARG;
  out[0] = su->table_c; out[1] = su->table_nwin; out[2] = su->wit_c; out[3] = su->wit_nwin;   // the witness table is built on first proof
  // once a batched prove call has built the tables of all multiples, those are what the commitments of a batch run over
  if (su->direct) { out[0] = su->direct->t.c; out[1] = su->direct->t.rows; }
  if (su->direct_wit) { out[2] = su->direct_wit->t.c; out[3] = su->direct_wit->t.rows; }
  return AVRF_OK;
}
uint64_t avrf_ring_table_bytes(int suite, size_t ring_size, int kind, int c) {
  if (!ring_suite(suite) || ring_size == 0 || ring_size > ((size_t)1 << 40) || (kind != 0 && kind != 1) || c < 8 || c > 16) return 0;
  const size_t pcs = avrf_ring_pcs_domain_size(suite, ring_size), N = (pcs - 1) / 3;
  return direct_bytes(pairing_curve_of(suite), kind ? 2 * N + 1 : pcs, c);
}
int avrf_ring_setup_set_table_budget(avrf_ring_setup *su, uint64_t bytes) {
  if (!su) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  if (!su->n_srs) return AVRF_SRS_LOOKUP_FAILED;
  su->table_budget = bytes;                                            // (read at the next build; the tables held stay)
  return AVRF_OK;
}
int avrf_ring_setup_build_tables(avrf_ring_setup *su) {
  if (!su) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  if (!su->n_srs) return AVRF_SRS_LOOKUP_FAILED;
  if (hipSetDevice(su->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  // a new budget: the tables of the old plan are released first, so that the new ones can take their memory; the same plan: the held
  // tables stay (a no-op, or a retry of the tables that were not built)
  if (su->planned_budget != su->table_budget) { std::lock_guard<std::mutex> lk(g_direct_mu); drop_tables_locked(su); }
  su->direct_tried = false;
  if (int st = guarded([&] { ensure_direct(su); return (int)AVRF_OK; })) return st;
  return su->table_missed ? AVRF_ERR_NO_DEVICE : AVRF_OK;
}
int avrf_ring_setup_release_tables(avrf_ring_setup *su) {
  if (!su) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  if (!su->n_srs) return AVRF_SRS_LOOKUP_FAILED;
  (void)hipSetDevice(su->device);                                      // (the entry's destructor frees on its own device)
  std::lock_guard<std::mutex> lk(g_direct_mu);
  su->direct_tried = true;                                             // no lazy build again until avrf_ring_setup_build_tables
  su->table_missed = false;
  drop_tables_locked(su);
  return AVRF_OK;
}
int avrf_ring_setup_tables(const avrf_ring_setup *su, uint64_t out[10]) {
  if (!su || !out) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  if (!su->n_srs) return AVRF_SRS_LOOKUP_FAILED;
  const bool expl = su->table_budget != UINT64_MAX, off = tables_disabled(su);
  std::lock_guard<std::mutex> lk(g_direct_mu);
  for (int i = 0; i < 10; i++) out[i] = 0;
  out[0] = (su->direct ? 1u : 0u) | (su->direct_wit ? 2u : 0u) | (expl ? 4u : 0u) | (su->table_missed ? 8u : 0u) | (off ? 16u : 0u);
  out[1] = expl ? su->table_budget : off ? 0 : (uint64_t)(direct_env_budget_gb() * 1e9);
  if (su->direct) { out[2] = (uint64_t)su->direct->t.c; out[3] = (uint64_t)su->direct->t.rows; out[4] = su->direct->t.bytes; }
  if (su->direct_wit) { out[5] = (uint64_t)su->direct_wit->t.c; out[6] = (uint64_t)su->direct_wit->t.rows; out[7] = su->direct_wit->t.bytes; }
  out[8] = su->table_batches.load();
  out[9] = held_bytes_locked(su->device);
  return AVRF_OK;
}

int avrf_ring_index(avrf_ring_setup *su, const uint8_t *pks_xy, size_t n_keys, avrf_ring_key **out, uint8_t *commitment_out) {
  if (!su || !out || (n_keys && !pks_xy)) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  *out = nullptr;
  if (!su->n_srs) return AVRF_SRS_LOOKUP_FAILED;                       // verifier-only setup
  if (hipSetDevice(su->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  std::unique_ptr<avrf_ring_key> k;
  if (int st = guarded([&] { return with_ring(su->suite, [&](auto r) { return r.index(su, pks_xy, n_keys, k); }); })) return st;
  if (commitment_out) encode_commitment(su->curve, k->C, commitment_out);
  *out = k.release();
  return AVRF_OK;
}
void avrf_ring_key_free(avrf_ring_key *k) { delete k; }

int avrf_ring_vk_builder_new(avrf_ring_setup *su, avrf_ring_vk_builder **out) {
  if (!su || !out) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  *out = nullptr;
  if (!su->n_srs) return AVRF_SRS_LOOKUP_FAILED;
  if (hipSetDevice(su->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  return guarded([&] { return with_ring(su->suite, [&](auto r) { return r.builder_new(su, out); }); });
}
void avrf_ring_vk_builder_free(avrf_ring_vk_builder *b) { delete b; }
size_t avrf_ring_vk_builder_free_slots(const avrf_ring_vk_builder *b) { return b ? b->setup->keyset - b->curr : 0; }
int avrf_ring_vk_builder_append(avrf_ring_vk_builder *b, const uint8_t *pks_xy, size_t n) {
  if (!b || (n && !pks_xy)) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(b->setup->ctx)) return AVRF_ERR_BAD_ARG;
  if (hipSetDevice(b->setup->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  return guarded([&] { return with_ring(b->setup->suite, [&](auto r) { return r.builder_append(b, pks_xy, n); }); });
}
int avrf_ring_vk_builder_finalize(const avrf_ring_vk_builder *b, uint8_t *commitment_out) {
  if (!b || !commitment_out) return AVRF_ERR_BAD_ARG;
  encode_commitment(b->setup->curve, b->C, commitment_out);
  return AVRF_OK;
}

int avrf_ring_prove(avrf_ring_key *k, size_t n, const uint32_t *key_index, const uint8_t *blindings, int blinding_mode, uint8_t *proofs_out) {
  if (!k || (n && (!key_index || !blindings || !proofs_out))) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(k->setup->ctx)) return AVRF_ERR_BAD_ARG;
  if (blinding_mode != 0 && blinding_mode != 1) return AVRF_ERR_BAD_ARG;
  if (hipSetDevice(k->setup->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  const size_t plen = ring_proof_len(k->setup->curve);
  // proofs proved in lockstep per device round: at most 512, and a call of up to 1024 proofs is cut in TWO so that both lanes
  // work (the host rounds of one chunk hide behind the device rounds of the other) -- a rank of an 8-GPU node proves 128 proofs
  // per context (BASELINE configs[3]: 4096 proofs / 8 ranks / 4 contexts), which as ONE chunk on one lane left the device
  // idle during every transcript round: 8.99 -> 10.0 k proofs/s for 512 proofs on 4 contexts with 2 host cores
  size_t chunk = 512;
  if (n >= 32 && n <= 1024) chunk = (n + 1) / 2;
  if (const char *e = getenv("AVRF_RING_CHUNK")) { long v = atol(e); if (v >= 1 && v <= 4096) chunk = (size_t)v; }   // (test hook: re-read per call)
  avrf_ring_setup *su = k->setup;
  if (!n) return AVRF_OK;
  for (size_t i = 0; i < n; i++) if (key_index[i] >= k->n_keys) return AVRF_ERR_BAD_ARG;   // (a refused call builds nothing)
  // everything the chunks share is built here, before a chunk is in flight: the tables of all multiples and the witness table
  if (n >= 64) if (int st = guarded([&] { ensure_direct(su); return (int)AVRF_OK; })) return st;
  if (int st = guarded([&] { return with_ring(su->suite, [&](auto r) { r.ensure_lagrange(su); return (int)AVRF_OK; }); })) return st;
  auto run = [&](RingLane &lane, size_t i) {
    const size_t m = n - i < chunk ? n - i : chunk;
    return guarded([&] {
      return with_ring(su->suite, [&](auto r) { return r.prove_chunk(k, lane, m, key_index + i, blindings + 32 * i, blinding_mode == 1, proofs_out + plen * i); }); });
  };
  const char *le = getenv("AVRF_RING_LANES"); const bool one_lane = le && atoi(le) == 1;
  if (n <= chunk || one_lane) {
    for (size_t i = 0; i < n; i += chunk) if (int st = run(su->lane[0], i)) return st;
    return AVRF_OK;
  }
  // two chunks in flight: chunks alternate between the two lanes
  RingLane *lanes[2] = {&su->lane[0], &su->lane[1]};
  if (int st = guarded([&] {                                           // the second lane's stream, on the first two-lane call
        RingLane &l = su->lane[1];
        if (!l.owns_stream) { HIP_CHECK(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking)); l.owns_stream = true; }
        return (int)AVRF_OK; })) return st;
  std::atomic<int> status{AVRF_OK};
  std::thread th[2];
  for (int t = 0; t < 2; t++) th[t] = std::thread([&, t] {
    if (hipSetDevice(su->device) != hipSuccess) { status = AVRF_ERR_NO_DEVICE; return; }
    for (size_t i = (size_t)t * chunk; i < n && status == AVRF_OK; i += 2 * chunk) if (int st = run(*lanes[t], i)) status = st;
  });
  for (auto &x : th) x.join();
  return status;
}

static int copy_out(const std::vector<uint8_t> &v, uint8_t *out, size_t cap, size_t *out_len) {
  if (out_len) *out_len = v.size();
  if (!out || cap < v.size()) return AVRF_ERR_BAD_ARG;
  memcpy(out, v.data(), v.size());
  return AVRF_OK;
}
int avrf_ring_verifier_setup_load(avrf_ctx *ctx, const uint8_t *params, size_t params_len, size_t ring_size, avrf_ring_setup **out) {
  if (!ctx || !params || !out || ring_size == 0) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(ctx)) return AVRF_ERR_BAD_ARG;
  *out = nullptr;
  if (!ring_suite(avrf_ctx_suite_(ctx))) return AVRF_ERR_BAD_ARG;
  return guarded([&] { return with_ring(avrf_ctx_suite_(ctx), [&](auto r) { return r.verifier_setup_load(ctx, params, params_len, ring_size, out); }); });
}
int avrf_ring_pcs_verifier_params_serialize(avrf_ring_setup *su, int compress, uint8_t *out, size_t out_cap, size_t *out_len) {
  if (!su) return AVRF_ERR_BAD_ARG;
  std::vector<uint8_t> v;
  int st = guarded([&] { return with_ring(su->suite, [&](auto r) { return r.verifier_params_serialize(su, compress != 0, v); }); });
  return st ? st : copy_out(v, out, out_cap, out_len);
}
int avrf_ring_setup_serialize(avrf_ring_setup *su, int compress, uint8_t *out, size_t out_cap, size_t *out_len) {
  if (!su) return AVRF_ERR_BAD_ARG;
  if (!su->n_srs) return AVRF_SRS_LOOKUP_FAILED;
  std::vector<uint8_t> v;
  int st = guarded([&] { return with_ring(su->suite, [&](auto r) { return r.setup_serialize(su, compress != 0, v); }); });
  return st ? st : copy_out(v, out, out_cap, out_len);
}
int avrf_ring_builder_params_serialize(avrf_ring_setup *su, int compress, uint8_t *out, size_t out_cap, size_t *out_len) {
  if (!su) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  if (!su->n_srs) return AVRF_SRS_LOOKUP_FAILED;
  if (hipSetDevice(su->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  std::vector<uint8_t> v;
  int st = guarded([&] { return with_ring(su->suite, [&](auto r) { return r.builder_params_serialize(su, compress != 0, v); }); });
  return st ? st : copy_out(v, out, out_cap, out_len);
}

int avrf_ring_verify_each(avrf_ring_setup *su, size_t n, const uint8_t *ring_commitments, size_t n_rings, const uint32_t *ring_of_item,
                          const uint8_t *instances_xy, const uint8_t *ring_proofs, int32_t *status_out) {
  if (!su || (n && (!ring_commitments || !n_rings || !instances_xy || !ring_proofs || !status_out))) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  if (hipSetDevice(su->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  return guarded([&] {
    return with_ring(su->suite, [&](auto r) { return r.verify_batch(su, n, ring_commitments, ring_of_item, n_rings, instances_xy, ring_proofs, status_out); }); });
}

int avrf_ring_pairing_check(avrf_ring_setup *su, size_t n, const uint8_t *a_xy, const uint8_t *b_xy, int32_t *ok_out) {
  if (!su || (n && (!a_xy || !b_xy || !ok_out))) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  if (hipSetDevice(su->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  return guarded([&] { return with_ring(su->suite, [&](auto r) { return r.pairing_check(su, n, a_xy, b_xy, ok_out); }); });
}

int avrf_ring_batch_verify(avrf_ring_setup *su, size_t n, const uint8_t *ring_commitments, size_t n_rings, const uint32_t *ring_of_item,
                           const uint8_t *instances_xy, const uint8_t *ring_proofs) {
  if (!su || (n && (!ring_commitments || !n_rings || !instances_xy || !ring_proofs))) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  if (hipSetDevice(su->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  return guarded([&] {
    return with_ring(su->suite, [&](auto r) { return r.verify_batch(su, n, ring_commitments, ring_of_item, n_rings, instances_xy, ring_proofs); }); });
}

// n_seg independent ring BatchVerifiers (src/ring.rs:682-735) over consecutive runs of the n items: include/avrf.h.  Every refusal for
// the arguments is decided before anything is decoded or launched.
int avrf_ring_batch_verify_segments(avrf_ring_setup *su, size_t n, const uint8_t *ring_commitments, size_t n_rings, const uint32_t *ring_of_item,
                                    const uint8_t *instances_xy, const uint8_t *ring_proofs, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) {
  if (!su || su->g2_raw.empty() || (n && (!ring_commitments || !n_rings || !instances_xy || !ring_proofs)) || (n_seg && !status_out)) return AVRF_ERR_BAD_ARG;
  if (avrf_ctx_busy_(su->ctx)) return AVRF_ERR_BAD_ARG;
  RingSegLayout lay;
  if (int st = ring_segments_layout(n, n_seg, seg_items, lay)) return st;
  for (size_t i = 0; ring_of_item && i < n; i++) if (ring_of_item[i] >= n_rings) return AVRF_ERR_BAD_ARG;
  if (hipSetDevice(su->device) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  return guarded([&] {
    return with_ring(su->suite, [&](auto r) { return r.verify_segments(su, n, ring_commitments, ring_of_item, n_rings, instances_xy, ring_proofs, lay, status_out); }); });
}
int avrf_ring_segments_layout(size_t n, size_t n_seg, const uint32_t *seg_items, uint64_t out[4]) {
  if (!out) return AVRF_ERR_BAD_ARG;
  RingSegLayout lay;
  if (int st = ring_segments_layout(n, n_seg, seg_items, lay)) return st;
  out[0] = lay.L; out[1] = lay.rounds; out[2] = lay.padded; out[3] = lay.c;
  return AVRF_OK;
}
// test probe: the two G1 sums the last segmented call on this setup formed for segment `seg` (all-zero: infinity, an empty segment or
// one the host part had condemned before any sum was formed)
int avrf_ring_segment_sums(avrf_ring_setup *su, size_t seg, uint8_t *a_xy, uint8_t *b_xy) {
  if (!su || !a_xy || !b_xy || seg >= su->seg_sums_n) return AVRF_ERR_BAD_ARG;
  const size_t e1 = su->seg_sums.size() / (2 * su->seg_sums_n);
  memcpy(a_xy, &su->seg_sums[2 * seg * e1], e1); memcpy(b_xy, &su->seg_sums[(2 * seg + 1) * e1], e1);
  return AVRF_OK;
}

}  // extern "C"
