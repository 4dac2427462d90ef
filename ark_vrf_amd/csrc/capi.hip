// capi.hip -- the C ABI of libavrf.so (include/avrf.h): contexts, staging, orchestration.
//
// Host-side counterpart of the reference's scheme layer for the accelerated path
// (src/thin.rs:188-326 BatchVerifier; src/pedersen.rs:303-426).  All group/field work is
// launched on the context's HIP stream; the host only (1) runs the sequential weight
// transcript (host_sha512.h), (2) finishes the MSM's O(256)-step window Horner (host_te.h).
#include "capi_internal.h"
#include "host_sha512.h"
#include "host_shake128.h"
#include "host_sha256.h"
#include "host_sha512_mb.h"
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include "proto_dev.h"
#include "vrf_batch.h"
#include "thin_shared.h"
#include "thin_seg.h"
#include "host_pool.h"
#include "suite_dispatch.h"
#include <chrono>
#include <optional>
#include <stdlib.h>
#include <string.h>

using namespace avrf;

namespace avrf {
double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace avrf

// A run opened by avrf_batch_run_begin owns the context's stream, staged buffers and MSM workspace until avrf_batch_run_end
// (or an error) closes it: every other entry point that touches them refuses with AVRF_ERR_BAD_ARG meanwhile (include/avrf.h;
// ctx_busy, capi_internal.h).

// fixed-base tables for the provers: built once per context, on the context's stream
static int ensure_fixed(avrf_ctx *c) {
  if (c->fixed_ready) return AVRF_OK;
  if (c->d_fixed.ensure((size_t)2 * 32 * 256 * sizeof(te_pre_raw)) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  AVRF_SINGLE(c->suite, fixed_table(c->d_fixed.as<te_pre_raw>(), c->stream));
  c->fixed_ready = true;
  return AVRF_OK;
}

static BatchDev batch_of(avrf_ctx *c) {
  BatchDev b;
  b.pks_xy = c->d_pks.as<uint8_t>(); b.ios_xy = c->d_ios.as<uint8_t>(); b.io_off = c->d_io_off.as<uint32_t>();
  b.ads = c->d_ads.as<uint8_t>(); b.ad_off = c->d_ad_off.as<uint32_t>(); b.proofs = c->d_proofs.as<uint8_t>();
  b.sks = c->d_sks.as<uint8_t>(); b.n = (uint32_t)c->n;
  b.fixed = (const te_pre *)c->d_fixed.p;
  b.tabs = (te_ext *)c->d_tabs.p; b.first = 0;     // per-item window tables (sized by per_item_chunks)
  b.weights = nullptr; b.records = nullptr;
  return b;
}

// The independent per-item kernels (vrf_single.hip) keep ITEM_TAB_SLOTS window-table entries of 128 bytes per item (5 KB) in
// the context's workspace.  A call of any size walks its items in chunks of at most ITEM_CHUNK (two residency rounds of the
// chip: 65 536 lanes at one wave per SIMD), launched back to back on the context's stream, so the workspace is bounded by
// ITEM_CHUNK x 5 KB = 671 MB whatever n is; `launch` receives the BatchDev of one chunk (first .. n).
static constexpr size_t ITEM_CHUNK = 131072;
template <class F> static int per_item_chunks(avrf_ctx *c, bool with_pks, F launch) {
  if (int fs = ensure_fixed(c)) return fs;
  const size_t chunk = c->n < ITEM_CHUNK ? c->n : ITEM_CHUNK;
  if (c->d_tabs.ensure(chunk * (size_t)ITEM_TAB_SLOTS * sizeof(te_ext_raw)) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  BatchDev b = batch_of(c);
  if (!with_pks) b.pks_xy = nullptr;
  for (size_t i = 0; i < c->n; i += chunk) {
    b.first = (uint32_t)i; b.n = (uint32_t)(c->n - i < chunk ? c->n : i + chunk);
    launch(b);
  }
  return AVRF_OK;
}

// Validate::Yes over every point of the staged batch (pk, I/O pairs, proof points) when the context asks for it;
// rec_status (device, n x int32) receives 2 for items with a bad point (per-item verifiers), else NULL.
// n0, a0 (a chunk pushed to an open batch, without rec_status): only the items from n0 and the pairs from a0 on.
static void validate_staged(avrf_ctx *c, int kind, int32_t *d_rec_status, size_t n0 = 0, size_t a0 = 0) {
  if (c->validate <= 0 || c->n <= n0) return;
  uint32_t *fl = c->d_flags.as<uint32_t>();
  const uint32_t n = (uint32_t)(c->n - n0);
  const KindFacts &k = kind_facts(kind);
  if (c->n_shared && !d_rec_status) {                                  // a shared table: every row once, not once per reference; the outputs where they were gathered
    // (a status per item is wanted by the per-item calls, which restage through ctx_stage and so never see a shared staging, and by the
    // attribution pass of a segmented run, which takes the plain route below over the rows as shared_plan gathered them)
    AVRF_SINGLE(c->suite, validate_xy(c->d_table.as<uint8_t>(), 64, 1, (uint32_t)c->n_shared, c->validate, fl, nullptr, c->stream));
    AVRF_SINGLE(c->suite, validate_xy(c->d_ios.as<uint8_t>() + 64, 128, 1, (uint32_t)c->tot_io, c->validate, fl, nullptr, c->stream));
    AVRF_SINGLE(c->suite, validate_xy(c->d_proofs.as<uint8_t>(), (uint32_t)k.xy_proof(), (uint32_t)k.points, n, c->validate, fl, nullptr, c->stream));
    return;
  }
  if (k.pk && c->d_pks.p) AVRF_SINGLE(c->suite, validate_xy(c->d_pks.as<uint8_t>() + 64 * n0, 64, 1, n, c->validate, fl, d_rec_status, c->stream));
  if (k.points) AVRF_SINGLE(c->suite, validate_xy(c->d_proofs.as<uint8_t>() + k.xy_proof() * n0, (uint32_t)k.xy_proof(), (uint32_t)k.points, n, c->validate, fl, d_rec_status, c->stream));
  if (c->tot_io > a0) {
    if (!d_rec_status) AVRF_SINGLE(c->suite, validate_xy(c->d_ios.as<uint8_t>() + 128 * a0, 128, 2, (uint32_t)(c->tot_io - a0), c->validate, fl, nullptr, c->stream));
    else {   // per-item status: the I/O pairs of item j are records io_off[j] .. io_off[j+1]; uniform M = 1 is the common case
      const uint32_t *io_off = c->h_io.as<uint32_t>();
      bool uniform = c->tot_io == c->n;
      for (size_t j = 0; uniform && j < c->n; j++) uniform = io_off[j] == j;
      if (uniform) AVRF_SINGLE(c->suite, validate_xy(c->d_ios.as<uint8_t>(), 128, 2, n, c->validate, fl, d_rec_status, c->stream));
      else AVRF_SINGLE(c->suite, validate_xy(c->d_ios.as<uint8_t>(), 128, 2, (uint32_t)c->tot_io, c->validate, fl, d_rec_status, c->stream,
                                             c->d_io_off.as<uint32_t>(), n));     // one launch: every lane looks its item up in the staged offsets
    }
  }
}

namespace avrf {
int ctx_create(int suite, int device, bool lane_owner, avrf_ctx **out) {
  if (!out || suite < 0 || suite >= AVRF_N_SUITES) return AVRF_ERR_BAD_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return AVRF_ERR_NO_DEVICE;
  HIP_TRY(hipSetDevice(device));
  avrf_ctx *c = new avrf_ctx();
  c->suite = suite; c->device = device; c->lane_owner = lane_owner;
  if (lane_owner) {
    if (hipStreamCreateWithFlags(&c->own.stream, hipStreamNonBlocking) != hipSuccess) { delete c; return AVRF_ERR_NO_DEVICE; }
    c->stream = c->own.stream;
  }
  if (c->d_flags.ensure(64) != hipSuccess || c->h_flags.ensure(64) != hipSuccess) { avrf_ctx_destroy(c); return AVRF_ERR_NO_DEVICE; }
  *out = c;
  return AVRF_OK;
}
}  // namespace avrf

extern "C" {

int avrf_ctx_set_validation(avrf_ctx *c, int level) {
  if (!c || level < 0 || level > 2) return AVRF_ERR_BAD_ARG;
  c->validate = level;
  return AVRF_OK;
}

// accessors for the other translation units of the library (ring.hip)
hipStream_t avrf_ctx_stream_(avrf_ctx *c) { return c->stream; }
int avrf_ctx_suite_(avrf_ctx *c) { return c->suite; }
int avrf_ctx_device_(avrf_ctx *c) { return c->device; }
int avrf_ctx_busy_(avrf_ctx *c) { return c && ctx_busy(c); }

const char *avrf_version(void) { return "avrf 0.3 (gfx950; tiny/thin/pedersen/ring VRF over Bandersnatch, Baby-JubJub, JubJub; device pairing)"; }

int avrf_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int avrf_device_set_blocking_sync(int device, int on) {
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return AVRF_ERR_NO_DEVICE; }
  const hipError_t e = hipSetDeviceFlags(on ? hipDeviceScheduleBlockingSync : hipDeviceScheduleAuto);
  (void)hipSetDevice(prev);
  if (e != hipSuccess) (void)hipGetLastError();          // the runtime's last-error slot is sticky: later calls of this thread poll it
  return e == hipSuccess ? AVRF_OK : AVRF_ERR_NO_DEVICE;
}

int avrf_ctx_create(int suite, int device, avrf_ctx **out) { return ctx_create(suite, device, true, out); }

void avrf_ctx_destroy(avrf_ctx *c) {
  if (!c) return;
  delete c;                                                            // (~avrf_ctx, capi_internal.h: the order things go in)
}

}  // extern "C"
// A call into the MSM engine (msm.h): what the engine refuses is AVRF_ERR_BAD_ARG, a failed HIP call or allocation AVRF_ERR_NO_DEVICE (guarded).
template <class F> static int msm_guarded(F f) { return guarded([&] { return f() ? (int)AVRF_ERR_BAD_ARG : 0; }); }
// MSM over the first n terms of the context's lane (c->L->d_pre, c->L->d_scalars) on its stream, waited for
static int lane_msm(avrf_ctx *c, size_t n, HostExt *r) {
  return msm_guarded([&] { return msm_te_device(c->suite, c->L->d_pre.as<te_pre_raw>(), c->L->d_scalars.as<uint32_t>(), n, c->L->ws, c->stream, r); });
}
// the same for nv scalar vectors over the lane's first n bases through the single-launch form (msm.h msm_te_small_vectors): r[v]
static int lane_msm_vectors(avrf_ctx *c, size_t n, size_t nv, HostExt *r) {
  return msm_guarded([&] { return msm_te_small_vectors(c->suite, c->L->d_pre.as<te_pre_raw>(), c->L->d_scalars.as<uint32_t>(), n, nv, c->L->ws, c->stream, r); });
}
// n_seg independent MSMs of L terms each over arrays of the context's, through the segmented chain (msm.h msm_te_segments): sums[v]
static int lane_msm_segments(avrf_ctx *c, const DevBuf &d_pre, const DevBuf &d_scalars, size_t L, size_t n_seg, HostExt *sums) {
  return msm_guarded([&] { return msm_te_segments(c->suite, d_pre.as<te_pre_raw>(), d_scalars.as<uint32_t>(), L, n_seg, c->L->ws, c->stream, sums); });
}
extern "C" {

static int finish_point(avrf_ctx *c, const HostExt &r, uint8_t out_xy[64]) {
  with_suite(c->suite, [&](auto tag) { using S = typename decltype(tag)::type; HostTe<S>::to_affine_bytes(r, out_xy); });
  return AVRF_OK;
}
static bool point_is_identity(avrf_ctx *c, const HostExt &r) {
  return with_suite(c->suite, [&](auto tag) { using S = typename decltype(tag)::type; return HostTe<S>::is_identity(r); });
}
static bool scalar_in_range(int suite, const uint8_t *s) {
  H256 v; memcpy(v.l, s, 32);
  return with_suite(suite, [&](auto tag) { using S = typename decltype(tag)::type; return !HostField<typename S::Fr>::geq_p(v); });
}

// n affine bases into d_misc, the scalars into the lane's array, the input flag cleared (avrf_msm_te, _mont, avrf_scalar_mul's few-points route)
static int upload_bases_and_scalars(avrf_ctx *c, size_t n, const uint8_t *bases_xy, const uint8_t *scalars, size_t scalar_bytes) {
  HIP_TRY(c->d_misc.ensure(n * 64)); HIP_TRY(c->L->d_scalars.ensure(scalar_bytes)); HIP_TRY(c->L->d_pre.ensure(n * sizeof(te_pre_raw)));
  HIP_TRY(hipMemcpyAsync(c->d_misc.p, bases_xy, n * 64, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->L->d_scalars.p, scalars, scalar_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_flags.p, 0, 4, c->stream));
  return AVRF_OK;
}

// avrf_msm_te, and (`mont`) the same MSM on arkworks' IN-MEMORY values (SURVEY.md 8b "zero-copy option"): bases = n x Affine { x, y }
// with each coordinate an Fp<MontBackend, 4> (four little-endian u64 limbs, Montgomery form R = 2^256), scalars = n x ScalarField in
// the same form -- what `msm_unchecked(&[Affine], &[ScalarField])` is handed (src/thin.rs:319) -- and the result as Montgomery x || y.
// The canonical <-> Montgomery conversions of avrf_msm_te disappear on the host side; the device converts the scalars (one
// multiplication each, range-checked there) and takes the bases as they are.
static int msm_te_call(avrf_ctx *c, size_t n, const uint8_t *bases_xy, const uint8_t *scalars, uint8_t out_xy[64], bool mont) {
  if (!c || !out_xy || (n && (!bases_xy || !scalars))) return AVRF_ERR_BAD_ARG;
  if (ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  for (size_t i = 0; !mont && i < n; i++) if (!scalar_in_range(c->suite, scalars + 32 * i)) return AVRF_INVALID_DATA;
  HostExt r;
  if (n) {
    if (int e = upload_bases_and_scalars(c, n, bases_xy, scalars, n * 32)) return e;
    launch_pre_from_affine(c->suite, c->d_misc.as<uint8_t>(), n, c->L->d_pre.as<te_pre_raw>(), c->d_flags.as<uint32_t>(), 0, c->stream, mont);
    if (mont) launch_scalars_from_mont(c->suite, c->L->d_scalars.as<uint32_t>(), n, c->d_flags.as<uint32_t>(), c->stream);
    HIP_TRY(hipMemcpyAsync(c->h_flags.p, c->d_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
  }
  c->staged_kind = 0;
  if (int e = lane_msm(c, n, &r)) return e;
  if (n && *c->h_flags.as<uint32_t>()) return AVRF_INVALID_DATA;
  finish_point(c, r, out_xy);
  if (mont) with_suite(c->suite, [&](auto tag) { using S = typename decltype(tag)::type; using Fq = HostField<typename S::Fq>;
    Fq::store_le(out_xy, Fq::to_mont(Fq::load_le(out_xy))); Fq::store_le(out_xy + 32, Fq::to_mont(Fq::load_le(out_xy + 32))); });
  return AVRF_OK;
}
int avrf_msm_te(avrf_ctx *c, size_t n, const uint8_t *bases_xy, const uint8_t *scalars, uint8_t out_xy[64]) { return msm_te_call(c, n, bases_xy, scalars, out_xy, false); }
int avrf_msm_te_mont(avrf_ctx *c, size_t n, const uint8_t *bases_mont_xy, const uint8_t *scalars_mont, uint8_t out_mont_xy[64]) { return msm_te_call(c, n, bases_mont_xy, scalars_mont, out_mont_xy, true); }

// G1 MSM of the suite's pairing curve (KZG commit / open): bases as canonical little-endian x || y
// (48+48 bytes BLS12-381, 32+32 bytes BN254; all-zero = infinity), scalars LE32 < r.
int avrf_g1_msm(avrf_ctx *c, size_t n, const uint8_t *bases_xy, const uint8_t *scalars, uint8_t *out_xy) {
  if (!c || !out_xy || (n && (!bases_xy || !scalars))) return AVRF_ERR_BAD_ARG;
  if (ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  const int curve = pairing_curve_of(c->suite);
  const size_t fqb = curve == 0 ? 48 : 32;
  for (size_t i = 0; i < n; i++) {
    H256 v; memcpy(v.l, scalars + 32 * i, 32);
    bool ok = curve == 0 ? !HostField<FqBandersnatch>::geq_p(v) : !HostField<FqBabyJubJub>::geq_p(v);   // Fr of the pairing curve
    if (!ok) return AVRF_INVALID_DATA;
  }
  c->staged_kind = 0;
  if (n) {
    HIP_TRY(c->d_misc.ensure(n * 2 * fqb)); HIP_TRY(c->L->d_scalars.ensure(n * 32)); HIP_TRY(c->L->d_pre.ensure(n * 2 * fqb));
    HIP_TRY(hipMemcpyAsync(c->d_misc.p, bases_xy, n * 2 * fqb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->L->d_scalars.p, scalars, n * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_flags.p, 0, 4, c->stream));
    launch_g1_bases(curve, c->d_misc.as<uint8_t>(), n, c->L->d_pre.as<uint32_t>(), c->d_flags.as<uint32_t>(), c->stream);
    HIP_TRY(hipMemcpyAsync(c->h_flags.p, c->d_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (int e = msm_guarded([&] { return msm_g1_device(curve, c->L->d_pre.as<uint32_t>(), c->L->d_scalars.as<uint32_t>(), n, c->L->ws, c->stream, out_xy); })) return e;
  if (n && *c->h_flags.as<uint32_t>()) return AVRF_INVALID_DATA;
  return AVRF_OK;
}
// n_seg independent <E::G1 as VariableBaseMSM>::msm calls of L terms each (segment v: bases and scalars [v L, v L + L)) as ONE launch
// chain with the Horner and the affine conversion on the device (msm.h msm_g1_segments), for every n_seg >= 1: the probe of that chain.
int avrf_g1_msm_segments(avrf_ctx *c, size_t n_seg, size_t L, const uint8_t *bases_xy, const uint8_t *scalars, uint8_t *out_xy) {
  if (!c || (n_seg && !out_xy) || (n_seg && L && (!bases_xy || !scalars))) return AVRF_ERR_BAD_ARG;
  if (ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  if (L > (size_t)AVRF_SEGMENT_TERMS_MAX || n_seg > 0x0fffffffULL) return AVRF_ERR_BAD_ARG;
  const int curve = pairing_curve_of(c->suite);
  const size_t fqb = curve == 0 ? 48 : 32, n = n_seg * L;
  if (!n) { if (n_seg) memset(out_xy, 0, n_seg * 2 * fqb); return AVRF_OK; }
  if (n > (size_t)AVRF_SEGMENTS_PADDED_TERMS_MAX || n_seg * (size_t)msm_g1_segments_windows(curve, L) > (size_t)AVRF_SEGMENTS_WINDOWS_MAX) return AVRF_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  for (size_t i = 0; i < n; i++) {
    H256 v; memcpy(v.l, scalars + 32 * i, 32);
    bool ok = curve == 0 ? !HostField<FqBandersnatch>::geq_p(v) : !HostField<FqBabyJubJub>::geq_p(v);   // Fr of the pairing curve
    if (!ok) return AVRF_INVALID_DATA;
  }
  c->staged_kind = 0;
  HIP_TRY(c->d_misc.ensure(n * 2 * fqb)); HIP_TRY(c->L->d_scalars.ensure(n * 32)); HIP_TRY(c->L->d_pre.ensure(n * 2 * fqb));
  HIP_TRY(hipMemcpyAsync(c->d_misc.p, bases_xy, n * 2 * fqb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->L->d_scalars.p, scalars, n * 32, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_flags.p, 0, 4, c->stream));
  launch_g1_bases(curve, c->d_misc.as<uint8_t>(), n, c->L->d_pre.as<uint32_t>(), c->d_flags.as<uint32_t>(), c->stream);
  HIP_TRY(hipMemcpyAsync(c->h_flags.p, c->d_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
  if (int e = msm_guarded([&] { return msm_g1_segments(curve, c->L->d_pre.as<uint32_t>(), c->L->d_scalars.as<uint32_t>(), L, n_seg, c->L->ws, c->stream, out_xy); })) return e;
  if (*c->h_flags.as<uint32_t>()) return AVRF_INVALID_DATA;
  return AVRF_OK;
}

// ---------------------------------------------------------------- staging

}  // extern "C"
namespace avrf {
// HOST_WEIGHTS is exactly "the transcript is not the counter-mode SHA-512 one" (run_hash squeezes a sponge's or SHA-256's stream)
template <class... S> constexpr bool host_weights_defined = ((S::HOST_WEIGHTS == (S::XOF_SHAKE || S::TR_SHA256)) && ...);
static_assert(host_weights_defined<SuiteBandersnatch, SuiteBabyJubJub, SuiteJubJub, SuiteEd25519, SuiteBandersnatchSW, SuiteBandersnatchShake, SuiteTesting, SuiteSecp256r1>);
bool suite_host_weights(int suite) { return with_suite(suite, [&](auto tag) { using S = typename decltype(tag)::type; return (bool)S::HOST_WEIGHTS; }); }

// The weight transcript (src/thin.rs:274-279, src/pedersen.rs:361-367): new(SUITE_ID); absorb [0x50]; per item absorb LE32(c) || LE32(s)
// [|| LE32(sb)] -- the message  prefix || per item c(16) || 0(16) || resp(rsz)  into any hasher with update() (host_sha512_mb.h's lanes build the same bytes)
static size_t batch_prefix(int suite, uint8_t prefix[64]) {
  size_t pl = 0;
  with_suite(suite, [&](auto tag_) { using S = typename decltype(tag_)::type; memcpy(prefix, S::SUITE_ID, S::SUITE_ID_LEN); pl = S::SUITE_ID_LEN; });
  prefix[pl++] = DS_BATCH_VERIFY;
  return pl;
}
template <class H> static void absorb_weight_message(H &h, const uint8_t *prefix, size_t prefix_len, size_t n, const uint8_t *c16, const uint8_t *resp, size_t rsz) {
  h.update(prefix, prefix_len);
  uint8_t rec[96]; memset(rec, 0, sizeof rec);
  for (size_t k = 0; k < n; k++) { memcpy(rec, c16 + 16 * k, 16); memcpy(rec + 32, resp + rsz * k, rsz); h.update(rec, 32 + rsz); }
}
static void weight_digest_scalar(WeightJob &j) {
  HostSha512 h;
  if (j.msg) h.update(j.msg, j.msg_len); else absorb_weight_message(h, j.prefix, j.prefix_len, j.n, j.c16, j.resp, j.rsz);
  h.final(j.digest);
}
// several transcripts together: one through the scalar code, more through the widest multi-buffer form the host CPU has
void sha512_many(WeightJob *const *jobs, int k) {
  if (k == 1 || !sha512_mb_available()) { for (int i = 0; i < k; i++) weight_digest_scalar(*jobs[i]); }
  else if (sha512_mb16_available()) sha512_weights_x16(jobs, k);
  else for (int i = 0; i < k; i += 8) sha512_weights_x8(jobs + i, k - i < 8 ? k - i : 8);
}

// d_scalars / d_pre / d_gpart of the context's lane for the staged batch's n_terms
static int ensure_terms(avrf_ctx *c) {
  HIP_TRY(c->L->d_scalars.ensure(c->n_terms * 32)); HIP_TRY(c->L->d_pre.ensure(c->n_terms * sizeof(te_pre_raw))); HIP_TRY(c->L->d_gpart.ensure(((c->n + 127) / 128) * 64 + 64));
  if (c->n_shared) HIP_TRY(c->L->d_shared.ensure(shared_scratch_words(c->n_contrib) * 4));
  return AVRF_OK;
}

// off[0 .. n]: the prefix sums of n counts, the total into *total; false when the total is over `limit`
static bool prefix_sums(const uint32_t *counts, size_t n, uint32_t *off, uint64_t limit, uint64_t *total) {
  uint64_t a = 0;
  for (size_t j = 0; j < n; j++) { off[j] = (uint32_t)a; a += counts[j]; }
  off[n] = (uint32_t)a; *total = a;
  return a <= limit;
}

// The opening every flavour shares: argument checks (`args_ok`: the flavour's own), state reset, prefix sums of io_counts / ad_lens into h_io
// with their limits, offsets and `ads` copied -- and between them the I/O pairs when they come as x || y.  n == 0 stages the empty batch.
static int stage_open(avrf_ctx *c, int kind, size_t n, bool args_ok, const uint8_t *ios, bool ios_xy, const uint32_t *io_counts,
                      const uint8_t *ads, const uint32_t *ad_lens) {
  if (!c || ctx_busy(c) || !args_ok) return AVRF_ERR_BAD_ARG;    // (a run in flight owns the staged buffers)
  if (n && (!io_counts || !ad_lens)) return AVRF_ERR_BAD_ARG;
  if (n > 0x0fffffffULL) return AVRF_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  // An open batch ends here (include/avrf.h "Implicit close").  Its chunks may still be queued on the stream: copies up that read the
  // page-locked offsets in h_io, prepare kernels that take their loop bounds from them, copies back into h_msg / h_c / h_flags.  All of
  // that is rewritten below and by the run, so it is waited for first -- the one place a staging call waits before it has enqueued anything.
  if (!c->open.chunks.empty()) { HIP_TRY(hipStreamSynchronize(c->stream)); c->open.chunks.clear(); }
  c->staged_kind = 0; c->n = n; c->tot_io = 0; c->n_terms = 0; c->n_shared = 0; c->n_contrib = 0; c->stage_gen++; c->wire_pending = false;
  if (n == 0) { c->staged_kind = kind; return AVRF_OK; }
  HIP_TRY(c->h_io.ensure((n + 1) * 8));
  uint32_t *io_off = c->h_io.as<uint32_t>(), *ad_off = io_off + (n + 1);
  uint64_t a = 0, b = 0;
  if (!prefix_sums(io_counts, n, io_off, 0x1fffffffULL, &a) || !prefix_sums(ad_lens, n, ad_off, 0x7fffffffULL, &b)) return AVRF_ERR_BAD_ARG;
  if ((a && !ios) || (b && !ads)) return AVRF_ERR_BAD_ARG;
  c->tot_io = (size_t)a;
  HIP_TRY(c->d_io_off.ensure((n + 1) * 4)); HIP_TRY(c->d_ad_off.ensure((n + 1) * 4));
  HIP_TRY(c->d_ios.ensure(a * 128 + 16)); HIP_TRY(c->d_ads.ensure(b + 16));
  HIP_TRY(hipMemcpyAsync(c->d_io_off.p, io_off, (n + 1) * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_ad_off.p, ad_off, (n + 1) * 4, hipMemcpyHostToDevice, c->stream));
  if (ios_xy && a) HIP_TRY(hipMemcpyAsync(c->d_ios.p, ios, a * 128, hipMemcpyHostToDevice, c->stream));
  if (b) HIP_TRY(hipMemcpyAsync(c->d_ads.p, ads, b, hipMemcpyHostToDevice, c->stream));
  return AVRF_OK;
}
// The close every flavour shares for a batch VERIFIER: the host copy of the responses (item 0's at `resp`, `stride` apart) for a sponge
// transcript, which absorbs them on the host (counter-mode ones hash the device's records); the term count; the buffers the run writes.
// n0 (a chunk appended to an open batch): `resp` is item n0's; the buffers are the open batch's, grown before (open_grow), and the
// lane's term arrays are left to the run (run_launch), which knows the final count.
static int stage_verifier(avrf_ctx *c, int kind, const uint8_t *resp, size_t stride, bool append = false, size_t n0 = 0) {
  const size_t n = c->n, rsz = kind_facts(kind).resp;
  if (suite_host_weights(c->suite)) {
    c->h_resp.resize(n * rsz);
    for (size_t j = n0; j < n; j++) memcpy(&c->h_resp[rsz * j], resp + stride * (j - n0), rsz);
  }
  c->n_terms = c->n_shared ? shared_n_terms(kind, n, c->tot_io, c->n_shared) : n_terms(kind, n, c->tot_io);
  HIP_TRY(c->d_c.ensure(n * 16)); HIP_TRY(c->h_c.ensure(n * 16));
  HIP_TRY(c->d_z.ensure(z_bytes(kind, n, c->tot_io, c->n_shared != 0)));
  return c->lane_owner && !append ? ensure_terms(c) : (int)AVRF_OK;
}

bool shared_indices_ok(const BatchSource &s) {
  if (!s.n) return true;
  const bool keys = kind_facts(s.kind).pk;                             // (a Pedersen item has no key: input_index alone)
  if (!s.n_shared || s.n_shared > 0x0fffffffULL || s.n > 0x0fffffffULL || (keys && !s.pk_index) || !s.io_counts) return false;
  uint64_t a = 0; uint32_t over = 0;
  for (size_t j = 0; j < s.n; j++) { if (keys) over |= s.pk_index[j] >= s.n_shared; a += s.io_counts[j]; }
  if (over || a > 0x1fffffffULL || (a && (!s.input_index || !s.outputs))) return false;
  for (size_t k = 0; k < a; k++) over |= s.input_index[k] >= s.n_shared;
  return !over;
}

// What ctx_stage enqueues behind stage_open for a batch of n > 0 items, and its close.  The payload is the flavour's own:
//   x || y        keys, secrets and proofs (each where given) go to the buffers the kernels read;
//   wire          (src/thin.rs:78-94, src/pedersen.rs:106-134 deserialise, then `push`) the caller's serialize_compressed
//                 bytes go to d_misc as they are (keys | I/O points | proofs), every point is decompressed (validate: + not the identity,
//                 + prime-order subgroup, src/lib.rs:410-433) STRAIGHT INTO the staged x || y buffers and the proofs' scalars are copied
//                 beside their points -- no decompressed byte crosses PCIe or a host core;
//   shared        (thin_shared.h) the table, the indices, the outputs and the proofs go up; shared_plan gathers the rows into the plain
//                 staged layout and sorts the references by row, rows_pre converts each row once -- the host only checks the indices;
//   shared + wire rows | outputs | proofs go to d_misc and ONE kernel does all the decoding (vrf_single.hip k_decode_shared_wire): every
//                 row, referenced or not, once to d_table (x || y) and d_table_rows (te_pre, what rows_pre leaves), every output to
//                 d_table_outs, every R || s to d_proofs (Pedersen: k_decode_ped_shared_wire, Yb, R, Ok and s || sb of every proof).
//                 What decodes is canonical, so the plan's range flag stays clear.
//   A Pedersen source over a table has no keys: its references are the tot_io inputs alone (nk = 0 below; thin_shared.h "Pedersen").
// A wire point that fails raises the decode flag (d_status -> h_flags[2]): AVRF_INVALID_DATA here, before any equation (as the
// reference's deserialisation would), or from run_collect when nothing was waited for (wire_pending).  What a shared staging
// leaves is reused by every run of it (resident reruns, the pool's resubmission without host sources).
static int stage_payload(avrf_ctx *c, const BatchSource &s, bool wait) {
  const KindFacts &k = kind_facts(s.kind);
  const bool shared = s.n_shared != 0;
  const size_t n = s.n, n0 = s.n0, a0 = s.a0, a = c->tot_io - a0, nk = shared && k.pk ? n : 0, nc = nk + a, ns = s.n_shared, psz = k.xy_proof();   // nk: references to key rows; n0, a0: what an open batch holds already
  const size_t L = s.wire ? (size_t)point_len_of(c->suite) : 0, plen = k.wire_proof(L);
  const size_t w_pks = shared ? ns * L : k.pk ? n * L : 0, w_ios = shared ? a * L : 2 * a * L, w_pr = n * plen;   // the wire bytes in d_misc
  uint8_t *dw = nullptr; uint32_t *d_flag = nullptr, *h_flag = c->h_flags.as<uint32_t>() + 2, *plan = nullptr;
  if (shared) {
    HIP_TRY(c->d_table.ensure(ns * 64)); HIP_TRY(c->d_table_idx.ensure(nc * 4)); HIP_TRY(c->d_table_outs.ensure(a * 64 + 16));
    HIP_TRY(c->d_table_rows.ensure(ns * sizeof(te_pre_raw))); HIP_TRY(c->d_table_plan.ensure(shared_plan_words(ns, nc) * 4));
    plan = c->d_table_plan.as<uint32_t>();
  }
  if (shared || s.wire) { HIP_TRY(c->d_proofs.ensure((n0 + n) * psz)); if (k.pk) HIP_TRY(c->d_pks.ensure((n0 + n) * 64)); }
  if (s.wire) {
    HIP_TRY(c->d_misc.ensure(w_pks + w_ios + w_pr + 64)); HIP_TRY(c->d_status.ensure(64));
    // the decode flag: d_status word 0, cleared per staging; a chunk of an open batch ORs into the BATCH's flag instead, d_flags word 2,
    // cleared at open alone -- d_status is reused for the per-item statuses of a segmented run's attribution pass (run_collect)
    dw = c->d_misc.as<uint8_t>(); d_flag = s.append ? c->d_flags.as<uint32_t>() + 2 : c->d_status.as<uint32_t>();
  }
  auto up = [&](void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream); };
  if (shared && s.wire) {
    HIP_TRY(up(dw, s.table, w_pks));
    if (w_ios) HIP_TRY(up(dw + w_pks, s.outputs, w_ios));
    HIP_TRY(up(dw + w_pks + w_ios, s.proofs, w_pr));
    if (nk) HIP_TRY(up(c->d_table_idx.p, s.pk_index, nk * 4));
    if (a) HIP_TRY(up(c->d_table_idx.as<uint32_t>() + nk, s.input_index, a * 4));
  } else if (shared) {
    HIP_TRY(up(c->d_table.p, s.table, ns * 64));
    if (nk) HIP_TRY(up(c->d_table_idx.p, s.pk_index, nk * 4));
    if (a) { HIP_TRY(up(c->d_table_idx.as<uint32_t>() + nk, s.input_index, a * 4)); HIP_TRY(up(c->d_table_outs.p, s.outputs, a * 64)); }
    HIP_TRY(up(c->d_proofs.p, s.proofs, n * psz));
  } else if (s.wire) {
    if (w_pks) HIP_TRY(up(dw, s.pks, w_pks));
    if (w_ios) HIP_TRY(up(dw + w_pks, s.ios, w_ios));
    HIP_TRY(up(dw + w_pks + w_ios, s.proofs, w_pr));
  } else {
    if (s.pks) { HIP_TRY(c->d_pks.ensure((n0 + n) * 64)); HIP_TRY(up(c->d_pks.as<uint8_t>() + 64 * n0, s.pks, n * 64)); }
    if (s.sks) { HIP_TRY(c->d_sks.ensure(n * 32)); HIP_TRY(up(c->d_sks.p, s.sks, n * 32)); }
    if (s.proofs) { HIP_TRY(c->d_proofs.ensure((n0 + n) * psz)); HIP_TRY(up(c->d_proofs.as<uint8_t>() + psz * n0, s.proofs, n * psz)); }
  }
  if (s.wire && !s.append) HIP_TRY(hipMemsetAsync(d_flag, 0, 4, c->stream));
  if (shared) HIP_TRY(hipMemsetAsync(shared_plan_flag(plan, ns, nc), 0, 4, c->stream));
  if (s.wire) {
    const uint8_t *dpr = dw + w_pks + w_ios;
    if (shared && s.kind == Pedersen)
      HIP_TRY(AVRF_SINGLE(c->suite, decode_ped_shared_wire(dw, (uint32_t)ns, (uint32_t)a, (uint32_t)n, c->d_table.as<uint8_t>(), c->d_table_rows.as<te_pre_raw>(),
                                                           c->d_table_outs.as<uint8_t>(), c->d_proofs.as<uint8_t>(), s.validate, d_flag, c->stream)));
    else if (shared)
      HIP_TRY(AVRF_SINGLE(c->suite, decode_shared_wire(dw, (uint32_t)ns, (uint32_t)a, (uint32_t)n, c->d_table.as<uint8_t>(), c->d_table_rows.as<te_pre_raw>(),
                                                       c->d_table_outs.as<uint8_t>(), c->d_proofs.as<uint8_t>(), s.validate, d_flag, c->stream)));
    else {
      uint8_t *d_pr = c->d_proofs.as<uint8_t>() + psz * n0;
      if (k.pk) AVRF_SINGLE(c->suite, decompress_strided(dw, (uint32_t)L, (uint32_t)n, c->d_pks.as<uint8_t>() + 64 * n0, 64, s.validate, d_flag, c->stream));
      AVRF_SINGLE(c->suite, decompress_strided(dw + w_pks, (uint32_t)L, (uint32_t)(2 * a), c->d_ios.as<uint8_t>() + 128 * a0, 64, s.validate, d_flag, c->stream));
      for (size_t p = 0; p < k.points; p++)
        AVRF_SINGLE(c->suite, decompress_strided(dpr + L * p, (uint32_t)plen, (uint32_t)n, d_pr + 64 * p, (uint32_t)psz, s.validate, d_flag, c->stream));
      HIP_TRY(hipMemcpy2DAsync(d_pr + 64 * k.points, psz, dpr + L * k.points, plen, k.tail, n, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(h_flag, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (shared) {
    HIP_TRY(shared_plan(c->d_table.as<uint8_t>(), (uint32_t)ns, c->d_table_idx.as<uint32_t>(), c->d_table_outs.as<uint8_t>(), (uint32_t)nk, (uint32_t)a,
                        c->d_pks.as<uint8_t>(), c->d_ios.as<uint8_t>(), plan, c->stream));
    if (!s.wire) HIP_TRY(AVRF_SHARED(c->suite, rows_pre(c->d_table.as<uint8_t>(), (uint32_t)ns, c->d_table_rows.as<te_pre_raw>(), shared_plan_flag(plan, ns, nc), c->stream)));
    c->n_shared = ns; c->n_contrib = nc;
  }
  if (s.proofs && s.kind != Tiny)                                      // (Tiny has no batch verifier, and a prover stages no proofs)
    if (int e = stage_verifier(c, s.kind, s.proofs + (s.wire ? k.resp_at_wire(L) : k.resp_at_xy()), s.wire ? plen : psz, s.append, n0)) return e;
  if (s.wire && !wait) { c->wire_pending = true; return AVRF_OK; }
  if (wait) HIP_TRY(hipStreamSynchronize(c->stream));
  if (s.wire) { HIP_TRY(hipGetLastError()); if (*h_flag) return AVRF_INVALID_DATA; }
  return AVRF_OK;
}

// kind: a ProofKind (proof_kind.h: Thin pks + 96-byte proofs, Pedersen 256-byte proofs, Tiny 48).  wait = false (pool.hip): the copies are
// left in flight on c->stream -- from buffers of avrf_host_alloc they are DMA transfers that cost no host time; the caller's buffers must
// stay untouched until the batch's verdict is out.  The flavour's argument check refuses before anything staged is touched; every later
// failure leaves nothing staged (staged_kind == 0) and no shared table.
int ctx_stage(avrf_ctx *c, const BatchSource &s, bool wait) {
  const bool shared = s.n_shared != 0;
  const bool args_ok = (!s.wire || s.kind == Thin || s.kind == Pedersen) && (!shared || s.kind == Thin || s.kind == Pedersen) &&
                       (!s.n || (shared ? s.table && s.proofs && shared_indices_ok(s) : !s.wire || (s.proofs && (s.kind != Thin || s.pks))));
  if (int e = stage_open(c, s.kind, s.n, args_ok, shared ? s.outputs : s.ios, !shared && !s.wire, s.io_counts, s.ads, s.ad_lens)) return e;
  if (s.n == 0) return AVRF_OK;
  const int st = stage_payload(c, s, wait);
  if (st) c->n_shared = c->n_contrib = 0; else c->staged_kind = s.kind;
  return st;
}
}  // namespace avrf
extern "C" {
int avrf_thin_batch_stage_wire(avrf_ctx *c, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                               const uint32_t *ad_lens, const uint8_t *proofs, int validate) {
  if (!c || ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  return ctx_stage(c, wire_source(plain_source(Thin, n, pks, ios, io_counts, ads, ad_lens, proofs), validate), true);
}
int avrf_pedersen_batch_stage_wire(avrf_ctx *c, size_t n, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                                   const uint32_t *ad_lens, const uint8_t *proofs, int validate) {
  if (!c || ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  return ctx_stage(c, wire_source(plain_source(Pedersen, n, nullptr, ios, io_counts, ads, ad_lens, proofs), validate), true);
}

int avrf_thin_batch_stage_shared(avrf_ctx *c, size_t n, size_t n_shared, const uint8_t *shared_xy, const uint32_t *pk_index, const uint32_t *input_index,
                                 const uint8_t *outputs_xy, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs) {
  if (n && !n_shared) return AVRF_ERR_BAD_ARG;                         // (no table: a source with n_shared == 0 is a plain one)
  return ctx_stage(c, shared_source(Thin, n, n_shared, shared_xy, pk_index, input_index, outputs_xy, io_counts, ads, ad_lens, proofs), true);
}
size_t avrf_thin_shared_n_terms(size_t n, size_t tot_io, size_t n_shared) { return thin_shared_n_terms(n, tot_io, n_shared); }
int avrf_thin_batch_stage_shared_wire(avrf_ctx *c, size_t n, size_t n_shared, const uint8_t *shared, const uint32_t *pk_index, const uint32_t *input_index,
                                      const uint8_t *outputs, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs,
                                      int validate) {
  if (!c || ctx_busy(c) || (n && !n_shared)) return AVRF_ERR_BAD_ARG;
  return ctx_stage(c, wire_source(shared_source(Thin, n, n_shared, shared, pk_index, input_index, outputs, io_counts, ads, ad_lens, proofs), validate), true);
}
int avrf_thin_batch_verify_shared_wire(avrf_ctx *c, size_t n, size_t n_shared, const uint8_t *shared, const uint32_t *pk_index, const uint32_t *input_index,
                                       const uint8_t *outputs, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs,
                                       int validate) {
  if (int e = avrf_thin_batch_stage_shared_wire(c, n, n_shared, shared, pk_index, input_index, outputs, io_counts, ads, ad_lens, proofs, validate)) return e;
  return avrf_thin_batch_run(c);
}

// Pedersen over a table of shared inputs (include/avrf.h).  n_shared == 0 is a table nothing can refer to: legal exactly when no item has a
// pair, and then the batch IS a plain one (ped_no_pairs: every io_count 0) and is staged as one.
static bool ped_no_pairs(size_t n, const uint32_t *io_counts) {
  if (n && !io_counts) return false;
  uint32_t any = 0;
  for (size_t j = 0; j < n; j++) any |= io_counts[j];
  return !any;
}
int avrf_pedersen_batch_stage_shared(avrf_ctx *c, size_t n, size_t n_shared, const uint8_t *shared_xy, const uint32_t *input_index, const uint8_t *outputs_xy,
                                     const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs) {
  if (n && !proofs) return AVRF_ERR_BAD_ARG;
  if (n && !n_shared && !ped_no_pairs(n, io_counts)) return AVRF_ERR_BAD_ARG;
  return ctx_stage(c, shared_source(Pedersen, n, n_shared, shared_xy, nullptr, input_index, outputs_xy, io_counts, ads, ad_lens, proofs), true);
}
size_t avrf_pedersen_shared_n_terms(size_t n, size_t n_shared) { return ped_shared_n_terms(n, n_shared); }
int avrf_pedersen_batch_stage_shared_wire(avrf_ctx *c, size_t n, size_t n_shared, const uint8_t *shared, const uint32_t *input_index, const uint8_t *outputs,
                                          const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate) {
  if (!c || ctx_busy(c) || (n && !n_shared && !ped_no_pairs(n, io_counts))) return AVRF_ERR_BAD_ARG;
  return ctx_stage(c, wire_source(shared_source(Pedersen, n, n_shared, shared, nullptr, input_index, outputs, io_counts, ads, ad_lens, proofs), validate), true);
}
int avrf_pedersen_batch_verify_shared_wire(avrf_ctx *c, size_t n, size_t n_shared, const uint8_t *shared, const uint32_t *input_index, const uint8_t *outputs,
                                           const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate) {
  if (int e = avrf_pedersen_batch_stage_shared_wire(c, n, n_shared, shared, input_index, outputs, io_counts, ads, ad_lens, proofs, validate)) return e;
  return avrf_pedersen_batch_run(c);
}

int avrf_thin_batch_stage(avrf_ctx *c, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                          const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs) {
  if (n && (!pks_xy || !proofs)) return AVRF_ERR_BAD_ARG;
  return ctx_stage(c, plain_source(Thin, n, pks_xy, ios_xy, io_counts, ads, ad_lens, proofs), true);
}
int avrf_pedersen_batch_stage(avrf_ctx *c, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts,
                              const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs) {
  if (n && !proofs) return AVRF_ERR_BAD_ARG;
  return ctx_stage(c, plain_source(Pedersen, n, nullptr, ios_xy, io_counts, ads, ad_lens, proofs), true);
}

// ---- the weight transcripts of the contexts in flight, hashed together (host_sha512_mb.h)
namespace {
// OPT-IN (AVRF_HASH_THREADS = number of workers; default 0 = every context hashes its own transcript on its own thread).
// Contexts hand their transcript to a small pool; a worker takes up to eight pending ones and advances them in the eight lanes
// of a 512-bit register (a lone request goes through the scalar code).  Measured on the bench host (16-CPU quota): one 8-lane
// pass takes ~10 ms against 4.4 ms for one scalar chain, i.e. 3.6x the hashes per core-second but twice the latency per batch;
// the contexts form a closed loop, so with 16 of them the longer wait costs more than the saved cycles return (55-68 M/s with
// 2-4 workers against 76-81 M/s), and 48 contexts with 8 workers only draw level (74 M/s).  Kept for hosts with fewer cores per GPU.
class WeightHashService {
 public:
  static WeightHashService &get() { static WeightHashService s; return s; }
  bool enabled() const { return !workers_.empty(); }
  void run(WeightJob &job) {
    Item it{&job, false};
    std::unique_lock<std::mutex> lk(m_);
    q_.push_back(&it);
    cv_work_.notify_one();
    cv_done_.wait(lk, [&] { return it.done; });
  }
 private:
  struct Item { WeightJob *job; bool done; };
  WeightHashService() {
    int n = 0;
    if (const char *e = getenv("AVRF_HASH_THREADS")) n = atoi(e);
    if (n < 0) n = 0; if (n > 16) n = 16;
    if (!sha512_mb_available()) n = 0;
    for (int i = 0; i < n; i++) workers_.emplace_back([this] { loop(); });
  }
  ~WeightHashService() {
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
    cv_work_.notify_all();
    for (auto &t : workers_) t.join();
  }
  void loop() {
    for (;;) {
      Item *take[8]; int cnt = 0;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_work_.wait(lk, [&] { return stop_ || !q_.empty(); });
        if (stop_) return;
        if (q_.size() == 1) cv_work_.wait_for(lk, std::chrono::microseconds(40), [&] { return stop_ || q_.size() >= 2; });   // companions on their way?
        if (stop_) return;
        while (cnt < 8 && !q_.empty()) { take[cnt++] = q_.front(); q_.pop_front(); }
      }
      WeightJob *jobs[8];
      for (int i = 0; i < cnt; i++) jobs[i] = take[i]->job;
      sha512_many(jobs, cnt);
      { std::lock_guard<std::mutex> lk(m_); for (int i = 0; i < cnt; i++) take[i]->done = true; }
      cv_done_.notify_all();
    }
  }
  std::mutex m_; std::condition_variable cv_work_, cv_done_; std::deque<Item *> q_; std::vector<std::thread> workers_; bool stop_ = false;
};
}  // namespace

// The run of a staged batch, for both batch verifiers and both shapes -- the whole batch under one verdict, or n_seg groups with a
// verdict each (capi_internal.h: the record c->run and the phases run_begin .. run_end).  The run calls of the C ABI walk the phases:
// batch_run and run_segments wait between them; avrf_batch_run_begin / _hash / _end let one host thread keep several contexts in
// flight (hash one context's transcript while the others' kernels run) instead of parking a thread per context; the pool's workers
// (pool.hip) call the phases themselves and hash several contexts' transcripts together (run_messages / run_job / run_seed).
}  // extern "C"
namespace avrf {
static Seed64 seed_of(const uint8_t digest[64]) {
  Seed64 seed;
  for (int i = 0; i < 8; i++) { uint64_t v; memcpy(&v, digest + 8 * i, 8); seed.w[i] = __builtin_bswap64(v); }
  return seed;
}
// the kind's prepare kernel (challenges into d_c, the terms kernel's other inputs into d_z, the checks into d_flags) and terms kernel
// The run's check flags start clear -- or, over a shared table, from what staging found in it (a non-canonical coordinate in any row)
// (items_only: a segmented run, whose verdicts depend on the rows a segment REFERENCES -- the prepare kernel checks those where they were gathered)
static hipError_t reset_flags(avrf_ctx *c, bool items_only = false) {
  if (!c->n_shared || items_only) return hipMemsetAsync(c->d_flags.p, 0, 4, c->stream);
  return hipMemcpyAsync(c->d_flags.p, shared_plan_flag(c->d_table_plan.as<uint32_t>(), c->n_shared, c->n_contrib), 4, hipMemcpyDeviceToDevice, c->stream);
}
// rows_stay: the inputs of a Pedersen batch stay rows of the table (k_ped_prepare<S, true>: no merged input) -- every run of a shared
// staging but a segmented one in the expanded layout
static void launch_prepare(avrf_ctx *c, int kind, const BatchDev &b, bool rows_stay) {
  if (kind == Thin) AVRF_BATCH(c->suite, thin_prepare(b, c->d_c.as<uint32_t>(), c->d_z.as<uint32_t>(), c->d_flags.as<uint32_t>(), c->stream));
  else AVRF_BATCH(c->suite, ped_prepare(b, c->d_c.as<uint32_t>(), c->d_z.as<uint8_t>(), c->d_flags.as<uint32_t>(), rows_stay, c->stream));
}
static void launch_terms(avrf_ctx *c, int kind, const BatchDev &b, const Seed64 &seed, uint64_t first, uint32_t *d_scalars) {
  if (kind == Thin && c->n_shared)
    AVRF_SHARED(c->suite, thin_terms(b, seed, first, c->d_c.as<uint32_t>(), c->d_z.as<uint32_t>(),
                                     shared_plan_view(c->d_table_plan.as<uint32_t>(), c->d_table_rows.as<te_pre_raw>(), c->n_shared, c->n_contrib),
                                     (uint32_t)c->tot_io, c->L->d_shared.as<uint32_t>(), d_scalars, c->L->d_pre.as<te_pre_raw>(), c->L->d_gpart.as<uint32_t>(), c->stream));
  else if (kind == Thin) AVRF_BATCH(c->suite, thin_terms(b, seed, first, c->d_c.as<uint32_t>(), c->d_z.as<uint32_t>(), d_scalars,
                                                    c->L->d_pre.as<te_pre_raw>(), c->L->d_gpart.as<uint32_t>(), (uint32_t)c->n_terms, c->stream));
  else if (c->n_shared)
    AVRF_SHARED(c->suite, ped_terms(b, seed, first, c->d_c.as<uint32_t>(), c->d_z.as<uint8_t>(),
                                    shared_plan_view(c->d_table_plan.as<uint32_t>(), c->d_table_rows.as<te_pre_raw>(), c->n_shared, c->n_contrib),
                                    c->L->d_shared.as<uint32_t>(), d_scalars, c->L->d_pre.as<te_pre_raw>(), c->L->d_gpart.as<uint32_t>(), c->stream));
  else AVRF_BATCH(c->suite, ped_terms(b, seed, first, c->d_c.as<uint32_t>(), c->d_z.as<uint8_t>(), d_scalars,
                                      c->L->d_pre.as<te_pre_raw>(), c->L->d_gpart.as<uint32_t>(), (uint32_t)c->n_terms, c->stream));
}

// ---- open batches (include/avrf.h avrf_*_batch_open / _push / avrf_batch_flush): what the run phases need of them
// open: BatchVerifier::new was called on the context and nothing has staged on it, or dropped what is staged, since
static bool ctx_open(const avrf_ctx *c) { return c->open.kind && c->open.gen == c->stage_gen && c->staged_kind == c->open.kind; }
// The batch's decode flag (h_flags[2], cleared at open, copied back behind every wire chunk): a point that did not decode or failed
// `validate`.  The batch is then gone, as a failed avrf_*_batch_stage_wire leaves the context.
static int open_wire_failed(avrf_ctx *c) {
  if (!c->h_flags.as<uint32_t>()[2]) return AVRF_OK;
  c->staged_kind = 0; c->wire_pending = false;
  return AVRF_INVALID_DATA;
}
// The running weight transcript takes the records of the chunks whose copy back has completed, oldest first: found with an event
// query, never a wait (all: the caller has waited for c->stream, every chunk is complete).
static int open_poll(avrf_ctx *c, bool all) {
  avrf_ctx::OpenBatch &o = c->open;
  const KindFacts &k = kind_facts(o.kind);
  uint8_t prefix[64]; const size_t pl = batch_prefix(c->suite, prefix);
  const bool host_weights = suite_host_weights(c->suite);
  while (!o.chunks.empty()) {
    const avrf_ctx::OpenBatch::Chunk &ch = o.chunks.front();
    if (!all) {
      const hipError_t e = hipEventQuery(ch.done);
      if (e == hipErrorNotReady) { (void)hipGetLastError(); break; }    // (not an error: the slot later calls poll must stay clear)
      HIP_TRY(e);
    }
    if (host_weights) o.ws.absorb_parts(c->h_c.as<uint8_t>() + 16 * ch.n0, c->h_resp.data() + k.resp * ch.n0, ch.n, k.resp);
    else o.ws.absorb(c->h_msg.as<uint8_t>() + pl + k.record() * ch.n0, ch.n, k.record());
    o.absorbed = ch.n0 + ch.n;
    o.chunks.pop_front();
  }
  return open_wire_failed(c);
}

// a run with nothing to do -- no items, or no segments: every verdict is Ok and there is no device work at all
static bool run_nothing(const avrf_ctx *c) { return !c->n || (c->run.shape.segmented && !c->run.shape.n_seg); }

// The ONE place the prepare step is enqueued: over the staged items from `first` on (their pairs from a0 on) on c->stream, nothing
// waited for and no run opened.  The flag word restarts (reset; items_only as reset_flags) or keeps what an open batch's earlier chunks
// raised; validation; the kind's prepare kernel, which writes the transcript's records where the suite hashes them; the copies back:
// records into h_msg behind the prefix (sponge / SHA-256 suites: challenges into h_c) -- or, for avrf_*_batch_challenges, the challenges
// to challenges_out and no records at all -- and the flag word.
struct Prepare { bool reset = true, items_only = false, rows_stay = false; uint8_t *challenges_out = nullptr; };
static int enqueue_prepare(avrf_ctx *c, int kind, size_t first, size_t a0, const Prepare &p) {
  const size_t n = c->n, count = n - first, recsz = kind_facts(kind).record();
  const bool records = !p.challenges_out && !suite_host_weights(c->suite);
  BatchDev b = batch_of(c);
  b.first = (uint32_t)first;
  if (p.reset) HIP_TRY(reset_flags(c, p.items_only));
  validate_staged(c, kind, nullptr, first, a0);
  // the weight transcript's message, prefix || records: the prepare kernel writes the records, one copy brings them back
  uint8_t prefix[64]; const size_t pl = batch_prefix(c->suite, prefix);
  if (records) {
    HIP_TRY(c->d_rec.ensure(n * recsz)); HIP_TRY(c->h_msg.ensure(pl + n * recsz));   // (an open batch's have grown before: open_grow)
    b.records = c->d_rec.as<uint8_t>();
  }
  launch_prepare(c, kind, b, p.rows_stay);
  if (records) {
    memcpy(c->h_msg.p, prefix, pl);
    HIP_TRY(hipMemcpyAsync(c->h_msg.as<uint8_t>() + pl + first * recsz, c->d_rec.as<uint8_t>() + first * recsz, count * recsz, hipMemcpyDeviceToHost, c->stream));
    c->h_msg_len = pl + n * recsz;
  } else
    HIP_TRY(hipMemcpyAsync(p.challenges_out ? p.challenges_out : c->h_c.as<uint8_t>() + 16 * first, c->d_c.as<uint8_t>() + 16 * first, count * 16, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(c->h_flags.p, c->d_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
  return AVRF_OK;
}

// The weight transcript of a sponge / SHA-256 suite (Shake128Transcript: the weights are the sponge's OUTPUT STREAM, 16 bytes per item,
// 32 for Pedersen -- sequential, so the host squeezes it and the terms kernel reads it from HBM instead of deriving block j / 4 from a
// seed; HashTranscript<Sha256> of the test suite takes the same route) over `items` staged items from `first` -- one BatchVerifier's:
// absorbed from h_c / h_resp at `first`, squeezed into h_weights (sized by run_collect) at `first`; a segmented run calls it once per group.
static void squeeze_weights(avrf_ctx *c, int kind, size_t first, size_t items) {
  const KindFacts &k = kind_facts(kind);
  uint8_t prefix[64]; const size_t pl = batch_prefix(c->suite, prefix);
  with_suite(c->suite, [&](auto tag_) {
    using S = typename decltype(tag_)::type;
    std::conditional_t<S::XOF_SHAKE, HostShake128, HostSha256> h;
    absorb_weight_message(h, prefix, pl, items, c->h_c.as<uint8_t>() + 16 * first, c->h_resp.data() + k.resp * first, k.resp);
    h.squeeze_copy(c->h_weights.data() + k.weight * first, items * k.weight);
  });
}
}  // namespace avrf

// ---------------------------------------------------------------- open batches: BatchVerifier::new / push (src/thin.rs:199-243, src/pedersen.rs:316-326)
// A push copies its chunk to page-locked memory, restates stage_open for an append (checks, prefix sums continued from the totals,
// only the chunk's offsets up), hands the chunk to stage_payload as a source with a base, and enqueues the chunk's validation, the
// prepare kernel over [n0, n0 + n) and the copy back of that range's records (enqueue_prepare) -- all on c->stream, nothing waited
// for.  The run phases find that work done (run_begin), read the accumulated flags (run_collect) and finalise a clone of the running
// transcript (run_hash).

// One buffer of the open batch at `bytes` or more with its first `used` bytes kept: device memory copied on c->stream, the old buffer
// handed to `old` (the caller waits ONCE for all the copies before the old buffers go), page-locked host memory copied here.
static int open_keep(avrf_ctx *c, DevBuf &buf, size_t used, size_t bytes, std::vector<DevBuf> &old) {
  if (buf.p && bytes <= buf.cap) return AVRF_OK;
  DevBuf nb;
  HIP_TRY(nb.ensure(bytes));
  if (buf.p && used) HIP_TRY(hipMemcpyAsync(nb.p, buf.p, used < buf.cap ? used : buf.cap, hipMemcpyDeviceToDevice, c->stream));
  old.push_back(std::move(buf));                                       // (kept until the copy out of it has completed)
  buf = std::move(nb);
  return AVRF_OK;
}
static int open_keep(PinBuf &buf, size_t used, size_t bytes) {
  if (buf.p && bytes <= buf.cap) return AVRF_OK;
  PinBuf nb;
  HIP_TRY(nb.ensure(bytes));
  if (buf.p && used) memcpy(nb.p, buf.p, used < buf.cap ? used : buf.cap);
  buf = std::move(nb);
  return AVRF_OK;
}
// Room for `items` items, `pairs` pairs and `ad` bytes of additional data in every buffer a push writes, what was pushed kept.  Within
// the capacities nothing happens; beyond them they double, and the call WAITS for c->stream once first: copies back into the
// page-locked record buffer and copies up from the offsets may be in flight, and the buffers they use are about to move.
static int open_grow(avrf_ctx *c, size_t items, size_t pairs, size_t ad) {
  avrf_ctx::OpenBatch &o = c->open;
  const bool fresh = !c->h_msg.p || !c->h_io.p || !o.h_ad_off.p;      // (the first open on a context: even an empty batch has a prefix and offsets [0])
  if (items <= o.cap_items && pairs <= o.cap_pairs && ad <= o.cap_ad && !fresh) return AVRF_OK;
  auto grown = [](size_t need, size_t cap, size_t least) { return need <= cap ? cap : need > 2 * cap ? (need > least ? need : least) : 2 * cap; };
  const size_t ci = grown(items, o.cap_items, 256), cp = grown(pairs, o.cap_pairs, 256), ca = grown(ad, o.cap_ad, 1024);
  const KindFacts &k = kind_facts(o.kind);
  const size_t n = c->n, a = c->tot_io, recsz = k.record();
  uint8_t prefix[64]; const size_t pl = batch_prefix(c->suite, prefix);
  std::vector<DevBuf> old;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (k.pk) if (int e = open_keep(c, c->d_pks, n * 64, ci * 64, old)) return e;
  if (int e = open_keep(c, c->d_proofs, n * k.xy_proof(), ci * k.xy_proof(), old)) return e;
  if (int e = open_keep(c, c->d_ios, a * 128, cp * 128 + 16, old)) return e;
  if (int e = open_keep(c, c->d_ads, o.ad_bytes, ca + 16, old)) return e;
  if (int e = open_keep(c, c->d_io_off, (n + 1) * 4, (ci + 1) * 4, old)) return e;
  if (int e = open_keep(c, c->d_ad_off, (n + 1) * 4, (ci + 1) * 4, old)) return e;
  if (int e = open_keep(c, c->d_c, n * 16, ci * 16, old)) return e;
  if (int e = open_keep(c, c->d_z, z_bytes(o.kind, n, a), z_bytes(o.kind, ci, cp), old)) return e;
  if (int e = open_keep(c, c->d_rec, n * recsz, ci * recsz + 16, old)) return e;
  if (!old.empty()) HIP_TRY(hipStreamSynchronize(c->stream));          // the device-to-device copies: one wait for all of them
  old.clear();
  if (int e = open_keep(c->h_io, (n + 1) * 4, (ci + 1) * 4)) return e;
  if (int e = open_keep(o.h_ad_off, (n + 1) * 4, (ci + 1) * 4)) return e;
  if (int e = open_keep(c->h_msg, pl + n * recsz, pl + ci * recsz)) return e;
  if (int e = open_keep(c->h_c, n * 16, ci * 16 + 16)) return e;
  o.cap_items = ci; o.cap_pairs = cp; o.cap_ad = ca;
  return AVRF_OK;
}
// `bytes` of page-locked memory for a chunk's copy: from the current block, or from a new one twice as large -- a block never moves or
// goes while the batch is open, so the copies up that read it stay valid
static uint8_t *open_arena_take(avrf_ctx *c, size_t bytes) {
  avrf_ctx::OpenBatch &o = c->open;
  if (o.arena.empty() || o.arena_used + bytes > o.arena.back().cap) {
    size_t want = o.arena.empty() ? (size_t)1 << 20 : 2 * o.arena.back().cap;
    if (want < bytes) want = bytes;
    PinBuf nb;
    if (nb.ensure(want) != hipSuccess) return nullptr;
    o.arena.push_back(std::move(nb)); o.arena_used = 0;
  }
  uint8_t *p = o.arena.back().as<uint8_t>() + o.arena_used;
  o.arena_used += bytes;
  return p;
}
static bool open_limits_ok(size_t items, size_t pairs, size_t ad) { return items <= 0x0fffffffULL && pairs <= 0x1fffffffULL && ad <= 0x7fffffffULL; }   // stage_open's

static int batch_open(avrf_ctx *c, int kind, size_t items_hint, size_t pairs_hint, size_t ad_hint) {
  if (!c || ctx_busy(c) || !c->lane_owner || !open_limits_ok(items_hint, pairs_hint, ad_hint)) return AVRF_ERR_BAD_ARG;
  avrf_ctx::OpenBatch &o = c->open;
  // the reset every staging makes (n == 0: the empty batch of `kind` is staged)
  if (int e = stage_open(c, kind, 0, true, nullptr, false, nullptr, nullptr, nullptr)) return e;     // (waits for the chunks of an open batch it replaces)
  c->staged_kind = 0;                                                  // (until everything below has succeeded)
  o.kind = kind; o.ad_bytes = 0; o.absorbed = 0; o.cap_items = o.cap_pairs = o.cap_ad = 0;
  if (o.arena.size() > 1) { HIP_TRY(hipStreamSynchronize(c->stream)); o.arena.erase(o.arena.begin(), o.arena.end() - 1); }   // (the largest block stays)
  o.arena_used = 0;
  if (int e = open_grow(c, items_hint, pairs_hint, ad_hint)) return e;
  // (the chunks are packed without padding, so hints that are exact for the batch are exact for the arena however many pushes bring it;
  // x || y chunks: wire ones are smaller)
  const size_t hint_bytes = items_hint * ((kind_facts(kind).pk ? 64 : 0) + kind_facts(kind).xy_proof()) + pairs_hint * 128 + ad_hint;
  if (hint_bytes && (o.arena.empty() || o.arena.back().cap < hint_bytes)) {
    if (!o.arena.empty()) { HIP_TRY(hipStreamSynchronize(c->stream)); o.arena.clear(); }
    if (!open_arena_take(c, hint_bytes)) return AVRF_ERR_NO_DEVICE;
    o.arena_used = 0;
  }
  uint8_t prefix[64]; const size_t pl = batch_prefix(c->suite, prefix);
  with_suite(c->suite, [&](auto tag_) { using S = typename decltype(tag_)::type;
    o.ws.begin(S::XOF_SHAKE ? WeightStream::SHAKE128 : S::TR_SHA256 ? WeightStream::SHA256 : WeightStream::SHA512, prefix, pl); });
  memcpy(c->h_msg.p, prefix, pl); c->h_msg_len = pl;
  c->h_io.as<uint32_t>()[0] = 0; o.h_ad_off.as<uint32_t>()[0] = 0;
  c->h_resp.clear();
  c->h_flags.as<uint32_t>()[0] = 0; c->h_flags.as<uint32_t>()[2] = 0;
  // the flag word (d_flags word 0) is the batch's: OR-ed across the chunks, cleared here alone; so is the decode flag of its wire chunks, word 2
  HIP_TRY(hipMemsetAsync(c->d_flags.p, 0, 12, c->stream));
  o.gen = c->stage_gen; c->staged_kind = kind;
  return AVRF_OK;
}

// s: the caller's arrays of the chunk (plain_source / wire_source)
static int batch_push(avrf_ctx *c, BatchSource s) {
  if (!c || ctx_busy(c) || !ctx_open(c) || c->open.kind != s.kind) return AVRF_ERR_BAD_ARG;
  const size_t n = s.n;
  if (!n) return AVRF_OK;
  if (!s.io_counts || !s.ad_lens || !s.proofs || (s.kind == Thin && !s.pks)) return AVRF_ERR_BAD_ARG;
  avrf_ctx::OpenBatch &o = c->open;
  const KindFacts &k = kind_facts(s.kind);
  const size_t n0 = c->n, a0 = c->tot_io, b0 = o.ad_bytes;
  if (n > 0x0fffffffULL) return AVRF_ERR_BAD_ARG;
  uint64_t a = 0, b = 0;
  for (size_t j = 0; j < n; j++) { a += s.io_counts[j]; b += s.ad_lens[j]; }
  if (!open_limits_ok(n0 + n, a0 + a, b0 + b) || (a && !s.ios) || (b && !s.ads)) return AVRF_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  // the records of earlier chunks that have come back meanwhile go into the transcript now; a wire chunk that failed ends the batch
  if (int e = open_poll(c, /*all=*/false)) return e;
  if (int e = open_grow(c, n0 + n, a0 + a, b0 + b)) { c->staged_kind = 0; return e; }
  // the page-locked copy: keys | I/O points | proofs | additional data, back to back (the copies up need no alignment)
  const size_t L = s.wire ? (size_t)point_len_of(c->suite) : 0, plen = s.wire ? k.wire_proof(L) : k.xy_proof();
  const size_t sz_pks = k.pk ? n * (s.wire ? L : 64) : 0, sz_ios = s.wire ? 2 * a * L : a * 128, sz_pr = n * plen;
  uint8_t *pin = open_arena_take(c, sz_pks + sz_ios + sz_pr + b);
  if (!pin) { c->staged_kind = 0; return AVRF_ERR_NO_DEVICE; }
  uint8_t *p_pks = pin, *p_ios = p_pks + sz_pks, *p_pr = p_ios + sz_ios, *p_ads = p_pr + sz_pr;
  if (sz_pks) memcpy(p_pks, s.pks, sz_pks);
  if (sz_ios) memcpy(p_ios, s.ios, sz_ios);
  if (b) memcpy(p_ads, s.ads, b);
  memcpy(p_pr, s.proofs, sz_pr);
  uint32_t *io_off = c->h_io.as<uint32_t>() + n0, *ad_off = o.h_ad_off.as<uint32_t>() + n0;
  uint64_t ta = a0, tb = b0;
  for (size_t j = 0; j < n; j++) { io_off[j] = (uint32_t)ta; ad_off[j] = (uint32_t)tb; ta += s.io_counts[j]; tb += s.ad_lens[j]; }
  io_off[n] = (uint32_t)ta; ad_off[n] = (uint32_t)tb;
  // from here on a failure leaves nothing open or staged
  c->staged_kind = 0;
  auto up = [&](void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream); };
  HIP_TRY(up(c->d_io_off.as<uint32_t>() + n0, io_off, (n + 1) * 4));
  HIP_TRY(up(c->d_ad_off.as<uint32_t>() + n0, ad_off, (n + 1) * 4));
  if (!s.wire && a) HIP_TRY(up(c->d_ios.as<uint8_t>() + 128 * a0, p_ios, a * 128));
  if (b) HIP_TRY(up(c->d_ads.as<uint8_t>() + b0, p_ads, b));
  c->n = n0 + n; c->tot_io = a0 + (size_t)a; o.ad_bytes = b0 + (size_t)b;
  s.pks = k.pk ? p_pks : nullptr; s.ios = p_ios; s.ads = p_ads; s.proofs = p_pr;
  s.append = true; s.n0 = n0; s.a0 = a0;
  if (int e = stage_payload(c, s, /*wait=*/false)) return e;
  Prepare chunk; chunk.reset = false;                                   // (the flag word is the batch's, OR-ed across its chunks)
  if (int e = enqueue_prepare(c, s.kind, n0, a0, chunk)) return e;
  avrf_ctx::OpenBatch::Chunk ch; ch.n0 = n0; ch.n = n;
  HIP_TRY(ch.done.create(hipEventDisableTiming));
  HIP_TRY(hipEventRecord(ch.done, c->stream));
  o.chunks.push_back(std::move(ch));
  c->staged_kind = s.kind;
  return AVRF_OK;
}

extern "C" {

int avrf_thin_batch_open(avrf_ctx *c, size_t items_hint, size_t pairs_hint, size_t ad_bytes_hint) { return batch_open(c, Thin, items_hint, pairs_hint, ad_bytes_hint); }
int avrf_pedersen_batch_open(avrf_ctx *c, size_t items_hint, size_t pairs_hint, size_t ad_bytes_hint) { return batch_open(c, Pedersen, items_hint, pairs_hint, ad_bytes_hint); }
int avrf_thin_batch_push(avrf_ctx *c, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts, const uint8_t *ads,
                         const uint32_t *ad_lens, const uint8_t *proofs) {
  return batch_push(c, plain_source(Thin, n, pks_xy, ios_xy, io_counts, ads, ad_lens, proofs));
}
int avrf_thin_batch_push_wire(avrf_ctx *c, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                              const uint32_t *ad_lens, const uint8_t *proofs, int validate) {
  return batch_push(c, wire_source(plain_source(Thin, n, pks, ios, io_counts, ads, ad_lens, proofs), validate));
}
int avrf_pedersen_batch_push(avrf_ctx *c, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                             const uint8_t *proofs) {
  return batch_push(c, plain_source(Pedersen, n, nullptr, ios_xy, io_counts, ads, ad_lens, proofs));
}
int avrf_pedersen_batch_push_wire(avrf_ctx *c, size_t n, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                                  const uint8_t *proofs, int validate) {
  return batch_push(c, wire_source(plain_source(Pedersen, n, nullptr, ios, io_counts, ads, ad_lens, proofs), validate));
}
// waits for everything pushed, absorbs it, and reports what a wire chunk left: AVRF_INVALID_DATA, the batch gone
int avrf_batch_flush(avrf_ctx *c) {
  if (!c || ctx_busy(c) || !ctx_open(c)) return AVRF_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) { (void)hipGetLastError(); c->staged_kind = 0; return AVRF_ERR_NO_DEVICE; }
  return open_poll(c, /*all=*/true);
}
size_t avrf_batch_pushed(const avrf_ctx *c, size_t out[3]) {
  const bool open = c && ctx_open(c);
  if (out) { out[0] = open ? c->n : 0; out[1] = open ? c->tot_io : 0; out[2] = open ? c->open.ad_bytes : 0; }
  return open ? c->n : 0;
}

}  // extern "C"
extern "C" {

// between run_begin and run_collect: c->stream has drained (and_last_error: and nothing enqueued on it failed); a failure closes the run
static int run_wait(avrf_ctx *c, bool and_last_error) {
  if (hipStreamSynchronize(c->stream) == hipSuccess && (!and_last_error || hipGetLastError() == hipSuccess)) return AVRF_OK;
  (void)hipGetLastError(); run_close(c);
  return AVRF_ERR_NO_DEVICE;
}

// the second of the three calls: wait for the prepare kernel, hash on the calling thread, enqueue terms + MSM
static int batch_hash(avrf_ctx *c, int kind) {
  if (!c || c->staged_kind != kind || c->run.phase != RunPhase::Begun) return AVRF_ERR_BAD_ARG;
  double tw = 0, t1 = 0;
  if (!run_nothing(c)) {
    HIP_TRY(hipSetDevice(c->device));
    tw = now_us();
    if (int e = run_wait(c, false)) return e;
    t1 = now_us();
  }
  if (int e = run_collect(c, kind)) return e;
  if (int e = run_hash(c, kind, /*spread=*/false)) return e;
  if (!run_nothing(c)) { c->timing[1] = c->run.begin_us + (t1 - tw); c->timing[2] = now_us() - t1; }
  return run_launch(c, kind);
}
// the third: the run's one status is the call's
static int batch_end(avrf_ctx *c, int kind) {
  int32_t st = AVRF_OK;
  const int e = run_end(c, kind, &st);
  return e ? e : (int)st;
}

static int batch_run(avrf_ctx *c, int kind) {
  if (int e = run_begin(c, kind)) return e;
  if (int e = batch_hash(c, kind)) return e;
  return batch_end(c, kind);
}

int avrf_thin_batch_run(avrf_ctx *c) { return batch_run(c, Thin); }
int avrf_pedersen_batch_run(avrf_ctx *c) { return batch_run(c, Pedersen); }
// (defensive: a run can only be open on a staged batch -- every entry point that would un-stage it is refused while the context is
// busy -- but should the two ever disagree the run is closed rather than leaving the context refusing every call)
static int run_call(avrf_ctx *c, int (*phase)(avrf_ctx *, int)) {
  if (!c) return AVRF_ERR_BAD_ARG;
  if (!c->staged_kind) {
    if (ctx_busy(c)) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); run_close(c); c->chain().disarm(); }
    return AVRF_ERR_BAD_ARG;
  }
  return phase(c, c->staged_kind);
}
int avrf_batch_run_begin(avrf_ctx *c) { return run_call(c, [](avrf_ctx *ctx, int kind) { return run_begin(ctx, kind); }); }
int avrf_batch_run_hash(avrf_ctx *c) { return run_call(c, batch_hash); }
int avrf_batch_run_end(avrf_ctx *c) { return run_call(c, batch_end); }

int avrf_thin_batch_verify(avrf_ctx *c, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                           const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs) {
  int st = avrf_thin_batch_stage(c, n, pks_xy, ios_xy, io_counts, ads, ad_lens, proofs);
  return st ? st : avrf_thin_batch_run(c);
}
int avrf_pedersen_batch_verify(avrf_ctx *c, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts,
                               const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs) {
  int st = avrf_pedersen_batch_stage(c, n, ios_xy, io_counts, ads, ad_lens, proofs);
  return st ? st : avrf_pedersen_batch_run(c);
}

// ---------------------------------------------------------------- one verdict per segment of the staged Thin or Pedersen batch (thin_seg.h)
}  // extern "C"

// `count` MSM terms of the context's device back to the host, each where wanted: the bases as canonical x || y, the scalars as they are.
// Returns count, 0 when a copy failed.
static size_t terms_to_host(avrf_ctx *c, const te_pre_raw *d_pre, const uint8_t *d_scalars, size_t count, uint8_t *bases_xy, uint8_t *scalars) {
  if (scalars) { if (hipMemcpy(scalars, d_scalars, count * 32, hipMemcpyDeviceToHost) != hipSuccess) return 0; }
  if (bases_xy) {
    std::vector<te_pre_raw> pre(count);
    if (hipMemcpy(pre.data(), d_pre, count * sizeof(te_pre_raw), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    for (size_t i = 0; i < count; i++) {
      H256 x, y; memcpy(x.l, pre[i].w, 32); memcpy(y.l, pre[i].w + 8, 32);
      with_suite(c->suite, [&](auto tag) { using S = typename decltype(tag)::type; x = HostField<typename S::Fq>::from_mont(x); y = HostField<typename S::Fq>::from_mont(y); });
      memcpy(bases_xy + 64 * i, x.l, 32); memcpy(bases_xy + 64 * i + 32, y.l, 32);
    }
  }
  return count;
}

// The layout of n_seg BatchVerifiers of `kind` over consecutive runs of n staged items (include/avrf.h avrf_thin_segments_layout,
// avrf_pedersen_segments_layout): item offsets into *seg_off (n_seg + 1) when wanted, out = { L, n_seg L, sum of the term counts, window
// bits }; io_off: n + 1 prefix sums of the items' pair counts (Thin only: a Pedersen item has five terms whatever its pairs).
// AVRF_ERR_BAD_ARG when the counts do not sum to n or a limit is exceeded.
static int seg_limits(size_t n_seg, uint64_t L, uint64_t out[4]) {
  if (L > (uint64_t)AVRF_SEGMENT_TERMS_MAX || n_seg * L > (uint64_t)AVRF_SEGMENTS_PADDED_TERMS_MAX) return AVRF_ERR_BAD_ARG;
  const uint64_t c = L ? (uint64_t)msm_segments_window_bits(L) : 0;
  // (windows of a 256-bit scalar: no suite's are more; fewer than eight segments run one after the other, msm.h msm_te_segments)
  if (n_seg >= 8 && L && n_seg * ((257 + c - 1) / c) > (uint64_t)AVRF_SEGMENTS_WINDOWS_MAX) return AVRF_ERR_BAD_ARG;
  out[0] = L; out[1] = n_seg * L; out[3] = c;
  return AVRF_OK;
}
// Over a table of T = n_shared rows (avrf_thin_shared_segments_layout, avrf_pedersen_shared_segments_layout; 0: a plain staging) a segment
// has a second, MERGED layout -- its item terms (Thin items + pairs, Pedersen 4 items), then T row terms, then its base term(s) -- and the
// run takes it exactly when its padded length is the smaller one (a tie goes to the expanded layout, which needs no plan): out[4] = 1,
// and *row0 (when wanted) the term of each segment's row 0, SHARED_NO_ROW for an empty segment.  The limits apply to the chosen L.
static int seg_layout(int kind, size_t n, size_t n_shared, size_t n_seg, const uint32_t *seg_items, const uint32_t *io_off, std::vector<uint32_t> *seg_off,
                      std::vector<uint32_t> *row0, uint64_t out[5]) {
  if ((n_seg && !seg_items) || n_seg > 0x0fffffffULL || n_shared > 0x0fffffffULL || (kind == Thin && n && !io_off)) return AVRF_ERR_BAD_ARG;
  if (seg_off) seg_off->assign(n_seg + 1, (uint32_t)n);
  const uint64_t T = n_shared, nbase = kind == Thin ? 1 : 2;
  uint64_t at = 0, L = 0, total = 0, body = 0, total_m = 0;
  for (size_t v = 0; v < n_seg; v++) {
    const uint64_t items = seg_items[v];
    if (at + items > n) return AVRF_ERR_BAD_ARG;
    if (seg_off) (*seg_off)[v] = (uint32_t)at;
    const uint64_t pairs = kind == Thin && items ? io_off[at + items] - io_off[at] : 0;
    const uint64_t n_v = items ? n_terms(kind, items, pairs) : 0;    // none for an empty segment
    const uint64_t b_v = kind == Thin ? items + pairs : 4 * items;   // the item terms of the merged layout
    if (n_v > L) L = n_v;
    if (b_v > body) body = b_v;
    total += n_v; total_m += items ? b_v + T + nbase : 0; at += items;
  }
  if (at != n) return AVRF_ERR_BAD_ARG;
  const uint64_t L_m = body ? body + T + nbase : 0;
  const bool merged = T && L_m < L;
  out[2] = merged ? total_m : total; out[4] = merged;
  if (int e = seg_limits(n_seg, merged ? L_m : L, out)) return e;
  if (row0) {
    row0->clear();
    for (size_t v = 0; merged && v < n_seg; v++) {
      const uint64_t first = (*seg_off)[v], items = seg_items[v];
      row0->push_back(items ? (uint32_t)(v * L_m + (kind == Thin ? items + (io_off[first + items] - io_off[first]) : 4 * items)) : (uint32_t)SHARED_NO_ROW);
    }
  }
  return AVRF_OK;
}
static int seg_layout4(int kind, size_t n, size_t n_seg, const uint32_t *seg_items, const uint32_t *io_off, uint64_t out[4]) {
  uint64_t lay[5];
  const int st = seg_layout(kind, n, 0, n_seg, seg_items, io_off, nullptr, nullptr, lay);
  if (st == AVRF_OK) memcpy(out, lay, 4 * sizeof(uint64_t));
  return st;
}

extern "C" {

int avrf_thin_segments_layout(size_t n, size_t n_seg, const uint32_t *seg_items, const uint32_t *io_counts, uint64_t out[4]) {
  if (!out || (n && !io_counts) || n > 0x0fffffffULL) return AVRF_ERR_BAD_ARG;
  std::vector<uint32_t> io_off(n + 1); uint64_t a;
  if (!prefix_sums(io_counts, n, io_off.data(), 0x1fffffffULL, &a)) return AVRF_ERR_BAD_ARG;
  return seg_layout4(Thin, n, n_seg, seg_items, io_off.data(), out);
}
int avrf_pedersen_segments_layout(size_t n, size_t n_seg, const uint32_t *seg_items, uint64_t out[4]) {
  if (!out || n > 0x0fffffffULL) return AVRF_ERR_BAD_ARG;
  return seg_layout4(Pedersen, n, n_seg, seg_items, nullptr, out);
}
int avrf_thin_shared_segments_layout(size_t n, size_t n_shared, size_t n_seg, const uint32_t *seg_items, const uint32_t *io_counts, uint64_t out[5]) {
  if (!out || (n && !io_counts) || n > 0x0fffffffULL) return AVRF_ERR_BAD_ARG;
  std::vector<uint32_t> io_off(n + 1); uint64_t a;
  if (!prefix_sums(io_counts, n, io_off.data(), 0x1fffffffULL, &a)) return AVRF_ERR_BAD_ARG;
  return seg_layout(Thin, n, n_shared, n_seg, seg_items, io_off.data(), nullptr, nullptr, out);
}
int avrf_pedersen_shared_segments_layout(size_t n, size_t n_shared, size_t n_seg, const uint32_t *seg_items, uint64_t out[5]) {
  if (!out || n > 0x0fffffffULL) return AVRF_ERR_BAD_ARG;
  return seg_layout(Pedersen, n, n_shared, n_seg, seg_items, nullptr, nullptr, nullptr, out);
}
}  // extern "C"

// The segmented run of either batch verifier (include/avrf.h avrf_thin_batch_run_segments, avrf_pedersen_batch_run_segments).  What the
// kind decides: the record and weight sizes (kind_facts), the scratch per item, the terms and flags launches, n_terms in seg_layout.
// Where a segmented run's padded term arrays live.  A context keeps arrays of its own for them, so that the plain run's terms on its lane
// stay what they were (avrf_batch_last_terms, avrf_*_segment_terms).  A pool slot uses the term arrays of the lane it borrows, as a plain
// pool job does: a slot that held them itself would grow by padded x 128 bytes (134 MB at the limit, times every slot).  Several chains
// queue on one lane, and reusing the lane's arrays is safe for the reason it is safe for plain jobs: everything that writes and reads
// them -- the copies up, the zeroing, the terms kernel, the chain -- is enqueued on the lane's one stream, so the next job's writes run
// behind this job's last read; and an array that has to grow is freed by hipFree, which waits for the device first.
struct SegArrays { DevBuf &scalars, &pre; };
static SegArrays seg_arrays(avrf_ctx *c) { return c->lane_owner ? SegArrays{c->d_seg_scalars, c->d_seg_pre} : SegArrays{c->L->d_scalars, c->L->d_pre}; }
static int seg_ensure(avrf_ctx *c, int kind) {
  const RunShape &r = c->run.shape; const SegArrays a = seg_arrays(c);
  // (scratch per item: Thin's w s z0, Pedersen's u s and u sb)
  HIP_TRY(a.scalars.ensure(r.padded * 32)); HIP_TRY(a.pre.ensure(r.padded * sizeof(te_pre_raw))); HIP_TRY(c->L->d_seg_wsz.ensure(c->n * (kind == Thin ? 32 : 64)));
  HIP_TRY(c->L->d_seg_off.ensure((r.n_seg + 1) * 4)); HIP_TRY(c->L->d_seg_seeds.ensure(r.n_seg * sizeof(Seed64)));
  if (r.merged) {                                                      // the run's plan, and the scratch of the row sums (the plain shared run's, ensure_terms)
    HIP_TRY(c->d_seg_plan.ensure(shared_seg_plan_words(r.n_seg, c->n_shared, c->n_contrib) * 4));
    HIP_TRY(c->L->d_shared.ensure(shared_scratch_words(c->n_contrib) * 4));
  }
  return AVRF_OK;
}
static void launch_seg_terms(avrf_ctx *c, int kind, const BatchDev &b, size_t n_seg, size_t L) {
  const uint32_t *off = c->L->d_seg_off.as<uint32_t>(); const Seed64 *seeds = c->L->d_seg_seeds.as<Seed64>(); const SegArrays a = seg_arrays(c);
  if (c->run.shape.merged) {
    const SharedPlan p = shared_seg_plan_view(c->d_seg_plan.as<uint32_t>(), c->d_table_rows.as<te_pre_raw>(), n_seg, c->n_shared, c->n_contrib);
    if (kind == Thin) AVRF_SHARED(c->suite, thin_seg_terms(b, off, (uint32_t)n_seg, (uint32_t)L, seeds, c->d_c.as<uint32_t>(), c->d_z.as<uint32_t>(), p, c->L->d_shared.as<uint32_t>(),
                                                           c->L->d_seg_wsz.as<uint32_t>(), a.scalars.as<uint32_t>(), a.pre.as<te_pre_raw>(), c->stream));
    else AVRF_SHARED(c->suite, ped_seg_terms(b, off, (uint32_t)n_seg, (uint32_t)L, seeds, c->d_c.as<uint32_t>(), c->d_z.as<uint8_t>(), p, c->L->d_shared.as<uint32_t>(),
                                             c->L->d_seg_wsz.as<uint32_t>(), a.scalars.as<uint32_t>(), a.pre.as<te_pre_raw>(), c->stream));
    return;
  }
  if (kind == Thin) AVRF_SEG(c->suite, thin_terms(b, off, (uint32_t)n_seg, (uint32_t)L, seeds, c->d_c.as<uint32_t>(), c->d_z.as<uint32_t>(), c->L->d_seg_wsz.as<uint32_t>(),
                                                  a.scalars.as<uint32_t>(), a.pre.as<te_pre_raw>(), c->stream));
  else AVRF_SEG(c->suite, ped_terms(b, off, (uint32_t)n_seg, (uint32_t)L, seeds, c->d_c.as<uint32_t>(), c->d_z.as<uint8_t>(), c->L->d_seg_wsz.as<uint32_t>(),
                                    a.scalars.as<uint32_t>(), a.pre.as<te_pre_raw>(), c->stream));
}
static void launch_seg_item_flags(avrf_ctx *c, int kind, const BatchDev &b) {
  if (kind == Thin) AVRF_SEG(c->suite, item_flags(b, c->d_status.as<int32_t>(), c->stream));
  else AVRF_SEG(c->suite, ped_item_flags(b, c->d_status.as<int32_t>(), c->stream));
}

namespace avrf {
// BatchRun::h_up: the item offsets, then (64-byte aligned) the seeds, then (the merged layout) each segment's row0
static size_t seg_up_seeds_at(size_t n_seg) { return ((n_seg + 1) * 4 + 63) / 64 * 64; }
static size_t seg_up_row0_at(size_t n_seg) { return seg_up_seeds_at(n_seg) + n_seg * sizeof(Seed64); }

int run_begin(avrf_ctx *c, int kind, const RunRequest &rq) {
  if (!c || c->staged_kind != kind || ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  if (rq.segmented && c->n_shared && !(rq.shared_ok && c->lane_owner)) return AVRF_ERR_BAD_ARG;
  // (the layout goes to a local first: a refusal leaves the last segmented run's description, and the context, as they were)
  RunShape sh; sh.segmented = rq.segmented;
  if (rq.segmented) {
    uint64_t lay[5];
    if (int e = seg_layout(kind, c->n, c->n_shared, rq.n_seg, rq.seg_items, c->h_io.as<uint32_t>(), &sh.off, &sh.row0, lay)) return e;
    sh.n_seg = rq.n_seg; sh.L = (size_t)lay[0]; sh.padded = (size_t)lay[1]; sh.merged = lay[4] != 0;
  }
  if (c->n && !c->n_terms) return AVRF_ERR_BAD_ARG;
  BatchRun &r = c->run;
  r.shape = std::move(sh); r.item_status.clear(); r.unit_weights = rq.unit_weights; memset(r.digest, 0, 64);
  if (run_nothing(c)) { r.phase = RunPhase::Begun; return AVRF_OK; }   // src/thin.rs:262-264, src/pedersen.rs:343-345
  HIP_TRY(hipSetDevice(c->device));
  if (rq.segmented) {
    const size_t n_seg = r.shape.n_seg;
    HIP_TRY(r.h_up.ensure(seg_up_row0_at(n_seg) + n_seg * 4));
    memcpy(r.h_up.p, r.shape.off.data(), (n_seg + 1) * 4);
    if (r.shape.merged) memcpy(r.h_up.as<uint8_t>() + seg_up_row0_at(n_seg), r.shape.row0.data(), n_seg * 4);
    if (c->lane_owner) if (int e = seg_ensure(c, kind)) return e;      // (a pool slot has no lane yet: run_launch sizes the lane's arrays)
    if (c->n_shared) c->chal_gen = 0;                                  // (what avrf_*_batch_challenges left in d_c / d_z is overwritten, for Pedersen in another form)
  }
  const double t0 = now_us();
  r.begin_us = 0;
  // prepare once, for all segments: the prepare kernels know nothing about batches, and their records are contiguous per item.
  // An open batch: every push has enqueued its chunk's validation, prepare kernel and copies back already
  if (!ctx_open(c)) {
    Prepare whole; whole.items_only = rq.segmented; whole.rows_stay = c->n_shared && !(rq.segmented && !r.shape.merged);
    if (int e = enqueue_prepare(c, kind, 0, 0, whole)) return e;
    r.begin_us = now_us() - t0;
  }
  r.phase = RunPhase::Begun;
  return AVRF_OK;
}

// the prepare kernel and the copies back have completed (the caller waited for c->stream or for an event behind them)
int run_collect(avrf_ctx *c, int kind) {
  if (!c || c->staged_kind != kind || c->run.phase != RunPhase::Begun) return AVRF_ERR_BAD_ARG;
  if (run_nothing(c)) return AVRF_OK;
  BatchRun &r = c->run;
  r.phase = RunPhase::Idle;                                            // an error below leaves the context idle
  // a wire point that failed to decode / validate is the whole run's status, before the checks of items that never decoded: the
  // sticky flag of an open batch's chunks, or of a staging that was not waited for (ctx_stage); the batch is then gone
  if (ctx_open(c)) if (int e = open_wire_failed(c)) return e;
  if (c->wire_pending) {
    c->wire_pending = false;
    if (c->h_flags.as<uint32_t>()[2]) { c->staged_kind = 0; return AVRF_INVALID_DATA; }
  }
  // The flag word is the batch's: a refused item refuses a whole-batch run (src/thin.rs:266-271, src/pedersen.rs:348-353).  A segmented
  // run finds out which items raised it -- the prepare kernel's checks again, per item, and the validation with a status per item
  // (the clean case pays nothing).  This rare path WAITS for the stream it runs on, c->stream: a pool worker sits here for one
  // prepare-sized kernel on its ingest stream, where only its own stagings queue.
  if (*c->h_flags.as<uint32_t>()) {
    if (!r.shape.segmented) return AVRF_INVALID_DATA;
    const size_t n = c->n;
    HIP_TRY(hipSetDevice(c->device));
    r.item_status.resize(n);
    HIP_TRY(c->d_status.ensure(n * 4));
    HIP_TRY(hipMemsetAsync(c->d_status.p, 0, n * 4, c->stream));
    launch_seg_item_flags(c, kind, batch_of(c));
    validate_staged(c, kind, c->d_status.as<int32_t>());
    HIP_TRY(hipMemcpyAsync(r.item_status.data(), c->d_status.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipGetLastError());
  }
  // room for what the hash writes: the weight stream of a sponge / SHA-256 suite, the groups' messages of a counter-mode one
  if (suite_host_weights(c->suite)) c->h_weights.resize(c->n * kind_facts(kind).weight);
  else if (r.shape.segmented) {
    uint8_t prefix[64]; const size_t pl = batch_prefix(c->suite, prefix);
    r.h_msg.resize(r.shape.n_seg * pl + c->n * kind_facts(kind).record());
  }
  r.phase = RunPhase::Begun;
  return AVRF_OK;
}

size_t run_messages(const avrf_ctx *c) {
  if (suite_host_weights(c->suite) || run_nothing(c)) return 0;
  return c->run.shape.segmented ? c->run.shape.n_seg : 1;
}
// The weight transcript v of the run, SUITE_ID || 0x50 || its items' records (src/thin.rs:274-279, src/pedersen.rs:361-367), described
// for sha512_many: the whole batch's where it is, in h_msg; a group's built in BatchRun::h_msg at a place of its own.
void run_job(avrf_ctx *c, size_t v, WeightJob *job) {
  BatchRun &r = c->run;
  if (!r.shape.segmented) { *job = WeightJob::whole(c->h_msg.as<uint8_t>(), c->h_msg_len); return; }
  uint8_t prefix[64]; const size_t pl = batch_prefix(c->suite, prefix), recsz = kind_facts(c->staged_kind).record();
  const size_t first = r.shape.off[v], items = r.shape.off[v + 1] - first;
  uint8_t *m = r.h_msg.data() + v * pl + first * recsz;
  memcpy(m, prefix, pl); memcpy(m + pl, c->h_msg.as<uint8_t>() + pl + first * recsz, items * recsz);
  *job = WeightJob::whole(m, pl + items * recsz);
}
void run_seed(avrf_ctx *c, size_t v, const uint8_t digest[64]) {
  BatchRun &r = c->run;
  if (!r.shape.segmented) memcpy(r.digest, digest, 64);
  else ((Seed64 *)(r.h_up.as<uint8_t>() + seg_up_seeds_at(r.shape.n_seg)))[v] = seed_of(digest);
}
int run_hash(avrf_ctx *c, int kind, bool spread) {
  if (!c || c->staged_kind != kind || c->run.phase != RunPhase::Begun) return AVRF_ERR_BAD_ARG;
  if (run_nothing(c)) return AVRF_OK;
  const RunShape &sh = c->run.shape;
  const bool host_weights = suite_host_weights(c->suite);
  auto each = [&](size_t count, auto fn) { if (spread) parallel_for(count, fn); else for (size_t i = 0; i < count; i++) fn(i); };
  if (!sh.segmented && ctx_open(c)) {
    // (the caller has waited for c->stream) what no push has absorbed yet, then a CLONE finalised: verify(&self) borrows, the batch
    // stays open and its transcript goes on (src/thin.rs:257)
    if (int e = open_poll(c, /*all=*/true)) { c->run.phase = RunPhase::Idle; return e; }
    const WeightStream fin = c->open.ws.clone();
    if (host_weights) fin.squeeze(c->h_weights.data(), c->h_weights.size()); else fin.digest(c->run.digest);
  } else if (host_weights) {
    // sponge / SHA-256 transcripts: the weight stream of the batch, or of every group, squeezed on the host: item j's 16 (Pedersen: 32) bytes at 16 (32) j
    if (!sh.segmented) squeeze_weights(c, kind, 0, c->n);
    else each(sh.n_seg, [&](size_t v) { if (sh.off[v + 1] != sh.off[v]) squeeze_weights(c, kind, sh.off[v], sh.off[v + 1] - sh.off[v]); });
  } else if (!sh.segmented) {
    // the context's own whole-batch transcript: through the hash service when AVRF_HASH_THREADS enables it
    WeightJob job; run_job(c, 0, &job);
    WeightHashService &svc = WeightHashService::get();
    if (svc.enabled()) svc.run(job); else weight_digest_scalar(job);
    run_seed(c, 0, job.digest);
  } else
    // counter-mode transcripts: sixteen messages at a time through the multi-buffer hash; a group builds its messages itself
    each((sh.n_seg + 15) / 16, [&](size_t g) {
      WeightJob jobs[16]; WeightJob *pj[16]; int cnt = 0;
      for (size_t v = 16 * g; v < sh.n_seg && v < 16 * g + 16; v++, cnt++) { run_job(c, v, &jobs[cnt]); pj[cnt] = &jobs[cnt]; }
      sha512_many(pj, cnt);
      for (int i = 0; i < cnt; i++) run_seed(c, 16 * g + i, jobs[i].digest);
    });
  return AVRF_OK;
}

int run_launch(avrf_ctx *c, int kind) {
  if (!c || c->staged_kind != kind || c->run.phase != RunPhase::Begun) return AVRF_ERR_BAD_ARG;
  BatchRun &r = c->run;
  if (run_nothing(c)) { r.phase = RunPhase::Launched; return AVRF_OK; }
  r.phase = RunPhase::Idle;                                            // an error below leaves the context idle
  HIP_TRY(hipSetDevice(c->device));
  const RunShape &sh = r.shape;
  const size_t n = c->n, n_seg = sh.n_seg;
  if (int e = sh.segmented ? seg_ensure(c, kind) : ensure_terms(c)) return e;
  BatchDev b = batch_of(c);
  if (r.unit_weights) {                                                // (Thin only) w_j = 1: the sum IS the item's own equation
    c->h_weights.assign(n * 16, 0);
    for (size_t j = 0; j < n; j++) c->h_weights[16 * j] = 1;
  }
  if (r.unit_weights || suite_host_weights(c->suite)) {                // the weights as a stream in HBM; else the terms kernel derives them from the seed(s)
    const size_t wbytes = n * kind_facts(kind).weight;
    HIP_TRY(c->d_weights.ensure(wbytes));
    HIP_TRY(hipMemcpyAsync(c->d_weights.p, c->h_weights.data(), wbytes, hipMemcpyHostToDevice, c->stream));
    b.weights = c->d_weights.as<uint8_t>();
  } else if (sh.segmented)
    HIP_TRY(hipMemcpyAsync(c->L->d_seg_seeds.p, r.h_up.as<uint8_t>() + seg_up_seeds_at(n_seg), n_seg * sizeof(Seed64), hipMemcpyHostToDevice, c->stream));
  else b.records = c->d_rec.as<uint8_t>();
  const double t2 = now_us();
  if (sh.segmented) {
    // terms into the padded layout (the padding scalars are zeroed on every run)
    HIP_TRY(hipMemcpyAsync(c->L->d_seg_off.p, r.h_up.p, (n_seg + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(seg_arrays(c).scalars.p, 0, sh.padded * 32, c->stream));
    if (sh.merged) {                                                   // this run's plan: the references sorted by (segment, row)
      uint32_t *plan = c->d_seg_plan.as<uint32_t>();
      HIP_TRY(hipMemcpyAsync(shared_seg_plan_row0(plan, n_seg, c->n_shared, c->n_contrib), r.h_up.as<uint8_t>() + seg_up_row0_at(n_seg), n_seg * 4,
                             hipMemcpyHostToDevice, c->stream));
      HIP_TRY(shared_seg_plan(c->d_table_idx.as<uint32_t>(), c->d_io_off.as<uint32_t>(), c->L->d_seg_off.as<uint32_t>(), (uint32_t)n_seg, (uint32_t)c->n_shared,
                              (uint32_t)c->n, (uint32_t)(c->n_contrib - c->tot_io), (uint32_t)c->tot_io, plan, c->stream));
    }
    launch_seg_terms(c, kind, b, n_seg, sh.L);
  } else launch_terms(c, kind, b, seed_of(r.digest), 0, c->L->d_scalars.as<uint32_t>());
  const double t3 = now_us();
  c->timing[3] = t3 - t2;
  // The MSMs as ONE chain on the lane.  Not for a segmented run of a context of its own lane: that keeps msm_te_segments' choice (fewer
  // than eight segments: one MSM each, waited for) in run_end; a chain that others queue behind -- a pool slot's -- is enqueued here
  if (!sh.segmented) {
    if (int e = msm_guarded([&] { return msm_te_enqueue(c->suite, c->L->d_pre.as<te_pre_raw>(), c->L->d_scalars.as<uint32_t>(), c->n_terms, c->L->ws, c->chain(), c->stream); })) return e;
  } else if (!c->lane_owner) {
    const SegArrays a = seg_arrays(c);
    if (int e = msm_guarded([&] { return msm_te_segments_enqueue(c->suite, a.pre.as<te_pre_raw>(), a.scalars.as<uint32_t>(), sh.L, n_seg, c->L->ws, c->chain(), c->stream); })) return e;
  }
  r.msm_us = now_us() - t3;
  r.phase = RunPhase::Launched;
  return AVRF_OK;
}

int run_end(avrf_ctx *c, int kind, int32_t *status_out) {
  if (!c || c->staged_kind != kind || c->run.phase != RunPhase::Launched) return AVRF_ERR_BAD_ARG;
  BatchRun &r = c->run;
  const RunShape &sh = r.shape;
  const size_t n_out = sh.segmented ? sh.n_seg : 1;
  if (n_out && !status_out) return AVRF_ERR_BAD_ARG;
  r.phase = RunPhase::Idle;
  for (size_t v = 0; v < n_out; v++) status_out[v] = AVRF_OK;          // what an empty batch or segment keeps (src/thin.rs:262-264, src/pedersen.rs:343-345)
  if (run_nothing(c)) return AVRF_OK;
  HIP_TRY(hipSetDevice(c->device));
  const double t3 = now_us();
  std::vector<HostExt> sums(n_out);
  if (!sh.segmented) { if (int e = msm_guarded([&] { return msm_te_finish(c->suite, c->L->ws, c->chain(), c->stream, sums.data()); })) return e; }
  else if (c->lane_owner) { const SegArrays a = seg_arrays(c); if (int e = lane_msm_segments(c, a.pre, a.scalars, sh.L, sh.n_seg, sums.data())) return e; }
  else if (int e = msm_guarded([&] { return msm_te_segments_finish(c->suite, c->L->ws, c->chain(), c->stream, sums.data()); })) return e;
  const double t4 = now_us();
  for (size_t v = 0; v < n_out; v++) {
    if (sh.segmented && sh.off[v] == sh.off[v + 1]) continue;
    status_out[v] = point_is_identity(c, sums[v]) ? AVRF_OK : AVRF_VERIFICATION_FAILURE;   // src/thin.rs:319-322, src/pedersen.rs:420-423
    if (!r.item_status.empty())                                        // (a segmented run's attribution pass) src/thin.rs:266-271, src/pedersen.rs:348-353
      for (size_t j = sh.off[v]; j < sh.off[v + 1]; j++) if (r.item_status[j]) status_out[v] = AVRF_INVALID_DATA;
  }
  const double t5 = now_us();
  // avrf_last_timing after a whole-batch run: time spent IN its calls (a segmented run's caller states wall time instead, run_segments)
  c->timing[4] = r.msm_us + (t4 - t3); c->timing[5] = t5 - t4;
  c->timing[0] = c->timing[1] + c->timing[2] + c->timing[3] + c->timing[4] + c->timing[5];
  if (sh.segmented && c->lane_owner) { c->last_seg.shape = sh; c->last_seg.gen = c->stage_gen; }   // what avrf_*_segment_terms describes
  return AVRF_OK;
}
}  // namespace avrf

// the context's segmented call: the phases one after the other, waiting for the stream between them
static int run_segments(avrf_ctx *c, int kind, size_t n_seg, const uint32_t *seg_items, int32_t *status_out, bool shared_ok = false) {
  if (!c || ctx_busy(c) || (n_seg && !status_out)) return AVRF_ERR_BAD_ARG;
  const double t0 = now_us();
  RunRequest rq; rq.segmented = true; rq.n_seg = n_seg; rq.seg_items = seg_items; rq.shared_ok = shared_ok;
  if (int e = run_begin(c, kind, rq)) return e;
  const bool device_work = !run_nothing(c);
  if (device_work) if (int e = run_wait(c, /*and_last_error=*/true)) return e;
  if (int e = run_collect(c, kind)) return e;
  const double t1 = now_us();
  if (int e = run_hash(c, kind, /*spread=*/true)) return e;
  const double t2 = now_us();
  if (int e = run_launch(c, kind)) return e;
  if (int e = run_end(c, kind, status_out)) return e;
  // avrf_last_timing: prepare + its wait (and the attribution pass), the transcripts, the terms launches, the MSM chain with its wait
  const double t4 = now_us();
  if (device_work) { c->timing[1] = t1 - t0; c->timing[2] = t2 - t1; c->timing[4] = t4 - t2 - c->timing[3]; c->timing[5] = 0; c->timing[0] = t4 - t0; }
  return AVRF_OK;
}
// the terms of one segment of the last segmented run, as avrf_batch_last_terms gives the plain run's
static size_t segment_terms(avrf_ctx *c, int kind, size_t seg, uint8_t *bases_xy, uint8_t *scalars) {
  const RunShape &sh = c ? c->last_seg.shape : RunShape();
  if (!c || ctx_busy(c) || c->staged_kind != kind || c->last_seg.gen != c->stage_gen || seg + 1 >= sh.off.size()) return 0;
  if (hipSetDevice(c->device) != hipSuccess) return 0;
  const uint32_t *io_off = c->h_io.as<uint32_t>();
  const size_t first = sh.off[seg], items = sh.off[seg + 1] - first;
  if (!items) return 0;
  const size_t t0 = seg * sh.L;
  // the merged layout of a shared-table staging: item terms up to the segment's row 0, the rows, the base term(s)
  const size_t count = !sh.row0.empty() ? (sh.row0[seg] - t0) + c->n_shared + (kind == Thin ? 1 : 2)
                                            : n_terms(kind, items, kind == Thin ? io_off[first + items] - io_off[first] : 0);
  return terms_to_host(c, c->d_seg_pre.as<te_pre_raw>() + t0, c->d_seg_scalars.as<uint8_t>() + 32 * t0, count, bases_xy, scalars);
}

extern "C" {

int avrf_thin_batch_run_segments(avrf_ctx *c, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) { return run_segments(c, Thin, n_seg, seg_items, status_out); }
int avrf_pedersen_batch_run_segments(avrf_ctx *c, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) { return run_segments(c, Pedersen, n_seg, seg_items, status_out); }
// the same on WHATEVER staging of the kind the context holds: over a shared table in the shorter of the merged and the expanded layout
// (seg_layout), on a plain staging exactly the calls above
int avrf_thin_batch_run_shared_segments(avrf_ctx *c, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) { return run_segments(c, Thin, n_seg, seg_items, status_out, true); }
int avrf_pedersen_batch_run_shared_segments(avrf_ctx *c, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) { return run_segments(c, Pedersen, n_seg, seg_items, status_out, true); }
int avrf_thin_batch_verify_shared_segments_wire(avrf_ctx *c, size_t n, size_t n_shared, const uint8_t *shared, const uint32_t *pk_index, const uint32_t *input_index,
                                                const uint8_t *outputs, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs,
                                                int validate, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) {
  int st = avrf_thin_batch_stage_shared_wire(c, n, n_shared, shared, pk_index, input_index, outputs, io_counts, ads, ad_lens, proofs, validate);
  return st ? st : avrf_thin_batch_run_shared_segments(c, n_seg, seg_items, status_out);
}
int avrf_pedersen_batch_verify_shared_segments_wire(avrf_ctx *c, size_t n, size_t n_shared, const uint8_t *shared, const uint32_t *input_index, const uint8_t *outputs,
                                                    const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate,
                                                    size_t n_seg, const uint32_t *seg_items, int32_t *status_out) {
  int st = avrf_pedersen_batch_stage_shared_wire(c, n, n_shared, shared, input_index, outputs, io_counts, ads, ad_lens, proofs, validate);
  return st ? st : avrf_pedersen_batch_run_shared_segments(c, n_seg, seg_items, status_out);
}

int avrf_thin_batch_verify_segments(avrf_ctx *c, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts, const uint8_t *ads,
                                    const uint32_t *ad_lens, const uint8_t *proofs, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) {
  int st = avrf_thin_batch_stage(c, n, pks_xy, ios_xy, io_counts, ads, ad_lens, proofs);
  return st ? st : avrf_thin_batch_run_segments(c, n_seg, seg_items, status_out);
}
int avrf_thin_batch_verify_segments_wire(avrf_ctx *c, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                                         const uint32_t *ad_lens, const uint8_t *proofs, int validate, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) {
  int st = avrf_thin_batch_stage_wire(c, n, pks, ios, io_counts, ads, ad_lens, proofs, validate);
  return st ? st : avrf_thin_batch_run_segments(c, n_seg, seg_items, status_out);
}

int avrf_pedersen_batch_verify_segments(avrf_ctx *c, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                                        const uint8_t *proofs, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) {
  int st = avrf_pedersen_batch_stage(c, n, ios_xy, io_counts, ads, ad_lens, proofs);
  return st ? st : avrf_pedersen_batch_run_segments(c, n_seg, seg_items, status_out);
}
int avrf_pedersen_batch_verify_segments_wire(avrf_ctx *c, size_t n, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                                             const uint8_t *proofs, int validate, size_t n_seg, const uint32_t *seg_items, int32_t *status_out) {
  int st = avrf_pedersen_batch_stage_wire(c, n, ios, io_counts, ads, ad_lens, proofs, validate);
  return st ? st : avrf_pedersen_batch_run_segments(c, n_seg, seg_items, status_out);
}

size_t avrf_thin_segment_terms(avrf_ctx *c, size_t seg, uint8_t *bases_xy, uint8_t *scalars) { return segment_terms(c, Thin, seg, bases_xy, scalars); }
size_t avrf_pedersen_segment_terms(avrf_ctx *c, size_t seg, uint8_t *bases_xy, uint8_t *scalars) { return segment_terms(c, Pedersen, seg, bases_xy, scalars); }

// n_seg independent MSMs of L terms through the segmented chain (msm.h msm_te_segments), beside avrf_msm_te
int avrf_msm_te_segments(avrf_ctx *c, size_t n_seg, size_t L, const uint8_t *bases_xy, const uint8_t *scalars, uint8_t *out_xy) {
  if (!c || ctx_busy(c) || (n_seg && !out_xy) || (n_seg && L && (!bases_xy || !scalars)) || n_seg > 0x0fffffffULL) return AVRF_ERR_BAD_ARG;
  uint64_t lay[4];
  if (int e = seg_limits(n_seg, L, lay)) return e;
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = n_seg * L;
  for (size_t i = 0; i < n; i++) if (!scalar_in_range(c->suite, scalars + 32 * i)) return AVRF_INVALID_DATA;
  std::vector<HostExt> sums(n_seg);
  if (n) {
    if (int e = upload_bases_and_scalars(c, n, bases_xy, scalars, n * 32)) return e;
    launch_pre_from_affine(c->suite, c->d_misc.as<uint8_t>(), n, c->L->d_pre.as<te_pre_raw>(), c->d_flags.as<uint32_t>(), 0, c->stream);
    HIP_TRY(hipMemcpyAsync(c->h_flags.p, c->d_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
  }
  c->staged_kind = 0;
  if (int e = lane_msm_segments(c, c->L->d_pre, c->L->d_scalars, L, n_seg, sums.data())) return e;
  if (n && *c->h_flags.as<uint32_t>()) return AVRF_INVALID_DATA;
  for (size_t v = 0; v < n_seg; v++) finish_point(c, sums[v], out_xy + 64 * v);
  return AVRF_OK;
}
// Test probe: the same MSMs through the two halves of the chain (msm.h msm_te_segments_enqueue / _finish) -- ONE chain whatever n_seg is,
// no per-segment loop below eight.  own_record != 0: the lane's own record, finish waits for the stream.  0: a record of the call's own,
// as a pool slot hands in; the call waits for the stream itself before it finishes, which then does not.
int avrf_msm_te_segments_chain(avrf_ctx *c, size_t n_seg, size_t L, const uint8_t *bases_xy, const uint8_t *scalars, int own_record, uint8_t *out_xy) {
  if (!c || ctx_busy(c) || (n_seg && !out_xy) || (n_seg && L && (!bases_xy || !scalars)) || n_seg > 0x0fffffffULL) return AVRF_ERR_BAD_ARG;
  uint64_t lay[4];
  if (int e = seg_limits(n_seg < 8 ? 8 : n_seg, L, lay)) return e;     // (the windows limit holds for every n_seg here: there is no looped route)
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = n_seg * L;
  for (size_t i = 0; i < n; i++) if (!scalar_in_range(c->suite, scalars + 32 * i)) return AVRF_INVALID_DATA;
  std::vector<HostExt> sums(n_seg);
  if (n) {
    if (int e = upload_bases_and_scalars(c, n, bases_xy, scalars, n * 32)) return e;
    launch_pre_from_affine(c->suite, c->d_misc.as<uint8_t>(), n, c->L->d_pre.as<te_pre_raw>(), c->d_flags.as<uint32_t>(), 0, c->stream);
    HIP_TRY(hipMemcpyAsync(c->h_flags.p, c->d_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
  }
  c->staged_kind = 0;
  MsmChain mine;
  MsmChain &rec = own_record ? c->L->ws.own : mine;
  int st = msm_guarded([&] { return msm_te_segments_enqueue(c->suite, c->L->d_pre.as<te_pre_raw>(), c->L->d_scalars.as<uint32_t>(), L, n_seg, c->L->ws, rec, c->stream); });
  if (st == AVRF_OK && !own_record && hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); st = AVRF_ERR_NO_DEVICE; }
  if (st == AVRF_OK) st = msm_guarded([&] { return msm_te_segments_finish(c->suite, c->L->ws, rec, c->stream, sums.data()); });
  if (st != AVRF_OK) { (void)hipStreamSynchronize(c->stream); rec.disarm(); return st; }   // (`mine` must not go while a copy into it is in flight)
  if (n && *c->h_flags.as<uint32_t>()) return AVRF_INVALID_DATA;
  for (size_t v = 0; v < n_seg; v++) finish_point(c, sums[v], out_xy + 64 * v);
  return AVRF_OK;
}

// ---------------------------------------------------------------- one batch split over several GPUs

// weight transcript of src/thin.rs:274-279 / src/pedersen.rs:361-367 over ALL items of a batch (host only)
int avrf_batch_weight_seed(int suite, int pedersen, size_t n, const uint8_t *c16, const uint8_t *resp, uint8_t seed_out[64]) {
  if (suite < 0 || suite >= AVRF_N_SUITES || !seed_out || (n && (!c16 || !resp))) return AVRF_ERR_BAD_ARG;
  // a sponge transcript has no seed to hand to the shards (its weight stream is sequential): the split-one-batch mode is for the
  // counter-mode (HashTranscript) suites; whole batches shard over GPUs for every suite
  if (suite_host_weights(suite)) return AVRF_ERR_BAD_ARG;
  uint8_t prefix[64]; const size_t pl = batch_prefix(suite, prefix);
  HostSha512 h;
  absorb_weight_message(h, prefix, pl, n, c16, resp, kind_facts(pedersen ? Pedersen : Thin).resp);
  h.final(seed_out);
  return AVRF_OK;
}

// the same for up to eight batches at once through the multi-buffer hash (host_sha512_mb.h); AVRF_ERR_NO_DEVICE when the host
// CPU has no AVX-512 (the library then hashes every transcript on its context's thread)
int avrf_batch_weight_seeds_x8(int suite, int pedersen, int count, const size_t *n, const uint8_t *const *c16, const uint8_t *const *resp, uint8_t *seeds_out) {
  if (suite < 0 || suite >= AVRF_N_SUITES || count < 1 || count > 8 || !n || !c16 || !resp || !seeds_out) return AVRF_ERR_BAD_ARG;
  if (suite_host_weights(suite)) return AVRF_ERR_BAD_ARG;
  if (!sha512_mb_available()) return AVRF_ERR_NO_DEVICE;
  uint8_t prefix[64]; const size_t pl = batch_prefix(suite, prefix);
  WeightJob jobs[8]; WeightJob *pj[8];
  for (int i = 0; i < count; i++) {
    if (n[i] && (!c16[i] || !resp[i])) return AVRF_ERR_BAD_ARG;
    jobs[i].prefix = prefix; jobs[i].prefix_len = pl; jobs[i].c16 = c16[i]; jobs[i].resp = resp[i]; jobs[i].n = n[i]; jobs[i].rsz = kind_facts(pedersen ? Pedersen : Thin).resp; pj[i] = &jobs[i];
  }
  sha512_weights_x8(pj, count);
  for (int i = 0; i < count; i++) memcpy(seeds_out + 64 * i, jobs[i].digest, 64);
  return AVRF_OK;
}

// SHA-512 of contiguous messages through ONE named form of the multi-buffer code, whatever sha512_many would pick: exported for tests
static int sha512_messages(int count, int lanes, bool available, void (*many)(WeightJob *const *, int), const uint8_t *const *msgs, const size_t *lens, uint8_t *digests_out) {
  if (count < 1 || count > lanes || !msgs || !lens || !digests_out) return AVRF_ERR_BAD_ARG;
  if (!available) return AVRF_ERR_NO_DEVICE;
  static const uint8_t empty = 0;
  WeightJob jobs[16]; WeightJob *pj[16];
  for (int i = 0; i < count; i++) {
    if (lens[i] && !msgs[i]) return AVRF_ERR_BAD_ARG;
    jobs[i] = WeightJob::whole(lens[i] ? msgs[i] : &empty, lens[i]); pj[i] = &jobs[i];
  }
  many(pj, count);
  for (int i = 0; i < count; i++) memcpy(digests_out + 64 * i, jobs[i].digest, 64);
  return AVRF_OK;
}
// the form avrf_*_batch_run hands to the hash service (prefix || records, one buffer per batch), eight lanes
int avrf_sha512_x8(int count, const uint8_t *const *msgs, const size_t *lens, uint8_t *digests_out) {
  return sha512_messages(count, 8, sha512_mb_available(), sha512_weights_x8, msgs, lens, digests_out);
}
// the form the pool uses (host_sha512_mb.h sha512_weights_x16: more than eight lanes run as two groups of eight in one interleaved round loop)
int avrf_sha512_x16(int count, const uint8_t *const *msgs, const size_t *lens, uint8_t *digests_out) {
  return sha512_messages(count, 16, sha512_mb16_available(), sha512_weights_x16, msgs, lens, digests_out);
}

// prepare (src/thin.rs:209-226, src/pedersen.rs:276-293) on the staged shard: per-item challenges, 16 bytes each
static int batch_challenges(avrf_ctx *c, int kind, uint8_t *c_out) {
  if (!c || c->staged_kind != kind || (c->n && !c_out)) return AVRF_ERR_BAD_ARG;
  if (ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  if (c->n == 0) return AVRF_OK;
  HIP_TRY(hipSetDevice(c->device));
  Prepare p; p.rows_stay = c->n_shared != 0; p.challenges_out = c_out;
  if (int e = enqueue_prepare(c, kind, 0, 0, p)) return e;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (*c->h_flags.as<uint32_t>()) return AVRF_INVALID_DATA;
  c->chal_gen = c->stage_gen;                                         // the challenges in d_c / d_z belong to THIS staging
  return AVRF_OK;
}
// MSM of the staged shard's terms under the GLOBAL weight stream `seed`; the shard's first item has global index first_index.
// Includes the shard's shares of the shared-generator terms (Thin: (G, -sum w s z0); Pedersen: the G and BLINDING_BASE terms), so
// the partial points of all shards add up to the batch MSM of src/thin.rs:319 / src/pedersen.rs:420.
static int batch_partial(avrf_ctx *c, int kind, const uint8_t seed64[64], uint64_t first_index, uint8_t out_xy[64]) {
  if (!c || c->staged_kind != kind || !seed64 || !out_xy) return AVRF_ERR_BAD_ARG;
  if (ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  // a sponge / SHA-256 transcript has no seed to hand to the shards (avrf_batch_weight_seed refuses those suites too)
  if (suite_host_weights(c->suite)) return AVRF_ERR_BAD_ARG;
  if (c->n && c->chal_gen != c->stage_gen) return AVRF_ERR_BAD_ARG;     // *_batch_challenges has not run on this staging (or it failed)
  HIP_TRY(hipSetDevice(c->device));
  HostExt r;
  if (c->n == 0) { r = with_suite(c->suite, [&](auto tag) { using S = typename decltype(tag)::type; return HostTe<S>::identity(); }); return finish_point(c, r, out_xy); }
  launch_terms(c, kind, batch_of(c), seed_of(seed64), first_index, c->L->d_scalars.as<uint32_t>());
  if (int e = lane_msm(c, c->n_terms, &r)) return e;
  return finish_point(c, r, out_xy);
}
int avrf_thin_batch_challenges(avrf_ctx *c, uint8_t *c_out) { return batch_challenges(c, Thin, c_out); }
int avrf_thin_batch_partial(avrf_ctx *c, const uint8_t seed64[64], uint64_t first_index, uint8_t out_xy[64]) { return batch_partial(c, Thin, seed64, first_index, out_xy); }
int avrf_pedersen_batch_challenges(avrf_ctx *c, uint8_t *c_out) { return batch_challenges(c, Pedersen, c_out); }
int avrf_pedersen_batch_partial(avrf_ctx *c, const uint8_t seed64[64], uint64_t first_index, uint8_t out_xy[64]) { return batch_partial(c, Pedersen, seed64, first_index, out_xy); }

// sum of k affine points on the host (combining per-GPU partial MSM results)
int avrf_points_sum(int suite, size_t k, const uint8_t *points_xy, uint8_t out_xy[64]) {
  if (suite < 0 || suite >= AVRF_N_SUITES || !out_xy || (k && !points_xy)) return AVRF_ERR_BAD_ARG;
  bool bad = false;
  with_suite(suite, [&](auto tag) { using S = typename decltype(tag)::type; using T = HostTe<S>;
    HostExt acc = T::identity(), p;
    for (size_t i = 0; i < k && !bad; i++) { if (!T::from_affine_bytes(points_xy + 64 * i, &p)) bad = true; else acc = T::add(acc, p); }
    if (!bad) T::to_affine_bytes(acc, out_xy); });
  if (bad) return AVRF_INVALID_DATA;
  return AVRF_OK;
}

size_t avrf_batch_last_terms(avrf_ctx *c, uint8_t *bases_xy, uint8_t *scalars) {
  if (!c || !c->staged_kind || !c->n_terms || ctx_busy(c)) return 0;
  if (hipSetDevice(c->device) != hipSuccess) return 0;
  return terms_to_host(c, c->L->d_pre.as<te_pre_raw>(), c->L->d_scalars.as<uint8_t>(), c->n_terms, bases_xy, scalars);
}

void avrf_last_timing(avrf_ctx *c, double out[8]) {
  if (!c || !out) return;
  for (int i = 0; i < 8; i++) out[i] = c->timing[i];
}

int avrf_kernel_stats(avrf_ctx *c, int reset, double *accum_ms_total, uint64_t *accum_launches, int32_t plan[4]) {
  if (!c) return AVRF_ERR_BAD_ARG;
  if (accum_ms_total) *accum_ms_total = c->L->ws.accum_ms_total;
  if (accum_launches) *accum_launches = c->L->ws.accum_launches;
  if (plan) { plan[0] = c->L->ws.last_plan.c; plan[1] = c->L->ws.last_plan.nwin; plan[2] = c->L->ws.last_plan.nb; plan[3] = c->L->ws.last_plan.lpb; }
  if (reset) { c->L->ws.accum_ms_total = 0; c->L->ws.accum_launches = 0; }
  return AVRF_OK;
}

}  // extern "C"
// ---------------------------------------------------------------- independent per-item calls

// the input flags, read once the stream has drained: AVRF_INVALID_DATA when a check refused an input
static int read_flags(avrf_ctx *c) {
  if (hipMemcpyAsync(c->h_flags.p, c->d_flags.p, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return AVRF_ERR_NO_DEVICE;
  if (hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess) return AVRF_ERR_NO_DEVICE;
  static const bool trace = getenv("AVRF_TRACE_FLAGS") != nullptr;   // which check refused the input: 1 range, 2 identity, 4 scalar, 8 curve
  if (trace && *c->h_flags.as<uint32_t>()) fprintf(stderr, "avrf: input flags 0x%x (suite %d)\n", *c->h_flags.as<uint32_t>(), c->suite);
  return *c->h_flags.as<uint32_t>() ? AVRF_INVALID_DATA : AVRF_OK;
}

// the context's stream has drained: AVRF_OK, or AVRF_ERR_NO_DEVICE when it (or anything before it) failed
static int sync_stream(avrf_ctx *c) {
  HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipGetLastError());
  return AVRF_OK;
}

// few items with one I/O pair each: the kernels that spread an item over 32 lanes (vrf_single.hip "few items")
static bool wave_shape(const avrf_ctx *c, size_t n, const uint32_t *io_counts) {
  if (!n || n > (size_t)AVRF_WAVE_ITEMS_MAX || c->tot_io != n) return false;
  static const bool off = getenv("AVRF_NO_WAVE_ITEMS") != nullptr;     // (A/B hook)
  if (off) return false;
  for (size_t j = 0; j < n; j++) if (io_counts[j] != 1) return false;
  return true;
}

// The one-item routes below take a call of ONE item through the MSM engine instead of a kernel per item.  Each answers the call's
// status, or nothing when the item is too large for it (the call then goes on to the kernels).
using Route = std::optional<int>;
static bool one_as_msm() { static const bool on = getenv("AVRF_NO_ONE_AS_MSM") == nullptr; return on; }   // (A/B hook)

// ONE thin / tiny proof with fewer than 1000 I/O pairs (vrf_single.hip k_thin_prove_begin / _end): the terms of R = k G + sum (k z_i) I_i,
// the single-launch MSM with the host's Horner, R back as canonical x || y, challenge and response.  0.71 -> ~0.3 ms
// for one proof; same bytes (any evaluation of R gives the same group element).  The nonce never leaves device memory.
static Route prove_one_as_msm(avrf_ctx *c, bool have_pk, bool tiny, uint8_t *proofs_out) {
  if (c->tot_io >= 1000) return {};
  const size_t nt = 1 + c->tot_io, plen = kind_facts(tiny ? Tiny : Thin).xy_proof(), sb = AVRF_SINGLE(c->suite, prove_state_bytes());
  HIP_TRY(c->h_c.ensure(64));
  if (!have_pk) { if (int fs = ensure_fixed(c)) return fs; }
  HIP_TRY(c->L->d_scalars.ensure(nt * 32)); HIP_TRY(c->L->d_pre.ensure(nt * sizeof(te_pre_raw))); HIP_TRY(c->d_misc.ensure(sb + 64)); HIP_TRY(c->d_out.ensure(plen));
  BatchDev b = batch_of(c);
  if (!have_pk) b.pks_xy = nullptr;
  uint8_t *d_state = c->d_misc.as<uint8_t>();
  AVRF_SINGLE(c->suite, thin_prove_begin(b, c->L->d_scalars.as<uint32_t>(), c->L->d_pre.as<te_pre_raw>(), d_state, c->stream, tiny));
  HostExt r;
  if (int e = lane_msm(c, nt, &r)) return e;
  uint8_t *rxy = c->h_c.as<uint8_t>();                                  // (pinned; the challenges are not in use by a prover)
  finish_point(c, r, rxy);
  HIP_TRY(hipMemcpyAsync(d_state + sb, rxy, 64, hipMemcpyHostToDevice, c->stream));
  AVRF_SINGLE(c->suite, thin_prove_end(b, d_state, d_state + sb, c->d_out.as<uint8_t>(), c->d_flags.as<uint32_t>(), c->stream, tiny));
  HIP_TRY(hipMemcpyAsync(proofs_out, c->d_out.p, plen, hipMemcpyDeviceToHost, c->stream));
  return read_flags(c);
}

// ONE Pedersen proof with up to 1000 I/O pairs the same way (vrf_single.hip k_ped_prove_begin / _mid / _end): Yb = pk + bl B as a
// two-term MSM, then R = k G + kb B and Ok = k I_m as two scalar vectors over {G, B, I_0, ..} in one launch; every doubling chain is
// the host's.  1.03 -> ~0.5 ms.
static Route prove_ped_one_as_msm(avrf_ctx *c, bool have_pk, uint8_t *proofs_out, uint8_t *blindings_out) {
  if (c->tot_io > 1000) return {};
  if (!have_pk) { if (int fs = ensure_fixed(c)) return fs; }
  const size_t m = c->tot_io, nt = 2 + m, sb = AVRF_SINGLE(c->suite, ped_state_bytes()), wb = (m * 32 + 63) / 64 * 64 + 64;
  HIP_TRY(c->L->d_scalars.ensure(2 * nt * 32)); HIP_TRY(c->L->d_pre.ensure(nt * sizeof(te_pre_raw)));
  HIP_TRY(c->d_misc.ensure(sb + wb + 192 + 32)); HIP_TRY(c->d_out.ensure(kind_facts(Pedersen).xy_proof())); HIP_TRY(c->h_c.ensure(192));
  BatchDev b = batch_of(c);
  if (!have_pk) b.pks_xy = nullptr;
  uint8_t *d_state = c->d_misc.as<uint8_t>(), *d_pts = d_state + sb + wb, *d_blind = d_pts + 192;
  uint32_t *d_wts = reinterpret_cast<uint32_t *>(d_state + sb);
  uint32_t *d_sc = c->L->d_scalars.as<uint32_t>(); te_pre_raw *d_pre = c->L->d_pre.as<te_pre_raw>();
  AVRF_SINGLE(c->suite, ped_prove_begin(b, d_sc, d_pre, d_state, d_wts, c->stream));
  HostExt r[2];
  if (int e = lane_msm(c, 2, &r[0])) return e;
  uint8_t *pts = c->h_c.as<uint8_t>();                                  // pinned: Yb | R | Ok
  finish_point(c, r[0], pts);
  HIP_TRY(hipMemcpyAsync(d_pts, pts, 64, hipMemcpyHostToDevice, c->stream));
  AVRF_SINGLE(c->suite, ped_prove_mid(b, d_sc, d_pre, d_state, d_wts, d_pts, c->stream));
  if (int e = lane_msm_vectors(c, nt, 2, r)) return e;
  finish_point(c, r[0], pts + 64); finish_point(c, r[1], pts + 128);
  HIP_TRY(hipMemcpyAsync(d_pts + 64, pts + 64, 128, hipMemcpyHostToDevice, c->stream));
  AVRF_SINGLE(c->suite, ped_prove_end(b, d_state, d_pts, c->d_out.as<uint8_t>(), blindings_out ? d_blind : nullptr, c->d_flags.as<uint32_t>(), c->stream));
  HIP_TRY(hipMemcpyAsync(proofs_out, c->d_out.p, kind_facts(Pedersen).xy_proof(), hipMemcpyDeviceToHost, c->stream));
  if (blindings_out) HIP_TRY(hipMemcpyAsync(blindings_out, d_blind, 32, hipMemcpyDeviceToHost, c->stream));
  return read_flags(c);
}

// ONE Thin item of up to 2048 MSM terms: its equation  R + c z0 pk + sum_i c z_i O_i - s z0 G - sum_i s z_i I_i == 0  (src/thin.rs:158-161
// expanded, the BatchVerifier's sum with the weight w = 1) through the prepare / terms kernels and the single-launch MSM
// (msm.hip k_msm_tiny_bits): the doubling chain runs on the host's Horner instead of a lone wave -- 0.54 -> 0.28 ms.  Same
// statuses as the per-item kernels: the flags of the prepare kernel and of the validation are InvalidData, a non-zero sum is
// VerificationFailure.  Everything is enqueued back to back; the one wait is in run_end.
static Route verify_one_as_msm(avrf_ctx *c, int32_t *status_out) {
  if (!c->n_terms || c->n_terms > 2048) return {};
  RunRequest rq; rq.unit_weights = true;
  int32_t verdict = AVRF_OK;
  int st = run_begin(c, Thin, rq);
  if (st == AVRF_OK) st = run_launch(c, Thin);
  if (st == AVRF_OK) st = run_end(c, Thin, &verdict);
  if (st != AVRF_OK) return st;
  status_out[0] = *c->h_flags.as<uint32_t>() ? AVRF_INVALID_DATA : verdict;
  return AVRF_OK;
}

// ONE Pedersen item of up to 2048 terms: its two equations (src/pedersen.rs:229-245) as two scalar vectors over the item's seven
// bases -- the terms kernel run with the weights (t, u) = (1, 0) and (0, 1) -- through the single-launch MSM with the host's two
// Horners side by side (see verify_one_as_msm): both sums must be the identity, exactly the reference's two checks.  0.52 -> ~0.33 ms.
static Route verify_ped_one_as_msm(avrf_ctx *c, int32_t *status_out) {
  if (!c->n_terms || c->n_terms > 2048) return {};
  HIP_TRY(hipSetDevice(c->device));
  if (int e = enqueue_prepare(c, Pedersen, 0, 0, Prepare())) return e;     // validation + prepare kernel (challenge, merged pair) + flags copy: no run is opened
  const size_t nt = c->n_terms;
  HIP_TRY(c->L->d_scalars.ensure(2 * nt * 32)); HIP_TRY(c->L->d_pre.ensure(nt * sizeof(te_pre_raw))); HIP_TRY(c->L->d_gpart.ensure(2 * 64 + 64));
  c->h_weights.assign(64, 0); c->h_weights[0] = 1; c->h_weights[32 + 16] = 1;                     // (t, u) = (1, 0) | (0, 1)
  HIP_TRY(c->d_weights.ensure(64));
  HIP_TRY(hipMemcpyAsync(c->d_weights.p, c->h_weights.data(), 64, hipMemcpyHostToDevice, c->stream));
  BatchDev b = batch_of(c);
  const uint8_t zero[64] = {0};
  for (int v = 0; v < 2; v++) {
    b.weights = c->d_weights.as<uint8_t>() + 32 * v;
    launch_terms(c, Pedersen, b, seed_of(zero), 0, c->L->d_scalars.as<uint32_t>() + (size_t)v * nt * 8);
  }
  HostExt r[2];
  if (int e = lane_msm_vectors(c, nt, 2, r)) return e;
  status_out[0] = *c->h_flags.as<uint32_t>() ? AVRF_INVALID_DATA : (point_is_identity(c, r[0]) && point_is_identity(c, r[1])) ? AVRF_OK : AVRF_VERIFICATION_FAILURE;
  return AVRF_OK;
}

// What a per-item entry point hands the route driver besides its inputs
struct ItemCall {
  int kind;                  // ProofKind (ctx_stage); the proofs are kind_facts(kind).xy_proof() bytes each
  bool prover;
  uint8_t *proofs_out;       // provers: n proofs
  uint8_t *blindings_out;    // the Pedersen prover: n blindings, or NULL
  int32_t *status_out;       // verifiers: n statuses
};

// The one body of avrf_{thin,tiny,pedersen}_{prove,verify}: stage the inputs, then the first route that takes the call --
// `one` (one item through the MSM engine), `wave` (few items with one I/O pair each, 32 lanes per item; false: the suite has no
// such kernel) unless an item comes back AVRF_WAVE_FALLBACK (a degenerate point), else `lane` (a lane per item, in ITEM_CHUNK
// chunks) -- then the proofs (and blindings) back and the input flags read, or the statuses back.
template <class One, class Wave, class Lane>
static int item_call(avrf_ctx *c, const ItemCall &k, size_t n, const uint8_t *sks, const uint8_t *pks_xy, const uint8_t *ios_xy,
                     const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, One one, Wave wave, Lane lane) {
  // Tiny waits for its staging copies; Thin and Pedersen leave them in flight (the call waits for the stream before it returns)
  BatchSource src = plain_source(k.kind, n, pks_xy, ios_xy, io_counts, ads, ad_lens, proofs);
  src.sks = sks;
  int st = ctx_stage(c, src, k.kind == Tiny);
  if (st || !n) return st;
  const size_t psz = kind_facts(k.kind).xy_proof();
  if (k.prover) {
    c->staged_kind = 0;       // (a Thin / Pedersen verifier leaves its batch staged: avrf_batch_last_terms and avrf_*_batch_run see it)
    HIP_TRY(c->d_out.ensure(n * psz));
    if (k.kind == Pedersen) HIP_TRY(c->d_misc.ensure(n * 32));                // the blindings
  } else HIP_TRY(c->d_status.ensure(n * 4));
  // the provers read the input flags back; the Tiny verifier has always cleared them too, the Thin / Pedersen verifiers never have
  if (k.prover || k.kind == Tiny) HIP_TRY(hipMemsetAsync(c->d_flags.p, 0, 4, c->stream));
  auto finish = [&](bool wave_statuses) -> int {
    if (!k.prover) {
      validate_staged(c, k.kind, c->d_status.as<int32_t>());           // Validate::Yes failures overwrite the item's status with InvalidData
      HIP_TRY(hipMemcpyAsync(k.status_out, c->d_status.p, n * 4, hipMemcpyDeviceToHost, c->stream));
      return sync_stream(c);
    }
    HIP_TRY(hipMemcpyAsync(k.proofs_out, c->d_out.p, n * psz, hipMemcpyDeviceToHost, c->stream));
    if (k.blindings_out) HIP_TRY(hipMemcpyAsync(k.blindings_out, c->d_misc.p, n * 32, hipMemcpyDeviceToHost, c->stream));
    if (wave_statuses) HIP_TRY(hipMemcpyAsync(c->h_c.p, c->d_status.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    return read_flags(c);
  };
  auto routes = [&]() -> int {
    if (n == 1 && one_as_msm()) { if (Route r = one()) return *r; }
    if ((!k.prover || pks_xy) && wave_shape(c, n, io_counts)) {      // (the wave provers take the public keys as given)
      if (k.prover && k.kind == Pedersen) { if (int fs = ensure_fixed(c)) return fs; }   // (the Pedersen one reads the fixed-base tables)
      if (k.prover) { HIP_TRY(c->d_status.ensure(n * 4)); HIP_TRY(c->h_c.ensure(n * 4)); }
      if (wave(batch_of(c))) {
        const int ws = finish(true);
        if (ws < 0) return ws;
        const int32_t *h_status = k.prover ? c->h_c.as<int32_t>() : k.status_out;
        bool fallback = false;
        for (size_t j = 0; j < n; j++) fallback |= h_status[j] == AVRF_WAVE_FALLBACK;
        if (!fallback) return ws;
        if (k.prover) HIP_TRY(hipMemsetAsync(c->d_flags.p, 0, 4, c->stream));   // (the lane-per-item kernel takes the call)
      }
    }
    if (int e = per_item_chunks(c, !k.prover || pks_xy, lane)) return e;
    return finish(false);
  };
  const double t0 = now_us();
  st = routes();
  c->timing[0] = now_us() - t0;               // avrf_last_timing: the routes' wall time, for every kind and on every return
  if (k.kind == Tiny && st == AVRF_OK) c->staged_kind = 0;                 // Tiny has no batch verifier: nothing stays staged
  return st;
}

// The opening of the point-wise calls below: AVRF_ERR_BAD_ARG for a missing argument (`args_ok` false), a busy context or more than
// 2^31 - 1 items, AVRF_OK for none; else `body` runs with the context's device selected and whatever was staged dropped.
template <class F> static int pointwise(avrf_ctx *c, size_t n, bool args_ok, F body) {
  if (!c || (n && !args_ok) || ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  if (!n) return AVRF_OK;
  if (n > 0x7fffffffULL) return AVRF_ERR_BAD_ARG;
  HIP_TRY(hipSetDevice(c->device));
  c->staged_kind = 0;
  return body();
}
extern "C" {

// thin::Prover::prove and tiny::Prover::prove (src/thin.rs:111-129, src/tiny.rs:163-176): the same kernels, told apart by `tiny`
static int thin_or_tiny_prove(avrf_ctx *c, bool tiny, size_t n, const uint8_t *sks, const uint8_t *pks_xy, const uint8_t *ios_xy,
                              const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, uint8_t *proofs_out) {
  if (n && (!sks || !proofs_out)) return AVRF_ERR_BAD_ARG;
  return item_call(c, {tiny ? Tiny : Thin, true, proofs_out, nullptr, nullptr}, n, sks, pks_xy, ios_xy, io_counts, ads, ad_lens, nullptr,
      [&] { return prove_one_as_msm(c, pks_xy != nullptr, tiny, proofs_out); },
      [&](const BatchDev &b) { return AVRF_SINGLE(c->suite, thin_prove_wave(b, c->d_out.as<uint8_t>(), c->d_flags.as<uint32_t>(), c->d_status.as<int32_t>(), c->stream, tiny)); },
      [&](const BatchDev &b) { AVRF_SINGLE(c->suite, thin_prove(b, c->d_out.as<uint8_t>(), c->d_flags.as<uint32_t>(), c->stream, tiny)); });
}

int avrf_thin_prove(avrf_ctx *c, size_t n, const uint8_t *sks, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                    const uint8_t *ads, const uint32_t *ad_lens, uint8_t *proofs_out) {
  return thin_or_tiny_prove(c, false, n, sks, pks_xy, ios_xy, io_counts, ads, ad_lens, proofs_out);
}

int avrf_thin_verify(avrf_ctx *c, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                     const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int32_t *status_out) {
  if (n && (!pks_xy || !proofs || !status_out)) return AVRF_ERR_BAD_ARG;
  return item_call(c, {Thin, false, nullptr, nullptr, status_out}, n, nullptr, pks_xy, ios_xy, io_counts, ads, ad_lens, proofs,
      [&] { return verify_one_as_msm(c, status_out); },
      [&](const BatchDev &b) { return AVRF_SINGLE(c->suite, thin_verify_wave(b, c->d_status.as<int32_t>(), c->stream)); },
      [&](const BatchDev &b) { AVRF_SINGLE(c->suite, thin_verify(b, c->d_status.as<int32_t>(), c->stream)); });
}

// tiny::Prover::prove / tiny::Verifier::verify (src/tiny.rs:163-214) for batches of independent items
int avrf_tiny_prove(avrf_ctx *c, size_t n, const uint8_t *sks, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                    const uint8_t *ads, const uint32_t *ad_lens, uint8_t *proofs_out) {
  return thin_or_tiny_prove(c, true, n, sks, pks_xy, ios_xy, io_counts, ads, ad_lens, proofs_out);
}
int avrf_tiny_verify(avrf_ctx *c, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                     const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int32_t *status_out) {
  if (n && (!pks_xy || !proofs || !status_out)) return AVRF_ERR_BAD_ARG;
  return item_call(c, {Tiny, false, nullptr, nullptr, status_out}, n, nullptr, pks_xy, ios_xy, io_counts, ads, ad_lens, proofs,
      [] { return Route(); },                                          // (no one-item route)
      [&](const BatchDev &b) { return AVRF_SINGLE(c->suite, tiny_verify_wave(b, c->d_status.as<int32_t>(), c->stream)); },
      [&](const BatchDev &b) { AVRF_SINGLE(c->suite, tiny_verify(b, c->d_status.as<int32_t>(), c->stream)); });
}

int avrf_pedersen_prove(avrf_ctx *c, size_t n, const uint8_t *sks, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                        const uint8_t *ads, const uint32_t *ad_lens, uint8_t *proofs_out, uint8_t *blindings_out) {
  if (n && (!sks || !proofs_out)) return AVRF_ERR_BAD_ARG;
  return item_call(c, {Pedersen, true, proofs_out, blindings_out, nullptr}, n, sks, pks_xy, ios_xy, io_counts, ads, ad_lens, nullptr,
      [&] { return prove_ped_one_as_msm(c, pks_xy != nullptr, proofs_out, blindings_out); },
      [&](const BatchDev &b) { return AVRF_SINGLE(c->suite, ped_prove_wave(b, c->d_out.as<uint8_t>(), c->d_misc.as<uint8_t>(), c->d_flags.as<uint32_t>(), c->d_status.as<int32_t>(), c->stream)); },
      [&](const BatchDev &b) { AVRF_SINGLE(c->suite, ped_prove(b, c->d_out.as<uint8_t>(), c->d_misc.as<uint8_t>(), c->d_flags.as<uint32_t>(), c->stream)); });
}

int avrf_pedersen_verify(avrf_ctx *c, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts,
                         const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int32_t *status_out) {
  if (n && (!proofs || !status_out)) return AVRF_ERR_BAD_ARG;
  return item_call(c, {Pedersen, false, nullptr, nullptr, status_out}, n, nullptr, nullptr, ios_xy, io_counts, ads, ad_lens, proofs,
      [&] { return verify_ped_one_as_msm(c, status_out); },
      [&](const BatchDev &b) { return AVRF_SINGLE(c->suite, ped_verify_wave(b, c->d_status.as<int32_t>(), c->stream)); },
      [&](const BatchDev &b) { AVRF_SINGLE(c->suite, ped_verify(b, c->d_status.as<int32_t>(), c->stream)); });
}

static int smul_common(avrf_ctx *c, size_t n, const uint8_t *scalars, const uint8_t *points_xy, uint8_t *out_xy) {
  return pointwise(c, n, scalars && out_xy, [&]() -> int {
    // A handful of variable-base products (Secret::output = sk * input, src/lib.rs:391-393: 80 us on a CPU core): a lane walks 253
    // doublings in 1.9 ms however few items there are.  Up to 32 go through the single-launch MSM instead, as n scalar vectors over
    // the n bases with the scalars on the diagonal (a zero scalar has no bit sums), the doubling chains folded side by side on the host pool: 0.15 ms for one, ~0.4 ms for 32.
    // The bit sums are the literal product for ANY curve point, like the lane kernel's window form (no endomorphism split).
    if (points_xy && n <= 32 && one_as_msm()) {
      for (size_t i = 0; i < n; i++) if (!scalar_in_range(c->suite, scalars + 32 * i)) return AVRF_INVALID_DATA;
      std::vector<uint8_t> diag(n * n * 32, 0);
      for (size_t i = 0; i < n; i++) memcpy(&diag[(i * n + i) * 32], scalars + 32 * i, 32);
      if (int e = upload_bases_and_scalars(c, n, points_xy, diag.data(), diag.size())) return e;
      launch_pre_from_affine(c->suite, c->d_misc.as<uint8_t>(), n, c->L->d_pre.as<te_pre_raw>(), c->d_flags.as<uint32_t>(), 0, c->stream);
      HIP_TRY(hipMemcpyAsync(c->h_flags.p, c->d_flags.p, 4, hipMemcpyDeviceToHost, c->stream));
      HostExt r[32];
      if (int e = lane_msm_vectors(c, n, n, r)) return e;
      if (*c->h_flags.as<uint32_t>()) return AVRF_INVALID_DATA;
      for (size_t i = 0; i < n; i++) finish_point(c, r[i], out_xy + 64 * i);
      return AVRF_OK;
    }
    HIP_TRY(c->d_sks.ensure(n * 32)); HIP_TRY(c->d_out.ensure(n * 64));
    HIP_TRY(hipMemcpyAsync(c->d_sks.p, scalars, n * 32, hipMemcpyHostToDevice, c->stream));
    if (points_xy) { HIP_TRY(c->d_misc.ensure(n * 64)); HIP_TRY(hipMemcpyAsync(c->d_misc.p, points_xy, n * 64, hipMemcpyHostToDevice, c->stream)); }
    HIP_TRY(hipMemsetAsync(c->d_flags.p, 0, 4, c->stream));
    if (!points_xy) { if (int fs = ensure_fixed(c)) return fs; }
    AVRF_SINGLE(c->suite, smul(c->d_sks.as<uint8_t>(), points_xy ? c->d_misc.as<uint8_t>() : nullptr, (uint32_t)n, c->d_out.as<uint8_t>(),
                               c->d_flags.as<uint32_t>(), c->d_fixed.as<te_pre_raw>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out_xy, c->d_out.p, n * 64, hipMemcpyDeviceToHost, c->stream));
    return read_flags(c);
  });
}
int avrf_scalar_mul_base(avrf_ctx *c, size_t n, const uint8_t *sks, uint8_t *out_xy) { return smul_common(c, n, sks, nullptr, out_xy); }
int avrf_scalar_mul(avrf_ctx *c, size_t n, const uint8_t *scalars, const uint8_t *points_xy, uint8_t *out_xy) {
  if (n && !points_xy) return AVRF_ERR_BAD_ARG;
  return smul_common(c, n, scalars, points_xy, out_xy);
}

size_t avrf_point_len(int suite) { return (suite < 0 || suite >= AVRF_N_SUITES) ? 0 : (size_t)point_len_of(suite); }

int avrf_points_decompress(avrf_ctx *c, size_t n, const uint8_t *in, uint8_t *out_xy, int validate, int32_t *status_out) {
  return pointwise(c, n, in && out_xy && status_out, [&]() -> int {
    const size_t pl = (size_t)point_len_of(c->suite);
    HIP_TRY(c->d_misc.ensure(n * pl)); HIP_TRY(c->d_out.ensure(n * 64)); HIP_TRY(c->d_status.ensure(n * 4));
    HIP_TRY(hipMemcpyAsync(c->d_misc.p, in, n * pl, hipMemcpyHostToDevice, c->stream));
    AVRF_SINGLE(c->suite, decompress(c->d_misc.as<uint8_t>(), (uint32_t)n, c->d_out.as<uint8_t>(), validate, c->d_status.as<int32_t>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out_xy, c->d_out.p, n * 64, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status_out, c->d_status.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
  });
}
int avrf_hash_to_curve(avrf_ctx *c, size_t n, const uint8_t *data, const uint32_t *data_lens, uint8_t *out_xy, int32_t *status_out) {
  // the messages' offsets are checked with the arguments, before the device is selected: lengths that sum to 2^32 or more, or no
  // data for messages that are not all empty, are AVRF_ERR_BAD_ARG (a call pointwise() refuses anyway is refused before the walk)
  if (!c || ctx_busy(c)) return AVRF_ERR_BAD_ARG;
  bool ok = data_lens && out_xy && status_out && n <= 0x7fffffffULL;
  std::vector<uint32_t> off(ok ? n + 1 : 0); uint64_t tot = 0;
  for (size_t i = 0; ok && i < n; i++) { off[i] = (uint32_t)tot; tot += data_lens[i]; ok = tot <= 0xffffffffULL; }
  if (ok) { off[n] = (uint32_t)tot; ok = !tot || data; }
  return pointwise(c, n, ok, [&]() -> int {
    HIP_TRY(c->d_ads.ensure(tot + 16)); HIP_TRY(c->d_ad_off.ensure((n + 1) * 4)); HIP_TRY(c->d_out.ensure(n * 64)); HIP_TRY(c->d_status.ensure(n * 4));
    if (tot) HIP_TRY(hipMemcpyAsync(c->d_ads.p, data, tot, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_ad_off.p, off.data(), (n + 1) * 4, hipMemcpyHostToDevice, c->stream));
    AVRF_SINGLE(c->suite, hash_to_curve(c->d_ads.as<uint8_t>(), c->d_ad_off.as<uint32_t>(), (uint32_t)n, c->d_out.as<uint8_t>(), c->d_status.as<int32_t>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out_xy, c->d_out.p, n * 64, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status_out, c->d_status.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
  });
}
// Output::hash::<N> of n output points (x || y in, N = hash_len <= 64 bytes each out)
int avrf_output_hash(avrf_ctx *c, size_t n, const uint8_t *points_xy, size_t hash_len, uint8_t *out) {
  if (hash_len < 1 || hash_len > 64) return AVRF_ERR_BAD_ARG;
  return pointwise(c, n, points_xy && out, [&]() -> int {
    HIP_TRY(c->d_misc.ensure(n * 64)); HIP_TRY(c->d_out.ensure(n * 64));
    HIP_TRY(hipMemcpyAsync(c->d_misc.p, points_xy, n * 64, hipMemcpyHostToDevice, c->stream));
    AVRF_SINGLE(c->suite, output_hash(c->d_misc.as<uint8_t>(), (uint32_t)n, (uint32_t)hash_len, c->d_out.as<uint8_t>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->d_out.p, n * hash_len, hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
  });
}
// Secret::from_seed for n 32-byte seeds: the secret scalars (LE32, canonical) and, when pks_xy_out is given, the public keys
int avrf_secret_from_seed(avrf_ctx *c, size_t n, const uint8_t *seeds, uint8_t *sks_out, uint8_t *pks_xy_out) {
  return pointwise(c, n, seeds && sks_out, [&]() -> int {
    HIP_TRY(c->d_misc.ensure(n * 32)); HIP_TRY(c->d_sks.ensure(n * 32));
    HIP_TRY(hipMemcpyAsync(c->d_misc.p, seeds, n * 32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_flags.p, 0, 4, c->stream));
    AVRF_SINGLE(c->suite, secret_from_seed(c->d_misc.as<uint8_t>(), (uint32_t)n, c->d_sks.as<uint8_t>(), c->d_flags.as<uint32_t>(), c->stream));
    HIP_TRY(hipMemcpyAsync(sks_out, c->d_sks.p, n * 32, hipMemcpyDeviceToHost, c->stream));
    // the reference zeroizes the seed and the intermediate scalar (src/lib.rs:367-368): the seeds are scrubbed from the scratch buffer
    // behind the kernel, the scalars behind the copy back (d_misc / d_sks are general scratch that later, non-secret calls reuse and
    // copy from).  sks_out is the caller's to scrub, as `Secret` is the caller's in the reference.
    HIP_TRY(hipMemsetAsync(c->d_misc.p, 0, n * 32, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_sks.p, 0, n * 32, c->stream));
    if (int st = read_flags(c)) return st;
    if (!pks_xy_out) return AVRF_OK;
    const int st = smul_common(c, n, sks_out, nullptr, pks_xy_out);        // (uploads the scalars into d_sks again for the base multiplication)
    if (hipMemsetAsync(c->d_sks.p, 0, n * 32, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipGetLastError(); return st ? st : (int)AVRF_ERR_NO_DEVICE; }
    return st;
  });
}
int avrf_points_compress(avrf_ctx *c, size_t n, const uint8_t *in_xy, uint8_t *out) {
  return pointwise(c, n, in_xy && out, [&]() -> int {
    const size_t pl = (size_t)point_len_of(c->suite);
    HIP_TRY(c->d_misc.ensure(n * 64)); HIP_TRY(c->d_out.ensure(n * pl));
    HIP_TRY(hipMemcpyAsync(c->d_misc.p, in_xy, n * 64, hipMemcpyHostToDevice, c->stream));
    AVRF_SINGLE(c->suite, compress(c->d_misc.as<uint8_t>(), (uint32_t)n, c->d_out.as<uint8_t>(), c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->d_out.p, n * pl, hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
  });
}

}  // extern "C"
