// msm.h -- Pippenger bucket MSM over twisted-Edwards curves for gfx950: kernel declarations
// and the host-side engine.  Takes over `VariableBaseMSM::msm_unchecked` at
// src/thin.rs:319, src/pedersen.rs:420, src/utils/common.rs:410-411.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "host_te.h"

namespace avrf {

struct te_pre_raw { uint32_t w[24]; };   // x | y | k, Montgomery, 8 x u32 each
struct te_ext_raw { uint32_t w[32]; };   // x | y | t | z

// thrown by the device engines on a failed HIP call; every extern "C" entry point catches it and returns AVRF_ERR_NO_DEVICE
struct HipFailure { hipError_t err; const char *file; int line; };

// One owned allocation of exactly the bytes asked for, device memory (DevMem) or page-locked host memory (PinMem): freed by its
// destructor on every path out, a throw included (hipFree waits for the device itself, so work in flight on a stream is over before
// the memory goes).  Movable, not copyable: a struct that holds one cannot be copied by accident.  (capi_internal.h DevBuf / PinBuf are
// the same storage under another size rule: staging buffers that round up so that batches of slowly growing size do not reallocate.)
template <bool PINNED> struct OwnedMem {
  void *p = nullptr; size_t cap = 0;
  OwnedMem() = default;
  explicit OwnedMem(size_t bytes) { ensure(bytes); }
  OwnedMem(const OwnedMem &) = delete;
  OwnedMem &operator=(const OwnedMem &) = delete;
  OwnedMem(OwnedMem &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  OwnedMem &operator=(OwnedMem &&o) noexcept { if (this != &o) { (void)release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  ~OwnedMem() { (void)release(); }
  // frees what it holds and allocates exactly `bytes`; the buffer is empty after a failure
  hipError_t reset(size_t bytes) {
    if (hipError_t e = release()) return e;
    if (hipError_t e = PINNED ? hipHostMalloc(&p, bytes) : hipMalloc(&p, bytes)) { p = nullptr; return e; }
    cap = bytes;
    return hipSuccess;
  }
  // grow-only: at least `bytes` afterwards, the contents are NOT kept across a growth.  Throws HipFailure (the buffer is then empty).
  void ensure(size_t bytes) { if (bytes > cap) if (hipError_t e = reset(bytes)) throw HipFailure{e, __FILE__, __LINE__}; }
  hipError_t release() { hipError_t e = !p ? hipSuccess : PINNED ? hipHostFree(p) : hipFree(p); p = nullptr; cap = 0; return e; }
  template <class T = uint32_t> T *as() const { return (T *)p; }
  explicit operator bool() const { return p != nullptr; }
};
using DevMem = OwnedMem<false>;
using PinMem = OwnedMem<true>;
// an owned HIP event, under the same rules
struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(const DevEvent &) = delete;
  DevEvent &operator=(const DevEvent &) = delete;
  DevEvent(DevEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
  DevEvent &operator=(DevEvent &&o) noexcept { if (this != &o) { destroy(); e = o.e; o.e = nullptr; } return *this; }
  ~DevEvent() { destroy(); }
  hipError_t create(unsigned flags = hipEventDefault) { destroy(); return hipEventCreateWithFlags(&e, flags); }
  void destroy() { if (e) (void)hipEventDestroy(e); e = nullptr; }
  operator hipEvent_t() const { return e; }
};

struct MsmPlan {
  int c;         // window bits
  int nwin;      // number of windows: nwin * c >= scalar bits + 1
  int nb;        // buckets per window = 2^(c-1) (signed digits)
  int lpb;       // entries per lane of the last k_accumulate launch (read back from the device plan)
};
MsmPlan msm_plan(size_t n, int scalar_bits);

// What the tail of a chain left in MsmChain::bits_host, vector after vector: `per` bit sums T_p (sum_p 2^p T_p), `per` window triples
// (W_w = P1 + 2^4 P2 + 2^lg P3, sum_w 2^(c w) W_w) or one finished point.  Set with the tail's copy back only; read by msm.hip msm_fold.
// (AFFINE: one finished Montgomery affine point x | y, (0, 0) = infinity -- the segmented G1 chain, read by msm_g1_segments itself.)
struct MsmResult {
  enum Form { NONE, BIT_SUMS, WINDOW_TRIPLES, POINTS, AFFINE } form = NONE;
  size_t vectors = 0;            // scalar vectors (independent MSMs) of the chain
  size_t per = 0;                // entries per vector: bit sums or windows (POINTS: 1)
  size_t words = 0;              // u32 words per point (accumulator layout of the curve policy)
  int lg = 0;                    // WINDOW_TRIPLES: the scale 2^lg of a triple's third point
  size_t stride() const { return per * (form == WINDOW_TRIPLES ? 3 : 1); }   // points per vector
};
// What ONE enqueued launch chain sends back to the host: the results and their description, the device's plan and the timing events of
// the dominant kernel.  Every workspace has one of its own, which serves a lane that runs one chain at a time.  A caller that queues
// several chains behind each other on one lane (stream + workspace; the device-side workspace is reused in stream order) hands in a
// record per chain instead: pool.hip gives every slot one.
struct MsmChain {
  PinMem bits_host, plan_host;   // results | 64 bytes: copy of the workspace's plan_dev
  DevEvent ev0, ev1;             // bracket the dominant kernel (k_accumulate) on the launch stream
  MsmPlan plan = {0, 0, 0, 0};
  MsmResult res;                 // what bits_host holds once the chain is collected
  size_t n = 0;
  bool armed = false;            // enqueued and not collected yet (msm_te_enqueue / msm_te_finish)
  void ensure(size_t bytes);     // the events, the plan words and room for `bytes` of results (grow-only)
  void disarm() { armed = false; }   // whoever gives up on an enqueued chain (an error between enqueue and finish) says so
  void release() { *this = MsmChain(); }
};

// Device workspace owned by a lane; grows on demand, never shrinks, frees itself.
struct MsmWorkspace {
  DevMem keys;       // nwin * n      u16: bucket | sign << 15
  DevMem sorted;     // nwin * n      term index | sign << 31, grouped by (window, bucket)
  DevMem hist;       // nwin * ntiles * nb   per-tile histograms -> per-tile prefixes
  DevMem cnts;       // nwin * nb     entries per bucket
  DevMem offsets;    // nwin * nb     first entry of the bucket in sorted[]
  DevMem win_tot;    // nwin          entries per window
  DevMem lane_base;  // nwin + 1      first k_accumulate lane of every window
  DevMem heavy;      // nwin * nb     buckets fed by many lanes (summed by k_heavy_sum)
  DevMem plan_dev;   // {entries per lane, lanes used, heavy buckets}
  // accumulator arrays (layout of the curve policy: te_ext 128 B, G1 XYZZ 4 * Fq)
  DevMem buckets;    // nwin * nb
  DevMem rc;         // nwin * (rows + cols) partial sums of the bucket reduction
  DevMem part;       // lanes + buckets slots: partial sum of lane t for bucket g at slot t + g
  DevMem bits;       // nwin * c
  MsmChain own;      // the record of a chain that no caller's record was handed in for; its results are sized with `bits`
  bool owns(const MsmChain &rec) const { return &rec == &own; }
  // per lane, read from outside (avrf_kernel_stats, avrf_pool_stats, ring.hip's trace): k_accumulate time and the plan of the chains collected
  double accum_ms_total = 0; uint64_t accum_launches = 0; float accum_ms_last = 0;
  MsmPlan last_plan = {0, 0, 0, 0};
  void ensure(size_t n, const MsmPlan &p, size_t acc_bytes, size_t batch, size_t lanes_max, size_t part_bytes = 0);   // part_bytes: one slot of `part` (0: acc_bytes)
  void release() { *this = MsmWorkspace(); }
};

// MSM of n precomputed device points (Montgomery form) with n plain 256-bit scalars (8 x u32 LE,
// already < r), on `stream`.  Result: extended point on the host.  suite: an id of include/avrf.h (0 .. AVRF_N_SUITES - 1).
int msm_te_device(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t n,
                  MsmWorkspace &ws, hipStream_t stream, HostExt *out);
// the same in two halves: msm_te_enqueue launches the whole kernel chain and the copies back on `stream` and returns without
// waiting; msm_te_finish collects the chain and folds the window sums on the host.  `rec` is the record the chain reports to.
// ws.own: one chain in flight per workspace, and msm_te_finish waits for the stream.  A caller's record (window-sum form only,
// msm_te_pending_supported): msm_te_finish does NOT wait -- the caller has seen an event recorded behind the chain complete.
// msm_te_finish on a record that no enqueue armed returns -1.
int msm_te_enqueue(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t n, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream);
int msm_te_finish(int suite, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream, HostExt *out);
// two or more scalar vectors over the SAME n <= 2048 bases (vector v's scalars start at element v * n) through the single-launch
// form: out[v] = sum_t s_{v,t} P_t.  Synchronises the stream.  Returns -1 when the shape is not the single-launch one.
int msm_te_small_vectors(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t n, size_t n_vectors, MsmWorkspace &ws, hipStream_t stream,
                         HostExt *out);
// n_seg independent MSMs in one chain: segment v is the L bases at d_pre + v * L with the L scalars at d_scalars + 8 v L, out[v] its
// sum.  A zero scalar is never gathered, so segments shorter than L are padded with zero scalars and the padding bases need not be
// initialised.  n_seg >= 8: one Pippenger chain of n_seg * nwin virtual windows with the Horner on the device; fewer: the single-MSM
// path, once per segment.  Synchronises the stream.  Returns -1 (nothing launched) beyond the limits below.
constexpr size_t MSM_SEG_TERMS_MAX = 8191;          // L: keeps nb <= 256, so one reduction kernel (k_bits_direct)
constexpr size_t MSM_SEG_WINDOWS_MAX = 65535;       // n_seg * nwin: the sort kernels carry the virtual window in blockIdx.y
int msm_te_segments(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t L, size_t n_seg, MsmWorkspace &ws, hipStream_t stream, HostExt *out);
// the chain in two halves, under the contract of msm_te_enqueue / msm_te_finish: msm_te_segments_enqueue launches the whole chain and
// the copy back of the n_seg finished points on `stream` and returns without waiting -- always ONE chain, whatever n_seg >= 1 is (no
// per-segment loop below eight) -- and msm_te_segments_finish collects it and folds out[0 .. n_seg).  ws.own: finish waits for the
// stream.  A caller's record (every suite: the device Horner's points fit any record): finish does NOT wait, the caller has seen an
// event recorded behind the chain complete.  Beyond the limits above enqueue returns -1 with nothing launched and the record not armed;
// finish on a record that no enqueue armed returns -1.
int msm_te_segments_enqueue(int suite, const te_pre_raw *d_pre, const uint32_t *d_scalars, size_t L, size_t n_seg, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream);
int msm_te_segments_finish(int suite, MsmWorkspace &ws, MsmChain &rec, hipStream_t stream, HostExt *out);
int msm_segments_window_bits(size_t L);             // the window width msm_plan gives an L-term MSM (host arithmetic)
bool msm_te_pending_supported(int suite);   // msm_te_enqueue: a caller's record is taken by the window-sum form of the chain only

// G1 MSM over a short-Weierstrass curve (curve: 0 BLS12-381, 1 BN254): d_bases = n Montgomery affine
// points (2 * Fq words each, (0,0) = infinity), d_scalars = n plain 256-bit scalars (< r).
// out_xy: canonical affine x || y little-endian (2 * FQ_BYTES), all-zero for the point at infinity.
// batch > 1: `batch` scalar vectors over the same bases (vector b starts at element b * scalar_stride; 0 = n),
// `batch` results in out_xy.  Eight or more vectors over SHARED bases without a window table stay correct through the host fold (the
// device Horner for G1, k_g1_horner_wave, belongs to the segmented chain below); nothing calls it so.
int msm_g1_device(int curve, const uint32_t *d_bases, const uint32_t *d_scalars, size_t n, MsmWorkspace &ws, hipStream_t stream, uint8_t *out_xy,
                  size_t batch = 1, size_t scalar_stride = 0);
// n_seg independent G1 MSMs in ONE Pippenger chain of n_seg * nwin virtual windows, beside msm_te_segments and under its limits
// (MSM_SEG_TERMS_MAX, MSM_SEG_WINDOWS_MAX, 32-bit entry offsets: -1 with nothing launched beyond them): vector v is the L bases at
// d_bases + v * L * 2 Fq words with the L scalars at d_scalars + 8 v L.  A zero scalar is never gathered, so shorter segments are padded
// with zero scalars.  The Horner and the affine conversion run on the device (k_g1_horner_wave, a wave per vector): the n_seg results are
// left as Montgomery affine points ((0, 0) = infinity, the layout launch_pairing_check reads) at d_out when it is given, and come back
// as canonical x || y in out_xy when that is given.  The chain for every n_seg >= 1 (no per-segment loop).  Synchronises the stream.
int msm_g1_segments(int curve, const uint32_t *d_bases, const uint32_t *d_scalars, size_t L, size_t n_seg, MsmWorkspace &ws, hipStream_t stream, uint8_t *out_xy,
                    uint32_t *d_out = nullptr);
int msm_g1_segments_windows(int curve, size_t L);   // windows per vector of that chain (host arithmetic)
// Fixed-base form for MSMs over one shared base set (the KZG SRS): build_g1_table fills
// table[w * n + i] = 2^(c w) * P_i (nwin = ceil((Fr bits + 1) / c) rows); msm_g1_fixed_device then treats all
// windows of a scalar vector as ONE bucket set (n may be smaller than the table's row length `table_stride`).
// d_base_idx != nullptr: sparse form -- entry i of vector b multiplies table base d_base_idx[b * n + i] instead of base i.
void build_g1_table(int curve, const uint32_t *d_bases, size_t n, int c, int nwin, uint32_t *d_table, hipStream_t stream);
int msm_g1_fixed_device(int curve, const uint32_t *d_table, int table_c, size_t table_stride, const uint32_t *d_scalars, size_t n,
                        size_t scalar_stride, MsmWorkspace &ws, hipStream_t stream, uint8_t *out_xy, size_t batch,
                        const uint32_t *d_base_idx = nullptr, int scalars_mont = 0);
// (scalars_mont: the scalar vectors hold Montgomery limbs -- 1 = BLS12-381 Fr, 2 = BN254 Fr -- and the digit kernel converts on load)
// Fixed-base form over a table of ALL multiples (msm.hip "fixed-base MSM over a table of ALL multiples"): for HBM-rich parts.  The table of
// a KZG SRS is built once per (device, SRS) and shared; a commitment is one gathered point per (coefficient, row), no buckets.
struct G1DirectTable {
  uint32_t *d = nullptr;            // affine Montgomery points, 2 * Fq words each; (w, m, i) = (m + 1) 2^(c w) P_i at off[w] + m * n + i
  int curve = 0, c = 0, rows = 0;   // rows: digit rows + the carry row where the recoding can carry out of the top one
  size_t n = 0;                     // bases per row
  uint64_t off[32] = {};            // first point of row w
  uint32_t mult[32] = {};           // multiples held for row w (1 .. mult[w])
  uint64_t points = 0, bytes = 0;
};
size_t g1_direct_table_shape(int curve, size_t n, int c, G1DirectTable *t);      // fills *t (no allocation), returns the table's bytes
void build_g1_direct_table(int curve, const uint32_t *d_bases, size_t n, int c, G1DirectTable *t, hipStream_t stream);   // allocates t->d, synchronises
void free_g1_direct_table(G1DirectTable *t);
// `batch` vectors of n Montgomery-or-plain scalars (vector b starts at element b * scalar_stride) -> `batch` affine results in out_xy
// (d_base_idx != nullptr: sparse form, as msm_g1_fixed_device's)
int msm_g1_direct_device(const G1DirectTable &t, const uint32_t *d_scalars, size_t n, size_t scalar_stride, MsmWorkspace &ws, hipStream_t stream,
                         uint8_t *out_xy, size_t batch, int scalars_mont = 0, const uint32_t *d_base_idx = nullptr);
// n compressed G1 points (FQ_BYTES each, ark-serialize) -> canonical x || y little-endian + ok[i] (0 invalid, 1 point, 2 infinity)
void launch_g1_decompress(int curve, const uint8_t *d_comp, size_t n, uint8_t *d_out_xy, uint8_t *d_ok, hipStream_t stream);
void launch_g1_bases(int curve, const uint8_t *d_xy, size_t n, uint32_t *d_out, uint32_t *d_flag, hipStream_t stream);
// sets bit 1 of *d_flag when one of the n Montgomery affine bases (as launch_g1_bases writes them) is outside the prime-order
// subgroup (BLS12-381: endomorphism test; BN254: cofactor 1, no-op)
// (d_rec_status != nullptr: record i / ppr of a failing point gets status 2)
void launch_g1_subgroup_check(int curve, const uint32_t *d_bases, size_t n, uint32_t *d_flag, hipStream_t stream, int32_t *d_rec_status = nullptr,
                              uint32_t ppr = 1);
// the same test over records of UNEQUAL length: entry i < n tests base d_point[i] (an index into d_bases, which the caller keeps inside
// the array) and gives record d_rec_of[i] (inside d_rec_status) status 2 when it fails; bit 1 of *d_flag as above
void launch_g1_subgroup_check_list(int curve, const uint32_t *d_bases, const uint32_t *d_point, const uint32_t *d_rec_of, size_t n, uint32_t *d_flag,
                                   int32_t *d_rec_status, hipStream_t stream);
// per item (16-lane group): point 0 = sum_{t < split} s_t P_t, point 1 = sum_{split <= t < tpi} s_t P_t over the item's tpi <= 16
// (base, scalar) pairs; out: n_items x 2 Montgomery affine points.  glv_split_scalars (BLS12-381 only): every 32-byte scalar slot
// holds k mod z^2 | (k div z^2) << 128 (g1_glv_split_bls) and the kernel takes the 128-doubling GLV chain.
void launch_g1_lincomb(int curve, const uint32_t *d_bases, const uint32_t *d_scalars, size_t n_items, uint32_t tpi, uint32_t split, uint32_t *d_out,
                       hipStream_t stream, bool glv_split_scalars = false);
// k (256-bit little-endian limbs, < 2^255) -> k mod z^2 in limbs 0..1, k div z^2 in limbs 2..3, z = 0xd201000000010000 (host)
void g1_glv_split_bls(uint64_t k[4]);

// canonical affine bytes (x||y LE32) -> te_pre (device); flags[i] |= 1 if a coordinate >= q, |= 2 if off-curve (when check_curve)
// (mont_in: the coordinates are Montgomery limbs already -- avrf_msm_te_mont)
void launch_pre_from_affine(int suite, const uint8_t *d_xy, size_t n, te_pre_raw *d_pre, uint32_t *d_flag,
                            int check_curve, hipStream_t stream, int mont_in = 0);
// n scalars as Montgomery limbs of the suite's Fr -> plain 256-bit integers, in place; *d_flag |= 4 for a limb value >= r
void launch_scalars_from_mont(int suite, uint32_t *d_scalars, size_t n, uint32_t *d_flag, hipStream_t stream);

}  // namespace avrf
