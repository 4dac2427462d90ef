/*
 * avrf.h -- C ABI of the MI355X-native batched VRF engine (libavrf.so).
 *
 * Drop-in boundary for the hot path of davxy/ark-vrf.  The reference has no
 * FFI of its own (`#![deny(unsafe_code)]`, src/lib.rs:95); each entry point below names the
 * reference interface it replaces (paths relative to the reference repo).  A Rust shim
 * re-implementing `thin::{Prover,Verifier,BatchVerifier}` / `pedersen::{...}` for
 * `Secret<S>` / `Public<S>` binds exactly these symbols.
 *
 * Conventions
 *  - plain pointers and sizes; the caller owns every buffer; handles are opaque.
 *  - scalars: 32-byte little-endian canonical integers (< group order), as
 *    `CanonicalSerialize` writes `ScalarField` (src/testing.rs:25-34).
 *  - "xy" points: 64 bytes, LE32(x) || LE32(y), canonical (non-Montgomery) affine
 *    twisted-Edwards coordinates, identity = (0, 1).  This is what a caller holding
 *    arkworks `Affine { x, y }` values has after deserialisation.
 *  - "compressed" points: 32 bytes, ark-serialize compressed form (LE32(y), bit 255 = x sign).
 *  - status codes mirror `ark_vrf::Error` (src/lib.rs:135-147).
 *  - every call runs on the context's own HIP stream; one context per host thread.
 *  - no CPU fallback: creating a context fails (AVRF_ERR_NO_DEVICE) without a gfx950 device.
 *  - host requirement: the library's host code is built for x86-64-v3 (AVX2, BMI2 -- the sequential SHA-512 weight transcript
 *    runs twice as fast with rorx / mulx); every MI355X host platform has it, an older CPU dies with SIGILL at load, not with
 *    a status code.  (The optional 8-lane multi-buffer hash additionally needs AVX-512 and IS checked at run time.)
 *  - short-Weierstrass suite (AVRF_SUITE_SECP256R1_SHA256_TAI): xy points are the curve's affine points, identity = 64 zero bytes.
 */
#ifndef AVRF_H
#define AVRF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  AVRF_OK = 0,                     /* Ok(())                                   */
  AVRF_VERIFICATION_FAILURE = 1,   /* Error::VerificationFailure               */
  AVRF_INVALID_DATA = 2,           /* Error::InvalidData                       */
  AVRF_RING_CAPACITY_EXCEEDED = 3, /* Error::RingCapacityExceeded              */
  AVRF_SRS_LOOKUP_FAILED = 4,      /* Error::SrsLookupFailed                   */
  AVRF_ERR_NO_DEVICE = -1,         /* no HIP device / kernels not loadable     */
  AVRF_ERR_BAD_ARG = -2
};

enum {
  AVRF_SUITE_BANDERSNATCH_SHA512_ELL2 = 0, /* src/suites/bandersnatch.rs:62-105 */
  AVRF_SUITE_BABYJUBJUB_SHA512_TAI = 1,    /* src/suites/baby_jubjub.rs:56-95   */
  AVRF_SUITE_JUBJUB_SHA512_TAI = 2,        /* src/suites/jubjub.rs:56-95 (ring proofs over BLS12-381) */
  AVRF_SUITE_ED25519_SHA512_TAI = 3,       /* src/suites/ed25519.rs:44-66 (Tiny / Thin / Pedersen; no RingSuite: avrf_ring_* -> BAD_ARG) */
  AVRF_SUITE_BANDERSNATCH_SHAKE128_ELL2 = 5, /* src/suites/bandersnatch_shake128.rs: suite 0's curve, Shake128Transcript, expand_message_xof */
  AVRF_SUITE_TESTING_SHA256_TAI = 6,        /* src/suites/testing.rs: the crate's own test suite (edwards25519, HashTranscript<Sha256>; no ring) */
  AVRF_SUITE_SECP256R1_SHA256_TAI = 7,      /* src/suites/secp256r1.rs:49-70: NIST P-256 (a = -3 short Weierstrass, cofactor 1, 256-bit fields with the
                                             * top bit set), HashTranscript<Sha256>; Tiny / Thin / Pedersen, no RingSuite.  xy points are the curve's own
                                             * affine points, the identity is the all-zero 64 bytes; compressed form: 33 bytes (avrf_point_len) */
  AVRF_SUITE_BANDERSNATCH_SW_SHA512_TAI = 4 /* src/suites/bandersnatch_sw.rs:60-112: Bandersnatch in its short-Weierstrass presentation.
                                             * xy points are the TEMapping (src/utils/te_sw_map.rs) of the suite's SWAffine; the compressed
                                             * form (avrf_points_*, *_wire) is its 33-byte serialize_compressed: see avrf_point_len */
};

typedef struct avrf_ctx avrf_ctx;

/* Library / build identification (no GPU needed). */
const char *avrf_version(void);
/* Number of visible HIP devices (0 when there is none; never initialises a context). */
int avrf_device_count(void);
/* How host threads wait for `device`: on = 1 sleeps in the driver until the stream is done (hipDeviceScheduleBlockingSync), on = 0
 * restores the runtime's default (a yielding spin).  A process that runs many contexts under a CPU quota wants 1: a spinning waiter
 * burns the cores the weight hashes of the other contexts need.  Device-wide, so the caller decides -- once, early, before the
 * contexts are created (that is the tested use); AVRF_OK / AVRF_ERR_NO_DEVICE. */
int avrf_device_set_blocking_sync(int device, int on);

/* One engine instance: suite parameterisation (trait Suite, src/lib.rs:177-250) + one HIP
 * stream + device workspace on `device`. */
int avrf_ctx_create(int suite, int device, avrf_ctx **out);
void avrf_ctx_destroy(avrf_ctx *ctx);

/* Input validation of the verifier entry points (SURVEY.md 8b "Input validation").  The reference's verifiers ASSUME points
 * on the curve and in the prime-order subgroup (src/thin.rs:78-94, src/pedersen.rs:103-120): its typed points have passed
 * CanonicalDeserialize with Validate::Yes / the checked constructors (src/lib.rs:410-433,440-444,471-494).  This ABI takes raw
 * coordinates, so the caller says who validates:
 *   level 0 (default)  "_unchecked": the caller guarantees on-curve subgroup points (e.g. they came from
 *                      avrf_points_decompress(validate = 1) or from an arkworks value); off-curve input gives undefined verdicts;
 *   level 1            every pk / I/O / proof point of avrf_{thin,pedersen}_{verify,batch_verify,batch_run,batch_challenges} must
 *                      be on the curve, else AVRF_INVALID_DATA (per item for the *_verify calls) before any equation is evaluated;
 *   level 2            additionally r * P = O for every point (one 253-bit scalar multiplication per point: opt-in).
 * The identity checks of the verifiers (src/thin.rs:140-149,266-271, src/pedersen.rs:204-213,348-353) are unconditional.
 *
 * PRIME-ORDER-SUBGROUP MEMBERSHIP IS A HARD PRECONDITION of every prove / verify / batch-verify entry point at levels 0 and 1
 * and of the wire flavour with validate = 0 -- exactly where the reference says "the caller must ensure ... otherwise the
 * behaviour is undefined" (src/thin.rs:78-94).  The kernels exploit it: scalars are reduced mod r before they meet a point
 * (one-pair forms (s z) I, (c z) O) and Bandersnatch multiplies through the GLV endomorphism, k P = k1 P + k2 psi(P) (glv.h),
 * both of which equal the reference's literal products only inside the subgroup.  For an on-curve point with a 2- or
 * 4-torsion component the verdict is unspecified and MAY DIFFER from the reference's: a consensus-critical caller that does
 * not hold validated points must use level 2 / validate = 1, which answers AVRF_INVALID_DATA for such a point before any
 * equation (tests/test_gpu_wire.py::test_torsion_points).  avrf_scalar_mul and avrf_msm_te compute literal products for
 * any curve point. */
int avrf_ctx_set_validation(avrf_ctx *ctx, int level);

/* <S::Affine as AffineRepr>::Group::msm_unchecked(&bases, &scalars)
 * (call sites src/thin.rs:319, src/pedersen.rs:420, src/utils/common.rs:410-411).
 * bases_xy: n x 64, scalars: n x 32, out_xy: normalised result (64 bytes).
 * "unchecked": no subgroup check; off-range coordinates / scalars give AVRF_INVALID_DATA. */
int avrf_msm_te(avrf_ctx *ctx, size_t n, const uint8_t *bases_xy, const uint8_t *scalars, uint8_t out_xy[64]);
/* The zero-copy flavour of the same call: everything as arkworks keeps it IN MEMORY -- bases n x Affine { x, y },
 * each coordinate an Fp<MontBackend, 4> (four little-endian u64 limbs, Montgomery form, R = 2^256); scalars n x ScalarField in
 * the same form; result Montgomery x || y.  A shim can pass `bases.as_ptr()` / `scalars.as_ptr()` of the slices handed to
 * `msm_unchecked` (the crate's Affine / Fp structs are plain limb arrays; the shim asserts their size: 64 / 32 bytes).
 * A limb value >= the modulus gives AVRF_INVALID_DATA.  The canonical-bytes flavour above remains the tested contract of the
 * other entry points (it is what the reference's vectors pin). */
int avrf_msm_te_mont(avrf_ctx *ctx, size_t n, const uint8_t *bases_mont_xy, const uint8_t *scalars_mont, uint8_t out_mont_xy[64]);

/* <E::G1 as VariableBaseMSM>::msm on the suite's pairing curve (BLS12-381 for Bandersnatch, BN254 for
 * Baby-JubJub) -- the KZG commit/open MSMs inside w3f-ring-proof reached from src/ring.rs:220,404,416,731.
 * bases_xy: n x (2*FQ) bytes, canonical little-endian x || y (FQ = 48 / 32), all-zero = point at infinity;
 * scalars: n x 32 (< r of the pairing curve); out_xy: same point format. */
int avrf_g1_msm(avrf_ctx *ctx, size_t n, const uint8_t *bases_xy, const uint8_t *scalars, uint8_t *out_xy);
/* n_seg independent <E::G1 as VariableBaseMSM>::msm calls (the same call sites, src/ring.rs:220,404,416,731) of L terms each in one
 * call, beside avrf_g1_msm: segment v is bases_xy[v L ..], scalars[v L ..]; out_xy: n_seg points in the format above.  ONE launch
 * chain for every n_seg >= 1 (no per-segment loop), with the Horner and the affine conversion on the device: it is the probe of the
 * chain avrf_ring_batch_verify_segments runs.  A coordinate >= p or a scalar >= r gives AVRF_INVALID_DATA; L > AVRF_SEGMENT_TERMS_MAX,
 * n_seg * L > AVRF_SEGMENTS_PADDED_TERMS_MAX or n_seg * windows(L) > AVRF_SEGMENTS_WINDOWS_MAX gives AVRF_ERR_BAD_ARG; L == 0 writes
 * n_seg points at infinity, n_seg == 0 nothing, both AVRF_OK. */
int avrf_g1_msm_segments(avrf_ctx *ctx, size_t n_seg, size_t L, const uint8_t *bases_xy, const uint8_t *scalars, uint8_t *out_xy);

/* thin::BatchVerifier::{new, push*, verify}  (src/thin.rs:188-326).
 * n items; item j has io_counts[j] VRF I/O pairs; ios_xy holds sum(io_counts) pairs as
 * input_xy(64) || output_xy(64); ads holds the concatenated additional-data strings with
 * lengths ad_lens[j]; proofs: R_xy(64) || s(32) per item.
 * Returns AVRF_OK, AVRF_INVALID_DATA (identity pk / io point, or malformed encodings),
 * or AVRF_VERIFICATION_FAILURE.  Empty batch => AVRF_OK (src/thin.rs:262-264). */
int avrf_thin_batch_verify(avrf_ctx *ctx, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy,
                           const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                           const uint8_t *proofs);

/* Two-phase form of the same call for callers that keep a batch resident in HBM
 * (bench.py times avrf_thin_batch_run only): stage copies the batch to the device,
 * run performs prepare + verify on the staged batch and may be called repeatedly. */
int avrf_thin_batch_stage(avrf_ctx *ctx, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy,
                          const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                          const uint8_t *proofs);
int avrf_thin_batch_run(avrf_ctx *ctx);
/* The run of a staged batch (Thin or Pedersen) in three non-overlapping calls, for a host thread that keeps several contexts
 * in flight: BatchVerifier::verify (src/thin.rs:257-325, src/pedersen.rs:341-426) is device work, then the sequential
 * weight transcript on the host (src/thin.rs:274-279), then device work again.
 *   avrf_batch_run_begin  enqueues validation + the prepare kernel + the copies back on the context's stream and returns;
 *   avrf_batch_run_hash   waits for them, returns AVRF_INVALID_DATA as the one-call form would, hashes the weight transcript
 *                         on the calling thread, enqueues the terms kernel and the MSM, returns without waiting;
 *   avrf_batch_run_end    waits for the MSM and returns the verdict (AVRF_OK / AVRF_VERIFICATION_FAILURE).
 * Results are those of avrf_thin_batch_run / avrf_pedersen_batch_run (which are these three in a row).  Between begin and
 * end the run owns the context: EVERY other entry point that takes the context (staging, MSMs, challenges / partials, scalar
 * multiplications, the point codecs, the per-item provers / verifiers, the avrf_ring_* calls of setups created from it)
 * returns AVRF_ERR_BAD_ARG and leaves the run undisturbed; _begin / _hash / _end out of order return AVRF_ERR_BAD_ARG too;
 * an error status from _hash or _end ends the run (the context is idle again). */
int avrf_batch_run_begin(avrf_ctx *ctx);
int avrf_batch_run_hash(avrf_ctx *ctx);
int avrf_batch_run_end(avrf_ctx *ctx);

/* ---- thin::BatchVerifier over a table of shared points.
 * Block and seal verification by a known validator set: a few hundred to a few thousand distinct keys, a handful of distinct
 * inputs.  The reference merges one shared base, the generator, into a single MSM term (src/thin.rs:303,316-317); here every
 * base that several items share is merged the same way -- the scalars of a row's references are added in the scalar field on
 * the device, which leaves sum scalar * base, and so the verdict, unchanged.  The MSM has n + tot_io + n_shared + 1 terms
 * instead of 2 n + 2 tot_io + 1, and an item sends 2 indices instead of 128 bytes of key and input.
 *
 * shared_xy: n_shared x 64 (x || y).  pk_index[j] is the row that is item j's public key; input_index[k] the row that is the
 * input of I/O pair k (k runs over sum(io_counts), item-major, as ios_xy does); outputs_xy: sum(io_counts) x 64; everything
 * else as avrf_thin_batch_stage.  A row may be referenced any number of times, by keys and inputs alike, or not at all.
 *
 * A batch staged this way runs through every run entry point unchanged (avrf_thin_batch_run, avrf_batch_run_begin / _hash /
 * _end, avrf_thin_batch_challenges / _partial, avrf_batch_last_terms; the pool's wait / resubmit / cycle), and its verdict is
 * the one avrf_thin_batch_verify gives for the EXPANDED batch, every index replaced by its row: AVRF_INVALID_DATA for an
 * identity key or I/O point (src/thin.rs:266-271), AVRF_OK for the empty batch.
 *   checks    the identity check applies to REFERENCED rows only, the canonical-range check to every row; under
 *             avrf_ctx_set_validation / avrf_pool_set_validation 1 or 2 the table is validated once per row (not once per
 *             reference), the outputs and R as in a plain batch.
 *   indices   an index >= n_shared (or n_shared == 0 with n > 0) is AVRF_ERR_BAD_ARG: nothing is staged, the context and
 *             what it had staged stay usable.  avrf_pool_submit_shared checks the indices on the calling thread, before it
 *             returns a ticket.  No kernel reads outside the table whatever the indices say.
 *   terms     (avrf_batch_last_terms; this layout is ABI) for item j with io0 = io_counts[0] + .. + io_counts[j - 1]:
 *             (R_j, w_j) at j + io0; (O_ji, w c z_i) at j + io0 + 1 + i; row r at n + tot_io + r with the scalar
 *             sum of w c z0 over the items whose key is r  -  sum of w s z_i over the pairs whose input is r   (mod r_order),
 *             0 for a row nothing refers to; (G, g) last.  avrf_thin_shared_n_terms = n + tot_io + n_shared + 1 (host
 *             arithmetic only, no device needed).
 * Measured (tools/shared_bench.py): 1 024 keys + 3 inputs, 65 536 items: 1.34 x the plain call resident and
 * 1.30 x from page-locked host buffers.  USE THE PLAIN CALL WHEN NOTHING IS SHARED: with every point its own row the term count
 * is the plain one and staging the table from the host costs a quarter of the throughput (0.74 x; resident runs 1.00 x). */
int avrf_thin_batch_stage_shared(avrf_ctx *ctx, size_t n, size_t n_shared, const uint8_t *shared_xy,
                                 const uint32_t *pk_index, const uint32_t *input_index, const uint8_t *outputs_xy,
                                 const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs);
size_t avrf_thin_shared_n_terms(size_t n, size_t tot_io, size_t n_shared);
/* The same batch from wire bytes, for a caller that holds its validator keys and slot inputs as the bytes it received.  With
 * L = avrf_point_len(suite): shared is n_shared x L (`serialize_compressed` points), outputs sum(io_counts) x L, proofs
 * n x (L + 32) laid out R || s (the Thin wire proof of avrf_thin_batch_stage_wire); pk_index, input_index, io_counts, ads and
 * ad_lens exactly as in avrf_thin_batch_stage_shared.  avrf_thin_batch_verify_shared_wire is stage + avrf_thin_batch_run.
 *   indices   checked on the host before anything is staged: a failure is AVRF_ERR_BAD_ARG and the context keeps what it had
 *             staged.  avrf_pool_submit_shared_wire checks on the submitting thread, before a ticket exists.
 *   decoding  one kernel launch per staging decodes EVERY table row -- referenced or not --, every output and every R, each
 *             once: a row costs one square root however many items refer to it.  validate = 0: the point must decode
 *             (Validate::No).  validate != 0: it must also be non-identity and in the prime-order subgroup (Validate::Yes,
 *             src/lib.rs:410-433).  THIS DIFFERS FROM THE x || y FLAVOUR ABOVE: under validate != 0 an identity row is refused
 *             even when nothing refers to it, because deserialising a key or an input with Validate::Yes refuses the identity.
 *             With validate = 0 an identity row decodes; the run then refuses it (AVRF_INVALID_DATA) only if it is
 *             referenced, as in the x || y flavour.
 *   failure   a point that fails makes the stage call return AVRF_INVALID_DATA with nothing staged (a following run answers
 *             as after a failed avrf_thin_batch_stage_wire); in the pool the verdict is AVRF_INVALID_DATA, which
 *             avrf_pool_resubmit with from_host = 0 and the cycle mode repeat, while from_host = 1 stages again from the
 *             eight host buffers.
 *   after     the staged batch is a shared-table batch in every respect: term layout and avrf_thin_shared_n_terms as above,
 *             every run entry point, the pool's wait / resubmit / cycle.  avrf_ctx_set_validation keeps acting on the staged
 *             x || y points at every run, independently of `validate`. */
int avrf_thin_batch_stage_shared_wire(avrf_ctx *ctx, size_t n, size_t n_shared, const uint8_t *shared,
                                      const uint32_t *pk_index, const uint32_t *input_index, const uint8_t *outputs,
                                      const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                                      const uint8_t *proofs, int validate);
int avrf_thin_batch_verify_shared_wire(avrf_ctx *ctx, size_t n, size_t n_shared, const uint8_t *shared,
                                       const uint32_t *pk_index, const uint32_t *input_index, const uint8_t *outputs,
                                       const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                                       const uint8_t *proofs, int validate);

/* ---- thin::BatchVerifier over SEGMENTS of one staged batch: one verdict per group of items (src/thin.rs:188-326).
 * n_seg independent BatchVerifiers over consecutive runs of the staged items -- segment v covers the next seg_items[v] items,
 * the counts sum to n -- each with its own weight transcript (src/thin.rs:274-279 over ITS items only) and its own verdict, in
 * one pass over the device: one prepare launch, one copy back, the n_seg transcripts hashed in groups, one terms pass, ONE MSM
 * chain of n_seg * windows virtual windows, n_seg points back.  For a caller whose big batch failed (segments of a few hundred
 * items locate the bad ones; avrf_thin_verify then runs on the failing segments only) and for a caller with many small
 * batches (a block importer: one verdict per block).
 *   statuses  status_out[v] is what avrf_thin_batch_verify answers for segment v's items alone: AVRF_OK,
 *             AVRF_VERIFICATION_FAILURE or AVRF_INVALID_DATA; an empty segment is AVRF_OK (src/thin.rs:262-264).  An identity
 *             key or I/O point, a non-canonical coordinate, a scalar >= r, or under avrf_ctx_set_validation 1 / 2 a point
 *             that fails, marks ITS segment AVRF_INVALID_DATA and no other.  The call itself returns AVRF_OK whenever the
 *             statuses were written.
 *   limits    a segment has at most AVRF_SEGMENT_TERMS_MAX MSM terms (2 items + 2 pairs + 1); the padded layout at most
 *             AVRF_SEGMENTS_PADDED_TERMS_MAX terms (n_seg * L, L = the longest segment's term count: about 1.7 KB of device
 *             workspace per padded term at the narrowest window); n_seg * windows(L) at most AVRF_SEGMENTS_WINDOWS_MAX.
 *   refusals  AVRF_ERR_BAD_ARG, with the context and its staged batch untouched and usable: counts that do not sum to n, a
 *             limit exceeded, nothing staged, a Pedersen batch staged, a shared-table batch staged (its rows are merged over the
 *             whole batch: avrf_thin_batch_run_shared_segments sums them per segment), a call between avrf_batch_run_begin and _end.
 *   after     avrf_thin_batch_run on the same staging gives its usual verdict and avrf_batch_last_terms its usual terms: the
 *             segmented terms live in buffers of their own.
 *   terms     (avrf_thin_segment_terms; this layout is ABI) segment v's terms are those of avrf_batch_last_terms for a batch
 *             of just its items, in the reference's order (src/thin.rs:287-317): R, pk, (O, I).., (G, g_v) last.
 * avrf_thin_batch_run_segments works on the batch the context holds (avrf_thin_batch_stage / avrf_thin_batch_stage_wire);
 * avrf_thin_batch_verify_segments / _wire are stage + run_segments with the arguments of avrf_thin_batch_verify / _wire (a
 * staging error is returned as it is and no status is written).
 * Runtime (tools/segments_bench.py; one context, 65 536 one-pair items resident): 256 segments of 256 items
 * 2.43 ms (26.9-27.0 M items/s), 1 024 x 64 3.3 ms, 64 x 1 024 2.8 ms; the same 256 batches as separate pool submissions 33 ms.
 * avrf_thin_verify on the same items, one verdict per ITEM, takes 2.35-2.39 ms: THE SEGMENTED CALL DOES NOT BEAT IT.  Use segments
 * to locate a few bad items in a large batch (then avrf_thin_verify on the failing segments only) and for many small batches;
 * use avrf_thin_verify when most items are suspect.  avrf_last_timing after a segmented run: [1] prepare + wait, [2] the
 * transcripts, [3] terms launches, [4] MSM chain + wait, [0] their sum (microseconds). */
enum {
  AVRF_SEGMENT_TERMS_MAX = 8191,
  AVRF_SEGMENTS_PADDED_TERMS_MAX = 1 << 20,
  AVRF_SEGMENTS_WINDOWS_MAX = 65535
};
int avrf_thin_batch_run_segments(avrf_ctx *ctx, size_t n_seg, const uint32_t *seg_items, int32_t *status_out);
int avrf_thin_batch_verify_segments(avrf_ctx *ctx, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy,
                                    const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                                    const uint8_t *proofs, size_t n_seg, const uint32_t *seg_items, int32_t *status_out);
int avrf_thin_batch_verify_segments_wire(avrf_ctx *ctx, size_t n, const uint8_t *pks, const uint8_t *ios,
                                         const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                                         const uint8_t *proofs, int validate, size_t n_seg, const uint32_t *seg_items,
                                         int32_t *status_out);
/* The layout of a segmented run (src/thin.rs:188-326: term counts of n_seg BatchVerifiers), host arithmetic only, no device:
 * out = { L, padded terms n_seg * L, total terms (the segments' own counts added up), window bits of the L-term MSMs }.
 * io_counts has n entries.  AVRF_ERR_BAD_ARG when the counts do not sum to n or a limit above is exceeded. */
int avrf_thin_segments_layout(size_t n, size_t n_seg, const uint32_t *seg_items, const uint32_t *io_counts, uint64_t out[4]);
/* The MSM terms the last avrf_thin_batch_run_segments built for segment `seg` (src/thin.rs:188-326; tests): returns their
 * number and fills bases_xy (count x 64) / scalars (count x 32) when given; 0 for an empty segment, without a segmented run on
 * the current staging, or for a busy context. */
size_t avrf_thin_segment_terms(avrf_ctx *ctx, size_t seg, uint8_t *bases_xy, uint8_t *scalars);
/* n_seg independent msm_unchecked calls (src/thin.rs:319) of L terms each in one call, beside avrf_msm_te: segment v is
 * bases_xy[v L ..], scalars[v L ..]; out_xy: n_seg x 64.  n_seg >= 8 runs as one chain, fewer as n_seg single MSMs.
 * L <= AVRF_SEGMENT_TERMS_MAX and the other limits above, else AVRF_ERR_BAD_ARG. */
int avrf_msm_te_segments(avrf_ctx *ctx, size_t n_seg, size_t L, const uint8_t *bases_xy, const uint8_t *scalars, uint8_t *out_xy);
/* Test probe: the same MSMs through the two halves the pool's segmented jobs use (enqueue the chain, collect it later): ONE chain
 * whatever n_seg >= 1 is, the windows limit holding for every n_seg.  own_record != 0: the context's own result record; 0: a record
 * of the call's own, as a pool slot hands in.  Results and refusals as avrf_msm_te_segments. */
int avrf_msm_te_segments_chain(avrf_ctx *ctx, size_t n_seg, size_t L, const uint8_t *bases_xy, const uint8_t *scalars, int own_record,
                               uint8_t *out_xy);

/* ---- pedersen::BatchVerifier over SEGMENTS of one staged batch (src/pedersen.rs:303-426): the five calls above for the Pedersen
 * verifier, with the same meaning, limits and refusals.  n_seg independent BatchVerifiers over consecutive runs of the staged
 * Pedersen items, each with its own weight transcript (SUITE_ID || 0x50 || c || s || sb of ITS items, src/pedersen.rs:361-367;
 * 32 weight bytes per item, t then u, :373-381) and its own verdict: one prepare launch, one copy back, the transcripts hashed
 * sixteen at a time, one terms pass, ONE MSM chain.
 *   statuses  status_out[v] is what avrf_pedersen_batch_verify answers for segment v's items alone; an empty segment is AVRF_OK
 *             (src/pedersen.rs:343-345).  An identity key commitment Yb or supplied I/O point (:348-353; the MERGED pair of an
 *             item without pairs is the identity legitimately, :264-267), a non-canonical coordinate, s or sb >= r, or under
 *             avrf_ctx_set_validation 1 / 2 a point that fails, marks ITS segment AVRF_INVALID_DATA and no other.
 *   layout    (avrf_pedersen_segment_terms; ABI) segment v covers the staged items [seg_off[v], seg_off[v + 1]) and has
 *             n_v = 5 items + 2 terms at [v L, v L + n_v) of arrays of n_seg L terms, L the largest n_v, in the reference's order
 *             (src/pedersen.rs:383-418): per item O, Ok, I, Yb, R, then (G, -sum u s), then (B, -sum u sb) last -- the terms of
 *             avrf_batch_last_terms for a batch of just its items.  Scalars behind n_v are zero and their bases unwritten; an
 *             empty segment has no terms.
 *   limits    the three above through the same check: 5 items + 2 <= AVRF_SEGMENT_TERMS_MAX makes 1 637 items (8 187 terms) the
 *             longest Pedersen segment.
 *   refusals  AVRF_ERR_BAD_ARG with the staging untouched: nothing staged, a Thin batch staged (and avrf_thin_batch_run_segments
 *             refuses a Pedersen one), counts that do not sum to n, a limit exceeded, a call between avrf_batch_run_begin and
 *             _end.  avrf_pedersen_batch_run afterwards gives its usual verdict and avrf_batch_last_terms its usual terms.
 * avrf_last_timing keeps the slots of the Thin call.
 * Runtime (tools/segments_bench.py --kind=pedersen; one context, 65 536 one-pair items resident):
 * 256 segments of 256 items 2.57-2.66 ms (24.6-25.5 M items/s), 1 024 x 64 3.5-3.7 ms, 64 x 1 024 3.0-3.9 ms; the same 256 batches as
 * separate pool submissions 41-52 ms (15-20 x slower).  avrf_pedersen_verify on the same items, one verdict per ITEM and staged
 * from the host, takes 2.83-3.42 ms: ON A RESIDENT BATCH THE SEGMENTED CALL BEATS IT (ranges apart, 20 % between the means); staged
 * from the host on every call (avrf_pedersen_batch_verify_segments, 3.25-3.30 ms) it does not.  Use segments for many small
 * batches and to locate a few bad items in a batch the context already holds (then avrf_pedersen_verify on the failing segments
 * only); use avrf_pedersen_verify when the items come from the host and most are suspect. */
int avrf_pedersen_batch_run_segments(avrf_ctx *ctx, size_t n_seg, const uint32_t *seg_items, int32_t *status_out);
int avrf_pedersen_batch_verify_segments(avrf_ctx *ctx, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts,
                                        const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, size_t n_seg,
                                        const uint32_t *seg_items, int32_t *status_out);
int avrf_pedersen_batch_verify_segments_wire(avrf_ctx *ctx, size_t n, const uint8_t *ios, const uint32_t *io_counts,
                                             const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate,
                                             size_t n_seg, const uint32_t *seg_items, int32_t *status_out);
/* ---- pedersen::BatchVerifier over a table of shared INPUTS.
 * The Pedersen proof is the half of a ring-VRF proof that runs here, and the ticket workload makes tens of thousands of them over
 * the same two or three VRF inputs.  The reference merges the two bases every item shares, G and BLINDING_BASE, into one MSM term
 * each (src/pedersen.rs:387-418); here the inputs get the same treatment: the scalars of a row's references are added in the scalar
 * field on the device, which leaves sum scalar * base, and so the verdict, unchanged.  The MSM has 4 n + n_shared + 2 terms instead
 * of 5 n + 2, an item carries four points instead of five, and it sends a 4-byte index instead of 64 bytes of input.
 *
 * The arguments are those of avrf_thin_batch_stage_shared without pk_index (a Pedersen item has no public key): shared_xy is
 * n_shared x 64 (x || y); input_index[k] is the row that is the input of I/O pair k (k runs over sum(io_counts), item-major);
 * outputs_xy: sum(io_counts) x 64; proofs: n x 256 as in avrf_pedersen_batch_stage.  A row may be referenced any number of times
 * or not at all.
 *
 * A batch staged this way runs through every run entry point unchanged (avrf_pedersen_batch_run, avrf_batch_run_begin / _hash /
 * _end, avrf_pedersen_batch_challenges / _partial, avrf_batch_last_terms; the pool's wait / resubmit, both from_host values, /
 * cycle), and its verdict is the one avrf_pedersen_batch_verify gives for the EXPANDED batch, every index replaced by its row;
 * AVRF_OK for the empty batch.
 *   checks    a REFERENCED identity row is AVRF_INVALID_DATA (io_identity, src/pedersen.rs:278,348-353), an unreferenced one is
 *             fine; a non-canonical coordinate in ANY row is AVRF_INVALID_DATA.  Under avrf_ctx_set_validation /
 *             avrf_pool_set_validation 1 or 2 the table is validated once per row (not once per reference), the outputs and the
 *             proof points as in a plain batch.
 *   no pairs  an item without pairs is legal: its merged pair is the identity legitimately (:264-267) and it contributes to no
 *             row.  n_shared == 0 is accepted exactly when sum(io_counts) == 0; nothing is shared then and the batch is staged as
 *             avrf_pedersen_batch_stage stages it (plain 5 n + 2 terms, segments allowed).
 *   indices   an index >= n_shared is AVRF_ERR_BAD_ARG, found on the host before anything is staged: the context keeps what it
 *             had staged.  avrf_pool_submit_pedersen_shared checks on the submitting thread, before a ticket exists.  No kernel
 *             reads outside the table whatever the indices say.
 *   terms     (avrf_batch_last_terms; this layout is ABI) item j has four terms at 4 j + k: k = 0 (O_merged, t c), 1 (Ok, t),
 *             2 (Yb, u c), 3 (R, u).  Row r is at 4 n + r with the scalar  - sum of t_j s_j z_ji over the pairs whose input is r
 *             (mod r_order), z_j0 = 1 and z_ji, i >= 1, the item's delinearisation scalars (src/utils/common.rs:345-363,389-419);
 *             0 for a row nothing refers to.  (G, -sum u s) is at 4 n + n_shared and (BLINDING_BASE, -sum u sb) last.
 *             avrf_pedersen_shared_n_terms = 4 n + n_shared + 2 (host arithmetic only, no device needed).
 *   pairs     the merged input of an item with several pairs is sum z_i I_i, so its term -t s I_merged IS the contributions
 *             -t s z_i to the pairs' rows (the reference's own linearity); the merged OUTPUT stays one term per item.
 *   segments  avrf_pedersen_batch_run_segments refuses a shared-table staging (AVRF_ERR_BAD_ARG: the rows are merged over the whole
 *             batch); avrf_pedersen_batch_run afterwards still answers.  avrf_pedersen_batch_run_shared_segments takes it.
 *   restaging a later avrf_pedersen_batch_stage on the same context gives the plain 5 n + 2 terms again; a failed shared staging
 *             leaves nothing staged.
 * Measured (tools/shared_bench.py --kind=pedersen; kind 2 pool, 65 536 one-pair items over 3 inputs): resident
 * 134.7-138.6 M items/s against 108.6-112.6 for avrf_pool_submit in the same process (1.24 x, ranges apart); from page-locked host
 * buffers 94.2-95.6 against 82.6-91.9 (1.07 x, ranges apart by little).  USE THE PLAIN CALL WHEN NOTHING IS SHARED: with every input
 * its own row (T = n) the term count is the plain one; resident runs are level (112.2-120.8 against 110.4-111.6) and staging the
 * table from the host costs a tenth of the throughput (80.9-85.8 against 89.9-91.8 M items/s, 0.90 x). */
int avrf_pedersen_batch_stage_shared(avrf_ctx *ctx, size_t n, size_t n_shared, const uint8_t *shared_xy,
                                     const uint32_t *input_index, const uint8_t *outputs_xy, const uint32_t *io_counts,
                                     const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs);
size_t avrf_pedersen_shared_n_terms(size_t n, size_t n_shared);
/* The same batch from wire bytes.  With L = avrf_point_len(suite): shared is n_shared x L (`serialize_compressed` points), outputs
 * sum(io_counts) x L, proofs n x (3 L + 64) laid out Yb || R || Ok || s || sb (the Pedersen wire proof of
 * avrf_pedersen_batch_stage_wire); input_index, io_counts, ads and ad_lens exactly as in avrf_pedersen_batch_stage_shared.
 * avrf_pedersen_batch_verify_shared_wire is stage + avrf_pedersen_batch_run.
 *   indices   checked on the host before anything is staged: a failure is AVRF_ERR_BAD_ARG and the context keeps what it had
 *             staged.  avrf_pool_submit_pedersen_shared_wire checks on the submitting thread, before a ticket exists.
 *   decoding  one kernel launch per staging decodes EVERY table row -- referenced or not --, every output and the three points of
 *             every proof, each once: a row costs one square root however many items refer to it, and an item four square roots
 *             instead of five.  validate = 0: the point must decode (Validate::No).  validate != 0: it must also be non-identity
 *             and in the prime-order subgroup (Validate::Yes, src/lib.rs:410-433).  AS IN THE THIN CALL, THIS DIFFERS FROM THE
 *             x || y FLAVOUR: under validate != 0 an identity row is refused even when nothing refers to it.  With validate = 0 an
 *             identity row decodes; the run then refuses it only if it is referenced.  As in avrf_pedersen_batch_stage_wire,
 *             validate != 0 refuses an item without pairs, because its Ok is the identity.
 *   failure   a point that fails makes the stage call return AVRF_INVALID_DATA with nothing staged; in the pool the verdict is
 *             AVRF_INVALID_DATA, which avrf_pool_resubmit with from_host = 0 and the cycle mode repeat, while from_host = 1
 *             stages again from the seven host buffers.
 *   after     the staged batch is a shared-table batch in every respect: term layout and avrf_pedersen_shared_n_terms as above,
 *             every run entry point, the pool's wait / resubmit / cycle.  avrf_ctx_set_validation keeps acting on the staged
 *             x || y points at every run, independently of `validate`.
 * Measured (tools/shared_wire_bench.py --kind=pedersen, validate = 1, from page-locked host buffers, same pool and items):
 * 57.8-58.6 M items/s against 41.3-46.0 for avrf_pool_submit_wire (1.34 x, ranges apart): four points decoded per item instead of
 * five and 4/5 of the MSM terms.  The x || y flavour of the same batch runs 93.6-96.4. */
int avrf_pedersen_batch_stage_shared_wire(avrf_ctx *ctx, size_t n, size_t n_shared, const uint8_t *shared,
                                          const uint32_t *input_index, const uint8_t *outputs, const uint32_t *io_counts,
                                          const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate);
int avrf_pedersen_batch_verify_shared_wire(avrf_ctx *ctx, size_t n, size_t n_shared, const uint8_t *shared,
                                           const uint32_t *input_index, const uint8_t *outputs, const uint32_t *io_counts,
                                           const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate);
/* The layout of a segmented Pedersen run (src/pedersen.rs:303-426: 5 items + 2 terms per BatchVerifier whatever the pair counts, so
 * no io_counts), host arithmetic only: out as avrf_thin_segments_layout.  AVRF_ERR_BAD_ARG when the counts do not sum to n or a
 * limit is exceeded. */
int avrf_pedersen_segments_layout(size_t n, size_t n_seg, const uint32_t *seg_items, uint64_t out[4]);
/* The MSM terms the last avrf_pedersen_batch_run_segments built for segment `seg` (src/pedersen.rs:303-426; tests), as
 * avrf_thin_segment_terms. */
size_t avrf_pedersen_segment_terms(avrf_ctx *ctx, size_t seg, uint8_t *bases_xy, uint8_t *scalars);

/* ---- SEGMENTS of a batch staged over a table of shared points: one verdict per group of items, rows still merged.
 * The two segmented calls above refuse a shared-table staging, because a row's merged scalar mixes the items of every segment.  Summed
 * per (segment, row) pair instead of per row, the merged rows do have a per-segment meaning: segment v gets exactly the treatment the
 * reference gives G and BLINDING_BASE (src/thin.rs:303,316-317, src/pedersen.rs:387-418), restricted to its own items.  For the ticket
 * workload that arrives per block (one verdict per block over two or three shared inputs) and for locating the bad items of a failed
 * shared-table batch without staging it again in expanded form.
 *   stagings  avrf_thin_batch_run_shared_segments / avrf_pedersen_batch_run_shared_segments work on WHATEVER batch of their kind the
 *             context holds.  On a shared-table staging (x || y or wire) they do what is described here; on a plain staging --
 *             including a Pedersen "shared" staging with n_shared == 0, which is staged plain -- they ARE avrf_thin_batch_run_segments /
 *             avrf_pedersen_batch_run_segments.  A caller that always stages through the shared calls never switches entry points.
 *             The two calls above keep refusing a shared staging.  *_verify_shared_segments_wire are avrf_*_batch_stage_shared_wire +
 *             the run (a staging error, e.g. AVRF_INVALID_DATA for a row that does not decode, is returned as it is and no status is
 *             written).
 *   statuses  status_out[v] is what avrf_thin_batch_verify / avrf_pedersen_batch_verify answers for segment v's items alone, every
 *             index replaced by its row: AVRF_OK, AVRF_VERIFICATION_FAILURE or AVRF_INVALID_DATA; an empty segment is AVRF_OK.  A row
 *             that nothing in segment v refers to has NO influence on status_out[v], whatever bytes it holds.  THIS DIFFERS FROM
 *             avrf_thin_batch_run / avrf_pedersen_batch_run ON THE SAME x || y STAGING, which refuse a non-canonical coordinate in ANY
 *             row.  A segment is AVRF_INVALID_DATA, and no other segment is, when a row it references is the identity, has a
 *             non-canonical coordinate or fails avrf_ctx_set_validation 1 / 2, or when one of its items has a defect the plain
 *             segmented call attributes to it (an output or proof point, a scalar >= r).  The call returns AVRF_OK whenever the
 *             statuses were written.
 *   layouts   two, chosen by host arithmetic alone (avrf_*_shared_segments_layout says which).  items_v / p_v: segment v's items and
 *             I/O pairs, T = n_shared, maxima over the non-empty segments.
 *             MERGED, Thin (this layout is ABI): n_v = items_v + p_v + T + 1 terms at [v L, v L + n_v).  With `first` the segment's first
 *             item and io_off the prefix sums of io_counts: (R_j, w_j) at v L + (j - first) + (io_off[j] - io_off[first]), its
 *             (O_ji, w c z_i) directly behind it; row r at v L + items_v + p_v + r with the scalar  sum of w c z0 over the SEGMENT's
 *             items whose key is r  -  sum of w s z_i over the SEGMENT's pairs whose input is r  (mod r_order), 0 -- and the base still
 *             written -- for a row the segment does not reference; (G, g_v) last.  The weights are those of the segment's own
 *             transcript, the item index taken inside the segment, as in avrf_thin_batch_run_segments.
 *             MERGED, Pedersen (ABI): n_v = 4 items_v + T + 2.  Item j's (O_merged, t c), (Ok, t), (Yb, u c), (R, u) at
 *             v L + 4 (j - first) + k; row r at v L + 4 items_v + r with the scalar  - sum of t s z_i over the segment's pairs whose
 *             input is r; then (G, -sum u s), then (BLINDING_BASE, -sum u sb).
 *             EXPANDED: the plain segmented layout of avrf_thin_batch_run_segments / avrf_pedersen_batch_run_segments over the rows
 *             as staging gathered them.
 *             L_m = max(items_v + p_v) + T + 1 (Thin), 4 max(items_v) + T + 2 (Pedersen); L_p as for the plain segmented call.  The
 *             run takes the merged layout exactly when L_m < L_p (a tie goes to expanded), so it is never a worse MSM than the
 *             expanded batch and never refused where the expanded batch would be accepted.  The three limits above apply to the
 *             chosen L: the merged layout admits segments the plain one cannot (2 048 one-pair Thin items over 1 027 rows are
 *             5 124 terms; the plain layout's 8 193 is over the limit).
 *   refusals  as for the plain segmented calls, AVRF_ERR_BAD_ARG with the staging untouched and usable: counts that do not sum to n,
 *             nothing staged, a staging of the other kind, a busy context or a call between avrf_batch_run_begin and _end, a limit
 *             exceeded.
 *   after     avrf_*_batch_run on the same staging gives its usual verdict and avrf_batch_last_terms its usual shared-layout terms
 *             (avrf_*_batch_challenges must be repeated before avrf_*_batch_partial).  avrf_thin_segment_terms /
 *             avrf_pedersen_segment_terms describe the last segmented run of either entry point, in the layout that run chose.
 *             avrf_last_timing keeps the slots of the segmented calls; the per-run plan is part of [3].
 * avrf_*_shared_segments_layout: host arithmetic only, no device, the same refusals: out = { L, n_seg * L, sum of the n_v of the
 * non-empty segments, window bits, mode } with mode 1 = merged, 0 = expanded; n_shared == 0 describes a plain staging (mode 0).
 * Term counts (derived): Pedersen 256 x 256 one-pair items over T = 3: L 1 029 against 1 282 (0.80 of the padded MSM); 4 096 x 16: 69
 * against 82 (0.84); Thin 64 x 1 024 over 1 024 keys + 3 inputs: 3 076 against 4 097 (0.75); Thin 256 x 256 on the same table: expanded
 * is chosen (1.00).  (Pedersen 4 096 x 16 is over AVRF_SEGMENTS_WINDOWS_MAX in either layout.)
 * Measured (tools/segments_bench.py --legs=g; 65 536 one-pair items over 1 024 keys + 3 inputs, against
 * avrf_*_batch_run_segments on the expanded staging of the same items in the same process, M items/s): resident, Thin 64 x 1 024
 * 24.2-29.0 against 22.3-23.3, Pedersen 256 x 256 25.9-26.3 against 25.0-25.3, Pedersen 1 024 x 64 19.3-19.6 against 18.3-18.5; from
 * page-locked x || y buffers 22.7-24.3 / 19.7-20.0, 20.7-20.8 / 20.2-20.3, 16.1-16.2 / 15.5-15.6; from wire bytes with validate = 1
 * 20.6-21.7 / 15.2-16.3, 17.6-17.7 / 15.4-15.6, 14.4-14.5 / 12.6-12.7: ahead with the ranges apart wherever the merged layout is chosen.
 * THE TERM RATIOS DO NOT REACH THE WALL CLOCK (1.03-1.07 x for Pedersen resident where 1.19-1.25 x is derived: the chain's tail does not
 * shrink with L).  THIN 256 x 256, WHERE EXPANDED IS CHOSEN, IS LEVEL (26.2-27.5 against 26.6-27.7 resident, 22.2-22.8 against 21.9-22.6
 * from x || y); only its wire run gains (19.8-20.3 against 16.4-18.0: each row decoded once). */
int avrf_thin_batch_run_shared_segments(avrf_ctx *ctx, size_t n_seg, const uint32_t *seg_items, int32_t *status_out);
int avrf_pedersen_batch_run_shared_segments(avrf_ctx *ctx, size_t n_seg, const uint32_t *seg_items, int32_t *status_out);
int avrf_thin_batch_verify_shared_segments_wire(avrf_ctx *ctx, size_t n, size_t n_shared, const uint8_t *shared,
                                                const uint32_t *pk_index, const uint32_t *input_index, const uint8_t *outputs,
                                                const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens,
                                                const uint8_t *proofs, int validate, size_t n_seg, const uint32_t *seg_items,
                                                int32_t *status_out);
int avrf_pedersen_batch_verify_shared_segments_wire(avrf_ctx *ctx, size_t n, size_t n_shared, const uint8_t *shared,
                                                    const uint32_t *input_index, const uint8_t *outputs, const uint32_t *io_counts,
                                                    const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate,
                                                    size_t n_seg, const uint32_t *seg_items, int32_t *status_out);
int avrf_thin_shared_segments_layout(size_t n, size_t n_shared, size_t n_seg, const uint32_t *seg_items, const uint32_t *io_counts,
                                     uint64_t out[5]);
int avrf_pedersen_shared_segments_layout(size_t n, size_t n_shared, size_t n_seg, const uint32_t *seg_items, uint64_t out[5]);

/* ---- Ownership of host buffers; page-locked memory (SURVEY.md 8b "Ownership").
 * Every entry point copies what it needs out of the caller's buffers before it returns, EXCEPT avrf_pool_submit (below), whose
 * copies are left in flight.  From ordinary (pageable) memory a copy to the device goes through the runtime's bounce buffers
 * at ~10 GB/s of a host core; from page-locked memory it is a DMA transfer that costs no host time and overlaps kernels.
 * avrf_host_alloc returns page-locked memory for the batch buffers (pks / ios / ads / proofs / counts); avrf_host_register
 * pins memory the caller already owns (page-aligned ranges are cheapest; unregister before freeing it). */
int avrf_host_alloc(size_t bytes, void **out);
/* NUMA placement (a two-socket host with several GPUs): the pool's worker threads run on the CPUs of their
 * device's NUMA node, and avrf_host_alloc allocates its pages from the node of the CURRENT device (hipGetDevice) -- both inside
 * the caller's affinity mask, both read from sysfs (/sys/bus/pci/devices/<bdf>/numa_node), both off with AVRF_POOL_NUMA=0.
 * avrf_numa_cpus_of_pci is the lookup itself (node_out: -1 = unknown; returns the CPUs written to cpus_out);
 * avrf_pool_numa_node the node a pool's workers were bound to (-1: not bound). */
int avrf_numa_cpus_of_pci(const char *pci_bdf, const char *sysfs_root_dir, int32_t *cpus_out, size_t cap, int32_t *node_out);
void avrf_host_free(void *p);
int avrf_host_register(void *p, size_t bytes);
int avrf_host_unregister(void *p);

/* ---- avrf_pool: many BatchVerifier::verify jobs in flight on one device (thin::BatchVerifier src/thin.rs:188-326 when
 * kind = 1, pedersen::BatchVerifier src/pedersen.rs:303-426 when kind = 2) -- the form a service that verifies batch after
 * batch wants, and the one bench.py measures.  The reference's verify() is one call on one thread; here a batch is device
 * work, 3.5 ms of a host core for the sequential weight transcript (src/thin.rs:274-279), then 0.6 ms of device work, so
 * throughput comes from overlapping many batches, and host time per batch is what bounds a node with several GPUs.
 *   n_slots    batches that can be staged at once (inputs + transcript records, ~30 MB each at 65 536 items);
 *   n_lanes    streams + MSM workspaces (~150 MB each) the MSM chains run on; waiting batches hold no lane;
 *   lane_depth chains queued behind each other on one lane (0 = 3): a host thread that has just hashed a group of transcripts
 *              enqueues ALL their chains at once and goes back to hashing while the device works through them (few streams,
 *              deep queues: more than ~20 streams in flight slow the device down);
 *   n_threads  native host threads; each owns a share of the slots and lanes and is driven by completion events;
 *   hash_group transcripts a thread hashes TOGETHER: 1 = one scalar SHA-512 chain at a time (lowest latency; right when the
 *              process has >= ~4 cores per GPU), 8 / 16 = the AVX-512 multi-buffer code (3.5-5 x the hashes per core-second at
 *              the price of latency; right for 1-3 cores per GPU; falls back to 1 without AVX-512).
 * avrf_pool_submit hands over one batch (arguments as avrf_thin_batch_stage; pks_xy NULL for kind 2) and returns a ticket
 * at once; THE BUFFERS MUST STAY UNTOUCHED UNTIL avrf_pool_wait HAS RETURNED FOR THAT TICKET (the copies are asynchronous).
 * It blocks while every slot is in flight and returns AVRF_ERR_BAD_ARG when every slot holds an uncollected verdict.
 * avrf_pool_wait blocks until the verdict of `ticket` is out: *status = AVRF_OK / AVRF_VERIFICATION_FAILURE /
 * AVRF_INVALID_DATA exactly as avrf_thin_batch_verify would return for that batch.  avrf_pool_resubmit runs the batch of a
 * collected ticket again (from_host = 0: the copy resident in HBM; 1: staged again from the same host buffers).
 * avrf_pool_cycle is the measurement loop: every slot that holds a collected batch is run again and again by the workers
 * themselves until the region consists of whole blocks of `steps_block` runs and has lasted `min_seconds` (0: one block;
 * max_steps bounds it), no foreign-function call per step; returns the runs made, how many returned something else than
 * `expect_status`, and the time from the first launch to the last verdict.
 * avrf_pool_stats: out[0..4] host-thread CPU microseconds spent in staging + prepare launches / collecting / hashing /
 * terms + MSM launches / folding, out[6] hash groups, out[7] transcripts hashed, out[8] times a thread slept, out[9] / out[10]
 * total milliseconds / launches of the dominant kernel (k_accumulate, HIP events on the lanes' streams); n_out >= 11. */
typedef struct avrf_pool avrf_pool;
int avrf_pool_create(int suite, int device, int kind, int n_slots, int n_lanes, int lane_depth, int n_threads, int hash_group, avrf_pool **out);
void avrf_pool_destroy(avrf_pool *pool);
int avrf_pool_set_validation(avrf_pool *pool, int level);
int avrf_pool_submit(avrf_pool *pool, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                     const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, uint64_t *ticket);
/* avrf_pool_submit_wire: the same job from wire bytes (`serialize_compressed` points; thin proofs R || s, pedersen proofs
 * Yb || R || Ok || s || sb as CanonicalSerialize writes them): decompression, and with validate != 0 the non-identity and
 * prime-order-subgroup checks of Validate::Yes (src/lib.rs:410-433), run on the device while the batch is staged; a point that
 * fails makes the verdict AVRF_INVALID_DATA.  Resubmission and the cycle mode work on such slots as on any other. */
int avrf_pool_submit_wire(avrf_pool *pool, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts,
                          const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate, uint64_t *ticket);
/* avrf_pool_submit_shared (kind 1 pools): the same job over a table of shared points, arguments and contract as
 * avrf_thin_batch_stage_shared above.  All eight host buffers must stay untouched until the verdict is out: shared_xy, pk_index,
 * input_index, outputs_xy, ads and proofs are copied asynchronously, io_counts and ad_lens are read when the batch is staged --
 * and all eight again by every avrf_pool_resubmit with from_host = 1.  The indices, and a missing outputs_xy or input_index where
 * there are I/O pairs, are refused here, before a ticket exists.  Resubmission and the cycle mode work on such slots as on any
 * other: without host sources they reuse the gathered rows and the plan. */
int avrf_pool_submit_shared(avrf_pool *pool, size_t n, size_t n_shared, const uint8_t *shared_xy, const uint32_t *pk_index,
                            const uint32_t *input_index, const uint8_t *outputs_xy, const uint32_t *io_counts,
                            const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, uint64_t *ticket);
/* avrf_pool_submit_shared_wire (kind 1 pools): the same job from wire bytes, arguments and contract as
 * avrf_thin_batch_stage_shared_wire above; ownership as avrf_pool_submit_shared: all eight host buffers stay untouched until the
 * verdict is out, and are read again by every avrf_pool_resubmit with from_host = 1. */
int avrf_pool_submit_shared_wire(avrf_pool *pool, size_t n, size_t n_shared, const uint8_t *shared, const uint32_t *pk_index,
                                 const uint32_t *input_index, const uint8_t *outputs, const uint32_t *io_counts,
                                 const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate,
                                 uint64_t *ticket);
/* avrf_pool_submit_pedersen_shared / _shared_wire (kind 2 pools; a kind 1 pool refuses them, as avrf_pool_submit_shared / _shared_wire
 * refuse a kind 2 pool): the Pedersen jobs over a table of shared inputs, arguments and contract as avrf_pedersen_batch_stage_shared /
 * _shared_wire above.  All seven host buffers must stay untouched until the verdict is out, and are read again by every
 * avrf_pool_resubmit with from_host = 1.  The indices, and a missing outputs or input_index where there are I/O pairs, are refused
 * here, before a ticket exists.  Resubmission and the cycle mode reuse the gathered rows and the plan. */
int avrf_pool_submit_pedersen_shared(avrf_pool *pool, size_t n, size_t n_shared, const uint8_t *shared_xy,
                                     const uint32_t *input_index, const uint8_t *outputs_xy, const uint32_t *io_counts,
                                     const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, uint64_t *ticket);
int avrf_pool_submit_pedersen_shared_wire(avrf_pool *pool, size_t n, size_t n_shared, const uint8_t *shared,
                                          const uint32_t *input_index, const uint8_t *outputs, const uint32_t *io_counts,
                                          const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate,
                                          uint64_t *ticket);
/* avrf_pool_submit_segments / _segments_wire: a SEGMENTED job -- n_seg independent BatchVerifiers over consecutive runs of the batch's
 * items, one verdict each (thin::BatchVerifier src/thin.rs:188-326 on a kind 1 pool, pedersen::BatchVerifier src/pedersen.rs:303-426 on
 * a kind 2 pool with pks NULL; every suite the pool accepts).  What avrf_thin_batch_run_segments / avrf_pedersen_batch_run_segments do
 * on one context, with other jobs in flight beside it: one prepare pass, the n_seg weight transcripts (src/thin.rs:274-279,
 * src/pedersen.rs:361-367, each over ITS items only) hashed through the pool's grouped hash -- a job with many segments fills groups
 * by itself, segments of different jobs share a group -- one terms pass and ONE MSM chain on a lane, whatever n_seg is.  Plain and
 * segmented jobs may be in flight in one pool at once.
 *   contract   arguments as avrf_pool_submit / avrf_pool_submit_wire, then the segments as avrf_thin_batch_run_segments takes them:
 *              segment v covers the next seg_items[v] items, the counts sum to n.
 *   ownership  seg_items is copied before the call returns; the other buffers follow avrf_pool_submit's rule (untouched until the
 *              verdict is out, read again by avrf_pool_resubmit with from_host = 1).
 *   refusals   AVRF_ERR_BAD_ARG on the submitting thread, before a ticket exists, by the layout check of the context's call
 *              (avrf_thin_segments_layout / avrf_pedersen_segments_layout): counts that do not sum to n, a segment over
 *              AVRF_SEGMENT_TERMS_MAX, a layout over AVRF_SEGMENTS_PADDED_TERMS_MAX or AVRF_SEGMENTS_WINDOWS_MAX (the windows limit
 *              holds for every n_seg here: the job is one chain, there is no looped route below eight segments).  There is no
 *              shared-table flavour, as the context's call refuses a shared staging.
 *   statuses   avrf_pool_wait_segments: status_out[v] (cap >= n_seg entries) is exactly what avrf_thin_batch_run_segments /
 *              avrf_pedersen_batch_run_segments answers for segment v -- an empty segment AVRF_OK, a bad item marks its own segment
 *              only -- and *status the largest of them (AVRF_OK when all are).  avrf_pool_wait on a segmented ticket returns that
 *              same fold, and avrf_pool_cycle compares expect_status with it.  A staging error -- a wire point that does not decode
 *              or, under validate, fails -- is the job's *status with status_out left unwritten, as
 *              avrf_thin_batch_verify_segments_wire returns it; runs from the resident state repeat it.  avrf_pool_wait_segments on
 *              a plain ticket, or with cap < n_seg, is AVRF_ERR_BAD_ARG and the ticket is not consumed.
 *   reruns     avrf_pool_resubmit (both from_host values) and the cycle mode run the same segmentation again.
 *   memory     the padded term arrays (n_seg * L terms of 128 bytes), the per-item scratch, the seeds and the offsets are the
 *              LANE's, as a plain job's terms are: a slot does not grow with the segmentation.
 * avrf_pool_stats: out[7] counts every segment's transcript.
 * Runtime (tools/segments_bench.py legs e and f; 65 536 one-pair Thin items as 256 segments of 256 per job, 24 jobs
 * in flight on 144 slots / 12 lanes / 6 threads): 38.6-43.6 M items/s from the resident state, 39.5-41.0 M staged from page-locked
 * buffers on every run (Pedersen 37.8-41.7 / 32.6-35.8).  That beats one context's segmented call (26.8-28.2) and the per-item
 * avrf_thin_verify (27.3-28.1), ranges apart.  IT DOES NOT BEAT what a caller could already do with k contexts on k host threads,
 * each calling avrf_thin_batch_verify_segments: 45.2-46.2 M items/s with four, 48.6-48.9 with eight (resident: 42.5-43.7 / 42.6-44.8,
 * overlapping the pool's range).  The pool form is a convenience -- one object, tickets, plain and segmented jobs side by side, no host
 * thread per context -- and a memory saving (lanes, not contexts, hold the workspaces), not a speed-up.  Jobs want MANY segments: sixteen
 * segments of 256 items per job run at 8.3-9.3 M items/s with 144 jobs in flight (0.45 ms per job: the chain's lone-wave kernels, a
 * few chains at a time). */
int avrf_pool_submit_segments(avrf_pool *pool, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                              const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, size_t n_seg,
                              const uint32_t *seg_items, uint64_t *ticket);
int avrf_pool_submit_segments_wire(avrf_pool *pool, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts,
                                   const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int validate, size_t n_seg,
                                   const uint32_t *seg_items, uint64_t *ticket);
int avrf_pool_wait_segments(avrf_pool *pool, uint64_t ticket, int *status, int32_t *status_out, size_t cap);
int avrf_pool_wait(avrf_pool *pool, uint64_t ticket, int *status);
int avrf_pool_resubmit(avrf_pool *pool, uint64_t ticket, int from_host, uint64_t *new_ticket);
int avrf_pool_cycle(avrf_pool *pool, int from_host, uint64_t steps_block, double min_seconds, uint64_t max_steps, int expect_status,
                    uint64_t *steps_done, uint64_t *mismatches, double *seconds);
int avrf_pool_stats(avrf_pool *pool, int reset, double *out, size_t n_out);
int avrf_pool_numa_node(avrf_pool *pool);

/* pedersen::BatchVerifier split the same way (src/pedersen.rs:341-426): stage the shard with avrf_pedersen_batch_stage,
 * avrf_pedersen_batch_challenges -> n_shard x 16 bytes, avrf_batch_weight_seed(pedersen = 1) over all items
 * (resp = s || sb, 64 bytes per item), avrf_pedersen_batch_partial(seed, first_index) -> the shard's partial point. */
int avrf_pedersen_batch_challenges(avrf_ctx *ctx, uint8_t *c_out);
int avrf_pedersen_batch_partial(avrf_ctx *ctx, const uint8_t seed64[64], uint64_t first_index, uint8_t out_xy[64]);

/* One BatchVerifier split over several GPUs; see ark_vrf_amd/dist.py.
 * The weights of src/thin.rs:274-289 depend on ALL items, so: every rank stages its shard and calls
 * avrf_thin_batch_challenges (per-item c_j, 16 bytes each); the c_j and response scalars are
 * all-gathered; avrf_batch_weight_seed hashes them (host, sequential) into the 64-byte stream seed;
 * avrf_thin_batch_partial returns the MSM of the shard's terms (incl. its share of the G term) under
 * that seed; the partial points are all-gathered and added with avrf_points_sum; the batch verifies
 * iff the sum is the identity (0, 1). */
int avrf_thin_batch_challenges(avrf_ctx *ctx, uint8_t *c_out);
int avrf_batch_weight_seed(int suite, int pedersen, size_t n, const uint8_t *c16, const uint8_t *resp, uint8_t seed_out[64]);
/* The same for `count` <= 8 batches in one pass: the chains of different batches are independent, so their transcripts are
 * hashed together, one batch per lane of an AVX-512 register (host_sha512_mb.h: 3.6 x the hashes per core-second at twice
 * the latency of one scalar chain).  Inside avrf_*_batch_run the same code runs behind AVRF_HASH_THREADS service threads
 * (default 0; for hosts that grant a GPU fewer cores than its contexts have transcripts to hash -- bench.py turns it on
 * from the CPU quota).  seeds_out: count x 64 bytes.  AVRF_ERR_NO_DEVICE when the host CPU lacks AVX-512. */
int avrf_batch_weight_seeds_x8(int suite, int pedersen, int count, const size_t *n, const uint8_t *const *c16, const uint8_t *const *resp, uint8_t *seeds_out);
/* SHA-512 of `count` <= 8 contiguous messages through that multi-buffer code (the form avrf_*_batch_run hands to the service:
 * prefix || records in one buffer); digests_out: count x 64 bytes. */
int avrf_sha512_x8(int count, const uint8_t *const *msgs, const size_t *lens, uint8_t *digests_out);
/* the same for `count` <= 16 messages through the pool's form (two interleaved groups of eight above eight messages) */
int avrf_sha512_x16(int count, const uint8_t *const *msgs, const size_t *lens, uint8_t *digests_out);
/* (AVRF_ERR_BAD_ARG unless avrf_thin_batch_challenges succeeded on the CURRENT staging: re-staging or any other call that
 * stages -- avrf_thin_verify, a prover -- invalidates the challenges) */
int avrf_thin_batch_partial(avrf_ctx *ctx, const uint8_t seed[64], uint64_t first_index, uint8_t out_xy[64]);
int avrf_points_sum(int suite, size_t k, const uint8_t *points_xy, uint8_t out_xy[64]);

/* Exposes the MSM the last avrf_thin_batch_run / avrf_pedersen_batch_run built
 * (bases_xy: n_terms x 64, scalars: n_terms x 32) so tests can compare weights and terms with
 * the oracle bit for bit.  Either output pointer may be NULL; returns the number of terms. */
size_t avrf_batch_last_terms(avrf_ctx *ctx, uint8_t *bases_xy, uint8_t *scalars);

/* Last-call timing breakdown in microseconds (host wall clock):
 * [0] total, [1] device prepare (hash), [2] host weight transcript, [3] scalars, [4] msm, [5] finish.
 * Time spent inside the calls: with avrf_batch_run_begin / _hash / _end the gaps between the three calls are not counted. */
void avrf_last_timing(avrf_ctx *ctx, double out[8]);

/* Device-side timing of the dominant kernel (MSM bucket accumulation), measured with HIP events
 * recorded on the context's stream around every launch since the last reset: total milliseconds,
 * number of launches, and the plan of the last MSM {window bits c, windows, buckets/window, entries/lane}. */
int avrf_kernel_stats(avrf_ctx *ctx, int reset, double *accum_ms_total, uint64_t *accum_launches, int32_t plan[4]);

/* ---- Independent items (the per-item Prover / Verifier traits).  Two device forms behind every entry point below, same
 * results: calls of up to 2 048 items with ONE I/O pair each (and a given public key, for the provers) on the twisted-Edwards
 * suites spread an item over 32 lanes -- latency of a call 0.5-1.1 ms whatever n (Thin 0.54 / 0.72 ms, Pedersen 0.52 / 1.03 ms);
 * ONE item per call goes through the MSM engine instead (its equations / its commitments as small MSMs in one launch,
 * the doubling chains folded on the host): Thin 0.28 ms verifying, 0.36 ms proving; Pedersen 0.35 / 0.69 ms; up to 30 pairs; everything else runs one lane per item (2-3.4 ms per call up to 65 536 items: 19-25 M items/s). */

/* thin::Prover::prove for a batch of independent (sk, ios, ad)  (src/thin.rs:111-129).
 * sks: n x 32; pks_xy: the cached `Secret::public` (n x 64) or NULL to derive sk*G on the device;
 * ios as above; proofs_out: n x 96 (R_xy || s). */
int avrf_thin_prove(avrf_ctx *ctx, size_t n, const uint8_t *sks, const uint8_t *pks_xy, const uint8_t *ios_xy,
                    const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, uint8_t *proofs_out);

/* thin::Verifier::verify for a batch of independent items (src/thin.rs:131-165);
 * status_out[j] receives the per-item status.  Returns AVRF_OK when the call itself ran. */
int avrf_thin_verify(avrf_ctx *ctx, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                     const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int32_t *status_out);

/* tiny::Prover::prove / tiny::Verifier::verify (src/tiny.rs:163-214) for batches of independent items: the Thin construction
 * under scheme tag 0x00 with the challenge kept in the proof, proof = LE16(c) || LE32(s) = 48 bytes (Proof's compressed
 * serialisation, src/tiny.rs:60-78).  No batch verifier exists for this scheme (src/tiny.rs:1-6).  Arguments as for
 * avrf_thin_prove / avrf_thin_verify; proofs(_out): n x 48. */
int avrf_tiny_prove(avrf_ctx *ctx, size_t n, const uint8_t *sks, const uint8_t *pks_xy, const uint8_t *ios_xy,
                    const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, uint8_t *proofs_out);
int avrf_tiny_verify(avrf_ctx *ctx, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                     const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int32_t *status_out);

/* pedersen::BatchVerifier::{new, push*, verify} (src/pedersen.rs:303-426).
 * proofs: Yb_xy(64) || R_xy(64) || Ok_xy(64) || s(32) || sb(32) = 256 bytes per item. */
int avrf_pedersen_batch_verify(avrf_ctx *ctx, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts,
                               const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs);
int avrf_pedersen_batch_stage(avrf_ctx *ctx, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts,
                              const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs);
int avrf_pedersen_batch_run(avrf_ctx *ctx);

/* pedersen::Prover::prove (src/pedersen.rs:136-186) for a batch; pks_xy as for avrf_thin_prove;
 * proofs_out: n x 256, blindings_out: n x 32 (may be NULL). */
int avrf_pedersen_prove(avrf_ctx *ctx, size_t n, const uint8_t *sks, const uint8_t *pks_xy, const uint8_t *ios_xy,
                        const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, uint8_t *proofs_out,
                        uint8_t *blindings_out);

/* pedersen::Verifier::verify (src/pedersen.rs:188-249) for a batch of independent items. */
int avrf_pedersen_verify(avrf_ctx *ctx, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts,
                         const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs, int32_t *status_out);

/* ---- Ring VRF (src/ring.rs).  Handles own device-resident state; free them with *_free. ----
 *
 * RingSetup::from_pcs_params (src/ring.rs:380-393) on an arkworks `URS` file (`serialize_uncompressed`,
 * e.g. data/srs/bls12-381-srs-2-11-uncompressed-zcash.bin): parses and uploads the first 3N+1 G1 powers,
 * keeps the two G2 powers, builds the PIOP domain for `ring_size` (src/ring.rs:810-843).
 * Returns AVRF_RING_CAPACITY_EXCEEDED when the SRS is too short for the ring size. */
typedef struct avrf_ring_setup avrf_ring_setup;
typedef struct avrf_ring_key avrf_ring_key;
int avrf_ring_setup_load(avrf_ctx *ctx, const uint8_t *srs, size_t srs_len, size_t ring_size, avrf_ring_setup **out);
void avrf_ring_setup_free(avrf_ring_setup *setup);
/* Kzg::setup as reached from RingSetup::from_rand / from_seed (src/ring.rs:359-374), with the trapdoor tau (32 B LE,
 * < r) and the generators given explicitly (g1: one `powers_in_g1` entry, g2: one `powers_in_g2` entry, both in the
 * URS serialize_uncompressed encoding, e.g. the first entries of an existing SRS file).  Writes the URS bytes
 * { tau^i g1, i < n_g1 ; g2, tau g2 } that avrf_ring_setup_load reads; *out_len = bytes needed (also when out is too
 * small -> AVRF_ERR_BAD_ARG).  n_g1 = avrf_ring_pcs_domain_size(suite, ring_size) for a ring of that size.
 * Insecure by construction (the caller knows tau) -- exactly like the reference's from_seed; for tests and benches. */
int avrf_ring_srs_generate(avrf_ctx *ctx, const uint8_t *tau, const uint8_t *g1, const uint8_t *g2, size_t n_g1,
                           uint8_t *out, size_t out_cap, size_t *out_len);
/* RingSetup::from_seed(ring_size, seed) (src/ring.rs:359-366): the deterministic setup of a 32-byte seed as the reference derives it --
 * Transcript::new(SUITE_ID), absorb_raw(seed), to_rng() (src/utils/transcript.rs:61-92), then Kzg::setup = URS::generate: tau = Fr::rand,
 * g1 = G1::rand, g2 = G2::rand from that stream -- so that two parties sharing only the seed hold the same SRS (README.md:181 of the
 * reference).  PARITY UNPINNED: the reference holds no vector of a seeded setup; the samplers (ark-ff Fp::rand, ark-ec
 * Projective::rand, rand 0.8 bool, w3f-pcs draw order) are restated from their published code, here and in oracle/ring_py.py
 * srs_from_seed, and the two restatements are tested against each other.  Insecure by construction (the seed gives tau), like the
 * reference's. */
int avrf_ring_setup_from_seed(avrf_ctx *ctx, const uint8_t *seed, size_t ring_size, avrf_ring_setup **out);
/* (avrf_ring_setup_load also accepts the serialize_compressed form of the same object: G1 / G2 points are decompressed on
 * the host, curve membership checked, no G2 subgroup check -- the SRS is trusted-setup material, src/ring.rs:466-474.)
 * CanonicalSerialize for RingSetup (= its PcsParams, truncated to the 3N+1 powers the setup keeps; src/ring.rs:484-521) and
 * for RingBuilderPcsParams (Vec<G1Affine>: the SRS in Lagrangian form L_i(tau) g1, i < N; src/ring.rs:523-529, obtained in the
 * reference from RingSetup::verifier_key_builder), compress = 0 / 1 for ark-serialize's two modes.  *out_len = bytes needed
 * (also when `out` is NULL or too small -> AVRF_ERR_BAD_ARG). */
int avrf_ring_setup_serialize(avrf_ring_setup *setup, int compress, uint8_t *out, size_t out_cap, size_t *out_len);
/* Verifier-only setup (src/ring.rs:466-482, verifier_key_from_commitment: "verifier-only users: no SRS required"):
 * avrf_ring_pcs_verifier_params_serialize writes RingSetup::pcs_verifier_params() (src/ring.rs:435) =
 * RawKzgVerifierKey { g1, g2, tau_in_g2 } in either ark-serialize mode; avrf_ring_verifier_setup_load builds from those bytes
 * (points validated) a setup handle that serves avrf_ring_batch_verify / avrf_ring_verify_each / avrf_ring_vrf_verify /
 * avrf_ring_pairing_check and nothing that needs the SRS (index, prove, builder, setup serialisation ->
 * AVRF_SRS_LOOKUP_FAILED). */
int avrf_ring_pcs_verifier_params_serialize(avrf_ring_setup *setup, int compress, uint8_t *out, size_t out_cap, size_t *out_len);
int avrf_ring_verifier_setup_load(avrf_ctx *ctx, const uint8_t *params, size_t params_len, size_t ring_size, avrf_ring_setup **out);
int avrf_ring_builder_params_serialize(avrf_ring_setup *setup, int compress, uint8_t *out, size_t out_cap, size_t *out_len);
size_t avrf_ring_pcs_domain_size(int suite, size_t ring_size);   /* pcs_domain_size, src/ring.rs:810-817 */
size_t avrf_ring_max_ring_size(const avrf_ring_setup *setup);   /* RingContext::max_ring_size, src/ring.rs:298-300 */
size_t avrf_ring_domain_size(const avrf_ring_setup *setup);     /* piop_domain_size, src/ring.rs:819-821 */
size_t avrf_ring_proof_len(const avrf_ring_setup *setup);       /* 592 (BLS12-381) / 480 (BN254) */
size_t avrf_ring_commitment_len(const avrf_ring_setup *setup);  /* 144 / 96 */
/* the suite a setup was loaded for (-1: NULL) and the setup a prover key was indexed on (owned by the caller as before) */
int avrf_ring_setup_suite(const avrf_ring_setup *setup);
avrf_ring_setup *avrf_ring_key_setup(const avrf_ring_key *key);
/* how the prover's KZG commitments are laid out as fixed-base MSMs (for op counts in reports): out = { window bits and rows of
 * the SRS window table, window bits and rows of the Lagrange-basis witness table (0 until the first proof builds it) }.  A prove call of
 * 64 or more proofs builds, once per device and SRS, the tables of ALL multiples of both base sets in the HBM that is free (DESIGN.md;
 * AVRF_RING_TABLE_GB, default 232, AVRF_RING_DIRECT=0 to keep the bucket form); from then on the figures are those tables'. */
int avrf_ring_setup_plan(const avrf_ring_setup *setup, int32_t out[4]);
/* ---- Tables of all multiples: per-setup HBM budget, explicit build and release.
 * Without these calls nothing changes: the first prove call of 64 or more proofs builds (or adopts from the per-device registry)
 * both tables within the process default (AVRF_RING_TABLE_GB, AVRF_RING_DIRECT, adapted to the HBM that is free at that moment).
 * Resource contract: a build takes the table's bytes (avrf_ring_table_bytes) plus transient scratch that is freed before the call
 * returns, 386 x rows x bases x 4 x (32-bit words of an Fq element: 12, 8) bytes -- 2.05 GB for the SRS table of a BLS12-381 ring of 1024 at c = 15 (18 rows),
 * 6.07 GB for that of a BN254 ring of 4096 at c = 13 (20 rows) -- and blocks the calling thread while it builds.
 * A table is shared by every setup over the same SRS on a device that plans the same width; the registry frees it with its last holder.
 *
 * Bytes of the table of all multiples for a ring of `ring_size` on a ring suite: kind 0 = the 3N+1 SRS powers, kind 1 = the 2N+1
 * witness bases; 0 when c is outside 8..16, the suite has no ring, or the table would hold 2^31 - 1 points or more (entry indices
 * are 31-bit).  Host arithmetic only: no device needed. */
uint64_t avrf_ring_table_bytes(int suite, size_t ring_size, int kind, int c);
/* HBM this setup's two tables may take together.  UINT64_MAX (the initial value) = the process default (the rule above); 0 = bucket
 * form only.  With an explicit budget the plan is a pure function of it: the SRS table gets the widest c in [the bucket width
 * (avrf_ring_setup_plan out[0] before any table), 16] whose bytes fit, the witness table the widest c in [8, 16] that fits what is
 * left.  Free memory does not change the widths: a planned table that does not fit in free HBM - 40 GB, or whose allocation or build
 * fails, is not built (state bit 8) and the bucket form runs for it; no narrower table is substituted.  A registry table is adopted
 * only at exactly the planned width.  Takes effect at the next build; tables already held stay until released. */
int avrf_ring_setup_set_table_budget(avrf_ring_setup *setup, uint64_t bytes);
/* Build (or adopt from the per-device registry) the tables the plan calls for, now -- e.g. inside a service's prover_key path.
 * Again with the same plan: a no-op (tables not built before are tried again); after a budget change: releases, then rebuilds.
 * AVRF_ERR_NO_DEVICE when a planned table could not be held (state bit 8); the setup stays fully usable on the bucket form. */
int avrf_ring_setup_build_tables(avrf_ring_setup *setup);
/* Drop this setup's (and its second lane's) references; the registry frees a table when its last holder goes.  A released setup
 * proves on the bucket form and does not build lazily again until avrf_ring_setup_build_tables is called. */
int avrf_ring_setup_release_tables(avrf_ring_setup *setup);
/* out = { state bits, budget in force (bytes), SRS table c, rows, bytes, witness table c, rows, bytes (0 when not held),
 *         commitment batches served from tables so far, bytes of all tables this process holds on the setup's device }.
 * State bits: 1 SRS table held, 2 witness table held, 4 an explicit budget is set, 8 a planned table was not built (bucket form
 * for it), 16 tables disabled (budget 0, or AVRF_RING_DIRECT=0 with no explicit budget).  The budget in force without an explicit
 * one is AVRF_RING_TABLE_GB x 10^9 (0 when disabled); free memory further limits it at a build.
 * All four setup calls: AVRF_SRS_LOOKUP_FAILED on a verifier-only setup, AVRF_ERR_BAD_ARG on a busy context. */
int avrf_ring_setup_tables(const avrf_ring_setup *setup, uint64_t out[10]);

/* RingSetup::prover_key / verifier_key -> ring_proof::index (src/ring.rs:399-417): fixed columns of the
 * ring `pks_xy` (n_keys x 64) and their three KZG commitments.  commitment_out (may be NULL) receives the
 * RingCommitment in its compressed serialisation (3 x G1), i.e. the `ring_pks_com` of the reference vectors.
 * AVRF_RING_CAPACITY_EXCEEDED if n_keys > max ring size. */
int avrf_ring_index(avrf_ring_setup *setup, const uint8_t *pks_xy, size_t n_keys, avrf_ring_key **out, uint8_t *commitment_out);
void avrf_ring_key_free(avrf_ring_key *key);

/* VerifierKeyBuilder (src/ring.rs:539-637): incremental construction of a ring commitment.  `new` = the ring of padding
 * points (VerifierKeyBuilder::new; the Lagrange-basis SRS the reference passes as RingBuilderPcsParams / SrsLookup is
 * derived from the setup's SRS on the device), `append` adds keys in order (AVRF_RING_CAPACITY_EXCEEDED and nothing
 * appended when they do not fit, AVRF_INVALID_DATA for a non-canonical coordinate), `finalize` writes the compressed
 * RingCommitment -- equal to avrf_ring_index's for the same key list. */
typedef struct avrf_ring_vk_builder avrf_ring_vk_builder;
int avrf_ring_vk_builder_new(avrf_ring_setup *setup, avrf_ring_vk_builder **out);
void avrf_ring_vk_builder_free(avrf_ring_vk_builder *builder);
size_t avrf_ring_vk_builder_free_slots(const avrf_ring_vk_builder *builder);          /* src/ring.rs:584-586 */
int avrf_ring_vk_builder_append(avrf_ring_vk_builder *builder, const uint8_t *pks_xy, size_t n);   /* :598-622 */
int avrf_ring_vk_builder_finalize(const avrf_ring_vk_builder *builder, uint8_t *commitment_out);   /* :625-627 */

/* RingProver::prove (the `ring_prover.prove(blinding)` half of ring::Prover::prove, src/ring.rs:219-221) for n
 * proofs over one ring: key_index[i] is the prover's position in the ring, blindings[i] the secret blinding
 * returned by avrf_pedersen_prove.  blinding_mode 0 = RingContext::new_without_blinding (deterministic,
 * reproduces the reference vectors); 1 = hiding (the reference's default RingContext): the last 3 rows of every
 * witness column are fresh uniformly random field elements (getrandom(2)), so proofs are not reproducible.  proofs_out: n x avrf_ring_proof_len bytes (the RingBareProof in its
 * compressed serialisation); the full ring-VRF proof is the Pedersen proof followed by it (src/ring.rs:160-166). */
int avrf_ring_prove(avrf_ring_key *key, size_t n, const uint32_t *key_index, const uint8_t *blindings, int blinding_mode,
                    uint8_t *proofs_out);

/* RingVerifier::verify (n = 1) and the multi-ring RingBatchVerifier::{push, verify} (src/ring.rs:242,682-735):
 * verifies n bare ring proofs (compressed serialisation, avrf_ring_proof_len bytes each) for the key
 * commitments instances_xy (n x 64: the Pedersen proof's Yb, src/ring.rs:237-241) against ring commitments
 * (n_rings x avrf_ring_commitment_len, cf. verifier_key_from_commitment src/ring.rs:477-482); ring_of_item[i]
 * selects the ring of item i (NULL = all items use ring 0).  One randomised check: two G1 MSMs on the GPU and
 * a 2-pairing check.  A complete ring-VRF (batch) verification is avrf_pedersen_(batch_)verify on the Pedersen
 * halves plus this call (src/ring.rs:236-242,729-735).  Returns AVRF_OK / AVRF_VERIFICATION_FAILURE /
 * AVRF_INVALID_DATA (undecodable point or scalar). */
int avrf_ring_batch_verify(avrf_ring_setup *setup, size_t n, const uint8_t *ring_commitments, size_t n_rings,
                           const uint32_t *ring_of_item, const uint8_t *instances_xy, const uint8_t *ring_proofs);

/* n x ring::Verifier::verify (src/ring.rs:228-247, the ring half): the same inputs as avrf_ring_batch_verify, but every proof is
 * checked on its own and gets its own status (status_out[i] = AVRF_OK / AVRF_VERIFICATION_FAILURE / AVRF_INVALID_DATA), so a
 * bad proof is identified instead of failing the batch: per proof two small G1 linear combinations and one 2-pairing check,
 * all on the device (Miller loops + final exponentiations of all proofs in one kernel, pairing.hip).  Few proofs are latency
 * cases -- one wave of the pairing kernel needs 11.7 ms whatever it carries -- so up to 16 checks are finished on the host pool
 * from the device's G1 sums (tabulated G2 lines, 1.0 ms per check and core), and n = 1 runs as a batch of one (1.7 ms; the
 * reference: 3.24 ms).  Same statuses either way.  A ring commitment that does not decode fails the call (AVRF_INVALID_DATA). */
int avrf_ring_verify_each(avrf_ring_setup *setup, size_t n, const uint8_t *ring_commitments, size_t n_rings, const uint32_t *ring_of_item,
                          const uint8_t *instances_xy, const uint8_t *ring_proofs, int32_t *status_out);

/* ---- ring BatchVerifier over SEGMENTS: one verdict per group of proofs (src/ring.rs:682-735, one BatchVerifier per segment).
 * n_seg independent ring BatchVerifiers over consecutive runs of the n items -- segment v covers the next seg_items[v] items, the
 * counts sum to n -- with the other arguments of avrf_ring_batch_verify.  Every segment derives its own randomisers, exactly as
 * avrf_ring_batch_verify on its items alone does (a one-item segment: r1 = 1), and gets its own 2-pairing check; the G1 sums of all
 * segments are ONE segmented MSM chain on the device (two vectors per segment, 10 items + 1 and 2 items terms, padded to
 * L = 10 (longest segment) + 1), whose finishing kernel leaves every segment's two points where the pairing kernel reads them.
 * For a caller with many small groups of proofs (a block importer: a handful of tickets per block).
 *   statuses  status_out[v] is what avrf_ring_batch_verify answers for segment v's items alone with the same commitments table;
 *             an empty segment is AVRF_OK.  Where avrf_ring_batch_verify may answer 1 or 2 for a batch that holds both kinds of
 *             defect, this call is deterministic: AVRF_INVALID_DATA wins (a proof point that does not decode or lies outside the
 *             subgroup, an evaluation or lin_zw >= r, an instance coordinate >= r), otherwise AVRF_VERIFICATION_FAILURE.  A defect
 *             marks ITS segment and no other.  The call returns AVRF_OK whenever the statuses were written.
 *   failures  of the call, no status written: a ring commitment that does not decode or lies outside the subgroup gives
 *             AVRF_INVALID_DATA (all 3 n_rings commitments are checked before any segment).  AVRF_ERR_BAD_ARG: counts that do not
 *             sum to n, a ring_of_item entry >= n_rings, a segment of more than 819 items (10 items + 1 <= AVRF_SEGMENT_TERMS_MAX),
 *             a busy handle.  These refusals are decided before anything is decoded or launched; the setup stays usable and
 *             avrf_ring_batch_verify / avrf_ring_verify_each behave as before.
 *   rounds    the NUMBER of segments is never refused: when 2 n_seg windows(L), the padded term count 2 n_seg L
 *             (AVRF_SEGMENTS_PADDED_TERMS_MAX) or the 32-bit entry offsets would be exceeded, the call runs several chains over
 *             consecutive runs of segments.  avrf_ring_segments_layout states them.
 *   pairings  up to 16 segments: on the host pool from the copied-back sums (as avrf_ring_verify_each); more: the device pairing
 *             kernel on the finishing kernel's output.  One segment is exactly avrf_ring_batch_verify.
 * Runtime (tools/ring_segments_bench.py, profiles/ring_segments_bench.txt; one setup, 4 096 valid proofs over one ring
 * of 1 024, Bandersnatch / BLS12-381): 256 segments of 16 proofs 20.8-21.6 ms, 64 x 64 21.8-22.1 ms, 16 x 256 12.6-13.3 ms.  The same
 * groups as separate avrf_ring_batch_verify calls: 513-518 / 256-261 / 82-83 ms (24 x, 12 x, 6 x slower).  avrf_ring_verify_each on the
 * same proofs, one verdict per PROOF: 25.3-25.8 ms -- behind the segmented call, ranges apart; avrf_ring_batch_verify on all of them,
 * ONE verdict: 11.4-11.5 ms.  The host reduction is not what bounds the segmented call (2.1 ms of it): the device pairing kernel
 * takes 9.6 ms whatever it carries and the chain's finishing kernel 3.3-4.0 ms.  Use segments for many small groups and to locate a
 * bad group; use avrf_ring_verify_each when a verdict per proof is what is wanted. */
int avrf_ring_batch_verify_segments(avrf_ring_setup *setup, size_t n, const uint8_t *ring_commitments, size_t n_rings,
                                    const uint32_t *ring_of_item, const uint8_t *instances_xy, const uint8_t *ring_proofs,
                                    size_t n_seg, const uint32_t *seg_items, int32_t *status_out);
/* The layout of such a call (src/ring.rs:682-735: term counts of n_seg BatchVerifiers), host arithmetic only, no device:
 * out = { L, rounds, padded terms of the largest round (2 segments-per-round L), window bits of the L-term MSMs }.
 * AVRF_ERR_BAD_ARG when the counts do not sum to n or a segment has more than 819 items. */
int avrf_ring_segments_layout(size_t n, size_t n_seg, const uint32_t *seg_items, uint64_t out[4]);
/* Test probe, like avrf_thin_segment_terms (src/ring.rs:693-735, the two sums of BatchVerifier::verify): the two G1 sums (canonical
 * little-endian x || y, all-zero = infinity) the last avrf_ring_batch_verify_segments on this setup formed for segment `seg` --
 * all-zero too for an empty segment and for one the host part had condemned before any sum was formed.  AVRF_ERR_BAD_ARG without
 * such a call (or after one that failed) and for seg out of range. */
int avrf_ring_segment_sums(avrf_ring_setup *setup, size_t seg, uint8_t *a_xy, uint8_t *b_xy);

/* The pairing half of the KZG verifier on the device (arkworks `Pairing::multi_pairing` + final exponentiation as reached
 * from RingVerifier::verify, src/ring.rs:242): for i < n,  ok_out[i] = 1 iff  e(A_i, g2) * e(B_i, tau g2) == 1  with (g2, tau g2)
 * the two `powers_in_g2` of the setup's SRS.  a_xy / b_xy: n G1 points each, canonical little-endian x || y (48+48 bytes
 * BLS12-381, 32+32 BN254; all-zero = infinity), assumed on the curve (they are outputs of the verifier's own MSMs).  Miller
 * loops and final exponentiations run as one kernel, an Fp12 element spread over 16 lanes (pairing.hip); the line tables of
 * the two G2 arguments are built on the device at first use (up to 16 checks: on the host pool, see avrf_ring_verify_each).
 * AVRF_INVALID_DATA for a coordinate >= p. */
int avrf_ring_pairing_check(avrf_ring_setup *setup, size_t n, const uint8_t *a_xy, const uint8_t *b_xy, int32_t *ok_out);

/* Input::new(data) = Suite::data_to_point (src/lib.rs:440-444 via src/utils/hash_to_curve.rs:34-100) for n messages:
 * Elligator2 with expand_message_xmd(SHA-512) for Bandersnatch, try-and-increment for Baby-JubJub.  data = the
 * messages concatenated, data_lens[i] their lengths.  out_xy: n x 64; status_out[i] = 0, or 2 (InvalidData) where
 * try-and-increment found no point (the reference returns None). */
int avrf_hash_to_curve(avrf_ctx *ctx, size_t n, const uint8_t *data, const uint32_t *data_lens, uint8_t *out_xy, int32_t *status_out);

/* CanonicalSerialize / CanonicalDeserialize of curve points, batched on the device
 * (ark-serialize compressed form; checked constructors src/lib.rs:410-494).
 * decompress: in n x L -> out n x 64; status_out[j] = AVRF_OK / AVRF_INVALID_DATA; L = avrf_point_len(suite) = 32 for the
 * twisted-Edwards suites (LE32(y), sign of x in bit 255), 33 for the short-Weierstrass presentation (LE32(x) || flags; the
 * xy side is then the TEMapping of the point, src/utils/te_sw_map.rs:32-47).
 * validate != 0 additionally requires prime-order-subgroup membership and non-identity. */
size_t avrf_point_len(int suite);
int avrf_points_decompress(avrf_ctx *ctx, size_t n, const uint8_t *in, uint8_t *out_xy, int validate, int32_t *status_out);
/* Output::hash::<N> (src/lib.rs:605-609 -> Suite::point_to_hash, src/utils/common.rs:290-305): the VRF output bytes `beta` of n
 * output points, hash_len = N <= 64 bytes each.  Secret::from_seed (src/lib.rs:346-369) for n 32-byte seeds: the secret scalars
 * (LE32) and, when pks_xy_out is not NULL, their public keys (Secret::from_scalar).  The device copies of the seeds and scalars are
 * zeroed before the call returns (the reference zeroizes seed and sk, src/lib.rs:367-368); sks_out is the caller's to scrub. */
int avrf_output_hash(avrf_ctx *ctx, size_t n, const uint8_t *points_xy, size_t hash_len, uint8_t *out);
int avrf_secret_from_seed(avrf_ctx *ctx, size_t n, const uint8_t *seeds, uint8_t *sks_out, uint8_t *pks_xy_out);
int avrf_points_compress(avrf_ctx *ctx, size_t n, const uint8_t *in_xy, uint8_t *out);

/* Secret::from_scalar / Secret::output: sk*G and sk*I for a batch (src/lib.rs:331-334,391-393). */
int avrf_scalar_mul_base(avrf_ctx *ctx, size_t n, const uint8_t *sks, uint8_t *out_xy);
int avrf_scalar_mul(avrf_ctx *ctx, size_t n, const uint8_t *scalars, const uint8_t *points_xy, uint8_t *out_xy);

/* ---- Wire-format flavour: the reference's `serialize_compressed` encodings and a `validate` flag. ----
 * Points are L-byte compressed, L = avrf_point_len(suite) (pks: n x L; ios: per pair input(L) || output(L)); proofs are the
 * reference's byte strings: thin R(L) || s(32) (src/thin.rs:43-48), tiny c(16) || s(32) (src/tiny.rs:60-78), pedersen
 * Yb || R || Ok || s || sb = 3 L + 64 (src/pedersen.rs:69-75), ring-VRF = pedersen proof || ring proof = 752 / 640 at L = 32,
 * 755 for Bandersnatch-SW (src/ring.rs:160-166).
 * validate = 0: CanonicalDeserialize with Validate::No (the point must decode, i.e. lie on the curve);
 * validate = 1: Validate::Yes as in the checked constructors (src/lib.rs:410-433): also prime-order subgroup and not the identity.
 * A point that fails gives AVRF_INVALID_DATA (for its item in the per-item calls) before any equation is evaluated.
 * These calls decompress on the device (avrf_points_decompress) and then run the xy entry points above: the xy flavour is
 * the fast path for callers that hold deserialised points, as the reference's own benches do (benches/thin.rs:46-90). */
/* Staging from wire bytes for the three-call run (avrf_*_batch_stage_wire, then avrf_thin_batch_run / avrf_pedersen_batch_run or
 * avrf_batch_run_begin / _hash / _end): every point is decompressed (and validated) on the device straight into the context's
 * staged buffers; AVRF_INVALID_DATA when a point does not decode / fails validation (nothing is staged then).  The *_batch_verify_wire
 * entry points below are exactly stage_wire + run. */
int avrf_thin_batch_stage_wire(avrf_ctx *ctx, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                               const uint32_t *ad_lens, const uint8_t *proofs, int validate);
int avrf_pedersen_batch_stage_wire(avrf_ctx *ctx, size_t n, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                                   const uint32_t *ad_lens, const uint8_t *proofs, int validate);
int avrf_thin_batch_verify_wire(avrf_ctx *ctx, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                                const uint32_t *ad_lens, const uint8_t *proofs, int validate);
int avrf_thin_verify_wire(avrf_ctx *ctx, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                          const uint32_t *ad_lens, const uint8_t *proofs, int validate, int32_t *status_out);
int avrf_tiny_verify_wire(avrf_ctx *ctx, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                          const uint32_t *ad_lens, const uint8_t *proofs, int validate, int32_t *status_out);
int avrf_pedersen_batch_verify_wire(avrf_ctx *ctx, size_t n, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                                    const uint32_t *ad_lens, const uint8_t *proofs, int validate);
int avrf_pedersen_verify_wire(avrf_ctx *ctx, size_t n, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                              const uint32_t *ad_lens, const uint8_t *proofs, int validate, int32_t *status_out);

/* ---- OPEN batches: BatchVerifier::new, push as items arrive, verify (src/thin.rs:188-326, src/pedersen.rs:303-426).
 * The reference's batch verifiers are incremental: `prepare` is "hashing only, no EC ops", so a caller pays for it when an item
 * arrives and leaves the MSM for `verify`.  An open batch is that on the device: every push enqueues its chunk's copies up, wire
 * decoding, validation, the prepare kernel over the chunk's items alone and the copy back of their transcript records, and the
 * host absorbs the records of EARLIER chunks into a running weight transcript -- so that by the time the last item is pushed,
 * `verify` has the last chunk's prepare, the terms kernel and the MSM left to do.
 *
 * verify is the existing calls, which accept an open batch of their kind exactly as a staged one: avrf_thin_batch_run /
 * avrf_pedersen_batch_run, avrf_batch_run_begin / _hash / _end, avrf_*_batch_run_segments, and afterwards avrf_batch_last_terms,
 * avrf_*_segment_terms, avrf_last_timing (the hash phase, out[2], is what was left to absorb).  An open batch into which items
 * 0 .. n-1 were pushed in ANY chunking is indistinguishable from avrf_*_batch_stage of the same items in the same order: same
 * terms bit for bit, same MSM point, same verdict -- AVRF_INVALID_DATA for an identity key / input / output, an out-of-range
 * coordinate or s >= r is found at verify, not at push, as in the reference (src/thin.rs:265-271) -- same segment statuses.  An
 * empty open batch verifies (AVRF_OK).  verify does not consume (verify(&self) borrows): more may be pushed and the batch run
 * again, and that run equals a staging of all items so far.
 *
 * Ownership: a push makes its own page-locked copy of the chunk before it returns, whatever memory the caller's arrays are in
 * (buffers of avrf_host_alloc / avrf_host_register included: they are copied too, not read in place); the caller may reuse them at
 * once.  Apart from that copy a push does NOT wait: everything is enqueued on the context's own stream.  The exception is
 * growth: pushing beyond the hints given to open grows the buffers with what was pushed kept, and that waits for the stream (twice
 * per doubling: before the buffers move and behind the copies that move them), and a page-locked block for the chunk copies is
 * allocated when the current one is full.  Hints that cover the batch avoid both, however many pushes bring it: the chunk copies are
 * packed without padding, so items x (64 + 96) + pairs x 128 + additional data bytes (Pedersen: items x 256 + ..) are enough.
 *
 * Refusals, decided before anything is touched (AVRF_ERR_BAD_ARG, the batch unchanged): no open batch of that kind; a NULL array
 * where the counts need one; the cumulative limits of a staging exceeded (items <= 0x0fffffff, pairs <= 0x1fffffff, additional data
 * <= 0x7fffffff bytes); the context is a slot of a pool; and, for open, push and flush alike, a run in flight on the context
 * (between avrf_batch_run_begin and avrf_batch_run_end).
 * Wire failures are sticky: whether a point of a wire chunk decodes (and passes `validate`) is known only when the chunk's kernels
 * have run; the next push, flush or run then returns AVRF_INVALID_DATA and the batch is gone -- nothing is open or staged, as a
 * failed avrf_*_batch_stage_wire leaves the context -- until a new open.  avrf_batch_flush is how a caller learns it before pushing more.
 * Implicit close: whatever stages on the context, or drops what is staged, ends the open batch (avrf_*_batch_stage*,
 * avrf_*_batch_verify*, the per-item provers and verifiers, the point-wise calls, avrf_msm_*).  A staging call (and a new open) that
 * ends an open batch whose chunks are still queued WAITS for the context's stream first: it is about to rewrite the page-locked
 * offsets and record buffers those chunks read and write.
 * Not covered: open batches over a shared table or through a pool; push_prepared with the caller's challenges; ring batches. */
/* BatchVerifier::new (src/thin.rs:199-202, src/pedersen.rs:316-318) on the context: an OPEN batch, empty.  The hints size the buffers
 * (0 = grow on demand).  Whatever was staged or open on the context before is dropped, as by a *_batch_stage call. */
int avrf_thin_batch_open(avrf_ctx *ctx, size_t items_hint, size_t pairs_hint, size_t ad_bytes_hint);
int avrf_pedersen_batch_open(avrf_ctx *ctx, size_t items_hint, size_t pairs_hint, size_t ad_bytes_hint);
/* BatchVerifier::push for n more items (src/thin.rs:234-243, src/pedersen.rs:324-326; n == 0 is a no-op): the arguments of
 * avrf_thin_batch_stage / avrf_pedersen_batch_stage (x || y) and of avrf_*_batch_stage_wire (serialize_compressed bytes, validate). */
int avrf_thin_batch_push(avrf_ctx *ctx, size_t n, const uint8_t *pks_xy, const uint8_t *ios_xy, const uint32_t *io_counts,
                         const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs);
int avrf_thin_batch_push_wire(avrf_ctx *ctx, size_t n, const uint8_t *pks, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                              const uint32_t *ad_lens, const uint8_t *proofs, int validate);
int avrf_pedersen_batch_push(avrf_ctx *ctx, size_t n, const uint8_t *ios_xy, const uint32_t *io_counts, const uint8_t *ads,
                             const uint32_t *ad_lens, const uint8_t *proofs);
int avrf_pedersen_batch_push_wire(avrf_ctx *ctx, size_t n, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                                  const uint32_t *ad_lens, const uint8_t *proofs, int validate);
/* waits for everything pushed, absorbs it into the running transcript, and reports a sticky wire failure (AVRF_INVALID_DATA) */
int avrf_batch_flush(avrf_ctx *ctx);
/* BatchVerifier::len: the items pushed so far; out (may be NULL) = { items, pairs, bytes of additional data }.  0 when nothing is open. */
size_t avrf_batch_pushed(const avrf_ctx *ctx, size_t out[3]);

/* ring::Prover::prove (src/ring.rs:211-226) as ONE call for n provers of the ring behind `key` (avrf_pedersen_prove +
 * avrf_ring_prove + serialisation): sks n x 32, key_index[i] = position of prover i's key in the ring, ios_xy as for
 * avrf_pedersen_prove; proofs_out: n x (160 + ring_proof_len) bytes, ring::Proof's compressed serialisation.
 * ring_proof_len must equal avrf_ring_proof_len(avrf_ring_key_setup(key)) -- it states the caller's buffer layout and is
 * checked, not trusted (AVRF_ERR_BAD_ARG otherwise, also when ctx and the key's setup are of different suites). */
int avrf_ring_vrf_prove(avrf_ctx *ctx, avrf_ring_key *key, size_t ring_proof_len, size_t n, const uint8_t *sks, const uint32_t *key_index,
                        const uint8_t *ios_xy, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, int blinding_mode,
                        uint8_t *proofs_out);
/* ring::Verifier::verify for every item (each != 0: status_out[i] per proof; src/ring.rs:228-247) or ring::BatchVerifier over
 * all items (each == 0: the return value is the batch's status; src/ring.rs:693-735).  ios wire-format as above; proofs: n x
 * (160 + avrf_ring_proof_len(setup)).  Pedersen half on the context, ring half on the setup (same suite, else AVRF_ERR_BAD_ARG). */
int avrf_ring_vrf_verify(avrf_ctx *ctx, avrf_ring_setup *setup, size_t n, const uint8_t *ring_commitments, size_t n_rings, const uint32_t *ring_of_item,
                         const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads, const uint32_t *ad_lens, const uint8_t *proofs,
                         int validate, int each, int32_t *status_out);
/* n_seg ring::BatchVerifiers (src/ring.rs:682-735) over consecutive runs of the n items, with the arguments of avrf_ring_vrf_verify:
 * the Pedersen half is the segmented Pedersen path on the context (avrf_pedersen_batch_run_segments over the decompressed proofs; a
 * staging or validation failure is returned as avrf_pedersen_batch_verify_segments_wire returns it, no status written), the ring
 * half avrf_ring_batch_verify_segments on the setup with the Yb of the Pedersen proofs as instances; the halves run side by side.
 * status_out[v] is AVRF_INVALID_DATA if either half says so, else AVRF_VERIFICATION_FAILURE if either half is not AVRF_OK, else
 * AVRF_OK.  Mismatched suites, counts that do not sum to n or a segment of more than 819 items give AVRF_ERR_BAD_ARG. */
int avrf_ring_vrf_verify_segments(avrf_ctx *ctx, avrf_ring_setup *setup, size_t n, const uint8_t *ring_commitments, size_t n_rings,
                                  const uint32_t *ring_of_item, const uint8_t *ios, const uint32_t *io_counts, const uint8_t *ads,
                                  const uint32_t *ad_lens, const uint8_t *proofs, int validate, size_t n_seg, const uint32_t *seg_items,
                                  int32_t *status_out);

#ifdef __cplusplus
}
#endif
#endif
