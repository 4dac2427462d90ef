// tools/fpu_probe.hip -- the unsaturated-limb field and point layer (fpu.h, fpu_te.h, fpu_g1.h, fpu_sqrt.h) on operands read from a file,
// raw results written to a file: tests/fpu_vectors.py places the operands at the ends of the intervals the headers document and
// tests/test_gpu_fpu.py checks every result against Python integers.  One workgroup of 256 lanes per (type, operation).  Stand-alone:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -enable-ipra=0 -Iark_vrf_amd/csrc -o fpu_probe tools/fpu_probe.hip && fpu_probe in.bin out.bin
// (a second build with -DAVRF_NO_FPU_ASM runs the C++ multipliers in place of the generated asm blocks on the same input, less the square-root jobs).
// File layout (u32 words; tests/fpu_vectors.py writes and reads it):
//   in:   per job, in the order of main() below:  job index, n, IN, OUT, then n x IN words.  n is a multiple of 64 (whole waves: g1u_madd and
//         g1r_add vote with __any), IN / OUT are the words per case of the job's Op struct (checked against the header).
//   out:  per job  n x OUT words.  Limbs are written as they leave the function (int32 as u32), canonical values as N saturated words.
// Records:  te accumulator = x y t z (L limbs each) + neg (37 words);  teu4 = x y t z (36);  te_pre = x y k, te_ext = x y t z (8 words each);
//           G1 accumulator / reduction point = x y zz zzz (L limbs each) + inf (4 L + 1 words).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fpu_te.h"
#include "curves.h"
#include "fpu_sqrt.h"
using namespace avrf;

template <int L> __device__ __forceinline__ fu<L> ld_fu(const uint32_t *p) { fu<L> r;
#pragma unroll
  for (int i = 0; i < L; i++) r.v[i] = (int32_t)p[i];
  return r; }
template <int L> __device__ __forceinline__ void st_fu(uint32_t *p, const fu<L> &a) {
#pragma unroll
  for (int i = 0; i < L; i++) p[i] = (uint32_t)a.v[i]; }
template <int N> __device__ __forceinline__ void ld_w(uint32_t (&w)[N], const uint32_t *p) {
#pragma unroll
  for (int i = 0; i < N; i++) w[i] = p[i]; }
template <int N> __device__ __forceinline__ void st_w(uint32_t *p, const uint32_t (&w)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) p[i] = w[i]; }

// ---- field level
template <class F, int S> struct OpSlice { static constexpr int IN = UL<F>::N, OUT = UL<F>::L;
  static __device__ void run(const uint32_t *in, uint32_t *out) { uint32_t w[UL<F>::N]; ld_w(w, in); st_fu(out, fu_slice<F, S>(w)); } };
template <class F> struct OpCneg { static constexpr int L = UL<F>::L, IN = L + 1, OUT = L;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_fu(out, fu_cneg<L>(ld_fu<L>(in), (int32_t)in[L])); } };
template <class F> struct OpCarry { static constexpr int L = UL<F>::L, IN = L, OUT = L;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_fu(out, fu_carry<F>(ld_fu<L>(in))); } };
// B + 5 A as teu_madd forms it: in = A | B
template <class F> struct OpCarryU { static constexpr int L = UL<F>::L, IN = 2 * L, OUT = L;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    const fu<L> A = ld_fu<L>(in), B = ld_fu<L>(in + L);
    uint32_t h[L - 1];
#pragma unroll
    for (int i = 0; i < L - 1; i++) h[i] = (uint32_t)B.v[i] + 5u * (uint32_t)A.v[i];
    st_fu(out, fu_carry_u<F>(h, B.v[L - 1] + 5 * A.v[L - 1]));
  } };
template <class F> struct OpTimes5 { static constexpr int L = UL<F>::L, IN = L, OUT = L;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_fu(out, fu_times5<F>(ld_fu<L>(in))); } };
template <class F> struct OpMul { static constexpr int L = UL<F>::L, IN = 2 * L, OUT = L;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_fu(out, fu_mul<F>(ld_fu<L>(in), ld_fu<L>(in + L))); } };
template <class F> struct OpSqr { static constexpr int L = UL<F>::L, IN = L, OUT = L;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_fu(out, fu_sqr<F>(ld_fu<L>(in))); } };
template <class F, int KB> struct OpPacked { static constexpr int L = UL<F>::L, IN = L, OUT = UL<F>::N;
  static __device__ void run(const uint32_t *in, uint32_t *out) { uint32_t w[UL<F>::N]; fu_to_packed<F, KB>(w, ld_fu<L>(in)); st_w(out, w); } };
// flags: is_zero_mod_p, maybe_zero_mod_p, is_zero_mod_p2, maybe_zero_mod_p2
template <class F> struct OpZero { static constexpr int L = UL<F>::L, IN = L, OUT = 4;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    const fu<L> a = ld_fu<L>(in);
    out[0] = fu_is_zero_mod_p<F>(a) ? 1u : 0u; out[1] = fu_maybe_zero_mod_p<F>(a) ? 1u : 0u;
    out[2] = fu_is_zero_mod_p2<F>(a) ? 1u : 0u; out[3] = fu_maybe_zero_mod_p2<F>(a) ? 1u : 0u;
  } };

// ---- twisted Edwards
template <class S> __device__ __forceinline__ te_acc_u<S> ld_acc(const uint32_t *p) {
  te_acc_u<S> a; a.x = ld_fu<9>(p); a.y = ld_fu<9>(p + 9); a.t = ld_fu<9>(p + 18); a.z = ld_fu<9>(p + 27); a.neg = p[36]; return a; }
template <class S> __device__ __forceinline__ void st_acc(uint32_t *p, const te_acc_u<S> &a) {
  st_fu(p, a.x); st_fu(p + 9, a.y); st_fu(p + 18, a.t); st_fu(p + 27, a.z); p[36] = a.neg; }
template <class S> __device__ __forceinline__ teu4<S> ld_t4(const uint32_t *p) {
  teu4<S> a; a.x = ld_fu<9>(p); a.y = ld_fu<9>(p + 9); a.t = ld_fu<9>(p + 18); a.z = ld_fu<9>(p + 27); return a; }
template <class S> __device__ __forceinline__ void st_t4(uint32_t *p, const teu4<S> &a) { st_fu(p, a.x); st_fu(p + 9, a.y); st_fu(p + 18, a.t); st_fu(p + 27, a.z); }
__device__ __forceinline__ te_pre ld_pre(const uint32_t *p) { te_pre q; ld_w(q.x.v, p); ld_w(q.y.v, p + 8); ld_w(q.k.v, p + 16); return q; }
__device__ __forceinline__ te_ext ld_ext(const uint32_t *p) { te_ext e; ld_w(e.x.v, p); ld_w(e.y.v, p + 8); ld_w(e.t.v, p + 16); ld_w(e.z.v, p + 24); return e; }
__device__ __forceinline__ void st_ext(uint32_t *p, const te_ext &e) { st_w(p, e.x.v); st_w(p + 8, e.y.v); st_w(p + 16, e.t.v); st_w(p + 24, e.z.v); }

template <class S> struct OpTeFromPre { static constexpr int IN = 25, OUT = 37;                          // te_pre | neg
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_acc<S>(out, teu_from_pre<S>(ld_pre(in), in[24] != 0)); } };
template <class S> struct OpTeMadd { static constexpr int IN = 37 + 24 + 1, OUT = 37;                    // accumulator | te_pre | neg
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_acc<S>(out, teu_madd<S>(ld_acc<S>(in), ld_pre(in + 37), in[61] != 0)); } };
template <class S> struct OpTeToExt { static constexpr int IN = 37, OUT = 32;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_ext(out, teu_to_ext<S>(ld_acc<S>(in))); } };
// out: the 40 stored words | teu_load_part | teu_load_part_coord 0..3 | teu_load_part_coord_raw 0..3
template <class S> struct OpTePart { static constexpr int IN = 37, OUT = TEU_PART_WORDS + 32 + 32 + 36;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    teu_store_part<S>(out, ld_acc<S>(in));
    st_ext(out + 40, teu_load_part<S>(out));
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const fp c = teu_load_part_coord<S>(out, j); st_w(out + 72 + 8 * j, c.v);
      st_fu(out + 104 + 9 * j, teu_load_part_coord_raw<S>(out, j));
    }
  } };
template <class S> struct OpT4FromExt { static constexpr int IN = 32, OUT = 36;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_t4<S>(out, teu4_from_ext<S>(ld_ext(in))); } };
template <class S> struct OpT4Dbl { static constexpr int IN = 36, OUT = 36;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_t4<S>(out, teu4_dbl<S>(ld_t4<S>(in))); } };
template <class S> struct OpT4AddSat { static constexpr int IN = 36 + 32, OUT = 36;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_t4<S>(out, teu4_add_sat<S>(ld_t4<S>(in), ld_ext(in + 36))); } };
template <class S> struct OpT4MaddPre { static constexpr int IN = 36 + 24, OUT = 36;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_t4<S>(out, teu4_madd_pre<S>(ld_t4<S>(in), ld_pre(in + 36))); } };
template <class S> struct OpT4ToExt { static constexpr int IN = 36, OUT = 32;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_ext(out, teu4_to_ext<S>(ld_t4<S>(in))); } };

// ---- G1 (XYZZ)
template <class C> struct G1Rec { static constexpr int L = UL<typename C::Fq>::L, N = C::Fq::N, W = 4 * L + 1, PART = G1UPart<C>::WORDS; };
template <class C, class P> __device__ __forceinline__ P ld_g1(const uint32_t *p) { constexpr int L = G1Rec<C>::L;
  P a; a.x = ld_fu<L>(p); a.y = ld_fu<L>(p + L); a.zz = ld_fu<L>(p + 2 * L); a.zzz = ld_fu<L>(p + 3 * L); a.inf = p[4 * L]; return a; }
template <class C, class P> __device__ __forceinline__ void st_g1(uint32_t *p, const P &a) { constexpr int L = G1Rec<C>::L;
  st_fu(p, a.x); st_fu(p + L, a.y); st_fu(p + 2 * L, a.zz); st_fu(p + 3 * L, a.zzz); p[4 * L] = a.inf; }

template <class C> struct OpG1FromAffine { using R = G1Rec<C>; static constexpr int IN = 2 * R::N + 1, OUT = R::W;   // x | y | neg
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    uint32_t x[R::N], y[R::N]; ld_w(x, in); ld_w(y, in + R::N);
    st_g1<C>(out, g1u_from_affine<C>(x, y, in[2 * R::N] != 0));
  } };
template <class C> struct OpG1FromXyzz { using R = G1Rec<C>; static constexpr int IN = 4 * R::N, OUT = R::W;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    uint32_t x[R::N], y[R::N], zz[R::N], zzz[R::N]; ld_w(x, in); ld_w(y, in + R::N); ld_w(zz, in + 2 * R::N); ld_w(zzz, in + 3 * R::N);
    st_g1<C>(out, g1u_from_xyzz<C>(x, y, zz, zzz));
  } };
// accumulator | x | y | neg; the doubling is what k_accumulate passes (curves.h AccumG1U::madd)
template <class C> struct OpG1Madd { using R = G1Rec<C>; static constexpr int IN = R::W + 2 * R::N + 1, OUT = R::W;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    using CV = G1Curve<C>; using Fq = typename C::Fq;
    typename CV::base_t q; ld_w(q.x.v, in + R::W); ld_w(q.y.v, in + R::W + R::N);
    const bool neg = in[R::W + 2 * R::N] != 0;
    st_g1<C>(out, g1u_madd<C>(ld_g1<C, g1_acc_u<C>>(in), q.x.v, q.y.v, neg, [&]() {
      typename CV::base_t t = q; if (neg) t.y = fp_neg<Fq>(t.y);
      const typename CV::acc_t r = CV::dbl_affine(t);
      return g1u_from_xyzz<C>(r.x.v, r.y.v, r.zz.v, r.zzz.v);
    }));
  } };
// out: the stored words | g1u_load_part's x y zz zzz
template <class C> struct OpG1Part { using R = G1Rec<C>; static constexpr int IN = R::W, OUT = R::PART + 4 * R::N;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    g1u_store_part<C>(out, ld_g1<C, g1_acc_u<C>>(in));
    uint32_t x[R::N], y[R::N], zz[R::N], zzz[R::N];
    g1u_load_part<C>(out, x, y, zz, zzz);
    st_w(out + R::PART, x); st_w(out + R::PART + R::N, y); st_w(out + R::PART + 2 * R::N, zz); st_w(out + R::PART + 3 * R::N, zzz);
  } };
template <class C> struct OpG1rFromSat { using R = G1Rec<C>; static constexpr int IN = 4 * R::N, OUT = R::W;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    uint32_t x[R::N], y[R::N], zz[R::N], zzz[R::N]; ld_w(x, in); ld_w(y, in + R::N); ld_w(zz, in + 2 * R::N); ld_w(zzz, in + 3 * R::N);
    st_g1<C>(out, g1r_from_sat<C>(x, y, zz, zzz));
  } };
template <class C> struct OpG1rDbl { using R = G1Rec<C>; static constexpr int IN = R::W, OUT = R::W;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_g1<C>(out, g1r_dbl<C>(ld_g1<C, g1_red<C>>(in))); } };
template <class C> struct OpG1rAdd { using R = G1Rec<C>; static constexpr int IN = 2 * R::W, OUT = R::W;
  static __device__ void run(const uint32_t *in, uint32_t *out) { st_g1<C>(out, g1r_add<C>(ld_g1<C, g1_red<C>>(in), ld_g1<C, g1_red<C>>(in + R::W))); } };
template <class C> struct OpG1rToSat { using R = G1Rec<C>; static constexpr int IN = R::W, OUT = 4 * R::N;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    uint32_t x[R::N], y[R::N], zz[R::N], zzz[R::N];
    g1r_to_sat<C>(ld_g1<C, g1_red<C>>(in), x, y, zz, zzz);
    st_w(out, x); st_w(out + R::N, y); st_w(out + 2 * R::N, zz); st_w(out + 3 * R::N, zzz);
  } };
// out: the stored words | g1r_load's record (padded to a multiple of four words: every case's stores are 16-byte aligned)
template <class C> struct OpG1rStore { using R = G1Rec<C>; static constexpr int IN = R::W, OUT = (R::PART + R::W + 3) / 4 * 4;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    g1r_store<C>(out, ld_g1<C, g1_red<C>>(in));
    st_g1<C>(out + R::PART, g1r_load<C>(out));
  } };

// ---- square root: u | v (saturated Montgomery words) -> flag, root of fu_sqrt_ratio_nf | flag, root of fp_sqrt_ratio_nf
#ifndef AVRF_NO_FPU_ASM
template <class F> struct OpSqrt { static constexpr int IN = 16, OUT = 18;
  static __device__ void run(const uint32_t *in, uint32_t *out) {
    fp u, v, r; ld_w(u.v, in); ld_w(v.v, in + 8);
    out[0] = fu_sqrt_ratio_nf<F>(u, v, &r) ? 1u : 0u; st_w(out + 1, r.v);
    out[9] = fp_sqrt_ratio_nf<F>(u, v, &r) ? 1u : 0u; st_w(out + 10, r.v);
  } };
#endif

template <class OP> __global__ void __launch_bounds__(256) k_job(const uint32_t *in, uint32_t n, uint32_t *out) {
  for (uint32_t i = threadIdx.x; i < n; i += 256) OP::run(in + (size_t)OP::IN * i, out + (size_t)OP::OUT * i);   // n % 64 == 0: whole waves
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

struct Ctx { std::vector<uint32_t> file; size_t pos = 0; uint32_t index = 0; FILE *fo = nullptr; };
template <class OP> void job(Ctx &c) {
  if (c.pos + 4 > c.file.size()) { fprintf(stderr, "job %u: input too short\n", c.index); exit(2); }
  const uint32_t idx = c.file[c.pos], n = c.file[c.pos + 1], in_w = c.file[c.pos + 2], out_w = c.file[c.pos + 3];
  if (idx != c.index || in_w != (uint32_t)OP::IN || out_w != (uint32_t)OP::OUT || n == 0 || n % 64 != 0 || n > (1u << 20)) {
    fprintf(stderr, "job %u: header (%u, %u, %u, %u) does not match (IN %d, OUT %d, n a multiple of 64)\n", c.index, idx, n, in_w, out_w, OP::IN, OP::OUT); exit(2);
  }
  const size_t words_in = (size_t)n * OP::IN, words_out = (size_t)n * OP::OUT;
  if (c.pos + 4 + words_in > c.file.size()) { fprintf(stderr, "job %u: input too short\n", c.index); exit(2); }
  uint32_t *d_in, *d_out;
  CK(hipMalloc(&d_in, words_in * 4)); CK(hipMalloc(&d_out, words_out * 4));
  CK(hipMemcpy(d_in, &c.file[c.pos + 4], words_in * 4, hipMemcpyHostToDevice));
  CK(hipMemset(d_out, 0xff, words_out * 4));
  hipLaunchKernelGGL((k_job<OP>), dim3(1), dim3(256), 0, 0, d_in, n, d_out);
  CK(hipGetLastError()); CK(hipDeviceSynchronize());
  std::vector<uint32_t> h(words_out);
  CK(hipMemcpy(h.data(), d_out, words_out * 4, hipMemcpyDeviceToHost));
  if (fwrite(h.data(), 4, words_out, c.fo) != words_out) { fprintf(stderr, "short write\n"); exit(2); }
  CK(hipFree(d_in)); CK(hipFree(d_out));
  c.pos += 4 + words_in; c.index++;
}
// the order of tests/fpu_vectors.py field_jobs / te_jobs / g1_jobs
template <class F> void field_jobs(Ctx &c) {
  job<OpSlice<F, 0>>(c); job<OpSlice<F, UL<F>::SH>>(c); job<OpCneg<F>>(c); job<OpCarry<F>>(c); job<OpCarryU<F>>(c); job<OpTimes5<F>>(c);
  job<OpMul<F>>(c); job<OpSqr<F>>(c); job<OpPacked<F, 2>>(c); job<OpZero<F>>(c);
}
template <class C> void g1_field_jobs(Ctx &c) {      // the base and entry shifts of G1U<C>
  using F = typename C::Fq; using K = G1U<C>;
  job<OpSlice<F, K::a>>(c); job<OpSlice<F, K::b>>(c); job<OpSlice<F, K::sx>>(c); job<OpSlice<F, K::sy>>(c);
}
template <class S> void te_jobs(Ctx &c) {
  job<OpTeFromPre<S>>(c); job<OpTeMadd<S>>(c); job<OpTeToExt<S>>(c); job<OpTePart<S>>(c);
  job<OpT4FromExt<S>>(c); job<OpT4Dbl<S>>(c); job<OpT4AddSat<S>>(c); job<OpT4MaddPre<S>>(c); job<OpT4ToExt<S>>(c);
}
template <class C> void g1_jobs(Ctx &c) {
  job<OpG1FromAffine<C>>(c); job<OpG1FromXyzz<C>>(c); job<OpG1Madd<C>>(c); job<OpG1Part<C>>(c);
  job<OpG1rFromSat<C>>(c); job<OpG1rDbl<C>>(c); job<OpG1rAdd<C>>(c); job<OpG1rToSat<C>>(c); job<OpG1rStore<C>>(c);
}
int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: fpu_probe in.bin out.bin\n"); return 2; }
  Ctx c;
  FILE *fi = fopen(argv[1], "rb"); if (!fi) { perror(argv[1]); return 2; }
  uint32_t buf[4096]; size_t k;
  while ((k = fread(buf, 4, 4096, fi)) > 0) c.file.insert(c.file.end(), buf, buf + k);
  fclose(fi);
  c.fo = fopen(argv[2], "wb"); if (!c.fo) { perror(argv[2]); return 2; }
  field_jobs<FqBandersnatch>(c);                     // subtractive reduction
  field_jobs<FqBabyJubJub>(c);
  field_jobs<FqEd25519>(c);
  field_jobs<FqBn254>(c); g1_field_jobs<G1Bn254>(c);
  field_jobs<FqBls12381>(c); g1_field_jobs<G1Bls12381>(c);        // 14 x 28
  job<OpPacked<FqBls12381, 4>>(c);                   // g1u_load_part: X of an affine point stored as it entered
  te_jobs<SuiteBandersnatch>(c);                     // a = -5
  te_jobs<SuiteBabyJubJub>(c);                       // a = 1
  te_jobs<SuiteJubJub>(c);                           // a = -1
  te_jobs<SuiteEd25519>(c);                          // a = -1, p = 2^255 - 19
  g1_jobs<G1Bls12381>(c);
  g1_jobs<G1Bn254>(c);
#ifndef AVRF_NO_FPU_ASM     // (with the C++ multipliers inlined the out-of-line fu_sqrt_ratio_nf is the shape tools/lint_device_code.py fences off: not built)
  job<OpSqrt<FqBandersnatch>>(c); job<OpSqrt<FqBabyJubJub>>(c); job<OpSqrt<FqEd25519>>(c);
#endif
  if (c.pos != c.file.size()) { fprintf(stderr, "input too long\n"); return 2; }
  if (fclose(c.fo) != 0) { perror(argv[2]); return 2; }
  printf("fpu probe ok\n");
  return 0;
}
