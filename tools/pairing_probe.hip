// tools/pairing_probe.hip -- the device pairing layer (ark_vrf_amd/csrc/pairing_dev.h) on operands read from a file, results written to a
// file: tests/test_gpu_pairing_values.py generates the operands (tests/pairing_vectors.py) and compares every coefficient of every result
// with oracle/pairing_py.F12 and Python integers.  The kernels here only load operands, call the library's device functions and store: the
// library's geometry (64-lane blocks, sixteen lanes per element, lane k < 12 owns the coefficient of w^k, lanes 12..15 store nothing, the
// groups past the last item repeat it), the library's constant block (pairing_consts) and the library's kernels k_g2_lines and, through
// pairing_miller / pairing_final_exp, the two halves of k_pairing_check.  Stand-alone:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -enable-ipra=0 -Iark_vrf_amd/csrc -o pairing_probe tools/pairing_probe.hip && pairing_probe in.bin out.bin
// File layout (u32 words; every field value is a Montgomery residue of N words, N = 12 for BLS12-381 and 8 for BN254; an Fp12 element is its
// twelve coefficients d_0 .. d_11 of w^0 .. w^11 in the direct basis):
//   in:   curve (0 BLS12-381, 1 BN254), then sections { op, n, np, payload } until the end of the file
//           OP_MUL, OP_MUL_LINE        payload n x (a, b)                 out n elements
//           OP_SQR .. OP_FINAL_EXP     payload n x a                      out n elements
//           OP_G2_LINES                payload n x (x.a, x.b, y.a, y.b)   out n x steps x 36 values (the table of k_g2_lines), then one value
//                                                                         whose first word is the kernel's flag
//           OP_MILLER, OP_MILLER_FE    payload np x (x.a, x.b, y.a, y.b) G2 arguments, then n x np x (x, y) G1 arguments ((0, 0) = infinity)
//                                                                         out n elements: the Miller product, or its final exponentiation
//   out:  the results of the sections in order, nothing else.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pairing_dev.h"
using namespace avrf;

enum Op : uint32_t { OP_MUL = 1, OP_SQR, OP_MUL_LINE, OP_CONJ, OP_FROB2, OP_FROB1, OP_INV, OP_POW_X, OP_FINAL_EXP, OP_CYCLO_SQR /* host program only */,
                     OP_G2_LINES, OP_MILLER, OP_MILLER_FE };

template <class C, uint32_t OP>
__global__ void __launch_bounds__(64, 2) k_f12_op(const uint32_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ cst, uint32_t *__restrict__ out) {
  using F = typename C::Fq; constexpr int N = F::N;
  constexpr uint32_t NIN = (OP == OP_MUL || OP == OP_MUL_LINE) ? 2 : 1;
  const uint32_t k = threadIdx.x & 15;
  uint32_t item = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const bool live = item < n;
  if (!live) item = n - 1;                                       // whole groups only, as k_pairing_check does
  const uint32_t kc = k < 12 ? k : 0;
  const uint32_t *src = in + ((size_t)item * NIN * 12 + kc) * N;
  fe<F> a = fp_load<N>(src), b = fp_load<N>(src + (size_t)(NIN - 1) * 12 * N), r;
  if (k >= 12) { a = fp_zero<N>(); b = fp_zero<N>(); }
  if constexpr (OP == OP_MUL) r = f12_mul<C>(a, b, k, cst);
  if constexpr (OP == OP_SQR) r = f12_sqr<C>(a, k, cst);
  if constexpr (OP == OP_MUL_LINE) r = f12_mul_line<C>(a, b, k, cst);
  if constexpr (OP == OP_CONJ) r = f12_conj<C>(a, k);
  if constexpr (OP == OP_FROB2) r = f12_frob2<C>(a, k, cst);
  if constexpr (OP == OP_FROB1) r = f12_frob1<C>(a, k, cst);
  if constexpr (OP == OP_INV) r = f12_inv<C>(a, k, cst);
  if constexpr (OP == OP_POW_X) r = f12_pow_x<C>(a, k, cst);
  if constexpr (OP == OP_FINAL_EXP) r = pairing_final_exp<C>(a, k, cst);
  if (live && k < 12) fp_store<N>(out + ((size_t)item * 12 + k) * N, r);
}

template <class C, bool FE>
__global__ void __launch_bounds__(64, 2) k_miller(const uint32_t *__restrict__ pts, const uint32_t *__restrict__ tab, const uint32_t *__restrict__ cst, uint32_t n,
                                                  uint32_t np, uint32_t steps, uint32_t *__restrict__ out) {
  using F = typename C::Fq; constexpr int N = F::N;
  const uint32_t k = threadIdx.x & 15;
  uint32_t item = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const bool live = item < n;
  if (!live) item = n - 1;
  fe<F> f = pairing_miller<C>(pts, tab, cst, item, np, steps, k);
  if constexpr (FE) f = pairing_final_exp<C>(f, k, cst);
  if (live && k < 12) fp_store<N>(out + ((size_t)item * 12 + k) * N, f);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)
static void fail(const char *m) { fprintf(stderr, "%s\n", m); exit(2); }

struct Dev {                                                   // one device buffer, freed at the end of its section
  uint32_t *p = nullptr;
  explicit Dev(size_t words) { CK(hipMalloc(&p, words * 4)); CK(hipMemset(p, 0xff, words * 4)); }
  ~Dev() { (void)hipFree(p); }
};
static void emit(FILE *fo, const uint32_t *d, size_t words) {
  CK(hipGetLastError()); CK(hipDeviceSynchronize());
  std::vector<uint32_t> h(words);
  CK(hipMemcpy(h.data(), d, words * 4, hipMemcpyDeviceToHost));
  if (fwrite(h.data(), 4, words, fo) != words) fail("short write");
}

template <class C, uint32_t OP> static void f12_section(const uint32_t *payload, uint32_t n, const uint32_t *d_cst, FILE *fo) {
  constexpr int N = C::Fq::N; constexpr size_t NIN = (OP == OP_MUL || OP == OP_MUL_LINE) ? 2 : 1;
  Dev in(n * NIN * 12 * N), out((size_t)n * 12 * N);
  CK(hipMemcpy(in.p, payload, n * NIN * 12 * N * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL((k_f12_op<C, OP>), dim3((n * 16 + 63) / 64), dim3(64), 0, 0, (const uint32_t *)in.p, n, d_cst, out.p);
  emit(fo, out.p, (size_t)n * 12 * N);
}

template <class C> static void run(const std::vector<uint32_t> &file, FILE *fo) {
  constexpr int N = C::Fq::N;
  const std::vector<uint32_t> csw = pairing_consts<C>();
  const uint32_t steps = (uint32_t)ate_steps<C>();
  Dev cst(csw.size());
  CK(hipMemcpy(cst.p, csw.data(), csw.size() * 4, hipMemcpyHostToDevice));
  size_t pos = 1;
  while (pos < file.size()) {
    if (pos + 3 > file.size()) fail("truncated section header");
    const uint32_t op = file[pos], n = file[pos + 1], np = file[pos + 2];
    pos += 3;
    if (n == 0 || n > 4096 || np > 8) fail("bad section header");
    size_t words;
    switch (op) {
      case OP_MUL: case OP_MUL_LINE: words = (size_t)n * 24 * N; break;
      case OP_SQR: case OP_CONJ: case OP_FROB2: case OP_FROB1: case OP_INV: case OP_POW_X: case OP_FINAL_EXP: words = (size_t)n * 12 * N; break;
      case OP_G2_LINES: words = (size_t)n * 4 * N; break;
      case OP_MILLER: case OP_MILLER_FE: if (np == 0) fail("bad section header"); words = ((size_t)np * 4 + (size_t)n * np * 2) * N; break;
      default: fail("unknown operation"); return;
    }
    if (pos + words > file.size()) fail("truncated section");
    const uint32_t *pl = &file[pos];
    pos += words;
    switch (op) {
      case OP_MUL: f12_section<C, OP_MUL>(pl, n, cst.p, fo); break;
      case OP_SQR: f12_section<C, OP_SQR>(pl, n, cst.p, fo); break;
      case OP_MUL_LINE: f12_section<C, OP_MUL_LINE>(pl, n, cst.p, fo); break;
      case OP_CONJ: f12_section<C, OP_CONJ>(pl, n, cst.p, fo); break;
      case OP_FROB2: f12_section<C, OP_FROB2>(pl, n, cst.p, fo); break;
      case OP_FROB1: f12_section<C, OP_FROB1>(pl, n, cst.p, fo); break;
      case OP_INV: f12_section<C, OP_INV>(pl, n, cst.p, fo); break;
      case OP_POW_X: f12_section<C, OP_POW_X>(pl, n, cst.p, fo); break;
      case OP_FINAL_EXP: f12_section<C, OP_FINAL_EXP>(pl, n, cst.p, fo); break;
      default: {
        const uint32_t nq = op == OP_G2_LINES ? n : np;
        const size_t tab_words = (size_t)nq * steps * 36 * N;
        Dev q((size_t)nq * 4 * N), tab(tab_words + N);            // the value after the table holds the flag
        CK(hipMemcpy(q.p, pl, (size_t)nq * 4 * N * 4, hipMemcpyHostToDevice));
        CK(hipMemset(tab.p + tab_words, 0, (size_t)N * 4));
        hipLaunchKernelGGL(k_g2_lines<C>, dim3((nq + 63) / 64), dim3(64), 0, 0, (const uint32_t *)q.p, nq, steps, (const uint32_t *)cst.p, tab.p, tab.p + tab_words);
        if (op == OP_G2_LINES) { emit(fo, tab.p, tab_words + N); break; }
        Dev pts((size_t)n * np * 2 * N), out((size_t)n * 12 * N);
        CK(hipMemcpy(pts.p, pl + (size_t)np * 4 * N, (size_t)n * np * 2 * N * 4, hipMemcpyHostToDevice));
        const dim3 grid((n * 16 + 63) / 64), block(64);
        if (op == OP_MILLER) hipLaunchKernelGGL((k_miller<C, false>), grid, block, 0, 0, (const uint32_t *)pts.p, (const uint32_t *)tab.p, (const uint32_t *)cst.p, n, np, steps, out.p);
        else hipLaunchKernelGGL((k_miller<C, true>), grid, block, 0, 0, (const uint32_t *)pts.p, (const uint32_t *)tab.p, (const uint32_t *)cst.p, n, np, steps, out.p);
        emit(fo, out.p, (size_t)n * 12 * N);
      }
    }
  }
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: pairing_probe in.bin out.bin\n"); return 2; }
  FILE *fi = fopen(argv[1], "rb"); if (!fi) { perror(argv[1]); return 2; }
  std::vector<uint32_t> file; uint32_t buf[4096]; size_t k;
  while ((k = fread(buf, 4, 4096, fi)) > 0) file.insert(file.end(), buf, buf + k);
  fclose(fi);
  if (file.empty() || file[0] > 1) fail("bad curve id");
  FILE *fo = fopen(argv[2], "wb"); if (!fo) { perror(argv[2]); return 2; }
  if (file[0] == 0) run<G1Bls12381>(file, fo); else run<G1Bn254>(file, fo);
  if (fclose(fo) != 0) { perror(argv[2]); return 2; }
  printf("pairing probe ok\n");
  return 0;
}
