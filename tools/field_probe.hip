// tools/field_probe.hip -- the field layer (fpn.h, and fp256.h's out-of-line inversion) on operands read from a file, results written to a
// file: tests/test_gpu_field.py generates the operands and checks every result against Python integers.  One workgroup of 256 lanes per
// (field, operation).  Stand-alone:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -enable-ipra=0 -Iark_vrf_amd/csrc -o field_probe tools/field_probe.hip && field_probe in.bin out.bin
// File layout (u32 words, fields in the order of main() below; tests/field_vectors.py writes and reads it):
//   in:   per field  n, nw, n x (a, b) with a, b < p, nw x (a, b) with p <= a < 2^(32 N), b < p          (N words per value)
//   out:  per field  one block of N words per item for each operation of enum Op in order, over the n pairs; OP_GE_P and (fields with the
//         top bit clear only) OP_MUL run over the nw wide pairs too, their blocks follow those of the n pairs.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fp256.h"
using namespace avrf;

enum Op { OP_ADD, OP_SUB, OP_NEG, OP_DBL, OP_MUL, OP_SQR, OP_TO_MONT, OP_FROM_MONT, OP_INV, OP_INV_FERMAT, OP_GE_P, OP_ROUNDTRIP, OP_COUNT };

// NF: the field of a VRF suite, whose per-item kernels invert through the out-of-line multiplier (fp_inv_nf / fp_inv_fermat_nf)
template <class F, int OP, bool NF> __global__ void __launch_bounds__(256) k_op(const uint32_t *in, uint32_t n, uint32_t *out) {
  constexpr int N = F::N;
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    const fe<F> a = fp_load<N>(in + 2 * N * (size_t)i), b = fp_load<N>(in + 2 * N * (size_t)i + N);
    fe<F> r = fp_zero<N>();
    if constexpr (OP == OP_ADD) r = fp_add<F>(a, b);
    if constexpr (OP == OP_SUB) r = fp_sub<F>(a, b);
    if constexpr (OP == OP_NEG) r = fp_neg<F>(a);
    if constexpr (OP == OP_DBL) r = fp_dbl<F>(a);
    if constexpr (OP == OP_MUL) r = fp_mul<F>(a, b);
    if constexpr (OP == OP_SQR) r = fp_sqr<F>(a);
    if constexpr (OP == OP_TO_MONT) r = fp_to_mont<F>(a);
    if constexpr (OP == OP_FROM_MONT) r = fp_from_mont<F>(a);
    if constexpr (OP == OP_INV) { if constexpr (NF) r = fp_inv_nf<F>(a); else r = fp_inv_gcd<F>(a); }
    if constexpr (OP == OP_INV_FERMAT) { if constexpr (NF) r = fp_inv_fermat_nf<F>(a); else r = fp_inv<F>(a); }
    if constexpr (OP == OP_GE_P) r.v[0] = ge_p<F>(a) ? 1u : 0u;
    if constexpr (OP == OP_ROUNDTRIP) r = a;
    fp_store(out + N * (size_t)i, r);
  }
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

template <class F, bool NF, int OP = 0> void launch_all(const uint32_t *in, uint32_t n, uint32_t *out) {
  if constexpr (OP < OP_COUNT) {
    hipLaunchKernelGGL((k_op<F, OP, NF>), dim3(1), dim3(256), 0, 0, in, n, out + (size_t)OP * n * F::N);
    launch_all<F, NF, OP + 1>(in, n, out);
  }
}
template <class F, bool NF> void run(const std::vector<uint32_t> &file, size_t &pos, FILE *fo) {
  constexpr int N = F::N;
  if (pos + 2 > file.size()) { fprintf(stderr, "input too short\n"); exit(2); }
  const uint32_t n = file[pos], nw = file[pos + 1];
  const size_t words_in = 2 * (size_t)N * (n + nw);
  if (n == 0 || nw == 0 || pos + 2 + words_in > file.size()) { fprintf(stderr, "input too short\n"); exit(2); }
  const size_t words_out = (size_t)N * ((size_t)OP_COUNT * n + 2 * (size_t)nw);
  uint32_t *d_in, *d_out;
  CK(hipMalloc(&d_in, words_in * 4)); CK(hipMalloc(&d_out, words_out * 4));
  CK(hipMemcpy(d_in, &file[pos + 2], words_in * 4, hipMemcpyHostToDevice));
  CK(hipMemset(d_out, 0xff, words_out * 4));
  launch_all<F, NF>(d_in, n, d_out);
  const uint32_t *d_wide = d_in + 2 * (size_t)N * n;
  uint32_t *o_wide = d_out + (size_t)OP_COUNT * n * N;
  hipLaunchKernelGGL((k_op<F, OP_GE_P, NF>), dim3(1), dim3(256), 0, 0, d_wide, nw, o_wide);
  size_t used = (size_t)N * ((size_t)OP_COUNT * n + nw);
  if constexpr (!F::FULL) { hipLaunchKernelGGL((k_op<F, OP_MUL, NF>), dim3(1), dim3(256), 0, 0, d_wide, nw, o_wide + (size_t)N * nw); used = words_out; }
  CK(hipGetLastError()); CK(hipDeviceSynchronize());
  std::vector<uint32_t> h(used);
  CK(hipMemcpy(h.data(), d_out, used * 4, hipMemcpyDeviceToHost));
  if (fwrite(h.data(), 4, used, fo) != used) { fprintf(stderr, "short write\n"); exit(2); }
  CK(hipFree(d_in)); CK(hipFree(d_out));
  pos += 2 + words_in;
}
int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: field_probe in.bin out.bin\n"); return 2; }
  FILE *fi = fopen(argv[1], "rb"); if (!fi) { perror(argv[1]); return 2; }
  std::vector<uint32_t> file; uint32_t buf[4096]; size_t k;
  while ((k = fread(buf, 4, 4096, fi)) > 0) file.insert(file.end(), buf, buf + k);
  fclose(fi);
  FILE *fo = fopen(argv[2], "wb"); if (!fo) { perror(argv[2]); return 2; }
  size_t pos = 0;
  run<FqBandersnatch, true>(file, pos, fo);      // asm multiplier, subtractive reduction in the unsaturated form
  run<FqEd25519, true>(file, pos, fo);
  run<FqSecp256r1, true>(file, pos, fo);         // F::FULL
  run<FrSecp256r1, true>(file, pos, fo);         // F::FULL
  run<FqBn254, false>(file, pos, fo);            // 8 limbs, G1 / pairing call sites
  run<FqBls12381, false>(file, pos, fo);         // 12 limbs
  if (pos != file.size()) { fprintf(stderr, "input too long\n"); return 2; }
  if (fclose(fo) != 0) { perror(argv[2]); return 2; }
  printf("field probe ok\n");
  return 0;
}
