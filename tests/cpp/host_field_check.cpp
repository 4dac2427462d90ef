// CPU-only check of the product's host field (host_te.h HostField) on every field struct of consts_gen.h: reads operands from a file,
// writes the results of every operation to a file; tests/test_host_logic.py generates the operands and compares with Python integers.
//   g++ -std=c++17 -O2 host_field_check.cpp -o hf && ./hf in.bin out.bin
// File layout (u32 words, fields in the order of main() below; tests/field_vectors.py writes and reads it -- the layout of tools/field_probe.hip):
//   in:   per field  n, nw, n x (a, b) with a, b < p, nw x (a, b) with p <= a < 2^(32 N), b < p          (N words per value)
//   out:  per field  one block of N words per item for each operation of enum Op in order, over the n pairs; then geq_p and (fields with
//         the top bit clear only) mul over the nw wide pairs.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../ark_vrf_amd/csrc/host_te.h"
using namespace avrf;

enum Op { OP_ADD, OP_SUB, OP_NEG, OP_DBL, OP_MUL, OP_SQR, OP_TO_MONT, OP_FROM_MONT, OP_INV, OP_INV_FERMAT, OP_GEQ_P, OP_ROUNDTRIP, OP_COUNT };

template <class F> static typename HostField<F>::El apply(int op, const typename HostField<F>::El &a, const typename HostField<F>::El &b) {
  using H = HostField<F>;
  switch (op) {
    case OP_ADD: return H::add(a, b);
    case OP_SUB: return H::sub(a, b);
    case OP_NEG: return H::neg(a);
    case OP_DBL: return H::dbl(a);
    case OP_MUL: return H::mul(a, b);
    case OP_SQR: return H::sqr(a);
    case OP_TO_MONT: return H::to_mont(a);
    case OP_FROM_MONT: return H::from_mont(a);
    case OP_INV: return H::inv(a);
    case OP_INV_FERMAT: return H::inv_fermat(a);
    case OP_GEQ_P: { typename H::El r = H::zero(); r.l[0] = H::geq_p(a) ? 1 : 0; return r; }
    default: { uint8_t bytes[8 * H::L]; H::store_le(bytes, a); return H::load_le(bytes); }
  }
}
template <class F> static void run(const std::vector<uint32_t> &file, size_t &pos, FILE *fo) {
  using H = HostField<F>; using El = typename H::El;
  constexpr int N = F::N;
  static_assert(sizeof(El) == 4 * N, "an element is the device's N words");
  if (pos + 2 > file.size()) { fprintf(stderr, "input too short\n"); exit(2); }
  const size_t n = file[pos], nw = file[pos + 1];
  if (pos + 2 + 2 * N * (n + nw) > file.size()) { fprintf(stderr, "input too short\n"); exit(2); }
  const uint32_t *pairs = &file[pos + 2], *wide = pairs + 2 * N * n;
  auto item = [&](int op, const uint32_t *w) {
    El a, b, r; memcpy(a.l, w, 4 * N); memcpy(b.l, w + N, 4 * N);
    r = apply<F>(op, a, b);
    if (fwrite(r.l, 4, N, fo) != (size_t)N) { fprintf(stderr, "short write\n"); exit(2); }
  };
  for (int op = 0; op < OP_COUNT; op++) for (size_t i = 0; i < n; i++) item(op, pairs + 2 * N * i);
  for (size_t i = 0; i < nw; i++) item(OP_GEQ_P, wide + 2 * N * i);
  if (!F::FULL) for (size_t i = 0; i < nw; i++) item(OP_MUL, wide + 2 * N * i);
  pos += 2 + 2 * N * (n + nw);
}
int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: host_field_check in.bin out.bin\n"); return 2; }
  FILE *fi = fopen(argv[1], "rb"); if (!fi) { perror(argv[1]); return 2; }
  std::vector<uint32_t> file; uint32_t buf[4096]; size_t k;
  while ((k = fread(buf, 4, 4096, fi)) > 0) file.insert(file.end(), buf, buf + k);
  fclose(fi);
  FILE *fo = fopen(argv[2], "wb"); if (!fo) { perror(argv[2]); return 2; }
  size_t pos = 0;
  run<FqBandersnatch>(file, pos, fo); run<FrBandersnatch>(file, pos, fo);
  run<FqBabyJubJub>(file, pos, fo); run<FrBabyJubJub>(file, pos, fo);
  run<FrJubJub>(file, pos, fo);
  run<FqEd25519>(file, pos, fo); run<FrEd25519>(file, pos, fo);
  run<FqSecp256r1>(file, pos, fo); run<FrSecp256r1>(file, pos, fo);
  run<FqBls12381>(file, pos, fo); run<FqBn254>(file, pos, fo);
  if (pos != file.size()) { fprintf(stderr, "input too long\n"); return 2; }
  if (fclose(fo) != 0) { perror(argv[2]); return 2; }
  printf("host field ok\n");
  return 0;
}
