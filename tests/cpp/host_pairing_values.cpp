// CPU-only run of the product's host pairing (host_pairing.h) on operands from a file, every result written to a file:
// tests/test_host_pairing_values.py generates the operands and compares every value with oracle/pairing_py.F12 and Python integers.
// The file layout is the one of tools/pairing_probe.hip (sections { op, n, np, payload }; Montgomery residues of N 32-bit words), except
// that an Fp12 element is the twelve values of struct F12 as they lie in memory (tests/pairing_vectors.py converts), and:
//   OP_MUL_LINE    the second operand is a line in the sparse shape of HostPairing::line(); f12_mul_line gets its c, m and yP
//   OP_CYCLO_SQR   f12_cyclo_sqr (operands in the cyclotomic subgroup); OP_POW_X squares with it too, so its operands are in that subgroup
//   OP_G2_LINES    out: per G2 point and step lam.a, lam.b, c.a, c.b; then one value whose first word is 1 if a table is not complete
//   OP_MILLER      out: 3 x n elements: miller() (generic), miller_lines(), miller_lines_par();   OP_MILLER_FE: final_exp of each
// Usage: host_pairing_values in.bin out.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ark_vrf_amd/csrc/host_pairing.h"

using namespace avrf;

enum Op : uint32_t { OP_MUL = 1, OP_SQR, OP_MUL_LINE, OP_CONJ, OP_FROB2, OP_FROB1, OP_INV, OP_POW_X, OP_FINAL_EXP, OP_CYCLO_SQR, OP_G2_LINES, OP_MILLER, OP_MILLER_FE };

static void fail(const char *m) { fprintf(stderr, "%s\n", m); exit(2); }

template <class G> static void run(const std::vector<uint32_t> &file, FILE *fo) {
  using HP = HostPairing<G>; using Fp = typename HP::Fp; using El = typename HP::El; using F12 = typename HP::F12; using F2 = typename HP::F2;
  constexpr int N = G::Fq::N;
  static_assert(sizeof(El) == 4 * N && sizeof(F12) == 12 * sizeof(El) && sizeof(F2) == 2 * sizeof(El), "an F12 is twelve packed field elements");
  auto put = [&](const void *p, size_t bytes) { if (fwrite(p, 1, bytes, fo) != bytes) fail("short write"); };
  size_t pos = 1;
  while (pos < file.size()) {
    if (pos + 3 > file.size()) fail("truncated section header");
    const uint32_t op = file[pos], n = file[pos + 1], np = file[pos + 2];
    pos += 3;
    if (n == 0 || n > 4096 || np > 8) fail("bad section header");
    size_t words;
    if (op == OP_MUL || op == OP_MUL_LINE) words = (size_t)n * 24 * N;
    else if (op >= OP_SQR && op <= OP_CYCLO_SQR) words = (size_t)n * 12 * N;
    else if (op == OP_G2_LINES) words = (size_t)n * 4 * N;
    else if ((op == OP_MILLER || op == OP_MILLER_FE) && np > 0) words = ((size_t)np * 4 + (size_t)n * np * 2) * N;
    else { fail("unknown operation"); return; }
    if (pos + words > file.size()) fail("truncated section");
    const uint32_t *pl = &file[pos];
    pos += words;
    auto el_at = [&](size_t i) { El e; memcpy(&e, pl + i * N, 4 * N); return e; };
    auto f12_at = [&](size_t i) { F12 e; memcpy(&e, pl + i * 12 * N, 12 * 4 * N); return e; };
    auto g2_at = [&](size_t i) { typename HP::G2 q; q.x = HP::f2(el_at(4 * i), el_at(4 * i + 1)); q.y = HP::f2(el_at(4 * i + 2), el_at(4 * i + 3)); q.inf = false; return q; };
    if (op <= OP_CYCLO_SQR) {
      const size_t nin = (op == OP_MUL || op == OP_MUL_LINE) ? 2 : 1;
      for (uint32_t i = 0; i < n; i++) {
        const F12 a = f12_at(i * nin), b = f12_at(i * nin + nin - 1);
        F12 r;
        switch (op) {
          case OP_MUL: r = HP::f12_mul(a, b); break;
          case OP_SQR: r = HP::f12_sqr(a); break;
          case OP_MUL_LINE:
            if (G::MTWIST) r = HP::f12_mul_line(a, b.c0.c0, b.c0.c1, b.c1.c1.a);      // (c + m v) + (yP v) w
            else r = HP::f12_mul_line(a, b.c1.c1, b.c1.c0, b.c0.c0.a);                // (yP) + (m + c v) w
            break;
          case OP_CONJ: r = HP::f12_conj(a); break;
          case OP_FROB2: r = HP::f12_frob2(a); break;
          case OP_FROB1: r = HP::f12_frob1(a); break;
          case OP_INV: r = HP::f12_inv(a); break;
          case OP_POW_X: r = HP::f12_pow_x(a); break;
          case OP_FINAL_EXP: r = HP::final_exp(a); break;
          default: r = HP::f12_cyclo_sqr(a); break;
        }
        put(&r, sizeof r);
      }
    } else if (op == OP_G2_LINES) {
      const size_t steps = [] { size_t s = 0; for (int bit = G::ATE_LOOP_BITS - 2; bit >= 0; bit--) s += 1 + ((G::ATE_LOOP[bit >> 6] >> (bit & 63)) & 1); return s; }();
      uint32_t flag[N] = {0};
      for (uint32_t i = 0; i < n; i++) {
        const typename HP::G2Lines t = HP::g2_lines(g2_at(i));
        if (t.inf || t.live_steps != steps || t.lam.size() != steps || t.c.size() != steps) flag[0] = 1;
        for (size_t s = 0; s < steps; s++) {
          const F2 zero = HP::f2_zero();
          put(s < t.lam.size() ? &t.lam[s] : &zero, sizeof(F2)); put(s < t.c.size() ? &t.c[s] : &zero, sizeof(F2));
        }
      }
      put(flag, sizeof flag);
    } else {
      std::vector<typename HP::G2> q(np);
      std::vector<typename HP::G2Lines> tabs(np);
      for (uint32_t j = 0; j < np; j++) { q[j] = g2_at(j); tabs[j] = HP::g2_lines(q[j]); }
      std::vector<F12> res(3 * (size_t)n);
      std::vector<El> px(np), py(np);
      bool pinf[8];                                               // np <= 8
      for (uint32_t i = 0; i < n; i++) {
        for (uint32_t j = 0; j < np; j++) {
          px[j] = el_at((size_t)np * 4 + ((size_t)i * np + j) * 2); py[j] = el_at((size_t)np * 4 + ((size_t)i * np + j) * 2 + 1);
          pinf[j] = Fp::is_zero(px[j]) && Fp::is_zero(py[j]);
        }
        res[i] = HP::miller(px.data(), py.data(), pinf, q.data(), (int)np);
        res[n + i] = HP::miller_lines(px.data(), py.data(), pinf, tabs.data(), (int)np);
        res[2 * (size_t)n + i] = HP::miller_lines_par(px.data(), py.data(), pinf, tabs.data(), (int)np, [](size_t k, auto fn) { for (size_t t = 0; t < k; t++) fn(t); });
      }
      if (op == OP_MILLER_FE) for (F12 &f : res) f = HP::final_exp(f);
      put(res.data(), res.size() * sizeof(F12));
    }
  }
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: host_pairing_values in.bin out.bin\n"); return 2; }
  FILE *fi = fopen(argv[1], "rb"); if (!fi) { perror(argv[1]); return 2; }
  std::vector<uint32_t> file; uint32_t buf[4096]; size_t k;
  while ((k = fread(buf, 4, 4096, fi)) > 0) file.insert(file.end(), buf, buf + k);
  fclose(fi);
  if (file.empty() || file[0] > 1) fail("bad curve id");
  FILE *fo = fopen(argv[2], "wb"); if (!fo) { perror(argv[2]); return 2; }
  if (file[0] == 0) run<G1Bls12381>(file, fo); else run<G1Bn254>(file, fo);
  if (fclose(fo) != 0) { perror(argv[2]); return 2; }
  printf("host pairing values ok\n");
  return 0;
}
