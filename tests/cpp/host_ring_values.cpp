// CPU-only run of the ring verifier's host arithmetic (host_ring.h) on cases from a file, every value written to a file:
// tests/test_host_ring_values.py builds the cases from the reference's ring vectors and compares every value with oracle/ring_py.py.
// in  (little-endian): u32 suite, u32 ring_size, u32 n_cases, u32 0; the verifier key as PcsVerifierParams, serialize_uncompressed
//     (g1 | g2 | tau g2); per case: ring commitment (3 compressed G1) | instance x || y (2 x LE32) | proof | r1 (LE32) | r2 (LE32)
// out: per case: i32 status of HostRing::reduce (2 as well when a point does not decode); the proof's seven points, serialize_uncompressed;
//     7 alphas, zeta, 8 nus; the 10 scalars of the first sum, gsc, the 2 scalars of the second -- all canonical LE32, zero unless status 0;
//     then the 32 n_cases bytes of HostRing::batch_randomisers for ONE batch of all cases, case i checked against ring i
// Usage: host_ring_values in.bin out.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ark_vrf_amd/csrc/host_ring.h"

using namespace avrf;

static void fail(const char *m) { fprintf(stderr, "%s\n", m); exit(2); }

template <class S, class G> static void run(const std::vector<uint8_t> &in, uint32_t ring_size, uint32_t n, FILE *fo) {
  using HR = HostRing<S, G>; using Fr = typename HR::Fr; using PL = RingProofLayout<G>; using F = typename S::Fq;
  constexpr size_t FQB = PL::FQB, CASE = PL::COMMITMENT_LEN + 64 + PL::LEN + 64, VK = 2 * FQB + 2 * 4 * FQB;
  if (in.size() != 16 + VK + (size_t)n * CASE) fail("bad input length");
  auto put = [&](const void *p, size_t bytes) { if (fwrite(p, 1, bytes, fo) != bytes) fail("short write"); };
  const uint8_t *vk = in.data() + 16, *cases = vk + VK;
  const G1Aff g1_0 = g1_from_raw<G>(vk);
  const std::vector<uint8_t> g2_raw(vk + 2 * FQB, vk + VK);
  // the domain constants as the setup derives them
  const size_t N = ring_domain_size(ring_size, S::Fr::BITS);
  const H256 w = Fr::sqr(Fr::sqr(HR::domain_root(4 * N))), ninv = Fr::inv_fermat(fr_small<F>(N));
  const typename HR::VerifierConsts vc(N, w, ninv);
  std::vector<uint8_t> commitments, instances, proofs; std::vector<uint32_t> ring_of_item;
  for (uint32_t c = 0; c < n; c++) {
    const uint8_t *com = cases + (size_t)c * CASE, *inst = com + PL::COMMITMENT_LEN, *proof = inst + 64, *rr = proof + PL::LEN;
    commitments.insert(commitments.end(), com, inst); instances.insert(instances.end(), inst, proof); proofs.insert(proofs.end(), proof, rr);
    ring_of_item.push_back(c);
    int32_t status = AVRF_OK;
    G1Aff fixed[3], pts[7];
    for (int i = 0; i < 3; i++) if (!g1_decompress<G>(com + FQB * i, &fixed[i])) status = AVRF_INVALID_DATA;
    for (int j = 0; j < 7; j++) if (!g1_decompress<G>(proof + PL::G1_OFF[j], &pts[j])) status = AVRF_INVALID_DATA;
    typename HR::Item o; memset(&o, 0, sizeof o);
    if (status == AVRF_OK) {
      const H256 r1 = Fr::to_mont(Fr::load_le(rr)), r2 = Fr::to_mont(Fr::load_le(rr + 32));
      status = HR::reduce(vc, HR::prelude(g1_0, g2_raw, fixed), pts, proof, inst, r1, r2, o);
      if (status != AVRF_OK) memset(&o, 0, sizeof o);
    } else memset(pts, 0, sizeof pts);
    put(&status, 4);
    std::vector<uint8_t> enc;
    for (int j = 0; j < 7; j++) g1_encode<G>(pts[j], false, enc);
    put(enc.data(), enc.size());
    uint8_t le[32];
    auto put_mont = [&](const H256 &v) { fr_store_le32<F>(le, v); put(le, 32); };
    for (int i = 0; i < 7; i++) put_mont(o.al[i]);
    put_mont(o.zeta);
    for (int i = 0; i < 8; i++) put_mont(o.nu[i]);
    put(o.s1, sizeof o.s1);
    put_mont(o.gsc);
    put(o.s2, sizeof o.s2);
  }
  const std::vector<uint8_t> rnd = HR::batch_randomisers(n, n, N, g1_0, g2_raw, ring_of_item.data(), commitments.data(), instances.data(), proofs.data());
  put(rnd.data(), rnd.size());
}

int main(int argc, char **argv) {
  if (argc != 3) fail("usage: host_ring_values in.bin out.bin");
  FILE *fi = fopen(argv[1], "rb"); if (!fi) fail("cannot open input");
  std::vector<uint8_t> in; uint8_t buf[65536]; size_t k;
  while ((k = fread(buf, 1, sizeof buf, fi)) > 0) in.insert(in.end(), buf, buf + k);
  fclose(fi);
  if (in.size() < 16) fail("truncated header");
  uint32_t hdr[4]; memcpy(hdr, in.data(), 16);
  if (hdr[1] == 0 || hdr[1] > (1u << 20) || hdr[2] == 0 || hdr[2] > 4096) fail("bad header");
  FILE *fo = fopen(argv[2], "wb"); if (!fo) fail("cannot open output");
  switch (hdr[0]) {
    case 0: run<SuiteBandersnatch, G1Bls12381>(in, hdr[1], hdr[2], fo); break;
    case 1: run<SuiteBabyJubJub, G1Bn254>(in, hdr[1], hdr[2], fo); break;
    case 2: run<SuiteJubJub, G1Bls12381>(in, hdr[1], hdr[2], fo); break;
    case 4: run<SuiteBandersnatchSW, G1Bls12381>(in, hdr[1], hdr[2], fo); break;
    case 5: run<SuiteBandersnatchShake, G1Bls12381>(in, hdr[1], hdr[2], fo); break;
    default: fail("not a ring suite");
  }
  if (fclose(fo) != 0) fail("close failed");
  printf("host ring values ok\n");
  return 0;
}
