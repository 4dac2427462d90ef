// CPU-only run of HostRing::segment_randomisers (host_ring.h) -- the randomisers every segment of avrf_ring_batch_verify_segments
// derives for its own items -- on items from a file: tests/test_ring_segments_host.py builds the items from the reference's ring vectors
// and compares the bytes with hashlib.shake_128 over every segment's own statement.
// in  (little-endian): u32 suite, u32 ring_size, u32 n_items, u32 n_seg; the verifier key as PcsVerifierParams, serialize_uncompressed
//     (g1 | g2 | tau g2); n_seg x u32 items per segment; per item: ring commitment (3 compressed G1) | instance x || y | proof
//     (item i is checked against ring i)
// out: 32 n_items bytes: segment after segment, HostRing::segment_randomisers of its items; then the 32 n_items bytes of
//     HostRing::batch_randomisers for ONE batch of all items
// Usage: host_ring_segments in.bin out.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ark_vrf_amd/csrc/host_ring.h"

using namespace avrf;

static void fail(const char *m) { fprintf(stderr, "%s\n", m); exit(2); }

template <class S, class G> static void run(const std::vector<uint8_t> &in, uint32_t ring_size, uint32_t n, uint32_t n_seg, FILE *fo) {
  using HR = HostRing<S, G>; using PL = RingProofLayout<G>;
  constexpr size_t FQB = PL::FQB, ITEM = PL::COMMITMENT_LEN + 64 + PL::LEN, VK = 2 * FQB + 2 * 4 * FQB;
  if (in.size() != 16 + VK + 4 * (size_t)n_seg + (size_t)n * ITEM) fail("bad input length");
  const uint8_t *vk = in.data() + 16, *segs = vk + VK, *items = segs + 4 * (size_t)n_seg;
  const G1Aff g1_0 = g1_from_raw<G>(vk);
  const std::vector<uint8_t> g2_raw(vk + 2 * FQB, vk + VK);
  const size_t N = ring_domain_size(ring_size, S::Fr::BITS);
  std::vector<uint8_t> commitments, instances, proofs; std::vector<uint32_t> ring_of_item;
  for (uint32_t c = 0; c < n; c++) {
    const uint8_t *com = items + (size_t)c * ITEM, *inst = com + PL::COMMITMENT_LEN, *proof = inst + 64;
    commitments.insert(commitments.end(), com, inst); instances.insert(instances.end(), inst, proof); proofs.insert(proofs.end(), proof, proof + PL::LEN);
    ring_of_item.push_back(c);
  }
  std::vector<uint8_t> rnd(32 * (size_t)n);
  size_t first = 0;
  for (uint32_t v = 0; v < n_seg; v++) {
    uint32_t cnt; memcpy(&cnt, segs + 4 * (size_t)v, 4);
    if (first + cnt > n) fail("segments beyond the items");
    HR::segment_randomisers(first, cnt, n, N, g1_0, g2_raw, ring_of_item.data(), commitments.data(), instances.data(), proofs.data(), rnd.data() + 32 * first);
    first += cnt;
  }
  if (first != n) fail("segments do not cover the items");
  if (fwrite(rnd.data(), 1, rnd.size(), fo) != rnd.size()) fail("short write");
  const std::vector<uint8_t> all = HR::batch_randomisers(n, n, N, g1_0, g2_raw, ring_of_item.data(), commitments.data(), instances.data(), proofs.data());
  if (fwrite(all.data(), 1, all.size(), fo) != all.size()) fail("short write");
}

int main(int argc, char **argv) {
  if (argc != 3) fail("usage: host_ring_segments in.bin out.bin");
  FILE *fi = fopen(argv[1], "rb"); if (!fi) fail("cannot open input");
  std::vector<uint8_t> in; uint8_t buf[65536]; size_t k;
  while ((k = fread(buf, 1, sizeof buf, fi)) > 0) in.insert(in.end(), buf, buf + k);
  fclose(fi);
  if (in.size() < 16) fail("truncated header");
  uint32_t hdr[4]; memcpy(hdr, in.data(), 16);
  if (hdr[1] == 0 || hdr[1] > (1u << 20) || hdr[2] == 0 || hdr[2] > 4096 || hdr[3] == 0 || hdr[3] > 4096) fail("bad header");
  FILE *fo = fopen(argv[2], "wb"); if (!fo) fail("cannot open output");
  switch (hdr[0]) {
    case 0: run<SuiteBandersnatch, G1Bls12381>(in, hdr[1], hdr[2], hdr[3], fo); break;
    case 1: run<SuiteBabyJubJub, G1Bn254>(in, hdr[1], hdr[2], hdr[3], fo); break;
    default: fail("not a ring suite of this test");
  }
  if (fclose(fo) != 0) fail("close failed");
  printf("host ring segments ok\n");
  return 0;
}
