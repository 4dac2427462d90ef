// weight_stream.cpp -- stand-alone check of ark_vrf_amd/csrc/host_weight_stream.h (host code only: built with g++ from that header
// alone, once plainly and once with -fsanitize=address,undefined; tests/test_open_batch_host.py).
//
//   weight_stream <prefix hex> [<prefix hex> ...]
//
// For every hash (0 SHA-512, 1 SHAKE128, 2 SHA-256), record size (64, 96), record count (1, 2, 129, 600) and prefix: the records are
// absorbed in every chunking of a fixed list and each must end in what ONE absorb of the whole message ends in; a clone finalised
// after the first half must equal the whole-message value of that half while the original goes on to the right end.  Prints
//   <hash> <record bytes> <records> <prefix bytes> <end value hex> <half value hex>
// per case (SHA-512: the 64-byte digest; the others: 16 or 32 stream bytes per record), which the test compares with hashlib and with
// avrf_batch_weight_seed.  Exit status 1 on the first mismatch.
#include "host_weight_stream.h"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

using avrf::WeightStream;

// record j: LE32(c) with a 16-byte c, then the responses -- bytes of a fixed formula the test restates
static void make_records(std::vector<uint8_t> &out, size_t n, size_t recsz) {
  out.assign(n * recsz, 0);
  for (size_t j = 0; j < n; j++)
    for (size_t i = 0; i < recsz; i++)
      if (i < 16 || i >= 32) out[j * recsz + i] = (uint8_t)(((uint32_t)j * 2654435761u + (uint32_t)i * 40503u + 12345u) >> 7);
}
static std::vector<uint8_t> value_of(const WeightStream &w, size_t n, size_t recsz) {
  std::vector<uint8_t> v(w.hash == WeightStream::SHA512 ? 64 : n * (recsz == 64 ? 16 : 32));
  if (w.hash == WeightStream::SHA512) w.digest(v.data()); else w.squeeze(v.data(), v.size());
  return v;
}
static std::vector<uint8_t> whole(WeightStream::Hash h, const std::vector<uint8_t> &prefix, const uint8_t *rec, size_t n, size_t recsz) {
  WeightStream w; w.begin(h, prefix.data(), prefix.size());
  w.absorb(rec, n, recsz);
  return value_of(w, n, recsz);
}
static void print_hex(const std::vector<uint8_t> &v) { if (v.empty()) printf("-"); for (uint8_t b : v) printf("%02x", b); }

int main(int argc, char **argv) {
  std::vector<std::vector<uint8_t>> prefixes;
  for (int a = 1; a < argc; a++) {
    const std::string s = argv[a]; std::vector<uint8_t> p;
    for (size_t i = 0; i + 1 < s.size(); i += 2) p.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    prefixes.push_back(p);
  }
  // chunkings: the sizes are taken in turn (the last one repeats) until the records run out
  const std::vector<std::vector<size_t>> chunkings = {{1}, {600}, {1, 127, 128, 129, 215}, {2, 3, 5, 7, 11, 13}, {64}, {300, 1, 299}};
  const size_t counts[4] = {1, 2, 129, 600}, recszs[2] = {64, 96};
  for (int h = 0; h < 3; h++) for (size_t recsz : recszs) for (size_t n : counts) for (const auto &prefix : prefixes) {
    const WeightStream::Hash hash = (WeightStream::Hash)h;
    std::vector<uint8_t> rec; make_records(rec, n, recsz);
    const size_t half = n / 2;
    const std::vector<uint8_t> end = whole(hash, prefix, rec.data(), n, recsz), mid = whole(hash, prefix, rec.data(), half, recsz);
    for (size_t q = 0; q < chunkings.size(); q++) {
      WeightStream w; w.begin(hash, prefix.data(), prefix.size());
      size_t at = 0, k = 0; bool cloned = false;
      auto clone_check = [&]() {
        // a clone finalised mid-way (twice: finalising must not disturb the clone's source either) leaves the original as it was
        const WeightStream c = w.clone();
        if (value_of(c, half, recsz) != mid || value_of(w, half, recsz) != mid) { fprintf(stderr, "clone mismatch: hash %d rec %zu n %zu chunking %zu\n", h, recsz, n, q); exit(1); }
        cloned = true;
      };
      while (at < n) {
        size_t take = chunkings[q][k < chunkings[q].size() ? k : chunkings[q].size() - 1]; k++;
        if (take > n - at) take = n - at;
        if (!cloned && at + take > half) {                                  // stop at the half first
          const size_t first = half - at;
          w.absorb(rec.data() + at * recsz, first, recsz); at += first; take -= first;
          clone_check();
        }
        w.absorb(rec.data() + at * recsz, take, recsz); at += take;
      }
      if (!cloned) clone_check();
      if (w.items != n || value_of(w, n, recsz) != end) { fprintf(stderr, "chunking mismatch: hash %d rec %zu n %zu chunking %zu\n", h, recsz, n, q); return 1; }
    }
    // the records given as their parts (16-byte challenges, responses) build the same message
    {
      std::vector<uint8_t> c16(16 * n), resp((recsz - 32) * n);
      for (size_t j = 0; j < n; j++) { memcpy(&c16[16 * j], &rec[j * recsz], 16); memcpy(&resp[(recsz - 32) * j], &rec[j * recsz + 32], recsz - 32); }
      WeightStream w; w.begin(hash, prefix.data(), prefix.size());
      w.absorb_parts(c16.data(), resp.data(), n, recsz - 32);
      if (value_of(w, n, recsz) != end) { fprintf(stderr, "parts mismatch: hash %d rec %zu n %zu\n", h, recsz, n); return 1; }
    }
    printf("%d %zu %zu %zu ", h, recsz, n, prefix.size()); print_hex(end); printf(" "); print_hex(mid); printf("\n");
  }
  return 0;
}
