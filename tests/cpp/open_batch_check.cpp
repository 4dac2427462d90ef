// open_batch_check.cpp -- thin::OpenBatchVerifier and pedersen::OpenBatchVerifier of include/avrf.hpp (BatchVerifier::new / push /
// verify as the reference has them, src/thin.rs:188-326, src/pedersen.rs:303-426) on items read from a file, one per line:
//   thin <pk xy> <input xy> <output xy> <ad hex or -> <proof: R xy || s>
//   ped  <input xy> <output xy> <ad hex or -> <proof: Yb xy || R xy || Ok xy || s || sb>
// Usage: open_batch_check <suite> <items file>.  Prints key=value lines (tests/test_gpu_open_batch_cpp.py).
#include "avrf.hpp"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

using namespace avrf;

static std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}
template <size_t N> static std::array<uint8_t, N> arr(const std::vector<uint8_t> &v, size_t at = 0) {
  std::array<uint8_t, N> a{};
  std::copy(v.begin() + at, v.begin() + at + N, a.begin());
  return a;
}
static std::string join(const std::vector<Status> &st) {
  std::string s;
  for (Status v : st) s += std::to_string(v);
  return s;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  Suite su((Suite::Id)atoi(argv[1]));
  std::vector<thin::OpenBatchVerifier::Item> th;
  std::vector<pedersen::OpenBatchVerifier::Item> pe;
  std::ifstream f(argv[2]);
  for (std::string line; std::getline(f, line);) {
    std::istringstream ls(line);
    std::string kind, a, b, c, d, e;
    ls >> kind;
    if (kind == "thin") {
      ls >> a >> b >> c >> d >> e;
      const std::vector<uint8_t> ad = unhex(d), pr = unhex(e);
      th.push_back({Public{arr<64>(unhex(a))}, {VrfIo{arr<64>(unhex(b)), arr<64>(unhex(c))}}, std::string(ad.begin(), ad.end()), thin::Proof{arr<64>(pr), arr<32>(pr, 64)}});
    } else if (kind == "ped") {
      ls >> a >> b >> c >> d;
      const std::vector<uint8_t> ad = unhex(c), pr = unhex(d);
      pe.push_back({{VrfIo{arr<64>(unhex(a)), arr<64>(unhex(b))}}, std::string(ad.begin(), ad.end()),
                    pedersen::Proof{arr<64>(pr), arr<64>(pr, 64), arr<64>(pr, 128), arr<32>(pr, 192), arr<32>(pr, 224)}});
    }
  }
  const uint32_t n = (uint32_t)th.size(), head = n / 2;
  {
    thin::OpenBatchVerifier v(su);
    printf("thin_empty=%d\n", v.verify());
    for (const auto &it : th) v.push(it.pk, it.ios, it.ad, it.proof);                        // one by one
    printf("thin_one_by_one=%d\nthin_len=%zu\n", v.verify(), v.len());
    printf("thin_segments=%s\n", join(v.verify_segments({head, n - head})).c_str());
    auto bad = th[1]; bad.proof.s[3] ^= 1;
    v.push(bad.pk, bad.ios, bad.ad, bad.proof);                                            // verify borrowed: push more, verify again
    printf("thin_after_bad=%d\nthin_segments_bad=%s\nthin_len_bad=%zu\n", v.verify(), join(v.verify_segments({n, 1})).c_str(), v.len());
  }
  {
    thin::OpenBatchVerifier v(su, n, n, 64);
    v.push_many(th);                                                                       // one chunk
    printf("thin_many=%d\n", v.verify());
    thin::BatchVerifier whole(su);                                                         // staging on the Suite ends the open batch
    for (const auto &it : th) whole.push(it.pk, it.ios, it.ad, it.proof);
    const Status staged = whole.verify();
    printf("thin_staged=%d\nthin_len_closed=%zu\n", staged, v.len());
    bool threw = false;
    try { v.push_many(th); } catch (const std::invalid_argument &) { threw = true; }
    printf("thin_push_closed_throws=%d\n", (int)threw);
  }
  {
    pedersen::OpenBatchVerifier v(su);
    for (const auto &it : pe) v.push(it.ios, it.ad, it.proof);
    printf("ped_one_by_one=%d\nped_len=%zu\n", v.verify(), v.len());
    printf("ped_segments=%s\n", join(v.verify_segments({head, n - head})).c_str());
    auto bad = pe[2]; bad.proof.sb[0] ^= 1;
    v.push_many({bad, pe[0]});
    printf("ped_after_bad=%d\nped_segments_bad=%s\n", v.verify(), join(v.verify_segments({n, 1, 1})).c_str());
  }
  {
    pedersen::OpenBatchVerifier v(su, n, n, 64);
    v.push_many(pe);
    printf("ped_many=%d\n", v.verify());
  }
  return 0;
}
