// host_weight_stream.h -- the batch verifiers' weight transcript (src/thin.rs:274-279, src/pedersen.rs:361-367) as a RUNNING hash:
// begin(prefix), absorb records as they become known, and at any moment clone the state and finalise the clone -- the digest that
// seeds the counter-mode weights (SHA-512 suites), or the first bytes of the weight stream itself (the SHAKE128 sponge, SHA-256's
// counter-mode squeeze).  The original goes on absorbing: BatchVerifier::verify(&self) borrows, so a batch can be verified, pushed
// to and verified again (include/avrf.h, open batches).  One record per item: LE32(c) || LE32(s) [|| LE32(sb)], 64 or 96 bytes.
// Host code over host_sha512.h / host_shake128.h / host_sha256.h alone: no HIP, no pool; any C++17 compiler takes it by itself.
#pragma once
#include "host_sha256.h"
#include "host_sha512.h"
#include "host_shake128.h"

namespace avrf {

struct WeightStream {
  enum Hash { SHA512 = 0, SHAKE128 = 1, SHA256 = 2 };
  Hash hash = SHA512; uint64_t items = 0;
  HostSha512 h512; HostShake128 shake; HostSha256 h256;    // (only `hash`'s is used; all three are plain values, so a copy IS a clone)

  void begin(Hash which, const uint8_t *prefix, size_t prefix_len) {
    *this = WeightStream(); hash = which;
    update(prefix, prefix_len);
  }
  // n whole records of rec_bytes each, contiguous
  void absorb(const uint8_t *records, size_t n, size_t rec_bytes) { update(records, n * rec_bytes); items += n; }
  // the same records given as their parts: 16-byte challenges (the upper 16 bytes of LE32(c) are zero) and resp_bytes of responses per item
  void absorb_parts(const uint8_t *c16, const uint8_t *resp, size_t n, size_t resp_bytes) {
    uint8_t rec[32 + 64]; memset(rec, 0, sizeof rec);
    for (size_t k = 0; k < n; k++) { memcpy(rec, c16 + 16 * k, 16); memcpy(rec + 32, resp + resp_bytes * k, resp_bytes); update(rec, 32 + resp_bytes); }
    items += n;
  }
  WeightStream clone() const { return *this; }
  // SHA512: the 64-byte digest of everything absorbed (finalises a clone: this stream continues)
  void digest(uint8_t out[64]) const { HostSha512 c = h512; c.final(out); }
  // SHAKE128 / SHA256: the first n bytes of the output stream of everything absorbed (of a clone, likewise)
  void squeeze(uint8_t *out, size_t n) const { if (hash == SHAKE128) shake.squeeze_copy(out, n); else h256.squeeze_copy(out, n); }

 private:
  void update(const uint8_t *p, size_t n) {
    if (hash == SHA512) h512.update(p, n); else if (hash == SHAKE128) shake.update(p, n); else h256.update(p, n);
  }
};

}  // namespace avrf
