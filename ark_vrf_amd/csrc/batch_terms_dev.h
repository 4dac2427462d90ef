// batch_terms_dev.h -- what the terms kernels of the batch verifiers share (vrf_batch.hip k_thin_terms / k_ped_terms, thin_shared.hip
// k_thin_terms_shared): a 128-bit little-endian value as a field element, and one MSM term (plain scalar + precomputed base).
#pragma once
#include "proto_dev.h"

namespace avrf {

AVRF_DI fp fp_from_u128(const uint32_t *w) {
  fp a = fp_zero(); uint4 v = *reinterpret_cast<const uint4 *>(w);
  a.v[0] = v.x; a.v[1] = v.y; a.v[2] = v.z; a.v[3] = v.w; return a;
}
template <class S> AVRF_DI void emit_term(uint32_t *scalars, te_pre *pre, uint32_t t, const fp &scalar_plain, const uint8_t *xy) {
  using Fq = typename S::Fq;
  fp_store(scalars + 8 * (size_t)t, scalar_plain);
  fp x = fp_to_mont<Fq>(fp_load_le(xy)), y = fp_to_mont<Fq>(fp_load_le(xy + 32));
  store_pre(pre + t, te_make_pre<S>(x, y));
}

}  // namespace avrf
