// The compare that ends share verification (share_verify.hip): a digest against the share's target and the job's
// network target, as 256-bit little-endian values (le256_leq of otedama/sha256.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "otedama/share_job.h"

namespace otedama_dev {

// a <= b for 256-bit values as little-endian words, word 7 most significant: the highest differing word decides.
__device__ __forceinline__ bool leq256(const uint32_t a[8], const uint32_t b[8]) {
  bool r = true;
#pragma unroll
  for (int w = 0; w < 8; ++w) r = a[w] != b[w] ? a[w] < b[w] : r;
  return r;
}

// kVerdictShare | kVerdictNetwork of the digest d0 | d1 against targets[idx] and the job's network target. The
// caller has checked idx against the table: nothing here guards the read.
__device__ __forceinline__ uint32_t share_verdict_bits(const otedama::ShareJobBlock* __restrict__ job,
                                                       const uint4* __restrict__ targets, uint32_t idx, uint4 d0,
                                                       uint4 d1) {
  const uint4 t0 = targets[2 * uint64_t(idx)], t1 = targets[2 * uint64_t(idx) + 1];
  const uint32_t d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
  const uint32_t t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
  uint32_t net[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) net[w] = job->net_target[w];
  return (leq256(d, t) ? otedama::kVerdictShare : 0u) | (leq256(d, net) ? otedama::kVerdictNetwork : 0u);
}

}  // namespace otedama_dev
