// share_results — live share verification on gfx950: one packed 128-byte ShareResult per share (layouts:
// otedama/share_job.h), so a pool's micro-batch is one buffer in and one buffer out.
//
//   otd_share_pack  after otd_share_headers (share_verify.hip) and the digest launches of the algorithm
//                   (digest_batch.hip): headers + digests -> result records. One share per lane, blocks of 256, a
//                   guard for the tail. Per lane: the two 256-bit compares of otd_share_verdict, then the record as
//                   eight 16-byte stores (header 5, hash 2, verdict and zeros 1). Every algorithm goes through it.
//
// A single-launch SHA-256d kernel (header build, SHA-256d and compares in registers, no headers or digests in
// memory) was built and measured against this chain and did not earn its place: docs/KERNELS.md, "Live share
// verification". It is not in the tree.
//
// The kernel lives in a file of its own: a kernel's neighbours in a file have changed its register allocation
// before (docs/KERNELS.md), and share_verify.hip stays byte for byte what it was. Job-block reads are indexed by
// kernel arguments only (scalar loads); no scratch, no LDS.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "otedama/search_launch.h"
#include "otedama/share_job.h"

namespace {
using otedama::ShareJobBlock;

static_assert(sizeof(otedama::ShareResult) == 8 * sizeof(uint4), "a result record is eight 16-byte stores");

// a <= b for 256-bit values as little-endian words, word 7 most significant: the highest differing word decides.
__device__ __forceinline__ bool leq256(const uint32_t a[8], const uint32_t b[8]) {
  bool r = true;
#pragma unroll
  for (int w = 0; w < 8; ++w) r = a[w] != b[w] ? a[w] < b[w] : r;
  return r;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void otd_share_pack(const ShareJobBlock* __restrict__ job,
                                                                 const uint4* __restrict__ recs,
                                                                 const uint4* __restrict__ headers,
                                                                 const uint4* __restrict__ digests,
                                                                 const uint4* __restrict__ targets,
                                                                 uint32_t n_targets, uint32_t n,
                                                                 uint4* __restrict__ results) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = recs[2 * uint64_t(i) + 1].w;
  const uint4* h = headers + uint64_t(i) * 5u;
  const uint4 h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4];
  const uint4 d0 = digests[2 * uint64_t(i)], d1 = digests[2 * uint64_t(i) + 1];
  uint32_t verdict = otedama::kVerdictBadIndex;
  if (idx < n_targets) {  // the guard: no read of the table for an index outside it
    const uint4 t0 = targets[2 * uint64_t(idx)], t1 = targets[2 * uint64_t(idx) + 1];
    const uint32_t d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
    const uint32_t t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    uint32_t net[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) net[w] = job->net_target[w];
    verdict = (leq256(d, t) ? otedama::kVerdictShare : 0u) | (leq256(d, net) ? otedama::kVerdictNetwork : 0u);
  }
  uint4* o = results + uint64_t(i) * 8u;
  o[0] = h0;
  o[1] = h1;
  o[2] = h2;
  o[3] = h3;
  o[4] = h4;
  o[5] = d0;
  o[6] = d1;
  o[7] = make_uint4(verdict, 0u, 0u, 0u);
}

namespace otedama {

static bool aligned16(uintptr_t a) { return (a & 15u) == 0; }

hipError_t launch_share_pack(const void* job, const uint8_t* records, const uint8_t* headers, const uint8_t* digests,
                             const uint8_t* targets, uint32_t n_targets, uint32_t n, uint8_t* results,
                             hipStream_t s) {
  if (n == 0 || n_targets == 0 || !job || !records || !headers || !digests || !targets || !results)
    return hipErrorInvalidValue;
  if (!aligned16(reinterpret_cast<uintptr_t>(job) | reinterpret_cast<uintptr_t>(records) |
                 reinterpret_cast<uintptr_t>(headers) | reinterpret_cast<uintptr_t>(digests) |
                 reinterpret_cast<uintptr_t>(targets) | reinterpret_cast<uintptr_t>(results)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_share_pack, dim3((n + 255u) / 256u), dim3(256), 0, s,
                     static_cast<const ShareJobBlock*>(job), reinterpret_cast<const uint4*>(records),
                     reinterpret_cast<const uint4*>(headers), reinterpret_cast<const uint4*>(digests),
                     reinterpret_cast<const uint4*>(targets), n_targets, n, reinterpret_cast<uint4*>(results));
  return hipGetLastError();
}

void py_launch_share_pack(uintptr_t job, uintptr_t records, uintptr_t headers, uintptr_t digests, uintptr_t targets,
                          uint32_t n_targets, uint32_t n, uintptr_t results, uintptr_t stream) {
  const hipError_t e =
      launch_share_pack(reinterpret_cast<const void*>(job), reinterpret_cast<const uint8_t*>(records),
                        reinterpret_cast<const uint8_t*>(headers), reinterpret_cast<const uint8_t*>(digests),
                        reinterpret_cast<const uint8_t*>(targets), n_targets, n, reinterpret_cast<uint8_t*>(results),
                        reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess)
    throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e) + " at launch_share_pack");
}

}  // namespace otedama
