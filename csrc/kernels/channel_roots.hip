// channel_roots — "one job, n extranonce prefixes in, n merkle roots out" on gfx950: what a pool needs when a new job
// goes to n Stratum V2 standard channels, each with its own extranonce prefix (layouts: otedama/share_job.h).
//
//   otd_channel_roots  prefixes (16 bytes each, the first en_size used) -> 32-byte merkle roots in header byte order.
//                      One prefix per lane, blocks of 256, a guard for the tail. Per lane: one 16-byte load, the
//                      coinbase SHA-256d from the job's midstate (the tail blocks with the lane's prefix patched in),
//                      the merkle fold over the job's branches, two 16-byte stores at roots + 32 * i.
//
// The coinbase-and-fold body is otd_share_headers' (share_verify.hip), copied and not shared: sharing it was
// measured and cost the latency-bound case 2 us (docs/KERNELS.md, "Channel roots"). The SHA-256 helpers under it are
// shared (sha256_fold_dev.h), with the gfx950 code unchanged. The same rules hold here. Everything that comes from
// the job block is the same for every lane: the template words, the branches, the midstate and the counts are read
// through indices formed from kernel arguments and loop counters only, so they are scalar loads into SGPRs. The loops
// over tail blocks and branches stay rolled (their trip counts are job values); the 64 rounds inside them unroll, so
// no array is indexed with a run-time value and nothing goes to scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cdna_bitops.h"
#include "sha256_fold_dev.h"
#include "otedama/hip_check.h"
#include "otedama/search_launch.h"
#include "otedama/share_job.h"

namespace {
using namespace otedama_dev;
using otedama::ShareJobBlock;

}  // namespace

extern "C" __global__ __launch_bounds__(256) void otd_channel_roots(const ShareJobBlock* __restrict__ job,
                                                                    const uint4* __restrict__ prefixes, uint32_t n,
                                                                    uint4* __restrict__ roots) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 r0 = prefixes[i];

  // Job-uniform values. The counts are clamped to the block's capacity: a block that share_job_prepare did not
  // build must still never be read past its end.
  const uint32_t en_size = job->en_size;
  const uint32_t en_offset = job->en_offset & 63u;
  const uint32_t tail_blocks = umin(job->tail_blocks, uint32_t(otedama::kShareMaxTailBlocks));
  const uint32_t n_branches = umin(job->n_branches, uint32_t(otedama::kShareMaxBranches));

  // The lane's prefix as a big-endian word stream, bytes from en_size on cleared, shifted right by the byte offset
  // of the extranonce inside its first word: P[k] belongs to tail word (en_offset / 4) + k.
  const uint32_t le[4] = {r0.x, r0.y, r0.z, r0.w};
  uint32_t E[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t have = en_size > uint32_t(4 * k) ? en_size - uint32_t(4 * k) : 0u;  // bytes of this word in use
    const uint32_t mask = have >= 4u ? 0xFFFFFFFFu : have == 3u ? 0xFFFFFF00u : have == 2u ? 0xFFFF0000u
                        : have == 1u ? 0xFF000000u : 0u;
    E[k] = __builtin_bswap32(le[k]) & mask;
  }
  const uint32_t sh = 8u * (en_offset & 3u);
  uint32_t P[5];
  P[0] = E[0] >> sh;
#pragma unroll
  for (int k = 1; k < 4; ++k) P[k] = __builtin_amdgcn_alignbit(E[k - 1], E[k], sh);
  P[4] = __builtin_amdgcn_alignbit(E[3], 0u, sh);
  const uint32_t w0 = en_offset >> 2;  // first tail word the extranonce touches

  // coinbase txid
  uint32_t st[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) st[k] = job->midstate[k];
  for (uint32_t b = 0; b < tail_blocks; ++b) {
    uint32_t msg[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) msg[j] = job->tail[16u * b + uint32_t(j)];
    // The template holds zeros where the extranonce goes. Which of the 16 words take which P[k] is a job value, the
    // same in every lane: selected with unrolled uniform compares, never by indexing msg or P at run time.
    if (16u * b + 15u >= w0 && 16u * b <= w0 + 4u) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint32_t d = 16u * b + uint32_t(j) - w0;  // wraps to a large value below w0
        uint32_t add = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) add = d == uint32_t(k) ? P[k] : add;
        msg[j] |= add;
      }
    }
    sha256_compress(st, msg);
  }
  uint32_t cur[8];
  sha256_of_digest(st, cur);

  // merkle fold: cur = sha256d(cur | branch)
  for (uint32_t b = 0; b < n_branches; ++b) {
    uint32_t msg[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      msg[k] = cur[k];
      msg[8 + k] = job->branches[8u * b + uint32_t(k)];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) st[k] = kSha256IVd[k];
    sha256_compress(st, msg);
    sha256_compress_pad64(st);
    sha256_of_digest(st, cur);
  }

  // the root's bytes are the state words big-endian
  uint4* o = roots + uint64_t(i) * 2u;
  o[0] = make_uint4(__builtin_bswap32(cur[0]), __builtin_bswap32(cur[1]), __builtin_bswap32(cur[2]),
                    __builtin_bswap32(cur[3]));
  o[1] = make_uint4(__builtin_bswap32(cur[4]), __builtin_bswap32(cur[5]), __builtin_bswap32(cur[6]),
                    __builtin_bswap32(cur[7]));
}

namespace otedama {

hipError_t launch_channel_roots(const void* job, const uint8_t* prefixes, uint32_t n, uint8_t* roots, hipStream_t s) {
  if (n == 0 || !job || !prefixes || !roots || !aligned16(job, prefixes, roots)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_channel_roots, dim3((n + 255u) / 256u), dim3(256), 0, s,
                     static_cast<const ShareJobBlock*>(job), reinterpret_cast<const uint4*>(prefixes), n,
                     reinterpret_cast<uint4*>(roots));
  return hipGetLastError();
}

}  // namespace otedama
