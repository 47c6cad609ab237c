// share_verify — the front and the back of "verify these pool shares" on gfx950 (layouts: otedama/share_job.h).
//
//   otd_share_headers  share records -> 80-byte headers. One share per lane, blocks of 256, a guard for the tail.
//                      Per lane: the coinbase SHA-256d from the job's midstate (the tail blocks with the lane's
//                      extranonce patched in), the merkle fold over the job's branches, the header packed as five
//                      16-byte stores at headers + 80 * i, the layout the digest ops read (digest_batch.hip).
//   otd_share_verdict  digests -> one verdict byte per share: the 256-bit little-endian compare (byte 31 most
//                      significant, le256_leq of otedama/sha256.h) against the share's target and the job's network
//                      target.
//   otd_share_pack     the live path's last step instead of otd_share_verdict: headers + digests -> one packed
//                      128-byte ShareResult per share, so a pool's micro-batch is one buffer in and one buffer out.
//                      Per lane: the same two compares (share_compare_dev.h), then the record as eight 16-byte
//                      stores (header 5, hash 2, verdict and zeros 1). Every algorithm goes through it. A
//                      single-launch SHA-256d kernel (header build, SHA-256d and compares in registers) was built and
//                      measured against this chain and did not earn its place: docs/KERNELS.md, "Live share
//                      verification". It is not in the tree.
//
// Everything that comes from the job block is the same for every lane: the template words, the branches, the
// midstate and the counts are read through indices formed from kernel arguments and loop counters only, so they are
// scalar loads into SGPRs. The loops over tail blocks and branches stay rolled (their trip counts are job values);
// the 64 rounds inside them unroll, so no array is indexed with a run-time value and nothing goes to scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cdna_bitops.h"
#include "sha256_fold_dev.h"
#include "share_compare_dev.h"
#include "otedama/hip_check.h"
#include "otedama/search_launch.h"
#include "otedama/share_job.h"

namespace {
using namespace otedama_dev;
using otedama::ShareJobBlock;

}  // namespace

extern "C" __global__ __launch_bounds__(256) void otd_share_headers(const ShareJobBlock* __restrict__ job,
                                                                    const uint4* __restrict__ recs, uint32_t n,
                                                                    uint4* __restrict__ headers) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 r0 = recs[2 * uint64_t(i)], r1 = recs[2 * uint64_t(i) + 1];

  // Job-uniform values. The counts are clamped to the block's capacity: a block that share_job_prepare did not
  // build must still never be read past its end.
  const uint32_t en_size = job->en_size;
  const uint32_t en_offset = job->en_offset & 63u;
  const uint32_t tail_blocks = umin(job->tail_blocks, uint32_t(otedama::kShareMaxTailBlocks));
  const uint32_t n_branches = umin(job->n_branches, uint32_t(otedama::kShareMaxBranches));

  // The lane's extranonce as a big-endian word stream, bytes from en_size on cleared, shifted right by the byte
  // offset of the extranonce inside its first word: P[k] belongs to tail word (en_offset / 4) + k.
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

  // version | prev_hash | root | ntime | nbits | nonce, as little-endian words; the root's bytes are the state
  // words big-endian
  uint32_t root[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) root[k] = __builtin_bswap32(cur[k]);
  uint4* h = headers + uint64_t(i) * 5u;
  h[0] = make_uint4(r1.z, job->prev_hash[0], job->prev_hash[1], job->prev_hash[2]);
  h[1] = make_uint4(job->prev_hash[3], job->prev_hash[4], job->prev_hash[5], job->prev_hash[6]);
  h[2] = make_uint4(job->prev_hash[7], root[0], root[1], root[2]);
  h[3] = make_uint4(root[3], root[4], root[5], root[6]);
  h[4] = make_uint4(root[7], r1.x, job->nbits, r1.y);
}

extern "C" __global__ __launch_bounds__(256) void otd_share_verdict(const ShareJobBlock* __restrict__ job,
                                                                    const uint4* __restrict__ recs,
                                                                    const uint4* __restrict__ digests,
                                                                    const uint4* __restrict__ targets,
                                                                    uint32_t n_targets, uint32_t n,
                                                                    uint8_t* __restrict__ verdicts) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t idx = recs[2 * uint64_t(i) + 1].w;
  if (idx >= n_targets) {  // the guard: no read of the table for an index outside it
    verdicts[i] = otedama::kVerdictBadIndex;
    return;
  }
  const uint4 d0 = digests[2 * uint64_t(i)], d1 = digests[2 * uint64_t(i) + 1];
  verdicts[i] = uint8_t(share_verdict_bits(job, targets, idx, d0, d1));
}

static_assert(sizeof(otedama::ShareResult) == 8 * sizeof(uint4), "a result record is eight 16-byte stores");

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
  if (idx < n_targets) verdict = share_verdict_bits(job, targets, idx, d0, d1);  // the guard, as above
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

hipError_t launch_share_headers(const void* job, const uint8_t* records, uint32_t n, uint8_t* headers, hipStream_t s) {
  if (n == 0 || !job || !records || !headers || !aligned16(job, records, headers)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_share_headers, dim3((n + 255u) / 256u), dim3(256), 0, s,
                     static_cast<const ShareJobBlock*>(job), reinterpret_cast<const uint4*>(records), n,
                     reinterpret_cast<uint4*>(headers));
  return hipGetLastError();
}

hipError_t launch_share_verdict(const void* job, const uint8_t* records, const uint8_t* digests, const uint8_t* targets,
                                uint32_t n_targets, uint32_t n, uint8_t* verdicts, hipStream_t s) {
  if (n == 0 || n_targets == 0 || !job || !records || !digests || !targets || !verdicts) return hipErrorInvalidValue;
  if (!aligned16(job, records, digests, targets)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_share_verdict, dim3((n + 255u) / 256u), dim3(256), 0, s,
                     static_cast<const ShareJobBlock*>(job), reinterpret_cast<const uint4*>(records),
                     reinterpret_cast<const uint4*>(digests), reinterpret_cast<const uint4*>(targets), n_targets, n,
                     verdicts);
  return hipGetLastError();
}

hipError_t launch_share_pack(const void* job, const uint8_t* records, const uint8_t* headers, const uint8_t* digests,
                             const uint8_t* targets, uint32_t n_targets, uint32_t n, uint8_t* results,
                             hipStream_t s) {
  if (n == 0 || n_targets == 0 || !job || !records || !headers || !digests || !targets || !results)
    return hipErrorInvalidValue;
  if (!aligned16(job, records, headers, digests, targets, results)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(otd_share_pack, dim3((n + 255u) / 256u), dim3(256), 0, s,
                     static_cast<const ShareJobBlock*>(job), reinterpret_cast<const uint4*>(records),
                     reinterpret_cast<const uint4*>(headers), reinterpret_cast<const uint4*>(digests),
                     reinterpret_cast<const uint4*>(targets), n_targets, n, reinterpret_cast<uint4*>(results));
  return hipGetLastError();
}

}  // namespace otedama
