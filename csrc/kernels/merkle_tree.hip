// merkle_tree — "t trees of n leaves in, each tree's root and its coinbase path out" on gfx950: what a pool needs when
// a block template arrives (the txid tree for the coinbase branches, the wtxid tree for the witness commitment).
//
//   otd_merkle_tree  nodes (32 bytes each, internal byte order) -> rows of 32 bytes: row 0 the root, row 1 + l node 1
//                    of level l (the sibling of the leftmost path). Levels fold pairwise with SHA-256d; an odd level
//                    pairs its last node with itself.
//
// One workgroup of 256 lanes folds one chunk of up to 512 nodes; blockIdx.y is the tree. Level 0 is hashed straight
// from global memory (lane i loads nodes 2i and 2i + 1, 64 contiguous bytes), the later levels from LDS, ping-pong
// between two buffers with one barrier per level. Lane 0 computes node 0 of every level, so it ends with the chunk's
// root in registers; chunk 0 stores node 1 of every level, the right half of lane 0's message, as a path row.
//
// A tree of more than 512 leaves takes two launches. In the first every chunk folds exactly nine levels, the last
// chunk too, however few nodes it holds (a chunk of one node is hashed nine times with itself): ceil(n / 2^l) and the
// last chunk's ceil(m / 2^l) have the same parity for l < 9, so the tree's duplicate-last rule is the chunk's own. Each
// chunk root goes to a scratch row. The second launch is the same kernel over the at most 512 chunk roots, its path
// rows offset by nine levels; it folds until one node is left, as the single launch of a small tree does.
//
// The SHA-256 helpers are the ones channel_roots.hip and share_verify.hip use (sha256_fold_dev.h; docs/KERNELS.md,
// "Template tree"). Every round loop unrolls, no array is indexed with a run-time value and nothing goes to scratch
// memory; the level loop stays rolled (its trip count is a launch value).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cdna_bitops.h"
#include "sha256_fold_dev.h"
#include "otedama/hip_check.h"
#include "otedama/search_launch.h"

namespace {
using namespace otedama_dev;

constexpr uint32_t kChunk = 512;       // nodes per workgroup
constexpr uint32_t kChunkLevels = 9;   // log2(kChunk)

__device__ __forceinline__ uint4 bswap4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return make_uint4(__builtin_bswap32(a), __builtin_bswap32(b), __builtin_bswap32(c), __builtin_bswap32(d));
}

}  // namespace

// in: t trees of n nodes, tree y at in + 2 * n * y (uint4 units). levels: how many levels this launch folds (at most
// nine). final = 0: every chunk folds `levels` levels and stores its root at scratch + 2 * (chunks * y + chunk).
// final != 0: one chunk per tree (n <= 512), 2^levels >= n, and the root goes to row 0 of the tree's out_rows rows at
// out. Chunk 0 stores node 1 of its level l at row 1 + level_base + l, where that row exists.
extern "C" __global__ __launch_bounds__(256) void otd_merkle_tree(const uint4* __restrict__ in, uint32_t n,
                                                                  uint32_t levels, uint32_t level_base, uint32_t final,
                                                                  uint4* __restrict__ scratch, uint4* __restrict__ out,
                                                                  uint32_t out_rows) {
  __shared__ uint4 nodes[2][2 * (kChunk / 2)];  // level l's nodes (big-endian state words) in nodes[l & 1]

  const uint32_t lane = threadIdx.x;
  const uint32_t chunk = blockIdx.x, tree = blockIdx.y;
  const uint32_t chunks = (n + kChunk - 1) / kChunk;
  if (chunk >= chunks || (final && chunk != 0)) return;   // the whole workgroup: no barrier is left waiting
  const uint32_t m = umin(kChunk, n - chunk * kChunk);    // this chunk's nodes, 1..512
  levels = umin(levels, kChunkLevels);                    // 2^levels nodes at most fit the LDS buffers

  const uint4* src = in + (uint64_t(tree) * n + uint64_t(chunk) * kChunk) * 2u;
  uint4* rows = out + uint64_t(tree) * out_rows * 2u;

  if (levels == 0) {  // a tree of one leaf: the leaf is the root, and there is no path
    if (final && lane == 0 && out_rows >= 1) {
      rows[0] = src[0];
      rows[1] = src[1];
    }
    return;
  }

  uint32_t cur[8] = {};
  for (uint32_t l = 0; l < levels; ++l) {
    const uint32_t c = (m + (1u << l) - 1u) >> l;  // nodes of this level in this chunk: ceil(m / 2^l) >= 1
    if (2u * lane < c) {                           // lane i makes node i of the next level from nodes 2i and 2i + 1
      const bool pair = 2u * lane + 1u < c;        // else the last node of an odd level: paired with itself
      uint32_t msg[16];
      if (l == 0) {
        const uint4* p = src + 4u * lane;
        const uint4 a0 = p[0], a1 = p[1];
        const uint4 b0 = pair ? p[2] : a0, b1 = pair ? p[3] : a1;  // nothing at or after node m is read
        const uint32_t le[16] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w,
                                 b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) msg[k] = __builtin_bswap32(le[k]);
      } else {
        const uint4* p = &nodes[(l - 1u) & 1u][4u * lane];
        const uint4 a0 = p[0], a1 = p[1];
        const uint4 b0 = pair ? p[2] : a0, b1 = pair ? p[3] : a1;
        const uint32_t be[16] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w,
                                 b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) msg[k] = be[k];
      }
      // the path row of this level: node 1, the right half of lane 0's message
      const uint32_t row = 1u + level_base + l;
      if (chunk == 0 && lane == 0 && row < out_rows) {
        rows[2u * row] = bswap4(msg[8], msg[9], msg[10], msg[11]);
        rows[2u * row + 1u] = bswap4(msg[12], msg[13], msg[14], msg[15]);
      }
      uint32_t st[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) st[k] = kSha256IVd[k];
      sha256_compress(st, msg);
      sha256_compress_pad64(st);
      sha256_of_digest(st, cur);
      if (l + 1u < levels) {
        uint4* q = &nodes[l & 1u][2u * lane];
        q[0] = make_uint4(cur[0], cur[1], cur[2], cur[3]);
        q[1] = make_uint4(cur[4], cur[5], cur[6], cur[7]);
      }
    }
    if (l + 1u < levels) __syncthreads();  // uniform: levels is a kernel argument
  }

  // lane 0 made node 0 of every level: it holds the chunk's root
  if (lane == 0) {
    uint4* o = final ? rows : scratch + (uint64_t(tree) * chunks + chunk) * 2u;
    if (!final || out_rows >= 1) {
      o[0] = bswap4(cur[0], cur[1], cur[2], cur[3]);
      o[1] = bswap4(cur[4], cur[5], cur[6], cur[7]);
    }
  }
}

namespace otedama {

hipError_t launch_merkle_tree(const uint8_t* leaves, uint32_t t, uint32_t n, uint8_t* scratch, uint8_t* out,
                              hipStream_t s) {
  if (t == 0 || t > kMerkleTreeMaxTrees || n == 0 || n > kMerkleTreeMaxLeaves || !leaves || !out ||
      !aligned16(leaves, out))
    return hipErrorInvalidValue;
  const uint32_t depth = merkle_tree_depth(n);
  const uint4* in = reinterpret_cast<const uint4*>(leaves);
  uint4* rows = reinterpret_cast<uint4*>(out);
  if (n <= kChunk) {
    hipLaunchKernelGGL(otd_merkle_tree, dim3(1, t), dim3(256), 0, s, in, n, depth, 0u, 1u,
                       static_cast<uint4*>(nullptr), rows, 1u + depth);
    return hipGetLastError();
  }
  if (!scratch || !aligned16(scratch)) return hipErrorInvalidValue;
  const uint32_t chunks = (n + kChunk - 1) / kChunk;  // 2..512
  uint4* roots = reinterpret_cast<uint4*>(scratch);
  hipLaunchKernelGGL(otd_merkle_tree, dim3(chunks, t), dim3(256), 0, s, in, n, kChunkLevels, 0u, 0u, roots, rows,
                     1u + depth);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(otd_merkle_tree, dim3(1, t), dim3(256), 0, s, static_cast<const uint4*>(roots), chunks,
                     depth - kChunkLevels, kChunkLevels, 1u, static_cast<uint4*>(nullptr), rows, 1u + depth);
  return hipGetLastError();
}

}  // namespace otedama
