// Native CPU twin of otd_merkle_tree (csrc/kernels/merkle_tree.hip): the same rows (otedama/merkle_tree.h), level by
// level over the whole tree, four pairs at a time so that SHA-NI's latency is hidden (sha256_compress_xn).
#include "otedama/merkle_tree.h"

#include <cstring>
#include <stdexcept>
#include <vector>

#include "otedama/sha256.h"

namespace otedama {

namespace {

// level: c nodes of 32 bytes -> (c + 1) / 2 nodes, in place (node p is written after pairs up to p + 3 were read).
void fold_level(uint8_t* level, size_t c) {
  uint8_t kPad[64] = {0x80};  // the second block of every 64-byte message
  kPad[62] = 0x02;            // 512 bits
  const size_t pairs = (c + 1) / 2;
  for (size_t p0 = 0; p0 < pairs; p0 += 4) {
    const int g = int(pairs - p0 < 4 ? pairs - p0 : 4);
    uint32_t st[4][8], dg[4][8];
    uint32_t* sp[4];
    uint32_t* dp[4];
    const uint8_t* bp[4];
    uint8_t last[64], blk[4][64];
    for (int k = 0; k < g; ++k) {
      const size_t p = p0 + size_t(k);
      std::memcpy(st[k], kSha256IV, 32);
      std::memcpy(dg[k], kSha256IV, 32);
      sp[k] = st[k];
      dp[k] = dg[k];
      if (2 * p + 1 < c) {
        bp[k] = level + 64 * p;
      } else {  // the last node of an odd level: paired with itself
        std::memcpy(last, level + 64 * p, 32);
        std::memcpy(last + 32, level + 64 * p, 32);
        bp[k] = last;
      }
    }
    sha256_compress_xn(g, sp, bp);
    for (int k = 0; k < g; ++k) bp[k] = kPad;
    sha256_compress_xn(g, sp, bp);
    for (int k = 0; k < g; ++k) {  // the digest, padded to one block
      std::memset(blk[k], 0, 64);
      for (int w = 0; w < 8; ++w) store_be32(blk[k] + 4 * w, st[k][w]);
      blk[k][32] = 0x80;
      blk[k][62] = 0x01;  // 256 bits
      bp[k] = blk[k];
    }
    sha256_compress_xn(g, dp, bp);
    for (int k = 0; k < g; ++k)
      for (int w = 0; w < 8; ++w) store_be32(level + 32 * (p0 + size_t(k)) + 4 * w, dg[k][w]);
  }
}

}  // namespace

void merkle_tree_cpu(const uint8_t* leaves, uint32_t t, uint32_t n, uint8_t* out) {
  if (t == 0 || t > kMerkleTreeMaxTrees) throw std::invalid_argument("merkle tree: t must be in 1..65535");
  if (n == 0 || n > kMerkleTreeMaxLeaves) throw std::invalid_argument("merkle tree: n must be in 1..262144");
  const uint32_t depth = merkle_tree_depth(n);
  std::vector<uint8_t> level(size_t(n) * 32);
  for (uint32_t y = 0; y < t; ++y) {
    std::memcpy(level.data(), leaves + size_t(y) * n * 32, size_t(n) * 32);
    uint8_t* rows = out + size_t(y) * (1 + depth) * 32;
    size_t c = n;
    for (uint32_t l = 0; l < depth; ++l) {  // c >= 2 here
      std::memcpy(rows + 32 * (1 + size_t(l)), level.data() + 32, 32);
      fold_level(level.data(), c);
      c = (c + 1) / 2;
    }
    std::memcpy(rows, level.data(), 32);
  }
}

}  // namespace otedama
