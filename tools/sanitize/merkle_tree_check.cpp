// Stand-alone host check of the template tree's CPU twin (csrc/cpu/merkle_tree.cpp) for ASan + UBSan builds
// (tools/sanitize/run.sh): merkle_tree_cpu on exactly sized heap buffers over small sizes, the chunk edges and a
// Bitcoin-sized tree, one and two trees a call, every root compared with a level-by-level sha256d fold written out
// here, plus the limit violations.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "otedama/merkle_tree.h"
#include "otedama/sha256.h"
using namespace otedama;
static void ref_root(std::vector<uint8_t> lv, size_t c, uint8_t out[32]) {
  while (c > 1) {
    std::vector<uint8_t> nx(((c + 1) / 2) * 32);
    for (size_t p = 0; p < (c + 1) / 2; ++p) {
      uint8_t m[64];
      std::memcpy(m, &lv[64 * p], 32);
      std::memcpy(m + 32, &lv[32 * ((2 * p + 1 < c) ? 2 * p + 1 : 2 * p)], 32);
      sha256d(m, 64, &nx[32 * p]);
    }
    lv.swap(nx); c = (c + 1) / 2;
  }
  std::memcpy(out, lv.data(), 32);
}
int main() {
  int fails = 0, cases = 0;
  for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 7u, 8u, 9u, 15u, 17u, 255u, 257u, 513u, 1025u, 4001u})
    for (uint32_t t : {1u, 2u}) {
      std::vector<uint8_t> leaves(size_t(t) * n * 32);  // exactly sized heap buffers
      for (size_t i = 0; i < leaves.size(); ++i) leaves[i] = uint8_t(i * 131 + n);
      const uint32_t d = merkle_tree_depth(n);
      std::vector<uint8_t> out(size_t(t) * (1 + d) * 32);
      merkle_tree_cpu(leaves.data(), t, n, out.data());
      for (uint32_t y = 0; y < t; ++y) {
        uint8_t r[32];
        ref_root(std::vector<uint8_t>(leaves.begin() + size_t(y) * n * 32, leaves.begin() + size_t(y + 1) * n * 32), n, r);
        fails += std::memcmp(r, &out[size_t(y) * (1 + d) * 32], 32) != 0;
        ++cases;
      }
    }
  int limits = 0;
  uint8_t leaf[32] = {0}, row[32];
  auto throws = [&](uint32_t t, uint32_t n) {
    try {
      merkle_tree_cpu(leaf, t, n, row);
    } catch (const std::invalid_argument&) {
      return 1;
    }
    return 0;
  };
  limits += throws(0, 1) + throws(1, 0) + throws(1, kMerkleTreeMaxLeaves + 1) + throws(kMerkleTreeMaxTrees + 1, 1);
  fails += limits != 4;
  std::printf("merkle_tree_check: %d trees, %d limit violations refused, %d failures\n", cases, limits, fails);
  return fails != 0;
}
