// Template tree (csrc/kernels/merkle_tree.hip, csrc/cpu/merkle_tree.cpp): the rows both write and the limits both keep.
//
// t merkle trees of n >= 1 leaves each, 32 bytes a leaf in internal byte order, tree y at leaves + 32 * n * y. Levels
// fold pairwise with SHA-256d; an odd level pairs its last node with itself (Bitcoin's rule). Each tree yields
// 1 + depth rows of 32 bytes, depth = (n - 1).bit_length(), at out + 32 * (1 + depth) * y: row 0 is the root, row
// 1 + l is node 1 of level l, the sibling of the leftmost path, so rows 1..depth are the merkle branches of leaf 0
// and do not depend on it.
#pragma once
#include <cstdint>

namespace otedama {

constexpr uint32_t kMerkleTreeMaxLeaves = 262144;  // 512 chunks of 512 nodes: two launches at most
constexpr uint32_t kMerkleTreeMaxTrees = 65535;    // the tree is the launch grid's y

inline uint32_t merkle_tree_depth(uint32_t n) {  // (n - 1).bit_length() for n >= 1
  uint32_t d = 0;
  while ((uint64_t(1) << d) < n) ++d;
  return d;
}

// The rows in plain C++ over the host SHA-256 (SHA-NI where present). Throws std::invalid_argument for t == 0 or
// above kMerkleTreeMaxTrees, n == 0 or above kMerkleTreeMaxLeaves.
void merkle_tree_cpu(const uint8_t* leaves, uint32_t t, uint32_t n, uint8_t* out);

}  // namespace otedama
