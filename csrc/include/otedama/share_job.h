// Share verification (csrc/kernels/share_verify.hip, csrc/cpu/share_job.cpp): the two layouts a batch of pool
// shares travels in. A pool holds a job (coinb1, coinb2, merkle branches, prev_hash, nbits) and receives shares
// (extranonce, ntime, nonce, version); the headers are never materialised on the host. The job becomes one
// ShareJobBlock, built once per job and uploaded; every share becomes one 32-byte ShareRec. Both the host code and
// the kernels include this file, so it is plain C++ with no HIP types.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace otedama {

constexpr int kShareMaxTailBlocks = 32;  // 64-byte SHA-256 blocks of coinbase after the midstate
constexpr int kShareMaxBranches = 32;
constexpr int kShareMaxExtranonce = 16;

// One share, little-endian, 16-byte aligned (two 16-byte loads).
struct alignas(16) ShareRec {
  uint8_t extranonce[16];  // the first en_size bytes are used, the rest ignored
  uint32_t ntime;
  uint32_t nonce;
  uint32_t version;  // the full rolled version
  uint32_t target_index;  // into the target table of the launch
};
static_assert(sizeof(ShareRec) == 32, "ShareRec is 32 bytes");

// Verdict byte of one share.
constexpr uint8_t kVerdictShare = 1;      // hash <= targets[target_index]
constexpr uint8_t kVerdictNetwork = 2;    // hash <= the network target of nbits
constexpr uint8_t kVerdictBadIndex = 0x80;  // target_index outside the table; no other bit is set

// One verified share, as the live path returns it (otd_share_pack of csrc/kernels/share_verify.hip): eight 16-byte
// stores.
struct alignas(16) ShareResult {
  uint8_t header[80];  // the bytes otd_share_headers writes
  uint8_t hash[32];    // the algorithm's hash of the header
  uint8_t verdict;     // as above; for kVerdictBadIndex the table was not read, header and hash are still written
  uint8_t zero[15];    // written as zeros
};
static_assert(sizeof(ShareResult) == 128, "ShareResult is 128 bytes");

// One job. Everything a kernel reads from it is the same for every share of the launch (wave-uniform).
//   coinbase = coinb1 | extranonce | coinb2. `midstate` is the SHA-256 state after the whole 64-byte blocks that lie
//   entirely inside coinb1; `tail` is the rest, coinb1_tail | zeros(en_size) | coinb2 with the SHA-256 padding and
//   the bit length of the whole coinbase applied, as big-endian words; the extranonce starts `en_offset` bytes
//   into it (any byte alignment, possibly across a block boundary).
struct alignas(16) ShareJobBlock {
  uint32_t magic;
  uint32_t en_size;      // 1..16
  uint32_t tail_blocks;  // 1..32
  uint32_t en_offset;    // 0..63
  uint32_t n_branches;   // 0..32
  uint32_t nbits;
  uint32_t reserved[2];
  uint32_t prev_hash[8];   // header bytes 4..35 as little-endian words
  uint32_t net_target[8];  // target of nbits as little-endian words, word 7 most significant
  uint32_t midstate[8];
  uint32_t tail[kShareMaxTailBlocks * 16];
  uint32_t branches[kShareMaxBranches * 8];  // big-endian words: the second half of each merkle message
};
constexpr uint32_t kShareJobMagic = 0x31424a53u;  // "SJB1"
static_assert(sizeof(ShareJobBlock) % 16 == 0, "ShareJobBlock is a whole number of 16-byte vectors");

// Builds the block. Throws std::invalid_argument for a tail of more than 32 blocks, more than 32 branches, en_size
// outside 1..16, a prev_hash or branch that is not 32 bytes, or an nbits without a valid target: the caller's cue
// to verify that job on the CPU.
ShareJobBlock share_job_prepare(const std::string& coinb1, const std::string& coinb2, int en_size,
                                const std::string& prev_hash, uint32_t nbits,
                                const std::vector<std::string>& branches);

// The job block walked in plain C++: n records -> n 80-byte headers at out + 80 * i, what otd_share_headers
// writes. Throws std::invalid_argument for a block that share_job_prepare could not have produced.
void share_headers_cpu(const ShareJobBlock& job, const ShareRec* recs, size_t n, uint8_t* out);

// What the live path writes for SHA-256d (otd_share_headers, the digest launch, otd_share_pack), in plain C++: n
// records against a table of n_targets 32-byte little-endian targets -> n ShareResult records (SHA-256d of
// share_headers_cpu's header, le256_leq against the share's target and the job's network target). A target index
// outside the table gives kVerdictBadIndex with header and hash still written. Throws std::invalid_argument like
// share_headers_cpu, and for an empty table.
void share_results_cpu(const ShareJobBlock& job, const ShareRec* recs, size_t n, const uint8_t* targets,
                       size_t n_targets, ShareResult* out);

// The merkle roots of n extranonce prefixes against one job (what otd_channel_roots of
// csrc/kernels/channel_roots.hip writes): prefixes + 16 * i holds prefix i, of which the first en_size bytes are used;
// out + 32 * i receives sha256d(coinb1 | prefix | coinb2) folded over the job's branches, in header byte order.
// Throws std::invalid_argument like share_headers_cpu.
void share_roots_cpu(const ShareJobBlock& job, const uint8_t* prefixes, size_t n, uint8_t* out);

}  // namespace otedama
