// Host side of share verification (otedama/share_job.h): the job block builder and a plain C++ walker of the same
// block, so that the block format (every len(coinb1) mod 64, every extranonce alignment, every padding edge) is
// testable without a GPU. otd_share_headers (csrc/kernels/share_verify.hip) does per lane what the walker does per
// record, otd_channel_roots (csrc/kernels/channel_roots.hip) what share_roots_cpu does per prefix.
#include "otedama/share_job.h"

#include <cstring>
#include <stdexcept>

#include "otedama/sha256.h"

namespace otedama {

namespace {

// The 256-bit target of a compact nBits value as 32 little-endian bytes (models/header.py target_from_nbits).
void target_from_nbits(uint32_t nbits, uint8_t out[32]) {
  const uint32_t exp = nbits >> 24, mant = nbits & 0x007FFFFFu;
  if (nbits & 0x00800000u) throw std::invalid_argument("nbits: negative mantissa bit set");
  if (exp < 3) throw std::invalid_argument("nbits: exponent below 3");
  if (mant == 0) throw std::invalid_argument("nbits: zero mantissa");
  std::memset(out, 0, 32);
  for (uint32_t k = 0; k < 3; ++k) {
    const uint8_t byte = uint8_t(mant >> (8 * k));
    const uint32_t pos = exp - 3 + k;
    if (pos < 32) out[pos] = byte;
    else if (byte) throw std::invalid_argument("nbits: target overflows 256 bits");
  }
}

void words_le(const uint8_t* p, int n, uint32_t* out) {
  for (int i = 0; i < n; ++i) out[i] = load_le32(p + 4 * i);
}

void check_block(const ShareJobBlock& job) {
  if (job.magic != kShareJobMagic || job.en_size < 1 || job.en_size > uint32_t(kShareMaxExtranonce) ||
      job.tail_blocks < 1 || job.tail_blocks > uint32_t(kShareMaxTailBlocks) || job.en_offset > 63 ||
      job.en_offset + job.en_size > job.tail_blocks * 64 || job.n_branches > uint32_t(kShareMaxBranches))
    throw std::invalid_argument("not a share job block");
}

// SHA-256 of a 32-byte digest given as its big-endian words: one padded block.
void sha256_of_digest(const uint32_t in[8], uint32_t out[8]) {
  uint8_t blk[64] = {0};
  for (int k = 0; k < 8; ++k) store_be32(blk + 4 * k, in[k]);
  blk[32] = 0x80;
  blk[62] = 0x01;  // 256 bits
  std::memcpy(out, kSha256IV, 32);
  sha256_compress(out, blk);
}

}  // namespace

ShareJobBlock share_job_prepare(const std::string& coinb1, const std::string& coinb2, int en_size,
                                const std::string& prev_hash, uint32_t nbits,
                                const std::vector<std::string>& branches) {
  if (en_size < 1 || en_size > kShareMaxExtranonce) throw std::invalid_argument("en_size must be in 1..16");
  if (prev_hash.size() != 32) throw std::invalid_argument("prev_hash must be 32 bytes");
  if (branches.size() > size_t(kShareMaxBranches)) throw std::invalid_argument("at most 32 merkle branches");
  for (const auto& b : branches)
    if (b.size() != 32) throw std::invalid_argument("every merkle branch must be 32 bytes");
  const size_t whole = coinb1.size() / 64;
  const size_t total = coinb1.size() + size_t(en_size) + coinb2.size();
  const size_t tail_len = total - whole * 64;
  const size_t blocks = (tail_len + 9 + 63) / 64;  // 0x80 and the 8-byte bit length
  if (blocks > size_t(kShareMaxTailBlocks)) throw std::invalid_argument("coinbase tail longer than 32 blocks");

  ShareJobBlock job;
  std::memset(&job, 0, sizeof job);
  job.magic = kShareJobMagic;
  job.en_size = uint32_t(en_size);
  job.tail_blocks = uint32_t(blocks);
  job.en_offset = uint32_t(coinb1.size() % 64);
  job.n_branches = uint32_t(branches.size());
  job.nbits = nbits;
  words_le(reinterpret_cast<const uint8_t*>(prev_hash.data()), 8, job.prev_hash);
  uint8_t tgt[32];
  target_from_nbits(nbits, tgt);
  words_le(tgt, 8, job.net_target);

  std::memcpy(job.midstate, kSha256IV, 32);
  for (size_t b = 0; b < whole; ++b)
    sha256_compress(job.midstate, reinterpret_cast<const uint8_t*>(coinb1.data()) + 64 * b);

  std::vector<uint8_t> tail(blocks * 64, 0);
  const size_t c1_tail = coinb1.size() - whole * 64;
  std::memcpy(tail.data(), coinb1.data() + whole * 64, c1_tail);
  std::memcpy(tail.data() + c1_tail + size_t(en_size), coinb2.data(), coinb2.size());
  tail[tail_len] = 0x80;
  const uint64_t bits = uint64_t(total) * 8;
  for (int k = 0; k < 8; ++k) tail[blocks * 64 - 1 - size_t(k)] = uint8_t(bits >> (8 * k));
  for (size_t w = 0; w < blocks * 16; ++w) job.tail[w] = load_be32(tail.data() + 4 * w);
  for (size_t b = 0; b < branches.size(); ++b)
    for (int k = 0; k < 8; ++k)
      job.branches[8 * b + size_t(k)] = load_be32(reinterpret_cast<const uint8_t*>(branches[b].data()) + 4 * k);
  return job;
}

namespace {

// The merkle root of one extranonce against a checked block, as big-endian state words: the coinbase txid (midstate,
// the tail blocks with the extranonce patched in, then the hash of that digest) folded over the branches.
void root_words(const ShareJobBlock& job, const uint8_t* extranonce, uint32_t cur[8]) {
  uint32_t st[8];
  std::memcpy(st, job.midstate, 32);
  for (uint32_t b = 0; b < job.tail_blocks; ++b) {
    uint8_t blk[64];
    for (int w = 0; w < 16; ++w) store_be32(blk + 4 * w, job.tail[16 * b + uint32_t(w)]);
    for (uint32_t j = 0; j < job.en_size; ++j) {
      const uint32_t at = job.en_offset + j;
      if (at / 64 == b) blk[at % 64] = extranonce[j];
    }
    sha256_compress(st, blk);
  }
  sha256_of_digest(st, cur);
  // merkle fold: cur = sha256d(cur | branch)
  for (uint32_t b = 0; b < job.n_branches; ++b) {
    uint8_t blk[64];
    for (int k = 0; k < 8; ++k) {
      store_be32(blk + 4 * k, cur[k]);
      store_be32(blk + 32 + 4 * k, job.branches[8 * b + uint32_t(k)]);
    }
    std::memcpy(st, kSha256IV, 32);
    sha256_compress(st, blk);
    uint8_t pad[64] = {0};
    pad[0] = 0x80;
    pad[62] = 0x02;  // 512 bits
    sha256_compress(st, pad);
    sha256_of_digest(st, cur);
  }
}

}  // namespace

void share_headers_cpu(const ShareJobBlock& job, const ShareRec* recs, size_t n, uint8_t* out) {
  check_block(job);
  for (size_t i = 0; i < n; ++i) {
    const ShareRec& r = recs[i];
    uint32_t cur[8];
    root_words(job, r.extranonce, cur);
    uint8_t* h = out + 80 * i;
    store_le32(h, r.version);
    for (int k = 0; k < 8; ++k) store_le32(h + 4 + 4 * k, job.prev_hash[k]);
    for (int k = 0; k < 8; ++k) store_be32(h + 36 + 4 * k, cur[k]);
    store_le32(h + 68, r.ntime);
    store_le32(h + 72, job.nbits);
    store_le32(h + 76, r.nonce);
  }
}

void share_roots_cpu(const ShareJobBlock& job, const uint8_t* prefixes, size_t n, uint8_t* out) {
  check_block(job);
  for (size_t i = 0; i < n; ++i) {
    uint32_t cur[8];
    root_words(job, prefixes + 16 * i, cur);
    for (int k = 0; k < 8; ++k) store_be32(out + 32 * i + 4 * k, cur[k]);
  }
}

void share_results_cpu(const ShareJobBlock& job, const ShareRec* recs, size_t n, const uint8_t* targets,
                       size_t n_targets, ShareResult* out) {
  if (n_targets == 0 || !targets) throw std::invalid_argument("the target table is empty");
  uint8_t net[32];
  for (int k = 0; k < 8; ++k) store_le32(net + 4 * k, job.net_target[k]);
  for (size_t i = 0; i < n; ++i) {
    ShareResult& r = out[i];
    std::memset(&r, 0, sizeof r);
    share_headers_cpu(job, recs + i, 1, r.header);
    sha256d(r.header, 80, r.hash);
    const uint32_t idx = recs[i].target_index;
    if (idx >= n_targets)
      r.verdict = kVerdictBadIndex;
    else
      r.verdict = uint8_t((le256_leq(r.hash, targets + 32 * size_t(idx)) ? kVerdictShare : 0) |
                          (le256_leq(r.hash, net) ? kVerdictNetwork : 0));
  }
}

}  // namespace otedama
