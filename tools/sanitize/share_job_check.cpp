// Stand-alone host check of the share job block (csrc/cpu/share_job.cpp) for ASan + UBSan builds
// (tools/sanitize/run.sh): share_job_prepare and share_headers_cpu over the length grid of
// tests/test_share_verify_cpu.py, each header compared with a straightforward rebuild (sha256d of the whole
// coinbase, the merkle fold, the packed header), share_roots_cpu's roots compared with those headers' roots, plus the
// limit violations. Exit status 0 = all equal.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "otedama/sha256.h"
#include "otedama/share_job.h"

using namespace otedama;

namespace {

uint64_t g_seed = 0x9E3779B97F4A7C15ull;
uint8_t next_byte() {
  g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
  return uint8_t(g_seed >> 32);
}
std::string bytes(size_t n) {
  std::string s(n, '\0');
  for (auto& c : s) c = char(next_byte());
  return s;
}

std::string reference_header(const std::string& c1, const std::string& c2, int en_size, const std::string& prev,
                             uint32_t nbits, const std::vector<std::string>& branches, const ShareRec& r) {
  std::string cb = c1 + std::string(reinterpret_cast<const char*>(r.extranonce), size_t(en_size)) + c2;
  uint8_t cur[32];
  sha256d(reinterpret_cast<const uint8_t*>(cb.data()), cb.size(), cur);
  for (const auto& b : branches) {
    uint8_t cat[64];
    std::memcpy(cat, cur, 32);
    std::memcpy(cat + 32, b.data(), 32);
    sha256d(cat, 64, cur);
  }
  std::string h(80, '\0');
  uint8_t* p = reinterpret_cast<uint8_t*>(&h[0]);
  store_le32(p, r.version);
  std::memcpy(p + 4, prev.data(), 32);
  std::memcpy(p + 36, cur, 32);
  store_le32(p + 68, r.ntime);
  store_le32(p + 72, nbits);
  store_le32(p + 76, r.nonce);
  return h;
}

template <class F>
bool throws(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

}  // namespace

int main() {
  const int len1s[] = {1, 2, 41, 55, 56, 62, 63, 64, 65, 119, 120, 128, 200};
  const int en_sizes[] = {1, 4, 8, 13, 16};
  const int total_mods[] = {0, 55, 56, 63};
  const int branch_counts[] = {0, 1, 12, 32};
  const uint32_t nbits = 0x2000FFFFu;
  int jobs = 0, failures = 0;
  for (int len1 : len1s)
    for (int en : en_sizes)
      for (int mod : total_mods)
        for (int nb : branch_counts) {
          const int len2 = ((mod - len1 - en) % 64 + 64) % 64 + 64 * ((len1 + mod) % 2);
          const std::string c1 = bytes(size_t(len1)), c2 = bytes(size_t(len2)), prev = bytes(32);
          std::vector<std::string> br;
          for (int k = 0; k < nb; ++k) br.push_back(bytes(32));
          const ShareJobBlock job = share_job_prepare(c1, c2, en, prev, nbits, br);
          std::vector<ShareRec> recs(3);
          for (auto& r : recs) {
            for (auto& b : r.extranonce) b = next_byte();  // bytes past en_size are set too: they must be ignored
            r.ntime = uint32_t(next_byte()) << 24 | next_byte();
            r.nonce = uint32_t(next_byte()) << 16 | next_byte();
            r.version = 0x20000000u | uint32_t(next_byte()) << 13;
            r.target_index = 0;
          }
          std::vector<uint8_t> out(80 * recs.size());
          share_headers_cpu(job, recs.data(), recs.size(), out.data());
          for (size_t i = 0; i < recs.size(); ++i) {
            const std::string want = reference_header(c1, c2, en, prev, nbits, br, recs[i]);
            if (std::memcmp(want.data(), out.data() + 80 * i, 80) != 0) {
              std::fprintf(stderr, "mismatch: len1=%d en=%d len2=%d branches=%d record %zu\n", len1, en, len2, nb, i);
              ++failures;
            }
          }
          // share_roots_cpu on exactly sized heap buffers: prefix rows in, the merkle roots of the headers out
          std::vector<uint8_t> rows(16 * recs.size()), roots(32 * recs.size());
          for (size_t i = 0; i < recs.size(); ++i) std::memcpy(rows.data() + 16 * i, recs[i].extranonce, 16);
          share_roots_cpu(job, rows.data(), recs.size(), roots.data());
          for (size_t i = 0; i < recs.size(); ++i)
            if (std::memcmp(roots.data() + 32 * i, out.data() + 80 * i + 36, 32) != 0) {
              std::fprintf(stderr, "root mismatch: len1=%d en=%d len2=%d branches=%d prefix %zu\n", len1, en, len2, nb,
                           i);
              ++failures;
            }
          ++jobs;
        }

  // limits: each must be refused, and the last sizes that fit must pass
  const std::string prev(32, '\x11'), c1(50, '\x22'), c2(60, '\x33');
  const std::vector<std::string> one{std::string(32, '\x44')};
  int limits = 0;
  limits += throws([&] { share_job_prepare(c1, c2, 0, prev, nbits, one); });
  limits += throws([&] { share_job_prepare(c1, c2, 17, prev, nbits, one); });
  limits += throws([&] { share_job_prepare(c1, c2, 8, prev, nbits, std::vector<std::string>(33, one[0])); });
  limits += throws([&] { share_job_prepare(c1, c2, 8, prev, nbits, {one[0], std::string(31, '\x44')}); });
  limits += throws([&] { share_job_prepare(c1, c2, 8, std::string(31, '\x11'), nbits, one); });
  limits += throws([&] { share_job_prepare("\x01", std::string(32 * 64 - 9 - 1 - 8 + 1, '\0'), 8, prev, nbits, one); });
  limits += throws([&] { share_job_prepare(c1, c2, 8, prev, 0x1D800000u, one); });
  limits += throws([&] { share_job_prepare(c1, c2, 8, prev, 0x22010000u, one); });
  ShareJobBlock bad = share_job_prepare("\x01", std::string(32 * 64 - 9 - 1 - 8, '\0'), 8, prev, nbits,
                                        std::vector<std::string>(32, one[0]));  // 32 blocks, 32 branches: fits
  ShareRec r{};
  uint8_t hdr[80];
  share_headers_cpu(bad, &r, 1, hdr);
  share_headers_cpu(bad, nullptr, 0, hdr);
  bad.tail_blocks = 33;
  limits += throws([&] { share_headers_cpu(bad, &r, 1, hdr); });
  bad.tail_blocks = 32;
  bad.n_branches = 33;
  limits += throws([&] { share_headers_cpu(bad, &r, 1, hdr); });
  bad.n_branches = 32;
  bad.en_size = 17;
  limits += throws([&] { share_headers_cpu(bad, &r, 1, hdr); });
  if (limits != 11) {
    std::fprintf(stderr, "only %d of 11 limit violations were refused\n", limits);
    ++failures;
  }
  std::printf("share_job_check: %d jobs, %d limit violations refused, %d failures\n", jobs, limits, failures);
  return failures ? 1 : 0;
}
