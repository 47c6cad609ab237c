// The GPU miner's search plan: which nonces a launch covers, how launches tile the 2^32 nonce range of a header
// variant, and which SHA-256d layout a stripe group gets. Plain integer arithmetic with no HIP in it, so the rules
// that decide whether a nonce is skipped or searched twice are tested on the CPU (tests/test_native_cpu.py,
// tools/sanitize/stress_runtime.cpp). csrc/runtime/gpu_miner.hip is the only production caller.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "otedama/job.h"

namespace otedama {

// Hit-ring records per launch (16 B each, host-coherent). Launches are sized from the share target so the expected
// candidates per launch stay at or below kHitCap / 8 (see launch_cap_hashes); what still overflows is counted.
constexpr uint32_t kHitCap = 4096;
constexpr uint64_t kMinLaunchHashes = 1ull << 22;  // below ~0.2 ms per launch the launch overhead would dominate
constexpr uint64_t kNoLaunchCap = 1ull << 40;      // above any batch: the launch is not cut
constexpr uint64_t kNonceSpace = 1ull << 32;

// Nonces per batch as the miner uses them: 0 or more than 2^32 means 2^30, and batches must tile the 2^32 nonce
// range exactly, so anything else is rounded down to a divisor of 2^32.
inline uint64_t normalize_batch(uint64_t batch_nonces) {
  if (batch_nonces == 0 || batch_nonces > kNonceSpace) batch_nonces = 1ull << 30;
  while (kNonceSpace % batch_nonces) --batch_nonces;
  return batch_nonces;
}

// Hashes per launch for a share target: the kernels' prefilter passes a hash whose top word is <= the target's,
// i.e. with probability (target_hi + 1) / 2^32, so expected candidates per launch = hashes * that. Launches are cut
// (powers of two, so they still tile 2^32) until that is <= kHitCap / 8; the hit ring then overflows only on a
// draw ~8 sigma above the mean at the floor target, and any overflow is counted. `capped` false
// (OTEDAMA_LAUNCH_CAP=0): launches keep their batch (overflow tests).
inline uint64_t launch_cap_hashes(uint32_t target_hi, bool capped) {
  if (!capped) return kNoLaunchCap;
  const double p = (double(target_hi) + 1.0) / 4294967296.0;
  const double lim = double(kHitCap / 8) / p;
  uint64_t cap = kNoLaunchCap;
  while (cap > kMinLaunchHashes && double(cap) > lim) cap >>= 1;
  return cap;
}

// SHA-256d layout of a stripe group: `nvar` header variants per launch; use_v = a version-parallel kernel (128 =
// two chains per lane, 64 = one), otherwise the K-variant kernel (nvar > 1) or the single-header kernel.
struct ShaLayout {
  int nvar = 1;
  bool use_v = false;
};

// The layout for a miner configured with `sha_variants` (GpuMiner's constructor argument; < 1 counts as 1) when
// `run` consecutive stripe positions share block 2. 128 and 64 are all-or-nothing; below them the K-variant kernel
// takes what the run supplies, at most 16, rounded down to an instantiated K (2, 3, 4, 6, 8, 12, 16). A
// sha_variants of 17..63 therefore means K = 16. pick_layout(sha_variants, kSha256dV2Group) is the largest layout
// the configuration can use, i.e. how long a run is worth looking for.
inline ShaLayout pick_layout(int sha_variants, int run) {
  const int sha_k = sha_variants < 1 ? 1 : sha_variants > kSha256dMaxK ? kSha256dMaxK : sha_variants;
  if (sha_variants >= kSha256dV2Group && run >= kSha256dV2Group) return {kSha256dV2Group, true};
  if (sha_variants >= kSha256dVGroup && run >= kSha256dVGroup) return {kSha256dVGroup, true};
  if (sha_k > 1) return {sha256d_k_floor(std::min(run, sha_k)), false};
  return {1, false};
}

enum class LaunchKind { kScrypt, kX11, kVersionParallel, kVariantK, kSingle };

// Nonces per variant of the next launch. `batch` is the miner's normalised batch, `cap` launch_cap_hashes() of the
// job's target, `nonce_off` the cursor; the launch never runs past 2^32.
//  * scrypt, X11: `lanes` nonces (the buffers' capacity), cut by the cap; the batch setting does not apply.
//  * version-parallel: W3 (big-endian nonce word) windows tile [0, 2^32) exactly like the nonce windows of the other
//    kernels; the launch's duration stays min(batch, cap) hashes over all `nvar` variants.
//  * K-variant: keeps one launch's duration about independent of K: nonces per variant = launch / (largest power of
//    two <= K); launch is a power of two that tiles 2^32, so this still tiles it. At K = 3, 6, 12 a launch therefore
//    holds 1.5x the capped hashes (K variants over launch / (2K/3) nonces). Known and kept.
//  * single: min(batch, cap) nonces.
inline uint64_t launch_count(LaunchKind kind, uint64_t batch, uint64_t cap, int nvar, uint64_t lanes,
                             uint64_t nonce_off) {
  const uint64_t remaining = kNonceSpace - nonce_off;
  const uint64_t launch = std::min(batch, cap);
  switch (kind) {
    case LaunchKind::kScrypt:
    case LaunchKind::kX11:
      return std::min({remaining, lanes, cap});
    case LaunchKind::kVersionParallel:
      return std::min(launch >= uint64_t(nvar) ? launch / uint64_t(nvar) : 1, remaining);
    case LaunchKind::kVariantK: {
      uint64_t div = 1;
      while (div * 2 <= uint64_t(nvar) && div * 2 <= launch) div *= 2;
      return std::min(launch / div, remaining);
    }
    case LaunchKind::kSingle:
      break;
  }
  return std::min(launch, remaining);
}

// Where the search stands inside a device's variant stripe: stripe position `k` of the current group and the next
// nonce of that group's 2^32 range.
struct SearchCursor {
  uint64_t k = 0;
  uint64_t nonce_off = 0;

  void reset() { k = 0; nonce_off = 0; }
  // A launch of `count` nonces over a group of `nvar` variants was queued: past 2^32 the next group starts.
  void advance(uint64_t count, int nvar) {
    nonce_off += count;
    if (nonce_off >= kNonceSpace) { nonce_off = 0; k += uint64_t(nvar); }
  }
  // MinerStats::variant_next: the first variant index of the stripe no launch has started on. While a group of `nvar`
  // variants is part-way through its nonces that is the group after it.
  uint64_t variant_next(uint64_t variant_start, uint64_t variant_stride, int nvar) const {
    return variant_start + (nonce_off == 0 ? k : k + uint64_t(nvar)) * variant_stride;
  }
};

// OTEDAMA_RESERVE_CUS=<cu>,<cu>,...: a CU mask of `ncu` bits without the listed CUs, and how many it left out.
// Out-of-range and repeated entries are ignored; parsing stops at the first thing that is not a number.
struct CuMask {
  std::vector<uint32_t> words;
  int reserved = 0;
};
inline CuMask parse_reserved_cus(const char* spec, int ncu) {
  CuMask m;
  m.words.assign(size_t(ncu + 31) / 32, 0xFFFFFFFFu);
  if (ncu % 32) m.words.back() = (1u << (ncu % 32)) - 1u;
  for (const char* q = spec; *q;) {
    char* end = nullptr;
    const long cu = std::strtol(q, &end, 10);
    if (end == q) break;
    if (cu >= 0 && cu < ncu && (m.words[size_t(cu) / 32] >> (cu % 32) & 1u)) {
      m.words[size_t(cu) / 32] &= ~(1u << (cu % 32));
      ++m.reserved;
    }
    q = (*end == ',') ? end + 1 : end;
  }
  return m;
}

// Hash accounting of a finished launch. A launch stopped by the abort word is credited what the rate of the
// completed launches says it did in its `ms` on the device, at most its `full` hashes (all of them until a rate is
// known).
inline uint64_t aborted_launch_hashes(uint64_t full, double rate_hpms, double ms) {
  return rate_hpms > 0 ? std::min<uint64_t>(full, uint64_t(rate_hpms * ms)) : full;
}
// Hashes per ms over completed launches (first sample, then an EMA).
inline double update_rate_hpms(double rate_hpms, uint64_t full, double ms) {
  return rate_hpms > 0 ? 0.8 * rate_hpms + 0.2 * (double(full) / ms) : double(full) / ms;
}
// Seconds per scrypt hash of one lane (= one full batch of `ms` on the device), an EMA.
inline double update_scrypt_hash_s(double scrypt_hash_s, double ms) { return 0.7 * scrypt_hash_s + 0.3e-3 * ms; }

}  // namespace otedama
