// GpuMiner: one host thread per GPU driving search batches on private HIP streams.
//
// Share path: a kernel publishes each hit the moment it is found into a ring of HitRecords in host-coherent
// pinned memory (record, system-scope fence, tag: otedama/hitsink.h). This thread polls the rings of the
// batches in flight every ~100 us, re-verifies each candidate on the CPU (full 256-bit compare against the
// job's current target) and pushes the share to the queue, whose eventfd wakes the control plane. A hit is
// therefore on its way to the pool while the launch that found it is still running, instead of after the
// batch (2^29 nonces, ~28 ms) and its copy-back.
//
// Job switches: new work opens a new launch epoch and writes it to an uncached device word. The CPU stores it
// straight into VRAM through the PCIe BAR when the runtime lets the CPU agent map the word; otherwise the store is a
// hipStreamWriteValue32 on a high-priority control stream, one more hardware queue (a 173 MiB host mapping,
// profiles/r4/c_host_abort/rss.jsonl). Every wave polls that word once per grid-stride trip, so batches of the old
// epoch stop within one trip (tens of us for SHA-256d, <= ~2 ms of ROMix for scrypt) and the first batch of the new
// work starts right behind them. The switch time (set_job -> new batch running) is recorded.
//
// Launch overlap: the two batches in flight sit on two streams (one per slot), so the next SHA-256d batch's waves
// fill the CUs that the running batch's tail leaves idle; without it a 2^29-nonce launch (28 ms) lost ~2.5% to its
// tail (profiles/r3/e_rehearsal). scrypt and X11 batches have per-slot buffers too (two 64 GiB halves of the scrypt
// pad, two X11 digest planes): the two scrypt half-batches run staggered by half a hash so that one of them reaches a
// ROMix phase boundary (its abort poll) every quarter hash, and a job switch waits ~T/8 instead of ~T/4 for the
// first half of the GPU to take the new work. OTEDAMA_SCRYPT_HALVES=0 / OTEDAMA_X11_OVERLAP=0 restore one shared
// buffer per algorithm with the batches chained (the A/B baselines).
//
// Device time: s_memrealtime (100 MHz) is mapped to CLOCK_MONOTONIC by a probe kernel at start-up (min round
// trip of several probes, before any search runs). After that every launch carries its own probe, queued on its
// stream just ahead of the search kernel: the host sees the stamp land while polling the hit rings, and each
// sighting bounds the offset from above (the store happened before it was seen). The mapping in use is the lowest
// bound of the last 2 s, so it follows drift between the two clocks without a stream or thread of its own, and a
// share carries the kernel's own hit time.
//
// The search-space arithmetic (launch sizes, the nonce / stripe cursor, the SHA-256d layout choice, the CU mask) is
// otedama/launch_plan.h: HIP-free and tested on the CPU.
//
// Parity: the reference's worker sends each share as it is found (internal/miner/worker.go:262-275) and picks
// up new work between 1024-nonce batches (worker.go:231-248).
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <immintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <stdexcept>
#include <string>
#include <unistd.h>

#include "otedama/clock_bounds.h"
#include "otedama/hip_check.h"
#include "otedama/hitsink.h"
#include "otedama/job.h"
#include "otedama/launch_plan.h"
#include "otedama/runtime.h"
#include "otedama/search_launch.h"
#include "otedama/sha256.h"
#include "otedama/trace.h"
#include "otedama/work_queue.h"
#include "otedama/x11_launch.h"

namespace otedama {

// Resident set of this process in MiB (/proc/self/statm), for the start-up phase record.
static double resident_mb() {
  FILE* f = std::fopen("/proc/self/statm", "r");
  if (!f) return 0;
  unsigned long size = 0, res = 0;
  const int n = std::fscanf(f, "%lu %lu", &size, &res);
  std::fclose(f);
  return n == 2 ? double(res) * double(sysconf(_SC_PAGESIZE)) / (1024.0 * 1024.0) : 0;
}

}  // namespace otedama

// Device clock probe: one lane stores the 64-bit 100 MHz real-time counter (vector store to host memory).
__global__ void otd_rt_probe(uint64_t* out) {
  if (threadIdx.x == 0) *out = __builtin_amdgcn_s_memrealtime();
}

namespace otedama {

namespace {
constexpr size_t kVerifyCap = 8192;  // scrypt candidates waiting for host verification (~1 ms each)
constexpr int kInflight = 2;
constexpr double kRtHz = 100e6;
constexpr auto kIdlePoll = std::chrono::microseconds(100);
constexpr double kClockWindowS = 2.0;  // per-launch clock bounds kept for the device -> host mapping
// Lane-cooperative full-line ROMix (gap 1, nt pad traffic, 16 blocks/CU = 128 GiB of HBM): ~16.75 MH/s vs
// 13.6-14.0 for the per-lane kernels at gap 1/2 (profiles/r1/scrypt_romix_ab.md).
constexpr int kScryptGap = kScryptCoop;
// X11: eleven stage kernels per batch over a 64 B/nonce digest buffer (512 MiB at 2^23).
constexpr uint32_t kX11Batch = 1u << 23;

// Let the CPU store to a device allocation directly: grant the CPU agent access (the allocation is VRAM, reachable
// through the PCIe BAR when the runtime exposes it) and confirm that the range is now mapped READ-WRITE in this process
// before anything touches it. libhsakmt reserves the GPU virtual-address range with PROT_NONE, so a mapping line alone
// proves nothing (small BAR, a VF without a mapped BAR): maps_range_writable requires the rw permissions. False leaves
// the word device-only (stores then go through a stream). The caller still verifies a store by reading it back.
bool cpu_store_map(void* p, size_t n) {
  hsa_agent_t cpu{};
  auto pick = [](hsa_agent_t a, void* data) -> hsa_status_t {
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) == HSA_STATUS_SUCCESS && t == HSA_DEVICE_TYPE_CPU) {
      *static_cast<hsa_agent_t*>(data) = a;
      return HSA_STATUS_INFO_BREAK;
    }
    return HSA_STATUS_SUCCESS;
  };
  if (hsa_iterate_agents(pick, &cpu) != HSA_STATUS_INFO_BREAK) return false;
  if (hsa_amd_agents_allow_access(1, &cpu, nullptr, p) != HSA_STATUS_SUCCESS) return false;
  FILE* f = std::fopen("/proc/self/maps", "r");
  if (!f) return false;
  std::string maps;
  char buf[4096];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) maps.append(buf, got);
  std::fclose(f);
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
  return maps_range_writable(maps, lo, lo + n);
}

// Owners of a run's HIP resources: the destructor releases the handle and ignores the error (on a faulted device
// every call fails and there is nothing left to do about it). Not copyable, so each handle is released once; when
// they are released is GpuMiner::Run's declaration order.
template <class T, class Drop>
struct Owned {
  T h{};
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { if (h) Drop()(h); }
  operator T() const { return h; }
};
struct FreeDevice { void operator()(void* p) const { (void)hipFree(p); } };
struct FreePinned { void operator()(void* p) const { (void)hipHostFree(p); } };
struct DestroyStream { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct DestroyEvent { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
template <class T> using DeviceMem = Owned<T*, FreeDevice>;
template <class T> using PinnedMem = Owned<T*, FreePinned>;
using Stream = Owned<hipStream_t, DestroyStream>;
using Event = Owned<hipEvent_t, DestroyEvent>;

// Header variants of one stripe group (up to 128 consecutive positions sharing block 2). Built once per
// (work generation, group) and shared by every launch of the group (~1000 launches at 2^29 nonces each).
struct Group {
  uint64_t gen = ~0ull, k = ~0ull;
  int nvar = 1;
  bool use_v = false;
  uint8_t header[kSha256dV2Group][80];
  uint32_t version[kSha256dV2Group] = {0}, ntime[kSha256dV2Group] = {0};
  uint64_t en2[kSha256dV2Group] = {0};
  Sha256dParamsV v_params{};
  Sha256dVariant v_table[kSha256dV2Group];
};

// A published hit handed to the verifier thread (scrypt), with everything needed to rebuild its header.
struct Candidate {
  std::shared_ptr<const JobTemplate> job;
  std::shared_ptr<const Group> group;
  uint64_t gen;
  uint32_t nonce, vi, stamp;
  double enq_host;
  uint32_t rt_enq;
  int nvar;
};

struct Batch {
  bool busy = false;
  std::shared_ptr<const JobTemplate> job;
  std::shared_ptr<const Group> group;
  uint64_t gen = 0;
  uint32_t epoch = 0, tag = 0;
  uint64_t count = 0;  // nonces per variant
  int nvar = 1;
  uint32_t consumed = 0;  // ring records already handled
  double enq_host = 0;    // monotonic seconds at enqueue
  uint32_t rt_enq = 0;    // device realtime (low 32 bits) estimated at enqueue
  bool started = false;
  hipStream_t stream = nullptr;  // this slot's stream (owned by the run; the slots may share one)
  Event start, done;
  DeviceMem<uint32_t> d_count;  // candidate counter (device memory)
  PinnedMem<uint32_t> h_count;  // pinned copy of the final count
  PinnedMem<HitRecord> ring;    // host-coherent records (host pointer)
  HitRecord* ring_dev = nullptr;  // the same records, device address
  DeviceMem<Sha256dVariant> d_vars;
  PinnedMem<Sha256dVariant> h_vars;
  uint64_t* h_clk = nullptr;  // this launch's clock probe (host-coherent; 0 until the probe ran)
  uint64_t* d_clk = nullptr;
  bool clk_pending = false;   // probe queued, its stamp not seen yet
  TraceId range = 0;
};

using JobPtr = std::shared_ptr<const JobTemplate>;
}  // namespace

GpuMiner::GpuMiner(int device, std::string device_id, uint64_t batch_nonces, int grid, size_t queue_cap, int sha_variants)
    : MinerBase(std::move(device_id), queue_cap), device_(device), batch_(normalize_batch(batch_nonces)), grid_(grid),
      sha_variants_(sha_variants) {}

GpuMiner::~GpuMiner() { stop(); }

void GpuMiner::start() {
  if (running_.exchange(true)) return;
  th_ = std::thread([this] {
    try {
      loop();
    } catch (const std::exception& ex) {
      // A device fault removes this device's stripe; the engine sees it in
      // stats().faulted and through the hashrate window.
      std::lock_guard<std::mutex> g(stats_mu_);
      stats_.faulted = true;
      stats_.error = ex.what();
    }
  });
}

void GpuMiner::stop() {
  if (!running_.exchange(false)) return;
  job_cv_.notify_all();
  if (th_.joinable()) th_.join();
}

// The device thread's state and HIP resources, alive for one start() .. stop() of its miner `m`.
//
// Release order. Everything is released on every exit, including a HIP error thrown mid-loop (device fault) with
// launches still queued, and nothing may be freed under a running kernel or copy. ~Run() therefore first stops and
// joins the verifier thread, then synchronises every search stream, then the control stream. After that the members
// go in reverse declaration order: device memory, pinned memory and events (the slots' included) are all declared
// BELOW the streams, so they are released before the search streams are destroyed, and the control stream goes last.
// A new buffer or event needs its declaration below the streams and nothing else.
struct GpuMiner::Run {
  explicit Run(GpuMiner& miner) : m(miner) {}

  GpuMiner& m;
  double t_phase = 0, t_loop = 0;  // start of the current start-up phase, and of the run

  // ---- streams: declared first, destroyed last
  Stream ctl;                // control stream: only when the CPU cannot store the abort word itself
  Stream search[kInflight];  // one per slot; [1] stays empty when the slots share [0] (OTEDAMA_SEARCH_STREAMS=1)

  // ---- device memory, pinned memory, events (and the raw addresses derived from them)
  bool host_abort = false;       // the CPU stores the abort word through the BAR
  DeviceMem<uint32_t> d_abort;   // uncached device word: the newest launch epoch that must keep running
  Event ref_ev;                  // device-timeline origin of hashes_done_at_s
  PinnedMem<uint64_t> h_rt;      // probe outputs (pinned, host-coherent): start-up probe, then one line per slot
  uint64_t* d_rt = nullptr;      // their device address
  DeviceMem<void> scratch;       // scrypt pad, allocated on the first scrypt job (one half per slot)
  DeviceMem<void> xbuf;
  DeviceMem<uint64_t> x11_h;     // X11 intermediate digests (8 u64 planes x batch, one set per slot)
  Batch slots[kInflight];

  // ---- configuration, fixed after start-up
  int cus = 256;
  ShaLayout max_layout;  // the largest SHA-256d layout this miner may use
  int scrypt_grid = 0;
  uint32_t scrypt_batch = 0;
  bool scrypt_halves = true, x11_overlap = true;
  bool cap_launches = true;  // OTEDAMA_LAUNCH_CAP "0": launches keep batch_ hashes (overflow tests)
  int grid_k = 0, grid_v = 0, grid_v2 = 0;

  // ---- device clock -> host clock
  double rt_offset = 0.0;  // host monotonic seconds at device realtime 0 (s_memrealtime, 100 MHz)
  double calib_rtt = 1e9;
  // Running: every launch's probe gives an upper bound on the offset (host time it was seen minus its device
  // time); the lowest bound of the last kClockWindowS seconds is the mapping in use.
  ClockBounds clk_bounds{kClockWindowS};

  // ---- search state
  std::shared_ptr<Group> group;  // current stripe group
  uint64_t cur_gen = ~0ull;
  SearchCursor cursor;  // variant-stripe position of the current group and the next nonce in it
  uint32_t epoch = 1, tag = 0;
  uint64_t epoch_gen = ~0ull;  // work generation the current epoch was opened for (0 = paused)
  bool switch_pending = false, first_switch = true;
  double switch_t0 = 0;
  double rate_hpms = 0;  // hashes per ms of completed full batches (for aborted-batch accounting)
  double scrypt_hash_s = 0.064;  // one lane's scrypt hash (= one full batch) on the device; refined per batch
  std::deque<int> fifo;  // in-flight slots, issue order
  BoundedWorkQueue<Candidate> vq{kVerifyCap};  // scrypt candidates awaiting host verification
  std::thread verifier;

  ~Run() {
    vq.stop(m.running_.load() ? ~size_t(0) : 64);  // shutting down: bound the work left (~1 ms each)
    if (verifier.joinable()) verifier.join();
    // in-flight batches are drained before anything is freed
    for (auto& s : search)
      if (s) (void)hipStreamSynchronize(s);
    if (ctl) (void)hipStreamSynchronize(ctl);
  }

  void phase(const char* name) {
    const double now = monotonic_seconds();
    std::lock_guard<std::mutex> g(m.stats_mu_);
    m.stats_.startup_ms.emplace_back(name, (now - t_phase) * 1e3);
    m.stats_.startup_rss_mb.emplace_back(name, resident_mb());
    t_phase = now;
  }

  void setup_streams() {
    const int ncu = gpu_cu_count(m.device_);
    cus = ncu > 0 ? ncu : 256;
    // Search streams: one per in-flight batch, so a launch's tail overlaps the next launch's first waves; with
    // OTEDAMA_SEARCH_STREAMS=1 the batches share one stream (one hardware queue less, 173 MiB of host memory).
    const char* ss_env = std::getenv("OTEDAMA_SEARCH_STREAMS");
    const bool one_stream = ss_env && std::atoi(ss_env) == 1;
    // OTEDAMA_RESERVE_CUS=<cu>,<cu>,...: the search streams get a CU mask without these CUs, so a kernel of another
    // process on the same GPU (a node rank's RCCL collective) finds a free slot at once instead of waiting for a
    // mining workgroup to finish (parallel/comm_probe.py measures the trade: the reserved CUs' share of the rate).
    CuMask mask;
    if (const char* rc_env = std::getenv("OTEDAMA_RESERVE_CUS")) mask = parse_reserved_cus(rc_env, cus);
    for (int i = 0; i < kInflight; ++i) {
      if (one_stream && i > 0) {
        slots[i].stream = search[0];
        continue;
      }
      if (mask.reserved > 0)
        OTD_HIP(hipExtStreamCreateWithCUMask(&search[i].h, uint32_t(mask.words.size()), mask.words.data()));
      else OTD_HIP(hipStreamCreateWithFlags(&search[i].h, hipStreamNonBlocking));
      slots[i].stream = search[i];
    }
    std::lock_guard<std::mutex> g(m.stats_mu_);
    m.stats_.reserved_cus = uint64_t(mask.reserved);
    m.stats_.search_streams = one_stream ? 1 : kInflight;
  }

  // The abort word must never wait behind a search kernel. The CPU stores it itself when it can map the word
  // (OTEDAMA_HOST_ABORT=0 forces the stream form). Otherwise the store goes on a high-priority stream: HIP
  // multiplexes streams of one priority onto GPU_MAX_HW_QUEUES (4) hardware queues, and with two search streams
  // plus torch's in the same process a control stream can land on a busy queue, where its write waits for a whole
  // 2^32-hash launch (the job switch grew from 0.3 ms to ~110 ms); high-priority streams come from a separate pool.
  // Every hardware queue costs a 173 MiB host mapping (tools/queue_rss.hip, profiles/r4/c_host_abort/rss.jsonl).
  void setup_abort_word() {
    hipStream_t s0 = slots[0].stream;
    OTD_HIP(hipExtMallocWithFlags(reinterpret_cast<void**>(&d_abort.h), 256, hipDeviceMallocUncached));
    // on a search stream: the first use of the null stream would give this process one more hardware queue
    // (tools/queue_rss.hip, profiles/r4/d_queues)
    OTD_HIP(hipMemsetAsync(d_abort, 0, 256, s0));
    OTD_HIP(hipStreamSynchronize(s0));
    const char* ha_env = std::getenv("OTEDAMA_HOST_ABORT");
    host_abort = !(ha_env && ha_env[0] == '0') && cpu_store_map(d_abort, 256);
    if (host_abort) {
      // Prove the path before trusting it: a CPU store must land in VRAM where the device (a copy on a search stream)
      // reads it back. Anything else (a mapping that swallows writes) falls back to the control stream.
      for (uint32_t probe : {0xA5C3E10Fu, 0u}) {
        __atomic_store_n(d_abort.h, probe, __ATOMIC_RELEASE);
        _mm_sfence();
        uint32_t back = ~probe;
        OTD_HIP(hipMemcpyAsync(&back, d_abort, sizeof back, hipMemcpyDeviceToHost, s0));
        OTD_HIP(hipStreamSynchronize(s0));
        if (back != probe) { host_abort = false; break; }
      }
      if (!host_abort) {  // the word must read 0 whichever path stores it from now on
        OTD_HIP(hipMemsetAsync(d_abort, 0, 256, s0));
        OTD_HIP(hipStreamSynchronize(s0));
      }
    }
    if (!host_abort) {
      int prio_lo = 0, prio_hi = 0;
      OTD_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
      OTD_HIP(hipStreamCreateWithPriority(&ctl.h, hipStreamNonBlocking, prio_hi));
    }
    std::lock_guard<std::mutex> g(m.stats_mu_);
    m.stats_.host_abort = host_abort;
  }

  // Control words, the per-slot buffers, and the launch geometry.
  void setup_buffers() {
    OTD_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_rt.h), 64 * (1 + kInflight),
                          hipHostMallocCoherent | hipHostMallocMapped));
    std::memset(h_rt, 0, 64 * (1 + kInflight));
    OTD_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_rt), h_rt, 0));
    for (int i = 0; i < kInflight; ++i) {
      slots[i].h_clk = h_rt.h + 8 * (1 + i);
      slots[i].d_clk = d_rt + 8 * (1 + i);
    }
    phase("control_words");
    max_layout = pick_layout(m.sha_variants_, kSha256dV2Group);
    for (auto& s : slots) {
      OTD_HIP(hipMalloc(&s.d_count.h, 64));
      OTD_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.h_count.h), 64, hipHostMallocDefault));
      OTD_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.ring.h), kHitCap * sizeof(HitRecord),
                            hipHostMallocCoherent | hipHostMallocMapped));
      std::memset(s.ring, 0, kHitCap * sizeof(HitRecord));
      OTD_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&s.ring_dev), s.ring, 0));
      OTD_HIP(hipEventCreate(&s.start.h));
      OTD_HIP(hipEventCreate(&s.done.h));
      if (max_layout.use_v) {
        OTD_HIP(hipMalloc(&s.d_vars.h, kSha256dV2Group * sizeof(Sha256dVariant)));
        OTD_HIP(hipHostMalloc(&s.h_vars.h, kSha256dV2Group * sizeof(Sha256dVariant), hipHostMallocDefault));
      }
    }
    phase("buffers");
    scrypt_grid = cus * 16;
    scrypt_batch = uint32_t(scrypt_grid) * 256u;
    const char* halves_env = std::getenv("OTEDAMA_SCRYPT_HALVES");
    scrypt_halves = !(halves_env && halves_env[0] == '0');
    const char* x11ov_env = std::getenv("OTEDAMA_X11_OVERLAP");
    x11_overlap = !(x11ov_env && x11ov_env[0] == '0');
    const char* cap_env = std::getenv("OTEDAMA_LAUNCH_CAP");
    cap_launches = !(cap_env && cap_env[0] == '0');
    // K-variant SHA-256d kernel: 16 blocks of 256 per CU (tools/bench_sha_k.py, profiles/r2/).
    grid_k = cus * 16;
    // Version-parallel kernel (8-waves/SIMD build): 64 blocks of 256 per CU (profiles/r2/sha_v).
    grid_v = cus * 64;
    // Two-chain kernel (4 waves/SIMD build): 128 blocks of 256 per CU (profiles/r2/sha_v2).
    grid_v2 = cus * 128;
    std::lock_guard<std::mutex> g(m.stats_mu_);
    m.stats_.scrypt_halves = scrypt_halves;
    m.stats_.x11_overlap = x11_overlap;
  }

  // Start-up: probes bracketed by the launch and the stream sync on an idle device; the tightest bracket wins.
  void probe_clock(hipStream_t on) {
    __atomic_store_n(h_rt.h, 0ull, __ATOMIC_RELEASE);
    const double t0 = monotonic_seconds();
    hipLaunchKernelGGL(otd_rt_probe, dim3(1), dim3(64), 0, on, d_rt);
    OTD_HIP(hipGetLastError());
    OTD_HIP(hipStreamSynchronize(on));
    const double t1 = monotonic_seconds();
    const uint64_t rt = __atomic_load_n(h_rt.h, __ATOMIC_ACQUIRE);
    if (rt && (t1 - t0) < calib_rtt) {
      rt_offset = 0.5 * (t0 + t1) - double(rt) / kRtHz;
      calib_rtt = t1 - t0;
      std::lock_guard<std::mutex> g(m.stats_mu_);
      m.stats_.clock_calib_rtt_us = (t1 - t0) * 1e6;
    }
  }

  void clock_seen(Batch& b) {
    const uint64_t rt = __atomic_load_n(b.h_clk, __ATOMIC_ACQUIRE);
    if (!rt) return;
    const double now = monotonic_seconds();  // after the load that saw the stamp: a valid upper bound
    b.clk_pending = false;
    rt_offset = clk_bounds.add(now, now - double(rt) / kRtHz);
    std::lock_guard<std::mutex> g(m.stats_mu_);
    m.stats_.clock_samples += 1;
  }

  void write_abort(uint32_t e) {
    if (host_abort) {
      __atomic_store_n(d_abort.h, e, __ATOMIC_RELEASE);
      _mm_sfence();  // out of the write-combining buffers and onto the bus now
    } else {
      OTD_HIP(hipStreamWriteValue32(ctl, d_abort, e, 0));
    }
  }

  // New work opens a new launch epoch and moves the device abort word: batches of older epochs stop at
  // their next poll. Called at the top of every loop trip and between hit verifications (a burst of scrypt hits
  // costs ~1 ms of CPU each and must not delay a switch).
  JobPtr check_epoch(uint64_t* gen_out) {
    uint64_t gen = 0;
    double set_at = 0;
    auto job = m.peek_job(&gen, &set_at);
    // A pause (no job) keeps the batches in flight running to their end (<= kInflight launches): moving the abort
    // word for it would skip the unsearched rest of those batches for good when the same work resumes, since the
    // cursor already moved past them. Only new work stops them.
    const uint64_t want_gen = job ? gen : epoch_gen;
    if (want_gen != epoch_gen) {
      epoch_gen = want_gen;
      ++epoch;
      if (!fifo.empty()) write_abort(epoch);
      if (job) { switch_pending = true; switch_t0 = set_at; }
    }
    if (gen_out) *gen_out = gen;
    return job;
  }

  void verify_push(const Candidate& b, uint32_t nonce, uint32_t vi, uint32_t stamp, bool stamped, const JobPtr& cur,
                   uint64_t cur_g, uint64_t* good, uint64_t* bad, const uint8_t* pre_hash = nullptr) {
    if (vi >= (uint32_t)b.nvar) { ++*bad; return; }
    uint8_t hdr[80];
    std::memcpy(hdr, b.group->header[vi], 80);
    store_le32(hdr + 76, nonce);
    ShareRecord r{};
    // A target-only update (same work generation) applies to batches in flight too: their hits are checked
    // against, and reported under, the current template (its target and control-plane epoch).
    const JobTemplate* tj = (cur && cur_g == b.gen) ? cur.get() : b.job.get();
    if (pre_hash) {
      std::memcpy(r.hash, pre_hash, 32);
      if (!le256_leq(r.hash, tj->target)) { ++*bad; return; }
    } else if (!verify_share(b.job->algo, hdr, tj->target, r.hash)) {
      ++*bad;
      return;
    }
    r.epoch = tj->epoch; r.job_id = tj->job_id; r.channel_id = tj->channel_id;
    r.nonce = nonce; r.ntime = b.group->ntime[vi]; r.version = b.group->version[vi]; r.extranonce2 = b.group->en2[vi];
    r.extranonce2_size = b.job->extranonce2_size; r.device_id = m.device_id_;
    r.found_at = monotonic_seconds();
    if (stamped) r.device_found_at = b.enq_host + double(int32_t(stamp - b.rt_enq)) / kRtHz;
    m.queue_.push(std::move(r));
    ++*good;
  }

  // The verifier thread. Scrypt candidates are re-hashed up to sixteen at a time (AVX-512 lanes, ~4x the scalar rate
  // per hash; AVX2 passes of eight without it), so a burst of easy-target hits drains in a fraction of the time.
  void verify_loop() {
    std::vector<Candidate> cs;
    cs.reserve(16);
    uint8_t hb[16][80], ho[16][32];
    const uint8_t* ip[16];
    uint8_t* op[16];
    for (int l = 0; l < 16; ++l) { ip[l] = hb[l]; op[l] = ho[l]; }
    while (cs.clear(), vq.pop_many(&cs, 16) > 0) {  // 0 once stopped and drained
      uint64_t good = 0, bad = 0, g = 0;
      auto cur = m.peek_job(&g, nullptr);
      int n = 0;
      for (const Candidate& c : cs) {
        if (c.job->algo != Algo::kScrypt || c.vi >= (uint32_t)c.nvar) continue;
        std::memcpy(hb[n], c.group->header[c.vi], 80);
        store_le32(hb[n] + 76, c.nonce);
        ++n;
      }
      if (n > 0) scrypt_1024_1_1_batch(n, ip, op);
      int l = 0;
      for (const Candidate& c : cs) {
        const bool batched = c.job->algo == Algo::kScrypt && c.vi < (uint32_t)c.nvar;
        verify_push(c, c.nonce, c.vi, c.stamp, true, cur, g, &good, &bad, batched ? ho[l] : nullptr);
        l += batched;
      }
      std::lock_guard<std::mutex> sg(m.stats_mu_);
      m.stats_.shares += good;
      m.stats_.rejected_candidates += bad;
    }
  }

  // Consume the published records of a batch; `final_n` = the batch's final count (after completion) or ~0u
  // while it runs. Returns the number of records handled.
  uint32_t drain_ring(Batch& b, uint32_t final_n, const JobPtr& cur, uint64_t cur_g) {
    const uint32_t limit = final_n == ~0u ? kHitCap : std::min(final_n, kHitCap);
    uint64_t good = 0, bad = 0, lost = 0, handled = 0;
    while (b.consumed < limit) {
      HitRecord* r = b.ring.h + b.consumed;
      const uint32_t tg = __atomic_load_n(&r->tag, __ATOMIC_ACQUIRE);
      if (tg != b.tag) {
        if (final_n == ~0u) break;  // not written yet
        ++lost;                     // completed launch without its record: count and skip (should not happen)
        ++b.consumed;
        continue;
      }
      const uint32_t nonce = __atomic_load_n(&r->nonce, __ATOMIC_RELAXED);
      const uint32_t vi = __atomic_load_n(&r->variant, __ATOMIC_RELAXED);
      const uint32_t stamp = __atomic_load_n(&r->stamp, __ATOMIC_RELAXED);
      if (b.job->algo == Algo::kScrypt) {
        // host scrypt costs ~1 ms per candidate: verified on the verifier thread so a burst of candidates never
        // holds up a job switch or the next launch. The queue is bounded: past kVerifyCap a candidate is refused
        // and counted (a share target far below the device's rate would otherwise grow it without limit).
        vq.push(Candidate{b.job, b.group, b.gen, nonce, vi, stamp, b.enq_host, b.rt_enq, b.nvar});
      } else {
        verify_push(Candidate{b.job, b.group, b.gen, 0, 0, 0, b.enq_host, b.rt_enq, b.nvar}, nonce, vi, stamp, true,
                    cur, cur_g, &good, &bad);
      }
      ++b.consumed;
      ++handled;
    }
    if (handled || lost) {
      const uint64_t refused = vq.refused(), peak = vq.peak();
      std::lock_guard<std::mutex> g(m.stats_mu_);
      m.stats_.shares += good;
      m.stats_.rejected_candidates += bad + lost;
      if (final_n == ~0u) m.stats_.ring_hits += handled;
      m.stats_.verify_dropped = refused;
      m.stats_.verify_queue_peak = peak;
    }
    return uint32_t(handled);
  }

  void finish(Batch& b, const JobPtr& cur, uint64_t cur_g) {
    trace_stop(b.range);
    const uint32_t n = *b.h_count.h;
    drain_ring(b, n, cur, cur_g);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, b.start, b.done);
    float done_ms = 0;  // device-timeline completion of this batch, for exact-window hash rates
    const bool have_done = hipEventElapsedTime(&done_ms, ref_ev, b.done) == hipSuccess;
    const uint64_t full = b.count * uint64_t(b.nvar);
    const bool aborted = int32_t(epoch - b.epoch) > 0;  // a newer epoch was opened after this batch
    const uint64_t done_hashes = aborted ? aborted_launch_hashes(full, rate_hpms, ms) : full;
    if (!aborted && ms > 0) rate_hpms = update_rate_hpms(rate_hpms, full, ms);
    if (!aborted && ms > 0 && b.job && b.job->algo == Algo::kScrypt)
      scrypt_hash_s = update_scrypt_hash_s(scrypt_hash_s, ms);
    std::lock_guard<std::mutex> g(m.stats_mu_);
    if (n > kHitCap) {  // the kernel counted these candidates but had no ring slot left to publish them
      if (m.stats_.ring_overflow == 0)
        std::fprintf(stderr, "otedama: %s: launch found %u candidates, hit ring holds %u: %u lost (counted in "
                     "ring_overflow)\n", m.device_id_.c_str(), n, kHitCap, n - kHitCap);
      m.stats_.ring_overflow += n - kHitCap;
    }
    m.stats_.hashes += done_hashes;
    if (have_done) m.stats_.hashes_done_at_s = std::max(m.stats_.hashes_done_at_s, double(done_ms) * 1e-3);
    m.stats_.candidates += n;
    m.stats_.busy_seconds += ms * 1e-3;
    m.stats_.launches += 1;
    m.stats_.inflight = fifo.size() - 1;  // both callers take this batch off the fifo next
    if (aborted) m.stats_.aborted_launches += 1;
    if (b.nvar > 1) m.stats_.variant_launches += 1;
    b.busy = false;
    b.job.reset();
    b.group.reset();
  }

  std::shared_ptr<Group> build_group(const JobPtr& job, uint64_t gen) {
    auto gp = std::make_shared<Group>();
    const uint64_t k = cursor.k;
    gp->gen = gen;
    gp->k = k;
    gp->nvar = 1;
    const uint64_t v = job->variant_start + k * job->variant_stride;
    job->variant_header(v, gp->header[0], &gp->version[0], &gp->ntime[0], &gp->en2[0]);
    if (job->algo != Algo::kSha256d || max_layout.nvar <= 1) return gp;
    // Consecutive stripe positions whose headers differ only in block 1 (version rolling) share block 2: up to
    // 128 (two-chain version-parallel kernel), 64 (one chain) or K (per-lane K-variant kernel). A group is
    // all-or-nothing per layout and depends only on (work, k), so all its launches use one kernel.
    int kv = 1;
    while (kv < max_layout.nvar) {
      const uint64_t vk = job->variant_start + (k + kv) * job->variant_stride;
      if (vk >= job->variant_space()) break;
      job->variant_header(vk, gp->header[kv], &gp->version[kv], &gp->ntime[kv], &gp->en2[kv]);
      if (std::memcmp(gp->header[kv] + 64, gp->header[0] + 64, 12) != 0) break;
      ++kv;
    }
    const ShaLayout lay = pick_layout(m.sha_variants_, kv);
    gp->nvar = lay.nvar;
    gp->use_v = lay.use_v;
    if (gp->use_v) {
      const uint8_t* hs[kSha256dV2Group];
      for (int j = 0; j < gp->nvar; ++j) hs[j] = gp->header[j];
      if (!sha256d_prepare_v(hs, gp->nvar, job->target, &gp->v_params, gp->v_table))
        throw std::runtime_error("sha256d_prepare_v");
      gp->v_params.occupancy8 = gp->nvar == kSha256dV2Group ? 0 : 1;
    }
    return gp;
  }

  uint64_t launch_cap(const JobTemplate& job) const {
    return launch_cap_hashes(load_le32(job.target + 28), cap_launches);
  }

  // One launch_* per kernel family: queue the search kernel of batch `s` at the cursor on its stream; each returns
  // the launch's nonces per variant.
  uint64_t launch_scrypt(Batch& s, const JobTemplate& job, const HitSink& sink) {
    if (!scratch) {
      OTD_HIP(hipMalloc(&scratch.h, scrypt_scratch_bytes(scrypt_grid, kScryptGap)));
      OTD_HIP(hipMalloc(&xbuf.h, uint64_t(scrypt_batch) * 128));
    }
    ScryptParams p;
    scrypt_prepare(group->header[0], job.target, &p);
    const int slot_i = int(&s - slots);
    // halves: each slot owns half the pad / X buffer and half the grid (the two run side by side)
    const int grid = scrypt_halves ? scrypt_grid / 2 : scrypt_grid;
    const uint32_t lanes = scrypt_halves ? scrypt_batch / 2 : scrypt_batch;
    char* pad = static_cast<char*>(scratch.h) +
                (scrypt_halves ? uint64_t(slot_i) * scrypt_scratch_bytes(grid, kScryptGap) : 0);
    char* xb = static_cast<char*>(xbuf.h) + (scrypt_halves ? uint64_t(slot_i) * lanes * 128ull : 0);
    const uint64_t count = launch_count(LaunchKind::kScrypt, m.batch_, launch_cap(job), 1, lanes, cursor.nonce_off);
    OTD_HIP(launch_scrypt_search(p, uint32_t(cursor.nonce_off), uint32_t(count), xb, pad, kScryptGap, sink, grid,
                                 s.stream));
    return count;
  }

  uint64_t launch_x11(Batch& s, const JobTemplate& job, const HitSink& sink) {
    if (!x11_h) OTD_HIP(hipMalloc(&x11_h.h, uint64_t(kX11Batch) * 64 * (x11_overlap ? kInflight : 1)));
    X11Params p;
    x11_prepare(group->header[0], job.target, &p);
    const int slot_i = int(&s - slots);
    const uint64_t count = launch_count(LaunchKind::kX11, m.batch_, launch_cap(job), 1, kX11Batch, cursor.nonce_off);
    uint64_t* H = x11_h.h + (x11_overlap ? uint64_t(slot_i) * kX11Batch * 8 : 0);
    OTD_HIP(x11_launch_chain(p, uint32_t(cursor.nonce_off), H, kX11Batch, uint32_t(count), &sink, s.stream));
    return count;
  }

  uint64_t launch_sha_v(Batch& s, const JobTemplate& job, const HitSink& sink) {
    const bool two = group->nvar == kSha256dV2Group;
    Sha256dParamsV vp = group->v_params;
    // The table is cached per (work, group) but a target-only update (SV2 SetTarget, V1 set_difficulty) keeps
    // the work generation: the share filter follows the job's current target on every launch.
    vp.target_hi = load_le32(job.target + 28);
    const size_t table_bytes = size_t(group->nvar) * sizeof(Sha256dVariant);
    std::memcpy(s.h_vars, group->v_table, table_bytes);
    OTD_HIP(hipMemcpyAsync(s.d_vars, s.h_vars, table_bytes, hipMemcpyHostToDevice, s.stream));
    const uint64_t count =
        launch_count(LaunchKind::kVersionParallel, m.batch_, launch_cap(job), group->nvar, 0, cursor.nonce_off);
    OTD_HIP(launch_sha256d_search_v(vp, s.d_vars, uint32_t(cursor.nonce_off), count, sink, two ? grid_v2 : grid_v,
                                    s.stream, 256, two ? 2 : 1));
    return count;
  }

  uint64_t launch_sha_k(Batch& s, const JobTemplate& job, const HitSink& sink) {
    Sha256dParamsK p;
    const uint8_t* hs[kSha256dMaxK];
    for (int j = 0; j < group->nvar; ++j) hs[j] = group->header[j];
    if (!sha256d_prepare_k(hs, group->nvar, job.target, &p)) throw std::runtime_error("sha256d_prepare_k");
    const uint64_t count =
        launch_count(LaunchKind::kVariantK, m.batch_, launch_cap(job), group->nvar, 0, cursor.nonce_off);
    OTD_HIP(launch_sha256d_search_k(p, uint32_t(cursor.nonce_off), count, sink, grid_k, s.stream));
    return count;
  }

  uint64_t launch_sha_single(Batch& s, const JobTemplate& job, const HitSink& sink) {
    Sha256dParams p;
    sha256d_prepare(group->header[0], job.target, &p);
    const uint64_t count = launch_count(LaunchKind::kSingle, m.batch_, launch_cap(job), 1, 0, cursor.nonce_off);
    OTD_HIP(launch_sha256d_search(p, uint32_t(cursor.nonce_off), count, sink, m.grid_, s.stream));
    return count;
  }

  // Queue the next launch on slot `s`. On its stream, in order: clear the candidate count, record `start`, the clock
  // probe, (version-parallel only) the variant table's copy to the device, the search kernel, the count's copy back,
  // record `done`.
  void enqueue(Batch& s, const JobPtr& job, uint64_t gen, const Batch* prev) {
    hipStream_t stream = s.stream;
    if (!group || group->gen != gen || group->k != cursor.k) group = build_group(job, gen);
    s.job = job;
    s.group = group;
    s.gen = gen;
    s.nvar = group->nvar;
    s.epoch = epoch;
    s.tag = ++tag == 0 ? ++tag : tag;
    s.consumed = 0;
    s.started = false;
    s.range = trace_start(job->algo == Algo::kScrypt ? "otd.scrypt.batch"
                          : job->algo == Algo::kX11  ? "otd.x11.batch"
                                                     : "otd.sha256d.batch");
    HitSink sink;
    sink.out = s.d_count;
    sink.ring = s.ring_dev;
    sink.abort = d_abort;
    sink.cap = kHitCap;
    sink.tag = s.tag;
    sink.epoch = s.epoch;
    sink.words = 2;
    // scrypt pad / X11 digests are shared by the batches: chain them; SHA-256d batches overlap freely
    const bool shared_buf = (job->algo == Algo::kScrypt && !scrypt_halves) || (job->algo == Algo::kX11 && !x11_overlap);
    if (prev && prev->busy && shared_buf) OTD_HIP(hipStreamWaitEvent(stream, prev->done, 0));
    OTD_HIP(hipMemsetAsync(s.d_count, 0, 64, stream));
    OTD_HIP(hipEventRecord(s.start, stream));
    __atomic_store_n(s.h_clk, 0ull, __ATOMIC_RELEASE);
    hipLaunchKernelGGL(otd_rt_probe, dim3(1), dim3(64), 0, stream, s.d_clk);
    OTD_HIP(hipGetLastError());
    s.clk_pending = true;
    s.enq_host = monotonic_seconds();
    s.rt_enq = uint32_t(uint64_t((s.enq_host - rt_offset) * kRtHz));
    s.count = job->algo == Algo::kScrypt ? launch_scrypt(s, *job, sink)
              : job->algo == Algo::kX11  ? launch_x11(s, *job, sink)
              : group->use_v             ? launch_sha_v(s, *job, sink)
              : group->nvar > 1          ? launch_sha_k(s, *job, sink)
                                         : launch_sha_single(s, *job, sink);
    OTD_HIP(hipMemcpyAsync(s.h_count, s.d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    OTD_HIP(hipEventRecord(s.done, stream));
    s.busy = true;
    cursor.advance(s.count, group->nvar);
    std::lock_guard<std::mutex> g(m.stats_mu_);
    m.stats_.variant_epoch = job->epoch;
    m.stats_.launch_hashes = s.count * uint64_t(s.nvar);
    m.stats_.variant_next = cursor.variant_next(job->variant_start, job->variant_stride, group->nvar);
    m.stats_.cursor_k = cursor.k;
    m.stats_.cursor_nonce_off = cursor.nonce_off;
    m.stats_.inflight = fifo.size() + 1;  // fill() puts this batch on the fifo next
    m.stats_.idle = false;
  }

  bool retire_completed(const JobPtr& job, uint64_t gen) {
    bool progressed = false;
    for (auto it = fifo.begin(); it != fifo.end();) {
      Batch& b = slots[*it];
      const hipError_t q = hipEventQuery(b.done);
      if (q == hipErrorNotReady) { ++it; continue; }
      OTD_HIP(q);
      if (!b.started) b.started = true;
      finish(b, job, gen);
      it = fifo.erase(it);
      progressed = true;
    }
    return progressed;
  }

  void record_switch(const JobPtr& job) {
    for (int i : fifo) {
      Batch& b = slots[i];
      if (b.epoch != epoch) continue;
      const hipError_t q = hipEventQuery(b.start);
      if (q == hipErrorNotReady) break;
      OTD_HIP(q);
      b.started = true;
      const double ms = (monotonic_seconds() - switch_t0) * 1e3;
      switch_pending = false;
      std::lock_guard<std::mutex> g(m.stats_mu_);
      MinerStats& st = m.stats_;
      if (first_switch) {
        first_switch = false;
        double before = 0;  // the start-up phases, so the wait is what is left of loop start -> set_job
        for (const auto& kv : st.startup_ms) before += kv.second;
        st.startup_ms.emplace_back("wait_first_job", std::max(0.0, (switch_t0 - t_loop) * 1e3 - before));
        st.startup_ms.emplace_back("first_batch", ms);
      }
      st.job_switches += 1;
      st.last_job_switch_ms = ms;
      st.job_switch_ms.push_back(ms);
      if (st.job_switch_ms.size() > 64) st.job_switch_ms.erase(st.job_switch_ms.begin());
      st.work_started.emplace_back(job ? job->epoch : 0, switch_t0 + ms * 1e-3);
      if (st.work_started.size() > 64) st.work_started.erase(st.work_started.begin());
      break;
    }
  }

  // The cursor is past the last variant of this device's stripe.
  bool stripe_exhausted(const JobTemplate& job) const {
    return job.variant_start + cursor.k * job.variant_stride >= job.variant_space();
  }

  bool fill(const JobPtr& job, uint64_t gen) {
    bool progressed = false;
    while (job && (int)fifo.size() < kInflight) {
      if (stripe_exhausted(*job)) break;  // wait for fresh work
      // scrypt halves: keep the two in flight half a hash apart (the second waits until the first is half way), so
      // their phase-boundary polls interleave; re-established after every switch
      if (job->algo == Algo::kScrypt && scrypt_halves && fifo.size() == 1) {
        const Batch& only = slots[fifo.front()];
        if (only.epoch == epoch && monotonic_seconds() - only.enq_host < 0.5 * scrypt_hash_s) break;
      }
      int free_slot = -1;
      for (int i = 0; i < kInflight; ++i)
        if (!slots[i].busy) { free_slot = i; break; }
      if (free_slot < 0) break;
      enqueue(slots[free_slot], job, gen, fifo.empty() ? nullptr : &slots[fifo.back()]);
      fifo.push_back(free_slot);
      progressed = true;
    }
    return progressed;
  }

  // Let the batches in flight finish (abort them first: the miner is stopping).
  void drain_inflight() {
    if (!fifo.empty()) {
      ++epoch;
      try {
        write_abort(epoch);
      } catch (const std::exception&) {
        // a faulted device: the drain below reports it
      }
    }
    uint64_t gen = 0;
    auto job = m.peek_job(&gen, nullptr);
    while (!fifo.empty()) {
      Batch& b = slots[fifo.front()];
      OTD_HIP(hipEventSynchronize(b.done));
      finish(b, job, gen);
      fifo.pop_front();
    }
  }

  void run() {
    trace_name_thread(("otedama-" + m.device_id_).c_str());
    t_phase = t_loop = monotonic_seconds();
    OTD_HIP(hipSetDevice(m.device_));
    OTD_HIP(hipFree(nullptr));  // force runtime / context creation here so the phase below is honest
    phase("hip_set_device");
    setup_streams();
    setup_abort_word();
    phase("streams");
    setup_buffers();
    for (int t = 0; t < 8; ++t) probe_clock(slots[0].stream);
    phase("clock_calibration");
    OTD_HIP(hipEventCreate(&ref_ev.h));
    OTD_HIP(hipEventRecord(ref_ev, slots[0].stream));  // before any search: the device-timeline origin
    verifier = std::thread([this] { verify_loop(); });

    while (m.running_.load()) {
      uint64_t gen = 0;
      auto job = check_epoch(&gen);
      if (job && gen != cur_gen) { cur_gen = gen; cursor.reset(); }
      // 1) hits of the batches in flight, oldest first, and the clock stamps of launches that just started
      bool progressed = false;
      for (int i : fifo)
        if (slots[i].clk_pending) clock_seen(slots[i]);
      for (int i : fifo) progressed |= drain_ring(slots[i], ~0u, job, gen) > 0;
      // 2) retire completed batches (the two streams may complete out of issue order)
      progressed |= retire_completed(job, gen);
      // 3) job-switch time: set_job -> the first batch of the new epoch running on the device
      if (switch_pending) record_switch(job);
      // 4) keep kInflight batches queued
      progressed |= fill(job, gen);
      // 5) nothing in flight and, for the job this trip looked at, nothing to queue: everything up to the cursor has
      // been searched and its hits handed on (stats().idle; set_job() clears it again)
      if (fifo.empty() && (!job || stripe_exhausted(*job))) m.mark_idle(job);
      if (!progressed) {
        if (!job && fifo.empty()) {
          uint64_t g2 = 0;
          (void)m.current_job(&g2);  // waits (<= 10 ms) for work instead of spinning
        } else {
          std::this_thread::sleep_for(kIdlePoll);
        }
      }
    }
    drain_inflight();
  }
};

void GpuMiner::loop() { Run(*this).run(); }

int gpu_device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

std::string gpu_arch_name(int device) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return "";
  return prop.gcnArchName;
}

int gpu_cu_count(int device) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return 0;
  return prop.multiProcessorCount;
}

}  // namespace otedama
