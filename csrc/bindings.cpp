// pybind11 bindings: `otedama_amd._native`.
//
// Exposes the host SHA-256 / scrypt primitives, the per-job folding for the
// gfx950 kernels, raw kernel launches (for torch-owned buffers / streams), and
// the native GpuMiner / CpuMiner runtime objects. The module function at the end
// is the list of bind_* functions; the helpers they share come first.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <atomic>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <tuple>

#include "otedama/aead.h"
#include "otedama/job.h"
#include "otedama/runtime.h"
#include "otedama/trace.h"
#include "otedama/sha256.h"
#include "otedama/sv2_frame.h"
#include "otedama/clock_bounds.h"
#include "otedama/hip_check.h"
#include "otedama/hitsink.h"
#include "otedama/launch_plan.h"
#include "otedama/search_launch.h"
#include "otedama/share_job.h"
#include "otedama/work_queue.h"
#include "otedama/x11.h"
#include "otedama/x11_launch.h"

namespace py = pybind11;
using namespace otedama;

namespace {

std::string need(const py::bytes& b, size_t n, const char* what) {
  std::string s = b;
  if (s.size() != n) throw std::invalid_argument(std::string(what) + ": expected " + std::to_string(n) + " bytes");
  return s;
}

py::bytes to_bytes(const uint8_t* p, size_t n) { return py::bytes(reinterpret_cast<const char*>(p), n); }

const uint8_t* u8(const std::string& s) { return reinterpret_cast<const uint8_t*>(s.data()); }
uint8_t* u8(std::string& s) { return reinterpret_cast<uint8_t*>(&s[0]); }

// Kernel parameter blocks and job blocks cross to Python as opaque bytes and are passed back in.
template <class T>
py::bytes pod_bytes(const T& v) { return py::bytes(reinterpret_cast<const char*>(&v), sizeof v); }
template <class T>
T pod_from(const py::bytes& b, const char* what) {
  const std::string s = need(b, sizeof(T), what);
  T v;
  std::memcpy(&v, s.data(), sizeof v);
  return v;
}
ShareJobBlock job_block_from(const py::bytes& b) { return pod_from<ShareJobBlock>(b, "job_block"); }

struct HeaderTarget {  // an 80-byte header and a 32-byte target, checked in that order
  std::string h, t;
  HeaderTarget(const py::bytes& hb, const py::bytes& tb) : h(need(hb, 80, "header")), t(need(tb, 32, "target")) {}
  const uint8_t* header() const { return u8(h); }
  const uint8_t* target() const { return u8(t); }
};

// sha256d_prepare, scrypt_prepare, x11_prepare: header and target in, the kernel's parameter block out.
template <class P, void (*Prepare)(const uint8_t*, const uint8_t*, P*)>
py::bytes prepare_params(const py::bytes& h, const py::bytes& t) {
  const HeaderTarget ht(h, t);
  P p;
  Prepare(ht.header(), ht.target(), &p);
  return pod_bytes(p);
}

// The header pointers of sha256d_prepare_k / _v: `store` keeps the strings alive.
std::vector<const uint8_t*> header_ptrs(const py::list& headers, std::vector<std::string>* store) {
  for (auto& h : headers) store->push_back(need(h.cast<py::bytes>(), 80, "header"));
  std::vector<const uint8_t*> ptrs;
  for (auto& h : *store) ptrs.push_back(u8(h));
  return ptrs;
}

std::vector<ShareRec> share_recs_from(const py::bytes& records) {
  const std::string rs = records;
  if (rs.size() % sizeof(ShareRec)) throw std::invalid_argument("records: expected a multiple of 32 bytes");
  std::vector<ShareRec> recs(rs.size() / sizeof(ShareRec));
  if (!recs.empty()) std::memcpy(recs.data(), rs.data(), rs.size());
  return recs;
}

// bytes, a bytearray or a memoryview, as contiguous bytes: a caller that packs into a bytearray can wipe its
// secrets afterwards.
py::buffer_info byte_view(const py::buffer& b, const char* what) {
  py::buffer_info info = b.request();
  if (info.ndim != 1 || info.itemsize != 1 || (info.size && info.strides[0] != 1))
    throw std::invalid_argument(std::string(what) + ": expected contiguous bytes");
  return info;
}

// For input that holds scalars or keys and work long enough to give up the GIL: out_size(in, size) checks the
// caller's bytes and sizes the result (it throws on bad input); run(in, size, out, out_size) then works without the
// GIL on a private copy, since the caller's buffer may change once the GIL is gone, and the copy is wiped after.
template <class Size, class Run>
py::bytes on_wiped_copy(const py::buffer& buf, const char* what, Size&& out_size, Run&& run) {
  const py::buffer_info info = byte_view(buf, what);
  std::string out(out_size(static_cast<const uint8_t*>(info.ptr), size_t(info.size)), '\0');
  std::string in(static_cast<const char*>(info.ptr), size_t(info.size));
  {
    py::gil_scoped_release r;
    run(u8(in), in.size(), u8(out), out.size());
  }
  volatile char* wipe = &in[0];
  for (size_t i = 0; i < in.size(); ++i) wipe[i] = 0;
  return py::bytes(out);
}

// Kernel launches: torch owns the buffers and the streams, so pointers and the stream arrive as integers, nothing
// synchronises, and a HIP error is thrown as std::runtime_error (hip_check).
struct dev {  // a device address from Python, as whatever pointer type the launch declares
  uintptr_t a;
  template <class T>
  operator T*() const { return reinterpret_cast<T*>(a); }
};
hipStream_t stream_of(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }
// hip_check with the launch's name as the place: "HIP error <string> at <launch name>"
#define LAUNCH(fn, ...) hip_check(fn(__VA_ARGS__), #fn)

// The ops API's sink: hits go to the legacy device-memory slots after out[0]; no abort word.
HitSink ops_sink(uintptr_t out, uint32_t cap, uint32_t words) {
  HitSink s;
  s.out = dev{out};
  s.cap = cap;
  s.words = words;
  return s;
}

std::shared_ptr<JobTemplate> make_job(const py::dict& d) {
  auto j = std::make_shared<JobTemplate>();
  auto get = [&](const char* k) -> py::object {
    if (d.contains(k)) return py::object(d[k]);
    return py::none();
  };
  std::string hdr = need(d["header"].cast<py::bytes>(), 80, "header");
  std::memcpy(j->header, hdr.data(), 80);
  std::string tgt = need(d["target"].cast<py::bytes>(), 32, "target");
  std::memcpy(j->target, tgt.data(), 32);
  if (!get("epoch").is_none()) j->epoch = d["epoch"].cast<uint64_t>();
  if (!get("job_id").is_none()) j->job_id = d["job_id"].cast<std::string>();
  if (!get("channel_id").is_none()) j->channel_id = d["channel_id"].cast<uint32_t>();
  if (!get("algo").is_none()) {
    auto a = d["algo"].cast<std::string>();
    if (a == "sha256d") j->algo = Algo::kSha256d;
    else if (a == "scrypt") j->algo = Algo::kScrypt;
    else if (a == "x11") j->algo = Algo::kX11;
    else throw std::invalid_argument("unsupported algo for the native miner: " + a);
  }
  if (!get("version_mask").is_none()) j->version_mask = d["version_mask"].cast<uint32_t>();
  if (!get("ntime_roll").is_none()) j->ntime_roll = d["ntime_roll"].cast<uint32_t>();
  if (!get("coinb1").is_none()) {
    j->has_coinbase = true;
    std::string c1 = d["coinb1"].cast<py::bytes>(), c2 = d["coinb2"].cast<py::bytes>();
    std::string e1 = d["extranonce1"].cast<py::bytes>();
    j->coinb1.assign(c1.begin(), c1.end());
    j->coinb2.assign(c2.begin(), c2.end());
    j->extranonce1.assign(e1.begin(), e1.end());
    j->extranonce2_size = d["extranonce2_size"].cast<uint32_t>();
    for (auto& br : d["merkle_branches"].cast<py::list>()) {
      std::string b = br.cast<py::bytes>();
      j->merkle_branches.emplace_back(b.begin(), b.end());
    }
  }
  if (!get("variant_start").is_none()) j->variant_start = d["variant_start"].cast<uint64_t>();
  if (!get("variant_stride").is_none()) j->variant_stride = d["variant_stride"].cast<uint64_t>();
  if (j->variant_stride == 0) j->variant_stride = 1;
  return j;
}

py::list shares_to_list(std::vector<ShareRecord>&& v) {
  py::list out;
  for (auto& s : v) {
    py::dict d;
    d["epoch"] = s.epoch;
    d["job_id"] = s.job_id;
    d["channel_id"] = s.channel_id;
    d["nonce"] = s.nonce;
    d["ntime"] = s.ntime;
    d["version"] = s.version;
    d["extranonce2"] = s.extranonce2;
    d["extranonce2_size"] = s.extranonce2_size;
    d["hash"] = to_bytes(s.hash, 32);
    d["device_id"] = s.device_id;
    d["found_at"] = s.found_at;
    d["device_found_at"] = s.device_found_at;
    out.append(d);
  }
  return out;
}

py::dict stats_to_dict(const MinerStats& s) {
  py::dict d;
  d["hashes"] = s.hashes;
  d["candidates"] = s.candidates;
  d["shares"] = s.shares;
  d["dropped"] = s.dropped;
  d["launches"] = s.launches;
  d["rejected_candidates"] = s.rejected_candidates;
  d["variant_launches"] = s.variant_launches;
  d["busy_seconds"] = s.busy_seconds;
  d["faulted"] = s.faulted;
  d["error"] = s.error;
  d["variant_next"] = s.variant_next;
  d["variant_epoch"] = s.variant_epoch;
  d["cursor_k"] = s.cursor_k;
  d["cursor_nonce_off"] = s.cursor_nonce_off;
  d["inflight"] = s.inflight;
  d["idle"] = s.idle;
  d["job_switches"] = s.job_switches;
  d["last_job_switch_ms"] = s.last_job_switch_ms;
  d["job_switch_ms"] = s.job_switch_ms;
  d["work_started"] = s.work_started;
  d["reserved_cus"] = s.reserved_cus;
  d["ring_overflow"] = s.ring_overflow;
  d["verify_dropped"] = s.verify_dropped;
  d["verify_queue_peak"] = s.verify_queue_peak;
  d["launch_hashes"] = s.launch_hashes;
  d["aborted_launches"] = s.aborted_launches;
  d["ring_hits"] = s.ring_hits;
  d["clock_calib_rtt_us"] = s.clock_calib_rtt_us;
  d["clock_samples"] = s.clock_samples;
  d["host_abort"] = s.host_abort;
  d["search_streams"] = s.search_streams;
  d["scrypt_halves"] = s.scrypt_halves;
  d["x11_overlap"] = s.x11_overlap;
  d["hashes_done_at_s"] = s.hashes_done_at_s;
  {
    py::dict ph;
    for (const auto& kv : s.startup_ms) ph[py::str(kv.first)] = kv.second;
    d["startup_ms"] = ph;
    py::dict rs;
    for (const auto& kv : s.startup_rss_mb) rs[py::str(kv.first)] = kv.second;
    d["startup_rss_mb"] = rs;
  }
  return d;
}

// ---- host hashes and AEAD ----
void bind_host_hashes(py::module_& m) {
  m.def("cpu_has_sha_ni", &cpu_has_sha_ni);
  m.def("sha256", [](const py::bytes& b) {
    std::string s = b; uint8_t o[32];
    sha256(u8(s), s.size(), o);
    return to_bytes(o, 32);
  });
  m.def("sha256d", [](const py::bytes& b) {
    std::string s = b; uint8_t o[32];
    { py::gil_scoped_release r; sha256d(u8(s), s.size(), o); }
    return to_bytes(o, 32);
  });
  m.def("hmac_sha256", [](const py::bytes& k, const py::bytes& msg) {
    std::string ks = k, ms = msg; uint8_t o[32];
    hmac_sha256(u8(ks), ks.size(), u8(ms), ms.size(), o);
    return to_bytes(o, 32);
  });
  m.def("aead_seal", [](int kind, const py::bytes& key, const py::bytes& nonce, const py::bytes& plain,
                        const py::bytes& aad) {
    std::string out = aead_seal(static_cast<AeadKind>(kind), key, nonce, plain, aad);
    return py::bytes(out);
  }, py::arg("kind"), py::arg("key"), py::arg("nonce"), py::arg("plain"), py::arg("aad") = py::bytes());
  m.def("aead_open", [](int kind, const py::bytes& key, const py::bytes& nonce, const py::bytes& sealed,
                        const py::bytes& aad) -> py::object {
    std::string out;
    if (!aead_open(static_cast<AeadKind>(kind), key, nonce, sealed, aad, &out)) return py::none();
    return py::bytes(out);
  }, py::arg("kind"), py::arg("key"), py::arg("nonce"), py::arg("sealed"), py::arg("aad") = py::bytes());
  m.attr("AEAD_AES256GCM") = 0;
  m.attr("AEAD_CHACHA20POLY1305") = 1;
  m.def("scrypt_1024_1_1_batch", [](const std::vector<py::bytes>& hs) {
    std::vector<std::string> in;
    for (const auto& h : hs) in.push_back(need(h, 80, "header"));
    std::vector<std::array<uint8_t, 32>> out(in.size());
    std::vector<const uint8_t*> ip;
    std::vector<uint8_t*> op;
    for (size_t i = 0; i < in.size(); ++i) {
      ip.push_back(u8(in[i]));
      op.push_back(out[i].data());
    }
    {
      py::gil_scoped_release r;
      scrypt_1024_1_1_batch(int(in.size()), ip.data(), op.data());
    }
    py::list res;
    for (const auto& o : out) res.append(to_bytes(o.data(), 32));
    return res;
  });
  m.def("scrypt_1024_1_1", [](const py::bytes& h) {
    std::string s = need(h, 80, "header"); uint8_t o[32];
    { py::gil_scoped_release r; scrypt_1024_1_1(u8(s), o); }
    return to_bytes(o, 32);
  });
  m.attr("X11_STAGES") = kX11StageCount;
  m.def("x11", [](const py::bytes& msg) {
    std::string s = msg; uint8_t o[32];
    { py::gil_scoped_release r; x11::x11(u8(s), s.size(), o, nullptr); }
    return to_bytes(o, 32);
  }, py::arg("msg"));
  m.def("x11_trace", [](const py::bytes& msg) {
    std::string s = msg; uint8_t o[32], t[64 * kX11StageCount];
    x11::x11(u8(s), s.size(), o, t);
    return to_bytes(t, sizeof t);
  }, py::arg("msg"), "The 11 intermediate 64-byte digests of the X11 chain, concatenated.");
  m.def("x11_stage", [](int i, const py::bytes& msg) {
    if (i < 0 || i >= kX11StageCount) throw std::invalid_argument("stage must be in [0, 11)");
    std::string s = msg; uint8_t o[64];
    x11::stage(i, u8(s), s.size(), o);
    return to_bytes(o, 64);
  }, py::arg("stage"), py::arg("msg"));
  m.def("x11_luffa_sbox_selfcheck", &x11::luffa_sbox_selfcheck);
  m.def(
      "sv2_scan",
      [](py::buffer b, uint32_t max_frame) {
        py::buffer_info info = b.request();
        if (info.itemsize != 1 || info.ndim != 1) throw std::invalid_argument("sv2_scan: need a contiguous byte buffer");
        const size_t n = (size_t)info.size;
        if (n > 0xFFFFFFFFull) throw std::invalid_argument("sv2_scan: buffer larger than 4 GiB");
        // Upper bound on frames in n bytes: every frame has a 6-byte header.
        std::vector<Sv2FrameRec> recs(n / kSv2HeaderSize + 1);
        size_t consumed = 0, k = 0;
        int status = kSv2Ok;
        {
          py::gil_scoped_release nogil;
          k = sv2_scan(static_cast<const uint8_t*>(info.ptr), n, max_frame, recs.data(), recs.size(), &consumed,
                       &status);
        }
        py::list frames(k);
        for (size_t i = 0; i < k; ++i) {
          const Sv2FrameRec& r = recs[i];
          frames[i] = py::make_tuple(r.extension_type, r.msg_type, r.offset, r.length);
        }
        return py::make_tuple(frames, consumed, status);
      },
      py::arg("buf"), py::arg("max_frame"),
      "Split complete SV2 frames: ([(extension_type, msg_type, payload_offset, payload_length)], consumed, status)");
  m.def("cpu_scan_sha256d", [](const py::bytes& h, const py::bytes& t, uint32_t start, uint64_t count) {
    const HeaderTarget ht(h, t);
    std::vector<uint32_t> hits;
    {
      py::gil_scoped_release r;
      hits = cpu_scan_sha256d(ht.header(), ht.target(), start, count);
    }
    return hits;
  }, py::arg("header"), py::arg("target"), py::arg("start"), py::arg("count"));
  m.def("cpu_scan_method", &cpu_scan_method);
  // A/B hook: the CPU scan with a given number of nonces in flight per step (1..4 SHA-NI chains, 16 AVX-512).
  m.def("_cpu_scan_lanes", [](int lanes, const py::bytes& h, const py::bytes& t, uint32_t start, uint64_t count) {
    const HeaderTarget ht(h, t);
    std::vector<uint32_t> hits;
    {
      py::gil_scoped_release r;
      hits = cpu_scan_sha256d_lanes(lanes, ht.header(), ht.target(), start, count);
    }
    return hits;
  });
}

// ---- job folding and *_prepare: parameter blocks are returned as opaque bytes and passed back in ----
void bind_job_prepare(py::module_& m) {
  m.def("merkle_root", [](const py::dict& job, uint64_t en2) {
    auto j = make_job(job); uint8_t root[32];
    merkle_root_from_coinbase(*j, en2, root);
    return to_bytes(root, 32);
  });
  m.def("variant_header", [](const py::dict& job, uint64_t v) {
    auto j = make_job(job);
    uint8_t hdr[80]; uint32_t ver, nt; uint64_t en2;
    j->variant_header(v, hdr, &ver, &nt, &en2);
    return py::make_tuple(to_bytes(hdr, 80), ver, nt, en2);
  });
  m.def("variant_space", [](const py::dict& job) { return make_job(job)->variant_space(); });

  m.def("sha256d_prepare", &prepare_params<Sha256dParams, sha256d_prepare>);
  m.attr("SHA256D_MAX_K") = kSha256dMaxK;
  {
    py::list ks;
    for (int k = 2; k <= kSha256dMaxK; ++k)
      if (sha256d_k_floor(k) == k) ks.append(k);
    m.attr("SHA256D_K_VALUES") = py::tuple(ks);
  }
  m.def("sha256d_prepare_k", [](const py::list& headers, const py::bytes& t) {
    std::string ts = need(t, 32, "target");
    std::vector<std::string> hs;
    const std::vector<const uint8_t*> ptrs = header_ptrs(headers, &hs);
    Sha256dParamsK p;
    if (!sha256d_prepare_k(ptrs.data(), (int)ptrs.size(), u8(ts), &p))
      throw std::invalid_argument("need K headers (K in SHA256D_K_VALUES) with identical bytes 64..75");
    return pod_bytes(p);
  }, py::arg("headers"), py::arg("target"));
  m.attr("SHA256D_V_GROUP") = kSha256dVGroup;
  m.attr("SHA256D_V2_GROUP") = kSha256dV2Group;
  m.def("sha256d_prepare_v", [](const py::list& headers, const py::bytes& t) {
    std::string ts = need(t, 32, "target");
    std::vector<std::string> hs;
    const std::vector<const uint8_t*> ptrs = header_ptrs(headers, &hs);
    Sha256dParamsV p;
    std::vector<Sha256dVariant> vars(hs.size());
    if (!sha256d_prepare_v(ptrs.data(), (int)ptrs.size(), u8(ts), &p, vars.data()))
      throw std::invalid_argument("need a positive multiple of 64 headers with identical bytes 64..75");
    return py::make_tuple(pod_bytes(p),
                          py::bytes(reinterpret_cast<const char*>(vars.data()), vars.size() * sizeof(Sha256dVariant)));
  }, py::arg("headers"), py::arg("target"));
  m.def("scrypt_prepare", &prepare_params<ScryptParams, scrypt_prepare>);
  m.def("x11_prepare", &prepare_params<X11Params, x11_prepare>);
  m.attr("SHA256D_PARAMS_SIZE") = sizeof(Sha256dParams);
  m.attr("SHA256D_V_PARAMS_SIZE") = sizeof(Sha256dParamsV);
  m.attr("SCRYPT_PARAMS_SIZE") = sizeof(ScryptParams);
  m.attr("SCRYPT_COOP") = kScryptCoop;
  m.attr("SCRYPT_LANE_W8") = kScryptLaneW8;
  m.attr("SCRYPT_COOP2") = kScryptCoop2;
  m.attr("SCRYPT_COOP_SPLIT") = kScryptCoopSplit;
  // Share verification: the job block is opaque bytes (otedama/share_job.h), built once per job and uploaded.
  m.def("share_job_prepare", [](const py::bytes& coinb1, const py::bytes& coinb2, int en_size,
                                const py::bytes& prev_hash, uint32_t nbits, const std::vector<py::bytes>& branches) {
    std::vector<std::string> bs(branches.begin(), branches.end());
    return pod_bytes(share_job_prepare(coinb1, coinb2, en_size, prev_hash, nbits, bs));
  }, py::arg("coinb1"), py::arg("coinb2"), py::arg("en_size"), py::arg("prev_hash"), py::arg("nbits"),
     py::arg("branches"));
  m.attr("SHARE_JOB_BLOCK_SIZE") = sizeof(ShareJobBlock);
}

// ---- CPU twins of the batch ops, with the constants of their layouts ----
void bind_cpu_twins(py::module_& m) {
  m.def("share_headers_cpu", [](const py::bytes& job_block, const py::bytes& records) {
    const ShareJobBlock job = job_block_from(job_block);
    const std::vector<ShareRec> recs = share_recs_from(records);
    std::string out(recs.size() * 80, '\0');
    share_headers_cpu(job, recs.data(), recs.size(), u8(out));
    return py::bytes(out);
  }, py::arg("job_block"), py::arg("records"));
  // Live share verification: 128-byte result records (otedama/share_job.h ShareResult).
  m.def("share_results_cpu", [](const py::bytes& job_block, const py::bytes& records, const py::bytes& targets) {
    const ShareJobBlock job = job_block_from(job_block);
    const std::vector<ShareRec> recs = share_recs_from(records);
    std::string ts = targets;
    if (ts.empty() || ts.size() % 32) throw std::invalid_argument("targets: expected a non-empty multiple of 32 bytes");
    std::vector<ShareResult> out(recs.size());
    share_results_cpu(job, recs.data(), recs.size(), u8(ts), ts.size() / 32, out.data());
    return py::bytes(reinterpret_cast<const char*>(out.data()), out.size() * sizeof(ShareResult));
  }, py::arg("job_block"), py::arg("records"), py::arg("targets"));
  m.attr("SHARE_RESULT_BYTES") = sizeof(ShareResult);
  // Channel roots: n 16-byte extranonce prefixes against one job block -> n 32-byte merkle roots.
  m.def("share_roots_cpu", [](const py::bytes& job_block, const py::bytes& prefixes) {
    const ShareJobBlock job = job_block_from(job_block);
    std::string ps = prefixes;
    if (ps.size() % 16) throw std::invalid_argument("prefixes: expected a multiple of 16 bytes");
    std::string out(ps.size() * 2, '\0');
    {
      py::gil_scoped_release r;  // a pool's fan-out may be tens of thousands of prefixes
      share_roots_cpu(job, u8(ps), ps.size() / 16, u8(out));
    }
    return py::bytes(out);
  }, py::arg("job_block"), py::arg("prefixes"));
  // Template tree: t trees of n 32-byte leaves -> 1 + depth rows of 32 bytes per tree (otedama/merkle_tree.h).
  m.def("merkle_tree_cpu", [](const py::bytes& leaves, uint32_t t, uint32_t n) {
    if (t == 0 || t > kMerkleTreeMaxTrees) throw std::invalid_argument("t must be in 1..65535");
    if (n == 0 || n > kMerkleTreeMaxLeaves) throw std::invalid_argument("n must be in 1..262144");
    std::string ls = need(leaves, size_t(t) * n * 32, "leaves");
    std::string out(size_t(t) * (1 + merkle_tree_depth(n)) * 32, '\0');
    {
      py::gil_scoped_release r;  // a full template is thousands of leaves in two trees
      merkle_tree_cpu(u8(ls), t, n, u8(out));
    }
    return py::bytes(out);
  }, py::arg("leaves"), py::arg("t"), py::arg("n"));
  m.attr("MERKLE_TREE_MAX_LEAVES") = kMerkleTreeMaxLeaves;
  m.attr("MERKLE_TREE_MAX_TREES") = kMerkleTreeMaxTrees;
  // secp256k1 multiplication: n 128-byte rows -> n 48-byte rows (otedama/secp256k1.h). A flush of the pool's
  // handshake batcher is thousands of ladders.
  m.def("secp256k1_mul_cpu", [](const py::buffer& rows) {
    return on_wiped_copy(rows, "rows",
        [](const uint8_t*, size_t size) {
          if (size == 0 || size % kSecpRowBytes || size / kSecpRowBytes > kSecpMaxRows)
            throw std::invalid_argument("rows: expected 1..65536 rows of 128 bytes");
          return size / kSecpRowBytes * kSecpOutBytes;
        },
        [](const uint8_t* in, size_t size, uint8_t* out, size_t) {
          secp256k1_mul_cpu(in, uint32_t(size / kSecpRowBytes), out);
        });
  }, py::arg("rows"));
  m.def("ellswift_encode_native", [](const py::bytes& x32, const py::bytes& rand_bytes) -> py::object {
    std::string x = need(x32, 32, "x32"), rnd = rand_bytes;
    uint8_t out[64];
    const int rc = ellswift_encode_cpu(u8(x), u8(rnd), rnd.size(), out);
    if (rc < 0) throw std::invalid_argument("ellswift: x is not on secp256k1");
    if (rc == 0) return py::none();
    return to_bytes(out, 64);
  }, py::arg("x32"), py::arg("rand_bytes"));
  m.attr("SECP_ROW_BYTES") = kSecpRowBytes;
  m.attr("SECP_OUT_BYTES") = kSecpOutBytes;
  m.attr("SECP_MAX_ROWS") = kSecpMaxRows;
  // Frame sealing: n heads and their data in one buffer -> the output regions (otedama/aead.h). The OpenSSL twin and
  // the kernel's arithmetic compiled for the host (test entries, leading underscore). A job's fan-out is two frames
  // for every channel of the pool.
  const auto seal_rows = [](const py::buffer& frames, uint32_t n,
                            void (*fn)(const uint8_t*, size_t, uint32_t, uint8_t*, size_t)) {
    return on_wiped_copy(frames, "frames",
        [n](const uint8_t* in, size_t size) { return aead_seal_check(in, size, n, 0); },
        [n, fn](const uint8_t* in, size_t size, uint8_t* out, size_t out_size) { fn(in, size, n, out, out_size); });
  };
  m.def("aead_seal_many_cpu", [seal_rows](const py::buffer& frames, uint32_t n) {
    return seal_rows(frames, n, aead_seal_many_cpu);
  }, py::arg("frames"), py::arg("n"));
  m.def("_aead_seal_rows_host", [seal_rows](const py::buffer& frames, uint32_t n) {
    return seal_rows(frames, n, aead_seal_rows_host);
  }, py::arg("frames"), py::arg("n"));
  m.def("_poly1305_rows_host", [](const py::buffer& rows) {
    const py::buffer_info info = byte_view(rows, "rows");
    const size_t size = size_t(info.size);
    if (size == 0 || size % kPolyRowBytes) throw std::invalid_argument("rows: expected rows of 160 bytes");
    std::string out(size / kPolyRowBytes * 16, '\0');
    poly1305_rows_host(static_cast<const uint8_t*>(info.ptr), uint32_t(size / kPolyRowBytes), u8(out));
    return py::bytes(out);
  }, py::arg("rows"));
  m.attr("SEAL_HEAD_BYTES") = kSealHeadBytes;
  m.attr("SEAL_MAX_PLAIN") = kSealMaxPlain;
  m.attr("SEAL_MAX_FRAMES") = kSealMaxFrames;
  m.attr("POLY_ROW_BYTES") = kPolyRowBytes;
  m.attr("POLY_MAX_MSG") = kPolyMaxMsg;
}

// ---- kernel launches: the argument rules here, the launch's own validation behind them (search_launch.h) ----
void bind_launches(py::module_& m) {
  m.def("launch_sha256d", [](const py::bytes& params, uint32_t base, uint64_t count, uintptr_t out, uint32_t cap,
                             int grid, uintptr_t stream) {
    const auto p = pod_from<Sha256dParams>(params, "params");
    if (count == 0 || count > (1ull << 32)) throw std::invalid_argument("count must be in [1, 2^32]");
    if (grid <= 0 || out == 0) throw std::invalid_argument("bad grid / out");
    LAUNCH(launch_sha256d_search, p, base, count, ops_sink(out, cap, 1), grid, stream_of(stream));
  }, py::arg("params"), py::arg("base"), py::arg("count"), py::arg("out"), py::arg("cap"), py::arg("grid"),
     py::arg("stream"));
  m.def("launch_sha256d_k", [](const py::bytes& params, uint32_t base, uint64_t count, uintptr_t out, uint32_t cap,
                               int grid, uintptr_t stream) {
    const auto p = pod_from<Sha256dParamsK>(params, "params");
    if (p.k < 2 || p.k > kSha256dMaxK) throw std::invalid_argument("bad K");
    if (count == 0 || count > (1ull << 32)) throw std::invalid_argument("count must be in [1, 2^32]");
    if (grid <= 0 || out == 0) throw std::invalid_argument("bad grid / out");
    LAUNCH(launch_sha256d_search_k, p, base, count, ops_sink(out, cap, 2), grid, stream_of(stream));
  }, py::arg("params"), py::arg("base"), py::arg("count"), py::arg("out"), py::arg("cap"), py::arg("grid"),
     py::arg("stream"));
  m.def("launch_sha256d_v", [](const py::bytes& params, uintptr_t vars, uint32_t base, uint64_t count, uintptr_t out,
                               uint32_t cap, int grid, uintptr_t stream, bool occupancy8, int block, int chains) {
    auto p = pod_from<Sha256dParamsV>(params, "params");
    p.occupancy8 = occupancy8 ? 1u : 0u;
    if (p.groups == 0 || count == 0 || count > (1ull << 32)) throw std::invalid_argument("bad groups / count");
    if (block != 64 && block != 256) throw std::invalid_argument("block must be 64 or 256 threads");
    if (chains < 1 || chains > 4) throw std::invalid_argument("chains must be 1..4");
    if (p.groups % uint32_t(chains) != 0)
      throw std::invalid_argument("chains variants per lane need a multiple of 64 * chains variants");
    if (grid <= 0 || (uint64_t(grid) * uint32_t(block / 64)) % (p.groups / uint32_t(chains)) != 0 || vars == 0 || out == 0)
      throw std::invalid_argument("the wave count must be a multiple of the variant groups; vars/out must be set");
    LAUNCH(launch_sha256d_search_v, p, dev{vars}, base, count, ops_sink(out, cap, 2), grid, stream_of(stream), block,
           chains);
  }, py::arg("params"), py::arg("vars"), py::arg("base"), py::arg("count"), py::arg("out"), py::arg("cap"),
     py::arg("grid"), py::arg("stream"), py::arg("occupancy8") = false, py::arg("block") = 256, py::arg("chains") = 1);
  m.def("launch_scrypt", [](const py::bytes& params, uint32_t base, uint32_t count, uintptr_t xbuf, uintptr_t scratch,
                            int gap, uintptr_t out, uint32_t cap, int grid, uintptr_t stream) {
    const auto p = pod_from<ScryptParams>(params, "params");
    if (!scrypt_gap_valid(gap))
      throw std::invalid_argument("gap must be 1, 2, 4, SCRYPT_COOP or SCRYPT_LANE_W8");
    if (grid <= 0 || out == 0 || xbuf == 0 || scratch == 0 || count == 0) throw std::invalid_argument("bad launch args");
    LAUNCH(launch_scrypt_search, p, base, count, dev{xbuf}, dev{scratch}, gap, ops_sink(out, cap, 1), grid,
           stream_of(stream));
  }, py::arg("params"), py::arg("base"), py::arg("count"), py::arg("xbuf"), py::arg("scratch"), py::arg("gap"),
     py::arg("out"), py::arg("cap"), py::arg("grid"), py::arg("stream"));

  // X11: without `out` the stages write H alone (a null sink).
  m.def("launch_x11_stage", [](const py::bytes& params, int stage, uint32_t base, uintptr_t H, uint32_t stride,
                               uint32_t n, uintptr_t out, uint32_t cap, uintptr_t stream) {
    const auto p = pod_from<X11Params>(params, "params");
    if (stage < 0 || stage >= kX11StageCount) throw std::invalid_argument("stage must be in [0, 11)");
    if (H == 0 || n == 0 || stride < n) throw std::invalid_argument("need H != 0, n > 0, stride >= n");
    const HitSink s = ops_sink(out, cap, 1);
    LAUNCH(x11_launch_stage, stage, p, base, dev{H}, stride, n, out ? &s : nullptr, stream_of(stream));
  }, py::arg("params"), py::arg("stage"), py::arg("base"), py::arg("H"), py::arg("stride"), py::arg("n"),
     py::arg("out") = 0, py::arg("cap") = 0, py::arg("stream") = 0);
  m.def("launch_x11", [](const py::bytes& params, uint32_t base, uintptr_t H, uint32_t stride, uint32_t n,
                         uintptr_t out, uint32_t cap, uintptr_t stream) {
    const auto p = pod_from<X11Params>(params, "params");
    if (H == 0 || n == 0 || stride < n) throw std::invalid_argument("need H != 0, n > 0, stride >= n");
    const HitSink s = ops_sink(out, cap, 1);
    LAUNCH(x11_launch_chain, p, base, dev{H}, stride, n, out ? &s : nullptr, stream_of(stream));
  }, py::arg("params"), py::arg("base"), py::arg("H"), py::arg("stride"), py::arg("n"), py::arg("out") = 0,
     py::arg("cap") = 0, py::arg("stream") = 0);

  // Digest ops: n unrelated 80-byte headers (device pointer, densely packed) -> n 32-byte digests. Alignment is left
  // to the launch: a misaligned array is its hipErrorInvalidValue, a RuntimeError.
  m.def("launch_sha256d_digest", [](uintptr_t headers, uint32_t n, uintptr_t out, uintptr_t stream) {
    if (headers == 0 || out == 0 || n == 0) throw std::invalid_argument("need headers != 0, out != 0, n > 0");
    LAUNCH(launch_sha256d_digest, dev{headers}, n, dev{out}, stream_of(stream));
  }, py::arg("headers"), py::arg("n"), py::arg("out"), py::arg("stream") = 0);
  m.def("launch_scrypt_digest", [](uintptr_t headers, uint32_t n, uintptr_t xbuf, uintptr_t scratch, int gap,
                                   uintptr_t out, int grid, uintptr_t stream) {
    if (headers == 0 || out == 0 || xbuf == 0 || scratch == 0 || n == 0 || grid <= 0)
      throw std::invalid_argument("bad launch args");
    if (uint64_t(n) > uint64_t(grid) * 256u) throw std::invalid_argument("n must be at most grid * 256");
    LAUNCH(launch_scrypt_digest, dev{headers}, n, dev{xbuf}, dev{scratch}, gap, dev{out}, grid, stream_of(stream));
  }, py::arg("headers"), py::arg("n"), py::arg("xbuf"), py::arg("scratch"), py::arg("gap"), py::arg("out"),
     py::arg("grid"), py::arg("stream") = 0);
  m.def("launch_x11_digest", [](uintptr_t headers, uintptr_t H, uint32_t stride, uint32_t n, uintptr_t out,
                                uintptr_t stream) {
    if (headers == 0 || out == 0 || H == 0 || n == 0 || stride < n)
      throw std::invalid_argument("need headers, H, out != 0, n > 0, stride >= n");
    LAUNCH(launch_x11_digest, dev{headers}, dev{H}, stride, n, dev{out}, stream_of(stream));
  }, py::arg("headers"), py::arg("H"), py::arg("stride"), py::arg("n"), py::arg("out"), py::arg("stream") = 0);

  // The later ops check alignment here, before the launch: a ValueError.
  m.def("launch_share_headers", [](uintptr_t job, uintptr_t records, uint32_t n, uintptr_t headers,
                                   uintptr_t stream) {
    if (job == 0 || records == 0 || headers == 0 || n == 0)
      throw std::invalid_argument("need job, records, headers != 0, n > 0");
    if ((job | records | headers) & 15u) throw std::invalid_argument("job, records and headers must be 16-byte aligned");
    LAUNCH(launch_share_headers, dev{job}, dev{records}, n, dev{headers}, stream_of(stream));
  }, py::arg("job"), py::arg("records"), py::arg("n"), py::arg("headers"), py::arg("stream") = 0);
  m.def("launch_share_verdict", [](uintptr_t job, uintptr_t records, uintptr_t digests, uintptr_t targets,
                                   uint32_t n_targets, uint32_t n, uintptr_t verdicts, uintptr_t stream) {
    if (job == 0 || records == 0 || digests == 0 || targets == 0 || verdicts == 0 || n == 0 || n_targets == 0)
      throw std::invalid_argument("need job, records, digests, targets, verdicts != 0, n > 0, n_targets > 0");
    if ((job | records | digests | targets) & 15u)
      throw std::invalid_argument("job, records, digests and targets must be 16-byte aligned");
    LAUNCH(launch_share_verdict, dev{job}, dev{records}, dev{digests}, dev{targets}, n_targets, n, dev{verdicts},
           stream_of(stream));
  }, py::arg("job"), py::arg("records"), py::arg("digests"), py::arg("targets"), py::arg("n_targets"), py::arg("n"),
     py::arg("verdicts"), py::arg("stream") = 0);
  m.def("launch_share_pack", [](uintptr_t job, uintptr_t records, uintptr_t headers, uintptr_t digests,
                                uintptr_t targets, uint32_t n_targets, uint32_t n, uintptr_t results,
                                uintptr_t stream) {
    if (job == 0 || records == 0 || headers == 0 || digests == 0 || targets == 0 || results == 0 || n == 0 ||
        n_targets == 0)
      throw std::invalid_argument("need job, records, headers, digests, targets, results != 0, n > 0, n_targets > 0");
    if ((job | records | headers | digests | targets | results) & 15u)
      throw std::invalid_argument("job, records, headers, digests, targets and results must be 16-byte aligned");
    LAUNCH(launch_share_pack, dev{job}, dev{records}, dev{headers}, dev{digests}, dev{targets}, n_targets, n,
           dev{results}, stream_of(stream));
  }, py::arg("job"), py::arg("records"), py::arg("headers"), py::arg("digests"), py::arg("targets"),
     py::arg("n_targets"), py::arg("n"), py::arg("results"), py::arg("stream") = 0);
  m.def("launch_channel_roots", [](uintptr_t job, uintptr_t prefixes, uint32_t n, uintptr_t roots, uintptr_t stream) {
    if (job == 0 || prefixes == 0 || roots == 0 || n == 0)
      throw std::invalid_argument("need job, prefixes, roots != 0, n > 0");
    if ((job | prefixes | roots) & 15u) throw std::invalid_argument("job, prefixes and roots must be 16-byte aligned");
    LAUNCH(launch_channel_roots, dev{job}, dev{prefixes}, n, dev{roots}, stream_of(stream));
  }, py::arg("job"), py::arg("prefixes"), py::arg("n"), py::arg("roots"), py::arg("stream") = 0);
  m.def("launch_merkle_tree", [](uintptr_t leaves, uint32_t t, uint32_t n, uintptr_t scratch, uintptr_t out,
                                 uintptr_t stream) {
    if (t == 0 || t > kMerkleTreeMaxTrees || n == 0 || n > kMerkleTreeMaxLeaves)
      throw std::invalid_argument("need t in 1..65535, n in 1..262144");
    if (leaves == 0 || out == 0 || (n > 512 && scratch == 0))
      throw std::invalid_argument("need leaves, out != 0, and scratch != 0 for n > 512");
    if ((leaves | out | scratch) & 15u) throw std::invalid_argument("leaves, scratch and out must be 16-byte aligned");
    LAUNCH(launch_merkle_tree, dev{leaves}, t, n, dev{scratch}, dev{out}, stream_of(stream));
  }, py::arg("leaves"), py::arg("t"), py::arg("n"), py::arg("scratch"), py::arg("out"), py::arg("stream") = 0);
  m.def("launch_secp256k1_mul", [](uintptr_t rows, uint32_t n, uintptr_t out, uintptr_t stream) {
    if (n == 0 || n > kSecpMaxRows) throw std::invalid_argument("need n in 1..65536");
    if (rows == 0 || out == 0) throw std::invalid_argument("need rows, out != 0");
    if ((rows | out) & 15u) throw std::invalid_argument("rows and out must be 16-byte aligned");
    LAUNCH(launch_secp256k1_mul, dev{rows}, n, dev{out}, stream_of(stream));
  }, py::arg("rows"), py::arg("n"), py::arg("out"), py::arg("stream") = 0);
  m.def("launch_aead_seal", [](uintptr_t frames, uint64_t in_bytes, uint32_t n, uintptr_t out, uint64_t out_bytes,
                               uintptr_t stream) {
    if (n == 0 || n > kSealMaxFrames) throw std::invalid_argument("need n in 1..2^24-1");
    if (frames == 0 || out == 0) throw std::invalid_argument("need frames, out != 0");
    if ((frames | out | in_bytes | out_bytes) & 15u)
      throw std::invalid_argument("frames, out and their sizes must be multiples of 16");
    if (in_bytes < uint64_t(n) * kSealHeadBytes || (in_bytes >> 32) || (out_bytes >> 32))
      throw std::invalid_argument("frames holds n 64-byte heads; both buffers are below 4 GiB");
    LAUNCH(launch_aead_seal, dev{frames}, in_bytes, n, dev{out}, out_bytes, stream_of(stream));
  }, py::arg("frames"), py::arg("in_bytes"), py::arg("n"), py::arg("out"), py::arg("out_bytes"),
     py::arg("stream") = 0);
  m.def("_launch_poly1305_rows", [](uintptr_t rows, uint32_t n, uintptr_t tags, uintptr_t stream) {
    if (n == 0 || n > kSealMaxFrames) throw std::invalid_argument("need n in 1..2^24-1");
    if (rows == 0 || tags == 0) throw std::invalid_argument("need rows, tags != 0");
    if ((rows | tags) & 15u) throw std::invalid_argument("rows and tags must be 16-byte aligned");
    LAUNCH(launch_poly1305_rows, dev{rows}, n, dev{tags}, stream_of(stream));
  }, py::arg("rows"), py::arg("n"), py::arg("tags"), py::arg("stream") = 0);
}

// ---- test hooks, device queries and trace ranges ----
void bind_test_hooks(py::module_& m) {
  // Test hook: the miner's device-clock estimate (ClockBounds) over a sequence of (seen at, offset bound) pairs;
  // returns the estimate after each.
  m.def("_clock_bounds", [](double window, const std::vector<std::pair<double, double>>& samples) {
    ClockBounds cb(window);
    std::vector<double> out;
    for (const auto& s : samples) out.push_back(cb.add(s.first, s.second));
    return out;
  });
  // Test hook: the miner's search-plan rules (otedama/launch_plan.h), each from its own arguments: the normalised
  // batch, the launch cap of a target, the SHA-256d layout of a run, the CU mask of a reservation list.
  m.def("_launch_plan_rules", [](uint64_t batch_nonces, uint32_t target_hi, bool capped, int sha_variants, int run,
                                 const std::string& reserve_cus, int ncu) {
    const ShaLayout lay = pick_layout(sha_variants, run);
    const CuMask cm = parse_reserved_cus(reserve_cus.c_str(), ncu);
    py::dict d;
    d["batch"] = normalize_batch(batch_nonces);
    d["cap"] = launch_cap_hashes(target_hi, capped);
    d["layout"] = py::make_tuple(lay.nvar, lay.use_v);
    d["cu_mask"] = cm.words;
    d["reserved"] = cm.reserved;
    return d;
  }, py::arg("batch_nonces") = 0, py::arg("target_hi") = 0, py::arg("capped") = true, py::arg("sha_variants") = 1,
     py::arg("run") = 1, py::arg("reserve_cus") = "", py::arg("ncu") = 256);
  // Test hook: the miner's cursor walked over launches of one kind ("scrypt", "x11", "v", "k", "single") from
  // nonce offset `start` until the stripe position moves (or `max_launches`): every launch's (base, count,
  // variant_next) and the stripe position reached.
  m.def("_launch_plan_walk", [](const std::string& kind, uint64_t batch, uint64_t cap, int nvar, uint64_t lanes,
                                uint64_t start, size_t max_launches, uint64_t variant_start, uint64_t variant_stride) {
    const LaunchKind lk = kind == "scrypt" ? LaunchKind::kScrypt : kind == "x11" ? LaunchKind::kX11
                        : kind == "v" ? LaunchKind::kVersionParallel : kind == "k" ? LaunchKind::kVariantK
                        : kind == "single" ? LaunchKind::kSingle
                        : throw std::invalid_argument("kind: scrypt, x11, v, k or single");
    if (start >= kNonceSpace) throw std::invalid_argument("start must be below 2^32");
    SearchCursor c;
    c.nonce_off = start;
    std::vector<std::tuple<uint64_t, uint64_t, uint64_t>> launches;
    while (c.k == 0 && launches.size() < max_launches) {
      const uint64_t base = c.nonce_off, count = launch_count(lk, batch, cap, nvar, lanes, c.nonce_off);
      c.advance(count, nvar);
      launches.emplace_back(base, count, c.variant_next(variant_start, variant_stride, nvar));
    }
    return py::make_tuple(launches, c.k);
  }, py::arg("kind"), py::arg("batch"), py::arg("cap"), py::arg("nvar") = 1, py::arg("lanes") = 0,
     py::arg("start") = 0, py::arg("max_launches") = size_t(1) << 20, py::arg("variant_start") = 0,
     py::arg("variant_stride") = 1);
  // Test hook: the scrypt verifier's bounded queue (BoundedWorkQueue) flooded by a producer that never waits, with
  // a consumer hashing every item on the host. batch > 1 takes up to that many items per pop_many and hashes them in
  // one scrypt_1024_1_1_batch pass, as the GPU miner's verifier does (16); batch 1 pops and hashes one at a time.
  m.def("_work_queue_flood", [](size_t cap, size_t n, bool hash_each, size_t batch) {
    BoundedWorkQueue<std::array<uint8_t, 80>> q(cap);
    std::atomic<uint64_t> processed{0};
    uint64_t accepted = 0;
    {
      py::gil_scoped_release r;
      std::thread consumer([&] {
        if (batch > 1) {
          std::vector<std::array<uint8_t, 80>> items;
          std::vector<const uint8_t*> ip;
          std::vector<std::array<uint8_t, 32>> outs(batch);
          std::vector<uint8_t*> op;
          for (auto& o : outs) op.push_back(o.data());
          while (items.clear(), q.pop_many(&items, batch) > 0) {
            ip.clear();
            for (const auto& it : items) ip.push_back(it.data());
            if (hash_each) scrypt_1024_1_1_batch(int(items.size()), ip.data(), op.data());
            processed.fetch_add(items.size());
          }
          return;
        }
        std::array<uint8_t, 80> h;
        uint8_t out[32];
        while (q.pop(&h)) {
          if (hash_each) scrypt_1024_1_1(h.data(), out);
          processed.fetch_add(1);
        }
      });
      for (size_t i = 0; i < n; ++i) {
        std::array<uint8_t, 80> h{};
        std::memcpy(h.data() + 76, &i, 4);
        if (q.push(std::move(h))) ++accepted;
      }
      q.stop(~size_t(0));
      consumer.join();
    }
    py::dict d;
    d["accepted"] = accepted;
    d["refused"] = q.refused();
    d["peak"] = q.peak();
    d["processed"] = processed.load();
    return d;
  }, py::arg("cap"), py::arg("n"), py::arg("hash_each") = true, py::arg("batch") = 1);
  // roctx ranges for Python-side spans (node collectives, share submit, bench steps): SURVEY §5.1.
  m.def("trace_push", [](const std::string& name) { trace_push(name.c_str()); });
  m.def("trace_pop", [] { trace_pop(); });
  m.def("trace_mark", [](const std::string& name) { trace_mark(name.c_str()); });
  m.def("gpu_device_count", &gpu_device_count);
  m.def("gpu_arch_name", &gpu_arch_name);
  m.def("gpu_cu_count", &gpu_cu_count);
  m.def("scrypt_scratch_bytes", &scrypt_scratch_bytes);
  // test hooks: what the launch files read from the environment (they launch nothing)
  m.def("x11_midstage_polls", [] { return x11k::x11_midstage_polls(); });
  m.def("_scrypt_romix_mode", [] {
    bool write_polls = false;
    uint32_t segments = 0;
    scrypt_romix_mode(&write_polls, &segments);
    py::dict d;
    d["write_polls"] = write_polls;
    d["segments"] = segments;
    return d;
  });
  // test hook: the /proc/self/maps check behind the CPU-stored abort word (GpuMiner host_abort)
  m.def("maps_range_writable", [](const std::string& maps, uint64_t lo, uint64_t hi) {
    return maps_range_writable(maps, uintptr_t(lo), uintptr_t(hi));
  });
}

// ---- the miner classes ----
void bind_miners(py::module_& m) {
  py::class_<MinerBase, std::shared_ptr<MinerBase>>(m, "Miner")
      .def("start", &MinerBase::start, py::call_guard<py::gil_scoped_release>())
      .def("stop", &MinerBase::stop, py::call_guard<py::gil_scoped_release>())
      .def("set_job", [](MinerBase& self, py::object job) {
        if (job.is_none()) { py::gil_scoped_release r; self.set_job(nullptr); return; }
        auto j = make_job(job.cast<py::dict>());
        py::gil_scoped_release r;
        self.set_job(j);
      })
      .def("poll", [](MinerBase& self, size_t max) {
        std::vector<ShareRecord> v;
        { py::gil_scoped_release r; v = self.poll(max); }
        return shares_to_list(std::move(v));
      }, py::arg("max") = 256)
      .def("stats", [](MinerBase& self) { return stats_to_dict(self.stats()); })
      .def("share_fd", &MinerBase::share_fd,
           "eventfd that becomes readable when shares are queued (read 8 bytes to reset, then poll())")
      .def_property_readonly("device_id", &MinerBase::device_id);

  py::class_<GpuMiner, MinerBase, std::shared_ptr<GpuMiner>>(m, "GpuMiner")
      .def(py::init<int, std::string, uint64_t, int, size_t, int>(), py::arg("device"), py::arg("device_id"),
           py::arg("batch_nonces") = (1ull << 32), py::arg("grid") = 2048, py::arg("queue_cap") = 1024,
           py::arg("sha_variants") = 128);
  py::class_<CpuMiner, MinerBase, std::shared_ptr<CpuMiner>>(m, "CpuMiner")
      .def(py::init<int, std::string, size_t>(), py::arg("threads"), py::arg("device_id") = "cpu-0",
           py::arg("queue_cap") = 1024);
}

}  // namespace

PYBIND11_MODULE(_native, m) {
  m.doc() = "Otedama MI355X native runtime (gfx950 HIP kernels + C++ host runtime)";
  bind_host_hashes(m);
  bind_job_prepare(m);
  bind_cpu_twins(m);
  bind_launches(m);
  bind_test_hooks(m);
  bind_miners(m);
}
