// Launch entry points of the gfx950 kernels (csrc/kernels/*.hip) and the device queries, declared once for the files
// that define them, the GPU miner and the Python bindings. The X11 stage launchers are in otedama/x11_launch.h.
// Plain C++: the runtime's API header and its vector types need no HIP compiler, so bindings.cpp, which the host
// compiler builds, calls the launches itself. Every launch enqueues on `stream` and synchronises nothing.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstdint>
#include <string>

#include "otedama/aead.h"
#include "otedama/hitsink.h"
#include "otedama/job.h"
#include "otedama/merkle_tree.h"
#include "otedama/secp256k1.h"

namespace otedama {

// Scratchpad bytes for `grid` ROMix blocks of 256 lane slots at lookup gap `gap` (scrypt_search.hip).
uint64_t scrypt_scratch_bytes(int grid, int gap);

// What the launch files read from the environment, for tests of those modes (read-only; nothing is launched).
// scrypt_search.hip: whether the one-launch cooperative ROMix polls the abort word inside its write loop
// (OTEDAMA_SCRYPT_POLL, read once per process) and the segment count of this moment (OTEDAMA_SCRYPT_SEGMENTS, read
// at every launch; 0 = one launch).
void scrypt_romix_mode(bool* write_polls, uint32_t* segments);
namespace x11k {
bool x11_midstage_polls();  // x11_stages_b.hip: OTEDAMA_X11_MIDPOLL, read once per process
}

// Device queries (gpu_miner.hip): 0 / "" when the runtime cannot answer.
int gpu_device_count();
std::string gpu_arch_name(int device);
int gpu_cu_count(int device);

// `count` nonces from `base` on `grid` blocks of 256 (sha256d_search.hip, sha256d_search_v.hip); hits go to `sink`.
hipError_t launch_sha256d_search(const Sha256dParams& p, uint32_t base, uint64_t count, const HitSink& sink, int grid,
                                 hipStream_t stream);
hipError_t launch_sha256d_search_k(const Sha256dParamsK& p, uint32_t base, uint64_t count, const HitSink& sink,
                                   int grid, hipStream_t stream);
hipError_t launch_sha256d_search_v(const Sha256dParamsV& p, const Sha256dVariant* vars, uint32_t base, uint64_t count,
                                   const HitSink& sink, int grid, hipStream_t stream, int block = 256, int chains = 1);

// xbuf: count * 128 bytes. scratch: scrypt_scratch_bytes(grid, gap) (scrypt_search.hip).
hipError_t launch_scrypt_search(const ScryptParams& p, uint32_t base, uint32_t count, void* xbuf, void* scratch,
                                int gap, const HitSink& sink, int grid, hipStream_t stream);

// The ROMix launch(es) of launch_scrypt_search alone, over the `count` PBKDF2-in states in xbuf (scrypt_search.hip).
hipError_t launch_scrypt_romix(uint32_t count, uint4* xbuf, uint4* scratch, int gap, const HitSink& sink, int grid,
                               hipStream_t stream);

// Digest ops (kernels in digest_batch.hip): n unrelated 80-byte headers at headers + 80 * i -> n digests at
// out + 32 * i, in the byte order PowAlgorithm.hash returns. Each returns hipErrorInvalidValue, before launching
// anything, for n == 0, n above the stated capacity, a null pointer or a header / digest array that is not 16-byte
// aligned.
hipError_t launch_sha256d_digest(const uint8_t* headers, uint32_t n, uint8_t* out, hipStream_t s);
// xbuf: grid * 256 * 128 bytes. scratch: scrypt_scratch_bytes(grid, gap). One header per lane slot.
hipError_t launch_scrypt_digest(const uint8_t* headers, uint32_t n, void* xbuf, void* scratch, int gap,
                                uint8_t* out, int grid, hipStream_t s);   // n <= grid * 256
// H: 8 * stride u64, the stage planes of the X11 chain (otedama/x11_launch.h).
hipError_t launch_x11_digest(const uint8_t* headers, uint64_t* H, uint32_t stride, uint32_t n, uint8_t* out,
                             hipStream_t s);                              // n <= stride

// Share verification (kernels in share_verify.hip; layouts in otedama/share_job.h): n 32-byte share records against
// one uploaded job block (job: a device copy of a ShareJobBlock) -> n 80-byte headers, and n digests against a table
// of n_targets 32-byte targets -> n verdict bytes. Each returns hipErrorInvalidValue, before launching anything, for
// n == 0, an empty target table, a null pointer or an array (the job block included, the verdicts excepted) that is
// not 16-byte aligned.
hipError_t launch_share_headers(const void* job, const uint8_t* records, uint32_t n, uint8_t* headers, hipStream_t s);
hipError_t launch_share_verdict(const void* job, const uint8_t* records, const uint8_t* digests,
                                const uint8_t* targets, uint32_t n_targets, uint32_t n, uint8_t* verdicts,
                                hipStream_t s);
// Live share verification (otd_share_pack): the headers and digests of the chain above -> n 128-byte ShareResult
// records, with the compares done there. The same conventions; here every array, the results included, is 16-byte
// aligned.
hipError_t launch_share_pack(const void* job, const uint8_t* records, const uint8_t* headers, const uint8_t* digests,
                             const uint8_t* targets, uint32_t n_targets, uint32_t n, uint8_t* results, hipStream_t s);
// Channel roots (otd_channel_roots of channel_roots.hip): n 16-byte extranonce prefixes (the job's first en_size bytes
// of each are used) against one uploaded job block -> n 32-byte merkle roots at roots + 32 * i, in header byte order.
// hipErrorInvalidValue, before launching anything, for n == 0, a null pointer or an array (the job block included)
// that is not 16-byte aligned.
hipError_t launch_channel_roots(const void* job, const uint8_t* prefixes, uint32_t n, uint8_t* roots, hipStream_t s);
// Template tree (otd_merkle_tree of merkle_tree.hip; rows, limits and the CPU twin: otedama/merkle_tree.h): t trees of
// n 32-byte leaves at leaves + 32 * n * y -> 1 + depth rows of 32 bytes per tree at out + 32 * (1 + depth) * y.
// scratch: 32 bytes per 512-leaf chunk per tree (t * ceil(n / 512) rows), read only when n > 512; may be null
// otherwise. hipErrorInvalidValue, before launching anything, for t == 0 or above kMerkleTreeMaxTrees, n == 0 or
// above kMerkleTreeMaxLeaves, a null or not 16-byte aligned leaves or out, and the same of scratch when n > 512.
hipError_t launch_merkle_tree(const uint8_t* leaves, uint32_t t, uint32_t n, uint8_t* scratch, uint8_t* out,
                              hipStream_t s);
// secp256k1 multiplication (otd_secp256k1_mul of secp256k1_mul.hip; rows, limits and the CPU twin:
// otedama/secp256k1.h): n 128-byte rows -> n 48-byte rows. hipErrorInvalidValue, before launching anything, for
// n == 0 or above kSecpMaxRows, and a null or not 16-byte aligned rows or out.
hipError_t launch_secp256k1_mul(const uint8_t* rows, uint32_t n, uint8_t* out, hipStream_t s);
// Frame sealing (otd_aead_seal of aead_seal.hip; heads, regions, limits and the CPU twin: otedama/aead.h): n heads and
// their data in one input buffer -> each frame's tag and ciphertext in its region of the output.
// hipErrorInvalidValue, before launching anything, for n == 0 or above kSealMaxFrames, a null or not 16-byte aligned
// buffer, an input shorter than its n heads, and a buffer size that is no multiple of 16 or is 4 GiB or more. The
// heads themselves are on the device: the kernel skips a lane whose head breaks the rules. otd_poly1305_rows is the
// test entry: n 160-byte rows -> n 16-byte tags.
hipError_t launch_aead_seal(const uint8_t* in, uint64_t in_bytes, uint32_t n, uint8_t* out, uint64_t out_bytes,
                            hipStream_t s);
hipError_t launch_poly1305_rows(const uint8_t* rows, uint32_t n, uint8_t* tags, hipStream_t s);

}  // namespace otedama
