// HIP error and pointer-alignment checks shared by the HIP translation units and the bindings (host side only; the
// runtime's API header is plain C++).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <stdexcept>
#include <string>

namespace otedama {

// Throws std::runtime_error("HIP error <hipGetErrorString> at <what>") unless e is hipSuccess.
inline void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e) + " at " + what);
}

// True when every pointer is 16-byte aligned: the kernels move headers, digests and records as 16-byte vectors.
template <class... P>
inline bool aligned16(const P*... p) {
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15u) == 0;
}

}  // namespace otedama

#define OTD_HIP(call) ::otedama::hip_check((call), #call)
