// Integer-multiply issue cost on gfx950, by the method of bench_valu.hip (profiles/r1/valu_issue_rates.md): cycles
// per wave64 instruction per SIMD for the multiplies the secp256k1 field arithmetic is built from
// (csrc/kernels/secp256k1_mul.hip), with v_add_u32 as the control.
//
// Each wave runs `iters` bodies of 64 independent instructions of one op on fixed registers; B blocks of 256 threads
// per CU put B waves on every SIMD. Reported per (op, B): the s_memtime cycles of a block and the hipEvent wall time
// at the device's clock, each divided by B * instructions per wave.
// Build: hipcc --offload-arch=gfx950 -O3 tools/experiments/bench_imul.hip -o build/bench_imul
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

#define CLOBBERS                                                                                                  \
  "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27", "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", \
      "v40", "v41", "v42", "v43", "s10", "s11", "vcc"

// destinations cycle over v20..v35; no instruction reads a register written in the body
#define EACH16(OP) OP(20) OP(21) OP(22) OP(23) OP(24) OP(25) OP(26) OP(27) OP(28) OP(29) OP(30) OP(31) OP(32) OP(33) OP(34) OP(35)
#define EACH8P(OP) OP(20, 21) OP(22, 23) OP(24, 25) OP(26, 27) OP(28, 29) OP(30, 31) OP(32, 33) OP(34, 35)
#define X4(B) B B B B
#define X8(B) B B B B B B B B

#define ADD_U32(d) "v_add_u32 v" #d ", v40, v41\n\t"
#define MUL_LO(d) "v_mul_lo_u32 v" #d ", v40, v41\n\t"
#define MUL_HI(d) "v_mul_hi_u32 v" #d ", v40, v41\n\t"
#define MAD_U64(lo, hi) "v_mad_u64_u32 v[" #lo ":" #hi "], s[10:11], v40, v41, v[42:43]\n\t"
#define MUL_U24(d) "v_mul_u32_u24 v" #d ", v40, v41\n\t"

constexpr int kBodyLen = 64;
static const char* kOpNames[] = {"add_u32_vop2", "mul_lo_u32", "mul_hi_u32", "mad_u64_u32", "mul_u32_u24"};
constexpr int kOps = 5;

template <int OP>
__device__ __forceinline__ void body() {
  if constexpr (OP == 0) asm volatile(X4(EACH16(ADD_U32))::: CLOBBERS);
  if constexpr (OP == 1) asm volatile(X4(EACH16(MUL_LO))::: CLOBBERS);
  if constexpr (OP == 2) asm volatile(X4(EACH16(MUL_HI))::: CLOBBERS);
  if constexpr (OP == 3) asm volatile(X8(EACH8P(MAD_U64))::: CLOBBERS);
  if constexpr (OP == 4) asm volatile(X4(EACH16(MUL_U24))::: CLOBBERS);
}

template <int OP>
__global__ __launch_bounds__(256) void k_imul(unsigned long long* cyc, uint32_t* out, int iters) {
  const uint32_t seed = threadIdx.x * 2654435761u ^ blockIdx.x;
  asm volatile("v_mov_b32 v40, %0\n\tv_add_u32 v41, 1, %0\n\tv_add_u32 v42, 2, %0\n\tv_add_u32 v43, 3, %0\n\t"
               "v_mov_b32 v20, %0\n\tv_mov_b32 v27, %0\n\tv_mov_b32 v35, %0" ::"v"(seed)
               : CLOBBERS);
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int i = 0; i < iters; ++i) body<OP>();
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  uint32_t r;
  asm volatile("v_bitop3_b32 %0, v20, v27, v35 bitop3:0x96" : "=v"(r)::CLOBBERS);
  out[blockIdx.x * 256 + threadIdx.x] = r;
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

using Kfn = void (*)(unsigned long long*, uint32_t*, int);
static const Kfn kKernels[] = {k_imul<0>, k_imul<1>, k_imul<2>, k_imul<3>, k_imul<4>};

int main() {
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  const double clk_hz = prop.clockRate * 1e3;
  const int iters = 1024, max_b = 8;
  unsigned long long* cyc;
  uint32_t* out;
  CHECK(hipMalloc(&cyc, sizeof(unsigned long long) * cus * max_b));
  CHECK(hipMalloc(&out, sizeof(uint32_t) * 256 * cus * max_b));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::printf("{\"cus\": %d, \"clock_mhz\": %.0f, \"iters\": %d, \"results\": [\n", cus, clk_hz / 1e6, iters);
  bool first = true;
  for (int op = 0; op < kOps; ++op) {
    for (int b : {2, 4, 8}) {
      const int grid = cus * b;
      double best_ms = 1e30, best_cyc = 1e30;
      for (int rep = 0; rep < 4; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(kKernels[op], dim3(grid), dim3(256), 0, 0, cyc, out, iters);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        std::vector<unsigned long long> c(grid);
        CHECK(hipMemcpy(c.data(), cyc, sizeof(unsigned long long) * grid, hipMemcpyDeviceToHost));
        double mean = 0;
        for (auto v : c) mean += (double)v;
        mean /= grid;
        best_ms = std::min(best_ms, (double)ms);
        best_cyc = std::min(best_cyc, mean);
      }
      const double instr_per_wave = (double)iters * kBodyLen;
      std::printf("%s {\"op\": \"%s\", \"waves_per_simd\": %d, \"cyc_per_instr\": %.3f, \"wall_cyc_per_instr\": %.3f}",
                  first ? " " : ",\n ", kOpNames[op], b, best_cyc / (b * instr_per_wave),
                  best_ms * 1e-3 * clk_hz / (b * instr_per_wave));
      first = false;
    }
  }
  std::printf("\n]}\n");
  CHECK(hipFree(cyc));
  CHECK(hipFree(out));
  return 0;
}
