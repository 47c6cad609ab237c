#!/usr/bin/env bash
# Host-only sanitizer builds of the native runtime + the job-epoch race stress.
# Usage: tools/sanitize/run.sh [seconds-per-run]   (also: make sanitize)
# GPU sanitizers are not used (no GPU ASan/XNACK on this pool): this covers the C++ host code only.
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
OUT="${OTEDAMA_SANITIZE_OUT:-$ROOT/build/sanitize}"
SECS="${1:-4}"
mkdir -p "$OUT"
SRCS=("$ROOT/csrc/cpu/sha256_cpu.cpp" "$ROOT/csrc/cpu/job_prepare.cpp" "$ROOT/csrc/cpu/aead.cpp" "$ROOT/csrc/cpu/x11_cpu.cpp"
      "$ROOT/csrc/runtime/miner_common.cpp" "$ROOT/tools/sanitize/stress_runtime.cpp")
# ROCm clang: its compiler-rt TSan intercepts pthread_cond_clockwait (libstdc++ wait_for);
# GCC 11's libtsan does not and reports a false "double lock" on the pause path.
CXX="${CXX:-/opt/rocm/lib/llvm/bin/clang++}"
FLAGS=(-std=c++17 -O1 -g -fno-omit-frame-pointer -march=x86-64-v2 "-I$ROOT/csrc/include" -pthread
       -DOTEDAMA_STRESS_HOOKS)

declare -A SAN=([tsan]="-fsanitize=thread" [asan]="-fsanitize=address,undefined -fno-sanitize-recover=undefined")
rc=0
for name in tsan asan; do
  bin="$OUT/stress_runtime_$name"
  # shellcheck disable=SC2086
  "$CXX" "${FLAGS[@]}" ${SAN[$name]} "${SRCS[@]}" -o "$bin" -lcrypto
  echo "== $name: $bin $SECS"
  if [ "$name" = tsan ]; then
    TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1" "$bin" "$SECS" || rc=$?
  else
    ASAN_OPTIONS="detect_leaks=1 abort_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" "$bin" "$SECS" || rc=$?
  fi
  [ "$rc" -eq 0 ] || { echo "$name run failed (rc=$rc)"; exit "$rc"; }
done
# The share job block (csrc/cpu/share_job.cpp) under ASan + UBSan: builder and walker over the length grid of the CPU
# tests, and the limit violations. A stand-alone program, host code only.
sj="$OUT/share_job_check"
# shellcheck disable=SC2086
"$CXX" "${FLAGS[@]}" ${SAN[asan]} "$ROOT/csrc/cpu/sha256_cpu.cpp" "$ROOT/csrc/cpu/share_job.cpp" \
  "$ROOT/tools/sanitize/share_job_check.cpp" -o "$sj" -lcrypto
echo "== share job block: $sj"
ASAN_OPTIONS="detect_leaks=1 abort_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" "$sj" || { echo "share_job_check failed"; exit 1; }
# The template tree's CPU twin (csrc/cpu/merkle_tree.cpp) under ASan + UBSan: exactly sized buffers over the chunk
# edges, the roots against a fold written out in the check. A stand-alone program, host code only.
mt="$OUT/merkle_tree_check"
# shellcheck disable=SC2086
"$CXX" "${FLAGS[@]}" ${SAN[asan]} "$ROOT/csrc/cpu/sha256_cpu.cpp" "$ROOT/csrc/cpu/merkle_tree.cpp" \
  "$ROOT/tools/sanitize/merkle_tree_check.cpp" -o "$mt" -lcrypto
echo "== template tree: $mt"
ASAN_OPTIONS="detect_leaks=1 abort_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" "$mt" || { echo "merkle_tree_check failed"; exit 1; }
# The batched secp256k1 multiplication's CPU twin (csrc/cpu/secp256k1.cpp) under ASan + UBSan against OpenSSL's
# EC_POINT_mul: special scalars, 2,000 random rows, batches of 1 and 65536, the bad rows. A stand-alone program, at -O2:
# the 65536-row batch is 300 million field multiplications.
sp="$OUT/secp256k1_check"
# shellcheck disable=SC2086
"$CXX" "${FLAGS[@]}" -O2 ${SAN[asan]} "$ROOT/csrc/cpu/secp256k1.cpp" "$ROOT/tools/sanitize/secp256k1_check.cpp" -o "$sp" -lcrypto
echo "== secp256k1: $sp"
ASAN_OPTIONS="detect_leaks=1 abort_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" "$sp" || { echo "secp256k1_check failed"; exit 1; }
# The frame seal's arithmetic (csrc/include/otedama/chacha_poly.h, what the gfx950 kernel runs) and its OpenSSL twin
# (csrc/cpu/aead.cpp) under ASan + UBSan against one EVP seal a frame: every length 0..130 and the block edges, batches
# of 1 to 257, Poly1305 rows against the big-integer table and OpenSSL, the refused heads. A stand-alone program.
cp="$OUT/chacha_poly_check"
# shellcheck disable=SC2086
"$CXX" "${FLAGS[@]}" ${SAN[asan]} "$ROOT/csrc/cpu/aead.cpp" "$ROOT/tools/sanitize/chacha_poly_check.cpp" -o "$cp" -lcrypto
echo "== chacha20-poly1305: $cp"
ASAN_OPTIONS="detect_leaks=1 abort_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" "$cp" || { echo "chacha_poly_check failed"; exit 1; }
# libFuzzer (ASan + UBSan) over the SV2 frame scanner and the CPU hash paths.
fz="$OUT/fuzz_native"
"$CXX" -std=c++17 -O1 -g -march=x86-64-v2 "-I$ROOT/csrc/include" -fsanitize=fuzzer,address,undefined \
  -fno-sanitize-recover=undefined -mllvm -asan-globals=0 "$ROOT/tools/sanitize/fuzz_native.cpp" \
  "$ROOT/csrc/cpu/sv2_frame.cpp" "$ROOT/csrc/cpu/sha256_cpu.cpp" "$ROOT/csrc/cpu/x11_cpu.cpp" -o "$fz" -lcrypto
echo "== fuzz: $fz ${SECS}s"
(cd "$OUT" && "$fz" -max_total_time="$SECS" -max_len=2048 -print_final_stats=1) || { echo "fuzz failed"; exit 1; }
echo "sanitize: tsan + asan/ubsan + fuzz clean"
