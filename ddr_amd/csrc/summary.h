// Launcher of the NaN-aware row summaries (summary.hip): count, min, max, mean, std and up to eight exact
// quantiles per row, called by the C ABI (capi.cpp: ddr_summary_f32 / ddr_summary_f64).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ddr {
constexpr int kSummaryMaxQ = 8;             // quantiles per call (DDR_SUMMARY_MAX_Q): 16 tracked ranks
constexpr int kSummaryThreads = 256;        // threads of every workgroup
constexpr int kSummaryTile = 4096;          // elements of a row that a workgroup takes at a time (DDR_SUMMARY_TILE)
constexpr int kSummaryMaxWgs = 256;         // workgroups per row at most: a long row is walked tile by tile
constexpr int kSummaryDigitBits = 8;        // radix digit: 256 bins, 4 passes over fp32 keys and 8 over fp64 keys
constexpr int64_t kSummaryMaxRows = 1 << 20;  // keeps every grid below 2^31 workgroups

struct SummaryArgs {
  const void* x;
  int64_t stride;  // row stride in elements
  int64_t R, N;
  int K, method, flags;
  double q[kSummaryMaxQ];
  double* out;  // (R, 5 + K)
  void* work;   // summary_work_bytes(R, K, elem_bytes), 16-byte aligned
};

size_t summary_work_bytes(int64_t R, int K, int elem_bytes);
// one launch that clears the histograms, one per digit pass (two when K == 0: the moments need two) and one that
// picks the last digit, reduces the partial moments and writes the row's record
template <typename T>
hipError_t launch_summary(const SummaryArgs& a, hipStream_t stream);
}  // namespace ddr
