// Launcher of the per-gauge evaluation metrics (metrics.hip), called by the C ABI (capi.cpp: ddr_metrics_f32).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ddr {
constexpr int64_t kMetricsMaxDays = 8192;      // the longest window (one workgroup's LDS holds the series)
constexpr int64_t kMetricsShortMaxDays = 512;  // up to here one wave owns a gauge, above it one workgroup
// out: (DDR_N_METRICS, G) fp64; nan_count: one device word, set to the number of NaN in pred
hipError_t launch_metrics(int64_t G, int64_t D, const float* pred, int64_t pred_stride, const float* target,
                          int64_t target_stride, double* out, int32_t* nan_count, hipStream_t stream);
}  // namespace ddr
