// Launcher of the masked daily training objectives (objective.hip), called by the C ABI (capi.cpp:
// ddr_daily_objective_f32).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ddr {
constexpr int64_t kObjectiveMaxDays = 8192;         // the longest window (ddr_metrics_f32's limit)
constexpr int64_t kObjectiveMaxGauges = 1 << 24;    // keeps every grid below 2^31 workgroups
constexpr int64_t kObjectiveShortMaxDays = 512;     // up to here one wave owns a gauge, above it one workgroup
constexpr int kObjectiveShortWaves = 4;             // gauges per workgroup of the one-wave kernels
constexpr int kObjectiveGradChunk = 256;            // days of one gauge that a wave of the gradient launch writes

struct ObjectiveArgs {
  const float* daily;
  const float* obs;
  int64_t ds, os;             // row strides in elements
  const unsigned char* drop;  // (G,) non-zero: the gauge contributes nothing; or null
  const float* weight;        // (G,) or null
  const float* count_dev;     // device scalar that overrides the normaliser W, or null
  double count;               // > 0: overrides W (when count_dev is null)
  int64_t G;
  int D, wd, kind;
  double eps;
  float* loss;
  float* grad;  // (G, D) row-major, or null
  double* terms;  // (3, G), or null
  double* work;   // objective_work_bytes(G)
};

size_t objective_work_bytes(int64_t G);
// moments + terms, the fixed-order reduction to the loss and W, then (grad != null) the gradient: 2 or 3 launches
hipError_t launch_objective(const ObjectiveArgs& a, hipStream_t stream);
}  // namespace ddr
