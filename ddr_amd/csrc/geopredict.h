// Launchers of the geometry predictor's two kernels (geopredict.hip), called by the C ABI (capi.cpp:
// ddr_attr_prepare_f32, ddr_geometry_predict_f32).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ddr {

constexpr int kGeoMaxF = 32;                           // the KAN's kKanMaxF (kan.h)
constexpr int64_t kGeoMaxRows = int64_t(1) << 38;      // one 256-row tile per workgroup: < 2^31 workgroups

// One denormalisation slot with its constants already rounded to fp32 (capi.cpp: geom_slot)
struct GeoSlot {
  int32_t column;  // column of u, or -1: `value`
  int32_t log_space;
  float a, b;      // linear: u * a + b with a = hi - lo, b = lo; log space: exp(u * a + b) with a = log_hi - log_lo, b = log_lo
  float value;
};

// raw: F columns of N floats (feature f at raw + f * feat_stride); x: (N, F) row-major; counts: (3, F) int64,
// zeroed by the caller, or NULL
hipError_t launch_attr_prepare(int64_t N, int F, const float* raw, int64_t feat_stride, const double* scale,
                               const double* offset, const int32_t* log10_flag, const float* mean, const float* std,
                               const float* p10, const float* p90, float* x, long long* counts, hipStream_t stream);
// u: (N, O); slots: n, q_spatial, p_spatial; out: DDR_N_GEOM rows of out_stride floats -- or, without discharge
// and slope, the three parameter rows n, p_spatial, q_spatial alone
hipError_t launch_geometry_predict(int64_t N, int O, const float* u, const GeoSlot (&slots)[3], const float* discharge,
                                   const float* slope, float discharge_lb, float slope_lb, float depth_lb,
                                   float bottom_width_lb, float* out, int64_t out_stride, hipStream_t stream);

}  // namespace ddr
