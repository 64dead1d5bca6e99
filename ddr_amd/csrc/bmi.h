// The BMI coupling's device side (bmi.hip): the launchers of the four kernels around the routing launch of one
// coupling interval, called by the C ABI (capi.cpp: ddr_bmi_*).  Arguments are checked by the callers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ddr {

// src_of_seg[key_seg[j]] = max(src_of_seg[..], i) for every i with ids[i] == keys[j]  (keys ascending)
hipError_t launch_bmi_nexus_plan(int64_t M, const int32_t* ids, int64_t n_keys, const int64_t* keys,
                                 const int32_t* key_seg, int64_t N, int32_t* src_of_seg, hipStream_t stream);
// lateral[s] = flows[src[s]] where 0 <= src[s] < M
hipError_t launch_bmi_set_inflow(int64_t N, const int32_t* src, int64_t M, const double* flows, double* lateral,
                                 hipStream_t stream);
// rows 0..K-1 of the fp32 window, row K = row K-1; then prev = cur, cur = 0
hipError_t launch_bmi_window(int64_t N, int K, int n_steps, bool linear, double* prev, double* cur, float* window,
                             int64_t row_stride, hipStream_t stream);
// out rows: discharge copy, velocity, depth
hipError_t launch_bmi_outputs(int64_t N, const float* q, const float* n, const float* q_spatial, const float* p,
                              int64_t p_stride, const float* slope, const float* top_width, const float* side_slope,
                              float depth_lb, float bottom_width_lb, float* out, int64_t out_stride,
                              hipStream_t stream);

}  // namespace ddr
