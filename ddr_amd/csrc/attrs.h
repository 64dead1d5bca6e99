// The per-batch attribute feed (attrs.hip): the batch's catchment attributes, flowpath tensors and flow_scale gathered
// on the device from tables that were uploaded once, called by the C ABI (capi.cpp: ddr_feed_attributes_f32,
// ddr_feed_attr_mean_f32, ddr_feed_flow_scale_f32).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ddr_mc.h"

namespace ddr {

constexpr int kAttrMaxA = DDR_ATTR_MAX_FEATURES;
constexpr int kAttrMeanBlocks = 256;  // partial sums per flagged attribute (ddr_feed_attr_mean_work_bytes)

ddr_status feed_attributes(const float* table, int64_t row_stride, int64_t n_conus, int32_t A, const int32_t* active,
                           int64_t N, const float* fill, const float* means, const float* stds, float* spatial,
                           float* normalized, const ddr_flowpath* path, float* flow_scale, hipStream_t stream);
int64_t feed_attr_mean_work_bytes(int32_t n_flagged);
ddr_status feed_attr_mean(const float* table, int64_t row_stride, int64_t n_conus, int32_t A, const int32_t* active,
                          int64_t N, const int32_t* flagged, int32_t n_flagged, float* fill, void* work,
                          int64_t work_bytes, hipStream_t stream);
ddr_status feed_flow_scale(const int32_t* gage_c, const int32_t* scale_rows, int64_t G, const float* factors,
                           const uint8_t* skip, int64_t n_factors, int64_t N, int32_t* winner, float* flow_scale,
                           hipStream_t stream);

}  // namespace ddr
