// The per-batch forcing feed (feed.hip): the gathers from the device-resident q' and observation stores, called by
// the C ABI (capi.cpp: ddr_feed_*).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ddr_mc.h"

namespace ddr {

ddr_status feed_qprime(const float* store, int64_t row_stride, int64_t n_rows, int64_t T_store, const int32_t* rows,
                       int64_t N, int64_t t0, int64_t n_cols, int32_t repeat, int64_t T_out, float fill, float* out,
                       uint8_t* valid, hipStream_t stream);
ddr_status feed_rows(const float* store, int64_t row_stride, int64_t n_rows, int64_t T_store, const int32_t* rows,
                     int64_t G, int64_t t0, int64_t n_cols, int32_t trim, float* out, int64_t out_stride,
                     uint8_t* has_nan, hipStream_t stream);

}  // namespace ddr
