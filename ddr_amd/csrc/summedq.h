// The summed-Q' baseline (summedq.hip): the plan of the per-gauge member lists and its launcher, called by the
// C ABI (capi.cpp: ddr_summedq_*).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ddr_mc.h"

namespace ddr {

// One piece of a gauge's member list: members [begin, begin + count) of the plan's index array.  A list of at
// most `chunk` members is one piece that writes the gauge's output row (slot < 0); a longer one is cut at
// multiples of `chunk` from its start, and piece p writes fp64 partial row first_slot + p of the scratch.
struct SummedQPiece {
  int64_t begin;
  int64_t slot;
  int32_t count;
  int32_t gauge;
};
struct SummedQSplit {  // a gauge with more than one piece
  int64_t first_slot;
  int32_t gauge;
  int32_t n_pieces;
};
struct SummedQPlan {
  int64_t G = 0, nnz = 0, chunk = 0;
  int64_t n_pieces = 0, n_splits = 0, n_slots = 0;
  int32_t max_index = -1;
  int device = -1;  // -1: built without a device (arguments are still checked; a launch fails)
  int32_t* d_idx = nullptr;
  SummedQPiece* d_pieces = nullptr;  // largest first
  SummedQSplit* d_splits = nullptr;
};

ddr_status summedq_plan_create(int64_t G, const int64_t* member_off, const int32_t* member_idx, int64_t chunk,
                               hipStream_t stream, SummedQPlan** plan);
void summedq_plan_destroy(SummedQPlan* plan);
int64_t summedq_scratch_bytes(const SummedQPlan* plan, int64_t D);
ddr_status summedq_run(const SummedQPlan* plan, const float* qr, int64_t n_rows, int64_t row_stride, int64_t T,
                       int32_t rho, float* out, int64_t out_stride, void* scratch, int64_t scratch_bytes,
                       hipStream_t stream);

}  // namespace ddr
