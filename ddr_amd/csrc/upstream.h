// The upstream index (upstream.hip, upstream_host.cpp): down[] of a dendritic network, built once, and the
// per-batch queries on it -- the label of every reach (nearest target at or downstream of it), the union
// subnetwork of a gauge batch and the per-gauge member lists -- called by the C ABI (capi.cpp: ddr_upstream_*).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/ddr_mc.h"

namespace ddr {

struct UpstreamIndex {
  int64_t n = 0, n_outlets = 0, max_depth = 0;
  int rounds = 0;             // doubling rounds of a device query: 2^rounds > max_depth
  std::vector<int32_t> down;  // host copy (-1: outlet); down[i] > i
  int device = -1;            // -1: host-only
  int32_t* d_down = nullptr;
};

// doubling rounds that carry every reach past its outlet: ceil(log2(max_depth)) + 1 (0 for a network without edges)
int upstream_rounds(int64_t max_depth);
// the targets of a query checked (DDR_ERR_ARG) and slot_of[g] = the smallest slot on g's reach
ddr_status upstream_slots(const UpstreamIndex* ix, const char* who, int64_t n_targets, const int32_t* targets,
                          std::vector<int32_t>& slot_of);

// upstream_host.cpp
ddr_status upstream_down_host(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                              std::vector<int32_t>& down);
void upstream_depth_host(UpstreamIndex* ix);
ddr_status upstream_label_host(const UpstreamIndex* ix, int64_t n_targets, const int32_t* targets, int32_t* label,
                               int32_t* slot_of);
ddr_status upstream_collate_host(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx, int32_t* active,
                                 int64_t active_cap, int64_t* n_active, int64_t* crow, int32_t* col, int64_t edge_cap,
                                 int64_t* nnz, int64_t* out_off, int32_t* out_idx, int64_t out_idx_cap,
                                 int32_t* gage_c);
ddr_status upstream_member_counts_host(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx,
                                       int64_t* off);
ddr_status upstream_members_host(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx,
                                 const int64_t* off, int32_t* idx);

// upstream.hip
ddr_status upstream_index_create(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols, int32_t flags,
                                 hipStream_t stream, UpstreamIndex** index);
void upstream_index_destroy(UpstreamIndex* ix);
int64_t upstream_scratch_bytes(const UpstreamIndex* ix, int64_t n_targets, int64_t n_members);
ddr_status upstream_label(const UpstreamIndex* ix, int64_t n_targets, const int32_t* targets, int32_t* label,
                          int32_t* slot_of, void* scratch, int64_t scratch_bytes, hipStream_t stream);
ddr_status upstream_collate(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx, int32_t* active,
                            int64_t active_cap, int64_t* n_active, int32_t* rows_c, int32_t* cols_c, int64_t edge_cap,
                            int64_t* nnz, int64_t* crow, int32_t* col, int64_t* out_off, int32_t* out_idx,
                            int64_t out_idx_cap, int32_t* gage_c, void* scratch, int64_t scratch_bytes,
                            hipStream_t stream);
ddr_status upstream_member_counts(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx, int64_t* off,
                                  int64_t* total, void* scratch, int64_t scratch_bytes, hipStream_t stream);
ddr_status upstream_members(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx, int64_t n_members,
                            int32_t* idx, void* scratch, int64_t scratch_bytes, hipStream_t stream);

}  // namespace ddr
