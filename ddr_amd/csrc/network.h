// The network build (network.hip, network_host.cpp): a raw flowpath table (ids, to_ids) in any row order to the
// engine's contract -- strictly lower-triangular COO, upstream reaches numbered first, dendritic, basins contiguous
// -- called by the C ABI (capi.cpp: ddr_network_*).  One deterministic answer, identical bits from both builders:
//   down[i]   the row of to_ids[i] in ids, -1 when no row has that id (an outlet)
//   dropped   the reaches on a cycle of down (a self-loop counts); a kept reach that drained into one is an outlet
//   new index the kept reaches sorted by (basin ascending, dist descending, row ascending): basin = the rank of the
//             reach's outlet row among all outlet rows, dist = edges to that outlet
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/ddr_mc.h"

namespace ddr {

constexpr int64_t kNetworkMaxRows = int64_t(1) << 30;  // refused at and above: dist sums and the sort key stay in range

struct Network {
  int64_t n = 0, kept = 0, nnz = 0, n_dropped = 0, n_basins = 0, max_depth = 0;
  int device = -1;  // -1: built by the host twin, the arrays below are the vectors
  // host build
  std::vector<int32_t> position, down, rows, cols, dropped;
  std::vector<int64_t> order;
  // device build: one block, carved
  void* block = nullptr;
  int32_t *d_position = nullptr, *d_down = nullptr, *d_rows = nullptr, *d_cols = nullptr, *d_dropped = nullptr;
  int64_t* d_order = nullptr;
};

// doubling rounds that cover any acyclic path of an n-row table: the smallest r with 2^r >= n
inline int network_rounds(int64_t n) {
  int r = 0;
  while ((int64_t(1) << r) < n) ++r;
  return r;
}
// bits of the fields of the sort key (basin | n - 1 - dist): values 0..n (n: a dropped reach's basin field)
inline int network_field_bits(int64_t n) {
  int b = 1;
  while ((int64_t(1) << b) <= n) ++b;
  return b;
}

// the checks both builders and both lookups make before anything else (network_host.cpp)
ddr_status network_build_checks(const char* who, int64_t n, const int64_t* ids, const int64_t* to_ids, const void* out);
ddr_status network_lookup_checks(const char* who, int64_t n, const int64_t* ids, int64_t m, const int64_t* queries,
                                 const int32_t* pos);

// network_host.cpp
ddr_status network_build_host(int64_t n, const int64_t* ids, const int64_t* to_ids, Network** out);
ddr_status network_lookup_host(int64_t n, const int64_t* ids, int64_t m, const int64_t* queries, int32_t* pos);

// network.hip
ddr_status network_build(int64_t n, const int64_t* ids, const int64_t* to_ids, int32_t flags, hipStream_t stream,
                         Network** out);
ddr_status network_lookup(int64_t n, const int64_t* ids, int64_t m, const int64_t* queries, int32_t* pos,
                          int32_t flags, hipStream_t stream);
ddr_status network_get(const Network* nw, int32_t* position, int64_t* order, int32_t* down, int32_t* rows,
                       int32_t* cols, int32_t* dropped, hipStream_t stream);
void network_destroy(Network* nw);

}  // namespace ddr
