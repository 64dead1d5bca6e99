// Host twin of the upstream index (upstream.hip).  Upstream reaches are numbered first (down[i] > i), so one
// descending sweep gives every reach the label of its downstream reach: no recursion, no graph library.
//   reference counterparts: engine/src/ddr_engine/merit/graph.py:89-115 (subset_upstream: rx.ancestors per gauge),
//   src/ddr/geodatazoo/merit.py:321-396 (_build_routing_data_target_catchments: rx.ancestors per target and a
//   mask over every CONUS edge)
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "internal.h"
#include "upstream.h"

namespace ddr {

int upstream_rounds(int64_t max_depth) {
  if (max_depth <= 0) return 0;
  int r = 0;
  while ((int64_t(1) << r) < max_depth) ++r;  // ceil(log2(max_depth))
  return r + 1;
}

ddr_status upstream_slots(const UpstreamIndex* ix, const char* who, int64_t n_targets, const int32_t* targets,
                          std::vector<int32_t>& slot_of) {
  const std::string w(who);
  if (!ix) return fail(DDR_ERR_ARG, w + ": null index");
  if (n_targets < 0) return fail(DDR_ERR_ARG, w + ": negative target count");
  if (n_targets > INT32_MAX) return fail(DDR_ERR_ARG, w + ": too many targets");
  if (n_targets > 0 && !targets) return fail(DDR_ERR_ARG, w + ": null targets");
  slot_of.resize((size_t)n_targets);
  std::unordered_map<int32_t, int32_t> first;
  first.reserve((size_t)n_targets * 2);
  for (int64_t g = 0; g < n_targets; ++g) {
    const int32_t t = targets[g];
    if (t < 0 || t >= ix->n)
      return fail(DDR_ERR_ARG, w + ": target " + std::to_string(g) + " (reach " + std::to_string(t) +
                                   ") is outside [0, " + std::to_string(ix->n) + ")");
    slot_of[g] = first.emplace(t, (int32_t)g).first->second;
  }
  return DDR_OK;
}

ddr_status upstream_down_host(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                              std::vector<int32_t>& down) {
  down.assign((size_t)n, -1);
  for (int64_t k = 0; k < e; ++k) {
    const int32_t r = rows[k], c = cols[k];
    if (r < 0 || r >= n || c < 0 || c >= n)
      return fail(DDR_ERR_ARG, "upstream_index_create: edge " + std::to_string(k) + " (" + std::to_string(r) + "," +
                                   std::to_string(c) + ") is out of range");
    if (r <= c)
      return fail(DDR_ERR_NOT_LOWER, "upstream_index_create: entry (" + std::to_string(r) + "," + std::to_string(c) +
                                         ") is not strictly lower triangular");
    if (down[c] < 0) down[c] = r;
    else if (down[c] != r)  // (the same edge twice is accepted, as the batch union accepts it)
      return fail(DDR_ERR_NOT_DENDRITIC, "upstream_index_create: reach " + std::to_string(c) + " drains into " +
                                             std::to_string(down[c]) + " and " + std::to_string(r));
  }
  return DDR_OK;
}

void upstream_depth_host(UpstreamIndex* ix) {
  const int64_t n = ix->n;
  std::vector<int32_t> depth((size_t)n);
  int64_t outlets = 0;
  int32_t deepest = 0;
  for (int64_t i = n - 1; i >= 0; --i) {
    const int32_t d = ix->down[i];
    depth[i] = d < 0 ? 0 : depth[d] + 1;
    outlets += d < 0;
    deepest = std::max(deepest, depth[i]);
  }
  ix->n_outlets = outlets;
  ix->max_depth = deepest;
  ix->rounds = upstream_rounds(deepest);
}

namespace {

// label of every reach and the slots; `label` has n entries
ddr_status sweep(const UpstreamIndex* ix, const char* who, int64_t n_targets, const int32_t* targets, int32_t* label,
                 std::vector<int32_t>& slot_of) {
  ddr_status st = upstream_slots(ix, who, n_targets, targets, slot_of);
  if (st) return st;
  std::fill(label, label + ix->n, -1);
  for (int64_t g = 0; g < n_targets; ++g)
    if (slot_of[g] == g) label[targets[g]] = (int32_t)g;
  for (int64_t i = ix->n - 1; i >= 0; --i)
    if (label[i] < 0 && ix->down[i] >= 0) label[i] = label[ix->down[i]];
  return DDR_OK;
}

// the gauge downstream of gauge g in the gauge forest (-1: none)
inline int32_t parent_of(const UpstreamIndex* ix, const int32_t* label, int32_t reach) {
  const int32_t d = ix->down[reach];
  return d < 0 ? -1 : label[d];
}

}  // namespace

ddr_status upstream_label_host(const UpstreamIndex* ix, int64_t n_targets, const int32_t* targets, int32_t* label,
                               int32_t* slot_of) {
  if (ix && !label) return fail(DDR_ERR_ARG, "upstream_label: null label_out");
  std::vector<int32_t> slots;
  ddr_status st = sweep(ix, "upstream_label", n_targets, targets, label, slots);
  if (st) return st;
  if (slot_of) std::copy(slots.begin(), slots.end(), slot_of);
  return DDR_OK;
}

ddr_status upstream_collate_host(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx, int32_t* active,
                                 int64_t active_cap, int64_t* n_active, int64_t* crow, int32_t* col, int64_t edge_cap,
                                 int64_t* nnz, int64_t* out_off, int32_t* out_idx, int64_t out_idx_cap,
                                 int32_t* gage_c) {
  if (!ix) return fail(DDR_ERR_ARG, "upstream_collate: null index");
  if (active_cap < 0 || edge_cap < 0 || out_idx_cap < 0) return fail(DDR_ERR_ARG, "upstream_collate: negative capacity");
  std::vector<int32_t> label((size_t)ix->n), slots;
  ddr_status st = sweep(ix, "upstream_collate", n_gauges, gage_idx, label.data(), slots);
  if (st) return st;
  if (!active || !n_active || !crow || !nnz || !out_off || (n_gauges > 0 && (!out_idx || !gage_c)))
    return fail(DDR_ERR_ARG, "upstream_collate: null output");
  std::vector<int32_t> rows, cols;
  int64_t members = 0;
  for (int64_t i = 0; i < ix->n; ++i) {
    if (label[i] < 0) continue;
    ++members;
    const int32_t d = ix->down[i];
    if (d >= 0 && label[d] >= 0) {
      rows.push_back(d);
      cols.push_back((int32_t)i);
    }
  }
  const int64_t e = (int64_t)rows.size();
  if (members > active_cap)
    return fail(DDR_ERR_ARG, "upstream_collate: the closure's " + std::to_string(members) +
                                 " reaches exceed active_cap (" + std::to_string(active_cap) + ")");
  if (e > edge_cap || (e > 0 && !col))
    return fail(DDR_ERR_ARG, "upstream_collate: the closure's " + std::to_string(e) + " edges exceed edge_cap (" +
                                 std::to_string(edge_cap) + ")");
  std::vector<int64_t> sub_off((size_t)n_gauges + 1, e);
  sub_off[0] = 0;
  return collate_gauges(ix->n, n_gauges, sub_off.data(), rows.data(), cols.data(), gage_idx, active, n_active, crow,
                        col, nnz, out_off, out_idx, out_idx_cap, gage_c);
}

ddr_status upstream_member_counts_host(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx,
                                       int64_t* off) {
  if (!ix) return fail(DDR_ERR_ARG, "upstream_member_counts: null index");
  std::vector<int32_t> label((size_t)ix->n), slots;
  ddr_status st = sweep(ix, "upstream_member_counts", n_gauges, gage_idx, label.data(), slots);
  if (st) return st;
  if (!off) return fail(DDR_ERR_ARG, "upstream_member_counts: null off");
  std::vector<int64_t> cnt((size_t)n_gauges, 0);
  for (int64_t i = 0; i < ix->n; ++i)
    for (int32_t g = label[i]; g >= 0; g = parent_of(ix, label.data(), gage_idx[g])) ++cnt[g];
  off[0] = 0;
  for (int64_t g = 0; g < n_gauges; ++g) off[g + 1] = off[g] + cnt[slots[g]];
  if (off[n_gauges] >= (int64_t(1) << 31))
    return fail(DDR_ERR_ARG, "upstream_member_counts: the member lists hold " + std::to_string(off[n_gauges]) +
                                 " entries, 2^31 or more do not fit int32 offsets downstream");
  return DDR_OK;
}

ddr_status upstream_members_host(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx,
                                 const int64_t* off, int32_t* idx) {
  if (!ix) return fail(DDR_ERR_ARG, "upstream_members: null index");
  std::vector<int32_t> label((size_t)ix->n), slots;
  ddr_status st = sweep(ix, "upstream_members", n_gauges, gage_idx, label.data(), slots);
  if (st) return st;
  if (!off || (n_gauges > 0 && !idx)) return fail(DDR_ERR_ARG, "upstream_members: null argument");
  std::vector<int64_t> want((size_t)n_gauges + 1);
  if ((st = upstream_member_counts_host(ix, n_gauges, gage_idx, want.data()))) return st;
  if (!std::equal(want.begin(), want.end(), off))
    return fail(DDR_ERR_ARG, "upstream_members: off is not what ddr_upstream_member_counts gives for these gauges");
  std::vector<int64_t> fill(off, off + n_gauges);
  for (int64_t i = 0; i < ix->n; ++i)  // ascending i: every list comes out ascending
    for (int32_t g = label[i]; g >= 0; g = parent_of(ix, label.data(), gage_idx[g])) idx[fill[g]++] = (int32_t)i;
  for (int64_t g = 0; g < n_gauges; ++g)
    if (slots[g] != g) std::copy(idx + off[slots[g]], idx + off[slots[g] + 1], idx + off[g]);
  return DDR_OK;
}

}  // namespace ddr
