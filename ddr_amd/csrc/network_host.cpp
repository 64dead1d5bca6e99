// Host twin of the network build (network.hip): the same outputs without a GPU, single-threaded.
//   reference counterparts: engine/src/ddr_engine/merit/build.py:20-107 (create_matrix: rustworkx topological sort,
//   cycle removal, renumbering) and lynker_hydrofabric/io.py:60-154 (create_matrix over flowpaths and nexus points)
#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "internal.h"
#include "network.h"

namespace ddr {

ddr_status network_build_checks(const char* who, int64_t n, const int64_t* ids, const int64_t* to_ids,
                                const void* out) {
  const std::string w(who);
  if (!out) return fail(DDR_ERR_ARG, w + ": null network pointer");
  if (n < 0) return fail(DDR_ERR_ARG, w + ": negative row count");
  if (n >= kNetworkMaxRows)
    return fail(DDR_ERR_ARG, w + ": " + std::to_string(n) + " rows, 2^30 or more are too large a table");
  if (n > 0 && (!ids || !to_ids)) return fail(DDR_ERR_ARG, w + ": null ids or to_ids");
  return DDR_OK;
}

ddr_status network_lookup_checks(const char* who, int64_t n, const int64_t* ids, int64_t m, const int64_t* queries,
                                 const int32_t* pos) {
  const std::string w(who);
  if (n < 0 || m < 0) return fail(DDR_ERR_ARG, w + ": negative count");
  if (n >= kNetworkMaxRows || m >= (int64_t(1) << 31))
    return fail(DDR_ERR_ARG, w + ": too large a table (2^30 rows or more) or query list (2^31 or more)");
  if (n > 0 && !ids) return fail(DDR_ERR_ARG, w + ": null ids");
  if (m > 0 && (!queries || !pos)) return fail(DDR_ERR_ARG, w + ": null queries or output");
  return DDR_OK;
}

namespace {

using Entry = std::pair<int64_t, int32_t>;  // (id, row)

// the table sorted by id; a duplicated id (the smallest one) is refused
ddr_status sorted_table(const char* who, int64_t n, const int64_t* ids, std::vector<Entry>& tab) {
  tab.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) tab[i] = Entry(ids[i], (int32_t)i);
  std::sort(tab.begin(), tab.end());
  for (int64_t i = 0; i + 1 < n; ++i)
    if (tab[i].first == tab[i + 1].first)
      return fail(DDR_ERR_ARG, std::string(who) + ": id " + std::to_string(tab[i].first) + " appears more than once");
  return DDR_OK;
}

inline int32_t find_row(const std::vector<Entry>& tab, int64_t id) {
  auto it = std::lower_bound(tab.begin(), tab.end(), id, [](const Entry& e, int64_t v) { return e.first < v; });
  return it != tab.end() && it->first == id ? it->second : -1;
}

}  // namespace

ddr_status network_lookup_host(int64_t n, const int64_t* ids, int64_t m, const int64_t* queries, int32_t* pos) {
  ddr_status st = network_lookup_checks("network_lookup", n, ids, m, queries, pos);
  if (st) return st;
  std::vector<Entry> tab;
  if ((st = sorted_table("network_lookup", n, ids, tab))) return st;
  for (int64_t k = 0; k < m; ++k) pos[k] = find_row(tab, queries[k]);
  return DDR_OK;
}

ddr_status network_build_host(int64_t n, const int64_t* ids, const int64_t* to_ids, Network** out) {
  ddr_status st = network_build_checks("network_build", n, ids, to_ids, out);
  if (st) return st;
  *out = nullptr;
  auto nw = std::make_unique<Network>();
  nw->n = n;
  std::vector<int32_t> down((size_t)n);
  {
    std::vector<Entry> tab;
    if ((st = sorted_table("network_build", n, ids, tab))) return st;
    for (int64_t i = 0; i < n; ++i) down[i] = find_row(tab, to_ids[i]);
  }
  // cycles of the functional graph: walk from every unvisited row, marking the path; meeting the own path closes one
  std::vector<uint8_t> state((size_t)n, 0), on_cycle((size_t)n, 0);  // state 1: on the current path, 2: finished
  std::vector<int32_t> path;
  for (int64_t i = 0; i < n; ++i) {
    if (state[i]) continue;
    path.clear();
    int32_t j = (int32_t)i;
    while (j >= 0 && state[j] == 0) {
      state[j] = 1;
      path.push_back(j);
      j = down[j];
    }
    if (j >= 0 && state[j] == 1)
      for (size_t k = path.size(); k-- > 0;) {
        on_cycle[path[k]] = 1;
        if (path[k] == j) break;
      }
    for (int32_t p : path) state[p] = 2;
  }
  for (int64_t i = 0; i < n; ++i) {
    if (on_cycle[i]) {
      nw->dropped.push_back((int32_t)i);
      down[i] = -1;
    } else if (down[i] >= 0 && on_cycle[down[i]]) {
      down[i] = -1;  // drained into a dropped reach: an outlet now
    }
  }
  nw->n_dropped = (int64_t)nw->dropped.size();
  nw->kept = n - nw->n_dropped;
  // dist to the outlet and the outlet's row, along paths that now all end
  std::vector<int32_t> dist((size_t)n, -1), root((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i) {
    if (on_cycle[i] || dist[i] >= 0) continue;
    path.clear();
    int32_t j = (int32_t)i;
    while (dist[j] < 0 && down[j] >= 0) {
      path.push_back(j);
      j = down[j];
    }
    if (dist[j] < 0) {
      dist[j] = 0;
      root[j] = j;
    }
    for (size_t k = path.size(); k-- > 0;) {
      const int32_t p = path[k];
      dist[p] = dist[down[p]] + 1;
      root[p] = root[down[p]];
    }
  }
  std::vector<int32_t> basin_of_outlet((size_t)n, -1);
  int32_t nb = 0, deepest = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (on_cycle[i]) continue;
    if (down[i] < 0) basin_of_outlet[i] = nb++;
    deepest = std::max(deepest, dist[i]);
  }
  nw->n_basins = nb;
  nw->max_depth = deepest;
  const int pb = network_field_bits(n);
  std::vector<std::pair<uint64_t, int32_t>> keyed;
  keyed.reserve((size_t)nw->kept);
  for (int64_t i = 0; i < n; ++i)
    if (!on_cycle[i])
      keyed.emplace_back(((uint64_t)basin_of_outlet[root[i]] << pb) | (uint64_t)(n - 1 - dist[i]), (int32_t)i);
  std::sort(keyed.begin(), keyed.end());
  const int64_t m = nw->kept;
  std::vector<int32_t> new_of((size_t)n, -1);
  nw->position.resize((size_t)m);
  nw->order.resize((size_t)m);
  nw->down.resize((size_t)m);
  for (int64_t k = 0; k < m; ++k) {
    nw->position[k] = keyed[k].second;
    new_of[keyed[k].second] = (int32_t)k;
  }
  for (int64_t k = 0; k < m; ++k) {
    const int32_t p = nw->position[k];
    nw->order[k] = ids[p];
    nw->down[k] = down[p] < 0 ? -1 : new_of[down[p]];
    if (nw->down[k] >= 0) {
      nw->rows.push_back(nw->down[k]);
      nw->cols.push_back((int32_t)k);
    }
  }
  nw->nnz = (int64_t)nw->rows.size();
  *out = nw.release();
  return DDR_OK;
}

}  // namespace ddr
