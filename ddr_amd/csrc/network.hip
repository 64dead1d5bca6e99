// The network build on the device: a raw flowpath table (ids, to_ids) in any row order to the engine's contract
// (network.h states the one answer; network_host.cpp is the host twin that gives the same bits).
//
//   lookup     radix sort of (id, row) on the signed 64-bit ids; equal neighbours are a duplicate (refused); one
//              binary search per to_id gives down[] (-1: no such row, an outlet)
//   doubling   16-byte states (ptr, dist, root) in two buffers, a round reads one and writes the other (jumping in
//              place is safe for ptr but races on dist); rounds = ceil(log2 n) is fixed from n alone, so nothing is
//              read back per round.  A finished state has ptr = -1, dist = edges to its outlet, root = the outlet's row
//   cycles     a state still unfinished after the last round lies on or upstream of a cycle and its ptr, f^(2^rounds)
//              of the reach, is ON the cycle; f^K permutes every cycle, so the image {ptr[i]} of the unfinished
//              states is exactly the on-cycle set: one scatter of flags.  Only then: the edges into flagged reaches
//              are cut and the doubling runs once more on the cleaned down[]
//   renumber   exclusive scan of the outlet flags (basin = rank of the outlet's row), one 64-bit key per reach,
//              (basin << b) | (n - 1 - dist) with b = bits of n, a dropped reach keyed past every basin; a stable
//              radix sort over the 2 b bits in use of rows given in ascending order breaks ties by row and leaves the
//              dropped rows ascending at the tail; the inverse permutation; the edges compacted in cols order by a
//              second scan
// dist <= 2^rounds < 2 n <= 2^31 - 2 below the refused size, so the int32 sums cannot wrap even on a cycle.  Every
// kernel is a grid-stride loop of 256-thread workgroups over contiguous rows (the states are one 16-byte load and
// store per reach; the gathers follow down[]); no workgroup waits for another.  The build reads the device twice:
// after the first doubling (duplicate?  any cycle?) and at the end (the counts), and is synchronous like
// ddr_upstream_collate.
#include "network.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <memory>
#include <string>

#include "internal.h"

namespace ddr {

namespace {

constexpr int kTB = 256;
constexpr int64_t kMaxGrid = 4096;
inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>(kMaxGrid, std::max<int64_t>(1, (n + kTB - 1) / kTB)); }
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

using word = unsigned long long;
struct alignas(16) State {
  int32_t ptr, dist, root, pad;
};
// agg words (int32): the counts the host reads
enum { kOpen = 0, kDropped = 1, kBasins = 2, kDepth = 3, kNnz = 4, kAggWords = 8 };

#define DDR_GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < (n); i += (int64_t)gridDim.x * kTB)

__global__ void __launch_bounds__(kTB) k_table(int64_t n, const int64_t* ids, int64_t* keys, int32_t* vals) {
  DDR_GRID_STRIDE(i, n) {
    keys[i] = ids[i];
    vals[i] = (int32_t)i;
  }
}
// the smallest sorted position whose neighbour holds the same id (the ids ascend: the smallest duplicated id)
__global__ void __launch_bounds__(kTB) k_duplicate(int64_t n, const int64_t* sorted, word* err) {
  DDR_GRID_STRIDE(i, n - 1)
    if (sorted[i] == sorted[i + 1]) atomicMin(err, (word)i);
}
__global__ void __launch_bounds__(kTB) k_find(int64_t m, int64_t n, const int64_t* sorted, const int32_t* row,
                                              const int64_t* queries, int32_t* pos) {
  DDR_GRID_STRIDE(k, m) {
    const int64_t q = queries[k];
    int64_t lo = 0, hi = n;  // the first entry >= q
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sorted[mid] < q) lo = mid + 1;
      else hi = mid;
    }
    pos[k] = lo < n && sorted[lo] == q ? row[lo] : -1;
  }
}

__global__ void __launch_bounds__(kTB) k_state_init(int64_t n, const int32_t* down, State* st) {
  DDR_GRID_STRIDE(i, n) {
    const int32_t d = down[i];
    st[i] = State{d, d >= 0 ? 1 : 0, d >= 0 ? -1 : (int32_t)i, 0};
  }
}
__global__ void __launch_bounds__(kTB) k_state_round(int64_t n, const State* __restrict__ in, State* __restrict__ out) {
  DDR_GRID_STRIDE(i, n) {
    State s = in[i];
    if (s.ptr >= 0) {
      const State v = in[s.ptr];
      s.ptr = v.ptr;
      s.dist += v.dist;
      s.root = v.root;
    }
    out[i] = s;
  }
}
// flags the image of the unfinished states (every writer stores the same 1) and counts them
__global__ void __launch_bounds__(kTB) k_mark_cycles(int64_t n, const State* st, int32_t* flag, int32_t* agg) {
  int32_t open = 0;
  DDR_GRID_STRIDE(i, n) {
    const int32_t p = st[i].ptr;
    if (p >= 0) {
      flag[p] = 1;
      ++open;
    }
  }
  for (int o = 32; o > 0; o >>= 1) open += __shfl_xor(open, o);
  if ((threadIdx.x & 63) == 0 && open) atomicAdd(agg + kOpen, open);
}
// a flagged reach and a reach that drained into one lose their edge (each thread writes its own row alone)
__global__ void __launch_bounds__(kTB) k_cut(int64_t n, const int32_t* flag, int32_t* down) {
  DDR_GRID_STRIDE(i, n) {
    const int32_t d = down[i];
    if (d >= 0 && (flag[i] || flag[d])) down[i] = -1;
  }
}
__global__ void __launch_bounds__(kTB) k_outlets(int64_t n, const int32_t* flag, const int32_t* down, int32_t* outlet) {
  DDR_GRID_STRIDE(i, n) outlet[i] = !flag[i] && down[i] < 0;
}
// the sort key of every row, its value the row; the deepest kept reach, the dropped count and the basin count
__global__ void __launch_bounds__(kTB) k_keys(int64_t n, int pb, const State* st, const int32_t* flag,
                                              const int32_t* outlet, const int32_t* rank, word* keys, int32_t* vals,
                                              int32_t* agg) {
  int32_t deep = 0, gone = 0;
  DDR_GRID_STRIDE(i, n) {
    const State s = st[i];
    word key;
    if (flag[i] || s.ptr >= 0 || s.root < 0) {  // (ptr >= 0 or root < 0 cannot happen after the cut: kept in bounds)
      key = ((word)n << pb) | (word)(n - 1);
      ++gone;
    } else {
      key = ((word)rank[s.root] << pb) | (word)(n - 1 - s.dist);
      deep = max(deep, s.dist);
    }
    keys[i] = key;
    vals[i] = (int32_t)i;
    if (i == n - 1) agg[kBasins] = rank[i] + outlet[i];
  }
  for (int o = 32; o > 0; o >>= 1) {
    deep = max(deep, __shfl_xor(deep, o));
    gone += __shfl_xor(gone, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (deep) atomicMax(agg + kDepth, deep);
    if (gone) atomicAdd(agg + kDropped, gone);
  }
}
// new_of[row] = the new index of a kept row, -1 of a dropped one (the sorted rows are a permutation: no two writers)
__global__ void __launch_bounds__(kTB) k_inverse(int64_t n, int pb, const word* keys, const int32_t* position,
                                                 int32_t* new_of) {
  DDR_GRID_STRIDE(k, n) new_of[position[k]] = (int64_t)(keys[k] >> pb) == n ? -1 : (int32_t)k;
}
__global__ void __launch_bounds__(kTB) k_emit(int64_t n, int pb, const word* keys, const int32_t* position,
                                              const int32_t* new_of, const int32_t* down, const int64_t* ids,
                                              int64_t* order, int32_t* down_new, int32_t* has_edge) {
  DDR_GRID_STRIDE(k, n) {
    const int32_t p = position[k];
    int32_t dn = -1;
    if ((int64_t)(keys[k] >> pb) != n) {
      const int32_t d = down[p];
      if (d >= 0) dn = new_of[d];
    }
    order[k] = ids[p];
    down_new[k] = dn;
    has_edge[k] = dn >= 0;
  }
}
__global__ void __launch_bounds__(kTB) k_edges(int64_t n, const int32_t* has_edge, const int32_t* at,
                                               const int32_t* down_new, int32_t* rows, int32_t* cols, int32_t* agg) {
  DDR_GRID_STRIDE(k, n) {
    if (has_edge[k]) {
      rows[at[k]] = down_new[k];
      cols[at[k]] = (int32_t)k;
    }
    if (k == n - 1) agg[kNnz] = at[k] + has_edge[k];
  }
}

struct Free {
  void operator()(void* p) const { (void)hipFree(p); }
};
using DevBlock = std::unique_ptr<void, Free>;

struct Carver {
  char* p;
  template <typename T>
  T* take(int64_t count) {
    T* r = reinterpret_cast<T*>(p);
    p += align256(std::max<int64_t>(count, 1) * (int64_t)sizeof(T));
    return r;
  }
};

// temporary storage of the largest hipcub call of a build over n rows
ddr_status temp_bytes(int64_t n, int pb, size_t* bytes) {
  size_t a = 0, b = 0, c = 0;
  DDR_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, a, static_cast<const int64_t*>(nullptr),
                                             static_cast<int64_t*>(nullptr), static_cast<const int32_t*>(nullptr),
                                             static_cast<int32_t*>(nullptr), (int)n, 0, 64, (hipStream_t) nullptr));
  DDR_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, b, static_cast<const word*>(nullptr), static_cast<word*>(nullptr),
                                             static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr),
                                             (int)n, 0, 2 * pb, (hipStream_t) nullptr));
  DDR_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, c, static_cast<const int32_t*>(nullptr),
                                           static_cast<int32_t*>(nullptr), (int)n, (hipStream_t) nullptr));
  *bytes = std::max(a, std::max(b, c));
  return DDR_OK;
}

// the table sorted by id on the device (keys, rows) and the duplicate word; nothing is read back here
ddr_status sort_table(int64_t n, const int64_t* d_ids, int64_t* keys_in, int32_t* vals_in, int64_t* keys, int32_t* rows,
                      void* temp, size_t tbytes, word* err, hipStream_t s) {
  hipLaunchKernelGGL(k_table, dim3(grid_for(n)), dim3(kTB), 0, s, n, d_ids, keys_in, vals_in);
  DDR_HIP(hipGetLastError());
  DDR_HIP(hipcub::DeviceRadixSort::SortPairs(temp, tbytes, keys_in, keys, vals_in, rows, (int)n, 0, 64, s));
  DDR_HIP(hipMemsetAsync(err, 0xFF, sizeof(word), s));
  if (n > 1) hipLaunchKernelGGL(k_duplicate, dim3(grid_for(n - 1)), dim3(kTB), 0, s, n, keys, err);
  DDR_HIP(hipGetLastError());
  return DDR_OK;
}

ddr_status duplicate_refusal(const char* who, word at, const int64_t* sorted_keys) {
  int64_t id = 0;
  DDR_HIP(hipMemcpy(&id, sorted_keys + at, sizeof(id), hipMemcpyDeviceToHost));
  return fail(DDR_ERR_ARG, std::string(who) + ": id " + std::to_string(id) + " appears more than once");
}

ddr_status current_device_alloc(size_t bytes, DevBlock& blk) {
  void* raw = nullptr;
  DDR_HIP(hipMalloc(&raw, std::max<size_t>(bytes, 256)));
  blk.reset(raw);
  return DDR_OK;
}

}  // namespace

ddr_status network_lookup(int64_t n, const int64_t* ids, int64_t m, const int64_t* queries, int32_t* pos,
                          int32_t flags, hipStream_t s) {
  ddr_status st = network_lookup_checks("network_lookup", n, ids, m, queries, pos);
  if (st) return st;
  if (flags & ~DDR_NETWORK_DEVICE_INPUT) return fail(DDR_ERR_ARG, "network_lookup: unknown flag");
  const bool dev_in = flags & DDR_NETWORK_DEVICE_INPUT;
  size_t tbytes = 0;
  if (n > 0 && (st = temp_bytes(n, 1, &tbytes))) return st;
  const int64_t n1 = std::max<int64_t>(n, 1), m1 = std::max<int64_t>(m, 1);  // (Carver::take rounds a count of 0 up)
  DevBlock blk;
  if ((st = current_device_alloc(
           (size_t)(2 * align256(8 * n1) + 2 * align256(4 * n1) + align256(std::max<int64_t>((int64_t)tbytes, 1)) + 256 +
                    (dev_in ? 0 : align256(8 * n1) + align256(8 * m1) + align256(4 * m1))),
           blk)))
    return st;
  Carver c{static_cast<char*>(blk.get())};
  int64_t* keys_in = c.take<int64_t>(n);
  int64_t* keys = c.take<int64_t>(n);
  int32_t* vals_in = c.take<int32_t>(n);
  int32_t* rows = c.take<int32_t>(n);
  void* temp = c.take<char>((int64_t)tbytes);
  word* err = c.take<word>(1);
  const int64_t* d_ids = ids;
  const int64_t* d_q = queries;
  int32_t* d_pos = pos;
  if (!dev_in) {
    int64_t* up_ids = c.take<int64_t>(n);
    int64_t* up_q = c.take<int64_t>(m);
    d_pos = c.take<int32_t>(m);
    if (n > 0) DDR_HIP(hipMemcpyAsync(up_ids, ids, sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
    if (m > 0) DDR_HIP(hipMemcpyAsync(up_q, queries, sizeof(int64_t) * m, hipMemcpyHostToDevice, s));
    d_ids = up_ids;
    d_q = up_q;
  }
  word herr = ~(word)0;
  if (n > 0) {
    if ((st = sort_table(n, d_ids, keys_in, vals_in, keys, rows, temp, tbytes, err, s))) return st;
    DDR_HIP(hipMemcpyAsync(&herr, err, sizeof(word), hipMemcpyDeviceToHost, s));
  }
  if (m > 0) {
    hipLaunchKernelGGL(k_find, dim3(grid_for(m)), dim3(kTB), 0, s, m, n, keys, rows, d_q, d_pos);
    DDR_HIP(hipGetLastError());
    if (!dev_in) DDR_HIP(hipMemcpyAsync(pos, d_pos, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
  }
  DDR_HIP(hipStreamSynchronize(s));
  if (herr != ~(word)0) return duplicate_refusal("network_lookup", herr, keys);
  return DDR_OK;
}

ddr_status network_build(int64_t n, const int64_t* ids, const int64_t* to_ids, int32_t flags, hipStream_t s,
                         Network** out) {
  ddr_status st = network_build_checks("network_build", n, ids, to_ids, out);
  if (st) return st;
  *out = nullptr;
  if (flags & ~DDR_NETWORK_DEVICE_INPUT) return fail(DDR_ERR_ARG, "network_build: unknown flag");
  const bool dev_in = flags & DDR_NETWORK_DEVICE_INPUT;
  auto nw = std::make_unique<Network>();
  nw->n = n;
  DDR_HIP(hipGetDevice(&nw->device));
  if (n == 0) {
    *out = nw.release();
    return DDR_OK;
  }
  const int pb = network_field_bits(n);
  size_t tbytes = 0;
  if ((st = temp_bytes(n, pb, &tbytes))) return st;
  DevBlock scratch, result;
  if ((st = current_device_alloc((size_t)((dev_in ? 2 : 4) * align256(8 * n) + 8 * align256(4 * n) +
                                          2 * align256(16 * n) + align256((int64_t)tbytes) + 2048),
                                 scratch)))
    return st;
  if ((st = current_device_alloc((size_t)(4 * align256(4 * n) + align256(8 * n)), result))) return st;
  Carver c{static_cast<char*>(scratch.get())};
  int64_t* keys_a = c.take<int64_t>(n);  // the id sort's, then the renumbering sort's keys
  int64_t* keys_b = c.take<int64_t>(n);
  int32_t* vals_a = c.take<int32_t>(n);
  int32_t* vals_b = c.take<int32_t>(n);
  int32_t* down = c.take<int32_t>(n);
  int32_t* flag = c.take<int32_t>(n);
  int32_t* mask = c.take<int32_t>(n);   // outlet flags, then has-edge flags
  int32_t* scan = c.take<int32_t>(n);   // their exclusive sums
  int32_t* new_of = c.take<int32_t>(n);
  State* st_a = c.take<State>(n);
  State* st_b = c.take<State>(n);
  void* temp = c.take<char>((int64_t)tbytes);
  word* err = c.take<word>(1);
  int32_t* agg = c.take<int32_t>(kAggWords);
  const int64_t* d_ids = ids;
  const int64_t* d_to = to_ids;
  if (!dev_in) {
    int64_t* up_ids = c.take<int64_t>(n);
    int64_t* up_to = c.take<int64_t>(n);
    DDR_HIP(hipMemcpyAsync(up_ids, ids, sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
    DDR_HIP(hipMemcpyAsync(up_to, to_ids, sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
    d_ids = up_ids;
    d_to = up_to;
  }
  Carver r{static_cast<char*>(result.get())};
  int32_t* position = r.take<int32_t>(n);
  int32_t* down_new = r.take<int32_t>(n);
  int32_t* rows = r.take<int32_t>(n);
  int32_t* cols = r.take<int32_t>(n);
  int64_t* order = r.take<int64_t>(n);
  const dim3 grid(grid_for(n)), block(kTB);

  // lookup
  if ((st = sort_table(n, d_ids, keys_a, vals_a, keys_b, vals_b, temp, tbytes, err, s))) return st;
  hipLaunchKernelGGL(k_find, grid, block, 0, s, n, n, keys_b, vals_b, d_to, down);
  // doubling, and the image of what it left unfinished
  const int rounds = network_rounds(n);
  State *cur = st_a, *nxt = st_b;
  auto doubling = [&]() {
    cur = st_a, nxt = st_b;
    hipLaunchKernelGGL(k_state_init, grid, block, 0, s, n, down, cur);
    for (int k = 0; k < rounds; ++k) {
      hipLaunchKernelGGL(k_state_round, grid, block, 0, s, n, cur, nxt);
      std::swap(cur, nxt);
    }
  };
  doubling();
  DDR_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t) * n, s));
  DDR_HIP(hipMemsetAsync(agg, 0, sizeof(int32_t) * kAggWords, s));
  hipLaunchKernelGGL(k_mark_cycles, grid, block, 0, s, n, cur, flag, agg);
  DDR_HIP(hipGetLastError());
  word herr = ~(word)0;
  int32_t hagg[kAggWords] = {};
  DDR_HIP(hipMemcpyAsync(&herr, err, sizeof(word), hipMemcpyDeviceToHost, s));
  DDR_HIP(hipMemcpyAsync(hagg, agg, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  DDR_HIP(hipStreamSynchronize(s));
  if (herr != ~(word)0) return duplicate_refusal("network_build", herr, keys_b);
  if (hagg[kOpen] > 0) {
    hipLaunchKernelGGL(k_cut, grid, block, 0, s, n, flag, down);
    doubling();
  }
  // renumbering
  hipLaunchKernelGGL(k_outlets, grid, block, 0, s, n, flag, down, mask);
  DDR_HIP(hipGetLastError());
  DDR_HIP(hipcub::DeviceScan::ExclusiveSum(temp, tbytes, mask, scan, (int)n, s));
  word* keys_in = reinterpret_cast<word*>(keys_a);
  word* keys = reinterpret_cast<word*>(keys_b);
  hipLaunchKernelGGL(k_keys, grid, block, 0, s, n, pb, cur, flag, mask, scan, keys_in, vals_a, agg);
  DDR_HIP(hipGetLastError());
  DDR_HIP(hipcub::DeviceRadixSort::SortPairs(temp, tbytes, keys_in, keys, vals_a, position, (int)n, 0, 2 * pb, s));
  hipLaunchKernelGGL(k_inverse, grid, block, 0, s, n, pb, keys, position, new_of);
  hipLaunchKernelGGL(k_emit, grid, block, 0, s, n, pb, keys, position, new_of, down, d_ids, order, down_new, mask);
  DDR_HIP(hipGetLastError());
  DDR_HIP(hipcub::DeviceScan::ExclusiveSum(temp, tbytes, mask, scan, (int)n, s));
  hipLaunchKernelGGL(k_edges, grid, block, 0, s, n, mask, scan, down_new, rows, cols, agg);
  DDR_HIP(hipGetLastError());
  DDR_HIP(hipMemcpyAsync(hagg, agg, sizeof(hagg), hipMemcpyDeviceToHost, s));
  DDR_HIP(hipStreamSynchronize(s));
  nw->n_dropped = hagg[kDropped];
  nw->kept = n - nw->n_dropped;
  nw->n_basins = hagg[kBasins];
  nw->max_depth = hagg[kDepth];
  nw->nnz = hagg[kNnz];
  nw->d_position = position;
  nw->d_dropped = position + nw->kept;  // the dropped rows sorted last, ascending
  nw->d_down = down_new;
  nw->d_rows = rows;
  nw->d_cols = cols;
  nw->d_order = order;
  nw->block = result.release();
  *out = nw.release();
  return DDR_OK;
}

ddr_status network_get(const Network* nw, int32_t* position, int64_t* order, int32_t* down, int32_t* rows,
                       int32_t* cols, int32_t* dropped, hipStream_t s) {
  if (!nw) return fail(DDR_ERR_ARG, "network_get: null network");
  if (nw->device < 0) {
    if (position) std::copy(nw->position.begin(), nw->position.end(), position);
    if (order) std::copy(nw->order.begin(), nw->order.end(), order);
    if (down) std::copy(nw->down.begin(), nw->down.end(), down);
    if (rows) std::copy(nw->rows.begin(), nw->rows.end(), rows);
    if (cols) std::copy(nw->cols.begin(), nw->cols.end(), cols);
    if (dropped) std::copy(nw->dropped.begin(), nw->dropped.end(), dropped);
    return DDR_OK;
  }
  if (!nw->block) return DDR_OK;  // (an empty device network)
  const struct {
    void* dst;
    const void* src;
    int64_t bytes;
  } parts[] = {{position, nw->d_position, 4 * nw->kept}, {order, nw->d_order, 8 * nw->kept},
               {down, nw->d_down, 4 * nw->kept},         {rows, nw->d_rows, 4 * nw->nnz},
               {cols, nw->d_cols, 4 * nw->nnz},          {dropped, nw->d_dropped, 4 * nw->n_dropped}};
  for (const auto& p : parts)
    if (p.dst && p.bytes > 0) DDR_HIP(hipMemcpyAsync(p.dst, p.src, (size_t)p.bytes, hipMemcpyDefault, s));
  DDR_HIP(hipStreamSynchronize(s));
  return DDR_OK;
}

void network_destroy(Network* nw) {
  if (!nw) return;
  if (nw->block) (void)hipFree(nw->block);
  delete nw;
}

}  // namespace ddr
