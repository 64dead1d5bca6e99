// The upstream index on the device: everything upstream of a set of reaches, from down[] alone.
//
// The network is dendritic and lower triangular (down[i] > i, -1 at an outlet), so "upstream of target t" is
// "t lies on the path from the reach to its outlet".  A query labels every reach with the slot of the nearest
// target at or downstream of it (-1: none) by pointer doubling over one 64-bit word per reach,
//   word = (label << 32) | jump      label >= 0: final;  label < 0: no target on the path [reach, jump), jump = -1
//                                    once the path has left the network
// starting from (slot, reach) at a target and (-1, down) elsewhere.  A round replaces an unfinished reach's word
// by the word of its jump reach.  The words are updated in place with single 8-byte relaxed atomic loads and
// stores: a reader sees a neighbour's word of this round or of the last one, never a torn pair, and either obeys
// the invariant above, so a round at least doubles the distance covered.  rounds = ceil(log2(max_depth)) + 1,
// fixed when the index is built: 2^rounds > max_depth hops carry the deepest reach past its outlet, and no query
// reads the device to know when to stop.  Every kernel is a grid-stride loop of 256-thread workgroups; no
// workgroup waits for another.
//
// From the labels:
//   collate   the closure's edges {(down[i], i) : label[i] >= 0 and label[down[i]] >= 0} are appended to a COO
//             (one atomic per wave; the order is arbitrary, the union canonicalises) and handed to the device union
//             of ddr_collate_gauges_device
//   members   the gauges form a forest, parent[g] = label[down[reach(g)]]; reach i belongs to gauge label[i] and
//             to every gauge on that gauge's chain.  Counts by one (wave-aggregated) atomic per (reach, chain
//             gauge), a scan, emission of (gauge * n + reach) keys, one radix sort: ascending lists whatever the
//             order the atomics ran in.  Gauges sharing a reach (aliases) copy the list of the smallest slot.
// Scratch comes from the caller; the query path allocates nothing of its own.
#include "upstream.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "internal.h"

namespace ddr {

namespace {

constexpr int kTB = 256;
constexpr int64_t kMaxGrid = 4096;
inline unsigned grid_for(int64_t n) { return (unsigned)std::min<int64_t>(kMaxGrid, std::max<int64_t>(1, (n + kTB - 1) / kTB)); }
inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

using word = unsigned long long;
__host__ __device__ __forceinline__ word pack(int32_t hi, int32_t lo) {
  return ((word)(uint32_t)hi << 32) | (word)(uint32_t)lo;
}
__device__ __forceinline__ int32_t hi_of(word w) { return (int32_t)(uint32_t)(w >> 32); }
__device__ __forceinline__ int32_t lo_of(word w) { return (int32_t)(uint32_t)w; }
__device__ __forceinline__ word load_word(const word* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_word(word* p, word w) {
  __hip_atomic_store(p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- index build ----------------------------------------------------------------------------------------------
enum { kErrRange = 0, kErrLower = 1, kErrDend = 2, kErrWords = 3 };

__global__ void __launch_bounds__(kTB) k_down(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                                              int32_t* down, word* err) {
  for (int64_t k = (int64_t)blockIdx.x * kTB + threadIdx.x; k < e; k += (int64_t)gridDim.x * kTB) {
    const int32_t r = rows[k], c = cols[k];
    if (r < 0 || r >= n || c < 0 || c >= n) {
      atomicMin(err + kErrRange, (word)k);
    } else if (r <= c) {
      atomicMin(err + kErrLower, (word)k);
    } else {
      const int32_t old = atomicCAS(down + c, -1, r);
      if (old != -1 && old != r) atomicMin(err + kErrDend, (word)c);
    }
  }
}
// word = (hops << 32) | jump: jump is `hops` reaches downstream; with jump == -1, hops = depth + 1
__global__ void __launch_bounds__(kTB) k_depth_init(int64_t n, const int32_t* down, word* st) {
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTB)
    st[i] = pack(1, down[i]);
}
__global__ void __launch_bounds__(kTB) k_depth_round(int64_t n, word* st) {
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTB) {
    const word w = load_word(st + i);
    const int32_t j = lo_of(w);
    if (j < 0) continue;
    const word v = load_word(st + j);
    store_word(st + i, pack(hi_of(w) + hi_of(v), lo_of(v)));
  }
}
// agg[0] = deepest reach, agg[1] = outlets, agg[2] = reaches whose walk has not left the network
__global__ void __launch_bounds__(kTB) k_depth_stats(int64_t n, const int32_t* down, const word* st, int32_t* agg) {
  int32_t deep = 0, outl = 0, open = 0;
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTB) {
    const word w = st[i];
    if (lo_of(w) >= 0) ++open;
    else deep = max(deep, hi_of(w) - 1);
    outl += down[i] < 0;
  }
  for (int o = 32; o > 0; o >>= 1) {
    deep = max(deep, __shfl_xor(deep, o));
    outl += __shfl_xor(outl, o);
    open += __shfl_xor(open, o);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(agg + 0, deep);
    if (outl) atomicAdd(agg + 1, outl);
    if (open) atomicAdd(agg + 2, open);
  }
}

// ---- label ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTB) k_label_init(int64_t n, const int32_t* down, word* st) {
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTB)
    st[i] = pack(-1, down[i]);
}
// tg[0..G) the target reaches, tg[G..2G) slot_of (checked on the host: in range); only the smallest slot of a
// reach writes, so no two threads store to one word
__global__ void __launch_bounds__(kTB) k_label_targets(int64_t G, const int32_t* tg, word* st) {
  for (int64_t g = (int64_t)blockIdx.x * kTB + threadIdx.x; g < G; g += (int64_t)gridDim.x * kTB)
    if (tg[G + g] == (int32_t)g) st[tg[g]] = pack((int32_t)g, tg[g]);
}
__global__ void __launch_bounds__(kTB) k_label_round(int64_t n, word* st) {
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTB) {
    const word w = load_word(st + i);
    const int32_t j = lo_of(w);
    if (hi_of(w) >= 0 || j < 0) continue;
    store_word(st + i, load_word(st + j));
  }
}
__global__ void __launch_bounds__(kTB) k_label_out(int64_t n, const word* st, int32_t* label) {
  for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTB)
    label[i] = hi_of(st[i]);
}

// ---- collate --------------------------------------------------------------------------------------------------
// the closure's edges appended to (rows, cols): one atomic per wave.  At most n - 1 edges exist, the arrays hold n.
__global__ void __launch_bounds__(kTB) k_closure_coo(int64_t n, const int32_t* down, const word* st, int32_t* rows,
                                                     int32_t* cols, word* count) {
  const int lane = threadIdx.x & 63;
  const int64_t span = (int64_t)gridDim.x * kTB;
  for (int64_t base = (int64_t)blockIdx.x * kTB; base < n; base += span) {  // (wave-uniform trip count)
    const int64_t i = base + threadIdx.x;
    int32_t d = -1;
    if (i < n && hi_of(st[i]) >= 0) {
      d = down[i];
      if (d >= 0 && hi_of(st[d]) < 0) d = -1;
    }
    const word m = __builtin_amdgcn_ballot_w64(d >= 0);
    if (m == 0) continue;
    const int leader = __builtin_ffsll((long long)m) - 1;
    word at = 0;
    if (lane == leader) at = atomicAdd(count, (word)__builtin_popcountll(m));
    at = __shfl(at, leader);
    if (d >= 0) {
      const int64_t p = (int64_t)at + __builtin_popcountll(m & (((word)1 << lane) - 1));
      rows[p] = d;
      cols[p] = (int32_t)i;
    }
  }
}

// ---- members --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTB) k_parent(int64_t G, const int32_t* tg, const int32_t* down, const word* st,
                                                int32_t* parent) {
  for (int64_t g = (int64_t)blockIdx.x * kTB + threadIdx.x; g < G; g += (int64_t)gridDim.x * kTB) {
    const int32_t d = down[tg[g]];
    parent[g] = d < 0 ? -1 : hi_of(st[d]);
  }
}
// Every reach walks its gauge chain; the lanes of a wave holding one gauge combine.  EMIT: also write the keys at
// coff[gauge] + the position the atomic returns.  The chain ends because a parent's reach lies strictly downstream.
template <bool EMIT>
__global__ void __launch_bounds__(kTB) k_chain(int64_t n, const word* st, const int32_t* parent, word* cnt,
                                               const int64_t* coff, word* keys) {
  const int lane = threadIdx.x & 63;
  const int64_t span = (int64_t)gridDim.x * kTB;
  for (int64_t base = (int64_t)blockIdx.x * kTB; base < n; base += span) {
    const int64_t i = base + threadIdx.x;
    int32_t g = i < n ? hi_of(st[i]) : -1;
    word m = __builtin_amdgcn_ballot_w64(g >= 0);
    while (m != 0) {  // (m is wave-uniform)
      const int leader = __builtin_ffsll((long long)m) - 1;
      const int32_t k = __shfl(g, leader);
      const bool mine = g == k;  // (k >= 0)
      const word mm = __builtin_amdgcn_ballot_w64(mine);
      word at = 0;
      if (lane == leader) at = atomicAdd(cnt + k, (word)__builtin_popcountll(mm));
      if (EMIT) {
        at = __shfl(at, leader);
        if (mine)
          keys[coff[k] + (int64_t)at + __builtin_popcountll(mm & (((word)1 << lane) - 1))] = (word)k * (word)n + (word)i;
      }
      if (mine) g = parent[k];
      m = __builtin_amdgcn_ballot_w64(g >= 0);
    }
  }
}
// off = exclusive scan of cnt[slot_of[g]] over all gauges, coff = of cnt[g] over the smallest slots alone (G + 1
// entries each).  One workgroup: a thread sums a contiguous run, the 256 run totals are scanned in LDS.
__global__ void __launch_bounds__(kTB) k_offsets(int64_t G, const int32_t* slot_of, const word* cnt, int64_t* off,
                                                 int64_t* coff) {
  __shared__ int64_t s_all[kTB], s_own[kTB];
  const int64_t per = (G + kTB - 1) / kTB;
  const int64_t g0 = per * threadIdx.x < G ? per * threadIdx.x : G, g1 = g0 + per < G ? g0 + per : G;
  int64_t a = 0, o = 0;
  for (int64_t g = g0; g < g1; ++g) {
    a += (int64_t)cnt[slot_of[g]];
    if (slot_of[g] == g) o += (int64_t)cnt[g];
  }
  s_all[threadIdx.x] = a;
  s_own[threadIdx.x] = o;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t ra = 0, ro = 0;
    for (int t = 0; t < kTB; ++t) {
      const int64_t va = s_all[t], vo = s_own[t];
      s_all[t] = ra;
      s_own[t] = ro;
      ra += va;
      ro += vo;
    }
    off[G] = ra;
    coff[G] = ro;
  }
  __syncthreads();
  a = s_all[threadIdx.x];
  o = s_own[threadIdx.x];
  for (int64_t g = g0; g < g1; ++g) {
    off[g] = a;
    coff[g] = o;
    a += (int64_t)cnt[slot_of[g]];
    if (slot_of[g] == g) o += (int64_t)cnt[g];
  }
}
// idx[p] for p in gauge g's segment: the reach of the sorted key at the same position of slot_of[g]'s list
__global__ void __launch_bounds__(kTB) k_gather(int64_t total, int64_t G, int64_t n, const int64_t* off,
                                                const int64_t* coff, const int32_t* slot_of, const word* keys,
                                                int32_t* idx) {
  for (int64_t p = (int64_t)blockIdx.x * kTB + threadIdx.x; p < total; p += (int64_t)gridDim.x * kTB) {
    int64_t lo = 0, hi = G;  // the last g with off[g] <= p (every list holds its gauge reach: none is empty)
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (off[mid] <= p) lo = mid;
      else hi = mid;
    }
    const int32_t s = slot_of[lo];
    idx[p] = (int32_t)(keys[coff[s] + (p - off[lo])] - (word)s * (word)n);
  }
}

inline int bits_for(uint64_t maxval) {
  int b = 1;
  while (b < 64 && (maxval >> b) != 0) ++b;
  return b;
}

size_t sort_temp_bytes(int64_t m) {
  size_t bytes = 0;
  if (m <= 0) return 0;
  if (hipcub::DeviceRadixSort::SortKeys(nullptr, bytes, static_cast<const word*>(nullptr), static_cast<word*>(nullptr),
                                        (int)m, 0, 64, (hipStream_t) nullptr) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return bytes;
}

// carves the caller's scratch
struct Carver {
  char* p;
  template <typename T>
  T* take(int64_t count) {
    T* r = reinterpret_cast<T*>(p);
    p += align256(std::max<int64_t>(count, 1) * (int64_t)sizeof(T));
    return r;
  }
};

// the checks every device query makes before it launches anything
ddr_status query_checks(const UpstreamIndex* ix, const char* who, int64_t n_targets, const int32_t* targets,
                        int64_t n_members, const void* scratch, int64_t scratch_bytes, std::vector<int32_t>& slot_of) {
  ddr_status st = upstream_slots(ix, who, n_targets, targets, slot_of);
  if (st) return st;
  const std::string w(who);
  if (ix->device < 0)
    return fail(DDR_ERR_ARG, w + ": the index is host-only (built with DDR_UPSTREAM_HOST_ONLY); use the _host query");
  if (scratch_bytes < 0) return fail(DDR_ERR_ARG, w + ": negative scratch_bytes");
  const int64_t need = upstream_scratch_bytes(ix, n_targets, n_members);
  if (scratch_bytes < need)
    return fail(DDR_ERR_ARG, w + ": scratch_bytes " + std::to_string(scratch_bytes) + " is below the " +
                                 std::to_string(need) + " of ddr_upstream_scratch_bytes");
  if (!scratch) return fail(DDR_ERR_ARG, w + ": null scratch");
  int cur = -1;
  DDR_HIP(hipGetDevice(&cur));
  if (cur != ix->device)
    return fail(DDR_ERR_ARG, w + ": the index lives on device " + std::to_string(ix->device) +
                                 ", the current device is " + std::to_string(cur));
  return DDR_OK;
}

// the words of every reach after the doubling rounds, and the target table tg = [reaches | slot_of] on the device
ddr_status label_words(const UpstreamIndex* ix, int64_t G, const int32_t* targets, const std::vector<int32_t>& slot_of,
                       word* st, int32_t* tg, hipStream_t s) {
  const int64_t n = ix->n;
  if (G > 0) {
    DDR_HIP(hipMemcpyAsync(tg, targets, sizeof(int32_t) * G, hipMemcpyHostToDevice, s));
    DDR_HIP(hipMemcpyAsync(tg + G, slot_of.data(), sizeof(int32_t) * G, hipMemcpyHostToDevice, s));
    DDR_HIP(hipStreamSynchronize(s));  // (the uploads read this call's host arrays; nothing is read back)
  }
  hipLaunchKernelGGL(k_label_init, dim3(grid_for(n)), dim3(kTB), 0, s, n, ix->d_down, st);
  if (G > 0) {
    hipLaunchKernelGGL(k_label_targets, dim3(grid_for(G)), dim3(kTB), 0, s, G, tg, st);
    for (int r = 0; r < ix->rounds; ++r) hipLaunchKernelGGL(k_label_round, dim3(grid_for(n)), dim3(kTB), 0, s, n, st);
  }
  DDR_HIP(hipGetLastError());
  return DDR_OK;
}

}  // namespace

int64_t upstream_scratch_bytes(const UpstreamIndex* ix, int64_t n_targets, int64_t n_members) {
  if (!ix || n_targets < 0 || n_members < 0) return -1;
  if (ix->device < 0) return 0;
  const int64_t n = ix->n, G1 = n_targets + 1;
  int64_t b = align256(8 * n) + 2 * align256(4 * n)  // words, closure COO
              + align256(8 * G1)                       // target table (2 G int32)
              + align256(4 * G1) + 3 * align256(8 * G1)  // parent, cnt, off, coff
              + 512;                                   // edge counter, slack
  if (n_members > 0) b += 2 * align256(8 * n_members) + align256((int64_t)sort_temp_bytes(n_members));
  return b;
}

ddr_status upstream_index_create(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols, int32_t flags,
                                 hipStream_t stream, UpstreamIndex** index) {
  if (!index) return fail(DDR_ERR_ARG, "upstream_index_create: null index pointer");
  *index = nullptr;
  if (n <= 0) return fail(DDR_ERR_ARG, "upstream_index_create: the network must have at least one reach");
  if (n >= (int64_t(1) << 31) - 1 || e >= (int64_t(1) << 31) - 1)
    return fail(DDR_ERR_ARG, "upstream_index_create: network too large for int32 reach ids");
  if (e < 0) return fail(DDR_ERR_ARG, "upstream_index_create: negative edge count");
  if (e > 0 && (!rows || !cols)) return fail(DDR_ERR_ARG, "upstream_index_create: null COO arrays");
  if (flags & ~(DDR_UPSTREAM_HOST_ONLY | DDR_UPSTREAM_DEVICE_COO))
    return fail(DDR_ERR_ARG, "upstream_index_create: unknown flag");
  const bool host_only = flags & DDR_UPSTREAM_HOST_ONLY, dev_coo = flags & DDR_UPSTREAM_DEVICE_COO;
  if (host_only && dev_coo)
    return fail(DDR_ERR_ARG, "upstream_index_create: a host-only index cannot read a device COO");
  auto ix = std::make_unique<UpstreamIndex>();
  ix->n = n;
  ddr_status st;
  if (!dev_coo) {
    if ((st = upstream_down_host(n, e, rows, cols, ix->down))) return st;
    upstream_depth_host(ix.get());
    if (host_only) {
      *index = ix.release();
      return DDR_OK;
    }
  }
  DDR_HIP(hipGetDevice(&ix->device));
  struct Free {
    void operator()(void* p) const { (void)hipFree(p); }
  };
  void* raw = nullptr;
  DDR_HIP(hipMalloc(&raw, sizeof(int32_t) * n));
  std::unique_ptr<void, Free> d_down(raw);
  int32_t* down = static_cast<int32_t*>(raw);
  if (!dev_coo) {
    DDR_HIP(hipMemcpyAsync(down, ix->down.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, stream));
    DDR_HIP(hipStreamSynchronize(stream));
  } else {
    // down[] by compare-and-swap, then the depth of every reach by doubling; ceil(log2(n)) + 1 rounds cover any
    // path of the network (its length is not known yet)
    DDR_HIP(hipMalloc(&raw, sizeof(word) * n + sizeof(word) * kErrWords + 16));
    std::unique_ptr<void, Free> tmp(raw);
    word* wst = static_cast<word*>(raw);
    word* err = wst + n;
    int32_t* agg = reinterpret_cast<int32_t*>(err + kErrWords);
    DDR_HIP(hipMemsetAsync(down, 0xFF, sizeof(int32_t) * n, stream));
    DDR_HIP(hipMemsetAsync(err, 0xFF, sizeof(word) * kErrWords, stream));
    DDR_HIP(hipMemsetAsync(agg, 0, 16, stream));
    if (e > 0) hipLaunchKernelGGL(k_down, dim3(grid_for(e)), dim3(kTB), 0, stream, n, e, rows, cols, down, err);
    hipLaunchKernelGGL(k_depth_init, dim3(grid_for(n)), dim3(kTB), 0, stream, n, down, wst);
    const int rounds = upstream_rounds(n);
    for (int r = 0; r < rounds; ++r) hipLaunchKernelGGL(k_depth_round, dim3(grid_for(n)), dim3(kTB), 0, stream, n, wst);
    hipLaunchKernelGGL(k_depth_stats, dim3(grid_for(n)), dim3(kTB), 0, stream, n, down, wst, agg);
    DDR_HIP(hipGetLastError());
    word herr[kErrWords];
    int32_t hagg[4];
    ix->down.resize((size_t)n);
    DDR_HIP(hipMemcpyAsync(herr, err, sizeof(herr), hipMemcpyDeviceToHost, stream));
    DDR_HIP(hipMemcpyAsync(hagg, agg, sizeof(hagg), hipMemcpyDeviceToHost, stream));
    DDR_HIP(hipMemcpyAsync(ix->down.data(), down, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream));
    DDR_HIP(hipStreamSynchronize(stream));
    const word none = ~(word)0;
    if (herr[kErrRange] != none)
      return fail(DDR_ERR_ARG, "upstream_index_create: edge " + std::to_string(herr[kErrRange]) + " is out of range");
    if (herr[kErrLower] != none) {
      int32_t rc[2];
      DDR_HIP(hipMemcpy(rc, rows + herr[kErrLower], 4, hipMemcpyDeviceToHost));
      DDR_HIP(hipMemcpy(rc + 1, cols + herr[kErrLower], 4, hipMemcpyDeviceToHost));
      return fail(DDR_ERR_NOT_LOWER, "upstream_index_create: entry (" + std::to_string(rc[0]) + "," +
                                         std::to_string(rc[1]) + ") is not strictly lower triangular");
    }
    if (herr[kErrDend] != none)
      return fail(DDR_ERR_NOT_DENDRITIC, "upstream_index_create: reach " + std::to_string(herr[kErrDend]) +
                                             " drains into two different reaches");
    if (hagg[2] != 0) return fail(DDR_ERR_HIP, "upstream_index_create: the depth pass did not finish");
    ix->max_depth = hagg[0];
    ix->n_outlets = hagg[1];
    ix->rounds = upstream_rounds(ix->max_depth);
  }
  ix->d_down = static_cast<int32_t*>(d_down.release());
  *index = ix.release();
  return DDR_OK;
}

void upstream_index_destroy(UpstreamIndex* ix) {
  if (!ix) return;
  if (ix->d_down) (void)hipFree(ix->d_down);
  delete ix;
}

ddr_status upstream_label(const UpstreamIndex* ix, int64_t n_targets, const int32_t* targets, int32_t* label,
                          int32_t* slot_of, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  std::vector<int32_t> slots;
  ddr_status st = query_checks(ix, "upstream_label", n_targets, targets, 0, scratch, scratch_bytes, slots);
  if (st) return st;
  if (!label) return fail(DDR_ERR_ARG, "upstream_label: null label_out");
  Carver c{static_cast<char*>(scratch)};
  word* wst = c.take<word>(ix->n);
  int32_t* tg = c.take<int32_t>(2 * n_targets);
  if ((st = label_words(ix, n_targets, targets, slots, wst, tg, s))) return st;
  hipLaunchKernelGGL(k_label_out, dim3(grid_for(ix->n)), dim3(kTB), 0, s, ix->n, wst, label);
  DDR_HIP(hipGetLastError());
  if (slot_of) std::copy(slots.begin(), slots.end(), slot_of);  // (host)
  return DDR_OK;
}

ddr_status upstream_collate(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx, int32_t* active,
                            int64_t active_cap, int64_t* n_active, int32_t* rows_c, int32_t* cols_c, int64_t edge_cap,
                            int64_t* nnz, int64_t* crow, int32_t* col, int64_t* out_off, int32_t* out_idx,
                            int64_t out_idx_cap, int32_t* gage_c, void* scratch, int64_t scratch_bytes,
                            hipStream_t s) {
  std::vector<int32_t> slots;
  ddr_status st = query_checks(ix, "upstream_collate", n_gauges, gage_idx, 0, scratch, scratch_bytes, slots);
  if (st) return st;
  if (active_cap < 0 || edge_cap < 0 || out_idx_cap < 0) return fail(DDR_ERR_ARG, "upstream_collate: negative capacity");
  if (!active || !n_active || !nnz || !crow || !out_off || (n_gauges > 0 && (!out_idx || !gage_c)))
    return fail(DDR_ERR_ARG, "upstream_collate: null output");
  const int64_t n = ix->n;
  Carver c{static_cast<char*>(scratch)};
  word* wst = c.take<word>(n);
  int32_t* tg = c.take<int32_t>(2 * n_gauges);
  int32_t* rows = c.take<int32_t>(n);
  int32_t* cols = c.take<int32_t>(n);
  word* count = c.take<word>(1);
  if ((st = label_words(ix, n_gauges, gage_idx, slots, wst, tg, s))) return st;
  DDR_HIP(hipMemsetAsync(count, 0, sizeof(word), s));
  hipLaunchKernelGGL(k_closure_coo, dim3(grid_for(n)), dim3(kTB), 0, s, n, ix->d_down, wst, rows, cols, count);
  DDR_HIP(hipGetLastError());
  word e = 0;
  DDR_HIP(hipMemcpyAsync(&e, count, sizeof(word), hipMemcpyDeviceToHost, s));
  DDR_HIP(hipStreamSynchronize(s));
  if ((int64_t)e > edge_cap || (e > 0 && (!rows_c || !cols_c || !col)))
    return fail(DDR_ERR_ARG, "upstream_collate: the closure's " + std::to_string(e) + " edges exceed edge_cap (" +
                                 std::to_string(edge_cap) + ")");
  return collate_gauges_device(n, n_gauges, (int64_t)e, rows, cols, tg, active, active_cap, n_active, rows_c, cols_c,
                               nnz, crow, col, out_off, out_idx, out_idx_cap, gage_c, s);
}

namespace {

ddr_status members_impl(const UpstreamIndex* ix, const char* who, int64_t G, const int32_t* gage_idx, int64_t* off_out,
                        int64_t* total_out, bool emit, int64_t n_members, int32_t* idx, void* scratch,
                        int64_t scratch_bytes, hipStream_t s) {
  std::vector<int32_t> slots;
  ddr_status st = query_checks(ix, who, G, gage_idx, n_members, scratch, scratch_bytes, slots);
  if (st) return st;
  const std::string w(who);
  if (!emit && (!off_out || !total_out)) return fail(DDR_ERR_ARG, w + ": null output");
  if (emit && n_members > 0 && !idx) return fail(DDR_ERR_ARG, w + ": null idx");
  if (n_members >= (int64_t(1) << 31)) return fail(DDR_ERR_ARG, w + ": 2^31 or more members");
  const int64_t n = ix->n;
  Carver c{static_cast<char*>(scratch)};
  word* wst = c.take<word>(n);
  int32_t* tg = c.take<int32_t>(2 * G);
  int32_t* parent = c.take<int32_t>(G);
  word* cnt = c.take<word>(G);
  int64_t* off = c.take<int64_t>(G + 1);
  int64_t* coff = c.take<int64_t>(G + 1);
  if ((st = label_words(ix, G, gage_idx, slots, wst, tg, s))) return st;
  DDR_HIP(hipMemsetAsync(cnt, 0, sizeof(word) * std::max<int64_t>(G, 1), s));
  if (G > 0) {
    hipLaunchKernelGGL(k_parent, dim3(grid_for(G)), dim3(kTB), 0, s, G, tg, ix->d_down, wst, parent);
    hipLaunchKernelGGL((k_chain<false>), dim3(grid_for(n)), dim3(kTB), 0, s, n, wst, parent, cnt, nullptr, nullptr);
  }
  hipLaunchKernelGGL(k_offsets, dim3(1), dim3(kTB), 0, s, G, tg + G, cnt, off, coff);
  DDR_HIP(hipGetLastError());
  int64_t totals[2] = {0, 0};
  DDR_HIP(hipMemcpyAsync(totals, off + G, 8, hipMemcpyDeviceToHost, s));
  DDR_HIP(hipMemcpyAsync(totals + 1, coff + G, 8, hipMemcpyDeviceToHost, s));
  if (!emit) DDR_HIP(hipMemcpyAsync(off_out, off, sizeof(int64_t) * (G + 1), hipMemcpyDeviceToDevice, s));
  DDR_HIP(hipStreamSynchronize(s));
  if (totals[0] >= (int64_t(1) << 31))
    return fail(DDR_ERR_ARG, w + ": the member lists hold " + std::to_string(totals[0]) +
                                 " entries, 2^31 or more do not fit int32 offsets downstream");
  if (!emit) {
    *total_out = totals[0];
    return DDR_OK;
  }
  if (totals[0] != n_members)
    return fail(DDR_ERR_ARG, w + ": n_members " + std::to_string(n_members) + " is not the " +
                                 std::to_string(totals[0]) + " of ddr_upstream_member_counts for these gauges");
  const int64_t m = totals[1];  // keys of the smallest slots alone (<= n_members)
  if (m == 0) return DDR_OK;
  word* keys = c.take<word>(n_members);
  word* sorted = c.take<word>(n_members);
  size_t tbytes = sort_temp_bytes(m);
  void* temp = c.take<char>((int64_t)tbytes);
  if (c.p > static_cast<char*>(scratch) + scratch_bytes) return fail(DDR_ERR_ARG, w + ": scratch too small for the sort");
  DDR_HIP(hipMemsetAsync(cnt, 0, sizeof(word) * G, s));
  hipLaunchKernelGGL((k_chain<true>), dim3(grid_for(n)), dim3(kTB), 0, s, n, wst, parent, cnt, coff, keys);
  DDR_HIP(hipGetLastError());
  DDR_HIP(hipcub::DeviceRadixSort::SortKeys(temp, tbytes, keys, sorted, (int)m, 0,
                                            bits_for((uint64_t)G * (uint64_t)n), s));
  hipLaunchKernelGGL(k_gather, dim3(grid_for(n_members)), dim3(kTB), 0, s, n_members, G, n, off, coff, tg + G, sorted,
                     idx);
  DDR_HIP(hipGetLastError());
  DDR_HIP(hipStreamSynchronize(s));
  return DDR_OK;
}

}  // namespace

ddr_status upstream_member_counts(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx, int64_t* off,
                                  int64_t* total, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  return members_impl(ix, "upstream_member_counts", n_gauges, gage_idx, off, total, false, 0, nullptr, scratch,
                      scratch_bytes, s);
}

ddr_status upstream_members(const UpstreamIndex* ix, int64_t n_gauges, const int32_t* gage_idx, int64_t n_members,
                            int32_t* idx, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  if (ix && n_members < 0) return fail(DDR_ERR_ARG, "upstream_members: negative n_members");
  return members_impl(ix, "upstream_members", n_gauges, gage_idx, nullptr, nullptr, true, n_members, idx, scratch,
                      scratch_bytes, s);
}

}  // namespace ddr
