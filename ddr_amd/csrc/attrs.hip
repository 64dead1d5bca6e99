// The per-batch attribute feed: what the reference's collate_fn still does on the host per batch -- _get_attributes
// and _build_common_tensors (src/ddr/geodatazoo/merit.py:92-124, 273-319; lynker_hydrofabric.py:105-135, 302-354)
// and build_flow_scale_tensor (io/readers.py:299-362) -- from tables that were uploaded once, addressed by the
// batch's CONUS indices (DeviceBatch.active).
//
// attr_gather_kernel -- one launch per batch.  The aligned table is reach-major, (n_conus, row_stride) with a row's A
// attributes contiguous, so a reach costs one contiguous read wherever it lies; a reach the attribute store lacks is
// a NaN row, an index outside [0, n_conus) reads nothing and is NaN in every attribute.  A workgroup owns kTR = 64
// batch reaches.  Lanes are laid over (reach, attribute) with the attribute innermost (Ap = A rounded up to a power
// of two lanes per reach), so a wave reads 64 / Ap whole rows per instruction and writes the same lanes to the
// reach-major normalized output (N, A), which is contiguous across the tile.  The attribute-major output (A, N) is the
// opposite layout: the filled values are staged in LDS (leading dimension odd, so both the row-wise writes and the
// lane = reach reads are conflict-free) and written along reaches, 256 contiguous bytes per wave.  Tiles are numbered
// so that neighbours run on one XCD (as feed.hip), where the output lines two tiles share are completed in its L2.
//   value       table[active[i]][a], NaN for a missing reach
//   fill        a NaN becomes fill[a]: means[a] (fill_nans, merit.py:124), or, where means[a] is itself NaN, the
//               NaN-mean of the attribute over this batch (merit.py:295-298), which attr_mean_* wrote there before
//   normalized  (value - means[a]) / stds[a]: one fp32 subtraction, one IEEE division (the build has no contraction
//               and correctly rounded division).  Where a result is a NaN its bits are those the reference's host
//               code gives it (x86; torch subtracts as fma(mean, -1, value)): the mean's NaN before the value's,
//               the numerator's before the divisor's, quieted, and the default NaN 0xffc00000 of an invalid
//               operation (inf - inf, 0 / 0) without a NaN operand
// The same launch gathers the flowpath arrays (length, slope, x, top_width, side_slope: out[i] = arr[active[i]], a NaN
// or an out-of-range index becomes the array's fill value; an array the dataset lacks is skipped, x without an array is
// the constant) and sets flow_scale to 1.0: one more read of active[i] each.  Values move as 32-bit words.  Addresses
// are 64-bit.  Plain vector loads and stores only.
//
// attr_mean_partial_kernel / attr_mean_final_kernel -- the per-batch NaN-mean of the flagged attributes only (the
// common case, every mean finite, launches neither): fp64 sums and counts per workgroup over a fixed slice of the
// batch, reduced in a fixed order (no atomics: the result does not depend on scheduling) and rounded to fp32 once.
//
// flow_scale_kernel -- the reference's sequential loop `for g: flow_scale[gage_c[g]] = factor[g]` with "the last
// gauge in batch order wins" made independent of scheduling: one workgroup resolves the winning gauge of every
// touched segment first (atomicMax of the gauge index into a per-segment word) and writes second.
#include "attrs.h"

#include <string>

#include "internal.h"

namespace ddr {

namespace {

constexpr int kTR = 64;  // batch reaches per tile
constexpr int kLDMax = kAttrMaxA + 1;
constexpr int kXcds = 8;  // accelerator dies, each with its own L2
constexpr int kPaths = DDR_FLOWPATH_ARRAYS;
constexpr uint32_t kQuietBit = 0x00400000u;
constexpr uint32_t kHostDefaultNaN = 0xffc00000u;  // x86's result of an invalid operation (0/0, inf - inf)
constexpr uint32_t kOne = 0x3f800000u;

__device__ __forceinline__ bool is_nan_bits(uint32_t x) { return (x & 0x7fffffffu) > 0x7f800000u; }

// the NaN an x86 host returns for an operation on (a, b) in its operand order: the first NaN operand, quieted;
// without one the operation was invalid
__device__ __forceinline__ uint32_t host_nan(uint32_t a, uint32_t b) {
  return is_nan_bits(a) ? (a | kQuietBit) : is_nan_bits(b) ? (b | kQuietBit) : kHostDefaultNaN;
}

struct AttrArgs {
  const uint32_t* table;
  int64_t row_stride;
  const int32_t* active;
  int64_t N;
  int64_t n_tiles, tiles_per_xcd;  // reach tiles, and ceil(n_tiles / kXcds)
  int32_t n_conus, A;
  int32_t log2_ap;  // lanes per reach = 1 << log2_ap >= A
  int32_t ld;       // leading dimension of the staged tile (odd)
  const uint32_t* fill;
  const float* means;
  const float* stds;
  uint32_t* spatial;     // (A, N)
  uint32_t* normalized;  // (N, A)
  const uint32_t* path_src[kPaths];
  uint32_t path_fill[kPaths];
  uint32_t* path_out[kPaths];
  uint32_t* flow_scale;
};

__global__ void __launch_bounds__(256) attr_gather_kernel(AttrArgs a) {
  __shared__ uint32_t tile[kTR * kLDMax];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // (blockIdx.x -> reach tile: workgroups b and b + 8 have been observed to share an XCD, feed.hip)
  const int64_t tile_n = (int64_t)(blockIdx.x & (kXcds - 1)) * a.tiles_per_xcd + (blockIdx.x / kXcds);
  if (tile_n >= a.n_tiles) return;  // (the whole workgroup, before the barrier)
  const int64_t n0 = tile_n * kTR;

  const int f = tid & ((1 << a.log2_ap) - 1);
  if (f < a.A) {
    const uint32_t fill = a.fill[f];
    const uint32_t mean_bits = reinterpret_cast<const uint32_t*>(a.means)[f];
    const uint32_t std_bits = reinterpret_cast<const uint32_t*>(a.stds)[f];
    const float mean = __uint_as_float(mean_bits), std = __uint_as_float(std_bits);
    const int step = 256 >> a.log2_ap;
    for (int r = tid >> a.log2_ap; r < kTR; r += step) {
      const int64_t n = n0 + r;
      if (n >= a.N) break;
      const int32_t c = a.active[n];
      uint32_t x = kHostDefaultNaN;
      if ((uint32_t)c < (uint32_t)a.n_conus) x = a.table[(int64_t)c * a.row_stride + f];
      if (is_nan_bits(x)) x = fill;
      tile[r * a.ld + f] = x;
      const float d = __uint_as_float(x) - mean;
      uint32_t d_bits = __float_as_uint(d);
      if (is_nan_bits(d_bits)) d_bits = host_nan(mean_bits, x);
      uint32_t q_bits = __float_as_uint(__uint_as_float(d_bits) / std);
      if (is_nan_bits(q_bits)) q_bits = host_nan(d_bits, std_bits);
      a.normalized[n * a.A + f] = q_bits;
    }
  }
  __syncthreads();

  const int64_t n = n0 + lane;
  if (n >= a.N) return;
  for (int c = w; c < a.A; c += 4) a.spatial[(int64_t)c * a.N + n] = tile[lane * a.ld + c];

  // the flowpath arrays and flow_scale: tasks 0 .. kPaths over the four waves
  int32_t c = -1;
  bool have = false;
  for (int k = w; k <= kPaths; k += 4) {
    if (k == kPaths) {
      if (a.flow_scale) a.flow_scale[n] = kOne;
      continue;
    }
    if (!a.path_out[k]) continue;
    uint32_t x = a.path_fill[k];
    if (a.path_src[k]) {
      if (!have) c = a.active[n], have = true;
      if ((uint32_t)c < (uint32_t)a.n_conus) {
        const uint32_t v = a.path_src[k][c];
        if (!is_nan_bits(v)) x = v;
      }
    }
    a.path_out[k][n] = x;
  }
}

// grid (blocks, n_flagged): workgroup (b, j) sums attribute flagged[j] over reaches b * 256 + tid, + blocks * 256, ...
__global__ void __launch_bounds__(256) attr_mean_partial_kernel(const uint32_t* table, int64_t row_stride,
                                                                int32_t n_conus, int32_t A, const int32_t* active,
                                                                int64_t N, const int32_t* flagged, double* sums,
                                                                int64_t* counts) {
  __shared__ double s_sum[256];
  __shared__ int64_t s_cnt[256];
  const int f = flagged[blockIdx.y];
  if ((uint32_t)f >= (uint32_t)A) return;  // (not an attribute: the whole workgroup, nothing is read or written)
  double sum = 0.0;
  int64_t cnt = 0;
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
    const int32_t c = active[n];
    if ((uint32_t)c >= (uint32_t)n_conus) continue;
    const uint32_t x = table[(int64_t)c * row_stride + f];
    if (is_nan_bits(x)) continue;
    sum += (double)__uint_as_float(x);
    ++cnt;
  }
  s_sum[threadIdx.x] = sum;
  s_cnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + h];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    sums[(int64_t)blockIdx.y * kAttrMeanBlocks + blockIdx.x] = s_sum[0];
    counts[(int64_t)blockIdx.y * kAttrMeanBlocks + blockIdx.x] = s_cnt[0];
  }
}

// grid (n_flagged): the partial sums of one attribute in a fixed order, then one division and one rounding to fp32
__global__ void __launch_bounds__(256) attr_mean_final_kernel(const double* sums, const int64_t* counts, int32_t blocks,
                                                              const int32_t* flagged, int32_t A, uint32_t* fill) {
  __shared__ double s_sum[256];
  __shared__ int64_t s_cnt[256];
  if ((uint32_t)flagged[blockIdx.x] >= (uint32_t)A) return;
  const bool in = (int)threadIdx.x < blocks;
  s_sum[threadIdx.x] = in ? sums[(int64_t)blockIdx.x * kAttrMeanBlocks + threadIdx.x] : 0.0;
  s_cnt[threadIdx.x] = in ? counts[(int64_t)blockIdx.x * kAttrMeanBlocks + threadIdx.x] : 0;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      s_sum[threadIdx.x] += s_sum[threadIdx.x + h];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // (no value at all: nansum / 0 on the reference's host; +inf and -inf in the row give a NaN sum likewise)
    const double m = s_sum[0] / (double)s_cnt[0];
    fill[flagged[blockIdx.x]] = (s_cnt[0] == 0 || m != m) ? kHostDefaultNaN : __float_as_uint((float)m);
  }
}

__global__ void __launch_bounds__(1024) flow_scale_kernel(const int32_t* gage_c, const int32_t* rows, int32_t G,
                                                          const uint32_t* factors, const uint8_t* skip,
                                                          int32_t n_factors, int64_t N, int32_t* winner,
                                                          uint32_t* out) {
  // a gauge writes when the table knows it, its factor is not marked "skip" and its segment lies in the batch
  auto segment = [&](int g) -> int64_t {
    const int32_t r = rows[g];
    if ((uint32_t)r >= (uint32_t)n_factors || (skip && skip[r])) return -1;
    const int32_t s = gage_c[g];
    return (int64_t)s < N ? (int64_t)s : -1;  // (a negative s is -1 or below: skipped)
  };
  for (int g = threadIdx.x; g < G; g += 1024) {
    const int64_t s = segment(g);
    if (s >= 0) winner[s] = -1;
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 1024) {
    const int64_t s = segment(g);
    if (s >= 0) atomicMax(&winner[s], g);
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 1024) {
    const int64_t s = segment(g);
    // (read where the atomics ran, not from this CU's L1)
    if (s >= 0 && __hip_atomic_load(&winner[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g)
      out[s] = factors[rows[g]];
  }
}

ddr_status check_table(const char* who, int64_t row_stride, int64_t n_conus, int32_t A, int64_t N) {
  const std::string w(who);
  if (row_stride < 0 || n_conus < 0 || N < 0) return fail(DDR_ERR_ARG, w + ": negative size");
  if (A < 1 || A > kAttrMaxA)
    return fail(DDR_ERR_ARG, w + ": 1 <= n_attrs <= " + std::to_string(kAttrMaxA) + " (got " + std::to_string(A) + ")");
  if (n_conus > INT32_MAX) return fail(DDR_ERR_ARG, w + ": n_conus exceeds the 32-bit reach index");
  if (row_stride < A) return fail(DDR_ERR_ARG, w + ": row_stride is shorter than a row");
  return DDR_OK;
}

}  // namespace

ddr_status feed_attributes(const float* table, int64_t row_stride, int64_t n_conus, int32_t A, const int32_t* active,
                           int64_t N, const float* fill, const float* means, const float* stds, float* spatial,
                           float* normalized, const ddr_flowpath* path, float* flow_scale, hipStream_t stream) {
  if (ddr_status s = check_table("feed_attributes", row_stride, n_conus, A, N); s != DDR_OK) return s;
  if (N == 0) return DDR_OK;
  if (!active || !fill || !means || !stds || !spatial || !normalized || (n_conus > 0 && !table))
    return fail(DDR_ERR_ARG, "feed_attributes: null argument");
  AttrArgs a{};
  if (path) {
    for (int k = 0; k < kPaths; ++k) {
      if (path->src[k] && !path->out[k])
        return fail(DDR_ERR_ARG, "feed_attributes: flowpath array " + std::to_string(k) + " has no output");
      a.path_src[k] = reinterpret_cast<const uint32_t*>(path->src[k]);
      a.path_out[k] = reinterpret_cast<uint32_t*>(path->out[k]);
      static_assert(sizeof(uint32_t) == sizeof(float), "fp32");
      __builtin_memcpy(&a.path_fill[k], &path->fill[k], sizeof(uint32_t));
    }
  }
  const int64_t n_tiles = (N + kTR - 1) / kTR, per_xcd = (n_tiles + kXcds - 1) / kXcds;
  const int64_t gx = per_xcd * kXcds;
  if (gx > INT32_MAX) return fail(DDR_ERR_ARG, "feed_attributes: too many tiles for one launch");
  int log2_ap = 0;
  while ((1 << log2_ap) < A) ++log2_ap;
  a.table = reinterpret_cast<const uint32_t*>(table);
  a.row_stride = row_stride;
  a.active = active;
  a.N = N;
  a.n_tiles = n_tiles;
  a.tiles_per_xcd = per_xcd;
  a.n_conus = (int32_t)n_conus;
  a.A = A;
  a.log2_ap = log2_ap;
  a.ld = A | 1;
  a.fill = reinterpret_cast<const uint32_t*>(fill);
  a.means = means;
  a.stds = stds;
  a.spatial = reinterpret_cast<uint32_t*>(spatial);
  a.normalized = reinterpret_cast<uint32_t*>(normalized);
  a.flow_scale = reinterpret_cast<uint32_t*>(flow_scale);
  hipLaunchKernelGGL(attr_gather_kernel, dim3((unsigned)gx), dim3(256), 0, stream, a);
  DDR_HIP(hipGetLastError());
  return DDR_OK;
}

int64_t feed_attr_mean_work_bytes(int32_t n_flagged) {
  if (n_flagged < 0 || n_flagged > kAttrMaxA) return -1;
  return (int64_t)n_flagged * kAttrMeanBlocks * (int64_t)(sizeof(double) + sizeof(int64_t));
}

ddr_status feed_attr_mean(const float* table, int64_t row_stride, int64_t n_conus, int32_t A, const int32_t* active,
                          int64_t N, const int32_t* flagged, int32_t n_flagged, float* fill, void* work,
                          int64_t work_bytes, hipStream_t stream) {
  if (ddr_status s = check_table("feed_attr_mean", row_stride, n_conus, A, N); s != DDR_OK) return s;
  if (n_flagged < 0 || n_flagged > A)
    return fail(DDR_ERR_ARG, "feed_attr_mean: 0 <= n_flagged <= n_attrs (got " + std::to_string(n_flagged) + ")");
  if (n_flagged == 0) return DDR_OK;
  if (!flagged || !fill || !work || (N > 0 && !active) || (N > 0 && n_conus > 0 && !table))
    return fail(DDR_ERR_ARG, "feed_attr_mean: null argument");
  if (work_bytes < feed_attr_mean_work_bytes(n_flagged))
    return fail(DDR_ERR_ARG, "feed_attr_mean: work_bytes is below ddr_feed_attr_mean_work_bytes");
  if (reinterpret_cast<uintptr_t>(work) & 7) return fail(DDR_ERR_ARG, "feed_attr_mean: work must be 8-byte aligned");
  int64_t blocks = (N + 1023) / 1024;  // (about four reaches per thread before a second slice)
  blocks = blocks < 1 ? 1 : blocks > kAttrMeanBlocks ? kAttrMeanBlocks : blocks;
  double* sums = static_cast<double*>(work);
  int64_t* counts = reinterpret_cast<int64_t*>(sums + (int64_t)n_flagged * kAttrMeanBlocks);
  hipLaunchKernelGGL(attr_mean_partial_kernel, dim3((unsigned)blocks, (unsigned)n_flagged), dim3(256), 0, stream,
                     reinterpret_cast<const uint32_t*>(table), row_stride, (int32_t)n_conus, A, active, N, flagged,
                     sums, counts);
  DDR_HIP(hipGetLastError());
  hipLaunchKernelGGL(attr_mean_final_kernel, dim3((unsigned)n_flagged), dim3(256), 0, stream, sums, counts,
                     (int32_t)blocks, flagged, A, reinterpret_cast<uint32_t*>(fill));
  DDR_HIP(hipGetLastError());
  return DDR_OK;
}

ddr_status feed_flow_scale(const int32_t* gage_c, const int32_t* scale_rows, int64_t G, const float* factors,
                           const uint8_t* skip, int64_t n_factors, int64_t N, int32_t* winner, float* flow_scale,
                           hipStream_t stream) {
  if (G < 0 || n_factors < 0 || N < 0) return fail(DDR_ERR_ARG, "feed_flow_scale: negative size");
  if (G > INT32_MAX || n_factors > INT32_MAX)
    return fail(DDR_ERR_ARG, "feed_flow_scale: too many gauges for the 32-bit gauge index");
  if (G == 0 || n_factors == 0 || N == 0) return DDR_OK;  // nothing can be written
  if (!gage_c || !scale_rows || !factors || !winner || !flow_scale)
    return fail(DDR_ERR_ARG, "feed_flow_scale: null argument");
  hipLaunchKernelGGL(flow_scale_kernel, dim3(1), dim3(1024), 0, stream, gage_c, scale_rows, (int32_t)G,
                     reinterpret_cast<const uint32_t*>(factors), skip, (int32_t)n_factors, N, winner,
                     reinterpret_cast<uint32_t*>(flow_scale));
  DDR_HIP(hipGetLastError());
  return DDR_OK;
}

}  // namespace ddr
