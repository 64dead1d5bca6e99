// NaN-aware summaries of long rows: count, min, max, mean, population std and up to eight exact quantiles of every
// row of a row-major (R, N) fp32 or fp64 array (numpy's nanmin / nanmax / nanmean / nanstd / nanquantile, the
// host code of io/statistics.py:45-52, validation/utils.py:110-112 and scripts/train.py:127-131).
//
// Selection is exact and sorts nothing.  A value maps to an unsigned key of its own width whose integer order is the
// values' order (sign bit flipped for positives, every bit for negatives: -0.0 sorts just below +0.0, NaN is
// excluded before the map).  The key is read most-significant digit first, kSummaryDigitBits = 8 bits per pass:
//   pass 0     every workgroup counts the top digit of its tiles into one 256-bin LDS histogram and adds the
//              non-zero bins to the row's histogram in global memory (integer atomics: the sums do not depend on
//              the order); it also leaves its partial count, sum, min and max;
//   pass p > 0 the prologue of every workgroup picks, for each tracked rank, the bin of pass p - 1 that holds it
//              (a wave scans the 256 merged bins) and so extends the rank's key prefix by one digit; the tiles then
//              count digit p of the elements whose leading digits equal a tracked prefix, one LDS histogram per
//              distinct prefix.  Pass 1 also sums (x - mean)^2: the mean is the fixed-order sum of pass 0's partials;
//   finish     one workgroup per row picks the last digit, turns the keys back into values, interpolates, reduces
//              the partial moments in workgroup order and writes the record.
// The tracked ranks are floor((n - 1) q) and its successor for each q: 2 K <= 16 of them, known once pass 0 has the
// count.  A workgroup never waits for another: what one launch wrote is read by the next launch only.
//
// The moments are fp64: a thread adds its elements in index order, the workgroup's 256 threads are added by a
// butterfly and in wave order, the row's workgroups in workgroup order.  The number of workgroups of a row depends
// on N alone, so a row's record does not depend on R or on the row's position, and two runs are identical.
#include "summary.h"

#include "../../include/ddr_mc.h"

namespace ddr {

namespace {

constexpr int NT = kSummaryThreads;
constexpr int NW = NT / 64;
constexpr int kBins = 1 << kSummaryDigitBits;
constexpr int kRanks = 2 * kSummaryMaxQ;
constexpr int kPer = kSummaryTile / NT;  // elements per thread and tile
static_assert(kBins == NT, "a thread merges one bin");
static_assert(kBins == 4 * 64, "a lane of the pick holds four bins");

enum { kCount = 0, kSum, kMin, kMax, kM2, kMoments };

template <typename T>
struct KeyOf;
template <>
struct KeyOf<float> {
  using U = uint32_t;
  static constexpr int kBits = 32;
  static __device__ __forceinline__ U key(float v) {
    const U u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
  }
  static __device__ __forceinline__ double value(unsigned long long k) {
    const U u = (U)k;
    return (double)__uint_as_float((u >> 31) ? (u ^ 0x80000000u) : ~u);
  }
};
template <>
struct KeyOf<double> {
  using U = unsigned long long;
  static constexpr int kBits = 64;
  static __device__ __forceinline__ U key(double v) {
    const U u = (U)__double_as_longlong(v);
    return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
  }
  static __device__ __forceinline__ double value(unsigned long long u) {
    return __longlong_as_double((long long)((u >> 63) ? (u ^ 0x8000000000000000ull) : ~u));
  }
};

// the work buffer of one row: the merged histograms [pass][slot][bin], the ranks' states entering each pass
// [pass][rank] (prefix, residual rank) and the workgroups' partial moments [moment][workgroup]
struct Layout {
  int passes, slots;
  size_t hist_words, state_off, part_off, row_bytes;
};
__host__ __device__ inline Layout layout_of(int K, int elem_bytes) {
  Layout l;
  l.passes = elem_bytes * 8 / kSummaryDigitBits;
  l.slots = K > 0 ? 2 * K : 1;
  l.hist_words = (size_t)l.passes * l.slots * kBins;
  l.state_off = l.hist_words * sizeof(uint32_t);
  l.part_off = l.state_off + (size_t)l.passes * kRanks * 2 * sizeof(unsigned long long);
  l.row_bytes = l.part_off + (size_t)kMoments * kSummaryMaxWgs * sizeof(double);
  return l;
}

struct RowWork {
  uint32_t* hist;
  unsigned long long* state;
  double* part;
};
__device__ __forceinline__ RowWork row_work(const SummaryArgs& a, const Layout& l, int64_t row) {
  char* base = static_cast<char*>(a.work) + (size_t)row * l.row_bytes;
  return {reinterpret_cast<uint32_t*>(base), reinterpret_cast<unsigned long long*>(base + l.state_off),
          reinterpret_cast<double*>(base + l.part_off)};
}

// what the prologue of a pass leaves in LDS
struct Shared {
  uint32_t hist[kRanks * kBins];
  double red[kMoments * NW];
  unsigned long long prefix[kRanks];  // the leading digits of the rank's key found so far
  uint32_t res[kRanks];               // the rank among the elements that share them
  int slot[kRanks];                   // the first rank with the same prefix: its histogram serves both
  unsigned long long lead_prefix[kRanks];
  int lead_slot[kRanks];
  int n_lead;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}

// the workgroup's values of moment `which` combined: the lanes by a butterfly, the waves in wave order; every thread
// gets the result.  `red` is reused: the leading barrier orders it after the previous call's reads.
__device__ __forceinline__ double group_reduce(double v, int which, double* red, int tid) {
  v = which == kMin ? wave_min(v) : which == kMax ? wave_max(v) : wave_sum(v);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) s = which == kMin ? fmin(s, red[w]) : which == kMax ? fmax(s, red[w]) : s + red[w];
  return s;
}

// moment `which` of the row from its W workgroups' partials, in workgroup order within a lane's share
__device__ __forceinline__ double row_moment(const double* part, int which, int W, double* red, int tid) {
  const double id = which == kMin ? __builtin_inf() : which == kMax ? -__builtin_inf() : 0.0;
  return group_reduce(tid < W ? part[which * kSummaryMaxWgs + tid] : id, which, red, tid);
}

__device__ __forceinline__ int tracked(const SummaryArgs& a, double n) { return n > 0.0 ? 2 * a.K : 0; }

// rank t of the row's n kept values: floor((n - 1) q) for even t, its successor (the same for `lower`) for odd t
__device__ __forceinline__ uint32_t rank_of(const SummaryArgs& a, double n, int t) {
  const double v = (n - 1.0) * a.q[t >> 1];
  double r = floor(v);
  if ((t & 1) && a.method == DDR_SUMMARY_LINEAR) r = fmin(r + 1.0, n - 1.0);
  return (uint32_t)r;
}

// slot[t]: the first rank whose prefix equals rank t's (thread 0, between barriers)
__device__ __forceinline__ void assign_slots(Shared& s, int nt) {
  for (int t = 0; t < nt; ++t) {
    int j = 0;
    while (s.prefix[j] != s.prefix[t]) ++j;  // (ends at j == t at the latest)
    s.slot[t] = j;
  }
}

// The state entering pass p >= 1 into s.prefix / s.res, and the distinct prefixes into s.lead_*: the state entering
// pass p - 1 (the ranks themselves for p - 1 == 0, otherwise what workgroup 0 of the previous launch stored) moved
// one digit on through the merged histogram of pass p - 1.  Every workgroup of the launch computes the same state.
__device__ void advance(const SummaryArgs& a, const Layout& l, const RowWork& rw, int p, double n, Shared& s, int tid) {
  const int nt = tracked(a, n);
  if (tid < nt) {
    if (p == 1) {
      s.prefix[tid] = 0;
      s.res[tid] = rank_of(a, n, tid);
    } else {
      const unsigned long long* st = rw.state + ((size_t)(p - 1) * kRanks + tid) * 2;
      s.prefix[tid] = st[0];
      s.res[tid] = (uint32_t)st[1];
    }
  }
  __syncthreads();
  if (tid == 0) assign_slots(s, nt);
  __syncthreads();
  const int lane = tid & 63;
  for (int t = tid >> 6; t < nt; t += NW) {  // (the whole wave: t depends on the wave alone)
    const uint32_t* h = rw.hist + ((size_t)(p - 1) * l.slots + s.slot[t]) * kBins;
    const uint4 c4 = reinterpret_cast<const uint4*>(h)[lane];
    const uint32_t c = c4.x + c4.y + c4.z + c4.w;
    uint32_t incl = c;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const uint32_t o = __shfl_up(incl, m, 64);
      if (lane >= m) incl += o;
    }
    const uint32_t r = s.res[t];
    const unsigned long long below = __ballot(r < incl);
    const int owner = below ? __ffsll((long long)below) - 1 : 63;
    if (lane == owner) {
      uint32_t e = incl - c;
      int b = 0;
      if (r >= e + c4.x) {
        e += c4.x;
        b = 1;
        if (r >= e + c4.y) {
          e += c4.y;
          b = 2;
          if (r >= e + c4.z) {
            e += c4.z;
            b = 3;
          }
        }
      }
      s.prefix[t] = (s.prefix[t] << kSummaryDigitBits) | (unsigned long long)(4 * lane + b);
      s.res[t] = r - e;
    }
  }
  __syncthreads();
  if (tid == 0) {
    assign_slots(s, nt);
    int nl = 0;
    for (int t = 0; t < nt; ++t)
      if (s.slot[t] == t) {
        s.lead_prefix[nl] = s.prefix[t];
        s.lead_slot[nl] = t;
        ++nl;
      }
    s.n_lead = nl;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(NT) summary_clear_kernel(SummaryArgs a, Layout l) {
  const size_t total = (size_t)a.R * l.hist_words;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
    const size_t row = i / l.hist_words;
    reinterpret_cast<uint32_t*>(static_cast<char*>(a.work) + row * l.row_bytes)[i - row * l.hist_words] = 0u;
  }
}

template <typename T>
__global__ void __launch_bounds__(NT) summary_pass_kernel(SummaryArgs a, Layout l, int p, int W) {
  using KO = KeyOf<T>;
  using U = typename KO::U;
  __shared__ Shared s;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x / W;
  const int w = (int)(blockIdx.x - row * W);
  const RowWork rw = row_work(a, l, row);
  const T* x = static_cast<const T*>(a.x) + row * a.stride;
  const bool skip_inf = (a.flags & DDR_SUMMARY_SKIP_INF) != 0;

  double mean = 0.0;
  if (p == 0) {
    if (tid == 0) {
      s.n_lead = 1;
      s.lead_prefix[0] = 0;
      s.lead_slot[0] = 0;
    }
  } else {
    const double n = row_moment(rw.part, kCount, W, s.red, tid);
    if (p == 1) mean = row_moment(rw.part, kSum, W, s.red, tid) / n;
    advance(a, l, rw, p, n, s, tid);
    const int nt = tracked(a, n);
    if (w == 0 && tid < nt) {
      unsigned long long* st = rw.state + ((size_t)p * kRanks + tid) * 2;
      st[0] = s.prefix[tid];
      st[1] = s.res[tid];
    }
  }
#pragma unroll
  for (int k = 0; k < kRanks; ++k) s.hist[k * kBins + tid] = 0u;
  __syncthreads();

  const int n_lead = s.n_lead;
  const int shift = KO::kBits - kSummaryDigitBits * (p + 1);
  double cnt = 0.0, sum = 0.0, mn = __builtin_inf(), mx = -__builtin_inf(), m2 = 0.0;
  for (int64_t base = (int64_t)w * kSummaryTile; base < a.N; base += (int64_t)W * kSummaryTile) {
    T v[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const int64_t i = base + j * NT + tid;
      v[j] = i < a.N ? x[i] : (T)__builtin_nan("");
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      const T e = v[j];
      const double d = (double)e;
      if (!(e == e) || (skip_inf && fabs(d) == __builtin_inf())) continue;
      if (p == 0) {
        cnt += 1.0;
        sum += d;
        mn = fmin(mn, d);
        mx = fmax(mx, d);
      } else if (p == 1) {
        const double c = d - mean;
        m2 += c * c;
      }
      const U key = KO::key(e);
      const int digit = (int)((key >> shift) & (U)(kBins - 1));
      const unsigned long long lead = p == 0 ? 0ull : (unsigned long long)(key >> (shift + kSummaryDigitBits));
      for (int u = 0; u < n_lead; ++u)
        if (lead == s.lead_prefix[u]) {
          atomicAdd(&s.hist[s.lead_slot[u] * kBins + digit], 1u);
          break;
        }
    }
  }
  __syncthreads();
  uint32_t* gh = rw.hist + (size_t)p * l.slots * kBins;
  for (int u = 0; u < n_lead; ++u) {
    const int slot = s.lead_slot[u];
    const uint32_t c = s.hist[slot * kBins + tid];
    if (c) atomicAdd(&gh[slot * kBins + tid], c);
  }
  if (p == 0) {
    cnt = group_reduce(cnt, kCount, s.red, tid);
    sum = group_reduce(sum, kSum, s.red, tid);
    mn = group_reduce(mn, kMin, s.red, tid);
    mx = group_reduce(mx, kMax, s.red, tid);
    if (tid == 0) {
      rw.part[kCount * kSummaryMaxWgs + w] = cnt;
      rw.part[kSum * kSummaryMaxWgs + w] = sum;
      rw.part[kMin * kSummaryMaxWgs + w] = mn;
      rw.part[kMax * kSummaryMaxWgs + w] = mx;
    }
  } else if (p == 1) {
    m2 = group_reduce(m2, kM2, s.red, tid);
    if (tid == 0) rw.part[kM2 * kSummaryMaxWgs + w] = m2;
  }
}

template <typename T>
__global__ void __launch_bounds__(NT) summary_finish_kernel(SummaryArgs a, Layout l, int W) {
  using KO = KeyOf<T>;
  __shared__ Shared s;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const RowWork rw = row_work(a, l, row);
  const double n = row_moment(rw.part, kCount, W, s.red, tid);
  const double sum = row_moment(rw.part, kSum, W, s.red, tid);
  const double mn = row_moment(rw.part, kMin, W, s.red, tid);
  const double mx = row_moment(rw.part, kMax, W, s.red, tid);
  const double m2 = row_moment(rw.part, kM2, W, s.red, tid);
  if (tracked(a, n) > 0) advance(a, l, rw, l.passes, n, s, tid);  // (uniform: every thread holds the same n)
  if (tid != 0) return;
  double* out = a.out + row * (DDR_SUMMARY_N_COLUMNS + a.K);
  const double nan = __builtin_nan("");
  out[DDR_SUMMARY_COUNT] = n;
  if (!(n > 0.0)) {
    for (int c = 1; c < DDR_SUMMARY_N_COLUMNS + a.K; ++c) out[c] = nan;
    return;
  }
  out[DDR_SUMMARY_MIN] = mn;
  out[DDR_SUMMARY_MAX] = mx;
  out[DDR_SUMMARY_MEAN] = sum / n;
  out[DDR_SUMMARY_STD] = sqrt(m2 / n);
  for (int k = 0; k < a.K; ++k) {
    const double lo = KO::value(s.prefix[2 * k]), hi = KO::value(s.prefix[2 * k + 1]);
    double r = lo;
    if (a.method == DDR_SUMMARY_LINEAR) {  // numpy's _lerp, each operation rounded on its own
      const double v = (n - 1.0) * a.q[k];
      const double g = v - floor(v);
      const double d = hi - lo;
      r = lo + d * g;
      if (g >= 0.5) r = hi - d * (1.0 - g);
    }
    out[DDR_SUMMARY_N_COLUMNS + k] = r;
  }
}

int workgroups_per_row(int64_t N) {
  const int64_t tiles = (N + kSummaryTile - 1) / kSummaryTile;
  return (int)(tiles < 1 ? 1 : (tiles > kSummaryMaxWgs ? kSummaryMaxWgs : tiles));
}

}  // namespace

size_t summary_work_bytes(int64_t R, int K, int elem_bytes) { return (size_t)R * layout_of(K, elem_bytes).row_bytes; }

template <typename T>
hipError_t launch_summary(const SummaryArgs& a, hipStream_t stream) {
  if (a.R == 0) return hipSuccess;
  const Layout l = layout_of(a.K, (int)sizeof(T));
  const int W = workgroups_per_row(a.N);
  const size_t words = (size_t)a.R * l.hist_words;
  const unsigned clear_wgs = (unsigned)((words + NT * 16 - 1) / (NT * 16) > 1024 ? 1024 : (words + NT * 16 - 1) / (NT * 16));
  hipLaunchKernelGGL(summary_clear_kernel, dim3(clear_wgs), dim3(NT), 0, stream, a, l);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int passes = a.K > 0 ? l.passes : 2;  // without quantiles only the moments' two passes
  for (int p = 0; p < passes; ++p) {
    hipLaunchKernelGGL(summary_pass_kernel<T>, dim3((unsigned)(a.R * W)), dim3(NT), 0, stream, a, l, p, W);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(summary_finish_kernel<T>, dim3((unsigned)a.R), dim3(NT), 0, stream, a, l, W);
  return hipGetLastError();
}

template hipError_t launch_summary<float>(const SummaryArgs&, hipStream_t);
template hipError_t launch_summary<double>(const SummaryArgs&, hipStream_t);

}  // namespace ddr
