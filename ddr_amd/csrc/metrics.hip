// Per-gauge evaluation metrics of daily series (reference src/ddr/validation/metrics.py:11-256, called per
// mini-batch by scripts/train.py:106-115 and once per evaluation by scripts/test.py:107): the 18 values
// bias, mae, rmse, ub_rmse, fdc_rmse, corr, corr_spearman, r2, nse, flv, fhv, pbias, pbias_mid, kge, kge_12,
// rmse_low, rmse_high, rmse_mid of every gauge, from device-resident (G, D) fp32 series into a (18, G) fp64
// table, without a host sync.
//
// One *group* of NT threads owns a gauge: a wave (NT = 64; four gauges share a workgroup) for windows of up to
// kMetricsShortMaxDays days -- training batches: few days, many gauges -- and a workgroup of 1024 threads above
// (evaluation, up to kMetricsMaxDays days).  Both run the same code; only the group's barrier differs.  The
// group's LDS holds four arrays of P = 2^ceil(log2 D) slots: a (key, day) pair array the bitonic sorts run
// in, the sorted valid targets, and the targets' ranks by day (128 KB of the CU's 160 KB at P = 8192).
//
// A day is valid when its target is not NaN; n = the valid days.  Per gauge:
//   pass 1   sums of d = pred - target, |d|, d^2, pred, target over the valid days, of pred over all days
//   sort 1   valid targets ascending -> sT, and their average ranks (ties share the mean of their positions,
//            scipy.stats.rankdata) scattered by day -> rt
//   pass 2   the centred sums (two-pass: the means are known) while the valid preds are laid out for
//   sort 2   valid preds ascending: the low / mid / high slices [0, lo), [lo, hi), [hi, n) against sT
//            elementwise, lo = rint(0.3 n), hi = rint(0.98 n); the preds' ranks against rt (Spearman)
//   sort 3   all D preds (only when a target is NaN: otherwise sort 2 already is that sort) for the flow
//            duration curve: element (int)(i / 100.0 * N) of the descending sort, i = 0..99
// Every sum is fp64 over fp32 inputs widened on load, accumulated per thread over its strided elements, then
// across the wave by a fixed butterfly and across the waves in wave order: the result depends on the gauge's
// series alone, not on the launch it is part of.  The sorts order (key, day) pairs, a total order, so the
// permutation is unique.  NaN in pred is counted into nan_count and sorted as +inf (the caller raises).
#include "metrics.h"

#include "../../include/ddr_mc.h"

namespace ddr {

namespace {

struct MetArgs {
  const float* pred;
  const float* targ;
  int64_t ps, ts;  // row strides
  int64_t G;
  int D, P;
  double* out;  // (DDR_N_METRICS, G)
  int* nan_count;
};

constexpr int kRedMax = 12;  // the widest batch of sums reduced at once

template <int NT>
__device__ __forceinline__ void group_sync() {
  if constexpr (NT > 64) {
    __syncthreads();
  } else {
    // one wave: its LDS operations complete in order; the fence keeps the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}

// the group's sums of x[0..K) (every thread gets them): wave butterfly, then the waves' partials in wave order
template <int NT, int K>
__device__ __forceinline__ void group_sum(double (&x)[K], double* red, int tid) {
  static_assert(K <= kRedMax, "reduction scratch");
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x[k] += __shfl_xor(x[k], m, 64);
  }
  if constexpr (NT > 64) {
    constexpr int NW = NT / 64;
    if ((tid & 63) == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * NW + (tid >> 6)] = x[k];
    }
    __syncthreads();
    if (tid < K) {  // thread k adds the waves' partials of sum k
      double s = red[tid * NW];
#pragma unroll 1
      for (int w = 1; w < NW; ++w) s += red[tid * NW + w];
      red[kRedMax * NW + tid] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = red[kRedMax * NW + k];
    __syncthreads();
  }
}

// ascending bitonic sort of the P (key, day) pairs, ordered by key then day
template <int NT>
__device__ __forceinline__ void group_sort(float* key, int* day, int P, int tid) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const bool asc = (i & k) == 0;
        const float a = key[i], b = key[l];
        const int da = day[i], db = day[l];
        const bool gt = a > b || (a == b && da > db);
        if (gt == asc) {
          key[i] = b;
          key[l] = a;
          day[i] = db;
          day[l] = da;
        }
      }
      group_sync<NT>();
    }
  }
}

// the average 1-based rank of the value x among the ascending key[0..n): its run of equal keys covers
// positions [first, last), ranks first + 1 .. last
__device__ __forceinline__ float average_rank(const float* key, int n, float x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (key[m] < x) lo = m + 1; else hi = m;
  }
  const int first = lo;
  hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (key[m] <= x) lo = m + 1; else hi = m;
  }
  return 0.5f * (float)(first + lo + 1);  // (a half-integer <= 8192.5: exact)
}

__device__ __forceinline__ double clamp_corr(double r) {  // (NaN passes through)
  if (r > 1.0) r = 1.0;
  if (r < -1.0) r = -1.0;
  return r;
}

template <int NT>
__device__ __forceinline__ void gauge_metrics(const MetArgs& a, int64_t g, int tid, float* kA, int* iA, float* sT,
                                              float* rt, double* red) {
  const int D = a.D, P = a.P;
  const float* pr = a.pred + g * a.ps;
  const float* tr = a.targ + g * a.ts;
  const float inf = __builtin_inff();
  const double nan = __builtin_nan("");

  // pass 1, and the valid targets laid out for sort 1 (slots without one: +inf behind every real day)
  double s1[7] = {0, 0, 0, 0, 0, 0, 0};  // n, sum pred (all days), pred, target, d, |d|, d^2 (valid days)
  int bad = 0;
  for (int i = tid; i < P; i += NT) {
    float k = inf;
    int d = P + i;
    if (i < D) {
      const float p = pr[i], t = tr[i];
      bad += p != p;
      s1[1] += (double)p;
      if (t == t) {
        const double e = (double)p - (double)t;
        s1[0] += 1.0;
        s1[2] += (double)p;
        s1[3] += (double)t;
        s1[4] += e;
        s1[5] += fabs(e);
        s1[6] += e * e;
        k = t;
        d = i;
      }
    }
    kA[i] = k;
    iA[i] = d;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) bad += __shfl_xor(bad, m, 64);
  if ((tid & 63) == 0 && bad) atomicAdd(a.nan_count, bad);
  group_sum<NT>(s1, red, tid);
  group_sync<NT>();
  const int n = (int)s1[0];
  const double dn = (double)n;
  const double mean_p_all = s1[1] / (double)D, mean_p = s1[2] / dn, mean_t = s1[3] / dn;

  group_sort<NT>(kA, iA, P, tid);
  for (int j = tid; j < n; j += NT) {
    const float t = kA[j];
    sT[j] = t;
    rt[iA[j] & (P - 1)] = average_rank(kA, n, t);
  }
  group_sync<NT>();

  // pass 2, and the valid preds laid out for sort 2
  double s2[4] = {0, 0, 0, 0};  // (anomaly difference)^2, (p - mean p)^2, (t - mean t)^2, their product
  for (int i = tid; i < P; i += NT) {
    float k = inf;
    int d = P + i;
    if (i < D) {
      const float p = pr[i], t = tr[i];
      if (t == t) {
        const double cp = (double)p - mean_p, ct = (double)t - mean_t;
        const double u = ((double)p - mean_p_all) - ct;
        s2[0] += u * u;
        s2[1] += cp * cp;
        s2[2] += ct * ct;
        s2[3] += cp * ct;
        k = p == p ? p : inf;
        d = i;
      }
    }
    kA[i] = k;
    iA[i] = d;
  }
  group_sum<NT>(s2, red, tid);
  group_sync<NT>();
  group_sort<NT>(kA, iA, P, tid);

  // the sorted slices and the rank correlation
  const int lo = (int)rint(0.3 * dn), hi = (int)rint(0.98 * dn);
  const double mean_r = 0.5 * (dn + 1.0);
  double s3[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // per slice: sum e, sum e^2, sum t; ranks: xx, yy, xy
  for (int j = tid; j < n; j += NT) {
    const float p = kA[j];
    const double t = (double)sT[j];
    const double e = (double)p - t;
    const bool in_s[3] = {j < lo, j >= lo && j < hi, j >= hi};
#pragma unroll
    for (int s = 0; s < 3; ++s) {  // (selects, not an indexed accumulator: the sums stay in registers)
      s3[3 * s] += in_s[s] ? e : 0.0;
      s3[3 * s + 1] += in_s[s] ? e * e : 0.0;
      s3[3 * s + 2] += in_s[s] ? t : 0.0;
    }
    const double x = (double)average_rank(kA, n, p) - mean_r;
    const double y = (double)rt[iA[j] & (P - 1)] - mean_r;
    s3[9] += x * x;
    s3[10] += y * y;
    s3[11] += x * y;
  }
  group_sum<NT>(s3, red, tid);
  group_sync<NT>();

  // the flow duration curves: all D preds ascending in kA
  if (n < D) {  // (group-uniform)
    for (int i = tid; i < P; i += NT) {
      float k = inf;
      if (i < D) {
        const float p = pr[i];
        k = p == p ? p : inf;
      }
      kA[i] = k;
      iA[i] = i < D ? i : P + i;
    }
    group_sync<NT>();
    group_sort<NT>(kA, iA, P, tid);
  }
  double s4[1] = {0};
  for (int i = tid; i < 100; i += NT) {
    const double frac = (double)i / 100.0;  // (the quotient is rounded before the product, as numpy does)
    const int ip = (int)(frac * (double)D);
    const double fp = (double)kA[D - 1 - ip];
    double ft = 0.0;  // (no valid target: the reference's curve of zeros)
    if (n > 0) {
      const int it = (int)(frac * dn);
      ft = (double)sT[n - 1 - it];
    }
    s4[0] += (fp - ft) * (fp - ft);
  }
  group_sum<NT>(s4, red, tid);

  if (tid != 0) return;
  double m[DDR_N_METRICS];
  m[DDR_METRIC_BIAS] = s1[4] / dn;
  m[DDR_METRIC_MAE] = s1[5] / dn;
  m[DDR_METRIC_RMSE] = sqrt(s1[6] / dn);
  m[DDR_METRIC_UB_RMSE] = sqrt(s2[0] / dn);
  m[DDR_METRIC_FDC_RMSE] = sqrt(s4[0] / 100.0);
  m[DDR_METRIC_PBIAS] = s1[4] / s1[3] * 100.0;
  const double len_lo = (double)lo, len_mid = (double)(hi - lo), len_hi = (double)(n - hi);
  m[DDR_METRIC_FLV] = s3[0] / s3[2] * 100.0;
  m[DDR_METRIC_RMSE_LOW] = sqrt(s3[1] / len_lo);
  m[DDR_METRIC_PBIAS_MID] = s3[3] / s3[5] * 100.0;
  m[DDR_METRIC_RMSE_MID] = sqrt(s3[4] / len_mid);
  m[DDR_METRIC_FHV] = s3[6] / s3[8] * 100.0;
  m[DDR_METRIC_RMSE_HIGH] = sqrt(s3[7] / len_hi);
  if (n >= 2) {
    const double corr = clamp_corr(s2[3] / (sqrt(s2[1]) * sqrt(s2[2])));
    const double std_p = sqrt(s2[1] / dn), std_t = sqrt(s2[2] / dn);
    const double c1 = corr - 1.0, beta = mean_p / mean_t - 1.0;
    const double alpha = std_p / std_t - 1.0;
    const double gamma = (std_p * mean_t) / (std_t * mean_p) - 1.0;
    m[DDR_METRIC_CORR] = corr;
    m[DDR_METRIC_CORR_SPEARMAN] = clamp_corr(s3[11] / (sqrt(s3[9]) * sqrt(s3[10])));
    m[DDR_METRIC_KGE] = 1.0 - sqrt(c1 * c1 + alpha * alpha + beta * beta);
    m[DDR_METRIC_KGE_12] = 1.0 - sqrt(c1 * c1 + gamma * gamma + beta * beta);
    m[DDR_METRIC_NSE] = 1.0 - s1[6] / s2[2];
    m[DDR_METRIC_R2] = m[DDR_METRIC_NSE];
  } else {
    m[DDR_METRIC_CORR] = m[DDR_METRIC_CORR_SPEARMAN] = m[DDR_METRIC_KGE] = m[DDR_METRIC_KGE_12] = nan;
    m[DDR_METRIC_NSE] = m[DDR_METRIC_R2] = nan;
  }
#pragma unroll
  for (int k = 0; k < DDR_N_METRICS; ++k) a.out[(int64_t)k * a.G + g] = m[k];
}

constexpr int kShortWaves = 4;  // gauges per workgroup of the short-window kernel

// a wave per gauge: the wave's four arrays at smem + wave * 16 P bytes
__global__ void __launch_bounds__(64 * kShortWaves) metrics_short_kernel(MetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char msm[];
  const int wave = threadIdx.x >> 6;
  const int64_t g = (int64_t)blockIdx.x * kShortWaves + wave;
  if (g >= a.G) return;  // (the whole wave; this kernel has no workgroup barrier)
  float* kA = reinterpret_cast<float*>(msm) + (size_t)wave * 4 * a.P;
  gauge_metrics<64>(a, g, threadIdx.x & 63, kA, reinterpret_cast<int*>(kA + a.P), kA + 2 * (size_t)a.P,
                    kA + 3 * (size_t)a.P, nullptr);
}

constexpr int kLongThreads = 1024;

// a workgroup per gauge: four arrays of P slots, then the reduction scratch
__global__ void __launch_bounds__(kLongThreads) metrics_long_kernel(MetArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char msm[];
  float* kA = reinterpret_cast<float*>(msm);
  double* red = reinterpret_cast<double*>(msm + 16 * (size_t)a.P);
  gauge_metrics<kLongThreads>(a, blockIdx.x, threadIdx.x, kA, reinterpret_cast<int*>(kA + a.P),
                              kA + 2 * (size_t)a.P, kA + 3 * (size_t)a.P, red);
}

}  // namespace

hipError_t launch_metrics(int64_t G, int64_t D, const float* pred, int64_t pred_stride, const float* target,
                          int64_t target_stride, double* out, int32_t* nan_count, hipStream_t stream) {
  if (G == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(nan_count, 0, sizeof(int32_t), stream);
  if (e != hipSuccess) return e;
  int P = 64;
  while (P < D) P <<= 1;
  MetArgs a{pred, target, pred_stride, target_stride, G, (int)D, P, out, nan_count};
  if (D <= kMetricsShortMaxDays) {
    const size_t smem = (size_t)kShortWaves * 16 * P;  // <= 32 KB
    const int64_t nwg = (G + kShortWaves - 1) / kShortWaves;
    hipLaunchKernelGGL(metrics_short_kernel, dim3((unsigned)nwg), dim3(64 * kShortWaves), smem, stream, a);
    return hipGetLastError();
  }
  const size_t smem = 16 * (size_t)P + sizeof(double) * kRedMax * (kLongThreads / 64 + 1);  // <= 129.6 KB
  e = hipFuncSetAttribute((const void*)metrics_long_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(metrics_long_kernel, dim3((unsigned)G), dim3(kLongThreads), smem, stream, a);
  return hipGetLastError();
}

}  // namespace ddr
