// Whole-period inference: the daily means of a period routed in several launches (scripts/router.py:88-201,
// scripts/test.py:57-112; scripts_utils.compute_daily_runoff: predictions[:, 13 + tau : -11 + tau] pooled to
// days of 24 hours).  The reference keeps the (R, hours) array of the whole period on the host and pools it at
// the end; here every routing launch is followed by one accumulation over its own saved states, and only the
// (R, days) series exists.
//
// The window starts at hour 13 + tau and launches start at multiples of 24, so every launch boundary splits a
// day.  Rule (one call per launch, stream-ordered, in period order): for every (row, day) whose 24-hour window
// meets the launch's hours, sum the shared hours in ascending order -- from 0 if they hold the window's first
// hour, else from the partial sum the previous call left in daily[row, day] -- and divide by 24 if they hold the
// window's last hour.  A finished day is then the same sequence of additions as one pass over its 24 hours:
// bit-identical whatever the chunking, no atomics, no clearing (days no call touches are not written).
//
// The hourly value is what the hourly paths give for the same launch: the gauge sum of gauge_reduce_kernel
// (gauge_hour, gauge_sum.h), or in all-reach mode max(x, q_lb), the forward's (N, T) runoff entry.
#include "period.h"

#include "gauge_sum.h"
#include "internal.h"
#include "physics.h"

namespace ddr {

namespace {

inline int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0)) ? 1 : 0); }

constexpr int kTileReaches = 64;  // one wave's lanes: consecutive positions, contiguous along a tick row
constexpr int kTileDays = 32;     // days per tile (a 30-day chunk meets 31 windows)
constexpr int kTileWaves = 4;

// the launch steps [t_lo, t_hi) of day d's window, and whether they hold its first / last hour
struct DaySpan {
  int64_t t_lo, t_hi;
  bool first, last;
};
__device__ __forceinline__ DaySpan span_of(const PeriodArgs& p, int64_t d) {
  const int64_t w0 = p.first_hour + 24 * d, w1 = w0 + 24;
  const int64_t lo = w0 > p.h0 ? w0 : p.h0;
  const int64_t hi = w1 < p.h0 + p.T ? w1 : p.h0 + p.T;
  return {lo - p.h0, hi - p.h0, lo == w0, hi == w1};
}

// Gauge rows: 32 lanes per (gauge, day of this launch).  Lane k takes the window's hour k -- the hourly values are
// independent, and each is a chain of dependent index loads -- then the 24 values are added in ascending order
// (lane shuffles; every lane keeps the same running sum) and lane 0 stores.  One thread per (gauge, day) walking
// its 24 hours took 25 us per 30-day chunk of 256 gauges, all of it load latency.
constexpr int kGaugeLanes = 32;
template <typename R>
__global__ void __launch_bounds__(256) period_gauge_kernel(GaugeArgs a, PeriodArgs p, const R* xsave, R* daily) {
  const int lane = threadIdx.x % kGaugeLanes;
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGaugeLanes;
  const bool live = w < a.G * p.nd;
  const int64_t g = live ? w / p.nd : 0, d = p.d_lo + (live ? w % p.nd : 0);
  const DaySpan sp = span_of(p, d);
  const int64_t t = p.first_hour + 24 * d + lane - p.h0;  // this lane's step of the launch
  const bool mine = live && lane < 24 && t >= sp.t_lo && t < sp.t_hi;
  const R v = mine ? gauge_hour<R>(a, xsave, g, t) : R(0);
  R* out = daily + g * p.D + d;
  R sum = (live && !sp.first) ? *out : R(0);
  const int k0 = (int)(sp.t_lo - (p.first_hour + 24 * d - p.h0)), k1 = k0 + (int)(sp.t_hi - sp.t_lo);
  for (int k = 0; k < 24; ++k) {
    const R vk = __shfl(v, k, kGaugeLanes);
    if (k >= k0 && k < k1) sum = sum + vk;
  }
  if (live && lane == 0) *out = sp.last ? sum / R(24) : sum;
}

// a reach's column of the schedule-layout x_save (state_at_kernel's access, gauges.hip): step t at xs[t * nloc]
template <typename R>
struct ReachColumn {
  const R* xs;
  int64_t nloc;
  int64_t ref;
};
template <typename R>
__device__ __forceinline__ ReachColumn<R> column_of(const DevSchedule& s, int64_t T, int64_t P, const R* xsave) {
  const BlockDesc B = s.blocks[s.block_of_pos[P]];
  return {xsave + T * B.pos0 + B.pre_dn + (int64_t)s.off[P] * B.nloc + (P - B.pos0), (int64_t)B.nloc,
          (int64_t)s.ref[P]};
}
template <typename R>
__device__ __forceinline__ R day_value(const ReachColumn<R>& c, const PeriodArgs& p, int64_t d, const R* daily) {
  const DaySpan sp = span_of(p, d);
  const R qlb = R(p.qlb);
  if (sp.first && sp.last) {
    // a whole day (all but two of a launch's): the 24 loads are independent, issue them together
    const R* x = c.xs + sp.t_lo * c.nloc;
    R v[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) v[k] = x[k * c.nloc];
    R sum = R(0);
#pragma unroll
    for (int k = 0; k < 24; ++k) sum = sum + rmax_nan(v[k], qlb);
    return sum / R(24);
  }
  R sum = sp.first ? R(0) : daily[c.ref * p.D + d];
  for (int64_t t = sp.t_lo; t < sp.t_hi; ++t) sum = sum + rmax_nan(c.xs[t * c.nloc], qlb);
  return sp.last ? sum / R(24) : sum;
}

// All reaches, tiled: a workgroup takes 64 consecutive positions x up to 32 days.  Lanes are positions, so
// the reads along a tick row are contiguous; each wave takes every fourth day.  The (N, D) output is indexed
// by reference id, so the lanes' rows are scattered but each row's days are contiguous: the tile goes through
// LDS and is written as one run of days per row.
template <typename R>
__global__ void __launch_bounds__(kTileReaches* kTileWaves)
    period_all_tiled_kernel(DevSchedule s, int64_t N, PeriodArgs p, const R* xsave, R* daily) {
  __shared__ R tile[kTileReaches][kTileDays + 1];
  __shared__ int64_t refs[kTileReaches];
  const int lane = threadIdx.x % kTileReaches, wave = threadIdx.x / kTileReaches;
  const int64_t P0 = (int64_t)blockIdx.x * kTileReaches;
  const int j0 = (int)blockIdx.y * kTileDays;
  const int nj = p.nd - j0 < kTileDays ? p.nd - j0 : kTileDays;
  if (P0 + lane < N) {
    const ReachColumn<R> c = column_of<R>(s, p.T, P0 + lane, xsave);
    if (wave == 0) refs[lane] = c.ref;
    for (int j = wave; j < nj; j += kTileWaves) tile[lane][j] = day_value<R>(c, p, p.d_lo + j0 + j, daily);
  }
  __syncthreads();
  const int nr = N - P0 < kTileReaches ? (int)(N - P0) : kTileReaches;
  for (int i = threadIdx.x; i < nr * nj; i += kTileReaches * kTileWaves) {
    const int r = i / nj, j = i % nj;
    daily[refs[r] * p.D + p.d_lo + j0 + j] = tile[r][j];
  }
}

// All reaches, direct: one thread per (position, day), positions along the lanes, each storing its own value
template <typename R>
__global__ void __launch_bounds__(256) period_all_direct_kernel(DevSchedule s, int64_t N, PeriodArgs p, const R* xsave,
                                                                R* daily) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= N * p.nd) return;
  const int64_t P = w % N, d = p.d_lo + w / N;
  const ReachColumn<R> c = column_of<R>(s, p.T, P, xsave);
  daily[c.ref * p.D + d] = day_value<R>(c, p, d, daily);
}

}  // namespace

void period_days(int64_t T, int64_t D, int64_t h0, int64_t first_hour, int64_t* d_lo, int32_t* nd) {
  // window [first_hour + 24 d, + 24) meets [h0, h0 + T): 24 d > h0 - first_hour - 24 and 24 d < h0 + T - first_hour
  int64_t lo = floor_div(h0 - first_hour - 24, 24) + 1;
  int64_t hi = floor_div(h0 + T - first_hour - 1, 24) + 1;  // exclusive
  if (lo < 0) lo = 0;
  if (hi > D) hi = D;
  *d_lo = lo;
  *nd = hi > lo ? (int32_t)(hi - lo) : 0;
}

template <typename R>
hipError_t launch_period_gauge(const GaugeArgs& a, const PeriodArgs& p, const R* xsave, R* daily, hipStream_t stream) {
  const int64_t total = a.G * p.nd * kGaugeLanes;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(period_gauge_kernel<R>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, p, xsave,
                     daily);
  return hipGetLastError();
}

template <typename R>
hipError_t launch_period_all(const Graph* g, const PeriodArgs& p, bool direct, const R* xsave, R* daily,
                             hipStream_t stream) {
  if (g->n == 0 || p.nd == 0) return hipSuccess;
  if (direct) {
    const int64_t total = g->n * p.nd;
    hipLaunchKernelGGL(period_all_direct_kernel<R>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, g->dev,
                       g->n, p, xsave, daily);
  } else {
    const dim3 grid((unsigned)((g->n + kTileReaches - 1) / kTileReaches), (unsigned)((p.nd + kTileDays - 1) / kTileDays));
    hipLaunchKernelGGL(period_all_tiled_kernel<R>, grid, dim3(kTileReaches * kTileWaves), 0, stream, g->dev, g->n, p,
                       xsave, daily);
  }
  return hipGetLastError();
}

template hipError_t launch_period_gauge<float>(const GaugeArgs&, const PeriodArgs&, const float*, float*, hipStream_t);
template hipError_t launch_period_gauge<double>(const GaugeArgs&, const PeriodArgs&, const double*, double*, hipStream_t);
template hipError_t launch_period_all<float>(const Graph*, const PeriodArgs&, bool, const float*, float*, hipStream_t);
template hipError_t launch_period_all<double>(const Graph*, const PeriodArgs&, bool, const double*, double*, hipStream_t);

}  // namespace ddr
