// Whole-period inference (period.hip): the daily means of a period routed in several launches, accumulated
// across launch boundaries; called by the C ABI (capi.cpp: ddr_period_daily_*).
#pragma once

#include "route_args.h"

namespace ddr {

// One launch's share of the period's daily series: period hours [h0, h0 + T) of the launch whose saved
// states are `xsave`, into daily (R, D); day d = hours [first_hour + 24 d, first_hour + 24 d + 24).
struct PeriodArgs {
  int64_t T, D;
  int64_t h0, first_hour;
  int64_t d_lo;  // first day whose window meets [h0, h0 + T)
  int32_t nd;    // days from d_lo on that do
  double qlb;
};
// the days [d_lo, d_lo + nd) of (0 <= d < D) whose window meets [h0, h0 + T); nd = 0: none
void period_days(int64_t T, int64_t D, int64_t h0, int64_t first_hour, int64_t* d_lo, int32_t* nd);

// gauge rows: the gauge sums of gauge_reduce_kernel (gauges.hip), `a` from gauge_args (capi.cpp)
template <typename R>
hipError_t launch_period_gauge(const GaugeArgs& a, const PeriodArgs& p, const R* xsave, R* daily, hipStream_t stream);
// every reach in reference order: the value the forward's (N, T) runoff holds.  direct: one thread per
// (reach, day) storing its own value, instead of the LDS tile written as per-row runs of days
template <typename R>
hipError_t launch_period_all(const Graph* g, const PeriodArgs& p, bool direct, const R* xsave, R* daily,
                             hipStream_t stream);

}  // namespace ddr
