// The hourly gauge value from a forward's saved states (mmc.py:405-412, 433-439), shared by the gauge
// kernels (gauges.hip) and the whole-period accumulation (period.hip).
#pragma once

#include "physics.h"
#include "route_args.h"

namespace ddr {

// Sum over gauge g's member reaches of Q(t) = clamp(x(t)), in list order; the carried state of step 0 is
// added unclamped (mmc.py:441, 557).
template <typename R>
__device__ __forceinline__ R gauge_sum(const GaugeArgs& a, const R* xsave, int64_t g, int64_t t) {
  R acc = R(0);
  for (int64_t k = a.goff[g]; k < a.goff[g + 1]; ++k) {
    const int P = a.pos_of_ref[a.gidx[k]];
    const BlockDesc B = a.s.blocks[a.block_of_pos[P]];
    const int r = P - B.pos0;
    const int64_t tick = t + a.s.off[P];
    const R x = xsave[a.T * B.pos0 + B.pre_dn + tick * B.nloc + r];
    acc = acc + ((t == 0 && a.carry) ? x : rmax_nan(x, R(a.qlb)));
  }
  return acc;
}

// out[g, t]: output[:, 0] = clamp(initial) (mmc.py:412); later steps are sums of clamped states
template <typename R>
__device__ __forceinline__ R gauge_hour(const GaugeArgs& a, const R* xsave, int64_t g, int64_t t) {
  const R acc = gauge_sum<R>(a, xsave, g, t);
  return (t == 0) ? rmax_nan(acc, R(a.qlb)) : acc;
}

}  // namespace ddr
