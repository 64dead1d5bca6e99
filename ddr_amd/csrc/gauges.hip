// Kernels that read a forward's saved states per gauge or per reach: the hourly gauge reduction, the
// t = 0 clamp mask, the fused daily objective and its adjoint seed, and Q(t) of every reach.
#include "gauge_sum.h"

namespace ddr {

// ============================================================================================
// Gauge reduction: out[g, t] = sum_{k} clamp(x_t[idx_k])  (mmc.py:405-411, 433-439)
// ============================================================================================
template <typename R>
__global__ void gauge_reduce_kernel(GaugeArgs a, const R* xsave, R* out) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.G * a.T) return;
  const int64_t g = w / a.T, t = w % a.T;
  out[g * a.T + t] = gauge_hour<R>(a, xsave, g, t);
}

// mask[g] = 1 where the t = 0 gauge sum (before its clamp, as gauge_reduce_kernel) is >= q_lb:
// torch.clamp's backward passes the gradient there (inclusive at the bound).
template <typename R>
__global__ void gauge_mask0_kernel(GaugeArgs a, const R* xsave, unsigned char* mask) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.G) return;
  mask[g] = (gauge_sum<R>(a, xsave, g, 0) >= R(a.qlb)) ? 1 : 0;
}

// ============================================================================================
// Gauge-mode training objective, fused: hourly gauge sums -> trim -> daily area means
// (scripts/train.py:78-82: downsample(runoff[:, 13 : -11 + tau], num_days), io/functions.py:7-23,
// F.interpolate(mode="area") = adaptive average pooling: day d averages hours
// [floor(d L / D), ceil((d + 1) L / D)) of the L-hour trimmed window).  The (G, T) hourly series is
// never materialised; only (G, D) leaves the kernel.
// ============================================================================================
__host__ __device__ inline int64_t pool_start(int64_t d, int64_t L, int64_t D) { return (d * L) / D; }
__host__ __device__ inline int64_t pool_end(int64_t d, int64_t L, int64_t D) { return ((d + 1) * L + D - 1) / D; }

template <typename R>
__global__ void gauge_daily_kernel(GaugeArgs a, const R* xsave, int64_t t0, int64_t L, int64_t D, R* out) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= a.G * D) return;
  const int64_t g = w / D, d = w % D;
  const int64_t h0 = pool_start(d, L, D), h1 = pool_end(d, L, D);
  R sum = R(0);
  for (int64_t h = h0; h < h1; ++h) sum = sum + gauge_hour<R>(a, xsave, g, t0 + h);
  out[w] = sum / R(h1 - h0);  // adaptive_avg_pool: sum / kh / kw with kh = 1
}

// Adjoint seed of the pooling: dL/dhourly[g, t] = sum over the days d whose window holds t - t0 of
// dL/ddaily[g, d] / len(d) (ascending d, as adaptive_avg_pool's backward accumulates), 0 outside
// the trimmed window.  Feeds the gauge-mode routing adjoint.
template <typename R>
__global__ void gauge_daily_seed_kernel(int64_t G, int64_t T, int64_t t0, int64_t L, int64_t D, const R* gd, R* gh) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= G * T) return;
  const int64_t g = w / T, t = w % T, h = t - t0;
  R acc = R(0);
  if (h >= 0 && h < L) {
    const int64_t dc = (h * D) / L;
    const int64_t dlo = dc > 0 ? dc - 1 : 0, dhi = dc + 1 < D ? dc + 1 : D - 1;
    for (int64_t d = dlo; d <= dhi; ++d)
      if (h >= pool_start(d, L, D) && h < pool_end(d, L, D)) acc = acc + gd[g * D + d] / R(pool_end(d, L, D) - pool_start(d, L, D));
  }
  gh[w] = acc;
}

// Q(t) of every reach, in reference order, from a forward's saved states (ddr_state_f32/f64): clamp(x(t)),
// the carried state at t = 0 unclamped (mmc.py:441, 557) -- e.g. Q(T - 2), the state the reported
// geometry of the last step was computed from (mmc.py:161-162), for that geometry's VJP
template <typename R>
__global__ void state_at_kernel(DevSchedule s, int64_t N, int64_t T, int64_t t, R qlb, int carry, const R* xsave,
                                R* out) {
  const int64_t P = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (P >= N) return;
  const BlockDesc B = s.blocks[s.block_of_pos[P]];
  const R x = xsave[T * B.pos0 + B.pre_dn + (t + s.off[P]) * B.nloc + (P - B.pos0)];
  out[s.ref[P]] = (t == 0 && carry) ? x : rmax_nan(x, qlb);
}

template <typename R>
hipError_t launch_state_at(const Graph* g, int64_t T, int64_t t, double qlb, bool carry, const R* xsave, R* out,
                           hipStream_t stream) {
  if (g->n == 0) return hipSuccess;
  hipLaunchKernelGGL(state_at_kernel<R>, dim3((unsigned)((g->n + 255) / 256)), dim3(256), 0, stream, g->dev, g->n, T, t,
                     R(qlb), carry ? 1 : 0, xsave, out);
  return hipGetLastError();
}
template hipError_t launch_state_at<float>(const Graph*, int64_t, int64_t, double, bool, const float*, float*, hipStream_t);
template hipError_t launch_state_at<double>(const Graph*, int64_t, int64_t, double, bool, const double*, double*,
                                            hipStream_t);

template <typename R>
hipError_t launch_gauge_mask0(const GaugeArgs& a, const R* xsave, unsigned char* mask, hipStream_t stream) {
  if (a.G == 0) return hipSuccess;
  hipLaunchKernelGGL(gauge_mask0_kernel<R>, dim3((unsigned)((a.G + 255) / 256)), dim3(256), 0, stream, a, xsave, mask);
  return hipGetLastError();
}

template <typename R>
hipError_t launch_gauge(const GaugeArgs& a, const R* xsave, R* out, hipStream_t stream) {
  const int64_t total = a.G * a.T;
  if (total == 0) return hipSuccess;
  const int threads = 256;
  const unsigned blocks = (unsigned)((total + threads - 1) / threads);
  hipLaunchKernelGGL(gauge_reduce_kernel<R>, dim3(blocks), dim3(threads), 0, stream, a, xsave, out);
  return hipGetLastError();
}

template <typename R>
hipError_t launch_gauge_daily(const GaugeArgs& a, const R* xsave, int64_t t0, int64_t L, int64_t D, R* out,
                              hipStream_t stream) {
  const int64_t total = a.G * D;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(gauge_daily_kernel<R>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a, xsave, t0,
                     L, D, out);
  return hipGetLastError();
}

template <typename R>
hipError_t launch_gauge_daily_seed(int64_t G, int64_t T, int64_t t0, int64_t L, int64_t D, const R* gd, R* gh,
                                   hipStream_t stream) {
  const int64_t total = G * T;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(gauge_daily_seed_kernel<R>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, G, T, t0,
                     L, D, gd, gh);
  return hipGetLastError();
}

template hipError_t launch_gauge_mask0<float>(const GaugeArgs&, const float*, unsigned char*, hipStream_t);
template hipError_t launch_gauge_mask0<double>(const GaugeArgs&, const double*, unsigned char*, hipStream_t);
template hipError_t launch_gauge<float>(const GaugeArgs&, const float*, float*, hipStream_t);
template hipError_t launch_gauge<double>(const GaugeArgs&, const double*, double*, hipStream_t);

template hipError_t launch_gauge_daily<float>(const GaugeArgs&, const float*, int64_t, int64_t, int64_t, float*, hipStream_t);
template hipError_t launch_gauge_daily<double>(const GaugeArgs&, const double*, int64_t, int64_t, int64_t, double*,
                                               hipStream_t);
template hipError_t launch_gauge_daily_seed<float>(int64_t, int64_t, int64_t, int64_t, int64_t, const float*, float*,
                                                   hipStream_t);
template hipError_t launch_gauge_daily_seed<double>(int64_t, int64_t, int64_t, int64_t, int64_t, const double*, double*,
                                                    hipStream_t);

}  // namespace ddr
