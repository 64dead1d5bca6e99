// The device side of the BMI coupling (src/ddr/bmi/ddr_bmi.py of the reference: set_value 417-438, update_until
// 264-318, _update_output_cache 577-630), gfx950.  Four element-wise kernels around the one routing launch of a
// coupling interval; each thread owns a nexus id or a segment.
//
// bmi_nexus_plan_kernel  once per set_value of the nexus ids: thread i looks ids[i] up in the ascending key table
//                        (binary search) and, on a hit, raises src_of_seg[segment] to i with atomicMax.  The
//                        reference scatters in a sequential loop over i, so the LAST i that maps to a segment
//                        wins: the maximum.  Unknown ids touch nothing; src_of_seg starts at -1.
// bmi_set_inflow_kernel  per set_value of the flows: lateral[s] = flows[src[s]] where src[s] >= 0; the other
//                        segments keep their inflow (the reference overwrites mapped segments only).
// bmi_window_kernel      per update_until: the K sub-steps' inflows as the fp32 window (K + 1, N) the routing
//                        kernel reads -- fp64 interpolation, one rounding to fp32, exactly
//                        torch.tensor((1.0 - a) * prev + a * cur, dtype=float32) -- then prev = cur, cur = 0.
//                        No clamp: the routing kernel clamps its steps, and its hot start reads row 0 raw.
// bmi_outputs_kernel     per update_until: depth and velocity of the routed discharge (ddr_bmi.py:602-627) in the
//                        reference's fp32 operation order, with physics.h's exact operation set.  Its pow reads
//                        the math tables from LDS, as every caller of pw does.
#include "bmi.h"

#include "internal.h"
#include "physics.h"

namespace ddr {

namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) bmi_nexus_plan_kernel(int64_t M, const int32_t* __restrict__ ids,
                                                                   int64_t n_keys, const int64_t* __restrict__ keys,
                                                                   const int32_t* __restrict__ key_seg, int64_t N,
                                                                   int32_t* __restrict__ src_of_seg) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= M) return;
  const int64_t id = (int64_t)ids[i];
  int64_t lo = 0, hi = n_keys;  // first key >= id
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= n_keys || keys[lo] != id) return;
  const int32_t seg = key_seg[lo];
  if (seg < 0 || (int64_t)seg >= N) return;  // (a table built by ddr_bmi_nexus_table holds none)
  atomicMax(&src_of_seg[seg], (int32_t)i);
}

__global__ void __launch_bounds__(kThreads) bmi_set_inflow_kernel(int64_t N, const int32_t* __restrict__ src, int64_t M,
                                                                   const double* __restrict__ flows,
                                                                   double* __restrict__ lateral) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= N) return;
  const int32_t i = src[s];
  if (i >= 0 && (int64_t)i < M) lateral[s] = flows[i];
}

template <bool Linear>
__global__ void __launch_bounds__(kThreads) bmi_window_kernel(int64_t N, int K, int n_steps, double* __restrict__ prev,
                                                               double* __restrict__ cur, float* __restrict__ window,
                                                               int64_t row_stride) {
  const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= N) return;
  const double c = cur[s];
  float last = (float)c;
  if constexpr (Linear) {
    const double p = prev[s];
    for (int k = 0; k < K; ++k) {
      const double a = (double)(k + 1) / (double)n_steps;  // ddr_bmi.py:276
      last = (float)(((1.0 - a) * p) + (a * c));           // ddr_bmi.py:277, 281
      window[(int64_t)k * row_stride + s] = last;
    }
  } else {
    for (int k = 0; k < K; ++k) window[(int64_t)k * row_stride + s] = last;
  }
  window[(int64_t)K * row_stride + s] = last;  // (never read: the routing step t reads row t - 1)
  prev[s] = c;                                 // ddr_bmi.py:314
  cur[s] = 0.0;                                // ddr_bmi.py:318
}

struct OutArgs {
  int64_t N, p_stride, out_stride;
  const float *q, *n, *qs, *p, *S, *tw, *z;
  float dlb, bwlb;
  float* out;
};

// pow_pos where its domain holds (x normal and finite); the library's powf elsewhere (a NaN or infinite operand,
// a denormal ratio), so every IEEE class comes out as torch.pow's
__device__ __forceinline__ float pw_any(float x, float y, const PowK& K) {
  if (x >= 1.17549435e-38f && x < __builtin_inff() && __builtin_fabsf(y) <= 4.0f) return pw(x, y, nullptr, K);
  return powf(x, y);
}
// torch.clamp(min, max) with its NaN propagation
__device__ __forceinline__ float rclamp_nan(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ void __launch_bounds__(kThreads) bmi_outputs_kernel(OutArgs a) {
  load_math_tables();
  __syncthreads();
  const PowK K = pow_consts();
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < a.N; i += step) {
    const float Q = a.q[i], n = a.n[i], S = a.S[i], tw = a.tw[i], z = a.z[i];
    const float p = a.p[i * a.p_stride];
    const float qe = a.qs[i] + 1e-6f;                                     // ddr_bmi.py:607
    const float num = (Q * n) * (qe + 1.0f);                              // :611
    const float sqrtS = rsqrt_(S);                                        // pow(s0, 0.5)
    const float den = p * sqrtS;                                          // :612
    const float expo = dv(3.0f, 5.0f + 3.0f * qe);                        // :615
    const float depth = rmax_nan(pw_any(dv(num, den + 1e-8f), expo, K), a.dlb);  // :613-617
    const float bw = rmax_nan(tw - (2.0f * z) * depth, a.bwlb);           // :620
    const float area = ((tw + bw) * depth) * 0.5f;                        // :621
    const float wp = bw + (2.0f * depth) * sq1p(1.0f + z * z);            // :622
    const float Rh = dv(area, wp);                                        // :623
    const float v = (dv(1.0f, n) * pw_any(Rh, two_thirds<float>(), K)) * sqrtS;  // :626
    a.out[i] = Q;                                                         // :589
    a.out[a.out_stride + i] = rclamp_nan(v, 0.0f, 15.0f);                 // :627
    a.out[2 * a.out_stride + i] = depth;
  }
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

hipError_t launch_bmi_nexus_plan(int64_t M, const int32_t* ids, int64_t n_keys, const int64_t* keys,
                                 const int32_t* key_seg, int64_t N, int32_t* src_of_seg, hipStream_t stream) {
  if (N == 0) return hipSuccess;
  const hipError_t e = hipMemsetAsync(src_of_seg, 0xFF, sizeof(int32_t) * (size_t)N, stream);  // -1
  if (e != hipSuccess) return e;
  if (M == 0 || n_keys == 0) return hipSuccess;
  hipLaunchKernelGGL(bmi_nexus_plan_kernel, dim3(blocks_for(M)), dim3(kThreads), 0, stream, M, ids, n_keys, keys,
                     key_seg, N, src_of_seg);
  return hipGetLastError();
}

hipError_t launch_bmi_set_inflow(int64_t N, const int32_t* src, int64_t M, const double* flows, double* lateral,
                                 hipStream_t stream) {
  if (N == 0 || M == 0) return hipSuccess;
  hipLaunchKernelGGL(bmi_set_inflow_kernel, dim3(blocks_for(N)), dim3(kThreads), 0, stream, N, src, M, flows, lateral);
  return hipGetLastError();
}

hipError_t launch_bmi_window(int64_t N, int K, int n_steps, bool linear, double* prev, double* cur, float* window,
                             int64_t row_stride, hipStream_t stream) {
  if (N == 0) return hipSuccess;
  if (linear)
    hipLaunchKernelGGL(bmi_window_kernel<true>, dim3(blocks_for(N)), dim3(kThreads), 0, stream, N, K, n_steps, prev,
                       cur, window, row_stride);
  else
    hipLaunchKernelGGL(bmi_window_kernel<false>, dim3(blocks_for(N)), dim3(kThreads), 0, stream, N, K, n_steps, prev,
                       cur, window, row_stride);
  return hipGetLastError();
}

hipError_t launch_bmi_outputs(int64_t N, const float* q, const float* n, const float* q_spatial, const float* p,
                              int64_t p_stride, const float* slope, const float* top_width, const float* side_slope,
                              float depth_lb, float bottom_width_lb, float* out, int64_t out_stride,
                              hipStream_t stream) {
  if (N == 0) return hipSuccess;
  OutArgs a{N, p_stride, out_stride, q, n, q_spatial, p, slope, top_width, side_slope, depth_lb, bottom_width_lb, out};
  // grid-stride over 256-segment tiles: few enough workgroups that the math tables are loaded a few thousand
  // times, not once per tile
  const int64_t tiles = (N + kThreads - 1) / kThreads;
  const unsigned nwg = (unsigned)(tiles < 4096 ? tiles : 4096);
  hipLaunchKernelGGL(bmi_outputs_kernel, dim3(nwg), dim3(kThreads), kMathTabBytes, stream, a);
  return hipGetLastError();
}

}  // namespace ddr
