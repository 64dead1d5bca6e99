// The geometry predictor's two kernels around the KAN (src/ddr/geometry/predictor.py:164-316,
// adapters.py:159-164 and scripts/geometry_predictor.py:153-173 of the reference), fp32, gfx950.
//
// attr_prepare_kernel      raw catchment attributes (feature-major columns) -> the KAN's input x (N, F):
//                          unit conversion (fp64, only where a feature has one), out-of-distribution counts,
//                          NaN fill with the training mean, z-score -- and the transpose.  A workgroup owns 256
//                          rows: thread t reads element t of every column (coalesced), the normalised values
//                          cross an LDS tile, and the tile leaves as ONE contiguous 256 F 4-byte span of x.
// geometry_predict_kernel  the KAN's output u (N, O) in [0, 1] -> n / p_spatial / q_spatial (denormalize,
//                          routing/utils.py:166-185) -> the trapezoid of trapezoidal.py:62-97 at one discharge
//                          and slope per reach, 11 coalesced rows.  One thread per reach; the operations are
//                          physics.h's exact set in the reference's order.
#include "geopredict.h"

#include "internal.h"
#include "physics.h"

namespace ddr {

namespace {

constexpr int kTileRows = 256;

struct PrepArgs {
  int64_t N, feat_stride;
  int F;
  const float* raw;
  const double *scale, *offset;
  const int32_t* log10_flag;
  const float *mean, *std, *p10, *p90;
  float* x;
  unsigned long long* counts;  // (3, F): filled, below, above
};

// LDS: the tile [256][F | 1] floats (an odd row pitch: the 32 lanes of a ds_write_b32 group hit 32 banks), then
// the workgroup's counters [3][F]
__global__ void __launch_bounds__(kTileRows) attr_prepare_kernel(PrepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char psm[];
  const int t = threadIdx.x, F = a.F, FP = F | 1;
  float* tile = reinterpret_cast<float*>(psm);
  unsigned* cnt = reinterpret_cast<unsigned*>(tile + kTileRows * FP);
  const int64_t base = (int64_t)blockIdx.x * kTileRows;
  const int rows = a.N - base < kTileRows ? (int)(a.N - base) : kTileRows;
  const bool counting = a.counts != nullptr, ranges = counting && a.p10 != nullptr;
  if (counting) {
    for (int i = t; i < 3 * F; i += kTileRows) cnt[i] = 0;
    __syncthreads();
  }
  const bool live = t < rows;
  const bool lead = (t & 63) == 0;
  for (int f = 0; f < F; ++f) {
    // (per-feature values: wave-uniform loads)
    const double sc = a.scale[f], of = a.offset[f];
    const bool lg = a.log10_flag[f] != 0;
    const float mean = a.mean[f], sd = a.std[f];
    float v = live ? a.raw[(int64_t)f * a.feat_stride + base + t] : 0.0f;
    if (lg || sc != 1.0 || of != 0.0) {  // adapters.py:159-162
      double w = (double)v * sc + of;
      if (lg) w = log10(w < 1e-6 ? 1e-6 : w);  // (numpy's clip: a NaN stays NaN)
      v = (float)w;
    }
    const bool nan = v != v;
    if (counting) {
      const unsigned c0 = (unsigned)__popcll(__ballot(live && nan));
      if (lead && c0) atomicAdd(&cnt[f], c0);
      if (ranges) {  // predictor.py:341-342 (a NaN is neither)
        const unsigned c1 = (unsigned)__popcll(__ballot(live && v < a.p10[f]));
        const unsigned c2 = (unsigned)__popcll(__ballot(live && v > a.p90[f]));
        if (lead && c1) atomicAdd(&cnt[F + f], c1);
        if (lead && c2) atomicAdd(&cnt[2 * F + f], c2);
      }
    }
    if (nan) v = mean;                  // predictor.py:257-259
    tile[t * FP + f] = (v - mean) / sd;  // predictor.py:270 (IEEE division: +-inf and a zero std as torch)
  }
  __syncthreads();
  const int total = rows * F;
  const float inv_f = 1.0f / (float)F;
  float* xo = a.x + base * F;
  for (int e = t; e < total; e += kTileRows) {
    // e / F for e < 8192, F <= 32: (e + 0.5) / F is at least 1 / 64 away from an integer
    const int row = (int)(((float)e + 0.5f) * inv_f);
    xo[e] = tile[row * FP + (e - row * F)];
  }
  if (counting) {
    for (int i = t; i < 3 * F; i += kTileRows)
      if (cnt[i]) atomicAdd(&a.counts[i], (unsigned long long)cnt[i]);
  }
}

struct GeoArgs {
  int64_t N, out_stride;
  int O;
  const float *u, *Q, *S;
  GeoSlot slot[3];  // n, q_spatial, p_spatial
  float qlb, slb, dlb, bwlb;
  float* out;
};

// routing/utils.py:166-185 with the scalars as torch holds them (fp32); a slot without a column: its default
// (predictor.py:307-316)
__device__ __forceinline__ float denormalize(const GeoSlot& s, const float* ui) {
  if (s.column < 0) return s.value;
  const float lin = ui[s.column] * s.a + s.b;
  return s.log_space ? expf(lin) : lin;
}

// pow_pos where its domain holds (x normal and finite, |y ln x| < 700); the library's powf elsewhere (a NaN or
// infinite operand, a denormal ratio), so every IEEE class comes out as torch.pow's
__device__ __forceinline__ float pw_any(float x, float y, const PowK& K) {
  if (x >= 1.17549435e-38f && x < __builtin_inff() && __builtin_fabsf(y) <= 4.0f) return pw(x, y, nullptr, K);
  return powf(x, y);
}
// torch.clamp(min, max) with its NaN propagation (rclamp's v_med3_f32 returns a bound for a NaN)
__device__ __forceinline__ float rclamp_nan(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

template <bool Geom>
__global__ void __launch_bounds__(256) geometry_predict_kernel(GeoArgs a) {
  if constexpr (Geom) {
    load_math_tables();
    __syncthreads();
  }
  const PowK K = pow_consts();
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.N; i += step) {
    const float* ui = a.u + i * a.O;
    const float n = denormalize(a.slot[0], ui);
    const float q = denormalize(a.slot[1], ui);
    const float p = denormalize(a.slot[2], ui);
    float* o = a.out + i;
    if constexpr (!Geom) {
      o[0] = n;
      o[a.out_stride] = p;
      o[2 * a.out_stride] = q;
    } else {
      // predictor.py:211-214: NaN stays NaN (a reach without a slope gets NaN geometry)
      const float Q = rmax_nan(a.Q[i], a.qlb);
      const float S = rmax_nan(a.S[i], a.slb);
      // trapezoidal.py:62-97, the order of ddr_amd/geometry/trapezoidal.py:22-36
      const float qe = q + 1e-6f;
      const float num = (Q * n) * (qe + 1.0f);
      const float sqrtS = rsqrt_(S);
      const float den = p * sqrtS;
      const float expo = dv(3.0f, 5.0f + 3.0f * qe);
      const float depth = rmax_nan(pw_any(dv(num, den + 1e-8f), expo, K), a.dlb);
      const float tw = p * pw_any(depth, qe, K);
      const float ss = rclamp_nan(dv(tw * qe, 2.0f * depth), 0.5f, 50.0f);
      const float bw = rmax_nan(tw - (2.0f * ss) * depth, a.bwlb);
      const float area = ((tw + bw) * depth) * 0.5f;
      const float wp = bw + (2.0f * depth) * sq1p(1.0f + ss * ss);
      const float Rh = dv(area, wp);
      const float v = (dv(1.0f, n) * pw_any(Rh, two_thirds<float>(), K)) * sqrtS;
      const int64_t r = a.out_stride;
      o[DDR_GEOM_DEPTH * r] = depth;
      o[DDR_GEOM_TOP_WIDTH * r] = tw;
      o[DDR_GEOM_BOTTOM_WIDTH * r] = bw;
      o[DDR_GEOM_SIDE_SLOPE * r] = ss;
      o[DDR_GEOM_CROSS_SECTIONAL_AREA * r] = area;
      o[DDR_GEOM_WETTED_PERIMETER * r] = wp;
      o[DDR_GEOM_HYDRAULIC_RADIUS * r] = Rh;
      o[DDR_GEOM_VELOCITY * r] = v;
      o[DDR_GEOM_N * r] = n;
      o[DDR_GEOM_P_SPATIAL * r] = p;
      o[DDR_GEOM_Q_SPATIAL * r] = q;
    }
  }
}

}  // namespace

hipError_t launch_attr_prepare(int64_t N, int F, const float* raw, int64_t feat_stride, const double* scale,
                               const double* offset, const int32_t* log10_flag, const float* mean, const float* std,
                               const float* p10, const float* p90, float* x, long long* counts, hipStream_t stream) {
  if (N == 0) return hipSuccess;
  PrepArgs a{N, feat_stride, F, raw, scale, offset, log10_flag, mean, std, p10, p90, x,
             reinterpret_cast<unsigned long long*>(counts)};
  const size_t smem = sizeof(float) * kTileRows * (size_t)(F | 1) + sizeof(unsigned) * 3 * (size_t)F;  // <= 34.2 KB
  const int64_t nwg = (N + kTileRows - 1) / kTileRows;
  hipLaunchKernelGGL(attr_prepare_kernel, dim3((unsigned)nwg), dim3(kTileRows), smem, stream, a);
  return hipGetLastError();
}

hipError_t launch_geometry_predict(int64_t N, int O, const float* u, const GeoSlot (&slots)[3], const float* discharge,
                                   const float* slope, float discharge_lb, float slope_lb, float depth_lb,
                                   float bottom_width_lb, float* out, int64_t out_stride, hipStream_t stream) {
  if (N == 0) return hipSuccess;
  GeoArgs a{N, out_stride, O, u, discharge, slope, {slots[0], slots[1], slots[2]}, discharge_lb, slope_lb, depth_lb,
            bottom_width_lb, out};
  // grid-stride over 256-reach tiles: enough workgroups to fill the device, few enough that the math tables
  // are loaded a few thousand times, not once per tile
  const int64_t tiles = (N + 255) / 256;
  const unsigned nwg = (unsigned)(tiles < 4096 ? tiles : 4096);
  if (discharge)
    hipLaunchKernelGGL(geometry_predict_kernel<true>, dim3(nwg), dim3(256), kMathTabBytes, stream, a);
  else
    hipLaunchKernelGGL(geometry_predict_kernel<false>, dim3(nwg), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace ddr
