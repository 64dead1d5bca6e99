// Masked training objectives over the gauges' daily series (the reference loop's scripts/train.py:84-97: drop the
// gauges whose observations hold a NaN, l1_loss over the rest after the warm-up, backward): L1, MSE, 1 - NSE and
// 1 - KGE with a NaN observation as a missing day and a dropped gauge as a mask, the loss and its gradient w.r.t.
// the predictions without a host sync, in three launches:
//   objective_*_kernel        per gauge, over its valid days V_g: the moments, the term and what the gradient needs
//                             of them (two passes: the means, then the centred sums), into the work table;
//   objective_reduce_kernel   one workgroup: the gauges' numerators and denominators in a fixed order -> the loss
//                             and the normaliser W;
//   objective_grad_kernel     every element of grad once (exactly +0.0 outside V_g and for gauges that are not used).
// The gradient needs W, a sum over all gauges, so it cannot be written by the launch that forms the moments; it
// re-reads the rows (the training batch is L2-resident) and is skipped when no gradient is asked for.
//
// Dispatch of the first launch follows metrics.hip: up to kObjectiveShortMaxDays days a wave owns a gauge (four
// gauges share a workgroup, no workgroup barrier), the row in registers for both passes, eight days per lane, and the
// reduction a cross-lane butterfly; longer windows take a workgroup of 256 threads per gauge, the waves' partials
// added in wave order through LDS.  Every sum is fp64 over the fp32 inputs widened on load, per thread over its
// strided days, in an order that depends on D alone: a gauge's values do
// not depend on the launch it is part of (a masked gauge and the same gauge in a physically filtered batch agree
// bit for bit), and two runs are identical.  No atomics.
#include "objective.h"

#include "../../include/ddr_mc.h"

namespace ddr {

namespace {

// rows of the work table (each G doubles), then the scalar W at kWorkRows * G
enum { kNum = 0, kDen, kUsed, kWgt, kU0, kU1, kU2, kMeanP, kMeanO, kWorkRows };

template <int NT, int K>
__device__ __forceinline__ void group_sum(double (&x)[K], double* red, int tid) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x[k] += __shfl_xor(x[k], m, 64);
  }
  if constexpr (NT > 64) {
    constexpr int NW = NT / 64;
    __syncthreads();  // (the scratch may still be read from the previous call)
    if ((tid & 63) == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * NW + (tid >> 6)] = x[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {  // every thread adds the waves' partials in wave order
      double s = red[k * NW];
#pragma unroll
      for (int w = 1; w < NW; ++w) s += red[k * NW + w];
      x[k] = s;
    }
  }
}

__device__ __forceinline__ void pass1(float p, float o, double (&s)[5]) {
  if (o == o) {
    const double e = (double)p - (double)o;
    s[0] += 1.0;
    s[1] += (double)p;
    s[2] += (double)o;
    s[3] += fabs(e);
    s[4] += e * e;
  }
}

__device__ __forceinline__ void pass2(float p, float o, double mp, double mo, double (&s)[3]) {
  if (o == o) {
    const double cp = (double)p - mp, co = (double)o - mo;
    s[0] += cp * cp;
    s[1] += co * co;
    s[2] += cp * co;
  }
}

// thread 0 of the group: the term, the loss's numerator and denominator and the gradient's coefficients of gauge g
__device__ void gauge_finish(const ObjectiveArgs& a, int64_t g, const double (&s1)[5], const double (&s2)[3]) {
  const double n = s1[0], A = s1[3], S = s1[4];
  const double mp = s1[1] / n, mo = s1[2] / n;
  const double Spp = s2[0], Soo = s2[1], Spo = s2[2];
  const double w = a.weight ? (double)a.weight[g] : 1.0;
  bool used = false;
  double term = 0.0, num = 0.0, den = 0.0, u0 = 0.0, u1 = 0.0, u2 = 0.0;
  if (a.kind == DDR_OBJECTIVE_L1) {
    used = n >= 1.0;
    term = A / n;
    num = w * A;
    den = w * n;
  } else if (a.kind == DDR_OBJECTIVE_MSE) {
    used = n >= 1.0;
    term = S / n;
    num = w * S;
    den = w * n;
    u2 = 2.0;
  } else if (a.kind == DDR_OBJECTIVE_NSE) {
    used = n >= 2.0 && (Soo != 0.0 || a.eps > 0.0);
    const double sd = sqrt(Soo / n) + a.eps;
    const double d2 = n * (sd * sd);
    term = S / d2;
    num = w * term;
    den = w;
    u2 = 2.0 / d2;
  } else {
    // ("not equal to zero" fails for NaN: a NaN prediction keeps the gauge counted and shows in the loss)
    used = n >= 2.0 && !(Soo == 0.0) && !(mo == 0.0) && !(Spp == 0.0);
    const double sp = sqrt(Spp / n), so = sqrt(Soo / n), rt = sqrt(Spp * Soo);
    const double r = Spo / rt, al = sp / so, be = mp / mo;
    const double E = sqrt((r - 1.0) * (r - 1.0) + (al - 1.0) * (al - 1.0) + (be - 1.0) * (be - 1.0));
    term = E;
    num = w * term;
    den = w;
    if (!(E == 0.0)) {
      u0 = (be - 1.0) / (n * mo) / E;
      u1 = (r - 1.0) / rt / E;
      u2 = ((al - 1.0) / (n * sp * so) - (r - 1.0) * r * sqrt(Soo / Spp) / rt) / E;
    }
  }
  const int64_t G = a.G;
  double* wk = a.work;
  wk[kNum * G + g] = used ? num : 0.0;
  wk[kDen * G + g] = used ? den : 0.0;
  wk[kUsed * G + g] = used ? 1.0 : 0.0;
  wk[kWgt * G + g] = w;
  wk[kU0 * G + g] = u0;
  wk[kU1 * G + g] = u1;
  wk[kU2 * G + g] = u2;
  wk[kMeanP * G + g] = mp;
  wk[kMeanO * G + g] = mo;
  if (a.terms) {
    a.terms[g] = used ? term : __builtin_nan("");
    a.terms[G + g] = n;
    a.terms[2 * G + g] = used ? 1.0 : 0.0;
  }
}

constexpr int NPL = (int)(kObjectiveShortMaxDays / 64);  // days per lane of the one-wave kernel

// a wave per gauge, the row in registers: day tid + 64 k in slot k (an observation outside V_g is held as NaN)
__global__ void __launch_bounds__(64 * kObjectiveShortWaves) objective_short_kernel(ObjectiveArgs a) {
  const int tid = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * kObjectiveShortWaves + (threadIdx.x >> 6);
  if (g >= a.G) return;  // (the whole wave; this kernel has no workgroup barrier)
  const float* pr = a.daily + g * a.ds;
  const float* ob = a.obs + g * a.os;
  const bool live = !(a.drop && a.drop[g]);
  const float nanf = __builtin_nanf("");
  float p[NPL], o[NPL];
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int i = tid + 64 * k;
    const bool in = live && i >= a.wd && i < a.D;
    p[k] = in ? pr[i] : 0.0f;
    o[k] = in ? ob[i] : nanf;
  }
  double s1[5] = {0, 0, 0, 0, 0};  // n, sum p, sum o, sum |p - o|, sum (p - o)^2
#pragma unroll
  for (int k = 0; k < NPL; ++k) pass1(p[k], o[k], s1);
  group_sum<64>(s1, nullptr, tid);
  double s2[3] = {0, 0, 0};  // sum (p - mean p)^2, (o - mean o)^2, their product
  if (a.kind >= DDR_OBJECTIVE_NSE) {
    const double mp = s1[1] / s1[0], mo = s1[2] / s1[0];
#pragma unroll
    for (int k = 0; k < NPL; ++k) pass2(p[k], o[k], mp, mo, s2);
    group_sum<64>(s2, nullptr, tid);
  }
  if (tid == 0) gauge_finish(a, g, s1, s2);
}

constexpr int kLongThreads = 256;

// a workgroup per gauge: the second pass reads the row again (it is in L2: at most 2 x 32 KB)
__global__ void __launch_bounds__(kLongThreads) objective_long_kernel(ObjectiveArgs a) {
  __shared__ double red[5 * (kLongThreads / 64)];
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x;
  const float* pr = a.daily + g * a.ds;
  const float* ob = a.obs + g * a.os;
  const bool live = !(a.drop && a.drop[g]);
  const int first = live ? a.wd : a.D;
  double s1[5] = {0, 0, 0, 0, 0};
  for (int i = first + tid; i < a.D; i += kLongThreads) pass1(pr[i], ob[i], s1);
  group_sum<kLongThreads>(s1, red, tid);
  double s2[3] = {0, 0, 0};
  if (a.kind >= DDR_OBJECTIVE_NSE) {
    const double mp = s1[1] / s1[0], mo = s1[2] / s1[0];
    for (int i = first + tid; i < a.D; i += kLongThreads) pass2(pr[i], ob[i], mp, mo, s2);
    group_sum<kLongThreads>(s2, red, tid);
  }
  if (tid == 0) gauge_finish(a, g, s1, s2);
}

constexpr int kReduceThreads = 1024;

// loss = sum num / W, W = sum den or the caller's count; W == 0 (nothing used): loss 0, and a zero gradient
__global__ void __launch_bounds__(kReduceThreads) objective_reduce_kernel(ObjectiveArgs a) {
  __shared__ double red[2 * (kReduceThreads / 64)];
  const int tid = threadIdx.x;
  double s[2] = {0, 0};
  for (int64_t g = tid; g < a.G; g += kReduceThreads) {
    s[0] += a.work[kNum * a.G + g];
    s[1] += a.work[kDen * a.G + g];
  }
  group_sum<kReduceThreads>(s, red, tid);
  if (tid == 0) {
    const double W = a.count_dev ? (double)a.count_dev[0] : (a.count > 0.0 ? a.count : s[1]);
    a.loss[0] = W == 0.0 ? 0.0f : (float)(s[0] / W);
    a.work[kWorkRows * a.G] = W;
  }
}

// a wave writes kObjectiveGradChunk days of one gauge: each element formed in fp64 and rounded once
__global__ void __launch_bounds__(64 * kObjectiveShortWaves) objective_grad_kernel(ObjectiveArgs a, int chunks) {
  const int tid = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kObjectiveShortWaves + (threadIdx.x >> 6);
  const int64_t g = wave / chunks;
  if (g >= a.G) return;
  const int c = (int)(wave - g * chunks);
  const int64_t G = a.G;
  const double W = a.work[kWorkRows * G];
  const bool used = a.work[kUsed * G + g] != 0.0 && !(W == 0.0);
  const double s = used ? a.work[kWgt * G + g] / W : 0.0;
  const double u0 = a.work[kU0 * G + g], u1 = a.work[kU1 * G + g], u2 = a.work[kU2 * G + g];
  const double mp = a.work[kMeanP * G + g], mo = a.work[kMeanO * G + g];
  const float* pr = a.daily + g * a.ds;
  const float* ob = a.obs + g * a.os;
  float* gr = a.grad + g * (int64_t)a.D;
  const int end = min(a.D, (c + 1) * kObjectiveGradChunk);
  for (int i = c * kObjectiveGradChunk + tid; i < end; i += 64) {
    float v = 0.0f;
    if (used && i >= a.wd) {
      const float of = ob[i];
      if (of == of) {
        const double p = (double)pr[i], o = (double)of;
        const double d = p - o;
        if (a.kind == DDR_OBJECTIVE_L1)
          v = (float)(d > 0.0 ? s : (d < 0.0 ? -s : (d != d ? d : 0.0)));
        else if (a.kind == DDR_OBJECTIVE_KGE)
          v = (float)(s * (u0 + u1 * (o - mo) + u2 * (p - mp)));
        else
          v = (float)(s * u2 * d);
      }
    }
    gr[i] = v;
  }
}

}  // namespace

size_t objective_work_bytes(int64_t G) { return sizeof(double) * ((size_t)kWorkRows * (size_t)G + 1); }

hipError_t launch_objective(const ObjectiveArgs& a, hipStream_t stream) {
  if (a.G == 0) return hipSuccess;
  const unsigned short_wgs = (unsigned)((a.G + kObjectiveShortWaves - 1) / kObjectiveShortWaves);
  if (a.D <= kObjectiveShortMaxDays)
    hipLaunchKernelGGL(objective_short_kernel, dim3(short_wgs), dim3(64 * kObjectiveShortWaves), 0, stream, a);
  else
    hipLaunchKernelGGL(objective_long_kernel, dim3((unsigned)a.G), dim3(kLongThreads), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(objective_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, stream, a);
  e = hipGetLastError();
  if (e != hipSuccess || !a.grad) return e;
  const int chunks = (a.D + kObjectiveGradChunk - 1) / kObjectiveGradChunk;
  const int64_t waves = a.G * chunks;  // <= 2^24 * 32
  hipLaunchKernelGGL(objective_grad_kernel, dim3((unsigned)((waves + kObjectiveShortWaves - 1) / kObjectiveShortWaves)),
                     dim3(64 * kObjectiveShortWaves), 0, stream, a, chunks);
  return hipGetLastError();
}

}  // namespace ddr
