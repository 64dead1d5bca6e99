// Linear Muskingum routing, RAPID's matrix scheme, on the Muskingum-Cunge forward's schedule: per-reach
// constant (k, x), the same sparse lower-triangular solve per sub-step, no physics.  One persistent launch
// routes all F * S sub-steps.  Shared with that forward, from route_device.h, internal.h and route_launch.h:
// the schedule and its per-reach words, the LDS layout, the virtual-inflow owner and its bounded waits, the
// launch plan.  Its own: the tick below (one general tick, no physics) and the interval outputs.
//
// Per reach, in the routed precision R, separately rounded operations (no contraction):
//   h = dt / 2, den = k (1 - x) + h, C1 = (h - k x) / den, C2 = (h + k x) / den, C3 = (k (1 - x) - h) / den
//   In+ = sum_j Q+_j                 (the upstream list's order, from the first)
//   Q+  = (C1 (In+ + qe) + C2 (In + qe)) + C3 Q
// No clamps: a negative C1 (dt < 2 k x) and negative discharge are RAPID's.
//
// A reach holds TS = F * S + 1 states: step 0 is the initial state (zeros, q0, or the steady state of
// forcing row 0, the hot start's fp64 sweep), step t >= 1 is sub-step t - 1 of interval (t - 1) / S.
// Reach i runs step t at tick t + off(i); its upstream reaches ran the same step one tick earlier, so the
// slots it reads hold their Q+ -- the implicit term -- and its own In register their Q.
#include "route_linear.h"

#include "route_device.h"
#include "route_launch.h"

namespace ddr {

template <typename R, int KR>
__global__ void __launch_bounds__(kBlockThreads, kBlocksPerCU * kBlockThreads / 256) route_linear_kernel(LinArgs a) {
  constexpr int BS = kBlockThreads;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int bid = take_ticket(a.status, kStatusTicketFwd, a.nblocks, false, reinterpret_cast<int*>(smem));
  const BlockDesc B = block_desc(a.s.blocks, bid);
  const int tid = threadIdx.x;
  const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63);
  const int S = a.slot_stride;
  // the forward's LDS layout (fwd_lds; x slots by tick parity at KR <= 2: one barrier per tick); the statics
  // region holds the coefficient table [S][kLinCoefs] = C1, C2, C3, 0
  constexpr int kXBuf = fwd_xbuf(KR);
  constexpr bool kDbl = kXBuf == 2;
  const FwdLds<R> lds = fwd_lds<R>(smem, S, kXBuf);
  double* sx = lds.x;
  R* ctab = lds.stat;
  double* ring = lds.ring;
  int* xl = reinterpret_cast<int*>(smem + a.xl_off);
  const int TS = a.TS;
  const int sub1 = a.S - 1;
  const int64_t F = a.F;
  const bool end = a.flags & DDR_LIN_END;
  const bool steady = a.flags & DDR_LIN_STEADY;
  const bool force_to = a.flags & kFlagForceTimeout;
  const R* q0p = static_cast<const R*>(a.q0);
  const R* qsb = static_cast<const R*>(a.qs) + F * B.pos0;  // the block's gathered forcing, [F][nloc]
  R* out = static_cast<R*>(a.out);
  R* qlast = static_cast<R*>(a.q_last);
  const double dsub = (double)a.S;

  // the schedule words of each reach (reach_words)
  int ref[KR], off[KR];
  unsigned up[KR];
  auto off_of = [&](int k) { return tick_off(off[k]); };
  // per-tick state: Q, the previous sub-step's upstream sum, the interval's fp64 sum; the forcing row of the
  // current step and the sub-step within it (advanced without a division)
  R Q[KR], In[KR], qa[KR], qb[KR];
  double acc[KR];
  int fr[KR], ph[KR];
  // fp32 rows of a multiple of four intervals are 16-B aligned: a reach keeps its last three values and
  // stores four at a time (per-interval 4-B stores: the whole call 1.6x slower at S = 1; fp64 has not the
  // registers at four reaches per thread)
  constexpr bool kRow4 = sizeof(R) == 4;
  const bool emit4 = kRow4 && (a.F & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
  R ob0[KR], ob1[KR], ob2[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const int r = tid + k * BS;
    const bool hk = r < B.nloc;
    const int P = B.pos0 + (hk ? r : 0);
    const ReachWords w = reach_words(a.s, B, P, S);
    ref[k] = w.ref;
    off[k] = w.off;
    up[k] = w.up;
    Q[k] = In[k] = qa[k] = qb[k] = R(0);
    acc[k] = 0.0;
    fr[k] = ph[k] = 0;
    ob0[k] = ob1[k] = ob2[k] = R(0);
    if (hk) {
      const R kk = static_cast<const R*>(a.k)[ref[k]], xx = static_cast<const R*>(a.x)[ref[k]];
      const R h = R(a.dt) / R(2);
      const R kx = kk * xx;
      const R k1 = kk * (R(1) - xx);
      const R den = k1 + h;
      R* c = ctab + kLinCoefs * r;
      c[0] = (h - kx) / den;
      c[1] = (h + kx) / den;
      c[2] = (k1 - h) / den;
      c[3] = R(0);
    }
  }
  if (tid == 0) sx[S - 1] = 0.0;
  if (kDbl && tid == 0) sx[2 * S - 1] = 0.0;
  const VirtOwner vo(a.s, B);
  load_xlist(a.s, B, xl);
  __syncthreads();

  // the forcing of the step each reach runs at tick `tau` (the gathered row of its interval; the carried
  // state at step 0), requested a tick ahead: fr / ph are those of tick tau - 1
  auto prefetch = [&](int tau, R(&dst)[KR], int tq0) {
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      if (wbase + k * BS >= B.nloc) continue;
      const int r = tq0 + k * BS;
      const int rs = r < B.nloc ? r : 0;
      const int t = tau - off_of(k);
      int row = fr[k] + ((t >= 2 && ph[k] == sub1) ? 1 : 0);
      row = row < (int)F ? row : (int)F - 1;
      const R v = qsb[(int64_t)row * B.nloc + rs];
      dst[k] = (q0p && t == 0) ? q0p[ref[k]] : v;
    }
  };

  // the next chunk of every virtual inflow (x of the upstream block's reach), at ticks 0 mod kChunkFwd
  auto import_chunk = [&](int tau) {
    if (B.nvirt > 0 && (tau % kChunkFwd) == 0 && vo.own)
      vo.import_chunk<false>(a.bnd + (int64_t)vo.v_edge * TS, TS, tau, ring, a.status, bid, force_to);
  };
  auto publish_virt = [&](int tau, double* dst) { vo.publish(tau, TS, ring, dst, B.nloc); };

  auto tick = [&](int tau, R(&qcur)[KR], R(&qnext)[KR]) {
    // the previous tick's prefetch and stores land here (as the forward's tick)
    __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);
    const int tq = opq(tid);
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      ref[k] = opq(ref[k]);
      off[k] = opq(off[k]);
      up[k] = opq(up[k]);
    }
    import_chunk(tau);
    prefetch(tau + 1, qnext, tq);
    double xk[KR];
    const double* sxr = sx + (kDbl ? ((tau + 1) & 1) * S : 0);  // the slots published at tick tau - 1
    double* sxw = sx + (kDbl ? (tau & 1) * S : 0);
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      xk[k] = 0.0;
      if (wbase + k * BS >= B.nloc) continue;
      const int r = tq + k * BS;
      const bool hk = r < B.nloc;
      const int t = tau - off_of(k);
      const bool act = hk && t >= 0 && t < TS;
      if (__builtin_amdgcn_ballot_w64(act) == 0) continue;
      const int nup = up_n(up[k]);
      const double x0v = sxr[up_0(up[k])];
      double x1v = sxr[nup > 2 ? S - 1 : up_f1(up[k])];  // (a list offset is not a slot)
      if (nup > 2) x1v = sxr[xl[up_f1(up[k]) + 1]];
      const R qe = qcur[k];
      // In+ = sum_j Q+_j in R, list order; hot: the steady state's fp64 sweep (step 0)
      R inn = R(0);
      inn = inn + (nup > 0 ? R(x0v) : R(0));
      inn = inn + (nup > 1 ? R(x1v) : R(0));
      double hot = (double)qe;
      hot = hot + x0v;
      hot = hot + x1v;
      if (nup > 2) {
        const int* lst = xl + up_f1(up[k]);
        const int c = lst[0];
        for (int j = 2; j < c; ++j) {
          const double xj = sxr[lst[j]];
          inn = inn + R(xj);
          hot = hot + xj;
        }
      }
      const R* c = ctab + kLinCoefs * (hk ? r : 0);
      const R c1 = c[0], c2 = c[1], c3 = c[2];
      const R Qr = ((c1 * (inn + qe)) + (c2 * (In[k] + qe))) + (c3 * Q[k]);
      // step 0: the initial state (qcur holds q0 there when one is given)
      const double x0 = steady ? hot : (q0p ? (double)qe : 0.0);
      const double x = t == 0 ? x0 : (double)Qr;
      const R Qn = R(x);
      xk[k] = x;
      if (kDbl && act) sxw[r] = x;  // published: read at tick tau + 1
      if (act) {
        if (t > 0) {
          acc[k] = acc[k] + (double)Q[k];  // the state at the beginning of the sub-step
          if (ph[k] == sub1) {
            const R v = end ? Qn : R(acc[k] / dsub);
            R* orow = out + (int64_t)ref[k] * F;
            if constexpr (kRow4) {
              if (!emit4) orow[fr[k]] = v;
              else if ((fr[k] & 3) == 3) store4(orow + (fr[k] - 3), ob0[k], ob1[k], ob2[k], v);
              ob0[k] = ob1[k];
              ob1[k] = ob2[k];
              ob2[k] = v;
            } else {
              orow[fr[k]] = v;
            }
            acc[k] = 0.0;
          }
          if (t == TS - 1) qlast[ref[k]] = Qn;
          // the next step's interval and sub-step
          const bool wrap = ph[k] == sub1;
          ph[k] = wrap ? 0 : ph[k] + 1;
          fr[k] = fr[k] + (wrap ? 1 : 0);
        }
        if (B.ncout > 0 && cut_rank(off[k])) {
          const int64_t e = B.cout0 + cut_rank(off[k]) - 1;
          store_granule(a.bnd + e * TS + t, x);
        }
        Q[k] = Qn;
        In[k] = inn;
      }
    }
    if constexpr (kDbl) {
      publish_virt(tau, sxw);
      lds_barrier();
      return;
    }
    lds_barrier();
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      if (wbase + k * BS >= B.nloc) continue;
      const int t = tau - off_of(k);
      const int r = tq + k * BS;
      if (r < B.nloc && t >= 0 && t < TS) sx[r] = xk[k];
    }
    publish_virt(tau, sx);
    lds_barrier();
  };

  const int TT = TS + B.dmax;
  prefetch(0, qa, tid);
  // two ticks per iteration, the prefetch registers swapping roles (as the forward)
#pragma unroll 1
  for (int tau = 0; tau < TT; tau += 2) {
    tick(tau, qa, qb);
    if (tau + 1 < TT) tick(tau + 1, qb, qa);
  }
}

// Gauge rows of the (N, F) output: the member reaches' rows added in list order, in R
template <typename R>
__global__ void linear_gauge_kernel(int64_t G, int64_t F, const int64_t* goff, const int64_t* gidx, const R* nf,
                                    R* out) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= G * F) return;
  const int64_t g = w / F, f = w % F;
  R acc = R(0);
  for (int64_t k = goff[g]; k < goff[g + 1]; ++k) acc = acc + nf[gidx[k] * F + f];
  out[w] = acc;
}

template <typename R, int KR>
static hipError_t launch_linear_kr(const Graph* g, LinArgs a, hipStream_t stream) {
  const RouteLds lds = route_lds_plan<R>(g, false, 0);
  set_schedule_args(a, g, lds);
  auto kern = route_linear_kernel<R, KR>;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds.smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)g->blocks.size()), dim3(kBlockThreads), lds.smem, stream, a);
  return hipGetLastError();
}

template <typename R>
hipError_t launch_route_linear(const Graph* g, LinArgs a, hipStream_t stream) {
  return dispatch_kr(g, [&](auto kr) { return launch_linear_kr<R, decltype(kr)::value>(g, a, stream); });
}

template <typename R>
int linear_resident_blocks(const Graph* g) {
  const void* f = dispatch_kr(g, [](auto kr) { return (const void*)route_linear_kernel<R, decltype(kr)::value>; });
  return resident_blocks(g, f, route_lds_plan<R>(g, false, 0).smem);
}

template <typename R>
hipError_t launch_linear_gauge(int64_t G, int64_t F, const int64_t* goff, const int64_t* gidx, const R* nf, R* out,
                               hipStream_t stream) {
  const int64_t total = G * F;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(linear_gauge_kernel<R>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, G, F, goff,
                     gidx, nf, out);
  return hipGetLastError();
}

template hipError_t launch_route_linear<float>(const Graph*, LinArgs, hipStream_t);
template hipError_t launch_route_linear<double>(const Graph*, LinArgs, hipStream_t);
template int linear_resident_blocks<float>(const Graph*);
template int linear_resident_blocks<double>(const Graph*);
template hipError_t launch_linear_gauge<float>(int64_t, int64_t, const int64_t*, const int64_t*, const float*, float*,
                                               hipStream_t);
template hipError_t launch_linear_gauge<double>(int64_t, int64_t, const int64_t*, const int64_t*, const double*, double*,
                                                hipStream_t);

}  // namespace ddr
