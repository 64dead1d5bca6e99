// The fused forward routing kernel (all T steps in one persistent launch), the last-step outputs and
// their launch.  The schedule, the hand-offs and the shared device helpers: route_device.h.
#include "route_device.h"
#include "route_launch.h"

namespace ddr {

// ============================================================================================
// Forward
// ============================================================================================
// Tick structure (one LDS slot per reach, single-buffered):
//   [import a chunk of virtual inflows]  prefetch q' of the next tick
//   compute: every reach reads its upstream x_j(t) from the slots (written last tick), runs the
//            physics and the fp64 column sweep, keeps x in a register          -- barrier --
//   publish: x into the reach's own slot (and virtual inflows into theirs)      -- barrier --
// The inflow I(t+1) = sum_j Q_j(t) is formed from the same x_j(t) reads (Q_j = clamp(x_j)).
// FM (fp32 only, DDR_FWD_FAST_MATH): the coefficients in hardware-approximate fp32 math
// (coefficients_fast, the operation set of the adjoint's recompute) instead of the reference's exact
// operation sequence; ~1e-6 relative per coefficient, and few enough registers that all of a
// thread's slices run their physics in lockstep.
// MATH: 0 exact (reference op order, correctly rounded pow), 1 fast (DDR_FWD_FAST_MATH), 2 faithful
// (DDR_FWD_FAITHFUL_MATH: exact op order and IEEE divisions, fp32 faithful-class pow).
// XB: the x slots' buffer count when not the KR rule's (fwd_xbuf): 2 = parity-indexed slots and one barrier
// per tick at KR = 4 too, where the launch finds the LDS for them (launch_forward_kr)
// PL (plain): the launch has none of the rarely used options -- no split basin, no profile, no daily
// accumulation -- and 1: runoff written with 16-B rows, q' from the tick-major gather; 2: no runoff (gauge mode),
// tick-major q'; 4: no runoff, q' from the row layout (daily q', qs_rows); so their tests and the uniform values
// behind them (held in scalar registers, spilled at KR = 4) leave the tick loop (C5 forward -6 %, C4 -8 %,
// C2 -15 %: profiles/r05/ab_r05.txt item 11)
template <typename R, int KR, int MATH, int XB = 0, int PL = 0>
__global__ void __launch_bounds__(kBlockThreads, kBlocksPerCU * kBlockThreads / 256) route_forward_kernel(RouteArgs a) {
  constexpr int BS = kBlockThreads;
  constexpr bool kFast = MATH == 1 && std::is_same<R, float>::value;
  constexpr bool kFaith = MATH == 2 && std::is_same<R, float>::value;
  // one slice's physics at a time (lockstep slice pairs, plain or in packed halves, measured slower:
  // DESIGN section 4)
  constexpr int NP = 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int bid = take_ticket(a.status, kStatusTicketFwd, a.nblocks, false, reinterpret_cast<int*>(smem));
  if (a.owned && !a.owned[bid]) return;  // split basin: another rank's block
  const BlockDesc B = block_desc(a.s.blocks, bid);
  const int tid = threadIdx.x;
  // first lane of this wave (scalar): waves with no reach in slice k skip it (scalar branch),
  // so a workgroup's tick costs ceil(nloc / 64) wave-slices, not KR * waves
  const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63);
  const int S = a.slot_stride;
  // kDbl: [2][S] x slots by tick parity -- tick tau reads buffer (tau - 1) & 1 and writes its results
  // straight into buffer tau & 1, one workgroup barrier per tick; else [S], written in a publish phase
  // between two barriers
  constexpr int kXBuf = XB > 0 ? XB : fwd_xbuf(KR);
  constexpr bool kDbl = kXBuf == 2;
  const FwdLds<R> lds = fwd_lds<R>(smem, S, kXBuf);
  double* sx = lds.x;              // [kXBuf][S] x_j(t), solve precision
  const StatTab<R> tab{lds.stat};  // [S][6]
  double* ring = lds.ring;         // [nvirt][kChunkFwd]
  int* xl = reinterpret_cast<int*>(smem + a.xl_off);  // confluence lists
  const Consts<R> cs = consts_of<R>(a, !kFast && !kFaith, KR >= kOpqInfMinKR);
  const int64_t T = a.T;
  const bool carry = a.flags & DDR_FWD_CARRY;
  const bool accum = !PL && (a.flags & DDR_FWD_ACCUMULATE);  // every step a hot start (daily accumulation)
  auto* const aprof = PL ? nullptr : a.prof;  // per-block tick profile (--block-profile)
  const int32_t xt_off = PL ? 0 : a.xt_off;   // split basin: the export-row table
  const bool force_to = a.flags & kFlagForceTimeout;
  R* xsave = static_cast<R*>(a.x_save);
  const int TTf = (int)T + B.dmax;
  const R* q0p = static_cast<const R*>(a.q0);
  const int64_t xs_base = T * B.pos0 + B.pre_dn;

  // the schedule words of each reach (reach_words)
  int ref[KR], off[KR];
  unsigned up[KR];
  auto off_of = [&](int k) { return tick_off(off[k]); };
  R Q[KR], In[KR], qa[KR], qb[KR], ex[KR], inv[KR];  // ex, inv: the static divisions, kept in registers
  // one reach per thread (small blocks: light loads, where a tick is one dependency chain long): the
  // statics stay in registers, off the chain's LDS round trips
  constexpr bool kStatReg = KR == 1 && sizeof(R) == 4;
  ReachStatic<R> sreg[kStatReg ? KR : 1];
  // runoff (N, T) written from here: the last four steps of each reach, stored 16 B at a time
  R ob0[KR], ob1[KR], ob2[KR], ob3[KR];
  R* runoff = static_cast<R*>(a.runoff);
  const bool emit = PL == 1 || (PL == 0 && runoff != nullptr && !(a.flags & DDR_FWD_NO_RUNOFF));
  // rows 16-B aligned: vector stores (per-step 4-B stores measured 1.6x slower for the whole kernel)
  const bool emit4 = PL == 1 || (T & 3) == 0;
  // Storer waves (one reach per thread, blocks of at most half a workgroup): the idle upper half of the
  // workgroup stores each reach's published x (x_save row, runoff) during the next tick, so a compute
  // wave's top-of-tick wait covers only its q' prefetch -- not the acknowledgement of its stores, which
  // is on a light block's critical path (up to 12 % of a C2 tick, profiles/r03/ab_r03.txt item 5).
  // The storers export the cut reaches' granules too: a cut reach's x reaches its consumer one tick later
  // (pipeline latency of that hand-off only), and no compute wave waits for a store at all.
  // Imports requested a chunk ahead (KR <= 2: registers for the chunk's raw granules).
  constexpr bool kPrefImport = KR <= 2;
  unsigned long long pfg[kChunkFwd];
#pragma unroll
  for (int i = 0; i < kChunkFwd; ++i) pfg[i] = 0ull;
  const bool storer_mode = KR == 1 && !(a.flags & kFlagNoStorer) && B.nloc <= BS / 2;
  const bool storer_wave = storer_mode && wbase >= BS / 2;
  const int sr = tid - BS / 2;  // a storer thread's reach
  int sref = 0, soff = 0;  // its ref and off words
  if (storer_wave && sr < B.nloc) {
    const ReachWords w = reach_words(a.s, B, B.pos0 + sr, S);
    sref = w.ref;
    soff = w.off;
  }
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const int r = tid + k * BS;
    const bool hk = r < B.nloc;
    const int P = B.pos0 + (hk ? r : 0);
    const ReachWords w = reach_words(a.s, B, P, S);
    ref[k] = w.ref;
    off[k] = w.off;
    up[k] = w.up;
    Q[k] = In[k] = R(0);
    qa[k] = qb[k] = R(0);
    ob0[k] = ob1[k] = ob2[k] = ob3[k] = R(0);
    const ReachStatic<R> st = load_static<R>(a, ref[k]);
    ex[k] = st.expo;
    inv[k] = st.inv_n;
    if (hk) tab.put(r, st);
    if constexpr (kStatReg) sreg[k] = tab.get_pre(hk ? r : 0, st.expo, st.inv_n);  // the values the LDS path reads
  }
  if (tid == 0) sx[S - 1] = 0.0;
  if (kDbl && tid == 0) sx[2 * S - 1] = 0.0;
  // virtual inflow vi is imported and published by thread BS - 1 - vi (route_device.h, VirtOwner, says why
  // there).  Its own scalars and its own import and publish text, not VirtOwner's: with the four words in a
  // struct the KR = 4 instances change their scalar spills, one of them upwards
  const int vi = BS - 1 - tid;
  const bool vown = vi < B.nvirt;
  int v_off = 0, v_edge = 0;
  if (vown) {
    v_off = a.s.v_off[B.virt0 + vi];
    v_edge = a.s.v_edge[B.virt0 + vi];
  }
  load_math_tables();
  load_xlist(a.s, B, xl);
  uintptr_t* xt = reinterpret_cast<uintptr_t*>(smem + xt_off);  // split: cut-outs' export rows
  if (xt_off) {
    for (int c = tid; c < B.ncout; c += BS) {
      const int64_t e = B.cout0 + c;
      const int xi = a.xid[e];
      xt[c] = xi >= 0 ? (reinterpret_cast<uintptr_t>(a.pxfwd[a.xcons[xi]] + (int64_t)xi * T) | 1u)
                      : reinterpret_cast<uintptr_t>(a.bnd + e * T);
    }
  }
  __syncthreads();
  unsigned long long prof_wait = 0;
  if (aprof && tid == 0) prof_begin(aprof, bid);
  PhaseProf phz;
  phz.start();

  // q'[max(t-1,0)] * flow_scale (gathered into the schedule layout: one row per tick), or the
  // carried Q0 at t = 0, for the step each reach runs at tick `tau`
  const R* qsb = static_cast<const R*>(a.qs) + xs_base;
  const bool qs_rows = PL == 4 || (PL == 0 && a.qs_rows > 0);
  // kSt (steady ticks, below): no reach is at its carried t = 0 step
  auto prefetch = [&](int tau, R(&dst)[KR], int tq0, auto sc) {
    constexpr bool kSt = decltype(sc)::value;
    const R* row = qsb + (int64_t)(tau < TTf ? tau : TTf - 1) * B.nloc;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      if (wbase + k * BS >= B.nloc) continue;
      const int r = tq0 + k * BS;
      const int rs = r < B.nloc ? r : 0;
      const R v = qs_rows ? *qs_at<R>(a, B, xs_base, tau, off_of(k), rs) : row[rs];
      dst[k] = (!kSt && carry && tau == off_of(k)) ? q0p[ref[k]] : v;
    }
  };

  // sc: std::integral_constant<bool, kSt>.  Steady ticks (tau in [dmax + 1, T - 1]) are those at which
  // every reach of the block runs a step t in [1, T - 1]: no activity tests, no idle-slice ballot, no
  // hot start or carried-state case -- the same operations on the same values as the general tick
  // storer threads: the stores of the x their reach published at tick `taup` (read from its slot before
  // the next publish overwrites it); the same values and rounding as the compute waves' stores
  auto store_pass = [&](int taup) {
    if (sr >= B.nloc) return;
    const int so = opq(soff);
    const int t = taup - tick_off(so);
    if (t < 0 || t >= T) return;
    const double xd = sx[(kDbl ? (taup & 1) * S : 0) + sr];
    const R xr = R(xd);
    if (B.ncout > 0 && cut_rank(so)) {
      const int64_t e = B.cout0 + cut_rank(so) - 1;
      if (xt_off) {
        const uintptr_t p = xt[cut_rank(so) - 1];
        double* row = reinterpret_cast<double*>(p & ~uintptr_t(1));
        if (p & 1u) store_granule_sys(row + t, xd);
        else store_granule(row + t, xd);
      } else {
        store_granule(a.bnd + e * T + t, xd);
      }
    }
    static_cast<R*>(a.x_save)[xs_base + (int64_t)taup * B.nloc + sr] = xr;
    if (emit) {
      ob0[0] = ob1[0];
      ob1[0] = ob2[0];
      ob2[0] = ob3[0];
      ob3[0] = rmax_nan(xr, cs.qlb);
      R* orow = runoff + (int64_t)opq(sref) * T;
      if (!emit4) orow[t] = ob3[0];
      else if ((t & 3) == 3) store4(orow + (t - 3), ob0[0], ob1[0], ob2[0], ob3[0]);
    }
  };

  // the import of the next chunk of every virtual inflow, at ticks tau = 0 mod kChunkFwd (owners only)
  auto import_chunk = [&](int tau) {
    if (B.nvirt > 0 && (tau % kChunkFwd) == 0) {
      // import the next chunk of every virtual inflow (x of the upstream block's reach): its owner
      // thread requests the kChunkFwd granules at once
      const unsigned long long w0 = aprof ? __builtin_amdgcn_s_memrealtime() : 0;
      if (kPrefImport && vown) {
        // (light and medium loads) the chunk was requested one chunk ago: its granules have landed while
        // the block ran, so the import waits only for those still unpublished, and the next chunk is
        // requested now -- the owner's wave (and the barrier after it) no longer pays a memory round
        // trip every kChunkFwd ticks
        const int xi = (!PL && a.xid) ? a.xid[v_edge] : -1;  // split basin: another rank's block, receive rows
        const double* row = xi >= 0 ? a.xfwd + (int64_t)xi * T : a.bnd + (int64_t)v_edge * T;
        const int64_t t0 = (int64_t)tau - v_off;
        double g[kChunkFwd];
        if (xi >= 0) {
          if (tau == 0) issue_granules<kChunkFwd, true>(row, t0, 0, T, pfg);
          poll_granules<kChunkFwd, true>(row, t0, 0, T, pfg, g, a.status, bid, force_to);
          issue_granules<kChunkFwd, true>(row, t0 + kChunkFwd, 0, T, pfg);
        } else {
          if (tau == 0) issue_granules<kChunkFwd, false>(row, t0, 0, T, pfg);
          poll_granules<kChunkFwd, false>(row, t0, 0, T, pfg, g, a.status, bid, force_to);
          issue_granules<kChunkFwd, false>(row, t0 + kChunkFwd, 0, T, pfg);
        }
#pragma unroll
        for (int i = 0; i < kChunkFwd; ++i) ring[vi * kChunkFwd + i] = g[i];
      } else if (vown) {
        // split basin: a cut edge from another rank's block arrives in this rank's receive rows
        const int xi = (!PL && a.xid) ? a.xid[v_edge] : -1;
        if (xi >= 0) {
#pragma unroll
          for (int h = 0; h < kChunkFwd; h += kImportBatch) {
            double g[kImportBatch];
            wait_granules<kImportBatch, true>(a.xfwd + (int64_t)xi * T, (int64_t)tau - v_off + h, 0, T, g, a.status,
                                              bid, force_to);
#pragma unroll
            for (int i = 0; i < kImportBatch; ++i) ring[vi * kChunkFwd + h + i] = g[i];
          }
        } else {
#pragma unroll
          for (int h = 0; h < kChunkFwd; h += kImportBatch) {
            double g[kImportBatch];
            wait_granules<kImportBatch>(a.bnd + (int64_t)v_edge * T, (int64_t)tau - v_off + h, 0, T, g, a.status,
                                        bid, force_to);
#pragma unroll
            for (int i = 0; i < kImportBatch; ++i) ring[vi * kChunkFwd + h + i] = g[i];
          }
        }
      }
      if (aprof) prof_wait += __builtin_amdgcn_s_memrealtime() - w0;
    }
  };
  // a virtual inflow's value of tick tau into its slot of buffer `dst` (owners only)
  auto publish_virt = [&](int tau, double* dst) {
    if (vown) {
      const int t = tau - v_off;
      if (t >= 0 && t < T) dst[B.nloc + vi] = ring[vi * kChunkFwd + (tau % kChunkFwd)];
    }
  };

  // One tick of the waves that route reaches (every wave outside storer mode)
  auto tick = [&](int tau, R(&qcur)[KR], R(&qnext)[KR], auto sc) {
    constexpr bool kSt = decltype(sc)::value;
    // the previous tick's q' prefetch and stores land here (see the backward kernel's tick); unconditional,
    // so the compiler's own wait analysis sees no load outstanding past it (a wait it could not prove made
    // it wait again, vmcnt(0), at the first use of qcur -- after this tick's prefetch was issued)
    __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);
    if constexpr (KR == 4) set_prio(3);
    if constexpr (KR == 1) __builtin_amdgcn_s_setprio(1);
    phz.mark(0);  // the previous tick's loads and stores
    // opaque per tick: everything derived from them (LDS / global offsets, masks) is recomputed
    // instead of being hoisted into registers held across the loop
    const int tq = opq(tid);
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      ref[k] = opq(ref[k]);
      off[k] = opq(off[k]);
      up[k] = opq(up[k]);
      ex[k] = opq(ex[k]);
      inv[k] = opq(inv[k]);
    }
    import_chunk(tau);
    phz.mark(1);  // import
    prefetch(tau + 1, qnext, tq, sc);
    R* xrow = xsave + xs_base + (int64_t)tau * B.nloc;  // this tick's row of the state layout
    double xk[KR];
    const double* sxr = sx + (kDbl ? ((tau + 1) & 1) * S : 0);  // the slots published at tick tau - 1
    double* sxw = sx + (kDbl ? (tau & 1) * S : 0);              // (kDbl) this tick's results
    // ---- compute, NP slices at a time: their physics in lockstep (NP independent dependency
    //      chains per wave: the tick is latency-bound at 4 waves per SIMD), then per slice the
    //      fp64 column sweep and the stores -------------------------------------------------------
#pragma unroll
    for (int k0 = 0; k0 < KR; k0 += NP) {
      if (wbase + k0 * BS >= B.nloc) continue;
      if constexpr (KR == 4) set_prio(KR - 1 - k0);
      if (!kSt) {
        // no lane of the wave runs a step this tick (before its first / after its last step: the
        // first and last dmax ticks of a block, most ticks of a short window): skip the slice
        bool act = false;
#pragma unroll
        for (int h = 0; h < NP; ++h) {
          const int t = tau - off_of(k0 + h);
          act = act || (tq + (k0 + h) * BS < B.nloc && t >= 0 && t < T);
        }
        if (__builtin_amdgcn_ballot_w64(act) == 0) continue;
      }
      ReachStatic<R> st[NP];
      R Qv[NP];
      PhysOut<R> ph[NP];
      // the upstream slots first: they do not depend on the physics, so their LDS latency hides under it
      // (the second upstream's slot is the packed word's f1; a confluence's comes from its list below)
      double x0a[NP], x1a[NP];
#pragma unroll
      for (int h = 0; h < NP; ++h) {
        x0a[h] = sxr[up_0(up[k0 + h])];
        x1a[h] = sxr[up_n(up[k0 + h]) > 2 ? S - 1 : up_f1(up[k0 + h])];  // (a list offset is not a slot)
      }
#pragma unroll
      for (int h = 0; h < NP; ++h) {
        const int r = tq + (k0 + h) * BS;
        if constexpr (kStatReg) st[h] = sreg[k0 + h];
        else st[h] = tab.get_pre(r < B.nloc ? r : 0, ex[k0 + h], inv[k0 + h]);
        Qv[h] = Q[k0 + h];
      }
      if (!accum) {
        if constexpr (kFast) {
#pragma unroll
          for (int h = 0; h < NP; ++h) ph[h] = coefficients_fast(st[h], Qv[h], cs);
        } else if constexpr (kFaith) {
#pragma unroll
          for (int h = 0; h < NP; ++h) ph[h] = coefficients_faithful(st[h], Qv[h], cs);
        } else {
          coefficients_np<R, NP>(st, Qv, cs, ph);
        }
      } else {
#pragma unroll
        for (int h = 0; h < NP; ++h) ph[h] = PhysOut<R>{R(0), R(0), R(0), R(0), R(0), R(0)};
      }
      if constexpr (KR == 1) __builtin_amdgcn_s_setprio(0);
#pragma unroll
      for (int h = 0; h < NP; ++h) {
        const int k = k0 + h;
        const int r = tq + k * BS;
        const bool hk = r < B.nloc;
        const int t = tau - off_of(k);
        const int nup = up_n(up[k]);
        const R qv = qcur[k];  // q' * flow_scale (mmc.py:303-304), applied by the gather
        const R qc = rmaxc(qv, cs.qlb, cs);                                        // mmc.py:421-424
        const R b = ((ph[h].c2 * In[k]) + (ph[h].c3 * Q[k])) + (ph[h].c4 * qc);  // mmc.py:535-538
        const double x0v = x0a[h];
        double x1v = x1a[h];
        if (nup > 2) x1v = sxr[xl[up_f1(up[k]) + 1]];  // a confluence: its list [c, u1, ...]
        // Q_j(t) of the upstream reaches (mmc.py:557; the carried state at t = 0 is not clamped)
        const bool raw = !kSt && (t == 0 && carry);
        auto qf = [&](double x) -> R {
          const R xr = R(x);
          return raw ? xr : rmaxc(xr, cs.qlb, cs);
        };
        const double dc1 = (double)ph[h].c1;
        double acc = (double)b;                                         // utils.py:587-600 (fp64)
        acc = acc + dc1 * x0v;                                          // (+ 0 for a missing upstream)
        acc = acc + dc1 * x1v;
        double hot = 0.0;
        if constexpr (!kSt) {
          hot = (double)qv;                                             // mmc.py:25-66 (hot start)
          hot = hot + x0v;
          hot = hot + x1v;
        }
        R inn = R(0);                                                   // I(t+1) = N @ Q_t, ascending columns
        inn = inn + (nup > 0 ? qf(x0v) : R(0));
        inn = inn + (nup > 1 ? qf(x1v) : R(0));
        if (nup > 2) {
          const int* lst = xl + up_f1(up[k]);
          const int c = lst[0];
          for (int j = 2; j < c; ++j) {
            const double xj = sxr[lst[j]];
            acc = acc + dc1 * xj;
            if constexpr (!kSt) hot = hot + xj;
            inn = inn + qf(xj);
          }
        }
        const double x = kSt ? acc : ((t == 0 && carry) ? (double)qcur[k] : ((t == 0 || accum) ? hot : acc));
        xk[k] = x;
        if (kDbl && hk && (kSt || (t >= 0 && t < T))) sxw[r] = x;  // published: read at tick tau + 1
        if (hk && (kSt || (t >= 0 && t < T))) {
          const R xr = R(x);
          const R Qn = raw ? xr : rmax_nan(xr, cs.qlb);
          const bool own_st = !storer_mode;  // (storer mode: the upper waves store)
          if (own_st) xrow[r] = xr;  // the routing state for the adjoint
          if (emit && own_st) {
            // runoff[ref, t] = max(x(t), qlb)  (mmc.py:412 for t = 0, mmc.py:557 after every step)
            ob0[k] = ob1[k];
            ob1[k] = ob2[k];
            ob2[k] = ob3[k];
            ob3[k] = rmax_nan(xr, cs.qlb);
            R* orow = runoff + (int64_t)ref[k] * T;
            if (!emit4) orow[t] = ob3[k];
            else if ((t & 3) == 3) store4(orow + (t - 3), ob0[k], ob1[k], ob2[k], ob3[k]);
          }
          if (B.ncout > 0 && cut_rank(off[k]) && !storer_mode) {
            const int64_t e = B.cout0 + cut_rank(off[k]) - 1;
            if (xt_off) {  // split basin: the row from the block's table (another rank's: system scope)
              const uintptr_t p = xt[cut_rank(off[k]) - 1];
              double* row = reinterpret_cast<double*>(p & ~uintptr_t(1));
              if (p & 1u) store_granule_sys(row + t, x);
              else store_granule(row + t, x);
            } else {
              store_granule(a.bnd + e * T + t, x);
            }
          }
          // (the last step's Q, top width and side slope: route_last_kernel, from the saved states --
          // no rarely taken stores, and no pointers held across the tick loop for them)
          Q[k] = Qn;
          In[k] = inn;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (kDbl) {
      // the virtual inflows' values of this tick, beside the reaches' (owners only read their own ring)
      publish_virt(tau, sxw);
      phz.mark(2);  // prefetch issue + compute + publish
      lds_barrier();
      phz.mark(3);  // the tick's one barrier
      return;
    }
    phz.mark(2);  // prefetch issue + compute
    lds_barrier();
    phz.mark(3);  // barrier 1
    // ---- publish ------------------------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      if (wbase + k * BS >= B.nloc) continue;
      const int t = tau - off_of(k);
      const int r = tq + k * BS;
      if (r < B.nloc && (kSt || (t >= 0 && t < T))) sx[r] = xk[k];
    }
    publish_virt(tau, sx);
    phz.mark(4);  // publish
    lds_barrier();
    phz.mark(5);  // barrier 2
  };

  const int TT = (int)T + B.dmax;
  if constexpr (KR == 1) {
    if (storer_wave) {
      // Storer waves (storer mode: the upper half of the workgroup): their own loop -- the import of the
      // virtual inflows they own, the stores of the x their reach published a tick earlier, the virtuals'
      // publish and the tick's barriers -- so the routing waves' tick carries no storer branch
#pragma unroll 1
      for (int tau = 0; tau < TT; ++tau) {
        import_chunk(tau);
        if (tau > 0) store_pass(tau - 1);
        if constexpr (kDbl) {
          publish_virt(tau, sx + (tau & 1) * S);
          lds_barrier();
        } else {
          lds_barrier();
          publish_virt(tau, sx);
          lds_barrier();
        }
      }
      store_pass(TT - 1);  // the last tick's publish (its barrier has passed)
      return;
    }
  }
  using Gen = std::integral_constant<bool, false>;
  using Steady = std::integral_constant<bool, true>;
  prefetch(0, qa, tid, Gen{});
  // two ticks per iteration, the prefetch registers swapping roles: copying the prefetched q'
  // (qa = qb) at the loop latch would wait for the loads just issued, and for every store of the tick.
  // Steady ticks [s0, s1) (even bounds, so the roles keep alternating) between the ramps.
  int s0 = B.dmax + 1, s1 = (int)T & ~1;
  s0 += s0 & 1;
  if ((a.flags & kFlagNoSteady) || accum || s1 <= s0) s0 = s1 = 0;
#pragma unroll 1
  for (int tau = 0; tau < s0; tau += 2) {
    if (aprof && tid == 0) prof_tick(aprof, bid, tau);
    tick(tau, qa, qb, Gen{});
    tick(tau + 1, qb, qa, Gen{});
  }
#pragma unroll 1
  for (int tau = s0; tau < s1; tau += 2) {
    if (aprof && tid == 0) prof_tick(aprof, bid, tau);
    tick(tau, qa, qb, Steady{});
    tick(tau + 1, qb, qa, Steady{});
  }
#pragma unroll 1
  for (int tau = s1; tau < TT; tau += 2) {
    if (aprof && tid == 0) prof_tick(aprof, bid, tau);
    tick(tau, qa, qb, Gen{});
    if (tau + 1 < TT) tick(tau + 1, qb, qa, Gen{});
  }
  if (aprof && tid == 0) prof_end(aprof, bid, prof_wait);
  phz.flush(aprof, a.nblocks, bid);
}

// The forward's last-step outputs (mmc.py:441 _discharge_t, mmc.py:161-162 top_width / side_slope), from
// the saved states: Q(T - 1) = clamp(x(T - 1)), and the geometry of step T - 1, whose physics ran on
// Q(T - 2) -- the same operations on the same values as the routing kernel's, so the same bits.  One
// thread per internal position.
template <typename R, int MATH>
__global__ void __launch_bounds__(256) route_last_kernel(RouteArgs a) {
  load_math_tables();
  __syncthreads();
  const int64_t P = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (P >= a.N) return;
  const BlockDesc B = a.s.blocks[a.s.block_of_pos[P]];
  const int r = (int)(P - B.pos0);
  const int64_t off = a.s.off[P];
  const int ref = a.s.ref[P];
  const int64_t T = a.T;
  if (a.owned && !a.owned[a.s.block_of_pos[P]]) {  // split basin: another rank routes this reach
    const R nan = R(__builtin_nan(""));
    if (a.q_last) static_cast<R*>(a.q_last)[ref] = nan;
    if (a.tw_last) static_cast<R*>(a.tw_last)[ref] = nan;
    if (a.ss_last) static_cast<R*>(a.ss_last)[ref] = nan;
    return;
  }
  const R* xs = static_cast<const R*>(a.x_save) + T * B.pos0 + B.pre_dn;
  const bool carry = a.flags & DDR_FWD_CARRY;
  const bool accum = a.flags & DDR_FWD_ACCUMULATE;
  const Consts<R> cs = consts_of<R>(a, false);
  auto Q_at = [&](int64_t t) {  // Q(t): the carried state at t = 0 is not clamped
    const R x = xs[(t + off) * B.nloc + r];
    return (t == 0 && carry) ? x : rmax_nan(x, cs.qlb);
  };
  if (a.q_last) static_cast<R*>(a.q_last)[ref] = Q_at(T - 1);
  if (T > 1 && !accum && (a.tw_last || a.ss_last)) {
    const ReachStatic<R> st = load_static<R>(a, ref);
    const R Qv = Q_at(T - 2);
    PhysOut<R> ph;
    constexpr bool kFast = MATH == 1 && std::is_same<R, float>::value;
    constexpr bool kFaith = MATH == 2 && std::is_same<R, float>::value;
    if constexpr (kFast) {
      ph = coefficients_fast(st, Qv, cs);
    } else if constexpr (kFaith) {
      ph = coefficients_faithful(st, Qv, cs);
    } else {
      ReachStatic<R> sa[1] = {st};
      R qa[1] = {Qv};
      PhysOut<R> pa[1];
      coefficients_np<R, 1>(sa, qa, cs, pa);
      ph = pa[0];
    }
    if (a.tw_last) static_cast<R*>(a.tw_last)[ref] = ph.tw;
    if (a.ss_last) static_cast<R*>(a.ss_last)[ref] = ph.ss;
  }
}

// the faithful forward instance for a plain code (route_forward_kernel's PL; 0: the general one)
template <typename R, int KR, int XB>
auto forward_faithful_of(int pl) {
  switch (pl) {
    case 1: return route_forward_kernel<R, KR, 2, XB, 1>;
    case 2: return route_forward_kernel<R, KR, 2, XB, 2>;
    case 4: return route_forward_kernel<R, KR, 2, XB, 4>;
    default: return route_forward_kernel<R, KR, 2, XB>;
  }
}

template <typename R, int KR>
hipError_t launch_forward_kr(const Graph* g, RouteArgs a, hipStream_t stream) {
  RouteLds lds = route_lds_plan<R>(g, false, 0);
  const dim3 grid((unsigned)g->blocks.size()), block(kBlockThreads);
  auto kern = route_forward_kernel<R, KR, 0>;
  if constexpr (std::is_same<R, float>::value) {
    // the plain instance (route_forward_kernel's PL) this launch can take: 0 none, 1 runoff rows, 2 none written
    const bool plain_ok = !(a.flags & kFlagNoPlain);
    const bool rows = a.runoff != nullptr && !(a.flags & DDR_FWD_NO_RUNOFF);
    int plain = 0;
    if (plain_ok && g->split.nranks == 0 && a.prof == nullptr && !(a.flags & DDR_FWD_ACCUMULATE)) {
      if (rows) plain = ((a.T & 3) == 0 && a.qs_rows <= 0) ? 1 : 0;
      else plain = a.qs_rows > 0 ? 4 : 2;
    }
    if (a.flags & DDR_FWD_FAST_MATH) kern = route_forward_kernel<R, KR, 1>;
    else if (a.flags & DDR_FWD_FAITHFUL_MATH) kern = forward_faithful_of<R, KR, 0>(plain);
    // KR = 4 (faithful): double-buffered x slots -- one barrier per tick -- where this graph's largest
    // block leaves the LDS for a second buffer (C5's blocks of <= ~3800 reaches; C3's 4096 do not)
    if constexpr (KR == 4) {
      const RouteLds lds2 = route_lds_plan<R>(g, false, 2);
      if ((a.flags & DDR_FWD_FAITHFUL_MATH) && lds2.smem <= kLdsBudget) {
        kern = forward_faithful_of<R, KR, 2>(plain);
        lds = lds2;
      }
    }
  }
  set_launch_args(a, g, lds);
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds.smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, grid, block, lds.smem, stream, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.q_last || a.tw_last || a.ss_last) {
    auto last = route_last_kernel<R, 0>;
    if constexpr (std::is_same<R, float>::value) {
      if (a.flags & DDR_FWD_FAST_MATH) last = route_last_kernel<R, 1>;
      else if (a.flags & DDR_FWD_FAITHFUL_MATH) last = route_last_kernel<R, 2>;
    }
    hipLaunchKernelGGL(last, dim3((unsigned)((g->n + 255) / 256)), dim3(256), kMathTabBytes, stream, a);
  }
  return hipGetLastError();
}

template <typename R>
hipError_t launch_route_forward(const Graph* g, const RouteArgs& a, hipStream_t stream) {
  return dispatch_kr(g, [&](auto kr) { return launch_forward_kr<R, decltype(kr)::value>(g, a, stream); });
}

template <typename R>
int forward_resident_blocks(const Graph* g) {
  const void* f = dispatch_kr(g, [](auto kr) { return (const void*)route_forward_kernel<R, decltype(kr)::value, 0>; });
  return resident_blocks(g, f, route_lds_plan<R>(g, false, 0).smem);
}

template hipError_t launch_route_forward<float>(const Graph*, const RouteArgs&, hipStream_t);
template hipError_t launch_route_forward<double>(const Graph*, const RouteArgs&, hipStream_t);
template int forward_resident_blocks<float>(const Graph*);
template int forward_resident_blocks<double>(const Graph*);

}  // namespace ddr
