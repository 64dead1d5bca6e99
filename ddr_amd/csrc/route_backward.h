// The fused adjoint routing kernel (reverse time, reverse topology, one persistent launch), the final
// gradient conversion and their launch.  The schedule, the hand-offs and the shared device helpers:
// route_device.h.  Compiled once per precision (route_backward_f32.hip, route_backward_f64.hip): the
// backward's instances are the longest compile of the library, and the two halves build side by side.
#pragma once

#include "route_device.h"
#include "route_launch.h"

namespace ddr {

// Tuning constants (each chosen by an A/B on MI355X; the rejected alternatives live in git history and
// profiles/r0*/ab_*.txt, not here):
// The backward's early loads (the next tick's x(t - 3) and virtual x requested at the top of the tick into a
// second register set) and its double-buffered slots at KR <= 2; KR = 4 has no registers for the second set
constexpr int kBwdEarlyMaxKR = 2;
// The backward's dL/drunoff groups as shift registers at KR <= 2 (c3s8 backward -4 %); at KR = 4 a select on
// t & 3 as two bit tests and three selects (C5 backward 59.5 vs 57.3 ms, profiles/r05/ab_r05.txt)
constexpr int kBwdShiftMaxKR = 2;
// Import waves: a chunk's cut-out granules requested this many ticks before its boundary tick
constexpr int kBwdImpEarly = 4;
// x / gradient helpers: their loads issued this many ticks ahead
constexpr int kBwdHelpAhead = 3;

// one reach-step's adjoint outputs: coefficients, dL/dQ_{t-1} and the parameter gradient terms
template <typename R>
struct AdjOutR {
  R c1, c2, c3, c4, gQ, gn, gq, gp;
};

template <typename R>
struct Grad4 {
  R a, b, c, d;
};
template <typename R>
__device__ __forceinline__ Grad4<R> make_grad4(R a, R b, R c, R d) { return Grad4<R>{a, b, c, d}; }

// ============================================================================================
// Backward (adjoint)
// ============================================================================================
// Reverse ticks (backward tick tb runs forward tick tau = TT - 1 - tb: reach i at step
// t = tau - off(i), its upstream reaches at t + 1, its downstream at t - 1); per tick:
//   [import a chunk of (c1 gb, c2 gb) from downstream blocks]
//   read:    publish x(t - 2) of every reach (and of every virtual inflow, from the forward's
//            boundary granules) into its slot; read the downstream reach's (c1_d gb_d, c2_d gb_d)
//            from its slot (or the ring); export the consumers' values of virtual inflows to the
//            upstream blocks                                                          -- barrier --
//   compute: from the upstream slots x_j(t - 1): the inflow I(t) of this step and the upstream sum
//            Sx(t - 1) of the next one (Sx(t) was formed last tick); VJP of one step; own slot
//            <- (c1 gb, c2 gb)                                                         -- barrier --
// Every global load of a tick is issued one tick (own states: two ticks) before its use: the
// states x(t - 3) (the schedule layout, coalesced rows), the virtual inflows' x, and dL/drunoff read
// straight from the API's (N, T) layout in 16-B groups of four steps (gauge mode: summed over the
// reach's gauges from (G, T)).
// GS (state gradients, DDR_BWD_GRAD_*): the sweep also runs step 0 -- the hot start's transposed solve
// (c1 = 1) into dL/d(q' * flow_scale)[0], or dL/dQ0 of a carried state -- and writes dL/d(q' * flow_scale)
// of every step (gb c4 [q' >= q_lb], mmc.py:421-424, 535-538) into gqs, the schedule layout of qs.
// XB: the slot buffers when not the KR rule's (bwd_xbuf): 1 = single-buffered slots where the double buffer
// does not fit the LDS (fp64 at KR = 2, bwd_xb_of)
// PL (plain, as the forward's): no split basin, no profile, no state seeds, 16-B (N, T) rows; 1: dL/drunoff per
// reach, 2: gauge mode -- the tests of those options and the uniform values behind them leave the tick loop
template <typename R, int KR, bool GS, int XB = 0, bool DF = false, int PL = 0>
__global__ void __launch_bounds__(kBlockThreads, kBlocksPerCU * kBlockThreads / 256) route_backward_kernel(RouteArgs a) {
  constexpr int BS = kBlockThreads;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int bid = take_ticket(a.status, kStatusTicketBwd, a.nblocks, true, reinterpret_cast<int*>(smem));
  if (a.owned && !a.owned[bid]) return;  // split basin: another rank's block
  const BlockDesc B = block_desc(a.s.blocks, bid);
  const int tid = threadIdx.x;
  // first lane of this wave (scalar): waves with no reach in slice k skip it (scalar branch),
  // so a workgroup's tick costs ceil(nloc / 64) wave-slices, not KR * waves
  const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63);
  const int S = a.slot_stride;
  // kDbl (KR <= 2): each slot array is [2][S] by tick parity -- a tick reads what its neighbours wrote the
  // tick before (the downstream's (c1 gb, c2 gb) in buffer (tb + 1) & 1, the upstream's x in buffer tb & 1)
  // and writes its own for the next tick into the other buffers: one workgroup barrier per tick.  Else
  // [S] each, a publish phase and a compute phase between two barriers.
  constexpr int kXB = XB > 0 ? XB : bwd_xbuf(KR);
  constexpr bool kDbl = kXB == 2 && KR <= kBwdEarlyMaxKR;
  const BwdLds<R> lds = bwd_lds<R>(smem, S, kXB);
  R* sa = lds.a;  // [kXB][S] c1_i gb_i (transposed solve, rounded to R)
  R* sb = lds.b;  // [kXB][S] c2_i gb_i (adjoint of the inflow)
  R* sx = lds.x;  // [kXB][S] x(t - 2) of each reach / virtual inflow; [S-1] = 0
  const StatTab<R> tab{lds.stat};  // [S][6]
  R* ring = lds.ring;              // [ncout][kChunkBwd][2]
  int* xl = reinterpret_cast<int*>(smem + a.xl_off);  // confluence lists
  const Consts<R> cs = consts_of<R>(a, true, KR >= kOpqInfMinKR);
  const int64_t T = a.T;
  const bool carry = a.flags & DDR_FWD_CARRY;
  const bool force_to = a.flags & kFlagForceTimeout;
  const R* xsave = static_cast<const R*>(a.x_save);
  const R* gout = static_cast<const R*>(a.grad_out);
  const int64_t xs_base = T * B.pos0 + B.pre_dn;
  double* gacc = a.bwd_bnd + 2 * a.n_cut * T;  // (N, 3) fp64 gradient accumulators (zeroed)
  const bool vec4 = PL || (T & 3) == 0;         // (N, T) rows 16-B aligned
  // (expressions at each use, not locals: the general instance then keeps the code and registers it had
  // before the plain ones existed -- locals held across the tick loop spill at KR = 4)
#define gauge (PL == 2 || (PL == 0 && a.g_roff != nullptr))  // dL/dout per gauge (G, T)
#define gseed (PL ? nullptr : a.gseed)                        // state seeds of steps T - 1, T - 2
#define aprof (PL ? nullptr : a.prof)
#define xt_off (PL ? 0 : a.xt_off)
  const int tmin = GS ? 0 : 1;                  // first step of the sweep (step 0: the hot start / Q0)
  R* gqs = static_cast<R*>(a.gqs);

  // od packs the tick offset (bits 16-30), dl (low 16, signed): local downstream (>= 0),
  // -(import slot + 2), or -1, and bit 31: the reach has no dL/drunoff row (gauge mode, ungauged
  // reach: its gradient loads, a dependent chain through the gauge map, are skipped)
  int ref[KR];
  unsigned od[KR];
  auto off_of = [&](int k) { return (int)((od[k] >> 16) & 0x7FFFu); };
  auto has_grad = [&](int k) { return (od[k] >> 31) == 0u; };
  auto dl_of = [&](int k) { return (int)(short)(od[k] & 0xFFFFu); };
  unsigned up[KR];
  // xc = x(t), xa = x(t-1), xb = x(t-2) (published this tick, then reloaded with x(t-3), while
  // x(t-2) stays readable in the reach's own slot); sxn = sum_j x_j(t) (upstream);
  // g0..g3: dL/drunoff of the four steps of t's group (t & ~3 .. t | 3)
  R lam[KR], xc[KR], xa[KR], xb[KR], pn[KR], pq[KR], pp[KR], g0[KR], g1[KR], g2[KR], g3[KR];
  // kDF (DDR_BWD_EXACT_ADJOINT, fp32 fast adjoint): the step's mass imbalances D1 = Q - qc - Sx, D2 = Q - qc - I
  // formed in fp64 from the fp32 states (physics.h adjoint_step_fast): the upstream sums carried in fp64, qc
  // re-read.  Else X (I - Sx) + (1 - X)(Q - x~) with x~ := x(t), the stored state
  constexpr bool kDF = DF && std::is_same<R, float>::value;
  using SxT = typename std::conditional<kDF, double, R>::type;
  SxT sxn[KR];
  // the gradient groups as shift registers (KR <= 2: c3s8 backward -4 %); at KR = 4 the select on t & 3 measured
  // faster (C5 backward 59.5 vs 57.3 ms, profiles/r05/ab_r05.txt)
  constexpr bool kShiftG = KR <= kBwdShiftMaxKR;
  // early loads: the next tick's x(t - 3) and virtual x are requested at the top
  // of the tick into a second register set (roles swap every tick: the loop is unrolled by two), so
  // they have the whole tick to land instead of the part after the first barrier
  R xb2[KR];
  constexpr bool kEarly = KR <= kBwdEarlyMaxKR;
  // gauge mode, KR <= 2: each reach's gauge when it has exactly one (else -1: none, or several -- the
  // reach -> gauge list is walked), so the tick's dL/dout loads are one address computation, not a chain of
  // three dependent loads each followed by a wait
  constexpr bool kGReg = KR <= 2;
  int gsg[kGReg ? KR : 1];
  constexpr bool kQs = GS || kDF;
  R qsv[kQs ? KR : 1];  // q' * flow_scale of this tick's step (prefetched a tick ahead): state gradients, kDF
  // one reach per thread: the derived statics stay in registers (see the forward)
  constexpr bool kStatReg = KR == 1 && sizeof(R) == 4;
  ReachStatic<R> sreg[kStatReg ? KR : 1];
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const int r = tid + k * BS;
    const bool hk = r < B.nloc;
    const int P = B.pos0 + (hk ? r : 0);
    ref[k] = a.s.ref[P];
    const bool nograd = gauge && a.g_roff[ref[k] + 1] == a.g_roff[ref[k]] && gseed == nullptr;
    if constexpr (kGReg) {
      gsg[k] = -1;
      if (gauge && a.g_roff[ref[k] + 1] - a.g_roff[ref[k]] == 1) gsg[k] = (int)a.g_rg[a.g_roff[ref[k]]];
    }
    od[k] = ((unsigned)a.s.off[P] << 16) | ((unsigned)a.s.dloc[P] & 0xFFFFu) | (nograd ? 0x80000000u : 0u);
    up[k] = pack_up(a.s, P, (unsigned)(S - 1));  // slot S-1 holds 0: missing upstreams add exactly 0
    lam[k] = R(0);
    sxn[k] = SxT(0);
    xc[k] = xa[k] = xb[k] = R(0);
    pn[k] = pq[k] = pp[k] = R(0);
    g0[k] = g1[k] = g2[k] = g3[k] = R(0);
    if (hk) tab.put(r, load_static<R>(a, ref[k]));
    if constexpr (kStatReg) {
      const ReachStatic<R> ls = load_static<R>(a, ref[k]);
      // the LDS path derives the same fields with the same operations each tick (StatTab::get)
      sreg[k] = derive_static<R, true>(ls.n, ls.qe, ls.p, ls.sqrtS, ls.L, ls.X);
    }
  }
  for (int c = 0; c < B.ncout; ++c) {
    const int loc = a.s.cout_loc[B.cout0 + c];
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (tid + k * BS == loc) od[k] = (od[k] & 0xFFFF0000u) | ((unsigned)(-(c + 2)) & 0xFFFFu);
  }
  if (tid == 0) sx[S - 1] = R(0);
  if (kDbl && tid == 0) sx[2 * S - 1] = R(0);
  const bool vown = tid < B.nvirt;
  // Import waves (KR = 1, blocks whose reaches, virtuals and chunk imports each fit half the workgroup):
  // the upper half's idle waves run the cut-out imports in a loop of their own, requesting each chunk's
  // granules kBwdImpEarly ticks before its boundary tick, so the routing waves' import phase shrinks
  // to the barrier that hands the ring over
  static_assert(kBwdImpEarly > 0 && kBwdImpEarly < kChunkBwd, "import lead within a chunk");
  const bool help_ok = KR == 1 && kDbl && !(a.flags & kFlagNoStorer) && B.nloc <= BS / 2 && B.nvirt <= BS / 2 &&
                       B.ncout * kChunkBwd <= BS / 2;
  const bool imp_mode = help_ok && B.ncout > 0;
  // x helpers (same blocks): the upper half also loads each reach's x(t - 4) row from x_save, kBwdHelpAhead
  // ticks ahead, and publishes it into the reach's slot, so the routing waves issue no x_save load and do
  // not wait at the tick's top for one
  const bool xhelp = help_ok;
  // gradient helpers (x-helper blocks, per-reach dL/drunoff, statics in registers): the same upper waves also
  // load each reach's dL/drunoff[:, t] kBwdHelpAhead ticks ahead and publish it into a parity-indexed LDS row
  // (the statics table's space, unused when the statics live in registers), so the routing waves issue no
  // global load and wait for none at the tick's top (a cold 16-B group load, one tick ahead, paced the light
  // backward: profiles/r05/ab_r05.txt item 12)
  const bool ghelp = kStatReg && kShiftG && xhelp && !(gauge);
  R* const sg = lds.stat;  // [2][S] (ghelp): dL/drunoff of each reach's step, by tick parity
  // virtual inflow owners (tid < nvirt): v_edge, v_off in registers; in LDS (own[tid], registers are
  // full) the virtual's consumer slot (low 16 bits) and the tick offset of cut-out `tid` (high 16 bits,
  // tid < ncout: its import owner)
  int v_edge = 0, v_off = 0;
  unsigned* own = reinterpret_cast<unsigned*>(smem + a.own_off);
  if (vown) {
    v_edge = a.s.v_edge[B.virt0 + tid];
    v_off = a.s.v_off[B.virt0 + tid];
  }
  if (tid < B.nvirt || tid < B.ncout)
    own[tid] = (vown ? (unsigned)a.s.v_dloc[B.virt0 + tid] & 0xFFFFu : 0u) |
               (tid < B.ncout ? (unsigned)a.s.off[B.pos0 + a.s.cout_loc[B.cout0 + tid]] << 16 : 0u);
  auto v_dloc_of = [&]() { return (int)(own[tid] & 0xFFFFu); };
  const int TT = (int)T + B.dmax;
  load_math_tables();
  load_xlist(a.s, B, xl);
  // split basin: [nvirt] the virtuals' export rows (to the producer block's rank), then [ncout] the
  // cut-outs' import rows (this rank's receive rows for edges from another rank's consumer)
  uintptr_t* xtv = reinterpret_cast<uintptr_t*>(smem + xt_off);
  uintptr_t* xtc = xtv + B.nvirt;
  if (xt_off) {
    for (int v = tid; v < B.nvirt; v += BS) {
      const int64_t e = a.s.v_edge[B.virt0 + v];
      const int xi = a.xid[e];
      xtv[v] = xi >= 0 ? (reinterpret_cast<uintptr_t>(a.pxbwd[a.xprod[xi]] + (int64_t)xi * T * 2) | 1u)
                       : reinterpret_cast<uintptr_t>(a.bwd_bnd + e * T * 2);
    }
    for (int c = tid; c < B.ncout; c += BS) {
      const int64_t e = B.cout0 + c;
      const int xi = a.xid[e];
      xtc[c] = xi >= 0 ? (reinterpret_cast<uintptr_t>(a.xbwd + (int64_t)xi * T * 2) | 1u)
                       : reinterpret_cast<uintptr_t>(a.bwd_bnd + e * T * 2);
    }
  }
  __syncthreads();
  unsigned long long prof_wait = 0;
  if (aprof && tid == 0) prof_begin(aprof, bid);
  PhaseProf phz;

  // x of this reach at forward tick `tau` (clamped into the block's rows)
  auto load_own = [&](int tau, R(&dst)[KR], int tq) {
    const int tc = tau < 0 ? 0 : (tau >= TT ? TT - 1 : tau);
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      if (wbase + k * BS >= B.nloc) continue;
      const int r = tq + k * BS;
      dst[k] = xsave[xs_base + (int64_t)tc * B.nloc + (r < B.nloc ? r : 0)];
    }
  };
  // x of a virtual inflow (the upstream reach of cut edge v_edge) at step t, from the forward's
  // boundary granules (t clamped into [0, T))
  // split basin: a virtual whose producer is another rank's block sends its x to this rank's receive rows;
  // split_finish_kernel copied them into this call's bnd after the forward
  const int vxi = (!PL && vown && a.xid) ? a.xid[v_edge] : -1;  // split basin: the virtual's cross-rank row
  auto load_virt = [&](int64_t t) -> double {
    const int64_t tc = t < 0 ? 0 : (t >= T ? T - 1 : t);
    return a.bnd[(int64_t)v_edge * T + tc];
  };
  // dL/drunoff of steps base .. base + 3 of reach slice k (mmc.py:380-412: runoff[ref, t] = Q_t; in
  // gauge mode every gauge sums its reaches' Q_t, mmc.py:405-411, 433-439).  `base` is 4-aligned except
  // for a reach's first group (un: base = T - 4, any alignment; steps outside [0, T) read clamped rows and
  // are never consumed)
  auto load_grad_out = [&](int ref, int64_t base, int gs, bool un) {
    R v0 = R(0), v1 = R(0), v2 = R(0), v3 = R(0);
    const bool v4 = vec4 && !(un && (base & 3) != 0);
    // !un (steady ticks): the group's steps lie in [1, T - 2], so the clamps (int64 compares and selects the
    // compiler hoists above the vec4 branch, run by the whole wave every tick) are dropped -- at KR = 4 (at
    // KR = 1 the light C5-shaped backward measured 6 % slower without them, r05_nc0)
    auto cl = [&](int64_t i) {
      return (!un && KR >= 4) ? i : (i < 0 ? int64_t(0) : (i < T ? i : T - 1));
    };
    const int64_t i0 = cl(base), i1 = cl(base + 1), i2 = cl(base + 2), i3 = cl(base + 3);
    // m0: the gauge's t = 0 sum passed its clamp (state gradients only; mmc.py:398-412)
    auto add_row = [&](const R* row, bool m0) {
      if (v4) {
        if constexpr (sizeof(R) == 4) {
          const float4 v = load_grad4(row + base);
          v0 = v0 + ((m0 || base != 0) ? v.x : 0.0f); v1 = v1 + v.y; v2 = v2 + v.z; v3 = v3 + v.w;
        } else {
          const double2 u = reinterpret_cast<const double2*>(row + base)[0];
          const double2 w = reinterpret_cast<const double2*>(row + base)[1];
          v0 = v0 + ((m0 || base != 0) ? u.x : 0.0); v1 = v1 + u.y; v2 = v2 + w.x; v3 = v3 + w.y;
        }
      } else {
        v0 = v0 + ((m0 || base != 0) ? row[i0] : R(0));
        v1 = v1 + ((m0 || base != -1) ? row[i1] : R(0));
        v2 = v2 + ((m0 || base != -2) ? row[i2] : R(0));
        v3 = v3 + ((m0 || base != -3) ? row[i3] : R(0));
      }
    };
    // a row's four values as loaded: no arithmetic on them in this tick, so the wave does not wait for the load
    // (it lands by the next tick's top; adding them to 0 would consume it now -- a full memory round trip)
    auto raw_row = [&](const R* row) {
      if (v4) {
        if constexpr (sizeof(R) == 4) {
          const float4 v = load_grad4(row + base);
          return make_grad4(v.x, v.y, v.z, v.w);
        } else {
          const double2 u = reinterpret_cast<const double2*>(row + base)[0];
          const double2 w = reinterpret_cast<const double2*>(row + base)[1];
          return make_grad4(u.x, u.y, w.x, w.y);
        }
      }
      return make_grad4(row[i0], row[i1], row[i2], row[i3]);
    };
    if (gauge) {
      const bool z = GS && a.gmask0 && base <= 0;  // the group holds step 0
      if (gs >= 0) {
        // the reach's only gauge (kGReg): the row address needs no dependent index loads in the tick
        // (its values as loaded instead of added to 0, so that this tick does not wait for them: no change
        // at c3s8, r05_gr)
        add_row(gout + (int64_t)gs * T, !(z && a.gmask0[gs] == 0));
        return make_grad4(v0, v1, v2, v3);
      }
      const int64_t q1 = a.g_roff[ref + 1];
      for (int64_t q = a.g_roff[ref]; q < q1; ++q) {
        const int64_t gi = a.g_rg[q];
        add_row(gout + gi * T, !(z && a.gmask0[gi] == 0));
      }
      return make_grad4(v0, v1, v2, v3);
    }
    // one reach row: the loaded values as they are
    return raw_row(gout + (int64_t)ref * T);
  };
  // ... plus the state seeds of steps T - 1 and T - 2 (a.gseed).  Only outside the steady ticks (seeded: the
  // steady range then starts late enough that no steady tick loads the groups of those steps), so the steady
  // loop's code and registers are those of an unseeded launch
  auto load_grad = [&](int ref, int64_t base, int gs, bool seeded) {
    Grad4<R> v = load_grad_out(ref, base, gs, seeded);
    if (seeded && gseed != nullptr && base + 3 >= T - 2) {
      const R* sd = static_cast<const R*>(gseed);
      const R s1 = sd[ref], s2 = sd[a.N + ref];
      auto add = [&](R& g, int64_t t) { g = g + (t == T - 1 ? s1 : (t == T - 2 ? s2 : R(0))); };
      add(v.a, base);
      add(v.b, base + 1);
      add(v.c, base + 2);
      add(v.d, base + 3);
    }
    return v;
  };

  // (ghelp) the value helper w publishes at backward tick tb, read by its reach at tick tb + 1: dL/drunoff of the
  // step t = TT - 2 - tb - off (0 outside [0, T)), plus the state seeds of steps T - 1 and T - 2
  // (rf, off: reach w's reference index and tick offset, loaded once)
  auto ghelp_load = [&](int rf, int off, int tb) -> R {
    const int64_t t = (int64_t)TT - 2 - tb - off;
    if (t < 0 || t >= T) return R(0);
    R v = gout[(int64_t)rf * T + t];
    if (gseed != nullptr && t >= T - 2) v = v + static_cast<const R*>(gseed)[(t == T - 1 ? 0 : a.N) + rf];
    return v;
  };

  // virtual inflow's x(t_v - 2), prefetched one tick ahead (kept as loaded: converting it would
  // wait for the load in the tick that issues it)
  double vx = 0.0, vx2 = 0.0;

  // xbc / vxc: loaded last tick, published now; xbn / vxn: loaded now for the next tick (the same
  // registers without early loads)
  // sc: std::integral_constant<bool, kSt>.  Steady ticks (forward tick tau in [dmax + 2, T - 1]) are
  // those at which every reach runs a step t in [2, T - 1]: no activity tests, no t = 1 carried-state
  // case, no step-0 sweep, the next step's gradient group always in range
  auto tick = [&](int tb, R(&xbc)[KR], R(&xbn)[KR], double& vxc, double& vxn, auto sc) {
    constexpr bool kSt = decltype(sc)::value;
    const int tau = TT - 1 - tb;  // forward tick
    // Every global load of the previous tick (states, virtual inflows, gradient groups) lands
    // here, a whole tick after its issue.  An explicit wait the compiler can see: without it, its
    // conservative count across the divergent load branches waits (vmcnt(0)) at the first use of a
    // previous-tick register, i.e. for the loads issued in THIS tick too.
    __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);
    if constexpr (KR == 4) set_prio(3);
    phz.mark(0);  // the previous tick's loads and stores
    const int tq = opq(tid);
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      ref[k] = opq(ref[k]);
      od[k] = opq(od[k]);
      up[k] = opq(up[k]);
    }
    // kDbl: this tick publishes (into the next tick's x buffer) the values loaded last tick, and loads
    // those it publishes next tick -- one tick further ahead than without double buffering
    const R* sar = sa + (kDbl ? ((tb + 1) & 1) * S : 0);  // the downstream's values of the previous tick
    const R* sbr = sb + (kDbl ? ((tb + 1) & 1) * S : 0);
    R* saw = sa + (kDbl ? (tb & 1) * S : 0);              // this tick's (c1 gb, c2 gb)
    R* sbw = sb + (kDbl ? (tb & 1) * S : 0);
    const R* sxr = sx + (kDbl ? (tb & 1) * S : 0);        // x published for this tick
    R* sxw = sx + (kDbl ? ((tb + 1) & 1) * S : 0);        // (kDbl) x published for the next tick
    if constexpr (kEarly) {
      constexpr int ahead = kDbl ? 1 : 0;
      if (!xhelp) load_own(tau - 3 - ahead, xbn, tq);              // x(t - 3) (kDbl: x(t - 4)), published next tick
      if (vown) vxn = load_virt((int64_t)tau - 1 - ahead - v_off - 2);  // the virtual's value for the next tick
    }
    if (B.ncout > 0 && (tb % kChunkBwd) == 0) {
      // one (cut-out, step) per thread and iteration, its (A, B) granule pair requested together; the
      // cut edge of cut-out c is B.cout0 + c (graph.cpp numbers cut edges in block order), its tick
      // offset is in the owner words
      const unsigned long long w0 = aprof ? __builtin_amdgcn_s_memrealtime() : 0;
      for (int w = tid; !imp_mode && w < B.ncout * kChunkBwd; w += BS) {
        const int c = w / kChunkBwd, sidx = w % kChunkBwd;
        const int t = (tau - sidx) - (int)(own[c] >> 16);
        R A = R(0), Bv = R(0);
        if (t >= tmin && t < T) {
          double g[2];
          const uintptr_t p = xt_off ? xtc[c] : reinterpret_cast<uintptr_t>(a.bwd_bnd + (int64_t)(B.cout0 + c) * T * 2);
          const double* row = reinterpret_cast<const double*>(p & ~uintptr_t(1)) + (int64_t)t * 2;
          if (p & 1u) wait_granules<2, true>(row, 0, 0, 2, g, a.status, bid, force_to);  // another rank's consumer
          else wait_granules<2>(row, 0, 0, 2, g, a.status, bid, force_to);
          A = R(g[0]);
          Bv = R(g[1]);
        }
        ring[(c * kChunkBwd + sidx) * 2] = A;
        ring[(c * kChunkBwd + sidx) * 2 + 1] = Bv;
      }
      lds_barrier();
      if (aprof) prof_wait += __builtin_amdgcn_s_memrealtime() - w0;
    }
    phz.mark(1);  // import
    // ---- read / publish ----------------------------------------------------------------------
    if (vown) {
      // export the consumer's (c1 gb, c2 gb) of step t (written last tick, when the consumer ran
      // step tau + 1 - off_c = tau - v_off) to the upstream block; publish the upstream reach's x
      // at the consumer's current step - 1 (kDbl: next step's, into the next tick's buffer)
      const int t = tau - v_off;
      if (t >= tmin && t < T) {
        const int dloc = v_dloc_of();
        if (vxi >= 0) {  // split basin: the producer block is another rank's (row from the block's table)
          double* dst = reinterpret_cast<double*>(xtv[tid] & ~uintptr_t(1)) + (int64_t)t * 2;
          store_granule_sys(dst, (double)sar[dloc]);
          store_granule_sys(dst + 1, (double)sbr[dloc]);
        } else {
          store_granule(a.bwd_bnd + ((int64_t)v_edge * T + t) * 2, (double)sar[dloc]);
          store_granule(a.bwd_bnd + ((int64_t)v_edge * T + t) * 2 + 1, (double)sbr[dloc]);
        }
      }
      sxw[B.nloc + tid] = R(vxc);
    }
    R A[KR], Bd[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      A[k] = R(0);
      Bd[k] = R(0);
      if (wbase + k * BS >= B.nloc) continue;
      const int r = tq + k * BS;
      // x(t - 2): the upstream value of the downstream reach's step t - 1 (kDbl: next tick's, x(t - 3))
      if (!xhelp && r < B.nloc) sxw[r] = xbc[k];
      const int dl = dl_of(k);
      if (dl >= 0) {
        A[k] = sar[dl];
        Bd[k] = sbr[dl];
      } else if (dl <= -2) {
        const int sidx = tb % kChunkBwd;
        A[k] = ring[((-dl - 2) * kChunkBwd + sidx) * 2];
        Bd[k] = ring[((-dl - 2) * kChunkBwd + sidx) * 2 + 1];
      }
    }
    phz.mark(2);  // read / publish
    if constexpr (!kDbl) lds_barrier();
    phz.mark(3);  // barrier 1
    if constexpr (!kEarly) {
      load_own(tau - 3, xbn, tq);                    // x(t - 3), published next tick
      if (vown) vxn = load_virt((int64_t)tau - 1 - v_off - 2);  // the virtual's value for the next tick
    }
    // ---- compute ------------------------------------------------------------------------------
    // per slice: the step's inputs (pre), its adjoint, its outputs (post) and the next loads (tail)
    struct Pre {
      int r, rs, t;
      bool hk, active, c0;
      R Sx, I, gk, xtk, lm, gb, Qp, D1, D2;
      double gb64;
      ReachStatic<R> st;
    };
    auto pre = [&](int k, Pre& P) {
      P.r = tq + k * BS;
      P.hk = P.r < B.nloc;
      P.rs = P.hk ? P.r : 0;
      P.t = tau - off_of(k);
      P.active = P.hk && (kSt || (P.t >= 1 && P.t < T));
      // upstream x_j(t - 1): I(t) = sum_j Q_j(t - 1) (mmc.py:535, ascending columns; the carried
      // state at t - 1 = 0 is not clamped) and Sx(t - 1) for the next tick
      P.c0 = !kSt && (P.t == 1 && carry);
      const bool c0 = P.c0;
      const int nup = up_n(up[k]);
      const R x0 = sxr[up_0(up[k])];
      const R x1 = sxr[up_1(up[k], xl)];
      SxT sxv = SxT(0) + SxT(x0);
      sxv = sxv + SxT(x1);
      SxT I = SxT(0);
      I = I + SxT(nup > 0 ? (c0 ? x0 : rmaxc(x0, cs.qlb, cs)) : R(0));
      I = I + SxT(nup > 1 ? (c0 ? x1 : rmaxc(x1, cs.qlb, cs)) : R(0));
      if (nup > 2) {
        const int* lst = xl + up_f1(up[k]);
        const int c = lst[0];
        for (int j = 2; j < c; ++j) {
          const R xj = sxr[lst[j]];
          sxv = sxv + SxT(xj);
          I = I + SxT(c0 ? xj : rmaxc(xj, cs.qlb, cs));
        }
      }
      const SxT Sx = sxn[k];  // sum_j x_j(t), the solve's upstream term of this step
      P.I = R(I);
      P.Sx = R(Sx);
      sxn[k] = sxv;
      if constexpr (kShiftG) {
        // dL/drunoff[:, t]: the group's registers shift by one step per tick (g3 holds step t: a group is loaded
        // the tick before its top step runs) -- no per-lane select on t & 3
        P.gk = g3[k];
        g3[k] = g2[k];
        g2[k] = g1[k];
        g1[k] = g0[k];
        if (kStatReg && ghelp) P.gk = sg[(tb & 1) * S + P.rs];  // published by the gradient helpers last tick
      } else {
        const int e4 = P.t & 3;
        // dL/drunoff[:, t] by two bit tests and three selects (a ternary chain on e4 compiles into divergent
        // branches)
        const bool b0 = (e4 & 1) != 0, b1 = (e4 & 2) != 0;
        const R lo = b0 ? g1[k] : g0[k], hi = b0 ? g3[k] : g2[k];
        P.gk = b1 ? hi : lo;
      }
      P.xtk = xc[k];
      P.st = kStatReg ? sreg[k] : tab.template get<true>(P.rs);
      P.lm = lam[k] + P.gk;                                 // dL/dQ_t (+ dL/dout[:, t])
      const R gx = (P.xtk >= cs.qlb) ? P.lm : R(0);         // clamp backward (inclusive)
      P.gb64 = (double)gx + (double)A[k];                   // (I - C1 N)^T gb = gx (utils.py:188-242)
      P.gb = R(P.gb64);
      P.Qp = c0 ? xa[k] : rmaxc(xa[k], cs.qlb, cs);              // Q_{t-1}
      if constexpr (kDF) {
        const SxT Qq = (SxT)P.Qp - (SxT)rmaxc(qsv[kQs ? k : 0], cs.qlb, cs);  // exact in fp64
        P.D1 = R(Qq - Sx);
        P.D2 = R(Qq - I);
      }
    };
    auto adjoint = [&](int k, const Pre& P, AdjOutR<R>& o) {
      if constexpr (std::is_same<R, float>::value) {
        AdjOut f;
        if constexpr (kDF) f = adjoint_step_fast<true>(P.st, P.Qp, cs, P.gb, P.D1, P.D2, R(0));
        else f = adjoint_step_fast<false>(P.st, P.Qp, cs, P.gb, P.xtk, P.Sx, P.I);
        o = AdjOutR<R>{f.c1, f.c2, f.c3, f.c4, f.gQ, f.gn, f.gq, f.gp};
      } else {
        const R qvk = *qs_at<R>(a, B, xs_base, tau, off_of(k), P.rs);  // q'[t-1] * flow_scale
        R tw, ss;
        Geom<R> geo;
        coefficients<R, true>(P.st, P.Qp, cs, o.c1, o.c2, o.c3, o.c4, tw, ss, &geo);
        const R qc = rmaxc(qvk, cs.qlb, cs);
        const R gc1 = P.gb * P.Sx, gc2 = P.gb * P.I, gc3 = P.gb * P.Qp, gc4 = P.gb * qc;
        coefficients_vjp<R, true>(P.st, P.Qp, cs, geo, o.c1, o.c2, o.c3, o.c4, gc1, gc2, gc3, gc4, o.gQ, o.gn,
                                            o.gq, o.gp);
      }
    };
    auto post = [&](int k, const Pre& P, const AdjOutR<R>& o) {
      const int r = P.r, t = P.t;
      const R gb = P.gb;
      if (P.active) {
        pn[k] = pn[k] + o.gn;
        pq[k] = pq[k] + o.gq;
        pp[k] = pp[k] + o.gp;
        // flush the fp32 partial sums into the fp64 accumulators every kGradFlush *steps* (aligned to
        // t, not to ticks, so the summation grouping -- and the result -- is independent of the
        // partition); one owner per address, so the atomics are deterministic
        if ((t % kGradFlush) == 1 || (!kSt && t == 1)) {
          double* g3p = gacc + (int64_t)ref[k] * 3;
          atomicAdd(g3p + 0, (double)pn[k]);
          atomicAdd(g3p + 1, (double)pq[k]);
          atomicAdd(g3p + 2, (double)pp[k]);
          pn[k] = pq[k] = pp[k] = R(0);
        }
        saw[r] = R((double)o.c1 * P.gb64);
        sbw[r] = o.c2 * gb;
        lam[k] = ((gb * o.c3) + o.gQ) + Bd[k];
        // dL/dqc = gb c4 (b = ... + c4 qc), through qc = clamp(q' * flow_scale) (mmc.py:421-424)
        if constexpr (GS) gqs[xs_base + (int64_t)tau * B.nloc + r] = (qsv[k] >= cs.qlb) ? gb * o.c4 : R(0);
      } else if (!kSt && GS && P.hk && t == 0) {
        if (carry) {
          // Q0 = q0 feeds step 1 unclamped; runoff[:, 0] = clamp(q0) per reach, or the gauge sum's clamp
          // (already folded into gk through gmask0)
          if (a.gq0) static_cast<R*>(a.gq0)[ref[k]] = gauge ? P.lm : lam[k] + ((P.xtk >= cs.qlb) ? P.gk : R(0));
          gqs[xs_base + (int64_t)tau * B.nloc + r] = R(0);
          saw[r] = R(0);
          sbw[r] = R(0);
        } else {
          // hot start x(0) = (I - N)^-1 q'[0] (mmc.py:25-66): its transposed solve (c1 = 1) is gb64
          gqs[xs_base + (int64_t)tau * B.nloc + r] = gb;
          saw[r] = gb;
          sbw[r] = R(0);
        }
      }
    };
    auto tail = [&](int k, const Pre& P) {
      if constexpr (kQs) {
        const int tn = tau > 0 ? tau - 1 : 0;  // the next backward tick's row
        qsv[k] = *qs_at<R>(a, B, xs_base, tn, off_of(k), P.rs);
      }
      // dL/drunoff of the next step's group, one tick ahead
      const int tn = P.t - 1;
      if (!ghelp && P.hk && has_grad(k) && (kSt ? (tn & 3) == 3 : (tn >= 0 && tn < T && ((tn & 3) == 3 || tn == T - 1)))) {
        const Grad4<R> v = load_grad(ref[k], kShiftG ? (int64_t)tn - 3 : (int64_t)(tn & ~3),
                                     kGReg ? opq(gsg[kGReg ? k : 0]) : -1, !kSt);
        g0[k] = v.a; g1[k] = v.b; g2[k] = v.c; g3[k] = v.d;
      }
    };
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      if (wbase + k * BS >= B.nloc) continue;
      if constexpr (KR == 4) set_prio(KR - 1 - k);
      Pre P;
      pre(k, P);
      AdjOutR<R> o;
      adjoint(k, P, o);
      post(k, P, o);
      tail(k, P);
      __builtin_amdgcn_sched_barrier(0);
    }
    phz.mark(4);  // loads issue + compute
    // next tick: x(t - 1) -> x(t); x(t - 2), still in the own slot -> x(t - 1).  kDbl: read before the
    // barrier (no one writes this tick's read buffer during the tick; after the barrier the x helpers
    // may already be writing it for the next tick)
    auto shift_x = [&]() {
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        if (wbase + k * BS >= B.nloc) continue;
        const int r = tq + k * BS;
        xc[k] = xa[k];
        xa[k] = r < B.nloc ? sxr[r] : R(0);
      }
    };
    if constexpr (kDbl) shift_x();
    lds_barrier();
    phz.mark(5);  // barrier 2
    if constexpr (!kDbl) shift_x();
  };

  // tick 0 runs forward tick TT-1: x(t) at row TT-1, x(t-1) at row TT-2, x(t-2) at row TT-3
  if constexpr (kQs) {
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int r = tid + k * BS;
      qsv[k] = *qs_at<R>(a, B, xs_base, TT - 1, off_of(k), r < B.nloc ? r : 0);
    }
  }
  load_own(TT - 1, xc, tid);
  load_own(TT - 2, xa, tid);
  load_own(TT - 3, xb, tid);
  // prologue: Sx of every reach's first step t0 = sum_j x_j(t0), where x_j(t0) is the upstream
  // reach's x one step before its own first step (its xa; a virtual inflow's granule) -- (kDbl) in buffer
  // 1, which tick 0 then overwrites
  R* sxp = sx + (kDbl ? S : 0);
#pragma unroll
  for (int k = 0; k < KR; ++k)
    if (tid + k * BS < B.nloc) sxp[tid + k * BS] = xa[k];
  if (vown) sxp[B.nloc + tid] = R(load_virt((int64_t)(TT - 1) - v_off - 1));
  __syncthreads();
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const int r = tid + k * BS;
    if (r >= B.nloc) continue;
    SxT v = SxT(0) + SxT(sxp[up_0(up[k])]);
    v = v + SxT(sxp[up_1(up[k], xl)]);
    if (up_n(up[k]) > 2) {
      const int* lst = xl + up_f1(up[k]);
      for (int j = 2; j < lst[0]; ++j) v = v + SxT(sxp[lst[j]]);
    }
    sxn[k] = v;
  }
  __syncthreads();
  if (vown) vx = load_virt((int64_t)(TT - 1) - v_off - 2);
  if constexpr (kDbl) {
    // tick 0's published values (x(t0 - 2), the virtuals') go into its read buffer now; the registers
    // then hold what tick 0 publishes for tick 1
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (tid + k * BS < B.nloc) sx[tid + k * BS] = xb[k];
    if (vown) sx[B.nloc + tid] = R(vx);
    load_own(TT - 4, xb, tid);
    if (vown) vx = load_virt((int64_t)(TT - 2) - v_off - 2);
    // (ghelp) tick 0's dL/drunoff row, written by the helper thread of each reach
    if (ghelp && tid >= BS / 2 && tid - BS / 2 < B.nloc) {
      const int P = B.pos0 + tid - BS / 2;
      sg[tid - BS / 2] = ghelp_load(a.s.ref[P], a.s.off[P], -1);
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < KR; ++k)
    if (!ghelp && tid + k * BS < B.nloc && has_grad(k) && TT - 1 - off_of(k) == T - 1) {
      const Grad4<R> v = load_grad(ref[k], kShiftG ? T - 4 : (T - 1) & ~int64_t(3), kGReg ? gsg[kGReg ? k : 0] : -1, true);
      g0[k] = v.a; g1[k] = v.b; g2[k] = v.c; g3[k] = v.d;
    }
  if ((imp_mode || xhelp) && wbase >= BS / 2) {
    // import waves: thread w owns (cut-out w / kChunkBwd, step slot w % kChunkBwd) of every chunk; per tick
    // the same barriers as the routing waves' tick (the ring hand-off at a chunk boundary, the tick's end).
    // x helpers: thread w < nloc publishes reach w's x(t - 4) (forward row TT - 4 - tb at tick tb, clamped)
    // into the next tick's x buffer, its loads issued kBwdHelpAhead ticks ahead
    const int w = tid - BS / 2;
    const bool wown = imp_mode && w < B.ncout * kChunkBwd;
    const bool xown = xhelp && w < B.nloc;
    constexpr int XD = kBwdHelpAhead;
    const R* xcol = xsave + xs_base + (xown ? w : 0);
    auto xload = [&](int tb) -> R {
      int tc = TT - 4 - tb;
      tc = tc < 0 ? 0 : (tc >= TT ? TT - 1 : tc);
      return xown ? xcol[(int64_t)tc * B.nloc] : R(0);
    };
    R xp[XD], gp[XD];
    const bool gown = ghelp && w < B.nloc;
    const int grf = gown ? a.s.ref[B.pos0 + w] : 0, goff = gown ? a.s.off[B.pos0 + w] : 0;
#pragma unroll
    for (int i = 0; i < XD; ++i) {
      xp[i] = xload(i);
      gp[i] = gown ? ghelp_load(grf, goff, i) : R(0);
    }
    const int c = wown ? w / kChunkBwd : 0, sidx = w % kChunkBwd;
    const uintptr_t p = !wown ? 0 : xt_off ? xtc[c] : reinterpret_cast<uintptr_t>(a.bwd_bnd + (int64_t)(B.cout0 + c) * T * 2);
    const bool sys = p & 1u;
    const double* prow = reinterpret_cast<const double*>(p & ~uintptr_t(1));
    const int coff = wown ? (int)(own[c] >> 16) : 0;
    auto step_of = [&](int tb) { return (TT - 1 - tb - sidx) - coff; };  // the step chunk tb's slot needs
    unsigned long long eg[2] = {0ull, 0ull};
    bool issued = false;
    auto htick = [&](int tb, R& xr, R& gr) {
      if (B.ncout > 0 && (tb % kChunkBwd) == 0) {
        if (wown) {
          const int t = step_of(tb);
          R A = R(0), Bv = R(0);
          if (t >= tmin && t < T) {
            double g[2];
            const double* row = prow + (int64_t)t * 2;
            if (issued) {
              if (sys) poll_granules<2, true>(row, 0, 0, 2, eg, g, a.status, bid, force_to);
              else poll_granules<2, false>(row, 0, 0, 2, eg, g, a.status, bid, force_to);
            } else {
              if (sys) wait_granules<2, true>(row, 0, 0, 2, g, a.status, bid, force_to);
              else wait_granules<2>(row, 0, 0, 2, g, a.status, bid, force_to);
            }
            A = R(g[0]);
            Bv = R(g[1]);
          }
          ring[(c * kChunkBwd + sidx) * 2] = A;
          ring[(c * kChunkBwd + sidx) * 2 + 1] = Bv;
        }
        issued = false;
        lds_barrier();
      }
      if (xown) {
        sx[((tb + 1) & 1) * S + w] = xr;  // the routing waves read it next tick
        xr = xload(tb + XD);
      }
      if (gown) {
        sg[((tb + 1) & 1) * S + w] = gr;
        gr = ghelp_load(grf, goff, tb + XD);
      }
      const int nb = tb + kBwdImpEarly;
      if (wown && (nb % kChunkBwd) == 0 && nb < TT) {
        const int t = step_of(nb);
        if (t >= tmin && t < T) {
          const double* row = prow + (int64_t)t * 2;
          if (sys) issue_granules<2, true>(row, 0, 0, 2, eg);
          else issue_granules<2, false>(row, 0, 0, 2, eg);
          issued = true;
        }
      }
      lds_barrier();  // the routing waves' tick end
    };
    // unrolled by XD: each prefetch register is consumed in place (a register copy would wait for its load)
#pragma unroll 1
    for (int tb = 0; tb < TT; tb += XD) {
#pragma unroll
      for (int i = 0; i < XD; ++i)
        if (tb + i < TT) htick(tb + i, xp[i], gp[i]);
    }
    return;
  }
  phz.start();
  using Gen = std::integral_constant<bool, false>;
  using Steady = std::integral_constant<bool, true>;
  // steady backward ticks [b0, b1): forward ticks tau = TT - 1 - tb in [dmax + 2, T - 1]
  // (state seeds: from forward tick T - 2 down, so that every load of the groups of steps T - 2 and T - 1 --
  // issued at forward ticks >= T - 1 -- runs in a general tick)
  int b0 = gseed != nullptr ? B.dmax + 1 : B.dmax, b1 = (int)T - 2;
  if (kEarly) {  // even bounds: the register roles keep alternating
    b0 += b0 & 1;
    b1 &= ~1;
  }
  if ((a.flags & kFlagNoSteady) || b1 <= b0) b0 = b1 = 0;
  if constexpr (kEarly) {
#pragma unroll 1
    for (int tb = 0; tb < b0; tb += 2) {
      if (aprof && tid == 0) prof_tick(aprof, bid, tb);
      tick(tb, xb, xb2, vx, vx2, Gen{});
      tick(tb + 1, xb2, xb, vx2, vx, Gen{});
    }
#pragma unroll 1
    for (int tb = b0; tb < b1; tb += 2) {
      if (aprof && tid == 0) prof_tick(aprof, bid, tb);
      tick(tb, xb, xb2, vx, vx2, Steady{});
      tick(tb + 1, xb2, xb, vx2, vx, Steady{});
    }
#pragma unroll 1
    for (int tb = b1; tb < TT; tb += 2) {
      if (aprof && tid == 0) prof_tick(aprof, bid, tb);
      tick(tb, xb, xb2, vx, vx2, Gen{});
      if (tb + 1 < TT) tick(tb + 1, xb2, xb, vx2, vx, Gen{});
    }
  } else {
#pragma unroll 1
    for (int tb = 0; tb < b0; ++tb) {
      if (aprof && tid == 0) prof_tick(aprof, bid, tb);
      tick(tb, xb, xb, vx, vx, Gen{});
    }
#pragma unroll 1
    for (int tb = b0; tb < b1; ++tb) {
      if (aprof && tid == 0) prof_tick(aprof, bid, tb);
      tick(tb, xb, xb, vx, vx, Steady{});
    }
#pragma unroll 1
    for (int tb = b1; tb < TT; ++tb) {
      if (aprof && tid == 0) prof_tick(aprof, bid, tb);
      tick(tb, xb, xb, vx, vx, Gen{});
    }
  }
  if (aprof && tid == 0) prof_end(aprof, bid, prof_wait);
  phz.flush(aprof, a.nblocks, bid);
#undef gauge
#undef gseed
#undef aprof
#undef xt_off
}

// Final fp64 accumulators -> R gradients (reference order).
template <typename R>
__global__ void finish_grads_kernel(int64_t N, const double* gacc, R* gn, R* gq, R* gp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  gn[i] = R(gacc[3 * i + 0]);
  gq[i] = R(gacc[3 * i + 1]);
  gp[i] = R(gacc[3 * i + 2]);
}

// The backward's slot buffers on this graph: the KR rule's, unless its double buffer does not fit a CU's
// LDS at this real size (fp64 at KR = 2: 96 B per slot, ~1.6K-reach blocks), then one -- two barriers per
// tick instead of DDR_ERR_CAPACITY (the graph packer sizes blocks for the fp32 layouts)
template <typename R>
int bwd_xb_of(const Graph* g) {
  if (bwd_xbuf(g->kr) == 1) return 1;
  return (sizeof(R) == 8 && g->kr == 2 && route_lds_plan<R>(g, true, 2).smem > kLdsBudget) ? 1 : 2;
}

// the backward kernel of this launch (state gradients: GS; single-buffered fp64 KR = 2 slots: bwd_xb_of)
// (exact adjoint of the fp32 trajectory, DDR_BWD_EXACT_ADJOINT: df)
template <typename R, int KR>
const void* backward_kernel_of(const Graph* g, bool gs, bool df = false, int pl = 0) {
  if constexpr (KR == 2 && sizeof(R) == 8) {
    if (bwd_xb_of<R>(g) == 1)
      return gs ? (const void*)route_backward_kernel<R, KR, true, 1> : (const void*)route_backward_kernel<R, KR, false, 1>;
  }
  if constexpr (sizeof(R) == 4) {
    if (df)
      return gs ? (const void*)route_backward_kernel<R, KR, true, 0, true>
                : (const void*)route_backward_kernel<R, KR, false, 0, true>;
  }
  if constexpr (sizeof(R) == 4) {
    if (!gs && pl == 2) return (const void*)route_backward_kernel<R, KR, false, 0, false, 2>;
  }
  return gs ? (const void*)route_backward_kernel<R, KR, true> : (const void*)route_backward_kernel<R, KR, false>;
}
// Whether a launch runs the exact adjoint of the fp32 trajectory (DF): on request (DDR_BWD_EXACT_ADJOINT), and
// for every hot-started window of at most kExactShortT steps.  A hot start is the steady state of q'[0], so
// the first steps' mass imbalances are only what q' has drifted since: the parameter gradient is the remainder
// of terms that cancel to 1e-2 ... 1e-3 of their size, and the default adjoint's Q - x~ from the stored fp32 x(t)
// (physics.h) is 1.3e-4 / 5.2e-5 / 2.5e-5 / 1.4e-5 of the gradient at T = 3 / 4 / 5 / 6 on a 300-reach tree
// (tests/test_gpu_time_axis.py), above the 5e-5 the fp32 gradients hold elsewhere.  DF holds 5e-7 there, and its
// extra work on a launch of a few ticks is not measurable.  Carried windows (route_timestep chains) start from
// an arbitrary state and keep the default.
constexpr int64_t kExactShortT = 8;
inline bool backward_exact_of(const RouteArgs& a) {
  return (a.flags & DDR_BWD_EXACT_ADJOINT) != 0 || (!(a.flags & DDR_FWD_CARRY) && a.T <= kExactShortT);
}
// the plain backward instance a launch can take (route_backward_kernel's PL), 0 when none
inline int backward_plain_of(const Graph* g, const RouteArgs& a) {
  if ((a.flags & kFlagNoPlain) || g->split.nranks > 0 || a.prof != nullptr || a.gseed != nullptr || (a.T & 3) != 0) return 0;
  // gauge mode only: c3s8 backward -4.5 %; per-reach dL/drunoff (PL = 1) measured 0.5-1.5 % slower at C5 and
  // 3 % at light load (r05_plain3, r05_pl1), so that instance is not built
  return a.g_roff != nullptr ? 2 : 0;
}

template <typename R, int KR>
hipError_t launch_backward_kr(const Graph* g, RouteArgs a, hipStream_t stream) {
  const RouteLds lds = route_lds_plan<R>(g, true, bwd_xb_of<R>(g));
  set_launch_args(a, g, lds);
  const dim3 grid((unsigned)g->blocks.size()), block(kBlockThreads);
  const void* kern = backward_kernel_of<R, KR>(g, a.gqs != nullptr, backward_exact_of(a), backward_plain_of(g, a));
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds.smem);
  if (e != hipSuccess) return e;
  void* kargs[] = {&a};
  e = hipLaunchKernel(kern, grid, block, kargs, lds.smem, stream);
  if (e != hipSuccess) return e;
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned fb = (unsigned)((g->n + 255) / 256);
  hipLaunchKernelGGL(finish_grads_kernel<R>, dim3(fb), dim3(256), 0, stream, g->n,
                     (const double*)(a.bwd_bnd + 2 * g->n_cut * a.T), (R*)a.gn, (R*)a.gq, (R*)a.gp);
  return hipGetLastError();
}

template <typename R>
hipError_t launch_route_backward(const Graph* g, const RouteArgs& a, hipStream_t stream) {
  return dispatch_kr(g, [&](auto kr) { return launch_backward_kr<R, decltype(kr)::value>(g, a, stream); });
}

template <typename R>
int backward_resident_blocks(const Graph* g) {
  const void* f = dispatch_kr(g, [&](auto kr) { return backward_kernel_of<R, decltype(kr)::value>(g, false); });
  return resident_blocks(g, f, route_lds_plan<R>(g, true, bwd_xb_of<R>(g)).smem);
}

// one unit per precision instantiates the launch and the occupancy query
#define DDR_INSTANTIATE_ROUTE_BACKWARD(R)                                                            \
  template hipError_t launch_route_backward<R>(const Graph*, const RouteArgs&, hipStream_t); \
  template int backward_resident_blocks<R>(const Graph*);

}  // namespace ddr
