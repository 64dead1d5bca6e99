// Device helpers shared by the fused routing kernels for gfx950 (MI355X): the Muskingum-Cunge forward over
// all T steps (route_forward.hip), its reverse-time / reverse-topological adjoint (route_backward.h) and the
// linear Muskingum forward (route_linear.hip).  All three walk the schedule described here; the two forwards
// share its per-reach words (reach_words), and VirtOwner states the virtual-inflow owner for the linear
// kernel and any later kernel on this schedule (the Muskingum-Cunge forward keeps scalars of its own).
//
// One persistent workgroup owns a block of reaches (whole basins, or a connected piece of a large
// basin) for the whole time window.  Reach i runs step t at tick t + off(i) with
// off(i) = dmax - dist_in_piece(i): every upstream reach is exactly one tick ahead, so one
// LDS slot per reach + two workgroup barriers per tick carry all in-block dependencies
// ("as late as possible" wavefront; T + dmax ticks instead of T x depth level syncs).
// Edges between blocks (cut edges) are exchanged through global memory as 8-byte granules that
// are their own ready flag (sentinel = all ones, re-initialised before every launch), imported in
// chunks of kChunkFwd / kChunkBwd ticks so the hand-off latency is paid once per chunk.
//
// Workgroups take their logical block from a ticket counter (take_ticket): blocks are numbered in
// piece-height order, so the producers of a running workgroup were taken by workgroups that are
// running or finished, whatever the grid size and the dispatch order.  A schedule with more blocks
// than resident workgroups therefore runs to completion (as "generations"); one that fits runs
// fully time-pipelined.  Every wait is bounded: a timeout records the device status word and yields
// NaN, so a failed hand-off can never pass for a number (capi.cpp reports it as DDR_ERR_TIMEOUT).
//
// Each thread owns KR <= 4 reaches (r = tid + k * 1024); one 1024-thread workgroup per CU (4 waves
// per SIMD).  The per-reach statics live in LDS; registers hold only the per-reach state and one
// tick of prefetched inputs.  Each tick: compute (reads upstream slots) -> barrier -> publish (own
// slot) -> barrier.
//
// Reference semantics (file:line in the reference DDR sources):
//   forward  src/ddr/routing/mmc.py:365-443, 487-559, 25-66; routing/utils.py:587-600 (fp64 solve)
//   backward routing/utils.py:629-692 + torch autograd of mmc.py/trapezoidal.py (hand adjoint)
#pragma once

#include <type_traits>

#include "internal.h"
#include "physics.h"
#include "route_args.h"

namespace ddr {

// Tuning constant (chosen by an A/B on MI355X; the rejected alternatives live in git history and
// profiles/r0*/ab_*.txt, not here):
// The clamps' infinity opaque to the compiler from this KR on (one v_med3_f32 per clamp)
constexpr int kOpqInfMinKR = 4;

namespace {

constexpr unsigned long long kSentinel = ~0ull;
static_assert(kMathTabBytes == (2 * kLnTabN + kExpTabN) * sizeof(double), "math table size");


__device__ __forceinline__ void lds_barrier() {
  // LDS hand-off only: global loads issued ahead (prefetch) stay in flight across the barrier.
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Wave priority by remaining slices: the SIMD's arbiter serves its oldest ready wave
// first, so the workgroup's first waves finish their slices early and the youngest runs its last slices
// alone at the end of every tick, one dependent chain issuing on the SIMD.  A wave at slice k of KR takes
// priority KR - 1 - k (the top of the tick: 3), so the waves with more work left go first and the
// SIMD's waves finish together.  KR = 4 (full load): C5 129.4 -> 126.2 ms, C3 forward 16.0 -> 14.4 ms
// (profiles/r04/ab_r04.txt item 28); at KR = 2 no gain was measured (C4), KR = 1 has one slice.
// (forward at KR = 1) a routing wave runs its step's physics at priority 1 and the rest at 0:
// of the two routing waves on a SIMD, the one ahead yields once its physics is done, so the two finish
// together (c3s8 forward 2.87 -> 2.75 ms; C2 and c5s8r5 within noise; the backward's adjoint showed no
// change; profiles/r04/ab_r04.txt item 30)
__device__ __forceinline__ void set_prio(int p) {
  switch (p) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}

__device__ __forceinline__ void store_granule(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long load_granule(const double* p) {
  return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
// Cross-rank granules (split basin): system scope, so a peer GPU's stores into this rank's receive
// rows and this rank's stores into a peer's are seen through neither side's L2
__device__ __forceinline__ void store_granule_sys(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned long long load_granule_sys(const double* p) {
  return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

// Granules requested together by one import batch (register budget: 2 VGPRs each).
constexpr int kImportBatch = 4;
// The bounded wait for granules, in two halves.  issue_granules requests row[t0 + s] (s < C; outside
// [lo, hi): 0) all at once, so a chunk costs one memory round trip, not C; an import requested a chunk
// ahead stops there, and its granules land while the block runs on.  poll_granules spins (bounded) until
// the still-unpublished ones are published.  On a timeout (or with the debug flag that forces one) it
// records it in the status block and returns NaN: the corruption then shows in the outputs.
template <int C, bool Sys>
__device__ __forceinline__ void issue_granules(const double* row, int64_t t0, int64_t lo, int64_t hi,
                                               unsigned long long (&v)[C]) {
#pragma unroll
  for (int s = 0; s < C; ++s) {
    const int64_t t = t0 + s;
    v[s] = (t >= lo && t < hi) ? (Sys ? load_granule_sys(row + t) : load_granule(row + t)) : 0ull;  // +0.0 outside
  }
}
template <int C, bool Sys>
__device__ __forceinline__ void poll_granules(const double* row, int64_t t0, int64_t lo, int64_t hi,
                                              unsigned long long (&v)[C], double (&out)[C], unsigned* status, int bid,
                                              bool force_timeout) {
  auto ld = [](const double* p) { return Sys ? load_granule_sys(p) : load_granule(p); };
  unsigned pend = 0;
#pragma unroll
  for (int s = 0; s < C; ++s) pend |= (v[s] == kSentinel ? 1u : 0u) << s;
  unsigned spins = 0;
  while (pend != 0u || force_timeout) {
    ++spins;
    const bool failed = (spins & 1023u) == 0u &&
                        __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    if (force_timeout || failed || spins > (1u << 24)) {
      atomicAdd(status, 1u);
      atomicCAS(status + 1, 0u, (unsigned)bid + 1u);
#pragma unroll
      for (int s = 0; s < C; ++s) {
        const int64_t t = t0 + s;
        const bool nan = ((pend >> s) & 1u) || (force_timeout && t >= lo && t < hi);
        v[s] = nan ? 0x7FF8000000000000ull : v[s];
      }
      break;
    }
    __builtin_amdgcn_s_sleep(2);
#pragma unroll
    for (int s = 0; s < C; ++s) {
      const unsigned long long w = ((pend >> s) & 1u) ? ld(row + (t0 + s)) : v[s];
      v[s] = w;
      pend &= ~((w != kSentinel ? 1u : 0u) << s);
    }
  }
#pragma unroll
  for (int s = 0; s < C; ++s) out[s] = __longlong_as_double(v[s]);
}
// Request and wait at once.  It states poll_granules' loop a second time on purpose: as issue_granules +
// poll_granules every backward instance compiles differently (the KR = 1 import waves merge the two inlined
// polls; with `out` passed on through two references all instances reschedule), some with more spills.
// Keep the two loops in step.
template <int C, bool Sys = false>
__device__ __forceinline__ void wait_granules(const double* row, int64_t t0, int64_t lo, int64_t hi,
                                              double (&out)[C], unsigned* status, int bid, bool force_timeout) {
  auto ld = [](const double* p) { return Sys ? load_granule_sys(p) : load_granule(p); };
  unsigned long long v[C];
  unsigned pend = 0;
#pragma unroll
  for (int s = 0; s < C; ++s) {
    const int64_t t = t0 + (int64_t)s;
    v[s] = (t >= lo && t < hi) ? ld(row + t) : 0ull;  // +0.0 outside the window
  }
#pragma unroll
  for (int s = 0; s < C; ++s) pend |= (v[s] == kSentinel ? 1u : 0u) << s;
  unsigned spins = 0;
  while (pend != 0u || force_timeout) {
    ++spins;
    // a hand-off already failed in this launch (e.g. a split-basin peer that never arrives): give up
    // at once instead of spinning out every later wait too
    const bool failed = (spins & 1023u) == 0u &&
                        __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    if (force_timeout || failed || spins > (1u << 24)) {
      atomicAdd(status, 1u);
      atomicCAS(status + 1, 0u, (unsigned)bid + 1u);
#pragma unroll
      for (int s = 0; s < C; ++s) {
        const int64_t t = t0 + (int64_t)s;
        const bool nan = ((pend >> s) & 1u) || (force_timeout && t >= lo && t < hi);
        v[s] = nan ? 0x7FF8000000000000ull : v[s];
      }
      break;
    }
    __builtin_amdgcn_s_sleep(2);
#pragma unroll
    for (int s = 0; s < C; ++s) {
      const unsigned long long w = ((pend >> s) & 1u) ? ld(row + (t0 + (int64_t)s)) : v[s];
      v[s] = w;
      pend &= ~((w != kSentinel ? 1u : 0u) << s);
    }
  }
#pragma unroll
  for (int s = 0; s < C; ++s) out[s] = __longlong_as_double(v[s]);
}

// Logical block of this workgroup: the next ticket of the launch (forward: blocks in piece-height
// order, backward: the reverse).  A workgroup waits only on blocks of lower logical index, whose
// tickets were taken by workgroups already running or finished: no co-residency assumption.
// The block descriptor of logical block `bid`, forced into SGPRs (behind the ticket atomic the
// compiler cannot prove the descriptor unclobbered and would load it per lane).
__device__ __forceinline__ BlockDesc block_desc(const BlockDesc* blocks, int bid) {
  const BlockDesc d = blocks[bid];
  BlockDesc u;
  u.pos0 = __builtin_amdgcn_readfirstlane(d.pos0);
  u.nloc = __builtin_amdgcn_readfirstlane(d.nloc);
  u.virt0 = __builtin_amdgcn_readfirstlane(d.virt0);
  u.nvirt = __builtin_amdgcn_readfirstlane(d.nvirt);
  u.cout0 = __builtin_amdgcn_readfirstlane(d.cout0);
  u.ncout = __builtin_amdgcn_readfirstlane(d.ncout);
  u.dmax = __builtin_amdgcn_readfirstlane(d.dmax);
  u.nxl = __builtin_amdgcn_readfirstlane(d.nxl);
  u.xl0 = __builtin_amdgcn_readfirstlane(d.xl0);
  u.pad = 0;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(d.pre_dn & 0xffffffffu));
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)d.pre_dn >> 32));
  u.pre_dn = (int64_t)(((unsigned long long)hi << 32) | lo);
  return u;
}

// `slot` is a scratch LDS word that nothing else uses before the second barrier.
__device__ __forceinline__ int take_ticket(unsigned* status, int word, int nblocks, bool reverse, int* slot) {
  if (threadIdx.x == 0) {
    const int t = (int)atomicAdd(status + word, 1u);
    *slot = reverse ? nblocks - 1 - t : t;
  }
  __syncthreads();
  const int bid = __builtin_amdgcn_readfirstlane(*slot);
  __syncthreads();
  return bid;
}

// s_waitcnt vmcnt(0) (expcnt, lgkmcnt unconstrained), gfx9 encoding: an explicit wait the compiler's
// waitcnt pass sees (inline asm it would not)
constexpr unsigned kWaitVmcnt0 = 0x0F70;

// Kernel-argument constants in R (pre-rounded on the host, so they stay scalar operands).
// pin_pow: keep the fp64 constants of the correctly rounded pow in VGPRs (kernels that evaluate it).
// opq_inf: the clamps' infinity opaque to the compiler (rmaxc: one v_med3_f32 per clamp; the KR = 4 kernels)
template <typename R>
__device__ __forceinline__ Consts<R> consts_of(const RouteArgs& a, bool pin_pow = true, bool opq_inf = false);
template <>
__device__ __forceinline__ Consts<float> consts_of<float>(const RouteArgs& a, bool pin_pow, bool opq_inf) {
  return Consts<float>{a.cf[0], a.cf[1], a.cf[2], a.cf[3], a.cf[4], a.cf[5], a.cf[6], a.cf[7],
                       pin_pow ? pow_consts_vgpr() : pow_consts(), a.ln_dlb,
                       opq_inf ? opaque_inf(__builtin_inff()) : __builtin_inff()};
}
template <>
__device__ __forceinline__ Consts<double> consts_of<double>(const RouteArgs& a, bool, bool) {
  return Consts<double>{a.c[0], a.c[1], a.c[2], a.c[3], a.c[4], a.c[5], a.c[6], a.c[7], pow_consts(), a.ln_dlb};
}

template <typename R>
__device__ __forceinline__ ReachStatic<R> load_static(const RouteArgs& a, int ref) {
  const R* n = static_cast<const R*>(a.n);
  const R* q = static_cast<const R*>(a.q);
  const R* p = static_cast<const R*>(a.p);
  const R* L = static_cast<const R*>(a.L);
  const R* S = static_cast<const R*>(a.S);
  const R* X = static_cast<const R*>(a.X);
  return make_static<R>(n[ref], q[ref], p[(int64_t)ref * a.p_stride], S[ref], L[ref], X[ref]);
}

// Packed upstream descriptor: u0 (13 bits) | f1 (13 bits) << 13 | min(nup, 15) << 26; a missing
// upstream reads slot `none` (the forward's zero slot).  f1 is the second upstream's slot, or for a
// confluence (nup > 2) the offset of its list [c, u1, ..., u_{c-1}] in the block's LDS copy of
// xlist: every upstream index of a tick comes from registers or LDS, never from a global load (whose
// wait would also drain the tick's prefetches, in-order vmcnt).
__device__ __forceinline__ unsigned pack_up(const DevSchedule& s, int P, unsigned none = 0u) {
  const int b = s.upb[P], c = s.upc[P];
  const unsigned u0 = c > 0 ? (unsigned)s.uplist[b] : none;
  const unsigned u1 = c > 2 ? (unsigned)s.xoff[P] : (c > 1 ? (unsigned)s.uplist[b + 1] : none);
  return u0 | (u1 << 13) | ((unsigned)(c < 15 ? c : 15) << 26);
}
// Copy the block's confluence lists into LDS (all threads; the caller synchronises).
__device__ __forceinline__ void load_xlist(const DevSchedule& s, const BlockDesc& B, int* xl) {
  for (int i = threadIdx.x; i < B.nxl; i += blockDim.x) xl[i] = s.xlist[B.xl0 + i];
}
// A forward kernel's schedule words of internal position P (block B, S slots per buffer).
// off: the tick offset (low 16 bits: tick_off) | 1 + rank among the block's cut reaches (high 16: cut_rank,
// 0 = not cut; its boundary granule row is B.cout0 + rank, graph.cpp numbers cut edges that way).
// up: pack_up with the zero slot S - 1 for a missing upstream, which then adds exactly 0.
struct ReachWords {
  int ref, off;
  unsigned up;
};
__device__ __forceinline__ ReachWords reach_words(const DevSchedule& s, const BlockDesc& B, int P, int S) {
  ReachWords w;
  w.ref = s.ref[P];
  const int e = s.cut[P];
  w.off = s.off[P] | (e >= 0 ? (e - B.cout0 + 1) << 16 : 0);
  w.up = pack_up(s, P, (unsigned)(S - 1));
  return w;
}
__device__ __forceinline__ int tick_off(int off) { return off & 0xFFFF; }
__device__ __forceinline__ int cut_rank(int off) { return off >> 16; }
// Make a per-reach value opaque inside the tick loop so the compiler recomputes what it derives
// from it (64-bit addresses, qe + 1, ...) each tick instead of hoisting and keeping it live: at
// KR reaches per thread the hoisted copies, not the state, exhaust the register file.
template <typename V>
__device__ __forceinline__ V opq(V x) {
  asm volatile("" : "+v"(x));
  return x;
}
__device__ __forceinline__ int up_n(unsigned u) { return (int)(u >> 26); }
// 16-B runoff row segments (plain stores: measured faster than 8-B segments and than nt stores)
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
// a dL/drunoff group (each 16-B piece of a row is read once per launch; plain loads: nt measured slower)
__device__ __forceinline__ float4 load_grad4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void store4(double* p, double a, double b, double c, double d) {
  reinterpret_cast<double2*>(p)[0] = make_double2(a, b);
  reinterpret_cast<double2*>(p)[1] = make_double2(c, d);
}
__device__ __forceinline__ int up_0(unsigned u) { return (int)(u & 8191u); }
__device__ __forceinline__ int up_f1(unsigned u) { return (int)((u >> 13) & 8191u); }
// slot of the second upstream (a confluence's from its LDS list)
__device__ __forceinline__ int up_1(unsigned u, const int* xl) { return up_n(u) > 2 ? xl[up_f1(u) + 1] : up_f1(u); }

// The forward kernels' virtual inflows (x of another block's reach, through cut edge v_edge): virtual vi is
// imported and published by thread kBlockThreads - 1 - vi.  The owners sit in the last waves, which hold fewer
// wave-slices than wave 0 when nloc is not a multiple of the workgroup (the import's global round trip lands
// on the lighter waves); only the owner reads its ring entries [vi][kChunkFwd], so the import needs no
// workgroup barrier.
struct VirtOwner {
  int vi, v_off, v_edge;
  bool own;
  __device__ __forceinline__ VirtOwner(const DevSchedule& s, const BlockDesc& B)
      : vi(kBlockThreads - 1 - (int)threadIdx.x), v_off(0), v_edge(0), own(vi < B.nvirt) {
    if (own) {
      v_off = s.v_off[B.virt0 + vi];
      v_edge = s.v_edge[B.virt0 + vi];
    }
  }
  // The chunk of ticks [tau, tau + kChunkFwd) from the edge's granule row of `len` steps into the ring,
  // requested and waited for now, kImportBatch granules at a time (owners only)
  template <bool Sys>
  __device__ __forceinline__ void import_chunk(const double* row, int64_t len, int tau, double* ring, unsigned* status, int bid,
                                         bool force_timeout) const {
#pragma unroll
    for (int h = 0; h < kChunkFwd; h += kImportBatch) {
      double g[kImportBatch];
      wait_granules<kImportBatch, Sys>(row, (int64_t)tau - v_off + h, 0, len, g, status, bid, force_timeout);
#pragma unroll
      for (int i = 0; i < kImportBatch; ++i) ring[vi * kChunkFwd + h + i] = g[i];
    }
  }
  // tick tau's value from the ring into the virtual's slot of buffer `dst` (after the block's nloc reaches)
  template <typename Len>
  __device__ __forceinline__ void publish(int tau, Len len, const double* ring, double* dst, int nloc) const {
    if (own) {
      const int t = tau - v_off;
      if (t >= 0 && t < len) dst[nloc + vi] = ring[vi * kChunkFwd + (tau % kChunkFwd)];
    }
  }
};

// Debug per-workgroup profile (ddr_set_block_profile): start, end, import wait, hardware id.
// Layout per workgroup: kProfWords uint64 = start, end, wait, hwid, then a timestamp every 1024 ticks.
constexpr int kProfWords = 16;
__device__ __forceinline__ void prof_begin(unsigned long long* p, int bid) {
  p += kProfWords * bid;
  p[0] = __builtin_amdgcn_s_memrealtime();
  const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID
  const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
  p[3] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
}
__device__ __forceinline__ void prof_tick(unsigned long long* p, int bid, int tick) {
  if ((tick & 1023) == 0 && (tick >> 10) < kProfWords - 4)
    p[kProfWords * bid + 4 + (tick >> 10)] = __builtin_amdgcn_s_memrealtime();
}
__device__ __forceinline__ void prof_end(unsigned long long* p, int bid, unsigned long long wait) {
  p += kProfWords * bid;
  p[1] = __builtin_amdgcn_s_memrealtime();
  p[2] = wait;
}

// Debug phase profile (-DDDR_PHASE_PROF=1 builds only): every wave accumulates the s_memtime cycles of
// each tick phase; at the end lane 0 writes them after the per-block words of the profile buffer:
// prof[kProfWords * nblocks + (bid * 16 + wave) * kPhases + phase].
#ifndef DDR_PHASE_PROF
#define DDR_PHASE_PROF 0
#endif
struct PhaseProf {
#if DDR_PHASE_PROF
  static constexpr int kPhases = 8;
  unsigned long long acc[kPhases] = {};
  unsigned long long t0 = 0;
  __device__ __forceinline__ void start() { t0 = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void mark(int ph) {
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    acc[ph] += t - t0;
    t0 = t;
  }
  __device__ __forceinline__ void flush(unsigned long long* prof, int nblocks, int bid) {
    if (!prof || (threadIdx.x & 63)) return;
    unsigned long long* q = prof + (size_t)kProfWords * nblocks + ((size_t)bid * 16 + (threadIdx.x >> 6)) * kPhases;
    for (int i = 0; i < kPhases; ++i) q[i] = acc[i];
  }
#else
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void flush(unsigned long long*, int, int) {}
#endif
};

}  // namespace

// Per-reach statics in LDS, interleaved [slot][6] (n, qe, p, sqrtS, L, X): one get is three
// 2-element LDS reads at immediate offsets (lane stride 24 B: conflict-free).  The derived fields
// (dd, expo, 1/n) are recomputed on read (derive_static), or taken from registers (get_pre).
template <typename R>
struct StatTab {
  R* s;
  using V2 = typename std::conditional<sizeof(R) == 4, float2, double2>::type;
  __device__ __forceinline__ void put(int r, const ReachStatic<R>& v) const {
    R* q = s + 6 * r;
    q[0] = v.n;
    q[1] = v.qe;
    q[2] = v.p;
    q[3] = v.sqrtS;
    q[4] = v.L;
    q[5] = v.X;
  }
  template <bool Fast = false>
  __device__ __forceinline__ ReachStatic<R> get(int r) const {
    const V2* q = reinterpret_cast<const V2*>(s + 6 * r);
    const V2 a = q[0], b = q[1], c = q[2];
    return derive_static<R, Fast>(a.x, a.y, b.x, b.y, c.x, c.y);
  }
  __device__ __forceinline__ ReachStatic<R> get_pre(int r, R expo, R inv_n) const {
    const V2* q = reinterpret_cast<const V2*>(s + 6 * r);
    const V2 a = q[0], b = q[1], c = q[2];
    ReachStatic<R> v;
    v.n = a.x;
    v.qe = a.y;
    v.p = b.x;
    v.sqrtS = b.y;
    v.dd = (b.x * b.y) + R(1e-8);
    v.expo = expo;
    v.inv_n = inv_n;
    v.L = c.x;
    v.X = c.y;
    return v;
  }
};

// The gathered q' * flow_scale of local position r running step t = tau - off at forward tick tau:
// the tick-major schedule layout (row tau), or the row layout of a multi-hour store (choose_qs_layout).
template <typename R>
__device__ __forceinline__ const R* qs_at(const RouteArgs& a, const BlockDesc& B, int64_t xs_base, int tau, int off,
                                          int r) {
  const R* qs = static_cast<const R*>(a.qs);
  if (a.qs_rows > 0) {
    int t = tau - off;
    t = t < 0 ? 0 : (t >= (int)a.T ? (int)a.T - 1 : t);
    t = t > a.qp_shift ? t - a.qp_shift : 0;
    const unsigned row = __umulhi((unsigned)t, a.qp_magic);  // t / qp_hours
    return qs + (int64_t)a.qs_rows * B.pos0 + (int64_t)row * B.nloc + r;
  }
  return qs + xs_base + (int64_t)tau * B.nloc + r;
}


}  // namespace ddr
