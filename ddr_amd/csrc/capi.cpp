// C ABI of libddr_mc.so (include/ddr_mc.h).  No exception crosses this boundary; errors are
// returned as ddr_status codes with a thread-local message (ddr_last_error).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <string>

#include "internal.h"
#include "route_args.h"
#include "route_linear.h"
#include "metrics.h"
#include "objective.h"
#include "train.h"
#include "kan.h"
#include "geopredict.h"
#include "summedq.h"
#include "bmi.h"
#include "network.h"
#include "upstream.h"
#include "feed.h"
#include "attrs.h"
#include "period.h"
#include "summary.h"

namespace ddr {

namespace {
thread_local std::string g_last_error;
}

void set_error(const std::string& msg) { g_last_error = msg; }
ddr_status fail(ddr_status code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
const char* last_error_cstr() { return g_last_error.c_str(); }
ddr_status hip_fail(hipError_t e, const char* where) {
  g_last_error = std::string(where) + ": " + hipGetErrorString(e);
  return DDR_ERR_HIP;
}

}  // namespace ddr


using namespace ddr;

namespace {

// Measurement hooks (ddr_set_kernel_timing / ddr_set_block_profile): process-wide, not for
// concurrent use from several host threads.
struct KernelTiming {
  bool on = false;
  hipEvent_t ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  bool recorded[2] = {false, false};
} g_timing;
unsigned long long* g_prof[2] = {nullptr, nullptr};
int32_t g_debug = [] {  // ddr_set_debug_flags (DDR_NO_STEADY=1: the general tick path only, for A/B)
  auto on = [](const char* name) {
    const char* v = std::getenv(name);
    return v && v[0] == '1';
  };
  return (on("DDR_NO_STEADY") ? kFlagNoSteady : 0) | (on("DDR_NO_STORER") ? kFlagNoStorer : 0) |
         (on("DDR_NO_PLAIN") ? kFlagNoPlain : 0);
}();

// Hand-off failures surface without a host sync on the hot path: after every routing launch the
// status block's first words are copied (async, same stream) into a pinned slot with an event
// behind it.  Every later entry point polls the completed slots and returns DDR_ERR_TIMEOUT for
// a launch that timed out; ddr_status_check(1) waits for all of them.
struct PendingStatus {
  static constexpr int kSlots = 64;
  std::mutex mu;
  unsigned* host = nullptr;  // pinned, kSlots x 4 words
  hipEvent_t ev[kSlots] = {};
  const char* what[kSlots] = {};
  const void* graph[kSlots] = {};  // the launch's graph and stream, named in the error message
  hipStream_t stream[kSlots] = {};
  unsigned long long seq[kSlots] = {};
  unsigned long long launches = 0;  // routing launches enqueued by this process
  int head = 0;
  bool failed = false;
  std::string msg;

  void harvest(int k) {
    const unsigned* w = host + 4 * k;
    if (w[0] && !failed) {
      failed = true;
      char id[96];
      snprintf(id, sizeof(id), " (graph %p, stream %p, routing launch #%llu of this process)", graph[k],
               (void*)stream[k], seq[k]);
      // word 1: first failing logical block + 1, or 0x40000000 + rank for a split basin's peer that never
      // arrived at the launch's epoch hand-shake (split.hip: split_barrier_kernel)
      const std::string where = w[1] >= 0x40000000u
                                    ? "split-basin hand-shake: rank " + std::to_string((int)(w[1] - 0x40000000u)) +
                                          " never arrived"
                                    : "first logical block " + std::to_string((int)w[1] - 1);
      msg = std::to_string(w[0]) + " inter-workgroup hand-offs of a " + what[k] + " launch" + id + " timed out (" +
            where + "); its outputs hold NaN. Reported by the next library call: call ddr_status_check(1) at the "
            "end of a run so that a timeout in the last launch is not missed";
    }
    (void)hipEventDestroy(ev[k]);
    ev[k] = nullptr;
  }
  // caller holds mu
  void poll(bool wait) {
    for (int k = 0; k < kSlots; ++k) {
      if (!ev[k]) continue;
      if (wait) (void)hipEventSynchronize(ev[k]);
      if (hipEventQuery(ev[k]) == hipSuccess) harvest(k);
    }
  }
  ddr_status take_error() {
    if (!failed) return DDR_OK;
    failed = false;
    return fail(DDR_ERR_TIMEOUT, msg);
  }
  ddr_status enqueue(const void* status, hipStream_t s, const char* which, const void* g) {
    std::lock_guard<std::mutex> lk(mu);
    if (!host) DDR_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), sizeof(unsigned) * 4 * kSlots, hipHostMallocDefault));
    const int k = head;
    head = (head + 1) % kSlots;
    if (ev[k]) {
      (void)hipEventSynchronize(ev[k]);
      harvest(k);
    }
    DDR_HIP(hipMemcpyAsync(host + 4 * k, status, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    DDR_HIP(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
    what[k] = which;
    graph[k] = g;
    stream[k] = s;
    seq[k] = ++launches;
    DDR_HIP(hipEventRecord(ev[k], s));
    return DDR_OK;
  }
  ddr_status check(bool wait) {
    std::lock_guard<std::mutex> lk(mu);
    if (host) poll(wait);
    return take_error();
  }
} g_pending;

// Restores the calling thread's current device on scope exit (entry points that act on a graph's own
// device, which need not be the caller's current one)
struct DeviceGuard {
  int prev = -1;
  hipError_t error = hipSuccess;
  explicit DeviceGuard(int dev) {
    error = hipGetDevice(&prev);
    if (error == hipSuccess && prev != dev) error = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// DDR_FWD_CHECK_QPRIME: per host thread and device, the NaN word of its last checked forward, copied to
// pinned memory behind the q' gather, and the event after that copy (ddr_qprime_nan_wait waits for the
// gather only).  Keyed by device: an event belongs to the device current at its creation, so a thread
// routing on several GPUs records each launch's event on that launch's own device
constexpr int kNanDevices = 64;
struct NanCheck {
  unsigned* host = nullptr;
  hipEvent_t ev = nullptr;
  bool armed = false;
};
thread_local NanCheck t_nan[kNanDevices];
thread_local int t_nan_dev = -1;  // device of the calling thread's last checked forward

hipError_t nan_check_mark(const void* status, hipStream_t s) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= kNanDevices) return hipErrorInvalidDevice;
  NanCheck& c = t_nan[dev];
  if (!c.host) {
    e = hipHostMalloc(reinterpret_cast<void**>(&c.host), 16, hipHostMallocDefault);
    if (e != hipSuccess) return e;
  }
  if (!c.ev) {
    e = hipEventCreateWithFlags(&c.ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  e = hipMemcpyAsync(c.host, static_cast<const unsigned*>(status) + kStatusNaN, sizeof(unsigned),
                     hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) return e;
  if (t_nan_dev >= 0) t_nan[t_nan_dev].armed = false;  // "the last checked forward" is this one
  c.armed = true;
  t_nan_dev = dev;
  return hipEventRecord(c.ev, s);
}

// Stream capture (a hipGraph of a whole training step, e.g. torch.cuda.graph): the launches are recorded and
// replayed later, so the host-side bookkeeping of a launch -- the status harvest (a D2H copy and an event per
// launch, polled by later calls), the kernel timers, the wait for the graph's upload event (recorded outside
// the capture: capture a step only after the graph has been used once) -- is skipped while the stream
// captures.  A timed-out hand-off inside a replayed step still writes NaN into its outputs.
bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
// Order `s` after the graph's build.  A capture cannot wait on the upload event (recorded outside it), so a
// device- or stream-built graph whose completion no launch outside a capture has waited for yet is refused
// there: its first replay could read a half-uploaded schedule.
ddr_status ready_for(const Graph* g, hipStream_t s) {
  if (capturing(s)) {
    if (g->ready && !g->ready_waited.load(std::memory_order_acquire))
      return fail(DDR_ERR_ARG, "graph used inside a stream capture before any launch outside it waited for its build: "
                               "route with it once outside the capture first");
    return DDR_OK;
  }
  DDR_HIP(graph_ready(g, s));
  g->ready_waited.store(true, std::memory_order_release);
  return DDR_OK;
}
#define DDR_TRY(call)                   \
  do {                                  \
    const ddr_status _st = (call);      \
    if (_st != DDR_OK) return _st;      \
  } while (0)

hipError_t timing_mark(int which, int edge, hipStream_t s) {
  if (!g_timing.on || capturing(s)) return hipSuccess;
  hipEvent_t& e = g_timing.ev[which][edge];
  if (!e) {
    hipError_t r = hipEventCreate(&e);
    if (r != hipSuccess) return r;
  }
  if (edge == 1) g_timing.recorded[which] = true;
  return hipEventRecord(e, s);
}

template <typename R>
ddr_status check_common(const ddr_graph* gh, const ddr_mc_consts* c, const ddr_mc_reaches* r, int64_t T) {
  if (!gh || !c || !r) return fail(DDR_ERR_ARG, "null graph/consts/reaches");
  if (T < 1) return fail(DDR_ERR_ARG, "T must be >= 1");
  if (!r->n || !r->q_spatial || !r->p_spatial || !r->length || !r->slope || !r->x_storage)
    return fail(DDR_ERR_ARG, "null per-reach input");
  if (r->p_stride != 0 && r->p_stride != 1) return fail(DDR_ERR_ARG, "p_stride must be 0 or 1");
  if (r->qprime_hours < 0 || r->qprime_hours > (int64_t(1) << 20)) return fail(DDR_ERR_ARG, "bad qprime_hours");
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (!g->uploaded) return fail(DDR_ERR_ARG, "graph was built host-only: upload it first (ddr_graph_upload)");
  if (T * (g->n + 1) > (int64_t(1) << 62)) return fail(DDR_ERR_ARG, "T * N overflows");
  return DDR_OK;
}

template <typename R>
void fill_common(RouteArgs& a, const Graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r, int64_t T,
                 const R* qprime, int32_t flags) {
  std::memset(&a, 0, sizeof(a));
  a.s = g->dev;
  a.N = g->n;
  a.T = T;
  a.flags = flags;
  a.p_stride = (int32_t)r->p_stride;
  a.n = r->n;
  a.q = r->q_spatial;
  a.p = r->p_spatial;
  a.L = r->length;
  a.S = r->slope;
  a.X = r->x_storage;
  a.fs = r->flow_scale;
  a.qp_hours = r->qprime_hours > 1 ? (int32_t)r->qprime_hours : 1;
  a.qp_shift = (flags & DDR_FWD_ACCUMULATE) ? 0 : 1;
  a.qp_valid = r->qprime_valid;
  choose_qs_layout(a);  // needs T, qp_hours, qp_shift
  a.qprime = qprime;
  a.c[0] = c->dt;
  a.c[1] = c->discharge_lb;
  a.c[2] = c->velocity_lb;
  a.c[3] = c->velocity_ub;
  a.c[4] = c->depth_lb;
  a.c[5] = c->bottom_width_lb;
  a.c[6] = c->side_slope_lb;
  a.c[7] = c->side_slope_ub;
  for (int i = 0; i < 8; ++i) a.cf[i] = (float)a.c[i];
  a.ln_dlb = std::log(sizeof(R) == 4 ? (double)a.cf[4] : a.c[4]);
}

// The routing kernels need no co-residency (ticket-ordered blocks, route_device.h), only that one
// workgroup fits a CU with the schedule's LDS.
template <typename R>
ddr_status check_launchable(const Graph* g, bool backward) {
  const int cap = backward ? backward_resident_blocks<R>(g) : forward_resident_blocks<R>(g);
  if (cap < 0) return fail(DDR_ERR_HIP, "occupancy query failed");
  if (cap == 0)
    return fail(DDR_ERR_CAPACITY, std::string("the ") + (backward ? "backward" : "forward") +
                                      " routing kernel does not fit a CU at this schedule's LDS size" +
                                      (sizeof(R) == 8 ? " (fp64: use a smaller max_block_reaches)" : ""));
  return DDR_OK;
}

// Split basin (SplitState): the launch's split arguments, its receive rows reset, and the epoch hand-shake
// with the other ranks of the split (slot 0: forward, 1: backward), all stream-ordered before the launch.
ddr_status split_prepare(const Graph* g, RouteArgs& a, int64_t T, int slot, hipStream_t s) {
  SplitState& sp = const_cast<Graph*>(g)->split;
  if (sp.nranks == 0) return DDR_OK;
  if (T > sp.t_cap) return fail(DDR_ERR_ARG, "split basin: T exceeds the receive rows' capacity (ddr_graph_set_split t_cap)");
  a.owned = sp.owned;
  a.xid = sp.xid;
  a.xcons = sp.xcons;
  a.xprod = sp.xprod;
  a.xedge = sp.xedge;
  a.xrank = sp.rank;
  auto rows = [&](char* base, int which) {
    double* f = reinterpret_cast<double*>(base + xmem_flags_bytes());
    return which == 0 ? f : f + sp.n_x * T;
  };
  a.xfwd = rows(sp.local, 0);
  a.xbwd = rows(sp.local, 1);
  SplitBarrierArgs b;
  std::memset(&b, 0, sizeof(b));
  for (int p = 0; p < sp.nranks; ++p) {
    a.pxfwd[p] = rows(sp.peers[p], 0);
    a.pxbwd[p] = rows(sp.peers[p], 1);
    b.peer[p] = reinterpret_cast<unsigned long long*>(sp.peers[p]);
  }
  if (sp.n_x > 0) {
    double* mine = slot == 0 ? a.xfwd : a.xbwd;
    DDR_HIP(hipMemsetAsync(mine, 0xFF, sizeof(double) * (size_t)(sp.n_x * T) * (slot == 0 ? 1 : 2), s));
  }
  b.mine = reinterpret_cast<unsigned long long*>(sp.local);
  b.rank = sp.rank;
  b.nranks = sp.nranks;
  b.slot = slot;
  b.epoch = ++sp.epoch[slot];
  b.status = a.status;
  DDR_HIP(launch_split_barrier(b, s));
  return DDR_OK;
}

template <typename R>
ddr_status forward_impl(const ddr_graph* gh, const ddr_mc_consts* c, const ddr_mc_reaches* r, const R* qprime,
                        int64_t T, const R* q0, R* runoff, R* x_save, double* bnd, void* status, R* q_last,
                        R* tw, R* ss, int32_t flags, void* stream) {
  ddr_status st = check_common<R>(gh, c, r, T);
  if (st) return st;
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (!qprime) return fail(DDR_ERR_ARG, "null qprime");
  if ((flags & DDR_FWD_CARRY) && !q0) return fail(DDR_ERR_ARG, "DDR_FWD_CARRY needs q0");
  if ((flags & DDR_FWD_CARRY) && (flags & DDR_FWD_ACCUMULATE))
    return fail(DDR_ERR_ARG, "DDR_FWD_ACCUMULATE has no carried state");
  if (!x_save) return fail(DDR_ERR_ARG, "x_save is required (routing state, and the staging of runoff)");
  if (g->n_cut > 0 && !bnd) return fail(DDR_ERR_ARG, "graph has cut edges: bnd buffer required");
  if (!status) return fail(DDR_ERR_ARG, "null status block");
  // a split basin's launches hand-shake per launch epoch with every peer: a launch only this rank makes
  // (a hot start, the daily accumulation) would leave the epochs of all later launches off by one
  if (g->split.nranks > 0 && (T < 2 || (flags & DDR_FWD_ACCUMULATE)))
    return fail(DDR_ERR_ARG, "split basin: hot-start (T = 1) and accumulation launches are not supported");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool cap = capturing(s);
  if (cap && (g->split.nranks > 0 || (flags & DDR_FWD_CHECK_QPRIME)))
    return fail(DDR_ERR_ARG, "stream capture: split-basin launches and the q' NaN check cannot be captured");
  if (!cap && (st = g_pending.check(false))) return st;
  if ((st = check_launchable<R>(g, false))) return st;
  DDR_TRY(ready_for(g, s));
  DDR_HIP(hipMemsetAsync(status, 0, kStatusBytes, s));
  if (g->n_cut > 0) DDR_HIP(hipMemsetAsync(bnd, 0xFF, sizeof(double) * g->n_cut * T, s));
  RouteArgs a;
  fill_common<R>(a, g, c, r, T, qprime, flags | g_debug);
  a.q0 = q0;
  a.runoff = (flags & DDR_FWD_NO_RUNOFF) ? nullptr : runoff;
  a.x_save = x_save;
  a.bnd = bnd;
  a.status = static_cast<unsigned*>(status);
  a.q_last = q_last;
  a.tw_last = tw;
  a.ss_last = ss;
  a.prof = g_prof[0];
  a.qs = x_save + (g->n * T + g->sum_dn);
  if ((st = split_prepare(g, a, T, 0, s))) return st;
  DDR_HIP(launch_gather_qprime<R>(g, a, s));
  if (flags & DDR_FWD_CHECK_QPRIME) DDR_HIP(nan_check_mark(status, s));
  DDR_HIP(timing_mark(0, 0, s));
  DDR_HIP(launch_route_forward<R>(g, a, s));
  DDR_HIP(timing_mark(0, 1, s));
  DDR_HIP(launch_split_finish<R>(g, a, s));
  // runoff (N, T) is written by the routing kernel itself (16-B row segments every 4 steps)
  return cap ? DDR_OK : g_pending.enqueue(status, s, "forward", gh);
}

template <typename R>
ddr_status gauge_args(const ddr_graph* gh, const R* x_save, int64_t T, const ddr_gauges* gz, double qlb,
                      int32_t flags, GaugeArgs& a);

// Workspace of the state-gradient backward: dL/d(q' * flow_scale) in the schedule layout, then one
// byte per gauge (the t = 0 clamp mask).
int64_t state_work_bytes(const Graph* g, int64_t T, int64_t n_gauges, size_t rsize) {
  return (int64_t)align16(rsize * (size_t)(g->n * T + g->sum_dn)) + n_gauges;
}

template <typename R>
ddr_status backward_impl(const ddr_graph* gh, const ddr_mc_consts* c, const ddr_mc_reaches* r, const R* qprime,
                         int64_t T, const R* x_save, const double* bnd, const R* grad, const ddr_gauges* gauges,
                         double* bwd_bnd, void* status, R* gn, R* gq, R* gp, int32_t flags, void* stream,
                         int64_t qp_rows = 0, R* gqp = nullptr, R* gq0 = nullptr, void* work = nullptr,
                         const R* seed = nullptr) {
  ddr_status st = check_common<R>(gh, c, r, T);
  if (st) return st;
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (!qprime || !x_save || !grad || !gn || !gq || !gp || !status)
    return fail(DDR_ERR_ARG, "null backward argument");
  if (g->n_cut > 0 && !bnd) return fail(DDR_ERR_ARG, "graph has cut edges: forward boundary buffer required");
  if (!bwd_bnd) return fail(DDR_ERR_ARG, "backward workspace required");
  if (flags & DDR_FWD_ACCUMULATE) return fail(DDR_ERR_ARG, "DDR_FWD_ACCUMULATE launches have no adjoint");
  if (gauges && (!gauges->reach_offsets || !gauges->reach_gauges))
    return fail(DDR_ERR_ARG, "gauge mode backward needs the reach->gauge map");
  if (g->split.nranks > 0 && (gauges || gqp || gq0))
    return fail(DDR_ERR_ARG, "split basin: gauge mode and state gradients are not supported");
  const bool state = gqp || gq0;
  if (state) {
    if (!work) return fail(DDR_ERR_ARG, "state gradients need the workspace (ddr_state_work_bytes)");
    if (gq0 && !(flags & DDR_FWD_CARRY)) return fail(DDR_ERR_ARG, "grad_q0 needs a carried-state forward (DDR_FWD_CARRY)");
    if (gqp && qp_rows < (T + std::max<int64_t>(1, r->qprime_hours) - 1) / std::max<int64_t>(1, r->qprime_hours))
      return fail(DDR_ERR_ARG, "grad_qprime has fewer rows than the window reads");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool cap = capturing(s);
  if (cap && g->split.nranks > 0) return fail(DDR_ERR_ARG, "stream capture: split-basin launches cannot be captured");
  if (!cap && (st = g_pending.check(false))) return st;
  if ((st = check_launchable<R>(g, true))) return st;
  DDR_TRY(ready_for(g, s));
  DDR_HIP(hipMemsetAsync(status, 0, kStatusBytes, s));
  if (g->n_cut > 0) DDR_HIP(hipMemsetAsync(bwd_bnd, 0xFF, sizeof(double) * 2 * g->n_cut * T, s));
  DDR_HIP(hipMemsetAsync(bwd_bnd + 2 * g->n_cut * T, 0, sizeof(double) * 3 * g->n, s));
  RouteArgs a;
  fill_common<R>(a, g, c, r, T, qprime, flags | g_debug);
  a.x_save = const_cast<R*>(x_save);
  a.qs = const_cast<R*>(x_save) + (g->n * T + g->sum_dn);
  a.bnd = const_cast<double*>(bnd);
  a.status = static_cast<unsigned*>(status);
  a.grad_out = grad;
  a.g_roff = gauges ? gauges->reach_offsets : nullptr;
  a.g_rg = gauges ? gauges->reach_gauges : nullptr;
  a.gseed = seed;
  a.bwd_bnd = bwd_bnd;
  a.gn = gn;
  a.gq = gq;
  a.gp = gp;
  // workspace: [2 n_cut T f64 boundary][3 N f64 accumulators]; the kernel reads grad (N, T) itself
  a.prof = g_prof[1];
  if (state) {
    a.gqs = work;
    a.gq0 = gq0;
    if (gauges && gauges->n_gauges > 0) {
      // the gauge sums' clamp at t = 0 (mmc.py:398-412) gates dL/dout[:, 0]
      GaugeArgs ga;
      if ((st = gauge_args<R>(gh, x_save, T, gauges, c->discharge_lb, flags, ga))) return st;
      unsigned char* mask = static_cast<unsigned char*>(work) + align16(sizeof(R) * (size_t)(g->n * T + g->sum_dn));
      DDR_HIP(launch_gauge_mask0<R>(ga, x_save, mask, s));
      a.gmask0 = mask;
    }
  }
  if ((st = split_prepare(g, a, T, 1, s))) return st;
  DDR_HIP(timing_mark(1, 0, s));
  DDR_HIP(launch_route_backward<R>(g, a, s));
  DDR_HIP(timing_mark(1, 1, s));
  if (gqp) DDR_HIP(launch_scatter_qprime_grad<R>(g, a, qp_rows, gqp, s));
  return cap ? DDR_OK : g_pending.enqueue(status, s, "backward", gh);
}

template <typename R>
ddr_status gauge_args(const ddr_graph* gh, const R* x_save, int64_t T, const ddr_gauges* gz, double qlb,
                      int32_t flags, GaugeArgs& a) {
  if (!gh || !x_save || !gz || T < 1) return fail(DDR_ERR_ARG, "bad gauge arguments");
  if (gz->n_gauges > 0 && (!gz->offsets || !gz->index)) return fail(DDR_ERR_ARG, "null gauge arrays");
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (!g->uploaded) return fail(DDR_ERR_ARG, "graph was built host-only: upload it first (ddr_graph_upload)");
  // a split rank holds the states of its own blocks only: a gauge sum would read rows no launch wrote
  if (g->split.nranks > 0) return fail(DDR_ERR_ARG, "split basin: gauge mode is not supported");
  std::memset(&a, 0, sizeof(a));
  a.s = g->dev;
  a.T = T;
  a.G = gz->n_gauges;
  a.goff = gz->offsets;
  a.gidx = gz->index;
  a.pos_of_ref = g->dev.pos_of_ref;
  a.block_of_pos = g->dev.block_of_pos;
  a.qlb = qlb;
  a.carry = (flags & DDR_FWD_CARRY) ? 1 : 0;
  return DDR_OK;
}

template <typename R>
ddr_status gauge_impl(const ddr_graph* gh, const R* x_save, int64_t T, const ddr_gauges* gz, double qlb,
                      int32_t flags, R* out, void* stream) {
  GaugeArgs a;
  ddr_status st = gauge_args<R>(gh, x_save, T, gz, qlb, flags, a);
  if (st) return st;
  if (!out) return fail(DDR_ERR_ARG, "null gauge output");
  DDR_TRY(ready_for(reinterpret_cast<const Graph*>(gh), static_cast<hipStream_t>(stream)));
  DDR_HIP(launch_gauge<R>(a, x_save, out, static_cast<hipStream_t>(stream)));
  return DDR_OK;
}

ddr_status check_window(int64_t T, int64_t t0, int64_t L, int64_t D) {
  if (t0 < 0 || L < 1 || t0 + L > T || D < 1 || D > L)
    return fail(DDR_ERR_ARG, "daily window must satisfy 0 <= t0, t0 + L <= T, 1 <= D <= L");
  return DDR_OK;
}

template <typename R>
ddr_status gauge_daily_impl(const ddr_graph* gh, const R* x_save, int64_t T, const ddr_gauges* gz, double qlb,
                            int32_t flags, int64_t t0, int64_t L, int64_t D, R* out, void* stream) {
  GaugeArgs a;
  ddr_status st = gauge_args<R>(gh, x_save, T, gz, qlb, flags, a);
  if (st) return st;
  if ((st = check_window(T, t0, L, D))) return st;
  if (!out) return fail(DDR_ERR_ARG, "null daily output");
  DDR_TRY(ready_for(reinterpret_cast<const Graph*>(gh), static_cast<hipStream_t>(stream)));
  DDR_HIP(launch_gauge_daily<R>(a, x_save, t0, L, D, out, static_cast<hipStream_t>(stream)));
  return DDR_OK;
}

template <typename R>
ddr_status gauge_daily_seed_impl(int64_t G, int64_t T, int64_t t0, int64_t L, int64_t D, const R* gd, R* gh,
                                 void* stream) {
  ddr_status st = check_window(T, t0, L, D);
  if (st) return st;
  if (G < 0 || (G > 0 && (!gd || !gh))) return fail(DDR_ERR_ARG, "bad daily seed arguments");
  DDR_HIP(launch_gauge_daily_seed<R>(G, T, t0, L, D, gd, gh, static_cast<hipStream_t>(stream)));
  return DDR_OK;
}

// One routing launch's share of a period's daily series (period.hip).  gz == nullptr: every reach.
template <typename R>
ddr_status period_daily_impl(const ddr_graph* gh, const R* x_save, int64_t T, const ddr_gauges* gz, double qlb,
                             int32_t flags, int64_t h0, int64_t first_hour, int64_t n_days, R* out, void* stream) {
  if (!gh) return fail(DDR_ERR_ARG, "period daily: null graph");
  if (!x_save) return fail(DDR_ERR_ARG, "period daily: null x_save");
  if (!out) return fail(DDR_ERR_ARG, "period daily: null daily output");
  if (T < 1) return fail(DDR_ERR_ARG, "period daily: T must be at least 1");
  if (h0 < 0 || first_hour < 0) return fail(DDR_ERR_ARG, "period daily: h0 and first_hour must not be negative");
  if (n_days < 1) return fail(DDR_ERR_ARG, "period daily: n_days must be at least 1");
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (!g->uploaded) return fail(DDR_ERR_ARG, "graph was built host-only: upload it first (ddr_graph_upload)");
  // a split rank holds the states of its own blocks only: the other rows would be read unwritten
  if (g->split.nranks > 0) return fail(DDR_ERR_ARG, "split basin: period inference is not supported");
  PeriodArgs p;
  p.T = T;
  p.D = n_days;
  p.h0 = h0;
  p.first_hour = first_hour;
  p.qlb = qlb;
  period_days(T, n_days, h0, first_hour, &p.d_lo, &p.nd);
  if (gz && gz->n_gauges > 0 && (!gz->offsets || !gz->index)) return fail(DDR_ERR_ARG, "null gauge arrays");
  if (p.nd == 0) return DDR_OK;  // no day's window meets this launch
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (gz) {
    GaugeArgs a;
    ddr_status st = gauge_args<R>(gh, x_save, T, gz, qlb, flags, a);
    if (st) return st;
    DDR_TRY(ready_for(g, s));
    DDR_HIP(launch_period_gauge<R>(a, p, x_save, out, s));
  } else {
    DDR_TRY(ready_for(g, s));
    DDR_HIP(launch_period_all<R>(g, p, (flags & DDR_PERIOD_DIRECT_STORE) != 0, x_save, out, s));
  }
  return DDR_OK;
}

}  // namespace

#define DDR_GUARD(body)                                  \
  try {                                                  \
    body                                                 \
  } catch (const std::exception& ex) {                   \
    return fail(DDR_ERR_ARG, std::string("internal: ") + ex.what()); \
  } catch (...) {                                        \
    return fail(DDR_ERR_ARG, "internal error");          \
  }

ddr_status pnet_forward_impl(int64_t n_rows, int32_t n_features, const float* x, const float* params,
                             const float* denorm, float* z_save, float* u_save, float* out_n, float* out_q,
                             float* out_p, void* stream) {
  if (n_rows < 0 || n_features < 1 || n_features > 12) return fail(DDR_ERR_ARG, "pnet: 0 <= rows, 1 <= features <= 12");
  if (n_rows > 0 && (!x || !params || !denorm || !z_save || !u_save || !out_n || !out_q || !out_p))
    return fail(DDR_ERR_ARG, "pnet: null argument");
  if (n_rows >= (int64_t(1) << 31) / 64 * 64) return fail(DDR_ERR_ARG, "pnet: too many rows");
  float* out[3] = {out_n, out_q, out_p};
  DDR_HIP(launch_pnet_forward(n_rows, n_features, x, params, denorm, z_save, u_save, out, static_cast<hipStream_t>(stream)));
  return DDR_OK;
}
ddr_status pnet_backward_impl(int64_t n_rows, int32_t n_features, const float* x, const float* params,
                              const float* denorm, const float* z_save, const float* u_save, const float* grad_n,
                              const float* grad_q, const float* grad_p, float* grad_params, void* work, void* stream) {
  if (n_rows < 0 || n_features < 1 || n_features > 12) return fail(DDR_ERR_ARG, "pnet: 0 <= rows, 1 <= features <= 12");
  if (!grad_params || !params || !denorm) return fail(DDR_ERR_ARG, "pnet: null argument");
  if (n_rows > 0 && (!x || !z_save || !u_save || !grad_n || !grad_q || !grad_p || !work))
    return fail(DDR_ERR_ARG, "pnet: null argument");
  if (n_rows >= (int64_t(1) << 31) / 64 * 64) return fail(DDR_ERR_ARG, "pnet: too many rows");
  const float* g[3] = {grad_n, grad_q, grad_p};
  DDR_HIP(launch_pnet_backward(n_rows, n_features, x, params, denorm, z_save, u_save, g, grad_params, work,
                               static_cast<hipStream_t>(stream)));
  return DDR_OK;
}

// kan.hip: descriptor and pointer checks of the KAN entry points (the envelope itself: kan_validate, kan.h)
ddr_status kan_check(const ddr_kan_desc* desc, int64_t n_rows) {
  const std::string why = kan_validate(desc);
  if (!why.empty()) return fail(DDR_ERR_ARG, why);
  if (n_rows < 1 || n_rows > (int64_t(1) << 30)) return fail(DDR_ERR_ARG, "kan: 1 <= rows <= 2^30");
  return DDR_OK;
}
ddr_status kan_forward_impl(const ddr_kan_desc* desc, int64_t n_rows, const float* x, const float* params,
                            const float* consts, float* h_save, float* u, void* work, void* stream) {
  ddr_status st = kan_check(desc, n_rows);
  if (st) return st;
  if (!x || !params || !consts || !u) return fail(DDR_ERR_ARG, "kan: null argument");
  if (!h_save && desc->n_layers > 1 && !work) return fail(DDR_ERR_ARG, "kan: work is needed when nothing is saved");
  DDR_HIP(launch_kan_forward(*desc, n_rows, x, params, consts, h_save, u, work, static_cast<hipStream_t>(stream)));
  return DDR_OK;
}
ddr_status kan_backward_impl(const ddr_kan_desc* desc, int64_t n_rows, const float* x, const float* params,
                             const float* consts, const float* h_save, const float* u, const float* grad_u,
                             float* grad_params, void* work, void* stream) {
  ddr_status st = kan_check(desc, n_rows);
  if (st) return st;
  if (!x || !params || !consts || !h_save || !u || !grad_u || !grad_params || !work)
    return fail(DDR_ERR_ARG, "kan: null argument");
  DDR_HIP(launch_kan_backward(*desc, n_rows, x, params, consts, h_save, u, grad_u, grad_params, work,
                              static_cast<hipStream_t>(stream)));
  return DDR_OK;
}

// geopredict.hip: the geometry predictor's two launches
ddr_status attr_prepare_impl(int64_t n_rows, int32_t n_features, const float* raw, int64_t feat_stride,
                             const double* scale, const double* offset, const int32_t* log10_flag, const float* mean,
                             const float* std, const float* p10, const float* p90, float* x, int64_t* counts,
                             void* stream) {
  if (n_rows < 0 || feat_stride < 0) return fail(DDR_ERR_ARG, "attr_prepare: negative size");
  if (n_features < 1 || n_features > kGeoMaxF)
    return fail(DDR_ERR_ARG, "attr_prepare: 1 <= n_features <= " + std::to_string(kGeoMaxF) + " (got " +
                                 std::to_string(n_features) + ")");
  if (n_rows == 0) return DDR_OK;
  if (n_rows > kGeoMaxRows) return fail(DDR_ERR_ARG, "attr_prepare: too many rows");
  if (feat_stride < n_rows && n_features > 1)
    return fail(DDR_ERR_ARG, "attr_prepare: feat_stride is shorter than a column");
  if (!raw || !scale || !offset || !log10_flag || !mean || !std || !x)
    return fail(DDR_ERR_ARG, "attr_prepare: null argument");
  if ((p10 == nullptr) != (p90 == nullptr)) return fail(DDR_ERR_ARG, "attr_prepare: p10 and p90 go together");
  if (p10 && !counts) return fail(DDR_ERR_ARG, "attr_prepare: null counts with p10 / p90");
  DDR_HIP(launch_attr_prepare(n_rows, n_features, raw, feat_stride, scale, offset, log10_flag, mean, std, p10, p90,
                              x, reinterpret_cast<long long*>(counts), static_cast<hipStream_t>(stream)));
  return DDR_OK;
}
// denormalize's scalars as torch holds them (routing/utils.py:177-185: fp32 tensors of bounds[0] + 1e-6 and
// bounds[1], their fp32 logs, and Python-double differences rounded when they meet the fp32 tensor)
GeoSlot geom_slot(const ddr_geom_slot& s) {
  GeoSlot g{s.column, s.log_space, 0.0f, 0.0f, (float)s.value};
  if (s.log_space) {
    const float log_lo = std::log((float)(s.lo + 1e-6)), log_hi = std::log((float)s.hi);
    g.a = log_hi - log_lo;
    g.b = log_lo;
  } else {
    g.a = (float)(s.hi - s.lo);
    g.b = (float)s.lo;
  }
  return g;
}
ddr_status geometry_predict_impl(int64_t n_rows, int32_t n_outputs, const float* u, const ddr_geom_slot* slot_n,
                                 const ddr_geom_slot* slot_q, const ddr_geom_slot* slot_p, const float* discharge,
                                 const float* slope, double discharge_lb, double slope_lb, double depth_lb,
                                 double bottom_width_lb, float* out, int64_t out_stride, void* stream) {
  if (n_rows < 0 || out_stride < 0) return fail(DDR_ERR_ARG, "geometry_predict: negative size");
  if (n_outputs < 1 || n_outputs > kKanMaxO)
    return fail(DDR_ERR_ARG, "geometry_predict: 1 <= n_outputs <= " + std::to_string(kKanMaxO) + " (got " +
                                 std::to_string(n_outputs) + ")");
  if (!slot_n || !slot_q || !slot_p) return fail(DDR_ERR_ARG, "geometry_predict: null slot");
  const ddr_geom_slot* slots[3] = {slot_n, slot_q, slot_p};
  const char* names[3] = {"n", "q_spatial", "p_spatial"};
  for (int k = 0; k < 3; ++k) {
    if (slots[k]->column >= n_outputs || slots[k]->column < -1)
      return fail(DDR_ERR_ARG, std::string("geometry_predict: the column of ") + names[k] + " is outside u (" +
                                   std::to_string(slots[k]->column) + " of " + std::to_string(n_outputs) + ")");
    if (k < 2 && slots[k]->column < 0)
      return fail(DDR_ERR_ARG, std::string("geometry_predict: ") + names[k] + " has no default: it needs a column of u");
  }
  if (n_rows == 0) return DDR_OK;
  if (n_rows > kGeoMaxRows) return fail(DDR_ERR_ARG, "geometry_predict: too many rows");
  if (!u || !out) return fail(DDR_ERR_ARG, "geometry_predict: null argument");
  if ((discharge == nullptr) != (slope == nullptr))
    return fail(DDR_ERR_ARG, "geometry_predict: null discharge or slope (both NULL: parameters only)");
  if (out_stride < n_rows) return fail(DDR_ERR_ARG, "geometry_predict: out_stride is shorter than a row");
  const GeoSlot gs[3] = {geom_slot(*slot_n), geom_slot(*slot_q), geom_slot(*slot_p)};
  DDR_HIP(launch_geometry_predict(n_rows, n_outputs, u, gs, discharge, slope, (float)discharge_lb, (float)slope_lb,
                                  (float)depth_lb, (float)bottom_width_lb, out, out_stride,
                                  static_cast<hipStream_t>(stream)));
  return DDR_OK;
}

ddr_status daily_l1_impl(int64_t n_gauges, int64_t n_days, int64_t warmup, const float* daily, const float* obs,
                         float inv_count, float* loss, float* grad, void* stream) {
  if (n_gauges < 0 || n_days < 0 || warmup < 0) return fail(DDR_ERR_ARG, "daily_l1: negative size");
  if (!loss || (n_gauges * n_days > 0 && (!daily || !obs))) return fail(DDR_ERR_ARG, "daily_l1: null argument");
  DDR_HIP(launch_daily_l1(n_gauges, n_days, warmup, daily, obs, inv_count, loss, grad, static_cast<hipStream_t>(stream)));
  return DDR_OK;
}
ddr_status metrics_impl(int64_t n_gauges, int64_t n_days, const float* pred, int64_t pred_stride, const float* target,
                        int64_t target_stride, double* out, int32_t* pred_nan_count, void* stream) {
  if (n_gauges < 0 || n_days < 0 || pred_stride < 0 || target_stride < 0)
    return fail(DDR_ERR_ARG, "metrics: negative size");
  if (n_gauges == 0) return DDR_OK;
  if (n_days < 1 || n_days > kMetricsMaxDays)
    return fail(DDR_ERR_ARG, "metrics: 1 <= n_days <= " + std::to_string(kMetricsMaxDays) + " (got " +
                                 std::to_string(n_days) + ")");
  if (n_gauges > INT32_MAX) return fail(DDR_ERR_ARG, "metrics: too many gauges");
  if (!pred || !target || !out || !pred_nan_count) return fail(DDR_ERR_ARG, "metrics: null argument");
  DDR_HIP(launch_metrics(n_gauges, n_days, pred, pred_stride, target, target_stride, out, pred_nan_count,
                         static_cast<hipStream_t>(stream)));
  return DDR_OK;
}
static_assert(kSummaryTile == DDR_SUMMARY_TILE && kSummaryMaxQ == DDR_SUMMARY_MAX_Q, "summary.h and ddr_mc.h disagree");
template <typename T>
ddr_status summary_impl(int64_t R, int64_t N, const T* x, int64_t row_stride, int32_t K, const double* q,
                        int32_t method, int32_t flags, double* out, void* work, void* stream) {
  if (R < 0 || N < 0 || row_stride < 0 || K < 0) return fail(DDR_ERR_ARG, "summary: negative size");
  if (K > kSummaryMaxQ)
    return fail(DDR_ERR_ARG, "summary: at most " + std::to_string(kSummaryMaxQ) + " quantiles per call (got " +
                                 std::to_string(K) + ")");
  if (method < 0 || method >= DDR_N_SUMMARY_METHODS)
    return fail(DDR_ERR_ARG, "summary: unknown method " + std::to_string(method));
  if (flags & ~DDR_SUMMARY_SKIP_INF) return fail(DDR_ERR_ARG, "summary: unknown flag in " + std::to_string(flags));
  if (K > 0 && !q) return fail(DDR_ERR_ARG, "summary: null q");
  SummaryArgs a{};
  for (int k = 0; k < K; ++k) {
    if (!(q[k] >= 0.0 && q[k] <= 1.0))
      return fail(DDR_ERR_ARG, "summary: q[" + std::to_string(k) + "] is outside [0, 1]");
    a.q[k] = q[k];
  }
  if (R == 0) return DDR_OK;
  if (N > INT32_MAX) return fail(DDR_ERR_ARG, "summary: N must be below 2^31");
  if (R > kSummaryMaxRows) return fail(DDR_ERR_ARG, "summary: too many rows");
  if (N > 0 && !x) return fail(DDR_ERR_ARG, "summary: null x");
  if (!out) return fail(DDR_ERR_ARG, "summary: null out");
  if (!work) return fail(DDR_ERR_ARG, "summary: null work (ddr_summary_work_bytes)");
  if (reinterpret_cast<uintptr_t>(work) % 16) return fail(DDR_ERR_ARG, "summary: work must be 16-byte aligned");
  a.x = x;
  a.stride = row_stride;
  a.R = R;
  a.N = N;
  a.K = K;
  a.method = method;
  a.flags = flags;
  a.out = out;
  a.work = work;
  DDR_HIP(launch_summary<T>(a, static_cast<hipStream_t>(stream)));
  return DDR_OK;
}
ddr_status daily_objective_impl(const ddr_objective_desc* desc, const float* daily, int64_t daily_stride,
                                const float* obs, int64_t obs_stride, const uint8_t* drop, const float* weight,
                                double count, const float* count_dev, float* loss, float* grad, double* terms,
                                void* work, void* stream) {
  if (!desc) return fail(DDR_ERR_ARG, "daily_objective: null descriptor");
  const int64_t G = desc->n_gauges, D = desc->n_days, wd = desc->warmup;
  if (G < 0 || D < 0 || wd < 0 || daily_stride < 0 || obs_stride < 0)
    return fail(DDR_ERR_ARG, "daily_objective: negative size");
  if (desc->kind < 0 || desc->kind >= DDR_N_OBJECTIVES)
    return fail(DDR_ERR_ARG, "daily_objective: unknown kind " + std::to_string(desc->kind));
  if (!(desc->eps >= 0.0)) return fail(DDR_ERR_ARG, "daily_objective: eps must be >= 0");
  if (!(count >= 0.0)) return fail(DDR_ERR_ARG, "daily_objective: count must be >= 0 (0: not given)");
  if (G == 0) return DDR_OK;
  if (D < 1 || D > kObjectiveMaxDays)
    return fail(DDR_ERR_ARG, "daily_objective: 1 <= n_days <= " + std::to_string(kObjectiveMaxDays) + " (got " +
                                 std::to_string(D) + ")");
  if (wd >= D)
    return fail(DDR_ERR_ARG, "daily_objective: warmup " + std::to_string(wd) + " leaves no day of " + std::to_string(D));
  if (G > kObjectiveMaxGauges) return fail(DDR_ERR_ARG, "daily_objective: too many gauges");
  if (!daily) return fail(DDR_ERR_ARG, "daily_objective: null daily");
  if (!obs) return fail(DDR_ERR_ARG, "daily_objective: null obs");
  if (!loss) return fail(DDR_ERR_ARG, "daily_objective: null loss");
  if (!work) return fail(DDR_ERR_ARG, "daily_objective: null work (ddr_daily_objective_work_bytes)");
  ObjectiveArgs a{daily, obs, daily_stride, obs_stride, drop, weight, count_dev, count, G, (int)D, (int)wd,
                  desc->kind, desc->eps, loss, grad, terms, static_cast<double*>(work)};
  DDR_HIP(launch_objective(a, static_cast<hipStream_t>(stream)));
  return DDR_OK;
}
ddr_status clip_adam_impl(int64_t n, float* params, const float* grad, float* m, float* v, float lr, double beta1,
                          double beta2, float eps, float* step, float max_norm, float* norm_out, void* work,
                          void* stream) {
  if (n < 0) return fail(DDR_ERR_ARG, "clip_adam: negative size");
  if (n > 0 && (!params || !grad || !m || !v)) return fail(DDR_ERR_ARG, "clip_adam: null argument");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(DDR_ERR_ARG, "clip_adam: betas in [0, 1)");
  if (!step || !work) return fail(DDR_ERR_ARG, "clip_adam: null step counter or workspace (ddr_clip_adam_work_bytes)");
  DDR_HIP(launch_clip_adam(n, params, grad, m, v, lr, beta1, beta2, eps, step, max_norm, norm_out, work,
                           static_cast<hipStream_t>(stream)));
  return DDR_OK;
}

template <typename R>
ddr_status state_impl(const ddr_graph* gh, const R* x_save, int64_t T, int64_t t, double qlb, int32_t flags, R* out,
                      void* stream) {
  if (!gh || !x_save || !out) return fail(DDR_ERR_ARG, "null state argument");
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (!g->uploaded) return fail(DDR_ERR_ARG, "graph was built host-only: upload it first (ddr_graph_upload)");
  if (T < 1 || t < 0 || t >= T) return fail(DDR_ERR_ARG, "state step out of [0, T)");
  // a split rank holds the states of its own blocks only
  if (g->split.nranks > 0) return fail(DDR_ERR_ARG, "split basin: the saved states are per rank");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DDR_TRY(ready_for(g, s));
  DDR_HIP(launch_state_at<R>(g, T, t, qlb, (flags & DDR_FWD_CARRY) != 0, x_save, out, s));
  return DDR_OK;
}

// Linear Muskingum routing (route_linear.hip): the forcing gathered once into the schedule's row layout
// (one row per forcing interval), the status block and the granules re-initialised as for the forward.
template <typename R>
ddr_status lin_route_impl(const ddr_graph* gh, const R* k, const R* x, double dt, int64_t S, int64_t F, const R* qext,
                          const R* fs, const uint8_t* valid, const R* q0, int32_t flags, R* out, R* q_last, void* work,
                          double* bnd, void* status, void* stream) {
  if (!gh || !k || !x || !qext || !out || !q_last) return fail(DDR_ERR_ARG, "null linear-routing argument");
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (!g->uploaded) return fail(DDR_ERR_ARG, "graph was built host-only: upload it first (ddr_graph_upload)");
  if (g->split.nranks > 0) return fail(DDR_ERR_ARG, "split basin: linear routing is not supported");
  if (S < 1 || F < 1) return fail(DDR_ERR_ARG, "substeps and forcing intervals must be >= 1");
  if (flags & ~(DDR_LIN_END | DDR_LIN_STEADY)) return fail(DDR_ERR_ARG, "unknown linear-routing flag");
  if ((flags & DDR_LIN_STEADY) && q0) return fail(DDR_ERR_ARG, "DDR_LIN_STEADY takes no q0");
  // ticks of the deepest block (F * S + 1 states + its depth) in an int; the forcing rows too
  if (F > INT32_MAX || S > INT32_MAX || F > (INT32_MAX - 2 - g->max_block_depth) / S)
    return fail(DDR_ERR_ARG, "F * S + the deepest block exceeds the tick counter");
  if (F * (g->n + 1) > (int64_t(1) << 60)) return fail(DDR_ERR_ARG, "F * N overflows");
  if (!work) return fail(DDR_ERR_ARG, "null workspace (ddr_lin_work_bytes)");
  if (g->n_cut > 0 && !bnd) return fail(DDR_ERR_ARG, "graph has cut edges: bnd buffer required");
  if (!status) return fail(DDR_ERR_ARG, "null status block");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool cap = capturing(s);
  ddr_status st;
  if (!cap && (st = g_pending.check(false))) return st;
  const int res = linear_resident_blocks<R>(g);
  if (res < 0) return fail(DDR_ERR_HIP, "occupancy query failed");
  if (res == 0)
    return fail(DDR_ERR_CAPACITY, "the linear routing kernel does not fit a CU at this schedule's LDS size");
  DDR_TRY(ready_for(g, s));
  const int64_t TS = F * S + 1;
  DDR_HIP(hipMemsetAsync(status, 0, kStatusBytes, s));
  if (g->n_cut > 0) DDR_HIP(hipMemsetAsync(bnd, 0xFF, sizeof(double) * g->n_cut * TS, s));
  RouteArgs ga;  // the gather's view: qext rows as a q' store in the row layout, one row per interval
  std::memset(&ga, 0, sizeof(ga));
  ga.s = g->dev;
  ga.N = g->n;
  ga.T = TS;
  ga.qp_hours = (int32_t)S;
  ga.qp_shift = 0;
  ga.qs_rows = (int32_t)F;
  ga.qprime = qext;
  ga.fs = fs;
  ga.qp_valid = valid;
  ga.qs = work;
  DDR_HIP(launch_gather_qprime<R>(g, ga, s));
  LinArgs a;
  std::memset(&a, 0, sizeof(a));
  a.s = g->dev;
  a.N = g->n;
  a.F = F;
  a.S = (int32_t)S;
  a.TS = (int32_t)TS;
  a.flags = flags | (g_debug & kFlagForceTimeout);
  a.dt = dt;
  a.k = k;
  a.x = x;
  a.q0 = q0;
  a.qs = work;
  a.out = out;
  a.q_last = q_last;
  a.bnd = bnd;
  a.status = static_cast<unsigned*>(status);
  DDR_HIP(launch_route_linear<R>(g, a, s));
  return cap ? DDR_OK : g_pending.enqueue(status, s, "linear", gh);
}

template <typename R>
ddr_status lin_gauge_impl(int64_t N, int64_t F, const ddr_gauges* gz, const R* nf, R* out, void* stream) {
  if (!gz || !nf || !out || N < 1 || F < 1) return fail(DDR_ERR_ARG, "bad linear gauge arguments");
  if (gz->n_gauges > 0 && (!gz->offsets || !gz->index)) return fail(DDR_ERR_ARG, "null gauge arrays");
  DDR_HIP(launch_linear_gauge<R>(gz->n_gauges, F, gz->offsets, gz->index, nf, out, static_cast<hipStream_t>(stream)));
  return DDR_OK;
}

extern "C" {

ddr_status ddr_graph_build(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols, const ddr_build_opts* opts,
                           ddr_graph** out) {
  DDR_GUARD({
    if (!out) return fail(DDR_ERR_ARG, "null out");
    Graph* g = nullptr;
    ddr_status st = build_graph(n, e, rows, cols, opts, &g);
    if (st) return st;
    *out = reinterpret_cast<ddr_graph*>(g);
    return DDR_OK;
  })
}

ddr_status ddr_graph_build_device(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                                  const ddr_build_opts* opts, void* stream, ddr_graph** out) {
  DDR_GUARD({
    if (!out) return fail(DDR_ERR_ARG, "null out");
    Graph* g = nullptr;
    ddr_status st = build_graph_device(n, e, rows, cols, opts, static_cast<hipStream_t>(stream), &g);
    if (st) return st;
    *out = reinterpret_cast<ddr_graph*>(g);
    return DDR_OK;
  })
}

ddr_status ddr_graph_build_device_begin(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                                        const ddr_build_opts* opts, void* stream, ddr_graph_pending** out) {
  DDR_GUARD({
    if (!out) return fail(DDR_ERR_ARG, "null out");
    DevBuild* b = nullptr;
    ddr_status st = build_graph_device_begin(n, e, rows, cols, opts, static_cast<hipStream_t>(stream), &b);
    if (st) return st;
    *out = reinterpret_cast<ddr_graph_pending*>(b);
    return DDR_OK;
  })
}

ddr_status ddr_graph_build_device_finish(ddr_graph_pending* p, ddr_graph** out) {
  DDR_GUARD({
    if (!p) return fail(DDR_ERR_ARG, "null pending build");
    if (!out) {
      build_graph_device_cancel(reinterpret_cast<DevBuild*>(p));
      return fail(DDR_ERR_ARG, "null out");
    }
    Graph* g = nullptr;
    ddr_status st = build_graph_device_finish(reinterpret_cast<DevBuild*>(p), &g);
    if (st) return st;
    *out = reinterpret_cast<ddr_graph*>(g);
    return DDR_OK;
  })
}

ddr_status ddr_graph_build_device_cancel(ddr_graph_pending* p) {
  DDR_GUARD({
    build_graph_device_cancel(reinterpret_cast<DevBuild*>(p));
    return DDR_OK;
  })
}

ddr_status ddr_graph_fingerprint(const ddr_graph* gh, uint64_t* fp) {
  DDR_GUARD({
    if (!gh || !fp) return fail(DDR_ERR_ARG, "null argument");
    const Graph* g = reinterpret_cast<const Graph*>(gh);
    HostSchedule H;
    if (g->uploaded) {
      ddr_status st = device_schedule_to_host(g, H);
      if (st) return st;
    } else {
      H = g->hs;
    }
    unsigned long long h = schedule_fingerprint(H);
    auto mix = [&](const std::vector<int32_t>& v) {
      for (int32_t x : v) h = (h ^ (unsigned)x) * 1099511628211ull;
    };
    mix(H.pos_of_ref);
    mix(H.block_of_pos);
    mix(H.rs_loc);
    mix(H.rs_ref);
    for (const BlockDesc& B : g->blocks) {
      mix({B.pos0, B.nloc, B.virt0, B.nvirt, B.cout0, B.ncout, B.dmax, B.nxl, (int32_t)B.pre_dn,
           (int32_t)(B.pre_dn >> 32), B.xl0});
    }
    *fp = h;
    return DDR_OK;
  })
}

ddr_status ddr_collate_gauges(int64_t n_conus, int64_t n_gauges, const int64_t* sub_off, const int32_t* rows,
                              const int32_t* cols, const int32_t* gage_idx, int32_t* active, int64_t* n_active,
                              int64_t* crow, int32_t* col, int64_t* nnz, int64_t* out_off, int32_t* out_idx,
                              int64_t out_idx_cap, int32_t* gage_c) {
  DDR_GUARD({
    return collate_gauges(n_conus, n_gauges, sub_off, rows, cols, gage_idx, active, n_active, crow, col, nnz,
                          out_off, out_idx, out_idx_cap, gage_c);
  })
}

ddr_status ddr_collate_gauges_device(int64_t n_conus, int64_t n_gauges, int64_t e, const int32_t* rows,
                                     const int32_t* cols, const int32_t* gage_idx, int32_t* active, int64_t active_cap,
                                     int64_t* n_active, int32_t* rows_c, int32_t* cols_c, int64_t* nnz, int64_t* crow,
                                     int32_t* col, int64_t* out_off, int32_t* out_idx, int64_t out_idx_cap,
                                     int32_t* gage_c, void* stream) {
  DDR_GUARD({
    return collate_gauges_device(n_conus, n_gauges, e, rows, cols, gage_idx, active, active_cap, n_active, rows_c,
                                 cols_c, nnz, crow, col, out_off, out_idx, out_idx_cap, gage_c,
                                 static_cast<hipStream_t>(stream));
  })
}

ddr_status ddr_graph_upload(ddr_graph* g) {
  DDR_GUARD({
    if (!g) return fail(DDR_ERR_ARG, "null graph");
    return upload_schedule(reinterpret_cast<Graph*>(g));
  })
}

ddr_status ddr_graph_upload_async(ddr_graph* g, void* stream) {
  DDR_GUARD({
    if (!g) return fail(DDR_ERR_ARG, "null graph");
    return upload_schedule_async(reinterpret_cast<Graph*>(g), static_cast<hipStream_t>(stream));
  })
}

ddr_status ddr_graph_build_async(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                                 const ddr_build_opts* opts, void* stream, ddr_graph** out) {
  DDR_GUARD({
    if (!out) return fail(DDR_ERR_ARG, "null out");
    ddr_build_opts o;
    std::memset(&o, 0, sizeof(o));
    if (opts) o = *opts;
    const bool host_only = o.flags & DDR_BUILD_HOST_ONLY;
    o.flags |= DDR_BUILD_HOST_ONLY;
    Graph* g = nullptr;
    ddr_status st = build_graph(n, e, rows, cols, &o, &g);
    if (st) return st;
    if (!host_only && (st = upload_schedule_async(g, static_cast<hipStream_t>(stream)))) {
      destroy_graph(g);
      return st;
    }
    *out = reinterpret_cast<ddr_graph*>(g);
    return DDR_OK;
  })
}

ddr_status ddr_graph_destroy(ddr_graph* g) {
  DDR_GUARD({
    Graph* gr = reinterpret_cast<Graph*>(g);
    if (!gr) return DDR_OK;
    // on the graph's own device (the caller may have another one current): its sync, and the null stream
    // the pool-release events are recorded on
    DeviceGuard dg(gr->device);
    if (dg.error != hipSuccess) return fail(DDR_ERR_HIP, hipGetErrorString(dg.error));
    // synchronous, as the header promises: the pooled blocks of a device-built graph go back to the pool
    // only once no launch on any stream can still read them (their release event is recorded on the null
    // stream, which does not order PyTorch's non-blocking streams)
    if (gr->device_built || !gr->async_allocations.empty()) DDR_HIP(hipDeviceSynchronize());
    destroy_graph(gr);
    return DDR_OK;
  })
}

ddr_status ddr_qprime_nan_wait(int32_t* has_nan) {
  DDR_GUARD({
    if (!has_nan) return fail(DDR_ERR_ARG, "null has_nan");
    if (t_nan_dev < 0 || !t_nan[t_nan_dev].armed) return fail(DDR_ERR_ARG, "no DDR_FWD_CHECK_QPRIME forward on this thread");
    NanCheck& c = t_nan[t_nan_dev];
    DDR_HIP(hipEventSynchronize(c.ev));
    *has_nan = *c.host ? 1 : 0;
    c.armed = false;
    return DDR_OK;
  })
}

ddr_status ddr_pool_trim(int64_t* freed_bytes) {
  DDR_GUARD({
    const int64_t f = pool_trim();
    if (freed_bytes) *freed_bytes = f;
    return DDR_OK;
  })
}

ddr_status ddr_graph_destroy_async(ddr_graph* g, void* stream) {
  DDR_GUARD({
    destroy_graph(reinterpret_cast<Graph*>(g), static_cast<hipStream_t>(stream));
    return DDR_OK;
  })
}

ddr_status ddr_xmem_alloc(int64_t bytes, void** ptr, void* handle, int32_t* kind) {
  DDR_GUARD({
    if (bytes <= 0 || !ptr || !handle) return fail(DDR_ERR_ARG, "bad ddr_xmem_alloc arguments");
    // uncached device memory (no stale L2 copy of a peer's stores); fine-grained, then plain device
    // memory where the uncached kind cannot be exported
    for (int k = 0; k < 3; ++k) {
      const unsigned flag = k == 0 ? hipDeviceMallocUncached : (k == 1 ? hipDeviceMallocFinegrained : hipDeviceMallocDefault);
      void* p = nullptr;
      if (hipExtMallocWithFlags(&p, (size_t)bytes, flag) != hipSuccess) {
        (void)hipGetLastError();
        continue;
      }
      hipIpcMemHandle_t h;
      if (hipIpcGetMemHandle(&h, p) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(p);
        continue;
      }
      DDR_HIP(hipMemset(p, 0, (size_t)bytes));
      std::memcpy(handle, &h, sizeof(h));
      *ptr = p;
      if (kind) *kind = k;
      return DDR_OK;
    }
    return fail(DDR_ERR_HIP, "ddr_xmem_alloc: no exportable device allocation");
  })
}

ddr_status ddr_xmem_open(const void* handle, void** ptr) {
  DDR_GUARD({
    if (!handle || !ptr) return fail(DDR_ERR_ARG, "null argument");
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, sizeof(h));
    DDR_HIP(hipIpcOpenMemHandle(ptr, h, hipIpcMemLazyEnablePeerAccess));
    return DDR_OK;
  })
}

ddr_status ddr_xmem_close(void* ptr, int32_t opened) {
  DDR_GUARD({
    if (!ptr) return DDR_OK;
    DDR_HIP(opened ? hipIpcCloseMemHandle(ptr) : hipFree(ptr));
    return DDR_OK;
  })
}

ddr_status ddr_xmem_bytes(int64_t n_x, int64_t T, int64_t* bytes) {
  if (n_x < 0 || T < 1 || !bytes) return fail(DDR_ERR_ARG, "bad ddr_xmem_bytes arguments");
  *bytes = (int64_t)xmem_bytes(n_x, T);
  return DDR_OK;
}

ddr_status ddr_graph_blocks(const ddr_graph* gh, int32_t* nloc, int64_t cap) {
  if (!gh || !nloc) return fail(DDR_ERR_ARG, "null argument");
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (cap < (int64_t)g->blocks.size()) return fail(DDR_ERR_ARG, "ddr_graph_blocks: capacity below n_blocks");
  for (size_t b = 0; b < g->blocks.size(); ++b) nloc[b] = g->blocks[b].nloc;
  return DDR_OK;
}

ddr_status ddr_graph_cut_blocks(const ddr_graph* gh, int32_t* prod, int32_t* cons, int64_t cap) {
  DDR_GUARD({
    if (!gh || !prod || !cons) return fail(DDR_ERR_ARG, "null argument");
    const Graph* g = reinterpret_cast<const Graph*>(gh);
    if (cap < g->n_cut) return fail(DDR_ERR_ARG, "ddr_graph_cut_blocks: capacity below n_cut");
    HostSchedule H;
    if (g->uploaded) {
      ddr_status st = device_schedule_to_host(g, H);
      if (st) return st;
    } else {
      H = g->hs;
    }
    for (int64_t e = 0; e < g->n_cut; ++e) prod[e] = cons[e] = -1;
    for (size_t b = 0; b < g->blocks.size(); ++b) {
      const BlockDesc& B = g->blocks[b];
      for (int i = 0; i < B.nloc; ++i) {
        const int32_t e = H.cut[B.pos0 + i];
        if (e >= 0) prod[e] = (int32_t)b;
      }
      for (int v = 0; v < B.nvirt; ++v) cons[H.v_edge[B.virt0 + v]] = (int32_t)b;
    }
    return DDR_OK;
  })
}

ddr_status ddr_graph_set_split(ddr_graph* gh, int32_t rank, int32_t nranks, const int32_t* block_rank, void* local,
                               void* const* peers, int64_t t_cap, int64_t* n_x_out) {
  DDR_GUARD({
    if (!gh || !block_rank || !local || !peers || t_cap < 1) return fail(DDR_ERR_ARG, "bad ddr_graph_set_split arguments");
    if (nranks < 2 || nranks > kMaxSplitRanks || rank < 0 || rank >= nranks)
      return fail(DDR_ERR_ARG, "split basin: 2 <= nranks <= 16, 0 <= rank < nranks");
    Graph* g = reinterpret_cast<Graph*>(gh);
    if (!g->uploaded) return fail(DDR_ERR_ARG, "graph was built host-only: upload it first (ddr_graph_upload)");
    if (g->split.nranks > 0) return fail(DDR_ERR_ARG, "split basin: already set");
    const int64_t nb = (int64_t)g->blocks.size();
    for (int64_t b = 0; b < nb; ++b)
      if (block_rank[b] < 0 || block_rank[b] >= nranks) return fail(DDR_ERR_ARG, "split basin: block rank out of range");
    std::vector<int32_t> prod((size_t)g->n_cut);
    std::vector<int32_t> cons((size_t)g->n_cut);
    ddr_status st = ddr_graph_cut_blocks(gh, prod.data(), cons.data(), g->n_cut);
    if (st) return st;
    std::vector<int32_t> xid((size_t)g->n_cut);
    std::fill(xid.begin(), xid.end(), -1);
    std::vector<int32_t> xcons;
    std::vector<int32_t> xprod;
    std::vector<int64_t> xedge;
    for (int64_t e = 0; e < g->n_cut; ++e) {
      if (prod[e] < 0 || cons[e] < 0) return fail(DDR_ERR_ARG, "split basin: cut edge without both blocks");
      if (block_rank[prod[e]] != block_rank[cons[e]]) {
        xid[e] = (int32_t)xcons.size();
        xcons.push_back(block_rank[cons[e]]);
        xprod.push_back(block_rank[prod[e]]);
        xedge.push_back(e);
      }
    }
    std::vector<uint8_t> owned(nb);
    for (int64_t b = 0; b < nb; ++b) owned[b] = block_rank[b] == rank ? 1 : 0;
    auto up = [&](const void* src, size_t bytes, void** dst) -> hipError_t {
      hipError_t e = hipMalloc(dst, bytes < 16 ? 16 : bytes);
      if (e != hipSuccess) return e;
      g->allocations.push_back(*dst);
      return bytes ? hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    SplitState sp;
    DDR_HIP(up(owned.data(), owned.size(), reinterpret_cast<void**>(&sp.owned)));
    DDR_HIP(up(xid.data(), xid.size() * 4, reinterpret_cast<void**>(&sp.xid)));
    DDR_HIP(up(xcons.data(), xcons.size() * 4, reinterpret_cast<void**>(&sp.xcons)));
    DDR_HIP(up(xprod.data(), xprod.size() * 4, reinterpret_cast<void**>(&sp.xprod)));
    DDR_HIP(up(xedge.data(), xedge.size() * 8, reinterpret_cast<void**>(&sp.xedge)));
    sp.rank = rank;
    sp.nranks = nranks;
    sp.n_x = (int32_t)xcons.size();
    sp.t_cap = t_cap;
    sp.local = static_cast<char*>(local);
    for (int p = 0; p < nranks; ++p) sp.peers[p] = static_cast<char*>(peers[p]);
    g->split = sp;
    if (n_x_out) *n_x_out = sp.n_x;
    return DDR_OK;
  })
}

ddr_status ddr_graph_clear_split(ddr_graph* gh) {
  if (!gh) return fail(DDR_ERR_ARG, "null graph");
  Graph* g = reinterpret_cast<Graph*>(gh);
  // the device arrays stay with the graph (freed at destroy); the receive memory is the caller's
  const SplitState none;
  g->split = none;
  return DDR_OK;
}

ddr_status ddr_graph_get_info(const ddr_graph* gh, ddr_graph_info* info) {
  if (!gh || !info) return fail(DDR_ERR_ARG, "null argument");
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  info->n = g->n;
  info->nnz = g->nnz;
  info->n_basins = g->n_basins;
  info->n_pieces = g->n_pieces;
  info->n_blocks = (int64_t)g->blocks.size();
  info->n_cut = g->n_cut;
  info->max_depth = g->max_depth;
  info->max_block_depth = g->max_block_depth;
  info->reaches_per_thread = g->kr;
  info->save_elems_per_t = 2 * g->n;  // x (routing states) | q' gathered into the same layout
  info->save_elems_fixed = 2 * g->sum_dn;
  info->bnd_elems_per_t = g->n_cut;
  info->bwd_elems_per_t = 2 * g->n_cut;
  info->bwd_elems_fixed = 3 * g->n;
  info->generations = g->generations;
  info->status_bytes = kStatusBytes;
  return DDR_OK;
}

ddr_status ddr_graph_csr(const ddr_graph* gh, int64_t* crow, int64_t* col) {
  if (!gh || !crow || (!col && reinterpret_cast<const Graph*>(gh)->nnz > 0)) return fail(DDR_ERR_ARG, "null argument");
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (g->device_built) DDR_GUARD({ return device_views_to_host(g, crow, col, nullptr, nullptr, nullptr, nullptr); })
  std::memcpy(crow, g->crow.data(), sizeof(int64_t) * (g->n + 1));
  if (g->nnz) std::memcpy(col, g->col.data(), sizeof(int64_t) * g->nnz);
  return DDR_OK;
}

ddr_status ddr_graph_structure(const ddr_graph* gh, int64_t* down, int64_t* dist, int64_t* basin, int64_t* block) {
  if (!gh) return fail(DDR_ERR_ARG, "null graph");
  const Graph* g = reinterpret_cast<const Graph*>(gh);
  if (g->device_built) DDR_GUARD({ return device_views_to_host(g, nullptr, nullptr, down, dist, basin, block); })
  const size_t b = sizeof(int64_t) * g->n;
  if (down) std::memcpy(down, g->down.data(), b);
  if (dist) std::memcpy(dist, g->dist.data(), b);
  if (basin) std::memcpy(basin, g->basin.data(), b);
  if (block) std::memcpy(block, g->block_of.data(), b);
  return DDR_OK;
}

ddr_status ddr_mc_forward_f32(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                              const float* qprime, int64_t T, const float* q0, float* runoff, float* x_save,
                              double* bnd, void* status, float* q_last, float* tw, float* ss, int32_t flags,
                              void* stream) {
  DDR_GUARD({ return forward_impl<float>(g, c, r, qprime, T, q0, runoff, x_save, bnd, status, q_last, tw, ss, flags, stream); })
}
ddr_status ddr_mc_forward_f64(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                              const double* qprime, int64_t T, const double* q0, double* runoff, double* x_save,
                              double* bnd, void* status, double* q_last, double* tw, double* ss, int32_t flags,
                              void* stream) {
  DDR_GUARD({ return forward_impl<double>(g, c, r, qprime, T, q0, runoff, x_save, bnd, status, q_last, tw, ss, flags, stream); })
}
ddr_status ddr_mc_backward_f32(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                               const float* qprime, int64_t T, const float* x_save, const double* bnd,
                               const float* grad, const ddr_gauges* gauges, double* bwd_bnd, void* status,
                               float* gn, float* gq, float* gp, int32_t flags, void* stream) {
  DDR_GUARD({ return backward_impl<float>(g, c, r, qprime, T, x_save, bnd, grad, gauges, bwd_bnd, status, gn, gq, gp, flags, stream); })
}
ddr_status ddr_mc_backward_f64(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                               const double* qprime, int64_t T, const double* x_save, const double* bnd,
                               const double* grad, const ddr_gauges* gauges, double* bwd_bnd, void* status,
                               double* gn, double* gq, double* gp, int32_t flags, void* stream) {
  DDR_GUARD({ return backward_impl<double>(g, c, r, qprime, T, x_save, bnd, grad, gauges, bwd_bnd, status, gn, gq, gp, flags, stream); })
}
ddr_status ddr_hotstart_f32(const ddr_graph* gh, const float* q, double discharge_lb, float* out, void* stream) {
  DDR_GUARD({
    if (!gh || !q || !out) return fail(DDR_ERR_ARG, "null hot-start argument");
    const Graph* g = reinterpret_cast<const Graph*>(gh);
    if (!g->uploaded) return fail(DDR_ERR_ARG, "graph was built host-only: upload it first (ddr_graph_upload)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one forward step in accumulation mode (every step a hot start, no coefficient physics): its
    // workspace is stream-ordered scratch; the per-reach statics are never read for their values
    const size_t xs = sizeof(float) * 2 * (size_t)(g->n + g->sum_dn);
    void* ws = device_get(xs + sizeof(double) * (size_t)std::max<int64_t>(g->n_cut, 1) + kStatusBytes, s);
    if (!ws) return fail(DDR_ERR_HIP, "hot start: out of device memory");
    ddr_mc_consts c;
    c.dt = 3600.0;
    c.discharge_lb = discharge_lb;
    c.velocity_lb = 0.01;
    c.velocity_ub = 15.0;
    c.depth_lb = 0.01;
    c.bottom_width_lb = 0.01;
    c.side_slope_lb = 0.5;
    c.side_slope_ub = 50.0;
    ddr_mc_reaches r{};
    r.n = r.q_spatial = r.p_spatial = r.length = r.slope = r.x_storage = q;
    r.p_stride = 1;
    unsigned char* base = static_cast<unsigned char*>(ws);
    ddr_status st = forward_impl<float>(gh, &c, &r, q, 1, nullptr, out, reinterpret_cast<float*>(base),
                                        reinterpret_cast<double*>(base + xs), base + xs + sizeof(double) * std::max<int64_t>(g->n_cut, 1),
                                        nullptr, nullptr, nullptr, DDR_FWD_ACCUMULATE, stream);
    device_put(ws, s);
    return st;
  })
}

int64_t ddr_state_work_bytes(const ddr_graph* g, int64_t T, int64_t n_gauges, int32_t real_bytes) {
  if (!g || T < 1 || n_gauges < 0 || (real_bytes != 4 && real_bytes != 8)) return -1;
  return state_work_bytes(reinterpret_cast<const Graph*>(g), T, n_gauges, (size_t)real_bytes);
}
ddr_status ddr_mc_backward_state_f32(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                                     const float* qprime, int64_t qprime_rows, int64_t T, const float* x_save,
                                     const double* bnd, const float* grad, const ddr_gauges* gauges, double* bwd_bnd,
                                     void* status, float* gn, float* gq, float* gp, float* grad_qprime,
                                     float* grad_q0, void* work, int32_t flags, void* stream) {
  DDR_GUARD({ return backward_impl<float>(g, c, r, qprime, T, x_save, bnd, grad, gauges, bwd_bnd, status, gn, gq, gp, flags, stream, qprime_rows, grad_qprime, grad_q0, work); })
}
ddr_status ddr_mc_backward_state_f64(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                                     const double* qprime, int64_t qprime_rows, int64_t T, const double* x_save,
                                     const double* bnd, const double* grad, const ddr_gauges* gauges, double* bwd_bnd,
                                     void* status, double* gn, double* gq, double* gp, double* grad_qprime,
                                     double* grad_q0, void* work, int32_t flags, void* stream) {
  DDR_GUARD({ return backward_impl<double>(g, c, r, qprime, T, x_save, bnd, grad, gauges, bwd_bnd, status, gn, gq, gp, flags, stream, qprime_rows, grad_qprime, grad_q0, work); })
}
ddr_status ddr_mc_backward_ex_f32(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                                  const float* qprime, int64_t qprime_rows, int64_t T, const float* x_save,
                                  const double* bnd, const float* grad, const ddr_gauges* gauges,
                                  const float* state_seed, double* bwd_bnd, void* status, float* gn, float* gq,
                                  float* gp, float* grad_qprime, float* grad_q0, void* work, int32_t flags,
                                  void* stream) {
  DDR_GUARD({ return backward_impl<float>(g, c, r, qprime, T, x_save, bnd, grad, gauges, bwd_bnd, status, gn, gq, gp, flags, stream, qprime_rows, grad_qprime, grad_q0, work, state_seed); })
}
ddr_status ddr_mc_backward_ex_f64(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                                  const double* qprime, int64_t qprime_rows, int64_t T, const double* x_save,
                                  const double* bnd, const double* grad, const ddr_gauges* gauges,
                                  const double* state_seed, double* bwd_bnd, void* status, double* gn, double* gq,
                                  double* gp, double* grad_qprime, double* grad_q0, void* work, int32_t flags,
                                  void* stream) {
  DDR_GUARD({ return backward_impl<double>(g, c, r, qprime, T, x_save, bnd, grad, gauges, bwd_bnd, status, gn, gq, gp, flags, stream, qprime_rows, grad_qprime, grad_q0, work, state_seed); })
}

int64_t ddr_pnet_param_count(int32_t n_features) {
  if (n_features < 1 || n_features > 12) return -1;
  return pnet_param_count(n_features);
}
int64_t ddr_pnet_work_bytes(int64_t n_rows, int32_t n_features) {
  if (n_rows < 0 || n_features < 1 || n_features > 12) return -1;
  return pnet_work_bytes(n_rows, n_features);
}
ddr_status ddr_pnet_forward_f32(int64_t n_rows, int32_t n_features, const float* x, const float* params,
                                const float* denorm, float* z_save, float* u_save, float* out_n, float* out_q,
                                float* out_p, void* stream) {
  DDR_GUARD({ return pnet_forward_impl(n_rows, n_features, x, params, denorm, z_save, u_save, out_n, out_q, out_p, stream); })
}
ddr_status ddr_pnet_backward_f32(int64_t n_rows, int32_t n_features, const float* x, const float* params,
                                 const float* denorm, const float* z_save, const float* u_save, const float* grad_n,
                                 const float* grad_q, const float* grad_p, float* grad_params, void* work,
                                 void* stream) {
  DDR_GUARD({ return pnet_backward_impl(n_rows, n_features, x, params, denorm, z_save, u_save, grad_n, grad_q, grad_p, grad_params, work, stream); })
}
int64_t ddr_kan_param_count(const ddr_kan_desc* desc) {
  if (!kan_validate(desc).empty()) return -1;
  return KanLayout(*desc).total();
}
int64_t ddr_kan_const_count(const ddr_kan_desc* desc) {
  if (!kan_validate(desc).empty()) return -1;
  return KanLayout(*desc).const_total();
}
int64_t ddr_kan_work_bytes(const ddr_kan_desc* desc, int64_t n_rows, int32_t backward) {
  if (!kan_validate(desc).empty() || n_rows < 1 || n_rows > (int64_t(1) << 30)) return -1;
  return kan_work_bytes(*desc, n_rows, backward != 0);
}
ddr_status ddr_kan_forward_f32(const ddr_kan_desc* desc, int64_t n_rows, const float* x, const float* params,
                               const float* consts, float* h_save, float* u, void* work, void* stream) {
  DDR_GUARD({ return kan_forward_impl(desc, n_rows, x, params, consts, h_save, u, work, stream); })
}
ddr_status ddr_kan_backward_f32(const ddr_kan_desc* desc, int64_t n_rows, const float* x, const float* params,
                                const float* consts, const float* h_save, const float* u, const float* grad_u,
                                float* grad_params, void* work, void* stream) {
  DDR_GUARD({ return kan_backward_impl(desc, n_rows, x, params, consts, h_save, u, grad_u, grad_params, work, stream); })
}
ddr_status ddr_daily_l1_f32(int64_t n_gauges, int64_t n_days, int64_t warmup, const float* daily, const float* obs,
                            float inv_count, float* loss, float* grad, void* stream) {
  DDR_GUARD({ return daily_l1_impl(n_gauges, n_days, warmup, daily, obs, inv_count, loss, grad, stream); })
}
ddr_status ddr_daily_objective_f32(const ddr_objective_desc* desc, const float* daily, int64_t daily_stride,
                                   const float* obs, int64_t obs_stride, const uint8_t* drop, const float* weight,
                                   double count, const float* count_dev, float* loss, float* grad, double* terms,
                                   void* work, void* stream) {
  DDR_GUARD({
    return daily_objective_impl(desc, daily, daily_stride, obs, obs_stride, drop, weight, count, count_dev, loss, grad,
                                terms, work, stream);
  })
}
ddr_status ddr_metrics_f32(int64_t n_gauges, int64_t n_days, const float* pred, int64_t pred_stride,
                           const float* target, int64_t target_stride, double* out, int32_t* pred_nan_count,
                           void* stream) {
  DDR_GUARD({ return metrics_impl(n_gauges, n_days, pred, pred_stride, target, target_stride, out, pred_nan_count, stream); })
}
int64_t ddr_summary_work_bytes(int64_t R, int32_t K, int32_t elem_bytes) {
  if (R < 0 || R > kSummaryMaxRows || K < 0 || K > kSummaryMaxQ || (elem_bytes != 4 && elem_bytes != 8)) return -1;
  return (int64_t)summary_work_bytes(R, K, elem_bytes);
}
ddr_status ddr_summary_f32(int64_t R, int64_t N, const float* x, int64_t row_stride, int32_t K, const double* q,
                           int32_t method, int32_t flags, double* out, void* work, void* stream) {
  DDR_GUARD({ return summary_impl<float>(R, N, x, row_stride, K, q, method, flags, out, work, stream); })
}
ddr_status ddr_summary_f64(int64_t R, int64_t N, const double* x, int64_t row_stride, int32_t K, const double* q,
                           int32_t method, int32_t flags, double* out, void* work, void* stream) {
  DDR_GUARD({ return summary_impl<double>(R, N, x, row_stride, K, q, method, flags, out, work, stream); })
}
ddr_status ddr_summedq_plan_create(int64_t n_gauges, const int64_t* member_off, const int32_t* member_idx,
                                   int64_t chunk, void* stream, ddr_summedq_plan* plan) {
  DDR_GUARD({
    return summedq_plan_create(n_gauges, member_off, member_idx, chunk, static_cast<hipStream_t>(stream),
                               reinterpret_cast<SummedQPlan**>(plan));
  })
}
ddr_status ddr_summedq_plan_destroy(ddr_summedq_plan plan) {
  summedq_plan_destroy(static_cast<SummedQPlan*>(plan));
  return DDR_OK;
}
int64_t ddr_summedq_scratch_bytes(ddr_summedq_plan plan, int64_t n_days) {
  return summedq_scratch_bytes(static_cast<const SummedQPlan*>(plan), n_days);
}
ddr_status ddr_summedq_f32(ddr_summedq_plan plan, const float* qr, int64_t n_rows, int64_t row_stride, int64_t n_steps,
                           int32_t hours_per_step, float* out, int64_t out_stride, void* scratch,
                           int64_t scratch_bytes, void* stream) {
  DDR_GUARD({
    return summedq_run(static_cast<const SummedQPlan*>(plan), qr, n_rows, row_stride, n_steps, hours_per_step, out,
                       out_stride, scratch, scratch_bytes, static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_feed_qprime_f32(const float* store, int64_t row_stride, int64_t n_rows, int64_t n_store_cols,
                               const int32_t* rows, int64_t n_reaches, int64_t t0, int64_t n_cols, int32_t repeat,
                               int64_t n_out, float fill, float* out, uint8_t* valid, void* stream) {
  DDR_GUARD({
    return feed_qprime(store, row_stride, n_rows, n_store_cols, rows, n_reaches, t0, n_cols, repeat, n_out, fill, out,
                       valid, static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_feed_rows_f32(const float* store, int64_t row_stride, int64_t n_rows, int64_t n_store_cols,
                             const int32_t* rows, int64_t n_out_rows, int64_t t0, int64_t n_cols, int32_t trim,
                             float* out, int64_t out_stride, uint8_t* has_nan, void* stream) {
  DDR_GUARD({
    return feed_rows(store, row_stride, n_rows, n_store_cols, rows, n_out_rows, t0, n_cols, trim, out, out_stride,
                     has_nan, static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_feed_attributes_f32(const float* table, int64_t row_stride, int64_t n_conus, int32_t n_attrs,
                                   const int32_t* active, int64_t n_reaches, const float* fill, const float* means,
                                   const float* stds, float* spatial, float* normalized, const ddr_flowpath* path,
                                   float* flow_scale, void* stream) {
  DDR_GUARD({
    return feed_attributes(table, row_stride, n_conus, n_attrs, active, n_reaches, fill, means, stds, spatial,
                           normalized, path, flow_scale, static_cast<hipStream_t>(stream));
  })
}
int64_t ddr_feed_attr_mean_work_bytes(int32_t n_flagged) { return feed_attr_mean_work_bytes(n_flagged); }
ddr_status ddr_feed_attr_mean_f32(const float* table, int64_t row_stride, int64_t n_conus, int32_t n_attrs,
                                  const int32_t* active, int64_t n_reaches, const int32_t* flagged, int32_t n_flagged,
                                  float* fill, void* work, int64_t work_bytes, void* stream) {
  DDR_GUARD({
    return feed_attr_mean(table, row_stride, n_conus, n_attrs, active, n_reaches, flagged, n_flagged, fill, work,
                          work_bytes, static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_feed_flow_scale_f32(const int32_t* gage_c, const int32_t* scale_rows, int64_t n_gauges,
                                   const float* factors, const uint8_t* skip, int64_t n_factors, int64_t n_reaches,
                                   int32_t* winner, float* flow_scale, void* stream) {
  DDR_GUARD({
    return feed_flow_scale(gage_c, scale_rows, n_gauges, factors, skip, n_factors, n_reaches, winner, flow_scale,
                           static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_upstream_index_create(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols, int32_t flags,
                                     void* stream, ddr_upstream_index* index) {
  DDR_GUARD({
    return upstream_index_create(n, e, rows, cols, flags, static_cast<hipStream_t>(stream),
                                 reinterpret_cast<UpstreamIndex**>(index));
  })
}
ddr_status ddr_upstream_index_destroy(ddr_upstream_index index) {
  upstream_index_destroy(static_cast<UpstreamIndex*>(index));
  return DDR_OK;
}
ddr_status ddr_upstream_index_info(ddr_upstream_index index, ddr_upstream_info* info) {
  if (!index || !info) return fail(DDR_ERR_ARG, "upstream_index_info: null argument");
  const auto* ix = static_cast<const UpstreamIndex*>(index);
  info->n = ix->n;
  info->n_outlets = ix->n_outlets;
  info->max_depth = ix->max_depth;
  info->rounds = ix->rounds;
  info->device = ix->device;
  return DDR_OK;
}
ddr_status ddr_upstream_index_down(ddr_upstream_index index, int32_t* down) {
  if (!index || !down) return fail(DDR_ERR_ARG, "upstream_index_down: null argument");
  const auto* ix = static_cast<const UpstreamIndex*>(index);
  std::copy(ix->down.begin(), ix->down.end(), down);
  return DDR_OK;
}
int64_t ddr_upstream_scratch_bytes(ddr_upstream_index index, int64_t n_targets, int64_t n_members) {
  return upstream_scratch_bytes(static_cast<const UpstreamIndex*>(index), n_targets, n_members);
}
ddr_status ddr_upstream_label(ddr_upstream_index index, int64_t n_targets, const int32_t* targets, int32_t* label_out,
                              int32_t* slot_of, void* scratch, int64_t scratch_bytes, void* stream) {
  DDR_GUARD({
    return upstream_label(static_cast<const UpstreamIndex*>(index), n_targets, targets, label_out, slot_of, scratch,
                          scratch_bytes, static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_upstream_collate(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx, int32_t* active,
                                int64_t active_cap, int64_t* n_active, int32_t* rows_c, int32_t* cols_c,
                                int64_t edge_cap, int64_t* nnz, int64_t* crow, int32_t* col, int64_t* out_off,
                                int32_t* out_idx, int64_t out_idx_cap, int32_t* gage_c, void* scratch,
                                int64_t scratch_bytes, void* stream) {
  DDR_GUARD({
    return upstream_collate(static_cast<const UpstreamIndex*>(index), n_gauges, gage_idx, active, active_cap, n_active,
                            rows_c, cols_c, edge_cap, nnz, crow, col, out_off, out_idx, out_idx_cap, gage_c, scratch,
                            scratch_bytes, static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_upstream_member_counts(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx, int64_t* off,
                                      int64_t* total, void* scratch, int64_t scratch_bytes, void* stream) {
  DDR_GUARD({
    return upstream_member_counts(static_cast<const UpstreamIndex*>(index), n_gauges, gage_idx, off, total, scratch,
                                  scratch_bytes, static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_upstream_members(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx, int64_t n_members,
                                int32_t* idx, void* scratch, int64_t scratch_bytes, void* stream) {
  DDR_GUARD({
    return upstream_members(static_cast<const UpstreamIndex*>(index), n_gauges, gage_idx, n_members, idx, scratch,
                            scratch_bytes, static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_upstream_label_host(ddr_upstream_index index, int64_t n_targets, const int32_t* targets,
                                   int32_t* label_out, int32_t* slot_of) {
  DDR_GUARD({
    return upstream_label_host(static_cast<const UpstreamIndex*>(index), n_targets, targets, label_out, slot_of);
  })
}
ddr_status ddr_upstream_collate_host(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx,
                                     int32_t* active, int64_t active_cap, int64_t* n_active, int64_t* crow,
                                     int32_t* col, int64_t edge_cap, int64_t* nnz, int64_t* out_off, int32_t* out_idx,
                                     int64_t out_idx_cap, int32_t* gage_c) {
  DDR_GUARD({
    return upstream_collate_host(static_cast<const UpstreamIndex*>(index), n_gauges, gage_idx, active, active_cap,
                                 n_active, crow, col, edge_cap, nnz, out_off, out_idx, out_idx_cap, gage_c);
  })
}
ddr_status ddr_upstream_member_counts_host(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx,
                                           int64_t* off) {
  DDR_GUARD({ return upstream_member_counts_host(static_cast<const UpstreamIndex*>(index), n_gauges, gage_idx, off); })
}
ddr_status ddr_upstream_members_host(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx,
                                     const int64_t* off, int32_t* idx) {
  DDR_GUARD({ return upstream_members_host(static_cast<const UpstreamIndex*>(index), n_gauges, gage_idx, off, idx); })
}
ddr_status ddr_network_build(int64_t n, const int64_t* ids, const int64_t* to_ids, int32_t flags, void* stream,
                             ddr_network* network) {
  DDR_GUARD({
    return network_build(n, ids, to_ids, flags, static_cast<hipStream_t>(stream),
                         reinterpret_cast<Network**>(network));
  })
}
ddr_status ddr_network_build_host(int64_t n, const int64_t* ids, const int64_t* to_ids, ddr_network* network) {
  DDR_GUARD({ return network_build_host(n, ids, to_ids, reinterpret_cast<Network**>(network)); })
}
ddr_status ddr_network_info(ddr_network network, ddr_network_counts* info) {
  if (!network || !info) return fail(DDR_ERR_ARG, "network_info: null argument");
  const auto* nw = static_cast<const Network*>(network);
  info->n = nw->n;
  info->kept = nw->kept;
  info->nnz = nw->nnz;
  info->n_dropped = nw->n_dropped;
  info->n_basins = nw->n_basins;
  info->max_depth = nw->max_depth;
  info->device = nw->device;
  return DDR_OK;
}
ddr_status ddr_network_get(ddr_network network, int32_t* position, int64_t* order, int32_t* down, int32_t* rows,
                           int32_t* cols, int32_t* dropped, void* stream) {
  DDR_GUARD({
    return network_get(static_cast<const Network*>(network), position, order, down, rows, cols, dropped,
                       static_cast<hipStream_t>(stream));
  })
}
ddr_status ddr_network_destroy(ddr_network network) {
  network_destroy(static_cast<Network*>(network));
  return DDR_OK;
}
ddr_status ddr_network_lookup_i64(int64_t n, const int64_t* ids, int64_t m, const int64_t* queries, int32_t* pos,
                                  int32_t flags, void* stream) {
  DDR_GUARD({ return network_lookup(n, ids, m, queries, pos, flags, static_cast<hipStream_t>(stream)); })
}
ddr_status ddr_network_lookup_i64_host(int64_t n, const int64_t* ids, int64_t m, const int64_t* queries,
                                       int32_t* pos) {
  DDR_GUARD({ return network_lookup_host(n, ids, m, queries, pos); })
}
ddr_status ddr_attr_prepare_f32(int64_t n_rows, int32_t n_features, const float* raw, int64_t feat_stride,
                                const double* scale, const double* offset, const int32_t* log10_flag,
                                const float* mean, const float* std, const float* p10, const float* p90, float* x,
                                int64_t* counts, void* stream) {
  DDR_GUARD({ return attr_prepare_impl(n_rows, n_features, raw, feat_stride, scale, offset, log10_flag, mean, std, p10, p90, x, counts, stream); })
}
ddr_status ddr_geometry_predict_f32(int64_t n_rows, int32_t n_outputs, const float* u, const ddr_geom_slot* slot_n,
                                    const ddr_geom_slot* slot_q, const ddr_geom_slot* slot_p, const float* discharge,
                                    const float* slope, double discharge_lb, double slope_lb, double depth_lb,
                                    double bottom_width_lb, float* out, int64_t out_stride, void* stream) {
  DDR_GUARD({ return geometry_predict_impl(n_rows, n_outputs, u, slot_n, slot_q, slot_p, discharge, slope, discharge_lb, slope_lb, depth_lb, bottom_width_lb, out, out_stride, stream); })
}
// ---- the BMI coupling (bmi.hip) ----
ddr_status ddr_bmi_nexus_table(int64_t n_keys, const int64_t* keys_host, const int32_t* seg_host, int64_t n_segments,
                               int64_t* keys, int32_t* key_seg, void* stream) {
  DDR_GUARD({
    if (n_keys < 0 || n_segments < 0) return fail(DDR_ERR_ARG, "bmi nexus table: negative size");
    if (n_segments > INT32_MAX) return fail(DDR_ERR_ARG, "bmi nexus table: more segments than int32 indices");
    if (n_keys == 0) return DDR_OK;
    if (!keys_host || !seg_host || !keys || !key_seg) return fail(DDR_ERR_ARG, "bmi nexus table: null argument");
    for (int64_t j = 0; j < n_keys; ++j) {
      if (j > 0 && keys_host[j] <= keys_host[j - 1])
        return fail(DDR_ERR_ARG, "bmi nexus table: keys must be strictly ascending (key " + std::to_string(j) + ")");
      if (seg_host[j] < 0 || seg_host[j] >= n_segments)
        return fail(DDR_ERR_ARG, "bmi nexus table: segment index " + std::to_string(seg_host[j]) + " of key " +
                                     std::to_string(j) + " is outside [0, " + std::to_string(n_segments) + ")");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    DDR_HIP(hipMemcpyAsync(keys, keys_host, sizeof(int64_t) * (size_t)n_keys, hipMemcpyHostToDevice, s));
    DDR_HIP(hipMemcpyAsync(key_seg, seg_host, sizeof(int32_t) * (size_t)n_keys, hipMemcpyHostToDevice, s));
    DDR_HIP(hipStreamSynchronize(s));  // (the host arrays are the caller's again on return)
    return DDR_OK;
  })
}
ddr_status ddr_bmi_nexus_plan(int64_t n_ids, const int32_t* ids, int64_t n_keys, const int64_t* keys,
                              const int32_t* key_seg, int64_t n_segments, int32_t* src_of_seg, void* stream) {
  DDR_GUARD({
    if (n_ids < 0 || n_keys < 0 || n_segments < 0) return fail(DDR_ERR_ARG, "bmi nexus plan: negative size");
    if (n_ids > INT32_MAX || n_segments > INT32_MAX)
      return fail(DDR_ERR_ARG, "bmi nexus plan: more ids or segments than int32 indices");
    if ((n_segments > 0 && !src_of_seg) || (n_ids > 0 && !ids) || (n_keys > 0 && (!keys || !key_seg)))
      return fail(DDR_ERR_ARG, "bmi nexus plan: null argument");
    DDR_HIP(launch_bmi_nexus_plan(n_ids, ids, n_keys, keys, key_seg, n_segments, src_of_seg,
                                  static_cast<hipStream_t>(stream)));
    return DDR_OK;
  })
}
ddr_status ddr_bmi_set_inflow_f64(int64_t n_segments, const int32_t* src, int64_t n_flows, const double* flows,
                                  double* lateral, void* stream) {
  DDR_GUARD({
    if (n_segments < 0 || n_flows < 0) return fail(DDR_ERR_ARG, "bmi set inflow: negative size");
    if (n_segments > 0 && n_flows > 0 && (!src || !flows || !lateral))
      return fail(DDR_ERR_ARG, "bmi set inflow: null argument");
    DDR_HIP(launch_bmi_set_inflow(n_segments, src, n_flows, flows, lateral, static_cast<hipStream_t>(stream)));
    return DDR_OK;
  })
}
ddr_status ddr_bmi_window_f32(int64_t n_segments, int32_t n_rows, int32_t n_steps, int32_t linear, double* prev,
                              double* cur, float* window, int64_t row_stride, void* stream) {
  DDR_GUARD({
    if (n_segments < 0) return fail(DDR_ERR_ARG, "bmi window: negative size");
    if (n_rows < 1 || n_steps < n_rows)
      return fail(DDR_ERR_ARG, "bmi window: need 1 <= n_rows <= n_steps (got " + std::to_string(n_rows) + ", " +
                                   std::to_string(n_steps) + ")");
    if (row_stride < n_segments) return fail(DDR_ERR_ARG, "bmi window: row_stride is shorter than a row");
    if (n_segments > 0 && (!prev || !cur || !window)) return fail(DDR_ERR_ARG, "bmi window: null argument");
    DDR_HIP(launch_bmi_window(n_segments, n_rows, n_steps, linear != 0, prev, cur, window, row_stride,
                              static_cast<hipStream_t>(stream)));
    return DDR_OK;
  })
}
ddr_status ddr_bmi_outputs_f32(int64_t n_segments, const float* discharge, const float* n_manning,
                               const float* q_spatial, const float* p_spatial, int64_t p_stride, const float* slope,
                               const float* top_width, const float* side_slope, double depth_lb,
                               double bottom_width_lb, float* out, int64_t out_stride, void* stream) {
  DDR_GUARD({
    if (n_segments < 0) return fail(DDR_ERR_ARG, "bmi outputs: negative size");
    if (p_stride != 0 && p_stride != 1) return fail(DDR_ERR_ARG, "bmi outputs: p_stride must be 0 or 1");
    if (out_stride < n_segments) return fail(DDR_ERR_ARG, "bmi outputs: out_stride is shorter than a row");
    if (n_segments > 0 &&
        (!discharge || !n_manning || !q_spatial || !p_spatial || !slope || !top_width || !side_slope || !out))
      return fail(DDR_ERR_ARG, "bmi outputs: null argument");
    DDR_HIP(launch_bmi_outputs(n_segments, discharge, n_manning, q_spatial, p_spatial, p_stride, slope, top_width,
                               side_slope, (float)depth_lb, (float)bottom_width_lb, out, out_stride,
                               static_cast<hipStream_t>(stream)));
    return DDR_OK;
  })
}
int64_t ddr_clip_adam_work_bytes(void) { return (int64_t)clip_adam_work_bytes(); }
int64_t ddr_daily_objective_work_bytes(int64_t n_gauges) {
  if (n_gauges < 0 || n_gauges > kObjectiveMaxGauges) return -1;
  return (int64_t)objective_work_bytes(n_gauges);
}
ddr_status ddr_clip_adam_f32(int64_t n, float* params, const float* grad, float* m, float* v, float lr, double beta1,
                             double beta2, float eps, float* step, float max_norm, float* norm_out, void* work,
                             void* stream) {
  DDR_GUARD({ return clip_adam_impl(n, params, grad, m, v, lr, beta1, beta2, eps, step, max_norm, norm_out, work, stream); })
}
ddr_status ddr_state_f32(const ddr_graph* g, const float* x_save, int64_t T, int64_t t, double discharge_lb,
                         int32_t flags, float* out, void* stream) {
  DDR_GUARD({ return state_impl<float>(g, x_save, T, t, discharge_lb, flags, out, stream); })
}
ddr_status ddr_state_f64(const ddr_graph* g, const double* x_save, int64_t T, int64_t t, double discharge_lb,
                         int32_t flags, double* out, void* stream) {
  DDR_GUARD({ return state_impl<double>(g, x_save, T, t, discharge_lb, flags, out, stream); })
}
ddr_status ddr_gauge_reduce_f32(const ddr_graph* g, const float* x_save, int64_t T, const ddr_gauges* gz,
                                double qlb, int32_t flags, float* out, void* stream) {
  DDR_GUARD({ return gauge_impl<float>(g, x_save, T, gz, qlb, flags, out, stream); })
}
ddr_status ddr_gauge_reduce_f64(const ddr_graph* g, const double* x_save, int64_t T, const ddr_gauges* gz,
                                double qlb, int32_t flags, double* out, void* stream) {
  DDR_GUARD({ return gauge_impl<double>(g, x_save, T, gz, qlb, flags, out, stream); })
}

ddr_status ddr_gauge_daily_f32(const ddr_graph* g, const float* x_save, int64_t T, const ddr_gauges* gz,
                               double qlb, int32_t flags, int64_t t0, int64_t L, int64_t D, float* out,
                               void* stream) {
  DDR_GUARD({ return gauge_daily_impl<float>(g, x_save, T, gz, qlb, flags, t0, L, D, out, stream); })
}
ddr_status ddr_gauge_daily_f64(const ddr_graph* g, const double* x_save, int64_t T, const ddr_gauges* gz,
                               double qlb, int32_t flags, int64_t t0, int64_t L, int64_t D, double* out,
                               void* stream) {
  DDR_GUARD({ return gauge_daily_impl<double>(g, x_save, T, gz, qlb, flags, t0, L, D, out, stream); })
}
ddr_status ddr_gauge_daily_seed_f32(int64_t G, int64_t T, int64_t t0, int64_t L, int64_t D, const float* grad_daily,
                                    float* grad_hourly, void* stream) {
  DDR_GUARD({ return gauge_daily_seed_impl<float>(G, T, t0, L, D, grad_daily, grad_hourly, stream); })
}
ddr_status ddr_gauge_daily_seed_f64(int64_t G, int64_t T, int64_t t0, int64_t L, int64_t D, const double* grad_daily,
                                    double* grad_hourly, void* stream) {
  DDR_GUARD({ return gauge_daily_seed_impl<double>(G, T, t0, L, D, grad_daily, grad_hourly, stream); })
}

ddr_status ddr_period_daily_f32(const ddr_graph* g, const float* x_save, int64_t T, const ddr_gauges* gz, double qlb,
                                int32_t flags, int64_t h0, int64_t first_hour, int64_t n_days, float* daily,
                                void* stream) {
  DDR_GUARD({ return period_daily_impl<float>(g, x_save, T, gz, qlb, flags, h0, first_hour, n_days, daily, stream); })
}
ddr_status ddr_period_daily_f64(const ddr_graph* g, const double* x_save, int64_t T, const ddr_gauges* gz, double qlb,
                                int32_t flags, int64_t h0, int64_t first_hour, int64_t n_days, double* daily,
                                void* stream) {
  DDR_GUARD({ return period_daily_impl<double>(g, x_save, T, gz, qlb, flags, h0, first_hour, n_days, daily, stream); })
}

ddr_status ddr_geometry_stats_f32(const float* q_daily, int64_t reach_stride, int64_t day_stride, int64_t n,
                                  int64_t days, const float* n_manning, const float* p_spatial, int64_t p_stride,
                                  const float* q_spatial, const float* slope, double depth_lb,
                                  double bottom_width_lb, float* out, void* stream) {
  DDR_GUARD({
    // the long-window kernel sorts one variable of a reach in LDS: 4 B per day, the next power of two
    if (n < 0 || days < 1 || days > kGeoLongMaxDays)
      return fail(DDR_ERR_ARG, "geometry statistics: need 1 <= days <= " + std::to_string(kGeoLongMaxDays));
    if (n > 0 && (!q_daily || !n_manning || !p_spatial || !q_spatial || !slope || !out))
      return fail(DDR_ERR_ARG, "null geometry statistics argument");
    if (p_stride != 0 && p_stride != 1) return fail(DDR_ERR_ARG, "p_stride must be 0 or 1");
    DDR_HIP(launch_geometry_stats(q_daily, reach_stride, day_stride, n, days, n_manning, p_spatial, p_stride,
                                  q_spatial, slope, (float)depth_lb, (float)bottom_width_lb, out,
                                  static_cast<hipStream_t>(stream)));
    return DDR_OK;
  })
}

int64_t ddr_lin_work_bytes(const ddr_graph* g, int64_t F, int32_t real_bytes) {
  if (!g || F < 1 || (real_bytes != 4 && real_bytes != 8)) return -1;
  return (int64_t)align16((size_t)real_bytes * (size_t)(reinterpret_cast<const Graph*>(g)->n * F));
}
ddr_status ddr_lin_route_f32(const ddr_graph* g, const float* k, const float* x, double dt, int64_t S, int64_t F,
                             const float* qext, const float* flow_scale, const uint8_t* valid, const float* q0,
                             int32_t flags, float* out, float* q_last, void* workspace, double* bnd, void* status,
                             void* stream) {
  DDR_GUARD({ return lin_route_impl<float>(g, k, x, dt, S, F, qext, flow_scale, valid, q0, flags, out, q_last, workspace, bnd, status, stream); })
}
ddr_status ddr_lin_route_f64(const ddr_graph* g, const double* k, const double* x, double dt, int64_t S, int64_t F,
                             const double* qext, const double* flow_scale, const uint8_t* valid, const double* q0,
                             int32_t flags, double* out, double* q_last, void* workspace, double* bnd, void* status,
                             void* stream) {
  DDR_GUARD({ return lin_route_impl<double>(g, k, x, dt, S, F, qext, flow_scale, valid, q0, flags, out, q_last, workspace, bnd, status, stream); })
}
ddr_status ddr_lin_gauge_f32(int64_t N, int64_t F, const ddr_gauges* gauges, const float* nf, float* out, void* stream) {
  DDR_GUARD({ return lin_gauge_impl<float>(N, F, gauges, nf, out, stream); })
}
ddr_status ddr_lin_gauge_f64(int64_t N, int64_t F, const ddr_gauges* gauges, const double* nf, double* out,
                             void* stream) {
  DDR_GUARD({ return lin_gauge_impl<double>(N, F, gauges, nf, out, stream); })
}

ddr_status ddr_graph_status(const void* status, void* stream) {
  if (!status) return fail(DDR_ERR_ARG, "null status");
  unsigned h[2] = {0, 0};
  DDR_HIP(hipMemcpyAsync(h, status, sizeof(h), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
  DDR_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  if (h[0]) return fail(DDR_ERR_TIMEOUT, std::to_string(h[0]) + " inter-workgroup hand-offs timed out (first block " +
                                             std::to_string((int)h[1] - 1) + ")");
  return DDR_OK;
}

ddr_status ddr_status_check(int32_t wait) {
  DDR_GUARD({ return g_pending.check(wait != 0); })
}

ddr_status ddr_set_debug_flags(int32_t flags) {
  g_debug = ((flags & DDR_DEBUG_FORCE_TIMEOUT) ? kFlagForceTimeout : 0) | ((flags & DDR_DEBUG_NO_STEADY) ? kFlagNoSteady : 0) |
            ((flags & DDR_DEBUG_NO_STORER) ? kFlagNoStorer : 0) | ((flags & DDR_DEBUG_NO_PLAIN) ? kFlagNoPlain : 0);
  return DDR_OK;
}

ddr_status ddr_set_kernel_timing(int32_t enable) {
  g_timing.on = enable != 0;
  return DDR_OK;
}

ddr_status ddr_kernel_ms(int32_t which, float* ms) {
  if ((which != 0 && which != 1) || !ms) return fail(DDR_ERR_ARG, "bad ddr_kernel_ms arguments");
  if (!g_timing.recorded[which]) return fail(DDR_ERR_ARG, "no timed launch recorded");
  DDR_HIP(hipEventSynchronize(g_timing.ev[which][1]));
  DDR_HIP(hipEventElapsedTime(ms, g_timing.ev[which][0], g_timing.ev[which][1]));
  return DDR_OK;
}

ddr_status ddr_set_block_profile(int32_t which, uint64_t* buf) {
  if (which != 0 && which != 1) return fail(DDR_ERR_ARG, "which must be 0 or 1");
  g_prof[which] = reinterpret_cast<unsigned long long*>(buf);
  return DDR_OK;
}

ddr_status ddr_device_info(int32_t* n_cu, int32_t* max_resident) {
  int dev = 0;
  DDR_HIP(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  DDR_HIP(hipGetDeviceProperties(&prop, dev));
  if (n_cu) *n_cu = prop.multiProcessorCount;
  if (max_resident) *max_resident = prop.multiProcessorCount;
  return DDR_OK;
}

const char* ddr_last_error(void) { return ddr::last_error_cstr(); }
#ifndef DDR_SOURCE_HASH
#define DDR_SOURCE_HASH "unknown"
#endif
// src: every library source; kern: the routing kernels' sources only (the Makefile's KERN_SRCS: the routing units and
// the headers they include) -- the key of the PMC counter files under profiles/counters (bench.py), which describe the
// kernels and stay valid across host-side changes.  The kernel hash is the last word.
#ifndef DDR_KERNEL_HASH
#define DDR_KERNEL_HASH "unknown"
#endif
const char* ddr_version(void) { return "ddr_mc 0.2.0 (gfx950) src " DDR_SOURCE_HASH " kern " DDR_KERNEL_HASH; }

}  // extern "C"
