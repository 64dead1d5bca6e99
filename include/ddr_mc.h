/*
 * ddr_mc.h -- C ABI of the MI355X-native Muskingum-Cunge routing hot path (libddr_mc.so).
 *
 * This is the drop-in boundary for DDR's routing engine (taddyb/ddr, src/ddr/routing).  Every entry
 * point takes plain pointers and sizes; device pointers are caller-allocated (e.g. by the PyTorch
 * caching allocator) and never freed by the library.  All work is enqueued on the caller's stream.
 * No C++ exception crosses this boundary: every call returns a ddr_status (0 = OK, < 0 = error)
 * and ddr_last_error() returns a thread-local message.
 *
 * Reference interfaces each entry point replaces (file:line in /root/reference):
 *   ddr_graph_build     src/ddr/geodatazoo/merit.py:197-223 (COO union -> scipy .tocsr())
 *                       + src/ddr/routing/utils.py:25-163 (PatternMapper / get_network_idx)
 *   ddr_graph_upload    (host build on a loader thread, then upload: the per-batch graph of training)
 *   ddr_graph_build_device  the same build on the device from a device-resident COO (merit.py:197-223,
 *                       builders.py:55-109 per training batch; north star (1))
 *   ddr_graph_csr       scipy.sparse.coo_matrix(...).tocsr() canonical CSR (bit-exact target)
 *   ddr_collate_gauges  src/ddr/io/builders.py:55-109 construct_network_matrix + merit.py:197-238
 *                       (per-batch gauge union, compression, outflow_idx); _device: the same on the device
 *   ddr_mc_forward      src/ddr/routing/mmc.py:365-443 (MuskingumCunge.forward) with
 *                       mmc.py:487-559 (route_timestep), mmc.py:25-66 (compute_hotstart_discharge),
 *                       mmc.py:102-168 + geometry/trapezoidal.py:14-108 (celerity),
 *                       mmc.py:460-485 (coefficients), routing/utils.py:535-627 (solver forward)
 *   ddr_mc_backward     torch autograd of the above + routing/utils.py:629-692 (solver backward,
 *                       _backward_cpu 188-242 / _backward_gpu 245-310, _compute_A_gradients 321-389)
 *   ddr_hotstart_f32    mmc.py:25-66 (compute_hotstart_discharge)
 *   ddr_gauge_reduce    mmc.py:344-363, 405-411, 433-439 (ragged outflow_idx scatter_add)
 *   ddr_tri_solve       routing/utils.py:695 triangular_sparse_solve (general CSR, non-unit diagonal)
 *   ddr_tri_grad_values routing/utils.py:321-389 _compute_A_gradients (gradA = -gradb[row]*x[col])
 *   ddr_lin_route       benchmarks/src/ddr_benchmarks/benchmark.py:121-234 (the fixed-parameter linear arm,
 *                       DiffRoute's LTIRouter with irf_fn="muskingum"), as RAPID's Muskingum scheme
 */
#ifndef DDR_MC_H
#define DDR_MC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int ddr_status;
enum {
  DDR_OK = 0,
  DDR_ERR_ARG = -1,           /* bad argument / shape                                  */
  DDR_ERR_NOT_LOWER = -2,     /* adjacency not strictly lower triangular (unsorted)     */
  DDR_ERR_NOT_DENDRITIC = -3, /* a reach drains into more than one downstream reach     */
  DDR_ERR_DUPLICATE = -4,     /* duplicate edge (summed value != 1)                     */
  DDR_ERR_HIP = -5,           /* HIP runtime error                                      */
  DDR_ERR_CAPACITY = -6,      /* graph does not fit the co-resident grid of this device */
  DDR_ERR_TIMEOUT = -7,       /* an inter-workgroup hand-off timed out (device status)  */
  DDR_ERR_SINGULAR = -8       /* zero on the diagonal (ddr_tri_solve)                   */
};

/* Opaque river-graph handle: canonical CSR, dendritic down[] pointers, basin/piece partition and the
 * per-workgroup schedule, uploaded to the current device.  Immutable after build: safe to share
 * across host threads and streams on its device. */
typedef struct ddr_graph ddr_graph;

enum { DDR_BUILD_HOST_ONLY = 1 };

typedef struct {
  int32_t flags;              /* DDR_BUILD_HOST_ONLY: validate/partition, no upload  [in]  */
  int32_t max_block_reaches;  /* cap on reaches per workgroup (0 = auto)             [in]  */
  int32_t target_blocks;      /* desired workgroups (0 = auto: CU count)             [in]  */
  int32_t max_resident;       /* co-resident workgroups of the device (0 = query)    [in]  */
  int32_t steps_hint;         /* expected timesteps per launch, for load balancing   [in]  */
                              /* (0 = 8760; any T is correct, this only weighs work)       */
} ddr_build_opts;

typedef struct {
  int64_t n;              /* reaches                                                      */
  int64_t nnz;            /* edges after canonicalisation                                  */
  int64_t n_basins;       /* connected components (outlet basins)                          */
  int64_t n_pieces;       /* schedulable pieces after splitting large basins               */
  int64_t n_blocks;       /* workgroups of one routing launch                              */
  int64_t n_cut;          /* inter-workgroup edges                                         */
  int64_t max_depth;      /* longest reach-to-outlet path (hops + 1)                       */
  int64_t max_block_depth;/* max over workgroups of the in-piece depth                    */
  int64_t reaches_per_thread; /* KR of the routing kernel instantiation                   */
  int64_t save_elems_per_t;   /* x_save elements = save_elems_per_t * T + save_elems_fixed  */
  int64_t save_elems_fixed;
  int64_t bnd_elems_per_t;    /* forward boundary buffer doubles = bnd_elems_per_t * T     */
  int64_t bwd_elems_per_t;    /* backward workspace doubles = bwd_elems_per_t * T + bwd_elems_fixed */
  int64_t bwd_elems_fixed;
  int64_t status_bytes;       /* device status word block (zeroed by the library)          */
  int64_t generations;        /* 1: every workgroup of a launch co-resident (time-pipelined);  */
                              /* g > 1: blocks exceed the device, they run in ~g waves       */
} ddr_graph_info;

/* Build from a host COO (rows = downstream reach, cols = upstream reach, int32, E entries), the
 * ddr-engine zarr contract (engine/src/ddr_engine/core/zarr_io.py:7-76).  Validates lower
 * triangularity and dendritic structure, canonicalises (rows sorted, columns ascending), splits
 * and packs basins into workgroups, and uploads the schedule to the current HIP device.
 * Synchronous (the only host-synchronising call besides ddr_graph_status). */
ddr_status ddr_graph_build(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                           const ddr_build_opts* opts, ddr_graph** out);
/* The same host build with the schedule upload stream-ordered on `stream` (SURVEY §8(b)'s
 * ddr_graph_build(..., hipStream_t, ...)): one pinned staging block, one pooled device block, one copy on
 * `stream`; routing launches on any stream wait for it (no hipMalloc / device-wide synchronisation).
 * The host part (validation, partition) is synchronous and returns the counts, as ddr_graph_build. */
ddr_status ddr_graph_build_async(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                                 const ddr_build_opts* opts, void* stream, ddr_graph** out);
/* The same build from a COO in DEVICE memory (rows / cols: int32 device pointers on the current HIP
 * device), computed on the device on `stream` (north star (1)): validation, canonical CSR, distance
 * to outlet, basins, the stem-preserving split and the whole per-workgroup schedule are device
 * passes; only the packing of the pieces (a few thousand) runs on the host, between two small reads
 * of the device per split pass.  The schedule equals ddr_graph_build's for the same COO, bit for bit
 * (ddr_graph_fingerprint).  Returns once the graph is complete on `stream`; its arrays are
 * device-resident (ddr_graph_csr / ddr_graph_structure copy them to the host on request). */
ddr_status ddr_graph_build_device(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                                  const ddr_build_opts* opts, void* stream, ddr_graph** out);
/* The same build in two halves, for a training loop that builds batch k + d while it trains on batch
 * k, all on its own stream: _begin enqueues every device pass up to the piece table and its copy to
 * pinned host memory and returns at once (no host wait); _finish waits for that copy (long complete
 * when begun a step or more ahead), packs the pieces on the host and enqueues the schedule emission
 * on the same stream.  _finish consumes the pending build (also on error); _cancel drops one unused.
 * rows / cols must stay valid until _finish returns. */
typedef struct ddr_graph_pending ddr_graph_pending;
ddr_status ddr_graph_build_device_begin(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols,
                                        const ddr_build_opts* opts, void* stream, ddr_graph_pending** out);
ddr_status ddr_graph_build_device_finish(ddr_graph_pending* p, ddr_graph** out);
ddr_status ddr_graph_build_device_cancel(ddr_graph_pending* p);
/* FNV-1a hash of a graph's whole schedule (per-reach arrays, block descriptors): equal for a host and
 * a device build of the same COO and options.  Synchronous (copies the device schedule). */
ddr_status ddr_graph_fingerprint(const ddr_graph* g, uint64_t* fp);
/* Per-batch gauge union, replacing construct_network_matrix (src/ddr/io/builders.py:55-109) and the
 * compression steps of Merit._collate_gages (src/ddr/geodatazoo/merit.py:197-238; Lynker twin
 * lynker_hydrofabric.py:198-266).  Host, O(E + n_conus), no device.
 *   in : n_conus; n_gauges subsets as one COO in CONUS numbering, subset g = entries
 *        [sub_off[g], sub_off[g+1]) of rows (downstream) / cols (upstream); gage_idx[g] (CONUS).
 *   out: active[n_active] CONUS ids of the union's reaches, ascending (capacity: min(n_conus,
 *        2 E + n_gauges)); crow[n_active + 1], col[nnz] canonical CSR of the compressed union
 *        (capacity of col: E); out_off[n_gauges + 1], out_idx (out_idx_cap entries; E + n_gauges
 *        suffices for consistent subsets, DDR_ERR_ARG when the lists would exceed it): outflow_idx
 *        of each gauge, the compressed upstream reaches of its reach ascending (itself when it has
 *        none); gage_c[n_gauges] each gauge's compressed index.
 * Rejects non-lower-triangular entries (DDR_ERR_NOT_LOWER) and a union in which a reach drains into
 * two reaches (DDR_ERR_NOT_DENDRITIC). */
ddr_status ddr_collate_gauges(int64_t n_conus, int64_t n_gauges, const int64_t* sub_off, const int32_t* rows,
                              const int32_t* cols, const int32_t* gage_idx, int32_t* active, int64_t* n_active,
                              int64_t* crow, int32_t* col, int64_t* nnz, int64_t* out_off, int32_t* out_idx,
                              int64_t out_idx_cap, int32_t* gage_c);
/* The same union on the device (all arrays device memory on the current HIP device, work on `stream`):
 * the subsets concatenated into one COO of e entries (rows / cols, CONUS numbering; the subset
 * boundaries do not matter to the union).  Outputs: active (active_cap entries) and *n_active (host);
 * the compressed union as a COO rows_c / cols_c (ascending cols; capacity e) with *nnz (host) entries
 * -- the input of ddr_graph_build_device -- and as canonical CSR crow (int64, n_active + 1) / col
 * (capacity e); out_off (int64, n_gauges + 1) / out_idx (out_idx_cap) and gage_c as
 * ddr_collate_gauges.  Bit-identical to ddr_collate_gauges; synchronous (returns the counts). */
ddr_status ddr_collate_gauges_device(int64_t n_conus, int64_t n_gauges, int64_t e, const int32_t* rows,
                                     const int32_t* cols, const int32_t* gage_idx, int32_t* active, int64_t active_cap,
                                     int64_t* n_active, int32_t* rows_c, int32_t* cols_c, int64_t* nnz, int64_t* crow,
                                     int32_t* col, int64_t* out_off, int32_t* out_idx, int64_t out_idx_cap,
                                     int32_t* gage_c, void* stream);
/* Upload the schedule of a graph built with DDR_BUILD_HOST_ONLY to the current HIP device (no-op
 * if already uploaded).  The host build needs no device: it can run on any host thread (e.g. a
 * data-loader worker preparing the next training batch, merit.py:197-223) while the device routes
 * the current one; only this step touches the device.  Synchronous. */
ddr_status ddr_graph_upload(ddr_graph* g);
/* ddr_graph_upload stream-ordered on `stream` (as ddr_graph_build_async): returns without a host wait. */
ddr_status ddr_graph_upload_async(ddr_graph* g, void* stream);
/* Any graph size builds: workgroups take ticket-ordered logical blocks, so a schedule with more
 * blocks than co-resident workgroups still completes (ddr_graph_info.generations > 1).
 * ddr_graph_destroy is synchronous: a graph with pooled (stream-ordered) memory waits for the device. */
ddr_status ddr_graph_destroy(ddr_graph* g);
/* Destroy a graph whose last use is queued on `stream`: a device-built graph's memory is released
 * stream-ordered (no device-wide synchronisation -- the per-batch graphs of a training loop); a
 * host-built one's as ddr_graph_destroy. */
ddr_status ddr_graph_destroy_async(ddr_graph* g, void* stream);
/* Release every idle block of the library's memory pools (device blocks of device-built graphs and
 * async uploads, pinned staging blocks) whose last user's queued work has finished; *freed_bytes
 * (may be NULL) receives the bytes returned to HIP.  Blocks handed out or still in use stay. */
ddr_status ddr_pool_trim(int64_t* freed_bytes);
ddr_status ddr_graph_get_info(const ddr_graph* g, ddr_graph_info* info);
/* Canonical CSR of the adjacency into host buffers: crow (n+1), col (nnz), int64. */
ddr_status ddr_graph_csr(const ddr_graph* g, int64_t* crow, int64_t* col);
/* Host copies of the dendritic structure: down (n, -1 = outlet), dist (n, hops to outlet),
 * basin (n, outlet reach id), block (n, workgroup id), each int64; any pointer may be NULL. */
ddr_status ddr_graph_structure(const ddr_graph* g, int64_t* down, int64_t* dist, int64_t* basin,
                               int64_t* block);

/* Physical constants of the routing step (mmc.py:192-208, trapezoidal.py:79, mmc.py:166). */
typedef struct {
  double dt;             /* seconds per step (3600; BMI may override, ddr_bmi.py:208) */
  double discharge_lb;   /* q_lb */
  double velocity_lb;
  double velocity_ub;    /* 15 */
  double depth_lb;
  double bottom_width_lb;
  double side_slope_lb;  /* 0.5 */
  double side_slope_ub;  /* 50 */
} ddr_mc_consts;

/* Per-reach inputs in the reference reach order.  Element type is float for the *_f32 entry
 * points and double for the *_f64 ones.  p_spatial may be a single value (p_stride = 0). */
typedef struct {
  const void* n;           /* Manning n, denormalised                 (N)   */
  const void* q_spatial;   /* Leopold & Maddock exponent, denormalised  (N)   */
  const void* p_spatial;   /* Leopold & Maddock coefficient        (N) or (1) */
  int64_t p_stride;        /* 1 (per reach) or 0 (scalar)                     */
  const void* length;      /* m                                         (N)   */
  const void* slope;       /* already clamped at the slope minimum     (N)   */
  const void* x_storage;   /* Muskingum X                               (N)   */
  const void* flow_scale;  /* optional per-reach q' multiplier (N) or NULL    */
  int64_t qprime_hours;    /* hours per stored q' row: 0/1 hourly (T, N); 24 a daily */
                           /* store (ceil(T / 24), N), indexed q'[t / 24] in-kernel, */
                           /* the reader's repeat(24) (readers.py:513-519)           */
  const uint8_t* qprime_valid; /* optional (N): 0 = divide missing from the store, */
                           /* its q' is 0.001 (readers.py:523-530); NULL = all valid */
} ddr_mc_reaches;

/* Gauge mode: out[g, t] = sum_{k in [off[g], off[g+1])} Q_t[idx[k]] (device int64 arrays,
 * indices already normalised to [0, N)); reach_offsets/reach_gauges list, per reach, the gauges
 * (with multiplicity) whose outflow set contains it. */
typedef struct {
  int64_t n_gauges;
  const int64_t* offsets;        /* (G+1)                                         */
  const int64_t* index;          /* (offsets[G]) reach ids                         */
  const int64_t* reach_offsets;  /* (N+1) inverse map used by the backward        */
  const int64_t* reach_gauges;   /* (offsets[G]) gauge id of each membership      */
} ddr_gauges;

/* DDR_FWD_SAVE_X is accepted for compatibility: x_save is always written.
 * DDR_FWD_ACCUMULATE: every step is a hot start, Q_t = max((I - N)^-1 q'_t, q_lb) with step t
 * reading q' row t -- the per-day discharge accumulation of scripts/geometry_predictor.py:193-212
 * (compute_hotstart_discharge, mmc.py:25-66) for all days in one launch. */
/* Forward coefficient arithmetic (fp32 only; default: the reference's operation order with IEEE
 * division and a correctly rounded pow -- bit-identical to the oracle):
 * DDR_FWD_FAITHFUL_MATH: the same operation order and IEEE divisions, pow in fp32 faithful-class
 *   arithmetic (like the reference's own Sleef powf; no fp64 on the chain);
 * DDR_FWD_FAST_MATH: hardware v_rcp / v_log / v_exp throughout (~1e-6 relative per coefficient). */
enum { DDR_FWD_SAVE_X = 1, DDR_FWD_CARRY = 2, DDR_FWD_NO_RUNOFF = 4, DDR_FWD_ACCUMULATE = 8, DDR_FWD_FAST_MATH = 16,
       DDR_FWD_FAITHFUL_MATH = 32, DDR_FWD_CHECK_QPRIME = 64, DDR_BWD_EXACT_ADJOINT = 128 };
/* DDR_BWD_EXACT_ADJOINT (backward flag, fp32; ignored by the forward): the adjoint of the fp32 trajectory the
 * forward computed to ~1e-6 on any depth.  dL/dk (the Muskingum K) is a sum of O(Q) terms that cancels to the
 * step's discharge change; by default the fp32 adjoint takes that change as Q(t-1) - x(t) from the stored
 * fp32 state (no q' re-read), which carries x's rounding into it: ~1e-3 of the gradient on a 2215-deep
 * basin, ~1e-7 on shallow ones.  With the flag it forms the step's mass imbalances Q(t-1) - q'c - sum x_j(t)
 * and Q(t-1) - q'c - I(t) exactly (fp64 upstream sums, q' re-read): 1.8e-7 there, +30 % backward time. */
/* DDR_FWD_CHECK_QPRIME: the forward also tests the flow-scaled q' of the window for NaN (the reference's
 * cold-start assertion, mmc.py:335) inside its q' gather -- no extra pass over q'.  The verdict of the
 * calling thread's last such launch: ddr_qprime_nan_wait, which waits for the gather only (an event
 * recorded behind it), not for the routing kernel queued after it. */
ddr_status ddr_qprime_nan_wait(int32_t* has_nan);

/* Fused forward over T steps (hot start at t = 0 unless DDR_FWD_CARRY, then q0 is Q_0).
 * Returns DDR_ERR_TIMEOUT instead of launching when an earlier launch's hand-off timed out
 * (ddr_status_check). 
 *   qprime     (T, N) lateral inflow, time-major, reference order
 *   q0         (N) carried discharge (DDR_FWD_CARRY) or NULL
 *   runoff     (N, T), or NULL / DDR_FWD_NO_RUNOFF (e.g. gauges: ddr_gauge_reduce afterwards)
 *   x_save     required workspace (save_elems_per_t * T + save_elems_fixed reals): the routed
 *              states, then q' * flow_scale, both in the schedule layout (runoff is written
 *              by the routing kernel itself); keep it unchanged for ddr_mc_backward
 *   bnd        forward boundary buffer (bnd_elems_per_t * T doubles; may be NULL if n_cut == 0);
 *              must be kept unchanged for ddr_mc_backward
 *   status     device status block (status_bytes)
 *   q_last, top_width_last, side_slope_last (N), any may be NULL */
ddr_status ddr_mc_forward_f32(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                              const float* qprime, int64_t T, const float* q0, float* runoff,
                              float* x_save, double* bnd, void* status, float* q_last,
                              float* top_width_last, float* side_slope_last, int32_t flags,
                              void* stream);
ddr_status ddr_mc_forward_f64(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                              const double* qprime, int64_t T, const double* q0, double* runoff,
                              double* x_save, double* bnd, void* status, double* q_last,
                              double* top_width_last, double* side_slope_last, int32_t flags,
                              void* stream);

/* Hot start (src/ddr/routing/mmc.py:25-66 compute_hotstart_discharge): out = max((I - N)^-1 q, lb) for
 * q (N) in reference order -- the accumulation solve of the routing graph in one launch, fp64 sums as
 * the reference's SciPy solve; device pointers, enqueued on `stream` (its workspace is stream-ordered
 * scratch).  The same sweep is step 0 of every ddr_mc_forward_f32 without DDR_FWD_CARRY. */
ddr_status ddr_hotstart_f32(const ddr_graph* g, const float* q, double discharge_lb, float* out, void* stream);

/* Reverse-time, reverse-topological adjoint.  grad_runoff is (N, T), or (G, T) with gauges != NULL.
 * bwd_bnd is the backward workspace (size in ddr_graph_info).
 * Writes per-reach dL/dn, dL/dq_spatial, dL/dp_spatial (N each; for a scalar p the caller sums). */
ddr_status ddr_mc_backward_f32(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                               const float* qprime, int64_t T, const float* x_save,
                               const double* bnd, const float* grad_runoff, const ddr_gauges* gauges,
                               double* bwd_bnd, void* status, float* grad_n, float* grad_q,
                               float* grad_p, int32_t flags, void* stream);
ddr_status ddr_mc_backward_f64(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                               const double* qprime, int64_t T, const double* x_save,
                               const double* bnd, const double* grad_runoff, const ddr_gauges* gauges,
                               double* bwd_bnd, void* status, double* grad_n, double* grad_q,
                               double* grad_p, int32_t flags, void* stream);

/* State-gradient adjoint: ddr_mc_backward plus the gradients the reference's autograd delivers to
 * the lateral inflow and the discharge state (routing/mmc.py:487-559 route_timestep is
 * differentiable w.r.t. q_prime_clamp and _discharge_t; the hot start mmc.py:25-66 w.r.t. q'[0]):
 *   grad_qprime (qprime_rows, N) dL/dq' in the caller's store layout (rows of qprime_hours steps;
 *               flow_scale applied, 0 for a divide filled by qprime_valid), or NULL
 *   grad_q0     (N) dL/dQ0 of a carried state (forward run with DDR_FWD_CARRY), or NULL
 *   work        device workspace of ddr_state_work_bytes(g, T, n_gauges, sizeof(real)) bytes
 * Replaces: torch autograd through mmc.py:421-424 (q' clamp), 535-538 (c4 q'), 25-66 (hot start)
 * and the carried _discharge_t (mmc.py:330-342). */
int64_t ddr_state_work_bytes(const ddr_graph* g, int64_t T, int64_t n_gauges, int32_t real_bytes);
ddr_status ddr_mc_backward_state_f32(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                                     const float* qprime, int64_t qprime_rows, int64_t T, const float* x_save,
                                     const double* bnd, const float* grad_runoff, const ddr_gauges* gauges,
                                     double* bwd_bnd, void* status, float* grad_n, float* grad_q,
                                     float* grad_p, float* grad_qprime, float* grad_q0, void* work,
                                     int32_t flags, void* stream);
ddr_status ddr_mc_backward_state_f64(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                                     const double* qprime, int64_t qprime_rows, int64_t T, const double* x_save,
                                     const double* bnd, const double* grad_runoff, const ddr_gauges* gauges,
                                     double* bwd_bnd, void* status, double* grad_n, double* grad_q,
                                     double* grad_p, double* grad_qprime, double* grad_q0, void* work,
                                     int32_t flags, void* stream);

/* The general adjoint: ddr_mc_backward_state (grad_qprime, grad_q0 and work may be NULL: with both NULL
 * this is ddr_mc_backward) plus per-reach gradients into the discharge state itself:
 *   state_seed  (2, N) reference order, or NULL: row 0 dL/dQ_{T-1} -- the final state `_discharge_t`
 *               (mmc.py:441, retained by dmc, torch_mc.py:196-216; an ordinary autograd tensor in gauge
 *               mode too, mmc.py:433-441) -- and row 1 dL/dQ_{T-2}, the state the reported top width /
 *               side slope of the last step were computed from (mmc.py:161-162; the caller forms it by
 *               differentiating that geometry, e.g. from ddr_state_f32's Q_{T-2})
 * Replaces: torch autograd through `_discharge_t` and `top_width` / `side_slope` after a forward. */
ddr_status ddr_mc_backward_ex_f32(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                                  const float* qprime, int64_t qprime_rows, int64_t T, const float* x_save,
                                  const double* bnd, const float* grad_runoff, const ddr_gauges* gauges,
                                  const float* state_seed, double* bwd_bnd, void* status, float* grad_n,
                                  float* grad_q, float* grad_p, float* grad_qprime, float* grad_q0, void* work,
                                  int32_t flags, void* stream);
ddr_status ddr_mc_backward_ex_f64(const ddr_graph* g, const ddr_mc_consts* c, const ddr_mc_reaches* r,
                                  const double* qprime, int64_t qprime_rows, int64_t T, const double* x_save,
                                  const double* bnd, const double* grad_runoff, const ddr_gauges* gauges,
                                  const double* state_seed, double* bwd_bnd, void* status, double* grad_n,
                                  double* grad_q, double* grad_p, double* grad_qprime, double* grad_q0,
                                  void* work, int32_t flags, void* stream);

/* Q_t (N, reference order) from a forward's saved states: max(x(t), discharge_lb), or x(0) unclamped for a
 * carried state (flags & DDR_FWD_CARRY) -- the routed discharge the reference holds as `_discharge_t`
 * after step t (mmc.py:441, 557).  Enqueued on `stream`; 0 <= t < T.
 * Replaces: reading MuskingumCunge._discharge_t / output[:, t] mid-window (mmc.py:428-441). */
ddr_status ddr_state_f32(const ddr_graph* g, const float* x_save, int64_t T, int64_t t, double discharge_lb,
                         int32_t flags, float* out, void* stream);
ddr_status ddr_state_f64(const ddr_graph* g, const double* x_save, int64_t T, int64_t t, double discharge_lb,
                         int32_t flags, double* out, void* stream);

/* Fused parameter network of the C3 training step (the bench's stand-in for the reference's KAN,
 * src/ddr/nn/kan.py:11-62, whose pykan dependency is not installed): attributes x (n_rows, n_features <= 12)
 * -> Linear(F, 128) -> SiLU -> Linear(128, 128) -> SiLU -> Linear(128, 128) -> SiLU -> Linear(128, 3) -> sigmoid
 * -> denormalize (routing/utils.py:166-185: y = u scale + offset, exp(y) for a log-space parameter) ->
 * out_n, out_q, out_p (n_rows each), on the fp32 matrix cores.
 *   params  flat fp32, ddr_pnet_param_count(F) values: W1 (128, F) | b1 (128) | W2 (128, 128) | b2 | W3 | b3 |
 *           W4 (3, 128) | b4 (3), torch.nn.Linear's (out, in) weight layout
 *   denorm  HOST array [3][3]: per output (scale, offset, log-space flag)
 *   z_save  (3, n_rows, 128) pre-activations, u_save (n_rows, 3) sigmoid outputs: kept for the backward
 *   grad_params (same layout as params) = dL/dparams given dL/d(out_n, out_q, out_p); work: device scratch of
 *           ddr_pnet_work_bytes bytes.  Deterministic (fixed-order reduction of per-workgroup partials).
 * Replaces: the network's forward (kan.py:50-62) and its torch autograd in scripts/train.py:54-104. */
int64_t ddr_pnet_param_count(int32_t n_features);
int64_t ddr_pnet_work_bytes(int64_t n_rows, int32_t n_features);
ddr_status ddr_pnet_forward_f32(int64_t n_rows, int32_t n_features, const float* x, const float* params,
                                const float* denorm, float* z_save, float* u_save, float* out_n, float* out_q,
                                float* out_p, void* stream);
ddr_status ddr_pnet_backward_f32(int64_t n_rows, int32_t n_features, const float* x, const float* params,
                                 const float* denorm, const float* z_save, const float* u_save, const float* grad_n,
                                 const float* grad_q, const float* grad_p, float* grad_params, void* work,
                                 void* stream);

/* The reference's parameter network (src/ddr/nn/kan.py:11-62): attributes x (n_rows, F) -> Linear(F, H) ->
 * L pykan KAN([H, H]) layers (grid G, order k, symbolic branch off) -> Linear(H, O) -> sigmoid -> u (n_rows, O)
 * in [0, 1]; the denormalisation stays with the routing engine, as in the reference.  One persistent launch
 * per KAN layer with the Linears fused in (csrc/kan.hip), against ~40 PyTorch launches per layer and an
 * (n_rows, H, G + k) basis tensor.
 * Supported: 1 <= F <= 32, 1 <= H <= 32, 1 <= O <= 8, 1 <= L <= 4, 1 <= k <= 3, G >= 1,
 * H H (G + k) <= 32768, 1 <= n_rows <= 2^30, every knot row strictly increasing (the caller's to check: the
 * knots are device memory); anything else is DDR_ERR_ARG with a message naming the limit.
 *   params  flat fp32, ddr_kan_param_count values: input.weight (H, F) | input.bias (H) | per layer: coef
 *           (H, H, G + k) [in, out, j] | scale_base (H, H) [in, out] | scale_sp (H, H) | output.weight (O, H) |
 *           output.bias (O)
 *   consts  flat fp32, ddr_kan_const_count values, per layer: grid (H, G + 1 + 2k) | mask (H, H) [in, out] |
 *           node_scale (H) | node_bias (H) | subnode_scale (H) | subnode_bias (H)
 *   h_save  (L + 1, n_rows, H): the input Linear's output and every layer's output, kept for the backward;
 *           NULL (inference) saves nothing, and the layers' activations pass through `work`
 *   work    device scratch of ddr_kan_work_bytes(desc, n_rows, backward) bytes
 *   grad_params (layout of params) = dL/dparams given grad_u = dL/du (n_rows, O); no gradient of x.
 *           Bitwise reproducible: no atomics, per-workgroup partials summed in a fixed order.
 * Replaces: ddr.nn.kan's forward (kan.py:50-62, pykan's MultKAN.forward / KANLayer.forward / B_batch) and its
 * torch autograd in scripts/train.py:54-104. */
typedef struct ddr_kan_desc {
  int32_t n_features; /* F */
  int32_t hidden;     /* H */
  int32_t n_outputs;  /* O */
  int32_t n_layers;   /* L */
  int32_t grid;       /* G */
  int32_t k;
} ddr_kan_desc;
int64_t ddr_kan_param_count(const ddr_kan_desc* desc);
int64_t ddr_kan_const_count(const ddr_kan_desc* desc);
int64_t ddr_kan_work_bytes(const ddr_kan_desc* desc, int64_t n_rows, int32_t backward);
ddr_status ddr_kan_forward_f32(const ddr_kan_desc* desc, int64_t n_rows, const float* x, const float* params,
                               const float* consts, float* h_save, float* u, void* work, void* stream);
ddr_status ddr_kan_backward_f32(const ddr_kan_desc* desc, int64_t n_rows, const float* x, const float* params,
                                const float* consts, const float* h_save, const float* u, const float* grad_u,
                                float* grad_params, void* work, void* stream);

/* The tail of a training step (scripts/train.py:91-100), one launch each, device pointers on `stream`:
 * ddr_daily_l1_f32: loss[0] = inv_count * sum_{g, d >= warmup} |daily[g, d] - obs[g, d]| over (G, D) row-major
 *   series, and (grad != NULL) grad[g, d] = inv_count * sign(daily - obs), 0 for d < warmup -- l1_loss
 *   (train.py:91-94; inv_count = 1 / (G (D - warmup)) is its mean) and its backward in one pass.
 * ddr_clip_adam_f32: clip_grad_norm_(max_norm) (train.py:99; max_norm <= 0: none) then one Adam step
 *   (torch.optim.Adam, no weight decay / amsgrad; train.py:100) on a flat parameter vector of n values with
 *   its moments m, v; step is a device fp32 counter (0 before the first step) that the launch increments and
 *   takes the bias corrections from, as torch's capturable Adam does -- no host value, so the launch can be
 *   captured into a graph and replayed.
 *   beta1, beta2 are doubles, as torch.optim.Adam holds them: the moments' weights are fp32(1 - beta) (1 - fp32(0.999)
 *   would be 1.3e-5 off) and the bias corrections 1 - beta^step are formed in double.
 *   norm_out (or NULL) receives the gradient's norm before clipping.  grad is not modified.  work: device
 *   scratch of ddr_clip_adam_work_bytes() bytes.
 * Both deterministic (fixed slices and reduction order).
 * Replaces: the ~15 PyTorch launches of l1_loss + backward, clip_grad_norm_ and Adam.step per step. */
ddr_status ddr_daily_l1_f32(int64_t n_gauges, int64_t n_days, int64_t warmup, const float* daily, const float* obs,
                            float inv_count, float* loss, float* grad, void* stream);
int64_t ddr_clip_adam_work_bytes(void);
ddr_status ddr_clip_adam_f32(int64_t n, float* params, const float* grad, float* m, float* v, float lr, double beta1,
                             double beta2, float eps, float* step, float max_norm, float* norm_out, void* work,
                             void* stream);

/* Masked training objectives over the gauges' daily series: the loss and its gradient w.r.t. the predictions with
 * a NaN observation as a missing day and a dropped gauge as a mask, without a host sync or a change of shape, so a
 * step on real (gappy) observations can be captured.  Replaces scripts/train.py:84-97 -- the filter that drops
 * every gauge whose observation window holds a NaN (boolean indexing: a host wait and a new shape per batch),
 * l1_loss over the rest after the warm-up, and its backward -- and adds per-gauge normalised objectives.
 *   desc    kind (DDR_OBJECTIVE_*), n_gauges G, n_days D (1 <= D <= 8192), warmup w (0 <= w < D: days excluded),
 *           eps >= 0 (NSE only).
 *   daily, obs  device fp32, row g at daily + g * daily_stride / obs + g * obs_stride (strides in elements), D
 *           values each.  daily is the only differentiated input.
 *   drop    device (G,) bytes, non-zero: the gauge contributes nothing (ObservationStore.window's has_nan reproduces
 *           the reference's filter); NULL: none.    weight  device (G,) fp32, >= 0 and finite; NULL: all 1.
 *   count, count_dev  the normaliser W when the caller knows better (ranks that all-reduce their counts): count_dev,
 *           a device fp32 scalar read by the launch (a captured step updates it in place), else count > 0 by value;
 *           count == 0 and count_dev == NULL: W as defined below.
 * For gauge g, V_g = {d >= w : obs[g, d] is not NaN}, empty when drop[g]; n_g = |V_g|.  Over V_g, in fp64 of the fp32
 * inputs: A = sum |p - o|, S = sum (p - o)^2, the means mu_p, mu_o, S_pp = sum (p - mu_p)^2, S_oo = sum (o - mu_o)^2,
 * S_po = sum (p - mu_p)(o - mu_o), sigma = sqrt(S_.. / n_g).
 *   L1   term A / n_g;  MSE  term S / n_g:  used when n_g >= 1;  loss = sum_used w_g n_g term_g / W, W = sum_used
 *        w_g n_g (unit weights: the mean over every counted day; with drop = has_nan, L1 is the reference's
 *        l1_loss(pred[keep][:, w:], target[keep][:, w:])).
 *   NSE  term S / (n_g (sigma_o + eps)^2), 1 - NSE at eps = 0: used when n_g >= 2 and (S_oo != 0 or eps > 0);
 *   KGE  term E = sqrt((r - 1)^2 + (alpha - 1)^2 + (beta - 1)^2), r = S_po / sqrt(S_pp S_oo), alpha = sigma_p /
 *        sigma_o, beta = mu_p / mu_o, 1 - KGE of validation/metrics.py:216-227: used when n_g >= 2 and none of
 *        S_oo == 0, mu_o == 0, S_pp == 0 holds (a NaN prediction keeps the gauge counted);
 *        loss = sum_used w_g term_g / W, W = sum_used w_g.
 * W == 0 (nothing used): loss 0, gradient 0.  A NaN prediction on a day of V_g makes the loss NaN and the gradient
 * NaN at that element at least (KGE: possibly that gauge's row); other gauges' rows are unchanged.
 *   loss    device fp32 scalar.
 *   grad    device fp32 (G, D) row-major or NULL (no gradient launch): d loss / d daily, each element formed in fp64
 *           and rounded once; exactly +0.0 outside V_g and for every gauge that is not used.  L1: w_g sign(p - o) / W
 *           (sign(0) = 0);  MSE: 2 w_g (p - o) / W;  NSE: 2 w_g (p - o) / (W n_g (sigma_o + eps)^2);  KGE: (w_g / W)
 *           [(r - 1) dr + (alpha - 1) dalpha + (beta - 1) dbeta] / E with dr = [(o - mu_o) - r sqrt(S_oo / S_pp)
 *           (p - mu_p)] / sqrt(S_pp S_oo), dalpha = (p - mu_p) / (n_g sigma_p sigma_o), dbeta = 1 / (n_g mu_o); 0
 *           where E == 0.
 *   terms   device fp64 (3, G) or NULL: row 0 the term (NaN when the gauge is not used), row 1 n_g, row 2 used (0/1).
 *   work    device scratch of ddr_daily_objective_work_bytes(G) bytes (8-byte aligned).
 * At most three launches on `stream` (moments per gauge; a fixed-order reduction; the gradient), no atomics, no
 * allocation: results are bitwise repeatable, and a gauge's term and gradient row do not depend on which other
 * gauges are in the batch beyond W.  n_gauges == 0 is a no-op. */
enum { DDR_OBJECTIVE_L1 = 0, DDR_OBJECTIVE_MSE, DDR_OBJECTIVE_NSE, DDR_OBJECTIVE_KGE, DDR_N_OBJECTIVES };
typedef struct ddr_objective_desc {
  int32_t kind;
  int32_t reserved; /* 0 */
  int64_t n_gauges, n_days, warmup;
  double eps;
} ddr_objective_desc;
int64_t ddr_daily_objective_work_bytes(int64_t n_gauges);
ddr_status ddr_daily_objective_f32(const ddr_objective_desc* desc, const float* daily, int64_t daily_stride,
                                   const float* obs, int64_t obs_stride, const uint8_t* drop, const float* weight,
                                   double count, const float* count_dev, float* loss, float* grad, double* terms,
                                   void* work, void* stream);

/* Gauge reduction of a forward's saved states x_save: runoff (G, T). */
ddr_status ddr_gauge_reduce_f32(const ddr_graph* g, const float* x_save, int64_t T,
                                const ddr_gauges* gauges, double discharge_lb, int32_t flags,
                                float* runoff, void* stream);
ddr_status ddr_gauge_reduce_f64(const ddr_graph* g, const double* x_save, int64_t T,
                                const ddr_gauges* gauges, double discharge_lb, int32_t flags,
                                double* runoff, void* stream);

/* Linear Muskingum routing, RAPID's matrix scheme (the fixed-parameter baseline of the reference's
 * benchmarks/ package): per reach C1 = (h - k x) / den, C2 = (h + k x) / den, C3 = (k (1 - x) - h) / den with
 * h = dt / 2, den = k (1 - x) + h, and per sub-step
 *   Q+ = (C1 (In+ + qe) + C2 (In + qe)) + C3 Q,  In+ = sum of the upstream Q+ (upstream-list order)
 * in the routed precision, separately rounded, no clamps.  One persistent launch routes F * S sub-steps.
 *   k, x        (N) storage constant (seconds) and weighting factor; dt: the sub-step in seconds
 *   S, F        sub-steps per forcing interval, forcing intervals; qext (F, N)
 *   flow_scale  (N) or NULL; valid (N) uint8 or NULL (0: forcing 0.001), as the Muskingum-Cunge forward's
 *   q0          (N) initial state or NULL (zeros); DDR_LIN_STEADY (q0 NULL): the steady state of qext row 0,
 *               (I - N)^-1 qext[0] in fp64 (the hot start's sweep)
 *   out         (N, F): the mean of the S states at the beginning of each sub-step (fp64 sum, one rounding;
 *               RAPID's Qout), or with DDR_LIN_END the state after the interval's last sub-step
 *   q_last      (N) the final state (RAPID's Qfinal)
 *   workspace   ddr_lin_work_bytes bytes; bnd: n_cut * (F * S + 1) doubles (NULL without cut edges);
 *   status      device status block (status_bytes)
 * No host synchronisation; capturable.  A split-basin graph is refused. */
enum { DDR_LIN_END = 1, DDR_LIN_STEADY = 2 };
int64_t ddr_lin_work_bytes(const ddr_graph* g, int64_t F, int32_t real_bytes);
ddr_status ddr_lin_route_f32(const ddr_graph* g, const float* k, const float* x, double dt, int64_t S, int64_t F,
                             const float* qext, const float* flow_scale, const uint8_t* valid, const float* q0,
                             int32_t flags, float* out, float* q_last, void* workspace, double* bnd, void* status,
                             void* stream);
ddr_status ddr_lin_route_f64(const ddr_graph* g, const double* k, const double* x, double dt, int64_t S, int64_t F,
                             const double* qext, const double* flow_scale, const uint8_t* valid, const double* q0,
                             int32_t flags, double* out, double* q_last, void* workspace, double* bnd, void* status,
                             void* stream);
/* Gauge rows of an (N, F) output of ddr_lin_route: out (G, F), each gauge's reaches added in list order.
 * (ddr_gauge_reduce reads the Muskingum-Cunge forward's saved states and clamps them; this output has neither.) */
ddr_status ddr_lin_gauge_f32(int64_t N, int64_t F, const ddr_gauges* gauges, const float* nf, float* out, void* stream);
ddr_status ddr_lin_gauge_f64(int64_t N, int64_t F, const ddr_gauges* gauges, const double* nf, double* out,
                             void* stream);

/* Gauge-mode training objective, fused (scripts/train.py:78-82 + io/functions.py:7-23): daily area
 * means of the gauge sums over the trimmed window [t0, t0 + L) of the routed states x_save,
 * out (G, D): day d averages hours t0 + [floor(d L / D), ceil((d + 1) L / D)) like
 * F.interpolate(mode="area").  The reference trims runoff[:, 13 : -11 + tau] and pools to
 * D = L // 24 days: t0 = 13, L = T - 24 + tau. */
ddr_status ddr_gauge_daily_f32(const ddr_graph* g, const float* x_save, int64_t T, const ddr_gauges* gauges,
                               double discharge_lb, int32_t flags, int64_t t0, int64_t L, int64_t D,
                               float* daily, void* stream);
ddr_status ddr_gauge_daily_f64(const ddr_graph* g, const double* x_save, int64_t T, const ddr_gauges* gauges,
                               double discharge_lb, int32_t flags, int64_t t0, int64_t L, int64_t D,
                               double* daily, void* stream);
/* Its adjoint: dL/d(hourly gauge series) (G, T) from dL/d(daily) (G, D), the seed of the gauge-mode
 * ddr_mc_backward (zero outside the trimmed window). */
ddr_status ddr_gauge_daily_seed_f32(int64_t G, int64_t T, int64_t t0, int64_t L, int64_t D,
                                    const float* grad_daily, float* grad_hourly, void* stream);
ddr_status ddr_gauge_daily_seed_f64(int64_t G, int64_t T, int64_t t0, int64_t L, int64_t D,
                                    const double* grad_daily, double* grad_hourly, void* stream);

/* Whole-period inference (scripts/router.py:88-201, scripts/test.py:57-112): the daily means of a period
 * routed in several launches.  Day d of row r is the mean of period hours [first_hour + 24 d,
 * first_hour + 24 d + 24) (first_hour = 13 + tau, scripts_utils.compute_daily_runoff); one call adds the
 * hours of one routing launch, period hours [h0, h0 + T), read from that launch's x_save: for every (row,
 * day) whose window meets the range it sums the shared hours in ascending order -- from 0 if they hold
 * the window's first hour, else from the partial sum already in daily[r, d] -- and divides by 24 if they
 * hold the window's last hour.  Calls are stream-ordered, one per launch in period order, so a finished
 * day is bit-identical to one sequential pass over its 24 hours whatever the chunking; days no call
 * touches are left alone (the buffer needs no clearing).  gauges == NULL: every reach, reference order,
 * the value ddr_mc_forward's (N, T) runoff holds; else the gauge sums of ddr_gauge_reduce.  daily is
 * (R, n_days) row-major; flags: DDR_FWD_CARRY as the forward was run
 * (DDR_PERIOD_DIRECT_STORE: the all-reach variant that stores per thread, for A/B timing). */
enum { DDR_PERIOD_DIRECT_STORE = 1 << 24 };
ddr_status ddr_period_daily_f32(const ddr_graph* g, const float* x_save, int64_t T, const ddr_gauges* gauges,
                                double discharge_lb, int32_t flags, int64_t h0, int64_t first_hour,
                                int64_t n_days, float* daily, void* stream);
ddr_status ddr_period_daily_f64(const ddr_graph* g, const double* x_save, int64_t T, const ddr_gauges* gauges,
                                double discharge_lb, int32_t flags, int64_t h0, int64_t first_hour,
                                int64_t n_days, double* daily, void* stream);

/* Per-reach temporal statistics of the trapezoid geometry (src/ddr/geometry/statistics.py:20-83):
 * q_daily holds the daily accumulated discharge, element (reach, day) at
 * reach * reach_stride + day * day_stride (1 <= days <= 32768); out is (24, n): for the variables
 * depth, top_width, bottom_width, side_slope, hydraulic_radius, discharge (in this order) the rows
 * min, max, median, mean (NaN skipped as numpy's nan* reductions).  Device pointers, float32. */
ddr_status ddr_geometry_stats_f32(const float* q_daily, int64_t reach_stride, int64_t day_stride, int64_t n,
                                  int64_t days, const float* n_manning, const float* p_spatial,
                                  int64_t p_stride, const float* q_spatial, const float* slope,
                                  double depth_lb, double bottom_width_lb, float* out, void* stream);

/* Per-gauge evaluation metrics of daily series (src/ddr/validation/metrics.py:11-256, the Metrics(pred, target)
 * call of scripts/train.py:106-115 and scripts/test.py:107), one launch, no host sync, no allocation.
 *   pred, target  device fp32, row g (a gauge) at pred + g * pred_stride / target + g * target_stride (strides in
 *           elements, so a caller passes daily[:, warmup:] without a copy), 1 <= n_days <= 8192 values each.  A day
 *           is valid when its target is not NaN.
 *   out     device fp64 (DDR_N_METRICS, n_gauges), metric-major in the DDR_METRIC_* order below.  Sums, means,
 *           roots and quotients are fp64 over the widened inputs, mean-dependent ones two-pass, in a fixed order:
 *           a gauge's row does not depend on the other gauges of the launch.  Empty slices and zero denominators
 *           follow IEEE (NaN, +-inf) like numpy; corr, corr_spearman, r2, nse, kge, kge_12 are NaN below two
 *           valid days.
 *   pred_nan_count  one device word, set to the number of NaN in pred (the reference's validator refuses them; a
 *           gauge whose pred holds NaN gets unspecified values).
 * n_gauges == 0 is a no-op. */
enum {
  DDR_METRIC_BIAS = 0,
  DDR_METRIC_MAE,
  DDR_METRIC_RMSE,
  DDR_METRIC_UB_RMSE,
  DDR_METRIC_FDC_RMSE,
  DDR_METRIC_CORR,
  DDR_METRIC_CORR_SPEARMAN,
  DDR_METRIC_R2,
  DDR_METRIC_NSE,
  DDR_METRIC_FLV,
  DDR_METRIC_FHV,
  DDR_METRIC_PBIAS,
  DDR_METRIC_PBIAS_MID,
  DDR_METRIC_KGE,
  DDR_METRIC_KGE_12,
  DDR_METRIC_RMSE_LOW,
  DDR_METRIC_RMSE_HIGH,
  DDR_METRIC_RMSE_MID,
  DDR_N_METRICS
};
ddr_status ddr_metrics_f32(int64_t n_gauges, int64_t n_days, const float* pred, int64_t pred_stride,
                           const float* target, int64_t target_stride, double* out, int32_t* pred_nan_count,
                           void* stream);

/* NaN-aware summaries of long rows (numpy's nanmin / nanmax / nanmean / nanstd / nanquantile: the attribute
 * statistics of src/ddr/io/statistics.py:45-52, the medians of src/ddr/validation/utils.py:110-112 and of
 * scripts/train.py:127-131), exact, with no host sync, no allocation and no copy: the call can be captured.
 *   x       device fp32 (ddr_summary_f32) or fp64 (ddr_summary_f64), row r at x + r * row_stride (in elements),
 *           0 <= N < 2^31 values each.  NaN never takes part; with DDR_SUMMARY_SKIP_INF neither does +-inf.
 *   q       host array of K <= DDR_SUMMARY_MAX_Q probabilities in [0, 1]; they travel as kernel arguments.
 *   method  DDR_SUMMARY_LINEAR: numpy's default.  With n the row's count and v = (n - 1) q in fp64, lo = floor(v),
 *           g = v - lo, a and b the order statistics lo and min(lo + 1, n - 1): a + (b - a) g, and
 *           b - (b - a) (1 - g) when g >= 0.5, each operation rounded on its own.
 *           DDR_SUMMARY_LOWER: the order statistic floor(v); q = 0.5 is torch.median's element (n - 1) / 2.
 *   out     device fp64 (R, DDR_SUMMARY_N_COLUMNS + K): the DDR_SUMMARY_* columns below, then the K quantiles.
 *           std is the population's (ddof = 0), two-pass: sqrt(sum (x - mean)^2 / count).  A row without a counted
 *           value gets count 0 and NaN in every other column.  The order statistics are selected through
 *           most-significant-digit radix histograms over order-preserving keys (nothing is sorted); the moments are
 *           fp64 sums in a fixed order: a row's record does not depend on R or on the row's position.
 *   work    device scratch of ddr_summary_work_bytes(R, K, sizeof element) bytes, 16-byte aligned.
 * Rows are walked DDR_SUMMARY_TILE elements per workgroup at a time.  R == 0 is a no-op; N == 0 writes the record of
 * an empty row.  ddr_summary_work_bytes returns -1 for arguments the calls would refuse. */
enum { DDR_SUMMARY_COUNT = 0, DDR_SUMMARY_MIN, DDR_SUMMARY_MAX, DDR_SUMMARY_MEAN, DDR_SUMMARY_STD, DDR_SUMMARY_N_COLUMNS };
enum { DDR_SUMMARY_LINEAR = 0, DDR_SUMMARY_LOWER, DDR_N_SUMMARY_METHODS };
#define DDR_SUMMARY_SKIP_INF 1
#define DDR_SUMMARY_MAX_Q 8
#define DDR_SUMMARY_TILE 4096
int64_t ddr_summary_work_bytes(int64_t R, int32_t K, int32_t elem_bytes);
ddr_status ddr_summary_f32(int64_t R, int64_t N, const float* x, int64_t row_stride, int32_t K, const double* q,
                           int32_t method, int32_t flags, double* out, void* work, void* stream);
ddr_status ddr_summary_f64(int64_t R, int64_t N, const double* x, int64_t row_stride, int32_t K, const double* q,
                           int32_t method, int32_t flags, double* out, void* work, void* stream);

/* The summed-Q' baseline of the evaluation (scripts/summed_q_prime.py:208-261, eval_q_prime): per gauge and day
 * the sum of the lateral inflow of the gauge's upstream divides, the unrouted series that routed results are
 * scored against.  With rho = hours_per_step (24: hourly store, 1: daily store) and D = n_steps / rho (trailing
 * steps that do not fill a day are dropped),
 *   daily[i][d] = (sum_{h < rho} qr[i][d * rho + h]) / rho      a plain mean: one NaN hour makes the day NaN
 *   out[g][d]   = sum over the members i of gauge g whose daily[i][d] is not NaN of daily[i][d]      (nansum)
 * An empty list, or a day on which every member is NaN, gives 0; +-inf follows IEEE.  Every sum and the division
 * run in fp64 over the fp32 inputs in an order fixed by the member's position in its list, and the result is
 * rounded once to fp32: a gauge's row does not depend on the other gauges of the plan or on the launch.
 *
 * ddr_summedq_plan_create: the member lists in CSR form, host arrays (copied): gauge g's members are
 *   member_idx[member_off[g] .. member_off[g + 1]), row indices into qr, summed in this order.  member_off starts
 *   at 0 and does not decrease; no index is negative.  A list longer than `chunk` members (1 <= chunk <= 2^30;
 *   4096 is a good default) is cut at multiples of `chunk` from its start into pieces summed by separate waves,
 *   whose fp64 partial rows are added in piece order: the value depends on `chunk` (in the last fp64 bits), not
 *   on anything else.  The device copies are made on the current device through `stream`, which is synchronised
 *   before the call returns.  Without a HIP device the plan is still made and ddr_summedq_f32 still checks its
 *   arguments, then fails with DDR_ERR_HIP.
 * ddr_summedq_scratch_bytes: the bytes of fp64 partial rows ddr_summedq_f32 needs for n_days days (0 when no list
 *   is cut); -1 for a null plan or a negative n_days.
 * ddr_summedq_f32: one or two launches on `stream`, no allocation, no host sync (capturable).
 *   qr      device fp32, row i at qr + i * row_stride (elements; row_stride >= n_steps, so a time slice of a
 *           wider store is passed without a copy), n_rows > the plan's largest index.  16-byte loads are used
 *           when qr is 16-byte aligned and row_stride a multiple of 4, 4-byte loads otherwise: same values.
 *   out     device fp32 (n_gauges, D), row g at out + g * out_stride (out_stride >= D)
 *   scratch device memory of at least ddr_summedq_scratch_bytes(plan, D) bytes (may be NULL when that is 0)
 * Refused with DDR_ERR_ARG before any launch: negative sizes, hours_per_step outside {1, 24}, n_steps <
 * hours_per_step, short strides, n_rows not above the largest index, short scratch, null pointers where data is
 * required.  A plan of 0 gauges is a no-op. */
typedef void* ddr_summedq_plan;
ddr_status ddr_summedq_plan_create(int64_t n_gauges, const int64_t* member_off, const int32_t* member_idx,
                                   int64_t chunk, void* stream, ddr_summedq_plan* plan);
ddr_status ddr_summedq_plan_destroy(ddr_summedq_plan plan);
int64_t ddr_summedq_scratch_bytes(ddr_summedq_plan plan, int64_t n_days);
ddr_status ddr_summedq_f32(ddr_summedq_plan plan, const float* qr, int64_t n_rows, int64_t row_stride, int64_t n_steps,
                           int32_t hours_per_step, float* out, int64_t out_stride, void* scratch,
                           int64_t scratch_bytes, void* stream);

/* The per-batch forcing feed: the batch's lateral inflow and observations gathered on the device from stores that
 * were uploaded once, in place of the reference's per-batch host readers (src/ddr/io/readers.py:461-531
 * StreamflowReader.forward; io/builders.py:112-129 with scripts/train.py:84-92 for the observations).
 * Both stores are device fp32 with time on the inner axis, row i at store + i * row_stride (elements; row_stride >=
 * n_store_cols, so a time slice or a view of a wider buffer is passed without a copy); `rows` is device int32, the
 * store row of every output reach / gauge, where any value outside [0, n_rows) means "the store lacks it" and is
 * never used as an address.  Values are copied as bits (NaN payloads, -0.0).  One launch each on `stream`, no
 * allocation, no host sync (capturable), no atomics.
 *
 * ddr_feed_qprime_f32: out (n_out, n_reaches) with reaches on the inner axis, the layout ddr_mc_forward reads:
 *     out[t][i] = store[rows[i]][t0 + t / repeat]        rows[i] in the store          valid[i] = 1
 *     out[t][i] = fill                                   otherwise (readers.py:523-530) valid[i] = 0
 *   repeat = 1 copies n_cols = n_out columns (an hourly store, or a daily store for qprime_hours = 24); repeat = 24
 *   expands a daily store to hours (readers.py:513-519); n_cols = ceil(n_out / repeat), the last column repeated
 *   only up to n_out.  16-byte loads are used when `store` is 16-byte aligned and row_stride a multiple of 4
 *   (whatever t0), 4-byte loads otherwise: same values.  valid is device uint8 (n_reaches).
 * ddr_feed_rows_f32: out (n_out_rows, n_cols - 2 * trim), row g at out + g * out_stride:
 *     out[g][j]  = store[rows[g]][t0 + trim + j]           (NaN throughout for a gauge the store lacks)
 *     has_nan[g] = 1 when any of the n_cols columns of the window is NaN, the trimmed ones included, or the gauge is
 *                  unknown (train.py:84-87); device uint8 (n_out_rows).  trim = 1 is the training loop's [:, 1:-1].
 * Refused with DDR_ERR_ARG before any launch: negative sizes, row_stride < n_store_cols, a window outside
 * [0, n_store_cols], repeat < 1, n_cols != ceil(n_out / repeat), n_cols < 2 * trim, a short out_stride, null
 * pointers where data is required.  Zero reaches / rows is a no-op. */
ddr_status ddr_feed_qprime_f32(const float* store, int64_t row_stride, int64_t n_rows, int64_t n_store_cols,
                               const int32_t* rows, int64_t n_reaches, int64_t t0, int64_t n_cols, int32_t repeat,
                               int64_t n_out, float fill, float* out, uint8_t* valid, void* stream);
ddr_status ddr_feed_rows_f32(const float* store, int64_t row_stride, int64_t n_rows, int64_t n_store_cols,
                             const int32_t* rows, int64_t n_out_rows, int64_t t0, int64_t n_cols, int32_t trim,
                             float* out, int64_t out_stride, uint8_t* has_nan, void* stream);

/* The per-batch attribute feed: the catchment attributes, flowpath tensors and flow_scale of a batch, gathered on the
 * device by the batch's CONUS indices (`active`, device int32, e.g. the active list of ddr_upstream_collate) in place
 * of the reference's per-batch host code (src/ddr/geodatazoo/merit.py:92-124 _get_attributes, 273-319
 * _build_common_tensors; lynker_hydrofabric.py:105-135, 302-354; io/readers.py:299-362 build_flow_scale_tensor).
 * `table` is the attribute store aligned to CONUS order once, device fp32 (n_conus, n_attrs) reach-major, row i at
 * table + i * row_stride (elements, row_stride >= n_attrs), NaN for a missing value and for every attribute of a reach
 * the store lacks.  An active[i] outside [0, n_conus) is a missing reach, never an address.  Values are copied as
 * bits.  Work is queued on `stream`: no allocation, no host sync (capturable).
 *
 * ddr_feed_attributes_f32, one launch:
 *     v              = table[active[i]][a]; a NaN becomes fill[a]
 *     spatial[a][i]  = v                                     (n_attrs, n_reaches)
 *     normalized[i][a] = (v - means[a]) / stds[a]            (n_reaches, n_attrs); one fp32 subtraction and one IEEE
 *                      division; a NaN result carries the bits the reference's host code gives it (the NaN of
 *                      means[a], else of v, else of stds[a], quieted; 0xffc00000 for inf - inf and 0 / 0)
 *   fill, means, stds are device fp32 (n_attrs).  fill[a] is means[a] (fill_nans, merit.py:124) except where means[a]
 *   is NaN: there it is the NaN-mean of the attribute over this batch (merit.py:295-298), which ddr_feed_attr_mean_f32
 *   writes into it before this call.
 *   path (host struct, may be null): the flowpath arrays in the order length, slope, x, top_width, side_slope.
 *     out[k][i] = src[k][active[i]], and fill[k] for a NaN or an out-of-range index (no clamping); src[k] null with
 *     out[k] set writes the constant fill[k] (MERIT's x = 0.3); out[k] null skips the array.  src / out are device
 *     fp32 of n_conus / n_reaches elements.
 *   flow_scale (device fp32 (n_reaches), may be null) is set to 1.0.
 * ddr_feed_attr_mean_f32: for each of the n_flagged attributes flagged[j] (device int32), fill[flagged[j]] = the mean
 *   of the batch's non-NaN values of that attribute, accumulated in fp64 in a fixed order (no atomics) and rounded to
 *   fp32 once; 0xffc00000 when the batch holds none.  `work`: device scratch of ddr_feed_attr_mean_work_bytes(n_flagged)
 *   bytes, 8-byte aligned.  Two launches; n_flagged = 0 launches nothing.
 * ddr_feed_flow_scale_f32: the reference's loop over the batch's gauges on a flow_scale that holds ones:
 *     for g in batch order: flow_scale[gage_c[g]] = factors[scale_rows[g]]
 *   skipping a gauge whose scale_rows[g] lies outside [0, n_factors) (an unknown gauge), whose skip[scale_rows[g]] is
 *   set (skip: device uint8 (n_factors), may be null) or whose gage_c[g] lies outside [0, n_reaches).  Of several
 *   gauges on one segment the last one in batch order that is not skipped wins, whatever the scheduling.  `winner` is
 *   device int32 scratch (n_reaches), uninitialised.  One launch of one workgroup; n_gauges = 0 launches nothing.
 * Refused with DDR_ERR_ARG before any launch: negative sizes, n_attrs outside [1, DDR_ATTR_MAX_FEATURES], row_stride <
 * n_attrs, n_conus or n_gauges beyond int32, n_flagged outside [0, n_attrs], a short or misaligned work buffer, a
 * flowpath source without an output, null pointers where data is required.  Zero reaches is a no-op. */
#define DDR_ATTR_MAX_FEATURES 64
#define DDR_FLOWPATH_ARRAYS 5
typedef struct ddr_flowpath {
  const float* src[DDR_FLOWPATH_ARRAYS];
  float* out[DDR_FLOWPATH_ARRAYS];
  float fill[DDR_FLOWPATH_ARRAYS];
} ddr_flowpath;
ddr_status ddr_feed_attributes_f32(const float* table, int64_t row_stride, int64_t n_conus, int32_t n_attrs,
                                   const int32_t* active, int64_t n_reaches, const float* fill, const float* means,
                                   const float* stds, float* spatial, float* normalized, const ddr_flowpath* path,
                                   float* flow_scale, void* stream);
int64_t ddr_feed_attr_mean_work_bytes(int32_t n_flagged);
ddr_status ddr_feed_attr_mean_f32(const float* table, int64_t row_stride, int64_t n_conus, int32_t n_attrs,
                                  const int32_t* active, int64_t n_reaches, const int32_t* flagged, int32_t n_flagged,
                                  float* fill, void* work, int64_t work_bytes, void* stream);
ddr_status ddr_feed_flow_scale_f32(const int32_t* gage_c, const int32_t* scale_rows, int64_t n_gauges,
                                   const float* factors, const uint8_t* skip, int64_t n_factors, int64_t n_reaches,
                                   int32_t* winner, float* flow_scale, void* stream);

/* The upstream index: everything upstream of a set of reaches, from the network's COO alone.  It replaces the
 * per-gauge rx.ancestors of the reference (engine/src/ddr_engine/merit/build.py:206-290 build_gauge_adjacencies,
 * graph.py:89-115 subset_upstream; src/ddr/geodatazoo/merit.py:321-396 _build_routing_data_target_catchments; the
 * membership step of scripts/summed_q_prime.py).  The network is the conus_adjacency contract: strictly lower
 * triangular COO (row = downstream reach), dendritic.
 *
 * ddr_upstream_index_create: builds down[n] (-1: outlet), the outlet count and max_depth, the longest
 *   reach-to-outlet path in edges.  rows/cols are host arrays, or with DDR_UPSTREAM_DEVICE_COO device arrays on the
 *   current device (down[] and the depths are then computed on the device).  DDR_UPSTREAM_HOST_ONLY builds an index
 *   that needs no device and serves the _host queries alone; any other index lives on the current device and serves
 *   both.  `stream` is synchronised before the call returns.  n >= 1; e == 0 is valid (every reach isolated).
 *   Refused: rows[k] <= cols[k] (DDR_ERR_NOT_LOWER), a reach with two different downstream reaches
 *   (DDR_ERR_NOT_DENDRITIC), an index out of range (DDR_ERR_ARG).  The same edge given twice is accepted.
 * ddr_upstream_index_info: rounds = 0 without edges, else ceil(log2(max_depth)) + 1, the doubling rounds of every
 *   device query (fixed by the index, so no query reads the device to know when to stop); device = -1: host-only.
 * ddr_upstream_index_down: down[n] copied to a host array.
 *
 * Queries.  `targets` / `gage_idx` are always HOST arrays of reach indices in [0, n) (checked before anything is
 * launched, then uploaded); several may name one reach: slot_of[g] is the smallest slot on g's reach, the others are
 * its aliases.  Every other array of a device query is device memory, of a _host query host memory.  Device queries
 * take `scratch` of at least ddr_upstream_scratch_bytes(index, n_targets, n_members) bytes (n_members = 0 except for
 * ddr_upstream_members) and allocate nothing themselves, apart from the pooled blocks of the union inside
 * ddr_upstream_collate.
 *
 * ddr_upstream_label: label_out[i] (int32[n]) = the slot of the nearest target at or downstream of reach i, -1
 *   without one; label >= 0 is the closure mask.  slot_of (host int32[n_targets], may be NULL).  Pointer doubling,
 *   one launch per round; the target upload is waited for, nothing is read back.
 * ddr_upstream_collate: the union subnetwork of the gauges' closures; the outputs are those of
 *   ddr_collate_gauges_device (bit-identical to collating the gauges' complete upstream subsets) with explicit
 *   capacities: active[active_cap], rows_c/cols_c/col[edge_cap] (n always suffices), out_idx[out_idx_cap].  A gauge
 *   whose reach has nothing upstream appears as itself.  Synchronous.
 * ddr_upstream_member_counts / ddr_upstream_members: off (int64[n_gauges + 1]) and idx (int32[n_members], n_members
 *   = *total = off[n_gauges]): gauge g's reach and everything upstream of it, ascending, at idx[off[g] .. off[g+1]).
 *   Nested gauges repeat their shared reaches; aliases get equal lists.  A total of 2^31 or more is refused.
 *   Synchronous.  The _host twin of ddr_upstream_members takes the off of ddr_upstream_member_counts_host.
 *
 * Refused with DDR_ERR_ARG and a message naming the fault, before any launch: null pointers, negative counts, a
 * target outside [0, n), scratch too small, a host-only index given to a device query. */
typedef void* ddr_upstream_index;
enum { DDR_UPSTREAM_HOST_ONLY = 1, DDR_UPSTREAM_DEVICE_COO = 2 };
typedef struct {
  int64_t n, n_outlets, max_depth, rounds, device;
} ddr_upstream_info;
ddr_status ddr_upstream_index_create(int64_t n, int64_t e, const int32_t* rows, const int32_t* cols, int32_t flags,
                                     void* stream, ddr_upstream_index* index);
ddr_status ddr_upstream_index_destroy(ddr_upstream_index index);
ddr_status ddr_upstream_index_info(ddr_upstream_index index, ddr_upstream_info* info);
ddr_status ddr_upstream_index_down(ddr_upstream_index index, int32_t* down);
int64_t ddr_upstream_scratch_bytes(ddr_upstream_index index, int64_t n_targets, int64_t n_members);
ddr_status ddr_upstream_label(ddr_upstream_index index, int64_t n_targets, const int32_t* targets, int32_t* label_out,
                              int32_t* slot_of, void* scratch, int64_t scratch_bytes, void* stream);
ddr_status ddr_upstream_collate(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx, int32_t* active,
                                int64_t active_cap, int64_t* n_active, int32_t* rows_c, int32_t* cols_c,
                                int64_t edge_cap, int64_t* nnz, int64_t* crow, int32_t* col, int64_t* out_off,
                                int32_t* out_idx, int64_t out_idx_cap, int32_t* gage_c, void* scratch,
                                int64_t scratch_bytes, void* stream);
ddr_status ddr_upstream_member_counts(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx, int64_t* off,
                                      int64_t* total, void* scratch, int64_t scratch_bytes, void* stream);
ddr_status ddr_upstream_members(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx, int64_t n_members,
                                int32_t* idx, void* scratch, int64_t scratch_bytes, void* stream);
ddr_status ddr_upstream_label_host(ddr_upstream_index index, int64_t n_targets, const int32_t* targets,
                                   int32_t* label_out, int32_t* slot_of);
ddr_status ddr_upstream_collate_host(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx,
                                     int32_t* active, int64_t active_cap, int64_t* n_active, int64_t* crow,
                                     int32_t* col, int64_t edge_cap, int64_t* nnz, int64_t* out_off, int32_t* out_idx,
                                     int64_t out_idx_cap, int32_t* gage_c);
ddr_status ddr_upstream_member_counts_host(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx,
                                           int64_t* off);
ddr_status ddr_upstream_members_host(ddr_upstream_index index, int64_t n_gauges, const int32_t* gage_idx,
                                     const int64_t* off, int32_t* idx);

/* The network build: a raw flowpath table in any row order to the contract every other entry point starts from
 * (strictly lower-triangular COO, upstream reaches numbered first, dendritic).  It replaces the engine's
 * create_matrix (engine/src/ddr_engine/merit/build.py:20-107, lynker_hydrofabric/io.py:60-154: rustworkx topological
 * sort, cycle removal, renumbering).  ids[n] are distinct int64 over the full range, to_ids[n] the id of each row's
 * downstream flowpath.  One deterministic answer, identical bits from the device build and its host twin:
 *   1. down[i] = the row of to_ids[i] in ids, -1 when no row has that id: an outlet (0, negative, any foreign id).
 *   2. A reach is on a cycle if following down returns to it (a self-loop counts).  On-cycle reaches are dropped, a
 *      kept reach that drained into one becomes an outlet, reaches upstream of a cycle are kept.
 *   3. dist = edges to the outlet, basin = the rank of the outlet's row among all outlets' rows.  The new index sorts
 *      the kept reaches by (basin ascending, dist descending, row ascending): basins are contiguous, row > col.
 *
 * ddr_network_build: on the current device and `stream`; ids / to_ids are host arrays, or with
 *   DDR_NETWORK_DEVICE_INPUT device arrays.  Synchronous (the counts come back).  ddr_network_build_host: the same
 *   without a device.  n == 0 gives an empty network.
 * ddr_network_info: kept = n - n_dropped reaches, nnz edges, n_basins outlets, max_depth the longest reach-to-outlet
 *   path in edges; device = -1 for a host build.
 * ddr_network_get: copies out position (int32[kept]: the row of new reach k), order (int64[kept]: its id), down
 *   (int32[kept]: new index of its downstream reach, -1), rows / cols (int32[nnz], the COO in ascending cols),
 *   dropped (int32[n_dropped], rows ascending).  NULL skips an array.  Host pointers; a device build also takes
 *   device pointers, and copies on `stream` before it returns.
 * ddr_network_lookup_i64 / _host: pos[k] (int32[m]) = the row of queries[k] in ids, -1 when absent; with
 *   DDR_NETWORK_DEVICE_INPUT every array of the device form is device memory.  Synchronous.
 *
 * Refused with DDR_ERR_ARG and a message naming the fault: null pointers, negative counts, an unknown flag, n >= 2^30
 * (all before any launch), and an id that appears more than once in ids (the message names the smallest one). */
typedef void* ddr_network;
enum { DDR_NETWORK_DEVICE_INPUT = 1 };
typedef struct {
  int64_t n, kept, nnz, n_dropped, n_basins, max_depth, device;
} ddr_network_counts;
ddr_status ddr_network_build(int64_t n, const int64_t* ids, const int64_t* to_ids, int32_t flags, void* stream,
                             ddr_network* network);
ddr_status ddr_network_build_host(int64_t n, const int64_t* ids, const int64_t* to_ids, ddr_network* network);
ddr_status ddr_network_info(ddr_network network, ddr_network_counts* info);
ddr_status ddr_network_get(ddr_network network, int32_t* position, int64_t* order, int32_t* down, int32_t* rows,
                           int32_t* cols, int32_t* dropped, void* stream);
ddr_status ddr_network_destroy(ddr_network network);
ddr_status ddr_network_lookup_i64(int64_t n, const int64_t* ids, int64_t m, const int64_t* queries, int32_t* pos,
                                  int32_t flags, void* stream);
ddr_status ddr_network_lookup_i64_host(int64_t n, const int64_t* ids, int64_t m, const int64_t* queries, int32_t* pos);

/* The geometry predictor around the KAN (src/ddr/geometry/predictor.py, adapters.py): two launches that with
 * ddr_kan_forward_f32 between them take raw catchment attributes to channel geometry.  Device pointers, fp32
 * unless stated, no host sync, no allocation; n_rows == 0 is a no-op.
 *
 * ddr_attr_prepare_f32: raw attributes -> the KAN's input x (n_rows, n_features) row-major.
 *   raw     n_features columns of n_rows floats, feature f at raw + f * feat_stride (elements)
 *   scale, offset (fp64), log10_flag (int32)  per feature: the source's unit conversion.  A feature with
 *           scale != 1, offset != 0 or the flag set is converted in fp64, w = (double)v * scale + offset,
 *           flagged: w = log10(max(w, 1e-6)) (NaN kept), and rounded to fp32 (adapters.py:159-162); any other
 *           feature passes unchanged
 *   p10, p90  both NULL or both given: counts[1][f] += (v < p10[f]), counts[2][f] += (v > p90[f]) on the
 *           converted value; a NaN is neither (predictor.py:320-350)
 *   mean, std  a NaN v becomes mean[f] and counts[0][f] += 1 (predictor.py:254-262; +-inf is left alone), then
 *           x[i][f] = (v - mean[f]) / std[f]: an fp32 subtraction and an IEEE division (predictor.py:270), so a
 *           zero std gives +-inf or NaN as the reference's does (std is device memory: not checked here)
 *   counts  NULL, or int64 (3, n_features) = filled, below, above, which the CALLER zeroes: integer atomics, one
 *           per counter and workgroup, so the totals are exact and independent of the order
 *   1 <= n_features <= 32 (the KAN's envelope).
 * Replaces: adapt_attributes' conversion, _check_distribution, _prepare_attributes (np.isnan / fill / stack /
 * subtract / divide / transpose: ~5 passes over (F, N) on the host and 3 launches).
 *
 * ddr_geometry_predict_f32: the KAN's output u (n_rows, n_outputs) in [0, 1] -> parameters and geometry.
 *   slot_n, slot_q, slot_p  where n, q_spatial and p_spatial come from: column of u (or -1: `value`,
 *           p_spatial only -- the reference has no default for the others, predictor.py:307-316), the bounds
 *           lo / hi and the log-space flag of denormalize (routing/utils.py:166-185): u (hi - lo) + lo, or
 *           exp(u (log(hi) - log(lo + 1e-6)) + log(lo + 1e-6)); every scalar is rounded to fp32 on the host
 *           before it is used, as torch's fp32 scalar tensors are
 *   discharge, slope  (n_rows) each, clamped from below by discharge_lb / slope_lb with torch.clamp's NaN
 *           rule (NaN stays NaN, predictor.py:211-214): a reach with a NaN slope or discharge gets its n / p / q
 *           and NaN in the eight geometry rows
 *   out     DDR_N_GEOM rows of out_stride >= n_rows floats in the DDR_GEOM_* order below (the reference's
 *           order, predictor.py:216-238): compute_trapezoidal_geometry (trapezoidal.py:62-97) in its operation
 *           order with IEEE division and square root, correctly rounded pow and the fixed side-slope clamp
 *           [0.5, 50]
 *   discharge == NULL and slope == NULL: parameters only -- out is three rows n, p_spatial, q_spatial
 *           (_predict_parameters, predictor.py:276-318), the same bits as rows DDR_GEOM_N.. of a full call.
 * Replaces: three denormalize calls, two clamps and the ~25 element-wise launches of
 * compute_trapezoidal_geometry, each over (n_rows,) temporaries. */
enum {
  DDR_GEOM_DEPTH = 0,
  DDR_GEOM_TOP_WIDTH,
  DDR_GEOM_BOTTOM_WIDTH,
  DDR_GEOM_SIDE_SLOPE,
  DDR_GEOM_CROSS_SECTIONAL_AREA,
  DDR_GEOM_WETTED_PERIMETER,
  DDR_GEOM_HYDRAULIC_RADIUS,
  DDR_GEOM_VELOCITY,
  DDR_GEOM_N,
  DDR_GEOM_P_SPATIAL,
  DDR_GEOM_Q_SPATIAL,
  DDR_N_GEOM
};
typedef struct ddr_geom_slot {
  int32_t column;    /* column of u, or -1: `value` */
  int32_t log_space; /* denormalize's log_space */
  double lo, hi;     /* the parameter's range */
  double value;      /* the default of a slot without a column */
} ddr_geom_slot;
ddr_status ddr_attr_prepare_f32(int64_t n_rows, int32_t n_features, const float* raw, int64_t feat_stride,
                                const double* scale, const double* offset, const int32_t* log10_flag,
                                const float* mean, const float* std, const float* p10, const float* p90, float* x,
                                int64_t* counts, void* stream);
ddr_status ddr_geometry_predict_f32(int64_t n_rows, int32_t n_outputs, const float* u, const ddr_geom_slot* slot_n,
                                    const ddr_geom_slot* slot_q, const ddr_geom_slot* slot_p, const float* discharge,
                                    const float* slope, double discharge_lb, double slope_lb, double depth_lb,
                                    double bottom_width_lb, float* out, int64_t out_stride, void* stream);

/* ---- The BMI coupling's device side (the reference's src/ddr/bmi/ddr_bmi.py; bmi.hip) ------------------------
 * Stateless: the caller (ddr_amd.bmi.DdrBmi) owns every array.  All pointers are device pointers unless named
 * *_host; every call is queued on `stream` and returns without a host sync except ddr_bmi_nexus_table.
 * Arguments are checked before anything is launched (DDR_ERR_ARG and a message).
 *
 * ddr_bmi_nexus_table  the nexus -> segment dictionary as two device arrays: checks on the host that keys_host
 *           is strictly ascending and every seg_host is in [0, n_segments), then copies both to keys / key_seg
 *           (n_keys elements each) and waits for the copies.
 * ddr_bmi_nexus_plan   set_value("land_surface_water_source__id") (ddr_bmi.py:432-433 and the loop of 424-427):
 *           src_of_seg (n_segments) is set to -1, then src_of_seg[key_seg[j]] = the LAST i with ids[i] == keys[j]
 *           (the reference's sequential loop: a repeated id, or two ids of one segment, leave the last value);
 *           ids absent from the table are skipped.
 * ddr_bmi_set_inflow_f64  lateral[s] = flows[src[s]] where 0 <= src[s] < n_flows; the other segments keep their
 *           value (ddr_bmi.py:427; with a host-built src also set_value_at_indices, 443-445).
 * ddr_bmi_window_f32   update_until's inflows (ddr_bmi.py:270-281, 313-318) for the n_rows sub-steps the call
 *           executes out of the n_steps it planned: window row k (k < n_rows, rows of row_stride floats) =
 *           (float)((1.0 - a) * prev + a * cur), a = (double)(k + 1) / n_steps, in separately rounded fp64
 *           (linear != 0), or (float)cur; row n_rows repeats row n_rows - 1 (the routing kernel's step t reads
 *           row t - 1, so a window of n_rows + 1 rows is n_rows steps).  Then prev = cur and cur = 0.  Nothing is
 *           clamped: the routing kernel clamps its steps and its hot start reads row 0 raw (ddr_bmi.py:284-297).
 * ddr_bmi_outputs_f32  _update_output_cache (ddr_bmi.py:587-630) in its fp32 operation order with IEEE division
 *           and square root and the correctly rounded pow: out row 0 = discharge, row 1 = velocity clamped to
 *           [0, 15], row 2 = depth clamped from below by depth_lb (rows of out_stride floats).  top_width /
 *           side_slope are the routing engine's; p_spatial is one value (p_stride = 0) or per segment (1).
 * Replaces, per coupling interval: a Python loop over every nexus id, n_rows host interpolations and uploads,
 * ~25 element-wise launches and three device-to-host copies. */
ddr_status ddr_bmi_nexus_table(int64_t n_keys, const int64_t* keys_host, const int32_t* seg_host, int64_t n_segments,
                               int64_t* keys, int32_t* key_seg, void* stream);
ddr_status ddr_bmi_nexus_plan(int64_t n_ids, const int32_t* ids, int64_t n_keys, const int64_t* keys,
                              const int32_t* key_seg, int64_t n_segments, int32_t* src_of_seg, void* stream);
ddr_status ddr_bmi_set_inflow_f64(int64_t n_segments, const int32_t* src, int64_t n_flows, const double* flows,
                                  double* lateral, void* stream);
ddr_status ddr_bmi_window_f32(int64_t n_segments, int32_t n_rows, int32_t n_steps, int32_t linear, double* prev,
                              double* cur, float* window, int64_t row_stride, void* stream);
ddr_status ddr_bmi_outputs_f32(int64_t n_segments, const float* discharge, const float* n_manning,
                               const float* q_spatial, const float* p_spatial, int64_t p_stride, const float* slope,
                               const float* top_width, const float* side_slope, double depth_lb,
                               double bottom_width_lb, float* out, int64_t out_stride, void* stream);

/* Synchronise `stream` and read the device status block written by the last launches:
 * returns DDR_OK or DDR_ERR_TIMEOUT. */
ddr_status ddr_graph_status(const void* status, void* stream);
/* Hand-off failures without a host sync: every routing launch queues an async copy of its status
 * words; every entry point returns DDR_ERR_TIMEOUT once a queued copy reports a timed-out hand-off
 * (whose outputs hold NaN).  wait = 1 blocks until every queued copy has landed.  No reference
 * counterpart (the reference solver raises ValueError on failure, routing/utils.py:598-600). */
ddr_status ddr_status_check(int32_t wait);
/* ---- One basin split across GPUs (no reference counterpart: the reference routes a basin on one
 * device; north star item (5)) ----------------------------------------------------
 * Every rank of a split builds the SAME graph of the basin (same COO and options: the builders are
 * deterministic), then ddr_graph_set_split tells it which logical blocks it runs (block_rank[b] ==
 * rank; the others are skipped).  A cut edge between blocks of two ranks carries its fp64 granules
 * through the receive memory of the rank that reads them: the consumer's in the forward, the
 * producer's in the backward, written with system-scope stores over xGMI.  Each rank allocates its
 * receive memory with ddr_xmem_alloc (uncached device memory, exported as an IPC handle of
 * DDR_XMEM_HANDLE_BYTES bytes), the ranks exchange handles (torch.distributed) and open the peers'
 * with ddr_xmem_open.  Before each routing launch the ranks reset their receive rows and hand-shake
 * on the device (an epoch word per peer), so no host synchronisation is needed; all ranks of a split
 * must call forward / backward the same number of times with the same T.  Gauge mode and state
 * gradients are not supported on a split graph. */
enum { DDR_XMEM_HANDLE_BYTES = 64 };
/* bytes of one rank's receive memory for n_x cross-rank cut edges and windows of up to T steps */
ddr_status ddr_xmem_bytes(int64_t n_x, int64_t T, int64_t* bytes);
/* kind: 0 uncached, 1 fine-grained, 2 plain device memory (the first kind that exports) */
ddr_status ddr_xmem_alloc(int64_t bytes, void** ptr, void* handle, int32_t* kind);
ddr_status ddr_xmem_open(const void* handle, void** ptr);
ddr_status ddr_xmem_close(void* ptr, int32_t opened);
/* reaches of every logical block (n_blocks entries, ticket order) */
ddr_status ddr_graph_blocks(const ddr_graph* g, int32_t* nloc, int64_t cap);
/* producer (upstream) and consumer (downstream) logical block of every cut edge (n_cut entries) */
ddr_status ddr_graph_cut_blocks(const ddr_graph* g, int32_t* prod, int32_t* cons, int64_t cap);
/* block_rank: n_blocks entries in [0, nranks); peers: every rank's receive memory (peers[rank] ==
 * local), each ddr_xmem_bytes(n_x, t_cap) bytes, n_x = the cut edges whose blocks differ in rank
 * (returned in *n_x) */
ddr_status ddr_graph_set_split(ddr_graph* g, int32_t rank, int32_t nranks, const int32_t* block_rank, void* local,
                               void* const* peers, int64_t t_cap, int64_t* n_x);
/* detach the split (before its receive memory is released): later launches run every block again.
 * One stream per split graph: its launch epochs are counted per graph. */
ddr_status ddr_graph_clear_split(ddr_graph* g);

/* Debug knobs.  DDR_DEBUG_FORCE_TIMEOUT: every inter-workgroup wait of the following launches
 * times out (tests the failure path).  DDR_DEBUG_NO_STEADY: the routing kernels run every tick
 * through their general path instead of the specialised steady-tick path (bitwise A/B; also set by
 * the environment variable DDR_NO_STEADY=1).  DDR_DEBUG_NO_STORER: light forward blocks store the
 * routing state and runoff from their compute waves instead of their idle waves (DDR_NO_STORER=1).
 * DDR_DEBUG_NO_PLAIN: launches without the rare options (split basin, profile, state seeds, daily
 * accumulation) run the general kernel instances instead of the plain ones compiled without those options
 * (bitwise A/B; DDR_NO_PLAIN=1). */
enum { DDR_DEBUG_FORCE_TIMEOUT = 1, DDR_DEBUG_NO_STEADY = 2, DDR_DEBUG_NO_STORER = 4, DDR_DEBUG_NO_PLAIN = 8 };
ddr_status ddr_set_debug_flags(int32_t flags);

/* General sparse triangular solve A x = b (lower) or A^T x = b (transpose = 1), CSR A with a
 * non-unit diagonal, fp32 values accumulated in fp64 (SciPy semantics, utils.py:587-600).
 * crow/col are HOST int64 arrays (the pattern); values, b, x are device float arrays.
 * Synchronous w.r.t. the pattern upload only. */
ddr_status ddr_tri_solve(int64_t n, int64_t nnz, const int64_t* crow_host, const int64_t* col_host,
                         const float* values, const float* b, float* x, int32_t lower,
                         int32_t transpose, void* stream);
/* ddr_tri_solve with SciPy's / CuPy's unit_diagonal (routing/utils.py:596, 611 forward; 239, 307
 * backward): unit_diagonal != 0 takes every diagonal entry as 1 without reading it (a missing one
 * included) and skips the diag^-1 scaling and the singular check (no host round trip). */
ddr_status ddr_tri_solve_ex(int64_t n, int64_t nnz, const int64_t* crow_host, const int64_t* col_host,
                            const float* values, const float* b, float* x, int32_t lower,
                            int32_t transpose, int32_t unit_diagonal, void* stream);
/* gradA[k] = -gradb[row(k)] * x[col(k)] for CSR (device int64 crow/col). */
ddr_status ddr_tri_grad_values(int64_t n, int64_t nnz, const int64_t* crow, const int64_t* col,
                               const float* gradb, const float* x, float* grad_values, void* stream);

/* Kernel timing (measurement hook, no reference counterpart).  While enabled, every routing
 * launch brackets its main kernel (route_forward_kernel / route_backward_kernel) with HIP events
 * on the launch stream.  ddr_kernel_ms(0 = forward, 1 = backward) synchronises on the last such
 * pair and returns its duration in milliseconds. */
ddr_status ddr_set_kernel_timing(int32_t enable);
ddr_status ddr_kernel_ms(int32_t which, float* ms);

/* Per-workgroup launch profile (debug).  When `buf` is non-null, the next routing launches write
 * 16 uint64 per workgroup: start and end (s_memrealtime, 100 MHz), time spent waiting on
 * inter-workgroup imports, the hardware id (HW_ID | XCC_ID << 32), then the time at every 1024th
 * tick.  `buf` is a zeroed device array of at least 16 * n_blocks uint64; which = 0 (forward) or
 * 1 (backward). */
ddr_status ddr_set_block_profile(int32_t which, uint64_t* buf);

/* Device capacity helpers. */
ddr_status ddr_device_info(int32_t* n_cu, int32_t* max_resident_blocks);
const char* ddr_last_error(void);
const char* ddr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DDR_MC_H */
