// ============================================================================================
// Lateral inflow into the schedule layout of x_save (per workgroup, tick-major: row tau = t + off(r)
// holds its nloc reaches contiguously).  Each thread issues all its loads before the first is
// consumed (memory-level parallelism).  And the adjoint: dL/dq' from the state-gradient backward.
// ============================================================================================
#include "internal.h"
#include "route_args.h"

namespace ddr {

// q'[max(t-1, 0), ref] * flow_scale[ref] -> qs[tick(t, r)] (mmc.py:303-304, 421-424): the routing
// kernels then read one contiguous row per tick instead of scattered 4-byte values of q' rows.
// One workgroup per (block, tile of gather_steps steps): reads walk the block's reaches in
// ascending reference order (runs of adjacent q' columns), writes walk positions (sorted by tick
// offset, so runs of one offset are contiguous in a tick row); the tile is staged in LDS.
// DDR_FWD_CHECK_QPRIME: the reference asserts that the flow-scaled q' holds no NaN before routing
// (mmc.py:335, `assert ~torch.any(torch.isnan(self.q_prime))`); the gathers see every value the window
// reads, so they set status word kStatusNaN instead of a separate pass over q' (28 GB at C5)
__device__ __forceinline__ void flag_nan(const RouteArgs& a, bool nan) {
  if (!(a.flags & DDR_FWD_CHECK_QPRIME)) return;
  if (__builtin_amdgcn_ballot_w64(nan) != 0 && (threadIdx.x & 63) == 0) atomicOr(a.status + kStatusNaN, 1u);
}
// ... and the one row no routing step reads: q' of the window's last hour (its row (T - 1) / qp_hours)
template <typename R>
__global__ void nan_last_row_kernel(RouteArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool nan = false;
  if (i < a.N) {
    const int64_t row = (a.T - 1) / (a.qp_hours > 0 ? a.qp_hours : 1);
    R v = static_cast<const R*>(a.qprime)[row * a.N + i];
    if (a.qp_valid && !a.qp_valid[i]) v = R(0.001f);
    if (a.fs) v = v * static_cast<const R*>(a.fs)[i];
    nan = v != v;
  }
  flag_nan(a, nan);
}

// One workgroup per (block, chunk of `chunk` steps, a multiple of G), G steps per LDS tile: each thread keeps
// its reaches' reference indices, LDS destinations, tick offsets and scale in registers for the whole chunk
// (a workgroup per tile re-read them: 12 B per reach per tile, a third of the q' bytes at G = 8), and the
// next tile's q' loads are in flight while the current tile leaves LDS for the schedule rows.  A chunk's
// tiles run on one CU back to back, so a tick row's segments written by consecutive tiles meet in its L2.
template <typename R, int G, int BS, int KG>
__global__ void __launch_bounds__(BS) gather_qprime_kernel(RouteArgs a, int chunk, int nchunks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
  R* tile = reinterpret_cast<R*>(gsm);  // [G][nloc]
  // one-dimensional grid, chunk-major: the dispatcher starts every block's first chunk before any second one
  // (mapping a contiguous eighth of this list to each XCD, so that blocks sharing q' lines read them through one
  // L2, measured 2.7 % slower: profiles/r06/ab_r06.txt)
  const int nbk = (int)(gridDim.x / (unsigned)nchunks);
  const int bk = (int)(blockIdx.x % (unsigned)nbk);
  if (a.owned && !a.owned[bk]) return;  // split basin: another rank's block
  const BlockDesc B = a.s.blocks[bk];
  const int64_t T = a.T, N = a.N;
  const int64_t tA = (int64_t)(blockIdx.x / (unsigned)nbk) * chunk;
  if (tA >= T) return;
  const int64_t tB = tA + chunk < T ? tA + chunk : T;
  const int nl = B.nloc;
  const int tid = threadIdx.x;
  const R* qp = static_cast<const R*>(a.qprime);
  const R* fs = static_cast<const R*>(a.fs);
  const unsigned char* valid = a.qp_valid;
  // read side (ascending reference order: runs of adjacent q' columns) and write side (positions, sorted by
  // tick offset: runs of one offset are contiguous in a tick row)
  int ref[KG], loc[KG];
  int64_t off[KG];
  R sc[KG];
  bool fill[KG];
#pragma unroll
  for (int k = 0; k < KG; ++k) {
    const int i = tid + k * BS;
    const bool h = i < nl;
    ref[k] = h ? a.s.rs_ref[B.pos0 + i] : 0;
    loc[k] = h ? a.s.rs_loc[B.pos0 + i] : 0;
    off[k] = h ? a.s.off[B.pos0 + i] : 0;
    sc[k] = fs ? fs[ref[k]] : R(1);
    fill[k] = valid && !valid[ref[k]];  // a divide missing from the store: the reader's 0.001 fill (readers.py:523-530)
  }
  // q' row of step t (t clamped into [0, T)): max(t - shift, 0) -- step t routes q'[t - 1] (mmc.py:421-424),
  // shift 0 in accumulation mode -- divided by the hours per stored row (readers.py:513-519)
  // (32-bit: T < 2^31; an int64 division is ~130 instructions per row, a branch around the row's loads)
  const unsigned H = (unsigned)a.qp_hours, shift = (unsigned)a.qp_shift;
  auto rowoff = [&](int64_t t64) {
    unsigned t = (unsigned)(t64 < T ? t64 : T - 1);
    t = t > shift ? t - shift : 0u;
    return (int64_t)(H == 1u ? t : t / H) * N;
  };
  R v[KG][G];
  auto load = [&](int64_t t0) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const R* row = qp + rowoff(t0 + j);
#pragma unroll
      for (int k = 0; k < KG; ++k)
        if (tid + k * BS < nl) v[k][j] = row[ref[k]];
    }
  };
  R* qs = static_cast<R*>(a.qs) + T * B.pos0 + B.pre_dn;
  bool nan = false;
  load(tA);
#pragma unroll 1
  for (int64_t t0 = tA; t0 < tB; t0 += G) {
#pragma unroll
    for (int k = 0; k < KG; ++k) {
      if (tid + k * BS >= nl) continue;
#pragma unroll
      for (int j = 0; j < G; ++j) {
        R x = fill[k] ? R(0.001f) : v[k][j];
        if (fs) x = x * sc[k];
        tile[j * nl + loc[k]] = x;
        nan = nan || x != x;
      }
    }
    __syncthreads();
    if (t0 + G < tB) load(t0 + G);  // lands while this tile is written out
    const int jn = (int)(tB - t0 < G ? tB - t0 : G);
#pragma unroll
    for (int k = 0; k < KG; ++k) {
      const int r = tid + k * BS;
      if (r >= nl) continue;
      R* col = qs + (t0 + off[k]) * nl + r;
      if (jn == G) {
#pragma unroll
        for (int j = 0; j < G; ++j) col[(int64_t)j * nl] = tile[j * nl + r];
      } else {
        for (int j = 0; j < jn; ++j) col[(int64_t)j * nl] = tile[j * nl + r];
      }
    }
    __syncthreads();
  }
  flag_nan(a, nan);
}

// Adjoint of gather_qprime: dL/dq'[s, ref] = flow_scale[ref] * sum over the steps t reading row s
// (ascending t) of gqs[tick(t, ref)]; 0 for a divide filled with 0.001 (readers.py:523-530).  Step t
// reads row max(t - 1, 0) / qp_hours (mmc.py:421-424 for t >= 1, the hot start for t = 0).  One
// thread per (row, reference reach): the writes are coalesced rows of q'.
template <typename R>
__global__ void scatter_qprime_grad_kernel(RouteArgs a, int64_t rows, R* out) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t N = a.N, T = a.T, H = a.qp_hours;
  if (w >= rows * N) return;
  const int64_t srow = w / N;
  const int ref = (int)(w % N);
  const int P = a.s.pos_of_ref[ref];
  const BlockDesc B = a.s.blocks[a.s.block_of_pos[P]];
  const int64_t r = P - B.pos0, o = a.s.off[P];
  const R* g = static_cast<const R*>(a.gqs) + T * B.pos0 + B.pre_dn;
  // steps whose row is srow: max(t - 1, 0) in [srow H, srow H + H)
  int64_t t0 = srow * H + 1, t1 = srow * H + H + 1;
  if (srow == 0) t0 = 0;
  t1 = t1 < T ? t1 : T;
  R acc = R(0);
  for (int64_t t = t0; t < t1; ++t) acc = acc + g[(t + o) * B.nloc + r];
  if (a.qp_valid && !a.qp_valid[ref]) acc = R(0);
  if (a.fs) acc = acc * static_cast<const R*>(a.fs)[ref];
  out[w] = acc;
}

// Row layout (a store of qp_hours > 1 steps per row): per block [qs_rows][nloc], row d holds q' row d
// of the store for every local position -- qp_hours times fewer bytes than the tick-major layout.
template <typename R, int G>
__global__ void __launch_bounds__(1024) gather_qprime_rows_kernel(RouteArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
  R* tile = reinterpret_cast<R*>(gsm);  // [G][nloc]
  if (a.owned && !a.owned[blockIdx.x]) return;  // split basin: another rank's block
  const BlockDesc B = a.s.blocks[blockIdx.x];
  const int64_t N = a.N, d0 = (int64_t)blockIdx.y * G;
  const int nl = B.nloc;
  const R* qp = static_cast<const R*>(a.qprime);
  const R* fs = static_cast<const R*>(a.fs);
  const int* rs_loc = a.s.rs_loc + B.pos0;
  const int* rs_ref = a.s.rs_ref + B.pos0;
  const int jn = (int)(a.qs_rows - d0 < G ? a.qs_rows - d0 : G);
  const unsigned char* valid = a.qp_valid;
  bool nan = false;
  for (int i = threadIdx.x; i < nl; i += 1024) {
    const int ref = rs_ref[i], loc = rs_loc[i];
    R v[G];
#pragma unroll
    for (int j = 0; j < G; ++j) v[j] = j < jn ? qp[(d0 + j) * N + ref] : R(0);
    if (valid && !valid[ref]) {
#pragma unroll
      for (int j = 0; j < G; ++j) v[j] = R(0.001f);  // readers.py:523-530
    }
    if (fs) {
      const R f = fs[ref];
#pragma unroll
      for (int j = 0; j < G; ++j) v[j] = v[j] * f;
    }
#pragma unroll
    for (int j = 0; j < G; ++j) {
      tile[j * nl + loc] = v[j];
      nan = nan || (j < jn && v[j] != v[j]);
    }
  }
  flag_nan(a, nan);
  __syncthreads();
  R* qs = static_cast<R*>(a.qs) + (int64_t)a.qs_rows * B.pos0;
  for (int r = threadIdx.x; r < nl; r += 1024) {
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (j < jn) qs[(d0 + j) * nl + r] = tile[j * nl + r];
  }
}

template <typename R>
hipError_t launch_gather_qprime(const Graph* g, RouteArgs& a, hipStream_t stream) {
  if (g->max_nloc == 0 || a.T == 0) return hipSuccess;
  if (a.flags & DDR_FWD_CHECK_QPRIME) {
    hipLaunchKernelGGL(nan_last_row_kernel<R>, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  constexpr int G = sizeof(R) == 4 ? 8 : 4;  // G * 4096 reaches * sizeof(R) <= 128 KiB of LDS
  const size_t smem = (size_t)G * g->max_nloc * sizeof(R);
  if (a.qs_rows > 0) {
    auto rk = gather_qprime_rows_kernel<R, G>;
    hipError_t e = hipFuncSetAttribute((const void*)rk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rk, dim3((unsigned)g->blocks.size(), (unsigned)((a.qs_rows + G - 1) / G)), dim3(1024), smem,
                       stream, a);
    return hipGetLastError();
  }
  // workgroups of (block, chunk of kTilesPerChunk tiles): short enough that the dispatcher balances blocks of
  // unequal size (a chunk of ~1000 steps left a ~1.5-ms tail behind the largest blocks), long enough that the
  // per-chunk index reads are a small fraction of the q' bytes
  auto launch = [&](auto kern, int gsteps, int bs) -> hipError_t {
    const size_t sm = (size_t)gsteps * g->max_nloc * sizeof(R);
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
    if (e != hipSuccess) return e;
    constexpr int64_t kTilesPerChunk = 4;  // C5: 13.35 ms (2: 13.34, 8: 13.45, 16: 13.73; r05's tile per workgroup 13.92)
    const int64_t nb = (int64_t)g->blocks.size();
    const int64_t chunk = kTilesPerChunk * gsteps;
    const int64_t y = (a.T + chunk - 1) / chunk;
    hipLaunchKernelGGL(kern, dim3((unsigned)(nb * y)), dim3(bs), sm, stream, a, (int)chunk, (int)y);
    return hipGetLastError();
  };
  // a workgroup covers KG * BS reaches: the last instance of each list must hold the packer's largest block
  static_assert(4 * 1024 >= kDefaultBlockReaches && kDefaultBlockReaches == kMaxKR * kBlockThreads,
                "gather_qprime_kernel<.., 1024, 4> covers fewer reaches than a block can hold");
  if constexpr (sizeof(R) == 4) {
    if (g->max_nloc <= 256) return launch(gather_qprime_kernel<R, 32, 256, 1>, 32, 256);
    if (g->max_nloc <= 512) return launch(gather_qprime_kernel<R, 32, 512, 1>, 32, 512);
    if (g->max_nloc <= 1024) return launch(gather_qprime_kernel<R, 16, 1024, 1>, 16, 1024);
    if (g->max_nloc <= 2048) return launch(gather_qprime_kernel<R, 16, 1024, 2>, 16, 1024);
    return launch(gather_qprime_kernel<R, G, 1024, 4>, G, 1024);
  } else {
    if (g->max_nloc <= 1024) return launch(gather_qprime_kernel<R, G, 1024, 1>, G, 1024);
    if (g->max_nloc <= 2048) return launch(gather_qprime_kernel<R, G, 1024, 2>, G, 1024);
    return launch(gather_qprime_kernel<R, G / 2, 1024, 4>, G / 2, 1024);  // (G = 4: spills at four reaches)
  }
}

template <typename R>
hipError_t launch_scatter_qprime_grad(const Graph* g, const RouteArgs& a, int64_t rows, R* out, hipStream_t stream) {
  const int64_t total = rows * g->n;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(scatter_qprime_grad_kernel<R>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a,
                     rows, out);
  return hipGetLastError();
}

template hipError_t launch_gather_qprime<float>(const Graph*, RouteArgs&, hipStream_t);
template hipError_t launch_gather_qprime<double>(const Graph*, RouteArgs&, hipStream_t);
template hipError_t launch_scatter_qprime_grad<float>(const Graph*, const RouteArgs&, int64_t, float*, hipStream_t);
template hipError_t launch_scatter_qprime_grad<double>(const Graph*, const RouteArgs&, int64_t, double*, hipStream_t);

}  // namespace ddr
