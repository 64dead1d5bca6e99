// Split basin (one basin's schedule shared by several ranks, SplitState in internal.h): the kernels around
// a routing launch -- the epoch hand-shake before it and the hand-over of received rows after a forward.
#include <algorithm>

#include "route_device.h"

namespace ddr {

// Split basin: before a routing launch, every rank of the split announces (system-scope store into each
// peer's epoch word) that its receive rows are reset for launch `epoch` and waits until every peer has
// announced the same; only then may a peer's blocks write into them.  Bounded: a peer that never
// arrives is recorded in the status block (DDR_ERR_TIMEOUT at the next library call).
__global__ void split_barrier_kernel(SplitBarrierArgs b) {
  if (threadIdx.x != 0) return;
  for (int p = 0; p < b.nranks; ++p) {
    if (p == b.rank) continue;
    __hip_atomic_store(b.peer[p] + b.slot * kMaxSplitRanks + b.rank, b.epoch, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
  for (int p = 0; p < b.nranks; ++p) {
    if (p == b.rank) continue;
    unsigned spins = 0;
    while (__hip_atomic_load(b.mine + b.slot * kMaxSplitRanks + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) <
           b.epoch) {
      if (++spins > (1u << 22)) {  // ~10 s
        atomicAdd(b.status, 1u);
        atomicCAS(b.status + 1, 0u, 0x40000000u + (unsigned)p);
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
  }
}

hipError_t launch_split_barrier(const SplitBarrierArgs& b, hipStream_t stream) {
  hipLaunchKernelGGL(split_barrier_kernel, dim3(1), dim3(64), 0, stream, b);
  return hipGetLastError();
}

// Split basin, after the forward (grid-stride over n_x rows x T): rows received from another rank
// (xcons == this rank) -> bnd[edge] (the per-call boundary buffer the autograd node keeps; a later forward
// on the same graph resets and rewrites the receive rows); and a NaN in column 0 of every runoff row of a
// reach whose block another rank runs (those rows are never written: misuse shows as NaN, not as stale
// memory).  The last-step outputs of those reaches are NaN as well (route_last_kernel).
template <typename R>
__global__ void split_finish_kernel(RouteArgs a, int64_t n_x) {
  const int64_t T = a.T;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_x * T; w += stride) {
    const int64_t xi = w / T, t = w % T;
    if (a.xcons[xi] != a.xrank) continue;
    a.bnd[a.xedge[xi] * T + t] = __longlong_as_double(load_granule_sys(a.xfwd + w));
  }
  if (a.runoff) {
    for (int64_t P = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; P < a.N; P += stride)
      if (!a.owned[a.s.block_of_pos[P]]) static_cast<R*>(a.runoff)[(int64_t)a.s.ref[P] * T] = R(__builtin_nan(""));
  }
}

template <typename R>
hipError_t launch_split_finish(const Graph* g, const RouteArgs& a, hipStream_t stream) {
  if (g->split.nranks == 0) return hipSuccess;
  const int64_t work = std::max<int64_t>((int64_t)g->split.n_x * a.T, g->n);
  const unsigned nb = (unsigned)std::min<int64_t>((work + 255) / 256, 4096);
  hipLaunchKernelGGL(split_finish_kernel<R>, dim3(nb), dim3(256), 0, stream, a, (int64_t)g->split.n_x);
  return hipGetLastError();
}

template hipError_t launch_split_finish<float>(const Graph*, const RouteArgs&, hipStream_t);
template hipError_t launch_split_finish<double>(const Graph*, const RouteArgs&, hipStream_t);

}  // namespace ddr
