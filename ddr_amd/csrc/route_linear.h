// Linear Muskingum routing (RAPID's matrix scheme) on the routing schedule: launch arguments and
// launchers of route_linear.hip.
#pragma once

#include "internal.h"

namespace ddr {

// ddr_lin_route flags (include/ddr_mc.h: DDR_LIN_END, DDR_LIN_STEADY) live in the low bits of `flags`;
// kFlagForceTimeout (internal.h) is honoured as in the Muskingum-Cunge forward.
struct LinArgs {
  DevSchedule s;
  int64_t N;
  int64_t F;            // forcing intervals (rows of qext, columns of out)
  int32_t S;            // sub-steps per forcing interval
  int32_t TS;           // states per reach: the initial one and F * S routed ones
  int32_t flags;
  int32_t slot_stride;  // LDS slots per buffer (route_slot_stride)
  int32_t nblocks;
  int32_t xl_off;       // byte offset of the confluence lists in the dynamic LDS
  double dt;            // sub-step, seconds
  const void* k;        // (N) storage constant, seconds (R)
  const void* x;        // (N) weighting factor (R)
  const void* q0;       // (N) initial state (R), or null
  const void* qs;       // gathered forcing, per block [F][nloc] (R)
  void* out;            // (N, F) (R)
  void* q_last;         // (N) (R)
  double* bnd;          // cut-edge granules [n_cut][TS]
  unsigned* status;
};

// the persistent launch over all F * S sub-steps (0 resident workgroups: hipErrorLaunchOutOfResources)
template <typename R>
hipError_t launch_route_linear(const Graph* g, LinArgs a, hipStream_t stream);
// workgroups of the kernel the device holds at this schedule's LDS size (0: none fits; -1: query failed)
template <typename R>
int linear_resident_blocks(const Graph* g);
// gauge rows of an (N, F) output: out[g, f] = sum over the gauge's reaches, in list order
template <typename R>
hipError_t launch_linear_gauge(int64_t G, int64_t F, const int64_t* goff, const int64_t* gidx, const R* nf, R* out,
                               hipStream_t stream);

}  // namespace ddr
