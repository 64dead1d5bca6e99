// Host side of a routing launch, shared by route_forward.hip, route_linear.hip and route_backward.h: the
// dynamic-LDS plan (one definition for the launches, the backward's buffer choice and the occupancy queries),
// the launch geometry and the dispatch on the graph's reaches per thread.
#pragma once

#include <type_traits>

#include "internal.h"
#include "route_args.h"

namespace ddr {

// Split basin: after the layout, each block's granule rows (tagged pointers, bit 0 = another rank's
// memory: system scope): forward, its cut-outs' export rows; backward, its virtuals' export rows then
// its cut-outs' import rows -- resolved once per launch, no dependent global load per hand-off
inline size_t split_table_bytes(const Graph* g, bool backward) {
  if (g->split.nranks == 0) return 0;
  return 8 * (size_t)(backward ? g->max_virt + g->max_cout : g->max_cout);
}

// Dynamic LDS of a routing launch on this graph (route_lds_bytes, internal.h): `base` bytes of layout
// closed by the confluence lists, then the split basin's row table; `smem` in all.  The offsets are the
// kernels' RouteArgs fields of the same names.
struct RouteLds {
  size_t base, smem;
  int32_t xl_off, own_off, xt_off;
};
// xb: the slot buffers when not the KR rule's (0), as route_lds_bytes
template <typename R>
RouteLds route_lds_plan(const Graph* g, bool backward, int xb) {
  RouteLds p;
  p.base = route_lds_bytes((size_t)route_slot_stride(g->max_slots), (size_t)g->max_virt, (size_t)g->max_cout,
                           (size_t)g->max_xl, backward, sizeof(R), g->kr, xb);
  p.smem = align16(p.base) + split_table_bytes(g, backward);
  p.xl_off = (int32_t)(p.base - (size_t)g->max_xl * 4);  // the lists close the base LDS layout
  p.own_off = p.xl_off - (int32_t)route_own_bytes((size_t)g->max_virt, (size_t)g->max_cout, true);
  p.xt_off = g->split.nranks > 0 ? (int32_t)align16(p.base) : 0;
  return p;
}

// The launch arguments that follow from the graph and the plan: those of every kernel on the schedule
// (RouteArgs, LinArgs), then the Muskingum-Cunge kernels' own
template <typename Args>
void set_schedule_args(Args& a, const Graph* g, const RouteLds& p) {
  a.slot_stride = route_slot_stride(g->max_slots);
  a.nblocks = (int32_t)g->blocks.size();
  a.xl_off = p.xl_off;
}
inline void set_launch_args(RouteArgs& a, const Graph* g, const RouteLds& p) {
  set_schedule_args(a, g, p);
  a.n_cut = g->n_cut;
  a.own_off = p.own_off;
  a.xt_off = p.xt_off;
}

// f(std::integral_constant<int, KR>{}) for the graph's reaches per thread (1, 2 or 4: kr_of_load)
template <typename F>
auto dispatch_kr(const Graph* g, F&& f) {
  switch (g->kr) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// Workgroups of kernel `f` resident on the device with `smem` bytes of dynamic LDS each (-1: query failed)
inline int resident_blocks(const Graph* g, const void* f, size_t smem) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, kBlockThreads, smem) != hipSuccess) return -1;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, g->device) != hipSuccess) return -1;
  return nb * prop.multiProcessorCount;
}

}  // namespace ddr
