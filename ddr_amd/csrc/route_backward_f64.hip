// The fp64 instances of the adjoint routing kernel and its launch (route_backward.h).
#include "route_backward.h"

namespace ddr {
DDR_INSTANTIATE_ROUTE_BACKWARD(double)
}  // namespace ddr
