"""Drop-in replacement of ``ddr.routing`` on the MI355X routing kernels."""

from .linear import LinearMuskingum, muskingum_coefficient_gradients, muskingum_coefficients, rapid_parameters
from .mmc import MuskingumCunge, compute_hotstart_discharge
from .torch_mc import dmc
from .utils import PatternMapper, denormalize, get_network_idx, triangular_sparse_solve

__all__ = ["MuskingumCunge", "compute_hotstart_discharge", "dmc", "PatternMapper", "denormalize",
           "get_network_idx", "triangular_sparse_solve", "LinearMuskingum", "muskingum_coefficients",
           "rapid_parameters", "muskingum_coefficient_gradients"]
