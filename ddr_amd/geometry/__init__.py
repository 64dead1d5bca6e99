"""``ddr.geometry`` on the HIP device: the trapezoid geometry, its temporal statistics and the geometry predictor."""

from .adapters import (HYDROATLAS_TO_MERIT, MERIT_ATTRIBUTE_NAMES, AttributeMapping, adapt_attributes,
                       detect_source)
from .predictor import GEOMETRY_OUTPUTS, GeometryPredictor
from .statistics import compute_geometry_statistics
from .trapezoidal import compute_trapezoidal_geometry

__all__ = ["GeometryPredictor", "GEOMETRY_OUTPUTS", "compute_geometry_statistics", "compute_trapezoidal_geometry",
           "MERIT_ATTRIBUTE_NAMES", "AttributeMapping", "HYDROATLAS_TO_MERIT", "detect_source", "adapt_attributes"]
