"""Drop-in for ``ddr.bmi`` (reference ``src/ddr/bmi``): the BMI 2.0 coupling of the routing to ngen, device-resident."""

from .config import BmiInitConfig
from .ddr_bmi import DdrBmi

__all__ = ["BmiInitConfig", "DdrBmi"]
