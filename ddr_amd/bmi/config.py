"""The YAML schema of ``DdrBmi.initialize`` (reference ``src/ddr/bmi/config.py``): the same fields and defaults."""

from __future__ import annotations

from pathlib import Path
from typing import Literal

from pydantic import BaseModel


class BmiInitConfig(BaseModel):
    """``ddr_config``: DDR's YAML config; ``kan_checkpoint``: the trained KAN; ``hydrofabric_gpkg`` /
    ``conus_adjacency``: overrides of the config's data sources; ``device``; ``timestep_seconds``: the routing step
    (a coupling interval of ngen is ``round(interval / timestep_seconds)`` sub-steps); ``interpolation``: how the
    sub-steps' lateral inflows are made, ``"constant"`` (hold) or ``"linear"`` (from the previous interval's inflows
    to this one's)."""

    ddr_config: Path
    kan_checkpoint: Path
    hydrofabric_gpkg: Path | None = None
    conus_adjacency: Path | None = None
    device: str = "cpu"
    timestep_seconds: float = 3600.0
    interpolation: Literal["constant", "linear"] = "constant"
