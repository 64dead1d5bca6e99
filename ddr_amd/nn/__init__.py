"""``ddr.nn`` on the HIP device: the KAN that produces the routing parameters."""

from .kan import TorchKan, kan, load_checkpoint

__all__ = ["kan", "TorchKan", "load_checkpoint"]
