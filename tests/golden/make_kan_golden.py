"""Generate ``kan_merit.npz`` and ``kan_lynker.npz``: the WEIGHTS of the reference's two published KAN
checkpoints.  BUILD-CONTAINER ONLY (it reads the reference checkout).

Each fixture holds only the checkpoint's ``model_state_dict`` arrays under their reference key names
(``input.weight``, ``layers.0.act_fun.0.coef`` ...; fp32, ~200 KB): no optimizer or RNG state, and no outputs.
They are weights, not reference results -- pykan cannot run where the tests run, so the expected values of
``tests/test_kan_api.py`` / ``tests/test_gpu_kan.py`` come from ``ddr_amd.nn.TorchKan`` in fp64 at test time.

    python tests/golden/make_kan_golden.py --reference <checkout of taddyb/ddr>
"""

from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
CHECKPOINTS = {
    "kan_merit": "examples/merit/ddr-v0.5.2-merit-geometry-weights.pt",
    "kan_lynker": "examples/lynker_hydrofabric/ddr-v0.5.2.lynker_hydrofabric_trained_weights.pt",
}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", type=Path, required=True, help="checkout of the reference (taddyb/ddr)")
    args = ap.parse_args()
    for name, rel in CHECKPOINTS.items():
        state = torch.load(args.reference / rel, map_location="cpu", weights_only=False)
        arrays = {k: v.numpy() for k, v in state["model_state_dict"].items()}
        np.savez(HERE / f"{name}.npz", **arrays)
        print(name, len(arrays), "arrays", sum(a.nbytes for a in arrays.values()), "bytes")


if __name__ == "__main__":
    main()
