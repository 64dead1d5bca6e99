"""Time ``GeometryPredictor.predict`` (csrc/geopredict.hip: two kernels around the KAN's launches) against the same
result composed from PyTorch ops around ``ddr_amd.nn.kan`` -- the path a user had before the predictor -- on the
same device, in the same run, the two sides alternating.  Attributes are already on the device as (F, N) in MERIT
units (the global MERIT run of scripts/geometry_predictor.py), ``check_distribution=False`` (no read-back), the
published checkpoint's architecture and weights, N = 2.9 M (MERIT global) and 800 k.

Each stage is timed on its own (HIP events around each repetition, warm-up, median of 20) and as a whole; the two
new kernels' achieved bytes/s use the algorithmic traffic: 80 B/row for the prepare kernel at F = 10 (read F,
write F floats), 64 B/row for the geometry kernel at O = 3 (read 3 + 2, write 11 floats).  Prints one JSON line per
size (committed as profiles/geopredict_time.txt).

    python tools/geopredict_time.py [--rows 2900000 800000] [--reps 20] [--warmup 3]
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from ddr_amd.geometry import GEOMETRY_OUTPUTS, GeometryPredictor, compute_trapezoidal_geometry  # noqa: E402
from ddr_amd.geometry.predictor import geometry_predict, prepare_attributes  # noqa: E402
from ddr_amd.nn import kan  # noqa: E402
from ddr_amd.routing.utils import denormalize  # noqa: E402

RANGES = {"n": [0.015, 0.25], "q_spatial": [0.0, 1.0], "p_spatial": [1.0, 200.0]}
MINS = {"discharge": 0.0001, "slope": 0.001, "velocity": 0.01, "depth": 0.01, "bottom_width": 0.01}
LEARN = ["n", "q_spatial", "p_spatial"]


def alternate_ms(fns: dict, warmup: int, reps: int) -> dict:
    """Median device time of each callable, the callables taking turns within every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[k].append(start.elapsed_time(stop))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def measure(N: int, net, dev, reps: int, warmup: int) -> dict:
    F = 10
    g = torch.Generator().manual_seed(N)
    mean = torch.randn(F, generator=g).to(dev)
    std = (torch.rand(F, generator=g) + 0.5).to(dev)
    raw = (torch.randn(F, N, generator=g) * 1.5).to(dev) * std[:, None] + mean[:, None]
    raw[:, ::97] = float("nan")  # ~1 % missing
    Q = torch.exp(torch.randn(N, generator=g) * 2).to(dev)
    S = torch.exp(torch.randn(N, generator=g) - 6).to(dev)
    S[::13] = float("nan")  # (reaches without a slope: NaN geometry)
    names = [f"a{i}" for i in range(F)]
    gp = GeometryPredictor(net, names, mean, std, RANGES, ["p_spatial"], {"p_spatial": 21}, MINS, device=dev,
                           check_distribution=False)
    one, zero = torch.ones(F, dtype=torch.float64, device=dev), torch.zeros(F, dtype=torch.float64, device=dev)
    flag = torch.zeros(F, dtype=torch.int32, device=dev)
    keep = {}

    # ---- the predictor, whole and by stage ----
    def fused():
        keep["fused"] = gp.predict(raw, Q, S)

    def fused_prepare():
        keep["x"] = prepare_attributes(raw, one, zero, flag, mean, std)

    def fused_kan():
        with torch.no_grad():
            o = net(inputs=keep["x"])
        keep["u"] = torch.stack([o[k] for k in LEARN], dim=1)

    def fused_geometry():
        keep["g"] = geometry_predict(keep["u"], gp._slots, Q, S, MINS)

    # ---- the same from PyTorch ops (predictor.py:241-274, 276-318, 203-238 of the reference, on the device) ----
    def torch_prepare():
        v = torch.where(torch.isnan(raw), mean[:, None], raw)
        keep["xt"] = ((v - mean[:, None]) / std[:, None]).T.contiguous()

    def torch_post():
        o = keep["o"]
        n = denormalize(o["n"], RANGES["n"], False)
        q = denormalize(o["q_spatial"], RANGES["q_spatial"], False)
        p = denormalize(o["p_spatial"], RANGES["p_spatial"], True)
        geo = compute_trapezoidal_geometry(n, p, q, torch.clamp(Q, min=MINS["discharge"]), torch.clamp(S, min=MINS["slope"]),
                                           depth_lb=MINS["depth"], bottom_width_lb=MINS["bottom_width"])
        keep["torch"] = dict(geo, n=n, p_spatial=p, q_spatial=q)

    def torch_kan():
        with torch.no_grad():
            keep["o"] = net(inputs=keep["xt"])

    def composed():
        torch_prepare()
        torch_kan()
        torch_post()

    fused_prepare(), fused_kan(), torch_prepare(), torch_kan()
    whole = alternate_ms({"predict": fused, "torch_composed": composed}, warmup, reps)
    stage = alternate_ms({"prepare_kernel": fused_prepare, "torch_prepare_ops": torch_prepare,
                          "geometry_kernel": fused_geometry, "torch_geometry_ops": torch_post,
                          "kan_launches": torch_kan, "kan_and_stack": fused_kan}, warmup, reps)
    torch.cuda.synchronize()
    # the two sides compute the same thing
    diff = {}
    for name in GEOMETRY_OUTPUTS:
        a, b = keep["fused"][name].double(), keep["torch"][name].double()
        fin = torch.isfinite(b)
        diff.setdefault("nan_mismatches", 0)
        diff["nan_mismatches"] += int((torch.isnan(a) != torch.isnan(b)).sum())
        diff[name] = float(((a - b)[fin].abs() / b[fin].abs()).max())
    new, old = stage["prepare_kernel"] + stage["geometry_kernel"], stage["torch_prepare_ops"] + stage["torch_geometry_ops"]
    return {"tool": "geopredict_time", "device": torch.cuda.get_device_name(0), "rows": N, "reps": reps, "warmup": warmup,
            "chunk_rows": gp.chunk_rows, "whole_ms": whole, "stage_ms": stage,
            "new_kernels_ms": round(new, 4), "torch_ops_replaced_ms": round(old, 4), "ratio": round(old / new, 2),
            "prepare_gb_per_s": round(80.0 * N / stage["prepare_kernel"] / 1e6, 1),
            "geometry_gb_per_s": round(64.0 * N / stage["geometry_kernel"] / 1e6, 1),
            "max_rel_diff_vs_torch": {k: float(f"{v:.3g}") for k, v in diff.items()}}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2_900_000, 800_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    net = kan([f"a{i}" for i in range(10)], LEARN, 21, 2, 50, 2, 0, device=dev)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(ROOT / "tests" / "golden" / "kan_merit.npz").items()})
    for N in args.rows:
        out = measure(N, net, dev, args.reps, args.warmup)
        print(json.dumps(out), flush=True)
        assert out["new_kernels_ms"] < out["torch_ops_replaced_ms"], "the two kernels are slower than the ops they replace"


if __name__ == "__main__":
    main()
