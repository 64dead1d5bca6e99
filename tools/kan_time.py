"""Time the fused KAN (``ddr_amd.nn.kan``, csrc/kan.hip) against ``TorchKan`` in fp32 on the same device, in the
same run: forward + backward (gradient of the flat parameter vector for L = sum u w) and the no-grad forward, at
the published checkpoints' architecture (F = 10, H = 21, 2 layers, G = 50, k = 2, 3 outputs) and C3's reach
count.  HIP events around each repetition, warm-up, median of 20.  Prints one JSON line
(committed as profiles/kan/kan_time.json).

    python tools/kan_time.py [--rows 900000] [--reps 20] [--warmup 3]
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

from ddr_amd.nn import TorchKan, kan  # noqa: E402


def median_ms(fn, warmup: int, reps: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=900_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = dict(input_var_names=[f"a{i}" for i in range(10)], learnable_parameters=["n", "q_spatial", "p_spatial"],
              hidden_size=21, num_hidden_layers=2, grid=50, k=2, seed=0)
    fused, base = kan(**kw, device=dev), TorchKan(**kw, device=dev)
    weights = ROOT / "tests" / "golden" / "kan_merit.npz"  # the trained weights: inputs spread far past the knots
    sd = {k: torch.from_numpy(v) for k, v in np.load(weights).items()}
    fused.load_state_dict(sd)
    base.load_state_dict(sd)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(args.rows, 10, generator=g).to(dev)
    w = torch.randn(args.rows, 3, generator=g).to(dev)

    def train(net):
        def step():
            net.flat.grad = None
            o = net(inputs=x)
            (torch.stack(list(o.values()), dim=1) * w).sum().backward()
        return step

    def infer(net):
        def step():
            with torch.no_grad():
                net(inputs=x)
        return step

    out = {"tool": "kan_time", "device": torch.cuda.get_device_name(0), "rows": args.rows,
           "arch": {"F": 10, "H": 21, "L": 2, "G": 50, "k": 2, "O": 3}, "reps": args.reps, "warmup": args.warmup,
           "weights": "tests/golden/kan_merit.npz", "inputs": "N(0, 1)"}
    for name, net in (("fused", fused), ("torchkan_fp32", base)):
        out[f"{name}_fwd_bwd_ms"] = round(median_ms(train(net), args.warmup, args.reps), 4)
        out[f"{name}_fwd_nograd_ms"] = round(median_ms(infer(net), args.warmup, args.reps), 4)
        torch.cuda.synchronize()
        out[f"{name}_peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2**30, 3)
        torch.cuda.reset_peak_memory_stats()
    out["speedup_fwd_bwd"] = round(out["torchkan_fp32_fwd_bwd_ms"] / out["fused_fwd_bwd_ms"], 2)
    out["speedup_fwd_nograd"] = round(out["torchkan_fp32_fwd_nograd_ms"] / out["fused_fwd_nograd_ms"], 2)
    # the two paths compute the same thing
    with torch.no_grad():
        a, b = fused(inputs=x[:4096]), base(inputs=x[:4096])
    out["max_abs_diff_4096_rows"] = float(max((a[k] - b[k]).abs().max() for k in a))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
