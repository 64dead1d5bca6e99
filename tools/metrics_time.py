#!/usr/bin/env python
"""Time ddr_amd.validation.metrics_device with HIP events on synthetic series (needs an MI355X, nothing else).

    python tools/metrics_time.py                      # 256 x 89 (a C3 training batch) and 3000 x 5479 (evaluation)
    python tools/metrics_time.py --shape 64x89 --reps 50

Prints, per shape, the median and the minimum of `reps` timed calls after `warmup` untimed ones (events around
the call on the current stream: the launch and its memset, no host sync inside) and one JSON line at the end.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ddr_amd.validation import metrics_device  # noqa: E402


def series(G: int, D: int, device, seed: int = 0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    walk = torch.exp(torch.randn(G, 1, generator=gen) + torch.cumsum(0.1 * torch.randn(G, D, generator=gen), dim=1))
    pred = walk * torch.exp(0.15 * torch.randn(G, D, generator=gen))
    target = walk.round(decimals=1)
    target[torch.rand(G, D, generator=gen) < 0.1] = float("nan")
    return pred.to(device), target.to(device)


def time_shape(G: int, D: int, reps: int, warmup: int, device) -> dict:
    pred, target = series(G, D, device)
    for _ in range(warmup):
        metrics_device(pred, target)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        metrics_device(pred, target)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"gauges": G, "days": D, "median_ms": statistics.median(ms), "min_ms": min(ms), "reps": reps}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", action="append", help="GxD, repeatable (default: 256x89 and 3000x5479)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_time needs a HIP device")
    device = torch.device("cuda:0")
    shapes = [tuple(int(v) for v in s.lower().split("x")) for s in (args.shape or ["256x89", "3000x5479"])]
    rows = []
    for G, D in shapes:
        r = time_shape(G, D, args.reps, args.warmup, device)
        print(f"{G} x {D}: median {r['median_ms']:.3f} ms, min {r['min_ms']:.3f} ms over {args.reps} calls")
        rows.append(r)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "metrics_ms": rows}))


if __name__ == "__main__":
    main()
