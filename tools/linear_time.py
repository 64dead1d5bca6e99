#!/usr/bin/env python
"""Time ddr_amd.routing.LinearMuskingum with HIP events (needs an MI355X) and write profiles/linear/linear.json.

    python tools/linear_time.py                       # both shapes
    python tools/linear_time.py --reps 5 --out /tmp/linear.json

Two shapes:

* ``c3``    the training batch of ``bench.py --workload c3`` (256 gauged subnetworks, 2136 hourly steps): S = 1,
            ``output="end"``, the benchmark arm's call;
* ``rapid`` 800 000 reaches, 80 forcing intervals of 12 sub-steps, ``output="mean"``: a RAPID-shaped run.

Per shape the linear route is timed against two references on the same device and graph: the forward of
``ops.route`` under ``no_grad`` at the same number of steps (existing code that does a superset of each tick's
work: the physics, the saved states, the runoff rows), and a streaming copy of the bytes the call must read and
write (the forcing once, the output once).  The ratios go into the JSON; the call's own two launches (the forcing
gather, the routing kernel) are timed apart as well.
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

from ddr_amd import _lib, synthetic  # noqa: E402
from ddr_amd.graph import RiverGraph  # noqa: E402
from ddr_amd.ops import route  # noqa: E402
from ddr_amd.routing import LinearMuskingum  # noqa: E402


def timed(fn, reps: int, warmup: int) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "reps": reps}


def shape(name: str, net, F: int, S: int, output: str, args, dev) -> dict:
    n, T = net.n, F * S
    g = RiverGraph(net.n, net.rows, net.cols, steps_hint=T)
    gen = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda lo, hi, *shp: torch.empty(shp, device=dev).uniform_(lo, hi, generator=gen)  # noqa: E731
    lm = LinearMuskingum(g, rnd(600.0, 40000.0, n), rnd(0.0, 0.5, n), dt=3600.0 if S == 1 else 900.0, substeps=S)
    qext = rnd(0.0, 3.0, F, n)
    with torch.no_grad():
        lin = timed(lambda: lm(qext, output=output), args.reps, args.warmup)
        out, _ = lm(qext, output=output)
        nbytes = qext.numel() * 4 + out.numel() * 4
        del out
        # the streaming copy of those bytes: half read, half written
        src = torch.empty(nbytes // 8, device=dev, dtype=torch.float32)
        dst = torch.empty_like(src)
        cp = timed(lambda: dst.copy_(src), args.reps, args.warmup)
        del src, dst
        # the Muskingum-Cunge forward at the same number of steps, on the same graph
        at = synthetic.reach_attributes(n, 3)
        u = synthetic.unit_parameters(n, 3)
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.float32)  # noqa: E731
        nn_, qq, pp = (tt(u["n"]) * 0.235 + 0.015, tt(u["q_spatial"]), tt(u["p_spatial"]) * 20.0 + 1.0)
        length, slope, xs = tt(at.length), tt(np.maximum(at.slope, np.float32(1e-3))), tt(at.x)
        qh = rnd(0.0, 3.0, T, n)
        mc = timed(lambda: route(g, qh, nn_, qq, pp, length, slope, xs, math="faithful"), args.reps, args.warmup)
    r = {"shape": name, "reaches": n, "F": F, "S": S, "steps": T, "output": output, "graph": repr(g),
         "linear": lin, "mc_forward": mc, "copy": cp, "bytes": nbytes,
         "linear_over_mc_forward": lin["median_ms"] / mc["median_ms"],
         "linear_over_copy": lin["median_ms"] / cp["median_ms"],
         "reach_steps_per_s": n * T / (lin["median_ms"] * 1e-3)}
    print(f"{name}: {g}\n  linear {lin['median_ms']:.3f} ms, MC forward {mc['median_ms']:.3f} ms "
          f"(ratio {r['linear_over_mc_forward']:.3f}), copy of {nbytes / 1e9:.2f} GB {cp['median_ms']:.3f} ms "
          f"(ratio {r['linear_over_copy']:.2f})", flush=True)
    return r


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("c3", "rapid"), default=None)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "linear" / "linear.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_time needs a HIP device")
    dev = torch.device("cuda:0")
    rows = []
    if args.only in (None, "c3"):
        net = synthetic.forest(synthetic.loguniform_sizes(256, 100, 20000, 3), seed=3, single_inflow=0.25)
        rows.append(shape("c3", net, 2136, 1, "end", args, dev))
        torch.cuda.empty_cache()
    if args.only in (None, "rapid"):
        net = synthetic.forest(synthetic.zipf_sizes(800_000, 1000, 0.375), seed=0)
        rows.append(shape("rapid", net, 80, 12, "mean", args, dev))
    args.out.parent.mkdir(parents=True, exist_ok=True)
    doc = {"device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(), "shapes": rows}
    args.out.write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
