#!/usr/bin/env python
"""Time the masked daily objectives (ddr_amd.train.daily_objective) with HIP events (needs an MI355X).

    python tools/objective_time.py                       # 256 x 89 (warm-up 3) and 3000 x 5113 (warm-up 0)
    python tools/objective_time.py --eval-gauges 1000 --reps 10 --out /tmp/objective.json

Series after the recipe of tests/objective_cases.py (a log-normal walk, targets quantised to 0.1); the observations
carry 10 % missing days in one gauge out of four, so the reference's filter keeps three quarters of the gauges.
Every variant is one forward + backward (loss and dL/d daily), timed as the median / minimum / maximum of ``reps``
windows of ``inner`` calls, the variants of a shape alternating inside every repetition (tools/feed_time.py's
``timed_group``).  Per kind:

* (a) ``fused``: ``daily_objective(daily, obs, warmup, kind, drop=has_nan)`` (for l1, so that it computes what (c)
  does; without ``drop`` for the other kinds: a NaN is a missing day);
* (b) ``torch``: the same objective as a sync-free PyTorch composition (``objective_cases.torch_objective``:
  ``torch.where`` masks, autograd);
* (c) ``boolean_index``, l1 only: the form INTEGRATION.md documented before, ``keep = ~has_nan``,
  ``l1_loss(daily[keep][:, w:], obs[keep][:, w:])`` -- boolean indexing, so the host waits for the device;
* (d) ``daily_l1``, l1 only, on gap-free observations: ``daily_l1_loss`` itself, next to ``fused_full``, the masked
  call on the same gap-free data.

Eager calls at the training shape are bound by the host (Python, the allocator, the launches), so every sync-free
variant is also timed as a captured graph (``*_graph``: one graph launch per forward + backward).

The launch counts of (a), (b) and (c) are taken from ``torch.profiler`` (device kernels and memory operations of one
call; null where the profiler gives none).  No condition is attached to the times: they are reported.  One JSON line
with the library's build hash, also written to ``--out`` (default ``profiles/objective/objective.json``).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import objective_cases as oc  # noqa: E402
from ddr_amd import _lib  # noqa: E402
from ddr_amd.capture import CapturedStep  # noqa: E402
from ddr_amd.train import OBJECTIVE_KINDS, daily_l1_loss, daily_objective  # noqa: E402
from feed_time import timed_group  # noqa: E402


def series(G: int, D: int, seed: int):
    rng = np.random.default_rng(seed)
    walk = np.exp(rng.normal(0.0, 1.0, (G, 1)) + np.cumsum(rng.normal(0.0, 0.1, (G, D)), axis=1))
    pred = (walk * np.exp(rng.normal(0.0, 0.15, (G, D)))).astype(np.float32)
    full = np.round(walk, 1).astype(np.float32) + np.float32(0.1)
    gappy = full.copy()
    holes = rng.uniform(size=(G, D)) < 0.1
    holes[np.arange(G) % 4 != 0] = False
    gappy[holes] = np.nan
    return pred, full, gappy


def device_launches(fn) -> int | None:
    """Device kernels and memory operations of one call of ``fn``, by torch.profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception as exc:  # the profiler is optional: the times do not depend on it
        print(f"launch count unavailable: {exc}", flush=True)
        return None


def shape_result(device, G: int, D: int, warmup: int, reps: int, warm: int, inner: int) -> dict:
    pred, full, gappy = series(G, D, 20140 + D)
    leaf = torch.from_numpy(pred).to(device).requires_grad_(True)
    obs_full = torch.from_numpy(full).to(device)
    obs = torch.from_numpy(gappy).to(device)
    has_nan = obs.isnan().any(dim=1)
    kept = int((~has_nan).sum())

    def backward_of(make_loss):
        def fn():
            leaf.grad = None
            make_loss().backward()
        return fn

    out = {"gauges": G, "days": D, "warmup": warmup, "kept_gauges": kept, "inner": inner, "kinds": {}}
    for kind in OBJECTIVE_KINDS:
        drop = has_nan if kind == "l1" else None
        fns = {
            "fused": backward_of(lambda: daily_objective(leaf, obs, warmup, kind, drop=drop)),
            "torch": backward_of(lambda: oc.torch_objective(leaf, obs, warmup, kind, drop=drop)),
        }
        if kind == "l1":
            fns["boolean_index"] = backward_of(lambda: oc.boolean_index_l1(leaf, obs, warmup))
            fns["fused_full"] = backward_of(lambda: daily_objective(leaf, obs_full, warmup, "l1"))
            fns["daily_l1"] = backward_of(lambda: daily_l1_loss(leaf, obs_full, warmup))
        # the same values, at the timed size: the fused call against the composition run in float64 on the device
        # (the fp32 composition's own distance from it is reported: it loses digits on long windows)
        fns["fused"]()
        a_loss, a_grad = daily_objective(leaf, obs, warmup, kind, drop=drop).item(), leaf.grad.clone()
        leaf64 = leaf.detach().double().requires_grad_(True)
        ref = oc.torch_objective(leaf64, obs.double(), warmup, kind, drop=drop)
        ref.backward()
        fns["torch"]()
        b_loss = oc.torch_objective(leaf, obs, warmup, kind, drop=drop).item()
        top = leaf64.grad.abs().max()
        agree = {"fused_loss_rel": abs(a_loss - ref.item()) / abs(ref.item()),
                 "fused_grad_rel": float((a_grad - leaf64.grad).abs().max() / top),
                 "torch_fp32_loss_rel": abs(b_loss - ref.item()) / abs(ref.item()),
                 "torch_fp32_grad_rel": float((leaf.grad - leaf64.grad).abs().max() / top)}
        del leaf64, ref
        if kind == "l1":
            fns["boolean_index"]()
            agree["boolean_index_grad_rel"] = float((a_grad - leaf.grad).abs().max() / leaf.grad.abs().max())
            fns["fused_full"]()
            g_full = leaf.grad.clone()
            fns["daily_l1"]()
            agree["daily_l1_grad_bits_equal"] = bool(torch.equal(g_full.view(torch.int32), leaf.grad.view(torch.int32)))
        if max(v for k, v in agree.items() if k.startswith(("fused_", "boolean_"))) > 1e-5:
            raise SystemExit(f"the variants disagree at {G} x {D} {kind}: {agree}")
        launches = {k: device_launches(fn) for k, fn in fns.items() if k in ("fused", "torch", "boolean_index")}
        # the sync-free variants once more as captured graphs (ddr_amd.capture.CapturedStep): one graph launch per
        # call, so the device's share of the time without the host's
        for k in [k for k in fns if k != "boolean_index"]:
            fns[k + "_graph"] = CapturedStep(fns[k])
        t = timed_group(fns, reps, warm, inner)
        for k, v in t.items():
            print(f"{G} x {D} {kind} {k}: median {v['median_ms'] * 1e3:.1f} us, min {v['min_ms'] * 1e3:.1f} us, "
                  f"max {v['max_ms'] * 1e3:.1f} us, launches {launches.get(k)}", flush=True)
        out["kinds"][kind] = {"timings": t, "launches_forward_backward": launches, "agreement": agree,
                              "fused_vs_torch": t["torch"]["median_ms"] / t["fused"]["median_ms"],
                              "fused_vs_torch_graph": t["torch_graph"]["median_ms"] / t["fused_graph"]["median_ms"]}
        if kind == "l1":
            out["kinds"][kind]["fused_vs_boolean_index"] = t["boolean_index"]["median_ms"] / t["fused"]["median_ms"]
            out["kinds"][kind]["fused_full_vs_daily_l1"] = t["daily_l1"]["median_ms"] / t["fused_full"]["median_ms"]
            out["kinds"][kind]["fused_full_vs_daily_l1_graph"] = (t["daily_l1_graph"]["median_ms"]
                                                                  / t["fused_full_graph"]["median_ms"])
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-gauges", type=int, default=256)
    ap.add_argument("--train-days", type=int, default=89)
    ap.add_argument("--train-warmup", type=int, default=3)
    ap.add_argument("--eval-gauges", type=int, default=3000)
    ap.add_argument("--eval-days", type=int, default=5113)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "objective" / "objective.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("objective_time needs a HIP device")
    device = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(),
              "fused_kernel_launches": {"forward_only": 2, "forward_backward": 3},
              "train": shape_result(device, args.train_gauges, args.train_days, args.train_warmup, args.reps,
                                    args.warmup, inner=50),
              "eval": shape_result(device, args.eval_gauges, args.eval_days, 0, args.reps, args.warmup, inner=5)}
    line = json.dumps(result)
    print(line)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
