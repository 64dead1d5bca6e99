#!/usr/bin/env python
"""Time ddr_amd.upstream.UpstreamIndex with HIP events at a training-batch-shaped size (needs an MI355X).

    python tools/upstream_time.py                                 # 8e5 reaches, 256 gauges
    python tools/upstream_time.py --rows 100000 --gauges 64 --reps 20

The network is ``synthetic.forest`` with Zipf basin sizes; the gauges are every basin's outlet plus random interior
reaches, so their closures nest.  Timed, each as the median / minimum / maximum of ``reps`` calls:

* ``index.collate(gauges)`` -- label, closure COO, device union;
* ``collate_gauges_device`` on the same batch's precomputed per-gauge subsets (what the engine's ``gages_adjacency``
  store holds), already on the device, and from host arrays (upload included);
* ``index.members_device(gauges)``;
* the index build, from a host COO and from a device COO.

The acceptance figure: the median of ``index.collate`` against the median of ``collate_gauges_device`` on uploaded
subsets plus that path's own min-to-max spread.  One JSON line with the library's build hash, also written to
``--out`` (default ``profiles/upstream/collate.json``).
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ddr_amd import _lib, synthetic  # noqa: E402
from ddr_amd.batching import collate_gauges_device  # noqa: E402
from ddr_amd.upstream import UpstreamIndex  # noqa: E402


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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=800_000)
    ap.add_argument("--basins", type=int, default=100)
    ap.add_argument("--gauges", type=int, default=256)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "upstream" / "collate.json"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("upstream_time needs a HIP device")
    device = torch.device("cuda:0")
    net = synthetic.forest(synthetic.zipf_sizes(args.rows, args.basins, 0.375), seed=args.seed)
    down = net.down
    rng = np.random.default_rng(args.seed)
    outlets = np.flatnonzero(down < 0)
    if len(outlets) >= args.gauges:
        gauges = outlets[: args.gauges]
    else:
        interior = rng.choice(np.flatnonzero(down >= 0), size=args.gauges - len(outlets), replace=False)
        gauges = np.concatenate([outlets, interior])
    gauges = gauges[rng.permutation(len(gauges))].tolist()

    subsets = UpstreamIndex(net.n, net.rows, net.cols).subsets(gauges)  # (the host twin: what the engine would store)
    edges_shipped = int(sum(len(r) for r, _, _ in subsets))
    subsets_dev = [(torch.from_numpy(r).to(device), torch.from_numpy(c).to(device), g) for r, c, g in subsets]
    rows_dev, cols_dev = torch.from_numpy(net.rows).to(device), torch.from_numpy(net.cols).to(device)

    index = UpstreamIndex(net.n, net.rows, net.cols, device=device)
    new = index.collate(gauges)
    old = collate_gauges_device(net.n, subsets_dev, device)
    same = all(torch.equal(getattr(new, k), getattr(old, k))
               for k in ("active", "rows", "cols", "crow", "col", "out_off", "out_idx", "gage_c"))
    if not same:
        raise SystemExit("index.collate and collate_gauges_device disagree")
    off, idx = index.members_device(gauges)
    print(f"{index}: {len(gauges)} gauges, union of {new.n} reaches / {int(new.cols.numel())} edges; the subsets hold "
          f"{edges_shipped} edges; {int(idx.numel())} members", flush=True)

    r = {
        "index_collate": timed(lambda: index.collate(gauges), args.reps, args.warmup),
        "collate_gauges_device_uploaded_subsets": timed(lambda: collate_gauges_device(net.n, subsets_dev, device),
                                                        args.reps, args.warmup),
        "collate_gauges_device_host_subsets": timed(lambda: collate_gauges_device(net.n, subsets, device), args.reps,
                                                    args.warmup),
        "members": timed(lambda: index.members_device(gauges), args.reps, args.warmup),
        "index_build_host_coo": timed(lambda: UpstreamIndex(net.n, net.rows, net.cols, device=device), args.reps,
                                      args.warmup),
        "index_build_device_coo": timed(lambda: UpstreamIndex(net.n, rows_dev, cols_dev, device=device), args.reps,
                                        args.warmup),
    }
    for k, v in r.items():
        print(f"{k}: median {v['median_ms']:.3f} ms, min {v['min_ms']:.3f} ms, max {v['max_ms']:.3f} ms")
    old_t, new_t = r["collate_gauges_device_uploaded_subsets"], r["index_collate"]
    bar = old_t["median_ms"] + (old_t["max_ms"] - old_t["min_ms"])
    result = {"device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(), "rows": net.n,
              "gauges": len(gauges), "outlets": int(index.n_outlets), "max_depth": index.max_depth,
              "rounds": index.rounds, "union_reaches": new.n, "union_edges": int(new.cols.numel()),
              "subset_edges": edges_shipped, "members": int(idx.numel()), "identical_outputs": same,
              "bar_ms": bar, "within_bar": new_t["median_ms"] <= bar, "timings": r}
    line = json.dumps(result)
    print(line)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
