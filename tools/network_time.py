#!/usr/bin/env python
"""Time the network build (ddr_amd.network.Network.build) at the C5 shape (needs an MI355X).

    python tools/network_time.py
    python tools/network_time.py --reps 5 --out /tmp/network.json

The table is ``synthetic.forest(zipf_sizes(800_000, 3000, 0.35), seed=5, single_inflow=0.35)`` with its rows shuffled
and ids spread above 32 bits.  Three builders of the same network from it:

* the device build, from device tensors (the build is synchronous: wall clock around the call);
* the host twin (``device=None``);
* ``networkx.lexicographical_topological_sort`` plus renumbering, the stand-in for the engine's rustworkx path
  (``merit/build.py:20-107``), which needs rustworkx and polars.  Its order differs from ours; its result is checked
  to be a valid contract network of the same edges.

Each is the median / minimum / maximum of ``reps`` windows after ``warmup`` calls, the builders alternating inside
every repetition.  No condition is attached to the times: they are reported.  One JSON line with the library's build
hash, also written to ``--out`` (default ``profiles/network/network.json``).
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ddr_amd import _lib, synthetic  # noqa: E402
from ddr_amd.network import Network  # noqa: E402


def shuffled_table(down: np.ndarray, seed: int):
    n = len(down)
    rng = np.random.default_rng(seed)
    reach_id = rng.permutation(n).astype(np.int64) * 7919 + (1 << 33)
    reach_to = np.where(down >= 0, reach_id[np.maximum(down, 0)], 0)
    reach_of_row = rng.permutation(n)
    return reach_id[reach_of_row], reach_to[reach_of_row]


def networkx_build(ids: np.ndarray, to: np.ndarray):
    """Topological sort and renumbering with networkx: (order ids, rows, cols)."""
    import networkx as nx

    g = nx.DiGraph()
    g.add_nodes_from(ids.tolist())
    known = set(ids.tolist())
    g.add_edges_from((a, b) for a, b in zip(ids.tolist(), to.tolist()) if b in known)
    order = list(nx.lexicographical_topological_sort(g))
    new_of = {v: k for k, v in enumerate(order)}
    cols = np.fromiter((new_of[a] for a, _ in g.edges()), np.int64, g.number_of_edges())
    rows = np.fromiter((new_of[b] for _, b in g.edges()), np.int64, g.number_of_edges())
    return np.asarray(order, np.int64), rows, cols


def timed(fns: dict, reps: dict, warmup: dict) -> dict:
    for k, fn in fns.items():
        for _ in range(warmup[k]):
            fn()
    ms = {k: [] for k in fns}
    for r in range(max(reps.values())):
        for k, fn in fns.items():
            if r >= reps[k]:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": len(v)}
            for k, v in ms.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reaches", type=int, default=800_000)
    ap.add_argument("--basins", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--networkx-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "network" / "network.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("network_time needs a HIP device")
    device = torch.device("cuda:0")
    net = synthetic.forest(synthetic.zipf_sizes(args.reaches, args.basins, 0.35), seed=5, single_inflow=0.35)
    ids, to = shuffled_table(net.down, 5)
    d_ids, d_to = torch.from_numpy(ids).to(device), torch.from_numpy(to).to(device)

    dev, host = Network.build(d_ids, d_to), Network.build(ids, to)
    for k in ("position", "ids", "down", "rows", "cols", "dropped"):
        if not np.array_equal(getattr(dev, k).cpu().numpy(), getattr(host, k)):
            raise SystemExit(f"the device build and the host twin disagree on {k}")
    order, rows, cols = networkx_build(ids, to)
    same_edges = (set(zip(order[cols].tolist(), order[rows].tolist()))
                  == set(zip(host.ids[host.cols].tolist(), host.ids[host.rows].tolist())))
    if not (same_edges and np.all(rows > cols) and len(order) == host.n):
        raise SystemExit("the networkx build is not the same network")

    t = timed({"device": lambda: Network.build(d_ids, d_to), "host": lambda: Network.build(ids, to),
               "networkx": lambda: networkx_build(ids, to)},
              {"device": args.reps, "host": args.host_reps, "networkx": args.networkx_reps},
              {"device": args.warmup, "host": 1, "networkx": 0})
    for k, r in t.items():
        print(f"{k}: median {r['median_ms']:.3f} ms, min {r['min_ms']:.3f} ms, max {r['max_ms']:.3f} ms ({r['reps']})")
    result = {"device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(),
              "rows": int(len(ids)), "reaches": host.n, "edges": host.nnz, "basins": host.n_basins,
              "max_depth": host.max_depth, "device_ms": t["device"]["median_ms"], "host_ms": t["host"]["median_ms"],
              "networkx_ms": t["networkx"]["median_ms"], "identical_outputs": True, "timings": t}
    line = json.dumps(result)
    print(line)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
