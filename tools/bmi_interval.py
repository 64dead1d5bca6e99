#!/usr/bin/env python
"""Wall time of one ngen coupling interval through the BMI coupling (needs an MI355X).

    python tools/bmi_interval.py                       # the 800k-reach network of bench.py's drop-in leg
    python tools/bmi_interval.py --reaches 50000 --basins 200 --out /tmp/interval.json

Every segment has one nexus and ngen sends all of them, in a shuffled order.  For K = 1 (a 3600 s routing step) and
K = 12 (300 s, linear interpolation) sub-steps per 3600 s interval the script times, per interval,

  (a) ``DdrBmi.set_value`` of the flows + ``update_until``: one upload and gather, then the window, ONE routing
      launch, the output kernel and one copy into the pinned arrays;
  (b) the same work done the reference's way (``src/ddr/bmi/ddr_bmi.py:246-318, 417-438, 577-630``) on this
      package's ``MuskingumCunge``: the Python loop over the nexus ids with a dict lookup each, and per sub-step a
      host interpolation, a ``torch.tensor`` upload, a clamp and one ``route_timestep``; then
      ``compute_trapezoidal_geometry`` and three ``.cpu()`` copies.

Both are host wall time around work that ends in a device synchronise: the mean of ``--intervals`` intervals after
``--warmup`` warm-ups (the cold start is in the warm-up).  The routing share of (a) is measured on its own: one
``ops.route`` launch over a (K + 1)-row window from a carried state, HIP events, the same count.  Both paths get
the same flows, so their final discharge is compared as well.  One JSON document, written to ``--out``.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ddr_amd import _lib, synthetic  # noqa: E402
from ddr_amd.bmi import DdrBmi  # noqa: E402
from ddr_amd.geometry.trapezoidal import compute_trapezoidal_geometry  # noqa: E402
from ddr_amd.ops import route  # noqa: E402
from ddr_amd.routing.mmc import MuskingumCunge, compute_hotstart_discharge  # noqa: E402

FLOW = "land_surface_water_source__volume_flow_rate"
PARAMS = dict(parameter_ranges={"n": [0.015, 0.25], "q_spatial": [0.0, 1.0], "p_spatial": [1.0, 200.0]},
              log_space_parameters=["p_spatial"], defaults={"p_spatial": 21},
              attribute_minimums={"discharge": 1e-4, "slope": 1e-3, "velocity": 0.01, "depth": 0.01,
                                  "bottom_width": 0.01})
COUPLING = 3600.0


class ReferenceWay:
    """The reference's set_value / update_until / _update_output_cache, line for line in structure, on the device
    engine of this package."""

    def __init__(self, dc, spatial, cfg, mapping, N, dt, interpolation, dev):
        self.mc = MuskingumCunge(cfg, device=dev)
        self.mc.t = torch.tensor(dt, device=dev)
        self.mc.setup_inputs(routing_dataclass=dc, streamflow=torch.zeros(1, N, device=dev),
                             spatial_parameters=spatial)
        self.mapper, _, _ = self.mc.create_pattern_mapper()
        self.mapping, self.dev, self.dt, self.interpolation = mapping, dev, dt, interpolation
        self.lateral, self.prev = np.zeros(N), np.zeros(N)
        self.has_prev = self.cold = False
        self.now = 0.0
        self.ids = np.empty(0, np.int32)
        self.discharge, self.velocity, self.depth = (np.zeros(N, np.float32) for _ in range(3))
        self.lb = float(cfg.params.attribute_minimums["discharge"])

    def set_flows(self, src):
        flows = src.flat[:len(self.ids)]
        for i, nex_id in enumerate(self.ids):
            seg = self.mapping.get(int(nex_id))
            if seg is not None:
                self.lateral[seg] = flows[i]

    def update_until(self, until):
        mc = self.mc
        n_steps = max(1, round((until - self.now) / self.dt))
        linear = self.interpolation == "linear" and self.has_prev and n_steps > 1
        for step in range(n_steps):
            if linear:
                alpha = (step + 1) / n_steps
                inflow = (1.0 - alpha) * self.prev + alpha * self.lateral
            else:
                inflow = self.lateral
            q_prime = torch.tensor(inflow, dtype=torch.float32, device=self.dev)
            if not self.cold:
                mc._discharge_t = compute_hotstart_discharge(q_prime, self.mapper, mc.discharge_lb, self.dev)
                self.cold = True
            with torch.no_grad():
                mc._discharge_t = mc.route_timestep(q_prime_clamp=torch.clamp(q_prime, min=self.lb),
                                                    mapper=self.mapper)
            self.now += self.dt
        with torch.no_grad():
            geo = compute_trapezoidal_geometry(mc.n, mc.p_spatial, mc.q_spatial, mc._discharge_t, mc.slope,
                                               depth_lb=float(mc.depth_lb), bottom_width_lb=float(mc.bottom_width_lb))
            v = torch.clamp(geo["velocity"], min=0.0, max=15.0)
        self.discharge[:] = mc._discharge_t.detach().cpu().numpy()
        self.velocity[:] = v.cpu().numpy()
        self.depth[:] = geo["depth"].cpu().numpy()
        self.prev[:] = self.lateral
        self.has_prev = True
        self.lateral[:] = 0.0


def wall(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reaches", type=int, default=800_000)
    ap.add_argument("--basins", type=int, default=3000)
    ap.add_argument("--largest", type=float, default=0.35)
    ap.add_argument("--intervals", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "bmi" / "interval.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bmi_interval needs a HIP device")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize

    net = synthetic.forest(synthetic.zipf_sizes(args.reaches, args.basins, args.largest), seed=5, single_inflow=0.35)
    N = net.n
    at = synthetic.reach_attributes(N, 11)
    u = synthetic.unit_parameters(N, 11)
    a = sp.coo_matrix((np.ones(len(net.rows), np.float32), (net.rows, net.cols)), shape=(N, N)).tocsr()
    adj = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)),
                                  torch.from_numpy(a.indices.astype(np.int64)), torch.from_numpy(a.data), size=(N, N))
    dc = SimpleNamespace(adjacency_matrix=adj, length=torch.from_numpy(at.length), slope=torch.from_numpy(at.slope),
                         x=torch.from_numpy(at.x), top_width=torch.empty(0), side_slope=torch.empty(0),
                         outflow_idx=None, gage_catchment=None, observations=None, flow_scale=None)
    cfg = SimpleNamespace(params=SimpleNamespace(**PARAMS))
    spatial = {k: torch.from_numpy(v).to(dev) for k, v in u.items()}
    rng = np.random.default_rng(0)
    mapping = {10_000_000 + int(s): int(s) for s in range(N)}
    ids = (10_000_000 + rng.permutation(N)).astype(np.int32)
    total = args.warmup + args.intervals
    flows = rng.lognormal(np.log(0.05), 1.0, (4, N))  # cycled: successive intervals differ
    print(f"{N} segments, {len(ids)} nexus ids, {args.intervals} timed intervals after {args.warmup} warm-ups",
          flush=True)

    rows = []
    for K, interpolation in ((1, "constant"), (12, "linear")):
        dt = COUPLING / K
        b = DdrBmi()
        b.initialize_from(dc, spatial, cfg, nexus_to_segment=mapping, timestep_seconds=dt,
                          interpolation=interpolation, device=dev)
        b.set_value("land_surface_water_source__id", ids)
        ref = ReferenceWay(dc, spatial, cfg, mapping, N, dt, interpolation, dev)
        ref.ids = ids
        t = {k: [] for k in ("a_set_value", "a_update_until", "b_set_value", "b_update_until")}
        for i in range(total):  # the two paths alternate, interval by interval
            f, until = flows[i % 4], COUPLING * (i + 1)
            ms = (wall(lambda: b.set_value(FLOW, f), sync), wall(lambda: b.update_until(until), sync),
                  wall(lambda: ref.set_flows(f), sync), wall(lambda: ref.update_until(until), sync))
            if i >= args.warmup:
                for k, v in zip(t, ms):
                    t[k].append(v)
        assert b.route_launches == total
        same = bool(np.array_equal(b.get_value_ptr("channel_exit_water_x-section__volume_flow_rate"), ref.discharge))
        # the routing share of (a): one launch over a (K + 1)-row window from the carried state
        mc = b._mc
        window = torch.from_numpy(np.maximum(flows[0], 1e-4).astype(np.float32)).to(dev).repeat(K + 1, 1)
        ev = []
        with torch.no_grad():
            for i in range(total):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                route(mc._graph, window, mc.n, mc.q_spatial, b._p, mc.length, mc.slope, mc.x_storage,
                      q0=mc._discharge_t, consts=b._consts, math=mc.math)
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    ev.append(e0.elapsed_time(e1))
        mean = {k: float(np.mean(v)) for k, v in t.items()}
        row = {"K": K, "timestep_seconds": dt, "interpolation": interpolation,
               "a_ddrbmi_ms": mean["a_set_value"] + mean["a_update_until"],
               "b_reference_way_ms": mean["b_set_value"] + mean["b_update_until"], **mean,
               "routing_math": mc.math, "a_route_window_launch_ms": float(np.mean(ev)),
               "a_min_ms": float(np.min(np.add(t["a_set_value"], t["a_update_until"]))),
               "b_min_ms": float(np.min(np.add(t["b_set_value"], t["b_update_until"]))),
               "final_discharge_bitwise_equal": same}
        rows.append(row)
        print(json.dumps(row), flush=True)
        b.finalize()
        del b, ref
        torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(), "segments": N,
           "nexus_ids": int(len(ids)), "intervals": args.intervals, "warmup": args.warmup,
           "what": "host wall time per 3600 s coupling interval, synchronised, mean; (a) DdrBmi set_value + "
                   "update_until, (b) the reference's loop structure on MuskingumCunge.route_timestep",
           "rows": rows}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
