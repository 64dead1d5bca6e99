#!/usr/bin/env python
"""Time the attribute feed (ddr_amd.io.AttributeStore.batch) with HIP events at the training-batch shape (needs an
MI355X).

    python tools/attrs_time.py                                    # >= 1.0e6 reaches, A = 10, 256 gauges
    python tools/attrs_time.py --rows 100000 --gauges 32 --reps 20 --out /tmp/attrs.json

The domain and the batch are those of tools/feed_time.py: ``synthetic.forest`` with the C3 workload's log-uniform basin
sizes, the batch everything upstream of ``--gauges`` basin outlets (``UpstreamIndex.collate``), so ``db.active`` comes
in runs, as a real batch's does.  The attribute store holds the domain's reaches in another order, one in 200 missing,
2 % of its values NaN; the flowpath arrays are Lynker-style (all five), 1 % NaN; every gauge has a flow_scale factor.

Timed, each as the median / minimum / maximum of ``reps`` windows of ``inner`` calls, the candidates alternating inside
every repetition:

* ``store.batch(db.active, gage_c=db.gage_c, scale_rows=rows)`` with the aligned table's rows at 10, 12 and 16 elements
  (40 bytes packed, padded to 16 bytes, padded to 64 bytes): the layout decision of DESIGN.md section 8;
* the same with one attribute's mean NaN (the per-batch mean's two extra launches);

against two yardsticks on the same device tensors:

* (a) the best PyTorch composition: ``index_select`` of the batch's columns (attribute-major table) or rows (reach-major
  table), ``where(isnan, mean, v)``, subtract / divide, ``.T.contiguous()`` for the other layout, five ``index_select``
  + ``where`` for the flowpath arrays, and ``ones`` + an indexed assignment for flow_scale; both table layouts are timed,
  the faster one is (a);
* (b) a streaming copy of the output's bytes (``b.copy_(a)``, as tools/copy_bw.py).

Bytes are computed from shapes: a call reads A values and the index of every reach and five flowpath values, and writes
2 A + 6 values per reach.  No condition is attached to the times: they are reported.  One JSON line with the library's
build hash, also written to ``--out`` (default ``profiles/attrs/attrs.json``).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ddr_amd import _lib, synthetic  # noqa: E402
from ddr_amd.io import AttributeStore, FlowScaleTable  # noqa: E402
from ddr_amd.upstream import UpstreamIndex  # noqa: E402
from feed_time import timed_group, with_rates  # noqa: E402

PATHS = ("length", "slope", "x", "top_width", "side_slope")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000, help="least number of CONUS reaches")
    ap.add_argument("--attrs", type=int, default=10)
    ap.add_argument("--gauges", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "attrs" / "attrs.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attrs_time needs a HIP device")
    device = torch.device("cuda:0")
    A = args.attrs

    n_basins = args.gauges
    while True:
        sizes = synthetic.loguniform_sizes(n_basins, 100, 20000, 3)
        if int(sizes.sum()) >= args.rows:
            break
        n_basins += max(1, n_basins // 16)
    net = synthetic.forest(sizes, seed=3, single_inflow=0.25)
    n = net.n
    rng = np.random.default_rng(args.seed)
    outlets = np.flatnonzero(net.down < 0)
    gauges = outlets[rng.permutation(len(outlets))[: args.gauges]].tolist()
    index = UpstreamIndex(n, net.rows, net.cols, device=device)
    db = index.collate(gauges)
    active = db.active.contiguous()
    N, G = int(active.numel()), len(gauges)

    # the store holds the domain's reaches in another order, one in 200 missing
    keep = rng.random(n) >= 0.005
    store_ids = np.roll(np.flatnonzero(keep), 12345)
    attrs = (rng.standard_normal((A, len(store_ids)), dtype=np.float32) * np.float32(3.0) + np.float32(1.5))
    attrs[rng.random(attrs.shape) < 0.02] = np.nan
    means = np.nanmean(attrs, axis=1).astype(np.float32)
    stds = np.nanstd(attrs, axis=1).astype(np.float32)
    paths = {}
    for name in PATHS:
        v = rng.uniform(0.1, 100.0, n).astype(np.float32)
        v[rng.random(n) < 0.01] = np.nan
        paths[name] = v
    staid = [f"{k:08d}" for k in range(G)]
    table_fs = FlowScaleTable({"STAID": staid, "FLOW_SCALE": rng.uniform(0.2, 1.0, G).tolist()}, device=device)
    rows = table_fs.rows(staid)

    def store_of(stride, mean_values=means):
        return AttributeStore(attrs, store_ids, mean_values, stds, np.arange(n), paths["length"], paths["slope"],
                              top_width=paths["top_width"], side_slope=paths["side_slope"], x=paths["x"],
                              device=device, row_stride=stride, scale_table=table_fs)

    stores = {s: store_of(s) for s in (A, -(-A // 4) * 4, -(-A // 16) * 16)}
    nan_mean = means.copy()
    nan_mean[A // 2] = np.nan
    store_mean = store_of(-(-A // 4) * 4, nan_mean)
    default = stores[-(-A // 4) * 4]
    print(f"{default}; batch of {G} gauges, N = {N} reaches", flush=True)

    # (a) the PyTorch composition on the same device tensors
    idx = active.long()
    table_rm = default.table[:, :A].contiguous()  # reach-major (n, A)
    table_am = table_rm.T.contiguous()            # attribute-major (A, n), the reference's layout
    m, s = default.means, default.stds
    dev_paths = [default.arrays[k] for k in PATHS]
    fills = [torch.tensor(float(default.fills[k]), device=device) for k in PATHS]
    gage_c = db.gage_c.long()
    factors = table_fs.factors[rows.long()]

    def torch_rest():
        out = [torch.where(v.isnan(), f, v) for v, f in ((a.index_select(0, idx), f) for a, f in zip(dev_paths, fills))]
        fs = torch.ones(N, device=device)
        fs[gage_c] = factors
        return out, fs

    def torch_am():
        sp = table_am.index_select(1, idx)
        sp = torch.where(sp.isnan(), m[:, None], sp)
        norm = ((sp - m[:, None]) / s[:, None]).T.contiguous()
        return sp, norm, torch_rest()

    def torch_rm():
        x = table_rm.index_select(0, idx)
        x = torch.where(x.isnan(), m[None, :], x)
        return x.T.contiguous(), (x - m[None, :]) / s[None, :], torch_rest()

    def feed(store):
        return lambda: store.batch(active, gage_c=db.gage_c, scale_rows=rows)

    # the same values, at the timed size
    ab = feed(default)()
    same = {}
    for name, fn in (("am", torch_am), ("rm", torch_rm)):
        sp, norm, (out, fs) = fn()
        # (the z-score within an ulp: the library divides with correct rounding, PyTorch's kernels may not)
        same[name] = bool(torch.equal(ab.spatial_attributes.view(torch.int32), sp.view(torch.int32))
                          and torch.allclose(ab.normalized_spatial_attributes, norm, rtol=2.0 ** -22, atol=0.0)
                          and all(torch.equal(getattr(ab, k).view(torch.int32), o.view(torch.int32))
                                  for k, o in zip(PATHS, out))
                          and torch.equal(ab.flow_scale, fs))
    for stride, st in stores.items():
        other = feed(st)()
        same[f"stride_{stride}"] = bool(
            torch.equal(other.spatial_attributes.view(torch.int32), ab.spatial_attributes.view(torch.int32))
            and torch.equal(other.normalized_spatial_attributes.view(torch.int32),
                            ab.normalized_spatial_attributes.view(torch.int32)))
    if not all(same.values()):
        raise SystemExit(f"the feed and the PyTorch composition disagree: {same}")
    del ab, sp, norm, out, fs, other
    torch.cuda.empty_cache()

    out_bytes = (2 * A + 6) * N * 4
    read_bytes = (A + 1 + 5) * N * 4
    src = torch.rand(out_bytes // 4, device=device)
    dst = torch.empty_like(src)
    fns = {f"batch_stride_{k}": feed(st) for k, st in stores.items()}
    fns["batch_with_mean"] = feed(store_mean)
    fns.update(torch_attribute_major=torch_am, torch_reach_major=torch_rm, copy=lambda: dst.copy_(src))
    t = timed_group(fns, args.reps, args.warmup, args.inner)
    r = {k: with_rates(v, out_bytes if k == "copy" else read_bytes, out_bytes) for k, v in t.items()}
    for k, v in r.items():
        print(f"{k}: median {v['median_ms']:.4f} ms, min {v['min_ms']:.4f} ms, max {v['max_ms']:.4f} ms, "
              f"{(v['read_bytes'] + v['write_bytes']) / 1e9:.3f} GB -> {v['gb_per_s']:.0f} GB/s")

    key = f"batch_stride_{-(-A // 4) * 4}"
    best_torch = min(("torch_attribute_major", "torch_reach_major"), key=lambda k: r[k]["median_ms"])
    result = {"device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(),
              "conus_reaches": n, "store_reaches": len(store_ids), "attributes": A, "gauges": G, "batch_reaches": N,
              "default_row_stride": -(-A // 4) * 4, "identical_outputs": True,
              "batch_ms": r[key]["median_ms"], "torch_ms": r[best_torch]["median_ms"], "torch_best": best_torch,
              "copy_ms": r["copy"]["median_ms"],
              "batch_vs_torch": r[best_torch]["median_ms"] / r[key]["median_ms"],
              "batch_vs_copy": r[key]["median_ms"] / r["copy"]["median_ms"], "timings": r}
    line = json.dumps(result)
    print(line)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
