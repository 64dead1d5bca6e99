#!/usr/bin/env python
"""Time the forcing feed (ddr_amd.io) with HIP events at the training-batch shape (needs an MI355X).

    python tools/feed_time.py                                     # >= 1.0e6 rows x 5000 days (>= 20 GB), 256 gauges
    python tools/feed_time.py --rows 100000 --days 400 --gauges 32 --reps 20 --out /tmp/feed.json

The domain is ``synthetic.forest`` with the C3 workload's log-uniform basin sizes, as many basins as reach ``--rows``
reaches; the batch is everything upstream of ``--gauges`` basin outlets (``UpstreamIndex.collate``), so its store rows
come in runs, as a real batch's do, and are looked up on the device (``aligned[db.active]``).  One divide in 200 is
missing from the store.  The q' store is seeded log-normal, generated on the device; rho = 90.

Timed, each as the median / minimum / maximum of ``reps`` windows of ``inner`` calls, the candidates of a group
alternating inside every repetition:

* ``flow.daily(rows, d0, rho - 1)`` -- the (89, N) input of ``ops.route(..., qprime_hours=24)``;
* ``flow.hourly(rows, d0, T)`` -- the (T, N) tensor of the drop-in call, expanded in the kernel (T = (rho - 1) * 24);
* ``flow(routing_dataclass=...)`` -- the drop-in call itself: the same kernel after the host id lookup and its upload;
* ``obs.window(rows, d0, rho)`` for the batch's gauges;

against two yardsticks on the same device tensors:

* (a) the best PyTorch composition, ``torch.where((rows >= 0)[None], qr[:, t0:t1].index_select(0,
  rows.clamp_min(0)).T.contiguous(), 0.001)`` (and ``.repeat_interleave(24, 0)[:T]`` for the hourly form);
* (b) a streaming copy of the output's bytes (``b.copy_(a)``, as tools/copy_bw.py).

Bytes are computed from shapes: a feed call reads the window of every valid row and the row indices and writes the
output and the mask; the copy reads and writes the output's bytes.  The condition: the medians of ``daily`` and
``hourly`` are not above those of (a).  The ratio to (b) is reported.  One JSON line with the library's build hash,
also written to ``--out`` (default ``profiles/feed/feed.json``).
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ddr_amd import _lib, synthetic  # noqa: E402
from ddr_amd.io import ObservationStore, StreamflowStore  # noqa: E402
from ddr_amd.upstream import UpstreamIndex  # noqa: E402


def lognormal_store(n: int, T: int, device, seed: int) -> torch.Tensor:
    gen = torch.Generator(device=device).manual_seed(seed)
    qr = torch.empty((n, T), device=device, dtype=torch.float32)
    scale = torch.empty((n, 1), device=device).log_normal_(float(np.log(0.5)), 1.0, generator=gen)
    for s in range(0, n, 65536):
        qr[s:s + 65536].log_normal_(0.0, 0.5, generator=gen).mul_(scale[s:s + 65536])
    return qr


def timed_group(fns: dict, reps: int, warmup: int, inner: int) -> dict:
    """Every function of ``fns`` timed ``reps`` times in windows of ``inner`` calls, one after the other inside each
    repetition (so that a drift of the machine touches all of them alike)."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": reps, "inner": inner}
            for k, v in ms.items()}


def with_rates(t: dict, read: int, write: int) -> dict:
    t = dict(t, read_bytes=int(read), write_bytes=int(write))
    t["gb_per_s"] = (read + write) / (t["median_ms"] * 1e-3) / 1e9
    return t


def dates_of(first_day: int, rho: int) -> SimpleNamespace:
    day0 = np.datetime64("1980-01-01", "D") + first_day
    return SimpleNamespace(numerical_time_range=np.arange(first_day, first_day + rho),
                           batch_hourly_time_range=day0.astype("datetime64[h]") + np.arange((rho - 1) * 24))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000, help="least number of store rows")
    ap.add_argument("--days", type=int, default=5000)
    ap.add_argument("--gauges", type=int, default=256)
    ap.add_argument("--rho", type=int, default=90)
    ap.add_argument("--day0", type=int, default=2001, help="first day of the batch's window")
    ap.add_argument("--obs-gauges", type=int, default=3000, help="rows of the observation store")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "feed" / "feed.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feed_time needs a HIP device")
    device = torch.device("cuda:0")
    rho, d0 = args.rho, args.day0
    T = (rho - 1) * 24

    n_basins = args.gauges
    while True:
        sizes = synthetic.loguniform_sizes(n_basins, 100, 20000, 3)
        if int(sizes.sum()) >= args.rows:
            break
        n_basins += max(1, n_basins // 16)
    net = synthetic.forest(sizes, seed=3, single_inflow=0.25)
    rng = np.random.default_rng(args.seed)
    outlets = np.flatnonzero(net.down < 0)
    gauges = outlets[rng.permutation(len(outlets))[: args.gauges]].tolist()
    index = UpstreamIndex(net.n, net.rows, net.cols, device=device)
    db = index.collate(gauges)

    # the store holds the domain's divides in another order, one in 200 missing
    keep = rng.random(net.n) >= 0.005
    store_ids = np.roll(np.flatnonzero(keep), 12345)
    qr = lognormal_store(len(store_ids), args.days, device, args.seed)
    flow = StreamflowStore(qr, store_ids, start="1980/01/01", is_hourly=False)
    aligned = flow.align(np.arange(net.n))
    rows = aligned[db.active.long()].contiguous()
    N = int(rows.numel())
    n_valid = int((rows >= 0).sum())
    batch = SimpleNamespace(divide_ids=db.active.cpu().numpy(), dates=dates_of(d0, rho))
    print(f"{flow}: {qr.numel() * 4 / 1e9:.1f} GB; batch of {len(gauges)} gauges, N = {N} reaches "
          f"({N - n_valid} not in the store), rho = {rho}, T = {T}", flush=True)

    obs_np = np.random.default_rng(args.seed + 1).lognormal(1.0, 1.0, (args.obs_gauges, args.days)).astype(np.float32)
    obs_np[np.random.default_rng(args.seed + 2).random(obs_np.shape) < 1e-3] = np.nan
    obs = ObservationStore(obs_np, np.arange(args.obs_gauges) + 1_000_000, device=device)
    g_rows = obs.rows(rng.choice(args.obs_gauges, size=min(args.gauges, args.obs_gauges), replace=False) + 1_000_000)
    G = int(g_rows.numel())

    rows64 = rows.clamp_min(0).long()
    mask = (rows >= 0)[None]

    def torch_daily():
        return torch.where(mask, qr[:, d0:d0 + rho - 1].index_select(0, rows64).T.contiguous(), 0.001)

    def torch_hourly():
        sel = qr[:, d0:d0 + rho - 1].index_select(0, rows64).T.contiguous()
        return torch.where(mask, sel.repeat_interleave(24, 0)[:T], 0.001)

    # the same values, at the timed size
    same_daily = torch.equal(flow.daily(rows, d0, rho - 1)[0].view(torch.int32), torch_daily().view(torch.int32))
    same_hourly = torch.equal(flow.hourly(rows, d0, T)[0].view(torch.int32), torch_hourly().view(torch.int32))
    same_dropin = torch.equal(flow(routing_dataclass=batch), flow.hourly(rows, d0, T)[0])
    if not (same_daily and same_hourly and same_dropin):
        raise SystemExit(f"the feed and the PyTorch composition disagree: daily {same_daily}, hourly {same_hourly}, "
                         f"drop-in {same_dropin}")
    torch.cuda.empty_cache()

    src_d = torch.rand((rho - 1, N), device=device)
    dst_d = torch.empty_like(src_d)
    src_h = torch.rand((T, N), device=device)
    dst_h = torch.empty_like(src_h)
    window_bytes = n_valid * (rho - 1) * 4 + N * 4
    r = {}
    t = timed_group({"daily": lambda: flow.daily(rows, d0, rho - 1), "torch_daily": torch_daily,
                     "copy_daily": lambda: dst_d.copy_(src_d)}, args.reps, args.warmup, inner=20)
    out_d = (rho - 1) * N * 4
    r["daily"] = with_rates(t["daily"], window_bytes, out_d + N)
    r["torch_daily"] = with_rates(t["torch_daily"], window_bytes, out_d)  # (its algorithmic bytes, not its traffic)
    r["copy_daily"] = with_rates(t["copy_daily"], out_d, out_d)
    t = timed_group({"hourly": lambda: flow.hourly(rows, d0, T), "torch_hourly": torch_hourly,
                     "copy_hourly": lambda: dst_h.copy_(src_h),
                     "dropin_call": lambda: flow(routing_dataclass=batch, device=device, dtype=torch.float32)},
                    args.reps, args.warmup, inner=2)
    out_h = T * N * 4
    r["hourly"] = with_rates(t["hourly"], window_bytes, out_h + N)
    r["torch_hourly"] = with_rates(t["torch_hourly"], window_bytes, out_h)
    r["copy_hourly"] = with_rates(t["copy_hourly"], out_h, out_h)
    r["dropin_call"] = with_rates(t["dropin_call"], window_bytes, out_h + N)
    t = timed_group({"obs_window": lambda: obs.window(g_rows, d0, rho)}, args.reps, args.warmup, inner=50)
    r["obs_window"] = with_rates(t["obs_window"], G * rho * 4 + G * 4, G * (rho - 2) * 4 + G)
    for k, v in r.items():
        print(f"{k}: median {v['median_ms']:.4f} ms, min {v['min_ms']:.4f} ms, max {v['max_ms']:.4f} ms, "
              f"{(v['read_bytes'] + v['write_bytes']) / 1e9:.3f} GB -> {v['gb_per_s']:.0f} GB/s")

    ok_d = r["daily"]["median_ms"] <= r["torch_daily"]["median_ms"]
    ok_h = r["hourly"]["median_ms"] <= r["torch_hourly"]["median_ms"]
    result = {"device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(),
              "store_rows": len(store_ids), "store_days": args.days, "store_bytes": qr.numel() * 4,
              "gauges": len(gauges), "batch_reaches": N, "batch_reaches_in_store": n_valid, "rho": rho, "T": T,
              "obs_gauges": G, "identical_outputs": True,
              "daily_vs_torch": r["torch_daily"]["median_ms"] / r["daily"]["median_ms"],
              "hourly_vs_torch": r["torch_hourly"]["median_ms"] / r["hourly"]["median_ms"],
              "daily_vs_copy": r["daily"]["median_ms"] / r["copy_daily"]["median_ms"],
              "hourly_vs_copy": r["hourly"]["median_ms"] / r["copy_hourly"]["median_ms"],
              "not_slower_than_torch": bool(ok_d and ok_h), "timings": r}
    line = json.dumps(result)
    print(line)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")
    if not (ok_d and ok_h):
        raise SystemExit("the feed is slower than the PyTorch composition: a defect of the kernel")


if __name__ == "__main__":
    main()
