#!/usr/bin/env python
"""Time whole-period inference (ddr_amd.inference.PeriodRouter) with HIP events at the C4 shape (needs an MI355X).

    python tools/period_time.py                                       # 350k reaches, 366 days, 30-day chunks
    python tools/period_time.py --reaches 20000 --basins 60 --days 40 --chunk-days 7 --reps 3 --out /tmp/p.json

The network is the C4 workload's (``synthetic.forest(zipf_sizes(350_000, 1000, 0.35), seed=4)``, x = 0.3), the forcing a
daily store ``(days, N)`` generated on the device, the modes every reach and ``--gauges`` single-reach gauges at basin
outlets.

Timed per mode, alternating inside every repetition, each a whole period ending in a device synchronise:

* (a) ``PeriodRouter.run``: per chunk one forward without runoff output and one daily accumulation;
* (b) the composition the library offered before: ``route()`` per chunk with hourly ``(R, T)`` output and ``q0``
  carried, ``torch.cat``, the ``[13 + tau : -11 + tau]`` slice and ``F.interpolate(mode="area")`` on the device.

Both read the same daily store (``qprime_hours=24``).  The peak device memory of each (``max_memory_allocated`` above
what was allocated before the call) is recorded, and the two daily series are compared at the timed size.

The daily accumulation alone, on the saved states of one full chunk placed at the second chunk's hour (so it meets
``chunk_days + 1`` windows, two of them partial): the all-reach kernel in both store variants -- the LDS tile written
as per-row runs of days, and one thread per (reach, day) storing its own value -- the gauge kernel, and a streaming
copy of the bytes the all-reach kernel reads (``b.copy_(a)`` of a ``(T, N)`` array, as tools/copy_bw.py: it reads and
writes those bytes, the kernel reads them and writes ``N * (chunk_days + 1)`` values).

The condition: (a)'s median is not above (b)'s by more than (b)'s spread (max - min), and (a)'s peak memory is below
(b)'s.  One JSON line with the library's build hash, also written to ``--out`` (default ``profiles/period/period.json``).
"""

from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ddr_amd import _lib, synthetic  # noqa: E402
from ddr_amd.graph import RiverGraph  # noqa: E402
from ddr_amd.inference import PeriodRouter, period_chunks  # noqa: E402
from ddr_amd.ops import GaugeMap, RouteConsts, mc_route, register_graph, route  # noqa: E402


def summary(v: list[float]) -> dict:
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": len(v)}


def timed_alternating(fns: dict, reps: int, warmup: int, inner: int = 1) -> dict:
    """Every function timed ``reps`` times in windows of ``inner`` calls, one after the other inside each repetition."""
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
    return {k: dict(summary(v), inner=inner) for k, v in ms.items()}


def peak_bytes(fn) -> int:
    """Peak device memory of one call above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    torch.cuda.empty_cache()
    return int(peak)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reaches", type=int, default=350_000)
    ap.add_argument("--basins", type=int, default=1000)
    ap.add_argument("--days", type=int, default=366)
    ap.add_argument("--chunk-days", type=int, default=30)
    ap.add_argument("--gauges", type=int, default=256)
    ap.add_argument("--tau", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "period" / "period.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("period_time needs a HIP device")
    dev = torch.device("cuda:0")
    n_days, B, tau = args.days, args.chunk_days, args.tau

    net = synthetic.forest(synthetic.zipf_sizes(args.reaches, args.basins, 0.35), seed=4, single_inflow=0.15)
    N = net.n
    at = synthetic.reach_attributes(N, 4, x_const=0.3)
    u = synthetic.unit_parameters(N, 4)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
    n = tt(0.015 + (0.25 - 0.015) * u["n"])
    q = tt(u["q_spatial"])
    p = tt(np.exp(np.log(1.0) + (np.log(200.0) - np.log(1.0)) * u["p_spatial"]))
    length, slope, x = tt(at.length), tt(np.maximum(at.slope, np.float32(1e-3))), tt(at.x)
    store = synthetic.lateral_inflow_torch(N, n_days, seed=4, device=dev)  # (days, N): a row per day
    assert store.shape == (n_days, N)
    outlets = np.flatnonzero(net.down < 0)
    pick = outlets[np.random.default_rng(0).permutation(len(outlets))[:args.gauges]]
    gauges = GaugeMap.build([np.array([o]) for o in pick], N, dev)
    g = RiverGraph(N, net.rows, net.cols)
    consts = RouteConsts()
    chunks = period_chunks(n_days, B)
    H, D = (n_days - 1) * 24, n_days - 2
    print(f"N = {N} reaches, {n_days} days in {len(chunks)} chunks of {B} days, {gauges.n_gauges} gauges, "
          f"{g.info.n_blocks} blocks", flush=True)

    def fused(gz):
        return PeriodRouter(g, length, slope, x, gauges=gz, consts=consts, tau=tau, chunk_days=B).run(
            n, q, p, store, n_days).daily

    @torch.no_grad()
    def composed(gz):
        parts, q0 = [], None
        for first, last in chunks:
            runoff, q0, _, _ = route(g, store[first:last + 1], n, q, p, length, slope, x, q0=q0, gauges=gz,
                                     consts=consts, steps=(last - first) * 24, qprime_hours=24)
            parts.append(runoff)
        hourly = torch.cat(parts, dim=1)
        del parts
        sl = hourly[:, 13 + tau:H - 11 + tau]
        return torch.nn.functional.interpolate(sl.unsqueeze(1), size=(D,), mode="area").squeeze(1)

    result = {"device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(), "reaches": N,
              "days": n_days, "chunk_days": B, "chunks": len(chunks), "tau": tau, "gauges": gauges.n_gauges,
              "blocks": g.info.n_blocks, "modes": {}}
    ok = True
    for mode, gz in (("all", None), ("gauge", gauges)):
        a, b = fused(gz), composed(gz)
        err = float(((a.double() - b.double()).abs() / b.double().abs()).max())
        del a, b
        mem = {"period_router": peak_bytes(lambda: fused(gz)), "composed": peak_bytes(lambda: composed(gz))}
        t = timed_alternating({"period_router": lambda: fused(gz), "composed": lambda: composed(gz)}, args.reps,
                              args.warmup)
        spread = t["composed"]["max_ms"] - t["composed"]["min_ms"]
        not_slower = t["period_router"]["median_ms"] <= t["composed"]["median_ms"] + spread
        less_memory = mem["period_router"] < mem["composed"]
        ok = ok and not_slower and less_memory and err <= 1e-6
        result["modes"][mode] = {
            "timings": t, "peak_bytes": mem, "max_rel_difference": err,
            "speedup": t["composed"]["median_ms"] / t["period_router"]["median_ms"],
            "memory_ratio": mem["composed"] / max(mem["period_router"], 1), "not_slower": bool(not_slower),
            "less_memory": bool(less_memory)}
        print(f"{mode}: PeriodRouter {t['period_router']['median_ms']:.1f} ms "
              f"[{t['period_router']['min_ms']:.1f}, {t['period_router']['max_ms']:.1f}], composed "
              f"{t['composed']['median_ms']:.1f} ms [{t['composed']['min_ms']:.1f}, {t['composed']['max_ms']:.1f}]; "
              f"peak {mem['period_router'] / 1e9:.2f} GB vs {mem['composed'] / 1e9:.2f} GB; max-rel {err:.2e}",
              flush=True)

    # ---- the daily accumulation alone, on one full chunk's saved states ----------------------------------------
    first, last = chunks[1] if len(chunks) > 1 else chunks[0]
    T = (last - first) * 24
    lib = _lib.load()
    stream = _lib.stream_ptr(dev)
    with torch.no_grad():
        out = mc_route(store[first:last + 1].contiguous(), n, q, p.reshape(-1), length, slope, x, None, None,
                       gauges.offsets, gauges.index, None, None, None, register_graph(g), consts.as_list(),
                       _lib.DDR_FWD_SAVE_X, T, 24, [])
    x_save = out[4]
    del out
    gzc = _lib.Gauges(gauges.n_gauges, gauges.offsets.data_ptr(), gauges.index.data_ptr(), None, None)
    d_all = torch.zeros((N, D), device=dev)
    d_gauge = torch.zeros((gauges.n_gauges, D), device=dev)
    src = torch.rand((T, N), device=dev)
    dst = torch.empty_like(src)

    def daily(buf, gref, flags):
        _lib.check(lib.ddr_period_daily_f32(g.handle, x_save.data_ptr(), T, gref, consts.discharge_lb, flags, first * 24,
                                            13 + tau, D, buf.data_ptr(), stream))

    d_direct = torch.zeros_like(d_all)
    daily(d_all, None, 0)
    daily(d_direct, None, _lib.DDR_PERIOD_DIRECT_STORE)
    variants_identical = bool(torch.equal(d_all, d_direct))
    del d_direct
    k = timed_alternating({"all_tiled": lambda: daily(d_all, None, 0),
                           "all_direct": lambda: daily(d_all, None, _lib.DDR_PERIOD_DIRECT_STORE),
                           "gauge": lambda: daily(d_gauge, C.byref(gzc), 0),
                           "copy_of_bytes_read": lambda: dst.copy_(src)}, max(args.reps, 10), 3, inner=10)
    read = N * T * 4
    for name in ("all_tiled", "all_direct"):
        k[name]["read_bytes"], k[name]["write_bytes"] = read, N * (T // 24 + 1) * 4
        k[name]["gb_per_s"] = (read + k[name]["write_bytes"]) / (k[name]["median_ms"] * 1e-3) / 1e9
    k["copy_of_bytes_read"].update(read_bytes=read, write_bytes=read,
                                   gb_per_s=2 * read / (k["copy_of_bytes_read"]["median_ms"] * 1e-3) / 1e9)
    result["daily_kernel"] = dict(k, chunk_hours=T, store_variants_identical=variants_identical, tiled_vs_direct=k["all_direct"]["median_ms"] / k["all_tiled"]["median_ms"],
                                  tiled_vs_copy=k["all_tiled"]["median_ms"] / k["copy_of_bytes_read"]["median_ms"])
    for name, v in k.items():
        print(f"daily kernel, {name}: median {v['median_ms']:.4f} ms [{v['min_ms']:.4f}, {v['max_ms']:.4f}]", flush=True)
    result["accepted"] = bool(ok)
    line = json.dumps(result)
    print(line)
    outp = Path(args.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    outp.write_text(line + "\n")
    if not ok:
        raise SystemExit("PeriodRouter is slower than, or needs more memory than, the composition it replaces")


if __name__ == "__main__":
    main()
