#!/usr/bin/env python
"""Time the device summaries (ddr_amd.stats.summarize) with HIP events at the two shapes the reference computes on the
host (needs an MI355X).

    python tools/stats_time.py
    python tools/stats_time.py --reps 10 --inner 20 --out /tmp/stats.json

Shapes:

* (a) the step's log record (``scripts/train.py:110-132``): three (939 409,) fp32 parameter rows and an (18, 256) fp64
  metrics table, ``ddr_amd.train.step_summary`` -- eager, and replayed as a captured graph;
* (b) the attribute statistics (``io/statistics.py:45-52``): a (10, 1 039 032) fp32 table with 1 % NaN,
  ``summarize(table, q=(0.1, 0.9))``.

Yardsticks, on the same device tensors:

* the best PyTorch composition, tried in several forms and the fastest kept: ``torch.median`` / ``nanquantile`` /
  ``sort`` + index / ``kthvalue`` for the order statistics, ``nanmean`` and ``where`` compositions for the moments, and
  the ``masked_select`` form (``nse[nse.isfinite()].median()``, which waits for the device);
* a streaming read (``sum``) of the rows' bytes times the number of digit passes (4 for fp32): the floor of a radix
  selection that reads the row once per pass;
* for (a), the reference's own form: ``.detach().cpu()`` of every tensor, ``min / torch.median / max`` and NumPy's
  ``nanmean / nanmedian`` on the host.

Each is the median / minimum / maximum of ``reps`` windows of ``inner`` calls, the candidates alternating inside every
repetition.  No condition is attached to the times: they are reported.  One JSON line with the library's build hash,
also written to ``--out`` (default ``profiles/stats/stats.json``).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ddr_amd import _lib  # noqa: E402
from ddr_amd.capture import CapturedStep  # noqa: E402
from ddr_amd.stats import summarize  # noqa: E402
from ddr_amd.train import step_summary  # noqa: E402
from ddr_amd.validation import METRIC_NAMES  # noqa: E402
from feed_time import timed_group  # noqa: E402

I_NSE, I_RMSE, I_KGE = (METRIC_NAMES.index(k) for k in ("nse", "rmse", "kge"))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reaches", type=int, default=939_409)
    ap.add_argument("--gauges", type=int, default=256)
    ap.add_argument("--attrs", type=int, default=10)
    ap.add_argument("--store", type=int, default=1_039_032)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-inner", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "stats" / "stats.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stats_time needs a HIP device")
    device = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    n, G, A, S = args.reaches, args.gauges, args.attrs, args.store

    # ---- (a) the step record
    ranges = {"n": (0.015, 0.25), "q_spatial": (0.0, 1.0), "p_spatial": (1.0, 200.0)}
    params = {k: torch.from_numpy(rng.uniform(lo, hi, n).astype(np.float32)).to(device)
              for k, (lo, hi) in ranges.items()}
    mv_host = rng.standard_normal((len(METRIC_NAMES), G))
    mv_host[I_NSE, :3] = (np.nan, np.inf, -np.inf)
    mv = torch.from_numpy(mv_host).to(device)
    rec = torch.empty((3 + len(params), 6), device=device, dtype=torch.float64)
    k_med = (n - 1) // 2

    def ours_step():
        return step_summary(mv, params, out=rec)

    graph = CapturedStep(ours_step)

    def metrics_nan():
        nse = mv[I_NSE]
        fin = torch.where(nse.isinf(), torch.nan, nse)
        return [f(r) for r in (fin, mv[I_RMSE], mv[I_KGE]) for f in (torch.nanmean, torch.nanmedian)]

    def metrics_masked():  # INTEGRATION.md's earlier example: boolean indexing waits for the device
        nse = mv[I_NSE]
        out = [nse[nse.isfinite()].mean(), nse[nse.isfinite()].median()]
        return out + [f(r) for r in (mv[I_RMSE], mv[I_KGE]) for f in (torch.nanmean, torch.nanmedian)]

    forms_a = {
        "torch_median": lambda: ([(p.min(), torch.median(p), p.max()) for p in params.values()], metrics_nan()),
        "torch_nanquantile": lambda: ([(p.min(), torch.nanquantile(p, 0.5, interpolation="lower"), p.max())
                                       for p in params.values()], metrics_nan()),
        "torch_sort": lambda: ([(s[0], s[k_med], s[-1]) for s in (p.sort().values for p in params.values())],
                               metrics_nan()),
        "torch_kthvalue": lambda: ([(p.min(), p.kthvalue(k_med + 1).values, p.max()) for p in params.values()],
                                   metrics_nan()),
        "torch_masked_select": lambda: ([(p.min(), torch.median(p), p.max()) for p in params.values()],
                                        metrics_masked()),
    }

    def reference_step():
        np_mv = mv.detach().cpu().numpy()
        nse = np_mv[I_NSE]
        nse = nse[~np.isinf(nse) & ~np.isnan(nse)]
        out = [np.nanmean(nse), np.nanmedian(nse), np.nanmean(np_mv[I_RMSE]), np.nanmedian(np_mv[I_RMSE]),
               np.nanmean(np_mv[I_KGE]), np.nanmedian(np_mv[I_KGE])]
        for p in params.values():
            h = p.detach().cpu()
            out += [h.min().item(), torch.median(h).item(), h.max().item()]
        return out

    # the same values, at the timed size
    v = ours_step().read()
    ref = reference_step()
    close = [abs(v[k] - r) <= 1e-12 * max(1.0, abs(r)) for k, r in zip(list(v)[:6], ref[:6])]
    exact = [v[f"{name}_{f}"] == ref[6 + 3 * i + j] for i, name in enumerate(params) for j, f in
             enumerate(("min", "median", "max"))]
    for name, fn in forms_a.items():
        triples, _ = fn()
        exact += [v[f"{pn}_{f}"] == t[j].item() for pn, t in zip(params, triples) for j, f in
                  enumerate(("min", "median", "max"))]
    if not (all(close) and all(exact)):
        raise SystemExit(f"the step record and its yardsticks disagree: {close} {exact}")

    passes = 4
    bytes_a = sum(p.numel() * 4 for p in params.values())
    stream_a = torch.rand(bytes_a * passes // 4, device=device)
    t_a = timed_group(dict(step_summary=ours_step, step_summary_graph=graph, stream_read=lambda: stream_a.sum(),
                           **forms_a), args.reps, args.warmup, args.inner)
    t_a.update(timed_group({"reference_host": reference_step}, args.reps, 1, args.host_inner))
    del stream_a

    # ---- (b) the attribute statistics
    table_host = (rng.standard_normal((A, S), dtype=np.float32) * np.float32(3.0) + np.float32(1.5))
    table_host[rng.random(table_host.shape) < 0.01] = np.nan
    table = torch.from_numpy(table_host).to(device)
    qs = torch.tensor([0.1, 0.9], device=device)  # (nanquantile takes q in the input's dtype)
    qs64 = torch.tensor([0.1, 0.9], device=device, dtype=torch.float64)

    def ours_attrs():
        return summarize(table, q=(0.1, 0.9))

    def moments():
        nan = table.isnan()
        mean = table.nanmean(1)
        std = ((table - mean[:, None]) ** 2).nanmean(1).sqrt()
        return torch.where(nan, torch.inf, table).amin(1), torch.where(nan, -torch.inf, table).amax(1), mean, std

    def attrs_nanquantile():
        return (*moments(), torch.nanquantile(table, qs, dim=1))

    def attrs_sort():
        s = table.sort(dim=1).values  # NaN sorts last
        cnt = (~table.isnan()).sum(1)
        v_ = (cnt - 1).to(torch.float64)[None, :] * qs64[:, None]
        lo = v_.floor()
        g = (v_ - lo)
        lo = lo.long()
        hi = torch.minimum(lo + 1, (cnt - 1)[None, :])
        a, b = s.gather(1, lo.T).double(), s.gather(1, hi.T).double()
        return (*moments(), a + (b - a) * g.T)

    def attrs_kthvalue():  # needs the counts on the host: one wait
        cnt = (~table.isnan()).sum(1).tolist()
        out = []
        for r, c in enumerate(cnt):
            for q in (0.1, 0.9):
                lo = int((c - 1) * q)
                out.append((table[r].kthvalue(lo + 1).values, table[r].kthvalue(min(lo + 2, c)).values))
        return (*moments(), out)

    forms_b = {"torch_nanquantile": attrs_nanquantile, "torch_sort": attrs_sort, "torch_kthvalue": attrs_kthvalue}
    got = ours_attrs().table.cpu().numpy()
    want = np.stack([np.nanmin(table_host, 1), np.nanmax(table_host, 1), np.nanmean(table_host.astype(np.float64), 1),
                     np.nanstd(table_host.astype(np.float64), 1),
                     *np.nanquantile(table_host.astype(np.float64), [0.1, 0.9], axis=1)], axis=1)
    if not np.allclose(got[:, 1:], want, rtol=1e-12, atol=0.0):
        raise SystemExit("summarize and NumPy disagree on the attribute table")
    srt = attrs_sort()[-1].cpu().numpy()
    if not np.allclose(srt, got[:, 5:], rtol=1e-12, atol=0.0):
        raise SystemExit("the sort composition and summarize disagree")

    bytes_b = A * S * 4
    stream_b = torch.rand(bytes_b * passes // 4, device=device)
    t_b = timed_group(dict(summarize=ours_attrs, stream_read=lambda: stream_b.sum(), **forms_b), args.reps,
                      args.warmup, max(1, args.inner // 4))

    for tag, t in (("a", t_a), ("b", t_b)):
        for k, r in t.items():
            print(f"({tag}) {k}: median {r['median_ms']:.4f} ms, min {r['min_ms']:.4f} ms, max {r['max_ms']:.4f} ms")
    best_a = min(forms_a, key=lambda k: t_a[k]["median_ms"])
    best_b = min(forms_b, key=lambda k: t_b[k]["median_ms"])
    result = {
        "device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(),
        "step": {"reaches": n, "gauges": G, "parameters": len(params), "row_bytes_times_passes": bytes_a * passes,
                 "step_summary_ms": t_a["step_summary"]["median_ms"],
                 "step_summary_graph_ms": t_a["step_summary_graph"]["median_ms"],
                 "torch_best": best_a, "torch_ms": t_a[best_a]["median_ms"],
                 "stream_read_ms": t_a["stream_read"]["median_ms"],
                 "reference_host_ms": t_a["reference_host"]["median_ms"], "timings": t_a},
        "attributes": {"attributes": A, "store_reaches": S, "nan_fraction": 0.01,
                       "row_bytes_times_passes": bytes_b * passes,
                       "summarize_ms": t_b["summarize"]["median_ms"], "torch_best": best_b,
                       "torch_ms": t_b[best_b]["median_ms"], "stream_read_ms": t_b["stream_read"]["median_ms"],
                       "timings": t_b},
        "identical_outputs": True,
    }
    line = json.dumps(result)
    print(line)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(line + "\n")


if __name__ == "__main__":
    main()
