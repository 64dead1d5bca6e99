#!/usr/bin/env python
"""Time ddr_amd.validation.SummedQPrime with HIP events at an evaluation-shaped size (needs an MI355X).

    python tools/summedq_time.py                                  # 8e5 rows, 3000 gauges, 5479 days and 8760 hours
    python tools/summedq_time.py --rows 100000 --gauges 400 --reps 5

The network is ``synthetic.forest`` with Zipf basin sizes (the largest basin about 3/8 of the rows); the gauges are
every basin's outlet plus random interior reaches, so the member lists overlap and run from 1 member to the largest
basin.  The q' store is log-normal, generated on the device.  Per store (daily: rho = 1, hourly: rho = 24) the
script prints the median and minimum of ``reps`` timed calls, the algorithmic bytes ``sum_g M_g * D * rho * 4`` and
the resulting TB/s; the same sums as the reference formulates them, on the same device tensors in PyTorch
(``reshape.mean`` first, then a loop over gauges of ``index_select`` + ``nansum``); and the largest gauge alone with
and without the cross-workgroup split.  One JSON line at the end, with the library's build hash.
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
from ddr_amd.validation import SummedQPrime  # noqa: E402


def upstream_lists(net, n_gauges: int, seed: int):
    """(off, idx, sizes): ascending upstream members (the reach itself included) of every basin outlet and of random
    interior reaches, ``n_gauges`` in all."""
    n, down = net.n, net.down
    size = np.ones(n, np.int64)
    for i in range(n):  # (reaches are numbered upstream first)
        if down[i] >= 0:
            size[down[i]] += size[i]
    pos = np.zeros(n, np.int64)  # preorder position: a reach's subtree is a contiguous range
    nxt = np.zeros(n, np.int64)
    start = 0
    for i in range(n - 1, -1, -1):
        d = down[i]
        if d < 0:
            pos[i] = start
            start += size[i]
        else:
            pos[i] = nxt[d]
            nxt[d] += size[i]
        nxt[i] = pos[i] + 1
    order = np.argsort(pos)
    outlets = np.nonzero(down < 0)[0]
    rng = np.random.default_rng(seed)
    if len(outlets) >= n_gauges:
        gauges = outlets[np.argsort(-size[outlets])[:n_gauges]]
    else:
        interior = rng.choice(np.nonzero(down >= 0)[0], size=n_gauges - len(outlets), replace=False)
        gauges = np.concatenate([outlets, interior])
    gauges = gauges[rng.permutation(len(gauges))]
    lists = [np.sort(order[pos[g]:pos[g] + size[g]]) for g in gauges]
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(m) for m in lists], out=off[1:])
    return off, np.concatenate(lists).astype(np.int32), size[gauges]


def lognormal_store(n: int, T: int, device, seed: int) -> torch.Tensor:
    gen = torch.Generator(device=device).manual_seed(seed)
    qr = torch.empty((n, T), device=device, dtype=torch.float32)
    scale = torch.empty((n, 1), device=device).log_normal_(float(np.log(0.5)), 1.0, generator=gen)
    for s in range(0, n, 65536):
        qr[s:s + 65536].log_normal_(0.0, 0.5, generator=gen).mul_(scale[s:s + 65536])
    return qr


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


def torch_loop(qr: torch.Tensor, rho: int, off: np.ndarray, idx: torch.Tensor) -> torch.Tensor:
    """The reference's formulation (scripts/summed_q_prime.py:230 and 258-259) on device tensors."""
    n, T = qr.shape
    D = T // rho
    daily = qr[:, : D * rho].reshape(n, D, rho).mean(dim=2) if rho > 1 else qr
    pred = torch.zeros((len(off) - 1, D), device=qr.device, dtype=torch.float32)
    for g in range(len(off) - 1):
        pred[g] = torch.nansum(daily.index_select(0, idx[off[g]:off[g + 1]]), dim=0)
    return pred


def time_store(name, qr, rho, off, idx, sizes, args, device) -> dict:
    D = qr.shape[1] // rho
    bytes_ = int(off[-1]) * D * rho * 4
    summed = SummedQPrime(off, idx, device=device, chunk=args.chunk)
    r = timed(lambda: summed(qr, rho), args.reps, args.warmup)
    r.update(store=name, rho=rho, days=D, gauges=len(off) - 1, members=int(off[-1]), largest=int(sizes.max()),
             algorithmic_bytes=bytes_, tb_per_s=bytes_ / (r["median_ms"] * 1e-3) / 1e12, chunk=args.chunk)
    print(f"{name}: {r['gauges']} gauges, {r['members']} members (largest {r['largest']}), D = {D}, rho = {rho}: "
          f"median {r['median_ms']:.3f} ms, min {r['min_ms']:.3f} ms, {bytes_ / 1e9:.2f} GB -> {r['tb_per_s']:.2f} TB/s")
    if not args.skip_torch:
        idx_dev = torch.from_numpy(idx.astype(np.int64)).to(device)
        t = timed(lambda: torch_loop(qr, rho, off, idx_dev), args.torch_reps, 1)
        r["torch_loop_median_ms"], r["torch_loop_min_ms"] = t["median_ms"], t["min_ms"]
        worst = float((torch_loop(qr, rho, off, idx_dev) / summed(qr, rho) - 1).abs().max())
        r["torch_loop_max_rel_diff"] = worst
        print(f"{name}: PyTorch loop (index_select + nansum per gauge) median {t['median_ms']:.1f} ms, "
              f"{t['median_ms'] / r['median_ms']:.1f}x the kernel; max relative difference {worst:.2e}")
    g = int(np.argmax(sizes))
    big_off = np.array([0, off[g + 1] - off[g]], np.int64)
    big_idx = idx[off[g]:off[g + 1]]
    for label, chunk in (("split", args.chunk), ("unsplit", 1 << 30)):
        alone = SummedQPrime(big_off, big_idx, device=device, chunk=chunk)
        t = timed(lambda: alone(qr, rho), max(3, args.reps // 4), 1)
        r[f"largest_alone_{label}_ms"] = t["median_ms"]
        print(f"{name}: the largest gauge alone ({int(big_off[1])} members), {label}: median {t['median_ms']:.3f} ms")
    return r


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=800_000)
    ap.add_argument("--basins", type=int, default=1000)
    ap.add_argument("--gauges", type=int, default=3000)
    ap.add_argument("--days", type=int, default=5479, help="columns of the daily store (0: skip it)")
    ap.add_argument("--hours", type=int, default=8760, help="columns of the hourly store (0: skip it)")
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true", help="skip the PyTorch loop")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("summedq_time needs a HIP device")
    device = torch.device("cuda:0")
    net = synthetic.forest(synthetic.zipf_sizes(args.rows, args.basins, 0.375), seed=args.seed)
    off, idx, sizes = upstream_lists(net, args.gauges, args.seed)
    print(f"{net.n} rows, {len(off) - 1} gauges, {int(off[-1])} members, lists from {int(sizes.min())} to "
          f"{int(sizes.max())} members (median {int(np.median(sizes))})", flush=True)
    rows = []
    for name, T, rho in (("daily", args.days, 1), ("hourly", args.hours, 24)):
        if T <= 0:
            continue
        qr = lognormal_store(net.n, T, device, args.seed + rho)
        rows.append(time_store(name, qr, rho, off, idx, sizes, args, device))
        del qr
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "build": _lib.load().ddr_version().decode(),
                      "rows": net.n, "summedq": rows}))


if __name__ == "__main__":
    main()
