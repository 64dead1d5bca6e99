"""ddr_amd.stats.summarize, attribute_statistics and step_summary on the device against NumPy on the float64 cast.

Every content below exists because one radix pass can get it wrong; every size because the walk over tiles can.
Bars (n the row's count, a and b the two order statistics of a quantile):
  count, min, max, every `lower` quantile and every `linear` quantile with g = 0: equal as numbers (NaN matches NaN);
  other `linear` quantiles: |dev - ref| <= 2^-50 max(|a|, |b|)  (three fp64 roundings, slack for NumPy versions);
  mean: |dev - ref| <= n 2^-52 mean|x|  (two recursive fp64 sums of n terms);
  std:  |dev - ref| <= n 2^-52 (std_ref + mean|x|).
"""

import math
import warnings

import numpy as np
import pytest
import torch

from ddr_amd.io import STATISTIC_KEYS, attribute_statistics
from ddr_amd.stats import TILE, summarize
from ddr_amd.train import step_summary
from ddr_amd.validation import METRIC_NAMES

pytestmark = pytest.mark.gpu

T = TILE
SIZES = [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1, 200_003]
F64_SIZES = [65, 3 * T + 1]
CONTENTS = ["normal", "equal", "low_digit", "high_digit", "specials", "duplicates", "nan_1pct", "nan_all_but_one",
            "nan_all", "offset"]
CASES = [(c, n, "f32") for c in CONTENTS for n in SIZES] + [(c, n, "f64") for c in CONTENTS for n in F64_SIZES]
EPS = 2.0 ** -52
worst = {"linear": 0.0, "mean": 0.0, "std": 0.0}


def make_row(content: str, N: int, dtype, rng) -> np.ndarray:
    f32 = dtype == np.float32
    if content == "normal":
        x = rng.standard_normal(N)
    elif content == "equal":
        x = np.full(N, -7.25)
    elif content == "low_digit":  # the keys differ in their last 8 bits only
        r = rng.integers(0, 256, N)
        return ((0x3F800000 | r).astype(np.uint32).view(np.float32) if f32 else
                (0x3FF0000000000000 | r).astype(np.uint64).view(np.float64))
    elif content == "high_digit":  # ... in their first 8 bits only (sign and seven exponent bits: never inf or NaN)
        r = rng.integers(0, 256, N)
        return (((r << 24) | 0x00400000).astype(np.uint32).view(np.float32) if f32 else
                ((r.astype(np.uint64) << np.uint64(56)) | np.uint64(0x0008000000000000)).view(np.float64))
    elif content == "specials":
        fi = np.finfo(dtype)
        sp = np.array([-0.0, 0.0, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.max, -fi.max,
                       fi.tiny, -fi.tiny, 1.5, -2.5, 0.0, -0.0], dtype=dtype)
        x = rng.standard_normal(N).astype(dtype)
        k = min(N, len(sp))
        x[rng.permutation(N)[:k]] = sp[:k]
        return x
    elif content == "duplicates":
        x = rng.integers(1, 4, N).astype(np.float64)
    elif content == "nan_1pct":
        x = rng.standard_normal(N)
        x[rng.permutation(N)[:max(1, N // 100)]] = np.nan  # (the same count in every row)
    elif content == "nan_all_but_one":
        x = np.full(N, np.nan)
        x[rng.integers(0, N)] = 3.5
    elif content == "nan_all":
        x = np.full(N, np.nan)
    elif content == "offset":  # mean >> std: a one-pass variance fails here
        x = 1e4 + rng.standard_normal(N)
    return x.astype(dtype)


def pick_q(n: int) -> list:
    """0, 0.1, 0.25, 0.5, 0.9, 1, one q with (n - 1) q an exact integer and one with g >= 0.5 (where n allows)."""
    q = [0.0, 0.1, 0.5, 0.9, 1.0, 0.25]
    m = n - 1
    if m >= 2:
        j = next(j for j in range(max(1, m // 3), m) if float(m) * (j / m) == float(j))
        q.append(j / m)
        v = float(m) * ((m // 2 + 0.75) / m)
        assert v - math.floor(v) >= 0.5
        q.append((m // 2 + 0.75) / m)
    else:
        q += [1.0 / 3.0, 0.75]  # (n = 2: g = 0.75; n <= 1: every g is 0)
    return q


def oracle(row64: np.ndarray, q, skip_inf=False):
    """NumPy on the float64 row: (count, min, max, mean, std, linear quantiles, lower quantiles, (a, b, g) per q)."""
    x = row64.copy()
    if skip_inf:
        x[np.isinf(x)] = np.nan
    kept = np.sort(x[~np.isnan(x)])
    n = kept.size
    if n == 0:
        nan = [np.nan] * len(q)
        return 0, np.nan, np.nan, np.nan, np.nan, nan, nan, [(np.nan, np.nan, 0.0)] * len(q)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        lin = np.nanquantile(x, q, method="linear")
        stats = (np.nanmin(x), np.nanmax(x), np.nanmean(x), np.nanstd(x))
    low, abg = [], []
    for p in q:
        v = (n - 1) * p
        lo = int(math.floor(v))
        low.append(kept[lo])
        abg.append((kept[lo], kept[min(lo + 1, n - 1)], v - lo))
    return (n, *stats, lin, low, abg)


def same(a, b) -> bool:
    return bool(a == b) or (a != a and b != b)


def check_row(dev_lin, dev_low, row64, q, skip_inf=False, tag=""):
    n, mn, mx, mean, std, lin, low, abg = oracle(row64, q, skip_inf)
    for dev in (dev_lin, dev_low):
        assert dev[0] == n, (tag, "count", dev[0], n)
        assert same(dev[1], mn) and same(dev[2], mx), (tag, "min/max", dev[1:3], mn, mx)
    if n == 0:
        assert np.isnan(dev_lin[1:]).all() and np.isnan(dev_low[1:]).all(), tag
        return
    x = row64[~np.isnan(row64)]
    if skip_inf:
        x = x[~np.isinf(x)]
    with np.errstate(all="ignore"):
        scale = float(np.mean(np.abs(x)))
    for dev in (dev_lin, dev_low):
        if not np.isfinite(mean):
            assert same(dev[3], mean), (tag, "mean", dev[3], mean)
        else:
            err = abs(dev[3] - mean)
            worst["mean"] = max(worst["mean"], err / (n * EPS * scale) if scale else err)
            assert err <= n * EPS * scale, (tag, "mean", dev[3], mean, err)
        if not np.isfinite(std):
            assert same(dev[4], std), (tag, "std", dev[4], std)
        else:
            err = abs(dev[4] - std)
            bound = n * EPS * (std + scale)
            worst["std"] = max(worst["std"], err / bound if bound else err)
            assert err <= bound, (tag, "std", dev[4], std, err)
    for k, p in enumerate(q):
        a, b, g = abg[k]
        assert same(dev_low[5 + k], low[k]), (tag, "lower", p, dev_low[5 + k], low[k])
        d, r = dev_lin[5 + k], lin[k]
        if g == 0.0 or same(d, r) or not np.isfinite(r):
            assert same(d, r), (tag, "linear", p, d, r)
        else:
            bound = 2.0 ** -50 * max(abs(a), abs(b))
            worst["linear"] = max(worst["linear"], abs(d - r) / bound)
            assert abs(d - r) <= bound, (tag, "linear", p, d, r, abs(d - r))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("content,N,prec", CASES, ids=[f"{c}-{n}-{p}" for c, n, p in CASES])
def test_summarize_matches_numpy(cuda, content, N, prec):
    dtype = np.float32 if prec == "f32" else np.float64
    rng = np.random.default_rng(1000 * CONTENTS.index(content) + N % 977 + (prec == "f64"))
    R, pad = 3, 5
    host = np.full((R, N + pad), 123.0, dtype=dtype)  # the padding must never be read as part of a row
    for r in range(R):
        host[r, :N] = make_row(content, N, dtype, rng)
    buf = torch.from_numpy(host).to(cuda)
    x = buf[:, :N]  # a sliced view: the row stride is N + 5
    n = int((~np.isnan(host[0, :N])).sum())
    q = pick_q(n)
    assert len(q) == 8
    lin = summarize(x, q, method="linear")
    again = summarize(x, q, method="linear")
    alone = summarize(buf[2:3, :N], q, method="linear")  # the same row alone: R = 1, another position
    low = summarize(x, q, method="lower")
    assert lin.table.shape == (R, 13) and lin.table.dtype == torch.float64 and lin.quantiles.shape == (R, 8)
    assert torch.equal(bits(lin.table), bits(again.table)), "two calls differ"
    assert torch.equal(bits(lin.table[2:3]), bits(alone.table)), "a row depends on R or on its position"
    assert torch.equal(lin.count, lin.table[:, 0]) and torch.equal(bits(lin.std), bits(lin.table[:, 4]))
    tl, tw = lin.table.cpu().numpy(), low.table.cpu().numpy()
    for r in range(R):
        check_row(tl[r], tw[r], host[r, :N].astype(np.float64), q, tag=(content, N, prec, r))
    print(f"worst so far, in units of the bound: {worst}")


@pytest.mark.parametrize("N", [65, T + 1])
def test_skip_inf(cuda, N):
    rng = np.random.default_rng(N)
    host = np.stack([make_row("specials", N, np.float32, rng) for _ in range(2)])
    assert np.isinf(host).sum(1).min() >= 2
    x = torch.from_numpy(host).to(cuda)
    q = pick_q(N - 2)
    for skip in (True, False):
        tl = summarize(x, q, skip_inf=skip).table.cpu().numpy()
        tw = summarize(x, q, method="lower", skip_inf=skip).table.cpu().numpy()
        for r in range(2):
            check_row(tl[r], tw[r], host[r].astype(np.float64), q, skip_inf=skip, tag=("skip_inf", skip, N, r))
        if skip:
            assert (tl[:, 0] == N - 2).all() and np.isfinite(tl[:, 1:5]).all()
        else:  # one +inf and one -inf: NumPy's mean is NaN
            assert (tl[:, 0] == N).all() and np.isnan(tl[:, 3]).all() and np.isinf(tl[:, 1:3]).all()


def test_shapes_and_out(cuda):
    x = torch.randn(7, 300, device=cuda)
    one = summarize(x[3], (0.5,))
    assert one.table.shape == (1, 6)
    assert torch.equal(bits(one.table), bits(summarize(x, (0.5,)).table[3:4]))
    out = torch.full((7, 6), -1.0, device=cuda, dtype=torch.float64)
    got = summarize(x, (0.5,), out=out)
    assert got.table is out and torch.equal(bits(out), bits(summarize(x, (0.5,)).table))
    # an inner stride != 1 is made contiguous; no quantiles: the five moments only
    xt = x.t()
    assert torch.equal(bits(summarize(xt).table), bits(summarize(xt.contiguous()).table))
    assert summarize(xt).table.shape == (300, 5)
    empty = summarize(torch.empty(2, 0, device=cuda), (0.5,)).table.cpu().numpy()
    assert (empty[:, 0] == 0).all() and np.isnan(empty[:, 1:]).all()
    assert summarize(torch.empty(0, 9, device=cuda), (0.5,)).table.shape == (0, 6)


def test_attribute_statistics(cuda):
    A, n = 4, 50_021
    rng = np.random.default_rng(7)
    table = np.empty((A, n), np.float32)
    table[0] = rng.lognormal(3.0, 2.0, n)                 # no NaN
    table[1] = np.nan                                     # all NaN
    table[2] = 250.0 + 40.0 * rng.standard_normal(n)
    table[2, rng.permutation(n)[:500]] = np.nan
    table[3] = rng.uniform(-5.0, 2.0, n)
    table[3, rng.permutation(n)[:n // 3]] = np.nan
    names = ["uparea", "missing", "elevation", "log_k"]
    got = attribute_statistics(table, names, device=cuda)
    dev = attribute_statistics(torch.from_numpy(table).to(cuda), names)
    assert list(got) == names and got.keys() == dev.keys()
    distance = 0.0
    for a, name in enumerate(names):
        assert tuple(got[name]) == STATISTIC_KEYS
        assert all(isinstance(v, float) for v in got[name].values())
        assert all(same(got[name][k], dev[name][k]) for k in STATISTIC_KEYS)
        if name == "missing":
            assert all(math.isnan(v) for v in got[name].values())
            continue
        data = table[a].astype(np.float64)
        ref = {"min": np.nanmin(data, axis=0), "max": np.nanmax(data, axis=0), "mean": np.nanmean(data, axis=0),
               "std": np.nanstd(data, axis=0), "p10": np.nanpercentile(data, 10, axis=0),
               "p90": np.nanpercentile(data, 90, axis=0)}
        kept = np.sort(data[~np.isnan(data)])
        cnt, scale = kept.size, float(np.mean(np.abs(kept)))
        assert got[name]["min"] == ref["min"] and got[name]["max"] == ref["max"]
        assert abs(got[name]["mean"] - ref["mean"]) <= cnt * EPS * scale
        assert abs(got[name]["std"] - ref["std"]) <= cnt * EPS * (ref["std"] + scale)
        for key, p in (("p10", 0.1), ("p90", 0.9)):
            lo = int(math.floor((cnt - 1) * p))
            assert abs(got[name][key] - ref[key]) <= 2.0 ** -50 * max(abs(kept[lo]), abs(kept[lo + 1]))
        # the reference's own arithmetic on a float32 store (NumPy stays in float32): printed, not asserted
        d32 = table[a]
        ref32 = {"min": np.nanmin(d32), "max": np.nanmax(d32), "mean": np.nanmean(d32), "std": np.nanstd(d32),
                 "p10": np.nanpercentile(d32, 10), "p90": np.nanpercentile(d32, 90)}
        for k in STATISTIC_KEYS:
            rel = abs(got[name][k] - float(ref32[k])) / max(abs(got[name][k]), 1e-300)
            distance = max(distance, rel)
            print(f"{name}.{k}: device {got[name][k]!r} float32 NumPy {float(ref32[k])!r} rel {rel:.3e}")
    print(f"largest relative distance from the float32 NumPy statistics: {distance:.3e}")


def test_step_summary(cuda):
    G, N = 37, 4099
    rng = np.random.default_rng(11)
    mv = rng.standard_normal((len(METRIC_NAMES), G))
    i_nse, i_rmse, i_kge = (METRIC_NAMES.index(k) for k in ("nse", "rmse", "kge"))
    mv[i_rmse] = np.abs(mv[i_rmse])
    mv[i_nse, [1, 8]] = np.nan
    mv[i_nse, 3] = np.inf
    mv[i_nse, [5, 30]] = -np.inf
    mv[i_kge, 2] = np.nan
    params = {"n": rng.uniform(0.015, 0.25, N).astype(np.float32),
              "q_spatial": rng.uniform(0.0, 1.0, N).astype(np.float32),
              "p_spatial": rng.uniform(1.0, 200.0, N).astype(np.float32)}
    params["q_spatial"][[17, 4000]] = np.nan
    dev = {k: torch.from_numpy(v).to(cuda) for k, v in params.items()}
    s = step_summary(torch.from_numpy(mv).to(cuda), dev)
    assert s.record.shape == (6, 6) and s.record.dtype == torch.float64 and s.names == tuple(params)
    v = s.read()
    nse = mv[i_nse]
    fin = nse[~np.isinf(nse) & ~np.isnan(nse)]  # scripts/train.py:112
    want = {"nse_mean": np.nanmean(fin), "nse_median": np.nanmedian(fin[~np.isinf(fin)]),
            "rmse_mean": np.nanmean(mv[i_rmse]), "rmse_median": np.nanmedian(mv[i_rmse]),
            "kge_mean": np.nanmean(mv[i_kge]), "kge_median": np.nanmedian(mv[i_kge])}
    for m, row in (("nse", fin), ("rmse", mv[i_rmse]), ("kge", mv[i_kge])):
        kept = np.sort(row[~np.isnan(row)])
        a, b = kept[(kept.size - 1) // 2], kept[kept.size // 2]  # the median's two order statistics
        assert abs(v[f"{m}_mean"] - want[f"{m}_mean"]) <= kept.size * EPS * float(np.mean(np.abs(kept))), m
        assert abs(v[f"{m}_median"] - want[f"{m}_median"]) <= 2.0 ** -50 * max(abs(a), abs(b)), m
    for name, p in params.items():
        t = torch.from_numpy(p[~np.isnan(p)])
        assert v[f"{name}_min"] == t.min().item() and v[f"{name}_max"] == t.max().item()
        assert v[f"{name}_median"] == torch.median(t).item()
        assert v[f"{name}_nan_count"] == int(np.isnan(p).sum())
        want.update({f"{name}_min": t.min().item(), f"{name}_median": torch.median(t).item(),
                     f"{name}_max": t.max().item()})
    assert v["q_spatial_nan_count"] == 2 and v["n_nan_count"] == 0
    rule = "----------------------------------------"
    lines = [rule, f"Epoch: {2:<9} | Mini Batch: {5:<8} ", rule,
             f"{'Metric':<10} | {'Mean':>12} | {'Median':>12}", rule,
             f"{'NSE':<10} | {want['nse_mean']:12.4f} | {want['nse_median']:12.4f}",
             f"{'RMSE':<10} | {want['rmse_mean']:12.4f} | {want['rmse_median']:12.4f}",
             f"{'KGE':<10} | {want['kge_mean']:12.4f} | {want['kge_median']:12.4f}", rule]
    for name in params:
        lines.append(f"{name}: min={want[f'{name}_min']:.6f}, median={want[f'{name}_median']:.6f}, "
                     f"max={want[f'{name}_max']:.6f}" + (" (nan_count=2)" if name == "q_spatial" else ""))
    assert s.lines(2, 5) == lines
