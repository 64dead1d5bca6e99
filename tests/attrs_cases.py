"""Shared by test_attrs_api.py and test_gpu_attrs.py: the golden fixture of the attribute feed and a NumPy model of
``AttributeStore.batch``'s four rules (ddr_amd/io/attributes.py, csrc/attrs.hip)."""

from __future__ import annotations

import functools

import numpy as np

from conftest import load_golden

CASES = ("b300", "b1", "allnan")
MERIT_PATHS = ("length", "slope")
LYNKER_PATHS = ("length", "slope", "x", "top_width", "side_slope")
QUIET = np.uint32(0x00400000)
HOST_NAN = np.uint32(0xFFC00000)  # an invalid operation's result on the reference's host


@functools.lru_cache(maxsize=1)
def golden() -> dict:
    g = load_golden("attrs")
    for v in g.values():
        v.setflags(write=False)
    return g


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and bool((bits(a) == bits(b)).all())


def gage_dicts(g: dict) -> dict:
    """The generator's three gauge dicts, rebuilt from the fixture's columns."""
    staid = g["gage_staid"].tolist()
    drain = g["gage_drain"].tolist()
    return {"fs": {"STAID": staid, "FLOW_SCALE": g["gage_flow_scale"].tolist(), "DRAIN_SQKM": drain},
            "raw": {"STAID": staid, "DRAIN_SQKM": drain, "COMID_DRAIN_SQKM": g["gage_comid_drain"].tolist(),
                    "COMID_UNITAREA_SQKM": g["gage_unit"].tolist()},
            "none": {"STAID": staid, "DRAIN_SQKM": drain}}


def _nan_result(res: np.ndarray, first: np.ndarray, second: np.ndarray) -> np.ndarray:
    """``res`` with every NaN replaced by the rule of csrc/attrs.hip: the first operand's NaN, else the second's,
    quieted; else the host's default NaN."""
    r = res.view(np.uint32).copy()
    a, b = np.broadcast_to(first, res.shape), np.broadcast_to(second, res.shape)
    pick = np.where(np.isnan(a), a.view(np.uint32) | QUIET, np.where(np.isnan(b), b.view(np.uint32) | QUIET, HOST_NAN))
    nan = np.isnan(res)
    r[nan] = pick[nan]
    return r.view(np.float32)


def model(table: np.ndarray, means: np.ndarray, stds: np.ndarray, active: np.ndarray, paths: dict, fills: dict):
    """The four rules in NumPy.  ``table`` (n_conus, >= A) aligned, ``paths`` name -> (n_conus,) array or a scalar,
    ``fills`` name -> float32.  Returns ``(spatial (A, N), normalized (N, A), {name: (N,)})``."""
    A = len(means)
    n_conus = table.shape[0]
    active = np.asarray(active, np.int64)
    ok = (active >= 0) & (active < n_conus)
    v = np.full((len(active), A), np.nan, np.float32)  # rule 1
    v[ok] = table[active[ok], :A]
    spatial = np.ascontiguousarray(v.T)
    for a in range(A):  # rule 2
        nan = np.isnan(spatial[a])
        fill = np.float32(means[a])
        if np.isnan(fill):
            have = spatial[a][~nan].astype(np.float64)
            with np.errstate(invalid="ignore"):
                m = np.float32(have.sum() / have.size) if have.size else np.float32(np.nan)
            fill = HOST_NAN.view(np.float32) if np.isnan(m) else m
        spatial[a].view(np.uint32)[nan] = np.float32(fill).view(np.uint32)
    with np.errstate(all="ignore"):  # rule 3
        m, s = means.astype(np.float32)[None, :], stds.astype(np.float32)[None, :]
        x = np.ascontiguousarray(spatial.T)
        d = _nan_result(x - m, m, x)
        normalized = _nan_result(d / s, d, s)
    out = {}
    for name, arr in paths.items():  # rule 4
        if np.ndim(arr) == 0:
            out[name] = np.full(len(active), np.float32(arr), np.float32)
            continue
        got = np.full(len(active), np.float32(fills[name]), np.float32)
        vals = arr[active[ok]].astype(np.float32)
        got[ok] = np.where(np.isnan(vals), np.float32(fills[name]), vals)
        out[name] = got
    return spatial, np.ascontiguousarray(normalized), out


def flow_scale_model(N: int, gage_c, rows, factors, skip) -> np.ndarray:
    """The reference's sequential loop (readers.py:335-360)."""
    out = np.ones(N, np.float32)
    for s, r in zip(np.asarray(gage_c).tolist(), np.asarray(rows).tolist()):
        if r < 0 or r >= len(factors) or (skip is not None and skip[r]) or s < 0 or s >= N:
            continue
        out[s] = factors[r]
    return out


def random_dataset(n_conus: int, A: int, seed: int, flagged=(), lynker: bool = True):
    """An aligned table with NaN, inf and missing rows, statistics (NaN means at ``flagged``, whose columns hold
    multiples of 1/8 so that every summation order is exact), and flowpath arrays with NaN and inf entries."""
    rng = np.random.default_rng(seed)
    table = (rng.normal(0.0, 1.0, (n_conus, A)) * rng.lognormal(0.0, 1.5, (1, A))).astype(np.float32)
    for a in flagged:
        table[:, a] = rng.integers(-8000, 8000, n_conus) / 8.0
    table[rng.random(table.shape) < 0.06] = np.nan
    table[rng.random(n_conus) < 0.08] = np.nan  # reaches the store lacks
    k = max(1, n_conus // 40)
    table[rng.integers(0, n_conus, k), rng.integers(0, A, k)] = np.inf
    table[rng.integers(0, n_conus, k), rng.integers(0, A, k)] = -np.inf
    for a in flagged:
        col = table[:, a]
        col[np.isinf(col)] = 640.0
    means = rng.normal(0.0, 1.0, A).astype(np.float32)
    stds = rng.uniform(0.5, 2.0, A).astype(np.float32)
    means[list(flagged)] = np.nan
    paths = {}
    for name in (LYNKER_PATHS if lynker else MERIT_PATHS):
        v = rng.uniform(0.1, 100.0, n_conus).astype(np.float32)
        v[rng.random(n_conus) < 0.05] = np.nan
        v[rng.integers(0, n_conus, 2)] = [np.inf, -np.inf]
        paths[name] = v
    return table, means, stds, paths
