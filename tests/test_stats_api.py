"""ddr_amd.stats, ddr_amd.io.statistics and ddr_amd.train.step_summary: argument checking, the constants against the
header, the statistics JSON and the log lines (no GPU)."""

import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from ddr_amd import _lib, stats
from ddr_amd.io import (STATISTIC_KEYS, attribute_statistics, read_statistics_json, write_statistics_json)
from ddr_amd.stats import SUMMARY_COLUMNS, SUMMARY_METHODS, summarize
from ddr_amd.train import StepSummary, step_summary

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"


def test_host_tensors_raise():
    with pytest.raises(RuntimeError, match="HIP device only"):
        summarize(torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="HIP device only"):
        summarize(torch.zeros(3, dtype=torch.float64), q=(0.5,))
    with pytest.raises(RuntimeError, match="HIP device only"):
        attribute_statistics(torch.zeros(2, 3), ["a", "b"])
    with pytest.raises(RuntimeError, match="HIP device only"):
        step_summary(torch.zeros(18, 4, dtype=torch.float64), {"n": torch.zeros(5)})


def test_summarize_argument_errors():
    """Checked before the device, so they raise for host tensors too."""
    z = torch.zeros
    with pytest.raises(TypeError):
        summarize(np.zeros((2, 3), np.float32))
    for dtype in (torch.float16, torch.int32, torch.bfloat16):
        with pytest.raises(ValueError, match="float32 or float64"):
            summarize(z(2, 3, dtype=dtype))
    for shape in ((), (2, 3, 4)):
        with pytest.raises(ValueError, match=r"\(N,\) or \(R, N\)"):
            summarize(z(shape))
    with pytest.raises(ValueError, match="method"):
        summarize(z(2, 3), method="nearest")
    with pytest.raises(ValueError, match="at most 8"):
        summarize(z(2, 3), q=[0.1] * 9)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            summarize(z(2, 3), q=(0.5, bad))
    with pytest.raises(ValueError, match="probabilities"):
        summarize(z(2, 3), q=("x",))
    for out in (z(2, 6), z(2, 7, dtype=torch.float64), z(3, 6, dtype=torch.float64),
                z(6, 2, dtype=torch.float64).t(), np.zeros((2, 6))):
        with pytest.raises(ValueError, match="out must be"):
            summarize(z(2, 3), q=(0.5,), out=out)


def test_attribute_statistics_argument_errors():
    with pytest.raises(ValueError, match="unique"):
        attribute_statistics(np.zeros((2, 3), np.float32), ["a", "a"])
    with pytest.raises(ValueError, match="float32 or float64"):
        attribute_statistics(np.zeros((2, 3), np.int32), ["a", "b"])
    with pytest.raises(ValueError, match="float32 or float64"):
        attribute_statistics(torch.zeros(2, 3, dtype=torch.float16), ["a", "b"])
    with pytest.raises(ValueError, match=r"\(A, n\)"):
        attribute_statistics(np.zeros(3, np.float32), ["a"])
    with pytest.raises(ValueError, match="2 rows for 3 names"):
        attribute_statistics(np.zeros((2, 3), np.float32), ["a", "b", "c"])


def test_step_summary_argument_errors():
    mv = torch.zeros(18, 4, dtype=torch.float64)
    ok = {"n": torch.zeros(5)}
    with pytest.raises(TypeError):
        step_summary(np.zeros((18, 4)), ok)
    for bad in (torch.zeros(18, 4), torch.zeros(17, 4, dtype=torch.float64), torch.zeros(18, dtype=torch.float64)):
        with pytest.raises(ValueError, match="metrics_device"):
            step_summary(bad, ok)
    with pytest.raises(ValueError, match="mapping"):
        step_summary(mv, [torch.zeros(5)])
    for bad in (torch.zeros(5, dtype=torch.float64), torch.zeros(2, 5), np.zeros(5, np.float32)):
        with pytest.raises(ValueError, match="parameter 'n'"):
            step_summary(mv, {"n": bad})
    for out in (torch.zeros(4, 6), torch.zeros(5, 6, dtype=torch.float64), torch.zeros(4, 5, dtype=torch.float64)):
        with pytest.raises(ValueError, match="out must be"):
            step_summary(mv, ok, out=out)


def _call(lib, fn, R=2, N=10, x=4096, stride=10, K=1, q=(0.5,), method=0, flags=0, out=4096, work=4096):
    qa = (C.c_double * 16)(*q) if q is not None else None
    return getattr(lib, fn)(R, N, x, stride, K, qa, method, flags, out, work, None)


@pytest.mark.parametrize("fn", ["ddr_summary_f32", "ddr_summary_f64"])
def test_c_abi_refuses_bad_arguments(fn):
    """The arguments are checked before any launch: no device needed.  (The pointers, 4096, are never dereferenced:
    every call below is refused or a no-op, and the stream is null.)"""
    lib = _lib.load()
    assert _call(lib, fn, R=0) == _lib.DDR_OK
    assert _call(lib, fn, R=0, N=0, x=None, out=None, work=None, K=0, q=None) == _lib.DDR_OK
    for kw in (dict(R=-1), dict(N=-1), dict(stride=-1), dict(K=-1)):
        assert _call(lib, fn, **kw) == _lib.DDR_ERR_ARG
        assert b"negative" in lib.ddr_last_error()
    assert _call(lib, fn, K=9, q=(0.5,) * 9) == _lib.DDR_ERR_ARG
    assert b"at most 8" in lib.ddr_last_error()
    for bad in (-0.25, 1.25, float("nan"), float("inf")):
        assert _call(lib, fn, K=2, q=(0.5, bad)) == _lib.DDR_ERR_ARG
        assert b"q[1]" in lib.ddr_last_error()
        assert _call(lib, fn, R=0, K=2, q=(0.5, bad)) == _lib.DDR_ERR_ARG  # refused even where nothing would run
    for method in (-1, 2, 7):
        assert _call(lib, fn, method=method) == _lib.DDR_ERR_ARG
        assert b"method" in lib.ddr_last_error()
    for flags in (2, 3, -1, 1 << 20):
        assert _call(lib, fn, flags=flags) == _lib.DDR_ERR_ARG
        assert b"flag" in lib.ddr_last_error()
    for kw in (dict(x=None), dict(out=None), dict(work=None), dict(q=None)):
        assert _call(lib, fn, **kw) == _lib.DDR_ERR_ARG
        assert b"null" in lib.ddr_last_error()
    assert _call(lib, fn, N=1 << 31, stride=1 << 31) == _lib.DDR_ERR_ARG
    assert b"2^31" in lib.ddr_last_error()
    assert _call(lib, fn, work=4100) == _lib.DDR_ERR_ARG
    assert b"aligned" in lib.ddr_last_error()


def test_work_bytes():
    lib = _lib.load()
    for args in ((-1, 1, 4), (1, -1, 4), (1, 9, 4), (1, 1, 2), (1, 1, 16), ((1 << 20) + 1, 1, 4)):
        assert lib.ddr_summary_work_bytes(*args) == -1
    assert lib.ddr_summary_work_bytes(0, 8, 4) == 0
    one = lib.ddr_summary_work_bytes(1, 8, 4)
    assert one > 0 and one % 16 == 0
    assert lib.ddr_summary_work_bytes(7, 8, 4) == 7 * one
    assert lib.ddr_summary_work_bytes(1, 8, 8) > one > lib.ddr_summary_work_bytes(1, 1, 4)


def test_constants_match_header():
    text = HEADER.read_text()
    body = re.search(r"enum\s*\{([^}]*DDR_SUMMARY_COUNT[^}]*)\}", text).group(1)
    names = [m.lower() for m in re.findall(r"DDR_SUMMARY_([A-Z0-9_]+)", body)]
    assert names[-1] == "n_columns"
    assert tuple(names[:-1]) == SUMMARY_COLUMNS == ("count", "min", "max", "mean", "std")
    assert re.search(r"DDR_SUMMARY_COUNT\s*=\s*0\b", body)
    body = re.search(r"enum\s*\{([^}]*DDR_SUMMARY_LINEAR[^}]*)\}", text).group(1)
    assert re.search(r"DDR_SUMMARY_LINEAR\s*=\s*0\b", body) and "DDR_N_SUMMARY_METHODS" in body
    methods = tuple(m.lower() for m in re.findall(r"DDR_SUMMARY_([A-Z]+)\b", body))
    assert methods == SUMMARY_METHODS == ("linear", "lower")

    def define(name):
        return int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1))

    assert define("DDR_SUMMARY_SKIP_INF") == stats.SUMMARY_SKIP_INF == _lib.SUMMARY_SKIP_INF
    assert define("DDR_SUMMARY_MAX_Q") == stats.MAX_QUANTILES == 8
    assert define("DDR_SUMMARY_TILE") == stats.TILE
    for fn in ("ddr_summary_f32", "ddr_summary_f64"):
        params = re.search(rf"ddr_status\s+{fn}\s*\(([^)]*)\)", text).group(1)
        assert len(params.split(",")) == len(_lib._SIGS[fn][1]) == 11
        assert fn in _lib.EXPORTED
    assert _lib._SIGS["ddr_summary_work_bytes"] == (C.c_int64, [C.c_int64, C.c_int32, C.c_int32])


def test_statistics_json_round_trip(tmp_path):
    stats_ = {"aridity": dict(zip(STATISTIC_KEYS, (0.0, 9.5, 1.25, 0.1 + 0.2, 0.3, 4.0))),
              "empty": dict.fromkeys(STATISTIC_KEYS, float("nan")),
              "log10_uparea": dict(zip(STATISTIC_KEYS, (-1.0, 6.0, 1.5, 1e-3, 1 / 3, 3.5)))}
    path = tmp_path / "merit_attribute_statistics_attrs.json"
    write_statistics_json(path, stats_)
    raw = json.loads(path.read_text())  # what the reference's json.load sees
    assert list(raw) == list(stats_)
    for name in raw:
        assert tuple(raw[name]) == STATISTIC_KEYS == ("min", "max", "mean", "std", "p10", "p90")
    back = read_statistics_json(path)
    assert list(back) == list(stats_)
    for name in stats_:
        for k in STATISTIC_KEYS:
            a, b = stats_[name][k], back[name][k]
            assert (a == b) or (a != a and b != b)
    assert back["aridity"]["std"] == 0.1 + 0.2  # a float survives to the last bit
    # the reference's writer: json.dump(dict of dicts, indent=2)
    assert path.read_text() == json.dumps(stats_, indent=2)
    with pytest.raises(ValueError, match="keys"):
        write_statistics_json(path, {"a": {"max": 1.0, "min": 0.0, "mean": 0.5, "std": 0.1, "p10": 0.1, "p90": 0.9}})


def test_step_summary_lines_from_a_host_record():
    s = StepSummary(record=None, names=("n", "q_spatial"), sizes=(10, 10))
    #        count  min    max   mean      std  median
    record = [[5.0, -3.0, 0.9, 0.123456, 0.1, 0.54321],
              [7.0, 0.1, 9.0, 12.5, 0.1, 3.0],
              [7.0, -0.4, 1.0, float("nan"), 0.1, -0.25],
              [10.0, 0.015, 0.25, 0.1, 0.0, 0.0312345678],
              [8.0, 0.0, 1.0, 0.5, 0.0, 0.5]]
    v = s.decode(record)
    assert list(v) == ["nse_mean", "nse_median", "rmse_mean", "rmse_median", "kge_mean", "kge_median",
                       "n_min", "n_median", "n_max", "n_nan_count",
                       "q_spatial_min", "q_spatial_median", "q_spatial_max", "q_spatial_nan_count"]
    assert v["n_nan_count"] == 0 and v["q_spatial_nan_count"] == 2
    assert list(s.decode(np.asarray(record)).values())[6:] == list(v.values())[6:]
    rule = "----------------------------------------"
    epoch, mini_batch = 3, 17
    want = [rule, f"Epoch: {epoch:<9} | Mini Batch: {mini_batch:<8} ", rule,
            f"{'Metric':<10} | {'Mean':>12} | {'Median':>12}", rule,
            f"{'NSE':<10} | {0.123456:12.4f} | {0.54321:12.4f}",
            f"{'RMSE':<10} | {12.5:12.4f} | {3.0:12.4f}",
            f"{'KGE':<10} | {float('nan'):12.4f} | {-0.25:12.4f}", rule,
            f"n: min={0.015:.6f}, median={0.0312345678:.6f}, max={0.25:.6f}",
            f"q_spatial: min={0.0:.6f}, median={0.5:.6f}, max={1.0:.6f} (nan_count=2)"]
    assert s.lines(epoch, mini_batch, values=v) == want
    assert s.lines(values=v) == want[2:]  # no header without an epoch and a mini-batch, as log_metrics
    with pytest.raises(ValueError, match="record"):
        s.decode(record[:4])
