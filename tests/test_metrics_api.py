"""ddr_amd.validation: argument checking, the metric order against the header, and the F14 fixture (no GPU)."""

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_golden
from ddr_amd.validation import METRIC_NAMES, metrics_device

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"
LISTED_CASES = [(5, 1), (5, 2), (6, 3), (7, 89), (7, 100), (5, 365), (4, 1000), (3, 5479), (2, 8192), (6, 512), (6, 513)]


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="HIP device only"):
        metrics_device(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="HIP device only"):
        metrics_device(torch.zeros(3), torch.zeros(3))


def test_argument_errors():
    """Shape, dtype and warm-up are checked before the device, so they raise for host tensors too."""
    z = torch.zeros
    with pytest.raises(ValueError, match="float32"):
        metrics_device(z(2, 3, dtype=torch.float64), z(2, 3))
    with pytest.raises(ValueError, match="float32"):
        metrics_device(z(2, 3), z(2, 3, dtype=torch.float16))
    with pytest.raises(ValueError, match="same"):
        metrics_device(z(2, 3), z(2, 4))
    with pytest.raises(ValueError, match="same"):
        metrics_device(z(2, 3), z(3))
    with pytest.raises(ValueError, match="same"):
        metrics_device(z(2, 3, 4), z(2, 3, 4))
    for warmup in (-1, 3, 7):
        with pytest.raises(ValueError, match="warmup"):
            metrics_device(z(2, 3), z(2, 3), warmup=warmup)
    with pytest.raises(TypeError):
        metrics_device(np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32))


def test_c_abi_refuses_bad_arguments():
    """ddr_metrics_f32 checks its arguments before any launch: no device needed."""
    from ddr_amd import _lib

    lib = _lib.load()
    p = 4096  # (never dereferenced: every call below is refused, or a no-op)
    assert lib.ddr_metrics_f32(0, 10, None, 0, None, 0, None, None, None) == _lib.DDR_OK
    assert lib.ddr_metrics_f32(0, 100000, p, 10, p, 10, p, p, None) == _lib.DDR_OK
    for G, D, ps, ts in ((-1, 10, 10, 10), (2, -1, 10, 10), (2, 10, -1, 10), (2, 10, 10, -1)):
        assert lib.ddr_metrics_f32(G, D, p, ps, p, ts, p, p, None) == _lib.DDR_ERR_ARG
        assert b"negative" in lib.ddr_last_error()
    for D in (0, 8193, 1 << 40):
        assert lib.ddr_metrics_f32(2, D, p, D, p, D, p, p, None) == _lib.DDR_ERR_ARG
        assert b"8192" in lib.ddr_last_error()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        pred, target, out, count = args
        assert lib.ddr_metrics_f32(2, 10, pred, 10, target, 10, out, count, None) == _lib.DDR_ERR_ARG
        assert b"null" in lib.ddr_last_error()


def test_metric_names_match_header():
    text = HEADER.read_text()
    body = re.search(r"enum\s*\{([^}]*DDR_METRIC_[^}]*)\}", text).group(1)
    names = [m.lower() for m in re.findall(r"DDR_METRIC_([A-Z0-9_]+)", body)]
    assert tuple(names) == METRIC_NAMES
    assert len(METRIC_NAMES) == 18
    assert re.search(r"DDR_METRIC_BIAS\s*=\s*0\b", body) and body.rstrip().rstrip(",").split()[-1] == "DDR_N_METRICS"


def test_fixture_holds_every_case():
    d = load_golden("metrics")
    assert tuple(d["names"]) == METRIC_NAMES
    have = {tuple(c) for c in d["cases"].tolist()}
    assert set(LISTED_CASES) <= have
    for G, D in LISTED_CASES:
        tag = f"{G}x{D}"
        assert d[f"pred_{tag}"].shape == (G, D) and d[f"pred_{tag}"].dtype == np.float32
        assert d[f"target_{tag}"].shape == (G, D) and d[f"target_{tag}"].dtype == np.float32
        assert d[f"ref_{tag}"].shape == (18, G) and d[f"ref_{tag}"].dtype == np.float64
        assert not np.isnan(d[f"pred_{tag}"]).any()
    # every special row kind occurs, at a short and at a long window
    names = list(d["special_names"])
    for lo, hi in ((1, 512), (513, 8192)):
        seen = set()
        for G, D in LISTED_CASES:
            if lo <= D <= hi:
                seen |= set(d[f"special_{G}x{D}"].tolist())
        assert seen >= set(range(len(names))), (lo, hi, seen)
