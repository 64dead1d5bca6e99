"""The attribute statistics on the device (mirrors ``ddr.io.statistics.set_statistics``, ``io/statistics.py:14-58``).

The reference walks the attribute store on the host once per dataset: ``nanmin / nanmax / nanmean / nanstd /
nanpercentile(10) / nanpercentile(90)`` of every attribute, cached as JSON.  :func:`attribute_statistics` computes the
same table in one :func:`ddr_amd.stats.summarize` call over the (A, n) table; :func:`write_statistics_json` and
:func:`read_statistics_json` use the reference's file layout, so a file written here is the one the reference's
``stats_file.exists()`` branch reads, and the other way round.

:class:`~ddr_amd.io.AttributeStore` and :class:`~ddr_amd.geometry.GeometryPredictor` are unchanged: they take the
table's values (``mean``, ``std``, ``p10``, ``p90``) as before, from either source.

The statistics are fp64 over the store's own values and rounded once.  The reference accumulates a float32 store in
float32 (NumPy returns float32 there), so a reference-written JSON differs from this one in float32's last digits.
"""

from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from ..stats import summarize

#: the keys of one attribute's entry, in the order ``set_statistics`` writes them
STATISTIC_KEYS = ("min", "max", "mean", "std", "p10", "p90")


def attribute_statistics(values, names, device="cuda") -> dict:
    """``{name: {"min", "max", "mean", "std", "p10", "p90"}}`` as Python floats, in that key order, for the (A, n)
    table ``values`` whose row a holds attribute ``names[a]`` (NaN is a missing value, as in ``np.nan*``; an
    attribute without a value gets NaN everywhere).

    A host array (float32 or float64) is uploaded once to ``device``; a device tensor is taken as it is.  One
    :func:`~ddr_amd.stats.summarize` call and one device-to-host copy of the (A, 7) table.  HIP device only.
    ``AttributeStore`` and ``GeometryPredictor`` are unchanged: they take these values as they took the JSON's."""
    names = [str(n) for n in names]
    if len(set(names)) != len(names):
        raise ValueError("attribute names must be unique")
    if isinstance(values, torch.Tensor):
        t = values
    else:
        a = np.asarray(values)
        if a.dtype not in (np.float32, np.float64):
            raise ValueError("values must be float32 or float64")
        t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError("values must be float32 or float64")
    if t.dim() != 2:
        raise ValueError("values must be an (A, n) table")
    if t.shape[0] != len(names):
        raise ValueError(f"values has {t.shape[0]} rows for {len(names)} names")
    if not t.is_cuda:
        if not isinstance(values, torch.Tensor):
            if not torch.cuda.is_available():
                raise RuntimeError("attribute_statistics runs on the HIP device only (no CPU fallback)")
            t = t.to(device)
        else:
            raise RuntimeError("attribute_statistics runs on the HIP device only (no CPU fallback): pass a HIP "
                               "tensor or a NumPy array")
    table = summarize(t, q=(0.1, 0.9)).table.cpu().numpy()
    # columns: count, min, max, mean, std, p10, p90
    return {name: {k: float(v) for k, v in zip(STATISTIC_KEYS, row[1:])} for name, row in zip(names, table)}


def write_statistics_json(path, stats: dict) -> None:
    """Write ``stats`` as ``set_statistics`` does (``json.dump(..., indent=2)``: NaN is written as ``NaN``)."""
    for name, entry in stats.items():
        if tuple(entry) != STATISTIC_KEYS:
            raise ValueError(f"{name}: keys must be {STATISTIC_KEYS} in this order, not {tuple(entry)}")
    with open(Path(path), "w") as f:
        json.dump({str(n): {k: float(v) for k, v in e.items()} for n, e in stats.items()}, f, indent=2)


def read_statistics_json(path) -> dict:
    """The table of a statistics file, written here or by the reference: ``{name: {key: float}}``."""
    with open(Path(path)) as f:
        raw = json.load(f)
    return {str(n): {str(k): float(v) for k, v in e.items()} for n, e in raw.items()}
