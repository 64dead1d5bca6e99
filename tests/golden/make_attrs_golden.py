"""Generate ``attrs.npz``: the reference's per-batch attribute collation on a synthetic dataset.  BUILD-CONTAINER ONLY.

Like ``make_golden.py`` this imports the reference from ``/root/reference`` (read-only) with stub modules for what is
not installed (xarray, icechunk, zarr, rustworkx) and for the ``ddr`` packages the functions run here never touch, and
runs the reference's own code on the CPU:

* ``Merit._get_attributes`` / ``Merit._build_common_tensors`` (geodatazoo/merit.py:92-124, 273-319) and the
  ``LynkerHydrofabric`` pair (lynker_hydrofabric.py:105-135, 302-354), with a stub ``self`` and a fake
  ``attribute_ds`` that supports the one ``ds[names].isel(<dim>=idx).compute().to_array(dim=...).values`` chain;
* ``fill_nans``, ``naninfmean`` and ``build_flow_scale_tensor`` (io/readers.py:299-410).

The dataset: 700 CONUS reaches; an attribute store of 640 columns in shuffled order (631 CONUS reaches, 8 foreign ids,
one CONUS reach twice: the last column wins), A = 10, about 5 % NaN and a few +-inf; attribute 3 has a NaN mean, so its
NaNs are filled with the per-batch NaN-mean -- its finite values are multiples of 1/8 below 1024 in magnitude, so the
reference's fp32 ``nanmean`` is exact in any summation order (checked here against the fp64 mean rounded once);
flowpath arrays with NaN and inf entries.  Batches (ascending ``active``): 300 reaches, 1 reach, and 40 reaches none of
which has a value of attribute 3 (the all-NaN row).  Gauge dicts of the three kinds (``FLOW_SCALE`` with NaN entries,
the raw area columns, neither) and a batch of 12 gauges with an unknown STAID, an un-padded id and segments shared by
two gauges (value then value, value then NaN-skip, NaN-skip then value).

Run:  python tests/golden/make_attrs_golden.py
"""

from __future__ import annotations

import importlib.util
import sys
import types
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference/src/ddr")

N_CONUS, N_STORE, A = 700, 640, 10
FLAGGED = 3  # the attribute whose mean is NaN
NAMES = [f"attr{k}" for k in range(A)]


class _Stub(types.ModuleType):
    """A module that has every name (as ``object``): enough for module-level imports, annotations and base classes."""
    __path__: list = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return object


def load_reference():
    for name in ["icechunk", "xarray", "zarr", "zarr.storage", "rustworkx", "ddr", "ddr.geodatazoo", "ddr.io",
                 "ddr.validation", "ddr.geodatazoo.base_geodataset", "ddr.geodatazoo.dataclasses", "ddr.io.builders",
                 "ddr.io.statistics", "ddr.validation.configs", "ddr.validation.enums"]:
        sys.modules[name] = _Stub(name)

    def _load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    readers = _load("ddr.io.readers", REF / "io/readers.py")
    merit = _load("ddr.geodatazoo.merit", REF / "geodatazoo/merit.py")
    lynker = _load("ddr.geodatazoo.lynker_hydrofabric", REF / "geodatazoo/lynker_hydrofabric.py")
    return readers, merit, lynker


class FakeDataset:
    """``ds[names].isel(<dim>=idx).compute().to_array(dim=...).values`` -> (A, len(idx)), like xarray's."""

    def __init__(self, values: np.ndarray, cols=None):
        self._values, self._cols = values, cols

    def __getitem__(self, names):
        assert list(names) == NAMES
        return self

    def isel(self, **kw):
        (idx,) = kw.values()
        return FakeDataset(self._values, list(idx))

    def compute(self):
        return self

    def to_array(self, dim):
        return SimpleNamespace(values=self._values[:, self._cols])


def dataset(rng):
    conus = rng.permutation(np.arange(N_CONUS) * 7 + 71000).astype(np.int64)
    in_store = rng.permutation(N_CONUS)[:631]
    foreign = np.arange(8, dtype=np.int64) + 5
    twice = conus[in_store[17]]
    store_ids = rng.permutation(np.concatenate([conus[in_store], foreign, [twice]]))
    assert len(store_ids) == N_STORE
    attrs = (rng.normal(0.0, 1.0, (A, N_STORE)) * rng.lognormal(1.0, 2.0, (A, 1))).astype(np.float32)
    attrs[FLAGGED] = rng.integers(-8000, 8000, N_STORE) / 8.0
    attrs[rng.random(attrs.shape) < 0.05] = np.nan
    for k, (a, c) in enumerate(zip(rng.integers(0, A, 6), rng.integers(0, N_STORE, 6))):
        attrs[a, c] = np.inf if k % 2 else -np.inf
    attrs[FLAGGED][np.isinf(attrs[FLAGGED])] = 512.0  # (keep that row's sums finite and exact)
    # 30 store columns of CONUS reaches without a value of the flagged attribute: the all-NaN batch
    no_value = rng.permutation(np.flatnonzero(np.isin(store_ids, conus)))[:30]
    attrs[FLAGGED, no_value] = np.nan
    means = np.nanmean(np.where(np.isfinite(attrs), attrs, np.nan), axis=1).astype(np.float32)
    stds = np.nanstd(np.where(np.isfinite(attrs), attrs, np.nan), axis=1).astype(np.float32)
    means[FLAGGED] = np.nan
    paths = {}
    for name, (lo, hi) in {"length": (200.0, 9000.0), "slope": (1e-5, 0.05), "top_width": (1.0, 300.0),
                           "side_slope": (0.5, 4.0), "x": (0.05, 0.45)}.items():
        v = rng.uniform(lo, hi, N_CONUS).astype(np.float32)
        v[rng.random(N_CONUS) < 0.04] = np.nan
        v[rng.integers(0, N_CONUS, 3)] = [np.inf, -np.inf, np.inf]
        paths[name] = v
    return conus, store_ids, attrs, means, stds, paths, no_value


def batches(rng, conus, store_ids, no_value):
    missing = np.flatnonzero(~np.isin(conus, store_ids))
    pos = {int(c): i for i, c in enumerate(conus)}
    twice = [c for c in np.unique(store_ids) if (store_ids == c).sum() == 2][0]
    b300 = rng.permutation(N_CONUS)[:300]
    if pos[int(twice)] not in b300:
        b300[0] = pos[int(twice)]  # (the reach the store holds twice belongs to the big batch)
    b300 = np.sort(b300)
    assert len(np.unique(b300)) == 300 and np.isin(b300, missing).any()
    b1 = np.array([np.flatnonzero(np.isin(conus, store_ids))[5]])
    none = np.array(sorted({pos[int(store_ids[c])] for c in no_value} - {pos[int(twice)]}))[:25]
    allnan = np.sort(np.concatenate([none, missing[:15]]))
    return {"b300": b300.astype(np.int64), "b1": b1.astype(np.int64), "allnan": allnan.astype(np.int64)}


def main():
    readers, merit, lynker = load_reference()
    rng = np.random.default_rng(20260)
    conus, store_ids, attrs, means, stds, paths, no_value = dataset(rng)
    out = {"conus_ids": conus, "store_ids": store_ids, "attributes": attrs, "means": means, "stds": stds,
           "flagged": np.int64(FLAGGED)}
    out.update({f"path_{k}": v for k, v in paths.items()})
    fills = {k: np.float32(readers.naninfmean(v)) for k, v in paths.items()}
    out.update({f"fill_{k}": v for k, v in fills.items()})

    t = lambda v: torch.tensor(v, device="cpu", dtype=torch.float32).unsqueeze(1)  # noqa: E731  (merit.py:58-80)
    common = dict(attributes_list=NAMES, attribute_ds=FakeDataset(attrs), means=t(means), stds=t(stds),
                  cfg=SimpleNamespace(device="cpu"), zarr_length_m=paths["length"], zarr_slope=paths["slope"])
    m_self = SimpleNamespace(**common, id_to_index={int(c): i for i, c in enumerate(store_ids)}, merit_ids=conus,
                             phys_means=t([readers.naninfmean(paths[k]) for k in ("length", "slope")]))
    m_self._get_attributes = lambda **kw: merit.Merit._get_attributes(m_self, **kw)
    cat = lambda ids: np.array([f"cat-{int(c)}" for c in ids])  # noqa: E731
    l_self = SimpleNamespace(**common, id_to_index={c: i for i, c in enumerate(cat(store_ids))}, hf_ids=cat(conus),
                             zarr_top_width=paths["top_width"], zarr_side_slope=paths["side_slope"],
                             zarr_muskingum_x=paths["x"],
                             phys_means=t([readers.naninfmean(paths[k])
                                           for k in ("length", "slope", "top_width", "side_slope", "x")]))
    l_self._get_attributes = lambda **kw: lynker.LynkerHydrofabric._get_attributes(l_self, **kw)

    for case, active in batches(rng, conus, store_ids, no_value).items():
        n = len(active)
        csr = sp.csr_matrix((n, n), dtype=np.float32)
        _, sa, nsa, fp = merit.Merit._build_common_tensors(m_self, csr, conus[active], active)
        _, sa_l, nsa_l, fp_l = lynker.LynkerHydrofabric._build_common_tensors(l_self, csr, cat(conus)[active], active)
        assert torch.equal(sa.view(torch.int32), sa_l.view(torch.int32))
        assert torch.equal(nsa.contiguous().view(torch.int32), nsa_l.contiguous().view(torch.int32))
        assert fp["top_width"].numel() == 0 and fp["side_slope"].numel() == 0
        assert sa.shape == (A, n) and nsa.shape == (n, A)
        out[f"{case}_active"] = active
        out[f"{case}_spatial"] = sa.numpy()
        out[f"{case}_normalized"] = nsa.contiguous().numpy()
        for k in ("length", "slope", "x"):
            out[f"{case}_merit_{k}"] = fp[k].numpy()
        for k in ("length", "slope", "x", "top_width", "side_slope"):
            out[f"{case}_lynker_{k}"] = fp_l[k].numpy()
        # the per-batch mean row: the reference's fp32 nanmean equals the fp64 mean rounded once
        raw = np.full(n, np.nan, np.float32)
        rows = np.array([m_self.id_to_index.get(int(c), -1) for c in conus[active]])
        raw[rows >= 0] = attrs[FLAGGED, rows[rows >= 0]]
        filled = sa.numpy()[FLAGGED][np.isnan(raw)]
        if np.isnan(raw).all():
            assert case == "allnan" and np.isnan(sa.numpy()[FLAGGED]).all()
        else:
            assert case != "allnan"
            want = np.float32(np.nanmean(raw.astype(np.float64)))
            assert filled.size or case == "b1"
            assert (filled.view(np.int32) == want.view(np.int32)).all(), (case, filled, want)
        print(case, n, "reaches;", int(np.isnan(raw).sum()), "without a value of the flagged attribute;",
              int((rows < 0).sum()), "not in the store")

    # flow_scale
    n_g = 20
    staid = [f"{1234000 + 7 * k:08d}" for k in range(n_g)]
    fs = rng.uniform(0.2, 1.0, n_g).round(6).tolist()
    for k in (2, 5, 11):
        fs[k] = float("nan")
    drain = rng.uniform(10.0, 500.0, n_g)
    comid_drain = drain + rng.normal(0.0, 20.0, n_g)
    unit = rng.uniform(5.0, 60.0, n_g)
    drain[3], comid_drain[6], unit[8], unit[9] = np.nan, np.nan, np.nan, 0.0
    dicts = {"fs": {"STAID": staid, "FLOW_SCALE": fs, "DRAIN_SQKM": drain.tolist()},
             "raw": {"STAID": staid, "DRAIN_SQKM": drain.tolist(), "COMID_DRAIN_SQKM": comid_drain.tolist(),
                     "COMID_UNITAREA_SQKM": unit.tolist()},
             "none": {"STAID": staid, "DRAIN_SQKM": drain.tolist()}}
    #        value,value on 40 | value,skip on 41 | skip,value on 42 | unknown | un-padded | plain ones
    batch = [staid[0], staid[1], staid[4], staid[2], staid[5], staid[7], "99999999", staid[3].lstrip("0"),
             staid[10], staid[11], staid[12], staid[19]]
    segs = [40, 40, 41, 41, 42, 42, 7, 90, 0, 299, 150, 151]
    num_segments = 300
    out.update(gage_staid=np.array(staid), gage_flow_scale=np.array(fs, np.float64), gage_drain=drain,
               gage_comid_drain=comid_drain, gage_unit=unit, fs_batch=np.array(batch), fs_segments=np.array(segs),
               fs_num_segments=np.int64(num_segments))
    for kind, d in dicts.items():
        got = readers.build_flow_scale_tensor(batch=batch, gage_dict=d, gage_compressed_indices=segs,
                                              num_segments=num_segments)
        out[f"fs_{kind}"] = got.numpy()
        # every gauge of the dict on a segment of its own: its factor, 1.0 where the reference skips it
        each = readers.build_flow_scale_tensor(batch=staid, gage_dict=d, gage_compressed_indices=list(range(n_g)),
                                               num_segments=n_g)
        out[f"fs_{kind}_each"] = each.numpy()
    assert out["fs_fs"][40] == np.float32(fs[1]) and out["fs_fs"][41] == np.float32(fs[4])
    assert out["fs_fs"][42] == np.float32(fs[7]) and (out["fs_none"] == 1).all()

    np.savez_compressed(HERE / "attrs.npz", **out)
    print("wrote", HERE / "attrs.npz", (HERE / "attrs.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
