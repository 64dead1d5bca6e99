"""The attribute feed without a GPU: its host halves (the alignment to CONUS order, the flowpath fill values, the
flow_scale factors) against the reference's golden, the NumPy model the GPU tests use against that golden, the Python
argument checks and the C ABI's declarations and refusals."""

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import attrs_cases as K
from ddr_amd import _lib
from ddr_amd.io import (AttributeStore, FlowScaleTable, RowIndex, align_attributes, flow_scale_factors, flowpath_fill,
                        pad_gage_ids)
from ddr_amd.io.attributes import padded_stride

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"
FUNCTIONS = ("ddr_feed_attributes_f32", "ddr_feed_attr_mean_work_bytes", "ddr_feed_attr_mean_f32",
             "ddr_feed_flow_scale_f32")


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.EXPORTED
        assert hasattr(_lib.load(), name)
    assert int(re.search(r"#define DDR_ATTR_MAX_FEATURES (\d+)", text).group(1)) == _lib.ATTR_MAX_FEATURES >= 64
    assert int(re.search(r"#define DDR_FLOWPATH_ARRAYS (\d+)", text).group(1)) == _lib.FLOWPATH_ARRAYS == 5


# ---- the host halves against the golden ---------------------------------------------------------------------------


def aligned_golden(g, **kw):
    return align_attributes(g["attributes"], g["store_ids"], g["conus_ids"], **kw)


@pytest.mark.parametrize("ids", ["int", "cat"])
def test_alignment_is_the_reference_dict(ids):
    g = K.golden()
    name = (lambda v: np.array([f"cat-{int(c)}" for c in v])) if ids == "cat" else (lambda v: v)
    table = align_attributes(g["attributes"], name(g["store_ids"]), name(g["conus_ids"]))
    A = g["attributes"].shape[0]
    assert table.dtype == np.float32 and table.shape == (len(g["conus_ids"]), padded_stride(A)) == (700, 12)
    lookup = {int(c): i for i, c in enumerate(g["store_ids"])}  # (the last column of a repeated id)
    n_twice = 0
    for i, c in enumerate(g["conus_ids"].tolist()):
        col = lookup.get(c)
        if col is None:
            assert np.isnan(table[i]).all()
        else:
            assert K.same_bits(table[i, :A], g["attributes"][:, col])
            n_twice += int((g["store_ids"] == c).sum() == 2)
        assert np.isnan(table[i, A:]).all()
    assert n_twice == 1 and sum(c not in lookup for c in g["conus_ids"].tolist()) == 700 - 631
    for stride in (10, 16):
        t = aligned_golden(g, row_stride=stride)
        assert t.shape[1] == stride and K.same_bits(t[:, :A], table[:, :A])
    with pytest.raises(ValueError, match="shorter than a row"):
        aligned_golden(g, row_stride=9)


def test_fill_values_are_the_reference_naninfmean():
    g = K.golden()
    for name in K.LYNKER_PATHS:
        fill = flowpath_fill(g[f"path_{name}"])
        assert isinstance(fill, np.float32) and K.same_bits(fill, g[f"fill_{name}"]), name
    assert np.isnan(flowpath_fill(np.array([np.nan, np.inf], np.float32)))
    wide = np.array([1.0, 1e-9, np.nan, -np.inf, 3.0])  # (its own dtype: the float64 mean, cast once)
    assert flowpath_fill(wide) == np.float32((1.0 + 1e-9 + 3.0) / 3)


def test_the_model_reproduces_the_golden():
    """The NumPy model of the four rules (attrs_cases.model), which the GPU tests compare the kernels with at other
    shapes, gives the reference's bits on every golden case."""
    g = K.golden()
    table = aligned_golden(g)
    lynker = {k: g[f"path_{k}"] for k in K.LYNKER_PATHS}
    fills = {k: g[f"fill_{k}"] for k in K.LYNKER_PATHS}
    for case in K.CASES:
        spatial, normalized, out = K.model(table, g["means"], g["stds"], g[f"{case}_active"], lynker, fills)
        assert K.same_bits(spatial, g[f"{case}_spatial"]), case
        assert K.same_bits(normalized, g[f"{case}_normalized"]), case
        for k in K.LYNKER_PATHS:
            assert K.same_bits(out[k], g[f"{case}_lynker_{k}"]), (case, k)
        for k in K.MERIT_PATHS:
            assert K.same_bits(out[k], g[f"{case}_merit_{k}"]), (case, k)
        assert K.same_bits(np.full(len(out["x"]), np.float32(0.3)), g[f"{case}_merit_x"])
    assert np.isnan(g["allnan_spatial"][int(g["flagged"])]).all() and np.isinf(g["b300_spatial"]).any()


@pytest.mark.parametrize("kind", ["fs", "raw", "none"])
def test_flow_scale_factors_against_the_reference(kind):
    g = K.golden()
    d = K.gage_dicts(g)[kind]
    host = flow_scale_factors(d)
    if kind == "none":
        assert host is None and (g["fs_none"] == 1).all()
        return
    factors, skip = host
    assert factors.dtype == np.float32 and skip.dtype == bool and len(factors) == len(skip) == len(d["STAID"])
    assert K.same_bits(np.where(skip, np.float32(1), factors), g[f"fs_{kind}_each"])
    assert skip.tolist() == ([isinstance(v, float) and np.isnan(v) for v in d["FLOW_SCALE"]] if kind == "fs"
                             else [False] * len(skip))
    assert skip.any() == (kind == "fs")
    # the batch of the golden through the same lookup FlowScaleTable.rows does, and the sequential loop
    rows = RowIndex(pad_gage_ids(d["STAID"])).lookup(pad_gage_ids(g["fs_batch"]))
    assert (rows == -1).sum() == 1 and rows[7] == 3  # the unknown gauge; the un-padded id
    got = K.flow_scale_model(int(g["fs_num_segments"]), g["fs_segments"], rows, factors, skip)
    assert K.same_bits(got, g[f"fs_{kind}"])


def test_flow_scale_factor_edge_cases():
    d = {"STAID": ["1", "2", "3", "4", "5", "6"], "DRAIN_SQKM": [100.0, 100.0, 100.0, 100.0, float("nan"), 100.0],
         "COMID_DRAIN_SQKM": [100.0, 90.0, 104.0, 130.0, 104.0, 104.0],
         "COMID_UNITAREA_SQKM": [10.0, 10.0, 10.0, 10.0, 10.0, 0.0]}
    factors, skip = flow_scale_factors(d)
    assert factors.tolist() == [1.0, 1.0, np.float32(0.6), 1.0, 1.0, 1.0] and not skip.any()
    f32nan = {"STAID": ["1", "2"], "FLOW_SCALE": [np.float32("nan"), 0.25]}  # (not a Python float: written as it is)
    factors, skip = flow_scale_factors(f32nan)
    assert np.isnan(factors[0]) and factors[1] == 0.25 and not skip.any()


# ---- argument checks ----------------------------------------------------------------------------------------------


def small(**over):
    kw = dict(attributes=np.zeros((3, 5), np.float32), attribute_ids=np.arange(5), means=np.zeros(3, np.float32),
              stds=np.ones(3, np.float32), conus_ids=np.arange(7), length=np.ones(7, np.float32),
              slope=np.ones(7, np.float32))
    kw.update(over)
    return kw


def test_python_argument_errors():
    """dtype, shape and lengths raise before a device is touched; a host store raises RuntimeError."""
    with pytest.raises(ValueError, match="float32"):
        AttributeStore(**small(attributes=np.zeros((3, 5), np.float64)))
    with pytest.raises(ValueError, match="float32"):
        AttributeStore(**small(means=np.zeros(3, np.float64)))
    with pytest.raises(ValueError, match="2-D"):
        AttributeStore(**small(attributes=np.zeros(15, np.float32)))
    with pytest.raises(ValueError, match="5 columns for 4 ids"):
        AttributeStore(**small(attribute_ids=np.arange(4)))
    with pytest.raises(ValueError, match="means has 4 entries for 3 attributes"):
        AttributeStore(**small(means=np.zeros(4, np.float32)))
    with pytest.raises(ValueError, match="stds has 2 entries"):
        AttributeStore(**small(stds=np.ones(2, np.float32)))
    with pytest.raises(ValueError, match="one value per CONUS reach"):
        AttributeStore(**small(length=np.ones(6, np.float32)))
    with pytest.raises(ValueError, match="one value per CONUS reach"):
        AttributeStore(**small(x=np.ones(8, np.float32)))
    with pytest.raises(ValueError, match="go together"):
        AttributeStore(**small(top_width=np.ones(7, np.float32)))
    with pytest.raises(ValueError, match="float32"):
        AttributeStore(**small(slope=np.ones(7, np.int32)))
    with pytest.raises(ValueError, match="attributes, not 65"):
        AttributeStore(**small(attributes=np.zeros((65, 5), np.float32), means=np.zeros(65, np.float32),
                               stds=np.ones(65, np.float32)))
    with pytest.raises(TypeError):
        AttributeStore(**small(attributes=[[0.0] * 5] * 3))
    with pytest.raises(TypeError):
        AttributeStore(**small(length=[1.0] * 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AttributeStore(**small(attributes=torch.zeros(3, 5)))  # a host tensor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AttributeStore(**small(length=torch.ones(7)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AttributeStore(**small(), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AttributeStore.from_aligned(torch.zeros(7, 3), np.zeros(3, np.float32), np.ones(3, np.float32), np.arange(7),
                                    np.ones(7, np.float32), np.ones(7, np.float32))
    with pytest.raises(ValueError, match="rows for 7 ids"):
        AttributeStore.from_aligned(np.zeros((6, 3), np.float32), np.zeros(3, np.float32), np.ones(3, np.float32),
                                    np.arange(7), np.ones(7, np.float32), np.ones(7, np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FlowScaleTable({"STAID": ["1"], "FLOW_SCALE": [0.5]}, device="cpu")


# ---- the C ABI's refusals (no device needed: every call is refused before a launch) --------------------------------


def test_feed_attributes_refusals():
    lib = _lib.load()
    p = 4096  # (never dereferenced)
    path = _lib.Flowpath()

    def run(table=p, stride=12, n_conus=100, A=10, active=p, N=5, fill=p, means=p, stds=p, spatial=p, normalized=p,
            path=None, flow_scale=None):
        return lib.ddr_feed_attributes_f32(table, stride, n_conus, A, active, N, fill, means, stds, spatial,
                                           normalized, path, flow_scale, None)

    for kw in ({"stride": -1}, {"n_conus": -1}, {"N": -1}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"negative" in lib.ddr_last_error(), kw
    for A in (0, -3, 65):
        assert run(A=A, stride=80) == _lib.DDR_ERR_ARG and b"n_attrs <= 64" in lib.ddr_last_error(), A
    assert run(stride=9) == _lib.DDR_ERR_ARG and b"row_stride" in lib.ddr_last_error()
    assert run(n_conus=2**31) == _lib.DDR_ERR_ARG and b"32-bit" in lib.ddr_last_error()
    for kw in ({"table": None}, {"active": None}, {"fill": None}, {"means": None}, {"stds": None},
               {"spatial": None}, {"normalized": None}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"null" in lib.ddr_last_error(), kw
    path.src[1] = p  # a source without an output
    assert run(path=C.byref(path)) == _lib.DDR_ERR_ARG and b"flowpath array 1" in lib.ddr_last_error()
    assert run(N=0, table=None, active=None, spatial=None, normalized=None) == _lib.DDR_OK  # no reaches: a no-op
    assert run(N=0, A=65, stride=80) == _lib.DDR_ERR_ARG  # (still checked)


def test_feed_attr_mean_refusals():
    lib = _lib.load()
    p = 4096
    assert lib.ddr_feed_attr_mean_work_bytes(0) == 0
    assert lib.ddr_feed_attr_mean_work_bytes(1) > 0 and lib.ddr_feed_attr_mean_work_bytes(64) > 0
    assert lib.ddr_feed_attr_mean_work_bytes(-1) < 0 and lib.ddr_feed_attr_mean_work_bytes(65) < 0
    need = lib.ddr_feed_attr_mean_work_bytes(2)

    def run(table=p, stride=12, n_conus=100, A=10, active=p, N=5, flagged=p, n_flagged=2, fill=p, work=p, nbytes=need):
        return lib.ddr_feed_attr_mean_f32(table, stride, n_conus, A, active, N, flagged, n_flagged, fill, work, nbytes,
                                          None)

    for kw in ({"stride": -1}, {"n_conus": -1}, {"N": -1}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"negative" in lib.ddr_last_error(), kw
    assert run(A=65, stride=80) == _lib.DDR_ERR_ARG and b"n_attrs <= 64" in lib.ddr_last_error()
    assert run(stride=9) == _lib.DDR_ERR_ARG and b"row_stride" in lib.ddr_last_error()
    for n in (-1, 11):
        assert run(n_flagged=n) == _lib.DDR_ERR_ARG and b"n_flagged" in lib.ddr_last_error()
    for kw in ({"table": None}, {"active": None}, {"flagged": None}, {"fill": None}, {"work": None}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"null" in lib.ddr_last_error(), kw
    assert run(nbytes=need - 1) == _lib.DDR_ERR_ARG and b"work_bytes" in lib.ddr_last_error()
    assert run(work=p + 4) == _lib.DDR_ERR_ARG and b"aligned" in lib.ddr_last_error()
    assert run(n_flagged=0, flagged=None, work=None, nbytes=0) == _lib.DDR_OK  # every mean finite: nothing to do


def test_feed_flow_scale_refusals():
    lib = _lib.load()
    p = 4096

    def run(gage_c=p, rows=p, G=12, factors=p, skip=None, n_factors=20, N=300, winner=p, out=p):
        return lib.ddr_feed_flow_scale_f32(gage_c, rows, G, factors, skip, n_factors, N, winner, out, None)

    for kw in ({"G": -1}, {"n_factors": -1}, {"N": -1}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"negative" in lib.ddr_last_error(), kw
    for kw in ({"G": 2**31}, {"n_factors": 2**31}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"32-bit" in lib.ddr_last_error(), kw
    for kw in ({"gage_c": None}, {"rows": None}, {"factors": None}, {"winner": None}, {"out": None}):
        assert run(**kw) == _lib.DDR_ERR_ARG and b"null" in lib.ddr_last_error(), kw
    assert run(G=0, gage_c=None, rows=None, winner=None, out=None) == _lib.DDR_OK  # no gauges: nothing is launched
