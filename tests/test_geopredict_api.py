"""ddr_amd.geometry's predictor surface without a GPU: the attribute adapters, the output order against the header,
the C ABI's refusals, host tensors, config loading and the geopredict fixture."""

import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import PARAMS_DEFAULT, load_golden
from ddr_amd import _lib
from ddr_amd.geometry import (GEOMETRY_OUTPUTS, HYDROATLAS_TO_MERIT, MERIT_ATTRIBUTE_NAMES, AttributeMapping,
                              GeometryPredictor, adapt_attributes, compute_geometry_statistics, detect_source)
from ddr_amd.geometry.predictor import geometry_predict, prepare_attributes
from ddr_amd.nn import TorchKan, kan

HEADER = Path(__file__).resolve().parents[1] / "include" / "ddr_mc.h"
BRANCHES = ("discharge_lb", "slope_lb", "depth_lb", "side_slope_lb", "side_slope_ub", "bottom_width_lb")


def columns(names, n=4):
    return {name: np.full(n, float(i), dtype=np.float32) for i, name in enumerate(names)}


# ---- adapters ----
def test_detect_source():
    assert detect_source(columns(MERIT_ATTRIBUTE_NAMES)) == "merit"
    assert detect_source(columns(HYDROATLAS_TO_MERIT)) == "hydroatlas"
    assert detect_source(list(HYDROATLAS_TO_MERIT) + ["extra"]) == "hydroatlas"
    assert detect_source(columns(["foo", "bar"])) is None
    assert detect_source(columns(MERIT_ATTRIBUTE_NAMES[:-1])) is None
    # both complete: MERIT wins (it is checked first)
    assert detect_source(columns(list(MERIT_ATTRIBUTE_NAMES) + list(HYDROATLAS_TO_MERIT))) == "merit"


def test_mapping_table():
    assert len(MERIT_ATTRIBUTE_NAMES) == 10 and len(HYDROATLAS_TO_MERIT) == 10
    assert [m.merit_name for m in HYDROATLAS_TO_MERIT.values()] == list(MERIT_ATTRIBUTE_NAMES)
    logs = [k for k, m in HYDROATLAS_TO_MERIT.items() if m.log_transform]
    assert logs == ["upa_sk_smx"] and HYDROATLAS_TO_MERIT["upa_sk_smx"].merit_name == "log10_uparea"
    assert AttributeMapping("x") == AttributeMapping(merit_name="x", scale=1.0, offset=0.0, log_transform=False)
    with pytest.raises(Exception):  # frozen
        AttributeMapping("x").scale = 2.0


@pytest.mark.parametrize("source", ["auto", "merit"])
def test_adapt_merit_is_a_selection(source):
    cols = columns(list(reversed(MERIT_ATTRIBUTE_NAMES)) + ["COMID"])
    a = adapt_attributes(cols, source=source)
    assert tuple(a.columns) == MERIT_ATTRIBUTE_NAMES and a.source == "merit"
    for name in MERIT_ATTRIBUTE_NAMES:
        assert a.columns[name] is cols[name]
    assert a.scale.dtype == np.float64 and a.offset.dtype == np.float64 and a.log10.dtype == np.int32
    assert (a.scale == 1).all() and (a.offset == 0).all() and (a.log10 == 0).all()


@pytest.mark.parametrize("source", ["auto", "hydroatlas"])
def test_adapt_hydroatlas_order_and_transform(source):
    cols = columns(sorted(HYDROATLAS_TO_MERIT))
    a = adapt_attributes(cols, source=source)
    assert tuple(a.columns) == MERIT_ATTRIBUTE_NAMES and a.source == "hydroatlas"
    for src, m in HYDROATLAS_TO_MERIT.items():
        assert a.columns[m.merit_name] is cols[src]  # untransformed: the kernel converts
    j = MERIT_ATTRIBUTE_NAMES.index("log10_uparea")
    assert a.log10.tolist() == [int(i == j) for i in range(10)]
    assert (a.scale == 1).all() and (a.offset == 0).all()


def test_adapt_errors():
    with pytest.raises(ValueError, match="Cannot auto-detect attribute source") as e:
        adapt_attributes(columns(["foo", "bar"]))
    assert "'bar', 'foo'" in str(e.value) and "hydroatlas" in str(e.value)
    with pytest.raises(ValueError, match="Unknown attribute source: 'nhdplus'"):
        adapt_attributes(columns(MERIT_ATTRIBUTE_NAMES), source="nhdplus")
    with pytest.raises(ValueError, match=r"Missing MERIT attributes: \['NDVI', 'Porosity'\]"):
        adapt_attributes(columns([n for n in MERIT_ATTRIBUTE_NAMES if n not in ("NDVI", "Porosity")]), source="merit")
    with pytest.raises(ValueError, match=r"Missing hydroatlas attributes: \['upa_sk_smx'\]"):
        adapt_attributes(columns([n for n in HYDROATLAS_TO_MERIT if n != "upa_sk_smx"]), source="hydroatlas")


# ---- the header ----
def test_geometry_outputs_match_header():
    text = HEADER.read_text()
    body = re.search(r"enum\s*\{([^}]*DDR_GEOM_[^}]*)\}", text).group(1)
    names = [m.lower() for m in re.findall(r"DDR_GEOM_([A-Z0-9_]+)", body)]
    assert tuple(names) == GEOMETRY_OUTPUTS
    assert len(GEOMETRY_OUTPUTS) == 11
    assert re.search(r"DDR_GEOM_DEPTH\s*=\s*0\b", body) and body.rstrip().rstrip(",").split()[-1] == "DDR_N_GEOM"
    assert compute_geometry_statistics.__module__ == "ddr_amd.geometry.statistics"


# ---- the C ABI, refused before any launch ----
def slot(column, log_space=0, lo=0.0, hi=1.0, value=0.0):
    return _lib.GeomSlot(column, log_space, lo, hi, value)


def test_c_abi_prepare_refuses_bad_arguments():
    lib = _lib.load()
    p = 4096  # (never dereferenced: every call below is refused, or a no-op)
    call = lib.ddr_attr_prepare_f32
    assert call(0, 10, None, 0, None, None, None, None, None, None, None, None, None, None) == _lib.DDR_OK
    assert call(0, 10, p, 0, p, p, p, p, p, p, p, p, p, None) == _lib.DDR_OK
    for N, stride in ((-1, 10), (5, -1)):
        assert call(N, 10, p, stride, p, p, p, p, p, None, None, p, None, None) == _lib.DDR_ERR_ARG
        assert b"negative" in lib.ddr_last_error()
    for F in (0, -3, 33, 1 << 20):
        assert call(5, F, p, 5, p, p, p, p, p, None, None, p, None, None) == _lib.DDR_ERR_ARG
        assert b"n_features <= 32" in lib.ddr_last_error()
    assert call(0, 33, p, 5, p, p, p, p, p, None, None, p, None, None) == _lib.DDR_ERR_ARG
    for k in range(7):  # raw, scale, offset, log10_flag, mean, std, x
        a = [p] * 7
        a[k] = None
        raw, sc, of, lg, mean, std, x = a
        assert call(5, 10, raw, 5, sc, of, lg, mean, std, None, None, x, None, None) == _lib.DDR_ERR_ARG
        assert b"null" in lib.ddr_last_error()
    for p10, p90 in ((p, None), (None, p)):
        assert call(5, 10, p, 5, p, p, p, p, p, p10, p90, p, p, None) == _lib.DDR_ERR_ARG
        assert b"together" in lib.ddr_last_error()
    assert call(5, 10, p, 5, p, p, p, p, p, p, p, p, None, None) == _lib.DDR_ERR_ARG
    assert b"counts" in lib.ddr_last_error()
    assert call(5, 10, p, 4, p, p, p, p, p, None, None, p, None, None) == _lib.DDR_ERR_ARG
    assert b"feat_stride" in lib.ddr_last_error()
    assert call(1 << 39, 10, p, 1 << 39, p, p, p, p, p, None, None, p, None, None) == _lib.DDR_ERR_ARG
    assert b"too many rows" in lib.ddr_last_error()


def test_c_abi_geometry_refuses_bad_arguments():
    lib = _lib.load()
    p = 4096
    sn, sq, sp = slot(0, 0, 0.015, 0.25), slot(1), slot(2, 1, 1.0, 200.0)
    by = C.byref

    def call(N, O, u, a, b, c, Q, S, out, stride):
        return lib.ddr_geometry_predict_f32(N, O, u, a, b, c, Q, S, 1e-4, 1e-3, 0.01, 0.01, out, stride, None)

    assert call(0, 3, None, by(sn), by(sq), by(sp), None, None, None, 0) == _lib.DDR_OK
    assert call(0, 3, p, by(sn), by(sq), by(sp), p, p, p, 0) == _lib.DDR_OK
    for N, stride in ((-1, 5), (5, -1)):
        assert call(N, 3, p, by(sn), by(sq), by(sp), p, p, p, stride) == _lib.DDR_ERR_ARG
        assert b"negative" in lib.ddr_last_error()
    for O in (0, -1, 9):
        assert call(5, O, p, by(sn), by(sq), by(sp), p, p, p, 5) == _lib.DDR_ERR_ARG
        assert b"n_outputs <= 8" in lib.ddr_last_error()
    # a column outside u
    for bad in (slot(3), slot(8), slot(-2)):
        for k in range(3):
            s = [sn, sq, sp]
            s[k] = bad
            assert call(5, 3, p, by(s[0]), by(s[1]), by(s[2]), p, p, p, 5) == _lib.DDR_ERR_ARG
            assert b"outside u" in lib.ddr_last_error()
    assert call(5, 2, p, by(sn), by(sq), by(sp), p, p, p, 5) == _lib.DDR_ERR_ARG  # p_spatial's column 2 of O = 2
    assert b"p_spatial" in lib.ddr_last_error()
    # n and q_spatial have no default; p_spatial has
    assert call(5, 3, p, by(slot(-1)), by(sq), by(sp), p, p, p, 5) == _lib.DDR_ERR_ARG
    assert b"n has no default" in lib.ddr_last_error()
    assert call(5, 3, p, by(sn), by(slot(-1)), by(sp), p, p, p, 5) == _lib.DDR_ERR_ARG
    assert b"q_spatial has no default" in lib.ddr_last_error()
    assert call(0, 2, p, by(sn), by(sq), by(slot(-1, value=21.0)), p, p, p, 0) == _lib.DDR_OK
    # null pointers
    assert call(5, 3, p, None, by(sq), by(sp), p, p, p, 5) == _lib.DDR_ERR_ARG
    assert b"null slot" in lib.ddr_last_error()
    for u, out in ((None, p), (p, None)):
        assert call(5, 3, u, by(sn), by(sq), by(sp), p, p, out, 5) == _lib.DDR_ERR_ARG
        assert b"null" in lib.ddr_last_error()
    for Q, S in ((None, p), (p, None)):
        assert call(5, 3, p, by(sn), by(sq), by(sp), Q, S, p, 5) == _lib.DDR_ERR_ARG
        assert b"discharge or slope" in lib.ddr_last_error()
    assert call(5, 3, p, by(sn), by(sq), by(sp), p, p, p, 4) == _lib.DDR_ERR_ARG
    assert b"out_stride" in lib.ddr_last_error()
    assert call(1 << 39, 3, p, by(sn), by(sq), by(sp), p, p, p, 1 << 39) == _lib.DDR_ERR_ARG
    assert b"too many rows" in lib.ddr_last_error()


# ---- the predictor on the host ----
NAMES = list(MERIT_ATTRIBUTE_NAMES)
KAN_CFG = dict(hidden_size=5, input_var_names=NAMES, num_hidden_layers=2, learnable_parameters=["n", "q_spatial", "p_spatial"],
               grid=4, k=2)


def host_predictor(learn=("n", "q_spatial", "p_spatial"), **kw):
    net = kan(NAMES, list(learn), 5, 1, 3, 2, 0)
    return GeometryPredictor(net, NAMES, torch.zeros(10), torch.ones(10), device="cpu", **PARAMS_DEFAULT, **kw)


def test_host_tensors_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_library)
    gp = host_predictor()
    z = torch.zeros
    with pytest.raises(RuntimeError, match="HIP device only"):
        gp.predict(z(10, 4), z(4), z(4))
    with pytest.raises(RuntimeError, match="HIP device only"):
        gp.predict(columns(NAMES), np.zeros(4, np.float32), np.zeros(4, np.float32))
    with pytest.raises(RuntimeError, match="HIP device only"):
        gp.predict_parameters(z(10, 4))
    with pytest.raises(RuntimeError, match="HIP device only"):
        gp.predict_statistics(None, z(3, 4), z(10, 4), z(4))
    f = lambda n, dt: z(n, dtype=dt)  # noqa: E731
    with pytest.raises(RuntimeError, match="HIP device only"):
        prepare_attributes(z(10, 4), f(10, torch.float64), f(10, torch.float64), f(10, torch.int32), z(10), z(10))
    with pytest.raises(RuntimeError, match="HIP device only"):
        geometry_predict(z(4, 3), gp._slots, z(4), z(4))


def test_constructor_refusals():
    with pytest.raises(ValueError, match="'q_spatial'"):
        host_predictor(learn=("n", "p_spatial"))
    with pytest.raises(ValueError, match="'n'"):
        host_predictor(learn=("q_spatial", "p_spatial"))
    with pytest.raises(TypeError, match="ddr_amd.nn.kan"):
        GeometryPredictor(TorchKan(NAMES, ["n", "q_spatial"], 5, 1, 3, 2, 0), NAMES, torch.zeros(10), torch.ones(10),
                          device="cpu", **PARAMS_DEFAULT)
    net = kan(NAMES, ["n", "q_spatial"], 5, 1, 3, 2, 0)
    with pytest.raises(ValueError, match="10 attributes"):
        GeometryPredictor(net, NAMES[:9], torch.zeros(9), torch.ones(9), device="cpu", **PARAMS_DEFAULT)
    with pytest.raises(ValueError, match="chunk_rows"):
        host_predictor(chunk_rows=0)
    # p_spatial not learned: the default (predictor.py:307-316), the reference's 21 when the config has none
    gp = host_predictor(learn=("n", "q_spatial"))
    assert gp._slots[2].column == -1 and gp._slots[2].value == 21.0
    assert [s.column for s in host_predictor(learn=("p_spatial", "q_spatial", "n"))._slots] == [2, 1, 0]
    assert [s.log_space for s in host_predictor()._slots] == [0, 0, 1]


def test_config_mapping_and_yaml_build_identical_predictors(tmp_path):
    import yaml

    model = TorchKan(NAMES, KAN_CFG["learnable_parameters"], 5, 2, 4, 2, seed=7)
    ckpt = tmp_path / "weights.pt"
    torch.save({"model_state_dict": model.state_dict(), "epoch": 3, "mini_batch": 0}, ckpt)
    rng = np.random.default_rng(0)
    stats = {a: {"mean": float(rng.normal()), "std": float(rng.uniform(0.5, 2)), "p10": -1.5 + i, "p90": 1.5 + i,
                 "min": -9.0, "max": 9.0} for i, a in enumerate(NAMES + ["unused"])}
    (tmp_path / "stats.json").write_text(json.dumps(stats))
    config = {"seed": 42, "kan": KAN_CFG,
              "params": {"parameter_ranges": {"n": [0.02, 0.2], "q_spatial": [0.0, 1.0], "p_spatial": [1.0, 200.0]},
                         "log_space_parameters": ["p_spatial"], "attribute_minimums": {"discharge": 1e-3, "slope": 1e-4}}}
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(config))
    a = GeometryPredictor.from_checkpoint(ckpt, config, stats_path=tmp_path / "stats.json", device="cpu")
    b = GeometryPredictor.from_checkpoint(ckpt, tmp_path / "config.yaml", stats_path=str(tmp_path / "stats.json"),
                                          device="cpu", chunk_rows=128, check_distribution=False)
    for gp in (a, b):
        assert gp.attribute_names == NAMES
        assert torch.equal(gp._nn.flat, model.flat) and torch.equal(gp._nn.consts, model.consts)
        assert gp._means.tolist() == [np.float32(stats[n]["mean"]) for n in NAMES]
        assert gp._stds.tolist() == [np.float32(stats[n]["std"]) for n in NAMES]
        assert gp._p10.tolist() == [-1.5 + i for i in range(10)] and gp._p90.tolist() == [1.5 + i for i in range(10)]
        assert gp._parameter_ranges["n"] == [0.02, 0.2]
        assert gp._defaults == {"p_spatial": 21}  # (missing from the config: the reference's default)
        assert gp._attribute_minimums == {"discharge": 1e-3, "slope": 1e-4}
    for sa, sb in zip(a._slots, b._slots):
        assert bytes(sa) == bytes(sb)
    assert (a.chunk_rows, a.check_distribution, b.chunk_rows, b.check_distribution) == (1 << 20, True, 128, False)
    with pytest.raises(FileNotFoundError, match="stats_path"):
        GeometryPredictor.from_checkpoint(ckpt, config, device="cpu")
    del stats["NDVI"]
    (tmp_path / "stats.json").write_text(json.dumps(stats))
    with pytest.raises(KeyError, match="NDVI"):
        GeometryPredictor.from_checkpoint(ckpt, config, stats_path=tmp_path / "stats.json", device="cpu")


# ---- the fixture ----
def test_fixture_holds_every_key():
    d = load_golden("geopredict")
    N, F = 300, 10
    assert tuple(d["outputs"]) == GEOMETRY_OUTPUTS and tuple(d["branches"]) == BRANCHES
    assert tuple(d["names_merit"]) == MERIT_ATTRIBUTE_NAMES and tuple(d["names_hydroatlas"]) == tuple(HYDROATLAS_TO_MERIT)
    for key in ("raw_merit", "raw_hydroatlas"):
        assert d[key].shape == (F, N) and d[key].dtype == np.float32
        assert np.isnan(d[key]).any(axis=1).all() and np.isnan(d[key][:, 7]).all()
        assert np.isposinf(d[key]).sum() == 1 and np.isneginf(d[key]).sum() == 1
    area = d["raw_hydroatlas"][MERIT_ATTRIBUTE_NAMES.index("log10_uparea")]
    assert (area <= 0).sum() >= 4 and ((area > 0) & (area < 1e-6)).sum() >= 4  # the log10 clip is active
    for key in ("mean", "std", "p10", "p90"):
        assert d[key].shape == (F,) and d[key].dtype == np.float32
    assert d["x_ref"].shape == (N, F) and d["x_ref"].dtype == np.float32
    assert d["counts"].shape == (3, F) and d["counts"].dtype == np.int64 and (d["counts"] > 0).all()
    assert d["bounds"].shape == (3, 2) and d["minimums"].shape == (4,)
    lo = int(np.ceil(0.05 * N))
    for tag, O in (("", 3), ("_o2", 2)):
        assert d["u" + tag].shape == (N, O) and d["u" + tag].dtype == np.float32
        for key in ("discharge", "slope"):
            assert d[key + tag].shape == (N,) and d[key + tag].dtype == np.float32
        assert np.isnan(d["slope" + tag]).sum() == 3 and np.isnan(d["discharge" + tag]).sum() == 2
        assert d["ref64" + tag].shape == (11, N) and d["ref64" + tag].dtype == np.float64
        assert d["ref32" + tag].shape == (11, N) and d["ref32" + tag].dtype == np.float32
        assert d["e32" + tag].shape == (11,) and (d["e32" + tag] < 1e-4).all()
        # every clamp is active and inactive on at least 5 % of the reaches
        counts, n_ok = d["branch_counts" + tag], int(d["n_finite" + tag])
        assert counts.shape == (6,) and (counts >= lo).all() and (n_ok - counts >= lo).all(), (tag, counts, n_ok)
        # a NaN slope or discharge: finite n / p / q beside NaN geometry
        bad = np.isnan(d["slope" + tag]) | np.isnan(d["discharge" + tag])
        assert np.isnan(d["ref64" + tag][:8, bad]).all() and np.isfinite(d["ref64" + tag][8:, bad]).all()
    assert (d["ref64_o2"][GEOMETRY_OUTPUTS.index("p_spatial")] == 21.0).all()
    assert int(d["seed_o2"]) == 23 and d["arch_o2"].tolist() == [11, 1, 3, 3]
