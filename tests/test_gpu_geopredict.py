"""The geometry predictor's kernels (csrc/geopredict.hip) and ``ddr_amd.geometry.GeometryPredictor`` on the device,
against the fixture ``geopredict.npz`` (the reference's own functions in fp64, tests/golden/make_geopredict_golden.py).

Bars.  ``attr_prepare_kernel``: bitwise on an identity feature (an fp32 subtraction and an IEEE division leave no
freedom), one fp32 ulp of the converted value on the log10 feature (the device's fp64 log10 may differ from
NumPy's in the last bit before the rounding to fp32), integer counters exact.  ``geometry_predict_kernel``: per
output row the max relative error against ``ref64`` over its finite values is at most max(4 e32, 2^-20), with
e32 the fixture's measured error of the reference's own fp32 run and 2^-20 = 8 fp32 ulp (about twice the 4.6e-7
this project measured for its faithful fp32 geometry against the reference's golden).  Every figure is printed
(``pytest -s``).

Measured on an MI355X (N = 300; max relative error, and in brackets the reference's own fp32 error e32):

    prepare, HydroATLAS naming: 0 of 300 log10 values differ from NumPy's; everything else is bitwise
    geometry kernel               published checkpoint (O = 3)    seeded KAN (O = 2, p_spatial = 21)
      depth                       5.25e-07 (5.25e-07)             7.10e-07 (7.10e-07)
      top_width                   2.96e-07 (2.96e-07)             3.65e-07 (3.65e-07)
      bottom_width                2.74e-06 (2.74e-06)             9.89e-07 (9.89e-07)
      side_slope                  3.61e-07 (2.54e-07)             2.49e-07 (2.49e-07)
      cross_sectional_area        6.64e-07 (6.64e-07)             8.74e-07 (8.74e-07)
      wetted_perimeter            5.27e-07 (5.27e-07)             6.85e-07 (6.85e-07)
      hydraulic_radius            3.36e-07 (3.36e-07)             4.91e-07 (4.91e-07)
      velocity                    4.34e-07 (4.34e-07)             4.76e-07 (4.76e-07)
      n                           7.86e-08 (7.86e-08)             8.24e-08 (8.24e-08)
      p_spatial                   1.56e-07 (1.56e-07)             0 (0)
      q_spatial                   0 (0)                           0 (0)
    end to end (HIP KAN): geometry at the KAN's own u <= 9.8e-07 (cross_sectional_area); n / p_spatial / q_spatial
    against the fp64 model 2.7e-07 / 3.9e-07 / 1.3e-07 with the KAN's output bar du = 2.5e-07 (fused KAN 6.2e-08)
"""

import logging

import numpy as np
import pytest
import torch

from conftest import load_golden
from ddr_amd import _lib
from ddr_amd.geometry import GEOMETRY_OUTPUTS, GeometryPredictor, compute_trapezoidal_geometry
from ddr_amd.geometry.predictor import geometry_predict, prepare_attributes
from ddr_amd.geometry.statistics import geometry_statistics_from_inflow
from ddr_amd.graph import RiverGraph
from ddr_amd.nn import TorchKan, kan
from ddr_amd.routing.utils import denormalize

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
LOG10_FEATURE = 6
NAMINGS = ("merit", "hydroatlas")
LEARN = {"": ["n", "q_spatial", "p_spatial"], "_o2": ["n", "q_spatial"]}
LOG_SPACE = ["p_spatial"]


@pytest.fixture(scope="module")
def fx():
    return load_golden("geopredict")


def mins_of(d):
    return dict(zip(("discharge", "slope", "depth", "bottom_width"), d["minimums"].tolist()))


def ranges_of(d):
    return dict(zip(("n", "q_spatial", "p_spatial"), d["bounds"].tolist()))


def torch_model(d, tag):
    """The fixture's network as a TorchKan on the host (fp32 parameters)."""
    names = [str(s) for s in d["names_merit"]]
    if tag == "":
        m = TorchKan(names, LEARN[tag], 21, 2, 50, 2, 0)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in load_golden("kan_merit").items()})
    else:
        H, L, G, k = d["arch_o2"].tolist()
        m = TorchKan(names, LEARN[tag], H, L, G, k, int(d["seed_o2"]))
    return m


def predictor(d, cuda, tag="", **kw):
    m = torch_model(d, tag)
    net = kan([str(s) for s in d["names_merit"]], LEARN[tag], m.hidden_size, m.num_hidden_layers, m.grid_size, m.k, 0,
              device=cuda)
    with torch.no_grad():
        net.flat.copy_(m.flat)
        net.consts.copy_(m.consts)
    names = [str(s) for s in d["names_merit"]]
    stats = {a: {"p10": float(d["p10"][i]), "p90": float(d["p90"][i])} for i, a in enumerate(names)}
    return GeometryPredictor(net, names, torch.from_numpy(d["mean"]), torch.from_numpy(d["std"]), ranges_of(d), LOG_SPACE,
                             {"p_spatial": float(d["default_p_o2"])}, mins_of(d), stats_ranges=stats, device=cuda, **kw)


def attrs_of(d, naming, rows=None):
    names = d[f"names_{naming}"]
    return {str(a): d[f"raw_{naming}"][i][:rows] for i, a in enumerate(names)}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def same_bits(a, b) -> bool:
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def transform(naming, cuda):
    F = 10
    lg = torch.zeros(F, dtype=torch.int32)
    if naming == "hydroatlas":
        lg[LOG10_FEATURE] = 1
    return (torch.ones(F, dtype=torch.float64, device=cuda), torch.zeros(F, dtype=torch.float64, device=cuda),
            lg.to(cuda))


# ---- attr_prepare_kernel ----
@pytest.mark.parametrize("rows", [300, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("naming", NAMINGS)
def test_prepare_kernel(cuda, fx, naming, rows):
    d = fx
    raw = torch.from_numpy(d[f"raw_{naming}"]).to(cuda)[:, :rows]  # (rows of a (F, 300) tensor: feat_stride = 300)
    dev = lambda k: torch.from_numpy(d[k]).to(cuda)  # noqa: E731
    counts = torch.zeros((3, 10), dtype=torch.int64, device=cuda)
    x = prepare_attributes(raw, *transform(naming, cuda), dev("mean"), dev("std"), dev("p10"), dev("p90"), counts)
    x, ref = x.cpu().numpy(), d["x_ref"][:rows]
    assert x.shape == (rows, 10)
    exact = np.ones(10, dtype=bool)
    if naming == "hydroatlas":
        exact[LOG10_FEATURE] = False
        # one ulp of the converted value v = x std + mean, carried through (v - mean) / std, plus x's own rounding
        xr = ref[:, LOG10_FEATURE].astype(np.float64)
        std, mean = float(d["std"][LOG10_FEATURE]), float(d["mean"][LOG10_FEATURE])
        tol = np.spacing(np.abs(xr * std + mean).astype(np.float32)).astype(np.float64) / std + np.spacing(np.abs(ref[:, LOG10_FEATURE]))
        got = x[:, LOG10_FEATURE]
        differ = int((got.view(np.int32) != ref[:, LOG10_FEATURE].view(np.int32)).sum())
        print(f"[prepare {naming} rows={rows}] log10 feature: {differ} of {rows} elements differ from NumPy's")
        assert np.array_equal(np.isnan(got), np.isnan(xr))
        assert (np.abs(got.astype(np.float64) - xr) <= tol)[~np.isnan(xr)].all()
    assert np.array_equal(x[:, exact].view(np.int32), ref[:, exact].view(np.int32))
    # the counters: exact (recounted for a slice of the fixture)
    v = d["raw_merit"][:, :rows]
    with np.errstate(invalid="ignore"):
        want = np.stack([np.isnan(v).sum(1), (v < d["p10"][:, None]).sum(1), (v > d["p90"][:, None]).sum(1)])
    if rows == 300:
        assert np.array_equal(want, d["counts"])
    assert np.array_equal(counts.cpu().numpy(), want)
    # without ranges only the fills are counted; without counters nothing is
    counts.zero_()
    x2 = prepare_attributes(raw, *transform(naming, cuda), dev("mean"), dev("std"), counts=counts)
    assert np.array_equal(counts.cpu().numpy(), np.stack([want[0], 0 * want[1], 0 * want[2]]))
    x3 = prepare_attributes(raw.contiguous(), *transform(naming, cuda), dev("mean"), dev("std"))
    assert np.array_equal(x2.cpu().numpy().view(np.int32), x.view(np.int32))
    assert np.array_equal(x3.cpu().numpy().view(np.int32), x.view(np.int32))


# ---- geometry_predict_kernel ----
def slots_of(d, tag):
    r = ranges_of(d)
    learn = LEARN[tag]
    out = []
    for name in ("n", "q_spatial", "p_spatial"):
        if name in learn:
            out.append(_lib.GeomSlot(learn.index(name), int(name in LOG_SPACE), r[name][0], r[name][1], 0.0))
        else:
            out.append(_lib.GeomSlot(-1, 0, 0.0, 0.0, float(d["default_p_o2"])))
    return out


def check_geometry(out, ref64, e32, tag, extra=None):
    """Per row: NaN where ref64 is NaN, and max-rel over the finite reference values <= max(4 e32, 2^-20) (+ extra)."""
    failures = []
    for k, name in enumerate(GEOMETRY_OUTPUTS):
        fin = np.isfinite(ref64[k])
        assert np.isnan(out[k][np.isnan(ref64[k])]).all(), name
        assert np.isfinite(out[k][fin]).all(), name
        err = float(np.max(np.abs(out[k][fin].astype(np.float64) - ref64[k][fin]) / np.abs(ref64[k][fin])))
        bar = max(4.0 * float(e32[k]), FLOOR) + (0.0 if extra is None else float(extra[k]))
        print(f"[{tag}] {name:22s} max-rel {err:.2e}  reference fp32 {float(e32[k]):.2e}  bar {bar:.2e}")
        if not err <= bar:
            failures.append((name, err, bar))
    assert not failures, failures


@pytest.mark.parametrize("tag", ["", "_o2"], ids=["published", "default_p"])
def test_geometry_kernel(cuda, fx, tag):
    d = fx
    u = torch.from_numpy(d["u" + tag]).to(cuda)
    Q, S = torch.from_numpy(d["discharge" + tag]).to(cuda), torch.from_numpy(d["slope" + tag]).to(cuda)
    slots, mins = slots_of(d, tag), mins_of(d)
    full = geometry_predict(u, slots, Q, S, mins)
    out, ref64 = full.cpu().numpy(), d["ref64" + tag]
    assert out.shape == (11, 300)
    check_geometry(out, ref64, d["e32" + tag], "geometry" + tag)
    r = dict(zip(GEOMETRY_OUTPUTS, out))
    w = dict(zip(GEOMETRY_OUTPUTS, ref64))
    # a NaN slope or discharge: NaN geometry beside finite parameters; parameters finite wherever u is
    bad = np.isnan(d["slope" + tag]) | np.isnan(d["discharge" + tag])
    assert bad.sum() == 5 and np.isnan(out[:8, bad]).all()
    assert np.isfinite(out[8:, np.isfinite(d["u" + tag]).all(1)]).all()
    # clamped reaches sit exactly on their bound
    for name, bound in (("side_slope", 0.5), ("side_slope", 50.0), ("bottom_width", mins["bottom_width"]),
                        ("depth", mins["depth"])):
        on = w[name] == bound
        assert on.sum() >= 15 and (r[name][on] == np.float32(bound)).all(), (name, bound)
    if tag == "_o2":
        assert (r["p_spatial"] == np.float32(21.0)).all()
    # parameters only: the same bits as the full call's rows
    par = geometry_predict(u, slots, None, None, mins)
    assert par.shape == (3, 300) and same_bits(par, full[8:])
    # another launch, the same bits
    assert same_bits(geometry_predict(u, slots, Q, S, mins), full)


# ---- GeometryPredictor ----
def reference_from_u(d, u64: torch.Tensor, tag, Q, S):
    """predictor.py:203-238 + 276-318 in fp64 with this package's drop-ins of the reference's functions (pinned to
    it by tests/test_trapezoidal.py and the golden tests): (11, N)."""
    r, mins, learn = ranges_of(d), mins_of(d), LEARN[tag]
    par = {k: denormalize(u64[:, learn.index(k)], r[k], k in LOG_SPACE) if k in learn
           else torch.full_like(u64[:, 0], float(d["default_p_o2"])) for k in ("n", "q_spatial", "p_spatial")}
    geo = compute_trapezoidal_geometry(par["n"], par["p_spatial"], par["q_spatial"],
                                       torch.clamp(torch.from_numpy(Q).double(), min=mins["discharge"]),
                                       torch.clamp(torch.from_numpy(S).double(), min=mins["slope"]),
                                       depth_lb=mins["depth"], bottom_width_lb=mins["bottom_width"])
    geo = dict(geo, **par)
    return torch.stack([geo[k] for k in GEOMETRY_OUTPUTS]).numpy()


def stack_u(model, x):
    o = model(inputs=x)
    return torch.stack([o[k] for k in model.learnable_parameters], dim=1).contiguous()


@pytest.mark.parametrize("naming", NAMINGS)
def test_end_to_end(cuda, fx, naming, caplog):
    d, tag = fx, ""
    gp = predictor(d, cuda)
    Q, S = d["discharge"], d["slope"]
    with caplog.at_level(logging.INFO, logger="ddr_amd.geometry"):
        got = gp.predict(attrs_of(d, naming), Q, S)
    assert tuple(got) == GEOMETRY_OUTPUTS and all(v.shape == (300,) and v.device == cuda for v in got.values())
    full = torch.stack([got[k] for k in GEOMETRY_OUTPUTS])
    # the counters, and the reference's two messages
    assert gp.last_counts == {k: {str(a): int(d["counts"][i, j]) for j, a in enumerate(d["names_merit"])}
                              for i, k in enumerate(("filled", "below", "above"))}
    text = caplog.text
    assert f"Attribute NDVI: filled {int(d['counts'][0, 4])} NaN values with training mean" in text
    assert (f"Attribute NDVI: {int(d['counts'][1, 4])}/300 values below training p10 ({float(d['p10'][4]):.3f}), "
            f"{int(d['counts'][2, 4])}/300 above training p90 ({float(d['p90'][4]):.3f})") in text
    # bitwise the three device stages called one by one
    dev = lambda k: torch.from_numpy(d[k]).to(cuda)  # noqa: E731
    raw = torch.from_numpy(d[f"raw_{naming}"]).to(cuda)
    x = prepare_attributes(raw, *transform(naming, cuda), dev("mean"), dev("std"))
    with torch.no_grad():
        u = stack_u(gp._nn, x)
    staged = geometry_predict(u, slots_of(d, tag), torch.from_numpy(Q).to(cuda), torch.from_numpy(S).to(cuda), mins_of(d))
    assert same_bits(full, staged)
    # rows without an infinite attribute (whose KAN output is NaN in the model and unspecified on the device)
    ok = np.isfinite(x.cpu().numpy()).all(1)
    assert (~ok).sum() == 2
    out = full.cpu().numpy()[:, ok]
    # (a) the geometry of the HIP KAN's own u: the kernel's bars
    ref_u = reference_from_u(d, u.cpu().double(), tag, Q, S)[:, ok]
    check_geometry(out, ref_u, d["e32"], f"end to end {naming}, at the HIP KAN's u")
    # (b) the parameters against the fp64 model (TorchKan fp64 on the same x): the kernel's bar plus test_gpu_kan's
    # output bar du = max(4 e32_kan, 2e-7) (max-abs in u; e32_kan: TorchKan in fp32 on the GPU against the fp64
    # model) carried through denormalize: |d theta| <= du (hi - lo) for a linear slot, and
    # |d p| / p <= expm1(du (log hi - log(lo + 1e-6))) for the log-space slot
    m = torch_model(d, tag)
    with torch.no_grad():
        u32 = stack_u(m.to(cuda), x).cpu().double()
        u64 = stack_u(m.cpu().double(), x.cpu().double())
    okt = torch.from_numpy(ok)
    du = max(4.0 * float((u32 - u64)[okt].abs().max()), 2e-7)
    print(f"[end to end {naming}] KAN output bar du = {du:.2e}; fused max-abs {float((u.cpu().double() - u64)[okt].abs().max()):.2e}")
    ref_m = reference_from_u(d, u64, tag, Q, S)[:, ok]
    r = ranges_of(d)
    extra = np.zeros(11)
    for name in ("n", "q_spatial", "p_spatial"):
        k = GEOMETRY_OUTPUTS.index(name)
        lo, hi = r[name]
        if name in LOG_SPACE:
            extra[k] = np.expm1(du * (np.log(hi) - np.log(lo + 1e-6)))
        else:
            extra[k] = du * (hi - lo) / float(np.min(np.abs(ref_m[k])))
    for k in range(8, 11):
        err = float(np.max(np.abs(out[k] - ref_m[k]) / np.abs(ref_m[k])))
        bar = max(4.0 * float(d["e32"][k]), FLOOR) + extra[k]
        print(f"[end to end {naming}] {GEOMETRY_OUTPUTS[k]:10s} vs the fp64 model: max-rel {err:.2e}  bar {bar:.2e}")
        assert err <= bar, GEOMETRY_OUTPUTS[k]
    if naming == "merit":  # x is x_ref bitwise: the fp64 model's u is the fixture's, so its parameters are ref64's
        assert np.allclose(ref_m[8:], d["ref64"][8:, ok], rtol=1e-6, atol=0)
    # predict_parameters: the same three rows
    n, p, q = gp.predict_parameters(attrs_of(d, naming))
    assert same_bits(torch.stack([n, p, q]), full[8:])


def test_chunks_runs_and_device_attributes_are_bitwise(cuda, fx):
    d, N = fx, 257
    Q, S = torch.from_numpy(d["discharge"][:N]).to(cuda), torch.from_numpy(d["slope"][:N]).to(cuda)
    attrs = attrs_of(d, "hydroatlas", N)
    outs = []
    for chunk in (64, 100, N, N):
        gp = predictor(d, cuda, chunk_rows=chunk)
        outs.append(torch.stack(list(gp.predict(attrs, Q, S).values())))
        assert gp.last_counts is not None
    quiet = predictor(d, cuda, chunk_rows=100, check_distribution=False)
    outs.append(torch.stack(list(quiet.predict(attrs, Q, S).values())))
    assert quiet.last_counts is None
    for o in outs[1:]:
        assert same_bits(o, outs[0])
    # a device tensor (F, N) in attribute_names order is the MERIT mapping's result; array-like discharge too
    gp = predictor(d, cuda, chunk_rows=64)
    a = torch.stack(list(gp.predict(attrs_of(d, "merit", N), d["discharge"][:N], d["slope"][:N]).values()))
    counts = gp.last_counts
    b = torch.stack(list(gp.predict(torch.from_numpy(d["raw_merit"][:, :N].copy()).to(cuda), Q, S).values()))
    c = torch.stack(list(gp.predict(torch.from_numpy(d["raw_merit"]).to(cuda)[:, :N], Q, S, source="merit").values()))
    assert same_bits(a, b) and same_bits(a, c) and gp.last_counts == counts


def test_default_p_spatial_end_to_end(cuda, fx):
    d, tag = fx, "_o2"
    gp = predictor(d, cuda, tag)
    Q, S = d["discharge_o2"], d["slope_o2"]
    got = gp.predict(attrs_of(d, "merit"), Q, S)
    assert bool((got["p_spatial"] == 21.0).all())
    full = torch.stack(list(got.values()))
    x = torch.from_numpy(d["x_ref"]).to(cuda)
    with torch.no_grad():
        u = stack_u(gp._nn, x)
    ok = np.isfinite(d["x_ref"]).all(1)
    check_geometry(full.cpu().numpy()[:, ok], reference_from_u(d, u.cpu().double(), tag, Q, S)[:, ok], d["e32_o2"],
                   "end to end, default p_spatial")
    n, p, q = gp.predict_parameters(attrs_of(d, "merit"))
    assert same_bits(torch.stack([n, p, q]), full[8:])


def test_predict_statistics(cuda, fx):
    d, t = fx, load_golden("tree300")
    N, D = int(t["n"]), 31
    assert N == 300
    from ddr_amd import synthetic

    q_daily = torch.from_numpy(synthetic.lateral_inflow(N, D, 44)).to(cuda)
    g = RiverGraph(N, t["rows"], t["cols"], max_block_reaches=400, target_blocks=1 << 20)
    gp = predictor(d, cuda)
    attrs, slope = attrs_of(d, "hydroatlas"), t["slope"]  # (about half of it below the 1e-3 minimum)
    assert 15 <= (slope < 1e-3).sum() <= 285
    got = gp.predict_statistics(g, q_daily, attrs, slope)
    n, p, q = gp.predict_parameters(attrs)
    want = geometry_statistics_from_inflow(g, q_daily, n, p, q, torch.from_numpy(np.maximum(slope, np.float32(1e-3))).to(cuda),
                                           mins_of(d))
    assert set(got) == set(want) and len(got) == 24
    for k, v in want.items():
        assert got[k].shape == (N,) and np.array_equal(got[k].view(np.int32), v.view(np.int32)), k


def test_refusals(cuda, fx):
    d = fx
    gp = predictor(d, cuda)
    raw = torch.from_numpy(d["raw_merit"]).to(cuda)
    Q, S = torch.from_numpy(d["discharge"]).to(cuda), torch.from_numpy(d["slope"]).to(cuda)
    with pytest.raises(RuntimeError, match="HIP device only"):
        gp.predict(raw.cpu(), Q, S)
    with pytest.raises(RuntimeError, match="HIP device only"):
        gp.predict(raw, Q.cpu(), S)
    with pytest.raises(RuntimeError, match="HIP device only"):
        gp.predict(raw, Q, S.cpu())
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="must be on"):
            gp.predict(raw.to("cuda:1"), Q, S)
        with pytest.raises(ValueError, match="must be on"):
            gp.predict(raw, Q.to("cuda:1"), S)
    with pytest.raises(ValueError, match=r"\(10, N\)"):
        gp.predict(raw[:9], Q, S)
    with pytest.raises(ValueError, match=r"\(10, N\)"):
        gp.predict(raw[0], Q, S)
    with pytest.raises(ValueError, match="float32"):
        gp.predict(raw.double(), Q, S)
    with pytest.raises(ValueError, match="source"):
        gp.predict(raw, Q, S, source="hydroatlas")
    for bad_q, bad_s in ((Q[:299], S), (Q, S[:299]), (Q.reshape(1, 300), S), (Q, np.zeros(301, np.float32))):
        with pytest.raises(ValueError, match="shape"):
            gp.predict(raw, bad_q, bad_s)
    for bad_q, bad_s in ((Q.double(), S), (Q, S.half())):
        with pytest.raises(ValueError, match="float32"):
            gp.predict(raw, bad_q, bad_s)
    with pytest.raises(ValueError, match="Missing MERIT attributes"):
        gp.predict({k: v for k, v in attrs_of(d, "merit").items() if k != "NDVI"}, Q, S, source="merit")
    # a KAN that does not learn n or q_spatial
    names = [str(s) for s in d["names_merit"]]
    for learn in (["q_spatial", "p_spatial"], ["n", "p_spatial"]):
        net = kan(names, learn, 5, 1, 3, 2, 0, device=cuda)
        with pytest.raises(ValueError, match="must learn"):
            GeometryPredictor(net, names, torch.from_numpy(d["mean"]), torch.from_numpy(d["std"]), ranges_of(d), LOG_SPACE,
                              {"p_spatial": 21.0}, mins_of(d), device=cuda)
    # a predictor whose KAN stayed on the host
    host = kan(names, LEARN[""], 5, 1, 3, 2, 0)
    mixed = GeometryPredictor(host, names, torch.from_numpy(d["mean"]), torch.from_numpy(d["std"]), ranges_of(d), LOG_SPACE,
                              {"p_spatial": 21.0}, mins_of(d), device=cuda)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mixed.predict(raw, Q, S)
    # after every refusal the predictor still works
    assert bool(torch.isfinite(gp.predict(raw, Q, S)["n"][:7]).all())


# ---- sizes at which the kernels take another path, or an index passes 2^31 ----
def test_geometry_kernel_grid_stride(cuda, fx):
    """More than 4096 tiles of 256 reaches: every workgroup walks several tiles.  A reach's result does not depend on
    the launch, so the fixture repeated gives the fixture's result repeated, bit for bit."""
    d, N = fx, 4096 * 256 + 300
    reps = -(-N // 300)
    rep = lambda a: torch.from_numpy(a).to(cuda).repeat(reps, *([1] * (a.ndim - 1)))[:N].contiguous()  # noqa: E731
    u, Q, S = rep(d["u"]), rep(d["discharge"]), rep(d["slope"])
    slots, mins = slots_of(d, ""), mins_of(d)
    small = geometry_predict(u[:300], slots, Q[:300], S[:300], mins)
    big = geometry_predict(u, slots, Q, S, mins)
    assert big.shape == (11, N) and same_bits(big, small.repeat(1, reps)[:, :N])
    par = geometry_predict(u, slots, None, None, mins)
    assert same_bits(par, big[8:])


def test_prepare_kernel_feature_stride_past_2_31(cuda, fx):
    """Columns 2^28 elements apart: feature f starts f 2^28 floats into the buffer (9 2^28 > 2^31)."""
    d, stride = fx, 1 << 28
    big = torch.empty((10, stride), dtype=torch.float32, device=cuda)  # (10 GiB, untouched but for 300 columns)
    big[:, :300] = torch.from_numpy(d["raw_merit"]).to(cuda)
    dev = lambda k: torch.from_numpy(d[k]).to(cuda)  # noqa: E731
    counts = torch.zeros((3, 10), dtype=torch.int64, device=cuda)
    x = prepare_attributes(big[:, :300], *transform("merit", cuda), dev("mean"), dev("std"), dev("p10"), dev("p90"), counts)
    assert np.array_equal(x.cpu().numpy().view(np.int32), d["x_ref"].view(np.int32))
    assert np.array_equal(counts.cpu().numpy(), d["counts"])


def test_rows_past_2_31_elements(cuda, fx):
    """N F > 2^31 in the prepare kernel (F = 32) and 10 N > 2^31 in the geometry kernel's last row: the ends of both
    results equal a small launch on the same rows."""
    d = fx
    g = torch.Generator(device=cuda).manual_seed(3)
    # prepare: x element (N - 1, 31) is at N F - 1 > 2^31
    F, N = 32, (1 << 26) + 77
    raw = torch.empty((F, N), dtype=torch.float32, device=cuda).normal_(generator=g)
    raw[:, -5] = float("nan")
    mean, std = torch.linspace(-1, 1, F, device=cuda), torch.linspace(0.5, 2, F, device=cuda)
    tf = (torch.ones(F, dtype=torch.float64, device=cuda), torch.zeros(F, dtype=torch.float64, device=cuda),
          torch.zeros(F, dtype=torch.int32, device=cuda))
    counts = torch.zeros((3, F), dtype=torch.int64, device=cuda)
    x = prepare_attributes(raw, *tf, mean, std, counts=counts)
    tail = raw[:, -1000:].cpu().numpy()
    want = ((np.where(np.isnan(tail), mean.cpu().numpy()[:, None], tail) - mean.cpu().numpy()[:, None])
            / std.cpu().numpy()[:, None]).astype(np.float32).T
    assert np.array_equal(x[-1000:].cpu().numpy().view(np.int32), want.view(np.int32))
    assert counts.cpu().numpy().tolist() == [[1] * F, [0] * F, [0] * F]
    del raw, x
    # geometry: row 10 of reach N - 1 is at 11 N - 1 > 2^31
    N = (1 << 28) + 5
    reps = -(-N // 300)
    rep = lambda a: torch.from_numpy(a).to(cuda).repeat(reps, *([1] * (a.ndim - 1)))[:N].contiguous()  # noqa: E731
    u, Q, S = rep(d["u"]), rep(d["discharge"]), rep(d["slope"])
    slots, mins = slots_of(d, ""), mins_of(d)
    big = geometry_predict(u, slots, Q, S, mins)
    small = geometry_predict(u[-300:].contiguous(), slots, Q[-300:].contiguous(), S[-300:].contiguous(), mins)
    assert same_bits(big[:, -300:], small) and same_bits(big[:, :300], geometry_predict(u[:300], slots, Q[:300], S[:300], mins))
