"""Generate ``geopredict.npz``: the fixture of the geometry predictor (``ddr_amd.geometry.GeometryPredictor``,
``csrc/geopredict.hip``).  BUILD-CONTAINER ONLY (it imports the reference's own functions by file).

The expected geometry comes from the REFERENCE's ``compute_trapezoidal_geometry``
(``src/ddr/geometry/trapezoidal.py``) and ``denormalize`` (``src/ddr/routing/utils.py:166-185``), loaded the way
``make_golden.py`` loads them, run once in fp64 (``ref64``) and once in fp32 (``ref32``) on the same fp32 inputs;
``e32`` is the deviation of the two, the reference's own fp32 error that the kernel is measured against.

The reference's ``adapt_attributes`` / ``_prepare_attributes`` / ``_check_distribution`` need xarray, which is not
installed; the few lines they apply per attribute are restated in NumPy below with their line numbers.

``u`` is ``ddr_amd.nn.TorchKan`` in fp64 (pykan cannot run here -- ``tests/test_gpu_kan.py`` pins the HIP KAN to
the same model) with the published MERIT geometry checkpoint's weights (``kan_merit.npz``).

    python tests/golden/make_geopredict_golden.py --reference <checkout of taddyb/ddr>
"""

from __future__ import annotations

import argparse
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))

from ddr_amd.geometry.adapters import HYDROATLAS_TO_MERIT, MERIT_ATTRIBUTE_NAMES  # noqa: E402
from ddr_amd.nn import TorchKan  # noqa: E402

N, F = 300, 10
GEOMETRY_OUTPUTS = ("depth", "top_width", "bottom_width", "side_slope", "cross_sectional_area", "wetted_perimeter",
                    "hydraulic_radius", "velocity", "n", "p_spatial", "q_spatial")
RANGES = {"n": [0.015, 0.25], "q_spatial": [0.0, 1.0], "p_spatial": [1.0, 200.0]}
LOG_SPACE = ["p_spatial"]
# the minimums: the reference's defaults for slope and bottom width; discharge and depth lower than its 1e-4 / 0.01,
# under which the published checkpoint's p and q cannot bring the side slope to its upper clamp (50)
MINS = {"discharge": 1e-9, "slope": 0.001, "depth": 0.0005, "bottom_width": 0.01}
BRANCHES = ("discharge_lb", "slope_lb", "depth_lb", "side_slope_lb", "side_slope_ub", "bottom_width_lb")
SEED_O2 = 23  # the seeded TorchKan of the second case (O = 2: n, q_spatial; p_spatial defaulted to 21)
ARCH_O2 = dict(hidden_size=11, num_hidden_layers=1, grid=3, k=3)


def load_reference(ref: Path):
    def _load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    for pkg in ["ddr", "ddr.routing", "ddr.geometry", "ddr.validation"]:
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    cfgmod = types.ModuleType("ddr.validation.configs")
    cfgmod.Config = object
    sys.modules["ddr.validation.configs"] = cfgmod
    trap = _load("ddr.geometry.trapezoidal", ref / "src/ddr/geometry/trapezoidal.py")
    utils = _load("ddr.routing.utils", ref / "src/ddr/routing/utils.py")
    return trap.compute_trapezoidal_geometry, utils.denormalize


def attributes(rng):
    """Raw attributes in both namings, the statistics, and what the reference makes of them."""
    mean = np.array([20.0, 1.1, 450.0, 900.0, 0.45, 3.0, 1.6, 40.0, 1100.0, 0.17], dtype=np.float32)
    std = np.array([8.0, 0.6, 380.0, 420.0, 0.2, 2.5, 0.9, 15.0, 300.0, 0.05], dtype=np.float32)
    # p10 / p90 of a normal: mean -+ 1.2816 std, so ~10 % of a sample drawn 1.5 x as wide lies beyond each
    p10 = (mean - np.float32(1.2816) * std).astype(np.float32)
    p90 = (mean + np.float32(1.2816) * std).astype(np.float32)
    hydro = (mean[:, None] + std[:, None] * 1.5 * rng.standard_normal((F, N))).astype(np.float32)
    j = MERIT_ATTRIBUTE_NAMES.index("log10_uparea")
    area = (10.0 ** (1.6 + 1.2 * rng.standard_normal(N))).astype(np.float32)  # km^2
    area[rng.choice(N, 24, replace=False)] = np.repeat(np.array([0.0, -3.5, 5e-7, 1e-9, 9.99e-7, 1e-6], np.float32), 4)
    hydro[j] = area
    for f in range(F):  # NaNs in every feature, one all-NaN row, one +inf and one -inf
        hydro[f, rng.choice(N, 3 + f % 3, replace=False)] = np.nan
    hydro[:, 7] = np.nan
    hydro[2, 11], hydro[5, 12] = np.inf, -np.inf
    names_h = list(HYDROATLAS_TO_MERIT)
    assert [HYDROATLAS_TO_MERIT[k].merit_name for k in names_h] == list(MERIT_ATTRIBUTE_NAMES)
    # adapters.py:159-164: values = ds[src].astype(np.float64) * scale + offset; log10(values.clip(min=1e-6))
    merit = hydro.copy()
    for f, k in enumerate(names_h):
        m = HYDROATLAS_TO_MERIT[k]
        v = hydro[f].astype(np.float64) * m.scale + m.offset
        if m.log_transform:
            v = np.log10(v.clip(min=1e-6))
            assert (hydro[f] <= 0).sum() >= 4 and ((hydro[f] > 0) & (hydro[f] < 1e-6)).sum() >= 4
        # predictor.py:253: np.asarray(adapted[attr_name].values, dtype=np.float32)
        merit[f] = v.astype(np.float32)
    assert np.array_equal(np.delete(merit, j, 0), np.delete(hydro, j, 0), equal_nan=True)
    # predictor.py:341-342 (values < p10, values > p90; a NaN is neither), on the fp32 values the kernel holds
    with np.errstate(invalid="ignore"):
        below, above = (merit < p10[:, None]).sum(1), (merit > p90[:, None]).sum(1)
    # predictor.py:254-259: arr[np.isnan(arr)] = means[i].item()
    nan = np.isnan(merit)
    filled = nan.sum(1)
    v = np.where(nan, mean[:, None], merit).astype(np.float32)
    # predictor.py:270-273: ((raw - means.unsqueeze(1)) / stds.unsqueeze(1)).T
    with np.errstate(invalid="ignore"):
        x_ref = ((v - mean[:, None]) / std[:, None]).astype(np.float32).T.copy()
    assert (filled > 0).all() and (below > 0).all() and (above > 0).all()
    counts = np.stack([filled, below, above]).astype(np.int64)
    return dict(raw_merit=merit, raw_hydroatlas=hydro, names_merit=np.array(MERIT_ATTRIBUTE_NAMES),
                names_hydroatlas=np.array(names_h), mean=mean, std=std, p10=p10, p90=p90, x_ref=x_ref, counts=counts)


def kan_u(model: TorchKan, x_ref: np.ndarray) -> np.ndarray:
    with torch.no_grad():
        o = model.double()(inputs=torch.from_numpy(x_ref).double())
    return torch.stack([o[k] for k in model.learnable_parameters], dim=1).to(torch.float32).numpy()


def reference_outputs(trapezoid, denormalize, u, learn, Q, S, dtype, default_p):
    """predictor.py:203-238 + 276-318 with the reference's functions, in ``dtype``: (11, N)."""
    ut = torch.from_numpy(u).to(dtype)
    par = {}
    for name in ("n", "q_spatial", "p_spatial"):
        if name in learn:
            par[name] = denormalize(value=ut[:, learn.index(name)], bounds=RANGES[name], log_space=name in LOG_SPACE)
        else:
            par[name] = torch.full_like(ut[:, 0], default_p)
    q_t = torch.clamp(torch.from_numpy(Q).to(dtype), min=MINS["discharge"])
    s_t = torch.clamp(torch.from_numpy(S).to(dtype), min=MINS["slope"])
    geo = trapezoid(n=par["n"], p_spatial=par["p_spatial"], q_spatial=par["q_spatial"], discharge=q_t, slope=s_t,
                    depth_lb=MINS["depth"], bottom_width_lb=MINS["bottom_width"])
    geo = dict(geo, **par)
    return torch.stack([geo[k] for k in GEOMETRY_OUTPUTS]).numpy()


def branch_counts(ref64, Q, S):
    """How many reaches sit on each clamp (of those whose geometry is finite)."""
    r = dict(zip(GEOMETRY_OUTPUTS, ref64))
    ok = np.isfinite(ref64).all(0)
    with np.errstate(invalid="ignore"):
        c = [Q < MINS["discharge"], S < MINS["slope"], r["depth"] == MINS["depth"], r["side_slope"] == 0.5,
             r["side_slope"] == 50.0, r["bottom_width"] == MINS["bottom_width"]]
    return np.array([int((m & ok).sum()) for m in c], dtype=np.int64), int(ok.sum())


def fields(rng, u, learn, trapezoid, denormalize, default_p, tag):
    """Discharge and slope that put every clamp on and off at >= 5 % of the reaches, for this u: each reach gets
    a target depth (from far below the depth bound, where the side slope passes 50, to tens of metres, where it
    falls below 0.5 and the bottom width to its bound) and the discharge that Manning's equation inverts to it."""
    S = (10.0 ** rng.uniform(-4.0, -0.7, N)).astype(np.float32)
    u64 = torch.from_numpy(np.nan_to_num(u, nan=0.5)).double()
    par = {k: (denormalize(value=u64[:, learn.index(k)], bounds=RANGES[k], log_space=k in LOG_SPACE).numpy()
               if k in learn else np.full(N, default_p)) for k in ("n", "q_spatial", "p_spatial")}
    depth = 10.0 ** np.where(rng.uniform(size=N) < 0.55, rng.uniform(-4.3, -2.0, N), rng.uniform(-2.0, 3.8, N))
    qe = par["q_spatial"] + 1e-6
    ratio = depth ** ((5.0 + 3.0 * qe) / 3.0)  # trapezoidal.py:62-71 solved for the discharge
    Q = ratio * (par["p_spatial"] * np.sqrt(np.maximum(S.astype(np.float64), MINS["slope"])) + 1e-8) / (par["n"] * (qe + 1))
    low = rng.choice(N, 36, replace=False)  # and some below the discharge bound
    Q[low] = MINS["discharge"] * 10.0 ** rng.uniform(-2.0, -0.01, 36)
    Q = Q.astype(np.float32)
    S[[3, 50, 200]] = np.nan
    Q[[4, 120]] = np.nan
    ref64 = reference_outputs(trapezoid, denormalize, u, learn, Q, S, torch.float64, default_p)
    ref32 = reference_outputs(trapezoid, denormalize, u, learn, Q, S, torch.float32, default_p)
    counts, n_ok = branch_counts(ref64, Q, S)
    print(tag, "finite reaches", n_ok, dict(zip(BRANCHES, counts.tolist())))
    lo = int(np.ceil(0.05 * N))
    assert ((counts >= lo) & (n_ok - counts >= lo)).all(), (tag, counts, n_ok)
    assert np.array_equal(np.isnan(ref64), np.isnan(ref32))
    fin = np.isfinite(ref64)
    e32 = np.array([np.max(np.abs(ref32[k][fin[k]].astype(np.float64) - ref64[k][fin[k]]) / np.abs(ref64[k][fin[k]]))
                    for k in range(len(GEOMETRY_OUTPUTS))])
    print(tag, "e32", dict(zip(GEOMETRY_OUTPUTS, (f"{e:.2e}" for e in e32))))
    return {f"discharge{tag}": Q, f"slope{tag}": S, f"ref64{tag}": ref64, f"ref32{tag}": ref32, f"e32{tag}": e32,
            f"branch_counts{tag}": counts, f"n_finite{tag}": np.int64(n_ok)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", type=Path, required=True, help="checkout of the reference (taddyb/ddr)")
    args = ap.parse_args()
    trapezoid, denormalize = load_reference(args.reference)
    rng = np.random.default_rng(20240519)
    out = attributes(rng)
    # case 1: the published MERIT geometry checkpoint (n, q_spatial, p_spatial)
    learn = ["n", "q_spatial", "p_spatial"]
    model = TorchKan(list(MERIT_ATTRIBUTE_NAMES), learn, 21, 2, 50, 2, 0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(HERE / "kan_merit.npz").items()})
    out["u"] = kan_u(model, out["x_ref"])
    out.update(fields(rng, out["u"], learn, trapezoid, denormalize, 21.0, ""))
    # case 2: O = 2, p_spatial defaulted; seeded random TorchKan weights, regenerated at test time
    learn2 = ["n", "q_spatial"]
    model2 = TorchKan(list(MERIT_ATTRIBUTE_NAMES), learn2, seed=SEED_O2, **ARCH_O2)
    out["u_o2"] = kan_u(model2, out["x_ref"])
    out.update(fields(rng, out["u_o2"], learn2, trapezoid, denormalize, 21.0, "_o2"))
    out.update(seed_o2=np.int64(SEED_O2), arch_o2=np.array([ARCH_O2[k] for k in ("hidden_size", "num_hidden_layers",
                                                                                  "grid", "k")], dtype=np.int64),
               default_p_o2=np.float64(21.0), outputs=np.array(GEOMETRY_OUTPUTS), branches=np.array(BRANCHES),
               bounds=np.array([RANGES["n"], RANGES["q_spatial"], RANGES["p_spatial"]], dtype=np.float64),
               minimums=np.array([MINS[k] for k in ("discharge", "slope", "depth", "bottom_width")], dtype=np.float64))
    np.savez_compressed(HERE / "geopredict.npz", **out)
    print("geopredict.npz", (HERE / "geopredict.npz").stat().st_size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
