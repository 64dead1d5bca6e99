"""Generate golden vectors from the reference's own routing code.  BUILD-CONTAINER ONLY.

This script imports the reference's hot-path modules from ``/root/reference`` (read-only) with
stub parent packages (``ddr`` itself needs Python >= 3.12 and hydra/xarray/pykan,
none of which are installed; the three routing modules need only torch + SciPy).  It runs the
reference ``MuskingumCunge`` forward + autograd backward on seeded inputs and writes small
``.npz`` fixtures next to this file.  The reference never travels to the GPU box: only the
fixtures do.

Fixtures:
  kat.npz       F1  reference KATs: general-diagonal solve + grads, hot-start chains, denormalize
  sandbox.npz   F2  RAPID Sandbox 5-reach topology (10,20->30; 30,40->50), synthetic q', default p
  tree300.npz   F3  300-reach random binary tree x 40 steps, learned n/q/p, loss = sum(W*out)
  gauge.npz     F4  gauge mode (ragged outflow_idx incl. a negative index) + carry_state batch 2
  c1.npz        F5  config C1 shape (2000 x 720): outlet series, sampled runoff, unit-param grads
  csr.npz       F6  canonical CSR + PatternMapper (crow, col) for the F3 and F5 graphs
  geostats.npz  F7  reference compute_geometry_statistics (statistics.py:20-83): 150 reaches x 31 and
                    x 30 days (odd / even median), NaN discharge entries, default and mock bounds
  geostats_edges.npz  the same on 40 reaches x 70 days with negative, zero, +inf and NaN days, an all-NaN
                    reach, default and (depth 0.5, bottom_width 0.1) bounds
  collate.npz   F9  per-batch gauge union: reference builders.construct_network_matrix + the network
                    half of Merit._collate_gages (merit.py:197-238) on a synthetic 3k-reach CONUS with
                    12 gauge subsets (nested gauges, a headwater gauge, a gauge missing from the store)
  deep.npz      F10 the reference on C5's 281k-reach, 2215-deep basin over 24 h: unit-parameter
                    gradients and the outlet series (fp32 gradient accuracy along deep chains)
  state.npz     F11 state gradients (route_timestep is differentiable w.r.t. q_prime_clamp and
                    _discharge_t, mmc.py:487-559; the hot start w.r.t. q'[0], mmc.py:25-66): dL/dstreamflow
                    of a hot-started forward, dL/dstreamflow + dL/dQ0 of a gauge-mode carried batch (one
                    gauge's carried sum below q_lb), and a 3-step route_timestep chain
  chain.npz     F12 gradients out of the final state and the reported geometry: two chained gauge-mode
                    batches (the second carries the first's _discharge_t with its graph), and one batch
                    with the loss also on _discharge_t, top_width and side_slope (gauge / all-output mode)
  timestep_geo.npz F13 a 3-step route_timestep chain whose loss includes every step's top_width /
                    side_slope (the geometry of the carried state, two carried values below q_lb)
  daily.npz     F8  the training objective of scripts/train.py:78-97 on a (7, 2136) gauge series:
                    downsample(runoff[:, 13:-8], 88) (io/functions.py:7-23), NaN-gauge mask, L1 with
                    warmup 3, and torch autograd's d loss / d runoff
  confluence.npz  a 300-reach tree with in-degrees up to 20 (tests/confluence_cases.py bushy) x 48 steps: outputs
                    and gradients, a carried second leg, a gauge-mode run with gauges on confluences, and
                    the CSR + PatternMapper layout

Run:  python tests/golden/make_golden.py [geostats daily]   (no argument: all fixtures)
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
REPO = HERE.parent.parent
sys.path.insert(0, str(REPO))
REF = Path("/root/reference/src/ddr")

from ddr_amd import synthetic  # noqa: E402


def load_reference():
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
    _load("ddr.geometry.trapezoidal", REF / "geometry/trapezoidal.py")
    utils = _load("ddr.routing.utils", REF / "routing/utils.py")
    mmc = _load("ddr.routing.mmc", REF / "routing/mmc.py")
    return utils, mmc


PARAMS_DEFAULT = dict(
    parameter_ranges={"n": [0.015, 0.25], "q_spatial": [0.0, 1.0], "p_spatial": [1.0, 200.0]},
    log_space_parameters=["p_spatial"],
    defaults={"p_spatial": 21},
    attribute_minimums={"discharge": 0.0001, "slope": 0.001, "velocity": 0.01, "depth": 0.01,
                        "bottom_width": 0.01},
)
# tests/routing/test_utils.py:31-65 (mock config)
PARAMS_MOCK = dict(
    parameter_ranges={"n": [0.01, 0.1], "q_spatial": [0.1, 0.9], "p_spatial": [1.0, 200.0]},
    log_space_parameters=["p_spatial"],
    defaults={"p_spatial": 1.0},
    attribute_minimums={"velocity": 0.1, "depth": 0.01, "discharge": 0.001, "bottom_width": 0.1,
                        "slope": 0.001},
)


def cfg_of(params):
    return SimpleNamespace(params=SimpleNamespace(**params))


def routing_dc(n, rows, cols, attrs, outflow_idx=None, flow_scale=None):
    a = sp.coo_matrix((np.ones(len(rows), dtype=np.float32), (rows, cols)), shape=(n, n)).tocsr()
    adj = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)),
                                  torch.from_numpy(a.indices.astype(np.int64)),
                                  torch.from_numpy(a.data.astype(np.float32)), size=(n, n))
    return SimpleNamespace(adjacency_matrix=adj, length=torch.from_numpy(attrs.length),
                           slope=torch.from_numpy(attrs.slope), x=torch.from_numpy(attrs.x),
                           top_width=torch.empty(0), side_slope=torch.empty(0), outflow_idx=outflow_idx,
                           gage_catchment=None, observations=None, flow_scale=flow_scale)


def run_ref(mmc, params, dc, qprime, u, W, carry_from=None):
    mc = mmc.MuskingumCunge(cfg_of(params), device="cpu")
    if carry_from is not None:
        mc._discharge_t = carry_from
    sp_params = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in u.items()}
    mc.setup_inputs(dc, torch.from_numpy(qprime), sp_params, carry_state=carry_from is not None)
    out = mc.forward()
    loss = (out * torch.from_numpy(W)).sum()
    loss.backward()
    grads = {f"grad_{k}": v.grad.numpy().copy() for k, v in sp_params.items()}
    return dict(runoff=out.detach().numpy(), q_last=mc._discharge_t.detach().numpy(),
                top_width=mc.top_width.detach().numpy(), side_slope=mc.side_slope.detach().numpy(),
                **grads), mc


def kat(utils, mmc):
    out = {}
    crow = torch.tensor([0, 1, 3, 5], dtype=torch.int32)
    col = torch.tensor([0, 0, 1, 1, 2], dtype=torch.int32)
    A = torch.tensor([2.0, 1.0, 3.0, 1.0, 4.0], requires_grad=True)
    b = torch.tensor([2.0, 7.0, 13.0], requires_grad=True)
    x = utils.triangular_sparse_solve(A, crow, col, b, True, False, "cpu")
    x.sum().backward()
    out.update(kat_crow=crow.numpy(), kat_col=col.numpy(), kat_A=A.detach().numpy(), kat_b=b.detach().numpy(),
               kat_x=x.detach().numpy(), kat_gradA=A.grad.numpy(), kat_gradb=b.grad.numpy())
    # hot start on linear chains (tests/routing/test_mmc.py:564-602)
    for name, q in (("uniform5", np.full(5, 2.0, np.float32)), ("nonuniform4", np.array([3, 1, 2, 4], np.float32)),
                    ("single", np.array([5.0], np.float32)), ("clamp3", np.full(3, 1e-5, np.float32))):
        nn_ = len(q)
        mc = mmc.MuskingumCunge(cfg_of(PARAMS_MOCK), device="cpu")
        adj = torch.zeros(nn_, nn_)
        for i in range(nn_ - 1):
            adj[i + 1, i] = 1.0
        mc.network = adj
        mapper, _, _ = mc.create_pattern_mapper()
        res = mmc.compute_hotstart_discharge(torch.from_numpy(q), mapper, mc.discharge_lb, "cpu")
        out[f"hot_{name}_q"] = q
        out[f"hot_{name}_out"] = res.numpy()
    u = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0])
    out["den_u"] = u.numpy()
    out["den_lin"] = utils.denormalize(u, [0.015, 0.25]).numpy()
    out["den_log"] = utils.denormalize(u, [1.0, 200.0], log_space=True).numpy()
    return out


def mapper_csr(mmc, n, rows, cols):
    mc = mmc.MuskingumCunge(cfg_of(PARAMS_DEFAULT), device="cpu")
    a = sp.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, n)).tocsr()
    mc.network = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)),
                                         torch.from_numpy(a.indices.astype(np.int64)),
                                         torch.from_numpy(a.data), size=(n, n))
    mapper, _, _ = mc.create_pattern_mapper()
    idx = (mapper.M_csr.to_dense().argmax(0)).numpy()
    return a.indptr.astype(np.int64), a.indices.astype(np.int64), mapper.crow_indices.numpy(), \
        mapper.col_indices.numpy(), idx


def case(mmc, params, net, T, seed, outflow_idx=None, learn_p=True):
    attrs = synthetic.reach_attributes(net.n, seed)
    q = synthetic.lateral_inflow(net.n, T, seed)
    u = synthetic.unit_parameters(net.n, seed)
    if not learn_p:
        u.pop("p_spatial")
    G = net.n if outflow_idx is None else len(outflow_idx)
    W = np.random.default_rng(seed + 4000).uniform(0, 1, (G, T)).astype(np.float32)
    dc = routing_dc(net.n, net.rows, net.cols, attrs, outflow_idx)
    res, mc = run_ref(mmc, params, dc, q, u, W)
    inputs = dict(n=np.int64(net.n), rows=net.rows, cols=net.cols, length=attrs.length, slope=attrs.slope,
                  x=attrs.x, qprime=q, W=W, **{f"u_{k}": v for k, v in u.items()})
    return inputs, res, mc, dc


def load_objective_modules():
    """statistics.py (needs ddr.geometry.trapezoidal) and io/functions.py, with stub parents."""
    load_reference()
    spec = importlib.util.spec_from_file_location("ddr.geometry.statistics", REF / "geometry/statistics.py")
    stats = importlib.util.module_from_spec(spec)
    sys.modules["ddr.geometry.statistics"] = stats
    spec.loader.exec_module(stats)
    spec = importlib.util.spec_from_file_location("ddr_io_functions", REF / "io/functions.py")
    fun = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fun)
    return stats, fun


def make_geostats():
    stats, _ = load_objective_modules()
    rng = np.random.default_rng(77)
    N = 150
    u = synthetic.unit_parameters(N, 77)
    n = (u["n"] * np.float32(0.235) + np.float32(0.015)).astype(np.float32)
    q = u["q_spatial"].astype(np.float32)
    lo, hi = np.log(np.float32(1.0 + 1e-6)), np.log(np.float32(200.0))
    p = np.exp(u["p_spatial"] * np.float32(hi - lo) + np.float32(lo)).astype(np.float32)
    slope = np.maximum(rng.lognormal(np.log(1e-3), 1.0, N).astype(np.float32), np.float32(1e-3))
    out = dict(n=n, p=p, q=q, slope=slope)
    for D in (31, 30):
        dq = rng.lognormal(np.log(5.0), 1.5, (D, N)).astype(np.float32)
        dq[rng.random((D, N)) < 0.02] = np.nan
        dq[:, 7] = np.nan  # a reach with no valid day
        for tag, mins in (("default", {"depth": 0.01, "bottom_width": 0.01}), ("mock", {"depth": 0.01, "bottom_width": 0.1})):
            with np.errstate(all="ignore"):
                import warnings

                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    res = stats.compute_geometry_statistics(torch.from_numpy(n), torch.from_numpy(p), torch.from_numpy(q),
                                                            torch.from_numpy(slope), dq, mins)
            for k, v in res.items():
                out[f"d{D}_{tag}_{k}"] = v
        out[f"d{D}_q"] = dq
    np.savez_compressed(HERE / "geostats.npz", **out)


def make_geostats_edges():
    """The reference's compute_geometry_statistics on the value classes geostats.npz lacks: negative
    discharge (pow gives NaN geometry while the discharge itself stays valid), exact zeros, one +inf day,
    NaN days and an all-NaN reach; 40 reaches x 70 days, both minimum sets."""
    stats, _ = load_objective_modules()
    rng = np.random.default_rng(78)
    N, D = 40, 70
    n = rng.uniform(0.015, 0.25, N).astype(np.float32)
    p = rng.uniform(1.0, 200.0, N).astype(np.float32)
    q = rng.uniform(0.0, 1.0, N).astype(np.float32)
    slope = rng.uniform(1e-3, 0.05, N).astype(np.float32)
    dq = rng.lognormal(0.0, 3.0, (D, N)).astype(np.float32)
    dq[rng.random((D, N)) < 0.03] = np.nan
    for r in range(0, N, 3):  # negative days, 1 to D / 2 of them
        days = rng.choice(D, int(rng.integers(1, D // 2 + 1)), replace=False)
        dq[days, r] = -np.abs(dq[days, r])
    dq[rng.random((D, N)) < 0.02] = 0.0
    dq[:, 9] = -rng.lognormal(0.0, 1.0, D).astype(np.float32)  # no valid geometry, valid discharge
    dq[:, 11] = 0.0
    for r in (4, 12, 21):
        dq[int(rng.integers(D)), r] = np.inf
    dq[:, 7] = np.nan  # a reach with no valid day
    out = dict(n=n, p=p, q=q, slope=slope, daily_q=dq)
    for tag, mins in (("default", {"depth": 0.01, "bottom_width": 0.01}), ("mock", {"depth": 0.5, "bottom_width": 0.1})):
        import warnings

        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            res = stats.compute_geometry_statistics(torch.from_numpy(n), torch.from_numpy(p), torch.from_numpy(q),
                                                    torch.from_numpy(slope), dq, mins)
        for k, v in res.items():
            out[f"{tag}_{k}"] = v
    np.savez_compressed(HERE / "geostats_edges.npz", **out)


def make_daily():
    _, fun = load_objective_modules()
    rng = np.random.default_rng(88)
    G, T, tau, warmup = 7, 2136, 3, 3
    runoff = torch.from_numpy(rng.lognormal(np.log(10.0), 1.0, (G, T)).astype(np.float32)).requires_grad_(True)
    num_days = len(runoff[0][13:(-11 + tau)]) // 24
    daily = fun.downsample(runoff[:, 13:(-11 + tau)], rho=num_days)
    obs = rng.lognormal(np.log(10.0), 1.0, (G, num_days)).astype(np.float32)
    obs[2, 40] = np.nan  # gauge 2 is dropped (train.py:84-90)
    keep = ~np.isnan(obs).any(axis=1)
    pred = daily[torch.from_numpy(keep)]
    target = torch.from_numpy(obs[keep])
    loss = torch.nn.functional.l1_loss(input=pred.transpose(0, 1)[warmup:].unsqueeze(2),
                                       target=target.transpose(0, 1)[warmup:].unsqueeze(2))
    loss.backward()
    np.savez_compressed(HERE / "daily.npz", runoff=runoff.detach().numpy(), obs=obs, tau=np.int64(tau),
                        warmup=np.int64(warmup), ref_daily=daily.detach().numpy(), ref_loss=np.float32(loss.item()),
                        ref_grad=runoff.grad.numpy())


def make_collate():
    """F9: the reference's batch collation on synthetic gauge subsets (builders.py:55-109,
    merit.py:197-238).  builders.py / merit.py import rustworkx, xarray, zarr and the ddr package at
    module level; none of those names is used by the two functions run here, so they are stub modules.
    The subsets store is a dict of objects with the zarr group interface the functions use
    (``group[name][:]``, ``.attrs``, ``.keys()``)."""
    load_reference()
    for name in ["rustworkx", "xarray", "zarr", "zarr.storage", "ddr.geodatazoo", "ddr.io",
                 "ddr.geodatazoo.base_geodataset", "ddr.geodatazoo.dataclasses", "ddr.io.readers",
                 "ddr.io.statistics", "ddr.validation.enums"]:
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["zarr"].Group = object
    sys.modules["rustworkx"].PyDiGraph = object
    sys.modules["zarr"].storage = sys.modules["zarr.storage"]
    sys.modules["xarray"].Dataset = object
    sys.modules["ddr.geodatazoo.base_geodataset"].BaseGeoDataset = object
    sys.modules["ddr.geodatazoo.dataclasses"].Dates = object
    sys.modules["ddr.geodatazoo.dataclasses"].RoutingDataclass = object
    for f in ["IcechunkUSGSReader", "build_flow_scale_tensor", "fill_nans", "filter_gages_by_area_threshold",
              "filter_gages_by_da_valid", "filter_headwater_gages", "naninfmean", "read_zarr"]:
        setattr(sys.modules["ddr.io.readers"], f, None)
    sys.modules["ddr.io.statistics"].set_statistics = None
    sys.modules["ddr.validation.enums"].Mode = object

    def _load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    builders = _load("ddr.io.builders", REF / "io/builders.py")
    merit = _load("ddr.geodatazoo.merit", REF / "geodatazoo/merit.py")
    captured = {}
    merit.build_flow_scale_tensor = lambda **kw: None
    merit.create_hydrofabric_observations = lambda **kw: None
    merit.RoutingDataclass = lambda **kw: captured.update(kw)

    net = synthetic.forest(synthetic.zipf_sizes(3000, 12, 0.35), seed=9, single_inflow=0.3)
    down = net.down
    n = net.n
    rng = np.random.default_rng(9)
    # upstream closure of a reach: every reach whose flow path passes through it (topological order:
    # upstream reaches have lower ids, so one descending sweep marks them)
    def upstream(x):
        inside = np.zeros(n, bool)
        inside[x] = True
        for j in range(x - 1, -1, -1):
            if down[j] >= 0 and inside[down[j]]:
                inside[j] = True
        inside[x] = False
        return np.flatnonzero(inside)

    outlets = np.flatnonzero(down < 0)
    big = outlets[np.argsort(-net.basin_sizes)][:4]
    gauges = list(big)
    # nested gauges inside the largest basin, a headwater gauge, random interior gauges
    up0 = upstream(big[0])
    gauges += list(rng.choice(up0, 4, replace=False))
    heads = np.setdiff1d(np.arange(n), down[down >= 0])
    gauges.append(int(rng.choice(heads)))
    gauges += list(rng.choice(np.flatnonzero(down >= 0), 3, replace=False))

    class Sub:
        def __init__(self, rows, cols, attrs):
            self._a = {"indices_0": rows, "indices_1": cols}
            self.attrs = attrs

        def __getitem__(self, k):
            return self._a[k]

    store = {}
    sub_rows, sub_cols, sub_off, gidx, ids = [], [], [0], [], []
    for k, x in enumerate(gauges):
        ups = upstream(int(x))
        rows = down[ups].astype(np.int32)
        cols = ups.astype(np.int32)
        perm = rng.permutation(len(rows))  # the engine's subset order is arbitrary
        rows, cols = rows[perm], cols[perm]
        gid = f"{1000000 + k:08d}"
        store[gid] = Sub(rows, cols, {"gage_idx": int(x), "gage_catchment": 70000 + k, "shape": [n, n]})
        sub_rows.append(rows)
        sub_cols.append(cols)
        sub_off.append(sub_off[-1] + len(rows))
        gidx.append(int(x))
        ids.append(gid)

    class Store(dict):
        pass

    st = Store(store)
    batch = np.array(ids[:6] + ["09999999"] + ids[6:])  # one gauge missing from the store
    coo, out_idx, out_wb = builders.construct_network_matrix([b for b in batch.tolist() if b in st], st)
    self_ = SimpleNamespace(gages_adjacency=st, merit_ids=np.arange(n, dtype=np.int64) + 500000,
                            obs_reader=SimpleNamespace(gage_dict={}), dates=None, observations=None,
                            _build_common_tensors=lambda csr, ids_, act: (csr, None, None, {k: None for k in (
                                "length", "slope", "side_slope", "top_width", "x")}))
    merit.Merit._collate_gages(self_, batch)
    csr = captured["adjacency_matrix"]
    of = captured["outflow_idx"]
    pairs = np.array(sorted(zip(coo.row.tolist(), coo.col.tolist())), dtype=np.int64).reshape(-1, 2)
    np.savez_compressed(HERE / "collate.npz", n_conus=np.int64(n), conus_rows=net.rows, conus_cols=net.cols,
                        sub_rows=np.concatenate(sub_rows), sub_cols=np.concatenate(sub_cols),
                        sub_off=np.array(sub_off, np.int64), gage_idx=np.array(gidx, np.int64), gage_ids=np.array(ids),
                        batch=batch, ref_union_pairs=pairs, ref_gage_idx=np.array(out_idx, np.int64),
                        ref_gage_catchment=np.array(out_wb, np.int64),
                        ref_divide_ids=np.asarray(captured["divide_ids"], np.int64),
                        ref_crow=csr.indptr.astype(np.int64), ref_col=csr.indices.astype(np.int64),
                        ref_outflow_flat=np.concatenate(of).astype(np.int64),
                        ref_outflow_off=np.concatenate([[0], np.cumsum([len(o) for o in of])]).astype(np.int64),
                        ref_gage_catchment_batch=np.array(captured["gage_catchment"], np.int64))


def deep_case(T=24):
    """The C5 forest's largest basin (281k reaches, depth 2215), routed alone (tests/conftest.py)."""
    sys.path.insert(0, str(HERE.parent))
    from conftest import deep_case as _deep

    return _deep(T)


def make_deep():
    """F10: the reference (fp32 elementwise + SciPy fp64 solve, torch autograd) on the 281k-reach,
    2215-deep basin of C5 over 24 hours: unit-parameter gradients of sum(W * runoff) and the outlet
    series.  Pins what fp32 arithmetic itself does to gradients along a 2215-hop chain."""
    import time

    _, mmc = load_reference()
    c = deep_case()
    dc = routing_dc(c.n, c.rows, c.cols, c.attrs)
    t0 = time.time()
    res, _ = run_ref(mmc, PARAMS_DEFAULT, dc, c.qprime, c.u, c.W)
    print(f"deep: reference fwd+bwd {time.time() - t0:.0f}s", flush=True)
    np.savez_compressed(HERE / "deep.npz", T=np.int64(c.qprime.shape[0]), n=np.int64(c.n),
                        ref_outlet=res["runoff"][c.n - 1], **{f"ref_{k}": v for k, v in res.items() if k.startswith("grad_")})


def make_state():
    """F11: gradients w.r.t. the lateral inflow and the carried discharge state from the reference's
    autograd (the fused kernel's state-gradient adjoint must reproduce them)."""
    _, mmc = load_reference()
    net = synthetic.random_binary_tree(90, seed=21)
    T = 24
    attrs = synthetic.reach_attributes(net.n, 21)
    u = synthetic.unit_parameters(net.n, 21)
    rng = np.random.default_rng(2100)
    out = dict(n=np.int64(net.n), rows=net.rows, cols=net.cols, length=attrs.length, slope=attrs.slope, x=attrs.x,
               **{f"u_{k}": v for k, v in u.items()})

    def run(qprime, W, outflow_idx=None, q0=None):
        dc = routing_dc(net.n, net.rows, net.cols, attrs, outflow_idx)
        mc = mmc.MuskingumCunge(cfg_of(PARAMS_DEFAULT), device="cpu")
        q0t = None
        if q0 is not None:
            q0t = torch.from_numpy(q0).clone().requires_grad_(True)
            mc._discharge_t = q0t
        sp_params = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in u.items()}
        qp = torch.from_numpy(qprime).clone().requires_grad_(True)
        mc.setup_inputs(dc, qp, sp_params, carry_state=q0 is not None)
        o = mc.forward()
        (o * torch.from_numpy(W)).sum().backward()
        r = dict(runoff=o.detach().numpy(), grad_qprime=qp.grad.numpy().copy(),
                 **{f"grad_{k}": v.grad.numpy().copy() for k, v in sp_params.items()})
        if q0t is not None:
            r["grad_q0"] = q0t.grad.numpy().copy()
        return r

    # (a) hot-started forward (per-reach outputs); a few q' below the clamp
    qa = synthetic.lateral_inflow(net.n, T, 21)
    qa[3, :7] = 2e-5
    hw = np.setdiff1d(np.arange(net.n), net.rows)[:3]
    qa[0, hw] = 1e-6  # headwaters whose hot start falls below q_lb (the clamp's backward masks them)
    Wa = rng.uniform(0, 1, (net.n, T)).astype(np.float32)
    ra = run(qa, Wa)
    out.update(qprime_a=qa, W_a=Wa, **{f"ref_a_{k}": v for k, v in ra.items()})
    # (b) gauge mode with a carried state: gauge 2 is one reach whose carried Q0 is below q_lb
    outflow = [np.array([-1]), np.array([10, 20, 31]), np.array([44]), np.array([5, 59, 60])]
    qb = synthetic.lateral_inflow(net.n, T, 22)
    q0 = rng.uniform(0.5, 5.0, net.n).astype(np.float32)
    q0[44] = 3e-5
    q0[20] = 5e-5
    Wb = rng.uniform(0, 1, (len(outflow), T)).astype(np.float32)
    rb = run(qb, Wb, outflow, q0)
    flat = np.concatenate(outflow)
    offs = np.cumsum([0] + [len(o) for o in outflow])
    out.update(qprime_b=qb, W_b=Wb, q0_b=q0, outflow_flat=flat, outflow_offsets=offs,
               **{f"ref_b_{k}": v for k, v in rb.items()})
    # (c) three chained route_timestep calls (the BMI update, bmi.py -> mmc.route_timestep)
    dc = routing_dc(net.n, net.rows, net.cols, attrs)
    mc = mmc.MuskingumCunge(cfg_of(PARAMS_DEFAULT), device="cpu")
    sp_params = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in u.items()}
    qc = synthetic.lateral_inflow(net.n, 3, 23)
    mc.setup_inputs(dc, torch.from_numpy(qc), sp_params)
    q0c = rng.uniform(0.5, 5.0, net.n).astype(np.float32)
    s0 = torch.from_numpy(q0c).clone().requires_grad_(True)
    mc._discharge_t = s0
    mapper, _, _ = mc.create_pattern_mapper()
    Wc = rng.uniform(0, 1, (3, net.n)).astype(np.float32)
    qcl = [torch.from_numpy(np.maximum(qc[k], np.float32(1e-4))).clone().requires_grad_(True) for k in range(3)]
    loss = 0.0
    states = []
    for k in range(3):
        q1 = mc.route_timestep(q_prime_clamp=qcl[k], mapper=mapper)
        mc._discharge_t = q1
        states.append(q1.detach().numpy().copy())
        loss = loss + (q1 * torch.from_numpy(Wc[k])).sum()
    loss.backward()
    out.update(qprime_c=qc, q0_c=q0c, W_c=Wc, ref_c_states=np.stack(states), ref_c_grad_q0=s0.grad.numpy().copy(),
               ref_c_grad_qclamp=np.stack([q.grad.numpy().copy() for q in qcl]),
               **{f"ref_c_grad_{k}": v.grad.numpy().copy() for k, v in sp_params.items()})
    np.savez_compressed(HERE / "state.npz", **out)


def make_chain():
    """F12: gradients out of the final discharge state and the reported geometry (the reference's autograd):
    (a) two chained gauge-mode batches -- the second carries the first one's ``_discharge_t`` with its graph
    (mmc.py:330-333, 433-441) and the loss is on both; (b) gauge mode and (c) all-output mode, one batch, the
    loss also on ``_discharge_t``, ``top_width`` and ``side_slope`` (mmc.py:161-162, 441)."""
    _, mmc = load_reference()
    net = synthetic.random_binary_tree(90, seed=31)
    T = 24
    attrs = synthetic.reach_attributes(net.n, 31)
    u = synthetic.unit_parameters(net.n, 31)
    rng = np.random.default_rng(3100)
    outflow = [np.array([-1]), np.array([10, 20, 31]), np.array([44]), np.array([5, 59, 60])]
    flat = np.concatenate(outflow)
    offs = np.cumsum([0] + [len(o) for o in outflow])
    out = dict(n=np.int64(net.n), rows=net.rows, cols=net.cols, length=attrs.length, slope=attrs.slope, x=attrs.x,
               outflow_flat=flat, outflow_offsets=offs, **{f"u_{k}": v for k, v in u.items()})
    leaf = lambda: {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in u.items()}  # noqa: E731
    grads = lambda sp_: {f"grad_{k}": v.grad.numpy().copy() for k, v in sp_.items()}  # noqa: E731

    # (a) two chained gauge-mode batches, one engine, the carried state keeps its graph
    q1 = synthetic.lateral_inflow(net.n, T, 31)
    q2 = synthetic.lateral_inflow(net.n, T, 31, t0=T)
    W1 = rng.uniform(0, 1, (len(outflow), T)).astype(np.float32)
    W2 = rng.uniform(0, 1, (len(outflow), T)).astype(np.float32)
    dc = routing_dc(net.n, net.rows, net.cols, attrs, outflow)
    mc = mmc.MuskingumCunge(cfg_of(PARAMS_DEFAULT), device="cpu")
    spa = leaf()
    mc.setup_inputs(dc, torch.from_numpy(q1), spa)
    o1 = mc.forward()
    mc.setup_inputs(dc, torch.from_numpy(q2), spa, carry_state=True)
    o2 = mc.forward()
    ((o1 * torch.from_numpy(W1)).sum() + (o2 * torch.from_numpy(W2)).sum()).backward()
    out.update(qprime_a1=q1, qprime_a2=q2, W_a1=W1, W_a2=W2, ref_a_out1=o1.detach().numpy(),
               ref_a_out2=o2.detach().numpy(), **{f"ref_a_{k}": v for k, v in grads(spa).items()})

    # (b) gauge mode / (c) all-output mode: loss on the output, _discharge_t, top_width and side_slope
    for tag, ofx in (("b", outflow), ("c", None)):
        qb = synthetic.lateral_inflow(net.n, T, 32 if tag == "b" else 33)
        G = len(ofx) if ofx is not None else net.n
        Wb = rng.uniform(0, 1, (G, T)).astype(np.float32)
        V = rng.uniform(-1, 1, (3, net.n)).astype(np.float32)
        dcb = routing_dc(net.n, net.rows, net.cols, attrs, ofx)
        mcb = mmc.MuskingumCunge(cfg_of(PARAMS_DEFAULT), device="cpu")
        spb = leaf()
        mcb.setup_inputs(dcb, torch.from_numpy(qb), spb)
        ob = mcb.forward()
        Vt = torch.from_numpy(V)
        loss = ((ob * torch.from_numpy(Wb)).sum() + (mcb._discharge_t * Vt[0]).sum() + (mcb.top_width * Vt[1]).sum()
                + (mcb.side_slope * Vt[2]).sum())
        loss.backward()
        out.update({f"qprime_{tag}": qb, f"W_{tag}": Wb, f"V_{tag}": V, f"ref_{tag}_out": ob.detach().numpy(),
                    f"ref_{tag}_q_last": mcb._discharge_t.detach().numpy(),
                    f"ref_{tag}_top_width": mcb.top_width.detach().numpy(),
                    f"ref_{tag}_side_slope": mcb.side_slope.detach().numpy(),
                    **{f"ref_{tag}_{k}": v for k, v in grads(spb).items()}})
    np.savez_compressed(HERE / "chain.npz", **out)


def make_timestep_geo():
    """F13: a 3-step ``route_timestep`` chain (the BMI update) whose loss includes every step's reported
    ``top_width`` / ``side_slope`` -- the geometry of the carried ``_discharge_t`` the step starts from
    (mmc.py:527-538, 161-162), so the geometry's gradient reaches the carried state, unclamped (two carried
    values below q_lb), and through it every earlier step."""
    _, mmc = load_reference()
    net = synthetic.random_binary_tree(90, seed=41)
    attrs = synthetic.reach_attributes(net.n, 41)
    u = synthetic.unit_parameters(net.n, 41)
    rng = np.random.default_rng(4100)
    dc = routing_dc(net.n, net.rows, net.cols, attrs)
    mc = mmc.MuskingumCunge(cfg_of(PARAMS_DEFAULT), device="cpu")
    sp = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in u.items()}
    qc = synthetic.lateral_inflow(net.n, 3, 41)
    mc.setup_inputs(dc, torch.from_numpy(qc), sp)
    q0 = rng.uniform(0.5, 5.0, net.n).astype(np.float32)
    q0[[7, 30]] = np.float32(2e-5)
    s0 = torch.from_numpy(q0).clone().requires_grad_(True)
    mc._discharge_t = s0
    mapper, _, _ = mc.create_pattern_mapper()
    W = rng.uniform(0, 1, (3, net.n)).astype(np.float32)
    V = rng.uniform(-1, 1, (3, 2, net.n)).astype(np.float32)
    qcl = [torch.from_numpy(np.maximum(qc[k], np.float32(1e-4))).clone().requires_grad_(True) for k in range(3)]
    loss = 0.0
    states, tws, sss = [], [], []
    for k in range(3):
        q1 = mc.route_timestep(q_prime_clamp=qcl[k], mapper=mapper)
        loss = loss + (q1 * torch.from_numpy(W[k])).sum() + (mc.top_width * torch.from_numpy(V[k, 0])).sum() \
            + (mc.side_slope * torch.from_numpy(V[k, 1])).sum()
        states.append(q1.detach().numpy().copy())
        tws.append(mc.top_width.detach().numpy().copy())
        sss.append(mc.side_slope.detach().numpy().copy())
        mc._discharge_t = q1
    loss.backward()
    np.savez_compressed(HERE / "timestep_geo.npz", n=np.int64(net.n), rows=net.rows, cols=net.cols,
                        length=attrs.length, slope=attrs.slope, x=attrs.x, **{f"u_{k}": v for k, v in u.items()},
                        qprime=qc, q0=q0, W=W, V=V, ref_states=np.stack(states), ref_top_width=np.stack(tws),
                        ref_side_slope=np.stack(sss), ref_grad_q0=s0.grad.numpy().copy(),
                        ref_grad_qclamp=np.stack([q.grad.numpy().copy() for q in qcl]),
                        **{f"ref_grad_{k}": v.grad.numpy().copy() for k, v in sp.items()})


def make_confluence():
    """The reference on a network whose reaches take up to 20 inflows (tests/confluence_cases.py ``bushy``; the
    other routing fixtures stop at two): 300 reaches x 48 steps, learned n / q / p, per-reach outputs; a second
    leg carried from the first one's final state; a hot-started gauge-mode run with gauges on confluences; and
    the canonical CSR + PatternMapper layout.  q' and W are regenerated from their seeds by the tests
    (``confluence_cases.golden_confluence``), which check the stored sums."""
    sys.path.insert(0, str(HERE.parent))
    import confluence_cases as cc

    torch.manual_seed(0)
    _, mmc = load_reference()
    seed, T = cc.GOLDEN_SEED, cc.T
    net = cc.bushy(cc.GOLDEN_N, seed)
    inputs, res, mc, dc = case(mmc, PARAMS_DEFAULT, net, T, seed)
    u = {k: inputs[f"u_{k}"] for k in ("n", "q_spatial", "p_spatial")}
    q2 = synthetic.lateral_inflow(net.n, T, seed, t0=T)
    W2 = np.random.default_rng(cc.GOLDEN_W2_SEED).uniform(0, 1, (net.n, T)).astype(np.float32)
    res2, _ = run_ref(mmc, PARAMS_DEFAULT, dc, q2, u, W2, carry_from=mc._discharge_t.detach().clone())
    outflow = cc.golden_gauges(net)
    inputs_g, res_g, _, _ = case(mmc, PARAMS_DEFAULT, net, T, seed, outflow_idx=outflow)
    for k in ("length", "slope", "x", "qprime", "u_n", "u_q_spatial", "u_p_spatial"):
        np.testing.assert_array_equal(inputs[k], inputs_g[k])
    c = mapper_csr(mmc, net.n, net.rows, net.cols)
    small = {k: v for k, v in inputs.items() if k not in ("qprime", "W")}
    f8 = lambda a: np.float64(a.astype(np.float64).sum())  # noqa: E731
    np.savez_compressed(HERE / "confluence.npz", **small, T=np.int64(T), qprime_sum=f8(inputs["qprime"]),
                        W_sum=f8(inputs["W"]), qprime2_sum=f8(q2), W2_sum=f8(W2), Wg_sum=f8(inputs_g["W"]),
                        outflow_flat=np.concatenate(outflow).astype(np.int64),
                        outflow_offsets=np.cumsum([0] + [len(o) for o in outflow]).astype(np.int64),
                        **{f"ref_{k}": v for k, v in res.items()}, **{f"ref2_{k}": v for k, v in res2.items()},
                        **{f"refg_{k}": v for k, v in res_g.items()},
                        crow=c[0], col=c[1], mcrow=c[2], mcol=c[3], mapidx=c[4])
    print("confluence.npz", (HERE / "confluence.npz").stat().st_size)


def main():
    if len(sys.argv) > 1:
        for name in sys.argv[1:]:
            {"geostats": make_geostats, "geostats_edges": make_geostats_edges, "daily": make_daily, "collate": make_collate, "deep": make_deep,
             "state": make_state, "chain": make_chain, "timestep_geo": make_timestep_geo,
             "confluence": make_confluence}[name]()
        return
    torch.manual_seed(0)
    utils, mmc = load_reference()
    np.savez_compressed(HERE / "kat.npz", **kat(utils, mmc))

    # F2 Sandbox: 10,20 -> 30 ; 30,40 -> 50 ; order [10, 20, 40, 30, 50] -> indices 0..4
    rows = np.array([3, 3, 4, 4], np.int32)
    cols = np.array([0, 1, 2, 3], np.int32)
    net = synthetic.SyntheticNetwork(5, rows, cols, np.array([5]))
    inputs, res, _, _ = case(mmc, PARAMS_MOCK, net, 80, 11, learn_p=False)
    np.savez_compressed(HERE / "sandbox.npz", **inputs, **{f"ref_{k}": v for k, v in res.items()})

    # F3 300-reach tree, learned p
    net3 = synthetic.random_binary_tree(300, seed=3)
    inputs, res, _, _ = case(mmc, PARAMS_DEFAULT, net3, 40, 3)
    np.savez_compressed(HERE / "tree300.npz", **inputs, **{f"ref_{k}": v for k, v in res.items()})

    # F4 gauge mode + carry_state
    net4 = synthetic.random_binary_tree(60, seed=4)
    outflow = [np.array([-1]), np.array([10, 20, 31]), np.array([45]), np.array([5, 59])]
    inputs, res, mc, dc = case(mmc, PARAMS_DEFAULT, net4, 30, 4, outflow_idx=outflow)
    q2 = synthetic.lateral_inflow(net4.n, 30, 4, t0=30)
    u = {k: inputs[f"u_{k}"] for k in ("n", "q_spatial", "p_spatial")}
    W2 = np.random.default_rng(99).uniform(0, 1, (len(outflow), 30)).astype(np.float32)
    res2, _ = run_ref(mmc, PARAMS_DEFAULT, dc, q2, u, W2, carry_from=mc._discharge_t.detach().clone())
    flat = np.concatenate(outflow)
    offs = np.cumsum([0] + [len(o) for o in outflow])
    np.savez_compressed(HERE / "gauge.npz", **inputs, outflow_flat=flat, outflow_offsets=offs,
                        qprime2=q2, W2=W2, **{f"ref_{k}": v for k, v in res.items()},
                        **{f"ref2_{k}": v for k, v in res2.items()})

    # F5 C1 shape
    net5 = synthetic.random_binary_tree(2000, seed=0)
    inputs, res, _, _ = case(mmc, PARAMS_DEFAULT, net5, 720, 0)
    sample = np.arange(0, 2000, 37)
    qsum = np.float64(inputs["qprime"].astype(np.float64).sum())
    small = {k: v for k, v in inputs.items() if k not in ("qprime", "W")}
    np.savez_compressed(HERE / "c1.npz", **small, qprime_sum=qsum, W_seed=np.int64(4000), sample=sample,
                        ref_runoff_sample=res["runoff"][sample], ref_outlet=res["runoff"][-1],
                        ref_q_last=res["q_last"], ref_top_width=res["top_width"],
                        ref_side_slope=res["side_slope"], ref_grad_n=res["grad_n"],
                        ref_grad_q_spatial=res["grad_q_spatial"], ref_grad_p_spatial=res["grad_p_spatial"])

    # F6 canonical CSR + PatternMapper layout
    c3 = mapper_csr(mmc, 300, net3.rows, net3.cols)
    c5 = mapper_csr(mmc, 2000, net5.rows, net5.cols)
    np.savez_compressed(HERE / "csr.npz", t300_crow=c3[0], t300_col=c3[1], t300_mcrow=c3[2], t300_mcol=c3[3],
                        t300_mapidx=c3[4], c1_crow=c5[0], c1_col=c5[1], c1_mcrow=c5[2], c1_mcol=c5[3],
                        c1_mapidx=c5[4])
    make_geostats()
    make_geostats_edges()
    make_daily()
    make_state()
    make_chain()
    make_timestep_geo()
    for f in sorted(HERE.glob("*.npz")):
        print(f.name, f.stat().st_size)


if __name__ == "__main__":
    main()
