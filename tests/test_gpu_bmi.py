"""GPU tests of the BMI coupling (``ddr_amd.bmi.DdrBmi``, ``csrc/bmi.hip``).

* the nexus scatter, the direct / indexed ``set_value`` branches and the sub-step window, bitwise against NumPy
  restatements of the reference's loops (``ddr_bmi.py:417-447, 270-281, 313-318``);
* the one-launch-per-interval routing against the same work done call by call on ``MuskingumCunge`` --
  ``compute_hotstart_discharge`` + clamp + a ``route_timestep`` loop, the reference's ``update_until`` -- bitwise;
* the reference's own results (``tests/golden/bmi.npz``, from its ``DdrBmi`` on CPU) at the bar the existing
  ``route_timestep`` chain tests hold, max-rel 1e-4, with the time and inflow bookkeeping exact;
* velocity and depth of the output kernel against the float64 evaluation of the same expressions: at most twice
  the reference fp32 result's own error, both measured here;
* the BMI contract: pointer stability, in-place refresh, no-op updates, cleared inflows, finalize.
"""

from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import PARAMS_DEFAULT, load_golden, maxrel
from ddr_amd import _lib, synthetic
from ddr_amd.bmi import DdrBmi
from ddr_amd.routing.mmc import MuskingumCunge, compute_hotstart_discharge

pytestmark = pytest.mark.gpu

ID = "land_surface_water_source__id"
FLOW = "land_surface_water_source__volume_flow_rate"
Q = "channel_exit_water_x-section__volume_flow_rate"
V = "channel_water_flow__speed"
D = "channel_water__mean_depth"
CFG = SimpleNamespace(params=SimpleNamespace(**PARAMS_DEFAULT))
CASES = {"lin": (900.0, "linear"), "con": (900.0, "constant"), "hr": (3600.0, "constant"), "span": (900.0, "linear")}


def dataclass_of(n, rows, cols, length, slope, x):
    a = sp.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, n)).tocsr()
    adj = torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)),
                                  torch.from_numpy(a.indices.astype(np.int64)), torch.from_numpy(a.data), size=(n, n))
    return SimpleNamespace(adjacency_matrix=adj, length=torch.from_numpy(length), slope=torch.from_numpy(slope),
                           x=torch.from_numpy(x), top_width=torch.empty(0), side_slope=torch.empty(0),
                           outflow_idx=None, gage_catchment=None, observations=None, flow_scale=None)


def small_bmi(N, dev, mapping=None, **kw):
    net = synthetic.random_binary_tree(N, seed=N)
    at = synthetic.reach_attributes(N, N)
    u = {k: torch.from_numpy(v).to(dev) for k, v in synthetic.unit_parameters(N, N).items()}
    b = DdrBmi()
    b.initialize_from(dataclass_of(N, net.rows, net.cols, at.length, at.slope, at.x), u, CFG,
                      nexus_to_segment=mapping, device=dev, **kw)
    return b


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ---- NumPy restatements of the reference loops --------------------------------------------------------------------
def ref_set_value(lateral, ids, mapping, src):
    if len(ids) > 0 and len(src) > 0:
        flows = src.flat[:len(ids)]
        for i, nex in enumerate(ids):
            seg = mapping.get(int(nex))
            if seg is not None:
                lateral[seg] = flows[i]
    else:
        n = min(len(src.flat), len(lateral))
        lateral[:n] = src.flat[:n]


def ref_set_at(lateral, inds, src):
    for i, idx in enumerate(inds):
        if idx < len(lateral):
            lateral[idx] = src[i]


def ref_window(prev, cur, K, linear, n_steps=None):
    n_steps = K if n_steps is None else n_steps
    rows = []
    for step in range(K):
        if linear:
            alpha = (step + 1) / n_steps
            inflow = (1.0 - alpha) * prev + alpha * cur
        else:
            inflow = cur
        rows.append(inflow.astype(np.float32))
    return np.stack(rows)


# ---- scatter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_nexus_scatter_matches_the_reference_loop(cuda, N):
    rng = np.random.default_rng(N)
    mapped = rng.permutation(N)[: max(1, (3 * N) // 4)]  # the other segments have no nexus
    mapping = {7000 + 5 * int(s): int(s) for s in mapped}
    mapping[7000 + 5 * int(mapped[0]) + 2] = int(mapped[0])  # two nexus ids of one segment
    known = np.array(sorted(mapping))
    b = small_bmi(N, cuda, mapping)
    want = np.zeros(N)
    for M in (0, 1, N, 3 * N):
        # 3N ids over fewer keys repeat ids; a tenth are unknown (among them ids below, between and above the keys)
        ids = rng.choice(known, M)
        unknown = rng.random(M) < 0.1
        ids[unknown] = rng.choice([1, 7001, 7000 + 5 * N + 9, 2**31 - 1], int(unknown.sum()))
        if M >= 2:
            ids[-1] = ids[0]  # one id certainly twice: the last flow wins
        for n_src in sorted({max(M, 1), M + 3, N, N + 2}):
            if n_src < M:
                continue
            src = rng.normal(0.0, 3.0, n_src)  # (negative flows are taken as they are)
            b.set_value(ID, ids.astype(np.int64))
            b.set_value(FLOW, src)
            ref_set_value(want, ids.astype(np.int32), mapping, src)
            got = b._lateral.cpu().numpy()
            assert np.array_equal(bits(got), bits(want)), (N, M, n_src)
    # the flows may be any shape; fewer flows than ids are refused before anything is written
    ids = known[: min(len(known), 6)]
    b.set_value(ID, ids)
    src = rng.normal(size=(2, len(ids)))
    b.set_value(FLOW, src)
    ref_set_value(want, ids.astype(np.int32), mapping, src)
    assert np.array_equal(b._lateral.cpu().numpy(), want)
    if len(ids) > 1:
        with pytest.raises(ValueError, match="flows for"):
            b.set_value(FLOW, src.reshape(-1)[: len(ids) - 1])
        assert np.array_equal(b._lateral.cpu().numpy(), want)


@pytest.mark.parametrize("N", [1, 64, 257])
def test_direct_and_indexed_assignment(cuda, N):
    rng = np.random.default_rng(100 + N)
    b = small_bmi(N, cuda)
    want = np.zeros(N)
    for n_src in (1, max(1, N // 2), N, N + 5):  # no ids set: the first min(len, N) values
        src = rng.normal(size=n_src)
        b.set_value(FLOW, src)
        ref_set_value(want, np.empty(0, np.int32), {}, src)
        assert np.array_equal(b._lateral.cpu().numpy(), want), n_src
    inds = np.concatenate([rng.integers(0, N, 2 * N + 1), [N, N + 7, 0, 0]])  # repeats; indices >= N are ignored
    rng.shuffle(inds)
    src = rng.normal(size=inds.size + 2)
    b.set_value_at_indices(FLOW, inds, src)
    ref_set_at(want, inds, src)
    assert np.array_equal(b._lateral.cpu().numpy(), want)
    b.set_value_at_indices(FLOW, np.array([N + 1]), np.array([5.0]))  # nothing in range
    b.set_value_at_indices("channel_water__id", np.array([0]), np.array([5.0]))  # another name: ignored
    assert np.array_equal(b._lateral.cpu().numpy(), want)


# ---- window -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_window_kernel_is_the_reference_interpolation(cuda, N):
    lib = _lib.load()
    rng = np.random.default_rng(200 + N)
    stream = _lib.stream_ptr(cuda)
    for K, n_steps in ((1, 1), (2, 2), (3, 3), (12, 12), (3, 7)):
        for linear in (0, 1):
            prev = rng.lognormal(0.0, 2.0, N) * rng.choice([1.0, 1.0, -1.0], N)
            cur = rng.lognormal(0.0, 2.0, N) * rng.choice([1.0, 1.0, -1.0], N)
            cur[::5] = 0.0
            stride = N + (K % 2)  # rows may be padded
            d_prev, d_cur = torch.from_numpy(prev).to(cuda), torch.from_numpy(cur).to(cuda)
            win = torch.full((K + 2, stride), -7.0, dtype=torch.float32, device=cuda)
            _lib.check(lib.ddr_bmi_window_f32(N, K, n_steps, linear, d_prev.data_ptr(), d_cur.data_ptr(),
                                              win.data_ptr(), stride, stream))
            got = win.cpu().numpy()
            want = ref_window(prev, cur, K, bool(linear), n_steps)
            assert np.array_equal(bits(got[:K, :N]), bits(want)), (K, n_steps, linear)
            assert np.array_equal(bits(got[K, :N]), bits(want[K - 1]))
            assert np.all(got[K + 1] == -7.0) and np.all(got[:, N:] == -7.0)  # nothing else is written
            assert np.array_equal(d_prev.cpu().numpy(), cur)  # ddr_bmi.py:314
            assert np.all(d_cur.cpu().numpy() == 0.0)         # ddr_bmi.py:318


def test_linear_falls_back_to_constant_on_the_first_interval(cuda):
    N, K = 65, 3
    b = small_bmi(N, cuda, timestep_seconds=1200.0, interpolation="linear")
    rng = np.random.default_rng(5)
    first, second = rng.lognormal(size=N), rng.lognormal(size=N)
    first[3] = -2.0
    b.set_value(FLOW, first)
    b.update_until(3600.0)
    assert np.array_equal(b._window[:K].cpu().numpy(), ref_window(np.zeros(N), first, K, False))
    b.set_value(FLOW, second)
    b.update_until(7200.0)
    assert np.array_equal(b._window[:K].cpu().numpy(), ref_window(first, second, K, True))
    b.set_value(FLOW, first)
    b.update_until(7200.0 + 1200.0)  # one sub-step: constant again (n_steps > 1 is required)
    assert np.array_equal(b._window[:1].cpu().numpy(), ref_window(second, first, 1, False))
    assert b.get_current_time() == 3600.0 + 3600.0 + 1200.0 and b.route_launches == 3


# ---- routing on the fixture's tree --------------------------------------------------------------------------------
def chained_reference_path(d, dc, spatial, mapping, dt, interpolation, untils, dev):
    """The reference's update_until on this package's MuskingumCunge, call by call: a host interpolation and an
    upload per sub-step, compute_hotstart_discharge on the first, clamp, route_timestep."""
    mc = MuskingumCunge(CFG, device=dev)
    mc.t = torch.tensor(dt, device=dev)
    N = len(d["length"])
    mc.setup_inputs(routing_dataclass=dc, streamflow=torch.zeros(1, N, device=dev), spatial_parameters=spatial)
    mapper, _, _ = mc.create_pattern_mapper()
    lateral, prev = np.zeros(N), np.zeros(N)
    has_prev = cold = False
    now, out = 0.0, []
    for i, until in enumerate(untils):
        ref_set_value(lateral, d["ids"], mapping, d["flows"][i])
        n_steps = max(1, round((until - now) / dt))
        linear = interpolation == "linear" and has_prev and n_steps > 1
        for step in range(n_steps):
            alpha = (step + 1) / n_steps
            inflow = (1.0 - alpha) * prev + alpha * lateral if linear else lateral
            q_prime = torch.tensor(inflow, dtype=torch.float32, device=dev)
            if not cold:
                mc._discharge_t = compute_hotstart_discharge(q_prime, mapper, mc.discharge_lb, dev)
                cold = True
            with torch.no_grad():
                mc._discharge_t = mc.route_timestep(q_prime_clamp=torch.clamp(q_prime, min=1e-4), mapper=mapper)
            now += dt
        prev[:] = lateral
        has_prev = True
        lateral[:] = 0.0
        out.append({"discharge": mc._discharge_t.cpu().numpy(), "top_width": mc.top_width.cpu().numpy(),
                    "side_slope": mc.side_slope.cpu().numpy()})
    return out


@pytest.fixture(scope="module")
def runs(cuda):
    """Every fixture case run once through DdrBmi and once through the chained path; shared by the tests below."""
    d = load_golden("bmi")
    N = len(d["length"])
    dc = dataclass_of(N, d["rows"], d["cols"], d["length"], d["slope"], d["x"])
    spatial = {k: torch.from_numpy(d[f"u_{k}"]).to(cuda) for k in ("n", "q_spatial", "p_spatial")}
    mapping = {int(k): int(s) for k, s in zip(d["map_keys"], d["map_segs"])}
    res = {}
    for name, (dt, interpolation) in CASES.items():
        untils = d[f"{name}_until"]
        b = DdrBmi()
        b.initialize_from(dc, spatial, CFG, nexus_to_segment=mapping, timestep_seconds=dt,
                          interpolation=interpolation, device=cuda)
        b.set_value(ID, d["ids"])
        calls = []
        for i, until in enumerate(untils):
            b.set_value(FLOW, d["flows"][i])
            lat_in = b._lateral.cpu().numpy()
            b.update_until(float(until))
            calls.append({"discharge": b.get_value_ptr(Q).copy(), "velocity": b.get_value_ptr(V).copy(),
                          "depth": b.get_value_ptr(D).copy(), "top_width": b._mc.top_width.cpu().numpy(),
                          "side_slope": b._mc.side_slope.cpu().numpy(), "time": b.get_current_time(),
                          "prev": b._prev.cpu().numpy(), "cur": b._lateral.cpu().numpy(), "lat_in": lat_in,
                          "static": [t.cpu().numpy() for t in (*b._static, b._p)]})
        assert b.route_launches == len(untils)  # one routing launch per coupling interval, whatever K is
        res[name] = (calls, chained_reference_path(d, dc, spatial, mapping, dt, interpolation, untils, cuda))
    return d, res


@pytest.mark.parametrize("name", list(CASES))
def test_one_launch_equals_chained_route_timestep(runs, name):
    """A window of K + 1 rows from the carried state is K chained route_timestep calls, and the cold start's
    step 0 is compute_hotstart_discharge on the raw first row: the same fp32 operations on the same fp32 state
    and inflow, so the same bits."""
    _, res = runs
    calls, chained = res[name]
    for i, (got, want) in enumerate(zip(calls, chained)):
        for k in ("discharge", "top_width", "side_slope"):
            print(name, i, k, "max-rel vs the chained path", maxrel(got[k], want[k]))
            assert np.array_equal(bits(got[k]), bits(want[k])), (name, i, k)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_parity(runs, name):
    d, res = runs
    calls, _ = res[name]
    lb = np.float32(PARAMS_DEFAULT["attribute_minimums"]["discharge"])
    for i, got in enumerate(calls):
        for k in ("discharge", "top_width", "side_slope"):
            err = maxrel(got[k], d[f"{name}_{k}"][i])
            print(name, i, k, "max-rel vs the reference", err)
            assert err <= 1e-4, (name, i, k, err)
        assert got["time"] == float(d[f"{name}_time"][i])
        assert np.array_equal(bits(got["prev"]), bits(d[f"{name}_prev"][i]))
        assert np.array_equal(bits(got["cur"]), bits(d[f"{name}_cur"][i]))
        assert np.array_equal(bits(got["lat_in"]), bits(d["lat_in"][i]))
        # the clamps are active where the reference's are: unmapped headwaters sit at the discharge bound
        at_lb = d[f"{name}_discharge"][i] == lb
        assert at_lb.any() and np.all(got["discharge"][at_lb] == lb)


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_are_the_kernel_on_the_engine_state(runs, cuda, name):
    """What get_value_ptr holds after a call is the output kernel on the engine's discharge, reported geometry and
    parameters (the wiring of update_until; the kernel's accuracy is measured below)."""
    _, res = runs
    for got in res[name][0]:
        n, qs, s0, p = got["static"]
        out = run_outputs(cuda, got["discharge"], n, qs, p, s0, got["top_width"], got["side_slope"],
                          p_stride=0 if len(p) == 1 else 1)
        for row, k in enumerate(("discharge", "velocity", "depth")):
            assert np.array_equal(bits(out[row]), bits(got[k])), (name, k)


# ---- velocity and depth -------------------------------------------------------------------------------------------
def run_outputs(dev, q, n, qs, p, s0, tw, z, depth_lb=0.01, bw_lb=0.01, p_stride=1):
    N = len(q)
    t = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in (q, n, qs, p, s0, tw, z)]
    out = torch.full((3, N), -1.0, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().ddr_bmi_outputs_f32(N, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                               p_stride, t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), depth_lb,
                                               bw_lb, out.data_ptr(), N, _lib.stream_ptr(dev)))
    return out.cpu().numpy()


def test_velocity_and_depth_error_against_float64(cuda):
    """The kernel's largest relative error over every call of every fixture case against twice the reference fp32
    result's own.  Measured on an MI355X: depth 4.13e-7 against 4.13e-7, velocity 2.79e-7 against 2.79e-7 (ratios
    1.000 and 1.000)."""
    d = load_golden("bmi")
    lb32 = np.float32(0.01)
    worst = {"depth": [0.0, 0.0], "velocity": [0.0, 0.0]}
    for name in CASES:
        for i in range(len(d[f"{name}_until"])):
            q, tw, z = (d[f"{name}_{k}"][i] for k in ("discharge", "top_width", "side_slope"))
            out = run_outputs(cuda, q, d["n"], d["q_spatial"], d["p_spatial"], d["slope_c"], tw, z)
            assert np.array_equal(bits(out[0]), bits(q))  # the discharge copy
            for row, k in ((2, "depth"), (1, "velocity")):
                exact = d[f"{name}_{k}64"][i]
                worst[k][0] = max(worst[k][0], maxrel(out[row], exact))
                worst[k][1] = max(worst[k][1], maxrel(d[f"{name}_{k}"][i], exact))
            clamped = d[f"{name}_depth64"][i] == np.float64(lb32)
            assert clamped.any() and np.all(out[2][clamped] == lb32)
            for bound in (0.0, 15.0):
                at = d[f"{name}_velocity64"][i] == bound
                assert np.all(out[1][at] == np.float32(bound))
    for k, (kernel, reference) in worst.items():
        print(f"{k}: kernel max-rel {kernel:.3e}, reference fp32 max-rel {reference:.3e}, ratio "
              f"{kernel / reference:.3f}")
        assert kernel <= 2.0 * reference, (k, kernel, reference)


def test_velocity_clamp_and_scalar_p(cuda):
    # a steep smooth channel in flood runs far above 15 m/s in exact arithmetic: the clamp value itself comes out
    N = 70
    rng = np.random.default_rng(3)
    q = rng.uniform(2e3, 2e4, N).astype(np.float32)
    n = np.full(N, 0.015, np.float32)
    qs = rng.uniform(0.2, 0.6, N).astype(np.float32)
    s0 = np.full(N, 0.5, np.float32)
    p = np.full(N, 21.0, np.float32)
    tw = rng.uniform(30.0, 60.0, N).astype(np.float32)
    z = rng.uniform(0.5, 2.0, N).astype(np.float32)
    f = lambda a: a.astype(np.float64)  # noqa: E731
    qe = f(qs) + 1e-6
    depth = np.maximum((f(q) * f(n) * (qe + 1) / (f(p) * np.sqrt(f(s0)) + 1e-8)) ** (3.0 / (5.0 + 3.0 * qe)), 0.01)
    bw = np.maximum(f(tw) - 2 * f(z) * depth, 0.01)
    v = (1.0 / f(n)) * (((f(tw) + bw) * depth / 2) / (bw + 2 * depth * np.sqrt(1 + f(z) ** 2))) ** (2.0 / 3.0) \
        * np.sqrt(f(s0))
    assert v.min() > 20.0
    out = run_outputs(cuda, q, n, qs, p, s0, tw, z)
    assert np.all(out[1] == np.float32(15.0))
    # fp32 depth: five roundings of 2^-24 in the ratio and three in the exponent, through a power of at most 0.6
    # with |exponent ln ratio| < 2, and the final rounding -- under 6e-7 in all
    assert maxrel(out[2], depth) <= 1e-6
    one = run_outputs(cuda, q, n, qs, p[:1], s0, tw, z, p_stride=0)  # one p for every segment
    assert np.array_equal(bits(one), bits(out))


# ---- initialize from files ----------------------------------------------------------------------------------------
def test_initialize_from_config_files(cuda, tmp_path, monkeypatch):
    """initialize(): the BMI YAML, DDR's YAML, a KAN checkpoint run once, the nexus mapping from a GeoPackage and
    the dataset_factory hook -- the same model as initialize_from with those pieces, bit for bit."""
    import sqlite3

    from ddr_amd.nn.kan import kan

    N = 65
    net = synthetic.random_binary_tree(N, seed=N)
    at = synthetic.reach_attributes(N, N)
    dc = dataclass_of(N, net.rows, net.cols, at.length, at.slope, at.x)
    dc.divide_ids = np.array([f"cat-{100 + i}" for i in range(N)])
    dc.normalized_spatial_attributes = torch.from_numpy(
        np.random.default_rng(1).normal(size=(N, 3)).astype(np.float32))
    arch = dict(input_var_names=["a", "b", "c"], learnable_parameters=["n", "q_spatial", "p_spatial"], hidden_size=5,
                num_hidden_layers=1, grid=3, k=3)
    model = kan(**arch, seed=4, device=cuda)
    with torch.no_grad():
        model.flat.add_(0.3 * torch.randn(model.flat.shape, generator=torch.Generator().manual_seed(2)).to(cuda))
    torch.save({"model_state_dict": model.state_dict(), "epoch": 1}, tmp_path / "kan.pt")
    gpkg = tmp_path / "hf.gpkg"
    con = sqlite3.connect(str(gpkg))
    con.execute("CREATE TABLE flowpaths (id TEXT, toid TEXT)")
    con.executemany("INSERT INTO flowpaths VALUES (?, ?)", [(f"wb-{100 + i}", f"nex-{500 + 2 * i}") for i in range(N)])
    con.commit()
    con.close()
    import yaml

    (tmp_path / "ddr.yaml").write_text(yaml.safe_dump(
        {"seed": 4, "kan": arch, "data_sources": {"geospatial_fabric_gpkg": "elsewhere.gpkg"}}))
    (tmp_path / "bmi.yaml").write_text(yaml.safe_dump(
        {"ddr_config": str(tmp_path / "ddr.yaml"), "kan_checkpoint": str(tmp_path / "kan.pt"),
         "hydrofabric_gpkg": str(gpkg), "device": "cuda:0", "timestep_seconds": 1800.0, "interpolation": "linear"}))
    seen = {}

    def factory(cfg):
        seen.update(device=cfg.device, mode=cfg.mode, gpkg=cfg.data_sources.geospatial_fabric_gpkg)
        return dc

    monkeypatch.setattr(DdrBmi, "dataset_factory", factory)
    b = DdrBmi()
    b.initialize(str(tmp_path / "bmi.yaml"))
    assert seen == {"device": "cuda:0", "mode": "route", "gpkg": str(gpkg)}
    mapping = {500 + 2 * i: i for i in range(N)}
    assert b._nexus_to_seg_idx == mapping
    assert np.array_equal(b.get_value_ptr("channel_water__id"), 100 + np.arange(N))
    assert b.get_time_step() == 1800.0 and b._interpolation == "linear" and b.get_grid_size(0) == N

    with torch.no_grad():
        spatial = model(inputs=dc.normalized_spatial_attributes.to(cuda))
    b2 = DdrBmi()
    b2.initialize_from(dc, spatial, CFG, nexus_to_segment=mapping, timestep_seconds=1800.0, interpolation="linear",
                       device=cuda)
    rng = np.random.default_rng(7)
    ids = (500 + 2 * rng.permutation(N)).astype(np.int32)
    for m in (b, b2):
        m.set_value(ID, ids)
    for i in range(2):
        flows = rng.lognormal(size=N)
        for m in (b, b2):
            m.set_value(FLOW, flows)
            m.update_until(3600.0 * (i + 1))
        for name in (Q, V, D):
            assert np.array_equal(bits(b.get_value_ptr(name)), bits(b2.get_value_ptr(name))), (i, name)
    assert np.all(b.get_value_ptr(Q) > 0)


# ---- the BMI contract ---------------------------------------------------------------------------------------------
def test_bmi_contract(cuda):
    N = 63
    b = small_bmi(N, cuda, timestep_seconds=900.0)
    ptrs = {name: b.get_value_ptr(name) for name in b.get_output_var_names()}
    assert ptrs[Q].dtype == np.float32 and ptrs["channel_water__id"].dtype == np.int64
    assert all(len(p) == N for p in ptrs.values())
    assert np.array_equal(ptrs["channel_water__id"], np.arange(N))
    assert b.get_grid_size(0) == N and b.get_grid_node_count(0) == N and b.get_grid_edge_count(0) == N - 1
    rng = np.random.default_rng(0)
    flows = rng.lognormal(size=N)
    b.set_value(FLOW, flows)
    b.update_until(0.0)    # nothing remains: no routing, and the inflows stay pending
    b.update_until(-50.0)
    assert b.route_launches == 0 and b.get_current_time() == 0.0
    assert np.array_equal(b._lateral.cpu().numpy(), flows) and np.all(ptrs[Q] == 0.0)
    b.update_until(3600.0)
    assert b.route_launches == 1 and b.get_current_time() == 3600.0
    assert np.all(b._lateral.cpu().numpy() == 0.0)  # cleared: ngen sends them again
    assert np.array_equal(b._prev.cpu().numpy(), flows)
    first = {k: v.copy() for k, v in ptrs.items()}
    assert np.all(first[Q] > 0) and np.all(first[V] > 0) and np.all(first[D] >= np.float32(0.01))
    b.set_value(FLOW, 3.0 * flows)
    b.update()             # one routing step
    assert b.get_current_time() == 4500.0
    for name, p in ptrs.items():
        assert b.get_value_ptr(name) is p  # the same array object, refilled in place
    assert not np.array_equal(ptrs[Q], first[Q]) and not np.array_equal(ptrs[D], first[D])
    dest = np.empty(N, np.float32)
    assert b.get_value(Q, dest) is dest and np.array_equal(dest, ptrs[Q])
    assert np.array_equal(b.get_value(V, np.empty(5, np.float32)), ptrs[V][:5])
    inds = np.array([N - 1, 0, 7])
    assert np.array_equal(b.get_value_at_indices(D, np.empty(3, np.float32), inds), ptrs[D][inds])
    with pytest.raises(ValueError, match="Unknown output variable"):
        b.get_value(FLOW, dest)
    b.finalize()
    with pytest.raises(RuntimeError, match="not initialized"):
        b.update()
    assert b.get_value_ptr(Q) is ptrs[Q]
