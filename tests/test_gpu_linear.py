"""Linear Muskingum routing on the device (``ddr_amd.routing.LinearMuskingum``, route_linear.hip) against the host
model of tests/linear_cases.py.  Every comparison with the model is bit for bit, in fp32 and in fp64: nothing in
the tick is approximate.

  sandbox      RAPID2's published Sandbox run through ``Network.build``: ``Qout``, ``Qfinal``, the steady start
  partitions   one, two and four reaches per thread, with and without cut edges: the same bits as the model
  time axis    (F, S) short and long, F * S around the deepest block's depth and an import chunk, both outputs
  confluences  reaches of three and more inflows, local and over cut edges: the upstream order
  carry        q_last -> q0 over chunks equals the one-shot route
  gauges       gauge rows, flow_scale and the valid mask
  physics      mass balance and linearity within fp32 rounding
  capture      a captured route replays the eager result
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import confluence_cases as CC
import linear_cases as LC
import time_axis_cases as TA
from ddr_amd import synthetic
from ddr_amd._lib import DDR_ERR_CAPACITY, DDRError
from ddr_amd.graph import RiverGraph
from ddr_amd.network import Network
from ddr_amd.ops import GaugeMap
from ddr_amd.routing import LinearMuskingum

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
# block caps of the 3758-reach forest by precision.  Four reaches per thread in fp64 need a block of more than 2048
# reaches whose slots (56 B each) still fit the LDS, at most ~2860: the forest's 3758-reach block of cap 4096 does
# not (refused, tested below), so fp64 runs four per thread on one 2500-reach tree ("T4") instead
L_CAPS = {"f32": {256: 1, 1536: 2, 4096: 4}, "f64": {256: 1, 1536: 2}}
DT = 900.0


def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, ref, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, got.shape, ref.dtype, ref.shape)
    bad = np.flatnonzero(bits(got).ravel() != bits(ref).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size} differ, first at {bad[0]}: " \
                          f"{got.ravel()[bad[0]]!r} vs {ref.ravel()[bad[0]]!r}"


@functools.lru_cache(maxsize=None)
def topo_of(name):
    if name == "T4":
        net = synthetic.random_binary_tree(2500, 8)
    else:
        net = TA.network(name) if name in ("S", "L") else CC.network(name)
    return net, LC.Topology.of_coo(net.n, net.rows, net.cols)


@functools.lru_cache(maxsize=None)
def model(name, F, S, prec, q0kind="zero", scale=False):
    """The host model of a network's standard case (read-only, shared)."""
    net, topo = topo_of(name)
    npd = DTYPES[prec][1]
    k, x = LC.parameters(net.n, 1, npd)
    q = LC.random_forcing(net.n, F, 2, npd)
    fs, valid = scale_inputs(net.n, npd) if scale else (None, None)
    q0 = {"zero": None, "steady": "steady", "array": start_state(net.n, npd)}[q0kind]
    return LC.route(topo, k, x, DT, S, LC.forcing(q, npd, fs, valid), q0=q0, dtype=npd)


def start_state(n, npd):
    return np.random.default_rng(77).uniform(0.0, 9.0, n).astype(npd)


def scale_inputs(n, npd):
    rng = np.random.default_rng(78)
    valid = np.ones(n, np.uint8)
    valid[rng.choice(n, 7, replace=False)] = 0
    return rng.uniform(0.5, 1.5, n).astype(npd), valid


def router(name, gkw, prec, dev, S):
    net, _ = topo_of(name)
    npd = DTYPES[prec][1]
    g = RiverGraph(net.n, net.rows, net.cols, **gkw)
    k, x = LC.parameters(net.n, 1, npd)
    return g, LinearMuskingum(g, dev_t(k, dev), dev_t(x, dev), dt=DT, substeps=S)


def check_case(name, gkw, prec, dev, F, S, q0kind="zero", kr=None):
    net, _ = topo_of(name)
    npd = DTYPES[prec][1]
    g, lm = router(name, gkw, prec, dev, S)
    if kr is not None:
        assert g.info.reaches_per_thread == kr, g
    q = dev_t(LC.random_forcing(net.n, F, 2, npd), dev)
    q0 = {"zero": None, "steady": "steady", "array": None}[q0kind]
    if q0kind == "array":
        q0 = dev_t(start_state(net.n, npd), dev)
    ref = model(name, F, S, prec, q0kind)
    for output in ("mean", "end"):
        out, q_last = lm(q, q0=q0, output=output)
        same_bits(out, ref[output], f"{name} {gkw} {prec} F={F} S={S} {q0kind} {output}")
        same_bits(q_last, ref["q_last"], f"{name} {gkw} {prec} F={F} S={S} {q0kind} q_last")
    return g


# ---- RAPID's Sandbox ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sandbox_case(cuda):
    d = LC.sandbox()
    net = Network.build(d["ids"], d["next_down"])
    g = RiverGraph(net.n, net.rows, net.cols)
    return d, net, g


def test_sandbox_fp64_reproduces_rapid(cuda, sandbox_case):
    d, net, g = sandbox_case
    lm = LinearMuskingum(g, float(d["k"]), float(d["x"]), dt=float(d["dt"]), substeps=int(d["substeps"]))
    q = dev_t(net.align(d["qext"], axis=1).astype(np.float64), cuda)
    out, q_last = lm(q, q0=dev_t(net.align(d["qinit"]), cuda))
    same_bits(out.cpu().numpy().astype(np.float32).T.copy(), np.ascontiguousarray(net.align(d["qout"], axis=1)), "Qout")
    ref = net.align(d["qfinal"])
    rel = float(np.max(np.abs(q_last.cpu().numpy() - ref) / np.abs(ref)))
    print(f"q_last vs Qfinal: {rel:.3e}")
    assert rel <= 1e-15


def test_sandbox_fp32_equals_the_model(cuda, sandbox_case):
    d, net, g = sandbox_case
    topo = LC.Topology.of_graph(g)
    lm = LinearMuskingum(g, float(d["k"]), float(d["x"]), dt=float(d["dt"]), substeps=int(d["substeps"]))
    qe, q0 = net.align(d["qext"], axis=1), net.align(d["qinit"]).astype(np.float32)
    ref = LC.route(topo, float(d["k"]), float(d["x"]), float(d["dt"]), int(d["substeps"]), qe, q0=q0, dtype=np.float32)
    for output in ("mean", "end"):
        out, q_last = lm(dev_t(qe, cuda), q0=dev_t(q0, cuda), output=output)
        same_bits(out, ref[output], f"sandbox fp32 {output}")
        same_bits(q_last, ref["q_last"], "sandbox fp32 q_last")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sandbox_steady_start_stays_steady(cuda, sandbox_case, prec):
    """Constant forcing [9, 9, 9, 18, 18] from q0="steady": the state is [9, 9, 27, 18, 63] at every interval.
    The coefficients -0.25, 0.375, 0.875 and every product are exact, so this is exact."""
    d, net, g = sandbox_case
    tdt, npd = DTYPES[prec]
    lm = LinearMuskingum(g, float(d["k"]), float(d["x"]), dt=float(d["dt"]), substeps=int(d["substeps"]))
    F = 6
    q = np.tile(net.align(np.array([9, 9, 9, 18, 18], npd)), (F, 1))
    want = np.tile(net.align(np.array([9, 9, 27, 18, 63], npd))[:, None], (1, F))
    for output in ("mean", "end"):
        out, q_last = lm(dev_t(q, cuda), q0="steady", output=output)
        same_bits(out, want, f"steady {output}")
        same_bits(q_last, np.ascontiguousarray(want[:, 0]), "steady q_last")


# ---- partitions ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("part", ["whole", "cut"])
def test_partitions_of_the_tree(cuda, part, prec):
    g = check_case("S", TA.S_PARTS[part], prec, cuda, 17, 3)
    assert g.info.n_cut == (9 if part == "cut" else 0)


@pytest.mark.parametrize("prec,cap", [(p, c) for p in ("f32", "f64") for c in L_CAPS[p]])
def test_partitions_of_the_forest(cuda, prec, cap):
    check_case("L", {"max_block_reaches": cap, "target_blocks": 1}, prec, cuda, 17, 3, kr=L_CAPS[prec][cap])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_four_reaches_per_thread_on_one_tree(cuda, prec):
    check_case("T4", TA.WHOLE, prec, cuda, 17, 3, kr=4)


def test_fp64_block_beyond_the_lds_is_refused(cuda):
    g, lm = router("L", {"max_block_reaches": 4096, "target_blocks": 1}, "f64", cuda, 1)
    with pytest.raises(DDRError) as e:
        lm(torch.ones(2, g.n, dtype=torch.float64, device=cuda))
    assert e.value.code == DDR_ERR_CAPACITY


# ---- the time axis -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("part", ["whole", "cut"])
def test_time_axis(cuda, part, prec):
    info = TA.host_info("S", part)
    cases = LC.TIME_AXIS + LC.depth_cases(info)
    d = int(info.max_block_depth)
    assert any(F * S < d for F, S in cases) and any(F * S > d for F, S in cases)
    for F, S in cases:
        check_case("S", TA.S_PARTS[part], prec, cuda, F, S)


@pytest.mark.parametrize("q0kind", ["array", "steady"])
def test_start_states_over_cut_edges(cuda, q0kind):
    for prec in ("f32", "f64"):
        check_case("S", TA.CUT, prec, cuda, 5, 7, q0kind=q0kind)


# ---- confluences ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part", ["whole", "cut64"])
def test_confluences(cuda, part):
    net, gkw = CC.pair("bushy600", part)
    assert np.bincount(net.rows, minlength=net.n).max() >= 17
    for prec in ("f32", "f64"):
        check_case("bushy600", gkw, prec, cuda, 9, 4)
        check_case("bushy600", gkw, prec, cuda, 3, 2, q0kind="steady")


# ---- state carry ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_state_carry_equals_one_shot(cuda, prec):
    net, _ = topo_of("S")
    npd = DTYPES[prec][1]
    _, lm = router("S", TA.CUT, prec, cuda, 3)
    q = dev_t(LC.random_forcing(net.n, 17, 2, npd), cuda)
    for output in ("mean", "end"):
        whole, last = lm(q, output=output)
        parts, state = [], None
        for a, b in ((0, 5), (5, 10), (10, 17)):
            o, state = lm(q[a:b], q0=state, output=output)
            parts.append(o)
        same_bits(torch.cat(parts, dim=1), whole.cpu().numpy(), f"carry {output}")
        same_bits(state, last.cpu().numpy(), "carry q_last")
        same_bits(whole, model("S", 17, 3, prec)[output], "one shot")


# ---- gauge mode, flow_scale, valid ---------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_gauges_flow_scale_and_valid(cuda, prec):
    net, _ = topo_of("S")
    tdt, npd = DTYPES[prec]
    F, S = 6, 4
    g, lm = router("S", TA.CUT, prec, cuda, S)
    gauges = TA.gauge_sets(net.n, 3)
    gz = GaugeMap.build(gauges, net.n, cuda)
    fs, valid = scale_inputs(net.n, npd)
    q = dev_t(LC.random_forcing(net.n, F, 2, npd), cuda)
    ref = model("S", F, S, prec, "zero", True)
    assert not np.array_equal(ref["mean"], model("S", F, S, prec)["mean"])
    for output in ("mean", "end"):
        kw = dict(output=output, flow_scale=dev_t(fs, cuda), valid=dev_t(valid, cuda).bool())
        out, q_last = lm(q, **kw)
        same_bits(out, ref[output], f"scaled {output}")
        rows, q_last_g = lm(q, gauges=gz, **kw)
        assert rows.shape == (len(gauges), F)
        same_bits(rows, LC.gauge_rows(ref[output], gauges, npd), f"gauge rows {output}")
        same_bits(q_last_g, ref["q_last"], "gauge q_last")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_gauge_rows_equal_gauge_reduce(cuda, prec):
    """The gauge rows against the existing ``ddr_gauge_reduce`` over the same (N, F) output.  That reducer reads the
    schedule layout of a forward's workspace, so the output is brought into it by the forward's own forcing gather
    (an accumulation launch with the output as its q': the second half of its workspace is q'[t, reach] at the
    reach's tick of step t), and it clamps at the discharge bound, here -inf."""
    import ctypes as C

    from ddr_amd import _lib
    from ddr_amd.ops import RouteConsts, mc_route, register_graph

    net, _ = topo_of("S")
    tdt, npd = DTYPES[prec]
    F, S = 6, 4
    g, lm = router("S", TA.CUT, prec, cuda, S)
    gauges = TA.gauge_sets(net.n, 3)
    gz = GaugeMap.build(gauges, net.n, cuda)
    q = dev_t(LC.random_forcing(net.n, F, 2, npd), cuda)
    out, _ = lm(q)
    rows, _ = lm(q, gauges=gz)
    assert float(out.min()) < 0  # unclamped: the reducer must not clamp either
    one = torch.ones(net.n, device=cuda, dtype=tdt)
    res = mc_route(out.T.contiguous(), one, one, one, one, one, one, None, None, None, None, None, None, None,
                   register_graph(g), RouteConsts().as_list(), _lib.DDR_FWD_ACCUMULATE, F, 1, [])
    staged = res[4][g.state_numel(F):]
    want = torch.empty_like(rows)
    lib = _lib.load()
    red = lib.ddr_gauge_reduce_f32 if prec == "f32" else lib.ddr_gauge_reduce_f64
    gs = _lib.Gauges(len(gauges), gz.offsets.data_ptr(), gz.index.data_ptr(), None, None)
    _lib.check(red(g.handle, staged.data_ptr(), F, C.byref(gs), float("-inf"), _lib.DDR_FWD_CARRY, want.data_ptr(),
                   _lib.stream_ptr(cuda)))
    torch.cuda.synchronize()
    same_bits(rows, want.cpu().numpy(), "gauge rows against ddr_gauge_reduce")


# ---- mass balance and linearity ------------------------------------------------------------------------------

def test_mass_balance(cuda):
    """Zero start, forcing that ends in zeros long enough to drain: every sub-step conserves
    dt ((In + In+) / 2 + qe - (Q + Q+) / 2) = k (x (In+ - In) + (1 - x) (Q+ - Q)), so with empty storage at both
    ends the outlet's end-of-step states sum to the forcing's.  k in [1800, 7200] s at dt = 3600 s keeps
    |C3| <= 0.6: 200 zero rows leave nothing at depth 16."""
    net, _ = topo_of("S")
    rng = np.random.default_rng(5)
    k = rng.uniform(1800.0, 7200.0, net.n).astype(np.float32)
    x = rng.uniform(0.0, 0.3, net.n).astype(np.float32)
    g = RiverGraph(net.n, net.rows, net.cols, **TA.CUT)
    lm = LinearMuskingum(g, dev_t(k, cuda), dev_t(x, cuda), dt=3600.0, substeps=1)
    q = LC.random_forcing(net.n, 224, 9, np.float32, tail_zeros=200)
    out, q_last = lm(dev_t(q, cuda), output="end")
    outlet = int(np.flatnonzero(net.down < 0)[0])
    vol_out = float(out[outlet].double().sum()) * 3600.0
    vol_in = float(q.astype(np.float64).sum()) * 3600.0
    print(f"mass balance: in {vol_in:.6e} out {vol_out:.6e} rel {abs(vol_out - vol_in) / vol_in:.3e}")
    assert float(q_last.abs().max()) < 1e-6 * float(out.abs().max())
    assert abs(vol_out - vol_in) <= 1e-5 * vol_in


def test_linearity(cuda):
    """route(a q1 + q2) against a route(q1) + route(q2) in fp32.  The forcing's own rounding (a q1 + q2: 2 ulp) and
    ~10 roundings per reach and sub-step enter a recurrence whose memory is 1 / (1 - |C3|) sub-steps, along paths of
    up to 17 reaches; as a random walk that is a few tens of ulp of the largest discharge: 1e-5 of it is the bar."""
    net, _ = topo_of("S")
    _, lm = router("S", TA.CUT, "f32", cuda, 3)
    a = np.float32(1.37)
    q1 = LC.random_forcing(net.n, 12, 21, np.float32)
    q2 = LC.random_forcing(net.n, 12, 22, np.float32)
    r1, _ = lm(dev_t(q1, cuda))
    r2, _ = lm(dev_t(q2, cuda))
    r12, _ = lm(dev_t(a * q1 + q2, cuda))
    want = float(a) * r1.double() + r2.double()
    err = float((r12.double() - want).abs().max() / want.abs().max())
    print(f"linearity: {err:.3e}")
    assert err <= 1e-5


# ---- capture and errors --------------------------------------------------------------------------------------

def test_captured_route_replays_the_eager_result(cuda):
    net, _ = topo_of("S")
    _, lm = router("S", TA.CUT, "f32", cuda, 3)
    q = dev_t(LC.random_forcing(net.n, 17, 2, np.float32), cuda)
    eager, eager_last = lm(q)  # the graph's first launch outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, last = lm(q)
    for _ in range(2):
        out.zero_()
        last.zero_()
        graph.replay()
        torch.cuda.synchronize()
        same_bits(out, eager.cpu().numpy(), "captured out")
        same_bits(last, eager_last.cpu().numpy(), "captured q_last")
    same_bits(eager, model("S", 17, 3, "f32")["mean"], "eager")


def test_errors_on_the_device(cuda):
    net, _ = topo_of("S")
    g, lm = router("S", TA.WHOLE, "f32", cuda, 1)
    q = torch.ones(3, net.n, device=cuda)
    with pytest.raises(NotImplementedError):
        lm(q.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        lm(q, q0=torch.ones(net.n, device=cuda, requires_grad=True))
    with pytest.raises(RuntimeError):
        lm(q.cpu())
    with pytest.raises(RuntimeError):
        lm(q, flow_scale=torch.ones(net.n))
    with pytest.raises(ValueError):
        lm(q.double(), q0=torch.ones(net.n, device=cuda))
