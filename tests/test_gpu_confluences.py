"""The routing kernels and both graph builders on reaches with more than two inflows.

Every other network of the suite has in-degree <= 2, so none reaches the kernels' confluence list (csrc/route_device.h
``pack_up`` / ``up_1``, the ``j = 2..c`` tails of the forward tick, the backward recompute and its prologue,
``load_xlist``) or its emission (csrc/graph.cpp, csrc/devgraph.hip ``xoff`` / ``xlist``).  The networks are those of
tests/confluence_cases.py; tests/test_confluence_cases.py asserts on the CPU that each (network, partition) used
here holds the classes of confluence its row in ``confluence_cases.PAIRS`` names (every inflow local, mixed, every
inflow cut, a cut inflow at list position 0 / 1 / >= 2, two lists in one block, in-degrees 3, 14, 15, 16, >= 17).

Bars (tests/test_gpu_route.py header, BASELINE north star; none is new):
  * fp32 kernel vs the reference's fp32 (tests/golden/confluence.npz): discharge and geometry max-rel <= 1e-4,
    gradients norm-rel <= 5e-5;
  * fp32 kernel vs the fp32 oracle on the kernel's own inputs: max-rel <= 1e-6;
  * fp64 kernel vs the fp64 oracle: runoff <= 1e-12, gradients norm-rel <= 1e-10 and element max-rel <= 1e-6;
  * state gradients and the exact adjoint at the bars of test_gpu_state.py and test_gpu_exact_adjoint.py;
  * bitwise: partition invariance, KR 4 == KR 1 / 2, steady == general path, run-to-run.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import confluence_cases as cc
from conftest import maxrel, normrel, synthetic_case
from ddr_amd import _lib
from ddr_amd.graph import RiverGraph
from ddr_amd.ops import GaugeMap, RouteConsts, route
from oracle import mc_oracle as O
from test_gpu_devgraph import _both, _same
from test_gpu_exact_adjoint import BAR, _check, _kernel, _reaches
from test_gpu_route import run_hip
from test_gpu_state import _dropin, physical, reaches_of
from test_gpu_steady import _run

pytestmark = pytest.mark.gpu

T = cc.T
GRADS = ("grad_n", "grad_q_spatial", "grad_p_spatial")
SEEDS = {"golden300": 3, "bushy600": 6, "bushy1500": 15, "bushy2600": 26, "hub": 20, "mix40": 40}


@functools.lru_cache(maxsize=None)
def case_of(name, steps=T):
    """The synthetic case of a network (attributes, unit parameters, q', W), shared read-only."""
    return synthetic_case(cc.network(name), steps, SEEDS[name])


def graph_of(name, part, **extra):
    net, gkw = cc.pair(name, part)
    return RiverGraph(net.n, net.rows, net.cols, **gkw, **extra)


def unit_grads(case, bw, dtype=np.float64):
    u = {k: v.astype(dtype) for k, v in case.u.items()}
    return O.param_grads_from_unit(bw["n"], bw["q_spatial"], bw["p_spatial"], u["n"], u["q_spatial"], u["p_spatial"],
                                   case.params["parameter_ranges"])


# ---- the reference's golden vectors ---------------------------------------------------------------------------


@pytest.mark.parametrize("part", ["whole", "cut64"])
def test_fp32_matches_reference_golden(cuda, part):
    leg1, leg2, gcase, d = cc.golden_confluence()
    _, gkw = cc.pair("golden300", part)
    res = run_hip(leg1, cuda, gkw=gkw)
    for k in ("runoff", "q_last", "top_width", "side_slope"):
        assert maxrel(res[k], d[f"ref_{k}"]) <= 1e-4, k
    for k in GRADS:
        assert normrel(res[k], d[f"ref_{k}"]) <= 5e-5, k
    # the second leg carries the first one's final state (q0 = ref_q_last), new q' and W
    res2 = run_hip(leg2, cuda, gkw=gkw, q0=d["ref_q_last"])
    for k in ("runoff", "q_last", "top_width", "side_slope"):
        assert maxrel(res2[k], d[f"ref2_{k}"]) <= 1e-4, k
    for k in GRADS:
        assert normrel(res2[k], d[f"ref2_{k}"]) <= 5e-5, k
    # gauge mode: the outlet (a 20-way confluence), three confluences summed, a headwater, a mixed pair
    gz = GaugeMap.build(d["outflow"], gcase.n, cuda)
    resg = run_hip(gcase, cuda, gkw=gkw, gauges=gz)
    assert resg["runoff"].shape == d["refg_runoff"].shape == (len(d["outflow"]), T)
    for k in ("runoff", "q_last", "top_width", "side_slope"):
        assert maxrel(resg[k], d[f"refg_{k}"]) <= 1e-4, k
    for k in GRADS:
        assert normrel(resg[k], d[f"refg_{k}"]) <= 5e-5, k


# ---- against the oracle ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,part", [("bushy600", "whole"), ("bushy1500", "whole"), ("bushy2600", "whole"),
                                       ("bushy2600", "cut64"), ("hub", "cut64"), ("mix40", "whole")])
def test_fp32_matches_fp32_oracle(cuda, name, part):
    case = case_of(name)
    g = graph_of(name, part)
    res = run_hip(case, cuda, graph=g, grads=False)
    ref = O.route(case.network(), res["reaches"], case.qprime, case.bounds, dtype=np.float32)
    assert maxrel(res["runoff"], ref["runoff"]) <= 1e-6
    assert maxrel(res["q_last"], ref["q_last"]) <= 1e-6


@pytest.mark.parametrize("name", ["bushy600", "hub"])
@pytest.mark.parametrize("part", ["whole", "cut64"])
def test_fp64_matches_fp64_oracle(cuda, name, part):
    case = case_of(name)
    res = run_hip(case, cuda, dtype=torch.float64, graph=graph_of(name, part))
    net, r, bd = case.network(), res["reaches"], case.bounds
    ref = O.route(net, r, case.qprime, bd, dtype=np.float64)
    assert maxrel(res["runoff"], ref["runoff"]) <= 1e-12
    bw = O.route_backward(net, r, case.qprime, ref["x"], case.W, bd)
    for k, v in unit_grads(case, bw).items():
        assert normrel(res[f"grad_{k}"], v) <= 1e-10, k
        assert maxrel(res[f"grad_{k}"], v, floor=1e-30 * float(np.abs(v).max())) <= 1e-6, k


@pytest.mark.parametrize("part", ["whole", "cut64"])
@pytest.mark.parametrize("mode", ["hot", "carry"])
def test_fp64_state_gradients_match_fp64_oracle(cuda, part, mode):
    """dL/dq' (with the hot start's transposed solve through the confluences) and dL/dQ0 of a carried state,
    at test_gpu_state.py's fp64 bar."""
    case = case_of("bushy600")
    u, n, q, p, slope, tt = physical(case, cuda, torch.float64)
    rng = np.random.default_rng(61)
    qs = case.qprime.astype(np.float64)
    qs[:2, 5] = 1e-6  # below the clamp
    q0 = rng.uniform(0.5, 5.0, case.n) if mode == "carry" else None
    if q0 is not None:
        q0[cc.network("bushy600").rows[:3]] = 5e-5  # carried states below q_lb on reaches that have inflows
    qp = tt(qs).requires_grad_(True)
    q0t = tt(q0).requires_grad_(True) if q0 is not None else None
    cs = RouteConsts(discharge_lb=1e-4, velocity_lb=0.01, depth_lb=0.01, bottom_width_lb=0.01)
    runoff, _, _, _ = route(graph_of("bushy600", part), qp, n, q, p, tt(case.length), slope, tt(case.x), q0=q0t,
                            consts=cs)
    W = rng.uniform(0, 1, tuple(runoff.shape))
    runoff.backward(tt(W))
    r = reaches_of(n, q, p, slope, case, np.float64)
    net, bd = case.network(), case.bounds
    ref = O.route(net, r, qs, bd, q0=q0, dtype=np.float64)
    assert maxrel(runoff.detach().cpu().numpy(), ref["runoff"]) <= 1e-12
    bw = O.route_backward(net, r, qs, ref["x"], W, bd, want_qprime=True, carry=q0 is not None)
    assert normrel(qp.grad.cpu().numpy(), bw["qprime"]) <= 1e-10
    if q0 is not None:
        assert normrel(q0t.grad.cpu().numpy(), bw["q0"]) <= 1e-10
    for k, v in unit_grads(case, bw).items():
        assert normrel(u[k].grad.cpu().numpy(), v) <= 1e-10, k


@pytest.mark.parametrize("mode", ["hot", "carry"])
def test_exact_adjoint_on_confluences(cuda, mode):
    """``exact_adjoint=True`` with state gradients, against the fp64 oracle adjoint on the kernel's fp32 states
    (test_gpu_exact_adjoint.py's bars), one block against cap 64."""
    name = "bushy2600"
    net = cc.network(name)
    case = case_of(name)
    r = _reaches(case.u, case)
    q0 = np.random.default_rng(22).uniform(0.5, 5.0, net.n).astype(np.float32) if mode == "carry" else None
    netO = case.network()
    fw = O.route(netO, r, case.qprime, O.Bounds(), q0=q0, dtype=np.float32)
    bw = O.route_backward(netO, r, case.qprime, fw["x"], case.W, O.Bounds(), want_qprime=True, carry=q0 is not None)
    ex = _kernel(cuda, net.n, net.rows, net.cols, r, case.qprime, case.W, exact=True, q0=q0, gkw=cc.WHOLE)
    np.testing.assert_array_equal(ex["runoff"], fw["runoff"])  # the oracle's states are the kernel's
    keys = ("n", "q_spatial", "p_spatial", "qprime") + (("q0",) if q0 is not None else ())
    _check(ex, bw, keys, BAR)
    cut = _kernel(cuda, net.n, net.rows, net.cols, r, case.qprime, case.W, exact=True, q0=q0, gkw=cc.CUT64)
    for k in keys + ("runoff",):
        np.testing.assert_array_equal(cut[k], ex[k], err_msg=k)


def test_hotstart_alone_matches_oracle(cuda):
    """The hot start on its own, (I - N) Q = q'[0] through the confluences: the C ABI's ddr_hotstart_f32 on
    whole and cut graphs, and the drop-in compute_hotstart_discharge (fp64 sums: bit-exact, test_gpu_dropin.py)."""
    from ddr_amd.routing import compute_hotstart_discharge

    lib = _lib.load()
    for name, part in (("bushy2600", "whole"), ("bushy2600", "cut64"), ("hub", "cut64"), ("mix40", "whole")):
        case = case_of(name)
        q = case.qprime[0].copy()
        q[::7] = 1e-6  # some below q_lb: the solve is unclamped, the result clamped
        ref = O.hotstart(case.network(), q, O.Bounds(), np.float32)
        g = graph_of(name, part)
        qt = torch.from_numpy(q).to(cuda)
        out = torch.empty(case.n, device=cuda)
        _lib.check(lib.ddr_hotstart_f32(g.handle, qt.data_ptr(), C.c_double(1e-4), out.data_ptr(), _lib.stream_ptr(cuda)))
        np.testing.assert_array_equal(out.cpu().numpy(), ref, err_msg=f"{name} {part}")
    case = case_of("mix40")
    mc, dc = _dropin(case, None, cuda)
    mc.setup_inputs(dc, torch.from_numpy(case.qprime).to(cuda), {k: torch.from_numpy(v).to(cuda) for k, v in case.u.items()})
    mapper, _, _ = mc.create_pattern_mapper()
    q = case.qprime[0]
    res = compute_hotstart_discharge(torch.from_numpy(q).to(cuda), mapper, mc.discharge_lb, cuda)
    np.testing.assert_array_equal(res.cpu().numpy(), O.hotstart(case.network(), q, O.Bounds(), np.float32))
    np.testing.assert_array_equal(mc._discharge_t.cpu().numpy(), res.cpu().numpy())


# ---- bitwise properties ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("math", ["exact", "faithful", "fast"])
def test_partition_invariance_and_determinism(cuda, math):
    """One block == cap 64 == cap 160 == cap 160 in generations of four workgroups, and run to run: a list entry
    that is a cut edge's virtual slot holds the bits the local slot would."""
    case = case_of("bushy600")
    keys = ("runoff", "q_last") + GRADS
    base = run_hip(case, cuda, graph=graph_of("bushy600", "whole"), math=math)
    again = run_hip(case, cuda, graph=graph_of("bushy600", "whole"), math=math)
    for k in keys:
        np.testing.assert_array_equal(again[k], base[k], err_msg=k)
    for part in ("cut64", "cut160", "gen4"):
        alt = run_hip(case, cuda, graph=graph_of("bushy600", part), math=math)
        assert alt["graph"].info.n_cut > 0
        for k in keys:
            np.testing.assert_array_equal(alt[k], base[k], err_msg=f"{part} {k}")
    hub = case_of("hub")
    a = run_hip(hub, cuda, graph=graph_of("hub", "whole"), math=math)
    b = run_hip(hub, cuda, graph=graph_of("hub", "cut64"), math=math)  # every inflow of the hub is cut
    for k in keys:
        np.testing.assert_array_equal(b[k], a[k], err_msg=f"hub {k}")


def test_faithful_kr4_block_equals_kr1_and_kr2_blocks(cuda):
    case = case_of("bushy2600")
    big = run_hip(case, cuda, graph=graph_of("bushy2600", "whole"), math="faithful")
    assert big["graph"].info.reaches_per_thread == 4
    for part, kr in (("cap500", 1), ("cap1500", 2)):
        alt = run_hip(case, cuda, graph=graph_of("bushy2600", part), math="faithful")
        assert alt["graph"].info.reaches_per_thread == kr and alt["graph"].info.n_cut > 0
        for k in ("runoff", "q_last") + GRADS:
            np.testing.assert_array_equal(alt[k], big[k], err_msg=f"{part} {k}")


@pytest.mark.parametrize("math", ["exact", "faithful", "fast"])
@pytest.mark.parametrize("part", ["whole", "cut64"])
@pytest.mark.parametrize("carry", [False, True], ids=["hot", "carry"])
def test_steady_path_is_bitwise_the_general_path(cuda, math, part, carry):
    case = case_of("bushy600")
    g = graph_of("bushy600", part)
    assert g.info.max_depth + 2 < T  # steady ticks exist
    q0 = np.random.default_rng(8).uniform(0.1, 5.0, case.n).astype(np.float32) if carry else None
    a = _run(case, cuda, g, math, q0=q0)
    b = _run(case, cuda, g, math, q0=q0, no_steady=True)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---- closed forms and finite differences ----------------------------------------------------------------------


@pytest.mark.parametrize("k", cc.STAR_KS)
def test_star_outlet_against_closed_form(cuda, k):
    """An outlet with k leaf inflows, fp64, against numpy written out here (no CSR code): the hot start is
    q' + sum of the inflows' hot starts; the first step is the one-reach formula with I = sum max(x_j, q_lb) and the
    solve's c1 * sum x_j(1).  The kernel takes k from the list's first entry (the packed word caps at 15)."""
    net = cc.star(k)
    case = synthetic_case(net, 4, 100 + k)
    case.qprime[0, 1] = 1e-6  # one inflow's hot start below q_lb: I sums the clamped values, the solve the raw ones
    res = run_hip(case, cuda, dtype=torch.float64, grads=False)
    assert res["graph"].info.n_blocks == 1
    r, bd, lb = res["reaches"], case.bounds, 1e-4
    qp = case.qprime.astype(np.float64)
    x0 = qp[0].copy()
    for j in range(k):
        x0[k] = x0[k] + x0[j]
    Q0 = np.maximum(x0, lb)
    c, _, _ = O.trapezoid_celerity(Q0, r.n, r.q, r.p, r.slope, bd, np.float64)
    c1, c2, c3, c4 = O.muskingum_coefficients(r.length, c, r.x, 3600.0, np.float64)
    qc = np.maximum(qp[0], lb)
    inflow = np.zeros(k + 1)
    for j in range(k):
        inflow[k] = inflow[k] + Q0[j]
    x1 = ((c2 * inflow) + (c3 * Q0)) + (c4 * qc)
    for j in range(k):
        x1[k] = x1[k] + c1[k] * x1[j]
    assert Q0[1] == lb and x0[1] < lb
    assert maxrel(res["runoff"][:, 0], Q0) <= 1e-12
    assert maxrel(res["runoff"][:, 1], np.maximum(x1, lb)) <= 1e-12
    # the fp32 hot start alone (fp64 sums in the same order: bit-exact)
    g = res["graph"]
    qt = torch.from_numpy(case.qprime[0].copy()).to(cuda)
    out = torch.empty(k + 1, device=cuda)
    _lib.check(_lib.load().ddr_hotstart_f32(g.handle, qt.data_ptr(), C.c_double(lb), out.data_ptr(), _lib.stream_ptr(cuda)))
    np.testing.assert_array_equal(out.cpu().numpy(), np.maximum(x0.astype(np.float32), np.float32(lb)))


def test_finite_difference_gradient_fp64_on_the_mix(cuda):
    """test_gpu_route.py test_finite_difference_gradient_fp64's method and step on the 40-reach mix, at a leaf of
    the 20-star, the 20-way hub, the 9-way hub, a chain reach and the 5-way outlet."""
    net = cc.mix40()
    steps, seed, h = 30, SEEDS["mix40"], 1e-6
    case = synthetic_case(net, steps, seed)
    res = run_hip(case, cuda, dtype=torch.float64)
    for k in ("n", "q_spatial", "p_spatial"):
        for i in (cc.MIX40_LEAF20, cc.MIX40_HUB20, cc.MIX40_HUB9, 12, cc.MIX40_OUTLET):
            vals = []
            for s in (+1, -1):
                c2 = synthetic_case(net, steps, seed)
                c2.u = {kk: vv.astype(np.float64).copy() for kk, vv in case.u.items()}
                c2.u[k][i] += s * h
                r = run_hip(c2, cuda, dtype=torch.float64, grads=False)
                vals.append(float(np.sum(r["runoff"] * case.W.astype(np.float64))))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - res[f"grad_{k}"][i]) <= 1e-5 * max(1.0, abs(fd)), (k, i, fd, res[f"grad_{k}"][i])


# ---- the device builder ---------------------------------------------------------------------------------------

KWS = [{}, {"max_block_reaches": 128, "target_blocks": 8}, {"max_block_reaches": 400, "target_blocks": 1 << 20}]


@pytest.mark.parametrize("kw", KWS, ids=["default", "cap128x8", "cap400"])
@pytest.mark.parametrize("name", ["bushy2600", "hub", "mix40", "confetti"] + [f"star{k}" for k in cc.STAR_KS])
def test_device_build_equals_host_build(cuda, name, kw):
    h, d = _both(cc.network(name), **kw)
    _same(h, d)


def test_device_build_equals_host_build_on_cut_pairs(cuda):
    """The partitions the routing tests above use (mixed and all-cut confluences, generations)."""
    for name, part, gkw, _, _ in cc.PAIRS:
        if part != "whole":
            h, d = _both(cc.network(name), **gkw)
            _same(h, d)


def test_device_build_star_envelope(cuda):
    """The widest stars (tests/test_confluence_cases.py test_star_envelope): what the host builds the device
    builds identically, and past it both raise DDR_ERR_CAPACITY."""
    for k in (500, cc.LARGEST_STAR):
        h, d = _both(cc.star(k))
        _same(h, d)
    for k in (cc.LARGEST_STAR + 1, 2048, 9000):
        net = cc.star(k)
        with pytest.raises(_lib.DDRError) as eh:
            RiverGraph(net.n, net.rows, net.cols, host_only=True)
        with pytest.raises(_lib.DDRError) as ed:
            RiverGraph(net.n, net.rows, net.cols, on_device=True)
        assert eh.value.code == ed.value.code == _lib.DDR_ERR_CAPACITY, (k, str(ed.value))


def test_gauge_batch_routes_through_device_built_graph(cuda):
    """GaugeMap + a device-built cut graph on the golden confluence network: gauge-mode runoff equals the oracle's."""
    _, _, gcase, d = cc.golden_confluence()
    net = cc.network("golden300")
    g = RiverGraph(net.n, torch.from_numpy(net.rows).to(cuda), torch.from_numpy(net.cols).to(cuda), **cc.CUT64)
    assert g.device_built and g.info.n_cut > 0
    gz = GaugeMap.build(d["outflow"], net.n, cuda)
    res = run_hip(gcase, cuda, graph=g, gauges=gz, grads=False)
    ref = O.route(gcase.network(), res["reaches"], gcase.qprime, gcase.bounds, dtype=np.float32, outflow_idx=d["outflow"])
    assert maxrel(res["runoff"], ref["runoff"]) <= 1e-6
    assert maxrel(res["runoff"], d["refg_runoff"]) <= 1e-4
