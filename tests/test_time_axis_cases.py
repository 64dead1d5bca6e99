"""The time-axis cases of tests/test_gpu_time_axis.py, on the CPU (tests/time_axis_cases.py has the builders):
that the window lengths reach every phase and edge they are meant to, on the partitions they are used with,
and that the checker itself -- the oracle's forward and hand adjoint -- is right along the time axis where no
other test has used it: against central finite differences at T = 2, 3, 5 and 129 (parameters, q' and the
carried state), a window against the same window split in two at every step, and the one-step window (no
parameter gradient; dL/dq'[0] is the hot start's transposed solve).
"""

from __future__ import annotations

import numpy as np
import pytest

import time_axis_cases as C
from conftest import maxrel
from oracle import mc_oracle as O


# ---- coverage ---------------------------------------------------------------------------------------------

def test_partitions_have_the_stated_shape():
    for part, cut in (("whole", False), ("cut", True)):
        info = C.host_info("S", part)
        assert info.reaches_per_thread == 1 and (info.n_cut > 0) == cut, (part, info)
        assert 12 <= info.max_depth <= 18
    assert C.host_info("S", "whole").n_blocks == 1
    assert C.network("L").n == 3758
    for cap, kr in C.L_KR.items():
        info = C.host_info("L", cap)
        assert info.reaches_per_thread == kr, (cap, info)
        assert info.max_depth >= 100
        if cap != 4096:
            assert info.n_cut > 0, (cap, info)


def _coverage(ts, dmaxes, want_flushes):
    ts = sorted(ts)
    assert {t % 4 for t in ts} == {0, 1, 2, 3}
    for d in dmaxes:
        assert {(t + d) % C.CHUNK_BWD for t in ts} == set(range(C.CHUNK_BWD)), d
        assert {(t + d) % C.CHUNK_FWD for t in ts} == set(range(C.CHUNK_FWD)), d
        assert any(t <= d for t in ts), d
        rng = [C.steady_range(t, d) for t in ts]
        assert any(s1 <= s0 for s0, s1 in rng), d          # no steady tick
        assert any(s1 == s0 + 2 for s0, s1 in rng), d      # a single steady iteration
        assert any(s1 > s0 + 2 for s0, s1 in rng), d
        # both sides of the backward's first steady tick, dmax + 2
        assert {d + 1, d + 2, d + 3} <= set(ts), d
    assert {C.flushes(t) for t in ts} >= set(want_flushes)


@pytest.mark.parametrize("name,parts,sub", [("S", ("whole", "cut"), None), ("L", (256, 1536, 4096), None),
                                            ("L", (256,), "flush_depth")])
def test_window_lengths_cover_every_phase(name, parts, sub):
    """Every residue of T mod 4 and of T + dmax mod 8 (and mod 4, the forward's chunk), 0 to 3 flushes of the
    gradient partials, windows no longer than the block is deep, empty / single / longer steady ranges: for each
    partition's own dmax values.  The oracle comparison on L (cap 256) runs T_FLUSH and T_DEPTH only: one to
    three flushes."""
    for p in parts:
        info = C.host_info(name, p)
        if sub is None:
            ts, fl = C.t_sweep(name, parts), (0, 1, 2, 3)
        else:
            ts, fl = set(C.T_FLUSH) | set(C.t_depth(info)), (1, 2, 3)
        _coverage(ts, C.dmax_values(info), fl)
    assert set(C.T_SMALL) == set(range(1, 18))
    assert set(C.T_FLUSH) == set(range(125, 134)) | set(range(253, 260))


def test_both_roundings_of_the_steady_bound_occur():
    """s0 = dmax + 1 rounded up to even: dmax even (rounded) and odd (not) both occur, on S alone (the fp64
    comparison) and over L's partitions."""
    for name, parts in (("S", C.S_PARTS), ("L", C.L_PARTS)):
        par = {d & 1 for p in parts for d in C.dmax_values(C.host_info(name, p))}
        assert par == {0, 1}, (name, par)


def test_store_and_daily_windows_cover_their_edges():
    from ddr_amd.ops import DailyWindow

    for H, ts in C.STORE_T.items():
        assert all(C.qs_rows_layout(t, H) for t in ts)
        assert any(t % H != 0 and t > H for t in ts), H      # a partial last row behind whole ones
        assert any(t % H == 0 for t in ts) and 1 in ts, H
        assert any(-(-t // H) > 4 for t in ts) or H == 24    # more rows than a tile of the fp64 gather (4)
    ls = [DailyWindow.for_training(t).L for t in C.DAILY_T]
    assert ls == [t - 21 for t in C.DAILY_T]
    assert {24, 25, 47, 48, 49, 72} <= set(ls)
    assert {DailyWindow.for_training(t).D for t in C.DAILY_T} == {1, 2, 3}
    with pytest.raises(ValueError):
        DailyWindow.for_training(C.DAILY_REFUSED_T)


# ---- the oracle along the time axis -----------------------------------------------------------------------

def _loss(case, inp, r, qh=None):
    fw = O.route(case.network(), r, C.routed_qprime(case, inp, np.float64) if qh is None else qh, case.bounds,
                 q0=None if inp["q0"] is None else inp["q0"].astype(np.float64), dtype=np.float64,
                 outflow_idx=inp["gauges"])
    return fw["runoff"]


def _reaches(case, u=None):
    from test_clamp_cases import reaches_of

    return reaches_of(case, {k: v.astype(np.float64) for k, v in (u or case.u).items()}, np.float64)


@pytest.mark.parametrize("T", [2, 3, 5, 129])
@pytest.mark.parametrize("mode", ["state", "state_carry"])
def test_oracle_adjoint_matches_finite_differences(T, mode):
    """``route_backward`` against central differences of the fp64 forward (h = 1e-6, the tolerance of
    test_gpu_route.test_finite_difference_gradient_fp64): the three largest elements of each parameter's gradient, of
    dL/dq' (among them the hot start's row 0 when the window has one) and of dL/dQ0."""
    case, inp = C.window_case("S", T), C.mode_inputs("S", T, mode)
    ref = C.oracle_reference(case, inp, _reaches(case), np.float64)
    Wd = inp["W"].astype(np.float64)
    h = 1e-6

    def fd_of(perturb, h=h):
        vals = [perturb(s * h) for s in (+1, -1)]
        return float(np.sum((vals[0] - vals[1]) * Wd)) / (2 * h)

    def check(tag, g, fd):
        assert abs(fd - g) <= 1e-5 * max(1.0, abs(fd)), (tag, fd, g)

    for k, g in ref["grads"].items():
        for i in np.argsort(-np.abs(g))[:3]:
            def pert(e, k=k, i=i):
                u2 = {kk: vv.astype(np.float64).copy() for kk, vv in case.u.items()}
                u2[k][i] += e
                return _loss(case, inp, _reaches(case, u2))
            check((k, i), g[i], fd_of(pert))
    fs = inp["flow_scale"].astype(np.float64)
    gq = ref["qprime"]
    assert np.all(gq[-1] == 0.0) or T == 1  # q'[T-1] feeds no step
    flat = np.argsort(-np.abs(gq), axis=None)[:3]
    rows = list(zip(*np.unravel_index(flat, gq.shape)))
    if mode == "state":
        rows.append((0, int(np.argmax(np.abs(gq[0])))))
    for t, i in rows:
        def pert(e, t=t, i=i):
            qp = case.qprime.astype(np.float64).copy()
            qp[t, i] += e
            return _loss(case, inp, _reaches(case), qh=qp * fs[None, :])
        check(("qprime", t, i), gq[t, i], fd_of(pert))
    if mode == "state_carry":
        for i in list(np.argsort(-np.abs(ref["q0"]))[:3]) + [11]:  # 11: carried below q_lb
            def pert(e, i=i):
                inp2 = dict(inp, q0=inp["q0"].astype(np.float64).copy())
                inp2["q0"][i] += e
                return _loss(case, inp2, _reaches(case))
            # (a step of at most 1e-3 of the state: the physics is strongly curved at the 5e-5 of reach 11)
            check(("q0", i), ref["q0"][i], fd_of(pert, min(h, 1e-3 * float(inp["q0"][i]))))
        assert ref["q0"][11] != 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_oracle_window_equals_its_two_halves(dtype):
    """``route`` over T steps equals ``route`` over T1 steps followed by a run of T - T1 + 1 steps that carries
    the first one's final state (its column 0 is that state), bit for bit, at every split point."""
    T = 21
    case = C.window_case("S", T)
    net, r, bd = case.network(), case.reaches().astype(dtype), case.bounds
    full = O.route(net, r, case.qprime, bd, dtype=dtype)
    for T1 in range(1, T + 1):
        a = O.route(net, r, case.qprime[:T1], bd, dtype=dtype)
        b = O.route(net, r, case.qprime[T1 - 1:], bd, q0=a["q_last"], dtype=dtype)
        np.testing.assert_array_equal(a["runoff"], full["runoff"][:, :T1])
        np.testing.assert_array_equal(b["runoff"], full["runoff"][:, T1 - 1:])
        np.testing.assert_array_equal(b["q_last"], full["q_last"])


def test_oracle_one_step_window():
    """T = 1 is the hot start alone: no parameter gradient at all, dL/dq'[0] = (I - N)^-T (W masked by the
    hot start's clamp), here against a dense solve."""
    case, inp = C.window_case("S", 1), C.mode_inputs("S", 1, "state")
    ref = C.oracle_reference(case, inp, _reaches(case), np.float64)
    for k, g in ref["grads"].items():
        assert np.all(g == 0.0), k
    n = case.n
    A = np.eye(n)
    A[case.rows, case.cols] -= 1.0
    x0 = ref["fw"]["x"][0]
    assert maxrel(np.linalg.solve(A, C.routed_qprime(case, inp, np.float64)[0]), x0) <= 1e-12
    g = inp["W"][:, 0].astype(np.float64) * (x0 >= case.bounds.discharge)
    want = np.linalg.solve(A.T, g) * inp["flow_scale"].astype(np.float64)
    assert ref["qprime"].shape == (1, n)
    assert maxrel(ref["qprime"][0], want) <= 1e-12
    # with the state seeds: the seed of Q_0 joins W, the geometry reports nothing
    inp = C.mode_inputs("S", 1, "seed")
    ref = C.oracle_reference(case, inp, _reaches(case), np.float64)
    assert all(np.all(g == 0.0) for g in ref["grads"].values())


def test_steady_windows_have_no_parameter_gradient():
    """``steady_window``: a hot-started window over one q' row stays in the hot start's steady state, so the
    oracle's parameter gradients are the rounding residue of cancelled terms (<= 1e-14 of ``gradient_scale``;
    measured 1.2e-16) -- or, with a q' below q_lb in that row (the stores), what those terms leave, <= 1e-4 of it.
    One step further the gradient is a well-conditioned one, above 1e-4 of the scale."""
    def top(ref):
        return max(float(np.abs(v).max()) for v in ref["grads"].values()) / ref["scale"]

    for mode in ("reach", "gauge", "state"):
        for T, steady in ((2, True), (3, False)):
            case, inp = C.window_case("S", T), C.mode_inputs("S", T, mode)
            ref = C.oracle_reference(case, inp, _reaches(case), np.float64)
            assert ref["steady"] == steady, (mode, T)
            assert (top(ref) <= 1e-14) if steady else (top(ref) >= 1e-4), (mode, T, top(ref))
    for mode in ("carry", "state_carry", "seed"):  # a carried state, the reported geometry: a gradient at T = 2
        case, inp = C.window_case("S", 2), C.mode_inputs("S", 2, mode)
        ref = C.oracle_reference(case, inp, _reaches(case), np.float64)
        assert not ref["steady"] and top(ref) >= 1e-4, (mode, top(ref))
    for H, T in C.STORE_CASES:
        if T == 1:
            continue
        case, inp = C.store_case("S", T, H)
        ref = C.oracle_reference(case, inp, _reaches(case), np.float64, qh=C.store_hourly(inp, T, np.float64))
        assert ref["steady"] == (T <= H + 1), (H, T)
        assert (top(ref) <= 1e-4) if ref["steady"] else (top(ref) >= 1e-4), (H, T, top(ref))


def test_store_and_daily_references_are_adjoint_pairs():
    """The pooling's adjoint and the store's row sum are the transposes of their forwards (dot-product test)."""
    from ddr_amd.ops import DailyWindow

    rng = np.random.default_rng(3)
    for T in C.DAILY_T:
        win = DailyWindow.for_training(T)
        x, gd = rng.uniform(0, 1, (5, T)), rng.uniform(0, 1, (5, win.D))
        lhs = float(np.sum(C.daily_pool(x, win) * gd))
        assert abs(lhs - float(np.sum(x * C.daily_pool_vjp(gd, win, T)))) <= 1e-12 * abs(lhs)
    for H, T in ((24, 50), (3, 18), (7, 1)):
        case, inp = C.store_case("S", T, H)
        g = rng.uniform(0, 1, (T, case.n))
        d = rng.uniform(0, 1, inp["store"].shape)
        moved = np.repeat((inp["store"] + d).astype(np.float64), H, axis=0)[:T] * inp["flow_scale"].astype(np.float64)
        base = np.repeat(inp["store"].astype(np.float64), H, axis=0)[:T] * inp["flow_scale"].astype(np.float64)
        delta = moved - base
        delta[:, inp["valid"] == 0] = 0.0
        lhs = float(np.sum(delta * g))
        assert abs(lhs - float(np.sum(C.store_grad(inp, g) * d))) <= 1e-9 * abs(lhs)
        assert np.all(C.store_grad(inp, g)[:, C.store_marks("S")[0]] == 0.0)
