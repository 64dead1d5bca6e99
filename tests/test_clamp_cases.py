"""The stress cases of tests/test_gpu_clamps.py, on the CPU: the builder of the three regimes (``stress_case``),
the census of the physics' clamps along a trajectory (``census``) and the preconditions every comparison of
those cases rests on (``assert_preconditions``), plus the check that the checker itself -- the fp64 oracle's
hand adjoint, ``mc_oracle.route_backward`` -- is right where the clamps and their gradient masks are active,
where no other test has used it: against central finite differences of the fp64 oracle's forward.

The physics has seven clamps (ddr_amd/csrc/physics.h, oracle ``trapezoid_celerity`` / ``route``): depth >= d_lb,
0.5 <= side slope <= 50, bottom width >= bw_lb, v_lb <= velocity <= 15, routed state >= q_lb, q' >= q_lb.
The inputs of every other test leave the depth, velocity and mid-run state clamps inactive; the regimes here
are built to hit them:

  low    q' scaled by 10^U(-6, -2) per reach: dry reaches at the depth and lower velocity bounds, headwaters
         whose state sits at q_lb or below it
  high   q' scaled by 10^U(2, 4.5), slope by 10^U(0.5, 2), u["n"] by 0.1: floods at the upper velocity bound
  flash  three windows of three consecutive zero hours of q' per reach, at random times: q' < q_lb on every
         reach, and reaches with c3 < 0 solve to x < q_lb, most of them to x < 0, in the middle of the run (one
         window gives 3-15 such reach-steps on 200 reaches, fewer than the 20 the case must have)

A dry headwater's steady state is x = (c3 + c4) q_lb = q_lb, up to the last bit: whether such a state counts as
below q_lb depends on the precision and on the platform's rounding (506 reach-steps of low / default in fp32,
151 in fp64), and its parameter gradient is zero either way.  The state-clamp count asked of flash therefore
takes only states below q_lb (1 - 1e-6) ("clear" below).

The 200-reach cases (random_binary_tree(200, seed), T = 48; the gradients are compared on these) take, per regime
and parameter set, the first seed from 4 upward that meets the preconditions on the fp32 and the fp64 trajectory.
Shares of the 200 x 47 reach-steps at which each clamp is active on the fp32 trajectory; ``x<q_lb`` also as the
number of reach-steps at t >= 2 and of the clear ones among them (fp64: the same clear ones); ``near``:
reach-steps with a recomputed clamped quantity (pw, ss_raw, bw_raw, v) within relative 1e-4 / 1e-3 of a bound;
``hit``: share of the reaches with a targeted clamp (TARGETS) active at some step, among all reaches / among
those whose gradient element is above 1e-3 of the largest (the smallest of n, q, p); ``zero``: reaches whose
velocity is clamped at every step, whose gradient is exactly zero:

  case           seed  depth  v low  v high  x<q_lb (t>=2, clear)  q'<q_lb  ss low/high  bw     near   hit          zero
  low / default     4  0.295  0.124  0       0.055 (506, 0)        0.583    0.010/0.356  0.035  0 / 1  0.38 / 0.15   24
  low / mock        6  0.179  0.728  0       0.010 (92, 0)         0.857    0.010/0.328  0.077  0 / 9  0.83 / 0.46  141
  high / default    4  0      0      0.417   0                     0        0.325/0.015  0.214  0 / 9  0.47 / 0.19   69
  high / mock       4  0      0      0.613   0                     0        0.282/0.015  0.202  0 / 5  0.62 / 0.12  117
  flash / default  14  0.006  0      0       0.005 (47, 29)        0.179    0.164/0.093  0.059  0 / 0  1.00 / 1.00    0
  flash / mock      4  0.005  0.048  0       0.005 (44, 39)        0.179    0.137/0.157  0.043  0 / 7  1.00 / 1.00    4

Between 23 % (low / mock) and 100 % (flash) of the reaches carry a gradient element above 1e-3 of the largest.
A reach whose velocity is clamped at a step gets no parameter gradient from that step, so the clamped reaches
are the small elements of a gradient: among the elements above 1e-3 of the largest fewer than 25 % belong to
clamped reaches in low / default and in high, on every seed from 4 to 79.  Precondition 2 is therefore asserted
over all reaches (each enters a norm), and the GPU comparisons add the same measures over the targeted reaches
alone, at their own scale.  On the larger graphs of the forward tests (a 3000-reach Hack basin, a 30 000-reach
forest at T = 24) the shares of depth and velocity are within 0.07 of these, and flash has 120-3200 mid-run
states below zero there.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

from conftest import PARAMS_DEFAULT, PARAMS_MOCK, synthetic_case
from ddr_amd import synthetic
from oracle import mc_oracle as O

REGIMES = ("low", "high", "flash")
PARAMS = {"default": PARAMS_DEFAULT, "mock": PARAMS_MOCK}
CASES = [(reg, pn) for reg in REGIMES for pn in PARAMS]
FLASH_HOURS, FLASH_EVENTS = 3, 3
# the clamps each regime is named for (keys of census()["active"])
TARGETS = {"low": ("depth", "v_low"), "high": ("v_high",), "flash": ("x_low", "qp_low")}
TREE, T_TREE = 200, 48
SEEDS = {("low", "default"): 4, ("low", "mock"): 6, ("high", "default"): 4, ("high", "mock"): 4,
         ("flash", "default"): 14, ("flash", "mock"): 4}
NEAR_GRAD, NEAR_FD = 1e-4, 1e-3


def stress_case(net, T, seed, params, regime):
    """A ``synthetic_case`` edited in place into one of the three regimes (module docstring)."""
    case = synthetic_case(net, T, seed, params)
    rng = np.random.default_rng(seed + 9000)
    f = np.float32
    if regime == "low":
        case.qprime = (case.qprime * (10.0 ** rng.uniform(-6, -2, net.n)).astype(f)[None, :]).astype(f)
    elif regime == "high":
        case.qprime = (case.qprime * (10.0 ** rng.uniform(2, 4.5, net.n)).astype(f)[None, :]).astype(f)
        case.slope = (case.slope * (10.0 ** rng.uniform(0.5, 2, net.n)).astype(f)).astype(f)
        case.u["n"] = (case.u["n"] * f(0.1)).astype(f)
    elif regime == "flash":
        for _ in range(FLASH_EVENTS):
            start = rng.integers(1, T - FLASH_HOURS, net.n)
            hours = start[None, :] + np.arange(FLASH_HOURS)[:, None]
            case.qprime[hours, np.arange(net.n)[None, :]] = 0.0
    else:
        raise ValueError(regime)
    return case


def tree_stress_case(regime, pname):
    seed = SEEDS[regime, pname]
    return stress_case(synthetic.random_binary_tree(TREE, seed), T_TREE, seed, PARAMS[pname], regime)


def reaches_of(case, u=None, dtype=np.float32):
    """The physical inputs (``Case.reaches`` in ``dtype``, optionally from other unit parameters)."""
    u = case.u if u is None else u
    rng, ls = case.params["parameter_ranges"], case.params["log_space_parameters"]
    den = lambda k: O.denormalize(u[k], rng[k], k in ls, dtype=dtype)  # noqa: E731
    slope = np.maximum(case.slope, np.float32(case.params["attribute_minimums"]["slope"])).astype(dtype)
    return O.Reaches(den("n"), den("q_spatial"), den("p_spatial"), case.length.astype(dtype), slope,
                     case.x.astype(dtype))


def census(case, r, x, dtype=np.float32):
    """Where each clamp is active along the trajectory ``x`` ((T, N), the unclamped solves of ``O.route``) and
    how close the recomputed clamped quantities come to their bounds.  Row k of every array is step k + 1: its
    physics reads the clamped state of step k, its solve gives x[k + 1], its lateral inflow is q'[k].

    Returns dict(active: name -> (T-1, N) bool; near: a function of the relative distance giving the (T-1, N)
    bool that some recomputed quantity (pw, ss_raw, bw_raw, v) is within it of one of its bounds; x; qlb)."""
    f = dtype
    bd = case.bounds
    r = r.astype(f)
    x = np.asarray(x, f)
    N = x.shape[1]
    qlb = f(bd.discharge)
    d = O.trapezoid_celerity(np.maximum(x, qlb)[:-1], r.n, r.q, np.broadcast_to(r.p, (N,)), r.slope, bd, f,
                             full=True)
    pairs = [(d["pw"], f(bd.depth)), (d["ss_raw"], f(bd.side_slope_min)), (d["ss_raw"], f(bd.side_slope_max)),
             (d["bw_raw"], f(bd.bottom_width)), (d["v"], f(bd.velocity)), (d["v"], f(bd.velocity_max))]
    active = {"depth": d["pw"] < f(bd.depth), "v_low": d["v"] < f(bd.velocity), "v_high": d["v"] > f(bd.velocity_max),
              "ss_low": d["ss_raw"] < f(bd.side_slope_min), "ss_high": d["ss_raw"] > f(bd.side_slope_max),
              "bw": d["bw_raw"] < f(bd.bottom_width), "x_low": x[1:] < qlb,
              # below q_lb by more than rounding: a dry headwater's steady state is q_lb to the last bit or two,
              # on either side of it by the precision and the platform
              "x_clear": x[1:].astype(np.float64) < float(qlb) * (1.0 - 1e-6),
              "qp_low": np.asarray(case.qprime, f)[:-1] < qlb}

    def near(tol):
        m = np.zeros(d["pw"].shape, bool)
        for v, b in pairs:
            m |= np.abs(v.astype(np.float64) - float(b)) <= tol * float(b)
        return m

    return {"active": active, "near": near, "x": x, "qlb": qlb}


def targeted(cen, regime):
    """(N,) bool: the reach had one of the regime's clamps active at some step."""
    return np.any([cen["active"][k].any(axis=0) for k in TARGETS[regime]], axis=0)


def assert_preconditions(cen, regime, grads=None, fp32_grads=False):
    """The preconditions of a stress case: plain asserts on oracle output.

    1. every clamp the regime is named for is active on at least 1 % of the reach-steps; the mid-run state clamp
       of flash on at least 20 reach-steps at t >= 2, counting only states clearly below q_lb;
    2. (``grads``: name -> (N,) reference gradient, where gradients are compared) at least 25 % of the reaches
       had such a clamp active at some step, and the gradients are finite;
    3. (``fp32_grads``: a gradient comparison of an fp32 kernel) no reach-step has a recomputed clamped quantity
       within relative 1e-4 of its bound: the adjoint recomputes them to ~1e-6, so no mask can differ from the
       reference's."""
    a = cen["active"]
    for k in TARGETS[regime]:
        if k != "x_low":
            assert a[k].mean() >= 0.01, (regime, k, float(a[k].mean()))
    if regime == "flash":
        assert int(a["x_clear"][1:].sum()) >= 20, (regime, int(a["x_clear"][1:].sum()))
    if grads is not None:
        assert targeted(cen, regime).mean() >= 0.25, (regime, float(targeted(cen, regime).mean()))
        for k, g in grads.items():
            assert np.all(np.isfinite(g)), k
    if fp32_grads:
        assert int(cen["near"](NEAR_GRAD).sum()) == 0, (regime, int(cen["near"](NEAR_GRAD).sum()))


def unit_grads(case, bw):
    u64 = {k: v.astype(np.float64) for k, v in case.u.items()}
    return O.param_grads_from_unit(bw["n"], bw["q_spatial"], bw["p_spatial"], u64["n"], u64["q_spatial"],
                                   u64["p_spatial"], case.params["parameter_ranges"])


@functools.lru_cache(maxsize=None)
def tree_reference(regime, pname):
    """The 200-reach case with its CPU-side results, computed once and read only: the fp32 oracle's trajectory
    and the fp64 adjoint on it (what the fp32 kernels are compared with), the fp64 oracle's forward and adjoint
    (what the fp64 kernel is compared with), and the census of each trajectory."""
    case = tree_stress_case(regime, pname)
    onet = case.network()
    r32 = case.reaches()
    fw32 = O.route(onet, r32, case.qprime, case.bounds, dtype=np.float32)
    bw32 = O.route_backward(onet, r32, case.qprime, fw32["x"], case.W, case.bounds)
    u64 = {k: v.astype(np.float64) for k, v in case.u.items()}
    r64 = reaches_of(case, u64, np.float64)
    fw64 = O.route(onet, r64, case.qprime, case.bounds, dtype=np.float64)
    bw64 = O.route_backward(onet, r64, case.qprime, fw64["x"], case.W, case.bounds)
    return dict(case=case, onet=onet, u64=u64, fw32=fw32, cen32=census(case, r32, fw32["x"]),
                grads32=unit_grads(case, bw32), fw64=fw64, cen64=census(case, r64, fw64["x"], np.float64),
                grads64=unit_grads(case, bw64))


@pytest.mark.parametrize("regime,pname", CASES)
def test_stress_cases_meet_their_preconditions(regime, pname):
    """Preconditions 1-3 on the fp32 trajectory and 1-2 on the fp64 one; the oracle's gradients are finite and
    at least 20 % of the reaches carry an element above 1e-3 of the largest."""
    c = tree_reference(regime, pname)
    assert_preconditions(c["cen32"], regime, c["grads32"], fp32_grads=True)
    assert_preconditions(c["cen64"], regime, c["grads64"])
    for g in (c["grads32"], c["grads64"]):
        for k, v in g.items():
            assert np.mean(np.abs(v) >= 1e-3 * np.abs(v).max()) >= 0.2, k


@pytest.mark.parametrize("regime,pname", CASES)
def test_oracle_adjoint_matches_finite_differences_under_clamps(regime, pname):
    """``route_backward`` against central finite differences of the fp64 oracle's forward: one u element, h = 1e-6,
    the tolerance of test_gpu_route.test_finite_difference_gradient_fp64.  Three elements per parameter: the
    largest gradient elements among the reaches with a targeted clamp active and no clamped quantity within 1e-3
    of a bound (a kink inside the difference quotient would make it meaningless; a state that sits at q_lb
    to the last bits -- a dry headwater's steady state -- is no kink, it does not depend on the parameters).  The
    low regime's gradients are small, so the absolute part of the tolerance is scaled down to the parameter's
    largest gradient element: never looser than the stated tolerance."""
    c = tree_reference(regime, pname)
    case, onet, cen, grads = c["case"], c["onet"], c["cen64"], c["grads64"]
    xr = np.abs(cen["x"][1:] / cen["qlb"] - 1.0)
    kink = cen["near"](NEAR_FD).any(axis=0) | ((xr > 1e-12) & (xr < NEAR_FD)).any(axis=0)
    ok = np.flatnonzero(targeted(cen, regime) & ~kink)
    assert len(ok) >= 3, (regime, pname, len(ok))
    Wd = case.W.astype(np.float64)
    h = 1e-6
    for k, g in grads.items():
        scale = min(1.0, float(np.abs(g).max()))
        for i in ok[np.argsort(-np.abs(g[ok]))[:3]]:
            vals = []
            for s in (+1, -1):
                u2 = {kk: vv.copy() for kk, vv in c["u64"].items()}
                u2[k][i] += s * h
                res = O.route(onet, reaches_of(case, u2, np.float64), case.qprime, case.bounds, dtype=np.float64)
                vals.append(res["runoff"])
            # the loss difference summed from the element-wise differences: the reaches the element does not
            # reach cancel exactly instead of leaving the rounding of a sum 1e5 times the difference (high)
            fd = float(np.sum((vals[0] - vals[1]) * Wd)) / (2 * h)
            assert g[i] != 0.0, (k, i)
            assert abs(fd - g[i]) <= 1e-5 * max(scale, abs(fd)), (k, i, fd, g[i])
