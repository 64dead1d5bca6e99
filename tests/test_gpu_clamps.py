"""The routing kernels where the physics' clamps and their gradient masks are active.

The seven clamps of ddr_amd/csrc/physics.h (depth, side slope low / high, bottom width, velocity low / high,
the routed state and q' at q_lb) each have a gradient mask in three adjoints: ``coefficients_vjp`` (fp64),
``adjoint_step_fast<false>`` (the fp32 default) and ``adjoint_step_fast<true>`` (``exact_adjoint=True``); the
exact fp32 forward has a branch that exists only under the depth clamp (``coefficients_np``: the second pow's
logarithm is the host's ``ln_dlb``).  The inputs of the other device tests never reach the depth, velocity or
mid-run state clamps with gradients, so a wrong mask direction, a mask on the clamped instead of the raw value
or a wrong ``ln_dlb`` would pass them.  Here the three stress regimes of tests/test_clamp_cases.py (low, high,
flash; its docstring has the seeds, the share of reach-steps at which each clamp is active and the number of
recomputed quantities near a bound -- zero on every 200-reach case) go through every forward and adjoint:

  A  exact fp32 forward == fp32 oracle (max-rel <= 1e-6, observed 0) on the 200-reach tree (whole, cut at 64),
     a 3000-reach Hack basin (cut at 64, whole) and a 30 000-reach forest at four reaches per thread; bitwise
     equal between the partitions; the depth-clamped top width pins the ``ln_dlb`` branch
  B  math="fast" / "faithful" forwards within 1e-4 of the oracle and of the exact kernel, per reach scale;
     their gradients in the high regime (no stored state at a bound) within 5e-5 of the exact kernel's
  C  fp64 kernel == fp64 oracle: forward 1e-12, gradients 1e-10 (norm) and 1e-6 (every element), exact zeros
  D  both fp32 adjoints against the fp64 oracle adjoint on the same fp32 trajectory
  E  dL/dq' under the q' and state masks, inclusive at q' == q_lb

Every case asserts its preconditions on the CPU first (test_clamp_cases.assert_preconditions), on the oracle's
trajectory from the physical inputs the kernel saw.  Gradient measures: norm-relative and element-wise over the
elements above 1e-3 of the largest, over all reaches and -- because a velocity-clamped step contributes no
parameter gradient, which makes the clamped reaches the small elements -- over the targeted reaches alone, at
their own scale.
"""

import functools

import numpy as np
import pytest
import torch

from conftest import maxrel, normrel
from ddr_amd import synthetic
from oracle import mc_oracle as O
from test_clamp_cases import (CASES, PARAMS, assert_preconditions, census, stress_case, targeted, tree_stress_case,
                              unit_grads)
from test_gpu_exact_adjoint import maxrel_above
from test_gpu_route import run_hip

pytestmark = pytest.mark.gpu

CUT = {"max_block_reaches": 64, "target_blocks": 1 << 20}
WHOLE_CUT = pytest.mark.parametrize("gkw", [None, CUT], ids=["whole", "cut"])
# graph -> (T, seed of the case, partitions: the oracle comparison's inputs are taken from the first)
GRAPHS = {"tree": (48, None, (None, CUT)),
          "hack": (48, 4, (CUT, None)),
          "forest": (24, 12, ({"target_blocks": 8}, {"max_block_reaches": 500, "target_blocks": 1 << 20}))}
OUTPUTS = ("runoff", "q_last", "top_width", "side_slope")
GRADS = ("n", "q_spatial", "p_spatial")


@functools.lru_cache(maxsize=None)
def _net(graph):
    if graph == "hack":
        return synthetic.hack_basin(3000, seed=4)
    # the forest of test_gpu_route.test_faithful_partition_invariance_with_full_workgroups
    return synthetic.forest(synthetic.zipf_sizes(30000, 60, 0.4), seed=12, single_inflow=0.35)


@functools.lru_cache(maxsize=None)
def _case(graph, regime, pname):
    """Read-only: shared by the tests of a case."""
    if graph == "tree":
        return tree_stress_case(regime, pname)
    T, seed, _ = GRAPHS[graph]
    return stress_case(_net(graph), T, seed, PARAMS[pname], regime)


_REF = {}


def _reference(graph, regime, pname, reaches, dtype=np.float32):
    """The oracle's forward from the physical inputs the kernel saw and the census of its trajectory, computed
    once per case and precision (the device's denormalize is deterministic: later runs see the same inputs)."""
    key = (graph, regime, pname, dtype)
    if key not in _REF:
        case = _case(graph, regime, pname)
        onet = case.network()
        fw = O.route(onet, reaches, case.qprime, case.bounds, dtype=dtype)
        _REF[key] = dict(onet=onet, reaches=reaches, fw=fw, cen=census(case, reaches, fw["x"], dtype))
    ref = _REF[key]
    for a, b in zip((reaches.n, reaches.q, reaches.p, reaches.slope), (ref["reaches"].n, ref["reaches"].q,
                                                                      ref["reaches"].p, ref["reaches"].slope)):
        np.testing.assert_array_equal(a, b)
    return ref


def _adjoint(ref, case):
    """The fp64 oracle adjoint on the reference's own trajectory, as u gradients (once per reference)."""
    if "grads" not in ref:
        bw = O.route_backward(ref["onet"], ref["reaches"], case.qprime, ref["fw"]["x"], case.W, case.bounds)
        ref["grads"] = unit_grads(case, bw)
        ref["zero"] = np.all([v == 0.0 for v in ref["grads"].values()], axis=0)
    return ref["grads"]


def _scaled(a, b):
    """max |a - b| over each reach's own scale max_t |b| ((N, T) series)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.max(np.abs(b), axis=1, keepdims=True)))


# ---- A ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regime,pname", CASES)
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_exact_forward_matches_fp32_oracle(cuda, graph, regime, pname):
    """The exact fp32 forward is the fp32 oracle's (max-rel <= 1e-6, observed 0: bit for bit in every case here,
    the states below q_lb and below zero of flash included) and bitwise the same for every partition: one to
    four reaches per thread, with and without cut edges.  In the low regime 15-29 % of the reaches are
    depth-clamped at the last step, so their top width comes from the ``ln_dlb`` branch of coefficients_np."""
    case = _case(graph, regime, pname)
    runs = [run_hip(case, cuda, gkw=gkw, grads=False) for gkw in GRAPHS[graph][2]]
    info = [r["graph"].info for r in runs]
    assert any(i.n_cut > 0 for i in info)
    if graph == "forest":
        assert info[0].reaches_per_thread == 4 and info[1].reaches_per_thread in (1, 2)
    ref = _reference(graph, regime, pname, runs[0]["reaches"])
    assert_preconditions(ref["cen"], regime)
    if regime == "low":
        # the reported geometry is that of the state the last step read: the census' last row
        assert ref["cen"]["active"]["depth"][-1].mean() >= 0.10
    for res in runs:
        for k in OUTPUTS:
            err = maxrel(res[k], ref["fw"][k])
            print(f"{graph} {regime} {pname} {k}: max-rel vs fp32 oracle {err:.2e}")
            assert err <= 1e-6, k
    for res in runs[1:]:
        for k in OUTPUTS:
            np.testing.assert_array_equal(res[k], runs[0][k], err_msg=k)


# ---- B ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", ["fast", "faithful"])
@pytest.mark.parametrize("regime,pname", CASES)
@pytest.mark.parametrize("graph,gkw", [("tree", None), ("tree", CUT), ("hack", CUT)], ids=["tree", "tree_cut", "hack_cut"])
def test_approximate_forwards_within_tolerance(cuda, graph, gkw, regime, pname, math):
    """The clamps are continuous, so the approximate forwards keep the 1e-4 bar of test_gpu_fastmath.py under
    them -- measured on each reach's own scale max_t |Q|, since a state that is the cancelled difference of
    larger terms (flash) amplifies a relative error: against the fp32 oracle and against the exact kernel;
    top width and side slope (one value per reach) plain max-rel.  Measured: <= 2.9e-6 (fast) and <= 1.8e-6
    (faithful) over all four outputs and all cases."""
    case = _case(graph, regime, pname)
    res = run_hip(case, cuda, gkw=gkw, grads=False, math=math)
    exact = run_hip(case, cuda, gkw=gkw, grads=False)
    ref = _reference(graph, regime, pname, res["reaches"])
    assert_preconditions(ref["cen"], regime)
    for name, b in (("oracle", ref["fw"]), ("exact kernel", exact)):
        err = _scaled(res["runoff"], b["runoff"])
        last = float(np.max(np.abs(res["q_last"].astype(np.float64) - b["q_last"])
                            / np.max(np.abs(b["runoff"]), axis=1)))
        tw, ss = maxrel(res["top_width"], b["top_width"]), maxrel(res["side_slope"], b["side_slope"])
        print(f"{graph} {regime} {pname} {math} vs {name}: runoff {err:.2e} q_last {last:.2e} tw {tw:.2e} ss {ss:.2e}")
        assert err <= 1e-4 and last <= 1e-4, name
        assert tw <= 1e-4 and ss <= 1e-4, name


@pytest.mark.parametrize("math", ["fast", "faithful"])
@pytest.mark.parametrize("pname", list(PARAMS))
@WHOLE_CUT
def test_approximate_forward_gradients_high(cuda, gkw, pname, math):
    """Gradients behind an approximate forward, in the high regime only: there no stored state or q' sits at
    q_lb, so the forward's rounding cannot flip a mask of a stored value, and no recomputed quantity is within
    1e-4 of a bound (precondition 3).  Against the exact kernel's gradients, the bar of test_gpu_fastmath.py, over
    all reaches and over the velocity-clamped ones alone (measured <= 1.1e-5 fast, 2.7e-6 faithful); the reaches
    with an exactly zero gradient are the same."""
    case = _case("tree", "high", pname)
    res = run_hip(case, cuda, gkw=gkw, math=math)
    exact = run_hip(case, cuda, gkw=gkw)
    ref = _reference("tree", "high", pname, res["reaches"])
    a = ref["cen"]["active"]
    assert not a["x_low"].any() and not a["qp_low"].any()
    assert_preconditions(ref["cen"], "high", {k: exact[f"grad_{k}"] for k in GRADS}, fp32_grads=True)
    hit = targeted(ref["cen"], "high")
    for k in GRADS:
        g, e = res[f"grad_{k}"], exact[f"grad_{k}"]
        err, err_hit = normrel(g, e), normrel(g[hit], e[hit])
        print(f"high {pname} {math} grad_{k}: norm-rel vs exact kernel {err:.2e}, targeted reaches {err_hit:.2e}")
        assert err <= 5e-5, k
        assert err_hit <= 5e-5, k
        assert np.array_equal(g == 0.0, e == 0.0), k


# ---- C ----------------------------------------------------------------------------------------------------

def _dry_steady(ref, case):
    """(N,) bool: headwaters that stay in the dry steady state Q = q' clamp = q_lb at every step.  Their
    parameter gradient is zero in exact arithmetic -- x = (c3 + c4) q_lb and c3 + c4 = 1 whatever the
    parameters -- and a rounding residue of the cancelled c3 and c4 terms in floating point."""
    cen, qlb = ref["cen"], float(ref["cen"]["qlb"])
    Q = np.maximum(cen["x"], qlb)[:-1].astype(np.float64)
    steady = (np.abs(Q / qlb - 1.0) < 1e-12).all(axis=0) & (np.asarray(case.qprime)[:-1] <= qlb).all(axis=0)
    return steady & (ref["onet"].height == 0)


@pytest.mark.parametrize("regime,pname", CASES)
@WHOLE_CUT
def test_fp64_kernel_matches_fp64_oracle(cuda, gkw, regime, pname):
    """The fp64 kernel (coefficients_vjp) against the fp64 oracle: forward 1e-12, gradients norm-rel 1e-10 and
    every element to 1e-6 (the floor of test_gpu_route.test_fp64_matches_fp64_oracle keeps the exact zeros out
    of the division).  A reach whose velocity is clamped at every step (24 / 141 / 69 / 117 / 0 / 4 of the 200
    reaches in low default / mock, high default / mock, flash default / mock; depth-clamped as well at every
    step on 13 / 27 of low's) has an exactly zero gradient in the oracle and must have one in the kernel.

    The dry steady headwaters of the low regime (29 / 9 reaches) are the one place where an element-wise
    relative error means nothing: their gradient is zero in exact arithmetic and both sides hold the rounding
    residue of two cancelled terms, measured <= 1.2e-16 of the largest element in the oracle and in the kernel,
    with either sign.  Those elements are held to 1e-12 of the largest element on both sides instead: four
    orders above that residue, far below anything a wrong mask would leave."""
    case = _case("tree", regime, pname)
    res = run_hip(case, cuda, dtype=torch.float64, gkw=gkw)
    assert (res["graph"].info.n_cut > 0) == (gkw is not None)
    ref = _reference("tree", regime, pname, res["reaches"], np.float64)
    grads = _adjoint(ref, case)
    assert_preconditions(ref["cen"], regime, grads)
    for k in OUTPUTS:
        assert maxrel(res[k], ref["fw"][k]) <= 1e-12, k
    a = ref["cen"]["active"]
    assert np.array_equal(ref["zero"], (a["v_low"] | a["v_high"]).all(axis=0))
    if regime != "flash":
        assert ref["zero"].sum() >= 20
    dry = _dry_steady(ref, case) & ~ref["zero"]
    assert dry.sum() <= (30 if regime == "low" else 0)
    hit = targeted(ref["cen"], regime)
    for k, v in grads.items():
        g = res[f"grad_{k}"]
        top = float(np.abs(v).max())
        err, err_hit = normrel(g, v), normrel(g[hit], v[hit])
        elem = maxrel(g[~dry], v[~dry], floor=1e-30 * top)
        print(f"fp64 {regime} {pname} grad_{k}: norm-rel {err:.2e} targeted {err_hit:.2e} element-wise {elem:.2e}")
        assert err <= 1e-10 and err_hit <= 1e-10, k
        assert elem <= 1e-6, k
        assert np.all(np.abs(g[dry]) <= 1e-12 * top) and np.all(np.abs(v[dry]) <= 1e-12 * top), k
        assert np.all(g[ref["zero"]] == 0.0), k


# ---- D ----------------------------------------------------------------------------------------------------

# bars: twice the measured value (the test's docstring), not below the project's bars for an fp32 gradient
# (5e-5 norm-relative, 1e-4 element-wise), the norm-relative one never above 2e-4 (the suite's loosest, measured on
# a 529-deep basin).  Every norm-relative figure measured here is below 1.5e-5, so that bar is the floor
# throughout; (regime, exact_adjoint) -> element-wise bar over all reaches
FLOOR_NORM, FLOOR_ELEM, CEIL_NORM = 5e-5, 1e-4, 2e-4
D_NORM = FLOOR_NORM
D_ELEM = {("low", False): 2 * 2.72e-4, ("high", False): 2 * 4.15e-4, ("flash", False): FLOOR_ELEM,
          ("low", True): FLOOR_ELEM, ("high", True): 2 * 7.77e-5, ("flash", True): FLOOR_ELEM}


@pytest.mark.parametrize("exact_adjoint", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("regime,pname", CASES)
@WHOLE_CUT
def test_fp32_adjoints_on_the_fp32_trajectory(cuda, gkw, regime, pname, exact_adjoint):
    """Both fp32 adjoints (adjoint_step_fast<false> / <true>) against the fp64 oracle adjoint fed the fp32
    forward's own states -- the fp32 oracle's, which the kernel's forward equals bit for bit (asserted) -- so
    every mask is evaluated on the same trajectory, and with no recomputed quantity within 1e-4 of a bound
    (precondition 3) every mask has the same value on both sides.  Reaches whose velocity is clamped at every
    step have exactly zero gradients.

    Measured on an MI355X, the larger of the two parameter sets and of whole / cut (which agree to the digits
    shown), n / q_spatial / p_spatial:

                       norm-relative                 element-wise, elements above 1e-3 of the largest
      low    default   3.6e-6 / 1.5e-5 / 1.1e-5      2.7e-4 / 2.7e-4 / 2.7e-4   targeted reaches 1.3e-5
             exact     2.7e-7 / 4.1e-7 / 3.0e-7      7.6e-6 / 9.7e-6 / 1.0e-5                    1.0e-5
      high   default   2.3e-6 / 2.4e-6 / 1.7e-6      4.2e-4 / 7.6e-5 / 3.8e-4                    6.0e-6
             exact     1.0e-6 / 2.3e-6 / 1.4e-6      7.8e-5 / 2.7e-5 / 7.8e-5                    8.5e-6
      flash  default   7.4e-7 / 1.7e-6 / 1.0e-6      3.1e-5 / 3.0e-5 / 3.1e-5   (every reach is targeted)
             exact     2.9e-7 / 4.3e-7 / 3.2e-7      9.1e-6 / 2.8e-5 / 1.1e-5

    The targeted reaches' norm-relative errors are <= 2.2e-6.  Where the default adjoint exceeds the 1e-4
    element-wise bar (low, high) it does so on unclamped reaches with elements near 1e-3 of the largest -- the
    cancellation of Q(t-1) - x(t) in the stored fp32 states that exact_adjoint removes (physics.h), not a mask:
    on the clamped reaches it is within 1.3e-5.  The targeted reaches are therefore held to the project's bars
    (5e-5, 1e-4) in every case."""
    case = _case("tree", regime, pname)
    res = run_hip(case, cuda, gkw=gkw, exact_adjoint=exact_adjoint)
    ref = _reference("tree", regime, pname, res["reaches"])
    grads = _adjoint(ref, case)
    assert_preconditions(ref["cen"], regime, grads, fp32_grads=True)
    np.testing.assert_array_equal(res["runoff"], ref["fw"]["runoff"])  # the oracle's states are the kernel's
    hit = targeted(ref["cen"], regime)
    bar_norm, bar_elem = D_NORM, D_ELEM[regime, exact_adjoint]
    assert FLOOR_NORM <= bar_norm <= CEIL_NORM and bar_elem >= FLOOR_ELEM
    errs = {}
    for k, v in grads.items():
        g = res[f"grad_{k}"]
        errs[k] = (normrel(g, v), maxrel_above(g, v, 1e-3), normrel(g[hit], v[hit]), maxrel_above(g[hit], v[hit], 1e-3))
        print(f"fp32 {regime} {pname} {'exact' if exact_adjoint else 'default'} {'cut' if gkw else 'whole'} grad_{k}: "
              "norm-rel %.2e element-wise %.2e targeted norm-rel %.2e element-wise %.2e" % errs[k])
    for k, e in errs.items():
        assert e[0] <= bar_norm and e[2] <= FLOOR_NORM, (k, e)
        assert e[1] <= bar_elem and e[3] <= FLOOR_ELEM, (k, e)
        assert np.all(res[f"grad_{k}"][ref["zero"]] == 0.0), k


# ---- E ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regime,pname", [c for c in CASES if c[0] != "high"])
@WHOLE_CUT
def test_fp64_qprime_gradient_under_the_masks(cuda, gkw, regime, pname):
    """dL/dq' of the fp64 kernel: exactly zero where q' < q_lb from the second row on (more than half of low's
    entries, the zero hours of flash; q'[0] also feeds the hot start, unclamped), equal to the oracle's nonzero
    value where q' == q_lb -- the mask is inclusive, like torch.clamp's backward.  40 entries are pinned: 20 to
    the bound itself as the fp64 kernel holds it (the double 1e-4 or 0.001) and 20 to the bound rounded to
    fp32, which lies 2.5e-8 (relative) below the double 1e-4 -- zero gradient -- and 4.7e-8 above 0.001, so
    both sides of the kink are held within 5e-8 of it.  Where a state is clamped in the middle of the run (C
    covers its mask through the parameters), dL/dq' of the step feeding it matches the oracle: zero in the
    zero hours, elsewhere what the reaches downstream pass back."""
    case = _case("tree", regime, pname)
    bd = case.bounds
    T, N = case.qprime.shape
    rng = np.random.default_rng(77)
    qp = case.qprime.astype(np.float64)
    flat = rng.choice((T - 2) * N, 40, replace=False)
    tt, ii = 1 + flat // N, flat % N
    qp[tt[:20], ii[:20]] = bd.discharge
    qp[tt[20:], ii[20:]] = float(np.float32(bd.discharge))
    res = run_hip(case, cuda, dtype=torch.float64, gkw=gkw, qprime=qp, qprime_grad=True)
    onet = case.network()
    fw = O.route(onet, res["reaches"], qp, bd, dtype=np.float64)
    assert maxrel(res["runoff"], fw["runoff"]) <= 1e-12
    bw = O.route_backward(onet, res["reaches"], qp, fw["x"], case.W, bd, want_qprime=True)
    want, got = bw["qprime"], res["grad_qprime"]
    assert normrel(got, want) <= 1e-10
    below = qp < bd.discharge
    below[0] = False  # q'[0] also feeds the hot start, which takes it unclamped (mmc.py:25-66)
    assert below.mean() >= 0.05
    assert np.all(got[below] == 0.0) and np.all(want[below] == 0.0)
    at = (tt[:20], ii[:20])
    assert np.all(want[at] != 0.0)
    assert maxrel(got[at], want[at]) <= 1e-10
    f32 = (tt[20:], ii[20:])
    if float(np.float32(bd.discharge)) < bd.discharge:
        assert np.all(got[f32] == 0.0)
    else:
        assert np.all(want[f32] != 0.0) and maxrel(got[f32], want[f32]) <= 1e-10
    assert np.all(got[-1] == 0.0)  # q'[T-1] feeds no step
    if regime == "flash":
        # the steps feeding a state clamped mid-run: x[t] < q_lb (t >= 2) takes q'[t-1], most of them zero hours
        xt, xi = np.nonzero(fw["x"][2:] < bd.discharge * (1.0 - 1e-6))
        assert len(xt) >= 20
        feed = (xt + 1, xi)
        assert np.array_equal(got[feed] == 0.0, want[feed] == 0.0)
        assert np.max(np.abs(got[feed] - want[feed])) <= 1e-10 * np.max(np.abs(want))
