"""The one-step physics and its adjoints over the parameter box (tests/physics_box.py), on the device.

Every forward coefficient form of ddr_amd/csrc/physics.h -- ``coefficients_np<R, NP>`` at one, two and four reaches
per thread, ``coefficients_faithful``, ``coefficients_fast`` -- and every adjoint -- ``coefficients_vjp`` (fp64),
``adjoint_step_fast<false>`` / ``<true>`` -- is evaluated once per point of the box: 60 000 reaches, a carried
two-step window, on both graphs (isolated reaches; chains 2i -> 2i + 1) and both parameter sets.  The box, its edge
planes, the references and the two exclusion masks (``tie``, ``near``) are physics_box's; the CPU side of this
file's preconditions is tests/test_physics_box.py.

  A  exact fp32 forward: bitwise the fp32 oracle outside the pow-tie mask (which is empty on this seed), bitwise
     equal between one, two and four reaches per thread; the same at the smallest T with a steady tick
  B  fp64 forward within 1e-12 of the fp64 oracle, x1 against the scale |Q| + |q'c| + |Sx| + |I| that does not cancel
  C  math="faithful" / "fast": geometry within 1e-4 per element; x1's error e on that scale, faithful by quantile
     against the fp32 oracle's own e, fast <= 1e-4
  D  gradients of sum(w runoff[:, 1]), w random signed: the fp64 kernel to 1e-6 per element; the fp32 adjoints
     against the fp64 VJP of the same fp32 inputs -- equal zero patterns, 5e-5 norm-relative, and the per-element
     error by quantile within C_RATIO of T's (PyTorch fp32 autograd of the same step on the CPU)

The kernel exposes x1 as runoff[:, 1] = max(x1, q_lb): both sides of every x1 comparison are clamped, and the
quantiles of e are taken over the points whose reference x1 is above q_lb (on the others both sides are q_lb and
e = 0, 35-42 % of the box; the maximum is over all points).

Measured on an MI355X (DESIGN.md section 5 has the tables): A 0 differing points of 60 000 in every case and
partition; B x1 <= 7.6e-16, geometry <= 6.7e-16; C faithful 1.00-1.14 times the fp32 oracle's e (max e 3.7e-7),
geometry 5.6e-7, fast max e 6.7e-7, geometry 1.4e-6; D fp64 element-wise <= 9.2e-11, fp32 norm-relative <= 6.3e-7,
quantile ratios to T <= 2.15.
"""

import numpy as np
import pytest
import torch

import physics_box as PB
from conftest import normrel
from ddr_amd.graph import RiverGraph
from ddr_amd.ops import RouteConsts, route
from oracle import mc_oracle as O
from tail_cases import MARGIN

pytestmark = pytest.mark.gpu

CASES = [(p, g) for p in PB.PARAMS for g in PB.GRAPHS]
CAPS = {256: 1, 1536: 2, 4096: 4}   # max_block_reaches (target_blocks = 16) -> reaches per thread
FP64_CAP = 1536                      # fp64 blocks of 4096 reaches do not fit a CU's LDS
OUTPUTS = ("runoff", "q_last", "top_width", "side_slope")
PARAM_GRADS = ("n", "q_spatial", "p_spatial")
ALL_GRADS = PARAM_GRADS + ("q0", "qprime")
E_QUANTILES = (0.5, 0.99, 0.999, 1.0)
# D: the fp32 adjoints' per-element relative error at each of PB.QUANTILES may be this many times T's: twice the
# largest ratio measured on an MI355X over both adjoints, graphs, parameter sets, runs and the five gradients,
# 2.15 (dL/dQ0, exact adjoint, mock, isolated, quantile 0.999; DESIGN.md section 5 has the table).  For
# dL/d(n, q, p) the largest is 1.40: one step's per-element error is the conditioning of the fp32 forward values
# both sides share, not the hardware rcp / log / exp, which would have allowed 16 to 64.
C_RATIO = 4.3


def consts_of(bd):
    return RouteConsts(discharge_lb=bd.discharge, velocity_lb=bd.velocity, depth_lb=bd.depth,
                       bottom_width_lb=bd.bottom_width)


def qprime_rows(b, T):
    """(T, N) float32: row 0 is the box's q'; later rows (T > 2) scale it so that the trajectory moves."""
    f = np.array([1.0, 0.5, 2.0, 1.0, 0.25, 4.0][:T], np.float32)
    return (f[:, None] * b.qp[None, :]).astype(np.float32)


def run_box(pname, graph, dev, dtype=torch.float32, cap=4096, math="exact", exact_adjoint=False, grads=(), T=2):
    """One launch over the box.  ``grads``: () forward only, PARAM_GRADS, or ALL_GRADS (dL/dQ0 and dL/dq' too: the
    general adjoint kernel).  Returns numpy outputs, ``grad_<name>`` and the graph's info."""
    b = PB.box(pname)
    tt = lambda a: torch.from_numpy(np.array(a)).to(dev, dtype)  # noqa: E731
    t = {k: tt(getattr(b, k)) for k in PB.FIELDS if k != "qp"}
    qp = tt(qprime_rows(b, T))
    leaves = {"n": t["n"], "q_spatial": t["q"], "p_spatial": t["p"], "q0": t["Q"], "qprime": qp}
    for k in grads:
        leaves[k].requires_grad_(True)
    rows, cols = PB.coo(graph)
    g = RiverGraph(PB.N, rows, cols, max_block_reaches=cap, target_blocks=16)
    runoff, q_last, tw, ss = route(g, qp, t["n"], t["q"], t["p"], t["length"], t["slope"], t["X"], q0=t["Q"],
                                   consts=consts_of(b.bounds), math=math, exact_adjoint=exact_adjoint)
    out = {"runoff": runoff, "q_last": q_last, "top_width": tw, "side_slope": ss}
    out = {k: v.detach().cpu().numpy() for k, v in out.items()}
    out["info"] = g.info
    if grads:
        (runoff[:, 1] * tt(PB.weights())).sum().backward()
        for k in grads:
            out[f"grad_{k}"] = leaves[k].grad.detach().cpu().numpy()
    torch.cuda.synchronize()
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


# ---- A ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pname,graph", CASES)
def test_exact_forward_is_the_fp32_oracle_over_the_box(cuda, pname, graph):
    """``coefficients_np<float, 1 / 2 / 4>`` (runoff[:, 1]) and ``route_last_kernel`` (top width, side slope) are
    the fp32 oracle bit for bit on every point outside the pow-tie mask, and bit for bit each other on every
    point; inside the mask the geometry is within 2 ulp.  This pins pow_pos's stated error (3e-16: the mask is 50
    times as wide), the shared logarithm of the two pows (ln pw = z + log1p(u)), the ``ln_dlb`` branch at
    pw == depth_lb and its neighbours, ln_tab at ratio = 2^j, 2^j +- 1 and 2 ulp, div_rn on the negative and
    cancelling numerators of c1 and c3, and sqrt_rn_normal up to 1 + 50^2."""
    ref = PB.reference(pname, graph)
    fw = ref.s32["fw"]
    keep = ~ref.tie
    runs = {}
    for cap, kr in CAPS.items():
        runs[cap] = res = run_box(pname, graph, cuda, cap=cap)
        assert res["info"].reaches_per_thread == kr, cap
        for k in OUTPUTS:
            want = fw[k]
            diff = bits(res[k]) != bits(want)
            bad = diff[keep] if diff.ndim == 1 else diff[keep].any(axis=1)
            print(f"{pname} {graph} kr={kr} {k}: {int(bad.sum())} points differ from the fp32 oracle outside the "
                  f"mask ({int(ref.tie.sum())} masked)")
            assert not bad.any(), (k, cap, np.flatnonzero(keep)[np.flatnonzero(bad)[:5]])
        for k in ("top_width", "side_slope"):
            assert np.all(PB.ulp_distance(res[k][ref.tie], fw[k][ref.tie]) <= 2), k
    for cap in list(CAPS)[1:]:
        for k in OUTPUTS:
            np.testing.assert_array_equal(bits(runs[cap][k]), bits(runs[256][k]), err_msg=f"{k} {cap}")


@pytest.mark.parametrize("pname,graph", CASES)
def test_exact_forward_steady_tick_is_the_fp32_oracle(cuda, pname, graph):
    """T = 4, the smallest T at which ``route_forward_kernel`` runs a steady tick on these graphs: the steady ticks
    are [s0, s1) with s0 = dmax + 1 rounded up to even and s1 = T rounded down to even (route_forward.hip, the
    tick loops), and dmax, the largest in-block distance to a root, is 0 on the isolated reaches and 1 on the
    chains, so s0 = 2 on both and s1 > s0 needs T >= 4 (ticks 2 and 3).  The whole trajectory (q' scaled by 1,
    0.5, 2 per step) is the fp32 oracle's bit for bit at four reaches per thread, on the points whose pows stay
    clear of a rounding tie at every step."""
    b, T = PB.box(pname), 4
    qp = qprime_rows(b, T)
    net, bd = PB.network(graph), b.bounds
    fw = O.route(net, PB.reaches(b), qp, bd, q0=b.Q, dtype=np.float32)
    tie = np.zeros(PB.N, bool)
    states = np.maximum(fw["x"], np.float32(bd.discharge))
    states[0] = b.Q
    for t in range(T - 1):
        tie |= PB.pow_tie(O.trapezoid_celerity(states[t], b.n, b.q, b.p, b.slope, bd, np.float32, full=True))
    tie = PB.as_unit(tie, graph)
    assert tie.mean() <= 1e-4
    res = run_box(pname, graph, cuda, cap=4096, T=T)
    assert res["info"].reaches_per_thread == 4 and res["info"].max_depth <= 2
    for k in OUTPUTS:
        diff = bits(res[k]) != bits(fw[k])
        bad = diff[~tie] if diff.ndim == 1 else diff[~tie].any(axis=1)
        print(f"{pname} {graph} T=4 {k}: {int(bad.sum())} points differ ({int(tie.sum())} masked)")
        assert not bad.any(), k


# ---- B ----------------------------------------------------------------------------------------------------

def _x1_error(res, s64, bd):
    """e per point: |runoff[:, 1] - max(x1, q_lb)| of the fp64 oracle over |Q| + |q'c| + |Sx| + |I|."""
    want = np.maximum(s64["x1"], bd.discharge)
    return np.abs(res["runoff"][:, 1].astype(np.float64) - want) / s64["scale"]


@pytest.mark.parametrize("pname,graph", CASES)
def test_fp64_forward_over_the_box(cuda, pname, graph):
    """``coefficients_np<double, 4>`` and the fp64 ``route_last_kernel``: x1 within 1e-12 of the scale that does
    not cancel, top width and side slope 1e-12 relative."""
    ref = PB.reference(pname, graph)
    res = run_box(pname, graph, cuda, dtype=torch.float64, cap=FP64_CAP)
    s, bd = ref.s64, ref.box.bounds
    e = _x1_error(res, s, bd)
    tw = np.abs(res["top_width"] / s["fw"]["top_width"] - 1.0)
    ss = np.abs(res["side_slope"] / s["fw"]["side_slope"] - 1.0)
    print(f"fp64 {pname} {graph}: x1 max e {e.max():.2e}, top width {tw.max():.2e}, side slope {ss.max():.2e}")
    assert e.max() <= 1e-12
    assert tw.max() <= 1e-12 and ss.max() <= 1e-12
    np.testing.assert_array_equal(res["q_last"], res["runoff"][:, 1])
    np.testing.assert_array_equal(res["runoff"][:, 0], np.maximum(ref.box.Q.astype(np.float64), bd.discharge))


# ---- C ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math", ["faithful", "fast"])
@pytest.mark.parametrize("pname,graph", CASES)
def test_approximate_forwards_over_the_box(cuda, pname, graph, math):
    """``coefficients_faithful`` / ``coefficients_fast`` against the fp64 oracle of the same fp32 inputs.  Top
    width and side slope do not cancel: 1e-4 per element, the project's bar.  x1 does (c3 < 0 on 55 % of the box):
    its error e is taken on the scale |Q| + |q'c| + |Sx| + |I|.  Faithful is the fp32 oracle's operation sequence
    with 1-ulp pows in place of correctly rounded ones, so at the quantiles 0.5, 0.99, 0.999 and the maximum its
    e is within tail_cases.MARGIN of the fp32 oracle's own; fast (c3 = 1 - c4, hardware rcp / log / exp) keeps
    max e <= 1e-4."""
    ref = PB.reference(pname, graph)
    res = run_box(pname, graph, cuda, math=math)
    s, bd = ref.s64, ref.box.bounds
    for k in ("top_width", "side_slope"):
        err = float(np.max(np.abs(res[k].astype(np.float64) / s["fw"][k] - 1.0)))
        print(f"{math} {pname} {graph} {k}: max-rel vs fp64 oracle {err:.2e}")
        assert err <= 1e-4, k
    e = _x1_error(res, s, bd)
    e32 = np.abs(np.maximum(ref.s32["x1"], np.float32(bd.discharge)).astype(np.float64)
                 - np.maximum(s["x1"], bd.discharge)) / s["scale"]
    live = s["x1"] > bd.discharge
    assert live.mean() >= 0.5
    qe, q32 = np.quantile(e[live], E_QUANTILES[:-1]), np.quantile(e32[live], E_QUANTILES[:-1])
    qe, q32 = np.append(qe, e.max()), np.append(q32, e32.max())
    print(f"{math} {pname} {graph} x1 e at {E_QUANTILES}: kernel {qe}, fp32 oracle {q32}, ratio {qe / q32}")
    if math == "faithful":
        assert np.all(q32 > 0.0)
        assert np.all(qe <= MARGIN * q32), (qe, q32)
    else:
        assert e.max() <= 1e-4


# ---- D ----------------------------------------------------------------------------------------------------

def _zeros_equal(g, v, keep, what):
    same = (g == 0.0) == (v == 0.0)
    assert np.all(same[keep]), (what, int((~same[keep]).sum()), np.flatnonzero(keep & ~same)[:5])


@pytest.mark.parametrize("grads", [PARAM_GRADS, ALL_GRADS], ids=["params", "all"])
@pytest.mark.parametrize("pname,graph", CASES)
def test_fp64_adjoint_over_the_box(cuda, pname, graph, grads):
    """``coefficients_vjp<double>``: every element of every gradient within 1e-6 of the fp64 oracle's VJP (the
    element-wise bar of test_gpu_route.test_fp64_matches_fp64_oracle) outside the near-bound mask; a zero of the
    oracle -- a velocity-clamped reach, a state or q' below q_lb -- is an exact zero of the kernel and the
    reverse.  With dL/dQ0 and dL/dq' asked for, the general adjoint kernel runs."""
    ref = PB.reference(pname, graph)
    res = run_box(pname, graph, cuda, dtype=torch.float64, cap=FP64_CAP, grads=grads)
    assert _x1_error(res, ref.s64, ref.box.bounds).max() <= 1e-12
    keep = ~ref.near
    d, bd = ref.s64["d"], ref.box.bounds
    vclamped = (d["v"] < bd.velocity) | (d["v"] > bd.velocity_max)
    for k in grads:
        v = ref.vjp64[k]
        g = res[f"grad_{k}"] if k != "qprime" else res["grad_qprime"][0]
        _zeros_equal(g, v, keep, k)
        if k in PARAM_GRADS and graph == "isolated":
            assert np.all(g[vclamped & keep] == 0.0) and (vclamped & keep).mean() >= 0.05, k
        nz = keep & (v != 0.0)
        err = float(np.max(np.abs(g[nz] - v[nz]) / np.abs(v[nz])))
        print(f"fp64 {pname} {graph} d/d{k}: max element-wise {err:.2e}, norm-rel {normrel(g[keep], v[keep]):.2e}")
        assert err <= 1e-6, k
    if "qprime" in grads:
        assert np.all(res["grad_qprime"][1] == 0.0)  # row 1 feeds no step


@pytest.mark.parametrize("exact_adjoint", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("grads", [PARAM_GRADS, ALL_GRADS], ids=["params", "all"])
@pytest.mark.parametrize("pname,graph", CASES)
def test_fp32_adjoints_over_the_box(cuda, pname, graph, grads, exact_adjoint):
    """``adjoint_step_fast<false>`` / ``<true>`` against the fp64 oracle VJP of the same fp32 inputs on the fp32
    forward's own states (the fp32 oracle's, which the kernel's equal bit for bit: asserted).  Outside the
    near-bound mask every gradient mask has the same value on both sides, so the zero patterns are equal; the
    norm-relative error over the box is within the project's 5e-5; and the per-element relative error, which is
    conditioning and not a defect (T, PyTorch's own fp32 autograd of this step, reaches 5e-3 on p at the 0.999
    quantile), is held at each of the quantiles 0.5, 0.9, 0.99, 0.999 to C_RATIO times T's."""
    ref = PB.reference(pname, graph)
    res = run_box(pname, graph, cuda, grads=grads, exact_adjoint=exact_adjoint)
    np.testing.assert_array_equal(bits(res["runoff"])[~ref.tie], bits(ref.s32["fw"]["runoff"])[~ref.tie])
    keep = ~ref.near & ~ref.tie
    tag = f"fp32 {'exact' if exact_adjoint else 'default'} {pname} {graph} {'all' if 'q0' in grads else 'params'}"
    for k in grads:
        v = ref.vjp32[k]
        g = res[f"grad_{k}"] if k != "qprime" else res["grad_qprime"][0]
        assert np.all(np.isfinite(g)), k
        _zeros_equal(g, v, keep, k)
        nr = normrel(g[keep], v[keep])
        qk, qt = PB.rel_quantiles(g, v, keep), ref.t_quantiles[k]
        ratio = qk / qt
        print(f"{tag} d/d{k}: norm-rel {nr:.2e}; element-wise at {PB.QUANTILES}: kernel {qk}, T {qt}, ratio {ratio}")
        assert nr <= 5e-5, k
        assert np.all(qk <= C_RATIO * qt), (k, ratio)
    if "qprime" in grads:
        assert np.all(res["grad_qprime"][1] == 0.0)
