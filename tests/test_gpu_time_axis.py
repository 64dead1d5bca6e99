"""The fused routing kernels along the time axis: every window phase and edge.

The kernels branch on the window length T (tests/time_axis_cases.py lists the branches and builds the cases;
tests/test_time_axis_cases.py asserts that the window lengths below reach each of them and checks the oracle
itself on the time axis).  One parametrized case is one window length:

  1  fp64 kernel == fp64 oracle on the 300-reach tree S, whole and cut, T in 1..17, 125..133, 253..259 and
     dmax - 1 .. dmax + 6, modes reach / gauge / carry / state / state_carry / seed: outputs 1e-12, every
     gradient (n, q_spatial, p_spatial, q', Q0) 1e-10 norm-relative and 1e-6 on every element; no parameter
     gradient at all at T = 1
  2  exact fp32 forward == fp32 oracle (1e-6; the number of differing values is printed) on S and on the
     3758-reach forest L at one reach per thread; both fp32 adjoints against the fp64 adjoint of that fp32
     trajectory (5e-5 default, 1e-5 exact_adjoint)
  3  one, two and four reaches per thread (L at block caps 256 / 1536 / 4096) are bitwise the same, exact and
     faithful arithmetic, outputs and every gradient, at every T of the sweep
  4  the debug-flag twins (no steady ticks, no storer waves, no plain instances) are bitwise the default at
     ragged T around dmax and around the 128-step flush
  5  q' stores of 2, 3, 7 and 24 hours per row (partial last rows, a missing divide, flow_scale; dL/dq' in the
     store's own shape) and the daily objective's window (L = T - 21 not a multiple of 24)
  6  a window equals, bit for bit, its first T1 steps followed by a window that carries their final state

A hot-started window whose steps all read one q' row (T = 2; a store window inside its first row) stays in the
hot start's steady state: its parameter gradients are what cancelled terms leave and are held to the same bars
as an error over the terms' scale (time_axis_cases.steady_window).

Measured on an MI355X: fp64 outputs <= 9.1e-13, gradients <= 5.7e-13 norm-relative and <= 9.4e-11 on every
element; the exact fp32 forward differs from the fp32 oracle in 0 values at every T; fp32 gradients on S
<= 1.7e-5 (default; <= 3.4e-7 up to T = 8) and <= 5.6e-6 (exact_adjoint) at every T; on L <= 5e-5 (default) except gauge
mode at T = 48 ... 51 (<= 7.7e-5, where the oracle's own fp32 sweep is 4.6e-5 ... 5.3e-5 from the fp64 one: the bound
there is twice that), exact_adjoint <= 2.8e-6; steady windows <= 5.7e-15 (fp64) and <= 5.2e-8 (fp32) of the
terms' scale.  283 cases in 51 s, the slowest 1.9 s.

Found and fixed: the default fp32 adjoint was 1.3e-4 (T = 3, gauge mode, q_spatial; p_spatial 6.7e-5; per-reach
runoff 5.2e-5) and 5.2e-5 (T = 4, gauge mode, q_spatial) from the fp64 adjoint, over the 5e-5 bar, and 2.5e-5 /
1.4e-5 at T = 5 / 6.  Two or three steps after a hot start the flow is close to the hot start's steady state and
the gradient is the small remainder of nearly cancelled terms (1e-2 ... 1e-3 of their scale): the default adjoint
forms Q - x~ from the stored fp32 x(t), whose rounding is of that remainder's size (physics.h).  Hot-started
windows of at most 8 steps now run the exact adjoint's kernel (route_backward.h, backward_exact_of), which held
3.5e-7 / 5.1e-7 there; the default and exact_adjoint=True runs of such a window are bitwise the same (asserted).
"""

import functools

import numpy as np
import pytest
import torch

import time_axis_cases as C
from conftest import maxrel, normrel
from ddr_amd import _lib
from ddr_amd.graph import RiverGraph
from ddr_amd.ops import DailyWindow, GaugeMap, route
from ddr_amd.routing.utils import denormalize
from oracle import mc_oracle as O
from test_gpu_route import consts_of

pytestmark = pytest.mark.gpu

T_S = C.t_sweep("S", C.S_PARTS)
T_L = C.t_sweep("L", C.L_PARTS)
T_L256 = tuple(sorted(set(C.T_FLUSH) | set(C.t_depth(C.host_info("L", 256)))))
STATE_GRADS = ("qprime", "q0")
FLAGS = {"no_steady": _lib.DDR_DEBUG_NO_STEADY, "no_storer": _lib.DDR_DEBUG_NO_STORER,
         "no_plain": _lib.DDR_DEBUG_NO_PLAIN}


@functools.lru_cache(maxsize=None)
def _graph(name, part):
    net = C.network(name)
    g = RiverGraph(net.n, net.rows, net.cols, **C.partition(name, part))
    want = C.host_info(name, part)
    assert (g.info.reaches_per_thread, g.info.n_cut, g.info.max_block_depth) == \
        (want.reaches_per_thread, want.n_cut, want.max_block_depth)
    return g


def run(case, dev, g, inp, dtype=torch.float32, math="exact", exact_adjoint=False, flags=0, grads=True):
    """Reference recipe on the device (denormalize in torch, fused route, backward) for a mode's inputs."""
    rng, ls = case.params["parameter_ranges"], case.params["log_space_parameters"]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)  # noqa: E731
    u = {k: tt(v).requires_grad_(grads) for k, v in case.u.items()}
    n, q, p = (denormalize(u[k], rng[k], k in ls) for k in C.PARAM_GRADS)
    slope = torch.clamp(tt(case.slope), min=case.params["attribute_minimums"]["slope"])
    T = case.qprime.shape[0]
    kw = {}
    if "store" in inp:
        qp = tt(inp["store"])
        kw = dict(steps=T, qprime_hours=inp["hours"], qprime_valid=torch.from_numpy(inp["valid"]))
    else:
        qp = tt(case.qprime)
    if "window" in inp:
        kw["daily"] = inp["window"]
    state = grads and inp["qprime_grad"]
    qp.requires_grad_(state)
    q0 = None if inp["q0"] is None else tt(inp["q0"]).requires_grad_(state)
    gz = None if inp["gauges"] is None else GaugeMap.build(inp["gauges"], case.n, dev)
    fs = None if inp["flow_scale"] is None else tt(inp["flow_scale"])
    lib = _lib.load()
    _lib.check(lib.ddr_set_debug_flags(flags))
    try:
        runoff, q_last, tw, ss = route(g, qp, n, q, p, tt(case.length), slope, tt(case.x), flow_scale=fs, q0=q0,
                                       gauges=gz, consts=consts_of(case), math=math, exact_adjoint=exact_adjoint,
                                       **kw)
        out = {"runoff": runoff.detach().cpu().numpy(), "q_last": q_last.detach().cpu().numpy(),
               "top_width": tw.detach().cpu().numpy(), "side_slope": ss.detach().cpu().numpy()}
        if grads:
            loss = (runoff * tt(inp["W"])).sum()
            if inp["V"] is not None:
                V = tt(inp["V"])
                loss = loss + (q_last * V[0]).sum()
                if T >= 2:  # a one-step window reports no geometry
                    loss = loss + (tw * V[1]).sum() + (ss * V[2]).sum()
            loss.backward()
            for k, v in u.items():
                out[f"grad_{k}"] = v.grad.detach().cpu().numpy()
            if state:
                out["grad_qprime"] = qp.grad.detach().cpu().numpy()
                if q0 is not None:
                    out["grad_q0"] = q0.grad.detach().cpu().numpy()
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.ddr_set_debug_flags(0))
    npd = np.float64 if dtype == torch.float64 else np.float32
    out["reaches"] = O.Reaches(n.detach().cpu().numpy(), q.detach().cpu().numpy(), p.detach().cpu().numpy(),
                               case.length.astype(npd), slope.detach().cpu().numpy(), case.x.astype(npd))
    return out


_REF = {}


def _reference(key, reaches, make):
    """An oracle reference, computed once per key from the physical inputs the kernel saw (the device's
    denormalize is deterministic: later runs of the key see the same inputs, asserted) and left unchanged."""
    if key not in _REF:
        _REF[key] = (reaches, make())
    first, ref = _REF[key]
    for a, b in zip((reaches.n, reaches.q, reaches.p, reaches.slope), (first.n, first.q, first.p, first.slope)):
        np.testing.assert_array_equal(a, b)
    return ref


def _mode_reference(name, T, mode, reaches, dtype):
    case, inp = C.window_case(name, T), C.mode_inputs(name, T, mode)
    return _reference((name, T, mode, dtype), reaches, lambda: C.oracle_reference(case, inp, reaches, dtype))


def _wanted_grads(ref):
    """name -> reference array, for every gradient the mode has."""
    want = {f"grad_{k}": v for k, v in ref["grads"].items()}
    for k in STATE_GRADS:
        if ref.get(k) is not None:
            want[f"grad_{k}"] = ref[k]
    return want


def _forward_errors(res, fw, T):
    """max-rel of the four outputs; a one-step window reports no geometry (zeros; the oracle: nothing)."""
    errs = {}
    for k in C.OUTPUTS:
        if T == 1 and k in ("top_width", "side_slope"):
            assert np.all(res[k] == 0.0) and fw[k].size == 0, k
            continue
        assert res[k].shape == fw[k].shape, k
        errs[k] = maxrel(res[k], fw[k])
    return errs


def _differing(res, fw, T):
    return sum(int(np.count_nonzero(res[k] != fw[k])) for k in C.OUTPUTS
               if not (T == 1 and k in ("top_width", "side_slope")))


def _steady_note(worst):
    return f", steady-window parameter gradients {worst['steady']:.2e} of the terms' scale" if "steady" in worst else ""


def _assert_bitwise(a, b, tag):
    keys = [k for k in a if k != "reaches"]
    assert set(keys) == {k for k in b if k != "reaches"}, tag
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (tag, k)
    return len(keys)


# ---- 1: fp64 kernel against the fp64 oracle ---------------------------------------------------------------

def _check_fp64(res, ref, T, tag, worst):
    fails = []
    for k, e in _forward_errors(res, ref["fw"], T).items():
        worst["fwd"] = max(worst["fwd"], e)
        if not e <= 1e-12:
            fails.append((tag, k, e))
    for k, v in _wanted_grads(ref).items():
        g = res[k]
        assert g.shape == v.shape, (tag, k)
        if ref["steady"] and k[5:] in C.PARAM_GRADS:
            # what cancelled terms leave (time_axis_cases.steady_window): the error against the terms' scale
            e = float(np.abs(g - v).max()) / ref["scale"]
            worst["steady"] = max(worst.get("steady", 0.0), e)
            if not e <= 1e-10:
                fails.append((tag, k, "steady", e))
            continue
        top = float(np.abs(v).max())
        en, ee = normrel(g, v), maxrel(g, v, floor=1e-30 * top) if top > 0 else float(np.abs(g).max())
        worst["norm"], worst["elem"] = max(worst["norm"], en), max(worst["elem"], ee)
        if not (en <= 1e-10 and ee <= 1e-6):
            fails.append((tag, k, en, ee))
        if T == 1 and k[5:] in C.PARAM_GRADS:
            assert np.all(g == 0.0) and np.all(v == 0.0), (tag, k)
    return fails


@pytest.mark.parametrize("T", T_S)
def test_fp64_kernel_matches_fp64_oracle(cuda, T):
    """Part 1.  Every mode, whole and cut; the backward runs at every T >= 1."""
    case = C.window_case("S", T)
    worst, fails = {"fwd": 0.0, "norm": 0.0, "elem": 0.0}, []
    for mode in C.MODES:
        inp = C.mode_inputs("S", T, mode)
        for part in C.S_PARTS:
            res = run(case, cuda, _graph("S", part), inp, dtype=torch.float64)
            ref = _mode_reference("S", T, mode, res["reaches"], np.float64)
            fails += _check_fp64(res, ref, T, (mode, part), worst)
    print(f"fp64 S T={T}: outputs max-rel {worst['fwd']:.2e}, gradients norm-rel {worst['norm']:.2e} "
          f"element-wise {worst['elem']:.2e}" + _steady_note(worst))
    assert not fails, "\n".join(map(str, fails))


# ---- 2: fp32 exact forward against the fp32 oracle, fp32 adjoints on that trajectory -----------------------

BAR_ADJOINT = {False: 5e-5, True: 1e-5}
EXACT_SHORT_T = 8  # kExactShortT (route_backward.h)


def _recipe_error(name, T, mode, reaches, ref, k):
    """Norm-relative distance of the reference recipe's fp32 adjoint (the oracle's sweep in fp32) from the fp64
    adjoint on the same fp32 trajectory: what an fp32 adjoint of this window can hold."""
    case, inp = C.window_case(name, T), C.mode_inputs(name, T, mode)
    own = _reference((name, T, mode, "fp32 adjoint"), reaches,
                     lambda: C.oracle_reference(case, inp, reaches, np.float32, adjoint_dtype=np.float32))
    return normrel(_wanted_grads(own)[k], _wanted_grads(ref)[k])


def _fp32_window(cuda, name, parts, modes, T):
    case = C.window_case(name, T)
    worst, fails, differ = {"fwd": 0.0, False: 0.0, True: 0.0}, [], 0
    for mode in modes:
        inp = C.mode_inputs(name, T, mode)
        for part in parts:
            pair = {}
            for exact_adjoint in (False, True):
                res = pair[exact_adjoint] = run(case, cuda, _graph(name, part), inp, exact_adjoint=exact_adjoint)
                if exact_adjoint and T <= EXACT_SHORT_T and inp["q0"] is None:
                    # a short hot-started window takes the exact adjoint's kernel by itself
                    _assert_bitwise(pair[False], pair[True], (mode, part, "short hot-started window"))
                ref = _mode_reference(name, T, mode, res["reaches"], np.float32)
                tag = (mode, part, "exact_adjoint" if exact_adjoint else "default")
                for k, e in _forward_errors(res, ref["fw"], T).items():
                    worst["fwd"] = max(worst["fwd"], e)
                    if not e <= 1e-6:
                        fails.append((tag, k, e))
                if not exact_adjoint:
                    differ += _differing(res, ref["fw"], T)
                for k, v in _wanted_grads(ref).items():
                    assert res[k].shape == v.shape, (tag, k)
                    bar = BAR_ADJOINT[exact_adjoint]
                    if ref["steady"] and k[5:] in C.PARAM_GRADS:
                        # what cancelled terms leave (time_axis_cases.steady_window): the error against the
                        # terms' scale, the same bar
                        e = float(np.abs(res[k] - v).max()) / ref["scale"]
                        worst["steady"] = max(worst.get("steady", 0.0), e)
                        if not e <= bar:
                            fails.append((tag, k, "steady", e))
                        continue
                    e = normrel(res[k], v)
                    worst[exact_adjoint] = max(worst[exact_adjoint], e)
                    if e > bar and name == "L":
                        # the larger of the project's bar and twice the reference recipe's own fp32 error here
                        own = _recipe_error(name, T, mode, res["reaches"], ref, k)
                        print(f"fp32 {name} T={T} {tag} {k}: {e:.2e} over the bar {bar:.0e}; the fp32 oracle adjoint "
                              f"is {own:.2e} from the fp64 one on the same trajectory")
                        bar = max(bar, 2.0 * own)
                    if not e <= bar:
                        fails.append((tag, k, e))
                    if T == 1 and k[5:] in C.PARAM_GRADS:
                        assert np.all(res[k] == 0.0), (tag, k)
    print(f"fp32 {name} T={T}: outputs max-rel {worst['fwd']:.2e} ({differ} values differ), gradients norm-rel "
          f"default {worst[False]:.2e} exact_adjoint {worst[True]:.2e}" + _steady_note(worst))
    assert not fails, "\n".join(map(str, fails))


@pytest.mark.parametrize("T", T_S)
def test_fp32_kernel_matches_fp32_oracle_small(cuda, T):
    """Part 2 on S, whole and cut, every mode."""
    _fp32_window(cuda, "S", tuple(C.S_PARTS), C.MODES, T)


@pytest.mark.parametrize("T", T_L256)
def test_fp32_kernel_matches_fp32_oracle_large(cuda, T):
    """Part 2 on L at one reach per thread (40 cut edges, storer and import waves): T_FLUSH and T_DEPTH of that
    partition.  Part 3 carries the agreement to two and four reaches per thread."""
    _fp32_window(cuda, "L", (256,), ("reach", "gauge", "carry", "state_carry"), T)


# ---- 3: one, two and four reaches per thread --------------------------------------------------------------

@pytest.mark.parametrize("math", ["exact", "faithful"])
@pytest.mark.parametrize("T", T_L)
def test_reaches_per_thread_are_bitwise_the_same(cuda, T, math):
    case = C.window_case("L", T)
    n = 0
    for mode in ("reach", "gauge", "carry", "state", "state_carry"):
        inp = C.mode_inputs("L", T, mode)
        runs = {cap: run(case, cuda, _graph("L", cap), inp, math=math) for cap in C.L_PARTS}
        for cap in (1536, 4096):
            n += _assert_bitwise(runs[cap], runs[256], (mode, cap))
    print(f"kr {math} T={T}: {n} arrays bitwise equal to one reach per thread")


# ---- 4: debug-flag twins at ragged T -----------------------------------------------------------------------

def _twin_windows():
    out = []
    for cap in C.L_PARTS:
        ts = {128, 129, 130, 131}
        for d in C.dmax_values(C.host_info("L", cap)):
            ts |= set(range(d + 2, d + 6))
        out += [(cap, t) for t in sorted(ts)]
    return out


@pytest.mark.parametrize("cap,T", _twin_windows())
def test_debug_flag_twins_at_ragged_windows(cuda, cap, T):
    case = C.window_case("L", T)
    g = _graph("L", cap)
    n = 0
    for mode in ("reach", "gauge", "carry", "state_carry"):
        inp = C.mode_inputs("L", T, mode)
        base = run(case, cuda, g, inp, math="faithful")
        for name, flag in FLAGS.items():
            n += _assert_bitwise(run(case, cuda, g, inp, math="faithful", flags=flag), base, (mode, name))
    print(f"twins cap={cap} T={T}: {n} arrays bitwise equal to the default kernels'")


# ---- 5: q' stores of several hours per row, the daily window ------------------------------------------------

@pytest.mark.parametrize("H,T", C.STORE_CASES)
def test_qprime_store_windows(cuda, H, T):
    """fp64 on S against the oracle on the repeated, filled, scaled hourly series, dL/dq' summed back per store
    row (the missing divide's column exactly zero); fp32 on L bitwise across one, two and four reaches per
    thread."""
    assert C.qs_rows_layout(T, H)
    case, inp = C.store_case("S", T, H)
    worst, fails = {"fwd": 0.0, "norm": 0.0, "elem": 0.0}, []
    for part in C.S_PARTS:
        res = run(case, cuda, _graph("S", part), inp, dtype=torch.float64)

        def make(reaches=res["reaches"]):
            ref = C.oracle_reference(case, inp, reaches, np.float64, qh=C.store_hourly(inp, T, np.float64))
            ref["qprime"] = C.store_grad(inp, ref["qprime"])
            return ref
        ref = _reference(("store", H, T), res["reaches"], make)
        assert res["grad_qprime"].shape == (-(-T // H), case.n)
        assert np.all(res["grad_qprime"][:, C.store_marks("S")[0]] == 0.0)
        fails += _check_fp64(res, ref, T, part, worst)
    caseL, inpL = C.store_case("L", T, H)
    runs = {cap: run(caseL, cuda, _graph("L", cap), inpL) for cap in C.L_PARTS}
    for cap in (1536, 4096):
        _assert_bitwise(runs[cap], runs[256], cap)
    print(f"store H={H} T={T}: fp64 outputs max-rel {worst['fwd']:.2e}, gradients norm-rel {worst['norm']:.2e} "
          f"element-wise {worst['elem']:.2e}" + _steady_note(worst))
    assert not fails, "\n".join(map(str, fails))


@pytest.mark.parametrize("T", C.DAILY_T)
def test_daily_window(cuda, T):
    """The fused daily series (G, D) of the training window against ``area_downsample`` of the oracle's gauge
    rows, gradients through the pooled output; fp32 on L bitwise across the partitions."""
    case, inp = C.window_case("S", T), C.daily_inputs("S", T)
    win = inp["window"]
    worst, fails = {"fwd": 0.0, "norm": 0.0, "elem": 0.0}, []
    for part in C.S_PARTS:
        res = run(case, cuda, _graph("S", part), inp, dtype=torch.float64)

        def make(reaches=res["reaches"]):
            ref = C.oracle_reference(case, inp, reaches, np.float64,
                                     grad_rows=C.daily_pool_vjp(inp["W"], win, T))
            ref["fw"] = dict(ref["fw"], runoff=C.daily_pool(ref["fw"]["runoff"], win))
            return ref
        ref = _reference(("daily", T), res["reaches"], make)
        assert res["runoff"].shape == (len(inp["gauges"]), win.D)
        fails += _check_fp64(res, ref, T, part, worst)
    caseL, inpL = C.window_case("L", T), C.daily_inputs("L", T)
    runs = {cap: run(caseL, cuda, _graph("L", cap), inpL) for cap in C.L_PARTS}
    for cap in (1536, 4096):
        _assert_bitwise(runs[cap], runs[256], cap)
    print(f"daily T={T} (L={win.L}, D={win.D}): fp64 outputs max-rel {worst['fwd']:.2e}, gradients norm-rel "
          f"{worst['norm']:.2e} element-wise {worst['elem']:.2e}")
    assert not fails, "\n".join(map(str, fails))


def test_daily_window_refuses_a_window_without_a_whole_day():
    with pytest.raises(ValueError):
        DailyWindow.for_training(C.DAILY_REFUSED_T)


# ---- 6: chained windows -------------------------------------------------------------------------------------

T_CHAIN = 140
NO_MODE = dict(gauges=None, q0=None, flow_scale=None, V=None, qprime_grad=False)


@functools.lru_cache(maxsize=None)
def _whole_window(dev, cap):
    return run(C.window_case("L", T_CHAIN), dev, _graph("L", cap), NO_MODE, grads=False)


@pytest.mark.parametrize("T1", [1, 2, 3, 4, 5, 127, 128, 129])
def test_chained_windows_are_bitwise_the_whole_window(cuda, T1):
    """A window of T steps equals its first T1 steps followed by a window of T - T1 + 1 steps that carries their
    final state and starts at q' row T1 - 1 (as route_timestep chains them; column 0 of the second window is the
    carried state): the t = 0 / t = 1 carried-state branches against the mid-window code, exact fp32 arithmetic,
    one, two and four reaches per thread."""
    import copy

    case = C.window_case("L", T_CHAIN)
    n = 0
    for cap in C.L_PARTS:
        g = _graph("L", cap)
        full = _whole_window(cuda, cap)
        a_case, b_case = copy.copy(case), copy.copy(case)
        a_case.qprime, b_case.qprime = case.qprime[:T1], case.qprime[T1 - 1:]
        a = run(a_case, cuda, g, NO_MODE, grads=False)
        b = run(b_case, cuda, g, dict(NO_MODE, q0=a["q_last"]), grads=False)
        assert np.array_equal(a["runoff"], full["runoff"][:, :T1]), cap
        assert np.array_equal(b["runoff"], full["runoff"][:, T1 - 1:]), cap
        for k in ("q_last", "top_width", "side_slope"):
            assert np.array_equal(b[k], full[k]), (cap, k)
        n += 5
    print(f"chain T1={T1} of {T_CHAIN}: {n} arrays bitwise equal to the whole window's")
