"""The one-step physics over the parameter box the configuration allows: the points, graphs and CPU-side
references shared by tests/test_physics_box.py (CPU) and tests/test_gpu_physics_box.py (device).

ddr_amd/csrc/physics.h is reached by the rest of the suite only along trajectories from
``synthetic.unit_parameters``.  Here every reach is one point of the box

    n ~ U[0.015, 0.25]   q_spatial ~ U[0, 1]   p log-uniform [1 + 1e-6, 200]   slope log-uniform [1e-4, 1]
    length log-uniform [10^1.5, 10^4.7]   X ~ U[0, 0.5]   Q log-uniform [1e-4, 10^5.5]   q' log-uniform [1e-6, 1e4]

and a carried two-step window (``route(..., q0=Q, steps=2)``) evaluates the physics once per reach: ``top_width``
and ``side_slope`` are the geometry at Q itself, ``runoff[:, 1]`` is max(x1, q_lb) with x1 = c1 Sx + c2 I + c3 Q +
c4 max(q', q_lb), and the backward is that step's VJP.  Two graphs over the same points: every reach isolated
(Sx = I = 0), and N / 2 chains 2i -> 2i + 1 (the downstream reach adds c1, c2 and the adjoint's Sx and I terms).

The N = 60 000 sampled points are float32 (the fp64 references read the same values); the last ``n_edge`` of them
are moved onto the edge planes, ``PLANE`` points each (``Box.planes``: name -> slice), by replacing one coordinate:

    q = 0, q = 1, p / n / slope at either end, X = 0, X = 0.5, Q = q_lb exactly
    ratio_k   Q solved (bisection over the float32 bit patterns: every operation is monotone in Q) so that the fp32
              ``ratio`` is 2^j + k ulp, k in -2 .. 2, 2^j the power of two nearest the drawn point's ratio, on every
              fifth candidate j = 0 (ratio = 1): the table-index and exponent boundaries of ``ln_tab``
    pw_k      Q solved the same way so that the fp32 ``pw`` is depth_lb + k ulp, k in -1 .. 1: the branch
              ``pw >= dlb`` of ``coefficients_np`` at equality

A solve can miss (the rounded map Q -> ratio skips values) or leave the box, so the solved planes are filled by
rejection: fresh points are drawn from the same generator until PLANE of them land on the target exactly with Q
inside the box.  The points depend on the parameter set only through its bounds (q_lb, depth_lb): ``box(pname)``.

Masks (``Reference``), per point, a chain masked as a unit:
  tie    some pow of the point (ratio^expo, depth^qe, Rh^(2/3)) has its fp64 value within 64 units of the last
         place of an fp32 rounding midpoint, |low 29 mantissa bits - 2^28| <= 64, 2^-46 relative: ~50 times the
         error fastmath.h states for pow_pos, inside which the kernel may round the other way than numpy's pow
  near   some clamped quantity (pw, ss_raw, bw_raw, v, x1) within 1e-4 relative of its bound, in the fp32 or the
         fp64 evaluation (``NEAR_GRAD`` of test_clamp_cases.py): a gradient mask may differ there
"""

from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from conftest import PARAMS_DEFAULT, PARAMS_MOCK
from oracle import mc_oracle as O

N = 60_000
SEED = 1
PLANE = 500        # points per plain edge plane (even: chains stay inside a plane)
NEAR = 1e-4        # test_clamp_cases.NEAR_GRAD
TIE = 64           # half-width of the pow-tie window in units of the fp64 value's last place
PARAMS = {"default": PARAMS_DEFAULT, "mock": PARAMS_MOCK}
GRAPHS = ("isolated", "chains")
DT = 3600.0
f32 = np.float32
RANGES = {"n": (0.015, 0.25), "q": (0.0, 1.0), "p": (1.0 + 1e-6, 200.0), "slope": (1e-4, 1.0),
          "length": (10 ** 1.5, 10 ** 4.7), "X": (0.0, 0.5), "Q": (1e-4, 10 ** 5.5), "qp": (1e-6, 1e4)}
LOG = ("p", "slope", "length", "Q", "qp")
FIELDS = tuple(RANGES)
QUANTILES = (0.5, 0.9, 0.99, 0.999)


def bounds_of(pname: str) -> O.Bounds:
    m = PARAMS[pname]["attribute_minimums"]
    return O.Bounds(discharge=m["discharge"], velocity=m["velocity"], depth=m["depth"], bottom_width=m["bottom_width"])


def sample(rng, count: int) -> dict:
    """``count`` points of the box, float32, clipped to the float32 images of its ends."""
    out = {}
    for k in FIELDS:
        lo, hi = RANGES[k]
        v = np.exp(rng.uniform(np.log(lo), np.log(hi), count)) if k in LOG else rng.uniform(lo, hi, count)
        out[k] = np.clip(v.astype(f32), f32(lo), f32(hi))
    return out


def _geom32(pt, Q, bd):
    return O.trapezoid_celerity(Q, pt["n"], pt["q"], pt["p"], pt["slope"], bd, f32, full=True)


def solve_q(fn, target, lo, hi):
    """Per element the smallest float32 Q in [lo, hi] with fn(Q) >= target (fn monotone non-decreasing in Q,
    element-wise): bisection over the bit patterns, which order the positive floats."""
    a, b = lo.astype(f32).view(np.int32).astype(np.int64), hi.astype(f32).view(np.int32).astype(np.int64)
    while np.any(a < b):
        mid = (a + b) // 2
        ge = fn(mid.astype(np.int32).view(f32)) >= target
        b = np.where(ge, mid, b)
        a = np.where(ge, a, mid + 1)
    return a.astype(np.int32).view(f32)


def _ulps(x, k):
    """x moved by k units of its last place (float32, positive normal)."""
    return (x.astype(f32).view(np.int32) + np.int32(k)).view(f32)


@functools.lru_cache(maxsize=None)
def box(pname: str):
    """The points of one parameter set (read-only): fields of FIELDS as (N,) float32, ``planes`` name -> slice,
    ``n_edge``, ``interior`` (the slice of the points no plane moved), ``bounds``."""
    bd = bounds_of(pname)
    rng = np.random.default_rng(SEED)
    pt = sample(rng, N)
    plain = [("q0", "q", 0.0), ("q1", "q", 1.0), ("p_lo", "p", RANGES["p"][0]), ("p_hi", "p", RANGES["p"][1]),
             ("n_lo", "n", RANGES["n"][0]), ("n_hi", "n", RANGES["n"][1]), ("slope_lo", "slope", RANGES["slope"][0]),
             ("slope_hi", "slope", RANGES["slope"][1]), ("X0", "X", 0.0), ("X_half", "X", 0.5),
             ("Q_qlb", "Q", bd.discharge)]
    solved = [f"ratio_{k:+d}" for k in range(-2, 3)] + [f"pw_{k:+d}" for k in range(-1, 2)]
    n_edge = PLANE * (len(plain) + len(solved))
    planes, at = {}, N - n_edge
    for name, key, val in plain:
        planes[name] = slice(at, at + PLANE)
        pt[key][planes[name]] = f32(val)
        at += PLANE
    qlo, qhi = f32(RANGES["Q"][0]), f32(RANGES["Q"][1])
    for name in solved:
        sl = planes[name] = slice(at, at + PLANE)
        at += PLANE
        k, M = int(name.split("_")[1]), 4 * PLANE
        sub, filled = {key: np.empty(PLANE, f32) for key in FIELDS}, 0
        while filled < PLANE:
            c = sample(rng, M)
            if name.startswith("ratio"):
                r0 = _geom32(c, c["Q"], bd)["ratio"].astype(np.float64)
                j = np.rint(np.log2(r0))
                j[::5] = 0.0
                target = _ulps(np.exp2(j).astype(f32), k)
                fn = lambda Q, c=c: _geom32(c, Q, bd)["ratio"]  # noqa: E731
                # ratio is proportional to Q: the target lies within a factor 2 of this Q's ratio
                guess = c["Q"].astype(np.float64) * target / r0
                lo, hi = (guess / 2).astype(f32), (guess * 2).astype(f32)
            else:
                target = np.full(M, _ulps(np.full(1, f32(bd.depth)), k)[0])
                fn = lambda Q, c=c: _geom32(c, Q, bd)["pw"]  # noqa: E731
                lo, hi = np.full(M, qlo / f32(2)), np.full(M, qhi)
            Q = solve_q(fn, target, lo, hi)
            take = np.flatnonzero((fn(Q) == target) & (Q >= qlo) & (Q <= qhi))[: PLANE - filled]
            c["Q"] = Q
            for key in FIELDS:
                sub[key][filled:filled + len(take)] = c[key][take]
            filled += len(take)
        for key in FIELDS:
            pt[key][sl] = sub[key]
    assert at == N
    for v in pt.values():
        v.setflags(write=False)
    return SimpleNamespace(**pt, planes=planes, n_edge=n_edge, interior=slice(0, N - n_edge), bounds=bd,
                           pname=pname)


@functools.lru_cache(maxsize=None)
def coo(graph: str):
    """(rows, cols) of the graph: rows[k] is the reach downstream of cols[k]."""
    if graph == "isolated":
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    up = np.arange(0, N, 2, dtype=np.int64)
    return up + 1, up


@functools.lru_cache(maxsize=None)
def network(graph: str) -> O.Network:
    rows, cols = coo(graph)
    return O.Network.from_coo(N, rows, cols)


def as_unit(mask, graph: str):
    """A per-point mask widened to the units that are compared together: on the chains a pair 2i, 2i + 1."""
    if graph == "isolated":
        return mask
    return np.repeat(mask[0::2] | mask[1::2], 2)


def reaches(b, dtype=f32) -> O.Reaches:
    return O.Reaches(*(np.asarray(getattr(b, k), dtype) for k in ("n", "q", "p", "length", "slope", "X")))


def qprime_rows(b, dtype=f32):
    """(2, N): row 0 feeds the step, row 1 feeds nothing."""
    return np.stack([b.qp, b.qp]).astype(dtype)


@functools.lru_cache(maxsize=None)
def weights():
    """Random signed weights of the loss sum(w * runoff[:, 1]), float32."""
    rng = np.random.default_rng(SEED + 1)
    return (rng.uniform(0.25, 1.0, N) * rng.choice([-1.0, 1.0], N)).astype(f32)


def pow_values(d):
    """The three pows of the physics in fp64, from the fp32 oracle's intermediates ``d`` (numpy's fp64 pow of
    the fp32 operands: what the fp32 oracle rounds once more)."""
    w = lambda a: np.asarray(a, np.float64)  # noqa: E731
    return (np.power(w(d["ratio"]), w(d["expo"])), np.power(w(d["depth"]), w(d["qe"])),
            np.power(w(d["R"]), w(f32(2.0 / 3.0))))


def pow_tie(d):
    """(N,) bool: some pow's fp64 value is within TIE units of its last place of an fp32 rounding midpoint."""
    m = np.zeros(np.shape(d["ratio"]), bool)
    for v in pow_values(d):
        low = v.view(np.int64) & ((1 << 29) - 1)
        m |= np.abs(low - (1 << 28)) <= TIE
    return m


def near_bound(d, x1, bd, dtype, tol=NEAR):
    m = np.zeros(np.shape(d["pw"]), bool)
    f = dtype
    for v, bnd in ((d["pw"], bd.depth), (d["ss_raw"], bd.side_slope_min), (d["ss_raw"], bd.side_slope_max),
                   (d["bw_raw"], bd.bottom_width), (d["v"], bd.velocity), (d["v"], bd.velocity_max),
                   (x1, bd.discharge)):
        m |= np.abs(np.asarray(v, np.float64) - float(f(bnd))) <= tol * float(f(bnd))
    return m


def one_step(b, graph, dtype):
    """The oracle's carried two-step window with the step's intermediates: dict(fw = ``O.route``'s result, d =
    ``trapezoid_celerity(full=True)`` at Q, c1..c4, x1 (unclamped), qc, Sx, I, scale = |Q| + |q'c| + |Sx| + |I|)."""
    net, bd, r = network(graph), b.bounds, reaches(b, dtype)
    Q = np.asarray(b.Q, dtype)
    fw = O.route(net, r, qprime_rows(b, dtype), bd, q0=Q, dtype=dtype)
    d = O.trapezoid_celerity(Q, r.n, r.q, r.p, r.slope, bd, dtype, full=True)
    c1, c2, c3, c4 = O.muskingum_coefficients(r.length, d["c"], r.x, DT, dtype)
    x1 = fw["x"][1]
    qc = np.maximum(np.asarray(b.qp, dtype), dtype(bd.discharge))
    Sx, I = net.spmv(x1), net.spmv(Q)
    scale = np.abs(Q.astype(np.float64)) + np.abs(qc) + np.abs(Sx) + np.abs(I)
    return dict(fw=fw, d=d, c1=c1, c2=c2, c3=c3, c4=c4, x1=x1, qc=qc, Sx=Sx, I=I, scale=scale.astype(np.float64))


def vjp(b, graph, xs):
    """The fp64 oracle adjoint of the loss on the states ``xs`` ((2, N): Q and the unclamped x1): n, q_spatial,
    p_spatial, q0 and qprime (row 0), each (N,)."""
    G = np.zeros((N, 2))
    G[:, 1] = weights()
    bw = O.route_backward(network(graph), reaches(b, np.float64), qprime_rows(b, np.float64), xs, G, b.bounds,
                          want_qprime=True, carry=True)
    return {"n": bw["n"], "q_spatial": bw["q_spatial"], "p_spatial": bw["p_spatial"], "q0": bw["q0"],
            "qprime": bw["qprime"][0]}


def torch_step(b, graph, dtype="float32", grads=True):
    """T: the same step in PyTorch on the CPU, ``compute_trapezoidal_geometry`` plus the Muskingum formulas
    (mmc.py:165-167, 479-484, 535-557), differentiated by autograd.  Returns numpy arrays: x1 (unclamped), runoff1,
    top_width, side_slope and, with ``grads``, the gradients of sum(w * runoff1) under ``vjp``'s names."""
    import torch

    from ddr_amd.geometry.trapezoidal import compute_trapezoidal_geometry

    bd, td = b.bounds, getattr(torch, dtype)
    t = {k: torch.tensor(np.asarray(getattr(b, k)), dtype=td, requires_grad=grads and k in ("n", "q", "p", "Q", "qp"))
         for k in FIELDS}
    geo = compute_trapezoidal_geometry(t["n"], t["p"], t["q"], t["Q"], t["slope"], depth_lb=bd.depth,
                                       bottom_width_lb=bd.bottom_width, side_slope_lb=bd.side_slope_min,
                                       side_slope_ub=bd.side_slope_max)
    cel = torch.clamp(geo["velocity"], min=bd.velocity, max=bd.velocity_max) * 5 / 3
    twok = 2.0 * (t["length"] / cel)
    X = t["X"]
    den = twok * (1.0 - X) + DT
    c1, c2 = (DT - twok * X) / den, (DT + twok * X) / den
    c3, c4 = (twok * (1.0 - X) - DT) / den, (2.0 * DT) / den
    qc = torch.clamp(t["qp"], min=bd.discharge)
    b0 = c3 * t["Q"] + c4 * qc
    if graph == "chains":
        x_up = b0[0::2]
        x_dn = (c2[1::2] * t["Q"][0::2] + b0[1::2]) + c1[1::2] * x_up
        x1 = torch.stack([x_up, x_dn], dim=1).reshape(-1)
    else:
        x1 = b0
    run1 = torch.clamp(x1, min=bd.discharge)
    out = {"x1": x1, "runoff1": run1, "top_width": geo["top_width"], "side_slope": geo["side_slope"]}
    if grads:
        g = torch.autograd.grad((run1 * torch.tensor(weights(), dtype=td)).sum(),
                                [t[k] for k in ("n", "q", "p", "Q", "qp")])
        out.update(dict(zip(("n", "q_spatial", "p_spatial", "q0", "qprime"), g)))
    return {k: v.detach().numpy() for k, v in out.items()}


class Reference:
    """Everything the comparisons of one (parameter set, graph) need, computed once on the CPU and read only."""

    def __init__(self, pname, graph):
        self.pname, self.graph = pname, graph
        self.box = b = box(pname)
        self.s32 = one_step(b, graph, f32)
        self.s64 = one_step(b, graph, np.float64)
        bd = b.bounds
        self.tie = as_unit(pow_tie(self.s32["d"]), graph)
        self.near = as_unit(near_bound(self.s32["d"], self.s32["x1"], bd, f32)
                            | near_bound(self.s64["d"], self.s64["x1"], bd, np.float64), graph)

    @functools.cached_property
    def vjp32(self):
        """fp64 adjoint of the fp32 inputs on the fp32 oracle's states: what the fp32 adjoints are compared with."""
        return vjp(self.box, self.graph, self.s32["fw"]["x"])

    @functools.cached_property
    def vjp64(self):
        return vjp(self.box, self.graph, self.s64["fw"]["x"])

    @functools.cached_property
    def t32(self):
        return torch_step(self.box, self.graph, "float32")

    @functools.cached_property
    def t_quantiles(self):
        """name -> T's per-element relative gradient error against ``vjp32`` at QUANTILES."""
        return {k: rel_quantiles(self.t32[k], self.vjp32[k], ~self.near) for k in self.vjp32}

    def census(self):
        """Share of the points at which each clamp is active and each coefficient negative (fp32 evaluation)."""
        d, bd, s = self.s32["d"], self.box.bounds, self.s32
        f = f32
        return {"depth": np.mean(d["pw"] < f(bd.depth)), "ss_low": np.mean(d["ss_raw"] < f(bd.side_slope_min)),
                "ss_high": np.mean(d["ss_raw"] > f(bd.side_slope_max)), "bw": np.mean(d["bw_raw"] < f(bd.bottom_width)),
                "v_low": np.mean(d["v"] < f(bd.velocity)), "v_high": np.mean(d["v"] > f(bd.velocity_max)),
                "x_low": np.mean(s["x1"] < f(bd.discharge)), "qp_low": np.mean(self.box.qp < f(bd.discharge)),
                "c1_neg": np.mean(s["c1"] < 0), "c3_neg": np.mean(s["c3"] < 0)}


@functools.lru_cache(maxsize=None)
def reference(pname: str, graph: str) -> Reference:
    return Reference(pname, graph)


def rel_quantiles(g, ref, keep, qs=QUANTILES):
    """Quantiles of |g - ref| / |ref| over the kept elements with ref != 0."""
    g, ref = np.asarray(g, np.float64), np.asarray(ref, np.float64)
    sel = keep & (ref != 0.0)
    return np.quantile(np.abs(g[sel] - ref[sel]) / np.abs(ref[sel]), qs)


def ulp_distance(a, b):
    """Units in the last place between two float32 arrays of one sign (bit-pattern difference)."""
    return np.abs(np.asarray(a, f32).view(np.int32).astype(np.int64) - np.asarray(b, f32).view(np.int32).astype(np.int64))
