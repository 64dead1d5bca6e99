"""The cases of tests/test_gpu_time_axis.py, on the CPU: the networks and partitions, the window lengths, the
modes and their oracle references (``oracle/mc_oracle.py`` only).

The fused routing kernels branch on the window length T: rows of four steps (``(T & 3) == 0``: 16-byte runoff
stores and dL/drunoff loads, the plain kernel instances; a reach's first gradient group at ``T - 4`` or at
``(T - 1) & ~3``), the fp32 gradient partials' flush every 128 steps, the cut-edge imports in chunks of 4
(forward) and 8 (backward) ticks over ``TT = T + dmax`` ticks, the steady tick range ``[s0, s1)`` that is empty
below ``T ~ dmax``, the last two steps the state seeds and the reported geometry read, the rows of a q' store of
several hours, and the daily objective's window.  The lists here put a window length on each side of every one
of those edges; tests/test_time_axis_cases.py asserts that they do.

Networks
  S  ``random_binary_tree(300, 6)``: one block of depth 16 (``WHOLE``, no cut edge) and ten blocks of depth <= 15
     with nine cut edges (``CUT``) -- both parities of ``dmax + 1``, so the steady range's lower bound is rounded
     up in one partition and not in the other.
  L  ``forest(loguniform_sizes(3, 100, 2500, 7), seed=7)``: 3758 reaches in basins of 748, 1796 and 1214, 109
     deep.  ``L_PARTS``: block cap 256 (one reach per thread, 40 cut edges, blocks <= 46 deep), 1536 (two per
     thread, five cut edges) and 4096 (four per thread, one block).

``dmax`` is read from the built graph: the deepest block (``max_block_depth``, the ``B.dmax`` of the kernels'
``TT``) and the network's depth (``max_depth``); ``t_depth`` takes both where they differ.
"""

from __future__ import annotations

import functools

import numpy as np

from conftest import PARAMS_DEFAULT, synthetic_case
from ddr_amd import synthetic
from ddr_amd.graph import RiverGraph
from oracle import mc_oracle as O

S_SEED, L_SEED = 6, 7
WHOLE = {"target_blocks": 1}
CUT = {"max_block_reaches": 64, "target_blocks": 1 << 20}
S_PARTS = {"whole": WHOLE, "cut": CUT}
L_PARTS = {cap: {"max_block_reaches": cap, "target_blocks": 1} for cap in (256, 1536, 4096)}
L_KR = {256: 1, 1536: 2, 4096: 4}

T_SMALL = tuple(range(1, 18))
T_FLUSH = tuple(range(125, 134)) + tuple(range(253, 260))
GRAD_FLUSH, CHUNK_FWD, CHUNK_BWD = 128, 4, 8  # kGradFlush, kChunkFwd, kChunkBwd (internal.h)

# window lengths of the q' stores of H hours per row and of the daily objective's window
STORE_T = {24: (1, 2, 23, 24, 25, 26, 47, 48, 49, 50, 73),
           **{H: (1, H, H + 1, H + 2, 2 * H, 2 * H + 1, 5 * H + 3) for H in (2, 3, 7)}}
STORE_CASES = [(H, T) for H in (24, 2, 3, 7) for T in STORE_T[H]]
DAILY_T = (45, 46, 47, 68, 69, 70, 93, 116)
DAILY_REFUSED_T = 44

MODES = ("reach", "gauge", "carry", "state", "state_carry", "seed")
OUTPUTS = ("runoff", "q_last", "top_width", "side_slope")
PARAM_GRADS = ("n", "q_spatial", "p_spatial")


@functools.lru_cache(maxsize=None)
def network(name):
    if name == "S":
        return synthetic.random_binary_tree(300, S_SEED)
    return synthetic.forest(synthetic.loguniform_sizes(3, 100, 2500, L_SEED), seed=L_SEED)


def partition(name, part):
    return (S_PARTS if name == "S" else L_PARTS)[part]


@functools.lru_cache(maxsize=None)
def host_info(name, part):
    """GraphInfo of a partition, from a host-only build (no device)."""
    net = network(name)
    return RiverGraph(net.n, net.rows, net.cols, host_only=True, **partition(name, part)).info


def dmax_values(info):
    return sorted({int(info.max_block_depth), int(info.max_depth)})


def t_depth(info):
    """dmax - 1 ... dmax + 6 for the deepest block and for the whole network."""
    return tuple(sorted({t for d in dmax_values(info) for t in range(d - 1, d + 7) if t >= 1}))


def t_sweep(name, parts):
    """T_SMALL, T_FLUSH and T_DEPTH of every partition given, sorted."""
    ts = set(T_SMALL) | set(T_FLUSH)
    for p in parts:
        ts |= set(t_depth(host_info(name, p)))
    return tuple(sorted(ts))


def steady_range(T, dmax):
    """The forward's steady ticks [s0, s1) (route_forward.hip): both bounds even, none when s1 <= s0."""
    s0 = dmax + 1
    s0 += s0 & 1
    return s0, T & ~1


def flushes(T):
    """How often the backward's sweep t = T - 1 ... 1 meets ``t % kGradFlush == 1``."""
    return sum(1 for t in range(1, T) if t % GRAD_FLUSH == 1)


def qs_rows_layout(T, H):
    """``choose_qs_layout`` (route_args.h): the row layout of a store of H > 1 hours per row is taken when the
    magic division by H is exact over the window."""
    if H <= 1 or T < 1:
        return False
    m = ((1 << 32) + H - 1) // H
    err = m * H - (1 << 32)
    return not (err > 0 and T * err >= (1 << 32) // H)


# ---- cases ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def window_case(name, T):
    """Read-only: shared by the tests of a window."""
    return synthetic_case(network(name), T, S_SEED if name == "S" else L_SEED, PARAMS_DEFAULT)


def gauge_sets(n, seed):
    """Gauges of one reach, of several reaches, two sharing a reach, one given by a negative index, the outlet
    (reach n - 1) in two of them: reaches with exactly one gauge (the backward's register path), with several
    (its list walk) and with none."""
    rng = np.random.default_rng(seed + 500)
    pick = rng.choice(n - 1, 12, replace=False).astype(np.int64)
    return [pick[:1], pick[1:5], pick[[5, 6]], pick[[6, 7]], np.array([-1]), np.array([int(pick[8]) - n, n - 1]),
            pick[9:12]]


@functools.lru_cache(maxsize=None)
def mode_inputs(name, T, mode):
    """What a mode adds to the plain window (read-only): dict(gauges, q0, flow_scale, V, qprime_grad, W)."""
    n = network(name).n
    rng = np.random.default_rng(1000 * T + MODES.index(mode) + (0 if name == "S" else 50))
    d = dict(gauges=None, q0=None, flow_scale=None, V=None, qprime_grad=False)
    if mode == "gauge":
        d["gauges"] = gauge_sets(n, T)
    if mode in ("carry", "state_carry"):
        q0 = rng.uniform(0.5, 5.0, n).astype(np.float32)
        q0[11] = 5e-5  # below q_lb: enters step 1 unclamped
        d["q0"] = q0
    if mode in ("state", "state_carry"):
        d["flow_scale"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
        d["qprime_grad"] = True
    if mode == "seed":
        d["V"] = rng.uniform(-1.0, 1.0, (3, n)).astype(np.float32)
    rows = len(d["gauges"]) if d["gauges"] is not None else n
    d["W"] = rng.uniform(0.0, 1.0, (rows, T)).astype(np.float32)
    return d


def routed_qprime(case, inp, dtype):
    """The series the kernel routes: q' times flow_scale, one multiplication in the kernel's precision."""
    qp = np.asarray(case.qprime, dtype)
    if inp["flow_scale"] is not None:
        qp = (qp * inp["flow_scale"].astype(dtype)[None, :]).astype(dtype)
    return qp


def unit_grads(case, gn, gq, gp):
    u64 = {k: v.astype(np.float64) for k, v in case.u.items()}
    return O.param_grads_from_unit(gn, gq, gp, u64["n"], u64["q_spatial"], u64["p_spatial"],
                                   case.params["parameter_ranges"])


def steady_window(inp, qh):
    """A hot-started window whose steps all read the same q' row (T = 2 always; a store window within its first
    row) stays in the hot start's own steady state: x(t) = Q0 whatever the parameters (c1 + c2 = c4 and
    c1 + c2 + c3 = 1), so every parameter gradient of the routing is zero in exact arithmetic and a rounding
    residue of cancelled terms in floating point -- on the oracle's side too (measured 5e-17 of
    ``gradient_scale``).  Where a q' of that row lies below q_lb the hot start (which takes it unclamped) is just
    off the steady state of the steps (which clamp it) and the gradient is what those cancelled terms leave,
    1e-6 to 1e-5 of their scale.  A relative error against such a remainder measures the cancellation, not the
    kernel: these gradients are held to the comparison's bar in max |g - reference| over ``gradient_scale``."""
    return inp["q0"] is None and qh.shape[0] >= 2 and bool(np.all(qh[:-1] == qh[0]))


def gradient_scale(inp, fw):
    """The size of one reach-step's term of a parameter gradient, dL/dQ times Q times a sensitivity of order
    one: max |W| max |Q|.  A rounding residue is ~1e-16 (fp64) or ~1e-7 (fp32) of a few such terms."""
    return float(np.abs(inp["W"]).max()) * float(np.abs(fw["runoff"]).max())


def oracle_reference(case, inp, reaches, dtype, grads=True, qh=None, grad_rows=None, adjoint_dtype=np.float64):
    """The oracle's forward in ``dtype`` from the physical inputs the kernel saw and the fp64 adjoint on that
    trajectory: dict(fw, grads: name -> (N,) u gradients, and with ``qprime_grad`` qprime (T, N) -- w.r.t. q', or
    w.r.t. the routed series when ``qh`` is given -- and q0 (carried windows)).
    ``qh``: the routed hourly series when it is not ``routed_qprime`` (a store); ``grad_rows``: dL/d(hourly
    output rows) when the loss is not ``W`` on them (the daily window); ``adjoint_dtype`` = float32: the
    reference recipe's own fp32 adjoint (``route_backward``), a measure and not a checker."""
    net, bd = case.network(), case.bounds
    own_series = qh is not None
    qh = qh if own_series else routed_qprime(case, inp, dtype)
    T = qh.shape[0]
    q0 = None if inp["q0"] is None else inp["q0"].astype(dtype)
    fw = O.route(net, reaches, qh, bd, q0=q0, dtype=dtype, outflow_idx=inp["gauges"])
    ref = {"fw": fw, "steady": inp["V"] is None and steady_window(inp, qh), "scale": gradient_scale(inp, fw)}
    if not grads:
        return ref
    r64 = reaches.astype(np.float64)
    seed, extra = None, (0.0, 0.0, 0.0)
    if inp["V"] is not None:
        V = inp["V"]
        gQ = np.zeros(net.n)
        if T >= 2:  # the reported geometry is that of Q_{T-2}; a one-step window reports none
            Qp = np.maximum(fw["x"][T - 2].astype(np.float64), bd.discharge)
            gQ, *extra = O.geometry_vjp(Qp, r64.n, r64.q, r64.p, r64.slope, bd, V[1], V[2])
        seed = np.stack([V[0], gQ])
    G = np.asarray(inp["W"], np.float64) if grad_rows is None else grad_rows
    bw = O.route_backward(net, reaches, qh, fw["x"], G, bd, outflow_idx=inp["gauges"],
                          want_qprime=inp["qprime_grad"], carry=q0 is not None, state_seed=seed,
                          dtype=adjoint_dtype)
    ref["grads"] = unit_grads(case, bw["n"] + extra[0], bw["q_spatial"] + extra[1], bw["p_spatial"] + extra[2])
    if inp["qprime_grad"]:
        ref["qprime"], ref["q0"] = bw["qprime"], bw["q0"]
        if not own_series and inp["flow_scale"] is not None:
            ref["qprime"] = bw["qprime"] * inp["flow_scale"].astype(np.float64)[None, :]
    return ref


# ---- a q' store of H hours per row ---------------------------------------------------------------------


def store_marks(name):
    """(the divide missing from the store, the divide whose first two rows are below the clamp): reaches with
    inflow from upstream.  A headwater fed a constant stays in the steady state x = (c3 + c4) q' = q', whose
    parameter gradient is zero in exact arithmetic and a rounding residue of cancelled terms in floating point
    (tests/test_gpu_clamps.py, the dry steady headwaters): no element-wise comparison could hold there."""
    net = network(name)
    inner = np.flatnonzero(np.bincount(net.rows, minlength=net.n) > 0)
    return int(inner[3]), int(inner[1])


@functools.lru_cache(maxsize=None)
def store_case(name, T, H):
    """A window of T steps over a store of ceil(T / H) rows, one divide missing from the store (the reader's
    0.001 fill), flow_scale, dL/dq' wanted (read-only): the window case and the mode's inputs."""
    net = network(name)
    case = window_case(name, T)
    rows = -(-T // H)
    rng = np.random.default_rng(7000 + 100 * H + T)
    store = synthetic.lateral_inflow(net.n, rows, 32 + H).astype(np.float32)
    missing, low = store_marks(name)
    store[:2, low] = 1e-6  # below the clamp
    valid = np.ones(net.n, np.uint8)
    valid[missing] = 0
    inp = dict(gauges=None, q0=None, V=None, qprime_grad=True, store=store, valid=valid, hours=H,
               flow_scale=rng.uniform(0.5, 1.5, net.n).astype(np.float32),
               W=rng.uniform(0.0, 1.0, (net.n, T)).astype(np.float32))
    return case, inp


def store_hourly(inp, T, dtype):
    """The hourly series a store window routes: rows repeated, the missing divide filled, scaled."""
    qh = np.repeat(inp["store"].astype(dtype), inp["hours"], axis=0)[:T]
    qh[:, inp["valid"] == 0] = dtype(np.float32(0.001))  # the reader's fill is a float32 0.001
    return (qh * inp["flow_scale"].astype(dtype)[None, :]).astype(dtype)


def store_grad(inp, g_hourly):
    """dL/d(store) from the gradient w.r.t. the routed hourly series: scaled, the fill a constant, summed per
    row (row 0 also takes step 0's, the hot start's)."""
    gh = g_hourly * inp["flow_scale"].astype(np.float64)[None, :]
    gh[:, inp["valid"] == 0] = 0.0
    out = np.zeros(inp["store"].shape)
    for t in range(gh.shape[0]):
        out[t // inp["hours"]] += gh[t]
    return out


# ---- the daily objective's window ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def daily_inputs(name, T):
    """Gauge mode with the training window of T hours (read-only); W is dL/d(daily series), (G, D)."""
    from ddr_amd.ops import DailyWindow

    win = DailyWindow.for_training(T)
    n = network(name).n
    rng = np.random.default_rng(9000 + T)
    gauges = gauge_sets(n, T)
    return dict(gauges=gauges, q0=None, flow_scale=None, V=None, qprime_grad=False, window=win,
                W=rng.uniform(0.0, 1.0, (len(gauges), win.D)).astype(np.float32))


def daily_pool(rows, win):
    """``area_downsample`` of hours [t0, t0 + L) of the (G, T) gauge rows."""
    return O.area_downsample(np.ascontiguousarray(rows[:, win.t0:win.t0 + win.L]), win.D)


def daily_pool_vjp(gd, win, T):
    """dL/d(hourly gauge rows) (G, T) from dL/d(daily series) (G, D): the pooling's adjoint."""
    gd = np.asarray(gd, np.float64)
    gh = np.zeros((gd.shape[0], T))
    for d in range(win.D):
        a, b = (d * win.L) // win.D, ((d + 1) * win.L + win.D - 1) // win.D
        gh[:, win.t0 + a:win.t0 + b] += gd[:, d:d + 1] / (b - a)
    return gh
