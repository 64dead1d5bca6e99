"""References of the linear routing's adjoint (tests/test_linear_adjoint_model.py, on the CPU).  The package has no
device adjoint yet (the linear section's "Not implemented"); these fix what one must compute.  The
closed-form coefficient derivatives the parameter gradients need are the package's
(``ddr_amd.routing.muskingum_coefficient_gradients``).

Two references:

* :func:`adjoint`: the reverse sweep of the linear routing (route_linear.hip's transposed recurrence) in NumPy, in
  fp32 or fp64, with a fixed operation order in which every sum has one owner and an order given by the graph and
  the time axis alone: a device adjoint written in that order can be held to it bit for bit, as the forward is held
  to tests/linear_cases.py.
* :func:`torch_route`: the *forward* restated in torch as one dense linear solve per sub-step; its fp64 autograd is
  the independent reference of :func:`adjoint`.

The operation order (R the routed dtype, every operation rounded separately; ``d`` the downstream reach,
an outlet adds an exact zero; ``f = (s - 1) // S`` the interval of sub-step ``s``)::

    lam = (gout[:, F - 1] if end else 0) + glast
    for s = F S .. 1, downstream reaches first:
        mu   = lam + a[d]                       a, b of the downstream reach at the same s
        a, b = C1 mu, C2 mu
        acc  = acc + float64(a + b)             fp64 over the interval; gqe[f] = R(acc) after its first sub-step
        g1   = g1 + float64(mu) float64(In^s + qe[f])          fp64, each accumulator in descending s
        g2   = g2 + float64(mu) float64(In^{s-1} + qe[f])
        g3   = g3 + float64(mu) float64(Q^{s-1})
        seed = gout[:, f] / R(S)  (mean)   |   gout[:, f - 1] if s - 1 = f S and f > 0 else 0   (end)
        lam  = (seed + b[d]) + C3 mu
    s = 0:  q0 array: gq0 = lam;   steady: mu = lam + a[d], a = mu, acc = acc + float64(mu);   gqe[0] = R(acc)
    (dk, dx) = ddr_amd.routing.muskingum_coefficient_gradients(k, x, dt)       (fp64; rounded once at the end)
    gk = ((dk[0] g1 + dk[1] g2) + dk[2] g3),   gx = ((dx[0] g1 + dx[1] g2) + dx[2] g3)
    gqext[f] = gqe[f] * flow_scale, 0 at invalid reaches
    gflow_scale = R(sum over f ascending of float64(gqe[f]) float64(q_filled[f]))

``In^s`` is the forward's upstream sum, in R and in the upstream list's order.  Gauge mode: ``gout[i]`` is the sum,
in R and in ascending gauge order, of the rows of the gauges that list reach ``i`` (with multiplicity).
"""

from __future__ import annotations

import numpy as np
import torch

import linear_cases as LC
from ddr_amd.routing import muskingum_coefficient_gradients


def downstream(topo: LC.Topology) -> np.ndarray:
    """down[i] (n for an outlet) from the upstream lists."""
    down = np.full(topo.n, topo.n, np.int64)
    for idx, ups in topo.levels:
        for a, i in enumerate(idx):
            for u in ups[a]:
                if u < topo.n:
                    down[u] = i
    return down


def forward_states(topo, c, S, q, q0, dtype):
    """(Q [FS + 1, n], In [FS + 1, n]) of the forward model (LC.route's operations)."""
    n = topo.n
    c1, c2, c3 = c
    F = q.shape[0]
    Q = np.zeros(n + 1, dtype)
    if isinstance(q0, str):
        hot = np.zeros(n + 1, np.float64)
        for idx, ups in topo.levels:
            acc = q[0, idx].astype(np.float64)
            for j in range(ups.shape[1]):
                acc = acc + hot[ups[:, j]]
            hot[idx] = acc
        Q[:n] = hot[:n].astype(dtype)
    elif q0 is not None:
        Q[:n] = np.asarray(q0, dtype)
    In = np.zeros(n, dtype)
    for lv in topo.levels:
        In[lv[0]] = LC._upsum(lv, Q, dtype)
    Qs, Ins = [Q[:n].copy()], [In.copy()]
    for f in range(F):
        qe = q[f]
        for _ in range(S):
            Qn = np.zeros(n + 1, dtype)
            Inn = np.zeros(n, dtype)
            for lv in topo.levels:
                idx = lv[0]
                inn = LC._upsum(lv, Qn, dtype)
                Qn[idx] = ((c1[idx] * (inn + qe[idx])) + (c2[idx] * (In[idx] + qe[idx]))) + (c3[idx] * Q[idx])
                Inn[idx] = inn
            Q, In = Qn, Inn
            Qs.append(Q[:n].copy())
            Ins.append(In.copy())
    return np.stack(Qs), np.stack(Ins)


def gauge_seeds(grows, gauges, n, F, dtype):
    """(N, F) seeds of (G, F) gauge rows: per reach the rows of its gauges, ascending gauge, with multiplicity."""
    out = np.zeros((n, F), dtype)
    for g, idx in enumerate(gauges):
        for i in np.asarray(idx).reshape(-1):
            i = int(i) % n if i < 0 else int(i)
            out[i] = out[i] + np.asarray(grows[g], dtype)
    return out


def adjoint(topo: LC.Topology, k, x, dt, substeps, qext, q0=None, output="mean", gout=None, glast=None,
            flow_scale=None, valid=None, dtype=np.float64, params=True):
    """The reverse sweep.  ``qext`` (F, N) raw; ``gout`` (N, F) or None; ``q0`` None, array or "steady".
    Returns dict(gqext (F, N), gq0, gk, gx, gflow_scale, and the fp64 sums of absolute terms gk_abs, gx_abs)."""
    n, S = topo.n, int(substeps)
    q = LC.forcing(qext, dtype, flow_scale, valid)
    F = q.shape[0]
    FS = F * S
    kk = np.broadcast_to(np.asarray(k, dtype), (n,))
    xx = np.broadcast_to(np.asarray(x, dtype), (n,))
    c1, c2, c3 = LC.coefficients(kk, xx, dt, dtype)
    down = downstream(topo)
    end = output == "end"
    steady = isinstance(q0, str)
    gout = np.zeros((n, F), dtype) if gout is None else np.asarray(gout, dtype)
    glast = np.zeros(n, dtype) if glast is None else np.asarray(glast, dtype)
    if params:
        Qs, Ins = forward_states(topo, (c1, c2, c3), S, q, q0, dtype)
    rev = topo.levels[::-1]
    Sr = dtype(S)
    lam = (gout[:, F - 1] if end else np.zeros(n, dtype)) + glast
    acc = np.zeros(n, np.float64)
    g1, g2, g3 = (np.zeros(n, np.float64) for _ in range(3))
    s1, s2, s3 = (np.zeros(n, np.float64) for _ in range(3))
    gqe = np.zeros((F, n), dtype)
    f64 = lambda v: v.astype(np.float64)  # noqa: E731
    for s in range(FS, 0, -1):
        f, ph = (s - 1) // S, (s - 1) % S
        a, b = np.zeros(n + 1, dtype), np.zeros(n + 1, dtype)
        mu = np.zeros(n, dtype)
        for idx, _ in rev:
            mu[idx] = lam[idx] + a[down[idx]]
            a[idx] = c1[idx] * mu[idx]
            b[idx] = c2[idx] * mu[idx]
        acc = acc + f64(a[:n] + b[:n])
        if params:
            t1, t2, t3 = f64(mu) * f64(Ins[s] + q[f]), f64(mu) * f64(Ins[s - 1] + q[f]), f64(mu) * f64(Qs[s - 1])
            g1, g2, g3 = g1 + t1, g2 + t2, g3 + t3
            s1, s2, s3 = s1 + np.abs(t1), s2 + np.abs(t2), s3 + np.abs(t3)
        if end:
            seed = gout[:, f - 1] if (ph == 0 and f > 0) else np.zeros(n, dtype)
        else:
            seed = gout[:, f] / Sr
        lam = (seed + b[down]) + (c3 * mu)
        if ph == 0 and f > 0:
            gqe[f] = acc.astype(dtype)
            acc = np.zeros(n, np.float64)
    gq0 = None
    if steady:
        a = np.zeros(n + 1, dtype)
        for idx, _ in rev:
            a[idx] = lam[idx] + a[down[idx]]
        acc = acc + f64(a[:n])
    elif q0 is not None:
        gq0 = lam.copy()
    gqe[0] = acc.astype(dtype)
    res = {"gq0": gq0, "gk": None, "gx": None}
    if params:
        # the package's closed-form coefficient derivatives, fp64 whatever the routed dtype
        wk, wx = muskingum_coefficient_gradients(kk, xx, dt)
        res["gk"] = (((wk[0] * g1) + (wk[1] * g2)) + (wk[2] * g3)).astype(dtype)
        res["gx"] = (((wx[0] * g1) + (wx[1] * g2)) + (wx[2] * g3)).astype(dtype)
        res["gk_abs"] = np.abs(wk[0]) * s1 + np.abs(wk[1]) * s2 + np.abs(wk[2]) * s3
        res["gx_abs"] = np.abs(wx[0]) * s1 + np.abs(wx[1]) * s2 + np.abs(wx[2]) * s3
    gqext = gqe.copy()
    if flow_scale is not None:
        gqext = (gqext * np.asarray(flow_scale, dtype)[None, :]).astype(dtype)
    qf = np.array(qext, dtype)
    if valid is not None:
        bad = np.asarray(valid) == 0
        gqext[:, bad] = 0
        qf[:, bad] = dtype(np.float32(0.001))
    gfs = np.zeros(n, np.float64)
    for f in range(F):
        gfs = gfs + (f64(gqe[f]) * f64(qf[f]))
    res["gqext"], res["gflow_scale"] = gqext, gfs.astype(dtype)
    return res


# ---- the independent reference: the forward in torch, differentiated by autograd ---------------------------

def adjacency(topo: LC.Topology) -> torch.Tensor:
    """Dense N (n, n), N[i, j] = 1 for every inflow j of reach i."""
    A = torch.zeros((topo.n, topo.n), dtype=torch.float64)
    for idx, ups in topo.levels:
        for a, i in enumerate(idx):
            for u in ups[a]:
                if u < topo.n:
                    A[int(i), int(u)] += 1.0
    return A


def torch_route(A, k, x, dt, substeps, qext, q0=None, flow_scale=None, valid=None):
    """(mean (N, F), end (N, F), q_last) of the scheme as one dense solve per sub-step:
    (I - C1 N) Q+ = C1 qe + C2 (N Q + qe) + C3 Q.  Tensors in, differentiable."""
    n, S = A.shape[0], int(substeps)
    q = qext
    if valid is not None:
        q = torch.where(torch.as_tensor(np.asarray(valid) != 0)[None, :], q, torch.full_like(q, float(np.float32(0.001))))
    if flow_scale is not None:
        q = q * flow_scale[None, :]
    h = dt / 2
    den = k * (1 - x) + h
    c1, c2, c3 = (h - k * x) / den, (h + k * x) / den, (k * (1 - x) - h) / den
    eye = torch.eye(n, dtype=q.dtype)
    M = eye - c1[:, None] * A
    if isinstance(q0, str):
        Q = torch.linalg.solve(eye - A, q[0])
    elif q0 is None:
        Q = torch.zeros(n, dtype=q.dtype)
    else:
        Q = q0
    mean, endl = [], []
    for f in range(q.shape[0]):
        acc = torch.zeros(n, dtype=q.dtype)
        for _ in range(S):
            acc = acc + Q
            rhs = c1 * q[f] + c2 * (A @ Q + q[f]) + c3 * Q
            Q = torch.linalg.solve(M, rhs)
        mean.append(acc / S)
        endl.append(Q)
    return torch.stack(mean, 1), torch.stack(endl, 1), Q


def autograd_reference(topo, k, x, dt, substeps, qext, q0, output, gout, glast, flow_scale=None, valid=None):
    """fp64 autograd gradients of <out, gout> + <q_last, glast>: dict(gqext, gq0, gk, gx, gflow_scale)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    kt, xt, qt = t(np.broadcast_to(np.asarray(k, np.float64), (topo.n,))), t(
        np.broadcast_to(np.asarray(x, np.float64), (topo.n,))), t(qext)
    q0t = t(q0) if (q0 is not None and not isinstance(q0, str)) else q0
    fst = t(flow_scale) if flow_scale is not None else None
    mean, endl, last = torch_route(adjacency(topo), kt, xt, float(dt), substeps, qt, q0t, fst, valid)
    out = endl if output == "end" else mean
    loss = torch.zeros((), dtype=torch.float64)
    if gout is not None:
        loss = loss + (out * torch.as_tensor(np.asarray(gout, np.float64))).sum()
    if glast is not None:
        loss = loss + (last * torch.as_tensor(np.asarray(glast, np.float64))).sum()
    wrt = {"gqext": qt, "gk": kt, "gx": xt}
    if isinstance(q0t, torch.Tensor):
        wrt["gq0"] = q0t
    if fst is not None:
        wrt["gflow_scale"] = fst
    grads = torch.autograd.grad(loss, list(wrt.values()), allow_unused=True)
    return {name: (np.zeros(tuple(v.shape)) if g is None else g.numpy()) for (name, v), g in zip(wrt.items(), grads)}


def random_seeds(n, F, seed, dtype):
    rng = np.random.default_rng(seed + 4300 + F)
    return rng.uniform(-1.0, 1.0, (n, F)).astype(dtype), rng.uniform(-1.0, 1.0, n).astype(dtype)
