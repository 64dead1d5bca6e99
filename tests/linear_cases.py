"""The linear Muskingum routing's host model, networks and case lists (tests/test_linear_model.py on the CPU,
tests/test_gpu_linear.py on the device).

The model restates RAPID's scheme in NumPy, in fp32 or fp64, with the kernel's operations in the kernel's order:

    h = dt / 2, den = k (1 - x) + h, C1 = (h - k x) / den, C2 = (h + k x) / den, C3 = (k (1 - x) - h) / den
    In+ = ((0 + Q+_a) + Q+_b) + ...          upstream reaches in the order of the CSR row (ascending)
    Q+  = (C1 (In+ + qe) + C2 (In + qe)) + C3 Q

Reaches of one level (longest path from a headwater) do not depend on each other, so a sub-step is one vector
operation per level and upstream slot; a missing slot adds an exact zero, as the kernel's zero slot does.
"""

from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

from ddr_amd.graph import RiverGraph

GOLDEN = Path(__file__).resolve().parent / "golden"

# (F, S) of the time-axis sweep; depth_cases() adds F * S around the deepest block's depth and an import chunk
TIME_AXIS = ((1, 1), (1, 12), (2, 1), (3, 2), (5, 7), (17, 3), (80, 12))
CHUNK_FWD = 4  # kChunkFwd (internal.h)
K_RANGE, X_RANGE = (600.0, 40000.0), (0.0, 0.5)


def depth_cases(info):
    """(F, 1) with F on both sides of the deepest block's depth and of the next multiple of the import chunk."""
    d = int(info.max_block_depth)
    m = CHUNK_FWD * (d // CHUNK_FWD + 1)
    return tuple((f, 1) for f in sorted({t for c in (d, m) for t in (c - 1, c, c + 1) if t >= 1}))


@functools.lru_cache(maxsize=None)
def sandbox():
    d = np.load(GOLDEN / "rapid_sandbox.npz")
    return {k: d[k] for k in d.files}


class Topology:
    """Upstream lists by level, from a CSR (row = downstream reach, columns ascending)."""

    def __init__(self, n, crow, col):
        self.n = int(n)
        crow, col = np.asarray(crow, np.int64), np.asarray(col, np.int64)
        deg = np.diff(crow)
        level = np.zeros(self.n, np.int64)
        for i in range(self.n):  # lower triangular: every upstream reach has a smaller index
            if deg[i]:
                level[i] = level[col[crow[i]:crow[i + 1]]].max() + 1
        self.levels = []
        for lv in range(int(level.max()) + 1 if self.n else 0):
            idx = np.flatnonzero(level == lv)
            width = int(deg[idx].max())
            ups = np.full((len(idx), width), self.n, np.int64)  # n: the zero entry
            for a, i in enumerate(idx):
                ups[a, :deg[i]] = col[crow[i]:crow[i + 1]]
            self.levels.append((idx, ups))

    @classmethod
    def of_graph(cls, g: RiverGraph):
        crow, col = g.csr()
        return cls(g.n, crow, col)

    @classmethod
    def of_coo(cls, n, rows, cols):
        return cls.of_graph(RiverGraph(n, rows, cols, host_only=True))


def coefficients(k, x, dt, dtype):
    k, x = np.asarray(k, dtype), np.asarray(x, dtype)
    h = dtype(dt) / dtype(2)
    kx = k * x
    k1 = k * (dtype(1) - x)
    den = k1 + h
    return (h - kx) / den, (h + kx) / den, (k1 - h) / den


def forcing(qext, dtype, flow_scale=None, valid=None):
    """The series the kernel routes: a missing reach's 0.001 fill, then one multiplication by flow_scale."""
    q = np.array(qext, dtype)
    if valid is not None:
        q[:, np.asarray(valid) == 0] = dtype(np.float32(0.001))
    if flow_scale is not None:
        q = (q * np.asarray(flow_scale, dtype)[None, :]).astype(dtype)
    return q


def _upsum(top_level, state, dtype):
    idx, ups = top_level
    acc = np.zeros(len(idx), dtype)
    for j in range(ups.shape[1]):
        acc = acc + state[ups[:, j]]
    return acc


def route(topo: Topology, k, x, dt, substeps, qext, q0=None, dtype=np.float64):
    """dict(mean (N, F), end (N, F), q_last (N,)); ``qext`` (F, N) as routed (see :func:`forcing`); ``q0``: None,
    an (N,) array or "steady"."""
    n, S = topo.n, int(substeps)
    q = np.asarray(qext, dtype)
    F = q.shape[0]
    c1, c2, c3 = coefficients(np.broadcast_to(np.asarray(k, dtype), (n,)), np.broadcast_to(np.asarray(x, dtype), (n,)),
                              dt, dtype)
    Q = np.zeros(n + 1, dtype)  # entry n stays 0
    if isinstance(q0, str):
        assert q0 == "steady"
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
        In[lv[0]] = _upsum(lv, Q, dtype)
    mean, end = np.zeros((n, F), dtype), np.zeros((n, F), dtype)
    for f in range(F):
        qe = q[f]
        acc = np.zeros(n, np.float64)
        for _ in range(S):
            acc = acc + Q[:n].astype(np.float64)
            Qn = np.zeros(n + 1, dtype)
            Inn = np.zeros(n, dtype)
            for lv in topo.levels:
                idx = lv[0]
                inn = _upsum(lv, Qn, dtype)
                Qn[idx] = ((c1[idx] * (inn + qe[idx])) + (c2[idx] * (In[idx] + qe[idx]))) + (c3[idx] * Q[idx])
                Inn[idx] = inn
            Q, In = Qn, Inn
        mean[:, f] = (acc / np.float64(S)).astype(dtype)
        end[:, f] = Q[:n]
    return {"mean": mean, "end": end, "q_last": Q[:n].copy()}


def gauge_rows(out_nf, gauges, dtype):
    """Gauge rows of an (N, F) output: each gauge's reaches added in list order."""
    n = out_nf.shape[0]
    rows = np.zeros((len(gauges), out_nf.shape[1]), dtype)
    for g, idx in enumerate(gauges):
        acc = np.zeros(out_nf.shape[1], dtype)
        for i in np.asarray(idx).reshape(-1):
            acc = acc + out_nf[int(i) % n if i < 0 else int(i)]
        rows[g] = acc
    return rows


def parameters(n, seed, dtype):
    rng = np.random.default_rng(seed + 4100)
    return rng.uniform(*K_RANGE, n).astype(dtype), rng.uniform(*X_RANGE, n).astype(dtype)


def random_forcing(n, F, seed, dtype, tail_zeros=0):
    rng = np.random.default_rng(seed + 4200 + F)
    q = rng.uniform(0.0, 3.0, (F, n)).astype(dtype)
    if tail_zeros:
        q[F - tail_zeros:] = 0
    return q
