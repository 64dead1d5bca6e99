"""Linear Muskingum routing on the device: RAPID's matrix scheme with per-reach constant (k, x).

The fixed-parameter baseline of the reference's ``benchmarks/`` package (DiffRoute's ``LTIRouter`` with
``irf_fn="muskingum"``, ``benchmark.py:121-234``) and the scheme RAPID runs operationally.  Per reach, with
the sub-step ``dt`` in seconds, ``h = dt / 2`` and ``den = k (1 - x) + h``::

    C1 = (h - k x) / den      C2 = (h + k x) / den      C3 = (k (1 - x) - h) / den
    Q+ = (C1 (In+ + qe) + C2 (In + qe)) + C3 Q          In+ = sum of the upstream Q+

in the routed precision, every operation rounded separately, no clamps: a negative ``C1`` (``dt < 2 k x``)
and negative discharge are RAPID's, not caught here.  The documented parameter range is ``k >= 0``,
``0 <= x <= 0.5``; values are not read back or checked, and NaN propagates.

No gradients: the benchmark runs this arm under ``no_grad``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..graph import RiverGraph
from ..ops import GaugeMap, _graph, register_graph

MODELS = ("muskingum", "linear_storage")
OUTPUTS = ("mean", "end")


def muskingum_coefficients(k, x, dt):
    """(C1, C2, C3) of RAPID's scheme in the kernel's operation order and in the dtype of ``k``: tensors (host or
    device) give tensors, anything else NumPy arrays.  ``dt`` and ``k`` in the same unit."""
    if isinstance(k, torch.Tensor):
        x = torch.as_tensor(x, dtype=k.dtype, device=k.device)
        h = torch.tensor(dt, dtype=k.dtype, device=k.device) / 2
        one = torch.ones((), dtype=k.dtype, device=k.device)
    else:
        k = np.asarray(k)
        if k.dtype not in (np.float32, np.float64):
            k = k.astype(np.float64)
        x = np.asarray(x, k.dtype)
        h = k.dtype.type(dt) / k.dtype.type(2)
        one = k.dtype.type(1)
    kx = k * x
    k1 = k * (one - x)
    den = k1 + h
    return (h - kx) / den, (h + kx) / den, (k1 - h) / den


def muskingum_coefficient_gradients(k, x, dt):
    """Closed-form derivatives of :func:`muskingum_coefficients`: ``((dC1/dk, dC2/dk, dC3/dk), (dC1/dx, dC2/dx,
    dC3/dx))``, with ``h = dt / 2`` and ``den = k (1 - x) + h``::

        dC/dk = (-h, h (2 x - 1), 2 h (1 - x)) / den^2        dC/dx = (-k^2, k (k + 2 h), -2 h k) / den^2

    Always evaluated and returned in float64, whatever the dtype of ``k``: each set sums to zero (C1 + C2 + C3 = 1),
    so a parameter gradient ``sum_j dL/dC_j dC_j/dk`` is the remainder of cancelling terms and is to be combined in
    fp64 and rounded once.  Tensors (host or device) give tensors, anything else NumPy arrays; ``h`` is taken from
    ``dt`` rounded as the routing rounds it, in the dtype of ``k``."""
    if isinstance(k, torch.Tensor):
        h = (torch.tensor(dt, dtype=k.dtype, device=k.device) / 2).to(torch.float64)
        x = torch.as_tensor(x, dtype=k.dtype, device=k.device).to(torch.float64)
        k = k.to(torch.float64)
    else:
        k = np.asarray(k)
        if k.dtype not in (np.float32, np.float64):
            k = k.astype(np.float64)
        h = np.float64(k.dtype.type(dt) / k.dtype.type(2))
        x = np.asarray(x, k.dtype).astype(np.float64)
        k = k.astype(np.float64)
    den = (k * (1.0 - x)) + h
    d2 = den * den
    dk = ((-h) / d2, (h * ((2.0 * x) - 1.0)) / d2, ((2.0 * h) * (1.0 - x)) / d2)
    dx = ((-(k * k)) / d2, (k * (k + (2.0 * h))) / d2, (-((2.0 * h) * k)) / d2)
    return dk, dx


def rapid_parameters(ids, reach_ids, k, x, k_units: str = "seconds"):
    """RAPID's parameter files aligned to a network: ``k`` (seconds) and ``x`` of reach ``ids[i]``, looked up in
    ``reach_ids`` (the order of RAPID's ``k`` and ``x`` files), as float64 arrays in the order of ``ids``
    (e.g. ``Network.ids``).  ``k_units``: ``"seconds"`` or ``"days"``.  An id missing from ``reach_ids`` raises."""
    if k_units not in ("seconds", "days"):
        raise ValueError(f"k_units must be 'seconds' or 'days', not {k_units!r}")
    ids = np.asarray(ids, np.int64).reshape(-1)
    reach_ids = np.asarray(reach_ids, np.int64).reshape(-1)
    k = np.asarray(k, np.float64).reshape(-1)
    x = np.asarray(x, np.float64).reshape(-1)
    if not (len(reach_ids) == len(k) == len(x)):
        raise ValueError("reach_ids, k and x differ in length")
    order = np.argsort(reach_ids, kind="stable")
    srt = reach_ids[order]
    if len(srt) > 1 and np.any(srt[1:] == srt[:-1]):
        raise ValueError("reach_ids holds duplicates")
    if len(srt) == 0:
        if len(ids):
            raise ValueError("an id of the network is missing from reach_ids")
        return k[:0], x[:0]
    at = np.minimum(np.searchsorted(srt, ids), len(srt) - 1)
    if np.any(srt[at] != ids):
        raise ValueError("an id of the network is missing from reach_ids")
    row = order[at]
    return k[row] * (86400.0 if k_units == "days" else 1.0), x[row]


@torch.library.custom_op("ddrx::lin_route", mutates_args=())
def lin_route(qext: torch.Tensor, k: torch.Tensor, x: torch.Tensor, flow_scale: torch.Tensor | None,
              valid: torch.Tensor | None, q0: torch.Tensor | None, g_off: torch.Tensor | None,
              g_idx: torch.Tensor | None, graph_id: int, dt: float, substeps: int, flags: int
              ) -> tuple[torch.Tensor, torch.Tensor]:
    """Returns (out, q_last): ``out`` (N, F), or (G, F) in gauge mode (``g_off`` / ``g_idx``)."""
    g = _graph(graph_id)
    F, N = qext.shape
    dev, dtp = qext.device, qext.dtype
    f32 = dtp == torch.float32
    lib = _lib.load()
    T1 = F * int(substeps) + 1
    out = torch.empty((N, F), device=dev, dtype=dtp)
    q_last = torch.empty(N, device=dev, dtype=dtp)
    work = torch.empty(int(lib.ddr_lin_work_bytes(g.handle, F, 4 if f32 else 8)), device=dev, dtype=torch.uint8)
    bnd = torch.empty(g.bnd_numel(T1), device=dev, dtype=torch.float64)
    status = torch.empty(g.info.status_bytes, device=dev, dtype=torch.uint8)
    stream = _lib.stream_ptr(dev)
    fn = lib.ddr_lin_route_f32 if f32 else lib.ddr_lin_route_f64
    _lib.check(fn(g.handle, k.data_ptr(), x.data_ptr(), float(dt), int(substeps), int(F), qext.data_ptr(),
                  _lib.ptr(flow_scale), _lib.ptr(valid), _lib.ptr(q0), int(flags), out.data_ptr(), q_last.data_ptr(),
                  work.data_ptr(), bnd.data_ptr() if bnd.numel() else None, status.data_ptr(), stream))
    if g_off is not None:
        G = g_off.numel() - 1
        rows = torch.empty((G, F), device=dev, dtype=dtp)
        gz = _lib.Gauges(G, g_off.data_ptr(), g_idx.data_ptr(), None, None)
        red = lib.ddr_lin_gauge_f32 if f32 else lib.ddr_lin_gauge_f64
        _lib.check(red(N, F, C.byref(gz), out.data_ptr(), rows.data_ptr(), stream))
        out = rows
    return out, q_last


@lin_route.register_fake
def _(qext, k, x, flow_scale, valid, q0, g_off, g_idx, graph_id, dt, substeps, flags):
    F, N = qext.shape
    G = g_off.shape[0] - 1 if g_off is not None else N
    return qext.new_empty((G, F)), qext.new_empty(N)


class LinearMuskingum:
    """Linear routing of one network with fixed per-reach parameters.

    ``k`` (seconds) and ``x``: (N,) device tensors or floats; ``dt`` the sub-step in seconds; the forcing holds
    over ``substeps`` sub-steps.  ``model="linear_storage"``: the same scheme with ``x = 0`` and ``k`` the time
    constant.  ``lm(qext, ...)`` routes ``qext`` (F, N), one row per forcing interval, and returns
    ``(out, q_last)``: ``out`` (N, F) -- (G, F) with ``gauges`` -- and the final state (N,).

    ``output="mean"``: the mean of the ``substeps`` states at the beginning of each sub-step (RAPID's ``Qout``;
    summed in fp64, rounded once); ``"end"``: the state after the interval's last sub-step.  ``q0``: ``None``
    (zeros), an (N,) tensor (RAPID's ``Qinit``, or a previous call's ``q_last``), or ``"steady"`` (the steady
    state of forcing row 0)."""

    def __init__(self, graph: RiverGraph, k, x=None, *, dt: float = 3600.0, substeps: int = 1,
                 model: str = "muskingum"):
        if model not in MODELS:
            raise ValueError(f"model must be one of {MODELS}, not {model!r}")
        if model == "linear_storage":
            if x is not None:
                raise ValueError("linear_storage takes no x (it is the scheme with x = 0)")
            x = 0.0
        elif x is None:
            raise ValueError("muskingum needs x")
        if isinstance(substeps, bool) or int(substeps) != substeps or int(substeps) < 1:
            raise ValueError("substeps must be an integer >= 1")
        if not float(dt) > 0.0:
            raise ValueError("dt must be positive")
        n = graph.n
        for name, v in (("k", k), ("x", x)):
            if isinstance(v, torch.Tensor):
                if v.dim() != 1 or v.numel() != n:
                    raise ValueError(f"{name} has shape {tuple(v.shape)}, the network has {n} reaches")
                if v.dtype not in (torch.float32, torch.float64):
                    raise ValueError(f"{name} must be float32 or float64")
                if v.requires_grad:
                    raise NotImplementedError("linear routing has no gradients (the adjoint is not implemented)")
            elif not isinstance(v, (int, float)):
                raise ValueError(f"{name} must be an (N,) tensor or a float")
        for name, v in (("k", k), ("x", x)):
            if isinstance(v, torch.Tensor) and not v.is_cuda:
                raise RuntimeError(f"{name} is a host tensor: linear routing runs on the HIP device only")
        self.graph, self.k, self.x = graph, k, x
        self.dt, self.substeps, self.model = float(dt), int(substeps), model
        self._cache = {}

    def _params(self, dtype, device):
        key = (dtype, str(device))
        if key not in self._cache:
            def full(v):
                if isinstance(v, torch.Tensor):
                    return v.detach().to(device=device, dtype=dtype).contiguous()
                return torch.full((self.graph.n,), float(v), dtype=dtype, device=device)
            self._cache[key] = (full(self.k), full(self.x))
        return self._cache[key]

    def __call__(self, qext, q0=None, output: str = "mean", gauges: GaugeMap | None = None, flow_scale=None,
                 valid=None):
        if output not in OUTPUTS:
            raise ValueError(f"output must be one of {OUTPUTS}, not {output!r}")
        n = self.graph.n
        if not isinstance(qext, torch.Tensor) or qext.dim() != 2 or qext.shape[1] != n or qext.shape[0] < 1:
            raise ValueError(f"qext must be an (F, {n}) tensor with F >= 1")
        if qext.dtype not in (torch.float32, torch.float64):
            raise ValueError("qext must be float32 or float64")
        steady = isinstance(q0, str)
        if steady and q0 != "steady":
            raise ValueError(f"q0 must be None, an (N,) tensor or 'steady', not {q0!r}")
        tensors = [("flow_scale", flow_scale), ("q0", None if steady else q0)]
        for name, t in tensors:
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != n:
                raise ValueError(f"{name} must be an (N,) tensor of {n} reaches")
            if t.dtype != qext.dtype:
                raise ValueError(f"{name} is {t.dtype}, qext is {qext.dtype}")
        if valid is not None and (not isinstance(valid, torch.Tensor) or valid.dim() != 1 or valid.numel() != n
                                  or valid.dtype not in (torch.bool, torch.uint8)):
            raise ValueError("valid must be an (N,) bool or uint8 mask")
        if gauges is not None and not isinstance(gauges, GaugeMap):
            raise ValueError("gauges must be an ops.GaugeMap")
        for name, t in [("qext", qext)] + tensors:
            if t is not None and t.requires_grad:
                raise NotImplementedError("linear routing has no gradients (the adjoint is not implemented)")
        for name, t in [("qext", qext), ("valid", valid)] + tensors:
            if t is not None and not t.is_cuda:
                raise RuntimeError(f"{name} is a host tensor: linear routing runs on the HIP device only "
                                   "(no CPU fallback)")
        dev = qext.device
        k, x = self._params(qext.dtype, dev)
        flags = (_lib.DDR_LIN_END if output == "end" else 0) | (_lib.DDR_LIN_STEADY if steady else 0)
        cont = lambda t: None if t is None else t.contiguous()  # noqa: E731
        vmask = None if valid is None else valid.to(torch.uint8).contiguous()
        gid = register_graph(self.graph)
        return lin_route(qext.contiguous(), k, x, cont(flow_scale), vmask, None if steady else cont(q0),
                         gauges.offsets if gauges else None, gauges.index if gauges else None, gid, self.dt,
                         self.substeps, flags)
