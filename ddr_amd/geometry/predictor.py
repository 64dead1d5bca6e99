"""Drop-in for ``ddr.geometry.predictor`` (reference ``src/ddr/geometry/predictor.py:41-414``) on the HIP device.

Catchment attributes -> trained KAN -> Manning's n and the Leopold & Maddock p / q -> trapezoid geometry at a
discharge and slope per reach.  The reference does this in ~40 PyTorch / NumPy passes around the KAN; here it is
two kernels around the KAN's launches (``csrc/geopredict.hip``)::

    raw (F, N) --attr_prepare_kernel--> x (chunk, F) --ddr_kan_forward_f32--> u (N, O)
                                                      --geometry_predict_kernel--> out (11, N)

* ``attr_prepare_kernel``: the source's unit conversion (fp64, ``adapters.py:159-162``), the p10 / p90
  out-of-distribution counts (``predictor.py:320-350``), the NaN fill with the training mean and the z-score
  (``predictor.py:241-274``), and the transpose to the KAN's row-major input.
* ``geometry_predict_kernel``: ``denormalize`` of the three parameters (``routing/utils.py:166-185``), the two
  lower clamps of discharge and slope (``predictor.py:211-214``, NaN kept) and ``compute_trapezoidal_geometry``
  (``trapezoidal.py:62-97``) in the reference's operation order.

xarray stays with the caller: attributes come in as a mapping ``name -> (N,)`` array-like (an ``xarray.Dataset``
works through the same ``attrs[name].values`` access) or as one device tensor (F, N), and the results are
device tensors.  HIP device and fp32 only; there is no CPU fallback.  No gradients (the reference runs the
predictor under ``no_grad``).
"""

from __future__ import annotations

import ctypes as C
import json
import logging
from collections.abc import Mapping
from pathlib import Path

import numpy as np
import torch

from .. import _lib
from ..nn.kan import _check_device_f32, kan, load_checkpoint
from .adapters import adapt_attributes

log = logging.getLogger(__name__)

# the rows of the (11, N) result: include/ddr_mc.h DDR_GEOM_*, the reference's order (predictor.py:216-238)
GEOMETRY_OUTPUTS = ("depth", "top_width", "bottom_width", "side_slope", "cross_sectional_area", "wetted_perimeter",
                    "hydraulic_radius", "velocity", "n", "p_spatial", "q_spatial")
COUNT_NAMES = ("filled", "below", "above")

# the reference's Params / Kan defaults (src/ddr/validation/configs.py:81-141) for what a config leaves out
_PARAMS_DEFAULT = dict(
    parameter_ranges={"n": [0.015, 0.25], "q_spatial": [0.0, 1.0], "p_spatial": [1.0, 200.0]},
    log_space_parameters=["p_spatial"], defaults={"p_spatial": 21},
    attribute_minimums={"discharge": 0.0001, "slope": 0.001, "velocity": 0.01, "depth": 0.01, "bottom_width": 0.01})
_KAN_DEFAULT = dict(hidden_size=11, num_hidden_layers=1, learnable_parameters=["n", "q_spatial"], grid=3, k=3)


def _need_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"GeometryPredictor runs on the HIP device only (no CPU fallback): {what} is on {t.device}")


def _f32(t: torch.Tensor, what: str) -> None:
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32 (got {t.dtype})")


def prepare_attributes(raw: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, log10: torch.Tensor,
                       mean: torch.Tensor, std: torch.Tensor, p10: torch.Tensor | None = None,
                       p90: torch.Tensor | None = None, counts: torch.Tensor | None = None,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """One ``ddr_attr_prepare_f32`` launch: raw (F, N) device fp32 (rows may be strided) -> x (N, F).

    ``scale`` / ``offset`` are fp64 (F,), ``log10`` int32 (F,), the rest fp32 (F,), all on raw's device;
    ``counts`` (3, F) int64 is accumulated into (zero it first)."""
    _need_device(raw, "the attribute tensor")
    _f32(raw, "the attribute tensor")
    if raw.dim() != 2 or (raw.shape[1] > 1 and raw.stride(1) != 1):
        raise ValueError("the attribute tensor must be (F, N) with contiguous rows")
    F, N = raw.shape
    dev = raw.device
    for name, t, dt in (("scale", scale, torch.float64), ("offset", offset, torch.float64), ("log10", log10, torch.int32),
                        ("mean", mean, torch.float32), ("std", std, torch.float32), ("p10", p10, torch.float32),
                        ("p90", p90, torch.float32)):
        if t is None:
            continue
        if t.device != dev or t.dtype != dt or tuple(t.shape) != (F,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape ({F},) on {dev}")
    if counts is not None and (counts.device != dev or counts.dtype != torch.int64 or tuple(counts.shape) != (3, F)
                               or not counts.is_contiguous()):
        raise ValueError(f"counts must be a contiguous int64 tensor of shape (3, {F}) on {dev}")
    if out is None:
        out = torch.empty((N, F), device=dev, dtype=torch.float32)
    elif out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != (N, F) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor of shape ({N}, {F}) on {dev}")
    _lib.check(_lib.load().ddr_attr_prepare_f32(
        N, F, raw.data_ptr(), raw.stride(0) if F > 1 else N, scale.data_ptr(), offset.data_ptr(), log10.data_ptr(),
        mean.data_ptr(), std.data_ptr(), _lib.ptr(p10), _lib.ptr(p90), out.data_ptr(), _lib.ptr(counts),
        _lib.stream_ptr(dev)))
    return out


def geometry_predict(u: torch.Tensor, slots, discharge: torch.Tensor | None, slope: torch.Tensor | None,
                     attribute_minimums: Mapping | None = None) -> torch.Tensor:
    """One ``ddr_geometry_predict_f32`` launch: u (N, O) device fp32 -> (11, N) in ``GEOMETRY_OUTPUTS`` order, or
    (3, N) = n, p_spatial, q_spatial when ``discharge`` and ``slope`` are None.  ``slots`` are three
    ``_lib.GeomSlot`` (n, q_spatial, p_spatial)."""
    _need_device(u, "the KAN output")
    _f32(u, "the KAN output")
    if u.dim() != 2 or not u.is_contiguous():
        raise ValueError("the KAN output must be a contiguous (N, O) tensor")
    N, O = u.shape
    if (discharge is None) != (slope is None):
        raise ValueError("discharge and slope go together")
    for name, t in (("discharge", discharge), ("slope", slope)):
        if t is None:
            continue
        _need_device(t, name)
        _f32(t, name)
        if t.device != u.device:
            raise ValueError(f"{name} must be on {u.device} (got {t.device})")
        if tuple(t.shape) != (N,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous tensor of shape ({N},), got {tuple(t.shape)}")
    mins = attribute_minimums or {}
    out = torch.empty((len(GEOMETRY_OUTPUTS) if discharge is not None else 3, N), device=u.device, dtype=torch.float32)
    sn, sq, sp = slots
    _lib.check(_lib.load().ddr_geometry_predict_f32(
        N, O, u.data_ptr(), C.byref(sn), C.byref(sq), C.byref(sp), _lib.ptr(discharge), _lib.ptr(slope),
        float(mins.get("discharge", 0.0001)), float(mins.get("slope", 0.001)), float(mins.get("depth", 0.01)),
        float(mins.get("bottom_width", 0.01)), out.data_ptr(), N, _lib.stream_ptr(u.device)))
    return out


def _get(cfg, key, default=None):
    if isinstance(cfg, Mapping):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _plain(v):
    """A config node as plain dicts / lists (a mapping, a namespace or a value)."""
    if isinstance(v, Mapping):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v


class GeometryPredictor:
    """``ddr.geometry.GeometryPredictor`` (``predictor.py:41-96``: the same constructor arguments) on the device.

    ``nn_model`` is a :class:`ddr_amd.nn.kan` holding the checkpoint's weights; ``means`` / ``stds`` the z-score
    statistics (n_attrs,); ``parameter_ranges`` / ``log_space_parameters`` / ``defaults`` / ``attribute_minimums``
    the reference's ``params.*``; ``stats_ranges`` the per-attribute ``{"p10", "p90"}`` of the training
    distribution (None: no out-of-distribution counts).  ``n`` and ``q_spatial`` must be among the KAN's learnable
    parameters (the reference has no default for them); ``p_spatial`` falls back to ``defaults["p_spatial"]``.

    ``chunk_rows`` bounds the KAN's input and workspace (the results do not depend on it, bit for bit).
    ``check_distribution=True`` reads the 3 F counters back after each call (one small copy, which waits for the
    launches), logs the reference's two messages and keeps them in ``last_counts``; ``False`` counts nothing and
    does not synchronise.

    A predictor can be *built* on any device (to inspect a checkpoint); every ``predict*`` call needs the HIP
    device and raises ``RuntimeError`` otherwise."""

    def __init__(self, nn_model: kan, attribute_names, means: torch.Tensor, stds: torch.Tensor, parameter_ranges,
                 log_space_parameters, defaults, attribute_minimums, stats_ranges=None, device="cuda",
                 chunk_rows: int = 1 << 20, check_distribution: bool = True) -> None:
        if not isinstance(nn_model, kan):
            raise TypeError("nn_model must be a ddr_amd.nn.kan (the HIP network; TorchKan is the PyTorch model)")
        self._nn = nn_model.eval()
        self._attribute_names = list(attribute_names)
        F = len(self._attribute_names)
        if F != nn_model.input_size:
            raise ValueError(f"the KAN takes {nn_model.input_size} attributes, attribute_names has {F}")
        self._device = torch.device(device)
        if self._device.type == "cuda" and self._device.index is None and torch.cuda.is_available():
            self._device = torch.device("cuda", torch.cuda.current_device())
        self._means = torch.as_tensor(means, dtype=torch.float32).reshape(-1).to(self._device).contiguous()
        self._stds = torch.as_tensor(stds, dtype=torch.float32).reshape(-1).to(self._device).contiguous()
        if self._means.numel() != F or self._stds.numel() != F:
            raise ValueError(f"means and stds must have {F} elements")
        self._parameter_ranges = {k: [float(x) for x in v] for k, v in _plain(parameter_ranges).items()}
        self._log_space_parameters = list(log_space_parameters)
        self._defaults = dict(_plain(defaults))
        self._attribute_minimums = dict(_plain(attribute_minimums))
        self._stats_ranges = _plain(stats_ranges) if stats_ranges is not None else None
        self.chunk_rows = int(chunk_rows)
        if self.chunk_rows < 1:
            raise ValueError("chunk_rows must be at least 1")
        self.check_distribution = bool(check_distribution)
        self.last_counts: dict | None = None
        self._slots = self._make_slots()
        self._p10 = self._p90 = None
        if self._stats_ranges is not None:  # an attribute without a range is never out of it (predictor.py:334)
            inf = float("inf")
            lo = [float(self._stats_ranges.get(a, {}).get("p10", -inf)) for a in self._attribute_names]
            hi = [float(self._stats_ranges.get(a, {}).get("p90", inf)) for a in self._attribute_names]
            self._p10 = torch.tensor(lo, dtype=torch.float32, device=self._device)
            self._p90 = torch.tensor(hi, dtype=torch.float32, device=self._device)
        self._transforms: dict = {}

    # ---- construction ----
    def _make_slots(self):
        learn = list(self._nn.learnable_parameters)
        slots = []
        for name in ("n", "q_spatial", "p_spatial"):
            learned = name in learn and name in self._parameter_ranges
            if not learned and name != "p_spatial":
                raise ValueError(f"the KAN must learn {name!r} with a range in parameter_ranges (learnable_parameters "
                                 f"= {learn}): the reference has a default for p_spatial only")
            if learned:
                lo, hi = self._parameter_ranges[name]
                slots.append(_lib.GeomSlot(learn.index(name), int(name in self._log_space_parameters), lo, hi, 0.0))
            else:
                slots.append(_lib.GeomSlot(-1, 0, 0.0, 0.0, float(self._defaults.get("p_spatial", 21.0))))
        return tuple(slots)

    @classmethod
    def from_checkpoint(cls, checkpoint_path, config, stats_path=None, device="cuda", **kwargs) -> GeometryPredictor:
        """``predictor.py:98-162``: build the KAN of ``config``, load ``checkpoint_path`` into it and read the
        attribute statistics JSON.  ``config`` is a mapping or the path of a YAML file with the fields of the
        reference's ``config/merit_geometry_config.yaml`` -- ``kan.*``, ``params.parameter_ranges`` /
        ``log_space_parameters`` / ``defaults`` / ``attribute_minimums``, ``seed`` -- anything missing takes the
        reference's default.  ``kwargs`` (``chunk_rows``, ``check_distribution``) go to the constructor."""
        if not isinstance(config, Mapping):
            import yaml

            with open(config) as f:
                config = yaml.safe_load(f)
        kcfg = dict(_KAN_DEFAULT, **_plain(_get(config, "kan") or {}))
        if "input_var_names" not in kcfg:
            raise ValueError("the config has no kan.input_var_names")
        pcfg = _plain(_get(config, "params") or {})
        params = {k: pcfg.get(k, v) for k, v in _PARAMS_DEFAULT.items()}
        names = list(kcfg["input_var_names"])
        model = kan(input_var_names=names, learnable_parameters=list(kcfg["learnable_parameters"]),
                    hidden_size=kcfg["hidden_size"], num_hidden_layers=kcfg["num_hidden_layers"], grid=kcfg["grid"],
                    k=kcfg["k"], seed=int(_get(config, "seed", 0) or 0), device=device)
        load_checkpoint(model, checkpoint_path, device)
        means, stds, ranges = cls._load_normalization_stats(config, names, stats_path, device)
        return cls(nn_model=model, attribute_names=names, means=means, stds=stds,
                   parameter_ranges=params["parameter_ranges"], log_space_parameters=params["log_space_parameters"],
                   defaults=params["defaults"], attribute_minimums=params["attribute_minimums"], stats_ranges=ranges,
                   device=device, **kwargs)

    @staticmethod
    def _load_normalization_stats(cfg, attribute_names, stats_path, device):
        """``predictor.py:352-414``: ``stats[attr]["mean" | "std" | "p10" | "p90"]`` of the statistics JSON; without
        ``stats_path`` the file the training wrote, ``{data_sources.statistics}/{geodataset}_attribute_statistics_
        {name of data_sources.attributes}.json``."""
        if stats_path is not None:
            json_path = Path(stats_path)
        else:
            ds = _plain(_get(cfg, "data_sources") or {})
            if "statistics" not in ds or "attributes" not in ds:
                raise FileNotFoundError("Attribute statistics file not found: the config names no data_sources.statistics "
                                        "/ data_sources.attributes. Provide stats_path explicitly.")
            json_path = Path(str(ds["statistics"])) / (f"{_get(cfg, 'geodataset')}_attribute_statistics_"
                                                       f"{Path(str(ds['attributes'])).name}.json")
        if not json_path.exists():
            raise FileNotFoundError(f"Attribute statistics file not found: {json_path}. Provide stats_path explicitly "
                                    "or run training first to generate statistics.")
        log.info("Loading normalization statistics from %s", json_path)
        with open(json_path) as f:
            stats = json.load(f)
        for attr in attribute_names:
            if attr not in stats:
                raise KeyError(f"Attribute {attr!r} not found in statistics file {json_path}")
        means = torch.tensor([float(stats[a]["mean"]) for a in attribute_names], device=device, dtype=torch.float32)
        stds = torch.tensor([float(stats[a]["std"]) for a in attribute_names], device=device, dtype=torch.float32)
        ranges = {a: {"p10": float(stats[a]["p10"]), "p90": float(stats[a]["p90"])} for a in attribute_names}
        return means, stds, ranges

    # ---- inputs ----
    @property
    def attribute_names(self) -> list[str]:
        return list(self._attribute_names)

    def _ready(self) -> torch.device:
        """RuntimeError unless the predictor and its KAN live on one HIP device."""
        _need_device(self._means, "the predictor")
        _need_device(self._nn.flat, "the KAN")
        if self._nn.flat.device != self._means.device:
            raise RuntimeError(f"the KAN is on {self._nn.flat.device}, the predictor on {self._means.device}")
        return self._means.device

    def _transform(self, adapted, dev):
        """The per-feature (scale, offset, log10) of a source in ``attribute_names`` order, on the device (kept)."""
        if adapted is None or adapted.source not in self._transforms:
            F = len(self._attribute_names)
            if adapted is None:
                sc, of, lg = np.ones(F), np.zeros(F), np.zeros(F, np.int32)
            else:
                order = [list(adapted.columns).index(a) for a in self._attribute_names]
                sc, of, lg = adapted.scale[order], adapted.offset[order], adapted.log10[order]
            t = (torch.tensor(sc, dtype=torch.float64, device=dev), torch.tensor(of, dtype=torch.float64, device=dev),
                 torch.tensor(lg, dtype=torch.int32, device=dev))
            self._transforms["merit" if adapted is None else adapted.source] = t
        return self._transforms["merit" if adapted is None else adapted.source]

    def _raw(self, attributes, source: str, dev: torch.device):
        """(raw (F, N) device fp32, the source's transform)."""
        F = len(self._attribute_names)
        if isinstance(attributes, torch.Tensor):
            _need_device(attributes, "the attribute tensor")
            if attributes.device != dev:
                raise ValueError(f"the attribute tensor must be on {dev} (got {attributes.device})")
            _f32(attributes, "the attribute tensor")
            if source not in ("auto", "merit"):
                raise ValueError("a tensor of attributes is in attribute_names order: source must be 'merit' or 'auto'")
            if attributes.dim() != 2 or attributes.shape[0] != F:
                raise ValueError(f"the attribute tensor must be ({F}, N) in attribute_names order, got "
                                 f"{tuple(attributes.shape)}")
            if attributes.shape[1] > 1 and attributes.stride(1) != 1:
                attributes = attributes.contiguous()
            return attributes, self._transform(None, dev)
        adapted = adapt_attributes(attributes, source=source)
        cols = []
        for name in self._attribute_names:  # (predictor.py:253: np.asarray(adapted[name].values, float32))
            col = adapted.columns[name]
            if isinstance(col, torch.Tensor):
                col = col.detach().cpu().numpy()
            cols.append(np.asarray(getattr(col, "values", col), dtype=np.float32).reshape(-1))
        if len({c.shape[0] for c in cols}) != 1:
            raise ValueError("the attributes do not have one length")
        raw = torch.from_numpy(np.stack(cols, axis=0)).to(dev)
        return raw, self._transform(adapted, dev)

    def _vector(self, v, what: str, N: int, dev: torch.device) -> torch.Tensor:
        if isinstance(v, torch.Tensor):
            _need_device(v, what)
            if v.device != dev:
                raise ValueError(f"{what} must be on {dev} (got {v.device})")
            _f32(v, what)
            t = v.detach()
        else:  # (predictor.py:207-208: np.asarray(x.values, float32))
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(getattr(v, "values", v), dtype=np.float32))).to(dev)
        if tuple(t.shape) != (N,):
            raise ValueError(f"{what} must have shape ({N},), got {tuple(t.shape)}")
        return t.contiguous()

    # ---- the pipeline ----
    def _kan_output(self, raw: torch.Tensor, transform):
        """raw attributes (F, N) -> u (N, O): per chunk one prepare launch and the KAN's L launches."""
        dev = raw.device
        scale, offset, log10 = transform
        F, N = raw.shape
        if N < 1:
            raise ValueError("no reaches")
        net = self._nn
        Fk, H, O, L, G, k = net.arch
        _check_device_f32(net.flat, dev, "parameters", net.flat.shape)
        _check_device_f32(net.consts, dev, "constants", net.consts.shape)
        net._validate_knots()
        lib = _lib.load()
        desc = _lib.KanDesc(Fk, H, O, L, G, k)
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            counts = torch.zeros((3, F), device=dev, dtype=torch.int64) if self.check_distribution else None
            p10, p90 = (self._p10, self._p90) if counts is not None else (None, None)
            rows = min(self.chunk_rows, N)
            x = torch.empty((rows, F), device=dev, dtype=torch.float32)
            work = None
            if L > 1:
                work = torch.empty(int(lib.ddr_kan_work_bytes(C.byref(desc), rows, 0)), device=dev, dtype=torch.uint8)
            u = torch.empty((N, O), device=dev, dtype=torch.float32)
            flat, consts = net.flat.detach(), net.consts
            for c0 in range(0, N, rows):
                r = min(rows, N - c0)
                prepare_attributes(raw[:, c0:c0 + r], scale, offset, log10, self._means, self._stds, p10, p90, counts,
                                   out=x[:r])
                _lib.check(lib.ddr_kan_forward_f32(C.byref(desc), r, x.data_ptr(), flat.data_ptr(), consts.data_ptr(),
                                                   None, u.data_ptr() + 4 * c0 * O, _lib.ptr(work), stream))
        self.last_counts = None
        if counts is not None:
            self._report(counts.cpu().numpy(), N)
        return u

    def _report(self, counts: np.ndarray, total: int) -> None:
        """The reference's two messages (``predictor.py:260-262, 343-350``) from the device counters."""
        self.last_counts = {k: {a: int(counts[i, j]) for j, a in enumerate(self._attribute_names)}
                            for i, k in enumerate(COUNT_NAMES)}
        for j, name in enumerate(self._attribute_names):
            filled, below, above = (int(c) for c in counts[:, j])
            if filled:
                log.info("Attribute %s: filled %d NaN values with training mean", name, filled)
            if below or above:
                r = self._stats_ranges[name]
                log.warning("Attribute %s: %d/%d values below training p10 (%.3f), %d/%d above training p90 (%.3f)",
                            name, below, total, r["p10"], above, total, r["p90"])

    def predict_parameters(self, attributes, source: str = "auto"):
        """``(n, p_spatial, q_spatial)`` in physical units (``_predict_parameters``, ``predictor.py:276-318``), device
        (N,) views of one (3, N) buffer."""
        with torch.no_grad():
            u = self._kan_output(*self._raw(attributes, source, self._ready()))
            out = geometry_predict(u, self._slots, None, None, self._attribute_minimums)
        return out[0], out[1], out[2]

    def predict(self, attributes, discharge, slope, source: str = "auto") -> dict[str, torch.Tensor]:
        """``predictor.py:164-238``: the 11 ``GEOMETRY_OUTPUTS`` per reach, device (N,) views of one (11, N) buffer.

        ``attributes``: a mapping name -> (N,) array-like under MERIT or HydroATLAS names (``source`` as
        ``adapt_attributes``), or a device tensor (F, N) in ``attribute_names`` order (MERIT units; nothing then
        touches the host).  ``discharge`` / ``slope``: (N,) device fp32 tensors, or array-likes that are copied
        over.  They are clamped from below by ``attribute_minimums["discharge" | "slope"]``; a NaN stays NaN and
        gives NaN geometry beside finite n / p_spatial / q_spatial."""
        with torch.no_grad():
            dev = self._ready()
            raw, transform = self._raw(attributes, source, dev)
            N = raw.shape[1]
            Q, S = self._vector(discharge, "discharge", N, dev), self._vector(slope, "slope", N, dev)
            out = geometry_predict(self._kan_output(raw, transform), self._slots, Q, S, self._attribute_minimums)
        return {name: out[i] for i, name in enumerate(GEOMETRY_OUTPUTS)}

    def predict_statistics(self, graph, q_prime_daily: torch.Tensor, attributes, slope, source: str = "auto"):
        """The reference's C4 pipeline (``scripts/geometry_predictor.py:153-229``) for the reaches of ``graph``:
        the KAN's n / p / q, the slope clamped to its minimum, the daily accumulated discharge of ``q_prime_daily``
        (n_days, N) and the per-reach statistics of the geometry -- n / p / q never leave the device.  Returns
        ``geometry_statistics_from_inflow``'s dict of (N,) arrays."""
        from .statistics import geometry_statistics_from_inflow

        dev = self._ready()
        _need_device(q_prime_daily, "q_prime_daily")
        n, p, q = self.predict_parameters(attributes, source)
        s = torch.clamp(self._vector(slope, "slope", n.shape[0], dev), min=self._attribute_minimums.get("slope", 0.001))
        return geometry_statistics_from_inflow(graph, q_prime_daily, n, p, q, s, self._attribute_minimums)
