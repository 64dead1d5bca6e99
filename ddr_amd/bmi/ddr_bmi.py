"""Drop-in for ``ddr.bmi.DdrBmi`` (reference ``src/ddr/bmi/ddr_bmi.py``): the BMI 2.0 model ngen loads in place of
t-route, with the same CSDMS names, units and types, so a realization changes ``python_type`` only.

Everything a coupling interval touches lives on the device: the lateral inflows of this interval and the previous
one (fp64, as the reference holds them), the routing state inside a :class:`~ddr_amd.routing.mmc.MuskingumCunge`,
and the outputs.  Per interval the reference runs a Python loop over every nexus id (``set_value``), and for each
routing sub-step a host interpolation, an upload and one ``route_timestep``; then a PyTorch geometry chain and
three device-to-host copies.  Here

* ``set_value`` of the nexus ids builds, in one launch, which id each segment takes its inflow from
  (``ddr_bmi_nexus_plan``: the reference loop's last-write-wins, by ``atomicMax``); ``set_value`` of the flows is
  one upload and one gather (``ddr_bmi_set_inflow_f64``);
* ``update_until`` is one window launch (``ddr_bmi_window_f32``: the K sub-steps' interpolated inflows, fp64 rounded
  once to fp32 like ``torch.tensor(inflow, dtype=float32)``), ONE routing launch over that window whatever K is --
  the persistent kernel routes K steps from the carried state exactly as K chained ``route_timestep`` calls; the
  cold start is the same window without a state, whose step 0 is the hot start on the raw first row -- one output
  launch (``ddr_bmi_outputs_f32``) and one copy into the pinned arrays ``get_value_ptr`` hands out.

Two deviations from the reference: a ``set_value`` of fewer flows than nexus ids raises ``ValueError`` before
anything is written (the reference fails part-way with ``IndexError``), and a host device raises ``RuntimeError``
(no CPU fallback, as everywhere in this package).
"""

from __future__ import annotations

import logging
import sqlite3
from pathlib import Path
from typing import Any

import numpy as np
import torch

from .. import _lib
from ..ops import route
from ..routing.mmc import MuskingumCunge
from .config import BmiInitConfig

try:  # the abstract base class when it is installed (ngen's Python environment has it)
    from bmipy import Bmi as _Base
except ImportError:
    _Base = object

log = logging.getLogger(__name__)

_ID = "land_surface_water_source__id"
_FLOW = "land_surface_water_source__volume_flow_rate"
_DT = "ngen_dt"
_OUT_ID = "channel_water__id"
_OUT_Q = "channel_exit_water_x-section__volume_flow_rate"
_OUT_V = "channel_water_flow__speed"
_OUT_D = "channel_water__mean_depth"

# t-route's CSDMS names (ddr_bmi.py:47-78)
_INPUT_VAR_NAMES = (_ID, _FLOW, _DT)
_OUTPUT_VAR_NAMES = (_OUT_ID, _OUT_Q, _OUT_V, _OUT_D)
_VAR_UNITS = {_ID: "-", _FLOW: "m3 s-1", _DT: "s", _OUT_ID: "-", _OUT_Q: "m3 s-1", _OUT_V: "m s-1", _OUT_D: "m"}
_VAR_TYPES = {_ID: "int32", _FLOW: "float64", _DT: "int32", _OUT_ID: "int64", _OUT_Q: "float32", _OUT_V: "float32",
              _OUT_D: "float32"}

_NOT_INITIALIZED = "Model not initialized. Call initialize() first."


def _strip_id(s) -> int:
    return int(str(s).replace("cat-", "").replace("wb-", ""))


def _no_dataset_factory(cfg):
    raise RuntimeError(
        "DdrBmi.initialize needs the routing dataclass of the hydrofabric, which this package does not build: set "
        "DdrBmi.dataset_factory = lambda cfg: cfg.geodataset.get_dataset_class(cfg=cfg).routing_dataclass (DDR's "
        "data engine), or call initialize_from(routing_dataclass, spatial_parameters, cfg, ...) directly")


class _Node(dict):
    """A YAML mapping read both ways the routing code reads its config: ``cfg.params.defaults["p_spatial"]``."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key) from None

    def __setattr__(self, key, value) -> None:
        self[key] = value


def _namespace(v):
    if isinstance(v, dict):
        return _Node({k: _namespace(x) for k, x in v.items()})
    return v


def _load_ddr_config(path):
    """DDR's YAML config without Hydra: an OmegaConf node where that is installed (then validated by DDR's own
    ``validate_config`` where that is too), else the plain YAML with the reference's defaults for the ``params``
    and ``kan`` fields it leaves out."""
    try:
        from omegaconf import OmegaConf
    except ImportError:
        import yaml

        from ..geometry.predictor import _KAN_DEFAULT, _PARAMS_DEFAULT

        raw = yaml.safe_load(Path(path).read_text()) or {}
        raw["params"] = {**_PARAMS_DEFAULT, **(raw.get("params") or {})}
        raw["kan"] = {**_KAN_DEFAULT, **(raw.get("kan") or {})}
        raw.setdefault("seed", 0)
        raw.setdefault("data_sources", {})
        return _namespace(raw), False
    return OmegaConf.load(str(path)), True


def _override(derived: torch.Tensor, data: torch.Tensor | None) -> torch.Tensor:
    # mmc.py:74-99 without the host sync of MuskingumCunge's version (the same values)
    if data is None or data.numel() == 0:
        return derived
    return torch.where(torch.isnan(data), derived, data)


def plan_interval(current_time: float, time: float, timestep: float) -> tuple[int, int, float] | None:
    """The scalar bookkeeping of one ``update_until(time)`` (``ddr_bmi.py:264-272, 308``), replayed exactly:
    ``None`` when nothing remains (a no-op that consumes no inflows), else ``(n_steps, executed, new_time)`` -- the
    planned sub-step count (Python's ``round``; the denominator of the linear weights), how many of them run before
    the time check stops the loop, and the time after them (``timestep`` added once per step, in that order)."""
    remaining = time - current_time
    if remaining <= 0.0:
        return None
    n_steps = max(1, round(remaining / timestep))
    executed = 0
    for _ in range(n_steps):
        if current_time >= time - 1e-6:
            break
        current_time += timestep
        executed += 1
    return n_steps, executed, current_time


class DdrBmi(_Base):
    """BMI 2.0 wrapper of the Muskingum-Cunge routing over the whole network (``ddr_bmi.py:81-631``).

    ``dataset_factory(cfg)`` returns the routing dataclass of ``initialize``'s config; the data engine is DDR's,
    so it is a hook to set (see the module docstring); :meth:`initialize_from` takes the dataclass directly."""

    dataset_factory = staticmethod(_no_dataset_factory)

    def __init__(self) -> None:
        self._initialized = False
        self._cold_started = False
        self._bmi_cfg: BmiInitConfig | None = None
        self._cfg: Any = None
        self._device: Any = "cpu"
        self._mc: MuskingumCunge | None = None
        self._spatial_params: dict[str, torch.Tensor] | None = None
        self._num_segments = 0
        self._nexus_to_seg_idx: dict[int, int] = {}
        self._segment_ids: np.ndarray = np.empty(0, dtype=np.int64)
        self._nexus_ids: np.ndarray = np.empty(0, dtype=np.int32)
        self._has_prev_inflow = False
        self._current_time = 0.0
        self._timestep = 3600.0
        self._ngen_dt = 3600
        self._interpolation = "constant"
        self._discharge: np.ndarray = np.empty(0, dtype=np.float32)
        self._velocity: np.ndarray = np.empty(0, dtype=np.float32)
        self._depth: np.ndarray = np.empty(0, dtype=np.float32)
        # device state (initialize_from)
        self._lateral: torch.Tensor | None = None  # fp64 (N): this interval's inflows
        self._prev: torch.Tensor | None = None     # fp64 (N): the previous interval's
        self._src_of_seg: torch.Tensor | None = None  # int32 (N): the nexus id position a segment reads, or -1
        self._keys = self._key_seg = None          # the nexus -> segment table, keys ascending
        self._n_keys = 0
        self._static = None
        self._window: torch.Tensor | None = None   # fp32 (rows, N)
        self._out_dev: torch.Tensor | None = None  # fp32 (3, N): discharge, velocity, depth
        self._out_host: torch.Tensor | None = None  # its pinned copy; the three arrays above are its rows
        self._ids_host: torch.Tensor | None = None
        self._consts = None
        self._p: torch.Tensor | None = None
        self.route_launches = 0  # routing launches issued so far (one per coupling interval)

    # ---- lifecycle ---------------------------------------------------------------------------------------------
    def initialize(self, config_file: str) -> None:
        """``ddr_bmi.py:137-240``: the BMI YAML, DDR's config, the hydrofabric's routing dataclass (through
        :attr:`dataset_factory`), the nexus mapping from the GeoPackage, the KAN run once for the static
        parameters, then :meth:`initialize_from`."""
        import yaml

        from ..nn.kan import kan, load_checkpoint

        bmi_cfg = BmiInitConfig(**yaml.safe_load(Path(config_file).read_text()))
        cfg, omega = _load_ddr_config(bmi_cfg.ddr_config)
        cfg.device = bmi_cfg.device
        cfg.mode = "route"
        if bmi_cfg.hydrofabric_gpkg is not None:
            cfg.data_sources.geospatial_fabric_gpkg = str(bmi_cfg.hydrofabric_gpkg)
        if bmi_cfg.conus_adjacency is not None:
            cfg.data_sources.conus_adjacency = str(bmi_cfg.conus_adjacency)
        if omega:
            try:
                from ddr.validation.configs import validate_config
            except ImportError:
                pass
            else:
                cfg = validate_config(cfg, save_config=False)
        if torch.device(bmi_cfg.device).type != "cuda":
            raise RuntimeError(f"DdrBmi runs on the HIP device only (no CPU fallback): device = {bmi_cfg.device!r}")

        routing_dc = type(self).dataset_factory(cfg)
        if routing_dc is None or routing_dc.adjacency_matrix is None:
            raise RuntimeError("Failed to build routing dataclass from hydrofabric")
        self._num_segments = int(routing_dc.adjacency_matrix.shape[0])
        divide_ids = getattr(routing_dc, "divide_ids", None)
        gpkg = getattr(cfg.data_sources, "geospatial_fabric_gpkg", None)
        if gpkg is None:
            raise RuntimeError("no hydrofabric GeoPackage: set hydrofabric_gpkg in the BMI config or "
                               "data_sources.geospatial_fabric_gpkg in the DDR config")
        mapping = self._build_nexus_mapping(Path(gpkg), divide_ids)

        model = kan(input_var_names=list(cfg.kan.input_var_names),
                    learnable_parameters=list(cfg.kan.learnable_parameters), hidden_size=cfg.kan.hidden_size,
                    num_hidden_layers=cfg.kan.num_hidden_layers, grid=cfg.kan.grid, k=cfg.kan.k,
                    seed=int(getattr(cfg, "seed", 0) or 0), device=bmi_cfg.device)
        load_checkpoint(model, bmi_cfg.kan_checkpoint, bmi_cfg.device)
        model.eval()
        attrs = routing_dc.normalized_spatial_attributes
        if attrs is None:
            raise RuntimeError("No normalized spatial attributes in routing dataclass")
        with torch.no_grad():
            spatial = model(inputs=attrs.to(bmi_cfg.device))
        del model
        self._bmi_cfg = bmi_cfg
        self.initialize_from(routing_dc, spatial, cfg, nexus_to_segment=mapping,
                             timestep_seconds=bmi_cfg.timestep_seconds, interpolation=bmi_cfg.interpolation,
                             device=bmi_cfg.device)

    def initialize_from(self, routing_dataclass, spatial_parameters, cfg, *, nexus_to_segment=None, segment_ids=None,
                        timestep_seconds: float = 3600.0, interpolation: str = "constant", device=None) -> None:
        """The programmatic entry ``initialize`` ends in: a routing dataclass, the KAN's normalised parameters
        (``n``, ``q_spatial``, optionally ``p_spatial``) and DDR's config (``params.*``).

        ``nexus_to_segment``: ``{nexus id: segment index}`` (default: a segment's own id, the reference's fallback);
        ``segment_ids``: the int64 ids ``channel_water__id`` reports (default: the dataclass's ``divide_ids``
        without their ``cat-`` / ``wb-`` prefix, else 0..N-1)."""
        if interpolation not in ("constant", "linear"):
            raise ValueError(f"interpolation must be 'constant' or 'linear', not {interpolation!r}")
        dev = torch.device(device if device is not None else (getattr(cfg, "device", None) or "cuda"))
        if dev.type != "cuda":
            raise RuntimeError(f"DdrBmi runs on the HIP device only (no CPU fallback): device = {str(dev)!r}")
        if not torch.cuda.is_available():
            raise RuntimeError("DdrBmi needs a HIP device and none is available (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        N = int(routing_dataclass.adjacency_matrix.shape[0])
        if N > np.iinfo(np.int32).max:
            raise ValueError("too many segments for int32 indices")
        divide_ids = getattr(routing_dataclass, "divide_ids", None)
        if segment_ids is None:
            segment_ids = (np.arange(N, dtype=np.int64) if divide_ids is None
                           else np.array([_strip_id(s) for s in divide_ids], dtype=np.int64))
        segment_ids = np.ascontiguousarray(segment_ids, dtype=np.int64).reshape(-1)
        if segment_ids.size != N:
            raise ValueError(f"segment_ids has {segment_ids.size} entries for {N} segments")
        if nexus_to_segment is None:
            nexus_to_segment = {int(s): i for i, s in enumerate(segment_ids)}
        keys = np.array(sorted(nexus_to_segment), dtype=np.int64)
        segs = np.array([nexus_to_segment[int(k)] for k in keys], dtype=np.int32)

        lib = _lib.load()
        with torch.cuda.device(dev):
            mc = MuskingumCunge(cfg, device=dev)
            mc.t = torch.tensor(float(timestep_seconds), device=dev)  # ddr_bmi.py:208
            with torch.no_grad():
                mc.setup_inputs(routing_dataclass=routing_dataclass, streamflow=torch.zeros(1, N, device=dev),
                                spatial_parameters=spatial_parameters)
            self._keys = torch.empty(max(1, keys.size), dtype=torch.int64, device=dev)
            self._key_seg = torch.empty(max(1, keys.size), dtype=torch.int32, device=dev)
            _lib.check(lib.ddr_bmi_nexus_table(keys.size, keys.ctypes.data, segs.ctypes.data, N,
                                               self._keys.data_ptr(), self._key_seg.data_ptr(),
                                               _lib.stream_ptr(dev)))
            self._lateral = torch.zeros(N, dtype=torch.float64, device=dev)
            self._prev = torch.zeros(N, dtype=torch.float64, device=dev)
            self._src_of_seg = torch.full((N,), -1, dtype=torch.int32, device=dev)
            self._window = torch.empty((2, N), dtype=torch.float32, device=dev)
            self._out_dev = torch.zeros((3, N), dtype=torch.float32, device=dev)
            self._out_host = torch.zeros((3, N), dtype=torch.float32).pin_memory()
            self._ids_host = torch.from_numpy(segment_ids.copy()).pin_memory()
            self._consts = mc._consts()  # (host copies of the engine's scalars, read once)
            self._p = mc._p_tensor(self._window).reshape(-1).contiguous()
            # the static per-segment inputs of the output kernel: contiguous fp32, as route() makes them
            self._static = tuple(t.detach().to(device=dev, dtype=torch.float32).contiguous()
                                 for t in (mc.n, mc.q_spatial, mc.slope))
        self._n_keys = int(keys.size)
        self._mc = mc
        self._cfg = cfg
        self._device = dev
        self._spatial_params = spatial_parameters
        self._num_segments = N
        self._nexus_to_seg_idx = {int(k): int(v) for k, v in nexus_to_segment.items()}
        self._segment_ids = self._ids_host.numpy()
        self._discharge, self._velocity, self._depth = (self._out_host[i].numpy() for i in range(3))
        self._nexus_ids = np.empty(0, dtype=np.int32)
        self._has_prev_inflow = False
        self._timestep = float(timestep_seconds)
        self._interpolation = interpolation
        self._current_time = 0.0
        self._cold_started = False
        self.route_launches = 0
        self._initialized = True
        log.info("DdrBmi initialized: %d segments, %d nexus mappings, device=%s, dt=%.0fs, interpolation=%s", N,
                 len(self._nexus_to_seg_idx), dev, self._timestep, interpolation)

    def update(self) -> None:
        self.update_until(self._current_time + self._timestep)

    def update_until(self, time: float) -> None:
        """``ddr_bmi.py:246-318``: the scalar bookkeeping on the host as the reference does it, the K sub-steps in
        one routing launch."""
        if not self._initialized or self._mc is None:
            raise RuntimeError(_NOT_INITIALIZED)
        plan = plan_interval(self._current_time, time, self._timestep)
        if plan is None:
            return  # nothing is consumed
        n_steps, K, now = plan
        use_linear = self._interpolation == "linear" and self._has_prev_inflow and n_steps > 1
        mc, N, dev = self._mc, self._num_segments, self._device
        lib = _lib.load()
        with torch.no_grad(), torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            if K > 0:
                if self._window.shape[0] < K + 1:
                    self._window = torch.empty((K + 1, N), dtype=torch.float32, device=dev)
                window = self._window[:K + 1]
                _lib.check(lib.ddr_bmi_window_f32(N, K, n_steps, int(use_linear), self._prev.data_ptr(),
                                                  self._lateral.data_ptr(), window.data_ptr(), N, stream))
                # rows 0..K-1 from the carried state are K chained route_timestep calls; without a state the
                # launch's step 0 is the hot start on the raw row 0 (ddr_bmi.py:284-304)
                q0 = mc._discharge_t if self._cold_started else None
                _, q_last, tw, ss = route(mc._graph, window, mc.n, mc.q_spatial, self._p, mc.length, mc.slope,
                                          mc.x_storage, q0=q0, consts=self._consts, math=mc.math,
                                          exact_adjoint=mc._exact_adjoint)
                self.route_launches += 1
                mc._discharge_t = q_last
                mc.top_width = _override(tw, mc._data_top_width)
                mc.side_slope = _override(ss, mc._data_side_slope)
                self._cold_started = True
            else:  # (a target within 1e-6 s: no step runs, the inflows still rotate)
                self._prev.copy_(self._lateral)
                self._lateral.zero_()
            if self._cold_started:
                n_, qs_, s0_ = self._static
                q_t, tw_, z_ = (t.contiguous() for t in (mc._discharge_t, mc.top_width, mc.side_slope))
                _lib.check(lib.ddr_bmi_outputs_f32(
                    N, q_t.data_ptr(), n_.data_ptr(), qs_.data_ptr(), self._p.data_ptr(),
                    0 if self._p.numel() == 1 else 1, s0_.data_ptr(), tw_.data_ptr(), z_.data_ptr(),
                    self._consts.depth_lb, self._consts.bottom_width_lb, self._out_dev.data_ptr(), N, stream))
                self._out_host.copy_(self._out_dev, non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()
        self._current_time = now
        self._has_prev_inflow = True

    def finalize(self) -> None:
        self._mc = None
        self._spatial_params = None
        self._lateral = self._prev = self._src_of_seg = self._window = self._out_dev = None
        self._keys = self._key_seg = self._p = self._static = None
        self._initialized = False
        log.info("DdrBmi finalized")

    # ---- variable info -----------------------------------------------------------------------------------------
    def get_component_name(self) -> str:
        return "DDR-MuskingumCunge"

    def get_input_item_count(self) -> int:
        return len(_INPUT_VAR_NAMES)

    def get_output_item_count(self) -> int:
        return len(_OUTPUT_VAR_NAMES)

    def get_input_var_names(self) -> tuple[str, ...]:
        return _INPUT_VAR_NAMES

    def get_output_var_names(self) -> tuple[str, ...]:
        return _OUTPUT_VAR_NAMES

    def get_var_grid(self, name: str) -> int:
        return 0

    def get_var_type(self, name: str) -> str:
        return _VAR_TYPES.get(name, "float64")

    def get_var_units(self, name: str) -> str:
        return _VAR_UNITS.get(name, "-")

    def get_var_itemsize(self, name: str) -> int:
        return int(np.dtype(self.get_var_type(name)).itemsize)

    def get_var_nbytes(self, name: str) -> int:
        raise NotImplementedError

    def get_var_location(self, name: str) -> str:
        return "node"

    # ---- time --------------------------------------------------------------------------------------------------
    def get_current_time(self) -> float:
        return self._current_time

    def get_start_time(self) -> float:
        return 0.0

    def get_end_time(self) -> float:
        return float("inf")  # ngen ends the simulation

    def get_time_units(self) -> str:
        return "s"

    def get_time_step(self) -> float:
        return self._timestep

    # ---- getters and setters -----------------------------------------------------------------------------------
    def get_value(self, name: str, dest: np.ndarray) -> np.ndarray:
        dest[:] = self.get_value_ptr(name)[: len(dest)]
        return dest

    def get_value_ptr(self, name: str) -> np.ndarray:
        """The variable's persistent (pinned) array: the same object for the model's lifetime, refilled in place by
        every ``update_until``."""
        if name == _OUT_Q:
            return self._discharge
        if name == _OUT_ID:
            return self._segment_ids
        if name == _OUT_V:
            return self._velocity
        if name == _OUT_D:
            return self._depth
        raise ValueError(f"Unknown output variable: {name}")

    def get_value_at_indices(self, name: str, dest: np.ndarray, inds: np.ndarray) -> np.ndarray:
        dest[:] = self.get_value_ptr(name)[inds]
        return dest

    def _gather(self, sel: torch.Tensor, flows: np.ndarray) -> None:
        dev = self._device
        with torch.cuda.device(dev):
            d_flows = torch.from_numpy(flows).to(dev)
            _lib.check(_lib.load().ddr_bmi_set_inflow_f64(self._num_segments, sel.data_ptr(), flows.size,
                                                          d_flows.data_ptr(), self._lateral.data_ptr(),
                                                          _lib.stream_ptr(dev)))

    def set_value(self, name: str, src: np.ndarray) -> None:
        """``ddr_bmi.py:417-438``."""
        src = np.asarray(src)
        if name == _FLOW:
            if not self._initialized:
                return  # (no segments yet: the reference writes nothing either)
            M = len(self._nexus_ids)
            flat = src.reshape(-1)
            if M > 0 and len(src) > 0:
                if flat.size < M:
                    raise ValueError(f"{name}: {flat.size} flows for {M} nexus ids")
                self._gather(self._src_of_seg, np.ascontiguousarray(flat[:M], dtype=np.float64))
            else:
                n = min(flat.size, self._num_segments)
                if n:
                    self._lateral[:n].copy_(torch.from_numpy(np.ascontiguousarray(flat[:n], dtype=np.float64)))
        elif name == _ID:
            self._nexus_ids = src.astype(np.int32).flatten()
            if self._initialized:
                dev, M = self._device, self._nexus_ids.size
                with torch.cuda.device(dev):
                    ids = torch.from_numpy(self._nexus_ids).to(dev) if M else None
                    _lib.check(_lib.load().ddr_bmi_nexus_plan(
                        M, _lib.ptr(ids), self._n_keys, self._keys.data_ptr(), self._key_seg.data_ptr(),
                        self._num_segments, self._src_of_seg.data_ptr(), _lib.stream_ptr(dev)))
        elif name == _DT:
            self._ngen_dt = int(src.flat[0])
        else:
            log.debug("Unknown input variable ignored: %s", name)  # BMI convention: no error

    def set_value_at_indices(self, name: str, inds: np.ndarray, src: np.ndarray) -> None:
        """``ddr_bmi.py:440-447``: indices >= N are ignored, a segment written twice keeps the last value."""
        if name != _FLOW:
            log.debug("set_value_at_indices not supported for: %s", name)
            return
        if not self._initialized:
            return
        N = self._num_segments
        idx = np.asarray(inds).reshape(-1).astype(np.int64)
        vals = np.asarray(src).reshape(-1)
        if vals.size < idx.size:
            raise ValueError(f"{name}: {vals.size} values for {idx.size} indices")
        if idx.size == 0:
            return
        if (idx < -N).any():
            raise IndexError(f"index {int(idx.min())} is out of bounds for {N} segments")
        keep = idx < N
        pos = np.nonzero(keep)[0].astype(np.int32)
        sel = np.full(N, -1, dtype=np.int32)
        np.maximum.at(sel, idx[keep] % N, pos)  # (a negative index counts from the end, as NumPy's does)
        self._gather(torch.from_numpy(sel).to(self._device), np.ascontiguousarray(vals[:idx.size], dtype=np.float64))

    # ---- grid (an unstructured network) -------------------------------------------------------------------------
    def get_grid_rank(self, grid: int) -> int:
        return 1

    def get_grid_size(self, grid: int) -> int:
        return self._num_segments

    def get_grid_type(self, grid: int) -> str:
        return "unstructured"

    def get_grid_shape(self, grid: int, shape: np.ndarray) -> np.ndarray:
        shape[0] = self._num_segments
        return shape

    def get_grid_spacing(self, grid: int, spacing: np.ndarray) -> np.ndarray:
        raise NotImplementedError("Spacing not defined for unstructured grid")

    def get_grid_origin(self, grid: int, origin: np.ndarray) -> np.ndarray:
        raise NotImplementedError("Origin not defined for unstructured grid")

    def get_grid_x(self, grid: int, x: np.ndarray) -> np.ndarray:
        raise NotImplementedError("Grid coordinates not available")

    def get_grid_y(self, grid: int, y: np.ndarray) -> np.ndarray:
        raise NotImplementedError("Grid coordinates not available")

    def get_grid_z(self, grid: int, z: np.ndarray) -> np.ndarray:
        raise NotImplementedError("Grid coordinates not available")

    def get_grid_node_count(self, grid: int) -> int:
        return self._num_segments

    def get_grid_edge_count(self, grid: int) -> int:
        if self._mc is not None and self._mc.network is not None:
            return int(self._mc.network._nnz())
        return 0

    def get_grid_face_count(self, grid: int) -> int:
        return 0

    def get_grid_edge_nodes(self, grid: int, edge_nodes: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    def get_grid_face_edges(self, grid: int, face_edges: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    def get_grid_face_nodes(self, grid: int, face_nodes: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    def get_grid_nodes_per_face(self, grid: int, nodes_per_face: np.ndarray) -> np.ndarray:
        raise NotImplementedError

    # ---- helpers -----------------------------------------------------------------------------------------------
    def _build_nexus_mapping(self, gpkg_path, divide_ids) -> dict[int, int]:
        """``{nexus id: segment index}`` from the GeoPackage's ``flowpaths`` table (``ddr_bmi.py:508-575``): the
        flowpath ``wb-<id>`` whose ``toid`` is ``nex-<nexus>`` drains into that nexus.  Segments are numbered by
        ``divide_ids`` (prefix stripped), or 0..N-1 without them; a file without a readable ``flowpaths`` table
        gives the identity mapping (a segment's id is its nexus id)."""
        if divide_ids is not None:
            index_of = {_strip_id(d): i for i, d in enumerate(divide_ids)}
        else:
            index_of = {i: i for i in range(self._num_segments)}
        try:
            con = sqlite3.connect(str(gpkg_path))
            try:
                rows = con.execute("SELECT id, toid FROM flowpaths WHERE toid LIKE 'nex-%'").fetchall()
            finally:
                con.close()
        except (sqlite3.OperationalError, sqlite3.DatabaseError):
            log.warning("Could not read flowpaths table from %s; falling back to identity mapping", gpkg_path)
            return dict(index_of)
        mapping: dict[int, int] = {}
        for flowpath, nexus in rows:
            flowpath = str(flowpath)
            if not flowpath.startswith(("wb-", "cat-")):
                continue
            seg = index_of.get(_strip_id(flowpath))
            if seg is not None:
                mapping[int(str(nexus).replace("nex-", ""))] = seg
        log.info("Built nexus mapping from GeoPackage: %d entries from %s", len(mapping), Path(gpkg_path).name)
        return mapping
