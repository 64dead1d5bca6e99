"""Device-resident catchment attributes, flowpath tensors and flow_scale, gathered per batch (``csrc/attrs.hip``).

The reference builds them in ``collate_fn``, on the host, once per batch: ``_get_attributes`` and
``_build_common_tensors`` (``src/ddr/geodatazoo/merit.py:92-124, 273-319``, ``lynker_hydrofabric.py:105-135,
302-354``) -- a Python loop of dict lookups over the batch's ids, an xarray ``isel(...).compute()``, a NaN fill, a
z-score and a transpose, fancy-indexed reads of the flowpath arrays with fills -- and ``build_flow_scale_tensor``
(``io/readers.py:299-362``), a Python loop over the batch's gauges; then an upload.  Here

* :class:`AttributeStore` -- the attribute store aligned to CONUS order once (a CONUS reach the store lacks is a NaN
  row) and uploaded together with the flowpath arrays; :meth:`AttributeStore.batch` produces every per-reach tensor of
  a batch from ``DeviceBatch.active`` alone, in one launch (two more when an attribute's mean is NaN, one more for
  the gauges' ``flow_scale``);
* :class:`FlowScaleTable` -- one factor per row of ``read_gage_info()``'s dict, computed on the host once;
* :class:`AttributeBatch` -- the result, and :meth:`AttributeBatch.routing_dataclass`, the namespace ``dmc`` reads.

The conventions are those of :mod:`ddr_amd.io.stores`: NumPy input is uploaded once, a device tensor is kept as it
is; there is no CPU fallback (a host store raises ``RuntimeError``); gathers run on the current stream and never
synchronise with the host; values are copied as bits; an index outside the store is a missing divide, never an
address.  The host halves (:func:`align_attributes`, :func:`flowpath_fill`, :func:`flow_scale_factors`) need no
device.
"""

from __future__ import annotations

import ctypes as C
import math
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib
from .stores import RowIndex, _device_of, pad_gage_ids

FLOWPATH = ("length", "slope", "x", "top_width", "side_slope")  # the order of ddr_flowpath
MERIT_X = 0.3  # merit.py:313-315
ROW_ALIGN = 4  # the aligned table's rows are padded to 16 bytes


def padded_stride(n_attrs: int) -> int:
    """Elements between two rows of the aligned table: ``n_attrs`` rounded up to 16 bytes."""
    return -(-int(n_attrs) // ROW_ALIGN) * ROW_ALIGN


def align_attributes(attributes: np.ndarray, attribute_ids, conus_ids, row_stride: int | None = None) -> np.ndarray:
    """The attribute store in CONUS order, reach-major: float32 ``(n_conus, row_stride)`` whose row ``i`` holds the
    ``A`` attributes of ``conus_ids[i]`` (bits copied) and NaN padding; a CONUS reach the store lacks is a NaN row.
    ``attributes`` is ``(A, n_store)`` as ``ds[names].to_array().values``; a repeated store id resolves to its last
    row, as in the reference's ``id_to_index`` dict."""
    A, n_store = attributes.shape
    stride = padded_stride(A) if row_stride is None else int(row_stride)
    if stride < A:
        raise ValueError(f"row_stride {stride} is shorter than a row of {A} attributes")
    rows = RowIndex(attribute_ids).lookup(conus_ids)
    table = np.full((rows.size, stride), np.nan, np.float32)
    have = rows >= 0
    table[have, :A] = np.ascontiguousarray(attributes.T)[rows[have]]
    return table


def flowpath_fill(values: np.ndarray) -> np.float32:
    """The reference's fill value of a flowpath array (``naninfmean``, readers.py:365-379, cast as at
    merit.py:76-80): the mean of its finite entries in the array's own dtype, then float32; NaN without any."""
    values = np.asarray(values)
    finite = values[np.isfinite(values)]
    return np.float32(np.mean(finite) if len(finite) > 0 else np.nan)


def _area_factor(drain, comid_drain, comid_unit) -> float:
    """The share of q' a gauge partway through its catchment keeps (``compute_flow_scale_factor``,
    readers.py:259-296); 1.0 for degenerate input."""
    if math.isnan(drain) or math.isnan(comid_drain) or math.isnan(comid_unit) or comid_unit <= 0:
        return 1.0
    short = comid_drain - drain
    if short <= 0 or short >= comid_unit:
        return 1.0
    return (comid_unit - short) / comid_unit


def flow_scale_factors(gage_dict) -> tuple[np.ndarray, np.ndarray] | None:
    """``(factors float32 (n,), skip bool (n,))`` for the rows of ``read_gage_info()``'s dict, or ``None`` when it
    has neither ``FLOW_SCALE`` nor the raw area columns (readers.py:347-348: the batch gets ones).  ``FLOW_SCALE`` is
    taken as it is, a float NaN marking "keep 1.0" (readers.py:340-342); otherwise the factor comes from
    ``DRAIN_SQKM``, ``COMID_DRAIN_SQKM`` and ``COMID_UNITAREA_SQKM`` and is always written.  Values are rounded to
    float32 as an assignment into the reference's float32 tensor rounds them."""
    n = len(gage_dict["STAID"])
    skip = np.zeros(n, bool)
    if "FLOW_SCALE" in gage_dict:
        values = list(gage_dict["FLOW_SCALE"])
        for i, v in enumerate(values):
            if isinstance(v, float) and math.isnan(v):
                skip[i], values[i] = True, 1.0
        return np.array(values, dtype=np.float64).astype(np.float32), skip
    if "COMID_DRAIN_SQKM" not in gage_dict or "COMID_UNITAREA_SQKM" not in gage_dict:
        return None
    factors = [_area_factor(d, c, u) for d, c, u in zip(gage_dict["DRAIN_SQKM"], gage_dict["COMID_DRAIN_SQKM"],
                                                        gage_dict["COMID_UNITAREA_SQKM"])]
    return np.array(factors, dtype=np.float64).astype(np.float32), skip


def _is_scalar(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating))


def _check_float32(values, name: str, ndim: int) -> None:
    if not isinstance(values, (np.ndarray, torch.Tensor)):
        raise TypeError(f"{name} must be a NumPy array or a torch tensor")
    if values.dtype not in (np.float32, torch.float32):
        raise ValueError(f"{name} must be float32, not {values.dtype}")
    if values.ndim != ndim:
        raise ValueError(f"{name} must be {ndim}-D")
    if isinstance(values, torch.Tensor) and not values.is_cuda:
        raise RuntimeError(f"{name} is a host tensor: the forcing stores live on the HIP device only (no CPU "
                           "fallback)")


def _to_device(values: np.ndarray, device) -> torch.Tensor:
    with warnings.catch_warnings():  # (a read-only array, e.g. a memory map: it is only read)
        warnings.simplefilter("ignore", UserWarning)
        return torch.from_numpy(np.ascontiguousarray(values)).to(device)


class FlowScaleTable:
    """The flow_scale factor of every gauge of ``read_gage_info()``'s dict on the device (:func:`flow_scale_factors`).
    ``rows(staids)`` looks a batch's gauges up (ids keyed zero-filled to 8 digits, readers.py:336) for
    ``AttributeStore.batch(..., scale_rows=rows)``."""

    def __init__(self, gage_dict, device="cuda") -> None:
        self.index = RowIndex(pad_gage_ids(gage_dict["STAID"]))
        host = flow_scale_factors(gage_dict)
        self.device = _device_of(device)
        self.factors = self.skip = None
        if host is not None:
            self.factors = _to_device(host[0], self.device)
            self.skip = _to_device(host[1].astype(np.uint8), self.device) if host[1].any() else None

    def __len__(self) -> int:
        return len(self.index)

    def rows(self, staids) -> torch.Tensor:
        """int32 ``(G,)`` on the device: the dict row of every gauge, -1 for an unknown one."""
        return torch.from_numpy(self.index.lookup(pad_gage_ids(staids))).to(self.device)


class _RoutingBatch:
    """The fields ``MuskingumCunge._set_network_context`` reads; ``divide_ids`` (host, one copy of ``active``) is
    resolved on first use."""

    def __init__(self, store: "AttributeStore", active: torch.Tensor, **fields) -> None:
        self.__dict__.update(fields)
        self._store, self._active = store, active

    @property
    def divide_ids(self) -> np.ndarray:
        ids = self.__dict__.get("_divide_ids")
        if ids is None:
            ids = self.__dict__["_divide_ids"] = self._store.conus_ids[self._active.cpu().numpy()]
        return ids


@dataclass
class AttributeBatch:
    """What the reference's ``_build_common_tensors`` and ``build_flow_scale_tensor`` give for a batch: float32 device
    tensors, contiguous, in the reference's layouts."""
    spatial_attributes: torch.Tensor             # (A, N)
    normalized_spatial_attributes: torch.Tensor  # (N, A)
    length: torch.Tensor                         # (N,)
    slope: torch.Tensor
    x: torch.Tensor
    top_width: torch.Tensor                      # (N,), or empty (MERIT)
    side_slope: torch.Tensor
    flow_scale: torch.Tensor | None              # (N,), None without gauges
    active: torch.Tensor
    store: "AttributeStore"

    def routing_dataclass(self, db, dates=None, observations=None):
        """The batch as the namespace ``dmc(routing_dataclass=...)`` takes, for ``db`` the :class:`DeviceBatch` whose
        ``active`` made this batch: the adjacency is the batch's CSR as a sparse tensor on the device."""
        n = int(self.active.numel())
        adjacency = torch.sparse_csr_tensor(db.crow, db.col.to(torch.int64),
                                            torch.ones(db.col.numel(), device=db.col.device, dtype=torch.float32),
                                            size=(n, n))
        return _RoutingBatch(self.store, self.active, adjacency_matrix=adjacency, outflow_idx=db.outflow_idx(),
                             gage_catchment=list(db.gage_idx), length=self.length, slope=self.slope, x=self.x,
                             top_width=self.top_width, side_slope=self.side_slope, flow_scale=self.flow_scale,
                             spatial_attributes=self.spatial_attributes,
                             normalized_spatial_attributes=self.normalized_spatial_attributes, dates=dates,
                             observations=observations)


class AttributeStore:
    """The catchment attributes and flowpath arrays of a dataset on the device.

    ``attributes`` float32 ``(A, n_store)`` as ``ds[input_var_names].to_array().values`` (attribute-major, NaN for a
    missing value) with ``attribute_ids`` its columns' ids; ``means`` / ``stds`` float32 ``(A,)``, rows 2 and 3 of the
    reference's statistics frame; ``conus_ids`` is ``conus_adjacency["order"]``; ``length``, ``slope`` and, for the
    Lynker hydrofabric, ``top_width``, ``side_slope`` and ``x`` are arrays in CONUS order (MERIT: ``x`` the scalar 0.3
    and no ``top_width`` / ``side_slope``: the batch gets empty tensors, merit.py:313-317).  NumPy input is aligned on
    the host and uploaded once; device tensors are aligned on the device and the flowpath tensors kept as they are.
    :meth:`from_aligned` takes a table that is already in CONUS order."""

    def __init__(self, attributes, attribute_ids, means, stds, conus_ids, length, slope, top_width=None,
                 side_slope=None, x=MERIT_X, device="cuda", row_stride: int | None = None,
                 scale_table: "FlowScaleTable | None" = None) -> None:
        _check_float32(attributes, "attributes", 2)
        A = int(attributes.shape[0])
        conus_ids = np.asarray(conus_ids)
        if conus_ids.ndim != 1:
            raise ValueError("conus_ids must be 1-D")
        if len(np.asarray(attribute_ids).reshape(-1)) != attributes.shape[1]:
            raise ValueError(f"attributes has {attributes.shape[1]} columns for "
                             f"{len(np.asarray(attribute_ids).reshape(-1))} ids")
        self._check_common(A, means, stds, len(conus_ids), length, slope, top_width, side_slope, x)
        if isinstance(attributes, np.ndarray):
            device = _device_of(device)
            table = _to_device(align_attributes(attributes, attribute_ids, conus_ids, row_stride), device)
        else:
            device = attributes.device
            stride = padded_stride(A) if row_stride is None else int(row_stride)
            if stride < A:
                raise ValueError(f"row_stride {stride} is shorter than a row of {A} attributes")
            rows = torch.from_numpy(RowIndex(attribute_ids).lookup(conus_ids)).to(device)
            table = torch.full((len(conus_ids), stride), float("nan"), device=device, dtype=torch.float32)
            have = (rows >= 0).nonzero().reshape(-1)
            table[have, :A] = attributes.detach().T.index_select(0, rows[have].long())
        self._setup(table, A, means, stds, conus_ids, length, slope, top_width, side_slope, x, device)
        self.scale_table = scale_table

    @classmethod
    def from_aligned(cls, table, means, stds, conus_ids, length, slope, top_width=None, side_slope=None, x=MERIT_X,
                     device="cuda", scale_table: "FlowScaleTable | None" = None) -> "AttributeStore":
        """A store over ``table``, float32 ``(n_conus, A)`` already in CONUS order with a reach's attributes on the
        inner axis (:func:`align_attributes`): a NumPy array is uploaded once, a device tensor (any row stride,
        ``stride(1) == 1``) is kept as it is."""
        self = cls.__new__(cls)
        _check_float32(table, "table", 2)
        A = int(len(np.asarray(means).reshape(-1))) if not isinstance(means, torch.Tensor) else int(means.numel())
        conus_ids = np.asarray(conus_ids)
        if table.shape[0] != len(conus_ids):
            raise ValueError(f"table has {table.shape[0]} rows for {len(conus_ids)} ids")
        if table.shape[1] < A:
            raise ValueError(f"table has {table.shape[1]} columns for {A} attributes")
        self._check_common(A, means, stds, len(conus_ids), length, slope, top_width, side_slope, x)
        if isinstance(table, np.ndarray):
            device = _device_of(device)
            table = _to_device(table, device)
        else:
            device = table.device
            if table.shape[1] > 1 and table.stride(1) != 1:
                raise ValueError("table must hold the attributes on the inner axis (stride(1) == 1)")
            if table.shape[0] > 1 and table.stride(0) < A:
                raise ValueError("table's rows overlap (stride(0) < A)")
            table = table.detach()
        self._setup(table, A, means, stds, conus_ids, length, slope, top_width, side_slope, x, device)
        self.scale_table = scale_table
        return self

    @staticmethod
    def _check_common(A, means, stds, n_conus, length, slope, top_width, side_slope, x) -> None:
        if not 1 <= A <= _lib.ATTR_MAX_FEATURES:
            raise ValueError(f"1 <= A <= {_lib.ATTR_MAX_FEATURES} attributes, not {A}")
        for name, v in (("means", means), ("stds", stds)):
            _check_float32(v, name, 1)
            if v.shape[0] != A:
                raise ValueError(f"{name} has {v.shape[0]} entries for {A} attributes")
        if (top_width is None) != (side_slope is None):
            raise ValueError("top_width and side_slope go together")
        arrays = [("length", length), ("slope", slope), ("top_width", top_width), ("side_slope", side_slope)]
        if not _is_scalar(x):
            arrays.append(("x", x))
        for name, v in arrays:
            if v is None:
                continue
            if not isinstance(v, (np.ndarray, torch.Tensor)):
                raise TypeError(f"{name} must be a NumPy array or a torch tensor")
            # (a float64 zarr array is taken too: its fill value is computed in float64, its values are cast once)
            if not (isinstance(v, np.ndarray) and v.dtype == np.float64):
                _check_float32(v, name, 1)
            if v.ndim != 1 or v.shape[0] != n_conus:
                raise ValueError(f"{name} must hold one value per CONUS reach ({n_conus}), not {tuple(v.shape)}")

    def _setup(self, table, A, means, stds, conus_ids, length, slope, top_width, side_slope, x, device) -> None:
        self.device = device
        self.table = table
        self.n_attrs = A
        self.n_conus = int(table.shape[0])
        self.conus_ids = conus_ids
        self._stride = max(int(table.stride(0)), A) if self.n_conus > 1 else max(int(table.shape[1]), A)

        def small(v):
            return _to_device(v, device) if isinstance(v, np.ndarray) else v.detach().to(device).contiguous()

        self.means, self.stds = small(means), small(stds)
        host_means = means if isinstance(means, np.ndarray) else means.detach().cpu().numpy()
        # the attributes whose mean is NaN: fill_nans leaves their NaN, the per-batch NaN-mean replaces it
        flagged = np.flatnonzero(np.isnan(host_means)).astype(np.int32)
        self.flagged = _to_device(flagged, device) if flagged.size else None
        self._work_bytes = int(_lib.load().ddr_feed_attr_mean_work_bytes(int(flagged.size))) if flagged.size else 0

        self.fills, self.arrays = {}, {}
        for name, v in zip(FLOWPATH, (length, slope, x, top_width, side_slope)):
            if v is None:
                continue
            if _is_scalar(v):
                self.fills[name], self.arrays[name] = np.float32(v), None
                continue
            host = v if isinstance(v, np.ndarray) else v.detach().cpu().numpy()
            self.fills[name] = flowpath_fill(host)
            if isinstance(v, np.ndarray):
                with np.errstate(over="ignore"):
                    v = _to_device(v.astype(np.float32, copy=False), device)
            else:
                v = v.detach().contiguous()
                if v.device != device:
                    raise ValueError(f"{name} is on {v.device}, the table on {device}")
            self.arrays[name] = v

    def _check_index(self, t, name: str, n: int | None = None) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor")
        if t.dtype != torch.int32:
            raise ValueError(f"{name} must be int32, not {t.dtype}")
        if t.dim() != 1:
            raise ValueError(f"{name} must be 1-D")
        if not t.is_cuda:
            raise RuntimeError(f"{name} is a host tensor: the feed runs on the HIP device only (no CPU fallback)")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, the store on {self.device}")
        if n is not None and t.numel() != n:
            raise ValueError(f"{name} has {t.numel()} entries for {n} gauges")
        return t.contiguous()

    def batch(self, active: torch.Tensor, gage_c: torch.Tensor | None = None,
              scale_rows: torch.Tensor | None = None, scale_table: FlowScaleTable | None = None) -> AttributeBatch:
        """Every per-reach tensor of the batch whose reaches are the CONUS indices ``active`` (int32 ``(N,)`` on the
        store's device, e.g. ``DeviceBatch.active``).  With ``gage_c`` (``DeviceBatch.gage_c``) the batch carries
        ``flow_scale``: ones, and for ``scale_rows = table.rows(staids)`` (``table`` the :class:`FlowScaleTable` given
        to the store, assigned to ``store.scale_table`` or passed as ``scale_table``) the gauges' factors, the last
        gauge of a segment in batch order winning."""
        active = self._check_index(active, "active")
        scale_table = self.scale_table if scale_table is None else scale_table
        if scale_rows is not None and scale_table is None:
            raise ValueError("scale_rows needs the FlowScaleTable they index: AttributeStore(..., scale_table=table) "
                             "or batch(..., scale_table=table)")
        if scale_rows is not None and gage_c is None:
            raise ValueError("scale_rows needs gage_c")
        G = 0
        if gage_c is not None:
            gage_c = self._check_index(gage_c, "gage_c")
            G = int(gage_c.numel())
            if scale_rows is not None:
                scale_rows = self._check_index(scale_rows, "scale_rows", G)
        N, A = int(active.numel()), self.n_attrs
        lib = _lib.load()
        with torch.cuda.device(self.device):
            f32 = dict(device=self.device, dtype=torch.float32)
            stream = _lib.stream_ptr(self.device)
            spatial = torch.empty((A, N), **f32)
            normalized = torch.empty((N, A), **f32)
            out = {name: torch.empty((N,), **f32) for name in self.fills}
            flow_scale = torch.empty((N,), **f32) if gage_c is not None else None
            fill = self.means
            if self.flagged is not None and N > 0:
                fill = self.means.clone()
                work = torch.empty((self._work_bytes // 8,), device=self.device, dtype=torch.int64)
                _lib.check(lib.ddr_feed_attr_mean_f32(
                    self.table.data_ptr(), self._stride, self.n_conus, A, active.data_ptr(), N,
                    self.flagged.data_ptr(), int(self.flagged.numel()), fill.data_ptr(), work.data_ptr(),
                    self._work_bytes, stream))
            path = _lib.Flowpath()
            for k, name in enumerate(FLOWPATH):
                if name in self.fills:
                    path.src[k] = _lib.ptr(self.arrays[name])
                    path.out[k] = out[name].data_ptr()
                    path.fill[k] = float(self.fills[name])
            _lib.check(lib.ddr_feed_attributes_f32(
                self.table.data_ptr(), self._stride, self.n_conus, A, active.data_ptr(), N, fill.data_ptr(),
                self.means.data_ptr(), self.stds.data_ptr(), spatial.data_ptr(), normalized.data_ptr(), C.byref(path),
                _lib.ptr(flow_scale), stream))
            if scale_rows is not None and scale_table.factors is not None and G > 0 and N > 0:
                winner = torch.empty((N,), device=self.device, dtype=torch.int32)
                _lib.check(lib.ddr_feed_flow_scale_f32(
                    gage_c.data_ptr(), scale_rows.data_ptr(), G, scale_table.factors.data_ptr(),
                    _lib.ptr(scale_table.skip), int(scale_table.factors.numel()), N, winner.data_ptr(),
                    flow_scale.data_ptr(), stream))
            empty = torch.empty(0)  # (merit.py:316-317)
        return AttributeBatch(spatial, normalized, out["length"], out["slope"], out["x"],
                              out.get("top_width", empty), out.get("side_slope", empty), flow_scale, active, self)

    def __repr__(self) -> str:
        return (f"AttributeStore({self.n_conus} reaches x {self.n_attrs} attributes, row stride {self._stride}, "
                f"{'Lynker' if 'top_width' in self.fills else 'MERIT'} flowpaths, {self.device})")
