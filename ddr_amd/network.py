"""The network build: a raw flowpath table, in any row order, to the contract every other entry point starts from.

That contract is the engine's ``conus_adjacency``: a strictly lower-triangular COO (row = downstream reach), upstream
reaches numbered first, dendritic (:mod:`ddr_amd.graph`).  The reference produces it offline with rustworkx, polars and
geopandas -- ``create_matrix`` of ``engine/src/ddr_engine/merit/build.py:20-107`` (``COMID``, ``up1..up4``) and of
``lynker_hydrofabric/io.py:60-154`` (flowpaths and nexus points): a topological sort, cycle removal, renumbering.
:class:`Network` does it from ``(id, to_id)`` alone, on the device (``csrc/network.hip``) or in the host twin
(``csrc/network_host.cpp``, no GPU), with identical bits from both:

1. ``down[i]`` is the row of ``to_ids[i]`` in ``ids``; a ``to_id`` that names no row (0, a negative value, any foreign
   id) makes the reach an outlet.  Ids are distinct int64 over the full range; a duplicate is refused.
2. A reach on a cycle of ``down`` (a self-loop counts) is dropped, a kept reach that drained into one becomes an outlet,
   reaches upstream of a cycle are kept.
3. The new index sorts the kept reaches by (basin ascending, distance to the outlet descending, row ascending), the
   basin being the rank of the outlet's row among all outlets' rows: basins stay contiguous and every edge has
   ``row > col``.

The order is this project's, not rustworkx's: any topological order satisfies the contract, and nothing that depends
on the particular order is promised equal to the engine's stores.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_I64_MIN = -(1 << 63)


def _tensor(a, device=None):
    """``a`` as a flat-or-2-D int64 torch tensor on ``device`` (None: where it is, host arrays on the CPU)."""
    import torch

    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if a.size and a.dtype.kind not in "iu":  # (an empty list arrives as float64)
            raise TypeError(f"ids must be integers, not {a.dtype}")
        a = np.ascontiguousarray(a, dtype=np.int64)
        a = torch.from_numpy(a if a.flags.writeable else a.copy())  # (torch takes no read-only array)
    elif a.dtype.is_floating_point or a.dtype == torch.bool:
        raise TypeError(f"ids must be integers, not {a.dtype}")
    a = a.to(torch.int64)
    return a if device is None else a.to(device)


def _array(a) -> np.ndarray:
    """``a`` (host data) as a flat contiguous int64 NumPy array."""
    import torch

    if isinstance(a, torch.Tensor):
        return _tensor(a).reshape(-1).contiguous().numpy()
    a = np.asarray(a).reshape(-1)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError(f"ids must be integers, not {a.dtype}")
    return np.ascontiguousarray(a, dtype=np.int64)


def _device_of(device, *arrays):
    import torch

    if device is not None:
        dev = torch.device(device)
        return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return None


def lookup(ids, queries, device=None):
    """int32 row of every query id in ``ids`` (distinct), -1 when absent: a NumPy array from the host twin
    (``device=None`` and host input), else a device tensor (``ddr_network_lookup_i64``)."""
    import torch

    dev = _device_of(device, ids, queries)
    lib = _lib.load()
    if dev is None:
        t, q = _array(ids), _array(queries)
        pos = np.empty(len(q), np.int32)
        _lib.check(lib.ddr_network_lookup_i64_host(len(t), t.ctypes.data if len(t) else None, len(q),
                                                   q.ctypes.data if len(q) else None,
                                                   pos.ctypes.data if len(q) else None))
        return pos
    with torch.cuda.device(dev):
        t = _tensor(ids, dev).reshape(-1).contiguous()
        q = _tensor(queries, dev).reshape(-1).contiguous()
        pos = torch.empty(q.numel(), dtype=torch.int32, device=dev)
        _lib.check(lib.ddr_network_lookup_i64(t.numel(), t.data_ptr() if t.numel() else None, q.numel(),
                                              q.data_ptr() if q.numel() else None,
                                              pos.data_ptr() if q.numel() else None, _lib.DDR_NETWORK_DEVICE_INPUT,
                                              _lib.stream_ptr(dev)))
    return pos


def _lookup_t(ids_t, q_t):
    """:func:`lookup` between tensors that live in one place, as an int64 tensor there."""
    import torch

    pos = lookup(ids_t, q_t)
    return (torch.from_numpy(pos) if isinstance(pos, np.ndarray) else pos).to(torch.int64)


def _foreign_id(ids_t) -> int:
    """An int64 that no row carries (a ``to_id`` equal to it makes an outlet)."""
    import torch

    for cand in (0, -1):
        if not bool((ids_t == cand).any()):
            return cand
    s = torch.sort(ids_t).values
    gap = torch.nonzero((s[1:] - s[:-1]) != 1)  # (a difference past 2^63 wraps, and is not 1 either)
    if gap.numel():
        return int(s[gap[0, 0]]) + 1
    return int(s[0]) - 1 if int(s[0]) > _I64_MIN else int(s[-1]) + 1


def parse_ids(strings, prefix: str) -> np.ndarray:
    """int64 ids of hydrofabric names: ``parse_ids(["wb-12", "wb-7"], "wb-")`` -> ``[12, 7]`` (the reference's
    ``_id_to_int``).  ``None`` or an empty string, a terminal nexus's missing ``toid``, gives -1."""
    out = np.empty(len(strings), np.int64)
    for i, s in enumerate(strings):
        if s is None or s == "":
            out[i] = -1
            continue
        if not s.startswith(prefix):
            raise ValueError(f"{s!r} does not start with {prefix!r}")
        out[i] = int(s[len(prefix):])
    return out


class Network:
    """The network of a flowpath table in the engine's contract.

    ``n`` kept reaches in the new order: ``ids[k]`` the id and ``position[k]`` the table row of new reach ``k``,
    ``down[k]`` the new index of its downstream reach (-1 at an outlet), ``rows`` / ``cols`` the COO in ascending
    ``cols`` (the engine's emission order), ``dropped`` the table rows that lay on a cycle (ascending), ``n_basins``
    the outlets and ``max_depth`` the longest reach-to-outlet path in edges.  The arrays are NumPy arrays from the
    host twin and device tensors from a device build.
    """

    def __init__(self, n_rows, device, position, ids, down, rows, cols, dropped, n_basins, max_depth):
        self.n_rows, self.device = int(n_rows), device
        self.position, self.ids, self.down, self.rows, self.cols, self.dropped = position, ids, down, rows, cols, dropped
        self.n, self.nnz = len(position), len(rows)
        self.n_basins, self.max_depth = int(n_basins), int(max_depth)
        self._host_position = None

    @classmethod
    def build(cls, ids, to_ids, device=None) -> "Network":
        """From ``ids[n]`` and ``to_ids[n]`` (NumPy arrays or tensors).  ``device=None`` with host input runs the host
        twin; a device, or device tensors (read in place), the HIP build on the current stream."""
        import torch

        dev = _device_of(device, ids, to_ids)
        lib = _lib.load()
        handle = C.c_void_p()
        info = _lib.NetworkCounts()
        if dev is None:
            a, b = _array(ids), _array(to_ids)
            if len(a) != len(b):
                raise ValueError("ids and to_ids differ in length")
            _lib.check(lib.ddr_network_build_host(len(a), a.ctypes.data if len(a) else None,
                                                  b.ctypes.data if len(a) else None, C.byref(handle)))
            try:
                _lib.check(lib.ddr_network_info(handle, C.byref(info)))
                i32 = lambda m: np.empty(int(m), np.int32)  # noqa: E731
                position, down, rows, cols, dropped = (i32(info.kept), i32(info.kept), i32(info.nnz), i32(info.nnz),
                                                       i32(info.n_dropped))
                order = np.empty(int(info.kept), np.int64)
                _lib.check(lib.ddr_network_get(handle, position.ctypes.data, order.ctypes.data, down.ctypes.data,
                                               rows.ctypes.data, cols.ctypes.data, dropped.ctypes.data, None))
            finally:
                lib.ddr_network_destroy(handle)
            return cls(len(a), None, position, order, down, rows, cols, dropped, info.n_basins, info.max_depth)
        with torch.cuda.device(dev):
            a = _tensor(ids, dev).reshape(-1).contiguous()
            b = _tensor(to_ids, dev).reshape(-1).contiguous()
            if a.numel() != b.numel():
                raise ValueError("ids and to_ids differ in length")
            st = _lib.stream_ptr(dev)
            n = a.numel()
            _lib.check(lib.ddr_network_build(n, a.data_ptr() if n else None, b.data_ptr() if n else None,
                                             _lib.DDR_NETWORK_DEVICE_INPUT, st, C.byref(handle)))
            try:
                _lib.check(lib.ddr_network_info(handle, C.byref(info)))
                i32 = lambda m: torch.empty(int(m), dtype=torch.int32, device=dev)  # noqa: E731
                position, down, rows, cols, dropped = (i32(info.kept), i32(info.kept), i32(info.nnz), i32(info.nnz),
                                                       i32(info.n_dropped))
                order = torch.empty(int(info.kept), dtype=torch.int64, device=dev)
                _lib.check(lib.ddr_network_get(handle, position.data_ptr(), order.data_ptr(), down.data_ptr(),
                                               rows.data_ptr(), cols.data_ptr(), dropped.data_ptr(), st))
            finally:
                lib.ddr_network_destroy(handle)
        return cls(n, dev, position, order, down, rows, cols, dropped, info.n_basins, info.max_depth)

    @classmethod
    def from_upstream_columns(cls, ids, ups, device=None) -> "Network":
        """The MERIT form (``COMID``, ``up1..up4``; ``merit/build.py:20-107``): ``ups`` is ``(n, k)``, row ``i`` lists
        the ids draining into ``ids[i]``, values ``<= 0`` are empty and an id absent from ``ids`` is ignored.  A reach
        listed as upstream of two different rows is refused (the reference asserts "not dendritic")."""
        import torch

        dev = _device_of(device, ids, ups)
        ids_t = _tensor(ids, dev).reshape(-1)
        ups_t = _tensor(ups, dev)
        n = ids_t.numel()
        if ups_t.dim() != 2 or ups_t.shape[0] != n:
            raise ValueError(f"ups must be (n, k) with n = {n} rows, not {tuple(ups_t.shape)}")
        flat = ups_t.reshape(-1)
        row = torch.arange(n, device=ids_t.device).repeat_interleave(ups_t.shape[1])
        listed = flat > 0
        up, row = _lookup_t(ids_t, flat[listed]), row[listed]
        known = up >= 0
        up, row = up[known], row[known]
        up, perm = torch.sort(up, stable=True)
        row = row[perm]
        clash = torch.nonzero((up[1:] == up[:-1]) & (row[1:] != row[:-1]))
        if clash.numel():
            k = int(clash[0, 0])
            raise ValueError(f"flowpath {int(ids_t[up[k]])} is listed as upstream of two different rows "
                             f"({int(ids_t[row[k]])} and {int(ids_t[row[k + 1]])}): the table is not dendritic")
        to = torch.full((n,), _foreign_id(ids_t) if n else 0, dtype=torch.int64, device=ids_t.device)
        to[up] = ids_t[row]
        return cls.build(ids_t, to, device=dev)

    @classmethod
    def from_nexus(cls, fp_ids, fp_to_nexus, nexus_ids, nexus_to_fp, device=None) -> "Network":
        """The Lynker hydrofabric form (``lynker_hydrofabric/io.py:60-154``): flowpath ``fp_ids[i]`` drains into nexus
        ``fp_to_nexus[i]``, nexus ``nexus_ids[j]`` into flowpath ``nexus_to_fp[j]``.  Nexus ids are deduplicated
        keeping the first; a nexus without a downstream flowpath among ``fp_ids`` is terminal.  Ghost nodes
        (``ghost=True`` there) are not built."""
        import torch

        dev = _device_of(device, fp_ids, fp_to_nexus, nexus_ids, nexus_to_fp)
        fp, fp_to, nx, nx_to = (_tensor(a, dev).reshape(-1) for a in (fp_ids, fp_to_nexus, nexus_ids, nexus_to_fp))
        if fp.numel() != fp_to.numel() or nx.numel() != nx_to.numel():
            raise ValueError("fp_ids / fp_to_nexus and nexus_ids / nexus_to_fp must pair up")
        s, perm = torch.sort(nx, stable=True)
        first = torch.ones(nx.numel(), dtype=torch.bool, device=nx.device)
        first[1:] = s[1:] != s[:-1]
        keep = perm[first]
        at = _lookup_t(nx[keep], fp_to)
        to = torch.full((fp.numel(),), _foreign_id(fp) if fp.numel() else 0, dtype=torch.int64, device=fp.device)
        hit = at >= 0
        to[hit] = nx_to[keep][at[hit]]
        return cls.build(fp, to, device=dev)

    # -- what the rest of the package takes ---------------------------------------------------------------------------
    def graph(self, **kw):
        """The :class:`ddr_amd.graph.RiverGraph` of this network (built on the device for a device build)."""
        from .graph import RiverGraph

        if self.device is not None:
            return RiverGraph(self.n, self.rows, self.cols, on_device=True, device=self.device, **kw)
        return RiverGraph(self.n, self.rows, self.cols, **kw)

    def upstream_index(self):
        """The :class:`ddr_amd.upstream.UpstreamIndex` of this network (per-gauge subsets, closures, members)."""
        from .upstream import UpstreamIndex

        return UpstreamIndex(self.n, self.rows, self.cols, device=self.device)

    def to_zarr(self, path, **attrs) -> None:
        """A ``conus_adjacency`` store (:func:`ddr_amd.zarr_coo.coo_to_zarr`) with ``order = ids``.  The engine's
        layout keeps ``order`` as int32, so ids outside int32 are refused."""
        from .zarr_coo import coo_to_zarr

        host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()  # noqa: E731
        ids = host(self.ids)
        if ids.size and (ids.min() < np.iinfo(np.int32).min or ids.max() > np.iinfo(np.int32).max):
            raise ValueError("the store's order array is int32: these ids do not fit")
        coo_to_zarr(path, self.n, host(self.rows), host(self.cols), order=ids, attrs=attrs or None)

    def align(self, column, axis: int = 0):
        """``column`` of the table (length, slope, a q' block, ...) in the network's order: ``column[position]`` along
        ``axis``.  A tensor on the network's device is gathered there; anything else on the host."""
        import torch

        if isinstance(column, torch.Tensor) and self.device is not None and column.device == self.device:
            return column.index_select(axis, self.position.to(torch.int64))
        if self._host_position is None:
            p = self.position
            self._host_position = p if isinstance(p, np.ndarray) else p.cpu().numpy()
        if isinstance(column, torch.Tensor):
            return column.index_select(axis, torch.from_numpy(self._host_position).to(column.device, torch.int64))
        return np.take(np.asarray(column), self._host_position, axis=axis)

    def __repr__(self) -> str:
        where = "host" if self.device is None else str(self.device)
        return (f"Network(n={self.n}, edges={self.nnz}, basins={self.n_basins}, max_depth={self.max_depth}, "
                f"dropped={len(self.dropped)} of {self.n_rows} rows, {where})")
