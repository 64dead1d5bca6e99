"""The upstream index: everything upstream of a set of reaches, from the network's COO alone.

The reference finds it offline or with rustworkx: the engine writes one ``gages_adjacency`` subset per gauge
(``engine/src/ddr_engine/merit/build.py:206-290`` ``build_gauge_adjacencies``, ``graph.py:89-115``
``subset_upstream``: ``rx.ancestors``), the target-catchments mode of ``scripts/router.py`` computes
``rx.ancestors`` per target and a Python mask over every CONUS edge
(``Merit._build_routing_data_target_catchments``, ``src/ddr/geodatazoo/merit.py:321-396``), and
``scripts/summed_q_prime.py`` looks every gauge's upstream divides up from those subsets.  The network itself
(``conus_adjacency``: strictly lower-triangular COO, dendritic, upstream reaches numbered first) determines all
three.  :class:`UpstreamIndex` keeps ``down[n]`` and the longest reach-to-outlet path, built once per network
(``csrc/upstream.hip``; the host twin ``csrc/upstream_host.cpp`` needs no GPU), and answers per batch:

* :meth:`UpstreamIndex.collate` -- the union subnetwork of a gauge batch, bit-identical to
  :func:`ddr_amd.batching.collate_gauges` / ``collate_gauges_device`` fed with the engine's complete subsets, without
  shipping them (nested gauges repeat their shared edges there);
* :meth:`UpstreamIndex.subnetwork` -- the target-catchments mode;
* :meth:`UpstreamIndex.members` -- the per-gauge member lists :class:`ddr_amd.validation.SummedQPrime` takes;
* :meth:`UpstreamIndex.subsets` -- the engine's per-gauge COO, so
  :func:`ddr_amd.zarr_coo.gauge_subsets_to_zarr` can write a ``gages_adjacency`` store without the engine.

One deliberate difference from the reference: its target mode takes ``unique(rows | cols)`` of the kept edges, so a
target that is an isolated headwater vanishes from the subnetwork (``merit.py:361``).  Here a target always belongs
to its own closure, as :func:`collate_gauges` already keeps a headwater gauge.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .batching import CollatedBatch, DeviceBatch


def _targets(a) -> np.ndarray:
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):
        raise ValueError("reach indices must fit int32")
    return np.ascontiguousarray(a.astype(np.int32))


class UpstreamIndex:
    """``down[n]`` of the network ``(n, rows, cols)`` (row = downstream reach) and the queries on it.

    ``device=None`` builds a host-only index (no GPU needed): ``collate`` returns a :class:`CollatedBatch` and every
    query runs in the C library's host twin.  With a device the index lives there, ``collate`` returns a
    :class:`DeviceBatch` and the queries are HIP launches; ``rows`` / ``cols`` may then be device tensors, which are
    read in place.  Gauges and targets are reach indices in ``[0, n)``; the same reach may be named more than once.
    """

    def __init__(self, n: int, rows, cols, device=None) -> None:
        import torch

        self._handle = C.c_void_p()
        self.device = None if device is None else torch.device(device)
        lib = _lib.load()
        on_device = isinstance(rows, torch.Tensor) and rows.is_cuda
        if on_device:
            if self.device is None:
                raise ValueError("a host-only index takes host arrays")
            rows = rows.reshape(-1).to(self.device, torch.int32).contiguous()
            cols = torch.as_tensor(cols).reshape(-1).to(self.device, torch.int32).contiguous()
            e, pr, pc = rows.numel(), rows.data_ptr(), cols.data_ptr()
        else:
            rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int32)
            cols = np.ascontiguousarray(np.asarray(cols).reshape(-1), dtype=np.int32)
            e, pr, pc = len(rows), rows.ctypes.data, cols.ctypes.data
        if e != (cols.numel() if on_device else len(cols)):
            raise ValueError("rows and cols differ in length")
        if self.device is None:
            code = lib.ddr_upstream_index_create(int(n), e, pr, pc, _lib.DDR_UPSTREAM_HOST_ONLY, None,
                                                 C.byref(self._handle))
        else:
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            with torch.cuda.device(self.device):
                code = lib.ddr_upstream_index_create(int(n), e, pr, pc,
                                                     _lib.DDR_UPSTREAM_DEVICE_COO if on_device else 0,
                                                     _lib.stream_ptr(self.device), C.byref(self._handle))
        _lib.check(code)
        info = _lib.UpstreamInfo()
        _lib.check(lib.ddr_upstream_index_info(self._handle, C.byref(info)))
        self.n, self.n_outlets, self.max_depth, self.rounds = (int(info.n), int(info.n_outlets), int(info.max_depth),
                                                               int(info.rounds))
        self._down = None
        self._deg = None

    @classmethod
    def from_zarr(cls, path, device=None) -> "UpstreamIndex":
        """From a ``conus_adjacency`` store (:func:`ddr_amd.zarr_coo.coo_from_zarr`)."""
        from .zarr_coo import coo_from_zarr

        n, rows, cols, _, _ = coo_from_zarr(path)
        return cls(n, rows, cols, device=device)

    def __del__(self) -> None:
        handle, self._handle = getattr(self, "_handle", None), None
        if handle:
            try:
                _lib.load().ddr_upstream_index_destroy(handle)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass

    @property
    def down(self) -> np.ndarray:
        """int32[n]: the downstream reach of every reach, -1 at an outlet (a host copy)."""
        if self._down is None:
            d = np.empty(self.n, np.int32)
            _lib.check(_lib.load().ddr_upstream_index_down(self._handle, d.ctypes.data))
            d.setflags(write=False)
            self._down = d
        return self._down

    # -- plumbing ---------------------------------------------------------------------------------------------------
    def _outflow_cap(self, t: np.ndarray) -> int:
        """Entries of the outflow_idx lists: per gauge the inflows of its reach, or the reach itself (gauges sharing
        a confluence each list its inflows, so n + G does not bound it)."""
        if self._deg is None:
            d = self.down
            self._deg = np.bincount(d[d >= 0], minlength=self.n)
        if not len(t) or t.min() < 0 or t.max() >= self.n:  # (an out-of-range gauge is the library's to refuse)
            return 0
        return int(np.maximum(self._deg[t], 1).sum())

    def _scratch(self, G: int, n_members: int = 0):
        import torch

        nbytes = int(_lib.load().ddr_upstream_scratch_bytes(self._handle, G, n_members))
        return torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=self.device), nbytes

    def _stream(self, stream):
        import torch

        return stream if stream is not None else torch.cuda.current_stream(self.device)

    # -- queries ----------------------------------------------------------------------------------------------------
    def label(self, targets, stream=None):
        """``(label, slot_of)``: ``label[i]`` (int32[n]; a device tensor on a device index) is the slot of the nearest
        target at or downstream of reach ``i``, -1 without one; ``slot_of[g]`` the smallest slot naming ``targets[g]``'s
        reach."""
        t = _targets(targets)
        G = len(t)
        slot_of = np.empty(G, np.int32)
        lib = _lib.load()
        if self.device is None:
            label = np.empty(self.n, np.int32)
            _lib.check(lib.ddr_upstream_label_host(self._handle, G, t.ctypes.data, label.ctypes.data,
                                                   slot_of.ctypes.data))
            return label, slot_of
        import torch

        with torch.cuda.device(self.device):
            st = self._stream(stream)
            with torch.cuda.stream(st):
                label = torch.empty(self.n, dtype=torch.int32, device=self.device)
                scratch, nbytes = self._scratch(G)
            _lib.check(lib.ddr_upstream_label(self._handle, G, t.ctypes.data, label.data_ptr(), slot_of.ctypes.data,
                                              scratch.data_ptr(), nbytes, st.cuda_stream))
        return label, slot_of

    def closure(self, targets) -> np.ndarray:
        """Ascending ids (int64) of every reach at or upstream of a target."""
        label, _ = self.label(targets)
        if self.device is None:
            return np.nonzero(label >= 0)[0].astype(np.int64)
        import torch

        return torch.nonzero(label >= 0).reshape(-1).cpu().numpy().astype(np.int64)

    def collate(self, gage_idx, gage_catchment=None, stream=None):
        """The union subnetwork of the gauges' closures: what ``collate_gauges`` (host index, a
        :class:`CollatedBatch`) or ``collate_gauges_device`` (device index, a :class:`DeviceBatch`) gives for the
        gauges' complete upstream subsets."""
        t = _targets(gage_idx)
        G = len(t)
        n = self.n
        lib = _lib.load()
        na, nnz = C.c_int64(), C.c_int64()
        if self.device is None:
            active = np.empty(n, np.int32)
            crow = np.empty(n + 1, np.int64)
            col = np.empty(n, np.int32)
            out_off = np.empty(G + 1, np.int64)
            out_idx = np.empty(max(self._outflow_cap(t), 1), np.int32)
            gage_c = np.empty(max(G, 1), np.int32)
            _lib.check(lib.ddr_upstream_collate_host(self._handle, G, t.ctypes.data, active.ctypes.data, n,
                                                     C.byref(na), crow.ctypes.data, col.ctypes.data, n, C.byref(nnz),
                                                     out_off.ctypes.data, out_idx.ctypes.data, len(out_idx),
                                                     gage_c.ctypes.data))
            m = na.value
            outflow = [out_idx[out_off[g]:out_off[g + 1]].astype(np.int64) for g in range(G)]
            return CollatedBatch(n, active[:m].astype(np.int64), crow[:m + 1].copy(), col[:nnz.value].astype(np.int64),
                                 outflow, [int(x) for x in gage_c[:G]], [int(x) for x in t],
                                 list(gage_catchment) if gage_catchment is not None else [None] * G)
        import torch

        cap = self._outflow_cap(t)
        with torch.cuda.device(self.device):
            st = self._stream(stream)
            with torch.cuda.stream(st):
                i32 = dict(dtype=torch.int32, device=self.device)
                active, rows_c, cols_c, col = (torch.empty(n, **i32) for _ in range(4))
                crow = torch.empty(n + 1, dtype=torch.int64, device=self.device)
                out_off = torch.empty(G + 1, dtype=torch.int64, device=self.device)
                out_idx = torch.empty(max(cap, 1), **i32)
                gage_c = torch.empty(max(G, 1), **i32)
                scratch, nbytes = self._scratch(G)
            _lib.check(lib.ddr_upstream_collate(
                self._handle, G, t.ctypes.data, active.data_ptr(), n, C.byref(na), rows_c.data_ptr(),
                cols_c.data_ptr(), n, C.byref(nnz), crow.data_ptr(), col.data_ptr(), out_off.data_ptr(),
                out_idx.data_ptr(), out_idx.numel(), gage_c.data_ptr(), scratch.data_ptr(), nbytes, st.cuda_stream))
        m, k = na.value, nnz.value
        return DeviceBatch(n, active[:m], rows_c[:k], cols_c[:k], crow[:m + 1], col[:k], out_off,
                           out_idx[:int(out_off[-1].item()) if G else 0], gage_c[:G], [int(x) for x in t])

    def subnetwork(self, targets, stream=None):
        """The reference's ``target_catchments`` mode (``merit.py:321-396``): everything at or above ``targets`` as
        one compressed network; ``.active`` maps its reaches back to the network's indices (and so to divide ids).
        Unlike the reference, an isolated headwater target stays in the subnetwork (module docstring)."""
        return self.collate(targets, stream=stream)

    def members_device(self, gage_idx, stream=None):
        """:meth:`members` as device tensors (device index only)."""
        if self.device is None:
            raise RuntimeError("members_device needs a device index")
        import torch

        t = _targets(gage_idx)
        G = len(t)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            st = self._stream(stream)
            with torch.cuda.stream(st):
                off = torch.empty(G + 1, dtype=torch.int64, device=self.device)
                scratch, nbytes = self._scratch(G)
            total = C.c_int64()
            _lib.check(lib.ddr_upstream_member_counts(self._handle, G, t.ctypes.data, off.data_ptr(), C.byref(total),
                                                      scratch.data_ptr(), nbytes, st.cuda_stream))
            M = total.value
            with torch.cuda.stream(st):
                idx = torch.empty(M, dtype=torch.int32, device=self.device)
                scratch, nbytes = self._scratch(G, M)
            _lib.check(lib.ddr_upstream_members(self._handle, G, t.ctypes.data, M, idx.data_ptr() if M else None,
                                                scratch.data_ptr(), nbytes, st.cuda_stream))
        return off, idx

    def members(self, gage_idx) -> tuple[np.ndarray, np.ndarray]:
        """``(off int64[G + 1], idx int32)``: gauge g's reach and everything upstream of it, ascending, at
        ``idx[off[g]:off[g + 1]]`` -- the lists ``SummedQPrime(off, idx)`` takes.  Nested gauges repeat their shared
        reaches; gauges on one reach get equal lists."""
        if self.device is not None:
            off, idx = self.members_device(gage_idx)
            return off.cpu().numpy(), idx.cpu().numpy()
        t = _targets(gage_idx)
        G = len(t)
        lib = _lib.load()
        off = np.empty(G + 1, np.int64)
        _lib.check(lib.ddr_upstream_member_counts_host(self._handle, G, t.ctypes.data, off.ctypes.data))
        idx = np.empty(int(off[-1]), np.int32)
        _lib.check(lib.ddr_upstream_members_host(self._handle, G, t.ctypes.data, off.ctypes.data,
                                                 idx.ctypes.data if len(idx) else None))
        return off, idx

    def subsets(self, gage_idx) -> list:
        """``[(rows, cols, gage_idx)]``: the engine's per-gauge COO (``build_gauge_adjacencies``), every edge between
        two reaches of the gauge's closure, ``cols`` ascending -- the input of ``collate_gauges*`` and of
        :func:`ddr_amd.zarr_coo.gauge_subsets_to_zarr`."""
        t = _targets(gage_idx)
        off, idx = self.members(t)
        down = self.down
        out = []
        for g, reach in enumerate(t):
            m = idx[off[g]:off[g + 1]]
            cols = m[m != reach]
            out.append((down[cols].astype(np.int32), cols.astype(np.int32), int(reach)))
        return out

    def __repr__(self) -> str:
        where = "host" if self.device is None else str(self.device)
        return (f"UpstreamIndex(n={self.n}, outlets={self.n_outlets}, max_depth={self.max_depth}, "
                f"rounds={self.rounds}, {where})")
