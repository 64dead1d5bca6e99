"""Per-gauge evaluation metrics on the device (``csrc/metrics.hip``), mirroring ``ddr.validation.metrics``.

The reference's loops call ``Metrics(pred, target)`` after every routing call (``scripts/train.py:106-115`` per
mini-batch, ``scripts/test.py:107`` once per evaluation): a host copy of the (G, D) daily series, a stream wait
and a Python loop per gauge (two sorts, ``pearsonr``, ``spearmanr`` and a dozen reductions each).  Here the 18
metrics of every gauge come out of one launch (``ddr_metrics_f32``):

* :func:`metrics_device` -- device tensors in, an (18, G) fp64 device tensor out, no host sync (capturable);
* :class:`Metrics` -- the reference's class: NumPy arrays or tensors in, the 18 names as NumPy attributes.

All arithmetic is fp64 over the fp32 inputs, two-pass where a mean is involved, in a fixed order: the values
agree with the reference run on the same inputs cast to fp64 to rounding, and a gauge's values do not depend
on the batch it is computed in.
"""

from __future__ import annotations

import json

import numpy as np
import torch

from .. import _lib

#: row order of :func:`metrics_device`'s result (``DDR_METRIC_*`` in ``include/ddr_mc.h``)
METRIC_NAMES = (
    "bias", "mae", "rmse", "ub_rmse", "fdc_rmse", "corr", "corr_spearman", "r2", "nse", "flv", "fhv", "pbias",
    "pbias_mid", "kge", "kge_12", "rmse_low", "rmse_high", "rmse_mid",
)
MAX_DAYS = 8192


def metrics_device(pred: torch.Tensor, target: torch.Tensor, warmup: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """The 18 metrics of ``pred[:, warmup:]`` against ``target[:, warmup:]``: two (G, D) or (D,) fp32 HIP tensors
    -> ``(values, pred_nan_count)``, an (18, G) fp64 tensor in :data:`METRIC_NAMES` order and a one-word int32
    tensor holding the number of NaN in ``pred``, both on the current stream without a host sync.

    A day is valid when its target is not NaN.  Any row stride is taken as it is (a sliced view costs no copy); a
    tensor whose innermost stride is not 1 is made contiguous.  At most 8192 days after the warm-up."""
    if not isinstance(pred, torch.Tensor) or not isinstance(target, torch.Tensor):
        raise TypeError("metrics_device takes torch tensors")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("pred and target must be float32")
    if pred.dim() not in (1, 2) or target.shape != pred.shape:
        raise ValueError("pred and target must be the same (G, D) or (D,) shape")
    if pred.dim() == 1:
        pred, target = pred.unsqueeze(0), target.unsqueeze(0)
    G, D = pred.shape
    if not 0 <= warmup < D:
        raise ValueError("warmup must be in [0, D)")
    if not pred.is_cuda or not target.is_cuda:
        raise RuntimeError("metrics_device runs on the HIP device only (no CPU fallback)")
    if target.device != pred.device:
        raise ValueError("pred and target must be on the same device")
    pred, target = pred[:, warmup:], target[:, warmup:]
    if pred.stride(1) != 1:
        pred = pred.contiguous()
    if target.stride(1) != 1:
        target = target.contiguous()
    with torch.cuda.device(pred.device):
        values = torch.empty((len(METRIC_NAMES), G), device=pred.device, dtype=torch.float64)
        count = torch.zeros(1, device=pred.device, dtype=torch.int32)
        _lib.check(_lib.load().ddr_metrics_f32(G, D - warmup, pred.data_ptr(), pred.stride(0), target.data_ptr(),
                                               target.stride(0), values.data_ptr(), count.data_ptr(),
                                               _lib.stream_ptr(pred.device)))
    return values, count


class Metrics:
    """``ddr.validation.Metrics`` computed on the device: ``Metrics(pred, target)`` takes NumPy arrays or tensors,
    1-D (one gauge) or 2-D (gauges, days), and exposes ``bias, mae, rmse, ub_rmse, fdc_rmse, corr, corr_spearman,
    r2, nse, flv, fhv, pbias, pbias_mid, kge, kge_12, rmse_low, rmse_high, rmse_mid`` as float64 arrays of shape
    (gauges,), plus ``pred``, ``target``, ``ngrid`` and ``nt``.

    Inputs of another floating dtype (the reference takes what it is given, usually fp32) are cast to float32
    first; the arithmetic on them is fp64.  ``device`` picks the HIP device for host inputs (default: the
    tensors' own, else the current one).  The results are copied to the host once.  Raises the reference
    validator's ``ValueError`` when ``pred`` holds NaN."""

    def __init__(self, pred, target, device=None) -> None:
        if not torch.cuda.is_available():
            raise RuntimeError("Metrics runs on the HIP device only (no CPU fallback)")
        p = self._as_device(pred, device)
        t = self._as_device(target, p.device)
        values, count = metrics_device(p, t)
        host = torch.cat([values.reshape(-1), count.to(torch.float64)]).cpu().numpy()  # the one copy of results
        if host[-1] > 0:
            raise ValueError("pred contains NaN, check your gradient chain")
        self.pred = np.atleast_2d(pred.detach().cpu().numpy() if isinstance(pred, torch.Tensor) else np.asarray(pred))
        self.target = np.atleast_2d(
            target.detach().cpu().numpy() if isinstance(target, torch.Tensor) else np.asarray(target))
        table = host[:-1].reshape(len(METRIC_NAMES), -1)
        for k, name in enumerate(METRIC_NAMES):
            setattr(self, name, np.ascontiguousarray(table[k]))

    @staticmethod
    def _as_device(x, device) -> torch.Tensor:
        if isinstance(x, torch.Tensor):
            x = x.detach()
            if device is not None:
                return x.to(device=device, dtype=torch.float32)
            return x.to(torch.float32) if x.is_cuda else x.to(device="cuda", dtype=torch.float32)
        a = np.asarray(x)
        if a.ndim not in (1, 2):
            raise ValueError("pred and target must be 1-D or 2-D")
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device if device is not None else "cuda")

    @property
    def ngrid(self) -> int:
        """Number of gauges."""
        return int(self.pred.shape[0])

    @property
    def nt(self) -> int:
        """Number of time steps."""
        return int(self.pred.shape[1])

    def model_dump(self) -> dict:
        """The 18 metrics as lists (the keys of the reference's JSON dump: ``pred`` / ``target`` dropped)."""
        return {name: getattr(self, name).tolist() for name in METRIC_NAMES}

    def model_dump_json(self, **kwargs) -> str:
        """JSON of :meth:`model_dump` with the reference dump's keys; NaN and +-inf are written as ``null``, as the
        reference's pydantic serialiser writes them.  ``kwargs`` go to :func:`json.dumps`."""
        def clean(v):
            return [x if np.isfinite(x) else None for x in v]

        return json.dumps({k: clean(v) for k, v in self.model_dump().items()}, **kwargs)
