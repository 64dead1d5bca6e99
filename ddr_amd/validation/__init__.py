"""Evaluation metrics on the device (mirrors ``ddr.validation``; the plots and ``log_metrics`` stay host code)."""

from .metrics import METRIC_NAMES, Metrics, metrics_device

__all__ = ["METRIC_NAMES", "Metrics", "metrics_device"]
