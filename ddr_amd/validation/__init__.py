"""Evaluation on the device (mirrors ``ddr.validation``; the plots and ``log_metrics`` stay host code): the
per-gauge metrics and the baselines they are read against (summed Q', fixed-parameter linear routing)."""

from .linear_baseline import linear_baseline
from .metrics import METRIC_NAMES, Metrics, metrics_device
from .summed_q_prime import SummedQPrime, members_from_ids, summed_q_prime_metrics

__all__ = ["METRIC_NAMES", "Metrics", "metrics_device", "SummedQPrime", "members_from_ids", "summed_q_prime_metrics",
           "linear_baseline"]
