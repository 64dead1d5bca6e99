"""The per-batch forcing feed on the device (mirrors ``ddr.io.readers``; reading the zarr / icechunk stores stays
host code): the lateral-inflow store and the gauge observations, uploaded once and gathered per batch."""

from .stores import (FILL, ObservationStore, RowIndex, StreamflowStore, daily_window, feed_plan, hourly_window,
                     pad_gage_ids)

__all__ = ["FILL", "ObservationStore", "RowIndex", "StreamflowStore", "daily_window", "feed_plan", "hourly_window",
           "pad_gage_ids"]
