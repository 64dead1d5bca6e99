"""The per-batch feed on the device (mirrors ``ddr.io.readers`` and the tensor half of ``ddr.geodatazoo``'s
``collate_fn``; reading the zarr / icechunk stores stays host code): the lateral-inflow store, the gauge observations
and the catchment attributes with the flowpath arrays, uploaded once and gathered per batch; and the attribute statistics
(``ddr.io.statistics``) as one device call."""

from .attributes import (AttributeBatch, AttributeStore, FlowScaleTable, align_attributes, flow_scale_factors,
                         flowpath_fill)
from .statistics import STATISTIC_KEYS, attribute_statistics, read_statistics_json, write_statistics_json
from .stores import (FILL, ObservationStore, RowIndex, StreamflowStore, daily_window, feed_plan, hourly_window,
                     pad_gage_ids)

__all__ = ["FILL", "STATISTIC_KEYS", "AttributeBatch", "AttributeStore", "FlowScaleTable", "ObservationStore",
           "RowIndex", "StreamflowStore", "align_attributes", "attribute_statistics", "daily_window", "feed_plan",
           "flow_scale_factors", "flowpath_fill", "hourly_window", "pad_gage_ids", "read_statistics_json",
           "write_statistics_json"]
