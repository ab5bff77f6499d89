"""Detection evaluation (AV2 sensor-dataset metric definitions) on the device -- see :mod:`.detection`."""

from .detection import AVERAGE_ROW, METRIC_COLUMNS, DetectionCfg, DetectionEvaluator, detection_cfg_factory, evaluate, match, summarize

__all__ = ["AVERAGE_ROW", "METRIC_COLUMNS", "DetectionCfg", "DetectionEvaluator", "detection_cfg_factory", "evaluate", "match", "summarize"]
