"""Detection evaluation on the device: the AV2 sensor-dataset metric definitions (:mod:`.detection`) and the Waymo Open Dataset ones
(:mod:`.waymo`)."""

from .detection import AVERAGE_ROW, METRIC_COLUMNS, DetectionCfg, DetectionEvaluator, detection_cfg_factory, evaluate, match, summarize
from .waymo import WaymoDetectionCfg, WaymoDetectionEvaluator, evaluate_waymo

__all__ = ["AVERAGE_ROW", "METRIC_COLUMNS", "DetectionCfg", "DetectionEvaluator", "detection_cfg_factory", "evaluate", "match", "summarize",
           "WaymoDetectionCfg", "WaymoDetectionEvaluator", "evaluate_waymo"]
