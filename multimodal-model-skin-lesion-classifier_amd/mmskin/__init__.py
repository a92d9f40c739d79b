"""mmskin: MI355X (gfx950) implementation of the MultimodalModel hot path.

Layout:
  csrc/      hand-written HIP kernels + the C ABI (built into libmmskin_hip.so)
  mmskin/    ctypes binding, autograd wrappers, parameter-holder modules, DP helper
  models/    drop-in modules with the reference's file / class names
"""
from . import _lib, criterion, evaluate  # noqa: F401
from .calibration import Calibration, TemperatureScaling  # noqa: F401
from .conformal import ConformalPredictor, ConformalReport  # noqa: F401
from .curves import FoldCurves  # noqa: F401
from .criterion import CrossEntropyLoss, EpochMeter, FocalLoss, SoftTargetCrossEntropy  # noqa: F401
from .evaluate import evaluate_model  # noqa: F401
from .permutation import MetadataPermutationImportance  # noqa: F401
from .subgroup import SubgroupAudit, group_ids  # noqa: F401
from .uncertainty import PredictiveUncertainty  # noqa: F401

__all__ = ["_lib", "criterion", "evaluate", "CrossEntropyLoss", "FocalLoss", "SoftTargetCrossEntropy", "EpochMeter", "evaluate_model",
           "MetadataPermutationImportance", "Calibration", "TemperatureScaling", "FoldCurves", "PredictiveUncertainty", "ConformalPredictor",
           "ConformalReport", "SubgroupAudit", "group_ids"]
