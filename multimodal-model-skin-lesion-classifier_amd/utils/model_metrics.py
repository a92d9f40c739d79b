"""evaluate_model on the HIP path -- drop-in name for the reference's utils/model_metrics.py.

One forward pass with nothing read back between batches: the confusion matrix, the loss and the soft-max rows ride on the
criterion's forward launch (EpochMeter), the one-vs-rest AUC is one launch of csrc/auc.hip; see mmskin/evaluate.py.
"""
import os
import sys

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from mmskin.evaluate import evaluate_model  # noqa: E402,F401
