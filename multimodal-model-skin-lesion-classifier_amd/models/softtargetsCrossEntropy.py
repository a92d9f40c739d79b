"""SoftTargetCrossEntropy on the HIP path -- drop-in name for the reference's models/softtargetsCrossEntropy.py.

One fused forward and one fused backward launch (csrc/criterion.hip); see mmskin/criterion.py.
"""
import os
import sys

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from mmskin.criterion import SoftTargetCrossEntropy  # noqa: E402,F401
