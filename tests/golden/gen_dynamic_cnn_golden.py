"""Writes tests/golden/dynamic_cnn.json from the REFERENCE's own `DynamicCNN` class (models/dynamicMultimodalmodel.py) on the CPU: for
the configurations of tests/dynamic_cnn_oracle.GOLDEN_CONFIGS, built under torch.manual_seed(GOLDEN_SEED), the state_dict keys and shapes
in order, the per-tensor [sum, sum of |.|] of the seeded initialisation, and the eval-mode logits of one forward on
dynamic_cnn_oracle.golden_inputs (N = 2, 3 x 32 x 32).  Runs only where the reference is present (oracle.ref_import); no test reads the
reference -- they read the fixture.

    python tests/golden/gen_dynamic_cnn_golden.py
"""
import importlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dynamic_cnn_oracle as do  # noqa: E402
from oracle import ref_import  # noqa: E402


def main():
    assert ref_import.available(), "the reference is not on this machine"
    sys.path.insert(0, ref_import.REF_MODELS)            # the class imports its `metablock` sibling by bare name
    DynamicCNN = importlib.import_module("dynamicMultimodalmodel").DynamicCNN
    out = {}
    for name, kw in do.GOLDEN_CONFIGS.items():
        torch.manual_seed(do.GOLDEN_SEED)
        m = DynamicCNN(**kw).eval()
        sd = m.state_dict()
        img, meta = do.golden_inputs(kw["vocab_size"])
        with torch.no_grad():
            logits = m(img, meta)
        out[name] = {"keys": [[k, list(v.shape)] for k, v in sd.items()], "sums": do.tensor_sums(sd), "logits": logits.double().tolist()}
    with open(os.path.join(HERE, "dynamic_cnn.json"), "w") as f:
        json.dump({"seed": do.GOLDEN_SEED, "configs": out}, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
