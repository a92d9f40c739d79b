"""Writes tests/golden/evaluate.json: what the REFERENCE's own evaluate_model (utils/model_metrics.py) returns, with the
scikit-learn installed beside it, for a stub model that hands back stored logits, on the seeded cases of
tests/evaluate_oracle.golden_inputs: six classes in batches of 40 / 40 / 17, two classes, six classes with one absent from the
labels, three classes with a single one present (the AUC is NaN) and duplicated logit rows (ties).  Every case stores the
logits, the labels, the batch sizes and the reference's metrics, predictions and probabilities.  Runs only where the reference
is present (oracle.ref_import); no test reads the reference -- they read the fixture.

    python tests/golden/gen_evaluate_golden.py
"""
import importlib.util
import json
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import evaluate_oracle as eo  # noqa: E402
from oracle import ref_import  # noqa: E402


def main():
    assert ref_import.available(), "the reference is not on this machine"
    path = os.path.join(os.path.dirname(ref_import.REF_MODELS), "utils", "model_metrics.py")
    spec = importlib.util.spec_from_file_location("reference_model_metrics", path)
    reference = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(reference)
    import sklearn
    cases = {}
    for name in eo.GOLDEN_CASES:
        logits, labels = eo.golden_inputs(name)
        sizes = eo.batch_sizes(name, len(labels))
        with tempfile.TemporaryDirectory() as td, warnings.catch_warnings():
            warnings.simplefilter("ignore")                                   # sklearn warns where a class has one kind of row
            metrics, all_labels, all_preds, all_probs = reference.evaluate_model(eo.StoredLogits(torch.from_numpy(logits)), eo.loader_for(labels, sizes),
                                                                                 None, "cpu", 3, td, "stub")
        assert np.array_equal(all_labels, labels)
        cases[name] = {"batches": list(sizes), "logits": logits.astype(np.float64).tolist(), "labels": labels.tolist(), "metrics": metrics,
                       "predictions": all_preds.tolist(), "probabilities": all_probs.astype(np.float64).tolist()}
    with open(os.path.join(HERE, "evaluate.json"), "w") as f:
        json.dump({"sklearn": sklearn.__version__, "probabilities_dtype": "float32", "cases": cases}, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
