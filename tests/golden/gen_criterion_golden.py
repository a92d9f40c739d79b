"""Writes tests/golden/criterion.json: what torch's nn.CrossEntropyLoss and the REFERENCE's own FocalLoss and
SoftTargetCrossEntropy classes give, in float64, on the seeded inputs of tests/criterion_oracle.golden_inputs, for every kind x
reduction x {class weights, none} (focal: gamma 0, 1.5, 2) on (B, C) = (3, 2), (7, 6), (5, 9): inputs, loss and d loss / d logits
(`none` is contracted with the recorded upstream vector).  Runs only where the reference is present (oracle.ref_import); no test
reads the reference -- they read the fixture.

    python tests/golden/gen_criterion_golden.py
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

import criterion_oracle as co  # noqa: E402
from oracle import ref_import  # noqa: E402


def main():
    assert ref_import.available(), "the reference is not on this machine"
    ref_import.load()                                                          # puts the reference's models/ on sys.path
    FocalLoss = importlib.import_module("focalLoss").FocalLoss
    SoftTargetCrossEntropy = importlib.import_module("softtargetsCrossEntropy").SoftTargetCrossEntropy
    shapes = {}
    for B, C in co.GOLDEN_SHAPES:
        inp = co.golden_inputs(B, C)
        t = {k: torch.from_numpy(v) for k, v in inp.items()}
        cases = {}
        for kind, reduction, weighted, gamma in co.golden_cases():
            z = t["logits"].clone().requires_grad_(True)
            w = t["weight"] if weighted else None
            if kind == "ce":
                loss = torch.nn.CrossEntropyLoss(weight=w, reduction=reduction)(z, t["labels"])
            elif kind == "focal":
                loss = FocalLoss(alpha=w, gamma=gamma, reduction=reduction)(z, t["labels"])
            else:
                loss = SoftTargetCrossEntropy(weight=w)(z, t["soft"])
            ((loss * t["upstream"]).sum() if reduction == "none" else loss).backward()
            cases[co.case_key(kind, reduction, weighted, gamma)] = {"loss": loss.detach().tolist(), "dlogits": z.grad.tolist()}
        shapes[f"{B}x{C}"] = {"inputs": {k: v.tolist() for k, v in inp.items()}, "cases": cases}
    with open(os.path.join(HERE, "criterion.json"), "w") as f:
        json.dump({"dtype": "float64", "shapes": shapes}, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
