"""Build container only (CPU, seconds): run the REFERENCE's own ScoreCAM class (interpretability/ScoreCam.py:62-155) on the CPU
oracle model and record what it saw and returned -> tests/golden/scorecam_resnet18.npz (data only).

    python tests/golden/gen_scorecam_golden.py

The reference file imports torchvision, matplotlib and its own `benchmark.models` package at module level; none of them is
used by the class, so empty stand-in module objects are registered for the import statement only.
Everything is seeded: det_init_ weights, det_inputs(1, 64, 20, 6).  Recorded: the hooked feature map of the last conv
[512, 2, 2], the logits of the 512 masked forwards [512, 6], the 512 soft-max scores of the target class, the heat map
[64, 64] and the target class.  tests/test_cpu_scorecam.py and tests/test_gpu_scorecam.py rebuild inputs and weights."""
import importlib.util
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import torch.nn as nn

from helpers import SMALL
from oracle.detinit import det_init_, det_inputs
from oracle.model import OracleMultimodalModel

REF_FILE = "/root/reference/src/scripts/benchmark/interpretability/ScoreCam.py"
OUT = os.path.join(ROOT, "tests", "golden", "scorecam_resnet18.npz")
KW = dict(SMALL, cnn_model_name="resnet-18", attention_mecanism="crossattention")     # common_dim 64, vocab 20, 6 classes
TARGET_CLASS = 2


def load_reference_class():
    def stub(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        for k, v in attrs.items():
            if not hasattr(m, k):
                setattr(m, k, v)
        sys.modules[name] = m
        return m

    stub("torchvision", transforms=stub("torchvision.transforms"))
    stub("matplotlib", pyplot=stub("matplotlib.pyplot"))
    models = stub("benchmark.models", multimodalIntraInterModal=types.ModuleType("multimodalIntraInterModal"),
                  multimodalIntraInterModalToOptimzeAfterFIneTunning=types.ModuleType("multimodalIntraInterModalToOptimzeAfterFIneTunning"))
    stub("benchmark", models=models)
    spec = importlib.util.spec_from_file_location("reference_scorecam", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ScoreCAM


def last_conv(module):
    last = None
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            last = m
    return last


def main():
    ScoreCAM = load_reference_class()
    model = det_init_(OracleMultimodalModel(**KW)).eval()
    img, meta, _ = det_inputs(1, 64, 20, 6)
    logits, fmaps = [], []
    model.register_forward_hook(lambda mod, i, o: logits.append(o.detach().clone()))
    last_conv(model.image_encoder).register_forward_hook(lambda mod, i, o: fmaps.append(o.detach().clone()))
    cam = ScoreCAM(model, last_conv(model.image_encoder), "cpu")
    heat = cam.generate_heatmap(img, meta, TARGET_CLASS)
    cam.remove_hook()
    fmap = fmaps[0][0].numpy().astype(np.float32)                                     # the unmasked forward's map
    masked_logits = torch.cat(logits[1:]).numpy().astype(np.float32)                  # logits[0]: the unmasked forward
    scores = torch.softmax(torch.from_numpy(masked_logits), dim=1)[:, TARGET_CLASS].numpy()
    assert fmap.shape == (512, 2, 2) and masked_logits.shape == (512, 6) and heat.shape == (64, 64), (fmap.shape, heat.shape)
    np.savez_compressed(OUT, fmap=fmap, logits=masked_logits, scores=scores.astype(np.float32), heat=heat.astype(np.float32),
                        target_class=np.int64(TARGET_CLASS))
    print(OUT, os.path.getsize(OUT), "bytes; heat", float(heat.min()), float(heat.max()), "sum of scores", float(scores.sum()))


if __name__ == "__main__":
    main()
