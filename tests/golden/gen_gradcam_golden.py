"""Build container only (CPU, seconds): run the REFERENCE's own Grad-CAM++ class (src/services/XAI/models/cam.py:29-70, a
torch-only file) on the CPU oracle model and record what it returned -> tests/golden/gradcam_resnet18.npz (data only).

    python tests/golden/gen_gradcam_golden.py

The model is the CPU half of the pair tests/test_gpu_model.py::test_gradcam_consumer_on_last_conv builds: resnet-18,
`concatenation`, det_init_ weights, hooked at the last conv.  The inputs are gradcam_oracle.det_rows(3, 64): the three images
of det_inputs(3, 64, 20, 6), each with five metadata rows (salts 0 .. 4).  As the reference's mosaic script does
(multiple_sample_using_gradcam_plusplus_atualizado.py:383-389), every row is explained for its own predicted class, taken from
a no_grad forward.  Recorded: the seeds' shape (images, variants, size), the logits [15, 6], the target classes [15] and the
Grad-CAM++ maps [15, 64, 64].

Plain Grad-CAM lives in interpretability/gradcam_atualizado.py:230-257, whose top-level imports want torchvision and the
reference's `models` package.  They are not used by the class, so empty stand-in modules are registered for the import
statement only; pandas, matplotlib and PIL are imported for real.  When the file loads, its GradCAM
maps are recorded as `gradcam_maps` (and its GradCAMPlusPlus must return what cam.py's does); when it does not, `gradcam_maps`
is left out and plain Grad-CAM is pinned on the restatement (tests/gradcam_oracle.py) alone -- tests/test_cpu_gradcam.py
checks whichever the fixture holds."""
import importlib.util
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
import torch.nn as nn

import gradcam_oracle as go
from helpers import SMALL
from oracle.detinit import det_init_
from oracle.model import OracleMultimodalModel

REF = "/root/reference/src"
OUT = os.path.join(ROOT, "tests", "golden", "gradcam_resnet18.npz")
KW = dict(SMALL, cnn_model_name="resnet-18", attention_mecanism="concatenation")
N_IMAGES, SIZE = 3, 64


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_plain_gradcam():
    """gradcam_atualizado.py behind stand-ins for torchvision and `models`; None when it does not load"""
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.transforms", "models", "models.multimodalIntraInterModal")}
    try:
        tv = types.ModuleType("torchvision")
        tv.transforms = types.ModuleType("torchvision.transforms")
        models = types.ModuleType("models")
        models.multimodalIntraInterModal = types.ModuleType("models.multimodalIntraInterModal")
        sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms, "models": models,
                            "models.multimodalIntraInterModal": models.multimodalIntraInterModal})
        return load(os.path.join(REF, "scripts/benchmark/interpretability/gradcam_atualizado.py"), "reference_gradcam_atualizado")
    except Exception as e:
        print("gradcam_atualizado.py does not load here:", type(e).__name__, e)
        return None
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def last_conv(module):
    last = None
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            last = m
    return last


def run(cls, model, img, meta, targets):
    layer = last_conv(model.image_encoder)
    before = set(layer._forward_hooks) | set(layer._backward_hooks)
    cam = cls(model, layer)
    try:
        return np.stack([cam.generate(img[r // go.VARIANTS:r // go.VARIANTS + 1].clone(), meta[r:r + 1], int(targets[r]))
                         for r in range(meta.shape[0])]).astype(np.float32)
    finally:
        for d in (layer._forward_hooks, layer._backward_hooks):          # the reference's classes keep no handle to remove
            for k in [k for k in d if k not in before]:
                del d[k]


def main():
    model = det_init_(OracleMultimodalModel(**KW)).eval()
    img, meta = go.det_rows(N_IMAGES, SIZE)
    with torch.no_grad():
        logits = model(img.repeat_interleave(go.VARIANTS, dim=0), meta)
    targets = logits.argmax(dim=1).numpy().astype(np.int64)
    pp = run(load(os.path.join(REF, "services/XAI/models/cam.py"), "reference_xai_cam").GradCAMPlusPlus, model, img, meta, targets)
    assert pp.shape == (N_IMAGES * go.VARIANTS, SIZE, SIZE) and np.isfinite(pp).all(), pp.shape
    record = dict(n_images=np.int64(N_IMAGES), variants=np.int64(go.VARIANTS), size=np.int64(SIZE),
                  logits=logits.numpy().astype(np.float32), targets=targets, plusplus_maps=pp)
    plain = load_plain_gradcam()
    if plain is not None:
        assert np.array_equal(run(plain.GradCAMPlusPlus, model, img, meta, targets), pp)
        record["gradcam_maps"] = run(plain.GradCAM, model, img, meta, targets)
    np.savez_compressed(OUT, **record)
    print(OUT, os.path.getsize(OUT), "bytes;", sorted(record), "targets", targets.tolist(), "max", float(pp.max()))


if __name__ == "__main__":
    main()
