"""-m gpu: mmskin.faithfulness end to end on the HIP model (resnet-18 + one-hot metadata + crossattention, fp32 backbone, 64x64
images, N = 2, S = 8, chunk = 16): CamFaithfulness.evaluate against a loop that runs the restatement's perturbed images
(tests/faithfulness_oracle.py) through the same model at the same chunk size, and compare_cam_methods against the CAM classes
run on their own.

Tolerance on a probability: the one tests/test_gpu_scorecam.py applies to soft-max scores, 0.5 * max over classes of
(1e-4 + 1e-3 |logit|) -- the fp32 eval logits tolerance of this encoder, halved because a soft-max output moves at most half
as much as its largest logit error.  The model inputs of both sides are bit-identical, so nothing looser is warranted."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import faithfulness_oracle as fo
from gpu_util import DEV
from helpers import SMALL
from mmskin.cam import GradCAM, GradCAMPlusPlus, ScoreCAM
from mmskin.faithfulness import CAM_METHODS, CamFaithfulness, compare_cam_methods
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_, det_inputs
from oracle.model import OracleMultimodalModel

pytestmark = pytest.mark.gpu

N, SIZE, S, CHUNK = 2, 64, 8, 16
P = 2 * S + 3


def hip_model(**kw):
    os.environ["MMSKIN_BACKBONE_DTYPE"] = "fp32"
    cpu = det_init_(OracleMultimodalModel(**dict(kw, device="cpu")))
    hip = M.MultimodalModel(**dict(kw, device=DEV))
    hip.load_state_dict(cpu.state_dict(), strict=True)
    return hip.to(DEV).eval()


def last_conv(module):
    last = None
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            last = m
    return last


def saliency_map():
    """smooth bumps, rectified like a CAM (about half of the pixels tie at zero), scaled into [0, 1]"""
    y, x = np.meshgrid(np.linspace(-1, 1, SIZE), np.linspace(-1, 1, SIZE), indexing="ij")
    maps = [np.exp(-((x - 0.3) ** 2 + (y + 0.2) ** 2) * 4) - 0.35, np.cos(3 * x) * np.sin(2 * y + 0.5)]
    return np.maximum(np.stack(maps), 0).astype(np.float32)


@pytest.fixture(scope="module")
def setup():
    model = hip_model(**dict(SMALL, cnn_model_name="resnet-18", attention_mecanism="crossattention"))
    img, meta, _ = det_inputs(N, SIZE, 20, 6)
    sal = saliency_map()
    with torch.no_grad():
        clean = model(img.to(DEV), meta.to(DEV)).float().cpu().numpy()
    return {"model": model, "img": img, "meta": meta, "sal": sal, "clean": clean}


def loop_logits(model, rows, row_image, meta, chunk):
    """the restatement's images through the same model, `chunk` rows per forward, the last chunk padded with zero rows"""
    R = rows.shape[0]
    out = []
    with torch.no_grad():
        for r0 in range(0, R, chunk):
            batch = np.zeros((chunk,) + rows.shape[1:], dtype=np.float32)
            idx = np.zeros(chunk, dtype=np.int64)
            n = min(chunk, R - r0)
            batch[:n], idx[:n] = rows[r0:r0 + n], row_image[r0:r0 + n]
            out.append(model(torch.from_numpy(batch).to(DEV), meta[idx].to(DEV)).float().cpu().numpy()[:n])
    return np.concatenate(out)


def probability_tolerance(logits):
    """per row of logits [R, K]"""
    return 0.5 * (1e-4 + 1e-3 * np.abs(logits)).max(axis=-1)


@pytest.fixture(scope="module")
def reference(setup):
    """the loop's logits and the restatement's curves of them, computed once"""
    rows = fo.perturbed_rows(setup["img"].numpy(), setup["sal"], S, "blur")
    row_image = fo.row_table(N, S)[:, 0]
    logits = loop_logits(setup["model"], rows, row_image, setup["meta"], CHUNK)
    return {"logits": logits, "tol": probability_tolerance(logits).reshape(N, P)}


def evaluate(setup, chunk=CHUNK, target=None, baseline="blur"):
    scorer = CamFaithfulness(setup["model"], DEV, steps=S, baseline=baseline, chunk=chunk)
    return scorer.evaluate(setup["img"].to(DEV), setup["meta"].to(DEV), setup["sal"], target)


def check_against(res, want, tol):
    """res: FaithfulnessResult on the host; want: the restatement's curves of the loop's logits; tol [N, P] per model row"""
    for name, lo in (("deletion", 0), ("insertion", S + 1)):
        got = getattr(res, name).numpy()
        err = np.abs(got - want[name])
        print(f"{name}: max error {err.max():.3e}, smallest tolerance {tol[:, lo:lo + S + 1].min():.3e}")
        assert got.shape == (N, S + 1) and got.dtype == np.float64 and (err <= tol[:, lo:lo + S + 1]).all()
    # an area is a convex combination of its curve's values: it moves at most as much as the worst of them
    assert (np.abs(res.deletion_auc.numpy() - want["deletion_auc"]) <= tol[:, :S + 1].max(axis=1)).all()
    assert (np.abs(res.insertion_auc.numpy() - want["insertion_auc"]) <= tol[:, S + 1:2 * S + 2].max(axis=1)).all()


def test_evaluate_matches_a_loop_through_the_same_model(setup, reference):
    res = evaluate(setup)
    assert res.deletion.is_cuda and res.deletion.dtype == torch.float64 and res.target.dtype == torch.int32
    res = res.cpu()
    want = fo.curves(reference["logits"], S, N)
    assert res.target.tolist() == want["target"].tolist()
    check_against(res, want, reference["tol"])
    # the scalars are the restatement's of the curves the call itself returned
    again = fo.curves(reference["logits"], S, N)
    for name in ("deletion_auc", "insertion_auc"):
        curve = getattr(res, name.split("_")[0]).numpy()
        assert np.abs(getattr(res, name).numpy() - [fo.trapezoid(c) for c in curve]).max() <= 1e-12
        assert abs(float(getattr(res, "mean_" + name)) - float(getattr(res, name).mean())) <= 1e-12
    assert ((res.average_drop.numpy() >= 0) & (res.average_drop.numpy() <= 1)).all()
    assert set(res.increase.tolist()) <= {0.0, 1.0} and again["increase"].shape == (N,)
    assert abs(float(res.mean_average_drop) - float(res.average_drop.mean())) <= 1e-12
    assert abs(float(res.mean_increase) - float(res.increase.mean())) <= 1e-12


def test_curve_end_points_are_the_clean_forward(setup):
    """deletion at k = 0 and insertion at k = S see the unmodified image; with target_class=None the targets are the argmax of
    the clean forward"""
    clean = setup["clean"]
    res = evaluate(setup).cpu()
    assert res.target.tolist() == clean.argmax(axis=1).tolist()
    e = np.exp(clean.astype(np.float64) - clean.max(axis=1, keepdims=True))
    prob = (e / e.sum(axis=1, keepdims=True))[np.arange(N), clean.argmax(axis=1)]
    tol = probability_tolerance(clean)
    print(f"end points: {np.abs(res.deletion[:, 0].numpy() - prob).max():.3e} / {np.abs(res.insertion[:, S].numpy() - prob).max():.3e}, "
          f"tolerance {tol.min():.3e}")
    assert (np.abs(res.deletion[:, 0].numpy() - prob) <= tol).all()
    assert (np.abs(res.insertion[:, S].numpy() - prob) <= tol).all()


@pytest.mark.parametrize("target", [3, "tensor"])
def test_given_targets_and_a_chunk_that_does_not_divide_the_rows(setup, reference, target):
    """N * P = 38 rows: chunk 19 divides them, chunk 16 leaves a ragged chunk of 6, chunk 7 one of 3"""
    classes = [3, 3] if target == 3 else [4, 1]
    given = 3 if target == 3 else torch.tensor(classes, device=DEV)
    want = fo.curves(reference["logits"], S, N, classes)
    for chunk in (19, 16, 7):
        res = evaluate(setup, chunk=chunk, target=given).cpu()
        assert res.target.tolist() == classes
        check_against(res, want, reference["tol"])
    with pytest.raises(ValueError, match="outside"):
        evaluate(setup, target=6)


@pytest.mark.parametrize("baseline", ["zero", "mean"])
def test_other_baselines_against_the_loop(setup, baseline):
    rows = fo.perturbed_rows(setup["img"].numpy(), setup["sal"], S, baseline)
    logits = loop_logits(setup["model"], rows, fo.row_table(N, S)[:, 0], setup["meta"], CHUNK)
    res = evaluate(setup, baseline=baseline).cpu()
    check_against(res, fo.curves(logits, S, N, res.target.tolist()), probability_tolerance(logits).reshape(N, P))


def test_compare_cam_methods(setup):
    """finite scores for all three methods; each method's maps are what its class returns on its own"""
    model, img, meta = setup["model"], setup["img"].to(DEV), setup["meta"].to(DEV)
    layer = last_conv(model.image_encoder)
    out = compare_cam_methods(model, layer, img, meta, steps=S, chunk=CHUNK)
    assert tuple(out) == CAM_METHODS and len(layer._forward_hooks) == 0
    target = torch.from_numpy(setup["clean"].argmax(axis=1)).to(DEV)
    own = {}
    for name, cls in (("gradcam", GradCAM), ("gradcam++", GradCAMPlusPlus)):
        cam = cls(model, layer)
        try:
            own[name] = cam.generate_batch(img, meta, target).cpu().numpy()
        finally:
            cam.remove_hook()
    cam = ScoreCAM(model, layer, DEV, chunk=CHUNK)
    try:
        own["scorecam"] = np.stack([cam.generate_heatmap(img[i:i + 1], meta[i:i + 1], int(target[i])) for i in range(N)])
    finally:
        cam.remove_hook()
    for name in CAM_METHODS:
        maps, res = out[name]["maps"], out[name]["result"].cpu()
        assert tuple(maps.shape) == (N, SIZE, SIZE) and np.array_equal(maps.cpu().numpy(), own[name]), name
        assert res.target.tolist() == target.tolist()
        for field in ("deletion", "insertion", "deletion_auc", "insertion_auc", "average_drop", "increase"):
            v = getattr(res, field).numpy()
            assert np.isfinite(v).all() and (v >= 0).all() and (v <= 1).all(), (name, field)
        for field in ("mean_deletion_auc", "mean_insertion_auc", "mean_average_drop", "mean_increase"):
            assert np.isfinite(float(getattr(res, field))), (name, field)
