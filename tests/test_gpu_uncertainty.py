"""-m gpu: mmskin.uncertainty.PredictiveUncertainty end to end on the small custom-cnn one-hot model of tests/test_gpu_sweep.py
(helpers.SMALL, fp32 backbone): Monte-Carlo dropout, test-time augmentation and the risk-coverage of the accumulated rows,
against plain forwards of the same model and against tests/uncertainty_oracle.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import uncertainty_oracle as uo
from gpu_util import DEV
from helpers import SMALL
from mmskin import _autograd, ops
from mmskin._lib import MMSkinError
from mmskin.uncertainty import STATS, PredictiveUncertainty
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_, det_inputs
from oracle.model import OracleMultimodalModel

pytestmark = pytest.mark.gpu

MECHS = ["crossattention", "metablock", "att-intramodal+residual+cross-attention-metadados"]
BATCHES = [(0, 5), (5, 8)]                                                       # a batch of 5, then one of 3
_models = {}


def model(mech):
    """the HIP model with the oracle's deterministic weights, built once per fusion and left in eval mode"""
    if mech not in _models:
        os.environ["MMSKIN_BACKBONE_DTYPE"] = "fp32"
        kw = dict(SMALL, attention_mecanism=mech)
        cpu = det_init_(OracleMultimodalModel(**kw), salt=1)
        hip = M.MultimodalModel(**dict(kw, device=DEV))
        hip.load_state_dict(cpu.state_dict(), strict=True)
        _models[mech] = hip.to(DEV).eval()
    return _models[mech]


def case():
    img, meta, lab = det_inputs(8, 32, 20, 6)
    return img.to(DEV), meta.to(DEV), lab.to(DEV)


def flags(m):
    return [mod.training for mod in m.modules()]


def host(result):
    return {k: getattr(result, k).cpu().numpy() for k in ("mean_prob", "prob_std", "votes", "pred", "stats")}


def check_against_oracle(got, logits, what):
    want = uo.reduce(logits.cpu().numpy())
    assert np.array_equal(got["pred"], want["pred"]) and np.array_equal(got["votes"], want["votes"]), what
    assert np.array_equal(got["stats"][:, 5], want["stats"][:, 5]), what
    for key in ("mean_prob", "prob_std", "stats"):
        print(f"{what} {key}: max |got - want| / max(|want|, 1) = {uo.worst(got[key], want[key]):.3e}")
        assert uo.close(got[key], want[key]), (what, key)


@pytest.mark.parametrize("mech", MECHS)
def test_mc_dropout_end_to_end(mech):
    hip = model(mech)
    img, meta, lab = case()
    before_flags, before_counter = flags(hip), _autograd._dropout_counter[0]
    encodes = []
    encode = hip.encode_image
    hip.encode_image = lambda image: (encodes.append(tuple(image.shape)), encode(image))[1]
    try:
        pu = PredictiveUncertainty(hip, DEV, rows_per_head_call=16)               # 40 and 24 rows: passes in calls of 3 + 3 + 2, and 5 + 3
        results = [pu.mc_dropout(img[r0:r1], meta[r0:r1], passes=8, seed=11, labels=lab[r0:r1]) for r0, r1 in BATCHES]
        assert encodes == [(5, 3, 32, 32), (3, 3, 32, 32)]                        # the encoder ran once per batch
    finally:
        del hip.encode_image
    for (r0, r1), res in zip(BATCHES, results):                                   # (a)
        assert tuple(res.logits.shape) == (8, r1 - r0, 6) and res.logits.dtype == torch.float32
        check_against_oracle(host(res), res.logits, f"{mech} rows {r0}:{r1}")
        with torch.no_grad():
            plain = hip(img[r0:r1], meta[r0:r1]).float()
        assert torch.equal(res.eval_logits, plain) and torch.equal(res.pred_eval.long(), plain.argmax(dim=1))
    assert pu.n_samples == 8 and results[-1].n_samples == 8
    for key in ("mean_prob", "prob_std", "votes", "pred", "stats"):               # the accumulated rows are the 8, in order
        assert torch.equal(getattr(pu, key), torch.cat([getattr(r, key) for r in results])), key
    assert torch.equal(pu.labels, lab.long()) and tuple(pu.stats.shape) == (8, 7)
    assert float(pu.stats[:, STATS.index("mutual_information")].max()) > 0        # the passes disagree: the dropouts were on
    # (b) the same arguments repeat bit for bit, another seed or another chunking draws other masks
    again = PredictiveUncertainty(hip, DEV, rows_per_head_call=16)
    other = PredictiveUncertainty(hip, DEV, rows_per_head_call=16)
    wider = PredictiveUncertainty(hip, DEV, rows_per_head_call=40)
    r0, r1 = BATCHES[0]
    rerun = again.mc_dropout(img[r0:r1], meta[r0:r1], passes=8, seed=11, labels=lab[r0:r1])
    assert torch.equal(rerun.logits, results[0].logits) and torch.equal(rerun.stats, results[0].stats)
    assert not torch.equal(other.mc_dropout(img[r0:r1], meta[r0:r1], passes=8, seed=12).logits, results[0].logits)
    assert not torch.equal(wider.mc_dropout(img[r0:r1], meta[r0:r1], passes=8, seed=11).logits, results[0].logits)
    # (c) one image and metadata row four times: 32 different draws
    same = PredictiveUncertainty(hip, DEV).mc_dropout(img[:1].repeat(4, 1, 1, 1), meta[:1].repeat(4, 1), passes=8, seed=3)
    rows = same.logits.reshape(32, 6)
    assert len({tuple(r) for r in rows.cpu().numpy().tolist()}) == 32
    assert torch.equal(same.eval_logits[0], same.eval_logits[3])                  # ... of one deterministic row
    # (e) nothing of the model or of the global dropout counter has moved
    assert flags(hip) == before_flags and not hip.training and _autograd._dropout_counter[0] == before_counter
    assert not _autograd._dropout_streams


@pytest.mark.parametrize("mech", MECHS)
def test_mc_dropout_without_dropout_is_the_plain_forward(mech):
    """(d) every Dropout.p at 0: each pass is model(images, metadata) bit for bit, and the passes carry no information"""
    hip = model(mech)
    img, meta, _ = case()
    drops = [m for m in hip.modules() if isinstance(m, nn.Dropout)]
    saved = [m.p for m in drops]
    try:
        for m in drops:
            m.p = 0.0
        res = PredictiveUncertainty(hip, DEV).mc_dropout(img[:5], meta[:5], passes=4, seed=0)
        with torch.no_grad():
            plain = hip(img[:5], meta[:5]).float()
    finally:
        for m, p in zip(drops, saved):
            m.p = p
    for t in range(4):
        assert torch.equal(res.logits[t], plain), t
    mi = res.stat("mutual_information")
    print(f"{mech}: max mutual information of 4 equal passes {float(mi.max()):.3e}")
    assert float(mi.max()) <= 1e-14 and bool((res.stat("variation_ratio") == 0).all())


def test_mc_dropout_refuses_train_mode_and_restores_after_an_error():
    hip = model("metablock")
    img, meta, _ = case()
    pu = PredictiveUncertainty(hip, DEV)
    hip.train()
    try:
        with pytest.raises(MMSkinError, match="eval mode"):                       # (f)
            pu.mc_dropout(img[:2], meta[:2], passes=2)
    finally:
        hip.eval()
    before_flags, before_counter = flags(hip), _autograd._dropout_counter[0]
    calls, fuse = [], hip.fuse

    def failing(feats, metas):                                                    # the second head call is the first stochastic one
        calls.append(feats.shape[0])
        if len(calls) == 2:
            raise RuntimeError("boom")
        return fuse(feats, metas)

    hip.fuse = failing
    try:
        with pytest.raises(RuntimeError, match="boom"):
            pu.mc_dropout(img[:2], meta[:2], passes=2)
    finally:
        del hip.fuse
    assert calls == [2, 4]
    assert flags(hip) == before_flags and _autograd._dropout_counter[0] == before_counter and not _autograd._dropout_streams
    with pytest.raises(MMSkinError, match="MAX_PASSES"):
        pu.mc_dropout(img[:2], meta[:2], passes=ops.UNCERTAINTY_MAX_PASSES + 1)
    assert pu.n_samples == 0


# --------------------------------------------------------------------------------------------------------------- tta
def torch_view(x, v):
    y = torch.rot90(x, v & 3, (2, 3))
    return (torch.flip(y, (3,)) if v & 4 else y).contiguous()


@pytest.mark.parametrize("mech", MECHS[:2])
def test_tta_views_are_plain_forwards(mech):
    hip = model(mech)
    img, meta, lab = case()
    pu = PredictiveUncertainty(hip, DEV, images_per_model_call=5)                # one view of the batch per model call
    res = pu.tta(img[:5], meta[:5], views="dihedral", labels=lab[:5])
    assert tuple(res.logits.shape) == (8, 5, 6)
    with torch.no_grad():
        for v in range(8):
            assert torch.equal(res.logits[v], hip(torch_view(img[:5], v), meta[:5]).float()), v
    assert torch.equal(res.eval_logits, res.logits[0])
    check_against_oracle(host(res), res.logits, f"{mech} tta")
    sub = PredictiveUncertainty(hip, DEV, images_per_model_call=5).tta(img[:5], meta[:5], views=[1, 6])
    assert torch.equal(sub.logits[0], res.logits[1]) and torch.equal(sub.logits[1], res.logits[6]) and sub.eval_logits is None
    # ragged model calls (40 images in calls of 16): the same views, within the project's fp32 logits tolerance
    ragged = PredictiveUncertainty(hip, DEV, images_per_model_call=16).tta(img[:5], meta[:5], views="dihedral")
    err = (ragged.logits - res.logits).abs()
    print(f"{mech}: max |ragged - per-view calls| {float(err.max()):.3e}")
    assert bool((err <= 1e-5 + 1e-3 * res.logits.abs()).all())


def test_tta_flips_run_on_a_non_square_batch_and_dihedral_is_refused():
    hip = model("metablock")
    img, meta, lab = case()
    tall = img[:3, :, :, :24].contiguous()                                        # [3, 3, 32, 24]
    pu = PredictiveUncertainty(hip, DEV, images_per_model_call=3)
    res = pu.tta(tall, meta[:3], views="flips", labels=lab[:3])
    assert tuple(res.logits.shape) == (4, 3, 6) and pu.n_samples == 3
    with torch.no_grad():
        for t, v in enumerate((0, 2, 4, 6)):
            assert torch.equal(res.logits[t], hip(torch_view(tall, v), meta[:3]).float()), v
    kept = pu.stats.clone()
    with pytest.raises(MMSkinError, match="H == W"):
        pu.tta(tall, meta[:3], views="dihedral", labels=lab[:3])
    with pytest.raises(MMSkinError, match="H == W"):
        pu.tta(tall, meta[:3], views=[0, 3], labels=lab[:3])
    assert pu.n_samples == 3 and torch.equal(pu.stats, kept)                      # nothing was written


# --------------------------------------------------------------------------------------------------------------- the fold
def test_from_logits_risk_coverage_and_save(tmp_path):
    """the small model's own predictions on 64 drawn rows, as 8 Monte-Carlo passes handed over as logits"""
    hip = model("metablock")
    img, meta, lab = det_inputs(64, 32, 20, 6)
    src = PredictiveUncertainty(hip, DEV).mc_dropout(img.to(DEV), meta.to(DEV), passes=8, seed=5)
    logits = src.logits
    labels = torch.where(torch.arange(64, device=DEV) % 3 == 0, src.pred.long(), lab.to(DEV))   # a third right for sure: both kinds of row
    pu = PredictiveUncertainty(None, DEV)
    first = pu.from_logits(logits[:, :40], labels=labels[:40])                    # a strided slice, read in place
    pu.from_logits(logits[:, 40:], labels=labels[40:])
    assert torch.equal(pu.stats, src.stats) and torch.equal(pu.pred, src.pred) and first.eval_logits is None and pu.pred_eval is None
    stats, wrong = pu.stats.cpu().numpy(), (pu.pred.long() != labels).cpu().numpy().astype(np.uint8)
    assert 0 < wrong.sum() < 64
    for k, name in enumerate(STATS):
        rc = pu.risk_coverage(score=name)
        score = -stats[:, k] if name in ("confidence", "margin") else stats[:, k]
        want_counts = uo.risk_counts(score, wrong)
        want = uo.risk_summary(want_counts, wrong)
        got = rc.summary.cpu().numpy()
        print(f"{name}: aurc {got[0]:.6f} optimal {got[1]:.6f} e-aurc {got[2]:.6f} error auroc {got[3]:.6f}")
        assert np.array_equal(rc.counts.cpu().numpy(), want_counts), name
        assert uo.close(got, want), (name, got, want)
        assert rc.aurc == got[0] and rc.n == 64 and rc.n_wrong == int(wrong.sum()) and rc.score_name == name
        cov, risk = (t.cpu().numpy() for t in rc.curve())
        want_cov, want_risk = uo.risk_curve(want_counts)
        assert np.array_equal(cov, want_cov) and np.array_equal(risk, want_risk) and len(cov) == rc.n_distinct
        assert rc.risk_at_coverage(1.0) == want[4] and rc.coverage_at_risk(1.0) == 1.0
    path = tmp_path / "uncertainty.npz"
    pu.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(["mean_prob", "prob_std", "votes", "pred", "stats", "labels", "stat_names"])
        for key in ("mean_prob", "prob_std", "votes", "pred", "stats", "labels"):
            assert np.array_equal(z[key], getattr(pu, key).cpu().numpy(), equal_nan=True), key
        assert tuple(z["stat_names"]) == STATS
    bad = logits.clone()
    bad[2, 7, 1] = float("inf")
    nan_rows = PredictiveUncertainty(None, DEV)
    nan_rows.from_logits(bad, labels=labels)
    with pytest.raises(ValueError, match="NaN"):                                  # the driver refuses a score column that holds NaN
        nan_rows.risk_coverage(score="confidence")
    pu.reset()
    assert pu.n_samples == 0 and pu.stats is None
