"""mmskin.calibration end to end on the GPU: Calibration (host and device inputs, from_fold_dir, the resampled study and its
weights, replicates_per_call, quantile bins) and TemperatureScaling (the root, its special cases, probabilities against logits)."""
import numpy as np
import pytest
import torch

import bootstrap_oracle as bo
import calibration_oracle as co
from mmskin import Calibration, TemperatureScaling, ops
from calibration_oracle import fold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12


def same_point(a, b, tol=TOL):
    for m in ops.CALIBRATION_METRICS + ops.CALIBRATION_CLASS_METRICS:
        assert np.allclose(a.point[m], b.point[m], rtol=tol, atol=0, equal_nan=True), m


@pytest.mark.parametrize("binning", ["uniform", "quantile"])
def test_host_and_device_inputs_agree(binning, tmp_path):
    N, K = 257, 6
    probs, labels = fold(N, K, "eighths" if binning == "uniform" else "continuous")
    labels[5] = -1                                                                                     # dropped first
    cal = Calibration(n_bins=8, binning=binning)
    host = cal.evaluate(probs, labels)
    device = cal.evaluate(torch.from_numpy(probs).to(DEV), torch.from_numpy(labels).to(DEV))
    assert np.array_equal(host.tables, device.tables) and np.array_equal(host.edges, device.edges)   # the integers: exactly
    assert host.tables[0, :, 0].sum() == N - 1
    same_point(host, device)
    keep = labels >= 0
    edges = co.uniform_edges(K, 8) if binning == "uniform" else co.quantile_edges(probs[keep], 8)
    want = co.metrics(co.tables(co.codes(probs[keep], labels[keep], edges), 8), co.sums(probs[keep], labels[keep]))
    assert np.allclose([device.point[m] for m in ops.CALIBRATION_METRICS], want[:6], rtol=TOL, atol=0)
    assert np.allclose(device.point["per_class_ece"], want[6:], rtol=TOL, atol=0)
    np.save(tmp_path / "probabilities.npy", probs)
    np.save(tmp_path / "labels.npy", labels)
    np.save(tmp_path / "predictions.npy", probs.argmax(axis=1))
    from_dir = cal.from_fold_dir(str(tmp_path))
    assert np.array_equal(from_dir.tables, host.tables)
    same_point(from_dir, host, tol=0)
    if binning == "quantile":                                                                          # tie-free: ceil(N / n_bins) +- 1 rows a bin
        per_bin = -(-(N - 1) // 8)
        assert (np.abs(host.tables[:, :, 0] - per_bin) <= 1).all()


@pytest.mark.parametrize("stratified", [False, True])
def test_resampled_study(stratified):
    N, K, B, n_bins = 200, 3, 24, 10
    probs, labels = fold(N, K, "continuous")
    rep = Calibration(n_bins).evaluate(probs, labels, n_resamples=B, seed=5, confidence=0.9, stratified=stratified)
    w = bo.weights(5, N, 0, B, labels if stratified else None)                                         # the bootstrap's own resamples
    tables = ops.bootstrap_tables(torch.from_numpy(probs).to(DEV), torch.from_numpy(labels).to(DEV)) if stratified else None
    assert np.array_equal(ops.bootstrap_weights(5, N, B, DEV, tables=tables).cpu().numpy(), w)
    the_codes = co.codes(probs, labels, co.uniform_edges(K, n_bins))
    want = np.stack([co.metrics(co.tables(the_codes, n_bins, w[b]), co.sums(probs, labels, w[b])) for b in range(B)], axis=1)
    got = np.concatenate([np.stack([rep.replicates[m] for m in ops.CALIBRATION_METRICS]), rep.replicates["per_class_ece"].T])
    assert np.allclose(got, want, rtol=TOL, atol=0)
    summary = bo.summary(want, 0.9)
    for k, m in enumerate(ops.CALIBRATION_METRICS):
        assert rep.n_valid[m] == B
        assert np.allclose([rep.mean[m], rep.std[m], rep.low[m], rep.high[m]], summary[1:, k], rtol=1e-10, atol=0), m
        assert rep.interval(m) == (rep.low[m], rep.high[m]) and rep.low[m] <= rep.high[m]
    assert rep.low["per_class_ece"].shape == (K,) and rep.replicates["per_class_ece"].shape == (B, K)
    same_point(rep, Calibration(n_bins).evaluate(probs, labels))
    for step in (1, 7, B):
        cut = Calibration(n_bins, replicates_per_call=step).evaluate(probs, labels, n_resamples=B, seed=5, confidence=0.9, stratified=stratified)
        for m in rep.replicates:
            assert np.array_equal(cut.replicates[m], rep.replicates[m]), (step, m)
            assert np.array_equal(cut.low[m], rep.low[m]) and np.array_equal(cut.std[m], rep.std[m]), (step, m)


def fitted_fold(N=2000, K=5, seed=3):
    rng = np.random.default_rng(seed)
    z0 = rng.normal(0, 1, (N, K))
    p0 = np.exp(z0) / np.exp(z0).sum(axis=1, keepdims=True)
    labels = np.array([rng.choice(K, p=p) for p in p0]).astype(np.int64)                              # drawn from softmax(z0)
    return (3 * z0).astype(np.float32), labels


def test_temperature_scaling_finds_the_root_and_closes_the_loop():
    z, labels = fitted_fold()
    ts = TemperatureScaling().fit(torch.from_numpy(z).to(DEV), torch.from_numpy(labels).to(DEV), from_logits=True)
    _, g, h = co.temperature_stats(z, labels, [ts.beta])[0]                                            # the oracle at the device's beta
    print(f"T = {ts.temperature:.6f}, launches = {ts.n_launches}, |g| / (h beta) = {abs(g) / (h * ts.beta):.3e}")
    assert abs(g) / (h * ts.beta) <= 1e-9
    assert 2.5 < ts.temperature < 3.6 and not ts.at_bound and 2 <= ts.n_launches <= 30
    assert ts.nll_after <= ts.nll_before
    nll = co.temperature_stats(z, labels, [1.0, ts.beta])[:, 0] / len(labels)
    assert np.allclose([ts.nll_before, ts.nll_after], nll, rtol=TOL, atol=0)
    calibrated = ts.apply(z)
    assert isinstance(calibrated, np.ndarray) and calibrated.dtype == np.float32 and calibrated.shape == z.shape
    cal = Calibration(15)
    before = cal.evaluate(co.softmax(z, 1.0).astype(np.float32), labels)
    after = cal.evaluate(calibrated, labels)
    assert after.point["nll"] < before.point["nll"] and after.point["ece"] < before.point["ece"]
    assert abs(after.point["nll"] - ts.nll_after) <= 1e-6                                              # fp32 rounding of the calibrated rows


def test_temperature_from_probabilities_agrees_with_logits():
    z, labels = fitted_fold()
    probs = co.softmax(z, 1.0).astype(np.float32)
    a = TemperatureScaling().fit(z, labels, from_logits=True)
    b = TemperatureScaling().fit(probs, labels)
    print(f"T from logits {a.temperature!r}, from probabilities {b.temperature!r}, relative gap {abs(a.temperature - b.temperature) / a.temperature:.3e}")
    assert abs(a.temperature - b.temperature) <= 1e-6 * a.temperature
    assert np.abs(b.apply(probs) - a.apply(z)).max() <= 1e-5


def test_temperature_special_cases():
    K = 3
    labels = (np.arange(12) % K).astype(np.int64)
    sure = (5 * np.eye(K)[labels]).astype(np.float32)                                                  # every row confidently right
    ts = TemperatureScaling(bounds=(0.125, 8.0)).fit(sure, labels, from_logits=True)
    assert ts.at_bound and ts.temperature == 0.125 and ts.n_launches == 1 and ts.nll_after < ts.nll_before
    wrong = (5 * np.eye(K)[(labels + 1) % K]).astype(np.float32)                                       # every row confidently wrong
    ts = TemperatureScaling(bounds=(0.125, 8.0)).fit(wrong, labels, from_logits=True)
    assert ts.at_bound and ts.temperature == 8.0 and ts.nll_after < ts.nll_before
    flat = TemperatureScaling().fit(np.full((7, K), 1 / 3, dtype=np.float32), labels[:7])             # h = 0: T does nothing
    assert flat.temperature == 1.0 and not flat.at_bound and flat.nll_before == flat.nll_after == pytest.approx(np.log(3), rel=1e-7)
    one = TemperatureScaling().fit(np.array([[2.0, 0.0, -1.0]], dtype=np.float32), np.array([0]), from_logits=True)   # N = 1, right
    assert one.at_bound and one.temperature == 1 / 64
    z1 = np.array([[2.0, 1.5, -4.0]], dtype=np.float32)                                                # N = 1, the label second: a root
    one = TemperatureScaling().fit(z1, np.array([1]), from_logits=True)
    beta, at_bound = co.fit_temperature(z1, np.array([1]))
    assert not one.at_bound and not at_bound and abs(one.beta - beta) <= 1e-9 * beta
