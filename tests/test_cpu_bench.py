"""CPU: bench.py --dump-outputs writes the same seeded sample of every parameter / gradient in every run."""
import os

import numpy as np
import torch
import torch.nn as nn

import bench


def _model():
    torch.manual_seed(0)
    m = nn.Sequential(nn.Linear(300, 40), nn.Linear(40, 6))   # 12 000-element weight: sampled; the rest: whole
    with torch.no_grad():
        m[0].weight.copy_(torch.arange(12000.).reshape(40, 300) / 12000)   # distinct, ascending: a value gives its index
    m(torch.randn(8, 300)).sum().backward()
    return m


def test_dump_outputs_is_deterministic_and_sampled(tmp_path):
    logits, loss = torch.randn(8, 6), torch.tensor(1.25)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), _model(), logits, loss)
    bench.dump_outputs(str(b), _model(), logits, loss)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"logits.npy", "loss.npy", "param.0.weight.npy", "grad.0.weight.npy", "param.1.bias.npy", "grad.1.bias.npy"} <= set(names)
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and np.array_equal(x, y), n
    assert np.load(a / "param.0.weight.npy").shape == (bench.DUMP_SAMPLE,)
    assert np.load(a / "param.1.weight.npy").shape == (240,)
    assert np.load(a / "logits.npy").shape == (8, 6) and float(np.load(a / "loss.npy")) == 1.25
    # the sample: distinct flat indices in order, the same ones for parameter and gradient
    m = _model()
    w, g = m[0].weight.detach().reshape(-1).numpy(), m[0].weight.grad.reshape(-1).numpy()
    pw, pg = np.load(a / "param.0.weight.npy"), np.load(a / "grad.0.weight.npy")
    pos = np.searchsorted(w, pw)
    assert np.array_equal(w[pos], pw) and np.all(np.diff(pos) > 0) and np.array_equal(g[pos], pg)


def test_inference_dump_holds_logits_only(tmp_path):
    bench.dump_outputs(str(tmp_path), _model(), torch.randn(4, 6), None)
    assert os.listdir(tmp_path) == ["logits.npy"]
