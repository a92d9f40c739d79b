"""-m gpu: a plain `bench.py` run (no --full) times exactly --steps steps, prints the headline line without the
--full extras, and --dump-outputs writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dump(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "images/sec" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"] is None and "cpu_baseline" not in d
    names = os.listdir(tmp_path)
    total = sum(os.path.getsize(tmp_path / n) for n in names)
    assert total <= 64 << 20
    logits, loss = np.load(tmp_path / "logits.npy"), np.load(tmp_path / "loss.npy")
    assert logits.shape == (256, 6) and logits.dtype == np.float32 and np.isfinite(logits).all()
    assert abs(float(loss) - d["loss"]) <= 1e-4
    params = [n for n in names if n.startswith("param.image_encoder.")]
    grads = [n for n in names if n.startswith("grad.image_encoder.")]
    assert params and len(grads) == len(params)
    for n in params + grads:
        a = np.load(tmp_path / n)
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size <= 4096 and np.isfinite(a).all(), n
