"""bench.py's plain run on the MI355X: the headline line alone, exactly --steps timed steps, and --dump-outputs writing what the
last timed step returned (the embeddings are the encode of the benchmark's own seeded images)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, relerr

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["unit"] == "images/sec" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0
    assert abs(line["value"] - 1024 * 1e3 / line["ms_per_step"]) < 1e-3 * line["value"]
    assert not {"roofline", "extra_legs", "cpu_baseline", "fp32_input_mfma"} & set(line)      # those need --full

    emb, logits, loss = (np.load(out / f"{nm}.npy") for nm in ("embeddings", "logits", "loss"))
    assert emb.dtype == logits.dtype == loss.dtype == np.float32
    assert emb.shape == (1024, 1024) and logits.shape == (1024, 2) and loss.shape == ()
    assert np.isfinite(emb).all() and np.isfinite(logits).all() and np.isfinite(loss)

    import bench
    _, model, _, R, _, _ = bench.build_step("RN50", torch.device("cuda"), 1, 0, 1024)
    images, _, _ = bench.synthetic_batch(R, 1024, 1, 0, torch.device("cuda"))
    with torch.no_grad():
        want = model.encode_image(images).cpu()
    assert relerr(torch.from_numpy(emb), want) < 1e-6
