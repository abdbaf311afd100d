"""`python bench.py --gpus N` starts its own N ranks (the driver's command shape): the parent launches torch.distributed.run as a
child before anything touches the GPU, forwards the ranks' output and returns their exit code."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)


@pytest.fixture
def bench(monkeypatch):
    import bench as B
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return B


def test_no_launch_for_one_gpu_or_inside_a_launcher(bench, monkeypatch):
    assert bench.self_launch(["--steps", "2"]) is None
    assert bench.self_launch(["--gpus", "1"]) is None
    monkeypatch.setenv("WORLD_SIZE", "2")                    # already a rank of torch.distributed.run
    assert bench.self_launch(["--gpus", "2"]) is None


def test_launch_command(bench, monkeypatch):
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setenv("DBMM_DIST_BACKEND", "gloo")
    rc = bench.self_launch(["--gpus", "4", "--steps", "3", "--warmup", "1"])
    assert rc == 7                                           # the children's return code is the parent's
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_rccl_needs_one_gpu_per_rank(bench, monkeypatch, capsys):
    import torch
    monkeypatch.setattr(subprocess, "call", lambda *a, **k: pytest.fail("must not launch"))
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    monkeypatch.delenv("DBMM_DIST_BACKEND", raising=False)
    assert bench.self_launch(["--gpus", "2"]) == 2
    assert "needs 2 GPUs" in capsys.readouterr().err


def test_self_launched_ranks_meet_and_print_one_line():
    """end to end on the CPU: `python bench.py --gpus 2` with no launcher environment -> two ranks under torch.distributed.run on
    127.0.0.1 (gloo), rank 0's JSON line on the parent's stdout, return code 0"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(DBMM_DIST_BACKEND="gloo", DBMM_BENCH_DRYRUN="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    assert lines[0]["n_gpus"] == 2 and lines[0]["max_over_ranks"] == 2.0
    assert sorted(r["rank"] for r in lines[0]["ranks"]) == [0, 1]


def test_failing_rank_fails_the_parent():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(DBMM_DIST_BACKEND="gloo", DBMM_BENCH_DRYRUN="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-such-flag"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0


def test_full_and_dump_outputs_are_options_and_steps_must_be_positive(tmp_path):
    """--full and --dump-outputs DIR parse (dry run, no GPU); --steps 0 is refused before anything runs"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(DBMM_BENCH_DRYRUN="1")
    bench_py = os.path.join(ROOT, "bench.py")
    p = subprocess.run([sys.executable, bench_py, "--gpus", "1", "--steps", "3", "--warmup", "1", "--full",
                        "--dump-outputs", str(tmp_path / "out")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert line["steps"] == 3 and line["warmup"] == 1
    p = subprocess.run([sys.executable, bench_py, "--gpus", "1", "--steps", "0"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--steps" in p.stderr


def test_dump_outputs_float32_within_budget(bench, tmp_path, monkeypatch):
    """what --dump-outputs writes: one float32 .npy per output; an output over its share of the budget becomes a fixed, seeded
    sample of its rows with the row indices beside it (float64)"""
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 16)
    emb = torch.arange(512 * 64, dtype=torch.float64).view(512, 64)           # 128 KiB as float32: over the budget
    outs = {"loss": torch.tensor(1.5), "logits": torch.ones(512, 2, dtype=torch.float16), "embeddings": emb}
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["embeddings.npy", "embeddings_rows.npy", "logits.npy", "loss.npy"]
    total = 0
    for nm in names:
        a, b = np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)      # the same sample every run
        total += a.nbytes
    assert total <= 1 << 16
    assert np.load(tmp_path / "a" / "loss.npy").shape == () and np.load(tmp_path / "a" / "logits.npy").shape == (512, 2)
    rows = np.load(tmp_path / "a" / "embeddings_rows.npy").astype(np.int64)
    sample = np.load(tmp_path / "a" / "embeddings.npy")
    assert 0 < len(rows) < 512 and np.all(np.diff(rows) > 0)
    assert np.array_equal(sample, emb.numpy()[rows].astype(np.float32))
