"""tl_method linear_probing and adapter_reg against the reference's OWN driver: tests/golden/schedule_*.npz hold what final_main.py's
train_all_epochs (train_one_epoch / train_reg_one_epoch / validate / validate_zs / balance_val, unmodified) produced on a synthetic
embedding set (tools/make_golden_schedules.py), per pass: batch index stream, learning rates, loss, accuracy and the integer (n, correct)
counters per group, plus the same run on inputs scaled by 1 + 2^-23 and 1 + 2^-20 (the reference's own sensitivity).
trainer.train_all_epochs replays each on the MI355X from the same seeds, every step one fused C call."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN
from dbmm_amd import optim, synth, trainer

pytestmark = pytest.mark.gpu


def _sample(t, n=256):
    f = t.detach().double().flatten()
    return f[::max(1, f.numel() // n)][:n].float().numpy()


@pytest.fixture(scope="module", params=["schedule_adapter_reg.npz", "schedule_adapter_reg_cls.npz", "schedule_linear_probing.npz"])
def run(request, tmp_path_factory):
    g = np.load(os.path.join(GOLDEN, request.param), allow_pickle=False)
    cfg, o = json.loads(str(g["config"])), json.loads(str(g["opt"]))
    d = tmp_path_factory.mktemp("schedules")
    tcls, tspu, tgrp = synth.embedding_text(cfg["seed"], cfg["dim"])
    for key, m, cols in (("text_embedding_dir", tcls, ["c0", "c1"]), ("text_spurious_embedding_dir", tspu, ["s0", "s1"]),
                         ("text_group_embedding_dir", tgrp, ["g0", "g1", "g2", "g3"])):
        o[key] = os.path.join(d, key + ".json")
        json.dump({n: m[:, i].numpy().tolist() for i, n in enumerate(cols)}, open(o[key], "w"))
    opt = SimpleNamespace(**o)
    tables = []
    for split, n in (("train", cfg["n_train"]), ("val", cfg["n_val"]), ("test", cfg["n_test"])):
        x, y, c = synth.embedding_dataset(cfg["seed"], split, n, cfg["dim"])
        tables.append(trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda"))
    optim.set_seed(opt.random_seed)
    log = []
    final = trainer.train_all_epochs(opt, *tables, log=log)
    return g, opt, log, final


def test_initialisation_and_batches_are_the_references(run):
    g, opt, log, _ = run
    inits = [e for e in log if e["kind"] == "init"]
    assert len(inits) == 1
    for k, v in inits[0]["state"].items():
        assert np.array_equal(_sample(v), g[f"init0/{k}_sample"]), k
    passes = [e for e in log if e["kind"] in ("train1", "train_reg", "validate", "validate_zs")]
    assert len(passes) == int(g["n_phases"])
    for i, e in enumerate(passes):
        assert e["kind"] == str(g[f"p{i}/kind"]), i
        if e["kind"] in ("train1", "train_reg"):
            assert np.array_equal(e["order"], g[f"p{i}/idx"]), i
        if e["kind"] == "train_reg":
            assert e["use_group"] == bool(g[f"p{i}/use_group"])
        assert np.array_equal(e["counts"][:, 0], g[f"p{i}/counts"][:, 0]), i


def test_counts_losses_and_worst_group_accuracy(run):
    g, opt, log, final = run
    keys = [str(k) for k in g["acc_keys"]]
    passes = [e for e in log if e["kind"] in ("train1", "train_reg", "validate", "validate_zs")]
    flips = 0
    for i, e in enumerate(passes):
        ref = g[f"p{i}/counts"]
        sens = np.maximum(np.abs(g[f"p{i}/counts_1ulp"] - ref), np.abs(g[f"p{i}/counts_8ulp"] - ref))[:, 1]
        d = np.abs(e["counts"][:, 1] - ref[:, 1])
        flips += int(d.sum())
        assert (d <= sens + 1).all(), (i, e["kind"], e["counts"][:, 1].tolist(), ref[:, 1].tolist())
        lref = float(g[f"p{i}/loss"])
        ltol = 2e-3 * max(1.0, abs(lref)) + 4 * max(abs(float(g[f"p{i}/loss_1ulp"]) - lref), abs(float(g[f"p{i}/loss_8ulp"]) - lref))
        assert abs(e["loss"] - lref) <= ltol, (i, e["kind"], e["loss"], lref)
    print(f"{opt.tl_method} replay: {flips} flipped predictions")
    (btr, bva, bte), (zs, zss) = final
    assert [e for e in log if e["kind"] == "final"][0]["best_epoch"] == int(g["final/best_epoch"])
    ref_test = dict(zip(keys, g["final/best_test"]))
    assert abs(bte["worst_acc"] - ref_test["worst_acc"]) <= 0.002 + 1e-9, (bte, ref_test)
    assert abs(bte["weighted_mean_acc"] - ref_test["weighted_mean_acc"]) <= 0.002 + 1e-9
    if opt.tl_method == "linear_probing":                 # the CLIP zero-shot baseline: raw embeddings against the prompts, no head
        for got, name in ((zs, "final/zs_class"), (zss, "final/zs_spurious")):
            ref = dict(zip(keys, g[name]))
            for k in keys:
                assert abs(got[k] - ref[k]) <= 1e-4, (name, k, got[k], ref[k])
    else:
        ref_zs = dict(zip(keys, g["final/zs_spurious"]))
        assert abs(zss["mean_acc"] - ref_zs["mean_acc"]) <= 0.002 + 1e-9
