"""The lock-step sweep is scheduled like its runs alone, no GPU: trainer.train_sweep and the per-seed trainer.train_all_epochs runs go
through the one schedule of trainer.py with two executors of a pass; here both executors' device calls are replaced by torch
stand-ins (perfect predictions, zero loss) -- adapter.SweepAdapters / SweepLinear .step and .evaluate for the lock-step executor;
train_step / loss of the ordinary modules, adapter.group_counts, ops.gather_rows and trainer.validate_zs_linear_probing for the
single run -- and every host-side decision of a replica (initial weights, row orders, balanced subsets, prompt choice, learning
rate of every step, group sizes, record sequence, best epoch) must be the one of its own sequential run.  Tables and options are
those of the schedule fixtures under tests/golden/ (their `config` and `opt` entries; the recorded streams are not read here)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from dbmm_amd import adapter, ops, optim, synth, trainer


def _setup(fixture, tmp_path):
    g = np.load(os.path.join(GOLDEN, fixture), allow_pickle=False)
    cfg, o = json.loads(str(g["config"])), json.loads(str(g["opt"]))
    tcls, tspu, tgrp = synth.embedding_text(cfg["seed"], cfg["dim"])
    for key, m, cols in (("text_embedding_dir", tcls, ["c0", "c1"]), ("text_spurious_embedding_dir", tspu, ["s0", "s1"]),
                         ("text_group_embedding_dir", tgrp, ["g0", "g1", "g2", "g3"])):
        o[key] = os.path.join(tmp_path, key + ".json")
        json.dump({n: m[:, i].numpy().tolist() for i, n in enumerate(cols)}, open(o[key], "w"))
    tables = []
    for split, n in (("train", cfg["n_train"]), ("val", cfg["n_val"]), ("test", cfg["n_test"])):
        x, y, c = synth.embedding_dataset(cfg["seed"], split, n, cfg["dim"])
        tables.append(trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cpu"))
    return SimpleNamespace(**o), tables


def _stand_ins(monkeypatch, single_steps, sweep_steps):
    """single_steps: list of (lr, use_group, rows) per step of the running single run; sweep_steps[r]: the same per replica"""
    def fake_step(self, features, labels, optimizer, use_group=False):
        single_steps.append((optimizer.param_groups[0]["lr"], use_group, labels.shape[0]))
        return torch.zeros(()), torch.nn.functional.one_hot(labels, 4 if use_group else 2).float(), torch.zeros(labels.shape[0])

    def fake_loss(self, features, labels, use_group=False, spurious=False):
        return torch.zeros(()), torch.nn.functional.one_hot(labels, 2).float(), torch.zeros(labels.shape[0])

    def fake_counts(logits, y, g_, n_groups, counts=None):
        counts = torch.zeros((n_groups, 2), dtype=torch.int64) if counts is None else counts
        n = torch.bincount(g_, minlength=n_groups)
        counts[:, 0] += n; counts[:, 1] += n
        return counts

    def fake_zs(table, text_embedding_dir, temperature, batch_size, train_group_ratio, target="class", stats=None):
        trainer._epoch_batches(len(table), batch_size, False, None)          # one loader pass: the random stream advances once
        c = np.stack([np.bincount(table.group_array, minlength=4)] * 2, 1).astype(np.int64)
        if stats is not None:
            stats.update(counts=c)
        return 0.0, 1.0, {k: 1.0 for k in trainer.NEW_ORDER_FOR_PRINT}
    for cls in (adapter.CustomCLIP, adapter.LinearClassifier):
        monkeypatch.setattr(cls, "train_step", fake_step)
        monkeypatch.setattr(cls, "loss", fake_loss)
    monkeypatch.setattr(adapter, "group_counts", fake_counts)
    monkeypatch.setattr(ops, "gather_rows", lambda table, idx: table[idx])
    monkeypatch.setattr(trainer, "validate_zs_linear_probing", fake_zs)
    monkeypatch.setattr(trainer.ops, "get_option", lambda name: 1)

    def count_rows(counts, groups, rows):                                   # counts [R, G, 2] += the group sizes of rows [R, B]
        for r in range(rows.shape[0]):
            n = torch.bincount(groups[rows[r]], minlength=counts.shape[1])
            counts[r, :, 0] += n; counts[r, :, 1] += n

    def sweep_step(self, table, idx, labels, groups, which, lrs, momentum, weight_decay, counts, loss_sum, counted=True):
        assert idx.shape[0] == self.R == len(lrs) and which in ("class", "group")
        for r in range(self.R):
            sweep_steps[r].append((lrs[r], which == "group", idx.shape[1]))
        if counted:
            count_rows(counts, groups, idx)

    def sweep_evaluate(self, table, idx, labels, groups, which, counts, loss_sum, row0=0, n=None, best=False):
        rows = torch.arange(row0, row0 + n) if idx is None else idx
        count_rows(counts, groups, rows.expand(self.R, -1))
    monkeypatch.setattr(adapter.SweepAdapters, "step", sweep_step)
    monkeypatch.setattr(adapter.SweepAdapters, "evaluate", sweep_evaluate)
    monkeypatch.setattr(adapter.SweepLinear, "step", lambda self, table, idx, labels, groups, *a, **k: sweep_step(self, table, idx, labels, groups, "class", *a, **k))
    monkeypatch.setattr(adapter.SweepLinear, "evaluate",
                        lambda self, table, idx, labels, groups, *a, **k: sweep_evaluate(self, table, idx, labels, groups, "class", *a, **k))


CASES = {
    "linear_probing": ("schedule_linear_probing.npz", [3, 13, 23], None),
    "adapter_reg with balance_val": ("schedule_adapter_reg.npz", [11, 12, 13], None),
    "adapter_reg with use_cls_prompt_in_reg": ("schedule_adapter_reg_cls.npz", [5, 6], [0.1, 0.03]),
    "adapter_reg_seq_alter with add_adapter, balance_val, continue_from_best": ("two_stage.npz", [42, 32], [0.1, 0.05]),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_replica_of_a_sweep_is_scheduled_like_its_own_run(case, tmp_path, monkeypatch):
    fixture, seeds, learning_rates = CASES[case]
    opt, tables = _setup(fixture, tmp_path)
    opt.lr_multiple = 0.5
    replicas = trainer._sweep_replicas(opt, seeds, learning_rates)
    R = len(replicas)
    single_steps, sweep_steps = [], [[] for _ in range(R)]
    _stand_ins(monkeypatch, single_steps, sweep_steps)

    sweep_log = []
    sweep_out = trainer.train_sweep(opt, *tables, seeds, learning_rates=learning_rates, log=sweep_log)
    assert len(sweep_log) == len(sweep_out) == R
    assert all(sweep_steps) and not single_steps                             # the lock-step executor ran, the single-run one did not
    for r, (o, seed) in enumerate(replicas):
        del single_steps[:]
        optim.set_seed(seed)
        log = []
        out = trainer.train_all_epochs(o, *tables, log=log)
        mine = sweep_log[r]
        assert [e["kind"] for e in mine] == [e["kind"] for e in log], (r, "record kinds")
        n_init = 0
        for i, (a, b) in enumerate(zip(mine, log)):
            for key in ("epoch", "split", "target", "use_group", "n_train_rows", "best_epoch"):
                assert (key in a) == (key in b) and a.get(key) == b.get(key), (r, i, key)
            if a["kind"] == "init":
                n_init += 1
                assert sorted(a["state"]) == sorted(b["state"])
                assert all(torch.equal(a["state"][k], b["state"][k]) for k in b["state"]), (r, i)
            elif a["kind"] != "final":
                assert np.array_equal(a["counts"][:, 0], b["counts"][:, 0]), (r, i)
                assert ("order" in a) == ("order" in b) == (a["kind"] in ("train1", "train2", "train_reg"))
                if "order" in a:
                    assert a["order"].dtype == b["order"].dtype == np.int64 and np.array_equal(a["order"], b["order"]), (r, i)
        assert n_init == (2 if opt.tl_method != "linear_probing" and opt.add_adapter else 1)
        assert sweep_steps[r] == single_steps, (r, "learning rate, prompt choice and rows of every step")
        assert sweep_out[r] == out
    if learning_rates is not None:                                           # replicas of different learning rates did differ
        assert [s[0] for s in sweep_steps[0]] != [s[0] for s in sweep_steps[-1]]
