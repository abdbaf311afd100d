"""Generate tests/golden/schedule_{adapter_reg,adapter_reg_cls,linear_probing}.npz from the REFERENCE's own train_all_epochs.

Like `oracle/make_golden.py two_stage`: the reference's final_main.py is imported in place (needs the reference tree, read-only),
parse_option() + train_all_epochs() run unmodified on the CPU over a synthetic embedding set, and its loop functions are wrapped
(not replaced) to record what every pass saw and produced.  Only numbers are saved.

    python tools/make_golden_schedules.py [adapter_reg] [adapter_reg_cls] [linear_probing]      # default: all three
"""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as MG  # noqa: E402  (path setup, dbmm_amd shim)
from make_golden import _synthetic_embedding_module, _write_text_json, ref_final_main, summary  # noqa: E402
import adapter_oracle as AO  # noqa: E402
from dbmm_amd import synth  # noqa: E402

# adapter_reg with the balanced reg subset (per-epoch balance_val, global numpy RNG) and group prompts in the reg loop; --warm keeps
# every epoch in warm-up, whose batch index restarts with the reg loader
ADAPTER_REG = dict(seed=41, n_train=1024, n_val=1200, n_test=768, dim=1024,
                   argv=["--dataset", "celeba", "--tl_method", "adapter_reg", "--balance_val", "--warm", "--epochs", "4",
                         "--batch_size", "256", "--batch_size_reg", "16", "--learning_rate", "0.5", "--random_seed", "11"])
# adapter_reg on the shuffled, un-balanced reg half with the CLASS prompts (those batches count toward loss / accuracy), step decay
ADAPTER_REG_CLS = dict(seed=43, n_train=896, n_val=1000, n_test=768, dim=1024,
                       argv=["--dataset", "celeba", "--tl_method", "adapter_reg", "--use_cls_prompt_in_reg", "--epochs", "4",
                             "--batch_size", "128", "--batch_size_reg", "64", "--learning_rate", "0.1", "--lr_decay_epochs", "2,3",
                             "--lr_decay_rate", "0.5", "--random_seed", "5"])
# linear probing (the reference's default method): 1793 = 14 x 128 + 1 train rows leave a one-row last batch; step decay
LINEAR_PROBING = dict(seed=47, n_train=1793, n_val=1000, n_test=768, dim=1024,
                      argv=["--dataset", "celeba", "--tl_method", "linear_probing", "--epochs", "5", "--batch_size", "128",
                            "--learning_rate", "0.05", "--lr_decay_epochs", "3,4", "--lr_decay_rate", "0.5", "--random_seed", "3"])
CONFIGS = {"adapter_reg": ADAPTER_REG, "adapter_reg_cls": ADAPTER_REG_CLS, "linear_probing": LINEAR_PROBING}
KEYS = ["weighted_mean_acc", "worst_acc", "acc_0_0", "acc_0_1", "acc_1_0", "acc_1_1", "mean_acc"]


def run_reference(FM, cfg, paths, scale=1.0):
    """parse_option() + train_all_epochs() of the reference on the synthetic set, with train_one_epoch / train_reg_one_epoch /
    validate / validate_zs / update_dict / set_model / warmup_learning_rate / balance_val wrapped to record every pass"""
    log = []
    mod, plain = _synthetic_embedding_module(FM, cfg, scale, log)
    saved_mods = {k: sys.modules.get(k) for k in ("data.celeba_embeddings", "data.celeba_embeddings_reg")}
    sys.modules["data.celeba_embeddings"], sys.modules["data.celeba_embeddings_reg"] = plain, mod
    import data as _data_pkg  # noqa: F401                                       `from data.x import ...` resolves through sys.modules
    argv = sys.argv
    sys.argv = ["final_main.py"] + cfg["argv"] + ["--text_embedding_dir", paths[0], "--text_spurious_embedding_dir", paths[1],
                                                 "--text_group_embedding_dir", paths[2], "--image_embedding_dir", "/nonexistent/e.json",
                                                 "--data_dir", "/nonexistent"]
    rec = {"epochs": [], "inits": []}
    cur = {}
    names = ("train_one_epoch", "train_reg_one_epoch", "validate", "validate_zs", "update_dict", "set_model", "warmup_learning_rate",
             "balance_val")
    orig = {n: getattr(FM, n) for n in names}

    def phase(kind, fn):
        def wrapped(*a, **k):
            cur.clear(); cur.update(counts=np.zeros((4, 2), dtype=np.int64), start=len(log), lr=[], n_train=None)
            out = fn(*a, **k)
            loss, acc, gacc = out
            rows = log[cur["start"]:]
            rec["epochs"].append(dict(kind=kind, use_group=bool(k.get("group_prompt", False)), target=k.get("target"), loss=float(loss),
                                      acc=float(acc), counts=cur["counts"].copy(), group_acc={kk: float(v) for kk, v in gacc.items()},
                                      idx=[i for _, i in rows], n_train=sum(1 for s, _ in rows if s == "train"), lr=list(cur["lr"])))
            return out
        return wrapped

    def update_dict(acc_groups, y, g, logits):
        cur["counts"] += AO.group_counts(logits.detach(), y, g)
        return orig["update_dict"](acc_groups, y, g, logits)

    def warm(args, epoch, batch_id, total, optimizer):
        orig["warmup_learning_rate"](args, epoch, batch_id, total, optimizer)
        cur["lr"].append(float(optimizer.param_groups[0]["lr"]))

    def set_model(*a, **k):
        out = orig["set_model"](*a, **k)
        m = out[0]
        sd = m.state_dict() if isinstance(m, FM.LinearClassifier) else m.adapter.state_dict()     # fc.* / adapter layers
        rec["inits"].append({kk: v.detach().clone().numpy() for kk, v in sd.items()})
        return out

    def balance(loader, opt, print_procedure=False):
        out = orig["balance_val"](loader, opt, print_procedure)
        rec.setdefault("balanced", []).append((np.asarray(out.dataset.indices).copy(), int(out.batch_size)))
        return out
    FM.train_one_epoch = phase("train1", orig["train_one_epoch"])
    FM.train_reg_one_epoch = phase("train_reg", orig["train_reg_one_epoch"])
    FM.validate = phase("validate", orig["validate"])
    FM.validate_zs = phase("validate_zs", orig["validate_zs"])
    FM.update_dict, FM.warmup_learning_rate, FM.set_model, FM.balance_val = update_dict, warm, set_model, balance
    try:
        opt = FM.parse_option()                                                   # set_seed(opt.random_seed) runs in here
        rec["opt"] = {k: v for k, v in vars(opt).items() if isinstance(v, (int, float, str, bool, list))}
        # set_model only moves the classifier under `if torch.cuda.is_available()`; .cuda() is the identity here (ref_final_main)
        cuda_avail, torch.cuda.is_available = torch.cuda.is_available, (lambda: True)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                rec["final"] = FM.train_all_epochs(opt)
        finally:
            torch.cuda.is_available = cuda_avail
    finally:
        sys.argv = argv
        for n, f in orig.items():
            setattr(FM, n, f)
        for k, v in saved_mods.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return rec


def gen(FM, name):
    cfg = CONFIGS[name]
    tmp = tempfile.mkdtemp()
    tcls, tspu, tgrp = synth.embedding_text(cfg["seed"], cfg["dim"])
    paths = [os.path.join(tmp, n) for n in ("clip_class.json", "clip_spurious.json", "clip_group.json")]
    _write_text_json(paths[0], tcls, ["c0", "c1"]); _write_text_json(paths[1], tspu, ["s0", "s1"])
    _write_text_json(paths[2], tgrp, ["g0", "g1", "g2", "g3"])
    rec = run_reference(FM, cfg, paths)
    pert = run_reference(FM, cfg, paths, scale=1.0 + 2.0 ** -23)                  # the reference's own sensitivity: 1 ulp of its input
    pert8 = run_reference(FM, cfg, paths, scale=1.0 + 2.0 ** -20)                 # 8 ulp: the size of an fp32 kernel's rounding differences
    out = {"config": np.array(json.dumps(cfg)), "opt": np.array(json.dumps(rec["opt"])), "n_phases": np.int64(len(rec["epochs"])),
           "acc_keys": np.array(KEYS)}
    for i, (e, pe, pe8) in enumerate(zip(rec["epochs"], pert["epochs"], pert8["epochs"])):
        assert e["kind"] == pe["kind"] and e["idx"] == pe["idx"]
        out[f"p{i}/kind"] = np.array(e["kind"]); out[f"p{i}/use_group"] = np.bool_(e["use_group"])
        out[f"p{i}/target"] = np.array(str(e["target"])); out[f"p{i}/n_train"] = np.int64(e["n_train"])
        out[f"p{i}/loss"] = np.float64(e["loss"]); out[f"p{i}/acc"] = np.float64(e["acc"])
        out[f"p{i}/counts"] = e["counts"]; out[f"p{i}/counts_1ulp"] = pe["counts"]; out[f"p{i}/loss_1ulp"] = np.float64(pe["loss"])
        out[f"p{i}/counts_8ulp"] = pe8["counts"]; out[f"p{i}/loss_8ulp"] = np.float64(pe8["loss"])
        out[f"p{i}/group_acc"] = np.array([e["group_acc"].get(k, np.nan) for k in KEYS], dtype=np.float64)
        out[f"p{i}/idx"] = np.asarray(e["idx"], dtype=np.int64); out[f"p{i}/lr"] = np.asarray(e["lr"], dtype=np.float64)
    for i, (bi, bs) in enumerate(rec.get("balanced", [])):
        out[f"balanced{i}/indices"], out[f"balanced{i}/batch_size"] = bi.astype(np.int64), np.int64(bs)
    for i, sd in enumerate(rec["inits"]):
        for k, v in sd.items():
            out[f"init{i}/{k}_sums"], out[f"init{i}/{k}_sample"] = summary(torch.from_numpy(np.asarray(v)))
    (btr, bva, bte), (zs, zss) = rec["final"]
    out["final/best_test"] = np.array([bte[k] for k in KEYS]); out["final/best_val"] = np.array([bva[k] for k in KEYS])
    out["final/zs_class"] = np.array([zs[k] for k in KEYS]); out["final/zs_spurious"] = np.array([zss[k] for k in KEYS])
    vals = [e for e in rec["epochs"] if e["kind"] == "validate"][0::2]                # per epoch: val, then test
    best, best_acc = 0, 0.0
    for j, wv in enumerate(v["group_acc"]["worst_acc"] for v in vals):             # train_all_epochs' strict ">" selection
        if wv > best_acc:
            best, best_acc = j + 1, wv
    out["final/best_epoch"] = np.int64(best)
    print(f"[{name}] phases:", " ".join(e["kind"] for e in rec["epochs"]))
    for i, e in enumerate(rec["epochs"]):
        d = (np.abs(e["counts"] - pert["epochs"][i]["counts"]).max(), np.abs(e["counts"] - pert8["epochs"][i]["counts"]).max())
        print(f"[{name}] p{i:02d} {e['kind']:11s} n={e['counts'][:, 0].sum():5d} loss {e['loss']:.4f} acc {e['acc']:.4f} worst "
              f"{e['group_acc'].get('worst_acc', float('nan')):.4f}  group correct {e['counts'][:, 1].tolist()}  |1 / 8 ulp count diff| {d}")
    print(f"[{name}] best epoch {best}")
    path = os.path.join(MG.GOLD, f"schedule_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"[{name}] wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    which = [a for a in sys.argv[1:] if a in CONFIGS] or list(CONFIGS)
    FM = ref_final_main()
    for name in which:
        gen(FM, name)
