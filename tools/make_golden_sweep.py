"""Generate tests/golden/sweep_wb.npz from the REFERENCE's own sweep driver, run_multiple/final_main_iteration_wb.py.

Same method as tools/make_golden_schedules.py: the driver is imported in place (needs the reference tree, read-only) and its own
`if __name__ == '__main__':` block -- the seed loop around train_all_epochs and the pandas table code -- is compiled from the file and
executed unmodified in the module's namespace, on the CPU, over a synthetic embedding set.  Its loop functions are wrapped (not
replaced) to record what every pass of every seed saw and produced.  Only numbers and names are saved: per seed and pass the batch
index stream, learning rates, loss, accuracy and (n, correct) counters, the same for the runs on inputs scaled by 1 + 2^-23 and
1 + 2^-20 (the reference's own sensitivity), samples of the initial weights, the five dicts train_all_epochs returned, and the
final table (values, row labels, columns) with its file name.

Condition, asserted before anything is written: for every seed the perturbed runs select the same best epoch as the unperturbed
one -- otherwise a best-epoch comparison against this fixture would test the dice.

    python tools/make_golden_sweep.py
"""
import ast
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
from make_golden import _load_by_path, _synthetic_embedding_module, _write_text_json, summary  # noqa: E402
import adapter_oracle as AO  # noqa: E402
from dbmm_amd import synth  # noqa: E402

# three seeds of adapter_reg_seq_alter with every option of the two-stage schedule: MultipleAdapter, the per-epoch balanced reg subset,
# restart from the best stage-1 model; 6 epochs with the switch in the middle.  dim = 1024 is the driver's own model_dict width.
SWEEP_WB = dict(seed=61, n_train=1024, n_val=1200, n_test=768, dim=1024,
                argv=["--dataset", "celeba", "--tl_method", "adapter_reg_seq_alter", "--add_adapter", "--balance_val", "--continue_from_best",
                      "--epochs", "6", "--epochs_feature_learning", "3", "--batch_size", "256", "--batch_size_reg", "16",
                      "--learning_rate", "0.1", "--learning_rate_reg", "0.05", "--lr_decay_epochs", "5", "--lr_decay_rate", "0.5",
                      "--num_iter", "3", "--random_seeds", "42,32,22"])
KEYS = ["weighted_mean_acc", "worst_acc", "acc_0_0", "acc_0_1", "acc_1_0", "acc_1_1", "mean_acc"]
DRIVER = os.path.join(MG.REF, "run_multiple", "final_main_iteration_wb.py")


def load_driver(cfg):
    """the driver module, loaded under another name so that its __main__ block does not run yet; the data modules it imports at the
    top (which read CSV / JSON files that are not here) are the synthetic stand-ins from the start"""
    MG.ref_final_main()                                                           # stubs for the imports the CPU run does not need
    mod, plain = _synthetic_embedding_module(None, cfg)
    for k, v in (("data.celeba_embeddings", plain), ("data.celeba_embeddings_reg", mod), ("data.waterbirds_embeddings", plain)):
        sys.modules[k] = v
    plain.WaterbirdsEmbeddings, plain.load_waterbirds_embeddings = plain.CelebaEmbeddings, plain.load_celeba_embeddings
    with contextlib.redirect_stdout(io.StringIO()):
        return _load_by_path("ref_iteration_wb", DRIVER)


def main_block():
    """the body of the driver's `if __name__ == '__main__':`, compiled from its file"""
    tree = ast.parse(open(DRIVER).read(), DRIVER)
    for node in tree.body:
        if isinstance(node, ast.If) and isinstance(node.test, ast.Compare) and getattr(node.test.left, "id", "") == "__name__":
            return compile(ast.Module(body=node.body, type_ignores=[]), DRIVER, "exec")
    raise RuntimeError("no __main__ block in " + DRIVER)


def run_driver(FM, cfg, paths, scale=1.0):
    """the driver's own seed loop and table code, with set_seed / train_all_epochs / the loop functions wrapped to record every pass"""
    log = []
    mod, plain = _synthetic_embedding_module(FM, cfg, scale, log)
    saved_mods = {k: sys.modules.get(k) for k in ("data.celeba_embeddings", "data.celeba_embeddings_reg")}
    sys.modules["data.celeba_embeddings"], sys.modules["data.celeba_embeddings_reg"] = plain, mod
    argv, cwd = sys.argv, os.getcwd()
    sys.argv = ["final_main_iteration_wb.py"] + cfg["argv"] + ["--text_embedding_dir", paths[0], "--text_spurious_embedding_dir", paths[1],
                                                               "--text_group_embedding_dir", paths[2], "--image_embedding_dir",
                                                               "/nonexistent/e.json", "--data_dir", "/nonexistent"]
    runs = []                                                                     # one record per seed
    cur = {}
    names = ("train_one_epoch", "train_reg_seq_one_epoch", "train_reg_one_epoch", "validate", "validate_zs", "update_dict", "set_model", "set_model_multiple_adapter",
             "warmup_learning_rate", "warmup_learning_rate_reg", "balance_val", "set_seed", "train_all_epochs")
    orig = {n: getattr(FM, n) for n in names}

    def phase(kind, fn):
        def wrapped(*a, **k):
            cur.clear(); cur.update(counts=np.zeros((4, 2), dtype=np.int64), start=len(log), lr=[])
            out = fn(*a, **k)
            loss, acc, gacc = out
            optimizer = a[5] if kind == "train_reg" else a[4] if kind in ("train1", "train2") else None
            rows = log[cur["start"]:]
            runs[-1]["epochs"].append(dict(kind=kind, use_group=bool(k.get("use_group", k.get("group_prompt", False))), target=k.get("target"),
                                           n_train=sum(1 for s, _ in rows if s == "train"), loss=float(loss),
                                           acc=float(acc), counts=cur["counts"].copy(), group_acc={kk: float(v) for kk, v in gacc.items()},
                                           idx=[i for _, i in rows], lr=list(cur["lr"]),
                                           lr_end=float(optimizer.param_groups[0]["lr"]) if optimizer is not None else float("nan")))
            return out
        return wrapped

    def update_dict(acc_groups, y, g, logits):
        cur["counts"] += AO.group_counts(logits.detach(), y, g)
        return orig["update_dict"](acc_groups, y, g, logits)

    def warm(fn):
        def wrapped(args, epoch, batch_id, total, optimizer):
            fn(args, epoch, batch_id, total, optimizer)
            cur["lr"].append(float(optimizer.param_groups[0]["lr"]))
        return wrapped

    def model_maker(fn, which):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            m = out[0]                                                            # fc.* of a LinearClassifier / the adapter's layers
            ad = m.new_adapter if which == "stage2" else m if isinstance(m, FM.LinearClassifier) else m.adapter
            runs[-1]["inits"].append({kk: v.detach().clone().numpy() for kk, v in ad.state_dict().items()})
            return out
        return wrapped

    def balance(loader, opt, print_procedure=False):
        out = orig["balance_val"](loader, opt, print_procedure)
        runs[-1]["balanced"].append((np.asarray(out.dataset.indices).copy(), int(out.batch_size)))
        return out

    def set_seed(seed):
        if shared.get("parsed"):                                                     # parse_option seeds once itself, before the loop
            runs.append(dict(seed=int(seed), epochs=[], inits=[], balanced=[]))
        return orig["set_seed"](seed)

    def train_all_epochs(opt):
        out = orig["train_all_epochs"](opt)
        runs[-1]["final"] = out
        return out

    def parse_option():
        opt = orig_parse()
        shared["parsed"] = True
        shared["opt"] = {k: v for k, v in vars(opt).items() if isinstance(v, (int, float, str, bool, list))}
        return opt
    shared = {}
    orig_parse = FM.parse_option
    FM.parse_option = parse_option
    FM.train_one_epoch = phase("train1", orig["train_one_epoch"])
    FM.train_reg_seq_one_epoch = phase("train2", orig["train_reg_seq_one_epoch"])
    FM.train_reg_one_epoch = phase("train_reg", orig["train_reg_one_epoch"])
    FM.validate = phase("validate", orig["validate"])
    FM.validate_zs = phase("validate_zs", orig["validate_zs"])
    FM.update_dict, FM.balance_val, FM.set_seed, FM.train_all_epochs = update_dict, balance, set_seed, train_all_epochs
    FM.warmup_learning_rate, FM.warmup_learning_rate_reg = warm(orig["warmup_learning_rate"]), warm(orig["warmup_learning_rate_reg"])
    FM.set_model, FM.set_model_multiple_adapter = model_maker(orig["set_model"], "stage1"), model_maker(orig["set_model_multiple_adapter"], "stage2")
    tmp = tempfile.mkdtemp()
    cuda_avail, torch.cuda.is_available = torch.cuda.is_available, (lambda: True)      # .cuda() is the identity here (ref_final_main)
    try:
        os.chdir(tmp)                                                             # the driver writes results_iterative/<name>.csv
        with contextlib.redirect_stdout(io.StringIO()):
            exec(main_block(), FM.__dict__)
        frame, name = FM.__dict__["final_df"], FM.__dict__["final_result_file_path"]
        assert os.path.exists(os.path.join(tmp, "results_iterative", name + ".csv"))
    finally:
        os.chdir(cwd)
        torch.cuda.is_available = cuda_avail
        sys.argv = argv
        FM.parse_option = orig_parse
        for n, f in orig.items():
            setattr(FM, n, f)
        for k, v in saved_mods.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return dict(runs=runs, opt=shared["opt"], frame=frame, name=name)


def best_epoch(run):
    """train_all_epochs' strict ">" selection on the val worst-group accuracy (per epoch: a val pass, then a test pass)"""
    vals = [e for e in run["epochs"] if e["kind"] == "validate"][0::2]
    best, best_acc = 0, 0.0
    for j, wv in enumerate(v["group_acc"]["worst_acc"] for v in vals):
        if wv > best_acc:
            best, best_acc = j + 1, wv
    return best


def gen(cfg=SWEEP_WB, fname="sweep_wb.npz"):
    FM = load_driver(cfg)
    tmp = tempfile.mkdtemp()
    tcls, tspu, tgrp = synth.embedding_text(cfg["seed"], cfg["dim"])
    paths = [os.path.join(tmp, n) for n in ("clip_class.json", "clip_spurious.json", "clip_group.json")]
    _write_text_json(paths[0], tcls, ["c0", "c1"]); _write_text_json(paths[1], tspu, ["s0", "s1"])
    _write_text_json(paths[2], tgrp, ["g0", "g1", "g2", "g3"])
    rec = run_driver(FM, cfg, paths)
    pert = run_driver(FM, cfg, paths, scale=1.0 + 2.0 ** -23)                     # the reference's own sensitivity: 1 ulp of its input
    pert8 = run_driver(FM, cfg, paths, scale=1.0 + 2.0 ** -20)                    # 8 ulp: the size of an fp32 kernel's rounding differences
    out = {"config": np.array(json.dumps(cfg)), "opt": np.array(json.dumps(rec["opt"])), "n_seeds": np.int64(len(rec["runs"])),
           "acc_keys": np.array(KEYS), "seeds": np.array([r["seed"] for r in rec["runs"]], dtype=np.int64)}
    for s, (run, p1, p8) in enumerate(zip(rec["runs"], pert["runs"], pert8["runs"])):
        be = best_epoch(run), best_epoch(p1), best_epoch(p8)
        print(f"[seed {run['seed']}] best epoch {be[0]} (1 ulp: {be[1]}, 8 ulp: {be[2]})  phases: " + " ".join(e["kind"] for e in run["epochs"]))
        assert be[0] == be[1] == be[2] and be[0] > 0, f"seed {run['seed']}: the perturbed runs select another best epoch {be}; pick other sizes / seeds"
        out[f"s{s}/best_epoch"], out[f"s{s}/n_phases"] = np.int64(be[0]), np.int64(len(run["epochs"]))
        for i, (e, pe, pe8) in enumerate(zip(run["epochs"], p1["epochs"], p8["epochs"])):
            assert e["kind"] == pe["kind"] == pe8["kind"] and e["idx"] == pe["idx"] == pe8["idx"]
            k = f"s{s}/p{i}/"
            out[k + "kind"] = np.array(e["kind"]); out[k + "use_group"] = np.bool_(e["use_group"]); out[k + "target"] = np.array(str(e["target"]))
            out[k + "loss"] = np.float64(e["loss"]); out[k + "acc"] = np.float64(e["acc"]); out[k + "counts"] = e["counts"]
            out[k + "counts_1ulp"], out[k + "loss_1ulp"] = pe["counts"], np.float64(pe["loss"])
            out[k + "counts_8ulp"], out[k + "loss_8ulp"] = pe8["counts"], np.float64(pe8["loss"])
            out[k + "group_acc"] = np.array([e["group_acc"].get(kk, np.nan) for kk in KEYS], dtype=np.float64)
            out[k + "lr"], out[k + "lr_end"] = np.asarray(e["lr"], dtype=np.float64), np.float64(e["lr_end"])
            if e["kind"] in ("train1", "train2", "train_reg"):                    # evaluation passes read their split in order
                out[k + "idx"] = np.asarray(e["idx"], dtype=np.int32)
            if e["kind"] == "train_reg":                                          # the train loader's rows come first, then the reg loop's
                out[k + "n_train"] = np.int64(e["n_train"])
            d = (np.abs(e["counts"] - pe["counts"]).max(), np.abs(e["counts"] - pe8["counts"]).max())
            print(f"[seed {run['seed']}] p{i:02d} {e['kind']:11s} n={e['counts'][:, 0].sum():5d} loss {e['loss']:.4f} worst "
                  f"{e['group_acc'].get('worst_acc', float('nan')):.4f} correct {e['counts'][:, 1].tolist()} |1 / 8 ulp count diff| {d}")
        for i, (bi, bs) in enumerate(run["balanced"]):
            out[f"s{s}/balanced{i}/indices"], out[f"s{s}/balanced{i}/batch_size"] = bi.astype(np.int32), np.int64(bs)
        for i, sd in enumerate(run["inits"]):
            for kk, v in sd.items():
                out[f"s{s}/init{i}/{kk}_sums"], out[f"s{s}/init{i}/{kk}_sample"] = summary(torch.from_numpy(np.asarray(v)))
        (btr, bva, bte), (zs, zss) = run["final"]
        for tag, d in (("tr", btr), ("val", bva), ("test", bte), ("zs_tg", zs), ("zs_spu", zss)):
            out[f"s{s}/final/{tag}_keys"] = np.array(list(d))
            out[f"s{s}/final/{tag}"] = np.array([float(v) for v in d.values()], dtype=np.float64)
    frame = rec["frame"]
    out["table/values"] = frame.to_numpy(dtype=np.float64)
    out["table/index"] = np.array([str(i) for i in frame.index])
    out["table/columns"] = np.array([str(c) for c in frame.columns])
    out["table/name"] = np.array(rec["name"])
    print(frame)
    print("file name:", rec["name"])
    path = os.path.join(MG.GOLD, fname)
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    gen()
