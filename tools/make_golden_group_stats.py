"""Generate tests/golden/group_stats.npz from the REFERENCE's own representation-report code, demo/visualizer.py.

Same method as tools/make_golden_sweep.py: nothing of the reference is copied.  Its module cannot be imported here (UMAP, sklearn,
matplotlib, torchvision at the top), so the definitions the report's numbers come from -- get_top_k_indices, find_closest_sample,
compute_mean_vector, compute_vector_norm, compute_averaged_pairwise_distance, GetGroupWiseStatEbd, GetGroupWiseStatConf -- and the
table statements of VisHandler.VisRepAll (the index / column lists and the `for split in [...]` loop) are compiled from the file in
place (needs the reference tree, read-only) and run unmodified on the CPU over seeded synthetic splits of dbmm_amd.synth.  Only
numbers and names are saved: distances, norms, mean-vector samples, group labels, confidence means, nearest-row indices, the
zero-shot accuracy dicts fed to the table, and the tables' values, index and columns.  The inputs are regenerated from the seed on
both sides and never stored.

Conditions, asserted before anything is written (they are what the GPU test's bounds rest on):
  * every off-diagonal squared distance exceeds 1 % of the mean centred squared norm (so a 7e-7 error of the squared distance
    relative to the norms stays under 4e-5 of the distance);
  * the top-(k + 1) similarity scores of find_closest_sample are more than 1e-4 apart;
  * no table value lies within 1e-4 of a boundary of rounding to 3 places.

    python tools/make_golden_group_stats.py
"""
import ast
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as MG  # noqa: E402  (path setup, dbmm_amd shim)
from dbmm_amd import synth  # noqa: E402

# scale: the whole set is multiplied by it; with 30 table values and a 20 % forbidden band each, a seed alone almost never meets the
# rounding condition, so the seed was taken for the top-k condition and the scale then scanned (find_scale) for the rounding one
CFG = dict(seed=102, scale=1.235107421875, sizes=dict(train=1500, val=700, test=900), dim=1024, p_y=0.23, p_agree=0.95, top_k=5, temperature=0.01)
KEYS = ["weighted_mean_acc", "worst_acc", "acc_0_0", "acc_0_1", "acc_1_0", "acc_1_1", "mean_acc"]
VIS = os.path.join(MG.REF, "demo", "visualizer.py")
FUNCS = ("get_top_k_indices", "find_closest_sample", "compute_mean_vector", "compute_vector_norm", "compute_averaged_pairwise_distance",
         "GetGroupWiseStatEbd", "GetGroupWiseStatConf")
SAMPLE_STRIDE = 16                                                 # every 16th coordinate of a mean vector is recorded


def split_inputs(cfg, split):
    """(embeddings fp32 [n, dim], groups int64 [n], confidences fp32 [n]) of one split, from the seed alone"""
    x, y, c = synth.embedding_dataset(cfg["seed"], split, cfg["sizes"][split], cfg["dim"], p_y=cfg["p_y"], p_agree=cfg["p_agree"])
    conf = synth.uniform(cfg["seed"], split + "/conf", (cfg["sizes"][split],), 0.5, 1.0)
    return (x * cfg["scale"]).contiguous(), 2 * y + c, conf


def anchor(cfg):
    """the prompt embedding find_closest_sample is asked about: the second class prompt"""
    return synth.embedding_text(cfg["seed"], cfg["dim"])[0][:, 1].contiguous()


def zero_shot_acc(cfg, x, g, ratio):
    """the group-accuracy dict a zero-shot pass gives on these rows (the reference's get_results layout, rounded to 4 places): what
    VisRepAll reads as self.zs_results[split]"""
    t = synth.embedding_text(cfg["seed"], cfg["dim"])[0].double()
    xn = x.double() / x.double().norm(dim=1, keepdim=True)
    pred = (xn @ (t / t.norm(dim=0, keepdim=True))).argmax(1)
    ok = (pred == g // 2).double()
    acc = [ok[g == k].mean().item() for k in range(4)]
    n = [(g == k).sum().item() for k in range(4)]
    d = {"weighted_mean_acc": float((np.array(acc) * np.array(ratio)).sum()), "worst_acc": min(acc)}
    d.update({f"acc_{k // 2}_{k % 2}": acc[k] for k in range(4)})
    d["mean_acc"] = float(sum(a * m for a, m in zip(acc, n)) / sum(n))
    return {k: np.round(d[k], 4) for k in KEYS}


def reference_code():
    """(namespace with the reference's functions, the code object of VisRepAll's table statements), compiled from its file"""
    tree = ast.parse(open(VIS).read(), VIS)
    import pandas as pd
    from numpy.linalg import norm
    from scipy.spatial.distance import cdist
    ns = {"np": np, "pd": pd, "norm": norm, "cdist": cdist}
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(d.name for d in defs) == sorted(FUNCS), "the reference's statistics functions moved"
    exec(compile(ast.Module(body=defs, type_ignores=[]), VIS, "exec"), ns)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "VisHandler")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "VisRepAll")
    table = []
    for node in fn.body:
        names = {t.id for t in getattr(node, "targets", []) if isinstance(t, ast.Name)}
        if isinstance(node, ast.Assign) and names & {"group_wise_indexes", "columns", "dfs"}:
            table.append(node)
        if isinstance(node, ast.For) and isinstance(node.iter, ast.List) and [getattr(e, "value", None) for e in node.iter.elts] == ["train", "val", "test"]:
            table.append(node)
    assert len(table) == 4, "the reference's table statements moved"
    return ns, compile(ast.Module(body=table, type_ignores=[]), VIS, "exec")


def find_scale(cfg, margin=0.13):
    """a scale near 1 at which every Div. / Centr. Norm. value of the three tables is `margin` of a rounding step away from a
    boundary (they are linear in the scale up to fp32 rounding of the inputs; main() asserts the condition proper)"""
    ns, _ = reference_code()
    vals = []
    for split in cfg["sizes"]:
        x, g, _ = split_inputs(dict(cfg, scale=1.0), split)
        st = ns["GetGroupWiseStatEbd"](x.numpy(), g.numpy())
        vals += list(st["pairwise_distance"].values()) + list(st["mean_vector_norm"].values())
    vals = np.array(vals, dtype=np.float64)
    for s in np.arange(1.0, 2.0, 1.0 / 16384):
        v = vals * s * 1000
        if (np.abs(v - np.floor(v) - 0.5) > margin).all():
            return float(s)
    raise RuntimeError("no scale found")


def main():
    cfg = CFG
    if "--find-scale" in sys.argv:
        print("scale =", find_scale(cfg))
        return
    ns, table_code = reference_code()
    out = {"seed": np.array(cfg["seed"]), "dim": np.array(cfg["dim"]), "splits": np.array(list(cfg["sizes"])),
           "sizes": np.array(list(cfg["sizes"].values())), "p_y": np.array(cfg["p_y"]), "p_agree": np.array(cfg["p_agree"]),
           "top_k": np.array(cfg["top_k"]), "scale": np.array(cfg["scale"], dtype=np.float64), "sample_stride": np.array(SAMPLE_STRIDE), "acc_keys": np.array(KEYS)}
    a = anchor(cfg).numpy()
    this = SimpleNamespace(zs_results={}, group_wise_stat_ebd={})
    xtr, gtr, _ = split_inputs(cfg, "train")
    ratio = [(gtr == k).float().mean().item() for k in range(4)]
    for split in cfg["sizes"]:
        x, g, conf = split_inputs(cfg, split)
        xn, gn = x.numpy(), g.numpy()
        # the condition behind the 1e-4 bound of the GPU test
        xc = x.double() - x.double().mean(0)
        d2 = torch.cdist(xc, xc, compute_mode="donot_use_mm_for_euclid_dist") ** 2
        d2.fill_diagonal_(float("inf"))
        floor = d2.min().item() / (xc ** 2).sum(1).mean().item()
        assert floor > 0.01, f"{split}: smallest squared distance is {floor:.4f} of the mean centred squared norm"
        st = ns["GetGroupWiseStatEbd"](xn, gn)
        this.group_wise_stat_ebd[split] = st
        this.zs_results[split] = zero_shot_acc(cfg, x, g, ratio)
        keys = list(st["pairwise_distance"])
        assert keys[0] == "full" and [int(k) for k in keys[1:]] == sorted(set(gn.tolist()))
        out[f"{split}/groups"] = np.array([int(k) for k in keys[1:]])
        out[f"{split}/pairwise_distance"] = np.array([st["pairwise_distance"][k] for k in keys], dtype=np.float64)
        out[f"{split}/mean_vector_norm"] = np.array([st["mean_vector_norm"][k] for k in keys], dtype=np.float64)
        out[f"{split}/mean_vector_samples"] = np.stack([st["mean_vector"][k][::SAMPLE_STRIDE] for k in keys]).astype(np.float32)
        nd = ns["GetGroupWiseStatEbd"](xn, gn, return_dist=False)
        assert "pairwise_distance" not in nd or not nd["pairwise_distance"]
        cs = ns["GetGroupWiseStatConf"](conf.numpy(), gn)
        out[f"{split}/conf"] = np.array([cs[k] for k in cs], dtype=np.float64)
        idx = ns["find_closest_sample"](xn, a, top_k=cfg["top_k"])
        scores = np.sort((xn / np.linalg.norm(xn, axis=1, keepdims=True)).astype(np.float64) @ (a / np.linalg.norm(a)).astype(np.float64))[::-1]
        gaps = -np.diff(scores[:cfg["top_k"] + 1])
        assert gaps.min() > 1e-4, f"{split}: top-k similarity scores only {gaps.min():.2e} apart"
        out[f"{split}/closest"] = np.asarray(idx, dtype=np.int64)
        out[f"{split}/zs_acc"] = np.array([this.zs_results[split][k] for k in KEYS], dtype=np.float64)
    tns = dict(ns, self=this)
    exec(table_code, tns)
    for split, df in zip(cfg["sizes"], tns["dfs"]):
        raw = np.array([list(this.zs_results[split].values())[:-1],
                        [out[f"{split}/pairwise_distance"][0], 0, *out[f"{split}/pairwise_distance"][1:]],
                        [out[f"{split}/mean_vector_norm"][0], 0, *out[f"{split}/mean_vector_norm"][1:]]], dtype=np.float64)
        frac = np.abs(raw * 1000 - np.floor(raw * 1000) - 0.5)
        assert (frac[1:][raw[1:] != 0] > 0.1).all(), f"{split}: a table value lies within 1e-4 of a rounding boundary"
        out[f"{split}/table"] = df.to_numpy(dtype=np.float64)
        out[f"{split}/table_index"] = np.array(list(df.index))
        out[f"{split}/table_columns"] = np.array(list(df.columns))
    path = os.path.join(ROOT, "tests", "golden", "group_stats.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
