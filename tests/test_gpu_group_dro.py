"""Group-DRO training on the MI355X: the group-reduction / q-update kernel, the one-call robust step, the autograd path, the
replica-batched step and the schedule, against a float64 torch-CPU restatement written here (adapter forward in train mode, cosine
logits over T, the robust loss of tests/test_group_dro_host.py's gdro_update, autograd, SGD with momentum)."""
import copy
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dbmm_amd import adapter, ops, optim, synth, trainer
from test_group_dro_host import gdro_update

pytestmark = pytest.mark.gpu
T, LR, MU, WD, ETA = 0.01, 0.1, 0.9, 5e-5, 0.01
KEYS = ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias", "layers.3.weight", "layers.3.bias")


def _text_paths(tmp_path_factory, D, seed=1):
    d = tmp_path_factory.mktemp(f"text{D}")
    paths = []
    for name, C, tag in (("clip_class", 2, "class"), ("clip_spurious", 2, "spurious"), ("clip_group", 4, "group")):
        m = synth.text_matrix(seed, D, C, tag)
        p = os.path.join(d, name + ".json")
        json.dump({f"{tag}{i}": m[:, i].numpy().tolist() for i in range(C)}, open(p, "w"))
        paths.append(p)
    return paths


@pytest.fixture(scope="module")
def text_paths_by_dim(tmp_path_factory):
    cache = {}

    def get(D):
        if D not in cache:
            cache[D] = _text_paths(tmp_path_factory, D)
        return cache[D]
    return get


def _ns():
    return SimpleNamespace(learning_rate=LR, learning_rate_reg=LR, momentum=MU, weight_decay=WD)


def _batch(B, D, G=4):
    """rows, class labels and group ids with a one-row group (the last one) when G > 1"""
    x = synth.normal(5, f"gdro_x{B}_{D}", (B, D), 0.5)
    y = synth.labels(6, B)[0]
    g = torch.arange(B) % max(G - 1, 1)
    if G > 1:
        g[5] = G - 1
    return x, y, g


def _make(D, H, paths, multiple):
    ad = adapter.Adapter(D, H); ad.load_state_dict(synth.adapter_state_dict(3, D, H))
    clf = adapter.CustomCLIP(ad, *paths, temperature=T)
    if multiple:
        new = adapter.Adapter(D, H); new.load_state_dict(synth.adapter_state_dict(4, D, H))
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            clf = adapter.MultipleAdapter(clf, new, init_near_identity=False)
        return clf.cuda().train(), optim.set_optimizer_reg(_ns(), clf)
    return clf.cuda().train(), optim.set_optimizer(_ns(), clf)


def _trainable(m):
    return m.new_adapter if isinstance(m, adapter.MultipleAdapter) else m.adapter


def _momenta(m, opt):
    return [opt.state[p]["momentum_buffer"] for p in _trainable(m).parameters()]


# ---- the float64 oracle ---------------------------------------------------------------------------------------------------------
def _oracle_adapter(sd, x, eps=1e-5):
    """train-mode Linear -> BatchNorm1d -> ReLU -> Linear; returns (z, batch mean, unbiased batch variance)"""
    h = x @ sd["layers.0.weight"].t() + sd["layers.0.bias"]
    mean, var = h.mean(0), h.var(0, unbiased=False)
    hn = (h - mean) / torch.sqrt(var + eps) * sd["layers.1.weight"] + sd["layers.1.bias"]
    return torch.relu(hn) @ sd["layers.3.weight"].t() + sd["layers.3.bias"], mean.detach(), h.var(0, unbiased=True).detach()


def _oracle_run(D, H, x, y, g, text, multiple, robust, G, steps=3):
    """`steps` SGD-momentum steps in float64 from the states _make() loads: -> ({key: update of the trainable tensor}, q)"""
    x, text = x.double(), text.double()
    new = {k: v.double() for k, v in synth.adapter_state_dict(4 if multiple else 3, D, H).items()}
    old = {k: v.double() for k, v in synth.adapter_state_dict(3, D, H).items()} if multiple else None
    start = {k: new[k].clone() for k in KEYS}
    bufs = {}
    q = np.full((G,), 1.0 / G)
    tn = text / text.norm(dim=0, keepdim=True)
    for _ in range(steps):
        ps = {k: new[k].clone().requires_grad_() for k in KEYS}
        z, _, _ = _oracle_adapter(ps, x)
        f = z / z.norm(dim=1, keepdim=True)
        if multiple:
            with torch.no_grad():
                zo, _, _ = _oracle_adapter(old, x)
            f = 0.5 * zo / zo.norm(dim=1, keepdim=True) + 0.5 * f
        rows = torch.nn.functional.cross_entropy(f @ tn / T, y, reduction="none")
        if robust:
            _, _, q, w, _ = gdro_update(rows.detach().numpy(), g.numpy(), q, ETA, G)
            inside = (g >= 0) & (g < G)
            wrow = torch.where(inside, torch.from_numpy(w)[g.clamp(0, G - 1)], torch.zeros((), dtype=torch.float64))
            loss = (wrow * rows).sum()
        else:
            loss = rows.mean()
        loss.backward()
        for k in KEYS:
            gr = ps[k].grad + WD * new[k]
            bufs[k] = gr if k not in bufs else MU * bufs[k] + gr
            new[k] = new[k] - LR * bufs[k]
    return {k: new[k] - start[k] for k in KEYS}, q


def _gpu_run(D, H, x, y, g, paths, multiple, robust, G, steps=3):
    clf, opt = _make(D, H, paths, multiple)
    ad = _trainable(clf)
    start = {k: v.detach().clone() for k, v in ad.state_dict().items() if k in KEYS}
    state = adapter.GroupDRO(G, ETA, "cuda") if robust else None
    xd, yd, gd = x.cuda(), y.cuda(), g.cuda()
    for _ in range(steps):
        clf.train_step(xd, yd, opt, robust=(state, gd) if robust else None)
    sd = ad.state_dict()
    return {k: (sd[k].double() - start[k].double()).cpu() for k in KEYS}, None if state is None else state.q.double().cpu().numpy()


# ---- 1. the weights kernel alone -------------------------------------------------------------------------------------------------
def _weights_case():
    B, G = 37, 4
    loss = synth.uniform(7, "gdro_loss", (B,), 0.0, 200.0)          # T = 0.01: a row's CE reaches hundreds
    g = torch.arange(B) % 2                                          # groups 0 and 1 ...
    g[3] = 3                                                         # ... a single row in group 3, none in group 2 ...
    g[11] = 9                                                        # ... and a group id out of range
    return loss, g, B, G


def test_weights_kernel_against_float64():
    """q within rtol 1e-5: with eta L <= 2 the fp32 rounding of L and of exp is a few 1e-7; that with a 10x margin.  L_g, the row
    weights and the robust loss are fp32 roundings of float64 results (the kernel sums and divides in float64): 1e-6 relative."""
    loss, g, B, G = _weights_case()
    q0 = torch.tensor([0.1, 0.2, 0.3, 0.4])
    n, L, q, w, rl = gdro_update(loss.double().numpy(), g.numpy(), q0.double().numpy(), ETA, G)
    assert n.tolist() == [19, 16, 0, 1] and ETA * L.max() <= 2.0
    qd = q0.cuda()
    robust, stats = ops.group_dro_weights(loss.cuda(), g.cuda(), qd, ETA)
    stats, got_q = stats.double().cpu().numpy(), qd.double().cpu().numpy()
    print("q", got_q, "rel err", np.abs(got_q - q).max() / q.max(), "L err", np.abs(stats[1] - L).max() / L.max())
    assert stats[2].tolist() == n.tolist()
    assert np.abs(stats[1] - L).max() <= 1e-6 * L.max()
    assert (np.abs(got_q - q) <= 1e-5 * q).all()
    assert (np.abs(stats[0] - w) <= 1e-5 * w).all() and stats[0][2] == 0.0
    assert abs(robust.item() - rl) <= 1e-5 * rl
    # q_out given: q_in is left alone
    q_in, q_out = q0.cuda(), torch.zeros(G, device="cuda")
    ops.group_dro_weights(loss.cuda(), g.cuda(), q_in, ETA, q_out=q_out)
    assert torch.equal(q_in.cpu(), q0) and torch.equal(q_out, qd)


def test_weights_kernel_huge_step_size_and_determinism():
    loss, g, B, G = _weights_case()
    ld, gd = loss.cuda(), g.cuda()
    L = gdro_update(loss.double().numpy(), g.numpy(), np.full(G, 0.25), 50.0, G)[1]
    q = torch.full((G,), 0.25, device="cuda")
    ops.group_dro_weights(ld, gd, q, 50.0)
    qc = q.double().cpu().numpy()
    assert np.isfinite(qc).all() and abs(qc.sum() - 1.0) <= 1e-6 and qc.argmax() == int(np.argmax(L)) and qc.max() > 0.999
    outs = []
    for _ in range(2):
        q = torch.tensor([0.1, 0.2, 0.3, 0.4], device="cuda")
        robust, stats = ops.group_dro_weights(ld, gd, q, ETA)
        outs.append((q.clone(), robust.clone(), stats.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_wrappers_check_their_operands():
    loss, g, B, G = _weights_case()
    ld, gd = loss.cuda(), g.cuda()
    with pytest.raises(RuntimeError):
        ops.group_dro_weights(ld, gd[:-1].contiguous(), torch.full((G,), 0.25, device="cuda"), ETA)
    with pytest.raises(RuntimeError):
        ops.group_dro_weights(ld, gd, torch.full((9,), 1 / 9, device="cuda"), ETA)
    with pytest.raises(RuntimeError):
        ops.group_dro_weights(ld, gd.int(), torch.full((G,), 0.25, device="cuda"), ETA)
    with pytest.raises(RuntimeError):
        ops.group_dro_weights(loss, g, torch.full((G,), 0.25), ETA)                  # CPU tensors
    with pytest.raises(ValueError):
        adapter.GroupDRO(9)
    assert ops.adapter_step_launches(256, 1024, 128) == 8 and ops.adapter_step_launches(256, 1024, 128, robust=True) == 10
    assert ops.adapter_step_launches(256, 1024, 128, with_old=True, robust=True) == 13
    assert ops.adapter_step_launches(10, 64, 16, robust=True) is None


def test_state_object_copies_and_pickles():
    import pickle
    s = adapter.GroupDRO(4, 0.05, "cuda")
    s.q.copy_(torch.tensor([0.1, 0.2, 0.3, 0.4]))
    for c in (copy.deepcopy(s), pickle.loads(pickle.dumps(s))):
        assert torch.equal(c.q, s.q) and c.q.data_ptr() != s.q.data_ptr() and (c.n_groups, c.step_size) == (4, 0.05)
    s.reset()
    assert torch.equal(s.q.cpu(), torch.full((4,), 0.25))
    assert adapter.GroupDRO(4, replicas=3, device="cuda").q.shape == (3, 4)


# ---- 2. the one-call step against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,H,multiple", [(37, 128, 128, False), (10, 64, 16, False), (37, 128, 128, True)],
                         ids=["fast", "generic", "old_adapter"])
def test_one_call_step_against_float64_oracle(B, D, H, multiple, text_paths_by_dim):
    """Three consecutive robust steps (q and the momentum carry over): per trainable tensor, err = max|update - update_ref| /
    max|update_ref| of the three steps' total update.  Tolerance: 4 x the same quantity of the ERM train_step against its float64
    restatement on the same inputs, measured here (a one-row group's weight is up to B times ERM's 1 / B, so the cancellation in the
    batch reductions differs).  layers.0.bias is left out of the relative comparison: its gradient is analytically zero (a bias in
    front of train-mode BatchNorm), so its update is weight decay plus rounding noise of the column sums of dh; tests/
    test_gpu_adapter.py bounds that gradient by 1e-5 absolute under ERM, and the same 4 x margin on it through three momentum steps
    (factors 1, 1.9, 2.71 of lr) bounds the update here.  q against the oracle's, per step: the kernel's own rtol 1e-5, plus eta
    times the error of a group's mean CE, which the project's bound on a cosine logit at T = 0.01 (1e-3 absolute) puts below 2e-3;
    three steps.
    Measured on an MI355X, worst tensor by robust / ERM ratio (ERM err -> robust err; the ratio must stay <= 4): fast
    layers.0.weight 3.2e-07 -> 9.3e-07 (2.9 x), generic layers.3.bias 8.4e-08 -> 2.7e-07 (3.2 x), old adapter layers.3.weight
    2.9e-07 -> 8.2e-07 (2.9 x); every robust err <= 2.2e-06.  layers.0.bias: |update - ref| <= 3e-09 absolute (3e-02 ... 9e-02
    of its own tiny update, under ERM as well).  q: 1.1e-07 ... 2.4e-07 relative."""
    G = 4
    x, y, g = _batch(B, D, G)
    paths = text_paths_by_dim(D)
    text = synth.text_matrix(1, D, 2, "class")
    erm_ref, _ = _oracle_run(D, H, x, y, g, text, multiple, False, G)
    erm, _ = _gpu_run(D, H, x, y, g, paths, multiple, False, G)
    rob_ref, q_ref = _oracle_run(D, H, x, y, g, text, multiple, True, G)
    rob, q = _gpu_run(D, H, x, y, g, paths, multiple, True, G)
    err = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    for k in KEYS:
        e_erm, e_rob = err(erm[k], erm_ref[k]), err(rob[k], rob_ref[k])
        print(f"B={B} D={D} H={H} old={multiple} {k}: ERM err {e_erm:.3e}, robust err {e_rob:.3e}, allowed {4 * e_erm:.3e}")
    print("q", q, "oracle", q_ref, "rel err", np.abs(q - q_ref).max() / q_ref.max())
    for k in KEYS:
        if k == "layers.0.bias":
            assert (rob[k] - rob_ref[k]).abs().max().item() <= 4 * 1e-5 * LR * (1 + 1.9 + 2.71), k
        else:
            assert err(rob[k], rob_ref[k]) <= 4 * err(erm[k], erm_ref[k]), k
    assert (np.abs(q - q_ref) <= 3 * (1e-5 + ETA * 2e-3) * q_ref).all() and abs(q.sum() - 1.0) <= 1e-6
    assert not np.allclose(q, 0.25)                                              # q did move


# ---- 3. the one-call step and the autograd path give the same bits --------------------------------------------------------------
@pytest.mark.parametrize("B,D,H,multiple", [(37, 128, 128, False), (37, 128, 128, True), (10, 64, 16, False)])
def test_one_call_step_equals_autograd_path(B, D, H, multiple, text_paths_by_dim):
    G = 4
    x, y, g = (t.cuda() for t in _batch(B, D, G))
    a, oa = _make(D, H, text_paths_by_dim(D), multiple)
    b, ob = _make(D, H, text_paths_by_dim(D), multiple)
    sa, sb = adapter.GroupDRO(G, ETA, "cuda"), adapter.GroupDRO(G, ETA, "cuda")
    for step in range(3):
        la, logits_a, rows_a = a.loss(x, y, robust=(sa, g))
        oa.zero_grad(); la.backward(); oa.step()
        lb, logits_b, rows_b = b.train_step(x, y, ob, robust=(sb, g))
        assert torch.equal(logits_a, logits_b) and torch.equal(rows_a, rows_b) and torch.equal(la.detach(), lb), step
        assert torch.equal(sa.q, sb.q), step
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):      # parameters and running statistics
        assert torch.equal(va, vb), k
    for ma, mb in zip(_momenta(a, oa), _momenta(b, ob)):
        assert torch.equal(ma, mb)
    assert not torch.equal(sa.q.cpu(), torch.full((G,), 0.25))


# ---- 4. one group: the robust step is the ERM step -------------------------------------------------------------------------------
def test_single_group_equals_erm_step(text_paths_by_dim):
    B, D, H = 64, 128, 128
    x, y, _ = (t.cuda() for t in _batch(B, D, 1))
    g = torch.zeros(B, dtype=torch.int64, device="cuda")
    a, oa = _make(D, H, text_paths_by_dim(D), False)
    b, ob = _make(D, H, text_paths_by_dim(D), False)
    state = adapter.GroupDRO(1, ETA, "cuda")
    for step in range(3):
        la, logits_a, _ = a.train_step(x, y, oa)
        lb, logits_b, _ = b.train_step(x, y, ob, robust=(state, g))
        assert torch.equal(logits_a, logits_b), step
        assert state.q.item() == 1.0
        assert abs(la.item() - lb.item()) <= 1e-6 * abs(la.item())                # (the mean: fp32 tree there, float64 sum here)
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(va, vb), k
    for ma, mb in zip(_momenta(a, oa), _momenta(b, ob)):
        assert torch.equal(ma, mb)


# ---- 5. the replica-batched step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_old", [False, True])
def test_sweep_step_equals_sequential_steps(with_old, text_paths_by_dim):
    R, B, D, H, G, N = 3, 37, 128, 128, 4, 300
    gen = torch.Generator().manual_seed(17)
    table = trainer.EmbeddingTable((torch.randn(N, D, generator=gen) * 0.5).numpy(), torch.randint(0, 2, (N,), generator=gen).numpy(),
                                   torch.randint(0, 2, (N,), generator=gen).numpy(), device="cuda")
    mods = []
    for r in range(R):
        torch.manual_seed(100 + r)
        m = adapter.CustomCLIP(adapter.Adapter(D, H), *text_paths_by_dim(D), temperature=T)
        if with_old:
            import contextlib, io
            with contextlib.redirect_stdout(io.StringIO()):
                m = adapter.MultipleAdapter(m, adapter.Adapter(D, H), init_near_identity=False, ebd_weight=0.5)
        mods.append(m.cuda().train())
    sweep = adapter.SweepAdapters.from_modules(copy.deepcopy(mods), "cuda")
    lrs = [0.05, 0.1, 0.2]
    opts = [optim.SGD([p for n, p in m.named_parameters() if "old_cls" not in n], lr=lrs[r], momentum=MU, weight_decay=WD)
            for r, m in enumerate(mods)]
    states = [adapter.GroupDRO(G, ETA, "cuda") for _ in range(R)]
    stacked = adapter.GroupDRO(G, ETA, "cuda", replicas=R)
    counts = torch.zeros((R, G, 2), dtype=torch.int64, device="cuda")
    loss_sum = torch.zeros((R,), dtype=torch.float64, device="cuda")
    ref_counts = torch.zeros((R, G, 2), dtype=torch.int64, device="cuda")
    ref_sum = [torch.zeros((), dtype=torch.float64, device="cuda") for _ in range(R)]
    names = ("w1", "b1", "gamma", "beta", "running_mean", "running_var", "nbt", "w2", "b2")
    for step in range(3):
        idx = torch.randint(0, N, (R, B), generator=gen).cuda()
        loss, logits, rows = sweep.step(table.embeddings, idx, table.targets, table.targets_group, "class", lrs, MU, WD, counts, loss_sum,
                                        robust=stacked)
        for r, m in enumerate(mods):
            emb, lab, grp = table.batch(idx[r])
            l1, lg1, rw1 = m.train_step(emb, lab, opts[r], robust=(states[r], grp))
            assert torch.equal(logits[r], lg1) and torch.equal(rows[r], rw1) and torch.equal(loss[r], l1), (step, r)
            assert torch.equal(stacked.q[r], states[r].q), (step, r)
            ref_sum[r] += l1.double() * B
            adapter.group_counts(lg1, lab, grp, G, ref_counts[r])
            for name, got, want in zip(names, sweep.new, adapter._adapter_tensors(_trainable(m))):
                assert torch.equal(got[r], want.detach()), (step, r, name)
            if with_old:
                for name, got, want in zip(names, sweep.old, adapter._adapter_tensors(m.old_cls.adapter)):
                    assert torch.equal(got[r], want.detach()), (step, r, "old." + name)
            for k, mb in enumerate(_momenta(m, opts[r])):
                assert torch.equal(sweep.mom[k][r], mb), (step, r, "momentum", k)
        assert torch.equal(counts, ref_counts) and torch.equal(loss_sum, torch.stack(ref_sum)), step
    assert not torch.equal(stacked.q[0], stacked.q[1])


# ---- 6. the schedule ---------------------------------------------------------------------------------------------------------------
def _schedule_opt(method, paths, **k):
    o = dict(batch_size=128, batch_size_reg=16, epochs=2, learning_rate=0.1, learning_rate_reg=0.05, lr_decay_epochs=[6, 7], lr_decay_rate=0.5,
             weight_decay=5e-5, momentum=0.9, dataset="celeba", cosine=False, warm=False, warm_reg=False, train_target="class",
             tl_method=method, balance_val=False, resample_ce=False, use_cls_prompt_in_reg=False, add_adapter=False,
             init_near_identity=False, epochs_feature_learning=1, continue_from_best=False, adapter_feat_dim=128, zs_temperature=0.01,
             random_seed=42, n_cls=2, text_embedding_dir=paths[0], text_spurious_embedding_dir=paths[1], text_group_embedding_dir=paths[2])
    o.update(k)
    return SimpleNamespace(**o)


@pytest.fixture(scope="module")
def schedule_data(tmp_path_factory):
    D, seed = 128, 21
    d = tmp_path_factory.mktemp("gdro_schedule")
    paths = []
    for name, m, cols in zip(("c", "s", "g"), synth.embedding_text(seed, D), (["c0", "c1"], ["s0", "s1"], ["g0", "g1", "g2", "g3"])):
        paths.append(os.path.join(d, name + ".json"))
        json.dump({n: m[:, i].numpy().tolist() for i, n in enumerate(cols)}, open(paths[-1], "w"))
    tables = []
    for split, n in (("train", 512), ("val", 400), ("test", 256)):
        # (class signal strong enough for 128 dimensions that every group scores above 0 after one epoch: a best model exists)
        x, y, c = synth.embedding_dataset(seed, split, n, D, s_class=0.15, s_spur=0.05)
        tables.append(trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda"))
    return paths, tables


def _same_records(a, b):
    assert [e["kind"] for e in a] == [e["kind"] for e in b]
    for ea, eb in zip(a, b):
        if ea["kind"] == "init":
            assert all(torch.equal(ea["state"][k].cpu(), eb["state"][k].cpu()) for k in ea["state"])
        elif ea["kind"] != "final":
            assert ea["loss"] == eb["loss"] and np.array_equal(ea["counts"], eb["counts"]), ea["kind"]
            if "q" in ea:
                assert len(ea["q"]) == len(eb["q"]) and all(np.array_equal(x, y) for x, y in zip(ea["q"], eb["q"]))
        else:
            sa, sb = ea["best_model"].state_dict(), eb["best_model"].state_dict()
            assert ea["best_epoch"] == eb["best_epoch"] and all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.mark.parametrize("method,extra", [("adapter", {}), ("adapter_reg_seq_alter", {"add_adapter": True})], ids=["adapter", "seq_alter_add_adapter"])
def test_schedule_runs_robust_and_equals_sweep(method, extra, schedule_data, monkeypatch):
    paths, tables = schedule_data
    resets = []
    reset = adapter.GroupDRO.reset

    def spy(self):
        assert not torch.allclose(self.q, torch.full_like(self.q, 0.25), atol=1e-5)      # stage 1 had moved it
        reset(self)
        resets.append(self.q.detach().cpu().clone())
    monkeypatch.setattr(adapter.GroupDRO, "reset", spy)
    opt = _schedule_opt(method, paths, robust=True, robust_step_size=0.05, **extra)
    optim.set_seed(42)
    log = []
    trainer.train_all_epochs(opt, *tables, log=log)
    kinds = [e["kind"] for e in log]
    trains = [e for e in log if e["kind"] in ("train1", "train2")]
    assert len(trains) == 2 and all(np.isfinite(e["loss"]) for e in trains)
    for e in trains:                                                             # one q per pass: a distribution, moved off 1 / G
        assert len(e["q"]) == 1 and abs(float(e["q"][0].astype(np.float64).sum()) - 1.0) <= 1e-6
        assert not np.allclose(e["q"][0], 0.25, atol=1e-5)
    if method == "adapter":
        assert kinds.count("train1") == 2 and not resets
    else:                                                                        # efl = 1: epoch 2 is stage 2; q starts over at the switch, once
        assert [e["kind"] for e in trains] == ["train1", "train2"]
        assert len(resets) == 1 and torch.equal(resets[0], torch.full((4,), 0.25))
    # train_sweep with one seed is the run itself; with two seeds (the replica-batched path) replica 0 still is, bit for bit
    for seeds in ([42], [42, 43]):
        del resets[:]
        logs = []
        trainer.train_sweep(opt, *tables, seeds, log=logs)
        _same_records(log, logs[0])
        if method != "adapter":                                                  # (the lock-step run resets its stacked [R, G] state once)
            assert len(resets) == 1 and bool((resets[0] == 0.25).all())
    # without the flag the records carry no q
    plain = _schedule_opt(method, paths, **extra)
    optim.set_seed(42)
    log0 = []
    trainer.train_all_epochs(plain, *tables, log=log0)
    assert all("q" not in e for e in log0)
    assert [e["loss"] for e in log0 if e["kind"] in ("train1", "train2")] != [e["loss"] for e in trains]


def test_linear_probing_with_robust_is_refused(schedule_data):
    paths, tables = schedule_data
    opt = _schedule_opt("linear_probing", paths, robust=True)
    with pytest.raises(ops.DbmmUnsupported):
        trainer.train_all_epochs(opt, *tables)
