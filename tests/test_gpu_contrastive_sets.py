"""The contrastive adapter's sets head on the MI355X (csrc/supcon_sets.hip): the four kernels against the reference's own
SupervisedContrastiveLoss (tests/golden/contrastive_sets.npz) and the float64 restatement of tests/test_contrastive_sets_host.py,
the one-call step against the autograd path (bits) and against a float64 torch-CPU restatement, and the schedule.

Bound on l_t and L / scale: 2e-5 / tau absolute, the bound tests/test_gpu_supcon.py uses for l_i (the project bounds a cosine by 1e-5;
a shift of at most eps in every s_j moves the logsumexp and the positive mean by at most eps each).  L sums T such terms times scale.
Backward and step: at most 4 x the error of the same formula composed from torch fp32 ops on the device, on the same inputs -- the
margin tests/test_gpu_supcon.py and tests/test_gpu_group_dro.py grant a fixed-order fp32 reduction against torch's order."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dbmm_amd import _lib, adapter, ops, optim, synth, trainer
from test_contrastive_sets_host import head_cases, sets_ref
from test_gpu_group_dro import KEYS, LR, MU, WD, _make, _momenta, _oracle_adapter, text_paths_by_dim  # noqa: F401  (the last one is a fixture)
from test_gpu_supcon import _Guarded

pytestmark = pytest.mark.gpu
C = ops.SETS_CHUNK_ROWS
SCALE, TAU = 0.75 / 4, 0.1
# (T, A, P, N, D): one row of each kind; odd sizes; extra anchors at a D that is no multiple of 64 floats; S = c, c + 1, 2c - 1 (one
# full chunk, one row into the second, one row short of two); several chunks per set with D = 1024 (four 16-byte columns per lane)
SHAPES = [(1, 1, 1, 1, 64), (3, 1, 5, 7, 128), (2, 2, 3, 40, 132), (2, 1, 5, C - 6, 256), (2, 1, 5, C - 5, 256), (2, 1, 5, 2 * C - 7, 256),
          (5, 1, 70, 130, 1024)]
IDS = ["one_each", "odd", "extra_anchors", "S=c", "S=c+1", "S=2c-1", "multi_chunk"]


def _bound(tau):
    return 2e-5 / tau


def _case(T, A, P, N, D):
    """T * S rows of uneven length"""
    B = T * (A + P + N)
    z = synth.normal(31, f"sets_z{B}_{D}", (B, D), 1.0) * synth.uniform(31, f"sets_s{B}_{D}", (B, 1), 0.5, 2.0)
    return z.contiguous()


def _edge_case():
    """tau = 0.01 with a positive equal to the anchor (cos = 1, the logit 100) and duplicated negatives"""
    T, A, P, N, D = 2, 1, 3, 6, 128
    z = _case(T, A, P, N, D).view(T, A + P + N, D).clone()
    z[:, 2] = z[:, 0]
    z[:, 6] = z[:, 5]
    z[:, 9] = 3.0 * z[:, 5]
    return z.view(-1, D).contiguous(), (T, A, P, N)


def _torch_sets(z, sets, scale, tau):
    """the loss composed from torch ops (norm, bmm, logsumexp; autograd for the gradient) in z's dtype, on z's device"""
    T, A, P, N = sets
    zn = (z / z.norm(dim=1, keepdim=True)).view(T, A + P + N, -1)
    s = torch.bmm(zn[:, A:], zn[:, :1].transpose(1, 2)).squeeze(2) / tau
    l = torch.logsumexp(s, dim=1) - s[:, :P].mean(1)
    return scale * l.sum(), l


def _all_cases():
    for (T, A, P, N, D), name in zip(SHAPES, IDS):
        yield name, _case(T, A, P, N, D), (T, A, P, N), TAU
    z, sets = _edge_case()
    yield "edge_tau0.01", z, sets, 0.01


# ---- 1. forward ----------------------------------------------------------------------------------------------------------------------
def test_forward_against_the_reference_class():
    """every golden head case: l_t against the reference class's float64 `loss.mean()` of one call per set, L against their sum.
    Measured on an MI355X: max |l_t - ref| 2.4e-07 ... 6.7e-07, |L - ref| <= 1.2e-06 against bounds of 2e-4 (tau 0.1) and 4e-4 (0.05)."""
    n = 0
    for name, z, (P, N), tau, loss_ref, _ in head_cases():
        T, S, D = z.shape
        L, l, _ = ops.supcon_sets_fwd(torch.from_numpy(z).view(T * S, D).cuda(), (T, 1, P, N), 1.0, tau)
        e_l, e_L = np.abs(l.double().cpu().numpy() - loss_ref).max(), abs(L.item() - loss_ref.sum())
        print(f"{name}: max |l_t - ref| {e_l:.3e}, |L - ref| {e_L:.3e}, bound {_bound(tau):.1e}")
        assert e_l <= _bound(tau) and e_L <= T * _bound(tau), name
        n += 1
    assert n == 6


def test_forward_against_float64():
    """Measured on an MI355X: max |l_t - ref| 3.5e-08 ... 4.0e-07 at tau 0.1 (bound 2e-4), 4.3e-06 in the tau = 0.01 case (bound 2e-3)."""
    for name, z, sets, tau in _all_cases():
        l_ref, L_ref, _ = sets_ref(z.numpy(), sets, SCALE, tau)
        L, l, _ = ops.supcon_sets_fwd(z.cuda(), sets, SCALE, tau)
        assert L.dim() == 0 and tuple(l.shape) == (sets[0],) and torch.isfinite(l).all()
        e_l, e_L = np.abs(l.double().cpu().numpy() - l_ref).max(), abs(L.item() - L_ref)
        print(f"{name}: max |l_t - ref| {e_l:.3e}, |L - ref| {e_L:.3e}, bound {_bound(tau):.1e}")
        assert e_l <= _bound(tau) and e_L <= SCALE * sets[0] * _bound(tau), name
        # L is the float64 sum of the kernel's own l_t in set order, times scale, rounded once
        acc = 0.0
        for v in l.double().cpu().numpy():
            acc += v
        assert L.item() == float(np.float32(float(np.float32(SCALE)) * acc)), name


# ---- 2. backward ---------------------------------------------------------------------------------------------------------------------
def test_backward_against_float64():
    """err = max|dz - ref| / max|ref| against the float64 restatement; allowed: 4 x the same error of the torch fp32 composition on
    the device.  The rows of extra anchors are exactly zero.
    Measured on an MI355X, kernel err (ratio to the torch composition's): one_each 3.9e-07 (0.90), odd 2.0e-07 (0.73), extra_anchors
    2.3e-07 (1.06), S=c 2.1e-07 (1.21), S=c+1 2.8e-07 (1.08), S=2c-1 2.2e-07 (0.54), multi_chunk 1.8e-07 (0.38), tau 0.01 1.1e-07 (0.82)."""
    for name, z, sets, tau in _all_cases():
        T, A, P, N = sets
        ref = torch.from_numpy(sets_ref(z.numpy(), sets, SCALE, tau)[2])
        zd = z.cuda()
        _, _, ws = ops.supcon_sets_fwd(zd, sets, SCALE, tau)
        dz = ops.supcon_sets_bwd(zd, sets, SCALE, tau, ws)
        zt = zd.clone().requires_grad_()
        _torch_sets(zt, sets, SCALE, tau)[0].backward()
        err = lambda a: ((a.double().cpu() - ref).abs().max() / ref.abs().max()).item()
        e_k, e_t = err(dz), err(zt.grad)
        print(f"{name}: kernel err {e_k:.3e}, torch fp32 err {e_t:.3e}, ratio {e_k / e_t:.2f} (allowed 4)")
        assert torch.isfinite(dz).all() and e_k <= 4 * e_t, name
        if A > 1:
            extra = dz.view(T, A + P + N, -1)[:, 1:A]
            assert extra.numel() and not extra.any(), name


def test_autograd_function_scales_with_the_incoming_gradient():
    z, sets = _case(3, 1, 5, 7, 128).cuda(), (3, 1, 5, 7)
    za, zb = z.clone().requires_grad_(), z.clone().requires_grad_()
    La, la = adapter._SetsFn.apply(za, sets, SCALE, TAU)
    Lb, _ = adapter._SetsFn.apply(zb, sets, SCALE, TAU)
    La.backward(); (2.0 * Lb).backward()
    assert not la.requires_grad and torch.equal(zb.grad, 2.0 * za.grad) and za.grad.abs().max() > 0


# ---- 3. same inputs, same bits; guard zones ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5], SHAPES[6]], ids=[IDS[2], IDS[5], IDS[6]])
def test_repeatable_and_inside_its_buffers(shape, monkeypatch):
    """two calls on the same inputs give the same bits; outputs and workspace sit between guard zones, and the guards stay intact"""
    T, A, P, N, D = shape
    sets, zd = (T, A, P, N), _case(*shape).cuda()
    ga = _Guarded()
    monkeypatch.setattr(ops, "_empty", ga)
    runs = []
    for _ in range(2):
        L, l, ws = ops.supcon_sets_fwd(zd, sets, SCALE, TAU)
        runs.append((L, l, ops.supcon_sets_bwd(zd, sets, SCALE, TAU, ws)))
    torch.cuda.synchronize()
    assert len(ga.bufs) == 6                                               # per run: the workspace, (l_t, L), dz
    ga.check()
    assert ws.numel() * 4 == _lib.lib().dbmm_supcon_sets_workspace_bytes(T, A + P + N, D)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 4. the one-call step ---------------------------------------------------------------------------------------------------------------
STEP_SETS, STEP_D, STEP_H = (3, 1, 5, 7), 1024, 128


def _step_x(D=STEP_D):
    T, A, P, N = STEP_SETS
    return synth.normal(5, f"sets_x{D}", (T * (A + P + N), D), 0.5)


def test_one_call_step_equals_autograd_path(text_paths_by_dim):
    """sets_step and sets_loss(...).backward(); optimizer.step() from the same state: the same bits for the losses, parameters,
    momentum buffers and BatchNorm running statistics after three steps"""
    x = _step_x().cuda()
    a, oa = _make(STEP_D, STEP_H, text_paths_by_dim(STEP_D), False)
    b, ob = _make(STEP_D, STEP_H, text_paths_by_dim(STEP_D), False)
    for step in range(3):
        La, la = a.sets_loss(x, sets=STEP_SETS, contrastive=(SCALE, TAU))
        oa.zero_grad(); La.backward(); oa.step()
        Lb, lb = b.sets_step(x, ob, sets=STEP_SETS, contrastive=(SCALE, TAU))
        assert Lb.dim() == 0 and Lb.is_cuda and Lb.item() > 0 and tuple(lb.shape) == (STEP_SETS[0],)
        assert torch.equal(La.detach(), Lb) and torch.equal(la, lb), step
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["adapter.layers.1.num_batches_tracked"].item() == 3
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k                                # parameters and running statistics
    for ma, mb in zip(_momenta(a, oa), _momenta(b, ob)):
        assert torch.equal(ma, mb)


def test_generic_shape_and_multiple_adapter(text_paths_by_dim):
    """off the adapter's fast shape the one-call step raises DbmmUnsupported and the autograd path runs; MultipleAdapter raises"""
    D, H = 64, 16
    x = _step_x(D).cuda()
    clf, opt = _make(D, H, text_paths_by_dim(D), False)
    with pytest.raises(ops.DbmmUnsupported):
        clf.sets_step(x, opt, sets=STEP_SETS, contrastive=(SCALE, TAU))
    before = {k: v.clone() for k, v in clf.adapter.state_dict().items()}
    L, l = clf.sets_loss(x, sets=STEP_SETS, contrastive=(SCALE, TAU))
    opt.zero_grad(); L.backward(); opt.step()
    assert torch.isfinite(L) and torch.isfinite(l).all()
    assert not torch.equal(before["layers.3.weight"], clf.adapter.state_dict()["layers.3.weight"])
    multi, mopt = _make(D, H, text_paths_by_dim(D), True)
    with pytest.raises(ops.DbmmUnsupported):
        multi.sets_loss(x, sets=STEP_SETS, contrastive=(SCALE, TAU))
    with pytest.raises(ops.DbmmUnsupported):
        multi.sets_step(x, mopt, sets=STEP_SETS, contrastive=(SCALE, TAU))


def _torch_run(D, H, x, dtype, device, steps=3):
    """`steps` SGD-momentum steps composed from torch ops from the state _make() loads: train-mode BatchNorm over the whole step
    batch, normalise, set loss, SGD with momentum -> {key: update of the trainable tensor}"""
    x = x.to(device=device, dtype=dtype)
    new = {k: v.to(device=device, dtype=dtype) for k, v in synth.adapter_state_dict(3, D, H).items()}
    start = {k: new[k].clone() for k in KEYS}
    bufs = {}
    for _ in range(steps):
        ps = {k: new[k].clone().requires_grad_() for k in KEYS}
        z, _, _ = _oracle_adapter(ps, x)
        _torch_sets(z, STEP_SETS, SCALE, TAU)[0].backward()
        for k in KEYS:
            gr = ps[k].grad + WD * new[k]
            bufs[k] = gr if k not in bufs else MU * bufs[k] + gr
            new[k] = new[k] - LR * bufs[k]
    return {k: (new[k] - start[k]).double().cpu() for k in KEYS}


def test_step_against_float64_oracle(text_paths_by_dim):
    """Three consecutive steps (the momentum carries over): per trainable tensor, err = max|update - update_ref| / max|update_ref| of
    the three steps' total update against the float64 torch-CPU restatement; allowed 4 x the same error of the fp32 torch composition
    on the device.  layers.0.bias as in tests/test_gpu_supcon.py: its gradient is analytically zero (a bias in front of train-mode
    BatchNorm), so its update is bounded absolutely, 4 x 1e-5 on the gradient through three momentum steps.
    Measured on an MI355X, fused err -> torch fp32 err: layers.0.weight 6.9e-07 -> 9.6e-07, layers.1.weight 8.2e-06 -> 1.0e-05,
    layers.1.bias 1.1e-06 -> 1.3e-06, layers.3.weight 2.5e-06 -> 2.7e-06, layers.3.bias 4.4e-06 -> 4.4e-06; layers.0.bias 6.8e-03 of
    its own tiny update (the torch composition: 5.7e-03)."""
    x = _step_x()
    ref = _torch_run(STEP_D, STEP_H, x, torch.float64, "cpu")
    t32 = _torch_run(STEP_D, STEP_H, x, torch.float32, "cuda")
    clf, opt = _make(STEP_D, STEP_H, text_paths_by_dim(STEP_D), False)
    start = {k: v.detach().clone() for k, v in clf.adapter.state_dict().items() if k in KEYS}
    xd = x.cuda()
    for _ in range(3):
        L, _ = clf.sets_step(xd, opt, sets=STEP_SETS, contrastive=(SCALE, TAU))
        assert torch.isfinite(L)
    sd = clf.adapter.state_dict()
    got = {k: (sd[k].double() - start[k].double()).cpu() for k in KEYS}
    err = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    for k in KEYS:
        print(f"{k}: fused err {err(got[k], ref[k]):.3e}, torch fp32 err {err(t32[k], ref[k]):.3e}, allowed {4 * err(t32[k], ref[k]):.3e}")
    for k in KEYS:
        if k == "layers.0.bias":
            assert (got[k] - ref[k]).abs().max().item() <= 4 * 1e-5 * LR * (1 + 1.9 + 2.71), k
        else:
            assert err(got[k], ref[k]) <= 4 * err(t32[k], ref[k]), k


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_operands():
    z, sets = _case(3, 1, 5, 7, 128), (3, 1, 5, 7)
    with pytest.raises(_lib.DbmmError):
        ops.supcon_sets_fwd(z, sets, SCALE, TAU)                           # CPU tensors
    _, _, ws = ops.supcon_sets_fwd(z.cuda(), sets, SCALE, TAU)
    with pytest.raises(_lib.DbmmError):
        ops.supcon_sets_bwd(z, sets, SCALE, TAU, ws)
    with pytest.raises(RuntimeError):
        ops.supcon_sets_fwd(z.cuda()[:-1].contiguous(), sets, SCALE, TAU)  # a row count other than T * S
    with pytest.raises(RuntimeError):
        ops.supcon_sets_bwd(z.cuda(), (3, 1, 5, 8), SCALE, TAU, ws)
    with pytest.raises(ValueError):
        ops.supcon_sets_fwd(z.cuda(), (3, 1, 0, 12), SCALE, TAU)
    with pytest.raises(_lib.DbmmError):
        ops.supcon_sets_fwd(z.cuda().double(), sets, SCALE, TAU)
    table = z.cuda()
    idx = torch.arange(12, device="cuda").view(3, 4)
    assert torch.equal(ops.gather_sets(table, idx), table[:12])
    with pytest.raises(_lib.DbmmError):
        ops.gather_sets(table, idx.int())                                  # int32 index tensors
    with pytest.raises(_lib.DbmmError):
        ops.gather_sets(table, idx.cpu())


# ---- 6. the schedule ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contrastive_data(tmp_path_factory):
    D, seed = 128, 21
    d = tmp_path_factory.mktemp("contrastive_schedule")
    paths = []
    for name, m, cols in zip(("c", "s", "g"), synth.embedding_text(seed, D), (["c0", "c1"], ["s0", "s1"], ["g0", "g1", "g2", "g3"])):
        paths.append(os.path.join(d, name + ".json"))
        json.dump({n: m[:, i].numpy().tolist() for i, n in enumerate(cols)}, open(paths[-1], "w"))
    tables = []
    for split, n in (("train", 400), ("val", 300), ("test", 256)):
        x, y, c = synth.embedding_dataset(seed, split, n, D, s_class=0.15, s_spur=0.05)
        y_pred = np.where(np.random.default_rng(seed + n).random(n) < 0.12, 1 - y.numpy(), y.numpy())    # unequal slices, ~50 failures
        tables.append(trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), y_pred=y_pred, device="cuda"))
    opt = SimpleNamespace(tl_method="contrastive_adapter", adapter_feat_dim=128, zs_temperature=0.01, train_target="class", epochs=2,
                          batch_size=128, learning_rate=0.01, momentum=0.9, weight_decay=5e-5, cosine=False, lr_decay_epochs=[6, 7],
                          lr_decay_rate=0.5, warm=False, num_positive=4, num_negative=6, batch_factor=4, contrastive_weight=0.75,
                          cl_temperature=0.1, text_embedding_dir=paths[0], text_spurious_embedding_dir=paths[1],
                          text_group_embedding_dir=paths[2])
    return opt, tables


def _schedule(opt, tables, seed):
    optim.set_seed(seed)
    log = []
    out = trainer.train_contrastive_adapter(opt, *tables, log=log)
    return out, log


def test_schedule_runs_and_repeats(contrastive_data):
    """The contrastive loss alone does not tie the adapter's output to the class prompts, so on synthetic tables whether every group of
    the val split scores above 0 -- the condition for a best model -- depends on the initialisation: seeds 42 and 43 at lr 0.01 do."""
    opt, tables = contrastive_data
    out_a, log_a = _schedule(opt, tables, 42)
    out_b, log_b = _schedule(opt, tables, 42)
    _, log_c = _schedule(opt, tables, 43)
    assert [e["kind"] for e in log_a] == ["init", "sets"] + ["train_cl", "validate", "validate"] * 2 + ["validate_zs", "validate_zs", "final"]
    n_sets = int((tables[0].targets != tables[0].y_pred).sum().item())
    for e in log_a:
        if e["kind"] == "train_cl":
            assert np.isfinite(e["loss"]) and e["loss"] > 0 and e["n_sets"] == n_sets and e["n_steps"] == -(-n_sets // opt.batch_factor)
        elif e["kind"] in ("validate", "validate_zs"):
            assert np.isfinite(e["loss"]) and 0.0 <= e["acc"] <= 1.0
    assert isinstance(log_a[-1]["best_model"], adapter.CustomCLIP) and log_a[-1]["best_epoch"] in (1, 2)
    (tr, va, te), (zc, zs) = out_a
    assert np.isfinite(tr["loss"]) and va["worst_acc"] > 0 and "worst_acc" in te and "mean_acc" in zc and "mean_acc" in zs
    assert out_a == out_b
    for ea, eb in zip(log_a, log_b):                                       # the same seed: the same records
        if ea["kind"] == "init":
            assert all(torch.equal(ea["state"][k], eb["state"][k]) for k in ea["state"])
        elif ea["kind"] in ("sets", "train_cl"):
            assert np.array_equal(ea["order"], eb["order"]) and ea.get("loss") == eb.get("loss")
        elif ea["kind"] == "final":
            sa, sb = ea["best_model"].state_dict(), eb["best_model"].state_dict()
            assert ea["best_epoch"] == eb["best_epoch"] and all(torch.equal(sa[k], sb[k]) for k in sa)
        else:
            assert ea["loss"] == eb["loss"] and np.array_equal(ea["counts"], eb["counts"])
    assert not np.array_equal(log_a[1]["order"], log_c[1]["order"])        # another seed: other sets
    with pytest.raises(ValueError):                                        # the general schedule keeps refusing the method by name
        trainer.train_all_epochs(opt, *tables)
