"""Out-of-range ids in the head, step and sweep kernels: the contract of include/dbmm.h (at dbmm_l2norm_sim_ce_fwd), each rule against
a plain torch restatement on int64 / float64 tensors written here.  Every comparison of an id is on its 64-bit value:

  * a group id outside [0, G) is in no counter (under group DRO: weight 0, in no n_g or L_g);
  * a label outside [0, C) scores NaN, leaves logits and pred alone, gets no one-hot, is counted in n and never as correct;
  * a row index outside [0, N) in a sweep's idx is clamped to 0 or N - 1 at every use (embedding, label, group, row weight);
  * the argmax behind pred and behind the counters is the FIRST maximum.

The edge values FAR_G / FAR_Y / FAR_I hold 2^32 + k, -(2^32), 2^33 + G - 1 and 2^62 + 1, whose low 32 bits are valid ids: a kernel that
narrows an id to int before comparing it counts such a row as group (class, row) k.  The counters' reference is computed from the
logits the call returned: pred = index of the first maximum, n_g = (grp == g).sum(), correct_g = ((grp == g) & (pred == lab)).sum().
Float results are held to test_gpu_head_shapes.py's bound, e_kernel <= 4 * e_torch + 2^-23 against float64."""
from types import SimpleNamespace

import pytest
import torch

from dbmm_amd import _lib, ops, synth
from test_gpu_head_shapes import F32, F64, head_ref, hold

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, D_AD, H = 64, 128, 128                                       # table rows; the adapter sweeps' width and hidden width
T, MU, WD, ETA, EBD = 0.01, 0.9, 5e-5, 0.01, 0.5
PAD, FILL = 256, -7                                             # guard zones around the counters
I64 = torch.int64


def FAR_G(G):
    return [-1, G, 2 ** 31, 2 ** 32, 2 ** 32 + 1, -(2 ** 32), 2 ** 33 + G - 1, 2 ** 62 + 1]


FAR_Y = FAR_G


def FAR_I(n):
    return [-5, n, n + 7, 2 ** 32 + 3, -(2 ** 40), 2 ** 40]


FAR_ROWS = [1, 4, 9, 12, 17, 22, 27, 30]                        # the table rows that hold FAR_G(G) / FAR_Y(C), in list order
# the order in which a batch meets them: the values whose low 32 bits are a valid id first (2^32 + 1, 2^32, 2^33 + G - 1, -(2^32),
# 2^62 + 1), so that a batch of 5 rows already holds three of them
HIT_ORDER = [4, 3, 6, 5, 7, 0, 1, 2]


def id_column(n_valid, far=None):
    """[N] ids: row i holds i % n_valid, the rows FAR_ROWS the edge values.  Every id below min(n_valid, 8) keeps rows (at
    n_valid = 64 the ids 1, 4, 9, ... of FAR_ROWS lose their only row; id 63 stays at row 63 and FAR_G(64) brings 64)"""
    col = torch.arange(N) % n_valid
    if far is not None:
        col[FAR_ROWS] = torch.tensor(far, dtype=I64)
    return col


def batch_idx(R, B):
    """[R, B] table rows: the rows of FAR_ROWS in HIT_ORDER interleaved with ordinary rows, then the rest of the table; replica r
    starts two places later (so its first row holds the next edge value)"""
    far = [FAR_ROWS[i] for i in HIT_ORDER]
    rest = [i for i in range(N) if i not in FAR_ROWS]
    seq = [v for pair in zip(far, rest[:8]) for v in pair] + rest[8:]
    assert sorted(seq) == list(range(N))
    return torch.tensor([[seq[(b + 2 * r) % N] for b in range(B)] for r in range(R)], dtype=I64)


def first_max(lg):
    cls = torch.arange(lg.shape[-1]).expand_as(lg)
    return torch.where(lg == lg.max(-1, keepdim=True).values, cls, torch.full_like(cls, lg.shape[-1])).min(-1).values


def ref_counts(logits, lab, grp, G):
    """logits [R, B, C], lab / grp int64 [R, B] -> [R, G, 2] (n, correct), the comparisons on int64"""
    logits, lab, grp = logits.detach().cpu(), lab.cpu(), grp.cpu()
    pred = first_max(logits)
    out = torch.zeros((logits.shape[0], G, 2), dtype=I64)
    for g in range(G):
        m = grp == g
        out[:, g, 0] = m.sum(1)
        out[:, g, 1] = (m & (pred == lab)).sum(1)
    return out


def guarded_counts(R, G):
    buf = torch.full((2 * PAD + R * G * 2,), FILL, dtype=I64, device=DEV)
    counts = buf[PAD:PAD + R * G * 2].view(R, G, 2)
    counts.zero_()
    return buf, counts


def guards_intact(buf, R, G):
    return bool((buf[:PAD] == FILL).all()) and bool((buf[PAD + R * G * 2:] == FILL).all())


def loss_acc(R):
    return torch.zeros((R,), dtype=F64, device=DEV)


def prompts(C, D, tie=False):
    text = synth.normal(41, f"ids_text{D}_{C}", (D, C), 1.0)
    if tie:
        text[:, 3] = text[:, 1]
    return (text / text.norm(dim=0, keepdim=True)).t().contiguous()


def table_of(D):
    return synth.normal(42, f"ids_table{D}", (N, D), 0.5)


def row_weights(R=None):
    """distinct per-row weights in [0.25, 2): [N], or [R, N] with every replica's own"""
    w = 0.25 + 1.75 * ((torch.arange(N) * 37) % N).float() / N
    return w if R is None else torch.stack([w + 0.015625 * r for r in range(R)]).contiguous()


# ---- the stacked states ------------------------------------------------------------------------------------------------------------
def adapter_stack(R, seed):
    D = D_AD
    return [synth.normal(seed, "w1", (R, H, D), D ** -0.5), synth.normal(seed, "b1", (R, H), 0.02), synth.uniform(seed, "gamma", (R, H), 0.5, 1.5),
            synth.normal(seed, "beta", (R, H), 0.1), synth.normal(seed, "rmean", (R, H), 0.1), synth.uniform(seed, "rvar", (R, H), 0.5, 1.5),
            torch.zeros((R,), dtype=I64), synth.normal(seed, "w2", (R, D, H), H ** -0.5), synth.normal(seed, "b2", (R, D), 0.02)]


def adapter_state(R, with_old=False, warm=False):
    """R stacked adapters on the device with their momentum buffers (zeros, or `warm`: as after earlier steps) and sweep operands"""
    new = [t.to(DEV) for t in adapter_stack(R, 31)]
    bufs = [(synth.normal(33, f"mom{i}", tuple(new[i].shape), 0.01).to(DEV) if warm else torch.zeros_like(new[i])) for i in (0, 1, 2, 3, 7, 8)]
    old = [t.to(DEV) for t in adapter_stack(R, 32)] if with_old else None
    return SimpleNamespace(R=R, new=new, bufs=bufs, old=old, args=ops.adapter_sweep_args(R, D_AD, H, new, bufs, old))


def adapter_tensors(st):
    return st.new + st.bufs + (st.old or [])


def linear_state(R, C, D, warm=False, tie=False):
    w, b = synth.normal(35, f"lw{C}_{D}", (R, C, D), D ** -0.5), synth.normal(35, f"lb{C}", (R, C), 0.02)
    if tie:
        w[:, 3], b[:, 3] = w[:, 1], b[:, 1]
    mw = synth.normal(36, f"lmw{C}_{D}", (R, C, D), 0.01) if warm else torch.zeros_like(w)
    mb = synth.normal(36, f"lmb{C}", (R, C), 0.01) if warm else torch.zeros_like(b)
    return SimpleNamespace(R=R, w=w.to(DEV), b=b.to(DEV), mw=mw.to(DEV), mb=mb.to(DEV))


def lrs_of(R):
    return [0.05 * (r + 1) for r in range(R)]


def run_adapter(kind, st, table, idx, lab, grp, tn, counts, loss_sum, counted=True, q=None, rw=None, first=True):
    """-> (losses [R] or None, logits [R, B, C], per-row CE [R, B]); `eval` scores the rows of idx[0] with every replica"""
    if kind == "eval":
        return (None,) + tuple(ops.adapter_sweep_eval(table, idx[0].contiguous(), lab, grp, st.args, EBD, tn, T, counts, loss_sum))
    return ops.adapter_sweep_step(table, idx, lab, grp, st.args, EBD, tn, T, lrs_of(st.R), MU, WD, first, counts, loss_sum, counted=counted,
                                  robust=(q, ETA) if kind == "robust" else None, row_weights=rw if kind == "weighted" else None)


def run_linear(kind, st, table, idx, lab, grp, counts, loss_sum, counted=True, rw=None, first=True):
    if kind == "eval":
        return (None,) + tuple(ops.linear_sweep_eval(table, idx[0].contiguous(), lab, grp, st.w, st.b, counts, loss_sum))
    return ops.linear_sweep_step(table, idx, lab, grp, st.w, st.b, st.mw, st.mb, lrs_of(st.R), MU, WD, first, counts, loss_sum, counted=counted,
                                 row_weights=rw if kind == "weighted" else None)


def batch_ids(kind, col, idx):
    """the column's values of the batch rows, [R, B] (eval: the rows of idx[0] for every replica)"""
    rows = idx.clamp(0, N - 1)
    if kind == "eval":
        rows = rows[:1].expand(idx.shape[0], -1)
    return col[rows]


def gdro_ref(rows, grp, q0, eta, G):
    """one online group-DRO update in float64 on per-row CE `rows` [B]; a row whose id is outside [0, G) is in no group, so it has
    weight 0 and is in no n_g or L_g -> (q, robust loss)"""
    rows, q0 = rows.double().cpu(), q0.double().cpu()
    L, n = torch.zeros(G, dtype=F64), torch.zeros(G, dtype=F64)
    for g in range(G):
        m = grp.cpu() == g
        n[g] = m.sum()
        if m.any():
            L[g] = rows[m].mean()
    top = L[n > 0].max() if bool((n > 0).any()) else torch.zeros((), dtype=F64)
    qn = q0 * torch.exp(eta * (L - top))
    q = qn / qn.sum()
    return q, (q * L).sum()


# ---- 1. counters ---------------------------------------------------------------------------------------------------------------------
def check_counters(kind, R, B, C, G, make_state, run, table, lab, tn_args=()):
    """one counted call, a second counted call from the same state on the same counters, and (steps) an uncounted one"""
    grp = id_column(G, FAR_G(G))
    idx = batch_idx(R, B)
    tabd, labd, grpd, idxd = table.to(DEV), lab.to(DEV), grp.to(DEV), idx.to(DEV)
    rw = row_weights().to(DEV)
    buf, counts = guarded_counts(R, G)
    loss_sum = loss_acc(R)
    q = torch.full((R, G), 1.0 / G, device=DEV) if kind == "robust" else None
    kw = dict(q=q, rw=rw) if make_state is adapter_state else dict(rw=rw)
    loss, logits, rows = run(kind, make_state(R), tabd, idxd, labd, grpd, *tn_args, counts, loss_sum, **kw)
    torch.cuda.synchronize()
    b_lab, b_grp = batch_ids(kind, lab, idx), batch_ids(kind, grp, idx)
    want = ref_counts(logits, b_lab, b_grp, G)
    # every edge value the batch holds is outside [0, G), and the batch holds some whose low 32 bits are a valid id
    far = ~((b_grp >= 0) & (b_grp < G))
    assert int(far.sum()) >= min(B, 3) and int(want[:, :, 0].sum()) == b_grp.numel() - int(far.sum())
    assert torch.equal(counts.cpu(), want), (kind, R, B, C, G)
    assert bool(torch.isfinite(rows).all())
    first_sum = loss_sum.clone()
    if kind == "robust":
        for r in range(R):
            q_ref, rl = gdro_ref(rows[r], b_grp[r], torch.full((G,), 1.0 / G), ETA, G)
            got_q = q[r].double().cpu()
            assert bool(((got_q - q_ref).abs() <= 1e-5 * q_ref).all()), (got_q, q_ref)       # the weights kernel's own bounds:
            assert abs(loss[r].item() - rl.item()) <= 1e-5 * abs(rl.item())                  # tests/test_gpu_group_dro.py
            assert abs(got_q.sum().item() - 1.0) <= 1e-6
        assert torch.equal(loss_sum, loss.double() * B)
        q.fill_(1.0 / G)
    loss2, logits2, _ = run(kind, make_state(R), tabd, idxd, labd, grpd, *tn_args, counts, loss_sum, **kw)
    assert torch.equal(logits2, logits) and torch.equal(counts.cpu(), 2 * want) and torch.equal(loss_sum, 2 * first_sum)
    if kind != "eval":
        run(kind, make_state(R), tabd, idxd, labd, grpd, *tn_args, counts, loss_sum, counted=False, **kw)
        assert torch.equal(counts.cpu(), 2 * want) and torch.equal(loss_sum, 2 * first_sum)
    assert guards_intact(buf, R, G)


@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("B", [5, 37])
@pytest.mark.parametrize("kind", ["plain", "weighted", "robust", "eval"])
def test_adapter_sweep_counters(kind, B, R, C):
    table, lab, tn = table_of(D_AD), id_column(C), prompts(C, D_AD).to(DEV)
    for G in ((1, 4, 8) if kind == "robust" else (1, 4, 64)):                    # 64: every LDS counter sc[64][2]; 8: group DRO's limit
        check_counters(kind, R, B, C, G, adapter_state, run_adapter, table, lab, (tn,))


@pytest.mark.parametrize("B", [1, 37, 513])
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("D", [20, 512])
@pytest.mark.parametrize("kind", ["plain", "weighted", "eval"])
def test_linear_sweep_counters(kind, D, C, B):
    table, lab = table_of(D), id_column(C)
    for R in (1, 3):
        for G in (1, 4, 64):
            check_counters(kind, R, B, C, G, lambda r: linear_state(r, C, D), run_linear, table, lab)


# ---- 2. the first maximum on a tie ---------------------------------------------------------------------------------------------------
def check_tie(logits, counts, lab, grp, G):
    lg = logits.detach().cpu()
    assert torch.equal(lg[..., 1], lg[..., 3])                                   # bit-equal: the same operands in the same order
    tie_is_max = lg[..., 1] == lg.max(-1).values
    assert bool(tie_is_max.any())
    assert bool((first_max(lg)[tie_is_max] == 1).all())
    assert torch.equal(counts.cpu(), ref_counts(lg, lab, grp, G))
    return tie_is_max


@pytest.mark.parametrize("kind", ["plain", "weighted", "robust", "eval"])
def test_adapter_tie_takes_the_lower_class(kind):
    """prompts 1 and 3 identical; every label is 1, so a row whose tied logit is the maximum is correct only under the first maximum"""
    R, B, C, G = 2, 37, 5, 4
    table, tn = table_of(D_AD), prompts(C, D_AD, tie=True).to(DEV)
    lab, grp, idx = torch.ones(N, dtype=I64), id_column(G), batch_idx(R, B)
    counts = torch.zeros((R, G, 2), dtype=I64, device=DEV)
    q = torch.full((R, G), 1.0 / G, device=DEV)
    _, logits, _ = run_adapter(kind, adapter_state(R), table.to(DEV), idx.to(DEV), lab.to(DEV), grp.to(DEV), tn, counts, loss_acc(R), q=q,
                               rw=row_weights().to(DEV))
    tie = check_tie(logits, counts, batch_ids(kind, lab, idx), batch_ids(kind, grp, idx), G)
    assert int(counts[:, :, 1].sum()) >= int(tie.sum())


def test_head_pred_tie_takes_the_lower_class():
    B, D, C = 37, 260, 5
    tn = prompts(C, D, tie=True).to(DEV)
    z = synth.normal(43, "tie_z", (B, D), 0.5).to(DEV)
    logits, _, _, pred, _ = ops.l2norm_sim_ce_fwd(z, tn, T, want_pred=True)
    lg = logits.cpu()
    assert torch.equal(lg[:, 1], lg[:, 3])
    tie_is_max = lg[:, 1] == lg.max(1).values
    assert bool(tie_is_max.any())
    assert torch.equal(pred.cpu(), first_max(lg)) and bool((pred.cpu()[tie_is_max] == 1).all())


@pytest.mark.parametrize("kind", ["plain", "weighted", "eval"])
def test_linear_tie_takes_the_lower_class(kind):
    R, B, C, D, G = 2, 37, 5, 260, 4
    lab, grp, idx = torch.ones(N, dtype=I64), id_column(G), batch_idx(R, B)
    counts = torch.zeros((R, G, 2), dtype=I64, device=DEV)
    _, logits, _ = run_linear(kind, linear_state(R, C, D, tie=True), table_of(D).to(DEV), idx.to(DEV), lab.to(DEV), grp.to(DEV), counts, loss_acc(R),
                              rw=row_weights().to(DEV))
    check_tie(logits, counts, batch_ids(kind, lab, idx), batch_ids(kind, grp, idx), G)


# ---- 3. labels outside [0, C) --------------------------------------------------------------------------------------------------------
FAR_B = [1, 3, 5, 8, 11, 14, 17, 20]                            # the batch rows of the head / linear entries that hold FAR_Y(C)


def far_labels(B, C):
    y = torch.arange(B) % C
    rows = [b for b in FAR_B if b < B]
    y[rows] = torch.tensor(FAR_Y(C)[:len(rows)] if len(rows) < 8 else FAR_Y(C), dtype=I64)
    return y


@pytest.mark.parametrize("C", [3, 8])
def test_head_labels_outside_the_classes(C):
    B, D, G = 21, 260, 4
    z, text = synth.normal(44, f"lab_z{C}", (B, D), 0.5), synth.normal(45, f"lab_t{C}", (D, C), 1.0)
    y = far_labels(B, C)
    far = ~((y >= 0) & (y < C))
    assert int(far.sum()) == 8 and -100 not in y.tolist()
    y[0] = -100                                                                  # no ignore_index: one more label outside [0, C)
    far[0] = True
    ones = torch.full((B,), 1.0 / B)
    r64, r32 = head_ref(z, None, text, y, ones, F64), head_ref(z, None, text, y, ones, F32)
    assert torch.equal(torch.isnan(r64["rows"]), far)
    zd, yd = z.to(DEV), y.to(DEV)
    tn = ops.text_colnorm(text.to(DEV))
    lg, rows, mean, pred, inv = ops.l2norm_sim_ce_fwd(zd, tn, T, labels=yd, want_pred=True)
    assert torch.equal(torch.isnan(rows).cpu(), far) and bool(torch.isnan(mean))
    hold("logits", lg, r64["logits"], r32["logits"])
    hold("loss_rows", rows, r64["rows"], r32["rows"])                           # (errs() holds the NaNs to their places)
    assert int((r64["gap"] <= 1e-3).sum()) == 0 and torch.equal(pred.cpu(), r64["pred"])
    dz = ops.l2norm_sim_ce_bwd(zd, inv, tn, T, logits=lg, labels=yd)
    hold("dz", dz, r64["dz"], r32["dz"])
    rw = torch.tensor([0.5, -1.25, 3.5, 0.75, 1.0])[torch.arange(B) % 5]
    w64, w32 = head_ref(z, None, text, y, rw / B, F64), head_ref(z, None, text, y, rw / B, F32)
    hold("dz(rows)", ops.l2norm_sim_ce_bwd_rows(zd, inv, tn, T, lg, yd, rw.to(DEV)), w64["dz"], w32["dz"])
    g, gw = torch.arange(B) % G, torch.tensor([0.5, 0.125, 2.0, 0.03125])
    g64, g32 = head_ref(z, None, text, y, gw[g], F64), head_ref(z, None, text, y, gw[g], F32)
    hold("dz(group weights)", ops.l2norm_sim_ce_bwd_weighted(zd, inv, tn, T, lg, yd, g.to(DEV), gw.to(DEV)), g64["dz"], g32["dz"])
    # a one-hot at the label's low 32 bits would show here: the float64 gradient WITH it differs by far more than the bound
    wrong = head_ref(z, None, text, torch.where(far, (y & 0xFFFFFFFF) % C, y), ones, F64)["dz"]
    assert ((wrong - r64["dz"]).abs().max() / r64["dz"].abs().max()).item() > 1e-2


def linear_ref(x, w, b, y, dtype):
    x, w, b = x.cpu().to(dtype), w.cpu().to(dtype), b.cpu().to(dtype)
    lg = x @ w.t() + b
    valid = (y >= 0) & (y < w.shape[0])
    rows = torch.logsumexp(lg, 1) - lg.gather(1, y.clamp(0, w.shape[0] - 1)[:, None])[:, 0]
    return lg, torch.where(valid, rows, torch.full_like(rows, float("nan")))


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("B", [13, 37], ids=["one_launch", "two_launches"])
def test_linear_labels_outside_the_classes(B, C, option):
    option("linear_step_one_launch_max_b", 16)                                   # B = 13: one launch; B = 37: the two-launch path
    D = 260
    x = synth.normal(46, f"lin_x{B}", (B, D), 0.5)
    y = far_labels(B, C)
    far = ~((y >= 0) & (y < C))
    assert int(far.sum()) == len([b for b in FAR_B if b < B])
    st = linear_state(1, C, D)
    w0, b0 = st.w[0].clone(), st.b[0].clone()
    (lg64, rows64), (lg32, rows32) = linear_ref(x, w0, b0, y, F64), linear_ref(x, w0, b0, y, F32)
    xd, yd = x.to(DEV), y.to(DEV)
    mean, lg, rows = ops.linear_ce_fwd(xd, yd, w0, b0)
    assert torch.equal(torch.isnan(rows).cpu(), far) and bool(torch.isnan(mean))
    hold("fwd logits", lg, lg64, lg32)
    hold("fwd loss_rows", rows, rows64, rows32)
    for rw in (None, (0.25 + torch.arange(B).float() / B).to(DEV)):
        w, b = w0.clone(), b0.clone()
        mw, mb = torch.zeros_like(w), torch.zeros_like(b)
        mean, lg, rows = ops.linear_train_step(xd, yd, w, b, mw, mb, 0.1, MU, WD, True, row_weights=rw)
        assert torch.equal(torch.isnan(rows).cpu(), far) and bool(torch.isnan(mean))
        hold("step logits", lg, lg64, lg32)
        hold("step loss_rows", rows, rows64, rows32)
        assert all(bool(torch.isfinite(t).all()) for t in (w, b, mw, mb)) and not torch.equal(w, w0)


def adapter_fwd_ref(stack, r, x, train, dtype, eps=1e-5):
    w1, b1, gamma, beta, rmean, rvar, _, w2, b2 = [t[r].cpu().to(dtype) if t.dtype != I64 else t for t in stack]
    h = x.to(dtype) @ w1.t() + b1
    mean, var = (h.mean(0), h.var(0, unbiased=False)) if train else (rmean, rvar)
    return torch.relu((h - mean) / torch.sqrt(var + eps) * gamma + beta) @ w2.t() + b2


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("entry", ["adapter_step", "adapter_eval", "linear_step", "linear_eval"])
def test_sweep_labels_outside_the_classes(entry, C):
    R, B, G = 2, 21, 4
    family, kind = entry.split("_")
    kind = "plain" if kind == "step" else "eval"
    D = D_AD if family == "adapter" else 260
    table, lab, grp, idx = table_of(D), id_column(C, FAR_Y(C)), id_column(G), batch_idx(R, B)
    b_lab, b_grp = batch_ids(kind, lab, idx), batch_ids(kind, grp, idx)
    far = ~((b_lab >= 0) & (b_lab < C))
    assert int(far[0].sum()) == 8
    counts, loss_sum = torch.zeros((R, G, 2), dtype=I64, device=DEV), loss_acc(R)
    tn = prompts(C, D)
    if family == "adapter":
        st = adapter_state(R)
        start = [t.clone() for t in st.new]
        loss, logits, rows = run_adapter(kind, st, table.to(DEV), idx.to(DEV), lab.to(DEV), grp.to(DEV), tn.to(DEV), counts, loss_sum)
        params = adapter_tensors(st)
    else:
        st = linear_state(R, C, D)
        start = [st.w.clone(), st.b.clone()]
        loss, logits, rows = run_linear(kind, st, table.to(DEV), idx.to(DEV), lab.to(DEV), grp.to(DEV), counts, loss_sum)
        params = [st.w, st.b, st.mw, st.mb]
    assert torch.equal(torch.isnan(rows).cpu(), far)
    assert bool(torch.isnan(loss_sum).all()) and (loss is None or bool(torch.isnan(loss).all()))
    ones = torch.full((B,), 1.0 / B)
    for r in range(R):
        x = table[idx[0 if kind == "eval" else r].clamp(0, N - 1)]
        ref = []
        for dtype in (F64, F32):
            if family == "adapter":
                z = adapter_fwd_ref(start, r, x, kind != "eval", dtype)
                h = head_ref(z, None, None, b_lab[r], ones, dtype, tn=tn)
                ref.append((h["logits"], h["rows"]))
            else:
                ref.append(linear_ref(x, start[0][r], start[1][r], b_lab[r], dtype))
        hold(f"{entry} r{r} logits", logits[r], ref[0][0], ref[1][0])
        hold(f"{entry} r{r} loss_rows", rows[r], ref[0][1], ref[1][1])
    # counted in n, never as correct: the int64 label equals no class index
    want = ref_counts(logits, b_lab, b_grp, G)
    assert torch.equal(counts.cpu(), want) and int(want[:, :, 0].sum()) == R * B
    pred = first_max(logits.detach().cpu())
    assert int(want[:, :, 1].sum()) == int(((pred == b_lab) & ~far).sum())
    assert all(bool(torch.isfinite(t).all()) for t in params if t.is_floating_point())
    if kind != "eval":
        assert not torch.equal(params[0], start[0])


# ---- 4. the index clamp --------------------------------------------------------------------------------------------------------------
def far_idx(R, B):
    """[R, B] table rows with FAR_I(N) at batch rows r, r + 2, r + 4, ... of replica r"""
    idx = (torch.arange(B)[None, :] * 5 + torch.arange(R)[:, None] * 3) % N
    for r in range(R):
        for k, v in enumerate(FAR_I(N)):
            idx[r, (r + 2 * k) % B] = v
    return idx


def clamp_table(D, C, G):
    """rows 3 and N - 1 differ in embedding, label, group and weight: index 2^32 + 3 read as 32 bits would be row 3, clamped it is N - 1"""
    table, lab, grp = table_of(D), id_column(C), id_column(G)
    lab[N - 1], grp[N - 1] = (lab[3] + 1) % C, (grp[3] + 1) % G
    w1, wR = row_weights(), row_weights(3)
    assert not torch.equal(table[3], table[N - 1]) and lab[3] != lab[N - 1] and grp[3] != grp[N - 1] and w1[3] != w1[N - 1]
    assert not torch.equal(table[0], table[N - 1]) and w1[0] != w1[N - 1] and bool((wR[:, 3] != wR[:, N - 1]).all())
    return table, lab, grp, w1, wR


def check_weighted_mean(loss, rows, rw, idx):
    """the loss a weighted sweep step returns is (1 / B) sum_b CE_b w[table row of b], the weight read at the CLAMPED table row.  Bound:
    B rounded products, B - 1 float32 additions in some order and one division: (B + 2) 2^-24 of (1 / B) sum |terms|"""
    rows, w, tab = rows.double().cpu(), rw.double().cpu(), idx.clamp(0, N - 1)
    B = rows.shape[1]
    for r in range(rows.shape[0]):
        terms = rows[r] * (w if w.dim() == 1 else w[r])[tab[r]]
        assert abs(loss[r].item() - terms.sum().item() / B) <= (B + 2) * 2.0 ** -24 * terms.abs().sum().item() / B, r


ADAPTER_CLAMP = [("plain", False), ("plain", True), ("weighted", False), ("weighted_R", False), ("weighted_R", True), ("robust", False),
                 ("robust", True), ("eval", False), ("eval", True)]


@pytest.mark.parametrize("kind,with_old", ADAPTER_CLAMP, ids=[f"{k}{'_old' if o else ''}" for k, o in ADAPTER_CLAMP])
def test_adapter_sweep_index_clamp(kind, with_old):
    R, B, C, G = 3, 37, 5, 4
    table, lab, grp, w1, wR = clamp_table(D_AD, C, G)
    tn = prompts(C, D_AD).to(DEV)
    idx = far_idx(R, B)
    assert int(((idx < 0) | (idx >= N)).sum()) == R * len(FAR_I(N))
    rw = (wR if kind == "weighted_R" else w1).to(DEV)
    outs = []
    for ix in (idx, idx.clamp(0, N - 1)):
        st = adapter_state(R, with_old, warm=True)
        counts, loss_sum = torch.zeros((R, G, 2), dtype=I64, device=DEV), loss_acc(R)
        q = torch.tensor([[0.1, 0.2, 0.3, 0.4]] * R, device=DEV)
        res = run_adapter(kind.split("_")[0], st, table.to(DEV), ix.to(DEV), lab.to(DEV), grp.to(DEV), tn, counts, loss_sum, q=q, rw=rw, first=False)
        outs.append([t for t in res if t is not None] + adapter_tensors(st) + [counts, loss_sum, q])
    assert len(outs[0]) == len(outs[1])
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), (kind, with_old, i)
    if kind.startswith("weighted"):
        check_weighted_mean(outs[0][0], outs[0][2], rw, idx)
    if kind != "eval":                                                           # the run did train: parameters and momenta moved
        fresh = adapter_state(R, with_old, warm=True)
        assert not torch.equal(outs[0][3], fresh.new[0]) and not torch.equal(outs[0][3 + 9], fresh.bufs[0])


@pytest.mark.parametrize("D", [20, 512])
@pytest.mark.parametrize("kind", ["plain", "weighted", "weighted_R", "eval"])
def test_linear_sweep_index_clamp(kind, D):
    R, B, C, G = 3, 37, 5, 4
    table, lab, grp, w1, wR = clamp_table(D, C, G)
    idx = far_idx(R, B)
    rw = (wR if kind == "weighted_R" else w1).to(DEV)
    outs = []
    for ix in (idx, idx.clamp(0, N - 1)):
        st = linear_state(R, C, D, warm=True)
        counts, loss_sum = torch.zeros((R, G, 2), dtype=I64, device=DEV), loss_acc(R)
        res = run_linear(kind.split("_")[0], st, table.to(DEV), ix.to(DEV), lab.to(DEV), grp.to(DEV), counts, loss_sum, rw=rw, first=False)
        outs.append([t for t in res if t is not None] + [st.w, st.b, st.mw, st.mb, counts, loss_sum])
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), (kind, D, i)
    if kind.startswith("weighted"):
        check_weighted_mean(outs[0][0], outs[0][2], rw, idx)
    if kind != "eval":
        assert not torch.equal(outs[0][3], linear_state(R, C, D, warm=True).w)


def test_clamped_rows_are_the_table_ends():
    """what the two runs above agree on is the right thing: the eval logits of index -5 / -(2^40) are row 0's, those of N, N + 7,
    2^32 + 3 and 2^40 are row N - 1's (bit for bit: every row is scored on its own)"""
    R, C, D, G = 2, 5, 260, 4
    table, lab, grp, _, _ = clamp_table(D, C, G)
    st = linear_state(R, C, D)
    far = torch.tensor(FAR_I(N), dtype=I64)
    ends = torch.where(far < 0, torch.zeros_like(far), torch.full_like(far, N - 1))
    res = []
    for ix in (far, ends):
        counts = torch.zeros((R, G, 2), dtype=I64, device=DEV)
        res.append(ops.linear_sweep_eval(table.to(DEV), ix.to(DEV), lab.to(DEV), grp.to(DEV), st.w, st.b, counts, loss_acc(R)) + (counts,))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    whole = ops.linear_sweep_eval(table.to(DEV), None, lab.to(DEV), grp.to(DEV), st.w, st.b, torch.zeros((R, G, 2), dtype=I64, device=DEV), loss_acc(R))
    assert torch.equal(res[0][0], whole[0][:, ends]) and not torch.equal(whole[0][:, 3], whole[0][:, N - 1])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_sweeps_refuse_rows_outside_the_table_and_too_many_groups():
    R, C, G = 2, 3, 4
    lab, grp = id_column(C).to(DEV), id_column(G).to(DEV)
    tn = prompts(C, D_AD).to(DEV)
    ta, tl = table_of(D_AD).to(DEV), table_of(260).to(DEV)
    ast, lst = adapter_state(R), linear_state(R, C, 260)
    buf, counts = guarded_counts(R, G)
    loss_sum = loss_acc(R)
    for row0, n in ((N - 10, 11), (-1, 5), (N, 1)):
        with pytest.raises(_lib.DbmmError):
            ops.adapter_sweep_eval(ta, None, lab, grp, ast.args, EBD, tn, T, counts, loss_sum, row0=row0, n=n)
        with pytest.raises(_lib.DbmmError):
            ops.linear_sweep_eval(tl, None, lab, grp, lst.w, lst.b, counts, loss_sum, row0=row0, n=n)
    idx = batch_idx(R, 5).to(DEV)
    buf65, c65 = guarded_counts(R, 65)
    for call in (lambda: ops.adapter_sweep_eval(ta, idx[0].contiguous(), lab, grp, ast.args, EBD, tn, T, c65, loss_sum),
                 lambda: ops.adapter_sweep_step(ta, idx, lab, grp, ast.args, EBD, tn, T, lrs_of(R), MU, WD, True, c65, loss_sum),
                 lambda: ops.linear_sweep_eval(tl, idx[0].contiguous(), lab, grp, lst.w, lst.b, c65, loss_sum),
                 lambda: ops.linear_sweep_step(tl, idx, lab, grp, lst.w, lst.b, lst.mw, lst.mb, lrs_of(R), MU, WD, True, c65, loss_sum)):
        with pytest.raises(_lib.DbmmError):
            call()
    buf9, c9 = guarded_counts(R, 9)
    with pytest.raises(_lib.DbmmError):
        ops.adapter_sweep_step(ta, idx, lab, grp, ast.args, EBD, tn, T, lrs_of(R), MU, WD, True, c9, loss_sum,
                               robust=(torch.full((R, 9), 1.0 / 9, device=DEV), ETA))
    torch.cuda.synchronize()
    # a refused call wrote nothing
    assert guards_intact(buf, R, G) and guards_intact(buf65, R, 65) and guards_intact(buf9, R, 9)
    assert not bool(counts.any()) and not bool(c65.any()) and not bool(c9.any()) and not bool(loss_sum.any())
    fresh = adapter_state(R)
    assert all(torch.equal(a, b) for a, b in zip(adapter_tensors(ast), adapter_tensors(fresh)))
