"""Debiasing-adapter classes and step helpers with the reference's call signatures
(/root/reference/final_main.py:43-174, 383-424) over the MI355X kernels.

Module protocol kept: ordinary nn.Parameters, state-dict keys
`adapter.layers.{0,1,3}.*` / `old_cls.adapter.layers.*` / `new_adapter.layers.*`,
`.train()/.eval()`, `copy.deepcopy`, `loss.backward()` through torch.autograd.Function
wrappers whose forward/backward call the C ABI.  There is no torch fallback: CPU tensors
raise.

Two ways to take a training step:
  * drop-in: `logits = classifier(x.detach(), use_group)` then any torch criterion
    (final_main.py:455-466) -- the criterion's d(loss)/d(logits) is fed to the fused
    normalise+similarity backward kernel.
  * fused:   `loss, logits = classifier.loss(x, labels, use_group)` -- row L2-norm, image x
    text logits and mean cross-entropy in one kernel (and one backward kernel).
"""
import json
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops


class LinearClassifier(nn.Module):
    """Linear probing head (final_main.py:43-49) on the MFMA GEMM."""
    def __init__(self, input_dim, num_classes=2):
        super().__init__()
        self.fc = nn.Linear(input_dim, num_classes)

    def forward(self, features):
        return _LinearFn.apply(features, self.fc.weight, self.fc.bias)

    def loss(self, features, labels, use_group=False, spurious=False):
        """eval forward (validate, final_main.py:655-713): (mean CE, logits, per-row CE) in one launch.  The reference's
        LinearClassifier has no prompts, so `use_group` / `spurious` cannot apply to it."""
        if use_group or spurious:
            raise ValueError("LinearClassifier has no group / spurious prompts (final_main.py:43-49)")
        with torch.no_grad():
            return ops.linear_ce_fwd(features.detach().contiguous(), labels.contiguous(), self.fc.weight.detach(), self.fc.bias.detach())

    def train_step(self, features, labels, optimizer, use_group=False, row_weights=None):
        """The step body of train_one_epoch (final_main.py:455-466) for the linear probe -- logits, mean CE, backward and the
        SGD-momentum update -- as ONE C call (one kernel launch up to the library's one-launch batch size).  Uses the optimiser's
        lr / momentum / weight_decay and its `momentum_buffer` state, so it mixes freely with `loss.backward(); optimizer.step()`.
        Requires train mode.  Returns (mean CE, logits, per-row CE), all on the device.  `row_weights` (float32 [B], taken as they
        are): the step minimises and returns (1 / B) sum_b w_b CE_b, in the same launches; per-row CE stays unweighted."""
        if use_group:
            raise ValueError("LinearClassifier.forward takes no use_group (final_main.py:43-49)")
        if not self.training:
            raise RuntimeError("train_step needs classifier.train()")
        w, b = self.fc.weight, self.fc.bias
        owned = [p for g in optimizer.param_groups for p in g["params"]]
        if len(optimizer.param_groups) != 1 or len(owned) != 2 or {id(p) for p in owned} != {id(w), id(b)}:
            raise RuntimeError("train_step: the optimiser must hold exactly fc.weight and fc.bias in one param group")
        group = optimizer.param_groups[0]
        first = False
        bufs = []
        for p in (w, b):
            st = optimizer.state[p]
            if st.get("momentum_buffer") is None:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                first = True
            bufs.append(st["momentum_buffer"])
        with torch.no_grad():
            return ops.linear_train_step(features.detach().contiguous(), labels.contiguous(), w.data, b.data, bufs[0], bufs[1],
                                         group["lr"], group.get("momentum", 0.0), group.get("weight_decay", 0.0), first,
                                         row_weights=row_weights)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x = x.contiguous()
        ctx.save_for_backward(x, w)
        return ops.gemm(x, w.detach(), b.detach())

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        # dW[n][k] = sum_b g[b][n] x[b][k]: the batch-major operand needs 16-B rows, so the
        # num_classes columns of g are zero-padded to a multiple of 4.
        n = w.shape[0]
        npad = (n + 3) // 4 * 4
        gp = torch.zeros((g.shape[0], npad), device=g.device)
        gp[:, :n] = g
        dw = ops.gemm(gp, x, trans_a=True, trans_w=True)[:n]
        db = ops.colsum(gp)[:n]
        dx = None
        if ctx.needs_input_grad[0]:
            wp = torch.zeros((npad, w.shape[1]), device=w.device); wp[:n] = w
            dx = ops.gemm(gp, wp, trans_w=True)
        return dx, dw, db


class _AdapterFn(torch.autograd.Function):
    """Adapter.forward as one fused op: Linear -> BatchNorm1d -> ReLU -> Linear."""

    @staticmethod
    def forward(ctx, x, w1, b1, gamma, beta, w2, b2, bn, training):
        x = x.contiguous()
        if training and x.shape[0] < 2:
            raise ValueError("Expected more than 1 value per channel when training (BatchNorm1d)")
        z, h, mean, invstd, r = ops.adapter_fwd(x, w1.detach(), b1.detach(), gamma.detach(), beta.detach(),
                                                bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                                w2.detach(), b2.detach(), training, bn.eps, bn.momentum)
        if not training:
            # eval-mode backward is not needed by the reference (validate() runs under no_grad)
            mean, invstd = bn.running_mean, torch.rsqrt(bn.running_var + bn.eps)
        ctx.save_for_backward(x, h, mean, invstd, r, gamma, beta, w1, w2)
        ctx.training = training
        return z

    @staticmethod
    def backward(ctx, dz):
        x, h, mean, invstd, r, gamma, beta, w1, w2 = ctx.saved_tensors
        if not ctx.training:
            raise RuntimeError("dbmm_amd Adapter: backward in eval mode is not implemented "
                               "(the reference never back-propagates through eval-mode BatchNorm)")
        dw1, db1, dgamma, dbeta, dw2, db2, dh = ops.adapter_bwd(x, dz.contiguous(), h, mean, invstd, r,
                                                                gamma.detach(), beta.detach(), w2.detach())
        dx = ops.gemm(dh, w1.detach(), trans_w=True) if ctx.needs_input_grad[0] else None
        return dx, dw1, db1, dgamma, dbeta, dw2, db2, None, None


class Adapter(nn.Module):
    """final_main.py:160-174; `layers` keeps the reference's Sequential so the state-dict keys
    (`layers.0`, `layers.1`, `layers.3`) and deepcopy/load_state_dict behave identically."""
    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.BatchNorm1d(hidden_dim), nn.ReLU(),
                                    nn.Linear(hidden_dim, input_dim))

    def forward(self, features):
        l0, bn, l3 = self.layers[0], self.layers[1], self.layers[3]
        return _AdapterFn.apply(features, l0.weight, l0.bias, bn.weight, bn.bias, l3.weight, l3.bias, bn,
                                self.training)


class _SimFn(torch.autograd.Function):
    """logits = (w*norm(z_old) + (1-w)*norm(z)) @ colnorm(text) / T with z_old detached."""

    @staticmethod
    def forward(ctx, z, z_old, tn, temperature, ebd_weight):
        logits, _, _, _, inv_norm = ops.l2norm_sim_ce_fwd(z, tn, temperature, z_old=z_old, ebd_weight=ebd_weight)
        ctx.save_for_backward(z, inv_norm, tn)
        ctx.cfg = (temperature, ebd_weight, z_old is not None)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        z, inv_norm, tn = ctx.saved_tensors
        T, w, blended = ctx.cfg
        dz = ops.l2norm_sim_ce_bwd(z, inv_norm, tn, T, dlogits=dlogits.contiguous(), blended=blended, ebd_weight=w)
        return dz, None, None, None, None


class _SimCEFn(torch.autograd.Function):
    """Fused logits + mean cross-entropy; returns (loss, logits)."""

    @staticmethod
    def forward(ctx, z, z_old, tn, temperature, ebd_weight, labels):
        logits, loss_rows, loss_mean, _, inv_norm = ops.l2norm_sim_ce_fwd(z, tn, temperature, labels=labels,
                                                                          z_old=z_old, ebd_weight=ebd_weight)
        ctx.save_for_backward(z, inv_norm, tn, logits, labels)
        ctx.cfg = (temperature, ebd_weight, z_old is not None)
        ctx.mark_non_differentiable(logits, loss_rows)
        return loss_mean, logits, loss_rows

    @staticmethod
    def backward(ctx, gloss, _gl, _gr):
        z, inv_norm, tn, logits, labels = ctx.saved_tensors
        T, w, blended = ctx.cfg
        # gloss is a 0-dim device tensor (1.0 for loss.backward()); fold it in on device
        dz = ops.l2norm_sim_ce_bwd(z, inv_norm, tn, T, logits=logits, labels=labels, blended=blended, ebd_weight=w)
        return dz * gloss, None, None, None, None, None


class _SimCEWeightedFn(torch.autograd.Function):
    """Fused logits + cross-entropy under fixed per-row weights: returns (L = (1 / B) sum_b w_b CE_b, logits, per-row CE).  The
    launches of _SimCEFn (forward rows, mean; backward rows), each reading the weights; the one-call step's bits."""

    @staticmethod
    def forward(ctx, z, z_old, tn, temperature, ebd_weight, labels, row_w):
        logits, loss_rows, _, _, inv_norm = ops.l2norm_sim_ce_fwd(z, tn, temperature, labels=labels, z_old=z_old, ebd_weight=ebd_weight,
                                                                  want_mean=False)
        loss = ops.weighted_mean(loss_rows, row_w)
        ctx.save_for_backward(z, inv_norm, tn, logits, labels, row_w)
        ctx.cfg = (temperature, ebd_weight, z_old is not None)
        ctx.mark_non_differentiable(logits, loss_rows)
        return loss, logits, loss_rows

    @staticmethod
    def backward(ctx, gloss, _gl, _gr):
        z, inv_norm, tn, logits, labels, row_w = ctx.saved_tensors
        T, w, blended = ctx.cfg
        dz = ops.l2norm_sim_ce_bwd_rows(z, inv_norm, tn, T, logits, labels, row_w, blended=blended, ebd_weight=w)
        return dz * gloss, None, None, None, None, None, None


def _row_weight_operands(row_weights, robust, contrastive):
    """a `row_weights=` argument beside the other heads' arguments: they do not combine (raised before anything is launched)"""
    if robust is not None or contrastive is not None:
        raise ops.DbmmUnsupported("row_weights= does not combine with robust= or contrastive=: those heads have no per-row weighted form")
    return row_weights


class GroupDRO:
    """State of online group DRO (Sagawa et al. 2020, Algorithm 1): the adversarial group distribution `q` (float32 [n_groups] on the
    device, or [replicas, n_groups] for a sweep), initialised to 1 / n_groups, and its step size.  A robust step -- `loss(...,
    robust=(state, groups))`, `train_step(..., robust=(state, groups))`, `SweepAdapters.step(..., robust=state)` -- updates `q` in
    place from the batch's group losses and minimises sum_g q_g L_g.  Holds one tensor and two numbers: deepcopy and pickle work."""

    def __init__(self, n_groups, step_size=0.01, device="cuda", replicas=None):
        if not 1 <= int(n_groups) <= ops.GDRO_MAX_GROUPS:
            raise ValueError(f"GroupDRO: n_groups must be in 1 .. {ops.GDRO_MAX_GROUPS}, got {n_groups}")
        self.n_groups, self.step_size = int(n_groups), float(step_size)
        shape = (self.n_groups,) if replicas is None else (int(replicas), self.n_groups)
        self.q = torch.full(shape, 1.0 / self.n_groups, dtype=torch.float32, device=device)

    def reset(self):
        """q = 1 / n_groups again (a new stage of the schedule)"""
        self.q.fill_(1.0 / self.n_groups)


class _SimCERobustFn(torch.autograd.Function):
    """Fused logits + group-DRO loss; returns (robust loss, logits, per-row CE).  Three launches: forward rows, group reduction + q
    update (in place, in the forward), weighted backward rows."""

    @staticmethod
    def forward(ctx, z, z_old, tn, temperature, ebd_weight, labels, groups, q, eta):
        logits, loss_rows, _, _, inv_norm = ops.l2norm_sim_ce_fwd(z, tn, temperature, labels=labels, z_old=z_old, ebd_weight=ebd_weight,
                                                                  want_mean=False)
        robust, stats = ops.group_dro_weights(loss_rows, groups, q, eta)
        ctx.save_for_backward(z, inv_norm, tn, logits, labels, groups, stats)
        ctx.cfg = (temperature, ebd_weight, z_old is not None)
        ctx.mark_non_differentiable(logits, loss_rows)
        return robust, logits, loss_rows

    @staticmethod
    def backward(ctx, gloss, _gl, _gr):
        z, inv_norm, tn, logits, labels, groups, stats = ctx.saved_tensors
        T, w, blended = ctx.cfg
        dz = ops.l2norm_sim_ce_bwd_weighted(z, inv_norm, tn, T, logits, labels, groups, stats[0], blended=blended, ebd_weight=w)
        return dz * gloss, None, None, None, None, None, None, None, None


def _robust_operands(robust, n_rows):
    """(groups, q, eta) of a `robust=(state, groups)` argument"""
    state, groups = robust
    if not isinstance(state, GroupDRO) or state.q.dim() != 1:
        raise TypeError("robust=(GroupDRO state of one run, group ids of the batch) expected")
    groups = groups.contiguous()
    if groups.numel() != n_rows:
        raise RuntimeError(f"robust: {groups.numel()} group ids for a batch of {n_rows} rows")
    return groups, state.q, state.step_size


class _SimCESupConFn(torch.autograd.Function):
    """Fused logits + mean CE mixed with the supervised-contrastive loss of z: returns (mixed loss, logits, per-row CE, L_con).  The
    launches of the one-call step's head: CE rows forward, Gram tiles, reduction + mixed loss; CE rows backward, contrastive
    backward onto the CE head's dz."""

    @staticmethod
    def forward(ctx, z, z_old, tn, temperature, ebd_weight, labels, weight, tau):
        logits, loss_rows, _, _, inv_norm = ops.l2norm_sim_ce_fwd(z, tn, temperature, labels=labels, z_old=z_old, ebd_weight=ebd_weight,
                                                                  want_mean=False)
        con, _, stats, n_anchors, ws, mixed = ops.supcon_fwd(z, labels, tau, ce_rows=loss_rows, weight=weight)
        ctx.save_for_backward(z, inv_norm, tn, logits, labels, stats, n_anchors, ws)
        ctx.cfg = (temperature, ebd_weight, z_old is not None, weight, tau)
        ctx.mark_non_differentiable(logits, loss_rows, con)
        return mixed, logits, loss_rows, con

    @staticmethod
    def backward(ctx, gloss, _gl, _gr, _gc):
        z, inv_norm, tn, logits, labels, stats, n_anchors, ws = ctx.saved_tensors
        T, w, blended, weight, tau = ctx.cfg
        dz = ops.l2norm_sim_ce_bwd(z, inv_norm, tn, T, logits=logits, labels=labels, blended=blended, ebd_weight=w)
        dz = ops.supcon_bwd(z, labels, tau, stats, n_anchors, ws, weight, dz_in=dz, dz_in_scale=ops.supcon_ce_weight(weight))
        return dz * gloss, None, None, None, None, None, None, None


class _SetsFn(torch.autograd.Function):
    """The contrastive loss of T sampled sets [anchor(s); positives; negatives] of adapter outputs z: returns (L = scale * sum_t
    l_t, l_t).  The head's four launches: forward rows, reduction; backward rows, anchor merge (csrc/supcon_sets.hip)."""

    @staticmethod
    def forward(ctx, z, sets, scale, tau):
        z = z.contiguous()
        loss, loss_sets, ws = ops.supcon_sets_fwd(z, sets, scale, tau)
        ctx.save_for_backward(z, ws)
        ctx.cfg = (sets, scale, tau)
        ctx.mark_non_differentiable(loss_sets)
        return loss, loss_sets

    @staticmethod
    def backward(ctx, gloss, _gs):
        z, ws = ctx.saved_tensors
        sets, scale, tau = ctx.cfg
        return ops.supcon_sets_bwd(z, sets, scale, tau, ws) * gloss, None, None, None


def _sets_operands(sets, contrastive):
    """((T, A, P, N), scale, tau) of `sets=(T, A, P, N)` and `contrastive=(scale, temperature)`"""
    T, A, P, N = (int(v) for v in sets)
    scale, tau = contrastive
    if min(T, A, P, N) < 1 or not float(tau) > 0.0:
        raise ValueError(f"sets=(T, A, P, N) all >= 1 and contrastive=(scale, temperature > 0) expected, got {sets!r}, {contrastive!r}")
    return (T, A, P, N), float(scale), float(tau)


def _contrastive_operands(contrastive, robust):
    """(weight, tau) of a `contrastive=(weight, tau)` argument"""
    if robust is not None:
        raise ops.DbmmUnsupported("contrastive= and robust= do not combine: the group-DRO head has no contrastive form")
    weight, tau = contrastive
    if not 0.0 <= float(weight) <= 1.0 or not float(tau) > 0.0:
        raise ValueError(f"contrastive=(weight in [0, 1], temperature > 0) expected, got {contrastive!r}")
    return float(weight), float(tau)


def _step_key(new_ad, old_ad, optimizer):
    """every device address the fused step's argument block holds (15 of the trainable adapter incl. its six momentum buffers, 9 of the
    frozen one), or None while a momentum buffer does not exist yet"""
    key = []
    state = optimizer.state
    for ad, trainable in ((new_ad, True), (old_ad, False)):
        if ad is None:
            continue
        mods = ad.layers._modules
        l0, bn, l3 = mods["0"], mods["1"], mods["3"]
        ps = (l0._parameters["weight"], l0._parameters["bias"], bn._parameters["weight"], bn._parameters["bias"],
              l3._parameters["weight"], l3._parameters["bias"])
        bufs = bn._buffers
        key += [p.data_ptr() for p in ps]
        key += [bufs["running_mean"].data_ptr(), bufs["running_var"].data_ptr(), bufs["num_batches_tracked"].data_ptr()]
        if trainable:
            for p in ps:
                mb = state[p].get("momentum_buffer") if p in state else None
                if mb is None:
                    return None
                key.append(mb.data_ptr())
    key.append(id(optimizer))
    return tuple(key)


_text_cache = {}


def get_text_embedding(text_embedding_dir):
    """JSON {prompt: [D floats]} -> [D, C] (final_main.py:414-424; insertion order = columns).
    Parsed once per (path, mtime): the reference re-reads the group file every forward
    (final_main.py:72,131), which changes nothing numerically."""
    st = os.stat(text_embedding_dir)
    key = (os.path.abspath(text_embedding_dir), st.st_mtime_ns, st.st_size)
    if key not in _text_cache:
        with open(text_embedding_dir, "r") as f:
            d = json.load(f)
        _text_cache[key] = torch.stack([torch.tensor(v) for v in d.values()], dim=1)
    return _text_cache[key].clone()


class _TextBank:
    """device copies + column-normalised [C, D] forms of the prompt matrices."""
    def __init__(self):
        self._tn = {}

    def normalised(self, text):
        key = (text.data_ptr(), text._version, tuple(text.shape), str(text.device))
        tn = self._tn.get(key)
        if tn is None:
            tn = ops.text_colnorm(text.contiguous().float())
            self._tn = {key: tn} if len(self._tn) > 8 else {**self._tn, key: tn}
        return tn


class CustomCLIP(nn.Module):
    """final_main.py:53-92."""
    def __init__(self, adapter, text_embedding_dir, text_spurious_embedding_dir, text_group_embedding_dir,
                 temperature=0.01):
        super().__init__()
        self.text_embedding_dir = text_embedding_dir
        self.text_spurious_embedding_dir = text_spurious_embedding_dir
        self.text_group_embedding_dir = text_group_embedding_dir
        self.adapter = adapter
        self.temperature = temperature
        self.text_features = get_text_embedding(text_embedding_dir)
        self.n_cls = self.text_features.shape[0]       # = D, kept for compatibility (final_main.py:63)
        self.text_spurious_features = get_text_embedding(text_spurious_embedding_dir)
        self._bank = _TextBank()
        self._group = None

    def _apply(self, fn, *a, **k):
        # the reference keeps the text matrices as plain attributes moved with .cuda() at
        # construction; here they follow the module
        self.text_features = fn(self.text_features)
        self.text_spurious_features = fn(self.text_spurious_features)
        self._group = None
        return super()._apply(fn, *a, **k)

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_step_plan":                    # raw device addresses of THIS module's tensors: the copy builds its own
                continue
            new.__dict__[k] = _TextBank() if k == "_bank" else copy.deepcopy(v, memo)
        return new

    def __getstate__(self):                          # torch.save(module) / pickle: same rule as __deepcopy__
        state = dict(self.__dict__)
        state.pop("_step_plan", None)
        state["_bank"] = None
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__["_bank"] = _TextBank()

    def _text(self, which, device):
        if which == "group":
            if self._group is None or self._group.device != device:
                self._group = get_text_embedding(self.text_group_embedding_dir).to(device)
            t = self._group
        elif which == "spurious":
            t = self.text_spurious_features
        else:
            t = self.text_features
        if t.device != device:
            t = t.to(device)
        return self._bank.normalised(t)

    def _features(self, features):
        return self.adapter(features), None

    def forward(self, features, use_group=False):
        z, z_old = self._features(features)
        tn = self._text("group" if use_group else "class", features.device)
        return _SimFn.apply(z, z_old, tn, self.temperature, getattr(self, "ebd_weight", 0.5))

    def forward_spurious(self, features):
        z, z_old = self._features(features)
        tn = self._text("spurious", features.device)
        return _SimFn.apply(z, z_old, tn, self.temperature, getattr(self, "ebd_weight", 0.5))

    def loss(self, features, labels, use_group=False, spurious=False, robust=None, contrastive=None, row_weights=None):
        """fused step body: returns (mean CE, logits, per-row CE); `spurious`: against the spurious-attribute prompts
        (forward_spurious + criterion, final_main.py:764-766).  `robust` = (GroupDRO state, group ids of the batch): the loss is the
        group-DRO robust loss and the state's q is updated in place.  `contrastive` = (weight, temperature): returns (mixed loss,
        logits, per-row CE, L_con) with mixed = (1 - weight) * mean CE + weight * L_con, L_con the supervised-contrastive loss of the
        trainable adapter's output under `labels`.  `row_weights` (float32 [B] on the device, taken as they
        are): the loss is (1 / B) sum_b w_b CE_b; logits and per-row CE are the unweighted ones, and a row
        of weight 0 still takes part in the train-mode BatchNorm statistics."""
        if row_weights is not None:
            row_weights = _row_weight_operands(row_weights, robust, contrastive)
            ops._row_weights("loss", row_weights, features.device, features.shape[0])
        if contrastive is not None:
            contrastive = _contrastive_operands(contrastive, robust)
        z, z_old = self._features(features)
        tn = self._text("spurious" if spurious else "group" if use_group else "class", features.device)
        if contrastive is not None:
            return _SimCESupConFn.apply(z, z_old, tn, self.temperature, getattr(self, "ebd_weight", 0.5), labels.contiguous(), *contrastive)
        if robust is not None:
            groups, q, eta = _robust_operands(robust, features.shape[0])
            return _SimCERobustFn.apply(z, z_old, tn, self.temperature, getattr(self, "ebd_weight", 0.5), labels, groups, q, eta)
        if row_weights is not None:
            return _SimCEWeightedFn.apply(z, z_old, tn, self.temperature, getattr(self, "ebd_weight", 0.5), labels.contiguous(), row_weights)
        return _SimCEFn.apply(z, z_old, tn, self.temperature, getattr(self, "ebd_weight", 0.5), labels)

    def _step_adapters(self):
        """(trainable adapter, frozen old adapter or None)"""
        return self.adapter, None

    def _plan(self, optimizer, what):
        """(the argument block of the one-call steps for this module and `optimizer`, whether this is the optimiser's first step)"""
        if not self.training:
            raise RuntimeError(f"{what} needs classifier.train()")
        new_ad, old_ad = self._step_adapters()
        plan = self.__dict__.get("_step_plan")
        first = False
        # The argument block of the C call holds 24 raw pointers.  It is rebuilt whenever ANY tensor it points at was replaced or
        # moved (a parameter / buffer / momentum buffer re-assigned, `.data` swapped, the old adapter reloaded, another optimiser):
        # the key is the tuple of every tensor's data_ptr(), read through the modules' own dicts (~4 us; the step is launch-bound).
        key = _step_key(new_ad, old_ad, optimizer)
        if plan is None or plan["key"] != key or key is None:
            def pack(ad):
                l0, bn, l3 = ad.layers[0], ad.layers[1], ad.layers[3]
                return (l0.weight, l0.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                        l3.weight, l3.bias)
            new = pack(new_ad)
            trainable = [new[0], new[1], new[2], new[3], new[7], new[8]]
            owned = {id(p) for g in optimizer.param_groups for p in g["params"]}
            if len(optimizer.param_groups) != 1 or any(id(p) not in owned for p in trainable):
                raise RuntimeError(f"{what}: the optimiser must hold the adapter's six tensors in one param group")
            first = any("momentum_buffer" not in optimizer.state[p] for p in trainable)
            bufs = []
            for p in trainable:
                st = optimizer.state[p]
                if "momentum_buffer" not in st or st["momentum_buffer"] is None:
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                bufs.append(st["momentum_buffer"])
            # plain integer addresses (no ctypes objects, no module / optimiser references): the plan never keeps anything alive
            # and never travels with the module (__deepcopy__ / __getstate__ drop it)
            plan = dict(key=_step_key(new_ad, old_ad, optimizer),
                        args=ops.adapter_step_args([t.data for t in new], bufs,
                                                   [t.data for t in pack(old_ad)] if old_ad is not None else None),
                        H=new[0].shape[0], with_old=old_ad is not None)
            self.__dict__["_step_plan"] = plan
        return plan, first

    def sets_loss(self, features, sets, contrastive):
        """The contrastive-adapter loss of one step (Zhang & Re 2022; the reference's train_one_epoch_cl, demo/visualizer_supcon.py:
        412-508, with its SupervisedContrastiveLoss) on the autograd path.  `features` [T * S, D]: T sets of S = A + P + N rows
        [anchor, extra anchors; positives; negatives], `sets` = (T, A, P, N), `contrastive` = (scale, temperature).  Returns (L, l_t):
        l_t = log sum_{P u N} exp(s_j) - mean_P s_p with s_j the cosine of the anchor's and row j's adapter outputs / temperature,
        L = scale * sum_t l_t; extra anchors take no loss.  No prompts and no CE take part.  Departures from the dead reference
        path: the step's T * S rows pass the adapter as ONE train-mode BatchNorm batch (the reference would
        have pushed [anchor; positives] and [anchor; negatives] through separately); no ca_pre_norm and no ca_head -- the adapter
        is fed raw embeddings, as in forward(); the max subtracted is over P u N, which gives the same value."""
        sets, scale, tau = _sets_operands(sets, contrastive)
        return _SetsFn.apply(self.adapter(features), sets, scale, tau)

    def sets_step(self, features, optimizer, sets, contrastive):
        """sets_loss(...), backward and the SGD-momentum update as ONE C call (dbmm_adapter_train_step_sets); the same bits as
        `sets_loss(...)[0].backward(); optimizer.step()`.  The adapter's fast shape only (hidden width 128, D % 128 == 0): other
        shapes raise ops.DbmmUnsupported.  Requires train mode.  Returns (L, l_t), on the device."""
        sets, scale, tau = _sets_operands(sets, contrastive)
        plan, first = self._plan(optimizer, "sets_step")
        group = optimizer.param_groups[0]
        with torch.no_grad():
            return ops.adapter_train_step_sets(features.detach().contiguous(), plan["args"], plan["H"], sets, scale, tau, group["lr"],
                                               group.get("momentum", 0.0), group.get("weight_decay", 0.0), first)

    def train_step(self, features, labels, optimizer, use_group=False, robust=None, contrastive=None, row_weights=None):
        """The whole step body of final_main.py:455-466 / :610-623 -- forward, mean CE, backward and
        the SGD-momentum update -- as ONE C call (~20 launches back to back, no autograd graph, no
        host round trip).  Uses the optimiser's lr / momentum / weight_decay and its
        `momentum_buffer` state, so it can be mixed freely with `loss.backward(); optimizer.step()`.
        Requires train mode.  Returns (mean CE, logits, per-row CE), all on the device.  `robust` = (GroupDRO state, group ids of
        the batch): the group-DRO step (two launches more) -- the state's q is updated in place, the returned loss is the robust
        loss.  `contrastive` = (weight, temperature): the step with the supervised-contrastive head (three launches more); returns
        (mixed loss, logits, per-row CE, L_con).  `row_weights` (float32 [B] on the device, taken as they are): the step minimises
        and returns (1 / B) sum_b w_b CE_b in ERM's launches; the bits of `loss(..., row_weights=)`, backward, `optimizer.step()`."""
        if row_weights is not None:
            row_weights = _row_weight_operands(row_weights, robust, contrastive)
            ops._row_weights("train_step", row_weights, features.device, features.shape[0])
        if contrastive is not None:
            contrastive = _contrastive_operands(contrastive, robust)
        plan, first = self._plan(optimizer, "train_step")
        group = optimizer.param_groups[0]
        tn = self._text("group" if use_group else "class", features.device)
        with torch.no_grad():
            return ops.adapter_train_step(
                features.detach().contiguous(), labels.contiguous(), plan["args"], plan["H"], plan["with_old"],
                getattr(self, "ebd_weight", 0.5), tn, self.temperature, group["lr"], group.get("momentum", 0.0),
                group.get("weight_decay", 0.0), first, robust=None if robust is None else _robust_operands(robust, features.shape[0]),
                contrastive=contrastive, row_weights=row_weights)


class MultipleAdapter(CustomCLIP):
    """final_main.py:97-158.  Quirks kept: the old adapter also runs in
    train mode under `.train()`, its feature is detached, the blend is not re-normalised."""
    def __init__(self, old_cls, new_adapter, init_near_identity=True, ebd_weight=0.5):
        nn.Module.__init__(self)
        self.old_cls = old_cls
        self.text_embedding_dir = old_cls.text_embedding_dir
        self.text_spurious_embedding_dir = old_cls.text_spurious_embedding_dir
        self.text_group_embedding_dir = old_cls.text_group_embedding_dir
        self.text_features = get_text_embedding(self.text_embedding_dir)
        self.n_cls = self.text_features.shape[0]
        self.text_spurious_features = get_text_embedding(self.text_spurious_embedding_dir)
        self.new_adapter = new_adapter
        self.ebd_weight = ebd_weight
        if init_near_identity:
            print("Initialize paramters of [New adapter] from [Old adapter]")
            self.new_adapter.load_state_dict(self.old_cls.adapter.state_dict())
        self.temperature = old_cls.temperature
        self._bank = _TextBank()
        self._group = None

    def _features(self, features):
        with torch.no_grad():
            z_old = self.old_cls.adapter(features)     # detached branch; BN stats still update in train mode
        return self.new_adapter(features), z_old

    def _step_adapters(self):
        return self.new_adapter, self.old_cls.adapter

    def sets_loss(self, features, sets, contrastive):
        raise ops.DbmmUnsupported("the contrastive adapter (sets_loss / sets_step) covers CustomCLIP; MultipleAdapter has no sets head")

    def sets_step(self, features, optimizer, sets, contrastive):
        raise ops.DbmmUnsupported("the contrastive adapter (sets_loss / sets_step) covers CustomCLIP; MultipleAdapter has no sets head")


# ---------------------------------------------------------------------------------------
# stacked adapters / linear probes of a seed sweep (trainer.train_sweep, csrc/adapter_sweep.hip, csrc/linear_sweep.hip)
# ---------------------------------------------------------------------------------------

def _adapter_tensors(ad):
    """the nine tensors of an Adapter in the order of the C ABI's stacked arrays"""
    l0, bn, l3 = ad.layers[0], ad.layers[1], ad.layers[3]
    return [l0.weight, l0.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, l3.weight, l3.bias]


_TRAINABLE = (0, 1, 2, 3, 7, 8)          # w1, b1, gamma, beta, w2, b2 among the nine


class SweepAdapters:
    """R adapters of one sweep group as stacked contiguous tensors: `new` -- the nine tensors of the trainable adapters
    (w1 [R, H, D], b1, gamma, beta, running_mean, running_var [R, H], num_batches_tracked int64 [R], w2 [R, D, H], b2 [R, D]) --,
    `mom` their six momentum buffers, optionally `old`, the nine tensors of the frozen old adapters of R MultipleAdapters, and the
    shared prompt matrices.  One `step` trains all replicas in the launches of one single-run step, `evaluate` scores them on the
    same rows; `replica(r)` gives replica r back as an ordinary CustomCLIP / MultipleAdapter (the reference's state-dict keys).
    A second stacked set holds each replica's best model: `snapshot(mask)` / `restore(mask)` copy the masked replicas to / from it
    (best-model selection and --continue_from_best); a replica's best model may be of either kind, whatever the others are."""

    def __init__(self, new, old, D, H, device, text_dirs, temperature=0.01, ebd_weight=0.5):
        self.new, self.old = new, old
        self.R, self.D, self.H, self.device = new[0].shape[0], D, H, torch.device(device)
        self.text_dirs, self.temperature, self.ebd_weight = tuple(text_dirs), temperature, ebd_weight
        self.mom = [torch.zeros_like(self.new[i]) for i in _TRAINABLE]
        self.first_step = True
        self.best_new = self.best_old = None
        self.best_has_old = [False] * self.R
        self.has_best = [False] * self.R
        self._args = {}
        self._tn = {}

    @classmethod
    def from_modules(cls, modules, device="cuda"):
        """from R CustomCLIP modules (stage 1) or R MultipleAdapter modules (old_cls.adapter frozen, new_adapter trained)"""
        multi = isinstance(modules[0], MultipleAdapter)
        if any(isinstance(m, MultipleAdapter) != multi for m in modules):
            raise ValueError("SweepAdapters.from_modules: all replicas must be of one kind")
        news = [m.new_adapter if multi else m.adapter for m in modules]
        olds = [m.old_cls.adapter for m in modules] if multi else None
        m0 = modules[0]
        D, H = _adapter_tensors(news[0])[0].shape[1], _adapter_tensors(news[0])[0].shape[0]
        return cls(cls._stack(news, device), cls._stack(olds, device) if olds else None, D, H, device,
                   (m0.text_embedding_dir, m0.text_spurious_embedding_dir, m0.text_group_embedding_dir), m0.temperature,
                   getattr(m0, "ebd_weight", 0.5))

    @staticmethod
    def _stack(adapters, device):
        per = [[t.detach() for t in _adapter_tensors(a)] for a in adapters]
        return [torch.stack([p[i] for p in per]).to(device).contiguous() for i in range(9)]

    # ---- the two stage switches of train_all_epochs -----------------------------------------------------------------
    def reset_optimizer(self):
        """a fresh optimiser over the trainable set (set_optimizer_reg): momentum starts over"""
        for m in self.mom:
            m.zero_()
        self.first_step = True

    def add_adapters(self, new_adapters, init_near_identity):
        """MultipleAdapter(classifier, new_adapter, init_near_identity) for every replica: the current adapters become the frozen
        old ones, `new_adapters` (R fresh Adapter modules) the trainable ones -- loaded with the old state dicts (parameters and
        BatchNorm buffers) when `init_near_identity`"""
        if self.old is not None:
            raise RuntimeError("SweepAdapters.add_adapters: the replicas already are MultipleAdapters")
        self.old = self.new
        self.new = [t.clone() for t in self.old] if init_near_identity else self._stack(new_adapters, self.device)
        self._args = {}
        self.reset_optimizer()

    # ---- best models ------------------------------------------------------------------------------------------------
    def snapshot(self, mask):
        """best[r] = deepcopy(model r) for the replicas with mask[r]"""
        rs = [r for r in range(self.R) if mask[r]]
        if not rs:
            return
        if self.best_new is None:
            self.best_new = [torch.zeros_like(t) for t in self.new]
        if self.old is not None and self.best_old is None:
            self.best_old = [torch.zeros_like(t) for t in self.old]
            self._args.pop("best", None)
        ix = torch.as_tensor(rs, device=self.device)
        for dst, src in zip(self.best_new, self.new):
            dst[ix] = src[ix]
        if self.old is not None:
            for dst, src in zip(self.best_old, self.old):
                dst[ix] = src[ix]
        for r in rs:
            self.has_best[r], self.best_has_old[r] = True, self.old is not None
        self._args.pop("best", None)

    def restore(self, mask):
        """model r = deepcopy(best[r]) for the replicas with mask[r] (--continue_from_best; only before add_adapters)"""
        rs = [r for r in range(self.R) if mask[r]]
        if any(not self.has_best[r] for r in rs):
            raise RuntimeError("SweepAdapters.restore: a replica has no best model yet")
        if any(self.best_has_old[r] for r in rs) or self.old is not None:
            raise RuntimeError("SweepAdapters.restore: only plain (stage-1) best models can be continued from")
        if rs:
            ix = torch.as_tensor(rs, device=self.device)
            for dst, src in zip(self.new, self.best_new):
                dst[ix] = src[ix]

    def subset(self, rs, best=False):
        """a SweepAdapters of (copies of) the replicas `rs`, of their best models when `best`; they must be of one kind"""
        new, old = (self.best_new, self.best_old) if best else (self.new, self.old)
        kinds = {self.best_has_old[r] for r in rs} if best else {self.old is not None}
        if len(kinds) != 1:
            raise ValueError("SweepAdapters.subset: replicas of both kinds")
        ix = torch.as_tensor(list(rs), device=self.device)
        return SweepAdapters([t[ix].contiguous() for t in new], [t[ix].contiguous() for t in old] if kinds.pop() else None, self.D, self.H,
                             self.device, self.text_dirs, self.temperature, self.ebd_weight)

    def replica(self, r, best=False):
        """replica r (its best model when `best`) as an ordinary module on the sweep's device, in eval mode"""
        new, old = (self.best_new, self.best_old) if best else (self.new, self.old)
        with_old = self.best_has_old[r] if best else self.old is not None
        if best and not self.has_best[r]:
            return None

        def build(stack):
            ad = Adapter(self.D, self.H)
            with torch.no_grad():
                for dst, src in zip(_adapter_tensors(ad), stack):
                    dst.copy_(src[r])
            return ad
        prev = torch.get_rng_state()                 # Adapter() draws its initial weights: the caller's random stream is left alone
        try:
            m = CustomCLIP(build(old if with_old else new), *self.text_dirs, temperature=self.temperature)
            if with_old:
                import contextlib, io
                with contextlib.redirect_stdout(io.StringIO()):
                    m = MultipleAdapter(m, build(new), init_near_identity=False, ebd_weight=self.ebd_weight)
        finally:
            torch.set_rng_state(prev)
        return m.to(self.device).eval()

    # ---- the two batched calls ----------------------------------------------------------------------------------------
    def text(self, which):
        """column-normalised [C, D] prompt matrix: "class", "spurious" or "group" """
        tn = self._tn.get(which)
        if tn is None:
            path = self.text_dirs[{"class": 0, "spurious": 1, "group": 2}[which]]
            tn = ops.text_colnorm(get_text_embedding(path).to(self.device).contiguous().float())
            self._tn[which] = tn
        return tn

    def _call_args(self, best=False):
        key = "best" if best else "cur"
        a = self._args.get(key)
        if a is None:
            if best:
                a = ops.adapter_sweep_args(self.R, self.D, self.H, self.best_new, None, self.best_old if self.best_has_old[0] else None)
            else:
                a = ops.adapter_sweep_args(self.R, self.D, self.H, self.new, self.mom, self.old)
            self._args[key] = a
        return a

    def step(self, table, idx, labels, groups, which, lrs, momentum, weight_decay, counts, loss_sum, counted=True, robust=None, row_weights=None):
        """one training step of every replica on rows idx[r] of `table` against the `which` prompts.  Returns (mean CE [R], logits
        [R, B, C], per-row CE [R, B]).  `robust`: a GroupDRO state with q [R, G] over the groups of `groups` -- the group-DRO step of
        every replica; q is updated in place and the robust losses take the means' place.  `row_weights` (float32 [N] / [1, N] shared,
        or [R, N], over the TABLE's rows): every replica's step under per-row loss weights; the counters stay unweighted"""
        if robust is not None and (not isinstance(robust, GroupDRO) or robust.q.dim() != 2):
            raise TypeError("SweepAdapters.step: robust must be a GroupDRO state built with replicas=R")
        if row_weights is not None:
            _row_weight_operands(row_weights, robust, None)
        out = ops.adapter_sweep_step(table, idx, labels, groups, self._call_args(), self.ebd_weight, self.text(which), self.temperature, lrs,
                                     momentum, weight_decay, self.first_step, counts, loss_sum, counted,
                                     robust=None if robust is None else (robust.q, robust.step_size), row_weights=row_weights)
        self.first_step = False
        return out

    def evaluate(self, table, idx, labels, groups, which, counts, loss_sum, row0=0, n=None, best=False):
        """eval-mode forward of every replica (of the best models when `best`: they must be of one kind) over the same rows"""
        if best and len({self.best_has_old[r] for r in range(self.R)}) != 1:
            raise ValueError("SweepAdapters.evaluate(best=True): best models of both kinds; evaluate subset()s")
        return ops.adapter_sweep_eval(table, idx, labels, groups, self._call_args(best), self.ebd_weight, self.text(which), self.temperature,
                                      counts, loss_sum, row0, n)


class SweepLinear:
    """R LinearClassifiers of one sweep group as stacked contiguous tensors: `w` [R, C, D], `b` [R, C], and their momentum buffers
    `mom_w`, `mom_b` (one SGD optimiser per replica for the whole run).  One `step` trains all replicas in the launch of one
    single-run step (csrc/linear_sweep.hip), `evaluate` scores them on the same rows; `replica(r)` gives replica r back as an
    ordinary LinearClassifier (the reference's state-dict keys fc.weight / fc.bias).  A second stacked pair holds each replica's
    best model: `snapshot(mask)` copies the masked replicas into it (best-model selection)."""

    def __init__(self, w, b, device):
        self.w, self.b = w, b
        self.R, self.C, self.D = w.shape
        self.device = torch.device(device)
        self.mom_w, self.mom_b = torch.zeros_like(w), torch.zeros_like(b)
        self.first_step = True
        self.best_w = self.best_b = None
        self.has_best = [False] * self.R

    @classmethod
    def from_modules(cls, modules, device="cuda"):
        """from R LinearClassifier modules of one shape"""
        if any(not isinstance(m, LinearClassifier) for m in modules):
            raise ValueError("SweepLinear.from_modules: LinearClassifier modules expected")
        if len({tuple(m.fc.weight.shape) for m in modules}) != 1:
            raise ValueError("SweepLinear.from_modules: all replicas must be of one shape")
        w = torch.stack([m.fc.weight.detach() for m in modules]).to(device).contiguous()
        b = torch.stack([m.fc.bias.detach() for m in modules]).to(device).contiguous()
        return cls(w, b, device)

    def snapshot(self, mask):
        """best[r] = deepcopy(model r) for the replicas with mask[r]"""
        rs = [r for r in range(self.R) if mask[r]]
        if not rs:
            return
        if self.best_w is None:
            self.best_w, self.best_b = torch.zeros_like(self.w), torch.zeros_like(self.b)
        ix = torch.as_tensor(rs, device=self.device)
        self.best_w[ix] = self.w[ix]
        self.best_b[ix] = self.b[ix]
        for r in rs:
            self.has_best[r] = True

    def replica(self, r, best=False):
        """replica r (its best model when `best`; None if it has none) as an ordinary module on the sweep's device, in eval mode"""
        if best and not self.has_best[r]:
            return None
        w, b = (self.best_w, self.best_b) if best else (self.w, self.b)
        prev = torch.get_rng_state()                 # nn.Linear draws its initial weights: the caller's random stream is left alone
        try:
            m = LinearClassifier(self.D, self.C)
        finally:
            torch.set_rng_state(prev)
        with torch.no_grad():
            m.fc.weight.copy_(w[r])
            m.fc.bias.copy_(b[r])
        return m.to(self.device).eval()

    def step(self, table, idx, labels, groups, lrs, momentum, weight_decay, counts, loss_sum, counted=True, row_weights=None):
        """one training step of every replica on rows idx[r] of `table`.  Returns (mean CE [R], logits [R, B, C], per-row CE [R, B]).
        `row_weights` (float32 [N] / [1, N] shared, or [R, N], over the TABLE's rows): the step under per-row loss weights"""
        out = ops.linear_sweep_step(table, idx, labels, groups, self.w, self.b, self.mom_w, self.mom_b, lrs, momentum, weight_decay,
                                    self.first_step, counts, loss_sum, counted, row_weights=row_weights)
        self.first_step = False
        return out

    def evaluate(self, table, idx, labels, groups, counts, loss_sum, row0=0, n=None, best=False):
        """eval forward of every replica (of the best models when `best`) over the same rows.  Returns (logits [R, B, C], per-row
        CE [R, B])"""
        if best and not all(self.has_best):
            raise ValueError("SweepLinear.evaluate(best=True): a replica has no best model yet")
        w, b = (self.best_w, self.best_b) if best else (self.w, self.b)
        return ops.linear_sweep_eval(table, idx, labels, groups, w, b, counts, loss_sum, row0, n)


# ---------------------------------------------------------------------------------------
# metrics (final_main.py:383-412, demo/util.py:18-46)
# ---------------------------------------------------------------------------------------

class AverageMeter(object):
    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def group_counts(logits, y, g, n_groups, counts=None):
    """device-side (n, correct) per group as int64 [G, 2]; accumulates into `counts`."""
    if counts is None:
        counts = torch.zeros((n_groups, 2), dtype=torch.int64, device=logits.device)
    return ops.group_count(logits.detach().contiguous().float(), y.contiguous(), g.to(logits.device).contiguous(), counts)


def update_dict(acc_groups, y, g, logits):
    """final_main.py:383-391 with the argmax / compare / per-group counting on the GPU and a
    single 64-byte D2H copy instead of 2 syncs per group."""
    counts = group_counts(logits, y, g, len(acc_groups)).cpu().numpy()
    for g_val in range(counts.shape[0]):
        n, corr = int(counts[g_val, 0]), int(counts[g_val, 1])
        if n:
            acc_groups[g_val].update(corr / n, n)


def get_y_p(g, n_places):
    return g // n_places, g % n_places


def get_results(acc_groups, get_yp_func):
    groups = acc_groups.keys()
    results = {f"acc_{get_yp_func(g)[0]}_{get_yp_func(g)[1]}": acc_groups[g].avg for g in groups}
    all_correct = sum(acc_groups[g].sum for g in groups)
    all_total = sum(acc_groups[g].count for g in groups)
    results.update({"mean_acc": all_correct / all_total})
    results.update({"worst_acc": min(results.values())})
    return results


def accuracy(output, target, batch_size=None):
    with torch.no_grad():
        return torch.sum(output.argmax(dim=1).eq(target)).item() / target.size(0)


def per_group_loss(loss_rows, g, n_groups=4):
    """mean CE per group (build-side addition) -> float32 [G] on device."""
    sums = torch.zeros((n_groups,), device=loss_rows.device, dtype=torch.float32)
    ops.group_loss_sum(loss_rows.contiguous(), g.contiguous(), sums)
    n = torch.bincount(g, minlength=n_groups).clamp_min(1).float()
    return sums / n


def group_index(y, confounder):
    """data/celeba_embeddings_reg.py:34-38: -1 -> 0 recode, group = 2*y + confounder (int64)."""
    y = np.array(y, dtype=np.int64).copy()
    c = np.array(confounder, dtype=np.int64).copy()
    y[y == -1] = 0
    c[c == -1] = 0
    return y, c, y * 2 + c


def balance_val_indices(group_array, n_groups, batch_size_reg):
    """Index generation of balance_val (final_main.py:346-379) on a plain group array; uses the
    global numpy RNG exactly like the reference so seeds reproduce its epochs."""
    g_idx = [np.where(group_array == g)[0] for g in range(n_groups)]
    min_g = np.min([len(g) for g in g_idx])
    for i, g in enumerate(g_idx):
        np.random.shuffle(g)
        g_idx[i] = g[:min_g]
    balanced = np.array(list(zip(*g_idx))).reshape(-1)
    return balanced, (batch_size_reg if batch_size_reg <= len(balanced) else len(balanced))


def stratified_split_indices(group_array, test_size=0.5):
    """Index arrays of stratified_split_dataset (data/celeba_embeddings_reg.py:95-102): the
    reference delegates to sklearn's train_test_split with random_state=42 stratified on the group
    array, and so does this (same dependency, same RNG stream -> identical indices)."""
    from sklearn.model_selection import train_test_split
    group_array = np.asarray(group_array)
    reg_idx, val_idx = train_test_split(np.arange(len(group_array)), test_size=test_size, random_state=42,
                                        stratify=group_array)
    return reg_idx, val_idx


def stratified_split_dataset(dataset, test_size=0.5):
    """data/celeba_embeddings_reg.py:95-107: two torch Subsets (reg, val) of a dataset that carries
    `.group_array`."""
    reg_idx, val_idx = stratified_split_indices(dataset.group_array, test_size)
    return torch.utils.data.Subset(dataset, reg_idx), torch.utils.data.Subset(dataset, val_idx)


def minority_flags(dataset, target, target_s, pred):
    """clip_inference.py:219-233."""
    if dataset == "waterbirds":
        is_minor_pred = (((target == 0) & (pred == 1)) | ((target == 1) & (pred == 0))).long()
        is_minor = (((target == 0) & (target_s == 1)) | ((target == 1) & (target_s == 0))).long()
    elif dataset == "celeba":
        is_minor_pred = ((target == 1) & (pred == 1)).long()
        is_minor = ((target == 1) & (target_s == 1)).long()
    else:
        raise NotImplementedError(dataset)
    return is_minor, is_minor_pred


def zeroshot_tail(image_features, zeroshot_weights, temperature=0.02):
    """clip_inference.py:207-216 fused: normalise rows, @ W / T, argmax (softmax is monotone,
    so `pred` equals torch.max(probs)); returns logits and int64 pred.  The input is left
    un-normalised like the `--normalized`-off branch that saves raw embeddings."""
    f = image_features.float().contiguous()
    W = zeroshot_weights.float().contiguous()
    tn = W.t().contiguous()                      # zero-shot weights are used as given (not re-normalised)
    logits, _, _, pred, _ = ops.l2norm_sim_ce_fwd(f, tn, temperature, want_pred=True)
    return logits, pred
