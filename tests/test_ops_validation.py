"""The C ABI sees raw pointers, sizes and leading dimensions; the Python wrappers therefore refuse operands that do not hold what the
kernels will index, before anything is launched (CPU tensors are refused earlier still).  These checks run without a GPU and without the
built library: tests/ops_audit.py puts a recording stub in the library's place, so a bad operand that reaches a C entry is seen as a
recorded call, not as a read past an allocation.  Only the last test hands anything to the real library, and only the valid calls."""
import glob
import os

import pytest
import torch

import ops_audit as A
from dbmm_amd import _lib, ops

REFUSALS = (_lib.DbmmError, RuntimeError, TypeError, ValueError)
CASE_IDS = [c.id for c in A.CASES]


def test_wrappers_refuse_cpu_tensors_before_any_launch():
    with pytest.raises(Exception):
        ops.gemm(torch.zeros(4, 8), torch.zeros(4, 8))
    with pytest.raises(Exception):
        ops.attnpool(torch.zeros(1, 2, 2, 64), torch.zeros(5, 64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(128, 64), torch.zeros(128),
                     torch.zeros(32, 64), torch.zeros(32), 1)


def test_sized_helper():
    ops._sized("bias", None, 5)
    ops._sized("bias", torch.zeros(5), 5)
    with pytest.raises(RuntimeError, match="bias"):
        ops._sized("bias", torch.zeros(4), 5)


def _run(case, monkeypatch, kwargs=None, unsupported=None, marked=False, refusals=REFUSALS):
    """one call under the stub: (result or the refusal it raised, recorded calls, audit findings)"""
    stub, reg = A.install(monkeypatch, unsupported)
    kwargs = case.kwargs if kwargs is None else kwargs
    reg.add_tree(kwargs)
    if marked:
        ops.mark_static(*[t for _, t in A.leaves(kwargs)])
    try:
        result = case.call(kwargs)
    except refusals as e:
        result = e
    reg.add_tree(result if not isinstance(result, Exception) else ())       # a converted operand the wrapper hands back (embed_gather's ids)
    return result, stub.calls, A.audit(stub, reg)


def _check_outputs(case, result):
    outs = [o for o in (result if isinstance(result, (tuple, list)) else (result,)) if o is None or isinstance(o, torch.Tensor)]
    assert len(outs) == len(case.outs), f"{case.id}: {len(outs)} tensors returned, {len(case.outs)} documented"
    for got, want in zip(outs, case.outs):
        if want is None:
            assert got is None
        else:
            assert got is not None and (tuple(got.shape), got.dtype) == want, f"{case.id}: returned {tuple(got.shape)} {got.dtype}, documented {want}"
    return outs


@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_valid_call_passes_the_audit(case, monkeypatch):
    result, calls, found = _run(case, monkeypatch)
    assert not isinstance(result, Exception), f"{case.id} was refused: {result}"
    assert calls, f"{case.id} reached no C entry"
    assert not found, "\n".join(found)
    _check_outputs(case, result)


@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_valid_call_passes_the_audit_on_the_fall_through_path(case, monkeypatch):
    """the fused entries answer DBMM_E_UNSUPPORTED: the wrapper answers None or composes the unfused entries, whose operands are audited too"""
    result, calls, found = _run(case, monkeypatch, unsupported=A.fused_unsupported)
    assert not isinstance(result, Exception), f"{case.id} was refused: {result}"
    assert calls and not found, "\n".join(found)
    if result is None:
        assert case.may_be_none
    else:
        _check_outputs(case, result)


def mutation_failures(case, monkeypatch, marked=False):
    """(wrapper, operand, mutation, what happened) of every generated bad call that was not refused before a C entry was reached.
    marked: every tensor of the bad call was first handed to ops.mark_static, as a plan builder would"""
    failed = []
    for path, name, kwargs in A.mutations(case):
        operand = ".".join(str(p) for p in path)
        with monkeypatch.context() as m:
            try:
                # (None for an operand the wrapper reads itself: Python's own AttributeError is a refusal too, if nothing was launched)
                result, calls, found = _run(case, m, kwargs, marked=marked, refusals=REFUSALS + ((AttributeError,) if name == "none" else ()))
            except Exception as e:                                     # not one of the documented refusals
                failed.append((case.fn, operand, name, f"raised {type(e).__name__}: {e}"))
                continue
        served = (path, name) in case.free or (path[0] in case.converted and name in ("width", "noncontig"))
        if name == "none" and calls:                                   # the entry must take NULL there: the audit's NULL check says
            if found:
                failed.append((case.fn, operand, name, f"{found}"))
        elif served:                                                     # another valid call: it must be one, all the way down
            if isinstance(result, Exception) or found:
                failed.append((case.fn, operand, name, f"a valid call, but: {result if isinstance(result, Exception) else found}"))
        elif calls:
            failed.append((case.fn, operand, name, "reached " + ", ".join(c[0] for c in calls)))
        elif not isinstance(result, Exception) and result is not None:
            failed.append((case.fn, operand, name, "answered without a launch and without a refusal"))
    return failed


@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_mutated_operands_are_refused_before_any_launch(case, monkeypatch):
    """every tensor operand of every valid call, plan dicts and tuples included: one element short, one row short (2-D), the other width of
    its kind, a non-contiguous view of the right shape, on another device, and empty for the *_absmax scalars.  The wrapper raises (or
    answers None where that is its answer to the condition) and no C entry is reached."""
    failed = mutation_failures(case, monkeypatch)
    assert not failed, "\n".join(" | ".join(f) for f in failed)


@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_static_marks_let_nothing_through(case, monkeypatch):
    """ops.mark_static records what a plan's tensors are so that a launch need not ask again: a valid call whose operands are all marked
    passes the audit, and a marked operand that does not hold what the call implies is refused like an unmarked one"""
    monkeypatch.setattr(ops, "_static", {})
    result, calls, found = _run(case, monkeypatch, marked=True)
    assert not isinstance(result, Exception) and calls and not found, f"{case.id}: {result} {found}"
    failed = mutation_failures(case, monkeypatch, marked=True)
    assert not failed, "\n".join(" | ".join(f) for f in failed)


def test_every_operand_is_mutated():
    """the generator is not vacuous: each tensor operand of each case gets the element-short (or, for a scalar, empty), width and device
    mutations at least"""
    for case in A.CASES:
        got = {}
        for path, name, _ in A.mutations(case):
            got.setdefault(path, set()).add(name)
        assert set(got) == {p for p, _ in A.leaves(case.kwargs)}
        for path, names in got.items():
            assert "meta" in names and ("short1" in names or "empty" in names), (case.id, path, names)


# ---- closure and self-check ----------------------------------------------------------------------------------------------------------

def test_every_export_is_audited_launchless_or_listed():
    assert set(_lib.EXPORTS) == A.AUDITED | A.LAUNCHLESS | A.NO_WRAPPER | A.NOT_AUDITED_YET
    assert all(n.startswith(A.NOT_AUDITED_FAMILIES) for n in A.NOT_AUDITED_YET)
    for a, b in ((A.AUDITED, A.LAUNCHLESS), (A.AUDITED, A.NO_WRAPPER), (A.AUDITED, A.NOT_AUDITED_YET), (A.NO_WRAPPER, A.NOT_AUDITED_YET),
                 (A.LAUNCHLESS, A.NO_WRAPPER), (A.LAUNCHLESS, A.NOT_AUDITED_YET)):
        assert not a & b
    # NO_WRAPPER means it: no module of the package names these entries
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    text = "".join(open(p).read() for p in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True) if not p.endswith("_lib.py"))
    for name in A.NO_WRAPPER:
        assert name + "(" not in text, f"{name} has a wrapper now: audit it"


def test_every_audited_entry_is_reached_by_a_valid_call(monkeypatch):
    reached = set()
    for unsupported in (None, A.fused_unsupported):
        for case in A.CASES:
            with monkeypatch.context() as m:
                reached |= {c[0] for c in _run(case, m, unsupported=unsupported)[1]}
    assert reached == A.AUDITED


def test_every_pointer_argument_has_a_spec_cell():
    for entry, (names, _, cells) in A.SPEC.items():
        names = names.split()
        assert len(names) == len(_lib._SIGS[entry]), entry
        for i in A.pointer_positions(entry):
            assert names[i] in cells or names[i] in ("stream", "workspace"), f"{entry}: argument {i} ({names[i]}) has no spec cell"
        assert names[-1] == "stream" and set(cells) <= set(names), entry
        if "workspace" in names:
            assert names[names.index("workspace") + 1] == "workspace_bytes" and _lib._SIGS[entry][names.index("workspace") + 1] is _lib._Z


def test_the_audit_sees_a_wrong_wrapper(monkeypatch):
    """a wrapper that checks nothing: one tensor an element short, then an fp16 tensor for an fp32 argument -- the audit reports both"""
    stub, reg = A.install(monkeypatch)

    def careless_l2norm_rows(x, B, D):
        y = ops._empty((B, D), dtype=torch.float32)
        _lib.lib().dbmm_l2norm_rows(ops.ptr(x), ops.ptr(y), B, D, ops.stream())

    good, short, half = torch.zeros(4 * 64), torch.zeros(4 * 64 - 1), torch.zeros(4 * 64, dtype=torch.float16)
    for t in (good, short, half):
        reg.add(t)
    careless_l2norm_rows(good, 4, 64)
    assert A.audit(stub, reg) == []
    careless_l2norm_rows(short, 4, 64)
    careless_l2norm_rows(half, 4, 64)
    found = A.audit(stub, reg)
    assert len(found) == 2 and "255 elements where the entry indexes 256" in found[0] and "torch.float16 where the entry reads torch.float32" in found[1]
    careless_l2norm_rows(torch.empty(4, 64, device="meta"), 4, 64)          # another device: a pointer the registry does not know
    assert "no tensor on the device" in A.audit(stub, reg)[2]


# ---- the valid calls against the real library -----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", A.CASES, ids=CASE_IDS)
def test_valid_calls_are_valid_for_the_real_library(case):
    """ties the spec table's idea of a valid call to the real ABI: no refusal, the documented shapes and dtypes, finite values"""
    result = case.call(A.mapped(case.kwargs, lambda t: t.cuda()))
    torch.cuda.synchronize()
    assert result is not None, f"{case.id}: the library has no kernel for a shape the matrix calls served"
    for out in _check_outputs(case, result):
        if out is not None:
            assert out.is_cuda and torch.isfinite(out.float()).all(), case.id
