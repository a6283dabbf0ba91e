"""The table of tests/ops_contract.py on the GPU.

Accepted views: the wrapper on every view family against the same wrapper on dense operands - ``torch.equal``, no tolerance (the dense
path is held per element by tests/test_gpu_kernel_oracles.py; a view changes addresses, not arithmetic) - with every byte of the
enclosing buffers outside the destination view and every input unchanged.

Refused cases run under the stub library of ops_contract (nothing is ever forwarded to the real one): the declared exception, nothing
entered, the outputs still holding their fill.
"""
import pytest
import torch

import ops_contract as T

pytestmark = pytest.mark.gpu


def _ops():
    from msod_amd import ops
    return ops


def _run(e, ops, o):
    """{name: tensor} of everything the call produced: what it returned and the operands it writes."""
    ret = e.call(ops, o)
    ret = ret if isinstance(ret, (tuple, list)) else (ret,)
    got = {f"ret{i}": r for i, r in enumerate(ret) if isinstance(r, torch.Tensor)}
    got.update({k: o[k] for k, a in e.args.items() if a.role in ("out", "inout")})
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in got.items()}


def _fresh(e, o0):
    """The pristine operands with private copies of what a call updates in place."""
    return {k: (v.clone() if k in e.args and e.args[k].role == "inout" and k not in e.aliases else v) for k, v in o0.items()}


@pytest.mark.parametrize("e,dtype", T.CASES, ids=T.CASE_IDS)
def test_accepted_views_are_bit_identical_to_the_dense_call(dev, e, dtype):
    ops = _ops()
    o0 = e.build(ops, dtype, dev)
    cases = T.accepted_cases(e, ops, dtype, o0)
    dense = _run(e, ops, _alias(e, _fresh(e, o0)))
    failures = []
    for cid, over, bufs in cases:
        over = dict(over)
        ref = dense
        if "__dense__" in over:
            ref = _run(e, ops, dict(_fresh(e, o0), **over.pop("__dense__")))
        o = _alias(e, dict(_fresh(e, o0), **over), over)
        written = [o[k] for k, a in e.args.items() if a.role in ("out", "inout")]
        inputs = {k: v for k, v in T.tensors_of(o).items() if not any(v is w for w in written)}       # (an operand that IS the output is no input)
        before = {k: v.clone() for k, v in inputs.items()}
        bufs_before = [b.clone() for b, _ in bufs]
        got = _run(e, ops, o)
        for k in ref:
            if got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype or not torch.equal(got[k], ref[k]):
                failures.append(f"{cid}: {k} differs from the dense call ({(got[k].double() - ref[k].double()).abs().max().item():.3e})")
        for (b, m), b0 in zip(bufs, bufs_before):
            if not torch.equal(b[~m], b0[~m]):
                failures.append(f"{cid}: {int((b[~m] != b0[~m]).sum())} elements outside the view were written")
        for k, v in inputs.items():
            if not torch.equal(v, before[k]):
                failures.append(f"{cid}: input {k} was changed")
    assert not failures, "\n".join(failures)


def _alias(e, o, over=()):
    """Operands that ARE another operand in the dense call (the in-place residual stream) follow it, unless the case replaced them."""
    for k, tgt in e.aliases.items():
        if k not in over:
            o[k] = o[tgt]
    return o


@pytest.mark.parametrize("e,dtype", T.CASES, ids=T.CASE_IDS)
def test_refused_cases_raise_with_nothing_entered(dev, e, dtype, monkeypatch):
    ops = _ops()
    stub = T.install_stub(monkeypatch, host=False)          # from here on nothing reaches the real library
    o0 = e.build(ops, dtype, dev)
    primary = next(iter(e.args))
    cases = T.refused_cases(e, ops, dtype, o0) + [(f"{primary}:on-the-host", {primary: o0[primary].cpu()}, RuntimeError)]
    failures = []
    for cid, over, exc in cases:
        o = dict(o0, **over)
        held = {k: v for k, v in T.tensors_of(o).items() if v.device.type != "meta"}
        before = {k: v.clone() for k, v in held.items()}
        del stub.calls[:]
        try:
            e.call(ops, o)
            failures.append(f"{cid}: returned")
        except T.Reached as r:
            failures.append(f"{cid}: reached {r}")
        except Exception as ex:          # noqa: BLE001 - reported with the others
            if type(ex) is not exc:
                failures.append(f"{cid}: {type(ex).__name__} ({ex}), expected {exc.__name__}")
            elif stub.calls:
                failures.append(f"{cid}: raised after entering {stub.calls[0][0]}")
        for k, v in held.items():
            if not torch.equal(v, before[k]):
                failures.append(f"{cid}: {k} no longer holds its fill")
    assert not failures, "\n".join(failures)
