"""What the wrappers of ``msod_amd.ops`` hand to the library, on a machine without a GPU: the table of tests/ops_contract.py run with
CPU tensors against a stub library that records the call and raises instead of launching.

Every refused case must raise its declared exception before the stub is entered; every accepted view must reach the wrapper's entry
point with 16-byte aligned tensor pointers and the scalars of the dense call (but for the strides of the operand that was replaced).
"""
import ctypes
import re

import pytest
import torch

import ops_contract as T


@pytest.fixture
def stub(monkeypatch):
    return T.install_stub(monkeypatch, host=True)


def _ops():
    import msod_amd  # noqa: F401
    from msod_amd import ops
    return ops


def _parameters():
    """{entry point: [parameter names]} from include/cft_hip.h (``_lib.SIGNATURES`` keeps the types only)."""
    from msod_amd import _lib
    with open(_lib.HEADER) as fh:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", fh.read(), flags=re.S)
    names = {}
    for name, args in re.findall(r"\b(cft_\w+)\s*\(([^()]*)\)\s*;", text):
        names[name] = [re.findall(r"\w+", a)[-1] for a in args.split(",") if a.strip() not in ("", "void")]
    return names


def _reach(e, ops, stub, o):
    """(entry point, args) of the call that ended in the stub."""
    del stub.calls[:]
    try:
        e.call(ops, o)
    except T.Reached:
        return stub.calls[-1]
    if stub.calls and stub.calls[-1][0] == e.entry_point:      # (a wrapper whose own entry point is one of the stub's silent helpers)
        return stub.calls[-1]
    raise AssertionError("the call returned without entering the library")


def test_every_public_wrapper_is_in_the_table():
    ops = _ops()
    covered = {e.wrapper for e in T.TABLE}
    assert set(T.WRAPPERS) <= covered, sorted(set(T.WRAPPERS) - covered)
    for w in covered:
        assert callable(getattr(ops, w))
    assert len({e.name for e in T.TABLE}) == len(T.TABLE)


def test_parameter_names_match_the_signatures():
    from msod_amd import _lib
    names = _parameters()
    for fn, (_, argtypes) in _lib.SIGNATURES.items():
        assert len(names[fn]) == len(argtypes), fn
    every = {p for ps in names.values() for p in ps}
    for e in T.TABLE:
        for a in e.args.values():
            assert set(a.ld) <= every, (e.name, a.ld)


@pytest.mark.parametrize("e,dtype", T.CASES, ids=T.CASE_IDS)
def test_accepted_views_reach_the_library(e, dtype, stub):
    from msod_amd import _lib
    ops = _ops()
    o = e.build(ops, dtype, "cpu")
    name0, args0 = _reach(e, ops, stub, o)
    assert name0 == e.entry_point
    params, argtypes = _parameters()[name0], _lib.SIGNATURES[name0][1]
    failures = []
    cases = T.accepted_cases(e, ops, dtype, o)
    assert cases or not any(a.accepted() for a in e.args.values())
    for cid, over, _ in [("dense", {}, [])] + cases:
        over = dict(over)
        ref = args0
        try:
            if "__dense__" in over:
                ref = _reach(e, ops, stub, dict(o, **over.pop("__dense__")))[1]
            name, args = _reach(e, ops, stub, dict(o, **over))
        except Exception as ex:          # noqa: BLE001 - the case is reported with the others
            failures.append(f"{cid}: {type(ex).__name__}: {ex}")
            continue
        free = {p for k in over if k in e.args for p in e.args[k].ld}
        if name != name0:
            failures.append(f"{cid}: ended in {name}, the dense call in {name0}")
            continue
        for p, ty, a, a0 in zip(params, argtypes, args, ref):
            if ty is ctypes.c_void_p:
                if (a is None) != (a0 is None) or (a is not None and a % 16 and p not in T.ANY_ALIGNMENT.get(name, ())):
                    failures.append(f"{cid}: pointer {p} = {a} (dense call: {a0}) is not 16-byte aligned")
            elif a != a0 and p not in free:
                failures.append(f"{cid}: {p} = {a}, the dense call passes {a0}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("e,dtype", T.CASES, ids=T.CASE_IDS)
def test_refused_cases_raise_before_the_library(e, dtype, stub):
    ops = _ops()
    o = e.build(ops, dtype, "cpu")
    failures = []
    for cid, over, exc in T.refused_cases(e, ops, dtype, o):
        before = {k: v.clone() for k, v in T.tensors_of(o).items() if v.device.type != "meta"}
        del stub.calls[:]
        try:
            e.call(ops, dict(o, **over))
            failures.append(f"{cid}: returned")
        except T.Reached as r:
            failures.append(f"{cid}: reached {r}")
        except Exception as ex:          # noqa: BLE001
            if type(ex) is not exc:
                failures.append(f"{cid}: {type(ex).__name__} ({ex}), expected {exc.__name__}")
            elif stub.calls:
                failures.append(f"{cid}: raised after entering {stub.calls[0][0]}")
        assert all(torch.equal(v, before[k]) for k, v in T.tensors_of(o).items() if k in before), cid
    assert not failures, "\n".join(failures)
