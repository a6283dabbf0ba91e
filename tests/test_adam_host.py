"""CPU tests of the Adam / AdamW half of msod_amd.utils.optim: the float64 oracle and bound of tests/adam_ref.py against
torch.optim.Adam / AdamW, the wrong forms the bound must catch, the ABI of cft_adam_step, the Python-side validation, the state-dict
layout shared with torch, and the reference's groups and warm-up under ``--adam``."""
import copy
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import adam_ref as A
import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "optim")
N = 20001                      # the grid below on 200 001 elements gives the same worst ratios to two digits; this runs in 2 s


@pytest.fixture(scope="module")
def mods():
    import msod_amd  # noqa: F401
    from msod_amd.utils import general, optim
    return optim, general


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLDEN, "adam_cases.pt"), weights_only=False)["adam"]


def test_oracle_reproduces_torch_adam_and_adamw():
    worst = [0.0, 0.0, 0.0]
    for (cls, decoupled), wd, beta1, lr, eps in itertools.product(((torch.optim.Adam, False), (torch.optim.AdamW, True)), (0.0, 5e-4, 1e-2),
                                                                  (0.937, 0.9, 0.0), (1e-2, 1e-3), (1e-8, 1e-3)):
        rng = np.random.default_rng(7)
        p = nn.Parameter(A.log_uniform(rng, N, -4, 3))                         # seven decades
        opt = cls([p], lr=lr, betas=(beta1, 0.999), eps=eps, weight_decay=wd, foreach=False)
        m = v = None
        for k in range(5):
            g = A.step_grads(rng, N, k)
            assert bool(((g == 0) | (g.abs() >= 1e-12)).all())
            p0, p.grad = p.detach().clone(), g
            opt.step()
            p1, m1, v1, bp, bm, bv = A.adam_step(p0, g, m, v, k + 1, lr, beta1, 0.999, eps, wd, decoupled)
            m, v = opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()
            w = (A.worst(p.detach(), p1, bp), A.worst(m, m1, bm), A.worst(v, v1, bv))
            assert max(w) <= 1.0, (cls.__name__, wd, beta1, lr, eps, k, w)
            worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"torch CPU against float64, worst |err| / bound: params {worst[0]:.3f}, exp_avg {worst[1]:.3f}, exp_avg_sq {worst[2]:.3f}")


def _wrong(form, p, g, m, v, step, lr, beta1, beta2, eps, wd):
    """Float64 Adam (L2) with one deliberate mistake."""
    p, g, m, v = (x.numpy().astype(np.float64) for x in (p, g, m, v))
    if form == "beta1 for beta2":
        beta2 = beta1
    p0, g1 = (p * (1 - lr * wd), g) if form == "decoupled decay" else (p, g + wd * p)
    m1 = m + (1 - beta1) * (g1 - m)
    v1 = beta2 * v + (1 - beta2) * g1 * g1
    bc1, bc2 = (1.0, 1.0) if form == "no bias correction" else (1 - beta1 ** step, 1 - beta2 ** step)
    den = np.sqrt(v1 + eps) / math.sqrt(bc2) if form == "eps inside the root" else np.sqrt(v1) / math.sqrt(bc2) + eps
    return p0 - lr / bc1 * m1 / den


def test_oracle_bound_catches_wrong_forms():
    rng = np.random.default_rng(7)
    p, m = A.log_uniform(rng, N, -4, 3), A.log_uniform(rng, N, -6, 1)
    v = A.log_uniform(rng, N, -6, 1).abs() ** 2
    g = A.step_grads(rng, N, 0)
    args = (3, 1e-2, 0.937, 0.999, 1e-8, 5e-4)
    p1, _, _, bp, _, _ = A.adam_step(p, g, m, v, *args, False)
    assert A.worst(torch.from_numpy(_wrong(None, p, g, m, v, *args).astype(np.float32)), p1, bp) <= 1.0      # the right form, rounded once
    for form in ("decoupled decay", "no bias correction", "eps inside the root", "beta1 for beta2"):
        w = A.worst(torch.from_numpy(_wrong(form, p, g, m, v, *args).astype(np.float32)), p1, bp)
        print(f"{form}: {w:.3g} times the bound")
        assert w > 10, form


def test_header_declares_cft_adam_step():
    import ctypes as c
    import msod_amd  # noqa: F401
    from msod_amd import _lib
    with open(_lib.HEADER) as fh:
        sig, consts = _lib.parse_header(fh.read())
    p, i, l = c.c_void_p, c.c_int, c.c_long
    assert sig["cft_adam_step"] == (i, [p, p, i, l, i, i, p, i, p, p, p, p])
    assert consts["CFT_ADAM_SEG_BYTES"] == 56 and consts["CFT_ABI_VERSION"] == 19
    with open(os.path.join(_lib.CSRC, "runtime.hip")) as fh:
        assert "cft_adam_step" in fh.read()


def test_errors_are_raised_before_any_device_work(mods):
    optim = mods[0]
    w = nn.Parameter(torch.zeros(4))
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(ValueError, match="amsgrad"):
            cls([w], amsgrad=True)
        with pytest.raises(ValueError, match="maximize"):
            cls([w], maximize=True)
        for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, -0.5)):
            with pytest.raises(ValueError, match="beta"):
                cls([w], betas=betas)
        for kw in ({"lr": -1.0}, {"eps": -1e-8}, {"weight_decay": -0.1}):
            with pytest.raises(ValueError, match="Invalid"):
                cls([w], **kw)
    opt = optim.Adam([w], lr=0.1)
    assert opt.step() is None and opt.table_uploads == 0 and len(opt.state) == 0       # no gradient anywhere: nothing to do, as in torch
    for dtype in (torch.float64, torch.float16):
        q = nn.Parameter(torch.zeros(4, dtype=dtype))
        q.grad = torch.zeros(4, dtype=dtype)
        with pytest.raises(ValueError, match="float32"):
            optim.Adam([q]).step()
    s = nn.Parameter(torch.zeros(4, 6)[:, ::2])                         # a view with gaps
    s.grad = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="dense"):
        optim.Adam([s]).step()
    t = nn.Parameter(torch.zeros(3, 4).t())                             # dense, but its gradient is laid out otherwise
    t.grad = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="layout"):
        optim.Adam([t]).step()
    w.grad = torch.zeros(4)
    with pytest.raises(ValueError, match=r"GPU only \(torch.optim.Adam works"):     # right tensors, wrong device: still no kernel for it
        opt.step()
    with pytest.raises(ValueError, match=r"torch.optim.AdamW works"):
        optim.AdamW([w]).step()
    for key, value, match in (("amsgrad", True, "amsgrad"), ("maximize", True, "maximize"), ("betas", (0.9, 1.5), "beta"),
                              ("lr", -0.1, "learning rate"), ("eps", -1.0, "epsilon"), ("weight_decay", -1.0, "weight_decay")):
        edited = optim.Adam([w], lr=0.1)
        edited.param_groups[0][key] = value                             # groups edited after construction are checked in step()
        with pytest.raises(ValueError, match=match):
            edited.step()
    with pytest.raises(ValueError, match="at most 8"):
        many = optim.Adam([nn.Parameter(torch.zeros(1))], lr=0.1)
        for _ in range(8):
            many.add_param_group({"params": [nn.Parameter(torch.zeros(1))]})


def _torch_adam(net, hyp, cls=torch.optim.Adam):
    pg0, pg1, pg2 = [], [], []
    for m in net.modules():
        if isinstance(getattr(m, "bias", None), nn.Parameter):
            pg2.append(m.bias)
        if isinstance(m, nn.BatchNorm2d):
            pg0.append(m.weight)
        elif isinstance(getattr(m, "weight", None), nn.Parameter):
            pg1.append(m.weight)
    opt = cls(pg0, lr=hyp["lr0"], betas=(hyp["momentum"], 0.999), foreach=False)
    opt.add_param_group({"params": pg1, "weight_decay": hyp["weight_decay"]})
    opt.add_param_group({"params": pg2})
    return opt


def test_state_dict_round_trip_with_torch_adam(mods, golden):
    optim = mods[0]
    hyp = golden["hyp"]
    net = R.SmallNet()
    net.load_state_dict(R.seeded_state(net, 0))
    theirs = _torch_adam(net, hyp)
    for n, gr in R.seeded_grads(net, 0).items():
        net.get_parameter(n).grad = gr
    theirs.step()
    sd = copy.deepcopy(theirs.state_dict())
    assert all(v["step"].device.type == "cpu" for v in sd["state"].values())
    ours = optim.build_adam_optimizer(net, hyp)
    assert set(ours.param_groups[0]) == set(theirs.param_groups[0])                     # the same keys before any load
    assert {k: v for k, v in ours.defaults.items()} == {k: v for k, v in theirs.defaults.items()} | {"foreach": None}
    ours.load_state_dict(copy.deepcopy(sd))                                             # torch's -> ours
    for p in net.parameters():
        assert set(ours.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and float(ours.state[p]["step"]) == 1.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(ours.state[p][k], theirs.state[p][k])
    for a, b in zip(ours.param_groups, theirs.param_groups):
        assert set(a) == set(b)
        assert all(a[k] == b[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "decoupled_weight_decay"))
    back = copy.deepcopy(ours.state_dict())                                             # ours -> torch's
    assert set(back) == set(sd) and set(back["param_groups"][0]) == set(sd["param_groups"][0])
    assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in back["state"].values()) and set(back["state"]) == set(sd["state"])
    again = _torch_adam(net, hyp)
    again.load_state_dict(back)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    again.step()                                                         # and torch steps on from it
    want = {n: p.detach().clone() for n, p in net.named_parameters()}
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(before[n])
    theirs.step()
    for n, p in net.named_parameters():
        assert torch.equal(p, want[n]), n
        assert float(again.state[p]["step"]) == 2.0
    # a state dict of the reference's time: a Python int as step, none of the newer keys
    old = copy.deepcopy(sd)
    for st in old["state"].values():
        st["step"] = int(st["step"])
    for grp in old["param_groups"]:
        for k in ("maximize", "foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay"):
            grp.pop(k)
    ours.load_state_dict(old)
    assert all(x["maximize"] is False and x["decoupled_weight_decay"] is False and x["capturable"] is False for x in ours.param_groups)
    adamw = optim.build_adam_optimizer(net, hyp, decoupled=True)
    assert type(adamw) is optim.AdamW and [x["decoupled_weight_decay"] for x in adamw.param_groups] == [True] * 3
    assert [x["weight_decay"] for x in adamw.param_groups] == [0, hyp["weight_decay"], 0]
    assert optim.AdamW([nn.Parameter(torch.zeros(1))]).defaults == torch.optim.AdamW([nn.Parameter(torch.zeros(1))]).defaults


@pytest.mark.parametrize("cfg", ["yolov5s_fusion_add_vedai", "yolov5s_fusion_transformerx3_vedai"])
def test_build_adam_optimizer_groups_equal_reference(mods, cfg):
    optim = mods[0]
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    with open(os.path.join(GOLDEN, "groups.json")) as fh:
        want = json.load(fh)[cfg]
    model = Model(named_config(cfg))
    hyp = {"lr0": 0.01, "momentum": 0.937, "weight_decay": 0.0005}
    opt = optim.build_adam_optimizer(model, hyp)
    assert type(opt) is optim.Adam
    got = R.group_names(model, [g["params"] for g in opt.param_groups])
    for name, g, w in zip(("pg0", "pg1", "pg2"), got, (want["pg0"], want["pg1"], want["pg2"])):
        assert g == w, name
    g0 = opt.param_groups[0]
    assert g0["betas"] == (hyp["momentum"], 0.999) and g0["lr"] == hyp["lr0"] and all("momentum" not in g for g in opt.param_groups)
    assert [g["weight_decay"] for g in opt.param_groups] == [0, hyp["weight_decay"], 0]
    assert all(g["betas"] == (hyp["momentum"], 0.999) and g["eps"] == 1e-8 for g in opt.param_groups)


def test_warmup_moves_lr_only(mods, golden):
    optim, general = mods
    hyp, nw, nbs, tbs = golden["hyp"], golden["nw"], golden["nbs"], golden["total_batch_size"]
    net = R.SmallNet()
    adam, sgd = optim.build_adam_optimizer(net, hyp), optim.build_optimizer(net, hyp)
    assert R.group_names(net, [x["params"] for x in adam.param_groups]) == golden["groups"]
    lf = general.one_cycle(1, hyp["lrf"], golden["epochs"])
    for opt in (adam, sgd):
        torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lf)
    for step in golden["steps"]:
        acc = optim.warmup(adam, step["ni"], nw, golden["epoch"], lf, hyp, nbs, tbs)
        assert acc == optim.warmup(sgd, step["ni"], nw, golden["epoch"], lf, hyp, nbs, tbs) == step["accumulate"]
        assert [float(x["lr"]) for x in adam.param_groups] == step["lr"] == [float(x["lr"]) for x in sgd.param_groups]
        assert [tuple(x["betas"]) for x in adam.param_groups] == step["betas"] == [(hyp["momentum"], 0.999)] * 3
        assert all("momentum" not in x for x in adam.param_groups)


def test_golden_recording_is_within_the_bound_of_the_oracle(golden):
    net = R.SmallNet()
    names = dict(net.named_parameters())
    params = {k: v for k, v in R.seeded_state(net, 0).items() if k in names}
    m = v = None
    group_of = {n: j for j, group in enumerate(golden["groups"]) for n in group}
    assert sorted(group_of) == sorted(params)
    for k, step in enumerate(golden["steps"]):
        grads = R.seeded_grads(net, k)
        for n in params:
            j = group_of[n]
            assert step["step"][n] == k + 1
            p1, m1, v1, bp, bm, bv = A.adam_step(params[n], grads[n], m[n] if m else None, v[n] if v else None, k + 1, step["lr"][j],
                                                 *step["betas"][j], step["eps"][j], step["weight_decay"][j], False)
            assert A.worst(step["params"][n], p1, bp) <= 1.0 and A.worst(step["exp_avg"][n], m1, bm) <= 1.0, (k, n)
            assert A.worst(step["exp_avg_sq"][n], v1, bv) <= 1.0, (k, n)
        params, m, v = step["params"], step["exp_avg"], step["exp_avg_sq"]
