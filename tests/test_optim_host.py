"""CPU tests of the optimiser half of a training step: the float64 oracle (tests/optim_ref.py) against torch.optim.SGD and the
reference's ModelEMA recorded in tests/golden/optim/, the parameter-group rule, schedule and warm-up, the optimiser's state-dict
layout, the checkpoint functions, the ABI and the Python-side validation of msod_amd.utils.optim."""
import copy
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "optim")


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLDEN, "optim_cases.pt"), weights_only=False)


@pytest.fixture(scope="module")
def mods():
    import msod_amd  # noqa: F401
    from msod_amd.utils import general, optim, torch_utils
    return optim, torch_utils, general


def test_oracle_reproduces_reference_ema(golden):
    net = R.SmallNet()
    prev = R.seeded_state(net, 0)
    assert [r["updates"] for r in golden["ema"]] == [1, 2, 3, 2000]
    for rec in golden["ema"]:
        d = 0.9999 * (1 - np.exp(-rec["updates"] / 2000))
        assert abs(d - rec["decay"]) <= 1e-15
        model = R.seeded_state(net, rec["model_state"])
        for k, v in rec["state"].items():
            if not v.dtype.is_floating_point:
                assert torch.equal(v, prev[k]) and int(v) == 0, k       # num_batches_tracked: never averaged
                continue
            ref, bound = R.ema_update(prev[k], model[k], rec["decay"])
            assert R.worst(v, ref, bound) <= 1.0, (rec["updates"], k)
        prev = rec["state"]


def test_oracle_reproduces_torch_sgd(golden):
    g = golden["sgd"]
    net = R.SmallNet()
    params, buffers = {k: v for k, v in R.seeded_state(net, 0).items() if k in dict(net.named_parameters())}, None
    group_of = {n: j for j, names in enumerate(g["groups"]) for n in names}
    assert sorted(group_of) == sorted(params)
    for k, step in enumerate(g["steps"]):
        grads = R.seeded_grads(net, k)
        for n in params:
            j = group_of[n]
            p1, b1, bp, bb = R.sgd_step(params[n], grads[n], buffers[n] if buffers else None, step["lr"][j], step["momentum"][j],
                                        step["weight_decay"][j], True)
            assert R.worst(step["params"][n], p1, bp) <= 1.0, (k, n)
            assert R.worst(step["buffers"][n], b1, bb) <= 1.0, (k, n)
        params, buffers = step["params"], step["buffers"]


def test_oracle_bound_catches_wrong_forms():
    rng = np.random.default_rng(5)
    p, g, b = (torch.from_numpy(rng.standard_normal(4001).astype(np.float32)) for _ in range(3))
    p1, b1, bp, bb = R.sgd_step(p, g, b, 0.01, 0.937, 5e-4, True)
    wrong = [R.sgd_step(p, g, b, 0.01, 0.937, 5e-4, False), R.sgd_step(p, g, b, 0.01, 0.937, 0.0, True), R.sgd_step(p, g, b, -0.01, 0.937, 5e-4, True)]
    # the smallest of these errors is the dropped decay: lr * wd * (1 + m) |p| = 9.7e-6 |p| against a bound of about 4.8e-7 |p|
    for w in wrong:
        assert R.worst(torch.from_numpy(w[0].astype(np.float32)), p1, bp) > 10
    assert R.worst(torch.from_numpy(p1.astype(np.float32)), p1, bp) <= 1.0
    e1, be = R.ema_update(p, g, 0.9)
    assert R.worst(torch.from_numpy(R.ema_update(p, g, 0.1)[0].astype(np.float32)), e1, be) > 100


@pytest.mark.parametrize("cfg", ["yolov5s_fusion_add_vedai", "yolov5s_fusion_transformerx3_vedai"])
def test_param_groups_equal_reference(mods, cfg):
    optim = mods[0]
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    with open(os.path.join(GOLDEN, "groups.json")) as fh:
        want = json.load(fh)[cfg]
    model = Model(named_config(cfg))
    got = R.group_names(model, optim.param_groups(model))
    for name, g, w in zip(("pg0", "pg1", "pg2"), got, (want["pg0"], want["pg1"], want["pg2"])):
        assert g == w, name
    grouped = {n for g in got for n in g}
    ungrouped = [n for n, _ in model.named_parameters() if n not in grouped]
    assert ungrouped == want["ungrouped"]
    assert all(n.endswith("pos_emb") for n in ungrouped) and (len(ungrouped) == 3) == ("transformerx3" in cfg)


def test_one_cycle_matches_reference(mods, golden):
    rec = golden["one_cycle"]
    lf = mods[2].one_cycle(*rec["args"])
    assert [lf(x) for x in rec["x"]] == rec["y"]
    assert lf(0) == 1 and abs(lf(300) - 0.2) < 1e-15


def _reference_setup(optim, general, g, net, cls=None):
    hyp = g["hyp"]
    if cls is None:
        opt = optim.build_optimizer(net, hyp)
    else:
        pg0, pg1, pg2 = optim.param_groups(net)
        opt = cls(pg0, lr=hyp["lr0"], momentum=hyp["momentum"], nesterov=True)
        opt.add_param_group({"params": pg1, "weight_decay": hyp["weight_decay"]})
        opt.add_param_group({"params": pg2})
    lf = general.one_cycle(1, hyp["lrf"], g["epochs"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lf)
    return opt, lf, sched


def test_warmup_matches_interp_and_recording(mods, golden):
    optim, _, general = mods
    g = golden["sgd"]
    hyp, nw, nbs, tbs = g["hyp"], g["nw"], g["nbs"], g["total_batch_size"]
    net = R.SmallNet()
    opt, lf, _ = _reference_setup(optim, general, g, net)
    assert R.group_names(net, [x["params"] for x in opt.param_groups]) == g["groups"]
    assert [x["weight_decay"] for x in opt.param_groups] == [0, hyp["weight_decay"], 0] and all(x["nesterov"] for x in opt.param_groups)
    for ni in (0, nw // 2, nw):
        acc = optim.warmup(opt, ni, nw, 0, lf, hyp, nbs, tbs)
        assert acc == max(1, np.interp(ni, [0, nw], [1, nbs / tbs]).round())
        for j, x in enumerate(opt.param_groups):
            assert x["lr"] == np.interp(ni, [0, nw], [hyp["warmup_bias_lr"] if j == 2 else 0.0, hyp["lr0"] * lf(0)])
            assert x["momentum"] == np.interp(ni, [0, nw], [hyp["warmup_momentum"], hyp["momentum"]])
    for step in g["steps"]:
        assert optim.warmup(opt, step["ni"], nw, g["epoch"], lf, hyp, nbs, tbs) == step["accumulate"]
        assert [float(x["lr"]) for x in opt.param_groups] == step["lr"]
        assert [float(x["momentum"]) for x in opt.param_groups] == step["momentum"]
    before = [(x["lr"], x["momentum"]) for x in opt.param_groups]
    assert optim.warmup(opt, nw + 1, nw, 0, lf, hyp, nbs, tbs) == 4 and before == [(x["lr"], x["momentum"]) for x in opt.param_groups]


def test_linear_and_cosine_schedules_drive_the_optimizer(mods, golden):
    optim, _, general = mods
    g = golden["sgd"]
    net = R.SmallNet()
    opt, lf, sched = _reference_setup(optim, general, g, net)
    assert all(x["initial_lr"] == g["hyp"]["lr0"] for x in opt.param_groups)
    epochs, lrf = 10, g["hyp"]["lrf"]
    linear = torch.optim.lr_scheduler.LambdaLR(optim.build_optimizer(net, g["hyp"]), lr_lambda=lambda x: (1 - x / (epochs - 1)) * (1.0 - lrf) + lrf)
    assert linear.get_last_lr() == [g["hyp"]["lr0"]] * 3


def test_state_dict_round_trip_with_torch_sgd(mods, golden):
    optim, _, general = mods
    g = golden["sgd"]
    net = R.SmallNet()
    net.load_state_dict(R.seeded_state(net, 0))
    theirs, _, _ = _reference_setup(optim, general, g, net, cls=torch.optim.SGD)
    for n, gr in R.seeded_grads(net, 0).items():
        net.get_parameter(n).grad = gr
    theirs.step()
    sd = copy.deepcopy(theirs.state_dict())      # (load_state_dict keeps the tensors it is given: without copies the three would share buffers)
    ours = optim.build_optimizer(net, g["hyp"])
    ours.load_state_dict(copy.deepcopy(sd))                                            # torch's -> ours
    assert [len(x["params"]) for x in ours.param_groups] == [len(x["params"]) for x in theirs.param_groups]
    for p in net.parameters():
        assert torch.equal(ours.state[p]["momentum_buffer"], theirs.state[p]["momentum_buffer"])
    for a, b in zip(ours.param_groups, theirs.param_groups):
        assert {k: a[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "initial_lr")} == \
               {k: b[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "initial_lr")}
    back = copy.deepcopy(ours.state_dict())                                            # ours -> torch's
    assert set(back) == set(sd) and set(back["param_groups"][0]) == set(sd["param_groups"][0])
    again, _, _ = _reference_setup(optim, general, g, net, cls=torch.optim.SGD)
    again.load_state_dict(back)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    again.step()                                                        # and torch steps on from it
    want = {n: p.detach().clone() for n, p in net.named_parameters()}
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(before[n])
    theirs.step()
    for n, p in net.named_parameters():
        assert torch.equal(p, want[n]), n
    # a state dict of the reference's time has no maximize / foreach keys
    old = ours.state_dict()
    for grp in old["param_groups"]:
        for k in ("maximize", "foreach", "differentiable", "fused"):
            grp.pop(k)
    ours.load_state_dict(old)
    assert all(x["maximize"] is False for x in ours.param_groups)


class _Stub(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 1)
        self.bn = nn.BatchNorm2d(4)
        self.names = ["a", "b"]


def test_checkpoint_keys_and_dtypes(mods, tmp_path, golden):
    optim, torch_utils, general = mods
    model = _Stub()
    model._cft_cache = ("stale", object())                              # a cache must not travel
    ema = torch_utils.ModelEMA(model, updates=7)
    assert not ema.ema.training and all(not p.requires_grad for p in ema.ema.parameters()) and "_cft_cache" not in ema.ema.__dict__
    assert "_cft_cache" in model.__dict__ and ema.updates == 7 and abs(ema.decay(2000) - 0.9999 * (1 - np.exp(-1))) < 1e-15
    ema.update_attr(model, include=("names",))
    opt = optim.build_optimizer(model, golden["sgd"]["hyp"])
    last, best = str(tmp_path / "last.pt"), str(tmp_path / "best.pt")
    general.save_checkpoint(last, 3, 0.5, model, ema, opt, training_results="r")
    ck = torch.load(last, weights_only=False)
    assert set(ck) == {"epoch", "best_fitness", "training_results", "model", "ema", "updates", "optimizer", "wandb_id"}
    assert ck["epoch"] == 3 and ck["best_fitness"] == 0.5 and ck["updates"] == 7 and ck["wandb_id"] is None and ck["training_results"] == "r"
    assert set(ck["optimizer"]) == {"state", "param_groups"} and len(ck["optimizer"]["param_groups"]) == 3
    for k in ("model", "ema"):
        assert all(p.dtype == torch.float16 for p in ck[k].parameters()) and "_cft_cache" not in ck[k].__dict__
        assert ck[k].bn.num_batches_tracked.dtype == torch.int64
    assert next(model.parameters()).dtype == torch.float32 and next(ema.ema.parameters()).dtype == torch.float32
    with torch.no_grad():
        ck["ema"].conv.weight.fill_(0.25)
    torch.save(ck, last)
    general.strip_optimizer(last, best)
    st = torch.load(best, weights_only=False)
    assert set(st) == set(ck) and st["epoch"] == -1
    assert all(st[k] is None for k in ("optimizer", "training_results", "wandb_id", "ema", "updates"))
    assert all(p.dtype == torch.float16 and not p.requires_grad for p in st["model"].parameters())
    assert float(st["model"].conv.weight.float().mean()) == 0.25        # the EMA replaced the model
    general.strip_optimizer(last)                                       # in place
    assert torch.load(last, weights_only=False)["optimizer"] is None


def test_header_declares_the_entry_points():
    import msod_amd  # noqa: F401
    from msod_amd import _lib
    with open(_lib.HEADER) as fh:
        text = fh.read()
    sig, consts = _lib.parse_header(text)
    assert _lib.ABI_VERSION >= 19 and int(re.search(r"^#define\s+CFT_ABI_VERSION\s+(\d+)", text, re.M).group(1)) == _lib.ABI_VERSION
    assert "optim.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "optim.hip"))
    import ctypes as c
    p, i, l, f = c.c_void_p, c.c_int, c.c_long, c.c_float
    assert sig["cft_sgd_step"] == (i, [p, p, i, l, i, i, p, i, p, p, p])
    assert sig["cft_ema_update"] == (i, [p, p, i, l, i, i, f, f, p])
    assert consts["CFT_OPTIM_MAX_GROUPS"] == 8 and consts["CFT_OPTIM_CHUNK"] % 1024 == 0
    assert (consts["CFT_SGD_SEG_BYTES"], consts["CFT_EMA_SEG_BYTES"], consts["CFT_OPTIM_WORK_BYTES"]) == (40, 24, 16)
    with open(os.path.join(_lib.CSRC, "runtime.hip")) as fh:
        assert f"{_lib.ABI_VERSION}: cft_sgd_step" in fh.read()


def test_work_rows_are_the_canonical_cut(mods):
    optim = mods[0]
    c = optim.CHUNK
    counts = [1, 0, c - 1, c, c + 1, 2 * c + 3]
    want = [(0, 0), (2, 0), (3, 0), (4, 0), (4, c), (5, 0), (5, c), (5, 2 * c)]
    assert [tuple(r) for r in optim.work_rows(counts).tolist()] == want
    assert optim.work_rows([]).shape == (0, 2) and optim.work_rows([0, 0]).shape == (0, 2)


def test_errors_are_raised_before_any_device_work(mods):
    optim, torch_utils, _ = mods
    w = nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError, match="[Nn]esterov"):
        optim.SGD([w], lr=0.1, momentum=0, nesterov=True)
    with pytest.raises(ValueError, match="dampening"):
        optim.SGD([w], lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match="maximize"):
        optim.SGD([w], lr=0.1, maximize=True)
    with pytest.raises(ValueError):
        optim.SGD([w], lr=-1.0)
    with pytest.raises(NotImplementedError, match="torch.optim.Adam"):
        optim.build_optimizer(R.SmallNet(), {"lr0": 0.01, "momentum": 0.9, "weight_decay": 0.0}, adam=True)
    opt = optim.SGD([w], lr=0.1, momentum=0.9)
    assert opt.step() is None and opt.table_uploads == 0                # no gradient anywhere: nothing to do, as in torch
    dbl = nn.Parameter(torch.zeros(4, dtype=torch.float64))
    dbl.grad = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="float32"):
        optim.SGD([dbl], lr=0.1).step()
    h = nn.Parameter(torch.zeros(4, dtype=torch.float16))
    h.grad = torch.zeros(4, dtype=torch.float16)
    with pytest.raises(ValueError, match="float32"):
        optim.SGD([h], lr=0.1).step()
    s = nn.Parameter(torch.zeros(4, 6)[:, ::2])                         # a view with gaps
    s.grad = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="dense"):
        optim.SGD([s], lr=0.1).step()
    t = nn.Parameter(torch.zeros(3, 4).t())                             # dense, but its gradient is laid out otherwise
    t.grad = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="layout"):
        optim.SGD([t], lr=0.1).step()
    w.grad = torch.zeros(4)
    with pytest.raises(ValueError, match="GPU"):                        # right tensors, wrong device: still no kernel for it
        opt.step()
    opt.param_groups[0]["dampening"] = 0.5
    with pytest.raises(ValueError, match="dampening"):
        opt.step()
    with pytest.raises(ValueError, match="at most 8"):
        many = optim.SGD([nn.Parameter(torch.zeros(1))], lr=0.1)
        for _ in range(8):
            many.add_param_group({"params": [nn.Parameter(torch.zeros(1))]})
    ema = torch_utils.ModelEMA(R.SmallNet())
    with pytest.raises(ValueError, match="GPU"):
        ema.update(R.SmallNet())
    half = R.SmallNet().half()
    with pytest.raises(ValueError, match="float32"):
        torch_utils.ModelEMA(half).update(half)
