"""GPU tests of the optimiser half of a training step (csrc/optim.hip, utils/optim.py, utils/torch_utils.py, the checkpoint
functions of utils/general.py) against the float64 oracle of tests/optim_ref.py, torch.optim.SGD on the CPU and the reference's
ModelEMA recorded in tests/golden/optim/.  The bound is optim_ref's: |got - ref64| <= 8 * 2^-24 * (sum of the |terms|)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import optim_ref as R
from launch_trace import recording

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "optim", "optim_cases.pt")
LOSS_GOLDEN = os.path.join(ROOT, "tests", "golden", "loss", "loss_cases.pt")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def _mods():
    import msod_amd  # noqa: F401
    from msod_amd.utils import general, optim, torch_utils
    return optim, torch_utils, general


def _randn(rng, n, lo=-3, hi=0):
    return torch.from_numpy((rng.standard_normal(n) * 10.0 ** rng.uniform(lo, hi, n)).astype(np.float32))


class _Params:
    """The synthetic parameter list of the numerics tests: every size at which the kernel takes another path (dword tails, one
    element short of / exactly / one past a chunk, several chunks), one full chunk at storage offset 1 (misaligned for 16-byte
    access), one parameter without a gradient and one outside every group."""

    def __init__(self, dev, chunk, seed=3):
        rng = np.random.default_rng(seed)
        self.sizes = [1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
        self.params = [_randn(rng, n, -2, 1).to(dev).requires_grad_() for n in self.sizes]
        base = torch.zeros(chunk + 1, device=dev)
        view = base[1:]
        view.copy_(_randn(rng, chunk, -2, 1))
        assert view.storage_offset() == 1 and view.data_ptr() % 16 == 4
        self.params.append(view.requires_grad_())
        self.no_grad = _randn(rng, 300, -2, 1).to(dev).requires_grad_()          # in a group, .grad stays None
        self.frozen = _randn(rng, 300, -2, 1).to(dev)                             # requires_grad False, in no group
        self.group_of = [i % 3 for i in range(len(self.params))]
        self.rng = rng

    def groups(self):
        gs = [[p for p, j in zip(self.params, self.group_of) if j == k] for k in range(3)]
        gs[1].append(self.no_grad)
        return gs

    def new_grads(self, scale=1.0):
        for p in self.params:
            p.grad = (_randn(self.rng, p.numel()) * scale).to(p.device)


def _make(optim_cls, groups, lrs, moms, wds, nesterov, **kw):
    opt = optim_cls(groups[0], lr=lrs[0], momentum=moms[0], weight_decay=wds[0], nesterov=nesterov, **kw)
    for k in (1, 2):
        opt.add_param_group({"params": groups[k], "lr": lrs[k], "momentum": moms[k], "weight_decay": wds[k]})
    return opt


def _snapshot(ps, opt):
    return ([p.detach().cpu().clone() for p in ps.params],
            [opt.state[p]["momentum_buffer"].cpu().clone() if "momentum_buffer" in opt.state.get(p, {}) else None for p in ps.params])


def _check_step(what, ps, before, after, grads, hyp, nesterov, grad_scale=None):
    (p0, b0), (p1, b1) = before, after
    lrs, moms, wds = hyp
    worst_p = worst_b = 0.0
    for i, j in enumerate(ps.group_of):
        rp, rb, bp, bb = R.sgd_step(p0[i], grads[i], b0[i], lrs[j], moms[j], wds[j], nesterov, grad_scale)
        worst_p = max(worst_p, R.worst(p1[i], rp, bp))
        if moms[j] != 0:
            worst_b = max(worst_b, R.worst(b1[i], rb, bb))
        else:
            assert b1[i] is None, f"{what}: a buffer without momentum"
    print(f"{what}: worst |err| / bound: params {worst_p:.3f}, buffers {worst_b:.3f}")
    assert worst_p <= 1.0 and worst_b <= 1.0, what


@pytest.mark.parametrize("nesterov,wd,momentum", list(itertools.product((True, False), (0.0, 5e-4), (0.0, 0.937))))
def test_sgd_numerics(dev, nesterov, wd, momentum):
    optim = _mods()[0]
    lrs, moms, wds = (0.01, 0.02, 0.1), (momentum, momentum * 0.9, momentum * 0.5), (wd, wd * 2, 0.0)
    if nesterov and momentum == 0:
        with pytest.raises(ValueError, match="[Nn]esterov"):                     # as torch.optim.SGD
            _make(optim.SGD, _Params(dev, optim.CHUNK).groups(), lrs, moms, wds, nesterov)
        return

    def run(check):
        ps = _Params(dev, optim.CHUNK)
        opt = _make(optim.SGD, ps.groups(), lrs, moms, wds, nesterov)
        keep = (ps.no_grad.detach().clone(), ps.frozen.clone())
        trail = []
        for step in range(3):
            ps.new_grads()
            before = _snapshot(ps, opt)
            grads = [p.grad.cpu().clone() for p in ps.params]
            opt.step()
            after = _snapshot(ps, opt)
            trail.append(after)
            if not check:
                continue
            what = f"nesterov {nesterov} wd {wd} momentum {momentum} step {step}"
            _check_step(what, ps, before, after, grads, (lrs, moms, wds), nesterov)
            # torch.optim.SGD on the CPU from the same state: both are within the bound of the float64 value, so within twice of each other
            cpu = [p.clone().requires_grad_() for p in before[0]]
            cgroups = [[p for p, j in zip(cpu, ps.group_of) if j == k] for k in range(3)]
            ref = _make(torch.optim.SGD, cgroups, lrs, moms, wds, nesterov)
            for p, g, b in zip(cpu, grads, before[1]):
                p.grad = g.clone()
                if b is not None:
                    ref.state[p]["momentum_buffer"] = b.clone()
            ref.step()
            for i, j in enumerate(ps.group_of):
                _, _, bp, bb = R.sgd_step(before[0][i], grads[i], before[1][i], lrs[j], moms[j], wds[j], nesterov)
                assert R.worst(after[0][i], cpu[i].detach().numpy().astype(np.float64), 2 * bp) <= 1.0, (what, i)
                if moms[j] != 0:
                    assert R.worst(after[1][i], ref.state[cpu[i]]["momentum_buffer"].numpy().astype(np.float64), 2 * bb) <= 1.0, (what, i)
        assert torch.equal(ps.no_grad, keep[0]) and torch.equal(ps.frozen, keep[1])          # untouched: bit-identical
        assert ps.no_grad not in opt.state or "momentum_buffer" not in opt.state[ps.no_grad]
        assert 1 <= opt.table_uploads <= 3       # fresh gradient tensors every step here: the table follows them where they moved
        return trail

    first, second = run(True), run(False)
    for a, b in zip(first, second):                                                            # the same run to run, bit for bit
        for x, y in zip(a[0] + [t for t in a[1] if t is not None], b[0] + [t for t in b[1] if t is not None]):
            assert torch.equal(x, y)


def test_cut_and_grid_do_not_change_the_result(dev):
    """The rule is per element, so neither the cut of the table nor the number of workgroups that walk it can show in the result:
    chunk 1024 on two workgroups (33 work rows for the step, 11 for the EMA: every workgroup wraps, the chunk boundaries fall
    elsewhere) gives, bit for bit, what the defaults give - and stays within the oracle's bound.  Group 1 has no momentum: the
    walk's absent stream."""
    optim, torch_utils, _ = _mods()
    lrs, moms, wds = (0.01, 0.02, 0.1), (0.937, 0.0, 0.5), (0.0, 5e-4, 0.0)

    def sgd(**cut):
        ps = _Params(dev, optim.CHUNK)
        opt = _make(optim.SGD, ps.groups(), lrs, moms, wds, False, **cut)
        trail = []
        for step in range(3):
            ps.new_grads()
            before, grads = _snapshot(ps, opt), [p.grad.cpu().clone() for p in ps.params]
            opt.step()
            trail.append(_snapshot(ps, opt))
            if cut:
                _check_step(f"chunk 1024, 2 workgroups, step {step}", ps, before, trail[-1], grads, (lrs, moms, wds), False)
        return trail, opt._table

    def ema(cut):
        net = R.SmallNet().to(dev)
        net.load_state_dict(R.seeded_state(net, 0))
        avg = torch_utils.ModelEMA(net, updates=2000)                             # decay 0.63: both terms of the rule count
        if cut:
            avg._table, avg._max_blocks = optim.DeviceTable(1024), 2
        trail = [{name: v.cpu().clone() for name, v in avg.ema.state_dict().items()}]
        for k in (1, 2, 3):
            model = R.seeded_state(net, k)
            net.load_state_dict(model)
            avg.update(net)
            trail.append({name: v.cpu().clone() for name, v in avg.ema.state_dict().items()})
            for name, v in trail[-1].items():
                if cut and v.dtype.is_floating_point:
                    ref, bound = R.ema_update(trail[-2][name], model[name], avg.decay(avg.updates))
                    assert R.worst(v, ref, bound) <= 1.0, (k, name)
        return trail, avg._table

    (want, table), (got, cut_table) = sgd(), sgd(chunk=1024, max_blocks=2)
    assert (table.chunk, cut_table.chunk) == (optim.CHUNK, 1024) and cut_table.nwork == 33 > table.nwork
    for a, b in zip(want, got):
        for x, y in zip(a[0] + a[1], b[0] + b[1]):
            assert (x is None and y is None) if x is None or y is None else torch.equal(x, y)
    (want, table), (got, cut_table) = ema(False), ema(True)
    assert (table.chunk, cut_table.chunk) == (optim.CHUNK, 1024) and cut_table.nwork == 11 > table.nwork
    for a, b in zip(want, got):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_one_launch_no_synchronise(dev, golden):
    optim, torch_utils, _ = _mods()
    ps = _Params(dev, optim.CHUNK)
    lrs, moms, wds = [0.01, 0.02, 0.1], (0.937, 0.9, 0.5), (0.0, 5e-4, 0.0)
    opt = _make(optim.SGD, ps.groups(), lrs, moms, wds, True)
    net = R.SmallNet().to(dev)
    ema = torch_utils.ModelEMA(net)
    ps.new_grads()
    opt.step()
    ema.update(net)
    assert opt.table_uploads == 1
    for p in ps.params:                                      # same gradient tensors, new values: what loss.backward() does after zero_grad(False)
        p.grad.copy_(_randn(ps.rng, p.numel()).to(dev))
    versions = [p._version for p in ps.params]
    before, grads = _snapshot(ps, opt), [p.grad.cpu().clone() for p in ps.params]
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with recording(dev) as events:
            opt.step()
            ema.update(net)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    names = [e.split()[0] for e in events]
    assert names == ["cft_sgd_step", "cft_ema_update"], names
    assert opt.table_uploads == 1 and ema._table.uploads == 1
    assert all(p._version > v for p, v in zip(ps.params, versions))          # Model's caches key on the version counters
    _check_step("second step", ps, before, _snapshot(ps, opt), grads, (lrs, moms, wds), True)
    # a new lr takes effect with the table as it is
    opt.param_groups[1]["lr"] = lrs[1] = 0.5
    before = _snapshot(ps, opt)
    opt.step()
    assert opt.table_uploads == 1
    _check_step("new lr", ps, before, _snapshot(ps, opt), grads, (lrs, moms, wds), True)
    # a gradient set to None drops its parameter from the step
    ps.params[4].grad = None
    before = _snapshot(ps, opt)
    opt.step()
    after = _snapshot(ps, opt)
    assert opt.table_uploads == 2
    assert torch.equal(after[0][4], before[0][4]) and torch.equal(after[1][4], before[1][4])
    assert not torch.equal(after[0][5], before[0][5])


def test_grad_scaler(dev):
    optim = _mods()[0]
    ps = _Params(dev, optim.CHUNK)
    lrs, moms, wds = (0.01, 0.02, 0.1), (0.937, 0.9, 0.5), (0.0, 5e-4, 0.0)
    opt = _make(optim.SGD, ps.groups(), lrs, moms, wds, True)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.)
    scaler.scale(torch.zeros(1, device=dev))                                   # (creates the scale tensor, as scaler.scale(loss) does)
    ps.new_grads(scale=1024.0)                                                 # what backward of the scaled loss leaves
    before, grads = _snapshot(ps, opt), [p.grad.cpu().clone() for p in ps.params]
    scaler.step(opt)
    scaler.update()
    after = _snapshot(ps, opt)
    _check_step("scaled step", ps, before, after, grads, (lrs, moms, wds), True, grad_scale=1024.0)
    assert scaler.get_scale() == 1024.0 and not hasattr(opt, "grad_scale")
    ps.new_grads(scale=1024.0)
    ps.params[7].grad[5] = float("inf")
    scaler.step(opt)
    scaler.update()
    skipped = _snapshot(ps, opt)
    for a, b in zip(after[0] + after[1], skipped[0] + skipped[1]):
        assert torch.equal(a, b)                                                # found_inf: nothing is written
    assert scaler.get_scale() == 512.0


def test_ema_numerics(dev, golden):
    _, torch_utils, _ = _mods()
    net = R.SmallNet().to(dev)
    net.load_state_dict(R.seeded_state(net, 0))
    ema = torch_utils.ModelEMA(net)
    assert not ema.ema.training and all(not p.requires_grad for p in ema.ema.parameters())
    prev = {k: v.cpu().clone() for k, v in ema.ema.state_dict().items()}
    for rec in golden["ema"]:
        if rec["updates"] == 2000:
            ema.updates = 1999
            ema.ema.load_state_dict(golden["ema"][2]["state"])                  # exactly the state the recording went on from
            prev = golden["ema"][2]["state"]
        model = R.seeded_state(net, rec["model_state"])
        net.load_state_dict(model)
        ema.update(net)
        assert ema.updates == rec["updates"] and abs(ema.decay(ema.updates) - rec["decay"]) <= 1e-15
        got = {k: v.cpu().clone() for k, v in ema.ema.state_dict().items()}
        for k, v in got.items():
            if not v.dtype.is_floating_point:
                assert int(v) == 0 and int(model[k]) == rec["model_state"], k     # num_batches_tracked: left alone
                continue
            ref, bound = R.ema_update(prev[k], model[k], rec["decay"])
            w = R.worst(v, ref, bound)
            assert w <= 1.0, (rec["updates"], k, w)
        prev = got
    # against the recording itself, each update from the recorded state before it: the kernel rounds twice (d * e, the fma), the
    # reference three times, each by at most half an ulp <= 2^-24 T: together 5/8 of the bound
    prev = R.seeded_state(net, 0)
    for rec in golden["ema"]:
        ema.ema.load_state_dict(prev)
        ema.updates = rec["updates"] - 1
        model = R.seeded_state(net, rec["model_state"])
        net.load_state_dict(model)
        ema.update(net)
        for k, v in ema.ema.state_dict().items():
            if v.dtype.is_floating_point:
                _, bound = R.ema_update(prev[k], model[k], rec["decay"])
                assert R.worst(v, rec["state"][k].numpy().astype(np.float64), bound) <= 1.0, (rec["updates"], k)
        prev = rec["state"]


def _small_model(dev, seed=7):
    from msod_amd.models.configs import cft_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils.seeded import seeded_inputs, seeded_state_dict
    cfg = cft_config("s", "add", 1)
    model = Model(cfg)
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed))
    rgb, ir = seeded_inputs(1, 64, 64, seed)
    return cfg, model.to(dev).eval(), rgb.to(dev), ir.to(dev)


def _fresh_forward(cfg, state_dict, dev, x, x2):
    from msod_amd.models.yolo_test import Model
    fresh = Model(cfg)
    fresh.load_state_dict({k: v.cpu() for k, v in state_dict.items()})
    with torch.no_grad():
        return fresh.to(dev).eval()(x, x2)[0]


def _seeded_model_grads(model, seed=5):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    for p in model.parameters():
        p.grad = (torch.randn(p.shape, generator=g) * p.detach().abs().mean().cpu()).to(p.device)


def test_step_invalidates_packed_weights(dev, golden):
    optim = _mods()[0]
    cfg, model, x, x2 = _small_model(dev)
    with torch.no_grad():
        before = model(x, x2)[0].clone()                      # packed weights exist now
    opt = optim.build_optimizer(model, golden["sgd"]["hyp"])
    for g in opt.param_groups:
        g["lr"] = 0.1                                          # large enough to move 16-bit packed weights
    _seeded_model_grads(model)
    opt.step()
    with torch.no_grad():
        after = model(x, x2)[0].clone()
    want = _fresh_forward(cfg, model.state_dict(), dev, x, x2)
    assert torch.isfinite(after).all()
    assert not torch.equal(after, before), "the forward still runs the weights of before the step"
    assert torch.equal(after, want)


def test_ema_update_invalidates_packed_weights_and_graphs(dev):
    _, torch_utils, _ = _mods()
    from msod_amd.utils.seeded import seeded_state_dict
    cfg, model, x, x2 = _small_model(dev)
    with torch.no_grad():
        model.capture(1, 64, 64)
        kept = model(x, x2)[0].clone()
        ema = torch_utils.ModelEMA(model)                      # a model with packed weights, plans and a captured graph
        assert len(model._graphs) == 1 and ema.ema._graphs == {} and torch.equal(model(x, x2)[0], kept)
        for a, b in zip(ema.ema.state_dict().values(), model.state_dict().values()):
            assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
        ema.ema.capture(1, 64, 64)
        first = ema.ema(x, x2)[0].clone()
        assert torch.equal(first, kept)
        model.load_state_dict(seeded_state_dict(model.state_dict(), 77))          # "training" moved the model
        ema.update(model)
        got = ema.ema(x, x2)[0].clone()
        assert len(ema.ema._graphs) == 0                                           # the graph of the old average is gone
    want = _fresh_forward(cfg, ema.ema.state_dict(), dev, x, x2)
    assert not torch.equal(got, first) and torch.equal(got, want)
    assert ema.updates == 1


def test_closed_loop_on_hip_kernels(dev):
    optim = _mods()[0]
    from make_loss_golden import StubModel
    from msod_amd.utils.loss import ComputeLoss
    cases = torch.load(LOSS_GOLDEN, weights_only=False)["cases"]
    c = min((c for c in cases if c["targets"].shape[0] and not c["autobalance"]), key=lambda c: sum(t.numel() for t in c["calls"][0]["p"]))
    p = [t.float().to(dev).requires_grad_() for t in c["calls"][0]["p"]]
    cl = ComputeLoss(StubModel(c["nc"], c["hyp"], c["gr"]).to(dev))
    opt = optim.SGD(p, lr=0.5, momentum=0.9, nesterov=True)
    targets = c["targets"].to(dev)
    losses = []
    for _ in range(10):
        loss, _ = cl(p, targets)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    print(f"closed loop on case {c['name']}: losses {losses}")
    assert all(np.isfinite(losses)) and all(torch.isfinite(t).all() for t in p)
    assert losses[9] < losses[0]
    cl.check()


def test_checkpoint_round_trip(dev, golden, tmp_path):
    optim, torch_utils, general = _mods()
    from msod_amd import compat
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils.seeded import seeded_state_dict
    cfg, model, x, x2 = _small_model(dev)
    with torch.no_grad():
        model(x, x2)
    ema = torch_utils.ModelEMA(model)
    opt = optim.build_optimizer(model, golden["sgd"]["hyp"])
    _seeded_model_grads(model)
    opt.step()
    model.load_state_dict(seeded_state_dict(model.state_dict(), 78))
    ema.update(model)
    last, best = str(tmp_path / "last.pt"), str(tmp_path / "best.pt")
    general.save_checkpoint(last, 2, 0.1, model, ema, opt, training_results="")
    ck = torch.load(last, weights_only=False)
    assert ck["updates"] == 1 and len(ck["optimizer"]["state"]) == sum(len(g["params"]) for g in opt.param_groups)
    assert next(ema.ema.parameters()).dtype == torch.float32 and next(model.parameters()).dtype == torch.float32
    for name in (last, best):
        if name == best:
            general.strip_optimizer(last, best)
        loaded = compat.attempt_load(name, map_location="cpu").to(dev)
        # what the file holds: the average rounded to half precision, widened again, BatchNorm folded by fuse() on the host
        fresh = Model(cfg)
        fresh.load_state_dict({k: (v.half().float() if v.dtype.is_floating_point else v).cpu() for k, v in ema.ema.state_dict().items()})
        fresh = fresh.float().fuse().eval().to(dev).set_compute_dtype(loaded.compute_dtype)
        with torch.no_grad():
            assert loaded.compute_dtype == torch.float32 and torch.equal(loaded(x, x2)[0], fresh(x, x2)[0]), name
