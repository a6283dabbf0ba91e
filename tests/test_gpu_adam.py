"""GPU tests of the Adam / AdamW step (cft_adam_step in csrc/optim.hip, utils/optim.Adam / AdamW / build_adam_optimizer) against the
float64 oracle of tests/adam_ref.py, torch.optim.Adam / AdamW on the CPU and the reference's ``--adam`` optimiser recorded in
tests/golden/optim/adam_cases.pt.  The bound is adam_ref's (first order, propagated, u = 2^-24): at most 1 against float64, at most 1
against twice the bound between the kernel and another float32 implementation.  Gradients are exactly 0 or at least 1e-12 in
magnitude (the bound assumes no float32 underflow in g * g)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import adam_ref as A
import optim_ref as R
from launch_trace import recording

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "optim", "adam_cases.pt")
LOSS_GOLDEN = os.path.join(ROOT, "tests", "golden", "loss", "loss_cases.pt")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)["adam"]


def _mods():
    import msod_amd  # noqa: F401
    from msod_amd.utils import general, optim, torch_utils
    return optim, torch_utils, general


class _Params:
    """The synthetic parameter list of the numerics tests: every size at which the kernel takes another path (dword tails, one
    element short of / exactly / one past a chunk, several chunks), one full chunk at storage offset 1 (misaligned for 16-byte
    access), one parameter without a gradient and one outside every group."""

    def __init__(self, dev, chunk, seed=3):
        rng = np.random.default_rng(seed)
        self.sizes = [1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
        self.params = [A.log_uniform(rng, n, -3, 2).to(dev).requires_grad_() for n in self.sizes]
        base = torch.zeros(chunk + 1, device=dev)
        view = base[1:]
        view.copy_(A.log_uniform(rng, chunk, -3, 2))
        assert view.storage_offset() == 1 and view.data_ptr() % 16 == 4
        self.params.append(view.requires_grad_())
        self.no_grad = A.log_uniform(rng, 300, -3, 2).to(dev).requires_grad_()          # in a group, .grad stays None
        self.frozen = A.log_uniform(rng, 300, -3, 2).to(dev)                             # requires_grad False, in no group
        self.group_of = [i % 3 for i in range(len(self.params))]
        self.rng = rng

    def groups(self):
        gs = [[p for p, j in zip(self.params, self.group_of) if j == k] for k in range(3)]
        gs[1].append(self.no_grad)
        return gs

    def new_grads(self, k=0, scale=1.0, skip=()):
        """Gradient set ``k`` (adam_ref.step_grads: 1 has a zeroed block, 2 is tiny) times ``scale`` into fresh ``.grad`` tensors;
        returns the CPU copies.  Parameters in ``skip`` get ``None`` (the random stream advances all the same)."""
        out = []
        for i, p in enumerate(self.params):
            g = A.step_grads(self.rng, p.numel(), k) * scale
            p.grad = None if i in skip else g.to(p.device)
            out.append(g)
        return out


class _Hyp:
    """Three groups that differ in every hyper-parameter."""

    def __init__(self, wd=5e-4, beta1=0.937, eps=1e-8):
        self.lr = [1e-2, 1e-3, 2e-2]
        self.betas = [(beta1, 0.999), (beta1 * 0.9, 0.99), (beta1 * 0.5, 0.9995)]
        self.eps = [eps, eps * 10, eps * 0.5]
        self.wd = [wd, wd * 2, 0.0]

    def make(self, cls, groups, **kw):
        opt = cls(groups[0], lr=self.lr[0], betas=self.betas[0], eps=self.eps[0], weight_decay=self.wd[0], **kw)
        for k in (1, 2):
            opt.add_param_group({"params": groups[k], "lr": self.lr[k], "betas": self.betas[k], "eps": self.eps[k], "weight_decay": self.wd[k]})
        return opt


def _snapshot(ps, opt):
    def get(p, key):
        st = opt.state.get(p, {})
        return st[key].detach().cpu().clone() if key in st else None
    steps = [get(p, "step") for p in ps.params]
    return ([p.detach().cpu().clone() for p in ps.params], [get(p, "exp_avg") for p in ps.params], [get(p, "exp_avg_sq") for p in ps.params],
            [0.0 if s is None else float(s) for s in steps])


def _check_step(what, ps, before, after, grads, hyp, decoupled, counts, grad_scale=None, skip=()):
    """``after`` against the float64 oracle from ``before``; ``counts[i]`` = the step count parameter i must have now."""
    worst = [0.0, 0.0, 0.0]
    for i, j in enumerate(ps.group_of):
        assert after[3][i] == counts[i], f"{what}: parameter {i} counts step {after[3][i]}, expected {counts[i]}"
        if i in skip:
            assert all(torch.equal(after[k][i], before[k][i]) if before[k][i] is not None else after[k][i] is None for k in range(3)), (what, i)
            continue
        ref = A.adam_step(before[0][i], grads[i], before[1][i], before[2][i], counts[i], hyp.lr[j], *hyp.betas[j], hyp.eps[j], hyp.wd[j],
                          decoupled, grad_scale)
        w = [A.worst(after[k][i], ref[k], ref[3 + k]) for k in range(3)]
        worst = [max(a, b) for a, b in zip(worst, w)]
    print(f"{what}: worst |err| / bound: params {worst[0]:.3f}, exp_avg {worst[1]:.3f}, exp_avg_sq {worst[2]:.3f}")
    assert max(worst) <= 1.0, (what, worst)
    return worst


def _check_against_torch(what, ps, before, after, grads, hyp, decoupled, counts):
    """torch.optim.Adam / AdamW on the CPU (single-tensor path) from the same state: both are within the bound of the float64
    value, so within twice the bound of each other."""
    cpu = [p.clone().requires_grad_() for p in before[0]]
    ref = hyp.make(torch.optim.AdamW if decoupled else torch.optim.Adam, [[p for p, j in zip(cpu, ps.group_of) if j == k] for k in range(3)])
    for g in ref.param_groups:
        g["foreach"] = False
    for i, p in enumerate(cpu):
        p.grad = grads[i].clone()
        if before[1][i] is not None:
            ref.state[p] = {"step": torch.tensor(float(before[3][i])), "exp_avg": before[1][i].clone(), "exp_avg_sq": before[2][i].clone()}
    ref.step()
    worst = 0.0
    for i, j in enumerate(ps.group_of):
        b = A.adam_step(before[0][i], grads[i], before[1][i], before[2][i], counts[i], hyp.lr[j], *hyp.betas[j], hyp.eps[j], hyp.wd[j], decoupled)
        theirs = (cpu[i].detach(), ref.state[cpu[i]]["exp_avg"], ref.state[cpu[i]]["exp_avg_sq"])
        assert float(ref.state[cpu[i]]["step"]) == counts[i]
        for k in range(3):
            worst = max(worst, A.worst(after[k][i], theirs[k].numpy().astype(np.float64), 2 * b[3 + k]))
    print(f"{what}: worst |kernel - torch CPU| / (2 * bound): {worst:.3f}")
    assert worst <= 1.0, what


@pytest.mark.parametrize("decoupled,wd,beta1,eps", list(itertools.product((False, True), (0.0, 5e-4), (0.937, 0.0), (1e-8, 1e-3))))
def test_adam_numerics(dev, decoupled, wd, beta1, eps):
    optim = _mods()[0]
    hyp = _Hyp(wd, beta1, eps)

    def run(check):
        ps = _Params(dev, optim.CHUNK)
        opt = hyp.make(optim.AdamW if decoupled else optim.Adam, ps.groups())
        assert all(g["decoupled_weight_decay"] is decoupled for g in opt.param_groups)
        keep = (ps.no_grad.detach().clone(), ps.frozen.clone())
        trail = []
        for step in range(4):                                     # gradient set 1 has a zeroed block, 2 is 1e-10 .. 1e-8
            before = _snapshot(ps, opt)
            grads = ps.new_grads(step)
            opt.step()
            after = _snapshot(ps, opt)
            trail.append(after)
            if check:
                what = f"{'AdamW' if decoupled else 'Adam'} wd {wd} beta1 {beta1} eps {eps} step {step + 1}"
                counts = [step + 1.0] * len(ps.params)
                _check_step(what, ps, before, after, grads, hyp, decoupled, counts)
                _check_against_torch(what, ps, before, after, grads, hyp, decoupled, counts)
                assert all(opt.state[p]["step"].dim() == 0 and opt.state[p]["step"].dtype == torch.float32 for p in ps.params)
        assert torch.equal(ps.no_grad, keep[0]) and torch.equal(ps.frozen, keep[1])          # untouched: bit-identical
        assert len(opt.state.get(ps.no_grad, {})) == 0
        assert 1 <= opt.table_uploads <= 4       # fresh gradient tensors every step here: the table follows them where they moved
        return trail

    first, second = run(True), run(False)
    for a, b in zip(first, second):                                                            # the same run to run, bit for bit
        for x, y in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]):
            assert torch.equal(x, y)
        assert a[3] == b[3]


def test_cut_and_grid_do_not_change_the_result(dev):
    """The rule is per element, so neither the cut of the table nor the number of workgroups that walk it can show in the result:
    chunk 1024 on two workgroups (33 work rows: both workgroups wrap many times, the chunk boundaries fall elsewhere) gives, bit
    for bit, the parameters, moments and step counts that the defaults give - and stays within the oracle's bound."""
    optim = _mods()[0]
    hyp = _Hyp()

    def run(cls, **cut):
        ps = _Params(dev, optim.CHUNK)
        opt = hyp.make(cls, ps.groups(), **cut)
        trail = []
        for step in range(3):
            before = _snapshot(ps, opt)
            grads = ps.new_grads(step)
            opt.step()
            trail.append(_snapshot(ps, opt))
            if cut:
                _check_step(f"{cls.__name__}, chunk 1024, 2 workgroups, step {step + 1}", ps, before, trail[-1], grads, hyp, cls is optim.AdamW,
                            [step + 1.0] * len(ps.params))
        return trail, opt._table

    for cls in (optim.Adam, optim.AdamW):
        (want, table), (got, cut_table) = run(cls), run(cls, chunk=1024, max_blocks=2)
        assert (table.chunk, cut_table.chunk) == (optim.CHUNK, 1024) and cut_table.nwork == 33 > table.nwork
        for step, (a, b) in enumerate(zip(want, got)):
            assert all(torch.equal(x, y) for x, y in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]))
            assert a[3] == b[3] == [step + 1.0] * len(a[3])


def test_step_counts_are_per_tensor(dev):
    optim = _mods()[0]
    hyp = _Hyp()
    ps = _Params(dev, optim.CHUNK)
    opt = hyp.make(optim.Adam, ps.groups())
    away = (4, 8)                                                 # a dword tensor and a full chunk sit out the second step
    counts = [0.0] * len(ps.params)
    for step, skip in enumerate(((), away, ())):
        before = _snapshot(ps, opt)
        grads = ps.new_grads(0, skip=skip)
        opt.step()
        counts = [c + (i not in skip) for i, c in enumerate(counts)]
        _check_step(f"step {step + 1}, without {skip}", ps, before, _snapshot(ps, opt), grads, hyp, False, counts, skip=skip)
    assert [counts[i] for i in away] == [2.0, 2.0] and set(c for i, c in enumerate(counts) if i not in away) == {3.0}
    assert [float(opt.state[ps.params[i]]["step"]) for i in away] == [2.0, 2.0]      # own bias correction: checked against the oracle at step 2


def test_one_entry_no_synchronise(dev):
    optim = _mods()[0]
    hyp = _Hyp()
    ps = _Params(dev, optim.CHUNK)
    opt = hyp.make(optim.Adam, ps.groups())
    ps.new_grads(0)
    opt.step()
    assert opt.table_uploads == 1
    grads = []
    for p in ps.params:                                      # same gradient tensors, new values: what loss.backward() does after zero_grad(False)
        grads.append(A.step_grads(ps.rng, p.numel(), 3))
        p.grad.copy_(grads[-1])
    versions = [p._version for p in ps.params]
    before = _snapshot(ps, opt)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with recording(dev) as events:
            opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    names = [e.split()[0] for e in events]
    assert names == ["cft_adam_step"], names
    assert opt.table_uploads == 1
    assert all(p._version > v for p, v in zip(ps.params, versions))          # Model's caches key on the version counters
    n = len(ps.params)
    _check_step("second step", ps, before, _snapshot(ps, opt), grads, hyp, False, [2.0] * n)
    # a new lr and new betas take effect with the table as it is
    opt.param_groups[1]["lr"] = hyp.lr[1] = 0.5
    opt.param_groups[0]["betas"] = hyp.betas[0] = (0.5, 0.9)
    before = _snapshot(ps, opt)
    opt.step()
    assert opt.table_uploads == 1
    _check_step("new lr and betas", ps, before, _snapshot(ps, opt), grads, hyp, False, [3.0] * n)
    # a gradient set to None drops its parameter from the step
    ps.params[4].grad = None
    before = _snapshot(ps, opt)
    opt.step()
    after = _snapshot(ps, opt)
    assert opt.table_uploads == 2
    assert all(torch.equal(after[k][4], before[k][4]) for k in range(3)) and after[3][4] == 3.0 and after[3][5] == 4.0
    assert not torch.equal(after[0][5], before[0][5])


def test_grad_scaler(dev):
    optim = _mods()[0]
    hyp = _Hyp()
    n = len(_Params(dev, optim.CHUNK).params)

    def start():
        ps = _Params(dev, optim.CHUNK)
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.)
        scaler.scale(torch.zeros(1, device=dev))                               # (creates the scale tensor, as scaler.scale(loss) does)
        return ps, hyp.make(optim.Adam, ps.groups()), scaler

    ps, opt, scaler = start()
    twin_ps, twin, twin_scaler = start()                                       # never sees the skipped step
    before = _snapshot(ps, opt)
    grads = ps.new_grads(0, scale=1024.0)                                      # what backward of the scaled loss leaves
    twin_ps.new_grads(0, scale=1024.0)
    for s, o in ((scaler, opt), (twin_scaler, twin)):
        s.step(o)
        s.update()
    after = _snapshot(ps, opt)
    _check_step("scaled step", ps, before, after, grads, hyp, False, [1.0] * n, grad_scale=1024.0)
    assert scaler.get_scale() == 1024.0 and not hasattr(opt, "grad_scale")
    rng_state = ps.rng.bit_generator.state
    ps.new_grads(3, scale=1024.0)
    ps.rng.bit_generator.state = rng_state                                     # (the twin's stream did not draw these)
    ps.params[7].grad[5] = float("inf")
    scaler.step(opt)
    scaler.update()
    skipped = _snapshot(ps, opt)
    for k in range(3):
        for a, b in zip(after[k], skipped[k]):
            assert torch.equal(a, b)                                            # found_inf: nothing is written
    assert skipped[3] == after[3] == [1.0] * n                                 # ... the step counters included
    assert scaler.get_scale() == 512.0 and twin_scaler.get_scale() == 1024.0
    grads = ps.new_grads(3, scale=512.0)                                       # the same gradients under each scaler's scale: exact in binary
    twin_ps.new_grads(3, scale=1024.0)
    for s, o in ((scaler, opt), (twin_scaler, twin)):
        s.step(o)
        s.update()
    good, want = _snapshot(ps, opt), _snapshot(twin_ps, twin)
    _check_step("the step after the skipped one", ps, skipped, good, grads, hyp, False, [2.0] * n, grad_scale=512.0)
    for k in range(3):
        for a, b in zip(good[k], want[k]):
            assert torch.equal(a, b)
    assert good[3] == want[3] == [2.0] * n


def test_golden_reference_steps(dev, golden):
    optim, _, general = _mods()
    hyp, nw = golden["hyp"], golden["nw"]
    net = R.SmallNet().to(dev)
    opt = optim.build_adam_optimizer(net, hyp)
    lf = general.one_cycle(1, hyp["lrf"], golden["epochs"])
    torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lf)
    names = dict(net.named_parameters())
    group_of = {n: j for j, group in enumerate(golden["groups"]) for n in group}
    assert R.group_names(net, [g["params"] for g in opt.param_groups]) == golden["groups"]
    prev = {"params": {k: v for k, v in R.seeded_state(net, 0).items() if k in names}}
    worst = 0.0
    for k, rec in enumerate(golden["steps"]):
        with torch.no_grad():
            for n, p in names.items():                      # exactly the recorded state before this step
                p.copy_(prev["params"][n])
                if k:
                    opt.state[p]["exp_avg"].copy_(prev["exp_avg"][n])
                    opt.state[p]["exp_avg_sq"].copy_(prev["exp_avg_sq"][n])
                    opt.state[p]["step"] = torch.tensor(prev["step"][n])          # a CPU tensor, as a loaded checkpoint has: adopted
        assert optim.warmup(opt, rec["ni"], nw, golden["epoch"], lf, hyp, golden["nbs"], golden["total_batch_size"]) == rec["accumulate"]
        assert [float(g["lr"]) for g in opt.param_groups] == rec["lr"] and [tuple(g["betas"]) for g in opt.param_groups] == rec["betas"]
        grads = R.seeded_grads(net, k)
        for n, p in names.items():
            p.grad = grads[n].to(dev)
        opt.step()
        for n, p in names.items():
            j = group_of[n]
            b = A.adam_step(prev["params"][n], grads[n], prev["exp_avg"][n] if k else None, prev["exp_avg_sq"][n] if k else None, k + 1,
                            rec["lr"][j], *rec["betas"][j], rec["eps"][j], rec["weight_decay"][j], False)
            st = opt.state[p]
            assert float(st["step"]) == rec["step"][n] == k + 1
            for got, key, bound in ((p, "params", b[3]), (st["exp_avg"], "exp_avg", b[4]), (st["exp_avg_sq"], "exp_avg_sq", b[5])):
                w = A.worst(got, rec[key][n].numpy().astype(np.float64), 2 * bound)
                worst = max(worst, w)
                assert w <= 1.0, (k, n, key, w)
        prev = rec
    print(f"five recorded reference steps: worst |kernel - recording| / (2 * bound): {worst:.3f}")


def _small_model(dev, seed=7):
    from msod_amd.models.configs import cft_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils.seeded import seeded_inputs, seeded_state_dict
    cfg = cft_config("s", "add", 1)
    model = Model(cfg)
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed))
    rgb, ir = seeded_inputs(1, 64, 64, seed)
    return cfg, model.to(dev).eval(), rgb.to(dev), ir.to(dev)


def _seeded_model_grads(model, seed=5):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    for p in model.parameters():
        p.grad = (torch.randn(p.shape, generator=g) * p.detach().abs().mean().cpu()).to(p.device)


def test_resume_from_checkpoint(dev, golden, tmp_path):
    optim, torch_utils, general = _mods()
    from msod_amd import compat
    from msod_amd.models.yolo_test import Model
    cfg, model, x, x2 = _small_model(dev)
    ema = torch_utils.ModelEMA(model)
    opt = optim.build_adam_optimizer(model, golden["hyp"])
    for seed in (5, 6):
        _seeded_model_grads(model, seed)
        opt.step()
    ema.update(model)
    last, best = str(tmp_path / "last.pt"), str(tmp_path / "best.pt")
    general.save_checkpoint(last, 2, 0.1, model, ema, opt, training_results="")
    at_save = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _seeded_model_grads(model, 7)
    opt.step()                                                                  # the uninterrupted run
    ck = torch.load(last, weights_only=False)
    nparams = sum(len(g["params"]) for g in opt.param_groups)
    assert len(ck["optimizer"]["state"]) == nparams and all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in ck["optimizer"]["state"].values())
    assert all(float(v["step"]) == 2.0 for v in ck["optimizer"]["state"].values())
    resumed = Model(cfg).to(dev)
    resumed.load_state_dict(at_save)
    again = optim.build_adam_optimizer(resumed, golden["hyp"])
    again.load_state_dict(ck["optimizer"])
    _seeded_model_grads(resumed, 7)
    again.step()
    for (n, p), q in zip(model.named_parameters(), resumed.parameters()):
        assert torch.equal(p, q), n
        if p in opt.state:
            assert float(again.state[q]["step"]) == float(opt.state[p]["step"]) == 3.0
            assert torch.equal(opt.state[p]["exp_avg"], again.state[q]["exp_avg"]) and torch.equal(opt.state[p]["exp_avg_sq"], again.state[q]["exp_avg_sq"])
    assert again.table_uploads == 1
    general.strip_optimizer(last, best)
    assert torch.load(best, weights_only=False)["optimizer"] is None
    for name in (last, best):
        loaded = compat.attempt_load(name, map_location="cpu").to(dev)
        # what the file holds: the average rounded to half precision, widened again, BatchNorm folded by fuse() on the host
        fresh = Model(cfg)
        fresh.load_state_dict({k: (v.half().float() if v.dtype.is_floating_point else v).cpu() for k, v in ema.ema.state_dict().items()})
        fresh = fresh.float().fuse().eval().to(dev).set_compute_dtype(loaded.compute_dtype)
        with torch.no_grad():
            assert loaded.compute_dtype == torch.float32 and torch.equal(loaded(x, x2)[0], fresh(x, x2)[0]), name


def test_step_invalidates_packed_weights(dev, golden):
    optim = _mods()[0]
    from msod_amd.models.yolo_test import Model
    cfg, model, x, x2 = _small_model(dev)
    with torch.no_grad():
        before = model(x, x2)[0].clone()                      # packed weights exist now
    opt = optim.build_adam_optimizer(model, golden["hyp"])    # lr0 = 0.01: a first Adam step moves every weight by about lr
    _seeded_model_grads(model)
    opt.step()
    with torch.no_grad():
        after = model(x, x2)[0].clone()
    fresh = Model(cfg)
    fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        want = fresh.to(dev).eval()(x, x2)[0]
    assert torch.isfinite(after).all()
    assert not torch.equal(after, before), "the forward still runs the weights of before the step"
    assert torch.equal(after, want)


def test_closed_loop_on_hip_kernels(dev):
    optim = _mods()[0]
    from make_loss_golden import StubModel
    from msod_amd.utils.loss import ComputeLoss
    cases = torch.load(LOSS_GOLDEN, weights_only=False)["cases"]
    c = min((c for c in cases if c["targets"].shape[0] and not c["autobalance"]), key=lambda c: sum(t.numel() for t in c["calls"][0]["p"]))
    p = [t.float().to(dev).requires_grad_() for t in c["calls"][0]["p"]]
    cl = ComputeLoss(StubModel(c["nc"], c["hyp"], c["gr"]).to(dev))
    opt = optim.Adam(p, lr=0.05)
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
    assert all(float(opt.state[t]["step"]) == 10.0 for t in p)
    cl.check()
