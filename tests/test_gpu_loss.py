"""GPU tests of ComputeLoss (csrc/loss.hip, utils/loss.py) and of evaluate(..., compute_loss=...) against the reference's own
ComputeLoss and test.test() recorded in tests/golden/loss/loss_cases.pt, and against the float64 restatement in tests/loss_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

import loss_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss", "loss_cases.pt")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_loss_golden import StubModel, unpack_grad  # noqa: E402

HYP = dict(box=0.05, obj=1.0, cls=0.5, cls_pw=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def _loss_mod():
    import msod_amd  # noqa: F401
    from msod_amd.utils import loss
    return loss


def _grad_ok(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = 1e-5 * np.abs(want) + 1e-6 * np.abs(want).max()
    bad = np.abs(got - want) > tol
    return not bad.any(), float((np.abs(got - want) / np.maximum(tol, 1e-300)).max())


def _stub(nc, hyp, gr, dev, outputs=()):
    return StubModel(nc, hyp, gr, outputs).to(dev)


def _run(cl, p, targets, grad=True):
    p = [t.detach().clone().requires_grad_(grad) for t in p]
    loss, items = cl(p, targets)
    grads = None
    if grad:
        loss.backward()
        grads = [t.grad for t in p]
    return loss, items, grads


def test_candidate_lists_equal_reference(dev, golden):
    L = _loss_mod()
    for c in golden["cases"]:
        cl = L.ComputeLoss(_stub(c["nc"], c["hyp"], c["gr"], dev))
        for k, call in enumerate(c["calls"]):
            p = [t.float().to(dev) for t in call["p"]]
            tcls, tbox, indices, anch = cl.build_targets(p, c["targets"].to(dev))
            for i, bt in enumerate(call["bt"]):
                what = f"{c['name']} call {k} level {i}"
                for name, got in zip(("b", "a", "gj", "gi"), indices[i]):
                    assert torch.equal(got.cpu(), bt[name]), f"{what} {name}"
                if c["nc"] > 1:
                    assert torch.equal(tcls[i].cpu(), bt["c"]), what
                assert torch.equal(tbox[i].cpu(), bt["tbox"]), what
                assert torch.equal(anch[i].cpu(), bt["anch"]), what


def test_values_and_gradients_match_reference_and_restatement(dev, golden):
    L = _loss_mod()
    for c in golden["cases"]:
        cl = L.ComputeLoss(_stub(c["nc"], c["hyp"], c["gr"], dev), autobalance=c["autobalance"])
        bal = [4.0, 1.0, 0.4]
        for k, call in enumerate(c["calls"]):
            what = f"{c['name']} call {k}"
            p = [t.float().to(dev) for t in call["p"]]
            ref = loss_ref.compute([t.float() for t in call["p"]], c["targets"], c["anchors"], c["hyp"], c["gr"], bal,
                                   c["autobalance"], ssi=1)
            bal = ref["balance"]
            loss, items, grads = _run(cl, p, c["targets"])
            assert loss.shape == (1,) and items.shape == (4,), what
            items = items.cpu().double().numpy()
            np.testing.assert_allclose(items, call["items"].double().numpy(), rtol=1e-5, atol=1e-7, err_msg=what)
            np.testing.assert_allclose(items, ref["items"], rtol=1e-6, atol=1e-8, err_msg=what)
            np.testing.assert_allclose(loss.item(), call["loss"].item(), rtol=1e-5, err_msg=what)
            np.testing.assert_allclose(loss.item(), ref["loss"], rtol=1e-6, err_msg=what)
            np.testing.assert_allclose(cl.balance, call["balance"], rtol=1e-6, err_msg=what)
            for i, (g, gd, gr) in enumerate(zip(grads, call["grads"], ref["grads"])):
                ok, r = _grad_ok(g.cpu().numpy(), unpack_grad(gd).numpy())
                assert ok, f"{what} level {i}: gradient vs reference, worst {r:.3g} x tolerance"
                ok, r = _grad_ok(g.cpu().numpy(), gr)
                assert ok, f"{what} level {i}: gradient vs restatement, worst {r:.3g} x tolerance"
        cl.check()


def _random_case(g, B, hw, nc, nt, dev):
    p = [torch.from_numpy((g.standard_normal((B, 3, hw // s, hw // s, nc + 5)) * 1.5).astype(np.float32)).to(dev) for s in (8, 16, 32)]
    t = np.stack([g.integers(0, B, nt), g.integers(0, nc, nt), g.uniform(0, 1, nt), g.uniform(0, 1, nt), g.uniform(0.005, 0.6, nt),
                  g.uniform(0.005, 0.6, nt)], 1).astype(np.float32)
    t[: nt // 20, 2] = 1.0                                  # some at the far border (the clamp)
    t[nt // 20: nt // 10, 3] = 0.0
    return p, torch.from_numpy(t)


@pytest.mark.parametrize("B,hw,nc,nt", [(64, 640, 3, 4000), (8, 320, 80, 1500)])
def test_random_cases_match_restatement(dev, golden, B, hw, nc, nt):
    L = _loss_mod()
    g = np.random.default_rng(B + nc)
    p, t = _random_case(g, B, hw, nc, nt, dev)
    hyp = dict(HYP, label_smoothing=0.05) if nc == 80 else HYP
    cl = L.ComputeLoss(_stub(nc, hyp, 1.0, dev))
    loss, items, grads = _run(cl, p, t.to(dev))
    ref = loss_ref.compute([x.cpu() for x in p], t, golden["cases"][0]["anchors"], hyp, 1.0, [4.0, 1.0, 0.4])
    np.testing.assert_allclose(items.cpu().double().numpy(), ref["items"], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(loss.item(), ref["loss"], rtol=1e-6)
    for i, (gg, gr) in enumerate(zip(grads, ref["grads"])):
        ok, r = _grad_ok(gg.cpu().numpy(), gr)
        assert ok, f"level {i}: worst {r:.3g} x tolerance"
    # determinism: a second run is bit-identical
    loss2, items2, grads2 = _run(cl, p, t.to(dev))
    assert torch.equal(items, items2) and torch.equal(loss, loss2)
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2))


def test_graph_capture_equals_eager(dev, golden):
    """Forward plus backward (loss_and_grads: the kernels of __call__ + backward, no autograd graph) captured in a
    torch.cuda.graph and replayed equals eager bit for bit, and eager equals the autograd path."""
    L = _loss_mod()
    g = np.random.default_rng(5)
    p, t = _random_case(g, 16, 320, 3, 800, dev)
    t = t.to(dev)
    cl = L.ComputeLoss(_stub(3, dict(HYP, fl_gamma=1.5), 0.5, dev))
    ps = [x.clone() for x in p]

    def step():
        loss, items, grads = cl.loss_and_grads(ps, t)
        return (loss, items, *grads)

    eager = [x.clone() for x in step()]
    loss, items, grads = _run(cl, p, t)
    assert all(torch.equal(a, b) for a, b in zip(eager, (loss.detach(), items, *grads)))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, out))
    for x, y in zip(ps, p):
        x.copy_(y * 0.5)
    graph.replay()
    want = [x.clone() for x in step()]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, out))


def test_no_host_synchronisation(dev):
    L = _loss_mod()
    g = np.random.default_rng(6)
    p, t = _random_case(g, 8, 320, 3, 500, dev)
    cl = L.ComputeLoss(_stub(3, HYP, 1.0, dev), autobalance=True)
    ps = [x.clone().requires_grad_(True) for x in p]
    td = t.to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, items = cl(ps, td)
        loss.backward()
        loss2, items2 = cl(p, t)                       # host targets, no graph
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert loss.requires_grad and not loss2.requires_grad
    cl.check()


def test_bad_targets_are_skipped_and_reported(dev):
    L = _loss_mod()
    g = np.random.default_rng(7)
    p, t = _random_case(g, 4, 128, 3, 40, dev)
    t[3, 0] = 4.0           # image index == B
    t[5, 0] = -3.0
    t[7, 1] = 3.0           # class == nc
    cl = L.ComputeLoss(_stub(3, HYP, 1.0, dev))
    loss, items, grads = _run(cl, p, t.to(dev))
    ref = loss_ref.compute([x.cpu() for x in p], t, StubModel(3, HYP, 1.0).model[-1].anchors, HYP, 1.0, [4.0, 1.0, 0.4])
    assert ref["err"] == 3
    np.testing.assert_allclose(items.cpu().double().numpy(), ref["items"], rtol=1e-6, atol=1e-8)
    with pytest.raises(ValueError, match="image index"):
        cl.check()
    cl.check()              # cleared


def test_real_model_outputs(dev):
    """ComputeLoss on the raw list of a real Model forward (synthetic yolov5s x3 weights), training and eval mode."""
    from msod_amd import ops
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils.seeded import seeded_inputs, seeded_state_dict
    L = _loss_mod()
    c = torch.load(os.path.join(ROOT, "tests", "golden", "s_x3_train_96.pt"), weights_only=False)["case"]
    model = Model(named_config(c["cfg"]))
    model.load_state_dict(seeded_state_dict(model.state_dict(), c["seed"]))
    model = model.to(dev).set_compute_dtype(torch.float32)
    model.hyp, model.gr = dict(HYP), 1.0
    rgb, ir = seeded_inputs(2, 128, 128, c["seed"])
    g = np.random.default_rng(8)
    nc = model.model[-1].nc
    t = torch.from_numpy(np.stack([g.integers(0, 2, 30), g.integers(0, nc, 30), g.uniform(0, 1, 30), g.uniform(0, 1, 30),
                                   g.uniform(0.02, 0.5, 30), g.uniform(0.02, 0.5, 30)], 1).astype(np.float32))
    cl = L.ComputeLoss(model)
    for mode in ("train", "eval"):
        getattr(model, mode)()
        with torch.no_grad():
            ops.manual_dropout_seed(3)
            out = model(rgb.to(dev), ir.to(dev))
        raws = out if mode == "train" else out[1]
        loss, items, grads = _run(cl, raws, t.to(dev))
        ref = loss_ref.compute([r.cpu() for r in raws], t, model.model[-1].anchors, HYP, 1.0, [4.0, 1.0, 0.4])
        np.testing.assert_allclose(items.cpu().double().numpy(), ref["items"], rtol=1e-6, atol=1e-8, err_msg=mode)
        for gg, gr in zip(grads, ref["grads"]):
            assert _grad_ok(gg.cpu().numpy(), gr)[0], mode


def test_evaluate_with_compute_loss_reproduces_test_py(dev, golden):
    import msod_amd  # noqa: F401
    from msod_amd.evaluate import evaluate
    L = _loss_mod()
    e = golden["end_to_end"]
    H, W = e["img_hw"]

    def run(with_loss):
        outputs = [(b["rows"].to(dev), [r.float().to(dev) for r in b["raws"]]) for b in e["batches"]]
        model = _stub(e["nc"], e["hyp"], e["gr"], dev, outputs)
        loader = [(torch.zeros((b["rows"].shape[0], 6, H, W), dtype=torch.uint8), b["targets"].clone(), None, b["shapes"])
                  for b in e["batches"]]
        return evaluate(model, loader, e["nc"], compute_loss=L.ComputeLoss(model) if with_loss else None)

    res, maps = run(True)
    assert len(res) == 8
    np.testing.assert_allclose(res[:5], e["results"][:5], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res[5:], e["results"][5:], rtol=1e-5)
    np.testing.assert_allclose(maps, e["maps"].numpy(), rtol=0, atol=1e-12)
    res0, maps0 = run(False)
    assert len(res0) == 5 and list(res0) == list(res[:5])
    assert np.array_equal(maps0, maps)
