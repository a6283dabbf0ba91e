"""GPU tests of the mAP evaluator (csrc/metrics.hip, utils/metrics.py, evaluate.py) against the reference's own test.py
statistics recorded in tests/golden/eval/eval_cases.pt and against the host restatement in tests/eval_ref.py."""
import os

import numpy as np
import pytest
import torch

import eval_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval", "eval_cases.pt")


@pytest.fixture(scope="module")
def cases():
    return torch.load(GOLDEN, weights_only=False)["cases"]


def _metrics():
    import msod_amd  # noqa: F401
    from msod_amd.utils import metrics
    return metrics


def test_match_batch_reproduces_reference_stats(dev, cases):
    m = _metrics()
    for case in cases:
        if case["stats"] is None:
            continue
        stats = []
        for b in case["batches"]:
            dets = [d.to(dev) for d in b["dets"]]
            res = m.match_batch(dets, None, b["targets"], b["img_hw"], b["shapes"], single_cls=case["single_cls"])
            stats.extend(res.to_stats())
        tp, conf, pcls, tcls = [np.concatenate([np.asarray(s[i]) for s in stats], 0) for i in range(4)]
        s = case["stats"]
        assert np.array_equal(tp, s["tp"].numpy()), case["name"]
        assert np.array_equal(conf, s["conf"].numpy()), case["name"]
        assert np.array_equal(pcls, s["pred_cls"].numpy()), case["name"]
        assert np.array_equal(tcls.astype(np.float64), s["target_cls"].numpy()), case["name"]


def test_ap_per_class_reproduces_reference(dev, cases):
    m = _metrics()
    for case in cases:
        if case["stats"] is None:
            continue
        s, want = case["stats"], case["ap_out"]
        p, r, ap, f1, ap_class = m.ap_per_class(s["tp"], s["conf"], s["pred_cls"], s["target_cls"].numpy())
        assert np.array_equal(ap_class, want["ap_class"].numpy()) and ap_class.dtype == np.int32, case["name"]
        for name, got in (("p", p), ("r", r), ("ap", ap), ("f1", f1)):
            np.testing.assert_allclose(got, want[name].numpy(), rtol=0, atol=1e-12, err_msg=f"{case['name']} {name}")


def _run_evaluator(m, case, dev):
    from msod_amd.utils.general import batched_nms
    nc = 1 if case["single_cls"] else case["nc"]
    ev = m.DetectionEvaluator(nc, single_cls=case["single_cls"])
    for b in case["batches"]:
        dets, counts = batched_nms(b["rows"].to(dev), case["conf_thres"], case["iou_thres"], multi_label=True, agnostic=case["single_cls"])
        ev.update(dets, counts, b["targets"].to(dev), b["img_hw"], b["shapes"])
    return ev.compute()


def test_end_to_end_reproduces_test_py(dev, cases):
    m = _metrics()
    for case in cases:
        res = _run_evaluator(m, case, dev)
        got, maps = res.as_test_tuple()
        np.testing.assert_allclose(got, case["results"], rtol=0, atol=1e-12, err_msg=case["name"])
        np.testing.assert_allclose(maps, case["maps"].numpy(), rtol=0, atol=1e-12, err_msg=case["name"])
        assert res.seen == sum(b["rows"].shape[0] for b in case["batches"])
        if case["stats"] is None:
            assert len(res.ap_class) == 0 and torch.equal(res.nt, torch.zeros(1))
        else:
            tc = case["stats"]["target_cls"].numpy().astype(np.int64)
            assert np.array_equal(res.nt, np.bincount(tc, minlength=len(maps)))
            assert np.array_equal(res.ap_class, case["ap_out"]["ap_class"].numpy())


class _RowsModel(torch.nn.Module):
    """Stands in for the network: returns each batch's recorded pre-NMS rows."""

    def __init__(self, rows):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.rows = rows

    def forward(self, x, x2):
        assert x.dtype == torch.uint8 and x.shape[1] == 3 and x2.shape == x.shape
        return self.rows.pop(0), None


def test_evaluate_reproduces_test_py(dev, cases):
    import msod_amd  # noqa: F401
    from msod_amd.evaluate import evaluate
    for case in cases:
        model = _RowsModel([b["rows"].to(dev) for b in case["batches"]]).to(dev)
        loader = [(torch.zeros((b["rows"].shape[0], 6, *b["img_hw"]), dtype=torch.uint8), b["targets"].clone(), None, b["shapes"])
                  for b in case["batches"]]
        got, maps = evaluate(model, loader, case["nc"], single_cls=case["single_cls"])
        np.testing.assert_allclose(got, case["results"], rtol=0, atol=1e-12, err_msg=case["name"])
        np.testing.assert_allclose(maps, case["maps"].numpy(), rtol=0, atol=1e-12, err_msg=case["name"])


def test_large_ap_with_ties_matches_host_oracle(dev):
    m = _metrics()
    g = np.random.default_rng(5)
    n, nc = 5000 * 300, 80
    target_cls = g.integers(0, nc - 3, 5000 * 20).astype(np.float64)          # classes 77-79 have no labels
    pred_cls = g.integers(0, nc, n).astype(np.float32)
    conf = (g.integers(1, 2000, n) / 2000.0).astype(np.float32)             # many tied confidences
    iou = g.random(n)
    tp = (iou[:, None] > np.linspace(0.5, 0.95, 10)[None]) & (g.random(n) < 0.4)[:, None]
    got1 = m.ap_per_class(tp, conf, pred_cls, target_cls)
    got2 = m.ap_per_class(tp, conf, pred_cls, target_cls)
    for a, b in zip(got1, got2):
        assert np.array_equal(a, b)                                           # deterministic, bit for bit
    want = eval_ref.ap_per_class(tp, conf, pred_cls, target_cls)
    assert np.array_equal(got1[4], want[4])
    for name, a, b in zip(("p", "r", "ap", "f1"), got1[:4], want[:4]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12, err_msg=name)


def _random_batch(g, B, max_det, nc, H, W, dev):
    dets = torch.zeros((B, max_det, 6))
    counts = torch.from_numpy(g.integers(0, max_det + 1, B).astype(np.int32))
    counts[0] = 0
    tg, shapes = [], []
    for b in range(B):
        h0, w0 = int(g.integers(300, 900)), int(g.integers(300, 900))
        r = min(H / h0, W / w0)
        shapes.append(((h0, w0), ((r, r), ((W - w0 * r) / 2, (H - h0 * r) / 2))) if b % 2 else ((h0, w0), None))
        nl = int(g.integers(0, 30)) if b != 1 else 5
        lab = np.column_stack([g.integers(0, nc, nl), g.uniform(0.2, 0.8, (nl, 2)), g.uniform(0.05, 0.3, (nl, 2))])
        tg += [(b, *l) for l in lab]
        n = int(counts[b])
        k = g.integers(0, max(nl, 1), n)
        if nl:
            cxy = lab[k, 1:3] * [W, H] + g.normal(0, 6, (n, 2))
            wh = lab[k, 3:5] * [W, H] * np.exp(g.normal(0, 0.2, (n, 2)))
            cls = np.where(g.random(n) < 0.8, lab[k, 0], g.integers(0, nc, n))
        else:
            cxy, wh, cls = g.uniform(0, W, (n, 2)), g.uniform(5, 60, (n, 2)), g.integers(0, nc, n)
        d = np.column_stack([cxy - wh / 2, cxy + wh / 2, np.sort(g.random(n))[::-1], cls])
        dets[b, :n] = torch.from_numpy(d.astype(np.float32))
    targets = torch.tensor(tg, dtype=torch.float32).reshape(-1, 6)
    return dets.to(dev), counts.to(dev), targets, shapes


def test_update_no_sync_and_random_batches_match_host(dev):
    m = _metrics()
    g = np.random.default_rng(9)
    nc, H, W = 7, 384, 640
    ev = m.DetectionEvaluator(nc)
    stats = []
    batches = [_random_batch(g, 16, 300, nc, H, W, dev) for _ in range(3)]
    for dets, counts, targets, shapes in batches:
        t_dev = targets.to(dev)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ev.update(dets, counts, t_dev, (H, W), shapes)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        t = targets.numpy()
        cnt = counts.cpu().numpy()
        batch_stats = []
        for si in range(dets.shape[0]):
            d = dets[si, :cnt[si]].cpu().numpy()
            labels = t[t[:, 0] == si, 1:]
            corr, cf, pc, _ = eval_ref.match_image(d, labels, (H, W), shapes[si])
            if len(d) or len(labels):
                batch_stats.append((corr, cf, pc, labels[:, 0]))
        stats.extend(batch_stats)
        got = m.match_batch(dets, counts, targets, (H, W), shapes).to_stats()
        assert len(got) == len(batch_stats)
        for (gc, gf, gp, gt), (wc, wf, wp, wt) in zip(got, batch_stats):
            assert np.array_equal(np.asarray(gc).reshape(wc.shape), wc) and np.array_equal(np.asarray(gf), wf)
            assert np.array_equal(np.asarray(gp), wp) and np.array_equal(np.asarray(gt, np.float32), wt)
    tp, conf, pcls = (np.concatenate([s[i] for s in stats]) for i in range(3))
    tcls = np.concatenate([s[3] for s in stats]).astype(np.float64)
    got, maps = ev.compute().as_test_tuple()
    want, wmaps, _, _ = eval_ref.test_results(tp, conf, pcls, tcls, nc)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(maps, wmaps, rtol=0, atol=1e-12)


def test_edge_cases(dev):
    m = _metrics()
    shapes = [((100, 120), None)] * 3
    dets = torch.zeros((3, 300, 6), device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    # all counts zero, no labels
    ev = m.DetectionEvaluator(3)
    ev.update(dets, counts, torch.zeros((0, 6)), (64, 96), shapes)
    res = ev.compute()
    assert res.as_test_tuple()[0] == (0.0,) * 5 and res.seen == 3 and len(res.ap_class) == 0
    assert m.match_batch(dets, counts, torch.zeros((0, 6)), (64, 96), shapes).to_stats() == []
    # labels on images without detections
    targets = torch.tensor([[0, 1, 0.5, 0.5, 0.2, 0.2], [2, 0, 0.3, 0.3, 0.1, 0.1]])
    st = m.match_batch(dets, counts, targets, (64, 96), shapes).to_stats()
    assert len(st) == 2 and st[0][0].shape == (0, 10) and st[0][3] == [1.0] and st[1][3] == [0.0]
    ev.update(dets, counts, targets, (64, 96), shapes)
    res = ev.compute()
    assert res.as_test_tuple()[0] == (0.0,) * 5 and torch.equal(res.nt, torch.zeros(1))
    # an evaluator that saw nothing
    assert m.DetectionEvaluator(2).compute().as_test_tuple()[0] == (0.0,) * 5
    # labels of a class outside [0, nc) are an error, not a silent drop
    ev = m.DetectionEvaluator(2)
    ev.update(dets, counts, torch.tensor([[0, 5, 0.5, 0.5, 0.2, 0.2]]), (64, 96), shapes)
    with pytest.raises(ValueError, match="outside"):
        ev.compute()
    # more labels in one image than the LDS holds: the global-memory path gives the same matches as the host
    g = np.random.default_rng(3)
    nl = 1500
    lab = np.column_stack([np.zeros(nl), g.uniform(0.1, 0.9, (nl, 2)), g.uniform(0.01, 0.05, (nl, 2))])
    targets = torch.from_numpy(np.column_stack([np.zeros(nl), lab]).astype(np.float32))
    cxy = lab[:300, 1:3] * [96, 64] + g.normal(0, 0.3, (300, 2))
    wh = lab[:300, 3:5] * [96, 64]
    d = np.column_stack([cxy - wh / 2, cxy + wh / 2, np.linspace(0.9, 0.1, 300), np.zeros(300)]).astype(np.float32)
    dd = torch.zeros((1, 300, 6))
    dd[0] = torch.from_numpy(d)
    res = m.match_batch(dd.to(dev), torch.tensor([300], dtype=torch.int32, device=dev), targets, (64, 96), shapes[:1])
    want, _, _, _ = eval_ref.match_image(d, lab, (64, 96), shapes[0])
    assert want[:, 0].sum() > 100
    assert np.array_equal(res.correct[0].cpu().numpy(), want)
