"""GPU tests of the confusion matrix (cft_eval_confusion), the save_txt / save_hybrid / save_json export (cft_eval_export) and the
evaluate() options built on them, against the reference's own results in tests/golden/eval/confusion_cases.pt and against the host
restatement in tests/confusion_ref.py.  Counts and file texts are compared exactly: the counts are integers, and every exported
value is a chain of single correctly rounded float32 operations in the reference's order."""
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import confusion_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval", "confusion_cases.pt")
EVAL_GOLDEN = os.path.join(ROOT, "tests", "golden", "eval", "eval_cases.pt")


@pytest.fixture(scope="module")
def cases():
    return torch.load(GOLDEN, weights_only=False)["cases"]


def _metrics():
    import msod_amd  # noqa: F401
    from msod_amd.utils import metrics
    return metrics


class _RowsModel(torch.nn.Module):
    """Stands in for the network: returns each batch's recorded pre-NMS rows."""

    def __init__(self, rows):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.rows = list(rows)

    def forward(self, x, x2):
        return self.rows.pop(0), None


def _evaluate(case, dev, **kw):
    import msod_amd  # noqa: F401
    from msod_amd.evaluate import evaluate
    model = _RowsModel([b["rows"].to(dev) for b in case["batches"]]).to(dev)
    loader = [(torch.zeros((b["rows"].shape[0], 6, *b["img_hw"]), dtype=torch.uint8), b["targets"].clone(), b.get("paths"), b["shapes"])
              for b in case["batches"]]
    return evaluate(model, loader, case["nc"], conf_thres=case["conf_thres"], iou_thres=case["iou_thres"], single_cls=case["single_cls"], **kw)


def _nc(case):
    return 1 if case["single_cls"] else case["nc"]


def test_evaluate_confusion_reproduces_reference_matrix(dev, cases):
    for case in cases:
        res = _evaluate(case, dev, confusion=True)
        assert len(res) == 3 and res[2]["jdict"] is None
        got, want = res[2]["confusion_matrix"], case["matrix"].numpy()
        print(case["name"], "evaluate(confusion=True) matrix\n", got, "\nreference\n", want)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got, want), case["name"]


def test_process_batch_loop_reproduces_reference_matrix(dev, cases):
    m = _metrics()
    for case in cases:
        cm = m.ConfusionMatrix(_nc(case))
        assert cm.conf == 0.25 and cm.iou_thres == 0.45 and cm.nc == _nc(case)
        for det, lab in case["process_batch"]:
            cm.process_batch(det.to(dev), lab.to(dev))
        got = cm.matrix
        print(case["name"], "process_batch loop matrix\n", got)
        assert np.array_equal(got, case["matrix"].numpy()), case["name"]


def test_accumulation_equals_sum_of_batches(dev, cases):
    m = _metrics()
    from msod_amd.utils.general import batched_nms
    for case in cases:
        nc = _nc(case)
        total = m.ConfusionMatrix(nc)
        parts = np.zeros((nc + 1, nc + 1))
        for b in case["batches"]:
            dets, counts = batched_nms(b["rows"].to(dev), case["conf_thres"], case["iou_thres"], multi_label=True, agnostic=case["single_cls"])
            total.update(dets, counts, b["targets"], b["img_hw"], b["shapes"], case["single_cls"])
            one = m.ConfusionMatrix(nc)
            one.update(dets, counts, b["targets"].to(dev), b["img_hw"], b["shapes"], case["single_cls"])
            want, bad = confusion_ref.batch_matrix([d.numpy() for d in b["dets"]], b["targets"].numpy(), b["img_hw"], b["shapes"], nc,
                                                   single_cls=case["single_cls"])
            assert bad == 0 and np.array_equal(one.matrix, want.astype(np.float64)), case["name"]
            parts += one.matrix
        assert np.array_equal(total.matrix, parts), case["name"]
        assert np.array_equal(total.matrix, case["matrix"].numpy()), case["name"]


def _read_labels(d):
    return {f.stem: f.read_text() for f in sorted((Path(d) / "labels").glob("*.txt"))}


def _first_difference(got, want):
    for k in sorted(set(got) | set(want)):
        if got.get(k) != want.get(k):
            return f"{k}:\n got  {got.get(k)!r}\n want {want.get(k)!r}"
    return ""


def test_save_txt_files_equal_reference(dev, cases, tmp_path):
    for case in cases:
        for key, kw in (("txt_conf", dict(save_txt=True, save_conf=True)), ("txt", dict(save_txt=True)),
                        ("hybrid", dict(save_hybrid=True, save_conf=True))):
            d = tmp_path / f"{case['name']}_{key}"
            res = _evaluate(case, dev, save_dir=d, **kw)
            assert len(res) == 3
            got = _read_labels(d)
            assert got == case[key], f"{case['name']} {key}: {_first_difference(got, case[key])}"


def test_save_json_equals_reference(dev, cases, tmp_path):
    import json
    for case in cases:
        d = tmp_path / f"{case['name']}_json"
        _, _, extras = _evaluate(case, dev, save_json=True, save_dir=d)
        got, want = extras["jdict"], case["jdict"]
        assert len(got) == len(want), case["name"]
        for g, w in zip(got, want):
            assert g == w and type(g["image_id"]) is type(w["image_id"]), f"{case['name']}: {g} != {w}"
        assert json.load(open(d / "predictions.json")) == want
        assert extras["confusion_matrix"] is None


def _tie_batch(dev):
    """Two images of multi-label duplicates: identical boxes carrying two classes, both above 0.25, on identical labels."""
    nc, H, W = 3, 128, 128
    shapes = [((128, 128), None)] * 3
    # image 0: two identical labels (classes 0, 1) under three identical detections (classes 2, 0, 1) and a duplicate pair elsewhere;
    # image 1: one label under two identical detections; a far label; image 2: detections only (does not contribute)
    d0 = [[10, 10, 60, 60, 0.9, 2], [10, 10, 60, 60, 0.8, 0], [10, 10, 60, 60, 0.7, 1], [70, 70, 120, 120, 0.6, 1], [70, 70, 120, 120, 0.5, 0]]
    d1 = [[20, 20, 80, 80, 0.9, 1], [20, 20, 80, 80, 0.85, 2], [20, 20, 80, 80, 0.2, 0]]
    d2 = [[5, 5, 50, 50, 0.9, 1]]
    dets = [torch.tensor(d, dtype=torch.float32) for d in (d0, d1, d2)]
    box = lambda x1, y1, x2, y2: [(x1 + x2) / 2 / W, (y1 + y2) / 2 / H, (x2 - x1) / W, (y2 - y1) / H]  # noqa: E731
    targets = torch.tensor([[0, 0, *box(10, 10, 60, 60)], [0, 1, *box(10, 10, 60, 60)], [0, 2, *box(70, 70, 120, 120)],
                            [1, 2, *box(20, 20, 80, 80)], [1, 0, *box(90, 90, 120, 120)]], dtype=torch.float32)
    return nc, (H, W), shapes, dets, targets


def test_ties_follow_the_documented_rule(dev):
    m = _metrics()
    nc, hw, shapes, dets, targets = _tie_batch(dev)
    want, bad = confusion_ref.batch_matrix([d.numpy() for d in dets], targets.numpy(), hw, shapes, nc)
    assert bad == 0
    # image 0: detection 0 (class 2) is label 0's match, label 1 is background, detections 1, 2 are left over; the pair at (70, 70)
    # goes to detection 3 (class 1); image 1: detection 0 (class 1) matches the class-2 label, detection 1 is left over
    exp = np.zeros((4, 4), np.int64)
    exp[2, 0] += 1; exp[3, 1] += 1; exp[0, 3] += 1; exp[1, 3] += 1; exp[1, 2] += 1; exp[0, 3] += 1      # noqa: E702
    exp[1, 2] += 1; exp[2, 3] += 1; exp[3, 0] += 1                                                         # noqa: E702
    assert np.array_equal(want, exp)
    runs = []
    for _ in range(2):
        cm = m.ConfusionMatrix(nc)
        cm.update([d.to(dev) for d in dets], None, targets, hw, shapes)
        runs.append(cm.matrix)
    print("tie case\n", runs[0])
    assert np.array_equal(runs[0], want.astype(np.float64))
    assert np.array_equal(runs[0], runs[1])
    t = targets.numpy()
    labels = t[t[:, 0] < 2]                                                  # images 0 and 1 contribute
    for c in range(nc):
        assert runs[0][:, c].sum() == (labels[:, 1] == c).sum()


def test_bad_class_raises_and_the_other_images_count(dev):
    m = _metrics()
    nc, hw, shapes, dets, targets = _tie_batch(dev)
    good, _ = confusion_ref.batch_matrix([d.numpy() for d in dets], targets.numpy(), hw, shapes, nc)
    only1, _ = confusion_ref.batch_matrix([dets[0][:0].numpy(), dets[1].numpy(), dets[2].numpy()], targets.numpy(), hw, shapes, nc)
    # a label class outside [0, nc) in image 0
    bad_t = targets.clone()
    bad_t[0, 1] = 7
    cm = m.ConfusionMatrix(nc)
    cm.update([d.to(dev) for d in dets], None, bad_t, hw, shapes)
    with pytest.raises(ValueError, match="outside"):
        cm.matrix
    counted = cm._m.cpu().numpy()
    want, skipped = confusion_ref.batch_matrix([d.numpy() for d in dets], bad_t.numpy(), hw, shapes, nc)
    assert skipped == 1 and np.array_equal(counted, want)
    assert counted.sum() == good.sum() - 1 and (counted >= only1).all() and only1.sum() > 0      # image 1 still counts in full
    # a detection class outside [0, nc)
    bad_d = [d.clone() for d in dets]
    bad_d[1][1, 5] = -3
    cm = m.ConfusionMatrix(nc)
    cm.update([d.to(dev) for d in bad_d], None, targets, hw, shapes)
    with pytest.raises(ValueError, match="detections"):
        cm.matrix
    want, skipped = confusion_ref.batch_matrix([d.numpy() for d in bad_d], targets.numpy(), hw, shapes, nc)
    assert skipped == 1 and np.array_equal(cm._m.cpu().numpy(), want)
    # through the evaluator
    ev = m.DetectionEvaluator(nc, confusion=True)
    ev.update([d.to(dev) for d in bad_d], None, targets, hw, shapes)
    with pytest.raises(ValueError, match="outside"):
        ev.compute()


def test_default_path_is_unchanged(dev):
    m = _metrics()
    from msod_amd.utils.general import batched_nms
    for case in torch.load(EVAL_GOLDEN, weights_only=False)["cases"]:
        nc = _nc(case)
        ev = m.DetectionEvaluator(nc, single_cls=case["single_cls"])
        for b in case["batches"]:
            dets, counts = batched_nms(b["rows"].to(dev), case["conf_thres"], case["iou_thres"], multi_label=True, agnostic=case["single_cls"])
            ev.update(dets, counts, b["targets"], b["img_hw"], b["shapes"])
        res = ev.compute()
        want, wmaps = res.as_test_tuple()
        assert res.confusion_matrix is None
        out = _evaluate(case, dev)
        assert len(out) == 2
        assert out[0] == want and np.array_equal(out[1], wmaps), case["name"]
        # the new options do not change the metrics either
        with_cm = _evaluate(case, dev, confusion=True)
        assert with_cm[0] == want and np.array_equal(with_cm[1], wmaps), case["name"]


def test_update_with_confusion_does_not_synchronise(dev, cases):
    m = _metrics()
    from msod_amd.utils.general import batched_nms
    case = cases[2]
    nc = _nc(case)
    ev = m.DetectionEvaluator(nc, confusion=True)
    m.ConfusionMatrix(nc).update(*batched_nms(case["batches"][0]["rows"].to(dev), 0.001, 0.6, multi_label=True), case["batches"][0]["targets"],
                                 case["batches"][0]["img_hw"], case["batches"][0]["shapes"])       # library loaded, kernels resident
    for b in case["batches"]:
        dets, counts = batched_nms(b["rows"].to(dev), case["conf_thres"], case["iou_thres"], multi_label=True, agnostic=False)
        for targets in (b["targets"].to(dev), b["targets"]):
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                ev.update(dets, counts, targets, b["img_hw"], b["shapes"])
            finally:
                torch.cuda.set_sync_debug_mode("default")
    res = ev.compute()
    assert np.array_equal(res.confusion_matrix, 2 * case["matrix"].numpy())      # every batch went in twice


def test_export_matches_host_restatement(dev, cases):
    m = _metrics()
    for case in cases:
        for b in case["batches"]:
            n = [len(d) for d in b["dets"]]
            dets = torch.zeros((len(n), max(1, max(n)), 6))
            for i, d in enumerate(b["dets"]):
                dets[i, :n[i]] = d
            out = m.export_batch(dets.to(dev), torch.tensor(n, dtype=torch.int32, device=dev), b["img_hw"], b["shapes"], case["single_cls"]).cpu().numpy()
            for i, d in enumerate(b["dets"]):
                cls, conf, nxywh, tl = confusion_ref.export_values(d.numpy(), b["img_hw"], b["shapes"][i], case["single_cls"])
                assert out[i, :, 6].sum() == n[i] and not out[i, n[i]:].any()
                assert np.array_equal(out[i, :n[i], 4], conf) and np.array_equal(out[i, :n[i], 5], cls)
                assert np.array_equal(out[i, :n[i], 8:12], nxywh) and np.array_equal(out[i, :n[i], 12:16], tl)


def test_many_labels_and_empty_inputs(dev):
    m = _metrics()
    # more labels in one image than the LDS holds
    g = np.random.default_rng(4)
    nl, nc = 1500, 4
    lab = np.column_stack([g.integers(0, nc, nl), g.uniform(0.1, 0.9, (nl, 2)), g.uniform(0.01, 0.05, (nl, 2))])
    targets = torch.from_numpy(np.column_stack([np.zeros(nl), lab]).astype(np.float32))
    cxy = lab[:300, 1:3] * [96, 64] + g.normal(0, 0.3, (300, 2))
    wh = lab[:300, 3:5] * [96, 64]
    d = np.column_stack([cxy - wh / 2, cxy + wh / 2, np.linspace(0.9, 0.1, 300), g.integers(0, nc, 300)]).astype(np.float32)
    shapes = [((100, 120), None)]
    want, bad = confusion_ref.batch_matrix([d], targets.numpy(), (64, 96), shapes, nc)
    assert bad == 0 and want[:nc, :nc].sum() > 50
    cm = m.ConfusionMatrix(nc)
    cm.update([torch.from_numpy(d).to(dev)], None, targets, (64, 96), shapes)
    assert np.array_equal(cm.matrix, want.astype(np.float64))
    # nothing seen, no labels, no detections
    assert not m.ConfusionMatrix(2).matrix.any() and m.ConfusionMatrix(2).matrix.shape == (3, 3)
    cm = m.ConfusionMatrix(2)
    cm.update(torch.zeros((2, 300, 6), device=dev), torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros((0, 6)), (64, 96), shapes * 2)
    cm.update(torch.zeros((2, 300, 6), device=dev), torch.zeros(2, dtype=torch.int32, device=dev),
              torch.tensor([[0, 1, 0.5, 0.5, 0.2, 0.2]]), (64, 96), shapes * 2)
    assert not cm.matrix.any()
    # process_batch without detections counts the labels as background, as the reference's method does
    cm.process_batch(torch.zeros((0, 6), device=dev), torch.tensor([[1, 0, 0, 5, 5]], dtype=torch.float32, device=dev))
    assert cm.matrix[2, 1] == 1 and cm.matrix.sum() == 1


def test_plot_and_print(dev, cases, tmp_path, capsys):
    m = _metrics()
    cm = m.ConfusionMatrix(3)
    for det, lab in cases[0]["process_batch"]:
        cm.process_batch(det.to(dev), lab.to(dev))
    cm.print()
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines == [' '.join(map(str, row)) for row in cases[0]["matrix"].numpy()]
    cm.plot(save_dir=tmp_path, names=["a", "b", "c"])
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    assert (tmp_path / "confusion_matrix.png").stat().st_size > 0
    cm.plot(save_dir=tmp_path / "missing" / "dir", names=["a", "b", "c"])        # silent, as the reference's try / except
