"""CPU tests of the mAP evaluator: the host restatement (tests/eval_ref.py) reproduces the reference's own test.py statistics
recorded in tests/golden/eval/eval_cases.pt, the fixture covers the rules that matter, the Python layer fails loudly without a GPU
and on bad arguments, and every new kernel runs without scratch memory."""
import os
import re

import numpy as np
import pytest
import torch

import eval_ref
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval", "eval_cases.pt")
SRC = os.path.join(ROOT, "multispectral-object-detection_amd", "csrc", "metrics.hip")


@pytest.fixture(scope="module")
def cases():
    return torch.load(GOLDEN, weights_only=False)["cases"]


def _tp_cases(cases):
    return [c for c in cases if c["stats"] is not None]


def test_iouv_matches_torch_linspace():
    assert np.array_equal(eval_ref.IOUV, torch.linspace(0.5, 0.95, 10).numpy())


def test_restated_matching_reproduces_reference(cases):
    for case in _tp_cases(cases):
        tp, conf, pcls, tcls, _, _ = eval_ref.match_case(case)
        s = case["stats"]
        assert np.array_equal(tp, s["tp"].numpy()), case["name"]
        assert np.array_equal(conf, s["conf"].numpy()), case["name"]
        assert np.array_equal(pcls, s["pred_cls"].numpy()), case["name"]
        assert np.array_equal(tcls, s["target_cls"].numpy()), case["name"]


def test_restated_ap_per_class_reproduces_reference(cases):
    for case in _tp_cases(cases):
        s, want = case["stats"], case["ap_out"]
        p, r, ap, f1, ap_class = eval_ref.ap_per_class(s["tp"].numpy(), s["conf"].numpy(), s["pred_cls"].numpy(), s["target_cls"].numpy())
        assert np.array_equal(ap_class, want["ap_class"].numpy()), case["name"]
        for name, got in (("p", p), ("r", r), ("ap", ap), ("f1", f1)):
            np.testing.assert_allclose(got, want[name].numpy(), rtol=0, atol=1e-12, err_msg=f"{case['name']} {name}")


def test_restated_results_reproduce_test_py(cases):
    for case in cases:
        tp, conf, pcls, tcls, _, _ = eval_ref.match_case(case)
        nc = 1 if case["single_cls"] else case["nc"]
        res, maps, nt, ap_class = eval_ref.test_results(tp, conf, pcls, tcls, nc)
        np.testing.assert_allclose(res, case["results"], rtol=0, atol=1e-12, err_msg=case["name"])
        np.testing.assert_allclose(maps, case["maps"].numpy(), rtol=0, atol=1e-12, err_msg=case["name"])
        if case["stats"] is None:
            assert ap_class.size == 0 and np.array_equal(nt, np.zeros(1))


def test_fixture_covers_the_rules(cases):
    assert {c["nc"] for c in cases} >= {1, 3, 9}
    assert any(c["single_cls"] for c in cases)
    assert any(c["stats"] is None for c in cases)                     # no TP at all
    shapes = [s for c in cases for b in c["batches"] for s in b["shapes"]]
    assert any(s[1] is None for s in shapes) and any(s[1] is not None and s[1][1][0] > 0 for s in shapes)
    assert any(s[1] is not None and s[1][0][0] != 1.0 for s in shapes)   # a real gain
    quirk = all_matched = no_labels = no_dets = unlabelled_pred = 0
    ious = []
    for case in _tp_cases(cases):
        tp, conf, pcls, tcls, infos, per_image = eval_ref.match_case(case)
        for (r, best, bi, was_taken, row_ious, ti) in infos:
            ious.append(bi)
            # the best label is already taken although another label of the class would qualify: the reference does not fall back
            if was_taken and bi > 0.5 and (row_ious > 0.5).sum() > 1:
                quirk += 1
        all_matched += sum(1 for n, nl, m in per_image if nl and m == nl)
        no_labels += sum(1 for n, nl, m in per_image if nl == 0)
        no_dets += sum(1 for n, nl, m in per_image if n == 0)
        unlabelled_pred += int(np.isin(pcls, np.unique(tcls), invert=True).sum())
    assert quirk >= 1 and all_matched >= 1 and no_labels >= 1 and no_dets >= 1 and unlabelled_pred >= 1, \
        (quirk, all_matched, no_labels, no_dets, unlabelled_pred)
    ious = np.array(ious)
    assert ious[ious > 0].min() < 0.4 and ious.max() > 0.95
    for case in cases:                                                 # confidences are distinct within a case
        confs = torch.cat([d[:, 4] for b in case["batches"] for d in b["dets"]])
        assert confs.unique().numel() == confs.numel(), case["name"]
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_interp_restatement_matches_numpy():
    g = np.random.default_rng(0)
    xp = np.sort(g.choice(np.linspace(0, 1, 40), 60))                  # repeated xp values
    fp = g.random(60)
    x = np.concatenate([g.uniform(-0.2, 1.2, 500), xp])
    assert np.array_equal(eval_ref.interp(x, xp, fp, left=0), np.interp(x, xp, fp, left=0))


def test_python_layer_fails_loudly(monkeypatch):
    import msod_amd  # noqa: F401
    from msod_amd.utils import metrics
    dets = torch.zeros((2, 300, 6))
    counts = torch.zeros(2, dtype=torch.int32)
    targets = torch.zeros((0, 6))
    shapes = [((100, 100), None)] * 2
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.match_batch(dets, counts, targets, (64, 64), shapes)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.DetectionEvaluator(3).update(dets, counts, targets, (64, 64), shapes)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.match_batch([torch.zeros((0, 6))], None, targets, (64, 64), shapes[:1])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.ap_per_class(np.ones((4, 10), bool), np.ones(4), np.zeros(4), np.zeros(3))
    with pytest.raises(NotImplementedError, match="out of scope"):
        metrics.ap_per_class(np.ones((4, 10), bool), np.ones(4), np.zeros(4), np.zeros(3), plot=True)
    with pytest.raises(ValueError):
        metrics.ap_per_class(np.ones(4, bool), np.ones(4), np.zeros(4), np.zeros(3))
    with pytest.raises(ValueError):
        metrics.ap_per_class(np.ones((4, 10), bool), np.ones(3), np.zeros(4), np.zeros(3))
    with pytest.raises(ValueError):
        metrics.ap_per_class(np.ones((4, 10), bool), np.ones(4), np.zeros(4), np.array([0.5]))
    with pytest.raises(ValueError):
        metrics.DetectionEvaluator(0)


def test_geometry_rounds_like_aten():
    import msod_amd  # noqa: F401
    from msod_amd.utils.metrics import geometry
    shapes = [((480, 640), ((0.4, 0.4), (0.0, 16.0))), ((333, 517), None)]
    g = geometry(shapes, (256, 320)).numpy()
    for i, s in enumerate(shapes):
        assert np.array_equal(g[i], np.array(eval_ref.geometry(s, (256, 320)), np.float32))


def test_eval_kernels_use_no_scratch():
    notes = helpers.kernel_notes(SRC)
    assert len(notes) == len(re.findall(r"__global__", open(SRC).read())) == 10, sorted(notes)
    for name, m in notes.items():
        assert m["private_segment_fixed_size"] == 0, name
        assert m["vgpr_spill_count"] == 0, name
        assert m["sgpr_spill_count"] == 0, name
