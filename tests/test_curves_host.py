"""CPU tests of the validation curves: the host restatement (tests/curves_ref.py) reproduces the arrays the reference's own
ap_per_class(plot=True) handed to its plot functions (tests/golden/eval/curve_cases.pt), the miss rate holds on hand-evaluated cases,
the Python layer fails loudly without a GPU and on bad arguments, and csrc/curves.hip compiles without scratch memory."""
import os
import re

import numpy as np
import pytest
import torch

import curves_ref
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval", "curve_cases.pt")
SRC = os.path.join(ROOT, "multispectral-object-detection_amd", "csrc", "curves.hip")


@pytest.fixture(scope="module")
def cases():
    return torch.load(GOLDEN, weights_only=False)["cases"]


def _metrics():
    import msod_amd  # noqa: F401
    from msod_amd.utils import metrics
    return metrics


def _ref(case, **kw):
    return curves_ref.curves(case["tp"].numpy(), case["conf"].numpy(), case["pred_cls"].numpy(), case["target_cls"].numpy(),
                             case["n_images"], **kw)


def test_fixture_holds_the_cases(cases):
    names = [c["name"] for c in cases]
    assert {"nc3_rect", "nc1_square_nopad", "nc9_rect", "single_cls", "nc3_holes", "nc1_600"} <= set(names)
    holes = cases[names.index("nc3_holes")]
    pc, tc = holes["pred_cls"].numpy(), holes["target_cls"].numpy()
    assert (tc == 1).any() and not (pc == 1).any()                       # labels, no predictions
    assert (pc == 2).any() and not (tc == 2).any()                       # predictions, no labels
    assert holes["py_classes"].tolist() == [0] and holes["ap_class"].tolist() == [0, 1]
    assert cases[names.index("nc1_600")]["conf"].numel() == 600
    for c in cases:                                                      # the reference's argsort is unstable under ties
        assert c["conf"].unique().numel() == c["conf"].numel(), c["name"]
        assert np.array_equal(c["px"].numpy(), curves_ref.PX)
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_restatement_reproduces_reference_curves(cases):
    for case in cases:
        got = _ref(case)
        assert np.array_equal(got.ap_class, case["ap_class"].numpy()), case["name"]
        for name in ("p", "r", "f1"):
            np.testing.assert_allclose(getattr(got, name), case[name].numpy(), rtol=0, atol=1e-12, err_msg=f"{case['name']} {name}")
        rows = np.flatnonzero(np.isin(got.ap_class, case["py_classes"].numpy()))      # the reference has no py row without predictions
        np.testing.assert_allclose(got.py[rows], case["py"].numpy(), rtol=0, atol=1e-12, err_msg=f"{case['name']} py")
        others = np.setdiff1d(np.arange(len(got.ap_class)), rows)
        assert not got.py[others].any()
        assert got.best == case["best"] == int(case["f1"].numpy().mean(0).argmax()), case["name"]


def test_miss_rate_hand_cases():
    ref = curves_ref.FPPI_REF
    assert ref[0] == 0.01 and ref[4] == 0.1 and ref[8] == 1.0 and 1 / 100 == ref[0] and 10 / 100 == ref[4] and 100 / 100 == ref[8]
    # all TP: no false positive ever, the sentinel (fppi -1) is passed at once and the last prediction holds to +inf
    mr = curves_ref.miss_rate(np.ones(5, bool), 5, 10, ref)
    assert np.array_equal(mr, np.zeros(9))
    assert curves_ref.log_average_miss_rate(mr) == pytest.approx(1e-10, rel=1e-12)
    # all FP, and no predictions: every label missed everywhere
    assert np.array_equal(curves_ref.miss_rate(np.zeros(300, bool), 5, 10, ref), np.ones(9))
    assert np.array_equal(curves_ref.miss_rate(np.zeros(0, bool), 5, 10, ref), np.ones(9))
    assert curves_ref.log_average_miss_rate(np.ones(9)) == 1.0
    # n_images = 100, 200 labels; a TP before each of the FPs number 1, 10 and 100: the FP counts land exactly on ref[0], ref[4],
    # ref[8], and `<=` takes the equal point (the TP that FOLLOWS the FP at the same count is included: the LAST index counts)
    tp = np.zeros(150, bool)
    tp[[0, 2, 12, 103]] = True        # tpc: 1 before FP 1; 2 after FP 1; 3 after FP 10 (position 12 = 10 FPs + 2 TPs before it); 4 after FP 100
    fpc = np.cumsum(~tp)
    assert fpc[2] == 1 and fpc[12] == 10 and fpc[103] == 100
    mr = curves_ref.miss_rate(tp, 200, 100, ref)
    want = lambda k: 1.0 - k / (200 + 1e-16)  # noqa: E731
    assert mr[0] == want(2) and mr[4] == want(3) and mr[8] == want(4)
    assert mr[1] == mr[2] == mr[3] == want(2) and mr[5] == want(3)
    # below the first fppi: the sentinel's 1.0, also for a value below the sentinel's own -1
    assert np.array_equal(curves_ref.miss_rate(np.array([True]), 4, 10, [-5.0, -1.0, -0.5, 0.0]), [1.0, 1.0, 1.0, 0.75])
    assert curves_ref.miss_rate(np.array([False, True]), 4, 10, [0.05, 0.1, 0.2])[0] == 1.0
    assert np.array_equal(curves_ref.miss_rate(np.array([False, True]), 4, 10, [0.05, 0.1, 0.2])[1:], [0.75, 0.75])


def test_mr_is_monotone_and_lamr(cases):
    for case in cases:
        got = _ref(case)
        assert np.all(np.diff(got.mr_ref, axis=1) <= 0) and np.all(np.diff(got.mr_curve, axis=1) <= 0), case["name"]
        assert np.all((got.mr_ref >= 0) & (got.mr_ref <= 1))
        assert np.array_equal(got.lamr, np.exp(np.log(np.maximum(1e-10, got.mr_ref)).mean(1)))
        assert got.mlamr == got.lamr.mean()
        if case["name"] == "nc3_holes":
            assert np.array_equal(got.mr_ref[1], np.ones(9)) and got.lamr[1] == 1.0


def test_log_average_miss_rate():
    m = _metrics()
    mr = np.array([[1.0] * 9, [0.0] * 9, [0.5] * 9, np.logspace(0, -2, 9)])
    got = m.log_average_miss_rate(mr)
    np.testing.assert_allclose(got, [1.0, 1e-10, 0.5, 0.1], rtol=1e-12)
    assert np.array_equal(got, curves_ref.log_average_miss_rate(mr))
    assert m.log_average_miss_rate(mr[2]) == pytest.approx(0.5, rel=1e-12)
    assert np.array_equal(m.FPPI_REF, curves_ref.FPPI_REF) and np.array_equal(m.FPPI_PLOT, curves_ref.FPPI_PLOT)


def test_merged_grid_keeps_the_reference_points():
    m = _metrics()
    plot, merged, ref_at, plot_at = m._fppi_grids(None)
    assert merged.size == 1009 and np.all(np.diff(merged) >= 0)
    assert np.array_equal(merged[ref_at], m.FPPI_REF) and np.array_equal(merged[plot_at], plot)
    plot, merged, ref_at, plot_at = m._fppi_grids([0.01, 0.01, 1.0])          # repeated values, values equal to reference points
    assert np.array_equal(merged[ref_at], m.FPPI_REF) and np.array_equal(merged[plot_at], [0.01, 0.01, 1.0])


def test_python_layer_fails_loudly(monkeypatch):
    m = _metrics()
    tp, conf, pc, tc = np.ones((4, 10), bool), np.linspace(0.9, 0.1, 4), np.zeros(4), np.zeros(3)
    with pytest.raises(ValueError):
        m.curves_per_class(np.ones(4, bool), conf, pc, tc, 2)
    with pytest.raises(ValueError):
        m.curves_per_class(tp, conf[:3], pc, tc, 2)
    with pytest.raises(ValueError):
        m.curves_per_class(tp, conf, pc, np.array([0.5]), 2)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="n_images"):
            m.curves_per_class(tp, conf, pc, tc, bad)
    for grid in ([], [0.1, 0.05], [0.1, float("nan")], [0.1, float("inf")], np.ones((2, 2)), np.ones(4088)):
        with pytest.raises(ValueError, match="fppi_grid"):
            m.curves_per_class(tp, conf, pc, tc, 2, fppi_grid=grid)
    with pytest.raises(ValueError, match="which"):
        m.plot_mc_curve(None, "ap")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU"):
        m.curves_per_class(tp, conf, pc, tc, 2)
    with pytest.raises(NotImplementedError, match="out of scope"):       # the switch of ap_per_class stays as it was
        m.ap_per_class(tp, conf, pc, tc, plot=True)
    # an evaluator that saw nothing has empty curves, with or without a GPU
    cv = m.DetectionEvaluator(3).curves()
    assert cv.p.shape == cv.r.shape == cv.f1.shape == cv.py.shape == (0, 1000) and cv.mr_curve.shape == (0, 1000)
    assert cv.mr_ref.shape == (0, 9) and cv.lamr.shape == (0,) and cv.mlamr == 0.0 and cv.best == 0 and cv.ap_class.size == 0
    assert np.array_equal(cv.px, curves_ref.PX) and np.array_equal(cv.fppi, curves_ref.FPPI_PLOT)


def test_evaluate_curves_needs_a_save_dir():
    import msod_amd  # noqa: F401
    from msod_amd.evaluate import evaluate
    with pytest.raises(ValueError, match="save_dir"):
        evaluate(torch.nn.Linear(1, 1), [], 3, curves=True)


def test_plot_functions_write_files(tmp_path, cases):
    pytest.importorskip("matplotlib")
    m = _metrics()
    case = next(c for c in cases if c["name"] == "nc3_rect")
    ref = _ref(case)
    cv = m.EvalCurves(**vars(ref))
    m.plot_pr_curve(cv, case["ap"].numpy(), tmp_path, names=["person", "car", "bike"])
    for which in ("f1", "p", "r"):
        m.plot_mc_curve(cv, which, tmp_path, names={0: "person", 1: "car"})
    m.plot_mr_curve(cv, tmp_path)
    for f in ("PR_curve.png", "F1_curve.png", "P_curve.png", "R_curve.png", "MR_curve.png"):
        assert (tmp_path / f).stat().st_size > 0, f
    m.plot_mr_curve(cv, tmp_path / "missing" / "dir")                   # silent on failure, like ConfusionMatrix.plot


def test_header_declares_the_entry_points():
    import ctypes
    import msod_amd  # noqa: F401
    from msod_amd import _lib
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib.SIGNATURES["cft_eval_curves_workspace_bytes"] == (i, [l, i, vp])
    assert _lib.SIGNATURES["cft_eval_curves"] == (i, [vp, vp, vp, l, vp, i, i, vp, vp, vp, i, vp, l, vp, vp, vp, vp, vp, vp, vp])
    assert "curves.hip" in _lib.SOURCES
    assert not _lib.missing_symbols()


def test_curves_kernels_use_no_scratch():
    notes = helpers.kernel_notes(SRC)
    assert len(notes) == len(re.findall(r"__global__", open(SRC).read())) == 2, sorted(notes)
    for name, m in notes.items():
        assert m["private_segment_fixed_size"] == 0, name
        assert m["vgpr_spill_count"] == 0, name
        assert m["sgpr_spill_count"] == 0, name
