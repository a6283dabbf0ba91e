"""GPU tests of the validation curves (cft_eval_curves in csrc/curves.hip, utils.metrics.curves_per_class / DetectionEvaluator.curves,
evaluate(curves=True)) against the arrays the reference's own ap_per_class(plot=True) handed to its plot functions
(tests/golden/eval/curve_cases.pt) and against the whole-array restatement in tests/curves_ref.py.

Bounds: py, p, r, f1 within 1e-12 (the bound tests/test_eval_host.py uses for the same float64 arithmetic: the kernel evaluates numpy's
interpolation formula, the compiler may not contract it, and what remains is the last-bit freedom of numpy's own loops).  The miss rate
must be EQUAL: its counts are exact integers and each value is one correctly rounded division and one subtraction in double."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import curves_ref
import launch_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval", "curve_cases.pt")
EVAL_GOLDEN = os.path.join(ROOT, "tests", "golden", "eval", "eval_cases.pt")
DATA = os.path.join(ROOT, "tests", "golden", "dataset")
FIELDS = ("py", "p", "r", "f1")


@pytest.fixture(scope="module")
def cases():
    return torch.load(GOLDEN, weights_only=False)["cases"]


def _metrics():
    import msod_amd  # noqa: F401
    from msod_amd.utils import metrics
    return metrics


def _check(got, want, what):
    """An EvalCurves against the restatement's namespace."""
    assert np.array_equal(got.ap_class, want.ap_class) and got.ap_class.dtype == np.int32, what
    for name in FIELDS:
        np.testing.assert_allclose(getattr(got, name), getattr(want, name), rtol=0, atol=1e-12, err_msg=f"{what} {name}")
    assert got.best == want.best, what
    assert np.array_equal(got.mr_ref, want.mr_ref), what
    assert np.array_equal(got.mr_curve, want.mr_curve), what
    assert np.array_equal(got.lamr, want.lamr) and got.mlamr == want.mlamr, what
    assert np.array_equal(got.px, curves_ref.PX) and np.array_equal(got.fppi, want.fppi), what


def test_recorded_cases(dev, cases):
    m = _metrics()
    for case in cases:
        args = (case["tp"].numpy(), case["conf"].numpy(), case["pred_cls"].numpy(), case["target_cls"].numpy(), case["n_images"])
        got = m.curves_per_class(*args)
        assert np.array_equal(got.ap_class, case["ap_class"].numpy()), case["name"]
        for name in ("p", "r", "f1"):
            np.testing.assert_allclose(getattr(got, name), case[name].numpy(), rtol=0, atol=1e-12, err_msg=f"{case['name']} {name}")
        rows = np.flatnonzero(np.isin(got.ap_class, case["py_classes"].numpy()))      # the reference has no py row without predictions
        np.testing.assert_allclose(got.py[rows], case["py"].numpy(), rtol=0, atol=1e-12, err_msg=f"{case['name']} py")
        assert got.best == case["best"], case["name"]
        _check(got, curves_ref.curves(*args), case["name"])
        # the tensor form of the arguments, and the results ap_per_class reads at `best`
        p, r, _, f1, _ = m.ap_per_class(*args[:4])
        assert np.array_equal(got.p[:, got.best], p) and np.array_equal(got.r[:, got.best], r) and np.array_equal(got.f1[:, got.best], f1)


def _synthetic(g, sizes, nc, labelled, ties=True, mode="mixed"):
    """Classes `labelled` get labels; class c gets sizes[c] predictions (classes beyond len(sizes): none)."""
    pred_cls = np.concatenate([np.full(k, c) for c, k in enumerate(sizes)] + [np.zeros(0)]).astype(np.float64)
    n = len(pred_cls)
    order = g.permutation(n)
    pred_cls = pred_cls[order]
    conf = ((g.integers(1, 40, n) / 40.0) if ties else g.permutation(np.linspace(0.01, 0.99, n))).astype(np.float32)
    tp0 = {"mixed": g.random(n) < 0.5, "all_tp": np.ones(n, bool), "all_fp": np.zeros(n, bool)}[mode]
    tp = tp0[:, None] & (g.random((n, 10)) < 0.7)
    tp[:, 0] = tp0
    target_cls = np.concatenate([np.full(int(g.integers(1, 400)), c) for c in labelled]).astype(np.float64)
    assert max(labelled) == nc - 1
    return tp, conf, pred_cls, target_cls


@pytest.mark.parametrize("sizes, nc, labelled, mode", [
    ((1,), 1, (0,), "mixed"),
    ((255,), 1, (0,), "mixed"),
    ((256,), 1, (0,), "all_tp"),
    ((257,), 1, (0,), "all_fp"),
    ((513,), 1, (0,), "mixed"),
    ((513, 0, 256, 40), 3, (0, 1, 2), "mixed"),          # class 1: labels and no predictions; class 3: predictions of a class beyond nc
    ((257, 300, 255), 3, (0, 2), "mixed"),               # class 1: predictions and no labels
    (tuple(range(1, 78)) + (0, 513, 256), 80, tuple(range(0, 70)) + (77, 79), "mixed"),
])
def test_chunk_boundaries_against_restatement(dev, sizes, nc, labelled, mode):
    m = _metrics()
    g = np.random.default_rng(len(sizes) * 1000 + sum(sizes))
    args = _synthetic(g, sizes, nc, labelled, ties=True, mode=mode) + (17,)
    got = m.curves_per_class(*args)
    _check(got, curves_ref.curves(*args), str(sizes[:4]))
    again = m.curves_per_class(*args)
    for name in FIELDS + ("mr_curve", "mr_ref", "lamr"):
        assert np.array_equal(getattr(got, name), getattr(again, name)), name            # bit for bit, run to run
    assert got.best == again.best
    if mode == "all_tp":
        assert (got.mr_curve == 1.0 - 256 / (np.sum(args[3] == 0) + 1e-16)).all()        # no false positive: the last prediction owns every value
    if mode == "all_fp":
        assert np.array_equal(got.mr_ref, np.ones((1, 9))) and np.array_equal(got.lamr, [1.0])
    if nc == 3 and labelled == (0, 1, 2):
        assert np.array_equal(got.mr_curve[1], np.ones(1000)) and not got.py[1].any() and not got.p[1].any()


@pytest.mark.parametrize("grid", [np.array([0.3]), np.sort(np.random.default_rng(1).uniform(-2.0, 30.0, 4087)),
                                  np.repeat(np.array([0.0, 0.01, 0.01, 0.5, 2.0]), 3)], ids=["one", "full", "repeated"])
def test_grids(dev, grid):
    """One value, the largest grid the device takes (4087 + the nine reference points = 4096, some below every fppi, some negative)
    and repeated values."""
    m = _metrics()
    g = np.random.default_rng(4)
    args = _synthetic(g, (300, 20), 2, (0, 1)) + (9,)
    got = m.curves_per_class(*args, fppi_grid=grid)
    want = curves_ref.curves(*args, fppi_grid=grid)
    assert got.mr_curve.shape == (2, len(grid))
    _check(got, want, f"grid of {len(grid)}")
    if len(grid) == 4087:
        assert m._fppi_grids(grid)[1].size == m.MAX_FPPI_GRID == 4096
        assert (got.mr_curve[:, grid < 0] == 1.0).all()


def test_no_predictions_at_all(dev):
    m = _metrics()
    got = m.curves_per_class(np.zeros((0, 10), bool), np.zeros(0), np.zeros(0), np.array([0.0, 2.0, 2.0]), 5)
    assert got.ap_class.tolist() == [0, 2] and got.best == 0
    assert not got.p.any() and not got.r.any() and not got.f1.any() and not got.py.any()
    assert np.array_equal(got.mr_curve, np.ones((2, 1000))) and np.array_equal(got.lamr, [1.0, 1.0]) and got.mlamr == 1.0
    empty = m.curves_per_class(np.zeros((0, 10), bool), np.zeros(0), np.zeros(0), np.zeros(0), 5)
    assert empty.p.shape == (0, 1000) and empty.mlamr == 0.0


def _fill_evaluator(m, case, dev, **kw):
    from msod_amd.utils.general import batched_nms
    nc = 1 if case["single_cls"] else case["nc"]
    ev = m.DetectionEvaluator(nc, single_cls=case["single_cls"], **kw)
    for b in case["batches"]:
        dets, counts = batched_nms(b["rows"].to(dev), case["conf_thres"], case["iou_thres"], multi_label=True, agnostic=case["single_cls"])
        ev.update(dets, counts, b["targets"].to(dev), b["img_hw"], b["shapes"])
    return ev


def test_evaluator_curves_agree_with_compute(dev, cases):
    """DetectionEvaluator.curves() on the recorded batches: the reference's arrays, p / r / f1 at `best` equal to compute()'s, and
    compute() before and after: identical results and the identical launch list."""
    m = _metrics()
    by_name = {c["name"]: c for c in cases}
    for case in torch.load(EVAL_GOLDEN, weights_only=False)["cases"]:
        ev = _fill_evaluator(m, case, dev)
        with launch_trace.recording(dev) as before:
            res0 = ev.compute()
        with launch_trace.recording(dev) as during:
            cv = ev.curves()
        with launch_trace.recording(dev) as after:
            res1 = ev.compute()
        assert launch_trace.first_difference(after, before) is None
        assert [e.split()[0] for e in before] == ["cft_eval_ap_workspace_bytes", "cft_eval_ap"]
        assert [e.split()[0] for e in during] == ["cft_eval_curves_workspace_bytes", "cft_eval_curves"]
        for f in ("mp", "mr", "map50", "map75", "map", "seen"):
            assert getattr(res0, f) == getattr(res1, f), (case["name"], f)
        for f in ("maps", "p", "r", "ap", "f1", "ap_class"):
            assert np.array_equal(np.asarray(getattr(res0, f)), np.asarray(getattr(res1, f))), (case["name"], f)
        if case["stats"] is None:                      # labels, predictions, no TP: compute() reports zeros, the curves still exist
            assert len(cv.ap_class) == 3 and not cv.r.any() and np.array_equal(cv.mr_ref, np.ones((3, 9)))
            continue
        want = by_name[case["name"]]
        for name in ("p", "r", "f1", "py"):
            np.testing.assert_allclose(getattr(cv, name), want[name].numpy(), rtol=0, atol=1e-12, err_msg=f"{case['name']} {name}")
        assert cv.best == want["best"]
        assert np.array_equal(cv.p[:, cv.best], res0.p) and np.array_equal(cv.r[:, cv.best], res0.r)
        assert np.array_equal(cv.f1[:, cv.best], res0.f1)
        s = case["stats"]
        ref = curves_ref.curves(s["tp"].numpy(), s["conf"].numpy(), s["pred_cls"].numpy(), s["target_cls"].numpy(), ev.seen)
        assert np.array_equal(cv.mr_curve, ref.mr_curve) and np.array_equal(cv.mr_ref, ref.mr_ref) and cv.mlamr == ref.mlamr


def test_curves_synchronise_once(dev):
    m = _metrics()
    case = torch.load(EVAL_GOLDEN, weights_only=False)["cases"][0]
    ev = _fill_evaluator(m, case, dev)
    ev.curves()                                         # the grids are uploaded and cached
    _, merged, _, _ = m._fppi_grids(None)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = m._curves_device(ev._tp, ev._conf, ev._pcls, ev.n, ev._hist, ev.nc, ev.seen, merged, dev)      # the device stage
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out.numel() == 4 * ev.nc * 1000 + ev.nc * 1009 + 1
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ev.curves()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message)]
    assert len(syncs) == 1, [str(w.message) for w in caught]


def test_bad_arguments_launch_nothing(dev):
    """Every refusal comes from the checks in front of the first launch: the status is CFT_EINVAL and the outputs keep their fill."""
    import msod_amd  # noqa: F401
    from msod_amd import _lib
    lib = _lib.load()
    einval = _lib.parse_header(open(_lib.HEADER).read())[1]["CFT_EINVAL"]
    n, nc, ng = 100, 3, 9
    g = np.random.default_rng(0)
    tp = torch.from_numpy(g.integers(0, 2, n).astype(np.int16)).to(dev)
    conf = torch.from_numpy(g.random(n).astype(np.float32)).to(dev)
    pcls = torch.from_numpy(g.integers(0, nc, n).astype(np.int32)).to(dev)
    hist = torch.tensor([5, 0, 7, 0], dtype=torch.int32, device=dev)
    px = torch.from_numpy(curves_ref.PX).to(dev)
    grid = np.ascontiguousarray(curves_ref.FPPI_REF)
    grid_dev = torch.from_numpy(grid).to(dev)
    nbytes = ctypes.c_long(0)
    assert lib.cft_eval_curves_workspace_bytes(n, nc, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    assert lib.cft_eval_curves_workspace_bytes(-1, nc, ctypes.byref(nbytes)) == einval
    assert lib.cft_eval_curves_workspace_bytes(n, 0, ctypes.byref(nbytes)) == einval
    assert lib.cft_eval_curves_workspace_bytes(n, nc, None) == einval
    ws = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=dev)
    fill = -7.0
    out = torch.full((4 * nc * 1000 + nc * ng + 1,), fill, dtype=torch.float64, device=dev)
    k = nc * 1000

    def call(**kw):
        a = dict(tp=tp.data_ptr(), conf=conf.data_ptr(), pcls=pcls.data_ptr(), n=n, hist=hist.data_ptr(), nc=nc, n_images=4, px=px.data_ptr(),
                 grid=grid_dev.data_ptr(), grid_host=grid.ctypes.data, ng=ng, ws=ws.data_ptr(), ws_bytes=nbytes.value, p=out.data_ptr(),
                 r=out.data_ptr() + 8 * k, f1=out.data_ptr() + 16 * k, py=out.data_ptr() + 24 * k, mr=out.data_ptr() + 32 * k,
                 best=out.data_ptr() + 32 * k + 8 * nc * ng)
        a.update(kw)
        return lib.cft_eval_curves(*a.values(), None)

    down = np.ascontiguousarray(grid[::-1])
    nan = grid.copy()
    nan[3] = np.nan
    inf = grid.copy()
    inf[-1] = np.inf
    bad = [dict(tp=None), dict(conf=None), dict(pcls=None), dict(hist=None), dict(px=None), dict(grid=None), dict(grid_host=None), dict(ws=None),
           dict(p=None), dict(r=None), dict(f1=None), dict(py=None), dict(mr=None), dict(best=None), dict(n=-1), dict(n=1 << 30), dict(nc=0),
           dict(nc=65536), dict(n_images=0), dict(n_images=-3), dict(ng=0), dict(ng=4097), dict(grid_host=down.ctypes.data),
           dict(grid_host=nan.ctypes.data), dict(grid_host=inf.ctypes.data), dict(ws_bytes=nbytes.value - 1), dict(ws=ws.data_ptr() + 8),
           dict(mr=out.data_ptr() + 32 * k + 4), dict(best=out.data_ptr() + 32 * k + 8 * nc * ng + 2), dict(px=px.data_ptr() + 4)]
    for kw in bad:
        assert call(**kw) == einval, kw
        assert b"cft_eval_curves" in lib.cft_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == fill).all())                    # nothing was launched
    assert call() == 0                                  # and the good call fills every slot
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert not (host[:-1] == fill).any() and host[-1:].view(np.int32)[0] in range(1000)
    assert not host[k:2 * k].reshape(nc, 1000)[1].any() and not host[4 * k:4 * k + nc * ng].reshape(nc, ng)[1].any()      # class 1: no labels


def test_evaluate_curves(dev, tmp_path):
    """evaluate(curves=True, confusion=True) on the ten pairs of tests/golden/dataset (the loader keeps eight) with the seeded tiny model:
    the five curve images and the confusion-matrix image, metrics identical to a run without the switch, and the mean log-average miss
    rate of the restatement fed from match_batch's statistics of the same detections."""
    import contextlib
    import io
    from types import SimpleNamespace
    pytest.importorskip("matplotlib")
    from msod_amd.evaluate import evaluate
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils import datasets as D
    from msod_amd.utils.general import batched_nms
    from msod_amd.utils.seeded import seeded_state_dict
    m = _metrics()
    model = Model(named_config("cfg2"))
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7))
    model = model.to(dev)
    with contextlib.redirect_stdout(io.StringIO()):
        loader, _ = D.create_dataloader_rgb_ir(os.path.join(DATA, "rgb", "images"), os.path.join(DATA, "ir", "images"), 64, 2, 32,
                                               SimpleNamespace(single_cls=True), pad=0.5, rect=True)
    batches = [(img.clone(), t.clone(), p, s) for img, t, p, s in loader]
    plain = evaluate(model, batches, 1, single_cls=True, confusion=True)
    details = {}
    run = tmp_path / "run"
    got = evaluate(model, batches, 1, single_cls=True, confusion=True, curves=True, save_dir=str(run), names=["object"], details=details)
    np.testing.assert_equal(got[0], plain[0])
    np.testing.assert_equal(np.asarray(got[1]), np.asarray(plain[1]))
    assert np.array_equal(got[2]["confusion_matrix"], plain[2]["confusion_matrix"])
    files = sorted(f.name for f in run.iterdir())
    assert files == sorted(["PR_curve.png", "F1_curve.png", "P_curve.png", "R_curve.png", "MR_curve.png", "confusion_matrix.png"])
    assert all((run / f).stat().st_size > 0 for f in files)
    stats = []
    for img, targets, _, shapes in batches:
        img = img.to(dev)
        with torch.no_grad():
            out = model(img[:, :3], img[:, 3:])[0]
            dets, counts = batched_nms(out, 0.001, 0.6, multi_label=True, agnostic=True)
        stats.extend(m.match_batch(dets, counts, targets, img.shape[2:], shapes, single_cls=True).to_stats())
    tp, conf, pcls, tcls = [np.concatenate([np.asarray(s[i]) for s in stats], 0) for i in range(4)]
    cv = details["curves"]
    want = curves_ref.curves(tp, conf, pcls, tcls, sum(b[0].shape[0] for b in batches))
    assert isinstance(cv, m.EvalCurves) and cv.mlamr == want.mlamr and np.array_equal(cv.mr_ref, want.mr_ref)
    assert details["result"].seen == 8
