"""GPU tests of autoanchor (csrc/autoanchor.hip, utils/autoanchor.py) against tests/anchor_ref.py and the reference's own results in
tests/golden/autoanchor/anchor_cases.pt."""
import contextlib
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import anchor_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "autoanchor", "anchor_cases.pt")
NAMES = ["small_170_n9", "tiny_px_170_n9", "mid_2400_n9", "mid_2400_n12", "big_22k_n9", "good_anchors", "not_better", "dropped_cluster"]


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in torch.load(GOLDEN, weights_only=False)["cases"]}


def dataset(case):
    return SimpleNamespace(shapes=case["shapes"].numpy(), labels=anchor_ref.labels_of(case["counts"].numpy(), case["wh"].numpy()))


def quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn(*a, **k)
    return out, buf.getvalue()


def lognormal_wh(g, n):
    return np.exp(g.normal(np.log(40.0), 0.9, (n, 2))).clip(1.0, 620.0).astype(np.float32)


@pytest.mark.parametrize("name", NAMES)
def test_metric_counts_and_sums_equal_the_restatement(dev, cases, name):
    from msod_amd.utils.autoanchor import anchor_metric
    c = cases[name]
    ds = dataset(c)
    np.random.seed(c["seed"])
    scale = np.random.uniform(0.9, 1.1, size=(len(ds.shapes), 1))
    wh = anchor_ref.label_wh(ds.shapes, ds.labels, 640, scale).astype(np.float32)
    ks = [np.array([[10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90], [156, 198], [373, 326]], np.float32)]
    if c["k"] is not None:
        ks.append(c["k"].numpy().astype(np.float32))
    for k in ks:
        got, want = anchor_metric(torch.from_numpy(wh).to(dev), k, 0.25), anchor_ref.metric(wh, k, 0.25)
        assert (got.n_best_above, got.n_x_above) == (want["n_best_above"], want["n_x_above"])
        assert got.sum_x == want["sum_x"] and got.sum_best == want["sum_best"]
        assert got.sum_x_above == want["sum_x_above"] and got.sum_best_above == want["sum_best_above"]
        assert got.bpr.tobytes() == want["bpr"].tobytes() and got.aat.tobytes() == want["aat"].tobytes()
        assert got.fitness.tobytes() == anchor_ref.fitness(wh, k, 0.25).tobytes()
    if c["check"]:
        m = anchor_metric(wh, c["before"]["anchor_grid"].view(-1, 2), 0.25)
        assert f"anchors/target = {m.aat:.2f}, Best Possible Recall (BPR) = {m.bpr:.4f}" in c["check_text"]


def test_metric_rejects_thresholds_outside_the_exact_range(dev):
    from msod_amd.utils.autoanchor import anchor_metric
    wh = torch.ones(4, 2, device=dev)
    for thr in (1 / 65, 1.5):
        with pytest.raises(RuntimeError, match="anchor_t|thr"):
            anchor_metric(wh, [[1.0, 1.0]], thr)


@pytest.mark.parametrize("name", NAMES)
def test_kmeans_equals_scipys(dev, cases, name):
    from msod_amd.utils.autoanchor import device_kmeans
    c = cases[name]
    ds = dataset(c)
    wh0 = anchor_ref.label_wh(ds.shapes, ds.labels, 640)
    wh = wh0[(wh0 >= 2.0).any(1)]
    s = wh.std(0)
    np.random.seed(c["seed"])
    idx = anchor_ref.draw_restarts(len(wh), c["n"])
    book, dist, info = device_kmeans(wh / s, c["n"], idx, dev)
    book2, dist2, info2 = device_kmeans(wh / s, c["n"], idx, dev)
    assert book.tobytes() == book2.tobytes() and dist == dist2 and info == info2          # two runs, the same bits
    rbook, rdist, _ = anchor_ref.kmeans(wh / s, c["n"], idx)
    assert len(book) == len(rbook)
    # two restarts that reach the same optimum differ in the last bits of their distortion and in the order of their codes: which
    # of them wins depends on the summation order, the set of codes does not
    by_area = lambda b: b[np.lexsort((b[:, 0], b.prod(1)))]      # noqa: E731
    np.testing.assert_allclose(by_area(book), by_area(rbook), rtol=1e-9, atol=0)
    # Where scipy keeps every cluster the distortion is far from zero and rtol 1e-9 alone holds.  In the dropped-cluster case every
    # label equals its code, so the distortion is exactly zero in real arithmetic and what both sides return is only the rounding of
    # the codes: a code is sum / count of up to n equal float64 values, off by at most n 2^-53 |code| per coordinate in either
    # summation order, each distance by at most sqrt(2) times that, on both sides: 4 n 2^-53 max|obs| bounds the difference.
    obs = wh / s
    atol = 0 if c["k0"] is not None else 4 * len(obs) * 2.0 ** -53 * np.abs(obs).max()
    print(f"{name}: distortion {dist!r} restatement {rdist!r} atol {atol!r}")
    np.testing.assert_allclose(dist, rdist, rtol=1e-9, atol=atol)
    if c["k0"] is None:
        assert len(book) < c["n"] and f"returned only {len(book)}" in c["text0"]        # scipy's count
    else:
        k = book * s
        np.testing.assert_allclose(k[np.argsort(k.prod(1))], c["k0"].numpy(), rtol=1e-9, atol=0)


EVOLVE = [(1, 3, 5), (1, 9, 0), (7, 3, 1), (63, 9, 20), (64, 12, 20), (65, 3, 20), (100, 9, 0), (170, 9, 40), (255, 12, 40), (257, 3, 40),
          (300, 9, 1), (513, 9, 60), (1000, 12, 60), (1023, 3, 60), (2049, 9, 80), (4097, 12, 50), (5000, 9, 100), (9999, 3, 100),
          (20001, 9, 60), (70001, 12, 30), (270001, 9, 12), (300000, 9, 3)]


@pytest.mark.parametrize("n,na,gen", EVOLVE)
def test_evolution_equals_the_restatement_bit_for_bit(dev, n, na, gen):
    from msod_amd.utils.autoanchor import device_evolve
    g = np.random.default_rng(1000 * na + gen + n)
    wh = lognormal_wh(g, n)
    k0 = np.sort(np.exp(g.normal(np.log(40.0), 0.8, (na, 2))), 0)
    np.random.seed(n + na + gen)
    v = anchor_ref.draw_mutations(k0.shape, gen)
    k, f, flags, fg = device_evolve(torch.from_numpy(wh).to(dev), k0, 0.25, v)
    rk, rf, rflags, rfg = anchor_ref.evolve(wh, k0, 0.25, v)
    assert np.array_equal(flags, rflags)
    assert fg.tobytes() == rfg.tobytes() and np.float32(f).tobytes() == np.float32(rf).tobytes()
    assert k.tobytes() == rk.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_kmean_anchors_end_to_end(dev, cases, name):
    from msod_amd.utils import autoanchor as aa
    c = cases[name]
    ds = dataset(c)
    np.random.seed(c["seed"])
    if c["k"] is None:
        with pytest.raises(AssertionError):
            quiet(aa.kmean_anchors, ds, n=c["n"], img_size=640, thr=4.0, gen=c["gen"], verbose=False)
        return
    k, text = quiet(aa.kmean_anchors, (ds.shapes, ds.labels), n=c["n"], img_size=640, thr=4.0, gen=c["gen"], verbose=True)
    assert np.random.random() == c["rand"]
    np.testing.assert_allclose(k, c["k"].numpy(), rtol=1e-9, atol=0)
    # the same generations were accepted: one print_results per improvement, whose anchor lines are the reference's
    assert text.count("best possible recall") == c["text"].count("best possible recall")
    anchor_lines = lambda t: [l.split("-mean: ")[1] for l in t.splitlines() if "-mean: " in l]      # noqa: E731
    assert anchor_lines(text) == anchor_lines(c["text"])
    assert text.splitlines()[0] == c["text"].splitlines()[0]
    np.random.seed(c["seed"])
    k0, _ = quiet(aa.kmean_anchors, ds, n=c["n"], img_size=640, thr=4.0, gen=0, verbose=False)
    assert np.random.random() == c["rand0"]
    np.testing.assert_allclose(k0, c["k0"].numpy(), rtol=1e-9, atol=0)


def small_model(dev, anchors=None):
    from msod_amd.models.configs import named_config
    from msod_amd.models.yolo_test import Model
    from msod_amd.utils.seeded import seeded_state_dict
    cfg = named_config("cfg2")
    if anchors is not None:
        cfg = dict(cfg, anchors=anchors)
    model = Model(cfg)
    model.load_state_dict(seeded_state_dict(model.state_dict(), seed=7))
    return model.to(dev)


@pytest.mark.parametrize("name", ["small_170_n9", "tiny_px_170_n9", "mid_2400_n9", "mid_2400_n12", "not_better", "dropped_cluster"])
def test_check_anchors_buffers_and_text(dev, cases, name):
    from msod_amd.utils import autoanchor as aa
    c = cases[name]
    model = small_model(dev, c["check_anchor_list"])
    m = model.model[-1]
    np.testing.assert_allclose(m.anchor_grid.cpu().numpy(), c["before"]["anchor_grid"].numpy(), rtol=1e-6)
    np.random.seed(c["seed"])
    _, text = quiet(getattr(aa, c["check"]), dataset(c), model, thr=4.0, imgsz=640)
    assert np.random.random() == c["check_rand"]
    np.testing.assert_allclose(m.anchor_grid.cpu().numpy(), c["after"]["anchor_grid"].numpy(), rtol=1e-6)
    np.testing.assert_allclose(m.anchors.cpu().numpy(), c["after"]["anchors"].numpy(), rtol=1e-6)
    assert m.anchors.dtype == torch.float32 and m.anchor_grid.dtype == torch.float32
    assert text.rstrip().splitlines()[-1] == c["check_text"].rstrip().splitlines()[-1]
    if name == "dropped_cluster":
        assert "ERROR" in text and torch.equal(m.anchor_grid.cpu(), c["before"]["anchor_grid"])


def test_new_anchors_reach_the_decode_kernel_and_drop_graphs(dev, cases):
    from msod_amd.utils import autoanchor as aa
    from msod_amd.utils.seeded import seeded_inputs
    c = cases["small_170_n9"]
    model = small_model(dev)
    model.set_compute_dtype(torch.float32)
    rgb, ir = (t.to(dev) for t in seeded_inputs(2, 128, 128, seed=7))
    with torch.no_grad():
        model.capture(2, 128, 128)
        old = model(rgb, ir)[0].clone()
        assert len(model._graphs) == 1
        np.random.seed(c["seed"])
        quiet(aa.check_anchors, dataset(c), model, thr=4.0, imgsz=640)
        assert len(model._graphs) == 0                       # the graph captured before the call is gone, not replayed
        eager = model(rgb, ir)[0].clone()
        model.capture(2, 128, 128)
        replay = model(rgb, ir)[0].clone()
        fresh = small_model(dev)
        fresh.load_state_dict(model.state_dict())
        fresh.set_compute_dtype(torch.float32)
        want = fresh(rgb, ir)[0]
    np.testing.assert_allclose(model.model[-1].anchor_grid.cpu().numpy(), c["after"]["anchor_grid"].numpy(), rtol=1e-6)
    assert torch.equal(eager, want) and torch.equal(replay, want)
    assert not torch.equal(old, want)


def test_good_anchors_leave_the_model_untouched(dev, cases):
    from msod_amd.utils import autoanchor as aa
    from msod_amd.utils.seeded import seeded_inputs
    c = cases["good_anchors"]
    model = small_model(dev)
    model.set_compute_dtype(torch.float32)
    rgb, ir = (t.to(dev) for t in seeded_inputs(2, 128, 128, seed=7))
    with torch.no_grad():
        graph = model.capture(2, 128, 128)
        model(rgb, ir)
    det = model.model[-1]
    cache, key, before = det.__dict__.get("_cft_cache"), model.weights_key(), {k: v.clone() for k, v in model.state_dict().items()}
    np.random.seed(c["seed"])
    _, text = quiet(aa.check_anchors, dataset(c), model, thr=4.0, imgsz=640)
    assert np.random.random() == c["check_rand"]
    assert text.rstrip().splitlines()[-1] == c["check_text"].rstrip().splitlines()[-1] and "Attempting" not in text
    assert det.__dict__.get("_cft_cache") is cache and model.weights_key() == key
    assert list(model._graphs.values()) == [graph]
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
