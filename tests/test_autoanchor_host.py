"""Host tests of autoanchor: tests/anchor_ref.py (a numpy restatement from the rules) against the reference's own results in
tests/golden/autoanchor/anchor_cases.pt (made with scipy's kmeans), and the C ABI's declarations."""
import os

import numpy as np
import pytest
import torch

import anchor_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "autoanchor", "anchor_cases.pt")
NAMES = ["small_170_n9", "tiny_px_170_n9", "mid_2400_n9", "mid_2400_n12", "big_22k_n9", "good_anchors", "not_better", "dropped_cluster"]


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in torch.load(GOLDEN, weights_only=False)["cases"]}


def dataset(case):
    return case["shapes"].numpy(), anchor_ref.labels_of(case["counts"].numpy(), case["wh"].numpy())


def test_golden_is_data_and_covers_the_cases(cases):
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert list(cases) == NAMES
    n = {k: len(c["wh"]) for k, c in cases.items()}
    assert 150 <= n["small_170_n9"] <= 200 and 2300 <= n["mid_2400_n9"] <= 2500 and 21000 <= n["big_22k_n9"] <= 24000
    assert cases["mid_2400_n12"]["n"] == 12 and cases["big_22k_n9"]["gen"] == 1000
    assert "WARNING: Extremely small objects" in cases["tiny_px_170_n9"]["text0"]
    assert "Attempting" not in cases["good_anchors"]["check_text"]
    assert "Original anchors better" in cases["not_better"]["check_text"]
    d = cases["dropped_cluster"]
    assert d["k0"] is None and "returned only" in d["text0"] and "ERROR" in d["check_text"]
    assert torch.equal(d["before"]["anchor_grid"], d["after"]["anchor_grid"])
    for c in cases.values():
        if c["k"] is not None:
            assert c["gap"] >= c["margin"] == 4 * (c["D"] + 1)


@pytest.mark.parametrize("name", NAMES)
def test_restated_kmeans_equals_scipys(cases, name):
    """rtol 1e-9: float64 sums of <= 2^20 positive terms differ by at most about n 2^-53 ~ 1e-10 between orders."""
    c = cases[name]
    shapes, labels = dataset(c)
    wh0 = anchor_ref.label_wh(shapes, labels, c["img_size"])
    wh = wh0[(wh0 >= 2.0).any(1)]
    s = wh.std(0)
    np.random.seed(c["seed"])
    book, dist, _ = anchor_ref.kmeans(wh / s, c["n"], anchor_ref.draw_restarts(len(wh), c["n"]))
    if c["k0"] is None:
        assert len(book) < c["n"]
        assert f"returned only {len(book)}" in c["text0"]
        return
    k = book * s
    np.testing.assert_allclose(k[np.argsort(k.prod(1))], c["k0"].numpy(), rtol=1e-9, atol=0)
    # gen = 0 consumed nothing after the restarts' draws
    assert np.random.random() == c["rand0"]


@pytest.mark.parametrize("name", [n for n in NAMES if n != "dropped_cluster"])
def test_restated_evolution_ends_at_the_references_anchors(cases, name):
    c = cases[name]
    shapes, labels = dataset(c)
    np.random.seed(c["seed"])
    r = anchor_ref.kmean_anchors(shapes, labels, c["n"], c["img_size"], c["thr"], c["gen"])
    np.testing.assert_allclose(r["k"], c["k"].numpy(), rtol=1e-9, atol=0)
    assert np.random.random() == c["rand"]
    # from the reference's own gen = 0 anchors the float64 products are the reference's: equal bits
    k, _, flags, _ = anchor_ref.evolve(r["wh"], c["k0"].numpy(), 1. / c["thr"], r["v"])
    assert np.array_equal(k[np.argsort(k.prod(1))], c["k"].numpy())
    assert flags.sum() == c["text"].count("best possible recall") - 2          # verbose: one print per improvement, one before, one after


def test_exact_fitness_is_within_ulps_of_a_float32_mean(cases):
    c = cases["mid_2400_n9"]
    shapes, labels = dataset(c)
    wh = anchor_ref.label_wh(shapes, labels, 640).astype(np.float32)
    k = c["k0"].numpy()
    f, g = anchor_ref.fitness(wh, k, 0.25), anchor_ref.torch_style_fitness(wh, k, 0.25)
    assert abs(float(f) - float(g)) <= 4 * np.spacing(np.float32(f))


def test_metric_restatement_matches_printed_check_line(cases):
    """bpr / aat of check_anchors' first line, to their printed precision, from the restated metric on the scaled labels."""
    for name in ("small_170_n9", "mid_2400_n9", "good_anchors", "not_better"):
        c = cases[name]
        shapes, labels = dataset(c)
        np.random.seed(c["seed"])
        scale = np.random.uniform(0.9, 1.1, size=(len(shapes), 1))
        wh = anchor_ref.label_wh(shapes, labels, 640, scale).astype(np.float32)
        m = anchor_ref.metric(wh, c["before"]["anchor_grid"].view(-1, 2).numpy(), 0.25)
        assert f"anchors/target = {m['aat']:.2f}, Best Possible Recall (BPR) = {m['bpr']:.4f}" in c["check_text"], name


def test_abi_declares_the_entry_points():
    import msod_amd  # noqa: F401
    from msod_amd import _lib
    assert _lib.ABI_VERSION >= 16
    for name in ("cft_anchor_metric", "cft_anchor_kmeans", "cft_anchor_kmeans_workspace_bytes", "cft_anchor_evolve",
                 "cft_anchor_evolve_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
    assert "autoanchor.hip" in _lib.SOURCES
    src = open(os.path.join(_lib.CSRC, "autoanchor.hip")).read()
    assert "atomicAdd(float" not in src and "hipMalloc" not in src and "Synchronize" not in src


def test_module_surface():
    import inspect
    import msod_amd  # noqa: F401
    from msod_amd.utils import autoanchor as aa
    assert str(inspect.signature(aa.kmean_anchors)) == "(path, n=9, img_size=640, thr=4.0, gen=1000, verbose=True)"
    assert str(inspect.signature(aa.check_anchors)) == "(dataset, model, thr=4.0, imgsz=640)"
    assert str(inspect.signature(aa.check_anchors_rgb_ir)) == "(dataset, model, thr=4.0, imgsz=640)"
    with pytest.raises(NotImplementedError, match="LoadImagesAndLabels"):
        aa.kmean_anchors("data/coco128.yaml")
    src = open(aa.__file__).read()
    assert "import scipy" not in src and "from scipy" not in src
