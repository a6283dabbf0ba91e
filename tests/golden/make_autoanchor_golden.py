"""Generate ``tests/golden/autoanchor/anchor_cases.pt``: the reference's own ``kmean_anchors`` / ``check_anchors`` /
``check_anchors_rgb_ir`` (utils/autoanchor.py, with scipy's kmeans) on seeded synthetic datasets.

Runs ONLY in the build container (needs the reference checkout next to ``make_golden.py``'s ``REF``, and scipy).  The reference runs
unmodified on CPU under ``make_golden.install_reference()``'s stand-ins; ``check_anchors`` runs on the reference's own ``Detect`` as the
last layer of a two-layer ``nn.Sequential`` model.

    python tests/golden/make_autoanchor_golden.py       # rewrites tests/golden/autoanchor/anchor_cases.pt

The file holds data only: label sizes, image shapes, seeds, the reference's anchors, printed text, Detect buffers and the next
``np.random.random()`` after each call.

A decision of the reference's genetic loop can hinge on the last bit of a float32 mean, which no other summation order reproduces.  So
the seed of every case is searched (at most 200 tries, then the script fails): the numpy restatement tests/anchor_ref.py, started from the
reference's gen = 0 anchors and the same random state, must end at the reference's anchors (every decision agreed), and the smallest
|fg - f| of its trace must be at least 4 (D + 1) float32 ulps of f, D being the largest deviation seen between torch's float32 mean and
the exact fitness.  D, the gap and the margin are stored.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_golden  # noqa: E402
import anchor_ref  # noqa: E402

OUT = os.path.join(HERE, "autoanchor", "anchor_cases.pt")
DEFAULT_ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
ANCHORS_12 = [[8, 10, 12, 20, 24, 16, 30, 34], [36, 70, 70, 50, 64, 120, 100, 100], [120, 90, 160, 200, 300, 240, 380, 330]]

# name, kind, images, labels per image, n, gen of the kmean_anchors run, check function (or None), first seed
CASES = [
    ("small_170_n9", "lognormal", 24, 7, 9, 1000, "check_anchors", 100),
    ("tiny_px_170_n9", "with_tiny", 24, 7, 9, 200, "check_anchors_rgb_ir", 200),
    ("mid_2400_n9", "lognormal", 300, 8, 9, 1000, "check_anchors", 300),
    ("mid_2400_n12", "lognormal", 300, 8, 12, 300, "check_anchors", 400),
    ("big_22k_n9", "lognormal", 2500, 9, 9, 1000, None, 500),
    ("good_anchors", "at_anchors", 60, 8, 9, 50, "check_anchors", 600),
    ("not_better", "at_anchors_and_specks", 60, 8, 9, 50, "check_anchors", 700),
    ("dropped_cluster", "few_values", 30, 6, 9, 50, "check_anchors", 800),
]


def make_dataset(kind, n_img, per_img, seed):
    """shapes [n_img, 2] (w, h), counts [n_img], wh [sum(counts), 2] float32 normalised label sizes."""
    g = np.random.default_rng(seed)
    shapes = np.stack([g.choice([640, 512, 480, 1280], n_img), g.choice([512, 480, 360, 1024], n_img)], 1).astype(np.float64)
    counts = g.integers(max(1, per_img - 3), per_img + 4, n_img)
    m = int(counts.sum())
    if kind in ("lognormal", "with_tiny"):
        wh = np.exp(g.normal(np.log(0.05), 0.9, (m, 2))).clip(0.004, 0.95)
        wh[:, 1] *= np.exp(g.normal(0.3, 0.3, m))
        wh = wh.clip(0.004, 0.95)
        if kind == "with_tiny":
            wh[g.choice(m, 12, replace=False)] = g.uniform(0.0005, 0.004, (12, 2))       # under 2 and under 3 pixels at 640
    elif kind in ("at_anchors", "at_anchors_and_specks"):
        a = np.array(DEFAULT_ANCHORS, np.float64).reshape(-1, 2)
        wh = a[g.integers(0, 9, m)] * g.uniform(0.8, 1.25, (m, 2)) / 640.0
        if kind == "at_anchors_and_specks":
            wh[g.choice(m, m // 10, replace=False)] = g.uniform(0.0008, 0.002, (m // 10, 2))   # about a pixel: nothing matches them
    elif kind == "few_values":
        shapes[:] = (640, 512)
        vals = np.array([[0.5, 0.03], [0.45, 0.04], [0.04, 0.6], [0.6, 0.05], [0.03, 0.5]])
        wh = vals[g.integers(0, 5, m)]
    return shapes, counts, wh.astype(np.float32)


class Dataset:
    def __init__(self, shapes, counts, wh):
        self.shapes = shapes
        self.labels = anchor_ref.labels_of(counts, wh)


def captured(fn, *a, **k):
    buf = io.StringIO()
    err = None
    with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
        try:
            out = fn(*a, **k)
        except AssertionError as e:
            out, err = None, repr(e)
    return out, buf.getvalue(), err, np.random.random()


def ulps(a, b, f):
    return abs(float(a) - float(b)) / float(np.spacing(np.float32(f)))


def torch_fitness(wh, k, thr):
    """The reference's anchor_fitness formula, evaluated by torch as the reference evaluates it."""
    r = wh[:, None] / torch.tensor(k, dtype=torch.float32)[None]
    best = torch.min(r, 1. / r).min(2)[0].max(1)[0]
    return (best * (best > thr).float()).mean()


def margins(wh, k0, thr, v):
    """(restated final anchors, D, gap, all in float32 ulps of f) of the genetic loop from k0 with the mutations v."""
    k, f, flags, fgs = anchor_ref.evolve(wh, k0, thr, v)
    wht = torch.tensor(wh)
    kk, ff = np.array(k0, np.float64), anchor_ref.fitness(wh, k0, thr)
    D, gap = ulps(torch_fitness(wht, kk, thr), ff, ff), np.inf
    for g in range(len(v)):
        kg = (kk * v[g]).clip(min=2.0)
        D = max(D, ulps(torch_fitness(wht, kg, thr), fgs[g], ff))
        gap = min(gap, ulps(fgs[g], ff, ff))
        if flags[g]:
            kk, ff = kg, fgs[g]
    return k, D, gap


def try_seed(aa, name, kind, n_img, per_img, n, gen, check, seed):
    from models.yolo_test import Detect            # the reference's
    shapes, counts, wh = make_dataset(kind, n_img, per_img, seed)
    ds = Dataset(shapes, counts, wh)
    case = {"name": name, "kind": kind, "seed": seed, "n": n, "img_size": 640, "thr": 4.0, "gen": gen, "shapes": torch.from_numpy(shapes),
            "counts": torch.from_numpy(counts), "wh": torch.from_numpy(wh), "check": check}
    np.random.seed(seed)
    k0, case["text0"], case["error0"], case["rand0"] = captured(aa.kmean_anchors, ds, n=n, img_size=640, thr=4.0, gen=0, verbose=False)
    np.random.seed(seed)
    k, case["text"], case["error"], case["rand"] = captured(aa.kmean_anchors, ds, n=n, img_size=640, thr=4.0, gen=gen, verbose=True)
    case["k0"], case["k"] = (None if k0 is None else torch.from_numpy(k0)), (None if k is None else torch.from_numpy(k))
    if k0 is not None:
        whf = anchor_ref.label_wh(shapes, ds.labels, 640)
        whf = whf[(whf >= 2.0).any(1)].astype(np.float32)
        np.random.seed(seed)
        anchor_ref.draw_restarts(len(whf), n)                       # the state after scipy's kmeans
        kr, D, gap = margins(whf, k0, 0.25, anchor_ref.draw_mutations(k0.shape, gen))
        if not np.array_equal(kr[np.argsort(kr.prod(1))], k) or gap < 4 * (D + 1):
            return None
        case["D"], case["gap"], case["margin"] = D, gap, 4 * (D + 1)
    if check:
        anchors = ANCHORS_12 if n == 12 else DEFAULT_ANCHORS
        det = Detect(nc=1, anchors=anchors, ch=(8, 8, 8))
        det.stride = torch.tensor([8., 16., 32.])
        det.anchors /= det.stride.view(-1, 1, 1)
        model = torch.nn.Module()
        model.model = torch.nn.Sequential(torch.nn.Identity(), det)
        before = {"anchors": det.anchors.clone(), "anchor_grid": det.anchor_grid.clone()}
        got, orig = [], aa.kmean_anchors

        def recording(*a, **kw):
            got.append(orig(*a, **kw))
            return got[-1]

        aa.kmean_anchors = recording
        try:
            np.random.seed(seed)
            _, case["check_text"], _, case["check_rand"] = captured(getattr(aa, check), ds, model, thr=4.0, imgsz=640)
        finally:
            aa.kmean_anchors = orig
        case["check_anchor_list"], case["before"] = anchors, before
        case["after"] = {"anchors": det.anchors.clone(), "anchor_grid": det.anchor_grid.clone()}
        case["check_k"] = torch.from_numpy(got[0]) if got else None
        if got:     # the run inside check_anchors (1000 generations, another random state) must be as decidable
            np.random.seed(seed)
            np.random.uniform(0.9, 1.1, size=(len(shapes), 1))
            r = anchor_ref.kmean_anchors(shapes, ds.labels, n, 640, 4.0, 1000)
            if r["survivors"] != n or not np.allclose(r["k"], got[0], rtol=1e-9, atol=0):
                return None
            _, D, gap = margins(r["wh"], r["k0"], 0.25, r["v"])
            if gap < 4 * (D + 1):
                return None
            case["check_D"], case["check_gap"] = D, gap
    return case


def main():
    make_golden.install_reference()
    sys.path.insert(0, make_golden.REF)
    from utils import autoanchor as aa      # the reference's
    cases = []
    for name, kind, n_img, per_img, n, gen, check, seed0 in CASES:
        for seed in range(seed0, seed0 + 200):
            case = try_seed(aa, name, kind, n_img, per_img, n, gen, check, seed)
            if case is not None:
                break
        else:
            raise SystemExit(f"{name}: no seed in [{seed0}, {seed0 + 200}) gives decisions that are {4}(D + 1) ulps clear")
        cases.append(case)
        print(f"{name}: seed {case['seed']}, {len(case['wh'])} labels, D = {case.get('D')}, gap = {case.get('gap')} ulps, "
              f"error0 = {case['error0']}, check: {case.get('check_text', '').strip().splitlines()[-1:] }")
    by = {c["name"]: c for c in cases}
    assert by["dropped_cluster"]["k0"] is None and "ERROR" in by["dropped_cluster"]["check_text"]
    assert "WARNING: Extremely small objects" in by["tiny_px_170_n9"]["text0"]
    assert "Attempting" not in by["good_anchors"]["check_text"]
    assert "Original anchors better" in by["not_better"]["check_text"]
    for nm in ("small_170_n9", "mid_2400_n9", "mid_2400_n12", "tiny_px_170_n9"):
        assert "New anchors saved" in by[nm]["check_text"], nm
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save({"cases": cases}, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e3:.1f} kB)")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
