"""Generate ``tests/golden/eval/curve_cases.pt``: the arrays the reference's own ``ap_per_class(plot=True)`` hands to its plot functions.

Runs ONLY in the build container (needs the reference checkout at ``make_golden.REF``).  The reference's ``utils/metrics.py`` runs
unmodified on the CPU; its ``plot_pr_curve`` and ``plot_mc_curve`` are bound, at run time, to functions that record their array
arguments instead of drawing.  Only those arrays (and the inputs) are stored.

    python tests/golden/make_curves_golden.py       # rewrites tests/golden/eval/curve_cases.pt

Cases: the ``stats`` of every case of ``eval_cases.pt`` that has any, and two synthetic ones: ``nc3_holes`` (class 0 with labels and
predictions, class 1 with labels and no predictions, class 2 with predictions and no labels) and ``nc1_600`` (one class, 600
predictions: more than two chunks of the kernel's walk).  The reference appends a ``py`` row only for a class with labels AND
predictions; ``py_classes`` names those rows.  Confidences are distinct within a case (the reference's argsort is unstable), which the
script asserts.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

SRC = os.path.join(HERE, "eval", "eval_cases.pt")
OUT = os.path.join(HERE, "eval", "curve_cases.pt")


def synthetic():
    g = np.random.default_rng(21)
    out = []
    # nc 3: class 0 labelled and predicted, class 1 labelled only, class 2 predicted only
    n = 90
    pred_cls = np.where(g.random(n) < 0.7, 0.0, 2.0)
    conf = g.permutation(np.linspace(0.02, 0.98, n)).astype(np.float32)
    tp = (g.random(n) < 0.6)[:, None] & (g.random((n, 10)) < np.linspace(1.0, 0.2, 10)[None])
    tp[pred_cls == 2.0] = False
    target_cls = np.concatenate([np.zeros(40), np.ones(7)])
    out.append(("nc3_holes", tp, conf, pred_cls, target_cls, 12))
    # nc 1, 600 predictions
    n = 600
    conf = g.permutation(np.linspace(0.001, 0.999, n)).astype(np.float32)
    tp = (g.random(n) < 0.2 + 0.6 * conf)[:, None] & (g.random((n, 10)) < np.linspace(1.0, 0.3, 10)[None])
    out.append(("nc1_600", tp, conf, np.zeros(n), np.zeros(250), 40))
    return out


def run(metrics, tp, conf, pred_cls, target_cls):
    rec = {}

    def pr(px, py, ap, save_dir=None, names=()):
        rec["px"], rec["py"], rec["ap"] = np.array(px), np.array(py).reshape(-1, 1000), np.array(ap)

    def mc(px, py, save_dir=None, names=(), xlabel=None, ylabel=None):
        rec[{"F1": "f1", "Precision": "p", "Recall": "r"}[ylabel]] = np.array(py)

    metrics.plot_pr_curve, metrics.plot_mc_curve = pr, mc
    out = metrics.ap_per_class(tp, conf, pred_cls, target_cls, plot=True)
    rec["best"] = int(rec["f1"].mean(0).argmax())
    rec["ap_class"] = np.array(out[4])
    assert np.array_equal(out[0], rec["p"][:, rec["best"]]) and np.array_equal(out[3], rec["f1"][:, rec["best"]])
    return rec


def main():
    make_golden.install_reference()
    import torchvision  # the stand-in module
    torchvision.ops = type(sys)("torchvision.ops")
    import utils.general  # noqa: F401  (first: the reference's general and metrics import each other)
    from utils import metrics  # the reference's utils/metrics.py
    inputs = []
    for case in torch.load(SRC, weights_only=False)["cases"]:
        if case["stats"] is None:
            continue
        s = case["stats"]
        seen = sum(b["rows"].shape[0] for b in case["batches"])
        inputs.append((case["name"], s["tp"].numpy(), s["conf"].numpy(), s["pred_cls"].numpy(), s["target_cls"].numpy(), seen))
    inputs += synthetic()
    cases = []
    for name, tp, conf, pred_cls, target_cls, n_images in inputs:
        assert np.unique(conf).size == conf.size, f"{name}: tied confidences"
        rec = run(metrics, tp, conf, pred_cls, target_cls)
        with_preds = [int(c) for c in rec["ap_class"] if (pred_cls == c).any()]
        assert rec["py"].shape[0] == len(with_preds), name
        case = {"name": name, "n_images": int(n_images), "py_classes": torch.tensor(with_preds, dtype=torch.int32),
                "tp": torch.from_numpy(np.ascontiguousarray(tp)), "conf": torch.from_numpy(np.ascontiguousarray(conf)),
                "pred_cls": torch.from_numpy(np.ascontiguousarray(pred_cls)),
                "target_cls": torch.from_numpy(np.array(target_cls, dtype=np.float64)), "best": rec["best"]}
        for k in ("px", "py", "p", "r", "f1", "ap", "ap_class"):
            case[k] = torch.from_numpy(np.ascontiguousarray(rec[k]))
        cases.append(case)
        print(f"{name}: {len(conf)} predictions, classes {rec['ap_class'].tolist()}, py rows {with_preds}, best {rec['best']}")
    torch.save({"cases": cases}, OUT)
    size = os.path.getsize(OUT)
    assert size < 1 << 20, size
    print(f"wrote {OUT} ({size / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
