"""Host restatement of the validation curves (cft_eval_curves, utils.metrics.curves_per_class), written from the formulas alone with
whole-array numpy (cumsum, np.interp, searchsorted): the other algorithm from the kernel's walk from the end.

Per class c of np.unique(target_cls), with the predictions in stable order of descending conf (ties keep insertion order):
  tpc = cumsum(tp[:, 0]), fpc = cumsum(1 - tp[:, 0]), recall = tpc / (n_l + 1e-16), precision = tpc / (tpc + fpc)
  r = np.interp(-px, -conf, recall, left=0), p = np.interp(-px, -conf, precision, left=1), f1 = 2 p r / (p + r + 1e-16)
  py = np.interp(px, mrec, mpre), mrec = [0, recall, recall[-1] + 0.01], mpre = reverse running max of [1, precision, 0]
  fppi = [-1, fpc / n_images], miss = [1, 1 - tpc / (n_l + 1e-16)], mr[g] = miss at the last index with fppi <= grid[g]
A class with labels and no predictions has zero p / r / f1 / py rows and a row of ones in mr."""
from types import SimpleNamespace

import numpy as np

PX = np.linspace(0, 1, 1000)
FPPI_REF = np.logspace(-2.0, 0.0, 9)
FPPI_PLOT = np.logspace(-3, 1, 1000)


def log_average_miss_rate(mr_ref):
    return np.exp(np.mean(np.log(np.maximum(1e-10, np.asarray(mr_ref, np.float64))), axis=-1))


def miss_rate(tp0, n_l, n_images, grid):
    """Miss rate of one class at every grid value: tp0 = the class's TP column (IoU 0.5) in descending-conf order."""
    tp0 = np.asarray(tp0, bool).astype(np.int64)
    tpc = np.cumsum(tp0)
    fpc = np.cumsum(1 - tp0)
    fppi = np.concatenate(([-1.0], fpc.astype(np.float64) / float(n_images)))
    miss = np.concatenate(([1.0], 1.0 - tpc.astype(np.float64) / (float(n_l) + 1e-16)))
    last = np.searchsorted(fppi, np.asarray(grid, np.float64), side="right") - 1
    return miss[np.maximum(last, 0)]                  # a grid value below the sentinel itself is below the first fppi too: 1.0


def curves(tp, conf, pred_cls, target_cls, n_images, fppi_grid=None):
    """Everything utils.metrics.EvalCurves holds, as a namespace with the same field names."""
    tp = np.asarray(tp, bool).reshape(len(tp), -1)[:, 0]
    conf = np.asarray(conf, np.float32)
    pred_cls = np.asarray(pred_cls, np.float64)
    target_cls = np.asarray(target_cls, np.float64)
    grid = FPPI_PLOT if fppi_grid is None else np.asarray(fppi_grid, np.float64)
    order = np.argsort(-conf, kind="stable")
    tp, conf, pred_cls = tp[order], conf[order].astype(np.float64), pred_cls[order]
    classes = np.unique(target_cls)
    k = len(classes)
    p, r, py = np.zeros((k, 1000)), np.zeros((k, 1000)), np.zeros((k, 1000))
    mr_curve, mr_ref = np.ones((k, len(grid))), np.ones((k, 9))
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        n_l = int((target_cls == c).sum())
        mr_curve[ci] = miss_rate(tp[sel], n_l, n_images, grid)
        mr_ref[ci] = miss_rate(tp[sel], n_l, n_images, FPPI_REF)
        if sel.sum() == 0:
            continue
        t = tp[sel].astype(np.int64)
        tpc, fpc = np.cumsum(t), np.cumsum(1 - t)
        recall = tpc / (n_l + 1e-16)
        precision = tpc / (tpc + fpc)
        r[ci] = np.interp(-PX, -conf[sel], recall, left=0)
        p[ci] = np.interp(-PX, -conf[sel], precision, left=1)
        mrec = np.concatenate(([0.0], recall, [recall[-1] + 0.01]))
        mpre = np.concatenate(([1.0], precision, [0.0]))
        mpre = np.maximum.accumulate(mpre[::-1])[::-1]
        py[ci] = np.interp(PX, mrec, mpre)
    f1 = 2 * p * r / (p + r + 1e-16)
    best = int(f1.mean(0).argmax()) if k else 0
    lamr = log_average_miss_rate(mr_ref) if k else np.zeros(0)
    return SimpleNamespace(px=PX, py=py, p=p, r=r, f1=f1, best=best, ap_class=classes.astype(np.int32), fppi=grid, mr_curve=mr_curve,
                           mr_ref=mr_ref, lamr=lamr, mlamr=float(lamr.mean()) if k else 0.0)
