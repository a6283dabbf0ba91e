"""Host restatement of test.py's statistics (matching :132-218, ap_per_class utils/metrics.py:18-108), written from the
rules alone.  The oracle of tests/test_eval_host.py (against the recorded reference) and of the large GPU cases.

Matching runs in float32 numpy in the reference's order of operations; the curves run in float64.  Sorting is stable
(ties in conf keep insertion order), which is what the GPU kernels guarantee."""
import numpy as np

F = np.float32
IOUV = np.linspace(0.5, 0.95, 10).astype(F)        # == torch.linspace(0.5, 0.95, 10) in float32 (checked in the tests)


def geometry(shape, img_hw):
    """(h0, w0, gain, padw, padh) with gain and pad rounded to float32, as ATen rounds a Python scalar."""
    H, W = img_hw
    (h0, w0), rp = shape[0], shape[1]
    if rp is None:
        gain = min(H / h0, W / w0)
        pad = (W - w0 * gain) / 2, (H - h0 * gain) / 2
    else:
        gain, pad = rp[0][0], rp[1]
    return F(h0), F(w0), F(gain), F(pad[0]), F(pad[1])


def to_native(xyxy, g):
    h0, w0, gain, pw, ph = g
    b = np.array(xyxy, dtype=F).reshape(-1, 4).copy()
    b[:, [0, 2]] = b[:, [0, 2]] - pw
    b[:, [1, 3]] = b[:, [1, 3]] - ph
    b = b / gain
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], F(0), w0)
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], F(0), h0)
    return b


def iou_row(p, t):
    """IoU of one box against rows t, float32: inter / (area1 + area2 - inter)."""
    iw = np.maximum(np.minimum(p[2], t[:, 2]) - np.maximum(p[0], t[:, 0]), F(0))
    ih = np.maximum(np.minimum(p[3], t[:, 3]) - np.maximum(p[1], t[:, 1]), F(0))
    inter = iw * ih
    a1 = (p[2] - p[0]) * (p[3] - p[1])
    a2 = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    return inter / ((a1 + a2) - inter)


def match_image(dets, labels, img_hw, shape, single_cls=False, iouv=IOUV):
    """dets [n, 6] (xyxy, conf, cls) letterbox pixels; labels [nl, 5] (cls, normalised xywh).  Returns (correct [n, niou] bool,
    conf, pred_cls, info) with info = per-prediction (best label, best IoU, best label already taken)."""
    dets = np.asarray(dets, dtype=F).reshape(-1, 6)
    labels = np.asarray(labels, dtype=F).reshape(-1, 5)
    H, W = img_hw
    g = geometry(shape, img_hw)
    pcls = dets[:, 5].copy()
    if single_cls:
        pcls[:] = 0
    n, nl = len(dets), len(labels)
    correct = np.zeros((n, len(iouv)), bool)
    info = []
    if n == 0 or nl == 0:
        return correct, dets[:, 4].copy(), pcls, info
    xywh = labels[:, 1:5] * np.array([W, H, W, H], dtype=F)
    half_w, half_h = xywh[:, 2] / F(2), xywh[:, 3] / F(2)
    tbox = to_native(np.stack([xywh[:, 0] - half_w, xywh[:, 1] - half_h, xywh[:, 0] + half_w, xywh[:, 1] + half_h], 1), g)
    pbox = to_native(dets[:, :4], g)
    taken = set()
    for r in range(n):                       # rows in order: within a class this is the reference's walk, classes are independent
        ti = np.flatnonzero(labels[:, 0] == pcls[r])
        if len(ti) == 0:
            continue
        ious = iou_row(pbox[r], tbox[ti])
        j = int(np.argmax(ious))              # first index of the max
        best, bi = int(ti[j]), ious[j]
        was_taken = best in taken
        info.append((r, best, float(bi), was_taken, ious, ti))
        if bi > iouv[0] and not was_taken:
            taken.add(best)
            correct[r] = bi > iouv
    return correct, dets[:, 4].copy(), pcls, info


def interp(x, xp, fp, left=None, right=None):
    """np.interp's rule, spelled out: j = last index with xp[j] <= x; exact hit -> fp[j]; else slope * (x - xp[j]) + fp[j]."""
    x, xp, fp = np.asarray(x, np.float64), np.asarray(xp, np.float64), np.asarray(fp, np.float64)
    left = fp[0] if left is None else left
    right = fp[-1] if right is None else right
    out = np.empty_like(x)
    for i, v in enumerate(x):
        j = int(np.searchsorted(xp, v, side="right")) - 1
        if j < 0:
            out[i] = left
        elif j == len(xp) - 1:
            out[i] = fp[j] if v == xp[j] else right
        elif v == xp[j]:
            out[i] = fp[j]
        else:
            out[i] = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (v - xp[j]) + fp[j]
    return out


def average_precision(recall, precision):
    mrec = np.concatenate(([0.0], recall, [recall[-1] + 0.01]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    x = np.linspace(0, 1, 101)
    y = interp(x, mrec, mpre)
    return float(np.sum(np.diff(x) * (y[1:] + y[:-1]) / 2.0))


def ap_per_class(tp, conf, pred_cls, target_cls):
    """(p, r, ap, f1, ap_class) with a stable sort by descending conf."""
    tp = np.asarray(tp, bool)
    conf = np.asarray(conf, np.float32)
    pred_cls = np.asarray(pred_cls, np.float64)
    target_cls = np.asarray(target_cls, np.float64)
    order = np.argsort(-conf, kind="stable")
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    classes = np.unique(target_cls)
    px = np.linspace(0, 1, 1000)
    nc, niou = len(classes), tp.shape[1]
    ap, p, r = np.zeros((nc, niou)), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        n_l = int((target_cls == c).sum())
        if sel.sum() == 0:
            continue
        tpc = np.cumsum(tp[sel].astype(np.int64), 0)
        fpc = np.cumsum(1 - tp[sel].astype(np.int64), 0)
        recall = tpc / (n_l + 1e-16)
        precision = tpc / (tpc + fpc)
        xc = -conf[sel].astype(np.float64)
        r[ci] = interp(-px, xc, recall[:, 0], left=0)
        p[ci] = interp(-px, xc, precision[:, 0], left=1)
        for j in range(niou):
            ap[ci, j] = average_precision(recall[:, j], precision[:, j])
    f1 = 2 * p * r / (p + r + 1e-16)
    mean = f1[0].copy() if nc else np.zeros(1000)
    for ci in range(1, nc):
        mean = mean + f1[ci]
    i = int(np.argmax(mean / max(nc, 1)))
    return p[:, i], r[:, i], ap, f1[:, i], classes.astype(np.int32)


def test_results(tp, conf, pred_cls, target_cls, nc):
    """test.py:226-236 and :291-294: ((mp, mr, map50, map75, map), maps, nt, ap_class)."""
    if len(tp) and np.asarray(tp).any():
        p, r, ap, f1, ap_class = ap_per_class(tp, conf, pred_cls, target_cls)
        ap50, ap75, apm = ap[:, 0], ap[:, 5], ap.mean(1)
        res = (p.mean(), r.mean(), ap50.mean(), ap75.mean(), apm.mean())
        nt = np.bincount(np.asarray(target_cls).astype(np.int64), minlength=nc)
    else:
        res, ap_class, apm, nt = (0.0,) * 5, [], [], np.zeros(1)
    maps = np.zeros(nc) + res[4]
    for i, c in enumerate(ap_class):
        maps[c] = apm[i]
    return tuple(float(v) for v in res), maps, nt, np.asarray(ap_class, np.int32)


def match_case(case):
    """Restated matching over every recorded batch of a fixture case -> (tp, conf, pred_cls, target_cls, infos, per-image)."""
    stats, infos, per_image = [], [], []
    for b in case["batches"]:
        t = b["targets"].numpy()
        for si, d in enumerate(b["dets"]):
            labels = t[t[:, 0] == si, 1:]
            d = d.numpy()
            corr, cf, pc, info = match_image(d, labels, b["img_hw"], b["shapes"][si], case["single_cls"])
            infos.extend(info)
            per_image.append((len(d), len(labels), int(corr[:, 0].sum())))
            if len(d) == 0:
                if len(labels):
                    stats.append((np.zeros((0, 10), bool), np.zeros(0, F), np.zeros(0, F), labels[:, 0].tolist()))
                continue
            stats.append((corr, cf, pc, labels[:, 0].tolist()))
    tp = np.concatenate([s[0] for s in stats], 0)
    conf = np.concatenate([s[1] for s in stats], 0)
    pcls = np.concatenate([s[2] for s in stats], 0)
    tcls = np.array([c for s in stats for c in s[3]], np.float64)
    return tp, conf, pcls, tcls, infos, per_image
