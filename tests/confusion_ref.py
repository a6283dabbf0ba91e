"""Host restatement of the confusion matrix of test.py's ``plots=True`` (ConfusionMatrix.process_batch) and of the box values of
save_txt / save_json, written from the rules alone.  The oracle of tests/test_confusion_host.py (against the recorded reference)
and of the constructed GPU cases.

Rules: detections with conf > 0.25 are kept, in order; classes are truncated toward zero; a (label, detection) pair is a
candidate if its float32 IoU > 0.45; each detection keeps its highest-IoU label, then each label keeps its highest-IoU detection
among those that kept it; class plays no part.  A matched label counts at [detection class, label class], any other label at
[nc, label class]; a kept detection in no match counts at [its class, nc], but only if the image has a match.  Exactly equal
IoUs: the lowest label index wins, then the lowest detection index.  An image counts only if it has labels and detections."""
import numpy as np

import eval_ref

F = np.float32


def iou_matrix(lab, det):
    """[M, N] float32 IoU of label boxes [M, 4] with detection boxes [N, 4] (xyxy): inter / (area + area - inter)."""
    out = np.zeros((len(lab), len(det)), F)
    for j, d in enumerate(det):
        out[:, j] = eval_ref.iou_row(d, lab)
    return out


def process_image(dets, labels, nc, conf=0.25, iou_thres=0.45, single_cls=False):
    """dets [N, 6] = xyxy, conf, class; labels [M, 5] = class, xyxy; native space.  Returns the image's (nc+1, nc+1) int64 counts
    and the number of skipped (out of range) classes."""
    m = np.zeros((nc + 1, nc + 1), np.int64)
    dets = np.asarray(dets, F).reshape(-1, 6)
    labels = np.asarray(labels, F).reshape(-1, 5)
    bad = 0
    if len(dets) == 0 or len(labels) == 0:
        return m, bad
    dets = dets[dets[:, 4] > F(conf)]
    gc = np.trunc(labels[:, 0]).astype(np.int64)
    dc = np.zeros(len(dets), np.int64) if single_cls else np.trunc(dets[:, 5]).astype(np.int64)
    iou = iou_matrix(labels[:, 1:], dets[:, :4])
    kept = np.full(len(dets), -1)                      # the label each detection keeps
    for j in range(len(dets)):
        best = F(0)
        for i in range(len(labels)):
            if iou[i, j] > F(iou_thres) and (kept[j] < 0 or iou[i, j] > best):      # strict: the lowest label index stays on a tie
                kept[j], best = i, iou[i, j]
    winner = np.full(len(labels), -1)                  # the detection each label keeps
    for i in range(len(labels)):
        best = F(0)
        for j in range(len(dets)):
            if kept[j] == i and (winner[i] < 0 or iou[i, j] > best):                # strict: the lowest detection index stays
                winner[i], best = j, iou[i, j]
    ok = lambda c: 0 <= c < nc  # noqa: E731
    for i in range(len(labels)):
        if winner[i] >= 0 and not ok(dc[winner[i]]):
            bad += 1
        elif not ok(gc[i]):
            bad += 1
        else:
            m[dc[winner[i]] if winner[i] >= 0 else nc, gc[i]] += 1
    if (winner >= 0).any():
        for j in range(len(dets)):
            if kept[j] >= 0 and winner[kept[j]] == j:
                continue
            if ok(dc[j]):
                m[dc[j], nc] += 1
            else:
                bad += 1
    return m, bad


def native_labels(labels, img_hw, shape):
    """labels [M, 5] = class, normalised xywh -> class, native xyxy (float32, the order of test.py:126, :191-192)."""
    labels = np.asarray(labels, F).reshape(-1, 5)
    H, W = img_hw
    xywh = labels[:, 1:5] * np.array([W, H, W, H], dtype=F)
    hw, hh = xywh[:, 2] / F(2), xywh[:, 3] / F(2)
    box = eval_ref.to_native(np.stack([xywh[:, 0] - hw, xywh[:, 1] - hh, xywh[:, 0] + hw, xywh[:, 1] + hh], 1), eval_ref.geometry(shape, img_hw))
    return np.concatenate([labels[:, :1], box], 1)


def native_dets(dets, img_hw, shape):
    dets = np.asarray(dets, F).reshape(-1, 6).copy()
    dets[:, :4] = eval_ref.to_native(dets[:, :4], eval_ref.geometry(shape, img_hw))
    return dets


def batch_matrix(dets, targets, img_hw, shapes, nc, single_cls=False, conf=0.25, iou_thres=0.45):
    """One batch: dets = per-image [n, 6] arrays in letterbox pixels, targets [nt, 6] normalised.  Returns (matrix, skipped)."""
    m, bad = np.zeros((nc + 1, nc + 1), np.int64), 0
    t = np.asarray(targets, F).reshape(-1, 6)
    for si, d in enumerate(dets):
        lab = t[t[:, 0] == si, 1:]
        mi, b = process_image(native_dets(d, img_hw, shapes[si]), native_labels(lab, img_hw, shapes[si]), nc, conf, iou_thres, single_cls)
        m += mi
        bad += b
    return m, bad


def export_values(dets, img_hw, shape, single_cls=False):
    """Per detection of one image: (class, conf, normalised xywh of save_txt, top-left xywh of save_json), float32 chains:
    centre = (x1 + x2) / 2, size = x2 - x1, / (w0, h0, w0, h0); left = centre - size / 2."""
    d = native_dets(dets, img_hw, shape)
    h0, w0 = F(shape[0][0]), F(shape[0][1])
    cx, cy = (d[:, 0] + d[:, 2]) / F(2), (d[:, 1] + d[:, 3]) / F(2)
    w, h = d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]
    nxywh = np.stack([cx / w0, cy / h0, w / w0, h / h0], 1)
    tl = np.stack([cx - w / F(2), cy - h / F(2), w, h], 1)
    cls = np.zeros(len(d), F) if single_cls else d[:, 5]
    return cls, d[:, 4], nxywh, tl
