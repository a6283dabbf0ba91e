"""Time the GPU mAP evaluator against a test.py-style statistics loop on GPU tensors.

    python tools/eval_bench.py [--batches 16] [--reps 5]

Per 64-image batch (300 detections and 20 labels per image, 3 classes): match_batch + DetectionEvaluator.update
versus a per-image / per-class Python loop in the style of test.py:132-218 (written here from the rules, on the
same GPU tensors).  Then DetectionEvaluator.compute() (ap_per_class) for 1013 x 300 detections with 3 classes and
5000 x 300 with 80 classes, taking turns with DetectionEvaluator.curves() (cft_eval_curves: the same sort, one more walk and a
larger device-to-host copy) on the same statistics.  The confusion / export leg times, on the same 64-image batch and alternating the sides round by
round: update() without and with confusion=True, a per-image process_batch loop in the reference's style (written here from
the algorithm, on GPU tensors), the two confusion launches alone, the two matching launches alone, and export_batch with its
device-to-host copy.  Both update() legs include their evaluator's reset(): the plain one reserves its statistics buffers again,
the confusion one also zeroes its matrix in place (nothing is allocated for it after the first round).  Prints one JSON line; every time ends in a device synchronisation.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msod_amd  # noqa: E402,F401
from msod_amd.utils.metrics import ConfusionMatrix, DetectionEvaluator, IOUV, export_batch, match_batch  # noqa: E402


def make_batch(g, B, nd, nl, nc, H, W, dev):
    tg, dets, shapes = [], torch.zeros((B, nd, 6)), []
    for b in range(B):
        lab = np.column_stack([g.integers(0, nc, nl), g.uniform(0.2, 0.8, (nl, 2)), g.uniform(0.05, 0.3, (nl, 2))])
        tg += [(b, *l) for l in lab]
        k = g.integers(0, nl, nd)
        cxy = lab[k, 1:3] * [W, H] + g.normal(0, 8, (nd, 2))
        wh = lab[k, 3:5] * [W, H] * np.exp(g.normal(0, 0.25, (nd, 2)))
        cls = np.where(g.random(nd) < 0.8, lab[k, 0], g.integers(0, nc, nd))
        dets[b] = torch.from_numpy(np.column_stack([cxy - wh / 2, cxy + wh / 2, np.sort(g.random(nd))[::-1], cls]).astype(np.float32))
        h0, w0 = 512, 640
        r = min(H / h0, W / w0)
        shapes.append(((h0, w0), ((r, r), ((W - w0 * r) / 2, (H - h0 * r) / 2))))
    return dets.to(dev), torch.full((B,), nd, dtype=torch.int32, device=dev), torch.tensor(tg, dtype=torch.float32, device=dev), shapes


def _box_iou(a, b):
    area = lambda x: (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])  # noqa: E731
    inter = (torch.min(a[:, None, 2:], b[:, 2:]) - torch.max(a[:, None, :2], b[:, :2])).clamp(0).prod(2)
    return inter / (area(a)[:, None] + area(b) - inter)


def _native(boxes, img_hw, shape):
    gain, pad = shape[1][0][0], shape[1][1]
    boxes[:, [0, 2]] -= pad[0]
    boxes[:, [1, 3]] -= pad[1]
    boxes[:, :4] /= gain
    boxes[:, [0, 2]] = boxes[:, [0, 2]].clamp(0, shape[0][1])
    boxes[:, [1, 3]] = boxes[:, [1, 3]].clamp(0, shape[0][0])
    return boxes


def loop_stats(dets, counts, targets, img_hw, shapes):
    """The per-image, per-class statistics loop of test.py, in its style (nonzero, .item() per match), on GPU tensors."""
    H, W = img_hw
    iouv = IOUV.to(dets.device)
    t = targets.clone()
    t[:, 2:] *= torch.tensor([W, H, W, H], device=dets.device)
    stats = []
    for si in range(dets.shape[0]):
        pred = dets[si, :int(counts[si])]
        labels = t[t[:, 0] == si, 1:]
        correct = torch.zeros(pred.shape[0], 10, dtype=torch.bool, device=dets.device)
        if len(labels):
            predn = _native(pred[:, :4].clone(), img_hw, shapes[si])
            xy, wh = labels[:, 1:3], labels[:, 3:5]
            tbox = _native(torch.cat([xy - wh / 2, xy + wh / 2], 1), img_hw, shapes[si])
            taken = set()
            for c in torch.unique(labels[:, 0]):
                ti = (labels[:, 0] == c).nonzero().view(-1)
                pi = (pred[:, 5] == c).nonzero().view(-1)
                if pi.shape[0]:
                    ious, i = _box_iou(predn[pi], tbox[ti]).max(1)
                    for j in (ious > iouv[0]).nonzero():
                        d = ti[i[j]].item()
                        if d not in taken:
                            taken.add(d)
                            correct[pi[j]] = ious[j] > iouv
        stats.append((correct.cpu(), pred[:, 4].cpu(), pred[:, 5].cpu(), labels[:, 0].tolist()))
    return stats


def loop_confusion(dets, counts, targets, img_hw, shapes, nc, conf=0.25, iou_thres=0.45):
    """A per-image confusion matrix in the reference's style (boolean filter, torch.where, argsort / np.unique on the host, one
    Python loop over labels and one over detections), on GPU tensors."""
    H, W = img_hw
    t = targets.clone()
    t[:, 2:] *= torch.tensor([W, H, W, H], device=dets.device)
    matrix = np.zeros((nc + 1, nc + 1))
    for si in range(dets.shape[0]):
        pred = dets[si, :int(counts[si])]
        labels = t[t[:, 0] == si, 1:]
        if not len(pred) or not len(labels):
            continue
        predn = pred.clone()
        _native(predn[:, :4], img_hw, shapes[si])
        xy, wh = labels[:, 1:3], labels[:, 3:5]
        tbox = _native(torch.cat([xy - wh / 2, xy + wh / 2], 1), img_hw, shapes[si])
        d = predn[predn[:, 4] > conf]
        gtc, dc = labels[:, 0].int(), d[:, 5].int()
        iou = _box_iou(tbox, d[:, :4])
        x = torch.where(iou > iou_thres)
        if x[0].shape[0]:
            mt = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()
            mt = mt[mt[:, 2].argsort()[::-1]]
            mt = mt[np.unique(mt[:, 1], return_index=True)[1]]
            mt = mt[mt[:, 2].argsort()[::-1]]
            mt = mt[np.unique(mt[:, 0], return_index=True)[1]]
        else:
            mt = np.zeros((0, 3))
        m0, m1 = mt[:, 0].astype(int), mt[:, 1].astype(int)
        for i, gc in enumerate(gtc):
            j = m0 == i
            if j.sum() == 1:
                matrix[dc[m1[j]], gc] += 1
            else:
                matrix[nc, gc] += 1
        if len(mt):
            for i, c in enumerate(dc):
                if not (m1 == i).any():
                    matrix[c, nc] += 1
    return matrix


def alternated(fns, rounds, warm=3):
    """Median seconds of each callable, the callables taking turns round by round (drift hits every side alike)."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    return {k: float(np.median(v)) for k, v in ts.items()}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs a GPU")
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    H, W = 512, 640
    batch = make_batch(g, 64, 300, 20, 3, H, W, dev)
    ev = DetectionEvaluator(3)

    def gpu_step():
        ev.reset()
        ev.update(*batch[:3], (H, W), batch[3])
    res = {"metric": "eval_bench"}
    res["update_ms_per_64"] = timed(gpu_step, a.reps * 4) * 1e3
    res["loop_ms_per_64"] = timed(lambda: loop_stats(*batch[:3], (H, W), batch[3]), 2) * 1e3
    # confusion / export leg
    ev_cm = DetectionEvaluator(3, confusion=True)
    cm = ConfusionMatrix(3)

    def cm_step():
        ev_cm.reset()
        ev_cm.update(*batch[:3], (H, W), batch[3])
    med = alternated({"update_ms_per_64_alt": gpu_step, "update_confusion_ms_per_64": cm_step,
                      "confusion_only_ms_per_64": lambda: cm.update(*batch[:3], (H, W), batch[3]),
                      "match_only_ms_per_64": lambda: match_batch(*batch[:3], (H, W), batch[3]),
                      "export_d2h_ms_per_64": lambda: export_batch(*batch[:2], (H, W), batch[3]).cpu()}, a.reps * 8)
    res.update({k: v * 1e3 for k, v in med.items()})
    res["confusion_loop_ms_per_64"] = timed(lambda: loop_confusion(*batch[:3], (H, W), batch[3], 3), 2) * 1e3
    cm1 = ConfusionMatrix(3)
    cm1.update(*batch[:3], (H, W), batch[3])
    res["confusion_matches_loop"] = bool(np.array_equal(cm1.matrix, loop_confusion(*batch[:3], (H, W), batch[3], 3)))
    for name, n_img, nc in (("flir_1013x300_nc3", 1013, 3), ("coco_5000x300_nc80", 5000, 80)):
        ev = DetectionEvaluator(nc)
        b64 = make_batch(g, 64, 300, 20, nc, H, W, dev)
        left = n_img
        while left > 0:
            k = min(64, left)
            ev.update(b64[0][:k].contiguous(), b64[1][:k].contiguous(), b64[2][b64[2][:, 0] < k], (H, W), b64[3][:k])
            left -= k
        torch.cuda.synchronize()
        med = alternated({f"compute_ms_{name}": ev.compute, f"curves_ms_{name}": ev.curves}, a.reps, warm=1)
        res.update({k: v * 1e3 for k, v in med.items()})
        res[f"map_{name}"] = ev.compute().map
    print(json.dumps(res))


if __name__ == "__main__":
    main()
