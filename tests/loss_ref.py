"""Host restatement of the YOLOv5 ComputeLoss (build_targets, CIoU box loss, class / objectness BCE with the focal option)
and of its gradient, written from the published algorithm for the tests of csrc/loss.hip.

build_targets' decisions are taken in float32 with numpy (IEEE division, fmod-based remainder), as the reference takes them on
torch float32 tensors; the losses are then computed in float64 with torch autograd, which also gives the gradient.  Targets
whose image index is outside [0, B) (and, with nc > 1, whose class is outside [0, nc)) are skipped after the anchor test, the
rule this package defines where the reference would raise.
"""
import numpy as np
import torch

OFFSETS = ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (-0.5, 0.0), (0.0, -0.5))
F32 = np.float32


def _rem1(v):
    m = np.fmod(v, F32(1))
    return np.where((m != 0) & (m < 0), m + F32(1), m)


def build_targets(shapes, targets, anchors, anchor_t, nc):
    """shapes: the [B, na, ny, nx, no] of every level; targets [nt, 6]; anchors [nl, na, 2] grid units.
    Returns per level a dict of int64 b, a, gj, gi, c, float32 tbox [n, 4], in candidate order, and the error bits."""
    t = np.asarray(targets, np.float32).reshape(-1, 6)
    anchors = np.asarray(anchors, np.float32)
    nt, err, out = t.shape[0], 0, []
    for i, shp in enumerate(shapes):
        B, na, ny, nx = shp[0], shp[1], shp[2], shp[3]
        gx, gy = F32(nx), F32(ny)
        a_of = np.repeat(np.arange(na), nt)
        tt = np.tile(t, (na, 1))
        x, y, w, h = tt[:, 2] * gx, tt[:, 3] * gy, tt[:, 4] * gx, tt[:, 5] * gy
        anc = anchors[i][a_of]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r0, r1 = w / anc[:, 0], h / anc[:, 1]
            keep = np.maximum(np.maximum(r0, F32(1) / r0), np.maximum(r1, F32(1) / r1)) < F32(anchor_t)
        bad_img = keep & ~((tt[:, 0] > -1) & (tt[:, 0] < B))
        err |= 1 if bad_img.any() else 0
        keep &= ~bad_img
        if nc > 1:
            bad_cls = keep & ~((tt[:, 1] > -1) & (tt[:, 1] < nc))
            err |= 2 if bad_cls.any() else 0
            keep &= ~bad_cls
        xi, yi = gx - x, gy - y
        sel = [keep, keep & (_rem1(x) < 0.5) & (x > 1), keep & (_rem1(y) < 0.5) & (y > 1),
               keep & (_rem1(xi) < 0.5) & (xi > 1), keep & (_rem1(yi) < 0.5) & (yi > 1)]
        parts = []
        for (ox, oy), s in zip(OFFSETS, sel):
            k = np.nonzero(s)[0]
            gi = np.trunc(x[k] - F32(ox)).astype(np.int64).clip(0, nx - 1)
            gj = np.trunc(y[k] - F32(oy)).astype(np.int64).clip(0, ny - 1)
            tbox = np.stack([x[k] - gi.astype(np.float32), y[k] - gj.astype(np.float32), w[k], h[k]], 1).astype(np.float32)
            c = tt[k, 1].astype(np.int64) if nc > 1 else np.zeros(len(k), np.int64)
            parts.append((tt[k, 0].astype(np.int64), a_of[k], gj, gi, c, tbox))
        cat = [np.concatenate([p[j] for p in parts]) for j in range(6)]
        out.append(dict(b=cat[0], a=cat[1], gj=cat[2], gi=cat[3], c=cat[4], tbox=cat[5].reshape(-1, 4)))
    return out, err


def _bce(x, y, pw, gamma):
    """BCE with logits and positive weight pw, elementwise; focal modulation (alpha 0.25) when gamma > 0."""
    lw = 1.0 + (pw - 1.0) * y
    loss = (1.0 - y) * x + lw * (torch.clamp(-x, min=0) + torch.log1p(torch.exp(-x.abs())))
    if gamma > 0:
        p = torch.sigmoid(x)
        pt = y * p + (1.0 - y) * (1.0 - p)
        loss = loss * (y * 0.25 + (1.0 - y) * 0.75) * (1.0 - pt) ** gamma
    return loss


def _ciou(p4, t4, eps=1e-7):
    """Complete IoU of xywh boxes; the aspect weight alpha is a constant (no gradient)."""
    ax1, ax2 = p4[:, 0] - p4[:, 2] / 2, p4[:, 0] + p4[:, 2] / 2
    ay1, ay2 = p4[:, 1] - p4[:, 3] / 2, p4[:, 1] + p4[:, 3] / 2
    bx1, bx2 = t4[:, 0] - t4[:, 2] / 2, t4[:, 0] + t4[:, 2] / 2
    by1, by2 = t4[:, 1] - t4[:, 3] / 2, t4[:, 1] + t4[:, 3] / 2
    inter = (torch.min(ax2, bx2) - torch.max(ax1, bx1)).clamp(0) * (torch.min(ay2, by2) - torch.max(ay1, by1)).clamp(0)
    w1, h1 = ax2 - ax1, ay2 - ay1 + eps
    w2, h2 = bx2 - bx1, by2 - by1 + eps
    iou = inter / (w1 * h1 + w2 * h2 - inter + eps)
    c2 = (torch.max(ax2, bx2) - torch.min(ax1, bx1)) ** 2 + (torch.max(ay2, by2) - torch.min(ay1, by1)) ** 2 + eps
    rho2 = ((bx1 + bx2 - ax1 - ax2) ** 2 + (by1 + by2 - ay1 - ay2) ** 2) / 4
    v = (4 / np.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    with torch.no_grad():
        alpha = v / (v - iou + (1 + eps))
    return iou - (rho2 / c2 + v * alpha)


def compute(p, targets, anchors, hyp, gr, balance, autobalance=False, ssi=0, grad=True):
    """p: list of float32 arrays / tensors [B, na, ny, nx, nc + 5].  Returns dict(loss, items (float64 [4]), grads (list of
    float64 arrays or None), balance (the updated list), cand (build_targets' output), err)."""
    p = [torch.as_tensor(np.asarray(pi.detach().cpu() if isinstance(pi, torch.Tensor) else pi, np.float32)).double() for pi in p]
    for pi in p:
        pi.requires_grad_(grad)
    nc = p[0].shape[4] - 5
    cp, cn = float(F32(1.0 - 0.5 * hyp.get("label_smoothing", 0.0))), float(F32(0.5 * hyp.get("label_smoothing", 0.0)))
    anchors = np.asarray(anchors.detach().cpu() if isinstance(anchors, torch.Tensor) else anchors, np.float32)
    cand, err = build_targets([tuple(pi.shape) for pi in p], targets, anchors, hyp["anchor_t"], nc)
    gamma = float(hyp["fl_gamma"])
    balance = list(balance)
    lbox = lobj = lcls = torch.zeros((), dtype=torch.float64)
    for i, pi in enumerate(p):
        c = cand[i]
        n = len(c["b"])
        tobj = torch.zeros(pi.shape[:4], dtype=torch.float64)
        if n:
            b, a, gj, gi = (torch.from_numpy(c[k]) for k in ("b", "a", "gj", "gi"))
            ps = pi[b, a, gj, gi]
            anc = torch.from_numpy(anchors[i][c["a"]]).double()
            pxy = torch.sigmoid(ps[:, :2]) * 2 - 0.5
            pwh = (torch.sigmoid(ps[:, 2:4]) * 2) ** 2 * anc
            ciou = _ciou(torch.cat((pxy, pwh), 1), torch.from_numpy(c["tbox"]).double())
            lbox = lbox + (1.0 - ciou).mean()
            # the objectness target of a cell is the one of its last candidate
            val = ((1.0 - gr) + gr * ciou.detach().float().clamp(0)).float().double()
            flat = ((b * pi.shape[1] + a) * pi.shape[2] + gj) * pi.shape[3] + gi
            last = np.full(int(np.prod(pi.shape[:4])), -1, np.int64)
            np.maximum.at(last, flat.numpy(), np.arange(n))
            cells = np.nonzero(last >= 0)[0]
            tobj.view(-1)[torch.from_numpy(cells)] = val[torch.from_numpy(last[cells])]
            if nc > 1:
                t = torch.full((n, nc), cn, dtype=torch.float64)
                t[torch.arange(n), torch.from_numpy(c["c"])] = cp
                lcls = lcls + _bce(ps[:, 5:], t, hyp["cls_pw"], gamma).mean()
        obji = _bce(pi[..., 4], tobj, hyp["obj_pw"], gamma).mean()
        lobj = lobj + obji * balance[i]
        if autobalance:
            balance[i] = balance[i] * 0.9999 + 0.0001 / obji.item()
    if autobalance:
        balance = [x / balance[ssi] for x in balance]
    lbox, lobj, lcls = lbox * hyp["box"], lobj * hyp["obj"], lcls * hyp["cls"]
    loss = lbox + lobj + lcls
    bs = p[0].shape[0]
    grads = None
    if grad:
        (loss * bs).backward()
        grads = [pi.grad.numpy() for pi in p]
    items = np.array([lbox.item(), lobj.item(), lcls.item(), loss.item()])
    return dict(loss=loss.item() * bs, items=items, grads=grads, balance=balance, cand=cand, err=err)
