"""Time the GPU ComputeLoss (csrc/loss.hip) against a torch-op restatement of the reference's ComputeLoss on the same GPU tensors.

    python tools/loss_bench.py [--batch 64] [--size 640] [--nc 3] [--nt 4000] [--iters 50]

The bench shape: 64 image pairs at 640 x 640, the FLIR nc = 3 head (grids 80, 40, 20), nt random targets.  Per path: ms
per call of the forward (no autograd graph) and of forward + backward (loss.backward() on heads that require grad), and the
kernel launches per call counted with torch.profiler.  The torch-op version is written from the algorithm (like
tests/loss_ref.py) in float32: boolean-mask filtering, per-level index_put, autograd for the gradient.  Prints one JSON line; every time ends
in a device synchronisation.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msod_amd  # noqa: E402,F401
from msod_amd.utils.loss import ComputeLoss  # noqa: E402

ANCHORS_PX = ((10, 13, 16, 30, 33, 23), (30, 61, 62, 45, 59, 119), (116, 90, 156, 198, 373, 326))
STRIDES = (8.0, 16.0, 32.0)
HYP = dict(box=0.05, obj=1.0, cls=0.5, cls_pw=1.0, obj_pw=1.0, anchor_t=4.0, fl_gamma=0.0, label_smoothing=0.0)


class Det(torch.nn.Module):
    def __init__(self, nc):
        super().__init__()
        self.nc, self.nl, self.na = nc, 3, 3
        self.stride = torch.tensor(STRIDES)
        self.register_buffer("anchors", torch.tensor(ANCHORS_PX).float().view(3, 3, 2) / self.stride.view(-1, 1, 1))


class Stub(torch.nn.Module):
    def __init__(self, nc):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.model = torch.nn.ModuleList([Det(nc)])
        self.hyp, self.gr = dict(HYP), 1.0


def _corners(xy, wh):
    return xy - wh / 2, xy + wh / 2


def _ciou_t(pxy, pwh, txy, twh, eps=1e-7):
    """Complete IoU of predicted and target xywh boxes (torch, float32); the aspect weight is a constant."""
    (p0, p1), (t0, t1) = _corners(pxy, pwh), _corners(txy, twh)
    lo, hi = torch.maximum(p0, t0), torch.minimum(p1, t1)
    overlap = (hi - lo).clamp(min=0).prod(1)
    pw, ph = pwh[:, 0], pwh[:, 1] + eps
    tw, th = twh[:, 0], twh[:, 1] + eps
    iou = overlap / (pw * ph + tw * th - overlap + eps)
    span = torch.maximum(p1, t1) - torch.minimum(p0, t0)
    diag2 = (span ** 2).sum(1) + eps
    centre2 = (((t0 + t1) - (p0 + p1)) ** 2).sum(1) / 4
    aspect = (4 / math.pi ** 2) * (torch.atan(tw / th) - torch.atan(pw / ph)) ** 2
    with torch.no_grad():
        weight = aspect / (aspect - iou + (1 + eps))
    return iou - (centre2 / diag2 + aspect * weight)


SHIFTS = ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (-0.5, 0.0), (0.0, -0.5))


def torch_loss(p, targets, anchors, hyp, gr, balance, nc, pw_cls, pw_obj):
    """The YOLOv5 loss written with torch ops on the tensors' device, in float32, structured like tests/loss_ref.py.  It keeps the
    traits of a torch implementation that are measured here: per-level candidate selection by boolean masks (every
    nonzero() synchronises with the host), a per-level index_put for the objectness targets, autograd for the gradient.
    pw_cls / pw_obj: the BCE positive weights as device tensors [1]."""
    dev = targets.device
    na, nt = anchors.shape[1], targets.shape[0]
    shifts = torch.tensor(SHIFTS, device=dev)
    pair_anchor = torch.arange(na, device=dev).repeat_interleave(nt)      # anchor-major (anchor, target) pairs
    pair = targets.repeat(na, 1)
    box_term, obj_term, cls_term = (p[0].new_zeros(()) for _ in range(3))
    for i, pi in enumerate(p):
        ny, nx = pi.shape[2], pi.shape[3]
        grid = torch.tensor([nx, ny], dtype=torch.float32, device=dev)
        cxy, wh = pair[:, 2:4] * grid, pair[:, 4:6] * grid
        ratio = wh / anchors[i][pair_anchor]
        fits = torch.maximum(ratio, ratio.reciprocal()).amax(1) < hyp["anchor_t"]
        back = grid - cxy
        low = (torch.remainder(cxy, 1.0) < 0.5) & (cxy > 1.0)
        high = (torch.remainder(back, 1.0) < 0.5) & (back > 1.0)
        keep = (fits, fits & low[:, 0], fits & low[:, 1], fits & high[:, 0], fits & high[:, 1])
        rows = [m.nonzero().squeeze(1) for m in keep]                    # candidate order: offset-major, then pair order
        who = torch.cat(rows)
        shift = torch.cat([shifts[o].expand(len(r), 2) for o, r in enumerate(rows)])
        cell = (cxy[who] - shift).long()
        gi, gj = cell[:, 0].clamp(0, nx - 1), cell[:, 1].clamp(0, ny - 1)
        img, anc = pair[who, 0].long(), pair_anchor[who]
        tobj = torch.zeros(pi.shape[:4], device=dev)
        if len(who):
            ps = pi[img, anc, gj, gi]
            pxy = torch.sigmoid(ps[:, :2]) * 2 - 0.5
            pwh = (torch.sigmoid(ps[:, 2:4]) * 2) ** 2 * anchors[i][anc]
            ciou = _ciou_t(pxy, pwh, cxy[who] - torch.stack((gi, gj), 1), wh[who])
            box_term = box_term + (1 - ciou).mean()
            tobj.index_put_((img, anc, gj, gi), (1 - gr) + gr * ciou.detach().clamp(min=0))
            if nc > 1:
                onehot = torch.zeros_like(ps[:, 5:])
                onehot[torch.arange(len(who), device=dev), pair[who, 1].long()] = 1.0
                cls_term = cls_term + F.binary_cross_entropy_with_logits(ps[:, 5:], onehot, pos_weight=pw_cls)
        obj_term = obj_term + F.binary_cross_entropy_with_logits(pi[..., 4], tobj, pos_weight=pw_obj) * balance[i]
    lbox, lobj, lcls = box_term * hyp["box"], obj_term * hyp["obj"], cls_term * hyp["cls"]
    loss = lbox + lobj + lcls
    return loss * p[0].shape[0], torch.stack((lbox, lobj, lcls, loss)).detach()


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as ex:  # the profiler is optional here
        return f"n/a ({type(ex).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--nc", type=int, default=3)
    ap.add_argument("--nt", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    B, S, nc, nt = a.batch, a.size, a.nc, a.nt
    p = [torch.from_numpy((g.standard_normal((B, 3, S // int(s), S // int(s), nc + 5)) * 1.5).astype(np.float32)).to(dev) for s in STRIDES]
    t = torch.from_numpy(np.stack([g.integers(0, B, nt), g.integers(0, nc, nt), g.uniform(0.02, 0.98, nt), g.uniform(0.02, 0.98, nt),
                                   g.uniform(0.01, 0.4, nt), g.uniform(0.01, 0.4, nt)], 1).astype(np.float32)).to(dev)
    stub = Stub(nc).to(dev)
    cl = ComputeLoss(stub)
    anchors = stub.model[-1].anchors
    ps = [x.clone().requires_grad_(True) for x in p]
    pw_cls = torch.tensor([HYP["cls_pw"]], device=dev)
    pw_obj = torch.tensor([HYP["obj_pw"]], device=dev)

    def gpu_fwd():
        return cl(p, t)

    def gpu_fb():
        loss, _ = cl(ps, t)
        loss.backward()

    def ref_fwd():
        with torch.no_grad():
            return torch_loss(p, t, anchors, HYP, 1.0, [4.0, 1.0, 0.4], nc, pw_cls, pw_obj)

    def ref_fb():
        loss, _ = torch_loss(ps, t, anchors, HYP, 1.0, [4.0, 1.0, 0.4], nc, pw_cls, pw_obj)
        loss.backward()

    items_gpu, items_ref = gpu_fwd()[1].cpu(), ref_fwd()[1].cpu()
    out = {"shape": {"batch": B, "size": S, "nc": nc, "nt": nt},
           "items_gpu": [round(float(x), 6) for x in items_gpu], "items_torch": [round(float(x), 6) for x in items_ref],
           "gpu_fwd_ms": round(timed(gpu_fwd, a.iters), 4), "gpu_fwd_bwd_ms": round(timed(gpu_fb, a.iters), 4),
           "torch_fwd_ms": round(timed(ref_fwd, a.iters), 4), "torch_fwd_bwd_ms": round(timed(ref_fb, a.iters), 4),
           "gpu_fwd_launches": launches(gpu_fwd), "gpu_fwd_bwd_launches": launches(gpu_fb),
           "torch_fwd_launches": launches(ref_fwd), "torch_fwd_bwd_launches": launches(ref_fb)}
    out["speedup_fwd"] = round(out["torch_fwd_ms"] / out["gpu_fwd_ms"], 2)
    out["speedup_fwd_bwd"] = round(out["torch_fwd_bwd_ms"] / out["gpu_fwd_bwd_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
