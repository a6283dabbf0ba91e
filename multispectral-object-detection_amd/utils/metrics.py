"""mAP statistics of the reference's ``test.py`` on the GPU (the step after batched NMS).

The reference walks images, then classes, in Python (``test.py:132-218``: ``nonzero()`` and one ``.item()`` per
matched detection) and then runs ``ap_per_class`` (``utils/metrics.py:18-108``) in numpy.  Here both are HIP kernels
(``csrc/metrics.hip``):

* ``match_batch``          one batch's ``batched_nms`` output against its labels (``cft_eval_match``);
* ``ap_per_class``         the reference's function, same signature and return value (``cft_eval_ap``);
* ``DetectionEvaluator``   accumulates batches on the device without host synchronisation and computes
                           ``test.py``'s metrics with one synchronisation;
* ``ConfusionMatrix``      the reference's class (``utils/metrics.py:111-183``): ``process_batch`` per image as there, and a
                           batched ``update`` on the ``batched_nms`` output (``cft_eval_confusion``), accumulated on the device;
* ``curves_per_class``     the curves behind it (``cft_eval_curves``, ``csrc/curves.hip``): what ``ap_per_class(plot=True)`` hands to the
                           reference's plot functions, plus the miss rate over false positives per image and the log-average
                           miss rate; ``DetectionEvaluator.curves()`` gives the same from the accumulated batches, and
                           ``plot_pr_curve`` / ``plot_mc_curve`` / ``plot_mr_curve`` draw them with matplotlib on the host;
* ``export_batch``         the box values of ``save_txt`` / ``save_json`` for every detection slot (``cft_eval_export``);
                           ``txt_line`` and ``json_entry`` format them as ``test.py:156-158`` and ``:179-182`` do.

Every rule is the reference's: float32 box arithmetic as ATen does it, float64 curves as numpy does them.

The confusion matrix keeps the reference's quirks: only an image with labels and NMS detections counts (``test.py:140-143``,
``:186``); detections are kept if ``conf > 0.25`` and pairs are candidates if ``iou > 0.45`` (both strict); each detection
keeps its highest-IoU label, then each label its highest-IoU detection among those that kept it, whatever their classes;
unmatched kept detections count as background only in an image that has a match (``if n:``, ``utils/metrics.py:154``); without
a kept detection every label of the image counts as background.  The reference leaves exactly equal IoUs to numpy's unstable
argsort; here the lowest label index wins, then the lowest detection index.  A class outside ``[0, nc)`` is not counted and
makes ``.matrix`` raise.
"""
import ctypes
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch

from .. import _lib
from ..ops import _require_cuda, _stream

IOUV = torch.linspace(0.5, 0.95, 10)         # test.py:76, built on the host in float32 as there
NIOU = IOUV.numel()
PX = np.linspace(0, 1, 1000)                 # utils/metrics.py:40
XG = np.linspace(0, 1, 101)                  # utils/metrics.py:97

_grid_cache = {}


def _to_device(t, device):
    """Host tensor -> device without a blocking copy (pinned staging): keeps update() free of host synchronisation."""
    if t.device == device:
        return t
    if t.device.type != "cpu":
        return t.to(device)
    return t.contiguous().pin_memory().to(device, non_blocking=True)


def _grids(device):
    g = _grid_cache.get(device)
    if g is None:
        g = _grid_cache[device] = (_to_device(torch.from_numpy(PX), device), _to_device(torch.from_numpy(XG), device))
    return g


def geometry(shapes, img_hw):
    """Per-image float32 [h0, w0, gain, padw, padh] of scale_coords (reference utils/general.py:353-366), from test.py's
    ``shapes[si] = ((h0, w0), ratio_pad)``.  ratio_pad None: gain and pad from the shapes, in double, as the reference."""
    H, W = int(img_hw[0]), int(img_hw[1])
    g = np.empty((len(shapes), 5), np.float64)
    for i, s in enumerate(shapes):
        (h0, w0), rp = s[0], s[1] if len(s) > 1 else None
        h0, w0 = float(h0), float(w0)
        if rp is None:
            gain = min(H / h0, W / w0)
            pad = (W - w0 * gain) / 2, (H - h0 * gain) / 2
        else:
            gain = float(rp[0][0])
            pad = float(rp[1][0]), float(rp[1][1])
        g[i] = (h0, w0, gain, pad[0], pad[1])
    return torch.from_numpy(g.astype(np.float32))      # ATen rounds the Python scalars to float32


def _pack_dets(dets, counts, device):
    """(dets [B, max_det, 6], counts [B]) or the list form of non_max_suppression -> device tensors, no host sync."""
    if isinstance(dets, (list, tuple)):
        if counts is not None:
            raise ValueError("match: give counts only with a dets tensor, not with the list form")
        if len(dets) == 0:
            raise ValueError("match: empty batch")
        ns = [int(d.shape[0]) for d in dets]
        packed = torch.zeros((len(dets), max(1, max(ns)), 6), dtype=torch.float32, device=device)
        for i, d in enumerate(dets):
            if d.dim() != 2 or d.shape[1] != 6:
                raise ValueError(f"match: detections of image {i} must be [n, 6], got {tuple(d.shape)}")
            if ns[i]:
                packed[i, :ns[i]].copy_(d)
        return packed, _to_device(torch.tensor(ns, dtype=torch.int32), device)
    if not isinstance(dets, torch.Tensor) or dets.dim() != 3 or dets.shape[2] != 6 or dets.shape[0] == 0 or dets.shape[1] == 0:
        raise ValueError(f"match: dets must be a [B, max_det, 6] tensor with B, max_det >= 1, got {getattr(dets, 'shape', type(dets))}")
    if counts is None or not isinstance(counts, torch.Tensor) or counts.shape != (dets.shape[0],):
        raise ValueError("match: counts must be a [B] tensor (the batched_nms output)")
    _require_cuda(dets, "match_batch")
    _require_cuda(counts, "match_batch")
    if dets.dtype != torch.float32 or not dets.is_contiguous():
        raise ValueError("match: dets must be contiguous float32 (the batched_nms output)")
    return dets, counts.to(torch.int32).contiguous()


@dataclass
class MatchResult:
    """Device tensors of one batch, slot (b, r) = detection r of image b (rows r >= counts[b] are empty: pred_cls -1)."""
    correct: torch.Tensor      # bool [B, max_det, niou]
    conf: torch.Tensor         # float32 [B, max_det]
    pred_cls: torch.Tensor     # int32 [B, max_det]
    counts: torch.Tensor       # int32 [B]
    tcls: torch.Tensor         # int32 [nt], label classes grouped by image in target order
    nl: torch.Tensor           # int32 [B], labels per image

    def to_stats(self):
        """test.py's ``stats`` entries of the batch (:140-143, :221): (correct, conf, pred_cls, tcls) per image, in image order,
        skipping images without detections and labels.  Copies to the host (synchronises)."""
        correct, conf, pcls = self.correct.cpu(), self.conf.cpu(), self.pred_cls.cpu()
        counts, nl, tcls = self.counts.cpu().tolist(), self.nl.cpu().tolist(), self.tcls.cpu().tolist()
        stats, l0 = [], 0
        for b, (n, m) in enumerate(zip(counts, nl)):
            tc = [float(c) for c in tcls[l0:l0 + m]]
            l0 += m
            if n == 0:
                if m:
                    stats.append((torch.zeros(0, correct.shape[2], dtype=torch.bool), torch.Tensor(), torch.Tensor(), tc))
                continue
            stats.append((correct[b, :n], conf[b, :n], pcls[b, :n].float(), tc))
        return stats


def _match(dets, counts, targets, img_hw, shapes, single_cls, tp_bits, conf, pcls, correct, label_hist, nc, tcls, nl):
    B, max_det = dets.shape[0], dets.shape[1]
    device = dets.device
    if not isinstance(targets, torch.Tensor) or targets.dim() != 2 or targets.shape[1] != 6:
        raise ValueError(f"match: targets must be an [nt, 6] tensor (image, class, x, y, w, h), got {getattr(targets, 'shape', type(targets))}")
    if len(shapes) != B:
        raise ValueError(f"match: {len(shapes)} shapes for a batch of {B} images")
    H, W = int(img_hw[0]), int(img_hw[1])
    if H <= 0 or W <= 0:
        raise ValueError(f"match: bad image size {img_hw}")
    targets = _to_device(targets.float(), device).contiguous()
    geom = _to_device(geometry(shapes, img_hw), device)
    nt = targets.shape[0]
    lib = _lib.load()
    ws = torch.empty((lib.cft_eval_match_workspace_bytes(B, nt),), dtype=torch.uint8, device=device)
    iouv = np.ascontiguousarray(IOUV.numpy(), dtype=np.float32)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    st = lib.cft_eval_match(dets.data_ptr(), counts.data_ptr(), B, max_det, ptr(targets) if nt else None, nt, H, W, geom.data_ptr(),
                            iouv.ctypes.data, NIOU, int(bool(single_cls)), ws.data_ptr(), ws.numel(), ptr(correct), tp_bits.data_ptr(),
                            ptr(conf), ptr(pcls), ptr(label_hist), int(nc), ptr(tcls), ptr(nl), _stream())
    _lib.check(st, "cft_eval_match")


def match_batch(dets, counts, targets, img_hw, shapes, single_cls=False, out=None):
    """Match one batch's detections to its labels on the GPU (test.py:132-218).

    dets, counts: the ``batched_nms`` output (or ``non_max_suppression``'s list, with counts=None); targets [nt, 6] as the
    dataloader yields them (normalised xywh); img_hw = the letterboxed (height, width); shapes = the dataloader's shapes.
    Returns a ``MatchResult``; ``.to_stats()`` gives test.py's per-image ``stats`` entries.  ``out`` (optional) is a
    ``MatchResult`` whose tensors are written instead of fresh ones."""
    device = dets[0].device if isinstance(dets, (list, tuple)) and len(dets) else getattr(dets, "device", None)
    if device is None or device.type != "cuda":
        raise RuntimeError("match_batch: detections must be on the GPU (this package has no CPU path)")
    dets, counts = _pack_dets(dets, counts, device)
    B, max_det = dets.shape[0], dets.shape[1]
    nt = targets.shape[0] if isinstance(targets, torch.Tensor) else 0
    if out is None:
        out = MatchResult(torch.empty((B, max_det, NIOU), dtype=torch.bool, device=device),
                          torch.empty((B, max_det), dtype=torch.float32, device=device),
                          torch.empty((B, max_det), dtype=torch.int32, device=device), counts,
                          torch.empty((max(nt, 1),), dtype=torch.int32, device=device)[:nt],
                          torch.empty((B,), dtype=torch.int32, device=device))
    else:
        out.counts = counts
    tp_bits = torch.empty((B, max_det), dtype=torch.int16, device=device)
    _match(dets, counts, targets, img_hw, shapes, single_cls, tp_bits, out.conf, out.pred_cls, out.correct.view(torch.uint8), None, 0,
           out.tcls if nt else None, out.nl)
    return out


def _ap_device(tp_bits, conf, pcls, n, niou, hist, nc, device):
    """cft_eval_ap on device buffers -> device float64 [nc * (4 + niou)] = p | r | f1 | ntp | ap[nc, niou]."""
    lib = _lib.load()
    px, xg = _grids(device)
    ws = torch.empty((lib.cft_eval_ap_workspace_bytes(n, nc),), dtype=torch.uint8, device=device)
    out = torch.empty((nc * (4 + niou),), dtype=torch.float64, device=device)
    ptr = lambda t: t.data_ptr() if n else None  # noqa: E731
    st = lib.cft_eval_ap(ptr(tp_bits), ptr(conf), ptr(pcls), n, niou, hist.data_ptr(), nc, px.data_ptr(), xg.data_ptr(), ws.data_ptr(),
                         ws.numel(), out.data_ptr(), _stream())
    _lib.check(st, "cft_eval_ap")
    return out


def _split(out, nc, niou):
    return out[:nc], out[nc:2 * nc], out[2 * nc:3 * nc], out[3 * nc:4 * nc], out[4 * nc:].reshape(nc, niou)


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, save_dir='.', names=()):
    """The reference's ap_per_class (utils/metrics.py:18-79) on the GPU: returns numpy (p, r, ap, f1, ap_class).

    tp [n, niou] bool, conf [n], pred_cls [n], target_cls [nl] (numpy arrays or tensors).  Classes must be non-negative integers.
    Ties in conf keep their input order (numpy's argsort leaves them unspecified); conf is taken in float32 as test.py hands it."""
    if plot:
        raise NotImplementedError("ap_per_class: plotting (PR / F1 / P / R curves) is out of scope of this package")
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
    tp, conf, pred_cls, target_cls = as_np(tp), as_np(conf), as_np(pred_cls), as_np(target_cls)
    if tp.ndim != 2 or not 1 <= tp.shape[1] <= 16:
        raise ValueError(f"ap_per_class: tp must be [n, niou] with 1 <= niou <= 16, got {tp.shape}")
    n, niou = tp.shape
    if conf.shape != (n,) or pred_cls.shape != (n,):
        raise ValueError(f"ap_per_class: conf and pred_cls must be [{n}], got {conf.shape} and {pred_cls.shape}")
    tc = target_cls.astype(np.float64).reshape(-1)
    if tc.size and (not np.all(tc >= 0) or not np.all(tc == np.floor(tc)) or tc.max() > 65534):
        raise ValueError("ap_per_class: target classes must be integers in [0, 65534]")
    if not torch.cuda.is_available():
        raise RuntimeError("ap_per_class: needs a GPU (this package has no CPU path; oracle/ and the tests hold CPU restatements)")
    if tc.size == 0:
        return np.zeros(0), np.zeros(0), np.zeros((0, niou)), np.zeros(0), np.zeros(0, np.int32)
    nc = int(tc.max()) + 1
    hist = np.bincount(tc.astype(np.int64), minlength=nc).astype(np.int32)
    pc = pred_cls.astype(np.float64)
    ok = (pc >= 0) & (pc < nc) & (pc == np.floor(pc))
    pci = np.where(ok, pc, -1).astype(np.int32)
    bits = (tp.astype(bool) * (1 << np.arange(niou))).sum(1).astype(np.uint16).view(np.int16) if n else np.zeros(0, np.int16)
    device = torch.device("cuda", torch.cuda.current_device())
    d = lambda a: _to_device(torch.from_numpy(np.ascontiguousarray(a)), device)  # noqa: E731
    out = _ap_device(d(bits), d(conf.astype(np.float32)), d(pci), n, niou, d(hist), nc, device).cpu().numpy()
    p, r, f1, _, ap = _split(out, nc, niou)
    ap_class = np.flatnonzero(hist > 0)
    return p[ap_class], r[ap_class], ap[ap_class], f1[ap_class], ap_class.astype(np.int32)


FPPI_REF = np.logspace(-2.0, 0.0, 9)         # the nine reference points of the log-average miss rate (Dollar et al.)
FPPI_PLOT = np.logspace(-3, 1, 1000)         # default grid of the MR-FPPI plot
MAX_FPPI_GRID = 4096                         # cft_eval_curves: values of the one grid handed to the device


@dataclass
class EvalCurves:
    """The curves of a validation run, one row per class of ``ap_class`` (float64 numpy arrays).  ``py`` rows of a class with labels
    and no predictions are zero (the reference's ``ap_per_class`` appends no row for such a class)."""
    px: np.ndarray             # [1000] np.linspace(0, 1, 1000): confidence for p / r / f1, recall for py
    py: np.ndarray             # [k, 1000] precision over recall at IoU 0.5 (PR_curve)
    p: np.ndarray              # [k, 1000] precision over confidence (P_curve)
    r: np.ndarray              # [k, 1000] recall over confidence (R_curve)
    f1: np.ndarray             # [k, 1000] F1 over confidence (F1_curve)
    best: int                  # f1.mean(0).argmax(): the px index at which ap_per_class reads p, r and f1
    ap_class: np.ndarray       # [k] int32 classes with labels
    fppi: np.ndarray           # [m] the plotting grid of false positives per image
    mr_curve: np.ndarray       # [k, m] miss rate at fppi
    mr_ref: np.ndarray         # [k, 9] miss rate at np.logspace(-2, 0, 9)
    lamr: np.ndarray           # [k] log-average miss rate of each class
    mlamr: float               # its mean over ap_class (0.0 without classes)


def log_average_miss_rate(mr_ref):
    """exp(mean(log(max(1e-10, mr)))) over the last axis: the geometric mean of the miss rate at the nine reference FPPI values."""
    mr_ref = np.ascontiguousarray(mr_ref, dtype=np.float64)      # one summation order whatever layout the caller's array has
    return np.exp(np.mean(np.log(np.maximum(1e-10, mr_ref)), axis=-1))


def _fppi_grids(fppi_grid):
    """(plotting grid, merged grid for the device, positions of the nine reference points, positions of the plotting grid)."""
    plot = FPPI_PLOT if fppi_grid is None else np.asarray(fppi_grid, np.float64)
    if plot.ndim != 1 or not 1 <= plot.size <= MAX_FPPI_GRID - FPPI_REF.size:
        raise ValueError(f"curves: fppi_grid must be one-dimensional with 1 to {MAX_FPPI_GRID - FPPI_REF.size} values")
    if not np.all(np.isfinite(plot)) or np.any(np.diff(plot) < 0):
        raise ValueError("curves: fppi_grid must be finite and non-decreasing")
    merged = np.sort(np.concatenate((FPPI_REF, plot)), kind="stable")
    return plot, merged, np.searchsorted(merged, FPPI_REF), np.searchsorted(merged, plot)


def _curves_device(tp_bits, conf, pcls, n, hist, nc, n_images, grid, device):
    """cft_eval_curves on device buffers with the FPPI grid ``grid`` (host float64) -> one device float64 buffer
    p | r | f1 | py (each nc * 1000) | mr (nc * len(grid)) | best (an int32 in the last slot).  No synchronisation."""
    lib = _lib.load()
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    ng = int(grid.size)
    px, _ = _grids(device)
    nbytes = ctypes.c_long(0)
    _lib.check(lib.cft_eval_curves_workspace_bytes(n, nc, ctypes.byref(nbytes)), "cft_eval_curves_workspace_bytes")
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=device)
    k = nc * len(PX)
    out = torch.empty((4 * k + nc * ng + 1,), dtype=torch.float64, device=device)
    grid_dev = _to_device(torch.from_numpy(grid), device)
    ptr = lambda t: t.data_ptr() if n else None  # noqa: E731
    o = lambda i: out.data_ptr() + 8 * i  # noqa: E731
    st = lib.cft_eval_curves(ptr(tp_bits), ptr(conf), ptr(pcls), n, hist.data_ptr(), nc, int(n_images), px.data_ptr(), grid_dev.data_ptr(),
                             grid.ctypes.data, ng, ws.data_ptr(), ws.numel(), o(0), o(k), o(2 * k), o(3 * k), o(4 * k), o(4 * k + nc * ng),
                             _stream())
    _lib.check(st, "cft_eval_curves")
    return out


def _empty_curves(plot):
    z = np.zeros((0, len(PX)))
    return EvalCurves(PX.copy(), z, z.copy(), z.copy(), z.copy(), 0, np.zeros(0, np.int32), plot, np.zeros((0, plot.size)),
                      np.zeros((0, FPPI_REF.size)), np.zeros(0), 0.0)


def _curves_result(out, hist, nc, plot, merged, ref_at, plot_at):
    """The host buffer of _curves_device -> EvalCurves over the classes with labels."""
    k, ng = nc * len(PX), merged.size
    ap_class = np.flatnonzero(hist[:nc] > 0)
    if ap_class.size == 0:
        return _empty_curves(plot)
    p, r, f1, py = (out[i * k:(i + 1) * k].reshape(nc, len(PX))[ap_class] for i in range(4))
    mr = out[4 * k:4 * k + nc * ng].reshape(nc, ng)[ap_class]
    best = int(out[4 * k + nc * ng:].view(np.int32)[0])
    # (C order: numpy sums a row of a column-gathered array in another order than a row of a contiguous one, a last-bit difference)
    mr_ref, mr_curve = np.ascontiguousarray(mr[:, ref_at]), np.ascontiguousarray(mr[:, plot_at])
    lamr = log_average_miss_rate(mr_ref)
    return EvalCurves(PX.copy(), py, p, r, f1, best, ap_class.astype(np.int32), plot, mr_curve, mr_ref, lamr, float(lamr.mean()))


def curves_per_class(tp, conf, pred_cls, target_cls, n_images, fppi_grid=None):
    """The curves behind ``ap_per_class`` on the GPU (``cft_eval_curves``), from the same arrays: what the reference's
    ``ap_per_class(plot=True)`` hands to its plot functions (py, p, r, f1 at the 1000 px points, utils/metrics.py:57-75), the px index it
    reads its results at, and the miss rate over false positives per image with the log-average miss rate (``EvalCurves``).

    ``n_images``: the images the statistics come from (``seen`` of test.py).  ``fppi_grid``: the plotting grid of the MR curve
    (default ``np.logspace(-3, 1, 1000)``), non-decreasing.  The device walks ONE grid, the sorted merge of it and the nine reference
    points ``np.logspace(-2, 0, 9)``; ``lamr`` is taken on the host.  The miss-rate definition is this package's (include/cft_hip.h):
    the reference publishes LLVIP miss rates but ships no code for them."""
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
    tp, conf, pred_cls, target_cls = as_np(tp), as_np(conf), as_np(pred_cls), as_np(target_cls)
    if tp.ndim != 2 or not 1 <= tp.shape[1] <= 16:
        raise ValueError(f"curves_per_class: tp must be [n, niou] with 1 <= niou <= 16, got {tp.shape}")
    n = tp.shape[0]
    if conf.shape != (n,) or pred_cls.shape != (n,):
        raise ValueError(f"curves_per_class: conf and pred_cls must be [{n}], got {conf.shape} and {pred_cls.shape}")
    tc = target_cls.astype(np.float64).reshape(-1)
    if tc.size and (not np.all(tc >= 0) or not np.all(tc == np.floor(tc)) or tc.max() > 65534):
        raise ValueError("curves_per_class: target classes must be integers in [0, 65534]")
    if isinstance(n_images, bool) or int(n_images) != n_images or int(n_images) < 1:
        raise ValueError(f"curves_per_class: n_images must be a positive integer, got {n_images}")
    plot, merged, ref_at, plot_at = _fppi_grids(fppi_grid)
    if not torch.cuda.is_available():
        raise RuntimeError("curves_per_class: needs a GPU (this package has no CPU path; oracle/ and the tests hold CPU restatements)")
    if tc.size == 0:
        return _empty_curves(plot)
    nc = int(tc.max()) + 1
    hist = np.bincount(tc.astype(np.int64), minlength=nc).astype(np.int32)
    pc = pred_cls.astype(np.float64)
    ok = (pc >= 0) & (pc < nc) & (pc == np.floor(pc))
    pci = np.where(ok, pc, -1).astype(np.int32)
    bits = tp[:, 0].astype(bool).astype(np.uint16).view(np.int16) if n else np.zeros(0, np.int16)
    device = torch.device("cuda", torch.cuda.current_device())
    d = lambda a: _to_device(torch.from_numpy(np.ascontiguousarray(a)), device)  # noqa: E731
    out = _curves_device(d(bits), d(conf.astype(np.float32)), d(pci), n, d(hist), nc, int(n_images), merged, device).cpu().numpy()
    return _curves_result(out, hist, nc, plot, merged, ref_at, plot_at)


def _class_name(names, c):
    """The display name of class c: names may be a list or a dict, as in the reference; without one, the class number."""
    try:
        return str(names[int(c)])
    except (KeyError, IndexError, TypeError):
        return str(int(c))


def _curve_figure(x, rows, classes, labels, mean, mean_label, xlabel, ylabel, logx=False):
    """One line per class (named in the legend when there are fewer than 21, else thin grey) and a bold blue line for ``mean``."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(1, 1, figsize=(9, 6), tight_layout=True)
    few = 0 < len(classes) < 21
    for i in range(len(classes)):
        if few:
            ax.plot(x, rows[i], linewidth=1, label=labels[i])
        else:
            ax.plot(x, rows[i], linewidth=1, color='grey')
    if mean is not None:
        ax.plot(x, mean, linewidth=3, color='blue', label=mean_label)
    ax.set_xlabel(xlabel)
    ax.set_ylabel(ylabel)
    if logx:
        ax.set_xscale('log')
        ax.set_yscale('log')
        ax.set_xlim(float(x[0]) if x[0] > 0 else 1e-3, float(x[-1]))
        ax.set_ylim(1e-2, 1.0)
        ax.grid(True, which='both', linewidth=0.3)
    else:
        ax.set_xlim(0, 1)
        ax.set_ylim(0, 1)
    return fig, ax, plt


def plot_pr_curve(curves, ap, save_dir='.', names=()):
    """``save_dir/PR_curve.png``: precision over recall at IoU 0.5 for every class of ``curves`` (an ``EvalCurves``), each named with
    its AP@0.5, and their mean named with mAP@0.5.  ``ap``: ap_per_class's [k, niou] array (or its column 0).  Silent on failure."""
    try:
        ap = np.asarray(ap, np.float64)
        ap50 = ap[:, 0] if ap.ndim == 2 else ap
        labels = [f"{_class_name(names, c)} {a:.3f}" for c, a in zip(curves.ap_class, ap50)]
        mean = curves.py.mean(0) if len(curves.ap_class) else None
        fig, ax, plt = _curve_figure(curves.px, curves.py, curves.ap_class, labels, mean,
                                     f"all classes {ap50.mean():.3f} mAP@0.5" if len(ap50) else None, 'Recall', 'Precision')
        ax.legend(bbox_to_anchor=(1.04, 1), loc="upper left")
        fig.savefig(Path(save_dir) / 'PR_curve.png', dpi=250)
        plt.close(fig)
    except Exception:
        pass


_MC_CURVES = {"f1": ("F1_curve.png", "F1"), "p": ("P_curve.png", "Precision"), "r": ("R_curve.png", "Recall")}


def plot_mc_curve(curves, which, save_dir='.', names=()):
    """``save_dir/F1_curve.png``, ``P_curve.png`` or ``R_curve.png`` (``which`` = 'f1', 'p' or 'r'): the metric over confidence for
    every class and their mean, whose legend entry names its maximum and the confidence there.  Silent on failure (an unknown
    ``which`` is an error)."""
    if which not in _MC_CURVES:
        raise ValueError(f"plot_mc_curve: which must be one of {sorted(_MC_CURVES)}, got {which!r}")
    fname, ylabel = _MC_CURVES[which]
    try:
        rows = getattr(curves, which)
        labels = [_class_name(names, c) for c in curves.ap_class]
        mean = rows.mean(0) if len(curves.ap_class) else None
        label = f"all classes {mean.max():.2f} at {curves.px[mean.argmax()]:.3f}" if mean is not None else None
        fig, ax, plt = _curve_figure(curves.px, rows, curves.ap_class, labels, mean, label, 'Confidence', ylabel)
        ax.legend(bbox_to_anchor=(1.04, 1), loc="upper left")
        fig.savefig(Path(save_dir) / fname, dpi=250)
        plt.close(fig)
    except Exception:
        pass


def plot_mr_curve(curves, save_dir='.', names=()):
    """``save_dir/MR_curve.png``: miss rate over false positives per image on log-log axes for every class, the nine reference
    points marked, the log-average miss rate of each class (and the mean) in the legend.  Silent on failure."""
    try:
        labels = [f"{_class_name(names, c)} {100 * v:.2f}%" for c, v in zip(curves.ap_class, curves.lamr)]
        fig, ax, plt = _curve_figure(curves.fppi, curves.mr_curve, curves.ap_class, labels, None, None, 'False positives per image',
                                     'Miss rate', logx=True)
        for i in range(len(curves.ap_class)):
            ax.plot(FPPI_REF, curves.mr_ref[i], linestyle='none', marker='o', markersize=4, color='black')
        ax.plot([], [], linestyle='none', marker='o', markersize=4, color='black', label=f"mean MR^-2 {100 * curves.mlamr:.2f}%")
        ax.legend(bbox_to_anchor=(1.04, 1), loc="upper left")
        fig.savefig(Path(save_dir) / 'MR_curve.png', dpi=250)
        plt.close(fig)
    except Exception:
        pass


def _geom_device(shapes, img_hw, B, device, what):
    if len(shapes) != B:
        raise ValueError(f"{what}: {len(shapes)} shapes for a batch of {B} images")
    if int(img_hw[0]) <= 0 or int(img_hw[1]) <= 0:
        raise ValueError(f"{what}: bad image size {img_hw}")
    return _to_device(geometry(shapes, img_hw), device)


class ConfusionMatrix:
    """The reference's ConfusionMatrix (utils/metrics.py:111-183) on the GPU: ``matrix[predicted class, true class]`` with row and
    column ``nc`` for the background, as ``process_batch`` fills it (the rules and the tie rule are in the module docstring).
    Counts accumulate in an int64 matrix on the device; neither ``process_batch`` nor ``update`` synchronises with the host."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        if int(nc) < 1 or int(nc) > 32767:
            raise ValueError(f"ConfusionMatrix: nc must be in [1, 32767], got {nc}")
        self.nc = int(nc)  # number of classes
        self.conf = conf
        self.iou_thres = iou_thres
        self._m = self._flag = None

    def reset(self):
        """Zero the counts and the bad-class flag (in place on the device, no synchronisation)."""
        if self._m is not None:
            self._m.zero_()
            self._flag.zero_()

    def _launch(self, dets, counts, targets, H, W, geom, single_cls, native):
        device = dets.device
        if self._m is None:
            self._m = torch.zeros((self.nc + 1, self.nc + 1), dtype=torch.int64, device=device)
            self._flag = torch.zeros((1,), dtype=torch.int32, device=device)
        elif device != self._m.device:
            raise ValueError(f"ConfusionMatrix: batch on {device}, earlier batches on {self._m.device}")
        B, max_det, nt = dets.shape[0], dets.shape[1], targets.shape[0]
        lib = _lib.load()
        nbytes = ctypes.c_long(0)
        _lib.check(lib.cft_eval_confusion_workspace_bytes(B, nt, max_det, ctypes.byref(nbytes)), "cft_eval_confusion_workspace_bytes")
        ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=device)
        st = lib.cft_eval_confusion(dets.data_ptr(), counts.data_ptr(), B, max_det, targets.data_ptr() if nt else None, nt, H, W,
                                    geom.data_ptr() if geom is not None else None, float(self.conf), float(self.iou_thres),
                                    int(bool(single_cls)), int(native), self.nc, ws.data_ptr(), ws.numel(), self._m.data_ptr(),
                                    self._flag.data_ptr(), _stream())
        _lib.check(st, "cft_eval_confusion")

    def process_batch(self, detections, labels):
        """One image, as the reference: detections [N, 6] = x1, y1, x2, y2, conf, class and labels [M, 5] = class, x1, y1, x2, y2,
        both in native image space, tensors on the GPU.  Updates the matrix."""
        _require_cuda(detections, "ConfusionMatrix.process_batch")
        _require_cuda(labels, "ConfusionMatrix.process_batch")
        if detections.dim() != 2 or detections.shape[1] != 6 or labels.dim() != 2 or labels.shape[1] != 5:
            raise ValueError(f"ConfusionMatrix.process_batch: detections [N, 6] and labels [M, 5], got {tuple(detections.shape)} and "
                             f"{tuple(labels.shape)}")
        N, M = detections.shape[0], labels.shape[0]
        if N == 0 and M == 0:
            return
        device = detections.device
        dets = torch.zeros((1, max(N, 1), 6), dtype=torch.float32, device=device)
        dets[0, :N].copy_(detections)
        targets = torch.zeros((M, 6), dtype=torch.float32, device=device)          # image 0 | class | xyxy
        targets[:, 1:].copy_(labels)
        if N == 0:
            # the reference's process_batch counts every label as background when it is handed no detection (test.py never does):
            # a slot below the conf filter stands in, so that the image is not taken for one without NMS detections
            dets[0, 0, 4] = float("-inf")
        counts = _to_device(torch.tensor([max(N, 1)], dtype=torch.int32), device)
        self._launch(dets, counts, targets, 0, 0, None, False, 1)

    def update(self, dets, counts, targets, img_hw, shapes, single_cls=False):
        """One batch, as test.py:193-194 feeds process_batch image by image: (dets, counts) from batched_nms (or
        non_max_suppression's list with counts=None); targets [nt, 6], img_hw and shapes as for match_batch."""
        device = dets[0].device if isinstance(dets, (list, tuple)) and len(dets) else getattr(dets, "device", None)
        if device is None or device.type != "cuda":
            raise RuntimeError("ConfusionMatrix.update: detections must be on the GPU (this package has no CPU path)")
        dets, counts = _pack_dets(dets, counts, device)
        if not isinstance(targets, torch.Tensor) or targets.dim() != 2 or targets.shape[1] != 6:
            raise ValueError(f"ConfusionMatrix.update: targets must be an [nt, 6] tensor, got {getattr(targets, 'shape', type(targets))}")
        geom = _geom_device(shapes, img_hw, dets.shape[0], device, "ConfusionMatrix.update")
        targets = _to_device(targets.float(), device).contiguous()
        self._launch(dets, counts, targets, int(img_hw[0]), int(img_hw[1]), geom, single_cls, 0)

    @property
    def matrix(self):
        """(nc + 1, nc + 1) float64 numpy array, as the reference's attribute.  Synchronises once."""
        if self._m is None:
            return np.zeros((self.nc + 1, self.nc + 1))
        both = torch.cat((self._m.reshape(-1), self._flag.to(torch.int64))).cpu().numpy()
        if both[-1]:
            what = " and ".join(w for bit, w in ((1, "labels"), (2, "detections")) if both[-1] & bit)
            raise ValueError(f"ConfusionMatrix: {what} with a class outside [0, {self.nc}) were skipped")
        return both[:-1].reshape(self.nc + 1, self.nc + 1).astype(np.float64)

    def plot(self, save_dir='', names=()):
        """The reference's normalised heat map (utils/metrics.py:162-179) with matplotlib alone (it uses seaborn); like there, any
        failure (matplotlib missing, unwritable directory) is silent."""
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            m = self.matrix
            array = m / (m.sum(0).reshape(1, self.nc + 1) + 1E-6)  # normalize
            array[array < 0.005] = np.nan  # don't annotate (would appear as 0.00)
            fig, ax = plt.subplots(figsize=(12, 9), tight_layout=True)
            im = ax.imshow(array, cmap='Blues')
            fig.colorbar(im, ax=ax)
            if self.nc < 30:
                for i in range(self.nc + 1):
                    for j in range(self.nc + 1):
                        if not np.isnan(array[i, j]):
                            ax.text(j, i, f"{array[i, j]:.2f}", ha="center", va="center", fontsize=8)
            names = list(names)
            if 0 < len(names) < 99 and len(names) == self.nc:  # apply names to ticklabels
                ax.set_xticks(range(self.nc + 1))
                ax.set_xticklabels(names + ['background FP'], rotation=90)
                ax.set_yticks(range(self.nc + 1))
                ax.set_yticklabels(names + ['background FN'])
            ax.set_xlabel('True')
            ax.set_ylabel('Predicted')
            fig.savefig(Path(save_dir) / 'confusion_matrix.png', dpi=250)
            plt.close(fig)
        except Exception:
            pass

    def print(self):
        m = self.matrix
        for i in range(self.nc + 1):
            print(' '.join(map(str, m[i])))


EXPORT_FLOATS = 16      # per slot: xyxy | conf cls valid 0 | save_txt xywh | save_json xywh (include/cft_hip.h, cft_eval_export)


def export_batch(dets, counts, img_hw, shapes, single_cls=False):
    """float32 [B, max_det, 16] on the device, per detection slot of the batched_nms output: native-space xyxy | conf, class,
    valid (1 / 0), 0 | the normalised xywh of save_txt (test.py:153-155) | the top-left xywh of save_json (:176-177)."""
    device = getattr(dets, "device", None)
    if device is None or device.type != "cuda":
        raise RuntimeError("export_batch: detections must be on the GPU (this package has no CPU path)")
    dets, counts = _pack_dets(dets, counts, device)
    B, max_det = dets.shape[0], dets.shape[1]
    geom = _geom_device(shapes, img_hw, B, device, "export_batch")
    out = torch.empty((B, max_det, EXPORT_FLOATS), dtype=torch.float32, device=device)
    st = _lib.load().cft_eval_export(dets.data_ptr(), counts.data_ptr(), B, max_det, geom.data_ptr(), int(bool(single_cls)),
                                     out.data_ptr(), _stream())
    _lib.check(st, "cft_eval_export")
    return out


def txt_line(cls, xywh, conf=None):
    """One line of a save_txt label file (test.py:156-158): class, normalised xywh and, with save_conf, the confidence."""
    line = (cls, *xywh, conf) if conf is not None else (cls, *xywh)
    return ('%g ' * len(line)).rstrip() % line + '\n'


def json_entry(stem, cls, box, score):
    """One entry of the save_json list (test.py:175-182): box = top-left xywh in native pixels."""
    return {'image_id': int(stem) if stem.isnumeric() else stem, 'category_id': int(cls), 'bbox': [round(x, 3) for x in box],
            'score': round(score, 5)}


def export_rows(export, paths):
    """Host side of save_txt / save_json: the export buffer of one batch (one device-to-host copy) -> per image
    (stem, rows [n, 16] as Python floats), skipping images without detections (test.py:140-143)."""
    rows = export.cpu()
    B = rows.shape[0]
    if paths is None or len(paths) != B:
        raise ValueError(f"save_txt / save_json need the image paths of the batch ({B} images)")
    out = []
    for b in range(B):
        n = int(rows[b, :, 6].sum())
        if n:
            out.append((Path(paths[b]).stem, rows[b, :n].tolist()))
    return out


@dataclass
class EvalResult:
    """test.py's metrics (:227-236, :292-294).  p, r, ap, f1, ap_class as ap_per_class returns them; nt = labels per class."""
    mp: float
    mr: float
    map50: float
    map75: float
    map: float
    maps: np.ndarray
    p: np.ndarray
    r: np.ndarray
    ap: np.ndarray
    f1: np.ndarray
    ap_class: np.ndarray
    nt: object
    seen: int
    confusion_matrix: object = None     # (nc + 1, nc + 1) float64 numpy array with DetectionEvaluator(confusion=True), else None

    def as_test_tuple(self):
        """test.py's ``((mp, mr, map50, map75, map), maps)`` (without the validation losses)."""
        return (self.mp, self.mr, self.map50, self.map75, self.map), self.maps


class DetectionEvaluator:
    """Accumulates test.py's statistics on the GPU.  ``update()`` never synchronises with the host: every batch appends its
    B * max_det slots (empty ones are dropped later), so buffer offsets are known on the host.  ``compute()`` synchronises once
    (once more for the confusion matrix).  ``confusion=True`` also feeds every batch to a ``ConfusionMatrix`` (one more launch pair, still no synchronisation);
    ``EvalResult.confusion_matrix`` then holds its matrix."""

    def __init__(self, nc, single_cls=False, confusion=False):
        if int(nc) < 1 or int(nc) > 65535:
            raise ValueError(f"DetectionEvaluator: nc must be in [1, 65535], got {nc}")
        self.nc = int(nc)
        self.single_cls = bool(single_cls)
        self.confusion = bool(confusion)
        self.device = None
        self.reset()

    def reset(self):
        self.n = 0
        self.seen = 0
        self._tp = self._conf = self._pcls = self._hist = None
        if not self.confusion:
            self.confusion_matrix = None
        elif getattr(self, "confusion_matrix", None) is None:
            self.confusion_matrix = ConfusionMatrix(self.nc)                               # test.py:97
        else:
            self.confusion_matrix.reset()

    def _reserve(self, device, need):
        if self.device is None or self._hist is None:
            self.device = device
            self._hist = torch.zeros((self.nc + 1,), dtype=torch.int32, device=device)
        elif device != self.device:
            raise ValueError(f"DetectionEvaluator: batch on {device}, earlier batches on {self.device}")
        cap = 0 if self._tp is None else self._tp.numel()
        if need <= cap:
            return
        cap = max(need, 2 * cap, 1 << 14)
        tp = torch.empty((cap,), dtype=torch.int16, device=device)
        conf = torch.empty((cap,), dtype=torch.float32, device=device)
        pcls = torch.empty((cap,), dtype=torch.int32, device=device)
        if self.n:
            tp[:self.n].copy_(self._tp[:self.n])
            conf[:self.n].copy_(self._conf[:self.n])
            pcls[:self.n].copy_(self._pcls[:self.n])
        self._tp, self._conf, self._pcls = tp, conf, pcls

    def update(self, dets, counts, targets, img_hw, shapes):
        """Add one batch: (dets, counts) from batched_nms, or non_max_suppression's list with counts=None; targets, img_hw and
        shapes as for match_batch."""
        device = dets[0].device if isinstance(dets, (list, tuple)) and len(dets) else getattr(dets, "device", None)
        if device is None or device.type != "cuda":
            raise RuntimeError("DetectionEvaluator.update: detections must be on the GPU (this package has no CPU path)")
        dets, counts = _pack_dets(dets, counts, device)
        B, max_det = dets.shape[0], dets.shape[1]
        k = B * max_det
        self._reserve(device, self.n + k)
        sl = slice(self.n, self.n + k)
        _match(dets, counts, targets, img_hw, shapes, self.single_cls, self._tp[sl], self._conf[sl], self._pcls[sl], None,
               self._hist, self.nc, None, None)
        if self.confusion_matrix is not None:
            self.confusion_matrix.update(dets, counts, targets, img_hw, shapes, self.single_cls)
        self.n += k
        self.seen += B

    def compute(self):
        nc, niou = self.nc, NIOU
        maps0 = np.zeros(nc)
        empty = EvalResult(0., 0., 0., 0., 0., maps0, 0., 0., [], 0., [], torch.zeros(1), self.seen)
        cm = empty.confusion_matrix = self.confusion_matrix.matrix if self.confusion_matrix is not None else None
        if self._hist is None:
            return empty
        out = _ap_device(self._tp, self._conf, self._pcls, self.n, niou, self._hist, nc, self.device)
        out, hist = out.cpu().numpy(), self._hist.cpu().numpy()       # the one synchronisation
        if hist[nc]:
            raise ValueError(f"DetectionEvaluator: {int(hist[nc])} labels have a class outside [0, {nc})")
        p, r, f1, ntp, ap = _split(out, nc, niou)
        if not ntp.sum() > 0:                     # test.py:227: no TP at any threshold -> all zero (a TP is always a TP at iouv[0])
            return empty
        ap_class = np.flatnonzero(hist[:nc] > 0)
        p, r, f1, ap = p[ap_class], r[ap_class], f1[ap_class], ap[ap_class]
        # test.py:229-232
        ap50, ap75, apm = ap[:, 0], ap[:, 5], ap.mean(1)
        mp, mr, map50, map75, map_ = p.mean(), r.mean(), ap50.mean(), ap75.mean(), apm.mean()
        nt = hist[:nc].astype(np.int64)
        maps = np.zeros(nc) + map_              # test.py:291-293
        for i, c in enumerate(ap_class):
            maps[c] = apm[i]
        return EvalResult(float(mp), float(mr), float(map50), float(map75), float(map_), maps, p, r, ap, f1, ap_class.astype(np.int32),
                          nt, self.seen, cm)

    def curves(self, fppi_grid=None):
        """The curves of the accumulated statistics (``EvalCurves``, see ``curves_per_class``) with ``seen`` as the image count: two
        launches after the sort of ``compute()``, which it repeats on a workspace of its own, and one synchronisation.  ``compute()`` is
        not needed before it and is not changed by it.  Before any ``update()`` it returns empty arrays."""
        plot, merged, ref_at, plot_at = _fppi_grids(fppi_grid)
        if self._hist is None:
            return _empty_curves(plot)
        nc = self.nc
        out = _curves_device(self._tp, self._conf, self._pcls, self.n, self._hist, nc, max(self.seen, 1), merged, self.device)
        both = torch.cat((out.view(torch.int32), self._hist)).cpu().numpy()       # the one synchronisation
        hist = both[-(nc + 1):]
        if hist[nc]:
            raise ValueError(f"DetectionEvaluator: {int(hist[nc])} labels have a class outside [0, {nc})")
        return _curves_result(both[:-(nc + 1)].view(np.float64), hist, nc, plot, merged, ref_at, plot_at)
