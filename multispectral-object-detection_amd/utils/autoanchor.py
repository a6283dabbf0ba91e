"""The reference's ``utils/autoanchor.py`` on the GPU (``csrc/autoanchor.hip``): the pre-flight ``train.py:220-221`` runs unless
``--noautoanchor`` is given.

    check_anchors(dataset, model=model, thr=hyp['anchor_t'], imgsz=imgsz)      # before ComputeLoss(model) is built
    k = kmean_anchors(dataset, n=9, img_size=640, thr=4.0, gen=1000)           # dataset: .shapes / .labels, or (shapes, labels)

The host keeps what is random and what is O(n) once: numpy's global ``RandomState`` draws the augment scale, the k-means starting rows
and the mutations with the reference's own calls, so the state ends where the reference leaves it; the labels are scaled, filtered
and whitened in numpy.  The device does the rest: the ratio metric (``cft_anchor_metric``), scipy's ``kmeans(obs, n, iter=30)`` with its
convergence test (``cft_anchor_kmeans``) and the whole genetic loop with its accept decisions (``cft_anchor_evolve``).

Fitness is defined exactly: the reference's ``(best * (best > thr).float()).mean()`` depends on torch's float32 summation order, here it
is ``float32(S / (2^29 * n))`` with ``S`` the integer sum of ``best * 2^29`` over ``best > thr`` - the same on every device and in numpy.
It agrees with the reference's value to about one float32 ulp; a mutation whose gain is smaller than that may be decided differently.

Quirks kept: ``thr`` is compared as float32; ``print_results`` sorts by area; a k-means that loses a cluster prints the reference's
message and raises ``AssertionError``, which ``check_anchors`` turns into ``ERROR`` and the old anchors.  Quirk not kept: the reference's
``print_results`` and ``new_bpr`` divide by the float64 numpy anchors (torch promotes); here the anchors are rounded to float32 first, as in
``anchor_fitness``.  The progress bar is not drawn, and with ``verbose`` the per-improvement lines come after the evolution, in order.

After a replacement ``check_anchors`` calls ``invalidate_packed`` on the model, so the next forward decodes with the new anchors and no
captured graph replays the old ones.  ``ComputeLoss`` copies ``Detect.anchors`` when it is constructed: build it after ``check_anchors``,
which is ``train.py``'s order.
"""
import ctypes
from fractions import Fraction

import numpy as np
import torch

from .. import _lib
from ..models.common import invalidate_packed
from ..models.yolo_test import check_anchor_order as _check_anchor_order
from ..ops import _require_cuda, _stream

PREFIX = "\033[34m\033[1mautoanchor: \033[0m"      # colorstr('autoanchor: '): blue, bold
KMEANS_RESTARTS = 30                               # kmeans(wh / s, n, iter=30)


def check_anchor_order(m):
    """``models.yolo_test.check_anchor_order`` with the reference's message (utils/autoanchor.py:12-20)."""
    before = m.anchors.clone()
    _check_anchor_order(m)
    if not torch.equal(before, m.anchors):
        print("Reversing anchor order")


class AnchorMetric:
    """Counts and sums of the ratio metric over ``n`` labels and ``na`` anchors.  The sums are exact rationals."""

    def __init__(self, words, n, na):
        w = [int(x) for x in words]
        self.n, self.na = n, na
        self.n_best_above, self.n_x_above = w[0], w[1]
        self.sum_x = Fraction(w[2], 1 << 29) + Fraction(w[3], 1 << 61)
        self.sum_best = Fraction(w[4], 1 << 29) + Fraction(w[5], 1 << 61)
        self.sum_x_above = Fraction(w[6], 1 << 29)
        self.sum_best_above = Fraction(w[7], 1 << 29)
        self.fitness_sum = w[7]

    @property
    def bpr(self):          # (best > thr).float().mean()
        return np.float32(self.n_best_above) / np.float32(self.n)

    @property
    def aat(self):          # (x > thr).float().sum(1).mean()
        return np.float32(self.n_x_above) / np.float32(self.n)

    @property
    def fitness(self):      # the exact fitness of the module docstring
        return np.float32(np.float64(self.fitness_sum) / (float(1 << 29) * self.n))


def _device_of(t=None):
    if t is not None and t.is_cuda:
        return t.device
    return torch.device("cuda", torch.cuda.current_device())


def anchor_metric(wh, anchors, thr):
    """The metric of ``check_anchors`` / ``print_results`` for labels ``wh`` [n, 2] and ``anchors`` [na, 2] (anything ``torch.as_tensor``
    takes; rounded to float32), ``thr = 1 / anchor_t``.  One launch, one synchronisation (the read-back)."""
    wh = torch.as_tensor(wh)
    dev = _device_of(wh)
    wh = wh.to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
    k = torch.as_tensor(anchors).to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
    _require_cuda(wh, "anchor_metric")
    out = torch.empty(8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _lib.load().cft_anchor_metric(wh.data_ptr(), wh.shape[0], k.data_ptr(), k.shape[0], float(thr), out.data_ptr(), _stream())
    _lib.check(st, "cft_anchor_metric")
    return AnchorMetric(out.cpu().tolist(), wh.shape[0], k.shape[0])


def device_kmeans(obs, k, idx, device=None):
    """``scipy.cluster.vq.kmeans(obs, k, iter=len(idx))`` for float64 ``obs`` [n, 2], starting restart r from the rows ``idx[r]``.
    Returns ``(book [survivors, 2] float64, distortion, info)``; one synchronisation."""
    dev = device or _device_of()
    obs = torch.as_tensor(np.ascontiguousarray(obs, dtype=np.float64)).to(dev)
    idx = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
    n, iters = obs.shape[0], idx.shape[0]
    lib = _lib.load()
    nbytes = ctypes.c_long(0)
    _lib.check(lib.cft_anchor_kmeans_workspace_bytes(n, ctypes.byref(nbytes)), "cft_anchor_kmeans_workspace_bytes")
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    res = torch.zeros(2 * k + 1 + 2, dtype=torch.float64, device=dev)          # book | dist | 4 ints
    info = res[2 * k + 1:].view(torch.int32)
    with torch.cuda.device(dev):
        st = lib.cft_anchor_kmeans(obs.data_ptr(), n, int(k), idx.data_ptr(), iters, ws.data_ptr(), ws.numel(), res.data_ptr(),
                                   res[2 * k:].data_ptr(), info.data_ptr(), _stream())
    _lib.check(st, "cft_anchor_kmeans")
    host = res.cpu()
    info = host[2 * k + 1:].view(torch.int32).tolist()
    if info[3]:
        raise RuntimeError("cft_anchor_kmeans: a restart did not converge (non-finite labels?)")
    return host[:2 * k].view(k, 2)[:info[0]].numpy().copy(), float(host[2 * k]), info


def device_evolve(wh, k, thr, v):
    """The genetic loop from anchors ``k`` [na, 2] float64 with the mutations ``v`` [gen, na, 2] float64 on labels ``wh`` (float32, on
    the device).  Returns ``(k, f, flags [gen], fg [gen])``; gen + 1 launches, one synchronisation."""
    dev = wh.device
    na, gen = k.shape[0], v.shape[0]
    lib = _lib.load()
    nbytes = ctypes.c_long(0)
    _lib.check(lib.cft_anchor_evolve_workspace_bytes(gen, ctypes.byref(nbytes)), "cft_anchor_evolve_workspace_bytes")
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    kd = torch.as_tensor(np.ascontiguousarray(k, dtype=np.float64)).to(dev)
    vd = torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).to(dev) if gen else None
    # one read-back: k (2 na doubles) | f, fg[gen] float32 | flags[gen] int32
    res = torch.zeros(2 * na * 8 + 4 * (1 + gen) + 4 * gen, dtype=torch.uint8, device=dev)
    ko = res[:2 * na * 8].view(torch.float64)
    fo = res[2 * na * 8:2 * na * 8 + 4 * (1 + gen)].view(torch.float32)
    flo = res[2 * na * 8 + 4 * (1 + gen):].view(torch.int32)
    ko.copy_(kd.reshape(-1))
    with torch.cuda.device(dev):
        st = lib.cft_anchor_evolve(wh.data_ptr(), wh.shape[0], na, float(thr), vd.data_ptr() if gen else None, gen, ko.data_ptr(),
                                   fo.data_ptr(), flo.data_ptr() if gen else None, fo[1:].data_ptr() if gen else None, ws.data_ptr(),
                                   ws.numel(), _stream())
    _lib.check(st, "cft_anchor_evolve")
    host = res.cpu()
    f = host[2 * na * 8:2 * na * 8 + 4 * (1 + gen)].view(torch.float32).numpy().copy()
    return (host[:2 * na * 8].view(torch.float64).numpy().reshape(na, 2).copy(), f[0],
            host[2 * na * 8 + 4 * (1 + gen):].view(torch.int32).numpy().astype(bool), f[1:])


def draw_mutations(shape, gen, mp=0.9, s=0.1):
    """The ``gen`` mutation arrays of the genetic loop, drawn with the reference's calls (utils/autoanchor.py:190-192) including its
    redraw while nothing changed: they do not depend on the anchors, so they can all be drawn first."""
    npr = np.random
    out = np.empty((gen,) + tuple(shape))
    for g in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            v = ((npr.random(shape) < mp) * npr.random() * npr.randn(*shape) * s + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def _shapes_labels(path):
    if isinstance(path, str):
        raise NotImplementedError("kmean_anchors: this package has no LoadImagesAndLabels; pass a dataset object with .shapes and .labels "
                                  "or a (shapes, labels) pair instead of a *.yaml path")
    if isinstance(path, (tuple, list)) and len(path) == 2:
        return np.asarray(path[0]), path[1]
    return np.asarray(path.shapes), path.labels


def kmean_anchors(path, n=9, img_size=640, thr=4.0, gen=1000, verbose=True):
    """k-means anchors evolved by the genetic loop (reference utils/autoanchor.py:103-201).  Returns ``k`` [n, 2] float64, sorted by area.
    ``path``: a dataset object with ``.shapes`` and ``.labels`` - ``utils.datasets.LoadMultiModalImagesAndLabels(path_rgb, path_ir, ...)`` is
    the way to run it on a dataset on disk - or a ``(shapes, labels)`` pair; a ``*.yaml`` path raises."""
    thr = 1. / thr
    dataset_shapes, labels = _shapes_labels(path)
    dev = _device_of()

    def print_results(k):
        k = k[np.argsort(k.prod(1))]  # sort small to large
        m = anchor_metric(wh0_d, k, thr)
        aat = np.float32(m.n_x_above) / np.float32(m.n * n) * n
        print(f'{PREFIX}thr={thr:.2f}: {m.bpr:.4f} best possible recall, {aat:.2f} anchors past thr')
        past = float(m.sum_x_above / m.n_x_above) if m.n_x_above else float('nan')
        print(f'{PREFIX}n={n}, img_size={img_size}, metric_all={float(m.sum_x / (m.n * n)):.3f}/{float(m.sum_best / m.n):.3f}-mean/best, '
              f'past_thr={past:.3f}-mean: ', end='')
        for i, x in enumerate(k):
            print('%i,%i' % (round(x[0]), round(x[1])), end=',  ' if i < len(k) - 1 else '\n')  # use in *.cfg
        return k

    # Get label wh
    shapes = img_size * dataset_shapes / dataset_shapes.max(1, keepdims=True)
    wh0 = np.concatenate([l[:, 3:5] * s for s, l in zip(shapes, labels)])  # wh

    # Filter
    i = (wh0 < 3.0).any(1).sum()
    if i:
        print(f'{PREFIX}WARNING: Extremely small objects found. {i} of {len(wh0)} labels are < 3 pixels in size.')
    wh = wh0[(wh0 >= 2.0).any(1)]  # filter > 2 pixels

    # Kmeans calculation: the starting rows of every restart come from numpy's global state, as scipy draws them
    print(f'{PREFIX}Running kmeans for {n} anchors on {len(wh)} points...')
    s = wh.std(0)  # sigmas for whitening
    rng = np.random.mtrand._rand
    idx = np.stack([rng.choice(wh.shape[0], size=int(n), replace=False) for _ in range(KMEANS_RESTARTS)])
    k, dist, _ = device_kmeans(wh / s, n, idx, dev)
    assert len(k) == n, print(f'{PREFIX}ERROR: scipy.cluster.vq.kmeans requested {n} points but returned only {len(k)}')
    k *= s
    wh_d = torch.tensor(wh, dtype=torch.float32).to(dev)  # filtered
    wh0_d = torch.tensor(wh0, dtype=torch.float32).to(dev)  # unfiltered
    k = print_results(k)

    # Evolve
    v = draw_mutations(k.shape, gen)
    k0 = k
    k, f, flags, fg = device_evolve(wh_d, k, thr, v)
    if verbose:
        kk = k0
        for g in np.flatnonzero(flags):
            kk = (kk * v[g]).clip(min=2.0)
            print_results(kk)
    return print_results(k)


def _check(dataset, model, m, thr, imgsz, show_module):
    print(f'\n{PREFIX}Analyzing anchors... ', end='')
    if show_module:
        print(m)
    dshapes = np.asarray(dataset.shapes)
    shapes = imgsz * dshapes / dshapes.max(1, keepdims=True)
    scale = np.random.uniform(0.9, 1.1, size=(shapes.shape[0], 1))  # augment scale
    wh = torch.tensor(np.concatenate([l[:, 3:5] * s for s, l in zip(shapes * scale, dataset.labels)])).float()  # wh
    dev = _device_of(m.anchor_grid)
    wh = wh.to(dev)

    def metric(k):
        r = anchor_metric(wh, k, 1. / thr)
        return r.bpr, r.aat

    anchors = m.anchor_grid.clone().view(-1, 2)  # current anchors
    bpr, aat = metric(anchors)
    print(f'anchors/target = {aat:.2f}, Best Possible Recall (BPR) = {bpr:.4f}', end='')
    if bpr < 0.98:  # threshold to recompute
        print('. Attempting to improve anchors, please wait...')
        na = m.anchor_grid.numel() // 2  # number of anchors
        try:
            anchors = kmean_anchors(dataset, n=na, img_size=imgsz, thr=thr, gen=1000, verbose=False)
        except Exception as e:
            print(f'{PREFIX}ERROR: {e}')
        new_bpr = metric(anchors)[0]
        if new_bpr > bpr:  # replace anchors
            anchors = torch.tensor(anchors, device=m.anchors.device).type_as(m.anchors)
            with torch.no_grad():
                m.anchor_grid[:] = anchors.clone().view_as(m.anchor_grid)  # for inference
                m.anchors[:] = anchors.clone().view_as(m.anchors) / m.stride.to(m.anchors.device).view(-1, 1, 1)  # loss
                check_anchor_order(m)
            invalidate_packed(model)       # the decode kernel reads a packed copy of anchor_grid; captured graphs replay it
            print(f'{PREFIX}New anchors saved to model. Update model *.yaml to use these anchors in the future.')
        else:
            print(f'{PREFIX}Original anchors better than new anchors. Proceeding with original anchors.')
    print('')  # newline


def check_anchors(dataset, model, thr=4.0, imgsz=640):
    """Check the anchors' fit to the data and recompute them if BPR < 0.98 (reference utils/autoanchor.py:23-59)."""
    m = model.module.model[-1] if hasattr(model, 'module') else model.model[-1]  # Detect()
    _check(dataset, model, m, thr, imgsz, show_module=False)


def check_anchors_rgb_ir(dataset, model, thr=4.0, imgsz=640):
    """``check_anchors`` as the two-stream train.py calls it (reference utils/autoanchor.py:62-100): the head is the last child, and it
    is printed."""
    m = list(model.model.children())[-1]
    _check(dataset, model, m, thr, imgsz, show_module=True)
