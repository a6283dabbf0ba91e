"""Time kmean_anchors(n=9, gen=1000) on synthetic log-normal labels against a torch-op GPU version written from the algorithm.

    python tools/anchor_bench.py [--sizes 2400 22000 200000] [--gen 1000] [--reps 3]

Per size one JSON line: the whole call, its k-means and evolution legs (each ends with its one device-to-host read), the kernel
launches per call (gen + 1 evolution launches, one k-means launch, three print_results metric launches) and the same work in
eager torch ops on the same GPU tensors: Lloyd iterations with a host read of the mean distance per iteration, and one host
decision per generation.  Medians of --reps calls after one warm-up call; no time here is a pass criterion.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msod_amd  # noqa: E402,F401
from msod_amd.utils import autoanchor as aa  # noqa: E402


def labels(n, seed=0):
    g = np.random.default_rng(seed)
    per = 8
    imgs = max(1, n // per)
    shapes = np.stack([g.choice([640, 512, 1280], imgs), g.choice([512, 480, 1024], imgs)], 1).astype(np.float64)
    out = []
    for _ in range(imgs):
        l = np.zeros((per, 5))
        l[:, 3:5] = np.exp(g.normal(np.log(0.05), 0.9, (per, 2))).clip(0.004, 0.95)
        out.append(l)
    return shapes, out


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def torch_kmeans(obs, k, idx):
    best, best_d = None, float("inf")
    for rows in idx:
        book, prev = obs[rows], float("inf")
        while True:
            d = book[None] - obs[:, None]
            ds = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
            low, code = ds.min(1)
            avg = float(low.sqrt().mean())                       # the host decides: one read per iteration
            cnt = torch.bincount(code, minlength=len(book))
            new = torch.zeros_like(book).index_add_(0, code, obs) / cnt[:, None]
            book = new[cnt > 0]
            diff, prev = abs(prev - avg), avg
            if not diff > 1e-5:
                break
        if avg < best_d:
            best, best_d = book, avg
    return best


def torch_evolve(wh, k, thr, v):
    def fit(kk):
        r = wh[:, None] / kk.float()[None]
        best = torch.min(r, 1. / r).min(2)[0].max(1)[0]
        return (best * (best > thr).float()).mean()
    f = fit(k)
    for g in range(len(v)):
        kg = (k * v[g]).clamp(min=2.0)
        fg = fit(kg)
        if fg > f:                                               # the host decides: one read per generation
            f, k = fg, kg
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2400, 22000, 200000])
    ap.add_argument("--gen", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for n in a.sizes:
        shapes, lab = labels(n)
        wh = np.concatenate([l[:, 3:5] * s for s, l in zip(640 * shapes / shapes.max(1, keepdims=True), lab)])
        wh = wh[(wh >= 2.0).any(1)]
        s = wh.std(0)
        np.random.seed(0)
        idx = np.stack([np.random.choice(len(wh), 9, replace=False) for _ in range(30)])
        v = aa.draw_mutations((9, 2), a.gen)
        whd = torch.tensor(wh, dtype=torch.float32, device=dev)
        obs = torch.tensor(wh / s, device=dev)
        k0 = aa.device_kmeans(wh / s, 9, idx, dev)[0] * s
        vd, idxd = torch.tensor(v, device=dev), torch.tensor(idx, device=dev)

        def whole():
            np.random.seed(0)
            with contextlib.redirect_stdout(io.StringIO()):
                aa.kmean_anchors((shapes, lab), n=9, img_size=640, thr=4.0, gen=a.gen, verbose=False)

        row = {"labels": len(wh), "gen": a.gen, "kmean_anchors_ms": round(timed(whole, a.reps), 2),
               "kmeans_ms": round(timed(lambda: aa.device_kmeans(wh / s, 9, idx, dev), a.reps), 2),
               "evolve_ms": round(timed(lambda: aa.device_evolve(whd, k0, 0.25, v), a.reps), 2),
               "kmeans_iterations": aa.device_kmeans(wh / s, 9, idx, dev)[2][2],
               "launches_per_call": {"kmeans": 1, "evolve": a.gen + 1, "metric": 3},
               "torch_ops_kmeans_ms": round(timed(lambda: torch_kmeans(obs, 9, idxd), a.reps), 2),
               "torch_ops_evolve_ms": round(timed(lambda: torch_evolve(whd, torch.tensor(k0, device=dev), 0.25, vd), a.reps), 2)}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
