"""numpy restatement of the autoanchor algorithms, written from their rules for the tests of csrc/autoanchor.hip and
utils/autoanchor.py: the ratio metric in float32, k-means as scipy.cluster.vq.kmeans runs it (float64), the genetic loop of
kmean_anchors with the exact integer fitness, and the random draws both need."""
from fractions import Fraction

import numpy as np

SHIFT = 29                    # a float32 in [2^-6, 1] is a multiple of 2^-29
KMEANS_THRESH = 1e-5          # scipy's default


def ratio_x(wh, k):
    """x [n, na] float32 = min over the two dims of min(r, 1 / r), r = wh / k, every operation one float32 rounding."""
    wh, k = np.asarray(wh, np.float32), np.asarray(k, np.float32)
    r = wh[:, None, :] / k[None, :, :]
    return np.minimum(r, np.float32(1) / r).min(2)


def exact_sum(v):
    """Sum of a float array as an exact rational."""
    return sum((Fraction(float(t)) for t in np.asarray(v).ravel()), Fraction(0))


def metric(wh, k, thr):
    """What cft_anchor_metric returns, from the rules: integer counts, exact sums, and bpr / aat formed in float32."""
    thr = np.float32(thr)
    x = ratio_x(wh, k)
    best = x.max(1)
    n = x.shape[0]
    out = {"n_best_above": int((best > thr).sum()), "n_x_above": int((x > thr).sum()), "sum_x": exact_sum(x), "sum_best": exact_sum(best),
           "sum_x_above": exact_sum(x[x > thr]), "sum_best_above": exact_sum(best[best > thr])}
    out["bpr"] = np.float32(out["n_best_above"]) / np.float32(n)
    out["aat"] = np.float32(out["n_x_above"]) / np.float32(n)
    return out


def fitness_sum(wh, k, thr):
    """S = sum of best * 2^29 over best > thr, an integer (thr >= 2^-6)."""
    thr = np.float32(thr)
    assert np.float32(2.0 ** -6) <= thr <= np.float32(1)
    best = ratio_x(wh, np.asarray(k, np.float64).astype(np.float32)).max(1)
    t = best[best > thr].astype(np.float64) * float(1 << SHIFT)
    assert (t == np.floor(t)).all()
    return int(t.astype(np.int64).sum())


def fitness(wh, k, thr):
    """The exact fitness: float32(S / (2^29 n))."""
    n = len(wh)
    assert n < 1 << 24
    return np.float32(np.float64(fitness_sum(wh, k, thr)) / (float(1 << SHIFT) * n))


def torch_style_fitness(wh, k, thr):
    """(best * (best > thr)).mean() in float32 with numpy's (pairwise) summation: one of the orders a float32 mean can take."""
    best = ratio_x(wh, np.asarray(k, np.float64).astype(np.float32)).max(1)
    return (best * (best > np.float32(thr)).astype(np.float32)).mean(dtype=np.float32)


def draw_restarts(n, k, iters=30):
    """The rows scipy's kmeans starts its restarts from: rng.choice(n, size=k, replace=False) per restart, numpy's global state."""
    rng = np.random.mtrand._rand
    return np.stack([rng.choice(n, size=int(k), replace=False) for _ in range(iters)])


def kmeans_once(obs, book):
    """scipy's _kmeans: returns (book, mean distance, iterations)."""
    prev, it = np.inf, 0
    while True:
        d0 = book[None, :, 0] - obs[:, None, 0]
        d1 = book[None, :, 1] - obs[:, None, 1]
        ds = d0 * d0 + d1 * d1                               # two roundings per product-sum: numpy does not fuse
        code = ds.argmin(1)                                  # the first strictly smallest
        avg = np.sqrt(ds[np.arange(len(obs)), code]).mean()
        kc = len(book)
        cnt = np.bincount(code, minlength=kc)
        with np.errstate(invalid="ignore", divide="ignore"):
            new = np.stack([np.bincount(code, weights=obs[:, 0], minlength=kc) / cnt,
                            np.bincount(code, weights=obs[:, 1], minlength=kc) / cnt], 1)
        book = new[cnt > 0]
        it += 1
        diff = abs(prev - avg)
        prev = avg
        if not diff > KMEANS_THRESH:
            return book, avg, it


def kmeans(obs, k, idx):
    """scipy.cluster.vq.kmeans(obs, k, iter=len(idx)) with the given starting rows: (book, distortion, winning restart)."""
    obs = np.asarray(obs, np.float64)
    best_book, best_dist, best_r = None, np.inf, -1
    for r, rows in enumerate(idx):
        book, dist, _ = kmeans_once(obs, obs[np.asarray(rows)])
        if dist < best_dist:
            best_book, best_dist, best_r = book, dist, r
    return best_book, best_dist, best_r


def draw_mutations(shape, gen, mp=0.9, s=0.1):
    """The mutations of the genetic loop, with its redraw while nothing changed."""
    npr = np.random
    out = np.empty((gen,) + tuple(shape))
    for g in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            v = ((npr.random(shape) < mp) * npr.random() * npr.randn(*shape) * s + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def evolve(wh, k, thr, v):
    """The genetic loop with the exact fitness: (k, f, flags, fg)."""
    k = np.array(k, np.float64)
    f = fitness(wh, k, thr)
    flags, fgs = np.zeros(len(v), bool), np.zeros(len(v), np.float32)
    for g in range(len(v)):
        kg = (k * v[g]).clip(min=2.0)
        fg = fitness(wh, kg, thr)
        fgs[g] = fg
        if fg > f:
            f, k, flags[g] = fg, kg, True
    return k, f, flags, fgs


def label_wh(shapes, labels, img_size, scale=None):
    shapes = np.asarray(shapes)
    shapes = img_size * shapes / shapes.max(1, keepdims=True)
    if scale is not None:
        shapes = shapes * scale
    return np.concatenate([l[:, 3:5] * s for s, l in zip(shapes, labels)])


def kmean_anchors(shapes, labels, n, img_size, thr, gen):
    """kmean_anchors without its printing, numpy's global state consumed as the reference consumes it.  Returns a dict with the gen = 0
    anchors (sorted by area), the final ones (sorted), the trace, and the number of surviving clusters."""
    wh0 = label_wh(shapes, labels, img_size)
    wh = wh0[(wh0 >= 2.0).any(1)]
    s = wh.std(0)
    book, dist, _ = kmeans(wh / s, n, draw_restarts(len(wh), n))
    if len(book) != n:
        return {"survivors": len(book)}
    k = book * s
    k = k[np.argsort(k.prod(1))]
    v = draw_mutations(k.shape, gen)
    kf, f, flags, fgs = evolve(wh.astype(np.float32), k, 1. / thr, v)
    return {"survivors": n, "k0": k, "dist": dist, "k": kf[np.argsort(kf.prod(1))], "k_unsorted": kf, "f": f, "flags": flags, "fg": fgs, "v": v,
            "wh": wh.astype(np.float32), "wh0": wh0.astype(np.float32)}


def labels_of(counts, wh):
    """Per-image label arrays [m, 5] = class, x, y, w, h (float64) from the stored per-image counts and float32 sizes."""
    wh = np.asarray(wh, np.float64)
    out, o = [], 0
    for c in np.asarray(counts).tolist():
        l = np.zeros((c, 5))
        l[:, 1:3] = 0.5
        l[:, 3:5] = wh[o:o + c]
        out.append(l)
        o += c
    return out
