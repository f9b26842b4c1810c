"""The numpy mirror of include/emap_score_hip.h (emap_amd.edge_score, csrc/score.hip): the mask rule, the exact squared Euclidean distance
transform - by brute force over all pixel pairs, and separably (the column sweeps and the row minimum the kernels compute) for larger maps -,
the statistics of one set read against the distance map of another, and the Python-level dict.  All distances are integers.  A plain
module: not collected, no tests of its own."""
import math

import numpy as np

NONE = 2147483647                      # EMAP_SCORE_NONE
G_NONE = 65535                         # the workspace's "no SET pixel in this column"
BYTE_TABLE = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32).astype(np.float64)      # (double)(float)((double)b / 255.0)


def mask_ref(maps, threshold):
    """SET iff v > threshold, strictly; a NaN is not SET.  uint8: v is the table value; float32: the float widened to double."""
    m = np.asarray(maps)
    if m.ndim == 4:
        m = m[..., 0]
    assert m.dtype in (np.uint8, np.float32), m.dtype
    v = BYTE_TABLE[m] if m.dtype == np.uint8 else m.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return v > float(threshold)


def d2_brute(mask):
    """(F, h, w) bool -> (F, h, w) int32: the minimum over every SET pixel of the frame of dx^2 + dy^2; NONE in a frame without one."""
    F, h, w = mask.shape
    out = np.full((F, h, w), NONE, dtype=np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for f in range(F):
        ys, xs = np.nonzero(mask[f])
        if len(ys):
            d = (yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2
            out[f] = d.min(axis=-1)
    return out.astype(np.int32)


def column_pass(mask):
    """g (F, h, w) int64: the vertical distance to the nearest SET pixel of the same column, G_NONE without one - a sweep down, a sweep up."""
    F, h, w = mask.shape
    g = np.full((F, h, w), G_NONE, dtype=np.int64)
    dist = np.full((F, w), G_NONE, dtype=np.int64)
    for y in range(h):
        dist = np.where(mask[:, y], 0, np.where(dist == G_NONE, G_NONE, dist + 1))
        g[:, y] = dist
    dist = np.full((F, w), G_NONE, dtype=np.int64)
    for y in range(h - 1, -1, -1):
        dist = np.where(g[:, y] == 0, 0, np.where(dist == G_NONE, G_NONE, dist + 1))
        g[:, y] = np.minimum(g[:, y], dist)
    return g


def d2_separable(mask, budget=1 << 24):
    """The same map as d2_brute through the two passes: per row the minimum over the columns x' that have a SET pixel of (x - x')^2 + g^2."""
    F, h, w = mask.shape
    g = column_pass(mask)
    out = np.full((F, h, w), NONE, dtype=np.int64)
    x = np.arange(w, dtype=np.int64)
    for f in range(F):
        cols = np.nonzero(g[f, 0] != G_NONE)[0]                  # a column has a SET pixel in every row's g or in none
        if not len(cols):
            continue
        dx2 = (x[:, None] - cols[None, :]) ** 2                  # (w, n)
        rows = max(1, budget // dx2.size)
        for y0 in range(0, h, rows):
            g2 = g[f, y0:y0 + rows][:, cols] ** 2                # (r, n)
            out[f, y0:y0 + rows] = (dx2[None] + g2[:, None, :]).min(axis=-1)
    assert out.max() <= NONE
    return out.astype(np.int32)


def limits_ref(thresholds):
    """The fp64 products t * t the counts compare (double)d with."""
    with np.errstate(over="ignore"):                             # a huge threshold squares to +inf: every distance but NONE is within it
        return [np.float64(t) * np.float64(t) for t in thresholds]


def stats_ref(mask_a, d2_b, thresholds, ids=None, n_ids=None):
    """-> counts (F, 1 + K) int64, sums (F) float64 (math.fsum: the exactly rounded sum), edge_counts (n_ids, 1 + K) int64 or None."""
    F = mask_a.shape[0]
    K = len(thresholds)
    lim = limits_ref(thresholds)
    counts, sums = np.zeros((F, 1 + K), dtype=np.int64), np.zeros(F, dtype=np.float64)
    edge = None if ids is None else np.zeros((n_ids, 1 + K), dtype=np.int64)
    for f in range(F):
        d = d2_b[f][mask_a[f]].astype(np.int64)
        within = [(d != NONE) & (d.astype(np.float64) <= lim[k]) for k in range(K)]
        counts[f, 0] = d.size
        for k in range(K):
            counts[f, 1 + k] = int(within[k].sum())
        if d.size:
            sums[f] = math.inf if (d == NONE).any() else math.fsum(np.sqrt(d.astype(np.float64)))
        if ids is not None:
            e = ids[f][mask_a[f]]
            ok = (e >= 0) & (e < n_ids)
            np.add.at(edge[:, 0], e[ok], 1)
            for k in range(K):
                np.add.at(edge[:, 1 + k], e[ok & within[k]], 1)
    return counts, sums, edge


def f_score_ref(p, r):
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2 * p * r / (p + r)


def score_ref(pred, gt, thresholds=(1.0, 2.0, 4.0), pred_threshold=0.5, gt_threshold=0.5, ids=None, n_ids=None, d2=d2_separable):
    """The dict of emap_amd.edge_score.score_edge_maps from the mirror's own statistics: pooled values, and (F,) arrays under "per_frame"."""
    mp, mg = mask_ref(pred, pred_threshold), mask_ref(gt, gt_threshold)
    cp, sp, ec = stats_ref(mp, d2(mg), thresholds, ids, n_ids)
    cg, sg, _ = stats_ref(mg, d2(mp), thresholds)

    def div(a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64)

    def metrics(cp, sp, cg, sg):
        out = {"n_pred": cp[..., 0], "n_gt": cg[..., 0]}
        for k, t in enumerate(thresholds):
            p, r = div(cp[..., 1 + k], cp[..., 0]), div(cg[..., 1 + k], cg[..., 0])
            out[f"precision_{t}"], out[f"recall_{t}"], out[f"fscore_{t}"] = p, r, f_score_ref(p, r)
        out["acc_px"], out["comp_px"] = div(sp, cp[..., 0]), div(sg, cg[..., 0])
        out["chamfer_px"] = out["acc_px"] + out["comp_px"]
        return out
    out = {k: int(v) if k in ("n_pred", "n_gt") else float(v) for k, v in metrics(cp.sum(0), sp.sum(), cg.sum(0), sg.sum()).items()}
    out["per_frame"] = metrics(cp, sp, cg, sg)
    if ids is not None:
        out["edge_pixels"] = ec[:, 0]
        for k, t in enumerate(thresholds):
            out[f"edge_support_{t}"] = div(ec[:, 1 + k], ec[:, 0])
    return out


def random_masks(F, h, w, density, seed):
    """(F, h, w) bool, each pixel SET with probability `density`."""
    return np.random.default_rng(seed).random((F, h, w)) < density


def maps_of(mask, dtype, seed=0):
    """A map of `dtype` whose mask at threshold 0.5 is `mask`: SET pixels get values above 0.5, the others values at or below it - the
    threshold itself and, for float32, a NaN among them."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return np.where(mask, rng.integers(128, 256, mask.shape), rng.integers(0, 128, mask.shape)).astype(np.uint8)
    lo = rng.choice(np.array([0.0, 0.25, 0.5, np.nan, -1.0], dtype=np.float32), size=mask.shape)
    hi = rng.choice(np.array([0.50000006, 0.75, 1.0, 3.0, np.inf], dtype=np.float32), size=mask.shape)
    return np.where(mask, hi, lo).astype(np.float32)
