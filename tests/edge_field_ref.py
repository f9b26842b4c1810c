"""The scalar-order numpy mirror of include/emap_field_hip.h (emap_amd.edge_field, csrc/field.hip): every formula of the header in IEEE
doubles, one numpy operation per arithmetic operation (numpy fuses nothing), every sum in the header's order - what the device result must
equal bit for bit -, and the inputs the CPU and the GPU tests share.  A plain module: not collected, no tests of its own, no device work."""
import math

import numpy as np

from emap_amd import synthetic
import edge_raster_ref as RR

STATS_THREADS = 1024                   # FIELD_STATS_THREADS of csrc/field.hip (the tests assert that the source says so)


def expand_ref(lines, curves, curve_segments):
    """-> segs (n_seg, 2, 3) float64, seg_edge (n_seg) int32: lines first, then curve by curve, chord k from B(k / n) to B((k + 1) / n)."""
    lines = np.asarray(lines, dtype=np.float64).reshape(-1, 2, 3)
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 4, 3)
    n = int(curve_segments)
    segs, edge = [lines], [np.arange(len(lines))]
    for c in range(len(curves)):
        for k in range(n):
            a = RR.bezier_ref(curves[c], np.float64(k) / np.float64(n))
            b = RR.bezier_ref(curves[c], np.float64(k + 1) / np.float64(n))
            segs.append(np.stack([a, b])[None])
            edge.append(np.array([len(lines) + c]))
    return np.concatenate(segs).astype(np.float64), np.concatenate(edge).astype(np.int32)


def pair_ref(p, a, b):
    """(d2, tt) of the points p (n, 3) float64 against ONE segment a -> b, in the header's grouping."""
    with np.errstate(all="ignore"):
        ux, uy, uz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
        uu = (ux * ux + uy * uy) + uz * uz
        r = np.float64(0.0) if uu == 0 else np.float64(1.0) / uu
        q = ((p[:, 0] - a[0]) * ux + (p[:, 1] - a[1]) * uy) + (p[:, 2] - a[2]) * uz
        qr = q * r
        lo = np.where(qr > 0.0, qr, 0.0)                         # a NaN and -0 give +0
        tt = np.where(lo < 1.0, lo, 1.0)
        ex, ey, ez = p[:, 0] - (a[0] + tt * ux), p[:, 1] - (a[1] + tt * uy), p[:, 2] - (a[2] + tt * uz)
        d2 = (ex * ex + ey * ey) + ez * ez
    return d2, tt


def point_distances_ref(points, segs):
    """-> d2 (n) float64, seg (n) int32, t (n) float64: a loop over the segments in rising index; a candidate wins by d2 < best, or against
    nothing when its d2 is not a NaN (equal d2: the earlier, lower index stays).  float32 points are widened exactly."""
    p = np.asarray(points).astype(np.float64)
    segs = np.asarray(segs, dtype=np.float64)
    n = len(p)
    best, seg, t = np.full(n, np.nan), np.full(n, -1, dtype=np.int32), np.zeros(n)
    for s in range(len(segs)):
        d2, tt = pair_ref(p, segs[s, 0], segs[s, 1])
        with np.errstate(invalid="ignore"):
            win = (d2 < best) | ((seg < 0) & ~np.isnan(d2))
        best, seg, t = np.where(win, d2, best), np.where(win, np.int32(s), seg), np.where(win, tt, t)
    return best, seg, t


def tree_sum(values, threads=STATS_THREADS):
    """The header's order: element i belongs to thread i mod threads, which adds in ascending i from 0.0; then partial t + s into partial t
    for s = threads / 2, ..., 1."""
    v = np.asarray(values, dtype=np.float64)
    part = np.zeros(threads)
    with np.errstate(invalid="ignore"):
        for start in range(0, len(v), threads):
            chunk = v[start:start + threads]
            part[:len(chunk)] = part[:len(chunk)] + chunk
        s = threads // 2
        while s:
            part[:s] = part[:s] + part[s:2 * s]
            s //= 2
    return part[0]


def stats_ref(d2, thresholds, ids=None, n_ids=None):
    """-> counts (1 + K) int64, sums (2) float64 - sums[0] in the header's order -, edge_counts (n_ids, 1 + K) int64 or None."""
    d2 = np.asarray(d2, dtype=np.float64)
    K = len(thresholds)
    with np.errstate(over="ignore", invalid="ignore"):
        lim = [np.float64(t) * np.float64(t) for t in thresholds]
        within = [d2 < lim[k] for k in range(K)]
        root = np.sqrt(d2)
    counts = np.array([len(d2)] + [int(w.sum()) for w in within], dtype=np.int64)
    ok = ~np.isnan(d2)
    sums = np.array([tree_sum(root), d2[ok].max() if ok.any() else 0.0])
    edge = None
    if ids is not None:
        ids = np.asarray(ids)
        edge = np.zeros((n_ids, 1 + K), dtype=np.int64)
        inside = (ids >= 0) & (ids < n_ids)
        np.add.at(edge[:, 0], ids[inside], 1)
        for k in range(K):
            np.add.at(edge[:, 1 + k], ids[inside & within[k]], 1)
    return counts, sums, edge


def fsum_of_roots(d2):
    """math.fsum of sqrt(d2): the exactly rounded sum the summation bound is stated against."""
    return math.fsum(np.sqrt(np.asarray(d2, dtype=np.float64)).tolist())


def chord_deviation(curves, curve_segments, samples=4097):
    """The largest distance from `samples` points of each true cubic to its own chords."""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 4, 3)
    worst = 0.0
    for c in range(len(curves)):
        segs, _ = expand_ref([], curves[c:c + 1], curve_segments)
        pts = np.stack([RR.bezier_ref(curves[c], t) for t in np.linspace(0.0, 1.0, samples)])
        worst = max(worst, float(np.sqrt(point_distances_ref(pts, segs)[0].max())))
    return worst


# ------------------------------------------------------------------------------------------------ the shared inputs
TIE_SEGMENTS = np.array([[[-0.5, 0.0, 0.0], [-0.5, 1.0, 0.5]], [[0.5, 0.0, 0.0], [0.5, 1.0, 0.5]]])
TIE_POINT = np.array([0.0, 0.3, 0.7])


def make_segments(n_seg, seed=0, nan_segment=True):
    """n_seg segments: the curved wire frame at 32 chords (204 segments) as far as it goes, then seeded segments in [-1, 1]^3; from four
    segments on, slots 1 .. 3 hold a zero-length segment, a segment with a NaN coordinate and a copy of segment 0 (a tie)."""
    lines, curves = synthetic.curved_wireframe()
    wire, _ = expand_ref(lines, curves, 32)
    rng = np.random.default_rng(1000 + seed)
    segs = np.concatenate([wire, rng.uniform(-1.0, 1.0, (max(n_seg - len(wire), 0), 2, 3))])[:n_seg].copy()
    if n_seg >= 4:
        segs[1, 1] = segs[1, 0]
        if nan_segment:
            segs[2, 0, 1] = np.nan
        segs[3] = segs[0]
    return segs


def tie_table(n_seg, first):
    """n_seg segments far from TIE_POINT (seeded, moved 10 down the z axis) with the symmetric pair TIE_SEGMENTS at `first` and
    `first + 1`: the point's two nearest segments, at bit-equal d2."""
    segs = np.random.default_rng(3000 + n_seg).uniform(-1.0, 1.0, (n_seg, 2, 3))
    segs[:, :, 2] -= 10.0
    segs[first:first + 2] = TIE_SEGMENTS
    return segs


def make_points(n, seed=0, dtype=np.float64):
    """n seeded points in [-1, 1]^3 of `dtype`; from three points on, point 1 is TIE_POINT and point 2 has a NaN coordinate."""
    p = np.random.default_rng(2000 + seed).uniform(-1.0, 1.0, (n, 3))
    if n >= 3:
        p[1] = TIE_POINT
        p[2, 2] = np.nan
    return p.astype(dtype)


