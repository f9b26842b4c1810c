"""The numpy definition of the edge fitting (emap_amd.edge_fitting, csrc/fitting.hip, include/emap_fit_hip.h), stage by stage, in the
kernels' scalar order: every 3-term sum is (x + y) + z, numpy's elementwise operations are IEEE and never fused.  A plain module like
gpu_helpers.py: not collected, no tests of its own, no device work.  Used by the CPU and GPU tests, by tests/golden/make_goldens_edge_fitting.py
(which asserts, with ``Margins``, that no decision of the recorded cases is within 1e-9 of its threshold) and by scripts/bench_edge_fitting.py.

The rules that make the reference's random routines reproducible (the reference draws seeds and RANSAC pairs with np.random.choice and lets
the order of list(set) decide ties): the seed of a polyline is the LOWEST unvisited index, the lowest index wins a tie, the consensus fit
looks at every pair i < j in lexicographic order."""
import numpy as np


class Margins:
    """The smallest |value - threshold| and the smallest best / second-best gap seen."""

    def __init__(self):
        self.least = np.inf
        self.n = 0

    def note(self, diff):
        d = np.abs(np.asarray(diff, dtype=np.float64)).reshape(-1)
        d = d[np.isfinite(d)]
        if d.size:
            self.least = min(self.least, float(d.min()))
            self.n += int(d.size)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def norm3(a):
    return np.sqrt(dot3(a, a))


# ---------------------------------------------------------------------------------------------------------------- the test clouds
def wire_cloud(res, seed, segments):
    """(N, 6) points and unit directions: the segments (m, 2, 3) and two planar half circles (r = 0.55 at z = 0.3, r = 0.35 at z = -0.4),
    int(length * res) points each at the parameters (k + 0.5) / n, Gaussian noise of 0.15 / res on positions and 0.02 on directions,
    directions renormalised, rows permuted.  res 32 gives N = 466, res 64 N = 945."""
    rng = np.random.default_rng(seed)
    pts, dirs = [], []
    for a, b in np.asarray(segments, dtype=np.float64):
        length = float(np.linalg.norm(b - a))
        n = int(length * res)
        t = (np.arange(n) + 0.5) / n
        pts.append(a + t[:, None] * (b - a))
        dirs.append(np.repeat(((b - a) / length)[None], n, axis=0))
    for r, z in ((0.55, 0.3), (0.35, -0.4)):
        n = int(np.pi * r * res)
        th = np.pi * (np.arange(n) + 0.5) / n
        pts.append(np.stack([r * np.cos(th), r * np.sin(th), np.full(n, z)], axis=1))
        dirs.append(np.stack([-np.sin(th), np.cos(th), np.zeros(n)], axis=1))
    p, d = np.concatenate(pts), np.concatenate(dirs)
    p = p + rng.normal(0.0, 0.15 / res, p.shape)
    d = d + rng.normal(0.0, 0.02, d.shape)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    perm = rng.permutation(len(p))
    return np.ascontiguousarray(np.concatenate([p, d], axis=1)[perm])


# ---------------------------------------------------------------------------------------------------------------- voxel down-sample
def voxel_down_sample_ref(points, colors, voxel_size):
    """One point per occupied voxel: the mean of the voxel's points and colours; voxel index floor((p - (min - voxel / 2)) / voxel), the
    output ordered by index, first axis slowest."""
    p, c = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(colors, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return p, c
    idx = np.floor((p - (p.min(axis=0) - voxel_size / 2)) / voxel_size).astype(np.int64)
    keys, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv, minlength=len(keys)).astype(np.float64)
    op, oc = np.zeros((len(keys), 3)), np.zeros((len(keys), 3))
    np.add.at(op, inv, p)
    np.add.at(oc, inv, c)
    return op / cnt[:, None], oc / cnt[:, None]


def line_directions_ref(colors):
    d = np.asarray(colors, np.float64) * 2 - 1
    return d / (np.linalg.norm(d, axis=1)[:, None] + 1e-6)


# ---------------------------------------------------------------------------------------------------------------- linking
def link_ref(points, thr, angle, nms, keep_short, margins=None, stats=None):
    """connect_points as an all-points scan.  -> list of lists of indices.  ``stats``: a dict that receives the numbers of steps (the
    last, failing step of every direction included) and seeds."""
    P = np.asarray(points, np.float64).reshape(-1, 6)
    n = len(P)
    X, D = P[:, :3], P[:, 3:6]
    visited = np.zeros(n, bool)
    one_m = 1.0 - angle

    def step(s, fwd):
        e = X - X[s]
        dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        if margins is not None:
            margins.note(dist[~visited] - thr)
        idx = np.nonzero(~visited & (dist < thr))[0]
        if len(idx) == 0:
            return 0, -1
        u = e[idx] / (dist[idx] + 1e-6)[:, None]
        dot = (u[:, 0] * D[s, 0] + u[:, 1] * D[s, 1]) + u[:, 2] * D[s, 2]
        key = dot if fwd else -dot
        ok = ~np.isnan(key)
        if not ok.any():
            return 0, -1
        b = int(np.nonzero(ok & (key == key[ok].max()))[0][0])        # idx ascends: the lowest index among equals
        w, dw = int(idx[b]), dot[b]
        if margins is not None:
            margins.note(np.delete(key, b)[ok[np.arange(len(key)) != b]] - key[b])
            margins.note([dw - one_m] if fwd else [abs(dw) - one_m, dw])
        if (dw <= one_m) if fwd else (abs(dw) <= one_m or dw >= 0):
            return 0, -1
        lim = nms * dw
        dc = dist[idx]
        mark = (dc <= dc[b]) & (dot < dw) & (dot >= lim) if fwd else (dc <= dc[b]) & (dot > dw) & (dot <= lim)
        mark[b] = False
        if margins is not None:
            others = np.arange(len(idx)) != b
            margins.note((dc - dc[b])[others])
            margins.note((dot - lim)[others])
        visited[idx[mark]] = True
        dv = D[w] if fwd else -D[w]
        t = (dv[0] * u[b, 0] + dv[1] * u[b, 1]) + dv[2] * u[b, 2]
        if margins is not None:
            margins.note([t - 0.5])
        if t <= 0.5:
            return 1, w
        visited[w] = True
        return 2, w

    out, cursor, steps, seeds = [], 0, 0, 0
    for _ in range(n):
        while cursor < n and visited[cursor]:
            cursor += 1
        if cursor >= n:
            break
        seed = cursor
        seeds += 1
        visited[seed] = True
        line = [seed]
        for fwd in (True, False):
            anchor = seed
            for _ in range(n):
                st, w = step(anchor, fwd)
                steps += 1
                if st == 0:
                    break
                line.append(w) if fwd else line.insert(0, w)
                if st == 1:
                    break
                anchor = w
        if len(line) > (1 if keep_short else 3):
            out.append(line)
    if stats is not None:
        stats.update(steps=steps, seeds=seeds)
    return out


def chain_offsets(polylines):
    """list of lists -> (chain int32, offsets int32), the kernel's two outputs"""
    off = np.zeros(len(polylines) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in polylines])
    chain = np.array([i for p in polylines for i in p], dtype=np.int32)
    return chain, off


# ---------------------------------------------------------------------------------------------------------------- consensus lines
def principal_direction_ref(pts):
    """Unit principal direction of the centred points, signed so that u . (last - first) >= 0."""
    q = np.asarray(pts, np.float64)
    u = np.linalg.svd(q - q.mean(axis=0), full_matrices=False)[2][0]
    u = u / np.linalg.norm(u)
    return -u if np.dot(u, q[-1] - q[0]) < 0 else u


def lines_ref(pts, inlier_thr, min_inliers, max_lines, margins=None):
    """The exhaustive consensus fit of one polyline (n, 3).  -> (segments (k, 6), labels (n) int32: line number or -1)."""
    P = np.asarray(pts, np.float64).reshape(-1, 3)
    n0 = len(P)
    remaining = np.arange(n0)
    labels = np.full(n0, -1, np.int32)
    segs = []
    for _ in range(max_lines):
        m = len(remaining)
        if m < min_inliers:
            break
        Q = P[remaining]
        best, best_ij, best_mask = 0, None, None
        for i in range(m - 1):
            e = Q[i + 1:] - Q[i]
            nrm = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
            u = e / nrm[:, None]                                          # rows of pairs the kernel skips are dropped below
            v = Q - Q[i]
            cx = v[None, :, 1] * u[:, None, 2] - v[None, :, 2] * u[:, None, 1]
            cy = v[None, :, 2] * u[:, None, 0] - v[None, :, 0] * u[:, None, 2]
            cz = v[None, :, 0] * u[:, None, 1] - v[None, :, 1] * u[:, None, 0]
            dist = np.sqrt((cx * cx + cy * cy) + cz * cz)
            usable = ~(nrm < 1e-6)
            if margins is not None:
                margins.note(dist[usable] - inlier_thr)
                margins.note(nrm - 1e-6)
            mask = (dist < inlier_thr) & usable[:, None]
            cnt = mask.sum(axis=1)
            if cnt.size and cnt.max() > best:
                r = int(np.argmax(cnt))                                  # the first maximum: the lowest j
                best, best_ij, best_mask = int(cnt[r]), (i, i + 1 + r), mask[r]
            if best == m:                                                # every point: no later pair can have more, and > is strict
                break
        if best == 0 or best < min_inliers or best / n0 < 1.0 / max_lines:
            break
        inl = Q[best_mask]
        u = principal_direction_ref(inl)
        p1 = Q[best_ij[0]]
        proj = dot3(inl - p1, u[None])
        segs.append(np.concatenate([p1 + proj.min() * u, p1 + proj.max() * u]))
        labels[remaining[best_mask]] = len(segs) - 1
        remaining = remaining[~best_mask]
    return np.array(segs).reshape(-1, 6), labels


def split_sublists_ref(numbers, max_long=2, min_length=4):
    """split_into_monotonic_sublists with a defined order: runs of consecutive indices, longer first, equal lengths by first index."""
    runs, cur = [], []
    for v in numbers:
        if cur and v == cur[-1] + 1:
            cur.append(v)
        else:
            if len(cur) > 1:
                runs.append(cur)
            cur = [v]
    if len(cur) > 1:
        runs.append(cur)
    runs.sort(key=lambda r: (-len(r), r[0]))
    long_runs, short_runs = runs[:max_long], runs[max_long:]
    curves = []
    for r in long_runs:
        (curves if len(r) >= min_length else short_runs).append(r)
    pairs = [[r[j], r[j + 1]] for r in short_runs for j in range(len(r) - 1)]
    return curves, pairs


# ---------------------------------------------------------------------------------------------------------------- Beziers
def bernstein_matrix(n):
    t = np.linspace(0, 1, n)
    s = 1 - t
    return np.stack([s * s * s, 3 * t * s * s, 3 * t * t * s, t * t * t], axis=1)


def bezier_ref(pts):
    """Linear least squares for the 4 control points at t = linspace(0, 1, n).  -> (ctrl (12), rmse)."""
    q = np.asarray(pts, np.float64).reshape(-1, 3)
    B = bernstein_matrix(len(q))
    ctrl = np.linalg.lstsq(B, q, rcond=None)[0]
    res = q - B @ ctrl
    return ctrl.reshape(-1), float(np.sqrt(np.mean(np.sum(res ** 2, axis=1))))


# ---------------------------------------------------------------------------------------------------------------- edge_fitting
def edge_fitting_ref(polylines, res, min_inliers=4, max_lines=3, max_curves=2, keep_short_lines=True, margins=None):
    """edge_fitting of the reference over polylines (each (n, >= 3)).  -> dict(lines (L, 6), raw_lines list of (k, 3), curves (C, 12),
    raw_curves list of (k, 3), labels list of (n) int32 for the polylines that went through the consensus fit)."""
    lines, raw_lines, curves, raw_curves, all_labels = [], [], [], [], []
    for poly in polylines:
        xyz = np.asarray(poly, np.float64)[:, :3]
        if len(xyz) < 4 and keep_short_lines:
            for i in range(len(xyz) - 1):
                lines.append(np.concatenate([xyz[i], xyz[i + 1]]))
                raw_lines.append(xyz[i:i + 2].copy())
            continue
        segs, labels = lines_ref(xyz, 1.0 / res, min_inliers, max_lines, margins)
        all_labels.append(labels)
        for k, s in enumerate(segs):
            lines.append(s)
            raw_lines.append(xyz[labels == k])
        remaining = np.nonzero(labels < 0)[0].tolist()
        if remaining:
            cand, pairs = split_sublists_ref(remaining, max_curves)
            if keep_short_lines:
                for a, b in pairs:
                    lines.append(np.concatenate([xyz[a], xyz[b]]))
                    raw_lines.append(xyz[[a, b]])
            for c in cand:
                ctrl, rmse = bezier_ref(xyz[c])
                if margins is not None:
                    margins.note([rmse - 5.0 / res])
                if rmse > 5.0 / res:
                    continue
                curves.append(ctrl)
                raw_curves.append(xyz[c])
    return dict(lines=np.array(lines).reshape(-1, 6), raw_lines=raw_lines, curves=np.array(curves).reshape(-1, 12), raw_curves=raw_curves,
                labels=all_labels)


# ---------------------------------------------------------------------------------------------------------------- merging
def components_ref(adj):
    """Labels = smallest member index of every connected component of the symmetric boolean matrix."""
    n = len(adj)
    lab = np.arange(n)
    for _ in range(n + 1):
        new = lab.copy()
        for i in range(n):
            nb = np.nonzero(adj[i])[0]
            if len(nb):
                new[i] = min(new[i], lab[nb].min())
        new = np.minimum(new, new[new])
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def seg_point_dist_ref(seg, q):
    p1, dl = seg[:3], seg[3:] - seg[:3]
    with np.errstate(invalid="ignore", divide="ignore"):
        u = dot3(q - p1, dl) / dot3(dl, dl)
    u = 0.0 if u < 0 else (1.0 if u > 1 else u)
    return norm3((p1 + u * dl) - q)


def lines_adjacency_ref(lines, dist_thr, similarity, margins=None):
    L = len(lines)
    adj = np.zeros((L, L), bool)
    d = lines[:, 3:] - lines[:, :3]
    nrm = norm3(d)
    nd = d / np.where(nrm == 0, 1.0, nrm)[:, None]
    for i in range(L):
        for j in range(i + 1, L):
            d0, d1 = seg_point_dist_ref(lines[i], lines[j, :3]), seg_point_dist_ref(lines[i], lines[j, 3:])
            dist = d1 if d1 < d0 else d0
            cos = dot3(nd[i], nd[j])
            if margins is not None:
                margins.note([dist - dist_thr, cos - similarity])
            adj[i, j] = adj[j, i] = bool(dist <= dist_thr and cos >= similarity)
    return adj


def refit_ref(pts):
    q = np.asarray(pts, np.float64).reshape(-1, 3)
    c = q.mean(axis=0)
    u = principal_direction_ref(q)
    proj = dot3(q - c, u[None])
    return np.concatenate([c + u * proj.min(), c + u * proj.max()])


def merge_lines_ref(lines, raw_lines, dist_thr, similarity, margins=None):
    """-> (merged (n_components, 6) in ascending smallest member, labels (L))"""
    lines = np.asarray(lines, np.float64).reshape(-1, 6)
    lab = components_ref(lines_adjacency_ref(lines, dist_thr, similarity, margins))
    out = []
    for root in np.unique(lab):
        members = np.nonzero(lab == root)[0]
        out.append(lines[root] if len(members) == 1 else refit_ref(np.concatenate([np.asarray(raw_lines[k], np.float64).reshape(-1, 3) for k in members])))
    return np.array(out).reshape(-1, 6), lab


def merge_endpoints_ref(endpoints, dist_thr, margins=None):
    """-> (merged (E, 3), labels (E))"""
    e = np.asarray(endpoints, np.float64).reshape(-1, 3)
    diff = e[:, None] - e[None]
    dist = np.sqrt((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2])
    if margins is not None:
        margins.note((dist - dist_thr)[~np.eye(len(e), dtype=bool)])
    adj = dist <= dist_thr
    np.fill_diagonal(adj, False)
    lab = components_ref(adj)
    out = e.copy()
    for root in np.unique(lab):
        members = np.nonzero(lab == root)[0]
        if len(members) > 1:
            s = np.zeros(3)
            for k in members:
                s = s + e[k]
            out[members] = s / len(members)
    return out, lab


def merge_ref(fitted, edge_thr=5.0, endpoint_thr=1.0, similarity=0.98, margins=None):
    """merge of the reference on dict(lines, raw_lines, curves) at fitted["resolution"].  -> dict(lines (L', 6), curves (C, 12),
    line_labels, endpoint_labels)"""
    res = int(fitted["resolution"])
    lines, curves = np.asarray(fitted["lines"], np.float64).reshape(-1, 6), np.asarray(fitted["curves"], np.float64).reshape(-1, 12)
    line_labels = np.arange(len(lines))
    if len(lines):
        lines, line_labels = merge_lines_ref(lines, fitted["raw_lines"], edge_thr / res / 2.0, similarity, margins)
    ends = np.concatenate([lines.reshape(-1, 3), curves[:, [0, 1, 2, 9, 10, 11]].reshape(-1, 3)])
    merged, end_labels = merge_endpoints_ref(ends, endpoint_thr / res, margins)
    L = len(lines)
    out_curves = curves.copy()
    if len(curves):
        ce = merged[2 * L:].reshape(-1, 6)
        out_curves[:, :3], out_curves[:, 9:] = ce[:, :3], ce[:, 3:]
    return dict(lines=merged[:2 * L].reshape(-1, 6), curves=out_curves, line_labels=line_labels, endpoint_labels=end_labels)


# ---------------------------------------------------------------------------------------------------------------- comparisons
def unordered_pairs_close(a, b, tol):
    """rows (.., 6) equal as unordered pairs of end points"""
    a, b = np.asarray(a).reshape(-1, 6), np.asarray(b).reshape(-1, 6)
    if a.shape != b.shape:
        return False
    same = np.abs(a - b).max(axis=1, initial=0) <= tol
    swap = np.abs(a - b[:, [3, 4, 5, 0, 1, 2]]).max(axis=1, initial=0) <= tol
    return bool((same | swap).all())


def canonical_rows(a, width):
    """rows sorted after each row is put in its canonical direction (the smaller end first): for set comparisons"""
    a = np.asarray(a, np.float64).reshape(-1, width)
    if len(a) == 0:
        return a
    rev = a.reshape(len(a), -1, 3)[:, ::-1].reshape(len(a), width)
    flip = np.array([tuple(r[:3]) > tuple(r[-3:]) for r in a])
    c = np.where(flip[:, None], rev, a)
    return c[np.lexsort(c.T[::-1])]


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return len(a) == len(b) and len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))
