"""CPU yardsticks of the parametric-edge tests (tests/test_parametric_edges_cpu.py, tests/test_gpu_parametric_edges.py): vectorised numpy
restatements of the reference's bezier_curve_length (src/eval/eval_util.py:90-135), get_pred_points_and_directions (:300-415) /
process_geometry_data (src/edge_extraction/extract_parametric_edge.py:65-134) and compute_visibility (:137-213), and the fixture of
tests/golden/g22_parametric_edges.npz.  Nothing here imports the package under test (the fixture takes the wire frame as an argument)."""
import hashlib

import numpy as np

M = np.array([[-1, 3, -3, 1], [3, -6, 3, 0], [-3, 3, 0, 0], [1, 0, 0, 0]], dtype=np.float64)       # the reference's Bernstein matrix


def derivative_ref(curves, t):
    """derivative_bezier (:94-105) of (C, 4, 3) curves at t (C, ...): the three terms in index order.  -> (C, ..., 3)"""
    d = curves[:, 1:] - curves[:, :-1]
    d = d.reshape((len(curves), 3) + (1,) * (t.ndim - 1) + (3,))
    t = t[..., None]
    return (3 * (1 - t) ** 2 * d[:, 0] + 6 * (1 - t) * t * d[:, 1]) + 3 * t ** 2 * d[:, 2]


def bezier_lengths_ref(curves, num_samples=100, chunk=64):
    """bezier_curve_length for every curve of (C, 4, 3): the nested composite Simpson rule, all sub-intervals at once.  The sums are
    numpy's (pairwise), the reference's and the kernel's are sequential: a few ulps apart on 1.01e4 positive terms."""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 4, 3)
    ns = int(num_samples)
    s = np.arange(ns)
    a, b = s / ns, (s + 1) / ns
    h = (b - a) / ns
    i = np.arange(ns + 1)
    t = a[:, None] + i[None, :] * h[:, None]                                  # (ns, ns + 1): a + i h; column ns is replaced by b
    out = np.zeros(len(curves))
    for c0 in range(0, len(curves), chunk):
        cv = curves[c0:c0 + chunk]
        speed = np.linalg.norm(derivative_ref(cv, np.broadcast_to(t, (len(cv),) + t.shape)), axis=-1)      # (c, ns, ns + 1)
        end = np.linalg.norm(derivative_ref(cv, np.broadcast_to(b, (len(cv), ns))), axis=-1)              # (c, ns)
        sum1 = speed[:, :, 1:ns:2].sum(axis=2)
        sum2 = speed[:, :, 2:ns - 1:2].sum(axis=2) if ns > 3 else np.zeros_like(sum1)
        out[c0:c0 + chunk] = ((speed[:, :, 0] + 4 * sum1 + 2 * sum2 + end) * h / 3).sum(axis=1)
    return out


def lengths_counts_ref(curves, lines, resolution=0.005, num_samples=100):
    """Lengths and sample counts int(length // resolution) of curves (C, 4, 3) then lines (L, 2, 3)."""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 4, 3)
    lines = np.asarray(lines, dtype=np.float64).reshape(-1, 2, 3)
    lengths = np.concatenate([bezier_lengths_ref(curves, num_samples), np.linalg.norm(lines[:, 0] - lines[:, 1], axis=1)])
    return lengths, (lengths // resolution).astype(np.int64)


def sample_edges_ref(curves, lines, resolution=0.005, num_samples=100):
    """The sampling loops of get_pred_points_and_directions / process_geometry_data: -> points (n, 3), directions (n, 3), edge_id (n),
    counts (C + L), lengths (C + L), n_curve_points.  Curve directions by the reference's expression (:340-385), which is NOT the
    derivative (A and B hold its factors 3 and 2 and are multiplied by 3 t^2 and 2 t again); tangents_ref has the tangents.  Line points as
    process_geometry_data's np.outer(t, p1 - p0) + p0 (:131)."""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 4, 3)
    lines = np.asarray(lines, dtype=np.float64).reshape(-1, 2, 3)
    lengths, counts = lengths_counts_ref(curves, lines, resolution, num_samples)
    pts, dirs, eid = [np.zeros((0, 3))], [np.zeros((0, 3))], [np.zeros(0, np.int32)]
    with np.errstate(invalid="ignore", divide="ignore"):
        for e, P in enumerate(curves):
            t = np.linspace(0, 1, counts[e])
            U = np.array([t ** 3, t ** 2, t, np.ones_like(t)])
            pts.append(U.T.dot(M).dot(P))
            A, B, C = -3 * P[0] + 9 * P[1] - 9 * P[2] + 3 * P[3], 6 * P[0] - 12 * P[1] + 6 * P[2], -3 * P[0] + 3 * P[1]
            v = A[None] * (3 * t ** 2)[:, None] + B[None] * (2 * t)[:, None] + C[None]
            dirs.append(v / np.linalg.norm(v, axis=1, keepdims=True))
            eid.append(np.full(len(t), e, np.int32))
        for j, line in enumerate(lines):
            t = np.linspace(0, 1, counts[len(curves) + j])
            pts.append(np.outer(t, line[1] - line[0]) + line[0])
            direction = line[1] - line[0]
            dirs.append(np.broadcast_to(direction / (np.linalg.norm(direction) + 1e-6), (len(t), 3)))
            eid.append(np.full(len(t), len(curves) + j, np.int32))
    return np.concatenate(pts), np.concatenate(dirs), np.concatenate(eid), counts, lengths, int(counts[:len(curves)].sum())


def tangents_ref(curves, lines, counts):
    """The unit tangents at the samples of sample_edges_ref: B'(t) / |B'(t)| with derivative_ref (NaN where it vanishes), for a line
    (p1 - p0) / |p1 - p0|.  -> (n, 3)"""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 4, 3)
    lines = np.asarray(lines, dtype=np.float64).reshape(-1, 2, 3)
    out = [np.zeros((0, 3))]
    with np.errstate(invalid="ignore", divide="ignore"):
        for e, P in enumerate(curves):
            v = derivative_ref(P[None], np.linspace(0, 1, counts[e])[None])[0]
            out.append(v / np.linalg.norm(v, axis=1, keepdims=True))
        for j, line in enumerate(lines):
            d = line[1] - line[0]
            out.append(np.broadcast_to(d / np.linalg.norm(d), (int(counts[len(curves) + j]), 3)))
    return np.concatenate(out)


def project_ref(intrinsic, camtoworld, X):
    """project2D_single (:204-213) with compute_visibility's K, R, T (:156-159): (n, 3) -> (n, 2) fp64 pixel coordinates, not rounded."""
    K = np.asarray(intrinsic, dtype=np.float64)[:3, :3]
    worldtocam = np.linalg.inv(np.asarray(camtoworld, dtype=np.float64))
    R, T = worldtocam[:3, :3], worldtocam[:3, 3:]
    with np.errstate(invalid="ignore", divide="ignore"):
        x = (K @ (R @ X.reshape(-1, 3).T + T)).T
        return (x / x[:, -1:])[:, :2]


def visibility_ref(all_curve_points, all_line_points, edges, intrinsics_list, camtoworld_list, h, w, threshold, frames):
    """compute_visibility restated per (edge, frame) with fp64 means.  -> visible (E) bool, table (E, F) bool, means (E, F) (NaN: no valid
    point), n_valid (E, F), and per (edge, frame) whether every gathered value is exactly 0.0 or 1.0."""
    per_edge = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in list(all_curve_points) + list(all_line_points)]
    edges = np.asarray(edges)
    edges = edges[..., 0] if edges.ndim == 4 else edges
    E, F = len(per_edge), len(edges)
    table, means = np.zeros((E, F), bool), np.full((E, F), np.nan)
    n_valid, binary = np.zeros((E, F), np.int64), np.ones((E, F), bool)
    for f in range(F):
        for e, X in enumerate(per_edge):
            if len(X) == 0:
                continue
            uv = np.round(project_ref(intrinsics_list[f], camtoworld_list[f], X))
            ok = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
            if not ok.any():
                continue
            vals = edges[f][uv[ok, 1].astype(np.int64), uv[ok, 0].astype(np.int64)].astype(np.float64)
            n_valid[e, f], means[e, f] = len(vals), vals.sum() / len(vals)
            binary[e, f] = bool(np.all((vals == 0.0) | (vals == 1.0)))
            table[e, f] = means[e, f] > threshold and vals.max() > 0.5
    return table.sum(axis=1) > frames, table, means, n_valid, binary


def fixture(wireframe_segments):
    """The edge set of g22: -> curves (6, 4, 3), lines (25, 2, 3).  ``wireframe_segments`` is emap_amd.synthetic.wireframe_segments()."""
    rng = np.random.default_rng(22)
    a, b = wireframe_segments[:, 0], wireframe_segments[:, 1]
    segs = np.stack([a + 0.013 * (b - a), b - 0.021 * (b - a)], axis=1)
    spur = rng.uniform(-0.4, 0.4, (6, 2, 3))
    far = rng.uniform(2, 4, (3, 2, 3))
    lines = np.concatenate([np.array([[[.1, .1, .1], [.1, .1, .103]]]), segs, spur, far, np.array([[[.2, 0, 0], [.2, 0, 0]]]),
                            np.array([[[.3, 0, 0], [.3, .0073, 0]]])])

    def bulged(seg, bulge):
        p, q = seg
        d = q - p
        n = np.cross(d, [0.3, 0.5, 0.7])
        n /= np.linalg.norm(n)
        return np.array([p, p + d / 3 + bulge * n, p + 2 * d / 3 + bulge * n, q])

    s3a, s3b = segs[3]
    curves = np.stack([bulged(segs[1], 0.004), bulged(segs[5], 0.05), rng.uniform(-0.4, 0.4, (4, 3)), np.array([s3a, s3a, s3b, s3b]),
                       rng.uniform(2, 3, (4, 3)), np.tile(a[:1], (4, 1))])            # the last: four equal control points, a corner of the wire frame
    return curves, lines


def edge_dict(curves, lines):
    """A parametric_edges.json's two lists, flat per edge as the reference writes them."""
    return {"curves_ctl_pts": np.asarray(curves).reshape(-1, 12).tolist(), "lines_end_pts": np.asarray(lines).reshape(-1, 6).tolist()}


WORLDTOGT = np.array([[0.36, 0.48, -0.8, 0.11], [-0.8, 0.6, 0.0, -0.07], [0.48, 0.64, 0.6, 0.05], [0, 0, 0, 1]]) * np.array([[1.1], [1.1], [1.1], [1]])
VALID_CURVE = np.array([True, False, True, True, False, True])
VALID_LINE = np.arange(25) % 3 != 1


def ulp_diff(a, b):
    """Distance in units of the last place between two fp32 arrays of finite values of either sign."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def edges_sha256(edges):
    return hashlib.sha256(np.ascontiguousarray(edges).tobytes()).hexdigest()


def frac_margin(lengths, resolution):
    """Condition (a): over the lengths > 0 the least distance of frac(length / resolution) from 0 and 1."""
    q = np.asarray(lengths)[np.asarray(lengths) > 0] / resolution
    fr = q - np.floor(q)
    return float(np.minimum(fr, 1 - fr).min()) if len(q) else 1.0
