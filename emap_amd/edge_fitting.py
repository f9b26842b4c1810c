"""Parametric edge fitting and merging on the device: the reference's ``src/edge_extraction/edge_fitting`` (``connect_points``,
``edge_fitting``, ``edge_fit``) and ``src/edge_extraction/merging`` (``merge``), and ``get_parametric_edge`` of
``src/edge_extraction/extract_parametric_edge.py:216-300`` on top of them - the step between the extracted point cloud
(``extraction.get_pointcloud_from_udf``) and the ``parametric_edges.json`` that ``parametric_edges`` / ``dtu_eval`` score.

Kernels: csrc/fitting.hip behind include/emap_fit_hip.h (``_lib.fit_api()``); all device arithmetic is fp64 without FMA contraction and
every result is a pure function of its inputs.  The scalar-order numpy restatement of every stage is tests/edge_fitting_ref.py.  There is no
CPU fallback for the kernels; the host-side argument checks run before any HIP call.

Where the reference is random, this module follows rules a second implementation can reproduce:

* ``connect_points`` seeds a polyline at the LOWEST unvisited index (the reference: ``np.random.choice``) and resolves equal dot products by
  the lowest index (the reference: the order of ``list(set)``).  With ``np.random.choice`` patched to the lowest index the reference gives
  the same polylines (tests/golden/make_goldens_edge_fitting.py).
* The line fit is the reference's RANSAC as ``max_iterations -> infinity``, not its 100 seeded draws: EVERY pair i < j of the remaining
  points is a hypothesis, the first pair in lexicographic order with the most inliers wins.  It is deterministic and its inlier count is at
  least that of any draw.  ``max_iterations`` is accepted and unused.
* Bezier curves: ``curve_fit`` with ``t`` fixed to ``linspace(0, 1, n)`` is a linear least-squares problem; it is solved directly (normal
  equations in the Bernstein basis), where the reference stops at its optimiser's tolerance (1e-8).
* ``split_into_monotonic_sublists`` orders sublists of equal length by their first index (the reference: a set's order).

The voxel down-sampling that replaces open3d's ``voxel_down_sample`` is torch on the device (``voxel_down_sample``).
"""
import math

import numpy as np
import torch

from . import _inputs, _lib, parametric_edges

MAX_POLYLINE_POINTS = _lib.FIT_MAX_POLYLINE_POINTS     # csrc/fitting.hip: FIT_MAX_PTS - 8 scene units of edge at res 256
MAX_LINES = _lib.FIT_MAX_LINES
MAX_MERGE = 65536                                      # csrc/fitting.hip: MERGE_MAX
LINK_THREADS = 64                                      # csrc/fitting.hip: LINK_THREADS
LINK_MAX_CELLS = 1 << 21                               # cap of the dense cell table (8 MiB of int32); the cell edge doubles until it fits
LINK_CELL_SLACK = 1.0 + 2.0 ** -20                     # cell edge = thr * slack: rounding of (p - lo) / edge cannot separate two points closer than thr by two cells


def _finite(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(float(v))


# ---------------------------------------------------------------------------------------------------------------- voxel down-sample
def voxel_down_sample(points, colors, voxel_size):
    """One point per occupied voxel: the mean of the voxel's points AND colours, as ``pcd.voxel_down_sample(voxel_size)`` in ``edge_fit``.
    The voxel index is ``floor((p - (min_bound - voxel_size / 2)) / voxel_size)`` with ``min_bound`` the points' own minimum - open3d's
    documented rule; the output is ordered by index, first axis slowest.  Tensors (n, 3) in, tensors on the same device out (fp64); torch
    only (a stable sort, ``unique_consecutive``, differences of an fp64 cumulative sum, as ``edge_metrics.downsample_point_cloud_average``), so it runs on CPU
    and GPU tensors, deterministically.

    open3d's OUTPUT ORDER is unspecified (a hash map's), and open3d is not available to this project, so its result could not be compared;
    ``connect_points`` depends on the order through its seed rule, so the polylines of a cloud are those of THIS order."""
    if not (_finite(voxel_size) and voxel_size > 0):
        raise ValueError(f"voxel_down_sample: voxel_size must be finite and > 0 (got {voxel_size!r})")
    p, c = points.detach().to(torch.float64).reshape(-1, 3), colors.detach().to(torch.float64).reshape(-1, 3)
    if p.shape[0] != c.shape[0]:
        raise ValueError(f"voxel_down_sample: {p.shape[0]} points, {c.shape[0]} colours")
    if p.shape[0] == 0:
        return p, c
    lo = p.min(dim=0).values - voxel_size / 2
    key3 = torch.floor((p - lo) / voxel_size).to(torch.int64)
    dims = key3.max(dim=0).values + 1
    key = (key3[:, 0] * dims[1] + key3[:, 1]) * dims[2] + key3[:, 2]
    key, order = torch.sort(key, stable=True)
    _, counts = torch.unique_consecutive(key, return_counts=True)
    both = torch.cat([p, c], dim=1)[order]
    csum = torch.cat([both.new_zeros(1, 6), torch.cumsum(both, dim=0)])
    ends = torch.cumsum(counts, dim=0)
    mean = (csum[ends] - csum[ends - counts]) / counts.unsqueeze(1).to(torch.float64)
    return mean[:, :3].contiguous(), mean[:, 3:].contiguous()


def line_directions(colors):
    """``colour * 2 - 1`` divided by ``(norm + 1e-6)``: the line direction ``edge_fit`` recovers from the colours."""
    d = colors.to(torch.float64) * 2 - 1
    return d / (torch.linalg.norm(d, dim=1, keepdim=True) + 1e-6)


# ---------------------------------------------------------------------------------------------------------------- linking
def _check_link_args(distance_threshold, angle_threshold, nms_factor):
    if not (_finite(distance_threshold) and distance_threshold > 0):
        raise ValueError(f"connect_points: distance_threshold must be finite and > 0 (got {distance_threshold!r})")
    if not _finite(angle_threshold) or not _finite(nms_factor):
        raise ValueError(f"connect_points: angle_threshold and nms_factor must be finite (got {angle_threshold!r}, {nms_factor!r})")


def link_grid(xyz, thr, cell_scale=1.0):
    """The uniform grid ``emap_fit_link`` walks: ``(cell_xyz (n, 3) int32, cell_start (cells + 1) int32, order (n) int32, (gx, gy, gz))`` for
    the positions ``xyz`` (n, 3) fp64 on the device.  The cell edge is ``thr * LINK_CELL_SLACK * cell_scale`` (``cell_scale >= 1``), doubled
    until the dense table has at most ``LINK_MAX_CELLS`` cells; a non-finite extent gives one cell.  Torch on the device of ``xyz``; one
    host synchronisation (the grid's dimensions)."""
    if not cell_scale >= 1.0:
        raise ValueError(f"link_grid: cell_scale must be >= 1 (got {cell_scale!r})")
    n = int(xyz.shape[0])
    dev = xyz.device
    if n == 0:
        return (torch.zeros(0, 3, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev),
                torch.zeros(0, dtype=torch.int32, device=dev), (1, 1, 1))
    lo, hi = xyz.min(dim=0).values, xyz.max(dim=0).values
    ext = (hi - lo).tolist()                                           # the synchronisation
    edge = float(thr) * LINK_CELL_SLACK * float(cell_scale)
    if not all(math.isfinite(e) for e in ext) or not math.isfinite(edge):
        dims = (1, 1, 1)
    else:
        for _ in range(64):
            dims = tuple(int(math.floor(e / edge)) + 1 for e in ext)
            if dims[0] * dims[1] * dims[2] <= LINK_MAX_CELLS:
                break
            edge *= 2.0
        else:
            dims = (1, 1, 1)
    q = torch.floor((xyz - lo) / edge)
    q = torch.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0)
    top = torch.tensor([d - 1 for d in dims], dtype=torch.float64, device=dev)
    cell = torch.minimum(torch.clamp(q, min=0.0), top).to(torch.int64)
    key = (cell[:, 0] * dims[1] + cell[:, 1]) * dims[2] + cell[:, 2]
    _, order = torch.sort(key, stable=True)
    counts = torch.bincount(key, minlength=dims[0] * dims[1] * dims[2])
    start = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=start[1:])
    return cell.to(torch.int32).contiguous(), start.to(torch.int32).contiguous(), order.to(torch.int32).contiguous(), dims


def link(points, distance_threshold, angle_threshold, nms_factor, keep_short_lines, device="cuda", vis_global=False, cell_scale=1.0,
         return_stats=False):
    """``emap_fit_link`` on points (n, 6): ``(chain int32, offsets int32, n_polylines)`` with chain and offsets on the device - polyline k
    is ``chain[offsets[k]:offsets[k + 1]]``.  ``vis_global`` and ``cell_scale`` change where the visited bits live and how coarse the grid
    is, never the result.  ``return_stats`` adds a dict with the numbers of steps and seeds of the walk."""
    _check_link_args(distance_threshold, angle_threshold, nms_factor)
    pts = _inputs.to_device(points, device).reshape(-1, 6)
    _lib.require_cuda(pts, "points")
    n, dev = int(pts.shape[0]), pts.device
    cell_xyz, cell_start, order, dims = link_grid(pts[:, :3], distance_threshold, cell_scale)
    chain = torch.empty(3 * n, dtype=torch.int32, device=dev)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
    count = torch.empty(4, dtype=torch.int32, device=dev)
    use_global = bool(vis_global) or n > _lib.FIT_LINK_LDS_POINTS
    vis = torch.empty((n + 31) // 32, dtype=torch.int32, device=dev) if use_global else None
    with _lib.on_device(pts):
        _lib.fit_api().fit_link(pts, n, cell_xyz, cell_start, order, dims[0], dims[1], dims[2], float(distance_threshold), float(angle_threshold),
                                float(nms_factor), int(bool(keep_short_lines)), int(use_global), chain, offsets, count, vis, _lib.stream_ptr(dev))
    k, overflow, steps, seeds = count.tolist()
    if overflow:
        raise RuntimeError("connect_points: the chain buffer overflowed (3 n entries): this cannot happen")
    if return_stats:
        return chain, offsets[:k + 1], int(k), {"steps": int(steps), "seeds": int(seeds)}
    return chain, offsets[:k + 1], int(k)


def connect_points(points, distance_threshold, angle_threshold, nms_factor, keep_short_lines, device="cuda"):
    """Mirror of ``connect_points`` (edge_fitting/main.py:93-228): greedy linking of points (n, 6) - position and line direction - into
    polylines, one launch.  -> a list of lists of point indices.  The seed of a polyline is the lowest unvisited index and ties go to the
    lowest index (module docstring); the terminal point of a direction that fails the 0.5 test stays unvisited, as in the reference."""
    chain, offsets, k = link(points, distance_threshold, angle_threshold, nms_factor, keep_short_lines, device)
    off = offsets.tolist()
    flat = chain[:off[-1]].tolist()
    return [flat[off[i]:off[i + 1]] for i in range(k)]


# ---------------------------------------------------------------------------------------------------------------- lines and curves
def split_into_monotonic_sublists(numbers, max_longsublists=2, min_length=4):
    """Mirror of ``split_into_monotonic_sublists`` (line_fit.py:4-49): runs of consecutive numbers; the ``max_longsublists`` longest with at
    least ``min_length`` members are curve candidates, the others split into consecutive pairs.  Sublists of equal length are ordered by
    their first index (the reference: the order of a set).  -> ``(curve_sublists, line_pairs)``; ``[]`` for no numbers, as the reference."""
    if not numbers:
        return []
    runs, cur = [], [numbers[0]]
    for v in numbers[1:]:
        if v == cur[-1] + 1:
            cur.append(v)
        else:
            if len(cur) > 1:
                runs.append(cur)
            cur = [v]
    if len(cur) > 1:
        runs.append(cur)
    runs = sorted(runs, key=lambda r: (-len(r), r[0]))
    k = min(max_longsublists, len(runs))
    long_runs, short_runs = runs[:k], runs[k:]
    curves = []
    for r in long_runs:
        if len(r) < min_length:
            short_runs.append(r)
        else:
            curves.append(list(r))
    return curves, [[r[j], r[j + 1]] for r in short_runs for j in range(len(r) - 1)]


def _ragged(arrays, device):
    """list of (k, 3) arrays -> (points (sum k, 3) fp64 on the device, offsets (len + 1) int32 on the device)"""
    off = np.zeros(len(arrays) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    if off[-1] >= 2 ** 31:
        raise ValueError("edge_fitting: more than 2^31 - 1 points in one call")
    flat = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in arrays]) if len(arrays) else np.zeros((0, 3))
    return torch.as_tensor(np.ascontiguousarray(flat)).to(device), torch.as_tensor(off.astype(np.int32)).to(device)


def fit_lines(polylines, inlier_threshold, min_inliers, max_lines, device="cuda"):
    """``emap_fit_lines`` over a list of polylines (each (n, 3)): ``(segments (P, max_lines, 6), n_lines (P), labels list of (n) int32)``
    as numpy.  ``ValueError`` before any launch for a polyline of more than ``MAX_POLYLINE_POINTS`` points."""
    if not (_finite(inlier_threshold) and inlier_threshold > 0):
        raise ValueError(f"fit_lines: inlier_threshold must be finite and > 0 (got {inlier_threshold!r})")
    if int(min_inliers) < 2:
        raise ValueError(f"fit_lines: min_inliers must be >= 2 (got {min_inliers!r})")
    if not 1 <= int(max_lines) <= MAX_LINES:
        raise ValueError(f"fit_lines: max_lines must be in 1..{MAX_LINES} (got {max_lines!r})")
    polylines = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in polylines]
    longest = max((len(p) for p in polylines), default=0)
    if longest > MAX_POLYLINE_POINTS:
        raise ValueError(f"fit_lines: a polyline has {longest} points, at most {MAX_POLYLINE_POINTS} are fitted (they sit in LDS)")
    P = len(polylines)
    if P == 0:
        return np.zeros((0, int(max_lines), 6)), np.zeros(0, np.int32), []
    pts, off = _ragged(polylines, device)
    _lib.require_cuda(pts, "polylines")
    segs = torch.empty(P, int(max_lines), 6, dtype=torch.float64, device=pts.device)
    n_lines = torch.empty(P, dtype=torch.int32, device=pts.device)
    labels = torch.empty(max(int(pts.shape[0]), 1), dtype=torch.int32, device=pts.device)
    with _lib.on_device(pts):
        _lib.fit_api().fit_lines(pts, off, P, float(inlier_threshold), int(min_inliers), int(max_lines), segs, n_lines, labels, _lib.stream_ptr(pts.device))
    lab, o = labels.cpu().numpy(), off.cpu().numpy()
    return segs.cpu().numpy(), n_lines.cpu().numpy(), [lab[o[i]:o[i + 1]] for i in range(P)]


def fit_beziers(candidates, device="cuda"):
    """``emap_fit_beziers`` over a list of point runs (each (n, 3), n >= 4): ``(ctrl (Q, 12), rmse (Q))`` as numpy."""
    candidates = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in candidates]
    if any(len(c) < 4 for c in candidates):
        raise ValueError("fit_beziers: a cubic needs at least 4 points")
    Q = len(candidates)
    if Q == 0:
        return np.zeros((0, 12)), np.zeros(0)
    pts, off = _ragged(candidates, device)
    _lib.require_cuda(pts, "candidates")
    ctrl = torch.empty(Q, 12, dtype=torch.float64, device=pts.device)
    rmse = torch.empty(Q, dtype=torch.float64, device=pts.device)
    with _lib.on_device(pts):
        _lib.fit_api().fit_beziers(pts, off, Q, ctrl, rmse, _lib.stream_ptr(pts.device))
    return ctrl.cpu().numpy(), rmse.cpu().numpy()


_BEZIER_W = np.array([[-1, 3, -3, 1], [3, -6, 3, 0], [-3, 3, 0, 0], [1, 0, 0, 0]], dtype=np.float64)


def bezier_curve(tt, *p):
    """The reference's ``bezier_curve`` (bezier_fit.py:5-17): points of the cubic with the 12 parameters ``p`` at ``tt``, flattened."""
    tt = np.asarray(tt, dtype=np.float64)
    T = np.stack([tt ** 3, tt ** 2, tt, np.ones_like(tt)], axis=1)
    return np.dot(np.dot(T, _BEZIER_W), np.asarray(p, dtype=np.float64).reshape(4, 3)).reshape(-1)


def edge_fitting(polylines_wld, voxel_size=256, max_iterations=100, min_inliers=4, max_lines=3, max_curves=2, keep_short_lines=True,
                 device="cuda"):
    """Mirror of ``edge_fitting`` (edge_fitting/main.py:231-301) over a list of polylines (each (n, >= 3): positions first): lines by the
    exhaustive consensus fit (all polylines in one launch), the runs of points it leaves as cubic Beziers (all candidates in one launch; a
    candidate with ``rmse > 5 / voxel_size`` is dropped), short runs and - with ``keep_short_lines`` - polylines of fewer than 4 points as
    consecutive segments.  -> the reference's 5-tuple ``(straight_lines (L, 6), raw_points_on_straight_lines, bezier_curve_params (C, 12),
    bezier_curve_points (100 C, 3), raw_points_on_curves)``, empty lists where the reference returns them.

    This is the reference's RANSAC as ``max_iterations -> infinity``, not its 100 seeded draws (module docstring); ``max_iterations`` is
    accepted and unused.  A polyline of more than ``MAX_POLYLINE_POINTS`` points raises ``ValueError`` before any launch."""
    if not (_finite(voxel_size) and voxel_size > 0):
        raise ValueError(f"edge_fitting: voxel_size must be finite and > 0 (got {voxel_size!r})")
    if int(max_curves) < 0:
        raise ValueError(f"edge_fitting: max_curves must be >= 0 (got {max_curves!r})")
    polys = [np.asarray(p.detach().cpu() if isinstance(p, torch.Tensor) else p, dtype=np.float64) for p in polylines_wld]
    polys = [p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)[:, :3] for p in polys]
    fitted_idx = [k for k, p in enumerate(polys) if not (len(p) < 4 and keep_short_lines)]
    segs, n_lines, labels = fit_lines([polys[k] for k in fitted_idx], 1.0 / voxel_size, min_inliers, max_lines, device)      # checks first
    per_poly, candidates = {}, []
    for slot, k in enumerate(fitted_idx):
        remaining = np.nonzero(labels[slot] < 0)[0].tolist()
        curve_idx, pair_idx = split_into_monotonic_sublists(remaining, max_curves) if remaining else ([], [])
        per_poly[k] = (slot, pair_idx, [len(candidates) + i for i in range(len(curve_idx))])
        candidates.extend(polys[k][c] for c in curve_idx)
    ctrl, rmse = fit_beziers(candidates, device)
    straight_lines, raw_lines, curve_params, curve_points, raw_curves = [], [], [], [], []
    t_fit = np.linspace(0, 1, 100)
    for k, xyz in enumerate(polys):
        if k not in per_poly:
            for i in range(len(xyz) - 1):
                straight_lines.append(np.concatenate([xyz[i], xyz[i + 1]]))
                raw_lines.append(xyz[i:i + 2].tolist())
            continue
        slot, pair_idx, cand = per_poly[k]
        for j in range(int(n_lines[slot])):
            straight_lines.append(segs[slot, j])
            raw_lines.append(xyz[labels[slot] == j].tolist())
        if keep_short_lines:
            for a, b in pair_idx:
                straight_lines.append(np.concatenate([xyz[a], xyz[b]]))
                raw_lines.append(xyz[[a, b]].tolist())
        for c in cand:
            if not rmse[c] <= 5.0 / voxel_size:
                continue
            curve_params.append(ctrl[c])
            curve_points.append(bezier_curve(t_fit, *ctrl[c]).reshape(-1, 3))
            raw_curves.append(candidates[c].tolist())
    straight_lines = np.array(straight_lines)
    if curve_points:
        curve_points, curve_params = np.concatenate(curve_points, axis=0), np.array(curve_params)
    return straight_lines, raw_lines, curve_params, curve_points, raw_curves


def edge_fit(edge_data=None, angle_threshold=0.03, nms_factor=0.9, fit_distance_threshold=10.0, min_inliers=4, max_lines=4, max_curves=3,
             keep_short_lines=True, device="cuda"):
    """Mirror of ``edge_fit`` (edge_fitting/main.py:304-373): ``edge_data`` holds ``resolution``, ``points`` (n, 3) and ``ld_colors`` (n, 3)
    (lists, numpy, or tensors - tensors are used where they are).  Voxel down-sample at ``2 / resolution`` (``voxel_down_sample``),
    recover the line directions, link (``emap_fit_link``), fit (``edge_fitting``).  -> the reference's ``fitted_edge_dict``."""
    if edge_data is None:
        raise ValueError("edge_fit: edge_data is required")
    res = float(np.asarray(edge_data["resolution"]))
    if not (math.isfinite(res) and res > 0):
        raise ValueError(f"edge_fit: resolution must be finite and > 0 (got {res!r})")
    _check_link_args(fit_distance_threshold / res, angle_threshold, nms_factor)
    pts, col = _inputs.to_device(edge_data["points"], device).reshape(-1, 3), _inputs.to_device(edge_data["ld_colors"], device).reshape(-1, 3)
    if pts.shape[0] != col.shape[0]:
        raise ValueError(f"edge_fit: {pts.shape[0]} points, {col.shape[0]} ld_colors")
    _lib.require_cuda(pts, "points")
    pts, col = voxel_down_sample(pts, col.to(pts.device), 2.0 / res)
    points_wld = torch.cat([pts, line_directions(col)], dim=1).contiguous()
    chain, offsets, k = link(points_wld, fit_distance_threshold / res, angle_threshold, nms_factor, keep_short_lines, device)
    off = offsets.tolist()
    gathered = points_wld[chain[:off[-1]].long()].cpu().numpy()
    polylines_wld = [gathered[off[i]:off[i + 1]] for i in range(k)]
    lines, raw_lines, curves, _, raw_curves = edge_fitting(polylines_wld, voxel_size=res, max_iterations=100, min_inliers=min_inliers,
                                                           max_lines=max_lines, max_curves=max_curves, keep_short_lines=keep_short_lines,
                                                           device=pts.device)
    return {"resolution": int(res),
            "lines_end_pts": lines.tolist() if len(lines) > 0 else [],
            "raw_points_on_lines": raw_lines if len(raw_lines) > 0 else [],
            "curves_ctl_pts": curves.tolist() if len(curves) > 0 else [],
            "raw_points_on_curves": raw_curves if len(raw_curves) > 0 else []}


# ---------------------------------------------------------------------------------------------------------------- merging
def _merge_workspace(n, device):
    return torch.empty(max(n * ((n + 31) // 32), 1), dtype=torch.int32, device=device)


def merge_line_segments(line_segments, raw_points_on_lines, distance_threshold, similarity_threshold, device="cuda", return_labels=False):
    """Mirror of ``merge_line_segments`` (merging/main.py:120-156) through ``emap_fit_merge_lines``: lines (L, 6) whose one-sided distance
    is ``<= distance_threshold`` and whose SIGNED cosine is ``>= similarity_threshold`` are adjacent; a component of more than one line
    is refitted from the union of its lines' raw points.  -> merged lines (L', 6) in ascending smallest member index, numpy."""
    if isinstance(distance_threshold, float) and math.isnan(distance_threshold) or isinstance(similarity_threshold, float) and math.isnan(similarity_threshold):
        raise ValueError("merge_line_segments: the thresholds must not be NaN")
    lines = np.asarray(line_segments, dtype=np.float64).reshape(-1, 6)
    L = len(lines)
    if L > MAX_MERGE:
        raise ValueError(f"merge_line_segments: {L} lines, at most {MAX_MERGE} are merged in one call")
    if len(raw_points_on_lines) != L:
        raise ValueError(f"merge_line_segments: {L} lines, {len(raw_points_on_lines)} sets of raw points")
    if L == 0:
        return (lines, np.zeros(0, np.int32)) if return_labels else lines
    raw, raw_off = _ragged(list(raw_points_on_lines), device)
    _lib.require_cuda(raw, "line_segments")
    dev = raw.device
    lines_t = torch.as_tensor(lines).to(dev)
    labels = torch.empty(L, dtype=torch.int32, device=dev)
    merged = torch.empty(L, 6, dtype=torch.float64, device=dev)
    ws = _merge_workspace(L, dev)
    with _lib.on_device(raw):
        _lib.fit_api().fit_merge_lines(lines_t, L, raw, raw_off, float(distance_threshold), float(similarity_threshold), labels, merged, ws,
                                       ws.numel() * 4, _lib.stream_ptr(dev))
    lab = labels.cpu().numpy()
    out = merged.cpu().numpy()[lab == np.arange(L)]
    return (out, lab) if return_labels else out


def merge_endpoints(merged_line_segments, merged_bezier_curves, distance_threshold, device="cuda", return_labels=False):
    """Mirror of ``merge_endpoints`` (merging/main.py:222-268) through ``emap_fit_merge_endpoints``: the 2 L line end points, then the 2 C
    curve end points; those within ``distance_threshold`` of each other form components, every member of a component of more than one is
    replaced by the component's mean; the inner control points of curves are untouched.  -> ``(lines (L, 6), curves (C, 12))`` as numpy,
    ``[]`` in place of an empty one, as the reference."""
    if isinstance(distance_threshold, float) and math.isnan(distance_threshold):
        raise ValueError("merge_endpoints: distance_threshold must not be NaN")
    lines = np.asarray(merged_line_segments, dtype=np.float64).reshape(-1, 6)
    curves = np.asarray(merged_bezier_curves, dtype=np.float64).reshape(-1, 12)
    L, Cn = len(lines), len(curves)
    E = 2 * L + 2 * Cn
    if E > MAX_MERGE:
        raise ValueError(f"merge_endpoints: {E} end points, at most {MAX_MERGE} are merged in one call")
    if E == 0:
        return ([], [], np.zeros(0, np.int32)) if return_labels else ([], [])
    ends = np.concatenate([lines.reshape(-1, 3), curves[:, [0, 1, 2, 9, 10, 11]].reshape(-1, 3)])
    ends_t = torch.as_tensor(np.ascontiguousarray(ends)).to(device)
    _lib.require_cuda(ends_t, "merged_line_segments")
    dev = ends_t.device
    labels = torch.empty(E, dtype=torch.int32, device=dev)
    merged = torch.empty(E, 3, dtype=torch.float64, device=dev)
    ws = _merge_workspace(E, dev)
    with _lib.on_device(ends_t):
        _lib.fit_api().fit_merge_endpoints(ends_t, E, float(distance_threshold), labels, merged, ws, ws.numel() * 4, _lib.stream_ptr(dev))
    m = merged.cpu().numpy()
    out_lines = m[:2 * L].reshape(-1, 6) if L > 0 else []
    out_curves = []
    if Cn > 0:
        out_curves = curves.copy()
        ce = m[2 * L:].reshape(-1, 6)
        out_curves[:, :3], out_curves[:, 9:] = ce[:, :3], ce[:, 3:]
    return (out_lines, out_curves, labels.cpu().numpy()) if return_labels else (out_lines, out_curves)


def merge(out_dir, fitted_edge_dict, merge_edge_distance_threshold=5.0, merge_endpoints_distance_threshold=1.0, merge_similarity_threshold=0.98,
          merge_endpoints_flag=True, merge_edge_flag=True, merge_curve_flag=False, save_ply=False, device="cuda"):
    """Mirror of ``merge`` (merging/main.py:295-385): lines are merged (``merge_line_segments`` at half the edge threshold), then the end
    points of lines and curves (``merge_endpoints``); both thresholds are divided by the dict's ``resolution``.  ``merge_curve_flag=True``
    (nothing in the reference sets it) and ``save_ply=True`` (open3d file output) raise ``NotImplementedError``; ``out_dir`` is unused
    without them.  -> ``{"lines_end_pts": ..., "curves_ctl_pts": ...}`` as lists."""
    if merge_curve_flag:
        raise NotImplementedError("merge: merge_curve_flag=True (merge_bezier_curves) is not implemented; nothing in the reference sets it")
    if save_ply:
        raise NotImplementedError("merge: save_ply=True writes .ply files through open3d, which this project does not have")
    resolution = int(fitted_edge_dict["resolution"])
    if resolution <= 0:
        raise ValueError(f"merge: resolution must be > 0 (got {resolution})")
    lines = np.array(fitted_edge_dict["lines_end_pts"], dtype=np.float64).reshape(-1, 6)
    curves = np.array(fitted_edge_dict["curves_ctl_pts"], dtype=np.float64).reshape(-1, 12)
    edge_thr = merge_edge_distance_threshold / resolution
    end_thr = merge_endpoints_distance_threshold / resolution
    if merge_edge_flag and len(lines) > 0:
        lines = merge_line_segments(lines, fitted_edge_dict["raw_points_on_lines"], edge_thr / 2.0, merge_similarity_threshold, device)
    if merge_endpoints_flag:
        lines, curves = merge_endpoints(lines, curves, end_thr, device)
    return {"lines_end_pts": lines.tolist() if len(lines) > 0 else [],
            "curves_ctl_pts": curves.tolist() if len(curves) > 0 else []}


# ---------------------------------------------------------------------------------------------------------------- the whole step
def get_parametric_edge(edge_dict, visible_checking=False, edges=None, intrinsics_list=None, camtoworld_list=None, h=None, w=None, device="cuda"):
    """Mirror of ``get_parametric_edge`` (extract_parametric_edge.py:216-300): ``edge_fit``, ``merge`` and
    ``parametric_edges.finish_parametric_edges`` with the reference's fixed parameters (:228-237: nms 0.95, angle 0.03, fit distance 10,
    min_inliers 5, max_lines 4, max_curves 3, merge 5.0 / 2.0 / 0.98).  ``edge_dict`` is what ``get_pointcloud_from_udf`` returns
    (``resolution``, ``points``, ``ld_colors``).  The maps and cameras the reference reads with ``get_edge_maps`` are arguments, as in
    ``finish_parametric_edges``.  -> ``(pred_points float32 numpy, return_edge_dict)``."""
    if visible_checking and (edges is None or intrinsics_list is None or camtoworld_list is None or h is None or w is None):
        raise ValueError("get_parametric_edge: visible_checking needs edges, intrinsics_list, camtoworld_list, h and w")
    fitted_edge_dict = edge_fit(edge_data=edge_dict, angle_threshold=0.03, nms_factor=0.95, fit_distance_threshold=10.0, min_inliers=5, max_lines=4,
                                max_curves=3, device=device)
    merged_edge_dict = merge(edge_dict.get("result_dir") if hasattr(edge_dict, "get") else None, fitted_edge_dict,
                             merge_edge_distance_threshold=5.0, merge_endpoints_distance_threshold=2.0, merge_similarity_threshold=0.98, device=device)
    return parametric_edges.finish_parametric_edges(merged_edge_dict, visible_checking, edges, intrinsics_list, camtoworld_list, h, w, device=device)
