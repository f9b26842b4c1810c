"""Edge metrics on the device: how good an extracted edge point cloud is against a ground truth.

Mirrors of the reference's evaluation (src/eval/eval_util.py): ``chamfer_distance`` (:20-58), ``compute_chamfer_distance`` (:61-73),
``f_score`` (:76-87), ``compute_precision_recall_IOU`` (:138-191), ``downsample_point_cloud_average`` (:418-456) and the per-segment
sampling of ``get_gt_points`` (:271-278), plus ``evaluate_edges``: the ``process_scan`` sequence of src/eval/eval_ABC.py:63-89.  The
reference rests on ``point_cloud_utils``' k-d tree on the CPU; here the exact 1-nearest-neighbour search is a brute-force HIP kernel
(``emap_nearest_neighbors``, csrc/metrics.hip) and the sums and threshold counts one more launch (``emap_dist_stats``).  The search is a
pure function of its inputs: d2 = (dx*dx + dy*dy) + dz*dz in fp32 without FMA contraction, the lowest index among equal d2 - a k-d
tree breaks ties arbitrarily, this does not.  Distances are fp32 (2e-7 relative of an fp64 tree's); thresholds are compared in fp32.

Arguments may be numpy arrays, as the reference passes them: they are moved to ``device``.  Tensors are used where they are.
There is no CPU fallback for the search; ``metrics_from_stats``, ``f_score``, ``sample_segments`` and
``downsample_point_cloud_average`` (torch, any device) need no GPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _inputs, _lib

NN_Q_TILE = 1024        # queries per workgroup of the search kernel (csrc/metrics.hip: NN_Q_TILE)
NN_R_TILE = 1024        # references per LDS tile                     (csrc/metrics.hip: NN_R_TILE)
MAX_THRESHOLDS = 8      # thresholds per emap_dist_stats launch


def nearest_neighbors(a, b, split=0, device="cuda"):
    """For every row of ``a`` (n_a, 3) its nearest row of ``b`` (n_b, 3): ``(dist (n_a) fp32, idx (n_a) int64)`` on the device, the
    plain distance as ``pcu.k_nearest_neighbors(a, b, k=1, squared_distances=False)``.  Bit-exact and deterministic (module docstring);
    ``split`` forces the number of splits of ``b`` over workgroups (0: automatic) and never changes the result.  A row of ``a`` with a
    NaN gets idx -1 and dist NaN."""
    a, b = _inputs.points(a, device, "edge_metrics"), _inputs.points(b, device, "edge_metrics")
    _lib.require_cuda(a, "a")
    _lib.require_cuda(b, "b")
    if b.device != a.device:
        raise ValueError(f"nearest_neighbors: a is on {a.device}, b on {b.device}")
    n_a, n_b = int(a.shape[0]), int(b.shape[0])
    dist = torch.empty(n_a, device=a.device, dtype=torch.float32)
    idx = torch.empty(n_a, device=a.device, dtype=torch.int64)
    nb = _lib.size_of("nn_workspace_bytes", n_a)
    ws = torch.empty(max(nb, 8) // 8, device=a.device, dtype=torch.int64)       # per call: this is not a graph path
    with _lib.on_device(a):
        _lib.api().nearest_neighbors(a, n_a, b, n_b, int(split), dist, idx, ws, ws.numel() * 8, _lib.stream_ptr(a.device))
    return dist, idx


def _stats_into(dist, thresholds, out):
    """Enqueue emap_dist_stats: out (1 + len(thresholds)) fp64 on the device <- [sum, count(dist < thr) ...]."""
    thr = (C.c_float * max(len(thresholds), 1))(*[float(t) for t in thresholds])
    with _lib.on_device(dist):
        _lib.api().dist_stats(dist, int(dist.shape[0]), thr, len(thresholds), out, _lib.stream_ptr(dist.device))


def dist_stats(dist, thresholds=()):
    """``[sum(dist) in fp64, count(dist < float32(thr)) for thr in thresholds]`` as a device tensor of 1 + len(thresholds) doubles
    (at most 8 thresholds).  A NaN distance is never counted and makes the sum NaN.  The same bits on every run."""
    _lib.require_cuda(dist, "dist")
    dist = _lib.f32c(dist).reshape(-1)
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f"dist_stats: at most {MAX_THRESHOLDS} thresholds per call (got {len(thresholds)})")
    out = torch.empty(1 + len(thresholds), device=dist.device, dtype=torch.float64)
    _stats_into(dist, thresholds, out)
    return out


def _both_ways(pred, gt, thresholds, device):
    """The two searches and their statistics: (stats (2, 1 + n_thr) on the HOST - row 0 pred -> gt, row 1 gt -> pred -, idx pred -> gt,
    idx gt -> pred).  One search per direction whatever the number of thresholds; one device-to-host copy."""
    pred, gt = _inputs.points(pred, device, "edge_metrics"), _inputs.points(gt, device, "edge_metrics")
    thresholds = list(thresholds)
    d_pg, i_pg = nearest_neighbors(pred, gt)
    d_gp, i_gp = nearest_neighbors(gt, pred)
    stats = torch.empty(2, 1 + len(thresholds), device=pred.device, dtype=torch.float64)
    if len(thresholds) <= MAX_THRESHOLDS:
        _stats_into(d_pg, thresholds, stats[0])
        _stats_into(d_gp, thresholds, stats[1])
    else:                                   # more thresholds than one launch takes: groups of 8, the sum from the first
        for h in range(0, len(thresholds), MAX_THRESHOLDS):
            part = thresholds[h:h + MAX_THRESHOLDS]
            rows = torch.empty(2, 1 + len(part), device=pred.device, dtype=torch.float64)
            _stats_into(d_pg, part, rows[0])
            _stats_into(d_gp, part, rows[1])
            stats[:, 1 + h:1 + h + len(part)] = rows[:, 1:]
            if h == 0:
                stats[:, 0] = rows[:, 0]
    return stats.cpu().numpy(), i_pg, i_gp


def f_score(precision, recall):
    """eval_util.py:76-87."""
    return 2 * precision * recall / (precision + recall)


def chamfer_distance(x, y, return_index=False, p_norm=2, max_points_per_leaf=10, device="cuda"):
    """Mirror of ``chamfer_distance`` (eval_util.py:20-58): ``(cham_dist, Acc, Comp)``, or with ``return_index`` ``(cham_dist,
    corrs_x_to_y, corrs_y_to_x)`` (numpy int64).  In the reference's naming ``Comp`` is the mean distance from each ``y`` to its
    neighbour in ``x`` and ``Acc`` from each ``x`` to its neighbour in ``y`` (:48-52).  Only ``p_norm=2``; ``max_points_per_leaf``
    is accepted and unused (there is no tree)."""
    if p_norm != 2:
        raise NotImplementedError(f"chamfer_distance: p_norm={p_norm!r} (only the Euclidean norm, p_norm=2)")
    stats, corrs_x_to_y, corrs_y_to_x = _both_ways(x, y, (), device)
    with np.errstate(invalid="ignore", divide="ignore"):
        Acc = stats[0, 0] / np.float64(corrs_x_to_y.shape[0])
        Comp = stats[1, 0] / np.float64(corrs_y_to_x.shape[0])
    cham_dist = Comp + Acc
    if return_index:
        return cham_dist, corrs_x_to_y.cpu().numpy(), corrs_y_to_x.cpu().numpy()
    return cham_dist, Acc, Comp


def compute_chamfer_distance(pred_sampled, gt_points):
    """eval_util.py:61-73."""
    chamfer_dist, acc, comp = chamfer_distance(pred_sampled, gt_points)
    return chamfer_dist, acc, comp


def _counts(row):
    return [np.int64(round(c)) for c in row[1:]]


def compute_precision_recall_IOU(pred_sampled, gt_points, metrics, thresh_list=[0.02], edge_type="all", device="cuda"):
    """Mirror of ``compute_precision_recall_IOU`` (eval_util.py:138-191), both branches: ``edge_type == "all"`` appends precision,
    recall, fscore and IOU per threshold to the lists of ``metrics`` and returns it; any other ``edge_type`` returns ``(correct_gt_list,
    num_gt, correct_pred_list, num_pred, acc, comp)``.  The search runs once per direction, not once per threshold; ``fscore`` and
    ``IOU`` divide as numpy does (NaN on 0/0, no exception)."""
    thresh_list = list(thresh_list)
    stats, i_pg, i_gp = _both_ways(pred_sampled, gt_points, thresh_list, device)
    num_pred, num_gt = int(i_pg.shape[0]), int(i_gp.shape[0])
    correct_pred_list, correct_gt_list = _counts(stats[0]), _counts(stats[1])
    with np.errstate(invalid="ignore", divide="ignore"):
        if edge_type == "all":
            for thresh, correct_pred, correct_gt in zip(thresh_list, correct_pred_list, correct_gt_list):
                precision = correct_pred / np.float64(num_pred)
                recall = correct_gt / np.float64(num_gt)
                metrics[f"precision_{thresh}"].append(precision)
                metrics[f"recall_{thresh}"].append(recall)
                metrics[f"fscore_{thresh}"].append(f_score(precision, recall))
                intersection = min(correct_pred, correct_gt)
                union = num_pred + num_gt - max(correct_pred, correct_gt)
                metrics[f"IOU_{thresh}"].append(intersection / np.float64(union))
            return metrics
        acc, comp = stats[0, 0] / np.float64(num_pred), stats[1, 0] / np.float64(num_gt)
    return correct_gt_list, num_gt, correct_pred_list, num_pred, acc, comp


def metrics_from_stats(n_pred, n_gt, stats_pred, stats_gt, thresholds):
    """The pure formulas, from plain numbers: ``stats_pred`` = [sum of the pred -> gt distances, count below each threshold],
    ``stats_gt`` the same for gt -> pred.  -> dict with ``chamfer`` = acc + comp, ``acc`` = mean pred -> gt, ``comp`` = mean gt ->
    pred (eval_util.py:48-53) and per threshold t ``precision_t``, ``recall_t``, ``fscore_t``, ``IOU_t`` (:157-175), plus ``n_pred`` /
    ``n_gt``.  Divisions as numpy's: 0/0 is NaN."""
    sp, sg = np.asarray(stats_pred, dtype=np.float64), np.asarray(stats_gt, dtype=np.float64)
    if sp.shape != (1 + len(thresholds),) or sg.shape != sp.shape:
        raise ValueError(f"metrics_from_stats: {len(thresholds)} thresholds need statistics rows of {1 + len(thresholds)} numbers")
    n_pred, n_gt = np.float64(n_pred), np.float64(n_gt)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc, comp = sp[0] / n_pred, sg[0] / n_gt
        out = {"n_pred": int(n_pred), "n_gt": int(n_gt), "chamfer": float(acc + comp), "acc": float(acc), "comp": float(comp)}
        for k, t in enumerate(thresholds):
            correct_pred, correct_gt = sp[1 + k], sg[1 + k]
            precision, recall = correct_pred / n_pred, correct_gt / n_gt
            union = n_pred + n_gt - max(correct_pred, correct_gt)
            out[f"precision_{t}"] = float(precision)
            out[f"recall_{t}"] = float(recall)
            out[f"fscore_{t}"] = float(f_score(precision, recall))
            out[f"IOU_{t}"] = float(min(correct_pred, correct_gt) / union)
    return out


def _downsample(points, num_voxels_per_axis, min_bound, max_bound):
    """tensor (n, 3) -> tensor (n', 3), same dtype and device: see downsample_point_cloud_average."""
    p = points.detach().to(torch.float64)
    n = [int(num_voxels_per_axis)] * 3 if isinstance(num_voxels_per_axis, int) else [int(v) for v in num_voxels_per_axis]
    if p.shape[0] == 0:
        return points[:0]
    lo = p.min(dim=0).values if min_bound is None else torch.as_tensor(np.asarray(min_bound, dtype=np.float64), device=p.device)
    hi = p.max(dim=0).values if max_bound is None else torch.as_tensor(np.asarray(max_bound, dtype=np.float64), device=p.device)
    voxel_size = (hi - lo) / torch.tensor(n, dtype=torch.float64, device=p.device)
    inside = ((p >= lo) & (p <= hi)).all(dim=1)
    p = p[inside]
    safe = torch.where(voxel_size > 0, voxel_size, torch.ones_like(voxel_size))       # a flat axis: every key 0
    key3 = torch.floor((p - lo) / safe).to(torch.int64)
    key = (key3[:, 0] * (n[1] + 1) + key3[:, 1]) * (n[2] + 1) + key3[:, 2]            # a point ON max_bound has key n on that axis
    key, order = torch.sort(key, stable=True)
    _, counts = torch.unique_consecutive(key, return_counts=True)
    csum = torch.cat([p.new_zeros(1, 3), torch.cumsum(p[order], dim=0)])
    ends = torch.cumsum(counts, dim=0)
    sums = csum[ends] - csum[ends - counts]
    return (sums / counts.unsqueeze(1).to(torch.float64)).to(points.dtype if points.dtype.is_floating_point else torch.float32)


def downsample_point_cloud_average(points, num_voxels_per_axis=256, min_bound=None, max_bound=None):
    """Mirror of ``downsample_point_cloud_average`` (eval_util.py:418-456): one point per occupied voxel, the mean of the voxel's points.
    ``voxel_size = (max_bound - min_bound) / num_voxels_per_axis`` (an int, or a 3-tuple: per axis; :444-449), the bounds default to
    the points' own extent (:433-441).  The voxel key is ``floor((p - min_bound) / voxel_size)`` per axis; the output is ordered by key
    (first axis slowest); points outside ``[min_bound, max_bound]`` are dropped.  Written in torch - a stable sort, ``unique_consecutive``,
    differences of an fp64 cumulative sum - so it runs on CPU and GPU tensors, deterministically.  A numpy array gives a numpy array, a
    tensor a tensor on its device.

    The reference delegates to ``pcu.downsample_point_cloud_on_voxel_grid`` (:452).  point_cloud_utils is not available to this project,
    so its OUTPUT ORDER and its treatment of OUT-OF-BOUNDS points could not be compared; no metric depends on the order."""
    if isinstance(points, torch.Tensor):
        return _downsample(points, num_voxels_per_axis, min_bound, max_bound)
    pts = np.asarray(points)
    return _downsample(torch.as_tensor(pts), num_voxels_per_axis, min_bound, max_bound).numpy().astype(pts.dtype if pts.dtype.kind == "f" else np.float32)


def sample_segments(segments, interval=0.005):
    """The per-segment sampling of ``get_gt_points`` (eval_util.py:271-278) for an (m, 2, 3) array of end points ``(current, next)``:
    ``num = int(|next - current| // interval)`` points ``t * current + (1 - t) * next``, ``t = linspace(0, 1, num)`` - none for a segment
    shorter than ``interval``.  -> (n, 3) float32 (:295).  ``sample_segments(synthetic.wireframe_segments())`` is the ground truth
    of the synthetic wire frame."""
    segments = np.asarray(segments, dtype=np.float64).reshape(-1, 2, 3)
    out = []
    for current, nxt in segments:
        num = int(np.linalg.norm(nxt - current) // interval)
        t = np.linspace(0, 1, num)
        out.append(t[:, None] * current + (1 - t)[:, None] * nxt)
    return (np.concatenate(out) if out else np.zeros((0, 3))).astype(np.float32)


def evaluate_edges(pred, gt, thresholds=(0.005, 0.01, 0.02), downsample=256, device="cuda"):
    """The ``process_scan`` sequence of src/eval/eval_ABC.py:63-89 on the device: down-sample ``pred`` to one point per voxel of a
    ``downsample``^3 grid on [-1, 1]^3 (None: as it is), search pred -> gt and gt -> pred, two statistics launches, ONE device-to-host
    copy of the two statistics rows, then ``metrics_from_stats``.  -> its dict (``n_pred`` counts the down-sampled points)."""
    thresholds = tuple(thresholds)
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f"evaluate_edges: at most {MAX_THRESHOLDS} thresholds (got {len(thresholds)})")
    pred, gt = _inputs.points(pred, device, "edge_metrics"), _inputs.points(gt, device, "edge_metrics")
    if downsample is not None:
        pred = _downsample(pred, downsample, [-1, -1, -1], [1, 1, 1])
    if pred.shape[0] == 0 or gt.shape[0] == 0:
        raise ValueError(f"evaluate_edges: empty point set (pred {int(pred.shape[0])} points inside [-1, 1]^3, gt {int(gt.shape[0])})")
    stats, _, _ = _both_ways(pred, gt, thresholds, device)
    return metrics_from_stats(int(pred.shape[0]), int(gt.shape[0]), stats[0], stats[1], thresholds)
