"""CPU yardsticks of the edge-metric tests (tests/test_edge_metrics_cpu.py, tests/test_gpu_edge_metrics.py): restatements in plain
numpy of the search contract of csrc/metrics.hip and of the reference's evaluation (src/eval/eval_util.py, src/eval/eval_ABC.py).
Nothing here imports the package under test."""
import numpy as np


def nn_ref(q, r, chunk=512):
    """The contract of emap_nearest_neighbors in numpy fp32: d2 = (dx*dx + dy*dy) + dz*dz with every operation rounded to fp32,
    np.argmin (first occurrence = lowest index among equal d2, NaN rows of r skipped), np.sqrt.  A query whose every d2 is NaN gets
    idx -1 and NaN.  -> (d2 (n_q) fp32, dist (n_q) fp32, idx (n_q) int64)."""
    q, r = np.ascontiguousarray(q, dtype=np.float32), np.ascontiguousarray(r, dtype=np.float32)
    d2o, idx = np.empty(len(q), np.float32), np.empty(len(q), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(0, len(q), chunk):
            c = q[h:h + chunk]
            dx = c[:, None, 0] - r[None, :, 0]
            dy = c[:, None, 1] - r[None, :, 1]
            dz = c[:, None, 2] - r[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            nan = np.isnan(d2)
            key = np.where(nan, np.float32(np.inf), d2)
            i = np.argmin(key, axis=1)                   # first occurrence
            # +inf is a legal minimum, a NaN is not: where the winner is a NaN slot, take the first non-NaN one (all of them are +inf)
            rows = np.arange(len(c))
            bad = nan[rows, i]
            first_ok = np.argmax(~nan, axis=1)
            i = np.where(bad, first_ok, i)
            none = nan.all(axis=1)
            d2o[h:h + chunk] = np.where(none, np.float32(np.nan), d2[rows, i])
            idx[h:h + chunk] = np.where(none, -1, i)
        return d2o, np.sqrt(d2o), idx


def ulp_diff(a, b):
    """Distance in units of the last place between two fp32 arrays of non-negative finite values."""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def sample_segments_ref(segments, interval=0.005):
    """get_gt_points' per-segment loop (eval_util.py:271-278, cast of :295)."""
    pts = []
    for seg in np.asarray(segments, dtype=np.float64):
        current, nxt = seg[0], seg[1]
        num = int(np.linalg.norm(nxt - current) // interval)
        linspace = np.linspace(0, 1, num)
        pts.append(linspace[:, None] * current + (1 - linspace)[:, None] * nxt)
    return np.concatenate(pts).astype(np.float32)


def downsample_ref(points, num_voxels_per_axis=256, min_bound=None, max_bound=None):
    """A dictionary of voxels: key = floor((p - min_bound) / voxel_size) per axis with voxel_size as at eval_util.py:444-449, the mean
    of each voxel's points, ordered by key; points outside [min_bound, max_bound] are dropped."""
    p = np.asarray(points, dtype=np.float64)
    lo = p.min(axis=0) if min_bound is None else np.array(min_bound, dtype=np.float64)
    hi = p.max(axis=0) if max_bound is None else np.array(max_bound, dtype=np.float64)
    if isinstance(num_voxels_per_axis, int):
        vs = (hi - lo) / num_voxels_per_axis
    else:
        vs = np.array([(hi[i] - lo[i]) / num_voxels_per_axis[i] for i in range(3)])
    voxels = {}
    for row in p:
        if np.any(row < lo) or np.any(row > hi):
            continue
        voxels.setdefault(tuple(int(k) for k in np.floor((row - lo) / vs)), []).append(row)
    return np.array([np.mean(voxels[k], axis=0) for k in sorted(voxels)]).reshape(-1, 3)


def metrics_ref(d_pred, d_gt, thresholds):
    """chamfer_distance's tail (eval_util.py:48-53) and the "all" branch of compute_precision_recall_IOU (:153-175) from the two
    distance arrays (pred -> gt, gt -> pred)."""
    d_pred, d_gt = np.asarray(d_pred), np.asarray(d_gt)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc, comp = np.mean(d_pred), np.mean(d_gt)
        out = {"n_pred": len(d_pred), "n_gt": len(d_gt), "chamfer": comp + acc, "acc": acc, "comp": comp}
        for thresh in thresholds:
            correct_pred = np.sum(d_pred < thresh)
            precision = correct_pred / np.float64(len(d_pred))
            correct_gt = np.sum(d_gt < thresh)
            recall = correct_gt / np.float64(len(d_gt))
            out[f"precision_{thresh}"] = precision
            out[f"recall_{thresh}"] = recall
            out[f"fscore_{thresh}"] = 2 * precision * recall / (precision + recall)
            intersection = min(correct_pred, correct_gt)
            union = len(d_pred) + len(d_gt) - max(correct_pred, correct_gt)
            out[f"IOU_{thresh}"] = intersection / np.float64(union)
            out[f"correct_pred_{thresh}"], out[f"correct_gt_{thresh}"] = int(correct_pred), int(correct_gt)
    return out


def wireframe_case(seed):
    """The end-to-end case: gt = the sampled wire frame, pred = 3000 of its points + N(0, 0.006), every tenth displaced by N(0, 0.05).
    Draw order of default_rng(seed): integers, normal (3000, 3), normal (300, 3)."""
    from emap_amd.synthetic import wireframe_segments
    gt = sample_segments_ref(wireframe_segments())
    rng = np.random.default_rng(seed)
    pick = rng.integers(len(gt), size=3000)
    pred = gt[pick].astype(np.float64) + rng.normal(0, 0.006, (3000, 3))
    pred[::10] += rng.normal(0, 0.05, (300, 3))
    return pred.astype(np.float32), gt


def kdtree_distances(a, b):
    """fp64 nearest-neighbour distances a -> b with scipy's cKDTree (stands in for point_cloud_utils' tree)."""
    from scipy.spatial import cKDTree
    return cKDTree(np.asarray(b, np.float64)).query(np.asarray(a, np.float64), k=1)[0]
