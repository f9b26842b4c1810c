"""The DTU evaluation on the device: the ground-truth edge points of a DTU scan and the precision / recall against them.

Mirrors of the reference's ``compute_visibility`` / ``project2D`` and the per-scan body of ``main`` (scripts/get_gt_points_DTU.py:94-140,
:251-288) and of ``process_scan`` (src/eval/eval_DTU.py:39-69).  The reference projects every point of the structured-light scan (10-30
million) into every edge map (49-64) through an (n, F) float64 matrix on the CPU; here that is ONE launch of ``emap_point_visibility``
(csrc/visibility.hip, include/emap_eval_hip.h): one thread per point, the frame loop inside it, an int32 count per point and nothing else.
The rest is composition of what the package has: ``edge_metrics.downsample_point_cloud_average``, ``edge_metrics.nearest_neighbors``,
``parametric_edges.sample_edges``.

Projection conventions are those of ``parametric_edges.compute_visibility`` (a different routine: the mean over a handful of control points
per fitted edge): fp64, ``K @ (R @ X + T)`` with K, R and T formed on the host (``_inputs.world_to_camera``), divided by
its third row, no depth test, pixels rounded half to even, a point valid when ``0 <= u < w`` and ``0 <= v < h`` on the rounded doubles.
The kernel takes every 3-term sum left to right without FMA contraction, so the pixel is a pure function of the inputs.

Edge maps may be bytes: ``invert=True`` evaluates ``1 - g / 255.0`` in double per pixel, bit for bit what the reference's ``get_edge_maps``
(:87-88) stores as float64.  Bytes are the recommended storage - a DTU scan's maps are 94-123 MB as bytes, which the 256 MB Infinity Cache
holds, and 0.75-1 GB as float64, which it does not - and are passed through unconverted.  float32 maps are compared as the float32 value
widened to double, which can differ from a float64 map within float32 rounding of the threshold; byte maps cannot differ.

numpy inputs go to ``device``; tensors are used where they are.  There is no CPU fallback: without a GPU the calls raise ``RuntimeError``.
"""
import os

import numpy as np
import torch

from . import _inputs, _lib, edge_metrics, parametric_edges

VIS_THREADS = 256          # csrc/visibility.hip: VIS_THREADS
VIS_CHUNK = 64             # frames whose cameras sit in LDS at a time        (csrc/visibility.hip: VIS_CHUNK)
VIS_MAX_BLOCKS = 2048      # workgroups of a launch; more than VIS_MAX_BLOCKS * VIS_THREADS points take the grid stride
POINT_DTYPES = (torch.float32, torch.float64)       # _lib.EVAL_POINTS_DTYPES: points of these stay as they are, any other becomes float64

# scan -> (edge_visibility_threshold, edge_visibility_frames_ratio): the table of scripts/get_gt_points_DTU.py:229-236
DTU_SCANS = {
    "scan37": (0.55, 0.3),
    "scan83": (0.65, 0.2),
    "scan105": (0.65, 0.2),
    "scan110": (0.5, 0.3),
    "scan118": (0.5, 0.3),
    "scan122": (0.35, 0.4),
}


def visibility_frames(edge_visibility_frames_ratio, num_frames):
    """``max(1, round(ratio * num_frames))`` with Python's ``round`` (half to even), as scripts/get_gt_points_DTU.py:264-266."""
    return max(1, round(edge_visibility_frames_ratio * num_frames))


def _maps(edge_maps, h, w, device):
    """(F, h, w) contiguous tensor of uint8 / float32 / float64: the reference's (F, h, w, 1) numpy array goes to ``device`` in its own
    dtype (any other dtype as float64), a tensor stays where it is."""
    t = _inputs.to_device(edge_maps, device, torch.float64, keep=tuple(_lib.EVAL_MAPS_DTYPES))
    return _inputs.edge_maps(t, h, w, "dtu_eval: edge_maps", nonempty=True)


def _cameras(intrinsics_list, camtoworld_list, F, device):
    """K (F, 3, 3), R (F, 3, 3), T (F, 3) fp64 on ``device`` (``_inputs.world_to_camera``, as the reference forms them per frame: :110-111,
    :133-134): three small copies."""
    if len(intrinsics_list) != F or len(camtoworld_list) != F:
        raise ValueError(f"dtu_eval: {F} edge maps, {len(intrinsics_list)} intrinsics, {len(camtoworld_list)} poses")
    return tuple(torch.as_tensor(a).to(device) for a in _inputs.world_to_camera(intrinsics_list, camtoworld_list))


def _visibility(points, edge_maps, intrinsics_list, camtoworld_list, h, w, threshold, invert, min_frames, want_mask, device):
    """The launch: -> (count (n) int32, mask (n) uint8 or None) on the device of the points."""
    pts = _inputs.points(points, device, "dtu_eval", POINT_DTYPES)
    maps = _maps(edge_maps, h, w, device)
    _lib.require_cuda(pts, "points")
    _lib.require_cuda(maps, "edge_maps")
    dev = pts.device
    if maps.device != dev:
        raise ValueError(f"dtu_eval: points are on {dev}, edge_maps on {maps.device}")
    F, n = int(maps.shape[0]), int(pts.shape[0])
    K, R, T = _cameras(intrinsics_list, camtoworld_list, F, dev)
    count = torch.empty(n, device=dev, dtype=torch.int32)
    mask = torch.empty(n, device=dev, dtype=torch.uint8) if want_mask else None
    with _lib.on_device(pts):
        _lib.eval_api().point_visibility(pts, _lib.EVAL_POINTS_DTYPES[pts.dtype], n, K, R, T, maps, _lib.EVAL_MAPS_DTYPES[maps.dtype], F,
                                         int(h), int(w), 1 if invert else 0, float(threshold), int(min_frames), count, mask,
                                         _lib.stream_ptr(dev))
    return count, mask


def point_visibility_counts(points, edge_maps, intrinsics_list, camtoworld_list, h, w, edge_visibility_threshold, invert=False, device="cuda"):
    """For each of the n points the number of frames in which it projects onto a pixel whose edge strength exceeds
    ``edge_visibility_threshold``: the row sums of the reference's ``point_visibility_matrix`` (:105-128) as an int32 (n) device tensor,
    without the matrix.  ``points`` (n, 3) fp64 or fp32; ``edge_maps`` the reference's (F, h, w, 1) float64 numpy array or an
    (F, h, w[, 1]) tensor of uint8 / float32 / float64 (``invert``: strength ``1 - g / 255`` for bytes, else ``g / 255``; float maps are
    taken as they are); ``intrinsics_list`` (F, 4, 4) or (F, 3, 3); ``camtoworld_list`` (F, 4, 4).  One launch, no synchronisation,
    the same bits on every run."""
    return _visibility(points, edge_maps, intrinsics_list, camtoworld_list, h, w, edge_visibility_threshold, invert, 0, False, device)[0]


def compute_point_visibility(gt_points, edge_maps, intrinsics_list, camtoworld_list, h, w, edge_visibility_threshold, edge_visibility_frames,
                             invert=False, device="cuda"):
    """Mirror of ``compute_visibility`` (scripts/get_gt_points_DTU.py:94-128), the reference's parameters in the reference's order: the
    bool array ``count > edge_visibility_frames`` - numpy for numpy points, a device tensor for tensor points."""
    _, mask = _visibility(gt_points, edge_maps, intrinsics_list, camtoworld_list, h, w, edge_visibility_threshold, invert,
                          edge_visibility_frames, True, device)
    mask = mask.bool()
    return mask if isinstance(gt_points, torch.Tensor) else mask.cpu().numpy()


def _affine(p, m):
    """``p @ m[:3, :3].T + m[:3, 3]`` for (n, 3) fp64 device points and a (4, 4) host matrix, every row sum left to right in separate
    elementwise operations: the same bits on every run and on every device, whatever a BLAS would do with an (n, 3) x (3, 3) product."""
    a = torch.as_tensor(np.ascontiguousarray(m[:3, :3].T)).to(p.device)          # rows of a: the coefficients of x, y, z
    t = torch.as_tensor(np.ascontiguousarray(m[:3, 3])).to(p.device)
    return ((p[:, 0:1] * a[0] + p[:, 1:2] * a[1]) + p[:, 2:3] * a[2]) + t


def gt_edge_points(gt_points, worldtogt, edge_maps, intrinsics_list, camtoworld_list, h, w, edge_visibility_threshold,
                   edge_visibility_frames_ratio, num_voxels_per_axis=256, invert=False, device="cuda"):
    """The per-scan body of ``main`` (scripts/get_gt_points_DTU.py:251-288): the scan's points ``gt_points`` (n, 3), in the ground-truth
    frame, to the scan's edge points (m, 3) in the same frame, as an fp64 device tensor.  ``gttoworld = inv(worldtogt)``, the points in
    world coordinates, their visibility in more than ``max(1, round(ratio * F))`` frames (``visibility_frames``), the selection,
    ``edge_metrics.downsample_point_cloud_average`` over the survivors' own extent, and the transform back.  No point data goes through
    the host.  The selection synchronises once, for the number of survivors; the down-sampling's own dynamic shapes (points inside the
    bounds, occupied voxels) are further synchronisations of torch's."""
    worldtogt = _inputs.host64(worldtogt)
    gttoworld = np.linalg.inv(worldtogt)
    pts = _inputs.points(gt_points, device, "dtu_eval", POINT_DTYPES).to(torch.float64)
    _lib.require_cuda(pts, "gt_points")
    pts = _affine(pts, gttoworld)
    frames = visibility_frames(edge_visibility_frames_ratio, len(edge_maps))
    _, mask = _visibility(pts, edge_maps, intrinsics_list, camtoworld_list, h, w, edge_visibility_threshold, invert, frames, True, device)
    edge_points = pts[mask.bool()]
    down = edge_metrics.downsample_point_cloud_average(edge_points, num_voxels_per_axis=num_voxels_per_axis)
    return _affine(down, worldtogt)


def evaluate_dtu(pred, gt_edge_points, worldtogt, threshold=5.0, num_voxels_per_axis=256, device="cuda"):
    """``process_scan`` of src/eval/eval_DTU.py:39-69.  ``pred`` is the path of a ``parametric_edges.json`` - sampled on the device through
    ``parametric_edges.sample_edges``, curves first as the reference concatenates them - or an (n, 3) array of points in world
    coordinates; ``gt_edge_points`` (m, 3) in the ground-truth frame (``gt_edge_points()``'s result, or a loaded ``edge_points.ply``).  The
    prediction is transformed by ``worldtogt`` in fp64, down-sampled to one point per occupied voxel of a ``num_voxels_per_axis``^3 grid on
    its own extent, searched against the ground truth and back (``edge_metrics.nearest_neighbors``: fp32 distances), and the distances
    ``<= float32(threshold)`` are counted, in fp32.  One device-to-host copy, of the two counts.
    -> ``{"precision", "recall", "n_pred", "n_gt", "hits_pred", "hits_gt"}``: precision = hits_pred / n_pred over the down-sampled
    prediction, recall = hits_gt / n_gt over the ground truth."""
    if isinstance(pred, (str, os.PathLike)):
        d = _inputs.load_edge_dict(pred)
        pts = parametric_edges.sample_edges(d["curves_ctl_pts"], d["lines_end_pts"], device=device).points
    else:
        pts = _inputs.points(pred, device, "dtu_eval", POINT_DTYPES).to(torch.float64)
    _lib.require_cuda(pts, "pred")
    gt = _inputs.points(gt_edge_points, pts.device, "edge_metrics")
    pts = _affine(pts, _inputs.host64(worldtogt))
    down = edge_metrics.downsample_point_cloud_average(pts, num_voxels_per_axis=num_voxels_per_axis)
    if down.shape[0] == 0 or gt.shape[0] == 0:
        raise ValueError(f"evaluate_dtu: empty point set (pred {int(down.shape[0])} points after down-sampling, gt {int(gt.shape[0])})")
    dist_d2s, _ = edge_metrics.nearest_neighbors(down, gt)
    dist_s2d, _ = edge_metrics.nearest_neighbors(gt, down)
    thr = torch.tensor(float(np.float32(threshold)), dtype=torch.float32, device=dist_d2s.device)
    hits_pred, hits_gt = torch.stack([(dist_d2s <= thr).sum(), (dist_s2d <= thr).sum()]).tolist()       # the one copy
    n_pred, n_gt = int(down.shape[0]), int(gt.shape[0])
    return {"precision": hits_pred / n_pred, "recall": hits_gt / n_gt, "n_pred": n_pred, "n_gt": n_gt, "hits_pred": int(hits_pred),
            "hits_gt": int(hits_gt)}
