"""Points on fitted parametric edges, on the device: the link between a ``parametric_edges.json`` and the edge metrics.

Mirrors of the reference's ``bezier_curve_length`` (src/eval/eval_util.py:90-135 and its copy src/edge_extraction/extract_util.py:291-336),
``get_pred_points_and_directions`` (eval_util.py:300-415), ``process_geometry_data`` / ``compute_visibility`` / ``project2D_single``
(src/edge_extraction/extract_parametric_edge.py:65-134, :137-213) and the tail of ``get_parametric_edge`` (:257-300), plus
``sample_edges`` - the two HIP launches behind them (``emap_edge_sample_counts``, ``emap_edge_sample_fill``; csrc/parametric.hip) - and
``evaluate_parametric_edges``: a parametric edge set and a ground truth to the metrics dict in one call whose points never leave the device.

The reference evaluates ``bezier_curve_length`` in nested Python loops (10^4 derivative norms per curve); the kernel forms the same sums in
the same order in fp64, so the lengths agree to the last bits and the sample counts ``int(length // resolution)`` are equal wherever
``length / resolution`` is not within rounding of an integer.  Everything is fp64 until the reference casts (``process_geometry_data`` returns
float32).  There is no CPU fallback for the sampling; ``compute_visibility`` is torch on whatever device the edge maps live on (its data are
a handful of points per edge and frame) and needs no GPU.  Only cubic Beziers and segments, as the reference's evaluation.

``directions`` are what ``get_pred_points_and_directions`` returns, formula for formula, and on curves that is NOT the tangent: the
reference multiplies ``A = -3 P0 + 9 P1 - 9 P2 + 3 P3`` by ``3 t^2`` and ``B = 6 P0 - 12 P1 + 6 P2`` by ``2 t`` (eval_util.py:340-381), and
A and B already carry the derivative's factors 3 and 2 - it normalises ``9 t^2 a3 + 4 t a2 + a1`` where the derivative is
``3 t^2 a3 + 2 t a2 + a1``.  The two agree at t = 0 only; on the recorded fixture they are up to more than 90 degrees apart.  They are
reproduced because this module mirrors the reference's outputs; ``sample_edges(..., tangents=True)`` also returns the true unit tangents.
"""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _inputs, _lib, edge_metrics

MAX_NUM_SAMPLES = 1024     # sub-intervals of the Simpson rule (csrc/parametric.hip: PE_MAX_SAMPLES)


class EdgeSamples(NamedTuple):
    """What ``sample_edges`` returns.  Edge e < C is curve e, edge C + j is line j; the points of an edge are contiguous, edges in order."""
    points: torch.Tensor            # (n, 3) fp64, device
    directions: torch.Tensor        # (n, 3) fp64, device: the reference's direction vectors - on curves NOT the tangents (module docstring)
    edge_id: torch.Tensor           # (n) int32, device
    counts: torch.Tensor            # (C + L) int64, device: samples per edge
    lengths: torch.Tensor           # (C + L) fp64, device
    n_curve_points: int             # the first n_curve_points rows belong to curves
    tangents: Optional[torch.Tensor] = None     # (n, 3) fp64, device: unit tangents (NaN where the derivative is zero); with tangents=True


def sample_edges(curves_ctl_pts, lines_end_pts, sample_resolution=0.005, num_samples=100, device="cuda", tangents=False):
    """Sample C cubic Beziers (C, 4, 3) and L segments (L, 2, 3): per edge ``int(length // sample_resolution)`` points at
    ``t = linspace(0, 1, num)`` with the reference's direction vectors (not tangents on curves: module docstring), curves first; with
    ``tangents=True`` also the unit tangents ``B'(t) / |B'(t)|`` (lines: ``(p1 - p0) / |p1 - p0|``).  -> ``EdgeSamples``.  Lists and numpy
    arrays go to ``device``; tensors are used where they are and must be on a GPU.  ``num_samples`` is the reference's Simpson
    resolution of ``bezier_curve_length`` (100 everywhere it is called).  One launch for lengths and counts, ``torch.cumsum``, ONE host
    synchronisation (the totals), one launch that fills the points.  Raises ``ValueError`` when a length is not finite - the reference's
    ``int(nan)`` raises there too - or when ``length / sample_resolution`` is 9e18 or more.  Bit-identical from run to run."""
    curves, lines = _inputs.to_device(curves_ctl_pts, device).reshape(-1, 4, 3), _inputs.to_device(lines_end_pts, device).reshape(-1, 2, 3)
    if not (math.isfinite(sample_resolution) and sample_resolution > 0):
        raise ValueError(f"sample_edges: sample_resolution must be finite and > 0 (got {sample_resolution!r})")
    if not 1 <= int(num_samples) <= MAX_NUM_SAMPLES:
        raise ValueError(f"sample_edges: num_samples must be in 1..{MAX_NUM_SAMPLES} (got {num_samples!r})")
    _lib.require_cuda(curves, "curves_ctl_pts")
    _lib.require_cuda(lines, "lines_end_pts")
    dev = curves.device
    if lines.device != dev:
        raise ValueError(f"sample_edges: curves_ctl_pts is on {dev}, lines_end_pts on {lines.device}")
    C, L = int(curves.shape[0]), int(lines.shape[0])
    lengths = torch.empty(C + L, device=dev, dtype=torch.float64)
    counts = torch.empty(C + L, device=dev, dtype=torch.int64)
    offsets = torch.zeros(C + L + 1, device=dev, dtype=torch.int64)
    n = n_curve = 0
    if C + L > 0:
        with _lib.on_device(curves):
            _lib.api().edge_sample_counts(curves, C, lines, L, float(sample_resolution), int(num_samples), lengths, counts, _lib.stream_ptr(dev))
        torch.cumsum(counts.clamp(min=0), 0, out=offsets[1:])
        n, n_curve, lowest = torch.stack([offsets[-1], offsets[C], counts.min()]).tolist()       # the one synchronisation
        if lowest < 0:
            bad = torch.nonzero(counts < 0).reshape(-1).tolist()
            raise ValueError(f"sample_edges: the length of edge(s) {bad[:8]} is not finite, or too long for sample_resolution (length / "
                             f"sample_resolution >= 9e18); curves are edges 0..{C - 1}, lines follow")
    points = torch.empty(n, 3, device=dev, dtype=torch.float64)
    directions = torch.empty(n, 3, device=dev, dtype=torch.float64)
    edge_id = torch.empty(n, device=dev, dtype=torch.int32)
    tang = torch.empty(n, 3, device=dev, dtype=torch.float64) if tangents else None
    if n > 0:
        with _lib.on_device(curves):
            if tangents:
                _lib.api().edge_sample_fill_tangents(curves, C, lines, L, offsets, points, directions, tang, edge_id, n, _lib.stream_ptr(dev))
            else:
                _lib.api().edge_sample_fill(curves, C, lines, L, offsets, points, directions, edge_id, n, _lib.stream_ptr(dev))
    return EdgeSamples(points, directions, edge_id, counts, lengths, int(n_curve), tang)


def bezier_curve_length(control_points, num_samples):
    """Mirror of ``bezier_curve_length`` (eval_util.py:90-135) for ONE cubic (4, 3): the nested composite Simpson rule, on the device.
    -> float.  The reference's routine takes any degree; any other raises ``NotImplementedError`` (nothing in the reference calls it
    with one)."""
    cp = np.asarray(control_points, dtype=np.float64)
    if cp.ndim != 2 or cp.shape[1] != 3:
        raise ValueError(f"bezier_curve_length: control_points must be (4, 3), got {cp.shape}")
    if cp.shape[0] != 4:
        raise NotImplementedError(f"bezier_curve_length: {cp.shape[0]} control points (only cubic Beziers, 4 control points)")
    if not 1 <= int(num_samples) <= MAX_NUM_SAMPLES:
        raise ValueError(f"bezier_curve_length: num_samples must be in 1..{MAX_NUM_SAMPLES} (got {num_samples!r})")
    curves = torch.as_tensor(cp.reshape(1, 4, 3)).to("cuda")
    lengths = torch.empty(1, device=curves.device, dtype=torch.float64)
    counts = torch.empty(1, device=curves.device, dtype=torch.int64)
    with _lib.on_device(curves):
        _lib.api().edge_sample_counts(curves, 1, None, 0, 1.0, int(num_samples), lengths, counts, _lib.stream_ptr(curves.device))
    return float(lengths[0])


def get_pred_points_and_directions(json_path_or_dict, sample_resolution=0.005):
    """Mirror of ``get_pred_points_and_directions`` (eval_util.py:300-415): ``(all_curve_points (nc, 3), all_line_points (nl, 3),
    all_curve_directions (nc, 3), all_line_directions (nl, 3))`` as fp64 numpy arrays.  Differences: a dict is accepted in place of the
    path; the directions are arrays, not Python lists of arrays; line points are ``p0 + t (p1 - p0)`` as in ``process_geometry_data``
    (here the reference forms ``(1 - t) p0 + t p1``: one rounding apart).  The curve directions are the reference's, which are NOT the
    curves' tangents (module docstring): on a curve whose last two control points coincide the "direction" at t = 1 is ``6 (P0 - P3)``
    normalised, against the direction of travel, where the tangent is undefined.  ``sample_edges(..., tangents=True)`` has the tangents."""
    d = _inputs.load_edge_dict(json_path_or_dict)
    s = sample_edges(d["curves_ctl_pts"], d["lines_end_pts"], sample_resolution)
    k = s.n_curve_points
    p, v = s.points.cpu().numpy(), s.directions.cpu().numpy()
    return p[:k], p[k:], v[:k], v[k:]


def _select(edge_dict, valid_curve, valid_line):
    """process_geometry_data's dict handling (:88-107): -> curves (C, 4, 3), lines (L, 2, 3) after the masks, and return_edge_dict."""
    curve_paras = np.array(edge_dict["curves_ctl_pts"], dtype=np.float64).reshape(-1, 12)
    if valid_curve is not None:
        curve_paras = curve_paras[valid_curve]
    curve_paras = curve_paras.reshape(-1, 4, 3)
    lines = np.array(edge_dict["lines_end_pts"], dtype=np.float64).reshape(-1, 6)
    if valid_line is not None:
        lines = lines[valid_line]
    return curve_paras, lines.reshape(-1, 2, 3), {"curves_ctl_pts": curve_paras.tolist(), "lines_end_pts": lines.tolist()}


def process_geometry_data(edge_dict, worldtogt=None, valid_curve=None, valid_line=None, sample_resolution=0.005, device="cuda"):
    """Mirror of ``process_geometry_data`` (extract_parametric_edge.py:65-134): ``(points (n, 3) float32 numpy, return_edge_dict)``.
    ``valid_curve`` / ``valid_line`` select edges (a bool mask or indices), ``worldtogt`` (4, 4) is applied to the control points before
    sampling while ``return_edge_dict`` holds the selected, UNtransformed parameters - all as the reference.  The cast to float32 happens on
    the device (round to nearest, as numpy's)."""
    curves, lines, return_edge_dict = _select(edge_dict, valid_curve, valid_line)
    if worldtogt is not None:
        worldtogt = np.asarray(worldtogt, dtype=np.float64)
        curves = curves @ worldtogt[:3, :3].T + worldtogt[:3, 3]
        lines = lines @ worldtogt[:3, :3].T + worldtogt[:3, 3]
    s = sample_edges(curves, lines, sample_resolution, device=device)
    return s.points.float().cpu().numpy(), return_edge_dict


def _ragged_points(all_curve_points, all_line_points):
    """The reference's ragged lists (one (k, 3)-shaped list per edge, k >= 0) -> points (N, 3) fp64 numpy, edge index (N) int64, E."""
    per_edge = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in list(all_curve_points) + list(all_line_points)]
    E = len(per_edge)
    if E == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64), 0
    eid = np.repeat(np.arange(E, dtype=np.int64), [len(p) for p in per_edge])
    return np.concatenate(per_edge), eid, E


def edge_frame_visibility(all_curve_points, all_line_points, edges, intrinsics_list, camtoworld_list, h, w, edge_visibility_threshold):
    """The (edge, frame) table behind ``compute_visibility``: ``(visible (E, F) bool, means (E, F) fp64, n_valid (E, F) int64)`` on the
    device of ``edges``.  ``means`` is the mean of the edge map over the edge's points whose rounded pixel lies in the image (NaN when
    there is none)."""
    maps = edges if isinstance(edges, torch.Tensor) else torch.as_tensor(np.asarray(edges))       # where and as they are: no copy, no cast
    if maps.dim() == 4:
        maps = maps[..., :1]                                              # the reference reads channel 0 of (F, H, W, c)
    maps = _inputs.edge_maps(maps, h, w, "compute_visibility: edges")
    F = int(maps.shape[0])
    if len(intrinsics_list) != F or len(camtoworld_list) != F:
        raise ValueError(f"compute_visibility: {F} edge maps, {len(intrinsics_list)} intrinsics, {len(camtoworld_list)} poses")
    dev = maps.device
    pts, eid, E = _ragged_points(all_curve_points, all_line_points)
    if E == 0 or F == 0:
        return (torch.zeros(E, F, dtype=torch.bool, device=dev), torch.full((E, F), float("nan"), dtype=torch.float64, device=dev),
                torch.zeros(E, F, dtype=torch.int64, device=dev))
    # K, R, T per frame on the host as the reference forms them (:156-159); F small matrices, T as (F, 3, 1) for the sum below
    K, R, T = (torch.as_tensor(a).to(dev) for a in _inputs.world_to_camera(intrinsics_list, camtoworld_list))
    T = T.unsqueeze(-1)
    X = torch.as_tensor(pts).to(dev)
    eid_t = torch.as_tensor(eid).to(dev)
    x = torch.matmul(K, torch.matmul(R, X.T.unsqueeze(0)) + T)            # (F, 3, N): K @ (R @ X + T), fp64
    uv = torch.round(x[:, :2] / x[:, 2:3])                                # half to even, as np.round
    u, v = uv[:, 0], uv[:, 1]
    valid = (u >= 0) & (u < w) & (v >= 0) & (v < h)                       # before the integer cast; NaN and inf compare false
    ui = torch.where(valid, u, torch.zeros_like(u)).long()
    vi = torch.where(valid, v, torch.zeros_like(v)).long()
    fi = torch.arange(F, device=dev).unsqueeze(1).expand_as(ui)
    vals = maps[fi, vi, ui].to(torch.float64)                             # (F, N)
    zero = torch.zeros_like(vals)
    sums = torch.zeros(E, F, dtype=torch.float64, device=dev).index_add_(0, eid_t, torch.where(valid, vals, zero).T.contiguous())
    n_valid = torch.zeros(E, F, dtype=torch.int64, device=dev).index_add_(0, eid_t, valid.T.contiguous().long())
    neg = torch.full_like(vals, float("-inf"))
    top = torch.full((E, F), float("-inf"), dtype=torch.float64, device=dev)
    top = top.scatter_reduce(0, eid_t.unsqueeze(1).expand(-1, F), torch.where(valid, vals, neg).T.contiguous(), reduce="amax", include_self=True)
    means = sums / n_valid.to(torch.float64)                              # 0 / 0 = NaN: no valid point
    visible = (n_valid > 0) & (means > edge_visibility_threshold) & (top > 0.5)
    return visible, means, n_valid


def compute_visibility(all_curve_points, all_line_points, edges, intrinsics_list, camtoworld_list, h, w, edge_visibility_threshold,
                       edge_visibility_frames):
    """Mirror of ``compute_visibility`` (extract_parametric_edge.py:137-213): a bool numpy array (E), curves first - edge e is kept when it
    is visible in MORE than ``edge_visibility_frames`` frames; visible in a frame means: the mean of the edge map over the edge's projected
    points that fall in the image exceeds ``edge_visibility_threshold`` and their maximum exceeds 0.5.  Projection in fp64 in the
    reference's order, ``K @ (R @ X + T)`` divided by its third row, no depth test; pixels rounded half to even; a point is valid when
    ``0 <= u < w`` and ``0 <= v < h`` (tested on the rounded fp64 values, so a non-finite coordinate is invalid where the reference's
    integer cast of it is undefined).  ``edges`` is the reference's (F, H, W, 1) numpy array, or an (F, H, W) tensor on any device: the
    computation runs there, in torch - the data are E * F * (2 or 4) points.  The mean is an fp64 sum over the valid points divided by
    their number; for 8-bit maps the sum is exact, so the result does not depend on the order of the reduction."""
    visible, _, _ = edge_frame_visibility(all_curve_points, all_line_points, edges, intrinsics_list, camtoworld_list, h, w,
                                          edge_visibility_threshold)
    return (visible.sum(dim=1) > edge_visibility_frames).cpu().numpy()


def finish_parametric_edges(merged_edge_dict, visible_checking=False, edges=None, intrinsics_list=None, camtoworld_list=None, h=None, w=None,
                            device="cuda"):
    """The tail of ``get_parametric_edge`` (extract_parametric_edge.py:257-300) behind the fitting and merging (``edge_fitting.edge_fit`` and
    ``edge_fitting.merge``; ``edge_fitting.get_parametric_edge`` runs all three): with ``visible_checking`` the edges whose control / end points are seen (threshold 0.5) in more than ``ceil(0.1 F)`` of the F edge maps
    are kept, then the kept edges are sampled with ``worldtogt`` = identity.  The maps and cameras the reference reads with
    ``get_edge_maps`` are arguments here.  -> ``(pred_points float32 numpy, return_edge_dict)``."""
    valid_curve = valid_line = None
    if visible_checking:
        if edges is None or intrinsics_list is None or camtoworld_list is None or h is None or w is None:
            raise ValueError("finish_parametric_edges: visible_checking needs edges, intrinsics_list, camtoworld_list, h and w")
        _, _, return_edge_dict = _select(merged_edge_dict, None, None)
        all_curve_points, all_line_points = return_edge_dict["curves_ctl_pts"], return_edge_dict["lines_end_pts"]
        edge_visibility_frames = math.ceil(0.1 * len(edges))
        edge_visibility = compute_visibility(all_curve_points, all_line_points, edges, intrinsics_list, camtoworld_list, h, w, 0.5,
                                             edge_visibility_frames)
        valid_curve, valid_line = edge_visibility[:len(all_curve_points)], edge_visibility[len(all_curve_points):]
    return process_geometry_data(merged_edge_dict, np.eye(4), valid_curve, valid_line, device=device)


def evaluate_parametric_edges(json_path_or_dict, gt_points, thresholds=(0.005, 0.01, 0.02), downsample=256, sample_resolution=0.005,
                              device="cuda"):
    """A ``parametric_edges.json`` (path or dict) against ground-truth points: sample the edges (``sample_edges``), cast to float32 as the
    reference's loaders do, and run ``edge_metrics.evaluate_edges`` - the ``process_scan`` sequence of src/eval/eval_ABC.py:63-89 with its
    prediction taken from the fitted edges.  The sampled points never leave the device.  ``device`` is where the edge set and a numpy
    ``gt_points`` go; a ``gt_points`` tensor is used where it is and must be on that device.  -> the metrics dict."""
    d = _inputs.load_edge_dict(json_path_or_dict)
    s = sample_edges(d["curves_ctl_pts"], d["lines_end_pts"], sample_resolution, device=device)
    return edge_metrics.evaluate_edges(s.points.float(), gt_points, thresholds=thresholds, downsample=downsample, device=device)
