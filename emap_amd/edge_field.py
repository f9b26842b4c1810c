"""The exact distance field of an edge set, on the device: point-to-edge distances, the error of a trained UDF, scores without sampling.

The 3D counterpart of ``edge_score.distance_maps``.  An edge set - line segments and cubic Beziers, or any polylines - becomes ONE segment
table (``edge_segments``: ``emap_field_expand_edges``; ``polyline_segments``), and ``point_edge_distances`` is ONE call of
``emap_field_point_distances`` (csrc/field.hip, include/emap_field_hip.h, where the semantics are stated): for every point the nearest
segment by brute force in fp64, with the squared distance, the segment and the foot parameter, the lowest index among equal distances.
A curve is its chord polyline: distances are exact to the table, and the table's deviation from the true cubic is the caller's choice of
``curve_segments`` (for ``synthetic.curved_wireframe`` 8.07e-4 at 32 chords, 1/64 of it at 256 - tests/test_edge_field_cpu.py measures
both), which is why the two evaluation functions default to 256 chords and the primitives to the rasteriser's 32.

``evaluate_udf`` answers how good a trained field is: |udf(x) - d(x)| over the lattice points within ``band`` of the wire frame.
``evaluate_points_on_edges`` scores a point cloud against the edges themselves: accuracy without sampling the ground truth, and per edge
how much of it was reconstructed.  tests/edge_field_ref.py is the numpy mirror.

EDGE e < L is line e, edge L + j is curve j - the rasteriser's convention.  numpy inputs go to ``device``; tensors are used where they
are.  There is no CPU fallback: without a GPU the calls raise ``RuntimeError``.
"""
import math

import numpy as np
import torch

from . import _inputs, _lib, edge_raster
from .edge_metrics import f_score

FIELD_Q_TILE = 1024            # csrc/field.hip: FIELD_Q_TILE - points per workgroup of the search
FIELD_S_TILE = 256             # csrc/field.hip: FIELD_S_TILE - segments per LDS tile
FIELD_STATS_THREADS = 1024     # csrc/field.hip: FIELD_STATS_THREADS - the summation order of emap_field_stats (the header states it)
FIELD_HIST_CAP = 4096          # csrc/field.hip: FIELD_HIST_CAP - n_ids * (1 + K) up to which per-id counts go through LDS
_CHUNK = 1 << 20               # lattice points per step of evaluate_udf


def _curve_segments(curve_segments):
    curve_segments = int(curve_segments)
    if not 1 <= curve_segments <= _lib.FIELD_MAX_CURVE_SEGMENTS:
        raise ValueError(f"edge_field: curve_segments must be in [1, {_lib.FIELD_MAX_CURVE_SEGMENTS}], got {curve_segments}")
    return curve_segments


def _edge_set(lines, curves, curve_segments, device):
    """The checked inputs of a table: lines (L, 6) and curves (C, 12) fp64 on one device, and n_seg."""
    lines_t = edge_raster._edges(lines, 6, "lines", device, tag="edge_field")
    curves_t = edge_raster._edges(curves, 12, "curves", device, tag="edge_field")
    L, Cn = int(lines_t.shape[0]), int(curves_t.shape[0])
    n_seg = L + Cn * curve_segments
    if not 1 <= n_seg <= _lib.FIELD_MAX_SEGMENTS:
        raise ValueError(f"edge_field: {L} lines and {Cn} curves of {curve_segments} chords are {n_seg} segments, a table holds 1 to {_lib.FIELD_MAX_SEGMENTS}")
    return lines_t, curves_t, n_seg


def edge_segments(lines, curves, curve_segments=32, device="cuda"):
    """The segment table of L segments ``lines`` (L, 2, 3) or (L, 6) and C cubic Beziers ``curves`` (C, 4, 3) or (C, 12), either may be
    empty: -> ``(segs (n_seg, 2, 3) fp64, seg_edge (n_seg) int32)`` on the device, lines first, then every curve as ``curve_segments``
    chords between B(k / n) and B((k + 1) / n) - the rasteriser's segments, bit for bit."""
    curve_segments = _curve_segments(curve_segments)
    lines_t, curves_t, n_seg = _edge_set(lines, curves, curve_segments, device)
    _lib.require_cuda(lines_t, "lines")
    _lib.require_cuda(curves_t, "curves")
    if curves_t.device != lines_t.device:
        raise ValueError(f"edge_field: lines are on {lines_t.device}, curves on {curves_t.device}")
    L, Cn = int(lines_t.shape[0]), int(curves_t.shape[0])
    segs = torch.empty((n_seg, 2, 3), device=lines_t.device, dtype=torch.float64)
    seg_edge = torch.empty(n_seg, device=lines_t.device, dtype=torch.int32)
    with _lib.on_device(segs):
        _lib.field_api().field_expand_edges(lines_t if L else None, L, curves_t if Cn else None, Cn, curve_segments, segs, seg_edge,
                                            _lib.stream_ptr(segs.device))
    return segs, seg_edge


def polyline_segments(polylines, device="cuda"):
    """The segment table of a list of polylines, ``(k_i, 3)`` vertex arrays with k_i >= 2 - ABC's per-edge vertex lists: polyline i is
    edge i, its k_i - 1 segments in order.  -> ``(segs, seg_edge)`` as ``edge_segments``; torch only, no kernel."""
    a, b, e = [], [], []
    for i, p in enumerate(polylines):
        v = _inputs.to_device(p, device)
        if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] < 2:
            raise ValueError(f"edge_field: polyline {i} must be (k, 3) with k >= 2, got {tuple(v.shape)}")
        a.append(v[:-1])
        b.append(v[1:])
        e.append(torch.full((int(v.shape[0]) - 1,), i, dtype=torch.int32, device=v.device))
    n_seg = sum(int(x.shape[0]) for x in a)
    if not 1 <= n_seg <= _lib.FIELD_MAX_SEGMENTS:
        raise ValueError(f"edge_field: the polylines have {n_seg} segments, a table holds 1 to {_lib.FIELD_MAX_SEGMENTS}")
    return torch.stack([torch.cat(a), torch.cat(b)], dim=1).contiguous(), torch.cat(e)


def _table(segs, seg_edge, device):
    s = _inputs.to_device(segs, device)
    if s.dim() != 3 or tuple(s.shape[1:]) != (2, 3) or not 1 <= int(s.shape[0]) <= _lib.FIELD_MAX_SEGMENTS:
        raise ValueError(f"edge_field: segs must be (n_seg, 2, 3) with n_seg in [1, {_lib.FIELD_MAX_SEGMENTS}], got {tuple(s.shape)}")
    if seg_edge is not None:
        seg_edge = _inputs.to_device(seg_edge, device, torch.int32)
        if tuple(seg_edge.shape) != (int(s.shape[0]),):
            raise ValueError(f"edge_field: seg_edge must be ({int(s.shape[0])},) like segs, got {tuple(seg_edge.shape)}")
    return s, seg_edge


def workspace_bytes(n, n_seg, split=0):
    """What ``emap_field_workspace_bytes`` reports for a search of n points in n_seg segments: 0 when the segments are one part."""
    nb = _lib.C.c_size_t()
    _lib.field_api().field_workspace_bytes(int(n), int(n_seg), int(split), nb)
    return nb.value


def _search(points, segs, split):
    """(d2, seg, t) of checked device tensors: the one call."""
    n, n_seg, dev = int(points.shape[0]), int(segs.shape[0]), points.device
    d2 = torch.empty(n, device=dev, dtype=torch.float64)
    seg = torch.empty(n, device=dev, dtype=torch.int32)
    t = torch.empty(n, device=dev, dtype=torch.float64)
    with _lib.on_device(points):
        nbytes = workspace_bytes(n, n_seg, split)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
        _lib.field_api().field_point_distances(points, _lib.FIELD_POINTS_DTYPES[points.dtype], n, segs, n_seg, int(split), d2, seg, t, ws, nbytes,
                                               _lib.stream_ptr(dev))
    return d2, seg, t


def point_edge_distances(points, segs, seg_edge=None, split=0, device="cuda"):
    """For every row of ``points`` (n, 3), fp32 or fp64 (a float is widened exactly), the nearest segment of the table ``segs``
    (n_seg, 2, 3): -> dict of device tensors

        d2, seg, t    the kernel's outputs: squared distance fp64, segment index int32 (the lowest among equal distances), foot parameter
        dist          sqrt(d2)
        edge          seg_edge[seg] int32 (with ``seg_edge``)
        closest       a + t (b - a) of the nearest segment, (n, 3) fp64

    A point with a NaN coordinate has seg = edge = -1, t = 0 and d2 = dist = closest = NaN.  ``split`` forces the number of parts the
    segments are divided into across workgroups (0: automatic) and never changes a bit.  No synchronisation."""
    if int(split) < 0:
        raise ValueError(f"edge_field: split must be 0 (automatic) or >= 1, got {split}")
    p = _inputs.points(points, device, "edge_field", keep=(torch.float32, torch.float64))
    s, seg_edge = _table(segs, seg_edge, device)
    if int(p.shape[0]) > _lib.FIELD_MAX_POINTS:
        raise ValueError(f"edge_field: {int(p.shape[0])} points, a call takes at most {_lib.FIELD_MAX_POINTS}")
    for t_, name in ((p, "points"), (s, "segs"), (seg_edge, "seg_edge")):
        if t_ is not None:
            _lib.require_cuda(t_, name)
            if t_.device != p.device:
                raise ValueError(f"edge_field: points are on {p.device}, {name} on {t_.device}")
    d2, seg, t = _search(p, s, split)
    out = {"d2": d2, "seg": seg, "t": t, "dist": d2.sqrt()}
    found = seg >= 0
    k = seg.clamp(min=0).long()
    if seg_edge is not None:
        out["edge"] = torch.where(found, seg_edge[k], seg)
    a, b = s[k, 0], s[k, 1]
    closest = a + t[:, None] * (b - a)
    out["closest"] = torch.where(found[:, None], closest, torch.full((), float("nan"), dtype=torch.float64, device=p.device))
    return out


def edge_udf(points, lines, curves, curve_segments=32, device="cuda"):
    """The exact unsigned distance field of an edge set at ``points`` (n, 3): ``dist`` (n) fp64 on the device."""
    p = _inputs.points(points, device, "edge_field", keep=(torch.float32, torch.float64))
    segs, _ = edge_segments(lines, curves, curve_segments, device=p.device if isinstance(points, torch.Tensor) else device)
    return point_edge_distances(p, segs)["dist"]


def _taus(thresholds):
    ts = tuple(thresholds)
    if not 1 <= len(ts) <= _lib.FIELD_MAX_THRESHOLDS:
        raise ValueError(f"edge_field: 1 to {_lib.FIELD_MAX_THRESHOLDS} thresholds (got {len(ts)})")
    if not all(math.isfinite(float(t)) and float(t) >= 0 for t in ts):
        raise ValueError(f"edge_field: thresholds must be finite and >= 0, got {ts}")
    return ts


def _stats_into(d2, ids, n_ids, taus, counts, sums, edge_counts):
    """Enqueue emap_field_stats of d2 (n) fp64 into views of one statistics buffer."""
    K = len(taus)
    with _lib.on_device(counts):
        _lib.field_api().field_stats(d2, ids, int(n_ids), (_lib.C.c_double * K)(*[float(t) for t in taus]), K, int(d2.shape[0]), counts, sums,
                                     edge_counts, _lib.stream_ptr(counts.device))


# ------------------------------------------------------------------------------------------------ the error of a field
def udf_error_metrics(n_band, sum_abs, sum_sq, max_abs, sum_err, n_true=None, n_pred=None, n_both=None):
    """The pure formulas of ``evaluate_udf`` from its accumulated numbers.  Divisions as numpy's: 0/0 is NaN."""
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.float64(n_band)
        out = {"n_band": int(n_band), "mae": float(np.float64(sum_abs) / n), "rmse": float(np.sqrt(np.float64(sum_sq) / n)),
               "max_abs": float(max_abs), "bias": float(np.float64(sum_err) / n)}
        if n_true is not None:
            union = np.float64(int(n_true) + int(n_pred) - int(n_both))
            out.update(n_true=int(n_true), n_pred=int(n_pred), n_both=int(n_both), iou=float(np.float64(n_both) / union))
    return out


def _values_fn(func):
    """x (P, 3) fp32 on the device -> udf (P) : a UDFNetwork or its bound ``.udf`` through the value kernel, else ``func(x)[0]``."""
    from .udf_model import UDFNetwork
    net = func if isinstance(func, UDFNetwork) else getattr(func, "__self__", None)
    if isinstance(net, UDFNetwork) and (func is net or getattr(func, "__name__", "") == "udf"):
        return lambda x: net.hip_udf(x, with_grad=False)[0].reshape(-1)
    if not callable(func):
        raise TypeError("edge_field: func must be a UDFNetwork, its .udf, or a callable x -> (udf, ...)")
    return lambda x: func(x)[0].detach().reshape(-1)


def evaluate_udf(func, lines, curves, N=64, band=0.05, udf_threshold=None, curve_segments=256, device="cuda"):
    """How close a field is to the exact distance field of the edge set, over the ``N^3`` lattice of ``extraction.lattice_points``.

    ``func``: a ``UDFNetwork`` or its bound ``.udf`` (evaluated by ``hip_udf(with_grad=False)``), or any callable ``x -> (udf, ...)`` - what
    ``extract_edge`` passes.  With u = func(x) and d = the exact distance of x to the edges (``curve_segments`` chords per curve), over the
    lattice points with d < band: -> dict of ``n_band``, ``mae`` = mean |u - d|, ``rmse``, ``max_abs`` and ``bias`` = mean (u - d).  With
    ``udf_threshold`` = tau also, over the whole lattice, ``n_true`` (d < tau), ``n_pred`` (u < tau), ``n_both`` and ``iou`` - what a
    threshold of the extraction would keep.  The lattice is walked in chunks of 2^20 points; counts are int64 and sums fp64 on the device,
    ONE device-to-host copy at the end, nothing of size N^3 is allocated."""
    from . import extraction
    N, band = int(N), float(band)
    if N < 2:
        raise ValueError(f"edge_field: N must be >= 2, got {N}")
    if not (math.isfinite(band) and band > 0):
        raise ValueError(f"edge_field: band must be finite and > 0, got {band}")
    tau = None if udf_threshold is None else float(udf_threshold)
    if tau is not None and not math.isfinite(tau):
        raise ValueError(f"edge_field: udf_threshold must be finite, got {tau}")
    curve_segments = _curve_segments(curve_segments)
    _edge_set(lines, curves, curve_segments, "cpu" if not isinstance(lines, torch.Tensor) else lines.device)      # the checks, before any device work
    values = _values_fn(func)
    dev = extraction._gpu(device)
    segs, _ = edge_segments(lines, curves, curve_segments, device=dev)
    acc = torch.zeros(8, device=dev, dtype=torch.int64)        # [n_band, n_true, n_pred, n_both | sum |e|, sum e^2, max |e|, sum e] as bits
    cnt, flt = acc[:4], acc[4:].view(torch.float64)
    xyz = torch.empty((min(_CHUNK, N ** 3), 3), device=dev, dtype=torch.float32)
    with torch.no_grad():
        for first in range(0, N ** 3, _CHUNK):
            x = extraction.lattice_points(N, first, min(_CHUNK, N ** 3 - first), device=dev, out=xyz)
            u = values(x).to(torch.float64)
            d = _search(x, segs, 0)[0].sqrt()
            near = d < band
            e = torch.where(near, u - d, torch.zeros((), dtype=torch.float64, device=dev))
            cnt[0] += near.sum()
            flt[0] += e.abs().sum()
            flt[1] += (e * e).sum()
            flt[2] = torch.maximum(flt[2], e.abs().max())
            flt[3] += e.sum()
            if tau is not None:
                true, pred = d < tau, u < tau
                cnt[1] += true.sum()
                cnt[2] += pred.sum()
                cnt[3] += (true & pred).sum()
        host = acc.cpu()                                         # the one copy
    c, f = host[:4].tolist(), host[4:].view(torch.float64).tolist()
    return udf_error_metrics(c[0], f[0], f[1], f[2], f[3], *(c[1:] if tau is not None else ()))


# ------------------------------------------------------------------------------------------------ points against edges
def points_on_edges_metrics(counts_pred, sums_pred, edge_pred, counts_gt, sums_gt, edge_gt, thresholds, n_lines):
    """The pure formulas of ``evaluate_points_on_edges`` from what its two ``emap_field_stats`` calls return: ``counts_*`` (1 + K),
    ``sums_*`` (2), ``edge_*`` (E, 1 + K), E = lines + curves, lines first.  Divisions as numpy's: 0/0 is NaN."""
    ts = tuple(thresholds)
    cp, cg = np.asarray(counts_pred, dtype=np.int64), np.asarray(counts_gt, dtype=np.int64)
    ep, eg = np.asarray(edge_pred, dtype=np.int64), np.asarray(edge_gt, dtype=np.int64)
    if cp.shape != (1 + len(ts),) or cg.shape != cp.shape or ep.ndim != 2 or ep.shape[1] != 1 + len(ts) or eg.shape != ep.shape:
        raise ValueError(f"edge_field: {len(ts)} thresholds need counts ({1 + len(ts)},) and edge counts (E, {1 + len(ts)}), got {cp.shape}, {cg.shape}, {ep.shape}, {eg.shape}")

    def ratio(a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64)

    out = {"n_pred": int(cp[0]), "n_gt": int(cg[0]), "accuracy": float(ratio(np.asarray(sums_pred)[0], cp[0])),
           "completeness": float(ratio(np.asarray(sums_gt)[0], cg[0]))}
    per_edge = {"n_pred": ep[:, 0], "n_gt": eg[:, 0]}
    pooled = {"line": {"num_pred": int(ep[:n_lines, 0].sum()), "num_gt": int(eg[:n_lines, 0].sum())},
              "curve": {"num_pred": int(ep[n_lines:, 0].sum()), "num_gt": int(eg[n_lines:, 0].sum())}}
    for k, t in enumerate(ts):
        p, r = ratio(cp[1 + k], cp[0]), ratio(cg[1 + k], cg[0])
        with np.errstate(invalid="ignore", divide="ignore"):
            out[f"precision_{t}"], out[f"recall_{t}"], out[f"fscore_{t}"] = float(p), float(r), float(f_score(p, r))
        per_edge[f"pred_within_{t}"], per_edge[f"gt_within_{t}"] = ep[:, 1 + k], eg[:, 1 + k]
        per_edge[f"precision_{t}"], per_edge[f"recall_{t}"] = ratio(ep[:, 1 + k], ep[:, 0]), ratio(eg[:, 1 + k], eg[:, 0])
        for name, sl in (("line", slice(0, n_lines)), ("curve", slice(n_lines, None))):      # the reference's edge_type branches: pooled counts
            row = pooled[name]
            row[f"correct_pred_{t}"], row[f"correct_gt_{t}"] = int(ep[sl, 1 + k].sum()), int(eg[sl, 1 + k].sum())
            row[f"precision_{t}"] = float(ratio(row[f"correct_pred_{t}"], row["num_pred"]))
            row[f"recall_{t}"] = float(ratio(row[f"correct_gt_{t}"], row["num_gt"]))
    out["per_edge"] = per_edge
    out.update(pooled)
    return out


def evaluate_points_on_edges(pred_points, lines, curves, thresholds=(0.005, 0.01, 0.02), interval=0.005, curve_segments=256, device="cuda"):
    """A point cloud ``pred_points`` (n, 3) against the edges themselves - L ``lines`` and C ``curves`` as ``edge_segments`` takes them.

    Accuracy side: the exact distance of every predicted point to the edge set (``curve_segments`` chords per curve), no ground-truth
    sampling: ``accuracy`` (the mean), ``precision_t`` (the share within t), and per edge the points whose nearest edge it is and how many
    of them are within t.  Completeness side: the samples of ``parametric_edges.sample_edges(curves, lines, interval)`` with their edge,
    searched in the prediction with ``nearest_neighbors``: ``completeness``, ``recall_t``, and per edge its samples and how many are
    within t - which ground-truth edges were reconstructed.  Also ``fscore_t``, ``n_pred``, ``n_gt``.  ``"per_edge"``: arrays of length
    L + C (lines first) - ``n_pred``, ``pred_within_t``, ``precision_t``, ``n_gt``, ``gt_within_t``, ``recall_t``; ``"line"`` and
    ``"curve"``: the same counts pooled by edge type, as the reference's ``edge_type`` branches pool them.  Two searches and two statistics
    calls on the device, ONE device-to-host copy of all statistics."""
    from . import parametric_edges
    from .edge_metrics import nearest_neighbors
    ts = _taus(thresholds)
    interval = float(interval)
    if not (math.isfinite(interval) and interval > 0):
        raise ValueError(f"edge_field: interval must be finite and > 0, got {interval}")
    curve_segments = _curve_segments(curve_segments)
    p = _inputs.points(pred_points, device, "edge_field", keep=(torch.float32, torch.float64))
    if int(p.shape[0]) < 1:
        raise ValueError("edge_field: evaluate_points_on_edges needs at least one predicted point")
    dev = p.device if isinstance(pred_points, torch.Tensor) else device
    lines_t, curves_t, _ = _edge_set(lines, curves, curve_segments, dev)
    L, Cn = int(lines_t.shape[0]), int(curves_t.shape[0])
    E, K = L + Cn, len(ts)
    _lib.require_cuda(p, "pred_points")
    segs, seg_edge = edge_segments(lines_t, curves_t, curve_segments, device=dev)
    if segs.device != p.device:
        raise ValueError(f"edge_field: pred_points are on {p.device}, the edges on {segs.device}")
    with torch.no_grad():
        # one buffer for every statistic, so that one copy brings them to the host: [counts pred | counts gt | sums pred | sums gt | edge pred | edge gt]
        buf = torch.empty(2 * (1 + K) + 4 + 2 * E * (1 + K), device=p.device, dtype=torch.int64)
        o = [0, 1 + K, 2 * (1 + K), 2 * (1 + K) + 2, 2 * (1 + K) + 4, 2 * (1 + K) + 4 + E * (1 + K), buf.numel()]
        views = [buf[o[i]:o[i + 1]] for i in range(6)]
        d2, seg, _ = _search(p, segs, 0)
        edge = torch.where(seg >= 0, seg_edge[seg.clamp(min=0).long()], seg)
        _stats_into(d2, edge, E, ts, views[0], views[2], views[4])
        samples = parametric_edges.sample_edges(curves_t.reshape(-1, 4, 3), lines_t.reshape(-1, 2, 3), interval, device=dev)
        ids = torch.where(samples.edge_id < Cn, samples.edge_id + L, samples.edge_id - Cn).to(torch.int32)     # curves first -> lines first
        dist, _ = nearest_neighbors(samples.points.float(), p.float())
        d2_gt = dist.double() * dist.double()                     # the square of a float is exact in fp64, and its root is the float again
        _stats_into(d2_gt, ids.contiguous(), E, ts, views[1], views[3], views[5])
        host = buf.cpu()                                          # the one copy
    h = [host[o[i]:o[i + 1]] for i in range(6)]
    return points_on_edges_metrics(h[0].numpy(), h[2].view(torch.float64).numpy(), h[4].reshape(E, 1 + K).numpy(),
                                   h[1].numpy(), h[3].view(torch.float64).numpy(), h[5].reshape(E, 1 + K).numpy(), ts, L)
