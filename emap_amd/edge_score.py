"""Edge maps scored against edge maps in image space, on the device: exact distance maps, pixel precision / recall / F, chamfer in pixels.

The score that needs no 3D ground truth.  ``distance_maps`` is ONE call of ``emap_score_distance_maps`` (csrc/score.hip,
include/emap_score_hip.h, where the semantics are stated): the exact squared Euclidean distance transform of every frame of a stack of
edge maps, in integers.  ``score_edge_maps`` compares two stacks with a pixel tolerance: the distance map of each, the SET pixels of the
other read against it (``emap_score_stats``: integer counts, one sum of distances per frame in a fixed order), ONE device-to-host copy
of all statistics.  With the ids of ``rasterize_edges(return_ids=True)`` it also gives, per fitted edge, the share of its drawn pixels
that the other maps support - what ``filter_edges_by_support`` drops hallucinated edges by.  tests/edge_score_ref.py is the numpy mirror.

A pixel of a map is SET iff its value exceeds the threshold, strictly; a byte b has the value float32(b / 255.0), the table of
``edge_raster.to_dataset_edges``, so a byte map and its float image have the same mask.

numpy inputs go to ``device``; tensors are used where they are.  There is no CPU fallback: without a GPU the calls raise ``RuntimeError``.
"""
import math

import numpy as np
import torch

from . import _inputs, _lib, edge_raster, validation
from .edge_metrics import f_score

SCORE_STATS_THREADS = 1024     # csrc/score.hip: SCORE_STATS_THREADS - the summation order of a frame's distances (the header states it)
SCORE_HIST_CAP = 8192          # csrc/score.hip: SCORE_HIST_CAP - n_ids * (1 + K) up to which per-edge counts go through LDS


def _maps(a, name, device):
    """(F, h, w) contiguous uint8 or float32 tensor from (F, h, w) or (F, h, w, 1); checked where it is, numpy goes to ``device`` last."""
    t = a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    if t.dim() == 4 and t.shape[3] == 1:
        t = t[..., 0]
    if t.dim() != 3:
        raise ValueError(f"edge_score: {name} must be (F, h, w) or (F, h, w, 1), got {tuple(t.shape)}")
    if t.dtype not in _lib.SCORE_MAPS_DTYPES:
        raise ValueError(f"edge_score: {name} must be uint8 or float32, got {t.dtype}")
    F, h, w = (int(v) for v in t.shape)
    if not 1 <= F <= _lib.SCORE_MAX_FRAMES:
        raise ValueError(f"edge_score: {name} has {F} frames, a call takes 1 to {_lib.SCORE_MAX_FRAMES}")
    if not (1 <= h <= _lib.SCORE_MAX_DIM and 1 <= w <= _lib.SCORE_MAX_DIM):
        raise ValueError(f"edge_score: h and w of {name} must be in [1, {_lib.SCORE_MAX_DIM}], got {h} x {w}")
    return (t if isinstance(a, torch.Tensor) else t.to(device)).contiguous()


def _threshold(v, name):
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"edge_score: {name} must be finite, got {v}")
    return v


def _thresholds_px(thresholds_px):
    ts = tuple(thresholds_px)
    if not 1 <= len(ts) <= _lib.SCORE_MAX_THRESHOLDS:
        raise ValueError(f"edge_score: 1 to {_lib.SCORE_MAX_THRESHOLDS} thresholds_px (got {len(ts)})")
    if not all(math.isfinite(float(t)) and float(t) >= 0 for t in ts):
        raise ValueError(f"edge_score: thresholds_px must be finite and >= 0, got {ts}")
    return ts


def workspace_bytes(F, h, w):
    """What ``emap_score_workspace_bytes`` reports: ``F * h * w * _lib.SCORE_WORKSPACE_PIXEL_BYTES``, the column pass's uint16 per pixel."""
    n = _lib.C.c_size_t()
    _lib.score_api().score_workspace_bytes(int(F), int(h), int(w), n)
    return n.value


def _distance(m, threshold, ws):
    """d2 (F, h, w) int32 of the checked device maps ``m``; ``ws`` is the workspace of their shape (shared by the calls of one score)."""
    F, h, w = m.shape
    d2 = torch.empty((F, h, w), device=m.device, dtype=torch.int32)
    _lib.score_api().score_distance_maps(m, _lib.SCORE_MAPS_DTYPES[m.dtype], threshold, F, h, w, d2, ws, ws.numel(), _lib.stream_ptr(m.device))
    return d2


def distance_maps(maps, threshold=0.5, squared=True, device="cuda"):
    """The exact Euclidean distance transform of every frame of ``maps`` (F, h, w) or (F, h, w, 1), uint8 or float32: -> (F, h, w) int32 on
    the device, the squared distance in pixels to the nearest pixel of the same frame whose value exceeds ``threshold`` - 0 on such a
    pixel, ``_lib.SCORE_NONE`` everywhere in a frame without one.  ``squared=False``: float64 distances, ``inf`` in such a frame.  h and w
    up to 32768.  The only allocations are the output and the workspace (2 bytes per pixel); no synchronisation, the same bits on every run."""
    threshold = _threshold(threshold, "threshold")
    m = _maps(maps, "maps", device)
    _lib.require_cuda(m, "maps")
    with _lib.on_device(m):
        ws = torch.empty(workspace_bytes(*m.shape), device=m.device, dtype=torch.uint8)
        d2 = _distance(m, threshold, ws)
    if squared:
        return d2
    return torch.where(d2 == _lib.SCORE_NONE, torch.full((), float("inf"), dtype=torch.float64, device=m.device), d2.to(torch.float64).sqrt())


def _ratio(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(a, dtype=np.float64) / np.asarray(b, dtype=np.float64)


def metrics_from_counts(counts_pred, sums_pred, counts_gt, sums_gt, thresholds_px, edge_counts=None):
    """The pure formulas, from what two ``emap_score_stats`` calls return: ``counts_*`` (F, 1 + K) - SET pixels, and how many of them lie
    within each threshold of the other set -, ``sums_*`` (F) the summed distances; -> the dict of ``score_edge_maps``.  Divisions as
    numpy's: 0/0 is NaN (and x/0 inf), no exception."""
    ts = tuple(thresholds_px)
    cp, cg = np.asarray(counts_pred, dtype=np.int64), np.asarray(counts_gt, dtype=np.int64)
    sp, sg = np.asarray(sums_pred, dtype=np.float64), np.asarray(sums_gt, dtype=np.float64)
    if cp.ndim != 2 or cp.shape[1] != 1 + len(ts) or cg.shape != cp.shape or sp.shape != cp.shape[:1] or sg.shape != sp.shape:
        raise ValueError(f"edge_score: {len(ts)} thresholds need counts (F, {1 + len(ts)}) and sums (F), got {cp.shape}, {cg.shape}, {sp.shape}, {sg.shape}")

    def metrics(cp, sp, cg, sg):            # per-frame arrays, or the pooled sums as 0-d arrays
        out = {"n_pred": cp[..., 0], "n_gt": cg[..., 0]}
        for k, t in enumerate(ts):
            out[f"precision_{t}"] = _ratio(cp[..., 1 + k], cp[..., 0])
            out[f"recall_{t}"] = _ratio(cg[..., 1 + k], cg[..., 0])
            with np.errstate(invalid="ignore", divide="ignore"):
                out[f"fscore_{t}"] = f_score(out[f"precision_{t}"], out[f"recall_{t}"])
        out["acc_px"], out["comp_px"] = _ratio(sp, cp[..., 0]), _ratio(sg, cg[..., 0])
        out["chamfer_px"] = out["acc_px"] + out["comp_px"]
        return out
    pooled = metrics(cp.sum(0), sp.sum(), cg.sum(0), sg.sum())
    out = {k: int(v) if k in ("n_pred", "n_gt") else float(v) for k, v in pooled.items()}
    out["per_frame"] = metrics(cp, sp, cg, sg)
    if edge_counts is not None:
        ec = np.asarray(edge_counts, dtype=np.int64)
        if ec.ndim != 2 or ec.shape[1] != 1 + len(ts):
            raise ValueError(f"edge_score: edge_counts must be (n_ids, {1 + len(ts)}), got {ec.shape}")
        out["edge_pixels"] = ec[:, 0]
        for k, t in enumerate(ts):
            out[f"edge_support_{t}"] = _ratio(ec[:, 1 + k], ec[:, 0])
    return out


def score_edge_maps(pred, gt, thresholds_px=(1.0, 2.0, 4.0), pred_threshold=0.5, gt_threshold=0.5, ids=None, n_ids=None, device="cuda"):
    """Two stacks of edge maps (F, h, w) or (F, h, w, 1), each uint8 or float32, compared frame by frame with a pixel tolerance.  Two
    distance maps and two statistics calls on the device, ONE device-to-host copy at the end.  -> dict of pooled values - all frames'
    pixels as one set -, and under ``"per_frame"`` the same keys as (F,) arrays:

        n_pred, n_gt          SET pixels (value > pred_threshold / gt_threshold)
        precision_t           pred pixels within t pixels of a gt pixel of the same frame, over n_pred;  recall_t the mirror image;
                              fscore_t = edge_metrics.f_score of the two, for every t of ``thresholds_px`` (1 to 8, keyed as given)
        acc_px, comp_px       the mean distance pred -> gt and gt -> pred;  chamfer_px = acc_px + comp_px

    ``ids`` (F, h, w) int32 as ``rasterize_edges(return_ids=True)`` returns them for ``pred``, with ``n_ids`` = its number of edges:
    also ``edge_pixels`` (n_ids,) - the SET pixels of pred with that id, over all frames - and ``edge_support_t`` (n_ids,), the share of
    them within t of a gt pixel.  Empty sets follow ``evaluate_edges``: divisions as numpy's, so with no pred pixel precision, acc_px,
    chamfer_px and fscore are NaN (0/0), an edge that drew nothing has support NaN, and fscore is NaN when precision = recall = 0;
    against an EMPTY other set every distance is inf: acc_px (or comp_px) is inf and the counts are 0."""
    ts = _thresholds_px(thresholds_px)
    pred_threshold, gt_threshold = _threshold(pred_threshold, "pred_threshold"), _threshold(gt_threshold, "gt_threshold")
    p, g = _maps(pred, "pred", device), _maps(gt, "gt", device)
    if p.shape != g.shape:
        raise ValueError(f"edge_score: pred is {tuple(p.shape)} and gt {tuple(g.shape)}: the same frames, height and width")
    if (ids is None) != (n_ids is None):
        raise ValueError("edge_score: ids and n_ids go together (the ids of rasterize_edges(return_ids=True) and its number of edges)")
    if ids is not None:
        n_ids = int(n_ids)
        if n_ids < 1:
            raise ValueError(f"edge_score: n_ids must be >= 1, got {n_ids}")
        i = ids.detach() if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
        if i.dtype != torch.int32 or i.shape != p.shape:
            raise ValueError(f"edge_score: ids must be int32 {tuple(p.shape)} like pred, got {i.dtype} {tuple(i.shape)}")
        ids = (i if isinstance(ids, torch.Tensor) else i.to(device)).contiguous()
    for t, name in ((p, "pred"), (g, "gt"), (ids, "ids")):
        if t is not None:
            _lib.require_cuda(t, name)
            if t.device != p.device:
                raise ValueError(f"edge_score: pred is on {p.device}, {name} on {t.device}")
    F, h, w = p.shape
    K, dev = len(ts), p.device
    taus = (_lib.C.c_double * K)(*[float(t) for t in ts])
    n_counts, n_edge = F * (1 + K), (n_ids * (1 + K) if ids is not None else 0)
    with _lib.on_device(p):
        # one buffer for every statistic, so that one copy brings them to the host: [counts pred | counts gt | sums pred | sums gt | edge counts]
        buf = torch.empty(2 * n_counts + 2 * F + n_edge, device=dev, dtype=torch.int64)
        counts_p, counts_g = buf[:n_counts], buf[n_counts:2 * n_counts]
        sums_p, sums_g = buf[2 * n_counts:2 * n_counts + F], buf[2 * n_counts + F:2 * n_counts + 2 * F]
        edge_counts = buf[2 * n_counts + 2 * F:] if ids is not None else None
        ws = torch.empty(workspace_bytes(F, h, w), device=dev, dtype=torch.uint8)
        st, A = _lib.stream_ptr(dev), _lib.score_api()
        d2 = _distance(g, gt_threshold, ws)
        A.score_stats(p, _lib.SCORE_MAPS_DTYPES[p.dtype], pred_threshold, d2, ids, n_ids or 0, taus, K, F, h, w, counts_p, sums_p, edge_counts, st)
        d2 = _distance(p, pred_threshold, ws)
        A.score_stats(g, _lib.SCORE_MAPS_DTYPES[g.dtype], gt_threshold, d2, None, 0, taus, K, F, h, w, counts_g, sums_g, None, st)
        host = buf.cpu()                                                        # the one copy
    cp, cg = host[:n_counts].reshape(F, 1 + K).numpy(), host[n_counts:2 * n_counts].reshape(F, 1 + K).numpy()
    sp = host[2 * n_counts:2 * n_counts + F].view(torch.float64).numpy()
    sg = host[2 * n_counts + F:2 * n_counts + 2 * F].view(torch.float64).numpy()
    ec = host[2 * n_counts + 2 * F:].reshape(n_ids, 1 + K).numpy() if ids is not None else None
    return metrics_from_counts(cp, sp, cg, sg, ts, ec)


def score_parametric_edges(json_path_or_dict, meta_or_sampler, gt_edges=None, half_width=1.5, curve_segments=32, **score_kw):
    """What ``get_parametric_edge`` writes, scored in the views it was reconstructed from: ``rasterize_parametric_edges(...,
    return_ids=True)`` against ``gt_edges`` (F, H, W[, 1]) - or, for a ``DeviceRaySampler`` and no ``gt_edges``, against the sampler's own
    device-resident maps; nothing goes through the host.  -> the dict of ``score_edge_maps`` with ``edge_pixels`` / ``edge_support_t``
    per edge, lines first, then curves (the order of ``edge_raster``).  ``score_kw``: ``thresholds_px``, ``pred_threshold``,
    ``gt_threshold``, ``device``."""
    unknown = set(score_kw) - {"thresholds_px", "pred_threshold", "gt_threshold", "device"}
    if unknown:
        raise TypeError(f"score_parametric_edges: unexpected keyword(s) {sorted(unknown)}")
    _thresholds_px(score_kw.get("thresholds_px", (1.0, 2.0, 4.0)))
    for k in ("pred_threshold", "gt_threshold"):
        _threshold(score_kw.get(k, 0.5), k)
    d = _inputs.load_edge_dict(json_path_or_dict)
    n_ids = len(d["lines_end_pts"]) + len(d["curves_ctl_pts"])
    if n_ids < 1:
        raise ValueError("edge_score: score_parametric_edges needs at least one line or curve")
    device = score_kw.pop("device", "cuda")
    if gt_edges is None:
        if isinstance(meta_or_sampler, dict):
            raise ValueError("edge_score: score_parametric_edges needs gt_edges with a meta dict (a DeviceRaySampler brings its own maps)")
        gt_edges, device = meta_or_sampler._edges, meta_or_sampler.device
    elif isinstance(gt_edges, torch.Tensor):
        device = gt_edges.device
    h, w = edge_raster.meta_cameras(meta_or_sampler)[2:]
    n_views = len(meta_or_sampler["frames"]) if isinstance(meta_or_sampler, dict) else int(meta_or_sampler.n_images)
    if not hasattr(gt_edges, "shape"):
        gt_edges = np.asarray(gt_edges)
    if tuple(gt_edges.shape) not in ((n_views, h, w), (n_views, h, w, 1)):
        raise ValueError(f"edge_score: gt_edges must be ({n_views}, {h}, {w}) or ({n_views}, {h}, {w}, 1), got {tuple(gt_edges.shape)}")
    pred, ids = edge_raster.rasterize_parametric_edges(d, meta_or_sampler, half_width=half_width, curve_segments=curve_segments,
                                                       return_ids=True, device=device)
    return score_edge_maps(pred, gt_edges, ids=ids, n_ids=n_ids, device=device, **score_kw)


def score_rendered_views(renderer, sampler, views, pred_threshold=0.5, **kw):
    """The held-out-view score: ``validation.render_view(renderer, sampler, v, to_numpy=False)`` for every v of ``views`` at
    ``resolution_level=1``, the rendered ``edge`` reshaped to (H, W), scored against the sampler's maps of those views.  -> the dict of
    ``score_edge_maps`` (frame i is ``views[i]``).  ``kw``: ``thresholds_px`` and ``gt_threshold`` go to the score, everything else
    (``launch_rays``, ``batch_size``, ``cos_anneal_ratio``, ``background_rgb``, ``near``, ``far``) to ``render_view``."""
    level = kw.pop("resolution_level", 1)
    if level != 1:
        raise ValueError(f"edge_score: score_rendered_views renders at resolution_level=1 only (got {level!r})")
    score_kw = {k: kw.pop(k) for k in ("thresholds_px", "gt_threshold") if k in kw}
    _thresholds_px(score_kw.get("thresholds_px", (1.0, 2.0, 4.0)))
    _threshold(score_kw.get("gt_threshold", 0.5), "gt_threshold")
    pred_threshold = _threshold(pred_threshold, "pred_threshold")
    views = [int(v) for v in views]
    if not views or not all(0 <= v < sampler.n_images for v in views):
        raise ValueError(f"edge_score: views must be a non-empty list of image ids in [0, {sampler.n_images}), got {views}")
    H, W = int(sampler.H), int(sampler.W)
    pred = torch.stack([validation.render_view(renderer, sampler, v, resolution_level=1, to_numpy=False, **kw)["edge"].reshape(H, W) for v in views])
    gt = sampler._edges[torch.as_tensor(views, device=sampler.device)]
    return score_edge_maps(pred.float(), gt, pred_threshold=pred_threshold, device=sampler.device, **score_kw)


def filter_edges_by_support(edge_dict, edge_support, min_support=0.5):
    """The ``parametric_edges.json`` dict without the lines and curves whose support - ``edge_support_t`` of ``score_parametric_edges``,
    one value per edge, lines first, then curves - is below ``min_support`` or NaN.  Other keys are passed through; the input is not
    changed."""
    lines, curves = list(edge_dict["lines_end_pts"]), list(edge_dict["curves_ctl_pts"])
    s = np.asarray(edge_support, dtype=np.float64)
    if s.shape != (len(lines) + len(curves),):
        raise ValueError(f"edge_score: edge_support must be ({len(lines) + len(curves)},) - one per line, then one per curve -, got {s.shape}")
    keep = s >= float(min_support)                # a NaN compares false
    out = dict(edge_dict)
    out["lines_end_pts"] = [e for e, k in zip(lines, keep[:len(lines)]) if k]
    out["curves_ctl_pts"] = [e for e, k in zip(curves, keep[len(lines):]) if k]
    return out
