"""Parametric edges back into image space: 3D line segments and cubic Beziers drawn into the edge maps of a camera list, on the device.

The map EMAP's input lives in.  ``rasterize_edges`` is ONE call of ``emap_raster_edges`` (csrc/raster.hip, include/emap_raster_hip.h, where
the semantics are stated): a launch that projects every (frame, segment) into a table in the workspace and a launch that gathers from it,
one workgroup per frame and tile of pixels, and stores every byte once.  The pixel formula is that of
``synthetic.make_wireframe_scene`` - distance to the projected segment, ``clip(half_width - d, 0, 1)``, the maximum over segments,
``rint(255 v)`` - so for that scene's segments and cameras the bytes are the generator's, bit for bit; curves are drawn as
``curve_segments`` chords.  All fp64 without FMA contraction: the same bits on every run (tests/edge_raster_ref.py is the numpy mirror).

EDGE e < L is line e, edge L + j is curve j: the order of the two list arguments, and the order ``weights`` and the ids follow.  Cameras are
what ``parametric_edges.compute_visibility`` and ``dtu_eval`` take: ``intrinsics_list`` (F, 4, 4) or (F, 3, 3), ``camtoworld_list``
(F, 4, 4), K, R and T formed on the host by ``_inputs.world_to_camera``.  There is no occlusion: the scene has no surfaces.

numpy inputs go to ``device``; tensors are used where they are.  There is no CPU fallback: without a GPU the calls raise ``RuntimeError``.
"""
import numpy as np
import torch

from . import _inputs, _lib, synthetic

RASTER_TILE_W = 64         # csrc/raster.hip: RASTER_TILE_W
RASTER_TILE_H = 16         # csrc/raster.hip: RASTER_TILE_H
RASTER_LIST_CHUNK = 256    # segments of a tile that sit in LDS at a time     (csrc/raster.hip: RASTER_LIST_CHUNK)


def _edges(a, per_edge, name, device, tag="edge_raster"):
    """(n, per_edge) contiguous fp64 tensor from (n, per_edge // 3, 3), (n, per_edge) or an empty list; finite.  ``tag`` names the calling
    module in the error (edge_field takes its edges through here too)."""
    t = _inputs.to_device(a, "cpu")                # numpy and lists are checked on the host and go to ``device`` last
    if t.numel() == 0:
        t = t.reshape(0, per_edge)
    if t.dim() == 3 and tuple(t.shape[1:]) == (per_edge // 3, 3):
        t = t.reshape(-1, per_edge)
    if t.dim() != 2 or t.shape[1] != per_edge:
        raise ValueError(f"{tag}: {name} must be (n, {per_edge // 3}, 3) or (n, {per_edge}), got {tuple(a.shape) if hasattr(a, 'shape') else np.shape(a)}")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{tag}: {name} holds a non-finite value")
    return (t if isinstance(a, torch.Tensor) else t.to(device)).contiguous()


def cameras(intrinsics_list, camtoworld_list):
    """intr (F, 4) = fx, fy, cx, cy; R (F, 3, 3), T (F, 3): fp64 numpy, each view checked and then taken through ``_inputs.world_to_camera``."""
    F = len(intrinsics_list)
    if F == 0 or len(camtoworld_list) != F:
        raise ValueError(f"edge_raster: {F} intrinsics, {len(camtoworld_list)} poses (one of each per view, at least one view)")
    if F > _lib.RASTER_MAX_FRAMES:
        raise ValueError(f"edge_raster: {F} views, at most {_lib.RASTER_MAX_FRAMES} per call")
    intr, R, T = np.empty((F, 4), dtype=np.float64), np.empty((F, 3, 3), dtype=np.float64), np.empty((F, 3), dtype=np.float64)
    for i, (k, c) in enumerate(zip(intrinsics_list, camtoworld_list)):
        k, c = _inputs.host64(k), _inputs.host64(c)
        if k.shape not in ((3, 3), (4, 4)) or c.shape != (4, 4):
            raise ValueError(f"edge_raster: view {i}: intrinsics must be (3, 3) or (4, 4) and camtoworld (4, 4), got {k.shape} and {c.shape}")
        if not (np.isfinite(k).all() and np.isfinite(c).all()):
            raise ValueError(f"edge_raster: view {i}: non-finite camera")
        K = k[:3, :3]                                   # what world_to_camera returns as K
        if K[0, 1] != 0 or K[1, 0] != 0 or tuple(K[2]) != (0.0, 0.0, 1.0):
            raise ValueError(f"edge_raster: view {i}: intrinsics must have no skew and the last row (0, 0, 1)")
        intr[i] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        try:                                            # one view at a time, so that the error names the view
            _, R[i:i + 1], T[i:i + 1] = _inputs.world_to_camera([k], [c])
        except np.linalg.LinAlgError as e:
            raise ValueError(f"edge_raster: view {i}: camtoworld has no inverse") from e
    if not (np.isfinite(R).all() and np.isfinite(T).all()):
        raise ValueError("edge_raster: a camtoworld matrix has no finite inverse")
    return intr, R, T


def workspace_bytes(n_lines, n_curves, curve_segments, F):
    """What ``emap_raster_workspace_bytes`` reports: ``F * (n_lines + n_curves * curve_segments) * _lib.RASTER_ROW_BYTES``."""
    n = _lib.C.c_size_t()
    _lib.raster_api().raster_workspace_bytes(int(n_lines), int(n_curves), int(curve_segments), int(F), n)
    return n.value


def rasterize_edges(lines_end_pts, curves_ctl_pts, intrinsics_list, camtoworld_list, h, w, half_width=1.5, weights=None, curve_segments=32,
                    z_near=1e-3, return_ids=False, device="cuda"):
    """Draw L segments ``lines_end_pts`` (L, 2, 3) or (L, 6) and C cubic Beziers ``curves_ctl_pts`` (C, 4, 3) or (C, 12) - either may be
    empty - into the F views: -> bytes (F, h, w) uint8 on the device, with ``return_ids`` also ids (F, h, w) int32, the lowest edge index
    that attains the pixel's maximum and -1 where nothing is drawn.  ``weights`` (L + C) in [0, 1] scale the edges (default 1);
    ``half_width`` in (0, 64] pixels is where the profile ``clip(half_width - d, 0, 1)`` reaches 0; a curve is ``curve_segments`` in
    [1, 256] chords; a segment is clipped at the camera depth ``z_near``.  At most 2**20 segments per call.  The only allocations are the
    outputs and the workspace; one call, no synchronisation, the same bits on every run."""
    h, w, curve_segments = int(h), int(w), int(curve_segments)
    half_width, z_near = float(half_width), float(z_near)
    if not (1 <= h <= _lib.RASTER_MAX_DIM and 1 <= w <= _lib.RASTER_MAX_DIM):
        raise ValueError(f"edge_raster: h and w must be in [1, {_lib.RASTER_MAX_DIM}], got {h} x {w}")
    if not (0.0 < half_width <= _lib.RASTER_MAX_HALF_WIDTH):
        raise ValueError(f"edge_raster: half_width must be in (0, {_lib.RASTER_MAX_HALF_WIDTH:g}], got {half_width}")
    if not (1 <= curve_segments <= _lib.RASTER_MAX_CURVE_SEGMENTS):
        raise ValueError(f"edge_raster: curve_segments must be in [1, {_lib.RASTER_MAX_CURVE_SEGMENTS}], got {curve_segments}")
    if not (0.0 < z_near < float("inf")):
        raise ValueError(f"edge_raster: z_near must be finite and > 0, got {z_near}")
    lines = _edges(lines_end_pts, 6, "lines_end_pts", device)
    curves = _edges(curves_ctl_pts, 12, "curves_ctl_pts", device)
    L, Cn = int(lines.shape[0]), int(curves.shape[0])
    if L + Cn * curve_segments > _lib.RASTER_MAX_SEGMENTS:
        raise ValueError(f"edge_raster: {L} lines and {Cn} curves of {curve_segments} segments are more than {_lib.RASTER_MAX_SEGMENTS} segments")
    intr, R, T = cameras(intrinsics_list, camtoworld_list)
    F = len(intr)
    if weights is not None:
        wt = _inputs.to_device(weights, "cpu")          # as _edges: checked where it is
        if wt.dim() != 1 or wt.shape[0] != L + Cn:
            raise ValueError(f"edge_raster: weights must be ({L + Cn},) - one per line, then one per curve -, got {tuple(wt.shape)}")
        if not bool(((wt >= 0) & (wt <= 1)).all()):
            raise ValueError("edge_raster: weights must lie in [0, 1]")
        wt = (wt if isinstance(weights, torch.Tensor) else wt.to(device)).contiguous()
    else:
        wt = None
    dev = lines.device
    _lib.require_cuda(lines, "lines_end_pts")
    _lib.require_cuda(curves, "curves_ctl_pts")
    if curves.device != dev or (wt is not None and wt.device != dev):
        raise ValueError(f"edge_raster: lines are on {dev}, curves on {curves.device}" + ("" if wt is None else f", weights on {wt.device}"))
    cams = torch.as_tensor(np.concatenate([intr.reshape(-1), R.reshape(-1), T.reshape(-1)])).to(dev)      # one small copy: (F, 16) doubles
    intr_d, R_d, T_d = cams[:4 * F], cams[4 * F:13 * F], cams[13 * F:]
    out = torch.empty((F, h, w), device=dev, dtype=torch.uint8)
    ids = torch.empty((F, h, w), device=dev, dtype=torch.int32) if return_ids else None
    with _lib.on_device(lines):
        nbytes = workspace_bytes(L, Cn, curve_segments, F)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8) if nbytes else None
        _lib.raster_api().raster_edges(lines if L else None, L, curves if Cn else None, Cn, curve_segments, wt, intr_d, R_d, T_d, F, h, w,
                                       half_width, z_near, out, ids, ws, nbytes, _lib.stream_ptr(dev))
    return (out, ids) if return_ids else out


def meta_cameras(meta_or_sampler):
    """(intrinsics (F, 4, 4), camtoworld (F, 4, 4), h, w) of a parsed ``meta_data.json`` or of a ``DeviceRaySampler``."""
    if isinstance(meta_or_sampler, dict):
        frames = meta_or_sampler["frames"]
        return ([np.asarray(f["intrinsics"], dtype=np.float64) for f in frames], [np.asarray(f["camtoworld"], dtype=np.float64)[:4, :4] for f in frames],
                int(meta_or_sampler["height"]), int(meta_or_sampler["width"]))
    s = meta_or_sampler
    return list(_inputs.host64(s.intrinsics_all)), list(_inputs.host64(s.pose_all)), int(s.H), int(s.W)


def rasterize_parametric_edges(json_path_or_dict, meta_or_sampler, half_width=1.5, weights=None, curve_segments=32, z_near=1e-3,
                               return_ids=False, device="cuda"):
    """What ``get_parametric_edge`` writes (a ``parametric_edges.json`` path or its dict: ``lines_end_pts`` (L, 6), ``curves_ctl_pts``
    (C, 12)) drawn into the views it was reconstructed from: the cameras of a parsed ``meta_data.json`` dict, or of the
    ``DeviceRaySampler`` built from one.  -> what ``rasterize_edges`` returns, at the dataset's height and width."""
    d = _inputs.load_edge_dict(json_path_or_dict)
    intrinsics, poses, h, w = meta_cameras(meta_or_sampler)
    return rasterize_edges(d["lines_end_pts"], d["curves_ctl_pts"], intrinsics, poses, h, w, half_width=half_width, weights=weights,
                           curve_segments=curve_segments, z_near=z_near, return_ids=return_ids, device=device)


_BYTE_TABLE = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)      # float32(b / 255.0), in IEEE doubles on the host


def to_dataset_edges(bytes_):
    """(F, h, w) uint8 -> (F, h, w, 1) float32 ``float32(b / 255.0)``, the format of ``DeviceRaySampler`` and ``make_wireframe_scene``
    (``cv.imread(..., 0) / 255``), through a 256-entry table computed on the host.  A tensor stays on its device; numpy gives numpy."""
    if isinstance(bytes_, torch.Tensor):
        if bytes_.dtype != torch.uint8 or bytes_.dim() != 3:
            raise ValueError(f"edge_raster: to_dataset_edges takes (F, h, w) uint8, got {tuple(bytes_.shape)} {bytes_.dtype}")
        table = torch.as_tensor(_BYTE_TABLE).to(bytes_.device)
        return table[bytes_.to(torch.int64)].unsqueeze(-1)
    b = np.asarray(bytes_)
    if b.dtype != np.uint8 or b.ndim != 3:
        raise ValueError(f"edge_raster: to_dataset_edges takes (F, h, w) uint8, got {b.shape} {b.dtype}")
    return _BYTE_TABLE[b][..., None]


def make_parametric_scene(lines, curves, n_images=16, H=200, W=200, radius=3.0, fov_deg=30.0, half_width=1.5, curve_segments=32,
                          device="cuda"):
    """A multi-view consistent synthetic dataset of parametric edges, lines AND curves: ``(meta, edges)`` in the wire format of
    ``synthetic.make_wireframe_scene`` - the ``meta`` of ``synthetic.ring_cameras`` and (n_images, H, W, 1) float32 numpy edge maps in
    [0, 1] -, the maps rasterised on the device.  For ``synthetic.wireframe_segments()`` and no curves both are make_wireframe_scene's,
    bit for bit."""
    meta = synthetic.ring_cameras(n_images, H, W, radius, fov_deg)
    intrinsics, poses, h, w = meta_cameras(meta)
    maps = rasterize_edges(lines, curves, intrinsics, poses, h, w, half_width=half_width, curve_segments=curve_segments, device=device)
    return meta, to_dataset_edges(maps).cpu().numpy()
