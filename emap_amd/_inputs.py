"""What the post-training wrappers (edge_metrics, parametric_edges, dtu_eval, edge_fitting, edge_raster) do to their arguments before a C
call, once: device placement, the host copy of a small matrix, the world-to-camera convention, the shape of the edge maps and the
``parametric_edges.json`` path-or-dict.  Private to the package; checks that only one module makes stay in that module.
"""
import json
import os

import numpy as np
import torch


def to_device(a, device, dtype=torch.float64, keep=()):
    """Contiguous tensor of ``dtype``: a tensor is detached and stays on its device - ``device`` is not consulted -, anything else (numpy, the
    json's nested lists) goes through ``np.asarray`` to ``device`` in one copy and is cast there.  A dtype in ``keep`` is left as it is."""
    t = a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).to(device)
    if t.dtype != dtype and t.dtype not in keep:
        t = t.to(dtype)
    return t.contiguous()


def points(a, device, tag, keep=(torch.float32,)):
    """``to_device`` for (n, 3) points: a dtype of ``keep`` stays, any other becomes the last of ``keep``; ``tag`` names the caller in the
    error."""
    t = to_device(a, device, keep[-1], keep)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{tag}: points must be (n, 3), got {tuple(t.shape)}")
    return t


def host64(a):
    """fp64 numpy array of a small matrix, whatever holds it: a tensor on any device, numpy, nested lists."""
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def world_to_camera(intrinsics_list, camtoworld_list):
    """K (F, 3, 3), R (F, 3, 3), T (F, 3), contiguous fp64 numpy: ``K = intrinsics[:3, :3]`` and ``[R | T] = np.linalg.inv(camtoworld)[:3]``,
    one ``inv`` per frame as the reference forms them, so that a point projects as ``K @ (R @ X + T)``.  ``intrinsics`` (4, 4) or (3, 3),
    ``camtoworld`` (4, 4); a singular pose raises ``np.linalg.LinAlgError``."""
    K = np.stack([host64(k)[:3, :3] for k in intrinsics_list])
    w2c = np.stack([np.linalg.inv(host64(c)) for c in camtoworld_list])
    return np.ascontiguousarray(K), np.ascontiguousarray(w2c[:, :3, :3]), np.ascontiguousarray(w2c[:, :3, 3])


def edge_maps(t, h, w, tag, nonempty=False):
    """(F, h, w) or (F, h, w, 1) tensor -> (F, h, w); ``tag`` names the caller and its argument in the error, ``nonempty`` asks for F > 0."""
    m = t[..., 0] if t.dim() == 4 and t.shape[3] == 1 else t
    if m.dim() != 3 or tuple(m.shape[1:]) != (int(h), int(w)) or (nonempty and m.shape[0] == 0):
        raise ValueError(f"{tag} must be (F, {h}, {w}) or (F, {h}, {w}, 1){' with F > 0' if nonempty else ''}, got {tuple(t.shape)}")
    return m


def load_edge_dict(path_or_dict):
    """The dict of a ``parametric_edges.json`` (``curves_ctl_pts``, ``lines_end_pts``): a path (``str``, ``os.PathLike``) is read, a dict is
    returned as it is."""
    if isinstance(path_or_dict, (str, os.PathLike)):
        with open(path_or_dict, "r") as f:
            return json.load(f)
    return path_or_dict
