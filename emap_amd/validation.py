"""Full-image rendering (SURVEY par. 8 f4): the render loop of ``Runner_UDF.validate`` (src/runner/runner_udf.py:297-407).

The reference splits the H*W rays of an image into ``batch_size`` chunks, calls ``renderer.render`` per chunk and copies
``edge``, ``depth`` and the weighted normal ``sum_s gradients_flip * weights`` of every chunk to the host (three
``.detach().cpu().numpy()`` round trips per chunk).  Here the same quantities are produced by ONE ``emap_render_fwd`` call over all
H*W rays (round 6; ``launch_rays=None``: up to 2**18 rays per call - every kernel of the path strides over its ray / point tiles
with a resident grid, so a 400 x 400 image is one chain of 10 launches instead of 20 chains of 5; rounds 1-5: 8192 rays per call)
in the renderer's REDUCED output mode - the compositing kernel is handed NULL
for every per-sample output and writes only edge, depth, the weighted normal and weight_sum: 28 B per ray instead of the
48 B per sample of the training dict - stay on the device and are copied to the host once.  The per-chunk jitter
draws of the reference (``torch.rand([chunk, 1])`` on the CPU generator, udf_renderer_blending.py:719) are reproduced in the
same order, so with the same seed the image is the reference's image.  Rays are independent, so the result does not depend
on how they are grouped into launches (tests/test_gpu_parity.py::test_image_render_is_chunk_invariant).
``render_view`` is the same loop for a view of a ``DeviceRaySampler``: each launch chunk's rays are generated on the device.
"""
import numpy as np
import torch


def default_launch_rays(S):
    """Rays per render call of ``render_image(launch_rays=None)`` at S samples per ray: 2**18 up to S = 256 - one call for any image up
    to 512 x 512; the workspace of a call is ~2 KiB per ray at S = 128 and grows linearly in S - and beyond that 2**18 * 256 / S rounded
    down to a power of two, which keeps a call's workspace at most what it is at S = 256."""
    if S <= 256:
        return 1 << 18
    n = (1 << 18) * 256 // S
    return 1 << (n.bit_length() - 1)


def render_image(renderer, rays_o, rays_d, near, far, depth_scale, batch_size, cos_anneal_ratio=None, background_rgb=None,
                 launch_rays=None, to_numpy=True):
    """rays_o, rays_d (H,W,3) or (n,3); depth_scale (H,W,1) or (n,1).  Returns {"edge": (n,1), "depth": (n,1),
    "normals": (n,3)} as numpy arrays (the lists ``out_edge_fine / out_depth / out_normal_fine`` of the reference, concatenated)."""
    ro = rays_o.reshape(-1, 3)
    rd = rays_d.reshape(-1, 3)
    ds = depth_scale.reshape(-1, 1)
    n = ro.shape[0]
    if launch_rays is None:
        launch_rays = default_launch_rays(renderer.samples_per_ray)
    def chunk(t):
        nr = near[t] if isinstance(near, torch.Tensor) and near.numel() > 1 else near
        fr = far[t] if isinstance(far, torch.Tensor) and far.numel() > 1 else far
        return ro[t], rd[t], ds[t], nr, fr
    return _render_chunks(renderer, chunk, n, ro.device, batch_size, cos_anneal_ratio, background_rgb, launch_rays, to_numpy)


def _render_chunks(renderer, chunk, n, dev, batch_size, cos_anneal_ratio, background_rgb, launch_rays, to_numpy):
    """The launch loop of render_image / render_view: ``chunk(slice)`` -> (rays_o, rays_d, depth_scale, near, far) of those rays."""
    # jitter: one draw per reference chunk, in the reference's order (render() :718-720 with perturb_overwrite = -1)
    t_rand = None
    if renderer.perturb > 0:
        t_rand = torch.cat([torch.rand([min(batch_size, n - h), 1]) - 0.5 for h in range(0, n, batch_size)]) if n else torch.zeros(0, 1)
    edge, depth, normals = [], [], []
    with torch.no_grad():
        for h in range(0, n, launch_rays):
            t = slice(h, min(h + launch_rays, n))
            ro, rd, ds, nr, fr = chunk(t)
            out = renderer.render_reduced(ro, rd, nr, fr, depth_scale=ds, cos_anneal_ratio=cos_anneal_ratio,
                                          background_rgb=background_rgb, perturb_overwrite=-1 if t_rand is not None else 0,
                                          t_rand=None if t_rand is None else t_rand[t])
            edge.append(out["edge"])
            depth.append(out["depth"])
            normals.append(out["normals"])        # = (gradients_flip * weights[:, :S, None]).sum(1), render_core :662
    cat = lambda xs, w: torch.cat(xs) if xs else torch.zeros(0, w, device=dev)
    res = {"edge": cat(edge, 1), "depth": cat(depth, 1), "normals": cat(normals, 3)}
    if to_numpy:
        res = {k: v.detach().cpu().numpy() for k, v in res.items()}
    return res


def render_view(renderer, sampler, img_idx, resolution_level=1, launch_rays=None, batch_size=None, cos_anneal_ratio=None,
                background_rgb=None, near=None, far=None, to_numpy=True):
    """The whole view ``img_idx`` of a ``DeviceRaySampler`` at ``resolution_level`` - ``Dataset.gen_rays_at`` (dataset.py:137-167) and
    the render loop of ``Runner_UDF.validate`` as one native chain.  Per launch chunk the rays are GENERATED on the device into one reused
    buffer (``sampler.rays_at_flat``, 28 B per ray) and rendered in the reduced-output mode: the view's rays never exist in full, no ray
    is built on or copied from the host.  Returns what ``render_image`` returns for the rays of ``sampler.gen_rays_at`` in row-major
    (H // l, W // l) order with every ray's OWN depth_scale (``to_images(res, H // l, W // l)``).
    near / far default to the sampler's scene box; ``batch_size`` (the reference's chunk, which sets the order of the jitter draws) is
    needed only when the renderer perturbs."""
    near = sampler.near if near is None else near
    far = sampler.far if far is None else far
    if near is None or far is None:
        raise ValueError("render_view: the sampler carries no near / far (DeviceRaySampler.from_meta sets them): pass near= and far=")
    if renderer.perturb > 0 and batch_size is None:
        raise ValueError("render_view: the renderer perturbs its samples: pass the reference's batch_size (it orders the jitter draws)")
    n = sampler.view_size(resolution_level)[0]
    if launch_rays is None:
        launch_rays = default_launch_rays(renderer.samples_per_ray)
    buf = torch.empty(7 * min(launch_rays, n), dtype=torch.float32, device=sampler.device)

    def chunk(t):
        return sampler.rays_at_flat(img_idx, resolution_level, t.start, t.stop - t.start, out=buf) + (near, far)
    return _render_chunks(renderer, chunk, n, sampler.device, batch_size, cos_anneal_ratio, background_rgb, launch_rays, to_numpy)


def to_images(res, H, W):
    """The reference's post-processing of the concatenated lists (runner_udf.py:409-440): edge*255 clipped to uint8 (H,W),
    depth (H,W), normals (H,W,3)."""
    edge = (np.asarray(res["edge"]).reshape(H, W) * 255).clip(0, 255).astype(np.uint8)
    return edge, np.asarray(res["depth"]).reshape(H, W), np.asarray(res["normals"]).reshape(H, W, 3)
