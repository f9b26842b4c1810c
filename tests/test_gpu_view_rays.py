"""GPU tests (-m gpu) of the full-image ray generation (emap_gen_rays_at: DeviceRaySampler.gen_rays_at / rays_at_flat,
validation.render_view, the drop-in's Dataset.gen_rays_at) against tests/golden/g20_view_rays.npz - the reference's own
``Dataset.gen_rays_at`` (src/dataset/dataset.py:137-167) on three cameras at resolution levels 1, 2, 3 and 5.

Tolerance of the ray directions and depth_scale: 2e-6 * max(1, max|reference|) absolute - the bound tests/test_ray_sampler.py
(test_device_sampler_vs_reference_golden, g11) applies to the random sampler's ray directions; the camera arithmetic is the same.
rays_o, pose and intrinsics are copies of inputs: bit-equal."""
import numpy as np
import pytest
import torch

from conftest import load_golden, net_state
import emap_amd
from emap_amd import dropin
from emap_amd.validation import render_image, render_view, to_images
from test_view_rays_cpu import LEVELS, view_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIR_TOL = 2e-6            # tests/test_ray_sampler.py:64

G = load_golden("g20_view_rays")
CASES = view_cases(G)
_samplers = {}


def sampler(W, H):
    """One DeviceRaySampler per image size over the fixture's three cameras (edge maps play no part in a view's rays)."""
    if (W, H) not in _samplers:
        _samplers[(W, H)] = emap_amd.DeviceRaySampler(torch.zeros(3, H, W), torch.from_numpy(G["intrinsics_all"]), torch.from_numpy(G["pose_all"]),
                                                      device=DEV, near=float(G["near"]), far=float(G["far"]))
    return _samplers[(W, H)]


def check_against_golden(out, W, H, cam, l):
    """`out`, a gen_rays_at 5-tuple, against the reference's for camera `cam` of the W x H view at level l."""
    tag = f"{W}x{H}.cam{cam}.l{l}"
    rays_o, rays_v, pose, intrinsics, depth_scale = out
    want = {k: torch.from_numpy(G[f"{tag}.{k}"]) for k in ("rays_o", "rays_v", "pose", "intrinsics", "depth_scale")}
    h, w = H // l, W // l
    assert rays_o.shape == (h, w, 3) and rays_v.shape == (h, w, 3) and pose.shape == (4, 4) and intrinsics.shape == (4, 4)
    assert depth_scale.shape == (w, h, 1)                                        # the reference does not transpose it (:152, :166)
    for k, got in (("rays_o", rays_o), ("rays_v", rays_v), ("pose", pose), ("intrinsics", intrinsics), ("depth_scale", depth_scale)):
        assert got.shape == want[k].shape and got.device == torch.device(DEV) and got.dtype == torch.float32, k
    assert torch.equal(pose.cpu(), want["pose"]) and torch.equal(intrinsics.cpu(), want["intrinsics"])
    assert torch.equal(rays_o.cpu(), want["rays_o"])
    for k, got in (("rays_v", rays_v), ("depth_scale", depth_scale)):
        err = float((got.cpu() - want[k]).abs().max())
        bound = DIR_TOL * max(1.0, float(want[k].abs().max()))
        print(f"{tag} {k}: max abs error {err:.3e} (bound {bound:.1e})")
        assert err <= bound, (tag, k, err)
    # the scale of a ray sits at the transposed index of the quirky layout
    assert torch.equal(depth_scale.transpose(0, 1).reshape(-1), sampler(W, H).rays_at_flat(cam, l)[2].reshape(-1))


@pytest.mark.parametrize("W,H,cam", CASES)
@pytest.mark.parametrize("l", LEVELS)
def test_gen_rays_at_vs_reference_golden(W, H, cam, l):
    check_against_golden(sampler(W, H).gen_rays_at(cam, l), W, H, cam, l)


@pytest.mark.parametrize("W,H,cam,l", [(37, 23, 0, 1), (37, 23, 2, 3), (64, 48, 1, 1), (64, 48, 1, 5)])
def test_chunks_are_bit_identical_to_the_single_call(W, H, cam, l):
    s = sampler(W, H)
    n = s.view_size(l)[0]
    whole = [x.clone() for x in s.rays_at_flat(cam, l)]
    assert [tuple(x.shape) for x in whole] == [(n, 3), (n, 3), (n, 1)]
    buf = torch.empty(7 * n + 5, device=DEV)                                      # a reused, larger buffer
    for chunk in (1, 63, 64, 65, n):
        parts = [[], [], []]
        for first in range(0, n, chunk):                                          # the last chunk is ragged unless chunk divides n
            out = s.rays_at_flat(cam, l, first, min(chunk, n - first), out=buf)
            assert out[0].data_ptr() == buf.data_ptr()
            for p, x in zip(parts, out):
                p.append(x.clone())
        for k, (p, w) in enumerate(zip(parts, whole)):
            assert torch.equal(torch.cat(p), w), (chunk, k)
    tail = s.rays_at_flat(cam, l, n - 7)                                          # count=None: to the end of the view
    assert all(torch.equal(a, b[n - 7:]) for a, b in zip(tail, whole))
    assert s.rays_at_flat(cam, l, n, 0)[0].shape == (0, 3)
    for first, count in ((n - 3, 4), (0, n + 1), (n + 1, 0), (-1, 2), (0, -1)):
        with pytest.raises(ValueError):
            s.rays_at_flat(cam, l, first, count)
    with pytest.raises(ValueError):
        s.rays_at_flat(cam, l, 0, 8, out=torch.empty(55, device=DEV))             # 7 * 8 floats are needed
    with pytest.raises(IndexError):
        s.gen_rays_at(3, l)
    with pytest.raises(RuntimeError, match="gen_rays_count"):
        s.gen_rays_at(cam, 0)


def test_image_perm_selects_the_permuted_camera():
    """With the runner's image permutation set, position k of it (``via_perm``) is looked up on the device: the rays, pose and
    intrinsics are those of golden camera perm[k]; a plain index still means the image itself."""
    W, H = 37, 23
    s = emap_amd.DeviceRaySampler(torch.zeros(3, H, W), torch.from_numpy(G["intrinsics_all"]), torch.from_numpy(G["pose_all"]), device=DEV)
    for k in range(4):                                                            # no permutation: position k is image k % 3
        check_against_golden(s.gen_rays_at(k, 2, via_perm=True), W, H, k % 3, 2)
    perm = [2, 0, 1]
    s.set_image_perm(perm)
    for k in range(5):
        for l in (1, 3):
            check_against_golden(s.gen_rays_at(k, l, via_perm=True), W, H, perm[k % 3], l)
    check_against_golden(s.gen_rays_at(1, 1), W, H, 1, 1)


def test_render_view_is_bit_identical_to_render_image_on_the_same_rays():
    """render_view generates each launch chunk's rays on the device and renders it; render_image is handed the rays of gen_rays_at in
    full - rays_o and rays_v as returned, depth_scale transposed back to the rays' (H, W) order, every ray with its OWN scale (the
    reference's validate pairs ray i with the scale at flat index i of the un-transposed array; render_view does not reproduce that).
    Same launch chunks, same kernels, same inputs: every returned entry is bit-identical."""
    W, H, cam = 37, 23, 0
    kw, state = net_state("d4w128L10")
    net = emap_amd.UDFNetwork(scale=1.0, precision="f16x3", **kw)
    net.load_state_dict(state)
    net = net.to(DEV)
    r = emap_amd.UDFRendererBlending(None, net, emap_amd.SingleVarianceNetwork(0.3).to(DEV),
                                     emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(DEV), 32, 32, 0, 4, 0.0, device=DEV)
    s = sampler(W, H)
    assert H * W == 851
    rays_o, rays_v, _, _, depth_scale = s.gen_rays_at(cam)
    for launch_rays in (64, 851, None):
        want = render_image(r, rays_o, rays_v, s.near, s.far, depth_scale.transpose(0, 1), batch_size=512, cos_anneal_ratio=1.0,
                            launch_rays=launch_rays)
        got = render_view(r, s, cam, launch_rays=launch_rays, cos_anneal_ratio=1.0)
        assert sorted(got) == sorted(want) == ["depth", "edge", "normals"]
        for k in want:
            assert isinstance(got[k], np.ndarray) and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (launch_rays, k)
        assert np.isfinite(got["edge"]).all() and float(np.abs(got["depth"]).max()) > 0
    edge, depth, normals = to_images(got, H, W)
    assert edge.shape == (23, 37) and edge.dtype == np.uint8 and depth.shape == (23, 37) and normals.shape == (23, 37, 3)
    dev_res = render_view(r, s, cam, launch_rays=64, cos_anneal_ratio=1.0, to_numpy=False)
    assert all(v.is_cuda and np.array_equal(v.cpu().numpy(), got[k]) for k, v in dev_res.items())
    # a lower resolution level, chunked: the same as render_image on that level's rays
    ro3, rv3, _, _, ds3 = s.gen_rays_at(cam, 3)
    want3 = render_image(r, ro3, rv3, s.near, s.far, ds3.transpose(0, 1), batch_size=512, cos_anneal_ratio=1.0, launch_rays=50)
    got3 = render_view(r, s, cam, 3, launch_rays=50, cos_anneal_ratio=1.0)
    assert got3["edge"].shape == (7 * 12, 1) and all(np.array_equal(got3[k], want3[k]) for k in want3)
    # a renderer that perturbs needs the reference's batch_size for the order of its jitter draws - and then draws what render_image draws
    r.perturb = 1.0
    with pytest.raises(ValueError, match="batch_size"):
        render_view(r, s, cam, cos_anneal_ratio=1.0)
    torch.manual_seed(5)
    want_p = render_image(r, rays_o, rays_v, s.near, s.far, depth_scale.transpose(0, 1), batch_size=300, cos_anneal_ratio=1.0, launch_rays=256)
    torch.manual_seed(5)
    got_p = render_view(r, s, cam, launch_rays=256, batch_size=300, cos_anneal_ratio=1.0)
    assert all(np.array_equal(got_p[k], want_p[k]) for k in want_p) and not np.array_equal(got_p["edge"], got["edge"])
    with pytest.raises(ValueError, match="near"):
        render_view(r, emap_amd.DeviceRaySampler(torch.zeros(3, H, W), torch.from_numpy(G["intrinsics_all"]), torch.from_numpy(G["pose_all"]),
                                                 device=DEV), cam)


def test_dropin_dataset_method_returns_the_samplers_tensors():
    W, H = 64, 48

    class Dataset:                                                                # attribute names of the reference's Dataset (dataset.py:86-135)
        def __init__(self):
            self.edges = torch.zeros(3, H, W, 1)
            self.intrinsics_all, self.pose_all = torch.from_numpy(G["intrinsics_all"]), torch.from_numpy(G["pose_all"])
            self.device = torch.device(DEV)

        def gen_rays_at(self, img_idx, resolution_level=1):
            raise AssertionError("the host routine must have been replaced")

    Dataset.gen_rays_at = dropin.dataset_view_method(original=Dataset.gen_rays_at)
    ds = Dataset()
    for l in (1, 5):
        got = ds.gen_rays_at(1, resolution_level=l)
        want = sampler(W, H).gen_rays_at(1, l)
        assert len(got) == 5 and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(got, want))
        check_against_golden(got, W, H, 1, l)
    assert isinstance(ds._emap_sampler, emap_amd.DeviceRaySampler)
