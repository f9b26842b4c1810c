"""The random part of emap_sample_rays (csrc/rays.hip: pixels, uniform or edge-weighted; the jitter t_rand; the image of the step) against
its definition in numpy (tests/ray_draw_ref.py, from include/emap_hip.h), bit for bit: every comparison is integer or bit equality.

The scenes are the smallest at which each path exists: A 3 images of 20 x 30 (no power of two, both pixel classes), B four hand-built
6 x 5 images without edge pixels / with nothing else / with a single one, C one image of 2 x 4099.  Seeds, steps and batches are fixed
here; CASES lists every (scene, image, seed, step, batch, importance) a test below compares, and tests/test_ray_draw_cpu.py asserts for
each of them that no class decision of a weighted ray is closer to its threshold than a fused multiply-add could move it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import emap_amd
from emap_amd import _lib, synthetic
from ray_draw_ref import draw

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAIRS = [(5, 7), (0, 0), ((0x01234567 << 32) | 0x89ABCDEF, 2 ** 32 + 3), (9, 2 ** 40 + 12345)]   # (seed, step): k1, c[3], and the vector (0, 0, 0)
BATCHES = [1, 5, 63, 64, 65, 1023, 1024, 1025, 2049]                 # odd, the wave, the one-workgroup limit 1024, more than one 256-thread workgroup
BIG_STEP = 2 ** 32 + 3
RAY_KEYS = ("rays_o", "rays_v", "edge", "rays_ndc_uv", "rays_norm_XYZ_cam", "depth_scale")


# ---------------------------------------------------------------------------------------------- scenes and the mirror
@functools.lru_cache(maxsize=None)
def scene(name):
    """-> edges (n, H, W), intrinsics (n, 4, 4), poses (n, 4, 4).  Shared; read only."""
    if name == "A":
        meta, edges = synthetic.make_scene(n_images=3, H=20, W=30)
        K = torch.stack([torch.tensor(f["intrinsics"], dtype=torch.float32) for f in meta["frames"]])
        P = torch.stack([torch.tensor(f["camtoworld"], dtype=torch.float32) for f in meta["frames"]])
        return torch.from_numpy(edges)[..., 0], K, P
    if name == "B":
        e = torch.zeros(4, 5, 6)                                      # 0: ne = 0, d = 0
        e[1] = 1.0                                                    # 1: nn = 0, d = 1
        e[2] = 0.5                                                    # 2: nn = 0, d = 0.5
        e[3, 2, 4] = 1.0                                              # 3: ne = 1
    else:
        e = torch.zeros(1, 2, 4099)                                   # C: the minimum height, a wide rand_below range
        e[0, :, ::7] = 0.75
    eye = torch.eye(4).repeat(e.shape[0], 1, 1)
    return e, eye, eye.clone()


def sampler(name, device=DEV, seed=0):
    return emap_amd.DeviceRaySampler(*scene(name), device=device, seed=seed)


def expect(s, img, seed, step, batch, importance):
    """the mirror's draw, from what the sampler uploaded for `img` -> pixels, t_rand, margin"""
    return draw(seed, step, batch, s.W, s.H, importance, int(s._n_edge[img]), float(s._density[img]), s._order[img].cpu().numpy())


def train_image(seed, step, images):
    """the image set_train_images(images) selects at `step`"""
    from test_gpu_trainer_checkpoint import epoch_order
    return epoch_order(seed, step // len(images), images)[step % len(images)]


def _cases():
    c = [("A", k % 3, seed, step, b, imp) for k, (seed, step) in enumerate(PAIRS) for imp in (0, 1) for b in BATCHES]       # draw equals mirror
    c += [("A", 2, 5, 7, b, 1) for b in (65, 1025)]                                                                         # rays follow the pixels
    c += [("B", img, 11, 3, b, 1) for img in range(4) for b in (4, 1100)]                                                   # degenerate images
    c += [("C", 0, 13, 2, b, imp) for b in (64, 1100) for imp in (0, 1)] + [("C", 0, 13, st, 1100, 0) for st in range(8)]   # scene C
    c += [("A", 0, 5, 7, b, 0) for b in (1024, 2048)]                                                                       # launch shapes
    c += [("A", 1, 5, 2 ** 33 + 1, b, 1) for b in (64, 1100)]                                                               # the offset entry
    c += [("A", img, 5, BIG_STEP, 65, 1) for img in ([2, 0, 1][BIG_STEP % 3], train_image(5, BIG_STEP, [2, 0]))]            # image of the step
    c += [("A", 1, 9, BIG_STEP + 2 + k, 64, 1) for k in range(2)]                                                           # captured replay
    return c


CASES = _cases()


# ---------------------------------------------------------------------------------------------- helpers
def same_bits(a, b):
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    if a.dtype.is_floating_point:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def outputs(sample):
    return {**sample["rays"], **{k: sample[k] for k in RAY_KEYS[3:]}}


def run(s, img, step, batch, importance):
    """one launch at `step` through the sampler (the counter path); the counter must then read step + 1"""
    s._counter.fill_(step)
    o = s.gen_random_rays_patches_at(img, batch, importance_sample=bool(importance))
    torch.cuda.synchronize()
    assert int(s._counter.item()) == step + 1, (step, batch)
    return o


def assert_draw(o, want, what):
    pixels, t_rand, _ = want
    assert o["pixels"].dtype == torch.int64 and torch.equal(o["pixels"].cpu(), torch.from_numpy(pixels)), what
    assert same_bits(o["t_rand"], torch.from_numpy(t_rand)), what


def raw_sample(s, img, batch, importance, seed, offset, counter):
    """emap_sample_rays itself -> (rc, the batch under the keys of the sampler's dict)"""
    f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=DEV)
    b = {"rays_o": f32(batch, 3), "rays_v": f32(batch, 3), "edge": f32(batch), "depth_scale": f32(batch), "rays_ndc_uv": f32(batch, 2),
         "rays_norm_XYZ_cam": f32(batch, 3), "pixels": torch.empty(batch, 2, dtype=torch.int64, device=DEV),
         "img_idx": torch.empty(1, dtype=torch.int32, device=DEV), "t_rand": f32(batch)}
    out = _lib.RayBatch(*[v.data_ptr() for v in b.values()])          # the dict is in the struct's field order
    assert [k for k, _ in _lib.RayBatch._fields_] == ["rays_o", "rays_v", "edge", "depth_scale", "ndc_uv", "p_cam", "pixels", "img_idx", "t_rand"]
    with torch.cuda.device(DEV):
        rc = _lib.lib().emap_sample_rays(C.byref(s._ds), img, batch, importance, seed, offset, None if counter is None else counter.data_ptr(),
                                         None, C.byref(out), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, b


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("importance", [0, 1])
@pytest.mark.parametrize("pair", range(len(PAIRS)))
def test_draw_equals_mirror(pair, importance):
    """Pixels and jitter of every batch size at 32- and 64-bit seeds and steps == the definition; the counter reads step + 1."""
    seed, step = PAIRS[pair]
    img = pair % 3
    s = sampler("A", seed=seed)
    for batch in BATCHES:
        o = run(s, img, step, batch, importance)
        assert_draw(o, expect(s, img, seed, step, batch, importance), (seed, step, batch))
        assert int(o["img_idx"]) == img
        if (seed, step) == (0, 0):                                    # ray 0 is the published vector of key 0, counter 0: its word 2 is bc57ac4c
            assert float(o["t_rand"][0]) == float(0xBC57AC4C >> 8) * 2.0 ** -24 - 0.5


@pytest.mark.parametrize("batch", [65, 1025])
def test_rays_follow_the_drawn_pixels(batch):
    """The rays of a draw are the rays of its pixels: the given-pixel path, which the parity tests hold to the reference, returns the same bits."""
    s = sampler("A", seed=5)
    o = run(s, 2, 7, batch, 1)
    assert_draw(o, expect(s, 2, 5, 7, batch, 1), batch)
    g = s.gen_random_rays_patches_at(2, batch, pixels=o["pixels"].cpu())
    torch.cuda.synchronize()
    assert torch.equal(g["pixels"], o["pixels"])
    a, b = outputs(o), outputs(g)
    for k in RAY_KEYS:
        assert same_bits(a[k], b[k]), k


@pytest.mark.parametrize("img", range(4))
def test_degenerate_images(img):
    """No edge pixel, only edge pixels (density 1 and 0.5), a single edge pixel: the class decision (u < we and ne > 0) or nn == 0."""
    s = sampler("B", seed=11)
    ne = int(s._n_edge[img])
    assert (ne, float(s._density[img])) == ([0, 30, 30, 1][img], float(scene("B")[0][img].mean())) and float(s._density[2]) == 0.5
    for batch in (4, 1100):
        o = run(s, img, 3, batch, 1)                                  # raises unless the status is EMAP_OK
        want = expect(s, img, 11, 3, batch, 1)
        assert_draw(o, want, (img, batch))
        px = o["pixels"].cpu()
        assert torch.equal(o["rays"]["edge"].cpu().reshape(-1), scene("B")[0][img][px[:, 1], px[:, 0]])
        rc, b = raw_sample(s, img, batch, 1, 11, 3, None)
        assert rc == 0 and torch.equal(b["pixels"], o["pixels"])
        if img == 3:                                                  # the weighted rays of the edge class are the one edge pixel order[0]
            first = int(s._order[3, 0])
            assert first == 2 * 6 + 4
            in_class = np.isfinite(want[2]) & (want[0][:, 0] == first % 6) & (want[0][:, 1] == first // 6)     # the mirror's positions
            hit = ((px[:, 0] == first % 6) & (px[:, 1] == first // 6)).numpy() & (np.arange(batch) >= batch // 2)
            assert np.array_equal(hit, in_class) and (batch < 1100 or 200 < hit.sum() < 350)     # P(edge class) = 1/2 of 550 rays


@pytest.mark.parametrize("batch", [64, 1100])
@pytest.mark.parametrize("importance", [0, 1])
def test_wide_image_of_two_rows(importance, batch):
    s = sampler("C", seed=13)
    o = run(s, 0, 2, batch, importance)
    assert_draw(o, expect(s, 0, 13, 2, batch, importance), (importance, batch))
    if importance == 0 and batch == 1100:                             # 8 steps: px reaches both ends of the 4099 columns
        px = []
        for step in range(8):
            o = run(s, 0, step, batch, 0)
            assert_draw(o, expect(s, 0, 13, step, batch, 0), step)
            px.append(o["pixels"][:, 0].cpu())
        px = torch.cat(px)
        # the columns drawn span more than 4000 of the 4099, and are as many as 8800 uniform draws give: 4099 (1 - e^-2.147) = 3620 distinct
        # ones in expectation, sd 17 (more than 4000 DISTINCT columns is out of reach of a uniform draw of this size); 3500 is 7 sd below
        assert int(px.min()) >= 0 and int(px.max()) <= 4098 and int(px.max()) - int(px.min()) > 4000
        assert len(set(px.tolist())) > 3500
        assert set(o["pixels"][:, 1].cpu().tolist()) == {0, 1}


def test_launch_shapes_agree():
    """One workgroup of 1024 threads (which also increments the counter) and 256-thread workgroups draw the same rays: index = ray."""
    s = sampler("A", seed=5)
    a, b = run(s, 0, 7, 1024, 0), run(s, 0, 7, 2048, 0)
    assert_draw(a, expect(s, 0, 5, 7, 1024, 0), 1024)
    assert_draw(b, expect(s, 0, 5, 7, 2048, 0), 2048)
    assert torch.equal(a["pixels"], b["pixels"][:1024]) and same_bits(a["t_rand"], b["t_rand"][:1024])
    x, y = outputs(a), outputs(b)
    for k in RAY_KEYS:
        assert same_bits(x[k], y[k][:1024]), k


@pytest.mark.parametrize("batch", [64, 1100])
def test_offset_entry_without_a_counter(batch):
    """counter_dev == NULL: the step is `offset`, and nothing is incremented."""
    step = 2 ** 33 + 1
    s = sampler("A", seed=5)
    s._counter.fill_(77)
    rc, b = raw_sample(s, 1, batch, 1, 5, step, None)
    assert rc == 0 and int(s._counter.item()) == 77
    want = expect(s, 1, 5, step, batch, 1)
    assert_draw(b, want, batch)
    o = run(s, 1, step, batch, 1)                                     # the counter path at that step
    assert_draw(o, want, batch)
    x = outputs(o)
    for k in RAY_KEYS:
        assert same_bits(x[k], b[k]), k
    assert int(b["img_idx"]) == 1
    rc, c = raw_sample(s, 1, batch, 1, 5, 12345, s._counter)          # with a counter the offset is not read
    assert rc == 0 and int(s._counter.item()) == step + 2 and torch.equal(c["pixels"], torch.from_numpy(expect(s, 1, 5, step + 1, batch, 1)[0]).to(DEV))


def test_image_of_the_step_beyond_2_32():
    """img_idx=None at a counter of 2^32 + 3: the image is perm[step % n] / the epoch order's, and the weighted draw reads the SELECTED
    image's n_edge, density and pixel order."""
    s = sampler("A", seed=5)
    assert int(s._n_edge[0]) != int(s._n_edge[2])
    s.set_image_perm([2, 0, 1])
    img = [2, 0, 1][BIG_STEP % 3]
    o = run(s, None, BIG_STEP, 65, 1)
    assert int(o["img_idx"]) == img == 0
    assert_draw(o, expect(s, img, 5, BIG_STEP, 65, 1), "image_perm")
    assert not np.array_equal(expect(s, 2, 5, BIG_STEP, 65, 1)[0], expect(s, img, 5, BIG_STEP, 65, 1)[0])   # another image would show
    px = o["pixels"].cpu()
    assert torch.equal(o["rays"]["edge"].cpu().reshape(-1), scene("A")[0][img][px[:, 1], px[:, 0]])
    t = sampler("A", seed=5)
    t.set_train_images([2, 0])
    img = train_image(5, BIG_STEP, [2, 0])
    o = run(t, None, BIG_STEP, 65, 1)
    assert int(o["img_idx"]) == img and int(t._epoch_tag.item()) == BIG_STEP // 2
    assert_draw(o, expect(t, img, 5, BIG_STEP, 65, 1), "train list")
    assert not np.array_equal(expect(t, 2 - img, 5, BIG_STEP, 65, 1)[0], expect(t, img, 5, BIG_STEP, 65, 1)[0])
    px = o["pixels"].cpu()
    assert torch.equal(o["rays"]["edge"].cpu().reshape(-1), scene("A")[0][img][px[:, 1], px[:, 0]])


def test_captured_replay_follows_the_counter():
    """One capture, two replays: the draws of steps k and k + 1 of the definition, k written into the counter after the capture."""
    k = BIG_STEP + 2
    s = sampler("A", seed=9)
    s.gen_random_rays_patches_at(1, 64, importance_sample=True)       # warm-up, then once on a side stream, as a capture needs
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s.gen_random_rays_patches_at(1, 64, importance_sample=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = s.gen_random_rays_patches_at(1, 64, importance_sample=True)
    s._counter.fill_(k)
    got = []
    for _ in range(2):
        g.replay()
        got.append({"pixels": cap["pixels"].clone(), "t_rand": cap["t_rand"].clone()})
    torch.cuda.synchronize()
    assert int(s._counter.item()) == k + 2
    for i in range(2):
        assert_draw(got[i], expect(s, 1, 9, k + i, 64, 1), i)
