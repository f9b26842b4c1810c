"""On-device ray / pixel sampler with the interface of ``Dataset.gen_random_rays_patches_at``
(reference src/dataset/dataset.py:222-307) - SURVEY.md par. 8 f3.

The reference draws the pixels of a training batch on the host (``torch.randint``; python ``random.choices`` over all H*W
pixel probabilities when ``importance_sample=True``), builds the rays with small CPU ops and copies six tensors to the GPU
every step.  ``DeviceRaySampler`` uploads the dataset ONCE (edge maps, inverse intrinsics, poses, per-image pixel lists for
the edge-weighted draw) and produces every batch with one kernel launch (``emap_sample_rays``): zero host->device copies
per step, no host synchronisation, graph-capturable (the step counter is a device word).

Wire format respected: ``meta_data.json`` {scene_box{near,far,radius,aabb}, height, width, frames[{intrinsics 4x4,
camtoworld 4x4, rgb_path}]} (dataset.py:66-104) via ``from_meta``; edge maps are whatever ``cv.imread(path, 0) / 255`` gave the
caller (dataset.py:133-135) - image decoding is outside the hot path and stays with the caller (no cv2 in this image).

``gen_rays_at`` / ``rays_at_flat`` are the rays of a whole validation view with the interface of ``Dataset.gen_rays_at``
(dataset.py:137-167), from the same device-resident K^-1 and poses (``emap_gen_rays_at``: one launch, 28 B written per ray).

``set_train_images`` walks a list of training images in a new order every epoch (the runner's ``torch.randperm`` per epoch,
runner_udf.py:249-250), re-derived on the device from the step counter; ``state_dict`` / ``load_state_dict`` are the sampler's part of a
checkpoint (``Trainer.save_checkpoint(path, sampler)``).

The host RNG streams (torch CPU generator, python ``random``) cannot be reproduced on a device: the draw is a
Philox4x32-10 stream keyed by ``seed``; the deterministic part (rays of given pixels) and the sampling distribution are what
the parity tests pin.  The draw itself - which pixel and jitter each (seed, step, ray) gives - is defined in include/emap_hip.h and held
to that definition bit for bit (tests/ray_draw_ref.py, tests/test_gpu_ray_draw.py).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib


class DeviceRaySampler:
    def __init__(self, edges, intrinsics_all, pose_all, device="cuda", seed=0, near=None, far=None):
        """edges: (n_images,H,W[,1]) float in [0,1]; intrinsics_all, pose_all: (n_images,4,4) (dataset.py:86-87,117-121)."""
        dev = torch.device(device)
        edges = torch.as_tensor(np.asarray(edges), dtype=torch.float32) if not isinstance(edges, torch.Tensor) else edges.float()
        if edges.dim() == 4:
            edges = edges[..., 0]
        self.n_images, self.H, self.W = [int(v) for v in edges.shape]
        self.image_pixels = self.H * self.W
        K = torch.as_tensor(intrinsics_all, dtype=torch.float32).reshape(self.n_images, 4, 4)
        P = torch.as_tensor(pose_all, dtype=torch.float32).reshape(self.n_images, 4, 4)
        self.intrinsics_all, self.pose_all = K.to(dev), P.to(dev)
        self.intrinsics_all_inv = torch.inverse(K)                  # dataset.py:119 (CPU, once)
        self.focal = K[0][0, 0]
        self.near, self.far = near, far
        self.device = dev
        self.seed = int(seed)
        flat = edges.reshape(self.n_images, -1)
        is_edge = flat > 0.1                                         # dataset.py:240
        # stable partition of the row-major pixel ids: edge pixels first
        order = torch.argsort((~is_edge).to(torch.uint8), dim=1, stable=True).to(torch.int32)
        self._edges = edges.contiguous().to(dev)
        self._order = order.contiguous().to(dev)
        self._n_edge = is_edge.sum(1).to(torch.int32).to(dev)
        self._density = flat.mean(1).float().to(dev)                 # edge_density = np.mean(img_np), :238
        self._kinv = self.intrinsics_all_inv[:, :3, :3].contiguous().to(dev)
        self._pose = P.contiguous().to(dev)
        self._perm, self._perm_host = None, None
        # set_train_images: [0, cap) the list, [cap, 2 cap) the current epoch's order of it (csrc/rays.hip), and the epoch that order is of.
        # Allocated once: a captured graph holds their addresses
        self._train, self._reshuffle, self._train_buf, self._epoch_tag = None, True, None, None
        self._counter = torch.zeros(1, dtype=torch.int64, device=dev)   # device-resident step counter (uint64 bits)
        self._ds = _lib.RayDataset(self._edges.data_ptr(), self._order.data_ptr(), self._n_edge.data_ptr(), self._density.data_ptr(),
                                   self._kinv.data_ptr(), self._pose.data_ptr(), None, self.n_images, self.H, self.W, 0)

    @classmethod
    def from_meta(cls, meta: dict, edges, device="cuda", seed=0):
        """meta: the parsed ``meta_data.json`` (dataset.py:66-104); edges: the decoded edge maps in frame order."""
        assert int(meta["height"]) == np.asarray(edges).shape[1] and int(meta["width"]) == np.asarray(edges).shape[2]
        K = torch.stack([torch.tensor(f["intrinsics"], dtype=torch.float32) for f in meta["frames"]])
        P = torch.stack([torch.tensor(f["camtoworld"], dtype=torch.float32)[:4, :4] for f in meta["frames"]])
        box = meta["scene_box"]
        return cls(edges, K, P, device=device, seed=seed, near=box["near"], far=box["far"])

    def set_image_perm(self, perm):
        """The runner's ``image_perm`` (runner_udf.py:79-82): with it ``img_idx=None`` walks the permutation on the device.  The list must
        have ``n_images`` entries (the kernel indexes it with ``step % n_images``); a shorter training list is ``set_train_images``."""
        perm = torch.as_tensor(perm, dtype=torch.int32).contiguous()
        self._perm_host = perm.cpu().tolist()
        self._perm = perm.to(self.device)
        self._ds.image_perm = self._perm.data_ptr()

    def set_train_images(self, images=None, reshuffle=True):
        """The images ``img_idx=None`` trains on (default: all), in a new order every epoch like the runner's ``torch.randperm`` per epoch
        (runner_udf.py:46, 249-250).  ``images``: distinct image ids, at most ``_lib.MAX_TRAIN_IMAGES``; fewer than ``n_images`` holds views
        out.  With L = len(images), step s of the device counter draws from position s % L of the order of epoch e = s // L,
        ``perm_e[j] = images[sigma_e(j)]`` with sigma_e the stable argsort of the L 64-bit keys (word 0 << 32 | word 1) of
        Philox4x32-10(key seed, stream 2**63 | e, index i) - a pure function of (seed, e, images): the counter is the whole state, and any
        sampler with the same seed and list walks the same order.  The sample kernel recomputes the order on the device whenever the
        counter has left the epoch its buffer holds (no host work per step; follows a counter written by a resume or a capture's
        rollback).  ``reshuffle=False``: every epoch walks ``images`` in the order given.

        The buffers are written in place, so a graph captured with a list of the same length follows a new list; L itself is a launch
        argument: capture again after changing it.  ``set_image_perm`` is not used while a training list is set."""
        imgs = list(range(self.n_images)) if images is None else [int(i) for i in images]
        L = _lib.lib()
        if L.emap_check_train_images((C.c_int32 * max(len(imgs), 1))(*imgs), len(imgs), self.n_images) != 0:
            raise ValueError("DeviceRaySampler.set_train_images: " + L.emap_last_error().decode("utf-8", "replace"))
        cap = min(self.n_images, _lib.MAX_TRAIN_IMAGES)
        if self._train_buf is None:
            self._train_buf = torch.zeros(2 * cap, dtype=torch.int32, device=self.device)
            self._epoch_tag = torch.full((1,), -1, dtype=torch.int64, device=self.device)
        lst = torch.tensor(imgs, dtype=torch.int32)
        self._train_buf[:len(imgs)].copy_(lst)
        self._train_buf[cap:cap + len(imgs)].copy_(lst)
        self._epoch_tag.fill_(-1)
        self._train, self._reshuffle = imgs, bool(reshuffle)

    # ---- the sampler's part of a checkpoint (Trainer.state_dict(sampler=...)); host only ----
    def state_dict(self):
        """seed, the device step counter (read: synchronises), the training list and its reshuffle flag, n_images - all of the sampler's
        state: the image order is a function of these (set_train_images)."""
        return {"seed": self.seed, "counter": int(self._counter.item()), "train_images": None if self._train is None else list(self._train),
                "reshuffle": bool(self._reshuffle), "n_images": self.n_images}

    def check_state_dict(self, state):
        """Raise ValueError (naming the key) where load_state_dict would; changes nothing."""
        for k in ("seed", "counter", "train_images", "reshuffle", "n_images"):
            if k not in state:
                raise ValueError(f"DeviceRaySampler.load_state_dict: missing key '{k}'")
        if int(state["n_images"]) != self.n_images:
            raise ValueError(f"DeviceRaySampler.load_state_dict: 'n_images' is {state['n_images']}, this sampler has {self.n_images}")
        if int(state["counter"]) < 0:
            raise ValueError(f"DeviceRaySampler.load_state_dict: 'counter' is negative ({state['counter']})")
        imgs = state["train_images"]
        if imgs is not None:
            imgs = [int(i) for i in imgs]
            L = _lib.lib()
            if L.emap_check_train_images((C.c_int32 * max(len(imgs), 1))(*imgs), len(imgs), self.n_images) != 0:
                raise ValueError("DeviceRaySampler.load_state_dict: 'train_images': " + L.emap_last_error().decode("utf-8", "replace"))

    def load_state_dict(self, state):
        """In place: the counter's and the training list's buffers keep their addresses, so a captured graph goes on from the loaded
        state (the seed and the list's length are launch arguments: a graph captured with other ones must be captured again)."""
        self.check_state_dict(state)
        self.seed = int(state["seed"])
        if state["train_images"] is None:
            self._train = None
        else:
            self.set_train_images(state["train_images"], state["reshuffle"])
        self._counter.fill_(int(state["counter"]))

    def gen_random_rays_patches_at(self, img_idx, batch_size, importance_sample=False, pixels=None):
        """-> the reference's ``sample`` dict (dataset.py:288-305), every tensor on the device.  img_idx=None: the image is
        chosen on the device from the step counter (graph-capturable).  pixels ((N,2) int64 x,y): bypass the random draw."""
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("emap_amd.DeviceRaySampler: the sampler kernel needs an MI355X (cuda) device; there is no CPU fallback "
                               "(the reference's own host sampler is Dataset.gen_random_rays_patches_at)")
        N = int(batch_size)
        f = torch.empty(N * 14, dtype=torch.float32, device=dev)
        rays_o, rays_v, edge, ds, uv, pc, tr = f[:3 * N].view(N, 3), f[3 * N:6 * N].view(N, 3), f[6 * N:7 * N].view(N, 1), \
            f[7 * N:8 * N].view(N, 1), f[8 * N:10 * N].view(N, 2), f[10 * N:13 * N].view(N, 3), f[13 * N:].view(N, 1)
        pix = torch.empty(N, 2, dtype=torch.int64, device=dev)
        img = torch.empty(1, dtype=torch.int32, device=dev)
        out = _lib.RayBatch(rays_o.data_ptr(), rays_v.data_ptr(), edge.data_ptr(), ds.data_ptr(), uv.data_ptr(), pc.data_ptr(),
                            pix.data_ptr(), img.data_ptr(), tr.data_ptr())
        pin = None
        if pixels is not None:
            px = torch.as_tensor(pixels)
            assert px.shape == (N, 2)
            if px.device.type == "cpu":      # given pixels index the edge maps in the kernel: reject out-of-range ones where it is free
                if bool(((px[:, 0] < 0) | (px[:, 0] >= self.W) | (px[:, 1] < 0) | (px[:, 1] >= self.H)).any()):
                    raise ValueError(f"DeviceRaySampler: pixels outside the {self.W}x{self.H} image")
                pin = px.to(torch.int64).to(dev).contiguous()
            else:                            # device pixels: clamped on the device (no host synchronisation)
                pin = torch.stack([px[:, 0].clamp(0, self.W - 1), px[:, 1].clamp(0, self.H - 1)], -1).to(torch.int64).contiguous()
        with torch.cuda.device(dev):
            if self._train is not None and (img_idx is None or int(img_idx) < 0):
                cap = self._train_buf.numel() // 2
                _lib.api().sample_rays_train(self._ds, self._train_buf if self._reshuffle else None, len(self._train), self._train_buf[cap:],
                                             self._epoch_tag, N, int(bool(importance_sample)), self.seed, self._counter, pin, out,
                                             _lib.stream_ptr(dev))
            else:
                _lib.api().sample_rays(self._ds, -1 if img_idx is None else int(img_idx), N, int(bool(importance_sample)), self.seed, 0,
                                       self._counter, pin, out, _lib.stream_ptr(dev))
        rays = {"rays_o": rays_o, "rays_v": rays_v, "edge": edge}
        # "t_rand" is not in the reference's dict: render()'s per-ray jitter (udf_renderer_blending.py:719 draws torch.rand([N,1]) - 0.5 on the
        # host generator), from the same device draw - pass it as render(..., t_rand=sample["t_rand"]) and the step has no host draw at all
        sample = {"rays": rays, "rays_ndc_uv": uv, "rays_norm_XYZ_cam": pc, "depth_scale": ds, "pixels": pix, "img_idx": img, "t_rand": tr}
        if img_idx is not None:
            sample["pose"] = self.pose_all[int(img_idx)]
            sample["intrinsics"] = self.intrinsics_all[int(img_idx)]
        return sample

    # ---- full-image rays: Dataset.gen_rays_at (dataset.py:137-167) ----

    def view_size(self, resolution_level=1):
        """-> (n, h, w): the (H // l) * (W // l) rays of a view at ``resolution_level`` l and its image size (host only)."""
        n, h, w = C.c_int64(), C.c_int(), C.c_int()
        _lib.api().gen_rays_count(self._ds, int(resolution_level), n, h, w)
        return n.value, h.value, w.value

    def _view_image(self, img_idx, via_perm):
        """(the index the kernel takes, the image it resolves to).  ``via_perm``: ``img_idx`` is a position in the runner's image
        permutation (``image_perm[img_idx % n_images]``, runner_udf.py:79-82), looked up on the device like the random sampler's."""
        img_idx = int(img_idx)
        if not via_perm:
            if not 0 <= img_idx < self.n_images:
                raise IndexError(f"DeviceRaySampler: image {img_idx} out of range ({self.n_images} images)")
            return img_idx, img_idx
        if self._train is not None:
            raise ValueError("DeviceRaySampler: via_perm addresses set_image_perm's list; with set_train_images active a position is "
                             "ambiguous (it depends on the epoch) - pass the image id")
        k = img_idx % self.n_images
        return -1 - k, (k if self._perm_host is None else self._perm_host[k])

    def rays_at_flat(self, img_idx, resolution_level=1, first=0, count=None, out=None, via_perm=False):
        """Rays [first, first + count) of a view in row-major (H // l, W // l) order, ONE launch (``emap_gen_rays_at``):
        -> rays_o (count, 3), rays_v (count, 3), depth_scale (count, 1), views of one buffer of 7 * count floats.  ``count=None``: up to the
        end of the view.  ``out``: a contiguous float32 tensor on the sampler's device with at least 7 * count elements to write into (a
        chunked caller reuses one)."""
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("emap_amd.DeviceRaySampler: the ray kernel needs an MI355X (cuda) device; there is no CPU fallback "
                               "(the reference's own host routine is Dataset.gen_rays_at)")
        n = self.view_size(resolution_level)[0]
        first = int(first)
        count = n - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > n:
            raise ValueError(f"DeviceRaySampler: rays [{first}, {first + count}) leave the view's {n} rays")
        if out is None:
            out = torch.empty(7 * count, dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or out.device != dev or not out.is_contiguous() or out.numel() < 7 * count:
            raise ValueError(f"DeviceRaySampler: `out` must be a contiguous float32 tensor on {dev} with at least {7 * count} elements")
        f = out.view(-1)
        rays_o, rays_v, ds = f[:3 * count].view(count, 3), f[3 * count:6 * count].view(count, 3), f[6 * count:7 * count].view(count, 1)
        with torch.cuda.device(dev):
            _lib.api().gen_rays_at(self._ds, self._view_image(img_idx, via_perm)[0], int(resolution_level), first, count,
                                   rays_o, rays_v, ds, _lib.stream_ptr(dev))
        return rays_o, rays_v, ds

    def gen_rays_at(self, img_idx, resolution_level=1, via_perm=False):
        """-> the reference's 5-tuple (dataset.py:161-167), every tensor on the device: rays_o, rays_v (H // l, W // l, 3), pose,
        intrinsics (4, 4) and depth_scale (W // l, H // l, 1).  The reference transposes rays_o and rays_v but NOT depth_scale, and
        ``Runner_UDF.validate`` reshapes it as it is (runner_udf.py:300); that layout is kept: depth_scale is the transposed view of the
        kernel's row-major (H // l, W // l, 1) output, so ``depth_scale.transpose(0, 1)`` is the scale of the ray at the same index."""
        _, h, w = self.view_size(resolution_level)
        rays_o, rays_v, ds = self.rays_at_flat(img_idx, resolution_level, via_perm=via_perm)
        img = self._view_image(img_idx, via_perm)[1]
        return rays_o.view(h, w, 3), rays_v.view(h, w, 3), self.pose_all[img], self.intrinsics_all[img], ds.view(h, w, 1).transpose(0, 1)
