"""Data-parallel training step over rays: one process per GPU, ``torch.distributed`` ("nccl" == RCCL over xGMI on ROCm;
"gloo" in the CPU tests).

EMAP itself is single-GPU (SURVEY.md par. 2a); this is the sharding the hot path admits (par. 8e): rays are independent
through sampling, MLP and compositing, so every rank renders its slice of ONE global batch with replicated weights.  The
step arithmetic restates reference src/runner/runner_udf.py:90-168 (mask of ones, MSE * edge_weight + igr_ns_weight *
ge_ns + igr_weight * ge, zero_grad / backward / step).

``Trainer`` is the native step (no autograd graph, no per-parameter copies):

  forward     emap_render_fwd on the rank's rays                                   (HIP, no collective)
  stats       [sum(relax), sum(near), sum(relax*err), sum(near*err), sum((edge-gt)^2)]   5 floats
  backward    emap_render_bwd writes dL/dtheta of the rank's share of the GLOBAL loss straight into one flat fp32 buffer laid
              out in parameters() order - the parameters themselves are views of one flat buffer as well
  all-reduce  ONE collective over that buffer (about 1.85 MB for d8 w256; the stats ride in its tail)
  Adam        one launch over the flat buffers (emap_adam_step: torch.optim.Adam's arithmetic with the reference's two parameter
              groups, runner_base.py:110-117); on the CPU (tests) torch.optim.Adam itself
The statistics, dL/d(edge) and the loss scalars are one small kernel each on the GPU (emap_train_stats / emap_train_loss) instead
of ~25 element-wise torch launches - at 2 ms per step their launch latencies were 7 % of it.

The eikonal terms are masked means over ALL rays of the batch (udf_renderer_blending.py:618-625): their denominators must be
the global mask sums for the step to equal the single-GPU step.  ``eikonal_sync="exact"`` (default) therefore all-reduces the 5
stats before the backward (20 bytes, the only other collective of the step); ``eikonal_sync="local"`` uses the rank's own
denominators (a mean of per-rank means - exact whenever the masks cover every sample, as they do for scenes inside the unit
sphere) and the step has exactly one collective.

``Trainer(..., schedule=TrainSchedule(...))`` also keeps the four numbers the runner changes every iteration (runner_base.py:128-180:
the two learning rates, cos_anneal_ratio, flip_saturation) on the device: every step first enqueues ``emap_train_schedule``, which
evaluates them from a device iteration counter, and the render, the backward and Adam read them from device memory.  A captured step
then follows the schedules, and with ``capture(sampler=...)`` the ray draw is in the graph too: one replay is one whole iteration of
runner_udf.py:63-170 with no per-step host work.

``Trainer(..., monitor=TrainMonitor(...))`` (emap_amd/monitor.py) also keeps what the runner reports about an iteration and its
500-iteration loss average (runner_udf.py:110-135, :172-244) on the device - one launch at the end of the step, in place of
emap_train_loss - and ``fit()`` drives a loop with the runner's report / save-best / validate cadence on top of it.

``Trainer.state_dict / load_state_dict`` (``save_checkpoint / load_checkpoint``) write and read the reference's checkpoint
(runner_udf.py:252-275: the three modules, the optimizer in torch.optim.Adam's layout, iter_step) plus one ``emap_native`` entry; a
load writes every buffer in place, so a captured step goes on from it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional

import torch
import torch.distributed as dist

from . import _lib


def shard(t: torch.Tensor, rank: int, world: int) -> torch.Tensor:
    """Rank's contiguous slice [rank*N/world, (rank+1)*N/world) of a global per-ray tensor."""
    n = t.shape[0]
    assert n % world == 0, "global ray batch must divide evenly over ranks"
    per = n // world
    return t[rank * per:(rank + 1) * per].contiguous()


def _world(group=None) -> int:
    return dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1


class OneShotAllReduce:
    """SUM all-reduce of a small fp32 bucket by direct peer reads over xGMI (csrc/allreduce.hip; SURVEY.md par. 8e "xGMI note"): every rank
    reads every other rank's staging buffer through ``hipIpcMemHandle`` mappings and sums in rank order - one launch, one synchronisation,
    bit-identical results on all ranks; no host work per call (graph-capturable).  The alternative to RCCL's ring for the step's
    latency-bound 1.85 MB gradient bucket (``Trainer(..., allreduce="oneshot")``, ``bench.py --allreduce oneshot``).

    Construction is collective: the ranks exchange their 64-byte IPC handles through ``torch.distributed`` (any backend, gloo included -
    the ranks may even share one GPU, which is how the one-GPU tests run it).  One node only (IPC handles do not cross hosts)."""

    def __init__(self, n_floats: int, device, group=None):
        assert dist.is_available() and dist.is_initialized(), "OneShotAllReduce needs an initialised process group (for the handle exchange)"
        self.group, self.device = group, torch.device(device)
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self.n_floats = int(n_floats)
        self.region_bytes = _lib.size_of("ar_local_bytes", self.n_floats)
        self._own = C.c_void_p()
        handle = (C.c_ubyte * 64)()
        with torch.cuda.device(self.device):
            _lib.api().ar_alloc(self.region_bytes, self._own, handle)
        handles = [None] * self.world
        dist.all_gather_object(handles, bytes(handle), group=group)
        self._peers = []
        regions = (C.c_void_p * self.world)()
        with torch.cuda.device(self.device):
            for r, h in enumerate(handles):
                if r == self.rank:
                    regions[r] = self._own.value
                    continue
                p = C.c_void_p()
                _lib.api().ar_open((C.c_ubyte * 64).from_buffer_copy(h), p)
                self._peers.append(p)
                regions[r] = p.value
        self._regions = regions
        dist.barrier(group=group)               # every rank has mapped every region before the first launch touches one

    def __call__(self, t: torch.Tensor) -> torch.Tensor:
        """In place: t <- sum over the ranks of t.  fp32, contiguous, on this device, at most n_floats elements; every rank must call it
        with the same number of elements, in the same order."""
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() <= self.n_floats
        with torch.cuda.device(t.device):
            _lib.api().ar_allreduce_sum(t, t.numel(), self.rank, self.world, self._regions, self.region_bytes, _lib.stream_ptr(t.device))
        return t

    @staticmethod
    def set_timeout_ms(ms: int):
        """Bound of one peer wait inside the kernel (default 10 s; x6 for a region's first two launches).  Process-wide."""
        _lib.api().ar_set_timeout_ms(int(ms))

    def check(self):
        """Raise if a launch gave up waiting for a peer (host read: synchronises).  Such a launch has also written NaN into its bucket
        (csrc/allreduce.hip step 4), so the loss and the parameters of this rank are NaN from that step on - the time-out cannot pass
        unnoticed even where nobody calls this."""
        e = C.c_int()
        with torch.cuda.device(self.device):
            _lib.api().ar_error(self._own, e)
        if e.value:
            raise RuntimeError("OneShotAllReduce: a peer's buffer did not arrive within the kernel's time-out (a rank died or the ranks do "
                               "not call the collective in lock step)")

    def close(self):
        if getattr(self, "_own", None) is None:
            return
        L = _lib.lib()                           # the raw view: tearing down goes on whatever a call answers
        try:
            torch.cuda.synchronize(self.device)
            dist.barrier(group=self.group)       # nobody unmaps while a peer may still read
        except Exception:
            pass
        with torch.cuda.device(self.device):
            for p in self._peers:
                L.emap_ar_close(p)
            L.emap_ar_free(self._own)
        self._peers, self._own = [], None


class FlatParams:
    """Re-homes `params` as views of ONE flat fp32 buffer (and their .grad as views of one flat gradient buffer), so that a
    gradient all-reduce and an optimizer step touch one tensor instead of one per parameter."""

    def __init__(self, params: Iterable[torch.nn.Parameter], extra: int = 0):
        self.params: List[torch.nn.Parameter] = list(params)
        dev = self.params[0].device
        self.numel = sum(p.numel() for p in self.params)
        self.data = torch.empty(self.numel, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.numel + extra, dtype=torch.float32, device=dev)   # tail: step statistics
        off = 0
        self.offsets = {}
        with torch.no_grad():
            for p in self.params:
                n = p.numel()
                self.data[off:off + n].copy_(p.detach().reshape(-1))
                p.data = self.data[off:off + n].view(p.shape)
                p.grad = self.grad[off:off + n].view(p.shape)
                self.offsets[id(p)] = off
                off += n

    def span(self, params: Iterable[torch.nn.Parameter]):
        """(start, end) of a run of parameters that are adjacent in the flat buffer."""
        ps = list(params)
        s = self.offsets[id(ps[0])]
        e = self.offsets[id(ps[-1])] + ps[-1].numel()
        assert e - s == sum(p.numel() for p in ps), "parameters are not contiguous in the flat buffer"
        return s, e


class _FlatAdam:
    """The state of emap_adam_step[_masked] over one flat fp32 buffer of `n` elements, the first `n_geo` of them the geometry range
    (ONE step counter, `t`: its parameters always step together) and the rest the tail (`tail_sizes`: the element counts of its
    parameters): every tail element has its own step count and a trainable mask.  Everything lives on the device - no host index
    tensors in the step, nothing a captured graph could bake in; a graph reads the mask BUFFER, so set_mask() between replays takes
    effect without re-capturing."""

    def __init__(self, n: int, n_geo: int, tail_sizes: List[int], dev):
        assert n_geo + sum(tail_sizes) == n
        self.n, self.n_geo, self.tail_sizes = n, n_geo, list(tail_sizes)
        self.m, self.v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        self.t = torch.zeros(1, device=dev)
        self.spare_t = torch.zeros(1, device=dev)      # the counter a launch over the tail alone bumps (step(geo_grad_ptr=...))
        nt = max(n - n_geo, 1)
        self.tail_mask, self.tail_step = torch.ones(nt, device=dev), torch.zeros(nt, device=dev)
        self.flags = None                              # per tail parameter, as last written to tail_mask
        self._pinned = torch.ones(nt).pin_memory() if dev.type == "cuda" else None

    def set_mask(self, flags, capturing: bool = False) -> bool:
        """tail_mask <- one flag per tail parameter (True: the step updates it).  Nothing happens while the flags stay as they are."""
        flags = tuple(flags)
        if flags == self.flags:
            return False
        if capturing or (self.m.is_cuda and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError("flat Adam: the set of trainable tail parameters changed inside a graph capture")
        vals = torch.tensor([1.0 if f else 0.0 for f, k in zip(flags, self.tail_sizes) for _ in range(k)])
        k = vals.numel()
        if self._pinned is not None:
            self._pinned[:k].copy_(vals)
            self.tail_mask[:k].copy_(self._pinned[:k], non_blocking=True)
        else:
            self.tail_mask[:k].copy_(vals)
        self.flags = flags
        return True

    def step(self, data, grad, lr_geo, lr_tail, betas, eps, geo_grad_ptr: Optional[int] = None, lr_dev: Optional[torch.Tensor] = None):
        """One Adam step of `data` (n floats).  `grad` holds all n gradients - one launch - or, with `geo_grad_ptr` (the address of the
        n_geo geometry gradients in a buffer of the caller), those of the tail alone: two launches on disjoint ranges with the same
        arithmetic, the geometry range first (it bumps `t`), then the tail with its own step counts.  `lr_dev` (two device floats:
        geometry, tail; one launch only): the learning rates are read on the device and `lr_geo` / `lr_tail` are not used."""
        A, dev = _lib.api(), data.device
        tail = (self.tail_mask, self.tail_step, _lib.stream_ptr(dev))
        if lr_dev is not None:
            assert geo_grad_ptr is None
            with torch.cuda.device(dev):
                A.adam_step_masked_sched(data, grad, self.m, self.v, self.t, self.n, self.n_geo, lr_dev, float(betas[0]), float(betas[1]),
                                         float(eps), *tail)
            return
        hyper = (float(lr_geo), float(lr_tail), float(betas[0]), float(betas[1]), float(eps))
        with torch.cuda.device(dev):
            if geo_grad_ptr is None:
                A.adam_step_masked(data, grad, self.m, self.v, self.t, self.n, self.n_geo, *hyper, *tail)
                return
            ng, nt = self.n_geo, self.n - self.n_geo
            A.adam_step(data, geo_grad_ptr, self.m, self.v, self.t, ng, ng, *hyper, tail[2])
            if nt > 0:
                A.adam_step_masked(data[ng:], grad, self.m[ng:], self.v[ng:], self.spare_t, nt, 0, *hyper, *tail)


def _loss_from_stats(stats, n_elem, edge_weight, igr_weight, igr_ns_weight):
    """(loss, edge_loss) of the GLOBAL batch from its statistics [sum relax, sum near, sum relax*err, sum near*err, sum diff^2] - the one
    order of the five floats everywhere (emap_train_stats / emap_train_loss are the device side of the same convention)."""
    edge_loss = stats[4] / n_elem * edge_weight
    loss = edge_loss + igr_weight * stats[2] / (stats[0] + 1e-5) + igr_ns_weight * stats[3] / (stats[1] + 1e-5)
    return loss, edge_loss


def _global_mask_sums(scalars, stats):
    """The forward's scalars with the rank's two eikonal mask sums ([4], [6]) replaced by the GLOBAL ones of the all-reduced `stats`."""
    sc = scalars.clone()
    sc[4], sc[6] = stats[0], stats[1]
    return sc


def _run_phases(fns, coll, S):
    """Call `fns` in order - the four phases of a step or the replays of their graphs - and after the i-th the collectives tagged i
    (Trainer._collectives).  Returns what the last one returned."""
    out = None
    for i, fn in enumerate(fns):
        out = fn()
        for after, c in coll:
            if after == i:
                c(S)
    return out


@dataclass
class _Step:
    """What the phases of one native step hand to each other (and to the collectives between them)."""
    call: Optional[dict] = None              # the forward: the prepared call, its outputs, its scalars
    v: Optional[dict] = None
    scalars: Optional[torch.Tensor] = None
    d_edge: Optional[torch.Tensor] = None
    n_glob: int = 0
    sync: Optional[str] = None               # several ranks: "exact" (also exact_lagged) or "local"; one rank: None
    sc_glob: Optional[torch.Tensor] = None   # `scalars` with the global mask sums ("exact")
    lagged: bool = False                     # exact_lagged on several ranks: the range maxima ride in the bucket's tail


class _AdamGroups:
    """What the step reads from `Trainer.optimizer` when the update runs in emap_adam_step: the two parameter groups of the
    reference (runner_base.py:110-117) with the keys its schedulers touch (`g["lr"] = ...`, runner_base.py:140-141,159-160)."""

    def __init__(self, trainer, lr_geo, lr, betas=(0.9, 0.999), eps=1e-8):
        self._t = trainer
        self.param_groups = [{"params": [trainer.p_geo], "lr": lr_geo, "betas": betas, "eps": eps},
                             {"params": [trainer.p_sc], "lr": lr, "betas": betas, "eps": eps}]

    def zero_grad(self, set_to_none: bool = False):       # the backward overwrites the flat gradient buffer
        pass

    def step(self):
        t, (g0, g1) = self._t, self.param_groups
        # with a schedule the two learning rates are the device words of emap_train_schedule: param_groups[*]["lr"] are not read
        t._adam.step(t.flat.data, t.flat.grad, g0["lr"], g1["lr"], g0["betas"], g0["eps"], lr_dev=t._sched)


class Trainer:
    """Native data-parallel training step of the render hot path (see the module docstring)."""

    N_STATS = 8          # tail of the gradient bucket: [0, 5) the step statistics ("local"); then 2 range maxima per rank ("exact_lagged")
    MAX_RANKS = 16

    def __init__(self, renderer, lr_geo: float = 1e-4, lr: float = 5e-4, edge_weight: float = 1.0, igr_weight: float = 0.1,
                 igr_ns_weight: float = 0.0, group=None, eikonal_sync: str = "exact", fused_adam: Optional[bool] = None,
                 native_tail: Optional[bool] = None, allreduce: str = "rccl", schedule=None, start_iter: int = 0, monitor=None):
        """schedule (emap_amd.TrainSchedule; None: nothing changes): the step evaluates the reference's per-iteration schedules on the
        device from its own iteration counter, which starts at `start_iter` (see iter_step / set_iter_step).  Then
        ``optimizer.param_groups[*]["lr"]`` are not read, and ``rays`` must not carry cos_anneal_ratio / flip_saturation.

        monitor (emap_amd.TrainMonitor; None: nothing new is enqueued): every step ends with emap_train_monitor, which writes the
        runner's per-iteration quantities and its running loss average into the monitor's device buffers and the step's
        [loss, edge_loss] with them.  Needs `schedule`: the monitor reads the iteration counter and the learning rates from it.
        On several ranks loss / edge_loss / psnr / the eikonal terms are the global batch's, udf_min / udf_mean / weight_sum the
        rank's own rays'.  Checkpoints do not carry the monitor.  (``native_tail=False``, the CPU tests: the eager step evaluates the
        schedule on the host, TrainSchedule.values, and feeds the monitor through TrainMonitor.update_host.)"""
        if monitor is not None and schedule is None:
            raise ValueError("Trainer: monitor= needs schedule= (the monitor takes the iteration number and the learning rates from the "
                             "schedule's device words; without a schedule the trainer has neither)")
        assert eikonal_sync in ("exact", "exact_lagged", "local")
        # only "exact_lagged" uses the rank-indexed maxima slots of the bucket's tail: "exact" / "local" run on any number of ranks
        assert eikonal_sync != "exact_lagged" or _world(group) <= self.MAX_RANKS, \
            f"eikonal_sync='exact_lagged' keeps two range maxima per rank in the gradient bucket's tail: at most {self.MAX_RANKS} ranks"
        self.r = renderer
        self.group = group
        self.eikonal_sync = eikonal_sync
        self.edge_weight, self.igr_weight, self.igr_ns_weight = float(edge_weight), float(igr_weight), float(igr_ns_weight)
        net = renderer.udf_network
        self.geo = list(net.parameters())
        self.scalars = [renderer.deviation_network.variance, renderer.beta_network.beta, renderer.beta_network.gamma]
        # tail of the bucket: the step statistics; "exact_lagged" only: + two range maxima per rank
        self.flat = FlatParams(self.geo + self.scalars, extra=self.N_STATS + (2 * self.MAX_RANKS if eikonal_sync == "exact_lagged" else 0))
        renderer._lay = None                      # the layout caches tensor identities / pointers: rebuild on the flat views
        lay = renderer._layout()
        assert lay.numel == self.flat.numel and all(lay.offsets[id(p)] == self.flat.offsets[id(p)] for p in self.flat.params)
        g0, g1 = self.flat.span(self.geo)
        s0, s1 = self.flat.span(self.scalars)
        # two flat "parameters" = the reference's two Adam groups (runner_base.py:110-117)
        self.p_geo = torch.nn.Parameter(self.flat.data[g0:g1])
        self.p_sc = torch.nn.Parameter(self.flat.data[s0:s1])
        self.p_geo.grad = self.flat.grad[g0:g1]
        self.p_sc.grad = self.flat.grad[s0:s1]
        dev = self.flat.data.device
        if fused_adam is None:
            fused_adam = dev.type == "cuda"
        # native tail (GPU default): statistics / loss scalars / Adam as three small HIP kernels (csrc/train.hip)
        if native_tail is None:      # native_tail=False: torch element-wise ops + torch.optim.Adam (the CPU tests; A/B 2.12 vs 2.05 ms)
            native_tail = dev.type == "cuda"
        self.native_tail = bool(native_tail)
        if self.native_tail:
            assert g0 == 0 and s0 == g1 and s1 == self.flat.numel, "flat layout: geometry parameters first, then the scalars"
            # the step counter, the scalars' trainable mask and their own step counts live on the device: the update is graph-capturable.
            # The mask is refreshed from requires_grad at every step() / replay().
            a = self._adam = _FlatAdam(self.flat.numel, g1, [p.numel() for p in self.scalars], dev)
            # the holder's buffers under the names the multi-process tests reset them by (the same tensors, not copies)
            self._m, self._v, self._adam_t, self._tail_step = a.m, a.v, a.t, a.tail_step
            self._stats = torch.zeros(5, device=dev)
            self.optimizer = _AdamGroups(self, lr_geo, lr)
        else:
            # capturable: the step counters live on the device, so a whole step can be captured in a hipGraph (capture())
            self.optimizer = torch.optim.Adam([{"params": [self.p_geo], "lr": lr_geo}, {"params": [self.p_sc]}], lr=lr,
                                              **({"fused": True, "capturable": True} if fused_adam else {}))
        # steady state: "exact" 3 (statistics SUM, range maxima MAX, gradients), "exact_lagged" 2 (the maxima ride in the gradient bucket
        # and are used one step late; the very first step takes the exact path), "local" 1
        self.collectives_per_step = 0 if _world(group) == 1 else {"exact": 3, "exact_lagged": 2, "local": 1}[eikonal_sync]
        self._lag = torch.zeros(2, device=dev)      # exact_lagged: the GLOBAL range maxima of the previous step
        self._lag_valid = False
        # "local": every rank normalises by its own mask sums, so the sum over ranks needs the 1/world of a mean of means
        k = 1.0 / _world(group) if eikonal_sync == "local" else 1.0
        self._igr = torch.tensor([self.igr_weight * k], device=dev)
        self._igr_ns = torch.tensor([self.igr_ns_weight * k], device=dev)
        self._idx = torch.tensor([4, 6, 3, 5], device=dev)
        self.last_stats = None
        # the gradient bucket's collective: "rccl" = torch.distributed.all_reduce on the group's backend (RCCL / gloo);
        # "oneshot" = direct peer reads over hipIpc mappings (OneShotAllReduce; one node, GPU only).  The 20-byte statistics / 8-byte
        # maxima exchanges of the exact modes stay on torch.distributed either way.
        assert allreduce in ("rccl", "oneshot")
        self.allreduce = allreduce
        self._oneshot = None
        if allreduce == "oneshot" and _world(group) > 1:
            self._oneshot = OneShotAllReduce(self.flat.grad.numel(), dev, group)
        # the reference's per-step schedules on the device: the iteration counter (every rank keeps its own, identical one) and the four
        # numbers emap_train_schedule writes at the top of every step [lr_geo, lr, cos_anneal_ratio, flip_saturation]
        self.schedule = schedule
        self._iter = self._sched = None
        if schedule is not None:
            if int(start_iter) < 0:
                raise ValueError(f"Trainer: start_iter must be >= 0 (got {start_iter})")
            self._iter = torch.full((1,), int(start_iter), dtype=torch.int64, device=dev)
            self._sched = torch.zeros(4, device=dev)
        self.monitor = monitor
        if monitor is not None:
            monitor.bind(dev)

    # ---- the scheduled step (schedule=TrainSchedule(...)) ----
    @property
    def iter_step(self) -> int:
        """The iteration the NEXT step runs at - the reference's iter_step (runner_udf.py:170).  Reads the device counter: synchronises."""
        if self._iter is None:
            raise RuntimeError("Trainer.iter_step: this trainer has no schedule")
        return int(self._iter.item())

    def set_iter_step(self, k: int):
        """Write the device iteration counter (resuming from a checkpoint's iter_step).  A captured graph reads the buffer, so a write
        between replays takes effect without re-capturing.  A monitor is reset(): its window and its rows belong to the iterations before."""
        if self._iter is None:
            raise RuntimeError("Trainer.set_iter_step: this trainer has no schedule")
        if int(k) < 0:
            raise ValueError(f"Trainer.set_iter_step: the iteration must be >= 0 (got {k})")
        self._iter.fill_(int(k))
        if self.monitor is not None:
            self.monitor.reset()

    def _check_scheduled(self, rays, capturing: bool = False):
        """The scheduled step has ONE source for the two render scalars - the device schedule - and runs on the native tail only.  (The
        one exception is the monitored torch tail of the CPU tests, whose eager step evaluates the schedule on the host: the monitor
        needs the iteration number and the learning rates from somewhere.)"""
        for k in ("cos_anneal_ratio", "flip_saturation"):
            if k in rays:
                raise ValueError(f"Trainer: rays['{k}'] given to a trainer with a schedule - the schedule on the device is the only source "
                                 "of cos_anneal_ratio / flip_saturation")
        if not self.native_tail and (capturing or self.monitor is None):
            raise RuntimeError("Trainer: schedule= needs the native tail (emap_train_schedule and the *_sched entry points are HIP kernels; "
                               "there is no CPU fallback)")

    @staticmethod
    def sampler_batch(sampler, batch_size: int, importance_sample: bool = False):
        """-> (rays, true_edge) of one training batch from a DeviceRaySampler, image ``image_perm[counter % n_images]`` (or, after
        ``sampler.set_train_images``, the counter's position in its epoch's order of the training list): what runner_udf.py:70-90 hands to render(), with the jitter draw of the same launch as rays['t_rand']."""
        if sampler.near is None or sampler.far is None:
            raise ValueError("Trainer.sampler_batch: the sampler has no near / far (DeviceRaySampler(..., near=, far=) or from_meta)")
        smp = sampler.gen_random_rays_patches_at(-1, batch_size, importance_sample)
        rays = {"rays_o": smp["rays"]["rays_o"], "rays_d": smp["rays"]["rays_v"], "near": float(sampler.near), "far": float(sampler.far),
                "depth_scale": smp["depth_scale"], "t_rand": smp["t_rand"]}
        return rays, smp["rays"]["edge"]

    # ---- the two HIP stages; the CPU tests substitute oracle implementations for them ----
    def _forward(self, rays):
        r = self.r
        car, fs = rays.get("cos_anneal_ratio"), rays.get("flip_saturation", 0.0)
        if self._sched is not None:
            car, fs = 1.0, 0.0        # place holders (the annealed cosine is on): the kernels read both from self._sched
        call = r._prepare(rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], rays.get("depth_scale"), car,
                          rays.get("perturb_overwrite", -1), rays.get("background_rgb"), fs, rays.get("t_rand"))
        call["sched"] = self._sched   # the backward of this call reads it from here as well
        v = r._render_hip(call)
        return call, v, v["edge"], v["scalars"]

    def _backward(self, call, v, d_edge, scalars_glob, flat_grad, stages=3):
        """stages: 3 the whole backward; 1 the compositing half (leaves the range maxima, renderer.bwd_absmax), 2 the MLP half"""
        self.r.backward_into(call, v, d_edge, None, self._igr, self._igr_ns if self.igr_ns_weight != 0.0 else None,
                             flat=flat_grad, scalars=scalars_glob, stages=stages)

    def _sync(self):
        """What several ranks exchange besides the gradients: "exact" - the statistics, all-reduced before the backward (also exact_lagged) -
        or "local" - nothing, the statistics ride in the gradient bucket's tail; None on one rank."""
        if _world(self.group) == 1:
            return None
        return "local" if self.eikonal_sync == "local" else "exact"

    def _stats_slot(self):
        """The five step statistics' slot in the tail of the gradient bucket ("local")"""
        return self.flat.grad[self.flat.numel:self.flat.numel + 5]

    def _scalar_flags(self):
        """Which of variance / beta / gamma the step updates: those with requires_grad, except `variance` under use_unbias_render=False,
        which the plain render does not reach (reference :551-559; torch.optim.Adam leaves a parameter without gradient untouched)."""
        for p in self.geo:
            if not p.requires_grad:
                raise NotImplementedError("Trainer: a UDF network parameter with requires_grad=False is not supported")
        plain = self.r.render_mode == _lib.RENDER_PLAIN
        return tuple(bool(p.requires_grad) and not (plain and i == 0) for i, p in enumerate(self.scalars))

    def check_errors(self):
        """Host-side health check (synchronises): the renderer's device error word and - ``allreduce="oneshot"`` - the collective's
        time-out word.  Call it wherever the loop reads the loss anyway (bench.py and scripts/train_synthetic.py do, every report)."""
        self.r.check_errors()
        if self._oneshot is not None:
            self._oneshot.check()

    def close(self):
        """Check for a timed-out collective one last time and unmap the peers' regions (collective: every rank calls it)."""
        one, self._oneshot = self._oneshot, None
        if one is not None:
            try:
                one.check()
            finally:
                one.close()

    def refresh_trainable_mask(self, capturing: bool = False):
        """Mirror `requires_grad` of variance / beta / gamma (runner_udf.py:141-154 flips them during training) into the device mask
        of the fused Adam.  Eager: called by every step.  Under a captured graph the mask BUFFER is what the graph reads, so a
        refresh between replays takes effect without re-capturing; a change inside a capture raises."""
        return self._adam.set_mask(self._scalar_flags(), capturing)

    # The native step is written as four device phases separated by the (at most three) collectives, so that it can run eagerly, be
    # captured whole in one hipGraph (one rank) or be captured phase by phase with the collectives launched between the replays
    # (any backend, also gloo whose collectives are host code): capture(segmented=True).
    def _phases(self, rays, true_edge, n_rays_global, batch=None):
        """-> (the step's record, its four phases): what _run_phases runs, or capture() records one by one.  `batch` (a callable ->
        (rays, true_edge), in place of the two): the first phase draws its own batch (capture(sampler=...))."""
        S = _Step()
        return S, [lambda: self._ph_forward(S, rays, true_edge, n_rays_global, batch), lambda: self._ph_composite_bwd(S),
                   lambda: self._ph_mlp_bwd(S), lambda: self._ph_update(S)]

    def _ph_forward(self, S, rays, true_edge, n_rays_global, batch=None):
        if self._sched is not None:      # this iteration's four scheduled numbers, then the counter moves on
            dev = self._sched.device
            with torch.cuda.device(dev):
                _lib.api().train_schedule(self._iter, *self.schedule.c_args(), self._sched, _lib.stream_ptr(dev))
        if batch is not None:
            rays, true_edge = batch()
        S.call, S.v, edge, S.scalars = self._forward(rays)
        dev = edge.device
        n_local = edge.numel()
        S.sync = self._sync()
        S.n_glob = n_rays_global if n_rays_global is not None else n_local * _world(self.group)
        te = true_edge.reshape(-1).to(torch.float32).contiguous()
        assert te.numel() == n_local
        S.d_edge = torch.empty(n_local, device=dev)
        with torch.cuda.device(dev):
            _lib.api().train_stats(edge, te, S.scalars, n_local, 2.0 * self.edge_weight / S.n_glob, S.d_edge, self._stats, _lib.stream_ptr(dev))

    def _ph_composite_bwd(self, S):
        exact = S.sync == "exact"            # self._stats now holds the GLOBAL sums
        S.sc_glob = _global_mask_sums(S.scalars, self._stats) if exact else S.scalars
        self._backward(S.call, S.v, S.d_edge, S.sc_glob, self.flat.grad[:self.flat.numel], stages=1 if exact else 3)
        S.lagged = exact and self.eikonal_sync == "exact_lagged"
        if S.lagged:
            # The two range maxima of this rank go into its slots of the bucket's tail (the SUM all-reduce of the bucket then works as an
            # all-gather of them: every other slot is zero) and become next step's GLOBAL maxima.  THIS step's sweep uses the previous
            # step's global maxima x 4 (the kernel rounds to a power of two) instead of waiting for a MAX all-reduce - or the rank's own
            # maxima where they exceed that, so that fp16 can never overflow: a rank whose gradients grew more than 4x in one step then
            # differs from the others in rounding for that step only.  The first step (no history) takes the exact path.
            self._lag_publish(self.r.bwd_absmax(S.call), dist.get_rank(self.group))

    def _lag_publish(self, cur: torch.Tensor, rank: int):
        """exact_lagged, before the sweep: write this rank's two range maxima `cur` into ITS two slots of the bucket's tail (all other
        slots zero: the bucket's SUM all-reduce is then an all-gather of them) and turn `cur` IN PLACE into the scale this step's sweep
        uses - 4 x last step's GLOBAL maxima, clamped to [own maxima, 16 x own maxima]: the lower clamp keeps fp16 from overflowing
        when the gradients GREW more than 4 x in one step, the upper one from flushing small adjoints when they SHRANK more than 4 x
        (a stale scale 1000 x too large leaves fp16 three binades).  Inside the clamp every rank uses the same number; at a
        clamp the ranks differ in rounding for that step only.  Without history (first step) `cur` is left alone."""
        tail = self._maxima_tail()
        tail.zero_()
        tail[2 * rank:2 * rank + 2] = cur
        if self._lag_valid:
            cur.copy_(torch.minimum(torch.maximum(self._lag * 4.0, cur), cur * 16.0))

    def _lag_collect(self):
        """exact_lagged, after the bucket's all-reduce: the gathered per-rank maxima of THIS step become next step's global maxima."""
        if self._lag_valid:
            self._lag.copy_(self._maxima_tail().view(self.MAX_RANKS, 2).max(dim=0).values)
        self._lag_valid = True

    def _maxima_tail(self):
        n = self.flat.numel + self.N_STATS
        return self.flat.grad[n:n + 2 * self.MAX_RANKS]

    def _ph_mlp_bwd(self, S):
        if S.lagged and not self._lag_valid:
            self._lag.copy_(self.r.bwd_absmax(S.call))       # first step: the MAX all-reduce just ran; it seeds the history
        if S.sync == "exact":
            self._backward(S.call, S.v, S.d_edge, S.sc_glob, self.flat.grad[:self.flat.numel], stages=2)
        if S.sync == "local":
            self._stats_slot().copy_(self._stats)      # the statistics ride in the bucket's tail

    def _ph_update(self, S):
        dev = self.flat.data.device
        if S.lagged:
            self._lag_collect()
        self.optimizer.step()      # frozen scalars are skipped inside the kernel (device mask, refresh_trainable_mask)
        self.r.udf_network.invalidate_packed()   # the flat update does not bump the per-parameter version counters
        stats = self._stats_slot() if S.sync == "local" else self._stats      # "local": the all-reduced bucket's tail holds the global sums
        out = torch.empty(2, device=dev)         # a fresh tensor per step: callers keep what step() returned
        weights = (self.edge_weight / S.n_glob, self.igr_weight, self.igr_ns_weight)
        if self.monitor is None:
            with torch.cuda.device(dev):
                _lib.api().train_loss(stats, *weights, out, _lib.stream_ptr(dev))
        else:                                    # the same two numbers, and the runner's report of this iteration (runner_udf.py:110-135, :172-241)
            self.monitor.launch(S.v["udf"], S.v["weight_sum"], S.call["N"], S.call["S"], stats, S.scalars, self._sched, self._iter, *weights,
                                S.n_glob, out)
        self.last_stats = out
        return out

    def _collectives(self):
        """The collectives of one step, in order, as (after_phase, callable): exact = [global eikonal mask sums + MSE sum (20 B),
        the two range maxima of the MLP backward (8 B, MAX), the flat gradient]; local = [the flat gradient with the statistics in
        its tail].  The maxima exchange makes every rank's backward use the SAME fp16 range scale, so the step does not depend on
        how the rays are sharded (beyond the order of the floating-point sums)."""
        if _world(self.group) == 1:
            return []
        ar = lambda t, op: (lambda S: dist.all_reduce(t(S), op=op, group=self.group))
        grad = ar(lambda S: self.flat.grad, dist.ReduceOp.SUM) if self._oneshot is None else (lambda S: self._oneshot(self.flat.grad))
        if self.eikonal_sync == "local":
            return [(2, grad)]
        stats = (0, ar(lambda S: self._stats, dist.ReduceOp.SUM))
        if self.eikonal_sync == "exact_lagged" and self._lag_valid:      # the maxima ride in the gradient bucket's tail
            return [stats, (2, grad)]
        return [stats, (1, ar(lambda S: self.r.bwd_absmax(S.call), dist.ReduceOp.MAX)), (2, grad)]

    def _step_native(self, rays: Dict, true_edge: torch.Tensor, n_rays_global: Optional[int], batch=None):
        coll = self._collectives()
        S, phases = self._phases(rays, true_edge, n_rays_global, batch)
        return _run_phases(phases, coll, S)

    def step(self, rays: Dict, true_edge: torch.Tensor, n_rays_global: Optional[int] = None):
        """One optimizer step on this rank's rays.  Returns the device tensor [loss, edge_loss] of the GLOBAL batch (no host
        synchronisation happens here)."""
        if self._sched is not None:
            self._check_scheduled(rays)
        if self.native_tail:
            self.refresh_trainable_mask()
            return self._step_native(rays, true_edge, n_rays_global)
        # the torch tail (the CPU tests): the native phases' arithmetic in element-wise torch ops, torch.optim.Adam, collectives in line
        if self._sched is not None:      # (monitored: _check_scheduled) emap_train_schedule on the host: the four numbers, then the counter moves on
            vals = self.schedule.values(int(self._iter.item()))
            self._sched.copy_(torch.tensor(vals, dtype=torch.float32))
            self.optimizer.param_groups[0]["lr"], self.optimizer.param_groups[1]["lr"] = vals[0], vals[1]
            self._iter += 1
        sync = self._sync()
        call, v, edge, scalars = self._forward(rays)
        n_local = edge.numel()
        n_glob = n_rays_global if n_rays_global is not None else n_local * _world(self.group)
        diff = edge.reshape(-1) - true_edge.reshape(-1).to(edge.dtype)
        # scalars[3:7] = e_rel, c_rel, e_ns, c_ns
        stats = torch.cat([scalars[self._idx], (diff * diff).sum().reshape(1)])
        sc_glob = scalars
        if sync == "exact":      # (no fp16 range scale on this path: lagged = exact)
            dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=self.group)
            sc_glob = _global_mask_sums(scalars, stats)
        self._backward(call, v, diff * (2.0 * self.edge_weight / n_glob), sc_glob, self.flat.grad[:self.flat.numel])
        if sync == "local":
            self._stats_slot().copy_(stats)      # the statistics ride in the bucket's tail
        if sync is not None:
            dist.all_reduce(self.flat.grad, op=dist.ReduceOp.SUM, group=self.group)
            stats = self._stats_slot().clone() if sync == "local" else stats
        # torch.optim.Adam on the two flat parameters cannot skip single elements: a frozen scalar (requires_grad = False,
        # runner_udf.py:144-154) is put back and its moments cleared (the native path masks inside the kernel)
        s0 = self.flat.span(self.scalars)[0]
        frozen = []                              # indices into p_sc
        for p, trainable in zip(self.scalars, self._scalar_flags()):
            if not trainable:
                a, b = self.flat.span([p])
                frozen += range(a - s0, b - s0)
        keep = self.p_sc.data[frozen].clone() if frozen else None
        self.optimizer.step()
        if frozen:
            self.p_sc.data[frozen] = keep
            st = self.optimizer.state.get(self.p_sc, {})
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st:
                    st[k][frozen] = 0.0
        self.r.udf_network.invalidate_packed()   # the flat update does not bump the per-parameter version counters
        self.last_stats = torch.stack(_loss_from_stats(stats, n_glob, self.edge_weight, self.igr_weight, self.igr_ns_weight))
        if self.monitor is not None:
            self.monitor.update_host(v["udf"].reshape(n_local, -1), v["weight_sum"], stats, scalars, self._sched, int(self._iter.item()),
                                     self.edge_weight / n_glob, self.igr_weight, self.igr_ns_weight, n_glob, loss_pair=self.last_stats)
        return self.last_stats

    def _train_state(self):
        """Every device buffer a step changes besides its outputs (capture() with a schedule rolls its warm-up steps back)."""
        a = self._adam
        return [self.flat.data, a.m, a.v, a.t, a.spare_t, a.tail_step, self._lag, self._iter] + (self.monitor.buffers() if self.monitor else [])

    def _sampled_step(self, batch, n_rays_global=None):
        """step() on a batch the first phase draws itself (`batch`: -> (rays, true_edge)), after the schedule launch"""
        self.refresh_trainable_mask()
        return self._step_native(None, None, n_rays_global, batch)

    def capture(self, rays: Optional[Dict] = None, true_edge: Optional[torch.Tensor] = None, n_rays_global: Optional[int] = None,
                warmup: int = 3, segmented: Optional[bool] = None, sampler=None, batch_size: Optional[int] = None,
                importance_sample: bool = False):
        """Capture one whole step (pack -> render forward -> statistics -> HIP backward -> [all-reduce] -> Adam) for this batch
        shape and return ``replay(rays=None, true_edge=None) -> [loss, edge_loss]`` (device tensor, static).  New rays / targets
        are copied into the static buffers before the replay.  `warmup` real steps are taken first (workspaces, function
        attributes, Adam state must exist before capturing).

        One rank: ONE hipGraph.  Several ranks (`segmented`, default then): one hipGraph per device phase and the collectives
        launched between the replays - nothing about the transport is assumed (works with RCCL and with gloo, whose collectives
        are host code and cannot be captured); `segmented=False` puts the collectives inside one graph (RCCL only).

        With a schedule the captured step begins with emap_train_schedule and follows the schedules from the device iteration counter.
        The warm-up steps (and the step a segmented capture takes) are then ROLLED BACK: parameters, Adam state and the counters are
        what they were before the call, so the first replay is iteration iter_step, exactly as the first eager step() would have been.
        A monitor is rolled back with them: after capture() it holds what it held before (steps == 0 for a new one) and the first
        replay writes the row of iteration iter_step + 1.

        `sampler` (a DeviceRaySampler with near / far; `batch_size` rays, `importance_sample` as runner_udf.py:71-75) in place of
        `rays` / `true_edge`, with a schedule: the sampler's launch - pixel draw, rays, true_edge, t_rand, image
        image_perm[counter % n_images] - is the graph's second node, and ``replay()`` takes no arguments: one replay is one complete
        reference iteration.  The captured region is one linear chain on one stream."""
        batch = None
        if sampler is not None:
            if rays is not None or true_edge is not None:
                raise ValueError("Trainer.capture: pass either rays / true_edge or sampler=, not both")
            if self._sched is None:
                raise ValueError("Trainer.capture(sampler=...) needs a trainer with a schedule (cos_anneal_ratio / flip_saturation must come "
                                 "from the device too)")
            if batch_size is None or int(batch_size) <= 0:
                raise ValueError("Trainer.capture(sampler=...): batch_size must be given")
            batch = lambda: self.sampler_batch(sampler, int(batch_size), importance_sample)
        elif rays is None or true_edge is None:
            raise ValueError("Trainer.capture: rays and true_edge (or sampler=) must be given")
        if self._sched is not None:
            self._check_scheduled(rays or {}, capturing=True)
        if not self.native_tail:
            if segmented:
                raise ValueError("Trainer.capture(segmented=True) needs the native tail (native_tail=True): the per-phase graphs are the "
                                 "native step's four device phases")
            segmented = False
        if segmented is None:
            segmented = _world(self.group) > 1
        if batch is None and rays.get("t_rand") is None and (rays.get("perturb_overwrite", -1) != 0) and self.r.perturb > 0:
            raise ValueError("Trainer.capture: pass rays['t_rand'] explicitly (the reference's CPU-generator jitter draw plus its "
                             "host-to-device copy cannot be part of a device graph)")
        dev = self.flat.data.device
        static = te = None
        if batch is None:
            static = {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in rays.items()}
            te = true_edge.detach().clone()
        one_step = (lambda: self.step(static, te, n_rays_global)) if batch is None else (lambda: self._sampled_step(batch, n_rays_global))
        saved = None
        if self._sched is not None:      # the warm-up is rolled back (see above)
            saved = [(t, t.clone()) for t in self._train_state() + ([sampler._counter] if sampler is not None else [])]
            lag_valid, mon_host = self._lag_valid, self.monitor.host_state() if self.monitor is not None else None
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 1)):
                one_step()
        torch.cuda.current_stream(dev).wait_stream(side)
        graphs, outs = [], []

        def captured(fn):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=graphs[0].pool() if graphs else None):
                outs.append(fn())
            graphs.append(g)
            return g

        if not segmented:
            captured(one_step)
            coll, S = [], None
        else:
            # capture does not execute: every phase is replayed as soon as it is captured and its collectives run, so that this pass is
            # one real step and the next phase is captured on real data
            coll = self._collectives()
            S, phases = self._phases(static, te, n_rays_global, batch)
            _run_phases([lambda ph=ph: captured(ph).replay() for ph in phases], coll, S)
        out = outs[-1]
        keep = self.r.live_buffers()
        if saved is not None:
            for t, was in saved:
                t.copy_(was)
            self._lag_valid = lag_valid
            if self.monitor is not None:
                self.monitor.set_host_state(mon_host)
            self.r.udf_network.invalidate_packed()

        def replay(rays: Optional[Dict] = None, true_edge: Optional[torch.Tensor] = None):
            if batch is not None and (rays is not None or true_edge is not None):
                raise ValueError("replay: this graph draws its own batch (capture(sampler=...)); it takes no arguments")
            if rays is not None and self._sched is not None:
                self._check_scheduled(rays)
            if self.native_tail:
                self.refresh_trainable_mask()     # a set_trainable() between replays reaches the captured Adam through its mask buffer
            if rays is not None:
                for k, v in rays.items():
                    if isinstance(v, torch.Tensor):
                        static[k].copy_(v)
            if true_edge is not None:
                te.copy_(true_edge)
            _run_phases([g.replay for g in graphs], coll, S)
            return out

        replay.graph = graphs[0] if len(graphs) == 1 else None
        replay.graphs = graphs
        replay.segmented = bool(segmented)
        replay._keep = keep
        return replay


    # ---- checkpoints: the reference's dict (runner_udf.py:269-275) plus one namespaced extra ----
    CKPT_VERSION = 1
    _CKPT_KEYS = ("udf_network_fine", "variance_network_fine", "beta_network", "optimizer", "iter_step")

    def _ckpt_modules(self):
        r = self.r
        return {"udf_network_fine": r.udf_network, "variance_network_fine": r.deviation_network, "beta_network": r.beta_network}

    def _ckpt_params(self):
        """The parameters in the order of the reference's optimizer (runner_base.py:106-117): group 0 the UDF network's, group 1 variance,
        second_variance, beta, gamma, zeta (group 2 is empty)."""
        m = self._ckpt_modules()
        return list(m["udf_network_fine"].parameters()), list(m["variance_network_fine"].parameters()) + list(m["beta_network"].parameters())

    def _adam_state(self):
        """-> (m, v: flat moments, the geometry range's step count, [the step count of every tail element]).  The native tail keeps
        exactly this (_FlatAdam).  The torch tail (CPU tests) has one step count for the three scalars: an element carries it while its
        parameter is trainable, 0 otherwise.  Reads step counters: a host synchronisation."""
        n, s0 = self.flat.numel, self.flat.span(self.scalars)[0]
        if self.native_tail:
            a = self._adam
            return a.m, a.v, float(a.t.item()), a.tail_step[:n - s0].tolist()
        m, v, steps = torch.zeros(n, device=self.flat.data.device), torch.zeros(n, device=self.flat.data.device), []
        for p, (a, b) in ((self.p_geo, (0, s0)), (self.p_sc, (s0, n))):
            st = self.optimizer.state.get(p)
            steps.append(float(st["step"]) if st else 0.0)
            if st:
                m[a:b], v[a:b] = st["exp_avg"], st["exp_avg_sq"]
        return m, v, steps[0], [steps[1] if f else 0.0 for f, p in zip(self._scalar_flags(), self.scalars) for _ in range(p.numel())]

    def state_dict(self, sampler=None) -> dict:
        """A checkpoint in the reference's layout (runner_udf.py:269-275) - ``Runner_UDF.load_checkpoint`` reads it - plus ``emap_native``:

          udf_network_fine, variance_network_fine, beta_network   the modules' state_dict(), cloned
          optimizer    what torch.optim.Adam built as in runner_base.py:110-117 over the modules returns from state_dict(): per-parameter
                       step / exp_avg / exp_avg_sq cut from the flat moments (a parameter that never stepped - second_variance, zeta, a
                       frozen variance - has no entry, as in torch); group lr = the schedule's value at the last step taken, or
                       param_groups[*]["lr"] without a schedule
          iter_step    int: the device schedule counter; without a schedule the geometry range's step count
          emap_native  {version, eikonal_sync, lag, lag_valid[, sampler: ``sampler.state_dict()``]}

        Nothing in it aliases a live buffer.  Reading the counters synchronises with the device: this is off the step path.  Every rank
        of a data-parallel run returns the same dict."""
        out = {k: {n: t.detach().clone() for n, t in mod.state_dict().items()} for k, mod in self._ckpt_modules().items()}
        m, v, t_geo, tail = self._adam_state()
        s0 = self.flat.span(self.scalars)[0]
        it = int(self._iter.item()) if self._iter is not None else int(t_geo)
        g = self.optimizer.param_groups
        lr_geo, lr = g[0]["lr"], g[1]["lr"]
        if self.schedule is not None and it > 0:
            lr_geo, lr = self.schedule.values(it - 1)[:2]
        geo, rest = self._ckpt_params()
        # the skeleton (groups, their keys, the parameter numbering) is a stock Adam's of the installed torch: its load_state_dict accepts it
        skel = torch.optim.Adam([{"params": geo, "lr": float(lr_geo)}, {"params": rest}, {"params": []}], lr=float(lr),
                                betas=tuple(g[0]["betas"]), eps=g[0]["eps"])
        for p in geo + rest:
            off = self.flat.offsets.get(id(p))
            step = 0.0 if off is None else (t_geo if off < s0 else tail[off - s0])
            if step > 0:
                k = p.numel()
                skel.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m[off:off + k].view(p.shape).clone(),
                                 "exp_avg_sq": v[off:off + k].view(p.shape).clone()}
        out["optimizer"] = skel.state_dict()
        out["iter_step"] = it
        out["emap_native"] = {"version": self.CKPT_VERSION, "eikonal_sync": self.eikonal_sync, "lag": self._lag.detach().clone(),
                              "lag_valid": bool(self._lag_valid)}
        if sampler is not None:
            out["emap_native"]["sampler"] = sampler.state_dict()
        return out

    def _check_ckpt(self, ckpt, sampler):
        """Everything load_state_dict can refuse, before it writes: -> (m, v, t_geo, tail steps, lag, lag_valid, group lrs / betas / eps,
        the sampler's state or None).  ValueError names the key."""
        E = lambda key, why: ValueError(f"Trainer.load_state_dict: '{key}' {why}")
        for k in self._CKPT_KEYS:
            if k not in ckpt:
                raise E(k, "is missing")
        for k, mod in self._ckpt_modules().items():
            for name, t in mod.state_dict().items():
                if name not in ckpt[k]:
                    raise E(f"{k}.{name}", "is missing")
                if tuple(ckpt[k][name].shape) != tuple(t.shape):
                    raise E(f"{k}.{name}", f"has shape {tuple(ckpt[k][name].shape)}, the module's is {tuple(t.shape)}")
            extra = set(ckpt[k]) - set(mod.state_dict())
            if extra:
                raise E(f"{k}.{sorted(extra)[0]}", "is not a key of the module")
        opt = ckpt["optimizer"]
        for k in ("state", "param_groups"):
            if k not in opt:
                raise E(f"optimizer.{k}", "is missing")
        geo, rest = self._ckpt_params()
        ids = [i for grp in opt["param_groups"] for i in grp["params"]]
        live = [grp for grp in opt["param_groups"] if len(grp["params"])]
        if len(ids) != len(geo) + len(rest) or len(live) != 2 or len(live[0]["params"]) != len(geo):
            raise E("optimizer.param_groups", f"must hold {len(geo)} + {len(rest)} parameters in two non-empty groups (runner_base.py:110-117)")
        n, s0 = self.flat.numel, self.flat.span(self.scalars)[0]
        dev = self.flat.data.device
        m, v, tail, geo_steps = torch.zeros(n, device=dev), torch.zeros(n, device=dev), [0.0] * (n - s0), set()
        for i, p in zip(ids, geo + rest):
            st = opt["state"].get(i)
            if st:
                for k in ("step", "exp_avg", "exp_avg_sq"):
                    if k not in st:
                        raise E(f"optimizer.state[{i}].{k}", "is missing")
                    if k != "step" and tuple(st[k].shape) != tuple(p.shape):
                        raise E(f"optimizer.state[{i}].{k}", f"has shape {tuple(st[k].shape)}, the parameter's is {tuple(p.shape)}")
            step = float(st["step"]) if st else 0.0
            off = self.flat.offsets.get(id(p))
            if off is None:               # second_variance, zeta: not trained here; a reference checkpoint has no state for them either
                continue
            k = p.numel()
            if st:
                m[off:off + k] = st["exp_avg"].reshape(-1).to(dev, torch.float32)
                v[off:off + k] = st["exp_avg_sq"].reshape(-1).to(dev, torch.float32)
            if off < s0:
                geo_steps.add(step)
            else:
                tail[off - s0:off - s0 + k] = [step] * k
        if len(geo_steps) > 1:
            raise E("optimizer.state[*].step", f"of the UDF network's parameters disagree ({sorted(geo_steps)}): they step together here")
        if not self.native_tail and len({x for x in tail if x > 0}) > 1:
            raise E("optimizer.state[*].step", "of variance / beta / gamma disagree: the torch tail keeps one step count for the three")
        it = ckpt["iter_step"]
        if isinstance(it, bool) or not isinstance(it, int) or it < 0:
            raise E("iter_step", f"must be an int >= 0 (got {it!r})")
        nat = ckpt.get("emap_native")
        lag, lag_valid, smp = torch.zeros(2, device=dev), False, None
        if nat is not None:           # (a checkpoint the reference wrote has none: the native extras start afresh)
            if "version" not in nat:
                raise E("emap_native.version", "is missing")
            if int(nat["version"]) > self.CKPT_VERSION:
                raise E("emap_native.version", f"is {nat['version']}: written by a later format than this build's {self.CKPT_VERSION}")
            for k in ("lag", "lag_valid"):
                if k not in nat:
                    raise E(f"emap_native.{k}", "is missing")
            if tuple(nat["lag"].shape) != (2,):
                raise E("emap_native.lag", f"has shape {tuple(nat['lag'].shape)}, not (2,)")
            lag, lag_valid, smp = nat["lag"].to(dev, torch.float32), bool(nat["lag_valid"]), nat.get("sampler")
        if sampler is not None and smp is not None:
            sampler.check_state_dict(smp)
        groups = [(float(grp["lr"]), tuple(grp["betas"]), float(grp["eps"])) for grp in live]
        return m, v, (geo_steps.pop() if geo_steps else 0.0), tail, lag, lag_valid, groups, smp

    @torch.no_grad()
    def load_state_dict(self, ckpt, sampler=None):
        """Resume from `ckpt` - state_dict()'s, or one the reference wrote (no ``emap_native``: the native extras start at their initial
        values, a parameter without optimizer state gets zero moments and step 0, and `sampler`'s counter becomes iter_step, the position
        the runner's ``image_perm[iter_step % len]`` is at).  Everything is validated first (ValueError naming the key: a missing key, a
        shape mismatch, geometry parameters whose step counts disagree, an emap_native.version from the future) and a failed load leaves
        every buffer as it was.  Then every buffer is written IN PLACE - parameters through the modules' own load_state_dict (the views of
        the flat buffer survive), the moments and step counts, the schedule counter, the lagged maxima, the sampler's counter and list -
        so a replay captured before the load goes on from the loaded state without re-capture, and a capture after it rolls its warm-up
        back onto the loaded state.  A monitor is reset() (checkpoints do not carry it).  Without a schedule the group learning rates (betas, eps) are restored as torch restores them; with
        one the schedule is their only source."""
        m, v, t_geo, tail, lag, lag_valid, groups, smp = self._check_ckpt(ckpt, sampler)
        for k, mod in self._ckpt_modules().items():
            mod.load_state_dict(ckpt[k])
        n, s0 = self.flat.numel, self.flat.span(self.scalars)[0]
        if self.native_tail:
            a = self._adam
            a.m.copy_(m); a.v.copy_(v); a.t.fill_(t_geo)
            a.tail_step[:n - s0].copy_(torch.tensor(tail))
        else:
            t_tail = max(tail) if tail else 0.0
            for p, (lo, hi), step in ((self.p_geo, (0, s0), t_geo), (self.p_sc, (s0, n), t_tail)):
                st = self.optimizer.state.get(p)
                if not st:
                    if step <= 0:
                        continue
                    grp = self.optimizer.param_groups[0]
                    on_dev = grp.get("capturable") or grp.get("fused")
                    st = self.optimizer.state[p] = {"step": torch.zeros((), dtype=torch.float32, device=p.device if on_dev else "cpu"),
                                                    "exp_avg": torch.zeros_like(p.data), "exp_avg_sq": torch.zeros_like(p.data)}
                st["step"].fill_(step)
                st["exp_avg"].copy_(m[lo:hi])
                st["exp_avg_sq"].copy_(v[lo:hi])
        if self._iter is not None:
            self._iter.fill_(int(ckpt["iter_step"]))
        else:
            for grp, (lr, betas, eps) in zip(self.optimizer.param_groups, groups):
                grp["lr"], grp["betas"], grp["eps"] = lr, betas, eps
        self._lag.copy_(lag)
        self._lag_valid = lag_valid
        if sampler is not None:
            if smp is not None:
                sampler.load_state_dict(smp)
            else:
                sampler._counter.fill_(int(ckpt["iter_step"]))
        if self.monitor is not None:     # checkpoints do not carry it: a resumed reference run starts with an empty loss_list too (runner_udf.py:53-54)
            self.monitor.reset()
        self.r.udf_network.invalidate_packed()

    def save_checkpoint(self, path, sampler=None):
        """torch.save(state_dict(sampler), path).  Every rank of a data-parallel run calls it (state_dict() is the same on all of them)
        and rank 0 writes."""
        ckpt = self.state_dict(sampler)
        if _world(self.group) == 1 or dist.get_rank(self.group) == 0:
            torch.save(ckpt, path)

    def load_checkpoint(self, path, sampler=None):
        """load_state_dict(torch.load(path, map_location=<the trainer's device>), sampler); returns the checkpoint's dict."""
        ckpt = torch.load(path, map_location=self.flat.data.device)
        self.load_state_dict(ckpt, sampler)
        return ckpt


class FitReports(list):
    """What fit() returns: the reports it handed to `on_report`, in order; ``best_loss`` after the last iteration and ``saved``, the
    iterations at which the best checkpoint was written."""
    best_loss = 1.0

    def __init__(self, *a):
        super().__init__(*a)
        self.saved = []


def fit(trainer, step, n_steps: int, monitor, report_freq: int = 1000, save_freq: int = 1000, val_freq: int = 0, best_path=None, sampler=None,
        on_report=None, on_validate=None, best_loss: float = 1.0) -> FitReports:
    """The cadence of the reference's loop (runner_udf.py:188-247) around `n_steps` calls of ``step()`` - a replay of
    ``trainer.capture(sampler=...)`` or any callable that takes one iteration of a trainer built with ``monitor=monitor``.

      every `report_freq` iterations (:188)   ONE ``monitor.read_rows()`` - record and unread rows from one device-to-host copy - and
                                              ``trainer.check_errors()``; the report
                                              ``{"iter_step", "record", "rows", "best_loss"}`` is appended to the result and handed
                                              to `on_report`
      iter_step % save_freq == 0 (:243-244)   if a loss window has closed and ``loss_avg < best_loss``: ``best_loss = loss_avg`` and
                                              ``trainer.save_checkpoint(best_path, sampler)`` - save_checkpoint's rule (:277-285).  The
                                              reference raises NameError at a save point before the first window closes; here that
                                              point is skipped.  Uses the report's record when the iteration has one, else one read().
      every `val_freq` iterations (:246)      ``on_validate(iter_step)``

    A frequency of 0 (or `best_path` None for the save rule) turns its line off.  There is no other host read: the iteration numbers
    are counted on the host from ``trainer.iter_step``, read once before the first step.  `best_loss` starts at the reference's 1.0
    (:54), or at what a previous call returned.  On several ranks every rank calls fit() with the same arguments (the record's loss
    fields are the global batch's, so all ranks decide alike; save_checkpoint writes on rank 0)."""
    it = trainer.iter_step
    reports = FitReports()
    reports.best_loss = float(best_loss)
    for _ in range(int(n_steps)):
        step()
        it += 1
        rec = None
        if report_freq > 0 and it % report_freq == 0:
            rec, rows = monitor.read_rows()
            trainer.check_errors()
            reports.append({"iter_step": it, "record": rec, "rows": rows, "best_loss": reports.best_loss})
            if on_report is not None:
                on_report(reports[-1])
        if save_freq > 0 and best_path is not None and it % save_freq == 0:
            rec = monitor.read() if rec is None else rec
            if rec["windows"] > 0 and rec["loss_avg"] < reports.best_loss:
                reports.best_loss = rec["loss_avg"]
                trainer.save_checkpoint(best_path, sampler)
                reports.saved.append(it)
        if val_freq > 0 and on_validate is not None and it % val_freq == 0:
            on_validate(it)
    return reports


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` for the drop-in's training loop (runner_base.py:106-117) as ONE kernel launch per step.

    Same constructor shape as ``torch.optim.Adam([{"params": geo, "lr": lr_geo}, {"params": rest}, ...], lr=lr)``: the parameters of
    the first non-empty group become the "geo" range, all later ones the tail.  On the first ``step()`` every parameter is re-homed as a
    view of one flat fp32 buffer (their values, ``requires_grad`` flags and identities are kept - the modules never notice); a
    step then gathers the gradients into one flat buffer (one ``torch.cat``) and calls ``emap_adam_step_masked``: a parameter whose
    ``.grad`` is None (frozen: ``variance`` before ``set_trainable()``) is skipped exactly as torch's Adam skips it and its step
    count starts when it first gets a gradient.  ``param_groups[i]["lr"]`` is read at every step, so the runner's schedulers work
    unchanged.  Replaces 32 tensors x ~6 element-wise launches of the stock optimizer."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        if not self._live_groups():
            raise ValueError("FusedAdam: no parameters")
        if len({g["lr"] for g in self._tail_groups}) > 1:
            raise ValueError("FusedAdam: the groups behind the first one must share one learning rate (the runner's do)")
        self._flat = None

    # The groups are looked up in ``self.param_groups`` at every use: ``Optimizer.load_state_dict`` / ``__setstate__`` REPLACE the group
    # dicts, and the runner's schedulers write ``lr`` into whatever dicts ``optimizer.param_groups`` holds at that time
    # (runner_base.py:128-150) - a reference bound in __init__ would keep reading the construction-time learning rate after a resume.
    def _live_groups(self):
        return [g for g in self.param_groups if len(g["params"])]

    @property
    def _geo_group(self):
        return self._live_groups()[0]

    @property
    def _tail_groups(self):
        return self._live_groups()[1:]

    @classmethod
    def from_adam(cls, adam: torch.optim.Optimizer) -> "FusedAdam":
        """A FusedAdam over the SAME parameter groups as a ``torch.optim.Adam`` (runner_base.py:106-117), taking over its learning rates,
        betas, eps and - if it has stepped already - its state (checkpoint layout, load_state_dict)."""
        groups = []
        for g in adam.param_groups:
            if g.get("amsgrad") or g.get("weight_decay") or g.get("maximize"):
                raise NotImplementedError("FusedAdam.from_adam: amsgrad / weight_decay / maximize are not implemented")
            groups.append({"params": list(g["params"]), "lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"]})
        g0 = next(g for g in groups if g["params"])
        opt = cls(groups, lr=g0["lr"], betas=g0["betas"], eps=g0["eps"])
        if len(adam.state):
            opt.load_state_dict(adam.state_dict())
        return opt

    def _build(self):
        geo = list(self._geo_group["params"])
        tail = [p for g in self._tail_groups for p in g["params"]]
        grads = [p.grad for p in geo + tail]    # FlatParams points .grad at its own flat buffer; this optimizer takes the gradients autograd
        self._flat = FlatParams(geo + tail)     # (or the caller) put there, so they are put back
        for p, g_ in zip(geo + tail, grads):
            p.grad = g_
        self._geo, self._tail = geo, tail
        self._adam = _FlatAdam(self._flat.numel, sum(p.numel() for p in geo), [p.numel() for p in tail], self._flat.data.device)
        self._zeros = {}

    # ---- checkpointing (runner_udf.py:260 saves optimizer.state_dict(), :273 loads it): torch.optim.Adam's per-parameter layout ----
    def _mirror_state(self):
        """Expose the flat moments as ``self.state[p] = {step, exp_avg, exp_avg_sq}`` (views of the flat buffers, torch.optim.Adam's
        keys), so that ``Optimizer.state_dict()`` writes a checkpoint a stock Adam can load and vice versa.  A parameter that has
        never been stepped (frozen so far) has no entry, exactly like torch's Adam.  Reads the step counters: a host sync."""
        A = self._adam
        t_geo = float(A.t.item())
        tail_steps = A.tail_step.tolist()
        self.state.clear()
        for p in self._geo + self._tail:
            a, b = self._flat.span([p])
            step = t_geo if a < A.n_geo else float(tail_steps[a - A.n_geo])
            if step <= 0:
                continue
            self.state[p] = {"step": torch.tensor(step, dtype=torch.float32), "exp_avg": A.m[a:b].view(p.shape),
                             "exp_avg_sq": A.v[a:b].view(p.shape)}

    def state_dict(self):
        if self._flat is not None:
            self._mirror_state()
        return super().state_dict()

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts a checkpoint of this class or of ``torch.optim.Adam`` over the same parameter groups: moments and step counts go into
        the flat buffers (the geometry range has ONE step counter - its parameters always step together; every tail element its own)."""
        super().load_state_dict(state_dict)           # validates the groups, casts the tensors to the parameters' device
        if self._flat is None:
            self._build()
        A = self._adam
        A.m.zero_(); A.v.zero_(); A.t.zero_(); A.tail_step.zero_()
        t_geo = 0.0
        for p in self._geo + self._tail:
            st = self.state.get(p)
            if not st:
                continue
            a, b = self._flat.span([p])
            A.m[a:b].copy_(st["exp_avg"].reshape(-1))
            A.v[a:b].copy_(st["exp_avg_sq"].reshape(-1))
            step = float(st["step"])
            if a < A.n_geo:
                t_geo = max(t_geo, step)
            else:
                A.tail_step[a - A.n_geo:b - A.n_geo] = step
        A.t.fill_(t_geo)
        A.flags = None                                # the next step writes the mask afresh
        self._mirror_state()

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        if self._flat is None:
            self._build()
        dev = self._flat.data.device
        parts = []
        # the geometry gradients may already BE one flat buffer (RenderFn.backward with direct_param_grads, or a Trainer-style caller):
        # consecutive fp32 views in this optimizer's order -> no gather
        geo_ptr, off = None, 0
        for p in self._geo:
            g_ = p.grad
            if g_ is None:
                raise NotImplementedError("FusedAdam: a parameter of the first group without gradient")
            if off == 0:
                geo_ptr = g_.data_ptr()
            if geo_ptr is not None and (g_.dtype != torch.float32 or not g_.is_contiguous() or g_.data_ptr() != geo_ptr + 4 * off):
                geo_ptr = None
            off += p.numel()
        if geo_ptr is None:
            parts = [p.grad.reshape(-1) for p in self._geo]
        for p in self._tail:
            if p.grad is not None:
                parts.append(p.grad.reshape(-1))
            else:
                z = self._zeros.get(p.numel())
                if z is None:
                    z = self._zeros[p.numel()] = torch.zeros(p.numel(), device=dev)
                parts.append(z)
        self._adam.set_mask(p.grad is not None for p in self._tail)      # changes rarely: a set_trainable() of the runner
        live = self._live_groups()              # the CURRENT group dicts (see _live_groups): lr is read per step
        geo_group, tail_groups = live[0], live[1:]
        lr_tail = tail_groups[0]["lr"] if tail_groups else geo_group["lr"]
        # geo_ptr: the geometry range straight from the caller's flat gradient buffer, the few tail scalars gathered as before
        grad = torch.cat(parts) if parts else None
        self._adam.step(self._flat.data, grad, geo_group["lr"], lr_tail, geo_group["betas"], geo_group["eps"], geo_grad_ptr=geo_ptr)
        # the in-place flat update is invisible to the per-tensor version counters UDFNetwork.packed() keys its fragment cache on
        inc = getattr(torch.autograd.graph, "increment_version", None)
        for p in self._geo:
            if inc is not None:
                inc(p)
            else:
                p.add_(0.0)
        return loss


# ---------------------------------------------------------------------------------------------
# generic autograd-based step (any differentiable render_fn; used with the drop-in classes and by the CPU tests)
# ---------------------------------------------------------------------------------------------
def training_step(render_fn: Callable[[], Dict[str, torch.Tensor]], true_edge: torch.Tensor, flat: FlatParams, optimizer,
                  edge_weight: float = 1.0, igr_weight: float = 0.1, igr_ns_weight: float = 0.0, group=None,
                  n_rays_global: Optional[int] = None):
    """One optimizer step on this rank's ray shard through autograd; equals the single-process step on the global batch.

    render_fn() -> render dict for this rank's rays (must contain "edge", "gradient_error", "gradient_error_near_surface" and
    "eikonal_sums" = [sum(relax*err), sum(relax), sum(near*err), sum(near)]).  `flat` holds the parameters (FlatParams): the
    gradients accumulate into its flat buffer and ONE all-reduce covers them.  Returns (loss_global, edge_loss_global)."""
    world = _world(group)
    out = render_fn()
    edge = out["edge"]
    n_local = edge.shape[0]
    n_glob = n_rays_global if n_rays_global is not None else n_local * world
    sums = out["eikonal_sums"].detach()
    mse_sum = ((edge - true_edge) ** 2).sum()
    stats = torch.stack([sums[1], sums[3], sums[0], sums[2], mse_sum.detach()]).to(torch.float32)      # the order of _loss_from_stats
    if world > 1:
        dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=group)   # global mask counts before backward (+ the loss statistics)
    # local numerators with gradient: ge_local * (c_local + 1e-5)
    e_rel = out["gradient_error"] * (sums[1] + 1e-5)
    e_ns = out["gradient_error_near_surface"] * (sums[3] + 1e-5)
    n_elem_glob = n_glob * (edge.numel() // n_local)
    loss_local = mse_sum / n_elem_glob * edge_weight + e_ns / (stats[1] + 1e-5) * igr_ns_weight + e_rel / (stats[0] + 1e-5) * igr_weight
    flat.grad.zero_()
    for p in flat.params:
        p.grad = flat.grad[flat.offsets[id(p)]:flat.offsets[id(p)] + p.numel()].view(p.shape)   # autograd accumulates in place
    loss_local.backward()
    if world > 1:
        dist.all_reduce(flat.grad, op=dist.ReduceOp.SUM, group=group)
    optimizer.step()
    return _loss_from_stats(stats, n_elem_glob, edge_weight, igr_weight, igr_ns_weight)
