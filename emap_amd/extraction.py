"""Dense-grid extraction queries (SURVEY par. 8 f2): the second consumer of the UDF field kernels.

Mirrors of ``get_udf_normals_grid``, ``get_udf_normals_slow`` and ``get_pointcloud_from_udf`` (src/edge_extraction/extract_pointcloud.py:5-95,
:98-193, :212-293): same arguments, same return values, same jitter draws (one ``torch.randn((n, sampling_N, 3), device=device)`` per
``max_batch`` points of a stage, in the same order), but
  * the grid, the thresholded subset and all jittered neighbourhoods are evaluated in a few launches of up to 2^20 points
    instead of the reference's N^3/4096 + 51 x n/4096 latency-bound calls of 4096 points - for ANY ``func`` / ``func_grad`` that acts point by point,
    in particular the closure ``Runner_UDF.extract_edge`` passes (runner_udf.py:520-527: ``udf_network.gradient`` followed by a normalisation),
  * the line direction ``F.normalize(torch.linalg.svd(grad_ld)[2][:, -1, :])`` (:86-88) is one HIP kernel over the
    3x3 matrices G^T G (``emap_null_direction``): no 50x3 SVD batch.
There is no CPU fallback: tensors must live on the GPU and libemap_hip.so must be loadable.

ONE evaluator (``_evaluator``) stands between the three routines and the callables.  It decides what ``(func, func_grad)`` are, and with
that how a point set is cut into calls.  The cut is part of the RESULT, to the last bit: the kernel that computes the gradient is chosen
by launch size (forward-mode tangents below 8 193 points, the reverse sweep above).  With B = ``_BIG``, M = ``_MAX_BATCH``:

  kind        what the callables are                                           the two query routines       get_pointcloud_from_udf
  fused       the network's own bound ``udf`` and ``gradient``                 hip_udf per B                streamed, hip_udf per B
  closure     bound ``udf`` + a callable that holds THAT network (rule 2)      point-wise if rule 1 sees    streamed: values hip_udf,
                                                                               the network, else opaque     gradients the closure, per B
  point-wise  both callables evaluate a package network (rule 1)               func / func_grad per B       composed (the query routines)
  opaque      anything else (may not act point by point, max_batch may bound   per max_batch, x sampling_N  composed
              its memory)                                                      for a neighbourhood
  grid: lattice values, gradients of the df < thr subset, the flattened n x sampling_N neighbourhood.  slow: fused: ONE hip_udf(with_grad=
  True) per B gives value and gradient; otherwise func, then func_grad; neighbourhood.  streamed: lattice per B; subset gradients per B;
  neighbourhoods in groups of max(B // (sampling_N x M), 1) x M points (whole draws, no tensor above B points), one call per group; per
  shift value + gradient per B; the last shift's neighbourhoods with the reference's 50 / 5e-3.
"""
import torch

from . import _lib

_BIG = 1 << 20          # points per launch of the fast path (bounds the temporaries: 12 MB in, 16 MB out)


def _gpu(device):
    if torch.device(device).type != "cuda":
        raise RuntimeError("emap_amd.extraction runs on the GPU only (no CPU fallback)")
    return torch.device(device)


def null_direction(grads: torch.Tensor) -> torch.Tensor:
    """(n, k, 3) gradient samples -> (n, 3) unit direction of least variation (sign arbitrary), extract_pointcloud.py:86-88."""
    _lib.require_cuda(grads, "grads")
    n, k = int(grads.shape[0]), int(grads.shape[1])
    g = _lib.f32c(grads)
    out = torch.empty(n, 3, device=g.device, dtype=torch.float32)
    if n:
        with _lib.on_device(g):
            _lib.api().null_direction(g, n, k, out, _lib.stream_ptr(g.device))
    return out


# what the callables are: one walk over what a callable holds, two owner rules, one evaluator
def _captured(f):
    """The objects a callable holds: its ``__self__``, the contents of its non-empty closure cells, its ``__defaults__``."""
    cells = []
    for c in (getattr(f, "__closure__", None) or ()):
        try:
            cells.append(c.cell_contents)
        except ValueError:                                   # an empty cell
            pass
    return [o for o in (getattr(f, "__self__", None), *cells, *(getattr(f, "__defaults__", None) or ())) if o is not None]


# The two owner rules below DISAGREE, and are kept apart on purpose: rule 1 sees an owner only through an attribute called
# ``udf_network``, rule 2 through any attribute or registered module.  So the runner's closure (its network is ``udf_network_fine``)
# streams through get_pointcloud_from_udf but gets max_batch chunks when handed straight to the two query routines.  Known and
# deferred: unifying them changes launch sizes, hence bits.
def _uses_package_net(f) -> bool:
    """Rule 1 (chunk size): ``f`` evaluates this package's UDFNetwork point by point - the network's own bound methods, or a closure
    over a network / over an object whose ``udf_network`` is one.  Such callables are driven with 2^20-point launches."""
    from .udf_model import UDFNetwork
    return any(isinstance(o, UDFNetwork) or isinstance(getattr(o, "udf_network", None), UDFNetwork) for o in _captured(f))


def _closes_over(f, net) -> bool:
    """Rule 2 (streaming): ``f`` holds ``net`` itself or an object one of whose attributes IS ``net`` - whatever the attribute is
    called.  The runner's closure holds the runner (``self``), whose network is ``self.udf_network_fine`` (runner_udf.py:520-527)."""
    def holds(o):
        if o is net:
            return True
        try:
            values = list(vars(o).values())
        except TypeError:
            return False
        values += list(getattr(o, "_modules", {}).values()) if isinstance(getattr(o, "_modules", None), dict) else []
        return any(v is net for v in values)
    return any(holds(o) for o in _captured(f))


def _cat(parts, pts, width):
    return (parts[0] if len(parts) == 1 else torch.cat(parts)).reshape(-1, width) if parts else pts.new_empty((0, width))


class _Evaluator:
    """The field behind ``(func, func_grad)``: ``kind`` as in the module docstring's table, ``net`` the network of the fused and closure
    kinds.  Owns the chunk rule, the ``detach`` and the shapes; an empty point set is answered without a call."""

    def __init__(self, kind, net, func, func_grad, pointwise, max_batch, streamed):
        self.kind, self.net, self.func, self.func_grad, self.max_batch = kind, net, func, func_grad, max_batch
        self.fused, self.streams = kind == "fused", kind in ("fused", "closure")
        self.direct = self.fused or (streamed and self.streams)      # values from the network's kernel, not through ``func``
        self.big = self.direct or pointwise

    def chunk(self, mult=1):
        """Points per call; ``mult`` = sampling_N for a flattened neighbourhood.  Reads the module constants at call time."""
        return _BIG if self.big else max(int(_MAX_BATCH if self.max_batch is None else self.max_batch) * mult, 1)

    def _each(self, fn, pts, mult=1):
        c = self.chunk(mult)
        return [fn(pts[h:h + c]) for h in range(0, int(pts.shape[0]), c)]

    def values(self, pts):                                    # (P, 3) -> (P, 1)
        fn = (lambda p: self.net.hip_udf(p, with_grad=False)[0]) if self.direct else (lambda p: self.func(p)[0].detach())
        return _cat(self._each(fn, pts), pts, 1)

    def gradients(self, pts, mult=1):                         # (P, 3) -> (P, 3), whether the callable returns (P, 3) or, as ``UDFNetwork.gradient``, (P, 1, 3)
        fn = (lambda p: self.net.hip_udf(p, with_grad=True)[1]) if self.fused else (lambda p: self.func_grad(p).detach().reshape(-1, 3))
        return _cat(self._each(fn, pts, mult), pts, 3)

    def values_and_gradients(self, pts):
        if not self.fused:
            return self.values(pts), self.gradients(pts)
        res = self._each(lambda p: self.net.hip_udf(p, with_grad=True), pts)          # the fused kernel gives both
        return _cat([r[0] for r in res], pts, 1), _cat([r[1] for r in res], pts, 3)


def _evaluator(func, func_grad, max_batch=None, streamed=False):
    """The one classification of ``(func, func_grad)``.  ``streamed``: closure values from the network's kernel, everything per ``_BIG``."""
    from .udf_model import UDFNetwork
    net, kind = getattr(func, "__self__", None), None
    if isinstance(net, UDFNetwork) and getattr(func, "__name__", "") == "udf":
        if getattr(func_grad, "__self__", None) is net and getattr(func_grad, "__name__", "") == "gradient":
            kind = "fused"
        elif callable(func_grad) and _closes_over(func_grad, net):
            kind = "closure"         # a closure over any other network, or over nothing recognisable, does not stream
    pointwise = _uses_package_net(func) and _uses_package_net(func_grad)
    if kind is None:
        kind, net = ("point-wise" if pointwise else "opaque"), None
    return _Evaluator(kind, net, func, func_grad, pointwise, max_batch, streamed)


def _draw(n, sampling_N, max_batch, device):
    """The reference's draw sequence: one randn per ``max_batch`` points of a stage, in order (:75-79, :163-167)."""
    return torch.cat([torch.randn((min(max_batch, n - h), sampling_N, 3), device=device) for h in range(0, n, max_batch)])


def _line_directions(ev, pts, sampling_N, sampling_delta, noise, max_batch, group=None):
    """(n, 3) null direction of the gradients in a jittered neighbourhood of every point (:75-88).  ``noise`` (n, sampling_N, 3)
    replaces the draws.  ``group``: points per neighbourhood tensor - the whole set, or a multiple of ``max_batch`` (whole draws)."""
    n = int(pts.shape[0])
    if noise is not None and tuple(noise.shape) != (n, sampling_N, 3):
        raise ValueError(f"noise {tuple(noise.shape)} given for a stage of {n} points x {sampling_N} samples")
    out = torch.empty(n, 3, device=pts.device)
    group = group or max(n, 1)
    for h in range(0, n, group):
        t = min(h + group, n)
        z = _draw(t - h, sampling_N, max_batch, pts.device) if noise is None else noise[h:t]
        g = ev.gradients(jitter_points(pts[h:t], z, sampling_delta), mult=sampling_N)
        out[h:t] = null_direction(g.reshape(t - h, sampling_N, 3))
    return out


def get_udf_normals_grid(func, func_grad, N, udf_threshold, is_linedirection=False, sampling_N=50, sampling_delta=0.005,
                         max_batch=int(2 ** 12), device="cuda", noise=None):
    """See the module docstring.  ``noise`` (n_below_threshold, sampling_N, 3) replaces the jitter draws (parity tests)."""
    device = _gpu(device)
    ev = _evaluator(func, func_grad, max_batch)
    # the N^3 lattice on [-1, 1]^3, first coordinate slowest (the reference's point order and fp32 arithmetic, :36-54: index * 2/(N-1) - 1)
    voxel_size = 2.0 / (N - 1)
    axis = torch.arange(N, device=device, dtype=torch.float32) * voxel_size + (-1)
    samples = torch.zeros(N ** 3, 12, device=device)
    samples[:, :3] = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(-1, 3)

    with torch.no_grad():
        samples[:, 3:4] = ev.values(samples[:, :3].contiguous())
        norm_idx = torch.where(samples[:, 3] < udf_threshold)[0]            # :64-65
        sub = samples[norm_idx, :3].contiguous()
        # the reference normalises the (P,1,3) gradient along dim=1 - the singleton - i.e. per component (:71)
        samples[norm_idx, 4:7] = -torch.nn.functional.normalize(ev.gradients(sub).reshape(-1, 1, 3), dim=1)[:, 0]
        if is_linedirection:
            samples[norm_idx, 8:11] = _line_directions(ev, sub, sampling_N, sampling_delta, noise, max_batch)

    df_values = samples[:, 3].reshape(N, N, N)
    vecs = samples[:, 4:7].reshape(N, N, N, 3)
    ld = samples[:, 8:11].reshape(N, N, N, 3)
    return df_values, ld, vecs, samples, torch.tensor(voxel_size)


def get_udf_normals_slow(func, func_grad, voxel_size, xyz, is_linedirection, sampling_N=50, sampling_delta=0.005,
                         max_batch=int(2 ** 12), device="cuda", noise=None):
    """Mirror of ``get_udf_normals_slow`` (extract_pointcloud.py:98-193): values, normals (-grad/|grad|) and optional line
    directions at arbitrary points ``xyz`` (n,3).  Same return tuple ``(df_values, normals, ld, samples)`` with the
    reference's 13-column ``samples``; ``voxel_size`` is unused there as well."""
    device = _gpu(device)
    ev = _evaluator(func, func_grad, max_batch)
    xyz = xyz.to(device).float()
    samples = torch.cat([xyz, torch.zeros(xyz.shape[0], 10, device=device)], dim=-1)
    with torch.no_grad():
        pts = samples[:, 0:3].contiguous()
        df, grad = ev.values_and_gradients(pts)
        samples[:, 3] = df.squeeze(-1)
        samples[:, 4:7] = -torch.nn.functional.normalize(grad, dim=1)                     # :158-160
        if is_linedirection:
            samples[:, 7:10] = _line_directions(ev, pts, sampling_N, sampling_delta, noise, max_batch)    # :163-167
    return samples[:, 3], samples[:, 4:7], samples[:, 7:10], samples


# ---------------------------------------------------------------------------------------------------------------------------------
# get_pointcloud_from_udf (extract_pointcloud.py:212-293), streamed: the lattice is walked in chunks of _BIG points, the points
# below the threshold are appended to survivor buffers by a stable compaction kernel, and everything after the value pass
# (gradients, jitter neighbourhoods, null directions, shifts) touches survivors only.  Nothing of size N^3 is allocated.
_SURVIVORS0 = 1 << 16    # initial capacity of the survivor buffers (points); they double when the compaction reports an overflow
_SLOW_SAMPLING_N, _SLOW_SAMPLING_DELTA, _MAX_BATCH = 50, 0.005, 1 << 12    # what the reference's shift stage runs with (:274-281)


def lattice_points(N, first, count, device="cuda", out=None):
    """Points [first, first + count) of the N^3 lattice on [-1, 1]^3, first coordinate slowest: (count, 3), bit-identical to
    ``arange(N) * (2 / (N - 1)) + (-1)`` (the order and fp32 arithmetic of ``get_udf_normals_grid``)."""
    device = _gpu(device)
    count = int(count)
    if out is None:
        xyz = torch.empty(count, 3, device=device, dtype=torch.float32)
    else:
        if not (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[1] == 3 and out.is_contiguous()
                and out.shape[0] >= count):
            raise ValueError(f"lattice_points: `out` must be a contiguous float32 GPU tensor of at least ({count}, 3)")
        xyz = out[:count]
    with _lib.on_device(xyz):
        _lib.api().lattice_points(int(N), int(first), count, xyz, _lib.stream_ptr(xyz.device))
    return xyz


def jitter_points(x, noise, delta):
    """(n, 3) points, (n, k, 3) noise -> (n * k, 3) = ``(x.unsqueeze(1) + delta * noise).reshape(-1, 3)``, bit-identical."""
    _lib.require_cuda(x, "x")
    x, noise = _lib.f32c(x), _lib.f32c(noise.to(x.device))
    n, k = int(noise.shape[0]), int(noise.shape[1])
    if x.shape != (n, 3) or noise.shape != (n, k, 3):
        raise ValueError(f"jitter_points: x {tuple(x.shape)} and noise {tuple(noise.shape)} do not match")
    out = torch.empty(n * k, 3, device=x.device, dtype=torch.float32)
    with _lib.on_device(x):
        _lib.api().jitter_points(x, noise, n, k, delta, out, _lib.stream_ptr(x.device))
    return out


def shift_points(x, df, normals):
    """``x + df.unsqueeze(-1) * normals`` (extract_pointcloud.py:273), bit-identical."""
    _lib.require_cuda(x, "x")
    x, df, normals = _lib.f32c(x), _lib.f32c(df).reshape(-1), _lib.f32c(normals)
    n = int(x.shape[0])
    if x.shape != (n, 3) or normals.shape != (n, 3) or df.shape != (n,):
        raise ValueError("shift_points: x (n, 3), df (n), normals (n, 3) expected")
    out = torch.empty_like(x)
    with _lib.on_device(x):
        _lib.api().shift_points(x, df, normals, n, out, _lib.stream_ptr(x.device))
    return out


class Compactor:
    """Survivor buffers ``xyz`` (capacity, 3), ``df`` (capacity), ``idx`` (capacity, int64) filled by ``emap_compact_append``.
    ``append`` only enqueues; ``finish`` is the one host read of the device state: it returns the number of appended CALLS (all of them unless a
    call overflowed the capacity - then the buffers have been grown and the caller repeats from that call)."""

    def __init__(self, device, capacity=_SURVIVORS0):
        self.device, self.capacity = torch.device(device), max(int(capacity), 1)
        self.state = torch.zeros(4, dtype=torch.int64, device=self.device)
        self.ws = None
        self.count = 0
        self._alloc(self.capacity)

    def _alloc(self, cap, keep=0):
        old = (self.xyz, self.df, self.idx) if keep else None
        self.xyz = torch.empty(cap, 3, device=self.device)
        self.df = torch.empty(cap, device=self.device)
        self.idx = torch.empty(cap, dtype=torch.int64, device=self.device)
        if keep:
            for new, o in zip((self.xyz, self.df, self.idx), old):
                new[:keep] = o[:keep]
        self.capacity = cap

    def append(self, df, xyz, threshold, inclusive, first_index=0):
        _lib.require_cuda(df, "df")
        _lib.require_cuda(xyz, "xyz")
        df, xyz = _lib.f32c(df).reshape(-1), _lib.f32c(xyz)
        n = int(df.shape[0])
        if xyz.shape != (n, 3) or df.device != self.state.device or xyz.device != self.state.device:
            raise ValueError(f"Compactor.append: df ({n}) and xyz {tuple(xyz.shape)} must be n and (n, 3) on {self.state.device}")
        if n == 0:
            return
        nb = _lib.size_of("compact_workspace_bytes", n)
        if self.ws is None or self.ws.numel() < nb:
            self.ws = torch.empty(nb, dtype=torch.uint8, device=self.device)
        with _lib.on_device(df):
            _lib.api().compact_append(df, xyz, n, int(first_index), threshold, int(bool(inclusive)), self.xyz, self.df, self.idx,
                                      self.capacity, self.state, self.ws, self.ws.numel(), _lib.stream_ptr(df.device))

    def finish(self):
        """-> (survivors so far, calls appended so far, overflowed).  After an overflow the buffers are already larger and the error
        flag is cleared: repeat the calls from number ``calls`` on."""
        count, err, calls, need = self.state.tolist()
        if err:
            self._alloc(max(2 * self.capacity, int(need)), keep=count)
            self.state[1] = 0
        self.count = count
        return count, calls, bool(err)

    def result(self):
        n = self.count
        return self.xyz[:n], self.df[:n], self.idx[:n]

    def run(self, heads, append_from):
        """``append_from(h)`` for every h of ``heads``; after an overflow the calls are repeated from the one that did not fit.  -> ``result()``"""
        done = 0
        while True:
            for h in heads[done:]:
                append_from(h)
            _, done, overflowed = self.finish()
            if not overflowed:
                return self.result()


def compact(df, xyz, threshold, inclusive, capacity=_SURVIVORS0, chunk=_BIG):
    """Order-preserving ``(xyz[mask], df[mask], torch.where(mask)[0])`` with ``mask = df <= threshold`` (inclusive) or
    ``df < threshold``: the input goes through the compaction kernel in chunks, the survivor buffers grow when a chunk reports
    that it does not fit, and that chunk is repeated."""
    _lib.require_cuda(df, "df")
    df = _lib.f32c(df).reshape(-1)
    xyz = _lib.f32c(xyz)
    c = Compactor(df.device, capacity)
    return c.run(range(0, int(df.shape[0]), chunk), lambda h: c.append(df[h:h + chunk], xyz[h:h + chunk], threshold, inclusive, first_index=h))


def _stream_fns(func, func_grad):
    """(net, grad) for the streamed path - grad None: the fused kind - or None: the composed path.  A view of the one classification."""
    ev = _evaluator(func, func_grad)
    return (ev.net, None if ev.fused else func_grad) if ev.streams else None


def _pointcloud_stream(net, grad_fn, N, thr, sampling_N, sampling_delta, is_pointshift, iters, is_linedirection, device, noise, trace=None):
    """The streamed routine on what ``_stream_fns`` returned; returns device tensors (points, line directions).  Host reads per stage: the
    compaction state, once (again after a grown buffer), plus at the grid stage the index build of the df < thr subset.
    ``trace`` is TEST-ONLY scaffolding and not reachable through the public function: a dict that receives references (no copies)
    to each stage's lattice indices, which the parity test needs to align the reference's recorded jitter rows with this run's
    point sets.  Production callers leave it None."""
    F = torch.nn.functional
    ev = _evaluator(net.udf, grad_fn or net.gradient, streamed=True)
    noise = iter(noise) if noise is not None else iter(())

    def directions(pts, sampling_N, sampling_delta):
        # groups of whole _MAX_BATCH draws (the reference's: one randn per 4096 points, in order), no neighbourhood tensor above _BIG points
        return _line_directions(ev, pts, sampling_N, sampling_delta, next(noise, None), _MAX_BATCH,
                                group=max(_BIG // (sampling_N * _MAX_BATCH), 1) * _MAX_BATCH)

    total = N ** 3
    with torch.no_grad():
        # grid stage: value pass + compaction of clamp(df, 0) <= thr.  For thr >= 0 that set is df <= thr, which also holds every
        # point of the normals' set df < thr; for thr < 0 it is empty while df < thr may not be - then the raw set is kept.
        c = Compactor(device)
        buf = torch.empty(min(_BIG, total), 3, device=device)

        def walk(h):
            xyz = lattice_points(N, h, min(_BIG, total - h), device, out=buf)
            c.append(ev.values(xyz), xyz, thr, thr >= 0, first_index=h)
        xyz, df, idx = c.run(range(0, total, _BIG), walk)
        del buf
        below = torch.where(df < thr)[0]                                    # :65 - normals and directions live here (the stage's one index build)
        sub = xyz[below]
        n = int(xyz.shape[0])
        normals, lds = torch.zeros(n, 3, device=device), torch.zeros(n, 3, device=device)
        normals[below] = -F.normalize(ev.gradients(sub).reshape(-1, 1, 3), dim=1)[:, 0]    # per component: the reference's dim=1 on (P, 1, 3), :72
        if is_linedirection:
            lds[below] = directions(sub, sampling_N, sampling_delta)
        if trace is not None:
            trace["grid"] = dict(idx=idx, below=below, df=df)
        # :259-262, clamp(df, 0) <= thr: every compacted point for thr >= 0 (df <= thr, and a negative df clamps to 0), none for thr < 0
        if thr >= 0:
            df = df.clamp(min=0)
        else:
            xyz, df, idx, normals, lds = xyz[:0], df[:0], idx[:0], normals[:0], lds[:0]

        if is_pointshift and iters > 0:
            for it in range(iters):
                shifted = shift_points(xyz, df, normals)                    # :273
                n = int(shifted.shape[0])
                sdf, grad = ev.values_and_gradients(shifted)
                sdf = sdf.reshape(-1)
                snormals = -F.normalize(grad, dim=1)                        # :160-161
                # the last shift: the reference's own sampling_N / delta here, not the caller's
                slds = directions(shifted, _SLOW_SAMPLING_N, _SLOW_SAMPLING_DELTA) if it == iters - 1 else torch.zeros(n, 3, device=device)
                sxyz, sdf_kept, src = compact(sdf, shifted, thr, True, capacity=n)      # :282
                if trace is not None:
                    trace[f"shift{it}"] = dict(idx=idx, df=sdf, xyz=shifted, kept=src)
                xyz, df, idx, normals, lds = sxyz, sdf_kept, idx[src], snormals[src], slds[src]
        if trace is not None:
            trace["final_idx"] = idx
    return xyz, lds


def _pointcloud_composed(func, func_grad, N_MC, udf_threshold, sampling_N, sampling_delta, is_pointshift, iters, is_linedirection,
                         device, noise):
    """Any other callable: the reference's own composition of the two query routines (extract_pointcloud.py:240-293).  Not bit-identical
    to the streamed routine (other launch shapes), and the only path for callables that cannot stream."""
    noise = iter(noise) if noise is not None else iter(())
    df, lds, normals, samples, voxel_size = get_udf_normals_grid(
        func, func_grad, N_MC, udf_threshold, is_linedirection, sampling_N, sampling_delta, device=device,
        noise=next(noise, None) if is_linedirection else None)
    df, lds, normals, xyz = df.reshape(-1), lds.reshape(-1, 3), normals.reshape(-1, 3), samples.reshape(-1, 12)[:, 0:3]
    df = df.clamp(min=0)
    keep = df <= udf_threshold
    xyz, lds, normals, df = xyz[keep], lds[keep], normals[keep], df[keep]
    if is_pointshift and iters > 0:
        for it in range(iters):
            last = it == iters - 1
            shifted = xyz + df.unsqueeze(-1) * normals
            sdf, snormals, lds, _ = get_udf_normals_slow(func, func_grad, voxel_size, shifted, last, device=device,
                                                         noise=next(noise, None) if last else None)
            keep = sdf <= udf_threshold
            xyz, df, normals, lds = shifted[keep], sdf[keep], snormals[keep], lds[keep]
    return xyz, lds


def get_pointcloud_from_udf(func, func_grad, N_MC=128, udf_threshold=1.0, sampling_N=50, sampling_delta=5e-3, is_pointshift=False,
                            iters=1, is_linedirection=False, device="cuda", noise=None):
    """Mirror of ``get_pointcloud_from_udf`` (extract_pointcloud.py:212-293): the edge point cloud of the N_MC^3 lattice and its line
    directions, two numpy arrays ``(points (n, 3), line_directions (n, 3))``.  See the section comment above for the streamed path
    (taken for this package's ``UDFNetwork.udf`` with its ``.gradient`` or a closure over the network); any other callable goes
    through ``get_udf_normals_grid`` / ``get_udf_normals_slow`` as in the reference.  ``noise``: a list with one (n_stage,
    sampling_N, 3) tensor per stage that draws jitter, in order - the grid stage (if ``is_linedirection``; rows follow the lattice
    points with df < threshold) and the last shift iteration (always 50 samples there, as in the reference) - replacing the randn draws."""
    device = _gpu(device)
    N_MC, thr = int(N_MC), float(udf_threshold)
    fns = _stream_fns(func, func_grad)
    if fns is not None:
        xyz, lds = _pointcloud_stream(*fns, N_MC, thr, int(sampling_N), float(sampling_delta), is_pointshift, int(iters),
                                      is_linedirection, device, noise)
    else:
        xyz, lds = _pointcloud_composed(func, func_grad, N_MC, thr, sampling_N, sampling_delta, is_pointshift, int(iters),
                                        is_linedirection, device, noise)
    return xyz.cpu().numpy(), lds.cpu().numpy()
