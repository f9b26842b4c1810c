"""Dense-grid extraction queries (SURVEY par. 8 f2): the second consumer of the UDF field kernels.

Mirror of ``get_udf_normals_grid`` (src/edge_extraction/extract_pointcloud.py:5-95): same arguments, same return tuple,
same jitter draws (one ``torch.randn((n, sampling_N, 3), device=device)`` per ``max_batch`` chunk, in the same order), but
  * the grid, the thresholded subset and all jittered neighbourhoods are evaluated in a few launches of up to 2^20 points
    instead of the reference's N^3/4096 + 51 x n/4096 calls of 4096 points - for ANY ``func`` / ``func_grad``, in particular the
    closure ``Runner_UDF.extract_edge`` passes (runner_udf.py:520-527: ``udf_network.gradient`` followed by a normalisation).
    Both callables act point by point, so the chunk size cannot change a result; it only decides whether the field kernels
    see 4096 points (a latency-bound launch) or a million (large gradient launches run the reverse-sweep kernel).  When the
    callables are this package's bound ``UDFNetwork.udf`` / ``.gradient`` the wrappers are skipped as well,
  * the line direction ``F.normalize(torch.linalg.svd(grad_ld)[2][:, -1, :])`` (:86-88) is one HIP kernel over the
    3x3 matrices G^T G (``emap_null_direction``): no 50x3 SVD batch.
There is no CPU fallback: tensors must live on the GPU and libemap_hip.so must be loadable.
"""
import torch

from . import _lib

_BIG = 1 << 20          # points per launch of the fast path (bounds the temporaries: 12 MB in, 16 MB out)


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


def _fast_net(func, func_grad):
    from .udf_model import UDFNetwork
    net = getattr(func, "__self__", None)
    if isinstance(net, UDFNetwork) and getattr(func_grad, "__self__", None) is net \
            and func.__name__ == "udf" and func_grad.__name__ == "gradient":
        return net
    return None


def _uses_package_net(f) -> bool:
    """True for a callable that evaluates this package's UDFNetwork point by point: the network's own bound methods, or a closure
    over the network / over an object that owns one (the runner's normalising closure, runner_udf.py:520-527).  Such callables are
    driven with 2^20-point launches; any OTHER callable keeps the caller's ``max_batch`` chunks (it may not act point by point, and
    ``max_batch`` may be its memory bound)."""
    from .udf_model import UDFNetwork
    owns = lambda o: isinstance(o, UDFNetwork) or isinstance(getattr(o, "udf_network", None), UDFNetwork)
    if owns(getattr(f, "__self__", None)):
        return True
    cells = [c.cell_contents for c in (getattr(f, "__closure__", None) or []) if c is not None]
    return any(owns(o) for o in cells) or any(owns(o) for o in (getattr(f, "__defaults__", None) or ()))


def _chunk(func, func_grad, max_batch, mult=1):
    return _BIG if (_uses_package_net(func) and _uses_package_net(func_grad)) else max(int(max_batch) * mult, 1)


def _eval(fn, pts, chunk):
    return torch.cat([fn(pts[h:h + chunk]) for h in range(0, pts.shape[0], chunk)]) if pts.shape[0] else fn(pts)


def get_udf_normals_grid(func, func_grad, N, udf_threshold, is_linedirection=False, sampling_N=50, sampling_delta=0.005,
                         max_batch=int(2 ** 12), device="cuda", noise=None):
    """See the module docstring.  ``noise`` (n_below_threshold, sampling_N, 3) replaces the jitter draws (parity tests)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("emap_amd.extraction runs on the GPU only (no CPU fallback)")
    net = _fast_net(func, func_grad)
    # the N^3 lattice on [-1, 1]^3, first coordinate slowest (the reference's point order and fp32 arithmetic, :36-54: index * 2/(N-1) - 1)
    voxel_size = 2.0 / (N - 1)
    axis = torch.arange(N, device=device, dtype=torch.float32) * voxel_size + (-1)
    samples = torch.zeros(N ** 3, 12, device=device)
    samples[:, :3] = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(-1, 3)

    with torch.no_grad():
        pts = samples[:, :3].contiguous()
        if net is not None:
            df = _eval(lambda p: net.hip_udf(p, with_grad=False)[0], pts, _BIG)
        else:
            df = _eval(lambda p: func(p)[0].detach(), pts, _chunk(func, func_grad, max_batch))
        samples[:, 3:4] = df

        norm_idx = torch.where(samples[:, 3] < udf_threshold)[0]            # :64-65
        sub = samples[norm_idx, :3].contiguous()
        if net is not None:
            grad = _eval(lambda p: net.hip_udf(p, with_grad=True)[1], sub, _BIG).reshape(-1, 1, 3) if len(norm_idx) else sub.reshape(-1, 1, 3)
        else:
            grad = _eval(lambda p: func_grad(p).detach(), sub, _chunk(func, func_grad, max_batch)) if len(norm_idx) else sub.reshape(-1, 1, 3)
        # the reference normalises the (P,1,3) gradient along dim=1 - the singleton - i.e. per component (:71)
        samples[norm_idx, 4:7] = -torch.nn.functional.normalize(grad, dim=1)[:, 0]

        if is_linedirection and len(norm_idx):
            if noise is None:
                # same draw sequence as the reference: one randn per max_batch chunk of the thresholded points (:75-79)
                noise = torch.cat([torch.randn((min(max_batch, len(norm_idx) - h), sampling_N, 3), device=device)
                                   for h in range(0, len(norm_idx), max_batch)])
            ld_pts = (sub.unsqueeze(1) + sampling_delta * noise.to(device)).reshape(-1, 3)
            if net is not None:
                grad_ld = _eval(lambda p: net.hip_udf(p, with_grad=True)[1], ld_pts, _BIG)
            else:
                grad_ld = _eval(lambda p: func_grad(p).detach().reshape(-1, 3), ld_pts, _chunk(func, func_grad, max_batch, sampling_N))
            samples[norm_idx, 8:11] = null_direction(grad_ld.reshape(len(norm_idx), sampling_N, 3))

    df_values = samples[:, 3].reshape(N, N, N)
    vecs = samples[:, 4:7].reshape(N, N, N, 3)
    ld = samples[:, 8:11].reshape(N, N, N, 3)
    return df_values, ld, vecs, samples, torch.tensor(voxel_size)


def get_udf_normals_slow(func, func_grad, voxel_size, xyz, is_linedirection, sampling_N=50, sampling_delta=0.005,
                         max_batch=int(2 ** 12), device="cuda", noise=None):
    """Mirror of ``get_udf_normals_slow`` (extract_pointcloud.py:98-193): values, normals (-grad/|grad|) and optional line
    directions at arbitrary points ``xyz`` (n,3).  Same return tuple ``(df_values, normals, ld, samples)`` with the
    reference's 13-column ``samples``; ``voxel_size`` is unused there as well."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("emap_amd.extraction runs on the GPU only (no CPU fallback)")
    net = _fast_net(func, func_grad)
    xyz = xyz.to(device).float()
    n = xyz.shape[0]
    samples = torch.cat([xyz, torch.zeros(n, 10, device=device)], dim=-1)
    with torch.no_grad():
        pts = samples[:, 0:3].contiguous()
        if net is not None:
            res = [net.hip_udf(pts[h:h + _BIG], with_grad=True) for h in range(0, n, _BIG)] if n else []
            df = torch.cat([r[0] for r in res]) if n else pts[:, :1]
            grad = torch.cat([r[1] for r in res]) if n else pts
        else:
            df = _eval(lambda p: func(p)[0].detach(), pts, _chunk(func, func_grad, max_batch))
            grad = _eval(lambda p: func_grad(p).detach()[:, 0], pts, _chunk(func, func_grad, max_batch))
        samples[:, 3] = df.squeeze(-1)
        samples[:, 4:7] = -torch.nn.functional.normalize(grad, dim=1)                     # :158-160
        if is_linedirection and n:
            if noise is None:
                noise = torch.cat([torch.randn((min(max_batch, n - h), sampling_N, 3), device=device)
                                   for h in range(0, n, max_batch)])                           # :163-167, per chunk
            ld_pts = (pts.unsqueeze(1) + sampling_delta * noise.to(device)).reshape(-1, 3)
            if net is not None:
                grad_ld = _eval(lambda p: net.hip_udf(p, with_grad=True)[1], ld_pts, _BIG)
            else:
                grad_ld = _eval(lambda p: func_grad(p.float()).detach()[:, 0], ld_pts, _chunk(func, func_grad, max_batch, sampling_N))
            samples[:, 7:10] = null_direction(grad_ld.reshape(n, sampling_N, 3))
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
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("emap_amd.extraction runs on the GPU only (no CPU fallback)")
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


def compact(df, xyz, threshold, inclusive, capacity=_SURVIVORS0, chunk=_BIG):
    """Order-preserving ``(xyz[mask], df[mask], torch.where(mask)[0])`` with ``mask = df <= threshold`` (inclusive) or
    ``df < threshold``: the input goes through the compaction kernel in chunks, the survivor buffers grow when a chunk reports
    that it does not fit, and that chunk is repeated."""
    _lib.require_cuda(df, "df")
    df = _lib.f32c(df).reshape(-1)
    xyz = _lib.f32c(xyz)
    c = Compactor(df.device, capacity)
    heads = list(range(0, int(df.shape[0]), chunk))
    done = 0
    while True:
        for h in heads[done:]:
            c.append(df[h:h + chunk], xyz[h:h + chunk], threshold, inclusive, first_index=h)
        _, done, overflowed = c.finish()
        if not overflowed:
            return c.result()


def _closes_over(f, net) -> bool:
    """True if the closure ``f`` holds ``net`` itself or an object one of whose attributes IS ``net`` - whatever the attribute is
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
    cells = []
    for c in (getattr(f, "__closure__", None) or ()):
        try:
            cells.append(c.cell_contents)
        except ValueError:                                   # an empty cell
            pass
    return any(holds(o) for o in [getattr(f, "__self__", None), *cells, *(getattr(f, "__defaults__", None) or ())] if o is not None)


def _stream_fns(func, func_grad):
    """(net, grad) for the streamed path, or None: ``func`` is this package's bound ``UDFNetwork.udf`` and ``func_grad`` its bound
    ``.gradient`` (grad = None: the fused value + gradient kernel) or a closure over THAT network or over an object that owns it -
    the runner's normalising closure over ``self`` (runner_udf.py:520-527) - which is then called on up to 2^20 points at a time.
    A closure over any other network, or over nothing recognisable, takes the composed path."""
    from .udf_model import UDFNetwork
    net = _fast_net(func, func_grad)
    if net is not None:
        return net, None
    net = getattr(func, "__self__", None)
    if isinstance(net, UDFNetwork) and getattr(func, "__name__", "") == "udf" and callable(func_grad) and _closes_over(func_grad, net):
        return net, func_grad
    return None


def _gradients(net, grad_fn, pts):
    """(P, 3) gradients at pts (P <= 2^20 per launch)."""
    if grad_fn is None:
        return _eval(lambda p: net.hip_udf(p, with_grad=True)[1], pts, _BIG)
    return _eval(lambda p: grad_fn(p).detach().reshape(-1, 3), pts, _BIG)


def _line_directions(net, grad_fn, pts, sampling_N, sampling_delta, noise, device):
    """Null direction of the gradients in a jittered neighbourhood of every point, in groups of whole ``max_batch`` draws so that
    no neighbourhood tensor exceeds 2^20 points.  The draws are the reference's: one randn per 4096 points, in order."""
    n = int(pts.shape[0])
    out = torch.empty(n, 3, device=device)
    if noise is not None and tuple(noise.shape) != (n, sampling_N, 3):
        raise ValueError(f"noise {tuple(noise.shape)} given for a stage of {n} points x {sampling_N} samples")
    group = max(_BIG // (sampling_N * _MAX_BATCH), 1) * _MAX_BATCH
    for h in range(0, n, group):
        t = min(h + group, n)
        if noise is None:
            z = torch.cat([torch.randn((min(_MAX_BATCH, t - b), sampling_N, 3), device=device) for b in range(h, t, _MAX_BATCH)])
        else:
            z = noise[h:t].to(device)
        g = _gradients(net, grad_fn, jitter_points(pts[h:t], z, sampling_delta))
        out[h:t] = null_direction(g.reshape(t - h, sampling_N, 3))
    return out


def _pointcloud_stream(net, grad_fn, N, thr, sampling_N, sampling_delta, is_pointshift, iters, is_linedirection, device, noise, trace=None):
    """The streamed routine; returns device tensors (points, line directions).  Host reads per stage: the compaction state, once
    (again after a grown buffer), plus at the grid stage the index build of the df < thr subset.
    ``trace`` is TEST-ONLY scaffolding and not reachable through the public function: a dict that receives references (no copies)
    to each stage's lattice indices, which the parity test needs to align the reference's recorded jitter rows with this run's
    point sets.  Production callers leave it None."""
    F = torch.nn.functional
    noise = iter(noise) if noise is not None else None
    take = (lambda: next(noise, None)) if noise is not None else (lambda: None)
    total = N ** 3
    with torch.no_grad():
        # grid stage: value pass + compaction of clamp(df, 0) <= thr.  For thr >= 0 that set is df <= thr, which also holds every
        # point of the normals' set df < thr; for thr < 0 it is empty while df < thr may not be - then the raw set is kept.
        c = Compactor(device)
        buf = torch.empty(min(_BIG, total), 3, device=device)
        heads, done = list(range(0, total, _BIG)), 0
        while True:
            for h in heads[done:]:
                xyz = lattice_points(N, h, min(_BIG, total - h), device, out=buf)
                c.append(net.hip_udf(xyz, with_grad=False)[0], xyz, thr, thr >= 0, first_index=h)
            _, done, overflowed = c.finish()
            if not overflowed:
                break
        del buf
        xyz, df, idx = c.result()
        below = torch.where(df < thr)[0]                                    # :65 - normals and directions live here (the stage's one index build)
        sub = xyz[below]
        n = int(xyz.shape[0])
        normals, lds = torch.zeros(n, 3, device=device), torch.zeros(n, 3, device=device)
        grad = _gradients(net, grad_fn, sub).reshape(-1, 1, 3)
        normals[below] = -F.normalize(grad, dim=1)[:, 0]                    # per component: the reference's dim=1 on (P, 1, 3), :72
        if is_linedirection:
            lds[below] = _line_directions(net, grad_fn, sub, sampling_N, sampling_delta, take(), device)
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
                last = it == iters - 1
                n = int(shifted.shape[0])
                if grad_fn is None:
                    res = [net.hip_udf(shifted[h:h + _BIG], with_grad=True) for h in range(0, n, _BIG)]
                    sdf = torch.cat([r[0] for r in res]).reshape(-1) if n else shifted[:, 0]
                    grad = torch.cat([r[1] for r in res]) if n else shifted
                else:
                    sdf = _eval(lambda p: net.hip_udf(p, with_grad=False)[0], shifted, _BIG).reshape(-1) if n else shifted[:, 0]
                    grad = _gradients(net, grad_fn, shifted) if n else shifted
                snormals = -F.normalize(grad, dim=1)                        # :160-161
                slds = torch.zeros(n, 3, device=device)
                if last:                                                    # the reference's own sampling_N / delta here, not the caller's
                    slds = _line_directions(net, grad_fn, shifted, _SLOW_SAMPLING_N, _SLOW_SAMPLING_DELTA, take(), device)
                sxyz, sdf_kept, src = compact(sdf, shifted, thr, True, capacity=n)      # :282
                if trace is not None:
                    trace[f"shift{it}"] = dict(idx=idx, df=sdf, xyz=shifted, kept=src)
                xyz, df, idx, normals, lds = sxyz, sdf_kept, idx[src], snormals[src], slds[src]
        if trace is not None:
            trace["final_idx"] = idx
    return xyz, lds


def _pointcloud_composed(func, func_grad, N_MC, udf_threshold, sampling_N, sampling_delta, is_pointshift, iters, is_linedirection,
                         device, noise):
    """Any other callable: the reference's own composition of the two query routines (extract_pointcloud.py:240-293)."""
    noise = iter(noise) if noise is not None else None
    take = (lambda: next(noise, None)) if noise is not None else (lambda: None)
    df, lds, normals, samples, voxel_size = get_udf_normals_grid(
        func, func_grad, N_MC, udf_threshold, is_linedirection, sampling_N, sampling_delta, device=device,
        noise=take() if is_linedirection else None)
    df, lds, normals, xyz = df.reshape(-1), lds.reshape(-1, 3), normals.reshape(-1, 3), samples.reshape(-1, 12)[:, 0:3]
    df = df.clamp(min=0)
    keep = df <= udf_threshold
    xyz, lds, normals, df = xyz[keep], lds[keep], normals[keep], df[keep]
    if is_pointshift and iters > 0:
        for it in range(iters):
            last = it == iters - 1
            shifted = xyz + df.unsqueeze(-1) * normals
            sdf, snormals, lds, _ = get_udf_normals_slow(func, func_grad, voxel_size, shifted, last, device=device,
                                                         noise=take() if last else None)
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
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("emap_amd.extraction runs on the GPU only (no CPU fallback)")
    N_MC, thr = int(N_MC), float(udf_threshold)
    fns = _stream_fns(func, func_grad)
    if fns is not None:
        xyz, lds = _pointcloud_stream(fns[0], fns[1], N_MC, thr, int(sampling_N), float(sampling_delta), is_pointshift, int(iters),
                                      is_linedirection, device, noise)
    else:
        xyz, lds = _pointcloud_composed(func, func_grad, N_MC, thr, sampling_N, sampling_delta, is_pointshift, int(iters),
                                        is_linedirection, device, noise)
    return xyz.cpu().numpy(), lds.cpu().numpy()
