"""The call schedule of the three extraction routines: which of ``net.hip_udf``, ``func`` and ``func_grad`` is called on how many points,
in which order, for every kind of callable.

The gradient kernel is chosen by launch size, so the partition of a point set into calls is part of the result.  The rules
(DESIGN 3.6), with B = extraction._BIG and M = extraction._MAX_BATCH, both shrunk here so that small shapes cross every boundary:
  get_udf_normals_grid   values over the lattice, then gradients of the df < thr subset, per B (the network's own methods, or callables
                         that evaluate the package's network point by point) or per max_batch (anything else); the flattened
                         n x sampling_N neighbourhood per B, or per max_batch x sampling_N
  get_udf_normals_slow   the network's own methods: ONE hip_udf(with_grad=True) per B gives value and gradient; otherwise func, then
                         func_grad, per chunk; the neighbourhood as above
  get_pointcloud_from_udf, streamed (func is the network's udf, func_grad its gradient or a closure that holds the network)
                         lattice per B through hip_udf(with_grad=False); subset gradients per B; neighbourhoods in groups of
                         max(B // (sampling_N x M), 1) x M points, one call per group; each shift: the fused kernel per B, or
                         hip_udf(with_grad=False) per B then the closure per B; the last shift's neighbourhoods with 50 samples
  get_pointcloud_from_udf, any other callable: the grid routine, then the slow routine per shift, at their default max_batch of 4096.
A bound method cannot be wrapped without turning it into another kind of callable, so the recorders are an instance attribute
``net.hip_udf`` and closures that keep their kind; ``net.udf`` and ``net.gradient`` show up as the hip_udf call they make."""
import functools
import types

import numpy as np
import pytest
import torch

from emap_amd import extraction
from gpu_helpers import mk, DEV
from test_gpu_extraction_digests import callables

pytestmark = pytest.mark.gpu

B, M = 4096, 64
N = 24                         # 13 824 lattice points: three chunks of B and a ragged fourth
QUANTILE = 0.40                # more than B survivors: two chunks per shift stage, and a ragged last neighbourhood group
HIP_VALUE, HIP_GRAD, FUNC, FUNC_GRAD = ("hip_udf", False), ("hip_udf", True), ("func", None), ("func_grad", None)
# per kind: what one value / one gradient evaluation of a chunk records, whether the point cloud streams, whether chunks are B or max_batch
KINDS = {
    "bound": dict(value=[HIP_VALUE], grad=[HIP_GRAD], streams=True, big=True),
    "runner_fine": dict(value=[HIP_VALUE], grad=[FUNC_GRAD, HIP_GRAD], streams=True, big=False),     # the owner rules disagree on this one
    "owner": dict(value=[HIP_VALUE], grad=[FUNC_GRAD, HIP_GRAD], streams=True, big=True),
    "lambdas": dict(value=[FUNC, HIP_VALUE], grad=[FUNC_GRAD, HIP_GRAD], streams=False, big=True),
    "analytic": dict(value=[FUNC], grad=[FUNC_GRAD], streams=False, big=False),
}


@functools.lru_cache(maxsize=None)
def _net():
    return mk("d4w128L10", "f16x3")[0]


def recorded(kind, net, rec):
    """(func, func_grad) of the kind, recording ("func" | "func_grad", points, None) where the kind leaves room for a recorder."""
    def note(which, fn):
        def wrapped(p):
            rec.append((which, int(p.shape[0]), None))
            return fn(p)
        return wrapped

    if kind == "bound":
        return net.udf, net.gradient
    if kind == "runner_fine":
        owner = types.SimpleNamespace(udf_network_fine=net)

        def func_grad(p):                                     # a closure over the owner, as Runner_UDF.extract_edge's
            rec.append(("func_grad", int(p.shape[0]), None))
            g = owner.udf_network_fine.gradient(p)
            return g / (torch.linalg.norm(g, ord=2, dim=-1, keepdim=True) + 1e-5)
        return net.udf, func_grad
    if kind == "owner":
        owner = types.SimpleNamespace(udf_network=net)

        def func_grad(p):
            rec.append(("func_grad", int(p.shape[0]), None))
            return owner.udf_network.gradient(p)
        return net.udf, func_grad
    if kind == "lambdas":
        def func(p):
            rec.append(("func", int(p.shape[0]), None))
            return net.udf(p)

        def func_grad(p):
            rec.append(("func_grad", int(p.shape[0]), None))
            return net.gradient(p)
        return func, func_grad
    f, g = callables("analytic")
    return note("func", f), note("func_grad", g)


@pytest.fixture
def setup(monkeypatch):
    monkeypatch.setattr(extraction, "_BIG", B)
    monkeypatch.setattr(extraction, "_MAX_BATCH", M)
    net, rec = _net(), []
    real = net.hip_udf

    def hip_udf(x, with_grad=False, precision=None):
        rec.append(("hip_udf", int(x.reshape(-1, 3).shape[0]), bool(with_grad)))
        return real(x, with_grad, precision)
    net.hip_udf = hip_udf
    yield net, rec
    del net.hip_udf


def chunks(n, c):
    return [min(c, n - h) for h in range(0, n, c)]


def calls(parts, sizes):
    return [(which, n, with_grad) for n in sizes for which, with_grad in parts]


def neighbourhood(k, n, sampling_N, max_batch):
    return calls(k["grad"], chunks(n * sampling_N, B if k["big"] else max_batch * sampling_N))


def expected_grid(k, n_below, sampling_N, max_batch, directions=True):
    c = B if k["big"] else max_batch
    e = calls(k["value"], chunks(N ** 3, c)) + calls(k["grad"], chunks(n_below, c))
    return e + (neighbourhood(k, n_below, sampling_N, max_batch) if directions else [])


def expected_slow(k, n, sampling_N, max_batch, directions=True):
    c = B if k["big"] else max_batch
    e = calls([HIP_GRAD], chunks(n, B)) if k["value"] == [HIP_VALUE] and k["grad"] == [HIP_GRAD] else \
        calls(k["value"], chunks(n, c)) + calls(k["grad"], chunks(n, c))
    return e + (neighbourhood(k, n, sampling_N, max_batch) if directions else [])


def expected_stream(k, n_below, n_in, sampling_N):
    def groups(n, s):
        return [x for g in chunks(n, max(B // (s * M), 1) * M) for x in chunks(g * s, B)]
    e = calls([HIP_VALUE], chunks(N ** 3, B)) + calls(k["grad"], chunks(n_below, B)) + calls(k["grad"], groups(n_below, sampling_N))
    for it, n in enumerate(n_in):
        e += calls([HIP_GRAD], chunks(n, B)) if k["grad"] == [HIP_GRAD] else calls([HIP_VALUE], chunks(n, B)) + calls(k["grad"], chunks(n, B))
        if it == len(n_in) - 1:
            e += calls(k["grad"], groups(n, 50))
    return e


def expected_composed(k, n_below, n_in, sampling_N):
    e = expected_grid(k, n_below, sampling_N, 4096)
    for it, n in enumerate(n_in):
        last = it == len(n_in) - 1
        e += expected_slow(k, n, 50, 4096, directions=last)
    return e


def _threshold(func, func_grad, rec):
    df = extraction.get_udf_normals_grid(func, func_grad, N, -1.0, False, device=DEV)[0].reshape(-1).cpu().numpy()
    thr = float(np.float32(np.quantile(df.astype(np.float64), QUANTILE)))
    rec.clear()
    return thr, int((df < np.float32(thr)).sum()), int((np.maximum(df, 0) <= np.float32(thr)).sum())


CASES = [(kind, 4096) for kind in KINDS] + [("analytic", 256), ("runner_fine", 256)]


@pytest.mark.parametrize("kind,max_batch", CASES)
def test_grid_schedule(setup, kind, max_batch):
    net, rec = setup
    func, func_grad = recorded(kind, net, rec)
    thr, n_below, _ = _threshold(func, func_grad, rec)
    assert N ** 3 % B and n_below > B
    extraction.get_udf_normals_grid(func, func_grad, N, thr, True, sampling_N=24, max_batch=max_batch, device=DEV)
    assert rec == expected_grid(KINDS[kind], n_below, 24, max_batch)


@pytest.mark.parametrize("kind,max_batch", CASES)
def test_slow_schedule(setup, kind, max_batch):
    net, rec = setup
    func, func_grad = recorded(kind, net, rec)
    n = 5000                                                  # two chunks of B, the second ragged
    xyz = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).random((n, 3), dtype=np.float32) * 2 - 1)
    for directions in (True, False):
        rec.clear()
        extraction.get_udf_normals_slow(func, func_grad, None, xyz, directions, sampling_N=24, max_batch=max_batch, device=DEV)
        assert rec == expected_slow(KINDS[kind], n, 24, max_batch, directions)


@pytest.mark.parametrize("kind", list(KINDS))
def test_point_cloud_schedule(setup, kind):
    net, rec = setup
    func, func_grad = recorded(kind, net, rec)
    thr, n_below, n_grid = _threshold(func, func_grad, rec)
    args = dict(N_MC=N, udf_threshold=thr, sampling_N=24, is_pointshift=True, device=DEV)
    n_shifted = len(extraction.get_pointcloud_from_udf(func, func_grad, iters=1, is_linedirection=False, **args)[0])
    assert n_grid > B and n_shifted % M and n_below % (2 * M)      # two chunks in the first shift, ragged last groups
    rec.clear()
    extraction.get_pointcloud_from_udf(func, func_grad, iters=2, is_linedirection=True, **args)
    k = KINDS[kind]
    want = (expected_stream if k["streams"] else expected_composed)(k, n_below, [n_grid, n_shifted], 24)
    assert rec == want
