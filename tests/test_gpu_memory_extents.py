"""GPU tests (-m gpu) of WHERE the C ABI writes and what it reads before writing ("Memory extents and workspace independence").

Every case builds its arguments in a guard_bands.Arena - inputs frozen, outputs and workspaces of exactly the documented / queried size,
each between two guard bands - calls the entry point through _lib.api() (a non-zero rc raises), synchronises, and asserts
  (a) rc = 0 and a zero error word where the call has one,
  (b) Arena.check(): no guard byte touched, no input changed,
  (c) no prefill sentinel left in any output the header says the call writes,
  (d) two runs with zero-filled outputs and workspaces are bit-identical,
  (e) a run with every output and workspace byte prefilled 0xA5 is bit-identical to them.
In-out and accumulated buffers (accumulate = 1, Adam's state, the monitor's record) get the same finite prefill in every run, so they take
part in (d) and (e) as well; what a caller must initialise by the header (the monitor's workspace, compaction's state) is initialised so.
COVERED / EXCLUDED are read by tests/test_memory_extents_cpu.py: every symbol of _lib.SYMBOLS is in exactly one of them.  Nothing here
touches the device at import."""
import ctypes as C
import hashlib

import pytest
import torch

from emap_amd import _lib, synthetic
from guard_bands import Arena
from gpu_helpers import mk, rel, DEV

pytestmark = pytest.mark.gpu

HOST_ONLY = "host-only"
MULTI_PROCESS = "multi-process with its own region contract: tests/test_gpu_multi.py"
EXCLUDED = {k: HOST_ONLY for k in (
    "emap_abi_version", "emap_last_error", "emap_set_grad_mode", "emap_set_fused_sampling", "emap_set_fused_composite", "emap_packed_bytes",
    "emap_udf_scratch_bytes", "emap_compact_workspace_bytes", "emap_nn_workspace_bytes", "emap_render_workspace_bytes",
    "emap_udf_vjp_workspace_bytes", "emap_render_bwd_workspace_bytes", "emap_render_bwd_absmax_offset", "emap_check_train_images",
    "emap_gen_rays_count", "emap_train_monitor_workspace_bytes", "emap_profile_enable", "emap_profile_read", "emap_profile_read_kernel",
    "emap_profile_read_clock", "emap_linspace_host")}
EXCLUDED.update({k: MULTI_PROCESS for k in (
    "emap_ar_local_bytes", "emap_ar_alloc", "emap_ar_open", "emap_ar_close", "emap_ar_free", "emap_ar_allreduce_sum", "emap_ar_error",
    "emap_ar_set_timeout_ms")})
COVERED = {}


def covers(*entries):
    """registers the test function under each entry point it calls in an arena"""
    def deco(f):
        for e in entries:
            COVERED.setdefault(e, []).append(f.__name__)
        return f
    return deco


NETS = ("d8w256L10", "d4w128L10")
PRECS = ("bf16", "bf16x3", "f16", "f16x3", "f16x3m", "f16x3e")
SPLIT = ("bf16x3", "f16x3", "f16x3m", "f16x3e")
NET_PRECS = [(n, p) for n in NETS for p in PRECS if p != "f16x3m" or n == "d8w256L10"]      # f16x3m needs d_hidden = 256


# ------------------------------------------------------------------------------------------------ the harness
class Fill:
    """how one run prefills: `out` the outputs, `ws` the workspaces"""
    def __init__(self, out, ws):
        self.out, self.ws = out, ws


RUNS = (Fill("nan", "pattern"), Fill("zero", "zero"), Fill("zero", "zero"), Fill("pattern", "pattern"))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def stream():
    return _lib.stream_ptr(DEV)


def extents(case, capacity=32 << 20, what=""):
    """Run `case(arena, fill) -> {name: output view}` under the four prefills and assert (a) - (e).  The case makes the call itself; the
    key "err_flags", if present, is the call's device error word.  Returns the outputs of the first zero-filled run (clones)."""
    results = []
    for i, f in enumerate(RUNS):
        a = Arena(DEV, capacity)
        with torch.cuda.device(DEV):
            out = case(a, f)
        torch.cuda.synchronize()
        a.check()                                                                           # (b)
        if "err_flags" in out:
            assert int(out["err_flags"].item()) == 0, (what, int(out["err_flags"].item()))  # (a)
        for k, v in out.items():
            if i == 0:
                Arena.check_written(v, f"{what} {k}")                                      # (c)
        results.append({k: v.clone() for k, v in out.items()})
    for k in results[1]:
        assert same_bits(results[1][k], results[2][k]), f"{what} {k}: two zero-filled runs differ (d)"
        assert same_bits(results[1][k], results[3][k]), f"{what} {k}: the 0xA5-filled run differs from the zero-filled one (e)"
        assert same_bits(results[1][k], results[0][k]), f"{what} {k}: the sentinel-filled run differs from the zero-filled one (e)"
    return results[1]


def table(ptrs):
    ptrs = [int(p) for p in ptrs]
    return (C.c_void_p * len(ptrs))(*ptrs)


@pytest.fixture(scope="module")
def nets():
    """(network name, precision) -> (cfg struct, precision code, packed buffer, state dict, oracle config, module): packed once per module"""
    cache = {}

    def get(name, prec):
        if (name, prec) not in cache:
            net, state, ocfg = mk(name, prec)
            cache[name, prec] = (net.net_config(), _lib.PRECISIONS[prec], net.packed(prec), state, ocfg, net)
        return cache[name, prec]
    return get


def gvb(state, n_lin):
    key = "lin{}.parametrizations.weight.original{}"
    return ([state[key.format(l, 0)] for l in range(n_lin)], [state[key.format(l, 1)] for l in range(n_lin)],
            [state[f"lin{l}.bias"] for l in range(n_lin)])


# ------------------------------------------------------------------------------------------------ weights
@covers("emap_pack_weights")
@pytest.mark.parametrize("name,prec", NET_PRECS)
def test_pack_weights(nets, name, prec):
    cfg, pc, packed_ref, state, _, _ = nets(name, prec)
    nbytes = _lib.size_of("packed_bytes", cfg, pc)
    assert nbytes == packed_ref.numel()
    res = {}
    for fill in ("pattern", "zero"):
        a = Arena(DEV, 64 << 20)
        g, v, b = [[a.frozen(t, f"{n}{l}") for l, t in enumerate(ts)] for n, ts in zip("gvb", gvb(state, cfg.n_lin))]
        buf = a.bytes(nbytes, fill, "packed")
        _lib.api().pack_weights(cfg, table(t.data_ptr() for t in g), table(t.data_ptr() for t in v), table(t.data_ptr() for t in b), buf, pc,
                                stream())
        torch.cuda.synchronize()
        a.check()
        res[fill] = buf.clone()
    # Which bytes the packer writes, and to what, is pinned by tests/test_gpu_packing.py: the sha256 of the whole buffer after a 0xA5 prefill,
    # alignment padding included.  The 0xA5 run here must be that buffer byte for byte - here packed into exactly emap_packed_bytes between
    # guards, from frozen g / v / b.  What this test adds beside the guards: the zero-prefilled run differs from the pinned one only where
    # the pinned one still holds its prefill (the bytes "left alone") and holds its own prefill, 0, there.  The mask of those bytes is taken
    # from the pinned result, not from the layout: a byte the packer should write but never did is the digest's to find, not this test's.
    from test_gpu_packing import DIGESTS
    assert hashlib.sha256(res["pattern"].cpu().numpy().tobytes()).hexdigest() == DIGESTS[(name, prec)]
    alone = res["pattern"] == 0xA5
    assert torch.equal(res["pattern"][~alone], res["zero"][~alone])
    differs = res["pattern"] != res["zero"]
    assert bool((res["zero"][differs] == 0).all()) and bool(alone[differs].all())
    assert torch.equal(res["zero"], packed_ref)                # what the package packed into its own zeroed buffer


# ------------------------------------------------------------------------------------------------ fields
P_SPLIT = (1, 15, 17, 31, 33, 63, 65, 257, 8191, 8193)
P_SINGLE = P_SPLIT + (16383, 16385)
P_REV = (1, 31, 33, 65, 8193)
# one point more than the 512 persistent workgroups of the reverse sweep take in one round (64 points each): every workgroup's slab of the
# scratch is in use, the last one's included - a scratch query that reports too little is seen only here (f16x3m keeps the PE block's lo parts
# in the last 8 KiB of each slab, f16x3e its third sigma' plane)
P_ALL_WORKGROUPS = 512 * 64 + 1
# the reverse sweep against the oracle: test_gpu_parity.py, test_reverse_mode_ragged_sizes_vs_oracle (f16x3, f16) and the reverse-mode
# launches of the test above it (bf16x3, bf16); f16x3m / f16x3e are f16x3's gate (include/emap_hip.h)
REV_TOL = {"f16x3": (1e-4, 1e-4), "f16x3m": (1e-4, 1e-4), "f16x3e": (1e-4, 1e-4), "bf16x3": (1e-4, 1e-4), "f16": (3e-3, 1e-2), "bf16": (2e-2, 8e-2)}


def _points(P):
    return torch.rand(P, 3, generator=torch.Generator().manual_seed(P)) * 2 - 1


def _field_case(cfg, pc, packed, x, with_grad):
    P = x.shape[0]
    nb = _lib.size_of("udf_scratch_bytes", cfg, pc, P) if with_grad else 0

    def case(a, f):
        xs = a.frozen(x, "x")
        udf = a.buf((P,), torch.float32, f.out, "udf")
        if not with_grad:
            _lib.api().udf_fwd(cfg, packed, pc, xs, P, udf, stream())
            return {"udf": udf}
        grad = a.buf((P, 3), torch.float32, f.out, "grad3")
        scr = a.bytes(nb, f.ws, "scratch") if nb else None
        _lib.api().udf_fwd_grad(cfg, packed, pc, xs, P, udf, grad, scr, nb, stream())
        return {"udf": udf, "grad3": grad}
    return case, nb


@covers("emap_udf_fwd", "emap_udf_fwd_grad")
@pytest.mark.parametrize("name,prec", NET_PRECS)
def test_fields(nets, name, prec):
    cfg, pc, packed, _, _, _ = nets(name, prec)
    L = _lib.lib()
    has_rev = cfg.skip_l < cfg.n_lin - 1
    rev_min = 8193 if prec in SPLIT else 16384
    prev = L.emap_set_grad_mode(-1)
    try:
        for P in (P_SPLIT if prec in SPLIT else P_SINGLE) + ((P_ALL_WORKGROUPS,) if has_rev and prec in ("f16x3", "f16x3m", "f16x3e") else ()):
            x = _points(P)
            extents(_field_case(cfg, pc, packed, x, False)[0], what=f"udf_fwd {name} {prec} P={P}")
            fwd = None
            for mode in (-1, 0) + ((1,) if P in P_REV else ()):
                L.emap_set_grad_mode(mode)
                case, nb = _field_case(cfg, pc, packed, x, True)
                uses_rev = has_rev and mode != 0 and (mode == 1 or P >= rev_min)
                assert (nb > 0) == uses_rev, (name, prec, P, mode, nb)
                o = extents(case, capacity=(32 << 20) + nb, what=f"udf_fwd_grad {name} {prec} P={P} grad mode {mode}")
                if mode == 0:
                    fwd = o
                elif mode == 1 and uses_rev:
                    # the forced reverse sweep against forward-mode tangents at the same points, under the tolerance the reverse sweep is
                    # held to against the oracle
                    tu, tg = REV_TOL[prec]
                    assert rel(o["udf"], fwd["udf"]) <= tu and rel(o["grad3"], fwd["grad3"]) <= tg, (
                        name, prec, P, rel(o["udf"], fwd["udf"]), rel(o["grad3"], fwd["grad3"]))
    finally:
        L.emap_set_grad_mode(prev)


@covers("emap_embed")
@pytest.mark.parametrize("multires", [0, 6, 10])
def test_embed(multires):
    from emap_amd.embedder import embed_torch
    for P in (1, 255, 257):
        x = _points(P)

        def case(a, f):
            xs = a.frozen(x, "x")
            pe = a.buf((P, 3 + 6 * multires), torch.float32, f.out, "pe")
            _lib.api().embed(xs, P, multires, pe, stream())
            return {"pe": pe}
        o = extents(case, what=f"embed P={P} multires={multires}")
        assert rel(o["pe"], embed_torch(x.double(), multires)) <= 1e-5


# ------------------------------------------------------------------------------------------------ sampler
SAMPLER_SHAPES = [(2, 1), (64, 16), (65, 16), (129, 70), (257, 64), (513, 511), (1008, 16)]
INDEX_MISMATCH_SHARE, INDEX_MISMATCH_BY = 0.005, 1        # tests/test_gpu_samples_per_ray.py: near-ties of the cdf may go either way


def sampler_inputs(N, n, m, seed=0):
    """rays, a strictly increasing z (N, n) with udf in (1e-3, 0.2) - a well-conditioned reference - new samples z_new (N, m) with their
    udf, pdf weights (N, n - 1) and uniform draws u (N, m).  CPU tensors, seeded."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * m + N + seed)
    ro = torch.randn(N, 3, generator=gen) * 0.3
    rd = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    z = 0.5 + torch.cumsum(torch.rand(N, n, generator=gen) * (4.0 / n) + 1e-3, dim=-1)
    udf = torch.rand(N, n, generator=gen) * 0.199 + 1e-3
    z_new = torch.sort(torch.rand(N, m, generator=gen) * (z[:, -1:] - z[:, :1]) + z[:, :1], dim=-1).values
    udf_new = torch.rand(N, m, generator=gen) * 0.199 + 1e-3
    w = torch.rand(N, n - 1, generator=gen)
    u = torch.rand(N, m, generator=gen)
    return dict(ro=ro, rd=rd, z=z, udf=udf, z_new=z_new, udf_new=udf_new, w=w, u=u, sd=torch.tensor([4.0 / n]))


def index_rule(got, ref, what):
    """the index comparison of tests/test_gpu_samples_per_ray.py: at most 0.5 % of the indices differ, and those by one"""
    bad = got != ref
    assert float(bad.float().mean()) <= INDEX_MISMATCH_SHARE, (what, int(bad.sum()), bad.numel())
    if bad.any():
        assert int((got - ref)[bad].abs().max()) == INDEX_MISMATCH_BY, what


def sampler_references(d, m, inv_s=64.0, beta=128.0, gamma=80.0):
    """the oracle's indices of the three sampling calls on sampler_inputs(): sample_pdf (grid), sample_pdf (draws u), up_sample_unbias"""
    from oracle import emap_oracle as O
    return {"pdf": O.sample_pdf(d["z"], d["w"], m, det=True, return_inds=True)[1],
            "pdf_u": O.sample_pdf(d["z"], d["w"], m, det=False, return_inds=True, u=d["u"])[1],
            "unbias": O.up_sample_unbias(d["ro"], d["rd"], d["z"], d["udf"], float(d["sd"]), m, inv_s, beta, gamma, return_all=True)["inds"]}


@covers("emap_sample_pdf", "emap_sample_pdf_u", "emap_upsample_step", "emap_upsample_step_plain", "emap_merge_sorted")
@pytest.mark.parametrize("n,m", SAMPLER_SHAPES)
@pytest.mark.parametrize("N", [1, 3])
def test_sampler(N, n, m):
    d = sampler_inputs(N, n, m)
    ref = sampler_references(d, m)
    A = _lib.api()
    for optional in (True, False):
        def pdf(a, f, with_u):
            z, w = a.frozen(d["z"], "bins"), a.frozen(d["w"], "weights")
            u = a.frozen(d["u"], "u") if with_u else None
            s = a.buf((N, m), torch.float32, f.out, "samples")
            i = a.buf((N, m), torch.int64, f.out, "inds") if optional else None
            err = a.buf((1,), torch.int32, "zero", "err_flags")
            if with_u:
                A.sample_pdf_u(z, w, u, N, n, m, s, i, err, stream())
            else:
                A.sample_pdf(z, w, N, n, m, s, i, err, stream())
            return {"samples": s, "err_flags": err, **({"inds": i} if optional else {})}

        def step(a, f, plain):
            ro, rd = a.frozen(d["ro"], "rays_o"), a.frozen(d["rd"], "rays_d")
            z, udf, sd = a.frozen(d["z"], "z"), a.frozen(d["udf"], "udf"), a.frozen(d["sd"], "sample_dist")
            zn = a.buf((N, m), torch.float32, f.out, "z_new")
            i = a.buf((N, m), torch.int64, f.out, "inds") if optional else None
            err = a.buf((1,), torch.int32, "zero", "err_flags")
            if plain:      # rays_o / rays_d are accepted and may be NULL: given with the optional pointers, NULL without
                A.upsample_step_plain(ro if optional else None, rd if optional else None, z, udf, N, n, m, sd, 128.0, 80.0, zn, i, err, stream())
            else:
                A.upsample_step(ro, rd, z, udf, N, n, m, sd, 64.0, 128.0, 80.0, zn, i, err, stream())
            return {"z_new": zn, "err_flags": err, **({"inds": i} if optional else {})}

        def merge(a, f):
            z, zn = a.frozen(d["z"], "z"), a.frozen(d["z_new"], "z_new")
            u, un = (a.frozen(d["udf"], "udf"), a.frozen(d["udf_new"], "udf_new")) if optional else (None, None)
            zo = a.buf((N, n + m), torch.float32, f.out, "z_out")
            uo = a.buf((N, n + m), torch.float32, f.out, "udf_out") if optional else None
            perm = a.buf((N, n + m), torch.int64, f.out, "perm") if optional else None
            A.merge_sorted(z, zn, u, un, N, n, m, zo, uo, perm, stream())
            return {"z_out": zo, **({"udf_out": uo, "perm": perm} if optional else {})}

        tag = f"N={N} n={n} m={m} optional={optional}"
        o_pdf = extents(lambda a, f: pdf(a, f, False), what="sample_pdf " + tag)
        o_pdf_u = extents(lambda a, f: pdf(a, f, True), what="sample_pdf_u " + tag)
        o_un = extents(lambda a, f: step(a, f, False), what="upsample_step " + tag)
        o_pl = extents(lambda a, f: step(a, f, True), what="upsample_step_plain " + tag)
        o_m = extents(merge, what="merge_sorted " + tag)
        for o, k in ((o_pdf, "samples"), (o_pdf_u, "samples"), (o_un, "z_new"), (o_pl, "z_new")):
            v = o[k].cpu()
            assert bool(torch.isfinite(v).all()) and bool((v >= d["z"][:, :1] - 1e-5).all()) and bool((v <= d["z"][:, -1:] + 1e-5).all()), (tag, k)
        zs, order = torch.sort(torch.cat([d["z"], d["z_new"]], -1), dim=-1, stable=True)
        assert torch.equal(o_m["z_out"].cpu(), zs), tag
        if optional:
            index_rule(o_pdf["inds"].cpu(), ref["pdf"], "sample_pdf " + tag)
            index_rule(o_pdf_u["inds"].cpu(), ref["pdf_u"], "sample_pdf_u " + tag)
            index_rule(o_un["inds"].cpu(), ref["unbias"], "upsample_step " + tag)
            # emap_upsample_step_plain has no value reference here (oracle.emap_oracle has no plain step): its z_new is held to the range of
            # z above and its inds go through checks (a) - (e) only; its values are tests/test_gpu_samples_per_ray.py's (goldens g18)
            assert torch.equal(o_m["perm"].cpu(), order), tag
            assert torch.equal(o_m["udf_out"].cpu(), torch.gather(torch.cat([d["udf"], d["udf_new"]], -1), 1, order)), tag


# ------------------------------------------------------------------------------------------------ compositing
PER_SAMPLE = ("weights", "alpha", "mid_z", "dists", "inside_sphere", "gradient_mag")
PER_RAY = {"edge": 1, "depth": 1, "weight_sum": 1, "normals": 3}
MODES = {"unbiased": _lib.RENDER_UNBIASED, "normcos": _lib.RENDER_UNBIASED_NORMCOS, "plain": _lib.RENDER_PLAIN}
SCALARS_WRITTEN = 12     # include/emap_hip.h: `scalars` receives [0] .. [11] of its 16 floats


def render_params(a, N, ns, ni, steps, mode, car=1.0, fs=0.9):
    """EmapRenderParams with variance / beta / gamma read from the device (frozen in the arena), as the package passes them"""
    sc = a.frozen(torch.tensor([0.3, 0.5, 0.3]), "variance/beta/gamma")
    p = _lib.RenderParams()
    p.n_rays, p.n_samples, p.n_importance, p.up_sample_steps = N, ns, ni, steps
    p.cos_anneal_ratio, p.has_cos_anneal, p.flip_saturation = car, 1, fs
    p.near_surface, p.sparse_scale, p.background, p.has_background = 0.05, 25000.0, 0.0, 0
    p.variance_dev, p.beta_dev, p.gamma_dev = sc.data_ptr(), sc.data_ptr() + 4, sc.data_ptr() + 8
    p.beta_min, p.render_mode = 5e-5, mode
    return p


def composite_out(a, N, S, fill, reduced=False):
    """(EmapCompositeOut, {name: the view the call writes}): every output, or the reduced set of UDFRendererBlending.render_reduced"""
    co, out = _lib.CompositeOut(), {}
    if not reduced:
        for k in PER_SAMPLE:
            out[k] = a.buf((N, S), torch.float32, fill, k)
        out["gradients_flip"] = a.buf((N, S, 3), torch.float32, fill, "gradients_flip")
    for k, w in PER_RAY.items():
        out[k] = a.buf((N, w), torch.float32, fill, k)
    sc = a.buf((16,), torch.float32, fill, "scalars")
    for k, v in out.items():
        setattr(co, k, v.data_ptr())
    co.scalars = sc.data_ptr()
    out["scalars"] = sc[:SCALARS_WRITTEN]
    return co, out


def composite_inputs(N, S, seed=0):
    gen = torch.Generator().manual_seed(300 + S + 7 * N + seed)
    ro = torch.randn(N, 3, generator=gen) * 0.3
    rd = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    z = 0.5 + torch.cumsum(torch.rand(N, S, generator=gen) * (2.0 / S) + 1e-4, dim=-1)
    udf = torch.rand(N, S, generator=gen) * 0.2 + 1e-3
    grads = torch.nn.functional.normalize(torch.randn(N, S, 3, generator=gen), dim=-1) * (0.8 + 0.4 * torch.rand(N, S, 1, generator=gen))
    ds = torch.rand(N, generator=gen) * 0.5 + 0.5
    return dict(ro=ro, rd=rd, z=z, udf=udf, grads=grads, ds=ds, sd=torch.tensor([0.03]), d_edge=torch.randn(N, generator=gen) / N,
                d_depth=torch.randn(N, generator=gen) * 0.1 / N)


def composite_forward_reference(d, mode, car=1.0, fs=0.9):
    """alpha, weights, edge, depth in float64: the forward recomputation of tests/test_gpu_backward.py
    (test_composite_kernels_at_every_chunking, the default mode) and of tests/test_gpu_samples_per_ray.py
    (test_plain_composite_bwd_vs_float64_autograd, the plain mode)"""
    from oracle import emap_oracle as O
    dt = torch.float64
    N, S = d["z"].shape
    var, bp, gp = torch.tensor([0.3], dtype=dt), torch.tensor([0.5], dtype=dt), torch.tensor([0.3], dtype=dt)
    inv_s, beta, gamma = O.inv_s_from_variance(var), O.beta_from_param(bp), O.gamma_from_param(gp)
    z, u, g, rd = d["z"].to(dt), d["udf"].to(dt), d["grads"].to(dt), d["rd"].to(dt)
    one = torch.ones(N, 1, dtype=dt)
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), float(d["sd"]), dtype=dt)], -1)
    E = torch.exp(-beta * u)
    occ = 1.0 - torch.exp(-torch.relu(beta * E / (1 + E) ** 2) * gamma * dists)
    if mode == "plain":
        alpha = occ
    else:
        tc = (rd[:, None, :] * g).sum(-1)
        vm = torch.cat([(tc[:, 1:] < 0.01).to(dt), one], -1)
        vp = torch.cumprod(torch.cat([one, (1.0 - occ + fs * vm).clip(0, 1) + 1e-7], -1), -1)[:, :-1].clip(0, 1)
        ap = O.sdf2alpha(u.reshape(-1, 1), -tc.abs().reshape(-1, 1), dists.reshape(-1, 1), inv_s, car).reshape(N, S)
        am = O.sdf2alpha(-u.reshape(-1, 1), -tc.abs().reshape(-1, 1), dists.reshape(-1, 1), inv_s, car).reshape(N, S)
        alpha = ap * vp + am * (1 - vp)
    w = alpha * torch.cumprod(torch.cat([one, 1.0 - alpha + 1e-7], -1), -1)[:, :-1]
    return {"alpha": alpha, "weights": w, "edge": w.sum(-1, keepdim=True), "depth": (((z + dists * 0.5) * w).sum(-1) * d["ds"].to(dt)).view(N, 1)}


def composite_backward_reference(d, mode, scalars, car=1.0, fs=0.9):
    """(dL/dudf, dL/dgrad3) in float64 for L = sum(d_edge edge) + sum(d_depth depth) + 0.1 gradient_error + 0.05 gradient_error_near_surface:
    oracle/vjp_mirror.composite_bwd as tests/test_gpu_backward.py calls it (default mode), float64 autograd through the plain tail as
    tests/test_gpu_samples_per_ray.py:test_plain_composite_bwd_vs_float64_autograd writes it (plain mode)"""
    from oracle import emap_oracle as O
    from oracle import vjp_mirror as M
    N, S = d["z"].shape
    dt = torch.float64
    var, bp, gp = torch.tensor([0.3], dtype=dt), torch.tensor([0.5], dtype=dt), torch.tensor([0.3], dtype=dt)
    inv_s, beta, gamma = O.inv_s_from_variance(var), O.beta_from_param(bp), O.gamma_from_param(gp)
    ro, rd, z, ds = d["ro"].to(dt), d["rd"].to(dt), d["z"].to(dt), d["ds"].to(dt)
    d_edge, d_depth = d["d_edge"].to(dt), d["d_depth"].to(dt)
    if mode == "unbiased":
        s = scalars.double()
        return M.composite_bwd(ro, rd, z, float(d["sd"]), d["udf"].to(dt), d["grads"].to(dt), inv_s, beta, gamma, car, fs, 0.05, None,
                               d_edge.view(N, 1), d_depth.view(N, 1), ds, float(0.1 / (s[4] + 1e-5)), float(0.05 / (s[6] + 1e-5)))[:2]
    assert mode == "plain"
    u = d["udf"].to(dt).requires_grad_(True)
    g = d["grads"].to(dt).requires_grad_(True)
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), float(d["sd"]), dtype=dt)], -1)
    E = torch.exp(-float(beta) * u)
    alpha = 1.0 - torch.exp(-torch.relu(float(beta) * E / (1 + E) ** 2) * float(gamma) * dists)
    w = alpha * torch.cumprod(torch.cat([torch.ones(N, 1, dtype=dt), 1.0 - alpha + 1e-7], -1), -1)[:, :-1]
    mid = z + dists * 0.5
    edge, depth = w.sum(-1), (mid * w).sum(-1) * ds
    pn = torch.linalg.norm(ro[:, None, :] + rd[:, None, :] * mid[..., None], dim=-1)
    relax, near = (pn < 2.4).to(dt), (u.detach() < 0.05).to(dt)
    err = (torch.linalg.norm(g, dim=-1) - 1.0) ** 2
    loss = ((d_edge * edge).sum() + (d_depth * depth).sum() + 0.1 * (relax * err).sum() / (relax.sum() + 1e-5)
            + 0.05 * (near * err).sum() / (near.sum() + 1e-5))
    loss.backward()
    return u.grad, g.grad


def _frozen_composite_inputs(a, d):
    return [a.frozen(d[k], k) for k in ("ro", "rd", "z", "udf", "grads", "ds")], a.frozen(d["sd"], "sample_dist")


@covers("emap_composite_fwd_p", "emap_composite_bwd")
@pytest.mark.parametrize("S", [2, 64, 65, 257, 1024])
@pytest.mark.parametrize("N", [1, 29])
@pytest.mark.parametrize("mode", list(MODES))
def test_compositing(mode, N, S):
    d = composite_inputs(N, S)
    A = _lib.api()
    for reduced in (False, True):
        def fwd(a, f):
            ins, sd = _frozen_composite_inputs(a, d)
            p = render_params(a, N, S, 0, 0, MODES[mode])
            co, out = composite_out(a, N, S, f.out, reduced)
            partials = a.buf((N, 8), torch.float32, f.ws, "partials")
            err = a.buf((1,), torch.int32, "zero", "err_flags")
            A.composite_fwd_p(*ins, N, S, sd, p, co, partials, err, stream())
            return {**out, "err_flags": err}
        o = extents(fwd, what=f"composite_fwd_p {mode} N={N} S={S} reduced={reduced}")
        if mode != "normcos":
            # 1e-4 of each tensor's max up to 256 samples per ray, 3e-4 above: the gates of the two tests the reference is taken from
            want = composite_forward_reference(d, mode)
            for k in ("edge", "depth") if reduced else ("alpha", "weights", "edge", "depth"):
                assert rel(o[k], want[k]) <= (1e-4 if S <= 256 else 3e-4), (k, rel(o[k], want[k]))
    scalars = torch.cat([o["scalars"].cpu(), torch.zeros(16 - SCALARS_WRITTEN)])
    for accumulate in (0, 1):
        def bwd(a, f):
            ins, sd = _frozen_composite_inputs(a, d)
            p = render_params(a, N, S, 0, 0, MODES[mode])
            cg = _lib.CompositeGrads()
            keep = [a.frozen(d["d_edge"], "d_edge"), a.frozen(d["d_depth"], "d_depth"), a.frozen(torch.tensor([0.1]), "d_ge"),
                    a.frozen(torch.tensor([0.05]), "d_ge_ns"), a.frozen(scalars, "scalars")]
            cg.d_edge, cg.d_depth, cg.d_gradient_error, cg.d_gradient_error_near_surface, cg.scalars = [t.data_ptr() for t in keep]
            fill = torch.tensor([0.25, -0.5, 2.0]) if accumulate else f.out
            dscal = a.buf((3,), torch.float32, fill, "d_variance/d_beta/d_gamma")
            cg.d_variance, cg.d_beta, cg.d_gamma = dscal.data_ptr(), dscal.data_ptr() + 4, dscal.data_ptr() + 8
            cg.grad_scale, cg.accumulate = 0.5, accumulate
            tail = a.buf((3,), torch.float32, torch.tensor([1.0, 2.0, 3.0]) if accumulate else f.out, "zero_tail")
            cg.zero_tail, cg.n_zero_tail = tail.data_ptr(), 3
            du = a.buf((N, S), torch.float32, f.out, "d_udf")
            dg = a.buf((N, S, 3), torch.float32, f.out, "d_grad3")
            partials = a.buf((N, 4), torch.float32, f.ws, "partials")
            A.composite_bwd(*ins, N, S, sd, p, cg, du, dg, partials, stream())
            return {"d_udf": du, "d_grad3": dg, "d_scalars": dscal, "zero_tail": tail}
        ob = extents(bwd, what=f"composite_bwd {mode} N={N} S={S} accumulate={accumulate}")
        if accumulate:
            assert ob["zero_tail"].tolist() == [1.0, 2.0, 3.0]        # cleared only when accumulate == 0
        else:
            assert ob["zero_tail"].tolist() == [0.0, 0.0, 0.0]
        assert bool(torch.isfinite(ob["d_udf"]).all()) and bool(torch.isfinite(ob["d_grad3"]).all())
        if mode != "normcos" and not accumulate and S <= 256:
            # d_udf and d_grad3 (they do not carry grad_scale) under the gate of the tests the reference is taken from: 1e-4 of each
            # tensor's max.  Not asserted above 256 samples per ray: those tests' 3e-4 was measured on 29 / 37 rays under one maximum, and
            # on the 1 and 29 rays of this test the fp32 arithmetic itself does not keep it - the SAME formulas in fp32 (the mirror on fp32
            # inputs) are 4e-5 ... 1.4e-3 off the fp64 mirror at S = 1024 depending on the seed of the rays (the kernels measured 1.4e-3 at
            # N = 1 and 3.5e-4 at N = 29 where the fp32 mirror is 1.4e-3 and 3.6e-4 off).  The adjoint's values at those sample counts are
            # tests/test_gpu_samples_per_ray.py's; here S = 257 and 1024 get the guards and checks (a) - (e).  The normcos mode has no
            # value reference in this file either, forward or adjoint: finiteness and (a) - (e) only.
            want_u, want_g = composite_backward_reference(d, mode, scalars)
            assert rel(ob["d_udf"], want_u) <= 1e-4 and rel(ob["d_grad3"], want_g) <= 1e-4, (rel(ob["d_udf"], want_u), rel(ob["d_grad3"], want_g))


@covers("emap_composite_fwd")
def test_composite_fwd_by_value():
    import math
    N, S = 29, 65
    d = composite_inputs(N, S)
    inv_s, beta, gamma = [min(max(math.exp(10 * v), 1e-6), 1e6) for v in (0.3, 0.5, 0.3)]

    def fwd(a, f, by_value):
        ins, sd = _frozen_composite_inputs(a, d)
        co, out = composite_out(a, N, S, f.out)
        partials = a.buf((N, 8), torch.float32, f.ws, "partials")
        err = a.buf((1,), torch.int32, "zero", "err_flags")
        if by_value:
            _lib.api().composite_fwd(*ins, N, S, sd, inv_s, beta, gamma, 1.0, 1, 0.9, 0.05, 25000.0, 0.0, 0, co, partials, err, stream())
        else:
            p = render_params(a, N, S, 0, 0, _lib.RENDER_UNBIASED)
            p.variance_dev = p.beta_dev = p.gamma_dev = None
            p.inv_s, p.beta, p.gamma, p.beta_min = inv_s, beta, gamma, 0.0
            _lib.api().composite_fwd_p(*ins, N, S, sd, p, co, partials, err, stream())
        return {**out, "err_flags": err}
    o = extents(lambda a, f: fwd(a, f, True), what="composite_fwd")
    o_p = extents(lambda a, f: fwd(a, f, False), what="composite_fwd_p, scalars by value")
    for k in o:      # emap_composite_fwd is emap_composite_fwd_p with the three scalars by value (csrc/api.hip): the same bits
        assert same_bits(o[k], o_p[k]), k


# ------------------------------------------------------------------------------------------------ forward render
# (n_samples, n_importance, up_sample_steps, N, render mode, emap_set_fused_sampling, emap_set_fused_composite, network)
RENDER_CASES = {
    "no_upsampling": (64, 0, 4, 33, "unbiased", 1, 1, "d8w256L10"),
    "fused_sampling_N1": (64, 64, 4, 1, "unbiased", 1, 1, "d8w256L10"),
    "fused_sampling_N33": (64, 64, 4, 33, "unbiased", 1, 1, "d8w256L10"),
    "fused_sampling_N33_d4": (64, 64, 4, 33, "unbiased", 1, 1, "d4w128L10"),
    "chain_N1": (64, 64, 4, 1, "unbiased", 0, 1, "d8w256L10"),
    "chain_N33": (64, 64, 4, 33, "unbiased", 0, 1, "d8w256L10"),
    "m_below_16": (64, 50, 5, 33, "unbiased", 1, 1, "d8w256L10"),
    "plain": (64, 64, 4, 33, "plain", 1, 1, "d8w256L10"),
    "normcos": (64, 64, 4, 33, "normcos", 1, 1, "d8w256L10"),
    "S_above_256": (64, 448, 4, 33, "unbiased", 1, 1, "d8w256L10"),
    "fused_composite": (64, 64, 4, 130, "unbiased", 1, 1, "d8w256L10"),
    "separate_composite": (64, 64, 4, 130, "unbiased", 1, 0, "d8w256L10"),
}
SAME_RESULT = [("fused_sampling_N1", "chain_N1"), ("fused_sampling_N33", "chain_N33"), ("fused_composite", "separate_composite")]


def render_capacity(cfg, pc, shape, N, mode):
    """arena bytes of one render case: the queried workspace, 64 B per sample of outputs, the bands of its ~30 buffers"""
    p = _lib.RenderParams()
    p.n_rays, p.n_samples, p.n_importance, p.up_sample_steps, p.render_mode = N, *shape, MODES[mode]
    m = shape[1] // shape[2] if shape[1] > 0 and shape[2] > 0 else 0
    return _lib.size_of("render_workspace_bytes", cfg, pc, p) + 64 * N * (shape[0] + m * shape[2]) + (64 << 20)


def render_case(cfg, pc, packed, shape, N, mode, jitter, sched=None, seed=5):
    ns, ni, steps = shape
    m = ni // steps if ni > 0 and steps > 0 else 0
    S = ns + m * steps
    rays = synthetic.make_rays(N, seed=seed)
    tr = synthetic.make_t_rand(N) if jitter else None

    def case(a, f):
        ro, rd, near, far, ds = [a.frozen(t.reshape(-1) if t.shape[-1] == 1 else t, k) for t, k in
                                 zip(rays, ("rays_o", "rays_d", "near", "far", "depth_scale"))]
        t_rand = a.frozen(tr.reshape(-1), "t_rand") if jitter else None
        p = render_params(a, N, ns, ni, steps, MODES[mode])
        out = {"z_vals": a.buf((N, S), torch.float32, f.out, "z_vals"), "udf": a.buf((N, S), torch.float32, f.out, "udf"),
               "grad3": a.buf((N, S, 3), torch.float32, f.out, "grad3")}
        co, cout = composite_out(a, N, S, f.out)
        nb = _lib.size_of("render_workspace_bytes", cfg, pc, p)
        ws = a.bytes(nb, f.ws, "workspace")
        sample_dist = ws[:4].view(torch.float32)      # the first float of the workspace: what emap_render_bwd is handed as sample_dist_dev
        if f.out == "nan":
            sample_dist.fill_(float("nan"))          # the sentinel check (c) looks for: the pattern's bytes are a finite float
        err = a.buf((1,), torch.int32, "zero", "err_flags")
        args = (cfg, packed, pc, p, ro, rd, near, far, t_rand, ds, out["z_vals"], out["udf"], out["grad3"], co, ws, nb, err, stream())
        if sched is None:
            _lib.api().render_fwd(*args)
        else:
            p.cos_anneal_ratio, p.flip_saturation = 0.123, 0.456            # not read: the kernels take both from sched_dev
            _lib.api().render_fwd_sched(*args, a.frozen(sched, "sched_dev"))
        return {**out, **cout, "err_flags": err, "sample_dist": sample_dist}
    return case, S


def run_render_case(nets, case, jitter):
    """one entry of RENDER_CASES under its launch switches, through extents()"""
    ns, ni, steps, N, mode, fused_sampling, fused_composite, name = RENDER_CASES[case]
    cfg, pc, packed, _, _, _ = nets(name, "f16x3")
    L = _lib.lib()
    prev = L.emap_set_fused_sampling(fused_sampling), L.emap_set_fused_composite(fused_composite)
    try:
        fn, S = render_case(cfg, pc, packed, (ns, ni, steps), N, mode, jitter)
        o = extents(fn, capacity=render_capacity(cfg, pc, (ns, ni, steps), N, mode), what=f"render_fwd {case} jitter={jitter}")
    finally:
        L.emap_set_fused_sampling(prev[0]), L.emap_set_fused_composite(prev[1])
    assert bool((o["z_vals"][:, 1:] >= o["z_vals"][:, :-1]).all())
    return o


@covers("emap_render_fwd")
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("case", [c for c in RENDER_CASES if not any(c in pair for pair in SAME_RESULT)])
def test_render_fwd(nets, case, jitter):
    run_render_case(nets, case, jitter)


@covers("emap_render_fwd")
@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("with_switch,without", SAME_RESULT)
def test_render_fwd_launch_switches(nets, with_switch, without, jitter):
    """the fused importance sampling against the launch chain, the fused compositing tail against the separate launches: each side through
    extents(), and the two the same bits (include/emap_hip.h: emap_set_fused_sampling, emap_set_fused_composite)"""
    a_, b_ = run_render_case(nets, with_switch, jitter), run_render_case(nets, without, jitter)
    for k, v in a_.items():
        assert same_bits(v, b_[k]), (with_switch, without, k)


@covers("emap_render_fwd_sched")
@pytest.mark.parametrize("case", ["fused_sampling_N33", "fused_composite", "plain"])
def test_render_fwd_sched(nets, case):
    ns, ni, steps, N, mode, _, _, name = RENDER_CASES[case]
    cfg, pc, packed, _, _, _ = nets(name, "f16x3")
    sched = torch.tensor([1e-3, 5e-3, 1.0, 0.9])         # [2] = cos_anneal_ratio, [3] = flip_saturation: render_params()'s by-value pair
    cap = render_capacity(cfg, pc, (ns, ni, steps), N, mode)
    by_value = extents(render_case(cfg, pc, packed, (ns, ni, steps), N, mode, True)[0], capacity=cap, what=f"render_fwd {case}")
    fed = extents(render_case(cfg, pc, packed, (ns, ni, steps), N, mode, True, sched=sched)[0], capacity=cap,
                  what=f"render_fwd_sched {case}")
    for k in by_value:
        assert same_bits(by_value[k], fed[k]), k


# ------------------------------------------------------------------------------------------------ backward
def param_grads(a, state, n_lin, f, weight_norm, accumulate):
    """(EmapParamGrads, keep-alive, {name: gradient buffer}): g / v frozen, every dg / dv / db an arena buffer of the parameter's shape"""
    g, v, b = gvb(state, n_lin)
    fg = [a.frozen(t, f"g{l}") for l, t in enumerate(g)]
    fv = [a.frozen(t, f"v{l}") for l, t in enumerate(v)]
    gen = torch.Generator().manual_seed(77)
    pre = (lambda t: torch.randn(t.shape, generator=gen) * 1e-3) if accumulate else (lambda t: f.out)
    out = {}
    for l in range(n_lin):
        if weight_norm:
            out[f"dg{l}"] = a.buf(g[l].shape, torch.float32, pre(g[l]), f"dg{l}")
        out[f"dv{l}"] = a.buf(v[l].shape, torch.float32, pre(v[l]), f"dv{l}")
        out[f"db{l}"] = a.buf(b[l].shape, torch.float32, pre(b[l]), f"db{l}")
    pg = _lib.ParamGrads()
    keep = [table(t.data_ptr() for t in fv), table(out[f"dv{l}"].data_ptr() for l in range(n_lin)),
            table(out[f"db{l}"].data_ptr() for l in range(n_lin))]
    pg.v_host, pg.dv_host, pg.db_host = keep
    if weight_norm:
        keep += [table(t.data_ptr() for t in fg), table(out[f"dg{l}"].data_ptr() for l in range(n_lin))]
        pg.g_host, pg.dg_host = keep[3], keep[4]
    pg.weight_norm, pg.accumulate, pg.grad_scale = int(weight_norm), int(accumulate), 0.5
    return pg, keep, out


def vjp_inputs(P):
    gen = torch.Generator().manual_seed(P + 1)
    return torch.rand(P, 3, generator=gen) * 2 - 1, torch.randn(P, generator=gen), torch.randn(P, 3, generator=gen) * 0.1


def vjp_case(cfg, pc, packed, state, P, nbytes, weight_norm, accumulate):
    x, du, dg = vjp_inputs(P)

    def case(a, f):
        xs, dus, dgs = a.frozen(x, "x"), a.frozen(du, "d_udf"), a.frozen(dg, "d_grad3")
        pg, keep, out = param_grads(a, state, cfg.n_lin, f, weight_norm, accumulate)
        ws = a.bytes(nbytes, f.ws, "workspace")
        err = a.buf((1,), torch.int32, "zero", "err_flags")
        _lib.api().udf_vjp(cfg, packed, pc, xs, P, dus, dgs, pg, ws, nbytes, err, stream())
        return {**out, "err_flags": err}
    return case


@covers("emap_udf_vjp")
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("weight_norm", [1, 0])
@pytest.mark.parametrize("P", [1, 33, 8192 + 1])
@pytest.mark.parametrize("name,prec", [("d8w256L10", "f16x3"), ("d4w128L10", "f16x3"), ("d8w256L10", "f16x3e")])
def test_udf_vjp(nets, name, prec, P, weight_norm, accumulate):
    cfg, pc, packed, state, _, _ = nets(name, prec)
    nb = _lib.size_of("udf_vjp_workspace_bytes", cfg, pc, P)
    o = extents(vjp_case(cfg, pc, packed, state, P, nb, weight_norm, accumulate), capacity=nb + (96 << 20),
                what=f"udf_vjp {name} {prec} P={P} weight_norm={weight_norm} accumulate={accumulate}")
    assert all(bool(torch.isfinite(v).all()) for v in o.values())
    if weight_norm and not accumulate and P <= 33:
        # against the fp64 mirror, as tests/test_gpu_backward.py:test_udf_vjp_ragged_sizes does and under its tolerances (TOL);
        # the outputs carry grad_scale = 0.5
        from test_gpu_backward import _mirror_param_grads, _cmp, TOL
        ref = _mirror_param_grads(state, nets(name, prec)[4], *vjp_inputs(P))
        key = {"dg": "lin{}.parametrizations.weight.original0", "dv": "lin{}.parametrizations.weight.original1", "db": "lin{}.bias"}
        got = {key[k[:2]].format(k[2:]): v.cpu() * 2.0 for k, v in o.items() if k != "err_flags"}
        assert set(got) == set(ref)
        _cmp(got, ref, TOL[prec], f"udf_vjp {name} {prec} P={P}")


@covers("emap_udf_vjp")
@pytest.mark.parametrize("name", NETS)
def test_udf_vjp_bounded_workspace(nets, name):
    """2 x 8192 + 77 points through the workspace of 8192: the bounded-workspace chunking of tests/test_gpu_backward.py's ws_points.  As
    there, one 4 KiB page is added to the size queried for 8192 points: the head of the workspace holds one word per tile of the ACTUAL
    launch, so the bare size is a little short of an 8192-point chunk of a longer launch (and is refused: EMAP_E_WORKSPACE)."""
    cfg, pc, packed, state, _, _ = nets(name, "f16x3")
    P = 2 * 8192 + 77
    nb = _lib.size_of("udf_vjp_workspace_bytes", cfg, pc, 8192) + 4096
    assert nb + 4096 < _lib.size_of("udf_vjp_workspace_bytes", cfg, pc, 8192 + 32)
    bounded = extents(vjp_case(cfg, pc, packed, state, P, nb, 1, 0), capacity=nb + (96 << 20), what=f"udf_vjp {name} bounded workspace")
    full_nb = _lib.size_of("udf_vjp_workspace_bytes", cfg, pc, P)
    full = extents(vjp_case(cfg, pc, packed, state, P, full_nb, 1, 0), capacity=full_nb + (96 << 20), what=f"udf_vjp {name} preferred workspace")
    for k, v in full.items():      # "same results to the rounding of the partial sums" (include/emap_hip.h): the bound of the chunking test
        if k != "err_flags":
            assert rel(bounded[k], v) <= 1e-3, (k, rel(bounded[k], v))


_forward_cache = {}


def forward_for_backward(nets, name, N, ns, ni, steps, mode):
    """z_vals, udf, grad3, scalars, sample_dist of one emap_render_fwd (its own arena, checked): the backward's inputs"""
    key = (name, N, ns, ni, steps, mode)
    if key not in _forward_cache:
        cfg, pc, packed, _, _, _ = nets(name, "f16x3")
        o = extents(render_case(cfg, pc, packed, (ns, ni, steps), N, mode, True, seed=9)[0], capacity=render_capacity(cfg, pc, (ns, ni, steps), N, mode),
                    what="render_fwd for the backward")
        _forward_cache[key] = {k: v.cpu() for k, v in o.items()}
    return _forward_cache[key]


def render_bwd_case(cfg, pc, packed, state, fw, shape, N, mode, weight_norm, accumulate, calls, sched=None):
    """`calls`: the stages of the emap_render_bwd_staged calls made in a row ((3,), (1, 2)), or None for emap_render_bwd"""
    ns, ni, steps = shape
    rays = synthetic.make_rays(N, seed=9)
    gen = torch.Generator().manual_seed(N)
    d_edge, d_depth = torch.randn(N, generator=gen) / N, torch.randn(N, generator=gen) * 0.1 / N
    scalars = torch.cat([fw["scalars"], torch.zeros(16 - SCALARS_WRITTEN)])

    def case(a, f):
        ro, rd, ds = a.frozen(rays[0], "rays_o"), a.frozen(rays[1], "rays_d"), a.frozen(rays[4].reshape(-1), "depth_scale")
        z, udf, g3, sd = [a.frozen(fw[k], k) for k in ("z_vals", "udf", "grad3", "sample_dist")]
        p = render_params(a, N, ns, ni, steps, MODES[mode])
        cg = _lib.CompositeGrads()
        keep = [a.frozen(d_edge, "d_edge"), a.frozen(d_depth, "d_depth"), a.frozen(torch.tensor([0.1]), "d_ge"),
                a.frozen(torch.tensor([0.05]), "d_ge_ns"), a.frozen(scalars, "scalars")]
        cg.d_edge, cg.d_depth, cg.d_gradient_error, cg.d_gradient_error_near_surface, cg.scalars = [t.data_ptr() for t in keep]
        dscal = a.buf((3,), torch.float32, torch.tensor([0.25, -0.5, 2.0]) if accumulate else f.out, "d_variance/d_beta/d_gamma")
        cg.d_variance, cg.d_beta, cg.d_gamma = dscal.data_ptr(), dscal.data_ptr() + 4, dscal.data_ptr() + 8
        cg.grad_scale, cg.accumulate = 0.5, accumulate
        tail = a.buf((3,), torch.float32, torch.tensor([1.0, 2.0, 3.0]) if accumulate else f.out, "zero_tail")
        cg.zero_tail, cg.n_zero_tail = tail.data_ptr(), 3
        pg, keep2, out = param_grads(a, state, cfg.n_lin, f, weight_norm, accumulate)
        nb = _lib.size_of("render_bwd_workspace_bytes", cfg, pc, p)
        ws = a.bytes(nb, f.ws, "workspace")
        err = a.buf((1,), torch.int32, "zero", "err_flags")
        args = (cfg, packed, pc, p, ro, rd, ds, z, udf, g3, sd, cg, pg, ws, nb, err, stream())
        if calls is None:
            _lib.api().render_bwd(*args)
        elif sched is not None:
            p.cos_anneal_ratio, p.flip_saturation = 0.123, 0.456
            sd_ = a.frozen(sched, "sched_dev")
            for st in calls:
                _lib.api().render_bwd_staged_sched(*args, st, sd_)
        else:
            for st in calls:
                _lib.api().render_bwd_staged(*args, st)
        return {**out, "d_scalars": dscal, "zero_tail": tail, "err_flags": err}
    return case


@covers("emap_render_bwd", "emap_render_bwd_staged", "emap_render_bwd_staged_sched")
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("weight_norm", [1, 0])
@pytest.mark.parametrize("name,N,shape,mode", [("d8w256L10", 33, (64, 64, 4), "unbiased"), ("d8w256L10", 3, (65, 192, 4), "unbiased"),
                                               ("d4w128L10", 33, (64, 64, 4), "plain"), ("d4w128L10", 3, (65, 192, 4), "normcos")])
def test_render_bwd(nets, name, N, shape, mode, weight_norm, accumulate):
    """N = 33, S = 128 and N = 3, S = 257: emap_render_bwd, the staged call with stages 3, with stages 1 then 2, and device-fed - all the
    same bits"""
    cfg, pc, packed, state, _, _ = nets(name, "f16x3")
    fw = forward_for_backward(nets, name, N, *shape, mode)
    S = fw["z_vals"].shape[1]
    assert S == shape[0] + shape[1] and (N, S) in ((33, 128), (3, 257))
    p = _lib.RenderParams()
    p.n_rays, p.n_samples, p.n_importance, p.up_sample_steps, p.render_mode = N, *shape, MODES[mode]
    cap = _lib.size_of("render_bwd_workspace_bytes", cfg, pc, p) + (128 << 20)
    tag = f"{name} N={N} S={S} {mode} weight_norm={weight_norm} accumulate={accumulate}"
    mk_case = lambda calls, sched=None: render_bwd_case(cfg, pc, packed, state, fw, shape, N, mode, weight_norm, accumulate, calls, sched)
    whole = extents(mk_case(None), capacity=cap, what="render_bwd " + tag)
    variants = {"stages 3": mk_case((3,)), "stages 1 then 2": mk_case((1, 2))}
    if accumulate == 0 and weight_norm == 1:
        variants["device-fed, stages 1 then 2"] = mk_case((1, 2), torch.tensor([1e-3, 5e-3, 1.0, 0.9]))
    for vname, case in variants.items():
        o = extents(case, capacity=cap, what=f"render_bwd_staged {vname} {tag}")
        for k, v in whole.items():
            assert same_bits(v, o[k]), (vname, k)
    assert all(bool(torch.isfinite(v).all()) for v in whole.values())
    assert whole["zero_tail"].tolist() == ([1.0, 2.0, 3.0] if accumulate else [0.0, 0.0, 0.0])


# ------------------------------------------------------------------------------------------------ training and rays
ADAM = (1e-3, 5e-3, 0.9, 0.999, 1e-8)     # lr_geo, lr, beta1, beta2, eps


@covers("emap_adam_step", "emap_adam_step_masked", "emap_adam_step_masked_sched")
@pytest.mark.parametrize("n", [1, 255, 257])
def test_adam(n):
    n_geo = n // 2
    nt = n - n_geo
    gen = torch.Generator().manual_seed(n)
    params, grads, m = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01
    mask = (torch.arange(nt) % 3 != 1).float()
    results = {}
    for which in ("plain", "masked", "masked_sched"):
        def case(a, f):
            st = {"params": a.buf((n,), torch.float32, params, "params"), "exp_avg": a.buf((n,), torch.float32, m, "exp_avg"),
                  "exp_avg_sq": a.buf((n,), torch.float32, v, "exp_avg_sq"), "step": a.buf((1,), torch.float32, torch.tensor([3.0]), "step_dev")}
            g = a.frozen(grads, "grads")
            head = (st["params"], g, st["exp_avg"], st["exp_avg_sq"], st["step"], n, n_geo)
            if which == "plain":
                _lib.api().adam_step(*head, *ADAM, stream())
                return st
            tm = a.frozen(mask, "tail_mask")
            st["tail_step"] = a.buf((nt,), torch.float32, torch.full((nt,), 3.0), "tail_step")
            if which == "masked":
                _lib.api().adam_step_masked(*head, *ADAM, tm, st["tail_step"], stream())
            else:
                _lib.api().adam_step_masked_sched(*head, a.frozen(torch.tensor(ADAM[:2]), "lr_dev"), *ADAM[2:], tm, st["tail_step"], stream())
            return st
        results[which] = extents(case, what=f"adam {which} n={n}")
    for k, v_ in results["masked"].items():
        assert same_bits(v_, results["masked_sched"][k]), k                 # device-fed learning rates: the same bits as by value
    frozen = n_geo + torch.nonzero(mask == 0).reshape(-1)
    assert torch.equal(results["masked"]["params"].cpu()[frozen], params[frozen])           # a frozen tail element: no update, no state change
    assert torch.equal(results["plain"]["params"].cpu()[:n_geo], results["masked"]["params"].cpu()[:n_geo])
    assert not torch.equal(results["plain"]["params"].cpu(), params)
    # one torch.optim.Adam step (no weight decay, no amsgrad) at step 4 in float64, under tests/test_gpu_adam.py's tolerance
    lr_geo, lr, b1, b2, eps = ADAM
    g64, lrs = grads.double(), torch.cat([torch.full((n_geo,), lr_geo), torch.full((nt,), lr)]).double()
    m1, v1 = b1 * m.double() + (1 - b1) * g64, b2 * v.double() + (1 - b2) * g64 * g64
    want = params.double() - lrs / (1 - b1 ** 4) * m1 / (v1.sqrt() / (1 - b2 ** 4) ** 0.5 + eps)
    got = results["plain"]
    assert float(got["step"]) == 4.0 and torch.allclose(got["params"].cpu().double(), want, rtol=2e-6, atol=1e-7)
    assert torch.allclose(got["exp_avg"].cpu().double(), m1, rtol=2e-6, atol=1e-7) and torch.allclose(got["exp_avg_sq"].cpu().double(), v1, rtol=2e-6, atol=1e-7)


@covers("emap_train_stats", "emap_train_loss", "emap_train_schedule", "emap_train_monitor")
@pytest.mark.parametrize("N", [1, 257])
def test_training_tail(N):
    S = 132
    gen = torch.Generator().manual_seed(N)
    edge, true_edge = torch.rand(N, generator=gen), torch.rand(N, generator=gen)
    scalars = torch.rand(16, generator=gen) + 0.5
    udf, wsum = torch.rand(N, S, generator=gen) * 0.2, torch.rand(N, generator=gen)
    A = _lib.api()

    def stats(a, f):
        out = {"d_edge": a.buf((N,), torch.float32, f.out, "d_edge"), "stats5": a.buf((5,), torch.float32, f.out, "stats5")}
        A.train_stats(a.frozen(edge, "edge"), a.frozen(true_edge, "true_edge"), a.frozen(scalars, "scalars"), N, 2.0 * 0.7 / N, out["d_edge"],
                      out["stats5"], stream())
        return out
    o = extents(stats, what=f"train_stats N={N}")
    assert rel(o["d_edge"], (edge - true_edge).double() * (2.0 * 0.7 / N)) <= 1e-6
    assert rel(o["stats5"][4], ((edge - true_edge).double() ** 2).sum()) <= 1e-5
    assert o["stats5"][:4].tolist() == [float(scalars[i]) for i in (4, 6, 3, 5)]
    stats5 = o["stats5"].cpu()

    def loss(a, f):
        out2 = a.buf((2,), torch.float32, f.out, "out2")
        A.train_loss(a.frozen(stats5, "stats5"), 0.7 / N, 0.1, 0.05, out2, stream())
        return {"out2": out2}
    o_loss = extents(loss, what="train_loss")

    def schedule(a, f):
        it = a.buf((1,), torch.int64, torch.tensor([5]), "iter_dev")
        sched = a.buf((4,), torch.float32, f.out, "sched_dev")
        A.train_schedule(it, 12, 2.0, 1.0, 4.0, 5e-4, 1e-4, 0.05, 0, 3, 0.9, sched, stream())
        return {"iter_dev": it, "sched_dev": sched}
    o_s = extents(schedule, what="train_schedule")
    assert int(o_s["iter_dev"].item()) == 6
    sched = o_s["sched_dev"].cpu()
    nb = _lib.size_of("train_monitor_workspace_bytes", N)

    def monitor(a, f):
        record = a.buf((_lib.MON_FIELDS,), torch.float64, "zero", "record")          # a zeroed record: an empty monitor
        ring = a.buf((5, _lib.MON_ROW), torch.float64, "zero", "ring")               # one row per call is written: the caller's history
        out2 = a.buf((2,), torch.float32, f.out, "loss_out2")
        ws = a.bytes(nb, "zero", "workspace")                                        # zeroed once by the caller: the header's contract
        A.train_monitor(a.frozen(udf, "udf"), a.frozen(wsum, "weight_sum"), N, S, a.frozen(stats5, "stats5"), a.frozen(scalars, "scalars"),
                        a.frozen(sched, "sched_dev"), a.frozen(torch.tensor([6]), "iter_dev"), 0.7 / N, 0.1, 0.05, N, 3, 5, record, ring, out2,
                        ws, nb, stream())
        return {"record": record, "ring": ring, "loss_out2": out2, "ticket": ws[:8].view(torch.int64)}
    o_m = extents(monitor, what=f"train_monitor N={N}")
    assert same_bits(o_m["loss_out2"], o_loss["out2"])                               # exactly as emap_train_loss writes them
    assert int(o_m["ticket"].item()) == 0                                            # every call leaves its ticket word zero again
    rec = o_m["record"].tolist()
    assert rec[_lib.MON["iter_step"]] == 6.0 and rec[_lib.MON["steps"]] == 1.0
    assert rec[_lib.MON["udf_mean"]] == pytest.approx(float(udf.double().mean()), rel=1e-6)


def _dataset(a):
    """the three-image scene of tests/test_gpu_ray_draw.py, uploaded as DeviceRaySampler uploads it, frozen in the arena"""
    from test_gpu_ray_draw import sampler
    s = sampler("A")
    t = {k: a.frozen(getattr(s, "_" + k), k) for k in ("edges", "order", "n_edge", "density", "kinv", "pose")}
    perm = a.frozen(torch.tensor([2, 0, 1], dtype=torch.int32), "image_perm")
    ds = _lib.RayDataset(t["edges"].data_ptr(), t["order"].data_ptr(), t["n_edge"].data_ptr(), t["density"].data_ptr(), t["kinv"].data_ptr(),
                         t["pose"].data_ptr(), perm.data_ptr(), s.n_images, s.H, s.W, 0)
    return ds, s


def _ray_batch(a, f, batch):
    widths = {"rays_o": 3, "rays_v": 3, "edge": 1, "depth_scale": 1, "ndc_uv": 2, "p_cam": 3}
    out = {k: a.buf((batch, w), torch.float32, f.out, k) for k, w in widths.items()}
    out["pixels"] = a.buf((batch, 2), torch.int64, f.out, "pixels")
    out["img_idx"] = a.buf((1,), torch.int32, f.out, "img_idx")
    out["t_rand"] = a.buf((batch,), torch.float32, f.out, "t_rand")
    rb = _lib.RayBatch(*[out[k].data_ptr() for k, _ in _lib.RayBatch._fields_])
    return rb, out


@covers("emap_sample_rays", "emap_sample_rays_train")
@pytest.mark.parametrize("importance", [0, 1])
@pytest.mark.parametrize("batch", [1, 1023, 1025])
def test_sample_rays(batch, importance):
    def plain(a, f, img):
        ds, _ = _dataset(a)
        rb, out = _ray_batch(a, f, batch)
        counter = a.buf((1,), torch.int64, torch.tensor([7]), "counter_dev")
        _lib.api().sample_rays(ds, img, batch, importance, 5, 0, counter, None, rb, stream())
        return {**out, "counter_dev": counter}

    def train(a, f):
        ds, _ = _dataset(a)
        rb, out = _ray_batch(a, f, batch)
        counter = a.buf((1,), torch.int64, torch.tensor([7]), "counter_dev")
        images = a.frozen(torch.tensor([2, 0], dtype=torch.int32), "train_images")
        perm = a.buf((2,), torch.int32, f.out, "perm")
        tag = a.buf((1,), torch.int64, torch.tensor([-1]), "epoch_tag")
        _lib.api().sample_rays_train(ds, images, 2, perm, tag, batch, importance, 5, counter, None, rb, stream())
        return {**out, "counter_dev": counter, "perm": perm, "epoch_tag": tag}
    for img in (1, -1):
        o = extents(lambda a, f: plain(a, f, img), what=f"sample_rays batch={batch} importance={importance} img={img}")
        assert int(o["counter_dev"].item()) == 8 and int(o["img_idx"].item()) == (1 if img == 1 else [2, 0, 1][7 % 3])
        assert bool((o["pixels"][:, 0] >= 0).all()) and bool((o["pixels"][:, 0] < 30).all()) and bool((o["pixels"][:, 1] < 20).all())
    o = extents(train, what=f"sample_rays_train batch={batch} importance={importance}")
    assert int(o["counter_dev"].item()) == 8 and int(o["epoch_tag"].item()) == 3 and sorted(o["perm"].tolist()) == [0, 2]
    assert int(o["img_idx"].item()) == int(o["perm"][7 % 2])


@covers("emap_gen_rays_at")
@pytest.mark.parametrize("level", [1, 3])
def test_gen_rays_at(level):
    def gen(a, f, first, count):
        ds, _ = _dataset(a)
        out = {"rays_o": a.buf((count, 3), torch.float32, f.out, "rays_o"), "rays_d": a.buf((count, 3), torch.float32, f.out, "rays_d"),
               "depth_scale": a.buf((count,), torch.float32, f.out, "depth_scale")}
        _lib.api().gen_rays_at(ds, 1, level, first, count, out["rays_o"], out["rays_d"], out["depth_scale"], stream())
        return out
    h, w = 20 // level, 30 // level
    n = h * w
    whole = extents(lambda a, f: gen(a, f, 0, n), what=f"gen_rays_at level={level} whole view")
    mid = w + w // 2 + 1                                            # a chunk that ends mid-row, and the one that ends at the last pixel
    for first, count in ((0, mid), (mid, n - mid), (n - 1, 1)):
        o = extents(lambda a, f: gen(a, f, first, count), what=f"gen_rays_at level={level} [{first}, {first + count})")
        for k, v in o.items():
            assert same_bits(v, whole[k][first:first + count]), (k, first, count)


# ------------------------------------------------------------------------------------------------ extraction, metrics, parametric edges
@covers("emap_null_direction")
@pytest.mark.parametrize("n", [1, 63, 65])
def test_null_direction(n):
    k = 50
    grads = torch.randn(n, k, 3, generator=torch.Generator().manual_seed(n))

    def case(a, f):
        d = a.buf((n, 3), torch.float32, f.out, "dir")
        _lib.api().null_direction(a.frozen(grads, "grads"), n, k, d, stream())
        return {"dir": d}
    o = extents(case, what=f"null_direction n={n}")
    assert rel(o["dir"].norm(dim=1), torch.ones(n)) <= 1e-5


@covers("emap_lattice_points", "emap_jitter_points", "emap_shift_points")
def test_extraction_stages():
    N, first, count = 12, 12 ** 3 // 3 + 1, 12 ** 3 // 2 + 1          # a range that starts and ends mid-row

    def lattice(a, f):
        xyz = a.buf((count, 3), torch.float32, f.out, "xyz")
        _lib.api().lattice_points(N, first, count, xyz, stream())
        return {"xyz": xyz}
    o = extents(lattice, what="lattice_points")
    axis = torch.arange(N, dtype=torch.float32) * (2.0 / (N - 1)) + (-1)
    ref = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=-1).reshape(-1, 3)
    assert torch.equal(o["xyz"].cpu(), ref[first:first + count])
    for n, k in ((1, 1), (301, 50), (4097, 3)):
        gen = torch.Generator().manual_seed(n + k)
        x, noise = torch.rand(n, 3, generator=gen) * 2 - 1, torch.randn(n, k, 3, generator=gen)
        df, nrm = torch.rand(n, generator=gen), torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=1)

        def jitter(a, f):
            out = a.buf((n * k, 3), torch.float32, f.out, "out")
            _lib.api().jitter_points(a.frozen(x, "x"), a.frozen(noise, "noise"), n, k, 0.005, out, stream())
            return {"out": out}

        def shift(a, f):
            out = a.buf((n, 3), torch.float32, f.out, "out")
            _lib.api().shift_points(a.frozen(x, "x"), a.frozen(df, "df"), a.frozen(nrm, "normal"), n, out, stream())
            return {"out": out}
        # the fp32 torch expressions (tests/test_gpu_pointcloud.py), evaluated on the device as there: multiply, then add
        xd, nd, dd, rd = x.to(DEV), noise.to(DEV), df.to(DEV), nrm.to(DEV)
        assert torch.equal(extents(jitter, what=f"jitter_points n={n} k={k}")["out"], (xd.unsqueeze(1) + 0.005 * nd).reshape(-1, 3))
        assert torch.equal(extents(shift, what=f"shift_points n={n}")["out"], xd + dd.unsqueeze(-1) * rd)


@covers("emap_compact_append")
@pytest.mark.parametrize("n", [1, 2049, 3 * 2048 + 5])
def test_compact_append(n):
    gen = torch.Generator().manual_seed(n)
    df, xyz = torch.rand(n, generator=gen), torch.randn(n, 3, generator=gen)
    df[::5] = 0.25
    df[0] = 0.1
    mask = df <= 0.25
    keep = int(mask.sum())                                           # capacity = exactly the survivor count
    nb = _lib.size_of("compact_workspace_bytes", n)

    def case(a, f):
        out = {"out_xyz": a.buf((keep, 3), torch.float32, f.out, "out_xyz"), "out_df": a.buf((keep,), torch.float32, f.out, "out_df"),
               "out_idx": a.buf((keep,), torch.int64, f.out, "out_idx")}
        state = a.buf((4,), torch.int64, "zero", "state")              # zeroed by the caller before the first call
        ws = a.bytes(nb, f.ws, "workspace")
        _lib.api().compact_append(a.frozen(df, "df"), a.frozen(xyz, "xyz"), n, 100, 0.25, 1, out["out_xyz"], out["out_df"], out["out_idx"], keep,
                                  state, ws, nb, stream())
        return {**out, "state": state}
    o = extents(case, what=f"compact_append n={n}")
    assert o["state"].tolist() == [keep, 0, 1, 0]
    assert torch.equal(o["out_idx"].cpu(), torch.where(mask)[0] + 100) and torch.equal(o["out_df"].cpu(), df[mask])
    assert torch.equal(o["out_xyz"].cpu(), xyz[mask])


@covers("emap_nearest_neighbors", "emap_dist_stats")
@pytest.mark.parametrize("n_q,n_r", [(1, 1), (65, 1027), (2049, 77)])
def test_metrics(n_q, n_r):
    from edge_metrics_ref import nn_ref, ulp_diff
    gen = torch.Generator().manual_seed(n_q + n_r)
    q, r = torch.rand(n_q, 3, generator=gen), torch.rand(n_r, 3, generator=gen)
    nb = _lib.size_of("nn_workspace_bytes", n_q)

    def search(a, f):
        out = {"dist": a.buf((n_q,), torch.float32, f.out, "dist"), "idx": a.buf((n_q,), torch.int64, f.out, "idx")}
        ws = a.bytes(nb, f.ws, "workspace")
        _lib.api().nearest_neighbors(a.frozen(q, "q"), n_q, a.frozen(r, "r"), n_r, 0, out["dist"], out["idx"], ws, nb, stream())
        return out
    o = extents(search, what=f"nearest_neighbors n_q={n_q} n_r={n_r}")
    _, want_d, want_i = nn_ref(q.numpy(), r.numpy())
    # tests/test_gpu_edge_metrics.py's standard: the index bit for bit, dist within 1 ulp of np.sqrt(d2)
    assert torch.equal(o["idx"].cpu(), torch.from_numpy(want_i).to(torch.int64)) and int(ulp_diff(o["dist"].cpu().numpy(), want_d).max()) <= 1
    dist = o["dist"].cpu()
    thr = (C.c_float * 3)(0.05, 0.1, 0.2)

    def stats(a, f):
        out = a.buf((4,), torch.float64, f.out, "out")
        _lib.api().dist_stats(a.frozen(dist, "dist"), n_q, thr, 3, out, stream())
        return {"out": out}
    s = extents(stats, what=f"dist_stats n={n_q}")["out"].tolist()
    assert s[0] == pytest.approx(float(dist.double().sum()), rel=1e-12)
    assert s[1:] == [float((dist < t).sum()) for t in (torch.tensor(0.05), torch.tensor(0.1), torch.tensor(0.2))]


@covers("emap_edge_sample_counts", "emap_edge_sample_fill", "emap_edge_sample_fill_tangents")
@pytest.mark.parametrize("n_curves,n_lines", [(3, 5), (0, 1), (67, 0)])
def test_parametric_edges(n_curves, n_lines):
    gen = torch.Generator().manual_seed(10 * n_curves + n_lines)
    curves = torch.rand(n_curves, 4, 3, generator=gen, dtype=torch.float64)
    lines = torch.rand(n_lines, 2, 3, generator=gen, dtype=torch.float64)
    E = n_curves + n_lines
    A = _lib.api()

    def inputs(a):
        return (a.frozen(curves, "curves") if n_curves else None, n_curves, a.frozen(lines, "lines") if n_lines else None, n_lines)

    def counts(a, f):
        out = {"lengths": a.buf((E,), torch.float64, f.out, "lengths"), "counts": a.buf((E,), torch.int64, f.out, "counts")}
        A.edge_sample_counts(*inputs(a), 0.05, 16, out["lengths"], out["counts"], stream())
        return out
    o = extents(counts, what=f"edge_sample_counts C={n_curves} L={n_lines}")
    assert torch.equal(o["counts"].cpu(), torch.floor(o["lengths"].cpu() / 0.05).to(torch.int64))
    if n_lines:
        assert rel(o["lengths"][n_curves:], (lines[:, 1] - lines[:, 0]).norm(dim=1)) <= 1e-12
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(o["counts"].cpu(), 0)])
    n = int(offsets[-1])
    assert n > 0

    def fill(a, f, tangents, optional):
        out = {"points": a.buf((n, 3), torch.float64, f.out, "points")}
        if optional:
            out["directions"] = a.buf((n, 3), torch.float64, f.out, "directions")
            out["edge_id"] = a.buf((n,), torch.int32, f.out, "edge_id")
        off = a.frozen(offsets, "offsets")
        if tangents:
            out["tangents"] = a.buf((n, 3), torch.float64, f.out, "tangents")
            A.edge_sample_fill_tangents(*inputs(a), off, out["points"], out.get("directions"), out["tangents"], out.get("edge_id"), n, stream())
        else:
            A.edge_sample_fill(*inputs(a), off, out["points"], out.get("directions"), out.get("edge_id"), n, stream())
        return out
    full = extents(lambda a, f: fill(a, f, True, True), what="edge_sample_fill_tangents")
    for tangents, optional in ((False, True), (False, False), (True, False)):
        o2 = extents(lambda a, f: fill(a, f, tangents, optional), what=f"edge_sample_fill tangents={tangents} optional={optional}")
        for k, v in o2.items():
            assert same_bits(v, full[k]), k
    assert torch.equal(full["edge_id"].cpu(), torch.repeat_interleave(torch.arange(E, dtype=torch.int32), o["counts"].cpu()))
