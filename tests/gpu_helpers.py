"""What several GPU test modules (tests/test_gpu_*.py, -m gpu) and the probes under scripts/ share: the device, the error measures, the
seeded networks and renderer of the goldens, render_core through the C ABI on given z_vals, the measured bounds of the sampler's
discontinuity, and the fused importance sampler against the launch chain.  A plain module: not collected, no tests of its own.  Helpers that differ between files in arithmetic, seeds or shapes
stay in their files."""
import ctypes as C

import torch

from conftest import t, net_state
import emap_amd
from emap_amd import _lib, synthetic
from oracle import emap_oracle as O

DEV = "cuda:0"


# ---------------------------------------------------------------------------------------- error measures
def rel(a, b):
    a = a.detach().cpu().double().reshape(-1)
    b = b.detach().cpu().double().reshape(-1)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def rel_floored(a, b):
    """max-normalised difference.  The floor of 1e-4 stands for the fp32 noise of quantities that are all near zero: the d8 network's
    plain-mode edge is 0 and its normalised-cosine weights sit at ~1e-5 (the + 1e-5 of sample_pdf's scale), where |g| from sqrt vs
    torch.linalg.norm alone moves them by an ulp."""
    a = a.detach().cpu().double().reshape(-1)
    b = b.detach().cpu().double().reshape(-1)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-4))


def rel_p999(a, b, floor=1e-6):
    """99.9th percentile of the ELEMENT-WISE relative error |a - b| / max(|b|, floor * max|b|)."""
    a = a.detach().cpu().double().reshape(-1)
    b = b.detach().cpu().double().reshape(-1)
    e = (a - b).abs() / torch.clamp(b.abs(), min=floor * float(b.abs().max()))
    return float(torch.quantile(e, 0.999)) if e.numel() > 1 else float(e.max())


# ---------------------------------------------------------------------------------------- guard-band coverage of a header
def assert_covered_or_excluded(symbols, covered, excluded, namespace):
    """Every entry point of the binding table `symbols` is in exactly one of a test module's two tables: `covered` - it returns an rc and
    names guard-band cases that exist in `namespace` -, or `excluded` as "host-only" - no parameter of it is a device pointer."""
    for name in symbols:
        assert (name in covered) != (name in excluded), name
    assert not (set(covered) | set(excluded)) - set(symbols)
    for name, cases in covered.items():
        assert symbols[name][0] is _lib._RC and cases and all(c in namespace for c in cases), name
    for name, reason in excluded.items():
        assert reason == "host-only" and _lib._P not in symbols[name][1], name


# ---------------------------------------------------------------------------------------- networks and renderer of the goldens
def mk(name, precision="f16x3", scale=1.0):
    kw, state = net_state(name)
    net = emap_amd.UDFNetwork(scale=scale, precision=precision, **kw)
    net.load_state_dict(state)
    cfg = O.UDFConfig(d_hidden=kw["d_hidden"], n_layers=kw["n_layers"], multires=kw["multires"], scale=scale)
    return net.to(DEV), state, cfg


def mk_renderer(net, ns, ni, steps, **mode):
    """`mode`: the render-mode switches of UDFRendererBlending (use_unbias_render, use_norm_grad_for_cosine); none = the default mode."""
    dev = emap_amd.SingleVarianceNetwork(0.3).to(DEV)
    bet = emap_amd.BetaNetwork(0.5, 0.3, 0.3, 5e-5, True, True, False).to(DEV)
    return emap_amd.UDFRendererBlending(None, net, dev, bet, ns, ni, 0, steps, 1.0, device=DEV, **mode)


# ---------------------------------------------------------------------------------------- the sampler's discontinuity
# measured on MI355X (round 2) + margin: fraction of rays with any sample moved by > 1e-3 w.r.t. the reference's z_vals (the
# sampler is discontinuous in its inputs; the per-step kernels are bit-exact on reference inputs, see the chain test of
# tests/test_gpu_parity.py) (measured 0.062 / 0.031 / 0.25 / 0.0)
MOVED_BOUND = {"c64_50_5": 0.13, "c64_64_4": 0.10, "c32_32_4_small": 0.35, "c64_64_4_L6": 0.07}
# up-sampling steps on reference inputs (max over steps): (index mismatch fraction, fraction of samples off by > 2e-6, the same among
# the well-conditioned samples, fraction of rays whose chained final z_vals equal the golden's) - measured on MI355X (round 2) + margin
# measured: indices 0 / 0 / 0 mismatches; samples 0 / 0 / 3.5 % (one |p| < 1 decision of the d4 case flips); chained rays equal to the
# golden 97 / 94 / 81 % - the CPU oracle on the same host reaches 97 / 94 / 62 % against the golden recorded on another CPU
CHAIN_BOUND = {"c64_64_4": (0.002, 0.01, 0.01, 0.90), "c64_50_5": (0.002, 0.01, 0.01, 0.85), "c32_32_4_small": (0.002, 0.07, 0.07, 0.70)}


def _well_conditioned(z, weights, inds, m):
    """samples whose inverse-CDF lerp is well conditioned: the pdf mass of their interval is >= 1e-3 (sample_pdf :92-96 divides
    by it; in empty intervals the reference's own result depends on the last ulp of its cumsum)"""
    w = weights + 1e-5
    pdf = w / w.sum(-1, keepdim=True)
    below = (inds - 1).clamp(min=0)
    above = inds.clamp(max=z.shape[1] - 1)
    mass = torch.where(above > below, torch.gather(pdf, 1, below.clamp(max=pdf.shape[1] - 1)), torch.zeros_like(z[:, :m]))
    return mass >= 1e-3


# ---------------------------------------------------------------------------------------- render_core on fixed z
def _render_core_on_z(net, r, g, z, car, fs, bg=None):
    """MLP value+grad at the reference's z_vals + emap_composite_fwd_p: render_core (:418-677) through the C ABI."""
    L = _lib.lib()
    ro, rd, near, far, ds = [t(g[k]).to(DEV) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    N, S = z.shape
    sd = ((far - near) / r.n_samples).mean().reshape(1)
    z = z.to(DEV).contiguous()
    dists = torch.cat([z[:, 1:] - z[:, :-1], sd.expand(N, 1)], -1)
    mid = z + dists * 0.5
    pts = (ro[:, None, :] + rd[:, None, :] * mid[..., None]).reshape(-1, 3)
    with torch.no_grad():
        udf, grad = net.hip_udf(pts, with_grad=True)
    p = r._params(N, car, fs, bg)
    names = ["weights", "alpha", "mid_z", "dists", "inside_sphere", "gradient_mag"]
    bufs = {k: torch.empty(N, S, device=DEV) for k in names}
    bufs.update(gradients_flip=torch.empty(N, S, 3, device=DEV), edge=torch.empty(N, 1, device=DEV), depth=torch.empty(N, 1, device=DEV),
                weight_sum=torch.empty(N, 1, device=DEV), normals=torch.empty(N, 3, device=DEV), scalars=torch.zeros(16, device=DEV))
    co = _lib.CompositeOut()
    for k, v in bufs.items():
        setattr(co, k, v.data_ptr())
    partials = torch.empty(N, 8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ds_flat = ds.reshape(-1).contiguous()
    _lib.check(L.emap_composite_fwd_p(_lib.ptr(ro), _lib.ptr(rd), _lib.ptr(z), _lib.ptr(udf), _lib.ptr(grad), _lib.ptr(ds_flat),
                                      N, S, _lib.ptr(sd), C.byref(p), C.byref(co), _lib.ptr(partials), _lib.ptr(err), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    out = dict(bufs)
    out.update(udf=udf.view(N, S), gradients=grad.view(N, S, 3), mid_z_vals=bufs["mid_z"], gradient_error=bufs["scalars"][0],
               gradient_error_near_surface=bufs["scalars"][1])
    return out


# ---------------------------------------------------------------------------------------- fused importance sampling vs the launch chain
def _fused_vs_chain(netname, N, prec, n_samples=64, n_importance=64, steps=4, fused_mode=(2, 1)):
    """ABI v8: importance_sample (udf_renderer_blending.py:802-841) as ONE launch - the sampler steps run inside the workgroups of the narrow MLP
    passes, the ray's lists stay in LDS (udf_mlp_kernel.inc, IS) - against the chain of 2 K - 1 launches it replaces
    (emap_set_fused_sampling(0)): z_vals and every rendered quantity identical bit for bit (same device code, same arithmetic), for every
    workgroup geometry the launcher picks (2 rays x 8 waves, 2 x 4, 1 x 8 / 1 x 4, odd ray counts), with and without the per-ray jitter.
    `fused_mode`: one mode or several, each against one render of the chain - 2: the fused kernel whatever the size rule of
    launch_is_mode says (the rule hands 768 ... 1024 rays at m = 16 to the chain), 1: the rule's pick."""
    modes = fused_mode if isinstance(fused_mode, tuple) else (fused_mode,)
    net, _, _ = mk(netname, prec)
    r = mk_renderer(net, n_samples, n_importance, steps)
    ro, rd, near, far, ds = [v.to(DEV) for v in synthetic.make_rays(N, seed=5)]
    tr = synthetic.make_t_rand(N).to(DEV)
    L = _lib.lib()
    outs = {}
    try:
        for fused in modes + (0,):
            L.emap_set_fused_sampling(fused)
            with torch.no_grad():
                o1 = r.render(ro, rd, near, far, ds, cos_anneal_ratio=1.0, flip_saturation=0.9, t_rand=tr)
                o2 = r.render(ro, rd, near, far, ds, cos_anneal_ratio=1.0, perturb_overwrite=0, flip_saturation=0.9)
            torch.cuda.synchronize()
            r.check_errors()
            outs[fused] = {tag + k: v.clone() for tag, o in (("jitter.", o1), ("plain.", o2)) for k, v in o.items() if isinstance(v, torch.Tensor)}
    finally:
        L.emap_set_fused_sampling(1)
    b = outs[0]
    for fused in modes:
        a = outs[fused]
        assert set(a) == set(b) and "jitter.z_vals" in a and "plain.z_vals" in a
        assert a["jitter.z_vals"].shape == (N, n_samples + n_importance)
        for k in a:
            assert torch.equal(a[k], b[k]), (fused, k)
