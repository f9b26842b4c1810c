"""The training backward bit for bit: sha256 of the flat parameter-gradient buffer after emap_udf_vjp and emap_render_bwd[_staged].

The parity tests (test_gpu_backward.py, test_gpu_render_modes.py) bound the gradients by tolerances; a host-side slip - a wrong stash
offset, chunk boundary, pass order or accumulate flag - could hide under them.  The backward is deterministic
(test_large_launches_are_bit_stable_run_to_run), so every case here compares the digest of the WHOLE flat buffer, the slots the call
leaves alone included, with the digest recorded on an MI355X from the library as it stood before the backward's host path (plan_vjp,
run_vjp, the wgrad launchers) was consolidated.  The points and loss gradients of the emap_udf_vjp cases come from numpy's PCG64 and the
weights from synthetic.make_udf_state: they do not depend on the torch version."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden, t
from emap_amd import _lib
from emap_amd.backward import ParamLayout
from gpu_helpers import mk, mk_renderer, DEV, _render_core_on_z
from test_gpu_render_modes import _setup, _train_golden

pytestmark = pytest.mark.gpu


def _digest(flat):
    torch.cuda.synchronize()
    return hashlib.sha256(flat.cpu().numpy().tobytes()).hexdigest()


def _ws_bytes(net, P):
    nb = C.c_size_t()
    cfg = net.net_config()
    _lib.check(_lib.lib().emap_udf_vjp_workspace_bytes(C.byref(cfg), _lib.PRECISIONS[net.precision], P, C.byref(nb)))
    return nb.value


def udf_vjp_digest(name, prec, P, ws_points=None, accumulate=0, weight_norm=1):
    """emap_udf_vjp on P points.  ws_points: the workspace is the preferred one of a launch of that many points (fewer than P: several chunks).
    The flat buffer starts as a fixed pattern: accumulate = 1 adds to it, weight_norm = 0 leaves the g slots as they are."""
    net, _, _ = mk(name, prec)
    rng = np.random.Generator(np.random.PCG64(1000 + P))
    x = torch.from_numpy((rng.random((P, 3), dtype=np.float32) * 2 - 1)).to(DEV)
    du = torch.from_numpy(rng.standard_normal(P, dtype=np.float32) * np.float32(1e-3)).to(DEV)
    dg = torch.from_numpy(rng.standard_normal((P, 3), dtype=np.float32) * np.float32(1e-4)).to(DEV)
    lay = ParamLayout(net)
    flat = (torch.arange(lay.numel, dtype=torch.float32, device=DEV) % 17 - 8) * 2.0 ** -12
    pg, keep = lay._tables(flat)
    pg.accumulate = accumulate
    if not weight_norm:
        pg.weight_norm, pg.g_host, pg.dg_host = 0, None, None
    nbytes = _ws_bytes(net, P if ws_points is None else ws_points)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    cfg = net.net_config()
    _lib.check(_lib.lib().emap_udf_vjp(C.byref(cfg), _lib.ptr(net.packed()), _lib.PRECISIONS[prec], _lib.ptr(x), P, _lib.ptr(du), _lib.ptr(dg),
                                       C.byref(pg), _lib.ptr(ws), nbytes, _lib.ptr(err), _lib.stream_ptr()), "udf_vjp")
    d = _digest(flat)
    assert int(err.item()) == 0
    return d


def render_bwd_digest(mode, stages):
    """emap_render_bwd_staged on the training golden of one render mode, once per entry of `stages`, into a flat buffer full of NaN"""
    if mode == "default":
        g = load_golden("g6_training_0")
        net, _, _ = mk(str(g["netname"]), "f16x3")
        ns, ni, steps = [int(v) for v in g["cfg"]]
        r = mk_renderer(net, ns, ni, steps)
        ew, igr, igr_ns = [float(v) for v in g["weights3"]]
    else:
        g0, net, r, (ns, ni, steps) = _setup(mode, "c64_64_4")
        g = _train_golden(g0)
        g["cos_anneal_ratio"], g["flip_saturation"] = g0["cos_anneal_ratio"], g0["flip_saturation"]
        ew, igr, igr_ns = 1.0, float(g["igr_weight"]), None
    car, fs = float(g["cos_anneal_ratio"]), float(g["flip_saturation"])
    z = t(g["z_vals"])
    fwd = _render_core_on_z(net, r, g, z, car, fs)
    a = [t(g[k]).to(DEV) for k in ("rays_o", "rays_d", "near", "far", "depth_scale")]
    call = r._prepare(a[0], a[1], a[2], a[3], a[4], car, 0, None, fs, None)
    N = z.shape[0]
    sd = ((a[3] - a[2]) / ns).mean().reshape(1).contiguous()
    v = {"z_vals": z.to(DEV).contiguous(), "udf": fwd["udf"].contiguous(), "gradients": fwd["gradients"].contiguous(),
         "scalars": fwd["scalars"], "_ws": sd}
    d_edge = 2.0 * (fwd["edge"] - t(g["true_edge"]).to(DEV)) / N * ew
    d_ns = None if igr_ns is None else torch.tensor([igr_ns], device=DEV)
    flat = torch.full((r._layout().numel,), float("nan"), device=DEV)
    for st in stages:
        r.backward_into(call, v, d_edge, None, torch.tensor([igr], device=DEV), d_ns, flat=flat, stages=st)
    d = _digest(flat)
    r.check_errors()
    assert bool(torch.isfinite(flat).all())
    return d


RAGGED = 4099                  # 129 tiles, the last one with 3 points
CHUNKED = 600 * 32 + 5         # 601 tiles in the preferred workspace of 300 (its fixed part grows by 4 bytes per tile: 299 fit): chunk_tiles < tiles, three chunks
UDF_CASES = {f"{n}/{p}/P{RAGGED}": (n, p, RAGGED, {}) for n in ("d8w256L10", "d4w128L10") for p in ("f16x3", "f16x3e", "bf16x3", "bf16")}
UDF_CASES.update({
    "d8w256L10/f16x3/chunked": ("d8w256L10", "f16x3", CHUNKED, dict(ws_points=300 * 32)),
    "d8w256L10/f16x3e/chunked": ("d8w256L10", "f16x3e", CHUNKED, dict(ws_points=300 * 32)),
    "d8w256L10/f16x3/accumulate": ("d8w256L10", "f16x3", RAGGED, dict(accumulate=1)),
    "d8w256L10/f16x3/no_weight_norm": ("d8w256L10", "f16x3", RAGGED, dict(weight_norm=0)),
})
RENDER_CASES = {f"{m}/{'+'.join(map(str, st))}": (m, st) for m in ("default", "plain", "normcos") for st in ((3,), (1, 2))}

# recorded on an MI355X from the library as it stood before the backward's host path was consolidated
DIGESTS = {
    "d8w256L10/f16x3/P4099": "899bb73c2cf4c48700f4693ea1e58a5545d297fe5b27bbe09d836318a9222489",
    "d8w256L10/f16x3e/P4099": "d6c8763b137675edf3749def4b2799ee2e7267ff1908ef55a176b87a5550acf7",
    "d8w256L10/bf16x3/P4099": "68b02fc1db5d53f824c3b7520455a7d7fd79c64c5ef937433622cb98bc75335c",
    "d8w256L10/bf16/P4099": "a711a3131976687746884ee15f2459416c8e82165017544646a800d71d9128f1",
    "d4w128L10/f16x3/P4099": "881a03efccd5ebcca1d9bd5e9a7ec5b975fed23e7b7539221326c8d4d4baeed4",
    "d4w128L10/f16x3e/P4099": "dfe383b68064440f0d858bc6b1b42cd90fb9bad99085328ab6615f5d61daf2ed",
    "d4w128L10/bf16x3/P4099": "9953298e4ba74971fbaf244e55290f95a2fe3567acf90a3731634c3ea12779a0",
    "d4w128L10/bf16/P4099": "207f444cf86666d2ee6cb2fb0f52c672ce8130e1aa89ccdc2d4193cf967a3962",
    "d8w256L10/f16x3/chunked": "9061614d6bbd8ca3d96880fca86dd8948b269ebaacf2783463792845fad24a1c",
    "d8w256L10/f16x3e/chunked": "e2f5d3f5ac2446900665fbc03088a2950664b2a74e60673229459927b8c03851",
    "d8w256L10/f16x3/accumulate": "b84d017bf07a8a890ee483a649e0ed0c424d301dbdd990bbc82e0eceac4202f8",
    "d8w256L10/f16x3/no_weight_norm": "f38c4eb34b5c367f73ced5bdfea6a7cc4d0c92b30adce66722ec3235635d202c",
    "default/3": "6ab1227dafca4dc2ed5db2c0ef8c6e0cf47a318bd4412917562a9aaf08203e42",
    "default/1+2": "6ab1227dafca4dc2ed5db2c0ef8c6e0cf47a318bd4412917562a9aaf08203e42",
    "plain/3": "37b854618353005936cfe1554dbc5f5e9970338f6f649f0cf4955c3ff5d6d68e",
    "plain/1+2": "37b854618353005936cfe1554dbc5f5e9970338f6f649f0cf4955c3ff5d6d68e",
    "normcos/3": "c99661ed674d7afb10d2f9c82a062ad25e92f2c53dd1339239f4dcd12feedf1d",
    "normcos/1+2": "c99661ed674d7afb10d2f9c82a062ad25e92f2c53dd1339239f4dcd12feedf1d",
}


def compute(case):
    if case in UDF_CASES:
        n, p, P, kw = UDF_CASES[case]
        return udf_vjp_digest(n, p, P, **kw)
    return render_bwd_digest(*RENDER_CASES[case])


@pytest.mark.parametrize("case", list(UDF_CASES) + list(RENDER_CASES))
def test_backward_digest(case):
    assert compute(case) == DIGESTS[case]
