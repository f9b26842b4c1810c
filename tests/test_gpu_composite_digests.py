"""Compositing and its adjoint bit for bit: sha256 of everything emap_composite_fwd_p and emap_composite_bwd write, at every lane chunking.

composite_kernel and composite_bwd_kernel run ONE ray forward (composite_dev.inc:composite_forward); before that the adjoint carried a
second copy of it, and a slip in either copy would have stayed inside every tolerance of the parity tests.  Each case here calls the two
entry points through the C ABI on seeded synthetic rays and compares the digests of their outputs with the digests recorded on an MI355X
from the library as it stood before the two copies were merged: that library was built into a tree of its own, loaded through
EMAP_HIP_LIB, and this module's __main__ printed the table below.

N = 37 rays; S on both sides of every boundary of the launchers' with_chunk (C = 1, 2, 4, 8, 16 samples per lane) with ragged last
lanes; the three render modes; two parameter sets (PSETS).  The rays come from numpy's PCG64, so they do not depend on the torch version,
and a few samples are placed by hand so that every clip and mask of the forward has samples on both sides
(tests/test_composite_digests_cpu.py asserts that on the CPU: the digests cannot go blind)."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from emap_amd import _lib

pytestmark = pytest.mark.gpu

N = 37
SAMPLES = (1, 63, 64, 65, 128, 129, 200, 256, 257, 512, 513, 700, 1024)
MODES = (_lib.RENDER_UNBIASED, _lib.RENDER_UNBIASED_NORMCOS, _lib.RENDER_PLAIN)
NEAR_SURFACE, SPARSE_SCALE, BETA_MIN = 0.05, 10.0, 5e-5
# 1: no cosine annealing, inv_s / beta / gamma by value.  2: annealed cosine, no flip saturation, a background, and the three scalars from
# device parameters p: x = exp(10 p) (variance 0.3, beta 0.5, gamma 0.3)
PSETS = {
    1: dict(inv_s=64.0, beta=128.0, gamma=80.0, cos_anneal_ratio=1.0, has_cos_anneal=0, flip_saturation=0.9, background=0.0,
            has_background=0, dev=None),
    2: dict(inv_s=64.0, beta=128.0, gamma=80.0, cos_anneal_ratio=0.4, has_cos_anneal=1, flip_saturation=0.0, background=0.25,
            has_background=1, dev=(0.3, 0.5, 0.3)),
}
CASES = {f"S{S}/m{m}/p{p}": (S, m, p) for S in SAMPLES for m in MODES for p in PSETS}


def make_rays(S):
    """Seeded rays of S samples as float32 numpy arrays.  Random: origins within ~0.5 of the centre, unit directions, sorted z in
    [0.5, 3.2], udf in (0, 0.2), gradients of length 0.8 ... 1.2.  Placed by hand (S >= 63):
      ray 0: z[1] = z[0], so dists[0] = 0, the first visibility factor is 1 + 1e-7 and the visibility product exceeds 1;
      ray 1: sample k = S // 2 opaque (udf 1e-5 and a gap of 2 behind it: exp(-relu(raw) gamma dists) = 0) before a sample whose
             true_cos is 0.5, so the visibility factor is 0 before its clip;
      ray 2: gradients 0 exactly at samples 0, S // 3 and S - 1;
      rays 3, 4: cosines 0.005 and 0.015 between direction and gradient at samples 1 ... 8 (either side of the visibility threshold 0.01);
      ray 5: udf = 2 at sample S // 5 (exp(-beta udf) underflows: udf2logistic = 0)."""
    rng = np.random.Generator(np.random.PCG64(7000 + S))
    f = np.float32
    ro = (rng.standard_normal((N, 3)) * 0.3).astype(f)
    rd = rng.standard_normal((N, 3))
    rd = (rd / np.linalg.norm(rd, axis=-1, keepdims=True)).astype(f)
    z = np.sort(rng.random((N, S)) * 2.7 + 0.5, axis=-1).astype(f)
    udf = (rng.random((N, S)) * 0.2 + 1e-3).astype(f)
    g = rng.standard_normal((N, S, 3))
    g = g / np.linalg.norm(g, axis=-1, keepdims=True) * (0.8 + 0.4 * rng.random((N, S, 1)))
    if S >= 63:
        k = S // 2
        z[0, 1] = z[0, 0]
        z[1, k + 1:] += f(2.0)
        udf[1, k] = 1e-5
        g[1, k + 1] = 0.5 * rd[1].astype(np.float64)
        g[2, [0, S // 3, S - 1]] = 0.0
        for ray, c in ((3, 0.005), (4, 0.015)):
            d = rd[ray].astype(np.float64)
            perp = np.cross(d, [1.0, 0.0, 0.0] if abs(d[0]) < 0.9 else [0.0, 1.0, 0.0])
            perp /= np.linalg.norm(perp)
            g[ray, 1:9] = (c * d + np.sqrt(1 - c * c) * perp) * np.linalg.norm(g[ray, 1:9], axis=-1, keepdims=True)
        udf[5, S // 5] = 2.0
    ds = (rng.random(N) * 0.5 + 0.5).astype(f)
    sd = np.array([2.7 / S], f)
    d_edge, d_depth = (rng.standard_normal(N) / N).astype(f), (rng.standard_normal(N) * 0.1 / N).astype(f)
    return dict(rays_o=ro, rays_d=rd, z=z, udf=udf, grad=g.astype(f), depth_scale=ds, sample_dist=sd, d_edge=d_edge, d_depth=d_depth)


def render_params(S, mode, pset, keep):
    """EmapRenderParams of a case; `keep` collects the device tensors it points to"""
    q = PSETS[pset]
    p = _lib.RenderParams()
    p.n_rays, p.n_samples, p.n_importance, p.up_sample_steps = N, S, 0, 0
    for k in ("inv_s", "beta", "gamma", "cos_anneal_ratio", "has_cos_anneal", "flip_saturation", "background", "has_background"):
        setattr(p, k, q[k])
    p.near_surface, p.sparse_scale, p.beta_min, p.render_mode = NEAR_SURFACE, SPARSE_SCALE, BETA_MIN, mode
    if q["dev"] is not None:
        dev = torch.tensor(q["dev"], dtype=torch.float32, device="cuda")
        keep.append(dev)
        p.variance_dev, p.beta_dev, p.gamma_dev = dev.data_ptr(), dev.data_ptr() + 4, dev.data_ptr() + 8
    return p


def _sha(tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for v in tensors:
        h.update(v.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def compute(case):
    """(forward digest, adjoint digest) of one case"""
    S, mode, pset = CASES[case]
    r = {k: torch.from_numpy(v).cuda() for k, v in make_rays(S).items()}
    keep = []
    p = render_params(S, mode, pset, keep)
    L = _lib.lib()
    inputs = [_lib.ptr(r[k]) for k in ("rays_o", "rays_d", "z", "udf", "grad", "depth_scale")]

    def nan(*shape):
        return torch.full(shape, float("nan"), device="cuda")
    out = {"weights": nan(N, S), "alpha": nan(N, S), "mid_z": nan(N, S), "dists": nan(N, S), "inside_sphere": nan(N, S),
           "gradient_mag": nan(N, S), "gradients_flip": nan(N, S, 3), "edge": nan(N), "depth": nan(N), "weight_sum": nan(N),
           "normals": nan(N, 3), "scalars": torch.zeros(16, device="cuda")}
    co = _lib.CompositeOut()
    for k, v in out.items():
        setattr(co, k, v.data_ptr())
    part8 = torch.zeros(N, 8, device="cuda")
    _lib.check(L.emap_composite_fwd_p(*inputs, N, S, _lib.ptr(r["sample_dist"]), C.byref(p), C.byref(co), _lib.ptr(part8), None,
                                      _lib.stream_ptr()), "composite_fwd_p")
    fwd = _sha(list(out.values()) + [part8[:, :5]])
    cg = _lib.CompositeGrads()
    d_ge, d_ns = torch.tensor([0.1], device="cuda"), torch.tensor([0.05], device="cuda")
    cg.d_edge, cg.d_depth, cg.d_gradient_error, cg.d_gradient_error_near_surface = [v.data_ptr() for v in (r["d_edge"], r["d_depth"], d_ge, d_ns)]
    cg.scalars = out["scalars"].data_ptr()
    d_par = nan(3)
    cg.d_variance, cg.d_beta, cg.d_gamma = d_par.data_ptr(), d_par.data_ptr() + 4, d_par.data_ptr() + 8
    cg.grad_scale, cg.accumulate = 1.0, 0
    d_udf, d_grad, part4 = nan(N, S), nan(N, S, 3), torch.zeros(N, 4, device="cuda")
    _lib.check(L.emap_composite_bwd(*inputs, N, S, _lib.ptr(r["sample_dist"]), C.byref(p), C.byref(cg), _lib.ptr(d_udf), _lib.ptr(d_grad),
                                    _lib.ptr(part4), _lib.stream_ptr()), "composite_bwd")
    return fwd, _sha([d_udf, d_grad, d_par, part4[:, :3]])


# case: (forward, adjoint), recorded on an MI355X from the library built at the commit before composite_forward (see the module docstring)
DIGESTS = {
    "S1/m0/p1": ('fa17a788cf959cf94fd577fbb4b262485d54c0aa72ef9f33d17b9a1e6629682c', '95584ec08b9bc7e45db021a728e0a7e5bf8311190785b00150c7b1cdc969619f'),
    "S1/m0/p2": ('ab704170a9fdf3fff694f00cd7137901ffb991184ceab4dfdd07d0832c242c7b', 'b326bc08b856515740c4cb2c83d16c77da28e161ce742e5aa17448938e015471'),
    "S1/m1/p1": ('22bde3f699c5960f8ffe3344ae6317c830b9b129a7cd344250085ef4dc934ff9', '45f782a7319ef3bd717363b6cf320f86f7f7f9213bcee610f08fb74ff9037434'),
    "S1/m1/p2": ('d5abab307e56679230ddbc5bc92cb833e69ead371a8b45f98ba6c76a68a8e59b', '4a2675c7bbfe8a66a894c209d41185f4b1d7bd769f33ac53a1b65b15193d638e'),
    "S1/m2/p1": ('f9312cf239fd0532add79f83008c4b5aefead61371b2369a97fe51222ce39974', '7bea133f39cdc9ad399387f2e1ca26b5a77cbf8f9945cf0c17f04ddcb53f4fb6'),
    "S1/m2/p2": ('fbf864d88e80bad2dca5d543545e30c5ba3b51b9cea72f706498f627ccc8d55c', 'd1adf059cc3122296dcb70cc55fdf640f1fcf4046b5c171bba38658ba44600c6'),
    "S63/m0/p1": ('0653877046341a9d401e7158b72fbfa9b05c041978ab209f08c8defdb49e9261', 'c045dd5f34734ccd9a7bdd7730b82c9397b060ce86f381706ce22da387c854f7'),
    "S63/m0/p2": ('20e22a76bfc4c2cb5db507e897109f2e5a272ff765bd77012f9adf4bf145a40d', '9446ba1093237bdd3c6ddd55c3eb27e07ee016cab156787cc08f62b243720ad5'),
    "S63/m1/p1": ('120844e00b2e0d1b24e7bb4082795b6ff1d28e10b0f0a4577aee2bd27b093050', '43dc320529708d0bcb9b7949b4c427b1fdc0aa59d70a33c06e7a104c1fc67695'),
    "S63/m1/p2": ('995670f69ee8ef8de840060b82430d9536806a8fcb33e65ff9c9b2bbf8b9afcd', '6f5f95860cda66db183cfe2c313056e43ebe918f6ef9826bcb7622c966c41788'),
    "S63/m2/p1": ('63389ee8edb329666bcb044646e0bf32c4347820ccb0e2b3bfca8ad505ab412b', 'f1cc857269d956f3ba7f119af47570a212c63d84f55283d381470d46d2fe35f6'),
    "S63/m2/p2": ('341d1f27d58c4d1ea1101c372ffa49f038a3dfe9a044a02ffd0f9321dc15e64a', '623ed1abca91b5e9fc023d232ee5d61dce72b07823c2b08167e65033acfc4065'),
    "S64/m0/p1": ('594a6920439dca7170a09f66c2ab810c6a89afcf06b1c28968a2ddde33100d61', 'bbc075394db2e897cc64fdfb8e14305c3dbb7294666fe6d94c2c09fb7cfdb030'),
    "S64/m0/p2": ('5cc58ff67aeb14101acefc4c101bc2a6a1754c5d051549a2e225cbac970b75ca', '7f655de2b9349eb39eb4dea8830bd6c9f7e69236b697c1b4eff62318a971e7a7'),
    "S64/m1/p1": ('aab608feac558e0ca7899a62a31e84ee72771373be05292c433d0846c6f0df0b', '2727156330515840e583f7ef4a1033a3965989b02e2274f5b394e2f449734319'),
    "S64/m1/p2": ('7919548a563fec6763ca2d05a5cdbce0d0e95ed895d1e69f421f62c0578b1710', '2f583622ce9af242f79f58f4af3ed8d3f16891ce13da1887f151b8f5eb5782d1'),
    "S64/m2/p1": ('2fc33ee0e7394302af8d6257a2b313336912b45c1c5f1cecc618d7bbe22c9ad8', '5abb096bd7c4f7ac83849481694a1efa9c72bf5f94b7cc05ab71659a4fa56dff'),
    "S64/m2/p2": ('8632ea00a7d6bed0aceddee2e0503923722b5dd5503ae4a995d4132bb763b116', '447b45253360ac5036b5c221157054a15da3178a0d5a7f616bbf8daa42ccc108'),
    "S65/m0/p1": ('5d5d281e0989010dfdbc085838e651308b012eab58481a6119903c3e1a19b822', '2b3a564415c2f9fbe6f6299b77a5e0444b48e96bd5dd1e46b377e8aaebc2c845'),
    "S65/m0/p2": ('03ef78c332d8f5adb8693fdd64fbc3a3e2b8a405d753d8f556c4afa7afc807a6', 'b4132c9587d52575725132d333d1f765e0b26fef0f7a87e51cb530dd146571df'),
    "S65/m1/p1": ('f618dae9aa793bbf1ee148583e902d1fbdcccddaaf92d23dc295a496e93ae2cf', 'e8576b75934ab3467c88f13c0d1971ba1f34e695987861bdaacbb51516555ce8'),
    "S65/m1/p2": ('8ae4470b3a68b84d12050c7bccea1e0a12bdbe1b5b4bbace9f3df047ae7f9874', '57d5cec69a89fa308dca740b9a85f3f66bf0fbcb9aa19622a4448c4c2e1e267c'),
    "S65/m2/p1": ('161f745447c10a0335d40a6010601653589d244e159639daf1698bb77db59dcb', '0c59d5c4bae7d4c26b7a8256f95150f86accdbea07297f52de7d2b218b6b852a'),
    "S65/m2/p2": ('2b1823934888a35060ab033af4c6f8063e117d97f8beef5bf979d998bf61f0fc', 'd9ade28bee89be92c8ab00d012761ad24d8c2a92059960009565a59e2d56a860'),
    "S128/m0/p1": ('4a82bfe9b19599a25fb616283e641417acdc1bab8ecfb21c60514ac43181fba6', '975323b6b1282894344bb7481efacd68ef399b3e3d9151f83b05dc03c8d7dee8'),
    "S128/m0/p2": ('79feed015a3ebbf3822c22d947842dabf330eaaab581acac05732a32c7538143', 'f440551c0a2cb4c27f709c1f3fb5222ae555675fec5e50f11fb541fca2f3f792'),
    "S128/m1/p1": ('4377bc7729aeffde13bfc74d36beac25627bfae1f970d37bf385613c21605322', 'a7981e97376fbe67ace0df298cd03ca73069c001947385f6b04bffcd961e92ed'),
    "S128/m1/p2": ('456f4f350dad7418d1348a261e1bbd4fd1b83b5bf5d9dff50821bdcaa92c20f7', '4707aea74863da3799c66d929000112bd566bdc32a9c232d36c0bc4dbe7173ee'),
    "S128/m2/p1": ('099db6459abe4e1702e3ebaf25218a674a0aa9f9a585b90538672de0a7abac32', '107f49492131e30177910b543cdc44c7b4b6b948d0eee71a333963eecf6f2e4e'),
    "S128/m2/p2": ('3a4a4eceb7b8060450da37595a16cc9b08d890f278c78f835a7e6c29b2895316', '4e92816da9ada48070a77041843a23b6c853a8e7cbc2c48bf2af4e3521697ebc'),
    "S129/m0/p1": ('57c9dd1c34abdc26f19e61b1d9497e7c00864f3204d4a8f49297feb869fa835d', 'ed39ffce6a2994a44044d4a6afd0d5ecd9ee3922857aa3386d731e93a93257e5'),
    "S129/m0/p2": ('59b7395a51cf9b3a698a0784b73dc26c00fd7bb2f175f1aaf26ee8ad343d2a76', 'b9034d433a915cd6b89e393033be9c08e04f51e602025d9ebd8f090b29c31c77'),
    "S129/m1/p1": ('32e08636d8b490a9138b9a466ae1e7ec6c1cd509862dbc8a5a51210daec0629a', '65d22c81669602f0e1c2bec916c9ec83a5bf1dbc3804e05874f948ad3302fcdb'),
    "S129/m1/p2": ('1ddddace0f97cdb31e5e8c63791c1488c6a499709fe7f76df5b04faafda5e00c', 'e0be1877e11953ec1b4886c6b23d6f6bf2b3c7838e5165da0c3e1a1e8bb175d1'),
    "S129/m2/p1": ('a4c0b4055f25953a38085b3a5ffe1a203ef1f07f9e9fa1c7aaa498d10632ab95', '4064c090a534f36aa1a09e679f848f32d02698f147e860b7d82724c3214e71ff'),
    "S129/m2/p2": ('10bec08dc77e8124f281fc6c8128541f6ea6fba6f38e00d3116e75a353a4a7aa', '47697aa3da7542698cd0fc6724b3bc302ad7edd8604cdbe877266f3739968d26'),
    "S200/m0/p1": ('9802b5263dc63113fea8b428d9f4de5b7d6133e6fc4a1a170774c29d372e0e5e', '3510b6dfb5457c21f502c8df3cdf939061095782f14fd3bd9e307f6ff4fccc1c'),
    "S200/m0/p2": ('55d1f96961392d74d73ad23adf402f0249ac68805f215263d90bd8819dc2c1f0', 'ef84f4362f202682fefdd1f7be22d2ffa386aeca9d72841e209f1d90b149500d'),
    "S200/m1/p1": ('8703b80c49486d4b4c0b01c231e5e4be13dfe6dbee64e9d2d113e91dcee62d76', 'e19e4f94cb270d367c3783498d8f3d16cbab7d83d90e259f9717bd3f3f366387'),
    "S200/m1/p2": ('dde0d8b7d396a4c795a80604ccc0f720af476f046cf18ce01be9893204edbab2', '510a193d63bcdb075bd1022f7b8e1a33a66b26613472d574336def4106e445c5'),
    "S200/m2/p1": ('cda588cd4cbe25b70d9f9a22394f66131bf70c1db8076eefd20132707fae2722', '64eaa85ffbccf1337420f3caded277882803f735bdac9bc5e829472192638934'),
    "S200/m2/p2": ('f962cef2e442c134055c9cd364123fd5e6ae279a158b8a9457753625e9ba2be2', '3df8b84293c54885dff0e91998799324ee78e6273084a0c50baf303c4e30253b'),
    "S256/m0/p1": ('46263dff48d5752e41d1c02b303f1ddec713c792c678a035404ee6f69a4f5401', '3b54039bc4bdb890e200416deb56fec657130fcf78e6139aaaae361183a8ae9c'),
    "S256/m0/p2": ('e82964de8d1b37862b9038099ff6a7476644b90aade023faca7e959d301326f6', '1385d6d87b4216127e114701f8fbb29bc25c749d094b9406a8ab5f8f6624daa9'),
    "S256/m1/p1": ('04bf7cf271cc442833fa0ff92f4c14bc1c77d03f0a52fc58189b0e84789f9e9a', '993e284836f714db17772178587be7b5ea56b1364444d023a23f12179fb3758d'),
    "S256/m1/p2": ('2ff1f63dd9d4972d9c830e267d1bb2eb9ba2711bca91fc9ac4b90acfe0b2081c', 'f2576799dc44c0e2d6e3d9a517d4ae2dea12c25e3627f2e3ade3a0213e7df317'),
    "S256/m2/p1": ('cd36ff1c1fe0c6f164c0bdb4dea8030ccc0a68f21d550333169dbe399ce963a5', '61ed5db695808ca6d5fc151ce1d297830d3e2a6102703bf3c16f5b3a54319d50'),
    "S256/m2/p2": ('e1deec6d20f4fc262a653798c9e104def05c14c34613cacc1679556ba8ffe2a4', '7381a817a2c7c4cbaede2d0866d5f3cb09428f486aa6bfa86be0dd9f8041112a'),
    "S257/m0/p1": ('88ab5691557d8a4007cc49304fa8e99f61892d38cbc8ac330221258dcb57c61d', '16a6d71a4c61493ed346c0cbf9e828f2896d16464d434bdf165ee33fd2caaf7f'),
    "S257/m0/p2": ('3e7b0b531c619d03d8051210f649f0680d4b51a1dcd6e7c8dee9a18f86cec359', 'e01dfe690f0bb70085b84dbc6180d7d298364742915681a5bcef6df5bb7bd9d0'),
    "S257/m1/p1": ('a52c128936952cd7619be944f3d9223816c6c3f9989c4ee93e2662bf0a23836c', '4cfab1a2c98ce24fdab2b99cbe35372f830c6931221ae5fe98a00d3561792d3e'),
    "S257/m1/p2": ('3ab87b57311963870ad8312705de0ba54cdefe33b3f1b84aa1ce9cc396aae815', '3fb4a0b53659974ec1f6362c683f770af0e24fe0dad27e1062f0f03b6358e323'),
    "S257/m2/p1": ('e5fd5371d3857c99462eac22f0e436777fa04299e29a5d80cff790af554ada27', 'a12b091db935e2755cd392137e586fc7fdcea0fd7a42c7960adf7151bace25d7'),
    "S257/m2/p2": ('93d7b790e407467c4c87f71e6192d534838a569b4fc708d15965f4d6c47d699a', '462508f6f400c908900b96aa2c28b90160a196ba711ccd90777463f8556e6d7f'),
    "S512/m0/p1": ('c59a7854d74c3ff7669796fe51a1277a97cb4d04da63bc43a428524edd3d8195', '3872f230473219f39e608184d861ce5b50af964c6e68252d25a41fda411f3777'),
    "S512/m0/p2": ('845c438c61542fbbed4c26f8a3f99ee5ec49539f23a12c08849e2c8189c10019', '42bdd907965679e0f9ff8ca69b03222c3f4ceb628782c4420fbeda5589623b82'),
    "S512/m1/p1": ('3a7ae25f6f6ffafcaf6de755c113a1f5bcf6084d0e634914f4dff065bf8768b4', 'f693a4447df1c857b33c2afe371a699bf5ddedcadf6c74c380d3499d8d2a82ce'),
    "S512/m1/p2": ('256cb161126a91371fab0d33c66c5e0a1880c7e64fd84227d47c30eb8bf898d6', 'b81c4d74bd8fe5e76b8af3cd02ee74659d53c8ccf2cd5e880ec831ec2178ac83'),
    "S512/m2/p1": ('408bb36efd50fd1541ea8c5f647872b7fd3271ca6af62f396b08a18f85f3032b', '6cfbeeebb11af2f7603f49741ea528a4c9af7653b51ca43ab41ebd41f84b061d'),
    "S512/m2/p2": ('67ecd82a981d50d97abb1f5a3fc8ee42f99d92deda04716c4568beea2dab622b', 'ed27e0a8d25c33f0fb15b0ca151372087e5b56f3d2208ce2a0c8dc188dd5b73c'),
    "S513/m0/p1": ('1ddfc2b0aeafcc2a640947a26204926fc19fd1168922641024d1d108f5f5b906', '7ab56b1710bec33e4d30e874a9b4c5887e3f0f3ddf5bc4fdaacd2bb87ca132bd'),
    "S513/m0/p2": ('827bc29ab4b083af62e63e66277fb6a5f0e3cc27965aed92df0b740a5e542ad5', '5afe4bdbb04883d1de3308aab8d8703041964d826aaa21778ac1e71244c3511d'),
    "S513/m1/p1": ('852161fa1c9a4b5c9b450486587729f81c879b8e4ef741550066ab8e4f2f54a7', 'd98b3344a58c6cc676b7540b20c6f1bc5936180fb5ff9ba535965086638d4e1a'),
    "S513/m1/p2": ('60e187de54625d4baf371ae6764ecf54da16ca36d360d7be26f5d885156943cc', '075cf10202e37c3d73711dcd9ded381f7c4b85f7c429614cc41dcfc902f1d01d'),
    "S513/m2/p1": ('1e7cd52a2b1cc6f697c280155e7d65a15422736229a84107e7e7e0e1a9d3e161', '8352f680e6c04da5f2028766afd8fa06899eefdb6b665ff9b7f02b2aec2629a1'),
    "S513/m2/p2": ('e3b2905176a648c9cd954cc18ec6fee4c70b3b75cd928d6ef63a36a38a3c338d', '442312be38e058e091e4b42217d36b645490ce810fac71ccb005294e0702a592'),
    "S700/m0/p1": ('8fa304bfaa2ad1a4797a276d11356fcff0b0d58137908e51cf7a9a4bd2ae9198', 'ef36ec458579baa0703d7472256f02bfd33bd50aed376e865fb2e179abef9313'),
    "S700/m0/p2": ('fc51055bd5f3f058d75ea8bb246376fe2d09278f1376aa3df6d1ce874fee08ce', '12f31c962cccb293bd219f617620993e6f3a8c68d8e23d35fe1c334350eb17de'),
    "S700/m1/p1": ('604b03667cd60ac54d1e7393bc61be1234a870c03e04ae02745284b37b5fa02a', '17df0dbe05882b0af5ab4c8437c6a80c3acc7d21dfa0842051cc4b3af99ba359'),
    "S700/m1/p2": ('a12ecf1ded05e0ce61e154a7c5ac05d0e3bf63563ad6ab0ba72c11f101ec527e', '49e9db62e3f17a6dbeaf2881b9334e08d8157f87d3ce5a7d24d68e00aba419bc'),
    "S700/m2/p1": ('7060879023a9a10ae3e4d27838be0bc45cd9bba6774531c394720e1a8568e708', '651abedf0612a04b59bafefd368dd43dc1af230ff84bd42f9b74e1d966896789'),
    "S700/m2/p2": ('a5ce98c9ebd432d4ee36101f23bdcf8be0dc7a83377c9f9b54e4fa5a09c013ad', '670ec9b6da9103840e9268686456bb5268240588b7cd87dc4ab1ede77a5becfc'),
    "S1024/m0/p1": ('f0d01dec87349fe0558bc2a4d99780a6476cf723ac3e2c9cd8a7c0cef74e4da1', '6b96a386ccff7f9824d0a30ee6d9fd12c01d23f34ccc61820bd5bb3e0291c306'),
    "S1024/m0/p2": ('7115e6ff6f97443ed9ceae37549f96f22c8c88a1a13194b515c75a47d4d3c443', 'c249494542c31785fd0a109167e27f6672c2fc3f001acd57963870196f28a7d6'),
    "S1024/m1/p1": ('941df8191206ee85bbd14f6278a170e081600f9528f3883a9f309c9dba2e07f7', '4ef7faa346e123301a6d6f5e321c7a7903089f6166ade57cb850cebd2b265a4e'),
    "S1024/m1/p2": ('c3816ed002d3d99c4d89ec397ff72c5472f36833761b1b8f47b942e1358e4773', 'c871f763685ffcd8db198a562af136a4ca8d038a11c181b7a9236efbe005201c'),
    "S1024/m2/p1": ('5a517fc63e2b34e6ad7ebfb726d59544418b3f418dae96933b9868bf04874abb', '265f6781f3a34491147c02e14d38de2ccf938d716ac21a69448e34e8c2e38982'),
    "S1024/m2/p2": ('026c994d5c3b47916b4e2f67897d559910fc110a54bbf677988d40e7fab4ee3c', '0e20085f4b37077a7fe2d7019544da17b7cdc5112f580ac0d73c29102b9d2869'),
}


@pytest.mark.parametrize("case", list(CASES))
def test_composite_digest(case):
    assert compute(case) == DIGESTS[case]


if __name__ == "__main__":
    print("DIGESTS = {")
    for c in CASES:
        print(f'    "{c}": {compute(c)!r},')
    print("}")
