"""The rays of tests/test_gpu_composite_digests.py reach both sides of every clip and mask of render_core's tail, so a forward and an adjoint
that decided one of them differently could not produce the recorded digests.  Checked on the forward recomputation of
oracle/vjp_mirror.py:composite_bwd (its lines before "---- backward ----"), evaluated here in float64 for every case's rays."""
import numpy as np
import pytest

from test_gpu_composite_digests import BETA_MIN, NEAR_SURFACE, PSETS, SAMPLES, make_rays


def scalars(pset):
    q = PSETS[pset]
    if q["dev"] is None:
        return q["inv_s"], q["beta"], q["gamma"]
    v, b, g = (np.exp(10.0 * x) for x in q["dev"])
    return float(np.clip(v, 1e-6, 1e6)), float(np.clip(np.clip(b, 0.0, 1.0 / BETA_MIN), 1e-6, 1e6)), float(np.clip(g, 1e-6, 1e6))


@pytest.mark.parametrize("pset", list(PSETS))
@pytest.mark.parametrize("S", [S for S in SAMPLES if S >= 63])      # one sample per ray (S = 1) has one side of everything
def test_rays_reach_both_sides_of_every_branch(S, pset):
    r = {k: v.astype(np.float64) for k, v in make_rays(S).items()}
    _, beta, gamma = scalars(pset)
    fs = PSETS[pset]["flip_saturation"]
    z, udf, g, d = r["z"], r["udf"], r["grad"], r["rays_d"]
    dists = np.concatenate([z[:, 1:] - z[:, :-1], np.full((z.shape[0], 1), r["sample_dist"][0])], -1)
    mid = z + dists * 0.5
    pn = np.linalg.norm(r["rays_o"][:, None, :] + d[:, None, :] * mid[..., None], axis=-1)
    gm = np.linalg.norm(g, axis=-1)
    E = np.exp(-beta * udf)
    raw = beta * E / (1 + E) ** 2
    eq = np.exp(-np.maximum(raw, 0.0) * gamma * dists)
    assert (gm == 0).any() and (gm > 0).any()
    for tc in ((d[:, None, :] * g).sum(-1), (d[:, None, :] * g / (gm[..., None] + 1e-5)).sum(-1)):      # default, normalised cosine
        assert (tc > 0).any() and (tc < 0).any() and (tc == 0).any()
        nxt = tc[:, 1:]
        assert ((nxt > 0.0) & (nxt < 0.01)).any() and ((nxt > 0.01) & (nxt < 0.02)).any()
        vm = np.concatenate([(nxt < 0.01).astype(np.float64), np.ones((z.shape[0], 1))], -1)
        a_in = 1.0 - (1.0 - eq) + fs * vm
        assert (a_in <= 0).any() and (a_in >= 1).any() and ((a_in > 0) & (a_in < 1)).any()
        if fs > 0:
            assert (a_in > 1).any()
        vp_raw = np.cumprod(np.concatenate([np.ones((z.shape[0], 1)), np.clip(a_in, 0, 1) + 1e-7], -1), -1)[:, :-1]
        assert (vp_raw > 1).any() and (vp_raw < 1).any()
    assert (udf < NEAR_SURFACE).any() and (udf > NEAR_SURFACE).any()
    assert (pn < 2.0).any() and ((pn > 2.0) & (pn < 2.4)).any() and (pn > 2.4).any()
    # fp32 exp underflows below -104: udf2logistic = 0 (the adjoint's raw > 0 test) on one side, > 0 on the other
    assert (beta * udf > 110).any() and (beta * udf < 80).any()
