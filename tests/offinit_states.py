"""Weight-normed network states AWAY from the initialisation statistics (plain module: numpy + torch CPU, no GPU import).

Every state the suite evaluates otherwise has g > 0 and g / ||v|| in [0.04, 1.06] (synthetic.make_udf_state: g = ||v|| perturbed by 2 %; the
reference-initialised goldens alike).  Weight-norm training moves g and ||v|| apart by orders of magnitude and g changes sign; the seeded
(numpy PCG64) transformations below produce such states from a `net_state` dict.  Each returns (new state, what it did per row): a list
with one int64 tensor [out_dim] per layer -

  scale_v          the exponent k of the 2^k its `original1` row was multiplied by.  W = g v / ||v|| is unchanged EXACTLY
  flip_and_zero_g  the factor on g: -1 (one row in eight of every layer with >= 8 rows; the single row of the last layer with
                   flip_last=True), 0 (row ZERO_ROW of layer ZERO_LAYER) or +1.  W rows are negated / zeroed exactly, so every quantised
                   form of W is exactly the negation / zero: the precision is that of the base state
  spread_g         the exponent e in {-1, 0, 1} of the 2^e on g
  zero_last_g      the factor on g: 0 for the last layer, 1 elsewhere.  The field is the constant |b_last|; only dg_last and db_last are non-zero

off_init = scale_v o flip_and_zero_g o spread_g returns a dict of the three lists.  Inputs are not modified.

The seeds are fixed.  spread_g's compounds over the layers (a factor of up to 2 per layer); its seed was picked from twenty on the CPU oracle in
fp64, looking only at the field on the tests' 777 points, so that both test networks stay a usable field: udf in [0.003, 4.5], |grad_x udf|
<= 310, g / ||v|| of off_init from 0 to 5e2, every autograd gradient finite (tests/test_vjp_math.py checks the last two).
"""
import numpy as np
import torch

ZERO_LAYER, ZERO_ROW = 2, 5


def _g(l):
    return f"lin{l}.parametrizations.weight.original0"


def _v(l):
    return f"lin{l}.parametrizations.weight.original1"


def n_lin(state):
    return sum(1 for k in state if k.endswith(".bias"))


def _copy(state):
    return {k: t.clone() for k, t in state.items()}


def scale_v(state, kmin=-8, kmax=8, seed=101):
    rng = np.random.Generator(np.random.PCG64(seed))
    out, ks = _copy(state), []
    for l in range(n_lin(state)):
        v = out[_v(l)]
        k = torch.from_numpy(rng.integers(kmin, kmax + 1, size=v.shape[0]))
        out[_v(l)] = torch.ldexp(v, k.to(torch.int32).view(-1, 1))         # a power of two: exact in every float format
        ks.append(k)
    return out, ks


def flip_and_zero_g(state, flip_last=False, seed=102):
    rng = np.random.Generator(np.random.PCG64(seed))
    out, fs = _copy(state), []
    n = n_lin(state)
    for l in range(n):
        g = out[_g(l)]
        rows = g.shape[0]
        f = torch.ones(rows, dtype=torch.int64)
        if rows >= 8:
            f[torch.from_numpy(rng.permutation(rows)[:rows // 8])] = -1
        if l == n - 1 and flip_last:
            f[:] = -1
        if l == ZERO_LAYER:
            f[ZERO_ROW] = 0
        out[_g(l)] = g * f.to(g.dtype).view(-1, 1)
        out[_g(l)][f == 0] = 0.0            # +0, whatever the sign of g was
        fs.append(f)
    return out, fs


def spread_g(state, seed=107):
    rng = np.random.Generator(np.random.PCG64(seed))
    out, es = _copy(state), []
    for l in range(n_lin(state)):
        g = out[_g(l)]
        e = torch.from_numpy(rng.integers(-1, 2, size=g.shape[0]))
        out[_g(l)] = torch.ldexp(g, e.to(torch.int32).view(-1, 1))
        es.append(e)
    return out, es


def zero_last_g(state):
    out, fs = _copy(state), []
    n = n_lin(state)
    for l in range(n):
        f = torch.ones(out[_g(l)].shape[0], dtype=torch.int64)
        if l == n - 1:
            f[:] = 0
            out[_g(l)] = torch.zeros_like(out[_g(l)])
        fs.append(f)
    return out, fs


def off_init(state):
    s, e = spread_g(state)
    s, f = flip_and_zero_g(s)
    s, k = scale_v(s)
    return s, {"scale_v": k, "flip_and_zero_g": f, "spread_g": e}


STATES = {"scale_v": scale_v, "flip_and_zero_g": flip_and_zero_g, "spread_g": spread_g, "zero_last_g": zero_last_g, "off_init": off_init,
          "flip_last_g": lambda state: flip_and_zero_g(state, flip_last=True)}


GATED = ("base", "flip_and_zero_g", "spread_g", "off_init", "flip_last_g")     # the states whose field is compared with a reference
KINK_BAND = 1.5e-2            # the widest value gate of the forward (single-pass bf16, tests/test_gpu_parity.py)


def vjp_inputs(cfg, base, n=777, seed=11):
    """(x, du, dg) for the parameter-gradient tests: du, dg are those of tests/test_gpu_backward.py::test_udf_vjp_vs_mirror (seed 11, 1e-3 / 1e-4,
    the zeroed entries); x is uniform in [-1, 1]^3 like there, but CLEAR OF THE KINK of udf = |h|: grad_x udf = sign(h) grad_x h jumps at
    h = 0, so at a point whose |h| is below a mode's value error a correct kernel may return the other sign, and no gate on grad_x or on the
    parameter gradients can hold there.  2n candidates are drawn; the first n are taken at which every GATED state's fp64 oracle udf is
    at least KINK_BAND x that field's maximum over the candidates - a kernel that meets its value gate cannot flip such a point.
    About 10 % of the candidates go (d4w128L10; none on d8w256L10).  Decided by the CPU oracle alone."""
    from oracle import emap_oracle as O
    gen = torch.Generator().manual_seed(seed)
    torch.rand(n, 3, generator=gen)                       # the suite's x draw: du, dg below are the suite's
    du = torch.randn(n, generator=gen) * 1e-3
    dg = torch.randn(n, 3, generator=gen) * 1e-4
    du[::7] = 0
    dg[::5] = 0
    cand = torch.rand(2 * n, 3, generator=gen) * 2 - 1
    keep = torch.ones(2 * n, dtype=torch.bool)
    for family in GATED:
        st = base if family == "base" else STATES[family](base)[0]
        u = O.udf_value_and_grad({k: v.double() for k, v in st.items()}, cfg, cand.double())[0][:, 0]
        keep &= u >= KINK_BAND * float(u.max())
    assert int(keep.sum()) >= n, int(keep.sum())
    return cand[keep][:n].contiguous(), du, dg


def ratio_range(state):
    """(min, max) of |g| / ||v|| over all rows, and whether any g is negative"""
    r = torch.cat([(state[_g(l)].double().abs().reshape(-1) / torch.linalg.norm(state[_v(l)].double(), dim=1)) for l in range(n_lin(state))])
    neg = any(bool((state[_g(l)] < 0).any()) for l in range(n_lin(state)))
    return float(r.min()), float(r.max()), neg
