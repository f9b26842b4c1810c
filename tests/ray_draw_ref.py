"""The random draw of emap_sample_rays, as include/emap_hip.h defines it (par. "on-device ray / pixel sampler": the stream, key and index
of the Philox draw, and the formulas that turn its four words into a pixel and a jitter), in numpy.  Integer-exact: the tests that
hold the kernel to it (tests/test_gpu_ray_draw.py) compare with equality.  A plain module: not collected, imports without a GPU.

The one floating-point decision is the class of a weighted ray, `u < we`.  The kernel forms we + wn = ne (1 - d) + nn d in fp64 where
the compiler may fuse the last product into the sum, which moves u by at most 2^-51 relative; `draw` therefore also returns how far
each decision is from its threshold (`margin`), and tests/test_ray_draw_cpu.py asserts margin > MARGIN_MIN for every case the GPU
tests use."""
import numpy as np

MARGIN_MIN = 2.0 ** -40

_U = np.uint64
_LO, _32 = _U(0xFFFFFFFF), _U(32)


def philox4x32_10(seed, stream, index):
    """-> the four uint32 word arrays of Philox4x32-10 for an array of 64-bit indices: counter [index lo, index hi, stream lo, stream hi],
    key [seed lo, seed hi], multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds."""
    seed, stream = int(seed), int(stream)
    assert 0 <= seed < 1 << 64 and 0 <= stream < 1 << 64
    index = np.atleast_1d(np.asarray(index, dtype=_U))
    c = [index & _LO, index >> _32, np.full(index.shape, stream & 0xFFFFFFFF, _U), np.full(index.shape, stream >> 32, _U)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = _U(0xD2511F53) * c[0], _U(0xCD9E8D57) * c[2]           # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> _32) ^ c[1] ^ _U(k0), p1 & _LO, (p0 >> _32) ^ c[3] ^ _U(k1), p0 & _LO]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(w.astype(np.uint32) for w in c)


def rand_below(r, n):
    """(uint64(r) * n) >> 32: an integer in [0, n) from 32 random bits"""
    assert 0 <= int(n) < 1 << 31
    return ((np.asarray(r).astype(_U) * _U(int(n))) >> _32).astype(np.int64)


def draw(seed, step, batch, W, H, importance, n_edge=None, density=None, order=None):
    """The draw of one launch: -> pixels (batch, 2) int64 x,y; t_rand (batch,) float32; margin (batch,) float64.
    n_edge, density, order: the image's entries of what the sampler uploaded (needed with importance only).
    margin = |u - we| / (we + wn) of a weighted ray whose class depends on u, inf everywhere else."""
    w0, w1, w2, _ = philox4x32_10(seed, step, np.arange(batch, dtype=_U))
    px, py = rand_below(w0, W), rand_below(w1, H)
    margin = np.full(batch, np.inf)
    if importance:
        half = batch // 2
        ne = int(n_edge)
        nn = H * W - ne
        d = np.float64(np.float32(density))
        we, wn = np.float64(ne) * (1.0 - d), np.float64(nn) * d
        u = ((w0.astype(np.float64) + 0.5) * 2.0 ** -32) * (we + wn)
        edge = ((u < we) & (ne > 0)) | (nn == 0)
        member = np.where(edge, rand_below(w1, ne), ne + rand_below(w1, nn))
        pix = np.asarray(order, dtype=np.int64).reshape(-1)[member]
        weighted = np.arange(batch) >= half
        px, py = np.where(weighted, pix % W, px), np.where(weighted, pix // W, py)
        if ne > 0 and nn > 0:
            margin = np.where(weighted, np.abs(u - we) / (we + wn), np.inf)
    t_rand = (w2 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24) - np.float32(0.5)
    return np.stack([px, py], -1).astype(np.int64), t_rand, margin
