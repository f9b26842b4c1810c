"""tests/ray_draw_ref.py, the numpy definition of the sampler's random draw (include/emap_hip.h), on the CPU: the published
Philox4x32-10 vectors, the epoch keys, rand_below's range, the batch split, and - for every case tests/test_gpu_ray_draw.py compares
on the device - that no class decision of a weighted ray sits within rounding of its threshold."""
import numpy as np
import pytest

from ray_draw_ref import MARGIN_MIN, draw, philox4x32_10, rand_below
import test_gpu_ray_draw as G


# the three known-answer vectors of Philox4x32-10 (Random123 kat_vectors): counter words 0..3 = index lo, hi, stream lo, hi; key = seed lo, hi
KAT = [
    (0, 0, 0, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    (0x299F31D0A4093822, 0x0370734413198A2E, 0x85A308D3243F6A88, (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("seed,stream,index,words", KAT)
def test_philox_known_answers(seed, stream, index, words):
    w = philox4x32_10(seed, stream, [index])
    assert all(x.dtype == np.uint32 and x.shape == (1,) for x in w)
    assert tuple(int(x[0]) for x in w) == words
    # inside an array of indices, next to other ones, the same words
    idx = np.array([index ^ 1, index, (index + 1) % 2 ** 64], dtype=np.uint64)
    assert tuple(int(x[1]) for x in philox4x32_10(seed, stream, idx)) == words


# (w0 << 32) | w1 of the epoch-order stream, recorded from the numpy body philox_keys of test_gpu_trainer_checkpoint.py had before it moved
# onto philox4x32_10: all four keys of (seed 17, stream 2^63 | 3), and of (2024, 2^63 | 255, 64 keys) the first and last three and the sum
KEYS_17 = [0xA42BA19F2617DA15, 0xFFE8F1408F31C093, 0x9A8B331256F6CA85, 0x4D51EA951353D3DB]
KEYS_2024_HEAD = [0x5BA8E4ECD571DD71, 0x83A29C7E35C79C1E, 0x93BCA21D70357B8E]
KEYS_2024_TAIL = [0x59905FA19BA4BF9C, 0xAA36C5D5A7E341D7, 0x3E0C6789491F4CF6]
KEYS_2024_SHA256 = "239a880edce703ffa24892ef90e6bcecef3a23544a7b963d71a2d7fe9734d5f6"     # of the 64 keys as little-endian uint64


def test_epoch_keys_are_what_they_were():
    import hashlib
    from test_gpu_trainer_checkpoint import philox_keys
    a = philox_keys(17, (1 << 63) | 3, 4)
    assert a.dtype == np.uint64 and [int(x) for x in a] == KEYS_17
    b = philox_keys(2024, (1 << 63) | 255, 64)
    assert b.dtype == np.uint64 and b.shape == (64,)
    assert [int(x) for x in b[:3]] == KEYS_2024_HEAD and [int(x) for x in b[-3:]] == KEYS_2024_TAIL
    assert hashlib.sha256(b.astype("<u8").tobytes()).hexdigest() == KEYS_2024_SHA256


@pytest.mark.parametrize("n", [2, 3, 30, 4099])
def test_rand_below_range(n):
    assert int(rand_below(np.uint32(0), n)) == 0
    assert int(rand_below(np.uint32(2 ** 32 - 1), n)) == n - 1
    r = np.concatenate([np.arange(0, 2 ** 32, 65521, dtype=np.uint64), (np.arange(1, n + 1, dtype=np.uint64) << np.uint64(32)) // np.uint64(n),
                        (np.arange(1, n + 1, dtype=np.uint64) << np.uint64(32)) // np.uint64(n) - np.uint64(1)])
    r = r[r < 2 ** 32].astype(np.uint32)                              # a coarse sweep and both sides of every step of the result
    v = rand_below(r, n)
    assert v.dtype == np.int64 and int(v.min()) == 0 and int(v.max()) == n - 1
    assert [int(x) for x in v] == [(int(x) * n) >> 32 for x in r]


def _scalar_weighted_pixel(seed, step, i, W, H, ne, density, order):
    """one weighted ray with python integers and floats, from the header's words"""
    w0, w1 = (int(w[0]) for w in philox4x32_10(seed, step, [i])[:2])
    nn = H * W - ne
    d = float(np.float32(density))
    we, wn = ne * (1.0 - d), nn * d
    u = ((w0 + 0.5) / 4294967296.0) * (we + wn)
    pix = int(order[(w1 * ne) >> 32]) if (u < we and ne > 0) or nn == 0 else int(order[ne + ((w1 * nn) >> 32)])
    return pix % W, pix // W


@pytest.mark.parametrize("batch,uniform", [(1, 0), (5, 2), (64, 32), (65, 32)])
def test_batch_split(batch, uniform):
    """With importance rays i < batch // 2 are uniform and the others weighted: batch 1 has no uniform ray, batch 5 has two."""
    s = G.sampler("A", device="cpu")
    ne, d, order = int(s._n_edge[1]), float(s._density[1]), s._order[1].numpy()
    pix, t_rand, margin = draw(5, 7, batch, s.W, s.H, 1, ne, d, order)
    plain, t_plain, m_plain = draw(5, 7, batch, s.W, s.H, 0)
    assert pix.shape == (batch, 2) and pix.dtype == np.int64 and t_rand.dtype == np.float32 and margin.dtype == np.float64
    assert int(np.isinf(margin).sum()) == uniform and bool(np.isinf(margin[:uniform]).all()) and bool(np.isinf(m_plain).all())
    assert np.array_equal(pix[:uniform], plain[:uniform]) and np.array_equal(t_rand, t_plain)
    assert 0 <= plain[:, 0].min() and plain[:, 0].max() < s.W and 0 <= plain[:, 1].min() and plain[:, 1].max() < s.H
    for i in range(uniform, batch):
        assert tuple(pix[i]) == _scalar_weighted_pixel(5, 7, i, s.W, s.H, ne, d, order), i
    assert float(t_rand.min()) >= -0.5 and float(t_rand.max()) < 0.5
    w2 = philox4x32_10(5, 7, np.arange(batch, dtype=np.uint64))[2]
    assert [float(x) for x in t_rand] == [(int(w) >> 8) / 16777216.0 - 0.5 for w in w2]


def test_the_vector_of_key_0_counter_0_reaches_ray_0():
    _, t_rand, _ = draw(0, 0, 1, 30, 20, 0)
    assert float(t_rand[0]) == float(0xBC57AC4C >> 8) * 2.0 ** -24 - 0.5
    pix, _, _ = draw(0, 0, 1, 30, 20, 0)
    assert tuple(pix[0]) == ((0x6627E8D5 * 30) >> 32, (0xE169C58D * 20) >> 32)


def test_no_gpu_case_decides_within_rounding_of_its_threshold():
    """The kernel may fuse nn * d into we + wn, which moves u by at most 2^-51 relative: a class decision is common to every correct
    build when |u - we| / (we + wn) > 2^-40.  Holds for every case of the GPU tests, so none of them ever leaves a ray out."""
    samplers = {name: G.sampler(name, device="cpu") for name in "ABC"}
    smallest = np.inf
    assert {c[0] for c in G.CASES} == set("ABC")
    for name, img, seed, step, batch, importance in G.CASES:
        margin = G.expect(samplers[name], img, seed, step, batch, importance)[2]
        assert margin.shape == (batch,) and float(margin.min()) > MARGIN_MIN, (name, img, seed, step, batch, importance, float(margin.min()))
        smallest = min(smallest, float(margin.min()))
    print(f"smallest margin over the {len(G.CASES)} GPU cases: {smallest:.3e}")
    assert np.isfinite(smallest)                                      # weighted rays whose class depends on u are among the cases
    # the scene of the GPU tests at 4096 rays, for the record: about 1e-4, eight orders of magnitude above the bound
    m = G.expect(samplers["A"], 0, 5, 7, 4096, 1)[2]
    assert 2.0 ** -40 < float(m.min()) < 1e-2
