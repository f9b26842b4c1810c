"""CPU yardstick of the DTU-evaluation tests (tests/test_dtu_eval_cpu.py, tests/test_gpu_dtu_eval.py) and the CPU baseline of
scripts/bench_dtu_eval.py: a numpy restatement, in scalar order, of the semantics include/emap_eval_hip.h fixes for emap_point_visibility,
and of the two sequences around it (scripts/get_gt_points_DTU.py:251-288, src/eval/eval_DTU.py:39-69 of the reference).  numpy's
elementwise multiply and add round once each and never fuse, so the expressions below are the kernel's operations one for one.  Nothing
here imports the package under test."""
import numpy as np


def cameras_ref(intrinsics_list, camtoworld_list):
    """K (F, 3, 3), R (F, 3, 3), T (F, 3): K = intrinsic[:3, :3], [R | T] = inv(camtoworld)[:3], fp64."""
    K = np.stack([np.asarray(k, dtype=np.float64)[:3, :3] for k in intrinsics_list])
    w2c = np.stack([np.linalg.inv(np.asarray(c, dtype=np.float64)) for c in camtoworld_list])
    return K, np.ascontiguousarray(w2c[:, :3, :3]), np.ascontiguousarray(w2c[:, :3, 3])


def project_ref(K, R, T, X):
    """One frame: (n, 3) points -> p0 / p2, p1 / p2, p2 (n) fp64, not rounded.  c = (R X) + T and p = K c, every 3-term sum left to right."""
    X = np.asarray(X).astype(np.float64)            # float32 widens exactly
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        c0 = ((R[0, 0] * x + R[0, 1] * y) + R[0, 2] * z) + T[0]
        c1 = ((R[1, 0] * x + R[1, 1] * y) + R[1, 2] * z) + T[1]
        c2 = ((R[2, 0] * x + R[2, 1] * y) + R[2, 2] * z) + T[2]
        p0 = (K[0, 0] * c0 + K[0, 1] * c1) + K[0, 2] * c2
        p1 = (K[1, 0] * c0 + K[1, 1] * c1) + K[1, 2] * c2
        p2 = (K[2, 0] * c0 + K[2, 1] * c1) + K[2, 2] * c2
        return p0 / p2, p1 / p2, p2


def strength_ref(maps, invert=False):
    """(F, h, w[, 1]) -> (F, h, w) fp64 edge strength: bytes g / 255.0, with invert 1.0 - g / 255.0; float maps widened as they are."""
    m = np.asarray(maps)
    m = m[..., 0] if m.ndim == 4 else m
    if m.dtype == np.uint8:
        s = m.astype(np.float64) / 255.0
        return 1.0 - s if invert else s
    return m.astype(np.float64)


def counts_ref(points, maps, intrinsics_list, camtoworld_list, h, w, threshold, invert=False):
    """int32 (n): the frames in which a point's rounded pixel (half to even) lies in the image - tested on the doubles: NaN and +-inf are
    outside, -0.0 is pixel 0 - and the strength there exceeds the threshold.  No depth test."""
    K, R, T = cameras_ref(intrinsics_list, camtoworld_list)
    S = strength_ref(maps, invert)
    n = len(points)
    count = np.zeros(n, dtype=np.int32)
    for f in range(len(S)):
        a, b, _ = project_ref(K[f], R[f], T[f], points)
        with np.errstate(all="ignore"):
            u, v = np.rint(a), np.rint(b)
            ok = (u >= 0) & (u < w) & (v >= 0) & (v < h)
        ui, vi = u[ok].astype(np.int64), v[ok].astype(np.int64)
        hit = np.zeros(n, dtype=bool)
        hit[ok] = S[f][vi, ui] > threshold
        count += hit
    return count


def margins_ref(points, intrinsics_list, camtoworld_list):
    """The conditions of exact agreement: (least distance of any finite p0 / p2, p1 / p2 from a rounding boundary x.5, least |p2|)."""
    K, R, T = cameras_ref(intrinsics_list, camtoworld_list)
    half, depth = np.inf, np.inf
    for f in range(len(K)):
        a, b, p2 = project_ref(K[f], R[f], T[f], points)
        for c in (a, b):
            c = c[np.isfinite(c)]
            if len(c):
                half = min(half, float(np.abs(c - np.floor(c) - 0.5).min()))
        depth = min(depth, float(np.abs(p2).min()))
    return half, depth


def affine_ref(p, m):
    """p @ m[:3, :3].T + m[:3, 3], every row sum left to right."""
    p, m = np.asarray(p, dtype=np.float64), np.asarray(m, dtype=np.float64)
    a = m[:3, :3].T
    return ((p[:, 0:1] * a[0] + p[:, 1:2] * a[1]) + p[:, 2:3] * a[2]) + m[:3, 3]


def voxel_average_ref(points, num_voxels_per_axis=256):
    """One point per occupied voxel of a grid over the points' own extent, the mean of the voxel's points, rows ordered by key:
    key = floor((p - min) / voxel_size), voxel_size = (max - min) / num_voxels_per_axis.  With a power of two per axis the voxel size is
    exact and the point ON the upper bound of an axis has key n there."""
    p = np.asarray(points, dtype=np.float64)
    if len(p) == 0:
        return p.reshape(0, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    vs = (hi - lo) / num_voxels_per_axis
    key = np.floor((p - lo) / np.where(vs > 0, vs, 1.0)).astype(np.int64)
    voxels = {}
    for k, row in zip(map(tuple, key), p):
        voxels.setdefault(k, []).append(row)
    return np.array([np.mean(voxels[k], axis=0) for k in sorted(voxels)]).reshape(-1, 3)


def visibility_frames_ref(ratio, num_frames):
    return max(1, round(ratio * num_frames))


def gt_edge_points_ref(gt_points, worldtogt, maps, intrinsics_list, camtoworld_list, h, w, threshold, ratio, num_voxels_per_axis=256, invert=False):
    """The per-scan sequence of the ground truth: to world coordinates, visible in more than max(1, round(ratio F)) frames, one point per
    voxel, back to the ground-truth frame."""
    worldtogt = np.asarray(worldtogt, dtype=np.float64)
    pts = affine_ref(gt_points, np.linalg.inv(worldtogt))
    keep = counts_ref(pts, maps, intrinsics_list, camtoworld_list, h, w, threshold, invert) > visibility_frames_ref(ratio, len(maps))
    return affine_ref(voxel_average_ref(pts[keep], num_voxels_per_axis), worldtogt)


def sort_rows(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])]


def look_at_views(n_frames, h, w, seed):
    """n_frames cameras on a ring around the unit cube, looking at a point near the origin, a different focal length per frame:
    -> intrinsics (F, 4, 4), camtoworld (F, 4, 4) (columns right, down, forward, position), byte maps (F, h, w)."""
    rng = np.random.default_rng(seed)
    intr, c2w = [], []
    for f in range(n_frames):
        ang = 2 * np.pi * f / n_frames + 0.3
        pos = np.array([3.2 * np.cos(ang), 3.2 * np.sin(ang), 1.1 + 0.4 * np.sin(3 * ang)])
        fwd = rng.uniform(-0.15, 0.15, 3) - pos
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, fwd, pos
        focal = (0.9 + 0.35 * (f % 7)) * w
        k = np.eye(4)
        k[0, 0], k[1, 1], k[0, 2], k[1, 2] = focal, focal * 1.03, w / 2 - 0.37, h / 2 + 0.21
        intr.append(k), c2w.append(m)
    maps = rng.integers(0, 256, (n_frames, h, w), dtype=np.uint8)
    return np.stack(intr), np.stack(c2w), maps


EXACT_FOCAL, EXACT_THRESHOLD = 4.0, 0.2


def exact_cases(h, w):
    """Hand-made points whose projection is exact in every order of operations: one camera with R = I, T = 0, focal length 4 and the
    principal point at pixel (0, 0), so u = 4 x / z and v = 4 y / z with z in {1, 2, 4} (and -2, 0).  The byte map is 255 everywhere but
    pixels (v, u) = (3, 5), (3, 6), (3, 7) = 51, 52, 50: with the threshold 0.2 and no inversion 51 / 255.0 IS the double 0.2, so pixel
    (3, 5) is exactly at the threshold.  -> intrinsics (1, 3, 3), camtoworld (1, 4, 4), maps (1, h, w) uint8, points (m, 3), expected (m)
    counts, names (m)."""
    assert h >= 8 and w >= 8
    intr = np.array([[[EXACT_FOCAL, 0, 0], [0, EXACT_FOCAL, 0], [0, 0, 1.0]]])
    c2w = np.eye(4)[None]
    maps = np.full((1, h, w), 255, dtype=np.uint8)
    maps[0, 3, 5:8] = [51, 52, 50]

    def at(u, v, z):
        return [u * z / EXACT_FOCAL, v * z / EXACT_FOCAL, z]
    nan, inf = float("nan"), float("inf")
    even = lambda k: k % 2 == 0
    cases = [
        ("u = v = -0.5 rounds to -0: pixel (0, 0)", at(-0.5, -0.5, 1.0), 1),
        ("u = -0.5, z = 4", at(-0.5, 2.0, 4.0), 1),
        ("u = -1.5 rounds to -2", at(-1.5, 2.0, 2.0), 0),
        ("u = w - 0.5 rounds to the even neighbour", at(w - 0.5, 1.0, 1.0), 1 if even(w - 1) else 0),
        ("v = h - 0.5 rounds to the even neighbour", at(1.0, h - 0.5, 2.0), 1 if even(h - 1) else 0),
        ("u = w - 1.5 is inside either way", at(w - 1.5, 1.0, 4.0), 1),
        ("u = w exactly", at(float(w), 1.0, 1.0), 0),
        ("v = h exactly", at(1.0, float(h), 2.0), 0),
        ("u = w - 1, v = h - 1: the last pixel", at(w - 1.0, h - 1.0, 4.0), 1),
        ("u = w - 1, v = 0: a swapped h / w or u / v reads outside", at(w - 1.0, 0.0, 1.0), 1),
        ("behind the camera, inside the image: counts", at(4.0, 2.0, -2.0), 1),
        ("z = 0: p2 = 0, infinite coordinates", [1.0, 1.0, 0.0], 0),
        ("the origin: 0 / 0", [0.0, 0.0, 0.0], 0),
        ("a NaN coordinate", [nan, 0.5, 1.0], 0),
        ("an infinite coordinate", [inf, 0.5, 1.0], 0),
        ("strength exactly the threshold: not visible", at(5.0, 3.0, 2.0), 0),
        ("strength one step above the threshold", at(6.0, 3.0, 1.0), 1),
        ("strength one step below the threshold", at(7.0, 3.0, 4.0), 0),
    ]
    return intr, c2w, maps, np.array([c[1] for c in cases], dtype=np.float64), np.array([c[2] for c in cases], dtype=np.int32), [c[0] for c in cases]
