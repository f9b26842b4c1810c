"""The scalar-order numpy mirror of the edge rasteriser (include/emap_raster_hip.h, emap_amd/csrc/raster.hip): every formula of the header
in IEEE doubles, one numpy operation per arithmetic operation (numpy fuses nothing), every sum in the header's order - what the device
result must equal bit for bit -, and the inputs the CPU and the GPU tests share.  A plain module like dtu_eval_ref.py: not collected, no
device work."""
import numpy as np

MAX_COORD = 1099511627776.0          # EMAP_RASTER_MAX_COORD
LIST_CHUNK = 256                     # RASTER_LIST_CHUNK of csrc/raster.hip (the tests assert that the source says so)
TILE_W, TILE_H = 64, 16


def cameras_ref(intrinsics_list, camtoworld_list):
    """intr (F, 4) = fx, fy, cx, cy; R (F, 3, 3), T (F, 3) from np.linalg.inv(camtoworld): what the package passes to the library."""
    K = np.stack([np.asarray(k, dtype=np.float64)[:3, :3] for k in intrinsics_list])
    w2c = np.stack([np.linalg.inv(np.asarray(c, dtype=np.float64)) for c in camtoworld_list])
    intr = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1)
    return np.ascontiguousarray(intr), np.ascontiguousarray(w2c[:, :3, :3]), np.ascontiguousarray(w2c[:, :3, 3])


def cameras_generator(meta):
    """The generator's own camera route (synthetic.make_wireframe_scene: R^T (X - c)) in the table's form: R = c2w[:3, :3]^T and
    T = -(R c) summed left to right."""
    intr, Rs, Ts = [], [], []
    for fr in meta["frames"]:
        K, c2w = np.asarray(fr["intrinsics"], dtype=np.float64), np.asarray(fr["camtoworld"], dtype=np.float64)
        R = np.ascontiguousarray(c2w[:3, :3].T)
        c = c2w[:3, 3]
        Ts.append(-((R[:, 0] * c[0] + R[:, 1] * c[1]) + R[:, 2] * c[2]))
        Rs.append(R)
        intr.append([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    return np.array(intr), np.array(Rs), np.array(Ts)


def bezier_ref(P, t):
    """B(t) of control points P (..., 4, 3) at the scalar t, in the header's association."""
    t = np.float64(t)
    u = np.float64(1.0) - t
    b0, b1, b2, b3 = (u * u) * u, (np.float64(3.0) * (u * u)) * t, (np.float64(3.0) * u) * (t * t), (t * t) * t
    return (b0 * P[..., 0, :] + b1 * P[..., 1, :]) + (b2 * P[..., 2, :] + b3 * P[..., 3, :])


def segments_ref(lines, curves, curve_segments):
    """-> A (S, 3), B (S, 3), edge (S): lines first, then curve by curve, k ascending."""
    lines = np.asarray(lines, dtype=np.float64).reshape(-1, 2, 3)
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 4, 3)
    n = int(curve_segments)
    A, B, E = [lines[:, 0]], [lines[:, 1]], [np.arange(len(lines))]
    for c in range(len(curves)):
        for k in range(n):
            A.append(bezier_ref(curves[c], np.float64(k) / np.float64(n))[None])
            B.append(bezier_ref(curves[c], np.float64(k + 1) / np.float64(n))[None])
            E.append(np.array([len(lines) + c]))
    return np.concatenate(A), np.concatenate(B), np.concatenate(E).astype(np.int64)


def _camera(R, T, X):
    return [((R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1]) + R[i, 2] * X[:, 2]) + T[i] for i in range(3)]


def table_ref(A, B, intr, R, T, h, w, half_width, z_near):
    """The rows of one frame: x0, y0, x1, y1 (S) and the inclusive pixel box (S, 4) = bx0, by0, bx1, by1, empty (0, 0, -1, -1) for a
    dropped segment."""
    with np.errstate(all="ignore"):
        ca, cb = _camera(R, T, A), _camera(R, T, B)
        a_behind, b_behind = ca[2] < z_near, cb[2] < z_near
        drawn = ~(a_behind & b_behind)
        t = (z_near - ca[2]) / (cb[2] - ca[2])
        m = [ca[i] + t * (cb[i] - ca[i]) for i in range(3)]
        one = a_behind != b_behind
        ca = [np.where(one & a_behind, m[i], ca[i]) for i in range(3)]
        cb = [np.where(one & b_behind, m[i], cb[i]) for i in range(3)]
        fx, fy, cx, cy = intr
        x0, y0 = (fx * ca[0]) / ca[2] + cx, (fy * ca[1]) / ca[2] + cy
        x1, y1 = (fx * cb[0]) / cb[2] + cx, (fy * cb[1]) / cb[2] + cy
        drawn &= (np.abs(x0) < MAX_COORD) & (np.abs(y0) < MAX_COORD) & (np.abs(x1) < MAX_COORD) & (np.abs(y1) < MAX_COORD)
        box = np.tile(np.array([0, 0, -1, -1], dtype=np.int64), (len(x0), 1))
        for s in np.nonzero(drawn)[0]:
            lo_x, hi_x = np.floor(min(x0[s], x1[s]) - half_width) - 1.0, np.ceil(max(x0[s], x1[s]) + half_width) + 1.0
            lo_y, hi_y = np.floor(min(y0[s], y1[s]) - half_width) - 1.0, np.ceil(max(y0[s], y1[s]) + half_width) + 1.0
            if lo_x <= w - 1 and hi_x >= 0 and lo_y <= h - 1 and hi_y >= 0:
                box[s] = int(max(lo_x, 0.0)), int(max(lo_y, 0.0)), int(min(hi_x, w - 1.0)), int(min(hi_y, h - 1.0))
    return x0, y0, x1, y1, box, drawn


def pixel_values(xs, ys, x0, y0, x1, y1, half_width, weight):
    """v of the pixels (xs, ys) - float64 arrays - for one segment: the header's pixel formula."""
    ux, uy = x1 - x0, y1 - y0
    t = ((xs - x0) * ux + (ys - y0) * uy) / ((ux * ux + uy * uy) + 1e-9)
    t = np.minimum(np.maximum(t, 0.0), 1.0)
    ex, ey = xs - (x0 + t * ux), ys - (y0 + t * uy)
    d = np.sqrt(ex * ex + ey * ey)
    return np.minimum(np.maximum(half_width - d, 0.0), 1.0) * weight


def raster_ref(lines, curves, intr, R, T, h, w, half_width=1.5, weights=None, curve_segments=32, z_near=1e-3, full_image=False):
    """-> bytes (F, h, w) uint8, ids (F, h, w) int32, value (F, h, w) float64.  ``full_image``: every drawn segment against every pixel
    instead of the pixels of its box - the same maps below the coordinate bound."""
    A, B, E = segments_ref(lines, curves, curve_segments)
    n_edges = len(np.asarray(lines).reshape(-1, 6)) + len(np.asarray(curves).reshape(-1, 12))
    wt = np.ones(n_edges) if weights is None else np.asarray(weights, dtype=np.float64)
    F = len(intr)
    val = np.zeros((F, h, w), dtype=np.float64)
    ids = np.full((F, h, w), -1, dtype=np.int32)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    for f in range(F):
        x0, y0, x1, y1, box, drawn = table_ref(A, B, intr[f], R[f], T[f], h, w, half_width, z_near)
        for s in range(len(A)):                     # ascending edge order; only a strictly larger v replaces: the lowest edge wins a tie
            if full_image:
                if not drawn[s]:
                    continue
                bx0, by0, bx1, by1 = 0, 0, w - 1, h - 1
            else:
                bx0, by0, bx1, by1 = box[s]
                if bx1 < bx0 or by1 < by0:
                    continue
            sl = (slice(by0, by1 + 1), slice(bx0, bx1 + 1))
            v = pixel_values(xs[sl], ys[sl], x0[s], y0[s], x1[s], y1[s], half_width, wt[E[s]])
            better = v > val[f][sl]
            val[f][sl] = np.where(better, v, val[f][sl])
            ids[f][sl] = np.where(better, E[s], ids[f][sl])
    return np.rint(255.0 * val).astype(np.uint8), ids, val


def raster_meta_ref(lines, curves, meta, **kw):
    """raster_ref in the cameras of a meta_data dict, through np.linalg.inv as the package forms them."""
    intr, R, T = cameras_ref([f["intrinsics"] for f in meta["frames"]], [f["camtoworld"] for f in meta["frames"]])
    return raster_ref(lines, curves, intr, R, T, int(meta["height"]), int(meta["width"]), **kw)


# ------------------------------------------------------------------------------------------------ the shared test scene
def look_at(eye, target=(0.0, 0.0, 0.0)):
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    zax = (target - eye) / np.linalg.norm(target - eye)
    xax = np.cross([0.0, 1.0, 0.0], zax)
    xax /= np.linalg.norm(xax)
    yax = np.cross(zax, xax)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = xax, yax, zax, eye
    return c2w


def scene_views(F, h, w):
    """F cameras: view 0 at (0, 0, -2) looking down +z with the axes aligned (x right, y down) - the hand-placed geometry of scene_edges is
    written for it -, the others on a ring of radius 2.  fx != fy, principal point off centre."""
    fx, fy = 0.9 * max(w, 2), 1.1 * max(h, 2)
    K = np.array([[fx, 0, (w - 1) / 2 + 0.25, 0], [0, fy, (h - 1) / 2 - 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    poses = [look_at((0.0, 0.0, -2.0))]
    for i in range(1, F):                         # a fixed angular step: the views of a smaller F are the first of a larger one
        th = 1.1 * i + 0.3
        poses.append(look_at((2 * np.sin(th), 0.4 * np.cos(3 * th), -2 * np.cos(th))))
    return [K] * F, poses


def pixel_to_world(K, px, py, depth=2.0):
    """The world point that view 0 of scene_views (at (0, 0, -2), axes aligned) projects to pixel (px, py), at camera depth `depth`."""
    return [(px - K[0, 2]) * depth / K[0, 0], (py - K[1, 2]) * depth / K[1, 1], depth - 2.0]


def scene_edges(h, w):
    """Five lines and three curves whose projections into view 0 of scene_views(F, h, w) cover the cases the tile kernel can get wrong:
    -> lines (5, 2, 3), curves (3, 4, 3), weights (8).
      line 0   crosses the near plane of view 0 (one end behind the camera)
      line 1   wholly behind the camera of view 0
      line 2   wholly outside the image of view 0 (far to the right)
      line 3   zero length: a dot on a pixel centre
      line 4   along the top image border (y = 0), across the full width and past both sides
      curve 0  a straight cubic ON line 4: both saturate the same pixels, the lower edge index (4) must win; weight 1 like line 4
      curves 1, 2   an arc and an S through the middle of the image, weights < 1
    """
    K = scene_views(1, h, w)[0][0]
    P = lambda px, py, d=2.0: pixel_to_world(K, px, py, d)
    lines = np.array([
        [P(0.3 * w, 0.8 * h), [0.05, 0.02, -2.5]],
        [[-0.3, 0.1, -2.5], [0.4, -0.2, -3.0]],
        [P(5.0 * w + 40, 0.2 * h), P(6.0 * w + 40, 0.7 * h)],
        [P(w // 4, h // 2), P(w // 4, h // 2)],
        [P(-3.0, 0.0), P(w + 2.0, 0.0)],
    ], dtype=np.float64)
    a, b = np.array(P(-3.0, 0.0)), np.array(P(w + 2.0, 0.0))
    curves = np.array([
        [a, a + (b - a) / 3, a + 2 * (b - a) / 3, b],
        [P(0.1 * w, 0.9 * h), P(0.1 * w, 0.1 * h, 1.6), P(0.9 * w, 0.1 * h, 2.4), P(0.9 * w, 0.9 * h)],
        [P(0.2 * w, 0.3 * h), P(1.1 * w, 0.3 * h), P(-0.1 * w, 0.7 * h), P(0.8 * w, 0.7 * h)],
    ], dtype=np.float64)
    weights = np.array([1.0, 1.0, 1.0, 0.75, 1.0, 1.0, 0.5, 0.8125])
    return lines, curves, weights


def tiny_segments(h, w, n):
    """n short segments (a third of a pixel) packed inside one 64 x 16 tile of view 0 of scene_views(1, h, w): (n, 2, 3)."""
    K = scene_views(1, h, w)[0][0]
    x_hi, y_hi = min(w, TILE_W) - 1, min(h, TILE_H) - 1
    out = []
    for i in range(n):
        px, py = (i * 0.37) % max(x_hi, 1), (i * 0.61) % max(y_hi, 1)
        out.append([pixel_to_world(K, px, py), pixel_to_world(K, px + 0.3, py + 0.1)])
    return np.array(out, dtype=np.float64)
