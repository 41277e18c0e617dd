"""The rule of include/monosowa_lift.h restated pixel by pixel in Python scalars (a Python float is an IEEE double; every operation
rounds on its own), a literal numpy statement of the reference's steps on the same float32 points, a scalar gather, and the generator
of the test scenes.  Written from the header, not from monosowa_amd/lift.py: the erosion here is scipy's ``binary_dilation`` of the
inverted mask, the medians are ``np.median`` on float64 copies."""
import functools
import math

import numpy as np
import scipy.ndimage

OK, FEW, FAR, BEHIND, ABSENT, CLIPPED = 0, 1, 2, 3, 4, 8
CFG = {"filtering": {"moving_detection_threshold": 2, "filter_diameter": 4},
       "frames_creation": {"use_pseudo_lidar": True, "max_distance_pseudo_lidar": 75.0, "nscans_before": 1}}
THR, D, MAX_RANGE, REF_FRAME = 2, 4.0, 75.0, 1
FIELDS = ("points", "counts", "total", "centres", "range", "truncated", "status", "shrink")
MARGIN = 1e-6


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


# ---------------------------------------------------------------------------------------------------------------- the rule
def eroded(mask, r):
    """E_r by scipy: cross structuring element, border value 0 for the dilation of the complement (outside counts as set)."""
    return ~scipy.ndimage.binary_dilation(~mask, iterations=r)


def _points(depth, intr, chosen):
    """rule 1 over the pixels of bool ``chosen`` in row-major order -> list of (x, y, z) np.float32"""
    fx, fy, cx, cy = (float(v) for v in intr)
    out = []
    for v, u in np.argwhere(chosen):
        z = depth[v, u]
        if not (np.isfinite(z) and z > 0):
            continue
        zd = float(z)
        out.append((np.float32(((float(u) - cx) / fx) * zd), np.float32(((float(v) - cy) / fy) * zd), np.float32(z)))
    return out


def _median(pts):
    return [float(m) for m in np.median(np.asarray(pts, dtype=np.float64).reshape(-1, 3), axis=0)]


def _circle(pts, m, d, margins):
    keep = []
    for p in pts:
        dx, dz = float(p[0]) - m[0], float(p[2]) - m[2]
        q = dx * dx + dz * dz
        margins["circle"] = min(margins["circle"], abs(q - d * d) / (d * d))
        if q < d * d:
            keep.append(p)
    return keep


def _move(T, x, y, z):
    return [((float(T[a, 0]) * x + float(T[a, 1]) * y) + float(T[a, 2]) * z) + float(T[a, 3]) for a in range(3)]


def lift_rule(depth, intrinsics, masks, mask_count=None, poses=None, nmax=40, thr=THR, d=D, use_range=True, max_range=MAX_RANGE):
    """-> (dict of the eight outputs as numpy arrays, with rows of ``points`` at and beyond counts zero; margins: the smallest
    relative distance of any circle, range or sign decision from its threshold)"""
    F, M, H, W = masks.shape
    out = {"points": np.zeros((F, M, nmax, 3), np.float32), "counts": np.zeros((F, M), np.int32), "total": np.zeros((F, M), np.int32),
           "centres": np.zeros((F, M, 3)), "range": np.zeros((F, M)), "truncated": np.zeros((F, M), bool),
           "status": np.full((F, M), ABSENT, np.int32), "shrink": np.full((F, M), -1, np.int32)}
    margins = {"circle": np.inf, "range": np.inf, "front": np.inf}
    for f in range(F):
        T = np.eye(3, 4) if poses is None else np.asarray(poses[f], dtype=np.float64)
        count = M if mask_count is None else max(0, min(int(mask_count[f]), M))
        for m in range(count):
            mask = np.asarray(masks[f, m]) != 0
            out["status"][f, m] = FEW
            out["truncated"][f, m] = bool(mask[:10].any() or mask[-10:].any())
            s = 2 + math.isqrt(int(mask.sum())) // 10
            for chosen, shrink in ((eroded(mask, s), s), (eroded(mask, 1), 1), (mask, -1)):
                S = _points(depth[f], intrinsics[f], chosen)
                if len(S) >= thr:
                    break
            else:
                continue
            out["shrink"][f, m] = shrink
            med = _median(S)
            inside = _circle(S, med, d, margins)
            if inside:
                med = _median(inside)
            if use_range:
                r2 = (med[0] * med[0] + med[1] * med[1]) + med[2] * med[2]
                margins["range"] = min(margins["range"], abs(r2 - max_range * max_range) / (max_range * max_range))
                if r2 > max_range * max_range:
                    out["status"][f, m] = FAR
                    continue
            c = _move(T, *med)
            terms = max(abs(float(T[2, a]) * med[a]) for a in range(3))
            if not math.isnan(c[2]):
                margins["front"] = min(margins["front"], abs(c[2]) / max(terms, abs(float(T[2, 3])), 1e-300))
            if not c[2] > 0:
                out["status"][f, m] = BEHIND
                continue
            cloud = _points(depth[f], intrinsics[f], mask)
            cloud = _circle(cloud, _median(cloud), d, margins)
            if len(cloud) < thr:
                continue
            with np.errstate(all="ignore"):
                moved = [[np.float32(v) for v in _move(T, float(p[0]), float(p[1]), float(p[2]))] for p in cloud]
            n = min(len(cloud), nmax)
            out["points"][f, m, :n] = np.asarray(moved[:n], dtype=np.float32).reshape(-1, 3)
            out["counts"][f, m], out["total"][f, m] = n, len(cloud)
            out["centres"][f, m] = c
            out["range"][f, m] = math.sqrt(med[0] * med[0] + med[2] * med[2])
            out["status"][f, m] = OK | (CLIPPED if len(cloud) > nmax else 0)
    return out, margins


def assert_same(got, want, what=""):
    """Every output bit for bit; ``points`` over the rows below counts (the others are not written: whatever the buffer held)."""
    for k in FIELDS:
        if k == "points":
            continue
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (what, k, g.tolist(), w.tolist())
    F, M = want["counts"].shape
    assert got["points"].shape == want["points"].shape and got["points"].dtype == np.float32
    for f in range(F):
        for m in range(M):
            n = want["counts"][f, m]
            assert np.array_equal(bits(got["points"][f, m, :n]), bits(want["points"][f, m, :n])), (what, "points", f, m)


# ---------------------------------------------------------------------------------------------------------------- the reference, literally
def lift_literal(depth, intrinsics, masks, mask_count, poses, thr=THR, d=D, max_range=MAX_RANGE):
    """The reference's steps on the float32-rounded points as float64: ``sqrt(...) < d``, ``sqrt(...) > max``, ``np.matmul`` ->
    per slot (status, shrink, centre or None, cloud float64 [n, 3] or None, largest |term| of the centre's rows)."""
    F, M, H, W = masks.shape
    out = {}
    for f in range(F):
        fx, fy, cx, cy = intrinsics[f]
        T = np.concatenate([np.asarray(poses[f], dtype=np.float64), [[0, 0, 0, 1]]]) if poses is not None else np.eye(4)
        z = depth[f]
        valid = np.isfinite(z) & (z > 0)
        with np.errstate(all="ignore"):
            u, v = np.meshgrid(np.arange(W), np.arange(H))
            x32 = (((u - cx) / fx) * z.astype(np.float64)).astype(np.float32)
            y32 = (((v - cy) / fy) * z.astype(np.float64)).astype(np.float32)
        scan = np.stack([x32[valid], y32[valid], z[valid], v[valid], u[valid]]).astype(np.float64)       # rows x y z v u
        behind = lambda mk: np.array([scan[0, mk], scan[1, mk], scan[2, mk]]).T.reshape(-1, 3)
        count = M if mask_count is None else max(0, min(int(mask_count[f]), M))
        for m in range(M):
            if m >= count:
                out[f, m] = (ABSENT, -1, None, None, None)
                continue
            mask_old = np.asarray(masks[f, m]) != 0
            pick = lambda mk: behind(mk[scan[3].astype(int), scan[4].astype(int)])
            shrink = int(2 + np.sqrt(np.count_nonzero(mask_old)) // 10)
            mask = np.invert(scipy.ndimage.binary_dilation(np.invert(mask_old), iterations=shrink))
            lidar = pick(mask)
            if lidar.shape[0] < thr:
                shrink = 1
                lidar = pick(np.invert(scipy.ndimage.binary_dilation(np.invert(mask_old), iterations=1)))
                if lidar.shape[0] < thr:
                    shrink = -1
                    lidar = pick(mask_old)
                    if lidar.shape[0] < thr:
                        out[f, m] = (FEW, -1, None, None, None)
                        continue
            mean = np.median(lidar, axis=0)
            dist = np.sqrt((mean[0] - lidar[:, 0]) ** 2 + (mean[2] - lidar[:, 2]) ** 2)
            lidar = lidar[dist < d]
            if lidar.shape[0] > 0:
                mean = np.median(lidar, axis=0)
            if np.sqrt(mean[0] ** 2 + mean[1] ** 2 + mean[2] ** 2) > max_range:
                out[f, m] = (FAR, shrink, None, None, None)
                continue
            with np.errstate(all="ignore"):
                moved = np.matmul(T[0:3, 0:3], mean.T).transpose() + T[0:3, 3]
            if not moved[2] > 0.:
                out[f, m] = (BEHIND, shrink, None, None, None)
                continue
            lidar = pick(mask_old)
            mean2 = np.median(lidar, axis=0)
            dist = np.sqrt((mean2[0] - lidar[:, 0]) ** 2 + (mean2[2] - lidar[:, 2]) ** 2)
            lidar = lidar[dist < d]
            with np.errstate(all="ignore"):
                lidar = np.matmul(T[0:3, 0:3], lidar.T).T + T[0:3, 3]
            if lidar.shape[0] < thr:
                out[f, m] = (FEW, shrink, None, None, None)
                continue
            with np.errstate(all="ignore"):
                terms = np.abs(np.concatenate([T[0:3, 0:3] * mean[None, :], T[0:3, 3:4]], axis=1)).max(axis=1)
            out[f, m] = (OK, shrink, moved, lidar, terms)
    return out


# ---------------------------------------------------------------------------------------------------------------- gather
def gather_rule(fields, tracks, moving, ref_frame, max_views, K):
    """Rule 7 track by track, point by point -> (points float32 [B, K, 3] with the rows beyond counts zero, counts int32 [B],
    centres float64 [B, 3])"""
    F, M = fields["status"].shape
    B = len(tracks)
    points, counts, centres = np.zeros((B, K, 3), np.float32), np.zeros(B, np.int32), np.zeros((B, 3))
    for b, track in enumerate(tracks):
        views = []
        for v, (f, m) in enumerate(track):
            if not (0 <= f < F and 0 <= m < M) or (int(fields["status"][f, m]) & 7) != OK:
                continue
            if moving is not None and moving[b]:
                if f == ref_frame and not views:
                    views.append((0.0, v, f, m))
                continue
            views.append((float(fields["range"][f, m]) + (5.0 if fields["truncated"][f, m] else 0.0), v, f, m))
        views = sorted(views, key=lambda t: (t[0], t[1]))[:max_views]
        if not views:
            continue
        rows = [fields["points"][f, m, j] for _, _, f, m in views for j in range(int(fields["counts"][f, m]))]
        n = len(rows)
        kept = [rows[j] for j in range(n) if n <= K or ((j + 1) * K) // n > (j * K) // n]
        assert len(kept) == min(n, K)
        points[b, :len(kept)], counts[b] = np.asarray(kept, dtype=np.float32).reshape(-1, 3), len(kept)
        centres[b] = np.median(np.asarray([fields["centres"][f, m] for _, _, f, m in views], dtype=np.float64), axis=0)
    return points, counts, centres


def assert_same_gather(got, want, what=""):
    (gp, gc, gm), (wp, wc, wm) = got, want
    assert np.array_equal(gc, wc) and gc.dtype == np.int32, (what, gc.tolist(), wc.tolist())
    assert np.array_equal(bits(np.asarray(gm, dtype=np.float64)), bits(wm)), (what, gm.tolist(), wm.tolist())
    for b, n in enumerate(wc):
        assert np.array_equal(bits(np.asarray(gp[b, :n])), bits(wp[b, :n])), (what, b)


# ---------------------------------------------------------------------------------------------------------------- the scenes
H, W, M, NMAX = 24, 40, 6, 40
INTR = (31.7, 30.9, 19.3, 11.6)
FAMILIES = {}                                           # (frame, mask) -> what the slot is there for


def _rect(r0, r1, c0, c1, h=H, w=W):
    mk = np.zeros((h, w), dtype=bool)
    mk[r0:r1, c0:c1] = True
    return mk


def _frame(rng, masks, depths, background=30.0):
    """depth: a noisy background with each mask's object (a noisy plane at ``depths[k]``) painted one pixel inside the mask's rows
    and columns where the mask is thicker than four pixels, so that the mask's rim lies on the background"""
    depth = (background + rng.uniform(-0.5, 0.5, size=(H, W))).astype(np.float32)
    for mk, z in zip(masks, depths):
        if z is None or not mk.any():
            continue
        core = eroded(mk, 1) if eroded(mk, 2).any() else mk
        depth[core] = (z + rng.uniform(-0.4, 0.4, size=int(core.sum()))).astype(np.float32)
    return depth


def _turn_y(angle, t):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, 0, s, t[0]], [0, 1, 0, t[1]], [-s, 0, c, t[2]]], dtype=np.float64)


def _scene(seed):
    rng = np.random.default_rng(seed)
    fam, frames = {}, []

    def add(masks, depths, count, pose, names, edit=None):
        f = len(frames)
        masks = list(masks) + [np.zeros((H, W), dtype=bool)] * (M - len(masks))
        depth = _frame(rng, masks, list(depths) + [None] * (M - len(depths)))
        if edit:
            edit(depth)
        frames.append((depth, np.stack(masks), count, pose))
        for m, name in enumerate(names):
            fam[f, m] = name

    hole = _rect(6, 15, 14, 25)
    hole[10, 19] = False
    strip3 = _rect(19, 22, 2, 16)

    def kill_middle(depth):
        depth[20, 2:16] = np.nan
    add([_rect(0, 10, 0, 13), _rect(14, 24, 28, 40), hole, _rect(11, 13, 27, 39), strip3], [10.0, 12.0, 9.0, 11.0, 8.0], 6, np.eye(3, 4),
        ["touches the top and left borders", "touches the bottom and right borders", "a one-pixel hole",
         "a 2-px strip: E_s and E_1 empty", "a 3-px strip whose middle row has no depth: E_1 has no point", "A = 0"], kill_middle)
    few, bad = _rect(2, 3, 30, 35), _rect(12, 22, 26, 38)

    def spoil(depth):
        depth[2, 30:35] = (np.nan, 0.0, 7.5, -3.0, np.inf)
        for (r, c), v in zip(((13, 28), (14, 30), (15, 33), (16, 29), (18, 35), (19, 31)), (0.0, -2.0, np.nan, np.inf, -np.inf, -0.0)):
            depth[r, c] = v
        depth[1:5, 1:5] = np.float32(10.25)             # an even count, every z the same
        depth[12:17, 2:5] = np.float32(9.5)             # an odd count
    add([_rect(1, 10, 8, 19), _rect(1, 11, 20, 30), few, bad, _rect(1, 5, 1, 5), _rect(12, 17, 2, 5)], [10.0, 11.0, None, 9.0, None, None], 6,
        _turn_y(0.3, (1.5, -0.2, 4.0)),
        ["A = 99: s = 2", "A = 100: s = 3", "one valid pixel: fewer than thr", "0, negative, NaN, +-Inf and -0 depth inside",
         "even count, repeated values at the median", "odd count, repeated values"], spoil)
    blob = _rect(4, 20, 5, 30) & (rng.uniform(size=(H, W)) < 0.8)
    wide = _rect(2, 22, 2, 38)
    common = [_rect(2, 12, 3, 15), _rect(13, 23, 3, 15), wide, blob, _rect(8, 20, 30, 38)]
    add(common, [90.0, 10.0, None, 12.0, 20.0], 6, np.eye(3, 4),
        ["beyond 75 m", "plain", "mostly background, beyond 4 m of the median plane", "ragged", "plain, 20 m", "A = 0"])
    add(common, [12.0, 10.0, 14.0, 12.0, 20.0], 6, _turn_y(math.pi, (0.0, 0.0, 2.0)), ["a pose that turns the object behind the camera"] * 5)
    nan_t = np.eye(3, 4)
    nan_t[2, 3] = np.nan
    add(common, [12.0, 10.0, 14.0, 12.0, 20.0], 6, nan_t, ["NaN in the pose's third row: BEHIND"] * 5)
    nan_x = _turn_y(-0.2, (0.0, 0.0, 1.0))
    nan_x[0, 1] = np.nan
    add(common, [12.0, 10.0, 14.0, 12.0, 20.0], 6, nan_x, ["NaN in the pose's first row: OK with NaN x"] * 5)
    add(common, [12.0, 10.0, 14.0, 12.0, 20.0], 0, np.eye(3, 4), ["mask_count = 0"] * 6)
    add(common, [12.0, 10.0, 14.0, 12.0, 20.0], 3, _turn_y(0.1, (0.3, 0.0, -1.0)), ["mask_count = 3 of 6"] * 6)
    depth = np.stack([fr[0] for fr in frames])
    masks = np.stack([fr[1] for fr in frames])
    counts = np.array([fr[2] for fr in frames], dtype=np.int32)
    poses = np.stack([fr[3] for fr in frames])
    intr = np.tile(np.array(INTR, dtype=np.float64), (len(frames), 1))
    intr[1] = (29.3, 33.1, 20.7, 12.2)
    return depth, intr, masks, counts, poses, fam


@functools.lru_cache(maxsize=None)
def scene():
    """The eight small frames (H = 24, W = 40, M = 6) with every edge family, what the rule makes of them at Nmax = 40, and its
    margins: the first seed whose decisions all keep 1e-6 relative from their thresholds.  Computed once; do not write into it."""
    for seed in range(100):
        depth, intr, masks, counts, poses, fam = _scene(seed)
        want, margins = lift_rule(depth, intr, masks, counts, poses, nmax=NMAX)
        if min(margins.values()) > MARGIN:
            FAMILIES.update(fam)
            return (depth, intr, masks, counts, poses), want, margins
    raise AssertionError("no seed keeps the margin")


@functools.lru_cache(maxsize=None)
def large_scene():
    """F = 1, H = 96, W = 320, M = 3: a 60 x 60 mask (s = 8), a 70 x 120 mask (8,400 points, clipped at Nmax = 4096), a ragged one."""
    h, w = 96, 320
    for seed in range(100):
        rng = np.random.default_rng(1000 + seed)
        ragged = _rect(20, 90, 215, 315, h, w) & (rng.uniform(size=(h, w)) < 0.93)
        ragged[40:70, 240:290] = True
        masks = np.stack([_rect(5, 65, 3, 63, h, w), _rect(20, 90, 80, 200, h, w), ragged])[None]
        depth = (40.0 + rng.uniform(-0.5, 0.5, size=(1, h, w))).astype(np.float32)
        for mk, z in zip(masks[0], (9.0, 11.0, 14.0)):
            inner = eroded(mk, 2) if z != 11.0 else mk
            depth[0][inner] = (z + rng.uniform(-0.6, 0.6, size=int(inner.sum()))).astype(np.float32)
        intr = np.array([[260.4, 255.8, 161.3, 47.2]])
        poses = _turn_y(0.05, (0.4, -0.1, 2.5))[None]
        args = (depth, intr, masks, np.array([3], dtype=np.int32), poses)
        want, margins = lift_rule(*args, nmax=4096)
        if min(margins.values()) > MARGIN:
            return args, want, margins
    raise AssertionError("no seed keeps the margin")


def planted_box(centre=(1.0, 1.0, 12.0), dims=(1.5, 1.6, 3.9), h=64, w=128, intr=(120.0, 120.0, 63.5, 31.5)):
    """A box (height, width, length; yaw 0) rendered by ray casting into a depth map over a 40 m background, with its mask
    -> (depth [1, h, w] float32, intrinsics [1, 4], masks [1, 1, h, w] bool)"""
    fx, fy, cx, cy = intr
    lo = np.array([centre[0] - dims[1] / 2, centre[1] - dims[0] / 2, centre[2] - dims[2] / 2])
    hi = np.array([centre[0] + dims[1] / 2, centre[1] + dims[0] / 2, centre[2] + dims[2] / 2])
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1)
    with np.errstate(all="ignore"):
        t0, t1 = lo / ray, hi / ray
    near, far = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)
    hit = (near <= far) & (near > 0)
    depth = np.where(hit, near, 40.0).astype(np.float32)
    return depth[None], np.array([intr], dtype=np.float64), hit[None, None]
