"""Object clouds: a metric depth map and instance masks to what the template search takes (include/monosowa_lift.h has the rule).

    lifter = ObjectLifter(cfg=None, device=None, max_points=16384)      cfg with the reference's key names (``lift_config``)
    res = lifter.lift(depth, intrinsics, masks, mask_count=None, poses=None)              -> LiftResult, tensors on the device
    res = lift_host(depth, intrinsics, masks, mask_count, poses, cfg, max_points)         the same contract in numpy (a CPU device;
                                                                        the fallback beyond the kernel's limits: res.host says so)
    clouds, counts, centres = res.gather(tracks, moving=None, max_views=10, max_points=10000)
    fit = TemplateFitter(template).fit((clouds, counts), centres, moving=moving)

What it reproduces: the reference's ``decode_img`` (a depth map back-projected to a pseudo-lidar), ``get_car_locations_from_img`` (the
mask shrunk by ``binary_dilation`` of its complement, the points behind it, medians, the circle filter, the range cut, the move into the
reference frame) and ``standing_concatenate_lidar_clever`` / ``moving_lidar_keep_ref`` (the best views of a track concatenated).
Stated deviations: float32 points with double medians (the reference's points are float64); the circle and range tests compare squares;
mask membership is read at the pixel itself; a track beyond ``max_points`` is thinned by even spacing, not ``np.random.choice``;
products run left to right.  ``tracks`` and ``moving`` come from the tracker (monosowa_amd/track.py: ``ObjectTracker.track(res)``, then
``res.gather(*tr.gather_args())``) or from the caller; ICP stays with the caller.  HDBSCAN and context-aware growing are refused with ``ValueError``.
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmonosowa_lift.so")
ABI_VERSION = 1
NULL, BAD_SIZE, TOO_LARGE = -1, -2, -3
MAX_SIDE, MAX_M, MAX_F, MAX_POINTS, MAX_TRACKS, MAX_VIEWS = 4096, 256, 4096, 1 << 20, 65536, 256
MAX_PIXELS = 2530 * 2530 - 1        # s + 1 <= 255: the clipped distances are bytes
OK, FEW, FAR, BEHIND, ABSENT, CLIPPED = 0, 1, 2, 3, 4, 8
RECORD_INTS = 16
STAGES = (("box", 1), ("columns", 2), ("rows", 4), ("cloud", 8))
ALL_STAGES = 15

LiftConfig = collections.namedtuple("LiftConfig", "thr d use_range max_range ref_frame")

_DEFAULTS = {
    "filtering": {"moving_detection_threshold": 2, "filter_diameter": 4},
    "frames_creation": {"use_pseudo_lidar": True, "max_distance_pseudo_lidar": 75.0, "nscans_before": 30, "use_hdbscan": False,
                        "use_growing_for_point_extraction": False},
}

_lib = None


def load():
    """libmonosowa_lift.so; a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_PATH):
        raise RuntimeError("HIP extension %s is missing: build it with `python -m monosowa_amd.build`" % _PATH)
    lib = ctypes.CDLL(_PATH)
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.mono_lift_abi_version.restype = I
    lib.mono_lift_objects_f32.restype = I
    lib.mono_lift_objects_f32.argtypes = [P, P, P, P, P, I, I, I, I, I, I, D, I, D, I, P, P, P, P, P, P, P, P, P, P, P, P]
    lib.mono_lift_gather_f32.restype = I
    lib.mono_lift_gather_f32.argtypes = [P, P, P, P, P, P, I, I, I, P, P, I, I, I, I, I, P, P, P, P]
    if lib.mono_lift_abi_version() != ABI_VERSION:
        raise RuntimeError("ABI version mismatch in %s" % _PATH)
    _lib = lib
    return lib


# ---------------------------------------------------------------------------------------------------------------- configuration
def _flag(key, v):
    if not isinstance(v, bool):
        raise ValueError("%s = %r is not true or false" % (key, v))
    return v


def _count(key, v, least):
    if isinstance(v, bool) or not isinstance(v, int) or v < least:
        raise ValueError("%s = %r is not an integer >= %d" % (key, v, least))
    return v


def _length(key, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0 or not math.isfinite(float(v) * float(v)):
        raise ValueError("%s = %r is not a positive finite number with a finite square" % (key, v))
    return float(v)


def lift_config(cfg=None):
    """A dict with the reference's sections and key names -> a checked ``LiftConfig``; absent keys take the reference's defaults, keys
    this module does not read are left alone, anything malformed or unsupported is a ValueError."""
    if cfg is None:
        cfg = {}
    if isinstance(cfg, LiftConfig):
        return cfg
    if not isinstance(cfg, dict):
        raise ValueError("cfg = %r is not a mapping" % (cfg,))
    get = {}
    for section, keys in _DEFAULTS.items():
        given = cfg.get(section) or {}
        if not isinstance(given, dict):
            raise ValueError("%s = %r is not a mapping" % (section, given))
        for k, default in keys.items():
            get[k] = given.get(k, default)
    if _flag("frames_creation.use_hdbscan", get["use_hdbscan"]):
        raise ValueError("frames_creation.use_hdbscan = True: HDBSCAN and the isolation-forest ensemble are not built")
    if _flag("frames_creation.use_growing_for_point_extraction", get["use_growing_for_point_extraction"]):
        raise ValueError("frames_creation.use_growing_for_point_extraction = True: context-aware growing is not built")
    return LiftConfig(_count("filtering.moving_detection_threshold", get["moving_detection_threshold"], 1),
                      _length("filtering.filter_diameter", get["filter_diameter"]),
                      _flag("frames_creation.use_pseudo_lidar", get["use_pseudo_lidar"]),
                      _length("frames_creation.max_distance_pseudo_lidar", get["max_distance_pseudo_lidar"]),
                      _count("frames_creation.nscans_before", get["nscans_before"], 0))


# ---------------------------------------------------------------------------------------------------------------- the host routine
def l1_distance(mask, cap):
    """Rule 2's D, clipped at ``cap``: the L1 distance from each pixel of bool ``mask`` [H, W] to the nearest in-image pixel that is
    not set, as the kernels find it: a sweep down and up every column, then min over |du| < cap of that + |du| along every row."""
    H, W = mask.shape
    g = np.zeros((H, W), dtype=np.int32)
    run = np.full(W, cap, dtype=np.int32)
    for r in range(H):
        run = np.where(mask[r], np.minimum(run + 1, cap), 0)
        g[r] = run
    run = np.full(W, cap, dtype=np.int32)
    for r in range(H - 1, -1, -1):
        run = np.where(mask[r], np.minimum(run + 1, cap), 0)
        g[r] = np.minimum(g[r], run)
    D = g.copy()
    for du in range(1, min(cap, W)):
        D[:, du:] = np.minimum(D[:, du:], g[:, :-du] + du)
        D[:, :-du] = np.minimum(D[:, :-du], g[:, du:] + du)
    return D


def _median(p):
    """float64 [n, 3], n > 0 -> the per-axis median, (lo + hi) * 0.5"""
    srt = np.sort(p, axis=0)
    n = p.shape[0]
    return (srt[(n - 1) // 2] + srt[n // 2]) * 0.5


def _in_circle(p, m, d):
    dx, dz = p[:, 0] - m[0], p[:, 2] - m[2]
    return dx * dx + dz * dz < d * d


def _move(T, x, y, z):
    """rows of [3, 4] ``T`` applied as ((r0 x + r1 y) + r2 z) + t -> three arrays (or scalars)"""
    return [((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)]


def _as_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _checked(depth, intrinsics, masks, mask_count, poses, shape_of=lambda a: tuple(a.shape if hasattr(a, "shape") else np.shape(a))):
    """The shapes of ``lift``'s arguments -> (F, M, H, W); a ValueError says which one is wrong."""
    if len(shape_of(depth)) != 3:
        raise ValueError("depth must be [F, H, W], got %s" % (shape_of(depth),))
    F, H, W = shape_of(depth)
    if H < 1 or W < 1:
        raise ValueError("depth has an empty image: %s" % (shape_of(depth),))
    if len(shape_of(masks)) != 4 or shape_of(masks)[0] != F or shape_of(masks)[2:] != (H, W):
        raise ValueError("masks must be [%d, M, %d, %d], got %s" % (F, H, W, shape_of(masks)))
    if shape_of(intrinsics) != (F, 4):
        raise ValueError("intrinsics must be [%d, 4] (fx, fy, cx, cy), got %s" % (F, shape_of(intrinsics)))
    if mask_count is not None and shape_of(mask_count) != (F,):
        raise ValueError("mask_count must be [%d], got %s" % (F, shape_of(mask_count)))
    if poses is not None and shape_of(poses) != (F, 3, 4):
        raise ValueError("poses must be [%d, 3, 4], got %s" % (F, shape_of(poses)))
    return F, shape_of(masks)[1], H, W


def _max_points(v):
    return _count("max_points", v, 1)


def lift_host(depth, intrinsics, masks, mask_count=None, poses=None, cfg=None, max_points=16384):
    """``ObjectLifter.lift`` in numpy under the rule: float32 points, everything else in float64.  CPU tensors out."""
    c, Nmax = lift_config(cfg), _max_points(max_points)
    depth, intrinsics, masks = _as_numpy(depth), _as_numpy(intrinsics), _as_numpy(masks)
    mask_count = None if mask_count is None else _as_numpy(mask_count)
    poses = None if poses is None else _as_numpy(poses)
    F, M, H, W = _checked(depth, intrinsics, masks, mask_count, poses)
    if masks.dtype.kind not in "bui":
        raise ValueError("masks must be bool or uint8, got %s" % masks.dtype)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    intrinsics = np.asarray(intrinsics, dtype=np.float64)
    masks = masks != 0
    mask_count = np.full(F, M, dtype=np.int64) if mask_count is None else np.clip(np.asarray(mask_count, dtype=np.int64), 0, M)
    poses = np.tile(np.eye(3, 4), (F, 1, 1)) if poses is None else np.asarray(poses, dtype=np.float64)
    out = {"points": np.zeros((F, M, Nmax, 3), dtype=np.float32), "counts": np.zeros((F, M), dtype=np.int32),
           "total": np.zeros((F, M), dtype=np.int32), "centres": np.zeros((F, M, 3)), "range": np.zeros((F, M)),
           "truncated": np.zeros((F, M), dtype=bool), "status": np.full((F, M), ABSENT, dtype=np.int32),
           "shrink": np.full((F, M), -1, dtype=np.int32)}
    u, v = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    with np.errstate(all="ignore"):
        for f in range(F):
            fx, fy, cx, cy = intrinsics[f]
            z32 = depth[f]
            valid = np.isfinite(z32) & (z32 > 0)
            z64 = z32.astype(np.float64)
            x32 = (((u - cx) / fx)[None, :] * z64).astype(np.float32)
            y32 = (((v - cy) / fy)[:, None] * z64).astype(np.float32)
            T = poses[f]
            for m in range(int(mask_count[f])):
                _lift_one(out, f, m, masks[f, m], valid, x32, y32, z32, T, c, Nmax)
    return LiftResult(c, True, **{k: torch.from_numpy(a) for k, a in out.items()})


def _lift_one(out, f, m, mask, valid, x32, y32, z32, T, c, Nmax):
    H = mask.shape[0]
    out["status"][f, m] = FEW
    rows = np.flatnonzero(mask.any(axis=1))
    out["truncated"][f, m] = bool(rows.size and (rows[0] < 10 or rows[-1] >= H - 10))
    area = int(np.count_nonzero(mask))
    s = 2 + math.isqrt(area) // 10
    if area == 0:
        return
    cols = np.flatnonzero(mask.any(axis=0))
    # the box with one more pixel on every side that the image has: those pixels are not set, the image's own edge is left open
    r0, r1, c0, c1 = max(rows[0] - 1, 0), min(rows[-1] + 2, H), max(cols[0] - 1, 0), min(cols[-1] + 2, mask.shape[1])
    box = (slice(r0, r1), slice(c0, c1))
    mk, ok = mask[box], valid[box]
    D = l1_distance(mk, s + 1)
    pts = np.stack([x32[box], y32[box], z32[box]], axis=-1)
    for chosen, shrink in (((D >= s + 1) & ok, s), ((D >= 2) & ok, 1), (mk & ok, -1)):
        if np.count_nonzero(chosen) >= c.thr:
            break
    else:
        return
    out["shrink"][f, m] = shrink
    S = pts[chosen].astype(np.float64)
    med = _median(S)
    inside = _in_circle(S, med, c.d)
    if inside.any():
        med = _median(S[inside])
    if c.use_range and (med[0] * med[0] + med[1] * med[1]) + med[2] * med[2] > c.max_range * c.max_range:
        out["status"][f, m] = FAR
        return
    centre = np.array(_move(T, med[0], med[1], med[2]))
    if not centre[2] > 0:
        out["status"][f, m] = BEHIND
        return
    cloud = pts[mk & ok].astype(np.float64)
    cloud = cloud[_in_circle(cloud, _median(cloud), c.d)]
    total = cloud.shape[0]
    if total < c.thr:
        return
    moved = np.stack(_move(T, cloud[:, 0], cloud[:, 1], cloud[:, 2]), axis=1).astype(np.float32)
    n = min(total, Nmax)
    out["points"][f, m, :n] = moved[:n]
    out["counts"][f, m], out["total"][f, m] = n, total
    out["centres"][f, m] = centre
    out["range"][f, m] = np.sqrt(med[0] * med[0] + med[2] * med[2])
    out["status"][f, m] = OK | (CLIPPED if total > Nmax else 0)


def _track_table(tracks, F, M):
    """a list of lists of (frame, mask) pairs, or an integer table [B, V, 2] -> int32 [B, V, 2] (tensor or array), -1 where a row
    has fewer views"""
    if isinstance(tracks, (torch.Tensor, np.ndarray)):
        if tracks.ndim != 3 or tracks.shape[2] != 2 or tracks.shape[1] < 1:
            raise ValueError("a track table must be int32 [B, V, 2] with V >= 1, got %s" % (tuple(tracks.shape),))
        if (tracks.dtype.is_floating_point if isinstance(tracks, torch.Tensor) else tracks.dtype.kind not in "iu"):
            raise ValueError("a track table must hold integers, got %s" % tracks.dtype)
        return tracks
    rows = [list(t) for t in tracks]
    table = np.full((len(rows), max([len(t) for t in rows] + [1]), 2), -1, dtype=np.int32)
    for b, t in enumerate(rows):
        for v, pair in enumerate(t):
            pair = tuple(pair)
            if len(pair) != 2 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in pair):
                raise ValueError("tracks[%d][%d] = %r is not a (frame, mask) pair of integers" % (b, v, pair))
            if not (0 <= pair[0] < F and 0 <= pair[1] < M):
                raise ValueError("tracks[%d][%d] = %r lies outside %d frames x %d masks" % (b, v, pair, F, M))
            table[b, v] = pair
    return table


def gather_host(fields, table, moving, ref_frame, max_views, K):
    """Rule 7 in numpy: ``fields`` the numpy arrays of a LiftResult, ``table`` int [B, V, 2], ``moving`` bool [B] ->
    (points float32 [B, K, 3], counts int32 [B], centres float64 [B, 3])"""
    F, M = fields["status"].shape
    B = table.shape[0]
    points, counts, centres = np.zeros((B, K, 3), dtype=np.float32), np.zeros(B, dtype=np.int32), np.zeros((B, 3))
    for b in range(B):
        views, keys = [], []
        for v, (f, m) in enumerate(table[b].tolist()):
            if not (0 <= f < F and 0 <= m < M) or (fields["status"][f, m] & 7) != OK or (moving[b] and f != ref_frame):
                continue
            views.append((f, m))
            keys.append(float(v) if moving[b] else fields["range"][f, m] + (5.0 if fields["truncated"][f, m] else 0.0))
        order = np.argsort(np.asarray(keys, dtype=np.float64), kind="stable")[:1 if moving[b] else max_views]
        kept = [views[i] for i in order]
        if not kept:
            continue
        cloud = np.concatenate([fields["points"][f, m, :fields["counts"][f, m]] for f, m in kept], axis=0)
        n = cloud.shape[0]
        if n > K:
            j = np.arange(n, dtype=np.int64)
            cloud = cloud[((j + 1) * K) // n > (j * K) // n]
        points[b, :cloud.shape[0]], counts[b] = cloud, cloud.shape[0]
        cs = np.array([fields["centres"][f, m] for f, m in kept]).reshape(-1, 3)
        centres[b] = np.where(np.isnan(cs).any(axis=0), np.nan, _median(np.where(np.isnan(cs), np.inf, cs)))
    return points, counts, centres


# ---------------------------------------------------------------------------------------------------------------- results
class LiftResult:
    """Per (frame, mask) slot: ``points`` float32 [F, M, Nmax, 3] in the reference frame (rows at and beyond ``counts`` hold nothing),
    ``counts`` int32, ``total`` int32 (before clipping at Nmax), ``centres`` float64 [F, M, 3], ``range`` float64, ``truncated`` bool,
    ``status`` int32 (OK, FEW, FAR, BEHIND, ABSENT; OK | CLIPPED when total > Nmax), ``shrink`` int32 (the erosion radius taken; -1:
    the mask itself).  ``host``: the lift went through ``lift_host``."""
    FIELDS = ("points", "counts", "total", "centres", "range", "truncated", "status", "shrink")

    def __init__(self, config, host, **fields):
        self.config, self.host = config, host
        for k in self.FIELDS:
            setattr(self, k, fields[k])
        self.timing = None

    def numpy(self):
        """The fields as numpy arrays (a synchronisation for a result on the GPU)."""
        return {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}

    def gather(self, tracks, moving=None, max_views=10, max_points=10000):
        """``tracks``: a list of lists of (frame, mask) pairs, or an int32 table [B, V, 2] (rows padded with -1).  The two differ in
        one point: a pair of a list that lies outside F x M is a ValueError (the list is checked on the host anyway); a table, which
        may live on the device, is not read back, and a pair outside F x M in it is skipped, as rule 7 says.  ``moving``: per
        track, true = only the view of the reference frame (index ``nscans_before``).  -> ``clouds`` float32 [B, max_points, 3],
        ``counts`` int32 [B], ``centres`` float64 [B, 3]: ``TemplateFitter.fit((clouds, counts), centres, moving=moving)``.  On a GPU
        everything is decided on the device from status, range and counts; nothing is read back."""
        F, M, Nmax = (int(x) for x in self.points.shape[:3])
        K, max_views = _max_points(max_points), _count("max_views", max_views, 1)
        table = _track_table(tracks, F, M)
        B, V = int(table.shape[0]), int(table.shape[1])
        if moving is not None and not isinstance(moving, torch.Tensor):
            moving = np.asarray(list(moving), dtype=bool)
        if moving is not None and tuple(moving.shape) != (B,):
            raise ValueError("moving has shape %s for %d tracks" % (tuple(moving.shape), B))
        dev = self.points.device
        if dev.type != "cuda" or B > MAX_TRACKS or V > MAX_VIEWS or K > MAX_POINTS or B == 0:
            mv = np.zeros(B, dtype=bool) if moving is None else _as_numpy(moving).astype(bool)
            out = gather_host(self.numpy(), _as_numpy(table).astype(np.int64), mv, self.config.ref_frame, max_views, K)
            return tuple(torch.from_numpy(a).to(dev) for a in out)
        table = torch.as_tensor(table).to(device=dev, dtype=torch.int32).contiguous()
        if moving is not None:
            moving = (torch.as_tensor(moving).to(dev) != 0).view(torch.uint8).contiguous()
        points = torch.empty((B, K, 3), dtype=torch.float32, device=dev)
        counts = torch.empty((B,), dtype=torch.int32, device=dev)
        centres = torch.empty((B, 3), dtype=torch.float64, device=dev)
        trunc = self.truncated.view(torch.uint8) if self.truncated.dtype == torch.bool else self.truncated
        ptr = lambda t: t.data_ptr()
        with torch.cuda.device(dev):
            call = lambda: load().mono_lift_gather_f32(
                ptr(self.points), ptr(self.counts), ptr(self.status), ptr(self.range), ptr(trunc), ptr(self.centres),
                F, M, Nmax, ptr(table), None if moving is None else ptr(moving), B, V, self.config.ref_frame, max_views, K, ptr(points),
                ptr(counts), ptr(centres), torch.cuda.current_stream().cuda_stream)
            _check(_timed(self.timing, "gather", call), "mono_lift_gather_f32")
        return points, counts, centres


def _timed(timing, name, call):
    if timing is None:
        return call()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = call()
    end.record()
    timing.append((name, start, end))
    return out


def _check(code, what):
    if code:
        raise RuntimeError("%s failed with code %d" % (what, code))


class ObjectLifter:
    """``cfg``: see ``lift_config``.  ``device``: where ``lift`` runs (default: the current GPU when there is one, else the CPU, where
    ``lift`` is ``lift_host``).  ``max_points``: Nmax, the rows kept per (frame, mask) slot."""

    def __init__(self, cfg=None, device=None, max_points=16384):
        self.config = lift_config(cfg)
        self.max_points = _max_points(max_points)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self.timing = None          # a list: every stage appends (name, start event, end event) to it (tools/lift_rate.py)

    def within_limits(self, F, M, H, W):
        """Whether the kernels take this lift (include/monosowa_lift.h: Limits)."""
        return (F <= MAX_F and M <= MAX_M and H <= MAX_SIDE and W <= MAX_SIDE and H * W <= MAX_PIXELS
                and self.max_points <= MAX_POINTS)

    def lift(self, depth, intrinsics, masks, mask_count=None, poses=None):
        """``depth`` float32 [F, H, W]; ``intrinsics`` float64 [F, 4] (fx, fy, cx, cy); ``masks`` bool or uint8 [F, M, H, W];
        ``mask_count`` [F] (default: M everywhere); ``poses`` float64 [F, 3, 4], current frame to reference frame (default: the
        identity).  On a GPU: launches on the current stream and no host synchronisation; beyond the kernel's limits, or on a CPU
        device, ``lift_host`` (``result.host``)."""
        F, M, H, W = _checked(depth, intrinsics, masks, mask_count, poses)
        kind = masks.dtype if isinstance(masks, torch.Tensor) else np.asarray(masks).dtype
        if kind not in (torch.bool, torch.uint8, np.dtype(bool), np.dtype(np.uint8)):
            raise ValueError("masks must be bool or uint8, got %s" % (kind,))
        if self.device.type != "cuda" or F == 0 or M == 0 or not self.within_limits(F, M, H, W):
            return lift_host(depth, intrinsics, masks, mask_count, poses, self.config, self.max_points)
        dev, c, Nmax = self.device, self.config, self.max_points
        put = lambda a, dtype: torch.as_tensor(a).to(device=dev, dtype=dtype).contiguous()
        depth, intrinsics = put(depth, torch.float32), put(intrinsics, torch.float64)
        masks = torch.as_tensor(masks).to(dev).contiguous()
        masks = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        mask_count = torch.full((F,), M, dtype=torch.int32, device=dev) if mask_count is None else put(mask_count, torch.int32)
        poses = None if poses is None else put(poses, torch.float64)
        empty = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        dist, sets = empty((F, M, H, W), torch.uint8), empty((F, M, H, W), torch.uint8)
        record = empty((F, M, RECORD_INTS), torch.int32)
        out = {"points": empty((F, M, Nmax, 3), torch.float32), "counts": empty((F, M), torch.int32), "total": empty((F, M), torch.int32),
               "centres": empty((F, M, 3), torch.float64), "range": empty((F, M), torch.float64),
               "truncated": empty((F, M), torch.uint8), "status": empty((F, M), torch.int32), "shrink": empty((F, M), torch.int32)}
        ptr = lambda t: t.data_ptr()
        with torch.cuda.device(dev):
            lib, stream = load(), torch.cuda.current_stream().cuda_stream
            run = lambda stages: lib.mono_lift_objects_f32(
                ptr(depth), ptr(intrinsics), ptr(masks), ptr(mask_count), None if poses is None else ptr(poses), F, M, H, W, Nmax, c.thr,
                c.d, int(c.use_range), c.max_range, stages, ptr(dist), ptr(sets), ptr(record), ptr(out["points"]), ptr(out["counts"]),
                ptr(out["total"]), ptr(out["centres"]), ptr(out["range"]), ptr(out["truncated"]), ptr(out["status"]), ptr(out["shrink"]),
                stream)
            if self.timing is None:
                _check(run(ALL_STAGES), "mono_lift_objects_f32")
            else:
                for name, stage in STAGES:
                    _check(_timed(self.timing, name, lambda: run(stage)), "mono_lift_objects_f32")
        result = LiftResult(c, False, **dict(out, truncated=out["truncated"].view(torch.bool)))
        result.timing = self.timing
        return result
