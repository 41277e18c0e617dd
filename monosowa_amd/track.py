"""Object tracks: the centres of a lifted window to tracks, moving flags and headings (include/monosowa_track.h has the rule).

    tracker = ObjectTracker(cfg=None, device=None, max_tracks=None)     cfg with the reference's key names (``track_config``)
    tr = tracker.track(res)                                             res: a LiftResult, or a list of them with equal F, M
                                                                        -> TrackResult, tensors on the device, nothing waited for
    clouds, counts, centres = res.gather(*tr.gather_args())             rows of dropped tracks gather nothing
    kept, moving, theta = tr.objects()                                  the one call that waits for the device
    fit = fitter.fit((clouds[kept], counts[kept]), centres[kept], moving=moving, theta=theta)
    tr = track_host(centres, status, cfg, max_tracks)                   the same contract in numpy (a CPU result; the fallback beyond
                                                                        the kernel's limits: tr.host says so)

What it reproduces: the reference's ``perform_3D_tracking_kitti`` (its default tracker, ``tracker_for_merging: 3D``),
``decide_if_standing_or_moving_both5``, ``filter_moving_and_not_visible``, ``choose_proper_mask``, the pseudo-lidar branch of
``filter_hidden_standing_cars_tracked`` and ``estimate_angle_from_movement_tracked``.  Stated deviations: squared distances are
compared, not their roots; a non-finite centre is no detection; the z-score test is written without its division.  ICP, the 2D ODTrack
tracker and the merge of the two trackers are refused with ``ValueError``.
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch

from .lift import OK, MAX_M, MAX_VIEWS, LiftResult, _as_numpy, _check, _count, _flag, _timed

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmonosowa_track.so")
ABI_VERSION = 1
NULL, BAD_SIZE, TOO_LARGE = -1, -2, -3
MAX_TRACKS, MAX_WINDOWS = 896, 65536
Z0 = 0.2                            # the z-score the reference hard-codes
HALF_PI = math.pi / 2
STAGES = (("associate", 1), ("summary", 2))
ALL_STAGES = 3

TrackConfig = collections.namedtuple("TrackConfig", "d_track d_move d_angle z0 use_pseudo_lidar ref_frame")

_DEFAULTS = {
    "frames_creation": {"dist_treshold_tracking": 10.0, "dist_treshold_moving": 5.0, "nscans_before": 30, "use_pseudo_lidar": True,
                        "tracker_for_merging": "3D", "use_icp": False},
    "optimization": {"moving_cars_min_dist_for_angle": 3.0, "merge_two_trackers": False},
}

_lib = None


def load():
    """libmonosowa_track.so; a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_PATH):
        raise RuntimeError("HIP extension %s is missing: build it with `python -m monosowa_amd.build`" % _PATH)
    lib = ctypes.CDLL(_PATH)
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.mono_track_abi_version.restype = I
    lib.mono_track_objects_f64.restype = I
    lib.mono_track_objects_f64.argtypes = [P, P, I, I, I, I, D, D, D, D, I, I, I, P, P, P, P, P, P, P, P, P, P]
    if lib.mono_track_abi_version() != ABI_VERSION:
        raise RuntimeError("ABI version mismatch in %s" % _PATH)
    _lib = lib
    return lib


# ---------------------------------------------------------------------------------------------------------------- configuration
def _distance(key, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError("%s = %r is not a finite number >= 0" % (key, v))
    return float(v)


def track_config(cfg=None):
    """A dict with the reference's sections and key names -> a checked ``TrackConfig``; absent keys take the defaults of the reference's
    ``config.yaml``, keys this module does not read are left alone, anything malformed or unsupported is a ValueError."""
    if cfg is None:
        cfg = {}
    if isinstance(cfg, TrackConfig):
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
    tracker = get["tracker_for_merging"]
    if tracker not in ("2D", "3D"):
        raise ValueError("frames_creation.tracker_for_merging = %r is neither 2D nor 3D" % (tracker,))
    if tracker == "2D":
        raise ValueError("frames_creation.tracker_for_merging = 2D: the ODTrack 2D tracker is not built")
    if _flag("frames_creation.use_icp", get["use_icp"]):
        raise ValueError("frames_creation.use_icp = True: ICP pose refinement is not built")
    if _flag("optimization.merge_two_trackers", get["merge_two_trackers"]):
        raise ValueError("optimization.merge_two_trackers = True: there is one tracker to merge")
    return TrackConfig(_distance("frames_creation.dist_treshold_tracking", get["dist_treshold_tracking"]),
                       _distance("frames_creation.dist_treshold_moving", get["dist_treshold_moving"]),
                       _distance("optimization.moving_cars_min_dist_for_angle", get["moving_cars_min_dist_for_angle"]),
                       Z0, _flag("frames_creation.use_pseudo_lidar", get["use_pseudo_lidar"]),
                       _count("frames_creation.nscans_before", get["nscans_before"], 0))


def _max_tracks(v, F, M, limit=None):
    if v is None:
        return F * M if limit is None else min(F * M, limit)
    return _count("max_tracks", v, 1)


# ---------------------------------------------------------------------------------------------------------------- the host routine
def _square3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _first_least(q):
    """Rule 2's scan along the last axis: start at index 0, move on only when q < the best so far (numpy's argmin but for NaNs)."""
    least = np.where(np.isnan(q), np.inf, q).argmin(axis=-1)
    return np.where(np.isnan(q[..., 0]), 0, least)


def _predict(L):
    """the centres of a track, float64 [n, 3] in append order -> its prediction [3]"""
    n = L.shape[0]
    if n == 1:
        return L[0]
    k = min(n - 1, 4)
    total = L[n - 1] - L[n - 2]
    for j in range(2, k + 1):
        total = total + (L[n - j] - L[n - j - 1])
    return total / np.float64(k) + L[n - 1]


def _summary(L, r, c):
    """the centres of a track [n, 3] and the position of its reference view (or None) -> (moving, theta)"""
    n = L.shape[0]
    moving = False
    if n - 1 > 1:
        N = np.float64(n - 1)
        total = np.zeros(3)
        for k in range(n - 1):
            total = total + (L[k + 1] - L[k])
        mean = total / N
        total = np.zeros(3)
        for k in range(n - 1):
            e = (L[k + 1] - L[k]) - mean
            total = total + e * e
        var = total / N
        mm, vv, net2 = _square3(mean), (var[0] + var[1]) + var[2], _square3(L[n - 1] - L[0])
        z0, d_move = np.float64(c.z0), np.float64(c.d_move)
        moving = bool(mm > ((z0 * z0) * np.float64(0.5)) * vv and net2 > d_move * d_move)
    theta = np.nan
    if moving and r is not None and n >= 3:
        da2, angles = np.float64(c.d_angle) * np.float64(c.d_angle), []
        for walk, sign in ((range(r - 1, -1, -1), -1.0), (range(r + 1, n), 1.0)):
            taken = 0
            for i in walk:
                if taken == 5:
                    break
                dx, dz = (L[r, 0] - L[i, 0], L[r, 2] - L[i, 2]) if sign < 0 else (L[i, 0] - L[r, 0], L[i, 2] - L[r, 2])
                if dx * dx + dz * dz > da2:
                    angles.append(math.atan2(dz, dx))
                    taken += 1
        if len(angles) >= 3:
            if len(angles) % 2 == 0:
                angles.append(angles[-1])
            theta = (-sorted(angles)[len(angles) // 2]) + HALF_PI
    return moving, theta


def _track_window(centres, status, c, Tmax):
    F, M = status.shape
    out = {"tracks": np.full((Tmax, F, 2), -1, dtype=np.int32), "length": np.zeros(Tmax, dtype=np.int32),
           "ref_mask": np.full(Tmax, -1, dtype=np.int32), "moving": np.zeros(Tmax, dtype=bool), "visible": np.zeros(Tmax, dtype=bool),
           "keep": np.zeros(Tmax, dtype=bool), "theta": np.full(Tmax, np.nan)}
    views, dropped = [], 0                          # per track: its (frame, slot) pairs in append order
    dt2 = np.float64(c.d_track) * np.float64(c.d_track)
    for f in range(F):
        det = [m for m in range(M) if (status[f, m] & 7) == OK and np.isfinite(centres[f, m]).all()]
        if not det:
            continue
        z = centres[f, det]
        T = len(views)
        target = [None] * len(det)
        if T:
            pred = np.stack([_predict(np.stack([centres[v] for v in t[-5:]])) for t in views])
            q = _square3(z[:, None, :] - pred[None, :, :])
            a, b = _first_least(q), _first_least(q.T)
            target = [int(a[i]) if b[a[i]] == i and q[i, a[i]] < dt2 else None for i in range(len(det))]
        for i, m in enumerate(det):
            if target[i] is not None:
                views[target[i]].append((f, m))
            elif len(views) < Tmax:
                views.append([(f, m)])
            else:
                dropped += 1
    for t, row in enumerate(views):
        L = np.stack([centres[v] for v in row])
        at_ref = [i for i, (f, _) in enumerate(row) if f == c.ref_frame]
        r = at_ref[0] if at_ref else None
        moving, theta = _summary(L, r, c)
        for f, m in row:
            out["tracks"][t, f] = (f, m)
        out["length"][t], out["moving"][t], out["visible"][t], out["theta"][t] = len(row), moving, r is not None, theta
        out["ref_mask"][t] = -1 if r is None else row[r][1]
        out["keep"][t] = r is not None or (not c.use_pseudo_lidar and not moving)
    return out, len(views), dropped


def track_host(centres, status, cfg=None, max_tracks=None):
    """``ObjectTracker.track`` in numpy under the rule.  ``centres`` float64 [F, M, 3] or [S, F, M, 3], ``status`` int [F, M] or
    [S, F, M].  CPU tensors out."""
    c = track_config(cfg)
    centres, status = np.asarray(_as_numpy(centres), dtype=np.float64), np.asarray(_as_numpy(status))
    if status.dtype.kind not in "iu":
        raise ValueError("status must hold integers, got %s" % status.dtype)
    if status.ndim == 2:
        centres, status = centres[None], status[None]
    if status.ndim != 3 or centres.shape != status.shape + (3,) or status.shape[1] < 1 or status.shape[2] < 1:
        raise ValueError("centres must be [S, F, M, 3] and status [S, F, M], got %s and %s" % (centres.shape, status.shape))
    S, F, M = status.shape
    Tmax = _max_tracks(max_tracks, F, M)
    with np.errstate(all="ignore"):
        windows = [_track_window(centres[s], status[s].astype(np.int64), c, Tmax) for s in range(S)]
    fields = {k: torch.from_numpy(np.stack([w[0][k] for w in windows])) for k in windows[0][0]} if S else {
        "tracks": torch.zeros((0, Tmax, F, 2), dtype=torch.int32), "length": torch.zeros((0, Tmax), dtype=torch.int32),
        "ref_mask": torch.zeros((0, Tmax), dtype=torch.int32), "moving": torch.zeros((0, Tmax), dtype=torch.bool),
        "visible": torch.zeros((0, Tmax), dtype=torch.bool), "keep": torch.zeros((0, Tmax), dtype=torch.bool),
        "theta": torch.zeros((0, Tmax), dtype=torch.float64)}
    fields["count"] = torch.tensor([w[1] for w in windows], dtype=torch.int32)
    fields["dropped"] = torch.tensor([w[2] for w in windows], dtype=torch.int32)
    return TrackResult(c, True, **fields)


# ---------------------------------------------------------------------------------------------------------------- results
class TrackResult:
    """Per window s and track t < ``count[s]``: ``tracks`` int32 [S, Tmax, F, 2] (position f: (f, slot), or (-1, -1) without a view
    there), ``length`` int32, ``ref_mask`` int32 (the slot in the reference frame, -1: not visible), ``moving``, ``visible``, ``keep``
    bool, ``theta`` float64 (NaN: none), ``count`` and ``dropped`` int32 [S].  Rows at and beyond ``count``: -1, 0, false and NaN.
    ``host``: the tracks went through ``track_host``."""
    FIELDS = ("tracks", "length", "ref_mask", "moving", "visible", "keep", "theta", "count", "dropped")

    def __init__(self, config, host, **fields):
        self.config, self.host = config, host
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    def numpy(self):
        """The fields as numpy arrays (a synchronisation for a result on the GPU)."""
        return {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}

    def gather_args(self, s=0):
        """``(tracks[s], moving[s])``: what ``LiftResult.gather`` takes, where they are.  Every row below Tmax is gathered; a row
        beyond ``count`` gathers nothing."""
        return self.tracks[s], self.moving[s]

    def objects(self, s=0):
        """Waits for the device.  -> (the indices of the kept tracks, their ``moving`` as a list of bools, their ``theta`` as a list
        of floats or None): ``TemplateFitter.fit(..., moving=, theta=)`` groups objects by mode on the host."""
        keep, moving, theta = (getattr(self, k)[s].cpu().numpy() for k in ("keep", "moving", "theta"))
        kept = np.flatnonzero(keep).tolist()
        return kept, [bool(moving[t]) for t in kept], [None if math.isnan(theta[t]) else float(theta[t]) for t in kept]


class ObjectTracker:
    """``cfg``: see ``track_config``.  ``device``: where ``track`` runs (default: where the lift's result lives).  ``max_tracks``: Tmax,
    the rows per window (default: min(F * M, the kernel's limit), so that nothing is dropped within the limit).  Without
    ``max_tracks``, windows with F * M > 896 differ by path: the kernels run with Tmax = 896 and count what they drop in ``dropped``,
    while ``track_host`` -- taken for a CPU result, a missing library, or F or M beyond the limits -- runs with Tmax = F * M and
    drops nothing, so the shape of the result and ``dropped`` say which path ran (as ``result.host`` does).  Give ``max_tracks`` to
    have the same Tmax on both."""

    def __init__(self, cfg=None, device=None, max_tracks=None):
        self.config = track_config(cfg)
        self.max_tracks = None if max_tracks is None else _count("max_tracks", max_tracks, 1)
        self.device = None if device is None else torch.device(device)
        self.timing = None          # a list: every stage appends (name, start event, end event) to it (tools/track_rate.py)

    def within_limits(self, S, F, M, Tmax):
        """Whether the kernels take these windows (include/monosowa_track.h: Limits)."""
        return S <= MAX_WINDOWS and F <= MAX_VIEWS and M <= MAX_M and Tmax <= MAX_TRACKS

    def track(self, result):
        """``result``: a LiftResult or a list of them with equal F and M (S windows, one launch).  On a GPU: launches on the current
        stream and no host synchronisation; beyond the kernel's limits, for a CPU result or without the library, ``track_host``
        (``result.host``)."""
        windows = [result] if isinstance(result, LiftResult) else list(result)
        if not windows or not all(isinstance(w, LiftResult) for w in windows):
            raise ValueError("track takes a LiftResult or a non-empty list of them")
        shape = tuple(windows[0].status.shape)
        if any(tuple(w.status.shape) != shape for w in windows):
            raise ValueError("the windows differ in F x M: %s" % ([tuple(w.status.shape) for w in windows],))
        (F, M), S, c = shape, len(windows), self.config
        dev = windows[0].centres.device if self.device is None else self.device
        on_gpu = dev.type == "cuda" and all(w.centres.is_cuda for w in windows) and F >= 1 and M >= 1
        Tmax = _max_tracks(self.max_tracks, F, M, MAX_TRACKS if on_gpu else None)
        if not on_gpu or not self.within_limits(S, F, M, Tmax) or not os.path.exists(_PATH):
            return track_host(np.stack([_as_numpy(w.centres) for w in windows]), np.stack([_as_numpy(w.status) for w in windows]),
                              c, _max_tracks(self.max_tracks, F, M))
        put = lambda ts, dtype: (ts[0][None] if S == 1 else torch.stack(ts)).to(device=dev, dtype=dtype).contiguous()
        centres, status = put([w.centres for w in windows], torch.float64), put([w.status for w in windows], torch.int32)
        empty = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        out = {"tracks": empty((S, Tmax, F, 2), torch.int32), "length": empty((S, Tmax), torch.int32),
               "ref_mask": empty((S, Tmax), torch.int32), "moving": empty((S, Tmax), torch.uint8), "visible": empty((S, Tmax), torch.uint8),
               "keep": empty((S, Tmax), torch.uint8), "theta": empty((S, Tmax), torch.float64), "count": empty((S,), torch.int32),
               "dropped": empty((S,), torch.int32)}
        ptr = lambda t: t.data_ptr()
        with torch.cuda.device(dev):
            lib, stream = load(), torch.cuda.current_stream().cuda_stream
            run = lambda stages: lib.mono_track_objects_f64(
                ptr(centres), ptr(status), S, F, M, c.ref_frame, c.d_track, c.d_move, c.d_angle, c.z0, int(c.use_pseudo_lidar), Tmax,
                stages, *(ptr(out[k]) for k in TrackResult.FIELDS), stream)
            if self.timing is None:
                _check(run(ALL_STAGES), "mono_track_objects_f64")
            else:
                for name, stage in STAGES:
                    _check(_timed(self.timing, name, lambda: run(stage)), "mono_track_objects_f64")
        for k in ("moving", "visible", "keep"):
            out[k] = out[k].view(torch.bool)
        return TrackResult(c, False, **out)
