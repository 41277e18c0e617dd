"""Template fitting: the first 3D pseudo-label of an object from its aggregated point cloud (include/monosowa_fit.h has the rule).

    fitter = TemplateFitter(template, cfg=None, device=None)     template float [T, 3]; cfg with the reference's key names
    result = fitter.fit(clouds, centres=None, moving=None, theta=None, loc_only=None)       -> FitResult, tensors on the device
    result = fitter.fit_host(...)                                 the same contract in numpy float32 / float64 (a CPU device; the
                                                                  fallback beyond the kernel's limits: result.host says so)
    rows = result.rows(P2, img_size, boxes2d=None, cls_id=0)      float64 [n, 14] in decode_detections' column order
    template = sample_mesh(path, n=1000, seed=0, dims=(h, w, l), axes="xyz")

What it reproduces: the KITTI-frame behaviour of the reference's ``optimize_coarse`` -> ``optimize_fine``, ``optimize_moving`` and
``optimize_loc_only`` with ``loss_function: binary2way`` or ``binary1way`` -- a brute-force search over a grid of placements
(x offset, z offset, yaw), each scored by two counts: template points with a scan point within ``binary_loss_threshold`` and scan points
with a template point within it.  Stated deviations: the range search is exact (the reference asks an approximate IVF index with
``nprobe = 1``); the arithmetic is the float32 contract of the header; KITTI frame only.  The Waymo axis convention, the other five
losses, the scale detector and dimension estimation are refused with ``ValueError``.

Modes per object.  Static (default): the coarse grid, then 360 angles at the coarse winner's position.  ``moving[o]``: the ``dz`` range
shifted by +1; ``theta[o]`` alone when given, else the coarse angle list; no fine stage.  ``loc_only[o]``: the angles
``{theta[o], theta[o] + pi}``; no fine stage.  Objects are grouped by grid shape into as few launches as there are shapes.
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmonosowa_fit.so")
ABI_VERSION = 1
NULL, BAD_SIZE, TOO_LARGE = -1, -2, -3
MAX_T, MAX_N, MAX_H, MAX_B, MAX_DIM, MAX_TCELLS, MAX_CELLS = 2048, 65536, 1 << 20, 4096, 32, 4096, 32 * 32 * 32
OK, EMPTY = 0, 1
RESULT_INTS = 6
SLACK = np.float32(1.01)
FINE_ANGLES = 360
LOSSES = ("binary2way", "binary1way")
OTHER_LOSSES = ("medboth", "med1way", "diffbin", "chamfer", "trimmed")

FitConfig = collections.namedtuple("FitConfig", "x_min x_max x_iters z_min z_max z_iters theta_iters one_way r height width length")

_DEFAULTS = {
    "optimization": {"opt_param1_min": -2.0, "opt_param1_max": 2.0, "opt_param1_iters": 40, "opt_param2_min": -1.0,
                     "opt_param2_max": 3.0, "opt_param2_iters": 40, "opt_param3_iters": 40,
                     "use_dimensions_estimation_during_optim": False},
    "loss_functions": {"loss_function": "binary2way", "binary_loss_threshold": 0.2},
    "templates": {"template_height": 1.526, "template_width": 1.63, "template_length": 3.88},
    "scale_detector": {"use_scale_detector": False},
}


class Grid(ctypes.Structure):
    """``mono_fit_grid_t``."""
    _fields_ = [("origin", ctypes.c_float * 3), ("inv", ctypes.c_float * 3), ("dim", ctypes.c_int32 * 3), ("ncell", ctypes.c_int32)]


_lib = None


def load():
    """libmonosowa_fit.so; a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_PATH):
        raise RuntimeError("HIP extension %s is missing: build it with `python -m monosowa_amd.build`" % _PATH)
    lib = ctypes.CDLL(_PATH)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.mono_fit_abi_version.restype = I
    lib.mono_fit_grid_f32.restype = I
    lib.mono_fit_grid_f32.argtypes = [P, P, I, I, F, P, P, P, P, P, P]
    lib.mono_fit_search_f32.restype = I
    lib.mono_fit_search_f32.argtypes = [P, P, ctypes.POINTER(Grid), I, P, P, P, P, I, I, P, P, P, P, I, I, I, P, F, P, P]
    lib.mono_fit_reduce_f64.restype = I
    lib.mono_fit_reduce_f64.argtypes = [P, P, I, I, I, I, I, I, P, I, P, P, P]
    if lib.mono_fit_abi_version() != ABI_VERSION:
        raise RuntimeError("ABI version mismatch in %s" % _PATH)
    _lib = lib
    return lib


# ---------------------------------------------------------------------------------------------------------------- configuration
def _number(key, v, positive=False):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and not v > 0):
        raise ValueError("%s = %r is not a %sfinite number" % (key, v, "positive " if positive else ""))
    return float(v)


def _iters(key, v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError("%s = %r is not an integer >= 1" % (key, v))
    return v


def fit_config(cfg=None):
    """A dict with the reference's sections and key names -> a checked ``FitConfig``; absent keys take the reference's defaults, keys
    this module does not read are left alone, anything malformed or unsupported is a ValueError."""
    if cfg is None:
        cfg = {}
    if not isinstance(cfg, dict):
        raise ValueError("cfg = %r is not a mapping" % (cfg,))
    get = {}
    for section, keys in _DEFAULTS.items():
        given = cfg.get(section) or {}
        if not isinstance(given, dict):
            raise ValueError("%s = %r is not a mapping" % (section, given))
        for k, default in keys.items():
            get[k] = given.get(k, default)
    dataset = cfg.get("dataset")
    name = dataset.get("name", "kitti") if isinstance(dataset, dict) else ("kitti" if dataset is None else dataset)
    if name not in ("kitti", "all", "waymo_converted"):
        raise ValueError("dataset = %r: only the KITTI camera frame is built (the Waymo axis convention is not)" % (name,))
    loss = get["loss_function"]
    if loss not in LOSSES:
        raise ValueError("loss_functions.loss_function = %r: %s" % (
            loss, "only binary2way and binary1way are built" if loss in OTHER_LOSSES else "not a loss of the reference"))
    if get["use_scale_detector"] is not False:
        raise ValueError("scale_detector.use_scale_detector = %r: the scale detector is not built" % (get["use_scale_detector"],))
    if get["use_dimensions_estimation_during_optim"] is not False:
        raise ValueError("optimization.use_dimensions_estimation_during_optim = %r: dimension estimation is not built"
                         % (get["use_dimensions_estimation_during_optim"],))
    lim = [_number("optimization." + k, get[k]) for k in ("opt_param1_min", "opt_param1_max", "opt_param2_min", "opt_param2_max")]
    its = [_iters("optimization." + k, get[k]) for k in ("opt_param1_iters", "opt_param2_iters", "opt_param3_iters")]
    r = _number("loss_functions.binary_loss_threshold", get["binary_loss_threshold"], positive=True)
    with np.errstate(all="ignore"):
        r32 = np.float32(r)
        squared = bool(np.isfinite(r32) and r32 * r32 > 0 and np.isfinite(r32 * r32 * SLACK))
    if not squared:
        raise ValueError("loss_functions.binary_loss_threshold = %r has no float32 square" % (r,))
    dims = [_number("templates." + k, get[k], positive=True) for k in ("template_height", "template_width", "template_length")]
    return FitConfig(lim[0], lim[1], its[0], lim[2], lim[3], its[1], its[2], loss == "binary1way", r, *dims)


def coarse_angles(k):
    return np.linspace(0, 2 * np.pi - (2 * np.pi / k), num=k)


def wrap_ry(theta):
    """``theta - pi/2`` wrapped once into [-pi, pi] (the reference's output.py)."""
    yaw = np.asarray(theta, dtype=np.float64) - np.pi / 2.
    return np.where(yaw > np.pi, yaw - 2 * np.pi, np.where(yaw < -np.pi, yaw + 2 * np.pi, yaw))


# ---------------------------------------------------------------------------------------------------------------- the template's grid
def _axis_grid(lo, hi, hmin):
    """csrc/template_fit.hip: axis_grid, in float32."""
    with np.errstate(all="ignore"):
        ext = np.float32(hi) - np.float32(lo)
        if not np.isfinite(ext):
            return np.float32(-1.0), 1
        q = ext / hmin
        if q >= np.float32(MAX_DIM - 1):
            return np.float32(1.0) / max(hmin, ext / np.float32(MAX_DIM)), MAX_DIM
        return np.float32(1.0) / hmin, int(q) + 1


def build_grid(points, r):
    """The uniform grid of the header over float32 ``points`` [T, 3] -> (Grid, points ordered by cell then index, start int32
    [ncell + 1], the order).  Cells are ``1.01 r`` wide or wider; points that are not finite get the id ``ncell``."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    hmin = np.float32(r) * SLACK
    ok = np.isfinite(pts).all(axis=1)
    g = Grid()
    cells, dims = np.zeros((pts.shape[0], 3), dtype=np.int64), []
    with np.errstate(all="ignore"):
        for a in range(3):
            lo, hi = (pts[ok, a].min(), pts[ok, a].max()) if ok.any() else (np.float32(0), np.float32(0))
            inv, dim = _axis_grid(lo, hi, hmin)
            g.origin[a], g.inv[a], g.dim[a] = float(lo), float(inv), dim
            dims.append(dim)
            if inv >= 0:
                u = (pts[:, a] - np.float32(lo)) * np.float32(inv)
                cells[ok, a] = np.clip(np.where(u[ok] < dim, np.floor(u[ok]), dim - 1), 0, dim - 1).astype(np.int64)
    g.ncell = dims[0] * dims[1] * dims[2]
    ids = np.where(ok, (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0], g.ncell)
    order = np.argsort(ids, kind="stable")
    start = np.searchsorted(ids[order], np.arange(g.ncell + 1), side="left").astype(np.int32)
    return g, np.ascontiguousarray(pts[order]), start, order


# ---------------------------------------------------------------------------------------------------------------- the host routine
def placement_counts(tmpl, scan, tx, ty, tz, c, s, r2):
    """a(h), b(h) of one placement under the rule: float32 arrays ``tmpl`` [T, 3] and ``scan`` [N, 3], float32 scalars."""
    X, Y, Z = tmpl[:, 0], tmpl[:, 1], tmpl[:, 2]
    with np.errstate(all="ignore"):
        wx = (c * X + s * Z) + tx
        wy = Y + ty
        wz = (c * Z - s * X) + tz
        ex, ey, ez = scan[None, :, 0] - wx[:, None], scan[None, :, 1] - wy[:, None], scan[None, :, 2] - wz[:, None]
        a = int(((ex * ex + ey * ey) + ez * ez < r2).any(axis=1).sum())
        px, py, pz = scan[:, 0] - tx, scan[:, 1] - ty, scan[:, 2] - tz
        lx = c * px - s * pz
        lz = s * px + c * pz
        ex, ey, ez = lx[:, None] - X[None, :], py[:, None] - Y[None, :], lz[:, None] - Z[None, :]
        b = int(((ex * ex + ey * ey) + ez * ez < r2).any(axis=1).sum())
    return a, b


def search_host(tmpl, scan, tx, ty, tz, cs, r, one_way):
    """One object's search in the nested loop order: float32 lists ``tx`` [I], ``tz`` [J], ``cs`` [K, 2] and scalar ``ty`` ->
    (h, a, b, L, status, ab int32 [H, 2])."""
    T, N = tmpl.shape[0], scan.shape[0]
    I, J, K = len(tx), len(tz), len(cs)
    ab = np.zeros((I * J * K, 2), dtype=np.int32)
    if T == 0 or N == 0:
        return 0, 0, 0, 0.0, EMPTY, ab
    r2 = np.float32(r) * np.float32(r)
    best, at = np.inf, 0
    for i in range(I):
        for j in range(J):
            for k in range(K):
                h = (i * J + j) * K + k
                a, b = placement_counts(tmpl, scan, tx[i], ty, tz[j], cs[k, 0], cs[k, 1], r2)
                ab[h] = a, b
                L = -(np.float64(a) / np.float64(T)) if one_way else -(np.float64(a) / np.float64(T) + np.float64(b) / np.float64(N))
                if L < best:
                    best, at = L, h
    return at, int(ab[at, 0]), int(ab[at, 1]), float(best), OK, ab


# ---------------------------------------------------------------------------------------------------------------- results
class FitResult:
    """Per object: ``x, y, z, theta`` float64 (the template's centre and its rotation about y, from the float64 list values), ``a, b``
    int32, ``loss`` float64, ``h_coarse`` / ``h_fine`` int32 (flat placement indices; ``h_fine`` -1 without a fine stage), ``status``
    int32 (0, or 1 = EMPTY), ``score`` float64 in [0, 1].  ``host``: the fit went through ``fit_host``."""
    FIELDS = ("x", "y", "z", "theta", "a", "b", "loss", "h_coarse", "h_fine", "status", "score")

    def __init__(self, config, host, **fields):
        self.config, self.host = config, host
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    def __len__(self):
        return int(self.x.shape[0])

    def numpy(self):
        """The fields as numpy arrays (a synchronisation for a result on the GPU)."""
        return {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}

    def rows(self, P2, img_size, boxes2d=None, cls_id=0):
        """float64 ``[n, 14]`` rows (class, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score) for ``write_kitti_results``: ``ry =
        theta - pi/2`` wrapped once, ``y`` the box's bottom centre, the dimensions the configuration's.  ``boxes2d`` ``[n, 4]``: the
        caller's 2D boxes (a mask's); without, the hull of the eight projected corners clipped to the image (corners behind the camera
        take no part; none in front: an empty box at 0).  EMPTY objects give no row."""
        from .kitti_dataset import Calibration
        f = self.numpy()
        c = self.config
        P2 = np.asarray(P2, dtype=np.float64).reshape(3, 4)
        calib = Calibration({"P2": P2, "R0": np.eye(3), "Tr_velo2cam": np.zeros((3, 4))})
        W, H = float(img_size[0]), float(img_size[1])
        if boxes2d is not None:
            boxes2d = np.asarray(boxes2d, dtype=np.float64).reshape(-1, 4)
            if boxes2d.shape[0] != len(self):
                raise ValueError("boxes2d has %d rows for %d objects" % (boxes2d.shape[0], len(self)))
        ry = wrap_ry(f["theta"])
        out = []
        for o in range(len(self)):
            if f["status"][o] != OK:
                continue
            x, yb, z = f["x"][o], f["y"][o] + c.height / 2., f["z"][o]
            if boxes2d is not None:
                box = boxes2d[o]
            else:
                l2, w2 = c.length / 2., c.width / 2.
                cx = np.array([l2, l2, -l2, -l2, l2, l2, -l2, -l2])
                cy = np.array([0., 0., 0., 0., -c.height, -c.height, -c.height, -c.height])
                cz = np.array([w2, -w2, -w2, w2, w2, -w2, -w2, w2])
                co, si = np.cos(ry[o]), np.sin(ry[o])
                corners = np.stack([co * cx + si * cz + x, cy + yb, -si * cx + co * cz + z, np.ones(8)], axis=1)
                p = corners @ P2.T
                front = p[:, 2] > 0
                if front.any():
                    u, v = p[front, 0] / p[front, 2], p[front, 1] / p[front, 2]
                    box = np.array([np.clip(u.min(), 0, W - 1), np.clip(v.min(), 0, H - 1), np.clip(u.max(), 0, W - 1),
                                    np.clip(v.max(), 0, H - 1)])
                else:
                    box = np.zeros(4)
            alpha = calib.ry2alpha(ry[o], (box[0] + box[2]) / 2)
            out.append([cls_id, alpha, box[0], box[1], box[2], box[3], c.height, c.width, c.length, x, yb, z, ry[o], f["score"][o]])
        return np.asarray(out, dtype=np.float64).reshape(-1, 14)


_Group = collections.namedtuple("_Group", "objects dx dz theta fine")


class TemplateFitter:
    """``template``: float ``[T, 3]``, centred at the origin, width along x, height along y, length along z.  ``cfg``: see
    ``fit_config``.  ``device``: where ``fit`` runs (default: the current GPU when there is one, else the CPU, where ``fit`` is
    ``fit_host``)."""

    def __init__(self, template, cfg=None, device=None):
        self.config = fit_config(cfg)
        t = np.asarray(template)
        if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "fiu":
            raise ValueError("template must be a float array [T, 3], got %s %s" % (t.dtype, t.shape))
        self.template = np.ascontiguousarray(t, dtype=np.float32)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.device = torch.device(device)
        self.grid, self.sorted_template, self.start, _ = build_grid(self.template, self.config.r)
        self._dev = None
        self.timing = None          # a list: every stage of ``fit`` appends (name, start event, end event) to it (tools/template_fit_rate.py)

    def _timed(self, name, call):
        if self.timing is None:
            return call()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = call()
        end.record()
        self.timing.append((name, start, end))
        return out

    # ------------------------------------------------------------------------------------------------------------ inputs
    def _modes(self, B, moving, theta, loc_only):
        flag = lambda v, name: [False] * B if v is None else [bool(x) for x in _sized(v, B, name)]
        moving, loc_only = flag(moving, "moving"), flag(loc_only, "loc_only")
        theta = [None] * B if theta is None else [None if t is None else _number("theta[%d]" % o, float(t))
                                                  for o, t in enumerate(_sized(theta, B, "theta"))]
        c = self.config
        groups = collections.OrderedDict()
        for o in range(B):
            if moving[o] and loc_only[o]:
                raise ValueError("object %d is both moving and loc_only" % o)
            if loc_only[o] and theta[o] is None:
                raise ValueError("loc_only[%d] needs theta[%d]" % (o, o))
            shift = 1.0 if moving[o] else 0.0
            dz = np.linspace(c.z_min + shift, c.z_max + shift, num=c.z_iters)
            if loc_only[o]:
                th = np.array([theta[o], theta[o] + np.pi])
            elif moving[o] and theta[o] is not None:
                th = np.array([theta[o]], dtype=np.float64)
            else:
                th = coarse_angles(c.theta_iters)
            fine = not moving[o] and not loc_only[o]
            groups.setdefault((len(th), fine), []).append((o, dz, th))
        dx = np.linspace(c.x_min, c.x_max, num=c.x_iters)
        return [_Group([m[0] for m in members], dx, np.stack([m[1] for m in members]), np.stack([m[2] for m in members]), fine)
                for (_, fine), members in groups.items()]

    def _clouds_host(self, clouds, centres):
        """list of arrays -> (list of float32 [N_o, 3], centres float64 [B, 3])"""
        pts = []
        for o, cl in enumerate(clouds):
            a = cl.detach().cpu().numpy() if isinstance(cl, torch.Tensor) else np.asarray(cl)
            if a.size == 0:
                a = np.zeros((0, 3), dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "fiu":
                raise ValueError("clouds[%d] must be a float array [N, 3], got %s %s" % (o, a.dtype, a.shape))
            pts.append(np.ascontiguousarray(a, dtype=np.float32))
        if isinstance(centres, torch.Tensor):
            centres = centres.detach().cpu().numpy()
        if centres is None:
            with np.errstate(all="ignore"):
                centres = np.array([np.median(p.astype(np.float64), axis=0) if len(p) else np.zeros(3) for p in pts]).reshape(-1, 3)
        centres = np.asarray(centres, dtype=np.float64)
        if centres.shape != (len(pts), 3):
            raise ValueError("centres must be [%d, 3], got %s" % (len(pts), centres.shape))
        return pts, centres

    # ------------------------------------------------------------------------------------------------------------ host
    def fit_host(self, clouds, centres=None, moving=None, theta=None, loc_only=None):
        """``fit`` in numpy: float32 under the rule, losses and poses in float64.  CPU tensors out."""
        if isinstance(clouds, tuple):
            points, counts = clouds
            points, counts = points.detach().cpu().numpy(), np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts)
            clouds = [points[o, :max(0, min(int(counts[o]), points.shape[1]))] for o in range(points.shape[0])]
        pts, centres = self._clouds_host(clouds, centres)
        B, c = len(pts), self.config
        out = {"x": np.zeros(B), "y": np.zeros(B), "z": np.zeros(B), "theta": np.zeros(B), "a": np.zeros(B, np.int32),
               "b": np.zeros(B, np.int32), "loss": np.zeros(B), "h_coarse": np.zeros(B, np.int32), "h_fine": np.full(B, -1, np.int32),
               "status": np.zeros(B, np.int32)}
        fine_theta = coarse_angles(FINE_ANGLES)
        with np.errstate(all="ignore"):
            for g in self._modes(B, moving, theta, loc_only):
                J, K = g.dz.shape[1], g.theta.shape[1]
                for m, o in enumerate(g.objects):
                    ctr = centres[o]
                    tx, ty, tz = (g.dx + ctr[0]).astype(np.float32), np.float32(ctr[1]), (g.dz[m] + ctr[2]).astype(np.float32)
                    cs = np.stack([np.cos(g.theta[m]), np.sin(g.theta[m])], axis=1).astype(np.float32)
                    h, a, b, L, status, _ = search_host(self.template, pts[o], tx, ty, tz, cs, c.r, c.one_way)
                    i, j, k = h // (J * K), (h // K) % J, h % K
                    th = g.theta[m][k]
                    out["h_coarse"][o] = h
                    if g.fine and status == OK:
                        cs = np.stack([np.cos(fine_theta), np.sin(fine_theta)], axis=1).astype(np.float32)
                        hf, a, b, L, status, _ = search_host(self.template, pts[o], tx[i:i + 1], ty, tz[j:j + 1], cs, c.r, c.one_way)
                        out["h_fine"][o], th = hf, fine_theta[hf]
                    elif g.fine:
                        out["h_fine"][o] = 0
                    if status == OK:
                        pose = (g.dx[i] + ctr[0], ctr[1], g.dz[m][j] + ctr[2], th)
                    else:
                        pose = (ctr[0], ctr[1], ctr[2], 0.0)
                    out["x"][o], out["y"][o], out["z"][o], out["theta"][o] = pose
                    out["a"][o], out["b"][o], out["loss"][o], out["status"][o] = a, b, L, status
        out["score"] = -out["loss"] if c.one_way else -out["loss"] / 2
        return FitResult(c, True, **{k: torch.from_numpy(v) for k, v in out.items()})

    # ------------------------------------------------------------------------------------------------------------ device
    def _template_on_device(self):
        if self._dev is None:
            pts = self.sorted_template if self.sorted_template.size else np.zeros((1, 3), dtype=np.float32)
            self._dev = (torch.from_numpy(pts).to(self.device), torch.from_numpy(self.start).to(self.device))
        return self._dev

    def within_limits(self, n_max, groups):
        """Whether the kernels take this fit (include/monosowa_fit.h: Limits)."""
        c = self.config
        biggest = max([c.x_iters * c.z_iters * g.theta.shape[1] for g in groups] + [FINE_ANGLES])
        return (self.template.shape[0] <= MAX_T and self.grid.ncell <= MAX_TCELLS and n_max <= MAX_N and biggest <= MAX_H
                and max(len(g.objects) for g in groups) <= MAX_B)

    def fit(self, clouds, centres=None, moving=None, theta=None, loc_only=None):
        """``clouds``: a list of ``[N_o, 3]`` arrays, or ``(points [B, Nmax, 3] float32 tensor, counts int32 [B])``.  ``centres``
        float64 ``[B, 3]`` (default: the per-axis median of each cloud).  ``moving`` / ``loc_only``: per-object flags; ``theta``: per-object
        angles or None.  On a GPU: launches on the current stream and no host synchronisation; beyond the kernel's limits, or on a
        CPU device, ``fit_host`` (``result.host``)."""
        if self.device.type != "cuda":
            return self.fit_host(clouds, centres, moving, theta, loc_only)
        dev = self.device
        if isinstance(clouds, tuple):
            points, counts = clouds
            if not (isinstance(points, torch.Tensor) and points.dim() == 3 and points.shape[2] == 3 and points.dtype == torch.float32):
                raise ValueError("padded clouds must be a float32 tensor [B, Nmax, 3]")
            B = points.shape[0]
            counts = torch.as_tensor(counts, dtype=torch.int32).to(dev)
            if tuple(counts.shape) != (B,):
                raise ValueError("counts must be int32 [%d]" % B)
            points = points.to(dev)
            if centres is None:
                centres = _median_rows(points, counts)
        else:
            pts, centres = self._clouds_host(clouds, centres)
            B = len(pts)
            width = max([len(p) for p in pts] + [1])
            padded = np.zeros((B, width, 3), dtype=np.float32)
            for o, p in enumerate(pts):
                padded[o, :len(p)] = p
            points = torch.from_numpy(padded).to(dev)
            counts = torch.tensor([len(p) for p in pts], dtype=torch.int32).to(dev)
        centres = torch.as_tensor(centres, dtype=torch.float64).to(dev)
        if tuple(centres.shape) != (B, 3):
            raise ValueError("centres must be [%d, 3], got %s" % (B, tuple(centres.shape)))
        groups = self._modes(B, moving, theta, loc_only)
        if B == 0 or not self.within_limits(points.shape[1], groups):
            return self.fit_host((points, counts) if B else [], centres if B else None, moving, theta, loc_only)
        if points.shape[1] == 0:
            points = points.new_zeros((B, 1, 3))
        c = self.config
        f64 = lambda: torch.zeros(B, dtype=torch.float64, device=dev)
        i32 = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
        out = {"x": f64(), "y": f64(), "z": f64(), "theta": f64(), "a": i32(), "b": i32(), "loss": f64(), "h_coarse": i32(),
               "h_fine": i32(), "status": i32()}
        with torch.cuda.device(dev):
            for g in groups:
                self._fit_group(g, points, counts, centres, out)
        out["score"] = -out["loss"] if c.one_way else -out["loss"] / 2
        return FitResult(c, False, **out)

    def _fit_group(self, g, points, counts, centres, out):
        lib, dev, c = load(), self.device, self.config
        stream = torch.cuda.current_stream().cuda_stream
        whole = len(g.objects) == points.shape[0]
        idx = torch.tensor(g.objects, dtype=torch.int64).to(dev)
        pts = points.contiguous() if whole else points.index_select(0, idx).contiguous()
        cnt = counts.contiguous() if whole else counts.index_select(0, idx).contiguous()
        ctr = centres if whole else centres.index_select(0, idx)
        B, Nmax = pts.shape[0], pts.shape[1]
        I, J, K = len(g.dx), g.dz.shape[1], g.theta.shape[1]
        dx, dz, th = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (g.dx, g.dz, g.theta))
        tx = (dx[None, :] + ctr[:, 0:1]).float().contiguous()
        ty = ctr[:, 1].float().contiguous()
        tz = (dz + ctr[:, 2:3]).float().contiguous()
        cs = torch.from_numpy(np.stack([np.cos(g.theta), np.sin(g.theta)], axis=2).astype(np.float32)).to(dev)
        tmpl, tstart = self._template_on_device()
        T = self.template.shape[0]
        empty = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        grid, srt = empty((B, 10), torch.int32), empty((B, Nmax, 4), torch.float32)
        start, cell, scell = empty((B, MAX_CELLS + 1), torch.int32), empty((B, Nmax), torch.int32), empty((B, Nmax), torch.int32)
        _check(self._timed("grid", lambda: lib.mono_fit_grid_f32(
            pts.data_ptr(), cnt.data_ptr(), B, Nmax, c.r, grid.data_ptr(), srt.data_ptr(), start.data_ptr(), cell.data_ptr(),
            scell.data_ptr(), stream)), "mono_fit_grid_f32")

        def stage(cs_, K_, fix):
            H = K_ if fix is not None else I * J * K_
            ab, res, loss = empty((B, H, 2), torch.int32), empty((B, RESULT_INTS), torch.int32), empty((B,), torch.float64)
            fixp = None if fix is None else fix.data_ptr()
            which = "fine" if fix is not None else "coarse"
            _check(self._timed("search " + which, lambda: lib.mono_fit_search_f32(
                tmpl.data_ptr(), tstart.data_ptr(), ctypes.byref(self.grid), T, grid.data_ptr(), srt.data_ptr(), start.data_ptr(),
                cnt.data_ptr(), B, Nmax, tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), cs_.data_ptr(), I, J, K_, fixp, c.r, ab.data_ptr(),
                stream)), "mono_fit_search_f32")
            _check(self._timed("reduce " + which, lambda: lib.mono_fit_reduce_f64(
                ab.data_ptr(), cnt.data_ptr(), B, Nmax, T, I, J, K_, fixp, int(c.one_way), res.data_ptr(), loss.data_ptr(), stream)),
                "mono_fit_reduce_f64")
            return res, loss, ab
        res, loss, _ = stage(cs, K, None)
        h_coarse = res[:, 0]
        i, j = res[:, 4].long(), res[:, 5].long()
        theta = th.gather(1, (res[:, 0].long() % K)[:, None])[:, 0]
        h_fine = torch.full_like(h_coarse, -1)
        if g.fine:
            fine = coarse_angles(FINE_ANGLES)
            cs_f = torch.from_numpy(np.tile(np.stack([np.cos(fine), np.sin(fine)], axis=1).astype(np.float32), (B, 1, 1))).to(dev)
            res, loss, _ = stage(cs_f, FINE_ANGLES, res)
            h_fine = res[:, 0]
            theta = torch.from_numpy(fine).to(dev)[res[:, 0].long()]
        ok = res[:, 3] == OK
        x = torch.where(ok, dx[i] + ctr[:, 0], ctr[:, 0])
        z = torch.where(ok, dz.gather(1, j[:, None])[:, 0] + ctr[:, 2], ctr[:, 2])
        theta = torch.where(ok, theta, torch.zeros_like(theta))
        fields = {"x": x, "y": ctr[:, 1], "z": z, "theta": theta, "a": res[:, 1], "b": res[:, 2], "loss": loss, "h_coarse": h_coarse,
                  "h_fine": h_fine, "status": res[:, 3]}
        for k, v in fields.items():
            if whole:
                out[k] = v.contiguous()
            else:
                out[k].index_copy_(0, idx, v.contiguous())


def _check(code, what):
    if code:
        raise RuntimeError("%s failed with code %d" % (what, code))


def _sized(v, B, name):
    v = list(v)
    if len(v) != B:
        raise ValueError("%s has %d entries for %d objects" % (name, len(v), B))
    return v


def _median_rows(points, counts):
    """``np.median`` per axis of each object's first ``counts[o]`` points, in float64, on the device: [B, 3]."""
    B, N, _ = points.shape
    if N == 0:
        return torch.zeros((B, 3), dtype=torch.float64, device=points.device)
    n = counts.clamp(0, N).long()
    live = torch.arange(N, device=points.device)[None, :] < n[:, None]
    p = points.double()
    nan = (torch.isnan(p) & live[:, :, None]).any(dim=1)
    srt = torch.where(live[:, :, None], p, torch.full_like(p, float("inf"))).nan_to_num(nan=float("inf")).sort(dim=1).values
    lo, hi = ((n - 1).clamp(min=0) // 2), (n // 2).clamp(max=N - 1)
    take = lambda at: srt.gather(1, at[:, None, None].expand(B, 1, 3))[:, 0]
    med = (take(lo) + take(hi)) / 2
    med = torch.where(nan, torch.full_like(med, float("nan")), med)
    return torch.where((n == 0)[:, None], torch.zeros_like(med), med)


# ---------------------------------------------------------------------------------------------------------------- a template from a mesh
def sample_mesh(path, n=1000, seed=0, dims=(1.526, 1.63, 3.88), axes="xyz"):
    """``n`` area-weighted surface points of a Wavefront OBJ (``v`` / ``f`` lines; polygons fanned into triangles), float32 [n, 3]:
    the mesh centred on its axis-aligned bounding box and each axis scaled so that its extents are ``dims`` = (height, width,
    length) -- width along x, height along y, length along z.  ``axes``: which mesh axis becomes x, y, z, e.g. ``"xzy"``, a ``-``
    in front of a letter mirrors it.  Stated deviations: the reference centres on open3d's minimal oriented box and samples with
    open3d's generator; glTF is not read."""
    verts, tris = [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            parts = line.split("#")[0].split()
            if not parts or parts[0] not in ("v", "f"):
                continue
            try:
                if parts[0] == "v":
                    if len(parts) < 4:
                        raise ValueError("a vertex needs three coordinates")
                    verts.append([float(x) for x in parts[1:4]])
                else:
                    ids = [int(p.split("/")[0]) for p in parts[1:]]
                    if len(ids) < 3:
                        raise ValueError("a face needs three vertices")
                    ids = [i - 1 if i > 0 else len(verts) + i for i in ids]
                    if any(i < 0 or i >= len(verts) for i in ids):
                        raise ValueError("a face names a vertex that is not defined yet")
                    tris.extend([ids[0], ids[k], ids[k + 1]] for k in range(1, len(ids) - 1))
            except ValueError as e:
                raise ValueError("%s, line %d: %s (%r)" % (path, no, e, line.strip())) from None
    if not tris:
        raise ValueError("%s holds no face" % path)
    order, signs, letters = [], [], axes.replace("-", "")
    if sorted(letters) != ["x", "y", "z"]:
        raise ValueError("axes = %r is not a permutation of xyz" % (axes,))
    rest = axes
    for _ in range(3):
        sign = -1.0 if rest[0] == "-" else 1.0
        rest = rest[1:] if rest[0] == "-" else rest
        order.append("xyz".index(rest[0]))
        signs.append(sign)
        rest = rest[1:]
    v = np.asarray(verts, dtype=np.float64)[:, order] * np.asarray(signs)
    lo, hi = v.min(axis=0), v.max(axis=0)
    if not (hi > lo).all():
        raise ValueError("%s: the mesh is flat along an axis" % path)
    h, w, l = (float(d) for d in dims)
    v = (v - (lo + hi) / 2) * (np.array([w, h, l]) / (hi - lo))
    t = np.asarray(tris, dtype=np.int64)
    p0, p1, p2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    area = np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1) / 2
    if not area.sum() > 0:
        raise ValueError("%s: the mesh has no area" % path)
    rng = np.random.default_rng(seed)
    face = rng.choice(len(t), size=n, p=area / area.sum())
    u = rng.random((n, 2))
    flip = u.sum(axis=1) > 1
    u[flip] = 1 - u[flip]
    pts = p0[face] + u[:, 0:1] * (p1[face] - p0[face]) + u[:, 1:2] * (p2[face] - p0[face])
    return pts.astype(np.float32)
