"""An independent restatement of the template-pose search (include/monosowa_fit.h; the reference's optimizer.py:53-155, 293-345,
426-488 and loss.py:61-75), and the generator of the inputs the CPU and GPU tests share.

(i)  ``counts_f32`` / ``search_f32`` / ``fit_f32``: the rule's float32 arithmetic, carried out in float64 with a rounding to float32
     after every single operation.  A product of two float32 numbers is exact in float64, and a float64 sum of two float32 numbers
     rounds to float32 like the float32 sum (53 >= 2 * 24 + 2 bits), so this is float32 with every operation rounded on its own and
     nothing contracted -- by another route than numpy's float32 loops.  ``counts_scalar`` is the same in plain scalar loops.
(ii) ``search_f64``: float64 with scipy's Rotation and ``cdist`` in the reference's loop order and strict ``<``, no float32 anywhere.
"""
import numpy as np
from scipy.spatial.distance import cdist
from scipy.spatial.transform import Rotation

DIMS = (1.526, 1.63, 3.88)          # template height, width, length
R_THRESHOLD = 0.2
GRID = {"opt_param1_min": -2.0, "opt_param1_max": 2.0, "opt_param1_iters": 6, "opt_param2_min": -1.0, "opt_param2_max": 3.0,
        "opt_param2_iters": 6, "opt_param3_iters": 12}
CFG = {"optimization": GRID, "loss_functions": {"loss_function": "binary2way", "binary_loss_threshold": R_THRESHOLD}}
PLACES = ((0.0, 0.0, 0.0), (8.0, 1.6, 40.0), (-20.0, 1.6, 60.0))
MARGIN = 1e-3                        # a placement with a pair inside |d^2 - r^2| < MARGIN r^2 is not compared between (i) and (ii)


def r32(x):
    """Rounds float64 values to float32 and back."""
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def angles(k):
    return np.linspace(0, 2 * np.pi - (2 * np.pi / k), num=k)


# ---------------------------------------------------------------------------------------------------------------- (i) float32
def host_lists(centre, dx, dz, theta):
    """The float32 numbers the kernels see (as float64 values): tx [I], ty, tz [J], cos [K], sin [K]."""
    c = np.asarray(centre, dtype=np.float64)
    return r32(np.asarray(dx) + c[0]), float(r32(c[1])), r32(np.asarray(dz) + c[2]), r32(np.cos(theta)), r32(np.sin(theta))


def counts_f32(tmpl, scan, tx, ty, tz, c, s, r2):
    t, p = np.asarray(tmpl, dtype=np.float64), np.asarray(scan, dtype=np.float64)
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    with np.errstate(all="ignore"):
        wx = r32(r32(r32(c * x) + r32(s * z)) + tx)
        wy = r32(y + ty)
        wz = r32(r32(r32(c * z) - r32(s * x)) + tz)
        ex, ey, ez = r32(p[None, :, 0] - wx[:, None]), r32(p[None, :, 1] - wy[:, None]), r32(p[None, :, 2] - wz[:, None])
        d = r32(r32(r32(ex * ex) + r32(ey * ey)) + r32(ez * ez))
        a = int((d < r2).any(axis=1).sum())
        px, py, pz = r32(p[:, 0] - tx), r32(p[:, 1] - ty), r32(p[:, 2] - tz)
        lx = r32(r32(c * px) - r32(s * pz))
        lz = r32(r32(s * px) + r32(c * pz))
        ex, ey, ez = r32(lx[:, None] - x[None, :]), r32(py[:, None] - y[None, :]), r32(lz[:, None] - z[None, :])
        d = r32(r32(r32(ex * ex) + r32(ey * ey)) + r32(ez * ez))
        b = int((d < r2).any(axis=1).sum())
    return a, b


def counts_scalar(tmpl, scan, tx, ty, tz, c, s, r2):
    """The same two counts, one np.float32 scalar operation at a time."""
    f = np.float32
    tx, ty, tz, c, s, r2 = f(tx), f(ty), f(tz), f(c), f(s), f(r2)
    a = b = 0
    with np.errstate(all="ignore"):
        for x, y, z in np.asarray(tmpl, dtype=np.float32):
            wx, wy, wz = (c * x + s * z) + tx, y + ty, (c * z - s * x) + tz
            for p in np.asarray(scan, dtype=np.float32):
                ex, ey, ez = p[0] - wx, p[1] - wy, p[2] - wz
                if (ex * ex + ey * ey) + ez * ez < r2:
                    a += 1
                    break
        for p in np.asarray(scan, dtype=np.float32):
            px, py, pz = p[0] - tx, p[1] - ty, p[2] - tz
            lx, ly, lz = c * px - s * pz, py, s * px + c * pz
            for x, y, z in np.asarray(tmpl, dtype=np.float32):
                ex, ey, ez = lx - x, ly - y, lz - z
                if (ex * ex + ey * ey) + ez * ez < r2:
                    b += 1
                    break
    return a, b


def loss_of(a, b, T, N, one_way):
    return -(float(a) / T) if one_way else -(float(a) / T + float(b) / N)


def search_f32(tmpl, scan, centre, dx, dz, theta, r=R_THRESHOLD, one_way=False):
    """-> (h, a, b, L, ab int [H, 2]): the first minimum in the nested loop order."""
    T, N = len(tmpl), len(scan)
    tx, ty, tz, co, si = host_lists(centre, dx, dz, theta)
    r2 = float(r32(r32(r) * r32(r)))
    ab = np.zeros((len(tx) * len(tz) * len(co), 2), dtype=np.int64)
    best, at, h = np.inf, 0, 0
    for i in range(len(tx)):
        for j in range(len(tz)):
            for k in range(len(co)):
                ab[h] = counts_f32(tmpl, scan, tx[i], ty, tz[j], co[k], si[k], r2)
                L = loss_of(ab[h, 0], ab[h, 1], T, N, one_way)
                if L < best:
                    best, at = L, h
                h += 1
    return at, int(ab[at, 0]), int(ab[at, 1]), best, ab


def fit_f32(tmpl, clouds, centres=None, moving=None, theta=None, loc_only=None, grid=GRID, r=R_THRESHOLD, one_way=False):
    """The whole fit per object -> dict of arrays named like ``FitResult``'s fields."""
    B = len(clouds)
    names = ("x", "y", "z", "theta", "loss", "score")
    out = {k: np.zeros(B) for k in names}
    out.update({k: np.zeros(B, dtype=np.int32) for k in ("a", "b", "h_coarse", "h_fine", "status")})
    for o, scan in enumerate(clouds):
        scan = np.asarray(scan, dtype=np.float32).reshape(-1, 3)
        if centres is not None:
            c = np.asarray(centres[o], dtype=np.float64)
        else:
            c = np.median(scan.astype(np.float64), axis=0) if len(scan) else np.zeros(3)
        mov, loc = bool(moving[o]) if moving is not None else False, bool(loc_only[o]) if loc_only is not None else False
        th = theta[o] if theta is not None else None
        dx = np.linspace(grid["opt_param1_min"], grid["opt_param1_max"], num=grid["opt_param1_iters"])
        dz = np.linspace(grid["opt_param2_min"] + (1. if mov else 0.), grid["opt_param2_max"] + (1. if mov else 0.), num=grid["opt_param2_iters"])
        if loc:
            ths = [th, th + np.pi]
        elif mov and th is not None:
            ths = [th]
        else:
            ths = angles(grid["opt_param3_iters"])
        out["h_fine"][o] = -1
        if len(scan) == 0 or len(tmpl) == 0:
            out["x"][o], out["y"][o], out["z"][o] = c
            out["status"][o] = 1
            if not mov and not loc:
                out["h_fine"][o] = 0
            continue
        h, a, b, L, _ = search_f32(tmpl, scan, c, dx, dz, ths, r, one_way)
        K = len(ths)
        i, j, k = h // (len(dz) * K), (h // K) % len(dz), h % K
        angle = ths[k]
        out["h_coarse"][o] = h
        if not mov and not loc:
            fine = np.linspace(0, 2 * np.pi - (2 * np.pi / 360), num=360)
            hf, a, b, L, _ = search_f32(tmpl, scan, c, dx[i:i + 1], dz[j:j + 1], fine, r, one_way)
            out["h_fine"][o], angle = hf, fine[hf]
        out["x"][o], out["y"][o], out["z"][o], out["theta"][o] = dx[i] + c[0], c[1], dz[j] + c[2], angle
        out["a"][o], out["b"][o], out["loss"][o] = a, b, L
    out["score"] = -out["loss"] if one_way else -out["loss"] / 2
    return out


# ---------------------------------------------------------------------------------------------------------------- (ii) float64
def search_f64(tmpl, scan, centre, dx, dz, theta, r=R_THRESHOLD, one_way=False, margin=MARGIN):
    """The reference's loop in float64 -> (h, L, ab int [H, 2], near bool [H]: a pair lies within ``margin`` r^2 of the threshold)."""
    t, p, c = np.asarray(tmpl, dtype=np.float64), np.asarray(scan, dtype=np.float64), np.asarray(centre, dtype=np.float64)
    H = len(dx) * len(dz) * len(theta)
    ab, near = np.zeros((H, 2), dtype=np.int64), np.zeros(H, dtype=bool)
    best, at, h = np.inf, 0, 0
    for p1 in dx:
        for p2 in dz:
            for p3 in theta:
                rot = Rotation.from_euler("zyx", [0, p3, 0], degrees=False)
                placed = np.matmul(rot.as_matrix(), t.T).T
                placed[:, 0] += p1 + c[0]
                placed[:, 1] += c[1]
                placed[:, 2] += p2 + c[2]
                d = cdist(p, placed, "sqeuclidean")
                ab[h] = np.sum(np.min(d, axis=0) < r ** 2), np.sum(np.min(d, axis=1) < r ** 2)
                near[h] = bool((np.abs(d - r ** 2) < margin * r ** 2).any())
                loss = loss_of(ab[h, 0], ab[h, 1], t.shape[0], p.shape[0], one_way)
                if loss < best:
                    best, at = loss, h
                h += 1
    return at, best, ab, near


# ---------------------------------------------------------------------------------------------------------------- the generator
def box_template(T, seed):
    """``T`` points on the surface of the template box (width x, height y, length z), float32."""
    rng = np.random.default_rng(seed)
    h, w, l = DIMS
    half = np.array([w / 2, h / 2, l / 2])
    pts = rng.uniform(-1, 1, (T, 3)) * half
    axis = rng.integers(0, 3, T)
    pts[np.arange(T), axis] = np.where(rng.random(T) < 0.5, -1, 1) * half[axis]
    return pts.astype(np.float32)


def noisy_copy(tmpl, N, pose, seed, sigma=0.02):
    """``N`` template points (drawn with replacement) rotated about y by pose[3], moved to pose[:3], with Gaussian noise."""
    rng = np.random.default_rng(seed)
    t = np.asarray(tmpl, dtype=np.float64)[rng.integers(0, len(tmpl), N)]
    c, s = np.cos(pose[3]), np.sin(pose[3])
    pts = np.stack([c * t[:, 0] + s * t[:, 2] + pose[0], t[:, 1] + pose[1], c * t[:, 2] - s * t[:, 0] + pose[2]], axis=1)
    return (pts + rng.normal(0, sigma, pts.shape)).astype(np.float32)


def poses(n, seed):
    """``n`` poses inside the search range around PLACES, cycled."""
    rng = np.random.default_rng(seed)
    out = []
    for o in range(n):
        px, py, pz = PLACES[o % len(PLACES)]
        out.append((px + rng.uniform(-1.2, 1.2), py, pz + rng.uniform(-0.2, 2.2), rng.uniform(0, 2 * np.pi)))
    return out


def batch(T, sizes=(160, 130, 1, 0, 64), seed=0):
    """-> (template [T, 3], list of clouds with ``sizes`` points, centres [B, 3]): noisy rotated copies, the centre the place itself
    (a fixed number, so that the pose's offset lies inside the grid)."""
    tmpl = box_template(T, seed + 100 * T)
    ps = poses(len(sizes), seed + 1)
    clouds = [noisy_copy(tmpl, n, ps[o], seed + 10 + o) for o, n in enumerate(sizes)]
    centres = np.array([PLACES[o % len(PLACES)] for o in range(len(sizes))], dtype=np.float64)
    return tmpl, clouds, centres


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same(got, want, what=""):
    """Every field of a fit: floats by their bits."""
    assert set(got) == set(want)
    for k in want:
        if want[k].dtype == np.float64:
            assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, got[k].tolist(), want[k].tolist())
        else:
            assert np.array_equal(got[k], want[k]), (what, k, got[k].tolist(), want[k].tolist())
