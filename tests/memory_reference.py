"""Helpers of test_teacher_memory_cpu.py / test_teacher_memory_gpu.py (no tests in here): an independent restatement of the label
memory's rule (include/monosowa_kitti.h, mono_memory_merge_f64) in scalar Python floats -- IEEE doubles, one rounding per operation,
no fused multiply-add -- with the overlaps from the float64 oracle tests/fuse_reference.py uses, and the seeded generator of the
passes both tests merge."""
import math

import numpy as np

import fuse_reference as F

MARGIN = F.MARGIN          # every same-class (row, entry) pair is bit-coincident or further than this from the threshold
BEV = F.BEV
MOMENTUM, IOU, DROP = 0.5, 0.5, 0.2


def bits(a):
    """float64 array -> its int64 view (a copy): what 'byte for byte' compares."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64).copy()


def _rect(row):
    with np.errstate(over="ignore"):
        return [float(np.float32(row[c])) for c in BEV]


def overlap(a, b):
    """(coincident, IoU) of two float32 rectangles: by the rule a rectangle with a side that is not > 0 overlaps nothing (0.0), five
    equal finite numbers overlap by 1.0 without a routine, everything else is the float64 oracle's IoU."""
    if not (a[2] > 0 and a[3] > 0 and b[2] > 0 and b[3] > 0):
        return False, 0.0
    if all(math.isfinite(v) for v in a + b) and a == b:
        return True, 1.0
    if not all(math.isfinite(v) for v in a + b):
        return False, float("nan")
    if math.hypot(a[0] - b[0], a[1] - b[1]) > (math.hypot(a[2], a[3]) + math.hypot(b[2], b[3])) / 2:
        return False, 0.0                                     # centres further apart than the half-diagonals: disjoint
    return False, float(F.R.rotate_iou(np.array([a]), np.array([b]), -1)[0, 0])


def merge(rows, count, frame, bank, bank_count, momentum=MOMENTUM, iou=IOU, drop_below=DROP):
    """The rule on lists of Python floats.  ``bank`` [N, M, 16] / ``bank_count`` [N] are updated in place ->
    (out_rows [B, M, 14], out_count int32 [B], stats int32 [B, 6], pairs): pairs = (coincident, IoU) of EVERY same-class
    (row, entry) pair of the call, eligible or not, walked or not."""
    B, R = rows.shape[0], rows.shape[1]
    N, M = bank.shape[0], bank.shape[1]
    out_rows, out_count, stats = np.zeros((B, M, 14)), np.zeros(B, dtype=np.int32), np.zeros((B, 6), dtype=np.int32)
    w = 1.0 - float(momentum)
    threshold = np.float32(iou)
    pairs = []
    for b in range(B):
        f = int(frame[b])
        if not 0 <= f < N:
            continue
        n = max(0, min(int(count[b]), R))
        k = max(0, min(int(bank_count[f]), M))
        new = [[float(v) for v in rows[b, i]] for i in range(n)]
        old = [[float(v) for v in bank[f, e]] for e in range(k)]
        flags = [[False] * k for _ in range(n)]
        for i in range(n):
            for e in range(k):
                if new[i][0] == old[e][0]:
                    coincident, value = overlap(_rect(new[i]), _rect(old[e]))
                    pairs.append((coincident, value))
                    flags[i][e] = math.isfinite(new[i][13]) and (coincident or bool(np.float32(value) >= threshold))
        claimed_by, created, skipped = {}, [], 0
        for i in range(n):
            if not math.isfinite(new[i][13]):
                skipped += 1
                continue
            free = [e for e in range(k) if flags[i][e] and e not in claimed_by]
            if free:
                claimed_by[free[0]] = i
            else:
                created.append(i)
        cands = []                                            # (smoothed score, where it came from, the 16 values)
        for e in range(k):
            s = old[e][13]
            if e in claimed_by:
                r = new[claimed_by[e]]
                d = r[13] - s
                t = w * d
                entry = r[:13] + [s + t, old[e][14] + 1.0, 0.0]
            else:
                d = 0.0 - s
                t = w * d
                entry = old[e][:13] + [s + t, old[e][14], old[e][15] + 1.0]
            cands.append(entry)
        for i in created:
            cands.append(new[i][:14] + [1.0, 0.0])
        alive = [j for j, c in enumerate(cands) if c[13] >= drop_below]
        ranked = [None] * len(alive)
        for j in alive:                                       # rank by counting, ties to the lower candidate index
            rank = sum(1 for q in alive if cands[q][13] > cands[j][13] or (cands[q][13] == cands[j][13] and q < j))
            ranked[rank] = j
        kept = ranked[:M]
        bank[f] = 0.0
        for r, j in enumerate(kept):
            bank[f, r] = np.array(cands[j], dtype=np.float64)      # float() and back keep every bit
            out_rows[b, r] = bank[f, r, :14]
        bank_count[f] = out_count[b] = len(kept)
        stats[b] = (len(claimed_by), len(created), k - len(claimed_by), len(cands) - len(alive), len(alive) - len(kept), skipped)
    return out_rows, out_count, stats, pairs


# ------------------------------------------------------------------------------------------------ generated passes
def _row(rng, cls, x, z, l, w, ry, score):
    x1 = 600.0 + 700.0 * x / z
    return [float(cls), ry - math.atan2(x, z), x1 - 40.0, rng.uniform(120, 170), x1 + 40.0, rng.uniform(190, 300), rng.uniform(1.4, 1.7),
            w, l, x, rng.uniform(1.4, 1.8), z, ry, score]


def _object(rng, j):
    """Object j of a frame: 20 m from every other one, class j mod 3."""
    return _row(rng, j % 3, -30.0 + 20.0 * (j % 4) + rng.uniform(-1, 1), 15.0 + 25.0 * (j // 4) + rng.uniform(-1, 1),
                rng.uniform(3.6, 4.4), rng.uniform(1.6, 1.9), rng.uniform(-3, 3), 0.0)


def _seen(rng, base, score, jitter=True):
    """A later look at the same object: a few centimetres and a hundredth of a radian off (IoU about 0.9), or the very row."""
    r = list(base)
    if jitter:
        r[9] += rng.uniform(-0.04, 0.04)
        r[11] += rng.uniform(-0.04, 0.04)
        r[8] *= rng.uniform(0.99, 1.01)
        r[7] *= rng.uniform(0.99, 1.01)
        r[12] += rng.uniform(-0.01, 0.01)
    r[13] = score
    return r


def _partial(base, score):
    """The same class two thirds of a length further along the object's axis: IoU (l - s) / (l + s) = 0.2 with the object."""
    r = list(base)
    s = r[8] * 2.0 / 3.0
    r[9], r[11], r[13] = r[9] + s * math.cos(r[12]), r[11] - s * math.sin(r[12]), score
    return r


def _pack(images, R):
    rows = np.zeros((len(images), R, 14))
    for b, items in enumerate(images):
        assert len(items) <= R
        for i, r in enumerate(items):
            rows[b, i] = r
    return rows


def small_passes(seed=0):
    """B = 4, N = 6, M = 4, R = 8, three passes -> (bank0 [6, 4, 16], bank_count0 [6], [(rows, count, frame) x 3]).  The families:
    empty bank, all matched, all missed, survivors above M, decay below drop_below, NaN / +Inf / -Inf scores, a box with a zero
    side, bit-identical duplicate rows, equal boxes of different classes, count above R and negative, bank_count -1 and M + 3."""
    rng = np.random.default_rng(seed)
    M, R, N = 4, 8, 6
    objs = [[_object(rng, j) for j in range(8)] for _ in range(N)]
    bank, bank_count = np.zeros((N, M, 16)), np.zeros(N, dtype=np.int32)
    # hostile counts: frame 5 says -1 (and holds rubbish that must not be read as entries), frame 3 says M + 3 over M real entries
    bank_count[5], bank_count[3] = -1, M + 3
    bank[5, :, :] = 7.25
    for e in range(M):
        bank[3, e, :14] = _seen(rng, objs[3][e], [0.8, 0.6, 0.45, 0.3][e], jitter=False)
        bank[3, e, 14:] = (3.0, float(e % 2))
    o = objs
    p1 = [
        [_seen(rng, o[2][0], 0.9), _seen(rng, o[2][1], 0.7), _seen(rng, o[2][2], 0.3)],                       # image 0, frame 2: empty bank
        [_seen(rng, o[0][j], 0.95 - 0.1 * j) for j in range(6)],                                              # image 1, frame 0: 6 > M
        [],                                                                                                   # image 2, frame 5: below
        [_seen(rng, o[3][0], 0.5), _seen(rng, o[3][2], 0.9), _partial(o[3][1], 0.55)],                        # image 3, frame 3: M + 3
    ]
    flat = _seen(rng, o[5][0], 0.8)
    flat[7] = 0.0                                                                                             # a zero side
    twin = _seen(rng, o[5][1], 0.6)
    other = list(twin)
    other[0], other[13] = (twin[0] + 1) % 3, 0.5                                                              # equal box, other class
    p1[2] = [flat, twin, list(twin), other]
    p2 = [
        [_seen(rng, o[2][0], 0.5), _seen(rng, o[2][1], 0.8), _seen(rng, o[2][2], 0.35), _partial(o[2][0], 0.6)],     # all matched + one
        [_seen(rng, o[0][0], float("nan")), _seen(rng, o[0][1], float("inf")), _seen(rng, o[0][2], float("-inf")),
         _seen(rng, o[0][3], 0.4), _seen(rng, o[0][6], 0.99), _seen(rng, o[0][7], 0.1), _seen(rng, o[0][0], 0.7),
         _seen(rng, o[0][0], 0.65)],                                                                          # count says R + 5
        [list(flat), list(twin), list(twin), list(other)],                                                    # the very rows again
        [_seen(rng, o[1][j], 0.3 + 0.1 * j) for j in range(3)],                                               # frame 1: empty bank
    ]
    p3 = [
        [],                                                                                                   # all missed
        [_seen(rng, o[0][j], 0.5) for j in range(4)],                                                         # count says -2
        [_seen(rng, o[5][1], 0.9), _seen(rng, o[5][2], 0.21)],
        [_seen(rng, o[3][0], 0.25), _seen(rng, o[3][1], 0.6), _seen(rng, o[3][3], 0.7)],                      # frame 3 again
    ]
    counts = [np.array([3, 6, 4, 3], dtype=np.int32), np.array([4, R + 5, 4, 3], dtype=np.int32), np.array([0, -2, 2, 3], dtype=np.int32)]
    frames = [np.array([2, 0, 5, 3], dtype=np.int32), np.array([2, 0, 5, 1], dtype=np.int32), np.array([2, 0, 5, 3], dtype=np.int32)]
    return bank, bank_count, [(_pack(p, R), c, f) for p, c, f in zip((p1, p2, p3), counts, frames)]


def wide_passes(seed=1):
    """One image at M = 64, R = 130 (a full wave of entries, three wave blocks of rows), N = 2 with the image on frame 1 -> as
    ``small_passes``.  Pass 1 brings 130 rows over 80 objects (50 of them seen twice), pass 2 another look at the same, pass 3 a
    look at every other object with a third of the scores low."""
    rng = np.random.default_rng(seed)
    M, R = 64, 130
    objs = [_row(rng, j % 3, -90.0 + 20.0 * (j % 10) + rng.uniform(-1, 1), 12.0 + 20.0 * (j // 10) + rng.uniform(-1, 1),
                 rng.uniform(3.6, 4.4), rng.uniform(1.6, 1.9), rng.uniform(-3, 3), 0.0) for j in range(80)]
    scores = lambda m, lo, hi: rng.permutation(np.linspace(lo, hi, m)).tolist()
    s1, s2, s3 = scores(130, 0.25, 0.95), scores(130, 0.1, 0.95), scores(40, 0.05, 0.9)
    p1 = [_seen(rng, objs[j % 80], s1[j]) for j in range(130)]
    p2 = [_seen(rng, objs[(j * 7) % 80], s2[j]) for j in range(130)]
    p3 = [_seen(rng, objs[2 * j], s3[j]) for j in range(40)]
    bank, bank_count = np.zeros((2, M, 16)), np.zeros(2, dtype=np.int32)
    one = lambda p, c: (_pack([p], R), np.array([c], dtype=np.int32), np.array([1], dtype=np.int32))
    return bank, bank_count, [one(p1, 130), one(p2, 130), one(p3, 40)]


def run(passes_of, **settings):
    """The restatement over the generated passes, state carried -> per pass (bank, bank_count, out_rows, out_count, stats, pairs),
    the bank as it is AFTER the pass."""
    bank, bank_count, passes = passes_of()
    out = []
    for rows, count, frame in passes:
        got = merge(rows, count, frame, bank, bank_count, **settings)
        out.append((bank.copy(), bank_count.copy()) + got)
    return out


def margin_holds(pairs, iou=IOU):
    """Every same-class pair: bit-coincident, or its float64 IoU further than MARGIN from the threshold (a NaN is neither)."""
    return all(coincident or abs(value - iou) > MARGIN for coincident, value in pairs)
