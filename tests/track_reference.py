"""The track rule of include/monosowa_track.h restated in the reference's own shape -- Python lists of tracks, ``cdist`` and ``norm``
distances, ``np.mean`` / ``np.std`` / ``np.median``, the z-score as a quotient -- and the scenes the track tests share.

The restatement decides with square roots and quotients where the rule compares squares and products, so the two may differ within a
few ulp of a threshold.  ``track_literal`` therefore records how far every decision was from its threshold or tie, and
``check_margins`` holds every scene to ``MARGIN`` (relative); neighbouring candidate angles are ``ANGLE_GAP`` apart, so that a median
that picked a neighbouring element cannot pass for the right one.  The one exception are deliberate exact ties, built from multiples
of 1/8: squares, sums and roots of those are exact, and both formulations must pick the lowest index."""
import numpy as np
from scipy.spatial.distance import cdist

OK, FEW, FAR, BEHIND, ABSENT, CLIPPED = 0, 1, 2, 3, 4, 8
MARGIN = 1e-9
ANGLE_GAP = 1e-6
THETA_TOL = 4 * np.spacing(np.pi)          # 4 ulp of pi: the same element chosen, given ANGLE_GAP
F, M = 8, 6
FIELDS = ("tracks", "length", "ref_mask", "moving", "visible", "keep", "theta", "count", "dropped")
EXACT = ("tracks", "length", "ref_mask", "moving", "visible", "keep", "count", "dropped")


def cfg(d_track=10.0, d_move=5.0, d_angle=3.0, ref=3, pseudo=True):
    """the reference's sections and key names"""
    return {"frames_creation": {"dist_treshold_tracking": d_track, "dist_treshold_moving": d_move, "nscans_before": ref,
                                "use_pseudo_lidar": pseudo, "tracker_for_merging": "3D", "use_icp": False},
            "optimization": {"moving_cars_min_dist_for_angle": d_angle, "merge_two_trackers": False}}


def _note(margins, kind, value, threshold):
    if margins is not None and np.isfinite(value):
        margins.append((kind, abs(value - threshold) / threshold if threshold > 0 else abs(value - threshold)))


def _note_argmin(margins, dists):
    if margins is None:
        return
    for table in (dists, dists.T):
        if table.shape[1] > 1:
            two = np.sort(table, axis=1)[:, :2]
            for lo, hi in two:
                margins.append(("argmin", (hi - lo) / hi if hi > 0 else 0.0))


def track_literal(centres, status, config, tmax=None, z0=0.2, margins=None):
    """One window, centres [F, M, 3] and status [F, M] -> the fields of a TrackResult for it (numpy, no window axis)."""
    fc, opt = config["frames_creation"], config["optimization"]
    d_track, d_move, ref, pseudo = fc["dist_treshold_tracking"], fc["dist_treshold_moving"], fc["nscans_before"], fc["use_pseudo_lidar"]
    d_angle = opt["moving_cars_min_dist_for_angle"]
    n_frames, n_slots = status.shape
    tmax = n_frames * n_slots if tmax is None else tmax
    cars, car_slots = [], []
    for f in range(n_frames):
        found = [m for m in range(n_slots) if status[f, m] % 8 == OK and np.all(np.isfinite(centres[f, m]))]
        cars.append(np.array([centres[f, m] for m in found]).reshape(-1, 3))
        car_slots.append(found)
    tracked, tracked_slots, dropped = [], [], 0             # tracked[t]: rows (x, y, z, frame), as the reference appends them

    def open_track(f, z):
        nonlocal dropped
        if len(tracked) < tmax:
            tracked.append([np.append(cars[f][z], f)])
            tracked_slots.append([car_slots[f][z]])
        else:
            dropped += 1

    for f in range(n_frames):
        cur = cars[f]
        if len(cur) == 0:
            continue
        if len(tracked) == 0:
            for z in range(len(cur)):
                open_track(f, z)
            continue
        estimates = []
        for car in tracked:
            if len(car) == 1:
                estimates.append(car[0][:3])
                continue
            est = car[-1][:3] - car[-2][:3]
            for back in range(2, min(len(car) - 1, 4) + 1):
                est = est + (car[-back][:3] - car[-back - 1][:3])
            estimates.append(est / min(len(car) - 1, 4) + car[-1][:3])
        estimates = np.array(estimates)
        dists = cdist(cur, estimates)
        _note_argmin(margins, dists)
        cur_to_track, track_to_cur = np.argmin(dists, axis=1), np.argmin(dists, axis=0)
        fresh = []
        for z in range(len(cur)):
            t = cur_to_track[z]
            if track_to_cur[t] == z:
                dist = np.linalg.norm(cur[z] - estimates[t])
                _note(margins, "d_track", dist, d_track)
                if dist < d_track:
                    tracked[t].append(np.append(cur[z], f))
                    tracked_slots[t].append(car_slots[f][z])
                    continue
            fresh.append(z)
        for z in fresh:
            open_track(f, z)

    out = {"tracks": np.full((tmax, n_frames, 2), -1, dtype=np.int32), "length": np.zeros(tmax, dtype=np.int32),
           "ref_mask": np.full(tmax, -1, dtype=np.int32), "moving": np.zeros(tmax, dtype=bool), "visible": np.zeros(tmax, dtype=bool),
           "keep": np.zeros(tmax, dtype=bool), "theta": np.full(tmax, np.nan), "count": np.int32(len(tracked)),
           "dropped": np.int32(dropped)}
    for t, (car, slots) in enumerate(zip(tracked, tracked_slots)):
        locations = np.array(car)
        for row, m in zip(car, slots):
            out["tracks"][t, int(row[3])] = (int(row[3]), m)
        out["length"][t] = len(car)
        # standing or moving
        moving = False
        diffs = locations[1:, :3] - locations[:-1, :3]
        if len(diffs) > 1:
            with np.errstate(all="ignore"):
                means, sigma = np.mean(diffs, axis=0), np.std(diffs, axis=0) / np.sqrt(2)
                z_score = np.linalg.norm(means) / np.linalg.norm(sigma)
            displacement = np.linalg.norm(locations[-1, :3] - locations[0, :3])
            _note(margins, "z0", z_score, z0)
            _note(margins, "d_move", displacement, d_move)
            moving = bool(z_score > z0 and displacement > d_move)
        out["moving"][t] = moving
        # the view of the reference frame
        ref_idx = None
        for i in range(len(car)):
            if car[i][3] == ref:
                ref_idx = i
        out["visible"][t] = ref_idx is not None
        out["ref_mask"][t] = -1 if ref_idx is None else slots[ref_idx]
        out["keep"][t] = ref_idx is not None or (not pseudo and not moving)
        # the heading of a moving track
        if moving and ref_idx is not None and len(car) >= 3:
            angles = []
            for step in (-1, 1):
                i, taken = ref_idx + step, 0
                while 0 <= i < len(car) and taken < 5:
                    a, b = (locations[i], locations[ref_idx]) if step < 0 else (locations[ref_idx], locations[i])
                    dist = np.sqrt(np.power(b[0] - a[0], 2) + np.power(b[2] - a[2], 2))
                    _note(margins, "d_angle", dist, d_angle)
                    if dist > d_angle:
                        angles.append(np.arctan2(b[2] - a[2], b[0] - a[0]))
                        taken += 1
                    i += step
            if len(angles) >= 3:
                if margins is not None:
                    margins.extend(("angle", gap) for gap in np.diff(np.sort(angles)))
                if len(angles) % 2 == 0:
                    angles.append(angles[-1])
                out["theta"][t] = -np.median(np.array(angles)) + np.pi / 2
    return out


def check_margins(margins, exact_ties=False, what=""):
    """Every decision of a scene lies MARGIN away from its threshold, every pair of candidate angles ANGLE_GAP apart; ``exact_ties``:
    the scene holds argmin ties on purpose (and nothing between an exact tie and MARGIN)."""
    for kind, value in margins:
        if kind == "angle":
            assert value >= ANGLE_GAP, (what, kind, value)
        elif kind == "argmin" and exact_ties and value == 0.0:
            continue
        else:
            assert value > MARGIN, (what, kind, value)


def assert_same(got, want, what=""):
    """``got``: one window's fields (numpy).  Exact on every integer and flag; theta: the same NaNs, finite values within THETA_TOL."""
    for k in EXACT:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (what, k, got[k], want[k])
    g, w = np.asarray(got["theta"]), np.asarray(want["theta"])
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, "theta", g, w)
    worst = float(np.max(np.abs(g - w)[~np.isnan(w)], initial=0.0))
    assert worst <= THETA_TOL, (what, "theta", worst)
    return worst


def window_of(result, s):
    """window ``s`` of TrackResult.numpy()"""
    return {k: v[s] for k, v in result.items()}


# ---------------------------------------------------------------------------------------------------------------- scenes
def window(places, n_frames=F, n_slots=M):
    """(frame, slot, centre[, status]) placements -> centres [F, M, 3], status [F, M]; every other slot ABSENT with a zero centre"""
    centres, status = np.zeros((n_frames, n_slots, 3)), np.full((n_frames, n_slots), ABSENT, dtype=np.int32)
    for f, m, c, *st in places:
        assert status[f, m] == ABSENT, (f, m)
        centres[f, m], status[f, m] = c, (st[0] if st else OK)
    return centres, status


def _jitter(k, scale=0.01):
    """a small, fixed, irregular offset: keeps differences from being equal by accident"""
    return scale * np.array([np.sin(12.9898 * k + 1.0), np.sin(78.233 * k + 2.0), np.sin(37.719 * k + 3.0)])


def _line(start, step, frames, slot, bend=0.0, jitter=0.01, key=0):
    """an object at start + i * step (+ bend * i^2 in z) in each of ``frames`` (i = the frame number); slot(f) or a fixed slot"""
    return [(f, slot(f) if callable(slot) else slot, np.asarray(start, float) + f * np.asarray(step, float) + [0.0, 0.0, bend * f * f]
             + _jitter(31 * key + f, jitter)) for f in frames]


def scenes():
    """name -> dict(centres, status, config, tmax, exact_ties): every family of the issue at F = 8, M = 6."""
    out = {}

    def add(name, places, config=None, tmax=None, exact_ties=False):
        centres, status = window(places)
        out[name] = {"centres": centres, "status": status, "config": config or cfg(), "tmax": tmax, "exact_ties": exact_ties}

    # a car driving through all frames (heading from 2 + 3 candidates, the neighbours of the reference view inside d_angle), a standing
    # one, one that is seen again after a gap of three frames, one that shows up late; the slots change from frame to frame
    drive = _line((-30.0, 1.0, 20.0), (2.0, 0.0, 1.5), range(8), lambda f: (f * 5) % 6, bend=0.05, key=1)
    stand = _line((0.0, 1.2, 35.0), (0.0, 0.0, 0.0), range(8), lambda f: (f * 5 + 1) % 6, key=2)
    again = _line((40.0, 1.1, 25.0), (0.1, 0.0, 0.0), (0, 1, 5, 6), lambda f: (f * 5 + 2) % 6, key=3)
    late = _line((80.0, 0.9, 50.0), (0.0, 0.0, 0.2), (6, 7), lambda f: (f * 5 + 3) % 6, key=4)
    add("mixed", drive + stand + again + late)
    add("mixed_real_lidar", drive + stand + again + late, cfg(pseudo=False))
    add("empty_first_frame", [p for p in drive + stand if p[0] >= 2])
    add("frame_without_detections", [p for p in drive + stand + again if p[0] != 4])
    # lengths 1 .. 6: object j is seen in frames 0 .. j; the longest passes every velocity window k = 1 .. 4
    add("lengths", sum([_line((-60.0 + 25.0 * j, 1.0, 30.0 + j), (1.0, 0.0, 0.5), range(j + 1), j, key=10 + j) for j in range(6)], []))
    # two detections nearest to one track: the nearer is appended, the other opens a track; a mutual pair beyond d_track
    add("two_to_one", [(0, 0, (0.0, 1.0, 20.0)), (1, 2, (2.0, 1.0, 21.0)), (1, 4, (1.0, 1.0, 20.25)), (2, 1, (1.5, 1.0, 20.0)),
                       (2, 3, (2.5, 1.0, 21.25))])
    add("mutual_but_far", [(0, 3, (0.0, 1.0, 20.0)), (1, 0, (9.0, 1.0, 26.0)), (2, 5, (9.5, 1.0, 26.0)), (3, 5, (0.5, 1.0, 20.0))])
    # exact ties, multiples of 1/8: two detections equally near one track (the lower detection wins), one detection equally near two
    # tracks (the lower track wins), and a square on whose diagonal both happen at once
    add("exact_ties", [(0, 1, (0.0, 1.0, 8.0)), (1, 0, (-1.0, 1.0, 8.0)), (1, 3, (1.0, 1.0, 8.0)), (2, 2, (0.0, 1.0, 8.125)),
                       (0, 4, (40.0, 1.0, 16.0)), (0, 5, (44.0, 1.0, 16.0)), (1, 5, (42.0, 1.0, 16.0)),
                       (3, 0, (41.0, 1.0, 17.0)), (3, 1, (43.0, 1.0, 15.0)), (3, 4, (-0.5, 1.0, 8.5))], exact_ties=True)
    # centres that are not finite, every status that is not OK (each with a centre that would match), OK with the CLIPPED bit
    add("not_detections", [(0, 0, (0.0, 1.0, 20.0)), (0, 1, (30.0, 1.0, 20.0), OK | CLIPPED), (1, 0, (np.nan, 1.0, 20.0)),
                           (1, 1, (0.2, 1.0, np.inf)), (1, 2, (0.1, -np.inf, 20.0)), (1, 3, (30.5, 1.0, 20.0), OK | CLIPPED),
                           (2, 0, (0.3, 1.0, 20.0), FEW), (2, 1, (0.2, 1.0, 20.1), FAR), (2, 2, (0.1, 1.0, 20.2), BEHIND),
                           (2, 3, (0.4, 1.0, 20.3), ABSENT), (2, 4, (31.0, 1.0, 20.0), FEW | CLIPPED), (3, 5, (0.5, 1.0, 20.0)),
                           (3, 2, (31.5, 1.0, 20.0))])
    # more detections than rows: four tracks open, two detections are dropped at once and every later one that matches none
    many = sum([_line((-50.0 + 20.0 * j, 1.0, 30.0), (0.2, 0.0, 0.1), range(4), (j + 2) % 6, key=20 + j) for j in range(6)], [])
    add("overflow", many, tmax=4)
    add("overflow_by_one", many, tmax=5)
    # moving: one difference; equal differences (no variance) over more than d_move; no movement at all; multiples of 1/8 throughout
    add("moving_edges", [(f, 0, (8.0 * f, 1.0, 20.0)) for f in (2, 3)] + [(f, 1, (-40.0 + 2.0 * f, 1.0, 30.0 + f)) for f in range(1, 5)]
        + [(f, 2, (60.0, 1.5, 40.0)) for f in range(8)] + [(f, 3, (-80.0 + 0.125 * f, 1.0, 25.0)) for f in range(8)])
    # the z-score either side of z0: differences m + s, m - s, .. along x give z = sqrt 2 * m / s exactly in the reals
    for name, factor in (("z_above", 1.0 + 1e-6), ("z_below", 1.0 - 1e-6)):
        s, x, places = np.sqrt(2.0) / (0.2 * factor), 0.0, []
        for f in range(7):
            places.append((f + 1, f % 6, (x, 1.0, 30.0)))
            x += 1.0 + (s if f % 2 == 0 else -s)
        add(name, places, cfg(d_track=100.0, ref=0))       # no view in the reference frame: on a straight line the angles agree
    # the net displacement either side of d_move, five views on a line with a little sideways jitter
    for name, factor in (("net_above", 1.0 + 1e-6), ("net_below", 1.0 - 1e-6)):
        add(name, [(f, 2, (5.0 * factor * f / 4.0, 1.0 + (0.01 if f % 2 else 0.0), 30.0)) for f in range(5)], cfg(ref=2))
    # headings.  An arc, so that no two candidate angles agree; step 4 > d_angle.  Three views: two candidates, no heading.  Five views
    # about the reference view: four candidates, the last repeated.  The reference view first / last of eight: five of seven taken.
    arc = lambda frames, slot: _line((-10.0, 1.0, 30.0), (4.0, 0.0, 0.5), frames, slot, bend=0.15, key=40)
    add("heading_two", arc((2, 3, 4), 1))
    add("heading_four", arc((1, 2, 3, 4, 5), 2))
    add("heading_ref_first", arc(range(8), 3), cfg(ref=0))
    add("heading_ref_last", arc(range(8), 4), cfg(ref=7))
    add("heading_hidden", arc((0, 1, 2, 4, 5), 5))                     # moving, no view in the reference frame: not kept
    add("heading_hidden_real_lidar", arc((0, 1, 2, 4, 5), 5) + stand[:2], cfg(pseudo=False))
    # steps of 2 < d_angle: the neighbours of the reference view are inside, the next ones (4) outside
    add("heading_inside", _line((-5.0, 1.0, 30.0), (2.0, 0.0, 0.1), range(8), 0, bend=0.06, key=41))
    return out


def random_window(seed, n_frames, n_slots, objects, spread=40.0, seen=0.7, speed=1.5):
    """``objects`` cars on lines from well separated starts, each seen in a frame with probability ``seen``, in shuffled slots; about
    one slot in five of the rest holds a status that is not OK with a centre near a car"""
    rng = np.random.default_rng(seed)
    assert objects <= n_slots
    centres, status = np.zeros((n_frames, n_slots, 3)), np.full((n_frames, n_slots), ABSENT, dtype=np.int32)
    starts = np.stack([spread * np.arange(objects), np.ones(objects), 30.0 + rng.uniform(0, 10, objects)], axis=1)
    steps = rng.uniform(-speed, speed, (objects, 3)) * [1.0, 0.02, 1.0] * (rng.uniform(size=(objects, 1)) < 0.6)
    for f in range(n_frames):
        slots = rng.permutation(n_slots)
        for j in range(objects):
            here = starts[j] + f * steps[j] + rng.normal(0, 0.05, 3)
            if rng.uniform() < seen:
                centres[f, slots[j]], status[f, slots[j]] = here, OK | (CLIPPED if rng.uniform() < 0.1 else 0)
            elif rng.uniform() < 0.5:
                centres[f, slots[j]], status[f, slots[j]] = here, rng.choice([FEW, FAR, BEHIND])
    return centres, status


def far_apart(n_frames, n_slots):
    """every detection of every frame more than d_track from every other: F * M tracks of one view"""
    centres = np.zeros((n_frames, n_slots, 3))
    for f in range(n_frames):
        for m in range(n_slots):
            centres[f, m] = (25.0 * m + 0.37 * f, 1.0 + 0.01 * f, 20.0 + 30.0 * f + 0.11 * m)
    return centres, np.zeros((n_frames, n_slots), dtype=np.int32)


LIFT_CFG = {"filtering": {"moving_detection_threshold": 2, "filter_diameter": 4},
            "frames_creation": {"dist_treshold_tracking": 3.0, "dist_treshold_moving": 1.0, "use_pseudo_lidar": True,
                                "max_distance_pseudo_lidar": 75.0, "tracker_for_merging": "3D", "use_icp": False},
            "optimization": {"moving_cars_min_dist_for_angle": 0.5, "merge_two_trackers": False}}


def lift_config(ref):
    """LIFT_CFG with the reference frame at index ``ref``: one dict for the lifter, the tracker and the restatement"""
    return dict(LIFT_CFG, frames_creation=dict(LIFT_CFG["frames_creation"], nscans_before=ref))


def lift_window(n_frames):
    """Inputs of a lift on the 24 x 40 image of lift_reference, ``n_frames`` frames under one pose: a car that stands (10 m), one
    that drives across the image and away (four columns and 0.4 m a frame, from 9 m), one that is seen in the first frame only, and a
    mask without depth.  The slots of the first two swap in odd frames.  -> (depth, intrinsics, masks, mask_count, poses)"""
    import lift_reference as L
    rng = np.random.default_rng(11)
    depth, masks = [], []
    for f in range(n_frames):
        stands, drives = L._rect(13, 23, 3, 15), L._rect(2, 11, 4 + 4 * f, 13 + 4 * f)
        once, empty = L._rect(12, 22, 28, 38) if f == 0 else np.zeros((L.H, L.W), dtype=bool), L._rect(1, 2, 36, 39)
        order = [stands, drives] if f % 2 == 0 else [drives, stands]
        planes = [10.0, 9.0 + 0.4 * f] if f % 2 == 0 else [9.0 + 0.4 * f, 10.0]
        frame = order + [once, empty] + [np.zeros((L.H, L.W), dtype=bool)] * (L.M - 4)
        image = L._frame(rng, frame, planes + [14.0, None] + [None] * (L.M - 4))
        image[1, 36:39] = np.nan
        depth.append(image)
        masks.append(np.stack(frame))
    poses = np.tile(L._turn_y(0.05, (0.2, 0.0, 0.5)), (n_frames, 1, 1))
    return (np.stack(depth), np.tile(np.array(L.INTR, dtype=np.float64), (n_frames, 1)), np.stack(masks),
            np.full(n_frames, 4, dtype=np.int32), poses)
