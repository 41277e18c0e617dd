"""Object tracks on the host: ``track_host`` against the restatement of tests/track_reference.py on every scene family, the
configuration's defaults and refusals, and tools/lift_clouds.py --track on a generated window."""
import hashlib
import importlib.util
import math
import os

import numpy as np
import pytest

import track_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(sc, name=""):
    """(what the restatement makes of a scene, what ``track_host`` makes of it); the scene's margins are checked on the way"""
    from monosowa_amd import track_host
    margins = []
    want = R.track_literal(sc["centres"], sc["status"], sc["config"], sc["tmax"], margins=margins)
    R.check_margins(margins, sc["exact_ties"], name)
    res = track_host(sc["centres"], sc["status"], sc["config"], sc["tmax"])
    assert res.host and not res.tracks.is_cuda and res.moving.dtype.is_floating_point is False
    return want, R.window_of(res.numpy(), 0)


# ================================================================================================ 1. the host routine
@pytest.mark.parametrize("name", sorted(R.scenes()))
def test_track_host_equals_the_restatement(name):
    want, got = _both(R.scenes()[name], name)
    print(name, {k: np.asarray(v)[:int(want["count"])].tolist() for k, v in want.items() if k not in ("tracks", "count", "dropped")})
    R.assert_same(got, want, name)
    n, tmax = int(want["count"]), want["length"].shape[0]
    # rows at and beyond the count: -1, 0, false, NaN
    assert (got["tracks"][n:] == -1).all() and (got["ref_mask"][n:] == -1).all() and not got["length"][n:].any()
    assert not got["moving"][n:].any() and not got["visible"][n:].any() and not got["keep"][n:].any() and np.isnan(got["theta"][n:]).all()
    assert tmax == (R.F * R.M if R.scenes()[name]["tmax"] is None else R.scenes()[name]["tmax"])
    # position f of a row holds (f, slot) or (-1, -1); the slot is an OK detection of that frame
    for t in range(n):
        for f in range(R.F):
            ff, m = got["tracks"][t, f]
            assert (ff, m) == (-1, -1) or (ff == f and R.scenes()[name]["status"][f, m] & 7 == R.OK), (t, f)


@pytest.mark.parametrize("routine", ["track_host", "restatement"])
def test_the_scenes_hold_every_family(routine):
    """What each scene is there for, read off ``track_host``'s result and off the restatement's."""
    from monosowa_amd import track_host
    sc, w = R.scenes(), {}
    for name in sc:
        args = (sc[name]["centres"], sc[name]["status"], sc[name]["config"], sc[name]["tmax"])
        w[name] = R.window_of(track_host(*args).numpy(), 0) if routine == "track_host" else R.track_literal(*args)
    count = lambda name: int(w[name]["count"])
    rows = lambda name, key: w[name][key][:count(name)].tolist()
    # an empty first frame opens nothing; the tracks start at frame 2
    assert not (sc["empty_first_frame"]["status"][:2] == R.OK).any() and (w["empty_first_frame"]["tracks"][:2, :2] == -1).all()
    assert rows("empty_first_frame", "length") == [6, 6]
    # a frame without detections between two with: skipped, and the driving car is found again behind it
    assert (sc["frame_without_detections"]["status"][4] != R.OK).all() and rows("frame_without_detections", "length") == [7, 7, 4]
    assert rows("lengths", "length") == [1, 2, 3, 4, 5, 6]
    # a rematch after a gap: frames 0, 1, 5, 6 in one track
    assert [f for f in range(R.F) if w["mixed"]["tracks"][2, f, 0] >= 0] == [0, 1, 5, 6]
    # two detections nearest to one track: slot 4 is appended, slot 2 opens a track
    assert rows("two_to_one", "length") == [3, 2]
    assert w["two_to_one"]["tracks"][0, 1].tolist() == [1, 4] and w["two_to_one"]["tracks"][1, 1].tolist() == [1, 2]
    assert rows("mutual_but_far", "length") == [2, 2] and w["mutual_but_far"]["tracks"][1, 1].tolist() == [1, 0]
    # exact ties: the lower detection is appended (slot 0 of frame 1), the lower track takes the one in the middle (slot 5 of frame 1)
    t = w["exact_ties"]["tracks"]
    assert t[0, 1].tolist() == [1, 0] and t[3, 1].tolist() == [1, 3] and t[1, 1].tolist() == [1, 5] and t[2, 1].tolist() == [-1, -1]
    assert count("exact_ties") == 5
    # nothing but OK (clipped or not) with a finite centre is a detection
    assert count("not_detections") == 2 and rows("not_detections", "length") == [2, 3]
    assert int(w["overflow"]["dropped"]) == 8 and count("overflow") == 4 and int(w["overflow_by_one"]["dropped"]) == 4
    # moving: no movement at all, equal differences below and above d_move, one difference
    assert rows("moving_edges", "moving") == [False, False, True, False] and rows("moving_edges", "length") == [8, 8, 4, 2]
    assert rows("z_above", "moving") == [True] and rows("z_below", "moving") == [False]
    assert rows("net_above", "moving") == [True] and rows("net_below", "moving") == [False]
    # headings
    assert rows("heading_two", "moving") == [True] and np.isnan(w["heading_two"]["theta"][0])
    for name in ("heading_four", "heading_ref_first", "heading_ref_last", "heading_inside", "mixed"):
        assert np.isfinite(w[name]["theta"][0]), name
    assert rows("heading_hidden", "keep") == [False] and rows("heading_hidden", "moving") == [True]
    # use_pseudo_lidar both ways: hidden standing tracks are kept without it, hidden moving ones never
    assert rows("mixed", "keep") == [True, True, False, False] and rows("mixed_real_lidar", "keep") == [True, True, True, True]
    assert rows("heading_hidden_real_lidar", "keep") == [True, False] and rows("heading_hidden_real_lidar", "visible") == [False, False]


def _candidates(name):
    """the number of angles each walk of the heading takes in a one-track scene: (backward, forward, examined and rejected)"""
    sc = R.scenes()[name]
    margins = []
    w = R.track_literal(sc["centres"], sc["status"], sc["config"], sc["tmax"], margins=margins)
    examined = sum(1 for kind, _ in margins if kind == "d_angle")
    gaps = sum(1 for kind, _ in margins if kind == "angle")
    return int(w["length"][0]), examined, gaps + 1 if gaps else 0


def test_the_heading_scenes_take_the_candidates_they_are_there_for():
    assert _candidates("heading_two") == (3, 2, 0)              # two candidates: no heading
    assert _candidates("heading_four") == (5, 4, 4)             # four: the last one repeated
    assert _candidates("heading_ref_first") == (8, 5, 5)        # seven behind the reference view, five taken
    assert _candidates("heading_ref_last") == (8, 5, 5)
    assert _candidates("heading_inside") == (8, 7, 5)           # the two neighbours of the reference view lie inside d_angle
    # an even count repeats the last angle: the median is the upper of the two middle ones when the last is the largest
    sc = R.scenes()["heading_four"]
    from monosowa_amd import track_host
    theta = track_host(sc["centres"], sc["status"], sc["config"]).theta[0, 0].item()
    L = sc["centres"][1:6, 2]
    angles = [math.atan2(L[2, 2] - L[i, 2], L[2, 0] - L[i, 0]) for i in (1, 0)] + [math.atan2(L[i, 2] - L[2, 2], L[i, 0] - L[2, 0]) for i in (3, 4)]
    assert theta == -sorted(angles + [angles[-1]])[2] + math.pi / 2


@pytest.mark.parametrize("what", ["m70", "far", "w61", "w61_close"])
def test_track_host_equals_the_restatement_on_the_larger_windows(what):
    centres, status, config, tmax = larger_window(what)
    sc = {"centres": centres, "status": status, "config": config, "tmax": tmax, "exact_ties": False}
    want, got = _both(sc, what)
    R.assert_same(got, want, what)
    if what == "far":
        assert int(want["count"]) == 350 and (want["length"] == 1).all()
    if what == "m70":
        assert ((status & 7) == R.OK).sum(axis=1)[:2].min() > 64          # more tracks and more detections than a wavefront


def larger_window(what):
    """the windows the GPU tests run beside the families -> (centres, status, config, tmax)"""
    if what == "m70":
        return R.random_window(5, 3, 70, 70, seen=0.97) + (R.cfg(ref=1), None)
    if what == "far":
        return R.far_apart(5, 70) + (R.cfg(ref=2), None)
    if what == "w61":
        return R.random_window(7, 61, 8, 6) + (R.cfg(ref=30), 64)
    return R.random_window(8, 61, 8, 8, spread=12.0) + (R.cfg(ref=30), 64)


def test_several_windows_and_tensors():
    """[S, F, M, 3] in: each window as its own run; torch tensors are taken as well."""
    import torch
    from monosowa_amd import track_host
    names = ["mixed", "lengths", "exact_ties"]
    sc = R.scenes()
    centres, status = np.stack([sc[n]["centres"] for n in names]), np.stack([sc[n]["status"] for n in names])
    res = track_host(torch.from_numpy(centres), torch.from_numpy(status), R.cfg()).numpy()
    for s, n in enumerate(names):
        R.assert_same(R.window_of(res, s), R.track_literal(sc[n]["centres"], sc[n]["status"], R.cfg()), n)
    assert res["count"].tolist() == [4, 6, 5]
    for bad in ((centres[0], status), (centres[..., :2], status), (centres, status.astype(np.float64))):
        with pytest.raises(ValueError):
            track_host(*bad)


def test_objects_and_gather_args():
    from monosowa_amd import track_host
    sc = R.scenes()["mixed_real_lidar"]
    res = track_host(sc["centres"], sc["status"], sc["config"])
    kept, moving, theta = res.objects()
    assert kept == [0, 1, 2, 3] and moving == [True, False, False, False] and theta[1:] == [None] * 3
    assert isinstance(theta[0], float) and theta[0] == res.theta[0, 0].item() and all(isinstance(m, bool) for m in moving)
    table, flags = res.gather_args()
    assert tuple(table.shape) == (R.F * R.M, R.F, 2) and tuple(flags.shape) == (R.F * R.M,) and flags[:4].tolist() == moving


# ================================================================================================ 2. the configuration
def test_the_defaults_are_the_reference_configuration():
    from monosowa_amd import track_config
    from monosowa_amd import track as T
    c = track_config()
    assert c == T.TrackConfig(10.0, 5.0, 3.0, 0.2, True, 30) and track_config({}) == c and track_config(c) is c
    assert track_config({"frames_creation": {"tracker_for_merging": "3D", "use_icp": False}, "general": {"x": 1}}) == c
    c = track_config(R.cfg(d_track=2, d_move=0.0, d_angle=1.5, ref=0, pseudo=False))
    assert c == T.TrackConfig(2.0, 0.0, 1.5, 0.2, False, 0) and isinstance(c.d_track, float)
    assert T.Z0 == 0.2 and T.HALF_PI == math.pi / 2 and T.MAX_TRACKS * 156 + 256 * 40 + 32 <= 160 * 1024


@pytest.mark.parametrize("cfg", [
    {"frames_creation": {"tracker_for_merging": "2D"}}, {"frames_creation": {"tracker_for_merging": "4D"}},
    {"frames_creation": {"tracker_for_merging": 3}}, {"frames_creation": {"use_icp": True}}, {"frames_creation": {"use_icp": 1}},
    {"optimization": {"merge_two_trackers": True}}, {"optimization": {"merge_two_trackers": "no"}},
    {"frames_creation": {"dist_treshold_tracking": -1.0}}, {"frames_creation": {"dist_treshold_tracking": float("nan")}},
    {"frames_creation": {"dist_treshold_tracking": "10"}}, {"frames_creation": {"dist_treshold_moving": float("inf")}},
    {"frames_creation": {"dist_treshold_moving": True}}, {"frames_creation": {"nscans_before": -1}},
    {"frames_creation": {"nscans_before": 1.5}}, {"frames_creation": {"use_pseudo_lidar": 1}},
    {"optimization": {"moving_cars_min_dist_for_angle": -0.5}}, {"optimization": {"moving_cars_min_dist_for_angle": None}},
    {"frames_creation": [1, 2]}, {"optimization": 3}, [1], "3D"])
def test_a_malformed_or_unsupported_configuration_is_refused(cfg):
    from monosowa_amd import ObjectTracker, track_config
    with pytest.raises(ValueError):
        track_config(cfg)
    with pytest.raises(ValueError):
        ObjectTracker(cfg, device="cpu")


def test_malformed_arguments_are_refused():
    from monosowa_amd import ObjectTracker, lift_host, track_host
    sc = R.scenes()["mixed"]
    for kw in (dict(max_tracks=0), dict(max_tracks=2.5), dict(max_tracks=True)):
        with pytest.raises(ValueError):
            ObjectTracker(R.cfg(), **kw)
        with pytest.raises(ValueError):
            track_host(sc["centres"], sc["status"], R.cfg(), **kw)
    tracker = ObjectTracker(R.cfg())
    three, four = (lift_host(*R.lift_window(n), cfg=R.lift_config(1), max_points=40) for n in (3, 4))
    for bad in ([], [three, four], sc["centres"], [three, None]):
        with pytest.raises(ValueError):
            tracker.track(bad)
    res = tracker.track([three, three])                        # CPU results: the host routine, and it says so
    assert res.host and res.count.tolist() == [3, 3] and tuple(res.tracks.shape) == (2, 18, 3, 2)


# ================================================================================================ 3. the tool
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def _contents_hash(folder):
    """sha256 over the arrays of every .npz of a folder: names, dtypes, shapes, bytes (the files' own bytes hold time stamps)"""
    h = hashlib.sha256()
    for name in sorted(os.listdir(folder)):
        h.update(name.encode() + b"\0")
        with np.load(os.path.join(folder, name), allow_pickle=False) as z:
            for key in sorted(z.files):
                a = np.ascontiguousarray(z[key])
                h.update(("%s %s %s" % (key, a.dtype.str, a.shape)).encode() + b"\0" + a.tobytes())
    return h.hexdigest()


# what tools/lift_clouds.py wrote for the window below before it knew --track (recorded from the parent commit with _contents_hash)
EACH_BEFORE = "061c39dbf0103d9ceb632f8357090777865ac65f0a06ee9d0ebc9f364bef5a58"
TRACKED_BEFORE = "578c733898ff84afcd79731ab02b858a40409c9de760cf78749b4e2118049a24"


def test_lift_clouds_tracks_a_window_and_writes_what_it_wrote_before_without_the_flag(tmp_path):
    import yaml
    import lift_reference as LR
    from monosowa_amd import lift_host
    from monosowa_amd.lift import gather_host
    lift_clouds, fit_labels = _tool("lift_clouds"), _tool("fit_labels")
    n_frames, ref, tmp = 3, 1, str(tmp_path)
    depth, intr, masks, counts, poses = R.lift_window(n_frames)
    for d in ("depth", "masks"):
        os.makedirs(os.path.join(tmp, d))
    for f in range(n_frames):
        np.save(os.path.join(tmp, "depth", "%06d.npy" % (20 + f)), depth[f])
        np.save(os.path.join(tmp, "masks", "%06d.npy" % (20 + f)), masks[f, :counts[f]])
    P2 = np.array([[intr[0, 0], 0, intr[0, 2], 0], [0, intr[0, 1], intr[0, 3], 0], [0, 0, 1, 0]])
    np.save(os.path.join(tmp, "calib.npy"), P2)
    np.save(os.path.join(tmp, "poses.npy"), poses)
    np.savez(os.path.join(tmp, "tracks.npz"), tracks=np.array([[(0, 0), (1, 1), (2, 0)], [(0, 1), (1, 0), (2, 1)]]), moving=np.array([0, 1]))
    with open(os.path.join(tmp, "config.yaml"), "w") as fh:
        yaml.safe_dump(R.lift_config(ref), fh)
    common = ["--depth", os.path.join(tmp, "depth"), "--masks", os.path.join(tmp, "masks"), "--calib", os.path.join(tmp, "calib.npy"),
              "--config", os.path.join(tmp, "config.yaml"), "--device", "cpu", "--max-points", "40"]
    with_poses = common + ["--poses", os.path.join(tmp, "poses.npy")]
    # without the flag: the arrays of the parent commit
    assert lift_clouds.main(common + ["--out", os.path.join(tmp, "each")]) == 0
    assert _contents_hash(os.path.join(tmp, "each")) == EACH_BEFORE
    assert lift_clouds.main(with_poses + ["--tracks", os.path.join(tmp, "tracks.npz"), "--out", os.path.join(tmp, "tracked")]) == 0
    assert _contents_hash(os.path.join(tmp, "tracked")) == TRACKED_BEFORE
    # the flag needs the poses and excludes a track file
    for bad in (common + ["--track"], with_poses + ["--track", "--tracks", os.path.join(tmp, "tracks.npz")]):
        with pytest.raises(SystemExit):
            lift_clouds.main(bad + ["--out", os.path.join(tmp, "refused")])
    assert not os.path.exists(os.path.join(tmp, "refused"))
    # with it: the restatement's tracks, gathered by gather_host
    assert lift_clouds.main(with_poses + ["--track", "--out", os.path.join(tmp, "auto")]) == 0
    assert os.listdir(os.path.join(tmp, "auto")) == ["000021.npz"]
    got_P2, size, clouds, box2d, moving, theta = fit_labels.read_frame(os.path.join(tmp, "auto", "000021.npz"))
    fields = lift_host(depth, intr, masks, counts, poses, R.lift_config(ref), 40).numpy()
    margins = []
    want = R.track_literal(fields["centres"], fields["status"], R.lift_config(ref), margins=margins)
    R.check_margins(margins)
    kept = np.flatnonzero(want["keep"]).tolist()
    assert kept == [0, 1] and want["moving"][:3].tolist() == [False, True, False] and int(want["count"]) == 3
    assert moving == [bool(want["moving"][t]) for t in kept] and theta == [None, None]          # three views: two candidates at most
    ref_points, ref_counts, _ = gather_host(fields, want["tracks"].astype(np.int64), want["moving"], ref, 10, 10000)
    assert np.array_equal(got_P2, P2) and size == [40.0, 24.0] and len(clouds) == 2
    for cloud, box, t in zip(clouds, box2d, kept):
        assert ref_counts[t] > 0 and np.array_equal(LR.bits(cloud), LR.bits(ref_points[t, :ref_counts[t]]))
        mk = masks[ref, want["ref_mask"][t]]
        rows, cols = np.flatnonzero(mk.any(axis=1)), np.flatnonzero(mk.any(axis=0))
        assert box.tolist() == [cols[0], rows[0], cols[-1], rows[-1]]
    assert ref_counts[0] == 120 and ref_counts[1] == 40                                         # three views of the standing car, one of the other
    # use_pseudo_lidar: false keeps the car that is seen in frame 0 only; it has no mask in the reference frame and is left out
    real = R.lift_config(ref)
    real["frames_creation"]["use_pseudo_lidar"] = False
    with open(os.path.join(tmp, "real.yaml"), "w") as fh:
        yaml.safe_dump(real, fh)
    at = with_poses.index("--config") + 1
    assert lift_clouds.main(with_poses[:at] + [os.path.join(tmp, "real.yaml")] + with_poses[at + 1:] + ["--track", "--out", os.path.join(tmp, "real")]) == 0
    hidden = R.track_literal(fields["centres"], fields["status"], real)
    assert hidden["keep"][:3].tolist() == [True, True, True] and hidden["ref_mask"][2] == -1 and not hidden["moving"][2]
    _, _, clouds_real, box_real, moving_real, theta_real = fit_labels.read_frame(os.path.join(tmp, "real", "000021.npz"))
    assert len(clouds_real) == 2 == len(box_real) and moving_real == moving and theta_real == [None, None]
    assert np.array_equal(box_real, box2d) and all(np.array_equal(a, b) for a, b in zip(clouds_real, clouds))
