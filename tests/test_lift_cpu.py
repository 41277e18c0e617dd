"""Object clouds without a GPU: ``lift_host`` against the pixel-by-pixel restatement of tests/lift_reference.py bit for bit over
every edge family, the distance transform against scipy, ``lift_host`` against a literal statement of the reference's steps away
from the thresholds, ``gather`` against a scalar restatement, a planted box through lift -> gather -> ``TemplateFitter.fit_host``,
and every ValueError."""
import numpy as np
import pytest
import scipy.ndimage
import torch

import lift_reference as R


def _host(args, nmax):
    from monosowa_amd import lift_host
    res = lift_host(*args, cfg=R.CFG, max_points=nmax)
    assert res.host and not res.points.is_cuda
    return res


# ================================================================================================ 1. bit for bit
def test_lift_host_equals_the_restatement_bit_for_bit():
    args, want, _ = R.scene()
    R.assert_same(_host(args, R.NMAX).numpy(), want)
    large, want_large, _ = R.large_scene()
    R.assert_same(_host(large, 4096).numpy(), want_large)
    # without the optional arguments: every slot present, the identity pose
    depth, intr, masks, _, _ = args
    from monosowa_amd import ObjectLifter
    got = ObjectLifter(R.CFG, device="cpu", max_points=7).lift(torch.from_numpy(depth[:3]), intr[:3], torch.from_numpy(masks[:3]))
    R.assert_same(got.numpy(), R.lift_rule(depth[:3], intr[:3], masks[:3], nmax=7)[0])
    # uint8 masks, any non-zero value set; no range cut
    cfg = {"filtering": R.CFG["filtering"], "frames_creation": dict(R.CFG["frames_creation"], use_pseudo_lidar=False)}
    from monosowa_amd import lift_host
    got = lift_host(depth[2:4], intr[2:4], masks[2:4].astype(np.uint8) * 3, poses=args[4][2:4], cfg=cfg, max_points=500)
    want_open = R.lift_rule(depth[2:4], intr[2:4], masks[2:4], None, args[4][2:4], nmax=500, use_range=False)[0]
    R.assert_same(got.numpy(), want_open)
    assert want_open["status"][0, 0] == R.OK                   # the 90 m object is kept when the cut is off


def test_the_scene_holds_every_family():
    """What the rule makes of the scene is what each slot was built to show."""
    args, _, _ = R.scene()
    depth, intr, masks, counts, poses = args
    want = _host(args, R.NMAX).numpy()                         # what lift_host makes of it
    st, sh, tot = want["status"], want["shrink"], want["total"]
    fam = {name: slot for slot, name in R.FAMILIES.items()}
    area = lambda name: int(masks[fam[name]].sum())
    assert area("A = 99: s = 2") == 99 and sh[fam["A = 99: s = 2"]] == 2
    assert area("A = 100: s = 3") == 100 and sh[fam["A = 100: s = 3"]] == 3
    for name in ("a 2-px strip: E_s and E_1 empty", "a 3-px strip whose middle row has no depth: E_1 has no point"):
        assert sh[fam[name]] == -1 and st[fam[name]] == R.OK, name
    assert not R.eroded(masks[fam["a 2-px strip: E_s and E_1 empty"]], 1).any()
    assert st[fam["one valid pixel: fewer than thr"]] == R.FEW and st[0, 5] == R.FEW and area("A = 0") == 0
    assert st[fam["beyond 75 m"]] == R.FAR
    assert (st[3, :5] == R.BEHIND).all() and (st[4, :5] == R.BEHIND).all()
    assert (st[5, :5] & 7 == R.OK).all() and np.isnan(want["centres"][5, :5, 0]).all() and np.isnan(want["points"][5, 0, 0, 0])
    assert (st[6] == R.ABSENT).all() and (st[7, 3:] == R.ABSENT).all() and (st[7, :3] != R.ABSENT).all()
    assert (st == (R.OK | R.CLIPPED)).any() and ((st == R.OK) & (tot > 0)).any() and (tot[st == (R.OK | R.CLIPPED)] > R.NMAX).all()
    assert sh[fam["even count, repeated values at the median"]] == 1 and sh[fam["odd count, repeated values"]] == 1
    assert tot[fam["even count, repeated values at the median"]] % 2 == 0 and tot[fam["odd count, repeated values"]] % 2 == 1
    hole = masks[fam["a one-pixel hole"]]
    assert not hole[10, 19] and hole[9:12, 18:21].sum() == 8
    assert want["truncated"][0, 0] and want["truncated"][0, 1] and not want["truncated"][0, 3]      # rows 11 and 12 of 24
    bad = depth[1][masks[1, 3]]
    assert np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any() and (bad == 0).any() and (bad < 0).any()
    # the circle bites: the mask that is mostly background loses points
    wide = fam["mostly background, beyond 4 m of the median plane"]
    assert 0 < tot[wide] < np.isfinite(depth[wide[0]][masks[wide]]).sum()


@pytest.mark.parametrize("seed", range(4))
def test_the_distance_transform_equals_scipy(seed):
    from monosowa_amd.lift import l1_distance
    rng = np.random.default_rng(seed)
    h, w = ((17, 23), (1, 9), (12, 1), (30, 31))[seed]
    for fill in (0.5, 0.9, 0.98, 1.0, 0.0):
        mask = rng.uniform(size=(h, w)) < fill
        for r in (1, 2, 3, 7):
            D = l1_distance(mask, r + 1)
            assert D.max() <= r + 1
            assert np.array_equal(D > r, ~scipy.ndimage.binary_dilation(~mask, iterations=r)), (fill, r)


# ================================================================================================ 2. the reference, literally
def _ulps32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    key = lambda x: np.where(x.view(np.int32) < 0, np.int64(-2 ** 31) - x.view(np.int32).astype(np.int64), x.view(np.int32).astype(np.int64))
    return np.where(np.isnan(a) & np.isnan(b), 0, np.abs(key(a) - key(b)))


@pytest.mark.parametrize("which", ["scene", "large_scene"])
def test_lift_host_equals_the_reference_steps_away_from_the_thresholds(which):
    args, rule, margins = getattr(R, which)()
    # the margin first, by the restatement alone: no circle, range or sign decision within 1e-6 relative of its threshold
    assert min(margins.values()) > R.MARGIN, margins
    nmax = rule["points"].shape[2]
    want = _host(args, nmax).numpy()                           # the product's host routine, compared with the literal steps itself
    big = _host(args, 20000).numpy() if which == "scene" else want                 # unclipped clouds to compare in full
    literal = R.lift_literal(*args)
    worst_point, worst_centre = 0, 0.0
    for (f, m), (status, shrink, centre, cloud, terms) in literal.items():
        assert (want["status"][f, m] & 7) == status and want["shrink"][f, m] == shrink, (f, m, R.FAMILIES.get((f, m)))
        if status != R.OK:
            assert want["counts"][f, m] == 0 and want["total"][f, m] == 0
            continue
        assert want["total"][f, m] == len(cloud) and want["counts"][f, m] == min(len(cloud), nmax), (f, m)
        n = big["counts"][f, m]
        with np.errstate(all="ignore"):
            ulps = _ulps32(big["points"][f, m, :n], cloud[:n].astype(np.float32))
        assert ulps.max() <= 1, (f, m, ulps.max())
        worst_point = max(worst_point, int(ulps.max()))
        with np.errstate(all="ignore"):
            err = np.abs(want["centres"][f, m] - centre) / (terms * np.finfo(np.float64).eps)
        same_nan = np.isnan(want["centres"][f, m]) == np.isnan(centre)
        assert same_nan.all() and (err[~np.isnan(err)] <= 4).all(), (f, m, err)
        worst_centre = max([worst_centre] + err[~np.isnan(err)].tolist())
    print("%s: clouds within %d float32 ulp, centres within %.2f double ulp of the largest term" % (which, worst_point, worst_centre))


# ================================================================================================ 3. gather
def _made_up_fields(seed=3, F=4, M=3, nmax=7):
    """Slots with chosen status, range, truncated and counts: what gather reads."""
    rng = np.random.default_rng(seed)
    f = {"points": rng.standard_normal((F, M, nmax, 3)).astype(np.float32), "centres": rng.standard_normal((F, M, 3)),
         "counts": np.array([[7, 5, 3], [6, 7, 0], [4, 2, 7], [1, 7, 7]], dtype=np.int32),
         "status": np.array([[0, 0, 1], [0, 8, 4], [0, 3, 0], [2, 0, 8]], dtype=np.int32),
         "range": np.array([[10.0, 12.0, 1.0], [10.0, 8.0, 0.0], [14.0, 2.0, 9.5], [3.0, 12.0, 7.0]]),
         "truncated": np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], dtype=bool)}
    f["total"] = f["counts"].copy()
    f["shrink"] = np.full((F, M), 2, dtype=np.int32)
    f["counts"][f["status"] & 7 != 0] = 0
    return f


TRACKS = [
    [(1, 1), (0, 0), (1, 0), (0, 1), (2, 2)],             # 8 + 5 = 13 after 10, 10 (a tie: the earlier entry first), 12; 9.5 + 5 = 14.5 last
    [(2, 0), (0, 1), (3, 1), (0, 0), (3, 2), (1, 1), (1, 0)],     # more views than max_views
    [(0, 0), (1, 1), (1, 0)],                              # moving: the first OK view of frame 1
    [(0, 0), (2, 0), (3, 1)],                              # moving without a view of the reference frame
    [(0, 2), (1, 2), (2, 1), (3, 0)],                      # FEW, ABSENT, BEHIND, FAR: no OK view
    [],                                                    # no view at all
    [(3, 2), (3, 1), (2, 2)],                              # 7 + 7 + 7 = 21 points
    [(0, 0), (0, 0)],                                      # the same view twice
]
MOVING = [False, False, True, True, False, False, False, True]


def _result(fields):
    from monosowa_amd import LiftResult, lift_config
    return LiftResult(lift_config(R.CFG), True, **{k: torch.from_numpy(v.copy()) for k, v in fields.items()})


@pytest.mark.parametrize("max_views,K", [(10, 50), (3, 50), (1, 50), (10, 19), (10, 18), (10, 6), (2, 4), (10, 1)])
def test_gather_equals_the_scalar_restatement(max_views, K):
    fields = _made_up_fields()
    got = _result(fields).gather(TRACKS, MOVING, max_views=max_views, max_points=K)
    want = R.gather_rule(fields, TRACKS, MOVING, R.REF_FRAME, max_views, K)
    assert got[0].shape == (len(TRACKS), K, 3) and got[0].dtype == torch.float32 and got[2].dtype == torch.float64
    R.assert_same_gather([g.numpy() for g in got], want, (max_views, K))
    pts, cnt, ctr = want
    if max_views == 10:
        assert cnt[0] == min(K, 7 + 6 + 5 + 7 + 7) and cnt[4] == 0 and cnt[5] == 0 and cnt[3] == 0 and cnt[2] == min(K, 7)
        assert not ctr[3].any() and not ctr[4].any() and not ctr[5].any()
        assert np.array_equal(ctr[2], fields["centres"][1, 1])          # (1, 1), not the nearer (1, 0): the first of the track
    if (max_views, K) == (10, 50):
        order = np.concatenate([fields["points"][f, m, :fields["counts"][f, m]] for f, m in ((0, 0), (1, 0), (0, 1), (1, 1), (2, 2))])
        assert np.array_equal(pts[0, :cnt[0]], order)


def test_gather_thins_a_long_track_to_exactly_K_in_order():
    """Track 1 has n = 43 points; at K = n, n - 1 and (n - 1) / 3 the rule keeps exactly K of them, evenly spaced."""
    fields = _made_up_fields()
    full = R.gather_rule(fields, TRACKS, MOVING, R.REF_FRAME, 10, 50)
    n = int(full[1][1])                                   # 4 + 5 + 7 + 7 + 7 + 7 + 6 = 43 = 3 * 14 + 1
    assert n == 43
    for K in (43, 42, 14):                                # n = K, K + 1, 3 K + 1
        got = _result(fields).gather(TRACKS, MOVING, max_views=10, max_points=K)
        want = R.gather_rule(fields, TRACKS, MOVING, R.REF_FRAME, 10, K)
        R.assert_same_gather([g.numpy() for g in got], want, K)
        kept = got[0][1, :K].numpy()
        assert int(got[1][1]) == K
        at = [int(np.flatnonzero((full[0][1, :n] == row).all(axis=1))[0]) for row in kept]
        assert at == sorted(set(at)) and len(at) == K     # a subsequence: in order, nothing twice
        if K == 14:
            assert max(np.diff(at)) - min(np.diff(at)) <= 1


def test_gather_takes_a_table_and_skips_what_lies_outside():
    fields = _made_up_fields()
    table = np.full((len(TRACKS) + 1, 7, 2), -1, dtype=np.int32)
    for b, t in enumerate(TRACKS):
        table[b, :len(t)] = np.asarray(t, dtype=np.int32).reshape(-1, 2)
    table[-1, :3] = [(9, 0), (0, 0), (0, 5)]                # outside F x M on both sides of a good view
    got = _result(fields).gather(torch.from_numpy(table), torch.tensor(MOVING + [False]), max_views=3, max_points=11)
    want = R.gather_rule(fields, TRACKS + [[(9, 0), (0, 0), (0, 5)]], MOVING + [False], R.REF_FRAME, 3, 11)
    R.assert_same_gather([g.numpy() for g in got], want)


def test_gather_on_the_scene_and_a_nan_centre():
    args, want, _ = R.scene()
    tracks = [[(0, 0), (2, 1), (5, 1), (7, 0)], [(5, 0), (5, 2)], [(1, m) for m in range(6)], [(f, 1) for f in range(8)]]
    got = _result(want).gather(tracks, max_views=10, max_points=100)
    ref = R.gather_rule(want, tracks, None, R.REF_FRAME, 10, 100)
    R.assert_same_gather([g.numpy() for g in got], ref)
    assert np.isnan(ref[2][1, 0]) and not np.isnan(ref[2][1, 1:]).any() and np.isnan(ref[2][0, 0])


# ================================================================================================ 4. end to end
def test_a_planted_box_is_found_within_one_search_step():
    """A 1.5 x 1.6 x 3.9 m box at (1, 1, 12), yaw 0, rendered by ray casting; lift, gather, then the template search on the host with
    a 9 x 9 x 4 grid.  The search moves the template in steps of (2 - -2) / 8 = 0.5 m along x and (3 - -1) / 8 = 0.5 m along z about
    the gathered centre, so its best node can be no nearer than a step to the planted position in the worst case, and need not be
    farther: the bound is one step per axis, from the configuration."""
    import fit_reference as FR
    from monosowa_amd import ObjectLifter, TemplateFitter
    planted, dims = (1.0, 1.0, 12.0), (1.5, 1.6, 3.9)
    depth, intr, masks = R.planted_box(planted, dims)
    res = ObjectLifter(R.CFG, device="cpu", max_points=4096).lift(depth, intr, masks)
    assert res.status.tolist() == [[R.OK]] and int(res.counts[0, 0]) > 200
    clouds, counts, centres = res.gather([[(0, 0)]], max_views=10, max_points=300)
    assert counts.tolist() == [300]
    grid = dict(FR.GRID, opt_param1_iters=9, opt_param2_iters=9, opt_param3_iters=4)
    rng = np.random.default_rng(0)
    h, w, l = dims
    face = rng.integers(0, 3, 240)
    tmpl = rng.uniform(-0.5, 0.5, size=(240, 3))
    tmpl[np.arange(240), face] = np.where(rng.uniform(size=240) < 0.5, -0.5, 0.5)
    tmpl = (tmpl * np.array([w, h, l])).astype(np.float32)
    fitter = TemplateFitter(tmpl, {"optimization": grid, "loss_functions": {"loss_function": "binary2way", "binary_loss_threshold": 0.2},
                                   "templates": {"template_height": h, "template_width": w, "template_length": l}}, device="cpu")
    fit = fitter.fit_host((clouds, counts), centres).numpy()
    step_x = (grid["opt_param1_max"] - grid["opt_param1_min"]) / (grid["opt_param1_iters"] - 1)
    step_z = (grid["opt_param2_max"] - grid["opt_param2_min"]) / (grid["opt_param2_iters"] - 1)
    print("centre", centres.tolist(), "fit", fit["x"], fit["z"], fit["theta"], fit["a"], fit["b"])
    assert fit["status"].tolist() == [0]
    assert abs(fit["x"][0] - planted[0]) <= step_x and abs(fit["z"][0] - planted[2]) <= step_z


# ================================================================================================ 5. errors
@pytest.mark.parametrize("cfg", [
    {"frames_creation": {"use_hdbscan": True}}, {"frames_creation": {"use_growing_for_point_extraction": True}},
    {"frames_creation": {"use_hdbscan": "no"}}, {"frames_creation": {"use_growing_for_point_extraction": 0}},
    {"frames_creation": {"use_pseudo_lidar": 1}}, {"frames_creation": {"max_distance_pseudo_lidar": 0}},
    {"frames_creation": {"max_distance_pseudo_lidar": float("nan")}}, {"frames_creation": {"max_distance_pseudo_lidar": "75"}},
    {"frames_creation": {"max_distance_pseudo_lidar": 1e200}}, {"frames_creation": {"nscans_before": -1}},
    {"frames_creation": {"nscans_before": 1.5}}, {"frames_creation": {"nscans_before": True}},
    {"filtering": {"moving_detection_threshold": 0}}, {"filtering": {"moving_detection_threshold": 2.0}},
    {"filtering": {"moving_detection_threshold": True}}, {"filtering": {"filter_diameter": -4}},
    {"filtering": {"filter_diameter": float("inf")}}, {"filtering": {"filter_diameter": None}}, {"filtering": [1, 2]},
    {"frames_creation": 3}, "config.yaml", 7])
def test_a_malformed_or_unsupported_configuration_is_refused(cfg):
    from monosowa_amd import ObjectLifter, lift_config
    with pytest.raises(ValueError):
        lift_config(cfg)
    with pytest.raises(ValueError):
        ObjectLifter(cfg, device="cpu")


def test_the_defaults_are_the_reference_configuration():
    from monosowa_amd import lift_config
    c = lift_config()
    assert (c.thr, c.d, c.use_range, c.max_range, c.ref_frame) == (2, 4.0, True, 75.0, 30)
    assert lift_config({"optimization": {"opt_param1_iters": 3}, "frames_creation": {"nscans_after": 30, "use_icp": True}}) == c
    assert lift_config(R.CFG).ref_frame == R.REF_FRAME


def test_malformed_arguments_are_refused():
    from monosowa_amd import ObjectLifter
    (depth, intr, masks, counts, poses), _, _ = R.scene()
    lifter = ObjectLifter(R.CFG, device="cpu", max_points=8)
    bad = [dict(depth=depth[0]), dict(depth=depth[:, :, :5]), dict(intrinsics=intr[:, :3]), dict(intrinsics=intr[:2]),
           dict(masks=masks[:, 0]), dict(masks=masks[:3]), dict(masks=masks[:, :, :5]), dict(masks=masks.astype(np.float32)),
           dict(mask_count=counts[:2]), dict(mask_count=counts[:, None]), dict(poses=poses[:, :, :3]), dict(poses=poses[:1]),
           dict(depth=np.zeros((8, 0, 40), np.float32))]
    for kw in bad:
        call = dict(depth=depth, intrinsics=intr, masks=masks, mask_count=counts, poses=poses)
        call.update(kw)
        with pytest.raises(ValueError):
            lifter.lift(**call)
    for kw in (dict(max_points=0), dict(max_points=2.5), dict(max_points=True)):
        with pytest.raises(ValueError):
            ObjectLifter(R.CFG, device="cpu", **kw)
    res = lifter.lift(depth, intr, masks, counts, poses)
    for tracks, kw in (([[(0, 0, 0)]], {}), ([[(0.5, 0)]], {}), ([[(8, 0)]], {}), ([[(0, 6)]], {}), ([[(-1, 0)]], {}),
                       (np.zeros((2, 3), np.int32), {}), (np.zeros((2, 0, 2), np.int32), {}), (np.zeros((2, 3, 2), np.float32), {}),
                       ([[(0, 0)]], dict(moving=[True, False])), ([[(0, 0)]], dict(max_views=0)), ([[(0, 0)]], dict(max_points=0)),
                       ([[(0, 0)]], dict(max_views=1.5))):
        with pytest.raises(ValueError):
            res.gather(tracks, **kw)


# ================================================================================================ 6. the tool
def test_lift_clouds_writes_what_fit_labels_reads(tmp_path):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def tool(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        return module
    lift_clouds, fit_labels = tool("lift_clouds"), tool("fit_labels")
    (depth, intr, masks, counts, poses), want, _ = R.scene()
    frames = (0, 1, 2, 7)
    for d in ("depth", "masks", "each", "tracked"):
        os.makedirs(tmp_path / d)
    P2 = np.zeros((len(frames), 3, 4))
    for i, f in enumerate(frames):
        np.save(tmp_path / "depth" / ("%06d.npy" % (10 + f)), depth[f])
        np.save(tmp_path / "masks" / ("%06d.npy" % (10 + f)), masks[f, :counts[f]])
        P2[i] = [[intr[f, 0], 0, intr[f, 2], 0], [0, intr[f, 1], intr[f, 3], 0], [0, 0, 1, 0]]
    np.save(tmp_path / "calib.npy", P2)
    np.save(tmp_path / "poses.npy", poses[list(frames)])
    np.savez(tmp_path / "tracks.npz", tracks=np.array([[(0, 0), (1, 0), (2, 1)], [(1, 1), (3, 1), (-1, -1)], [(0, 1), (2, 4), (-1, -1)]]),
             moving=np.array([0, 1, 0]))
    with open(tmp_path / "config.yaml", "w") as fh:
        fh.write("filtering:\n  moving_detection_threshold: 2\nframes_creation:\n  nscans_before: 1\n")
    common = ["--depth", str(tmp_path / "depth"), "--masks", str(tmp_path / "masks"), "--calib", str(tmp_path / "calib.npy"),
              "--config", str(tmp_path / "config.yaml"), "--device", "cpu", "--max-points", str(R.NMAX)]
    assert lift_clouds.main(common + ["--out", str(tmp_path / "each")]) == 0
    own = R.lift_rule(depth, intr, masks, counts, None, nmax=R.NMAX)[0]       # every frame in its own coordinates
    for i, f in enumerate(frames):
        got_P2, size, clouds, box2d, moving, theta = fit_labels.read_frame(str(tmp_path / "each" / ("%06d.npz" % (10 + f))))
        ok = [m for m in range(masks.shape[1]) if (own["status"][f, m] & 7) == R.OK]
        assert len(clouds) == len(ok) == len(box2d) and np.array_equal(got_P2, P2[i]) and size == [40.0, 24.0] and not any(moving)
        for cloud, box, m in zip(clouds, box2d, ok):
            assert np.array_equal(R.bits(cloud), R.bits(own["points"][f, m, :own["counts"][f, m]]))
            rows, cols = np.flatnonzero(masks[f, m].any(axis=1)), np.flatnonzero(masks[f, m].any(axis=0))
            assert box.tolist() == [cols[0], rows[0], cols[-1], rows[-1]]
    assert lift_clouds.main(common + ["--poses", str(tmp_path / "poses.npy"), "--tracks", str(tmp_path / "tracks.npz"),
                                      "--out", str(tmp_path / "tracked")]) == 0
    assert os.listdir(tmp_path / "tracked") == ["000011.npz"]                   # the reference frame: index 1 of the four
    _, _, clouds, box2d, moving, _ = fit_labels.read_frame(str(tmp_path / "tracked" / "000011.npz"))
    sub = {k: v[list(frames)] for k, v in want.items()}
    ref = R.gather_rule(sub, [[(0, 0), (1, 0), (2, 1)], [(1, 1), (3, 1)], [(0, 1), (2, 4)]], [False, True, False], 1, 10, 10000)
    assert len(clouds) == 2 and moving == [False, True]                         # the third track has no view in the reference frame
    for b in range(2):
        assert np.array_equal(R.bits(clouds[b]), R.bits(ref[0][b, :ref[1][b]]))
