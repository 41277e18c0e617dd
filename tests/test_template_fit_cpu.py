"""Template fitting without a GPU: ``fit_host`` against the scalar-rounded restatement bit for bit, the restatement against the
float64 oracle away from the threshold, ``sample_mesh``, the label rows through the writer and the dataset, the conventions, every
refused configuration value, the tool (tests/fit_reference.py has the restatements and the generator)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fit_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fitter(tmpl, **loss):
    from monosowa_amd import TemplateFitter
    cfg = dict(R.CFG, loss_functions=dict(R.CFG["loss_functions"], **loss))
    return TemplateFitter(tmpl, cfg, device="cpu")


assert_same = R.assert_same


# ================================================================================================ 1. fit_host and restatement (i)
@pytest.mark.parametrize("T", [96, 65])
def test_fit_host_equals_the_restatement_bit_for_bit(T):
    tmpl, clouds, centres = R.batch(T)
    result = _fitter(tmpl).fit(clouds, centres)
    assert result.host and len(result) == 5
    got, want = result.numpy(), R.fit_f32(tmpl, clouds, centres)
    assert_same(got, want, T)
    assert want["status"].tolist() == [0, 0, 0, 1, 0] and (want["h_fine"] >= 0).all()
    assert ((got["score"] >= 0) & (got["score"] <= 1)).all()


def test_modes_and_one_way_equal_the_restatement():
    tmpl, clouds, centres = R.batch(65)
    moving, theta, loc = [True, True, False, False, False], [None, 0.4, 1.1, None, None], [False, False, True, False, False]
    for one_way in (False, True):
        f = _fitter(tmpl, loss_function="binary1way" if one_way else "binary2way")
        got = f.fit(clouds, centres, moving=moving, theta=theta, loc_only=loc).numpy()
        assert_same(got, R.fit_f32(tmpl, clouds, centres, moving, theta, loc, one_way=one_way), one_way)
        assert got["h_fine"][:4].tolist() == [-1, -1, -1, 0] and got["h_fine"][4] >= 0
    # the default centre is the per-axis median in float64
    got = _fitter(tmpl).fit(clouds[:2]).numpy()
    assert_same(got, R.fit_f32(tmpl, clouds[:2]), "median")


def test_the_array_restatement_equals_scalar_loops():
    tmpl, clouds, centres = R.batch(65)
    dx, dz, th = np.linspace(-2, 2, 6), np.linspace(-1, 3, 6), R.angles(12)
    tx, ty, tz, co, si = R.host_lists(centres[1], dx, dz, th)
    r2 = float(R.r32(R.r32(0.2) * R.r32(0.2)))
    from monosowa_amd.template_fit import placement_counts
    f = np.float32
    for i, j, k in ((3, 2, 5), (2, 2, 0), (4, 3, 11)):
        want = R.counts_scalar(tmpl, clouds[1], tx[i], ty, tz[j], co[k], si[k], r2)
        assert R.counts_f32(tmpl, clouds[1], tx[i], ty, tz[j], co[k], si[k], r2) == want
        assert placement_counts(tmpl, clouds[1], f(tx[i]), f(ty), f(tz[j]), f(co[k]), f(si[k]), f(r2)) == want
    assert max(want) > 0


# ================================================================================================ 2. float32 against float64
@pytest.mark.parametrize("T,sizes", [(96, (160, 130, 160)), (65, (130, 160, 130))])
def test_restatement_equals_the_float64_oracle_away_from_the_threshold(T, sizes):
    """Seed 1 of the generator: chosen by the float64 oracle's own flags (no winner within the margin), not by any float32 result."""
    tmpl, clouds, centres = R.batch(T, sizes=sizes, seed=1)
    dx, dz, th = np.linspace(-2, 2, 6), np.linspace(-1, 3, 6), R.angles(12)
    for o in range(3):
        h, a, b, L, ab = R.search_f32(tmpl, clouds[o], centres[o], dx, dz, th)
        h64, L64, ab64, near = R.search_f64(tmpl, clouds[o], centres[o], dx, dz, th)
        print("T %d object %d: %d of %d placements excluded, %d counts differ among all, winner %d / %d" % (
            T, o, near.sum(), len(near), (ab != ab64).sum(), h, h64))
        assert near.sum() <= 0.05 * len(near)
        assert np.array_equal(ab[~near], ab64[~near])
        assert not near[h64] and h == h64 and L == L64


# ================================================================================================ 3. sample_mesh
_BOX = """# a box, one quad face among triangles
v 0 0 0
v 2 0 0
v 2 1 0
v 0 1 0
v 0 0 4
v 2 0 4
v 2 1 4
v 0 1 4
f 1 2 3 4
f 5 6 7
f 5/1/1 7/2/1 8/3/1
f 1 2 6
f 1 6 5
f 2 3 7
f 2 7 6
f 3 4 8
f 3 8 7
f -5 -8 -4
f 4 5 8
"""


def test_sample_mesh(tmp_path):
    from monosowa_amd.template_fit import sample_mesh
    path = tmp_path / "box.obj"
    path.write_text(_BOX)
    dims = (1.5, 1.6, 3.9)
    pts = sample_mesh(str(path), n=4000, seed=3, dims=dims)
    assert pts.dtype == np.float32 and pts.shape == (4000, 3)
    half = np.array([dims[1], dims[0], dims[2]]) / 2
    assert (np.abs(pts) <= half * (1 + 1e-6)).all()
    assert np.allclose(pts.max(0), half, atol=0.02) and np.allclose(pts.min(0), -half, atol=0.02)
    assert (np.isclose(np.abs(pts), half, atol=1e-6).any(axis=1)).all()                 # every point lies on a face
    assert np.array_equal(pts, sample_mesh(str(path), n=4000, seed=3, dims=dims))
    assert not np.array_equal(pts, sample_mesh(str(path), n=4000, seed=4, dims=dims))
    # the quad's face z = -l/2 gets its share of the scaled surface, w h / (2 (w h + w l + h l)) = 0.0828; 20,000 draws have a
    # standard deviation of 0.002, the bound is five of them
    h, w, l = dims
    many = sample_mesh(str(path), n=20000, seed=3, dims=dims)
    share = np.isclose(many[:, 2], -half[2], atol=1e-6).mean()
    print("share of the quad face: %.4f" % share)
    assert abs(share - w * h / (2 * (w * h + w * l + h * l))) < 0.01
    swapped = sample_mesh(str(path), n=100, seed=3, dims=dims, axes="zyx")
    assert np.allclose(np.abs(swapped).max(0), half, atol=0.1)
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 zero\nf 1 2 3\n")
    with pytest.raises(ValueError, match="line 3"):
        sample_mesh(str(bad))
    bad.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 9\n")
    with pytest.raises(ValueError, match="line 4"):
        sample_mesh(str(bad))
    bad.write_text("v 0 0 0\n")
    with pytest.raises(ValueError, match="no face"):
        sample_mesh(str(bad))
    with pytest.raises(ValueError, match="axes"):
        sample_mesh(str(path), axes="xyy")


# ================================================================================================ 4. rows() through the writer and the dataset
from test_ignore_regions_cpu import kitti_root  # noqa: E402,F401  (the generated KITTI tree)


def test_rows_round_trip_through_the_writer_and_the_dataset(kitti_root, tmp_path):  # noqa: F811
    from monosowa_amd.helpers.tester_helper import write_kitti_results
    from monosowa_amd.kitti_dataset import KITTI_Dataset, Calibration
    cfg, root, files = kitti_root
    calib = Calibration(str(root / "training" / "calib" / "000003.txt"))
    tmpl = R.box_template(96, 5)
    pose = (1.3, 1.0, 20.7, 0.9)
    clouds = [R.noisy_copy(tmpl, 160, pose, 6), np.zeros((0, 3), dtype=np.float32)]
    centres = np.array([[1.0, 1.0, 20.0], [0.0, 0.0, 0.0]])
    result = _fitter(tmpl).fit(clouds, centres)
    rows = result.rows(calib.P2, (1242, 375), cls_id=1)
    f = result.numpy()
    assert rows.shape == (1, 14) and rows.dtype == np.float64                          # the EMPTY object gives no row
    h, w, l = R.DIMS
    assert rows[0, 0] == 1 and rows[0, 6:9].tolist() == [h, w, l]
    assert rows[0, 9] == f["x"][0] and rows[0, 10] == f["y"][0] + h / 2 and rows[0, 11] == f["z"][0] and rows[0, 13] == f["score"][0]
    assert abs(f["x"][0] - pose[0]) <= 0.4 and abs(f["z"][0] - pose[2]) <= 0.4
    x1, y1, x2, y2 = rows[0, 2:6]
    assert 0 <= x1 < x2 <= 1241 and 0 <= y1 < y2 <= 374
    u, _ = calib.rect_to_img(np.array([[f["x"][0], f["y"][0], f["z"][0]]], dtype=np.float32))
    assert x1 < u[0, 0] < x2 and y1 < u[0, 1] < y2
    assert rows[0, 1] == calib.ry2alpha(rows[0, 12], (x1 + x2) / 2)
    given = result.rows(calib.P2, (1242, 375), boxes2d=[[10, 20, 30, 40], [0, 0, 0, 0]], cls_id=1)
    assert given[0, 2:6].tolist() == [10, 20, 30, 40] and given[0, 1] == calib.ry2alpha(rows[0, 12], np.float64(20.0))
    with pytest.raises(ValueError, match="boxes2d"):
        result.rows(calib.P2, (1242, 375), boxes2d=[[10, 20, 30, 40]])
    # written by the Detector's writer, read back by the dataset as the next round's label
    out = tmp_path / "fit_out"
    write_kitti_results({3: rows.tolist()}, ["Pedestrian", "Car", "Cyclist"], str(out))
    line = (out / "000003.txt").read_text().splitlines()
    assert len(line) == 1 and line[0].startswith("Car 0.0 0 ") and len(line[0].split(" ")) == 16
    (root / "training" / "label_2" / "000003.txt").write_text((out / "000003.txt").read_text())
    ds = KITTI_Dataset("train", dict(cfg, random_flip=0.0, random_crop=0.0))
    item = [i.strip() for i in ds.idx_list].index("000003")
    objects = ds.get_label(int(ds.idx_list[item]))
    assert len(objects) == 1 and objects[0].cls_type == "Car"
    assert np.allclose([objects[0].h, objects[0].w, objects[0].l], [round(v, 2) for v in R.DIMS])
    assert np.allclose(objects[0].pos, np.round(rows[0, 9:12], 2)) and abs(objects[0].ry - rows[0, 12]) <= 0.005
    np.random.seed(0)
    _, _, t, _ = ds[item]
    assert int(t["mask_2d"].sum()) == 1


# ================================================================================================ 5. the conventions
def test_conventions():
    from monosowa_amd.template_fit import wrap_ry, coarse_angles, FINE_ANGLES
    th = np.array([0.0, np.pi / 2, np.pi, 1.5 * np.pi + 0.25, 2 * np.pi - 2 * np.pi / 360, -0.6 * np.pi, 4.6 * np.pi])
    want = []
    for yaw in (th - np.pi / 2.).tolist():                     # output.py: one wrap, `if` / `elif`
        if yaw > np.pi:
            yaw -= 2 * np.pi
        elif yaw < -np.pi:
            yaw += 2 * np.pi
        want.append(yaw)
    assert wrap_ry(th).tolist() == want and (np.abs(wrap_ry(th)[:6]) <= np.pi).all()
    assert wrap_ry(th)[6] > np.pi                              # wrapped once, as the reference does
    assert np.array_equal(coarse_angles(FINE_ANGLES), np.linspace(0, 2 * np.pi - (2 * np.pi / 360), num=360))
    # moving: the dz range moves by +1, so a copy placed one metre ahead of the static range's end is found on the grid's last node
    tmpl = R.box_template(65, 9)
    cloud = R.noisy_copy(tmpl, 130, (np.linspace(-2, 2, 6)[3], 0.0, 4.0, 0.3), 10, sigma=0.0)
    f = _fitter(tmpl)
    centre = np.zeros((1, 3))
    static = f.fit([cloud], centre).numpy()
    moving = f.fit([cloud], centre, moving=[True], theta=[0.3]).numpy()
    assert moving["z"][0] == 4.0 and moving["x"][0] == np.linspace(-2, 2, 6)[3] and moving["theta"][0] == 0.3 and moving["h_fine"][0] == -1
    assert moving["b"][0] == 130                               # every scan point is a template point at that node
    assert static["z"][0] <= 3.0 and static["b"][0] < 130 and static["a"][0] < moving["a"][0]
    # the label's y is the bottom centre: y + h / 2
    rows = f.fit([cloud], np.array([[0.0, 1.0, 0.0]]), moving=[True], theta=[0.3]).rows(np.array([[700., 0, 600, 0], [0, 700., 180, 0], [0, 0, 1, 0]]), (1242, 375))
    assert rows[0, 10] == 1.0 + R.DIMS[0] / 2 and rows[0, 12] == 0.3 - np.pi / 2
    with pytest.raises(ValueError, match="loc_only"):
        f.fit([cloud], centre, loc_only=[True])
    with pytest.raises(ValueError, match="both"):
        f.fit([cloud], centre, moving=[True], loc_only=[True], theta=[0.1])
    with pytest.raises(ValueError, match="entries"):
        f.fit([cloud], centre, moving=[True, False])
    with pytest.raises(ValueError, match="centres"):
        f.fit([cloud], np.zeros((2, 3)))
    with pytest.raises(ValueError, match=r"clouds\[0\]"):
        f.fit([np.zeros((4, 2))])


# ================================================================================================ 6. refused configuration values
@pytest.mark.parametrize("cfg,match", [
    ({"loss_functions": {"loss_function": "medboth"}}, "only binary2way"),
    ({"loss_functions": {"loss_function": "med1way"}}, "only binary2way"),
    ({"loss_functions": {"loss_function": "diffbin"}}, "only binary2way"),
    ({"loss_functions": {"loss_function": "chamfer"}}, "only binary2way"),
    ({"loss_functions": {"loss_function": "trimmed"}}, "only binary2way"),
    ({"loss_functions": {"loss_function": "binary"}}, "not a loss"),
    ({"loss_functions": {"binary_loss_threshold": 0}}, "binary_loss_threshold"),
    ({"loss_functions": {"binary_loss_threshold": -0.2}}, "binary_loss_threshold"),
    ({"loss_functions": {"binary_loss_threshold": float("nan")}}, "binary_loss_threshold"),
    ({"loss_functions": {"binary_loss_threshold": "0.2"}}, "binary_loss_threshold"),
    ({"loss_functions": {"binary_loss_threshold": 1e-30}}, "float32 square"),
    ({"loss_functions": {"binary_loss_threshold": 1e30}}, "float32 square"),
    ({"loss_functions": 3}, "mapping"),
    ({"dataset": "waymo"}, "Waymo"),
    ({"dataset": {"name": "waymo"}}, "Waymo"),
    ({"scale_detector": {"use_scale_detector": True}}, "scale detector"),
    ({"optimization": {"use_dimensions_estimation_during_optim": True}}, "dimension estimation"),
    ({"optimization": {"opt_param1_iters": 0}}, "opt_param1_iters"),
    ({"optimization": {"opt_param2_iters": 2.5}}, "opt_param2_iters"),
    ({"optimization": {"opt_param3_iters": True}}, "opt_param3_iters"),
    ({"optimization": {"opt_param1_min": float("inf")}}, "opt_param1_min"),
    ({"optimization": {"opt_param2_max": None}}, "opt_param2_max"),
    ({"templates": {"template_height": 0.0}}, "template_height"),
    ({"templates": {"template_length": "long"}}, "template_length"),
    ("binary2way", "mapping"),
])
def test_refused_configuration_values(cfg, match):
    from monosowa_amd import TemplateFitter
    with pytest.raises(ValueError, match=match):
        TemplateFitter(np.zeros((4, 3), dtype=np.float32), cfg, device="cpu")


def test_defaults_are_the_reference_configuration():
    from monosowa_amd.template_fit import fit_config
    c = fit_config()
    assert c == fit_config({}) == fit_config({"dataset": {"dataset_stride": 20}, "general": {"device": "cpu"}, "optimization": None})
    assert (c.x_min, c.x_max, c.x_iters, c.z_min, c.z_max, c.z_iters, c.theta_iters) == (-2.0, 2.0, 40, -1.0, 3.0, 40, 40)
    assert (c.one_way, c.r, c.height, c.width, c.length) == (False, 0.2, 1.526, 1.63, 3.88)
    assert fit_config({"loss_functions": {"loss_function": "binary1way"}, "dataset": "waymo_converted"}).one_way
    from monosowa_amd import TemplateFitter
    for bad in (np.zeros((4, 2)), np.zeros(3), np.array([["a", "b", "c"]])):
        with pytest.raises(ValueError, match="template"):
            TemplateFitter(bad, device="cpu")


def test_template_grid_holds_every_point_once():
    from monosowa_amd.template_fit import build_grid, MAX_DIM
    tmpl = R.box_template(96, 2)
    tmpl[5, 1], tmpl[17, 0] = np.nan, np.inf
    g, srt, start, order = build_grid(tmpl, 0.2)
    assert sorted(order.tolist()) == list(range(96)) and start[0] == 0 and start[-1] == 94 and (np.diff(start) >= 0).all()
    assert all(1 <= d <= MAX_DIM for d in g.dim) and g.ncell == g.dim[0] * g.dim[1] * g.dim[2] and len(start) == g.ncell + 1
    assert not np.isfinite(srt[94:]).all(axis=1).any() and np.isfinite(srt[:94]).all()
    assert all(1.0 / g.inv[a] >= np.float32(0.2) * np.float32(1.01) for a in range(3))
    wide = build_grid(np.array([[0, 0, 0], [100, 0.1, 3e38], [-3e38, 0, -3e38]], dtype=np.float32), 0.2)[0]
    assert list(wide.dim) == [MAX_DIM, 1, 1] and wide.inv[2] < 0 and wide.inv[0] > 0


# ================================================================================================ 7. the tool
def test_the_tool_on_two_generated_frames(tmp_path):
    tmpl = R.box_template(65, 11)
    np.save(tmp_path / "template.npy", tmpl)
    P2 = np.array([[721.5, 0, 609.5, 44.8], [0, 721.5, 172.8, 0.2], [0, 0, 1, 0.003]])
    frames = tmp_path / "clouds"
    os.makedirs(frames)
    a = R.noisy_copy(tmpl, 130, (2.3, 1.0, 21.0, 0.8), 1)
    b = R.noisy_copy(tmpl, 64, (-3.0, 1.1, 15.5, 2.0), 2)
    np.savez(frames / "000004.npz", P2=P2, img_size=np.array([1242, 375]), points_0=a, points_1=b, points_2=np.zeros((0, 3)))
    np.savez(frames / "000011.npz", P2=P2, img_size=np.array([1242, 375]), points_0=b, box2d=np.array([[100., 150, 180, 210]]),
             moving=np.array([1]), theta=np.array([2.0]))
    (tmp_path / "fit.yaml").write_text("optimization:\n  opt_param1_iters: 6\n  opt_param2_iters: 6\n  opt_param3_iters: 12\n")
    out = tmp_path / "label_2"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fit_labels.py"), "--clouds", str(frames), "--template",
                          str(tmp_path / "template.npy"), "--out", str(out), "--config", str(tmp_path / "fit.yaml"), "--device", "cpu"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert sorted(os.listdir(out)) == ["000004.txt", "000011.txt"]
    first, second = (out / "000004.txt").read_text().splitlines(), (out / "000011.txt").read_text().splitlines()
    assert len(first) == 2 and len(second) == 1 and all(l.startswith("Car 0.0 0 ") and len(l.split(" ")) == 16 for l in first + second)
    from monosowa_amd.template_fit import TemplateFitter
    f = TemplateFitter(tmpl, R.CFG, device="cpu")
    want = f.fit([a, b, np.zeros((0, 3))]).rows(P2, (1242, 375), cls_id=1)
    assert first == ["Car 0.0 0 " + " ".join("%.2f" % v for v in row[1:]) for row in want]
    want = f.fit([b], moving=[True], theta=[2.0]).rows(P2, (1242, 375), boxes2d=[[100., 150, 180, 210]], cls_id=1)
    assert second == ["Car 0.0 0 " + " ".join("%.2f" % v for v in want[0, 1:])]
    assert second[0].split(" ")[4:8] == ["100.00", "150.00", "180.00", "210.00"]
