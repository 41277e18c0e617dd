"""dataset.device_aug on the CPU (monosowa_amd/image_prep.py, photometric.py draw / apply, KITTI_Dataset's raw mode): the raw
sample + its record carry everything the default mode computes, and ``prepare_reference`` -- the numpy restatement of Pillow's
affine bilinear transform and of the photometric chain -- equals the live CPU pipeline of this machine's Pillow / numpy on
EVERY element.  No tolerance anywhere except the reference fixture's own ``img_sum`` (1e-9, as tests/test_kitti_dataset.py).

The generated cases below (``generated_cases``) are shared with tests/test_image_prep_gpu.py."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESOLUTION = (1280, 384)
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)

# (config of which fixture, split, seeds): the samples both fixtures hold the reference's outputs for
FIXTURE_RUNS = (("kitti_dataset.npz", "val", (0,)), ("kitti_dataset.npz", "train", (11, 12, 13)), ("kitti_dataset_pd.npz", "train", (21, 22)))


def write_kitti_root(golden_dir, path):
    """The KITTI directory that travels inside kitti_dataset.npz -> ``path``; returns the two fixtures."""
    g = np.load(os.path.join(golden_dir, "kitti_dataset.npz"), allow_pickle=False)
    for i, name in enumerate(g["file_names"]):
        p = os.path.join(str(path), str(name))
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(g["file_%03d" % i].tobytes())
    return {"kitti_dataset.npz": g, "kitti_dataset_pd.npz": np.load(os.path.join(golden_dir, "kitti_dataset_pd.npz"), allow_pickle=False)}


def fixture_cfg(fixtures, name, root, **extra):
    return dict(json.loads(str(fixtures[name]["cfg_json"])), root_dir=str(root), **extra)


@pytest.fixture()
def kitti(golden_dir, tmp_path):
    return write_kitti_root(golden_dir, tmp_path), tmp_path


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_raw_mode_keeps_every_other_output_and_the_random_stream(kitti):
    """Items 1 and 2: P2, all targets, all shared info entries and numpy's random state equal the default mode's at the same
    seed; ``prepare_reference`` of the raw sample equals the default mode's image on every element, and through it the
    reference's fixture entries (``img_sub`` exactly, ``img_sum`` to 1e-9)."""
    from monosowa_amd.image_prep import RECORD_DOUBLES, prepare_reference
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    fixtures, root = kitti
    n = flips = distorted = 0
    for name, split, seeds in FIXTURE_RUNS:
        g = fixtures[name]
        ds = KITTI_Dataset(split, fixture_cfg(fixtures, name, root))
        ds_raw = KITTI_Dataset(split, fixture_cfg(fixtures, name, root, device_aug=True))
        assert not ds.device_aug and ds_raw.device_aug
        for seed in seeds:
            for item in range(len(ds)):
                np.random.seed(seed * 100 + item)
                img, P2, targets, info = ds[item]
                state = np.random.get_state()
                np.random.seed(seed * 100 + item)
                raw, P2r, targets_r, info_r = ds_raw[item]
                state_r = np.random.get_state()
                key = "%s_s%d_i%d__" % (split, seed, item)
                assert state[0] == state_r[0] and np.array_equal(state[1], state_r[1]) and state[2:] == state_r[2:], key
                assert raw.dtype == np.uint8 and raw.shape == (info["img_size"][1], info["img_size"][0], 3)
                assert _same(P2, P2r) and set(targets) == set(targets_r) and set(info_r) == set(info) | {"prep"}
                for k in targets:
                    assert _same(targets[k], targets_r[k]), (key, k)
                for k in info:
                    assert _same(info[k], info_r[k]), (key, k)
                rec = info_r["prep"]
                assert rec.dtype == np.float64 and rec.shape == (RECORD_DOUBLES,)
                assert np.array_equal(rec[2:8], np.asarray(info["affine_inv"], dtype=np.float64).reshape(-1))
                got = prepare_reference(raw, rec)
                assert got.dtype == np.float32 and got.shape == (3, 384, 1280)
                assert np.array_equal(got, img), (key, int((got != img).sum()))
                assert np.array_equal(got[:, ::8, ::8], g[key + "img_sub"]), key
                want_sum = float(g[key + "img_sum"])
                assert abs(got.astype(np.float64).sum() - want_sum) <= 1e-9 * max(1.0, abs(want_sum))
                n += 1
                flips += int(info["flip"])
                distorted += int(int(rec[8]) & 2 != 0)
    assert n == 36 and 0 < flips < n and distorted == 12          # 6 images: 1 + 3 + 2 seeds; both branches; aug_pd on for seeds 21, 22


def test_raw_mode_refuses_what_is_not_8_bit_rgb_and_keeps_the_test_arity(kitti):
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    fixtures, root = kitti
    cfg = fixture_cfg(fixtures, "kitti_dataset.npz", root, device_aug=True)
    ds = KITTI_Dataset("val", cfg)
    index = int(ds.idx_list[0])
    path = os.path.join(ds.image_dir, "%06d.png" % index)
    Image.open(path).convert("L").save(path)
    with pytest.raises(ValueError, match=re.escape("%06d.png" % index)):
        ds[0]
    # the `test` split: (image, P2, image, info), raw in both places
    os.makedirs(os.path.join(str(root), "testing"), exist_ok=True)
    for sub in ("image_2", "calib"):
        if not os.path.exists(os.path.join(str(root), "testing", sub)):
            os.symlink(os.path.join(str(root), "training", sub), os.path.join(str(root), "testing", sub))
    with open(os.path.join(str(root), "ImageSets", "test.txt"), "w") as f:
        f.write("\n".join(ds.idx_list[1:3]) + "\n")
    sample = KITTI_Dataset("test", cfg)[0]
    assert len(sample) == 4 and sample[0].dtype == np.uint8 and sample[2] is sample[0] and "prep" in sample[3]
    assert len(KITTI_Dataset("test", dict(cfg, device_aug=False))[0]) == 4


# ---------------------------------------------------------------------------------------------------------------------------------
# generated cases (item 3), shared with the GPU test
SIZES = ((1242, 375), (1224, 370), (1408, 376), (1920, 1280), (640, 200), (1280, 384))
# (crop scale, centre shift x, centre shift y) as fractions of the image size, through the product's get_affine_transform:
# identity, shrinking, growing (the window leaves the image on all sides), windows that leave it on the left / right / top / bottom
CROPS = ((1.0, 0.0, 0.0), (0.6, 0.0, 0.0), (1.4, 0.0, 0.0), (1.0, -0.2, 0.0), (1.0, 0.2, 0.0), (1.0, 0.0, -0.25), (1.0, 0.0, 0.25),
         (0.8, 0.17, -0.11), (1.25, -0.3, 0.2), (0.71, -0.2, 0.2))
N_PD, N_PLAIN = 60, 12


def _image(rng, size, smooth):
    w, h = size
    if not smooth:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ph = rng.uniform(0, 6.28, 3)
    chans = [127.5 + 127.5 * np.sin(xx / rng.uniform(20, 90) + yy / rng.uniform(15, 60) + p) for p in ph]
    return np.clip(np.stack(chans, -1) + rng.normal(0, 2, (h, w, 3)), 0, 255).astype(np.uint8)


def generated_cases():
    """N_PD cases with a photometric draw (numpy seed 5000 + i) and N_PLAIN without: dicts of raw uint8 [h, w, 3], the six
    affine coefficients, flip, the numpy seed of the draw (None: aug_pd off).  Sizes, contents, flips and crops cycle with
    coprime periods so that every combination class occurs."""
    from monosowa_amd.kitti_dataset import get_affine_transform
    rng = np.random.default_rng(20250)
    cases = []
    for i in range(N_PD + N_PLAIN):
        size = SIZES[i % len(SIZES)]
        scale, sx, sy = CROPS[(i // 2) % len(CROPS)] if i % 7 else (float(rng.uniform(0.6, 1.4)), float(rng.uniform(-0.2, 0.2)), float(rng.uniform(-0.2, 0.2)))
        img_size = np.array(size)
        center = img_size / 2 + img_size * np.array([sx, sy])
        _, inv = get_affine_transform(center, img_size * scale, 0, np.array(RESOLUTION), inv=1)
        cases.append({"raw": _image(rng, size, smooth=(i // 3) % 2 == 1), "a": tuple(inv.reshape(-1).tolist()), "flip": (i // 5) % 2 == 1,
                      "seed": 5000 + i if i < N_PD else None, "size": size})
    return cases


def case_record(case):
    """The record of a generated case, its photometric part drawn by PhotometricDistort.draw() at the case's seed."""
    from monosowa_amd.image_prep import make_record
    from monosowa_amd.photometric import PhotometricDistort
    pd = None
    if case["seed"] is not None:
        np.random.seed(case["seed"])
        pd = PhotometricDistort().draw()
    return make_record(case["size"], np.array(case["a"]).reshape(2, 3), case["flip"], pd), pd


def cpu_pipeline(case):
    """What KITTI_Dataset.__getitem__ does to the image (kitti_dataset.py), with the product's classes and this machine's Pillow."""
    from monosowa_amd.photometric import PhotometricDistort
    img = Image.fromarray(case["raw"])
    if case["seed"] is not None:
        np.random.seed(case["seed"])
        img = Image.fromarray(PhotometricDistort()(np.array(img).astype(np.float32)).astype(np.uint8))
    if case["flip"]:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    img = img.transform(RESOLUTION, method=Image.AFFINE, data=case["a"], resample=Image.BILINEAR)
    return ((np.array(img).astype(np.float32) / 255.0 - MEAN) / STD).transpose(2, 0, 1)


def outside_fraction(case):
    """Share of output pixels whose source coordinate lies outside the image (PIL's black fill)."""
    a, (w, h) = case["a"], case["size"]
    X, Y = np.meshgrid(np.arange(RESOLUTION[0]) + 0.5, np.arange(RESOLUTION[1]) + 0.5)
    xin, yin = a[0] * X + a[1] * Y + a[2], a[3] * X + a[4] * Y + a[5]
    return float(((xin < 0) | (xin >= w) | (yin < 0) | (yin >= h)).mean())


def assert_cases_take_every_branch(cases):
    """The coverage the issue asks of the generated cases; every statement is about the INPUTS (draws, geometry, pre-cast values)."""
    from monosowa_amd.photometric import PhotometricDistort, _PERMS
    perms, first, taken, skipped = set(), set(), set(), set()
    negative = over = 0
    for case in cases:
        rec, pd = case_record(case)
        if pd is None:
            continue
        perms.add(pd["perm"])
        first.add(pd["contrast_first"])
        for k in ("brightness", "contrast", "saturation", "hue", "perm"):
            (skipped if pd[k] is None else taken).add(k)
        pre = PhotometricDistort.apply(case["raw"], pd)
        assert pre.dtype == np.float32 and np.isfinite(pre).all()
        assert pre.min() > -2.0 ** 31 and pre.max() < 2.0 ** 31          # the truncate-then-low-byte rule presumes the int32 range
        negative += int(pre.min() <= -1.0)
        over += int(pre.max() >= 256.0)
    assert perms == set(_PERMS) | {None}
    assert first == {True, False}
    assert taken == skipped == {"brightness", "contrast", "saturation", "hue", "perm"}
    assert negative >= 1 and over >= 1                                   # both wraps of astype(uint8) occur
    fills = [outside_fraction(c) for c in cases]
    assert sum(f > 0.05 for f in fills) >= 4 and sum(f == 0.0 for f in fills) >= 4
    assert {c["size"] for c in cases} == set(SIZES) and {c["flip"] for c in cases} == {True, False}
    assert sum(c["seed"] is not None for c in cases) >= 48


def test_generated_cases_take_every_branch():
    assert_cases_take_every_branch(generated_cases())


def test_prepare_reference_equals_the_cpu_pipeline_on_generated_cases():
    """Item 3: ``prepare_reference`` == PhotometricDistort -> astype(uint8) -> transpose -> transform -> normalise, every element."""
    from monosowa_amd.image_prep import prepare_reference
    for i, case in enumerate(generated_cases()):
        rec, _ = case_record(case)
        got, want = prepare_reference(case["raw"], rec), cpu_pipeline(case)
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (3, 384, 1280)
        assert np.array_equal(got, want), (i, case["size"], case["flip"], case["seed"], int((got != want).sum()))


def test_wrapping_cast_is_what_astype_uint8_does_here():
    from monosowa_amd.photometric import wrap_to_uint8
    x = np.array([-3.7, -0.5, 255.9, 256.0, 300.2, -300.2, 511.5], dtype=np.float32)
    assert wrap_to_uint8(x).tolist() == [253, 0, 255, 0, 44, 212, 255]
    with np.errstate(invalid="ignore"):
        assert x.astype(np.uint8).tolist() == [253, 0, 255, 0, 44, 212, 255]
    y = np.random.default_rng(3).uniform(-600, 900, 100000).astype(np.float32)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(wrap_to_uint8(y), y.astype(np.uint8))


def test_collate_pads_mixed_sizes_to_one_canvas():
    """Item 4, first half: images of different sizes -> one zero canvas, each in the top-left corner; the rest default-collated."""
    from monosowa_amd.image_prep import RECORD_DOUBLES, collate_raw, is_raw_batch, make_record
    rng = np.random.default_rng(5)
    sizes = ((31, 17), (40, 12), (8, 25))
    samples = []
    for i, (w, h) in enumerate(sizes):
        raw = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
        info = {"img_id": i, "img_size": np.array([w, h]), "prep": make_record((w, h), np.eye(2, 3), i == 1)}
        samples.append((raw, np.full((3, 4), i, np.float32), {"labels": np.zeros(50, np.int8), "mask_2d": np.zeros(50, bool)}, info))
    canvas, calibs, targets, info = collate_raw(samples)
    assert is_raw_batch(canvas) and canvas.shape == (3, 25, 40, 3) and canvas.dtype == torch.uint8
    for i, (w, h) in enumerate(sizes):
        assert np.array_equal(canvas[i, :h, :w].numpy(), samples[i][0])
        assert int(canvas[i, h:].sum()) == 0 and int(canvas[i, :, w:].sum()) == 0
    assert calibs.shape == (3, 3, 4) and targets["labels"].shape == (3, 50) and targets["mask_2d"].dtype == torch.bool
    assert info["prep"].shape == (3, RECORD_DOUBLES) and info["prep"].dtype == torch.float64 and info["img_id"].tolist() == [0, 1, 2]
    assert info["prep"][:, 0].tolist() == [31, 40, 8] and info["prep"][:, 8].tolist() == [0, 1, 0]
    assert not is_raw_batch(torch.zeros(3, 3, 384, 1280))
    # the test split's (image, P2, image, info)
    again = collate_raw([(s[0], s[1], s[0], s[3]) for s in samples])
    assert len(again) == 4 and again[2] is again[0] and torch.equal(again[0], canvas)


def test_raw_loader_batches_feed_the_training_step_contract(kitti):
    """Item 4, second half: the loader contract of test_loader_batches_feed_the_training_step_contract in raw mode, then
    ``prepare_reference`` (through ``stage_batch`` on the CPU as well) -> [3, 3, 384, 1280] float32 equal to the default loader's."""
    from monosowa_amd.helpers.dataloader_helper import build_dataloader
    from monosowa_amd.helpers.trainer_helper import stage_batch
    from monosowa_amd.image_prep import collate_raw, is_raw_batch, prepare_reference
    from monosowa_amd.synthetic import prepare_targets
    fixtures, root = kitti
    cfg = fixture_cfg(fixtures, "kitti_dataset.npz", root, type="KITTI", train_split="train", test_split="val", batch_size=3)
    _, default_loader = build_dataloader(cfg, workers=0)
    train_loader, test_loader = build_dataloader(dict(cfg, device_aug=True), workers=0)
    assert default_loader.collate_fn is not collate_raw and test_loader.collate_fn is collate_raw and train_loader.collate_fn is collate_raw
    want_inputs, want_calibs, want_targets, want_info = next(iter(default_loader))
    raw, calibs, targets, info = next(iter(test_loader))
    assert is_raw_batch(raw) and raw.shape[0] == 3 and calibs.shape == (3, 3, 4) and torch.equal(calibs, want_calibs)
    assert targets["boxes_3d"].shape == (3, 50, 6) and targets["labels"].dtype == torch.int8 and targets["mask_2d"].dtype == torch.bool
    tl = prepare_targets(targets, 3)
    assert len(tl) == 3 and all(set(t) >= {"labels", "boxes", "boxes_3d", "depth", "size_3d", "heading_bin", "heading_res"} for t in tl)
    assert sum(len(t["labels"]) for t in tl) == int(targets["mask_2d"].sum())
    assert set(targets) == set(want_targets) and all(torch.equal(targets[k], want_targets[k]) for k in targets)
    assert all(torch.equal(torch.as_tensor(info[k]), torch.as_tensor(want_info[k])) for k in want_info)
    got = prepare_reference(raw, info["prep"])
    assert got.dtype == np.float32 and got.shape == (3, 3, 384, 1280) and np.array_equal(got, want_inputs.numpy())
    staged = stage_batch((raw, calibs, targets, info), torch.device("cpu"))
    assert staged[0].dtype == torch.float32 and torch.equal(staged[0], want_inputs)
    # a shuffled train batch through workers' code path (collate inside the loader) has the same contract
    np.random.seed(7)
    torch.manual_seed(7)
    raw, _, _, info = next(iter(train_loader))
    assert is_raw_batch(raw) and info["prep"].shape == (3, 16)


def test_default_mode_is_untouched_by_the_key(kitti):
    """The key off or absent: the same class of batch as before (float32 images from the default collate), no record."""
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    fixtures, root = kitti
    for extra in ({}, {"device_aug": False}):
        ds = KITTI_Dataset("val", fixture_cfg(fixtures, "kitti_dataset.npz", root, **extra))
        img, _, _, info = ds[0]
        assert img.dtype == np.float32 and img.shape == (3, 384, 1280) and "prep" not in info
    import yaml
    with open(os.path.join(ROOT, "configs", "monodetr.yaml")) as f:
        assert "device_aug" not in yaml.safe_load(f)["dataset"]


def test_photometric_draw_consumes_the_stream_like_call():
    """``draw()`` + ``apply()`` is ``__call__``: same result, same state of numpy's stream afterwards."""
    from monosowa_amd.photometric import PhotometricDistort
    pd = PhotometricDistort()
    image = np.random.default_rng(1).uniform(0, 255, (9, 11, 3)).astype(np.float32)
    for seed in range(40):
        np.random.seed(seed)
        out = pd(image)
        state = np.random.get_state()[1].copy()
        np.random.seed(seed)
        rec = pd.draw()
        assert np.array_equal(np.random.get_state()[1], state)
        assert np.array_equal(pd.apply(image, rec), out)


# ---------------------------------------------------------------------------------------------------------------------------------
# item 5: the library
def test_image_library_exports_exactly_what_the_header_declares():
    from monosowa_amd import build, image_prep
    text = open(os.path.join(ROOT, "include", "monosowa_image.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"#define MONO_IMAGE_([A-Z_]+) (\d+)", text)}
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(mono_image_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(image_prep.SYMBOLS) and len(names) == 2
    lib = ctypes.CDLL(image_prep._PATH)
    for n in names:
        assert hasattr(lib, n)
    exported = subprocess.run(["nm", "-D", "--defined-only", image_prep._PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\b(mono_[a-z0-9_]+)\b", exported))) == names
    # the Python mirror of the record layout and of the flag bits
    assert image_prep.load().mono_image_record_doubles() == image_prep.RECORD_DOUBLES == flags.pop("RECORD_DOUBLES")
    assert flags == {"FLIP": image_prep.FLIP, "PD": image_prep.PD, "BRIGHTNESS": image_prep.BRIGHTNESS, "CONTRAST_FIRST": image_prep.CONTRAST_FIRST,
                     "CONTRAST": image_prep.CONTRAST, "SATURATION": image_prep.SATURATION, "HUE": image_prep.HUE, "PERMUTE": image_prep.PERMUTE}
    # argument checks come before any device work
    f = image_prep.load().mono_image_prep_f32
    assert f(None, None, None, None, 1, 1, 1, 4, 4, None) == -1
    one = ctypes.c_void_p(16)
    assert f(one, one, one, one, 1, 8, 8, 4, 6, None) == -2 and f(one, one, one, one, 0, 8, 8, 4, 4, None) == -2
    # the build knows the library, keeps the FMA contraction off for it alone, and the binary is the committed source's
    tu, extra = build.LIBS["libmonosowa_image.so"]
    assert tu == "image_prep.hip" and "-ffp-contract=off" in extra
    assert all("-ffp-contract=off" not in e for n, (_, e) in build.LIBS.items() if n != "libmonosowa_image.so") and "-ffp-contract=off" not in build.FLAGS
    assert build._recorded_hash(image_prep._PATH) == build.source_hash(["hipcc"] + build.FLAGS + extra)


def test_image_kernel_uses_no_scratch(tmp_path):
    """-Rpass-analysis=kernel-resource-usage of the translation unit as the build compiles it: no scratch, no spills."""
    from monosowa_amd import build
    tu, extra = build.LIBS["libmonosowa_image.so"]
    cmd = [build.hipcc()] + build.FLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "image.so"), os.path.join(build.CSRC, tu)]
    report = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    assert "image_prep_kernel" in report
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report) == ["0"]
    assert re.findall(r"VGPRs Spill: (\d+)", report) == ["0"] and re.findall(r"SGPRs Spill: (\d+)", report) == ["0"]


def test_prepare_on_a_cpu_device_is_the_reference_and_checks_its_arguments():
    from monosowa_amd.image_prep import make_record, prepare, prepare_reference
    raw = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (2, 20, 30, 3), dtype=np.uint8))
    rec = torch.from_numpy(np.stack([make_record((30, 20), [[0.02, 0, 0.1], [0, 0.05, 0.2]], False), make_record((25, 18), [[0.02, 0, -1], [0, 0.05, 0]], True)]))
    out = prepare(raw, rec, "cpu")
    assert out.dtype == torch.float32 and out.shape == (2, 3, 384, 1280) and np.array_equal(out.numpy(), prepare_reference(raw, rec))
    with pytest.raises(ValueError):
        prepare(raw.float(), rec, "cpu")
    with pytest.raises(ValueError):
        prepare(raw, rec[:, :8], "cpu")
    bad = rec.clone()
    bad[1, 0] = 31                                                      # wider than the canvas
    with pytest.raises(ValueError):
        prepare(raw, bad, "cpu")
