"""The first 3D pseudo-labels from object point clouds: a car template fitted to every object of every frame
(monosowa_amd/template_fit.py), written as KITTI label files.

    python tools/fit_labels.py --clouds DIR --template FILE(.npy|.obj) --out DIR [--config YAML] [--device cpu|cuda]
                               [--dontcare-below X]

``--clouds``: one ``<frame number>.npz`` per frame with ``P2`` [3, 4], ``img_size`` (width, height), ``points_<k>`` float [N_k, 3] for
k = 0, 1, ... in the KITTI camera frame, and optionally ``box2d`` [n, 4], ``moving`` [n] (0 / 1) and ``theta`` [n] (NaN: none).
``--template``: float [T, 3] points as ``.npy``, or a Wavefront ``.obj`` sampled by ``sample_mesh`` at the configuration's dimensions.
``--config``: a YAML file with the reference's sections (``optimization``, ``loss_functions``, ``templates``); absent keys take its
defaults.  The files go through ``write_kitti_results``, the Detector's own writer; the class names are KITTI_Dataset's and every
object is a Car.  Objects without points get no line."""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402

CLASS_NAMES = ["Pedestrian", "Car", "Cyclist"]


def read_frame(path):
    """-> (P2, img_size, clouds, box2d or None, moving or None, theta or None)"""
    with np.load(path, allow_pickle=False) as z:
        n = 0
        while "points_%d" % n in z.files:
            n += 1
        clouds = [np.asarray(z["points_%d" % k], dtype=np.float32).reshape(-1, 3) for k in range(n)]
        box2d = np.asarray(z["box2d"], dtype=np.float64).reshape(-1, 4) if "box2d" in z.files else None
        moving = [bool(m) for m in z["moving"]] if "moving" in z.files else None
        theta = [None if np.isnan(t) else float(t) for t in z["theta"]] if "theta" in z.files else None
        return np.asarray(z["P2"], dtype=np.float64).reshape(3, 4), [float(v) for v in z["img_size"]], clouds, box2d, moving, theta


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--clouds", required=True)
    ap.add_argument("--template", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--config")
    ap.add_argument("--device")
    ap.add_argument("--dontcare-below", type=float)
    args = ap.parse_args(argv)
    from monosowa_amd.helpers.tester_helper import write_kitti_results
    from monosowa_amd.template_fit import TemplateFitter, fit_config, sample_mesh
    cfg = None
    if args.config:
        import yaml
        with open(args.config) as f:
            cfg = yaml.safe_load(f)
    c = fit_config(cfg)
    if args.template.endswith(".obj"):
        template = sample_mesh(args.template, dims=(c.height, c.width, c.length))
    else:
        template = np.load(args.template, allow_pickle=False)
    fitter = TemplateFitter(template, cfg, device=args.device)
    results = {}
    for path in sorted(glob.glob(os.path.join(args.clouds, "*.npz"))):
        frame = int(os.path.splitext(os.path.basename(path))[0])
        P2, img_size, clouds, box2d, moving, theta = read_frame(path)
        fit = fitter.fit(clouds, moving=moving, theta=theta)
        results[frame] = fit.rows(P2, img_size, boxes2d=box2d, cls_id=CLASS_NAMES.index("Car")).tolist()
        print("%06d: %d objects, %d labels%s" % (frame, len(clouds), len(results[frame]), " (host)" if fit.host else ""))
    write_kitti_results(results, CLASS_NAMES, args.out, dontcare_below=args.dontcare_below)
    return 0


if __name__ == "__main__":
    sys.exit(main())
