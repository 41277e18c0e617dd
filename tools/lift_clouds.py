"""Object clouds from depth maps and instance masks (monosowa_amd/lift.py), written as the per-frame ``.npz`` files that
tools/fit_labels.py reads.

    python tools/lift_clouds.py --depth DIR --masks DIR --calib FILE [--poses FILE] [--tracks FILE | --track] [--config YAML]
                                --out DIR [--device cpu|cuda] [--max-points 16384]

``--depth``: one ``<frame number>.npy`` per frame, float [H, W], metric depth.  ``--masks``: the same names, ``.npy`` or ``.npz`` (key
``masks``), bool or uint8 [M_f, H, W]; frames may differ in M_f.  ``--calib``: ``P2`` as ``.npy`` [3, 4] or [F, 3, 4], or ``.npz``
with the key ``P2``; fx, fy, cx, cy are read from it.  Frames are taken in the order of their numbers.

Without ``--tracks`` every mask with status OK is its own object of its own frame, in that frame's camera coordinates, and one
``<frame number>.npz`` is written per frame.  With ``--tracks`` (``.npz``: ``tracks`` int [B, V, 2] of (frame index, mask) pairs, -1
where a row has fewer views, and optionally ``moving`` [B]) and ``--poses`` (``.npy`` [F, 3, 4] or [F, 4, 4], each frame to the
reference frame, whose index is ``frames_creation.nscans_before``), the views of a track are gathered (the ten best of a standing
track, the reference frame's of a moving one) and one file is written, for the reference frame; a track without an OK view there is
left out, as the reference leaves out objects that are not visible in the labelled frame.  ``box2d`` is the bounding box of the
object's mask in the frame the file belongs to.  ``--track`` (with ``--poses``, instead of ``--tracks``) finds the tracks itself
(monosowa_amd/track.py): lift, track and gather run back to back on the device, and the one file holds the kept tracks' clouds, ``box2d``
from each track's mask in the reference frame, ``moving`` and ``theta`` (the heading of a moving track, NaN: none); a kept track
without a view in the reference frame (possible only with ``use_pseudo_lidar: false``) has no such mask and is left out.  ``--config``: a YAML
file with the reference's sections."""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402


def _load(path, key):
    a = np.load(path, allow_pickle=False)
    if isinstance(a, np.lib.npyio.NpzFile):
        with a:
            return np.asarray(a[key])
    return a


def _numbered(folder, suffixes):
    found = {}
    for suffix in suffixes:
        for path in glob.glob(os.path.join(folder, "*" + suffix)):
            found[int(os.path.splitext(os.path.basename(path))[0])] = path
    return found


def mask_box(mask):
    """(x1, y1, x2, y2) of a bool mask [H, W]; zeros for an empty one"""
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    return [float(cols[0]), float(rows[0]), float(cols[-1]), float(rows[-1])] if rows.size else [0.0] * 4


def read_inputs(depth_dir, masks_dir, calib, poses):
    """-> (frame numbers, depth [F, H, W], masks bool [F, M, H, W], mask_count [F], P2 [F, 3, 4], poses [F, 3, 4] or None)"""
    depths, masks = _numbered(depth_dir, (".npy",)), _numbered(masks_dir, (".npy", ".npz"))
    if not depths or sorted(depths) != sorted(masks):
        raise SystemExit("--depth and --masks must hold the same, non-empty set of frame numbers")
    numbers = sorted(depths)
    depth = np.stack([np.asarray(np.load(depths[n], allow_pickle=False), dtype=np.float32) for n in numbers])
    per_frame = [np.asarray(_load(masks[n], "masks")) != 0 for n in numbers]
    F, (H, W) = len(numbers), depth.shape[1:]
    M = max([m.shape[0] for m in per_frame] + [1])
    stacked = np.zeros((F, M, H, W), dtype=bool)
    for f, m in enumerate(per_frame):
        if m.ndim != 3 or m.shape[1:] != (H, W):
            raise SystemExit("masks of frame %d have shape %s, the depth map %s" % (numbers[f], m.shape, (H, W)))
        stacked[f, :m.shape[0]] = m
    P2 = np.asarray(_load(calib, "P2"), dtype=np.float64)
    P2 = np.broadcast_to(P2.reshape(-1, 3, 4), (F, 3, 4)) if P2.size in (12, 12 * F) else None
    if P2 is None:
        raise SystemExit("--calib must hold P2 as [3, 4] or [%d, 3, 4]" % F)
    if poses is not None:
        poses = np.asarray(np.load(poses, allow_pickle=False), dtype=np.float64)
        if poses.shape not in ((F, 3, 4), (F, 4, 4)):
            raise SystemExit("--poses must be [%d, 3, 4] or [%d, 4, 4], got %s" % (F, F, poses.shape))
        poses = np.ascontiguousarray(poses[:, :3])
    return numbers, depth, stacked, np.array([m.shape[0] for m in per_frame], dtype=np.int32), P2, poses


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--depth", required=True)
    ap.add_argument("--masks", required=True)
    ap.add_argument("--calib", required=True)
    ap.add_argument("--poses")
    ap.add_argument("--tracks")
    ap.add_argument("--track", action="store_true")
    ap.add_argument("--config")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device")
    ap.add_argument("--max-points", type=int, default=16384)
    args = ap.parse_args(argv)
    if args.track and (args.tracks is not None or args.poses is None):
        ap.error("--track needs --poses and excludes --tracks")
    from monosowa_amd.lift import ObjectLifter, OK
    cfg = None
    if args.config:
        import yaml
        with open(args.config) as f:
            cfg = yaml.safe_load(f)
    numbers, depth, masks, mask_count, P2, poses = read_inputs(args.depth, args.masks, args.calib, args.poses)
    F, M, H, W = masks.shape
    intrinsics = np.stack([P2[:, 0, 0], P2[:, 1, 1], P2[:, 0, 2], P2[:, 1, 2]], axis=1)
    lifter = ObjectLifter(cfg, device=args.device, max_points=args.max_points)
    os.makedirs(args.out, exist_ok=True)

    def write(f, clouds, boxes, moving, theta=None):
        arrays = {"P2": P2[f], "img_size": np.array([W, H], dtype=np.float64), "box2d": np.asarray(boxes, dtype=np.float64).reshape(-1, 4),
                  "moving": np.asarray(moving, dtype=np.uint8)}
        if theta is not None:
            arrays["theta"] = np.asarray([np.nan if t is None else t for t in theta], dtype=np.float64)
        arrays.update({"points_%d" % k: c for k, c in enumerate(clouds)})
        np.savez(os.path.join(args.out, "%06d.npz" % numbers[f]), **arrays)
        print("%06d: %d objects, %d points" % (numbers[f], len(clouds), sum(len(c) for c in clouds)))

    if args.tracks is None and not args.track:
        res = lifter.lift(depth, intrinsics, masks, mask_count).numpy()         # each frame in its own coordinates: no pose
        for f in range(F):
            ok = [m for m in range(M) if (res["status"][f, m] & 7) == OK]
            write(f, [res["points"][f, m, :res["counts"][f, m]] for m in ok], [mask_box(masks[f, m]) for m in ok], [0] * len(ok))
        return 0
    ref = lifter.config.ref_frame
    if not 0 <= ref < F:
        raise SystemExit("the reference frame, index %d (frames_creation.nscans_before), is not among the %d frames" % (ref, F))
    if args.track:
        from monosowa_amd.track import ObjectTracker
        res = lifter.lift(depth, intrinsics, masks, mask_count, poses)
        tr = ObjectTracker(cfg, device=args.device).track(res)
        clouds, counts, _ = res.gather(*tr.gather_args())
        kept, moving, theta = tr.objects()                                      # the one wait
        clouds, counts, ref_mask = clouds.cpu().numpy(), counts.cpu().numpy(), tr.ref_mask[0].cpu().numpy()
        # a kept track without a view in the reference frame (a hidden standing car, kept when use_pseudo_lidar is false) has no
        # mask to take a box from: left out, as the --tracks path leaves out a track without an OK view there
        rows = [(b, mv, th) for b, mv, th in zip(kept, moving, theta) if counts[b] > 0 and ref_mask[b] >= 0]
        write(ref, [clouds[b, :counts[b]] for b, _, _ in rows], [mask_box(masks[ref, ref_mask[b]]) for b, _, _ in rows],
              [int(mv) for _, mv, _ in rows], [th for _, _, th in rows])
        return 0
    with np.load(args.tracks, allow_pickle=False) as z:
        tracks = np.asarray(z["tracks"], dtype=np.int32)
        moving = np.asarray(z["moving"]).astype(bool) if "moving" in z.files else np.zeros(tracks.shape[0], dtype=bool)
    res = lifter.lift(depth, intrinsics, masks, mask_count, poses)
    clouds, counts, _ = res.gather(tracks, moving)
    clouds, counts, status = clouds.cpu().numpy(), counts.cpu().numpy(), res.status.cpu().numpy()
    kept, boxes = [], []
    for b in range(tracks.shape[0]):
        here = [m for f, m in tracks[b].tolist() if f == ref and 0 <= m < M and (status[ref, m] & 7) == OK]
        if here and counts[b] > 0:
            kept.append(b)
            boxes.append(mask_box(masks[ref, here[0]]))
    write(ref, [clouds[b, :counts[b]] for b in kept], boxes, [int(moving[b]) for b in kept])
    return 0


if __name__ == "__main__":
    sys.exit(main())
