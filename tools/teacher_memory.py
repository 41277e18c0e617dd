"""The label memory of a checkpoint written with ``trainer.teacher_memory`` (monosowa_amd/teacher_memory.py): the refined pseudo-label
set of the run, as KITTI label files for the next round, or in numbers.

    python tools/teacher_memory.py export  --checkpoint FILE --out DIR [--dontcare-below X] [--min-hits H]
    python tools/teacher_memory.py summary --checkpoint FILE

``export`` writes one label file per remembered frame through ``write_kitti_results`` -- the Detector's own writer, so the bytes are
the ones it would write for the same rows: column 13 is the smoothed score, rows scoring below ``--dontcare-below`` become DontCare
lines, rows seen in fewer than ``--min-hits`` passes are left out.  The class names are KITTI_Dataset's.  ``summary`` prints the number of frames and entries and the quantiles of the smoothed score, ``hits``
and ``misses``."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch   # noqa: E402

QUANTILES = (0.0, 0.25, 0.5, 0.75, 1.0)


def read_memory(checkpoint):
    """-> (ids [N], bank float64 [N, M, 16], count [N]) of a checkpoint's ``teacher_memory``; KeyError when it has none."""
    state = torch.load(checkpoint, map_location="cpu", weights_only=False)
    if state.get("teacher_memory") is None:
        raise KeyError("checkpoint '%s' has no 'teacher_memory': it was written without trainer.teacher_memory" % checkpoint)
    m = state["teacher_memory"]
    bank = m["bank"].numpy()
    return [int(i) for i in torch.as_tensor(m["ids"]).tolist()], bank, np.clip(m["count"].numpy(), 0, bank.shape[1])


def remembered_rows(ids, bank, count, min_hits=0):
    """{img_id: float64 [n, 14]}: every frame's entries with ``hits >= min_hits``, in slot order (score descending)."""
    out = {}
    for i, frame, n in zip(ids, bank, count):
        entries = frame[:int(n)]
        out[i] = entries[entries[:, 14] >= min_hits][:, :14]
    return out


def class_names():
    from monosowa_amd.kitti_dataset import KITTI_Dataset
    return list(KITTI_Dataset.settings({}).class_name)


def export(args):
    from monosowa_amd.helpers.tester_helper import write_kitti_results
    ids, bank, count = read_memory(args.checkpoint)
    rows = remembered_rows(ids, bank, count, args.min_hits)
    write_kitti_results(rows, class_names(), args.out, dontcare_below=args.dontcare_below)
    print(json.dumps({"frames": len(rows), "rows": int(sum(len(r) for r in rows.values())), "out": args.out}))


def summary(args):
    ids, bank, count = read_memory(args.checkpoint)
    entries = np.concatenate([frame[:int(n)] for frame, n in zip(bank, count)]) if len(ids) else np.zeros((0, 16))
    out = {"frames": len(ids), "frames_with_entries": int((count > 0).sum()), "entries": int(len(entries)), "slots": int(bank.shape[1]),
           "quantiles": list(QUANTILES)}
    for name, col in (("score", 13), ("hits", 14), ("misses", 15)):
        out[name] = [float(v) for v in np.quantile(entries[:, col], QUANTILES)] if len(entries) else None
    print(json.dumps(out))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    e = sub.add_parser("export")
    e.add_argument("--checkpoint", required=True)
    e.add_argument("--out", required=True)
    e.add_argument("--dontcare-below", type=float, default=None)
    e.add_argument("--min-hits", type=int, default=0)
    e.set_defaults(run=export)
    s = sub.add_parser("summary")
    s.add_argument("--checkpoint", required=True)
    s.set_defaults(run=summary)
    args = ap.parse_args(argv)
    args.run(args)


if __name__ == "__main__":
    main()
