"""The label audit's records (``trainer.label_audit``, monosowa_amd/label_audit.py) from the command line.

    python tools/label_audit.py report DIR [--last E] [--by COLUMN] [--top N] [--csv FILE]
    python tools/label_audit.py scan --config CFG --checkpoint FILE [--weights ema] [--split SPLIT] [--out FILE] [--workers N]
    python tools/label_audit.py weights DIR --out FILE [--last E] [--by COLUMN] (--huber X | --drop-above X)

``report`` merges the ``epoch_NNN.npz`` / ``epoch_NNN.rankR.npz`` files of ``DIR`` (``<output_dir>/label_audit``): every column is
averaged per ``(img_id, line)`` over the rows of the last ``E`` epochs found (all of them by default; ``count`` is the mean number of
pairs per sighting, ``seen`` the number of sightings), the labels are ranked by ``--by`` (default ``depth_abs``, largest first, NaN in
front), written to a CSV (default ``DIR/report.csv``) and the top ``N`` printed.

``scan`` audits a label set with a trained checkpoint: one pass of ``LabelAudit.scan`` in eval mode over ``--split`` (default: the
config's ``train_split``), every label paired with one query, into one ``.npz`` that ``report`` reads too.

``weights`` turns ``report``'s per-label means of ``--by`` into the CSV that ``dataset.label_weights`` reads (``img_id,line,weight``):
``--huber X`` gives 1 where the value is <= X and X / value beyond it (the IRLS weight that bounds an L1 term at X), ``--drop-above X``
gives 0 where the value is > X and 1 elsewhere; a NaN value gives 0; X must be positive.

The terms are measured in the frame of the step's augmentation (flip, crop, canonical depth), and only labels that pass the dataset's
filter and ``mask_2d`` ever appear."""
import argparse
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402

_FILE = re.compile(r"^epoch_(\d+)(?:\.rank(\d+))?\.npz$")


def epoch_files(directory):
    """{epoch: [paths of that epoch's files, rank order]} of a ``label_audit`` directory."""
    found = {}
    for name in sorted(os.listdir(directory)):
        m = _FILE.match(name)
        if m:
            found.setdefault(int(m.group(1)), []).append(os.path.join(directory, name))
    return found


def merge(paths):
    """The rows of several record files under one another."""
    parts = [np.load(p, allow_pickle=False) for p in paths]
    columns = [str(c) for c in parts[0]["columns"]]
    for p, part in zip(paths, parts):
        if [str(c) for c in part["columns"]] != columns:
            raise ValueError("%s has other columns than %s" % (p, paths[0]))
    out = {k: np.concatenate([part[k] for part in parts]) for k in ("img_id", "line", "cls", "values")}
    out["columns"] = columns
    return out


def report(directory, last=None, by="depth_abs"):
    """-> (columns, rows): one row per (img_id, line), the mean of every column over its sightings in the last ``last`` epochs, ranked by
    ``by`` (largest first, NaN in front).  A row: {"img_id", "line", "cls", "seen", <column>: mean ...}."""
    files = epoch_files(directory)
    if not files:
        raise FileNotFoundError("no epoch_NNN.npz in %s" % directory)
    epochs = sorted(files)
    if last is not None:
        if last < 1:
            raise ValueError("--last must be at least 1")
        epochs = epochs[-last:]
    data = merge([p for e in epochs for p in files[e]])
    columns = data["columns"]
    if by not in columns:
        raise ValueError("--by %r is not one of %s" % (by, ", ".join(columns)))
    keys = np.stack([data["img_id"].astype(str), data["line"].astype(str)], 1)
    uniq, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    seen = np.bincount(inverse, minlength=len(uniq))
    means = np.zeros((len(uniq), len(columns)))
    np.add.at(means, inverse, data["values"])
    means /= seen[:, None]
    score = means[:, columns.index(by)]
    order = np.lexsort((data["line"][first], data["img_id"][first], -np.nan_to_num(score, nan=np.inf)))
    rows = []
    for i in order:
        row = {"img_id": data["img_id"][first[i]].item(), "line": int(data["line"][first[i]]), "cls": int(data["cls"][first[i]]),
               "seen": int(seen[i])}
        row.update({c: float(v) for c, v in zip(columns, means[i])})
        rows.append(row)
    return columns, rows


def write_csv(path, columns, rows):
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["img_id", "line", "cls", "seen"] + list(columns))
        w.writeheader()
        w.writerows(rows)


def _report(args):
    columns, rows = report(args.dir, args.last, args.by)
    path = args.csv or os.path.join(args.dir, "report.csv")
    write_csv(path, columns, rows)
    print("%d labels, ranked by %s -> %s" % (len(rows), args.by, path))
    print("%12s %5s %4s %5s  " % ("img_id", "line", "cls", "seen") + " ".join("%10s" % c for c in columns))
    for r in rows[:args.top]:
        print("%12s %5d %4d %5d  " % (r["img_id"], r["line"], r["cls"], r["seen"]) + " ".join("%10.4g" % r[c] for c in columns))


def label_weights(values, huber=None, drop_above=None):
    """The weight of every per-label value: ``huber`` X -> 1 where value <= X else X / value; ``drop_above`` X -> 0 where value > X
    else 1; NaN -> 0.  Exactly one of the two, X > 0."""
    if (huber is None) == (drop_above is None):
        raise ValueError("give exactly one of --huber and --drop-above")
    x = float(huber if huber is not None else drop_above)
    if not x > 0 or not np.isfinite(x):
        raise ValueError("the threshold of --huber / --drop-above must be positive and finite, got %r" % (x,))
    v = np.asarray(values, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(v <= x, 1.0, x / v) if huber is not None else np.where(v > x, 0.0, 1.0)
    return np.where(np.isnan(v), 0.0, w)


def write_weights(path, rows, weights):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["img_id", "line", "weight"])
        for r, x in zip(rows, weights):
            w.writerow([r["img_id"], r["line"], repr(float(x))])


def _weights(args):
    _, rows = report(args.dir, args.last, args.by)
    w = label_weights([r[args.by] for r in rows], args.huber, args.drop_above)
    write_weights(args.out, rows, w)
    print("%d labels by %s -> %s: %d at weight 1, %d at weight 0, %d between" % (
        len(rows), args.by, args.out, int((w == 1).sum()), int((w == 0).sum()), int(((w > 0) & (w < 1)).sum())))


def _scan(args):
    from monosowa_amd import miopen_tuning
    miopen_tuning.use_shipped_db(0)
    import torch
    import yaml
    from torch.utils.data import DataLoader
    from monosowa_amd.helpers.dataloader_helper import build_dataset
    from monosowa_amd.helpers.model_helper import build_model
    from monosowa_amd.helpers.save_helper import load_checkpoint
    from monosowa_amd.label_audit import LabelAudit, save
    cfg = yaml.load(open(args.config, "r"), Loader=yaml.Loader)
    device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    model, criterion = build_model(cfg["model"])
    model = model.to(device)
    criterion.to(device)
    res = cfg["dataset"].get("resolution", (1280, 384))
    criterion.depth_map_size = (res[0] // 16, res[1] // 16)
    if device.type == "cuda":
        from monosowa_amd.helpers.model_helper import to_mi355x_layout
        to_mi355x_layout(model)
    load_checkpoint(model, None, args.checkpoint, device, weights=args.weights)
    dataset = build_dataset(cfg["dataset"], args.split or cfg["dataset"]["train_split"])
    collate = None
    if getattr(dataset, "device_aug", False):
        from monosowa_amd.image_prep import collate_raw as collate
    loader = DataLoader(dataset, batch_size=cfg["dataset"]["batch_size"], num_workers=args.workers, shuffle=False,
                        pin_memory=device.type == "cuda", drop_last=False, collate_fn=collate)
    audit = LabelAudit(max(len(dataset) * int(getattr(dataset, "max_objs", 50)), 1), device)
    record = audit.scan(model, criterion, loader, device)
    out = args.out or os.path.join(os.path.dirname(os.path.abspath(args.checkpoint)), "label_audit", "epoch_000.npz")
    save(out, record)
    err = record["values"][:, list(record["columns"]).index("depth_abs")]
    print("%d labels -> %s" % (len(err), out) + (", |d - d*| median %.4g, max %.4g" % (np.median(err), np.max(err)) if len(err) else ""))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    r = sub.add_parser("report", help="rank the labels of a label_audit directory")
    r.add_argument("dir")
    r.add_argument("--last", type=int, default=None, help="epochs to average over, counted from the last one found (default: all)")
    r.add_argument("--by", default="depth_abs")
    r.add_argument("--top", type=int, default=20)
    r.add_argument("--csv", default=None)
    r.set_defaults(run=_report)
    s = sub.add_parser("scan", help="audit a label set with a checkpoint")
    s.add_argument("--config", required=True)
    s.add_argument("--checkpoint", required=True)
    s.add_argument("--weights", default="model", choices=("model", "ema"))
    s.add_argument("--split", default=None)
    s.add_argument("--out", default=None)
    s.add_argument("--workers", type=int, default=4)
    s.set_defaults(run=_scan)
    w = sub.add_parser("weights", help="per-label loss weights (dataset.label_weights) from a label_audit directory")
    w.add_argument("dir")
    w.add_argument("--out", required=True)
    w.add_argument("--last", type=int, default=None, help="epochs to average over, counted from the last one found (default: all)")
    w.add_argument("--by", default="depth_abs")
    how = w.add_mutually_exclusive_group(required=True)
    how.add_argument("--huber", type=float, default=None, metavar="X", help="weight 1 up to X, X / value beyond")
    how.add_argument("--drop-above", type=float, default=None, metavar="X", help="weight 0 beyond X, 1 up to it")
    w.set_defaults(run=_weights)
    args = ap.parse_args(argv)
    if args.command == "weights":
        x = args.huber if args.huber is not None else args.drop_above
        if not x > 0:
            ap.error("the threshold of --huber / --drop-above must be positive, got %r" % (x,))
    args.run(args)


if __name__ == "__main__":
    main()
