"""Reference of the label audit (monosowa_amd/label_audit.py, ``mono_label_audit_f32``) for the tests: the nine columns per label from
the formulas of tests/criterion_reference.py, label by label, and the cases the tests share.

``rows(case, layer, dtype)`` evaluates every per-pair term in ``dtype`` (float64: the oracle; float32: the same expressions at the
kernel's precision, from which the tests' bound is measured), widens it to float64, and takes the mean over the label's pairs in
float64."""
import numpy as np
import torch

import criterion_reference as CR

PRED = ("logits", "boxes", "depth", "dims", "angle")
TARGET = ("labels", "t_box", "t_depth", "t_size", "t_bin", "t_res")
TINY = 1e-30


def pair_terms(case, layer, dtype):
    """[K, 8]: the eight per-pair terms of ``layer``'s matched pairs, evaluated in ``dtype``."""
    idx = case["idx"]
    b, q, t = idx[0, layer], idx[1, layer], idx[2, layer]
    f = lambda x: x.to(dtype)
    take = lambda name: f(case[name])[layer][b, q]
    pb, tb = take("boxes"), f(case["t_box"])[t]
    center = (pb[:, 0] - tb[:, 0]).abs() + (pb[:, 1] - tb[:, 1]).abs()
    bbox = ((pb[:, 2] - tb[:, 2]).abs() + (pb[:, 3] - tb[:, 3]).abs()) + ((pb[:, 4] - tb[:, 4]).abs() + (pb[:, 5] - tb[:, 5]).abs())
    giou, _, _ = CR._giou(CR._xyxy(pb), CR._xyxy(tb))
    pd, td = take("depth"), f(case["t_depth"]).reshape(-1)[t]
    dabs = (pd[:, 0] - td).abs()
    dep = 1.4142 * torch.exp(-pd[:, 1]) * dabs + pd[:, 1]
    size = (take("dims") - f(case["t_size"])[t]).abs().sum(1)
    pa = take("angle")
    bins = case["t_bin"].reshape(-1).long()[t].view(-1, 1)
    ce = -torch.gather(torch.log_softmax(pa[:, 0:12], dim=1), 1, bins).squeeze(1)
    res = torch.gather(pa[:, 12:24], 1, bins).squeeze(1)
    ang = ce + (res - f(case["t_res"]).reshape(-1)[t]).abs()
    cls = case["labels"].reshape(-1).long()[t].view(-1, 1)
    score = torch.sigmoid(torch.gather(take("logits"), 1, cls).squeeze(1))
    return torch.stack([center, bbox, 1 - giou, dep, dabs, size, ang, score], 1)


def rows(case, layer, dtype=torch.float64):
    """[T, 9] float64: per label the means of ``pair_terms`` over its pairs and their number; nine zeros without a pair."""
    T = case["labels"].shape[0]
    terms = pair_terms(case, layer, dtype).double()
    t = case["idx"][2, layer]
    out = torch.zeros(T, 9, dtype=torch.float64)
    for label in range(T):
        mine = terms[t == label]
        if len(mine):
            out[label, :8] = mine.sum(0) / len(mine)
            out[label, 8] = len(mine)
    return out


def rel_error(got, ref):
    """worst |got - ref| / max(|ref|, 1e-30) over all elements"""
    got, ref = got.double().cpu(), ref.double().cpu()
    return float(((got - ref).abs() / ref.abs().clamp_min(TINY)).max()) if ref.numel() else 0.0


def make_case(seed, NL, B, Q, C, G, sizes):
    """Random predictions (every layer its own) and KITTI-like targets; every label of image b is paired, in every layer, with one
    query of each of the G query groups (Q / G queries each), pairs in (image, group) order and sorted by query inside a group -- the
    layout of the matcher's flat index tensor [3, NL, K]."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)
    randn = lambda *s: torch.randn(*s, generator=g)
    T, per = sum(sizes), Q // G
    assert max(sizes) <= per
    case = {"logits": 2.0 * randn(NL, B, Q, C) - 1.0,
            "boxes": torch.cat([0.2 + 0.6 * rand(NL, B, Q, 2), 0.02 + 0.18 * rand(NL, B, Q, 4)], -1),
            "depth": torch.stack([5.0 + 55.0 * rand(NL, B, Q), -0.5 + 2.0 * rand(NL, B, Q)], -1),
            "dims": torch.tensor([1.53, 1.63, 3.88]) + 0.3 * randn(NL, B, Q, 3),
            "angle": torch.cat([2.0 * randn(NL, B, Q, 12), 0.3 * randn(NL, B, Q, 12)], -1),
            "labels": torch.randint(0, C, (T,), generator=g),
            "t_box": torch.cat([0.2 + 0.6 * rand(T, 2), 0.02 + 0.18 * rand(T, 4)], -1),
            "t_depth": 5.0 + 55.0 * rand(T),
            "t_size": torch.tensor([1.53, 1.63, 3.88]) + 0.1 * randn(T, 3),
            "t_bin": torch.randint(0, 12, (T,), generator=g),
            "t_res": (rand(T) - 0.5) * (np.pi / 6)}
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    layers = []
    for _ in range(NL):
        bi, qi, ti = [], [], []
        for b, n in enumerate(sizes):
            for grp in range(G):
                queries = torch.sort(torch.randperm(per, generator=g)[:n]).values + grp * per
                bi.append(torch.full((n,), b, dtype=torch.int64))
                qi.append(queries)
                ti.append(torch.randperm(n, generator=g) + int(offs[b]))
        layers.append(torch.stack([torch.cat(bi), torch.cat(qi), torch.cat(ti)]))
    case["idx"] = torch.stack(layers, 1).contiguous()                    # [3, NL, K]
    assert case["idx"].shape == (3, NL, G * T)
    return case


def flat_of(case):
    """The case's targets under the names ``LabelAudit.observe`` reads them by."""
    return {"labels": case["labels"], "boxes_3d": case["t_box"], "depth": case["t_depth"].view(-1, 1), "size_3d": case["t_size"],
            "heading_bin": case["t_bin"].view(-1, 1), "heading_res": case["t_res"].view(-1, 1)}


def case_of_observe(args):
    """The positional arguments of one ``observe`` call (predictions, idx, flat) as a case on the CPU."""
    logits, boxes, depth, dims, angle, idx = [a.detach().cpu() for a in args[:6]]
    flat = {k: v.detach().cpu() for k, v in args[6].items()}
    return {"logits": logits, "boxes": boxes, "depth": depth, "dims": dims, "angle": angle, "idx": idx, "labels": flat["labels"].reshape(-1),
            "t_box": flat["boxes_3d"], "t_depth": flat["depth"].reshape(-1), "t_size": flat["size_3d"], "t_bin": flat["heading_bin"].reshape(-1),
            "t_res": flat["heading_res"].reshape(-1)}


# The tests' two cases: (NL, B, C, Q, G, labels per image)
CASES = {"G3": (3, 3, 3, 60, 3, (12, 0, 18)), "G1": (3, 3, 3, 50, 1, (1, 0, 2))}
_MADE = {}


def shared_case(name):
    """One of ``CASES``, made once per process and never changed (clone before editing)."""
    if name not in _MADE:
        NL, B, C, Q, G, sizes = CASES[name]
        _MADE[name] = make_case(51 + len(name) + sum(sizes), NL, B, Q, C, G, sizes)
    return _MADE[name]
