"""tests/criterion_reference.py against the layer-by-layer, image-by-image criterion (``SetCriterion(fast=False)``, pinned to the
reference class by test_criterion_equals_reference_class_cpu) in float64 on the CPU, at the KITTI-like target layouts that
tests/test_criterion_kernels_gpu.py runs on the GPU.  Both are float64 evaluations of the same sums in a different order:
1e-12 relative leaves four decimal digits over the double rounding of ~9,000-term sums."""
import os

import numpy as np
import pytest
import torch
import yaml

import criterion_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (targets per image, queries, train mode): the layouts of section 3 of tests/test_criterion_kernels_gpu.py
LAYOUTS = {
    "mixed_b8": ([0, 50, 1, 0, 23, 50, 7, 3], 550, True),
    "empty_batch": ([0, 0, 0], 550, True),
    "eval_q50": ([5, 0, 50], 50, False),
    "full_b16": ([50] * 16, 550, True),
    "one_target": ([1], 550, True),
}
SEEDS = {name: 100 + i for i, name in enumerate(LAYOUTS)}
REL = 1e-12


class _RecordingMatcher(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.calls = inner, []

    def forward(self, outputs, targets, group_num=11):
        found = self.inner(outputs, targets, group_num=group_num)
        self.calls.append(found)
        return found


def triples(calls, sizes):
    """the matcher's per-layer, per-image (queries, targets) -> idx [3, NL, K] (image, query, flat target)"""
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    per_layer = []
    for found in calls:
        b = torch.cat([torch.full_like(s, i) for i, (s, _) in enumerate(found)])
        q = torch.cat([s for s, _ in found])
        t = torch.cat([t + int(offs[i]) for i, (_, t) in enumerate(found)])
        per_layer.append(torch.stack([b, q, t]))
    return torch.stack(per_layer, 1)


def layerwise_criterion(train):
    from monosowa_amd.monodetr import build_weight_dict
    from monosowa_amd.monodetr.criterion import SetCriterion
    from monosowa_amd.monodetr.matcher import build_matcher
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))["model"]
    losses = ["labels", "boxes", "cardinality", "depths", "dims", "angles", "center", "depth_map", "tfl"]
    crit = SetCriterion(cfg["num_classes"], _RecordingMatcher(build_matcher(cfg)), build_weight_dict(cfg), cfg["focal_alpha"], losses,
                        cfg=cfg, fast=False)
    return crit.train(train)


def test_generated_layouts_keep_every_branch_quantity_off_zero():
    """the odd / even grids of the generator: no component or corner difference between ANY prediction and ANY target of its
    image is below 2**-14, so the condition holds for whatever pairs a matcher forms"""
    outputs, targets = CR.make_layout_case(SEEDS["mixed_b8"], LAYOUTS["mixed_b8"][0], 550)
    st = CR.stack_layers(outputs)
    for b, t in enumerate(targets):
        if not len(t["labels"]):
            continue
        p, g = st["pred_boxes"][:, b].double().reshape(-1, 1, 6), t["boxes_3d"].double().reshape(1, -1, 6)
        assert float((p - g).abs().min()) >= CR.H
        pc, gc = torch.stack(CR._xyxy(p), -1), torch.stack(CR._xyxy(g), -1)
        assert float((pc - gc).abs().min()) >= CR.H
        cross = torch.stack([pc[..., 2] - gc[..., 0], gc[..., 2] - pc[..., 0], pc[..., 3] - gc[..., 1], gc[..., 3] - pc[..., 1]])
        assert float(cross.abs().min()) >= CR.H                                  # the candidates of iw and ih
        assert float((st["pred_depth"][:, b, :, :1].double().reshape(-1, 1) - t["depth"].double().reshape(1, -1)).abs().min()) >= 2.0 ** -10
        assert float((st["pred_3d_dim"][:, b].double().reshape(-1, 1, 3) - t["size_3d"].double().reshape(1, -1, 3)).abs().min()) >= 2.0 ** -8
        assert float((st["pred_angle"][:, b, :, 12:].double().reshape(-1, 1) - t["heading_res"].double().reshape(1, -1)).abs().min()) >= 2.0 ** -12
    # and the float32 tensors hold the grid values exactly
    assert torch.equal((st["pred_boxes"].double() / CR.H).round() * CR.H, st["pred_boxes"].double())


def test_matched_case_generator_builds_every_geometry_class():
    for K, NL in ((255, 1), (1474, 3)):
        case = CR.make_matched_case(3, NL, 16, 550, K)
        cls, margins = CR.census(*[case[k] for k in CR.MATCHED_ARGS])
        shares = CR.class_shares(cls)
        assert all(shares[c] >= 0.05 for c in CR.CLASSES), shares
        assert shares["disjoint"] >= 0.25, shares
        assert min(margins.values()) >= CR.MARGIN, margins
        rows = case["idx"][0] * 550 + case["idx"][1]
        assert all(len(set(r.tolist())) == K for r in rows)                      # unique per (layer, image, query)
        assert NL == 1 or not torch.equal(rows[0], rows[1])


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_helper_equals_the_layerwise_criterion_in_float64(name):
    """every loss key and the gradient of the weighted total with respect to every prediction tensor.  The two logging keys
    are float32 in the layer-wise formulation (``.float()`` before the division): compared to float32 rounding."""
    sizes, Q, train = LAYOUTS[name]
    outputs, targets = CR.make_layout_case(SEEDS[name], sizes, Q)
    crit = layerwise_criterion(train)
    group_num = crit.group_num if train else 1
    num_boxes = max(float(sum(sizes) * group_num), 1.0)

    out_a, tg = CR.cast_case(outputs, targets, "cpu", torch.float64)
    want = crit(out_a, tg)
    idx = triples(crit.matcher.calls, sizes)
    assert idx.shape == (3, 3, group_num * sum(min(n, Q // group_num) for n in sizes))
    out_b, _ = CR.cast_case(outputs, targets, "cpu", torch.float64)
    got = CR.criterion_losses(out_b, tg, idx, num_boxes, crit.focal_alpha)

    assert set(got) == {k for k in want if not k.startswith(("loss_tfl", "loss_mask", "loss_depth_map"))}
    for k, v in got.items():
        w, v = float(want[k].detach()), float(v.detach())
        assert np.isfinite(v), (k, v)
        if k.startswith("class_error"):                   # float32 ``100 - accuracy``: rounded at the magnitude of 100
            assert abs(v - w) <= 2.0 ** -22 * 100.0, (k, v, w)
            continue
        rel = 2.0 ** -22 if k.startswith("cardinality_error") else REL
        assert abs(v - w) <= rel * max(abs(w), 1e-300), (k, v, w)

    weights = {k: float(crit.weight_dict[k]) for k in got if k in crit.weight_dict}
    assert len(weights) == 21                                                    # seven differentiable losses of three layers
    la, lb = CR.leaves_of(out_a), CR.leaves_of(out_b)
    names = [n for n in la if n != "depth_map_logits"]
    ga = torch.autograd.grad(sum(want[k] * w for k, w in weights.items()), [la[n] for n in names], allow_unused=True)
    gb = torch.autograd.grad(sum(got[k] * w for k, w in weights.items()), [lb[n] for n in names], allow_unused=True)
    for n, a, b in zip(names, ga, gb):
        a = torch.zeros_like(la[n]) if a is None else a
        b = torch.zeros_like(lb[n]) if b is None else b
        assert torch.isfinite(b).all(), n
        assert float((a - b).abs().max()) <= REL * float(a.abs().max()), (n, float((a - b).abs().max()), float(a.abs().max()))
        if sum(sizes):
            assert n.endswith("pred_logits") or float(a.abs().max()) > 0, n
