"""The loss side of a training step on the GPU against float64, with the inputs that real KITTI batches contain.

Section A -- the kernels of csrc/matched_losses.hip by themselves (``pointwise.matched_losses``, ``pointwise.focal_classification``)
against tests/criterion_reference.py evaluated in float64 (R); P is the same helper in float32 on the GPU.
Section B -- exact ties against the autograd conventions of the plain PyTorch formulation.
Section C -- the whole ``SetCriterion`` of configs/monodetr.yaml at KITTI-like target layouts, three ways: F float32 with every
switch of tests/fused_switches.py shipped, P float32 with every switch plain, R float64 plain; F's matching is recorded and
handed to P and R.

Metrics.  Loss values: |x - x_R| / max(|x_R|, tiny) per key.  Gradients: ``criterion_reference.row_error`` -- per ROW (one
(layer, image, query) slice of a prediction tensor, one pixel's 81 bins of the depth-map logits), the maximum over all rows,
relative to max(||g_R,row||, 1e-4 * the tensor's largest row norm); the floor is explained there and is the same for F and P.
Counts (class_error, cardinality_error): equal to the float64 value to float32 rounding of the final division (rtol 2**-22);
rows that are not matched: exactly 0.

Bounds.  One per tensor group: 4 x the worst e_P of the group (plain float32 against R on the MI355X, over every case of the
section), rounded up to one significant digit; F and P must both meet it.  The factor 4 covers another summation order and other
exp / log roundings in a kernel (the practice of tests/test_train_step_grads_gpu.py).  Measured worst e_F / e_P beside each.

Conditions on the inputs are asserted from the float64 evaluation before a kernel result is looked at: every quantity whose sign
selects a branch is at least 1e-6 away from zero for every matched pair (none may violate it), the geometry classes have their
shares, and the depth map's painted bins and foreground mask are identical in float32 and float64."""
import os

import numpy as np
import pytest
import torch
import yaml

import criterion_reference as CR
from detector_reference import _FrozenMatcher
from fused_switches import fused_switches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 1e-30
COUNT_RTOL = 2.0 ** -22

# Section A: worst e_F / worst e_P over the cases (in brackets the case of the worst e_P), and 4 x e_P before rounding up
A_VALUE = 1e-6         # 1.3e-7 / 2.4e-7 (K 1474, one layer), 9.4e-7: per-layer sums of the six matched losses
A_BOXES = 3e-6         # 3.0e-7 / 5.2e-7 (K 8800), 2.1e-6
A_DEPTH = 9e-7         # 2.0e-7 / 2.0e-7 (K 8800), 8.0e-7
A_DIMS = 1e-6          # 1.6e-7 / 2.4e-7 (K 1474), 9.4e-7
A_ANGLE = 7e-7         # 2.0e-7 / 1.7e-7 (K 8800), 6.9e-7
A_FOCAL_VALUE = 3e-7   # 1.2e-7 / 6.8e-8 (B * Q = 32768), 2.7e-7: per-layer focal sum
A_FOCAL_LOGITS = 8e-6  # 2.3e-6 / 1.9e-6 (B * Q = 32768), 7.7e-6
# Section C (the layouts and the two shapes beyond the focal kernel's limits)
C_LOSS = 6e-7          # 1.5e-7 / 1.5e-7 (eval; B * Q = 32768 + Q), 6.0e-7: every loss key and the weighted total
C_LOGITS = 2e-5        # 3.2e-6 / 3.3e-6 (16 x 50 targets), 1.3e-5
C_BOXES = 8e-7         # 1.7e-7 / 2.0e-7 (16 x 50 targets), 7.9e-7
C_DEPTH = 4e-6         # 6.8e-7 / 8.1e-7 (257 images), 3.2e-6
C_DIMS = 7e-7          # 1.6e-7 / 1.6e-7 (eval), 6.3e-7
C_ANGLE = 7e-7         # 2.3e-7 / 1.7e-7 (257 images), 6.7e-7
C_DEPTH_MAP = 2e-6     # 5.5e-7 / 4.4e-7 (16 x 50 targets), 1.7e-6
# the table at the end of this file lists every case


def _rel(x, ref):
    return abs(float(x) - float(ref)) / max(abs(float(ref)), TINY)


def _show(section, case, group, e_f, e_p, bound):
    print("\nMEASURED %s %-34s %-14s e_F %.3e  e_P %.3e  bound %.0e" % (section, case, group, e_f, e_p, bound))


def _node_names(roots):
    """type names of every autograd node reachable from ``roots``"""
    seen, kept, stack, names = set(), [], [t.grad_fn for t in roots if t.grad_fn is not None], set()
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        kept.append(fn)
        names.add(type(fn).__name__)
        stack.extend(nxt for nxt, _ in fn.next_functions)
    return names


# =================================================================================================== A: matched-pair kernels
# (K, NL, B, Q): one pass of the kernels' 256-thread loops and its neighbours, the training shape's usual and largest K,
# and eval-like shapes
_MATCHED_CASES = [(1, 1, 3, 50), (1, 3, 16, 550), (55, 3, 3, 50)] + \
    [(K, NL, 16, 550) for K in (255, 256, 257, 1474, 8800) for NL in (1, 3)]


def _upstream(NL, case_no):
    """go [NL, 6]: all entries differ, one is 0 and one negative (their places move with the case)"""
    go = (0.25 + 0.25 * torch.arange(NL * 6, dtype=torch.float64)).reshape(NL, 6)
    go[0, case_no % 6] = 0.0
    go[NL - 1, (case_no + 1) % 6] *= -1.0
    return go


@pytest.mark.parametrize("case_no", range(len(_MATCHED_CASES)), ids=["K%d_NL%d_B%d_Q%d" % c for c in _MATCHED_CASES])
def test_matched_pair_kernels_equal_float64(case_no):
    from monosowa_amd.pointwise import matched_losses
    K, NL, B, Q = _MATCHED_CASES[case_no]
    case = CR.make_matched_case(11 + case_no, NL, B, Q, K)
    cls, margins = CR.census(*[case[k] for k in CR.MATCHED_ARGS])
    shares = CR.class_shares(cls)
    print("\nK %d NL %d: shares %s\nmargins %s" % (K, NL, {k: round(v, 3) for k, v in shares.items()}, margins))
    assert min(margins.values()) >= CR.MARGIN, margins
    if K >= 255:
        assert all(shares[c] >= 0.05 for c in CR.CLASSES) and shares["disjoint"] >= 0.25, shares
    rows = (torch.arange(NL).view(NL, 1) * B + case["idx"][0]) * Q + case["idx"][1]
    assert rows.unique().numel() == NL * K                                       # the kernel's precondition
    go = _upstream(NL, case_no)
    names = ("boxes", "depth", "dims", "angle")

    def run(fn, dtype):
        args = [case[k].cuda() for k in CR.MATCHED_ARGS]
        args = [a.to(dtype) if a.is_floating_point() else a for a in args]
        leaves = [a.requires_grad_(True) for a in args[:4]]
        out = fn(*args)
        grads = torch.autograd.grad((out * go.to(device="cuda", dtype=out.dtype)).sum(), leaves)
        return out.detach(), dict(zip(names, grads))

    vF, gF = run(matched_losses, torch.float32)
    vP, gP = run(CR.matched_sums, torch.float32)
    vR, gR = run(CR.matched_sums, torch.float64)
    assert vF.shape == (NL, 6) and vF.dtype == torch.float32
    assert torch.isfinite(vF).all() and all(torch.isfinite(g).all() for g in gF.values())

    label = "K%d_NL%d_B%d_Q%d" % (K, NL, B, Q)
    e_f = max(_rel(vF[l, j], vR[l, j]) for l in range(NL) for j in range(6))
    e_p = max(_rel(vP[l, j], vR[l, j]) for l in range(NL) for j in range(6))
    _show("A", label, "value", e_f, e_p, A_VALUE)
    bad = [("value", e_f, e_p)] if max(e_f, e_p) > A_VALUE else []
    for n, bound in zip(names, (A_BOXES, A_DEPTH, A_DIMS, A_ANGLE)):
        e_f, e_p = CR.row_error(gF[n], gR[n]), CR.row_error(gP[n], gR[n])
        _show("A", label, n, e_f, e_p, bound)
        if max(e_f, e_p) > bound:
            bad.append((n, e_f, e_p))
    # rows that no triple names: exactly 0 in all four gradients (one memset, plain stores)
    free = torch.ones(NL * B * Q, dtype=torch.bool)
    free[rows.reshape(-1)] = False
    for n in names:
        g = gF[n].reshape(NL * B * Q, -1).cpu()
        assert (g[free] == 0).all(), n
        assert (gR[n].reshape(NL * B * Q, -1).cpu()[free] == 0).all()
    assert not bad, "(group, e_F, e_P) beyond the bound: %s" % bad


# =================================================================================================== A: focal kernels
_MIXED_SIZES = [0, 50, 1, 0, 23, 50, 7, 3, 0, 12, 2, 0, 31, 5, 0, 9]
# name -> (NL, B, Q, sizes, groups, alpha, gamma, share of matched queries whose target class is planted as their arg-max)
_FOCAL_CASES = {
    "train_alpha.25_gamma2": (3, 16, 550, _MIXED_SIZES, 11, 0.25, 2.0, 0.0),
    "train_no_alpha": (3, 16, 550, _MIXED_SIZES, 11, -1.0, 2.0, 0.0),
    "train_gamma1.5_powf": (3, 16, 550, _MIXED_SIZES, 11, 0.25, 1.5, 0.0),
    "train_mostly_right": (3, 16, 550, _MIXED_SIZES, 11, 0.25, 2.0, 0.95),
    "eval_q50": (3, 3, 50, [5, 0, 50], 1, 0.25, 2.0, 0.0),
    "one_layer_one_target": (1, 1, 550, [1], 11, 0.25, 2.0, 0.0),
    "limit_cells_32768": (3, 64, 512, [(7 * i) % 11 if i % 4 else 0 for i in range(63)] + [50], 10, 0.25, 2.0, 0.0),
    "limit_images_256": (2, 256, 128, [i % 5 if i % 3 else 0 for i in range(255)] + [50], 2, 0.25, 2.0, 0.5),
}


def _focal_inputs(name):
    NL, B, Q, sizes, groups, alpha, gamma, right = _FOCAL_CASES[name]
    case = CR.make_focal_case(31 + list(_FOCAL_CASES).index(name), NL, B, Q, sizes, groups)
    idx, labels = case["idx"], case["labels"]
    K = idx.shape[2]
    if right:                                   # a trained model's class error is small: most matched queries name their target's class
        lay = torch.arange(NL).view(NL, 1).expand(NL, K)
        hit = torch.rand(NL, K, generator=torch.Generator().manual_seed(5)) < right
        boost = torch.zeros(NL, K, 3)
        boost.scatter_(2, labels[idx[2]].unsqueeze(-1), 12.0)
        case["logits"][lay[hit], idx[0][hit], idx[1][hit]] += boost[hit]
    return case, alpha, gamma


@pytest.mark.parametrize("name", list(_FOCAL_CASES))
def test_focal_kernels_equal_float64(name):
    from monosowa_amd.pointwise import focal_classification, focal_classification_supported
    case, alpha, gamma = _focal_inputs(name)
    NL, B, Q, sizes = _FOCAL_CASES[name][:4]
    assert set(case["labels"].tolist()) == {0, 1, 2} or sum(sizes) < 3
    if B >= 16:
        assert sum(1 for n in sizes if n == 0) >= 3 and max(sizes) == 50
    lg = case["logits"]
    assert (lg == 90).any() and (lg == -90).any() and (lg == 30).any() and (lg == -30).any()
    assert ((lg[..., 1] == lg[..., 2]) & (lg[..., 1] > lg[..., 0])).any()      # a tie of the maximum with the last class
    assert ((lg[..., 0] == lg[..., 1]) & (lg[..., 0] > lg[..., 2])).any()
    go = torch.tensor([[0.5, 3.0, 7.0], [-1.25, 5.0, 11.0], [2.0, 13.0, 17.0]], dtype=torch.float64)[:NL]

    def run(fn, dtype):
        logits = case["logits"].cuda().to(dtype).requires_grad_(True)
        out = fn(logits, case["idx"].cuda(), case["labels"].cuda(), case["sizes"].cuda().to(dtype), alpha, gamma)
        (grad,) = torch.autograd.grad((out * go.to(device="cuda", dtype=out.dtype))[:, 0].sum(), [logits])
        return out.detach(), grad

    assert focal_classification_supported(case["logits"].cuda(), case["idx"].cuda())
    vF, gF = run(focal_classification, torch.float32)
    vP, gP = run(CR.focal_sums, torch.float32)
    vR, gR = run(CR.focal_sums, torch.float64)
    assert vF.shape == (NL, 3) and torch.isfinite(vF).all() and torch.isfinite(gF).all()
    print("\n%s: class_error F %s R %s, cardinality_error F %s R %s" % (name, vF[:, 1].tolist(), vR[:, 1].tolist(), vF[:, 2].tolist(),
                                                                         vR[:, 2].tolist()))
    e_f = max(_rel(vF[l, 0], vR[l, 0]) for l in range(NL))
    e_p = max(_rel(vP[l, 0], vR[l, 0]) for l in range(NL))
    _show("A", name, "focal value", e_f, e_p, A_FOCAL_VALUE)
    g_f, g_p = CR.row_error(gF, gR), CR.row_error(gP, gR)
    _show("A", name, "focal logits", g_f, g_p, A_FOCAL_LOGITS)
    for l in range(NL):                                      # counts
        for j, what in ((1, "class_error"), (2, "cardinality_error")):
            assert abs(float(vF[l, j]) - float(vR[l, j])) <= COUNT_RTOL * abs(float(vR[l, j])), (what, l, float(vF[l, j]), float(vR[l, j]))
    assert max(e_f, e_p) <= A_FOCAL_VALUE and max(g_f, g_p) <= A_FOCAL_LOGITS, (e_f, e_p, g_f, g_p)


# =================================================================================================== the whole criterion
_CRIT = {}


def _criterion(train=True):
    """the shipped criterion (weights, alpha, group count of configs/monodetr.yaml) behind a matcher that replays its first matching"""
    from monosowa_amd.helpers.model_helper import build_model
    if "cfg" not in _CRIT:
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
        _CRIT["cfg"] = dict(cfg["model"], device="cuda", pretrained=False)
    _, crit = build_model(_CRIT["cfg"])
    assert crit.fast and crit.group_num == 11 and crit.focal_alpha == 0.25
    crit.matcher = _FrozenMatcher(crit.matcher)
    return crit.cuda().train(train)


class _GivenMatcher(torch.nn.Module):
    """hands out the triples it was given (section B: hand-written pairs)"""
    def __init__(self, idx):
        super().__init__()
        self.idx = idx

    def match_layers_begin(self, *args, **kwargs):
        return None

    def match_layers_end_flat(self, handle):
        return self.idx.numpy().copy()


def _evaluate(crit, outputs, targets, on, dtype):
    """-> (loss values by key, total, gradients by leaf name (zeros where the graph does not reach), autograd node names)"""
    from monosowa_amd.monodetr.criterion import weighted_total
    with fused_switches(on):
        out, tg = CR.cast_case(outputs, targets, "cuda", dtype)
        losses = crit(out, tg)
        total = weighted_total(losses, crit.weight_dict)
        nodes = _node_names([total])
        leaves = CR.leaves_of(out)
        grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
        grads = {n: (torch.zeros_like(v) if g is None else g).detach() for (n, v), g in zip(leaves.items(), grads)}
        values = {k: float(losses[k].detach()) for k in losses.keys()}
    return values, float(total.detach()), grads, nodes


_KERNEL_NODES = {"_MatchedLossesBackward", "_FocalClassificationBackward", "_DDNLossBackward"}
_GROUPS = (("pred_logits", "logits"), ("pred_boxes", "boxes"), ("pred_depth", "depth"), ("pred_3d_dim", "dims"), ("pred_angle", "angle"),
           ("depth_map_logits", "depth map"))


def _bounds_c():
    return {"logits": C_LOGITS, "boxes": C_BOXES, "depth": C_DEPTH, "dims": C_DIMS, "angle": C_ANGLE, "depth map": C_DEPTH_MAP}


def _rows(name, g):
    return g.permute(0, 2, 3, 1) if name == "depth_map_logits" else g               # a pixel's 81 bins last


def _compare(label, runs, ref_values, ref_total, ref_grads):
    """runs: {"F": (values, total, grads), "P": ...} against the float64 reference; prints every figure, then asserts"""
    (vF, tF, gF), (vP, tP, gP) = runs["F"], runs["P"]
    bad = []
    assert set(vF) == set(vP) and set(ref_values) <= set(vF), set(vF) ^ set(ref_values)
    diff = [k for k in ref_values if not k.startswith(("class_error", "cardinality_error"))]
    e_f = max([_rel(vF[k], ref_values[k]) for k in diff] + [_rel(tF, ref_total)])
    e_p = max([_rel(vP[k], ref_values[k]) for k in diff] + [_rel(tP, ref_total)])
    _show("C", label, "loss", e_f, e_p, C_LOSS)
    if max(e_f, e_p) > C_LOSS:
        bad.append(("loss", e_f, e_p, sorted((_rel(vF[k], ref_values[k]), k) for k in diff)[-3:]))
    for k in ref_values:
        if k.startswith(("class_error", "cardinality_error")):
            for tag, v in (("F", vF), ("P", vP)):
                if abs(v[k] - ref_values[k]) > COUNT_RTOL * abs(ref_values[k]):
                    bad.append((k, tag, v[k], ref_values[k]))
    bounds = _bounds_c()
    for key, group in _GROUPS:
        names = [n for n in ref_grads if n.endswith(key)]
        if not names:
            continue
        e_f = max(CR.row_error(_rows(n, gF[n]), _rows(n, ref_grads[n])) for n in names)
        e_p = max(CR.row_error(_rows(n, gP[n]), _rows(n, ref_grads[n])) for n in names)
        _show("C", label, group, e_f, e_p, bounds[group])
        if max(e_f, e_p) > bounds[group]:
            bad.append((group, e_f, e_p))
    assert not bad, "(group, e_F, e_P, ...) beyond the bound: %s" % bad


# =================================================================================================== B: exact ties
# target (cx, cy, l, r, t, b) = (.5, .5, .125, .125, .125, .125) for every pair: corners (.375, .375, .625, .625).  All numbers are
# dyadic, so float32 holds them and their sums exactly.
_TIE_TARGET = (0.5, 0.5, 0.125, 0.125, 0.125, 0.125)
_TIE_PREDS = {
    "l1_tie": (0.5, 0.5625, 0.0625, 0.1875, 0.125, 0.15625),         # cx = cx*, t = t*; no corner coincides
    "other_heads_tie": (0.5625, 0.46875, 0.09375, 0.15625, 0.0625, 0.21875),   # partial overlap; depth, one size, residual equal
    "identical": _TIE_TARGET,
    "touching": (0.6875, 0.5625, 0.0625, 0.09375, 0.0625, 0.15625),  # x0 = x1* = .625: iw == 0, ih = .125; no component equal
}


def _tie_case():
    names = list(_TIE_PREDS)
    n = len(names)
    f = lambda rows: torch.tensor(rows, dtype=torch.float32)
    g = torch.Generator().manual_seed(2)
    layer = {"pred_logits": torch.randn(1, n, 3, generator=g), "pred_boxes": f([_TIE_PREDS[k] for k in names]).view(1, n, 6),
             "pred_3d_dim": f([[1.75, 1.5, 4.25]] * n).view(1, n, 3), "pred_depth": f([[20.5, 0.25]] * n).view(1, n, 2),
             "pred_angle": torch.randn(1, n, 24, generator=g)}
    tgt = {"labels": torch.tensor([0, 1, 2, 1]), "boxes_3d": f([_TIE_TARGET] * n),
           "boxes": f([[0.5, 0.5, 0.25, 0.25]] * n), "depth": f([[30.0]] * n), "size_3d": f([[1.5, 1.625, 4.0]] * n),
           "heading_bin": torch.tensor([[3], [0], [11], [7]]), "heading_res": f([[0.125]] * n)}
    o = names.index("other_heads_tie")
    layer["pred_depth"][0, o, 0] = 30.0                    # d = d*
    layer["pred_3d_dim"][0, o, 0] = 1.5                    # s_0 = s*_0
    layer["pred_angle"][0, o, 12 + 0] = 0.125              # residual of the target bin (0) = residual*
    layer["aux_outputs"] = []
    layer["pred_depth_map_logits"] = torch.randn(1, 81, 24, 80, generator=g)
    idx = torch.tensor([[[0] * n], [list(range(n))], [list(range(n))]])
    return names, layer, [tgt], idx


def test_exact_ties_follow_the_plain_formulation_or_a_stated_side():
    """At a tie float64 is no arbiter; the autograd conventions of the plain PyTorch formulation (criterion.py with
    FUSED_MATCHED = False) on the same float32 inputs are.  Equal components (torch: sign(0) = 0), equal depths, sizes and
    residuals, and identical boxes give the same losses and gradients in the kernel.

    Boxes that touch along an edge (iw == 0) do NOT: ``clamp(min=0)`` passes the gradient at exactly 0, so autograd sends the
    intersection's term (weighted with ih) to the touching edge, while the kernel's ``iw > 0`` takes the side of disjoint boxes,
    where only the enclosing box carries a gradient.  Either is a sub-gradient of the same function; a float32 box lands on
    iw == 0 with probability zero, so the kernel is left as it is and what it does is asserted here: the same loss values, every
    other gradient equal, and the box gradient of the touching pair equal to the limit from the disjoint side (the float64
    gradient at a prediction moved away by 2**-22) -- and different from the plain formulation's.
    For identical boxes ``torch.max`` / ``torch.min`` split each tied gradient in halves where the kernel picks one side; the
    halves cancel in GIoU's two terms (both formulations give exactly the L1-free gradient 0), so they agree."""
    from monosowa_amd.monodetr import criterion as C
    names, layer, targets, idx = _tie_case()
    crit = _criterion()
    crit.matcher = _GivenMatcher(idx)

    def run(fused):
        saved = C.FUSED_MATCHED
        C.FUSED_MATCHED = fused
        try:
            out, tg = CR.cast_case(layer, targets, "cuda", torch.float32)
            losses = crit(out, tg)
            total = C.weighted_total(losses, crit.weight_dict)
            nodes = _node_names([total])
            leaves = CR.leaves_of(out)
            grads = torch.autograd.grad(total, [leaves["l0." + k] for k in CR.PRED_KEYS])
            return {k: float(losses[k].detach()) for k in CR.LOSS6}, dict(zip(CR.PRED_KEYS, [g[0].cpu() for g in grads])), nodes
        finally:
            C.FUSED_MATCHED = saved

    vK, gK, nK = run(True)
    vT, gT, nT = run(False)
    assert "_MatchedLossesBackward" in nK and "_MatchedLossesBackward" not in nT
    for k in CR.LOSS6:
        assert np.isfinite(vK[k]) and _rel(vK[k], vT[k]) <= 1e-6, (k, vK[k], vT[k])
    touching = names.index("touching")
    for key in CR.PRED_KEYS:
        assert torch.isfinite(gK[key]).all(), key
        for i, name in enumerate(names):
            if key == "pred_boxes" and i == touching:
                continue
            scale = float(gT[key].abs().max())
            assert float((gK[key][i] - gT[key][i]).abs().max()) <= 2e-6 * scale, (key, name, gK[key][i], gT[key][i])
    # the ties really are ties, and give the zeros of torch's sign(0)
    t = names.index("l1_tie")
    assert layer["pred_boxes"][0, t, 0] == 0.5 and layer["pred_boxes"][0, t, 4] == 0.125
    o = names.index("other_heads_tie")
    assert gK["pred_depth"][o, 0] == 0 and gK["pred_3d_dim"][o, 0] == 0 and gK["pred_angle"][o, 12] == 0
    assert float(gK["pred_boxes"][names.index("identical")].abs().max()) <= 2e-6 * float(gT["pred_boxes"].abs().max())
    # touching boxes: the kernel's box gradient is the disjoint side's
    moved = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in layer.items()}
    out64, tg64 = CR.cast_case(moved, targets, "cuda", torch.float64)
    with torch.no_grad():
        out64["pred_boxes"][0, touching, 0] += 2.0 ** -22
    num_boxes = float(len(names) * crit.group_num)
    want = CR.criterion_losses(out64, tg64, idx.cuda(), num_boxes, crit.focal_alpha)
    total = sum(want[k] * float(crit.weight_dict[k]) for k in CR.LOSS6)
    (g64,) = torch.autograd.grad(total, [out64["pred_boxes"]])
    side = g64[0, touching].cpu()
    assert float((gK["pred_boxes"][touching].double() - side).abs().max()) <= 1e-5 * float(side.abs().max()), (gK["pred_boxes"][touching], side)
    assert float((gK["pred_boxes"][touching] - gT["pred_boxes"][touching]).abs().max()) > 1e-2 * float(side.abs().max())


# =================================================================================================== C: KITTI-like layouts
# name -> (targets per image, queries, train mode, seed): the same cases as tests/test_criterion_reference.py
_LAYOUTS = {
    "mixed_b8": ([0, 50, 1, 0, 23, 50, 7, 3], 550, True, 100),
    "empty_batch": ([0, 0, 0], 550, True, 101),
    "eval_q50": ([5, 0, 50], 50, False, 102),
    "full_b16": ([50] * 16, 550, True, 103),
    "one_target": ([1], 550, True, 104),
}


def _depth_map_targets(crit, targets, dtype):
    """the painted bin map and the foreground mask of the depth-map loss, evaluated in ``dtype`` (criterion.py forward_fast +
    losses.py forward_padded)"""
    from monosowa_amd.monodetr import box_ops
    from monosowa_amd.monodetr.losses import lid_bin_indices, rasterize_boxes
    w, h = crit.depth_map_size
    sizes = [len(t["labels"]) for t in targets]
    maxn = max(max(sizes), 1)
    boxes = torch.zeros(len(sizes), maxn, 4, dtype=dtype)
    depth = torch.zeros(len(sizes), maxn, dtype=dtype)
    valid = torch.zeros(len(sizes), maxn, dtype=torch.bool)
    scale = torch.tensor([w, h, w, h], dtype=dtype)
    for b, t in enumerate(targets):
        n = sizes[b]
        boxes[b, :n] = box_ops.box_cxcywh_to_xyxy(t["boxes"].to(dtype) * scale)
        depth[b, :n] = t["depth"].to(dtype).squeeze(1)
        valid[b, :n] = True
    boxes[..., :2], boxes[..., 2:] = torch.floor(boxes[..., :2]), torch.ceil(boxes[..., 2:])
    painted, fg = rasterize_boxes(boxes.long(), depth, valid, h, w)
    return lid_bin_indices(painted, target=True), fg


def _layout_runs(crit, outputs, targets):
    F = _evaluate(crit, outputs, targets, True, torch.float32)
    assert crit.matcher.idx is not None
    P = _evaluate(crit, outputs, targets, False, torch.float32)
    R = _evaluate(crit, outputs, targets, False, torch.float64)
    return F, P, R


def _census_of(outputs, targets, idx):
    st, ft = CR.stack_layers(outputs), CR.flat_targets(targets)
    return CR.census(st["pred_boxes"], st["pred_depth"], st["pred_3d_dim"], st["pred_angle"], idx, ft["boxes_3d"], ft["depth"],
                     ft["size_3d"], ft["heading_bin"], ft["heading_res"])


@pytest.mark.parametrize("name", list(_LAYOUTS))
def test_criterion_at_kitti_like_layouts_equals_float64(name):
    sizes, Q, train, seed = _LAYOUTS[name]
    outputs, targets = CR.make_layout_case(seed, sizes, Q)
    crit = _criterion(train)
    groups = crit.group_num if train else 1
    # conditions on the inputs that do not need the matching
    bins32, fg32 = _depth_map_targets(crit, targets, torch.float32)
    bins64, fg64 = _depth_map_targets(crit, targets, torch.float64)
    assert torch.equal(bins32, bins64) and torch.equal(fg32, fg64)
    assert set(torch.cat([t["labels"] for t in targets]).tolist()) == {0, 1, 2} or sum(sizes) < 3

    (vF, tF, gF, nF), (vP, tP, gP, nP), (vR, tR, gR, nR) = _layout_runs(crit, outputs, targets)
    idx = torch.from_numpy(crit.matcher.idx)
    K = groups * sum(min(n, Q // groups) for n in sizes)
    assert idx.shape == (3, 3, K)
    cls, margins = _census_of(outputs, targets, idx)
    shares = CR.class_shares(cls)
    print("\n%s: K %d, shares %s\nmargins %s\ntotal F %.9g P %.9g R %.12g" % (name, K, {k: round(v, 3) for k, v in shares.items()},
                                                                             margins, tF, tP, tR))
    assert min(margins.values()) >= CR.MARGIN, margins
    if name in ("mixed_b8", "full_b16"):
        assert shares["disjoint"] >= 0.25, shares
    # which code ran
    assert not _KERNEL_NODES & nP and not _KERNEL_NODES & nR, sorted(_KERNEL_NODES & (nP | nR))
    if K:
        assert _KERNEL_NODES <= nF, sorted(_KERNEL_NODES - nF)
    else:                                                    # nothing to match: the PyTorch formulation over empty index tensors
        assert _KERNEL_NODES & nF == {"_DDNLossBackward"}, sorted(nF)
    assert all(np.isfinite(v) for v in vF.values()) and np.isfinite(tF) and all(torch.isfinite(g).all() for g in gF.values())
    # R is the float64 evaluation of the plain formulation; the independent helper agrees with it on what it covers
    out64, tg64 = CR.cast_case(outputs, targets, "cuda", torch.float64, requires_grad=False)
    num_boxes = max(float(sum(sizes) * groups), 1.0)
    helper = CR.criterion_losses(out64, tg64, idx.cuda(), num_boxes, crit.focal_alpha)
    ref = dict(vR)
    for k, v in helper.items():
        if k.startswith(("class_error", "cardinality_error")):
            ref[k] = float(v)             # the plain formulation forms the two counts in float32 whatever the inputs' type
            assert abs(float(v) - vR[k]) <= 2.0 ** -22 * 100.0, (k, float(v), vR[k])
        else:
            assert abs(float(v) - vR[k]) <= 1e-11 * max(abs(vR[k]), TINY), (k, float(v), vR[k])
    _compare(name, {"F": (vF, tF, gF), "P": (vP, tP, gP)}, ref, tR, gR)


def test_device_matcher_equals_host_solver_and_scipy_on_real_cost_blocks():
    """layout mixed_b8 (images without targets, with one, with 50): the assignments of the device solver, of the host solver and of
    scipy.optimize.linear_sum_assignment on the float32 cost blocks the cost kernel wrote, per (layer, image, group)"""
    from scipy.optimize import linear_sum_assignment
    from monosowa_amd.monodetr import matcher as M
    from monosowa_amd.pointwise import match_cost_blocks
    sizes, Q, _, seed = _LAYOUTS["mixed_b8"]
    outputs, targets = CR.make_layout_case(seed, sizes, Q)
    out, tg = CR.cast_case(outputs, targets, "cuda", torch.float32, requires_grad=False)
    st, ft = CR.stack_layers(out), CR.flat_targets(tg)
    m = _criterion().matcher.inner
    G, NL, B, T = 11, 3, len(sizes), sum(sizes)
    found = {}
    for device in (True, False):
        saved = M.DEVICE_LSAP
        M.DEVICE_LSAP = device
        try:
            got = m.match_layers_end_flat(m.match_layers_begin(st["pred_logits"], st["pred_boxes"], ft, sizes, G))
        finally:
            M.DEVICE_LSAP = saved
        assert torch.is_tensor(got) and got.is_cuda if device else True
        found[device] = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    m.check_device_status(block=True)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    cols = np.minimum(offs[:, None] + np.arange(max(sizes))[None, :], T - 1)
    blocks = match_cost_blocks(st["pred_logits"], st["pred_boxes"], ft["labels"], ft["boxes_3d"], torch.from_numpy(cols).cuda(),
                               m.cost_class, m.cost_3dcenter, m.cost_bbox, m.cost_giou).cpu().numpy()
    gq = Q // G
    want = []
    for l in range(NL):
        tri = []
        for b, n in enumerate(sizes):
            for g in range(G):
                r, c = linear_sum_assignment(blocks[l, b, g * gq:(g + 1) * gq, :n])
                tri += [(b, int(q) + g * gq, int(t) + int(offs[b])) for q, t in zip(r, c)]
        want.append(sorted(tri))
    for device, got in found.items():
        assert got.shape == (3, NL, G * sum(sizes)), got.shape
        for l in range(NL):
            assert sorted(map(tuple, got[:, l].T.tolist())) == want[l], (device, l)


# name -> (B, Q, train mode, sizes): one step beyond each limit of the focal kernel (focal_classification_supported)
_BEYOND = {
    "cells_32768_plus_Q": (65, 512, False, [(5 * i) % 9 if i % 3 else 0 for i in range(64)] + [50]),
    "images_257": (257, 110, True, [i % 4 if i % 5 else 0 for i in range(256)] + [10]),
}


@pytest.mark.parametrize("name", list(_BEYOND))
def test_beyond_the_focal_kernel_limits_the_pytorch_formulation_takes_over(name):
    """B * Q == 32768 + Q and B == 257: ``focal_classification_supported`` is false, and ``forward_fast`` returns the same losses
    and gradients through the PyTorch formulation of the classification side (the matched-pair kernels still run)"""
    from monosowa_amd.pointwise import focal_classification_supported
    B, Q, train, sizes = _BEYOND[name]
    outputs, targets = CR.make_layout_case(200 + list(_BEYOND).index(name), sizes, Q)
    crit = _criterion(train)
    groups = crit.group_num if train else 1
    assert B * Q == 32768 + Q or B == 257
    (vF, tF, gF, nF), (vP, tP, gP, nP), (vR, tR, gR, nR) = _layout_runs(crit, outputs, targets)
    idx = torch.from_numpy(crit.matcher.idx)
    assert not focal_classification_supported(outputs["pred_logits"].new_zeros(3, B, Q, 3).cuda(), idx.cuda())
    assert "_FocalClassificationBackward" not in nF and {"_MatchedLossesBackward", "_DDNLossBackward"} <= nF, sorted(nF)
    assert not _KERNEL_NODES & nP
    _, margins = _census_of(outputs, targets, idx)
    assert min(margins.values()) >= CR.MARGIN, margins
    # against the independent helper in float64 (it has no depth-map loss: that one against R)
    out64, tg64 = CR.cast_case(outputs, targets, "cuda", torch.float64)
    num_boxes = max(float(sum(sizes) * groups), 1.0)
    helper = CR.criterion_losses(out64, tg64, idx.cuda(), num_boxes, crit.focal_alpha)
    weights = {k: float(crit.weight_dict[k]) for k in helper if k in crit.weight_dict}
    leaves = CR.leaves_of(out64)
    named = [n for n in leaves if n != "depth_map_logits"]
    total = sum(helper[k] * w for k, w in weights.items())
    grads = dict(zip(named, torch.autograd.grad(total, [leaves[n] for n in named], allow_unused=True)))
    grads = {n: (torch.zeros_like(leaves[n]) if g is None else g) for n, g in grads.items()}
    values = {k: float(v.detach()) for k, v in helper.items()}
    values["loss_depth_map"] = vR["loss_depth_map"]
    total = float(total.detach()) + vR["loss_depth_map"] * float(crit.weight_dict["loss_depth_map"])
    grads["depth_map_logits"] = gR["depth_map_logits"]
    _compare(name, {"F": (vF, tF, gF), "P": (vP, tP, gP)}, values, total, grads)


# Measured on the MI355X, every case: group e_F/e_P (F the product, P plain float32, both against float64)
#   A K1_NL1_B3_Q50            value 2.8e-08/2.8e-08 | boxes 5.2e-08/4.7e-08 | depth 2.7e-08/2.7e-08 | dims 5.4e-08/5.4e-08 | angle 1.4e-08/1.4e-08
#   A K1_NL3_B16_Q550          value 7.5e-08/7.5e-08 | boxes 6.4e-08/7.5e-08 | depth 7.3e-08/7.3e-08 | dims 1.0e-07/1.0e-07 | angle 6.6e-08/6.6e-08
#   A K55_NL3_B3_Q50           value 1.3e-07/1.6e-07 | boxes 1.4e-07/1.8e-07 | depth 1.2e-07/1.4e-07 | dims 1.5e-07/1.5e-07 | angle 9.3e-08/1.1e-07
#   A K255_NL1_B16_Q550        value 6.7e-08/1.1e-07 | boxes 1.4e-07/3.1e-07 | depth 0.0e+00/0.0e+00 | dims 9.8e-08/9.7e-08 | angle 1.2e-07/1.2e-07
#   A K255_NL3_B16_Q550        value 6.5e-08/9.9e-08 | boxes 1.9e-07/2.5e-07 | depth 1.4e-07/1.5e-07 | dims 1.5e-07/1.5e-07 | angle 1.3e-07/1.0e-07
#   A K256_NL1_B16_Q550        value 9.4e-08/9.4e-08 | boxes 2.6e-07/2.8e-07 | depth 1.4e-07/1.7e-07 | dims 4.9e-08/4.9e-08 | angle 0.0e+00/0.0e+00
#   A K256_NL3_B16_Q550        value 9.9e-08/9.9e-08 | boxes 1.7e-07/2.9e-07 | depth 1.6e-07/1.5e-07 | dims 1.2e-07/2.2e-07 | angle 1.2e-07/1.7e-07
#   A K257_NL1_B16_Q550        value 5.2e-08/1.6e-07 | boxes 2.4e-07/2.9e-07 | depth 1.4e-07/1.2e-07 | dims 1.5e-07/1.5e-07 | angle 8.5e-08/1.3e-07
#   A K257_NL3_B16_Q550        value 8.2e-08/1.7e-07 | boxes 1.8e-07/2.3e-07 | depth 1.7e-07/1.5e-07 | dims 1.3e-07/2.0e-07 | angle 1.2e-07/1.3e-07
#   A K1474_NL1_B16_Q550       value 9.3e-08/2.4e-07 | boxes 1.8e-07/2.8e-07 | depth 0.0e+00/0.0e+00 | dims 1.3e-07/2.4e-07 | angle 1.4e-07/1.2e-07
#   A K1474_NL3_B16_Q550       value 6.6e-08/7.6e-08 | boxes 2.1e-07/3.3e-07 | depth 1.6e-07/1.6e-07 | dims 1.6e-07/8.6e-08 | angle 1.9e-07/1.4e-07
#   A K8800_NL1_B16_Q550       value 2.9e-08/2.9e-08 | boxes 2.9e-07/5.2e-07 | depth 1.8e-07/1.7e-07 | dims 1.2e-07/8.2e-08 | angle 0.0e+00/0.0e+00
#   A K8800_NL3_B16_Q550       value 1.1e-07/1.1e-07 | boxes 3.0e-07/4.0e-07 | depth 2.0e-07/2.0e-07 | dims 1.4e-07/1.2e-07 | angle 2.0e-07/1.7e-07
#   A train_alpha.25_gamma2    value 4.5e-08/4.5e-08 | logits 1.8e-06/1.6e-06
#   A train_no_alpha           value 1.4e-08/1.4e-08 | logits 2.1e-06/1.8e-06
#   A train_gamma1.5_powf      value 1.4e-08/1.4e-08 | logits 1.7e-06/1.3e-06
#   A train_mostly_right       value 5.4e-08/6.4e-08 | logits 1.1e-06/1.1e-06
#   A eval_q50                 value 1.1e-08/1.1e-08 | logits 6.8e-07/6.0e-07
#   A one_layer_one_target     value 3.4e-08/5.2e-08 | logits 7.5e-07/8.3e-07
#   A limit_cells_32768        value 1.2e-07/6.8e-08 | logits 2.3e-06/1.9e-06
#   A limit_images_256         value 2.0e-08/2.0e-08 | logits 1.3e-06/1.4e-06
#   C mixed_b8                 loss 1.0e-07/1.4e-07 | logits 1.7e-06/2.1e-06 | boxes 1.7e-07/1.6e-07 | depth 5.4e-07/4.6e-07 | dims 1.1e-07/1.1e-07 | angle 1.9e-07/1.4e-07 | map 2.8e-07/2.7e-07
#   C empty_batch              loss 1.4e-07/1.4e-07 | logits 9.3e-07/9.3e-07 | boxes 0.0e+00/0.0e+00 | depth 0.0e+00/0.0e+00 | dims 0.0e+00/0.0e+00 | angle 0.0e+00/0.0e+00 | map 4.0e-07/2.4e-07
#   C eval_q50                 loss 1.5e-07/1.5e-07 | logits 7.3e-07/7.9e-07 | boxes 1.2e-07/1.3e-07 | depth 4.5e-07/3.8e-07 | dims 1.6e-07/1.6e-07 | angle 1.2e-07/1.1e-07 | map 2.6e-07/4.0e-07
#   C full_b16                 loss 1.0e-07/1.0e-07 | logits 3.2e-06/3.3e-06 | boxes 1.5e-07/2.0e-07 | depth 5.4e-07/6.9e-07 | dims 1.3e-07/1.3e-07 | angle 2.3e-07/1.5e-07 | map 2.8e-07/4.4e-07
#   C one_target               loss 1.1e-07/1.3e-07 | logits 5.4e-07/1.3e-06 | boxes 1.3e-07/1.0e-07 | depth 1.3e-07/1.3e-07 | dims 5.0e-08/7.3e-08 | angle 9.7e-08/9.3e-08 | map 2.4e-07/2.5e-07
#   C cells_32768_plus_Q       loss 1.5e-07/1.5e-07 | logits 1.7e-06/1.7e-06 | boxes 1.2e-07/1.4e-07 | depth 4.5e-07/3.8e-07 | dims 1.5e-07/1.2e-07 | angle 1.4e-07/1.3e-07 | map 4.3e-07/3.6e-07
#   C images_257               loss 9.8e-08/9.8e-08 | logits 2.3e-06/2.3e-06 | boxes 1.5e-07/1.9e-07 | depth 6.8e-07/8.1e-07 | dims 1.1e-07/1.1e-07 | angle 1.8e-07/1.7e-07 | map 5.5e-07/4.3e-07
