"""Per-label loss weights on the GPU: the six weighted entry points of csrc/matched_losses.hip and csrc/ddn_loss.hip, the criterion's
routes that run them, and train steps of the shipped architecture with a ``label_weight`` in the batch.

F is the weighted kernel (``pointwise.matched_losses`` / ``focal_classification`` / ``ddn_loss`` with ``weight=``, or the whole
``SetCriterion`` with every switch of tests/fused_switches.py shipped), P the plain weighted formulation in float32 on the GPU
(tests/label_weights_reference.py in float32; for the whole criterion: every switch plain), R tests/label_weights_reference.py in float64.

Metrics: those of tests/test_criterion_kernels_gpu.py -- |x - x_R| / max(|x_R|, tiny) per loss value, ``criterion_reference.row_error``
per gradient tensor (a row: one (layer, image, query) slice, or one pixel's 81 bins); rows no pair names: exactly 0.

Bounds: one per tensor group, 4 x the worst e_P of the group over every case of its section on the MI355X, rounded up to one significant
digit; F and P must both meet it (the factor 4: another summation order, other exp / log roundings).  The measured worst e_F / e_P stand
beside each constant.

Exact properties (no tolerance): weights of 1 give the unweighted siblings' bytes, weights of 0.5 exactly half of the matched sums and
gradients, a weight of 0 exactly-zero gradient rows, and the bytes do not depend on where the outputs lie."""
import warnings

import numpy as np
import pytest
import torch

import criterion_reference as CR
import label_weights_reference as LW
from fused_switches import fused_switches
from test_accumulation_gpu import RES, _Rig, dev, shared      # noqa: F401  (fixtures)
from test_criterion_kernels_gpu import _MIXED_SIZES, _criterion, _node_names, _rel, _show, _upstream

pytestmark = pytest.mark.gpu
TINY = 1e-30
COUNT_RTOL = 2.0 ** -22
SENTINEL = 777.0

# Section A (the kernels alone): worst e_F / worst e_P over the cases (in brackets the case of the worst e_P), and 4 x e_P before rounding
A_VALUE = 8e-7         # 1.8e-7 / 1.9e-7 (K 256), 7.6e-7: per-layer sums of the six weighted matched losses
A_BOXES = 2e-6         # 2.4e-7 / 3.0e-7 (K 255), 1.2e-6
A_DEPTH = 9e-7         # 1.8e-7 / 2.1e-7 (K 256), 8.2e-7
A_DIMS = 9e-7          # 1.9e-7 / 2.1e-7 (K 256), 8.4e-7
A_ANGLE = 8e-6         # 1.8e-7 / 1.9e-6 (K 1474), 7.6e-6: P takes the heading's cross entropy as logsumexp - logit
A_FOCAL_VALUE = 5e-7   # 1.4e-7 / 1.0e-7 (exactly FOCAL_WEIGHTED_MAX_CELLS cells), 4.0e-7: per-layer weighted focal sum
A_FOCAL_LOGITS = 8e-6  # 2.2e-6 / 1.8e-6 (training shape), 7.1e-6
A_MAP_VALUE = 4e-7     # 9.5e-9 / 8.1e-8 (both layouts), 3.2e-7: the weighted depth-map loss
A_MAP_LOGITS = 5e-6    # 1.2e-6 / 1.0e-6 (both layouts), 4.2e-6
# Section C (the whole criterion: the fused tail, the matched kernels alone, and one image beyond the weighted focal kernel's reach)
C_LOSS = 6e-7          # 1.2e-7 / 1.3e-7 (mixed_b8), 5.2e-7: every loss key and the weighted total
C_LOGITS = 8e-6        # 2.0e-6 / 2.0e-6 (beyond_focal_reach), 7.8e-6
C_BOXES = 7e-7         # 1.5e-7 / 1.7e-7 (beyond_focal_reach), 6.7e-7
C_DEPTH = 3e-6         # 5.2e-7 / 7.4e-7 (mixed_b8), 2.9e-6
C_DIMS = 1e-6          # 1.5e-7 / 2.4e-7 (beyond_focal_reach), 9.6e-7
C_ANGLE = 6e-7         # 2.7e-7 / 1.3e-7 (beyond_focal_reach), 5.3e-7
C_DEPTH_MAP = 2e-6     # 4.7e-7 / 3.4e-7 (mixed_b8), 1.4e-6


def _check(bad, group, e_f, e_p, bound):
    if max(e_f, e_p) > bound:
        bad.append((group, e_f, e_p))


# =================================================================================================== A: matched-pair kernels
# (K, NL, B, Q): one pass of the kernels' 256-thread loop and its neighbours, and the training shape's usual K
_MATCHED_CASES = [(1, 1, 3, 50), (255, 3, 3, 550), (256, 3, 3, 550), (257, 1, 3, 550), (1474, 3, 16, 550)]
_NAMES = ("boxes", "depth", "dims", "angle")


def _matched_case(case_no):
    K, NL, B, Q = _MATCHED_CASES[case_no]
    case = CR.make_matched_case(511 + case_no, NL, B, Q, K)
    case["weight"] = LW.draw_weights(611 + case_no, K)
    return case


def _run_matched(fn, case, dtype, go, weight=None):
    args = [case[k].cuda() for k in CR.MATCHED_ARGS]
    args = [a.to(dtype) if a.is_floating_point() else a for a in args]
    leaves = [a.requires_grad_(True) for a in args[:4]]
    out = fn(*args) if weight is None else fn(*args, weight.cuda().to(dtype))
    grads = torch.autograd.grad((out * go.to(device="cuda", dtype=out.dtype)).sum(), leaves)
    return out.detach(), dict(zip(_NAMES, grads))


@pytest.mark.parametrize("case_no", range(len(_MATCHED_CASES)), ids=["K%d_NL%d_B%d_Q%d" % c for c in _MATCHED_CASES])
def test_weighted_matched_pair_kernels_equal_float64(case_no):
    from monosowa_amd.pointwise import matched_losses
    K, NL, B, Q = _MATCHED_CASES[case_no]
    case = _matched_case(case_no)
    w = case["weight"]
    assert (w > 1).any() and (K < 2 or (w == 0).any())            # (the single pair of K = 1 carries the weight 2)
    _, margins = CR.census(*[case[k] for k in CR.MATCHED_ARGS])
    assert min(margins.values()) >= CR.MARGIN, margins
    rows = (torch.arange(NL).view(NL, 1) * B + case["idx"][0]) * Q + case["idx"][1]
    assert rows.unique().numel() == NL * K
    go = _upstream(NL, case_no)
    vF, gF = _run_matched(lambda *a: matched_losses(*a[:-1], weight=a[-1]), case, torch.float32, go, w)
    vP, gP = _run_matched(LW.matched_sums, case, torch.float32, go, w)
    vR, gR = _run_matched(LW.matched_sums, case, torch.float64, go, w)
    assert vF.shape == (NL, 6) and vF.dtype == torch.float32
    assert torch.isfinite(vF).all() and all(torch.isfinite(g).all() for g in gF.values())
    label = "K%d_NL%d_B%d_Q%d" % (K, NL, B, Q)
    bad = []
    e_f = max(_rel(vF[l, j], vR[l, j]) for l in range(NL) for j in range(6))
    e_p = max(_rel(vP[l, j], vR[l, j]) for l in range(NL) for j in range(6))
    _show("A", label, "value", e_f, e_p, A_VALUE)
    _check(bad, "value", e_f, e_p, A_VALUE)
    for n, bound in zip(_NAMES, (A_BOXES, A_DEPTH, A_DIMS, A_ANGLE)):
        e_f, e_p = CR.row_error(gF[n], gR[n]), CR.row_error(gP[n], gR[n])
        _show("A", label, n, e_f, e_p, bound)
        _check(bad, n, e_f, e_p, bound)
    free = torch.ones(NL * B * Q, dtype=torch.bool)
    free[rows.reshape(-1)] = False
    zero = (w[case["idx"][2]] == 0)                               # [NL, K]: pairs of a label of weight 0
    for n in _NAMES:
        g = gF[n].reshape(NL * B * Q, -1).cpu()
        assert (g[free] == 0).all(), n
        assert (g[rows[zero]] == 0).all(), n
        if n in ("boxes", "angle"):                             # (a zero upstream factor may silence a whole depth or size head)
            assert (g[rows[~zero]].abs().sum(1) > 0).all(), n
    assert not bad, "(group, e_F, e_P) beyond the bound: %s" % bad


# =================================================================================================== A: focal kernels
def _max_cells():
    from monosowa_amd import pointwise
    assert pointwise.FOCAL_WEIGHTED_MAX_CELLS == pointwise.load().mono_focal_weighted_max_cells() >= 16384
    return pointwise.FOCAL_WEIGHTED_MAX_CELLS


# name -> (NL, B, Q, sizes, groups)
_FOCAL_CASES = {
    "train": (3, 16, 550, _MIXED_SIZES, 11),
    "eval_q50": (3, 3, 50, [5, 0, 50], 1),
    "limit_cells": (3, 32, 512, [(7 * i) % 11 if i % 4 else 0 for i in range(31)] + [50], 10),
}


def _focal_case(name):
    NL, B, Q, sizes, groups = _FOCAL_CASES[name]
    case = CR.make_focal_case(531 + list(_FOCAL_CASES).index(name), NL, B, Q, sizes, groups)
    case["weight"] = LW.draw_weights(631 + list(_FOCAL_CASES).index(name), sum(sizes))
    return case


def _run_focal(fn, case, dtype, go, weight):
    logits = case["logits"].cuda().to(dtype).requires_grad_(True)
    out = fn(logits, case["idx"].cuda(), case["labels"].cuda(), case["sizes"].cuda().to(dtype), weight, 0.25, 2.0)
    (grad,) = torch.autograd.grad((out * go.to(device="cuda", dtype=out.dtype))[:, 0].sum(), [logits])
    return out.detach(), grad


_FOCAL_GO = torch.tensor([[0.5, 3.0, 7.0], [-1.25, 5.0, 11.0], [2.0, 13.0, 17.0]], dtype=torch.float64)


@pytest.mark.parametrize("name", list(_FOCAL_CASES))
def test_weighted_focal_kernels_equal_float64(name):
    from monosowa_amd.pointwise import focal_classification, focal_classification_weighted_supported
    NL, B, Q, sizes, groups = _FOCAL_CASES[name]
    if name == "limit_cells":
        assert B * Q == _max_cells()
    case = _focal_case(name)
    w = case["weight"]
    assert (w == 0).any() and (w > 1).any() and 0 in sizes
    assert focal_classification_weighted_supported(case["logits"].cuda(), case["idx"].cuda())
    F = lambda lg, idx, lab, sz, wt, a, g: focal_classification(lg, idx, lab, sz, a, g, weight=wt)
    P = lambda lg, idx, lab, sz, wt, a, g: LW.focal_sums(lg, idx, lab, sz, wt, a, g)
    go = _FOCAL_GO[:NL]
    vF, gF = _run_focal(F, case, torch.float32, go, w.cuda())
    vP, gP = _run_focal(P, case, torch.float32, go, w.cuda())
    vR, gR = _run_focal(P, case, torch.float64, go, w.cuda().double())
    assert vF.shape == (NL, 3) and torch.isfinite(vF).all() and torch.isfinite(gF).all()
    bad = []
    e_f = max(_rel(vF[l, 0], vR[l, 0]) for l in range(NL))
    e_p = max(_rel(vP[l, 0], vR[l, 0]) for l in range(NL))
    _show("A", name, "focal value", e_f, e_p, A_FOCAL_VALUE)
    _check(bad, "focal value", e_f, e_p, A_FOCAL_VALUE)
    g_f, g_p = CR.row_error(gF, gR), CR.row_error(gP, gR)
    _show("A", name, "focal logits", g_f, g_p, A_FOCAL_LOGITS)
    _check(bad, "focal logits", g_f, g_p, A_FOCAL_LOGITS)
    for l in range(NL):                                      # the two counts are unweighted
        for j in (1, 2):
            assert abs(float(vF[l, j]) - float(vR[l, j])) <= COUNT_RTOL * abs(float(vR[l, j])), (l, j, float(vF[l, j]), float(vR[l, j]))
    # the queries of a label of weight 0: all C gradients exactly 0 (don't care); the others, matched or not, non-zero
    idx = case["idx"]
    zero = (w[idx[2]] == 0)
    g = gF.cpu()
    for l in range(NL):
        rows, ref = g[l, idx[0, l], idx[1, l]], gR[l].cpu()[idx[0, l], idx[1, l]].abs().sum(1)
        assert zero[l].any() and (rows[zero[l]] == 0).all()
        live = ~zero[l] & (ref > 1e-12)                       # (a saturated row's float64 gradient can lie below float32's range)
        assert live.sum() > 0.5 * (~zero[l]).sum() and (rows[live].abs().sum(1) > 0).all()
    assert not bad, "(group, e_F, e_P) beyond the bound: %s" % bad


# =================================================================================================== A: depth map
def _depth_map_case():
    """B = 3, a 24 x 80 map, up to 8 boxes per image (xyxy in map pixels): image 0 holds overlapping boxes, a box of weight 0 nearest
    over part of a trusted one and alone elsewhere, two covering boxes of equal depth and different weights (the lower slot decides), a
    box whose negative start wraps like a Python slice; image 1 no box; image 2 three boxes at fractional corners."""
    boxes = torch.zeros(3, 8, 4)
    depth, weight = torch.zeros(3, 8), torch.ones(3, 8)
    valid = torch.zeros(3, 8, dtype=torch.bool)
    img0 = [((10.25, 4.5, 40.0, 20.0), 30.0, 1.0),           # trusted
            ((25.0, 8.0, 50.5, 16.0), 12.0, 0.0),            # weight 0, nearer: over part of the trusted box and beyond it
            ((30.0, 2.0, 60.0, 10.0), 20.5, 2.0),            # overlaps both
            ((60.0, 10.0, 75.0, 22.0), 41.0, 0.5),           # equal depths, different weights: slot 3 decides where both cover
            ((65.0, 12.0, 79.5, 24.0), 41.0, 1.25),
            ((-3.5, 0.0, 10.0, 3.0), 17.0, 1.5),             # start -4 counts from the end: an empty slice
            ((0.0, 21.0, 8.0, 24.0), 55.0, 0.25),
            ((44.0, 18.0, 58.0, 23.5), 9.0, 0.0)]            # weight 0 alone
    for i, (b, d, w) in enumerate(img0):
        boxes[0, i], depth[0, i], weight[0, i], valid[0, i] = torch.tensor(b), d, w, True
    img2 = [((5.3, 3.7, 33.2, 15.1), 47.25, 0.75), ((20.6, 9.9, 70.4, 19.8), 8.5, 1.0), ((50.1, 0.2, 79.9, 23.9), 26.0, 0.0)]
    for i, (b, d, w) in enumerate(img2):
        boxes[2, i], depth[2, i], weight[2, i], valid[2, i] = torch.tensor(b), d, w, True
    depth = torch.from_numpy(CR._off_bin_edges(depth.double().numpy()).astype(np.float32))
    assert depth[0, 3] == depth[0, 4]
    logits = torch.randn(3, 81, 24, 80, generator=torch.Generator().manual_seed(77)) * 2
    return logits, boxes, depth, valid, weight


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_weighted_depth_map_kernels_equal_float64(layout):
    from monosowa_amd.pointwise import ddn_loss, ddn_loss_supported
    logits, boxes, depth, valid, weight = _depth_map_case()
    go = 1.75

    def run(fn, dtype):
        lg = logits.cuda().to(dtype)
        if layout == "channels_last":
            lg = lg.contiguous(memory_format=torch.channels_last)
        lg.requires_grad_(True)
        out, maps = fn(lg, boxes.cuda().to(dtype), depth.cuda().to(dtype), valid.cuda(), weight.cuda().to(dtype))
        (grad,) = torch.autograd.grad(out * go, [lg])
        return out.detach(), grad, maps

    def F(lg, bx, dp, vl, wt):
        assert ddn_loss_supported(lg, bx, dp, vl)
        return ddn_loss(lg, bx, dp, vl, 0.25, 2.0, 13, 1, weight=wt), None
    vF, gF, _ = run(F, torch.float32)
    vP, gP, (bins32, fg32, w32) = run(LW.depth_map_loss, torch.float32)
    vR, gR, (bins, fg, wmap) = run(LW.depth_map_loss, torch.float64)
    assert torch.equal(bins32, bins) and torch.equal(fg32, fg) and torch.equal(w32.double(), wmap)          # both precisions paint alike
    assert gF.stride() == ((155520, 1, 6480, 81) if layout == "channels_last" else (155520, 1920, 80, 1)) and torch.isfinite(gF).all()
    fg, wmap = fg.cpu(), wmap.cpu()
    # the cases are there: a pixel decided by the weight-0 box inside the trusted box, one decided by slot 3 of the equal pair, ...
    assert fg[0, 10, 30] and wmap[0, 10, 30] == 0.0 and fg[0, 6, 12] and wmap[0, 6, 12] == 1.0 and wmap[0, 5, 35] == 2.0
    assert wmap[0, 15, 70] == 0.5 and wmap[0, 23, 70] == 1.25 and wmap[0, 11, 62] == 0.5
    assert not fg[0, 1, 78] and not fg[0, 1, 5] and not fg[1].any() and wmap[0, 20, 50] == 0.0 and wmap[0, 22, 3] == 0.25
    assert sorted(wmap[2][fg[2]].unique().tolist()) == [0.0, 0.75, 1.0]
    bad = []
    e_f, e_p = _rel(vF, vR), _rel(vP, vR)
    _show("A", layout, "map value", e_f, e_p, A_MAP_VALUE)
    _check(bad, "map value", e_f, e_p, A_MAP_VALUE)
    rows = lambda x: x.permute(0, 2, 3, 1)
    g_f, g_p = CR.row_error(rows(gF), rows(gR)), CR.row_error(rows(gP), rows(gR))
    _show("A", layout, "map logits", g_f, g_p, A_MAP_LOGITS)
    _check(bad, "map logits", g_f, g_p, A_MAP_LOGITS)
    # every pixel whose deciding box has weight 0: 81 exactly-zero bins; every other pixel: a gradient
    dont_care = fg & (wmap == 0)
    g = rows(gF).cpu()
    assert dont_care.sum() > 100 and (g[dont_care] == 0).all() and (g[~dont_care].abs().sum(-1) > 0).all()
    assert not bad, "(group, e_F, e_P) beyond the bound: %s" % bad


# =================================================================================================== exact properties
def test_weights_of_one_give_the_unweighted_kernels_bytes():
    from monosowa_amd.pointwise import ddn_loss, focal_classification, matched_losses
    for case_no in (3, 4):
        case = _matched_case(case_no)
        NL = _MATCHED_CASES[case_no][1]
        go = _upstream(NL, case_no)
        v0, g0 = _run_matched(matched_losses, case, torch.float32, go)
        v1, g1 = _run_matched(lambda *a: matched_losses(*a[:-1], weight=a[-1]), case, torch.float32, go, torch.ones_like(case["weight"]))
        assert torch.equal(v0, v1) and all(torch.equal(g0[n], g1[n]) for n in _NAMES)
    for name in ("train", "eval_q50"):
        case = _focal_case(name)
        go = _FOCAL_GO[:_FOCAL_CASES[name][0]]
        one = torch.ones_like(case["weight"]).cuda()
        v0, g0 = _run_focal(lambda lg, idx, lab, sz, wt, a, g: focal_classification(lg, idx, lab, sz, a, g), case, torch.float32, go, None)
        v1, g1 = _run_focal(lambda lg, idx, lab, sz, wt, a, g: focal_classification(lg, idx, lab, sz, a, g, weight=wt), case, torch.float32,
                            go, one)
        assert torch.equal(v0, v1) and torch.equal(g0, g1)
    logits, boxes, depth, valid, weight = _depth_map_case()
    for cl in (False, True):
        res = []
        for wt in (None, torch.ones_like(weight).cuda()):
            lg = logits.cuda().contiguous(memory_format=torch.channels_last) if cl else logits.cuda()
            lg.requires_grad_(True)
            out = ddn_loss(lg, boxes.cuda(), depth.cuda(), valid.cuda(), 0.25, 2.0, 13, 1, weight=wt)
            res.append((out.detach(), torch.autograd.grad(out * 1.75, [lg])[0]))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_weights_of_one_half_halve_the_matched_sums_and_gradients_exactly():
    from monosowa_amd.pointwise import matched_losses
    for case_no in (2, 4):
        case = _matched_case(case_no)
        NL = _MATCHED_CASES[case_no][1]
        go = _upstream(NL, case_no)
        F = lambda *a: matched_losses(*a[:-1], weight=a[-1])
        v1, g1 = _run_matched(F, case, torch.float32, go, torch.ones_like(case["weight"]))
        vh, gh = _run_matched(F, case, torch.float32, go, torch.full_like(case["weight"], 0.5))
        assert torch.equal(vh, v1 * 0.5) and all(torch.equal(gh[n], g1[n] * 0.5) for n in _NAMES)
        assert (v1 != 0).all()


def test_two_placements_of_the_outputs_give_the_same_bytes_and_the_codes_are_the_siblings():
    from monosowa_amd import pointwise
    lib = pointwise.load()
    case = _matched_case(2)
    K, NL, B, Q = _MATCHED_CASES[2]
    f32 = lambda k: case[k].cuda().float().contiguous()
    args = [f32("boxes"), f32("depth"), f32("dims"), f32("angle"), case["idx"].cuda().contiguous(), f32("t_box"), f32("t_depth"),
            f32("t_size"), case["t_bin"].cuda().contiguous(), f32("t_res"), f32("weight")]
    ptrs = [a.data_ptr() for a in args]
    go = _upstream(NL, 2).float().cuda().contiguous()
    n = NL * B * Q
    buf = torch.full((2 * n * 35 + 4096,), SENTINEL, dtype=torch.float32, device="cuda")
    got = []
    for off in (3, 1030):
        out, comp = buf[off:off + NL * 6], buf[off + 64:off + 64 + NL]
        assert lib.mono_matched_losses_weighted_fwd_f32(*ptrs, out.data_ptr(), comp.data_ptr(), NL, B, Q, K, None) == 0
        start = 2048 + (0 if off == 3 else n * 35 + 5)
        grads = buf[start:start + n * 35]
        grads.zero_()
        g = [grads[:n * 6], grads[n * 6:n * 8], grads[n * 8:n * 11], grads[n * 11:]]
        assert lib.mono_matched_losses_weighted_bwd_f32(*ptrs, comp.data_ptr(), go.data_ptr(), *[x.data_ptr() for x in g], NL, B, Q, K, None) == 0
        got.append((out, comp, grads))
    torch.cuda.synchronize()
    for a, b in zip(*got):
        assert a.data_ptr() % 16 != b.data_ptr() % 16 or a.numel() > 100
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not (a == SENTINEL).any()
    assert (buf[:3] == SENTINEL).all() and (buf[3 + NL * 6:3 + 64] == SENTINEL).all() and (buf[2048 + 2 * n * 35 + 5:] == SENTINEL).all()
    # focal and depth-map forward outputs at two places
    fc = _focal_case("eval_q50")
    fNL, fB, fQ = _FOCAL_CASES["eval_q50"][:3]
    fa = [fc["logits"].cuda().contiguous(), fc["idx"].cuda().contiguous(), fc["labels"].cuda().contiguous(), fc["sizes"].cuda().contiguous(),
          fc["weight"].cuda().contiguous()]
    fp = [a.data_ptr() for a in fa]
    fK = fc["idx"].shape[2]
    logits, boxes, depth, valid, weight = _depth_map_case()
    da = [logits.cuda(), boxes.cuda().contiguous(), depth.cuda().contiguous(), valid.cuda().contiguous(), weight.cuda().contiguous()]
    dp = [a.data_ptr() for a in da]
    blocks = lib.mono_ddn_loss_blocks(3, 24, 80)
    sb, sc, sp = pointwise._ddn_strides(da[0])
    small = torch.full((2 * blocks + 4096,), SENTINEL, dtype=torch.float32, device="cuda")
    outs = []
    for off in (1, 2 * 1024 + 2 + blocks):
        fo, do = small[off:off + fNL * 3], small[off + 16:off + 16 + blocks]
        assert lib.mono_focal_weighted_fwd_f32(*fp, fo.data_ptr(), fNL, fB, fQ, 3, fK, 0.25, 2.0, None) == 0
        assert lib.mono_ddn_loss_weighted_fwd_f32(*dp, do.data_ptr(), 3, 81, 24, 80, 8, sb, sc, sp, 0.25, 2.0, 13.0, 1.0, 1e-3, 60.0, None) == 0
        outs.append((fo, do))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not (a == SENTINEL).any()
    # return codes: NULL weights -1, bad sizes -2, as the unweighted entry points answer NULL pointers and bad sizes; nothing is launched
    o = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda")
    assert lib.mono_matched_losses_weighted_fwd_f32(*ptrs[:10], None, o.data_ptr(), o[32:].data_ptr(), NL, B, Q, K, None) == -1
    assert lib.mono_matched_losses_weighted_fwd_f32(*ptrs, o.data_ptr(), o[32:].data_ptr(), NL, B, Q, 0, None) == -2
    assert lib.mono_matched_losses_weighted_bwd_f32(*ptrs[:10], None, o.data_ptr(), go.data_ptr(), *[o.data_ptr()] * 4, NL, B, Q, K, None) == -1
    assert lib.mono_focal_weighted_fwd_f32(*fp[:4], None, o.data_ptr(), fNL, fB, fQ, 3, fK, 0.25, 2.0, None) == -1
    assert lib.mono_focal_weighted_fwd_f32(*fp, o.data_ptr(), fNL, 33, 512, 3, fK, 0.25, 2.0, None) == -2
    assert lib.mono_focal_weighted_bwd_f32(*fp[:3], fp[4], o.data_ptr(), o.data_ptr(), fNL, 33, 512, 3, fK, 0.25, 2.0, None) == -2
    assert lib.mono_focal_weighted_fwd_f32(*fp, o.data_ptr(), fNL, fB, fQ, 256, fK, 0.25, 2.0, None) == -2
    assert lib.mono_ddn_loss_weighted_fwd_f32(*dp[:4], None, o.data_ptr(), 3, 81, 24, 80, 8, sb, sc, sp, 0.25, 2.0, 13.0, 1.0, 1e-3, 60.0, None) == -1
    assert lib.mono_ddn_loss_weighted_bwd_f32(*dp, o.data_ptr(), o.data_ptr(), 3, 81, 24, 80, 0, sb, sc, sp, 0.25, 2.0, 13.0, 1.0, 1e-3, 60.0, None) == -2
    torch.cuda.synchronize()
    assert (o == SENTINEL).all()


# =================================================================================================== C: the whole criterion
_KERNEL_NODES = {"_MatchedLossesWeightedBackward", "_FocalClassificationWeightedBackward", "_DDNLossWeightedBackward"}
_PLAIN_NODES = {"_MatchedLossesBackward", "_FocalClassificationBackward", "_DDNLossBackward"}
_GROUPS = (("pred_logits", "logits"), ("pred_boxes", "boxes"), ("pred_depth", "depth"), ("pred_3d_dim", "dims"), ("pred_angle", "angle"),
           ("depth_map_logits", "depth map"))
# name -> (targets per image, queries, train mode, seed)
_LAYOUTS = {
    "mixed_b8": ([0, 50, 1, 0, 23, 50, 7, 3], 550, True, 400),
    "beyond_focal_reach": ([(5 * i) % 9 if i % 3 else 0 for i in range(32)] + [50], 512, False, 401),
}


def _weighted_targets(tg, weights):
    """the TargetList ``prepare_targets`` would hand the criterion: device-resident weights and their host sum"""
    from monosowa_amd.synthetic import TargetList
    out = TargetList(LW.with_weights(tg, weights.to(tg[0]["boxes_3d"].device, tg[0]["boxes_3d"].dtype)))
    out.weight_sum = LW.weight_sum(weights)
    return out


def _evaluate(crit, outputs, targets, weights, on, dtype, focal=True):
    from monosowa_amd.monodetr import criterion as C
    saved = C.FUSED_FOCAL
    with fused_switches(on):
        if not focal:
            C.FUSED_FOCAL = False
        try:
            out, tg = CR.cast_case(outputs, targets, "cuda", dtype)
            if weights is not None:
                tg = _weighted_targets(tg, weights)
            losses = crit(out, tg)
            total = C.weighted_total(losses, crit.weight_dict)
            nodes = _node_names([total])
            leaves = CR.leaves_of(out)
            grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
            grads = {n: (torch.zeros_like(v) if g is None else g).detach() for (n, v), g in zip(leaves.items(), grads)}
            values = {k: losses[k].detach().clone() for k in losses.keys()}
        finally:
            C.FUSED_FOCAL = saved
    return values, total.detach(), grads, nodes


def _rows(name, g):
    return g.permute(0, 2, 3, 1) if name == "depth_map_logits" else g


def _compare(label, runs, vR, tR, gR):
    bounds = {"logits": C_LOGITS, "boxes": C_BOXES, "depth": C_DEPTH, "dims": C_DIMS, "angle": C_ANGLE, "depth map": C_DEPTH_MAP}
    bad = []
    for tag, (v, t, g) in runs.items():
        if tag == "P":
            continue
        vP, tP, gP = runs["P"]
        diff = [k for k in vR if not k.startswith(("class_error", "cardinality_error"))]
        e_f = max([_rel(v[k], vR[k]) for k in diff] + [_rel(t, tR)])
        e_p = max([_rel(vP[k], vR[k]) for k in diff] + [_rel(tP, tR)])
        _show("C", label + " " + tag, "loss", e_f, e_p, C_LOSS)
        _check(bad, tag + " loss", e_f, e_p, C_LOSS)
        for k in vR:
            if k.startswith(("class_error", "cardinality_error")):
                for who, x in ((tag, v), ("P", vP)):
                    if abs(float(x[k]) - float(vR[k])) > COUNT_RTOL * abs(float(vR[k])):
                        bad.append((k, who, float(x[k]), float(vR[k])))
        for key, group in _GROUPS:
            names = [n for n in gR if n.endswith(key)]
            e_f = max(CR.row_error(_rows(n, g[n]), _rows(n, gR[n])) for n in names)
            e_p = max(CR.row_error(_rows(n, gP[n]), _rows(n, gR[n])) for n in names)
            _show("C", label + " " + tag, group, e_f, e_p, bounds[group])
            _check(bad, tag + " " + group, e_f, e_p, bounds[group])
    return bad


def _reference(crit, outputs, targets, weights, idx, groups):
    out, tg = CR.cast_case(outputs, targets, "cuda", torch.float64)
    tg = LW.with_weights(tg, weights.cuda().double())
    want = LW.criterion_losses(out, tg, idx.cuda(), LW.num_boxes(weights, groups), crit.focal_alpha, crit.depth_map_size)
    total = sum(want[k] * float(crit.weight_dict[k]) for k in want if k in crit.weight_dict)
    leaves = CR.leaves_of(out)
    grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    grads = {n: (torch.zeros_like(v) if g is None else g).detach() for (n, v), g in zip(leaves.items(), grads)}
    return {k: v.detach() for k, v in want.items()}, total.detach(), grads


@pytest.mark.parametrize("name", list(_LAYOUTS))
def test_weighted_criterion_routes_equal_float64(name):
    """F: the fused tail (four weighted launches behind the matching); F2: FUSED_FOCAL off -- the classification side in plain PyTorch,
    the matched-pair losses through the weighted kernel; P: every switch plain.  One image beyond FOCAL_WEIGHTED_MAX_CELLS the predicate
    says no and F itself takes F2's route."""
    from monosowa_amd.pointwise import focal_classification_weighted_supported
    sizes, Q, train, seed = _LAYOUTS[name]
    outputs, targets = CR.make_layout_case(seed, sizes, Q)
    weights = LW.draw_weights(seed + 1000, sum(sizes))
    assert (weights == 0).any() and (weights > 1).any()
    crit = _criterion(train)
    groups = crit.group_num if train else 1
    vF, tF, gF, nF = _evaluate(crit, outputs, targets, weights, True, torch.float32)
    idx = torch.from_numpy(crit.matcher.idx)
    st, ft = CR.stack_layers(outputs), CR.flat_targets(targets)
    _, margins = CR.census(st["pred_boxes"], st["pred_depth"], st["pred_3d_dim"], st["pred_angle"], idx, ft["boxes_3d"], ft["depth"],
                           ft["size_3d"], ft["heading_bin"], ft["heading_res"])
    assert min(margins.values()) >= CR.MARGIN, margins
    v2, t2, g2, n2 = _evaluate(crit, outputs, targets, weights, True, torch.float32, focal=False)
    vP, tP, gP, nP = _evaluate(crit, outputs, targets, weights, False, torch.float32)
    vR, tR, gR = _reference(crit, outputs, targets, weights, idx, groups)
    reach = focal_classification_weighted_supported(torch.zeros(3, len(sizes), Q, 3, device="cuda"), idx.cuda())
    if name == "beyond_focal_reach":
        assert len(sizes) * Q == _max_cells() + Q and not reach
        assert _KERNEL_NODES & nF == {"_MatchedLossesWeightedBackward", "_DDNLossWeightedBackward"}, sorted(nF)
    else:
        assert reach and _KERNEL_NODES <= nF, sorted(_KERNEL_NODES - nF)
    assert _KERNEL_NODES & n2 == {"_MatchedLossesWeightedBackward", "_DDNLossWeightedBackward"}, sorted(n2)
    assert not (_KERNEL_NODES | _PLAIN_NODES) & nP and not _PLAIN_NODES & (nF | n2)
    bad = _compare(name, {"F": (vF, tF, gF), "F2": (v2, t2, g2), "P": (vP, tP, gP)}, vR, tR, gR)
    # a weight of 0: every gradient row of every query matched to the label, in every layer and every head, is exactly 0
    zero = (weights[idx[2]] == 0)
    for g in (gF, g2):
        for l in range(3):
            for key in CR.PRED_KEYS:
                rows = g["l%d.%s" % (l, key)].cpu()[idx[0, l], idx[1, l]]
                assert zero[l].any() and (rows[zero[l]] == 0).all(), (l, key)
                assert (rows[~zero[l]].abs().sum(1) > 0).all(), (l, key)
    assert not bad, "(group, e_F, e_P) beyond the bound: %s" % bad


def test_fused_criterion_with_weights_of_one_equals_the_key_absent_run_bit_for_bit():
    sizes, Q, train, seed = _LAYOUTS["mixed_b8"]
    outputs, targets = CR.make_layout_case(seed, sizes, Q)
    crit = _criterion(train)
    v0, t0, g0, n0 = _evaluate(crit, outputs, targets, None, True, torch.float32)
    v1, t1, g1, n1 = _evaluate(crit, outputs, targets, torch.ones(sum(sizes)), True, torch.float32)
    assert _PLAIN_NODES <= n0 and not _KERNEL_NODES & n0 and _KERNEL_NODES <= n1 and not _PLAIN_NODES & n1
    assert set(v0) == set(v1) and len(v0) > 20
    for k in v0:
        assert torch.equal(v0[k], v1[k]), k
    assert torch.equal(t0, t1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


def test_device_resident_weights_without_a_host_copy_are_refused(dev):
    from monosowa_amd.helpers.trainer_helper import Trainer
    from monosowa_amd.synthetic import attach_host_weight, make_batch, prepare_targets
    _, _, targets, _ = make_batch(2, dev, seed=3, resolution=RES)
    targets["label_weight"] = torch.ones(2, 50, device=dev)
    with pytest.raises(ValueError, match="attach_host_weight"):
        prepare_targets(targets, 2)
    with pytest.raises(ValueError, match="attach_host_weight"):
        Trainer._host_box_count((None, None, targets, None))
    attach_host_weight(targets["label_weight"], np.full((2, 50), 0.5, np.float32))
    n = int(targets["mask_2d"]._host_mask.sum())
    assert prepare_targets(targets, 2).weight_sum == 0.5 * n == Trainer._host_box_count((None, None, targets, None))
    crit = _criterion(True)
    tl = [dict(t) for t in prepare_targets(targets, 2)]
    with pytest.raises(ValueError, match="weight_sum"):
        crit._num_boxes(tl, 11, dev)


# =================================================================================================== the Trainer
SEEDS = [3, 7, 11, 13, 17, 19]


def _give_weights(rig, seed=9):
    """a ``label_weight`` of mixed values in every batch of the rig's loader; -> the valid labels' weights per batch"""
    per_batch = []
    for i, batch in enumerate(rig.loader.batches):
        mask = batch[2]["mask_2d"].numpy()
        w = np.ones((2, 50), np.float32)
        w[mask] = LW.draw_weights(seed + i, int(mask.sum())).numpy()
        batch[2]["label_weight"] = torch.from_numpy(w)
        per_batch.append(w[mask])
    return per_batch


def _steps(rig, K, steps, first=0):
    from monosowa_amd.helpers.trainer_helper import stage_batch
    out = []
    for s in range(first, first + steps):
        rig.k = s * K
        raws = rig.loader.batches[s * K:(s + 1) * K]
        total, ld = rig.trainer.train_step(*stage_batch(raws[0], rig.trainer.device)) if K == 1 else rig.trainer.train_cycle(raws)
        out.append(total.detach().clone())
    return out


@pytest.mark.parametrize("K", [1, 2])
def test_weighted_steps_do_not_synchronise_and_train_differently(shared, K):
    cfg = {"global_batch": 4} if K == 2 else {}
    plain = _Rig(shared, SEEDS[:3 * K], **cfg)
    _steps(plain, K, 3)
    rig = _Rig(shared, SEEDS[:3 * K], **cfg)
    per_batch = _give_weights(rig)
    assert any((w == 0).any() for w in per_batch) and any((w > 1).any() for w in per_batch)
    seen = []
    forward = rig.crit.forward
    rig.crit.forward = lambda *a, **k: (seen.append(k.get("num_boxes")), forward(*a, **k))[1]
    try:
        _steps(rig, K, 1)                                  # plans, tables and kernel selection belong to the first step
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        try:
            torch.cuda.set_sync_debug_mode("warn")
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                totals = _steps(rig, K, 2, first=1)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    finally:
        rig.crit.__dict__.pop("forward", None)
    assert [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()] == []
    assert all(torch.isfinite(t) for t in totals) and len(seen) == 3 * K
    if K == 2:                                             # the normaliser of a cycle: the weight sum of both its batches
        for s in range(3):
            want = LW.num_boxes(np.concatenate(per_batch[2 * s:2 * s + 2]), rig.crit.group_num, ranks=2)
            assert seen[2 * s] == seen[2 * s + 1] == want
    else:
        assert seen == [None] * 3
    a, b = plain.state(), rig.state()
    assert set(a) == set(b) and any(not torch.equal(a[k], b[k]) for k in a if k.startswith("param."))
    differ = [k for k in a if k.startswith("param.") and "class_embed" in k and not torch.equal(a[k], b[k])]
    assert differ
