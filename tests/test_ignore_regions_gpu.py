"""Ignore regions on the GPU: ``mono_ignore_flags_f32``, the four focal entry points with flag bytes (csrc/matched_losses.hip), the
criterion's routes that run them and train steps of the shipped architecture with ignore boxes in the batch.

F is the kernel (``pointwise.ignore_flags`` / ``focal_classification`` with ``ignore=``, or the whole ``SetCriterion`` with every switch
of tests/fused_switches.py shipped), P the plain formulation in float32 on the GPU (tests/ignore_reference.py in float32; for the whole
criterion: every switch plain), R tests/ignore_reference.py in float64.  The flags have no tolerance: numpy float32 gives their bytes.

Metrics: those of tests/test_criterion_kernels_gpu.py -- |x - x_R| / max(|x_R|, tiny) per loss value, ``criterion_reference.row_error``
per gradient tensor.

Bounds: one per tensor group, 4 x the worst e_P of the group over every case of its section on the MI355X, rounded up to one significant
digit; F and P must both meet it.  The measured worst e_F / e_P stand beside each constant.

Exact properties (no tolerance): an ignored row of the gradient is +0.0, every other row and -- with all flags zero -- every value is the
sibling kernel's, the two logging columns are the sibling's whatever the flags, and the bytes do not depend on where the outputs lie."""
import warnings

import numpy as np
import pytest
import torch

import criterion_reference as CR
import ignore_reference as IR
import label_weights_reference as LW
from fused_switches import fused_switches
from test_accumulation_gpu import RES, _Rig, dev, shared      # noqa: F401  (fixtures)
from test_criterion_kernels_gpu import _criterion, _node_names, _rel, _show

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
IOA = 0.5

# Section A (the focal kernels alone): worst e_F / worst e_P over the cases (in brackets the case of the worst e_P), and 4 x e_P before
# rounding
A_FOCAL_VALUE = 3e-7   # 1.2e-7 / 6.5e-8 (exactly 32,768 cells), 2.6e-7: per-layer focal sum with ignored cells left out
A_FOCAL_LOGITS = 7e-6  # 2.0e-6 / 1.7e-6 (K 257, plain), 6.6e-6
# Section C (the whole criterion: the fused tail, the matched kernels alone, one image beyond the weighted focal kernel's reach)
C_LOSS = 8e-7          # 1.6e-7 / 2.0e-7 (beyond_weighted_focal_reach), 7.9e-7: every loss key and the weighted total
C_LOGITS = 8e-6        # 1.8e-6 / 1.8e-6 (beyond_weighted_focal_reach), 7.1e-6
C_OTHER = 2e-6         # 4.1e-7 / 4.1e-7 (beyond_weighted_focal_reach), 1.6e-6: boxes, depth, sizes, angles and the depth map together


def _check(bad, group, e_f, e_p, bound):
    if max(e_f, e_p) > bound:
        bad.append((group, e_f, e_p))


# =================================================================================================== the flags kernel
_FLAG_CASES = {"single": (1, 1, 5, 1, None), "three_images_q70": (2, 3, 70, 3, 1), "full_slots_q400": (3, 3, 400, 50, None)}


@pytest.mark.parametrize("name", list(_FLAG_CASES))
def test_flags_kernel_equals_the_numpy_float32_restatement(name):
    from monosowa_amd import pointwise
    from monosowa_amd.pointwise import ignore_flags, ignore_flags_supported
    NL, B, Q, M, empty = _FLAG_CASES[name]
    boxes, ign, mask = IR.make_flag_case(40 + NL, NL, B, Q, M, empty_image=empty)
    if name == "single":                                         # (1, 1, 1, 1): one cell -- each planted row in turn, then all five
        for q in range(5):
            one = np.ascontiguousarray(boxes[:, :, q:q + 1])
            got, n = ignore_flags(torch.from_numpy(one).cuda(), torch.from_numpy(ign).cuda(), torch.from_numpy(mask).cuda(), IOA)
            assert got.shape == (1, 1, 1) and int(got) == IR.PLANTED_FLAGS[q] == int(n[0]) == IR.flags(one, ign, mask, IOA)[0].item()
    rng = np.random.default_rng(7)
    rb = np.concatenate([rng.uniform(0.1, 0.9, (NL, B, Q, 2)), rng.uniform(0.0, 0.15, (NL, B, Q, 4))], -1).astype(np.float32)
    lo = rng.uniform(0, 0.7, (B, M, 2))
    rg = np.concatenate([lo, lo + rng.uniform(0.02, 0.3, (B, M, 2))], -1).astype(np.float32)
    nan_boxes = rg.copy()
    nan_boxes[..., 3] = np.nan
    runs = [(boxes, ign, mask, IOA), (rb, rg, mask, 0.5), (rb, rg, mask, 0.3), (rb, rg, mask, 1.0), (rb, rg, np.zeros((B, M), bool), 0.5),
            (rb, nan_boxes, mask, 0.5)]
    for i, (p, g, m, ioa) in enumerate(runs):
        pt = torch.from_numpy(p).cuda()
        assert ignore_flags_supported(pt)
        buf = torch.full((NL * B * Q + 64,), 99, dtype=torch.uint8, device="cuda")      # the launch writes its cells and nothing else
        counts = torch.full((NL + 2,), -5, dtype=torch.int32, device="cuda")
        gm = torch.from_numpy(m).cuda().view(torch.uint8)
        code = pointwise.load().mono_ignore_flags_f32(pt.data_ptr(), torch.from_numpy(g).cuda().data_ptr(), gm.data_ptr(),
                                                     buf[32:].data_ptr(), counts[1:].data_ptr(), NL, B, Q, M, float(ioa), None)
        assert code == 0
        got, n = ignore_flags(pt, torch.from_numpy(g).cuda(), torch.from_numpy(m).cuda(), ioa)
        want, want_n = IR.flags(p, g, m, ioa)
        assert got.dtype == torch.uint8 and n.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(n.cpu().numpy(), want_n), (name, i)
        assert np.array_equal(buf[32:32 + NL * B * Q].cpu().numpy().reshape(NL, B, Q), want) and counts[1:NL + 1].tolist() == want_n.tolist()
        assert (buf[:32] == 99).all() and (buf[32 + NL * B * Q:] == 99).all() and counts[0] == -5 and counts[NL + 1] == -5
        if i == 0 or (i in (1, 2) and Q >= 70):
            assert 0 < want.sum() < want.size, (name, i)
        if i >= 4:
            assert not want.any()
    want = IR.flags(boxes, ign, mask, IOA)[0]
    assert tuple(want[0, 0, :5]) == IR.PLANTED_FLAGS or M > 1
    if empty is not None:
        assert not want[:, empty].any()
    lib = pointwise.load()
    o = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert lib.mono_ignore_flags_f32(None, o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), 1, 1, 1, 1, 0.5, None) == -1
    assert lib.mono_ignore_flags_f32(o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), None, 1, 1, 1, 1, 0.5, None) == -1
    assert lib.mono_ignore_flags_f32(o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), 1, 1, 1, 0, 0.5, None) == -2
    assert lib.mono_ignore_flags_f32(o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), o.data_ptr(), 0, 1, 1, 1, 0.5, None) == -2


# =================================================================================================== A: focal kernels
# name -> (NL, B, Q, sizes, groups): K = groups * sum(sizes) in {0, 5, 257} on the smallest shapes, and one case at exactly each sibling's
# cell limit
_FOCAL_CASES = {
    "K0_one_cell": (1, 1, 1, [0], 1),
    "K5_q70": (2, 3, 70, [2, 0, 3], 1),
    "K257_q400": (3, 3, 400, [257, 0, 0], 1),
    "limit_weighted_16384": (3, 32, 512, [(7 * i) % 11 if i % 4 else 0 for i in range(31)] + [50], 10),
    "limit_plain_32768": (3, 64, 512, [(7 * i) % 11 if i % 4 else 0 for i in range(63)] + [50], 10),
}
_FOCAL_GO = torch.tensor([[0.5, 3.0, 7.0], [-1.25, 5.0, 11.0], [2.0, 13.0, 17.0]], dtype=torch.float64)


def _focal_case(name):
    NL, B, Q, sizes, groups = _FOCAL_CASES[name]
    no = list(_FOCAL_CASES).index(name)
    case = CR.make_focal_case(731 + no, NL, B, Q, sizes, groups)
    case["weight"] = LW.draw_weights(831 + no, sum(sizes))
    rng = np.random.default_rng(931 + no)
    flag = (rng.random((NL, B, Q)) < 0.3).astype(np.uint8)
    if B * Q == 1:
        flag[:] = 1
    for l in range(NL):                                          # flagged cells that are matched are there too: they keep their terms
        k = case["idx"].shape[2]
        if k:
            flag[l, case["idx"][0, l, :(k + 1) // 2], case["idx"][1, l, :(k + 1) // 2]] = 1
    case["flag"] = torch.from_numpy(flag)
    case["ignored"] = IR.ignored_cells(flag, case["idx"])
    return case


def _run_focal(fn, case, dtype, go, logits=None):
    logits = (case["logits"] if logits is None else logits).cuda().to(dtype).requires_grad_(True)
    out = fn(logits, case["idx"].cuda(), case["labels"].cuda(), case["sizes"].cuda().to(dtype))
    (grad,) = torch.autograd.grad((out * go.to(device="cuda", dtype=out.dtype))[:, 0].sum(), [logits])
    return out.detach(), grad


def _focal_fns(case, weighted, flag=None):
    from monosowa_amd.pointwise import focal_classification
    w = case["weight"].cuda() if weighted else None
    flag = (case["flag"] if flag is None else flag).cuda()
    F = lambda lg, idx, lab, sz: focal_classification(lg, idx, lab, sz, 0.25, 2.0, weight=w, ignore=flag)
    S = lambda lg, idx, lab, sz: focal_classification(lg, idx, lab, sz, 0.25, 2.0, weight=w)
    P = lambda lg, idx, lab, sz: IR.focal_sums(lg, idx, lab, sz, None if w is None else w.to(lg.dtype), case["ignored"], 0.25, 2.0)
    return F, S, P


def _focal_params():
    from monosowa_amd.pointwise import FOCAL_WEIGHTED_MAX_CELLS
    out = []
    for name, (NL, B, Q, sizes, groups) in _FOCAL_CASES.items():
        out.append((name, False))
        if B * Q <= FOCAL_WEIGHTED_MAX_CELLS:
            out.append((name, True))
    return out


@pytest.mark.parametrize("name,weighted", _focal_params(), ids=lambda v: v if isinstance(v, str) else ("weighted" if v else "plain"))
def test_focal_ignore_kernels_equal_float64_and_their_siblings(name, weighted):
    from monosowa_amd import pointwise
    NL, B, Q, sizes, groups = _FOCAL_CASES[name]
    if name == "limit_weighted_16384":
        assert B * Q == pointwise.FOCAL_WEIGHTED_MAX_CELLS == pointwise.load().mono_focal_weighted_max_cells()
    if name == "limit_plain_32768":
        assert B * Q == 32768
    case = _focal_case(name)
    K = case["idx"].shape[2]
    assert K == groups * sum(sizes) and (name[0] != "K" or K == int(name[1:name.index("_")]))
    ignored, flag = case["ignored"], case["flag"].bool()
    assert ignored.any() and (K == 0 or (flag & ~ignored).any())
    F, S, P = _focal_fns(case, weighted)
    go = _FOCAL_GO[:NL]
    vF, gF = _run_focal(F, case, torch.float32, go)
    vS, gS = _run_focal(S, case, torch.float32, go)
    vP, gP = _run_focal(P, case, torch.float32, go)
    vR, gR = _run_focal(P, case, torch.float64, go)
    assert vF.shape == (NL, 3) and torch.isfinite(vF).all() and torch.isfinite(gF).all()
    bad = []
    label = "%s %s" % (name, "weighted" if weighted else "plain")
    e_f = max(_rel(vF[l, 0], vR[l, 0]) for l in range(NL))
    e_p = max(_rel(vP[l, 0], vR[l, 0]) for l in range(NL))
    _show("A", label, "focal value", e_f, e_p, A_FOCAL_VALUE)
    _check(bad, "focal value", e_f, e_p, A_FOCAL_VALUE)
    g_f, g_p = CR.row_error(gF, gR), CR.row_error(gP, gR)
    _show("A", label, "focal logits", g_f, g_p, A_FOCAL_LOGITS)
    _check(bad, "focal logits", g_f, g_p, A_FOCAL_LOGITS)
    # the two logging columns count every cell: the sibling's bytes
    assert torch.equal(vF[:, 1:], vS[:, 1:])
    # ignored rows: +0.0 bit for bit; every other row: the sibling's
    ig = ignored.cuda()
    assert (gF[ig].view(torch.int32) == 0).all() and torch.equal(gF[~ig], gS[~ig])
    if B * Q > 1:
        assert (gS[ig].abs().sum(1) > 0).float().mean() > 0.5 and (vF[:, 0] < vS[:, 0]).all()
    # all flags zero: the sibling's values and gradients
    F0, _, _ = _focal_fns(case, weighted, torch.zeros_like(case["flag"]))
    v0, g0 = _run_focal(F0, case, torch.float32, go)
    assert torch.equal(v0, vS) and torch.equal(g0, gS)
    # +inf / NaN logits in ignored cells: the sum and every other gradient are what they were
    poisoned = case["logits"].clone()
    cells = torch.nonzero(ignored)
    poisoned[tuple(cells[0])] = torch.tensor([float("inf"), float("nan"), 1.0])
    poisoned[tuple(cells[-1])] = float("nan")
    poisoned[tuple(cells[len(cells) // 2])] = float("inf")
    vN, gN = _run_focal(F, case, torch.float32, go, poisoned)
    assert torch.equal(vN[:, 0], vF[:, 0]) and torch.equal(gN, gF)
    assert not bad, "(group, e_F, e_P) beyond the bound: %s" % bad


def test_two_placements_of_the_outputs_give_the_same_bytes_and_the_codes_are_the_siblings():
    from monosowa_amd import pointwise
    lib = pointwise.load()
    name = "K257_q400"
    NL, B, Q, sizes, groups = _FOCAL_CASES[name]
    case = _focal_case(name)
    K = case["idx"].shape[2]
    a = [case["logits"].cuda().contiguous(), case["idx"].cuda().contiguous(), case["labels"].cuda().contiguous(),
         case["sizes"].cuda().contiguous(), case["weight"].cuda().contiguous(), case["flag"].cuda().contiguous()]
    lg, idx, lab, sz, wt, fl = [t.data_ptr() for t in a]
    go = _FOCAL_GO[:NL, 0].float().cuda().contiguous()
    n = NL * B * Q * 3
    buf = torch.full((2 * n + 4096,), SENTINEL, dtype=torch.float32, device="cuda")
    got = []
    for off in (1, 1030):
        o1, o2 = buf[off:off + NL * 3], buf[off + 32:off + 32 + NL * 3]
        start = 2048 + (0 if off == 1 else n + 5)
        g1 = buf[start:start + n]
        assert lib.mono_focal_ignore_fwd_f32(lg, idx, lab, sz, fl, o1.data_ptr(), NL, B, Q, 3, K, 0.25, 2.0, None) == 0
        assert lib.mono_focal_weighted_ignore_fwd_f32(lg, idx, lab, sz, wt, fl, o2.data_ptr(), NL, B, Q, 3, K, 0.25, 2.0, None) == 0
        assert lib.mono_focal_ignore_bwd_f32(lg, idx, lab, fl, go.data_ptr(), g1.data_ptr(), NL, B, Q, 3, K, 0.25, 2.0, None) == 0
        torch.cuda.synchronize()
        plain = g1.clone()
        assert lib.mono_focal_weighted_ignore_bwd_f32(lg, idx, lab, wt, fl, go.data_ptr(), g1.data_ptr(), NL, B, Q, 3, K, 0.25, 2.0, None) == 0
        torch.cuda.synchronize()
        got.append((o1.clone(), o2.clone(), plain, g1.clone()))
        g1.fill_(SENTINEL)
    for x, y in zip(*got):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and not (x == SENTINEL).any()
    assert (buf[:1] == SENTINEL).all() and (buf[1 + 32 + NL * 3:1030] == SENTINEL).all() and (buf[1030 + 32 + NL * 3:2048] == SENTINEL).all()
    assert (buf[2048:] == SENTINEL).all()
    # return codes: those of the siblings for a NULL pointer, K < 0 and too many cells; a NULL flag pointer is a NULL pointer; nothing is
    # launched
    o = torch.full((64,), SENTINEL, dtype=torch.float32, device="cuda")
    op = o.data_ptr()
    sib = [lib.mono_focal_fwd_f32(None, idx, lab, sz, op, NL, B, Q, 3, K, 0.25, 2.0, None),
           lib.mono_focal_fwd_f32(lg, idx, lab, sz, op, NL, B, Q, 3, -1, 0.25, 2.0, None),
           lib.mono_focal_fwd_f32(lg, idx, lab, sz, op, NL, 65, 512, 3, K, 0.25, 2.0, None),
           lib.mono_focal_bwd_f32(lg, idx, lab, None, op, NL, B, Q, 3, K, 0.25, 2.0, None),
           lib.mono_focal_bwd_f32(lg, idx, lab, op, op, NL, B, Q, 3, -1, 0.25, 2.0, None),
           lib.mono_focal_bwd_f32(lg, idx, lab, op, op, NL, 65, 512, 3, K, 0.25, 2.0, None),
           lib.mono_focal_weighted_fwd_f32(lg, idx, lab, sz, None, op, NL, B, Q, 3, K, 0.25, 2.0, None),
           lib.mono_focal_weighted_fwd_f32(lg, idx, lab, sz, wt, op, NL, B, Q, 3, -1, 0.25, 2.0, None),
           lib.mono_focal_weighted_fwd_f32(lg, idx, lab, sz, wt, op, NL, 33, 512, 3, K, 0.25, 2.0, None),
           lib.mono_focal_weighted_bwd_f32(lg, idx, lab, None, op, op, NL, B, Q, 3, K, 0.25, 2.0, None),
           lib.mono_focal_weighted_bwd_f32(lg, idx, lab, wt, op, op, NL, B, Q, 3, -1, 0.25, 2.0, None),
           lib.mono_focal_weighted_bwd_f32(lg, idx, lab, wt, op, op, NL, 33, 512, 3, K, 0.25, 2.0, None)]
    new = [lib.mono_focal_ignore_fwd_f32(None, idx, lab, sz, fl, op, NL, B, Q, 3, K, 0.25, 2.0, None),
           lib.mono_focal_ignore_fwd_f32(lg, idx, lab, sz, fl, op, NL, B, Q, 3, -1, 0.25, 2.0, None),
           lib.mono_focal_ignore_fwd_f32(lg, idx, lab, sz, fl, op, NL, 65, 512, 3, K, 0.25, 2.0, None),
           lib.mono_focal_ignore_bwd_f32(lg, idx, lab, fl, None, op, NL, B, Q, 3, K, 0.25, 2.0, None),
           lib.mono_focal_ignore_bwd_f32(lg, idx, lab, fl, op, op, NL, B, Q, 3, -1, 0.25, 2.0, None),
           lib.mono_focal_ignore_bwd_f32(lg, idx, lab, fl, op, op, NL, 65, 512, 3, K, 0.25, 2.0, None),
           lib.mono_focal_weighted_ignore_fwd_f32(lg, idx, lab, sz, None, fl, op, NL, B, Q, 3, K, 0.25, 2.0, None),
           lib.mono_focal_weighted_ignore_fwd_f32(lg, idx, lab, sz, wt, fl, op, NL, B, Q, 3, -1, 0.25, 2.0, None),
           lib.mono_focal_weighted_ignore_fwd_f32(lg, idx, lab, sz, wt, fl, op, NL, 33, 512, 3, K, 0.25, 2.0, None),
           lib.mono_focal_weighted_ignore_bwd_f32(lg, idx, lab, None, fl, op, op, NL, B, Q, 3, K, 0.25, 2.0, None),
           lib.mono_focal_weighted_ignore_bwd_f32(lg, idx, lab, wt, fl, op, op, NL, B, Q, 3, -1, 0.25, 2.0, None),
           lib.mono_focal_weighted_ignore_bwd_f32(lg, idx, lab, wt, fl, op, op, NL, 33, 512, 3, K, 0.25, 2.0, None)]
    assert new == sib == [-1, -2, -2] * 4
    assert lib.mono_focal_ignore_fwd_f32(lg, idx, lab, sz, None, op, NL, B, Q, 3, K, 0.25, 2.0, None) == -1
    assert lib.mono_focal_ignore_bwd_f32(lg, idx, lab, None, op, op, NL, B, Q, 3, K, 0.25, 2.0, None) == -1
    assert lib.mono_focal_weighted_ignore_fwd_f32(lg, idx, lab, sz, wt, None, op, NL, B, Q, 3, K, 0.25, 2.0, None) == -1
    assert lib.mono_focal_weighted_ignore_bwd_f32(lg, idx, lab, wt, None, op, op, NL, B, Q, 3, K, 0.25, 2.0, None) == -1
    torch.cuda.synchronize()
    assert (o == SENTINEL).all()


# =================================================================================================== C: the whole criterion
_IGNORE_NODE = "_FocalClassificationIgnoreBackward"
_FOCAL_NODES = {"_FocalClassificationBackward", "_FocalClassificationWeightedBackward"}
_GROUPS = (("pred_logits", "logits"), ("pred_boxes", "other"), ("pred_depth", "other"), ("pred_3d_dim", "other"), ("pred_angle", "other"),
           ("depth_map_logits", "other"))
# name -> (targets per image, queries, train mode, seed, with label weights)
_LAYOUTS = {
    "mixed_b4": ([0, 9, 1, 4], 110, True, 410, False),
    "mixed_b4_weighted": ([0, 9, 1, 4], 110, True, 411, True),
    "beyond_weighted_focal_reach": ([(5 * i) % 9 if i % 3 else 0 for i in range(32)] + [50], 512, False, 412, True),
}


def _ignore_boxes(B, seed, empty_image=1, M=6, valid=3):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0.05, 0.6, (B, M, 2))
    boxes = np.concatenate([lo, lo + rng.uniform(0.15, 0.35, (B, M, 2))], -1).astype(np.float32)
    mask = np.zeros((B, M), bool)
    mask[:, :valid] = True
    mask[empty_image] = False
    boxes[~mask] = 0
    return boxes, mask


def _targets(tg, weights, ignore):
    from monosowa_amd.synthetic import TargetList
    if weights is not None:
        tg = LW.with_weights(tg, weights.to(tg[0]["boxes_3d"].device, tg[0]["boxes_3d"].dtype))
    out = TargetList(tg)
    if weights is not None:
        out.weight_sum = LW.weight_sum(weights)
    if ignore is not None:
        out.ignore = (torch.from_numpy(ignore[0]).cuda(), torch.from_numpy(ignore[1]).cuda())
    return out


def _evaluate(crit, outputs, targets, weights, ignore, on, focal=True):
    from monosowa_amd.monodetr import criterion as C
    saved = C.FUSED_FOCAL
    with fused_switches(on):
        if not focal:
            C.FUSED_FOCAL = False
        try:
            out, tg = CR.cast_case(outputs, targets, "cuda", torch.float32)
            losses = crit(out, _targets(tg, weights, ignore))
            total = C.weighted_total(losses, crit.weight_dict)
            nodes = _node_names([total])
            leaves = CR.leaves_of(out)
            grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
            grads = {n: (torch.zeros_like(v) if g is None else g).detach() for (n, v), g in zip(leaves.items(), grads)}
            values = {k: losses[k].detach().clone() for k in losses.keys()}
        finally:
            C.FUSED_FOCAL = saved
    return values, total.detach(), grads, nodes


def _reference(crit, outputs, targets, weights, ignore, idx, groups):
    out, tg = CR.cast_case(outputs, targets, "cpu", torch.float64)
    w = weights if weights is not None else torch.ones(sum(len(t["labels"]) for t in targets))
    tg = LW.with_weights(tg, w.double())
    want, ignored = IR.criterion_losses(out, tg, idx, LW.num_boxes(w, groups), crit.focal_alpha, crit.depth_map_size, ignore[0], ignore[1], IOA)
    total = sum(want[k] * float(crit.weight_dict[k]) for k in want if k in crit.weight_dict)
    leaves = CR.leaves_of(out)
    grads = torch.autograd.grad(total, list(leaves.values()), allow_unused=True)
    grads = {n: (torch.zeros_like(v) if g is None else g).detach() for (n, v), g in zip(leaves.items(), grads)}
    return {k: v.detach() for k, v in want.items()}, total.detach(), grads, ignored


def _rows(name, g):
    return g.permute(0, 2, 3, 1) if name == "depth_map_logits" else g


@pytest.mark.parametrize("name", list(_LAYOUTS))
def test_criterion_routes_with_ignore_boxes_equal_float64(name):
    """F: the fused tail (the focal launches through the ignore entry points); F2: FUSED_FOCAL off -- the classification side in plain
    PyTorch, the matched-pair losses through their kernel; P: every switch plain.  One image beyond FOCAL_WEIGHTED_MAX_CELLS the weighted
    predicate says no and F itself takes F2's route."""
    from monosowa_amd import pointwise
    sizes, Q, train, seed, weighted = _LAYOUTS[name]
    outputs, targets = CR.make_layout_case(seed, sizes, Q)
    weights = LW.draw_weights(seed + 1000, sum(sizes)) if weighted else None
    ignore = _ignore_boxes(len(sizes), seed + 2000)
    crit = _criterion(train)
    groups = crit.group_num if train else 1
    vF, tF, gF, nF = _evaluate(crit, outputs, targets, weights, ignore, True)
    reportF = crit.ignore_report()
    idx = torch.from_numpy(crit.matcher.idx)
    v2, t2, g2, n2 = _evaluate(crit, outputs, targets, weights, ignore, True, focal=False)
    vP, tP, gP, nP = _evaluate(crit, outputs, targets, weights, ignore, False)
    vR, tR, gR, ignored = _reference(crit, outputs, targets, weights, ignore, idx, groups)
    n_ignored = ignored.sum((1, 2)).tolist()
    assert min(n_ignored) > 0 and not ignored[:, 1].any()
    assert reportF == (n_ignored, len(sizes) * Q) == crit.ignore_report()
    if name == "beyond_weighted_focal_reach":
        assert len(sizes) * Q == pointwise.FOCAL_WEIGHTED_MAX_CELLS + Q and _IGNORE_NODE not in nF
    else:
        assert _IGNORE_NODE in nF
    assert _IGNORE_NODE not in n2 and _IGNORE_NODE not in nP and not _FOCAL_NODES & (nF | n2 | nP)
    bounds = {"logits": C_LOGITS, "other": C_OTHER}
    bad = []
    for tag, (v, t, g) in {"F": (vF, tF, gF), "F2": (v2, t2, g2)}.items():
        diff = [k for k in vR if not k.startswith(("class_error", "cardinality_error"))]
        e_f = max([_rel(v[k], vR[k]) for k in diff] + [_rel(t, tR)])
        e_p = max([_rel(vP[k], vR[k]) for k in diff] + [_rel(tP, tR)])
        _show("C", name + " " + tag, "loss", e_f, e_p, C_LOSS)
        _check(bad, tag + " loss", e_f, e_p, C_LOSS)
        for k in vR:
            if k.startswith(("class_error", "cardinality_error")):
                assert abs(float(v[k]) - float(vR[k])) <= 2.0 ** -22 * abs(float(vR[k])), (tag, k)
        for group in ("logits", "other"):
            names = [n for n in gR for key, grp in _GROUPS if grp == group and n.endswith(key)]
            e_f = max(CR.row_error(_rows(n, g[n]), _rows(n, gR[n])) for n in names)
            e_p = max(CR.row_error(_rows(n, gP[n]), _rows(n, gR[n])) for n in names)
            _show("C", name + " " + tag, group, e_f, e_p, bounds[group])
            _check(bad, tag + " " + group, e_f, e_p, bounds[group])
        for l in range(3):
            rows = g["l%d.pred_logits" % l][ignored[l].cuda()]
            assert (rows.view(torch.int32) == 0).all(), (tag, l)
    assert not bad, "(group, e_F, e_P) beyond the bound: %s" % bad


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "label_weight"])
def test_fused_criterion_with_boxes_that_flag_nothing_equals_the_key_absent_run_bit_for_bit(weighted):
    sizes, Q, train, seed, _ = _LAYOUTS["mixed_b4"]
    outputs, targets = CR.make_layout_case(seed, sizes, Q)
    weights = LW.draw_weights(seed + 1000, sum(sizes)) if weighted else None
    crit = _criterion(train)
    v0, t0, g0, n0 = _evaluate(crit, outputs, targets, weights, None, True)
    far = (np.array([[[0.0, 0.0, 1.0, 2.0 ** -12], [1.5, 1.5, 2.0, 2.0]]] * 4, np.float32), np.ones((4, 2), bool))
    assert not IR.flags(CR.stack_layers(outputs)["pred_boxes"].detach().numpy(), far[0], far[1], IOA)[0].any()
    v1, t1, g1, n1 = _evaluate(crit, outputs, targets, weights, far, True)
    assert _FOCAL_NODES & n0 and _IGNORE_NODE not in n0 and _IGNORE_NODE in n1 and not _FOCAL_NODES & n1
    assert crit.ignore_report() == ([0, 0, 0], 4 * Q)
    assert set(v0) == set(v1) and len(v0) > 20
    for k in v0:
        assert torch.equal(v0[k], v1[k]), k
    assert torch.equal(t0, t1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# =================================================================================================== the Trainer
SEEDS = [3, 7, 11]


def _give_ignore_boxes(rig):
    """two ignore boxes in the first image of every batch of the rig's loader, none in the second"""
    for batch in rig.loader.batches:
        boxes, mask = torch.zeros(2, 50, 4), torch.zeros(2, 50, dtype=torch.bool)
        boxes[0, 0], boxes[0, 1] = torch.tensor([0.0, 0.0, 0.5, 1.0]), torch.tensor([0.5, 0.5, 1.0, 1.0])
        mask[0, :2] = True
        batch[2]["ignore_boxes"], batch[2]["ignore_mask"] = boxes, mask


def _steps(rig, steps, first=0):
    from monosowa_amd.helpers.trainer_helper import stage_batch
    out = []
    for s in range(first, first + steps):
        rig.k = s
        total, ld = rig.trainer.train_step(*stage_batch(rig.loader.batches[s], rig.trainer.device))
        out.append(total.detach().clone())
    return out


def _sync_warnings(rig, steps, first):
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            totals = _steps(rig, steps, first=first)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    return [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()], totals


def test_steps_with_ignore_boxes_do_not_synchronise_and_train_differently(shared):
    plain = _Rig(shared, SEEDS)
    _steps(plain, 1)
    torch.cuda.synchronize()
    plain_syncs, _ = _sync_warnings(plain, 2, 1)
    rig = _Rig(shared, SEEDS)
    _give_ignore_boxes(rig)
    _steps(rig, 1)                                         # plans, tables and kernel selection belong to the first step
    torch.cuda.synchronize()
    syncs, totals = _sync_warnings(rig, 2, 1)
    assert len(syncs) == len(plain_syncs) == 0, (syncs, plain_syncs)
    assert all(torch.isfinite(t) for t in totals)
    ignored, cells = rig.crit.ignore_report()              # (reads the device: after the counted steps)
    assert len(ignored) == 3 and min(ignored) > 0 and max(ignored) < cells
    a, b = plain.state(), rig.state()
    assert set(a) == set(b)
    differ = [k for k in a if k.startswith("param.") and "class_embed" in k and not torch.equal(a[k], b[k])]
    assert differ
