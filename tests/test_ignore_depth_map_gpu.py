"""``model.ignore_depth_map`` on the GPU: the four ignore entry points of csrc/ddn_loss.hip, the criterion's routes that run them, a train
step of the shipped architecture with the key on and off, and the evaluation's report under written DontCare detections.

F is the new kernels (``pointwise.ddn_loss`` with ``ignore=``, or the whole ``SetCriterion`` with every switch of tests/fused_switches.py
shipped), P the plain float32 formulation on the GPU (tests/ignore_depth_reference.py in float32; for the whole criterion: every switch
plain), R tests/ignore_depth_reference.py in float64.

Metrics: those of tests/test_label_weights_gpu.py, restated in the helper -- |x - x_R| / max(|x_R|, tiny) for the loss value,
``row_error`` for the gradient (a row: one pixel's 81 bins).

Bounds: 4 x the worst e_P over every case of the section on the MI355X, rounded up to one significant digit; F and P must both meet it.
The measured worst e_F / e_P stand beside each constant.

Exact properties (no tolerance): the painted bins, the foreground and the ignored mask; ignored rows all +0.0, every other row the
sibling's bytes; blocks without an ignored pixel the sibling's partial; ``ign_count``; placement independence; the error codes."""
import re
import warnings

import numpy as np
import pytest
import torch

import criterion_reference as CR
import ignore_depth_reference as ID
import label_weights_reference as LW
from fused_switches import fused_switches
from test_accumulation_gpu import RES, _Rig, dev, shared      # noqa: F401  (fixtures)
from test_criterion_kernels_gpu import _criterion, _node_names
from test_ignore_depth_map_cpu import dontcare_files
from test_ignore_regions_cpu import kitti_root      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
CONSTS = (0.25, 2.0, 13.0, 1.0, 1e-3, 60.0)

# Section A (the kernels alone): worst e_F / worst e_P over the 24 cases, and 4 x e_P before rounding
A_MAP_VALUE = 4e-7     # 1.5e-7 (24x80, M 50, weighted) / 8.1e-8 (5x7, M 1), 3.3e-7: the depth-map loss with ignored pixels
A_MAP_LOGITS = 4e-6    # 1.1e-6 / 7.5e-7 (both 24x80, M 1), 3.0e-6
# Section C (the whole criterion: the fused tail, the matched kernels alone, with and without label weights)
C_MAP_VALUE = 3e-7     # 2.7e-8 (plain) / 5.3e-8 (weighted), 2.1e-7: loss_depth_map of the whole criterion
C_MAP_LOGITS = 2e-6    # 2.8e-7 (weighted) / 2.6e-7 (both), 1.0e-6

_CASE_IDS = [(H, W, M) for H, W in ID.SIZES for M in ID.MS]


def _show(section, case, group, e_f, e_p, bound):
    print("\nMEASURED %s %-34s %-14s e_F %.3e  e_P %.3e  bound %.0e" % (section, case, group, e_f, e_p, bound))


def _rows(x):
    return x.permute(0, 2, 3, 1)


# =================================================================================================== A: the kernels against float64
_REF = {}


def _run(fn, case, dtype, weighted, layout="nchw", logits=None, go=1.75):
    lg = (case["logits"] if logits is None else logits).cuda().to(dtype)
    if layout == "channels_last":
        lg = lg.contiguous(memory_format=torch.channels_last)
    lg.requires_grad_(True)
    out, maps = fn(lg, case["boxes"].cuda().to(dtype), case["depth"].cuda().to(dtype), case["valid"].cuda(),
                   case["weight"].cuda().to(dtype) if weighted else None, case["ign_boxes"].cuda(), case["ign_valid"].cuda())
    (grad,) = torch.autograd.grad(out * go, [lg])
    return out.detach(), grad, maps


def _F(lg, bx, dp, vl, wt, gb, gv):
    from monosowa_amd.pointwise import ddn_loss, ddn_loss_supported
    assert ddn_loss_supported(lg, bx, dp, vl, (gb, gv))
    loss, count = ddn_loss(lg, bx, dp, vl, *CONSTS[:4], weight=wt, ignore=(gb, gv), return_count=True)
    return loss, count


def _reference(H, W, M, weighted):
    """R (float64) and P (float32) of a case, once"""
    key = (H, W, M, weighted)
    if key not in _REF:
        case = ID.case(H, W, M)
        _REF[key] = (_run(ID.depth_map_loss, case, torch.float64, weighted), _run(ID.depth_map_loss, case, torch.float32, weighted))
    return _REF[key]


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "label_weight"])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("H,W,M", _CASE_IDS)
def test_ignore_kernels_equal_float64(H, W, M, layout, weighted):
    case = ID.case(H, W, M)
    (vR, gR, (bins, fg, wmap, ign)), (vP, gP, (bins32, fg32, w32, ign32)) = _reference(H, W, M, weighted)
    assert torch.equal(bins32, bins) and torch.equal(fg32, fg) and torch.equal(ign32, ign) and torch.equal(ign.cpu(), case["ignored"])
    if weighted:
        assert torch.equal(w32.double(), wmap)
    vF, gF, count = _run(_F, case, torch.float32, weighted, layout)
    assert gF.stride() == ((81 * H * W, 1, 81 * W, 81) if layout == "channels_last" else (81 * H * W, H * W, W, 1))
    assert torch.isfinite(vF) and torch.isfinite(gF).all()
    assert count.dtype == torch.int32 and torch.equal(count.cpu().long(), ID.block_counts(case["ignored"]))
    label = "%dx%d_M%d_%s_%s" % (H, W, M, layout, "w" if weighted else "p")
    bad = []
    e_f, e_p = ID.rel(vF, vR), ID.rel(vP, vR)
    _show("A", label, "map value", e_f, e_p, A_MAP_VALUE)
    if max(e_f, e_p) > A_MAP_VALUE:
        bad.append(("map value", e_f, e_p))
    g_f, g_p = ID.row_error(_rows(gF), _rows(gR)), ID.row_error(_rows(gP), _rows(gR))
    _show("A", label, "map logits", g_f, g_p, A_MAP_LOGITS)
    if max(g_f, g_p) > A_MAP_LOGITS:
        bad.append(("map logits", g_f, g_p))
    # ignored rows: 81 bins of +0.0; every other row (but those decided by a label of weight 0) carries a gradient
    g = _rows(gF)
    assert int(ign.sum()) > 0 and (g[ign].view(torch.int32) == 0).all()
    silent = (fg & (wmap == 0)) if weighted else torch.zeros_like(ign)
    assert (g[~ign & ~silent].abs().sum(-1) > 0).all() and (g[silent] == 0).all()
    assert not bad, "(group, e_F, e_P) beyond the bound: %s" % bad


# =================================================================================================== A: exact properties
def _launch(lib, which, weighted, ignore, t, outs, dims=None, M=None, N=None, null=None):
    """one call of mono_ddn_loss[_weighted][_ignore]_{fwd,bwd}_f32 on the tensors ``t``; ``null``: the name of a pointer passed as NULL"""
    lg = t["logits"]
    B, C, H, W = lg.shape if dims is None else dims
    names = ["logits", "boxes", "depth", "valid"] + (["weight"] if weighted else []) + (["ign_boxes", "ign_valid"] if ignore else [])
    ptrs = [None if n == null else t[n].data_ptr() for n in names] + [None if null == "out%d" % i else o.data_ptr() for i, o in enumerate(outs)]
    fn = getattr(lib, "mono_ddn_loss_%s%s%s_f32" % ("weighted_" if weighted else "", "ignore_" if ignore else "", which))
    ints = [B, C, H, W, t["boxes"].shape[1] if N is None else N] + ([t["ign_boxes"].shape[1] if M is None else M] if ignore else [])
    return fn(*ptrs, *ints, lg.stride(0), lg.stride(1), lg.stride(3), *CONSTS, None)


def _device_case(case, all_invalid=False):
    t = {k: case[k].cuda().contiguous() for k in ("logits", "boxes", "depth", "valid", "weight", "ign_boxes", "ign_valid")}
    if all_invalid:
        t["ign_valid"] = torch.zeros_like(t["ign_valid"])
    return t


def _both(lib, weighted, ignore, t, blocks):
    """(partial, count or None, grad) of one forward and one backward launch into fresh sentinel-filled buffers"""
    partial = torch.full((blocks,), SENTINEL, dtype=torch.float32, device="cuda")
    count = torch.full((blocks,), 777, dtype=torch.int32, device="cuda")
    grad = torch.full_like(t["logits"], SENTINEL)
    one = torch.full((1,), 1.75, dtype=torch.float32, device="cuda")
    assert _launch(lib, "fwd", weighted, ignore, t, [partial] + ([count] if ignore else [])) == 0
    assert _launch(lib, "bwd", weighted, ignore, t, [one, grad]) == 0
    torch.cuda.synchronize()
    return partial, (count if ignore else None), grad


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "label_weight"])
@pytest.mark.parametrize("H,W,M", _CASE_IDS)
def test_ignore_entry_points_against_their_siblings_bit_for_bit(H, W, M, weighted):
    from monosowa_amd import pointwise
    lib = pointwise.load()
    case = ID.case(H, W, M)
    blocks = lib.mono_ddn_loss_blocks(3, H, W)
    assert blocks == (3 * H * W + ID.BLOCK_PIXELS - 1) // ID.BLOCK_PIXELS
    t = _device_case(case)
    p0, _, g0 = _both(lib, weighted, False, t, blocks)
    assert not (p0 == SENTINEL).any() and not (g0 == SENTINEL).any()
    # no valid ignore box: the siblings' bytes, nothing counted
    p1, c1, g1 = _both(lib, weighted, True, _device_case(case, all_invalid=True), blocks)
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32)) and torch.equal(g1.view(torch.int32), g0.view(torch.int32))
    assert (c1 == 0).all()
    # with regions
    p2, c2, g2 = _both(lib, weighted, True, t, blocks)
    ign = case["ignored"].cuda()
    want = ID.block_counts(case["ignored"])
    assert torch.equal(c2.cpu().long(), want)
    r0, r2 = _rows(g0), _rows(g2)
    assert torch.equal(r2[~ign].view(torch.int32), r0[~ign].view(torch.int32)) and (r2[ign].view(torch.int32) == 0).all()
    clean = (want == 0).cuda()
    assert clean.any() or (H, W) == (5, 7)                                    # (the generator plants such a block at 24 x 80)
    assert torch.equal(p2[clean].view(torch.int32), p0[clean].view(torch.int32))
    assert (p2[~clean] < p0[~clean]).all() and (p2 >= 0).all()
    # NaN / +-Inf logits under ignored pixels: the same bytes, finite everywhere
    poisoned = dict(t, logits=t["logits"].clone())
    where = torch.nonzero(ign)
    for i, bad in enumerate((float("nan"), float("inf"), -float("inf"))):
        b, y, x = where[(i * 7) % len(where)].tolist()
        poisoned["logits"][b, (11 * i) % 81, y, x] = bad
    b, y, x = where[-1].tolist()
    poisoned["logits"][b, :, y, x] = float("nan")
    p3, c3, g3 = _both(lib, weighted, True, poisoned, blocks)
    assert torch.isfinite(p3).all() and torch.isfinite(g3).all()
    assert torch.equal(p3.view(torch.int32), p2.view(torch.int32)) and torch.equal(g3.view(torch.int32), g2.view(torch.int32)) and torch.equal(c3, c2)


def test_two_placements_of_the_outputs_give_the_same_bytes_and_the_codes_are_the_siblings():
    from monosowa_amd import pointwise
    lib = pointwise.load()
    H, W, M = 5, 7, 3
    case = ID.case(H, W, M)
    t = _device_case(case)
    blocks = lib.mono_ddn_loss_blocks(3, H, W)
    n = t["logits"].numel()
    one = torch.full((1,), 1.75, dtype=torch.float32, device="cuda")
    fbuf = torch.full((2 * n + 4096,), SENTINEL, dtype=torch.float32, device="cuda")
    ibuf = torch.full((2048,), 777, dtype=torch.int32, device="cuda")
    got = []
    for off in (1, 1030):
        for weighted in (False, True):
            partial, count = fbuf[off:off + blocks], ibuf[off:off + blocks]
            start = 2048 + (0 if off == 1 else n + 5)
            grad = fbuf[start:start + n].view(t["logits"].shape)
            assert _launch(lib, "fwd", weighted, True, t, [partial, count]) == 0
            assert _launch(lib, "bwd", weighted, True, t, [one, grad]) == 0
            torch.cuda.synchronize()
            got.append((partial.clone(), count.clone(), grad.clone()))
            assert not (partial == SENTINEL).any() and not (count == 777).any() and not (grad == SENTINEL).any()
            partial.fill_(SENTINEL), count.fill_(777), grad.fill_(SENTINEL)
    for first, second in zip(got[:2], got[2:]):
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, second))
    torch.cuda.synchronize()
    assert (fbuf == SENTINEL).all() and (ibuf == 777).all()                    # nothing was written outside the outputs
    # return codes: the siblings' -1 for a NULL pointer and -2 for N <= 0; M <= 0 is -2 as well; nothing is written
    o = torch.full((blocks + n,), SENTINEL, dtype=torch.float32, device="cuda")
    oc = torch.full((blocks,), 777, dtype=torch.int32, device="cuda")
    og = o[blocks:].view(t["logits"].shape)
    for weighted in (False, True):
        sib = [_launch(lib, "fwd", weighted, False, t, [o], null="logits"), _launch(lib, "fwd", weighted, False, t, [o], N=0),
               _launch(lib, "bwd", weighted, False, t, [one, og], null="out1"), _launch(lib, "bwd", weighted, False, t, [one, og], N=0)]
        new = [_launch(lib, "fwd", weighted, True, t, [o, oc], null="logits"), _launch(lib, "fwd", weighted, True, t, [o, oc], N=0),
               _launch(lib, "bwd", weighted, True, t, [one, og], null="out1"), _launch(lib, "bwd", weighted, True, t, [one, og], N=0)]
        assert new == sib == [-1, -2, -1, -2]
        for which, outs in (("fwd", [o, oc]), ("bwd", [one, og])):
            for null in ("ign_boxes", "ign_valid", "boxes", "valid", "out0") + (("weight",) if weighted else ()) + (("out1",) if which == "fwd" else ()):
                assert _launch(lib, which, weighted, True, t, outs, null=null) == -1, (which, null)
            assert _launch(lib, which, weighted, True, t, outs, M=0) == -2 and _launch(lib, which, weighted, True, t, outs, M=-1) == -2
    torch.cuda.synchronize()
    assert (o == SENTINEL).all() and (oc == 777).all()


# =================================================================================================== C: the whole criterion
_NEW_NODES = {"_DDNLossIgnoreBackward", "_DDNLossWeightedIgnoreBackward"}
_OLD_NODES = {"_DDNLossBackward", "_DDNLossWeightedBackward"}
_SIZES, _Q, _SEED = [0, 5, 1, 3], 50, 510


def _ignore_boxes(B, seed, empty_image=0, M=6, valid=3):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(0.05, 0.6, (B, M, 2))
    boxes = np.concatenate([lo, lo + rng.uniform(0.15, 0.35, (B, M, 2))], -1).astype(np.float32)
    mask = np.zeros((B, M), bool)
    mask[:, :valid] = True
    mask[empty_image] = False
    return boxes, mask                                  # (the invalid slots keep their boxes: they must have no effect)


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
    return values, grads, nodes


def _map_reference(crit, outputs, targets, weights, ignore):
    """loss_depth_map and its gradient (times the criterion's weight) in float64 by the restatement"""
    w = weights if weights is not None else torch.ones(sum(len(t["labels"]) for t in targets))
    tg = LW.with_weights(targets, w)
    pb, pd, pv, pw = LW.padded_depth_map_inputs(tg, crit.depth_map_size, torch.float64)
    mw, mh = crit.depth_map_size
    px = torch.from_numpy(np.asarray(ignore[0], np.float32) * np.array([mw, mh, mw, mh], np.float32))
    lg = outputs["pred_depth_map_logits"].double().requires_grad_(True)
    loss, (_, fg, _, ign) = ID.depth_map_loss(lg, pb, pd, pv, pw, px, torch.from_numpy(ignore[1]))
    (grad,) = torch.autograd.grad(loss * float(crit.weight_dict["loss_depth_map"]), [lg])
    return loss.detach(), grad, ign


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "label_weight"])
def test_criterion_routes_with_the_key_on_equal_float64_and_move_nothing_else(weighted):
    """F: the fused tail; F2: FUSED_FOCAL off -- the matched kernels alone; P: every switch plain"""
    outputs, targets = CR.make_layout_case(_SEED, _SIZES, _Q)
    assert outputs["pred_depth_map_logits"].shape == (4, 81, 24, 80)
    weights = LW.draw_weights(_SEED + 1000, sum(_SIZES)) if weighted else None
    ignore = _ignore_boxes(4, _SEED + 2000)
    crit = _criterion(False)                                    # 50 queries: the eval-mode criterion (one group)
    assert crit.ignore_depth_map is False and tuple(crit.depth_map_size) == (80, 24)
    vR, gR, ign = _map_reference(crit, outputs, targets, weights, ignore)
    n_ign = int(ign.sum())
    assert n_ign > 100 and not ign[0].any()
    routes = {"F": dict(on=True), "F2": dict(on=True, focal=False), "P": dict(on=False)}
    got, off = {}, {}
    for tag, kw in routes.items():
        crit.ignore_depth_map = False
        off[tag] = _evaluate(crit, outputs, targets, weights, ignore, **kw)
        assert crit.ignore_depth_report() is None
        crit.ignore_depth_map = True
        got[tag] = _evaluate(crit, outputs, targets, weights, ignore, **kw)
        assert crit.ignore_depth_report() == (n_ign, 4 * 24 * 80), tag
        assert len(crit.ignore_report()) == 2
    crit.ignore_depth_map = False
    for tag in ("F", "F2"):
        assert got[tag][2] & _NEW_NODES == {"_DDNLossWeightedIgnoreBackward" if weighted else "_DDNLossIgnoreBackward"} and not got[tag][2] & _OLD_NODES
        assert off[tag][2] & _OLD_NODES == {"_DDNLossWeightedBackward" if weighted else "_DDNLossBackward"} and not off[tag][2] & _NEW_NODES
    assert not got["P"][2] & (_NEW_NODES | _OLD_NODES)
    bad = []
    vP, gP, _ = got["P"]
    for tag in ("F", "F2"):
        v, g, _ = got[tag]
        e_f, e_p = ID.rel(v["loss_depth_map"], vR), ID.rel(vP["loss_depth_map"], vR)
        _show("C", tag + (" weighted" if weighted else " plain"), "map value", e_f, e_p, C_MAP_VALUE)
        if max(e_f, e_p) > C_MAP_VALUE:
            bad.append((tag, "map value", e_f, e_p))
        g_f = ID.row_error(_rows(g["depth_map_logits"]), _rows(gR))
        g_p = ID.row_error(_rows(gP["depth_map_logits"]), _rows(gR))
        _show("C", tag + (" weighted" if weighted else " plain"), "map logits", g_f, g_p, C_MAP_LOGITS)
        if max(g_f, g_p) > C_MAP_LOGITS:
            bad.append((tag, "map logits", g_f, g_p))
    for tag in routes:                                          # every other key and gradient: the key-off run's, bit for bit
        v, g, _ = got[tag]
        v0, g0, _ = off[tag]
        assert list(v) == list(v0) and len(v) > 20
        for k in v0:
            assert torch.equal(v[k], v0[k]) != (k == "loss_depth_map"), (tag, k)
        for n in g0:
            assert torch.equal(g[n], g0[n]) != (n == "depth_map_logits"), (tag, n)
        rows = _rows(g["depth_map_logits"])[ign.cuda()]
        assert (rows.view(torch.int32) == 0).all(), tag
        if tag != "P":
            assert torch.equal(_rows(g["depth_map_logits"])[~ign.cuda()], _rows(g0["depth_map_logits"])[~ign.cuda()]), tag
    assert not bad, "(route, group, e_F, e_P) beyond the bound: %s" % bad


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


def _ddn_kernels(rig, step):
    """(BW, IG) template arguments of every DDN loss kernel a profiled step launches"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        _steps(rig, 1, first=step)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return [m.groups() for m in (re.search(r"ddn_loss_(fwd|bwd)_kernel<(\w+), ?(\w+)>", n) for n in names) if m]


def test_a_train_step_with_the_key_on_adds_no_wait_and_with_it_off_no_launch(shared, monkeypatch):
    calls = [0]
    sync = torch.cuda.synchronize
    crit = shared[2]
    assert crit.ignore_depth_map is False
    try:
        plain = _Rig(shared, SEEDS)
        _give_ignore_boxes(plain)
        _steps(plain, 1)
        torch.cuda.synchronize()
        plain_syncs, _ = _sync_warnings(plain, 1, 1)
        assert crit.ignore_depth_report() is None
        launched = _ddn_kernels(plain, 2)
        assert len(launched) == 2 and {k[0] for k in launched} == {"fwd", "bwd"} and all(k[2] in ("false", "0") for k in launched), launched
        rig = _Rig(shared, SEEDS)
        _give_ignore_boxes(rig)
        crit.ignore_depth_map = True
        _steps(rig, 1)                                         # plans, tables and kernel selection belong to the first step
        torch.cuda.synchronize()
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.__setitem__(0, calls[0] + 1), sync(*a, **k))[1])
        syncs, totals = _sync_warnings(rig, 1, 1)
        monkeypatch.undo()
        assert calls[0] == 0 and len(syncs) == len(plain_syncs) == 0, (calls, syncs, plain_syncs)
        assert all(torch.isfinite(t) for t in totals)
        n, N = crit.ignore_depth_report()                      # (reads the device: after the counted step)
        assert N == 2 * (RES[0] // 16) * (RES[1] // 16) and 0 < n <= N // 2
        launched = _ddn_kernels(rig, 2)
        assert len(launched) == 2 and all(k[2] in ("true", "1") for k in launched), launched
        state = rig.state()
        assert all(torch.isfinite(v).all() for k, v in state.items() if k.startswith("param."))
        a = plain.state()
        assert [k for k in a if k.startswith("param.") and "depth_predictor" in k and not torch.equal(a[k], state[k])]
    finally:
        crit.ignore_depth_map = False


# =================================================================================================== tester.dontcare_below
def test_the_evaluation_report_is_the_same_with_and_without_the_dontcare_detections(kitti_root, tmp_path):
    from monosowa_amd import kitti_eval as kitti
    with_dc, without, text, label_dir = dontcare_files(kitti_root, tmp_path)
    gt = kitti.get_label_annos(str(label_dir), [3])
    for cls in (0, 1):
        reports = [kitti.get_official_eval_result(gt, kitti.get_label_annos(str(d), [3]), cls)[0] for d in (with_dc, without)]
        assert reports[0] == reports[1] and "AP" in reports[0]
