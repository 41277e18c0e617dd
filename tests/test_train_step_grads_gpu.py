"""The gradient that training uses -- d(weighted loss) / d(every parameter) -- with the fused pieces wired together, against
float64.

Backbone: the trainable ResNet stages and the input projections in train mode (affine-in-kernel, forked-ReLU and
epilogue-GEMM nodes, pre-bias GroupNorm) against the float64 CPU evaluation of tests/backbone_reference.py, made
differentiable in the layer2-4 convolution weights and the projections' convolution / GroupNorm parameters.

Detector: the shipped architecture (configs/monodetr.yaml: 3 + 3 layers, 50 x 11 queries, aux loss, box refinement,
dropout 0) behind a backbone body that returns fixed C3 / C4 / C5 leaves, through ``forward_fast`` and ``weighted_total``,
evaluated three times from identical weights, features and targets:
  F  float32, every switch at its shipped value (the product),
  P  float32, every switch of tests/fused_switches.py at its plain-PyTorch value,
  R  float64, every switch plain (the f64 MSDA kernels are pinned to the C oracle by tests/test_msda_gpu.py),
  D  F's switches under torch.use_deterministic_algorithms(True): the kernels a deterministic training run selects.
The matching is discrete: F's [3, NL, K] indices are recorded and handed to P, R and D.  F and D are compared with R per tensor
by ||g - g_ref|| / ||g_ref||; P must meet the same bound, so no bound is tighter than honest float32 arithmetic.  D is evaluated
twice: every gradient has the same bits both times."""
import collections
import contextlib
import copy
import os
import time

import pytest
import torch
import yaml

from backbone_reference import _model, _reference
from detector_reference import _Body, _FrozenMatcher, trained_like_msda
from fused_switches import fused_switches
from test_eval_forward_gpu import _patched

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Per-tensor bounds on ||g - g_ref|| / ||g_ref||, one per group.  Measured on the MI355X (worst tensor of the group over
# every case of this module): e_F = product vs float64, e_P = plain float32 vs float64, e_D = product under the deterministic flag
# vs float64 (D runs MIOpen under cudnn.deterministic, whose other convolution algorithms move the few pixel-border steps).
# The float32 runs step across pixel borders that float64 does not (d(location) of MSDA jumps there) and through
# convolution algorithms of the library; both show in e_P as much as in e_F.  Measured worst tensor, e_F / e_P; e_D behind it:
BOUND_BACKBONE = 1e-2      # 2.2e-3 / 2.7e-3 (ResNet-101 96 x 320, ResNet-50 136 x 520: the library's 3x3 convolutions); e_D 1.9e-3
BOUND_INPUT_PROJ = 3e-3    # 7.0e-4 / 7.0e-4 (input_proj.2, 640 x 192); e_D 3.3e-4 (feature C3, batch 13)
BOUND_ENCODER = 1.5e-2     # 4.2e-3 / 4.2e-3 (layer 0 sampling_offsets, 640 x 192; level_embed 2.1e-3 / 2.1e-3); e_D 1.1e-3 (batch 13)
BOUND_DECODER = 2.5e-2     # 8.5e-3 / 8.5e-3 (reference_points.bias, 640 x 192 at batch 13); e_D 8.5e-3 (the same tensor)
BOUND_DEPTH = 2e-3         # 7.8e-4 / 7.8e-4 (downsample.0, 640 x 192 at batch 13); e_D 8.6e-5 (the same tensor)
BOUND_HEADS = 6e-3         # 1.7e-3 / 1.1e-3 (dim_embed.0 / bbox_embed.2 first layers, 640 x 192); e_D 7.1e-4 (bbox_embed.1, batch 13)
BOUND_LOSS = 2e-6          # 3.1e-7 / 3.5e-7: relative error of each differentiable loss term; e_D 3.1e-7


def _rel_norm(g, ref):
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    return float((g - ref).norm() / ref.norm().clamp_min(1e-300))


def _node_names(roots):
    """type names of every autograd node reachable from ``roots``"""
    seen, kept, stack, names = set(), [], [t.grad_fn for t in roots if t.grad_fn is not None], set()
    while stack:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen.add(id(fn))
        kept.append(fn)                     # alive until the walk ends: a freed wrapper's id could be handed to another node
        names.add(type(fn).__name__)
        stack.extend(nxt for nxt, _ in fn.next_functions)
    return names


@contextlib.contextmanager
def _mode(det):
    """torch's deterministic flag (and MIOpen's switch, as a deterministic training run sets both) for one evaluation"""
    was, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    miopen = torch.backends.cudnn.deterministic
    torch.use_deterministic_algorithms(det)
    torch.backends.cudnn.deterministic = det or miopen
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn_only)
        torch.backends.cudnn.deterministic = miopen


@contextlib.contextmanager
def _msda_backward_calls():
    """counts the fused operator's two backward entry points: re-evaluated prologue / saved prologue"""
    from monosowa_amd import MultiScaleDeformableAttention as MSDA
    calls = collections.Counter()

    def wrap(name):
        fn = getattr(MSDA, name)

        def spy(*args, **kwargs):
            calls[name] += 1
            return fn(*args, **kwargs)
        return spy
    with _patched([(MSDA, n, wrap(n)) for n in ("ms_deform_attn_fused_backward_merged", "ms_deform_attn_fused_backward_merged_saved")]):
        yield calls


def _report(title, errs):
    print("\n%s" % title)
    for name, e in sorted(errs.items(), key=lambda kv: -kv[1])[:6]:
        print("  %.3e  %s" % (e, name))


# --------------------------------------------------------------------------------------------------------------- backbone
_TRAINABLE = ("conv1.weight", "conv2.weight", "conv3.weight", "downsample.0.weight")


def _backbone_leaf(key):
    """a parameter the float64 reference differentiates in: layer2-4 convolutions, every input-projection parameter"""
    if key.startswith("input_proj."):
        return True
    parts = key.split(".")
    return key.startswith("backbone.0.body.layer") and parts[3] in ("layer2", "layer3", "layer4") and \
        ".".join(parts[5:]) in _TRAINABLE


@pytest.mark.parametrize("name,hw", [("resnet50", (96, 320)), ("resnet101", (96, 320)), ("resnet50", (136, 520))],
                         ids=["resnet50_96x320", "resnet101_96x320", "resnet50_136x520_odd"])
def test_backbone_and_input_projection_gradients_equal_float64(name, hw):
    """136 x 520 (1408 x 376 scaled down): odd extents at every stride that leaves the body (17 x 65, 9 x 33, 5 x 17, 3 x 9)."""
    H, W = hw
    model, sd = _model(name)
    model.train()
    gen = torch.Generator().manual_seed(3)
    images = torch.randn(2, 3, H, W, generator=gen)
    x = images.cuda().contiguous(memory_format=torch.channels_last)
    cot = None

    def run(on, det=False):
        nonlocal cot
        model.zero_grad(set_to_none=True)
        with fused_switches(on), _mode(det):
            if det:
                from monosowa_amd import gemm_lt, pointwise
                assert pointwise.DETERMINISTIC.sync() is True and gemm_lt.DETERMINISTIC.sync() is True
            features, pos = model.backbone(x)
            srcs, _, _ = model.project_features(features, pos)
            nodes = _node_names(srcs)
            if cot is None:
                cot = [torch.randn(s.shape, generator=gen, dtype=torch.float64) for s in srcs]
            torch.autograd.backward(srcs, [c.float().cuda().contiguous(memory_format=torch.channels_last) for c in cot])
        return {n: p.grad for n, p in model.named_parameters() if n.startswith(("backbone.", "input_proj."))}, nodes

    plain, plain_nodes = run(False)
    got, nodes = run(True)
    # D: the pre-bias GroupNorm and the epilogue GEMMs under the flag, MIOpen under cudnn.deterministic (the two ResNet-50 cases)
    got_d, nodes_d = run(True, det=True) if name == "resnet50" else (None, None)

    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if _backbone_leaf(k)}
    _, want = _reference(dict(sd, **leaves), name, images.double())
    torch.autograd.backward(want, cot)

    assert {n for n, g in plain.items() if g is not None} == set(leaves)
    assert {n for n, g in got.items() if g is not None} == set(leaves), sorted({n for n, g in got.items() if g is not None} ^ set(leaves))
    body = model.backbone[0].body
    assert body.conv1.weight.grad is None and all(p.grad is None for p in body.layer1.parameters())
    errs = {n: _rel_norm(got[n], leaf.grad) for n, leaf in leaves.items()}
    errs_p = {n: _rel_norm(plain[n], leaf.grad) for n, leaf in leaves.items()}
    _report("backbone %s %dx%d F" % (name, H, W), errs)
    _report("backbone %s %dx%d P" % (name, H, W), errs_p)
    print("nodes:", sorted(nodes))
    print("plain nodes:", sorted(plain_nodes))
    for n, e in errs.items():
        bound = BOUND_INPUT_PROJ if n.startswith("input_proj.") else BOUND_BACKBONE
        assert e <= bound and errs_p[n] <= bound, (n, e, errs_p[n], bound)
    # the trainable stages ran the fused nodes under test, and the projections the NHWC GroupNorm with the bias inside
    for fused in ("_AffineReluBackward", "_Conv1x1BnActBackward", "_GroupNormNHWCBackward"):
        assert fused in nodes, (fused, sorted(nodes))
    assert "_BiasActForkBackward" in plain_nodes and "_Conv1x1BnActBackward" not in plain_nodes, sorted(plain_nodes)
    if got_d is not None:
        assert {n for n, g in got_d.items() if g is not None} == set(leaves)
        assert {"_AffineReluBackward", "_Conv1x1BnActBackward", "_GroupNormNHWCBackward"} <= nodes_d, sorted(nodes_d)
        errs_d = {n: _rel_norm(got_d[n], leaf.grad) for n, leaf in leaves.items()}
        _report("backbone %s %dx%d D" % (name, H, W), errs_d)
        for n, e in errs_d.items():
            bound = BOUND_INPUT_PROJ if n.startswith("input_proj.") else BOUND_BACKBONE
            assert e <= bound, (n, e, bound)


# --------------------------------------------------------------------------------------------------------------- detector
LOSS_KEYS = [k + s for s in ("", "_0", "_1") for k in ("loss_ce", "loss_center", "loss_bbox", "loss_giou", "loss_depth", "loss_dim",
                                                       "loss_angle")] + ["loss_depth_map"]

# (W, H) of the image, batch: config 2 at 640 x 192, and 520 x 136 whose levels (65 x 17, 33 x 9, 17 x 5, 9 x 3) are odd
# 13 x 2,550 tokens: past the 32,768 from which the encoder layers run as the fused block nodes (encoder_block.supported)
_DET_CASES = {"config2_640x192_b2": ((640, 192), 2), "odd_520x136_b2": ((520, 136), 2), "config2_640x192_b13_blocks": ((640, 192), 13)}


def _group(name):
    if name.startswith(("input_proj.", "feature.")):
        return "input_proj", BOUND_INPUT_PROJ
    if name.startswith("depth_predictor."):
        return "depth predictor", BOUND_DEPTH
    if any(h in name for h in ("class_embed.", "bbox_embed.", "dim_embed", "angle_embed.", "depth_embed.")):
        return "heads", BOUND_HEADS
    if name.startswith(("depthaware_transformer.encoder.", "depthaware_transformer.level_embed")):
        return "encoder", BOUND_ENCODER
    if name.startswith(("depthaware_transformer.", "query_embed")):
        return "decoder", BOUND_DECODER
    raise AssertionError("parameter %s belongs to no group" % name)


@pytest.mark.parametrize("case", list(_DET_CASES))
def test_every_parameter_gradient_of_a_train_step_equals_float64(case):
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import make_batch, prepare_targets
    (W, H), B = _DET_CASES[case]
    levels = [(-(-H // s), -(-W // s)) for s in (8, 16, 32)]
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    mcfg = dict(cfg["model"], device="cuda", dropout=0.0, pretrained=False, depth_map_size=(levels[1][1], levels[1][0]))
    torch.manual_seed(7)
    model0, crit = build_model(mcfg)
    assert model0.aux_loss and model0.with_box_refine and model0.num_queries == 50 and model0.group_num == 11
    assert len(model0.depthaware_transformer.encoder.layers) == 3 and model0.depthaware_transformer.decoder.num_layers == 3
    for m in model0.modules():                      # the depth predictor hard-codes dropout 0.1 (depth_predictor.py:109)
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    gen = torch.Generator().manual_seed(23)
    trained_like_msda(model0, gen)
    model0.backbone[0].body = _Body()
    crit.matcher = _FrozenMatcher(crit.matcher)
    crit = crit.cuda().train()
    feats = [torch.randn(B, c, h, w, generator=gen, dtype=torch.float64) for c, (h, w) in zip((512, 1024, 2048), levels)]
    _, calibs, targets, _ = make_batch(B, "cuda", seed=5, resolution=(W, H))
    images = torch.zeros(B, 3, H, W, device="cuda")

    def run(on, dtype, det=False):
        with fused_switches(on), _mode(det), _msda_backward_calls() as calls:
            if det:
                from monosowa_amd import _lib, gemm_lt, pointwise
                assert _lib.MSDA_DETERMINISTIC.sync() is True and pointwise.DETERMINISTIC.sync() is True and gemm_lt.DETERMINISTIC.sync() is True
            model = to_mi355x_layout(copy.deepcopy(model0).to(device="cuda", dtype=dtype)).train()
            leaves = [f.to(device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True) for f in feats]
            model.backbone[0].body.feats = leaves
            c = crit.to(dtype)
            tg = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in targets.items()}
            tl = prepare_targets(tg, B)
            losses = c(model(images.to(dtype), calibs.to(dtype), tl, targets["img_size"]), tl)
            total = weighted_total(losses, c.weight_dict)
            nodes = _node_names([total])
            total.backward()
            grads = {n: p.grad for n, p in model.named_parameters() if p.requires_grad}
            grads.update({"feature.C%d" % (i + 3): f.grad for i, f in enumerate(leaves)})
            terms = {k: float(losses[k].detach()) for k in LOSS_KEYS}
            c.to(torch.float32)
            return total.item(), terms, grads, nodes, dict(calls)

    tF, lF, gF, nF, cF = run(True, torch.float32)
    tP, lP, gP, nP, _ = run(False, torch.float32)
    tR, lR, gR, nR, _ = run(False, torch.float64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tD, lD, gD, nD, cD = run(True, torch.float32, det=True)
    torch.cuda.synchronize()
    seconds_d = time.perf_counter() - t0
    tD2, lD2, gD2, _, _ = run(True, torch.float32, det=True)
    print("\n%s: total F %.9g P %.9g D %.9g R %.12g" % (case, tF, tP, tD, tR))
    print("D: %.2f s for model copy, forward and backward; MSDA backward calls F %s D %s" % (seconds_d, cF, cD))
    print("F nodes:", sorted(nF))
    print("P nodes:", sorted(nP))
    # D: the fused operator's backward re-evaluated its prologue all six times (3 encoder layers, 3 decoder layers): the
    # saved-prologue backward runs the row-tile scatter, which has no deterministic variant
    assert cD == {"ms_deform_attn_fused_backward_merged": 6}, cD
    assert sum(cF.values()) == 6, cF
    # D twice: the same bits (the first repeatability check at the odd pyramid and with the encoder as block nodes)
    assert tD == tD2 and lD == lD2 and set(gD) == set(gD2)
    for n, g in gD.items():
        assert (g is None and gD2[n] is None) or torch.equal(g, gD2[n]), "D: %s differs between two evaluations" % n

    loss_err = {k: abs(lF[k] - lR[k]) / max(abs(lR[k]), 1e-30) for k in LOSS_KEYS}
    loss_err_p = {k: abs(lP[k] - lR[k]) / max(abs(lR[k]), 1e-30) for k in LOSS_KEYS}
    loss_err_d = {k: abs(lD[k] - lR[k]) / max(abs(lR[k]), 1e-30) for k in LOSS_KEYS}
    _report("loss terms F", loss_err)
    _report("loss terms P", loss_err_p)
    _report("loss terms D", loss_err_d)

    assert set(gF) == set(gR) == set(gP) == set(gD)
    assert {n for n, g in gD.items() if g is None} == {n for n, g in gR.items() if g is None}
    none_f = {n for n, g in gF.items() if g is None}
    assert none_f == {n for n, g in gR.items() if g is None}, sorted(none_f ^ {n for n, g in gR.items() if g is None})
    assert none_f == {n for n, g in gP.items() if g is None}, sorted(none_f ^ {n for n, g in gP.items() if g is None})
    assert none_f == set(model0.unused_parameter_names()), sorted(none_f ^ set(model0.unused_parameter_names()))
    # the key projections' biases have a zero gradient in exact arithmetic (the softmax is invariant to a shift along the keys):
    # their error is measured against the norm of the same layer's key-weight gradient
    scale = lambda n: gR[n.replace("_proj.bias", "_proj.weight")] if n.endswith(("sa_kcontent_proj.bias", "sa_kpos_proj.bias")) else gR[n]
    err = lambda g, n: float((g.double() - gR[n].double()).norm() / scale(n).double().norm().clamp_min(1e-300))
    eF = {n: err(gF[n], n) for n in gF if gR[n] is not None}
    eP = {n: err(gP[n], n) for n in gP if gR[n] is not None}
    eD = {n: err(gD[n], n) for n in gD if gR[n] is not None}
    by_group = {}
    for n in eF:
        by_group.setdefault(_group(n), []).append(n)
    for (grp, bound), names in sorted(by_group.items()):
        _report("%s F (bound %.1e)" % (grp, bound), {n: eF[n] for n in names})
        _report("%s P" % grp, {n: eP[n] for n in names})
        _report("%s D" % grp, {n: eD[n] for n in names})
    # F ran the fused nodes under test; P ran none of them
    fused = {"MSDeformAttnFusedMergedFunctionBackward", "_DDNLossBackward", "_DepthExpectationBackward", "_FocalClassificationBackward",
             "_HeadTailBackward", "_MatchedLossesBackward", "_MergedValueProjBackward", "_TokenLinearBackward", "_GroupNormNHWCBackward"}
    if B * sum(-(-H // s) * -(-W // s) for s in (8, 16, 32, 64)) >= 32768:
        fused |= {"_AttnBlockBackward", "_FFNBlockBackward"}
    assert fused <= nF, sorted(fused - nF)
    assert fused <= nD, sorted(fused - nD)
    # (GroupNorm has no plain path; from 32,768 tokens on, token_linear splits the weight gradient whatever FAST_LINEAR says)
    assert not (fused - {"_GroupNormNHWCBackward", "_TokenLinearBackward"}) & nP, sorted(fused & nP)
    for k in LOSS_KEYS:
        assert loss_err[k] <= BOUND_LOSS and loss_err_p[k] <= BOUND_LOSS and loss_err_d[k] <= BOUND_LOSS, (k, loss_err[k], loss_err_p[k], loss_err_d[k])
    bad = [(n, eF[n], eP[n], eD[n], b) for (_, b), names in by_group.items() for n in names if eF[n] > b or eP[n] > b or eD[n] > b]
    assert not bad, "per-tensor ||g - g_ref|| / ||g_ref|| (name, F, P, D, bound): %s" % bad[:12]
