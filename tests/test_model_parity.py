"""Parity of the host-side restatement (MSDeformAttn module, depth-aware transformer, depth predictor,
matcher, position encoding, losses) against fixtures captured from the REFERENCE's own Python modules
(oracle/gen_golden.py: module / transformer / depth / misc).  Weights are filled deterministically by
state-dict key (tests/det_weights.py), so equal key manifests + equal outputs pin both the math and
checkpoint compatibility.

CPU runs swap the MSDA autograd Function for the oracle's grid_sample port (test-only; the product
raises "Not implemented on the CPU" exactly like the reference); ``-m gpu`` runs go through the HIP
kernels.
"""
import json
import os

import numpy as np
import pytest
import torch

from det_weights import fill_deterministic, key_manifest
from oracle import msda_oracle as O

KITTI_SMALL = [(12, 16), (6, 8), (3, 4), (2, 2)]


def _load(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    return {k: (torch.from_numpy(g[k]) if g[k].dtype.kind in "fbiu" and g[k].ndim > 0 else g[k]) for k in g.files}


class _OracleMSDA:
    """Test-only stand-in for MSDeformAttnFunction on CPU tensors."""
    @staticmethod
    def apply(value, shapes, lsi, loc, w, step):
        return O.msda_core_torch(value, shapes, loc, w)


@pytest.fixture
def cpu_msda(monkeypatch):
    import monosowa_amd.ms_deform_attn_func as f
    monkeypatch.setattr(f, "MSDeformAttnFunction", _OracleMSDA)


def _lsi(shapes):
    return torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def _assert_close(a, b, rel, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    assert err <= rel, "%s: %.3e > %.1e" % (what, err, rel)


def _same_manifest(module, fixture_manifest):
    mine = json.loads(key_manifest(module))
    ref = json.loads(str(fixture_manifest))
    assert mine == ref, (sorted(set(mine) ^ set(ref))[:8])


# ------------------------------------------------------------------------------------------ module
def _module_case(g, device, dtype, rel):
    from monosowa_amd.ms_deform_attn import MSDeformAttn
    m = fill_deterministic(MSDeformAttn(256, 4, 8, 4), 101)
    _same_manifest(m, g["manifest"])
    m = m.to(device=device, dtype=dtype)
    t = lambda k: g[k].to(device=device, dtype=dtype) if g[k].dtype.is_floating_point else g[k].to(device)
    shapes = t("shapes")
    out2 = m(t("query"), t("ref2"), t("src"), shapes, _lsi(shapes), t("pad"))
    out6 = m(t("query"), t("ref6"), t("src"), shapes, _lsi(shapes), t("pad"))
    _assert_close(out2, g["out2"], rel, "2-d reference points")
    _assert_close(out6, g["out6"], rel, "6-d reference points")


def test_msdeformattn_module_cpu(golden_dir, cpu_msda):
    _module_case(_load(golden_dir, "module_msdeformattn"), "cpu", torch.float64, 1e-9)


@pytest.mark.gpu
def test_msdeformattn_module_gpu(golden_dir):
    g = _load(golden_dir, "module_msdeformattn")
    _module_case(g, "cuda", torch.float64, 1e-9)
    _module_case(g, "cuda", torch.float32, 1e-4)


def test_msdeformattn_bad_reference_dim(cpu_msda):
    from monosowa_amd.ms_deform_attn import MSDeformAttn
    m = MSDeformAttn(64, 2, 2, 2)
    shapes = torch.tensor([(2, 2), (1, 1)])
    with pytest.raises(ValueError):
        m(torch.zeros(1, 3, 64), torch.zeros(1, 3, 2, 4), torch.zeros(1, 5, 64), shapes, _lsi(shapes))


# ------------------------------------------------------------------------------------- transformer
def _build_transformer(G):
    from monosowa_amd.monodetr.depthaware_transformer import DepthAwareTransformer, MLP
    t = DepthAwareTransformer(d_model=256, nhead=8, num_encoder_layers=3, num_decoder_layers=3, dim_feedforward=256,
                              dropout=0.0, return_intermediate_dec=True, num_feature_levels=4, dec_n_points=4,
                              enc_n_points=4, two_stage=False, two_stage_num_proposals=50, group_num=G)
    t.decoder.bbox_embed = torch.nn.ModuleList([MLP(256, 256, 6, 3) for _ in range(3)])
    t.decoder.dim_embed = torch.nn.ModuleList([MLP(256, 256, 3, 2) for _ in range(3)])
    return t


def _transformer_case(g, device, rel, dtype=torch.float64, check_grad=True, grad_rel=None):
    """The fixture is a float64 run of the reference (inputs are f32-representable, results stored as
    f32).  Gradients through MSDA contain grad_loc, which jumps at pixel borders, so the gradient check
    is only meaningful in float64 (an f32 run of the reference itself is 2e-3 away from its f64 run)."""
    G = int(g["group_num"])
    t = fill_deterministic(_build_transformer(G), 202)
    _same_manifest(t, g["manifest"])
    t = t.to(device=device, dtype=dtype)
    srcs = [g["src%d" % i].to(device=device, dtype=dtype) for i in range(4)]
    masks = [g["mask%d" % i].to(device) for i in range(4)]
    pos = [g["pos%d" % i].to(device=device, dtype=dtype) for i in range(4)]
    qe, dpe = g["query_embed"].to(device=device, dtype=dtype), g["depth_pos_embed"].to(device=device, dtype=dtype)
    for mode in ("eval", "train"):
        t.train(mode == "train")
        q = qe if mode == "train" else qe[:50]
        hs, init_ref, inter_refs, inter_dims, a, b = t(srcs, masks, pos, q, dpe, dpe)
        assert a is None and b is None
        _assert_close(hs, g[mode + "_hs"], rel, mode + " hs")
        _assert_close(init_ref, g[mode + "_init_ref"], rel, mode + " init_reference")
        _assert_close(inter_refs, g[mode + "_inter_refs"], rel, mode + " inter_references")
        _assert_close(inter_dims, g[mode + "_inter_dims"], rel, mode + " inter_dims")
    if check_grad:
        t.train(True)
        s0 = srcs[0].clone().requires_grad_(True)
        hs = t([s0] + srcs[1:], masks, pos, qe, dpe, dpe)[0]
        (hs * torch.linspace(-1, 1, hs.numel(), device=device, dtype=dtype).view_as(hs)).sum().backward()
        _assert_close(s0.grad, g["grad_src0"], grad_rel or rel, "d loss / d src0")


def test_transformer_cpu(golden_dir, cpu_msda):
    _transformer_case(_load(golden_dir, "transformer_small"), "cpu", 1e-6)


@pytest.mark.gpu
def test_transformer_gpu(golden_dir):
    g = _load(golden_dir, "transformer_small")
    _transformer_case(g, "cuda", 1e-6, torch.float64)                      # f64 HIP kernels, fwd + grad
    # f32 d32 fast path (fused prologue, window / record kernels, HIP attention): forward to 2e-4; the gradient directly against
    # the reference's float64 gradient -- 5e-3, because grad_loc jumps at pixel borders and an f32 run of the REFERENCE is
    # itself 2e-3 away from its f64 run (the tight f32 gradient bounds are the kernel-level oracle tests)
    _transformer_case(g, "cuda", 2e-4, torch.float32, check_grad=True, grad_rel=5e-3)


def test_transformer_rejects_unshipped_variants():
    from monosowa_amd.monodetr.depthaware_transformer import DepthAwareTransformer
    for kw in ({"two_stage": True}, {"use_dab": True}, {"two_stage_dino": True}):
        with pytest.raises(NotImplementedError):
            DepthAwareTransformer(**kw)


# --------------------------------------------------------------------------------- depth predictor
def _depth_case(g, device, rel):
    from monosowa_amd.monodetr.depth_predictor import DepthPredictor
    cfg = {"num_depth_bins": 80, "depth_min": 1e-3, "depth_max": 60.0, "hidden_dim": 256}
    m = fill_deterministic(DepthPredictor(cfg), 303).eval()
    _same_manifest(m, g["manifest"])
    m = m.to(device)
    _assert_close(m.depth_bin_values, g["bin_values"], 1e-7, "LID bin values")
    feats = [g["f%d" % i].to(device) for i in range(4)]
    logits, embed, wdepth, ip = m(feats, g["mask"].to(device), g["pos"].to(device))
    _assert_close(logits, g["logits"], rel, "depth logits")
    _assert_close(wdepth, g["weighted_depth"], rel, "weighted depth")
    _assert_close(ip, g["ip"], rel * 10, "depth positional embedding")
    _assert_close(embed, g["embed"], rel * 10, "depth embed")
    floor_idx = wdepth.clamp(min=0, max=60.0).floor().long().cpu()
    # integer bookkeeping: identical except where the f32 depth sits within rounding of an integer
    diff = (floor_idx != g["floor_idx"])
    near_int = (g["weighted_depth"] - g["weighted_depth"].round()).abs() < 1e-3
    assert not (diff & ~near_int).any()


def test_depth_predictor_cpu(golden_dir):
    _depth_case(_load(golden_dir, "depth_predictor"), "cpu", 2e-5)


@pytest.mark.gpu
def test_depth_predictor_gpu(golden_dir):
    _depth_case(_load(golden_dir, "depth_predictor"), "cuda", 2e-4)


# ------------------------------------------------------------------ matcher / position / losses
def _matcher_case(g, device):
    from monosowa_amd.monodetr.matcher import HungarianMatcher
    sizes = [int(x) for x in g["sizes"]]
    outputs = {"pred_logits": g["pred_logits"].to(device), "pred_boxes": g["pred_boxes"].to(device)}
    targets = [{k: g["t%d_%s" % (i, k)].to(device) for k in ("labels", "boxes_3d", "boxes")} for i in range(len(sizes))]
    ind = HungarianMatcher(cost_class=2, cost_3dcenter=10, cost_bbox=5, cost_giou=2)(outputs, targets, group_num=int(g["group_num"]))
    for i, (a, b) in enumerate(ind):
        assert a.dtype == torch.int64 and b.dtype == torch.int64
        assert torch.equal(a, g["ind%d_src" % i]) and torch.equal(b, g["ind%d_tgt" % i])     # bit-exact bookkeeping


def test_matcher_indices_cpu(golden_dir):
    _matcher_case(_load(golden_dir, "matcher"), "cpu")


@pytest.mark.gpu
def test_matcher_indices_gpu(golden_dir):
    _matcher_case(_load(golden_dir, "matcher"), "cuda")


def _position_case(golden_dir, device):
    from monosowa_amd.monodetr.misc import NestedTensor
    from monosowa_amd.monodetr.position_encoding import PositionEmbeddingSine
    g = _load(golden_dir, "position_sine")
    mask = torch.as_tensor(g["mask"]).to(device)
    pos = PositionEmbeddingSine(128, normalize=True)(NestedTensor(torch.zeros(2, 256, 6, 8, device=device), mask))
    assert pos.shape == g["pos"].shape
    _assert_close(pos.cpu(), g["pos"], 1e-6, "sine position encoding")
    if device == "cpu":
        assert torch.equal(pos, torch.as_tensor(g["pos"])), "the CPU evaluation reproduces the reference's floats"


def test_position_encoding(golden_dir):
    """Fixture made from the reference class (position_encoding.py:36-56) on a mask with padded rows and columns."""
    _position_case(golden_dir, "cpu")


@pytest.mark.gpu
def test_position_encoding_gpu(golden_dir):
    _position_case(golden_dir, "cuda")


def test_losses(golden_dir):
    from monosowa_amd.monodetr import losses as L
    g = _load(golden_dir, "losses")
    sfl = L.sigmoid_focal_loss(g["sfl_logits"], g["sfl_targets"], 7.0, alpha=0.25, gamma=2)
    _assert_close(sfl, torch.as_tensor(g["sfl"]), 1e-6, "sigmoid focal loss")
    num_gt = [int(x) for x in g["num_gt"]]
    crit = L.DDNLoss()
    boxes_int = L._int_boxes(g["boxes"])
    dm = crit.paint_boxes((2, 24, 80), boxes_int, num_gt, g["depth"], dtype=torch.float32, device="cpu")
    assert torch.equal(dm, g["depth_map"])
    bins = L.lid_bin_indices(dm, target=True)
    assert bins.dtype == torch.int64 and torch.equal(bins, g["depth_bins"])                   # integer, exact
    loss = crit(g["depth_logits"], g["boxes"].clone(), num_gt, g["depth"])
    _assert_close(loss, torch.as_tensor(g["ddn_loss"]), 1e-5, "DDN depth-map loss")


@pytest.mark.gpu
def test_optimised_train_step_reduces_the_loss_on_a_repeated_batch():
    """End to end through every fused backward (MSDA, attention, encoder blocks, norms, matched losses, AdamW): 40
    optimizer steps on one small synthetic batch must bring the weighted loss down and keep it finite."""
    import yaml
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.synthetic import make_batch, prepare_targets
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "configs", "monodetr.yaml")))
    torch.manual_seed(444)
    model, crit = build_model(dict(cfg["model"], device="cuda"))
    model = to_mi355x_layout(model.cuda()).train()
    crit = crit.cuda().train()
    opt = build_optimizer(cfg["optimizer"], model)
    inputs, calibs, targets, _ = make_batch(4, "cuda", seed=2, resolution=(640, 192))
    inputs = inputs.contiguous(memory_format=torch.channels_last)
    hist = []
    for i in range(40):
        tl = prepare_targets(targets, 4)
        opt.zero_grad(set_to_none=True)
        total = weighted_total(crit(model(inputs, calibs, tl, targets["img_size"]), tl), crit.weight_dict)
        total.backward()
        opt.step()
        hist.append(total.item())
    assert all(h == h and abs(h) < 1e6 for h in hist), hist
    assert min(hist[-5:]) < 0.75 * hist[0], hist


# (backbone, W x H, per-GPU batch, mixed cameras): BASELINE config 2 at half resolution with its batch of 16, then the FULL
# geometries of configs 4 and 5 at a small batch: ResNet-101 at 1408 x 376 (S = 11,044 tokens, a 24 x 88 depth
# map: odd extents at every stride), and 1920 x 1280 with a mixed-camera batch (S = 51,000 tokens, 9,600 depth tokens, per-sample
# Canonical Object Space scale and fu)
_STEP_CONFIGS = {"config2_half": ("resnet50", (640, 192), 16, False),
                 "config4_resnet101_1408x376": ("resnet101", (1408, 376), 2, False),
                 "config5_1920x1280_mixed_cameras": ("resnet50", (1920, 1280), 3, True)}


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(_STEP_CONFIGS))
def test_fused_training_path_tracks_the_module_by_module_path(config):
    """Three optimizer steps (dropout 0, same initial weights and batch) with every structural optimisation switched ON
    against the same steps with all of them OFF (module-by-module autograd, PyTorch matched losses, foreach AdamW,
    unmerged projections ...): the loss sequences and the updated weights must agree to fp32 training noise."""
    backbone_name, resolution, batch, mixed = _STEP_CONFIGS[config]
    import copy
    import yaml
    from fused_switches import fused_switches
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.monodetr import criterion
    from monosowa_amd.synthetic import make_batch, prepare_targets
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "configs", "monodetr.yaml")))
    mcfg = dict(cfg["model"], device="cuda", dropout=0.0, backbone=backbone_name, pretrained=False,
                depth_map_size=(resolution[0] // 16, resolution[1] // 16))
    torch.manual_seed(7)
    model0, crit = build_model(mcfg)
    for m in model0.modules():                       # the depth predictor hard-codes dropout 0.1 (depth_predictor.py:48)
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = 0.0
    crit = crit.cuda().train()
    inputs, calibs, targets, info = make_batch(batch, "cuda", seed=3, resolution=resolution, mixed_cameras=mixed)
    inputs = inputs.contiguous(memory_format=torch.channels_last)
    if mixed:                                        # the batch really mixes cameras: three fu, three canonical scales
        assert len(set(calibs[:, 0, 0].tolist())) == 3 and len(set(info["canonical_scale"].tolist())) == 3

    def run(on):
        with fused_switches(on):                     # every listed switch; a renamed one fails instead of becoming a no-op
            model = to_mi355x_layout(copy.deepcopy(model0).cuda()).train()
            opt = build_optimizer(cfg["optimizer"], model)
            if not on:
                opt._fused_step = lambda *a, **k: False
            losses = []
            for _ in range(3):
                tl = prepare_targets(targets, batch)
                opt.zero_grad(set_to_none=True)
                total = criterion.weighted_total(crit(model(inputs, calibs, tl, targets["img_size"]), tl), crit.weight_dict)
                total.backward()
                opt.step()
                losses.append(total.item())
            probe = [model.depthaware_transformer.level_embed.detach().clone(),
                     model.depthaware_transformer.encoder.layers[1].self_attn.sampling_offsets.weight.detach().clone(),
                     model.backbone[0].body.layer3[2].conv2.weight.detach().clone(), model.class_embed[0].weight.detach().clone()]
            return losses, probe
    l_on, w_on = run(True)
    l_off, w_off = run(False)
    for a, b in zip(l_on, l_off):
        assert abs(a - b) <= 2e-3 * abs(b), (l_on, l_off)
    w0 = [model0.depthaware_transformer.level_embed.detach().cuda(),
          model0.depthaware_transformer.encoder.layers[1].self_attn.sampling_offsets.weight.detach().cuda(),
          model0.backbone[0].body.layer3[2].conv2.weight.detach().cuda(), model0.class_embed[0].weight.detach().cuda()]
    for a, b, c in zip(w_on, w_off, w0):
        c = c.to(b.dtype).reshape(b.shape)
        upd_on, upd_off = (a - c).flatten().double(), (b - c).flatten().double()
        assert upd_off.norm() > 0
        # Adam's update is sign-like where the gradient is at noise level, so individual elements may differ by 2 lr;
        # the update VECTORS must point the same way
        cos = torch.dot(upd_on, upd_off) / (upd_on.norm() * upd_off.norm())
        assert cos.item() > 0.98, cos.item()
