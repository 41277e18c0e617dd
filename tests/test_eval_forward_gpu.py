"""The eval forward -- what ``Tester.inference`` runs, in ``eval()`` under ``torch.no_grad()`` -- and the detections decoded
from it, against float64.

Under no_grad the forward takes paths the train step never takes: the decoder's merged value projection hands out column
blocks of one F.linear, the decoder runs 50 queries per image without group folding (self-attention at 50 x 50, depth
cross-attention over the stride-16 tokens), the encoder runs layer by layer through the forward-only fused MSDA, the
decoder's LayerNorms see 50 x B rows, the head tail adds the reference boxes inside its kernel, and detections come from
the device kernel.  Each model is evaluated three times from identical weights and inputs:
  F  float32, every switch at its shipped value (the product),
  P  float32, every switch of tests/fused_switches.py plain, and the attention and dropout-add-LayerNorm of the decoder,
     encoder and depth encoder (which have no switch) through nn.MultiheadAttention / nn.LayerNorm,
  R  float64, every switch plain (the f64 MSDA kernels are pinned to the C oracle by tests/test_msda_gpu.py).
Every output tensor, aux_outputs and pred_depth_map_logits included, is compared with R by ||x - x_R|| / ||x_R||; F and P
must meet one bound per output group, so no bound is tighter than honest float32 arithmetic.  Counted spies on the eval-only
entry points show that F took them and P did not (no autograd graph exists under no_grad to inspect).

The real-backbone case feeds R with C3 / C4 / C5 of the float64 CPU ResNet-50 of tests/backbone_reference.py, and evaluates
the same F module again after two fused-AdamW steps, after a checkpoint reload and from a captured graph: every weight cache
(folded weights, frozen-norm scale / shift, the layer1 transposes) must follow the parameters."""
import collections
import contextlib
import copy
import os

import numpy as np
import pytest
import torch
import yaml

from backbone_reference import _model, _reference
from detector_reference import _Body, trained_like_msda
from fused_switches import fused_switches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Per-tensor bounds on ||x - x_R|| / ||x_R||, one per output group (final layer and aux layers alike), about 3x the worse of
# e_F and e_P.  Measured on the MI355X, worst tensor of the group over every case of this module, e_F / e_P:
BOUNDS = {
    "logits": 2.5e-6,              # 8.3e-7 / 8.3e-7 (pred_logits, 1280 x 384 at batch 9)
    "boxes": 7e-7,                 # 2.3e-7 / 2.4e-7 (pred_boxes, 1280 x 384 at batch 9)
    "dim": 8e-6,                   # 2.7e-6 / 2.8e-6 (aux1.pred_3d_dim, 1280 x 384 at batch 9)
    "depth": 4e-6,                 # 1.3e-6 / 4.0e-7 (aux1.pred_depth depth column, 1280 x 384 at batch 9)
    "depth log-variance": 1.1e-5,  # 3.5e-6 / 3.7e-6 (aux1.pred_depth log-variance column, 1280 x 384 at batch 9)
    "angle": 7e-6,                 # 2.2e-6 / 2.2e-6 (aux1.pred_angle, 1280 x 384 at batch 9)
    "depth map logits": 3.5e-6,    # 1.1e-6 / 9.2e-7 (pred_depth_map_logits, ResNet-50 320 x 96)
}
# Detections (decode_detections rows matched by image, query and class).  SCORE_MARGIN: a detection whose float64 score lies
# within this distance of the 0.2 threshold or of the top-50 boundary may appear on one side only; HEADING_MARGIN: the same
# for the top two heading bins (the 12 bin logits) when alpha and ry are compared.  Measured max |score_F - score_R|
# 1.4e-6 and max |angle_F - angle_R| 3.5e-6 (1280 x 384 at batch 9): the margins are about 7x those.
SCORE_MARGIN = 1e-5
HEADING_MARGIN = 2.5e-5
# worst |F - R| of a matched row: 2D box corners in pixels, h / w / l and x / y / z in metres (relative to max(1, |R|)), alpha and
# ry in radians, final score (relative to max(1, |R|)).  Measured (1280 x 384 at batch 9): box 4.6e-4, hwl 2.3e-6, xyz 3.7e-6,
# ry 2.4e-6, score 1.0e-6
DET_BOUNDS = {"box": 1.5e-3, "hwl": 7e-6, "xyz": 1.1e-5, "ry": 7.5e-6, "score": 3e-6}
CLS_MEAN_SIZE = np.array([[1.76, 0.66, 0.84], [1.53, 1.63, 3.88], [1.73, 0.60, 1.76]])     # h, w, l of the three classes


def _cfg(W, H):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    return cfg, dict(cfg["model"], device="cuda", pretrained=False, depth_map_size=(-(-W // 16), -(-H // 16)))


def _detections_visible(model, gen):
    """class logits around the 0.2 threshold (the initial prior of 0.01 keeps every score below it): some detections are
    kept, some are not"""
    with torch.no_grad():
        for lin in model.class_embed:
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) * 0.06)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen) * 0.3 - 2.0)


# --------------------------------------------------------------------------------------------------------------- P's plain paths
def _plain_norm(x, z, norm, dropout):
    return norm(x + dropout(z))


@contextlib.contextmanager
def _patched(table):
    """(owner, name, value): set, and restore afterwards; a name that no longer exists fails"""
    saved = []
    try:
        for owner, name, value in table:
            assert hasattr(owner, name), "%s.%s is gone: update tests/test_eval_forward_gpu.py" % (getattr(owner, "__name__", owner), name)
            saved.append((owner, name, name in vars(owner), vars(owner).get(name)))
            setattr(owner, name, value)
        yield
    finally:
        for owner, name, had, value in reversed(saved):
            if had:
                setattr(owner, name, value)
            else:
                delattr(owner, name)


def _plain_unswitched():
    """P: the attention cores and the dropout-add-LayerNorms have no switch; route them through the PyTorch modules"""
    from monosowa_amd.monodetr import depth_predictor as D, depthaware_transformer as T
    never = lambda *args, **kwargs: False
    return _patched([(T, "mha_supported", never), (D, "mha_supported", never),
                     (T, "dropout_add_layernorm", _plain_norm), (D, "dropout_add_layernorm", _plain_norm)])


# --------------------------------------------------------------------------------------------------------------- spies
def _spy_table(depth_tokens):
    from monosowa_amd import kitti_eval, ms_deform_attn_func, pointwise
    from monosowa_amd.monodetr import backbone, depthaware_transformer as T, monodetr

    def value_proj(a, k, r):
        if r is None:
            return ["merged_value_proj: None"]
        if torch.is_grad_enabled():
            return ["merged_value_proj: grad"]
        one_buffer = len({t.untyped_storage().data_ptr() for t in r}) == 1
        return ["merged_value_proj: no-grad column blocks" if one_buffer and r[0].stride(-2) == len(r) * r[0].shape[-1]
                else "merged_value_proj: no-grad, other layout"]

    def msda(a, k, r):
        value, proj, ref = a[0], a[3], a[4]
        tags = ["msda: encoder (Lq == S)" if proj.shape[1] == value.shape[1] and ref.shape[-1] == 2 else
                "msda: decoder (6-d reference)" if ref.shape[-1] == 6 else "msda: decoder (2-d reference)"]
        if value.shape[0] == 1 and not value.is_contiguous():
            tags.append("msda: N == 1 value view")
        return tags

    def mha(a, k, r):
        q, key = a[1], a[2]
        if q.shape[0] == key.shape[0] == 50:
            return ["mha_forward: decoder self-attention 50 x 50"]
        return ["mha_forward: decoder depth cross-attention" if key.shape[0] == depth_tokens else "mha_forward: other"]

    def layernorm(a, k, r):
        return ["layernorm: rows %d p %g" % (a[0].numel() // 256, a[4])]

    def head_tail(a, k, r):
        return ["head_tail: ref in kernel" if k.get("ref") is not None else "head_tail: no ref"]

    def returned(tag):
        return lambda a, k, r: [tag + (": tensor" if r is not None else ": None")]

    def called(tag):
        return lambda a, k, r: [tag]

    return [(T, "merged_value_proj", value_proj), (T._MergedValueProj, "apply", called("_MergedValueProj.apply")),
            (ms_deform_attn_func.MSDeformAttnFusedMergedFunction, "apply", msda), (T, "mha_forward", mha),
            (pointwise._DropoutAddLayerNorm, "apply", layernorm), (monodetr, "head_tail", head_tail),
            (pointwise._DepthExpectation, "apply", called("depth expectation kernel")),
            (kitti_eval, "extract_dets_device", called("extract_dets_device")),
            (backbone, "conv1x1_no_grad", returned("conv1x1_no_grad")), (backbone, "bias_relu_maxpool", called("bias_relu_maxpool")),
            (backbone, "conv1x1_head", called("conv1x1_head")), (backbone, "conv1x1_tail", called("conv1x1_tail")),
            (backbone, "conv1x1_tail_ds", called("conv1x1_tail_ds"))]


@contextlib.contextmanager
def _spies(depth_tokens):
    counts = collections.Counter()

    def wrap(fn, tags):
        def spy(*args, **kwargs):
            r = fn(*args, **kwargs)
            counts.update(tags(args, kwargs, r))
            return r
        return spy

    table = _spy_table(depth_tokens)
    with _patched([(owner, name, wrap(getattr(owner, name), tags)) for owner, name, tags in table]):
        yield counts


def _expected_detector_paths(B, real_backbone):
    want = {"merged_value_proj: no-grad column blocks": 1, "msda: encoder (Lq == S)": 3, "msda: decoder (6-d reference)": 2,
            "msda: decoder (2-d reference)": 1, "mha_forward: decoder self-attention 50 x 50": 3,
            "mha_forward: decoder depth cross-attention": 3, "layernorm: rows %d p 0" % (50 * B): 12, "head_tail: ref in kernel": 3,
            "depth expectation kernel": 1}
    if real_backbone:
        want.update({"bias_relu_maxpool": 1, "conv1x1_head": 3, "conv1x1_tail_ds": 1, "conv1x1_tail": 2})
    return want


def _check_paths(F_counts, P_counts, B, real_backbone=False):
    print("F paths:", dict(sorted(F_counts.items())))
    print("P paths:", dict(sorted(P_counts.items())))
    for tag, n in _expected_detector_paths(B, real_backbone).items():
        assert F_counts[tag] == n, (tag, F_counts[tag], n)
        assert P_counts[tag] == 0, (tag, P_counts[tag])
    assert F_counts["_MergedValueProj.apply"] == 0 and F_counts["mha_forward: other"] == 0
    assert all(tag.endswith(" p 0") for tag in F_counts if tag.startswith("layernorm:")), sorted(F_counts)
    if B == 1:
        assert F_counts["msda: N == 1 value view"] == 3, F_counts          # the decoder's column blocks, not copies
    if real_backbone:
        assert F_counts["conv1x1_no_grad: tensor"] > 0 and P_counts["conv1x1_no_grad: tensor"] == 0, (F_counts, P_counts)


# --------------------------------------------------------------------------------------------------------------- comparison
def _flat(out):
    """every output tensor by name; pred_depth as its two columns"""
    named = {"pred_depth_map_logits": out["pred_depth_map_logits"]}
    layers = [("aux%d." % i, a) for i, a in enumerate(out["aux_outputs"])] + [("", out)]
    for prefix, layer in layers:
        for k in ("pred_logits", "pred_boxes", "pred_3d_dim", "pred_angle"):
            named[prefix + k] = layer[k]
        named[prefix + "pred_depth.value"] = layer["pred_depth"][..., 0]
        named[prefix + "pred_depth.log_variance"] = layer["pred_depth"][..., 1]
    assert len(out["aux_outputs"]) == 2
    return named


def _group(name):
    for key, group in (("pred_logits", "logits"), ("pred_boxes", "boxes"), ("pred_3d_dim", "dim"), ("pred_depth.value", "depth"),
                       ("pred_depth.log_variance", "depth log-variance"), ("pred_angle", "angle"),
                       ("pred_depth_map_logits", "depth map logits")):
        if name.endswith(key):
            return group
    raise AssertionError("output %s belongs to no group" % name)


def _rel_norm(x, ref):
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    return float((x - ref).norm() / ref.norm().clamp_min(1e-300))


def _compare(title, outs, ref):
    """outs: {"F": out, "P": out}; asserts every bound, prints the worst tensor of every group"""
    want = _flat(ref)
    errs = {who: {n: _rel_norm(t, want[n]) for n, t in _flat(out).items()} for who, out in outs.items()}
    bad = []
    print("\n%s: ||x - x_R|| / ||x_R||, worst tensor per group" % title)
    for group, bound in BOUNDS.items():
        names = [n for n in want if _group(n) == group]
        assert names, group
        line = []
        for who, e in errs.items():
            worst = max(names, key=lambda n: e[n])
            line.append("e_%s %.2e (%s)" % (who, e[worst], worst))
            bad += [(who, n, e[n], bound) for n in names if not e[n] <= bound]
        print("  %-19s bound %.1e  %s" % (group, bound, "  ".join(line)))
    assert not bad, "(run, output, error, bound): %s" % bad[:12]
    for n, t in want.items():
        assert torch.isfinite(t).all(), n


# --------------------------------------------------------------------------------------------------------------- evaluation
def _evaluate(model, images, calibs, img_sizes, on, dtype, depth_tokens):
    """``Tester.inference``'s call, under the switches of F (on=True) or P / R (on=False); -> (outputs, entry-point counts)"""
    plain = contextlib.nullcontext() if on else _plain_unswitched()
    with fused_switches(on), plain, _spies(depth_tokens) as counts, torch.no_grad():
        model.eval()
        out = model(images.to(dtype), calibs.to(dtype), None, img_sizes, dn_args=0)
    torch.cuda.synchronize()
    return out, counts


def _stub_model(model0, feats, dtype):
    model = to_layout(copy.deepcopy(model0).to(device="cuda", dtype=dtype))
    model.backbone[0].body.feats = [f.to(device="cuda", dtype=dtype).contiguous(memory_format=torch.channels_last) for f in feats]
    return model


def to_layout(model):
    from monosowa_amd.helpers.model_helper import to_mi355x_layout
    return to_mi355x_layout(model)


def _info(B, img_sizes):
    return {"img_id": np.arange(B), "img_size": img_sizes.cpu().numpy(), "height_crop": np.ones(B, np.float32),
            "canonical_scale": np.full(B, 0.7, np.float32)}


# --------------------------------------------------------------------------------------------------------------- detections
def _extract(out, on):
    from monosowa_amd.helpers.decode_helper import extract_dets_from_outputs
    with fused_switches(on), _spies(-1) as counts:
        dets = extract_dets_from_outputs(out, K=50, topk=50)
    return dets, counts


def _decoded(dets, info, calibs):
    from monosowa_amd.helpers.decode_helper import PinholeCalib, decode_detections
    cals = [PinholeCalib(p) for p in calibs.double().cpu().numpy()]
    return decode_detections(dets.cpu().numpy(), info, cals, CLS_MEAN_SIZE, threshold=0.2)          # (as Tester.inference hands them)


def _check_detections(title, outF, outR, info, calibs):
    from monosowa_amd.helpers import decode_helper
    dF, cF = _extract(outF, True)
    dR, cR = _extract(outR, False)
    assert cF["extract_dets_device"] == 1 and cR["extract_dets_device"] == 0, (cF, cR)
    assert dF.dtype == torch.float32 and dR.dtype == torch.float64
    # the device kernel against the torch formulation on F's own outputs: gathered columns bit for bit, the rest to rounding
    with fused_switches(False):
        dT = decode_helper.extract_dets_from_outputs(outF, K=50, topk=50)
    gathered = [0] + list(range(6, 36))
    assert torch.equal(dF[:, :, gathered], dT[:, :, gathered])
    assert torch.allclose(dF, dT, rtol=2e-6, atol=1e-7)

    B, Q, C = outR["pred_logits"].shape
    prob = {"F": outF["pred_logits"].sigmoid(), "R": outR["pred_logits"].sigmoid()}
    score_err = float((prob["F"].double() - prob["R"]).abs().max())
    angle_err = float((outF["pred_angle"].double() - outR["pred_angle"]).abs().max())
    ranked = {}
    for who, d in (("F", dF), ("R", dR)):
        s, idx = torch.topk(prob[who].reshape(B, -1), 50, dim=1)
        assert torch.equal(d[:, :, 0].long(), idx % C) and torch.allclose(d[:, :, 1], s, rtol=2e-6, atol=0), who   # torch.topk's order
        ranked[who] = (idx // C).cpu().numpy(), (idx % C).cpu().numpy()
    pR = prob["R"].reshape(B, -1).sort(dim=1, descending=True).values.cpu().numpy()
    boundary = (pR[:, 49] + pR[:, 50]) / 2
    probR = prob["R"].cpu().numpy()

    rows = {}
    for who, d in (("F", dF), ("R", dR)):
        res = _decoded(d, info, calibs)
        keep = ~(d[:, :, 1].cpu().numpy() < 0.2)                   # decode_detections' own test
        rows[who] = {}
        for i in range(B):
            ranks = np.nonzero(keep[i])[0]
            assert len(ranks) == len(res[i])
            for rank, row in zip(ranks, res[i]):
                q, c = ranked[who][0][i, rank], ranked[who][1][i, rank]
                assert int(row[0]) == c
                rows[who][(i, int(q), int(c))] = (int(rank), np.asarray(row[1:], dtype=np.float64))
    near = lambda key: abs(probR[key] - 0.2) <= SCORE_MARGIN or abs(probR[key] - boundary[key[0]]) <= SCORE_MARGIN
    only = set(rows["F"]) ^ set(rows["R"])
    assert all(near(k) for k in only), [(k, probR[k]) for k in only if not near(k)]
    both = sorted(set(rows["F"]) & set(rows["R"]), key=lambda k: (k[0], rows["R"][k][0]))
    n_clear = sum(not near(k) for k in rows["R"])
    assert n_clear >= 2 * B, "too few detections clear of the margins to test anything: %d" % n_clear
    for a in both:          # rank order of every pair the float64 scores separate by more than the margin
        for b in both:
            if a[0] == b[0] and probR[a] > probR[b] + SCORE_MARGIN:
                assert rows["F"][a][0] < rows["F"][b][0], (a, b, probR[a], probR[b])
    # row: alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score
    err = collections.defaultdict(float)
    skipped_ry = 0
    for k in both:
        f, r = rows["F"][k][1], rows["R"][k][1]
        err["box"] = max(err["box"], np.abs(f[1:5] - r[1:5]).max())
        err["hwl"] = max(err["hwl"], (np.abs(f[5:8] - r[5:8]) / np.maximum(1, np.abs(r[5:8]))).max())
        err["xyz"] = max(err["xyz"], (np.abs(f[8:11] - r[8:11]) / np.maximum(1, np.abs(r[8:11]))).max())
        err["score"] = max(err["score"], abs(f[12] - r[12]) / max(1, abs(r[12])))
        bins = np.sort(dR[k[0], rows["R"][k][0], 7:19].cpu().numpy())
        if bins[-1] - bins[-2] <= HEADING_MARGIN:
            skipped_ry += 1
            continue
        for j in (0, 11):                    # alpha and ry: angles, compared modulo 2 pi
            err["ry"] = max(err["ry"], abs((f[j] - r[j] + np.pi) % (2 * np.pi) - np.pi))
    print("%s detections: %d kept by F, %d by R, %d matched, %d only on one side (all within the margins), %d clear of them; "
          "max |score_F - score_R| %.2e, max |angle_F - angle_R| %.2e, ry skipped %d" %
          (title, len(rows["F"]), len(rows["R"]), len(both), len(only), n_clear, score_err, angle_err, skipped_ry))
    print("  matched-row errors: " + "  ".join("%s %.2e (bound %.1e)" % (k, err[k], DET_BOUNDS[k]) for k in DET_BOUNDS))
    assert score_err <= SCORE_MARGIN / 3 and angle_err <= HEADING_MARGIN / 3, (score_err, angle_err)
    assert all(err[k] <= DET_BOUNDS[k] for k in DET_BOUNDS), dict(err)


# --------------------------------------------------------------------------------------------------------------- detector cases
# (W, H), batch: the shipped pyramid (160 x 48, 80 x 24, 40 x 12, 20 x 6: S = 10,200) at 9, the last partial batch of the 3,769
# image val split; 520 x 136 whose levels (65 x 17, 33 x 9, 17 x 5, 9 x 3) are odd; 640 x 192 at batch 1 (the N == 1 value
# view, LayerNorm on 50 rows)
_DET_CASES = {"shipped_1280x384_b9": ((1280, 384), 9), "odd_520x136_b3": ((520, 136), 3), "config2_640x192_b1": ((640, 192), 1)}


@pytest.mark.parametrize("case", list(_DET_CASES))
def test_eval_forward_and_detections_equal_float64(case):
    from monosowa_amd.helpers.model_helper import build_model
    from monosowa_amd.synthetic import make_batch
    (W, H), B = _DET_CASES[case]
    levels = [(-(-H // s), -(-W // s)) for s in (8, 16, 32)]
    cfg, mcfg = _cfg(W, H)
    torch.manual_seed(7)
    model0, _ = build_model(mcfg)
    assert model0.aux_loss and model0.with_box_refine and model0.num_queries == 50 and cfg["tester"]["threshold"] == 0.2
    gen = torch.Generator().manual_seed(29)
    trained_like_msda(model0, gen)
    _detections_visible(model0, gen)
    model0.backbone[0].body = _Body()
    feats = [torch.randn(B, c, h, w, generator=gen, dtype=torch.float64) for c, (h, w) in zip((512, 1024, 2048), levels)]
    _, calibs, targets, _ = make_batch(B, "cuda", seed=5, resolution=(W, H), mixed_cameras=True)
    img_sizes = targets["img_size"].clone()
    images = torch.zeros(B, 3, H, W, device="cuda")
    tokens = levels[1][0] * levels[1][1]

    outF, cF = _evaluate(_stub_model(model0, feats, torch.float32), images, calibs, img_sizes, True, torch.float32, tokens)
    outP, cP = _evaluate(_stub_model(model0, feats, torch.float32), images, calibs, img_sizes, False, torch.float32, tokens)
    outR, _ = _evaluate(_stub_model(model0, feats, torch.float64), images, calibs, img_sizes, False, torch.float64, tokens)
    _check_paths(cF, cP, B)
    _compare(case, {"F": outF, "P": outP}, outR)
    _check_detections(case, outF, outR, _info(B, img_sizes), calibs)


# --------------------------------------------------------------------------------------------------------------- real backbone
_RB_HW = (96, 320)


def _real_backbone_model():
    """ResNet-50 detector of tests/backbone_reference.py (frozen norms and projections away from the identity) with trained-like
    MSDA and visible detections; and a stub-body twin that has never run (R's template: no caches)"""
    model, _ = _model("resnet50")
    gen = torch.Generator().manual_seed(31)
    trained_like_msda(model, gen)
    _detections_visible(model, gen)
    template = copy.deepcopy(model)
    template.backbone[0].body = _Body()
    return model.eval(), template


def _state(model):
    return {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}


def _reference_eval(template, sd, images, calibs, img_sizes):
    """R: C3 / C4 / C5 from the float64 CPU ResNet-50 on ``images`` and ``sd``, then the float64 stub-body detector"""
    feats, _ = _reference(sd, "resnet50", images.double().cpu())
    model = copy.deepcopy(template).to(device="cuda", dtype=torch.float64)
    model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("backbone.0.body.")})
    model = to_layout(model)
    model.backbone[0].body.feats = [f.cuda().contiguous(memory_format=torch.channels_last) for f in feats]
    H, W = _RB_HW
    return _evaluate(model, torch.zeros(images.shape[0], 3, H, W, device="cuda"), calibs, img_sizes, False, torch.float64,
                     (H // 16) * (W // 16))[0]


def _batch(seed, B=2, camera_scale=1.0, img_size=(1242, 375)):
    from monosowa_amd.synthetic import make_batch
    H, W = _RB_HW
    images, calibs, targets, info = make_batch(B, "cuda", seed=seed, resolution=(W, H))
    calibs = calibs.clone()
    calibs[:, 0, 0] *= camera_scale
    calibs[:, 1, 1] *= camera_scale
    img_sizes = torch.tensor([img_size] * B, dtype=targets["img_size"].dtype, device="cuda")
    img_sizes[1:, 1] += 9                      # (the two images of a batch differ as well)
    return images, calibs, targets, img_sizes


def test_real_backbone_eval_after_train_steps_and_checkpoint_reload(tmp_path):
    """(1) the first eval; (2) two fused-AdamW train steps, then eval again against R rebuilt from the updated state dict;
    (3) the original weights restored by save_helper.load_checkpoint, then eval again against the first R.  The same module
    object throughout: a weight cache that misses an update serves stale weights to (2) or (3)."""
    from monosowa_amd.helpers.optimizer_helper import build_optimizer
    from monosowa_amd.helpers.save_helper import get_checkpoint_state, load_checkpoint, save_checkpoint
    from monosowa_amd.monodetr.criterion import weighted_total
    from monosowa_amd.helpers.model_helper import build_model
    from monosowa_amd.synthetic import make_batch, prepare_targets
    H, W = _RB_HW
    B, tokens = 2, (H // 16) * (W // 16)
    model, template = _real_backbone_model()
    images, calibs, targets, img_sizes = _batch(41)
    info = _info(B, img_sizes)
    sd0 = _state(model)
    save_checkpoint(get_checkpoint_state(model, None, epoch=0), str(tmp_path / "before"))

    plain = copy.deepcopy(model)
    outF, cF = _evaluate(model, images, calibs, img_sizes, True, torch.float32, tokens)
    outP, cP = _evaluate(plain, images, calibs, img_sizes, False, torch.float32, tokens)
    del plain
    outR = _reference_eval(template, sd0, images, calibs, img_sizes)
    _check_paths(cF, cP, B, real_backbone=True)
    _compare("resnet50 320x96 b2", {"F": outF, "P": outP}, outR)
    _check_detections("resnet50 320x96 b2", outF, outR, info, calibs)

    # (2) two train steps with the shipped optimizer (the fused AdamW kernel writes the parameters through raw pointers, without
    # bumping their versions); lr 2e-3 moves the weights by ~1 % per step, far past every bound
    cfg, mcfg = _cfg(W, H)
    _, crit = build_model(mcfg)
    crit = crit.cuda().train()
    opt = build_optimizer(dict(cfg["optimizer"], lr=2e-3), model)
    from monosowa_amd import pointwise
    fused = []
    real_step = pointwise.FusedAdamWPlan.step
    with _patched([(pointwise.FusedAdamWPlan, "step", lambda self, *a: fused.append(1) or real_step(self, *a))]):
        for seed in (51, 52):
            x, c, t, _ = make_batch(B, "cuda", seed=seed, resolution=(W, H))
            model.train()
            tl = prepare_targets(t, B)
            total = weighted_total(crit(model(x.contiguous(memory_format=torch.channels_last), c, tl, t["img_size"]), tl), crit.weight_dict)
            opt.zero_grad(set_to_none=True)
            total.backward()
            opt.step()
    assert len(fused) == 4, "the fused AdamW kernel took %d of the 4 group steps" % len(fused)
    sd1 = _state(model)
    moved = max(float((sd1[k] - sd0[k]).abs().max()) for k in sd0 if k.startswith("backbone.0.body.layer4."))
    assert moved > 1e-3, moved
    out1, c1 = _evaluate(model, images, calibs, img_sizes, True, torch.float32, tokens)
    _check_paths(c1, collections.Counter(), B, real_backbone=True)
    _compare("after two AdamW steps", {"F": out1}, _reference_eval(template, sd1, images, calibs, img_sizes))

    # (3) the original weights back through the checkpoint loader
    load_checkpoint(model, None, str(tmp_path / "before.pth"), map_location="cuda")
    assert all(torch.equal(v, sd0[k]) for k, v in _state(model).items())
    out2, _ = _evaluate(model, images, calibs, img_sizes, True, torch.float32, tokens)
    _compare("after the checkpoint reload", {"F": out2}, outR)


def test_graph_replay_of_the_eval_forward_equals_float64():
    """GraphedForward captured on batch a, replayed on batch b (other images, cameras and image sizes): every output against
    R(b); replayed on a again: the first replay of a.  The shipped mode is not bitwise reproducible (the GroupNorm statistics
    are added with float64 atomics in arrival order; measured: replays of a differ by up to 1.2e-6 in pred_depth_map_logits), so
    there the replays must agree within the bounds; under torch's deterministic mode the second replay of a must equal the
    first bit for bit."""
    from monosowa_amd.helpers.tester_helper import GraphedForward
    model, template = _real_backbone_model()
    sd = _state(model)
    a = _batch(61)
    b = _batch(62, camera_scale=1.3, img_size=(1224, 370))
    a, b = [(x[0], x[1], x[3]) for x in (a, b)]
    assert not torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])

    def replays():
        graph = GraphedForward(model, *a)
        out = [copy.deepcopy(graph(*x)) for x in (a, b, a)]
        torch.cuda.synchronize()
        return out

    first_a, got_b, again_a = replays()
    _compare("graph replay of batch b", {"F": got_b}, _reference_eval(template, sd, *b))
    _compare("graph replay of batch a", {"F": first_a}, _reference_eval(template, sd, *a))
    e = {n: _rel_norm(t, _flat(first_a)[n]) for n, t in _flat(again_a).items()}
    print("second replay of a against the first: worst %.2e (%s)" % max((v, n) for n, v in e.items()))
    assert all(v <= BOUNDS[_group(n)] for n, v in e.items()), e
    cublas_env = os.environ.pop("CUBLAS_WORKSPACE_CONFIG", None)
    os.environ["CUBLAS_WORKSPACE_CONFIG"] = ":4096:8"
    torch.use_deterministic_algorithms(True)
    try:
        first_a, got_b, again_a = replays()
    finally:
        torch.use_deterministic_algorithms(False)
        os.environ.pop("CUBLAS_WORKSPACE_CONFIG")
        if cublas_env is not None:
            os.environ["CUBLAS_WORKSPACE_CONFIG"] = cublas_env
    _compare("deterministic graph replay of batch b", {"F": got_b}, _reference_eval(template, sd, *b))
    for n, t in _flat(first_a).items():
        assert torch.equal(t, _flat(again_a)[n]), n
