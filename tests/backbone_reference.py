"""The backbone of this package (ResNet-50 / ResNet-101 body with frozen batch-norm, the input projections) built from the
shipped config with frozen-norm buffers and projection parameters away from the identity map, and an independent float64
CPU evaluation of the same state dict written with nothing but F.conv2d, the frozen-BN affine map, F.max_pool2d and
F.group_norm.  Shared by tests/test_backbone_gpu.py and tests/test_train_step_grads_gpu.py.

``_reference`` reads every weight from ``sd`` by key: entries replaced by leaves with ``requires_grad`` make it
differentiable in them."""
import os

import torch
import torch.nn.functional as F
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = {"resnet50": (3, 4, 6, 3), "resnet101": (3, 4, 23, 3)}


def _model(name):
    from monosowa_amd.helpers.model_helper import build_model, to_mi355x_layout
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "monodetr.yaml")))
    torch.manual_seed(5)
    model, _ = build_model(dict(cfg["model"], backbone=name, device="cuda", depth_map_size=(20, 6)))
    # frozen batch-norm buffers away from the identity map (a checkpoint's are), input projections with a bias
    gen = torch.Generator().manual_seed(11)
    for n, b in model.backbone.named_buffers():
        if n.endswith("running_var"):
            b.copy_(torch.rand(b.shape, generator=gen) * 1.5 + 0.5)
        elif n.endswith("weight"):
            b.copy_(torch.rand(b.shape, generator=gen) * 0.6 + 0.5)
        else:
            b.copy_(torch.randn(b.shape, generator=gen) * 0.2)
    for proj in model.input_proj:
        proj[0].bias.data.copy_(torch.randn(proj[0].bias.shape, generator=gen) * 0.3)
        proj[1].weight.data.copy_(torch.rand(proj[1].weight.shape, generator=gen) + 0.5)
        proj[1].bias.data.copy_(torch.randn(proj[1].bias.shape, generator=gen) * 0.3)
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    return to_mi355x_layout(model.cuda()), sd


def _reference(sd, name, x):
    """float64, plain PyTorch functions only."""
    def conv_bn(x, conv, bn, stride, padding):
        y = F.conv2d(x, sd[conv + ".weight"], None, stride, padding)
        scale = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + 1e-5)             # FrozenBatchNorm2d, backbone.py:52-65
        shift = sd[bn + ".bias"] - sd[bn + ".running_mean"] * scale
        return y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)

    p = "backbone.0.body."
    x = F.relu(conv_bn(x, p + "conv1", p + "bn1", 2, 3))
    x = F.max_pool2d(x, 3, 2, 1)
    feats = []
    for li, blocks in enumerate(DEPTHS[name], start=1):
        for b in range(blocks):
            q = "%slayer%d.%d." % (p, li, b)
            stride = 2 if (b == 0 and li > 1) else 1                                         # v1.5: the 3x3 carries the stride
            out = F.relu(conv_bn(x, q + "conv1", q + "bn1", 1, 0))
            out = F.relu(conv_bn(out, q + "conv2", q + "bn2", stride, 1))
            out = conv_bn(out, q + "conv3", q + "bn3", 1, 0)
            idt = conv_bn(x, q + "downsample.0", q + "downsample.1", stride, 0) if (q + "downsample.0.weight") in sd else x
            x = F.relu(out + idt)
        if li >= 2:
            feats.append(x)
    srcs = []
    for l in range(4):
        src_in = feats[l] if l < 3 else feats[2]
        k = "input_proj.%d." % l
        y = F.conv2d(src_in, sd[k + "0.weight"], sd[k + "0.bias"], 1 if l < 3 else 2, 0 if l < 3 else 1)
        srcs.append(F.group_norm(y, 32, sd[k + "1.weight"], sd[k + "1.bias"], 1e-5))
    return feats, srcs
