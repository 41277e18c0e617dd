"""The pieces that let the shipped MonoDETR detector be evaluated behind a fixed backbone body, in float32 and float64 from the
same weights and features.  Shared by tests/test_train_step_grads_gpu.py and tests/test_eval_forward_gpu.py.

``_Body`` stands in for the ResNet body and returns fixed C3 / C4 / C5 tensors; ``_FrozenMatcher`` hands the first
evaluation's matching to every later one; ``trained_like_msda`` moves the MSDA sampling offsets and attention logits off the
initial integer grid, as a trained checkpoint's are."""
import numpy as np
import torch


class _Body(torch.nn.Module):
    """backbone body stand-in: the fixed C3 / C4 / C5 leaves (the Backbone wraps them as all-valid NestedTensors)"""
    def __init__(self):
        super().__init__()
        self.feats = None

    def forward(self, images):
        return {str(i): f for i, f in enumerate(self.feats)}


class _FrozenMatcher(torch.nn.Module):
    """The first evaluation's assignment for every later one: ``match_layers_begin`` runs as usual, and
    ``match_layers_end_flat`` returns the [3, NL, K] indices recorded from the first call (criterion.py forward_fast)."""
    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.idx = None

    def match_layers_begin(self, *args, **kwargs):
        return self.inner.match_layers_begin(*args, **kwargs)

    def match_layers_end_flat(self, handle):
        got = self.inner.match_layers_end_flat(handle)
        if self.idx is None:
            self.idx = (got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).copy()
            return got
        return self.idx.copy()


def trained_like_msda(model, gen):
    """Sampling offsets away from the initial integer grid and attention logits away from uniform (a checkpoint's are): at the
    grid every sampling location sits on a pixel border, where d(location) jumps and f32 and f64 take different sides.
    Draws from ``gen`` in module order."""
    from monosowa_amd.ms_deform_attn import MSDeformAttn
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, MSDeformAttn):
                for lin, bias_scale in ((m.sampling_offsets, 0.5), (m.attention_weights, 0.3)):
                    lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen) * 0.02)
                    lin.bias.add_(((torch.rand(lin.bias.shape, generator=gen) - 0.5) * 2 * bias_scale).to(lin.bias.device))
