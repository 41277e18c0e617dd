"""Keep masks of the fused dropout kernels, replayed for reference computations in the tests.

The hash is not restated here.  A probe calls the product's own entry points with a recorded seed, the same p and the same
shape and strides as the real call, on constant inputs, and reads back keep / (1 - p):
- ``mono_dropout_add_layernorm_fwd_f32`` with x = 0, z = 1 saves the pre-norm sum s = keep / (1 - p) exactly;
- ``mono_relu_dropout_fwd_f32`` with h = 1 returns y = keep / (1 - p) exactly.

``record()`` wraps ``pointwise._next_seed`` and the two forward wrappers (in ``pointwise`` and in ``encoder_block``, which
imports them by name) and lists every draw in call order.
"""
import contextlib

import torch

from monosowa_amd import encoder_block, pointwise
from monosowa_amd._lib import on_device, raw_stream


def _like(desc):
    shape, stride, device = desc
    return torch.empty_strided(shape, stride, dtype=torch.float32, device=device)


def ln_mask(seed, p, like):
    """keep / (1 - p) of the LayerNorm kernel for (seed, p) over a row-dense tensor laid out like ``like`` (logical shape)."""
    zero, one = torch.zeros_like(like), torch.ones_like(like)
    y, s = torch.empty_like(like), torch.empty_like(like)
    assert s.stride() == like.stride() == zero.stride() == one.stride()
    rows = like.numel() // 256
    mean = torch.empty(rows, dtype=torch.float32, device=like.device)
    rstd = torch.empty_like(mean)
    gamma = torch.ones(256, dtype=torch.float32, device=like.device)
    beta = torch.zeros_like(gamma)
    with on_device(like.device):
        code = pointwise.load().mono_dropout_add_layernorm_fwd_f32(
            zero.data_ptr(), one.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), s.data_ptr(), mean.data_ptr(),
            rstd.data_ptr(), rows, 256, float(p), seed, 1e-5, raw_stream())
    assert code == 0, code
    return s


def relu_mask(seed, p, like):
    """keep / (1 - p) of the ReLU-dropout kernel for (seed, p) over a row-dense tensor laid out like ``like``."""
    one = torch.ones_like(like)
    y = torch.empty_like(like)
    assert y.stride() == like.stride() == one.stride()
    with on_device(like.device):
        code = pointwise.load().mono_relu_dropout_fwd_f32(one.data_ptr(), y.data_ptr(), like.numel(), float(p), seed, raw_stream())
    assert code == 0, code
    return y


class Draw:
    """One call of a dropout forward: ``kind`` ("ln" / "relu"), the seed it used (0 when p == 0), p and the layout of the tensor
    its mask covers (the saved sum s for "ln", the output for "relu").  ``active``: for "relu", where the output is positive."""

    def __init__(self, kind, seed, p, t):
        self.kind, self.seed, self.p = kind, seed, p
        self.desc = (tuple(t.shape), tuple(t.stride()), t.device)
        self.active = t > 0 if kind == "relu" else None

    def mask(self):
        """keep / (1 - p) in the draw's logical shape; all ones for p == 0."""
        like = _like(self.desc)
        if self.p == 0:
            return torch.ones_like(like)
        return (ln_mask if self.kind == "ln" else relu_mask)(self.seed, self.p, like)


@contextlib.contextmanager
def record():
    """Yields a list that fills with a ``Draw`` per dropout forward made inside the block, in call order."""
    draws, seeds = [], []
    next_seed, ln_forward, relu_dropout_forward = pointwise._next_seed, pointwise.ln_forward, pointwise.relu_dropout_forward

    def seed_hook():
        s = next_seed()
        seeds.append(s)
        return s

    def ln_hook(x, z, weight, bias, p, eps):
        n = len(seeds)
        out = ln_forward(x, z, weight, bias, p, eps)
        assert len(seeds) == n + (p > 0) and (p == 0 or out[4] == seeds[-1])
        draws.append(Draw("ln", out[4], p, out[1]))
        return out

    def relu_hook(h, p):
        n = len(seeds)
        y = relu_dropout_forward(h, p)
        assert len(seeds) == n + 1
        draws.append(Draw("relu", seeds[-1], p, y))
        return y

    pointwise._next_seed = seed_hook
    pointwise.ln_forward = encoder_block.ln_forward = ln_hook
    pointwise.relu_dropout_forward = encoder_block.relu_dropout_forward = relu_hook
    try:
        yield draws
    finally:
        pointwise._next_seed = next_seed
        pointwise.ln_forward = encoder_block.ln_forward = ln_forward
        pointwise.relu_dropout_forward = encoder_block.relu_dropout_forward = relu_dropout_forward


def relu_dropout(h, draw):
    """relu(h) * mask with the ReLU's kinks taken from the product's output (``draw.active``) where the mask keeps an element: a
    reference whose pre-activations equal the product's only up to rounding would otherwise flip the odd element near 0, and one
    flipped element moves a weight gradient by more than the tolerance.  Equal to relu(h) * mask wherever the signs agree."""
    return h * (draw.mask().to(h.dtype) * draw.active.to(h.dtype))


def rows_in_memory(t, like):
    """``t`` (logical shape of ``like``, last dim 256) as [rows, 256] in the memory order of ``like``'s rows: the order of the
    per-row outputs (mean, rstd) of the LayerNorm kernel."""
    order = sorted(range(like.dim() - 1), key=lambda d: -like.stride(d))
    return t.permute(*order, like.dim() - 1).reshape(-1, t.shape[-1])
