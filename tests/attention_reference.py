"""Plain-formula reference, input regimes and dropout-mask recovery for the tests of the fp32 attention core
(monosowa_amd/csrc/flash_attn.hip).  No tests in here: test_attention_reference_cpu.py checks this helper on the CPU,
test_attention_core_gpu.py uses it against the kernels."""
import math

import torch

REGIMES = ("randn", "sharp", "offset", "ascending", "descending", "late_spike", "early_spike", "scale_zero", "scale_one",
           "scale_negative")
# the spike key is SPIKE * u.  Its logit is SPIKE * (8 + q.u) / sqrt(32) with q.u ~ N(0, 1) -- about 17 on a typical row, 9 on
# the lowest of a few hundred -- against log(sum of the other keys' exp) of about 7: every row gives the key >= 0.9, the
# lowest rows leave the rest enough weight for gradients far above rounding (30 saturates to probability exactly 1.0)
SPIKE = 12.0


def reference(q, k, v, go, scale, key_padding_mask=None, keep=None, keep_scale=1.0, dtype=torch.float64):
    """o, dq, dk, dv, lse of softmax(q k^T * scale [masked_fill -inf]) [* keep * keep_scale] @ v through autograd, evaluated
    in ``dtype`` on the inputs' device.  lse: natural-log logsumexp of the (masked) logits, [B, H, Lq].
    key_padding_mask: [B, Lk], True / non-zero = the key takes no part; keep: [B, H, Lq, Lk] dropout keep mask."""
    before = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")            # the float32 run is a yardstick: plain float32 products
    try:
        qd, kd, vd = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
        s = (qd @ kd.transpose(-1, -2)) * scale
        if key_padding_mask is not None:
            s = s.masked_fill(key_padding_mask.bool()[:, None, None, :], float("-inf"))
        lse = torch.logsumexp(s, -1)
        p = torch.softmax(s, -1)
        if keep is not None:
            p = p * keep.to(dtype) * keep_scale
        o = p @ vd
        o.backward(go.detach().to(dtype))
    finally:
        torch.set_float32_matmul_precision(before)
    return o.detach(), qd.grad, kd.grad, vd.grad, lse.detach()


def make_case(name, B, H, Lq, Lk, generator):
    """q, k, v, go (float32 [B, H, L, 32] on the generator's device) and the softmax scale of one input regime:

    randn           unit normal inputs, scale 1/sqrt(32): logits within about +-5, flat rows
    sharp           q, k = 4 randn: peaked rows, logits of 50 and more
    offset          q, k = randn + 3: a large common part in every logit
    ascending       q += 8 u, k += linspace(0, 1, Lk) 16 u (u: a unit vector per (b, h)): the row maximum climbs from key tile
                    to key tile, so the online softmax rescales what it has accumulated at every tile
    descending      the same with -linspace: the first tile holds the maximum, nothing is ever rescaled
    late_spike      q += 8 u, last key = SPIKE u: the last key takes nearly all of the row and wipes out the earlier tiles
    early_spike     the same on key 0
    scale_zero / scale_one / scale_negative     randn inputs with softmax scale 0.0 / 1.0 / -0.3"""
    dev = generator.device
    rn = lambda L: torch.randn(B, H, L, 32, generator=generator, device=dev, dtype=torch.float32)
    q, k, v, go = rn(Lq), rn(Lk), rn(Lk), rn(Lq)
    scale = 1.0 / math.sqrt(32)
    if name == "sharp":
        q, k = 4 * q, 4 * k
    elif name == "offset":
        q, k = q + 3, k + 3
    elif name in ("ascending", "descending", "late_spike", "early_spike"):
        u = torch.randn(B, H, 1, 32, generator=generator, device=dev, dtype=torch.float32)
        u = u / u.norm(dim=-1, keepdim=True)
        q = q + 8 * u
        if name in ("ascending", "descending"):
            ramp = torch.linspace(0, 1, Lk, device=dev, dtype=torch.float32).view(1, 1, Lk, 1)
            k = k + (ramp if name == "ascending" else -ramp) * 16 * u
        else:
            k = k.clone()
            k[:, :, Lk - 1 if name == "late_spike" else 0] = SPIKE * u[:, :, 0]
    elif name == "scale_zero":
        scale = 0.0
    elif name == "scale_one":
        scale = 1.0
    elif name == "scale_negative":
        scale = -0.3
    elif name != "randn":
        raise ValueError("unknown regime %r" % (name,))
    return q, k, v, go, scale


def recover_keep(q, k, scale, p, seed, key_padding_mask=None):
    """The [B, H, Lq, Lk] boolean dropout keep mask that ``flash_attn.forward`` draws for (p, seed) at the geometry of q and k:
    ceil(Lk / 32) forwards with q = 0 -- every live probability is exactly 1 / live, so non-zero -- and one-hot value blocks, so
    that channel c of call i is the dropped probability of key 32 i + c.  The mask is a function of (seed, batch * head, query,
    key) alone, so the probabilities do not matter.  Padded keys carry no probability and read as False."""
    from monosowa_amd import flash_attn as FA
    B, H, Lq, _ = q.shape
    Lk = k.size(2)
    zero_q = torch.zeros(B, H, Lq, 32, dtype=torch.float32, device=q.device)
    keys = torch.arange(Lk, device=q.device)
    cols = []
    for i in range((Lk + 31) // 32):
        onehot = (keys[:, None] - 32 * i == torch.arange(32, device=q.device)[None, :]).float()
        pd = FA.forward(zero_q, k, onehot.expand(B, H, Lk, 32).contiguous(), scale, p, seed, key_padding_mask=key_padding_mask)[0]
        cols.append(pd != 0)
    return torch.cat(cols, -1)[..., :Lk]
