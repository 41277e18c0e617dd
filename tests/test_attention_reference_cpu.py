"""tests/attention_reference.py on the CPU: every input regime really is what its name says (asserted from the float64
evaluation, at the first shape test_attention_core_gpu.py uses), the reference is finite in float32 and float64, and its
dropout path equals a hand-written einsum evaluation -- so that the helper itself is not the bug."""
import math

import pytest
import torch

import attention_reference as AR

SHAPE = (2, 3, 130, 200)


def _case(name):
    return AR.make_case(name, *SHAPE, torch.Generator().manual_seed(7))


def _probs(q, k, scale):
    s = (q.double() @ k.double().transpose(-1, -2)) * scale
    return s, torch.softmax(s, -1)


def _tile_maxima(s):
    """[B, H, Lq, ceil(Lk / 64)]: the row maximum inside each 64-key tile of the kernels"""
    return torch.stack([t.amax(-1) for t in s.split(64, -1)], -1)


@pytest.mark.parametrize("name", AR.REGIMES)
def test_reference_is_finite_in_float32_and_float64(name):
    q, k, v, go, scale = _case(name)
    for dtype in (torch.float32, torch.float64):
        out = AR.reference(q, k, v, go, scale, dtype=dtype)
        assert len(out) == 5
        for x in out:
            assert x.dtype == dtype and torch.isfinite(x).all()
    for t in (q, k, v, go):
        assert t.dtype == torch.float32 and t.shape[:2] == SHAPE[:2] and t.shape[3] == 32


def test_sharp_rows_are_peaked_and_logits_large():
    q, k, _, _, scale = _case("sharp")
    s, p = _probs(q, k, scale)
    assert p.amax(-1).mean().item() >= 0.8
    assert s.abs().max().item() >= 50


def test_offset_logits_are_large():
    q, k, _, _, scale = _case("offset")
    assert _probs(q, k, scale)[0].abs().max().item() >= 50


def test_ascending_rows_raise_the_maximum_at_every_key_tile():
    assert SHAPE[3] >= 129
    q, k, _, _, scale = _case("ascending")
    tm = _tile_maxima(_probs(q, k, scale)[0])
    rising = (tm[..., 1:] > tm[..., :-1]).all(-1)
    assert rising.double().mean().item() >= 0.5


def test_descending_rows_never_raise_the_maximum():
    q, k, _, _, scale = _case("descending")
    tm = _tile_maxima(_probs(q, k, scale)[0])
    assert (tm[..., 1:] < tm[..., :-1]).all()


@pytest.mark.parametrize("name,key", [("late_spike", -1), ("early_spike", 0)])
def test_spike_key_dominates_every_row_and_leaves_gradients(name, key):
    q, k, v, go, scale = _case(name)
    assert (_probs(q, k, scale)[1][..., key] >= 0.9).all()
    _, dq, dk, _, _ = AR.reference(q, k, v, go, scale)
    assert dq.abs().max().item() >= 1e-3 and dk.abs().max().item() >= 1e-3


def test_scale_zero_is_the_key_mean_with_zero_gradients():
    q, k, v, go, scale = _case("scale_zero")
    assert scale == 0.0
    o, dq, dk, dv, lse = AR.reference(q, k, v, go, scale)
    assert (o - v.double().mean(2, keepdim=True)).abs().max().item() <= 1e-14
    assert (dq == 0).all() and (dk == 0).all()
    assert (lse - torch.log(torch.tensor(float(SHAPE[3]), dtype=torch.float64))).abs().max().item() <= 1e-14


def test_scales_of_the_scale_regimes():
    assert _case("scale_one")[4] == 1.0 and _case("scale_negative")[4] == -0.3
    assert _case("randn")[4] == 1.0 / math.sqrt(32)
    with pytest.raises(ValueError):
        _case("no_such_regime")


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "keypad"])
def test_reference_with_a_keep_mask_equals_a_hand_written_einsum_evaluation(masked):
    """o, dq, dk, dv and lse of reference(keep=..., keep_scale=...) against the closed-form backward of dropout(softmax) V written
    with einsum -- no autograd, no softmax / logsumexp call."""
    g = torch.Generator().manual_seed(11)
    B, H, Lq, Lk = 2, 3, 37, 70
    q, k, v, go, _ = AR.make_case("randn", B, H, Lq, Lk, g)
    scale, keep_scale = 0.37, 65536.0 / (65536.0 - 19661)
    keep = torch.rand(B, H, Lq, Lk, generator=g) >= 0.3
    kpm = None
    if masked:
        kpm = torch.zeros(B, Lk, dtype=torch.bool)
        kpm[0, 60:] = True
        kpm[1, ::5] = True
    o, dq, dk, dv, lse = AR.reference(q, k, v, go, scale, key_padding_mask=kpm, keep=keep, keep_scale=keep_scale)
    qd, kd, vd, gd = (t.double() for t in (q, k, v, go))
    s = torch.einsum("bhqd,bhkd->bhqk", qd, kd) * scale
    e = torch.exp(s - s.amax(-1, keepdim=True))
    if kpm is not None:
        e = e * (~kpm)[:, None, None, :]
    z = e.sum(-1, keepdim=True)
    p = e / z
    m = keep.double() * keep_scale
    want_o = torch.einsum("bhqk,bhkd->bhqd", p * m, vd)
    want_dv = torch.einsum("bhqk,bhqd->bhkd", p * m, gd)
    dp = torch.einsum("bhqd,bhkd->bhqk", gd, vd) * m
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    want_dq = torch.einsum("bhqk,bhkd->bhqd", ds, kd) * scale
    want_dk = torch.einsum("bhqk,bhqd->bhkd", ds, qd) * scale
    want_lse = s.amax(-1) + torch.log(z[..., 0])
    for name, a, b in (("o", o, want_o), ("dq", dq, want_dq), ("dk", dk, want_dk), ("dv", dv, want_dv), ("lse", lse, want_lse)):
        assert (a - b).abs().max().item() <= 1e-12 * max(b.abs().max().item(), 1.0), name
    if kpm is not None:
        dead = kpm[:, None, :, None].expand_as(dk)
        assert (dk[dead] == 0).all() and (dv[dead] == 0).all()
