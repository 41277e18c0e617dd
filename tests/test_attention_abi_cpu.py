"""The refusals of the attention C ABI (include/monosowa_attn.h): mono_attn_forward_keep_f32 and mono_attn_backward_keep_f32
return MONO_ATTN_E_NULLPTR (-1) / MONO_ATTN_E_SHAPE (-2) before any HIP call, so they are exercised on host buffers.

Only where NO GPU is present: should one of these checks ever be lost, the call must not become a kernel launch on made-up
pointers on a shared machine.  Without a device it comes back as a HIP error code in place of -2 and the test fails cleanly."""
import ctypes

import pytest
import torch

from monosowa_amd import flash_attn as FA

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="refusals are only provoked where no GPU could run the kernels")

E_NULLPTR, E_SHAPE = -1, -2
B, H, LQ, LK = 2, 3, 5, 7
_BUFFERS = []                                   # keeps the host memory behind the pointers alive


def _aligned(n_bytes):
    raw = ctypes.create_string_buffer(n_bytes + 16)
    _BUFFERS.append(raw)
    addr = (ctypes.addressof(raw) + 15) & ~15
    assert addr % 16 == 0
    return addr


def _dense(L):
    return FA._Strides(H * L * 32, L * 32, 32)


def _forward_args():
    """a call that passes every check of mono_attn_forward_keep_f32 (names -> values, in the ABI's order)"""
    n_q, n_k = B * H * LQ * 32 * 4, B * H * LK * 32 * 4
    return dict(q=_aligned(n_q), k=_aligned(n_k), v=_aligned(n_k), mask=None, keep=None, o=_aligned(n_q), lse=_aligned(B * H * LQ * 4),
                B=B, H=H, Lq=LQ, Lk=LK, head_dim=32, sq=_dense(LQ), sk=_dense(LK), sv=_dense(LK), so=_dense(LQ),
                scale=0.125, p=0.0, seed=1, stream=None)


def _backward_args():
    n_q, n_k = B * H * LQ * 32 * 4, B * H * LK * 32 * 4
    return dict(q=_aligned(n_q), k=_aligned(n_k), v=_aligned(n_k), mask=None, keep=None, o=_aligned(n_q), lse=_aligned(B * H * LQ * 4),
                dout=_aligned(n_q), dq=_aligned(n_q), dk=_aligned(n_k), dv=_aligned(n_k), delta=_aligned(B * H * LQ * 4),
                B=B, H=H, Lq=LQ, Lk=LK, head_dim=32, sq=_dense(LQ), sk=_dense(LK), sv=_dense(LK), so=_dense(LQ),
                sdq=_dense(LQ), sdk=_dense(LK), sdv=_dense(LK), scale=0.125, p=0.0, seed=1, stream=None)


ENTRIES = {"forward": ("mono_attn_forward_keep_f32", _forward_args, ("q", "k", "v", "o", "lse"), ("q", "k", "v", "o"),
                       (("q", "sq"), ("k", "sk"), ("v", "sv"), ("o", "so"))),
           "backward": ("mono_attn_backward_keep_f32", _backward_args,
                        ("q", "k", "v", "o", "lse", "dout", "dq", "dk", "dv", "delta"), ("q", "k", "v", "o", "dout", "dq", "dk", "dv"),
                        (("q", "sq"), ("k", "sk"), ("v", "sv"), ("o", "so"), ("dq", "sdq"), ("dk", "sdk"), ("dv", "sdv")))}


def _call(entry, **changes):
    symbol, make = ENTRIES[entry][:2]
    args = make()
    for name, value in changes.items():
        assert name in args
        args[name] = value
    return getattr(FA.load(), symbol)(*args.values())


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_required_pointers_are_refused(entry):
    for name in ENTRIES[entry][2]:
        assert _call(entry, **{name: None}) == E_NULLPTR, name


@pytest.mark.parametrize("entry", ENTRIES)
def test_shapes_and_dropout_rates_out_of_range_are_refused(entry):
    for head_dim in (0, 16, 31, 33, 64):
        assert _call(entry, head_dim=head_dim) == E_SHAPE, head_dim
    for name in ("B", "H", "Lq", "Lk"):
        for value in (0, -1):
            assert _call(entry, **{name: value}) == E_SHAPE, (name, value)
    for p in (-0.1, 1.0, float("nan")):
        assert _call(entry, p=p) == E_SHAPE, p
    # the planes are the grid's y dimension: 65535 at the most
    assert _call(entry, B=256, H=256) == E_SHAPE
    assert _call(entry, B=1, H=65536) == E_SHAPE


@pytest.mark.parametrize("entry", ENTRIES)
def test_pointers_and_strides_that_break_the_16_byte_loads_are_refused(entry):
    base = ENTRIES[entry][1]()
    for name in ENTRIES[entry][3]:
        assert _call(entry, **{name: base[name] + 4}) == E_SHAPE, name
    for name, strides in ENTRIES[entry][4]:
        L = LQ if name in ("q", "o", "dq") else LK
        for field in ("batch", "head", "token"):
            for off in (1, 2, 3):
                s = _dense(L)
                setattr(s, field, getattr(s, field) + off)
                assert _call(entry, **{strides: s}) == E_SHAPE, (name, field, off)


def test_keep_words():
    words = FA.load().mono_attn_keep_words
    for shape in ((0, 3, 5, 7), (2, 0, 5, 7), (2, 3, 0, 7), (2, 3, 5, 0), (-1, 3, 5, 7), (2, -3, 5, 7), (2, 3, -5, 7), (2, 3, 5, -7),
                  (-2, -3, 5, 7)):
        assert words(*shape) == 0, shape
    ceil = lambda a, b: -(-a // b)
    for b, h, lq, lk in ((1, 1, 1, 1), (2, 3, 5, 7), (2, 3, 128, 64), (2, 3, 129, 65), (1, 8, 1920, 1920), (16, 8, 550, 1920),
                         (255, 257, 4000, 4000)):
        assert words(b, h, lq, lk) == b * h * ceil(lq, 128) * ceil(lk, 64) * 256, (b, h, lq, lk)
    assert words(255, 257, 4000, 4000) > 2 ** 31
