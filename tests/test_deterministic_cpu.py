"""Deterministic mode (torch.use_deterministic_algorithms) at the C ABI and in the configuration: the switches exist, are
declared, validate their arguments and change nothing else (no GPU needed: none of these calls launches a kernel)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def msda_lib():
    from monosowa_amd import _lib
    lib = _lib.load()
    yield lib
    lib.msda_set_option(b"deterministic", 0)
    _lib.MSDA_DETERMINISTIC._on = False


@pytest.fixture
def torch_flag():
    was, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn_only)


def _declared(header, name):
    with open(os.path.join(ROOT, "include", header)) as f:
        return re.search(r"\b%s\s*\(" % name, f.read()) is not None


def test_msda_deterministic_option_validates_and_changes_the_stamp(msda_lib):
    from monosowa_amd import _lib
    assert msda_lib.msda_abi_version() == _lib.ABI_VERSION == 11
    stamp = msda_lib.msda_options_stamp()
    assert msda_lib.msda_set_option(b"deterministic", 1) == 0
    assert msda_lib.msda_options_stamp() != stamp
    assert msda_lib.msda_set_option(b"deterministic", 2) == -3          # MSDA_E_UNSUPPORTED
    assert msda_lib.msda_set_option(b"deterministic", -1) == -3
    assert msda_lib.msda_set_option(b"deterministic", 0) == 0
    assert msda_lib.msda_options_stamp() == stamp


def test_msda_workspace_size_is_the_default_modes(msda_lib):
    # encoder (Lq == S) and decoder shapes at B = 16 on the KITTI pyramid, f32 and f64
    shapes = [(16, 10200, 8, 32, 4, 10200, 4, 4), (16, 10200, 8, 32, 4, 550, 4, 4), (16, 10200, 8, 32, 4, 50, 4, 4),
              (2, 100, 2, 8, 1, 3, 2, 8)]
    default = [msda_lib.msda_backward_workspace_bytes(*s) for s in shapes]
    assert default[0] > 0
    assert msda_lib.msda_set_option(b"deterministic", 1) == 0
    assert [msda_lib.msda_backward_workspace_bytes(*s) for s in shapes] == default


def test_msda_save_supported_is_off_in_deterministic_mode(msda_lib):
    sh = (ctypes.c_int64 * 8)(48, 160, 24, 80, 12, 40, 6, 20)
    ls = (ctypes.c_int64 * 4)(0, 7680, 9600, 10080)
    args = (10200, 8, 32, 4, 10200, 4, 2, 256, 384, 384, ctypes.cast(sh, ctypes.c_void_p), ctypes.cast(ls, ctypes.c_void_p))
    on_default = msda_lib.msda_fused_save_supported_view(*args)
    assert msda_lib.msda_set_option(b"deterministic", 1) == 0
    assert msda_lib.msda_fused_save_supported_view(*args) == 0
    assert msda_lib.msda_set_option(b"deterministic", 0) == 0
    assert msda_lib.msda_fused_save_supported_view(*args) == on_default


def test_python_switch_follows_torchs_flag(msda_lib, torch_flag):
    from monosowa_amd import _lib
    stamp = msda_lib.msda_options_stamp()
    torch.use_deterministic_algorithms(True)
    assert _lib.MSDA_DETERMINISTIC.sync() is True
    assert msda_lib.msda_options_stamp() != stamp
    torch.use_deterministic_algorithms(False)
    assert _lib.MSDA_DETERMINISTIC.sync() is False
    assert msda_lib.msda_options_stamp() == stamp


def test_alert_raises_or_warns_once(torch_flag):
    from monosowa_amd import _lib
    _lib.alert_not_deterministic("some_op", "reason")                # mode off: nothing
    torch.use_deterministic_algorithms(True)
    with pytest.raises(RuntimeError, match="some_op does not have a deterministic implementation \\(reason\\)"):
        _lib.alert_not_deterministic("some_op", "reason")
    torch.use_deterministic_algorithms(True, warn_only=True)
    _lib._ALERTED.discard("some_op")
    with pytest.warns(UserWarning, match="some_op") as rec:
        _lib.alert_not_deterministic("some_op", "reason")
        _lib.alert_not_deterministic("some_op", "reason")
    assert len([r for r in rec if "some_op" in str(r.message)]) == 1


def test_pointwise_switch_exists_and_is_declared():
    from monosowa_amd import pointwise
    for name in ("mono_set_deterministic", "mono_groupnorm_stats_doubles", "mono_groupnorm_part_doubles"):
        assert name in pointwise.SYMBOLS and _declared("monosowa_pointwise.h", name)
    lib = pointwise.load()
    B, HW = 16, 48 * 160
    blocks = lib.mono_groupnorm_blocks(B, HW)
    assert lib.mono_set_deterministic(0) == 0
    assert lib.mono_groupnorm_stats_doubles(B, HW) == B * 64          # the default mode's buffers are unchanged
    assert lib.mono_groupnorm_part_doubles(B, HW) == B * 512
    assert lib.mono_set_deterministic(1) == 0
    try:
        assert lib.mono_groupnorm_stats_doubles(B, HW) == (B + blocks) * 64
        assert lib.mono_groupnorm_part_doubles(B, HW) == (B + blocks) * 512
    finally:
        assert lib.mono_set_deterministic(0) == 1
        pointwise.DETERMINISTIC._on = False


def test_gemm_switch_exists_and_is_declared():
    from monosowa_amd import gemm_lt
    assert "mono_gemm_set_deterministic" in gemm_lt.SYMBOLS and _declared("monosowa_gemm.h", "mono_gemm_set_deterministic")
    lib = gemm_lt.load()
    assert lib.mono_gemm_set_deterministic(1) == 0
    assert lib.mono_gemm_set_deterministic(0) == 1
    gemm_lt.DETERMINISTIC._on = False


def test_trainer_deterministic_key_reaches_torch(torch_flag, monkeypatch):
    import yaml
    from monosowa_amd.helpers.utils_helper import set_deterministic
    with open(os.path.join(ROOT, "configs", "monodetr.yaml")) as f:
        cfg = yaml.load(f, Loader=yaml.Loader)
    assert "deterministic" not in cfg["trainer"]                      # the shipped config is unchanged: the key is optional
    calls = []
    monkeypatch.setattr(torch, "use_deterministic_algorithms", lambda mode, **kw: calls.append(mode))
    assert set_deterministic(cfg["trainer"]) is False and calls == []
    assert set_deterministic(dict(cfg["trainer"], deterministic=False)) is False and calls == []
    monkeypatch.setenv("CUBLAS_WORKSPACE_CONFIG", "")               # (recorded, so that the teardown restores the session's value)
    monkeypatch.delenv("CUBLAS_WORKSPACE_CONFIG")
    assert set_deterministic(dict(cfg["trainer"], deterministic=True)) is True
    assert calls == [True]
    assert os.environ["CUBLAS_WORKSPACE_CONFIG"] == ":4096:8"
    with open(os.path.join(ROOT, "tools", "train_val.py")) as f:
        assert 'set_deterministic(cfg.get("trainer"))' in f.read()


# 4 x the plain float32 F.interpolate's own error against float64 on the CPU over exactly these sizes (forward 9.4e-7, gradient
# 8.9e-7, worst at (5, 17) -> (9, 33)), rounded up; the matrix-product form measured 9.5e-7 / 9.1e-7
BOUND_UPSAMPLE = 4e-6
UPSAMPLE_SIZES = [((6, 20), (12, 40)), ((5, 17), (9, 33)), ((3, 9), (5, 17)), ((12, 40), (24, 80)), ((12, 44), (24, 88)),
                  ((1, 1), (2, 3)), ((7, 9), (7, 9))]


@pytest.mark.parametrize("src,dst", UPSAMPLE_SIZES)
def test_upsample_bilinear_as_matrix_products_equals_float64_interpolate(torch_flag, src, dst):
    """depth_predictor.upsample_bilinear under the flag with a gradient wanted (two matrix products with the separable weights):
    forward and input gradient against F.interpolate(mode="bilinear") in float64; the output is channels-last."""
    import torch.nn.functional as F
    from monosowa_amd.monodetr.depth_predictor import upsample_bilinear
    torch.manual_seed(src[0] * 100 + dst[1])
    x = torch.randn(2, 256, *src)
    gy = torch.randn(2, 256, *dst)
    xr = x.double().requires_grad_(True)
    ref = F.interpolate(xr, size=dst, mode="bilinear")
    g_ref, = torch.autograd.grad(ref, xr, gy.double())
    torch.use_deterministic_algorithms(True)
    xd = x.clone().requires_grad_(True)
    y = upsample_bilinear(xd, dst)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    assert y.grad_fn is not None and "Upsample" not in type(y.grad_fn).__name__          # the matrix-product form did run
    g, = torch.autograd.grad(y, xd, gy)
    for name, got, want in (("forward", y, ref), ("grad_input", g, g_ref)):
        err = ((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30)).item()
        print("upsample_bilinear %s -> %s %s: e_D = %.2e" % (src, dst, name, err))
        assert err <= BOUND_UPSAMPLE, (name, err)
    # without a gradient wanted, or with the flag off, the function is F.interpolate itself
    assert torch.equal(upsample_bilinear(x, dst), F.interpolate(x, size=dst, mode="bilinear"))
    torch.use_deterministic_algorithms(False)
    assert torch.equal(upsample_bilinear(xd, dst), F.interpolate(xd, size=dst, mode="bilinear"))
