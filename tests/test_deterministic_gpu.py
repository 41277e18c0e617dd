"""Deterministic mode (torch.use_deterministic_algorithms) on the GPU: the native backward kernels give bitwise-identical
gradients run after run -- also with another kernel running beside them; a path without a deterministic variant refuses to
run.  That they still meet the f64-oracle tolerances that tests/test_msda_gpu.py applies to the default kernels is checked here on
one sample per case only: tests/test_deterministic_parity_gpu.py holds that claim, for every kernel the mode selects."""
import warnings

import numpy as np
import pytest
import torch

from oracle import msda_oracle as O

pytestmark = pytest.mark.gpu

KITTI_LEVELS = [(48, 160), (24, 80), (12, 40), (6, 20)]
RUNS = 5


@pytest.fixture
def deterministic():
    """torch's global flag on for the test, restored afterwards (warn_only included)."""
    was, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn_only)


def _msda():
    from monosowa_amd import MultiScaleDeformableAttention as MSDA
    MSDA.install()
    return MSDA


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(got, want, rel, what):
    got = got.detach().cpu().numpy().reshape(want.shape)
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max()) / scale
    assert err <= rel, "%s: max err / max|ref| = %.3e > %.1e" % (what, err, rel)


def _repeat(fn, side_load):
    """fn() RUNS times; every other run with a matrix product looping on a side stream (another kernel sharing the GPU)."""
    outs = []
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device="cuda")
    for r in range(RUNS):
        if side_load and r % 2:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(8):
                    a = a @ a * 1e-3
        outs.append([t.clone() for t in fn()])
    torch.cuda.synchronize()
    return outs


def _assert_all_equal(outs, names):
    for r in range(1, len(outs)):
        for k, name in enumerate(names):
            assert torch.equal(outs[0][k], outs[r][k]), "%s differs between run 0 and run %d" % (name, r)


def _encoder_case(B, seed, kind):
    rng = np.random.default_rng(seed)
    shapes = np.array(KITTI_LEVELS, dtype=np.int64)
    lsi = O.level_start_index(shapes)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    M, L, P = 8, 4, 4
    ref = np.concatenate([np.stack(np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h), -1).reshape(-1, 2)
                          for h, w in KITTI_LEVELS]).astype(np.float32)
    if kind == "initial":          # the module's initial pattern: point p of head m at (p + 1) px along the head's direction
        th = np.arange(M) * (2 * np.pi / M)
        grid = np.stack([np.cos(th), np.sin(th)], -1)
        grid = grid / np.abs(grid).max(-1, keepdims=True)
        off = grid[:, None, None, :] * (np.arange(P) + 1)[None, None, :, None]              # [M, 1, P, 2]
        offsets = np.broadcast_to(off[None, None], (B, S, M, L, P, 2)).astype(np.float32).copy()
    elif kind == "sigma8":         # trained-like offsets: N(0, 8 px), many points beyond any scan bound
        offsets = rng.normal(0.0, 8.0, (B, S, M, L, P, 2)).astype(np.float32)
    else:                          # pile-up: every point pulled onto a handful of pixels (hundreds of points per cell)
        targets = rng.uniform(0.2, 0.8, (4, 2)).astype(np.float32)
        pick = targets[rng.integers(0, 4, (S,))]
        d = pick - ref                                                                         # [S, 2] in [0, 1] units
        wh = np.array([[w, h] for h, w in KITTI_LEVELS], dtype=np.float32)                    # [L, 2]
        offsets = np.broadcast_to((d[:, None, None, :] * wh[:, None, :])[None, :, None], (B, S, M, L, P, 2)).astype(np.float32).copy()
        offsets += rng.uniform(-0.3, 0.3, offsets.shape).astype(np.float32)
    logits = rng.standard_normal((B, S, M, L * P)).astype(np.float32)
    value = rng.standard_normal((B, S, M, 32)).astype(np.float32)
    go = rng.standard_normal((B, S, M * 32)).astype(np.float32)
    return shapes, lsi, ref, offsets, logits, value, go


@pytest.mark.parametrize("kind", ["initial", "sigma8", "pileup"])
def test_encoder_fused_backward_is_bitwise_reproducible(deterministic, kind):
    """The encoder's operator (merged [B, S, 384] projection, KITTI pyramid, B = 16): grad_value, grad_offsets and
    grad_logits are bit-identical over 5 runs, with and without a concurrent kernel, and match the C oracle."""
    MSDA = _msda()
    B = 16
    shapes, lsi, ref, offsets, logits, value, go = _encoder_case(B, 7, kind)
    S, M = value.shape[1], value.shape[2]
    s, i = _dev(shapes), _dev(lsi)
    MSDA.attach_host_geometry(s, i, shapes.tolist(), lsi.tolist())
    proj = torch.cat([_dev(offsets).reshape(B, S, M * 32), _dev(logits).reshape(B, S, M * 16)], -1).contiguous()
    refp = _dev(np.broadcast_to(ref[None, :, None, :], (B, S, 4, 2)).copy())
    v, g = _dev(value), _dev(go)
    assert not MSDA.fused_save_supported(v, s, i, S)            # the saved prologue runs the row-tile scatter: off in this mode

    def once():
        gv, gproj = MSDA.ms_deform_attn_fused_backward_merged(v, s, i, proj, refp, g)
        return gv, gproj[..., :M * 32], gproj[..., M * 32:]

    for side_load in (False, True):
        outs = _repeat(once, side_load)
        _assert_all_equal(outs, ["grad_value", "grad_offsets", "grad_logits"])
    gv, g_off_got, g_log_got = outs[0]

    # one sample against the oracle, as test_msda_gpu.py checks the default kernels
    b = 3
    off_t = _dev(offsets[b:b + 1]).requires_grad_(True)
    log_t = _dev(logits[b:b + 1]).requires_grad_(True)
    norm = torch.stack([s[:, 1], s[:, 0]], -1).float()
    loc_t = refp[b:b + 1, :, None, :, None, :] + off_t / norm[None, None, None, :, None, :]
    aw_t = torch.softmax(log_t, -1).view(1, S, M, 4, 4)
    loc_b, aw_b = loc_t.detach().cpu().numpy(), aw_t.detach().cpu().numpy()
    want = O.backward(value[b:b + 1], shapes, lsi, loc_b, aw_b, go[b:b + 1])
    _close(gv[b:b + 1], want[0], 1e-4, "grad_value[%d]" % b)
    g_off, g_log = torch.autograd.grad([loc_t, aw_t], [off_t, log_t], [torch.from_numpy(want[1]).cuda(), torch.from_numpy(want[2]).cuda()])
    assert (g_off_got[b].reshape(g_off.shape) - g_off).abs().max() <= 1e-4 * g_off.abs().max(), "grad_offsets"
    assert (g_log_got[b].reshape(g_log.shape) - g_log).abs().max() <= 1e-4 * g_log.abs().max(), "grad_logits"


@pytest.mark.parametrize("Lq", [550, 50])
def test_decoder_backward_is_bitwise_reproducible(deterministic, Lq):
    """The decoder's cross-attention shape (Lq = 550 / 50 queries on the KITTI pyramid, B = 16): all three gradients
    bit-identical over 5 runs, with and without a concurrent kernel, and within the oracle tolerances."""
    MSDA = _msda()
    B, M, D, L, P = 16, 8, 32, 4, 4
    rng = np.random.default_rng(Lq)
    shapes = np.array(KITTI_LEVELS, dtype=np.int64)
    lsi = O.level_start_index(shapes)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    value = rng.standard_normal((B, S, M, D)).astype(np.float32)
    loc = rng.uniform(-0.05, 1.05, (B, Lq, M, L, P, 2)).astype(np.float32)
    w = rng.uniform(0, 1, (B, Lq, M, L, P)).astype(np.float32)
    go = rng.standard_normal((B, Lq, M * D)).astype(np.float32)
    s, i = _dev(shapes), _dev(lsi)
    MSDA.attach_host_geometry(s, i, shapes.tolist(), lsi.tolist())
    v, l_, w_, g = _dev(value), _dev(loc), _dev(w), _dev(go)

    def once():
        return MSDA.ms_deform_attn_backward(v, s, i, l_, w_, g, 64)

    for side_load in (False, True):
        outs = _repeat(once, side_load)
        _assert_all_equal(outs, ["grad_value", "grad_loc", "grad_attn_w"])
    b = 5
    d = lambda a: a.astype(np.float64)
    want = O.backward(d(value[b:b + 1]), shapes, lsi, d(loc[b:b + 1]), d(w[b:b + 1]), d(go[b:b + 1]))
    _close(outs[0][0][b:b + 1], want[0], 1e-4, "grad_value")
    _close(outs[0][2][b:b + 1], want[2], 1e-4, "grad_attn_w")
    # grad_loc jumps across pixel borders: against the f32 oracle (the kernel's own floor() decisions), as test_msda_gpu.py does
    want32 = O.backward(value[b:b + 1], shapes, lsi, loc[b:b + 1], w[b:b + 1], go[b:b + 1])
    _close(outs[0][1][b:b + 1], want32[1], 1e-4, "grad_loc")


def test_generic_f64_backward_refuses_or_warns(deterministic):
    """Contract: a native path without a deterministic variant never runs silently -- RuntimeError naming the op, or one
    warning per op under warn_only (and the op runs)."""
    MSDA = _msda()
    B, S, M, D, Lq, L, P = 1, 12, 2, 8, 3, 1, 2
    shapes = torch.tensor([[3, 4]], dtype=torch.int64, device="cuda")
    lsi = torch.tensor([0], dtype=torch.int64, device="cuda")
    value = torch.randn(B, S, M, D, dtype=torch.float64, device="cuda")
    loc = torch.rand(B, Lq, M, L, P, 2, dtype=torch.float64, device="cuda")
    w = torch.rand(B, Lq, M, L, P, dtype=torch.float64, device="cuda")
    go = torch.randn(B, Lq, M * D, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="ms_deform_attn_backward.*deterministic"):
        MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, w, go, 64)
    torch.use_deterministic_algorithms(True, warn_only=True)
    from monosowa_amd import _lib
    _lib._ALERTED.discard("ms_deform_attn_backward")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        g1 = MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, w, go, 64)
        MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, w, go, 64)
    hits = [r for r in rec if "ms_deform_attn_backward" in str(r.message)]
    assert len(hits) == 1, [str(r.message) for r in rec]
    assert torch.isfinite(g1[0]).all()


def _gn_inputs(relu, seed):
    torch.manual_seed(seed)
    gn = torch.nn.GroupNorm(32, 256).cuda()
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.uniform_(-0.2, 0.2)
    x = torch.randn(16, 256, 48, 160, device="cuda").contiguous(memory_format=torch.channels_last) * 3 + 1
    pre_bias = torch.randn(256, device="cuda", requires_grad=True)
    gy = torch.randn_like(x)
    return gn, x.requires_grad_(True), pre_bias, gy


@pytest.mark.parametrize("relu", [False, True])
def test_groupnorm_is_bitwise_reproducible(deterministic, relu):
    """GroupNorm(32, 256) on the depth predictor's 48 x 160 maps: forward and every gradient bit-identical over 5 runs and
    equal to the default mode's results up to f64-statistics rounding (and to PyTorch's GroupNorm)."""
    from monosowa_amd import pointwise
    gn, x, pre_bias, gy = _gn_inputs(relu, 3)

    def once():
        y = pointwise.group_norm(x, gn, relu=relu, pre_bias=pre_bias)
        gx, gb, gw, gbeta = torch.autograd.grad(y, [x, pre_bias, gn.weight, gn.bias], gy)
        return y, gx, gb, gw, gbeta

    for side_load in (False, True):
        outs = _repeat(once, side_load)
        _assert_all_equal(outs, ["y", "grad_x", "grad_pre_bias", "grad_weight", "grad_bias"])
    torch.use_deterministic_algorithms(False)
    default = once()
    for got, want, name in zip(outs[0], default, ["y", "grad_x", "grad_pre_bias", "grad_weight", "grad_bias"]):
        assert (got - want).abs().max() <= 1e-5 * want.abs().max(), name
    # the raw f64 statistics / parameter-gradient partials: the deterministic launch stores every element (a NaN-filled buffer
    # comes back finite; the default kernels would add into the NaNs) and gives the same bits every run
    from monosowa_amd._lib import raw_stream
    lib = pointwise.load()
    torch.use_deterministic_algorithms(True)
    assert pointwise.DETERMINISTIC.sync()
    B, C, H, W = x.shape
    xd = x.detach()
    mean_rstd = torch.empty(B, 32, 2, device="cuda")
    y = torch.empty_like(xd)
    n_stats, n_part = lib.mono_groupnorm_stats_doubles(B, H * W), lib.mono_groupnorm_part_doubles(B, H * W)
    assert n_stats == (B + lib.mono_groupnorm_blocks(B, H * W)) * 64
    raw = []
    for _ in range(3):
        stats = torch.full((n_stats,), float("nan"), dtype=torch.float64, device="cuda")
        part = torch.full((n_part,), float("nan"), dtype=torch.float64, device="cuda")
        assert lib.mono_groupnorm_nhwc_fwd_f32(xd.data_ptr(), pre_bias.data_ptr(), gn.weight.data_ptr(), gn.bias.data_ptr(), y.data_ptr(),
                                               stats.data_ptr(), mean_rstd.data_ptr(), B, H * W, C, 32, float(gn.eps), int(relu), raw_stream()) == 0
        gx, gbias = torch.empty_like(xd), torch.empty(C, device="cuda")
        partials = torch.empty(lib.mono_groupnorm_blocks(B, H * W) * C, device="cuda")
        gwb = torch.empty(2, C, device="cuda")
        assert lib.mono_groupnorm_nhwc_bwd_f32(gy.data_ptr(), xd.data_ptr(), pre_bias.data_ptr(), y.data_ptr() if relu else None,
                                               mean_rstd.data_ptr(), gn.weight.data_ptr(), gx.data_ptr(), part.data_ptr(), gbias.data_ptr(),
                                               partials.data_ptr(), gwb.data_ptr(), B, H * W, C, 32, int(relu), raw_stream()) == 0
        torch.cuda.synchronize()
        raw.append((stats[:B * 64].clone(), part[:B * 512].clone()))
    for stats, part in raw:
        assert torch.isfinite(stats).all() and torch.isfinite(part).all()
        assert torch.equal(stats, raw[0][0]) and torch.equal(part, raw[0][1])
    xr = x.detach().clone().requires_grad_(True)
    ref = gn(xr + pre_bias.detach().view(1, -1, 1, 1))
    ref = torch.relu(ref) if relu else ref
    assert (outs[0][0] - ref).abs().max() <= 1e-4 * ref.abs().max()


def test_head_tail_is_bitwise_reproducible(deterministic):
    """The detection heads' tail (depth map 48 x 160, 550 queries, B = 16), queries piled onto a few map cells: the depth-map
    gradient and every other gradient bit-identical over 5 runs, and equal to the default (atomic) kernel's within rounding."""
    from monosowa_amd import pointwise
    torch.manual_seed(11)
    B, Q, H, W = 16, 550, 48, 160
    tmp = torch.randn(B, Q, 6, device="cuda")
    tmp[..., :2] = torch.randn(B, Q, 2, device="cuda") * 0.05 + torch.tensor([0.3, -0.2], device="cuda")   # piled-up centres
    tmp.requires_grad_(True)
    size3d = torch.rand(B, Q, 3, device="cuda", requires_grad=True)
    depth_reg = torch.randn(B, Q, 2, device="cuda", requires_grad=True)
    wdepth = (torch.rand(B, H, W, device="cuda") * 40).requires_grad_(True)
    fu = torch.full((B,), 720.0, device="cuda")
    img_h = torch.full((B,), 384.0, device="cuda")
    g_coords = torch.randn(B, Q, 6, device="cuda")
    g_dave = torch.randn(B, Q, 2, device="cuda")
    assert pointwise.head_tail_supported(tmp, size3d, depth_reg, wdepth, fu, img_h)

    def once():
        coords, dave = pointwise._HeadTail.apply(tmp, size3d, depth_reg, wdepth, fu, img_h, None)
        return (coords, dave) + torch.autograd.grad([coords, dave], [tmp, size3d, depth_reg, wdepth], [g_coords, g_dave])

    names = ["coords", "depth_ave", "grad_tmp", "grad_size3d", "grad_depth_reg", "grad_wdepth"]
    for side_load in (False, True):
        outs = _repeat(once, side_load)
        _assert_all_equal(outs, names)
    torch.use_deterministic_algorithms(False)
    default = once()
    for got, want, name in zip(outs[0], default, names):
        assert (got - want).abs().max() <= 1e-5 * max(float(want.detach().abs().max()), 1e-30), name
    assert outs[0][5].abs().sum() > 0
