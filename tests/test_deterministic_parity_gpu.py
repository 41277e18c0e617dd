"""Deterministic mode (torch.use_deterministic_algorithms): the VALUES of every kernel the mode selects, against float64.

tests/test_deterministic_gpu.py and tests/test_deterministic_step_gpu.py pin the mode's bits (the same result run after run);
this module pins what those bits are worth.  Every case runs the operator twice under the flag, asserts bit identity of the two
results, then compares the first with a reference that shares no code with the kernels:
  MSDA backward      oracle/msda_oracle (C, float64; float32 for the two outputs that jump across pixel borders), fed with the
                     PyTorch prologue for the fused operator -- rule and tolerance of tests/test_msda_gpu.py
  GroupNorm          torch.nn.GroupNorm in float64 -- rule of test_groupnorm_nhwc_matches_torch
  head tail          the plain expression of monodetr.py in float64 on the GPU -- bounds measured from plain float32
  upsample_bilinear  F.interpolate in float64 -- bound of tests/test_deterministic_cpu.py
  hipBLASLt shim     the comparisons and bounds of tests/test_gemm_lt_gpu.py
Every case asserts that the deterministic path is the one that ran."""
import os
import re
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import msda_oracle as O
from test_deterministic_cpu import BOUND_UPSAMPLE, UPSAMPLE_SIZES      # (4e-6; its derivation is there)
from test_deterministic_gpu import _encoder_case
from test_msda_gpu import _close, _dev, _oracle_want, _random_case
import test_gemm_lt_gpu as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KITTI_LEVELS = [(48, 160), (24, 80), (12, 40), (6, 20)]
SMALL_LEVELS = [(12, 40), (6, 20), (3, 10), (2, 5)]
VIEW_LEVELS = [(24, 40), (12, 20), (6, 10), (3, 5)]
# name -> (levels, batch, samples compared with the oracle; None: all)
GEOMETRIES = {
    "kitti_b16": (KITTI_LEVELS, 16, (0, 7, 15)),                              # first, middle, last sample: the oracle is slow here
    "config4_1408x376_b2": ([(47, 176), (24, 88), (12, 44), (6, 22)], 2, None),
    "odd_b3": ([(17, 65), (9, 33), (5, 17), (3, 9)], 3, None),
    # 272 = kTileRows + W, 256 = kTileRows, 15 and 1 cells: two tiles with a ragged last one, exactly one full tile, single tiles
    "tile_edges_b2": ([(17, 16), (16, 16), (3, 5), (1, 1)], 2, None),
    "narrow_tall_b1": ([(300, 3), (40, 7), (12, 40), (2, 5)], 1, None),
}
REL = 1e-4               # tests/test_msda_gpu.py: max error / max |reference| of a float32 tensor
REL_HEAD = 1e-5          # test_fixed_point_scatter_keeps_small_rows_accurate_under_outliers: per head, of the head's own maximum


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


def _pyramid(levels):
    shapes = np.array(levels, dtype=np.int64)
    lsi = O.level_start_index(shapes)
    s, i = _dev(shapes), _dev(lsi)
    _msda().attach_host_geometry(s, i, shapes.tolist(), lsi.tolist())
    return shapes, lsi, s, i, int((shapes[:, 0] * shapes[:, 1]).sum())


def _ran_deterministic_msda(value, s, i, Lq, ref_dim=2):
    from monosowa_amd import _lib
    assert _lib.MSDA_DETERMINISTIC.sync() is True
    assert not _msda().fused_save_supported(value, s, i, Lq, ref_dim)       # no saved prologue: the backward re-evaluates it


def _twice(fn, names):
    """fn() twice -> the first results, after asserting that the second ones have the same bits"""
    first = [t.clone() for t in fn()]
    second = fn()
    torch.cuda.synchronize()
    for a, b, name in zip(first, second, names):
        assert torch.equal(a, b), "%s differs between two runs" % name
    return first


def _close_t(got, want, what, rel=REL):
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got.reshape(want.shape) - want).abs().max()) / scale
    assert err <= rel, "%s: max err / max|ref| = %.3e > %.1e" % (what, err, rel)


def test_the_tile_limit_these_geometries_are_built_around():
    """tile_edges_b2 puts one level at exactly kTileRows cells and one at kTileRows + W: move its levels with the constant."""
    with open(os.path.join(ROOT, "monosowa_amd", "csrc", "msda_common.h")) as f:
        assert int(re.search(r"constexpr int kTileRows = (\d+);", f.read()).group(1)) == 256
    with open(os.path.join(ROOT, "monosowa_amd", "csrc", "groupnorm.hip")) as f:
        assert re.search(r"kGnPix = (\d+)", f.read()).group(1) == "64"
    with open(os.path.join(ROOT, "monosowa_amd", "csrc", "head_tail.hip")) as f:
        assert int(re.search(r"kHeadMapCap = (\d+);", f.read()).group(1)) == 96 * 128


# ------------------------------------------------------------------------------------------------------------------- 1a MSDA
def _prologue(proj, ref, s, M):
    """sampling locations and attention weights as the module evaluates them (ms_deform_attn.py:146-155), float32, on autograd"""
    n, Lq = proj.shape[:2]
    off = proj[..., :M * 32].view(n, Lq, M, 4, 4, 2)
    aw = torch.softmax(proj[..., M * 32:].reshape(n, Lq, M, 16), -1).view(n, Lq, M, 4, 4)
    if ref.shape[-1] == 2:
        norm = torch.stack([s[:, 1], s[:, 0]], -1).float()
        loc = ref[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
    else:
        loc = ref[:, :, None, :, None, :2] + off / 4 * (ref[:, :, None, :, None, 2::2] + ref[:, :, None, :, None, 3::2]) * 0.5
    return loc, aw


def _fused_reference(value, mask, shapes, lsi, s, proj, ref, go, idx, pts_ratios=None):
    """The samples ``idx`` of the fused operator's backward: PyTorch prologue in float32 + the C oracle, chained through autograd.
    -> grad_value (float64 oracle; zero rows for padded tokens), grad_proj, grad_points (with ``pts_ratios``)."""
    M = value.shape[2]
    v = value[idx]
    if mask is not None:
        v = v.masked_fill(mask[idx][..., None, None], 0.0)
    p = proj[idx].detach().clone().requires_grad_(True)
    leaves = [p]
    if pts_ratios is not None:                                          # depthaware_transformer.py:590-596
        pts = pts_ratios[0][idx].detach().clone().requires_grad_(True)
        leaves.append(pts)
        ref_i = pts[:, :, None] * pts_ratios[1][idx][:, None]
    else:
        ref_i = ref[idx]
    loc, aw = _prologue(p, ref_i, s, M)
    want, want64 = _oracle_want(v.cpu().numpy(), shapes, lsi, loc.detach().cpu().numpy(), aw.detach().cpu().numpy(), go[idx].cpu().numpy())
    gv = want64[1].copy()
    if mask is not None:
        gv[mask[idx].cpu().numpy()] = 0.0                               # d masked_fill: nothing reaches a padded token's row
    # d location from the float32 oracle (the kernel's own floor() decisions), d weight from the float64 one
    grads = torch.autograd.grad([loc, aw], leaves, [torch.from_numpy(want[2]).cuda(), torch.from_numpy(want64[3].astype(np.float32)).cuda()])
    return (gv,) + tuple(grads)


def _check_fused(got_gv, got_gproj, want, idx, M, what):
    _close(got_gv[idx], want[0], REL, what + " grad_value")
    _close_t(got_gproj[idx][..., :M * 32], want[1][..., :M * 32], what + " grad_offsets")
    _close_t(got_gproj[idx][..., M * 32:], want[1][..., M * 32:], what + " grad_logits")


def _pixel_centres(levels):
    return np.concatenate([np.stack(np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h), -1).reshape(-1, 2)
                           for h, w in levels]).astype(np.float32)


def _cross_inputs(B, S, M, Lq, seed, ref_dim=6):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, device="cuda", generator=gen)
    n = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    value = n(B, S, M, 32)
    ref = torch.cat([r(B, Lq, 4, 2), r(B, Lq, 4, 4) * 0.3], -1) if ref_dim == 6 else r(B, Lq, 4, 2) * 1.2 - 0.1
    proj = torch.cat([n(B, Lq, M * 32) * 3.0, n(B, Lq, M * 16)], -1).contiguous()
    return value, ref.contiguous(), proj, n(B, Lq, M * 32)


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_unfused_backward_with_signed_weights_equals_the_oracle(deterministic, geom):
    """ms_deform_attn_backward (decoder form, Lq = 333) with weights uniform in [-1, 1] -- no softmax: bwd_bounds_kernel folds
    max |weight| over negative weights."""
    MSDA = _msda()
    levels, B, samples = GEOMETRIES[geom]
    value, shapes, lsi, loc, w, go = _random_case(len(geom) * 17 + B, B, 8, 32, 333, levels, 4, np.float32)
    w = np.random.default_rng(B).uniform(-1, 1, w.shape).astype(np.float32)
    _, _, s, i, _ = _pyramid(levels)
    v, l_, w_, g = _dev(value), _dev(loc), _dev(w), _dev(go)
    _ran_deterministic_msda(v, s, i, 333)
    gv, gl, gw = _twice(lambda: MSDA.ms_deform_attn_backward(v, s, i, l_, w_, g, 64), ["grad_value", "grad_loc", "grad_attn_w"])
    idx = list(samples or range(B))
    want, want64 = _oracle_want(value[idx], shapes, lsi, loc[idx], w[idx], go[idx])
    _close(gv[idx], want64[1], REL, "grad_value")
    _close(gw[idx], want64[3], REL, "grad_attn_w")
    _close(gl[idx], want[2], REL, "grad_loc")


def _self_attention_cases():
    for kind in ("initial", "sigma8", "pileup"):
        yield "kitti_b16", kind
    for geom in list(GEOMETRIES)[1:]:
        yield geom, "sigma3"


@pytest.mark.parametrize("geom,kind", list(_self_attention_cases()))
def test_fused_self_attention_backward_equals_the_oracle(deterministic, geom, kind):
    """The encoder's operator (Lq == S, 2-d reference points at the pixel centres, merged projection)."""
    MSDA = _msda()
    levels, B, samples = GEOMETRIES[geom]
    M = 8
    if geom == "kitti_b16":
        shapes, lsi, ref, offsets, logits, value, go = _encoder_case(B, 7, kind)
    else:
        rng = np.random.default_rng(len(geom))
        S = sum(h * w for h, w in levels)
        ref = _pixel_centres(levels)
        offsets = rng.normal(0.0, 3.0, (B, S, M, 4, 4, 2)).astype(np.float32)      # N(0, 3 px): near and far points, many outside
        logits = rng.standard_normal((B, S, M, 16)).astype(np.float32)
        value = rng.standard_normal((B, S, M, 32)).astype(np.float32)
        go = rng.standard_normal((B, S, M * 32)).astype(np.float32)
    shapes, lsi, s, i, S = _pyramid(levels)
    proj = torch.cat([_dev(offsets).reshape(B, S, M * 32), _dev(logits).reshape(B, S, M * 16)], -1).contiguous()
    refp = _dev(np.broadcast_to(ref[None, :, None, :], (B, S, 4, 2)).copy())
    v, g = _dev(value), _dev(go)
    _ran_deterministic_msda(v, s, i, S)
    gv, gproj = _twice(lambda: MSDA.ms_deform_attn_fused_backward_merged(v, s, i, proj, refp, g), ["grad_value", "grad_proj"])
    idx = list(samples or range(B))
    _check_fused(gv, gproj, _fused_reference(v, None, shapes, lsi, s, proj, refp, g, idx), idx, M, "%s %s" % (geom, kind))


@pytest.mark.parametrize("Lq", [550, 50, 333])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_fused_cross_attention_backward_equals_the_oracle(deterministic, geom, Lq):
    """The decoder's operator: Lq queries with 6-d reference boxes (location = centre + offset / P * half the box extent)."""
    MSDA = _msda()
    levels, B, samples = GEOMETRIES[geom]
    M = 8
    shapes, lsi, s, i, S = _pyramid(levels)
    v, refp, proj, g = _cross_inputs(B, S, M, Lq, Lq + len(geom))
    _ran_deterministic_msda(v, s, i, Lq, 6)
    gv, gproj = _twice(lambda: MSDA.ms_deform_attn_fused_backward_merged(v, s, i, proj, refp, g), ["grad_value", "grad_proj"])
    idx = list(samples or range(B))
    _check_fused(gv, gproj, _fused_reference(v, None, shapes, lsi, s, proj, refp, g, idx), idx, M, "%s Lq %d" % (geom, Lq))


@pytest.mark.parametrize("form", ["unfused", "self", "cross"])
def test_three_heads_two_images_leave_the_grouped_by_eight_grid_early(deterministic, form):
    """M = 3, B = 2: six (batch, head) pairs on a grid that walks them in groups of eight (the ``bm >= BM`` return)."""
    MSDA = _msda()
    B, M = 2, 3
    shapes, lsi, s, i, S = _pyramid(SMALL_LEVELS)
    if form == "unfused":
        value, _, _, loc, w, go = _random_case(5, B, M, 32, 333, SMALL_LEVELS, 4, np.float32)
        v, l_, w_, g = _dev(value), _dev(loc), _dev(w), _dev(go)
        _ran_deterministic_msda(v, s, i, 333)
        gv, gl, gw = _twice(lambda: MSDA.ms_deform_attn_backward(v, s, i, l_, w_, g, 64), ["grad_value", "grad_loc", "grad_attn_w"])
        want, want64 = _oracle_want(value, shapes, lsi, loc, w, go)
        _close(gv, want64[1], REL, "grad_value")
        _close(gw, want64[3], REL, "grad_attn_w")
        _close(gl, want[2], REL, "grad_loc")
        return
    Lq = S if form == "self" else 333
    v, refp, proj, g = _cross_inputs(B, S, M, Lq, 9, 6 if form == "cross" else 2)
    if form == "self":
        refp = _dev(np.broadcast_to(_pixel_centres(SMALL_LEVELS)[None, :, None, :], (B, S, 4, 2)).copy())
    _ran_deterministic_msda(v, s, i, Lq, refp.shape[-1])
    gv, gproj = _twice(lambda: MSDA.ms_deform_attn_fused_backward_merged(v, s, i, proj, refp, g), ["grad_value", "grad_proj"])
    idx = list(range(B))
    _check_fused(gv, gproj, _fused_reference(v, None, shapes, lsi, s, proj, refp, g, idx), idx, M, form)


@pytest.mark.parametrize("levels", [VIEW_LEVELS, GEOMETRIES["odd_b3"][0], GEOMETRIES["tile_edges_b2"][0]], ids=["24x40", "odd", "tile_edges"])
@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("masked,strided", [(True, False), (False, True), (True, True)])
def test_fused_operator_on_a_value_view_equals_the_oracle(deterministic, levels, kind, masked, strided):
    """``value`` as one 256-column block of a [B, S, 768] tensor and / or with a padding mask, built as
    test_fused_operator_on_a_value_view_equals_masked_fill_plus_the_unfused_operator builds them: in this mode padded tokens and
    the token stride reach bwd_scatter_kernel's exclusive write-back, which no default-mode call takes with a mask.  Padded
    tokens get exactly-zero gradient rows; the other two column blocks of the wide tensor get exactly zero."""
    from monosowa_amd.ms_deform_attn_func import MSDeformAttnFusedMergedFunction
    torch.manual_seed(31 + masked + 2 * strided)
    B, M, D = 2, 8, 32
    shapes, lsi, s, i, S = _pyramid(levels)
    if kind == "self":
        Lq = S
        ref = _dev(np.broadcast_to(_pixel_centres(levels)[None, :, None, :], (B, S, 4, 2)).copy())
    else:
        Lq = 333
        ref = torch.cat([torch.rand(B, Lq, 4, 2, device="cuda"), torch.rand(B, Lq, 4, 4, device="cuda") * 0.3], -1)
    wide = torch.randn(B, S, 3 * M * D, device="cuda")
    dense = wide[:, :, M * D:2 * M * D].contiguous().view(B, S, M, D)
    mask = (torch.rand(B, S, device="cuda") < 0.25) if masked else None
    proj0 = torch.cat([torch.randn(B, Lq, M * 32, device="cuda") * 3.0, torch.randn(B, Lq, M * 16, device="cuda")], -1)
    go = torch.randn(B, Lq, M * D, device="cuda")

    def once():
        proj = proj0.clone().requires_grad_(True)
        if strided:
            leaf = wide.detach().clone().requires_grad_(True)
            value_in = leaf[:, :, M * D:2 * M * D].view(B, S, M, D)
            assert not value_in.is_contiguous()
        else:
            leaf = value_in = dense.detach().clone().requires_grad_(True)
        _ran_deterministic_msda(value_in, s, i, Lq, ref.shape[-1])
        out = MSDeformAttnFusedMergedFunction.apply(value_in, s, i, proj, ref, mask)
        assert out.grad_fn.saved_prologue is False
        out.backward(go)
        return leaf.grad.reshape(B, S, -1), proj.grad

    g_leaf, gproj = _twice(once, ["grad_value", "grad_proj"])
    if strided:
        assert g_leaf[:, :, :M * D].abs().max() == 0 and g_leaf[:, :, 2 * M * D:].abs().max() == 0
        g_leaf = g_leaf[:, :, M * D:2 * M * D]
    gv = g_leaf.reshape(B, S, M, D)
    if masked:
        assert mask.any() and gv[mask].abs().max() == 0                  # padded tokens: exactly zero gradient rows
    idx = list(range(B))
    _check_fused(gv, gproj, _fused_reference(dense, mask, shapes, lsi, s, proj0, ref, go, idx), idx, M, "%s view" % kind)


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_fused_operator_hands_a_gradient_to_2d_reference_points(deterministic, geom):
    """The decoder's first layer (test_msda_gpu.py's construction): 2-d reference points from a learned embedding carry a gradient,
    which the Function derives from the kernels' d offsets."""
    from monosowa_amd.ms_deform_attn_func import MSDeformAttnFusedMergedFunction
    levels, B, samples = GEOMETRIES[geom]
    torch.manual_seed(41 + B)
    M, D, Lq = 8, 32, 275
    shapes, lsi, s, i, S = _pyramid(levels)
    value = torch.randn(B, S, M, D, device="cuda")
    pts0 = torch.rand(B, Lq, 2, device="cuda")
    ratios = torch.rand(B, 4, 2, device="cuda") * 0.2 + 0.8
    proj0 = torch.cat([torch.randn(B, Lq, M * 32, device="cuda") * 2, torch.randn(B, Lq, M * 16, device="cuda")], -1)
    go = torch.randn(B, Lq, M * D, device="cuda")

    def once():
        v, pts, proj = value.clone().requires_grad_(True), pts0.clone().requires_grad_(True), proj0.clone().requires_grad_(True)
        _ran_deterministic_msda(v, s, i, Lq)
        out = MSDeformAttnFusedMergedFunction.apply(v, s, i, proj, (pts[:, :, None] * ratios[:, None]).contiguous())
        assert out.grad_fn.saved_prologue is False
        out.backward(go)
        return v.grad, proj.grad, pts.grad

    gv, gproj, gpts = _twice(once, ["grad_value", "grad_proj", "grad_reference_points"])
    idx = list(samples or range(B))
    want = _fused_reference(value, None, shapes, lsi, s, proj0, None, go, idx, pts_ratios=(pts0, ratios))
    _check_fused(gv, gproj, want, idx, M, geom)
    _close_t(gpts[idx], want[2], "grad_reference_points")


def _per_head(gv, ref, what):
    """every head against the float64 oracle relative to that head's own maximum"""
    gv = gv.cpu().numpy().astype(np.float64).reshape(ref.shape)
    for m in range(ref.shape[2]):
        scale = np.abs(ref[:, :, m]).max()
        err = np.abs(gv[:, :, m] - ref[:, :, m]).max()
        assert err <= REL_HEAD * scale, "%s, head %d: max err / max|ref| = %.3e" % (what, m, err / max(scale, 1e-300))


@pytest.mark.parametrize("case", ["scale_1e-30", "scale_1e+30", "outlier_1e6", "bound_power_of_two", "one_head_zero"])
def test_fixed_point_scatter_range(deterministic, case):
    """The 64-bit fixed-point accumulators are scaled per (batch, head) by 2^(42 - exponent of max|weight| * max|grad_out|):
    tiny and huge gradients (the exponent clamp at 126, the ``bound < 3e38`` test), a 1e6 outlier in one head, a bound that is an
    exact power of two (frexp's fraction is then 0.5: the edge of the exponent arithmetic), and a (batch, head) whose grad_out
    is identically zero (``bound == 0``: exactly-zero rows)."""
    MSDA = _msda()
    B, M, D, Lq = 2, 8, 32, 300
    value, shapes, lsi, loc, w, go = _random_case(77, B, M, D, Lq, SMALL_LEVELS, 4, np.float32, 0.05, 0.95)
    go = go.reshape(B, Lq, M, D)
    if case.startswith("scale_"):
        go = go * np.float32(float(case[6:]))
    elif case == "outlier_1e6":
        go[0, 0, 0, :] = 1e6                                             # head 0 of image 0 only
    elif case == "bound_power_of_two":
        go[1, 5, 3, 0] = 8.0                                             # max |grad_out| = 8, max weight = 1: bound = 2^3 exactly
        w[1, 5, 3, 0, 0] = 1.0
        assert np.abs(go[1, :, 3]).max() == 8.0 and np.abs(w[1, :, 3]).max() == 1.0
    else:
        go[1, :, 2, :] = 0.0
    go = np.ascontiguousarray(go.reshape(B, Lq, M * D))
    _, _, s, i, _ = _pyramid(SMALL_LEVELS)
    v, l_, w_, g = _dev(value), _dev(loc), _dev(w), _dev(go)
    _ran_deterministic_msda(v, s, i, Lq)
    gv, gl, gw = _twice(lambda: MSDA.ms_deform_attn_backward(v, s, i, l_, w_, g, 64), ["grad_value", "grad_loc", "grad_attn_w"])
    d = lambda a: a.astype(np.float64)
    ref = O.backward(d(value), shapes, lsi, d(loc), d(w), d(go))
    for b in range(B):
        _per_head(gv[b:b + 1], ref[0][b:b + 1], "%s grad_value[%d]" % (case, b))
    _close(gw, ref[2], REL, "grad_attn_w")
    if case == "one_head_zero":
        assert not gv[1, :, 2].any() and not ref[0][1, :, 2].any()
        assert gv[1, :, 1].any() and gv[1, :, 3].any() and gv[0, :, 2].any()


def test_all_points_outside_and_nan_locations(deterministic):
    """What tests/test_msda_gpu.py asserts for the default kernels: nothing but zeros comes back."""
    MSDA = _msda()
    shapes = torch.tensor(KITTI_LEVELS, dtype=torch.long).cuda()
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    v = torch.randn(1, 10200, 8, 32).cuda()
    loc = torch.full((1, 5, 8, 4, 4, 2), 7.0).cuda()
    loc[0, 1] = float("nan")
    loc[0, 2] = 1e30
    loc[0, 3] = -1e30
    w = torch.full((1, 5, 8, 4, 4), 1 / 16).cuda()
    go = torch.ones(1, 5, 256).cuda()
    _ran_deterministic_msda(v, shapes, lsi, 5)
    out = MSDA.ms_deform_attn_forward(v, shapes, lsi, loc, w, 64)
    gv, gl, gw = _twice(lambda: MSDA.ms_deform_attn_backward(v, shapes, lsi, loc, w, go, 64), ["grad_value", "grad_loc", "grad_attn_w"])
    assert not out.any() and not gv.any() and not gl.any() and not gw.any()


# -------------------------------------------------------------------------------------------------------------- 1b GroupNorm
# 64 and 65 pixels: exactly one workgroup of kGnPix = 64 pixels, and one plus a ragged one (gn_fold_kernel adds one row / two)
GN_SHAPES = [(3, 256, 24, 80), (2, 256, 7, 9), (1, 256, 1, 1), (16, 256, 48, 160), (3, 256, 17, 65), (2, 256, 8, 8), (2, 256, 5, 13)]
GN_REL = 3e-5            # test_groupnorm_nhwc_matches_torch: max abs error <= 3e-5 * max(max |ref|, 1)


def _gn_case(shape, with_bias):
    torch.manual_seed(1)
    gn = torch.nn.GroupNorm(32, 256).cuda()
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.uniform_(-0.5, 0.5)
    x = (torch.randn(shape, device="cuda") * 2 + 5).contiguous(memory_format=torch.channels_last)
    go = torch.randn(shape, device="cuda").contiguous(memory_format=torch.channels_last)
    pre_bias = torch.randn(256, device="cuda") if with_bias else None
    return gn, x, go, pre_bias


def _gn_reference(gn, x, go, pre_bias, relu, y_got):
    """torch.nn.GroupNorm (+ ReLU) in float64 -> y, grad_x, grad_weight, grad_bias, grad_pre_bias.  ReLU's derivative jumps at 0 and
    the kernel's own float32 output decides which side an element is on.  Where that decision differs from float64's, the
    float64 pre-activation must itself be within the forward tolerance of 0; the reference's backward then takes the kernel's
    side at those elements (every element is compared, none left out)."""
    xd = x.detach().double().contiguous().requires_grad_(True)
    gnd = torch.nn.GroupNorm(32, 256).cuda().double()
    gnd.load_state_dict({k: v.double() for k, v in gn.state_dict().items()})
    bd = pre_bias.detach().double().requires_grad_(True) if pre_bias is not None else None
    pre = gnd(xd + bd.view(1, -1, 1, 1) if bd is not None else xd)
    y = torch.relu(pre) if relu else pre
    if relu:
        kept = y_got > 0
        differs = kept != (pre.detach() > 0)
        assert not differs.any() or pre.detach()[differs].abs().max() <= GN_REL, "ReLU decisions differ away from 0"
        torch.autograd.backward(pre * kept, go.double())
    else:
        torch.autograd.backward(pre, go.double())
    return [y.detach(), xd.grad, gnd.weight.grad, gnd.bias.grad] + ([bd.grad] if bd is not None else [])


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "prebias"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_equals_float64(deterministic, shape, relu, with_bias):
    from monosowa_amd import pointwise
    gn, x, go, pre_bias = _gn_case(shape, with_bias)
    names = ["y", "grad_x", "grad_weight", "grad_bias"] + (["grad_pre_bias"] if with_bias else [])

    def once():
        xl = x.clone().requires_grad_(True)
        bl = pre_bias.clone().requires_grad_(True) if with_bias else None
        assert pointwise.DETERMINISTIC.sync() is True
        y = pointwise.group_norm(xl, gn, relu=relu, pre_bias=bl)
        assert type(y.grad_fn).__name__ == "_GroupNormNHWCBackward" and y.is_contiguous(memory_format=torch.channels_last)
        grads = torch.autograd.grad(y, [xl, gn.weight, gn.bias] + ([bl] if with_bias else []), go)
        return (y.detach(),) + grads

    got = _twice(once, names)
    for a, b, n in zip(got, _gn_reference(gn, x, go, pre_bias, relu, got[0]), names):
        err = (a.double() - b).abs().max().item()
        assert err <= GN_REL * max(b.abs().max().item(), 1.0), (n, err, b.abs().max().item())


@pytest.mark.parametrize("shape", [(2, 256, 8, 8), (2, 256, 5, 13), (3, 256, 17, 65)], ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_stores_every_scratch_element_it_reads(deterministic, shape):
    """At the C ABI with NaN-filled statistics / partial-sum buffers (the wrapper hands over torch.empty): y, grad_x and the
    parameter gradients come back finite and with the bits the wrapper's call gives."""
    from monosowa_amd import pointwise
    from monosowa_amd._lib import raw_stream
    lib = pointwise.load()
    gn, x, go, pre_bias = _gn_case(shape, True)
    assert pointwise.DETERMINISTIC.sync() is True
    B, C, H, W = shape
    n_stats, n_part, blocks = lib.mono_groupnorm_stats_doubles(B, H * W), lib.mono_groupnorm_part_doubles(B, H * W), lib.mono_groupnorm_blocks(B, H * W)
    assert blocks == B * -(-H * W // 64) and n_stats == (B + blocks) * 64 and n_part == (B + blocks) * 512
    nan = lambda n, dtype: torch.full((n,), float("nan"), dtype=dtype, device="cuda")
    stats, part = nan(n_stats, torch.float64), nan(n_part, torch.float64)
    y, gx = nan(x.numel(), torch.float32).view(B, H, W, C).permute(0, 3, 1, 2), nan(x.numel(), torch.float32).view(B, H, W, C).permute(0, 3, 1, 2)
    mean_rstd, gbias, partials, gwb = nan(B * 64, torch.float32), nan(C, torch.float32), nan(blocks * C, torch.float32), nan(2 * C, torch.float32)
    assert lib.mono_groupnorm_nhwc_fwd_f32(x.data_ptr(), pre_bias.data_ptr(), gn.weight.data_ptr(), gn.bias.data_ptr(), y.data_ptr(),
                                           stats.data_ptr(), mean_rstd.data_ptr(), B, H * W, C, 32, float(gn.eps), 1, raw_stream()) == 0
    assert lib.mono_groupnorm_nhwc_bwd_f32(go.data_ptr(), x.data_ptr(), pre_bias.data_ptr(), y.data_ptr(), mean_rstd.data_ptr(),
                                           gn.weight.data_ptr(), gx.data_ptr(), part.data_ptr(), gbias.data_ptr(), partials.data_ptr(),
                                           gwb.data_ptr(), B, H * W, C, 32, 1, raw_stream()) == 0
    torch.cuda.synchronize()
    xl, bl = x.clone().requires_grad_(True), pre_bias.clone().requires_grad_(True)
    y_w = pointwise.group_norm(xl, gn, relu=True, pre_bias=bl)
    want = (y_w.detach(),) + torch.autograd.grad(y_w, [xl, bl, gn.weight, gn.bias], go)
    for name, a, b in zip(("y", "grad_x", "grad_pre_bias", "grad_weight", "grad_bias"), (y, gx, gbias, gwb[:C], gwb[C:]), want):
        assert torch.isfinite(a).all() and torch.equal(a, b), name
    assert torch.isfinite(stats[:B * 64]).all() and torch.isfinite(part[:B * 512]).all()


# -------------------------------------------------------------------------------------------------------------- 1c head tail
# max abs error / max |R| per output tensor, R = the plain expression of monodetr.py in float64.  Bound = 4 x the worst e_P (the same
# expression in plain float32 against R) over every case of this module on the MI355X, rounded up to one significant digit; the
# deterministic kernels (D), the default atomic kernel (F) and P all have to meet it.  Measured worst e_F / e_D / e_P beside each.
HEAD_TAIL_BOUNDS = {
    "coords": 6e-7,              # 1.56e-7 / 1.56e-7 / 1.37e-7
    "depth_ave": 5e-5,           # 1.18e-5 / 1.18e-5 / 1.17e-5  (a random map: 40 units per pixel times float32's error in the tap position)
    "grad_tmp": 3e-6,            # 4.24e-7 / 4.24e-7 / 6.47e-7
    "grad_size3d": 2e-6,         # 3.66e-7 / 3.66e-7 / 3.16e-7
    "grad_depth_reg": 2e-6,      # 3.16e-7 / 3.16e-7 / 3.31e-7
    "grad_wdepth": 7e-5,         # 1.81e-5 / 1.75e-5 / 1.75e-5
}
HEAD_TAIL_NAMES = list(HEAD_TAIL_BOUNDS)
HEAD_TAIL_MAPS = [(48, 160), (24, 88), (9, 33), (1, 7), (96, 128)]       # 96 x 128 = 12288 cells: exactly the cap of the LDS map
_HEAD_TAIL_WORST = {}


def _head_tail_plain(tmp, size3d, depth_reg, wdepth, fu, img_h, ref):
    """monodetr.py with FUSED_HEAD_TAIL = False, in the dtype of its arguments"""
    from monosowa_amd.monodetr.misc import inverse_sigmoid
    if ref is not None:
        inv = inverse_sigmoid(ref)
        tmp = tmp + inv if inv.shape[-1] == 6 else torch.cat([tmp[..., :2] + inv, tmp[..., 2:]], -1)
    coords = tmp.sigmoid()
    box2d_height = torch.clamp((coords[:, :, 4] + coords[:, :, 5]) * img_h[:, None], min=1.0)
    depth_geo = size3d[:, :, 0] / box2d_height * fu[:, None]
    centre = ((coords[..., :2] - 0.5) * 2).unsqueeze(2).detach()
    depth_map = F.grid_sample(wdepth.unsqueeze(1), centre, mode="bilinear", align_corners=True).squeeze(1)
    depth_ave = torch.cat([((1. / (depth_reg[:, :, 0:1].sigmoid() + 1e-6) - 1.) + depth_geo.unsqueeze(-1) + depth_map) / 3,
                           depth_reg[:, :, 1:2]], -1)
    return coords, depth_ave


def _head_tail_inputs(B, Q, H, W, centres, ref_dim, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *shape: torch.rand(*shape, device="cuda", generator=gen)
    n = lambda *shape: torch.randn(*shape, device="cuda", generator=gen)
    tmp = n(B, Q, 6)
    if centres == "spread":                                               # sigmoid(tmp) uniform over the map
        u = r(B, Q, 2) * 0.98 + 0.01
        tmp[..., :2] = torch.log(u / (1 - u))
    elif centres == "piled":                                              # the construction of test_head_tail_is_bitwise_reproducible
        tmp[..., :2] = n(B, Q, 2) * 0.05 + torch.tensor([0.3, -0.2], device="cuda")
    else:                                                                 # a tenth of the queries at +-20: float32 sigmoid saturates
        sat = (r(B, Q) < 0.1) | (torch.arange(Q, device="cuda") == 0)
        sign = torch.where(r(B, Q, 2) < 0.5, -20.0, 20.0)
        tmp[..., :2] = torch.where(sat[..., None], sign, tmp[..., :2])
    ref = None
    if ref_dim:
        ref = r(B, Q, ref_dim) * 0.9 + 0.05
        if centres == "saturated":
            tmp[..., :2] = tmp[..., :2] * 2                               # +-40: inverse_sigmoid(ref) adds up to +-2.9 and sigmoid(17) is not yet 1
    return dict(tmp=tmp, size3d=r(B, Q, 3) + 0.5, depth_reg=n(B, Q, 2), wdepth=r(B, H, W) * 40, fu=torch.full((B,), 720.0, device="cuda"),
                img_h=torch.full((B,), 384.0, device="cuda"), ref=ref, g_coords=n(B, Q, 6), g_dave=n(B, Q, 2))


def _head_tail_eval(inp, how, cotangent):
    """-> coords, depth_ave and the four gradients; how: "kernel" (fused, in torch's current mode), "P" (plain float32), "R" (float64)"""
    from monosowa_amd import pointwise
    dtype = torch.float64 if how == "R" else torch.float32
    leaves = [inp[k].to(dtype).clone().requires_grad_(True) for k in ("tmp", "size3d", "depth_reg", "wdepth")]
    fu, img_h = inp["fu"].to(dtype), inp["img_h"].to(dtype)
    ref = inp["ref"].to(dtype) if inp["ref"] is not None else None
    if how == "kernel":
        assert pointwise.head_tail_supported(*leaves, fu, img_h)
        coords, dave = pointwise.head_tail(*leaves, fu, img_h, ref=ref)
        assert type(coords.grad_fn).__name__ == "_HeadTailBackward"
    else:
        coords, dave = _head_tail_plain(*leaves, fu, img_h, ref)
    g_dave = inp["g_dave"].to(dtype).clone()
    if cotangent == "third_zero":
        g_dave[:, ::3, 0] = 0.0
    if cotangent == "coords_only":
        grads = torch.autograd.grad([coords], leaves, [inp["g_coords"].to(dtype)], allow_unused=True)
        grads = [torch.zeros_like(l) if g is None else g for g, l in zip(grads, leaves)]
    else:
        grads = torch.autograd.grad([coords, dave], leaves, [inp["g_coords"].to(dtype), g_dave])
    return [coords.detach(), dave.detach()] + list(grads)


def _head_tail_errors(got, want):
    return {n: float((g.double() - w).abs().max()) / max(float(w.abs().max()), 1e-30) for n, g, w in zip(HEAD_TAIL_NAMES, got, want)}


@pytest.mark.parametrize("centres", ["spread", "piled", "saturated"])
@pytest.mark.parametrize("hw", HEAD_TAIL_MAPS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("Q", [1, 256, 257, 550])
def test_head_tail_equals_float64(Q, hw, centres):
    """The deterministic kernels (the depth-map gradient summed in query order in LDS, into an uninitialised buffer) and the default
    atomic kernel against float64; reference points absent / 2-d / 6-d; full cotangents, d depth_ave[..., 0] = 0 for a third of
    the queries, and a backward from ``coords`` alone (the whole depth-map gradient is then exactly zero)."""
    from monosowa_amd import pointwise
    H, W = hw
    B = 16 if (Q, hw) == (550, (48, 160)) else 3
    was, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    failures = []
    try:
        for ref_dim in (0, 2, 6):
            for cotangent in ("full", "third_zero", "coords_only"):
                inp = _head_tail_inputs(B, Q, H, W, centres, ref_dim, Q + H + ref_dim)
                torch.use_deterministic_algorithms(False)
                r_ = _head_tail_eval(inp, "R", cotangent)
                evals = {"P": _head_tail_eval(inp, "P", cotangent), "F": _head_tail_eval(inp, "kernel", cotangent)}
                torch.use_deterministic_algorithms(True)
                assert pointwise.DETERMINISTIC.sync() is True
                evals["D"] = _twice(lambda: _head_tail_eval(inp, "kernel", cotangent), HEAD_TAIL_NAMES)
                if cotangent == "coords_only":
                    assert not evals["D"][5].any() and not evals["F"][5].any() and not r_[5].any()
                else:
                    assert bool(evals["D"][5].any()) == bool(r_[5].any())
                for how, got in evals.items():
                    for name, e in _head_tail_errors(got, r_).items():
                        key = (name, how)
                        _HEAD_TAIL_WORST[key] = max(_HEAD_TAIL_WORST.get(key, 0.0), e)
                        if not e <= HEAD_TAIL_BOUNDS[name]:
                            failures.append((how, name, "ref_dim %d" % ref_dim, cotangent, e, HEAD_TAIL_BOUNDS[name]))
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn_only)
    print("\nhead tail Q %d map %dx%d %s, worst so far: %s" % (Q, H, W, centres, "  ".join(
        "%s e_F %.2e e_D %.2e e_P %.2e" % ((n,) + tuple(_HEAD_TAIL_WORST.get((n, h), 0.0) for h in "FDP")) for n in HEAD_TAIL_NAMES)))
    assert not failures, failures


def test_head_tail_backward_without_a_depth_gradient_zeroes_the_whole_map(deterministic):
    """mono_head_tail_bwd_f32 with g_depth_ave = NULL and a NaN-filled g_wdepth: the deterministic kernel stores the whole map (the
    wrapper hands it an uninitialised buffer), so every cell comes back exactly zero."""
    from monosowa_amd import pointwise
    from monosowa_amd._lib import raw_stream
    B, Q, H, W = 3, 257, 9, 33
    inp = _head_tail_inputs(B, Q, H, W, "spread", 2, 3)
    assert pointwise.DETERMINISTIC.sync() is True
    g_tmp, g_size, g_dreg = torch.empty(B, Q, 6, device="cuda"), torch.empty(B, Q, 3, device="cuda"), torch.empty(B, Q, 2, device="cuda")
    g_wd = torch.full((B, H, W), float("nan"), device="cuda")
    code = pointwise.load().mono_head_tail_bwd_f32(
        inp["tmp"].data_ptr(), inp["size3d"].data_ptr(), inp["depth_reg"].data_ptr(), inp["wdepth"].data_ptr(), inp["fu"].data_ptr(),
        inp["img_h"].data_ptr(), inp["g_coords"].data_ptr(), None, g_tmp.data_ptr(), g_size.data_ptr(), g_dreg.data_ptr(), g_wd.data_ptr(),
        B, Q, H, W, inp["ref"].data_ptr(), 2, raw_stream())
    torch.cuda.synchronize()
    assert code == 0
    assert not g_wd.any() and not g_size.any() and not g_dreg.any()
    # with a depth gradient into the NaN-filled map: the bits of the wrapper's call (whose torch.empty may happen to be zeros)
    g_wd.fill_(float("nan"))
    code = pointwise.load().mono_head_tail_bwd_f32(
        inp["tmp"].data_ptr(), inp["size3d"].data_ptr(), inp["depth_reg"].data_ptr(), inp["wdepth"].data_ptr(), inp["fu"].data_ptr(),
        inp["img_h"].data_ptr(), inp["g_coords"].data_ptr(), inp["g_dave"].data_ptr(), g_tmp.data_ptr(), g_size.data_ptr(), g_dreg.data_ptr(),
        g_wd.data_ptr(), B, Q, H, W, inp["ref"].data_ptr(), 2, raw_stream())
    torch.cuda.synchronize()
    assert code == 0
    wrapped = _head_tail_eval(inp, "kernel", "full")
    for name, a, b in zip(HEAD_TAIL_NAMES[2:], (g_tmp, g_size, g_dreg, g_wd), wrapped[2:]):
        assert torch.equal(a, b), name
    torch.use_deterministic_algorithms(False)
    errs = _head_tail_errors(wrapped, _head_tail_eval(inp, "R", "full"))
    assert all(e <= HEAD_TAIL_BOUNDS[n] for n, e in errs.items()), errs


def test_head_tail_above_the_map_cap_refuses_or_warns(deterministic):
    """97 x 128 cells do not fit the LDS map: head_tail_supported says so (the model then takes the plain expression), and a direct
    call never runs silently -- RuntimeError naming the op, or one warning under warn_only (and the atomic kernel runs)."""
    from monosowa_amd import _lib, pointwise
    B, Q, H, W = 2, 50, 97, 128
    inp = _head_tail_inputs(B, Q, H, W, "spread", 0, 5)
    leaves = [inp[k].clone().requires_grad_(True) for k in ("tmp", "size3d", "depth_reg", "wdepth")]
    assert not pointwise.head_tail_supported(*leaves, inp["fu"], inp["img_h"])
    coords, dave = pointwise.head_tail(*leaves, inp["fu"], inp["img_h"])
    with pytest.raises(RuntimeError, match="head_tail does not have a deterministic implementation"):
        torch.autograd.grad([coords, dave], leaves, [inp["g_coords"], inp["g_dave"]], retain_graph=True)
    # the model's own route above the cap, the plain expression: torch refuses its grid_sample backward
    c2, d2 = _head_tail_plain(*leaves, inp["fu"], inp["img_h"], None)
    with pytest.raises(RuntimeError, match="deterministic"):
        torch.autograd.grad([c2, d2], leaves, [inp["g_coords"], inp["g_dave"]])
    torch.use_deterministic_algorithms(True, warn_only=True)
    _lib._ALERTED.discard("head_tail")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = torch.autograd.grad([coords, dave], leaves, [inp["g_coords"], inp["g_dave"]], retain_graph=True)
        torch.autograd.grad([coords, dave], leaves, [inp["g_coords"], inp["g_dave"]])
    assert len([r for r in rec if "head_tail does not have" in str(r.message)]) == 1, [str(r.message) for r in rec]
    torch.use_deterministic_algorithms(False)
    want = _head_tail_eval(inp, "R", "full")
    assert float((got[3].double() - want[5]).abs().max()) <= HEAD_TAIL_BOUNDS["grad_wdepth"] * float(want[5].abs().max())
    assert pointwise.head_tail_supported(*leaves, inp["fu"], inp["img_h"])           # (flag off: any map)


# ------------------------------------------------------------------------------------------------------ 1d upsample_bilinear
@pytest.mark.parametrize("src,dst", UPSAMPLE_SIZES)
def test_upsample_bilinear_as_matrix_products_equals_float64_interpolate(deterministic, src, dst):
    """On the MI355X plain float32 F.interpolate against float64 measures e_P = 9.3e-7 forward and 7.4e-7 gradient at worst over
    these sizes ((5, 17) -> (9, 33)), the matrix-product form e_D = 9.4e-7 / 7.6e-7: 4 x e_P rounds up to the CPU bound again."""
    from monosowa_amd.monodetr.depth_predictor import upsample_bilinear
    torch.manual_seed(src[0] * 100 + dst[1])
    x = torch.randn(2, 256, *src, device="cuda")
    gy = torch.randn(2, 256, *dst, device="cuda")
    xr = x.double().requires_grad_(True)
    ref = F.interpolate(xr, size=dst, mode="bilinear")
    torch.use_deterministic_algorithms(False)                            # (ATen's bilinear backward refuses to run under the flag)
    g_ref, = torch.autograd.grad(ref, xr, gy.double())
    xp = x.clone().requires_grad_(True)
    plain = upsample_bilinear(xp, dst)                                   # flag off: F.interpolate's own bits, gradient wanted or not
    assert torch.equal(plain, F.interpolate(x, size=dst, mode="bilinear"))
    g_plain, = torch.autograd.grad(plain, xp, gy)
    torch.use_deterministic_algorithms(True)
    assert torch.equal(upsample_bilinear(x, dst), F.interpolate(x, size=dst, mode="bilinear"))      # no gradient wanted

    def once():
        xd = x.clone().requires_grad_(True)
        y = upsample_bilinear(xd, dst)
        assert "Upsample" not in type(y.grad_fn).__name__ and y.is_contiguous(memory_format=torch.channels_last)
        return y.detach(), torch.autograd.grad(y, xd, gy)[0]

    y, g = _twice(once, ["forward", "grad_input"])
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))
    print("\nupsample %s -> %s: forward e_D %.2e e_P %.2e, gradient e_D %.2e e_P %.2e" % (src, dst, rel(y, ref), rel(plain, ref), rel(g, g_ref), rel(g_plain, g_ref)))
    assert rel(plain, ref) <= BOUND_UPSAMPLE and rel(g_plain, g_ref) <= BOUND_UPSAMPLE               # plain float32 meets it too
    assert rel(y, ref) <= BOUND_UPSAMPLE and rel(g, g_ref) <= BOUND_UPSAMPLE


# ---------------------------------------------------------------------------------------------------------- 1e hipBLASLt shim
def _gemm_deterministic():
    from monosowa_amd import gemm_lt
    assert gemm_lt.DETERMINISTIC.sync() is True
    return gemm_lt


@pytest.mark.parametrize("M,N,K", G.NT_SHAPES)
@pytest.mark.parametrize("scale,bias,residual,relu", G.NT_EPILOGUES)
def test_nt_epilogue_matches_float64(deterministic, M, N, K, scale, bias, residual, relu):
    """tests/test_gemm_lt_gpu.py's comparison with the kernel picked without timing (the heuristic's first candidate)."""
    _gemm_deterministic()
    _twice(lambda: G.check_nt_epilogue(M, N, K, scale, bias, residual, relu), ["product"])


@pytest.mark.parametrize("M,N,K", G.TN_SHAPES)
def test_tn_bgrad_gives_weight_and_bias_gradient(deterministic, M, N, K):
    _gemm_deterministic()
    _twice(lambda: G.check_tn_bgrad(M, N, K), ["grad_weight", "grad_bias", "grad_weight without bias"])


def test_nn_and_strided_views(deterministic):
    _gemm_deterministic()
    _twice(G.check_nn_and_strided_views, ["grad_input", "product of a view"])


def test_a_timed_selection_does_not_leak_into_the_deterministic_one(deterministic):
    """flag on -> off -> on in one process at shapes no other test uses: the mode is part of the selection cache's key, so the
    deterministic calls on both sides of a timed selection give the same bits."""
    gemm_lt = _gemm_deterministic()
    lib = gemm_lt.load()
    torch.manual_seed(12)
    a, w, b = torch.randn(1544, 200, device="cuda"), torch.randn(136, 200, device="cuda"), torch.randn(136, device="cuda")
    gy = torch.randn(1544, 136, device="cuda")
    run = lambda: [gemm_lt.gemm_nt(a, w, None, b, None, True)] + list(gemm_lt.gemm_tn_bgrad(gy, a)) + [gemm_lt.gemm_nn(gy, w)]
    n0 = lib.mono_gemm_cache_size()
    first = [t.clone() for t in run()]
    n1 = lib.mono_gemm_cache_size()
    assert n1 == n0 + 3
    torch.use_deterministic_algorithms(False)
    assert gemm_lt.DETERMINISTIC.sync() is False
    timed = run()
    assert lib.mono_gemm_cache_size() == n1 + 3                         # the timed selections: keys of their own
    torch.use_deterministic_algorithms(True)
    assert gemm_lt.DETERMINISTIC.sync() is True
    again = run()
    assert lib.mono_gemm_cache_size() == n1 + 3
    ref = [(a.double() @ w.double().t() + b.double()).clamp_min(0), gy.double().t() @ a.double(), gy.double().sum(0), gy.double() @ w.double()]
    for name, x, y, t, r, bound in zip(("nt", "tn", "bgrad", "nn"), first, again, timed, ref, (2e-6, 2e-5, 2e-5, 2e-5)):
        assert torch.equal(x, y), name
        assert G._rel(x, r) <= bound and G._rel(t, r) <= bound, name
