"""The dense kernels of the backbone and projection path -- csrc/pointwise.hip (bias / ReLU family, stem max-pool),
csrc/conv1x1_fused.hip (frozen bottleneck head / tail / tail with downsample), csrc/small_wgrad.hip (dW + db of the token linears),
csrc/groupnorm.hip -- where ``randn`` at a handful of shapes and a relative tolerance cannot see an error:

C1  the frozen bottleneck kernels on integer operands, ``torch.equal`` against float64 (tests/dense_reference.py: the exact-integer
    rule), at every strip / workgroup edge and past one grid pass, inputs followed by NaN rows, outputs surrounded by a sentinel;
C2  linear_wgrad the same way, over a list of row counts ASSERTED to reach every path of its software pipeline;
C3  the pointwise family past one grid pass (8,388,608 + 1,024 floats), exact;
C4  NaN / +Inf / -Inf through every ReLU site: the positions torch's composition gives, forward and backward;
C5  GroupNorm at the edges the deterministic-parity tests leave out, against float64 with a per-output, cancellation-aware bound.
C6  the column-sum family (colsum, colsum_any, colsum_strided, colsum_levels, sum_slices, relu_dropout_bwd_colsum): exact integers,
    canaries and poisoned scratch at every planner edge -- in tests/test_column_sums_gpu.py.
"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import dense_reference as R
import dropout_replay

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
EPS32 = torch.finfo(torch.float32).eps
PAD = 40                       # canary rows: more than one 32-row strip


def _lib():
    from monosowa_amd import pointwise
    return pointwise.load()


def _call(name, *args):
    from monosowa_amd._lib import raw_stream
    return getattr(_lib(), name)(*args, raw_stream())


def _p(t):
    return None if t is None else t.data_ptr()


# =====================================================================================================================================
# C1. frozen bottleneck kernels, exact
# =====================================================================================================================================
STRIP_EDGES = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257]            # 32-row strips, 8-strip (tail_ds: 16-strip) workgroups
WRAPPED = 131072 + 33                                               # 512 workgroups x 8 waves x 32 rows = one grid pass, and a partial strip
KINDS = ["head64", "head256", "tail", "tail_ds"]


def _conv_operands(kind, M, mode, seed):
    if kind.startswith("head"):
        return R.head_operands(M, int(kind[4:]), seed, mode, DEV)
    return R.tail_operands(M, seed, mode, DEV, downsample=kind == "tail_ds")


def _conv_want(kind, o):
    if kind.startswith("head"):
        return R.head64(o["x"], o["w"], o["b"])
    if kind == "tail":
        return R.tail64(o["x"], o["b_in"], o["w"], o["b_out"], o["res"])
    return R.tail_ds64(o["x"], o["b_in"], o["w"], o["x0"], o["wd"], o["b_out"])


def _conv_run(kind, o, y, M=None):
    """Launches ``kind`` on operands that are row-dense views (possibly inside canary buffers); returns the status code."""
    M = o["x"].shape[0] if M is None else M
    if kind.startswith("head"):
        return _call("mono_conv1x1_head_f32", _p(o["x"]), _p(o["w"]), _p(o["b"]), _p(y), M, o["x"].shape[1], 64)
    if kind == "tail":
        return _call("mono_conv1x1_tail_f32", _p(o["x"]), _p(o["b_in"]), _p(o["w"]), _p(o["b_out"]), _p(o["res"]), _p(y), M, 64, 256)
    return _call("mono_conv1x1_tail_ds_f32", _p(o["x"]), _p(o["b_in"]), _p(o["w"]), _p(o["x0"]), _p(o["wd"]), _p(o["b_out"]), _p(y), M, 64, 256)


def _conv_exact(kind, M, mode, seed):
    o = _conv_operands(kind, M, mode, seed)
    assert o["bound"] < R.EXACT_LIMIT
    want = _conv_want(kind, o).float()
    for k in ("x", "x0", "res"):                                     # NaN rows behind row M - 1: a result that used one turns NaN
        if k in o:
            o[k] = R.with_canary(o[k], PAD, 0, NAN)
    y = R.with_canary(torch.full(want.shape, R.SENTINEL, device=DEV), PAD, 0, R.SENTINEL, rows_before=PAD)
    assert _conv_run(kind, o, y) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(y).all(), "%d non-finite outputs: a row >= M was read" % int((~torch.isfinite(y)).sum())
    assert not (y == R.SENTINEL).any(), "%d outputs never written" % int((y == R.SENTINEL).sum())
    assert torch.equal(y, want), "%d of %d outputs differ, first at %s" % (int((y != want).sum()), y.numel(), (y != want).nonzero()[0].tolist())
    assert R.surroundings_hold(y, R.SENTINEL), "the kernel wrote outside its [M, N] output"
    return want


@pytest.mark.parametrize("M", STRIP_EDGES + [WRAPPED])
@pytest.mark.parametrize("kind", KINDS)
def test_bottleneck_kernels_are_exact_at_strip_edges_and_past_one_grid_pass(kind, M):
    want = _conv_exact(kind, M, "half", seed=M)
    if M >= 255:
        assert 0.3 < (want > 0).float().mean().item() < 0.7              # about half of the outputs clipped by the ReLU


@pytest.mark.parametrize("mode", ["dead", "alive"])
@pytest.mark.parametrize("kind", KINDS)
def test_bottleneck_kernels_all_dead_and_all_alive(kind, mode):
    want = _conv_exact(kind, 257, mode, seed=7)
    assert not want.any() if mode == "dead" else (want > 0).all()


def test_bottleneck_entry_points_refuse_what_they_do_not_serve():
    M = 64
    x, x256 = torch.zeros(M + 1, 64, device=DEV), torch.zeros(M + 1, 256, device=DEV)
    x0, res, y, y64 = torch.zeros_like(x), torch.zeros_like(x256), torch.zeros_like(x256), torch.zeros_like(x)
    w, wd, wh, wh256 = torch.zeros(64, 256, device=DEV), torch.zeros(64, 256, device=DEV), torch.zeros(64, 64, device=DEV), torch.zeros(256, 64, device=DEV)
    b_in, b_out = torch.zeros(64, device=DEV), torch.zeros(256, device=DEV)
    p = lambda t: t.data_ptr()
    tail = lambda *a: _call("mono_conv1x1_tail_f32", *a)
    good = [p(x), p(b_in), p(w), p(b_out), p(res), p(y), M, 64, 256]
    assert tail(*good) == 0
    # aliasing: the operands are __restrict__ and res is read a channel block ahead of the stores to y
    assert tail(p(x), p(b_in), p(w), p(b_out), p(y), p(y), M, 64, 256) == -2          # y == res
    assert tail(p(x256), p(b_in), p(w), p(b_out), p(res), p(x256), M, 64, 256) == -2  # y == x
    for K, N in ((128, 256), (256, 256), (64, 64), (64, 128), (0, 256)):
        assert tail(*good[:7], K, N) == -2
    assert tail(*good[:6], 0, 64, 256) == -2 and tail(*good[:6], -5, 64, 256) == -2
    for i in range(6):                                                                # null pointers, one at a time
        assert tail(*[None if j == i else a for j, a in enumerate(good)]) == -1
    for i in (0, 2, 4, 5):                                                            # x, w, res, y 4 bytes off a 16-byte boundary
        assert tail(*[a + 4 if j == i else a for j, a in enumerate(good)]) == -2

    ds = lambda *a: _call("mono_conv1x1_tail_ds_f32", *a)
    good = [p(x), p(b_in), p(w), p(x0), p(wd), p(b_out), p(y), M, 64, 256]
    assert ds(*good) == 0
    assert ds(p(x256), p(b_in), p(w), p(x0), p(wd), p(b_out), p(x256), M, 64, 256) == -2      # y == x
    assert ds(p(x), p(b_in), p(w), p(x256), p(wd), p(b_out), p(x256), M, 64, 256) == -2       # y == x0
    for K, N in ((128, 256), (64, 64), (256, 256)):
        assert ds(*good[:8], K, N) == -2
    assert ds(*good[:7], 0, 64, 256) == -2
    for i in range(7):
        assert ds(*[None if j == i else a for j, a in enumerate(good)]) == -1
    for i in (0, 2, 3, 4, 6):
        assert ds(*[a + 4 if j == i else a for j, a in enumerate(good)]) == -2

    head = lambda *a: _call("mono_conv1x1_head_f32", *a)
    good = [p(x), p(wh), p(b_in), p(y64), M, 64, 64]
    assert head(*good) == 0 and head(p(x256), p(wh256), p(b_in), p(y64), M, 256, 64) == 0
    for K, N in ((128, 64), (32, 64), (64, 256), (256, 32), (0, 64)):
        assert head(*good[:5], K, N) == -2
    assert head(*good[:4], 0, 64, 64) == -2
    for i in range(4):
        assert head(*[None if j == i else a for j, a in enumerate(good)]) == -1
    for i in (0, 1, 3):
        assert head(*[a + 4 if j == i else a for j, a in enumerate(good)]) == -2
    torch.cuda.synchronize()


# =====================================================================================================================================
# C2. linear_wgrad, exact
# =====================================================================================================================================
WG_SHAPES = [(64, 64), (128, 192), (192, 64), (256, 256)]
WG_ROWS = [64, 65, 66, 79, 80, 81, 127, 128, 129, 143, 256, 384, 512, 640, 768, 896, 897, 911, 1024, 1025, 2049]


def _splits(Rr, M, N):
    ws = _lib().mono_linear_wgrad_workspace(Rr, M, N)
    assert ws > 0 and ws % (M * N + M) == 0
    return R.wgrad_splits(Rr, ws // (M * N + M))


def test_wgrad_case_list_reaches_every_path_of_the_pipeline():
    """n_stages 0 .. 8 per split, each remainder-chain length behind a full group of four, tails of 0 / 1 / 2 / 15 rows, an empty
    trailing split and a split that is tail only: with the launcher's own split count S (read off its workspace size)."""
    lists = [_splits(Rr, M, N) for M, N in WG_SHAPES for Rr in WG_ROWS]
    for (M, N), Rr, sp in zip([s for s in WG_SHAPES for _ in WG_ROWS], WG_ROWS * len(WG_SHAPES), lists):
        assert sum(16 * a + b for a, b in sp) == Rr, (M, N, Rr, sp)
    missing = R.WGRAD_REQUIRED - R.wgrad_coverage(lists)
    assert not missing, "the case list misses %s" % sorted(missing)


@pytest.mark.parametrize("Rr", WG_ROWS)
@pytest.mark.parametrize("M,N", WG_SHAPES)
def test_wgrad_is_exact_on_integers(M, N, Rr):
    from monosowa_amd.pointwise import linear_wgrad, linear_wgrad_applies
    o = R.wgrad_operands(Rr, M, N, seed=Rr + M, device=DEV)
    assert o["bound"] == 9 * Rr < R.EXACT_LIMIT
    want_w, want_b = (t.float() for t in R.wgrad64(o["dy"], o["x"]))
    gw, gb = linear_wgrad(o["dy"], o["x"], True)
    assert gw.shape == (M, N) and gb.shape == (M,)
    assert torch.equal(gw, want_w), "dW: %d of %d entries differ" % (int((gw != want_w).sum()), gw.numel())
    assert torch.equal(gb, want_b), "db: %d entries differ" % int((gb != want_b).sum())
    gw, gb = linear_wgrad(o["dy"], o["x"], False)
    assert gb is None and torch.equal(gw, want_w)
    # views of wider, longer matrices: hidden columns and the rows behind R hold NaN
    dy, x = R.with_canary(o["dy"], 16, 32, NAN), R.with_canary(o["x"], 16, 64, NAN)
    assert dy.stride(0) == M + 32 and x.stride(0) == N + 64 and linear_wgrad_applies(dy, x)
    gw, gb = linear_wgrad(dy, x, True)
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all(), "a hidden column or a row behind R was read"
    assert torch.equal(gw, want_w) and torch.equal(gb, want_b)


# =====================================================================================================================================
# C3. the pointwise family past one grid pass, exact
# =====================================================================================================================================
BIG = 8388608 + 1024                        # grid_for_vec caps the grid at 8192 x 256 float4 = 8,388,608 floats: one more pass of 256 float4
PW_SHAPES = [(BIG // 4, 4), (BIG // 64, 64), (BIG // 256, 256), (1, 4)]          # (pixels, channels); [1, 4, 1, 1] is the odd small one


@functools.lru_cache(maxsize=None)
def _pw(rows, C):
    """Integer operands of one shape, drawn once and left unchanged (the in-place kernels get clones)."""
    o = R.pointwise_operands(rows, C, seed=C, device=DEV)
    o["scale"] = R.pow2_scales(C, seed=C + 1, device=DEV)
    return o


def _nhwc_clone(rows2d, requires_grad=False):
    """A fresh channels-last [1, C, 1, rows] tensor with the values of ``rows2d``; with ``requires_grad`` a NON-leaf one (the kernels
    work in place, like on a convolution's output) together with its leaf."""
    leaf = R.as_nhwc(rows2d.clone())
    if not requires_grad:
        return leaf
    leaf.requires_grad_(True)
    return leaf.clone(), leaf


def _rows(t4):
    return t4.permute(0, 2, 3, 1).reshape(-1, t4.shape[1])


@pytest.mark.parametrize("rows,C", PW_SHAPES)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
def test_bias_act_is_exact_past_one_grid_pass(rows, C, with_res, relu):
    from monosowa_amd.pointwise import bias_act
    o = _pw(rows, C)
    y = _nhwc_clone(o["y"])
    with torch.no_grad():
        out = bias_act(y, o["bias"], R.as_nhwc(o["res"]) if with_res else None, relu)
    assert out.data_ptr() == y.data_ptr()                          # the HIP path: in place
    want = R.bias_act64(o["y"], o["bias"], o["res"] if with_res else None, relu).float()
    assert torch.equal(_rows(out), want)


@contextlib.contextmanager
def _relu_mask(on):
    from monosowa_amd import pointwise
    was = pointwise.USE_RELU_MASK
    pointwise.USE_RELU_MASK = on
    try:
        yield
    finally:
        pointwise.USE_RELU_MASK = was


@pytest.mark.parametrize("rows,C", PW_SHAPES)
@pytest.mark.parametrize("use_mask", [True, False])
def test_bias_relu_forward_under_grad_and_its_backward_are_exact(rows, C, use_mask):
    """bias_relu_mask + relu_grad_mask (byte mask) / bias_act + relu_grad (mask read off the output)."""
    from monosowa_amd.pointwise import bias_act
    o = _pw(rows, C)
    pre = o["y"].double() + o["bias"].double() + o["res"].double()
    assert (pre == 0).any() or rows == 1                           # exact zeros in front of the ReLU: mask bit 0, gradient 0
    with _relu_mask(use_mask):
        y, leaf = _nhwc_clone(o["y"], True)
        res = R.as_nhwc(o["res"].clone()).requires_grad_(True)
        out = bias_act(y, o["bias"], res, True)
        assert torch.equal(_rows(out.detach()), torch.relu(pre).float())
        out.backward(R.as_nhwc(o["grads"][0]))
    want = R.relu_backward64(pre, o["grads"][0]).float()
    assert torch.equal(_rows(leaf.grad), want) and torch.equal(_rows(res.grad), want)


@pytest.mark.parametrize("rows,C", PW_SHAPES)
@pytest.mark.parametrize("n_out", [2, 3])
@pytest.mark.parametrize("use_mask", [True, False])
def test_bias_act_fork_and_its_backward_are_exact(rows, C, n_out, use_mask):
    """bias_relu_mask + relu_grad_mask<TWO> / relu_grad_mask3 (byte mask), bias_act + relu_grad2 (without)."""
    from monosowa_amd.pointwise import bias_act_fork
    o = _pw(rows, C)
    pre = o["y"].double() + o["bias"].double() + o["res"].double()
    with _relu_mask(use_mask):
        y, leaf = _nhwc_clone(o["y"], True)
        res = R.as_nhwc(o["res"].clone()).requires_grad_(True)
        outs = bias_act_fork(y, o["bias"], res, n_out)
        assert len(outs) == n_out and all(t.data_ptr() == y.data_ptr() for t in outs)
        assert torch.equal(_rows(outs[0].detach()), torch.relu(pre).float())
        torch.autograd.backward(list(outs), [R.as_nhwc(g) for g in o["grads"][:n_out]])
    want = R.relu_backward64(pre, sum(g.double() for g in o["grads"][:n_out])).float()
    assert torch.equal(_rows(leaf.grad), want) and torch.equal(_rows(res.grad), want)


@pytest.mark.parametrize("rows,C", PW_SHAPES)
def test_affine_relu_and_its_backward_are_exact(rows, C):
    from monosowa_amd.pointwise import affine_relu, affine_relu_supported
    o = _pw(rows, C)
    y, leaf = _nhwc_clone(o["y"], True)
    assert affine_relu_supported(y, o["scale"])
    out = affine_relu(y, o["scale"], o["bias"])
    pre = o["y"].double() * o["scale"].double() + o["bias"].double()             # power-of-two scales: exact
    assert torch.equal(_rows(out.detach()), torch.relu(pre).float())
    out.backward(R.as_nhwc(o["grads"][0]))
    assert torch.equal(_rows(leaf.grad), (R.relu_backward64(pre, o["grads"][0]) * o["scale"].double()).float())


@pytest.mark.parametrize("rows,C", PW_SHAPES)
def test_relu_grad_from_output_is_exact(rows, C):
    """relu_grad / relu_grad2 / relu_grad3 / relu_grad_scale on a ReLU output (zeros included)."""
    from monosowa_amd.pointwise import relu_grad_from_output
    o = _pw(rows, C)
    out2d = torch.relu(o["y"] + o["bias"])
    out, grads = R.as_nhwc(out2d), [R.as_nhwc(g) for g in o["grads"]]
    for n in (1, 2, 3):
        got = relu_grad_from_output(grads[:n], out)
        assert torch.equal(_rows(got), R.relu_backward64(out2d.double(), sum(g.double() for g in o["grads"][:n])).float()), n
    got = relu_grad_from_output(grads[:1], out, o["scale"])
    assert torch.equal(_rows(got), (R.relu_backward64(out2d.double(), o["grads"][0]) * o["scale"].double()).float())


@pytest.mark.parametrize("shape", [(1, 64, 725, 725), (2, 4, 5, 7), (1, 8, 1, 1), (3, 4, 2, 3), (1, 4, 6, 1)])
def test_bias_relu_maxpool_is_exact(shape):
    """[1, 64, 725, 725]: 363 x 363 x 16 = 2,108,304 output float4 > 8192 x 256, odd height and width."""
    from monosowa_amd.pointwise import bias_relu_maxpool, bias_relu_maxpool_supported
    g = torch.Generator(device=DEV).manual_seed(shape[2])
    y = R.ints(shape, -R.VEC_MAX, R.VEC_MAX, g, DEV).contiguous(memory_format=torch.channels_last)
    bias = R.ints((shape[1],), -R.VEC_MAX, R.VEC_MAX, g, DEV)
    assert bias_relu_maxpool_supported(y, bias)
    got = bias_relu_maxpool(y, bias)
    want = R.bias_relu_maxpool64(y, bias).float()
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got, want)
    if shape[0] == 1 and shape[2] == 725:
        assert got.numel() // 4 > 8192 * 256


# =====================================================================================================================================
# C4. non-finite propagation
# =====================================================================================================================================
NF_ROWS, NF_C = 33, 8                        # 264 floats = 66 float4


def _nf_positions(n):
    """One NaN, one +Inf, one -Inf: the second element, the middle, and the very last element (the last vector)."""
    return [1, n // 2, n - 1]


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("planted_in,with_res", [("y", False), ("y", True), ("res", True)])
def test_bias_act_propagates_nonfinite(planted_in, with_res, relu):
    from monosowa_amd.pointwise import bias_act
    o = R.pointwise_operands(NF_ROWS, NF_C, seed=3, device=DEV)
    src = {k: o[k].clone() for k in ("y", "res")}
    R.plant(src[planted_in], _nf_positions(NF_ROWS * NF_C))
    if with_res:                                                   # Inf + (-Inf) = NaN where the other addend is the opposite infinity
        other = "res" if planted_in == "y" else "y"
        src[other].view(-1)[NF_ROWS * NF_C // 2 + 1] = -INF
        src[planted_in].view(-1)[NF_ROWS * NF_C // 2 + 1] = INF
    with torch.no_grad():
        out = bias_act(_nhwc_clone(src["y"]), o["bias"], R.as_nhwc(src["res"]) if with_res else None, relu)
    want = R.bias_act64(src["y"], o["bias"], src["res"] if with_res else None, relu)
    assert torch.isnan(want).sum() >= 1 and R.same_nonfinite(_rows(out), want)


@pytest.mark.parametrize("use_mask", [True, False])
@pytest.mark.parametrize("fork", [0, 2, 3])
def test_bias_relu_backward_passes_the_gradient_where_torch_does(fork, use_mask):
    """Forward under grad (byte-mask variants and the plain one) and the ReLU backward, against torch autograd in float64: the
    gradient passes at a NaN (and +Inf) output and is 0 at -Inf and at exactly 0."""
    from monosowa_amd.pointwise import bias_act, bias_act_fork
    o = R.pointwise_operands(NF_ROWS, NF_C, seed=4, device=DEV)
    y0 = R.plant(o["y"].clone(), _nf_positions(NF_ROWS * NF_C))
    n = max(fork, 1)
    y64, r64 = y0.double().requires_grad_(True), o["res"].double().requires_grad_(True)
    ref = torch.relu(y64 + o["bias"].double() + r64)
    ref.backward(sum(g.double() for g in o["grads"][:n]))
    with _relu_mask(use_mask):
        y, leaf = _nhwc_clone(y0, True)
        res = R.as_nhwc(o["res"].clone()).requires_grad_(True)
        outs = bias_act_fork(y, o["bias"], res, fork) if fork else (bias_act(y, o["bias"], res, True),)
        assert R.same_nonfinite(_rows(outs[0].detach()), ref.detach())
        torch.autograd.backward(list(outs), [R.as_nhwc(g) for g in o["grads"][:n]])
    assert R.same_nonfinite(_rows(leaf.grad), y64.grad) and R.same_nonfinite(_rows(res.grad), r64.grad)


def test_affine_relu_propagates_nonfinite():
    from monosowa_amd.pointwise import affine_relu
    o = R.pointwise_operands(NF_ROWS, NF_C, seed=5, device=DEV)
    scale = torch.tensor([1.0, 0.0, -2.0, 0.5, 0.0, 4.0, -1.0, 0.0], device=DEV)        # zeros: Inf * 0 = NaN in both evaluations
    y0 = o["y"].clone()
    for c in range(NF_C):                                                                # every channel meets NaN, +Inf and -Inf
        y0[1, c], y0[NF_ROWS // 2, c], y0[NF_ROWS - 1, c] = NAN, INF, -INF
    y64 = y0.double().requires_grad_(True)
    ref = torch.relu(y64 * scale.double() + o["bias"].double())
    ref.backward(o["grads"][0].double())
    y, leaf = _nhwc_clone(y0, True)
    out = affine_relu(y, scale, o["bias"])
    assert R.same_nonfinite(_rows(out.detach()), ref.detach())
    out.backward(R.as_nhwc(o["grads"][0]))
    assert R.same_nonfinite(_rows(leaf.grad), y64.grad)


def test_relu_grad_from_output_passes_the_gradient_at_nonfinite_outputs():
    from monosowa_amd.pointwise import relu_grad_from_output
    o = R.pointwise_operands(NF_ROWS, NF_C, seed=6, device=DEV)
    out2d = R.plant(torch.relu(o["y"] + o["bias"]), [1, NF_ROWS * NF_C // 2], (NAN, INF))
    scale = R.pow2_scales(NF_C, seed=2, device=DEV)
    for n in (1, 2, 3):
        got = relu_grad_from_output([R.as_nhwc(g) for g in o["grads"][:n]], R.as_nhwc(out2d))
        assert R.same_nonfinite(_rows(got), R.relu_backward64(out2d.double(), sum(g.double() for g in o["grads"][:n])))
    got = relu_grad_from_output([R.as_nhwc(o["grads"][0])], R.as_nhwc(out2d), scale)
    assert R.same_nonfinite(_rows(got), R.relu_backward64(out2d.double(), o["grads"][0]) * scale.double())


def test_bias_relu_maxpool_propagates_nonfinite():
    from monosowa_amd.pointwise import bias_relu_maxpool
    g = torch.Generator(device=DEV).manual_seed(0)
    y = R.ints((2, 8, 9, 11), -R.VEC_MAX, R.VEC_MAX, g, DEV).contiguous(memory_format=torch.channels_last)
    bias = R.ints((8,), -R.VEC_MAX, R.VEC_MAX, g, DEV)
    y[0, 0, 3, 3], y[0, 1, 2, 2], y[0, 2, 4, 4] = NAN, INF, -INF               # tap of four windows / centre of one / never a maximum
    y[1, 7, 8, 10], y[1, 6, 8, 10], y[1, 5, 0, 0] = NAN, INF, NAN              # the last pixel of the last image (last vector), a corner
    y[1, 3, 4, 5], y[1, 3, 4, 6] = INF, NAN                                    # NaN beside +Inf in one window: NaN wins
    want = R.bias_relu_maxpool64(y, bias)
    assert torch.isnan(want).sum() >= 7 and torch.isposinf(want).sum() >= 2
    assert R.same_nonfinite(bias_relu_maxpool(y, bias), want)


def _conv_nf(kind, planted_in):
    M = 70                                                                      # rows 64 .. 69: the last, partial strip
    o = _conv_operands(kind, M, "half", seed=11)
    g = torch.Generator(device=DEV).manual_seed(12)
    for k in ("w", "wd"):
        if k in o:                                                              # a third of the weights zero: Inf * 0 = NaN in both evaluations
            o[k][R.ints(o[k].shape, 0, 2, g, DEV) == 0] = 0.0
    t = o[planted_in]
    C = t.shape[1]
    t[3, 5], t[40, C - 1], t[M - 1, 0] = NAN, INF, -INF
    t[41, 0], t[41, 3] = INF, INF                                               # two infinities meeting in one sum
    t[66, 1], t[66, 2] = INF, -INF
    want = _conv_want(kind, o)
    y = torch.full(want.shape, R.SENTINEL, device=DEV)
    assert _conv_run(kind, o, y) == 0
    return y, want


@pytest.mark.parametrize("kind,planted_in", [("head64", "x"), ("head256", "x"), ("tail", "x"), ("tail", "res"), ("tail_ds", "x"), ("tail_ds", "x0")])
def test_bottleneck_kernels_propagate_nonfinite(kind, planted_in):
    y, want = _conv_nf(kind, planted_in)
    assert torch.isnan(want).any() and torch.isposinf(want).any() and not torch.isneginf(want).any()
    assert R.same_nonfinite(y, want)


GN_C0_FWD, GN_C0_GX, GN_C0_GG = 4.0, 10.0, 4.0          # see test_group_norm_edges_against_float64


def _gn_product(x, gn, relu, pb, gy, det):
    """The product's forward and backward (optionally in deterministic mode, switched on around the product's calls only)."""
    from monosowa_amd import pointwise
    was, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    xg = x.clone().requires_grad_(True)
    pbg = pb.clone().requires_grad_(True) if pb is not None else None
    gn.weight.grad = gn.bias.grad = None
    torch.use_deterministic_algorithms(det)
    try:
        assert pointwise.DETERMINISTIC.sync() is det
        y = pointwise.group_norm(xg, gn, relu=relu, pre_bias=pbg)
        assert y.grad_fn is not None and "GroupNormNHWC" in type(y.grad_fn).__name__
        y.backward(gy)
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn_only)
        pointwise.DETERMINISTIC.sync()
    return y.detach(), xg.grad, gn.weight.grad.clone(), gn.bias.grad.clone(), (pbg.grad if pb is not None else None)


def _gn_reference(x, gn, relu, pb, gy, dtype=torch.float64):
    leaf = lambda t: t.detach().to(dtype).contiguous().clone().requires_grad_(True)
    x64, w64, b64 = leaf(x), leaf(gn.weight), leaf(gn.bias)
    pb64 = leaf(pb) if pb is not None else None
    y = F.group_norm(x64 if pb is None else x64 + pb64.view(1, -1, 1, 1), 32, w64, b64, gn.eps)
    y = torch.relu(y) if relu else y
    y.backward(gy.to(dtype).contiguous())
    return y.detach(), x64.grad, w64.grad, b64.grad, (pb64.grad if pb is not None else None)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("with_pre_bias", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_group_norm_propagates_nonfinite(relu, with_pre_bias, det):
    """One NaN / +Inf / -Inf makes its 8-channel x HW group NaN (F.group_norm), a ReLU behind it keeps the NaN; every returned
    gradient is non-finite exactly where torch's is.  Finite outputs within the bound of C5."""
    g = torch.Generator(device=DEV).manual_seed(1)
    B, H, W = 2, 7, 10                                                          # 70 pixels: two workgroups of 64
    x = torch.randn(B, 256, H, W, generator=g, device=DEV).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(B, 256, H, W, generator=g, device=DEV).contiguous(memory_format=torch.channels_last)
    x[0, 8, 0, 1] = NAN                                                         # image 0, group 1
    x[1, 255, H - 1, W - 1] = INF                                               # image 1, group 31: the last element (second workgroup)
    x[1, 3, 3, 3] = -INF                                                        # image 1, group 0
    x[0, 40, 2, 2], x[0, 41, 6, 9] = INF, -INF                                  # both infinities in one group (image 0, group 5)
    gn = torch.nn.GroupNorm(32, 256).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(256, generator=g, device=DEV))
        gn.bias.copy_(torch.randn(256, generator=g, device=DEV))
        gn.weight[9] = gn.weight[250] = gn.weight[100] = 0.0                    # NaN * 0 = NaN inside broken groups; a zero in a sound one
    pb = torch.randn(256, generator=g, device=DEV) if with_pre_bias else None
    got = _gn_product(x, gn, relu, pb, gy, det)
    want = _gn_reference(x, gn, relu, pb, gy)
    broken = torch.zeros(B, 256, dtype=torch.bool, device=DEV)
    broken[0, 8:16] = broken[1, 248:256] = broken[1, 0:8] = broken[0, 40:48] = True
    assert torch.equal(torch.isnan(want[0]).all(-1).all(-1), broken)           # the oracle: whole groups NaN, nothing else
    xs = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    scale = R.group_norm_error_scale(xs, gn.weight.detach(), gn.bias.detach(), gn.eps, pre_bias=pb)
    scale = torch.where(broken[:, :, None, None], torch.zeros_like(scale), scale)
    assert R.same_nonfinite(got[0], want[0], bound=GN_C0_FWD * EPS32 * scale)
    for name, a, b in zip(("gx", "ggamma", "gbeta", "gbias"), got[1:], want[1:]):
        if a is None:
            assert b is None
            continue
        assert torch.equal(~torch.isfinite(a), ~torch.isfinite(b)), "%s: non-finite at %d places, torch at %d" % (
            name, int((~torch.isfinite(a)).sum()), int((~torch.isfinite(b)).sum()))
        assert torch.equal(torch.isnan(a), torch.isnan(b)), name


def test_relu_dropout_propagates_nonfinite_in_training():
    """dropout(relu(h)) in train mode with the kernel's own keep mask (tests/dropout_replay.py), p = 1/2 (scale 2: exact on integers).
    A NaN stays NaN kept or dropped (NaN * 0), a dropped +Inf becomes NaN (Inf * 0), -Inf becomes 0: torch's table.
    Backward (relu_dropout_bwd, and relu_dropout_bwd_colsum with its column sums): equal to autograd everywhere except at DROPPED
    elements whose output is NaN, which are left out of the comparison -- the backward kernels read the mask off the output, and a
    NaN output does not say whether the element was kept (finite on both sides; the activation is NaN there)."""
    from monosowa_amd import pointwise
    g = torch.Generator(device=DEV).manual_seed(2)
    h = R.ints((64, 256), -R.VEC_MAX, R.VEC_MAX, g, DEV)
    gy = R.ints((64, 256), -R.VEC_MAX, R.VEC_MAX, g, DEV)
    n = h.numel()
    h.view(-1)[0:32] = NAN
    h.view(-1)[n // 2:n // 2 + 32] = INF
    h.view(-1)[n - 32:] = -INF
    h.view(-1)[n - 64:n - 32] = NAN                                             # the last vectors but the -Inf ones
    hg = h.clone().requires_grad_(True)
    with dropout_replay.record() as draws:
        y = pointwise._ReluDropout.apply(hg, 0.5)
    y.backward(gy)
    mask = draws[0].mask().double()                                             # keep / (1 - p): 0 or 2
    assert set(mask.unique().tolist()) == {0.0, 2.0}
    h64 = h.double().requires_grad_(True)
    ref = torch.relu(h64) * mask
    ref.backward(gy.double())
    assert torch.isnan(ref[0, :32]).all() and torch.isnan(ref).sum() > 64 and torch.isposinf(ref).sum() > 0
    assert R.same_nonfinite(y.detach(), ref.detach())
    dropped_nan = torch.isnan(ref.detach()) & (mask == 0)
    assert dropped_nan.any() and (~dropped_nan & torch.isnan(ref.detach())).any()
    outside = lambda t: torch.where(dropped_nan, torch.zeros_like(t), t)
    assert R.same_nonfinite(outside(hg.grad), outside(h64.grad))
    gh, colsum = pointwise.relu_dropout_backward_colsum(gy, y.detach(), 0.5)
    assert R.same_nonfinite(outside(gh), outside(h64.grad))
    assert torch.isfinite(gh).all() and torch.equal(colsum, gh.double().sum(0).float())          # small integers: the sums are exact


def test_relu_dropout_propagates_nonfinite_in_eval():
    """In eval mode (and below RELU_DROPOUT_MIN_NUMEL) ``relu_dropout`` is ``dropout(torch.relu(h))`` itself: no kernel of the library
    runs.  This only pins that the wrapper's fall-through keeps torch's table."""
    from monosowa_amd.pointwise import relu_dropout
    h = R.plant(torch.arange(-512.0, 512.0, device=DEV).reshape(4, 256), _nf_positions(1024))
    got = relu_dropout(h, torch.nn.Dropout(0.1).eval())
    assert R.same_nonfinite(got, torch.relu(h.double()))


# =====================================================================================================================================
# C5. GroupNorm edges
# =====================================================================================================================================
def _units(got, want, scale):
    """max over the outputs of |got - want| / (eps32 * scale): the error in units of one float32 rounding of the terms' magnitude."""
    err = (got.double() - want.double()).abs()
    live = scale > 0
    return (err[live] / (EPS32 * scale[live])).max().item() if live.any() else 0.0


@pytest.mark.parametrize("HW", [1, 2, 3, 5, 63, 64, 65, 129])
@pytest.mark.parametrize("B", [1, 5])
def test_group_norm_edges_against_float64(B, HW):
    """Per-output bound  c * eps32 * sum|terms|  (tests/dense_reference.py group_norm_error_scale for y; below for the gradients), with
    c = max(what float32 F.group_norm shows on the same input, C0):
      y      C0 = 4:  roundings of x + pre_bias, of the float32 mean, of the difference, of rstd, of rstd * gamma, of the product and
                      of + beta -- seven half-units = 3.5; the statistics themselves are float64.
      gx     C0 = 10: gx = rstd (gy gamma - bs - xhat a): xhat carries 2 units ((|x| + |mean|) rstd: mean rounding, difference,
                      rstd, product), `a` inherits them as a mean and adds its cast, then product, two differences, the outer product
                      and gy gamma's own rounding: 2 + 2.5 + 4 x 0.5 + ... < 10.
      ggamma C0 = 4:  sum gy xhat accumulated in float64: xhat's 2 units and the final cast; gbeta: the cast alone.
      gbias  the sum of gx in float32: gx's C0 plus half a unit per addition on the longest chain (a lane's pixels, the four waves, the
                      workgroups' partial rows).
    Measured on an MI355X (maximum over the 16 cases, kernel / torch float32): y 1.48 / 5.55, gx 1.22 / 1.59, ggamma 1.03 / 1.74,
    gbeta 0.47 / 0.73, gbias 0.23 / 0.43 -- the kernel is below torch's float32 path everywhere and at a third or less of each C0.
    Because c is the LARGER of the two, the bound in force for y is torch's own figure wherever that exceeds C0 (5.48 units at HW = 63,
    5.55 at HW = 129 with B = 1) and C0 = 4 elsewhere; for every gradient torch stays below C0, so C0 is the bound in force.
    Cases: a group constant over the image (variance 0: y = beta exactly as far as these bounds say, xhat = 0, rstd = eps^-1/2),
    gamma = 0 on some channels, one pixel of 1e4 among ones.  B = 5 runs with pre_bias, B = 1 without."""
    g = torch.Generator(device=DEV).manual_seed(100 * B + HW)
    x = torch.randn(B, 256, 1, HW, generator=g, device=DEV)
    x[0, 0:8] = 3.0                                                             # image 0, group 0: constant
    x[B - 1, 16:24] = 1.0
    x[B - 1, 17, 0, HW // 2] = 1e4                                              # last image, group 2: a one-pixel outlier among ones
    x = x.contiguous(memory_format=torch.channels_last)
    gy = torch.randn(B, 256, 1, HW, generator=g, device=DEV).contiguous(memory_format=torch.channels_last)
    gn = torch.nn.GroupNorm(32, 256).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(torch.randn(256, generator=g, device=DEV))
        gn.bias.copy_(torch.randn(256, generator=g, device=DEV))
        gn.weight[4] = gn.weight[32:40] = gn.weight[255] = 0.0
    pb = torch.zeros(256, device=DEV) if B == 5 else None                       # (zero on the constant group: x + pre_bias stays constant)
    if pb is not None:
        pb[8:] = torch.randn(248, generator=g, device=DEV)
    got = _gn_product(x, gn, False, pb, gy, False)
    want = _gn_reference(x, gn, False, pb, gy)
    t32 = _gn_reference(x, gn, False, pb, gy, torch.float32)                    # PyTorch's own float32 path (NCHW)
    gamma, beta = gn.weight.detach().double(), gn.bias.detach().double()
    # sum|terms| per output
    s_y = R.group_norm_error_scale(x, gamma, beta, gn.eps, pre_bias=pb)
    v = x.double() if pb is None else x.double() + pb.double().view(1, -1, 1, 1)
    mag = x.double().abs() if pb is None else x.double().abs() + pb.double().abs().view(1, -1, 1, 1)
    grp = lambda t: t.reshape(B, 32, -1)
    mean = grp(v).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((grp(v) - mean) ** 2).mean(-1, keepdim=True) + gn.eps)
    xh_mag = (grp(mag) + mean.abs()) * rstd                                     # >= |xhat|: the terms of x - mean, scaled
    t_abs = grp((gy.double() * gamma.view(1, -1, 1, 1)).abs())
    s_gx = (rstd * (t_abs + t_abs.mean(-1, keepdim=True) + xh_mag * (t_abs * xh_mag).mean(-1, keepdim=True))).reshape(x.shape)
    s_gg = (gy.double().abs() * xh_mag.reshape(x.shape)).sum((0, 2, 3))
    s_gb = gy.double().abs().sum((0, 2, 3))
    scales = (s_y, s_gx, s_gg, s_gb, s_gx.sum((0, 2, 3)))
    adds = -(-min(HW, 64) // 4) + 3 + B * -(-HW // 64)
    floors = (GN_C0_FWD, GN_C0_GX, GN_C0_GG, GN_C0_GG, GN_C0_GX + 0.5 * adds)
    report, failed = [], []
    for name, a, w, t, s, c0 in zip(("y", "gx", "ggamma", "gbeta", "gbias"), got, want, t32, scales, floors):
        if a is None:
            continue
        assert torch.isfinite(a).all(), name
        mine, torchs = _units(a, w, s), _units(t, w, s)
        report.append("%s kernel %.2f torch-f32 %.2f" % (name, mine, torchs))
        if mine > max(torchs, c0):
            failed.append(name)
    print("group_norm B=%d HW=%d error in eps32 * sum|terms|: %s" % (B, HW, "; ".join(report)))
    assert not failed, "%s above max(torch float32, C0): %s" % (failed, "; ".join(report))
    # the constant group: y = beta and gx = 0 up to the same bounds (checked above); and exactly no NaN from 0 * rstd
    assert (got[0][0, 0:8].double() - beta[0:8].view(8, 1, 1)).abs().max().item() <= GN_C0_FWD * EPS32 * s_y[0, 0:8].max().item()
