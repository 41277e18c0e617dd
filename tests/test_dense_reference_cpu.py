"""The oracle of tests/test_dense_kernels_gpu.py, checked on its own (no GPU):
- every integer generator of tests/dense_reference.py evaluates bit for bit the same in float32 and float64 -- the cap that makes
  ``torch.equal`` against float64 a legitimate demand on a float32 kernel;
- the plain float64 formulas equal torch's own operators and autograd;
- the NaN / Inf behaviour of the PyTorch compositions the kernels stand for, pinned as a table."""
import math

import pytest
import torch
import torch.nn.functional as F

import dense_reference as R

NAN, INF = float("nan"), float("inf")


# ---- 1. float32 == float64 on every generator ------------------------------------------------------------------------------------
def _both(formula32, formula64):
    a, b = formula32(), formula64()
    assert a.dtype == torch.float32 and b.dtype == torch.float64
    assert torch.equal(a.double(), b), "float32 evaluation differs from float64 at %d places" % int((a.double() != b).sum())


@pytest.mark.parametrize("mode", ["half", "dead", "alive"])
@pytest.mark.parametrize("K", [64, 256])
def test_head_operands_are_exact_in_float32(K, mode):
    o = R.head_operands(257, K, seed=1, mode=mode)
    assert o["bound"] < R.EXACT_LIMIT
    _both(lambda: torch.relu(o["x"] @ o["w"] + o["b"]), lambda: R.head64(o["x"], o["w"], o["b"]))
    # summed in another order (the kernel contracts k = s and k = K/2 + s together): still the same integers
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(0))
    _both(lambda: torch.relu(o["x"][:, perm] @ o["w"][perm] + o["b"]), lambda: R.head64(o["x"], o["w"], o["b"]))
    out = R.head64(o["x"], o["w"], o["b"])
    if mode == "dead":
        assert not out.any()
    elif mode == "alive":
        assert (out > 0).all()
    else:
        assert 0.3 < (out > 0).double().mean().item() < 0.7


@pytest.mark.parametrize("mode", ["half", "dead", "alive"])
@pytest.mark.parametrize("downsample", [False, True])
def test_tail_operands_are_exact_in_float32(downsample, mode):
    o = R.tail_operands(257, seed=2, mode=mode, downsample=downsample)
    assert o["bound"] < R.EXACT_LIMIT
    hidden = torch.relu(o["x"] + o["b_in"])
    if downsample:
        _both(lambda: torch.relu(hidden @ o["w"] + o["x0"] @ o["wd"] + o["b_out"]),
              lambda: R.tail_ds64(o["x"], o["b_in"], o["w"], o["x0"], o["wd"], o["b_out"]))
        out = R.tail_ds64(o["x"], o["b_in"], o["w"], o["x0"], o["wd"], o["b_out"])
    else:
        _both(lambda: torch.relu(hidden @ o["w"] + o["b_out"] + o["res"]),
              lambda: R.tail64(o["x"], o["b_in"], o["w"], o["b_out"], o["res"]))
        _both(lambda: torch.relu((o["res"] + o["b_out"]) + hidden @ o["w"]),             # another order of the addends
              lambda: R.tail64(o["x"], o["b_in"], o["w"], o["b_out"], o["res"]))
        out = R.tail64(o["x"], o["b_in"], o["w"], o["b_out"], o["res"])
    assert 0.3 < (o["x"] + o["b_in"] < 0).double().mean().item() < 0.7             # about half of the hidden ReLU's inputs negative
    if mode == "dead":
        assert not out.any()
    elif mode == "alive":
        assert (out > 0).all()
    else:
        assert 0.3 < (out > 0).double().mean().item() < 0.7


def test_wgrad_operands_are_exact_in_float32():
    o = R.wgrad_operands(2200, 128, 192, seed=3)
    assert o["bound"] == 9 * 2200 < R.EXACT_LIMIT
    w64, b64 = R.wgrad64(o["dy"], o["x"])
    _both(lambda: o["dy"].t() @ o["x"], lambda: w64)
    _both(lambda: o["dy"].sum(0), lambda: b64)
    # split-K in float32: partial images per 16-row stage, added in any order
    parts = [o["dy"][k:k + 16].t() @ o["x"][k:k + 16] for k in range(0, 2200, 16)]
    _both(lambda: torch.stack(parts[::-1]).sum(0), lambda: w64)
    with pytest.raises(AssertionError):
        R.partial_sum_bound(1 << 21, o["dy"], o["x"])                                # 9 * 2^21 >= 2^24: refused


def test_pointwise_operands_are_exact_in_float32():
    o = R.pointwise_operands(64, 12, seed=4)
    sc, sh = R.pow2_scales(12, seed=1), o["bias"]
    _both(lambda: torch.relu(o["y"] + o["bias"] + o["res"]), lambda: R.bias_act64(o["y"], o["bias"], o["res"]))
    _both(lambda: o["y"] + o["bias"], lambda: R.bias_act64(o["y"], o["bias"], None, relu=False))
    _both(lambda: torch.relu(o["y"] * sc + sh), lambda: R.affine_relu64(o["y"], sc, sh))
    ga, gb, gc = o["grads"]
    _both(lambda: (ga + gb) + gc, lambda: ga.double() + gb.double() + gc.double())
    _both(lambda: ga * sc, lambda: ga.double() * sc.double())
    assert ((o["y"] + o["bias"] + o["res"]) == 0).any() and ((o["y"] + o["bias"]) == 0).any()       # the kink is in the data


# ---- 2. the float64 formulas against torch's operators and autograd ---------------------------------------------------------------
def _nchw(rows, n, h, w):
    return rows.reshape(n, h, w, -1).permute(0, 3, 1, 2)


def test_conv_formulas_equal_conv2d_chains():
    g = torch.Generator().manual_seed(0)
    n, h, w = 2, 3, 5
    M = n * h * w
    x, x0 = torch.randn(M, 64, generator=g, dtype=torch.float64), torch.randn(M, 64, generator=g, dtype=torch.float64)
    res = torch.randn(M, 256, generator=g, dtype=torch.float64)
    wk, wd = torch.randn(64, 256, generator=g, dtype=torch.float64), torch.randn(64, 256, generator=g, dtype=torch.float64)
    b_in, b_out = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(256, generator=g, dtype=torch.float64)
    conv = lambda t, w_kn: F.conv2d(_nchw(t, n, h, w), w_kn.t().reshape(w_kn.shape[1], w_kn.shape[0], 1, 1))
    want = torch.relu(conv(torch.relu(x + b_in), wk) + b_out.view(1, -1, 1, 1) + _nchw(res, n, h, w))
    assert torch.allclose(_nchw(R.tail64(x, b_in, wk, b_out, res), n, h, w), want, rtol=1e-13, atol=1e-13)
    want = torch.relu(conv(torch.relu(x + b_in), wk) + conv(x0, wd) + b_out.view(1, -1, 1, 1))
    assert torch.allclose(_nchw(R.tail_ds64(x, b_in, wk, x0, wd, b_out), n, h, w), want, rtol=1e-13, atol=1e-13)
    xh, wh, bh = torch.randn(M, 256, generator=g, dtype=torch.float64), torch.randn(256, 64, generator=g, dtype=torch.float64), b_in
    want = torch.relu(conv(xh, wh) + bh.view(1, -1, 1, 1))
    assert torch.allclose(_nchw(R.head64(xh, wh, bh), n, h, w), want, rtol=1e-13, atol=1e-13)


def test_wgrad_and_relu_backward_formulas_equal_autograd():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(37, 8, generator=g, dtype=torch.float64)
    lin = torch.nn.Linear(8, 5).double()
    dy = torch.randn(37, 5, generator=g, dtype=torch.float64)
    lin(x).backward(dy)
    dw, db = R.wgrad64(dy, x)
    assert torch.allclose(dw, lin.weight.grad, rtol=1e-13, atol=1e-13) and torch.allclose(db, lin.bias.grad, rtol=1e-13, atol=1e-13)
    pre = torch.tensor([NAN, -1.0, 0.0, 2.0, INF, -INF], dtype=torch.float64, requires_grad=True)
    gr = torch.arange(1.0, 7.0, dtype=torch.float64)
    torch.relu(pre).backward(gr)
    assert torch.equal(R.relu_backward64(pre.detach(), gr), pre.grad)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_pre_bias", [False, True])
def test_group_norm_formula_equals_torch(with_pre_bias, relu):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 256, 2, 5, generator=g, dtype=torch.float64, requires_grad=True)
    gamma, beta = torch.randn(256, generator=g, dtype=torch.float64, requires_grad=True), torch.randn(256, generator=g, dtype=torch.float64, requires_grad=True)
    pb = torch.randn(256, generator=g, dtype=torch.float64) if with_pre_bias else None
    gy = torch.randn(3, 256, 2, 5, generator=g, dtype=torch.float64)
    want = F.group_norm(x if pb is None else x + pb.view(1, -1, 1, 1), 32, gamma, beta, 1e-5)
    want = torch.relu(want) if relu else want
    got = R.group_norm64(x.detach(), gamma.detach(), beta.detach(), 1e-5, pre_bias=pb, relu=relu)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    want.backward(gy)
    gy_in = R.relu_backward64(want.detach(), gy) if relu else gy           # relu: the sign of the output is the sign of its input
    gx, gg, gb = R.group_norm_backward64(x.detach(), gamma.detach(), 1e-5, gy_in, pre_bias=pb)
    assert torch.allclose(gx, x.grad, rtol=1e-11, atol=1e-11)
    assert torch.allclose(gg, gamma.grad, rtol=1e-11, atol=1e-11) and torch.allclose(gb, beta.grad, rtol=1e-11, atol=1e-11)
    scale = R.group_norm_error_scale(x.detach(), gamma.detach(), beta.detach(), 1e-5, pre_bias=pb)
    assert (scale >= got.abs() * (1 - 1e-12)).all() if not relu else True    # sum|terms| bounds |result|


def test_maxpool_formula_is_the_torch_composition():
    y = torch.randn(2, 4, 7, 9, generator=torch.Generator().manual_seed(3))
    b = torch.randn(4, generator=torch.Generator().manual_seed(4))
    want = F.max_pool2d(torch.relu(y.double() + b.double().view(1, -1, 1, 1)), 3, 2, 1)
    got = R.bias_relu_maxpool64(y, b)
    assert torch.equal(got, want) and got.shape == (2, 4, 4, 5)
    # relu(max(y) + b) = max(relu(y + b)): what the one-pass kernel relies on
    assert torch.equal(torch.relu(F.max_pool2d(y.double(), 3, 2, 1) + b.double().view(1, -1, 1, 1)), want)


# ---- 3. the NaN / Inf table of the PyTorch compositions ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_relu_table(dtype):
    v = torch.tensor([NAN, -1.0, 2.0, INF, -INF, 0.0], dtype=dtype, requires_grad=True)
    y = torch.relu(v)
    assert math.isnan(y[0].item()) and y[1:].tolist() == [0.0, 2.0, INF, 0.0, 0.0]
    y.backward(torch.full_like(y, 3.0))
    assert v.grad.tolist() == [3.0, 0.0, 3.0, 3.0, 0.0, 0.0]                 # the gradient PASSES at a NaN input; 0 at exactly 0
    # bias + residual in front: the same table on the sum; Inf - Inf = NaN
    s = R.bias_act64(torch.tensor([[INF, INF, 1.0, NAN]]), torch.tensor([0.0, 0.0, -INF, 0.0]), torch.tensor([[-INF, 1.0, 0.0, 0.0]]))
    assert math.isnan(s[0, 0].item()) and s[0, 1].item() == INF and s[0, 2].item() == 0.0 and math.isnan(s[0, 3].item())


def test_conv_table_inf_times_zero():
    x = torch.zeros(3, 64)
    x[0, 5], x[1, 6], x[2, 7] = NAN, INF, -INF
    w = torch.ones(64, 64)
    w[6, 0] = 0.0                                                            # Inf * 0 = NaN in channel 0 of pixel 1 only
    w[7, 1] = -1.0
    y = R.head64(x, w, torch.zeros(64))
    assert torch.isnan(y[0]).all()
    assert math.isnan(y[1, 0].item()) and (y[1, 1:] == INF).all()
    assert y[2, 1].item() == INF and y[2, 0].item() == 0.0 and (y[2, 2:] == 0).all()          # relu(-Inf) = 0
    # the hidden ReLU of the tail: relu(-Inf + b) = 0 is finite again, relu(NaN) stays
    t = R.tail64(x, torch.zeros(64), torch.ones(64, 256), torch.zeros(256), torch.zeros(3, 256))
    assert torch.isnan(t[0]).all() and (t[1] == INF).all() and (t[2] == 0).all()


def test_maxpool_window_table():
    y = torch.zeros(1, 4, 7, 7)
    y[0, 0, 3, 3] = NAN            # odd coordinates: the centre of ONE window's taps ... (2 oy - 1 + d = 3 -> oy in {1, 2})
    y[0, 1, 2, 2] = INF
    y[0, 2, 4, 4] = -INF
    out = R.bias_relu_maxpool64(y, torch.zeros(4))
    nan = torch.isnan(out[0, 0])
    want = torch.zeros(4, 4, dtype=torch.bool)
    want[1:3, 1:3] = True                                                     # pixel 3 is tap 2 of output 1 and tap 0 of output 2
    assert torch.equal(nan, want)
    inf = torch.isposinf(out[0, 1])
    want = torch.zeros(4, 4, dtype=torch.bool)
    want[1, 1] = True                                                         # pixel 2 = the centre tap of output 1 alone
    assert torch.equal(inf, want)
    assert torch.isfinite(out[0, 2]).all() and not out[0, 2].any()            # -Inf never wins a maximum and relu covers the rest


@pytest.mark.parametrize("relu", [False, True])
def test_group_norm_group_extent_table(relu):
    x = torch.randn(2, 256, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    x[0, 8, 1, 1] = NAN            # group 1 of image 0
    x[1, 255, 0, 0] = INF          # group 31 of image 1
    x[1, 0, 2, 2] = -INF           # group 0 of image 1
    gamma = torch.ones(256, dtype=torch.float64, requires_grad=True)
    gamma.data[9] = 0.0            # a zero weight inside a broken group: NaN * 0 = NaN
    beta = torch.zeros(256, dtype=torch.float64, requires_grad=True)
    xr = x.clone().requires_grad_(True)
    y = F.group_norm(xr, 32, gamma, beta, 1e-5)
    y = torch.relu(y) if relu else y
    want = torch.zeros(2, 256, dtype=torch.bool)
    want[0, 8:16] = want[1, 248:256] = want[1, 0:8] = True
    assert torch.equal(torch.isnan(y).all(-1).all(-1), want) and torch.equal(torch.isnan(y).any(-1).any(-1), want)     # whole groups, nothing else
    assert not torch.isinf(y).any()
    y.backward(torch.ones_like(y))
    assert torch.equal(torch.isnan(xr.grad).all(-1).all(-1), want) and torch.equal((~torch.isfinite(xr.grad)).any(-1).any(-1), want)
    gnan = torch.isnan(gamma.grad)
    assert gnan[0:16].all() and gnan[248:256].all() and not gnan[16:248].any()
    assert torch.isfinite(beta.grad).all()                                    # sum of gy: the ReLU passes gy at a NaN output
    mine = R.group_norm64(x, gamma.detach(), beta.detach(), 1e-5, relu=relu)
    assert torch.equal(torch.isnan(mine), torch.isnan(y)) and not torch.isinf(mine).any()


def test_dropout_of_relu_table():
    torch.manual_seed(0)
    h = torch.ones(4096)
    h[0:1024] = NAN
    h[1024:2048] = INF
    h[2048:3072] = -INF
    hr = h.clone().requires_grad_(True)
    y = F.dropout(torch.relu(hr), 0.5, training=True)
    assert torch.isnan(y[:1024]).all()                                        # kept or dropped: NaN * 0 = NaN
    kept = y[1024:2048] == INF
    assert 300 < int(kept.sum()) < 724 and torch.isnan(y[1024:2048][~kept]).all()                   # a dropped Inf is Inf * 0 = NaN
    assert not y[2048:3072].any()
    assert set(y[3072:].tolist()) == {0.0, 2.0}
    y.backward(torch.ones_like(y))
    assert set(hr.grad[:1024].tolist()) == {0.0, 2.0} and not hr.grad[2048:3072].any()             # mask / (1 - p) passes at NaN
    e = F.dropout(torch.relu(h), 0.5, training=False)
    assert torch.isnan(e[:1024]).all() and (e[1024:2048] == INF).all() and not e[2048:3072].any()


# ---- canaries, the comparison and the split arithmetic ---------------------------------------------------------------------------
def test_canary_buffers():
    t = torch.arange(12.0).reshape(3, 4)
    v = R.with_canary(t, 2, 4, NAN, rows_before=1)
    assert torch.equal(v, t) and v.stride() == (8, 1) and v._base.shape == (6, 8)
    assert R.surroundings_hold(v, NAN)
    v._base[5, 7] = 0.0
    assert not R.surroundings_hold(v, NAN)
    o = R.with_canary(torch.zeros(3, 4), 2, 0, R.SENTINEL, rows_before=2)
    assert o.is_contiguous() and R.surroundings_hold(o, R.SENTINEL)
    o.fill_(7.0)
    assert R.surroundings_hold(o, R.SENTINEL)
    o._base[1, 3] = 7.0
    assert not R.surroundings_hold(o, R.SENTINEL)
    n = R.as_nhwc(R.with_canary(torch.zeros(5, 8), 3, 0, NAN))
    assert n.shape == (1, 8, 1, 5) and n.is_contiguous(memory_format=torch.channels_last)


def test_same_nonfinite():
    a = torch.tensor([NAN, INF, -INF, 1.0, 0.0])
    assert R.same_nonfinite(a, a.double())
    assert R.same_nonfinite(a, torch.tensor([NAN, INF, -INF, 1.0, -0.0], dtype=torch.float64))
    for other in ([0.0, INF, -INF, 1.0, 0.0], [NAN, -INF, -INF, 1.0, 0.0], [NAN, INF, NAN, 1.0, 0.0], [NAN, INF, -INF, 1.5, 0.0],
                  [NAN, INF, -INF, 1.0, NAN]):
        with pytest.raises(AssertionError):
            R.same_nonfinite(a, torch.tensor(other, dtype=torch.float64))
    assert R.same_nonfinite(a, torch.tensor([NAN, INF, -INF, 1.0 + 1e-7, 0.0], dtype=torch.float64), bound=1e-6)
    with pytest.raises(AssertionError):
        R.same_nonfinite(a, torch.tensor([NAN, INF, -INF, 1.0 + 1e-5, 0.0], dtype=torch.float64), bound=1e-6)


def test_wgrad_split_arithmetic():
    assert R.wgrad_splits(64, 8) == [(1, 0)] * 4 + [(0, 0)] * 4                       # 16-row splits, four of them past the end
    assert R.wgrad_splits(65, 8) == [(1, 0)] * 4 + [(0, 1)] + [(0, 0)] * 3            # a split that is one row of tail only
    assert R.wgrad_splits(79, 8)[4] == (0, 15)
    assert R.wgrad_splits(2049, 32)[:26] == [(5, 0)] * 25 + [(3, 1)]
    assert R.wgrad_splits(8800, 16) == [(35, 0)] * 15 + [(25, 0)]                     # 550 rows per split -> 560; only the last is short
    assert sum(16 * s + t for s, t in R.wgrad_splits(8800, 16)) == 8800
    cov = R.wgrad_coverage([R.wgrad_splits(65, 8), R.wgrad_splits(2049, 32)])
    assert {"stages=0", "stages=1", "stages=3", "stages=5", "chain=1", "tail=1", "tail-only split", "empty trailing split"} <= cov
    assert "chain=3" not in cov and not R.WGRAD_REQUIRED <= cov


# ---- the column-sum family: operands, planners and case lists of tests/test_column_sums_gpu.py -----------------------------------------
def _sum_orders(g):
    """Float32 column sums of [rows, C] in several orders: torch's own, the rows reversed, one row at a time backwards, and in 4-wave /
    64-row / 16-way chunks added up afterwards (the kernels' shapes of split)."""
    rows = g.shape[0]
    yield g.sum(0)
    yield g.flip(0).sum(0)
    acc = torch.zeros(g.shape[1])
    for r in range(min(rows, 300) - 1, -1, -1):
        acc = acc + g[r]
    yield acc + g[300:].sum(0)
    for chunk in (4, 64):
        parts = torch.stack([g[k:k + chunk].sum(0) for k in range(0, rows, chunk)])
        yield parts.sum(0)
        yield parts.flip(0).sum(0)
    yield torch.stack([g[w::16].sum(0) for w in range(min(16, rows))]).sum(0)


@pytest.mark.parametrize("rows", [1, 5, 1025, 65537])
def test_colsum_operands_are_exact_in_float32_in_any_order(rows):
    o = R.colsum_operands(rows, 12, seed=5)
    assert o["bound"] == 3 * rows < R.EXACT_LIMIT and o["g"].abs().max() <= 3
    want = o["g"].double().sum(0)
    for got in _sum_orders(o["g"]):
        _both(lambda: got, lambda: want)
    if rows > 1000:
        assert (o["g"] == 0).any() and (o["g"] < 0).any() and want.abs().max() > 0
    with pytest.raises(AssertionError):
        R.colsum_operands(1 << 23, 1)                                                  # 3 * 2^23 >= 2^24: refused before allocating


def test_batched_slice_and_relu_dropout_operands_are_exact_in_float32():
    o = R.colsum_batched_operands(4, 777, 8, seed=6)
    assert o["bound"] == 3 * 8 * 4 * 777 < R.EXACT_LIMIT
    g = o["g"]
    for a, b in R.level_sets(777)["overlap"]:
        want = g[:, a:b].double().sum((0, 1))
        for got in _sum_orders(g[:, a:b].reshape(-1, 8)):
            _both(lambda: got, lambda: want)
    total = sum(g[:, a:b].sum((0, 1)) for a, b in R.NINE_LEVELS[777][:8])
    _both(lambda: total, lambda: sum(g[:, a:b].double().sum((0, 1)) for a, b in R.NINE_LEVELS[777][:8]))
    s = R.slices_operands(64, 260, seed=7)
    assert s["bound"] == 192
    for got in _sum_orders(s["x"]):
        _both(lambda: got, lambda: s["x"].double().sum(0))
    d = R.relu_dropout_colsum_operands(1025, seed=8)
    assert d["bound"] == 6 * 1025 and (d["y"] == 0).any() and (d["y"] < 0).any() and (d["y"] > 0).any()
    for scale in (1.0, 2.0):
        gh = torch.where(d["y"] > 0, d["gy"] * scale, torch.zeros(()))
        want = R.relu_backward64(d["y"], d["gy"]) * scale
        _both(lambda: gh, lambda: want)
        for got in _sum_orders(gh):
            _both(lambda: got, lambda: want.sum(0))


def test_colsum_planners():
    assert R.reduce_plan(1) == (1, 64) and R.reduce_plan(64) == (1, 64) and R.reduce_plan(65) == (2, 64)
    assert R.reduce_plan(65536) == (1024, 64) and R.reduce_plan(65537) == (513, 128)         # the two transitions
    assert R.reduce_plan(131072) == (1024, 128) and R.reduce_plan(131073) == (513, 256)
    assert R.reduce_plan(163200) == (638, 256)
    for rows in (1, 63, 65, 1025, 65535, 65537, 131073, 163200):
        grid, rpb = R.reduce_plan(rows)
        assert grid <= 1024 and rpb % 64 == 0 and (grid - 1) * rpb < rows <= grid * rpb       # no empty workgroup, every row owned
    assert R.colsum_any_plan(1) == (1, 1) and R.colsum_any_plan(128) == (1, 128) and R.colsum_any_plan(129) == (2, 65)
    assert R.colsum_any_plan(65536) == (512, 128) and R.colsum_any_plan(65537) == (512, 129)
    assert 512 * 129 - 65537 > 3 * 129 and 65537 - 508 * 129 == 5                           # three empty trailing workgroups, five rows in the last used one
    assert R.colsum_levels_plan(4, 777, [(0, 13), (77, 777)]) == [(1, 64), (44, 64)]
    for bad in ([(-1, 3)], [(3, 3)], [(4, 3)], [(0, 778)], [], [(0, 1)] * 9):
        assert R.colsum_levels_plan(4, 777, bad) is None
    assert R.colsum_levels_plan(0, 777, [(0, 1)]) is None


def test_colsum_case_lists_reach_every_path():
    cov = R.colsum_coverage(R.COLSUM_ALL_CASES)
    assert R.COLSUM_REQUIRED <= cov, "not reached: %s" % sorted(R.COLSUM_REQUIRED - cov)
    # the tags come from the right cases, and a list without them is seen to lack them
    assert {"grid=2", "last=1", "last%4=1", "rpb=64", "JJ=1,last=1", "n<16"} == R.colsum_coverage([("colsum", 65, 4)])
    assert "n=16" in R.colsum_coverage([("colsum", 1024, 4)]) and "n=1024" in R.colsum_coverage([("colsum", 65536, 4)])
    assert {"rpb=128", "n>16,%16!=0", "last=1"} <= R.colsum_coverage([("colsum", 65537, 4)])
    assert {"scalar empty trailing workgroup", "scalar 512-workgroup cap", "scalar rem=1"} <= R.colsum_coverage([("any", 65537, 17)])
    assert "scalar empty trailing workgroup" not in R.colsum_coverage([("any", 65536, 17)])
    assert "batch boundary on a workgroup edge" in R.colsum_coverage([("strided", 2, 64, 4, 0)])
    assert "batch boundary inside a four-row step" in R.colsum_coverage([("strided", 5, 65, 4, 4)])
    assert "batch boundary inside a four-row step" not in R.colsum_coverage([("strided", 2, 64, 4, 0)])
    lv = R.colsum_coverage([("levels", 3, 131, 384, ((0, 3), (3, 67), (67, 68), (68, 131)), 1)])
    assert {"level not at row 0", "level at an odd row", "level of one row", "batch boundary on a workgroup edge", "JJ=2,last=32"} <= lv
    assert not R.COLSUM_REQUIRED <= R.colsum_coverage(R.COLSUM_CASES)
    # what the issue lists is in the lists
    assert {r for _, r, _ in R.COLSUM_CASES} == {1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 65535, 65536, 65537, 131073}
    assert {c for _, _, c in R.COLSUM_CASES} == {4, 252, 256, 260, 508, 512, 516, 1020, 1024}
    assert {r for _, r, _ in R.ANY_CASES} == {1, 2, 3, 4, 5, 127, 128, 129, 65536, 65537}
    assert {c for _, _, c in R.ANY_CASES} == {1, 17, 81, 255, 257, 1023} and {c for _, _, c in R.ANY_WRAPPER_CASES} == {17, 81, 1023}
    assert max(r * c * 4 for _, r, c in R.COLSUM_CASES + R.ANY_CASES) < 150e6
    assert all(len(b) == 9 and R.colsum_levels_plan(2, S, b) is None and R.colsum_levels_plan(2, S, b[:8]) for S, b in R.NINE_LEVELS.items())
