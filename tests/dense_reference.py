"""Helpers for the tests of the dense backbone / projection kernels (csrc/pointwise.hip, conv1x1_fused.hip, small_wgrad.hip,
groupnorm.hip): operand generators, canary buffers, the non-finite comparison and plain float64 formulas.  No GPU code.

THE EXACT-INTEGER RULE.  A float32 holds every integer of magnitude <= 2^24 exactly.  When every operand of a product-sum

    sum_k a[k] * b[k] + bias + res,      a, b, bias, res integers,     K_total * max|a| * max|b| + max|bias| + max|res| < 2^24

is a small integer, every product and every partial sum -- in ANY order, with or without fused multiply-adds, split over any number
of accumulators -- is an integer below 2^24 and therefore exact in float32.  The float64 result cast to float32 is then the ONLY
correct float32 answer, and a kernel is compared with ``torch.equal``: one wrong address, one row used twice or skipped, one
stale pipeline slot changes an integer by at least 1, where ``randn`` and a relative tolerance could hide it.  Every generator
below returns its bound and asserts it; tests/test_dense_reference_cpu.py proves float32 == float64 on the reference alone.
"""
import math

import torch
import torch.nn.functional as F

EXACT_LIMIT = 1 << 24           # integers up to here are exact in float32
MAT_MAX, VEC_MAX = 3, 8         # |matrix entries| <= 3, |biases|, |residuals| <= 8
SENTINEL = -12345.0             # what an output's surroundings hold (no kernel here can produce it: outputs are >= 0 or small integers)


# ---- integer operands --------------------------------------------------------------------------------------------------------
def _gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


def ints(shape, lo, hi, gen, device="cpu"):
    """float32 tensor of integers drawn uniformly from [lo, hi] on ``device`` (``gen`` is a generator of that device)."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen, dtype=torch.int32, device=device).to(torch.float32)


def partial_sum_bound(k_total, a, b, *addends):
    """``K_total * amax * bmax + sum of max|addend|``: no partial sum of the composition exceeds it.  Asserted below 2^24."""
    amax = float(a.abs().max()) if a.numel() else 0.0
    bmax = float(b.abs().max()) if b.numel() else 0.0
    bound = k_total * amax * bmax + sum(float(t.abs().max()) for t in addends if t is not None and t.numel())
    assert bound < EXACT_LIMIT, "operands are not exact in float32: bound %g >= 2^24" % bound
    return bound


def _mat(shape, mode, gen, device):
    lo, hi = {"half": (-MAT_MAX, MAT_MAX), "dead": (-MAT_MAX, 0), "alive": (0, MAT_MAX)}[mode]
    return ints(shape, lo, hi, gen, device)


def _vec(shape, mode, gen, device):
    lo, hi = {"half": (-VEC_MAX, VEC_MAX), "dead": (-VEC_MAX, -1), "alive": (1, VEC_MAX)}[mode]
    return ints(shape, lo, hi, gen, device)


def head_operands(M, K, seed=0, mode="half", device="cpu"):
    """x [M, K], w [K, 64], b [64] of ``head64``.  mode "half": about half of the pre-ReLU values negative (symmetric operands);
    "dead": every output 0 (x >= 0, w <= 0, b < 0); "alive": every pre-ReLU value positive."""
    g = _gen(seed, device)
    x = ints((M, K), 0, MAT_MAX, g, device) if mode != "half" else ints((M, K), -MAT_MAX, MAT_MAX, g, device)
    w, b = _mat((K, 64), mode, g, device), _vec((64,), mode, g, device)
    return dict(x=x, w=w, b=b, bound=partial_sum_bound(K, x, w, b))


def tail_operands(M, seed=0, mode="half", device="cpu", downsample=False):
    """Operands of ``tail64`` (x [M, 64], b_in [64], w [64, 256], b_out [256], res [M, 256]) or, with ``downsample``, of
    ``tail_ds64`` (x0 [M, 64], wd [64, 256] instead of res).  "half": b_in symmetric around -x's mean, so about half of x + b_in is
    negative, and symmetric weights, so about half of the pre-ReLU output is; "dead" / "alive": every output 0 / positive."""
    g = _gen(seed, device)
    x = ints((M, 64), -MAT_MAX, MAT_MAX, g, device)
    b_in = ints((64,), -MAT_MAX, MAT_MAX, g, device)
    w, b_out = _mat((64, 256), mode, g, device), _vec((256,), mode, g, device)
    hidden = torch.relu(x + b_in)                                # integers in [0, 6]
    out = dict(x=x, b_in=b_in, w=w, b_out=b_out)
    if downsample:
        x0 = ints((M, 64), 0, MAT_MAX, g, device) if mode != "half" else ints((M, 64), -MAT_MAX, MAT_MAX, g, device)
        wd = _mat((64, 256), mode, g, device)
        out.update(x0=x0, wd=wd)
        out["bound"] = partial_sum_bound(64, hidden, w) + partial_sum_bound(64, x0, wd, b_out)
        assert out["bound"] < EXACT_LIMIT
    else:
        res = _vec((M, 256), mode, g, device)
        out.update(res=res, bound=partial_sum_bound(64, hidden, w, b_out, res))
    return out


def wgrad_operands(R, M, N, seed=0, device="cpu"):
    """dY [R, M], X [R, N] in [-3, 3]: dW = dY^T X and db = colsum(dY) are exact while 9 R < 2^24."""
    g = _gen(seed, device)
    dy, x = ints((R, M), -MAT_MAX, MAT_MAX, g, device), ints((R, N), -MAT_MAX, MAT_MAX, g, device)
    return dict(dy=dy, x=x, bound=partial_sum_bound(R, dy, x))


def pointwise_operands(rows, C, seed=0, device="cpu", n_grads=3):
    """y, res [rows, C], bias [C] in [-8, 8] (zeros of y + bias (+ res) included: the ReLU's kink) and ``n_grads`` integer gradients:
    one or two additions per element, |sums| <= 24."""
    g = _gen(seed, device)
    y, res, bias = ints((rows, C), -VEC_MAX, VEC_MAX, g, device), ints((rows, C), -VEC_MAX, VEC_MAX, g, device), ints((C,), -VEC_MAX, VEC_MAX, g, device)
    grads = [ints((rows, C), -VEC_MAX, VEC_MAX, g, device) for _ in range(n_grads)]
    bound = 3 * VEC_MAX
    assert bound < EXACT_LIMIT
    return dict(y=y, res=res, bias=bias, grads=grads, bound=bound)


def pow2_scales(C, seed=0, device="cpu"):
    """Per-channel scales from {+-1/4, +-1/2, +-1, +-2, +-4, 0}: a product with a small integer is exact (a shift of the exponent)."""
    g = _gen(seed, device)
    table = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0, -0.25, -0.5, -1.0, -2.0, -4.0, 0.0], device=device)
    return table[torch.randint(0, len(table), (C,), generator=g, device=device)]


# ---- canary buffers ----------------------------------------------------------------------------------------------------------
def with_canary(t, rows_after, cols_after, value, rows_before=0):
    """A view holding ``t`` ([R, C]) inside a larger [rows_before + R + rows_after, C + cols_after] allocation whose remainder is
    filled with ``value``: NaN behind an input (a kernel that reads a row >= R or a hidden column turns its result NaN), a
    sentinel around an output (``surroundings_hold``).  Everything is inside one valid allocation: nothing is out of bounds."""
    R, C = t.shape
    base = torch.full((rows_before + R + rows_after, C + cols_after), float(value), dtype=t.dtype, device=t.device)
    view = base[rows_before:rows_before + R, :C]
    view.copy_(t)
    assert view.data_ptr() % 16 == 0 or (C + cols_after) % 4
    return view


def surroundings_hold(view, value):
    """True when everything of ``view``'s allocation outside the view still holds ``value`` (NaN compares by isnan)."""
    base = view._base
    assert base is not None and base.dim() == 2 and view.dim() == 2
    ld = base.stride(0)
    off = view.storage_offset() - base.storage_offset()
    r0, c0 = off // ld, off % ld
    outside = torch.ones(base.shape, dtype=torch.bool, device=base.device)
    outside[r0:r0 + view.shape[0], c0:c0 + view.shape[1]] = False
    rest = base[outside]
    return bool(torch.isnan(rest).all()) if math.isnan(value) else bool((rest == value).all())


def as_nhwc(rows):
    """[M, C] rows (row stride C) as the channels-last 4-D tensor [1, C, 1, M] on the same memory."""
    M, C = rows.shape
    assert rows.stride() == (C, 1)
    return rows.view(1, 1, M, C).permute(0, 3, 1, 2)


# ---- comparison --------------------------------------------------------------------------------------------------------------
def same_nonfinite(got, want, bound=None):
    """NaN, +Inf and -Inf at exactly the same places, and the finite rest ``torch.equal`` (``bound`` None) or within the
    per-element ``bound`` (a tensor or a number, for the non-integer cases).  Raises AssertionError saying what differs."""
    want = want.to(got.dtype) if bound is None else want
    assert got.shape == want.shape, (got.shape, want.shape)
    for name, f in (("NaN", torch.isnan), ("+Inf", torch.isposinf), ("-Inf", torch.isneginf)):
        a, b = f(got), f(want)
        if not torch.equal(a, b):
            bad = (a != b).nonzero()
            raise AssertionError("%s masks differ at %d of %d places (kernel %d, reference %d), first %s: kernel %s, reference %s" % (
                name, len(bad), got.numel(), int(a.sum()), int(b.sum()), bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item()))
    fin = torch.isfinite(want)
    if bound is None:
        if not torch.equal(got[fin], want[fin]):
            bad = ((got != want) & fin).nonzero()
            raise AssertionError("finite values differ at %d places, first %s: kernel %r, reference %r" % (
                len(bad), bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item()))
    else:
        err = (got.double() - want.double()).abs()
        b = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
        over = fin & (err > b)
        if over.any():
            i = tuple(over.nonzero()[0])
            raise AssertionError("error above the bound at %d places, first %s: |err| %.3e > %.3e" % (int(over.sum()), list(i), err[i].item(), b[i].item()))
    return True


def plant(t, where, values=(float("nan"), float("inf"), float("-inf"))):
    """Writes the non-finite ``values`` at the flat positions ``where`` of the (row-dense) tensor ``t``, in place."""
    flat = t.view(-1) if t.is_contiguous() else t.reshape(-1)
    assert flat.data_ptr() == t.data_ptr()
    for pos, v in zip(where, values):
        flat[pos] = v
    return t


# ---- plain float64 formulas (rows = channels-last pixels) ----------------------------------------------------------------------
def head64(x, w, b):
    """relu(conv1x1(x, w) + b): x [M, K], w [K, 64]."""
    return torch.relu(x.double() @ w.double() + b.double())


def tail64(x, b_in, w, b_out, res):
    """relu(conv1x1(relu(x + b_in), w) + b_out + res)."""
    return torch.relu(torch.relu(x.double() + b_in.double()) @ w.double() + b_out.double() + res.double())


def tail_ds64(x, b_in, w, x0, wd, b_out):
    """relu(conv1x1(relu(x + b_in), w) + conv1x1(x0, wd) + b_out)."""
    return torch.relu(torch.relu(x.double() + b_in.double()) @ w.double() + x0.double() @ wd.double() + b_out.double())


def wgrad64(dy, x):
    """(dW, db) of y = x W^T + b for the output gradient dy."""
    return dy.double().t() @ x.double(), dy.double().sum(0)


def bias_act64(y, bias, res=None, relu=True):
    v = y.double() + bias.double()
    if res is not None:
        v = v + res.double()
    return torch.relu(v) if relu else v


def affine_relu64(y, scale, shift):
    return torch.relu(y.double() * scale.double() + shift.double())


def relu_backward64(pre, grad):
    """threshold_backward: the gradient where the ReLU's input is positive OR NaN, 0 elsewhere (0 at exactly 0)."""
    return torch.where(pre <= 0, torch.zeros_like(grad, dtype=torch.float64), grad.double())


def bias_relu_maxpool64(y_nchw, bias):
    return F.max_pool2d(torch.relu(y_nchw.double() + bias.double().view(1, -1, 1, 1)), kernel_size=3, stride=2, padding=1)


def group_norm64(x, gamma, beta, eps, groups=32, pre_bias=None, relu=False):
    """GroupNorm of an NCHW tensor written out: per (image, group) mean and BIASED variance over C / groups channels x H x W."""
    v = x.double() if pre_bias is None else x.double() + pre_bias.double().view(1, -1, 1, 1)
    B, C = v.shape[:2]
    g = v.reshape(B, groups, -1)
    mean = g.mean(-1, keepdim=True)
    var = ((g - mean) ** 2).mean(-1, keepdim=True)
    xhat = ((g - mean) / torch.sqrt(var + eps)).reshape(v.shape)
    y = xhat * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def group_norm_backward64(x, gamma, eps, gy, groups=32, pre_bias=None):
    """(gx, ggamma, gbeta) of ``group_norm64`` without ReLU:  gx = rstd (gy gamma - mean_g(gy gamma) - xhat mean_g(gy gamma xhat))."""
    v = x.double() if pre_bias is None else x.double() + pre_bias.double().view(1, -1, 1, 1)
    B, C = v.shape[:2]
    g = v.reshape(B, groups, -1)
    mean = g.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((g - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (g - mean) * rstd
    t = (gy.double() * gamma.double().view(1, -1, 1, 1)).reshape(B, groups, -1)
    gx = rstd * (t - t.mean(-1, keepdim=True) - xhat * (t * xhat).mean(-1, keepdim=True))
    xh4 = xhat.reshape(v.shape)
    return gx.reshape(v.shape), (gy.double() * xh4).sum((0, 2, 3)), gy.double().sum((0, 2, 3))


def group_norm_error_scale(x, gamma, beta, eps, groups=32, pre_bias=None):
    """sum|terms| of every output of GroupNorm, the cancellation-aware scale of its float32 error:
        y = (x - mean) rstd gamma + beta:   (|x| + |pre_bias| + |mean|) rstd |gamma| + |beta|
    (an output near 0 that is the difference of two large terms is allowed the rounding of those terms, not of the result)."""
    v = x.double() if pre_bias is None else x.double() + pre_bias.double().view(1, -1, 1, 1)
    mag = x.double().abs() if pre_bias is None else x.double().abs() + pre_bias.double().abs().view(1, -1, 1, 1)
    B, C = v.shape[:2]
    g = v.reshape(B, groups, -1)
    mean = g.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((g - mean) ** 2).mean(-1, keepdim=True) + eps)
    s = (mag.reshape(B, groups, -1) + mean.abs()) * rstd
    return s.reshape(v.shape) * gamma.double().abs().view(1, -1, 1, 1) + beta.double().abs().view(1, -1, 1, 1)


# ---- the split arithmetic of mono_linear_wgrad_f32 (csrc/pointwise.hip, small_wgrad.hip), as a function of S -------------------
STAGE_ROWS = 16


def wgrad_splits(R, S):
    """[(n_stages, tail_rows)] per split for R rows cut into S splits: rows_per_split = ceil(R / S) rounded up to a whole number of
    16-row stages; a split past the matrix's end is (0, 0).  S = mono_linear_wgrad_workspace(R, M, N) // (M N + M).  Used to ASSERT
    that a list of cases covers the pipeline's paths, never as the expected value of a result."""
    rows_per_split = -(-(-(-R // S)) // STAGE_ROWS) * STAGE_ROWS
    out = []
    for s in range(S):
        k0 = s * rows_per_split
        n = max(min(R, k0 + rows_per_split) - k0, 0)
        out.append((n // STAGE_ROWS, n % STAGE_ROWS))
    return out


def wgrad_coverage(split_lists):
    """What a collection of ``wgrad_splits`` results exercises, as a set of tags."""
    tags = set()
    for splits in split_lists:
        seen_rows = False
        for i, (stages, tail) in enumerate(splits):
            tags.add("stages=%d" % stages)
            tags.add("tail=%d" % tail)
            if stages >= 4 and stages % 4:
                tags.add("chain=%d" % (stages % 4))            # remainder stages behind at least one full group of four
            if stages == 0 and tail > 0:
                tags.add("tail-only split")
            if stages == 0 and tail == 0 and i == len(splits) - 1 and seen_rows:
                tags.add("empty trailing split")
            seen_rows = seen_rows or stages + tail > 0
    return tags


WGRAD_REQUIRED = ({"stages=%d" % n for n in range(9)} | {"chain=1", "chain=2", "chain=3"} | {"tail=0", "tail=1", "tail=2", "tail=15"}
                  | {"empty trailing split", "tail-only split"})
