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


# ---- the column-sum family of csrc/pointwise.hip (tests/test_column_sums_gpu.py) ---------------------------------------------------
def colsum_operands(rows, C, seed=0, device="cpu"):
    """g [rows, C] in [-3, 3]: every partial sum of a column, in any order and over any split, stays below 3 rows < 2^24."""
    bound = MAT_MAX * rows
    assert bound < EXACT_LIMIT, "operands are not exact in float32: bound %g >= 2^24" % bound
    return dict(g=ints((rows, C), -MAT_MAX, MAT_MAX, _gen(seed, device), device), bound=bound)


def colsum_batched_operands(B, S, C, seed=0, device="cpu"):
    """g [B, S, C] in [-3, 3] for the strided and per-level sums.  The bound 3 * 8 * B * S also covers the sum over up to eight levels
    that overlap (``with_total`` adds a row once per level that holds it)."""
    bound = MAT_MAX * 8 * B * S
    assert bound < EXACT_LIMIT, "operands are not exact in float32: bound %g >= 2^24" % bound
    return dict(g=ints((B, S, C), -MAT_MAX, MAT_MAX, _gen(seed, device), device), bound=bound)


def slices_operands(n, C, seed=0, device="cpu"):
    """x [n, C] in [-3, 3], a stack of n slices: |sums| <= 3 n."""
    bound = MAT_MAX * n
    assert bound < EXACT_LIMIT, "operands are not exact in float32: bound %g >= 2^24" % bound
    return dict(x=ints((n, C), -MAT_MAX, MAT_MAX, _gen(seed, device), device), bound=bound)


def relu_dropout_colsum_operands(rows, seed=0, device="cpu"):
    """gy [rows, 256] in [-3, 3], y [rows, 256] in [-8, 8] (zeros and negatives: the mask), for a scale of 1 or 2: |sums| <= 6 rows."""
    bound = 2 * MAT_MAX * rows
    assert bound < EXACT_LIMIT, "operands are not exact in float32: bound %g >= 2^24" % bound
    g = _gen(seed, device)
    return dict(gy=ints((rows, 256), -MAT_MAX, MAT_MAX, g, device), y=ints((rows, 256), -VEC_MAX, VEC_MAX, g, device), bound=bound)


# The launchers' planning arithmetic restated (used to ASSERT what a case list reaches, and compared with the library's own planner
# functions on the GPU box; never the expected value of a result).
def reduce_plan(rows):
    """(grid, rows_per_block) of mono_colsum_f32 / mono_colsum_strided_f32: mono_reduce_blocks doubles 64-row workgroups until at most
    1024 are left; the launcher then rounds ceil(rows / grid) up to a multiple of 64."""
    rpb = 64
    while -(-rows // rpb) > 1024:
        rpb *= 2
    grid = -(-rows // rpb)
    return grid, (-(-rows // grid) + 63) // 64 * 64


def colsum_any_plan(rows):
    """(grid, rows_per_block) of mono_colsum_any_f32: 128-row workgroups, 1 <= grid <= 512, rows_per_block = ceil(rows / grid)."""
    grid = min(max(-(-rows // 128), 1), 512)
    return grid, -(-rows // grid)


def colsum_levels_plan(batch, S, bounds):
    """[(grid, rows_per_block)] per level of mono_colsum_levels_f32, or None where mono_colsum_levels_blocks returns 0."""
    if batch <= 0 or not 0 < len(bounds) <= 8:
        return None
    if any(a < 0 or b <= a or b > S for a, b in bounds):
        return None
    return [reduce_plan(batch * (b - a)) for a, b in bounds]


def _vector_tags(tags, kind, grid, rpb, total, C):
    """Tags of one colsum_kernel / colsum_levels_kernel grid over ``total`` rows and of the fold over its ``grid`` partial rows."""
    last = total - (grid - 1) * rpb
    assert 0 < last <= rpb
    tags.update({"grid=%d" % grid if grid <= 2 else "grid>2", "rpb=%d" % rpb, "last%%4=%d" % (last % 4)})
    if last == 1:
        tags.add("last=1")
    if last == rpb:
        tags.add("last=full")
    _fold_tags(tags, grid)
    cv = C // 4
    tags.add("JJ=%d,last=%d" % (1 if C <= 256 else 2 if C <= 512 else 4, (cv - 1) % 64 + 1))


def _fold_tags(tags, n):
    """partial_sum_kernel / partial_sum_levels_kernel: 16 waves take partial rows k, k + 16, ..."""
    tags.add("n<16" if n < 16 else "n=16" if n == 16 else "n=1024" if n == 1024 else "n>16,%16!=0" if n % 16 else "n>16,%16=0")


def _boundary_tags(tags, batch, rows_b, rpb):
    """Rows k * rows_b, 0 < k < batch, of the virtual [batch * rows_b, C] matrix start a new batch.  The four waves of a workgroup take
    rows r0 + 4 i + (0..3) together and r0 is a multiple of 64: a boundary that is no multiple of 4 lies inside such a step."""
    for k in range(1, batch):
        if (k * rows_b) % 4:
            tags.add("batch boundary inside a four-row step")
        if (k * rows_b) % rpb == 0:
            tags.add("batch boundary on a workgroup edge")


def colsum_coverage(cases):
    """What a list of cases exercises, as a set of tags.  A case is a tuple led by the entry point's name:
    ("colsum", rows, C), ("any", rows, C), ("strided", batch, rows, C, gap), ("levels", B, S, C, bounds, with_total),
    ("slices", n, C), ("relu_dropout", rows, p)."""
    tags = set()
    for case in cases:
        kind = case[0]
        if kind == "colsum":
            _, rows, C = case
            _vector_tags(tags, kind, *reduce_plan(rows), rows, C)
        elif kind == "strided":
            _, batch, rows, C, gap = case
            grid, rpb = reduce_plan(batch * rows)
            _vector_tags(tags, kind, grid, rpb, batch * rows, C)
            _boundary_tags(tags, batch, rows, rpb)
            if gap:
                tags.add("gap between batches")
        elif kind == "levels":
            _, B, S, C, bounds, with_total = case
            plan = colsum_levels_plan(B, S, bounds)
            assert plan is not None, case
            for (a, b), (grid, rpb) in zip(bounds, plan):
                _vector_tags(tags, kind, grid, rpb, B * (b - a), C)
                _boundary_tags(tags, B, b - a, rpb)
                if a:
                    tags.add("level not at row 0")
                if a % 2:
                    tags.add("level at an odd row")
                if b - a == 1:
                    tags.add("level of one row")
            tags.add("levels=%d" % len(bounds))
            if with_total:
                _fold_tags(tags, sum(g for g, _ in plan))
        elif kind == "any":
            _, rows, C = case
            grid, rpb = colsum_any_plan(rows)
            counts = [max(min(rows, (i + 1) * rpb) - i * rpb, 0) for i in range(grid)]
            assert sum(counts) == rows
            tags.update("scalar rem=%d" % (n % 4) for n in counts if n)
            if counts[-1] == 0:
                tags.add("scalar empty trailing workgroup")
            if grid == 512 and -(-rows // 128) > 512:
                tags.add("scalar 512-workgroup cap")
            tags.add("scalar column passes=%d" % -(-C // 256))
        elif kind == "slices":
            _fold_tags(tags, case[1])
        elif kind == "relu_dropout":
            grid, _ = reduce_plan(case[1])
            _fold_tags(tags, grid)
            tags.add("relu_dropout wrap" if case[1] > 4 * grid else "relu_dropout one pass")       # rows beyond one grid pass of 4 waves
        else:
            raise ValueError(case)
    return tags


COLSUM_REQUIRED = ({"grid=1", "grid=2", "last=1", "last=full", "rpb=64", "rpb=128", "rpb=256"} | {"last%%4=%d" % k for k in range(4)}
                   | {"n<16", "n=16", "n>16,%16!=0", "n=1024"}
                   | {"JJ=%d,last=%d" % (jj, n) for jj in (1, 2, 4) for n in (1, 63, 64)}
                   | {"scalar rem=%d" % k for k in range(4)} | {"scalar empty trailing workgroup", "scalar 512-workgroup cap"}
                   | {"batch boundary inside a four-row step", "batch boundary on a workgroup edge", "level not at row 0",
                      "level at an odd row", "level of one row", "levels=8", "gap between batches", "relu_dropout wrap"})


# ---- the case lists: the smallest shapes that reach each path ----------------------------------------------------------------------
COLSUM_ROWS = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025]
COLSUM_WIDTHS = [4, 252, 256, 260, 508, 512]
COLSUM_ABI_WIDTHS = [516, 1020, 1024]                       # colsum_kernel<4>: pointwise.colsum sends these to torch
# 65535 / 65536 rows: 1024 workgroups of 64; 65537: 513 of 128; 131073: 513 of 256 -- narrow, and one wide case each (<= 135 MB)
COLSUM_BIG = [(65535, 4), (65535, 260), (65536, 4), (65536, 512), (65537, 4), (65537, 516), (131073, 4), (131073, 256)]
COLSUM_CASES = [("colsum", r, c) for r in COLSUM_ROWS for c in COLSUM_WIDTHS + COLSUM_ABI_WIDTHS] + [("colsum", r, c) for r, c in COLSUM_BIG]

ANY_ROWS = [1, 2, 3, 4, 5, 127, 128, 129]
ANY_ABI_WIDTHS = [1, 17, 81, 255, 257, 1023]
ANY_BIG = [(65536, 1), (65536, 81), (65536, 257), (65537, 1), (65537, 17), (65537, 257)]       # <= 68 MB
ANY_CASES = [("any", r, c) for r in ANY_ROWS for c in ANY_ABI_WIDTHS] + [("any", r, c) for r, c in ANY_BIG]
ANY_WRAPPER_CASES = [("any", r, c) for r in (1, 5, 129) for c in (17, 81, 1023)] + [("any", 65537, 81)]       # through pointwise.colsum

STRIDED_CASES = [("strided", b, r, c, gap) for b, r in ((1, 1), (3, 37), (2, 64), (5, 65), (16, 30)) for c in (4, 256, 260, 512)
                 for gap in (0, 4, 8 * c)]


def level_sets(S):
    """name -> bounds for a [B, S, C] tensor.  "tiled": adjacent levels, a one-row level, odd starts; "gapped": rows between the levels
    that belong to none (NaN in the test); "overlap": levels that share rows; "eight": the most one launch takes."""
    if S == 5:
        return {"tiled": [(0, 1), (1, 4), (4, 5)], "gapped": [(1, 2), (3, 5)], "overlap": [(0, 3), (1, 5), (2, 3)],
                "eight": [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (1, 4), (3, 5)]}
    if S == 131:
        # (3, 67): 64 rows, a batch boundary on a workgroup edge
        return {"tiled": [(0, 3), (3, 67), (67, 68), (68, 131)], "gapped": [(1, 30), (33, 97), (99, 100), (101, 130)],
                "overlap": [(0, 131), (5, 70), (64, 65)],
                "eight": [(0, 1), (1, 2), (3, 20), (20, 37), (41, 105), (105, 110), (111, 128), (129, 131)]}
    assert S == 777
    # (77, 777): 4 x 700 rows = 44 workgroups; (13, 269): 256 rows, 16 workgroups for 4 batches
    return {"tiled": [(0, 13), (13, 269), (269, 270), (270, 777)], "gapped": [(1, 2), (77, 777)], "overlap": [(0, 777), (5, 776), (333, 334)],
            "eight": [(0, 64), (65, 66), (67, 195), (195, 300), (301, 302), (303, 700), (700, 701), (705, 777)]}


LEVEL_CASES = [("levels", B, S, C, tuple(bounds), wt) for B, S in ((1, 5), (3, 131), (4, 777)) for C in (4, 256, 384, 512)
               for name, bounds in level_sets(S).items() for wt in (0, 1)]
NINE_LEVELS = {5: [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (1, 4), (3, 5), (2, 5)],
               131: [(0, 1), (1, 2), (3, 20), (20, 37), (41, 105), (105, 110), (111, 128), (129, 131), (7, 77)],
               777: [(0, 64), (65, 66), (67, 195), (195, 300), (301, 302), (303, 700), (700, 701), (705, 777), (1, 777)]}

SLICES_CASES = [("slices", n, c) for n in (1, 2, 15, 16, 17, 31, 32, 33, 64) for c in (4, 252, 256, 260, 65536)]
RELU_DROPOUT_CASES = [("relu_dropout", r, p) for r in (1, 3, 4, 5, 255, 256, 257, 65536, 65537) for p in (0.0, 0.5)]

COLSUM_ALL_CASES = COLSUM_CASES + ANY_CASES + ANY_WRAPPER_CASES + STRIDED_CASES + LEVEL_CASES + SLICES_CASES + RELU_DROPOUT_CASES
