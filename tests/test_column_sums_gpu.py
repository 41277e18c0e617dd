"""C6.  The column-sum family of csrc/pointwise.hip -- mono_colsum_f32, mono_colsum_any_f32, mono_colsum_strided_f32,
mono_colsum_levels_f32, mono_sum_slices_f32, mono_relu_dropout_bwd_colsum_f32 and their planners -- pinned the way sections C1-C4 of
tests/test_dense_kernels_gpu.py pin the bottleneck kernels: integer operands (tests/dense_reference.py: the exact-integer rule), so
that the float64 sum cast to float32 is the ONLY correct answer and one row used twice, skipped or taken from the wrong batch changes
an integer.  Every launch has

- its input between NaN rows, NaN in the gaps between batches and in the rows of no level: a finite result read none of them;
- its output inside a sentinel buffer: the kernel wrote its C floats (levels: [L (+ 1), C]) and nothing else;
- its own partial-row scratch, sized by the library's planner, NaN on entry and followed by a sentinel tail: every partial row read had
  been written, none behind the plan was;

and a second launch with NaN, +Inf, -Inf and a (+Inf, -Inf) pair planted in distinct columns at the rows where a workgroup, a batch or
the matrix begins and ends.  The case lists live in tests/dense_reference.py; tests/test_dense_reference_cpu.py proves on the CPU that
they reach COLSUM_REQUIRED.  No tolerance appears in this file."""
import ctypes

import pytest
import torch

import dense_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN, INF = float("nan"), float("inf")
PAD = 8                        # NaN rows before and behind an input: two four-row steps
TAIL = 64                      # sentinel floats behind the partial rows


def _pw():
    from monosowa_amd import pointwise
    return pointwise


def _lib():
    return _pw().load()


def _call(name, *args):
    from monosowa_amd._lib import raw_stream
    return getattr(_lib(), name)(*args, raw_stream())


def _p(t):
    return None if t is None else t.data_ptr()


def _int_array(values):
    return (ctypes.c_int * len(values))(*values)


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
def _framed(t):
    """``t`` [rows, C] between PAD NaN rows on either side, as a contiguous view."""
    return R.with_canary(t, PAD, 0, NAN, rows_before=PAD)


def _out(n_rows, C):
    """A sentinel-filled [n_rows, C] output with two sentinel rows on either side."""
    return R.with_canary(torch.full((n_rows, C), R.SENTINEL, device=DEV), 2, 0, R.SENTINEL, rows_before=2)


def _scratch(blocks, C):
    """``blocks`` partial rows of C floats, NaN, and TAIL sentinel floats behind them."""
    buf = torch.full((blocks * C + TAIL,), NAN, device=DEV)
    buf[blocks * C:] = R.SENTINEL
    return buf


def _tail_holds(buf):
    return bool((buf[-TAIL:] == R.SENTINEL).all())


def _assert_exact(got, want64, what):
    want = want64.to(torch.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~torch.isfinite(got)
    assert not bad.any(), "%s: %d non-finite outputs, first at %s: a canary or an unwritten partial row was read" % (
        what, int(bad.sum()), bad.nonzero()[0].tolist())
    if not torch.equal(got, want):
        diff = (got != want).nonzero()
        i = tuple(diff[0].tolist())
        raise AssertionError("%s: %d of %d outputs differ, first at %s: kernel %r, reference %r" % (
            what, len(diff), got.numel(), list(i), got[i].item(), want[i].item()))


def _plant(put, positions, C):
    """One (+Inf, -Inf) pair at the first and last of ``positions`` and NaN, +Inf, -Inf in turn at the others, every plant in a column of
    its own (``put(position, column, value)``); where C has fewer columns than there are plants, an even selection of them."""
    positions = list(dict.fromkeys(positions))
    plants = [("pair", positions[0], positions[-1])] if len(positions) > 1 else []
    plants += [("one", positions[i % len(positions)]) for i in range(max(3, len(positions)))]
    if len(plants) > C:
        plants = [plants[i] for i in sorted({round(k * (len(plants) - 1) / max(C - 1, 1)) for k in range(C)})]
    step, singles = max(C // len(plants), 1), 0
    for i, pl in enumerate(plants):
        assert i * step < C
        if pl[0] == "pair":
            put(pl[1], i * step, INF)
            put(pl[2], i * step, -INF)
        else:
            put(pl[1], i * step, (NAN, INF, -INF)[singles % 3])
            singles += 1
    return len(plants)


def _row_candidates(rows, rpb, *more):
    return [r for r in (0, 1, 2, 3, rpb - 1, rpb, rows - 2, rows - 1) + tuple(more) if 0 <= r < rows]


def _exact_then_planted(launch, want_fn, plant_fn, out_rows, C, blocks, what):
    """Launches twice with fresh sentinel / NaN buffers: on the integers (exact), then with non-finites planted (same places, rest exact)."""
    for planted in (False, True):
        if planted:
            plant_fn()
        out = _out(out_rows, C)
        scratch = _scratch(blocks, C) if blocks else None
        assert launch(out, scratch) == 0, what
        torch.cuda.synchronize()
        want = want_fn()
        if planted:
            assert not torch.isfinite(want).all(), "nothing was planted"
            assert R.same_nonfinite(out, want.to(torch.float32).view(out.shape)), what
        else:
            _assert_exact(out, want.view(out.shape), what)
        assert R.surroundings_hold(out, R.SENTINEL), "%s: the kernel wrote outside its output" % what
        assert scratch is None or _tail_holds(scratch), "%s: the kernel wrote behind its %d partial rows" % (what, blocks)


# ---- the planners ----------------------------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_path_and_the_planners_agree():
    lib = _lib()
    cov = R.colsum_coverage(R.COLSUM_ALL_CASES)
    assert R.COLSUM_REQUIRED <= cov, "not reached: %s" % sorted(R.COLSUM_REQUIRED - cov)
    for case in R.COLSUM_ALL_CASES:
        kind = case[0]
        if kind in ("colsum", "relu_dropout"):
            assert lib.mono_reduce_blocks(case[1]) == R.reduce_plan(case[1])[0], case
        elif kind == "strided":
            assert lib.mono_reduce_blocks(case[1] * case[2]) == R.reduce_plan(case[1] * case[2])[0], case
        elif kind == "any":
            assert lib.mono_colsum_any_blocks(case[1]) == R.colsum_any_plan(case[1])[0], case
        elif kind == "levels":
            _, B, S, C, bounds, _ = case
            flat = _int_array([v for ab in bounds for v in ab])
            assert lib.mono_colsum_levels_blocks(B, S, len(bounds), flat) == sum(g for g, _ in R.colsum_levels_plan(B, S, bounds)), case
    for rows in list(range(1, 300)) + [65535, 65536, 65537, 131072, 131073, 163200, 1 << 20, (1 << 20) + 1]:
        assert lib.mono_reduce_blocks(rows) == R.reduce_plan(rows)[0], rows
        assert lib.mono_colsum_any_blocks(rows) == R.colsum_any_plan(rows)[0], rows


# ---- mono_colsum_f32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [c[1:] for c in R.COLSUM_CASES])
def test_colsum_f32_is_exact(rows, C):
    g = _framed(R.colsum_operands(rows, C, seed=rows + C, device=DEV)["g"])
    grid, rpb = R.reduce_plan(rows)
    blocks = _lib().mono_reduce_blocks(rows)
    assert blocks == grid

    def put(r, col, v):
        g[r, col] = v
    _exact_then_planted(lambda out, scratch: _call("mono_colsum_f32", _p(g), _p(out), _p(scratch), rows, C),
                        lambda: g.double().sum(0), lambda: _plant(put, _row_candidates(rows, rpb, (grid - 1) * rpb), C),
                        1, C, blocks, "mono_colsum_f32 [%d, %d]" % (rows, C))


# ---- mono_colsum_any_f32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [c[1:] for c in R.ANY_CASES])
def test_colsum_any_f32_is_exact(rows, C):
    g = _framed(R.colsum_operands(rows, C, seed=rows + C, device=DEV)["g"])
    grid, rpb = R.colsum_any_plan(rows)
    blocks = _lib().mono_colsum_any_blocks(rows)
    assert blocks == grid

    def put(r, col, v):
        g[r, col] = v
    last_used = (rows - 1) // rpb * rpb
    _exact_then_planted(lambda out, scratch: _call("mono_colsum_any_f32", _p(g), _p(out), _p(scratch), rows, C),
                        lambda: g.double().sum(0), lambda: _plant(put, _row_candidates(rows, rpb, last_used, last_used + 3), C),
                        1, C, blocks, "mono_colsum_any_f32 [%d, %d]" % (rows, C))


@pytest.mark.parametrize("rows,C", [c[1:] for c in R.ANY_WRAPPER_CASES])
def test_colsum_wrapper_takes_odd_widths_exactly(rows, C):
    g = _framed(R.colsum_operands(rows, C, seed=rows + C, device=DEV)["g"])
    assert g.is_contiguous()
    _assert_exact(_pw().colsum(g), g.double().sum(0), "pointwise.colsum [%d, %d]" % (rows, C))


@pytest.mark.parametrize("rows,C", [(1, 4), (65, 260), (1025, 512), (65537, 256)])
def test_colsum_wrapper_takes_vector_widths_exactly(rows, C):
    g = _framed(R.colsum_operands(rows, C, seed=rows + C, device=DEV)["g"])
    _assert_exact(_pw().colsum(g), g.double().sum(0), "pointwise.colsum [%d, %d]" % (rows, C))


# ---- mono_colsum_strided_f32 -----------------------------------------------------------------------------------------------------------
def _strided(batch, rows, C, gap, seed, fill=None):
    """(flat NaN buffer, g3 = its [batch, rows, C] view with batch stride rows * C + gap, 8 * C NaN floats before and behind)."""
    stride = rows * C + gap
    front = PAD * C
    buf = torch.full((front + (batch - 1) * stride + rows * C + front,), NAN, device=DEV)
    g3 = torch.as_strided(buf, (batch, rows, C), (stride, C, 1), front)
    g3.copy_(R.colsum_batched_operands(batch, rows, C, seed, DEV)["g"] if fill is None else fill)
    assert g3.data_ptr() % 16 == 0 and int(torch.isnan(buf).sum()) == 2 * front + (batch - 1) * gap
    return buf, g3, stride


@pytest.mark.parametrize("batch,rows,C,gap", [c[1:] for c in R.STRIDED_CASES])
def test_colsum_strided_f32_is_exact(batch, rows, C, gap):
    buf, g3, stride = _strided(batch, rows, C, gap, seed=batch * rows + C)
    total = batch * rows
    grid, rpb = R.reduce_plan(total)
    blocks = _lib().mono_reduce_blocks(total)
    assert blocks == grid

    def put(v, col, val):
        g3[v // rows, v % rows, col] = val
    cand = _row_candidates(total, rpb, (batch - 1) * rows, rows - 1, rows)
    _exact_then_planted(lambda out, scratch: _call("mono_colsum_strided_f32", _p(g3), _p(out), _p(scratch), batch, rows, stride, C),
                        lambda: g3.double().sum((0, 1)), lambda: _plant(put, cand, C),
                        1, C, blocks, "mono_colsum_strided_f32 [%d, %d, %d] gap %d" % (batch, rows, C, gap))


def test_colsum_strided_f32_tells_batches_apart():
    """Every batch holds its own number in every element: the sum is rows * (1 + 2 + ... ) only when each batch is read once."""
    batch, rows, C, gap = 5, 65, 8, 8
    fill = torch.arange(1, batch + 1, device=DEV, dtype=torch.float32).view(batch, 1, 1).expand(batch, rows, C)
    buf, g3, stride = _strided(batch, rows, C, gap, 0, fill)
    out, scratch = _out(1, C), _scratch(_lib().mono_reduce_blocks(batch * rows), C)
    assert _call("mono_colsum_strided_f32", _p(g3), _p(out), _p(scratch), batch, rows, stride, C) == 0
    torch.cuda.synchronize()
    _assert_exact(out[0], torch.full((C,), float(rows * 15), dtype=torch.float64, device=DEV), "batches 1..5")


# ---- mono_colsum_levels_f32 ------------------------------------------------------------------------------------------------------------
def _leveled(B, S, C, bounds, seed):
    """g3 [B, S, C] between NaN rows; the rows of no level are NaN."""
    g3 = _framed(R.colsum_batched_operands(B, S, C, seed, DEV)["g"].view(B * S, C)).view(B, S, C)
    owned = torch.zeros(S, dtype=torch.bool, device=DEV)
    for a, b in bounds:
        owned[a:b] = True
    g3[:, ~owned] = NAN
    return g3


def _level_want(g3, bounds, with_total):
    sums = torch.stack([g3[:, a:b].double().sum((0, 1)) for a, b in bounds])
    return torch.cat([sums, sums.sum(0, keepdim=True)]) if with_total else sums


def _level_positions(B, bounds, plan):
    """(batch, row) of each level's first rows, workgroup edge, last rows and last batch."""
    pos = []
    for (a, b), (grid, rpb) in zip(bounds, plan):
        n = b - a
        for v in (0, 3, rpb - 1, rpb, B * n - 1, (B - 1) * n):
            if 0 <= v < B * n:
                pos.append((v // n, a + v % n))
    return pos


@pytest.mark.parametrize("B,S,C,bounds,with_total", [c[1:] for c in R.LEVEL_CASES])
def test_colsum_levels_f32_is_exact(B, S, C, bounds, with_total):
    g3 = _leveled(B, S, C, bounds, seed=S + C)
    L = len(bounds)
    flat = _int_array([v for ab in bounds for v in ab])
    plan = R.colsum_levels_plan(B, S, bounds)
    blocks = _lib().mono_colsum_levels_blocks(B, S, L, flat)
    assert blocks == sum(g for g, _ in plan) > 0

    def put(pos, col, v):
        g3[pos[0], pos[1], col] = v
    _exact_then_planted(lambda out, scratch: _call("mono_colsum_levels_f32", _p(g3), _p(out), _p(scratch), B, S, C, L, flat, with_total),
                        lambda: _level_want(g3, bounds, with_total), lambda: _plant(put, _level_positions(B, bounds, plan), C),
                        L + with_total, C, blocks, "mono_colsum_levels_f32 [%d, %d, %d] %s total %d" % (B, S, C, list(bounds), with_total))


@pytest.mark.parametrize("with_total", [False, True])
@pytest.mark.parametrize("C", [4, 256, 384, 512])
@pytest.mark.parametrize("B,S", [(1, 5), (3, 131), (4, 777)])
def test_colsum_levels_wrapper_takes_nine_levels_one_by_one(B, S, C, with_total):
    bounds = R.NINE_LEVELS[S]
    g3 = _leveled(B, S, C, bounds, seed=S + C + 1)
    got = _pw().colsum_levels(g3, bounds, with_total=with_total)
    want = _level_want(g3, bounds, False)
    what = "pointwise.colsum_levels, 9 levels of [%d, %d, %d]" % (B, S, C)
    if with_total:
        _assert_exact(got[0], want, what)
        _assert_exact(got[1], want.sum(0), what + ", total")
    else:
        _assert_exact(got, want, what)
    # the same bounds without the ninth level go through the one launch pair and agree
    eight = _pw().colsum_levels(g3, bounds[:8], with_total=with_total)
    _assert_exact(eight[0] if with_total else eight, want[:8], what + ", first eight")
    if with_total:
        _assert_exact(eight[1], want[:8].sum(0), what + ", total of eight")


# ---- mono_sum_slices_f32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C", [c[1:] for c in R.SLICES_CASES])
def test_sum_slices_f32_is_exact(n, C):
    x = _framed(R.slices_operands(n, C, seed=n + C, device=DEV)["x"])

    def put(r, col, v):
        x[r, col] = v
    _exact_then_planted(lambda out, scratch: _call("mono_sum_slices_f32", _p(x), _p(out), n, C),
                        lambda: x.double().sum(0), lambda: _plant(put, _row_candidates(n, 16, 14, 17), C),
                        1, C, 0, "mono_sum_slices_f32 [%d, %d]" % (n, C))


@pytest.mark.parametrize("n", [1, 17, 64])
def test_sum_slices_wrapper_is_exact(n):
    x = _framed(R.slices_operands(n, 260, seed=n, device=DEV)["x"])
    _assert_exact(_pw().sum_slices(x.view(n, 5, 52)), x.double().sum(0).view(5, 52), "pointwise.sum_slices [%d, 5, 52]" % n)


# ---- mono_relu_dropout_bwd_colsum_f32 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,p", [c[1:] for c in R.RELU_DROPOUT_CASES])
def test_relu_dropout_bwd_colsum_f32_is_exact(rows, p):
    o = R.relu_dropout_colsum_operands(rows, seed=rows, device=DEV)
    gy, y = _framed(o["gy"]), _framed(o["y"])
    scale = 1.0 / (1.0 - p)
    assert scale in (1.0, 2.0)
    grid, _ = R.reduce_plan(rows)
    blocks = _lib().mono_reduce_blocks(rows)
    assert blocks == grid
    what = "mono_relu_dropout_bwd_colsum_f32 [%d, 256] p %g" % (rows, p)
    state = {}

    def launch(out, scratch):
        state["gh"] = gh = R.with_canary(torch.full((rows, 256), R.SENTINEL, device=DEV), PAD, 0, R.SENTINEL, rows_before=PAD)
        return _call("mono_relu_dropout_bwd_colsum_f32", _p(gy), _p(y), _p(gh), _p(out), _p(scratch), rows, p)

    def want():
        gh64 = R.relu_backward64(y, gy) * scale
        state["want"] = gh64
        return gh64.sum(0)

    def put(r, col, v):
        gy[r, col] = v
        y[r, col] = 1.0                                    # a live element: the planted gradient passes
    for planted in (False, True):
        if planted:
            _plant(put, _row_candidates(rows, 4 * grid), 256)
        out, scratch = _out(1, 256), _scratch(blocks, 256)
        assert launch(out, scratch) == 0
        torch.cuda.synchronize()
        total, gh = want(), state["gh"]
        if planted:
            assert not torch.isfinite(total).all()
            assert R.same_nonfinite(gh, state["want"].to(torch.float32)) and R.same_nonfinite(out[0], total.to(torch.float32)), what
        else:
            _assert_exact(gh, state["want"], what + ", grad_h")
            _assert_exact(out[0], total, what + ", column sums")
            assert (gh == 0).any() and (state["want"] != 0).any()
        assert R.surroundings_hold(out, R.SENTINEL) and R.surroundings_hold(gh, R.SENTINEL) and _tail_holds(scratch), what


# ---- the same bits twice, and at another address ---------------------------------------------------------------------------------------
def _bits_cases():
    lib = _lib()
    g = torch.Generator(device=DEV).manual_seed(11)
    rn = lambda *shape: torch.randn(*shape, generator=g, device=DEV)
    bounds = R.level_sets(131)["tiled"]
    flat = _int_array([v for ab in bounds for v in ab])
    return {
        "colsum": ([rn(1025, 260)], lib.mono_reduce_blocks(1025) * 260, (1, 260),
                   lambda t, out, s: _call("mono_colsum_f32", _p(t[0]), _p(out), _p(s), 1025, 260)),
        "any": ([rn(1025, 81)], lib.mono_colsum_any_blocks(1025) * 81, (1, 81),
                lambda t, out, s: _call("mono_colsum_any_f32", _p(t[0]), _p(out), _p(s), 1025, 81)),
        "strided": ([rn(5 * (65 * 260 + 4))], lib.mono_reduce_blocks(5 * 65) * 260, (1, 260),
                    lambda t, out, s: _call("mono_colsum_strided_f32", _p(t[0]), _p(out), _p(s), 5, 65, 65 * 260 + 4, 260)),
        "levels": ([rn(3, 131, 384)], lib.mono_colsum_levels_blocks(3, 131, len(bounds), flat) * 384, (len(bounds) + 1, 384),
                   lambda t, out, s: _call("mono_colsum_levels_f32", _p(t[0]), _p(out), _p(s), 3, 131, 384, len(bounds), flat, 1)),
        "slices": ([rn(33, 260)], 4, (1, 260),
                   lambda t, out, s: _call("mono_sum_slices_f32", _p(t[0]), _p(out), 33, 260)),
        "relu_dropout": ([rn(1025, 256), rn(1025, 256), torch.empty(1025, 256, device=DEV)], lib.mono_reduce_blocks(1025) * 256, (1, 256),
                         lambda t, out, s: _call("mono_relu_dropout_bwd_colsum_f32", _p(t[0]), _p(t[1]), _p(t[2]), _p(out), _p(s), 1025, 0.5)),
    }


@pytest.mark.parametrize("kind", ["colsum", "any", "strided", "levels", "slices", "relu_dropout"])
def test_same_bits_twice_and_at_another_address(kind):
    tensors, scratch_floats, out_shape, launch = _bits_cases()[kind]
    keep = []                                             # every buffer stays alive: the next one is placed elsewhere

    def run(ts):
        out = torch.full(out_shape, R.SENTINEL, device=DEV)
        scratch = torch.full((scratch_floats,), NAN, device=DEV)
        keep.extend([out, scratch])
        assert launch(ts, out, scratch) == 0
        torch.cuda.synchronize()
        return out
    a, b = run(tensors), run(tensors)
    hold = torch.empty(12345, device=DEV)
    moved = [t.clone() for t in tensors]
    assert all(m.data_ptr() != t.data_ptr() for m, t in zip(moved, tensors))
    c = run(moved)
    del hold
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), "%s: two launches on the same buffers differ" % kind
    assert torch.equal(a, c), "%s: the result depends on where the operands lie" % kind
    if kind == "relu_dropout":
        assert torch.equal(tensors[2], moved[2])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_every_return_code_and_nothing_written_after_a_refusal():
    rows, C = 8, 8
    g = torch.zeros(4 * rows * C + 8, device=DEV)            # enough for every accepted shape below
    g256 = torch.zeros(rows * 256, device=DEV)
    out = torch.full((16 * 256,), R.SENTINEL, device=DEV)
    gh = torch.full((rows * 256,), R.SENTINEL, device=DEV)
    scratch = torch.full((16 * 1024,), R.SENTINEL, device=DEV)
    P = lambda t: t.data_ptr()
    bounds = _int_array([0, 2, 3, 8])

    def each_null(name, ptrs, rest, expect=-1):
        for i in range(len(ptrs)):
            args = list(ptrs)
            args[i] = None
            assert _call(name, *args, *rest) == expect, (name, "null pointer", i)

    each_null("mono_colsum_f32", [P(g), P(out), P(scratch)], [rows, C])
    each_null("mono_colsum_any_f32", [P(g), P(out), P(scratch)], [rows, C])
    each_null("mono_colsum_strided_f32", [P(g), P(out), P(scratch)], [2, rows, rows * C, C])
    each_null("mono_colsum_levels_f32", [P(g), P(out), P(scratch)], [2, rows, C, 2, bounds, 1])
    each_null("mono_sum_slices_f32", [P(g), P(out)], [rows, C])
    each_null("mono_relu_dropout_bwd_colsum_f32", [P(g256), P(g256), P(gh), P(out), P(scratch)], [rows, 0.5])

    colsum = lambda r, c: _call("mono_colsum_f32", P(g), P(out), P(scratch), r, c)
    for r, c in ((rows, 6), (rows, 1028), (rows, 0), (rows, -4), (0, C), (-1, C)):
        assert colsum(r, c) == -2, ("mono_colsum_f32", r, c)
    any_ = lambda r, c: _call("mono_colsum_any_f32", P(g), P(out), P(scratch), r, c)
    for r, c in ((rows, 1025), (rows, 0), (0, C), (-1, C)):
        assert any_(r, c) == -2, ("mono_colsum_any_f32", r, c)
    strided = lambda b, r, stride, c: _call("mono_colsum_strided_f32", P(g), P(out), P(scratch), b, r, stride, c)
    for b, r, stride, c in ((2, rows, rows * 6, 6), (2, rows, rows * 516, 516), (2, rows, rows * C, 0), (0, rows, rows * C, C), (-1, rows, rows * C, C),
                            (2, 0, rows * C, C), (2, -1, rows * C, C), (2, rows, rows * C + 2, C), (2, rows, rows * C + 1, C)):
        assert strided(b, r, stride, c) == -2, ("mono_colsum_strided_f32", b, r, stride, c)
    levels = lambda b, s, c, n, bd: _call("mono_colsum_levels_f32", P(g), P(out), P(scratch), b, s, c, n, bd, 1)
    for b, s, c in ((2, rows, 6), (2, rows, 516), (2, rows, 0), (0, rows, C), (-1, rows, C)):
        assert levels(b, s, c, 2, bounds) == -2, ("mono_colsum_levels_f32", b, s, c)
    lib = _lib()
    nine = _int_array([0, 1] * 9)
    for what, n, bd in (("a < 0", 2, _int_array([-1, 2, 3, 8])), ("b == a", 2, _int_array([0, 2, 3, 3])), ("b < a", 2, _int_array([0, 2, 5, 3])),
                        ("b > S", 2, _int_array([0, 2, 3, 9])), ("no level", 0, bounds), ("nine levels", 9, nine), ("null bounds", 2, None)):
        assert lib.mono_colsum_levels_blocks(2, rows, n, bd) == 0, what
        assert levels(2, rows, C, n, bd) == -2, what
    assert lib.mono_colsum_levels_blocks(2, rows, 2, bounds) == 2 and lib.mono_colsum_levels_blocks(0, rows, 2, bounds) == 0
    slices = lambda x, o, n, c: _call("mono_sum_slices_f32", x, o, n, c)
    for x, o, n, c in ((P(g), P(out), rows, 6), (P(g), P(out), rows, 0), (P(g), P(out), 0, C), (P(g), P(out), -1, C),
                       (P(g) + 4, P(out), rows, C), (P(g) + 8, P(out), rows, C), (P(g), P(out) + 4, rows, C), (P(g), P(out) + 8, rows, C)):
        assert slices(x, o, n, c) == -2, ("mono_sum_slices_f32", x % 16, o % 16, n, c)
    rd = lambda a, b, c, r, p: _call("mono_relu_dropout_bwd_colsum_f32", a, b, c, P(out), P(scratch), r, p)
    for a, b, c, r, p in ((P(g256), P(g256), P(gh), 0, 0.5), (P(g256), P(g256), P(gh), -1, 0.5), (P(g256), P(g256), P(gh), rows, 1.0),
                          (P(g256), P(g256), P(gh), rows, -0.5), (P(g256), P(g256), P(gh), rows, NAN), (P(g256) + 4, P(g256), P(gh), rows - 1, 0.5),
                          (P(g256), P(g256) + 4, P(gh), rows - 1, 0.5), (P(g256), P(g256), P(gh) + 4, rows - 1, 0.5)):
        assert rd(a, b, c, r, p) == -2, ("mono_relu_dropout_bwd_colsum_f32", a % 16, b % 16, c % 16, r, p)
    torch.cuda.synchronize()
    for name, t in (("out", out), ("grad_h", gh), ("scratch", scratch)):
        assert (t == R.SENTINEL).all(), "%s was written by a refused call" % name
    # and the same arguments, made good, are served
    assert colsum(rows, C) == 0 and any_(rows, C) == 0 and strided(2, rows, rows * C + 4, C) == 0 and levels(2, rows, C, 2, bounds) == 0
    assert slices(P(g), P(out), rows, C) == 0 and rd(P(g256), P(g256), P(gh), rows, 0.5) == 0
    torch.cuda.synchronize()


# ---- the wrappers' fallbacks -----------------------------------------------------------------------------------------------------------
def _unserved_layouts(shape, seed):
    """name -> integer tensor of ``shape`` (last dimension C) that the kernels do not serve: a view with a row pitch of 2 C, and a
    contiguous one that starts 4 bytes off a 16-byte boundary."""
    n = 1
    for s in shape:
        n *= s
    vals = R.ints(shape, -R.MAT_MAX, R.MAT_MAX, R._gen(seed, DEV), DEV)
    wide = torch.full(tuple(shape[:-1]) + (2 * shape[-1],), NAN, device=DEV)
    view = wide[..., :shape[-1]]
    view.copy_(vals)
    flat = torch.full((n + 1,), NAN, device=DEV)
    off = flat[1:].view(shape)
    off.copy_(vals)
    assert not view.is_contiguous() and off.is_contiguous() and off.data_ptr() % 16 == 4
    return {"non-contiguous": view, "misaligned": off}


def test_wrappers_fall_back_to_torch_exactly(monkeypatch):
    pw = _pw()
    bounds = R.level_sets(131)["gapped"]
    served = R.ints((3, 131, 8), -R.MAT_MAX, R.MAT_MAX, R._gen(1, DEV), DEV)
    want_served = _level_want(served, bounds, False)
    _assert_exact(pw.colsum_levels(served, bounds), want_served, "colsum_levels, served")           # the kernel path, before load() is barred

    def barred():
        raise AssertionError("a kernel path was taken")
    monkeypatch.setattr(pw, "load", barred)
    cases = dict(_unserved_layouts((129, 260), 2))
    cases["wider than 512"] = R.colsum_operands(129, 516, 3, DEV)["g"]
    cases["3 floats wide"] = R.colsum_operands(129, 3, 4, DEV)["g"]
    for name, g in cases.items():
        _assert_exact(pw.colsum(g), g.double().sum(0), "colsum, " + name)
    cases = dict(_unserved_layouts((3, 131, 260), 5))
    cases["wider than 512"] = R.colsum_batched_operands(3, 131, 516, 6, DEV)["g"]
    cases["3 floats wide"] = R.colsum_batched_operands(3, 131, 3, 7, DEV)["g"]
    for name, g3 in cases.items():
        for levels in (bounds, R.NINE_LEVELS[131]):
            want = _level_want(g3, levels, False)
            _assert_exact(pw.colsum_levels(g3, levels), want, "colsum_levels, " + name)
            got, total = pw.colsum_levels(g3, levels, with_total=True)
            _assert_exact(got, want, "colsum_levels with total, " + name)
            _assert_exact(total, want.sum(0), "colsum_levels total, " + name)
    cases = dict(_unserved_layouts((17, 260), 8))
    cases["3 floats per slice"] = R.slices_operands(17, 3, 9, DEV)["x"]
    cases["one dimension"] = R.slices_operands(1, 260, 10, DEV)["x"][0]
    for name, t in cases.items():
        _assert_exact(pw.sum_slices(t), t.double().sum(0), "sum_slices, " + name)


@pytest.mark.parametrize("one_launch", [1, 0])
def test_colsum_levels_raises_for_unusable_bounds(monkeypatch, one_launch):
    pw = _pw()
    monkeypatch.setattr(pw, "COLSUM_LEVELS_ONE_LAUNCH", one_launch)
    B, S, C = 2, 16, 8
    g3 = _framed(R.colsum_batched_operands(B, S, C, 0, DEV)["g"].view(B * S, C)).view(B, S, C)
    good = [(0, 4), (5, 16)]
    _assert_exact(pw.colsum_levels(g3, good), _level_want(g3, good, False), "usable bounds")
    for bad in ([(-1, 4)], [(0, 4), (4, 4)], [(0, 4), (9, 5)], [(0, 17)], [(0, 4), (16, 17)], [], [(0, 1)] * 8 + [(3, 17)], [(0, 1)] * 8 + [(-2, 3)]):
        for with_total in (False, True):
            with pytest.raises(RuntimeError):
                pw.colsum_levels(g3, bad, with_total=with_total)
        with pytest.raises(RuntimeError):
            pw.colsum_levels(g3[..., :3], bad)                                         # the torch path checks them too
    torch.cuda.synchronize()
    _assert_exact(pw.colsum_levels(g3, good), _level_want(g3, good, False), "usable bounds, afterwards")
