"""The fp32 attention core (monosowa_amd/csrc/flash_attn.hip: fwd_kernel, bwd_dq_kernel, bwd_dkdv_kernel) against float64 where
unit-normal inputs at the default scale cannot reach: peaked rows and logits of 50 - 80, a running maximum that climbs or is
wiped out by a late key, non-default softmax scales, lse itself, every tile edge of the three kernels, head / image indexing up
to the grid limit, mixed memory layouts in one call, dropout over several tiles against the recovered mask, the statistics of
that mask, bit repeatability, and masks the model does not produce.

Tolerance (``_compare``).  For each of o, dq, dk, dv, lse: e32 = max |reference(float32) - reference(float64)| with both
evaluated by PyTorch's own operators on the GPU on the same inputs, ek = max |kernel - reference(float64)|, and
    ek <= max(1e-5 max|x64|, M e32).
The first term is the project's standing tolerance; the second lets the kernels be as inaccurate as float32 arithmetic itself is
on peaked inputs, times the margin M below.  The ``randn`` regime is held to the plain 1e-5 (M = 0).  lse of the kernels is in
the log2 domain and converted with ln 2."""
import math

import pytest
import torch

import attention_reference as AR

pytestmark = pytest.mark.gpu

LN2 = math.log(2.0)
NAMES = ("o", "dq", "dk", "dv", "lse")
# Margin on the float32 yardstick: twice the worst measured ek / e32, rounded up to a power of two.  Worst ek / e32 per regime and
# quantity on the MI355X (section a, both shapes):
#                      o     dq    dk    dv    lse
#   randn             0.92  1.51  1.65  0.87  1.01
#   sharp             1.00  1.92  2.26  1.35  1.12
#   offset            1.14  2.05  0.99  0.98  0.94
#   ascending         1.05  1.23  1.35  1.48  1.04
#   descending        1.12  1.25  3.77  1.00  1.04
#   late_spike        0.73  1.81  2.29  2.03  0.99
#   early_spike       1.10  2.32  2.97  1.43  0.93
#   scale_zero        1.35   -     -    1.31  1.49      (dq = dk = 0 in all three evaluations)
#   scale_one         0.87  1.60  1.35  1.03  0.97
#   scale_negative    1.51  1.13  1.00  1.29  1.01
# and over the tile edges (section b): randn 1.83 3.70 2.86 2.54 1.26, sharp 1.73 3.20 3.15 3.60 1.87.  Worst 3.77, twice that 7.5.
# The second term of the bound decides only for dq and dk of the two spike regimes (ek up to 8e-4 of max|x64|, ek / e32 <= 2.97);
# everywhere else ek <= 1e-5 max|x64| as well.
# (Before bwd_dkdv rebuilt its scores from the forward's own products the worst was 4.28, dv of `sharp`, and 17.9 for dv of a
# single key -- a margin of 16 and 64: the finding behind that change, csrc/flash_attn.hip.)
M = 8.0


def _fa():
    from monosowa_amd import flash_attn as FA
    return FA


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _kernels(q, k, v, go, scale, kpm=None, p=0.0, seed=0):
    """o and lse (natural log, [B, H, Lq]) from FA.forward, dq / dk / dv through FA.attention(..., scale=scale)"""
    FA = _fa()
    B, H, Lq, _ = q.shape
    o, lse = FA.forward(q, k, v, scale, p, seed, key_padding_mask=kpm)
    qg, kg, vg = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    FA.attention(qg, kg, vg, dropout_p=p, scale=scale, seed=seed, key_padding_mask=kpm).backward(go)
    return o, qg.grad, kg.grad, vg.grad, lse.view(B, H, Lq).double() * LN2


def _references(q, k, v, go, scale, **kw):
    return AR.reference(q, k, v, go, scale, **kw), AR.reference(q, k, v, go, scale, dtype=torch.float32, **kw)


def _compare(what, got, ref64, ref32, m, pick=None):
    """every quantity is measured and printed before the first one may fail; pick: restricts all three to a part of the result"""
    bad = []
    for name, g, x64, x32 in zip(NAMES, got, ref64, ref32):
        if pick is not None:
            g, x64, x32 = pick(g), pick(x64), pick(x32)
        assert torch.isfinite(x64).all() and torch.isfinite(x32).all(), (what, name)
        ek = (g.double() - x64).abs().max().item()
        e32 = (x32.double() - x64).abs().max().item()
        mx = x64.abs().max().item()
        bound = max(1e-5 * mx, m * e32)
        print("ATTN-ERR %s %s ek %.3e e32 %.3e max %.3e ek/e32 %.2f ek/max %.2e" % (what, name, ek, e32, mx, ek / e32 if e32 else float("inf") if ek else 0.0, ek / mx if mx else float("inf") if ek else 0.0))
        if not ek <= bound:                                  # (a NaN fails)
            bad.append("%s: error %.3e above max(1e-5 * %.3e, %g * %.3e)" % (name, ek, mx, m, e32))
    assert not bad, "%s: %s" % (what, "; ".join(bad))


def _margin(regime):
    return 0.0 if regime == "randn" else M


def _pad_mask(B, Lk):
    """the last min(5, Lk - 1) keys of image 0 are padding"""
    kpm = torch.zeros(B, Lk, dtype=torch.bool, device="cuda")
    n = min(5, Lk - 1)
    if n:
        kpm[0, Lk - n:] = True
    return kpm


# ---------------------------------------------------------------------------------------------------------------- a. regimes
@pytest.mark.parametrize("shape", [(2, 3, 130, 200), (1, 2, 257, 193)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("regime", AR.REGIMES)
def test_regime_matches_float64(regime, shape):
    """o and lse of FA.forward, dq / dk / dv of FA.attention(scale=scale) in every input regime of attention_reference.make_case."""
    q, k, v, go, scale = AR.make_case(regime, *shape, _gen(7))
    got = _kernels(q, k, v, go, scale)
    ref64, ref32 = _references(q, k, v, go, scale)
    _compare("regime %s %s" % (regime, "x".join(map(str, shape))), got, ref64, ref32, _margin(regime))
    if regime == "scale_zero":
        assert (got[1] == 0).all() and (got[2] == 0).all()
        assert (got[0] - v.mean(2, keepdim=True)).abs().max().item() <= 1e-6


# ------------------------------------------------------------------------------------------------------------- b. tile edges
_EDGES = [(lq, lk) for lq in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257) for lk in (65, 129)]
_EDGES += [(lq, lk) for lq in (33, 129) for lk in (1, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 257) if (lq, lk) not in _EDGES]


@pytest.mark.parametrize("Lq,Lk", _EDGES)
@pytest.mark.parametrize("regime", ["randn", "sharp"])
def test_tile_edges_match_float64_with_and_without_padded_keys(regime, Lq, Lk):
    """Lq and Lk at and next to 32 (a key half), 64 (a key tile; the query tile of dK / dV) and 128 (the workgroup's rows of the
    forward and dQ, its keys in dK / dV), once without a mask and once with the last keys of image 0 padded: those keys' dk and dv
    are exactly 0.  With a single key dq and dk are 0 in float64 and in float32, so the bound is 0 there: the kernels have to
    cancel dP - delta exactly."""
    B, H = 2, 3
    q, k, v, go, scale = AR.make_case(regime, B, H, Lq, Lk, _gen(1000 * Lq + Lk))
    for kpm in (None, _pad_mask(B, Lk)):
        got = _kernels(q, k, v, go, scale, kpm=kpm)
        ref64, ref32 = _references(q, k, v, go, scale, key_padding_mask=kpm)
        _compare("edge %s %dx%d %s" % (regime, Lq, Lk, "nomask" if kpm is None else "keypad"), got, ref64, ref32, _margin(regime))
        if kpm is not None:
            dead = kpm[:, None, :, None].expand_as(got[2])
            assert (got[2][dead] == 0).all() and (got[3][dead] == 0).all()


# ------------------------------------------------------------------------------------------------- c. head and image indexing
@pytest.mark.parametrize("H", [1, 3, 8])
def test_every_plane_is_read_and_written_in_its_own_place(H):
    """The inputs of each (image, head) plane carry their own factor, and each plane is held to its own bound: a plane read from or
    written to another plane's place fails."""
    B, Lq, Lk = 3, 70, 130
    q, k, v, go, scale = AR.make_case("randn", B, H, Lq, Lk, _gen(H))
    factor = (0.5 + torch.arange(B * H, device="cuda", dtype=torch.float32) / (B * H)).view(B, H, 1, 1)
    q, k, v, go = q * factor, k * factor, v * factor, go * factor
    got = _kernels(q, k, v, go, scale)
    ref64, ref32 = _references(q, k, v, go, scale)
    for b in range(B):
        for h in range(H):
            _compare("plane %d.%d of %dx%d" % (b, h, B, H), got, ref64, ref32, 0.0, pick=lambda t: t[b, h])


def test_the_last_plane_of_the_largest_grid():
    """B * H = 65535, the most the grid's y dimension takes, with one query and one key: o = v, dv = go and dq = dk = 0.  The
    values are chosen so that the kernels' arithmetic is exact in any summation order -- v and go are small integers, k has one
    power of two per plane in a channel of its own, q is a single scaled product -- so the identities hold bit for bit."""
    FA = _fa()
    B, H = 255, 257
    g = _gen(3)
    ints = lambda: torch.randint(-8, 9, (B, H, 1, 32), generator=g, device="cuda").float()
    v, go = ints(), ints()
    plane = torch.arange(B * H, device="cuda").view(B, H, 1)
    q = torch.randn(B, H, 1, 32, generator=g, device="cuda")
    k = torch.zeros(B, H, 1, 32, device="cuda")
    k.scatter_(3, (plane % 32)[..., None], (2.0 ** (plane % 5 - 2).float())[..., None])
    assert FA.supported(q, k, v)
    o, dq, dk, dv, lse = _kernels(q, k, v, go, 0.25)
    assert torch.equal(o, v)
    assert torch.equal(dv, go)
    assert (dq == 0).all() and (dk == 0).all()
    want_lse = ((q.double() * k.double()).sum(-1) * 0.25)
    assert (lse - want_lse).abs().max().item() <= 1e-5 * want_lse.abs().max().item()


def test_more_planes_than_the_grid_takes_are_refused():
    FA = _fa()
    q = torch.zeros(256, 256, 1, 32, device="cuda")
    assert not FA.supported(q, q, q)
    with pytest.raises(RuntimeError):
        FA.attention(q, q, q)


# -------------------------------------------------------------------------------------------------- d. mixed layouts in one call
def test_mixed_layouts_in_one_call():
    """q a view of an [Lq, B, H*32] buffer, k and v the two column halves of one [B, Lk, 2*H*32] buffer, go dense [B, H, Lq, 32]
    (the copy branch of _Attention.backward): float64 values, each gradient laid out like its own input (_like_heads), inputs
    untouched."""
    FA = _fa()
    B, H, Lq, Lk = 2, 3, 70, 130
    q0, k0, v0, go, scale = AR.make_case("randn", B, H, Lq, Lk, _gen(5))
    qbuf = torch.empty(Lq, B, H * 32, device="cuda")
    kvbuf = torch.empty(B, Lk, 2 * H * 32, device="cuda")
    q = qbuf.view(Lq, B, H, 32).permute(1, 2, 0, 3)
    k = kvbuf[..., :H * 32].view(B, Lk, H, 32).permute(0, 2, 1, 3)
    v = kvbuf[..., H * 32:].view(B, Lk, H, 32).permute(0, 2, 1, 3)
    q.copy_(q0), k.copy_(k0), v.copy_(v0)
    assert torch.equal(q, q0) and torch.equal(k, k0) and torch.equal(v, v0) and FA.supported(q, k, v)
    saved = qbuf.clone(), kvbuf.clone(), go.clone()
    qg, kg, vg = (t.detach().requires_grad_(True) for t in (q, k, v))
    assert qg.stride() == q.stride() and kg.stride() == k.stride() and vg.stride() == v.stride()
    out = FA.attention(qg, kg, vg, scale=scale)
    assert out.stride() == (H * 32, 32, B * H * 32, 1) and go.stride() != out.stride()
    dq, dk, dv = torch.autograd.grad(out, (qg, kg, vg), go)
    o, lse = FA.forward(q, k, v, scale, 0.0, 0)
    assert torch.equal(o, out)
    ref64, ref32 = _references(q0, k0, v0, go, scale)
    _compare("mixed layouts", (o, dq, dk, dv, lse.view(B, H, Lq).double() * LN2), ref64, ref32, 0.0)
    assert dq.stride() == (H * 32, 32, B * H * 32, 1)                      # like q: [Lq, B, H*32]
    assert dk.stride() == (Lk * H * 32, 32, H * 32, 1)                     # like k: batch-major, dense [B, Lk, H*32]
    assert dv.stride() == (Lk * H * 32, 32, H * 32, 1)
    assert torch.equal(qbuf, saved[0]) and torch.equal(kvbuf, saved[1]) and torch.equal(go, saved[2])


# ---------------------------------------------------------------------------------------------- e. dropout over several tiles
def _thr(p):
    return int(p * 65536 + 0.5)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "keypad"])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_over_several_tiles_matches_float64_through_the_recovered_mask(p, masked):
    """Three query blocks and four key tiles: FA.forward's output, FA.attention's gradients and FA.backward's, from the saved
    keep bits and re-hashed, against float64 through the mask recover_keep reads out of the forward."""
    FA = _fa()
    B, H, Lq, Lk, seed = 2, 3, 260, 200, 2024
    q, k, v, go, scale = AR.make_case("randn", B, H, Lq, Lk, _gen(17))
    kpm = None
    if masked:
        kpm = torch.zeros(B, Lk, dtype=torch.bool, device="cuda")
        kpm[0, Lk - 37:] = True
        kpm[1, 3::11] = True
    keep = AR.recover_keep(q, k, scale, p, seed, key_padding_mask=kpm)
    assert keep.shape == (B, H, Lq, Lk) and keep.dtype == torch.bool
    if kpm is not None:
        assert not keep[kpm[:, None, None, :].expand_as(keep)].any()
    kw = dict(key_padding_mask=kpm, keep=keep, keep_scale=65536.0 / (65536 - _thr(p)))
    ref64, ref32 = _references(q, k, v, go, scale, **kw)
    what = "dropout %.1f %s" % (p, "keypad" if masked else "nomask")
    _compare(what + " attention()", _kernels(q, k, v, go, scale, kpm=kpm, p=p, seed=seed), ref64, ref32, 0.0)
    bits = FA.keep_bits_like(q, k, p)
    bits.fill_(-1)
    o, lse = FA.forward(q, k, v, scale, p, seed, key_padding_mask=kpm, keep_bits=bits)
    lse_n = lse.view(B, H, Lq).double() * LN2
    saved = FA.backward(q, k, v, o, lse, go, scale, p, seed, key_padding_mask=kpm, keep_bits=bits)
    _compare(what + " saved bits", (o,) + tuple(saved) + (lse_n,), ref64, ref32, 0.0)
    rehashed = FA.backward(q, k, v, o, lse, go, scale, p, seed, key_padding_mask=kpm)
    _compare(what + " re-hashed", (o,) + tuple(rehashed) + (lse_n,), ref64, ref32, 0.0)


# ------------------------------------------------------------------------------------------------------- f. mask statistics
def _six_sigma(rate, n):
    return 6.0 * math.sqrt(rate * (1.0 - rate) / n)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_statistics(p):
    """The mask of a (2, 3, 260, 200) call and of the next seed.  P = 1 - thr / 65536 is the exact keep probability of one 16-bit
    draw; every assertion allows the 6-sigma interval of the binomial share it looks at (derived, not measured).  Per p: 1 whole
    mask + 6 planes + 200 key columns + 260 query rows kept fractions, and 6 agreement rates against P^2 + (1 - P)^2 (two heads of
    one image, two images, the two 16-bit halves of one hash word, keys 32 apart, neighbouring queries, two seeds): 473
    assertions, 946 over both p.  The masks are a fixed function of the seed, so the outcome is the same on every run; had the
    seed been drawn afresh, 946 six-sigma intervals would raise a false alarm about once in 10^6 runs."""
    B, H, Lq, Lk, seed = 2, 3, 260, 200, 77
    q, k = torch.zeros(B, H, Lq, 32, device="cuda"), torch.zeros(B, H, Lk, 32, device="cuda")
    keep = AR.recover_keep(q, k, 1.0, p, seed).double()
    other = AR.recover_keep(q, k, 1.0, p, seed + 1).double()
    P = 1.0 - _thr(p) / 65536.0
    n_all = B * H * Lq * Lk

    def near(share, rate, n, what):
        worst = (share - rate).abs().max().item()
        assert worst <= _six_sigma(rate, n), "%s: %.5f off %.5f, 6 sigma = %.5f" % (what, worst, rate, _six_sigma(rate, n))
    near(keep.mean(), P, n_all, "whole mask")
    near(keep.mean((2, 3)), P, Lq * Lk, "planes")
    near(keep.mean((0, 1, 2)), P, B * H * Lq, "key columns")
    near(keep.mean((0, 1, 3)), P, B * H * Lk, "query rows")
    A = P * P + (1.0 - P) * (1.0 - P)
    agree = lambda a, b: (a == b).double().mean()
    near(agree(keep[0, 0], keep[0, 1]), A, Lq * Lk, "two heads of one image")
    near(agree(keep[0, 0], keep[1, 0]), A, Lq * Lk, "two images")
    near(agree(keep[..., 0::2], keep[..., 1::2]), A, n_all // 2, "the two halves of one hash word")
    near(agree(keep[..., :-32], keep[..., 32:]), A, B * H * Lq * (Lk - 32), "keys 32 apart")
    near(agree(keep[:, :, :-1], keep[:, :, 1:]), A, B * H * (Lq - 1) * Lk, "neighbouring queries")
    near(agree(keep, other), A, n_all, "two seeds")


# ------------------------------------------------------------------------------------------------------- g. bit repeatability
@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "dropout_keypad"])
def test_three_runs_give_the_same_bits(dropout):
    """Forward and backward three times into fresh buffers: o, lse, dq, dk, dv (and the keep bits) are torch.equal.  The keep bits
    buffer is the test's own and is poisoned before each run; the results are allocated inside FA.forward / FA.backward, so a
    NaN-filled block of each result's size is handed back to the allocator in front of every run."""
    FA = _fa()
    B, H, Lq, Lk = 2, 8, 300, 333
    q, k, v, go, scale = AR.make_case("randn", B, H, Lq, Lk, _gen(23))
    p, seed, kpm = 0.0, 0, None
    if dropout:
        p, seed = 0.1, 31337
        kpm = torch.rand(B, Lk, device="cuda", generator=_gen(24)) < 0.2
        kpm[:, 0] = False
    runs = []
    for _ in range(3):
        bits = FA.keep_bits_like(q, k, p)
        if bits is not None:
            bits.fill_(-1)
        poison = [torch.full((B, H, L, 32), float("nan"), device="cuda") for L in (Lq, Lq, Lk, Lk)]
        del poison
        o, lse = FA.forward(q, k, v, scale, p, seed, key_padding_mask=kpm, keep_bits=bits)
        dq, dk, dv = FA.backward(q, k, v, o, lse, go, scale, p, seed, key_padding_mask=kpm, keep_bits=bits)
        runs.append((o, lse, dq, dk, dv) + ((bits,) if bits is not None else ()))
    for x in runs[0][:5]:
        assert torch.isfinite(x).all()
    for other in runs[1:]:
        for name, a, b in zip(NAMES[:1] + ("lse", "dq", "dk", "dv", "keep bits"), runs[0], other):
            assert a.data_ptr() != b.data_ptr() and torch.equal(a, b), name


# -------------------------------------------------------------------------------------- h. masks the model does not produce
def test_uint8_and_strided_masks_give_the_bits_of_the_contiguous_bool_mask():
    B, H, Lq, Lk = 2, 3, 70, 130
    q, k, v, go, scale = AR.make_case("randn", B, H, Lq, Lk, _gen(41))
    kpm = torch.rand(B, Lk, device="cuda", generator=_gen(42)) < 0.3
    kpm[:, 0] = False
    wide = torch.zeros(B, 2 * Lk + 3, dtype=torch.bool, device="cuda")
    wide[:, 3::2] = kpm
    strided = wide[:, 3::2]
    assert not strided.is_contiguous() and torch.equal(strided, kpm)
    want = _kernels(q, k, v, go, scale, kpm=kpm)
    for name, mask in (("uint8", kpm.to(torch.uint8)), ("strided bool", strided)):
        for x, a, b in zip(NAMES, _kernels(q, k, v, go, scale, kpm=mask), want):
            assert torch.equal(a, b), (name, x)


def test_an_image_with_every_key_padded_is_nan_forward_and_backward_and_the_others_exact():
    """torch's softmax over a row of -inf is NaN, and so are the image's o and dv; its dq and dk are NaN as well when the mask is
    added to the logits, as nn.MultiheadAttention does (masked_fill, which the reference uses, hands its own zero gradient to a
    filled position).  The kernels give NaN for all four instead of inventing a value, and the other images (one of them partly
    padded) match float64 and are finite."""
    B, H, Lq, Lk = 3, 3, 70, 130
    q, k, v, go, scale = AR.make_case("randn", B, H, Lq, Lk, _gen(43))
    kpm = torch.zeros(B, Lk, dtype=torch.bool, device="cuda")
    kpm[1] = True
    kpm[2, 100:] = True
    got = _kernels(q, k, v, go, scale, kpm=kpm)
    ref64, ref32 = AR.reference(q, k, v, go, scale, key_padding_mask=kpm), AR.reference(q, k, v, go, scale, key_padding_mask=kpm, dtype=torch.float32)
    assert torch.isnan(ref64[0][1]).all() and torch.isnan(ref64[3][1]).all()
    for name, g in zip(NAMES[:4], got):
        assert torch.isnan(g[1]).all(), "%s of the all-padded image: %d of %d values are not NaN" % (name, (~torch.isnan(g[1])).sum().item(), g[1].numel())
    live = torch.tensor([0, 2], device="cuda")
    for x in got:
        assert torch.isfinite(x[live]).all()
    _compare("all-padded image, the others", got, ref64, ref32, 0.0, pick=lambda t: t[live])
