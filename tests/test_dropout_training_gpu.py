"""Train-mode dropout against references: the fused LayerNorm(x + dropout(z)) and ReLU-dropout kernels, the encoder's two
autograd nodes and the decoder / depth-encoder layers, with dropout ON.

The keep masks are read from the kernels themselves (tests/dropout_replay.py: the recorded seed replayed on constant
inputs), never restated: the properties below hold for any hash, and the references multiply by the probed masks.
Tolerances: elementwise results max|err| <= 2e-5 max|ref|; column sums (ggamma, gbeta, the fused bias sums) <= 2e-6 of the
largest column's sum of |terms| (as test_colsum_matches_torch); whole layers 3e-5 max(|ref|, 1e-3) (as the block test).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from monosowa_amd import pointwise
from monosowa_amd.pointwise import dropout_add_layernorm, ln_backward, relu_dropout_backward, relu_dropout_backward_colsum

import dropout_replay as R

pytestmark = pytest.mark.gpu


def ln_forward(*args):
    return pointwise.ln_forward(*args)              # looked up at call time: dropout_replay.record() wraps it


def relu_dropout_forward(*args):
    return pointwise.relu_dropout_forward(*args)

EPS = 1e-5
# rows -> (B, L) of the [B, L, 256] buffer whose [L, B, 256] view is the transposed layout; 1 and 3 rows fit in one pass of
# every grid, 4097 / 16,385 / 163,200 rows wrap the LayerNorm forward's (16,384 rows per pass) and the backward's grid-stride loops
ROWS = {1: (1, 1), 3: (3, 1), 4097: (17, 241), 16385: (5, 3277), 163200: (16, 10200)}


@pytest.fixture(autouse=True)
def _keep_seed_counter():
    saved = pointwise._seed_counter[0]
    yield
    pointwise._seed_counter[0] = saved


def _rows(rows, transposed, g=None):
    """A [.., 256] float32 tensor with ``rows`` rows: contiguous [rows, 256] or the [L, B, 256] view of a [B, L, 256] buffer."""
    B, L = ROWS[rows]
    if transposed:
        return torch.randn(B, L, 256, device="cuda", generator=g).transpose(0, 1)
    return torch.randn(rows, 256, device="cuda", generator=g)


def _close(got, ref, what, rel=2e-5):
    err = (got.double() - ref).abs().max().item()
    bound = rel * ref.abs().max().item()
    assert err <= bound, "%s: max|err| %.3e > %.3e" % (what, err, bound)


def _colsum_close(got, ref, terms, what, extra=0.0):
    """``terms``: [rows, C] whose column sums ``ref`` is; ``extra``: error the terms themselves carry in float32."""
    err = (got.double() - ref).abs().max().item()
    bound = 2e-6 * terms.abs().sum(0).max().item() + extra
    assert err <= bound, "%s: max|err| %.3e > %.3e" % (what, err, bound)


def _affine(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    gamma = torch.rand(256, device="cuda", generator=g) + 0.5
    beta = torch.rand(256, device="cuda", generator=g) - 0.5
    return gamma, beta


# ---- mask properties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True], ids=["contiguous", "LBC"])
@pytest.mark.parametrize("rows", sorted(ROWS))
def test_layernorm_backward_applies_the_forwards_mask(rows, transposed):
    """gz == gx * mask bitwise, and the forward's saved sum is x + z * mask, at row counts where the forward's and the
    backward's grids differ and their grid-stride loops wrap."""
    torch.manual_seed(rows)
    x = _rows(rows, transposed)
    z, gy = torch.randn_like(x), torch.randn_like(x)
    gamma, beta = _affine(rows)
    with R.record() as draws:
        y, s, mean, rstd, seed = ln_forward(x, z, gamma, beta, 0.3, EPS)
    assert [d.kind for d in draws] == ["ln"] and y.stride() == x.stride() == s.stride()
    mask = draws[0].mask()
    kept = mask[mask != 0].unique()
    assert kept.numel() == 1 and abs(kept.item() - 1 / 0.7) < 1e-6 and torch.equal(mask, R.ln_mask(seed, 0.3, x))
    assert torch.allclose(s, x + z * mask, rtol=1e-6, atol=1e-6)
    gx, gz, _, _, _ = ln_backward(gy, s, mean, rstd, gamma, 0.3, seed, with_gz_sum=True)
    assert gx.stride() == x.stride()
    assert torch.equal(gz, gx * mask)
    if rows > 16:
        assert 0.6 < (mask != 0).float().mean().item() < 0.8


@pytest.mark.parametrize("transposed", [False, True], ids=["contiguous", "LBC"])
@pytest.mark.parametrize("rows", sorted(ROWS))
def test_relu_dropout_backward_applies_the_forwards_mask(rows, transposed):
    """y == relu(h) * mask and gh == gy * mask * (h > 0) bitwise, through both backward entry points."""
    torch.manual_seed(rows + 1)
    h = _rows(rows, transposed)
    gy = torch.randn_like(h)
    with R.record() as draws:
        y = relu_dropout_forward(h, 0.3)
    assert [d.kind for d in draws] == ["relu"] and y.stride() == h.stride()
    mask = draws[0].mask()
    assert torch.equal(y, torch.relu(h) * mask)
    want = gy * mask * (h > 0)
    gh = relu_dropout_backward(gy, y, 0.3)
    gh2, _ = relu_dropout_backward_colsum(gy, y, 0.3)
    assert torch.equal(gh, want) and torch.equal(gh2, want)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_mask_statistics(p):
    """Kept fraction, per-channel keep rates, and the correlations between neighbouring elements, neighbouring rows, masks of
    consecutive seeds, and the ReLU-dropout and LayerNorm masks of one FFN block (consecutive draws) -- 5 sigma bounds."""
    torch.manual_seed(0)
    rows = 163200
    like = torch.empty(rows, 256, device="cuda")
    relu_seed, ln_seed, ln_seed2 = pointwise._next_seed(), pointwise._next_seed(), pointwise._next_seed()
    ln_keep = (R.ln_mask(ln_seed, p, like) != 0).double()
    n = ln_keep.numel()
    q = 1 - p
    assert abs(ln_keep.mean().item() - q) <= 5 * math.sqrt(p * q / n)
    assert (ln_keep.mean(0) - q).abs().max().item() <= 5 * math.sqrt(p * q / rows)
    relu_keep = (R.relu_mask(relu_seed, p, like) != 0).double()
    assert abs(relu_keep.mean().item() - q) <= 5 * math.sqrt(p * q / n)
    assert (relu_keep.mean(0) - q).abs().max().item() <= 5 * math.sqrt(p * q / rows)

    def corr(a, b):
        a, b = a.reshape(-1) - a.mean(), b.reshape(-1) - b.mean()
        return ((a * b).mean() / (a.square().mean() * b.square().mean()).sqrt()).item(), a.numel()
    pairs = {"neighbouring elements": (ln_keep[:, :-1], ln_keep[:, 1:]), "neighbouring rows": (ln_keep[:-1], ln_keep[1:]),
             "consecutive seeds": (ln_keep, (R.ln_mask(ln_seed2, p, like) != 0).double()),
             "relu vs LayerNorm": (relu_keep, ln_keep),
             "relu neighbouring elements": (relu_keep[:, :-1], relu_keep[:, 1:])}
    for name, (a, b) in pairs.items():
        r, m = corr(a, b)
        assert abs(r) <= 5 / math.sqrt(m), "%s: correlation %.2e" % (name, r)


def test_p0_is_a_plain_layernorm_and_draws_no_mask():
    torch.manual_seed(3)
    x, z, gy = (torch.randn(4097, 256, device="cuda") for _ in range(3))
    gamma, beta = _affine(3)
    counter = pointwise._seed_counter[0]
    y, s, mean, rstd, seed = ln_forward(x, z, gamma, beta, 0.0, EPS)
    assert seed == 0 and pointwise._seed_counter[0] == counter
    y0, s0, mean0, rstd0, _ = ln_forward(x + z, torch.zeros_like(z), gamma, beta, 0.0, EPS)
    assert torch.equal(y, y0) and torch.equal(s, s0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
    gx, gz, gg, gb, gzs = ln_backward(gy, s, mean, rstd, gamma, 0.0, 0, with_gz_sum=True)
    assert torch.equal(gx, gz)
    norm = torch.nn.LayerNorm(256).cuda()
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    drop = torch.nn.Dropout(0.0).train()
    _close(dropout_add_layernorm(x, z, norm, drop).detach(), F.layer_norm(x.double() + z.double(), (256,), gamma.double(), beta.double(), EPS), "y")
    assert pointwise._seed_counter[0] == counter


def test_resetting_the_seed_counter_reproduces_the_masks():
    """tools/deterministic_step.py replays a step by resetting pointwise._seed_counter."""
    torch.manual_seed(4)
    x, z, h = (torch.randn(16385, 256, device="cuda") for _ in range(3))
    gamma, beta = _affine(4)
    pointwise._seed_counter[0] = 100
    a = ln_forward(x, z, gamma, beta, 0.1, EPS)[0], relu_dropout_forward(h, 0.1)
    b = ln_forward(x, z, gamma, beta, 0.1, EPS)[0], relu_dropout_forward(h, 0.1)
    pointwise._seed_counter[0] = 100
    c = ln_forward(x, z, gamma, beta, 0.1, EPS)[0], relu_dropout_forward(h, 0.1)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


# ---- the kernels against float64 ------------------------------------------------------------------------------------------
LN_SHAPES = {"encoder": ((16, 10200), False), "decoder": ((16, 550), False), "depth_encoder": ((16, 1920), True),
             "7x1021": ((7, 1021), False), "1row": ((1,), False), "3rows": ((3,), False)}


def _ln_inputs(kind, lead, transposed, g):
    """x, z in the layout of the case: randn; rows offset by 100 with unit spread (a one-pass variance loses it); constant
    rows (values k / 4: the row sums are exact in float32) with z = 0."""
    x = torch.randn(*lead, 256, device="cuda", generator=g)
    z = torch.randn(*lead, 256, device="cuda", generator=g)
    if kind == "offset":
        x += 100
    elif kind == "constant":
        k = torch.randint(-40, 41, lead, device="cuda", generator=g).float() / 4
        x = k[..., None].expand_as(x).contiguous()
        z.zero_()
    if transposed:
        x = x.transpose(0, 1)
        z = z.transpose(0, 1).contiguous()          # another layout than x: the wrapper copies it into x's
    return x, z


@pytest.mark.parametrize("kind", ["randn", "offset", "constant"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", list(LN_SHAPES))
def test_layernorm_forward_and_backward_match_float64(shape, p, kind):
    """ln_forward / ln_backward(with_gz_sum=True) against float64 autograd of LayerNorm(x + z * mask): y, mean, rstd, gx, gz,
    ggamma, gbeta and the gz column sum (the bias gradient of output_proj / linear2 in the encoder blocks)."""
    lead, transposed = LN_SHAPES[shape]
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, shape + kind)) + int(p * 10))
    x, z = _ln_inputs(kind, lead, transposed, g)
    gy = torch.randn(x.shape, device="cuda", generator=g)
    gamma, beta = _affine(7)
    with R.record() as draws:
        y, s, mean, rstd, seed = ln_forward(x, z, gamma, beta, p, EPS)
    assert y.stride() == x.stride()
    mask = draws[0].mask().double()
    gx, gz, gg, gb, gzs = ln_backward(gy, s, mean, rstd, gamma, p, seed, with_gz_sum=True)

    x64, z64 = x.double().requires_grad_(), z.double().requires_grad_()
    g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    s64 = x64 + z64 * mask
    # normalised at the float32 sum the kernel saves (x = 100 + randn: its rounding moves xhat by ~4e-6), gradients exact
    s64 = s64 + ((x + z * mask.float()).double() - s64).detach()
    y64 = F.layer_norm(s64, (256,), g64, b64, EPS)
    y64.backward(gy.double())
    s64 = s64.detach()
    mean64 = s64.mean(-1, keepdim=True)
    rstd64 = ((s64 - mean64).square().mean(-1, keepdim=True) + EPS).rsqrt()
    _close(y, y64.detach(), "y")
    _close(mean, R.rows_in_memory(mean64, x).reshape(-1), "mean")
    _close(rstd, R.rows_in_memory(rstd64, x).reshape(-1), "rstd")
    _close(gx, x64.grad, "gx")
    _close(gz, z64.grad, "gz")
    gy64 = gy.double().reshape(-1, 256)
    # a float32 mean is resolved to ~1 ulp of |mean|, an offset every xhat of its row shares (rows at 100: 7.6e-6 * rstd)
    mean_ulp = (torch.finfo(torch.float32).eps * mean64.abs() * rstd64).reshape(-1, 1)
    _colsum_close(gg, g64.grad, gy64 * ((s64 - mean64) * rstd64).reshape(-1, 256), "ggamma",
                  (gy64.abs() * mean_ulp).sum(0).max().item())
    _colsum_close(gb, b64.grad, gy64, "gbeta")
    gz64 = z64.grad.reshape(-1, 256)
    _colsum_close(gzs, gz64.sum(0), gz64, "gz sum")
    if kind == "constant":
        assert torch.equal(y, beta.expand_as(y))
        assert all(torch.isfinite(t).all() for t in (gx, gz, gg, gb, gzs))


def test_public_dropout_add_layernorm_in_train_mode_matches_float64():
    torch.manual_seed(5)
    norm = torch.nn.LayerNorm(256).cuda()
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.uniform_(-0.5, 0.5)
    drop = torch.nn.Dropout(0.1).train()
    x = torch.randn(16, 550, 256, device="cuda", requires_grad=True)
    z = torch.randn(16, 550, 256, device="cuda", requires_grad=True)
    gy = torch.randn(16, 550, 256, device="cuda")
    with R.record() as draws:
        y = dropout_add_layernorm(x, z, norm, drop)
    assert "DropoutAddLayerNorm" in type(y.grad_fn).__name__ and [d.p for d in draws] == [0.1]
    y.backward(gy)
    mask = draws[0].mask().double()
    x64, z64 = x.detach().double().requires_grad_(), z.detach().double().requires_grad_()
    w64, b64 = norm.weight.detach().double().requires_grad_(), norm.bias.detach().double().requires_grad_()
    y64 = F.layer_norm(x64 + z64 * mask, (256,), w64, b64, norm.eps)
    y64.backward(gy.double())
    _close(y.detach(), y64.detach(), "y")
    _close(x.grad, x64.grad, "gx")
    _close(z.grad, z64.grad, "gz")
    _close(norm.weight.grad, w64.grad, "gweight")
    _close(norm.bias.grad, b64.grad, "gbias")


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows", [163200, 8800, 16385, 4097, 3, 1])
def test_relu_dropout_forward_and_backwards_match_float64(rows, p):
    """relu_dropout_forward / _backward / _backward_colsum against float64 relu(h) * mask; the two backward functions give
    bitwise-identical gh, and the fused column sum (d linear1.bias) matches a float64 sum."""
    g = torch.Generator(device="cuda").manual_seed(rows + int(p * 10))
    h = torch.randn(rows, 256, device="cuda", generator=g)
    gy = torch.randn(rows, 256, device="cuda", generator=g)
    with R.record() as draws:
        y = relu_dropout_forward(h, p)
    mask = draws[0].mask().double()
    pos = (h > 0).double()
    _close(y, h.double().clamp_min(0) * mask, "y")
    gh = relu_dropout_backward(gy, y, p)
    gh2, gsum = relu_dropout_backward_colsum(gy, y, p)
    assert torch.equal(gh, gh2)
    gh64 = gy.double() * mask * pos
    _close(gh, gh64, "gh")
    _colsum_close(gsum, gh64.sum(0), gh64, "gh column sum")


# ---- layers in train mode against PyTorch with the replayed masks ---------------------------------------------------------
LEVELS = [(24, 80), (12, 40), (6, 20), (3, 10)]


def _pyramid():
    from monosowa_amd import MultiScaleDeformableAttention as MSDA
    shapes = torch.tensor(LEVELS, dtype=torch.long, device="cuda")
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    starts = [0]
    for h, w in LEVELS[:-1]:
        starts.append(starts[-1] + h * w)
    MSDA.attach_host_geometry(shapes, lsi, LEVELS, starts)
    return shapes, lsi, sum(h * w for h, w in LEVELS)


ZERO_GRADIENTS = ("kcontent_proj.bias", "kpos_proj.bias")     # key biases shift every score of a query alike: d = 0 up to rounding


def _layer_close(got, ref, names):
    bad = []
    assert len(got) == len(ref) == len(names)
    for a, b, n in zip(got, ref, names):
        assert a is not None and b is not None, n
        a, b = a.double(), b.double()
        if n.endswith(ZERO_GRADIENTS):
            continue
        if n.endswith("in_proj_bias"):                          # the same for the key third of a packed projection
            a, b = torch.cat((a[:256], a[512:])), torch.cat((b[:256], b[512:]))
        err = (a - b).abs().max().item()
        bound = 3e-5 * max(b.abs().max().item(), 1e-3)
        if not err <= bound:
            bad.append("%s: max|err| %.3e > %.3e" % (n, err, bound))
    assert not bad, "; ".join(bad)


def _masks(draws, kinds):
    assert [d.kind for d in draws] == kinds, [d.kind for d in draws]
    return [d.mask() for d in draws]


@pytest.fixture
def deterministic():
    """torch's global flag on for the test, restored afterwards (warn_only included)."""
    was, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn_only)


def _ran_deterministic(value_like, shapes, lsi, Lq):
    """dropout > 0 together with the recomputing MSDA backward is what a deterministic training run executes"""
    from monosowa_amd import MultiScaleDeformableAttention as MSDA, _lib
    assert _lib.MSDA_DETERMINISTIC.sync() is True and pointwise.DETERMINISTIC.sync() is True
    assert not MSDA.fused_save_supported(value_like, shapes, lsi, Lq)


def test_visual_encoder_layer_blocks_in_train_mode_match_pytorch_with_the_replayed_masks():
    """The encoder's two autograd nodes (encoder_block) with dropout p against F.linear / F.layer_norm and the product's
    MSDA operator, dropout as a multiplication by the probed masks (attention LN, FFN ReLU-dropout, FFN LN): output, d src,
    d pos and every parameter gradient -- the fused bias sums of output_proj, linear2 and linear1 included."""
    _check_visual_encoder_layer_blocks(False)


def test_visual_encoder_layer_blocks_in_train_mode_match_pytorch_under_the_deterministic_flag(deterministic):
    """The same comparison, same bounds, under torch.use_deterministic_algorithms(True)."""
    _check_visual_encoder_layer_blocks(True)


def _check_visual_encoder_layer_blocks(det):
    from monosowa_amd.monodetr import depthaware_transformer as T
    torch.manual_seed(0)
    layer = T.VisualEncoderLayer(256, 256, 0.1, "relu", 4, 8, 4).cuda().train()
    shapes, lsi, S = _pyramid()
    B = 16
    src = torch.randn(B, S, 256, device="cuda", requires_grad=True)
    pos = torch.randn(B, S, 256, device="cuda", requires_grad=True)
    ref = torch.rand(B, S, 4, 2, device="cuda")
    go = torch.randn(B, S, 256, device="cuda")
    names, params = zip(*layer.named_parameters())
    if det:
        _ran_deterministic(torch.empty(B, S, 8, 32, device="cuda"), shapes, lsi, S)
    with R.record() as draws:
        y = layer(src, pos, ref, shapes, lsi, None)
    assert "FFNBlock" in type(y.grad_fn).__name__
    y.backward(go)
    ours = [y.detach().clone(), src.grad.clone(), pos.grad.clone()] + [p_.grad.clone() for p_ in params]
    assert [d.p for d in draws] == [0.1] * 3
    m_attn, _, m_ffn = _masks(draws, ["ln", "relu", "ln"])

    for t in (src, pos) + params:
        t.grad = None
    attn = layer.self_attn(src + pos, ref, src, shapes, lsi, None)
    n1, n2, l1, l2 = layer.norm1, layer.norm2, layer.linear1, layer.linear2
    s1 = F.layer_norm(src + attn * m_attn, (256,), n1.weight, n1.bias, n1.eps)
    hd = R.relu_dropout(F.linear(s1, l1.weight, l1.bias), draws[1])
    want = F.layer_norm(s1 + F.linear(hd, l2.weight, l2.bias) * m_ffn, (256,), n2.weight, n2.bias, n2.eps)
    want.backward(go)
    _layer_close(ours, [want.detach(), src.grad, pos.grad] + [p_.grad for p_ in params], ["y", "d src", "d pos"] + list(names))
    for d in (layer.dropout1, layer.dropout2, layer.dropout3):
        d.p = 0.0
    y0 = layer(src, pos, ref, shapes, lsi, None)
    assert "FFNBlock" in type(y0.grad_fn).__name__
    assert (y0 - y).abs().max().item() > 1e-2


def test_depth_aware_decoder_layer_in_train_mode_matches_pytorch_with_the_replayed_masks():
    """DepthAwareDecoderLayer (dropout 0.1, attention dropout off) at B = 16, 550 queries: its four fused LayerNorm dropouts and
    its ReLU-dropout against the same layer with F.layer_norm(x + z * mask) / relu(h) * mask in their place."""
    _check_depth_aware_decoder_layer(False)


def test_depth_aware_decoder_layer_in_train_mode_matches_pytorch_under_the_deterministic_flag(deterministic):
    """The same comparison, same bounds, under torch.use_deterministic_algorithms(True)."""
    _check_depth_aware_decoder_layer(True)


def _check_depth_aware_decoder_layer(det):
    from monosowa_amd.monodetr import depthaware_transformer as T
    torch.manual_seed(1)
    layer = T.DepthAwareDecoderLayer(256, 256, 0.1, "relu", 4, 8, 4, group_num=11, group_size=50).cuda().train()
    layer.cross_attn_depth.dropout = layer.self_attn.dropout = 0.0
    shapes, lsi, S = _pyramid()
    B, Q = 16, 550
    tgt = torch.randn(B, Q, 256, device="cuda", requires_grad=True)
    qpos = torch.randn(B, Q, 256, device="cuda", requires_grad=True)
    memory = torch.randn(B, S, 256, device="cuda", requires_grad=True)
    dpe = torch.randn(1920, B, 256, device="cuda", requires_grad=True)
    refp = torch.rand(B, Q, 4, 2, device="cuda")
    go = torch.randn(B, Q, 256, device="cuda")
    names, params = zip(*[(n, p_) for n, p_ in layer.named_parameters()])
    leaves = (tgt, qpos, memory, dpe) + params
    if det:
        _ran_deterministic(torch.empty(B, S, 8, 32, device="cuda"), shapes, lsi, Q)

    def run():
        for t in leaves:
            t.grad = None
        y = layer(tgt, qpos, refp, memory, shapes, lsi, None, dpe, None)
        y.backward(go)
        return [y.detach().clone()] + [None if t.grad is None else t.grad.clone() for t in leaves]
    with R.record() as draws:
        ours = run()
    _masks(draws, ["ln", "ln", "ln", "relu", "ln"])
    assert [d.p for d in draws] == [0.1] * 5
    masks = iter(draws)

    def ref_ln(x, z, norm, dropout):
        return F.layer_norm(x + z * next(masks).mask(), norm.normalized_shape, norm.weight, norm.bias, norm.eps)

    def ref_relu(h, dropout):
        return R.relu_dropout(h, next(masks))
    saved = T.dropout_add_layernorm, T.relu_dropout
    T.dropout_add_layernorm, T.relu_dropout = ref_ln, ref_relu
    try:
        want = run()
    finally:
        T.dropout_add_layernorm, T.relu_dropout = saved
    assert next(masks, None) is None
    keep = [i for i, w in enumerate(want) if w is not None]          # (sa_v_proj and the unused projections have no gradient)
    assert len(keep) > 20
    _layer_close([ours[i] for i in keep], [want[i] for i in keep],
                 [(["y", "d tgt", "d query_pos", "d memory", "d depth_pos_embed"] + list(names))[i] for i in keep])


def test_depth_encoder_layer_in_train_mode_matches_float64_with_the_replayed_masks():
    """DepthEncoderLayer (dropout 0.1, attention dropout off) at [1920, 16, 256] given as the [L, B, C] view of a batch-major
    buffer, against a float64 evaluation with the probed masks: output, d src, d pos and every parameter gradient."""
    from monosowa_amd.monodetr.depth_predictor import DepthEncoderLayer
    torch.manual_seed(2)
    layer = DepthEncoderLayer(256, 8, 256, 0.1).cuda().train()
    layer.self_attn.dropout = 0.0
    B, L = 16, 1920
    src_b = torch.randn(B, L, 256, device="cuda", requires_grad=True)
    pos_b = torch.randn(B, L, 256, device="cuda", requires_grad=True)
    go = torch.randn(L, B, 256, device="cuda")
    names, params = zip(*layer.named_parameters())
    with R.record() as draws:
        y = layer(src_b.transpose(0, 1), None, pos_b.transpose(0, 1))
    y.backward(go)
    ours = [y.detach(), src_b.grad, pos_b.grad] + [p_.grad for p_ in params]
    m1, _, m3 = (m.double() for m in _masks(draws, ["ln", "relu", "ln"]))
    assert [d.p for d in draws] == [0.1] * 3
    assert draws[0].desc[1] == src_b.transpose(0, 1).stride()            # the LayerNorm walked the [L, B, C] view in place

    P = {n: p_.detach().double().requires_grad_() for n, p_ in layer.named_parameters()}
    s64, p64 = src_b.detach().double().requires_grad_(), pos_b.detach().double().requires_grad_()
    src, pos = s64.transpose(0, 1), p64.transpose(0, 1)
    qk = src + pos
    attn = F.multi_head_attention_forward(qk, qk, src, 256, 8, P["self_attn.in_proj_weight"], P["self_attn.in_proj_bias"],
                                          None, None, False, 0.0, P["self_attn.out_proj.weight"], P["self_attn.out_proj.bias"],
                                          training=True, need_weights=False)[0]
    s1 = F.layer_norm(src + attn * m1, (256,), P["norm1.weight"], P["norm1.bias"], layer.norm1.eps)
    hd = R.relu_dropout(F.linear(s1, P["linear1.weight"], P["linear1.bias"]), draws[1])
    want = F.layer_norm(s1 + F.linear(hd, P["linear2.weight"], P["linear2.bias"]) * m3, (256,), P["norm2.weight"],
                        P["norm2.bias"], layer.norm2.eps)
    want.backward(go.double())
    _layer_close(ours, [want.detach(), s64.grad, p64.grad] + [P[n].grad for n in names], ["y", "d src", "d pos"] + list(names))
