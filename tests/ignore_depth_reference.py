"""Ignore regions in the depth-map loss (``model.ignore_depth_map``): an independent restatement, importing nothing from ``monosowa_amd``.

* ``covered``: the coverage rule in numpy float32, box by box: pixel (y, x) lies under a valid ignore box g (x1, y1, x2, y2 in depth-map
  pixels) when x >= floor(g.x1), x < ceil(g.x2), y >= floor(g.y1) and y < ceil(g.y2), each comparison on float32 values -- a NaN
  coordinate makes every comparison false, nothing is converted to an integer, and a negative start does NOT wrap the way the slice of
  a target box does.  ``ignored_mask``: covered and not foreground (foreground wins).
* ``depth_map_loss``: ``label_weights_reference.depth_map_loss`` with the ignored-pixel mask: the ignored pixels' logits are replaced by
  a constant before anything is computed from them (a non-finite one reaches nothing, their gradient is exactly zero) and their factor
  is 0; the divisor stays B H W.  Dtype-agnostic torch with autograd.
* ``rel`` / ``row_error``: the error measures of tests/test_label_weights_gpu.py, restated.
* ``make_case``: B = 3, C = 81, H x W = 5 x 7 (105 pixels, 840 lanes, a last block of dead lanes) or 24 x 80 (the training map), N = 3
  target slots, M in {1, 3, 50} ignore slots.  Each case asserts, on the CPU, the properties it names in ``case["holds"]``;
  ``ALL_PROPERTIES`` is what the cases of one map size hold together (``assert_family``).
"""
import numpy as np
import torch

import criterion_reference as CR
import label_weights_reference as LW

SIZES = ((5, 7), (24, 80))
MS = (1, 3, 50)
BLOCK_PIXELS = 32          # pixels of one 256-thread block at eight lanes per pixel
ALL_PROPERTIES = ("fractional", "integral_edge", "ulp_wider", "negative_start", "foreground_wins", "nan", "invalid_slot", "no_valid_box",
                  "whole_map", "last_pixel_ignored", "last_pixel_kept")
TINY = 1e-30


def rel(x, ref):
    return abs(float(x) - float(ref)) / max(abs(float(ref)), TINY)


def row_error(g, ref):
    """max over rows (the last dimension) of ||g_row - ref_row|| / max(||ref_row||, 1e-4 * the largest ||ref_row||)"""
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    g, ref = g.reshape(-1, g.shape[-1]), ref.reshape(-1, ref.shape[-1])
    norms = ref.norm(dim=1)
    floor = 1e-4 * float(norms.max())
    assert floor > 0
    return float(((g - ref).norm(dim=1) / norms.clamp_min(floor)).max())


def covered(ign_boxes, ign_valid, H, W):
    """bool [B, H, W]: the pixels under a valid ignore box; ign_boxes [B, M, 4] in depth-map pixels (taken as float32)"""
    g = np.asarray(ign_boxes, dtype=np.float32)
    m = np.asarray(ign_valid).astype(bool)
    B, M = m.shape
    xs = np.arange(W, dtype=np.float32)[None, :]
    ys = np.arange(H, dtype=np.float32)[:, None]
    out = np.zeros((B, H, W), dtype=bool)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            for j in range(M):
                if not m[b, j]:
                    continue
                x1, y1, x2, y2 = g[b, j]
                out[b] |= (xs >= np.floor(x1)) & (xs < np.ceil(x2)) & (ys >= np.floor(y1)) & (ys < np.ceil(y2))
    return out


def ignored_mask(ign_boxes, ign_valid, fg):
    """bool tensor [B, H, W]: covered by a valid ignore box and not foreground"""
    fg = fg.cpu()
    B, H, W = fg.shape
    return torch.from_numpy(covered(ign_boxes, ign_valid, H, W)) & ~fg


def block_counts(ign):
    """int64 [blocks]: ignored pixels per BLOCK_PIXELS consecutive pixels in (b, y, x) order"""
    flat = ign.reshape(-1).to(torch.int64)
    blocks = (flat.numel() + BLOCK_PIXELS - 1) // BLOCK_PIXELS
    pad = torch.zeros(blocks * BLOCK_PIXELS, dtype=torch.int64)
    pad[:flat.numel()] = flat
    return pad.view(blocks, BLOCK_PIXELS).sum(1)


def depth_map_loss(logits, boxes, depth, valid, weight, ign_boxes, ign_valid, alpha=0.25, gamma=2.0, fg_weight=13.0, bg_weight=1.0,
                   depth_min=1e-3, depth_max=60.0, eps=1e-6):
    """-> (loss, (bins, fg, wmap, ignored)).  ``weight`` None: all ones.  ign_boxes: float32 values in depth-map pixels."""
    B, C, H, W = logits.shape
    num_bins = C - 1
    if weight is None:
        weight = torch.ones_like(depth)
    d, fg, wmap = LW.depth_map_targets(boxes, depth, valid, weight, H, W)
    ign = ignored_mask(np.asarray(ign_boxes.detach().cpu().numpy(), dtype=np.float32), ign_valid.cpu().numpy(), fg)
    d, fg, wmap, ign_d = d.to(logits.device), fg.to(logits.device), wmap.to(device=logits.device, dtype=logits.dtype), ign.to(logits.device)
    x = torch.where(ign_d.unsqueeze(1), torch.zeros((), dtype=logits.dtype, device=logits.device), logits)      # before anything else
    bin_size = 2 * (depth_max - depth_min) / (num_bins * (1 + num_bins))
    pos = -0.5 + 0.5 * torch.sqrt(1 + 8 * (d.double() - depth_min) / bin_size)
    bad = (pos < 0) | (pos > num_bins) | ~torch.isfinite(pos)
    bins = torch.where(bad, torch.full_like(pos, num_bins), pos).long()
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    one = (bins.unsqueeze(1) == torch.arange(C, device=logits.device).view(1, C, 1, 1)).to(logits.dtype)
    pixel = ((one + eps) * (-alpha * (1 - p) ** gamma * logp)).sum(1)
    factor = torch.where(fg, fg_weight * wmap, torch.full_like(wmap, bg_weight))
    factor = torch.where(ign_d, torch.zeros_like(factor), factor)
    return (pixel * factor).sum() / (B * H * W), (bins, fg, wmap, ign_d)


# ------------------------------------------------------------------------------------------------------------------ cases
def make_case(H, W, M, seed=0):
    """-> dict(logits [3, 81, H, W], boxes [3, 3, 4], depth, valid, weight [3, 3], ign_boxes [3, M, 4] float32, ign_valid [3, M] bool,
    ignored bool [3, H, W], fg, holds: the names of ALL_PROPERTIES this case was checked to hold).  Boxes are xyxy in map pixels."""
    assert (H, W) in SIZES and M in MS
    f = np.float32
    nan = float("nan")
    boxes = torch.zeros(3, 3, 4)
    depth, weight = torch.zeros(3, 3), torch.ones(3, 3)
    valid = torch.zeros(3, 3, dtype=torch.bool)
    t_img0 = [((0.30 * W, 0.25 * H, 0.70 * W, 0.75 * H), 30.0, 1.0),      # trusted
              ((0.50 * W, 0.40 * H, 0.90 * W, 0.60 * H), 12.0, 0.0),      # weight 0, nearer, partly over the trusted box
              ((-3.5, 0.0, 2.0, 2.0), 17.0, 1.5)]                         # start -4 counts from the end: an empty slice
    for i, (b, d, w) in enumerate(t_img0):
        boxes[0, i], depth[0, i], weight[0, i], valid[0, i] = torch.tensor(b), d, w, True
    boxes[2, 0], depth[2, 0], weight[2, 0], valid[2, 0] = torch.tensor((0.1 * W, 0.1 * H, 0.3 * W, 0.3 * H)), 47.25, 0.75, True
    depth = torch.from_numpy(CR._off_bin_edges(depth.double().numpy()).astype(np.float32))

    g_fg = (0.55 * W + 0.3, 0.3 * H + 0.2, 0.95 * W + 0.4, 0.7 * H + 0.1)        # fractional corners, partly under both target boxes
    g_neg = (-3.5, 0.0, 2.0, 2.0)                                                # the empty target box's coordinates: columns 0 and 1
    g_edge = (0.0, H - 1.0, 1.0, float(H))                                       # right edge exactly 1: column 1 is out
    g_ulp = (0.0, H - 2.0, float(np.nextafter(f(1.0), f(2.0))), H - 1.0)         # one float32 ulp wider: column 1 is in
    g_nan = (nan, 0.0, float(W), float(H))
    g_all = (0.0, 0.0, float(W), float(H))
    g_lastrow = (-0.5, H - 1.0, W - 1.0, H + 2.0)                                # the last row but its last pixel
    g_rows = (0.0, H - 4.5, W + 3.0, H - 2.25)                                   # rows H-5 .. H-3, every column
    g_late = (0.6 * W + 0.2, 0.1 * H, 0.8 * W + 0.3, 0.3 * H + 0.1)
    plan = {1: [[(g_fg, True)], [(g_all, False)], [(g_all, True)]],
            3: [[(g_fg, True), (g_neg, True), (g_edge, True)], [(g_ulp, True), (g_nan, True), (g_all, False)],
                [(g_lastrow, True), (g_rows, True), (g_nan, True)]],
            50: [[(g_fg, True), (g_neg, True), (g_edge, True), (g_ulp, True), (g_nan, True), (g_all, False)], [(g_all, False)],
                 [(g_lastrow, True), (g_rows, True)]]}[M]
    rng = np.random.default_rng(1000 + seed + M)
    ign = np.zeros((3, M, 4), dtype=np.float32)
    ign_valid = np.zeros((3, M), dtype=bool)
    lo = rng.uniform(0, 0.6, (3, M, 2)) * (W, H)
    ign[..., :2], ign[..., 2:] = lo, lo + rng.uniform(0.1, 0.4, (3, M, 2)) * (W, H)       # invalid filler: boxes that would cover pixels
    for b in range(3):
        for j, (g, ok) in enumerate(plan[b]):
            ign[b, j], ign_valid[b, j] = np.asarray(g, dtype=np.float32), ok
    if M == 50:
        ign[2, 49], ign_valid[2, 49] = np.asarray(g_late, dtype=np.float32), True          # the loop reaches the last slot
    logits = torch.randn(3, 81, H, W, generator=torch.Generator().manual_seed(177 + seed)) * 2
    _, fg, wmap = LW.depth_map_targets(boxes, depth, valid, weight, H, W)
    cov = torch.from_numpy(covered(ign, ign_valid, H, W))
    ignored = cov & ~fg
    assert torch.equal(ignored, ignored_mask(ign, ign_valid, fg))

    holds = set()
    only = lambda g, b: torch.from_numpy(covered(np.asarray(g, np.float32).reshape(1, 1, 4), np.ones((1, 1), bool), H, W))[0]
    has = lambda b, g: any(ok and gg is g for gg, ok in plan[b])
    if has(0, g_fg):
        c = only(g_fg, 0)
        assert any(v != int(v) for v in g_fg) and c.any()
        holds.add("fractional")
        under_zero = c & fg[0] & (wmap[0] == 0)
        under_trusted = c & fg[0] & (wmap[0] == 1)
        assert under_zero.any() and under_trusted.any() and (c & ~fg[0]).any() and not (ignored[0] & fg[0]).any()
        holds.add("foreground_wins")
    if has(0, g_neg):
        c = only(g_neg, 0)
        assert c[:2, :2].all() and c.sum() == 4 and ignored[0, 0, 0] and ignored[0, 1, 1]
        assert tuple(boxes[0, 2].tolist()) == g_neg and not fg[0, :2, :2].any()          # the target box with these coordinates is empty
        holds.add("negative_start")
    for b in range(3):
        if has(b, g_edge):
            assert ignored[b, H - 1, 0] and not cov[b, H - 1, 1]
            holds.add("integral_edge")
        if has(b, g_ulp):
            assert g_ulp[2] > 1.0 and f(g_ulp[2]) == np.nextafter(f(1.0), f(2.0)) and ignored[b, H - 2, 0] and ignored[b, H - 2, 1]
            assert not cov[b, H - 2, 2]
            holds.add("ulp_wider")
        if has(b, g_nan):
            assert not only(g_nan, b).any()
            holds.add("nan")
        if any((not ok) and gg is g_all for gg, ok in plan[b]):
            assert only(g_all, b).all() and not cov[b].all()
            holds.add("invalid_slot")
        if not ign_valid[b].any():
            assert not ignored[b].any()
            holds.add("no_valid_box")
        if has(b, g_all):
            assert cov[b].all() and torch.equal(ignored[b], ~fg[b])
            holds.add("whole_map")
    if ignored[2, H - 1, W - 1]:
        holds.add("last_pixel_ignored")
    if not ignored[2, H - 1, W - 1] and ignored[2, H - 1, W - 2]:
        holds.add("last_pixel_kept")
    assert holds & {"last_pixel_ignored", "last_pixel_kept"}
    assert (ignored.reshape(3, -1).any(1) == torch.tensor([True, M == 3, True])).all()
    if (H, W) == (24, 80):
        per_block = block_counts(ignored)
        assert int(ignored.sum()) >= 100 and (per_block == 0).any() and (per_block == BLOCK_PIXELS).any()
    return {"logits": logits, "boxes": boxes, "depth": depth, "valid": valid, "weight": weight, "ign_boxes": torch.from_numpy(ign),
            "ign_valid": torch.from_numpy(ign_valid), "ignored": ignored, "fg": fg, "wmap": wmap, "holds": holds}


_CASES = {}


def case(H, W, M):
    """``make_case`` once per (H, W, M); the tensors are shared and must not be modified"""
    key = (H, W, M)
    if key not in _CASES:
        _CASES[key] = make_case(H, W, M)
    return _CASES[key]


def assert_family(H, W):
    """the cases of one map size hold every property together"""
    held = set().union(*[case(H, W, M)["holds"] for M in MS])
    assert held == set(ALL_PROPERTIES), set(ALL_PROPERTIES) - held
