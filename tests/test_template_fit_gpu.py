"""Template fitting on the GPU: the kernels of libmonosowa_fit.so against the restatement of tests/fit_reference.py bit for bit, the
edge families, a planted pose against the float64 oracle, nothing written outside the outputs, the same bytes wherever the buffers
lie, every return code, the fallback beyond the limits, and no host synchronisation."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fit_reference as R

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _fitter(tmpl, grid=R.GRID, **loss):
    from monosowa_amd import TemplateFitter
    return TemplateFitter(tmpl, {"optimization": grid, "loss_functions": dict(R.CFG["loss_functions"], **loss)}, device=_dev())


@functools.lru_cache(maxsize=None)
def _batch(T):
    """The generator's batch and what the restatement makes of it, computed once."""
    tmpl, clouds, centres = R.batch(T)
    dx, dz, th = np.linspace(-2, 2, 6), np.linspace(-1, 3, 6), R.angles(12)
    ab = [R.search_f32(tmpl, c, centres[o], dx, dz, th)[4] if len(c) else np.zeros((432, 2), dtype=np.int64) for o, c in enumerate(clouds)]
    return tmpl, clouds, centres, R.fit_f32(tmpl, clouds, centres), np.stack(ab)


def _carve(spec, shift_bytes):
    """Every array of ``spec`` (name, dtype, shape) as a view into one buffer of sentinel bytes, 40 of them in front of each, each
    start a multiple of 16 plus ``shift_bytes`` -> (buffer, views, bool mask of the bytes that belong to an array)."""
    cursor, places = 0, []
    for name, dtype, shape in spec:
        item = torch.empty((), dtype=dtype).element_size()
        start = (cursor + 40 + 15) // 16 * 16 + shift_bytes
        nbytes = int(np.prod(shape)) * item
        places.append((name, dtype, shape, start, nbytes))
        cursor = start + nbytes
    buf = torch.full((cursor + 64,), SENTINEL, dtype=torch.uint8, device=_dev())
    inside, views = np.zeros(cursor + 64, dtype=bool), {}
    for name, dtype, shape, start, nbytes in places:
        views[name] = buf[start:start + nbytes].view(dtype).view(shape)
        inside[start:start + nbytes] = True
    return buf, views, inside


def _abi_fit(fitter, clouds, centres, dx, dz, theta, shift=None, fine=True):
    """The three entry points called directly on one group: coarse search and reduce, then the 360-angle fine stage through ``fix``.
    ``shift``: the outputs carved out of sentinel bytes at that byte offset.  -> (numpy copies of the outputs, buffer, inside)"""
    from monosowa_amd import template_fit as F
    lib, c = F.load(), fitter.config
    B, Nmax = len(clouds), max([len(p) for p in clouds] + [1])
    padded = np.zeros((B, Nmax, 3), dtype=np.float32)
    for o, p in enumerate(clouds):
        padded[o, :len(p)] = p
    pts, cnt = _t(padded), _t(np.array([len(p) for p in clouds], dtype=np.int32))
    I, J, K = len(dx), len(dz), len(theta)
    lists = [R.host_lists(centres[o], dx, dz, theta) for o in range(B)]
    tx, ty, tz = (_t(np.array([l[n] for l in lists], dtype=np.float32)) for n in range(3))
    cs = _t(np.array([np.stack([l[3], l[4]], axis=1) for l in lists], dtype=np.float32))
    fine_th = R.angles(360)
    cs_fine = _t(np.tile(np.stack([np.cos(fine_th), np.sin(fine_th)], axis=1).astype(np.float32), (B, 1, 1)))
    tmpl, tstart = fitter._template_on_device()
    T = fitter.template.shape[0]
    spec = [("grid", torch.int32, (B, 10)), ("sorted", torch.float32, (B, Nmax, 4)), ("start", torch.int32, (B, F.MAX_CELLS + 1)),
            ("cell", torch.int32, (B, Nmax)), ("scell", torch.int32, (B, Nmax)), ("ab", torch.int32, (B, I * J * K, 2)),
            ("result", torch.int32, (B, F.RESULT_INTS)), ("loss", torch.float64, (B,)), ("ab_fine", torch.int32, (B, 360, 2)),
            ("result_fine", torch.int32, (B, F.RESULT_INTS)), ("loss_fine", torch.float64, (B,))]
    buf, v, inside = _carve(spec, 0 if shift is None else shift)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    codes = [lib.mono_fit_grid_f32(p(pts), p(cnt), B, Nmax, c.r, p(v["grid"]), p(v["sorted"]), p(v["start"]), p(v["cell"]), p(v["scell"]),
                                   stream)]
    for cs_, K_, fix, names in ((cs, K, None, ("ab", "result", "loss")), (cs_fine, 360, p(v["result"]), ("ab_fine", "result_fine", "loss_fine"))):
        if fix is not None and not fine:
            break
        ab, res, loss = (v[n] for n in names)
        codes.append(lib.mono_fit_search_f32(p(tmpl), p(tstart), ctypes.byref(fitter.grid), T, p(v["grid"]), p(v["sorted"]), p(v["start"]),
                                             p(cnt), B, Nmax, p(tx), p(ty), p(tz), p(cs_), I, J, K_, fix, c.r, p(ab), stream))
        codes.append(lib.mono_fit_reduce_f64(p(ab), p(cnt), B, Nmax, T, I, J, K_, fix, int(c.one_way), p(res), p(loss), stream))
    torch.cuda.synchronize()
    assert codes == [0] * len(codes), codes
    return {k: t.cpu().numpy() for k, t in v.items()}, buf.cpu().numpy(), inside


# ================================================================================================ 1. the kernels
@pytest.mark.parametrize("T", [96, 65])
def test_kernels_equal_the_restatement_bit_for_bit(T):
    tmpl, clouds, centres, want, want_ab = _batch(T)
    fitter = _fitter(tmpl)
    result = fitter.fit(clouds, centres)
    assert not result.host and result.x.is_cuda
    R.assert_same(result.numpy(), want, T)
    # every placement's two counts, not only the winner's
    out, _, _ = _abi_fit(fitter, clouds, centres, np.linspace(-2, 2, 6), np.linspace(-1, 3, 6), R.angles(12))
    assert np.array_equal(out["ab"], want_ab)
    assert np.array_equal(out["result"][:, 0], want["h_coarse"]) and np.array_equal(out["result_fine"][:, 0], want["h_fine"])
    assert np.array_equal(R.bits(out["loss_fine"]), R.bits(want["loss"]))
    # a padded tensor with counts, the centres left to the device's median
    width = max(len(c) for c in clouds)
    padded = np.full((len(clouds), width + 3, 3), 7.5, dtype=np.float32)
    for o, c in enumerate(clouds):
        padded[o, :len(c)] = c
    counts = torch.tensor([len(c) for c in clouds], dtype=torch.int32)
    got = fitter.fit((_t(padded), counts.to(_dev()))).numpy()
    R.assert_same(got, R.fit_f32(tmpl, clouds), "median")


# ================================================================================================ 2. the edge families
def _edge_cases():
    tmpl, clouds, centres = R.batch(65)
    scan, centre = clouds[1], centres[1]
    bad_scan = scan.copy()
    bad_scan[3, 0], bad_scan[40, 2], bad_scan[77] = np.nan, np.inf, (-np.inf, np.nan, 1.0)
    bad_tmpl = tmpl.copy()
    bad_tmpl[2, 1], bad_tmpl[30, 0], bad_tmpl[64, 2] = np.nan, np.inf, -np.inf
    # nodes 10 m apart, one of them the centre itself: every other placement has the whole template outside the scan's index
    wide = dict(R.GRID, opt_param1_min=-30.0, opt_param1_max=30.0, opt_param1_iters=7, opt_param2_min=-40.0, opt_param2_max=40.0,
                opt_param2_iters=9)
    far = (scan.astype(np.float64) + 500.0).astype(np.float32)
    cluster = (np.asarray(centre) + np.tile(tmpl[:4].astype(np.float64), (10, 1))
               + 0.01 * np.random.default_rng(5).standard_normal((40, 3))).astype(np.float32)
    yield "NaN and Inf in the scan", tmpl, [bad_scan], [centre], {}
    yield "NaN and Inf in the template", bad_tmpl, [scan], [centre], {}
    yield "NaN and Inf in both", bad_tmpl, [bad_scan], [centre], {}
    yield "a scan of non-finite points only", tmpl, [np.full((5, 3), np.nan, dtype=np.float32)], [centre], {}
    yield "all scan points identical", tmpl, [np.tile(scan[:1], (50, 1))], [centre], {}
    yield "duplicated points", np.concatenate([tmpl, tmpl[:20]]), [np.concatenate([scan, scan])], [centre], {}
    yield "T = 1", tmpl[:1], [scan], [centre], {}
    yield "a scan nowhere near", tmpl, [far], [centre], {}
    yield "placements outside the index", tmpl, [cluster, scan], [centre, centre], {"grid": wide}
    yield "moving with and without theta", tmpl, clouds, centres, {"moving": [True, True, False, True, False],
                                                                    "theta": [None, 0.4, None, 2.0, None]}
    yield "loc_only", tmpl, clouds[:2], centres[:2], {"loc_only": [True, False], "theta": [1.1, None]}
    yield "binary1way", tmpl, clouds, centres, {"one_way": True, "moving": [False, True, False, False, False]}


@pytest.mark.parametrize("case", list(_edge_cases()), ids=lambda c: c[0])
def test_edge_families(case):
    name, tmpl, clouds, centres, kw = case
    grid, one_way = kw.get("grid", R.GRID), kw.get("one_way", False)
    modes = {k: kw.get(k) for k in ("moving", "theta", "loc_only")}
    fitter = _fitter(tmpl, grid, loss_function="binary1way" if one_way else "binary2way")
    centres = np.asarray(centres, dtype=np.float64)
    result = fitter.fit(clouds, centres, **modes)
    assert not result.host
    got, want = result.numpy(), R.fit_f32(tmpl, clouds, centres, grid=grid, one_way=one_way, **modes)
    print(name, {k: got[k].tolist() for k in ("a", "b", "h_coarse", "h_fine", "loss")})
    R.assert_same(got, want, name)
    if name in ("a scan nowhere near", "a scan of non-finite points only"):
        assert got["loss"].tolist() == [0.0] and got["h_coarse"].tolist() == [0] and got["h_fine"].tolist() == [0]
        assert got["status"].tolist() == [0] and got["theta"].tolist() == [0.0] and got["x"][0] == centres[0][0] - 2.0
    if name == "placements outside the index":
        assert got["a"][0] >= 4 and got["b"][0] == 40 and got["x"][0] == centres[0][0] and got["z"][0] == centres[0][2]


# ================================================================================================ 3. a planted pose
def test_planted_pose_against_the_float64_oracle():
    """A 1,000-point template copied exactly onto node (5, 3, 6) of a 9 x 9 x 8 grid, plus 1,000 points 100 m away.  At the node
    L = -(1 + 1000 / 2000), the smallest value any placement can reach (the far points are out of every placement's reach), and a
    neighbouring node is 0.5 m or 45 degrees off, so no earlier placement ties.  The oracle runs on the 3 x 3 x 8 block around the
    node: the whole grid would take it 13 s.  With two million pairs per placement most placements have some pair near the
    threshold, so the margin here is the float32 contract's own error and no share of excluded placements is asked: coordinates
    near 40 m carry ulp / 2 = 1.9e-6 m per rounding, four roundings per axis give 8e-6 m, and at d = r = 0.2 m that moves d^2 by
    2 * 0.2 * sqrt(3) * 8e-6 = 5.5e-6 = 1.4e-4 r^2; 2.5e-4 r^2 is taken.  The node itself needs no margin: every point has a
    partner at distance zero."""
    T, node = 1000, (5, 3, 6)
    grid = dict(R.GRID, opt_param1_iters=9, opt_param2_iters=9, opt_param3_iters=8)
    tmpl = R.box_template(T, 21)
    centre = np.array([8.0, 1.6, 40.0])
    dx, dz, th = np.linspace(-2, 2, 9), np.linspace(-1, 3, 9), R.angles(8)
    f = np.float32
    tx, ty, tz = f(dx[node[0]] + centre[0]), f(centre[1]), f(dz[node[1]] + centre[2])
    c, s = f(np.cos(th[node[2]])), f(np.sin(th[node[2]]))
    planted = np.stack([(c * tmpl[:, 0] + s * tmpl[:, 2]) + tx, tmpl[:, 1] + ty, (c * tmpl[:, 2] - s * tmpl[:, 0]) + tz], axis=1)
    scan = np.concatenate([planted, planted + f(100.0)]).astype(np.float32)
    fitter = _fitter(tmpl, grid)
    got = fitter.fit([scan], centre[None]).numpy()
    h = (node[0] * 9 + node[1]) * 8 + node[2]
    assert got["h_coarse"].tolist() == [h] and got["x"][0] == dx[node[0]] + centre[0] and got["z"][0] == dz[node[1]] + centre[2]
    out, _, _ = _abi_fit(fitter, [scan], centre[None], dx, dz, th, fine=False)
    assert out["ab"][0, h].tolist() == [T, 1000] and out["loss"].tolist() == [-1.5] and out["result"][0, :4].tolist() == [h, T, 1000, 0]
    assert (got["a"][0], got["b"][0], got["loss"][0], got["score"][0]) == (T, 1000, -1.5, 0.75)      # the fine stage finds it again
    # the node's own angle is one of the 360 and reaches the same loss, so the first minimum lies at or before it; the oracle
    # counts the same at the angle found
    fine = R.angles(360)
    assert got["theta"][0] == fine[got["h_fine"][0]] and got["theta"][0] <= th[node[2]] == fine[270]
    _, L_fine, ab_fine, near_fine = R.search_f64(tmpl, scan, centre, dx[node[0]:node[0] + 1], dz[node[1]:node[1] + 1], [got["theta"][0]])
    assert near_fine[0] or (ab_fine[0].tolist() == [T, 1000] and L_fine == -1.5)
    block_i, block_j = slice(node[0] - 1, node[0] + 2), slice(node[1] - 1, node[1] + 2)
    h64, L64, ab64, near = R.search_f64(tmpl, scan, centre, dx[block_i], dz[block_j], th, margin=2.5e-4)
    mine = out["ab"][0].reshape(9, 9, 8, 2)[block_i, block_j].reshape(-1, 2)
    print("oracle block: %d of %d placements within the margin, %d counts differ" % (near.sum(), len(near), (mine != ab64).sum()))
    assert h64 == (1 * 3 + 1) * 8 + node[2] and L64 == -1.5 and mine[h64].tolist() == ab64[h64].tolist() == [T, 1000]
    assert np.array_equal(mine[~near], ab64[~near]) and (~near).sum() >= len(near) // 2


# ================================================================================================ 4 / 5. the outputs and nothing else
def test_nothing_outside_the_outputs_and_the_same_bytes_at_other_addresses():
    tmpl, clouds, centres, want, want_ab = _batch(65)
    fitter = _fitter(tmpl)
    dx, dz, th = np.linspace(-2, 2, 6), np.linspace(-1, 3, 6), R.angles(12)
    runs = []
    for shift in (0, 48):                                     # `sorted` stays 16-byte aligned, as the header asks
        out, buf, inside = _abi_fit(fitter, clouds, centres, dx, dz, th, shift=shift)
        assert (buf[~inside] == SENTINEL).all(), shift
        assert np.array_equal(out["ab"], want_ab) and np.array_equal(out["result_fine"][:, 0], want["h_fine"]), shift
        runs.append(out)
    first, second = runs
    counts = [len(c) for c in clouds]
    for k in ("grid", "ab", "result", "loss", "ab_fine", "result_fine", "loss_fine"):
        assert first[k].tobytes() == second[k].tobytes(), k
    for o, n in enumerate(counts):                             # what the contract says is written: rows below count, cells up to ncell
        cells = int(first["grid"][o, 9])
        assert first["sorted"][o, :n].tobytes() == second["sorted"][o, :n].tobytes(), o
        assert first["start"][o, :cells + 1].tobytes() == second["start"][o, :cells + 1].tobytes(), o
        assert sorted(map(tuple, first["sorted"][o, :n, :3].tolist())) == sorted(map(tuple, clouds[o].tolist()))
        assert first["start"][o, 0] == 0 and first["start"][o, cells] == n and (np.diff(first["start"][o, :cells + 1]) >= 0).all()
        # rows at and beyond count[o], cells beyond ncell: untouched
        assert (first["sorted"][o, n:].view(np.uint8) == SENTINEL).all() and (first["start"][o, cells + 1:].view(np.uint8) == SENTINEL).all()
    # two fits through the public call, whose buffers the allocator places: the same bytes again
    hold = torch.empty(12345, device=_dev())
    a, b = fitter.fit(clouds, centres).numpy(), fitter.fit(clouds, centres).numpy()
    del hold
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


# ================================================================================================ 6. return codes
def test_every_return_code():
    from monosowa_amd import template_fit as F
    lib, dev = F.load(), _dev()
    assert lib.mono_fit_abi_version() == F.ABI_VERSION
    tmpl = R.box_template(8, 1)
    fitter = _fitter(tmpl)
    B, N, I, J, K = 2, 5, 2, 3, 4
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    pts, cnt = z((B, N, 3), torch.float32), z((B,), torch.int32)
    grid, srt, start = z((B, 10), torch.int32), z((B, N, 4), torch.float32), z((B, F.MAX_CELLS + 1), torch.int32)
    cell, scell = z((B, N), torch.int32), z((B, N), torch.int32)
    tx, ty, tz, cs = z((B, I), torch.float32), z((B,), torch.float32), z((B, J), torch.float32), z((B, K, 2), torch.float32)
    ab, res, loss = z((B, I * J * K, 2), torch.int32), z((B, F.RESULT_INTS), torch.int32), z((B,), torch.float64)
    d_tmpl, d_tstart = fitter._template_on_device()
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def grid_call(ptrs=None, B=B, N=N, r=0.2):
        ptrs = ptrs or [p(pts), p(cnt), p(grid), p(srt), p(start), p(cell), p(scell)]
        code = lib.mono_fit_grid_f32(ptrs[0], ptrs[1], B, N, r, *ptrs[2:], stream)
        torch.cuda.synchronize()
        return code
    full = [p(pts), p(cnt), p(grid), p(srt), p(start), p(cell), p(scell)]
    assert grid_call() == 0 and grid_call(B=0) == 0
    for k in range(7):
        assert grid_call([None if j == k else q for j, q in enumerate(full)]) == F.NULL, k
    for bad in (dict(B=-1), dict(N=0), dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")), dict(r=1e-30), dict(r=1e30)):
        assert grid_call(**bad) == F.BAD_SIZE, bad
    for big in (dict(B=F.MAX_B + 1), dict(N=F.MAX_N + 1)):
        assert grid_call(**big) == F.TOO_LARGE, big
    assert grid_call(full[:3] + [p(srt) + 8] + full[4:]) == F.BAD_SIZE          # `sorted` must be 16-byte aligned

    def search_call(ptrs=None, tgrid=fitter.grid, T=8, B=B, N=N, I=I, J=J, K=K, fix=None, r=0.2):
        ptrs = ptrs or search_full
        code = lib.mono_fit_search_f32(ptrs[0], ptrs[1], None if tgrid is None else ctypes.byref(tgrid), T, ptrs[2], ptrs[3], ptrs[4], ptrs[5],
                                       B, N, ptrs[6], ptrs[7], ptrs[8], ptrs[9], I, J, K, fix, r, ptrs[10], stream)
        torch.cuda.synchronize()
        return code
    search_full = [p(d_tmpl), p(d_tstart), p(grid), p(srt), p(start), p(cnt), p(tx), p(ty), p(tz), p(cs), p(ab)]
    assert search_call() == 0 and search_call(B=0) == 0 and search_call(T=0) == 0 and search_call(fix=p(res)) == 0
    for k in range(11):
        assert search_call([None if j == k else q for j, q in enumerate(search_full)]) == F.NULL, k
    assert search_call(tgrid=None) == F.NULL
    assert search_call(search_full[:3] + [p(srt) + 4] + search_full[4:]) == F.BAD_SIZE
    for bad in (dict(B=-1), dict(N=0), dict(T=-1), dict(I=0), dict(J=0), dict(K=0), dict(r=0.0), dict(r=float("nan"))):
        assert search_call(**bad) == F.BAD_SIZE, bad
    for dims, ncell in (((0, 1, 1), 0), ((33, 1, 1), 33), ((2, 2, 2), 7)):
        g = F.Grid()
        g.dim[:], g.ncell = dims, ncell
        assert search_call(tgrid=g) == F.BAD_SIZE, dims
    g = F.Grid()
    g.dim[:], g.ncell = (32, 32, 32), 32768
    assert search_call(tgrid=g) == F.TOO_LARGE                 # more cells than the template's grid may have
    for big in (dict(T=F.MAX_T + 1), dict(B=F.MAX_B + 1), dict(N=F.MAX_N + 1), dict(I=1024, J=1024, K=2), dict(K=F.MAX_H + 1),
                dict(K=F.MAX_H + 1, fix=p(res)), dict(I=F.MAX_H + 1, fix=p(res))):
        assert search_call(**big) == F.TOO_LARGE, big

    def reduce_call(ptrs=None, B=B, N=N, T=8, I=I, J=J, K=K, fix=None, one_way=0):
        ptrs = ptrs or reduce_full
        code = lib.mono_fit_reduce_f64(ptrs[0], ptrs[1], B, N, T, I, J, K, fix, one_way, ptrs[2], ptrs[3], stream)
        torch.cuda.synchronize()
        return code
    reduce_full = [p(ab), p(cnt), p(res), p(loss)]
    assert reduce_call() == 0 and reduce_call(B=0) == 0 and reduce_call(one_way=1) == 0 and reduce_call(fix=p(res)) == 0
    for k in range(4):
        assert reduce_call([None if j == k else q for j, q in enumerate(reduce_full)]) == F.NULL, k
    for bad in (dict(B=-1), dict(N=0), dict(T=-1), dict(I=0), dict(J=0), dict(K=0)):
        assert reduce_call(**bad) == F.BAD_SIZE, bad
    for big in (dict(T=F.MAX_T + 1), dict(B=F.MAX_B + 1), dict(N=F.MAX_N + 1), dict(I=1024, J=1024, K=2), dict(K=F.MAX_H + 1, fix=p(res))):
        assert reduce_call(**big) == F.TOO_LARGE, big
    assert res.cpu()[:, 3].tolist() == [F.EMPTY, F.EMPTY]       # count = 0: the last successful call wrote EMPTY records


# ================================================================================================ 7. beyond the limits
def test_a_fit_beyond_the_limits_goes_through_fit_host_and_says_so():
    from monosowa_amd import template_fit as F
    small = dict(R.GRID, opt_param1_iters=2, opt_param2_iters=2, opt_param3_iters=2)
    tmpl = R.box_template(F.MAX_T + 1, 4)
    cloud = R.noisy_copy(tmpl, 40, (0.3, 0.0, 1.0, 0.5), 5)
    fitter = _fitter(tmpl, small)
    result = fitter.fit([cloud], np.zeros((1, 3)), moving=[True], theta=[0.5])
    assert result.host and not result.x.is_cuda
    R.assert_same(result.numpy(), fitter.fit_host([cloud], np.zeros((1, 3)), moving=[True], theta=[0.5]).numpy())
    R.assert_same(result.numpy(), R.fit_f32(tmpl, [cloud], np.zeros((1, 3)), [True], [0.5], grid=small))
    inside = _fitter(tmpl[:F.MAX_T], small).fit([cloud], np.zeros((1, 3)), moving=[True], theta=[0.5])
    assert not inside.host and inside.x.is_cuda
    R.assert_same(inside.numpy(), R.fit_f32(tmpl[:F.MAX_T], [cloud], np.zeros((1, 3)), [True], [0.5], grid=small))
    too_many = _fitter(tmpl[:10], dict(R.GRID, opt_param1_iters=1024, opt_param2_iters=1024, opt_param3_iters=2))
    assert not too_many.within_limits(40, too_many._modes(1, None, None, None))


# ================================================================================================ 8. no host synchronisation
def test_fit_calls_synchronize_zero_times(monkeypatch):
    tmpl, clouds, centres, want, _ = _batch(65)
    fitter = _fitter(tmpl)
    fitter.fit(clouds, centres)                               # the library and the template are on the device
    padded = np.zeros((len(clouds), 160, 3), dtype=np.float32)
    for o, c in enumerate(clouds):
        padded[o, :len(c)] = c
    points, counts = _t(padded), _t(np.array([len(c) for c in clouds], dtype=np.int32))
    torch.cuda.synchronize()
    syncs = [0]
    real = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.__setitem__(0, syncs[0] + 1), real(*a, **k))[1])
    first = fitter.fit(clouds, centres)
    second = fitter.fit((points, counts), _t(centres), moving=[False, True, False, False, True], theta=[None, 0.4, None, None, None])
    third = fitter.fit((points, counts))
    monkeypatch.undo()
    assert syncs[0] == 0
    torch.cuda.synchronize()
    R.assert_same(first.numpy(), want)
    R.assert_same(second.numpy(), R.fit_f32(tmpl, clouds, centres, [False, True, False, False, True], [None, 0.4, None, None, None]))
    R.assert_same(third.numpy(), R.fit_f32(tmpl, clouds))
