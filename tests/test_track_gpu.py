"""Object tracks on the GPU: the kernels of libmonosowa_track.so against ``track_host`` bit for bit on every integer and flag (theta:
the same NaNs, finite values within 4 ulp of pi -- the device's atan2 is the device library's, numpy's is libm's), several windows in
one launch, more detections than a wavefront and more tracks than a workgroup has lanes, nothing written outside the outputs at two
placements, every return code and the fallback beyond the limits, no synchronisation, and lift -> track -> gather -> fit on the device
against the same chain on the host."""
import numpy as np
import pytest
import torch

import track_reference as R
from test_track_cpu import larger_window

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
WORST = [0.0]                                  # the largest |theta(device) - theta(host)| seen, printed by every test that compares


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _as_lift(centres, status, config, device=None):
    """a LiftResult that holds these centres and statuses (what the tracker reads) and nothing else"""
    from monosowa_amd import LiftResult, lift_config
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if device == "cpu" else _t
    F, M = status.shape
    fields = {"points": np.zeros((F, M, 1, 3), np.float32), "counts": np.zeros((F, M), np.int32), "total": np.zeros((F, M), np.int32),
              "centres": centres, "range": np.zeros((F, M)), "truncated": np.zeros((F, M), bool), "status": status.astype(np.int32),
              "shrink": np.zeros((F, M), np.int32)}
    lift_keys = {"frames_creation": {"nscans_before": config["frames_creation"]["nscans_before"]}}
    return LiftResult(lift_config(lift_keys), device == "cpu", **{k: put(v) for k, v in fields.items()})


def _track(windows, config, tmax):
    """[(centres, status)] through the kernels in one launch -> TrackResult.numpy()"""
    from monosowa_amd import ObjectTracker
    lifts = [_as_lift(c, s, config) for c, s in windows]
    res = ObjectTracker(config, device=_dev(), max_tracks=tmax).track(lifts if len(lifts) > 1 else lifts[0])
    assert not res.host and res.tracks.is_cuda and res.moving.dtype == torch.bool and res.theta.dtype == torch.float64
    return res.numpy()


def _compare(got, windows, config, tmax, what):
    from monosowa_amd import track_host
    for s, (c, st) in enumerate(windows):
        want = R.window_of(track_host(c, st, config, tmax).numpy(), 0)
        WORST[0] = max(WORST[0], R.assert_same(R.window_of(got, s), want, (what, s)))
    print(what, "worst |theta(device) - theta(host)| so far: %.3e (4 ulp of pi: %.3e)" % (WORST[0], R.THETA_TOL))


# ================================================================================================ 1. the kernels
def test_kernels_equal_the_host_routine_on_every_family():
    """S = 3, F = 8, M = 6: the scenes of one configuration three at a time in one launch, each window equal to ``track_host`` of it
    and to its own single-window run."""
    groups = {}
    for name, sc in sorted(R.scenes().items()):
        groups.setdefault((repr(sc["config"]), sc["tmax"]), []).append((name, sc))
    launches = 0
    for (_, tmax), members in groups.items():
        config = members[0][1]["config"]
        for at in range(0, len(members), 3):
            names = [n for n, _ in members[at:at + 3]]
            windows = [(sc["centres"], sc["status"]) for _, sc in members[at:at + 3]]
            got = _track(windows, config, tmax)
            _compare(got, windows, config, tmax, names)
            launches += len(windows) == 3
            for s, w in enumerate(windows if len(windows) > 1 else []):
                alone = _track([w], config, tmax)
                for k in R.FIELDS:
                    assert got[k][s].tobytes() == alone[k][0].tobytes(), (names[s], k)
    assert launches >= 3


@pytest.mark.parametrize("what", ["m70", "far", "w61", "w61_close"])
def test_kernels_on_the_larger_windows(what):
    """F = 3, M = 70: more detections (and tracks) than a wavefront.  F = 5, M = 70, everything far apart: 350 tracks, more than the
    workgroup has lanes.  F = 61, M = 8, Tmax = 64: the workload's window length."""
    centres, status, config, tmax = larger_window(what)
    got = _track([(centres, status)], config, tmax)
    assert got["tracks"].shape == (1, {"m70": 210, "far": 350}.get(what, 64), status.shape[0], 2)
    _compare(got, [(centres, status)], config, tmax, what)
    if what == "far":
        assert got["count"].tolist() == [350]


def test_overflow_in_a_launch_of_several_windows():
    sc = R.scenes()
    windows = [(sc[n]["centres"], sc[n]["status"]) for n in ("overflow", "lengths", "mixed")]
    got = _track(windows, R.cfg(), 4)
    _compare(got, windows, R.cfg(), 4, "Tmax = 4")
    assert got["dropped"][0] == 8 and got["dropped"][1] >= 2 and got["dropped"][2] == 0 and got["count"].tolist() == [4, 4, 4]


# ================================================================================================ 2. the outputs and nothing else
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


def _abi_track(windows, config, tmax, shift):
    from monosowa_amd import track as T
    c = T.track_config(config)
    S, (F, M) = len(windows), windows[0][1].shape
    spec = [("tracks", torch.int32, (S, tmax, F, 2)), ("length", torch.int32, (S, tmax)), ("ref_mask", torch.int32, (S, tmax)),
            ("moving", torch.uint8, (S, tmax)), ("visible", torch.uint8, (S, tmax)), ("keep", torch.uint8, (S, tmax)),
            ("theta", torch.float64, (S, tmax)), ("count", torch.int32, (S,)), ("dropped", torch.int32, (S,))]
    buf, v, inside = _carve(spec, shift)
    centres, status = _t(np.stack([w[0] for w in windows])), _t(np.stack([w[1] for w in windows]).astype(np.int32))
    code = T.load().mono_track_objects_f64(centres.data_ptr(), status.data_ptr(), S, F, M, c.ref_frame, c.d_track, c.d_move, c.d_angle, c.z0,
                                           int(c.use_pseudo_lidar), tmax, T.ALL_STAGES, *(v[k].data_ptr() for k in R.FIELDS),
                                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == 0, code
    return {k: t.cpu().numpy() for k, t in v.items()}, buf.cpu().numpy(), inside


def test_nothing_outside_the_outputs_and_the_same_bytes_at_other_addresses():
    """The entry point called directly; there is no workspace (the association's state lives in LDS).  Doubles stay 8-byte aligned."""
    sc = R.scenes()
    cases = [([(sc[n]["centres"], sc[n]["status"]) for n in ("mixed", "exact_ties", "not_detections")], R.cfg(), 11),
             ([larger_window("far")[:2]], R.cfg(ref=2), 350), ([(sc["overflow"]["centres"], sc["overflow"]["status"])], R.cfg(), 4)]
    for windows, config, tmax in cases:
        runs = []
        for shift in (0, 8):
            out, buf, inside = _abi_track(windows, config, tmax, shift)
            assert (buf[~inside] == SENTINEL).all(), (tmax, shift)
            # every byte of every output is written: each equals the host's value, none of which is the sentinel pattern
            _compare({k: out[k].astype(bool) if k in ("moving", "visible", "keep") else out[k] for k in out}, windows, config, tmax,
                     ("placement", tmax, shift))
            assert all(int(b) in (0, 1) for k in ("moving", "visible", "keep") for b in np.unique(out[k]))
            runs.append(out)
        for k in runs[0]:
            assert runs[0][k].tobytes() == runs[1][k].tobytes(), (tmax, k)


# ================================================================================================ 3. return codes and the fallback
def test_every_return_code():
    from monosowa_amd import track as T
    from monosowa_amd import lift as L
    lib, dev = T.load(), _dev()
    assert lib.mono_track_abi_version() == T.ABI_VERSION
    S, F, M, N = 2, 3, 4, 5
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    bufs = [z((S, F, M, 3), torch.float64), z((S, F, M), torch.int32), z((S, N, F, 2), torch.int32), z((S, N), torch.int32),
            z((S, N), torch.int32), z((S, N), torch.uint8), z((S, N), torch.uint8), z((S, N), torch.uint8), z((S, N), torch.float64),
            z((S,), torch.int32), z((S,), torch.int32)]
    full, stream = [t.data_ptr() for t in bufs], torch.cuda.current_stream().cuda_stream

    def call(q=full, S=S, F=F, M=M, ref=1, dt=10.0, dm=5.0, da=3.0, z0=0.2, pl=1, N=N, stages=T.ALL_STAGES):
        code = lib.mono_track_objects_f64(q[0], q[1], S, F, M, ref, dt, dm, da, z0, pl, N, stages, *q[2:], stream)
        torch.cuda.synchronize()
        return code
    assert call() == 0 and call(stages=1) == 0 and call(stages=2) == 0 and call(ref=-1) == 0 and call(ref=F) == 0
    # all-zero centres, status OK: every detection ties, the first is appended to track 0 and the others open tracks until none is left
    want = T.track_host(np.zeros((S, F, M, 3)), np.zeros((S, F, M), np.int32), R.cfg(ref=1), N).numpy()
    assert bufs[9].cpu().tolist() == want["count"].tolist() == [N, N] and bufs[10].cpu().tolist() == want["dropped"].tolist() == [5, 5]
    assert bufs[2].cpu().numpy().tobytes() == want["tracks"].tobytes() and bufs[3].cpu().tolist() == want["length"].tolist()
    assert call(dt=0.0, dm=0.0, da=0.0, z0=0.0) == 0
    for k in range(len(full)):
        assert call([None if j == k else q for j, q in enumerate(full)]) == T.NULL, k
    for bad in (dict(S=0), dict(F=0), dict(M=0), dict(N=0), dict(S=-1), dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")),
                dict(dm=-1.0), dict(dm=float("nan")), dict(da=-0.5), dict(da=float("inf")), dict(z0=-0.2), dict(z0=float("nan")),
                dict(stages=0), dict(stages=4)):
        assert call(**bad) == T.BAD_SIZE, bad
    for big in (dict(S=T.MAX_WINDOWS + 1), dict(F=L.MAX_VIEWS + 1), dict(M=L.MAX_M + 1), dict(N=T.MAX_TRACKS + 1)):
        assert call(**big) == T.TOO_LARGE, big
    assert (T.NULL, T.BAD_SIZE, T.TOO_LARGE) == (-1, -2, -3) and T.MAX_TRACKS == 896 and T.MAX_WINDOWS == 65536


def test_windows_beyond_the_limits_go_through_track_host_and_say_so():
    from monosowa_amd import ObjectTracker, track_host
    from monosowa_amd import lift as L
    from monosowa_amd import track as T
    config = R.cfg(ref=1)
    for F, M, tmax in ((2, L.MAX_M + 1, 8), (L.MAX_VIEWS + 1, 2, 8), (3, 4, T.MAX_TRACKS + 1)):
        centres, status = R.random_window(3, F, M, min(M, 4))
        tracker = ObjectTracker(config, device=_dev(), max_tracks=tmax)
        assert not tracker.within_limits(1, F, M, tmax) and tracker.within_limits(1, min(F, L.MAX_VIEWS), min(M, L.MAX_M), 8)
        res = tracker.track(_as_lift(centres, status, config))
        assert res.host and not res.tracks.is_cuda and tuple(res.tracks.shape) == (1, tmax, F, 2)
        want = track_host(centres, status, config, tmax).numpy()
        for k in R.FIELDS:
            assert res.numpy()[k].tobytes() == want[k].tobytes(), (F, M, tmax, k)
    # the default Tmax is min(F * M, the limit): four frames of 256 slots stay on the device
    centres, status = R.random_window(4, 4, L.MAX_M, 5)
    res = ObjectTracker(config, device=_dev()).track(_as_lift(centres, status, config))
    assert not res.host and tuple(res.tracks.shape) == (1, T.MAX_TRACKS, 4, 2)
    _compare(res.numpy(), [(centres, status)], config, T.MAX_TRACKS, "M = 256, Tmax = 896")
    # a result on the CPU goes through the host routine whatever the tracker's device
    sc = R.scenes()["mixed"]
    res = ObjectTracker(R.cfg(), device=_dev()).track(_as_lift(sc["centres"], sc["status"], R.cfg(), device="cpu"))
    assert res.host and not res.tracks.is_cuda


# ================================================================================================ 4. no host synchronisation
def _count_host_reads(monkeypatch):
    """Counts every torch.cuda.synchronize and every tensor-to-host path taken until ``monkeypatch.undo()``."""
    seen = []
    for owner, name in ((torch.cuda, "synchronize"), (torch.Tensor, "cpu"), (torch.Tensor, "numpy"), (torch.Tensor, "item"),
                        (torch.Tensor, "tolist"), (torch.Tensor, "__bool__"), (torch.Tensor, "__int__"), (torch.Tensor, "__float__"),
                        (torch.Tensor, "__index__")):
        real = getattr(owner, name)

        def counted(*a, _real=real, _name=name, **k):
            seen.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(owner, name, counted)
    return seen


def _lifted(n_frames, ref):
    from monosowa_amd import ObjectLifter
    args = R.lift_window(n_frames)
    lifter = ObjectLifter(R.lift_config(ref), device=_dev(), max_points=40)
    return args, lifter, lifter.lift(*(_t(a) for a in args))


def test_track_synchronises_nothing_and_reads_nothing_back(monkeypatch):
    from monosowa_amd import ObjectTracker
    args, lifter, res = _lifted(6, 2)
    tracker = ObjectTracker(R.lift_config(2), device=_dev())
    tracker.track(res)                                        # the library is loaded
    res.gather([[(0, 0)]])
    torch.cuda.synchronize()
    seen = _count_host_reads(monkeypatch)
    again = lifter.lift(*(_t(a) for a in args))
    one = tracker.track(again)
    two = tracker.track([again, res])
    gathered = again.gather(*one.gather_args(), max_views=10, max_points=100)
    monkeypatch.undo()
    assert seen == [], seen
    torch.cuda.synchronize()
    assert not one.host and not two.host and gathered[0].is_cuda
    for k in R.FIELDS:
        assert two.numpy()[k][0].tobytes() == one.numpy()[k][0].tobytes() == two.numpy()[k][1].tobytes(), k
    seen = _count_host_reads(monkeypatch)
    one.objects()                                             # the one call that waits
    monkeypatch.undo()
    assert seen and "synchronize" not in seen


# ================================================================================================ 5. the chain
def test_lift_track_gather_and_fit_on_the_device_equal_the_chain_on_the_host():
    import fit_reference as FR
    import lift_reference as LR
    from monosowa_amd import ObjectTracker, TemplateFitter, lift_host
    from monosowa_amd.lift import gather_host
    ref, K = 2, 100
    config = R.lift_config(ref)
    args, lifter, res = _lifted(6, ref)
    tr = ObjectTracker(config, device=_dev()).track(res)
    clouds, counts, centres = res.gather(*tr.gather_args(), max_views=10, max_points=K)
    kept, moving, theta = tr.objects()
    tmpl = FR.box_template(65, 1)
    fitter = TemplateFitter(tmpl, FR.CFG, device=_dev())
    fit = fitter.fit((clouds[kept], counts[kept]), centres[kept], moving=moving, theta=theta)
    assert clouds.is_cuda and not tr.host and not fit.host
    # the host chain: lift_host, the restatement's tracks, gather_host
    fields = lift_host(*args, cfg=config, max_points=40).numpy()
    LR.assert_same(res.numpy(), fields)
    margins = []
    want = R.track_literal(fields["centres"], fields["status"], config, margins=margins)
    R.check_margins(margins)
    WORST[0] = max(WORST[0], R.assert_same(R.window_of(tr.numpy(), 0), want, "chain"))
    print("chain: worst |theta(device) - theta(host)| so far: %.3e" % WORST[0])
    assert want["moving"][:3].tolist() == [False, True, False] and np.isfinite(want["theta"][1]) and want["keep"][:3].tolist() == [True, True, False]
    host = gather_host(fields, want["tracks"].astype(np.int64), want["moving"], ref, 10, K)
    LR.assert_same_gather([clouds.cpu().numpy(), counts.cpu().numpy(), centres.cpu().numpy()], host, "gather")
    assert kept == np.flatnonzero(want["keep"]).tolist() and moving == [bool(want["moving"][t]) for t in kept]
    host_theta = [None if np.isnan(want["theta"][t]) else float(want["theta"][t]) for t in kept]
    host_fit = fitter.fit([host[0][t, :host[1][t]] for t in kept], host[2][kept], moving=moving, theta=host_theta)
    got, ref_fit = fit.numpy(), host_fit.numpy()
    assert set(got) == set(ref_fit)
    for k in ref_fit:
        if k == "theta":                                      # the moving object's is the tracker's heading: atan2 of two libraries
            assert np.max(np.abs(got[k] - ref_fit[k])) <= R.THETA_TOL, (got[k], ref_fit[k])
        else:
            assert np.asarray(got[k]).tobytes() == np.asarray(ref_fit[k]).tobytes(), (k, got[k], ref_fit[k])
