"""-m gpu: session traces (lmpc_rollout_set_trace / _fetch_trace; csrc/lmpc_trace.hip.h) -- the per-step predictions, selected safe-set points, solver words and
inertial positions of listed cars, kept for the whole session.

The reference of every plane is the session itself stepped one simulated step at a time: after each rollout_run(1), debug_rollout_qp shows the outputs of the step
just taken, which the next solve overwrites.  The trace must hold exactly those values, so everything is compared bit for bit (as int64 words, the way
tests/test_gpu_device_commit.py::_same does).  The XY planes are compared with oracle.get_global_position on the trace's own (s, ey) columns at 1e-12 (1 + |ref|),
the project's tolerance for this map (tests/test_gpu_plant_track.py).
Set-up: N = 12, the lmpc_n12 golden, the PID lap four times in both stores (tests/closed_loop_probe.py::rollout_probe), start states spread in ey, host-drawn noise
with a fixed seed, B = 5 cars and T = 12 steps unless a case says otherwise.  What needs no device is in tests/test_session_trace_host.py."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

N, B, T = 12, 5, 12
E_ARG, E_STATE = "error -1:", "error -4:"
PLANES = ("xPred", "uPred", "ssSel", "qSel", "iters", "status")       # what debug_rollout_qp shows of a step


@pytest.fixture(scope="module")
def g(built):
    return common.load_lmpc_golden()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), what


def _refused(code, call):
    from racinglmpc_amd import _capi
    with pytest.raises(_capi.LmpcError) as e:
        call()
    assert code in str(e.value), str(e.value)
    return str(e.value)


def _lmpc_ctx(g, max_batch=8, track=None):
    """An LMPC context seeded as rollout_probe seeds it: the PID lap four times in both stores."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g if track is None else track, N, max_batch=max_batch)
    ctx = _capi.Context(cfg)
    for _ in range(4):
        ctx.model_add_trajectory(g["xPID"], g["uPID"]); ctx.ss_add_trajectory(g["xPID"], g["uPID"])
    return ctx


def _inputs(g, nb=B, steps=T, seed=5):
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (nb, 1)); x0[:, 5] = np.linspace(-0.1, 0.1, nb); x0[:, 0] += np.linspace(0.0, 0.1, nb)
    xl = np.tile(np.array(g["xPID"])[None, 1:N + 2], (nb, 1, 1)); ul = np.tile(np.array(g["uPID"])[None, 1:N + 1], (nb, 1, 1))
    return x0, xl, ul, np.random.default_rng(seed).standard_normal((steps, nb, 3))


def _begin(ctx, inp):
    x0, xl, ul, noise = inp
    ctx.rollout_begin(x0, x0, xl, ul, noise)


def _step_through(ctx, cars, steps=T, selection=True):
    """The active session stepped with rollout_run(1); after every step debug_rollout_qp of the listed cars.  {plane: (steps, len(cars), ...)}."""
    rows = {k: [] for k in PLANES if selection or k not in ("ssSel", "qSel")}
    for t in range(steps):
        assert ctx.rollout_run(1)[0] == t + 1
        qs = [ctx.debug_rollout_qp(int(b), 1, selection=selection) for b in cars]
        for k in rows:
            rows[k].append(np.stack([q[k][0] for q in qs]))
    return {k: np.stack(v) for k, v in rows.items()}


def _compare(trace, ref, what, keys=None):
    for k in (ref if keys is None else keys):
        _same(trace[k], ref[k], (what, k))


def _check_xy(table, s_ey, xy, bad_rows, what):
    """xy (steps, cars, P, 2) against the oracle on s_ey (steps, cars, P, 2 = s, ey); a point the oracle raises on must be (0, 0) and marks its (step, car) in bad_rows."""
    from oracle import lmpc_oracle as orc
    pt = np.array(table, float)
    worst = 0.0
    for idx in np.ndindex(*s_ey.shape[:3]):
        s, ey = float(s_ey[idx][0]), float(s_ey[idx][1])
        try:
            if not np.isfinite(s):                     # (the reference's `while s > TrackLength` would not return)
                raise ValueError("s is not finite")
            ref = np.array(orc.get_global_position(pt, s, ey))
        except ValueError:
            assert xy[idx][0] == 0.0 and xy[idx][1] == 0.0, (what, idx, xy[idx])
            bad_rows[idx[0], idx[1]] = True
            continue
        err = np.abs(xy[idx] - ref) / (1 + np.abs(ref))
        worst = max(worst, float(err.max()))
        assert err.max() <= 1e-12, (what, idx, s, ey, xy[idx], ref)
    return worst


@pytest.fixture(scope="module")
def stepped(g):
    """Case 1's session: capture on, all planes, cars [3, 0, 4], stepped; what every other case on the shared track compares with.  Read-only."""
    from racinglmpc_amd import _capi
    cars = [3, 0, 4]
    ctx = _lmpc_ctx(g)
    try:
        ctx.debug_rollout_capture(True)
        ctx.rollout_set_trace(cars, _capi.TRACE_ALL)
        got_cars, got_what = ctx.rollout_trace()
        assert list(got_cars) == cars and got_what == _capi.TRACE_ALL
        _begin(ctx, _inputs(g))
        ref = _step_through(ctx, cars)
        full = ctx.rollout_fetch_trace(0, T)
        part = ctx.rollout_fetch_trace(5, 9)
        logs = ctx.rollout_fetch(0, T)
        ctx.rollout_end()
    finally:
        ctx.close()
    for d in (ref, full, part):
        for a in d.values():
            a.setflags(write=False)
    return dict(cars=cars, ref=ref, full=full, part=part, logs=logs)


# ---- 1
def test_trace_is_what_each_step_computed(stepped):
    """fetch_trace(0, 12) equals the stacked xPred, uPred, ssSel, qSel, iters and status debug_rollout_qp showed after each of the twelve steps, bit for bit;
    fetch_trace(5, 9) is rows 5..8 of it."""
    full, ref, part = stepped["full"], stepped["ref"], stepped["part"]
    assert set(full) == {"xPred", "uPred", "ssSel", "qSel", "xyPred", "xySS", "iters", "status", "mapStatus"}
    assert full["xPred"].shape == (T, 3, N + 1, 6) and full["uPred"].shape == (T, 3, N, 2) and full["ssSel"].shape == (T, 3, 48, 6) and full["qSel"].shape == (T, 3, 48)
    assert full["iters"].shape == (T, 3) and full["iters"].dtype == np.int32 and full["xyPred"].shape == (T, 3, N + 1, 2) and full["xySS"].shape == (T, 3, 48, 2)
    _compare(full, ref, "whole trace")
    assert (full["iters"] > 0).all() and np.abs(full["xPred"]).max() > 0.1 and np.abs(full["ssSel"]).max() > 0.1      # (not a comparison of zeros)
    assert not np.array_equal(full["xPred"][0], full["xPred"][T - 1])
    for k in full:
        _same(part[k], full[k][5:9], ("rows 5..8", k))
    # x_0 = x0: row 0 of the prediction is the state the plant logged at that step
    X = stepped["logs"][0]
    assert np.abs(full["xPred"][:, :, 0, :] - X[:, stepped["cars"], :]).max() <= 1e-12


# ---- 2
def test_tracing_does_not_perturb_the_session(g, stepped):
    """Two untraced sessions of the same inputs are bit-identical (the precondition); a traced one (capture off, every car, one rollout_run(12)) logs the same X, U, G,
    doneAt, status, finalX, finalG, and its trace equals the stepped session's on the cars both list."""
    from racinglmpc_amd import _capi
    inp = _inputs(g)
    names = ("X", "U", "G", "doneAt", "status", "finalX", "finalG")
    ctx = _lmpc_ctx(g)
    try:
        plain = []
        for _ in range(2):
            _begin(ctx, inp)
            assert ctx.rollout_run(T)[0] == T
            plain.append(ctx.rollout_fetch(0, T))
            _refused(E_STATE, lambda: ctx.rollout_fetch_trace(0, T))         # begun without a trace
            ctx.rollout_end()
        for n, a, b in zip(names, *plain):
            _same(a, b, ("two untraced sessions", n))
        ctx.rollout_set_trace(np.arange(B), _capi.TRACE_ALL)
        _begin(ctx, inp)
        assert ctx.rollout_run(T)[0] == T
        traced = ctx.rollout_fetch(0, T)
        trace = ctx.rollout_fetch_trace(0, T)
        ctx.rollout_end()
    finally:
        ctx.close()
    for n, a, b in zip(names, traced, plain[0]):
        _same(a, b, ("traced against untraced", n))
    for n, a, b in zip(names, stepped["logs"], plain[0]):
        _same(a, b, ("stepped against one run", n))
    for k, a in stepped["full"].items():
        _same(trace[k][:, stepped["cars"]], a, ("trace of every car against the stepped session", k))


# ---- 3
def test_xy_planes_on_the_shared_track(g, stepped):
    """xyPred and xySS against oracle.get_global_position on the trace's own (s, ey) columns; mapStatus is ST_NO_SEGMENT exactly on the rows with a point the
    oracle raises on."""
    from racinglmpc_amd import _capi
    full = stepped["full"]
    bad = np.zeros((T, 3), bool)
    w1 = _check_xy(g["track"], full["xPred"][..., 4:6], full["xyPred"], bad, "xyPred")
    w2 = _check_xy(g["track"], full["ssSel"][..., 4:6], full["xySS"], bad, "xySS")
    print("XY planes against the oracle, shared track: worst scaled error %.3e (predictions) %.3e (safe-set points); rows on no segment: %d" % (w1, w2, int(bad.sum())))
    assert np.array_equal(full["mapStatus"], np.where(bad, _capi.ST_NO_SEGMENT, 0).astype(np.int32))
    assert np.abs(full["xySS"]).max() > 0.5 and np.abs(full["xyPred"]).max() > 0.5


def test_xy_points_on_no_segment(g):
    """A car that starts behind the line (s < 0 lies on no row of the table: the reference raises): its points with s < 0 are (0, 0) and its rows carry
    ST_NO_SEGMENT in mapStatus; the car beside it maps as usual."""
    from racinglmpc_amd import _capi
    x0, xl, ul, noise = _inputs(g, nb=2, steps=4)
    x0[1, 4] = -0.4
    ctx = _lmpc_ctx(g)
    try:
        ctx.rollout_set_trace([1, 0], _capi.TRACE_XPRED | _capi.TRACE_XY | _capi.TRACE_SS)
        ctx.rollout_begin(x0, x0, xl, ul, noise)
        assert ctx.rollout_run(4)[0] == 4
        tr = ctx.rollout_fetch_trace(0, 4)
        ctx.rollout_end()
    finally:
        ctx.close()
    bad = np.zeros((4, 2), bool)
    _check_xy(g["track"], tr["xPred"][..., 4:6], tr["xyPred"], bad, "xyPred")
    _check_xy(g["track"], tr["ssSel"][..., 4:6], tr["xySS"], bad, "xySS")
    assert tr["xPred"][0, 0, 0, 4] == -0.4 and bad[0, 0] and not bad[:, 1].any(), bad
    assert np.array_equal(tr["mapStatus"], np.where(bad, _capi.ST_NO_SEGMENT, 0).astype(np.int32))


def test_xy_planes_with_one_track_per_car(g):
    """Three cars on the three tracks of tests/track_cases.py: car k's points are mapped on its own table."""
    from racinglmpc_amd import _capi
    from tests import track_cases as tk
    names = list(tk.NAMES)
    ctx = _lmpc_ctx(g)
    try:
        ctx.track_set(tk.rows_of(names))
        ctx.rollout_set_trace([2, 0, 1], _capi.TRACE_XPRED | _capi.TRACE_SS | _capi.TRACE_XY)
        # the cars start well apart along the recorded lap, so that predictions and selected points lie on rows where the three tables differ
        xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
        at = [150, 60, 240]
        x0 = xP[at].copy()
        xl = np.stack([xP[r + 1:r + N + 2] for r in at]); ul = np.stack([uP[r + 1:r + N + 1] for r in at])
        ctx.rollout_begin(x0, x0, xl, ul, np.random.default_rng(5).standard_normal((T, 3, 3)))
        assert ctx.rollout_run(T)[0] == T
        tr = ctx.rollout_fetch_trace(0, T)
        ctx.rollout_end()
    finally:
        ctx.close()
    assert set(tr) == {"xPred", "ssSel", "xyPred", "xySS", "mapStatus"}
    bad = np.zeros((T, 3), bool)
    for k, car in enumerate([2, 0, 1]):
        table = np.array(tk.table(names[car])[0])
        sl = slice(k, k + 1)
        w1 = _check_xy(table, tr["xPred"][:, sl, :, 4:6], tr["xyPred"][:, sl], bad[:, sl], ("xyPred", names[car]))
        w2 = _check_xy(table, tr["ssSel"][:, sl, :, 4:6], tr["xySS"][:, sl], bad[:, sl], ("xySS", names[car]))
        print("XY planes against the oracle, car %d on track %s: worst scaled error %.3e / %.3e, rows on no segment %d" % (car, names[car], w1, w2, int(bad[:, k].sum())))
    assert np.array_equal(tr["mapStatus"], np.where(bad, _capi.ST_NO_SEGMENT, 0).astype(np.int32))
    # the check can tell the tables apart: on the L track's table the points of the cars on the other two tracks lie elsewhere
    from oracle import lmpc_oracle as orc
    for k, car in enumerate([2, 0, 1]):
        if names[car] == "L":
            continue
        pts = np.concatenate([tr["xPred"][:, k, :, 4:6].reshape(-1, 2), tr["ssSel"][:, k, :, 4:6].reshape(-1, 2)])
        got = np.concatenate([tr["xyPred"][:, k].reshape(-1, 2), tr["xySS"][:, k].reshape(-1, 2)])
        off = 0.0
        for (s_, ey_), xy_ in zip(pts, got):
            try:
                off = max(off, float(np.abs(np.array(orc.get_global_position(np.array(tk.table("L")[0]), float(s_), float(ey_))) - xy_).max()))
            except ValueError:
                pass
        assert off > 0.1, (names[car], off)


# ---- 4
@pytest.mark.parametrize("ltv", [True, False], ids=["ltv", "lti"])
def test_plain_mpc_sessions(g, ltv):
    """lmpc_rollout_begin_mpc, both forms, B = 3 (the recipe of tests/test_gpu_mpc_stages.py): XPRED | UPRED | SOLVER | XY against stepping with
    debug_rollout_qp(selection=False); SS is refused on a context without a safe set."""
    from racinglmpc_amd import _capi
    from tests.test_gpu_mpc_stages import _mpc_setup
    ctx, par, x0, form = _mpc_setup(g, 3, ltv)
    what = _capi.TRACE_XPRED | _capi.TRACE_UPRED | _capi.TRACE_SOLVER | _capi.TRACE_XY
    cars = [2, 0]
    try:
        with pytest.raises(ValueError):
            ctx.rollout_set_trace(cars, what | _capi.TRACE_SS)
        c = np.array(cars, np.int32)
        assert ctx.lib.lmpc_rollout_set_trace(ctx._h, 2, c.ctypes.data, what | _capi.TRACE_SS) == -1
        assert ctx.lib.lmpc_rollout_set_trace(ctx._h, 2, c.ctypes.data, _capi.TRACE_QSEL) == -1
        assert ctx.rollout_trace()[1] == 0                                       # (nothing in force after the refusals)
        ctx.rollout_set_trace(cars)                                              # TRACE_DEFAULT: every plane a context without a safe set records
        assert ctx.rollout_trace()[1] == what
        noise = np.random.default_rng(31).standard_normal((T, 3, 3))
        ctx.rollout_begin_mpc(x0, x0, noise, **form)
        ref = _step_through(ctx, cars, selection=False)
        tr = ctx.rollout_fetch_trace(0, T)
        _refused(E_ARG, lambda: ctx.rollout_fetch_trace(0, T, keys=["xySS"]))    # no safe set: no such plane
        ctx.rollout_end()
    finally:
        ctx.close()
    assert set(tr) == {"xPred", "uPred", "iters", "status", "xyPred", "mapStatus"}
    _compare(tr, ref, "MPC session")
    assert (tr["iters"] > 0).all()
    bad = np.zeros((T, 2), bool)
    _check_xy(g["track"], tr["xPred"][..., 4:6], tr["xyPred"], bad, "xyPred")
    assert np.array_equal(tr["mapStatus"], np.where(bad, _capi.ST_NO_SEGMENT, 0).astype(np.int32))


# ---- 5
def test_kept_buffers_serve_the_next_session(g):
    """Two sessions of one shape with another car list, a third with other planes, a fourth after rollout_release: each trace equals its own stepped reference, and
    never shows a row of the session before."""
    from racinglmpc_amd import _capi
    ctx = _lmpc_ctx(g)
    seen = []
    try:
        ctx.debug_rollout_capture(True)
        for i, (cars, what, release) in enumerate((([1, 2], _capi.TRACE_ALL, False), ([4, 0], _capi.TRACE_ALL, False),
                                                    ([4, 0], _capi.TRACE_XPRED | _capi.TRACE_SOLVER, False), ([3, 1], _capi.TRACE_ALL, True))):
            if release:
                ctx.rollout_release()
            ctx.rollout_set_trace(cars, what)
            _begin(ctx, _inputs(g, seed=5 + i))
            ref = _step_through(ctx, cars)
            tr = ctx.rollout_fetch_trace(0, T)
            ctx.rollout_end()
            _compare(tr, ref, ("session", i), keys=[k for k in ref if k in tr])
            assert ("ssSel" in tr) == bool(what & _capi.TRACE_SS) and ("xyPred" in tr) == bool(what & _capi.TRACE_XY)
            seen.append(tr)
        assert not np.array_equal(seen[0]["xPred"], seen[1]["xPred"])            # (other cars, other noise: the kept planes were written again)
    finally:
        ctx.close()


# ---- 6
def test_planes_and_refusals(g):
    """SOLVER alone with every car; every refusal of set / begin / fetch leaves the trace in force and the session usable; fetch_trace without a trace, on a PID
    session and before begin is LMPC_E_STATE; rollout_trace_bytes is the sum of the planes' sizes."""
    import ctypes as C
    from racinglmpc_amd import _capi
    inp = _inputs(g)
    ctx = _lmpc_ctx(g)
    lib, h = ctx.lib, ctx._h
    try:
        _refused(E_STATE, lambda: ctx.rollout_fetch_trace(0, 0))                 # no session
        ctx.rollout_set_trace(np.arange(B), _capi.TRACE_SOLVER)

        def raw_set(cars, what, n=None):
            c = np.asarray(cars, np.int32)
            return lib.lmpc_rollout_set_trace(h, len(c) if n is None else n, c.ctypes.data if len(c) else None, what)
        for bad in (raw_set([0], 1, n=-1), raw_set([0, 1], 0), raw_set([0, 1], 64), raw_set([0, 1], 1 | 128), raw_set([0, -1], 1), raw_set([2, 0, 2], 1),
                    lib.lmpc_rollout_set_trace(h, 2, None, 1)):
            assert bad == -1
            cars, what = ctx.rollout_trace()
            assert list(cars) == list(range(B)) and what == _capi.TRACE_SOLVER   # the trace in force is kept
        _begin(ctx, inp)
        assert ctx.rollout_run(T)[0] == T
        tr = ctx.rollout_fetch_trace(0, T)
        assert set(tr) == {"iters", "status"} and tr["iters"].shape == (T, B) and (tr["iters"] > 0).all()
        _refused(E_ARG, lambda: ctx.rollout_fetch_trace(0, T, keys=["xPred"]))   # a plane the session does not record
        _refused(E_ARG, lambda: ctx.rollout_fetch_trace(0, T, keys=["iters", "mapStatus"]))
        out = _capi.TraceOut()
        for t0, t1 in ((-1, 2), (3, 2), (0, T + 1)):
            assert lib.lmpc_rollout_fetch_trace(h, t0, t1, C.byref(out)) == -1
        assert lib.lmpc_rollout_fetch_trace(h, 0, T, None) == -1
        # a `set` during the session reaches the next one only
        ctx.rollout_set_trace([1], _capi.TRACE_XPRED)
        _same(ctx.rollout_fetch_trace(0, T)["iters"], tr["iters"], "fetch after a set during the session")
        _same(ctx.rollout_fetch_trace(4, 4)["iters"], tr["iters"][4:4], "empty range")
        status = ctx.rollout_fetch(0, T)[4]
        ctx.rollout_end()
        per_step = np.bitwise_or.reduce(tr["status"], axis=0)                   # the accumulated word holds every step's own word (and the plant's bits)
        assert np.array_equal(status & per_step, per_step), (status, per_step)
        # a car the session does not have: refused at begin, named, no session left active
        ctx.rollout_set_trace([1, B], _capi.TRACE_XPRED)
        msg = _refused(E_ARG, lambda: _begin(ctx, inp))
        assert "car %d" % B in msg
        _refused(E_STATE, lambda: ctx.rollout_fetch_trace(0, 0))
        _refused(E_ARG, lambda: ctx.rollout_run(1))                               # (no session is active)
        # the PID launch ignores the trace
        x0 = inp[0]
        rng = np.random.default_rng(3)
        t, _ = ctx.rollout_pid(x0, x0, np.full(B, 0.8), rng.standard_normal((20, B, 2)), rng.standard_normal((20, B, 3)))
        _refused(E_STATE, lambda: ctx.rollout_fetch_trace(0, t))
        assert lib.lmpc_rollout_fetch_trace(h, 0, t, C.byref(out)) == -4
        ctx.rollout_end()
        # off again: the session records nothing
        ctx.rollout_set_trace(None)
        assert ctx.rollout_trace()[0].size == 0 and ctx.rollout_trace()[1] == 0
        _begin(ctx, inp)
        ctx.rollout_run(2)
        _refused(E_STATE, lambda: ctx.rollout_fetch_trace(0, 2))
        ctx.rollout_end()
        # bytes: the sum of the planes, per step and car
        d, i = 8, 4
        per = {_capi.TRACE_XPRED: (N + 1) * 6 * d, _capi.TRACE_UPRED: N * 2 * d, _capi.TRACE_SS: 48 * 6 * d, _capi.TRACE_QSEL: 48 * d, _capi.TRACE_SOLVER: 2 * i,
               _capi.TRACE_XY: (N + 1 + 48) * 2 * d + i}
        for what in (1, 2, 4, 8, 16, 32, 63, 17, 36):
            want = 400 * 7 * sum(v for bit, v in per.items() if what & bit)
            assert ctx.rollout_trace_bytes(7, what, 400) == want == _capi.trace_bytes(N, 48, 7, what, 400), what
        assert ctx.rollout_trace_bytes(0, 63, 400) == 0
        b = C.c_longlong()
        assert lib.lmpc_rollout_trace_bytes(h, 1, 64, 1, C.byref(b)) == -1 and lib.lmpc_rollout_trace_bytes(h, -1, 1, 1, C.byref(b)) == -1
    finally:
        ctx.close()


# ---- 7
def test_per_car_lmpc_keeps_one_trace_per_generation(g):
    """PerCarLMPC(trace=[0, 2]), 3 cars, 2 generations, with the laps added by the host and committed on the device: the same traces; TraceView of car 2 has one
    prediction per logged step of each lap, and row 0 of prediction i is the lap's logged state i (x_0 = x0 is an equality row of the QP)."""
    from racinglmpc_amd import _capi, rollout
    track = np.array(g["track"])
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=16, max_lap_len=1024)
    vt = np.array([0.75, 0.8, 0.85])
    runs = []
    for dev in (False, True):
        ctx = _capi.Context(cfg)
        try:
            ro = rollout.BatchedRollouts(ctx, track, seed=5, device_noise=True)
            ro.noise_shard = (0, 3, 3)
            seeds = ro.run_pid_laps(vt, max_steps=700, keep_invalid=True)
            assert ro.last_trace is None and all(l[4] >= 0 and l[5] == 0 for l in seeds)
            loop = rollout.PerCarLMPC(ro, T_max=400, ext=40, device_commit=dev, trace=[0, 2])
            loop.seed(seeds)
            outs = [loop.run() for _ in range(2)]
            assert not loop.retired and len(loop.traces) == 2 and loop.traces[1] is ro.last_trace
            runs.append(dict(traces=loop.traces, outs=outs, lap_times=[list(t) for t in loop.lap_times]))
        finally:
            ctx.close()
    host, dev = runs
    assert host["lap_times"] == dev["lap_times"]
    for gen, (a, b) in enumerate(zip(host["traces"], dev["traces"])):
        assert set(a) == set(b) and {"xPred", "uPred", "ssSel", "qSel", "xyPred", "xySS", "iters", "status", "mapStatus", "cars", "doneAt"} == set(a)
        for k in a:
            _same(a[k], b[k], ("generation", gen, k))
        assert list(a["cars"]) == [0, 2] and list(a["doneAt"]) == [host["lap_times"][0][gen], host["lap_times"][2][gen]]
    view = rollout.TraceView(track, 2, dev["traces"])
    assert view.it == 2 and view.N == N and view.numSS_Points == 48 and view.LapTime == host["lap_times"][2]
    worst = 0.0
    for it in range(2):
        lap = host["outs"][it][2]
        assert len(view.xStoredPredTraj[it]) == view.LapTime[it] == lap[0].shape[0] == len(view.SSStoredPredTraj[it]) == len(view.xyPred[it])
        assert view.xStoredPredTraj[it][0].shape == (N + 1, 6) and view.SSStoredPredTraj[it][0].shape == (48, 6) and view.xySS[it][0].shape == (48, 2)
        x0_rows = np.stack([view.xStoredPredTraj[it][i][0] for i in range(view.LapTime[it])])
        worst = max(worst, float(np.abs(x0_rows - lap[0]).max()))
        print("lap %d: row 0 of the predictions against the logged states, worst difference %.3e" % (it, worst))
        _same(x0_rows, lap[0], ("row 0 of the predictions against the logged states", it))
        _same(view.SS[it], lap[0], ("SS", it))
        # with the lap tuples at hand the view carries the plant's own x_glob
        v2 = rollout.TraceView(track, 2, list(zip(host["traces"], [o[2] for o in host["outs"]])))
        _same(v2.SS_glob[it], lap[2], ("SS_glob", it)); _same(v2.uSS[it], lap[1], ("uSS", it))
