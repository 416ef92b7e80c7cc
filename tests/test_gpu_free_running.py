"""-m gpu: a car starts its next lap inside the running session (lmpc_rollout_relaunch, lmpc_rollout_lap_start; rollout.FreeRunningLMPC).

The reference of every case is the path that existed before: the session ended and a fresh one begun from the host-computed start state (finX less TrackLength),
from the fetched rows 1 .. N + 1 and with the next lap word of the device noise -- and, for the driver, generations of rollout.PerCarLMPC(device_commit=True).
Everything is compared bit for bit (as int64 words): cars are independent problems, the kernels, routes and inputs are the same on both sides (same B, no reroute,
per-car tables, counter-based noise) -- the argument parking and device commit rest on.
N = 12, max_batch = 4, T_lap = 400, ext = 40, device noise, three cars seeded with PID laps at vt = 0.75, 0.8, 0.85 (tests/test_gpu_device_commit.py), so the cars cross
at different polls.  What needs no device is in tests/test_free_running_host.py."""
import ctypes as C

import numpy as np
import pytest

from tests import common, store_ref

pytestmark = pytest.mark.gpu

N = 12
SEED, T_LAP, EXT, CAP = 5, 400, 40, 3 * 408
VT = np.array([0.75, 0.8, 0.85])
E_ARG, E_STATE = -1, -4


@pytest.fixture(scope="module")
def g():
    return common.load_lmpc_golden()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), what


def _stores(ctx):
    """Everything the stores hold, as the public entry points show it (tests/test_gpu_device_commit.py)."""
    ss = [ctx.store_read_lap(1, l) + (ctx.ss_lap_time(l), ctx.ss_lap_rows(l)) for l in range(ctx.ss_num_laps())]
    nm = ctx.model_num_laps()
    return dict(ss=ss, model=[ctx.store_read_lap(0, p)[:2] for p in range(nm)], info=[ctx.model_lap_info(k) for k in range(nm)], image=[ctx.debug_model_image(k) for k in range(nm)])


def _same_stores(a, b, what):
    assert len(a["ss"]) == len(b["ss"]) and len(a["model"]) == len(b["model"]), what
    for l, (p, q) in enumerate(zip(a["ss"], b["ss"])):
        for k in range(3):
            _same(p[k], q[k], (what, "safe set", l, "xuq"[k]))
        assert p[3:] == q[3:], (what, "safe set", l, p[3:], q[3:])
    for l, (p, q) in enumerate(zip(a["model"], b["model"])):
        _same(p[0], q[0], (what, "regression store", l, "x")); _same(p[1], q[1], (what, "regression store", l, "u"))
    assert a["info"] == b["info"], (what, a["info"], b["info"])
    for l, (p, q) in enumerate(zip(a["image"], b["image"])):
        assert p[2] == q[2], (what, "image chunks", l)
        _same(p[0], q[0], (what, "image words", l)); _same(p[1], q[1], (what, "image parameters", l))


def _session_words(ctx, t):
    """What a refused call must leave alone: logs, books and the controller's carried state of the active session."""
    return ctx.rollout_fetch(0, t) + ctx.debug_rollout_peek(3) + ctx.rollout_lap_start()


def _seeded(g, cls, ref=None, **kw):
    """A context with three PID seed laps in both stores and a loop of class `cls` on it.  ref: a store_ref.RefStores that receives every lap the host hands in."""
    from racinglmpc_amd import _capi, rollout
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=16, max_lap_len=1024)
    ctx = _capi.Context(cfg)
    try:
        if ref is not None:
            for name in ("ss_add_trajectory", "model_add_trajectory"):
                def both(*args, _real=getattr(ctx, name), _ref=getattr(ref, name)):
                    _ref(*args)
                    return _real(*args)
                setattr(ctx, name, both)
        ro = rollout.BatchedRollouts(ctx, np.array(g["track"]), seed=SEED, device_noise=True)
        ro.noise_shard = (0, 3, 3)
        seeds = ro.run_pid_laps(VT, max_steps=700, keep_invalid=True)
        assert all(l[4] >= 0 and l[5] == 0 for l in seeds)
        loop = cls(ro, **kw)
        loop.seed(seeds)
    except Exception:
        ctx.close()
        raise
    return ctx, ro, loop


def _first_lap(ctx, ro, loop, T=CAP):
    """The first LMPC lap of all three cars in a session of capacity T, three steps past the poll that saw the last crossing (so that no car is at its crossing
    step), committed to both stores, books and tables updated as the loops update them and handed to the context.  The session stays active.  Returns t, done, st, fx, fg."""
    x0, xg0, xl, ul = loop._start_arrays()
    ro.begin(x0, xl, ul, xg0, T)
    t, nd = ctx.rollout_run(T_LAP)
    assert nd == 3 and t % 8 == 0 and t < T_LAP
    t, nd = ctx.rollout_run(3)
    _, _, _, done, st, fx, fg = ctx.rollout_fetch(0, 0)
    assert (done >= N + 2).all() and (done < t).all() and not (st & ~64).any(), (t, done, st)
    first, first_model = ctx.rollout_commit_laps([0, 1, 2])
    for k in range(3):
        loop.ss_hist.add(k, int(done[k]), first + k); loop.model_hist.add(k, int(done[k]), first_model + k); loop.last[k] = first + k
    loop._hand_tables()
    ctx.model_set_lap_table(ro.lap_table); ctx.ss_set_lap_table(ro.ss_table, ro.ss_last)
    return t, done, st, fx, fg


@pytest.fixture(scope="module")
def fresh(built, g):
    """The reference path, once: the first lap as _first_lap runs it, the session ended, a fresh one begun for the second lap of all three cars and run until every
    car has crossed.  What the relaunching sessions below must reproduce."""
    from racinglmpc_amd import rollout
    ctx, ro, loop = _seeded(g, rollout.PerCarLMPC, T_max=T_LAP, ext=EXT, device_commit=True)
    try:
        t1, done1, st1, fx, fg = _first_lap(ctx, ro, loop)
        X, U = ctx.rollout_fetch(0, N + 2)[:2]
        ctx.rollout_end()
        x0 = fx.copy(); x0[:, 4] -= ro.TL                                    # xF (SysModel.py:50) on the host: one FP64 subtraction
        xl = np.ascontiguousarray(X[1:N + 2].transpose(1, 0, 2)); ul = np.ascontiguousarray(U[1:N + 1].transpose(1, 0, 2))
        lap_word = ro.lap
        ro.begin(x0, xl, ul, fg.copy(), CAP)                                 # (the tables of _first_lap; rollout_set_noise(lap + 1): the rollouts object counts its sessions)
        assert ctx.rollout_get_noise()[2] == lap_word == 2                   # PID session 0, first lap 1, this one 2
        peek = ctx.debug_rollout_peek(3)
        starts = ctx.rollout_lap_start()
        t, nd = ctx.rollout_run(24)
        head = ctx.rollout_fetch(0, 24)
        t, nd = ctx.rollout_run(T_LAP)
        assert nd == 3
        whole = ctx.rollout_fetch(0, t)
        ctx.rollout_end()
        return dict(t1=t1, done1=done1, st1=st1, peek=peek, starts=starts, head=head, whole=whole, t=t)
    finally:
        ctx.close()


def test_relaunch_equals_a_fresh_begin(built, g, fresh):
    """All three cars relaunched three steps past the last poll: the carried state right after the call, the 24 rows logged from lapStart on, the status words and the
    lap books against a fresh session's -- and the session rows in front of lapStart untouched."""
    from racinglmpc_amd import rollout
    ctx, ro, loop = _seeded(g, rollout.PerCarLMPC, T_max=T_LAP, ext=EXT, device_commit=True)
    try:
        t1, done1, st1, fx, fg = _first_lap(ctx, ro, loop)
        assert t1 == fresh["t1"] and np.array_equal(done1, fresh["done1"]) and (done1 != t1).all()
        before = ctx.rollout_fetch(0, t1)
        for a, b in zip(ctx.rollout_lap_start(), fresh["starts"]):
            assert not a.any() and not b.any()                               # a session without a relaunch: zeros
        ctx.rollout_relaunch([0, 1, 2], T_LAP + 8)
        for k, (a, b) in enumerate(zip(ctx.debug_rollout_peek(3), fresh["peek"])):
            _same(a, b, ("peek right after the relaunch", k))
        start, lap = ctx.rollout_lap_start()
        assert start.tolist() == [t1] * 3 and lap.tolist() == [1, 1, 1]
        done, st, fx2, fg2 = ctx.rollout_fetch(0, 0)[3:]
        assert (done == -1).all() and not st.any() and not fx2.any() and not fg2.any()
        t, nd = ctx.rollout_run(24)
        assert t == t1 + 24 and nd == 0
        got = ctx.rollout_fetch(t1, t)
        for k, name in enumerate(("X", "U", "Xglob", "doneAt", "status", "finalX", "finalXglob")):
            _same(got[k], fresh["head"][k], ("24 steps after the relaunch", name))
        for k, name in enumerate(("X", "U", "Xglob")):
            _same(ctx.rollout_fetch(0, t1)[k], before[k], ("rows in front of the lap start", name))
        ctx.rollout_end()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def alone(built, g, fresh):
    """Car 0 relaunched alone (cars 1 and 2 stay done and keep being stepped) and run to its crossing; its second lap committed with rows=None and its first lap
    extended by the second's first EXT rows.  Every host-side lap, and the restatement of the two device calls from the fetched rows, goes to tests/store_ref.py."""
    from racinglmpc_amd import rollout
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=16, max_lap_len=1024)
    ref = store_ref.RefStores.like(cfg)
    ctx, ro, loop = _seeded(g, rollout.PerCarLMPC, ref=ref, T_max=T_LAP, ext=EXT, device_commit=True)
    try:
        t1, done1, st1, fx, fg = _first_lap(ctx, ro, loop)
        X1, U1 = ctx.rollout_fetch(0, t1)[:2]
        for b in range(3):
            ref.ss_add_trajectory(X1[:done1[b], b], U1[:done1[b], b]); ref.model_add_trajectory(X1[:done1[b], b], U1[:done1[b], b])
        _same_stores(_stores(ctx), ref.snapshot(), "first laps against the restatement")
        ctx.rollout_relaunch([0], T_LAP + 8)
        start, lap = ctx.rollout_lap_start()
        t, nd = ctx.rollout_run(T_LAP)
        X, U, G, done, st, fx2, fg2 = ctx.rollout_fetch(0, t)
        assert nd == 3 and done[0] > t1 and done[1] == done1[1] and done[2] == done1[2]
        out = dict(t1=t1, t=t, start=start, lap=lap, X=X, U=U, G=G, done=done, st=st, fx=fx2, fg=fg2)
        # lmpc_rollout_commit_laps / _extend_laps count from the lap start
        s, d = int(start[0]), int(done[0])
        out["first"] = ctx.rollout_commit_laps([0])
        ref.ss_add_trajectory(X[s:d, 0], U[s:d, 0]); ref.model_add_trajectory(X[s:d, 0], U[s:d, 0])
        out["after_commit"] = (_stores(ctx), ref.snapshot())
        out["extended"] = ctx.rollout_extend_laps([0], [int(loop.last[0])], EXT)
        ref.ss_extend_lap(int(loop.last[0]), X[s:s + EXT, 0], U[s:s + EXT, 0])
        out["after_extend"] = (_stores(ctx), ref.snapshot())
        out["explicit"] = ctx.rollout_commit_laps([0, 1], [t - s, 20], model=False)           # explicit rows: car 0 from its lap start, car 1 (never relaunched) from row 0
        ref.ss_add_trajectory(X[s:t, 0], U[s:t, 0]); ref.ss_add_trajectory(X[:20, 1], U[:20, 1])
        out["after_explicit"] = (_stores(ctx), ref.snapshot())
        out["too_many"] = ctx.lib.lmpc_rollout_commit_laps(ctx._h, 1, np.array([0], np.int32).ctypes.data, np.array([t - s + 1], np.int32).ctypes.data, 1, None, None)
        out["too_many_ext"] = ctx.lib.lmpc_rollout_extend_laps(ctx._h, 1, np.array([0], np.int32).ctypes.data, np.array([0], np.int32).ctypes.data, t - s + 1, np.zeros(1, np.int32).ctypes.data)
        out["metrics"] = ctx.lib.lmpc_rollout_lap_metrics(ctx._h, 1, np.array([1], np.int32).ctypes.data, None, np.zeros(32).ctypes.data)
        out["after_refusals"] = _stores(ctx)
        ctx.rollout_end()
        return out
    finally:
        ctx.close()


def test_timestep_is_the_laps(alone, fresh):
    """Car 0's whole second lap, relaunched alone at session step t1, against the same lap of a fresh session: the selection's Q-function shift near the line reads
    timeStep, which must count the steps of the lap (the session's t + 1 would differ from the first row on)."""
    s, d = int(alone["start"][0]), int(alone["done"][0])
    X, U, G, done, st, fx, fg = fresh["whole"]
    assert alone["start"].tolist() == [alone["t1"], 0, 0] and alone["lap"].tolist() == [1, 0, 0]
    assert d - s == done[0] and done[0] >= N + 2, (s, d, done)
    for name, a, b in (("X", alone["X"], X), ("U", alone["U"], U), ("Xglob", alone["G"], G)):
        _same(a[s:d, 0], b[:done[0], 0], ("second lap of car 0", name))
    assert alone["st"][0] == st[0]
    _same(alone["fx"][0], fx[0], "crossing state"); _same(alone["fg"][0], fg[0], "crossing state, global")


def test_commit_and_extend_count_from_the_lap_start(alone):
    """rows=None is doneAt - lapStart, explicit rows and n_rows are checked against t - lapStart, and the rows written are those of the lap: against
    ss_add_trajectory / model_add_trajectory / ss_extend_lap of the fetched rows [lapStart, ..), restated by tests/store_ref.py."""
    s, d, t = int(alone["start"][0]), int(alone["done"][0]), alone["t"]
    assert alone["first"] == (6, 6) and alone["extended"].tolist() == [True] and alone["explicit"] == (7, None)
    for key in ("after_commit", "after_extend", "after_explicit"):
        _same_stores(alone[key][0], alone[key][1], key)
    ss = alone["after_explicit"][0]["ss"]
    assert ss[6][3:] == (d - s, d - s) and ss[3][4] == ss[3][3] + EXT and ss[7][4] == t - s and ss[8][4] == 20
    assert alone["too_many"] == E_ARG and alone["too_many_ext"] == E_ARG and alone["metrics"] == E_STATE
    _same_stores(alone["after_refusals"], alone["after_explicit"][0], "after the refused calls")


def _history_laps(ctx, loop):
    """Per car, the laps its histories name, in the order they were added: (safe-set x, u, Qfun, LapTime, rows) and (regression-store x, u, image words, image
    parameters, chunks), read through the store indices the histories hold."""
    out = []
    for b in range(loop.B):
        ss, model = [], []
        for _, idx in loop.ss_hist.entries[b]:
            ss.append(ctx.store_read_lap(1, idx) + (ctx.ss_lap_time(idx), ctx.ss_lap_rows(idx)))
        for _, idx in loop.model_hist.entries[b]:
            model.append(tuple(ctx.store_read_lap(0, ctx.model_lap_info(idx)[1])[:2]) + tuple(ctx.debug_model_image(idx)))
        out.append((ss, model))
    return out


def _named(loop, table, hist):
    """A table's rows as (car, position in that car's history) pairs: which laps it names, whatever their store indices."""
    where = {}
    for b, e in enumerate(hist.entries):
        for k, (_, idx) in enumerate(e):
            where.setdefault(idx, (b, k))
    return [[where[int(i)] for i in row] for row in np.atleast_2d(table)]


def test_the_driver_equals_the_lockstep_loop(built, g):
    """FreeRunningLMPC.run(laps=3) against three PerCarLMPC(device_commit=True).run() generations from the same seeds: lap times, retired cars, every stored lap of
    every car (safe set with Qfun and extension rows, regression store with its prefilter image) read through the car's history, and the laps the tables name."""
    from racinglmpc_amd import rollout
    fctx, fro, free = _seeded(g, rollout.FreeRunningLMPC, T_lap=T_LAP, ext=EXT)
    lctx, lro, lock = _seeded(g, rollout.PerCarLMPC, T_max=T_LAP, ext=EXT, device_commit=True)
    try:
        out = free.run(laps=3)
        outs = [lock.run() for _ in range(3)]
        assert free.lap_times == lock.lap_times and all(len(t) == 3 for t in free.lap_times), (free.lap_times, lock.lap_times)
        assert free.retired == lock.retired == {}
        assert fro.lap == lro.lap and free.generation == lock.generation == 3
        assert free.steps[-1] <= sum(lock.steps), (free.steps, lock.steps)                      # one session, no longer than the three lockstep ones together (equal where one car is the slowest of every lap)
        fl, ll = _history_laps(fctx, free), _history_laps(lctx, lock)
        longer = 0
        for b in range(3):
            assert len(fl[b][0]) == len(ll[b][0]) and len(fl[b][1]) == len(ll[b][1])
            for k, (p, q) in enumerate(zip(fl[b][0], ll[b][0])):
                for j in range(3):
                    _same(p[j], q[j], ("safe set", b, k, "xuq"[j]))
                assert p[3:] == q[3:], ("LapTime and rows", b, k, p[3:], q[3:])
                longer += p[4] > p[3]
            for k, (p, q) in enumerate(zip(fl[b][1], ll[b][1])):
                for j in range(4):
                    _same(p[j], q[j], ("regression store", b, k, ("x", "u", "image words", "image parameters")[j]))
                assert p[4] == q[4]
            for gen in range(3):                                                                 # and what run() hands back, lap by lap
                fo, lo = out[b][gen], outs[gen][b]
                _same(fo[0], lo[0], (b, gen, "head x")); _same(fo[1], lo[1], (b, gen, "head u")); _same(fo[3], lo[3], (b, gen, "final state"))
                assert fo[2] is None and fo[4:] == lo[4:]
        assert longer >= 1                                                                       # the extension was exercised
        assert _named(free, fro.ss_table, free.ss_hist) == _named(lock, lro.ss_table, lock.ss_hist)
        assert _named(free, fro.lap_table, free.model_hist) == _named(lock, lro.lap_table, lock.model_hist)
        assert _named(free, free.last[:, None], free.ss_hist) == _named(lock, lock.last[:, None], lock.ss_hist)
        assert fctx.ss_num_laps() == lctx.ss_num_laps() == 12
    finally:
        fctx.close(); lctx.close()


def test_refusals_leave_session_and_stores_as_they_were(built, g):
    """Every refusal of lmpc_rollout_relaunch with its code and the car named, each leaving the session's logs, books and carried state and both stores bit for bit
    as before the call; and the sessions that cannot relaunch at all."""
    from racinglmpc_amd import _capi, rollout
    ctx, ro, loop = _seeded(g, rollout.PerCarLMPC, T_max=T_LAP, ext=EXT, device_commit=True)
    i32 = lambda v: np.array(v, np.int32)
    def call(cars, lap_rows=T_LAP, n=None):
        cars = None if cars is None else i32(cars)
        rc = ctx.lib.lmpc_rollout_relaunch(ctx._h, len(cars) if n is None else n, None if cars is None else cars.ctypes.data, lap_rows)
        return rc, ctx.lib.lmpc_last_error().decode()
    try:
        assert call([0])[0] == E_STATE                                                           # no session active
        with pytest.raises(_capi.LmpcError):
            ctx.rollout_lap_start()
        x0, xg0, xl, ul = loop._start_arrays()
        ro.begin(x0, xl, ul, xg0, CAP)
        t, _ = ctx.rollout_run(16)
        stores, words = _stores(ctx), _session_words(ctx, t)
        rc, msg = call([1])                                                                      # nobody has crossed after 16 steps
        assert rc == E_STATE and "car 1" in msg, msg
        t, nd = ctx.rollout_run(T_LAP)
        assert nd == 3
        stores, words = _stores(ctx), _session_words(ctx, t)
        for cars, kw, code, named in (([], {}, E_ARG, None), (None, dict(n=1), E_ARG, None), ([3], {}, E_ARG, "car 3"), ([-1], {}, E_ARG, "car -1"),
                                      ([0, 2, 0], {}, E_ARG, "car 0"), ([0], dict(lap_rows=0), E_ARG, None)):
            rc, msg = call(cars, **kw)
            assert rc == code and (named is None or named in msg), (cars, kw, rc, msg)
            for k, (a, b) in enumerate(zip(_session_words(ctx, t), words)):
                _same(a, b, ("session after a refused call", cars, kw, k))
            _same_stores(_stores(ctx), stores, ("stores after a refused call", cars, kw))
        ctx.rollout_relaunch([1], T_LAP)
        t, _ = ctx.rollout_run(8)                                                                # car 1 is 8 steps into its second lap, cars 0 and 2 are done
        words = _session_words(ctx, t)
        rc, msg = call([0, 1])
        assert rc == E_STATE and "car 1" in msg, msg
        for k, (a, b) in enumerate(zip(_session_words(ctx, t), words)):
            _same(a, b, ("session after a refused call", "car 1 has not crossed", k))
        ctx.rollout_end()
        # a lap with fewer than N + 2 rows: a start just in front of the line
        x0[:, 4] = ro.TL - 0.02
        ro.begin(x0, xl, ul, xg0, CAP)
        t, nd = ctx.rollout_run(8)
        done = ctx.rollout_fetch(0, 0)[3]
        short = [b for b in range(3) if 0 <= done[b] < N + 2]
        assert nd >= 1 and short, done
        words = _session_words(ctx, t)
        rc, msg = call(short[:1])
        assert rc == E_ARG and "car %d" % short[0] in msg, msg
        for k, (a, b) in enumerate(zip(_session_words(ctx, t), words)):
            _same(a, b, ("session after a refused call", "a lap shorter than N + 2 rows", k))
        ctx.rollout_end()
        # sessions begun with parking or with a trace in force
        x0, xg0, xl, ul = loop._start_arrays()
        ctx.rollout_set_parking(_capi.PARK_FINISHED)
        ro.begin(x0, xl, ul, xg0, CAP); ctx.rollout_run(T_LAP)
        assert call([0])[0] == E_STATE and "parking" in call([0])[1]
        ctx.rollout_end(); ctx.rollout_set_parking(0)
        ctx.rollout_set_trace([0], _capi.TRACE_SOLVER)
        ro.begin(x0, xl, ul, xg0, CAP); ctx.rollout_run(T_LAP)
        assert call([0])[0] == E_STATE and "trace" in call([0])[1]
        ctx.rollout_end(); ctx.rollout_set_trace(None)
        # a session of another kind
        ctx.rollout_pid(x0, xg0, VT, None, None, stop_at_line=True, T_max=700)
        assert call([0])[0] == E_STATE
        ctx.rollout_end()
        _same_stores(_stores(ctx), stores, "stores at the end")
    finally:
        ctx.close()


def test_unused_means_unchanged(built, g, fresh):
    """A session that never relaunches answers lapStart = lapNo = 0, and its fetch, commit and extend calls give what they gave before the entry point existed:
    the rows of the session from row 0, restated by tests/store_ref.py."""
    from racinglmpc_amd import rollout
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=16, max_lap_len=1024)
    ref = store_ref.RefStores.like(cfg)
    ctx, ro, loop = _seeded(g, rollout.PerCarLMPC, ref=ref, T_max=T_LAP, ext=EXT, device_commit=True)
    try:
        x0, xg0, xl, ul = loop._start_arrays()
        ro.begin(x0, xl, ul, xg0, CAP)
        t, nd = ctx.rollout_run(T_LAP)
        t, nd = ctx.rollout_run(3)
        assert t == fresh["t1"]
        start, lap = ctx.rollout_lap_start()
        assert start.dtype == lap.dtype == np.int32 and start.tolist() == lap.tolist() == [0, 0, 0]
        X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
        assert np.array_equal(done, fresh["done1"]) and np.array_equal(st, fresh["st1"])
        assert ctx.rollout_commit_laps([0, 1, 2]) == (3, 3)
        assert ctx.rollout_extend_laps([2, 0], [0, 4], EXT).tolist() == [True, True]
        assert ctx.rollout_commit_laps([1], [t], model=False) == (6, None)
        ctx.rollout_end()
        for b in range(3):
            ref.ss_add_trajectory(X[:done[b], b], U[:done[b], b]); ref.model_add_trajectory(X[:done[b], b], U[:done[b], b])
        ref.ss_extend_lap(0, X[:EXT, 2], U[:EXT, 2]); ref.ss_extend_lap(4, X[:EXT, 0], U[:EXT, 0])
        ref.ss_add_trajectory(X[:t, 1], U[:t, 1])
        _same_stores(_stores(ctx), ref.snapshot(), "a session without a relaunch against the restatement")
    finally:
        ctx.close()
