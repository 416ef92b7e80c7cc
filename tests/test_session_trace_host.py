"""CPU: session traces (lmpc_rollout_set_trace / _get_trace / _trace_bytes / _fetch_trace) -- what needs no device: exports, declarations and bindings; the plane
table and the byte count in Python; the argument checks of the Python layer that raise before the library is called; the hand-over by BatchedRollouts; and
rollout.TraceView indexed exactly as the reference's plots index an LMPC object (plot.py:50-103, :146-169).  The GPU side is tests/test_gpu_session_trace.py."""
import os
import re

import numpy as np
import pytest

from tests import common

NEW = ("lmpc_rollout_set_trace", "lmpc_rollout_get_trace", "lmpc_rollout_trace_bytes", "lmpc_rollout_fetch_trace")


def _header():
    with open(os.path.join(common.ROOT, "include", "lmpc_hip.h")) as f:
        return f.read()


def _header_decl(name):
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
    return None if m is None else [" ".join(a.replace("*", " * ").split()) for a in m.group(1).split(",")]


def test_entry_points_are_exported_declared_and_bound(built):
    """liblmpc_hip.so is version 110 or later and exports the four entry points; include/lmpc_hip.h declares them, the plane bits and lmpc_trace_out as the issue
    writes them; _capi binds them with those types and Context has the four methods.  Without a context every one is LMPC_E_ARG, not a crash."""
    import ctypes as C
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 110
    for name in NEW:
        assert name in _capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).restype is C.c_int, name
    types = lambda name: [a.rsplit(" ", 1)[0] for a in _header_decl(name)[1:]]
    assert types("lmpc_rollout_set_trace") == ["int", "const int *", "unsigned"]
    assert types("lmpc_rollout_get_trace") == ["int *", "int *", "unsigned *", "int"]
    assert types("lmpc_rollout_trace_bytes") == ["int", "unsigned", "int", "long long *"]
    assert types("lmpc_rollout_fetch_trace") == ["int", "int", "const lmpc_trace_out *"]
    assert lib.lmpc_rollout_set_trace.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    assert lib.lmpc_rollout_get_trace.argtypes == [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_uint), C.c_int]
    assert lib.lmpc_rollout_trace_bytes.argtypes == [C.c_void_p, C.c_int, C.c_uint, C.c_int, C.POINTER(C.c_longlong)]
    assert lib.lmpc_rollout_fetch_trace.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(_capi.TraceOut)]
    header = _header()
    bits = dict(re.findall(r"LMPC_TRACE_([A-Z]+)\s*=\s*(\d+)", header))
    assert bits == dict(XPRED="1", UPRED="2", SS="4", QSEL="8", SOLVER="16", XY="32")
    assert (_capi.TRACE_XPRED, _capi.TRACE_UPRED, _capi.TRACE_SS, _capi.TRACE_QSEL, _capi.TRACE_SOLVER, _capi.TRACE_XY, _capi.TRACE_ALL) == (1, 2, 4, 8, 16, 32, 63)
    m = re.search(r"typedef struct \{([^}]*)\} lmpc_trace_out;", header)
    members = [w.strip(" *") for part in m.group(1).split(";") if part.strip() for w in part.replace("double", "").replace("int", "").split(",")]
    assert members == [k for k, _ in _capi.TraceOut._fields_] == ["xPred", "uPred", "ssSel", "qSel", "xyPred", "xySS", "iters", "status", "mapStatus"]
    assert all(t is C.c_void_p for _, t in _capi.TraceOut._fields_)
    for meth in ("rollout_set_trace", "rollout_trace", "rollout_trace_bytes", "rollout_fetch_trace"):
        assert callable(getattr(_capi.Context, meth)), meth
    n, what, b, out = C.c_int(), C.c_uint(), C.c_longlong(), _capi.TraceOut()
    assert lib.lmpc_rollout_set_trace(None, 0, None, 0) == -1 and lib.lmpc_rollout_get_trace(None, C.byref(n), None, C.byref(what), 0) == -1
    assert lib.lmpc_rollout_trace_bytes(None, 1, 1, 1, C.byref(b)) == -1 and lib.lmpc_rollout_fetch_trace(None, 0, 0, C.byref(out)) == -1


def test_plane_table_and_byte_count():
    """_capi.trace_planes / trace_bytes against the plane table of include/lmpc_hip.h written out by hand: per (step, car) XPRED (N+1) x 6 doubles, UPRED N x 2,
    SS S x 6, QSEL S, SOLVER two ints, XY (N+1) x 2 + S x 2 doubles and one int; without a safe set (S = 0) the S planes do not exist."""
    from racinglmpc_amd import _capi
    for N, S in ((12, 48), (14, 0), (40, 160), (64, 384)):
        per = {1: (N + 1) * 6 * 8, 2: N * 2 * 8, 4: S * 6 * 8, 8: S * 8, 16: 2 * 4, 32: (N + 1) * 2 * 8 + S * 2 * 8 + 4}
        for what in list(per) + [63, 3, 20, 48, 0]:
            want = sum(v for bit, v in per.items() if what & bit)
            assert _capi.trace_bytes(N, S, 1, what, 1) == want, (N, S, what)
            assert _capi.trace_bytes(N, S, 7, what, 400) == 7 * 400 * want
        keys = [k for k, bit, shp, dt in _capi.trace_planes(N, S, 63)]
        full = ["xPred", "uPred", "ssSel", "qSel", "xyPred", "xySS", "iters", "status", "mapStatus"]
        assert keys == (full if S else [k for k in full if k not in ("ssSel", "qSel", "xySS")])
        shapes = {k: (shp, np.dtype(dt)) for k, bit, shp, dt in _capi.trace_planes(N, S, 63)}
        assert shapes["xPred"] == ((N + 1, 6), np.float64) and shapes["uPred"] == ((N, 2), np.float64) and shapes["xyPred"] == ((N + 1, 2), np.float64)
        assert shapes["iters"] == ((), np.int32) and shapes["status"] == ((), np.int32) and shapes["mapStatus"] == ((), np.int32)
        if S:
            assert shapes["ssSel"] == ((S, 6), np.float64) and shapes["qSel"] == ((S,), np.float64) and shapes["xySS"] == ((S, 2), np.float64)
    assert _capi.trace_bytes(12, 48, 1, 31, 1) == 3512                 # "about 3.5 KB per traced car and step" without the XY planes


class _NoLibrary:
    """Stands where the loaded library stands: any call is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def _bare_context(numSS_it):
    from racinglmpc_amd import _capi
    ctx = object.__new__(_capi.Context)
    ctx.lib = _NoLibrary(); ctx._h = None; ctx._pid = -1
    ctx.cfg = type("cfg", (), dict(numSS_it=numSS_it, numSS_points=48))()
    ctx.N, ctx.S = 12, 48 if numSS_it else 0
    ctx._ro_trace = None
    return ctx


def test_argument_checks_raise_before_the_library_is_called():
    """check_trace and Context.rollout_set_trace: no planes, unknown bits, a negative or repeated car, a list that is not one-dimensional or not of integers, SS / QSEL
    without a safe set -- ValueError, the library untouched.  TRACE_DEFAULT resolves to every plane the context can record."""
    from racinglmpc_amd import _capi
    lm, mpc = _bare_context(4), _bare_context(0)
    for ctx, cars, what in ((lm, [0, 1], 0), (lm, [0, 1], 64), (lm, [0, 1], -1), (lm, [0, -1], 1), (lm, [2, 0, 2], 1), (lm, [[0, 1]], 1), (lm, [0.5], 1),
                            (mpc, [0], _capi.TRACE_SS), (mpc, [0], _capi.TRACE_QSEL | _capi.TRACE_XPRED), (mpc, [0], _capi.TRACE_ALL)):
        with pytest.raises(ValueError):
            ctx.rollout_set_trace(cars, what)
    cars, what = _capi.check_trace([3, 0, 4], None, 4)
    assert cars.dtype == np.int32 and list(cars) == [3, 0, 4] and what == 63                     # (the order given is kept)
    assert _capi.check_trace([1], None, 0)[1] == 63 & ~(4 | 8)
    assert _capi.check_trace([1], _capi.TRACE_XY | _capi.TRACE_SOLVER, 0)[1] == 48
    for off in (None, [], np.zeros(0, np.int64)):
        cars, what = _capi.check_trace(off, 63, 4)
        assert cars.size == 0 and what == 0
    with pytest.raises(ValueError):
        lm.rollout_fetch_trace(5, 4)                                                              # t1 < t0
    with pytest.raises(ValueError):
        from racinglmpc_amd import rollout
        rollout.BatchedRollouts(lm, np.zeros((3, 6)), trace=[0, 0])


class _Recorder:
    """Stands where the device context stands for the lap runners: keeps the order of the calls and answers with scripted logs."""
    N = 12

    def __init__(self, numSS_it=4, done=(7, -1, 9)):
        self.cfg = type("cfg", (), dict(numSS_it=numSS_it, trToUse=4))()
        self.calls, self.done = [], np.array(done, np.int32)

    def rollout_set_trace(self, cars, what):
        self.calls.append(("set_trace", list(cars), what))

    def rollout_begin(self, x0, xg, xl, ul, noise, T_max=None):
        self.B = x0.shape[0]; self.calls.append(("begin",))

    def rollout_begin_mpc(self, x0, xg, noise, **kw):
        self.B = x0.shape[0]; self.calls.append(("begin_mpc",))

    def rollout_run(self, n):
        self.calls.append(("run", n)); return 10, 2

    def rollout_fetch(self, t0, t1):
        n, B = t1 - t0, self.B
        return np.zeros((n, B, 6)), np.zeros((n, B, 2)), np.zeros((n, B, 6)), self.done[:B], np.zeros(B, np.int32), np.zeros((B, 6)), np.zeros((B, 6))

    def rollout_fetch_trace(self, t0, t1):
        self.calls.append(("fetch_trace", t0, t1)); return dict(xPred=np.zeros((t1 - t0, 2, 13, 6)))

    def rollout_end(self):
        self.calls.append(("end",))


def test_batched_rollouts_hand_the_trace_over_and_keep_the_last_one():
    """BatchedRollouts(trace=): rollout_set_trace before every begin and run_mpc_laps; the trace is fetched before rollout_end and kept in last_trace with the listed
    cars and their crossing steps; return values unchanged; a listed car the session does not have is refused before the session begins; without trace= the context
    is not touched."""
    from racinglmpc_amd import rollout
    x0 = np.zeros((3, 6)); xl = np.zeros((13, 6)); ul = np.zeros((12, 2))
    ctx = _Recorder()
    ro = rollout.BatchedRollouts(ctx, np.zeros((3, 6)) + 1.0, prefetch=False, trace=[2, 0])
    assert ro.last_trace is None
    laps = ro.run_lap_device(x0, xl, ul, max_steps=20, keep_invalid=True)
    names = [c[0] for c in ctx.calls]
    assert names == ["set_trace", "begin", "run", "fetch_trace", "end"] and ctx.calls[0] == ("set_trace", [2, 0], 63) and ctx.calls[3] == ("fetch_trace", 0, 10)
    assert len(laps) == 3 and len(laps[0]) == 6
    assert set(ro.last_trace) == {"xPred", "cars", "doneAt"} and list(ro.last_trace["cars"]) == [2, 0] and list(ro.last_trace["doneAt"]) == [9, 7]
    with pytest.raises(ValueError):
        ro.run_lap_device(x0[:2], xl, ul, max_steps=20)                                           # car 2 of a two-car session
    assert [c[0] for c in ctx.calls].count("begin") == 1
    m = _Recorder(numSS_it=0)
    rm = rollout.BatchedRollouts(m, np.zeros((3, 6)) + 1.0, prefetch=False, trace=[1], trace_what=1 | 16)
    rm.run_mpc_laps(x0, A=np.zeros((3, 6, 6)), B=np.zeros((3, 6, 2)), max_steps=20, keep_invalid=True)
    assert [c[0] for c in m.calls] == ["set_trace", "begin_mpc", "run", "fetch_trace", "end"] and m.calls[0] == ("set_trace", [1], 17)
    assert list(rm.last_trace["doneAt"]) == [-1]
    plain = _Recorder()
    rp = rollout.BatchedRollouts(plain, np.zeros((3, 6)) + 1.0, prefetch=False)
    rp.run_lap_device(x0, xl, ul, max_steps=20, keep_invalid=True)
    assert [c[0] for c in plain.calls] == ["begin", "run", "end"] and rp.last_trace is None


class _Map:
    """What the reference's plots read of a Map (plot.py:57, :112): the table."""

    def __init__(self, table):
        self.PointAndTangent = table


def _synthetic_trace(cars, steps, done, N=12, S=48, seed=0, planes=None):
    rng = np.random.default_rng(seed)
    n = len(cars)
    tr = dict(xPred=rng.standard_normal((steps, n, N + 1, 6)), uPred=rng.standard_normal((steps, n, N, 2)), ssSel=rng.standard_normal((steps, n, S, 6)),
              qSel=rng.standard_normal((steps, n, S)), xyPred=rng.standard_normal((steps, n, N + 1, 2)), xySS=rng.standard_normal((steps, n, S, 2)),
              iters=rng.integers(1, 9, (steps, n)).astype(np.int32), status=np.zeros((steps, n), np.int32), mapStatus=np.zeros((steps, n), np.int32))
    tr["xPred"][..., 4] = np.abs(tr["xPred"][..., 4])                 # (s >= 0: on the track)
    if planes is not None:
        tr = {k: v for k, v in tr.items() if k in planes}
    tr["cars"] = np.array(cars, np.int32); tr["doneAt"] = np.array(done, np.int32)
    return tr


def test_trace_view_is_indexed_as_the_plots_index_an_lmpc():
    """TraceView on synthetic traces, read the way plot.py reads an LMPC object: plotClosedLoopLMPC (:50-103: SS_glob[i][0:LapTime[i], 4], SS[i][0:LapTime[i], k],
    uSS[i][0:LapTime[i] - 1, k], it) and animation_xy (:146-169: N, numSS_Points, LapTime[it], xStoredPredTraj[it][i][j, 4], SSStoredPredTraj[it][i][j, 5],
    SS_glob[it][i, 3..5]).  Each lap is cut at the car's crossing step; a car that did not cross keeps every recorded step."""
    from racinglmpc_amd import rollout
    table = np.array([[2.0, 0.0, 0.0, 0.0, 2.0, 0.0], [2.0, 2.0, np.pi, 2.0, np.pi, 1.0], [0.0, 2.0, np.pi, 2.0 + np.pi, 2.0, 0.0], [0.0, 0.0, 2 * np.pi, 4.0 + np.pi, np.pi, 1.0]])
    cars = [3, 0, 4]
    traces = [_synthetic_trace(cars, 20, [15, 20, -1], seed=1), _synthetic_trace(cars, 18, [18, 9, 12], seed=2)]
    k = 2                                                              # car 4 is entry 2 of the list
    for track in (table, _Map(table)):
        lmpc = rollout.TraceView(track, 4, traces)
        assert lmpc.it == 2 and lmpc.N == 12 and lmpc.numSS_Points == 48 and lmpc.LapTime == [20, 12] and lmpc.car == 4
        assert abs(lmpc.TrackLength - (4.0 + 2 * np.pi)) < 1e-12
        for it in range(lmpc.it):
            tr = traces[it]; LapTime = lmpc.LapTime
            assert len(lmpc.xStoredPredTraj[it]) == len(lmpc.SSStoredPredTraj[it]) == len(lmpc.uStoredPredTraj[it]) == LapTime[it]
            assert lmpc.SS_glob[it][0:LapTime[it], 4].shape == (LapTime[it],) and lmpc.SS[it][0:LapTime[it], 0].shape == (LapTime[it],)
            assert lmpc.uSS[it][0:LapTime[it] - 1, 1].shape == (LapTime[it] - 1,)
            for i in range(0, int(lmpc.LapTime[it])):
                for j in range(0, lmpc.N + 1):
                    assert lmpc.xStoredPredTraj[it][i][j, 4] == tr["xPred"][i, k, j, 4] and lmpc.xStoredPredTraj[it][i][j, 5] == tr["xPred"][i, k, j, 5]
                for j in range(0, lmpc.numSS_Points):
                    assert lmpc.SSStoredPredTraj[it][i][j, 4] == tr["ssSel"][i, k, j, 4] and lmpc.SSStoredPredTraj[it][i][j, 5] == tr["ssSel"][i, k, j, 5]
                assert lmpc.xStoredPredTraj[it][i].shape == (13, 6) and lmpc.SSStoredPredTraj[it][i].shape == (48, 6) and lmpc.uStoredPredTraj[it][i].shape == (12, 2)
                assert np.array_equal(lmpc.xyPred[it][i], tr["xyPred"][i, k]) and np.array_equal(lmpc.xySS[it][i], tr["xySS"][i, k]) and lmpc.iters[it][i] == tr["iters"][i, k]
                # without lap tuples the lap is row 0 of the predictions, and (X, Y) of SS_glob is row 0 of xyPred
                assert np.array_equal(lmpc.SS[it][i], tr["xPred"][i, k, 0]) and np.array_equal(lmpc.uSS[it][i], tr["uPred"][i, k, 0])
                x, y, psi = lmpc.SS_glob[it][i, 4], lmpc.SS_glob[it][i, 5], lmpc.SS_glob[it][i, 3]
                assert (x, y) == tuple(tr["xyPred"][i, k, 0]) and np.isfinite(psi)
    # the tangent angle SS_glob is put together with: straight rows carry their angle, an arc turns at its curvature
    assert np.allclose(rollout._track_angle(table, np.array([1.0, 2.0 + np.pi / 2, 2.0 + np.pi + 1.0, 4.0 + 1.5 * np.pi])), [0.0, np.pi / 2, np.pi, 1.5 * np.pi])
    # (trace, lap) pairs: the laps' own rows are taken, cut like the trace
    laps = [(np.full((25, 6), 1.0 + it), np.full((25, 2), 2.0 + it), np.full((25, 6), 3.0 + it)) for it in range(2)]
    v = rollout.TraceView(table, 0, list(zip(traces, laps)))
    assert v.LapTime == [20, 9] and v.SS[1].shape == (9, 6) and (v.SS[1] == 2.0).all() and (v.uSS[0] == 2.0).all() and (v.SS_glob[1] == 4.0).all() and v.SS_glob[0].shape == (20, 6)
    # one trace alone (BatchedRollouts.last_trace), fewer planes
    one = rollout.TraceView(table, 3, [_synthetic_trace(cars, 10, [4, 5, 6], planes=("xPred", "iters", "status"))])
    assert one.it == 1 and one.LapTime == [4] and one.numSS_Points is None and one.SSStoredPredTraj == [None] and np.isnan(one.uSS[0]).all() and np.isnan(one.SS_glob[0][:, 4:6]).all()
    with pytest.raises(ValueError):
        rollout.TraceView(table, 7, traces)                                                       # not a traced car
    with pytest.raises(ValueError):
        rollout.TraceView(table, 3, [_synthetic_trace(cars, 10, [4, 5, 6], planes=("uPred",))])   # no predictions
