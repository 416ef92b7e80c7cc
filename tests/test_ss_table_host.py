"""CPU: the per-problem safe-set lap table (lmpc_ss_set_lap_table / lmpc_ss_get_lap_table) -- the symbols, their declaration and binding, the row check of the
Python layer, the hand-over by BatchedRollouts, ContextPool and save_stores / restore_stores, the fixture of the GPU tests, and the bookkeeping of
rollout.PerCarLMPC on scripted lap lengths.  What needs a context on a device is in tests/test_gpu_ss_table.py."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from tests import common
from tests import standin_capi
from tests.test_lap_table_host import _header_decl


def test_entry_points_are_exported_declared_and_bound(built):
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 106
    for name in ("lmpc_ss_set_lap_table", "lmpc_ss_get_lap_table"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    d = _header_decl("lmpc_ss_set_lap_table")
    assert d is not None and [a.rsplit(" ", 1)[0] for a in d[1:]] == ["int", "const int *", "const int *"], d
    d = _header_decl("lmpc_ss_get_lap_table")
    assert d is not None and [a.rsplit(" ", 1)[0] for a in d[1:]] == ["int *", "int *", "int *", "int"], d
    assert lib.lmpc_ss_set_lap_table.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.lmpc_ss_get_lap_table.argtypes == [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int]
    n = C.c_int(7); rows = np.zeros(4, np.int32)
    assert lib.lmpc_ss_set_lap_table(None, 1, rows.ctypes.data, None) == -1 and lib.lmpc_ss_set_lap_table(None, 0, None, None) == -1
    assert lib.lmpc_ss_get_lap_table(None, C.byref(n), None, None, 0) == -1 and n.value == 7
    with open(os.path.join(common.ROOT, "include", "lmpc_hip.h")) as f:
        text = " ".join(f.read().split())
    assert "ONLY THE REGRESSION follows the table" in text and "safe set" in text and "its own table, lmpc_ss_set_lap_table" in text
    for meth in ("ss_set_lap_table", "ss_lap_table"):
        assert callable(getattr(_capi.Context, meth)), meth


def test_row_check_of_the_python_layer():
    """_capi.check_ss_table: the shape rules of check_lap_table with numSS_it entries per row; last: one integer per row, -1 or an index."""
    from racinglmpc_amd import _capi
    assert _capi.check_ss_table(None, 4) == (None, None) and _capi.check_ss_table([], 4) == (None, None)
    r, l = _capi.check_ss_table([[3, 1], [0, 0]], 2)
    assert r.dtype == np.int32 and r.flags["C_CONTIGUOUS"] and r.tolist() == [[3, 1], [0, 0]] and l is None
    r, l = _capi.check_ss_table([[3, 1], [0, 0]], 2, last=[-1, 5])
    assert l.dtype == np.int32 and l.tolist() == [-1, 5]
    r, l = _capi.check_ss_table([2, 0, 1, 1], 4, last=np.array([2], np.int64))
    assert r.tolist() == [[2, 0, 1, 1]] and l.tolist() == [2]
    assert _capi.check_ss_table([2, 0], 1, last=[0, 2])[0].tolist() == [[2], [0]]
    for bad, L, last in (([[0, 1, 2]], 2, None), ([[0, -1]], 2, None), ([[0.0, 1.0]], 2, None), ([[0, 1]], 2, [0, 1]), ([[0, 1]], 2, [-2]), ([[0, 1]], 2, [0.0]),
                         ([[0, 1]], 2, [[0]]), (None, 2, [1]), ([[0]], 0, None)):
        with pytest.raises(ValueError):
            _capi.check_ss_table(bad, L, last)


@pytest.mark.parametrize("N", [8, 12, 14, 20, 40])
def test_fixture_of_the_gpu_tests_raises_no_window(N):
    """The fixture of tests/test_gpu_ss_table.py and tests/test_gpu_table_routes.py on the CPU, at every built-in horizon: at least 5 laps of at least 3 lengths, two
    equal LapTimes, one lap extended past the line; problems 2, 3 and 5 cross the line and 0, 1 and 4 do not, one problem takes the wrap branch, the two crossing
    problems keep zt = xP[309] and xP[312]; for every one of the 36 (problem, row) pairs of both row sets the 13-row window of every selected lap lies inside the
    lap (no LMPC_ST_WINDOW), so no case is left out of a comparison."""
    from tests import ss_table_cases as c
    g = common.load_lmpc_golden(); TL = float(g["trackLength"])
    stored = c.cpu_stored(g)
    assert stored[c.EXTENDED][0].shape[0] == stored[c.EXTENDED][3] + 30
    lt = [s[3] for s in stored]
    assert len(lt) >= 5 and len(set(lt)) >= 3 and len(set(lt)) < len(lt)
    p = c.problems(g, 6, N)
    xP = np.array(g["xPID"])
    assert c.start_steps(12) == [100, 200, 296, 299, 150, 306]
    assert p["xLin"].shape == (6, N + 1, 6) and p["uLin"].shape == (6, N, 2) and p["xPredPrev"].shape == (6, N + 1, 6)
    assert np.array_equal(p["zt"][2], xP[309]) and np.array_equal(p["zt"][3], xP[312])
    crossed = (p["xPredPrev"][:, :, 4] > TL).any(1)
    assert crossed.tolist() == [False, False, True, True, False, True] and (p["timeStep"] != 0).all() and p["hasPred"].all()
    assert (p["zt"][:, 4] - p["x0"][:, 4] > TL / 2).tolist() == [False] * 5 + [True]
    for rows, last, L in ((c.ROWS4, c.LAST4, 4), (c.ROWS2, c.LAST2, 2)):
        for r in range(6):
            order = c.own_order(rows[r], last[r], lt)
            for b in range(6):
                assert c.oracle_selection(stored, order, p, b, TL, L, 12, N=N)[4], (N, L, r, b)


class _Ctx(standin_capi.Context):
    """The stand-in context with the session entry points and the per-car settings: records the calls in order."""

    def model_set_lap_table(self, rows):
        standin_capi._rec("model_set_lap_table", np.array(rows))

    def ss_set_lap_table(self, rows, last=None):
        standin_capi._rec("ss_set_lap_table", (np.array(rows), None if last is None else np.array(last)))

    def plant_set_params(self, par):
        standin_capi._rec("plant_set_params", None)

    def rollout_begin(self, x0, xglob0, xLin0, uLin0, noise):
        standin_capi._rec("rollout_begin", None)


def test_rollouts_hand_the_table_to_the_context_before_begin():
    """BatchedRollouts(ss_table=, ss_last=): Context.ss_set_lap_table(rows, last) before every rollout_begin, after the vehicle rows and the regression table; without
    rows the context's table is not touched; a row count that is neither 1 nor the number of cars is refused before the session begins."""
    from racinglmpc_amd import rollout, _capi
    g = common.load_lmpc_golden()
    track = np.array(g["track"])
    B = 3
    cfg = types.SimpleNamespace(N=12, numSS_it=2, numSS_points=24, trToUse=2, par=None, track=track, trackLength=float(g["trackLength"]))
    x0 = np.zeros((B, 6)); rows = np.array([[0, 1], [2, 2], [1, 0]]); last = np.array([1, -1, 4])
    keep = ("plant_set_params", "model_set_lap_table", "ss_set_lap_table", "rollout_begin")

    def begin(ro):
        n0 = len(standin_capi.CALLS)
        ro.begin(x0, np.zeros((13, 6)), np.zeros((12, 2)), max_steps=5)
        return [c for c in standin_capi.CALLS[n0:] if c[0] in keep]
    for tab, lst in ((rows, last), (rows[:1], last[:1]), (rows, None)):
        ro = rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False, plant_params=_capi.plant_params(1), lap_table=rows[:1], ss_table=tab, ss_last=lst)
        for _ in range(2):
            calls = begin(ro)
            assert [c[0] for c in calls] == ["plant_set_params", "model_set_lap_table", "ss_set_lap_table", "rollout_begin"]
            got_rows, got_last = calls[2][1]
            assert np.array_equal(got_rows, tab) and got_rows.dtype == np.int32
            assert (got_last is None) if lst is None else (np.array_equal(got_last, lst) and got_last.dtype == np.int32)
    assert [c[0] for c in begin(rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False))] == ["rollout_begin"]
    ro = rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False, ss_table=rows[:2], ss_last=last[:2])
    n0 = len(standin_capi.CALLS)
    with pytest.raises(ValueError):
        ro.begin(x0, np.zeros((13, 6)), np.zeros((12, 2)), max_steps=5)
    assert not [c for c in standin_capi.CALLS[n0:] if c[0] in ("ss_set_lap_table", "rollout_begin")]
    for kw in (dict(ss_table=np.zeros((B, 3), np.int32)), dict(ss_last=[0, 1, 2]), dict(ss_table=rows, ss_last=[0, 1])):
        with pytest.raises(ValueError):
            rollout.BatchedRollouts(_Ctx(cfg), track, **kw)


def test_context_pool_fans_the_table_out_to_every_member():
    from racinglmpc_amd import _capi
    seen = []
    pool = _capi.ContextPool.__new__(_capi.ContextPool)
    pool.members = [types.SimpleNamespace(ss_set_lap_table=lambda rows, last=None, i=i: seen.append(("set", i, rows, last)),
                                          ss_lap_table=lambda i=i: seen.append(("get", i)) or "rows of %d" % i) for i in range(3)]
    pool._next = 0
    pool.ss_set_lap_table([[1, 0]], last=[1])
    assert seen == [("set", i, [[1, 0]], [1]) for i in range(3)]
    del seen[:]
    assert pool.ss_lap_table() == "rows of 0" and seen == [("get", 0)]


class _SsLib:
    """Stands where liblmpc_hip.so stands for the safe-set entry points save_stores / restore_stores use.  No regression laps."""

    def __init__(self, L):
        self.L = L; self.laps = []; self.rows = np.zeros((0, L), np.int32); self.last = None

    @staticmethod
    def _arr(p, n, ct):
        return np.ctypeslib.as_array((ct * n).from_address(p.value if isinstance(p, C.c_void_p) else int(p)))

    def lmpc_model_num_laps(self, h, n):
        n._obj.value = 0; return 0

    def lmpc_ss_num_laps(self, h, n):
        n._obj.value = len(self.laps); return 0

    def lmpc_ss_add_trajectory(self, h, x, u, T):
        T = T.value
        self.laps.append([self._arr(x, T * 6, C.c_double).reshape(T, 6).copy(), self._arr(u, T * 2, C.c_double).reshape(T, 2).copy(), np.arange(T, 0, -1.0), T]); return 0

    def lmpc_ss_replace_lap(self, h, lap, x, u, q, T):
        T = T.value
        self.laps[lap.value][:3] = [self._arr(x, T * 6, C.c_double).reshape(T, 6).copy(), self._arr(u, T * 2, C.c_double).reshape(T, 2).copy(), self._arr(q, T, C.c_double).copy()]; return 0

    def lmpc_ss_get_laptime(self, h, lap, T):
        T._obj.value = self.laps[lap.value][3]; return 0

    def lmpc_store_read_lap(self, h, store, lap, x, u, q, T):
        assert store.value == 1
        xs, us, qs, _ = self.laps[lap.value]
        T._obj.value = xs.shape[0]
        if x is not None:
            self._arr(x, xs.size, C.c_double)[:] = xs.ravel(); self._arr(u, us.size, C.c_double)[:] = us.ravel(); self._arr(q, qs.size, C.c_double)[:] = qs
        return 0

    def lmpc_ss_set_lap_table(self, h, n, rows, last):
        self.rows = np.zeros((0, self.L), np.int32) if n == 0 else self._arr(rows, n * self.L, C.c_int).reshape(n, self.L).copy()
        self.last = None if (n == 0 or last is None) else self._arr(last, n, C.c_int).copy()
        return 0

    def lmpc_ss_get_lap_table(self, h, n, rows, last, capacity):
        n._obj.value = self.rows.shape[0]
        if rows is not None:
            self._arr(rows, self.rows.size, C.c_int)[:] = self.rows.ravel()
            self._arr(last, self.rows.shape[0], C.c_int)[:] = -2 if self.last is None else self.last
        return 0


def _ss_ctx(L):
    from racinglmpc_amd import _capi
    ctx = _capi.Context.__new__(_capi.Context)
    ctx.lib = _SsLib(L); ctx._h = C.c_void_p(); ctx._pid = os.getpid(); ctx.N = 12
    ctx.cfg = types.SimpleNamespace(trToUse=1, numSS_it=L)
    return ctx


def test_save_and_restore_keep_the_table(tmp_path):
    """save_stores / restore_stores carry rows and `last`; a table set without `last` restores without one; a file written without a table restores to "no table"."""
    rng = np.random.default_rng(3)
    a = _ss_ctx(2)
    for T in (9, 5, 7):
        a.ss_add_trajectory(rng.standard_normal((T, 6)), rng.standard_normal((T, 2)))
    rows = np.array([[2, 0], [1, 1]], np.int32); last = np.array([-1, 2], np.int32)
    for lst, name in ((last, "with"), (None, "nolast")):
        a.ss_set_lap_table(rows, lst)
        got = a.ss_lap_table()
        assert np.array_equal(got[0], rows) and ((got[1] is None) if lst is None else np.array_equal(got[1], lst))
        a.save_stores(str(tmp_path / name))
        b = _ss_ctx(2)
        b.restore_stores(str(tmp_path / name))
        got = b.ss_lap_table()
        assert len(b.lib.laps) == 3 and np.array_equal(got[0], rows) and ((got[1] is None) if lst is None else np.array_equal(got[1], lst))
    a.ss_set_lap_table(None)
    a.save_stores(str(tmp_path / "without"))
    with np.load(str(tmp_path / "without.npz")) as d:
        assert "ss_lap_table" not in d.files and "ss_lap_last" not in d.files
    e = _ss_ctx(2)
    e.restore_stores(str(tmp_path / "without"))
    assert e.ss_lap_table()[0].shape == (0, 2) and e.ss_lap_table()[1] is None and len(e.lib.laps) == 3


class _LoopCtx:
    """A context for PerCarLMPC's bookkeeping: lap stores that only count, and sessions whose cars finish after scripted numbers of steps with scripted status."""

    def __init__(self, numSS_it, trToUse, script):
        self.cfg = types.SimpleNamespace(numSS_it=numSS_it, trToUse=trToUse); self.N = 12
        self.ss, self.model, self.script, self.gen = [], [], script, -1
        self.tables = []; self.extended = []

    def ss_num_laps(self):
        return len(self.ss)

    def model_num_laps(self):
        return len(self.model)

    def ss_add_trajectory(self, x, u):
        self.ss.append(np.asarray(x).shape[0])

    def model_add_trajectory(self, x, u):
        self.model.append(np.asarray(x).shape[0])

    def model_set_lap_table(self, rows):
        self._model_rows = np.array(rows)

    def ss_set_lap_table(self, rows, last=None):
        self._ss_rows, self._ss_last = np.array(rows), np.array(last)

    def ss_extend_lap(self, lap, x, u):
        self.extended.append((self.gen, int(lap), np.asarray(x).shape[0]))

    def rollout_begin(self, x0, xglob0, xLin0, uLin0, noise):
        self.gen += 1; self.B = np.asarray(x0).shape[0]; self.t = 0
        self.tables.append((self._model_rows.copy(), self._ss_rows.copy(), self._ss_last.copy()))

    def rollout_run(self, n):
        self.t = min(60, self.t + n)
        return self.t, 0

    def rollout_fetch(self, t0, t1):
        B, n = self.B, t1 - t0
        done, st, early = self.script[self.gen]
        X = np.tile(np.arange(B, dtype=float)[None, :, None], (n, 1, 6)); U = np.zeros((n, B, 2))
        status = np.array(early if self.t <= 10 else st, np.int32)
        return X, U, np.zeros((n, B, 6)), np.array(done, np.int32), status, np.zeros((B, 6)), np.zeros((B, 6))

    def rollout_end(self):
        pass


def test_per_car_lmpc_bookkeeping_on_scripted_laps():
    """PerCarLMPC on scripted lap lengths, 4 cars, numSS_it = 3, trToUse = 2: seed rows are the car's fastest lap repeated; after each generation row b holds the
    fastest entries of car b's own history with multiplicities, ties in the order added (stable); last[b] is the lap just added; a car that does not finish, is
    flagged, or whose extension is skipped is retired with (generation, status), keeps its slot, and its later laps are ignored."""
    from racinglmpc_amd import rollout
    ST_INEXACT, ST_MAXITER = 64, 1
    # per generation: (done_at per car, status at the end, status after the ext steps)
    script = [([50, 40, 30, 45], [0, ST_INEXACT, 0, 0], [0, 0, 0, 0]),
              ([50, 40, -1, 44], [0, 0, 0, 0], [0, 0, 0, 0]),                    # car 2 does not finish
              ([35, 55, 20, 30], [0, 0, 0, ST_MAXITER], [0, ST_MAXITER, 0, 0]),  # car 1: extension skipped; car 3: flagged at the end; car 2 (retired) would have been fastest
              ([36, 10, 10, 10], [0, 0, 0, 0], [0, 0, 0, 0])]
    ctx = _LoopCtx(3, 2, script)
    track = np.array(common.load_lmpc_golden()["track"])
    ro = rollout.BatchedRollouts(ctx, track, seed=1, prefetch=False)
    loop = rollout.PerCarLMPC(ro, T_max=60, ext=10)
    lap = lambda T, ends: (np.zeros((T, 6)), np.zeros((T, 2)), None, np.zeros(12), T if ends else T - 20, 0)
    # car 0: one lap that ends at the line; car 1: two laps, the second faster; car 2 and 3: one whole (multi-lap) run each, rows past the line
    loop.seed([lap(50, True), [lap(70, True), lap(60, True)], lap(80, False), [lap(90, False)]])
    assert ctx.ss == [50, 70, 60, 80, 90] and ctx.model == ctx.ss
    assert ro.ss_table.tolist() == [[0, 0, 0], [2, 2, 1], [3, 3, 3], [4, 4, 4]] and ro.ss_last.tolist() == [0, 2, 3, 4]
    assert ro.lap_table.tolist() == [[0, 0], [2, 1], [3, 3], [4, 4]]
    out = loop.run()
    assert [None if o is None else o[4] for o in out] == [50, 40, 30, 45] and not loop.retired
    assert ctx.extended == [(0, 0, 10), (0, 2, 10)]                 # cars 0 and 1 extend their latest lap; the whole runs of cars 2 and 3 need none
    assert ctx.ss == [50, 70, 60, 80, 90, 50, 40, 30, 45]
    # car 0: 50 (seed, index 0, three times) and 50 (index 5): stable -- the entries added first come first
    assert ro.ss_table.tolist() == [[0, 0, 0], [6, 2, 2], [7, 3, 3], [8, 4, 4]] and ro.ss_last.tolist() == [5, 6, 7, 8]
    assert ro.lap_table.tolist() == [[0, 0], [6, 2], [7, 3], [8, 4]]
    loop.run()
    assert loop.retired == {2: (1, 0)} and ctx.ss[9:] == [50, 40, 44]
    assert ro.ss_table.tolist() == [[0, 0, 0], [6, 9 + 1, 2], [7, 3, 3], [11, 8, 4]] and ro.ss_last.tolist() == [9, 10, 7, 11]
    loop.run()
    assert loop.retired == {2: (1, 0), 1: (2, ST_MAXITER | rollout.PerCarLMPC.EXT_SKIPPED), 3: (2, ST_MAXITER)}
    assert ctx.ss[12:] == [35]                                      # only car 0's lap is stored
    assert [e for e in ctx.extended if e[0] == 2] == [(2, 9, 10), (2, 11, 10)]      # (car 1's extension was skipped, retired car 2 has none)
    assert ro.ss_table.tolist() == [[12, 0, 0], [6, 10, 2], [7, 3, 3], [11, 8, 4]] and ro.ss_last.tolist() == [12, 10, 7, 11]
    out = loop.run()
    assert [o is None for o in out] == [False, True, True, True] and ctx.ss[13:] == [36]
    assert ro.ss_table.tolist() == [[12, 13, 0], [6, 10, 2], [7, 3, 3], [11, 8, 4]] and ro.ss_last.tolist()[0] == 13
    assert loop.lap_times == [[50, 50, 35, 36], [40, 40], [30], [45, 44]]
    # every session was begun with the tables of the generation before it, one row per car, the retired cars' rows unchanged
    assert [t[1].shape for t in ctx.tables] == [(4, 3)] * 4 and ctx.tables[3][1].tolist() == [[12, 0, 0], [6, 10, 2], [7, 3, 3], [11, 8, 4]]
