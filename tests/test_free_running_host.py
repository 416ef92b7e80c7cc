"""CPU: free-running sessions -- the two entry points (lmpc_rollout_relaunch, lmpc_rollout_lap_start), their declaration and binding, _capi.check_relaunch, and the
bookkeeping of rollout.FreeRunningLMPC on a scripted stand-in context against rollout.PerCarLMPC(device_commit=True) on the same script, lap by lap.  What needs a
device is in tests/test_gpu_free_running.py."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import common
from tests.test_device_commit_host import _LoopCtx
from tests.test_lap_table_host import _header_decl

NEW = ("lmpc_rollout_relaunch", "lmpc_rollout_lap_start")


def test_entry_points_are_exported_declared_and_bound(built):
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() == 116
    for name in NEW:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    types_of = lambda name: [a.rsplit(" ", 1)[0] for a in _header_decl(name)[1:]]
    assert types_of("lmpc_rollout_relaunch") == ["int", "const int *", "int"]
    assert types_of("lmpc_rollout_lap_start") == ["int *", "int *"]
    assert lib.lmpc_rollout_relaunch.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert lib.lmpc_rollout_lap_start.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    with open(common.ROOT + "/include/lmpc_hip.h") as f:
        text = f.read()
    assert "host array the car goes on" in " ".join(text.split())                              # (what a session begun on a host noise array does is stated)
    # without a context both are an argument error and write nothing
    cars = np.zeros(1, np.int32); out = np.full(2, 7, np.int32)
    assert lib.lmpc_rollout_relaunch(None, 1, cars.ctypes.data, 10) == -1
    assert lib.lmpc_rollout_lap_start(None, out.ctypes.data, out.ctypes.data) == -1 and out.tolist() == [7, 7]
    for meth in ("rollout_relaunch", "rollout_lap_start"):
        assert callable(getattr(_capi.Context, meth)), meth
        assert meth not in _capi.ContextPool.__dict__                                          # (a session belongs to one context)


def test_check_relaunch():
    from racinglmpc_amd import _capi
    cars, rows = _capi.check_relaunch([2, 0], 408)
    assert cars.dtype == np.int32 and cars.tolist() == [2, 0] and rows == 408
    assert _capi.check_relaunch(np.int64(3), np.int32(1))[0].tolist() == [3]
    for bad, why in ((([], 8), "at least one car"), (([[0, 1]], 8), "one-dimensional"), (([0.5], 8), "integers"), (([0, -1], 8), "negative"),
                     (([1, 2, 1], 8), "twice"), (([0], 0), "lap_rows"), (([0], -3), "lap_rows"), (([0], 2.5), "lap_rows"), (([0], True), "lap_rows")):
        with pytest.raises(ValueError) as e:
            _capi.check_relaunch(*bad)
        assert why in str(e.value), (bad, str(e.value))


ST_INEXACT, ST_MAXITER = 64, 1
# per lap (lockstep: per generation): (steps to the crossing per car, -1: never; status at the crossing / at the end; status during the first `ext` steps).
# Lap 0: car 2 crosses at 30 (seen at the poll at 32); car 1 at 41, one step after a multiple of 8, car 3 at 45 and car 0 at 48, ON a multiple of 8 -- three cars
# inside the poll at 48.
SCRIPT = [([48, 41, 30, 45], [0, ST_INEXACT, 0, 0], [0, 0, 0, 0]),
          ([50, 40, -1, 44], [0, 0, 0, 0], [0, 0, 0, 0]),                    # car 2 does not finish its second lap
          ([35, 55, 20, 30], [0, 0, 0, ST_MAXITER], [0, ST_MAXITER, 0, 0]),  # car 1: extension skipped; car 3: flagged at its crossing
          ([36, 33, 25, 25], [0, 0, 0, 0], [0, 0, 0, 0])]
T_LAP = 60


class _FreeCtx:
    """A context for FreeRunningLMPC's bookkeeping: lap stores that only count rows, and ONE session in which car b's k-th lap crosses SCRIPT[k][0][b] steps after it
    began, with the scripted status words.  nonfinite: a set of (lap, car) whose extension comes back not extended.  Every call is logged in `calls`."""

    def __init__(self, numSS_it, trToUse, script, ext, nonfinite=()):
        self.cfg = types.SimpleNamespace(numSS_it=numSS_it, trToUse=trToUse); self.N = 12
        self.ss, self.model, self.rows, self.script, self.ext = [], [], [], script, ext
        self.nonfinite = set(nonfinite)
        self.calls = []; self.noise = None; self.sessions = 0

    def ss_num_laps(self):
        return len(self.ss)

    def model_num_laps(self):
        return len(self.model)

    def ss_add_trajectory(self, x, u):
        self.ss.append(np.asarray(x).shape[0]); self.rows.append(np.asarray(x).shape[0])

    def model_add_trajectory(self, x, u):
        self.model.append(np.asarray(x).shape[0])

    def model_set_lap_table(self, rows):
        self._model_rows = np.array(rows); self.calls.append(("model_table", getattr(self, "t", -1)))

    def ss_set_lap_table(self, rows, last=None):
        self._ss_rows, self._ss_last = np.array(rows), np.array(last); self.calls.append(("ss_table", getattr(self, "t", -1)))

    def rollout_set_noise(self, on, seed=0, lap=0, car0=0):
        self.noise = (bool(on), int(seed), int(lap), int(car0))

    def rollout_begin(self, x0, xglob0, xLin0, uLin0, noise, T_max=None):
        assert noise is None and self.noise[0]                                # the device source
        self.B = B = np.asarray(x0).shape[0]; self.t = 0; self.T_max = int(T_max); self.sessions += 1
        assert np.asarray(xLin0).shape == (B, self.N + 1, 6) and np.asarray(uLin0).shape == (B, self.N, 2)
        self.start = [0] * B; self.lap = [0] * B; self.done = [-1] * B
        self.calls.append(("begin", self.T_max, self.noise[2]))

    def _cross(self):
        for b in range(self.B):
            T = self.script[self.lap[b]][0][b] if self.lap[b] < len(self.script) else -1
            if self.done[b] < 0 and T >= 0 and self.t >= self.start[b] + T:
                self.done[b] = self.start[b] + T

    def rollout_run(self, n):
        assert n >= 1 and self.t + n <= (self.t // 8 + 1) * 8 and self.t < self.T_max       # a chunk ends at the next multiple of 8 at the latest
        self.t = min(self.T_max, self.t + n)
        self._cross()
        self.calls.append(("run", self.t))
        return self.t, sum(d >= 0 for d in self.done)

    def rollout_fetch(self, t0, t1):
        assert 0 <= t0 <= t1 <= self.t
        B, n = self.B, t1 - t0
        self.calls.append(("fetch", self.t, t0, n))
        st = []
        for b in range(B):
            lap = self.script[min(self.lap[b], len(self.script) - 1)]
            st.append(lap[1][b] if self.done[b] >= 0 or self.t - self.start[b] > self.ext else lap[2][b])
        X = np.tile(np.arange(B, dtype=float)[None, :, None], (n, 1, 6))
        return X, np.zeros((n, B, 2)), np.zeros((n, B, 6)), np.array(self.done, np.int32), np.array(st, np.int32), np.zeros((B, 6)), np.zeros((B, 6))

    def rollout_extend_laps(self, cars, laps, n_rows):
        assert len(cars) == len(laps) >= 1 and len(set(laps)) == len(laps)
        assert all(self.t - self.start[b] == n_rows and self.done[b] < 0 for b in cars)       # exactly n_rows steps into the lap
        self.calls.append(("extend", self.t, list(cars), list(laps), int(n_rows)))
        flags = []
        for b, lap in zip(cars, laps):
            ok = (self.lap[b], int(b)) not in self.nonfinite
            flags.append(ok)
            if ok:
                self.rows[int(lap)] += int(n_rows)
        return np.array(flags, bool)

    def rollout_commit_laps(self, cars, rows=None, ss=True, model=True):
        assert rows is None and ss and model and len(cars) >= 1 and list(cars) == sorted(cars)
        self.calls.append(("commit", self.t, list(cars)))
        first = len(self.ss)
        for b in cars:
            T = self.done[b] - self.start[b]
            assert self.done[b] >= 0 and T >= 1
            self.ss.append(T); self.rows.append(T); self.model.append(T)
        return first, first

    def rollout_relaunch(self, cars, lap_rows):
        assert len(cars) >= 1 and len(set(cars)) == len(cars) and all(self.done[b] >= 0 for b in cars)
        self.calls.append(("relaunch", self.t, list(cars), int(lap_rows), self._model_rows.copy(), self._ss_rows.copy(), self._ss_last.copy()))
        for b in cars:
            self.start[b] = self.t; self.lap[b] += 1; self.done[b] = -1

    def rollout_end(self):
        self.calls.append(("end", self.t))


def _seeds():
    lap = lambda T, ends: (np.zeros((T, 6)), np.zeros((T, 2)), None, np.zeros(12), T if ends else T - 20, 0)
    # car 0: one lap that ends at the line; car 1: two laps, the second faster; car 2 and 3: one whole (multi-lap) run each, rows past the line
    return [lap(50, True), [lap(70, True), lap(60, True)], lap(80, False), [lap(90, False)]]


def _free(ext=10, nonfinite=(), laps=4, script=SCRIPT, max_steps=None):
    from racinglmpc_amd import rollout
    ctx = _FreeCtx(3, 2, script, ext, nonfinite)
    ro = rollout.BatchedRollouts(ctx, np.array(common.load_lmpc_golden()["track"]), seed=1, device_noise=True)
    loop = rollout.FreeRunningLMPC(ro, T_lap=T_LAP, ext=ext)
    loop.seed(_seeds())
    out = loop.run(laps=laps, max_steps=max_steps)
    return ctx, ro, loop, out


def _lockstep(nonfinite=()):
    from racinglmpc_amd import rollout
    ctx = _LoopCtx(3, 2, SCRIPT, nonfinite)
    ro = rollout.BatchedRollouts(ctx, np.array(common.load_lmpc_golden()["track"]), seed=1, prefetch=False)
    loop = rollout.PerCarLMPC(ro, T_max=T_LAP, ext=10, device_commit=True)
    loop.seed(_seeds())
    outs = [loop.run() for _ in range(len(SCRIPT))]
    return ctx, ro, loop, outs


def _books(ctx, loop):
    """Per car: the lengths its histories name, in order, and the rows those safe-set laps hold now (extensions included) -- whatever their store indices."""
    return [([n for n, _ in loop.ss_hist.entries[b]], [ctx.rows[i] for _, i in loop.ss_hist.entries[b]], [n for n, _ in loop.model_hist.entries[b]], ctx.rows[int(loop.last[b])])
            for b in range(loop.B)]


@pytest.mark.parametrize("nonfinite", [(), ((1, 0),)], ids=["script", "script_with_a_nan_row"])
def test_the_books_equal_those_of_the_lockstep_loop(nonfinite):
    from racinglmpc_amd import rollout
    fc, fro, fl, fout = _free(nonfinite=nonfinite)
    lc, lro, ll, louts = _lockstep(nonfinite)
    assert fl.lap_times == ll.lap_times and fl.retired == ll.retired, (fl.lap_times, ll.lap_times, fl.retired, ll.retired)
    assert _books(fc, fl) == _books(lc, ll)
    assert sorted(fc.ss) == sorted(lc.ss) and sorted(fc.rows) == sorted(lc.rows) and fc.model == fc.ss       # the same laps, in crossing order here
    for b in range(4):                                                      # what run() returns: the car's laps in order
        want = [o[b] for o in louts if o[b] is not None]
        assert [(o[4], o[5], o[2]) for o in fout[b]] == [(o[4], o[5], None) for o in want]
        assert all(o[0].shape == (min(o[4], 14), 6) and o[1].shape == (min(o[4], 14), 2) for o in fout[b])
    if not nonfinite:
        assert fl.retired == {2: (1, 0), 1: (2, ST_MAXITER | rollout.PerCarLMPC.EXT_SKIPPED), 3: (2, ST_MAXITER)}
        assert fl.lap_times == [[48, 50, 35, 36], [41, 40], [30], [45, 44]]
    else:
        assert fl.retired[0] == (1, rollout.PerCarLMPC.EXT_SKIPPED) and fl.lap_times[0] == [48]
    assert fc.sessions == 1 and fro.lap == (3 if nonfinite else 4) and lro.lap == 0      # (the lockstep stand-in draws on the host; here: one session, then the laps the busiest car began)


def test_order_and_arguments_of_the_calls():
    """ext = 10: stops at every multiple of 8 and where a car is exactly 10 steps into a lap; at a stop the extension comes first, then ONE commit of the newly crossed
    cars in ascending order, the tables, ONE relaunch; the session is read only where the count of finished cars has moved, an extension is due or a car is overdue."""
    fc, fro, fl, fout = _free()
    assert [c[0] for c in fc.calls[:3]] == ["model_table", "ss_table", "begin"]                # (the rollouts object hands its rows over in front of the session)
    calls = fc.calls[2:]
    assert calls[0] == ("begin", 4 * (T_LAP + 8), 0) and calls[-1][0] == "end" and fc.noise == (True, 1, 0, 0)
    runs = [c[1] for c in calls if c[0] == "run"]
    assert runs[:11] == [8, 10, 16, 24, 32, 40, 42, 48, 52, 56, 58]        # 10: cars 0 and 1 (seeds that end at the line); 42: car 2, relaunched at 32; 52: car 1; 58: cars 0 and 3
    body = [c for c in calls if c[0] not in ("run", "fetch")]
    assert body[1] == ("extend", 10, [0, 1], [0, 2], 10)                   # each car's latest lap: store indices 0 and 2 (the seeds are laps 0 .. 4)
    assert body[2] == ("commit", 32, [2]) and [c[0] for c in body[2:6]] == ["commit", "model_table", "ss_table", "relaunch"]
    assert body[5][:4] == ("relaunch", 32, [2], T_LAP + 8)
    assert body[5][4][2].tolist() == [5, 3] and body[5][5][2].tolist() == [5, 3, 3] and body[5][6][2] == 5      # the tables in force at the relaunch name the lap just stored
    # the stop at 42 is car 2's extension; it also sees car 1, which crossed at 41, one step after a multiple of 8: the extension first, then commit and relaunch
    assert body[6] == ("extend", 42, [2], [5], 10) and body[7] == ("commit", 42, [1]) and body[10][:4] == ("relaunch", 42, [1], T_LAP + 8)
    assert body[11] == ("commit", 48, [0, 3]) and body[14][:4] == ("relaunch", 48, [0, 3], T_LAP + 8)          # crossings at 45 and at 48 inside one poll: one call each
    assert body[15] == ("extend", 52, [1], [6], 10) and body[16] == ("extend", 58, [0, 3], [7, 8], 10)
    # every relaunch directly behind the tables of its commit, every extension exactly ext steps in (the stand-in asserts it), one commit / relaunch / extend per stop
    for k, c in enumerate(body):
        if c[0] == "relaunch":
            assert [x[0] for x in body[k - 3:k]] == ["commit", "model_table", "ss_table"] and body[k - 3][1] == c[1] and set(c[2]) <= set(body[k - 3][2])
    for kind in ("commit", "relaunch", "extend"):
        at = [c[1] for c in body if c[0] == kind]
        assert len(at) == len(set(at)), (kind, at)
    # reads: only (0, 0) fetches and the heads of stored laps; never at a stop where nothing happened
    reads = [c for c in calls if c[0] == "fetch"]
    assert all(c[3] <= 14 for c in reads)
    read_at = {c[1] for c in reads if c[3] == 0}
    assert {8, 16, 24, 40, 56} & read_at == set() and {10, 32, 42, 48, 52, 58} <= read_at
    stops, n_reads, seconds = fl.stops[-1]
    assert stops == len(runs) and n_reads == len(read_at) < stops and seconds >= 0.0
    # the noise counter: one session begun, and the laps the busiest car began
    assert fc.sessions == 1 and fro.lap == 4 and fl.generation == 4 and fl.steps == [runs[-1]]


def test_an_extension_that_is_no_multiple_of_8():
    fc, fro, fl, fout = _free(ext=12)
    ext = [c for c in fc.calls if c[0] == "extend"]
    # (the stop at 44, car 2's extension, also sees car 1's crossing at 41 and relaunches it there: its own extension is due at 56)
    assert [(c[1], c[2]) for c in ext[:4]] == [(12, [0, 1]), (44, [2]), (56, [1]), (60, [0, 3])] and all(c[4] == 12 for c in ext)
    runs = [c[1] for c in fc.calls if c[0] == "run"]
    assert runs[:7] == [8, 12, 16, 24, 32, 40, 44]
    assert fl.lap_times == [[48, 50, 35, 36], [41, 40], [30], [45, 44]]


def test_retirement_rules():
    from racinglmpc_amd import rollout
    fc, fro, fl, fout = _free()
    # car 2: relaunched at 32, never crosses: retired at the first stop at least T_lap steps into the lap (92 = 32 + 60 or later), lap index 1, not relaunched again
    assert fl.retired[2] == (1, 0) and [c[2] for c in fc.calls if c[0] == "relaunch" and 2 in c[2]] == [[2]]
    assert any(c[0] == "fetch" and c[3] == 0 and 92 <= c[1] <= 96 for c in fc.calls)
    # car 1: flagged inside the extension rows of its third lap; car 3: flagged at the crossing of its third lap -- neither is committed or relaunched afterwards
    assert fl.retired[1] == (2, ST_MAXITER | rollout.PerCarLMPC.EXT_SKIPPED) and fl.retired[3] == (2, ST_MAXITER)
    assert len(fout[1]) == 2 and len(fout[3]) == 2 and len(fout[2]) == 1 and len(fout[0]) == 4
    assert sum(1 for c in fc.calls if c[0] == "commit" and 3 in c[2]) == 2 and sum(1 for c in fc.calls if c[0] == "relaunch" and 3 in c[2]) == 2
    # an extension that comes back not extended retires its car with EXT_SKIPPED and leaves the lap as it was
    fc2, _, fl2, _ = _free(nonfinite=((1, 0),))
    assert fl2.retired[0] == (1, rollout.PerCarLMPC.EXT_SKIPPED) and fc2.rows[int(fl2.last[0])] == 48
    # a lap left unfinished at max_steps is dropped
    fc3, fro3, fl3, out3 = _free(max_steps=40)
    assert fc3.calls[2] == ("begin", 40, 0) and fl3.lap_times == [[], [], [30], []] and fl3.steps == [40] and not fl3.retired and fro3.lap == 2


def test_refused_options():
    from racinglmpc_amd import rollout
    track = np.array(common.load_lmpc_golden()["track"])
    ctx = _FreeCtx(3, 2, SCRIPT, 10)
    ro = rollout.BatchedRollouts(ctx, track, seed=1, device_noise=True)
    for kw, why in ((dict(park=True), "park"), (dict(trace=[0]), "trace"), (dict(metrics=True), "metrics")):
        with pytest.raises(ValueError) as e:
            rollout.FreeRunningLMPC(ro, T_lap=T_LAP, ext=10, **kw)
        assert why in str(e.value)
    for kw, why in ((dict(park=True), "park"), (dict(trace=[0]), "trace"), (dict(metrics=True), "metrics")):
        with pytest.raises(ValueError) as e:
            rollout.FreeRunningLMPC(rollout.BatchedRollouts(ctx, track, seed=1, device_noise=True, **kw), T_lap=T_LAP, ext=10)
        assert why in str(e.value)
    with pytest.raises(ValueError) as e:
        rollout.FreeRunningLMPC(rollout.BatchedRollouts(ctx, track, seed=1, prefetch=False), T_lap=T_LAP, ext=10)
    assert "device_noise" in str(e.value)
    with pytest.raises(RuntimeError):
        rollout.FreeRunningLMPC(ro, T_lap=T_LAP, ext=10).run(laps=1)
    # a lap that crosses the line within its first `ext` steps
    short = [([48, 41, 30, 45], [0, 0, 0, 0], [0, 0, 0, 0]), ([9, 40, 40, 40], [0, 0, 0, 0], [0, 0, 0, 0])]
    with pytest.raises(ValueError) as e:
        _free(laps=2, script=short)
    assert "car 0" in str(e.value) and "extension" in str(e.value)
