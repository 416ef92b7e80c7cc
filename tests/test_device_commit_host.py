"""CPU: laps committed to the stores on the device -- the three entry points (lmpc_rollout_commit_laps, lmpc_rollout_extend_laps, lmpc_debug_model_image), their
declaration and binding, and the bookkeeping of rollout.PerCarLMPC(device_commit=True) on a scripted stand-in context against device_commit=False on the same
script.  What needs a device is in tests/test_gpu_device_commit.py."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import common
from tests.test_lap_table_host import _header_decl

NEW = ("lmpc_rollout_commit_laps", "lmpc_rollout_extend_laps", "lmpc_debug_model_image")


def test_entry_points_are_exported_declared_and_bound(built):
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 107
    for name in NEW:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    types_of = lambda name: [a.rsplit(" ", 1)[0] for a in _header_decl(name)[1:]]
    assert types_of("lmpc_rollout_commit_laps") == ["int", "const int *", "const int *", "unsigned", "int *", "int *"]
    assert types_of("lmpc_rollout_extend_laps") == ["int", "const int *", "const int *", "int", "int *"]
    assert types_of("lmpc_debug_model_image") == ["int", "unsigned *", "double *", "int *"]
    assert lib.lmpc_rollout_commit_laps.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert lib.lmpc_rollout_extend_laps.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert lib.lmpc_debug_model_image.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    with open(common.ROOT + "/include/lmpc_hip.h") as f:
        text = f.read()
    assert "#define LMPC_COMMIT_SS 1u" in text and "#define LMPC_COMMIT_MODEL 2u" in text and (_capi.COMMIT_SS, _capi.COMMIT_MODEL) == (1, 2)
    # without a context every one of them is an argument error and writes nothing
    cars = np.zeros(1, np.int32); n = C.c_int(7)
    assert lib.lmpc_rollout_commit_laps(None, 1, cars.ctypes.data, None, 3, C.byref(n), None) == -1 and n.value == 7
    assert lib.lmpc_rollout_extend_laps(None, 1, cars.ctypes.data, cars.ctypes.data, 1, cars.ctypes.data) == -1 and cars[0] == 0
    assert lib.lmpc_debug_model_image(None, 0, None, None, C.byref(n)) == -1 and n.value == 7
    for meth in ("rollout_commit_laps", "rollout_extend_laps", "debug_model_image"):
        assert callable(getattr(_capi.Context, meth)), meth


ST_INEXACT, ST_MAXITER = 64, 1
# the four-generation script of tests/test_ss_table_host.py -- per generation: (done_at per car, status at the end, status after the ext steps)
SCRIPT = [([50, 40, 30, 45], [0, ST_INEXACT, 0, 0], [0, 0, 0, 0]),
          ([50, 40, -1, 44], [0, 0, 0, 0], [0, 0, 0, 0]),                    # car 2 does not finish
          ([35, 55, 20, 30], [0, 0, 0, ST_MAXITER], [0, ST_MAXITER, 0, 0]),  # car 1: extension skipped; car 3: flagged at the end; car 2 (retired) would have been fastest
          ([36, 10, 10, 10], [0, 0, 0, 0], [0, 0, 0, 0])]


class _LoopCtx:
    """A context for PerCarLMPC's bookkeeping, both ways: lap stores that only count rows, sessions whose cars finish after scripted numbers of steps with scripted
    status, and -- nonfinite: a set of (generation, car) -- cars whose first logged rows hold a NaN: the host path sees it in the fetched rows, the device path in
    the `extended` flag of rollout_extend_laps."""

    def __init__(self, numSS_it, trToUse, script, nonfinite=()):
        self.cfg = types.SimpleNamespace(numSS_it=numSS_it, trToUse=trToUse); self.N = 12
        self.ss, self.model, self.rows, self.script, self.gen = [], [], [], script, -1
        self.nonfinite = set(nonfinite)
        self.tables = []; self.extended = []; self.fetched = []; self.commits = []; self.extends = []

    def ss_num_laps(self):
        return len(self.ss)

    def model_num_laps(self):
        return len(self.model)

    def ss_add_trajectory(self, x, u):
        self.ss.append(np.asarray(x).shape[0]); self.rows.append(np.asarray(x).shape[0])

    def model_add_trajectory(self, x, u):
        self.model.append(np.asarray(x).shape[0])

    def model_set_lap_table(self, rows):
        self._model_rows = np.array(rows)

    def ss_set_lap_table(self, rows, last=None):
        self._ss_rows, self._ss_last = np.array(rows), np.array(last)

    def ss_extend_lap(self, lap, x, u):
        assert np.isfinite(x).all() and np.isfinite(u).all()
        self.extended.append((self.gen, int(lap), np.asarray(x).shape[0])); self.rows[int(lap)] += np.asarray(x).shape[0]

    def rollout_begin(self, x0, xglob0, xLin0, uLin0, noise):
        self.gen += 1; self.B = np.asarray(x0).shape[0]; self.t = 0
        assert np.asarray(xLin0).shape == (self.B, self.N + 1, 6) and np.asarray(uLin0).shape == (self.B, self.N, 2)
        self.tables.append((self._model_rows.copy(), self._ss_rows.copy(), self._ss_last.copy()))

    def rollout_run(self, n):
        self.t = min(60, self.t + n)
        return self.t, 0

    def rollout_fetch(self, t0, t1):
        assert 0 <= t0 <= t1 <= self.t
        B, n = self.B, t1 - t0
        self.fetched.append((self.gen, n))
        done, st, early = self.script[self.gen]
        X = np.tile(np.arange(B, dtype=float)[None, :, None], (n, 1, 6)); U = np.zeros((n, B, 2))
        for gen, b in self.nonfinite:
            if gen == self.gen and n > 3:
                X[3, b, 1] = np.nan
        status = np.array(early if self.t <= 10 else st, np.int32)
        return X, U, np.zeros((n, B, 6)), np.array(done, np.int32), status, np.zeros((B, 6)), np.zeros((B, 6))

    def rollout_extend_laps(self, cars, laps, n_rows):
        assert len(cars) == len(laps) and len(set(laps)) == len(laps) and 1 <= n_rows <= self.t
        self.extends.append(self.gen)
        flags = []
        for b, lap in zip(cars, laps):
            ok = (self.gen, int(b)) not in self.nonfinite
            flags.append(ok)
            if ok:
                self.extended.append((self.gen, int(lap), int(n_rows))); self.rows[int(lap)] += int(n_rows)
        return np.array(flags, bool)

    def rollout_commit_laps(self, cars, rows=None, ss=True, model=True):
        assert rows is None and ss and model and len(cars) >= 1 and list(cars) == sorted(cars)
        self.commits.append(self.gen)
        done = self.script[self.gen][0]
        first = len(self.ss)
        for b in cars:
            assert done[b] >= 1
            self.ss.append(done[b]); self.rows.append(done[b]); self.model.append(done[b])
        return first, first

    def rollout_end(self):
        pass


def _run(device_commit, nonfinite=()):
    from racinglmpc_amd import rollout
    ctx = _LoopCtx(3, 2, SCRIPT, nonfinite)
    track = np.array(common.load_lmpc_golden()["track"])
    ro = rollout.BatchedRollouts(ctx, track, seed=1, prefetch=False)
    loop = rollout.PerCarLMPC(ro, T_max=60, ext=10, device_commit=device_commit)
    lap = lambda T, ends: (np.zeros((T, 6)), np.zeros((T, 2)), None, np.zeros(12), T if ends else T - 20, 0)
    # car 0: one lap that ends at the line; car 1: two laps, the second faster; car 2 and 3: one whole (multi-lap) run each, rows past the line
    loop.seed([lap(50, True), [lap(70, True), lap(60, True)], lap(80, False), [lap(90, False)]])
    gens = []
    for _ in range(len(SCRIPT)):
        out = loop.run()
        gens.append(dict(out=out, ss_table=ro.ss_table.tolist(), ss_last=ro.ss_last.tolist(), lap_table=ro.lap_table.tolist(), retired=dict(loop.retired),
                         lap_times=[list(t) for t in loop.lap_times]))
    return ctx, loop, gens


@pytest.mark.parametrize("nonfinite", [(), ((1, 0),)], ids=["script", "script_with_a_nan_row"])
def test_device_commit_keeps_the_books_of_the_host_loop(nonfinite):
    """The same script both ways: tables, `last`, retired cars, lap times and the stored lap lengths (extensions included) agree after every generation; the device
    run makes one commit and at most one extend call per generation and never fetches more than N + 2 rows."""
    from racinglmpc_amd import rollout
    hc, hl, hg = _run(False, nonfinite)
    dc, dl, dg = _run(True, nonfinite)
    for gen, (h, d) in enumerate(zip(hg, dg)):
        for k in ("ss_table", "ss_last", "lap_table", "retired", "lap_times"):
            assert h[k] == d[k], (gen, k, h[k], d[k])
        assert [o is None for o in h["out"]] == [o is None for o in d["out"]], gen
        for ho, do in zip(h["out"], d["out"]):
            if ho is not None:
                assert do[4] == ho[4] and do[5] == ho[5] and do[2] is None and do[0].shape == (min(ho[4], 14), 6) and do[1].shape == (min(ho[4], 14), 2)
                assert np.array_equal(do[0], ho[0][:14]) and np.array_equal(do[3], ho[3])
    assert hc.ss == dc.ss and hc.model == dc.model and hc.rows == dc.rows and hc.extended == dc.extended
    assert [t[1].tolist() for t in hc.tables] == [t[1].tolist() for t in dc.tables]
    # the reference run is the one tests/test_ss_table_host.py pins down (the plain script)
    if not nonfinite:
        assert hl.retired == {2: (1, 0), 1: (2, ST_MAXITER | rollout.PerCarLMPC.EXT_SKIPPED), 3: (2, ST_MAXITER)}
        assert hl.lap_times == [[50, 50, 35, 36], [40, 40], [30], [45, 44]]
        assert dc.extended == [(0, 0, 10), (0, 2, 10), (1, 5, 10), (1, 6, 10), (1, 7, 10), (1, 8, 10), (2, 9, 10), (2, 11, 10), (3, 12, 10)]
        assert dc.commits == [0, 1, 2, 3]                                                          # exactly one commit per generation
    assert dc.commits == [gen for gen, d in enumerate(dg) if any(o is not None for o in d["out"])]    # (one per generation that has a valid lap, none otherwise)
    assert not hc.commits and not hc.extends
    assert sorted(set(dc.extends)) == dc.extends                                                  # at most one extend call per generation
    assert max(n for _, n in dc.fetched) <= 14 and max(n for _, n in hc.fetched) > 14             # never more than N + 2 rows


def test_an_entry_that_is_not_extended_retires_its_car():
    """Car 0's first rows of generation 1 hold a NaN: rollout_extend_laps reports its entry as skipped, the car is retired with EXT_SKIPPED (and the status it had,
    none here), its lap keeps its rows, and the other cars of that call are extended."""
    from racinglmpc_amd import rollout
    dc, dl, dg = _run(True, ((1, 0),))
    assert dl.retired[0] == (1, rollout.PerCarLMPC.EXT_SKIPPED)
    assert [e for e in dc.extended if e[0] == 1] == [(1, 6, 10), (1, 7, 10), (1, 8, 10)] and dc.rows[5] == 50
    assert dg[1]["out"][0] is None and dl.lap_times[0] == [50] and dc.extends.count(1) == 1
