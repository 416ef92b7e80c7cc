"""CPU: per-car tracks (lmpc_track_row_from_config / lmpc_track_set / lmpc_track_get, lmpc_ss_add_trajectory_on / lmpc_ss_extend_lap_on) -- the symbols, their
declaration and binding, the table construction of racinglmpc_amd.track against the golden table and the oracle, the oracle's PID laps on the three reference
tracks (the inputs of tests/test_gpu_tracks.py), the row packing and row check of the Python layer, and the hand-over by BatchedRollouts / PerCarLMPC /
lap_from_global / LmpcGeneration on the stand-in (tests/standin_tracks.py).  What needs a context on a device is in tests/test_gpu_tracks.py."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from tests import common
from tests import standin_capi
from tests import standin_tracks
from tests import track_cases as tk
from tests.test_lap_table_host import _header_decl

NEW = ("lmpc_track_row_from_config", "lmpc_track_set", "lmpc_track_get", "lmpc_ss_add_trajectory_on", "lmpc_ss_extend_lap_on")


def test_entry_points_are_exported_declared_and_bound(built):
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 109
    for name in NEW:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    types_of = lambda name: [a.rsplit(" ", 1)[0] for a in _header_decl(name)[1:]]
    d = _header_decl("lmpc_track_row_from_config")
    assert d is not None and d[0] == "const lmpc_config *" and d[1].rsplit(" ", 1)[0] == "double *", d
    assert types_of("lmpc_track_set") == ["int", "const double *"]
    assert types_of("lmpc_track_get") == ["int *", "double *", "int"]
    assert types_of("lmpc_ss_add_trajectory_on") == ["int", "const double *", "const double *", "int"]
    assert types_of("lmpc_ss_extend_lap_on") == ["int", "int", "const double *", "const double *", "int"]
    assert lib.lmpc_track_set.argtypes == [C.c_void_p, C.c_int, C.c_void_p]
    assert lib.lmpc_track_get.argtypes == [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]
    n = C.c_int(7); row = np.zeros(98); x = np.zeros((2, 6)); u = np.zeros((2, 2))
    assert lib.lmpc_track_set(None, 1, row.ctypes.data) == -1 and lib.lmpc_track_set(None, 0, None) == -1
    assert lib.lmpc_track_get(None, C.byref(n), None, 0) == -1 and n.value == 7
    assert lib.lmpc_track_row_from_config(None, row.ctypes.data) == -1
    assert lib.lmpc_ss_add_trajectory_on(None, 0, x.ctypes.data, u.ctypes.data, 2) == -1
    assert lib.lmpc_ss_extend_lap_on(None, 0, 0, x.ctypes.data, u.ctypes.data, 2) == -1
    with open(common.ROOT + "/include/lmpc_hip.h") as f:
        text = " ".join(f.read().split())
    assert "#define LMPC_TRACK_NPAR 98" in text and _capi.TRACK_NPAR == 98
    for meth in ("track_set", "tracks"):
        assert callable(getattr(_capi.Context, meth)), meth
    assert "carry laps, not tracks" in _capi.Context.save_stores.__doc__


def test_tables_of_the_three_reference_specs():
    """table_from_spec(L) is the golden table and the oracle's, bit for bit; oval and goggle close on the x axis with heading 0, chain their cumulative s exactly
    and have 6 and 11 rows; the oval's closing row is the degenerate one (6e-16 m) and its length is 13.0 exactly."""
    from oracle import lmpc_oracle as orc
    from racinglmpc_amd import track
    tab, TL = tk.table("L")
    g = np.load(os.path.join(common.GOLDEN, "track_xy.npz"))
    assert tab.shape == g["track"].shape and tab.tobytes() == np.asarray(g["track"], float).tobytes() and TL == float(g["trackLength"])
    pt, TLo = orc.make_track()
    assert tab.tobytes() == np.asarray(pt, float).tobytes() and TL == TLo
    assert sorted(track.REFERENCE_SPECS) == ["L", "goggle", "oval"]
    for name in ("oval", "goggle"):
        t, L = tk.table(name)
        assert t.shape == (tk.TABLE_ROWS[name], 6) and t.shape[0] <= 16
        assert t[-2, 2] == 0.0 and abs(t[-2, 1]) < 1e-15, (name, t[-2])
        for i in range(1, t.shape[0]):
            assert t[i, 3] == t[i - 1, 3] + t[i - 1, 4], (name, i)
        assert L == t[-1, 3] + t[-1, 4] and np.all(t[:, 4] >= 0)
    t, L = tk.table("oval")
    assert L == 13.0 and 0 < t[-1, 4] < 1e-15
    assert tk.table("L")[0].shape[0] == tk.TABLE_ROWS["L"]
    with pytest.raises(ValueError):
        track.table_from_spec([1.0, 0.0])


@pytest.mark.parametrize("name", tk.NAMES)
def test_oracle_pid_lap_finishes_on_every_track(name):
    """oracle.pid_lap(table, 0.8, seed=7, multiLap=False): the rows measured with the oracle (300 / 200 / 295), the car inside the lane the whole lap -- the inputs
    of tests/test_gpu_tracks.py."""
    x, u, xg = tk.pid_lap(name)
    TL = tk.table(name)[1]
    print(name, "rows", x.shape[0], "worst |ey| %.3f" % np.abs(x[:, 5]).max(), "s[-1] %.4f of %.4f" % (x[-1, 4], TL))
    assert x.shape[0] == tk.PID_ROWS[name]
    assert x[-1, 4] <= TL and np.abs(x[:, 5]).max() < 0.4


def test_row_packing_and_row_check(built):
    """track_row / track_table round-trip a table; lmpc_track_row_from_config gives the row of the Python builder; check_tracks refuses what lmpc_track_set refuses."""
    from racinglmpc_amd import _capi
    lib = _capi.load()
    for name in tk.NAMES:
        t, L = tk.table(name)
        row = _capi.track_row(t)
        assert row.shape == (98,) and row[0] == t.shape[0] and row[1] == L and not row[2 + t.size:].any()
        back, Lb = _capi.track_table(row)
        assert back.tobytes() == t.tobytes() and Lb == L
        assert _capi.track_row(t, 2 * L)[1] == 2 * L
        cfg = _capi.config_from(12, np.zeros((6, 6)), np.zeros((2, 2)), np.zeros((6, 6)), [0, 0], [0, 0], np.zeros((2, 6)), [1, 1], np.zeros((4, 2)), [1, 1, 1, 1], np.zeros(6),
                                track=np.array(t), trackLength=L)
        got = np.full(98, np.nan)
        assert lib.lmpc_track_row_from_config(C.byref(cfg), got.ctypes.data) == 0
        assert got.tobytes() == row.tobytes()
    rows = tk.rows_of(tk.NAMES)
    assert rows.shape == (3, 98) and rows.dtype == np.float64 and rows.flags["C_CONTIGUOUS"]
    assert _capi.check_tracks(None) is None and _capi.check_tracks(np.zeros((0, 98))) is None
    assert np.array_equal(_capi.check_tracks(rows[1]), rows[1:2])                     # (one row: every car)

    def bad(i, j, v):
        r = rows.copy(); r[i, j] = v
        return r
    for r in (np.zeros((2, 97)), bad(1, 40, np.nan), bad(0, 1, np.inf), bad(2, 0, 0.0), bad(2, 0, 17.0), bad(0, 0, 6.5), bad(1, 1, 0.0), bad(1, 1, -13.0),
              bad(0, 2 + 6 * 3 + 4, -1e-9)):
        with pytest.raises(ValueError):
            _capi.check_tracks(r)
    assert _capi.check_tracks(bad(0, 2 + 6 * 12 + 4, -1.0)) is not None                # (a table row beyond the row count is not in use: only its finiteness is checked)
    with pytest.raises(ValueError):
        _capi.track_row(np.zeros((17, 6)))
    with pytest.raises(ValueError):
        _capi.track_row(np.zeros((3, 5)))


def _cfg(names):
    t, L = tk.table(names[0])
    return types.SimpleNamespace(N=12, numSS_it=2, numSS_points=24, trToUse=2, par=None, track=np.array(t), trackLength=L)


def _lap(T, TL, beyond=0.05):
    """A lap tuple that ends at the line: s rises to just below TL, the crossing state lies `beyond` past it."""
    x = np.zeros((T, 6)); x[:, 4] = np.linspace(0.0, TL - 0.01, T)
    fin = np.zeros(12); fin[4] = TL + beyond
    return (x, np.zeros((T, 2)), None, fin, T, 0)


def test_rollouts_hand_the_rows_to_the_context_and_use_each_cars_length():
    """BatchedRollouts(tracks=): track_set before every begin; TL per car.  PerCarLMPC on two tracks of different length: car b's lap is stored with track_row = b
    (its Q-function counts with its own TrackLength), its x0 is its crossing state shifted by its OWN TrackLength, its extension is appended with its own row; with one
    track for all cars the host writers are called as they were before there were rows."""
    from racinglmpc_amd import rollout
    names = ["L", "oval"]
    TLs = tk.lengths_of(names)
    assert TLs[0] != TLs[1]
    tabs = [np.array(tk.table(n)[0]) for n in names]
    ctx = standin_tracks.Context(_cfg(names), done=[30, 20])
    ro = rollout.BatchedRollouts(ctx, tabs[0], seed=1, prefetch=False, tracks=tabs)
    assert np.array_equal(ro.TL, TLs) and np.array_equal(ro.tracks, tk.rows_of(names)) and np.array_equal(ro.track_lengths(2), TLs)
    with pytest.raises(ValueError):
        ro.track_lengths(3)
    loop = rollout.PerCarLMPC(ro, T_max=60, ext=10)
    del standin_capi.CALLS[:]
    # car 0's lap is longer in s than the oval is long: with the oval's TrackLength its cost would stop counting early
    loop.seed([_lap(50, TLs[0]), _lap(40, TLs[1])])
    calls = [c for c in standin_capi.CALLS if c[0] in ("track_set", "ss_add_trajectory")]
    assert [c[0] for c in calls] == ["track_set", "ss_add_trajectory", "ss_add_trajectory"] and [c[1][1] for c in calls[1:]] == [0, 1]
    assert np.array_equal(ctx.tracks(), tk.rows_of(names))
    assert ctx.Qfun[0][0] == 49.0 and ctx.Qfun[1][0] == 39.0
    out = loop.run()
    x0 = ctx.begun[-1]
    assert x0[0, 4] == (TLs[0] + 0.05) - TLs[0] and x0[1, 4] == (TLs[1] + 0.05) - TLs[1]
    ext = [c[1] for c in standin_capi.CALLS if c[0] == "ss_extend_lap"]
    assert [(e[0], e[2]) for e in ext] == [(0, 0), (1, 1)]
    assert ctx.SS[0][50, 4] == 0.0 + TLs[0] and ctx.SS[1][40, 4] == 0.0 + TLs[1]          # (the appended rows: s + the car's own TrackLength)
    adds = [c[1] for c in standin_capi.CALLS if c[0] == "ss_add_trajectory"][2:]
    assert [a[1] for a in adds] == [0, 1] and [o[4] for o in out] == [30, 20]
    # the context refuses a host writer that names no car while one row per car is in force
    with pytest.raises(standin_tracks.LmpcError):
        ctx.ss_add_trajectory(np.zeros((3, 6)), np.zeros((3, 2)))
    # one track for every car: the calls of before
    ctx1 = standin_tracks.Context(_cfg(["oval"]), done=[30, 20])
    ro1 = rollout.BatchedRollouts(ctx1, tabs[1], seed=1, prefetch=False, tracks=tabs[1])
    loop1 = rollout.PerCarLMPC(ro1, T_max=60, ext=10)
    del standin_capi.CALLS[:]
    loop1.seed([_lap(50, TLs[1]), _lap(40, TLs[1])]); loop1.run()
    assert all(c[1][-1] is None for c in standin_capi.CALLS if c[0] in ("ss_add_trajectory", "ss_extend_lap"))
    assert np.array_equal(ctx1.begun[-1][:, 4], [(TLs[1] + 0.05) - TLs[1]] * 2) and ctx1.tracks().shape == (1, 98)
    # a row count that is neither 1 nor the number of cars is refused before the session begins
    ro3 = rollout.BatchedRollouts(standin_tracks.Context(_cfg(names), done=[1, 1, 1]), tabs[0], seed=1, prefetch=False, tracks=tabs)
    n0 = len(standin_capi.CALLS)
    with pytest.raises(ValueError):
        ro3.begin(np.zeros((3, 6)), np.zeros((13, 6)), np.zeros((12, 2)), max_steps=5)
    assert not [c for c in standin_capi.CALLS[n0:] if c[0] in ("track_set", "rollout_begin")]
    import inspect
    assert "tracks" in inspect.signature(rollout.bootstrap).parameters


def test_generation_loop_with_a_shared_safe_set_refuses_two_tracks():
    from racinglmpc_amd import rollout
    names = ["L", "oval"]
    tabs = [np.array(tk.table(n)[0]) for n in names]
    ctx = standin_tracks.Context(_cfg(names), done=[1, 1])
    with pytest.raises(ValueError, match="one track"):
        rollout.LmpcGeneration(rollout.BatchedRollouts(ctx, tabs[0], prefetch=False, tracks=tabs), 2, K=1)
    rollout.LmpcGeneration(rollout.BatchedRollouts(ctx, tabs[0], prefetch=False, tracks=[tabs[1], tabs[1]]), 2, K=1)      # (two cars, one track)
    rollout.LmpcGeneration(rollout.BatchedRollouts(ctx, tabs[0], prefetch=False), 2, K=1)


def test_lap_from_global_counts_laps_with_each_cars_own_length():
    """The oracle's multi-lap PID runs on L and on the oval (320 rows: the oval car crosses the line at row 200, the L car at row 300), as one (T, 2, 6) log in the
    inertial frame (the forward map of each car's own track) through rollout.lap_from_global on the stand-in with one row per car: every car's curvilinear rows return within 1e-12 with s continuous past ITS
    TrackLength; with the other car's length the lap count would be wrong."""
    from racinglmpc_amd import rollout
    names = ["L", "oval"]
    TLs = tk.lengths_of(names)
    T = 320
    laps = [tk.pid_lap(n, steps=T) for n in names]
    assert all(l[0].shape == (T, 6) for l in laps) and all(l[0][-1, 4] > TL for l, TL in zip(laps, TLs)) and laps[0][0][-1, 4] < 2 * TLs[1]
    glob = [tk.global_lap(n, l[0]) for n, l in zip(names, laps)]                  # (the rows under the forward map of each car's own track)
    log = np.stack(glob, axis=1)
    ctx = standin_tracks.Context(_cfg(names))
    ctx.track_set(tk.rows_of(names))
    x = rollout.lap_from_global(ctx, log, tk.MAX_EY)
    assert x.shape == (T, 2, 6)
    for b in range(2):
        err = np.abs(x[:, b] - laps[b][0]).max(axis=0)
        print(names[b], "worst |x - oracle| per column", err)
        assert err.max() <= 1e-12 and np.all(np.diff(x[:, b, 4]) > 0) and x[-1, b, 4] > TLs[b]
    assert np.array_equal(rollout.lap_from_global(ctx, log, tk.MAX_EY, TL=TLs), x)
    # one (T, 6) lap on a context with one row per car names no car
    with pytest.raises((ValueError, standin_tracks.LmpcError)):
        rollout.lap_from_global(ctx, log[:, 0], tk.MAX_EY)
    # seed_lmpc(from_global=True, track_rows=...): lap i converted on track i, stored with the TrackLength of row i
    ctx2 = standin_tracks.Context(_cfg(names))
    ctx2.track_set(tk.rows_of(names))
    rollout.seed_lmpc(ctx2, [(glob[0], laps[0][1]), (glob[1][:250], laps[1][1][:250])], from_global=True, max_ey=tk.MAX_EY, track_rows=[0, 1])
    assert ctx2.SS[0].shape == (T, 6) and ctx2.SS[1].shape == (250, 6) and np.abs(ctx2.SS[1] - laps[1][0][:250]).max() <= 1e-12
    from oracle import lmpc_oracle as orc
    assert np.array_equal(ctx2.Qfun[1], orc.compute_cost(ctx2.SS[1], TLs[1])) and np.array_equal(ctx2.Qfun[0], orc.compute_cost(ctx2.SS[0], TLs[0]))
    assert ctx2.Qfun[1][0] != orc.compute_cost(ctx2.SS[1], TLs[0])[0]


def test_context_pool_fans_the_rows_out_to_every_member():
    from racinglmpc_amd import _capi
    seen = []
    pool = _capi.ContextPool.__new__(_capi.ContextPool)
    pool.members = [types.SimpleNamespace(track_set=lambda rows, i=i: seen.append(("set", i, rows)), tracks=lambda i=i: seen.append(("get", i)) or "rows of %d" % i)
                    for i in range(3)]
    pool._next = 0
    pool.track_set("rows")
    assert seen == [("set", i, "rows") for i in range(3)]
    del seen[:]
    assert pool.tracks() == "rows of 0" and seen == [("get", 0)]
