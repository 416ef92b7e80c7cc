"""CPU: per-car controller tuning (lmpc_tuning_from_config / lmpc_tuning_set / lmpc_tuning_get) -- the symbols, their declaration and binding, the row builder and
row check of the Python layer, the hand-over by BatchedRollouts / PerCarLMPC / ContextPool, and the oracle facts about the rows of tests/tuning_cases.py that every
tolerance of tests/test_gpu_tuning.py rests on.  What needs a context on a device is in tests/test_gpu_tuning.py."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import common
from tests import standin_capi
from tests import tuning_cases as tc
from tests.test_lap_table_host import _header_decl

NEW = ("lmpc_tuning_from_config", "lmpc_tuning_set", "lmpc_tuning_get")


def test_entry_points_are_exported_declared_and_bound(built):
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 108
    for name in NEW:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    d = _header_decl("lmpc_tuning_from_config")
    assert d is not None and d[0] == "const lmpc_config *" and d[1].rsplit(" ", 1)[0] == "double *", d
    d = _header_decl("lmpc_tuning_set")
    assert d is not None and [a.rsplit(" ", 1)[0] for a in d[1:]] == ["int", "const double *"], d
    d = _header_decl("lmpc_tuning_get")
    assert d is not None and [a.rsplit(" ", 1)[0] for a in d[1:]] == ["int *", "double *", "int"], d
    assert lib.lmpc_tuning_set.argtypes == [C.c_void_p, C.c_int, C.c_void_p]
    assert lib.lmpc_tuning_get.argtypes == [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]
    n = C.c_int(7); rows = np.zeros(98)
    assert lib.lmpc_tuning_set(None, 1, rows.ctypes.data) == -1 and lib.lmpc_tuning_set(None, 0, None) == -1
    assert lib.lmpc_tuning_get(None, C.byref(n), None, 0) == -1 and n.value == 7
    assert lib.lmpc_tuning_from_config(None, rows.ctypes.data) == -1
    with open(common.ROOT + "/include/lmpc_hip.h") as f:
        text = " ".join(f.read().split())
    assert "#define LMPC_TUNING_NPAR 98" in text and _capi.TUNING_NPAR == 98
    assert "LMPC_FUSE=1" in text and "LMPC_CD=1" in text and "NEITHER the fused one-wave step" in text
    for meth in ("tuning_set", "tuning"):
        assert callable(getattr(_capi.Context, meth)), meth


def test_from_config_is_the_row_of_the_python_builder(built):
    """lmpc_tuning_from_config(lmpc_config_default) equals tuning_rows(cfg, 1), and every field sits in its TUNING_FIELDS slice -- on the default config and on one
    whose fields are all distinct numbers."""
    from racinglmpc_amd import _capi
    lib = _capi.load()
    sl = _capi.TUNING_FIELDS
    assert list(sl) == ["Q", "R", "Qf", "dR", "Qslack", "QtermSlack", "xRef", "bx", "bu"]
    assert [(s.start, s.stop) for s in sl.values()] == [(0, 36), (36, 40), (40, 76), (76, 78), (78, 80), (80, 86), (86, 92), (92, 94), (94, 98)]
    cfg = _capi.default_config()
    row = np.full(98, np.nan)
    assert lib.lmpc_tuning_from_config(C.byref(cfg), row.ctypes.data) == 0
    assert np.array_equal(row, _capi.tuning_rows(cfg, 1)[0])
    assert row[sl["dR"]].tolist() == [5.0, 50.0] and row[sl["Qslack"]].tolist() == [5.0, 25.0] and row[sl["QtermSlack"]].tolist() == [500.0] * 6
    assert row[sl["bx"]].tolist() == [0.4, 0.4] and row[sl["bu"]].tolist() == [0.5, 0.5, 10.0, 10.0] and not row[sl["Q"]].any()
    rng = np.random.default_rng(5)
    Q = rng.random((6, 6)); Q = Q + Q.T; Qf = rng.random((6, 6)); Qf = Qf + Qf.T; R = np.array([[1.5, 0.25], [0.25, 2.5]])
    par = types.SimpleNamespace(Q=Q, R=R, Qf=Qf, dR=[3.0, 4.0], Qslack=[6.0, 7.0], QterminalSlack=np.diag([11.0, 12, 13, 14, 15, 16]), xRef=np.arange(21.0, 27.0),
                                bx=[0.31, 0.32], bu=[0.41, 0.42, 0.43, 0.44])
    cfg = _capi.config_from(12, Q, R, Qf, par.dR, par.Qslack, np.zeros((2, 6)), par.bx, np.zeros((4, 2)), par.bu, par.xRef, QterminalSlack=par.QterminalSlack,
                            numSS_Points=48, numSS_it=4, trToUse=4)
    assert lib.lmpc_tuning_from_config(C.byref(cfg), row.ctypes.data) == 0
    assert np.array_equal(row, _capi.tuning_rows(cfg, 1)[0]) and np.array_equal(row, tc.row_of(par))
    for name, want in (("Q", Q.ravel()), ("R", R.ravel()), ("Qf", Qf.ravel()), ("dR", par.dR), ("Qslack", par.Qslack), ("QtermSlack", np.arange(11.0, 17.0)),
                       ("xRef", par.xRef), ("bx", par.bx), ("bu", par.bu)):
        assert np.array_equal(row[sl[name]], np.asarray(want, float)), name


def test_row_builder_broadcasts_and_validates(built):
    """tuning_rows: a scalar, an array for every car, an array with a leading B axis; a full diagonal 6 x 6 QterminalSlack; refusals."""
    from racinglmpc_amd import _capi
    sl = _capi.TUNING_FIELDS
    cfg, _ = common.lmpc_config(common.load_lmpc_golden(), 12)
    B = 3
    r = _capi.tuning_rows(cfg, B)
    assert r.shape == (B, 98) and r.dtype == np.float64 and r.flags["C_CONTIGUOUS"] and (r == r[0]).all()
    qs = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    r = _capi.tuning_rows(cfg, B, dR=[1.0, 10.0], Qslack=qs, xRef=0.5, QterminalSlack=100.0 * np.eye(6), Q=np.diag([0, 0, 0, 0, 0, 10.0]))
    assert np.array_equal(r[:, sl["dR"]], np.tile([1.0, 10.0], (B, 1))) and np.array_equal(r[:, sl["Qslack"]], qs)
    assert (r[:, sl["xRef"]] == 0.5).all() and (r[:, sl["QtermSlack"]] == 100.0).all() and np.array_equal(r[1, sl["Q"]].reshape(6, 6), np.diag([0, 0, 0, 0, 0, 10.0]))
    assert np.array_equal(r[:, sl["bu"]], np.tile([0.5, 0.5, 10.0, 10.0], (B, 1)))              # (untouched fields keep the config's values)
    T = np.stack([k * np.eye(6) for k in (1.0, 2.0, 3.0)])
    assert np.array_equal(_capi.tuning_rows(cfg, B, QterminalSlack=T)[:, sl["QtermSlack"]], np.repeat([[1.0], [2.0], [3.0]], 6, axis=1))
    # B = 6: a (6, 6) array is six per-car DIAGONALS under QtermSlack and one MATRIX under QterminalSlack -- never guessed
    D6 = np.arange(1.0, 37.0).reshape(6, 6)
    assert np.array_equal(_capi.tuning_rows(cfg, 6, QtermSlack=D6)[:, sl["QtermSlack"]], D6)
    assert np.array_equal(_capi.tuning_rows(cfg, 6, QterminalSlack=np.diag(D6[0]))[:, sl["QtermSlack"]], np.tile(D6[0], (6, 1)))
    for bad in (dict(QterminalSlack=D6), dict(QterminalSlack=D6[0]), dict(QtermSlack=T)):
        with pytest.raises(ValueError):
            _capi.tuning_rows(cfg, 6 if "QterminalSlack" in bad else B, **bad)
    assert np.array_equal(_capi.tuning_rows(cfg, B, QtermSlack=[1, 2, 3, 4, 5, 6.0])[2, sl["QtermSlack"]], np.arange(1.0, 7.0))
    assert np.array_equal(_capi.tuning_rows(cfg, 1, bu=[0.0, 0.5, 10, 10])[0, sl["bu"]], [0.0, 0.5, 10, 10])      # (bu <= 0 is the kernels' business: NOT_INTERIOR)
    off = 100.0 * np.eye(6); off[0, 1] = 1.0
    Qn = np.zeros((6, 6)); Qn[0, 1] = 1.0
    for bad in (dict(QterminalSlack=off), dict(Q=Qn), dict(Qf=Qn), dict(R=[[1.0, 0.5], [0.0, 1.0]]), dict(Qslack=np.ones((B + 1, 2))), dict(dR=np.ones((B + 1, 2))),
                dict(dR=[-1.0, 1.0]), dict(Qslack=[1.0, -1.0]), dict(QtermSlack=[1, 1, 1, 0, 1, 1.0]), dict(xRef=[np.nan] * 6), dict(bx=[1.0, 2.0, 3.0]), dict(nope=1.0)):
        with pytest.raises(ValueError):
            _capi.tuning_rows(cfg, B, **bad)
    with pytest.raises(ValueError):
        _capi.tuning_rows(cfg, 0)
    assert _capi.check_tuning(None) is None and _capi.check_tuning(np.zeros((0, 98))) is None
    with pytest.raises(ValueError):
        _capi.check_tuning(np.zeros((2, 97)))
    mpc, _ = common.mpc_config(common.load_lmpc_golden(), 12)
    assert _capi.tuning_rows(mpc, 2, xRef=[[0.6, 0, 0, 0, 0, 0], [1.0, 0, 0, 0, 0, 0]])[:, sl["xRef"]][:, 0].tolist() == [0.6, 1.0]      # (no terminal set: QtermSlack = 0 is no error)


def test_oracle_facts_of_the_rows():
    """The facts of tests/tuning_cases.py re-derived on 6 of its 12 problems (stores of LMPC lap 4, no previous prediction): every QP of every row certified to
    <= 1e-9 by the oracle, and the optima of two rows at least the recorded distance, halved, apart -- so a wrong row shows at more than 100 x TOL_XU wherever the
    GPU tests compare outputs (the smallest: R5b against R5a, one Qslack entry).  The rows of the batches also end clean in the NumPy model of the kernels' iteration."""
    try:
        from threadpoolctl import threadpool_limits
        lim = threadpool_limits(1)
    except Exception:                                 # noqa: BLE001
        lim = None
    g = common.load_lmpc_golden()
    idx = range(0, tc.NPROB, 2)
    try:
        res = tc.study(g, which=("lap4",), idx=idx, model=False)
        mod = tc.study(g, names=tc.SIX, which=("lap4",), idx=idx, model=True)
    finally:
        if lim is not None and hasattr(lim, "restore_original_limits"):
            lim.restore_original_limits()
    print("worst certificate %.2e; distances %s" % (res["cert"], {k: "%.3e" % v for k, v in sorted(res["dist"].items())}))
    assert res["cert"] <= 1e-9, res["cert"]
    assert set(res["dist"]) == set(tc.DIST_MEASURED)
    for pair, d in res["dist"].items():
        assert d >= 0.5 * tc.DIST_MEASURED[pair], (pair, d, tc.DIST_MEASURED[pair])
        assert tc.DIST_MEASURED[pair] > 100 * common.TOL_XU, pair
    assert tc.DIST_MEASURED[("RQf", "R0")] >= 1e-4
    for name, (row, against) in tc.FIELD_ROWS.items():
        assert (row, against) in tc.DIST_MEASURED, name
    assert not mod["not_converged"], mod["not_converged"]
    assert all(hi < 40 for lo, hi in mod["iters"].values())


class _Ctx(standin_capi.Context):
    """The stand-in context with the session entry points and the per-car settings: records the calls in order."""

    def model_set_lap_table(self, rows):
        standin_capi._rec("model_set_lap_table", None)

    def ss_set_lap_table(self, rows, last=None):
        standin_capi._rec("ss_set_lap_table", None)

    def tuning_set(self, rows):
        standin_capi._rec("tuning_set", np.array(rows))

    def rollout_begin(self, x0, xglob0, xLin0, uLin0, noise):
        standin_capi._rec("rollout_begin", None)

    def rollout_begin_mpc(self, x0, xglob0, noise, **kw):
        standin_capi._rec("rollout_begin_mpc", None)

    def rollout_run(self, n):
        return 1, 0

    def rollout_fetch(self, t0, t1):
        B = 3
        return np.zeros((1, B, 6)), np.zeros((1, B, 2)), np.zeros((1, B, 6)), np.full(B, -1, np.int32), np.zeros(B, np.int32), np.zeros((B, 6)), np.zeros((B, 6))

    def rollout_end(self):
        pass


def test_rollouts_hand_the_rows_to_the_context_before_begin(built):
    """BatchedRollouts(tuning=): Context.tuning_set(rows) before every rollout_begin, behind the tables, and before rollout_begin_mpc; without rows the context is
    not touched; a row count that is neither 1 nor the number of cars is refused before the session begins; PerCarLMPC(tuning=) hands the rows to its rollouts."""
    from racinglmpc_amd import rollout, _capi
    g = common.load_lmpc_golden()
    track = np.array(g["track"])
    B = 3
    real, _ = common.lmpc_config(g, 12)
    rows = _capi.tuning_rows(real, B, dR=np.array([[1.0, 10.0], [5.0, 50.0], [20.0, 200.0]]))
    cfg = types.SimpleNamespace(N=12, numSS_it=2, numSS_points=24, trToUse=2, par=None, track=track, trackLength=float(g["trackLength"]))
    x0 = np.zeros((B, 6))
    keep = ("model_set_lap_table", "ss_set_lap_table", "tuning_set", "rollout_begin", "rollout_begin_mpc")

    def calls(f):
        n0 = len(standin_capi.CALLS)
        f()
        return [c for c in standin_capi.CALLS[n0:] if c[0] in keep]
    for tab in (rows, rows[:1]):
        ro = rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False, lap_table=[[0, 1]], ss_table=[[0, 1]], tuning=tab)
        for _ in range(2):
            got = calls(lambda: ro.begin(x0, np.zeros((13, 6)), np.zeros((12, 2)), max_steps=5))
            assert [c[0] for c in got] == ["model_set_lap_table", "ss_set_lap_table", "tuning_set", "rollout_begin"]
            assert np.array_equal(got[2][1], tab) and got[2][1].dtype == np.float64
        got = calls(lambda: ro.run_mpc_laps(x0, A=np.zeros((B, 6, 6)), B=np.zeros((B, 6, 2)), max_steps=5, keep_invalid=True))
        assert [c[0] for c in got] == ["tuning_set", "rollout_begin_mpc"]
    ro = rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False)
    assert [c[0] for c in calls(lambda: ro.begin(x0, np.zeros((13, 6)), np.zeros((12, 2)), max_steps=5))] == ["rollout_begin"]
    ro = rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False, tuning=rows[:2])
    n0 = len(standin_capi.CALLS)
    with pytest.raises(ValueError):
        ro.begin(x0, np.zeros((13, 6)), np.zeros((12, 2)), max_steps=5)
    assert not [c for c in standin_capi.CALLS[n0:] if c[0] in ("tuning_set", "rollout_begin")]
    with pytest.raises(ValueError):
        rollout.BatchedRollouts(_Ctx(cfg), track, tuning=np.zeros((B, 97)))
    ro = rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False)
    loop = rollout.PerCarLMPC(ro, T_max=60, ext=10, device_commit=True, tuning=rows)
    assert np.array_equal(ro.tuning, rows) and loop.ro is ro
    import inspect
    assert "tuning" in inspect.signature(rollout.bootstrap).parameters
    assert "not saved" in _capi.Context.save_stores.__doc__ and "controller parameters" in _capi.Context.save_stores.__doc__


def test_context_pool_fans_the_rows_out_to_every_member():
    from racinglmpc_amd import _capi
    seen = []
    pool = _capi.ContextPool.__new__(_capi.ContextPool)
    pool.members = [types.SimpleNamespace(tuning_set=lambda rows, i=i: seen.append(("set", i, rows)), tuning=lambda i=i: seen.append(("get", i)) or "rows of %d" % i)
                    for i in range(3)]
    pool._next = 0
    pool.tuning_set("rows")
    assert seen == [("set", i, "rows") for i in range(3)]
    del seen[:]
    assert pool.tuning() == "rows of 0" and seen == [("get", 0)]
