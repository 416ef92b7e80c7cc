"""CPU: lap metrics reduced on the device (lmpc_rollout_lap_metrics) -- the entry point's declaration and binding, tests/metrics_ref.py (the NumPy restatement of the
kernel, term order and reduction order included) against plain NumPy on synthetic logs, and rollout.PerCarLMPC(metrics=True) on the scripted stand-in context of
tests/test_device_commit_host.py.  What needs a device is in tests/test_gpu_lap_metrics.py."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import common, metrics_ref
from tests import test_device_commit_host as tdc
from tests.test_lap_table_host import _header_decl

EPS = 2.0 ** -52
ROWS = (1, 2, 255, 256, 257, 513)


def test_entry_point_is_exported_declared_and_bound(built):
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 112
    assert "lmpc_rollout_lap_metrics" in _capi.EXPORTS and lib.lmpc_rollout_lap_metrics.restype is C.c_int
    assert [a.rsplit(" ", 1)[0] for a in _header_decl("lmpc_rollout_lap_metrics")[1:]] == ["int", "const int *", "const int *", "double *"]
    assert lib.lmpc_rollout_lap_metrics.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    with open(common.ROOT + "/include/lmpc_hip.h") as f:
        text = f.read()
    assert int(re.search(r"#define LMPC_METRICS_NCOL (\d+)", text).group(1)) == _capi.METRICS_NCOL == len(_capi.METRIC_FIELDS) == metrics_ref.NCOL
    for name, col in _capi.METRIC_FIELDS.items():                                                   # every column has its enumerator, in this order
        assert re.search(r"\bLMPC_MET_%s = %d\b" % (name.upper(), col), text), name
    assert sorted(_capi.METRIC_FIELDS.values()) == list(range(_capi.METRICS_NCOL))
    cars = np.zeros(1, np.int32); out = np.full(_capi.METRICS_NCOL, 7.0)
    assert lib.lmpc_rollout_lap_metrics(None, 1, cars.ctypes.data, None, out.ctypes.data) == -1 and (out == 7.0).all()
    assert callable(_capi.Context.rollout_lap_metrics)


def _logs(T, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, 6)) * np.array([0.3, 0.1, 0.5, 0.1, 0.0, 0.2]) + np.array([1.0, 0, 0, 0, 0, 0])
    X[:, 4] = np.cumsum(0.1 * np.abs(X[:, 0]))
    U = rng.standard_normal((T, 2)) * np.array([0.2, 0.8])
    G = np.cumsum(rng.standard_normal((T, 6)) * 0.1, axis=0)
    return X, U, G


def _weights(seed, bx=(0.4, 0.4)):
    rng = np.random.default_rng(100 + seed)
    M = rng.standard_normal((6, 6)); Q = M @ M.T; Q = (Q + Q.T) / 2
    return metrics_ref.weights(Q, [[1.5, 0.25], [0.25, 3.0]], [0.8, 0, 0, 0, 0, 0.05], bx, [0.5, 0.5, 10.0, 10.0])


FX = np.zeros((2, 6)); FX[0, 5] = 1.0; FX[1, 5] = -1.0
FU = np.array([[1.0, 0], [-1, 0], [0, 1], [0, -1]])


SUMS = {"vx_sum": metrics_ref.S_VX, "lane_excess_sum": metrics_ref.S_LE, "lane_excess_sqsum": metrics_ref.S_LE2, "du0_sqsum": metrics_ref.S_DU0, "du1_sqsum": metrics_ref.S_DU1,
        "cost_state": metrics_ref.S_CX, "cost_input": metrics_ref.S_CU, "path_length": metrics_ref.S_PATH}


def _plain(X, U, G, T, w, TL, fin_s):
    """The columns from plain NumPy: np.sum / np.nanmax / matrix products, no stated order.  Returns the values and, for every sum, sum |term|."""
    from racinglmpc_amd._capi import METRIC_FIELDS as F
    X, U, G = X[:T], U[:T], G[:T]
    out, mag = np.zeros(metrics_ref.NCOL), {}
    with np.errstate(all="ignore"), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        out[F["rows"]] = T
        out[F["t_cross"]] = np.nan if fin_s is None else (T - 1) + (TL - X[-1, 4]) / (fin_s - X[-1, 4])
        out[F["nonfinite_rows"]] = np.count_nonzero(~np.isfinite(np.concatenate([X, U, G], axis=1)).all(axis=1))
        out[F["vx_min"]], out[F["vx_max"]] = np.nanmin(X[:, 0]), np.nanmax(X[:, 0])
        out[F["ey_absmax"]], out[F["ey_absmax_row"]] = np.nanmax(np.abs(X[:, 5])), np.nanargmax(np.abs(X[:, 5]))
        out[F["epsi_absmax"]], out[F["alat_absmax"]] = np.nanmax(np.abs(X[:, 3])), np.nanmax(np.abs(X[:, 0] * X[:, 2]))
        v = np.maximum(0.0, X @ FX.T - w["bx"])
        out[F["lane_excess_max"]], out[F["lane_excess_rows"]] = np.nanmax(v), np.count_nonzero((v > 0).any(axis=1))
        out[F["input_margin_min"]] = np.nanmin(w["bu"] - U @ FU.T)
        # the sums: np.sum over the restatement's own per-row terms (the terms themselves are checked against matrix forms in test_row_terms_against_matrix_forms)
        terms = metrics_ref.row_terms(np.ascontiguousarray(X), np.ascontiguousarray(U), np.ascontiguousarray(G), w, FX, FU)["sum"]
        for k, col in SUMS.items():
            out[F[k]] = np.sum(terms[:, col]); mag[k] = np.sum(np.abs(terms[:, col]))
    return out, mag


@pytest.mark.parametrize("T", ROWS)
@pytest.mark.parametrize("case", ["plain", "tie", "nan_row", "zero_width_lane"])
def test_restatement_against_plain_numpy(T, case):
    """Extremes, counts and the argmax are equal; every sum is within T * 2^-52 * sum |term| of np.sum, the bound of a summation in any order ((T - 1) * 2^-53) with
    a factor 4 of margin."""
    from racinglmpc_amd._capi import METRIC_FIELDS as F
    X, U, G = _logs(T + 5, T)
    w = _weights(T, bx=(0.0, 0.0) if case == "zero_width_lane" else (0.15, 0.15))
    done = T if case != "tie" else T + 3                                                           # "tie": the entry does not end at the crossing step
    TL, fin_s = X[T - 1, 4] + 0.04, (X[T - 1, 4] + 0.1 if done == T else None)
    if case == "tie" and T > 270:
        X[:, 5] = np.clip(X[:, 5], -0.5, 0.5); X[260, 5] = 0.75; X[10, 5] = -0.75; X[300, 5] = 0.75   # row 260 sits in a lower lane than row 10: the lower ROW wins
    elif case == "tie" and T >= 2:
        X[:T, 5] = 0.25; X[0, 5] = -0.25
    if case == "nan_row" and T >= 2:
        X[1, 0] = np.nan
    got = metrics_ref.lap_metrics(X, U, G, T, w, FX, FU, TL, fin_s)
    want, mag = _plain(X, U, G, T, w, TL, fin_s)
    exact = ["rows", "nonfinite_rows", "vx_min", "vx_max", "ey_absmax", "ey_absmax_row", "epsi_absmax", "alat_absmax", "lane_excess_max", "lane_excess_rows", "input_margin_min"]
    for k in exact:
        assert got[F[k]] == want[F[k]], (k, got[F[k]], want[F[k]])
    for k, m in mag.items():
        if np.isnan(want[F[k]]):
            assert np.isnan(got[F[k]]), k
        else:
            assert abs(got[F[k]] - want[F[k]]) <= T * EPS * m, (k, got[F[k]], want[F[k]], T * EPS * m)
    if done == T:
        assert got[F["t_cross"]] == want[F["t_cross"]] and T - 1 < got[F["t_cross"]] < T
    else:
        assert np.array([got[F["t_cross"]]]).view(np.int64)[0] == 0x7ff8000000000000
    if case == "tie":
        assert got[F["ey_absmax_row"]] == (10 if T > 270 else 0)
    if case == "nan_row" and T >= 2:
        assert got[F["nonfinite_rows"]] == 1 and np.isnan(got[F["vx_sum"]]) and np.isnan(got[F["cost_state"]]) and np.isfinite(got[F["cost_input"]])
    if case == "zero_width_lane":
        assert got[F["lane_excess_rows"]] == np.count_nonzero(X[:T, 5]) and got[F["lane_excess_max"]] == got[F["ey_absmax"]] and got[F["lane_excess_sum"]] > 0
    if T == 1:
        assert got[F["du0_sqsum"]] == 0 and got[F["du1_sqsum"]] == 0 and got[F["path_length"]] == 0


def test_row_terms_against_matrix_forms():
    """The per-row terms the sums run over, against einsum / diff / hypot: a row's term is a sum of at most 42 products, so two evaluation orders differ by at most
    42 roundings of 2^-53 relative to the sum of the products' magnitudes (taken as 2^-52 times that sum times 42: a factor 2 of margin); hypot against
    sqrt(dX dX + dY dY) is within 2 ulp."""
    T = 300
    X, U, G = _logs(T, 9)
    w = _weights(9, bx=(0.05, 0.05))
    t = metrics_ref.row_terms(X, U, G, w, FX, FU)["sum"]
    e = X - w["xRef"]
    v = np.maximum(0.0, X @ FX.T - w["bx"])
    dU, dG = np.diff(U, axis=0), np.diff(G[:, 4:6], axis=0)
    want = {metrics_ref.S_VX: (X[:, 0], np.abs(X[:, 0]) * 0), metrics_ref.S_LE: (v.sum(axis=1), v.sum(axis=1)), metrics_ref.S_LE2: ((v * v).sum(axis=1), (v * v).sum(axis=1)),
            metrics_ref.S_CX: (np.einsum("ti,ij,tj->t", e, w["Q"], e), np.einsum("ti,ij,tj->t", np.abs(e), np.abs(w["Q"]), np.abs(e))),
            metrics_ref.S_CU: (np.einsum("ti,ij,tj->t", U, w["R"], U), np.einsum("ti,ij,tj->t", np.abs(U), np.abs(w["R"]), np.abs(U)))}
    for col, (val, mag) in want.items():
        assert (np.abs(t[:, col] - val) <= 42 * EPS * mag).all(), col
    assert (v > 0).any() and t[0, metrics_ref.S_DU0] == 0 and t[0, metrics_ref.S_DU1] == 0 and t[0, metrics_ref.S_PATH] == 0
    assert np.array_equal(t[1:, metrics_ref.S_DU0], dU[:, 0] * dU[:, 0]) and np.array_equal(t[1:, metrics_ref.S_DU1], dU[:, 1] * dU[:, 1])
    h = np.hypot(dG[:, 0], dG[:, 1])
    assert (np.abs(t[1:, metrics_ref.S_PATH] - h) <= 2 * np.spacing(h)).all()


def test_the_reduction_is_the_stated_tree():
    """The fold the restatement performs, spelled out thread by thread in Python floats for one sum and T = 513."""
    T = 513
    X, U, G = _logs(T, 3)
    w = _weights(3)
    term = metrics_ref.row_terms(X, U, G, w, FX, FU)["sum"][:, metrics_ref.S_CX]
    lanes = []
    for k in range(256):
        acc = 0.0
        for t in range(k, T, 256):
            acc = acc + float(term[t])
        lanes.append(acc)
    waves = []
    for wv in range(4):
        v = lanes[64 * wv:64 * wv + 64]
        off = 1
        while off < 64:
            v = [v[l] + v[l + off] if l + off < 64 else v[l] for l in range(64)]
            off *= 2
        waves.append(v[0])
    want = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    from racinglmpc_amd._capi import METRIC_FIELDS as F
    assert metrics_ref.lap_metrics(X, U, G, T, w, FX, FU, 1.0)[F["cost_state"]] == want


class _MetricsCtx(tdc._LoopCtx):
    """The scripted context with the metrics call: it records the cars listed and answers rows whose first column is the car's crossing step."""

    def __init__(self, *args):
        super().__init__(*args)
        self.metric_calls = []

    def rollout_lap_metrics(self, cars, rows=None):
        from racinglmpc_amd import _capi
        assert rows is None and len(cars) >= 1 and list(cars) == sorted(set(cars))
        self.metric_calls.append((self.gen, [int(b) for b in cars], len(self.ss)))
        done = self.script[self.gen][0]
        out = np.zeros((len(cars), _capi.METRICS_NCOL))
        out[:, 0] = [done[b] for b in cars]; out[:, 1] = [100 * self.gen + b for b in cars]
        return out


def _run_metrics(device_commit):
    from racinglmpc_amd import rollout
    ctx = _MetricsCtx(3, 2, tdc.SCRIPT, ())
    track = np.array(common.load_lmpc_golden()["track"])
    ro = rollout.BatchedRollouts(ctx, track, seed=1, prefetch=False)
    loop = rollout.PerCarLMPC(ro, T_max=60, ext=10, device_commit=device_commit, metrics=True)
    lap = lambda T, ends: (np.zeros((T, 6)), np.zeros((T, 2)), None, np.zeros(12), T if ends else T - 20, 0)
    loop.seed([lap(50, True), [lap(70, True), lap(60, True)], lap(80, False), [lap(90, False)]])      # (the seeds of tdc._run)
    gens = []
    for _ in range(len(tdc.SCRIPT)):
        out = loop.run()
        gens.append(dict(out=out, ss_table=ro.ss_table.tolist(), ss_last=ro.ss_last.tolist(), lap_table=ro.lap_table.tolist(), retired=dict(loop.retired),
                         lap_times=[list(t) for t in loop.lap_times]))
    return ctx, loop, gens


@pytest.mark.parametrize("device_commit", [False, True], ids=["host_loop", "device_commit"])
def test_per_car_lmpc_metrics_on_the_scripted_context(device_commit):
    """metrics[g] has values for exactly the valid cars of generation g and NaN rows for the others; one call per generation with a valid car, made before the laps
    of that generation are stored; histories, tables, lap_times, retired and the returned tuples are those of the run with metrics=False."""
    from racinglmpc_amd import _capi
    pc, pl, pg = tdc._run(device_commit)
    mc, ml, mg = _run_metrics(device_commit)
    assert pl.metrics == [] and len(ml.metrics) == len(tdc.SCRIPT)
    for gen, (p, m) in enumerate(zip(pg, mg)):
        for k in ("ss_table", "ss_last", "lap_table", "retired", "lap_times"):
            assert p[k] == m[k], (gen, k)
        assert [o is None for o in p["out"]] == [o is None for o in m["out"]]
        for po, mo in zip(p["out"], m["out"]):
            if po is not None:
                assert po[4:] == mo[4:] and np.array_equal(po[0], mo[0]) and np.array_equal(po[1], mo[1]) and np.array_equal(po[3], mo[3])
        valid = [b for b, o in enumerate(m["out"]) if o is not None]
        M = ml.metrics[gen]
        assert M.shape == (4, _capi.METRICS_NCOL)
        for b in range(4):
            if b in valid:
                assert M[b, 0] == tdc.SCRIPT[gen][0][b] and M[b, 1] == 100 * gen + b and not np.isnan(M[b]).any()
            else:
                assert np.isnan(M[b]).all(), (gen, b)
    assert pc.ss == mc.ss and pc.model == mc.model and pc.rows == mc.rows and pc.extended == mc.extended and pc.fetched == mc.fetched
    stored = 5                                                                                      # the seed laps
    for gen, m in enumerate(mg):
        valid = [b for b, o in enumerate(m["out"]) if o is not None]
        calls = [c for c in mc.metric_calls if c[0] == gen]
        assert calls == ([(gen, valid, stored)] if valid else []), (gen, calls, valid)             # (taken before the generation's laps enter the stores)
        stored += len(valid)
    assert [v for g_, v, _ in mc.metric_calls] == [[0, 1, 2, 3], [0, 1, 3], [0], [0]]


def test_both_paths_list_the_same_cars():
    hc, _, _ = _run_metrics(False)
    dc, _, _ = _run_metrics(True)
    assert hc.metric_calls == dc.metric_calls and len(hc.metric_calls) == 4
