"""-m gpu: lap metrics of a rollout session reduced on the device (lmpc_rollout_lap_metrics; rollout.PerCarLMPC(metrics=True)).

The reference of every case is tests/metrics_ref.py -- the kernel's terms and its reduction order restated in NumPy -- on the logs the same session returns through
rollout_fetch.  Results are compared bit for bit, as int64 words: every column, path_length (a device sqrt per row) and t_cross (a device division) included.
PID sessions are one launch; N = 12.  What needs no device is in tests/test_lap_metrics_host.py."""
import ctypes as C

import numpy as np
import pytest

from tests import common, metrics_ref, track_cases
from tests.test_gpu_device_commit import _pid, _refused, _same, _same_stores, _stores, E_ARG, E_STATE

pytestmark = pytest.mark.gpu

N = 12
VT = [0.7, 0.75, 0.8, 0.85, 0.9]
CARS, ROWS = [0, 1, 2, 3, 4, 4, 0], [1, 2, 255, 256, 257, 513, 513]          # every boundary of the 256-row fold; cars 4 and 0 listed twice


@pytest.fixture(scope="module")
def g():
    return common.load_lmpc_golden()


def _fxfu(cfg):
    return np.array(list(cfg.Fx)).reshape(2, 6), np.array(list(cfg.Fu)).reshape(4, 2)


def _ref(ctx, cfg, t, cars, rows, weights_of=None, TL_of=None):
    """metrics_ref on the fetched logs of the active session (t steps taken)."""
    X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
    Fx, Fu = _fxfu(cfg)
    w = metrics_ref.weights_of_config(cfg)
    return metrics_ref.session_metrics(X, U, G, done, fx, cars, rows, weights_of or (lambda c: w), Fx, Fu, TL_of or (lambda c: float(cfg.trackLength))), done


def _check_boundaries(ctx, cfg, t, weights_of=None, TL_of=None):
    from racinglmpc_amd._capi import METRIC_FIELDS as F
    got = ctx.rollout_lap_metrics(CARS, ROWS)
    want, done = _ref(ctx, cfg, t, CARS, ROWS, weights_of, TL_of)
    assert (done >= 0).all() and (done < t).all(), done
    for k, col in F.items():
        _same(got[:, col], want[:, col], ("explicit rows", k, got[:, col], want[:, col]))
    assert got[:, F["rows"]].tolist() == ROWS and (got[:, F["nonfinite_rows"]] == 0).all()
    assert (np.isnan(got[:, F["t_cross"]]) == (np.array(ROWS) != done[CARS])).all()               # t_cross exists only for an entry that ends at the crossing step
    assert got[0, F["du0_sqsum"]] == 0 and got[0, F["path_length"]] == 0 and got[1, F["path_length"]] > 0
    cars = [4, 3, 2, 1, 0]
    got2 = ctx.rollout_lap_metrics(cars)                                      # rows = None: up to each car's crossing step
    want2, _ = _ref(ctx, cfg, t, cars, None, weights_of, TL_of)
    for k, col in F.items():
        _same(got2[:, col], want2[:, col], ("rows=None", k, got2[:, col], want2[:, col]))
    assert got2[:, F["rows"]].tolist() == done[cars].tolist()
    tc = got2[:, F["t_cross"]]
    assert ((tc > done[cars] - 1) & (tc <= done[cars])).all(), (tc, done)     # the line lies between the last logged row and the state behind it
    return got, got2


def test_every_boundary_of_the_fold_bit_for_bit(built, g):
    """One PID session, B = 5, 600 steps, not stopping at the line: entries of 1, 2, 255, 256, 257 and 513 rows, two cars listed twice, one rows=None pass; the stores
    of a context that holds a lap are the same before and after (the call reads only)."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=4, max_lap_len=512)
    with _capi.Context(cfg) as A:
        xs, us = np.array(g["xPID"])[:100], np.array(g["uPID"])[:100]
        A.ss_add_trajectory(xs, us); A.model_add_trajectory(xs, us)
        before = _stores(A)
        t = _pid(A, VT, 600, False)
        assert t == 600
        got, got2 = _check_boundaries(A, cfg, t)
        again = A.rollout_lap_metrics(CARS, ROWS)
        _same(again, got, "the same call twice")
        A.rollout_end()
        _same_stores(_stores(A), before, "stores after the metrics calls")
        assert A.ss_num_laps() == 1 and A.model_num_laps() == 1


def test_per_car_tracks_and_tuning_rows(built, g):
    """The boundary case with two of the reference's tracks dealt over the cars and one tuning row per car: non-zero Q, R, xRef, and car 3 with bx = 0.01, whose
    lane-excess columns are then non-zero."""
    from racinglmpc_amd import _capi
    from racinglmpc_amd._capi import METRIC_FIELDS as F
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=4, max_lap_len=512)
    names = track_cases.deal(5, ("L", "oval"))
    rng = np.random.default_rng(4)
    M = rng.standard_normal((5, 6, 6)); Q = M @ M.transpose(0, 2, 1); Q = (Q + Q.transpose(0, 2, 1)) / 2
    R = np.tile(np.array([[1.5, 0.25], [0.25, 3.0]]), (5, 1, 1)) * (1 + np.arange(5))[:, None, None]
    xRef = np.tile(np.array([0.8, 0, 0, 0, 0, 0.05]), (5, 1)); xRef[:, 0] = VT
    bx = np.tile(np.array([0.4, 0.4]), (5, 1)); bx[3] = 0.01
    tune = _capi.tuning_rows(cfg, 5, Q=Q, R=R, xRef=xRef, bx=bx)
    TLs = track_cases.lengths_of(names)
    with _capi.Context(cfg) as A:
        A.track_set(track_cases.rows_of(names)); A.tuning_set(tune)
        t = _pid(A, VT, 600, False)
        got, got2 = _check_boundaries(A, cfg, t, lambda c: metrics_ref.weights_of_tuning_row(tune[c]), lambda c: float(TLs[c]))
        A.rollout_end()
    k3 = CARS.index(3)
    for name in ("lane_excess_max", "lane_excess_rows", "lane_excess_sum", "lane_excess_sqsum"):
        assert got[k3, F[name]] > 0, name
    others = [i for i, c in enumerate(CARS) if c != 3 and ROWS[i] > 2]
    assert (got[others, F["lane_excess_rows"]] == 0).all()
    assert (got[2:, F["cost_state"]] > 0).all() and (got[2:, F["cost_input"]] > 0).all()
    assert len(set(got2[:, F["cost_input"]].tolist())) == 5


def test_a_nan_car_touches_no_other_entry(built, g):
    """Car 1 starts with vx = NaN: every row of it counts as non-finite, and the rows of the other cars are those of the session without it."""
    from racinglmpc_amd import _capi
    from racinglmpc_amd._capi import METRIC_FIELDS as F
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=4, max_lap_len=128)
    vt = [0.7, 0.8, 0.9]
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (3, 1)); x0[1, 0] = np.nan
    cars, rows = [0, 1, 2, 1], [300, 300, 257, 1]
    with _capi.Context(cfg) as A:
        t = _pid(A, vt, 320, False, x0=x0)
        bad = A.rollout_lap_metrics(cars, rows)
        A.rollout_end()
        assert _pid(A, vt, 320, False) == t
        good = A.rollout_lap_metrics(cars, rows)
        A.rollout_end()
    assert bad[[1, 3], F["nonfinite_rows"]].tolist() == [300, 1] and bad[[0, 2], F["nonfinite_rows"]].tolist() == [0, 0]
    assert np.isnan(bad[1, F["vx_sum"]]) and bad[1, F["vx_max"]] == -np.inf and bad[1, F["vx_min"]] == np.inf      # (no comparable value: the identities)
    _same(bad[[0, 2]], good[[0, 2]], "the other cars")
    assert (good[:, F["nonfinite_rows"]] == 0).all()


def _raw(ctx, cars, rows):
    """The entry point itself on a caller's buffer: (return code, buffer untouched)."""
    cars = np.asarray(cars, np.int32); rows = None if rows is None else np.asarray(rows, np.int32)
    out = np.full((len(cars), 20), 7.0)
    rc = ctx.lib.lmpc_rollout_lap_metrics(ctx._h, len(cars), cars.ctypes.data, None if rows is None else rows.ctypes.data, out.ctypes.data)
    return rc, bool((out == 7.0).all()), ctx.lib.lmpc_last_error().decode()


def test_refusals_leave_out_untouched(built, g):
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=4, max_lap_len=128)
    with _capi.Context(cfg) as A:
        assert _raw(A, [0], [1])[:2] == (-4, True)                                                 # no session active
        _refused(E_STATE, lambda: A.rollout_lap_metrics([0], [1]))
        t = _pid(A, [0.9, 0.8, 0.45], 400, True)
        done = A.rollout_fetch(0, 0)[3]
        assert t == 400 and done[0] >= 0 and done[1] >= 0 and done[2] < 0, done
        rc, same, msg = _raw(A, [0, 1, 2], None)
        assert (rc, same) == (-4, True) and "car 2" in msg, msg                                    # has not crossed, no row count given
        for cars, rows in (([0, 2], [10, t + 1]),                                                  # beyond the steps taken
                           ([0, 1], [10, int(done[1]) + 1]),                                       # stop_at_line: a car is logged up to its crossing step only
                           ([0, 3], [10, 10]), ([0, -1], [10, 10]),                                # no such car
                           ([0, 1], [10, 0])):                                                     # no rows
            assert _raw(A, cars, rows)[:2] == (-1, True), (cars, rows)
        assert A.lib.lmpc_rollout_lap_metrics(A._h, 0, np.zeros(1, np.int32).ctypes.data, None, np.zeros(20).ctypes.data) == -1
        assert A.lib.lmpc_rollout_lap_metrics(A._h, 1, None, None, np.zeros(20).ctypes.data) == -1
        assert A.lib.lmpc_rollout_lap_metrics(A._h, 1, np.zeros(1, np.int32).ctypes.data, None, None) == -1
        _refused(E_ARG, lambda: A.rollout_lap_metrics([0, 1], [10, int(done[1]) + 1]))
        ok = A.rollout_lap_metrics([0, 1, 2], [int(done[0]), int(done[1]), t])                     # the most each car has
        assert ok[:, 0].tolist() == [done[0], done[1], t] and np.isnan(ok[2, 1]) and not np.isnan(ok[:2, 1]).any()
        A.rollout_end()
        assert _raw(A, [0], [1])[:2] == (-4, True)


def test_per_car_lmpc_metrics_equal_the_restatement_on_the_host_loops_laps(built, g):
    """One LMPC generation, 4 cars: PerCarLMPC(device_commit=True, park=True, metrics=True) against PerCarLMPC(metrics=False) on a second context, whose returned
    laps go through metrics_ref with finX from the tuples' final12.  Inside the first run's session, rows beyond a parked car's parking step are refused."""
    from racinglmpc_amd import _capi, rollout
    from racinglmpc_amd._capi import METRIC_FIELDS as F
    track = np.array(g["track"])
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=16, max_lap_len=1024)
    vt = np.array([0.75, 0.8, 0.85, 0.9])
    seen = {}
    ctxs = [_capi.Context(cfg), _capi.Context(cfg)]
    try:
        end = ctxs[0].rollout_end

        def end_after_a_refusal():
            at = ctxs[0].rollout_parked_at()[0]
            b = int(np.argmax(at >= 0))
            seen["at"] = at.copy()
            seen["refusal"] = _raw(ctxs[0], [b], [int(at[b]) + 1]) if at[b] >= 0 else None
            seen["inside"] = _raw(ctxs[0], [b], [int(at[b])])[0] if at[b] >= 0 else None
            return end()
        outs = []
        for ctx, dev in zip(ctxs, (True, False)):
            ro = rollout.BatchedRollouts(ctx, track, seed=5, device_noise=True)
            ro.noise_shard = (0, 4, 4)
            seeds = ro.run_pid_laps(vt, max_steps=700, keep_invalid=True)
            assert all(l[4] >= 0 and l[5] == 0 for l in seeds)
            loop = rollout.PerCarLMPC(ro, T_max=400, ext=40, device_commit=dev, park=dev, metrics=dev)
            loop.seed(seeds)
            if dev:
                ctx.rollout_end = end_after_a_refusal
            out = loop.run()
            assert not loop.retired and all(o is not None for o in out), (dev, loop.retired)
            outs.append((loop, out))
    finally:
        for c in ctxs:
            c.close()
    (dl, dout), (hl, hout) = outs
    assert hl.metrics == [] and len(dl.metrics) == 1 and dl.metrics[0].shape == (4, _capi.METRICS_NCOL)
    assert seen["refusal"] is not None and seen["refusal"][:2] == (-1, True) and "parked" in seen["refusal"][2] and seen["inside"] == 0, seen
    Fx, Fu = _fxfu(cfg)
    w = metrics_ref.weights_of_config(cfg)
    for b, lap in enumerate(hout):
        x, u, xg, f12, T = lap[0], lap[1], lap[2], lap[3], lap[4]
        assert dout[b][4] == T
        want = metrics_ref.lap_metrics(x, u, xg, T, w, Fx, Fu, float(cfg.trackLength), f12[4])
        _same(dl.metrics[0][b], want, ("car", b, dl.metrics[0][b], want))
    m = dl.metrics[0]
    assert (m[:, F["nonfinite_rows"]] == 0).all() and (m[:, F["t_cross"]] > m[:, F["rows"]] - 1).all() and (m[:, F["t_cross"]] <= m[:, F["rows"]]).all()
    assert np.isfinite(m).all() and (m[:, F["path_length"]] > 10).all()
