"""GPU: the contract the five per-car row sets share (csrc/lmpc_rows.h), one test over all of them on the N = 12 golden at max_batch = 3 -- the smallest batch
that tells "one row", "one per car" and "wrong count" apart -- and the two device images that are rebuilt from indices (safe-set table, lap table) growing from one
row to three.  What each set does to the numbers is tested where the set was introduced (test_gpu_plant_params, _lap_table, _ss_table, _tuning, _tracks)."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

B3 = 3
STEP_KEYS = ("xPred", "uPred", "slack", "lambd", "sTerm", "ztNext", "ztuNext", "ssSel", "qSel", "A", "B", "C", "status", "iters")


@pytest.fixture(scope="module")
def g():
    return common.load_lmpc_golden()


def _problems(g):
    """The first three recorded steps of LMPC lap 5 as one batch of three problems, and three plant inputs from the same records."""
    r = np.where(np.asarray(g["rec_lap"]) == 5)[0][:B3]
    p = dict(x0=g["rec_x0"][r], xLin=g["rec_xLin"][r], uLin=g["rec_uLin"][r], uOld=g["rec_OldInput"][r], zt=g["rec_zt"][r], xPredPrev=g["rec_xPredPrev"][r],
             hasPred=np.asarray(g["rec_hasPred"])[r].astype(np.int32), timeStep=np.asarray(g["rec_t"])[r].astype(np.int32))
    return {k: np.ascontiguousarray(v) for k, v in p.items()}


def _step(ctx, p, n=B3):
    out = ctx.step_batch(p["x0"][:n], p["xLin"][:n], p["uLin"][:n], p["uOld"][:n], zt=p["zt"][:n], xPredPrev=p["xPredPrev"][:n], hasPred=p["hasPred"][:n], timeStep=p["timeStep"][:n])
    return {k: np.array(out[k]) for k in STEP_KEYS}


def _plant(ctx, p, n=B3):
    u = p["uLin"][:n, 0]
    xn, xgn, st = ctx.plant_step_batch(p["x0"][:n], p["x0"][:n], u, np.full((n, 3), 0.01))
    return dict(xn=xn, xgn=xgn, status=st)


def _same(a, b, sel=slice(None)):
    return all(np.array_equal(a[k][sel], b[k][sel]) for k in a)


def _scaled_track(g, k):
    """The golden track scaled by k: a consistent PointAndTangent table (x, y, s, length times k, curvature over k) and its length."""
    from racinglmpc_amd import _capi
    t = np.array(g["track"], np.float64).reshape(-1, 6).copy()
    t[:, [0, 1, 3, 4]] *= k; t[:, 5] /= k
    return _capi.track_row(t, float(g["trackLength"]) * k)


def _sets(g, cfg):
    """name -> (three distinct rows, set, get, the call of n problems, the refusal of a B = 2 call (None: accepted, the at-least rule))."""
    from racinglmpc_amd import _capi
    err = "liblmpc_hip error -1: %s: B = 2 %s but %s holds 3 rows"
    return {
        "plant_params": (_capi.plant_params(B3, m=[1.98, 2.3, 1.7], Iz=[0.024, 0.03, 0.02]), "plant_set_params", "plant_params", _plant, None),
        "lap_table": (np.array([[0, 1, 2, 3], [1, 2, 3, 4], [4, 4, 4, 4]], np.int32), "model_set_lap_table", "model_lap_table", _step,
                      err % ("lap table", "problems", "lmpc_model_set_lap_table")),
        "ss_table": (np.array([[0, 1, 2, 3], [1, 2, 3, 4], [4, 3, 3, 0]], np.int32), "ss_set_lap_table", lambda ctx: ctx.ss_lap_table()[0], _step,
                     err % ("safe-set lap table", "problems", "lmpc_ss_set_lap_table")),
        "tuning": (_capi.tuning_rows(cfg, B3, dR=np.array([[5.0, 50.0], [6.0, 55.0], [7.0, 60.0]]), bx=np.array([[0.4, 0.4], [0.5, 0.5], [0.45, 0.45]])),
                   "tuning_set", "tuning", _step, err % ("tuning rows", "problems", "lmpc_tuning_set")),
        "tracks": (np.stack([_scaled_track(g, k) for k in (1.0, 1.03, 0.98)]), "track_set", "tracks", _step, err % ("track rows", "elements", "lmpc_track_set")),
    }


@pytest.fixture(scope="module")
def shared(built, g):
    """One context with nothing set, the batch, and what a context that never held a row gives (computed once, left unchanged)."""
    ctx, _ = common.make_lmpc_ctx(g, 5, max_batch=B3)
    fresh, _ = common.make_lmpc_ctx(g, 5, max_batch=B3)
    p = _problems(g)
    ref = {_step: _step(fresh, p), _plant: _plant(fresh, p)}
    fresh.close()
    yield dict(ctx=ctx, p=p, ref=ref, sets=_sets(g, ctx.cfg))
    ctx.close()


@pytest.mark.parametrize("name", ["plant_params", "lap_table", "ss_table", "tuning", "tracks"])
def test_row_set_contract(shared, name):
    from racinglmpc_amd import _capi
    ctx, p = shared["ctx"], shared["p"]
    rows, setter, getter, call, refusal = shared["sets"][name]
    set_ = getattr(ctx, setter)
    get_ = (lambda: getter(ctx)) if callable(getter) else getattr(ctx, getter)
    assert len({r.tobytes() for r in rows}) == B3
    try:
        assert get_().shape[0] == 0 and _same(call(ctx, p), shared["ref"][call])        # nothing in force: the config's value
        # (a) three distinct rows come back bit for bit
        set_(rows)
        got = get_()
        assert got.dtype == rows.dtype and got.shape == rows.shape and got.tobytes() == rows.tobytes()
        out3 = call(ctx, p)
        assert not _same(out3, shared["ref"][call])                                      # (the rows are read)
        # (b) a call of two
        if refusal is None:
            out2 = call(ctx, p, 2)                                                       # the first two of the three rows
            assert _same(out2, out3, slice(0, 2))
        else:
            with pytest.raises(_capi.LmpcError) as e:
                call(ctx, p, 2)
            assert str(e.value) == refusal
        # (c) the rows stay in force and the context stays usable
        assert get_().tobytes() == rows.tobytes()
        assert _same(call(ctx, p), out3)
        # (e) one row serves every problem: the same as three equal rows, and as row 1 of the distinct rows for problem 1
        set_(rows[1:2])
        assert get_().tobytes() == rows[1:2].tobytes()
        one = call(ctx, p)
        set_(np.repeat(rows[1:2], B3, axis=0))
        assert _same(call(ctx, p), one)
        assert _same(one, out3, slice(1, 2))
        set_(rows[1:2])
        assert _same(call(ctx, p, 2), one, slice(0, 2))                                  # (one row: any count)
        # (d) None: the outputs of a context that never held a row, bit for bit
        set_(None)
        assert get_().shape[0] == 0
        assert _same(call(ctx, p), shared["ref"][call])
    finally:
        set_(None)


def test_safe_set_image_is_rebuilt_and_grows_on_the_dirty_path(built, g):
    """The table set once before a lap is appended (one row: the image is built by the first launch) and once after (three rows that name the new lap: the image is
    marked dirty by the append and grows at the next launch).  Both solve; every car of the three-row call equals its row set alone."""
    ctx, _ = common.make_lmpc_ctx(g, 5, max_batch=B3)
    try:
        p = _problems(g)
        ctx.ss_set_lap_table(np.array([[0, 1, 2, 3]], np.int32))
        first = _step(ctx, p)
        assert not (first["status"] & ~64).any()
        ctx.ss_add_trajectory(g["lapx0"], g["lapu0"])                                    # lap 5; the one-row image is stale now
        assert _same(_step(ctx, p), first)                                               # (rebuilt: the row names none of the laps that changed)
        rows = np.array([[0, 1, 2, 5], [1, 2, 3, 5], [5, 3, 3, 4]], np.int32); last = np.array([5, -1, 4], np.int32)
        ctx.ss_set_lap_table(rows, last)
        out = _step(ctx, p)
        assert not (out["status"] & ~64).any()
        r, l = ctx.ss_lap_table()
        assert np.array_equal(r, rows) and np.array_equal(l, last)
        for b in range(B3):
            ctx.ss_set_lap_table(rows[b:b + 1], last[b:b + 1])
            assert _same(_step(ctx, p), out, slice(b, b + 1)), b
    finally:
        ctx.close()


def test_lap_table_image_grows_from_one_row_to_three(built, g):
    """lmpc_model_set_lap_table with one row and then with three: regress_batch with the three rows equals, car by car, the single-row tables."""
    ctx, _ = common.make_lmpc_ctx(g, 5, max_batch=B3)
    try:
        p = _problems(g)
        rows = np.array([[0, 1, 2, 3], [1, 2, 3, 4], [4, 4, 4, 4]], np.int32)
        ctx.model_set_lap_table(rows[:1])
        one = ctx.regress_batch(p["xLin"], p["uLin"])
        ctx.model_set_lap_table(rows)
        three = ctx.regress_batch(p["xLin"], p["uLin"])
        assert all(np.array_equal(a[0], b[0]) for a, b in zip(one, three))
        assert not np.array_equal(three[0][2], one[0][2])                                # (row 2 names another lap)
        for b in range(B3):
            ctx.model_set_lap_table(rows[b:b + 1])
            own = ctx.regress_batch(p["xLin"], p["uLin"])
            assert all(np.array_equal(a[b], c[b]) for a, c in zip(own, three)), b
    finally:
        ctx.close()
