"""-m gpu: per-car tracks (lmpc_track_set) -- each element of a batch on its own track table and length, in the regression kernel, the plant kernels, the
safe-set selection, the lap-store commit and the track maps.  Cars are dealt over the reference's three specs (tests/track_cases.py: L, oval, goggle) unless stated.

The method for the kernels is that of the lap tables (tests/test_gpu_table_routes.py): the reference of a car is a context of the same configuration in which its
track serves EVERY car (one row), run on the same batch -- same kernel, same batch shape, same route -- and the mixed context must give its BITS, car by car.
One row is in turn held against a context created with that track in its configuration (the kernels that read the parameter block), and the new tracks against
the oracle.  The stores of every context are the L fixture's (tests/ss_table_cases.py): data, not geometry -- what differs between contexts is the track alone."""
import contextlib
import ctypes

import numpy as np
import pytest

from tests import common
from tests import plant_ref as pr
from tests import ss_table_cases as cases
from tests import track_cases as tk
from tests import track_ref
from tests.test_gpu_routes import _knobs, _routes

pytestmark = pytest.mark.gpu

STEP_KEYS = ("xPred", "uPred", "lambd", "ztNext", "ztuNext", "status", "iters", "ssSel", "qSel", "A", "B", "C")
DEV_KEYS = tuple(k for k in STEP_KEYS if k != "qSel")                 # (step_dev_buffers(diagnostics=False) leaves qSel NULL)
SEL_KEYS = ("ssSel", "qSel", "succ", "succU", "ztUsed", "selStart", "status")
ROUTE_BOUND = 2e-7              # |x, u| between two solve routes on the same QP (lmpc_active_knobs, tests/test_gpu_routes.py)
BATCH = {64: 66, 300: 300, 600: 600, 1100: 1098}


@pytest.fixture(scope="module")
def g(built):
    return common.load_lmpc_golden()


def _same(a, b):
    """bit for bit, NaN and signed zeros included"""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _code(f):
    from racinglmpc_amd import _capi
    with pytest.raises(_capi.LmpcError) as e:
        f()
    return int(str(e.value).split()[2].rstrip(":")), str(e.value)


def _track_g(g, name):
    """What common.lmpc_config reads of a fixture, with the track `name` in it."""
    t, L = tk.table(name)
    return dict(track=np.array(t), trackLength=L)


@contextlib.contextmanager
def _ctx(g, max_batch, N=12, rows=None, config_track=None, runtime=False, knobs=None, fill=True, rows_first=False, **kw):
    """An LMPC context with the fixture's stores, filled BEFORE the rows are set: by the configuration's TrackLength, the L track's, in every context alike.
    rows_first (one row): the row is set first, so that the host-side writers fill the stores with ITS TrackLength, as a context configured with that track does."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g if config_track is None else _track_g(g, config_track), N, max_batch=max_batch, **kw)
    with _knobs(knobs or {}):
        c = _capi.Context(cfg, runtime_kernel=runtime)
    try:
        if rows is not None and rows_first:
            c.track_set(rows)
        if fill:
            cases.fill_table_context(c, g)
        if rows is not None and not rows_first:
            c.track_set(rows)
        yield c
    finally:
        c.close()


def _step(ctx, p):
    return ctx.step_batch(p["x0"], p["xLin"], p["uLin"], p["uOld"], p["zt"], p["xPredPrev"], p["hasPred"], p["timeStep"])


def _sel(ctx, p):
    return ctx.select_batch(p["x0"], p["zt"], p["xPredPrev"], p["hasPred"], p["timeStep"])


def _take(p, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in p.items()}


# ---- 1
def test_default_rows_are_the_old_path(g):
    """track_set with the configuration's own row -- one row for all cars, and one per car -- gives the bits of a context without rows: lmpc_plant_step_batch, a
    200-step PID launch and 30 LMPC steps on the 48 cars of test_gpu_plant_track._mixed_cars (the form of test_gpu_plant_params.test_default_rows_are_the_nominal_path);
    track_set(None) returns to the kernels that read the parameter block."""
    from racinglmpc_amd import _capi
    from tests.test_gpu_plant_track import _mixed_cars
    x, xg, u, nz = _mixed_cars(g)
    B = x.shape[0]
    ctx, _ = common.make_lmpc_ctx(g, 4, max_batch=64)
    row = _capi.track_row(g["track"], float(g["trackLength"]))
    own = np.zeros(98)
    assert ctx.lib.lmpc_track_row_from_config(ctypes.byref(ctx.cfg), own.ctypes.data) == 0 and _same(own, row)
    rng = np.random.default_rng(3)
    T = 200
    vt = 0.6 + 0.02 * (np.arange(B) % 30); nu = rng.standard_normal((T, B, 2)); nzp = rng.standard_normal((T, B, 3))
    xs = x.copy(); xs[~np.isfinite(xs) | (np.abs(xs) > 1e100)] = 66 * float(g["trackLength"])
    xl = np.tile(g["SS0"][1:14][None], (B, 1, 1)); ul = np.tile(g["uSS0"][1:13][None], (B, 1, 1)); nzl = rng.standard_normal((30, B, 3))

    def run():
        out = list(ctx.plant_step_batch(x, xg, u, nz))
        t, _ = ctx.rollout_pid(x, xg, vt, nu, nzp)
        out += list(ctx.rollout_fetch(0, t)); ctx.rollout_end()
        ctx.rollout_begin(xs, xg, xl, ul, nzl)
        t, _ = ctx.rollout_run(30)
        out += list(ctx.rollout_fetch(0, t)); ctx.rollout_end()
        return out
    try:
        ref = run()
        assert (ref[2] != 0).any() and (ref[2] == 0).any() and ctx.tracks().shape == (0, 98)
        for rows in (row[None], np.tile(row, (B, 1))):
            ctx.track_set(rows)
            assert _same(ctx.tracks(), rows)                              # (a row round-trips through the context)
            got = run()
            assert len(got) == len(ref)
            for i, (a, b) in enumerate(zip(got, ref)):
                assert _same(a, b), (rows.shape, i)
        ctx.track_set(None)
        assert ctx.tracks().shape == (0, 98)
        for i, (a, b) in enumerate(zip(run(), ref)):
            assert _same(a, b), i
    finally:
        ctx.close()


# ---- 2
def _everything(g, ctx, p, B, names, rng_seed, commit_names=None):
    """Every batched call on one context: regression, selection, step, plant step, an LMPC session of 20 steps whose first 10 rows then extend laps 0..5 by cars
    0..5 (after the last step: the safe set is shared, and a lap extended by another car's TrackLength must not reach this car's selection), and a PID session of 330
    steps whose finished cars are committed to the safe set.  names[b]: the track of car b; commit_names: only cars on these tracks extend and commit (a
    single-track context: the others cross its line at other steps or never).  Returns {name: array}, laps keyed by car."""
    rng = np.random.default_rng(rng_seed)
    out = {}
    A, Bm, C, rst = ctx.regress_batch(p["xLin"], p["uLin"])
    out.update(reg_A=A, reg_B=Bm, reg_C=C, reg_status=rst)
    out.update({"sel_" + k: v for k, v in _sel(ctx, p).items() if k in SEL_KEYS})
    out.update({"step_" + k: v for k, v in _step(ctx, p).items() if k in STEP_KEYS})
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    rows = (37 * np.arange(B)) % 600
    nz = rng.standard_normal((B, 3))
    xn, xgn, pst = ctx.plant_step_batch(xP[rows], xP[rows], uP[rows], nz)
    out.update(plant_x=xn, plant_xg=xgn, plant_status=pst)
    T = 330
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1))
    vt = 0.8 + 0.005 * (np.arange(B) % 7); nu = rng.standard_normal((T, B, 2)); nzp = rng.standard_normal((T, B, 3))
    nzl = rng.standard_normal((20, B, 3))
    ctx.rollout_begin(p["x0"], p["x0"], p["xLin"], p["uLin"], nzl)
    t, _ = ctx.rollout_run(20)
    X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
    out.update(lmpc_X=X, lmpc_U=U, lmpc_G=G, lmpc_done=done, lmpc_status=st)
    ext_cars = [b for b in range(6) if commit_names is None or names[b] in commit_names]
    ok = ctx.rollout_extend_laps(ext_cars, ext_cars, 10)
    ctx.rollout_end()
    assert ok.all()
    for b in ext_cars:
        x, u, q = ctx.store_read_lap(1, b)
        out["ext_x_%d" % b] = x; out["ext_q_%d" % b] = q
    t, _ = ctx.rollout_pid(x0, x0, vt, nu, nzp)
    X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
    out.update(pid_X=X, pid_U=U, pid_G=G, pid_done=done, pid_status=st, pid_finX=fx, pid_finG=fg)
    cars = [b for b in range(12) if done[b] >= 2 and (commit_names is None or names[b] in commit_names)]
    first = ctx.rollout_commit_laps(cars, ss=True, model=False) if cars else (None, None)
    ctx.rollout_end()
    for i, b in enumerate(cars):
        x, u, q = ctx.store_read_lap(1, first[0] + i)
        out["lap_x_%d" % b] = x; out["lap_u_%d" % b] = u; out["lap_q_%d" % b] = q
    return out


def _car(v, b, key):
    """Car b's part of an output: the whole array for a lap keyed by car, axis 1 for session logs (T, B, ..), else axis 0."""
    if key.startswith(("lap_", "ext_")):
        return v
    if key in ("pid_X", "pid_U", "pid_G", "lmpc_X", "lmpc_U", "lmpc_G"):
        return v[:, b]
    return v[b]


@pytest.mark.parametrize("permuted", [False, True], ids=["dealt", "permuted"])
def test_car_by_car_against_single_track_contexts(g, permuted):
    """B = 33: two plant work-groups, a lane pair without a car, track changes inside a work-group.  For each track a second context runs the same batch with that
    track's row for every car; car b of the mixed batch equals car b of the context of its track bit for bit in A, B, C and regression status, the selection's
    outputs, the step's outputs, plant states, the PID logs, doneAt, final states, the committed laps with their Qfun and the extended laps."""
    B = 33
    perm = np.random.default_rng(11).permutation(B) if permuted else None
    names = tk.deal(B, perm=perm)
    p = cases.problems(g, B, 12)
    with _ctx(g, B, rows=tk.rows_of(names), max_laps=32) as ctx:
        mixed = _everything(g, ctx, p, B, names, 5)
    assert not (mixed["step_status"] & ~64).any() and not (mixed["reg_status"] != 0).any()
    done = mixed["pid_done"]
    print("PID crossing steps per track:", {n: sorted(set(int(d) for d, m in zip(done, names) if m == n)) for n in tk.NAMES})
    assert all(done[b] >= 0 for b in range(B))
    refs = {}
    for n in tk.NAMES:
        with _ctx(g, B, rows=tk.rows_of([n]), max_laps=32) as ctx:
            refs[n] = _everything(g, ctx, p, B, names, 5, commit_names=(n,))
    fails = []
    for key, v in mixed.items():
        cars = [int(key.rsplit("_", 1)[1])] if key.startswith(("lap_", "ext_")) else range(B)
        for b in cars:
            ref = refs[names[b]]
            if key not in ref:
                fails.append("%s: missing on the context of track %s" % (key, names[b]))
            elif not _same(_car(v, b, key), _car(ref[key], b, key)):
                fails.append("%s, car %d (%s) differs from the context of its track" % (key, b, names[b]))
    assert not fails, "\n".join(fails[:20])
    assert sum(k.startswith("lap_q_") for k in mixed) == 12 and sum(k.startswith("ext_q_") for k in mixed) == 6
    # the comparison tells the tracks apart: a car on the oval or the goggle track differs from the L context in every family of outputs
    for key in ("reg_A", "sel_qSel", "step_xPred", "plant_x", "pid_X", "pid_done", "lmpc_X"):
        other = [b for b in range(B) if names[b] != "L" and not _same(_car(mixed[key], b, key), _car(refs["L"][key], b, key))]
        assert other, key
    # computeCost with the car's own TrackLength (exact), and addPoint's shift by it
    from oracle import lmpc_oracle as orc
    TL = dict(zip(tk.NAMES, tk.lengths_of(tk.NAMES)))
    for key in [k for k in mixed if k.startswith("lap_x_")]:
        b = int(key.rsplit("_", 1)[1])
        assert _same(mixed["lap_q_%d" % b], orc.compute_cost(mixed[key], TL[names[b]])), b
    stored = cases.cpu_stored(g)
    for b in range(6):
        T0 = stored[b][0].shape[0]
        assert _same(mixed["ext_x_%d" % b][T0:, 4], mixed["lmpc_X"][:10, b, 4] + TL[names[b]]), b


def _route_cases():
    out = []
    for name, B0, waves, knobs, rt, fused in _routes(12):
        out.append(pytest.param(12, BATCH[B0], waves, knobs, rt, id="N12-" + name.replace(" ", "_")))
    out.append(pytest.param(9, 66, 1, {}, True, id="N9-runtime_kernel"))
    return out


@pytest.mark.parametrize("N,B,waves,knobs,rt", _route_cases())
def test_every_solve_route_serves_the_rows(g, N, B, waves, knobs, rt):
    """The step on every route production takes at N = 12 (four, two, one wave per QP, LMPC_FUSE=1 -- not taken with rows: the two-kernel step --, the runtime kernel)
    and the runtime kernel at a horizon no fixed kernel serves: every problem of the mixed batch equals the problem of the context of its track, bit for bit."""
    names = tk.deal(B)
    p = cases.problems(g, B, N)
    with _ctx(g, B, N=N, rows=tk.rows_of(names), runtime=rt, knobs=knobs) as ctx:
        assert ctx.solver_kind == (2 if rt else 0) and (rt or ctx.solver_waves(B) == waves), (ctx.solver_kind, ctx.solver_waves(B))
        ctx.reset_stats()
        out = _step(ctx, p)
        assert int(ctx.stats().n_regress) == 1
    assert not (out["status"] & ~64).any(), np.unique(out["status"], return_counts=True)
    fails, told = [], []
    for n in tk.NAMES:
        with _ctx(g, B, N=N, rows=tk.rows_of([n]), runtime=rt, knobs=knobs) as ctx:
            ref = _step(ctx, p)
        mine = np.array([b for b in range(B) if names[b] == n])
        fails += ["%s: %s" % (n, k) for k in STEP_KEYS if not _same(np.asarray(out[k])[mine], np.asarray(ref[k])[mine])]
        other = np.array([b for b in range(B) if names[b] != n])              # (the comparison tells the tracks apart: the curvature on every track, the selection's
        assert not _same(np.asarray(out["A"])[other], np.asarray(ref["A"])[other]), n      #  TrackLength wherever the lengths place the predicted rows differently)
        told.append(not _same(np.asarray(out["qSel"])[other], np.asarray(ref["qSel"])[other]))
    assert not fails, fails
    assert any(told), told


# ---- 3
@pytest.mark.parametrize("name", ["oval", "goggle"])
def test_one_row_against_a_context_created_with_that_track(g, name):
    """n = 1 against a context whose lmpc_config holds the track: regression, plant, maps, PID session and committed laps agree bit for bit (the same arithmetic on
    the same numbers, read from the row instead of the parameter block); the QP answer within the project's route bound, 2e-7 on x and u -- the solve runs in the
    per-problem-rows instantiation on one side."""
    B = 33
    p = cases.problems(g, B, 12)
    names = [name] * B
    s_ = np.linspace(0.0, 2.5 * tk.table(name)[1], B); ey = np.linspace(-0.3, 0.3, B)

    def run(ctx):
        o = _everything(g, ctx, p, B, names, 9)
        o["map_xy"], o["map_st"] = ctx.global_position_batch(s_, ey)
        o["map_psi"], o["map_pst"] = ctx.track_angle(s_, 0.1 * ey)
        o["loc_s"], o["loc_ey"], o["loc_epsi"], o["loc_st"] = ctx.local_position(o["map_xy"][:, 0], o["map_xy"][:, 1], o["map_psi"], tk.MAX_EY)
        o["inv_x"], o["inv_st"] = ctx.state_from_global(o["pid_G"], tk.MAX_EY)
        return o
    with _ctx(g, B, rows=tk.rows_of([name]), rows_first=True, max_laps=32) as ctx:
        a = run(ctx)
    with _ctx(g, B, config_track=name, max_laps=32) as ctx:
        assert ctx.tracks().shape == (0, 98)
        b_ = run(ctx)
    worst = max(float(np.abs(a[k] - b_[k]).max()) for k in ("step_xPred", "step_uPred"))
    print("%s: one row against the configured context: worst |x, u| difference of the step %.3e" % (name, worst))
    assert worst <= ROUTE_BOUND
    # (what follows the QP's answer -- the multipliers, the next terminal point, the closed loop of the session and the rows it appends -- is held by the step's bound alone)
    soft = ("step_xPred", "step_uPred", "step_lambd", "step_ztNext", "step_ztuNext", "step_iters", "step_status")
    bad = [k for k in a if k not in soft and not k.startswith(("lmpc_", "ext_x_")) and not _same(a[k], b_[k])]
    assert not bad, bad
    assert (a["map_st"] == 0).all() and (a["loc_st"] == 0).all() and (a["inv_st"] == 0).any() and (a["pid_done"] > 0).all()


# ---- 4
@pytest.mark.parametrize("name", ["oval", "goggle"])
def test_new_tracks_against_the_oracle(g, name):
    """On the oval and the goggle track, six cars / points each on a context whose rows are [L, name] x 3 (so that the row, not the configuration, is what is read):
    the regression against oracle.regression_and_linearization at 3e-10 (relative, the project's bound for A, B, C of one point), the plant against
    plant_ref.oracle_step at 1e-12, the maps against tests/track_ref.py and the oracle's forward map on the end point of every table row (ey = 0: the equality branches), points 1 mm inside both
    ends of every row, the oval's 6e-16 closing row and s = TrackLength exactly (statuses equal, values within 1e-9), committed laps' Qfun against
    oracle.compute_cost exactly."""
    from oracle import lmpc_oracle as orc
    from racinglmpc_amd import _capi
    pt, TL = np.array(tk.table(name)[0]), tk.table(name)[1]
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    # -- regression and plant: cars 1, 3, 5 are on the new track
    n = 6
    names = ["L", name] * 3
    idx = np.array([40, 120, 200, 290, 310, 420])
    with _ctx(g, 64, rows=tk.rows_of(names)) as ctx:
        A, Bm, C, st = ctx.regress_points(xP[idx], uP[idx])
        nz = np.random.default_rng(1).standard_normal((n, 3))
        xn, xgn, pst = ctx.plant_step_batch(xP[idx], xP[idx], uP[idx], nz)
        t, _ = ctx.rollout_pid(np.tile([0.5, 0, 0, 0, 0, 0.0], (n, 1)), np.tile([0.5, 0, 0, 0, 0, 0.0], (n, 1)), np.full(n, 0.8),
                               np.random.default_rng(2).standard_normal((320, n, 2)), np.random.default_rng(3).standard_normal((320, n, 3)), stop_at_line=True)
        done = ctx.rollout_fetch(0, 0)[3]
        first = ctx.rollout_commit_laps([1, 3, 5], ss=True, model=False)
        ctx.rollout_end()
        laps = [ctx.store_read_lap(1, first[0] + i) for i in range(3)]
    assert (st == 0).all() and (pst == 0).all() and (done[[1, 3, 5]] > 100).all()
    worst_abc = worst_plant = 0.0
    for b in (1, 3, 5):
        Ao, Bo, Co = orc.regression_and_linearization([xP] * 4, [uP] * 4, [0, 1, 2, 3], pt, xP[idx[b]], uP[idx[b]])
        for got, ref in ((A[b], Ao), (Bm[b], Bo), (C[b], np.ravel(Co))):
            worst_abc = max(worst_abc, float((np.abs(got - ref) / (1 + np.abs(ref))).max()))
        ref = pr.oracle_step(pt, xP[idx[b]], xP[idx[b]], uP[idx[b]], nz[b])
        assert ref is not None
        worst_plant = max(worst_plant, float(pr.scaled_err(xn[b][None], ref[0][None])[0]), float(pr.scaled_err(xgn[b][None], ref[1][None])[0]))
    print("%s: worst A, B, C against the oracle %.3e; worst plant state %.3e" % (name, worst_abc, worst_plant))
    assert worst_abc < 3e-10 and worst_plant <= 1e-12
    for x, u, q in laps:
        assert _same(q, orc.compute_cost(x, TL)) and q[0] == x.shape[0] - 1 and x[-1, 4] <= TL
    # -- maps: forward (s, ey) -> (X, Y), psi; inverse on the images
    # (s = c0 exactly takes ey = 0 only: with ey != 0 the point lies ON the perpendicular through the row's end, where the reference's `|angle| <= pi / 2` is decided
    #  by the last ulp of arctan2 -- and ocml's differs from NumPy's by a few ulp, tests/test_gpu_track_inverse.py.  The forward maps have no such test.)
    s_list, ey_list, on_end = [], [], []
    for i in range(pt.shape[0]):
        c0, ln = pt[i, 3], pt[i, 4]
        for s in ([c0, c0 + 1e-3, c0 + ln / 2, c0 + ln - 1e-3] if ln > 1e-2 else [c0]):
            for ey in (0.0, 0.2, -0.2):
                s_list.append(s); ey_list.append(ey); on_end.append(s == c0 and ey != 0.0)
    s_list += [TL, TL + 0.7, 2 * TL + 0.5]; ey_list += [0.0, 0.1, -0.1]; on_end += [False] * 3
    s_arr, ey_arr, on_end = np.array(s_list), np.array(ey_list), np.array(on_end); m = s_arr.shape[0]
    with _ctx(g, 4 * m, rows=tk.rows_of(["L", name] * m), fill=False) as ctx:
        S2, E2 = np.repeat(s_arr, 2), np.repeat(ey_arr, 2)                 # (point 2 i on L, 2 i + 1 on the new track)
        xy, fst = ctx.global_position_batch(S2, E2)
        psi, ast = ctx.track_angle(S2, 0.05 + 0 * S2)
        xy, fst, psi, ast = xy[1::2], fst[1::2], psi[1::2], ast[1::2]
        want_xy, want_fst = [], []
        for s, ey in zip(s_arr, ey_arr):
            try:
                want_xy.append(orc.get_global_position(pt, float(s), float(ey))); want_fst.append(0)
            except Exception:                                            # noqa: BLE001  (the reference raises: s on no row)
                want_xy.append((0.0, 0.0)); want_fst.append(_capi.ST_NO_SEGMENT)
        want_psi, want_ast = track_ref.track_angle_batch(pt, s_arr, 0.05 + 0 * s_arr)
        assert np.array_equal(fst, np.array(want_fst, np.int32)) and np.array_equal(ast, want_ast), (fst, want_fst, ast, want_ast)
        ok = fst == 0
        print("%s: forward maps on %d points (%d on no row): worst |xy| %.3e, |psi| %.3e" % (name, m, (~ok).sum(), np.abs(xy - np.array(want_xy))[ok].max(),
                                                                                           np.abs(psi - want_psi)[ast == 0].max()))
        assert np.abs(xy - np.array(want_xy))[ok].max() <= 1e-9 and np.abs(psi - want_psi)[ast == 0].max() <= 1e-9
        # inverse: the row end points themselves (exact equality branches) and the images of the points above
        inv = ok & ~on_end
        px = np.concatenate([pt[:, 0], np.array(want_xy)[inv][:, 0]]); py = np.concatenate([pt[:, 1], np.array(want_xy)[inv][:, 1]])
        pp = np.concatenate([pt[:, 2], want_psi[inv]])
        k = px.shape[0]
        ctx.track_set(tk.rows_of(["L", name] * k))
        s_, ey_, ep_, ist = ctx.local_position(np.repeat(px, 2), np.repeat(py, 2), np.repeat(pp, 2), tk.MAX_EY)
        s_, ey_, ep_, ist = s_[1::2], ey_[1::2], ep_[1::2], ist[1::2]
        ws, wey, wep, wst, _ = track_ref.local_position_batch(pt, px, py, pp, tk.MAX_EY)
        assert np.array_equal(ist, wst), (np.where(ist != wst)[0], px[ist != wst], py[ist != wst])
        err = max(np.abs(s_ - ws).max(), np.abs(ey_ - wey).max(), np.abs(ep_ - wep).max())
        print("%s: inverse map on %d points (%d row end points): worst difference %.3e" % (name, k, pt.shape[0], err))
        assert err <= 1e-9


# ---- 5
def test_finish_line_per_car(g):
    """PID cars at the same target speed on the oval (13.0 m) and on L (19.23 m): each crosses ITS line -- doneAt is the first step after which s > TrackLength_b, read
    off the full log of a run that does not stop, finalX is the state right after that step -- and with stop_at_line each car is logged up to its own crossing."""
    B = 8
    names = tk.deal(B, names=("oval", "L"))
    TLs = tk.lengths_of(names)
    T = 330
    rng = np.random.default_rng(21)
    nu = rng.standard_normal((T, B, 2)); nz = rng.standard_normal((T, B, 3))
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1))
    with _ctx(g, B, rows=tk.rows_of(names), fill=False) as ctx:
        t, nd = ctx.rollout_pid(x0, x0, np.full(B, 0.8), nu, nz)
        X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
        ctx.rollout_end()
        t2, nd2 = ctx.rollout_pid(x0, x0, np.full(B, 0.8), nu, nz, stop_at_line=True)
        X2, U2, G2, done2, st2, fx2, fg2 = ctx.rollout_fetch(0, t2)
        ctx.rollout_end()
    print("crossing steps:", dict(zip(names, done.tolist())))
    assert t == T and nd == B and (st == 0).all() and np.array_equal(done, done2) and _same(fx, fx2) and _same(fg, fg2)
    for b in range(B):
        over = np.where(X[:, b, 4] > TLs[b])[0]
        assert over.size and done[b] == over[0] and X[done[b] - 1, b, 4] <= TLs[b], b            # (row t is the state BEFORE step t: the crossing step is done - 1)
        assert _same(fx[b], X[done[b], b]) and _same(fg[b], G[done[b], b]), b
        assert _same(X2[:done[b], b], X[:done[b], b]) and _same(U2[:done[b], b], U[:done[b], b]), b
    oval, ell = done[0::2], done[1::2]
    assert oval.max() < ell.min() and abs(int(np.median(oval)) - tk.PID_ROWS["oval"]) < 25 and abs(int(np.median(ell)) - tk.PID_ROWS["L"]) < 25


# ---- 6
def test_wrap_bookkeeping_of_the_selection(g):
    """One selection with hasPred = 1 and predicted rows beyond the shorter TrackLength but not the longer: the crossed count and the Qfun shift differ by car, the
    zt wrap test reads the car's own TrackLength, and every car equals oracle.terminal_components(..., TrackLength = TL_b) exactly."""
    B = 18
    names = tk.deal(B)
    TLs = tk.lengths_of(names)
    p = cases.problems(g, B, 12)
    crossed = np.array([(p["xPredPrev"][b, :, 4] > TLs[b]).sum() for b in range(B)])
    by_track = {n: sorted(set(int(c) for c, m in zip(crossed, names) if m == n)) for n in tk.NAMES}
    print("crossed predicted rows per track:", by_track)
    assert by_track["L"] != by_track["oval"] and any(0 < c < 13 for c in crossed)
    with _ctx(g, B, rows=tk.rows_of(names)) as ctx:
        stored = cases.read_laps(ctx)
        out = _sel(ctx, p)
    assert not (out["status"] & ~64).any()
    for b in range(B):
        SSsel, Qsel, Succ, SuccU, ok = cases.oracle_selection(stored, list(range(6)), p, b, TLs[b], 4, 12, N=12)
        assert ok and _same(out["ssSel"][b], SSsel) and _same(out["qSel"][b], Qsel) and _same(out["succ"][b], Succ) and _same(out["succU"][b], SuccU), (b, names[b])
    # ... and with the L length for every car the oval cars' terminal costs would be others
    SSl, Ql, _, _, _ = cases.oracle_selection(stored, list(range(6)), p, 1, TLs[0], 4, 12, N=12)
    assert names[1] == "oval" and not _same(out["qSel"][1], Ql)


# ---- 7
def test_deferred_retry_reads_the_rows_of_its_own_launch(g):
    """Device path, max_iter = 7, batch 66 (the form of test_gpu_table_routes.test_deferred_retry_reads_the_table_of_its_own_launch): a launch with rows T1 stays
    pending its retry pass; then the context gets T2 -- every car's track changed --, which resolves the pending launch before the image is overwritten, and a
    second launch on other buffers.  The first equals a context that only ever had T1, the second one that only ever had T2."""
    B = 66
    p = cases.problems(g, B, 12)
    n1 = tk.deal(B); n2 = n1[1:] + n1[:1]
    assert all(a != b for a, b in zip(n1, n2))
    T1, T2 = tk.rows_of(n1), tk.rows_of(n2)
    with _ctx(g, B, rows=T1, max_iter=7) as c:
        ref1 = _step(c, p)
        assert c.stats().n_retry == 1
    with _ctx(g, B, rows=T2, max_iter=7) as c:
        ref2 = _step(c, p)
        assert c.stats().n_retry == 1
    # (the two launches differ in what the regression reads -- the curvature -- and in what the selection reads -- the TrackLength of the Q-function shift --, and
    #  the retry pass selects again: its xPred follows the qSel of ITS rows)
    assert [k for k in ("qSel", "xPred", "A") if not _same(ref1[k], ref2[k])] == ["qSel", "xPred", "A"]
    with _ctx(g, B, rows=T1, max_iter=7) as ctx:
        a1, keep1 = ctx.step_dev_buffers(p, diagnostics=False); a2, keep2 = ctx.step_dev_buffers(p, diagnostics=False)
        try:
            ctx.step_batch_dev(B, a1)
            assert ctx.stats().n_retry == 0                                # pending
            ctx.track_set(T2)
            assert ctx.stats().n_retry == 1                                # the image is about to be overwritten: launch 1 got its pass first
            ctx.step_batch_dev(B, a2)
            out1 = ctx.step_dev_fetch(a1, B); out2 = ctx.step_dev_fetch(a2, B)
            assert ctx.stats().n_retry == 2
        finally:
            for q in keep1 + keep2:
                ctx.dev_free(q)
    bad1 = [k for k in DEV_KEYS if not _same(np.asarray(out1[k]), np.asarray(ref1[k]))]
    bad2 = [k for k in DEV_KEYS if not _same(np.asarray(out2[k]), np.asarray(ref2[k]))]
    assert not bad1, "the pending launch's %s differ from a context that only ever had its rows" % bad1
    assert not bad2, "the second launch's %s differ from a context that only ever had the second rows" % bad2


# ---- 8
def test_refusals_leave_the_context_usable(g):
    """A count different from n (every batched entry point), a set during a session, a host writer without _on at n > 1, malformed rows: the documented code, the rows
    in force kept, and the next well-formed call answers as before."""
    from racinglmpc_amd import _capi
    B = 6
    names = tk.deal(B)
    rows = tk.rows_of(names)
    p = cases.problems(g, B, 12)
    p4 = _take(p, slice(0, 4))
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    with _ctx(g, 16, rows=rows) as ctx:
        ref = _step(ctx, p)
        E_ARG, E_STATE = -1, -4
        x4 = xP[[10, 20, 30, 40]]; u4 = uP[[10, 20, 30, 40]]
        calls = dict(
            regress_batch=lambda: ctx.regress_batch(p4["xLin"], p4["uLin"]), regress_points=lambda: ctx.regress_points(x4, u4), step_batch=lambda: _step(ctx, p4),
            select_batch=lambda: _sel(ctx, p4), plant_step_batch=lambda: ctx.plant_step_batch(x4, x4, u4, np.zeros((4, 3))),
            rollout_begin=lambda: ctx.rollout_begin(p4["x0"], p4["x0"], p4["xLin"], p4["uLin"], np.zeros((5, 4, 3))),
            rollout_pid=lambda: ctx.rollout_pid(x4, x4, np.full(4, 0.8), np.zeros((5, 4, 2)), np.zeros((5, 4, 3))),
            global_position_batch=lambda: ctx.global_position_batch(np.ones(4), np.zeros(4)), local_position=lambda: ctx.local_position(np.ones(4), np.zeros(4), np.zeros(4), 0.85),
            track_angle=lambda: ctx.track_angle(np.ones(4), np.zeros(4)), state_from_global=lambda: ctx.state_from_global(np.zeros((3, 4, 6)), 0.85))
        for what, f in calls.items():
            code, msg = _code(f)
            assert code == E_ARG and "lmpc_track_set holds 6 rows" in msg, (what, code, msg)
        # a host writer names no car
        for f in (lambda: ctx.ss_add_trajectory(xP[:50], uP[:50]), lambda: ctx.ss_add_point(xP[0], uP[0]), lambda: ctx.ss_extend_lap(0, xP[:5], uP[:5])):
            code, msg = _code(f)
            assert code == E_STATE and "_on" in msg, (code, msg)
        assert _code(lambda: ctx.ss_add_trajectory(xP[:50], uP[:50], track_row=6))[0] == E_ARG and _code(lambda: ctx.ss_extend_lap(0, xP[:5], uP[:5], track_row=-1))[0] == E_ARG
        assert ctx.ss_num_laps() == 6
        # malformed rows: refused by the library itself (the Python check is bypassed), the rows in force stay
        def raw(r, n=None):
            r = np.ascontiguousarray(r, dtype=np.float64)
            return ctx.lib.lmpc_track_set(ctx._h, r.shape[0] if n is None else n, r.ctypes.data)

        def bad(i, j, v):
            r = rows.copy(); r[i, j] = v
            return r
        for r in (bad(1, 40, np.nan), bad(0, 1, np.inf), bad(2, 0, 0.0), bad(2, 0, 17.0), bad(0, 0, 6.5), bad(1, 1, 0.0), bad(1, 1, -13.0), bad(0, 2 + 6 * 3 + 4, -1e-9)):
            assert raw(r) == E_ARG and "the rows in force stay" in ctx.lib.lmpc_last_error().decode()
        assert raw(rows, -1) == E_ARG and ctx.lib.lmpc_track_set(ctx._h, 2, None) == E_ARG and raw(np.tile(rows, (3, 1))) == E_ARG      # (18 rows > max_batch = 16)
        assert _same(ctx.tracks(), rows)
        # a set during a session
        ctx.rollout_begin(p["x0"], p["x0"], p["xLin"], p["uLin"], np.zeros((5, B, 3)))
        code, msg = _code(lambda: ctx.track_set(rows[::-1]))
        assert code == E_STATE and "session" in msg
        code, msg = _code(lambda: ctx.track_set(None))
        assert code == E_STATE
        ctx.rollout_end()
        assert _same(ctx.tracks(), rows)
        again = _step(ctx, p)
        assert not [k for k in STEP_KEYS if not _same(again[k], ref[k])]
        # the _on forms: the Q-function counts with the named row's TrackLength, the extension shifts by it
        from oracle import lmpc_oracle as orc
        TLs = tk.lengths_of(names)
        ctx.ss_add_trajectory(xP[:330], uP[:330], track_row=1)
        x, u, q = ctx.store_read_lap(1, 6)
        assert _same(q, orc.compute_cost(xP[:330], TLs[1])) and not _same(q, orc.compute_cost(xP[:330], TLs[0]))
        ctx.ss_extend_lap(6, xP[:5], uP[:5], track_row=2)
        x, u, q = ctx.store_read_lap(1, 6)
        assert _same(x[330:, 4], xP[:5, 4] + TLs[2]) and x.shape[0] == 335
        ctx.track_set(rows[1:2])                                          # one row: the host writers use it
        ctx.ss_add_trajectory(xP[:330], uP[:330])
        assert _same(ctx.store_read_lap(1, 7)[2], orc.compute_cost(xP[:330], TLs[1]))


# ---- 9
def test_one_generation_end_to_end(g):
    """B = 6 cars, two per track: rollout.bootstrap(tracks=) -- PID, LTI-MPC and LTV-MPC laps, car b on its own track with its own regression lap --, then
    PerCarLMPC(device_commit=True) seeded with the cars' PID laps.  One generation completes with no status bit but INEXACT; each car's stored lap has
    Qfun[0] == rows - 1, starts behind the line (s[0] < 1.0) and ends before ITS TrackLength."""
    from racinglmpc_amd import _capi, rollout
    B, N = 6, 12
    names = tk.deal(B)
    TLs = tk.lengths_of(names)
    tabs = [np.array(tk.table(n)[0]) for n in names]
    boot = rollout.bootstrap(np.array(g["track"]), B, N, 0.8, seed=3, max_steps=1000, device_noise=True, per_car_store=True, tracks=tabs)
    for stage in ("pid", "mpc", "ltvmpc"):
        d = [l[4] for l in boot[stage]]; st = [l[5] for l in boot[stage]]
        print("bootstrap %-6s crossing steps %s status %s" % (stage, d, st))
        assert all(x > 0 for x in d) and not any(s & ~_capi.ST_INEXACT for s in st), stage
    # each car crossed ITS line: the oval cars first
    d = np.array([l[4] for l in boot["pid"]])
    assert d[1::3].max() < d[0::3].min()
    cfg, _ = common.lmpc_config(g, N, max_batch=B, max_laps=32, max_lap_len=1024)
    with _capi.Context(cfg) as ctx:
        ro = rollout.BatchedRollouts(ctx, g["track"], seed=3, device_noise=True, tracks=tabs)
        loop = rollout.PerCarLMPC(ro, T_max=400, ext=40, device_commit=True)
        loop.seed(boot["pid"])
        out = loop.run()
        print("lap steps per car:", dict((b, (names[b], loop.lap_times[b])) for b in range(B)), "retired:", loop.retired, "status:", loop.last_status)
        assert not loop.retired and all(o is not None for o in out)
        assert not (np.asarray(loop.last_status) & ~_capi.ST_INEXACT).any()
        assert _same(ctx.tracks(), tk.rows_of(names))
        for b in range(B):
            x, u, q = ctx.store_read_lap(1, int(loop.last[b]))
            assert x.shape[0] == loop.lap_times[b][0] and q[0] == x.shape[0] - 1 and x[0, 4] < 1.0 and x[-1, 4] < TLs[b], (b, names[b], x.shape, q[0], x[0, 4], x[-1, 4])
        loop.close()
