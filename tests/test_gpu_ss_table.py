"""-m gpu: per-problem safe sets (lmpc_ss_set_lap_table) -- each problem of a batch selects its terminal set from its own row of laps.

The reference of a row is a context that holds only that row's laps and runs the shared rule (tests/ss_table_cases.py: fixture, problems, own_order); a problem with
a table row must give the BITS of that context -- selection, full step, on every solve kernel, after store edits, on the device path and inside rollout
sessions -- and the selection must equal oracle.terminal_components with sortedLapTime and cur_it per car.  N = 12, numSS_it in {2, 4}."""
import numpy as np
import pytest

from tests import common
from tests import ss_table_cases as cases

pytestmark = pytest.mark.gpu

N = cases.N
SEL_KEYS = ("ssSel", "qSel", "succ", "succU", "ztUsed", "selStart", "status")
STEP_KEYS = ("xPred", "uPred", "lambd", "ztNext", "ztuNext", "status", "iters", "ssSel", "qSel")


def _same(a, b, keys, rows, what):
    for k in keys:
        assert np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k])[rows]), (what, k)


def _contexts(g, rows, last, numSS_it, max_batch, runtime_kernel=False, **kw):
    """(table context with the six rows in force, its stored laps, one reference context per row)."""
    from racinglmpc_amd import _capi
    cfg, par = common.lmpc_config(g, N, max_batch=max_batch, numSS_it=numSS_it, **kw)
    ctx = _capi.Context(cfg, runtime_kernel=runtime_kernel)
    cases.fill_table_context(ctx, g)
    ctx.ss_set_lap_table(rows, last)
    stored = cases.read_laps(ctx)
    lt = [s[3] for s in stored]
    owns = []
    for r in range(rows.shape[0]):
        own = _capi.Context(cfg, runtime_kernel=runtime_kernel)
        cases.fill_own_context(own, g, stored, cases.own_order(rows[r], last[r], lt))
        owns.append(own)
    return ctx, stored, owns, par


@pytest.fixture(scope="module")
def g():
    return common.load_lmpc_golden()


@pytest.fixture(scope="module")
def six(built, g):
    ctx, stored, owns, par = _contexts(g, cases.ROWS4, cases.LAST4, 4, 1100)
    yield dict(ctx=ctx, stored=stored, owns=owns, par=par, p=cases.problems(g, 6))
    for c in [ctx] + owns:
        c.close()


def _sel(ctx, p):
    return ctx.select_batch(p["x0"], p["zt"], p["xPredPrev"], p["hasPred"], p["timeStep"])


def _step(ctx, p):
    return ctx.step_batch(p["x0"], p["xLin"], p["uLin"], p["uOld"], p["zt"], p["xPredPrev"], p["hasPred"], p["timeStep"])


def test_selection_equals_own_contexts_and_the_oracle(six, g):
    """select_batch, B = 6, six different rows: every output of problem b is bit for bit that of the context holding only row b's laps; ssSel / qSel / succ / succU
    equal oracle.terminal_components exactly; no problem raises LMPC_ST_WINDOW; the problems cover crossing and non-crossing predictions and the wrap branch."""
    p, TL = six["p"], float(g["trackLength"])
    crossed = (p["xPredPrev"][:, :, 4] > TL).any(1)
    assert crossed.any() and not crossed.all() and (p["timeStep"] != 0).all() and (p["zt"][:, 4] - p["x0"][:, 4] > TL / 2).sum() == 1
    out = _sel(six["ctx"], p)
    assert not out["status"].any(), out["status"]
    lt = [s[3] for s in six["stored"]]
    for b in range(6):
        ref = _sel(six["owns"][b], p)
        _same(out, ref, SEL_KEYS, b, "row %d" % b)
        SSsel, Qsel, Succ, SuccU, ok = cases.oracle_selection(six["stored"], cases.own_order(cases.ROWS4[b], cases.LAST4[b], lt), p, b, TL, 4, 12)
        assert ok
        assert np.array_equal(out["ssSel"][b], SSsel) and np.array_equal(out["qSel"][b], Qsel) and np.array_equal(out["succ"][b], Succ) and np.array_equal(out["succU"][b], SuccU), b
    # the same laps listed in both orders (rows 2 and 3) select the same points: only `last` tells the two rows apart
    p2 = {k: np.repeat(v[2:3], 6, axis=0) for k, v in p.items()}
    o2 = _sel(six["ctx"], p2)
    assert np.array_equal(o2["ssSel"][2], o2["ssSel"][3]) and np.array_equal(o2["selStart"][2], o2["selStart"][3])
    assert not np.array_equal(o2["qSel"][2], o2["qSel"][3])          # (problem 2 crosses the line: lap 2 is the latest of row 2 and of no lap of row 3)


def test_full_step_equals_own_contexts_and_the_oracle_optimum(six, g):
    """step_batch on the six problems (four waves per QP): xPred, uPred, lambda, ztNext, ztuNext, status, iters bit for bit those of the own-context runs at the same
    batch size; xPred, uPred within 1e-6 of the oracle's certified optimum of the QP the oracle assembles from the per-car selection."""
    from oracle import lmpc_oracle as orc
    p, ctx, TL = six["p"], six["ctx"], float(g["trackLength"])
    assert ctx.solver_waves(6) == 4 and ctx.solver_kind == 0
    out = _step(ctx, p)
    assert not (out["status"] & ~64).any(), out["status"]
    lt = [s[3] for s in six["stored"]]
    pt = np.array(g["track"]); xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    nxu = 6 * (N + 1) + 2 * N
    for b in range(6):
        _same(out, _step(six["owns"][b], p), STEP_KEYS, b, "row %d" % b)
        SSsel, Qsel, _, _, _ = cases.oracle_selection(six["stored"], cases.own_order(cases.ROWS4[b], cases.LAST4[b], lt), p, b, TL, 4, 12)
        A, B, C = orc.compute_ltv_dynamics([xP] * 4, [uP] * 4, [0, 1, 2, 3], pt, p["xLin"][b], p["uLin"][b], N)
        P, q, Ao, lo, up = orc.assemble_lmpc_qp(six["par"], A, B, C, p["x0"][b], p["uOld"][b], SSsel.T, Qsel)
        ex, cert = orc.osqp_solve_exact(P, q, Ao, lo, up, want=1e-8)
        assert cert < 1e-7, (b, cert)
        r2 = orc.dense_ipm_solve(P, q, Ao, lo, up)           # (the rule of common.compare_with_oracle: the nearer of the oracle's two certified optima)
        w = np.concatenate([out["xPred"][b].ravel(), out["uPred"][b].ravel()])
        err = min(float((np.abs(w - o[:nxu]) / (1 + np.abs(o[:nxu]))).max()) for o in (ex.x, r2.x))
        print("row %d: |xu - z*| / (1 + |z*|) %.2e" % (b, err))
        assert err < common.TOL_XU, (b, err)


@pytest.mark.parametrize("route", ["2 waves", "1 wave", "runtime kernel"])
def test_every_kernel_route_serves_the_table(built, g, six, route):
    """The step on the two-wave, the one-wave and the runtime-(N, S) kernel, the six rows cycled over the batch: a fixed subset with every row in it equals the
    own-context runs at the same batch size, bit for bit."""
    if route == "runtime kernel":
        B = 66
        ctx, stored, owns, _ = _contexts(g, cases.ROWS2, cases.LAST2, 2, B, runtime_kernel=True)
        ctx.ss_set_lap_table(np.tile(cases.ROWS2, (B // 6, 1)), np.tile(cases.LAST2, B // 6))
        waves, kind = 1, 2
    else:
        B = 300 if route == "2 waves" else 1098
        ctx, owns = six["ctx"], six["owns"]
        ctx.ss_set_lap_table(np.tile(cases.ROWS4, (B // 6, 1)), np.tile(cases.LAST4, B // 6))
        waves, kind = (2 if route == "2 waves" else 1), 0
    try:
        assert ctx.solver_waves(B) == waves and ctx.solver_kind == kind and owns[0].solver_waves(B) == waves
        p = cases.problems(g, B)
        out = _step(ctx, p)
        assert not (out["status"] & ~64).any()
        for r in range(6):
            ref = _step(owns[r], p)
            _same(out, ref, STEP_KEYS, [r, r + 6, B - 6 + r], "%s, row %d" % (route, r))
    finally:
        if route == "runtime kernel":
            for c in [ctx] + owns:
                c.close()
        else:
            ctx.ss_set_lap_table(cases.ROWS4, cases.LAST4)


def test_n_and_argument_errors(six, g):
    """n = 1 serves every problem; B != n is LMPC_E_ARG with a message and the next correct call works; every argument error leaves the table in force; n = 0 after a
    table restores the shared selection bit for bit."""
    from racinglmpc_amd import _capi
    import ctypes as C
    ctx, p, lib = six["ctx"], six["p"], six["ctx"].lib
    shared_ctx_cfg, _ = common.lmpc_config(g, N, max_batch=8)
    fresh = _capi.Context(shared_ctx_cfg)
    try:
        cases.fill_table_context(fresh, g)
        shared = _sel(fresh, p)                          # a context that never had a table
        ctx.ss_set_lap_table(cases.ROWS4[1:2], cases.LAST4[1:2])
        one = _sel(ctx, p)
        ref = _sel(six["owns"][1], p)
        _same(one, ref, SEL_KEYS, slice(None), "n = 1")
        ctx.ss_set_lap_table(cases.ROWS4, cases.LAST4)
        p5 = {k: v[:5] for k, v in p.items()}
        with pytest.raises(_capi.LmpcError) as e:
            _sel(ctx, p5)
        assert "lmpc_ss_set_lap_table holds 6 rows" in str(e.value) and "B = 5" in str(e.value)
        with pytest.raises(_capi.LmpcError):
            _step(ctx, p5)
        _same(_sel(ctx, p), _sel(six["owns"][0], p), SEL_KEYS, 0, "after a refused batch")

        def in_force():
            rows, last = ctx.ss_lap_table()
            return np.array_equal(rows, cases.ROWS4) and np.array_equal(last, cases.LAST4)
        assert in_force()
        bad = np.array([[0, 1, 2, 6]], np.int32); neg = np.array([[0, -1, 2, 3]], np.int32); ok = cases.ROWS4[:1].copy()
        l_hi = np.array([6], np.int32); l_lo = np.array([-2], np.int32)
        for n, laps, last in ((1, bad, None), (1, neg, None), (1, ok, l_hi), (1, ok, l_lo), (-1, ok, None), (1, None, None)):
            rc = lib.lmpc_ss_set_lap_table(ctx._h, n, None if laps is None else laps.ctypes.data, None if last is None else last.ctypes.data)
            assert rc == -1 and in_force(), (n, laps, last)
        mcfg, _ = common.mpc_config(g, N, max_batch=4)
        with _capi.Context(mcfg) as plain:               # numSS_it = 0
            assert lib.lmpc_ss_set_lap_table(plain._h, 1, ok.ctypes.data, None) == -1
            assert lib.lmpc_ss_set_lap_table(plain._h, 0, None, None) == 0
        # last = NULL: the context-wide rule -- the latest lap is the last one stored (lap 5)
        ctx.ss_set_lap_table(cases.ROWS4, None)
        rows, last = ctx.ss_lap_table()
        assert np.array_equal(rows, cases.ROWS4) and last is None
        nolast = _sel(ctx, p)
        assert np.array_equal(nolast["qSel"][5], _sel(six["owns"][5], p)["qSel"][5])      # (row 5 holds lap 5 and had last = 5)
        ctx.ss_set_lap_table(None)
        n = C.c_int(-1)
        assert lib.lmpc_ss_get_lap_table(ctx._h, C.byref(n), None, None, 0) == 0 and n.value == 0
        _same(_sel(ctx, p), shared, SEL_KEYS, slice(None), "n = 0")
        _same(_step(ctx, p), _step(fresh, p), STEP_KEYS, slice(None), "n = 0, step")
    finally:
        fresh.close()
        ctx.ss_set_lap_table(cases.ROWS4, cases.LAST4)


def test_store_edits_after_set_reach_the_next_launch(built, g):
    """The table names laps, not snapshots: after ss_add_point, ss_extend_lap, ss_truncate_lap, ss_replace_lap on a named lap, a new ss_add_trajectory and a growth
    of both store dimensions (initial capacity 8 laps x 512 rows) the next select_batch equals the own-context result after the same edit."""
    from racinglmpc_amd import _capi
    rows = np.array([[0, 1, 2, 5], [2, 4, 4, 5], [3, 2, 1, 0]], np.int32); last = np.array([5, 5, 2], np.int32)
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=8, max_lap_len=512)
    p = {k: v[[2, 3, 5]] for k, v in cases.problems(g, 6).items()}          # (problems near the line: they select from the rows the edits touch)
    laps, ext = cases.fixture_laps(g)
    ctx = _capi.Context(cfg)
    try:
        cases.fill_table_context(ctx, g)
        ctx.ss_set_lap_table(rows, last)
        lt = [ctx.ss_lap_time(l) for l in range(6)]

        def check(what):
            stored = cases.read_laps(ctx)
            out = _sel(ctx, p)
            for r in range(3):
                with _capi.Context(cfg) as own:
                    cases.fill_own_context(own, g, stored, cases.own_order(rows[r], last[r], lt))
                    _same(out, _sel(own, p), SEL_KEYS, r, "%s, row %d" % (what, r))
            return out
        before = check("as set")
        xe, ue = np.array(g["xPID"])[360:362].copy(), np.array(g["uPID"])[360:362]
        xe[:, 4] -= float(g["trackLength"])
        ctx.ss_add_point(xe[0], ue[0])                    # (lap 5, the last one stored)
        check("ss_add_point")
        ctx.ss_extend_lap(2, np.array(g["lapx1"])[30:40], np.array(g["lapu1"])[30:40])
        check("ss_extend_lap")
        ctx.ss_truncate_lap(2, 262)
        check("ss_truncate_lap")
        x1, u1, q1 = ctx.store_read_lap(1, 1)
        ctx.ss_replace_lap(1, x1 * (1 + 1e-9), u1, q1 + 1.0)
        moved = check("ss_replace_lap")
        assert not np.array_equal(moved["qSel"][0], before["qSel"][0])     # (row 0 names lap 1: the edit is seen)
        ctx.ss_add_trajectory(*laps[0])                   # lap 6: the context-wide latest changes, the rows' own `last` does not
        check("ss_add_trajectory")
        for _ in range(3):                                # 10 laps > 8, and a lap of 612 rows > 512: both store dimensions grow
            ctx.ss_add_trajectory(*laps[1])
        ctx.ss_extend_lap(2, np.tile(np.array(g["lapx1"])[39:40], (350, 1)), np.tile(np.array(g["lapu1"])[39:40], (350, 1)))
        assert ctx.ss_num_laps() == 10 and ctx.ss_lap_rows(2) == 612
        check("store growth")
    finally:
        ctx.close()


def test_device_path_equals_host_path(six):
    """step_batch_dev with a table: every output equals step_batch."""
    ctx, p = six["ctx"], six["p"]
    host = _step(ctx, p)
    args, keep = ctx.step_dev_buffers(p)
    try:
        ctx.step_batch_dev(6, args)
        dev = ctx.step_dev_fetch(args, 6)
    finally:
        for q in keep:
            ctx.dev_free(q)
    _same(dev, host, STEP_KEYS, slice(None), "step_batch_dev")


def test_rollout_session_with_three_rows(built, g):
    """A session of three cars with three different rows and device noise, run until every car has crossed the line; after 10 steps a `set` with the wrong n makes
    rollout_run return LMPC_E_ARG before any launch of the step (the library's step count stays at 10), and after a correct `set` the session goes on.  X, U logs up to
    each car's crossing, the crossing step and the status word equal, bit for bit, those of one-car sessions on own contexts with the car's noise offset.
    (About 130 steps, not 25: a session opens with the reference's first terminal target zt = [0, 0, 0, 0, 10, 0], LMPC.__init__ :330, so the cars start near s = 8 --
    steps 100, 104, 108 of LMPC lap 4 of the golden closed loop -- and have eleven metres to go; a car started next to the line brakes for that target.)
    Rows: the latest lap in the row; last = -1; last = -1 on a row that holds the lap the shared rule would call the latest (lap 5)."""
    from racinglmpc_amd import _capi
    rows, last = np.array([[1, 1, 1, 5], [1, 1, 1, 1], [1, 1, 5, 5]], np.int32), np.array([5, -1, -1], np.int32)
    cfg, _ = common.lmpc_config(g, N, max_batch=4)
    t0 = np.array([100, 104, 108])
    assert (np.array(g["all_lap"])[t0] == 4).all() and (np.array(g["all_t"])[t0] == t0).all()
    x0 = np.array(g["all_x0"])[t0]; xl = np.array(g["all_xLin"])[t0]; ul = np.array(g["all_uLin"])[t0]
    T, SEED, CUT = 200, 78, 10
    ctx = _capi.Context(cfg)
    owns = []
    try:
        cases.fill_table_context(ctx, g)
        stored = cases.read_laps(ctx); lt = [s[3] for s in stored]
        ctx.ss_set_lap_table(rows, last)
        ctx.rollout_set_noise(True, SEED, 0, 0)
        ctx.rollout_begin(x0, x0, xl, ul, None, T_max=T)
        t, _ = ctx.rollout_run(CUT)
        assert t == CUT
        ctx.ss_set_lap_table(rows[:2], last[:2])
        with pytest.raises(_capi.LmpcError) as e:
            ctx.rollout_run(T)
        assert "holds 2 rows" in str(e.value)
        ctx.ss_set_lap_table(rows, last)
        t, _ = ctx.rollout_run(1)
        assert t == CUT + 1                                   # (the library's own count: the refused call took no step)
        t, _ = ctx.rollout_run(T)
        X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
        ctx.rollout_end()
        print("session: steps", t, "done", done, "status", st)
        assert (done >= 0).all() and (done > CUT + 1).all() and not (st & ~64).any(), (done, st)
        for b in range(3):
            own = _capi.Context(cfg); owns.append(own)
            cases.fill_own_context(own, g, stored, cases.own_order(rows[b], last[b], lt))
            own.rollout_set_noise(True, SEED, 0, b)
            own.rollout_begin(x0[b:b + 1], x0[b:b + 1], xl[b:b + 1], ul[b:b + 1], None, T_max=T)
            own.rollout_run(CUT); own.rollout_run(1)
            to, _ = own.rollout_run(T)
            Xo, Uo, _, done_o, st_o, _, _ = own.rollout_fetch(0, to)
            own.rollout_end()
            n = int(done[b])
            assert done_o[0] == done[b] and st_o[0] == st[b] and np.array_equal(Xo[:n, 0], X[:n, b]) and np.array_equal(Uo[:n, 0], U[:n, b]), b
    finally:
        for c in [ctx] + owns:
            c.close()


def test_last_decides_the_current_lap_not_the_shared_rule(six, g):
    """One problem whose prediction crosses the line (problem 2) on six rows that all hold lap 5, the lap the shared rule calls the latest: with last = -1 or a lap
    that is not in the row no entry takes the "current lap" branch, with last = 5 lap 5 does.  Bit for bit the own contexts, and exactly the oracle."""
    rows = np.array([[2, 4, 4, 5], [1, 1, 3, 5], [0, 1, 2, 5], [0, 5, 2, 3], [5, 5, 1, 1], [0, 3, 4, 5]], np.int32)
    last = np.array([-1, 4, 5, -1, -1, 2], np.int32)
    from racinglmpc_amd import _capi
    ctx, TL = six["ctx"], float(g["trackLength"])
    p = {k: np.repeat(v[2:3], 6, axis=0) for k, v in six["p"].items()}
    lt = [s[3] for s in six["stored"]]
    cfg, _ = common.lmpc_config(g, N, max_batch=8)
    try:
        ctx.ss_set_lap_table(rows, last)
        out = _sel(ctx, p)
        assert not out["status"].any()
        for r in range(6):
            order = cases.own_order(rows[r], last[r], lt)
            with _capi.Context(cfg) as own:
                cases.fill_own_context(own, g, six["stored"], order)
                _same(out, _sel(own, p), SEL_KEYS, r, "row %d" % r)
            SSsel, Qsel, Succ, SuccU, ok = cases.oracle_selection(six["stored"], order, p, r, TL, 4, 12)
            assert ok and np.array_equal(out["ssSel"][r], SSsel) and np.array_equal(out["qSel"][r], Qsel) and np.array_equal(out["succ"][r], Succ), r
        ctx.ss_set_lap_table(rows, None)                       # the shared rule instead: lap 5 is the current lap of every row
        shared = _sel(ctx, p)
        for r in (0, 1, 3, 4, 5):
            assert not np.array_equal(shared["qSel"][r], out["qSel"][r]), r
        assert np.array_equal(shared["qSel"][2], out["qSel"][2])
    finally:
        ctx.ss_set_lap_table(cases.ROWS4, cases.LAST4)


def test_per_car_lmpc_closed_loop(built, g):
    """PerCarLMPC, 3 cars, 2 generations, seeded from three different PID laps: every car's laps equal those of a one-car PerCarLMPC with that car's noise offset, and
    every QP of generation 2 selected only rows of its own car's laps."""
    from racinglmpc_amd import _capi, rollout
    track = np.array(g["track"]); TL = float(g["trackLength"])
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=16, max_lap_len=1024)
    SEED, T_MAX, EXT = 5, 400, 40

    def pid_laps(ctx, vt, car0):
        ro = rollout.BatchedRollouts(ctx, track, seed=SEED, device_noise=True)
        ro.noise_shard = (car0, car0 + len(vt), 3)
        return ro, ro.run_pid_laps(vt, max_steps=700, keep_invalid=True)

    vt = np.array([0.75, 0.8, 0.85])
    ctx = _capi.Context(cfg)
    others = []
    try:
        ro, seeds = pid_laps(ctx, vt, 0)
        assert all(l[4] >= 0 and l[5] == 0 for l in seeds) and len({l[4] for l in seeds}) == 3
        ctx.debug_rollout_capture(True)
        loop = rollout.PerCarLMPC(ro, T_max=T_MAX, ext=EXT)
        loop.seed(seeds)
        own_rows = []                       # generation 2: selected rows per step and car

        gen1 = loop.run()
        assert not loop.retired and all(l is not None for l in gen1), (loop.retired, loop.last_status, loop.last_done)
        # generation 2 step by step, to look at every QP's selection
        rows2, last2 = ro.ss_table, ro.ss_last           # (what the loop hands to the context in front of generation 2's session)
        assert rows2.shape == (3, 4) and last2.tolist() == [3, 4, 5]
        for b in range(3):
            assert set(rows2[b].tolist()) <= {b, 3 + b}, rows2          # car b: its PID lap and its first LMPC lap, nothing of the others
        real_run = ctx.rollout_run

        def stepwise(n):
            t_end = min(T_MAX, ctx._ro_t + n)
            while True:
                t, nd = real_run(1)
                q = ctx.debug_rollout_qp(0, 3, selection=True)
                own_rows.append(q["ssSel"].copy())
                if nd >= 3 or t >= t_end:
                    return t, nd
        ctx.rollout_run = stepwise
        try:
            gen2 = loop.run()
        finally:
            del ctx.rollout_run
        assert not loop.retired and all(l is not None for l in gen2), (loop.retired, loop.last_status)
        stored = cases.read_laps(ctx)
        for b in range(3):
            mine = np.concatenate([stored[l][0] for l in (b, 3 + b)])
            keys = {r.tobytes() for r in mine}
            for sel in own_rows:
                assert all(r.tobytes() in keys for r in sel[b]), b
        for b in range(3):
            c1 = _capi.Context(cfg); others.append(c1)
            ro1, s1 = pid_laps(c1, vt[b:b + 1], b)
            assert np.array_equal(s1[0][0], seeds[b][0])
            l1 = rollout.PerCarLMPC(ro1, T_max=T_MAX, ext=EXT)
            l1.seed(s1)
            for want in (gen1, gen2):
                got = l1.run()
                assert got[0] is not None and np.array_equal(got[0][0], want[b][0]) and np.array_equal(got[0][1], want[b][1]), b
        print("lap times per car:", loop.lap_times)
    finally:
        for c in [ctx] + others:
            c.close()
