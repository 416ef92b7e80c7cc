"""-m gpu: every solve route at the limits of horizon and safe-set size (tests/envelope_cases.py: the table, the problem sets, the stores, the oracle records).

Per case, on every route production takes for it (envelope_cases.routes: four waves, two waves, one wave with [A|B] in LDS / in global memory / LMPC_NO_ABG, the
runtime kernel), with the 64 problems P in rows 0 .. 63 of the batch and other problems behind them:
  * the route is asserted (Context.solver_waves, solver_kind, solver_lds): the case's class -- use_abg, multi-wave kernels or none, four waves throughout -- is
    stated in the table and checked against what the library reports;
  * every status word of P is 0;  A, B, C, ssSel, qSel and status are bit-identical on every route of the case;
  * xPred, uPred and ztNext agree with the case's first route to test_gpu_routes.TOL_ROUTE; the epilogue identities (test_gpu_routes._epilogue_fails) hold on each
    route's own outputs;
  * against the oracle on 8 (N >= 41 or S >= 378) or 16 problems of P: A, B, C to common.TOL_ABC, selections identical, (x, u) at the certified optimum to
    common.TOL_XU, zt by common.compare_with_oracle's rule.  With an odd number of points per lap (29, 59, 63) the reference's window has one column more per lap
    than its QP and the reference cannot run; the records then hold the first points-per-lap columns of the reference's window (oracle_pool.select_laps) -- the
    window's start is the reference's, the cut restates the library's own rule, so the selection comparison is independent for the start only.
Then the crossing count of the Q-function shift at N = 63 / 64 (65 predicted rows: one more than a wave has lanes), rollout sessions at N = 2 / 64 against the
host-stepped loop, and the boundary of the supported range: every (N, numSS_points) pair either solves P or is refused with LMPC_E_ARG and a message naming the limit.

LMPC_ENVELOPE_PROFILE=<file>: the per-route figures are appended to that file, one JSON object per line (profiles/envelope_corners.json is made of them)."""
import json
import os

import numpy as np
import pytest

from tests import common
from tests import envelope_cases as ec
from tests.test_gpu_routes import SAME_KEYS, TOL_ROUTE, _epilogue_fails, _mpc_compare

pytestmark = pytest.mark.gpu

R = slice(0, ec.P_SIZE)


def _step(ctx, inp):
    return ctx.step_batch(inp["x0"], inp["xLin"], inp["uLin"], inp["uOld"], zt=inp["zt"] if ctx.S else None, timeStep=inp["timeStep"] if ctx.S else None)


def _assert_class(c, ctx, lds, rt):
    """The case's class as the table states it, against the library's own constants."""
    what = ec.case_id(c)
    n_cu = lds["n_cu"]
    if rt:
        assert ctx.solver_kind == 2 and lds["lds_mw"] == 0 and lds["lds_1w_abg"] == 0 and lds["lds_1w"] + 1024 <= ec.LDS_CU, (what, lds)
        return
    assert ctx.solver_kind in (0, 1), (what, ctx.solver_kind)
    assert (lds["lds_1w_abg"] > 0) == c.abg and (not c.abg or ec.LDS_CU // lds["lds_1w"] == c.fit), (what, lds)
    assert (lds["lds_mw"] > 0) == (c.mw != "none"), (what, lds)
    assert lds["lds_1w"] <= ec.LDS_CU, (what, lds)
    throughout = 2 * (lds["lds_1w_abg"] or lds["lds_1w"]) > ec.LDS_CU
    assert throughout == (c.mw == "throughout" or (c.mw == "none" and 2 * lds["lds_1w"] > ec.LDS_CU)), (what, lds)
    # the whole staircase of the case: four waves up to one QP per CU (at every batch size in the "throughout" class), one wave everywhere without multi-wave kernels
    want = {"full": [4, 4, 2 if c.two else 1, 1], "throughout": [4, 4, 4, 4], "none": [1, 1, 1, 1]}[c.mw]
    got = [ctx.solver_waves(b) for b in (1, n_cu, n_cu + 1, 1 << 20)]
    assert got == want, (what, got, want)


@pytest.mark.parametrize("c", ec.CASES, ids=[ec.case_id(c) for c in ec.CASES])
def test_every_route_of_every_corner(built, c):
    N, S = c.N, ec.S_of(c)
    res, left_out = ec.certified(ec.oracle_records(c))          # forked workers, before this test makes a HIP context
    outs, fails, prof = {}, [], []
    first = None
    for name, B, waves, knobs, rt in ec.routes(c, _n_cu()):
        what = "%s, %s, batch %d" % (ec.case_id(c), name, B)
        ctx = ec.context(c, B, knobs, rt)
        try:
            lds = ctx.solver_lds()
            _assert_class(c, ctx, lds, rt)
            assert ctx.solver_waves(B) == waves and ctx.solver_kind == (2 if rt else 0 if (N, S) in _builtin() else 1), (what, ctx.solver_waves(B), ctx.solver_kind)
            if "global" in name:            # [A|B] from global memory: the batch is beyond the QPs that fit the CUs with it in LDS (lmpc_capi.hip, launch_solve)
                assert lds["lds_1w_abg"] > 0 and B > (ec.LDS_CU // lds["lds_1w"]) * lds["n_cu"], (what, lds)
            elif c.abg and not rt and not knobs and waves == 1:      # ... and a batch that fits keeps it in LDS
                assert B <= (ec.LDS_CU // lds["lds_1w"]) * lds["n_cu"], (what, lds)
            out = _step(ctx, ec.problems(N, B))
            sel = ctx.select_batch(ec.problems(N)["x0"], ec.problems(N)["zt"], timeStep=ec.problems(N)["timeStep"]) if S else None
        finally:
            ctx.close()
        outs[name] = out
        if first is None:
            first = name
        ref = outs[first]
        print(what)
        if not np.all(out["status"][R] == 0):
            fails.append("%s: status %s" % (what, np.unique(out["status"][R], return_counts=True)))
        same = [k for k in SAME_KEYS if not np.array_equal(out[k][R], ref[k][R])]
        if same:
            fails.append("%s: %s not bit-identical to %s" % (what, ", ".join(same), first))
        bad = _epilogue_fails(out, sel, N, S)
        if bad:
            fails.append("%s: epilogue: %s" % (what, ", ".join(bad)))
        dxu = max(float(np.abs(out["xPred"][R] - ref["xPred"][R]).max()), float(np.abs(out["uPred"][R] - ref["uPred"][R]).max()))
        dzt = float((np.abs(out["ztNext"][R] - ref["ztNext"][R]) / (1 + np.abs(ref["ztNext"][R]))).max())
        print("    |xu - %s| %.2e, |zt - .| / (1 + |zt|) %.2e; iterations mean %.2f max %d" % (first, dxu, dzt, out["iters"][R].mean(), out["iters"][R].max()))
        if not (dxu < TOL_ROUTE and dzt < TOL_ROUTE):
            fails.append("%s: |xu| differs from %s by %.2e, zt by %.2e" % (what, first, dxu, dzt))
        try:
            worst = (common.compare_with_oracle if S else _mpc_compare)(out, res, N, what)
        except AssertionError as e:
            fails.append("%s: oracle: %s" % (what, e))
            worst = dict(abc=float("nan"), xu=float("nan"), zt=float("nan"))
        prof.append(dict(case=[c.N, c.L, c.ppl], N=N, S=S, route=name, batch=B, waves=waves, lds_1w=lds["lds_1w"], lds_1w_abg=lds["lds_1w_abg"], lds_mw=lds["lds_mw"],
                         iters_mean=round(float(out["iters"][R].mean()), 3), iters_max=int(out["iters"][R].max()), problems_compared=len(res), left_out=left_out,
                         worst_abc=float(worst["abc"]), worst_xu=float(worst["xu"]), worst_zt=float(worst["zt"]), dxu_first_route=dxu, dzt_first_route=dzt))
    if os.environ.get("LMPC_ENVELOPE_PROFILE"):
        with open(os.environ["LMPC_ENVELOPE_PROFILE"], "a") as f:
            for p in prof:
                f.write(json.dumps(p) + "\n")
    assert not fails, "\n".join(fails)


_N_CU = []


def _n_cu():
    """CUs of the device (lmpc_solver_lds of a small built-in context): the batches of the routes follow it (envelope_cases.routes)."""
    if not _N_CU:
        from racinglmpc_amd import _capi
        ctx = _capi.Context(common.mpc_config(ec.golden(), 12, max_batch=1)[0])
        try:
            _N_CU.append(ctx.solver_lds()["n_cu"])
        finally:
            ctx.close()
        if _N_CU[0] < 96:
            pytest.skip("a device of %d CUs: the batch of 96 is not below one QP per CU" % _N_CU[0])
    return _N_CU[0]


def _builtin():
    from racinglmpc_amd import build
    return build.BUILTIN


# ---- the crossing count of the Q-function shift (selectPoints :502-512) at 64 and 65 predicted rows --------------------------------------------------------------

def _crossing_inputs(N):
    """16 problems: 4 of P (non-zero timeStep) x 4 previous predictions -- no row beyond the line, only row N, rows N - 1 and N, all rows."""
    TL = ec.golden()["TL"]
    P = ec.problems(N)
    rows = [1, 9, 22, 40]
    inp = {k: np.repeat(P[k][rows], 4, axis=0) for k in ("x0", "zt", "timeStep")}
    inp["timeStep"] = (inp["timeStep"] + 3).astype(np.int32)
    xp = np.repeat(np.concatenate([P["xLin"][rows][:, 1:], P["zt"][rows][:, None]], axis=1), 4, axis=0)      # (B, N + 1, 6): a plausible previous prediction
    xp[:, :, 4] = np.minimum(xp[:, :, 4], TL - 0.5)
    beyond = [[], [N], [N - 1, N], list(range(N + 1))]
    for i in range(16):
        for r in beyond[i % 4]:
            xp[i, r, 4] = TL + 0.01 * (r + 1)
    inp["xPredPrev"] = xp
    inp["hasPred"] = np.ones(16, np.int32)
    inp["xLin"] = np.repeat(P["xLin"][rows], 4, axis=0); inp["uLin"] = np.repeat(P["uLin"][rows], 4, axis=0); inp["uOld"] = np.repeat(P["uOld"][rows], 4, axis=0)
    return inp, [len(beyond[i % 4]) for i in range(16)]


@pytest.mark.parametrize("N", [63, 64])
def test_crossing_count_at_the_longest_horizons(built, N):
    """select_batch with hasPred = 1: qSel equals the oracle's selection with that prediction on the four-wave kernel (16 problems), the one-wave kernel (the 16 tiled
    beyond one QP per CU: 272) and the runtime kernel; four safe-set laps, so laps 0 .. 2 are older than cur_it - 1 (shift by their Q-function's first value) and lap 3 is the latest
    (shift by timeStep + N - crossed).  The shifts differ between the four predictions, so a miscount shows."""
    from tests import oracle_pool
    c = next(k for k in ec.CASES if (k.N, k.L, k.ppl) == (N, 4, 12))
    g = ec.golden()
    inp, crossed = _crossing_inputs(N)
    pid = (g["xPID"], g["uPID"])
    res = oracle_pool.oracle_batch(ec.params(c), g["track"], g["TL"], [pid] * 4, N, inp, range(16), ss_laps=ec.ss_laps(4), ppl=12)
    want = np.stack([r["Qsel"] for r in res]); want_ss = np.stack([r["SSsel"].T for r in res])
    # the four predictions of a problem give four different Q-function rows, except that "no row beyond" is the unshifted one
    for p in range(4):
        q = want[4 * p:4 * p + 4]
        assert len({tuple(row) for row in q}) == 4, p
        assert np.array_equal(q[1][36:] - q[0][36:], np.full(12, float(inp["timeStep"][4 * p] + N - 1)))      # lap 3 (the latest), one row beyond: timeStep + N - 1
        assert np.array_equal(q[3][36:] - q[0][36:], np.full(12, float(inp["timeStep"][4 * p] - 1)))          # every row beyond: N - (N + 1)
    fails = []
    for name, tile, rt in (("4 waves", 1, False), ("1 wave", _n_cu() // 16 + 1, False), ("runtime kernel", 1, True)):
        B = 16 * tile
        ctx = ec.context(c, B, {}, rt)
        try:
            assert ctx.solver_waves(B) == (4 if tile == 1 and not rt else 1) and ctx.solver_kind == (2 if rt else 1)
            t = lambda a: np.tile(a, (tile,) + (1,) * (a.ndim - 1))
            sel = ctx.select_batch(t(inp["x0"]), t(inp["zt"]), xPredPrev=t(inp["xPredPrev"]), hasPred=t(inp["hasPred"]), timeStep=t(inp["timeStep"]))
        finally:
            ctx.close()
        for k in range(tile):
            blk = slice(16 * k, 16 * k + 16)
            if not (np.array_equal(sel["qSel"][blk], want) and np.array_equal(sel["ssSel"][blk], want_ss) and np.all(sel["status"][blk] == 0)):
                bad = [i for i in range(16) if not np.array_equal(sel["qSel"][blk][i], want[i])]
                fails.append("N = %d, %s, rows %d..: qSel differs from the oracle on predictions with %s rows beyond the line" % (N, name, 16 * k, [crossed[i] for i in bad]))
                break
    assert not fails, "\n".join(fails)


# ---- rollout sessions at the shortest and the longest horizon --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [2, 64])
def test_mpc_sessions_at_the_ends_of_the_horizon_range(built, N):
    """LTV-MPC sessions (lmpc_rollout_begin_mpc) of 9 cars -- 8 (N + 1) threads per car in the shift kernel: 520 at N = 64, one car straddles work-groups of 256 and the
    last work-group is partial -- over 12 steps: the X, U, Xglob logs are bit-identical to the host-stepped loop over step_batch + plant_step_batch
    (tests/test_gpu_mpc_stages._host_stepped), and with parking on (car 4 parked from the start) the logs of the other cars are those same rows."""
    from racinglmpc_amd import _capi
    from tests.test_gpu_mpc_stages import X0, _host_stepped
    c = next(k for k in ec.CASES if (k.N, k.L) == (N, 0))
    g = ec.golden()
    B, T = 9, 12
    x0 = np.tile(X0, (B, 1)); x0[:, 5] = np.linspace(-0.15, 0.15, B); x0[:, 0] = 0.5 + 0.01 * (np.arange(B) % 7)
    form = dict(xLin0=np.tile(g["xPID"][None, 0:N + 1], (B, 1, 1)), uLin0=np.tile(g["uPID"][None, 0:N], (B, 1, 1)))
    noise = np.random.default_rng(31).standard_normal((T, B, 3))
    logs = {}
    for park in (None, (0, [4])):
        ctx = ec.context(c, B)
        try:
            assert ctx.solver_kind == 1 and ctx.solver_waves(B) == 4
            ctx.rollout_set_parking(*(park or (0, None)))
            ctx.rollout_begin_mpc(x0, x0, noise, **form)
            t, nd = ctx.rollout_run(T)
            X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
            ctx.rollout_end()
            assert t == T and np.all((st & ~64) == 0), (t, st)
            logs[park is not None] = (X, U, G)
            if park is None:
                Xh, Uh, Gh = _host_stepped(ctx, x0, form, noise)
        finally:
            ctx.close()
    X, U, G = logs[False]
    bad = [k for k in range(T) if not (np.array_equal(X[k], Xh[k]) and np.array_equal(U[k], Uh[k]) and np.array_equal(G[k], Gh[k]))]
    assert not bad, "N = %d: steps %s of the session differ from the host-stepped loop" % (N, bad)
    live = [b for b in range(B) if b != 4]
    Xp, Up, Gp = logs[True]
    bad = [k for k in range(T) if not (np.array_equal(Xp[k][live], X[k][live]) and np.array_equal(Up[k][live], U[k][live]) and np.array_equal(Gp[k][live], G[k][live]))]
    assert not bad, "N = %d, car 4 parked: steps %s of the live cars differ from the session without parking" % (N, bad)
    assert np.isfinite(X).all() and np.abs(X[-1, :, 5]).max() < 0.4


# ---- the boundary of the supported range ------------------------------------------------------------------------------------------------------------------------

E_ARG = -1          # LMPC_E_ARG (include/lmpc_hip.h)


def _refused(cfg, runtime_kernel, *words):
    from racinglmpc_amd import _capi
    with pytest.raises(_capi.LmpcError) as e:
        _capi.Context(cfg, runtime_kernel=runtime_kernel).close()
    msg = str(e.value)
    assert msg.startswith("liblmpc_hip error %d:" % E_ARG), msg
    assert all(w in msg for w in words), (msg, words)
    return msg


OUTSIDE = [
    # (N, numSS_it, numSS_points, runtime kernel, words of the message)
    (1, 4, 48, False, ("cfg->N >= 2",)),
    (65, 4, 48, False, ("cfg->N <= LMPC_MAX_N",)),
    (1, 4, 48, True, ("cfg->N >= 2",)),
    (65, 0, 0, True, ("cfg->N <= LMPC_MAX_N",)),
    (12, 33, 396, False, ("cfg->numSS_it <= LMPC_MAX_USED_LAPS",)),
    (12, 1, 385, False, ("cfg->numSS_points <= LMPC_MAX_SS_POINTS",)),
    (12, 5, 385, False, ("cfg->numSS_points <= LMPC_MAX_SS_POINTS",)),
    (12, 6, 384, False, ("cfg->numSS_points / cfg->numSS_it + 1 <= WAVE",)),          # 64 points per lap: the selection's window is points per lap + 1 rows, one per lane
    (12, 1, 64, True, ("cfg->numSS_points / cfg->numSS_it + 1 <= WAVE",)),
    (64, 32, 384, True, ("LDS of a CU",)),           # the runtime kernel's layout at the far corner: 209 KB
    (40, 32, 384, True, ("LDS of a CU",)),           # N = 40 with 384 points: 163 KB
    (64, 16, 192, True, ("LDS of a CU",)),           # ... and at 192 points: 168 KB (the fixed variant serves both: test_inside_the_range_every_pair_is_served)
]


@pytest.mark.parametrize("N,L,S,rt,words", OUTSIDE, ids=["N%d_L%d_S%d_%s" % (o[0], o[1], o[2], "rt" if o[3] else "fixed") for o in OUTSIDE])
def test_outside_the_range_is_refused_with_the_limit_named(built, N, L, S, rt, words):
    g = ec.golden()
    if L:
        cfg, _ = common.lmpc_config(g, 12, max_batch=4, numSS_it=L, numSS_Points=S, trToUse=4)
    else:
        cfg, _ = common.mpc_config(g, 12, max_batch=4)
    cfg.N = N
    _refused(cfg, rt, *words)


INSIDE = [(2, 4, 12), (2, 0, 0), (64, 4, 12), (64, 0, 0), (12, 32, 12), (12, 6, 63), (40, 32, 12), (64, 16, 12), (64, 32, 12)]


@pytest.mark.parametrize("key", INSIDE, ids=["N%d_L%d_ppl%d" % k for k in INSIDE])
def test_inside_the_range_every_pair_is_served(built, key):
    """The other side of every limit is a case of the table and solves P to the oracle in test_every_route_of_every_corner: N = 2 and N = 64, numSS_it = 32,
    numSS_points = 384, 63 points per lap; (40, 384), (64, 192) and (64, 384) on their fixed variants, whose one-wave layout fits a CU while the multi-wave layout and the
    runtime kernel's do not -- they run one wave per QP at every batch size.  Here: the pair creates, on the fixed variant and -- where the runtime kernel's layout
    fits -- on the runtime kernel, without a compiler, and says which kernels it has."""
    from racinglmpc_amd import _capi
    c = next(k for k in ec.CASES if (k.N, k.L, k.ppl) == key)
    for rt in ((False, True) if c.variant else (True,)):
        if rt and (c.N, ec.S_of(c)) in ec.RT_REFUSED:
            continue
        ctx = _capi.Context(ec.config(c, 8), runtime_kernel=rt)
        try:
            lds = ctx.solver_lds()
            assert ctx.solver_kind == (2 if rt else 1) and 0 < lds["lds_1w"] <= ec.LDS_CU, (key, rt, lds)
            if c.mw == "none" or rt:
                n = lds["n_cu"]
                assert lds["lds_mw"] == 0 and [ctx.solver_waves(b) for b in (1, 64, n, n + 1, 100000)] == [1] * 5, (key, rt, lds)
        finally:
            ctx.close()
