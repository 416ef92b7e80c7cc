"""-m gpu: one problem set, every solve route, one answer.

The library does not have one solve path: it picks a kernel per launch from the horizon, the batch size, the create flags and the environment knobs
(lmpc_capi.hip: pick_solver, create_body, launch_solve, lmpc_step_batch_dev).  Here the same 64 problems P (bench.synth_batch, four PID laps as regression
store and safe set, as bench.make_ctx / common.make_lmpc_ctx set them up) sit in rows 0..63 of batches whose size puts them on each route production takes
for that horizon.  The rows after 64 hold OTHER problems (another seed), so that a kernel that finds its problem by a block offset instead of its index shows.
Per horizon:
  * the route is asserted (Context.solver_waves, solver_kind, and a fused step launches no regression kernel): a moved threshold fails here instead of
    leaving a cell that silently stops being tested;
  * A, B, C, the selection (ssSel, qSel) and the status word are bit-identical on every route -- one regression kernel, one k2_select;
  * the fused step is bit-identical in EVERY output to the unfused step on the same one-wave kernel, the runtime kernel with LMPC_FUSE=1 to the runtime
    kernel without it, [A|B] in LDS (LMPC_NO_ABG) to [A|B] in global memory, the zero-copy single-problem path of a max_batch = 1 context (the drop-in
    classes) to the four-wave batch row;
  * the selection's other outputs (selStart, succ, succU, ztUsed: select_batch on a context of the route, on P) are bit-identical to the four-wave route's too;
  * the epilogue holds on the route's own outputs: ztNext = Succ lambda, ztuNext = SuccU lambda and sTerm = SS lambda - x_N to the rounding of a sum of that
    many terms in any order, (n - 1) u sum |terms| with u = 2^-53 and a factor 2 to spare (_epilogue_fails); plain MPC: ztNext = x_N, ztuNext = u_{N-1} bit for bit;
  * xPred, uPred agree with the four-wave route to 2e-7 and ztNext to 2e-7 (1 + |zt|): the 1e-7 a-posteriori termination rule;
  * every route meets the oracle on P: A, B, C to TOL_ABC, selections identical, (x, u) at the certified optimum to TOL_XU (common.compare_with_oracle;
    plain MPC: the certified optimum of the reference-form MPC QP).

Cells covered (batch sizes; "-": production never runs that kernel for the horizon; the knobs are set around Context() only):

   N   S | 4 waves | 2 waves | 1 wave, [A|B] in LDS     | 1 wave, [A|B] global | LMPC_FUSE=1 | runtime kernel | runtime + LMPC_FUSE=1 | max_batch = 1
   8  48 |   64    |   300   | 1100                     |  -                   | 1100        | 1100           | 1100                  |  -
  12  48 |   64    |   300   | 1100                     |  -                   | 1100        | 1100           | 1100                  | 8 of P
  14  48 |   64    |   300   | 600                      |  -                   | 600         | 600            | 600                   |  -
  20  48 |   64    |   300   | 600                      |  -                   | 600         | 600            | 600                   |  -
  40  48 |   64    |   -     | 300; 1100 + LMPC_NO_ABG  | 1100                 | 1100        | 1100           | 1100                  |  -
  12   0 |   64    |   300   | 1100                     |  -                   | 1100        | 1100           | 1100                  | 8 of P
"""
import contextlib
import os

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

P_SIZE = 64
SEED_P, SEED_FILL = 1234, 4321
ALL_KEYS = ("A", "B", "C", "xPred", "uPred", "slack", "lambd", "sTerm", "ztNext", "ztuNext", "ssSel", "qSel", "mu", "status", "iters")
SAME_KEYS = ("A", "B", "C", "ssSel", "qSel", "status")
SAME_SELECT_KEYS = ("selStart", "succ", "succU", "ztUsed")
TOL_ROUTE = 2e-7

CASES = [(8, 48), (12, 48), (14, 48), (20, 48), (40, 48), (12, 0)]


@contextlib.contextmanager
def _knobs(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _routes(N):
    """(name, batch, waves per QP, knobs, runtime kernel, fused) of every route production takes at horizon N."""
    one = 600 if 12 < N <= 24 else 1100
    r = [("4 waves", P_SIZE, 4, {}, False, False)]
    if N <= 24:
        r.append(("2 waves", 300, 2, {}, False, False))
    if N == 40:
        r += [("1 wave, [A|B] in LDS", 300, 1, {}, False, False), ("1 wave, [A|B] global", one, 1, {}, False, False),
              ("1 wave, [A|B] in LDS (LMPC_NO_ABG)", one, 1, {"LMPC_NO_ABG": "1"}, False, False)]
    else:
        r.append(("1 wave", one, 1, {}, False, False))
    r += [("LMPC_FUSE=1", one, 1, {"LMPC_FUSE": "1"}, False, True), ("runtime kernel", one, 1, {}, True, False),
          ("runtime kernel + LMPC_FUSE=1", one, 1, {"LMPC_FUSE": "1"}, True, False)]
    return r


# routes that must give the same bits in every output at the same batch: the fused step and the unfused step on the same one-wave kernel (N = 40: the
# fused step keeps [A|B] in LDS), the runtime kernel with and without LMPC_FUSE=1, [A|B] in LDS and in global memory
BIT_PAIRS = {"LMPC_FUSE=1": ("1 wave", "1 wave, [A|B] in LDS (LMPC_NO_ABG)"), "runtime kernel + LMPC_FUSE=1": ("runtime kernel",),
             "1 wave, [A|B] in LDS (LMPC_NO_ABG)": ("1 wave, [A|B] global",)}


def _batch(P, F, B):
    """P in rows 0..63, rows 64.. from the other problem set F."""
    return {k: np.concatenate([P[k], F[k][P_SIZE:B]]) for k in ("x0", "xLin", "uLin", "uOld", "zt", "timeStep")}


def _mpc_oracle(g, par, N, P, rows=range(P_SIZE)):
    """Plain LTV-MPC (no terminal set, regression on the one stored PID lap): A, B, C and the certified optimum of the reference-form QP per problem."""
    from oracle import lmpc_oracle as orc
    pt = np.array(g["track"]); xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    res = []
    for b in rows:
        A, B, C = orc.compute_ltv_dynamics([xP], [uP], [0], pt, P["xLin"][b], P["uLin"][b], N)
        Pq, q, Ao, lo, up = orc.assemble_mpc_qp(par, A, B, C, P["x0"][b], P["uOld"][b])
        ex, cert = orc.osqp_solve_exact(Pq, q, Ao, lo, up, want=1e-8)
        res.append(dict(b=b, A=np.array(A), B=np.array(B), C=np.array(C), opt=ex.x, cert=cert))
    return res


def _mpc_compare(out, res, N, what):
    nxu = 6 * (N + 1) + 2 * N
    worst_abc = worst_xu = 0.0
    for r in res:
        b = r["b"]
        assert r["cert"] < 1e-8, (what, b, r["cert"])
        for got, ref in ((out["A"][b], r["A"]), (out["B"][b], r["B"]), (out["C"][b], r["C"])):
            worst_abc = max(worst_abc, float((np.abs(got - ref) / (1 + np.abs(ref))).max()))
        w = np.concatenate([out["xPred"][b].ravel(), out["uPred"][b].ravel()])
        worst_xu = max(worst_xu, float((np.abs(w - r["opt"][:nxu]) / (1 + np.abs(r["opt"][:nxu]))).max()))
    print("%s: %d problems: worst relative |A,B,C - oracle| %.2e; |xu - z*| / (1 + |z*|) %.2e" % (what, len(res), worst_abc, worst_xu))
    assert worst_abc < common.TOL_ABC and worst_xu < common.TOL_XU, what
    return dict(abc=worst_abc, xu=worst_xu, zt=0.0)


def _context(g, N, S, B, knobs, runtime_kernel):
    from racinglmpc_amd import _capi
    pid = (np.array(g["xPID"]), np.array(g["uPID"]))
    cfg, _ = common.lmpc_config(g, N, max_batch=B) if S else common.mpc_config(g, N, max_batch=B)
    with _knobs(knobs):
        ctx = _capi.Context(cfg, runtime_kernel=runtime_kernel)
    for _ in range(4 if S else 1):
        ctx.model_add_trajectory(*pid)
        if S:
            ctx.ss_add_trajectory(*pid)
    return ctx


def _step(ctx, inp):
    return ctx.step_batch(inp["x0"], inp["xLin"], inp["uLin"], inp["uOld"], zt=inp["zt"] if ctx.S else None, timeStep=inp["timeStep"] if ctx.S else None)


def _epilogue_fails(out, sel, N, S):
    """The epilogue's identities on one route's own outputs, rows of P.  S > 0: with t_c = succ[c, j] lambda_c, |ztNext[j] - sum_c t_c| <= S 2^-52 sum_c |t_c| (ztuNext
    against succU likewise), and with t_c = ssSel[c, j] lambda_c, |sTerm[j] - (sum_c t_c - xPred[N, j])| <= (S + 1) 2^-52 (sum_c |t_c| + |xPred[N, j]|): the bound of an
    n-term floating-point sum in any order, (n - 1) u sum |terms|, u = 2^-53, with a factor 2 to spare.  The sums are formed in extended precision, so that the
    test's own rounding does not count.  S = 0: ztNext is x_N and ztuNext is u_{N-1}, bit for bit."""
    R = slice(0, P_SIZE)
    if not S:
        return [k for k, want in (("ztNext", out["xPred"][R, N]), ("ztuNext", out["uPred"][R, N - 1])) if not np.array_equal(out[k][R], want)]
    ld = np.longdouble
    lam = out["lambd"][R].astype(ld)[:, :, None]
    bad = []
    for k, rows in (("ztNext", sel["succ"][R]), ("ztuNext", sel["succU"][R])):
        t = rows.astype(ld) * lam
        err, bound = np.abs(out[k][R].astype(ld) - t.sum(axis=1)), S * ld(2.0) ** -52 * np.abs(t).sum(axis=1)
        print("    %-8s worst |error| / bound %.3f" % (k, float((err / bound).max())))
        if not np.all(err <= bound):
            bad.append(k)
    t = out["ssSel"][R].astype(ld) * lam
    xN = out["xPred"][R, N].astype(ld)
    err, bound = np.abs(out["sTerm"][R].astype(ld) - (t.sum(axis=1) - xN)), (S + 1) * ld(2.0) ** -52 * (np.abs(t).sum(axis=1) + np.abs(xN))
    print("    %-8s worst |error| / bound %.3f" % ("sTerm", float((err / bound).max())))
    if not np.all(err <= bound):
        bad.append("sTerm")
    return bad


@pytest.mark.parametrize("N,S", CASES, ids=["N%d_S%d" % c for c in CASES])
def test_every_route_gives_one_answer(built, N, S):
    import bench
    from oracle import lmpc_oracle as orc
    from tests import oracle_pool
    g = common.load_lmpc_golden()
    routes = _routes(N)
    P = bench.synth_batch(g, P_SIZE, N, seed=SEED_P)
    F = bench.synth_batch(g, max(r[1] for r in routes), N, seed=SEED_FILL)
    # the oracle first (forked workers, before this test makes a HIP context); K3 against the certified optimum on every problem of P
    if S:
        par = orc.QPParams.lmpc_default(N)
        pid = (np.array(g["xPID"]), np.array(g["uPID"]))
        res = oracle_pool.oracle_batch(par, np.array(g["track"]), float(g["trackLength"]), [pid] * 4, N, P, range(P_SIZE), solve_idx=range(P_SIZE))
    else:
        res = _mpc_oracle(g, orc.QPParams.mpc_default(N, 0.8), N, P)

    outs, sels, fails, rows = {}, {}, [], []
    for name, B, waves, knobs, rt, fused in routes:
        ctx = _context(g, N, S, B, knobs, rt)
        try:
            assert ctx.solver_waves(B) == waves and ctx.solver_kind == (2 if rt else 0), (name, B, ctx.solver_waves(B), ctx.solver_kind)
            ctx.reset_stats()
            out = _step(ctx, _batch(P, F, B))
            n_regress = int(ctx.stats().n_regress)
            sel = ctx.select_batch(P["x0"], P["zt"], timeStep=P["timeStep"]) if S else None
        finally:
            ctx.close()
        outs[name] = out; sels[name] = sel
        what = "N = %d, S = %d, %s, batch %d" % (N, S, name, B)
        print(what)
        if n_regress != (0 if fused else 1):                       # the fused step runs the regression inside the solve kernel; nothing else does
            fails.append("%s: %d regression launches" % (what, n_regress))
        if not np.all(out["status"][:P_SIZE] == 0):
            fails.append("%s: status %s" % (what, np.unique(out["status"][:P_SIZE], return_counts=True)))
        ref = outs["4 waves"]
        same = [k for k in SAME_KEYS if not np.array_equal(out[k][:P_SIZE], ref[k][:P_SIZE])]
        if same:
            fails.append("%s: %s not bit-identical to the four-wave route" % (what, ", ".join(same)))
        if S:
            same = [k for k in SAME_SELECT_KEYS if not np.array_equal(sel[k], sels["4 waves"][k])]
            if same:
                fails.append("%s: select_batch on P: %s not bit-identical to the four-wave route" % (what, ", ".join(same)))
        bad = _epilogue_fails(out, sel, N, S)
        if bad:
            fails.append("%s: epilogue: %s beyond the rounding of its sum" % (what, ", ".join(bad)) if S else "%s: epilogue: %s not the last predicted row bit for bit" % (what, ", ".join(bad)))
        dxu = max(float(np.abs(out["xPred"][:P_SIZE] - ref["xPred"][:P_SIZE]).max()), float(np.abs(out["uPred"][:P_SIZE] - ref["uPred"][:P_SIZE]).max()))
        dzt = float((np.abs(out["ztNext"][:P_SIZE] - ref["ztNext"][:P_SIZE]) / (1 + np.abs(ref["ztNext"][:P_SIZE]))).max())
        if not (dxu < TOL_ROUTE and dzt < TOL_ROUTE):
            fails.append("%s: |xu| differs from the four-wave route by %.2e, zt by %.2e" % (what, dxu, dzt))
        for other in BIT_PAIRS.get(name, ()):
            if other in outs:
                diff = [k for k in ALL_KEYS if not np.array_equal(out[k], outs[other][k])]
                if diff:
                    fails.append("%s: %s not bit-identical to %s at the same batch" % (what, ", ".join(diff), other))
        try:
            worst = (common.compare_with_oracle if S else _mpc_compare)(out, res, N, what)
        except AssertionError as e:
            fails.append("%s: oracle: %s" % (what, e))
            worst = dict(abc=np.nan, xu=np.nan, zt=np.nan)
        rows.append((name, B, waves, n_regress, dxu, dzt, worst["abc"], worst["xu"]))

    if N == 12:
        # the drop-in classes' path: a max_batch = 1 context, one problem per call, inputs and outputs in host-mapped memory
        ctx = _context(g, N, S, 1, {}, False)
        try:
            assert ctx.solver_waves(1) == 4 and ctx.solver_kind == 0
            for b in range(0, P_SIZE, 8):
                one = _step(ctx, {k: v[b:b + 1] for k, v in P.items()})
                diff = [k for k in ALL_KEYS if not np.array_equal(one[k][0], outs["4 waves"][k][b])]
                if diff:
                    fails.append("N = %d, S = %d, max_batch = 1, problem %d: %s not bit-identical to the four-wave batch row" % (N, S, b, ", ".join(diff)))
        finally:
            ctx.close()
        rows.append(("max_batch = 1 (8 of P)", 1, 4, 1, 0.0, 0.0, np.nan, np.nan))

    print("\nN = %d, S = %d: route, batch, waves, regression launches, |xu - 4 waves|, |zt - 4 waves| / (1 + |zt|), worst |A,B,C - oracle| rel, worst |xu - z*| rel" % (N, S))
    for r in rows:
        print("  %-36s %5d %d %d  %.2e  %.2e  %.2e  %.2e" % r)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("N,S", [(12, 48), (12, 0)], ids=["N12_S48", "N12_S0"])
def test_step_batch_copy_routes_give_one_answer(built, N, S):
    """lmpc_step_batch moves its arrays in one of two ways, and nothing else tests either beyond one problem: (a) a full batch of a small context runs on the
    host-mapped mirrors of the work buffers -- here max_batch = 4, B = 4; (b) any other call copies array by array -- the same context with B = 3, which owns
    mirrors and must not use them, and (c) a max_batch = 64 context, which owns none, with B = 4.  Problems: rows 0..3 of P, every timeStep non-zero, rows 1 and 3
    with previous predictions whose last rows lie beyond the finish line, so that the selection shifts the Q-function (rows 0 and 2: hasPred = 0).  All three run four
    waves per QP; every output is bit-identical between them on the rows they share, a second full batch on (a) after the B = 3 call reproduces the first (nothing
    stale in the mirrors), and every route meets the oracle.  Plain MPC (S = 0) gets the same inputs and must not read the selection's."""
    import bench
    from oracle import lmpc_oracle as orc
    from tests import oracle_pool
    g = common.load_lmpc_golden()
    TL = float(g["trackLength"])
    P = {k: v[:4].copy() for k, v in bench.synth_batch(g, P_SIZE, N, seed=SEED_P).items()}
    P["timeStep"] = (P["timeStep"] + 3).astype(np.int32)
    P["hasPred"] = np.array([0, 1, 0, 1], np.int32)
    P["xPredPrev"] = np.concatenate([P["xLin"][:, 1:], P["zt"][:, None]], axis=1)               # a plausible previous prediction: the linearisation shifted by one ...
    P["xPredPrev"][:, -3:, 4] = TL + 0.05 * np.arange(1, 4)                                       # ... whose last three rows have crossed the line
    assert np.all(P["timeStep"] > 0) and np.all(P["xPredPrev"][[1, 3], -1, 4] > TL)
    if S:
        pid = (np.array(g["xPID"]), np.array(g["uPID"]))
        res = oracle_pool.oracle_batch(orc.QPParams.lmpc_default(N), np.array(g["track"]), TL, [pid] * 4, N, P, range(4), solve_idx=range(4))
        # (the shift is really active: the selected Q-values of rows 1 and 3 differ from the ones a first step would get)
        plain = oracle_pool.oracle_batch(orc.QPParams.lmpc_default(N), np.array(g["track"]), TL, [pid] * 4, N, dict(P, hasPred=np.zeros(4, np.int32)), [1, 3])
        assert all(not np.array_equal(res[r["b"]]["Qsel"], r["Qsel"]) for r in plain)
    else:
        res = _mpc_oracle(g, orc.QPParams.mpc_default(N, 0.8), N, P, rows=range(4))

    def step(ctx, B):
        assert ctx.solver_waves(B) == 4 and ctx.solver_kind == 0
        return ctx.step_batch(P["x0"][:B], P["xLin"][:B], P["uLin"][:B], P["uOld"][:B], zt=P["zt"][:B], xPredPrev=P["xPredPrev"][:B], hasPred=P["hasPred"][:B], timeStep=P["timeStep"][:B])
    small = _context(g, N, S, 4, {}, False)
    try:
        outs = {"(a) max_batch 4, B 4": step(small, 4), "(b) max_batch 4, B 3": step(small, 3), "(a) again": step(small, 4)}
    finally:
        small.close()
    large = _context(g, N, S, P_SIZE, {}, False)
    try:
        outs["(c) max_batch 64, B 4"] = step(large, 4)
    finally:
        large.close()
    ref = outs["(a) max_batch 4, B 4"]
    fails = []
    for name, out in outs.items():
        B = out["status"].shape[0]
        what = "N = %d, S = %d, %s" % (N, S, name)
        if not np.all(out["status"] == 0):
            fails.append("%s: status %s" % (what, out["status"]))
        diff = [k for k in ALL_KEYS + ("resid",) if not np.array_equal(out[k], ref[k][:B])]
        if diff:
            fails.append("%s: %s not bit-identical to the full batch on the mirrors" % (what, ", ".join(diff)))
        try:
            (common.compare_with_oracle if S else _mpc_compare)(out, [r for r in res if r["b"] < B], N, what)
        except AssertionError as e:
            fails.append("%s: oracle: %s" % (what, e))
    assert not fails, "\n".join(fails)
