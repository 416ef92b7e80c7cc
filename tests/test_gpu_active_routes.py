"""-m gpu: every solve route on QPs whose optimum has ACTIVE inequality rows, at every built horizon, against the certified optimum.

test_gpu_routes.py runs every route production takes on benign batches (the 0.8 m/s PID lap with small noise: hardly a row active at the optimum).  The four
kernel families differ exactly inside the Newton iteration, and the barrier-weight cap exists because of active lane rows, so here the same routes -- the table is
test_gpu_routes._routes, imported, each route asserted as there -- get the hard-problem fixture tests/golden/lmpc_active.npz (tests/active_cases.py,
tests/golden/make_active_golden.py): directed problems on a 2.9 m/s lap with up to 32 lane slacks above zero and steering at +-0.5 on up to 35 steps, and QPs the
reference flow met in closed loop at N = 12 and N = 14.  The optimum z* = (x, u, slack, lambda, sTerm) of every problem is in the fixture (two oracle methods that
agree to 1e-9, certificates <= 1e-8); nothing is solved on this machine.  The oracle's regression and selection of the fixture's problems are recomputed here
(milliseconds per problem, the call that made the fixture; tests/test_oracle_golden.py pins a stored sample bit for bit).

A launch holds the K fixture problems tiled cyclically: row b is problem b mod K.

Through step_batch, per route: status 0 on every row; A, B, C to TOL_ABC; ssSel, qSel bit-identical to the oracle's selection; scaled |xPred, uPred - z*|,
|slack - s*| and |sTerm - sTerm*| <= TOL_XU; ztNext, ztuNext against Succ lambda* to TOL_ZT where lambda* is unique (the fixture's flag: the oracle's two methods
agree on Succ lambda to 1e-7), against the interval of valid values otherwise (common.zt_face_err); the kkt_batch certificate <= TOL_KKT on every row; every later
copy of a problem bit-identical to its first copy in every output (a kernel that depends on its block position shows).
Through qp_solve_batch (the solve alone, fed the oracle's A, B, C and selection: no regression or selection error can mask or cause a miss; every route but the
LMPC_FUSE ones, which exist for the full step only): the same bounds on x, u, slack, sTerm, the certificate and the copies -- directed problems at every
horizon, closed-loop records at N = 12 and N = 14.
A row with status 0 that lies more than TOL_XU from z* is a silent wrong answer: there is no list of excused problems.
Printed per cell: worst distance, iterations (mean, max), whether the retry pass ran (stats().n_retry; a retry is not a failure, a status bit after it is).
CHANGELOG.md ("active-set fixture") holds the table measured when this test was written.
"""
import numpy as np
import pytest

from tests import active_cases as ac, common
from tests.test_gpu_routes import ALL_KEYS, _knobs, _routes

pytestmark = pytest.mark.gpu

QP_KEYS = ("xPred", "uPred", "slack", "lambd", "sTerm", "mu", "status", "iters")
MAX_LAP_LEN = 256                         # the fixture's laps have 155 .. 163 rows


@pytest.fixture(scope="module")
def fx():
    return ac.load()


def _context(fx, N, B, knobs, runtime_kernel, stores=True):
    from racinglmpc_amd import _capi
    g = common.load_lmpc_golden()
    cfg, par = common.lmpc_config(g, N, max_batch=B, max_lap_len=MAX_LAP_LEN)
    with _knobs(knobs):
        ctx = _capi.Context(cfg, runtime_kernel=runtime_kernel)
    if stores:
        for x, u in ac.laps(fx):
            ctx.model_add_trajectory(x, u); ctx.ss_add_trajectory(x, u)
    return ctx, par


def _tile(a, B):
    a = np.asarray(a)
    return np.ascontiguousarray(a[np.arange(B) % a.shape[0]])


def _copies_differ(out, K, keys):
    """Keys in which some later copy of a problem differs from its first copy (row b against row b mod K)."""
    B = out["status"].shape[0]
    first = np.arange(B) % K
    return [k for k in keys if not np.array_equal(out[k], out[k][first])]


def _solution_errors(out, zs, K):
    """Worst scaled distances of the first copies to z* = (x, u, slack, lambda, sTerm): (xu, slack, sTerm), and the row of the worst xu."""
    exu = np.maximum((np.abs(out["xPred"][:K] - zs[0]) / (1 + np.abs(zs[0]))).reshape(K, -1).max(1), (np.abs(out["uPred"][:K] - zs[1]) / (1 + np.abs(zs[1]))).reshape(K, -1).max(1))
    return float(exu.max()), ac.scaled_err(out["slack"][:K], zs[2]), ac.scaled_err(out["sTerm"][:K], zs[4]), int(exu.argmax())


def _certificate(par, A, Bm, C, x0, uOld, out, ssSel, qSel):
    from tests import kkt_batch
    return kkt_batch.certificate(par, A, Bm, C, x0, uOld, out["xPred"], out["uPred"], out["slack"], out["mu"], ssSel=ssSel, qSel=qSel, lambd=out["lambd"], sTerm=out["sTerm"])["worst"]


def _report(title, rows):
    print("\n%s\n  %-36s batch waves  |xu - z*|  |s - s*|  |sT - sT*|  zt        KKT       iters mean max  retry" % (title, "route"))
    for r in rows:
        print("  %-36s %5d %d      %.2e   %.2e  %.2e    %.2e  %.2e  %5.2f %3d      %s" % r)


@pytest.mark.parametrize("N", ac.HORIZONS)
def test_step_batch_every_route_on_active_problems(built, fx, N):
    inp = ac.fixture_inputs(fx, N)
    K = inp["x0"].shape[0]
    res = ac.oracle_records(fx, N, inp, range(K))                        # (forked workers, before this test makes a HIP context: regression and selection only)
    p = "n%d_" % N
    zs = tuple(fx[p + k] for k in ("x", "u", "slack", "lambd", "sTerm"))
    uniq = fx[p + "lam_unique"]
    fails, rows = [], []
    for name, B, waves, knobs, rt, fused in _routes(N):
        ctx, par = _context(fx, N, B, knobs, rt)
        try:
            assert ctx.solver_waves(B) == waves and ctx.solver_kind == (2 if rt else 0), (name, B, ctx.solver_waves(B), ctx.solver_kind)
            ctx.reset_stats()
            big = {k: _tile(v, B) for k, v in inp.items()}
            out = ctx.step_batch(big["x0"], big["xLin"], big["uLin"], big["uOld"], zt=big["zt"], timeStep=big["timeStep"])
            st = ctx.stats()
            n_regress, n_retry = int(st.n_regress), int(st.n_retry)
        finally:
            ctx.close()
        what = "N = %d, %s, batch %d" % (N, name, B)
        if n_regress != (0 if fused else 1):
            fails.append("%s: %d regression launches" % (what, n_regress))
        if not np.all(out["status"] == 0):
            fails.append("%s: status %s" % (what, np.unique(out["status"], return_counts=True)))
        worst_abc = max(ac.scaled_err(out[k][r["b"]], np.asarray(r[k])) for r in res for k in ("A", "B", "C"))
        if not worst_abc <= common.TOL_ABC:
            fails.append("%s: |A, B, C - oracle| %.2e" % (what, worst_abc))
        sel = [r["b"] for r in res if not (np.array_equal(out["ssSel"][r["b"]], r["SSsel"].T) and np.array_equal(out["qSel"][r["b"]], r["Qsel"]))]
        if sel:
            fails.append("%s: selection differs from the oracle's on problems %s" % (what, sel))
        exu, es, et, at = _solution_errors(out, zs, K)
        if not (exu <= common.TOL_XU and es <= common.TOL_XU and et <= common.TOL_XU):
            fails.append("%s: |xu - z*| %.2e (problem %d: row %d, %s, %d active slacks, %d bound steps), |slack - s*| %.2e, |sTerm - sTerm*| %.2e" % (
                what, exu, at, fx[p + "t"][at], ac.FAMILIES[fx[p + "fam"][at]], fx[p + "nact_slack"][at], fx[p + "nact_u"][at], es, et))
        ezt = 0.0
        for r in res:
            b = r["b"]
            if uniq[b]:
                e = common.zt_err(out["ztNext"][b], out["ztuNext"][b], r["Succ"], r["SuccU"], zs[3][b])
            else:
                e = common.zt_face_err(out["ztNext"][b], out["ztuNext"][b], r["Succ"], r["SuccU"], r["SSsel"], r["Qsel"], zs[3][b])[0]
            ezt = max(ezt, e)
        if not ezt <= common.TOL_ZT:
            fails.append("%s: |zt - Succ lambda*| %.2e" % (what, ezt))
        kkt = float(_certificate(par, out["A"], out["B"], out["C"], big["x0"], big["uOld"], out, out["ssSel"], out["qSel"]).max())
        if not kkt <= common.TOL_KKT:
            fails.append("%s: KKT certificate %.2e" % (what, kkt))
        diff = _copies_differ(out, K, ALL_KEYS)
        if diff:
            fails.append("%s: %s of a later copy differ from the first copy of the problem" % (what, ", ".join(diff)))
        rows.append((name, B, waves, exu, es, et, ezt, kkt, out["iters"][:K].mean(), out["iters"][:K].max(), "yes" if n_retry else "no"))
    _report("step_batch, N = %d, %d directed problems (%d with an active lane slack, %d with an input at a bound)" % (N, K, (fx[p + "nact_slack"] > 0).sum(), (fx[p + "nact_u"] > 0).sum()), rows)
    assert not fails, "\n".join(fails)


def _qp_routes(N):
    return [r for r in _routes(N) if "LMPC_FUSE" not in r[3]]


def _qp_case(fx, N, A, Bm, C, x0, uOld, SS, Qsel, zs, title):
    """qp_solve_batch on every route; SS (K, 6, S) in the reference's layout."""
    K = x0.shape[0]
    ssSel = np.ascontiguousarray(np.transpose(SS, (0, 2, 1)))
    fails, rows = [], []
    for name, B, waves, knobs, rt, _ in _qp_routes(N):
        ctx, par = _context(fx, N, B, knobs, rt, stores=False)
        try:
            assert ctx.solver_waves(B) == waves and ctx.solver_kind == (2 if rt else 0), (name, B, ctx.solver_waves(B), ctx.solver_kind)
            ctx.reset_stats()
            big = [_tile(a, B) for a in (A, Bm, C, x0, uOld, ssSel, Qsel)]
            out = ctx.qp_solve_batch(*big)
            n_retry = int(ctx.stats().n_retry)
        finally:
            ctx.close()
        what = "%s, %s, batch %d" % (title, name, B)
        if not np.all(out["status"] == 0):
            fails.append("%s: status %s" % (what, np.unique(out["status"], return_counts=True)))
        exu, es, et, at = _solution_errors(out, zs, K)
        if not (exu <= common.TOL_XU and es <= common.TOL_XU and et <= common.TOL_XU):
            fails.append("%s: |xu - z*| %.2e (problem %d), |slack - s*| %.2e, |sTerm - sTerm*| %.2e" % (what, exu, at, es, et))
        kkt = float(_certificate(par, big[0], big[1], big[2], big[3], big[4], out, big[5], big[6]).max())
        if not kkt <= common.TOL_KKT:
            fails.append("%s: KKT certificate %.2e" % (what, kkt))
        diff = _copies_differ(out, K, QP_KEYS)
        if diff:
            fails.append("%s: %s of a later copy differ from the first copy of the problem" % (what, ", ".join(diff)))
        rows.append((name, B, waves, exu, es, et, np.nan, kkt, out["iters"][:K].mean(), out["iters"][:K].max(), "yes" if n_retry else "no"))      # (no zt: the solve alone)
    _report("qp_solve_batch, " + title, rows)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("N", ac.HORIZONS)
def test_qp_solve_batch_every_route_on_active_problems(built, fx, N):
    inp = ac.fixture_inputs(fx, N)
    K = inp["x0"].shape[0]
    res = ac.oracle_records(fx, N, inp, range(K))
    p = "n%d_" % N
    _qp_case(fx, N, np.stack([r["A"] for r in res]), np.stack([r["B"] for r in res]), np.stack([r["C"] for r in res]), inp["x0"], inp["uOld"],
             np.stack([r["SSsel"] for r in res]), np.stack([r["Qsel"] for r in res]), tuple(fx[p + k] for k in ("x", "u", "slack", "lambd", "sTerm")),
             "N = %d, %d directed problems" % (N, K))


@pytest.mark.parametrize("N", ac.CL_HORIZONS)
def test_qp_solve_batch_every_route_on_closed_loop_records(built, fx, N):
    p = "cl%d_" % N
    _qp_case(fx, N, fx[p + "A"], fx[p + "B"], fx[p + "C"], fx[p + "x0"], fx[p + "uOld"], fx[p + "SS"], fx[p + "Qsel"],
             tuple(fx[p + k] for k in ("x", "u", "slack", "lambd", "sTerm")), "N = %d, %d closed-loop records (up to %d active lane slacks)" % (N, fx[p + "x0"].shape[0], fx[p + "nact_slack"].max()))
