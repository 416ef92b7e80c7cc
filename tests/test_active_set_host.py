"""CPU: the NumPy model of the solve kernels (tests/ipm_model.py, default arguments = the kernels' rules) against the certified optima of the hard-problem fixture
tests/golden/lmpc_active.npz -- QPs whose optimum has active lane slacks and inputs at their bounds, at every built horizon (tests/active_cases.py).

Both statements of the QP are checked against each other on every problem, not only the two answers: the ORACLE's explicit reference-form QP (assemble_lmpc_qp)
certifies the MODEL's point with the model's own inequality multipliers in reference row order (common.certificate), so a cost term or a row that the structured
form states differently from the reference shows as a residual even where the two optima happen to lie close.

The N = 40 question of CHANGELOG.md ("active-set fixture"): a probe had the model 1e-2 .. 1.3e-1 from the optimum at N = 40 with every residual of its own at
rounding level.  Those were two different QPs -- the probe's model side took Qfun_sel from a selection at the raw zt, the oracle side from the selection at the
zt that addTerminalComponents wraps when zt[4] - x0[4] > TrackLength / 2 (PredictiveControllers.py:392-393), which a 40-step horizon on a 2.9 m/s lap reaches
and no shorter built horizon does.  test_fixture_covers_the_zt_wrap keeps such problems in the fixture and shows that the Q-values of the other selection move the
optimum by more than 1e-3: the routes are tested on the branch, and a test harness that mixes the two selections cannot pass.
"""
import numpy as np
import pytest

from oracle import lmpc_oracle as orc
from tests import active_cases as ac, common, ipm_model as im


@pytest.fixture(scope="module")
def fx():
    return ac.load()


def _check(par, N, rec, x0, uOld, zs, what, fails, worst):
    """One problem: rec holds A, B, C, SSsel (6, S), Qsel; zs = (x*, u*, slack*, lambda*, sTerm*)."""
    qp = im.StructQP(par, rec["A"], rec["B"], rec["C"], x0, uOld, rec["SSsel"], rec["Qsel"])
    P, q, Aq, l, u = orc.assemble_lmpc_qp(par, rec["A"], rec["B"], rec["C"], x0, uOld, rec["SSsel"], rec["Qsel"])
    mi = 8 * N + rec["Qsel"].shape[0]
    for name, kw in (("one-wave rules", {}), ("multi-wave rules", dict(exact_nu=False))):
        o = im.ipm_solve(qp, **kw)
        e_xu = ac.xu_err(o["x"], o["u"], zs[0], zs[1]); e_s = ac.scaled_err(o["s"].ravel(), zs[2]); e_t = ac.scaled_err(o["sT"], zs[4])
        w = np.concatenate([o["x"].ravel(), o["u"].ravel(), o["s"].ravel(), o["lam"], o["sT"]])
        c = common.certificate(P, q, Aq, l, u, w, o["mu"], mi)
        scale = max(1.0, np.abs(rec["Qsel"]).max())                # (the cost scale, as tests/kkt_batch.py: multipliers and stationarity are in units of Qfun_sel)
        cert = max(c["stationarity"] / scale, c["primal"], c["complementarity"] / scale, c["dual_sign"] / scale)
        k = worst.setdefault(name, [0.0, 0.0, 0.0, 0.0, 0])
        k[:] = [max(k[0], e_xu), max(k[1], e_s), max(k[2], e_t), max(k[3], cert), max(k[4], o["iters"])]
        if not (e_xu <= common.TOL_XU and e_s <= common.TOL_XU and e_t <= common.TOL_XU and cert <= common.TOL_KKT and o["iters"] < 40):
            fails.append("%s, %s: |xu - z*| %.2e, |slack - s*| %.2e, |sTerm - sTerm*| %.2e (scaled), oracle certificate of the model's point %.2e, %d iterations"
                         % (what, name, e_xu, e_s, e_t, cert, o["iters"]))


@pytest.mark.parametrize("N", ac.HORIZONS)
def test_model_reaches_the_certified_optimum_of_every_directed_problem(fx, N):
    par = orc.QPParams.lmpc_default(N)
    inp = ac.fixture_inputs(fx, N)
    K = inp["x0"].shape[0]
    res = ac.oracle_records(fx, N, inp, range(K))
    p = "n%d_" % N
    fails, worst = [], {}
    for r in res:
        b = r["b"]
        zs = tuple(fx[p + k][b] for k in ("x", "u", "slack", "lambd", "sTerm"))
        _check(par, N, r, inp["x0"][b], inp["uOld"][b], zs, "N = %d, problem %d (row %d, %s)" % (N, b, fx[p + "t"][b], ac.FAMILIES[fx[p + "fam"][b]]), fails, worst)
    for name, k in worst.items():
        print("N = %2d, %d problems, %-16s worst scaled |xu - z*| %.2e, slack %.2e, sTerm %.2e; oracle certificate of the model's point %.2e; iterations up to %d" % ((N, K, name) + tuple(k)))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("N", ac.CL_HORIZONS)
def test_model_reaches_the_certified_optimum_of_the_closed_loop_records(fx, N):
    par = orc.QPParams.lmpc_default(N)
    p = "cl%d_" % N
    fails, worst = [], {}
    for b in range(fx[p + "x0"].shape[0]):
        rec = dict(A=fx[p + "A"][b], B=fx[p + "B"][b], C=fx[p + "C"][b], SSsel=fx[p + "SS"][b], Qsel=fx[p + "Qsel"][b])
        zs = tuple(fx[p + k][b] for k in ("x", "u", "slack", "lambd", "sTerm"))
        _check(par, N, rec, fx[p + "x0"][b], fx[p + "uOld"][b], zs, "N = %d, closed-loop record %d" % (N, b), fails, worst)
    for name, k in worst.items():
        print("N = %2d closed loop, %-16s worst scaled |xu - z*| %.2e, slack %.2e, sTerm %.2e; oracle certificate of the model's point %.2e; iterations up to %d" % ((N, name) + tuple(k)))
    assert not fails, "\n".join(fails)


def test_fixture_holds_what_it_promises(fx):
    """Admission rule, coverage minima and counts, from the stored fields (the generator asserts the same when it writes them)."""
    assert [fx["lapx%d" % i].shape[0] for i in range(4)] == [155, 157, 161, 163]
    for N in ac.HORIZONS:
        p = "n%d_" % N
        K = fx[p + "x0"].shape[0]
        assert K >= 0.9 * 7 * len(ac.START_ROWS[N]) and fx[p + "cert"].max() <= 1e-8
        z = [np.concatenate([fx[p + k][b].ravel() for k in ("x", "u", "slack", "lambd", "sTerm")]) for b in range(K)]
        cnt = np.array([ac.active_counts(a, N) for a in z])
        assert np.array_equal(cnt[:, 0], fx[p + "nact_slack"]) and np.array_equal(cnt[:, 1], fx[p + "nact_u"])
        s, b = cnt[:, 0] > 0, cnt[:, 1] > 0
        assert s.sum() >= 8 and b.sum() >= 8 and (s & b).sum() >= 4 and (~s & ~b).sum() >= 2, (N, s.sum(), b.sum())
        assert set(fx[p + "fam"]) == set(range(len(ac.FAMILIES)))
    for N in ac.CL_HORIZONS:
        assert fx["cl%d_x0" % N].shape[0] == 32 and fx["cl%d_cert" % N].max() <= 1e-8


def test_fixture_covers_the_zt_wrap(fx):
    """addTerminalComponents (:392-393) moves zt[4] to max(zt[4] - TrackLength, 0) when zt lies more than half a lap ahead of x0: the safe-set window and its
    Q-values then come from the START of the laps.  Only the longest horizon on a fast lap gets there.  The fixture keeps such problems, and on them the Q-values of
    a selection at the raw zt give another optimum (more than 1e-3 away): the two must not be mixed."""
    g = common.load_lmpc_golden()
    TL = float(g["trackLength"])
    fires = {N: np.nonzero(fx["n%d_zt" % N][:, 4] - fx["n%d_x0" % N][:, 4] > TL / 2)[0] for N in ac.HORIZONS}
    assert all(fires[N].size == 0 for N in ac.HORIZONS if N <= 20) and fires[40].size >= 8, {N: v.size for N, v in fires.items()}
    N = 40
    par = orc.QPParams.lmpc_default(N)
    inp = ac.fixture_inputs(fx, N)
    lap_list = ac.laps(fx)
    xS = [l[0] for l in lap_list]; uS = [l[1] for l in lap_list]
    Qf = [orc.compute_cost(x, TL) for x in xS]
    moved = set()
    for r in ac.oracle_records(fx, N, inp, [b for b in fires[N] if fx["n40_t"][b] in (5, 30)]):
        b = r["b"]
        raw = orc.terminal_components(xS, uS, Qf, [x.shape[0] for x in xS], inp["zt"][b].copy(), 48, 4, None, 4, int(inp["timeStep"][b]), N, TL)
        assert not np.array_equal(raw[0], r["SSsel"]) and not np.array_equal(raw[1], r["Qsel"])
        o = im.ipm_solve(im.StructQP(par, r["A"], r["B"], r["C"], inp["x0"][b], inp["uOld"][b], r["SSsel"], raw[1]))      # the probe's mix-up: this window, those Q-values
        e = ac.xu_err(o["x"], o["u"], fx["n40_x"][b], fx["n40_u"][b])
        print("row %2d %-6s the raw-zt Q-values move the optimum by %.2e (gap %.1e, rd %.1e: a clean solve of another QP)" % (fx["n40_t"][b], ac.FAMILIES[fx["n40_fam"][b]], e, o["gap"], o["rd"]))
        assert e < 1e-7 or e > 1e-3, (b, e)
        if e > 1e-3:
            moved.add((int(fx["n40_t"][b]), ac.FAMILIES[fx["n40_fam"][b]]))
    # the Q-values differ by a constant per lap (40 .. 42 at row 5, 65 .. 69 at row 30): they only matter where lambda* spreads over laps or picks another lap --
    # all seven families at row 30 and epsi- at row 5, the eight problems of the probe
    assert moved == {(30, f) for f in ac.FAMILIES} | {(5, "epsi-")}, moved
