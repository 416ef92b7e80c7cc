"""CPU: the oracle restatement reproduces what the reference's own classes produced (golden fixtures made by
tests/golden/make_golden.py), and the restated OSQP returns certified optima."""
import numpy as np
import pytest

from oracle import lmpc_oracle as orc
from tests import common


def test_track_table_matches_reference():
    g = common.load_lmpc_golden()
    pt, TL = orc.make_track()
    assert np.array_equal(pt, g["track"]) and TL == float(g["trackLength"])
    for s, k in ((0.0, 0), (0.5, 0), (1.0, 1), (5.6, 2), (7.9, 3), (12.3, 4), (15.2, 5), (18.0, 6), (19.3, 0), (40.0, 1)):
        assert orc.curvature(pt, s) == pt[k, 5]


def test_pid_lap_restatement_is_bit_exact():
    """oracle plant + PID == reference Simulator.sim + PID (np.random.seed(0)), 1000 steps."""
    g = common.load_lmpc_golden()
    pt, _ = orc.make_track()
    x, u, xg = orc.pid_lap(pt, 0.8, 0, maxSimTime=15)          # first 150 steps are enough (same RNG stream)
    assert np.array_equal(x, g["xPID"][:150]) and np.array_equal(u, g["uPID"][:150]) and np.array_equal(xg, g["xPID_glob"][:150])


def test_regression_restatement_matches_reference():
    g = common.load_lmpc_golden()
    pt = g["track"]
    for r in (0, 1, 7, 30, 31, 45, 59):
        lap = int(g["rec_lap"][r])
        xs = [g["xStored%d" % i] for i in range(6)]; us = [g["uStored%d" % i] for i in range(6)]
        if lap == 4:
            xS, uS = xs[2:6], us[2:6]
        else:
            xS, uS = xs[1:6], us[1:6]
        A, B, C = orc.compute_ltv_dynamics(xS, uS, [0, 1, 2, 3], pt, g["rec_xLin"][r], g["rec_uLin"][r], 12)
        for got, ref in ((A, g["rec_A"][r]), (B, g["rec_B"][r]), (C, g["rec_C"][r])):
            assert (np.abs(got - ref) / (1 + np.abs(ref))).max() < 1e-10


def test_selection_and_assembly_restatement_bit_exact():
    g = common.load_lmpc_golden()
    par = orc.QPParams.lmpc_default(12)
    TL = float(g["trackLength"])
    for r in (0, 2, 9, 29, 30, 33, 44, 59):
        lap = int(g["rec_lap"][r]); nl = lap
        SS = [g["SS%d" % i][:g["rec_ssLen"][r][i]] for i in range(nl)]
        uSS = [g["uSS%d" % i][:g["rec_ssLen"][r][i]] for i in range(nl)]
        Qf = [g["Qfun%d" % i][:g["rec_ssLen"][r][i]] for i in range(nl)]
        zt = g["rec_zt"][r].copy()
        if zt[4] - g["rec_x0"][r][4] > TL / 2:
            zt[4] = np.max([zt[4] - TL, 0])
        xpp = g["rec_xPredPrev"][r] if g["rec_hasPred"][r] else None
        SSsel, Qsel, Succ, SuccU = orc.terminal_components(SS, uSS, Qf, list(g["rec_LapTime"][r][:nl]), zt, 48, 4, xpp, lap,
                                                           int(g["rec_t"][r]), 12, TL)
        assert np.array_equal(SSsel, g["rec_SSsel"][r]) and np.array_equal(Qsel, g["rec_Qsel"][r])
        assert np.array_equal(Succ, g["rec_Succ"][r]) and np.array_equal(SuccU, g["rec_SuccU"][r])
        P, q, A, l, u = orc.assemble_lmpc_qp(par, g["rec_A"][r], g["rec_B"][r], g["rec_C"][r], g["rec_x0"][r], g["rec_OldInput"][r], SSsel, Qsel)
        Pr, qr, Ar, lr, ur = common.dense_from_csc(g, r)
        assert np.array_equal(P, Pr) and np.array_equal(q, qr) and np.array_equal(A, Ar) and np.array_equal(l, lr) and np.array_equal(u, ur)


def test_compute_cost_restatement():
    g = common.load_lmpc_golden()
    TL = float(g["trackLength"])
    assert np.array_equal(orc.compute_cost(g["SS0"], TL)[:1000], g["Qfun0"])
    assert np.array_equal(orc.compute_cost(g["lapx1"], TL), g["Qfun5"])


def test_restated_osqp_certificates():
    """Default-settings run is within OSQP's own tolerance of the certified optimum; the exact mode is certified."""
    g = common.load_lmpc_golden()
    for r in (0, 6, 12, 36):
        P, q, A, l, u = common.dense_from_csc(g, r)
        res = orc.osqp_solve(P, q, A, l, u, polish=True)
        assert res.status == 1
        assert np.allclose(res.x, g["rec_sol"][r], atol=1e-12)            # deterministic
        ex, cert = orc.osqp_solve_exact(P, q, A, l, u)
        assert cert < 1e-8
        assert np.abs(ex.x[:102] - g["rec_sol_opt"][r][:102]).max() < 1e-8
        assert np.abs(res.x[78:102] - ex.x[78:102]).max() < 5e-2            # eps = 1e-3 ADMM iterate vs optimum


def test_ipm_model_matches_certified_optimum():
    """The NumPy model of the HIP solve kernel (tests/ipm_model.py) reaches the certified optimum."""
    from tests import ipm_model as im
    g = common.load_lmpc_golden()
    par = orc.QPParams.lmpc_default(12)
    for r in (0, 5, 13, 29, 41, 50):
        qp = im.StructQP(par, g["rec_A"][r], g["rec_B"][r], g["rec_C"][r], g["rec_x0"][r], g["rec_OldInput"][r], g["rec_SSsel"][r], g["rec_Qsel"][r])
        o = im.ipm_solve(qp, reg_l=1e-6)
        assert o["iters"] < 25
        w = np.concatenate([o["x"].ravel(), o["u"].ravel()])
        assert np.abs(w - g["rec_sol_opt"][r][:102]).max() < 1e-6


def test_global_position_oracle_matches_reference_fixture():
    """oracle.get_global_position vs Map.getGlobalPosition outputs recorded from the executed reference (tests/golden/track_xy.npz)."""
    import os
    t = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_xy.npz"))
    pt = t["track"]
    got = np.array([orc.get_global_position(pt, float(s), float(e)) for s, e in zip(t["s"], t["ey"])])
    assert np.abs(got - t["xy"]).max() < 1e-12
    with pytest.raises(ValueError):
        orc.get_global_position(pt, float(2 * t["trackLength"]), 0.0)      # wraps to TrackLength exactly: on no segment


def _regression_cases():
    import os
    g = common.load_lmpc_golden()
    r = np.load(os.path.join(common.GOLDEN, "regression.npz"))
    data = dict(pid=(g["xPID"], g["uPID"]), lap0=(g["lapx0"], g["lapu0"]), lap1=(g["lapx1"], g["lapu1"]), short=(g["xPID"][:40], g["uPID"][:40]))
    return [(str(c), data[str(c)][0], data[str(c)][1], float(r[str(c) + "_lamb"]), r[str(c) + "_A"], r[str(c) + "_B"], r[str(c) + "_Error"], float(r[str(c) + "_cond"]))
            for c in r["cases"]]


def test_lti_regression_restatement_matches_reference():
    """oracle.lti_regression vs the reference's Utilities.Regression output (fixture from the executed reference function)."""
    from oracle import lmpc_oracle as orc
    for name, x, u, lamb, A, B, E, cond in _regression_cases():
        A2, B2, E2 = orc.lti_regression(x, u, lamb)
        assert np.array_equal(A2, A) and np.array_equal(B2, B) and np.array_equal(E2, E), name


def test_oracle_noslack_assembly_matches_reference():
    """MPCParams(slacks=False): the restated buildIneqConstr / buildCost / buildEqConstr branches (PredictiveControllers.py:184-198, 218-221,
    248-254) reproduce the matrices the executed reference built (tests/golden/make_noslack_golden.py), bit for bit; the recorded optimum is certified."""
    import os
    g = np.load(os.path.join(common.GOLDEN, "ltvmpc_noslack_n12.npz"))
    par = orc.QPParams.mpc_default(12, 0.8); par.slacks = False; par.bx = np.array([float(g["bx"])] * 2)
    for r in range(len(g["x0"])):
        P, q, A, l, u = common.dense_from_csc(g, r, prefix="")
        P2, q2, A2, l2, u2 = orc.assemble_mpc_qp(par, g["A"][r], g["B"][r], g["C"][r], g["x0"][r], g["OldInput"][r])
        assert np.array_equal(P, P2) and np.array_equal(q, q2) and np.array_equal(A, A2) and np.array_equal(l, l2) and np.array_equal(u, u2)
        assert P.shape == (102, 102) and A.shape == (72 + 78, 102)
        assert max(orc.kkt_certificate(P, q, A, l, u, g["sol_opt"][r], g["y_opt"][r]).values()) < 1e-9


@pytest.mark.parametrize("name", ["lmpc_wide_n12", "lmpc_n14", "lmpc_n40"])
def test_other_configurations_restatement_matches_reference(name):
    """Fixtures recorded from the executed reference (tests/golden/make_wide_golden.py): numSS_it = 6, numSS_Points = 72 (more terminal columns
    than lanes of a wavefront) and main.py's own horizon N = 14: regression, selection with successors and Q-function shift, assembled QP."""
    g = common.load_variant_golden(name)
    N = int(g["N"])
    par = orc.QPParams.lmpc_default(N)
    par.numSS_Points, par.numSS_it = int(g["numSS_Points"]), int(g["numSS_it"])
    TL = float(g["trackLength"]); L = int(g["nSS"])
    SS, uSS, Qf = g["SS"], g["uSS"], g["Qf"]
    for r in range(g["x0"].shape[0]):
        A, B, C = orc.compute_ltv_dynamics([g["xPID"]] * 4, [g["uPID"]] * 4, [0, 1, 2, 3], g["track"], g["xLin"][r], g["uLin"][r], N)
        for got, ref in ((A, g["A"][r]), (B, g["B"][r]), (C, g["C"][r])):
            assert (np.abs(got - ref) / (1 + np.abs(ref))).max() < 1e-10
        zt = g["zt"][r].copy()
        if zt[4] - g["x0"][r][4] > TL / 2:
            zt[4] = np.max([zt[4] - TL, 0])
        xpp = g["xPredPrev"][r] if g["hasPred"][r] else None
        SSsel, Qsel, Succ, SuccU = orc.terminal_components(SS, uSS, Qf, [s_.shape[0] for s_ in SS], zt, par.numSS_Points, par.numSS_it, xpp, L,
                                                           int(g["t"][r]), N, TL)
        assert np.array_equal(SSsel, g["SSsel"][r]) and np.array_equal(Qsel, g["Qsel"][r])
        assert np.array_equal(Succ, g["Succ"][r]) and np.array_equal(SuccU, g["SuccU"][r])
        P, q, Aq, l, u = orc.assemble_lmpc_qp(par, g["A"][r], g["B"][r], g["C"][r], g["x0"][r], g["OldInput"][r], SSsel, Qsel)
        Pr, qr, Ar, lr, ur = common.dense_from_csc(g, r, prefix="")
        assert np.array_equal(P, Pr) and np.array_equal(q, qr) and np.array_equal(Aq, Ar) and np.array_equal(l, lr) and np.array_equal(u, ur)
        assert g["cert_opt"][r] < 1e-8


@pytest.mark.parametrize("name", ["lmpc_30laps_n12", "lmpc_30laps_stress_n12"])
def test_30_lap_stores_restatement_matches_reference(name):
    """BASELINE configs[2] on the executed reference (lmpc_30laps_n12.npz): 30 laps of different lengths through PredictiveModel.addTrajectory's
    sorted insert and LMPC.addTrajectory; regression over the first four of the sorted store, selection over the four fastest laps.
    lmpc_30laps_stress_n12.npz: the same laps with numSS_it = trToUse = 30, numSS_Points = 360 (SURVEY 8(d)'s stress variant) -- every lap in the
    regression (PredictiveModel.py:31, 52-58) and in the safe set (PredictiveControllers.py:395-412)."""
    g = common.load_30laps_golden(name)
    N = int(g["N"]); nl = int(g["nLaps"]); TL = float(g["trackLength"]); L = int(g["numSS_it"]); S = int(g["numSS_Points"])
    par = orc.QPParams.lmpc_default(N)
    model = orc.OracleModel(g["track"], int(g["trToUse"]))
    for i in range(nl):
        model.addTrajectory(g["lapx%d" % i], g["lapu%d" % i])
    order = [[j for j in range(nl) if g["lapx%d" % j].shape == xs.shape and np.array_equal(g["lapx%d" % j], xs)][0] for xs in model.xStored]
    assert np.array_equal(order, g["modelOrder"])
    SS = [g["lapx%d" % i] for i in range(nl)]; uSS = [g["lapu%d" % i] for i in range(nl)]
    Qf = [orc.compute_cost(g["lapx%d" % i], TL) for i in range(nl)]
    for i in range(nl):
        assert np.array_equal(Qf[i], g["Qfun%d" % i])
    for r in range(g["x0"].shape[0]):
        A, B, C = orc.compute_ltv_dynamics(model.xStored, model.uStored, model.usedIt, g["track"], g["xLin"][r], g["uLin"][r], N)
        for got, ref in ((A, g["A"][r]), (B, g["B"][r]), (C, g["C"][r])):
            assert (np.abs(got - ref) / (1 + np.abs(ref))).max() < 1e-10
        zt = g["zt"][r].copy()
        if zt[4] - g["x0"][r][4] > TL / 2:
            zt[4] = np.max([zt[4] - TL, 0])
        xpp = g["xPredPrev"][r] if g["hasPred"][r] else None
        SSsel, Qsel, Succ, SuccU = orc.terminal_components(SS, uSS, Qf, list(g["LapTime"]), zt, S, L, xpp, nl, int(g["t"][r]), N, TL)
        assert np.array_equal(SSsel, g["SSsel"][r]) and np.array_equal(Qsel, g["Qsel"][r])
        assert np.array_equal(Succ, g["Succ"][r]) and np.array_equal(SuccU, g["SuccU"][r])
        P, q, Aq, l, u = orc.assemble_lmpc_qp(par, g["A"][r], g["B"][r], g["C"][r], g["x0"][r], g["OldInput"][r], SSsel, Qsel)
        Pr, qr, Ar, lr, ur = common.dense_from_csc(g, r, prefix="")
        assert np.array_equal(P, Pr) and np.array_equal(q, qr) and np.array_equal(Aq, Ar) and np.array_equal(l, lr) and np.array_equal(u, ur)
        assert g["cert_opt"][r] < 1e-8


def test_mpc_n14_restatement_matches_reference():
    """main.py's stages 2 and 3 at its own horizon N = 14, recorded from the executed reference (mpc_n14.npz): LTI MPC on Utilities.Regression's
    (A, B), LTV MPC on the local regressions -- assembled QPs bit-exact, regressions to 1e-10."""
    g = dict(np.load(common.GOLDEN + "/mpc_n14.npz"))
    N = int(g["N"])
    par = orc.QPParams.mpc_default(N, 0.8)
    for r in range(g["lti_x0"].shape[0]):
        P, q, A, l, u = orc.assemble_mpc_qp(par, g["A_lti"], g["B_lti"], None, g["lti_x0"][r], g["lti_OldInput"][r])
        Pr, qr, Ar, lr, ur = common.dense_from_csc(g, r, prefix="lti_")
        assert np.array_equal(P, Pr) and np.array_equal(q, qr) and np.array_equal(A, Ar) and np.array_equal(l, lr) and np.array_equal(u, ur)
    for r in range(g["ltv_x0"].shape[0]):
        A, B, C = orc.compute_ltv_dynamics([g["xPID"]], [g["uPID"]], [0], g["track"], g["ltv_xLin"][r], g["ltv_uLin"][r], N)
        for got, ref in ((A, g["ltv_A"][r]), (B, g["ltv_B"][r]), (C, g["ltv_C"][r])):
            assert (np.abs(got - ref) / (1 + np.abs(ref))).max() < 1e-10
        P, q, Aq, l, u = orc.assemble_mpc_qp(par, list(g["ltv_A"][r]), list(g["ltv_B"][r]), list(g["ltv_C"][r]), g["ltv_x0"][r], g["ltv_OldInput"][r])
        Pr, qr, Ar, lr, ur = common.dense_from_csc(g, r, prefix="ltv_")
        assert np.array_equal(P, Pr) and np.array_equal(q, qr) and np.array_equal(Aq, Ar) and np.array_equal(l, lr) and np.array_equal(u, ur)


def test_oracle_flow_reproduces_the_executed_reference_closed_loop():
    """tests/golden/reference_flow_laps_n14.json holds lap-length sequences of main.py's LMPC experiment (40 laps, N = 14) produced by the EXECUTED
    reference classes (LMPC + PredictiveModel + Simulator.sim, np.random.seed(s); tests/golden/make_flow_golden.py) and, beside them, the oracle's
    restatement of that flow on the same RandomState stream.  The restatement reproduces the executed reference lap for lap while round-off has not
    been amplified (the two regressions agree to 1e-10, not to the bit; the closed loop is chaotic at the scale of single steps from about lap 10 on)
    and stays within its scatter afterwards.  The first laps are re-run here."""
    import json
    from tests import closed_loop
    with open(common.GOLDEN + "/reference_flow_laps_n14.json") as f:
        d = json.load(f)
    assert d["flow"] == "executed reference"
    for seed, ref in d["laps40"].items():
        orc_ = d["oracle_laps40"][seed]
        assert len(ref) == 40 and len(orc_) == 40
        same = next((i for i, (a, b) in enumerate(zip(ref, orc_)) if a != b), 40)
        assert same >= 10, (seed, same)                                  # identical for at least the first ten laps (measured 19 / 10 / 13)
        assert np.abs(np.array(ref) - np.array(orc_)).max() <= 6 and abs(np.mean(ref[-10:]) - np.mean(orc_[-10:])) <= 4.0
    for seed, ref in d["laps3"].items():
        assert ref == d["oracle_laps3"][seed], seed                     # eight seeds, three laps: identical
    g = common.load_lmpc_golden()
    live = closed_loop.run_laps(closed_loop.OracleFlow(g, 14, solver="osqp"), g, 3, seed=5, noise="legacy")     # ~15 s
    assert [r["steps"] for r in live] == d["laps40"]["5"][:3] == d["oracle_laps40"]["5"][:3]
    assert [r["lap_time"] for r in live] == d["qfun40"]["5"][:3]


def test_captured_closed_loop_singular_regressions_raise_in_the_oracle():
    """tests/golden/reg_singular_capture.npz (tools/capture_reg_singular.py on the GPU box: 768 rollouts, generation 2): the horizon points whose regression the
    HIP path flagged LMPC_ST_REG_SINGULAR in closed loop.  The oracle -- and the reference's cvxopt.qp (PredictiveModel.py:170-178) -- raises on exactly those
    points: no stored row lies inside the bandwidth h of the query (the predicted state has left the data: |wz| > 2, a ~ 4), the normal matrix is the zero matrix."""
    from oracle import lmpc_oracle as orc
    import os
    d = np.load(os.path.join(common.GOLDEN, "reg_singular_capture.npz"))
    N = int(d["N"]); laps = [(d["lapx%d" % j], d["lapu%d" % j]) for j in range(4)]
    xs, us = [l[0] for l in laps], [l[1] for l in laps]
    n_flag = 0
    for c in range(d["xLin"].shape[0]):
        for i in range(N):
            x, u = d["xLin"][c][i], d["uLin"][c][i]
            npts = sum(len(orc.compute_indices(xs[it], us[it], np.hstack((x[0:3], u)))[0]) for it in range(4))
            flagged = bool(d["rst"][c][i] & 2)
            if flagged:
                n_flag += 1
                assert npts == 0
                with pytest.raises(np.linalg.LinAlgError):
                    orc.regression_and_linearization(xs, us, [0, 1, 2, 3], d["track"], x, u)
            else:
                assert npts >= 5
                A, B, C = orc.regression_and_linearization(xs, us, [0, 1, 2, 3], d["track"], x, u)
                assert np.all(np.isfinite(A)) and np.all(np.isfinite(B)) and np.all(np.isfinite(C))
    assert n_flag == 6


# ---- round 6: reproducibility of the fixtures -------------------------------------------------------------------

def test_manifest_hashes_match_the_tree():
    """tests/golden/MANIFEST.json: content hash of every fixture, git blob hash of every generator and of the oracle sources the oracle-produced fields depend on.
    A fixture edited without its manifest entry, or an oracle edit without re-made fixtures (the round-5 staleness), fails here."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("golden_manifest", os.path.join(common.GOLDEN, "manifest.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    assert m.diff() == [], "run the generators, then `python tests/golden/manifest.py write`: %s" % m.diff()
    man = m.load()
    assert set(man["fixtures"]) >= {"lmpc_n12.npz", "lmpc_30laps_n12.npz", "lmpc_n40.npz", "reference_flow_laps_n14.json"}
    assert all(v["generator"] != "?" for v in man["fixtures"].values())


@pytest.mark.parametrize("name,prefix,records", [("lmpc_n12", "rec_", (0, 5, 11, 17, 23, 29, 35, 41, 47, 53, 59)), ("lmpc_wide_n12", "", (0, 6, 11)), ("lmpc_n14", "", (0, 5)),
                                                 ("lmpc_n40", "", (0, 3)), ("lmpc_30laps_n12", "", (0, 4)), ("lmpc_30laps_stress_n12", "", (0, 5)),
                                                 ("ltvmpc_n12", "", (0, 2)), ("ltvmpc_noslack_n12", "", (0, 3))])
def test_oracle_produced_fields_rederive_bit_for_bit(name, prefix, records):
    """The oracle-produced fields of the fixtures (`sol_opt`, `y_opt`, `cert_opt`: osqp_solve_exact on the reference-assembled QP stored next to them) come out of
    TODAY's oracle bit for bit -- 31 records over eight fixtures.  (The reference-produced fields are re-derived by the tests above and, where /root/reference exists,
    by re-running the generators.)"""
    g = np.load(common.GOLDEN + "/%s.npz" % name)
    for r in records:
        if r >= g[prefix + "q"].shape[0]:
            continue
        P, q, A, l, u = common.dense_from_csc(g, r, prefix=prefix)
        ex, cert = orc.osqp_solve_exact(P, q, A, l, u)
        assert np.array_equal(ex.x, g[prefix + "sol_opt"][r]), (name, r, np.abs(ex.x - g[prefix + "sol_opt"][r]).max())
        if prefix + "y_opt" in g.files:
            assert np.array_equal(ex.y, g[prefix + "y_opt"][r]), (name, r)
        assert cert == g[prefix + "cert_opt"][r] and cert < 1e-9


@pytest.mark.parametrize("N", [8, 12, 14, 20, 40])
def test_active_fixture_rederives_bit_for_bit(N):
    """tests/golden/lmpc_active.npz (make_active_golden.py; oracle-made throughout, no reference tree): of every horizon's directed problems the three whose A, B, C and
    selection are stored (first, middle, last) and two more come out of TODAY's oracle bit for bit -- regression, selection with successors, the optimum of
    osqp_solve_exact and both certificates -- and so do two closed-loop records per horizon from their stored A, B, C, SS, Qsel.  (The stores and the records' inputs
    come from a 30-lap closed loop of 40 s per horizon, which is not run again here; the manifest holds their content hash.)"""
    from tests import active_cases as ac
    f = ac.load()
    inp = ac.fixture_inputs(f, N)
    p = "n%d_" % N
    K = inp["x0"].shape[0]
    k1 = [int(b) for b in f[p + "k1"]]
    idx = sorted(set(k1) | {K // 4, (3 * K) // 4})
    for r in ac.oracle_records(f, N, inp, idx, solve=True, procs=1):
        b = r["b"]
        assert ac.admitted(r, N), (N, b)
        z = ac.split(r["opt"], N)
        for j, k in enumerate(("x", "u", "slack", "lambd", "sTerm")):
            assert np.array_equal(z[j], f[p + k][b]), (N, b, k)
        assert r["cert"] == f[p + "cert"][b][0] and r["cert2"] == f[p + "cert"][b][1]
        assert ac.active_counts(r["opt"], N) == (f[p + "nact_slack"][b], f[p + "nact_u"][b]) and ac.lambda_unique(r, N) == bool(f[p + "lam_unique"][b])
        if b in k1:
            for k in ("A", "B", "C", "SSsel", "Qsel", "Succ", "SuccU"):
                assert np.array_equal(np.asarray(r[k]), f[p + k][k1.index(b)]), (N, b, k)
    if N in ac.CL_HORIZONS:
        p = "cl%d_" % N
        par = orc.QPParams.lmpc_default(N)
        for b in (0, 31):
            P, q, A, l, u = orc.assemble_lmpc_qp(par, f[p + "A"][b], f[p + "B"][b], f[p + "C"][b], f[p + "x0"][b], f[p + "uOld"][b], f[p + "SS"][b], f[p + "Qsel"][b])
            ex, cert = orc.osqp_solve_exact(P, q, A, l, u)
            z = ac.split(ex.x, N)
            for j, k in enumerate(("x", "u", "slack", "lambd", "sTerm")):
                assert np.array_equal(z[j], f[p + k][b]), (N, b, k)
            assert cert == f[p + "cert"][b][0] and cert <= 1e-8


def test_dense_ipm_active_set_finish_reaches_the_optimum():
    """Round 6: the oracle's dense interior-point solver ends with an active-set finish (the reference's own polish idea, PredictiveControllers.py:275).  On flat /
    degenerate closed-loop QPs the interior iterate alone sat up to 7e-6 from the optimum with every residual test met -- found when the HIP kernels, with their
    a-posteriori step bound, turned out to be closer to a 1e-15 solve than their checker.  Here: recorded QPs, the finished point against the polished ADMM optimum."""
    g = common.load_lmpc_golden()
    for r in (0, 13, 31, 47, 59):
        P, q, A, l, u = common.dense_from_csc(g, r)
        r2 = orc.dense_ipm_solve(P, q, A, l, u)
        assert not r2.interior, r                                           # the finish was accepted
        assert max(orc.kkt_certificate(P, q, A, l, u, r2.x, r2.y).values()) < 1e-10
        assert np.abs(r2.x[:102] - g["rec_sol_opt"][r][:102]).max() < 1e-9     # (x, u) are unique
        r3 = orc.dense_ipm_solve(P, q, A, l, u, polish=False)
        assert r3.interior and np.abs(r3.x[:102] - r2.x[:102]).max() < 1e-5


def test_longdouble_plant_reference_is_pinned_to_the_oracle():
    """tests/plant_ref.dyn_model_ld (the high-precision plant the GPU plant tests measure against) against orc.dyn_model on every state family
    of tests/test_gpu_plant_track.py: the raise / no-raise decision agrees on every state, and on the smooth families the states agree to
    1e-13 (1 + |x|).  The other families are judged by the oracle itself (headings beyond 1.5e3, segment and lap boundaries) or by the
    longdouble reference alone (|1 - cur ey| down to 1e-6, where the float64 oracle loses 1e-10 relative)."""
    from tests import plant_ref as pr
    g = common.load_lmpc_golden()
    pt = np.array(g["track"])
    for f in pr.families(g):
        xn, xgn, raised, _ = pr.dyn_model_ld(pt, f.x, f.xg, f.u, f.nz)
        worst = 0.0
        for b in range(len(f)):
            o = pr.oracle_step(pt, f.x[b], f.xg[b], f.u[b], f.nz[b])
            assert (o is None) == bool(raised[b]), (f.name, b, f.x[b])
            if o is not None:
                worst = max(worst, pr.scaled_err(xn[b:b + 1], o[0])[0], pr.scaled_err(xgn[b:b + 1], o[1])[0])
        print("%-18s %4d states  %3d raise  longdouble vs oracle %.2e" % (f.name, len(f), raised.sum(), worst))
        if f.smooth:
            assert worst <= 1e-13, f.name
