"""-m gpu: the three stages in front of the LMPC laps (main.py:61-95) as device-resident batches -- lmpc_rollout_pid, lmpc_lti_regression_batch,
lmpc_rollout_begin_mpc (LTI path-following MPC and LTV-MPC) -- against the oracle, against the host-stepped loops over the existing entry points,
and against the drop-in MPC class."""
import multiprocessing as mp

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

X0 = np.array([0.5, 0, 0, 0, 0, 0.0])
_JOB = {}


@pytest.fixture(scope="module")
def g(built):
    return common.load_lmpc_golden()


def _pool_map(fn, items, procs=14):
    """fn over items in forked children that never touch HIP (they read _JOB, run NumPy, return arrays): tests/oracle_pool.py's pattern."""
    try:
        from threadpoolctl import threadpool_limits
        threadpool_limits(1)
    except Exception:                                  # noqa: BLE001
        pass
    with mp.get_context("fork").Pool(min(procs, max(1, len(items)))) as pool:
        return pool.map_async(fn, items, chunksize=max(1, len(items) // (4 * procs))).get(timeout=420)


def _pid_u(x, vt, nu):
    """Utilities.PID.solve (Utilities.py:60-67) for all cars, as bench.pid_laps writes it."""
    return np.stack([-0.6 * x[:, 5] - 0.9 * x[:, 3] + np.clip(nu[:, 0] * 0.25, -0.9, 0.9), 1.5 * (vt - x[:, 0]) + np.clip(nu[:, 1] * 0.10, -0.2, 0.2)], axis=1)


def _plant_car(b):
    """max over the logged steps of car b of |device row t + 1 - oracle.dyn_model(device row t)|."""
    from oracle import lmpc_oracle as orc
    X, U, G, nz, pt = _JOB["X"], _JOB["U"], _JOB["G"], _JOB["nz"], _JOB["pt"]
    worst = 0.0
    for t in range(X.shape[0] - 1):
        it = iter(nz[t, b])
        xo, go = orc.dyn_model(pt, X[t, b], G[t, b], U[t, b], lambda: next(it))
        worst = max(worst, np.abs(X[t + 1, b] - xo).max(), np.abs(G[t + 1, b] - go).max())
    return worst


def test_pid_rollout_matches_the_oracle_step_by_step(g):
    """lmpc_rollout_pid, 64 cars at vt = 0.6 + 0.02 (b mod 30), 300 steps.  Every logged step: u_t equals the control law evaluated in NumPy on the device's own row t
    (bit for bit: the kernel rounds every product and sum on its own), and row t + 1 is within 1e-12 of oracle.dyn_model(row t, u_t, draws of step t) -- the bound of
    test_plant_kernel_matches_reference_plant for one plant step; nothing accumulates because every step starts from the device's own previous row.
    One car additionally replays oracle.pid_lap(track, 0.8, seed 3) over its 1000 steps with the draws of RandomState(3) in the oracle's order (two for the control
    law, three for the plant, per step).  Measured whole-lap deviation (max over x, u, x_glob and the 1000 steps) on MI355X: 4.33e-14; asserted with a factor 10 over it.
    Measured worst one-step error of the 64 cars: 3.6e-15."""
    from oracle import lmpc_oracle as orc
    from racinglmpc_amd import _capi
    B, T = 64, 300
    cfg, _ = common.mpc_config(g, 12, max_batch=B)
    ctx = _capi.Context(cfg)
    pt = np.array(g["track"])
    rng = np.random.default_rng(21)
    vt = 0.6 + 0.02 * (np.arange(B) % 30)
    nu = rng.standard_normal((T, B, 2)) * 2.0; nz = rng.standard_normal((T, B, 3)) * 2.0        # (x 2: both clips are exercised)
    x0 = np.tile(X0, (B, 1))
    t, nd = ctx.rollout_pid(x0, x0, vt, nu, nz)
    assert t == T
    X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
    ctx.rollout_end()
    assert np.all(st == 0) and np.array_equal(X[0], x0)
    for k in range(T):
        assert np.array_equal(U[k], _pid_u(X[k], vt, nu[k])), k
    _JOB.update(X=X, U=U, G=G, nz=nz, pt=pt)
    worst = max(_pool_map(_plant_car, list(range(B))))
    _JOB.clear()
    print("PID rollout: worst |row t+1 - oracle.dyn_model(row t)| over %d steps x %d cars: %.3e; %d cars crossed the line" % (T - 1, B, worst, nd))
    assert worst < 1e-12
    for b in range(B):                                                                           # doneAt / finX: first row past the line
        past = np.where(X[1:, b, 4] > float(g["trackLength"]))[0]
        assert done[b] == past[0] + 1 if len(past) else done[b] in (-1, T)                       # (the state after the last step is not a logged row)
        if 0 < done[b] < T:
            assert np.array_equal(fx[b], X[done[b], b]) and np.array_equal(fg[b], G[done[b], b])
    # one car, the whole lap of oracle.pid_lap
    seed, T1 = 3, 1000
    xo, uo, go = orc.pid_lap(pt, 0.8, seed)
    d = np.random.RandomState(seed).randn(T1, 5)
    t, _ = ctx.rollout_pid(X0[None], X0[None], [0.8], d[:, None, 0:2], d[:, None, 2:5])
    X, U, G, done, st, _, _ = ctx.rollout_fetch(0, t)
    ctx.rollout_end(); ctx.close()
    dev = max(np.abs(X[:, 0] - xo).max(), np.abs(U[:, 0] - uo).max(), np.abs(G[:, 0] - go).max())
    print("PID rollout: whole-lap deviation from oracle.pid_lap over %d steps: %.3e" % (T1, dev))
    assert t == T1 and xo.shape == (T1, 6) and st[0] == 0
    assert dev < PID_LAP_DEVIATION * 10


PID_LAP_DEVIATION = 4.33e-14       # measured whole-lap deviation (MI355X) of the device PID lap from oracle.pid_lap; the assertion allows ten times this


def test_pid_rollout_is_bit_identical_to_the_host_stepped_loop(g):
    """The same cars and draws stepped through plant_step_batch with the control law in NumPy (bench.pid_laps' loop) give the same X, U, Xglob, doneAt bit for bit:
    the kernel calls the device function lmpc_plant_step_batch calls.  Also: stop_at_line logs a car up to its crossing step only."""
    from racinglmpc_amd import _capi
    B, T = 64, 400
    cfg, _ = common.mpc_config(g, 12, max_batch=B)
    ctx = _capi.Context(cfg)
    TL = float(g["trackLength"])
    rng = np.random.default_rng(22)
    vt = 0.6 + 0.02 * (np.arange(B) % 30)
    nu = rng.standard_normal((T, B, 2)); nz = rng.standard_normal((T, B, 3))
    x = np.tile(X0, (B, 1)); xg = x.copy()
    Xh, Uh, Gh = [], [], []; done_h = -np.ones(B, np.int32)
    for k in range(T):
        u = _pid_u(x, vt, nu[k])
        Xh.append(x.copy()); Uh.append(u); Gh.append(xg.copy())
        x, xg, st = ctx.plant_step_batch(x, xg, u, nz[k])
        done_h[(done_h < 0) & (x[:, 4] > TL)] = k + 1
    x0 = np.tile(X0, (B, 1))
    t, nd = ctx.rollout_pid(x0, x0, vt, nu, nz)
    X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
    ctx.rollout_end()
    assert t == T and nd == int((done_h >= 0).sum()) and nd > B // 2
    assert np.array_equal(X, np.stack(Xh)) and np.array_equal(U, np.stack(Uh)) and np.array_equal(G, np.stack(Gh)) and np.array_equal(done, done_h)
    t2, nd2 = ctx.rollout_pid(x0, x0, vt, nu, nz, stop_at_line=True)
    X2, U2, G2, done2, st2, fx2, fg2 = ctx.rollout_fetch(0, t2)
    ctx.rollout_end(); ctx.close()
    assert np.array_equal(done2, done) and np.array_equal(fx2, fx) and t2 == (done.max() if nd == B else T)
    for b in range(B):
        n = done[b] if done[b] >= 0 else T
        assert np.array_equal(X2[:n, b], X[:n, b]) and np.array_equal(U2[:n, b], U[:n, b]) and not X2[n:, b].any()


def _lti_laps(g, n):
    """n laps of different lengths cut from the recorded PID lap (1000 rows) and the two recorded LMPC laps."""
    src = [(np.array(g["xPID"]), np.array(g["uPID"])), (np.array(g["lapx0"]), np.array(g["lapu0"]))]
    laps = []
    for i in range(n):
        x, u = src[i % 2]
        a = (17 * i) % 50; T = min(x.shape[0] - a, 120 + 53 * i)
        laps.append((x[a:a + T].copy(), u[a:a + T].copy()))
    return laps


def test_batched_lti_regression(g):
    """lmpc_lti_regression_batch on 16 laps of different lengths against oracle.lti_regression at the bound of test_lti_regression_kernel_matches_reference
    (1e-7 (1 + |ref|) on A, B; 1e-9 on the residual extrema); B = 1 is bit-identical to lmpc_lti_regression, and so is every lap of the batch."""
    from oracle import lmpc_oracle as orc
    from racinglmpc_amd import _capi
    laps = _lti_laps(g, 16)
    assert len({x.shape[0] for x, _ in laps}) >= 12
    lamb = 1e-7
    A, B, E, st = _capi.lti_regression_batch(laps, lamb)
    assert np.all(st == 0)
    worst = 0.0
    for b, (x, u) in enumerate(laps):
        Ar, Br, Er = orc.lti_regression(x, u, lamb)
        err = max((np.abs(A[b] - Ar) / (1 + np.abs(Ar))).max(), (np.abs(B[b] - Br) / (1 + np.abs(Br))).max())
        worst = max(worst, err)
        assert err < 1e-7 and np.abs(E[b] - Er).max() < 1e-9, (b, err, np.abs(E[b] - Er).max())
        A1, B1, E1, s1 = _capi.lti_regression(x, u, lamb)
        assert np.array_equal(A1, A[b]) and np.array_equal(B1, B[b]) and np.array_equal(E1, E[b]) and s1 == 0
        Ab, Bb, Eb, sb = _capi.lti_regression_batch([(x, u)], lamb)
        assert np.array_equal(A1, Ab[0]) and np.array_equal(B1, Bb[0]) and np.array_equal(E1, Eb[0])
    print("batched LTI regression: worst rel err of A, B against the oracle %.2e" % worst)
    _, _, _, st = _capi.lti_regression_batch([laps[0], (np.zeros((30, 6)), np.zeros((30, 2)))], 0.0)
    assert st[0] == 0 and st[1] == _capi.ST_REG_SINGULAR
    with pytest.raises(_capi.LmpcError):
        _capi.lti_regression_batch([(np.zeros((2, 6)), np.zeros((2, 2)))], lamb)


def _mpc_setup(g, B, ltv, max_batch=None):
    """Context (initMPCParams values, N = 12), start states, and what selects the form: per-rollout (A_b, B_b) fitted to different cuts of the recorded laps, or the first
    linearisation trajectory of MPC.__init__ (:88-90) with the PID lap in the regression store."""
    from racinglmpc_amd import _capi
    cfg, par = common.mpc_config(g, 12, max_batch=max_batch or B)
    ctx = _capi.Context(cfg)
    x0 = np.tile(X0, (B, 1)); x0[:, 5] = np.linspace(-0.15, 0.15, B) if B > 1 else 0.0; x0[:, 0] = 0.5 + 0.01 * (np.arange(B) % 7)
    if ltv:
        ctx.model_add_trajectory(g["xPID"], g["uPID"])
        return ctx, par, x0, dict(xLin0=np.tile(g["xPID"][None, 0:13], (B, 1, 1)), uLin0=np.tile(g["uPID"][None, 0:12], (B, 1, 1)))
    laps = [(np.array(g["xPID"])[7 * b:], np.array(g["uPID"])[7 * b:]) for b in range(B)]
    A, Bm, E, st = _capi.lti_regression_batch(laps, 1e-7)
    assert np.all(st == 0)
    return ctx, par, x0, dict(A=A, B=Bm)


def _host_stepped(ctx, x0, form, noise, on_step=None):
    """The loop the parent commit offers: qp_solve_batch (LTI) / step_batch (LTV) + plant_step_batch per step, the tail of MPC.solve (:129-137) in NumPy."""
    N, B = ctx.N, x0.shape[0]
    x = x0.copy(); xg = x0.copy(); uOld = np.zeros((B, 2))
    X, U, G = [], [], []
    ltv = "xLin0" in form
    if ltv:
        xLin, uLin = form["xLin0"].copy(), form["uLin0"].copy()
    else:
        A = np.tile(form["A"][:, None], (1, N, 1, 1)); Bm = np.tile(form["B"][:, None], (1, N, 1, 1)); C = np.zeros((B, N, 6))
    for t in range(noise.shape[0]):
        out = ctx.step_batch(x, xLin, uLin, uOld) if ltv else ctx.qp_solve_batch(A, Bm, C, x, uOld)
        assert np.all((out["status"] & ~64) == 0), (t, out["status"])
        if on_step is not None:
            on_step(t, x, uOld, out)
        u = out["uPred"][:, 0].copy()
        X.append(x.copy()); U.append(u); G.append(xg.copy())
        x, xg, st = ctx.plant_step_batch(x, xg, u, noise[t])
        if ltv:
            xLin = np.concatenate([out["xPred"][:, 1:], out["xPred"][:, N:N + 1]], axis=1)
            uLin = np.concatenate([out["uPred"][:, 1:], out["uPred"][:, N - 1:N]], axis=1)
        uOld = u
    return np.stack(X), np.stack(U), np.stack(G)


@pytest.mark.parametrize("ltv", [False, True], ids=["lti", "ltv"])
def test_mpc_sessions_equal_the_host_stepped_loop(g, ltv):
    """B = 32, N = 12, initMPCParams values, 150 steps: the session's X, U, Xglob logs equal, bit for bit, those of the loop over qp_solve_batch (LTI) / step_batch
    (LTV) + plant_step_batch + the shift in NumPy at the same batch size -- the same kernels on the same route see the same inputs."""
    B, T = 32, 150
    ctx, par, x0, form = _mpc_setup(g, B, ltv)
    noise = np.random.default_rng(31).standard_normal((T, B, 3))
    ctx.rollout_begin_mpc(x0, x0, noise, **form)
    t, nd = ctx.rollout_run(T)
    X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
    ctx.rollout_end()
    assert t == T and np.all((st & ~64) == 0)
    Xh, Uh, Gh = _host_stepped(ctx, x0, form, noise)
    ctx.close()
    bad = [k for k in range(T) if not (np.array_equal(X[k], Xh[k]) and np.array_equal(U[k], Uh[k]) and np.array_equal(G[k], Gh[k]))]
    print("%s session against the host-stepped loop: %d of %d steps differ%s" % ("LTV-MPC" if ltv else "LTI-MPC", len(bad), T,
          "" if not bad else "; first at step %d: |dX| %.3e |dU| %.3e" % (bad[0], np.abs(X[bad[0]] - Xh[bad[0]]).max(), np.abs(U[bad[0]] - Uh[bad[0]]).max())))
    assert not bad
    assert np.abs(X[-1, :, 5]).max() < 0.4                                             # the cars hold the centre line


def _qp_job(k):
    from oracle import lmpc_oracle as orc
    q = _JOB["qps"][k]; par = _JOB["par"]
    res = {}
    if q["ltv"]:
        A, B, C = orc.compute_ltv_dynamics([_JOB["xP"]], [_JOB["uP"]], [0], _JOB["pt"], q["xLin"], q["uLin"], par.N)
        res["abc"] = max((np.abs(got - np.array(ref)) / (1 + np.abs(np.array(ref)))).max() for got, ref in ((q["A"], A), (q["B"], B), (q["C"], C)))
    P, qq, Ao, lo, up = orc.assemble_mpc_qp(par, list(q["A"]), list(q["B"]), list(q["C"]), q["x0"], q["uOld"])
    ex, cert = orc.osqp_solve_exact(P, qq, Ao, lo, up, want=1e-8)
    N = par.N
    res.update(cert=cert, xu=max(np.abs(q["xPred"].ravel() - ex.x[:6 * (N + 1)]).max(), np.abs(q["uPred"].ravel() - ex.x[6 * (N + 1):6 * (N + 1) + 2 * N]).max()))
    return res


@pytest.mark.parametrize("ltv", [False, True], ids=["lti", "ltv"])
def test_every_sampled_closed_loop_qp_against_the_oracle(g, ltv):
    """The sessions of the test above stepped with rollout_run(1): every 5th step of 8 cars, the QP the step solved (debug_rollout_qp: A, B, C, the answer; x0 / uOld:
    rows t - 1 / t - 2 of the logs) goes to oracle.assemble_mpc_qp + osqp_solve_exact: |xPred, uPred - z*| < 1e-6 (common.TOL_XU); LTV: A, B, C against
    oracle.compute_ltv_dynamics on the linearisation trajectory the step was asked (debug_rollout_peek before the step) to 3e-10 relative."""
    B, T, NB = 32, 150, 8
    ctx, par, x0, form = _mpc_setup(g, B, ltv)
    noise = np.random.default_rng(31).standard_normal((T, B, 3))
    ctx.rollout_begin_mpc(x0, x0, noise, **form)
    qps = []
    for k in range(T):
        sample = k % 5 == 0
        if sample and ltv:
            xl, ul, _, _ = ctx.debug_rollout_peek(B)
        t, _ = ctx.rollout_run(1)
        assert t == k + 1
        if sample:
            o = ctx.debug_rollout_qp(0, NB, selection=False)
            X, U, _, _, _, _, _ = ctx.rollout_fetch(max(0, k - 1), k + 1)
            assert np.all((o["status"] & ~64) == 0)
            for b in range(NB):
                qps.append(dict(ltv=ltv, A=o["A"][b], B=o["B"][b], C=o["C"][b], xPred=o["xPred"][b], uPred=o["uPred"][b], x0=X[-1, b],
                                uOld=U[0, b] if k > 0 else np.zeros(2), xLin=xl[b] if ltv else None, uLin=ul[b] if ltv else None))
                assert np.array_equal(o["xPred"][b][0], X[-1, b]) and np.array_equal(o["ztNext"][b], o["xPred"][b][-1]) and np.array_equal(o["ztuNext"][b], o["uPred"][b][-1])
                if not ltv:
                    assert np.array_equal(o["A"][b], np.tile(form["A"][b], (12, 1, 1))) and np.array_equal(o["B"][b], np.tile(form["B"][b], (12, 1, 1))) and not o["C"][b].any()
    ctx.rollout_end(); ctx.close()
    _JOB.update(qps=qps, par=par, pt=np.array(g["track"]), xP=np.array(g["xPID"]), uP=np.array(g["uPID"]))
    res = _pool_map(_qp_job, list(range(len(qps))))
    _JOB.clear()
    xu = max(r["xu"] for r in res); cert = max(r["cert"] for r in res); abc = max(r.get("abc", 0.0) for r in res)
    print("%s session: %d closed-loop QPs: worst |xu - z*| %.2e (oracle certificate %.1e), worst rel |A,B,C - oracle| %.2e" % ("LTV-MPC" if ltv else "LTI-MPC", len(res), xu, cert, abc))
    assert cert < 1e-7 and xu < common.TOL_XU and abc < 3e-10


def test_one_car_session_reproduces_the_dropin_mpc(g, monkeypatch):
    """One LTV-MPC car through the session and through racinglmpc_amd.PredictiveControllers.MPC driven by tests/test_gpu_dropin_main.py::_sim, same draws: both run the
    B = 1 route, so X, U, Xglob agree bit for bit.  _sim integrates with oracle.dyn_model, which differs from the plant kernel in the last bits (1e-13 per step:
    test_plant_kernel_matches_reference_plant), and a closed loop would carry that difference on; so for this test _sim's plant is the library's own
    lmpc_plant_step_batch (oracle.dyn_model is replaced while _sim runs, _sim itself is imported as it is) -- what is compared is the controller."""
    from oracle import lmpc_oracle as orc
    from racinglmpc_amd import PredictiveControllers as PC, PredictiveModel as PM
    from tests.test_gpu_dropin_main import _Map, _sim
    N, T, vt = 12, 120, 0.8
    map_ = _Map(g); pt, TL = map_.PointAndTangent, map_.TrackLength
    Fx = np.array([[0., 0., 0., 0., 0., 1.], [0., 0., 0., 0., 0., -1.]]); Fu = np.kron(np.eye(2), np.array([1, -1])).T

    def make():
        p = PC.MPCParams(n=6, d=2, N=N, Q=np.diag([1.0, 1.0, 1, 1, 0.0, 100.0]), R=np.diag([1.0, 10.0]), Fx=Fx, bx=(np.array([[2.], [2.]]),), Fu=Fu,
                         bu=np.array([[0.5], [0.5], [10.0], [10.0]]), xRef=np.array([vt, 0, 0, 0, 0, 0]), slacks=True, Qslack=1 * np.array([0, 50]))
        p.timeVarying = True
        pm = PM.PredictiveModel(6, 2, map_, 1); pm.addTrajectory(g["xPID"], g["uPID"])
        return PC.MPC(p, pm)
    a, b = make(), make()
    noise = np.random.default_rng(41).standard_normal((T, 1, 3))
    ctx = a._ctx
    ctx.rollout_begin_mpc(X0[None], X0[None], noise, xLin0=np.asarray(a.xLin, float)[None, 0:N + 1], uLin0=np.asarray(a.uLin, float)[None])
    t, _ = ctx.rollout_run(T)
    X, U, G, done, st, _, _ = ctx.rollout_fetch(0, t)
    ctx.rollout_end()
    assert t == T and (st[0] & ~64) == 0

    def device_plant(pt_, x, xg, u, randn):
        nz = np.array([randn(), randn(), randn()])
        xn, xgn, s = b._ctx.plant_step_batch(x[None], xg[None], u[None], nz[None])
        return xn[0], xgn[0]
    monkeypatch.setattr(orc, "dyn_model", device_plant)
    it = iter(noise.ravel())
    rng = type("Draws", (), {"standard_normal": staticmethod(lambda: next(it))})
    xS, uS, gS, _ = _sim(b, pt, TL, [X0, X0], rng, T)
    assert np.array_equal(X[:, 0], xS) and np.array_equal(U[:, 0], uS) and np.array_equal(G[:, 0], gS)


def test_argument_checks_and_memory_of_the_new_sessions(g):
    """lmpc_rollout_begin_mpc on an LMPC context and lmpc_rollout_begin on an MPC context: LMPC_E_ARG; the LTV form without stored laps: LMPC_E_STATE; a second begin
    inside a session is refused; B > max_batch and NULL combinations are refused; lmpc_rollout_release after each kind of session returns its memory."""
    import ctypes as C
    from racinglmpc_amd import _capi
    B, T = 64, 400
    noise = np.random.default_rng(51).standard_normal((T, B, 3)); nu = np.random.default_rng(52).standard_normal((T, B, 2))
    x0 = np.tile(X0, (B, 1))
    lm, _ = common.make_lmpc_ctx(g, 4, max_batch=B)
    ctx, par, _, lti = _mpc_setup(g, B, False)
    xl = np.tile(g["xPID"][None, 0:13], (B, 1, 1)); ul = np.tile(g["uPID"][None, 0:12], (B, 1, 1))

    def code(f):
        with pytest.raises(_capi.LmpcError) as e:
            f()
        return int(str(e.value).split()[2].rstrip(":"))
    assert code(lambda: lm.rollout_begin_mpc(x0, x0, noise, **lti)) == -1
    assert code(lambda: ctx.rollout_begin(x0, x0, xl, ul, noise)) == -1
    assert code(lambda: ctx.rollout_begin_mpc(x0, x0, noise, xLin0=xl, uLin0=ul)) == -4                       # no lap in the regression store
    big = np.tile(X0, (B + 1, 1))
    assert code(lambda: ctx.rollout_begin_mpc(big, big, np.zeros((T, B + 1, 3)), A=np.zeros((B + 1, 6, 6)), B=np.zeros((B + 1, 6, 2)))) == -1
    assert code(lambda: ctx.rollout_pid(big, big, np.ones(B + 1), np.zeros((T, B + 1, 2)), np.zeros((T, B + 1, 3)))) == -1
    p = lambda a: a.ctypes.data
    assert ctx.lib.lmpc_rollout_begin_mpc(ctx._h, B, T, p(x0), p(x0), None, None, p(lti["A"]), None, p(noise), 0) == -1      # A without B
    assert ctx.lib.lmpc_rollout_begin_mpc(ctx._h, B, T, p(x0), p(x0), p(xl), None, None, None, p(noise), 0) == -1            # LTV form without uLin0
    assert ctx.lib.lmpc_rollout_pid(ctx._h, B, T, p(x0), p(x0), None, p(nu), p(noise), 0, None, None) == -1                  # no target speeds
    ctx.model_add_trajectory(g["xPID"], g["uPID"])
    free0 = None
    for kind in ("warm", "lti", "ltv", "pid"):
        before = _capi.device_memory(0)[0]
        if kind == "pid":
            ctx.rollout_pid(x0, x0, np.full(B, 0.8), nu, noise)
        else:
            ctx.rollout_begin_mpc(x0, x0, noise, **(dict(xLin0=xl, uLin0=ul) if kind == "ltv" else lti))
        assert code(lambda: ctx.rollout_begin_mpc(x0, x0, noise, **lti)) == -1                                 # a session is active
        assert code(lambda: ctx.rollout_pid(x0, x0, np.full(B, 0.8), nu, noise)) == -1
        with pytest.raises(_capi.LmpcError):
            ctx.rollout_release()                                                                              # not inside a session
        if kind == "pid":
            assert code(lambda: ctx.rollout_run(1)) == -1                                                      # a PID session has run to its end
        else:
            assert ctx.rollout_run(8)[0] == 8
        alive = _capi.device_memory(0)[0]
        ctx.rollout_end(); ctx.rollout_release()
        after = _capi.device_memory(0)[0]
        print("%s session: free device memory before %.2f MB, alive %.2f MB, released %.2f MB" % (kind, before / 2**20, alive / 2**20, after / 2**20))
        if kind != "warm":                                       # (the first session also brings the code objects and the stream pool in)
            assert before - alive > 2**18 and abs(after - before) < 2**20, (kind, before, alive, after)
    ctx.close(); lm.close()


def test_bootstrap_runs_the_three_stages_on_the_device(g):
    """rollout.bootstrap (main.py:61-95 for B cars), B = 4, 300 steps per stage: every stage returns one lap tuple per car with all logged rows, the LTI models are
    those of lmpc_lti_regression on each car's PID lap, the stages equal the lap runners called by hand with the same generator, and the shared regression store holds
    the PID laps nearest to the tracked speed.  (Seeding an LMPC generation from the laps: test_bootstrap_end_to_end.)"""
    from racinglmpc_amd import _capi, rollout
    B, N, T, seed = 4, 12, 300, 9
    vt = np.array([0.7, 0.8, 0.95, 0.82])
    out = rollout.bootstrap(g["track"], B, N, vt, seed, max_steps=T, vt_mpc=0.8)
    assert out["store_laps"] == [1, 3, 0, 2] and np.all(out["lti_status"] == 0)
    for k in ("pid", "mpc", "ltvmpc"):
        assert len(out[k]) == B and all(l[0].shape == (T, 6) and l[1].shape == (T, 2) and l[2].shape == (T, 6) for l in out[k]), k
        print("bootstrap %s: done_at %s status %s" % (k, [l[4] for l in out[k]], [l[5] for l in out[k]]))
    assert all(l[5] == 0 for l in out["pid"])
    for b in range(B):
        A1, B1, E1, _ = _capi.lti_regression(out["pid"][b][0], out["pid"][b][1], rollout.LTI_LAMB)
        assert np.array_equal(A1, out["A"][b]) and np.array_equal(B1, out["B"][b]) and np.array_equal(E1, out["Error"][b])
    ctx = _capi.Context(rollout.mpc_stage_config(g["track"], N, 0.8, B, trToUse=4))
    ro = rollout.BatchedRollouts(ctx, g["track"], seed=seed, prefetch=False)
    x0 = np.tile(X0, (B, 1))
    pid = ro.run_pid_laps(vt, x0, max_steps=T, keep_invalid=True)
    mpc = ro.run_mpc_laps(x0, A=out["A"], B=out["B"], max_steps=T, keep_invalid=True)
    for b in out["store_laps"]:
        ctx.model_add_trajectory(pid[b][0], pid[b][1])
    ltv = ro.run_mpc_laps(x0, xLin0=pid[2][0][0:N + 1], uLin0=pid[2][1][0:N], max_steps=T, keep_invalid=True)
    ro.close(); ctx.close()
    for mine, theirs in ((pid, out["pid"]), (mpc, out["mpc"]), (ltv, out["ltvmpc"])):
        assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) and p[4] == q[4] and p[5] == q[5] for p, q in zip(mine, theirs))


def test_stop_at_line_ends_an_mpc_session_at_the_poll_after_the_last_crossing(g):
    """LTI-MPC session, 8 cars, T_max = 400: with stop_at_line the run ends at the first finished-lap poll (every 8 steps) after the last car has crossed the line;
    without it all 400 steps are simulated and doneAt keeps the first crossing.  Same draws: the common rows and doneAt agree bit for bit."""
    B, T = 8, 400
    ctx, par, x0, form = _mpc_setup(g, B, False)
    noise = np.random.default_rng(61).standard_normal((T, B, 3))
    ctx.rollout_begin_mpc(x0, x0, noise, stop_at_line=True, **form)
    t1, nd1 = ctx.rollout_run(T)
    X1, U1, G1, done1, st1, fx1, fg1 = ctx.rollout_fetch(0, t1)
    ctx.rollout_end()
    assert nd1 == B and np.all(done1 > 0) and np.all((st1 & ~64) == 0)
    assert t1 < T and t1 == 8 * ((int(done1.max()) + 7) // 8)
    ctx.rollout_begin_mpc(x0, x0, noise, **form)
    t0, nd0 = ctx.rollout_run(T)
    X0_, U0_, G0_, done0, st0, fx0, fg0 = ctx.rollout_fetch(0, t0)
    ctx.rollout_end(); ctx.close()
    assert t0 == T and nd0 == B and np.array_equal(done0, done1) and np.array_equal(fx0, fx1) and np.array_equal(fg0, fg1)
    assert np.array_equal(X0_[:t1], X1) and np.array_equal(U0_[:t1], U1) and np.all(X0_[-1, :, 4] > float(g["trackLength"]))


def test_bootstrap_end_to_end(g):
    """rollout.bootstrap(track, B = 16, N = 12, vt = 0.8, seed = 9, max_steps = 1000) -- main.py's own target speed and step count (main.py:50, 57) --, then an LMPC
    context seeded from the returned laps (rollout.seed_lmpc with the four PID laps of the shared store, main.py:102-110) runs one LmpcGeneration.run of 16 rollouts.
    Condition: ALL 16 cars yield a valid lap (finish line crossed, no status bit but INEXACT) in every stage, and every status word of the generation is clean in
    the same sense (the library's definition of a valid lap: racinglmpc_amd/rollout.py).

    Chosen on the CPU first (tools/bootstrap_precheck.py --cars 16 --vt 0.8 --seed 9 --steps 1000 --sim-steps 400: the oracle alone on the same draws -- PID loop,
    oracle.lti_regression, assemble_mpc_qp + osqp_solve_exact + dyn_model loops for the LTI and the LTV form, the first 400 of the 1000 steps, which is past every
    crossing; the oracle's regression store therefore holds the first 400 rows of the PID laps): every car finishes its lap in every stage; first rows past the line
    PID 284 .. 315, LTI-MPC 271 .. 297, LTV-MPC 325 (all cars); largest |ey| PID 0.432, LTI-MPC 0.069, LTV-MPC 0.022 (bound 2 = the MPC's bx); no QP left uncertified.
    On the device: PID 284 .. 315, LTI-MPC 275 .. 298, LTV-MPC 335; every status word 0."""
    from racinglmpc_amd import _capi, rollout
    B, N, T = 16, 12, 1000
    out = rollout.bootstrap(g["track"], B, N, 0.8, 9, max_steps=T)
    TL = float(g["trackLength"])
    for k in ("pid", "mpc", "ltvmpc"):
        done = np.array([l[4] for l in out[k]]); st = np.array([l[5] for l in out[k]]); ey = max(np.abs(l[0][:, 5]).max() for l in out[k])
        print("bootstrap %s: done_at %d .. %d, status bits %s, max |ey| %.3f" % (k, done.min(), done.max(), sorted(set(st.tolist())), ey))
        assert len(out[k]) == B and np.all(done > 0) and np.all((st & ~_capi.ST_INEXACT) == 0) and ey < 2.0, k
        assert all(l[0].shape == (T, 6) and l[0][l[4] - 1, 4] <= TL < l[0][-1, 4] for l in out[k]), k
    assert out["store_laps"] == [0, 1, 2, 3] and np.all(out["lti_status"] == 0)
    cfg, par = common.lmpc_config(g, N, max_batch=B)
    ctx = _capi.Context(cfg)
    seeds = [out["pid"][b] for b in out["store_laps"]]
    rollout.seed_lmpc(ctx, seeds)
    ro = rollout.BatchedRollouts(ctx, g["track"], seed=10)
    gen = rollout.LmpcGeneration(ro, B, K=4, T_max=400, ext=40)
    x0 = np.tile(X0, (B, 1)); x0[:, 5] = np.linspace(-0.05, 0.05, B)
    best = gen.run(x0, seeds[0][0][1:N + 2], seeds[0][1][1:N + 1])
    print("LMPC generation on the bootstrap laps: done_at %s status %s; best laps %s steps" % (gen.last_done.tolist(), gen.last_status.tolist(), [b[4] for b in best]))
    assert len(best) == 4 and np.all(gen.last_done > 0) and np.all((gen.last_status & ~_capi.ST_INEXACT) == 0)
    assert ctx.ss_num_laps() == 8 and max(b[4] for b in best) < min(l[4] for l in seeds)                       # the LMPC laps are faster than the PID laps
    gen.close(); ctx.close()
