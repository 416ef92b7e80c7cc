"""-m gpu: the per-problem lap table of the regression kernel (lmpc_model_set_lap_table): every car's A, B, C from its own laps.

Bit for bit against contexts that hold only a car's laps (include/lmpc_hip.h: A, B, C of a problem depend neither on the regression grid nor on the scan build, so a
context with other laps beside them -- hence possibly another scan build -- must give the same bits), against the oracle to the 3e-10 relative of
tests/test_gpu_mpc_stages.py, and end to end through rollout.bootstrap(per_car_store=True).  N = 12, numSS_it = 0 contexts.

Laps, three length classes: S and S2 (400 rows, cuts of the golden PID lap: inside the 8-rows-per-lane scan), M (800 rows: one quantisation chunk, 16 rows per lane),
L (1300 rows of a PID lap of run_pid_laps: a second chunk), XL (the 1500 rows of that lap: longer than the max_lap_len the growth test starts from), Z (400 all-zero
rows: a singular fit)."""
import ctypes as C

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

N = 12
_REF = {}                                              # (lap names, batch size, entry point, runtime kernel) -> results of a context holding only those laps


@pytest.fixture(scope="module")
def g(built):
    return common.load_lmpc_golden()


@pytest.fixture(scope="module")
def laps(g):
    from racinglmpc_amd import _capi, rollout
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    cfg, _ = common.mpc_config(g, N, max_batch=1)
    with _capi.Context(cfg) as ctx:
        ro = rollout.BatchedRollouts(ctx, g["track"], seed=77, prefetch=False)
        xl, ul = ro.run_pid_laps([0.8], max_steps=1500, keep_invalid=True)[0][:2]
        ro.close()
    assert xl.shape == (1500, 6) and np.all(np.isfinite(xl)) and np.all(np.isfinite(ul))
    out = dict(S=(xP[100:500], uP[100:500]), S2=(xP[500:900], uP[500:900]), M=(xP[150:950], uP[150:950]), L=(xl[:1300], ul[:1300]), XL=(xl, ul),
               E=(xP[200:600], uP[200:600]), E2=(xP[210:610], uP[210:610]), Z=(np.zeros((400, 6)), np.zeros((400, 2))))
    assert out["S"][0].shape[0] <= 512 < out["M"][0].shape[0] <= 1024 < out["L"][0].shape[0]
    return {k: (np.ascontiguousarray(x), np.ascontiguousarray(u)) for k, (x, u) in out.items()}


def _batch(g, B):
    """B linearisation trajectories: the rows of the golden PID lap that follow row 37 b mod 380 (the cars drive there; every lap of the fixture has rows nearby)."""
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    tb = (37 * np.arange(B)) % 380
    return np.stack([xP[t:t + N + 1] for t in tb]), np.stack([uP[t:t + N] for t in tb])


def _ctx(g, laps, names, trToUse, max_batch, runtime=False, **kw):
    from racinglmpc_amd import _capi
    cfg, _ = common.mpc_config(g, N, max_batch=max_batch, **kw)
    cfg.trToUse = trToUse
    ctx = _capi.Context(cfg, runtime_kernel=runtime)
    for k in names:
        ctx.model_add_trajectory(*laps[k])
    return ctx


def _only(g, laps, names, batch, runtime=False):
    """regress_batch of the batch (xLin, uLin) on a context holding exactly the laps `names` (trToUse = all of them), computed once per batch size."""
    xLin, uLin = batch
    B = xLin.shape[0]
    key = (tuple(names), B, "batch", runtime)
    if key not in _REF:
        with _ctx(g, laps, names, len(names), B, runtime) as ctx:
            _REF[key] = ctx.regress_batch(xLin, uLin)
    return _REF[key]


def _same(got, ref, b, what):
    for k, (p, q) in enumerate(zip(got, ref)):
        assert np.array_equal(p[b], q[b]), (what, b, "ABCs"[k], np.abs(p[b] - q[b]).max())


def _oracle(g, laps, names, xLin, uLin, n=N):
    """oracle.compute_ltv_dynamics on a model store holding exactly `names` (inserted as PredictiveModel.addTrajectory would), and the status the reference implies:
    LMPC_ST_REG_SINGULAR where its solve raises."""
    from oracle import lmpc_oracle as orc
    xs, us, lt = [], [], []
    for k in names:
        orc.model_sorted_insert(xs, us, lt, laps[k][0], laps[k][1])
    A, Bm, Cc, st = np.zeros((n, 6, 6)), np.zeros((n, 6, 2)), np.zeros((n, 6)), np.zeros(n, np.int32)
    for i in range(n):
        try:
            A[i], Bm[i], Cc[i] = orc.regression_and_linearization(xs, us, list(range(len(names))), np.array(g["track"]), xLin[i], uLin[i])
        except np.linalg.LinAlgError:
            st[i] = 2
    return A, Bm, Cc, st


OWN_TOL = 3e-11                                        # a tenth of the bound: what the oracle's own float64 arithmetic may cost a point that is judged against 3e-10


def _solve_ld(Q, r):
    """Q theta = r by Gaussian elimination with partial pivoting in longdouble (5 x 5)."""
    n = Q.shape[0]; M = np.hstack((Q.astype(np.longdouble), r.astype(np.longdouble)[:, None]))
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c]))); M[[c, p]] = M[[p, c]]
        for k in range(c + 1, n):
            M[k] = M[k] - M[c] * (M[k, c] / M[c, c])
    th = np.zeros(n, np.longdouble)
    for c in range(n - 1, -1, -1):
        th[c] = (M[c, n] - M[c, c + 1:n] @ th[c + 1:]) / M[c, c]
    return th


def _own_error(laps, names, x, u):
    """The oracle's own error at the point (x, u) on the laps `names`: its three local regressions (compute_Q_M / compute_b / LMPC_LocLinReg, PredictiveModel.py:141-178)
    as float64 NumPy evaluates them, against the same normal equations formed and solved in longdouble -- relative, |d theta| / (1 + |theta|).  The fits of a point are
    ill-conditioned where its nearest stored rows are consecutive samples of a smooth lap (condition 1e6 .. 3e7 on these laps): there the reference itself does not
    carry ten digits, and no implementation can be held to 3e-10 of it."""
    from oracle import lmpc_oracle as orc
    xu = np.hstack((x[0:3], u))
    sel = [(k,) + tuple(orc.compute_indices(laps[k][0], laps[k][1], xu)) for k in names]
    worst = 0.0
    for feat, ys in ((1, (0,)), (0, (1, 2))):
        M = np.vstack([np.hstack((laps[k][0][idx][:, 0:3], laps[k][1][idx][:, [feat]], np.ones((len(idx), 1)))) for k, idx, K in sel])
        K = np.concatenate([K for _, _, K in sel])
        for yi in ys:
            y = np.concatenate([laps[k][0][idx + 1, yi] for k, idx, _ in sel])
            th = np.linalg.solve(M.T @ np.diag(K) @ M, M.T @ np.diag(K) @ y)
            Ml, Kl, yl = M.astype(np.longdouble), K.astype(np.longdouble), y.astype(np.longdouble)
            tl = _solve_ld(Ml.T @ (Kl[:, None] * Ml), Ml.T @ (Kl * yl))
            worst = max(worst, float((np.abs(th - tl) / (1 + np.abs(tl))).max()))
    return worst


def _rel(got, ref):
    return float((np.abs(got - ref) / (1 + np.abs(ref))).max())


CYC = ("S", "M", "L")
PAIRS = ((0, 1), (2, 0), (1, 1), (2, 1), (0, 2), (1, 0))        # trToUse = 2 rows over (S, M, L): mixed classes, one duplicate pair, two rows the same laps in either order


@pytest.fixture(scope="module")
def six(g, laps):
    """The six cars of the B = 6 tests: car b's linearisation trajectory is N + 1 consecutive rows of the golden PID lap from the first start row t >= 37 b at which the
    ORACLE's own float64 arithmetic, on every horizon point and on each of the car's lap sets (its lap of CYC, its pair of PAIRS), is within OWN_TOL = 3e-11 of the
    same fit in longdouble (_own_error).  The local fits are ill-conditioned where a point's nearest stored rows are consecutive samples of a smooth lap (condition up
    to 3e7 on these laps, and the reference itself is then up to 4e-10 off): such a start row cannot carry a 3e-10 comparison with the reference and is passed over.
    The rule looks at the reference alone.  Every test of the six cars, bit for bit or against the oracle, uses these rows."""
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    rows = []
    for b in range(6):
        sets = ((CYC[b % 3],), tuple(CYC[k] for k in sorted(PAIRS[b])))
        for t in range(37 * b, 37 * b + 37):
            if all(_own_error(laps, names, xP[t + i], uP[t + i]) <= OWN_TOL for names in sets for i in range(N)):
                rows.append(t)
                break
        else:
            raise AssertionError("car %d: no start row in [%d, %d) where the oracle carries the comparison" % (b, 37 * b, 37 * b + 37))
    print("start rows of the six cars:", rows)
    return np.stack([xP[t:t + N + 1] for t in rows]), np.stack([uP[t:t + N] for t in rows])


@pytest.mark.parametrize("runtime", [False, True], ids=["fast", "runtime-kernel"])
def test_every_car_equals_a_context_holding_only_its_lap(g, laps, six, runtime):
    """regress_batch, B = 6, trToUse = 1, rows cycling through S, M, L: car b's A, B, C and status are, bit for bit, those of a context holding only that lap, given the
    same batch -- on the built-in route and on the runtime-(N, S) route."""
    B = 6
    xLin, uLin = six
    with _ctx(g, laps, CYC, 1, B, runtime) as ctx:
        assert ctx.solver_kind == (2 if runtime else 0)
        ctx.model_set_lap_table([[b % 3] for b in range(B)])
        got = ctx.regress_batch(xLin, uLin)
    for b in range(B):
        _same(got, _only(g, laps, (CYC[b % 3],), six, runtime), b, "trToUse 1")
    assert not got[3].any()


@pytest.mark.parametrize("runtime", [False, True], ids=["fast", "runtime-kernel"])
def test_two_laps_per_car_and_a_duplicate_pair(g, laps, six, runtime):
    """trToUse = 2, rows PAIRS: against contexts holding exactly those two laps, inserted by ascending insertion index (the duplicate pair: the lap added twice) -- on both routes."""
    B = 6
    xLin, uLin = six
    with _ctx(g, laps, CYC, 2, B, runtime) as ctx:
        ctx.model_set_lap_table(PAIRS)
        got = ctx.regress_batch(xLin, uLin)
    for b, row in enumerate(PAIRS):
        _same(got, _only(g, laps, tuple(CYC[k] for k in sorted(row)), six, runtime), b, "trToUse 2")


@pytest.mark.parametrize("runtime", [False, True], ids=["fast", "runtime-kernel"])
def test_regress_points_one_row_per_point(g, laps, runtime):
    """regress_points, 7 points, trToUse = 1: point e uses row e -- on both routes."""
    n = 7
    xLin, uLin = _batch(g, n)
    x, u = xLin[:, 0], uLin[:, 0]
    with _ctx(g, laps, CYC, 1, 2, runtime) as ctx:        # (max_batch 2: up to 24 points)
        ctx.model_set_lap_table([(e + 1) % 3 for e in range(n)])
        got = ctx.regress_points(x, u)
        with pytest.raises(Exception, match="lap table"):
            ctx.regress_points(x[:5], u[:5])
    for name in CYC:
        with _ctx(g, laps, (name,), 1, 2, runtime) as ctx:
            ref = ctx.regress_points(x, u)
        for e in range(n):
            if CYC[(e + 1) % 3] == name:
                _same(got, ref, e, "points")


@pytest.mark.parametrize("names", [CYC, ("S", "S2")], ids=["mixed-16-rows", "small-8-rows"])
def test_grid_larger_than_the_cu_count(g, laps, names):
    """B = 300 > the CU count: the occupancy build of the table kernel runs (one work-group per car and more work-groups than CUs), with the 16-rows-per-lane scan for
    the mixed table and the 8-rows-per-lane scan for the table of 400-row laps.  Same comparison."""
    B = 300
    xLin, uLin = _batch(g, B)
    with _ctx(g, laps, names, 1, B) as ctx:
        ctx.model_set_lap_table([[b % len(names)] for b in range(B)])
        got = ctx.regress_batch(xLin, uLin)
    for k, name in enumerate(names):
        ref = _only(g, laps, (name,), (xLin, uLin))
        for b in range(k, B, len(names)):
            _same(got, ref, b, "B = 300")


def test_caller_order_one_row_and_switching_back(g, laps, six):
    """The caller's order inside a row does not change the bits; n = 1 equals the n = B table of identical rows (and, a 400-row lap alone, runs the 8-rows-per-lane
    table build below the CU count); after set(0) the results are those of the untouched context."""
    B = 6
    xLin, uLin = six
    with _ctx(g, laps, CYC, 2, B) as ctx:
        untouched = ctx.regress_batch(xLin, uLin)
        ctx.model_set_lap_table(PAIRS)
        a = ctx.regress_batch(xLin, uLin)
        ctx.model_set_lap_table([row[::-1] for row in PAIRS])
        b = ctx.regress_batch(xLin, uLin)
        ctx.model_set_lap_table([[2, 0]])
        one = ctx.regress_batch(xLin, uLin)
        ctx.model_set_lap_table([[0, 2]] * B)
        many = ctx.regress_batch(xLin, uLin)
        ctx.model_set_lap_table(None)
        assert ctx.model_lap_table().shape == (0, 2)
        back = ctx.regress_batch(xLin, uLin)
    for k in range(4):
        assert np.array_equal(a[k], b[k]) and np.array_equal(one[k], many[k]) and np.array_equal(back[k], untouched[k]), k
    assert not np.array_equal(a[0], untouched[0])
    ref = _only(g, laps, ("S", "M"), six)                   # the untouched context: the first two laps of the sorted order
    for car in range(B):
        _same(untouched, ref, car, "default")
    with _ctx(g, laps, CYC, 1, B) as ctx:
        ctx.model_set_lap_table([[0]])
        small = ctx.regress_batch(xLin, uLin)
    for car in range(B):
        _same(small, _only(g, laps, ("S",), six), car, "one small row")


def test_table_survives_store_growth_lap_replacement_and_a_checkpoint(g, laps, six, tmp_path):
    """Table set, then a lap longer than max_lap_len is added (the stores are reallocated with another row stride) and a lap no row names is replaced: same bits, same
    table.  save_stores / restore_stores carry the table: the restored context, whose laps are numbered anew, gives the same bits."""
    B = 6
    xLin, uLin = six
    rows = [[(b % 3, 2 - b % 3)[b // 3]] for b in range(B)]                           # S M L L M S
    with _ctx(g, laps, ("S", "M", "L", "E"), 1, B, max_lap_len=1400, max_laps=4) as ctx:
        ctx.model_set_lap_table(rows)
        before = ctx.regress_batch(xLin, uLin)
        ctx.model_add_trajectory(*laps["XL"])                                         # 1500 rows > 1400, a fifth lap > max_laps
        grown = ctx.regress_batch(xLin, uLin)
        ctx.model_replace_lap(1, *laps["E2"])                                         # sorted order S E M L XL: position 1 is E
        replaced = ctx.regress_batch(xLin, uLin)
        assert ctx.model_lap_table().tolist() == rows
        ctx.save_stores(str(tmp_path / "stores"))
    with _ctx(g, laps, (), 1, B) as ctx:
        ctx.restore_stores(str(tmp_path / "stores"))
        assert ctx.model_lap_table().tolist() == [[{0: 0, 1: 2, 2: 3}[r[0]]] for r in rows]      # sorted order S E M L XL
        restored = ctx.regress_batch(xLin, uLin)
    for k in range(4):
        assert np.array_equal(before[k], grown[k]) and np.array_equal(before[k], replaced[k]) and np.array_equal(before[k], restored[k]), k
    for b in range(B):
        _same(before, _only(g, laps, (CYC[rows[b][0]],), six), b, "before the store changes")


def _host_stepped(ctx, x0, xLin0, uLin0, noise):
    """step_batch + plant_step_batch per step and the tail of MPC.solve (:129-137) in NumPy, as tests/test_gpu_mpc_stages.py steps its LTV sessions."""
    B = x0.shape[0]
    x = x0.copy(); xg = x0.copy(); uOld = np.zeros((B, 2)); xLin, uLin = xLin0.copy(), uLin0.copy()
    X, U, G = [], [], []
    for t in range(noise.shape[0]):
        out = ctx.step_batch(x, xLin, uLin, uOld)
        assert np.all((out["status"] & ~64) == 0), (t, out["status"])
        u = out["uPred"][:, 0].copy()
        X.append(x.copy()); U.append(u); G.append(xg.copy())
        x, xg, _ = ctx.plant_step_batch(x, xg, u, noise[t])
        xLin = np.concatenate([out["xPred"][:, 1:], out["xPred"][:, N:N + 1]], axis=1)
        uLin = np.concatenate([out["uPred"][:, 1:], out["uPred"][:, N - 1:N]], axis=1)
        uOld = u
    return np.stack(X), np.stack(U), np.stack(G)


def _session(ctx, x0, xLin0, uLin0, noise, between=None):
    T = noise.shape[0]
    ctx.rollout_begin_mpc(x0, x0, noise, xLin0=xLin0, uLin0=uLin0)
    t, _ = ctx.rollout_run(10)
    assert t == 10
    if between is not None:
        between()
    t, _ = ctx.rollout_run(T)
    X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
    ctx.rollout_end()
    assert t == T and np.all((st & ~64) == 0), (t, st)
    return X, U, G


def test_step_batch_and_an_ltv_session_follow_the_table(g, laps):
    """B = 6, 30 steps, noise given, rows cycling through S, M, L.  Car b's xPred / uPred of step_batch and its X, U, Xglob logs of a rollout_begin_mpc session equal those
    of the same 6-car call on a context holding only car b's lap (same B, same route).  The session equals the host-stepped loop over step_batch + plant_step_batch
    with the table set, and a table set after 10 of its steps does not reach it: the next session uses that one."""
    B, T = 6, 30
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    t0 = 160                                              # a row every lap of the table has neighbours of: the cars start at speed, a little off the recorded line
    x0 = np.tile(xP[t0], (B, 1)); x0[:, 5] += np.linspace(-0.05, 0.05, B); x0[:, 0] += 0.01 * np.arange(B)
    xLin0 = np.tile(xP[None, t0:t0 + N + 1], (B, 1, 1)); uLin0 = np.tile(uP[None, t0:t0 + N], (B, 1, 1))
    noise = np.random.default_rng(31).standard_normal((T, B, 3))
    rows = [[b % 3] for b in range(B)]
    with _ctx(g, laps, CYC, 1, B) as ctx:
        ctx.model_set_lap_table(rows)
        step = ctx.step_batch(x0, xLin0, uLin0, np.zeros((B, 2)))
        X, U, G = _session(ctx, x0, xLin0, uLin0, noise, between=lambda: ctx.model_set_lap_table([[2]]))
        assert ctx.model_lap_table().tolist() == [[2]]
        X2, U2, G2 = _session(ctx, x0, xLin0, uLin0, noise)                           # the table set meanwhile: every car on L
        ctx.model_set_lap_table(rows)
        Xh, Uh, Gh = _host_stepped(ctx, x0, xLin0, uLin0, noise)
    assert np.array_equal(X, Xh) and np.array_equal(U, Uh) and np.array_equal(G, Gh)
    differ = False
    for k, name in enumerate(CYC):
        with _ctx(g, laps, (name,), 1, B) as ctx:
            rstep = ctx.step_batch(x0, xLin0, uLin0, np.zeros((B, 2)))
            Xr, Ur, Gr = _session(ctx, x0, xLin0, uLin0, noise)
        for b in range(k, B, 3):
            for key in ("xPred", "uPred", "A", "B", "C", "status"):
                assert np.array_equal(step[key][b], rstep[key][b]), (key, b)
            assert np.array_equal(X[:, b], Xr[:, b]) and np.array_equal(U[:, b], Ur[:, b]) and np.array_equal(G[:, b], Gr[:, b]), b
        if name == "L":
            assert np.array_equal(X2, Xr) and np.array_equal(U2, Ur) and np.array_equal(G2, Gr)
        else:
            differ = differ or not np.array_equal(U[:, k], U2[:, k])
    assert differ                                          # (the laps do give different models: the comparison above is not vacuous)


def test_a_session_begun_without_a_table_keeps_the_default_laps(g, laps):
    """A session that began with no table reads the context-wide default -- here S, the first lap of the sorted order -- to its end: a table set after 10 of its 30 steps
    changes none of its logs (the header: a later set reaches the next session only), and the session begun afterwards uses the table."""
    B, T = 6, 30
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    t0 = 160
    x0 = np.tile(xP[t0], (B, 1)); x0[:, 5] += np.linspace(-0.05, 0.05, B); x0[:, 0] += 0.01 * np.arange(B)
    xLin0 = np.tile(xP[None, t0:t0 + N + 1], (B, 1, 1)); uLin0 = np.tile(uP[None, t0:t0 + N], (B, 1, 1))
    noise = np.random.default_rng(32).standard_normal((T, B, 3))
    with _ctx(g, laps, CYC, 1, B) as ctx:
        plain = _session(ctx, x0, xLin0, uLin0, noise)
        during = _session(ctx, x0, xLin0, uLin0, noise, between=lambda: ctx.model_set_lap_table([[2]]))
        after = _session(ctx, x0, xLin0, uLin0, noise)
    with _ctx(g, laps, ("L",), 1, B) as ctx:
        on_l = _session(ctx, x0, xLin0, uLin0, noise)
    for k in range(3):
        assert np.array_equal(plain[k], during[k]) and np.array_equal(after[k], on_l[k]), k
    assert not np.array_equal(plain[1], after[1])


def test_the_fused_step_is_not_taken_with_a_table(g, laps, monkeypatch):
    """LMPC_FUSE=1 and a batch that runs one wave per QP (B = 1100 at N = 12), where the fused one-wave step would otherwise run the regression on the laps of the
    parameter block: with a table in force the two-kernel step runs, so step_batch returns the bits of a context created without the knob -- A, B, C and the solution
    of every car, two thirds of which are on another lap than the block's."""
    B = 1100
    xLin, uLin = _batch(g, B)
    x0 = xLin[:, 0].copy(); uOld = np.zeros((B, 2))
    rows = [[b % 3] for b in range(B)]
    out = {}
    for fuse in (False, True):
        if fuse:
            monkeypatch.setenv("LMPC_FUSE", "1")
        else:
            monkeypatch.delenv("LMPC_FUSE", raising=False)
        with _ctx(g, laps, CYC, 1, B) as ctx:
            assert ctx.solver_waves(B) == 1
            ctx.model_set_lap_table(rows)
            out[fuse] = ctx.step_batch(x0, xLin, uLin, uOld)
    for key in ("A", "B", "C", "xPred", "uPred", "status", "iters"):
        assert np.array_equal(out[False][key], out[True][key]), key
    ref = _only(g, laps, ("M",), (xLin, uLin))
    assert all(np.array_equal(out[True]["A"][b], ref[0][b]) for b in range(1, B, 3))


def test_batch_size_against_the_rows_and_the_librarys_argument_checks(g, laps, six):
    """A call whose B is not the table's row count is LMPC_E_ARG at that call -- regress_batch, step_batch, the LTV session -- and the context stays usable.  The library's
    own checks: an index out of range at either end, n < 0 and NULL with n > 0 are LMPC_E_ARG and leave the table in force; get returns what set stored, min(n, capacity)
    rows of it; n = 0 restores the default."""
    from racinglmpc_amd import _capi
    B = 6
    xLin, uLin = six
    rows = np.array([[b % 3] for b in range(B)], np.int32)
    with _ctx(g, laps, CYC, 1, B) as ctx:
        lib, h = ctx.lib, ctx._h
        ctx.model_set_lap_table(rows)
        want = ctx.regress_batch(xLin, uLin)
        for call in (lambda: ctx.regress_batch(xLin[:4], uLin[:4]), lambda: ctx.step_batch(xLin[:4, 0], xLin[:4], uLin[:4], np.zeros((4, 2))),
                     lambda: ctx.rollout_begin_mpc(xLin[:4, 0], xLin[:4, 0], np.zeros((5, 4, 3)), xLin0=xLin[:4], uLin0=uLin[:4])):
            with pytest.raises(_capi.LmpcError, match=r"error -1: lap table: B = 4 problems but lmpc_model_set_lap_table holds 6 rows"):
                call()
        again = ctx.regress_batch(xLin, uLin)
        assert all(np.array_equal(p, q) for p, q in zip(want, again))
        n = C.c_int(-5)
        for bad_n, bad in ((1, np.array([3], np.int32)), (2, np.array([0, -1], np.int32)), (-1, rows), (1, None)):
            assert lib.lmpc_model_set_lap_table(h, bad_n, None if bad is None else bad.ctypes.data) == -1, (bad_n, bad)
            assert np.array_equal(ctx.model_lap_table(), rows)
        assert lib.lmpc_model_get_lap_table(h, None, None, 0) == -1 and lib.lmpc_model_get_lap_table(h, C.byref(n), None, -1) == -1
        part = np.full((4, 1), -7, np.int32)
        assert lib.lmpc_model_get_lap_table(h, C.byref(n), part.ctypes.data, 2) == 0 and n.value == B and part.ravel().tolist() == [0, 1, -7, -7]
        assert lib.lmpc_model_set_lap_table(h, 0, None) == 0
        assert lib.lmpc_model_get_lap_table(h, C.byref(n), None, 0) == 0 and n.value == 0
        default = ctx.regress_batch(xLin[:4], uLin[:4])                               # any B again
    ref = _only(g, laps, ("S",), six)
    for b in range(4):
        for k in range(4):
            assert np.array_equal(default[k][b], ref[k][b]), (k, b)


def test_against_the_oracle_and_a_singular_lap_on_one_car_only(g, laps, six):
    """Every car of the B = 6 cases above (one lap per car, two laps per car, points): A, B, C within 3e-10 relative of the oracle given only that car's lap(s) -- the
    bound tests/test_gpu_mpc_stages.py uses for the shared store -- and equal status words.  Every horizon point of every car is judged; the cars' rows are those
    of the fixture `six`.  (The first choice of rows, 37 b for car b without looking at the oracle's conditioning, gave 5.09e-10 on an MI355X at one point of car 5 on
    L, where the oracle's own float64 arithmetic is 4.29e-10 off its longdouble self; 4.66e-11 everywhere the oracle is within 3e-11.)  With an all-zero lap on car 3 that car alone carries LMPC_ST_REG_SINGULAR
    (the oracle's solve raises there), on every horizon point; the other cars stay bit-identical to the batch without that lap."""
    from racinglmpc_amd import _capi
    B = 6
    xLin, uLin = six
    worst = 0.0
    with _ctx(g, laps, CYC + ("Z",), 1, B) as ctx:
        ctx.model_set_lap_table([[b % 3] for b in range(B)])
        clean = ctx.regress_batch(xLin, uLin)
        ctx.model_set_lap_table([[0], [1], [2], [3], [1], [2]])
        withz = ctx.regress_batch(xLin, uLin)
        pts = ctx.regress_points(xLin[:, 0], uLin[:, 0])
    with _ctx(g, laps, CYC, 2, B) as ctx:
        ctx.model_set_lap_table(PAIRS)
        two = ctx.regress_batch(xLin, uLin)
    for b in range(B):
        mine = ("Z",) if b == 3 else (CYC[b % 3],)
        for got, names in ((clean, (CYC[b % 3],)), (withz, mine), (two, tuple(CYC[k] for k in sorted(PAIRS[b])))):
            A, Bm, Cc, st = _oracle(g, laps, names, xLin[b], uLin[b])
            assert np.array_equal(got[3][b], st), (b, names, got[3][b], st)
            if not st.any():
                e = np.array([max(_rel(got[0][b][i], A[i]), _rel(got[1][b][i], Bm[i]), _rel(got[2][b][i], Cc[i])) for i in range(N)])
                own = max(_own_error(laps, names, xLin[b, i], uLin[b, i]) for i in range(N))
                print("car %d on %s: worst relative error over its %d points %.2e (the oracle's own float64 error there: up to %.2e)" % (b, "+".join(names), N, e.max(), own))
                assert own <= OWN_TOL                                  # (the rule of the fixture `six`)
                worst = max(worst, e.max())
        A, Bm, Cc, st = _oracle(g, laps, mine, xLin[b, :1], uLin[b, :1], n=1)
        assert pts[3][b] == st[0]
        if not st.any():
            worst = max(worst, _rel(pts[0][b], A[0]), _rel(pts[1][b], Bm[0]), _rel(pts[2][b], Cc[0]))
        if b != 3:
            _same(withz, clean, b, "beside the singular car")
    print("lap table against the oracle: worst relative |A, B, C - oracle| %.2e over %d cars x 3 cases x %d points + points" % (worst, B, N))
    assert np.all(withz[3][3] == _capi.ST_REG_SINGULAR) and not clean[3].any() and not two[3].any()
    assert worst < 3e-10


def test_bootstrap_per_car_store_end_to_end(g):
    """rollout.bootstrap(B = 8, per_car_store=True) with four nominal cars and four at +-20 % mass and grip, 450 steps per stage (past every crossing): every car finishes
    every stage with no status bit other than INEXACT, store_laps lists all eight cars, and car b's first LTV step -- the regression of the first N + 1 rows of its own
    PID lap on that lap alone -- has A, B, C within 3e-10 relative of the oracle on that lap."""
    from racinglmpc_amd import _capi, rollout
    B, T = 8, 450
    sc = np.array([[1, 1]] * 4 + [[0.8, 0.8], [0.8, 1.2], [1.2, 0.8], [1.2, 1.2]], float)
    par = _capi.plant_params(B, m=1.98 * sc[:, 0], mu_f=0.8 * sc[:, 1], mu_r=0.8 * sc[:, 1])
    out = rollout.bootstrap(g["track"], B, N, 0.8, 9, max_steps=T, plant_params=par, per_car_store=True)
    assert out["store_laps"] == list(range(B)) and np.all(out["lti_status"] == 0)
    for k in ("pid", "mpc", "ltvmpc"):
        done = np.array([l[4] for l in out[k]]); st = np.array([l[5] for l in out[k]])
        print("per-car bootstrap %s: done_at %s status %s" % (k, done.tolist(), st.tolist()))
        assert len(out[k]) == B and np.all(done > 0) and np.all((st & ~_capi.ST_INEXACT) == 0), k
    xLin = np.stack([l[0][0:N + 1] for l in out["pid"]]); uLin = np.stack([l[1][0:N] for l in out["pid"]])
    with _capi.Context(rollout.mpc_stage_config(g["track"], N, 0.8, B, trToUse=1)) as ctx:
        for l in out["pid"]:
            ctx.model_add_trajectory(l[0], l[1])
        ctx.model_set_lap_table(np.arange(B).reshape(B, 1))
        A, Bm, Cc, st = ctx.regress_batch(xLin, uLin)
    assert not st.any()
    worst = 0.0
    lapd = {b: (out["pid"][b][0], out["pid"][b][1]) for b in range(B)}
    for b in range(B):
        Ao, Bo, Co, so = _oracle(g, lapd, (b,), xLin[b], uLin[b])
        assert not so.any()
        worst = max(worst, _rel(A[b], Ao), _rel(Bm[b], Bo), _rel(Cc[b], Co))
    print("per-car bootstrap: first LTV step against the oracle on each car's own PID lap: worst relative %.2e" % worst)
    assert worst < 3e-10
    assert not np.array_equal(A[0], A[4])                  # (another vehicle, another model)
