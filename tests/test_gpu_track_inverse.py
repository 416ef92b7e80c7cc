"""-m gpu: the inverse track map on the device -- lmpc_local_position_batch, lmpc_track_angle_batch, lmpc_state_from_global_batch (csrc/lmpc_track.hip.h) -- against
what the executed reference returned (tests/golden/local_position/track_local.npz: Map.getLocalPosition, Track.py:191-290; Map.getAngle, Track.py:312-349), through every launch shape,
round the device's own forward map, on the two logged frames of a PID session, and from rollout.seed_lmpc(from_global=True) into running LMPC rollouts.

Bounds.  A bound named MEASURED_* is the worst difference this file measured on an MI355X; the assertion allows ten times that and never more than CAP = 1e-9 (ocml's
atan2, sin and cos differ from NumPy's by a few ulp on values up to about 20 m).  Every test prints what it finds before it asserts."""
import numpy as np
import pytest

from tests import common
from tests import track_ref
from tests.test_track_inverse_host import fixture, fixture_rows

pytestmark = pytest.mark.gpu

CAP = 1e-9
X0 = np.array([0.5, 0, 0, 0, 0, 0.0])
# worst |device - fixture| over all 20054 getLocalPosition rows (s, ey, epsi) and the 600 getAngle rows (psi), measured on an MI355X.  psi: getAngle has no
# transcendental function in it and the kernel rounds every product and sum on its own, so the device returns NumPy's bits -- ten times nothing is nothing
MEASURED_PARITY = dict(s=1.776e-15, ey=4.441e-16, epsi=2.220e-15, psi=0.0)
# worst |local_position(global_position(s, ey), track_angle(s, epsi)) - (s, ey, epsi)| over the 3998 interior points, the device alone
MEASURED_ROUND_TRIP = dict(s=1.776e-15, ey=7.772e-16, epsi=2.331e-15)
# worst |xPred(seeded from the inertial frame) - xPred(seeded with the curvilinear laps)| of the first LMPC step
MEASURED_XPRED = 5.453e-13


def bound(measured):
    """Ten times the measured worst, never above CAP."""
    return min(10.0 * measured, CAP)


@pytest.fixture(scope="module")
def t(built):
    return fixture()


@pytest.fixture(scope="module")
def rows(t):
    return fixture_rows(t)


@pytest.fixture(scope="module")
def ctx(t):
    from racinglmpc_amd import _capi
    cfg, _ = common.mpc_config(t, 12, max_batch=64)
    c = _capi.Context(cfg)
    yield c
    c.close()


@pytest.fixture(scope="module")
def full(ctx, t, rows):
    """Every getLocalPosition row of the fixture in ONE call (n = 20054: not a multiple of 256) and every getAngle row in one: computed once, shared, left unchanged."""
    x, y, psi = rows[:3]
    out = ctx.local_position(x, y, psi, float(t["max_ey"])) + ctx.track_angle(t["e_s"], t["e_epsi"])
    for a in out:
        a.setflags(write=False)
    return out


def test_reference_parity(t, rows, full):
    """All fixture rows, no leave-out list: status exact (0 where the reference completes, LMPC_ST_NO_SEGMENT with 10000 three times where it does not), s, ey, epsi and
    psi within ten times the measured worst difference (MEASURED_PARITY), capped at 1e-9.  Measured on an MI355X: s 1.776e-15, ey 4.441e-16, epsi 2.220e-15 (the
    worst rows are interior points and their shifted-heading copies; the end-point and off-track rows return the reference's bits), psi 0."""
    from racinglmpc_amd import _capi
    x, y, psi, want, ok, row, group = rows
    s, ey, epsi, st, ang, ast = full
    assert x.shape[0] % 256 != 0
    assert np.array_equal(st, np.where(ok == 1, 0, _capi.ST_NO_SEGMENT).astype(np.int32))
    off = ok == 0
    assert np.all(s[off] == 10000.0) and np.all(ey[off] == 10000.0) and np.all(epsi[off] == 10000.0)
    worst = dict(s=np.abs(s - want[:, 0]).max(), ey=np.abs(ey - want[:, 1]).max(), epsi=np.abs(epsi - want[:, 2]).max(), psi=np.abs(ang - t["e_psi"]).max())
    for grp, name in enumerate("abcd"):
        m = group == grp
        print("(%s) %5d rows: worst |device - reference| s %.3e ey %.3e epsi %.3e" % (name, m.sum(), np.abs(s - want[:, 0])[m].max(), np.abs(ey - want[:, 1])[m].max(),
                                                                                    np.abs(epsi - want[:, 2])[m].max()))
    print("parity, all rows:", {k: "%.3e" % v for k, v in worst.items()})
    assert np.all(ast == 0)
    assert np.all(ey[group == 1] == 0.0)                                                   # the equality branches: ey is the literal 0
    for k, v in worst.items():
        assert v <= bound(MEASURED_PARITY[k]), (k, v)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_launch_shapes(ctx, t, rows, full, n):
    """A call with n points returns the bits of the same rows inside the full call -- the rows start at 3990, so they run over interior, end-point and off-track rows
    and both kinds of status --, for the three entry points (lmpc_state_from_global_batch as (n, 1, 6) and, where n = T B allows, as (T, B, 6))."""
    x, y, psi = rows[:3]
    o = 3990
    s, ey, epsi, st = ctx.local_position(x[o:o + n], y[o:o + n], psi[o:o + n], float(t["max_ey"]))
    for got, ref in zip((s, ey, epsi, st), full[:4]):
        assert np.array_equal(got, ref[o:o + n])
    ang, ast = ctx.track_angle(t["e_s"][5:5 + n], t["e_epsi"][5:5 + n])
    assert np.array_equal(ang, full[4][5:5 + n]) and np.array_equal(ast, full[5][5:5 + n])
    v = np.arange(3.0 * n).reshape(n, 3) + 0.25
    xg = np.concatenate([v, psi[o:o + n, None], x[o:o + n, None], y[o:o + n, None]], axis=1)
    shapes = [(n, 1)] + ([(n // 5, 5)] if n % 5 == 0 else []) + ([(1, n)] if n > 1 else [])
    for T, B in shapes:
        xs, sst = ctx.state_from_global(xg.reshape(T, B, 6), float(t["max_ey"]))
        xs = xs.reshape(n, 6)
        assert np.array_equal(xs[:, :3], v) and np.array_equal(sst.reshape(n), full[3][o:o + n])
        assert np.array_equal(xs[:, 3], full[2][o:o + n]) and np.array_equal(xs[:, 4], full[0][o:o + n]) and np.array_equal(xs[:, 5], full[1][o:o + n])


def test_round_trip_through_the_device_alone(ctx, t):
    """(s, ey, epsi) of the interior points -> lmpc_global_position_batch and lmpc_track_angle_batch -> lmpc_local_position_batch: back at the inputs within ten times
    the measured worst (MEASURED_ROUND_TRIP), capped at 1e-9; every row completes.  Measured on an MI355X: s 1.776e-15, ey 7.772e-16, epsi 2.331e-15."""
    xy, st0 = ctx.global_position_batch(t["a_s"], t["a_ey"])
    psi, st1 = ctx.track_angle(t["a_s"], t["a_epsi"])
    s, ey, epsi, st = ctx.local_position(xy[:, 0], xy[:, 1], psi, float(t["max_ey"]))
    assert not st0.any() and not st1.any() and not st.any()
    worst = dict(s=np.abs(s - t["a_s"]).max(), ey=np.abs(ey - t["a_ey"]).max(), epsi=np.abs(epsi - t["a_epsi"]).max())
    print("round trip on the device:", {k: "%.3e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= bound(MEASURED_ROUND_TRIP[k]), (k, v)


def _pid_u(x, vt, nu):
    return np.stack([-0.6 * x[:, 5] - 0.9 * x[:, 3] + np.clip(nu[:, 0] * 0.25, -0.9, 0.9), 1.5 * (vt - x[:, 0]) + np.clip(nu[:, 1] * 0.10, -0.2, 0.2)], axis=1)


def _frame_gap(x, conv, TL):
    """max |conv - x| per column (epsi, s on the circle of length TL, ey)."""
    ds = np.abs(np.mod(conv[..., 4], TL) - np.mod(x[..., 4], TL)); ds = np.minimum(ds, TL - ds)
    return np.array([np.abs(conv[..., 3] - x[..., 3]).max(), ds.max(), np.abs(conv[..., 5] - x[..., 5]).max()])


def test_rollout_self_consistency(ctx, t):
    """A 48-car, 120-step PID session (lmpc_rollout_pid, host noise given) logs X and Xglob, which plant_step_duo integrates independently (100 Euler sub-steps each, of
    different equations): lmpc_state_from_global_batch(Xglob) agrees with X in epsi, s mod TrackLength and ey up to the gap between the two integrations, which is a
    property of the plant.  That gap is measured on the CPU for the same draws (tests/plant_ref.py in extended precision, the control law in NumPy, tests/track_ref.py
    for the conversion); the device's gap may be at most twice it, per column.  vx, vy, wz are Xglob's, bit for bit; every status is 0.  Measured on an MI355X:
    the gap is (epsi, s, ey) = (2.177e-3, 3.490e-3, 2.968e-3) on the device and on the CPU alike; the two sessions differ by 7.3e-14."""
    from tests import plant_ref
    B, T = 48, 120
    pt = np.array(t["track"]); TL = float(t["trackLength"]); max_ey = float(t["max_ey"])
    rng = np.random.default_rng(31)
    vt = 0.6 + 0.01 * np.arange(B)
    nu = rng.standard_normal((T, B, 2)); nz = rng.standard_normal((T, B, 3))
    x0 = np.tile(X0, (B, 1))
    n, _ = ctx.rollout_pid(x0, x0, vt, nu, nz)
    X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, n)
    ctx.rollout_end()
    assert n == T and not st.any()
    conv, cst = ctx.state_from_global(G, max_ey)
    assert conv.shape == (T, B, 6) and cst.shape == (T, B) and not cst.any()
    assert np.array_equal(conv[..., :3], G[..., :3])
    gap_dev = _frame_gap(X, conv, TL)
    # the same session on the CPU
    x = x0.copy(); xg = x0.copy(); Xc, Gc = [], []
    for k in range(T):
        u = _pid_u(x, vt, nu[k])
        Xc.append(x); Gc.append(xg)
        xn, xgn, raised, _ = plant_ref.dyn_model_ld(pt, x, xg, u, nz[k])
        assert not raised.any()
        x = np.asarray(xn, np.float64); xg = np.asarray(xgn, np.float64)
    Xc = np.stack(Xc); Gc = np.stack(Gc)
    cconv, ccst = track_ref.state_from_global(pt, Gc, max_ey)
    assert not ccst.any()
    gap_cpu = _frame_gap(Xc, cconv, TL)
    print("gap between the two logged frames (epsi, s, ey): device %s, CPU %s; device session against CPU session %.3e" % (gap_dev, gap_cpu, np.abs(X - Xc).max()))
    assert np.all(gap_cpu > 0) and np.all(gap_dev <= 2.0 * gap_cpu), (gap_dev, gap_cpu)


def test_seed_from_global_end_to_end(t):
    """One 4-car PID session of 1000 steps; car 0's lap seeds three N = 12 LMPC contexts (four copies of the lap each, as main.py:102-110 seeds with its PID lap):
      A  seed_lmpc(ctx, [(x_glob, u)] * 4, from_global=True, max_ey=0.85) with the session's own logged Xglob -- the use the entry point exists for;
      B  seed_lmpc(ctx, [(x, u)] * 4) with the logged curvilinear lap;
      C  from_global again, with x_glob made from B's lap by the device's forward map (global_position_batch, track_angle): the lap B holds, seen from the inertial frame.
    Each then runs 20 steps of lmpc_rollout_begin / run for 4 cars: every status word is 0.  xPred of the first step of C matches B's within ten times the measured
    worst (MEASURED_XPRED), capped at 1e-9; measured on an MI355X: 5.453e-13 (A against B: 8e-2).  (A is not compared with B: its velocities are Xglob's, which carry no plant noise, and its positions differ from B's by
    the gap of test_rollout_self_consistency.)"""
    from racinglmpc_amd import _capi, rollout
    N, B, T, steps = 12, 4, 1000, 20
    TL = float(t["trackLength"])
    cfg, _ = common.lmpc_config(t, N, max_batch=B)
    rng = np.random.default_rng(41)
    x0 = np.tile(X0, (B, 1))
    ctxs = [_capi.Context(cfg) for _ in range(3)]
    try:
        n, _ = ctxs[0].rollout_pid(x0, x0, np.full(B, 0.8), rng.standard_normal((T, B, 2)), rng.standard_normal((T, B, 3)))
        X, U, G, done, st, _, _ = ctxs[0].rollout_fetch(0, n)
        ctxs[0].rollout_end()
        assert n == T and not st.any() and done[0] > 0
        x, u, xg = X[:, 0].copy(), U[:, 0].copy(), G[:, 0].copy()
        assert x[-1, 4] > 2 * TL                                                       # a multi-lap PID lap: s runs past TrackLength
        xy, s0 = ctxs[2].global_position_batch(x[:, 4], x[:, 5]); psi, s1 = ctxs[2].track_angle(x[:, 4], x[:, 3])
        assert not s0.any() and not s1.any()
        xg_c = np.concatenate([x[:, :3], psi[:, None], xy], axis=1)
        rollout.seed_lmpc(ctxs[0], [(xg, u)] * 4, from_global=True, max_ey=0.85)
        rollout.seed_lmpc(ctxs[1], [(x, u)] * 4)
        rollout.seed_lmpc(ctxs[2], [(xg_c, u)] * 4, from_global=True, max_ey=0.85)
        back = rollout.lap_from_global(ctxs[2], xg_c, 0.85)
        print("lap_from_global of the forward-mapped lap: worst |x - lap| per column", np.abs(back - x).max(axis=0))
        assert np.all(np.diff(back[:, 4]) > 0) and np.abs(back - x).max() <= CAP
        start = np.tile(X0, (B, 1)); start[:, 5] = np.linspace(-0.03, 0.03, B)
        noise = rng.standard_normal((steps, B, 3))
        xpred = []
        for c in ctxs:
            assert c.ss_num_laps() == 4
            c.rollout_begin(start, start, np.tile(x[None, 1:N + 2], (B, 1, 1)), np.tile(u[None, 1:N + 1], (B, 1, 1)), noise)
            c.rollout_run(1)
            xpred.append(c.debug_rollout_qp(0, B, selection=False)["xPred"].copy())
            n, _ = c.rollout_run(steps - 1)
            out = c.rollout_fetch(0, n)
            c.rollout_end()
            assert n == steps and not out[4].any(), out[4]
        d = np.abs(xpred[2] - xpred[1]).max()
        print("first step: worst |xPred(from the inertial frame) - xPred(curvilinear laps)| %.3e; against the session's own Xglob %.3e" % (d, np.abs(xpred[0] - xpred[1]).max()))
        assert d <= bound(MEASURED_XPRED), d
    finally:
        for c in ctxs:
            c.close()


def test_failing_inputs_and_argument_checks(ctx, t, rows):
    """Ordinary status paths: NaN / inf in any input give LMPC_ST_NO_SEGMENT and 10000 three times while the neighbours in the batch are untouched; max_ey = 0 completes
    only centre-line and end-point rows; s on no row gives psi = 0 with the status; the argument checks return LMPC_E_ARG and leave the context usable."""
    from racinglmpc_amd import _capi
    x, y, psi, want, ok, row, group = rows
    max_ey = float(t["max_ey"]); TL = float(t["trackLength"]); lib, h = ctx.lib, ctx._h
    xs, ys, ps = x[:8].copy(), y[:8].copy(), psi[:8].copy()
    xs[1] = np.nan; ys[3] = np.inf; ps[5] = -np.inf; ps[6] = np.nan
    s, ey, epsi, st = ctx.local_position(xs, ys, ps, max_ey)
    bad = np.array([0, 1, 0, 1, 0, 1, 1, 0], bool)
    assert np.array_equal(st, np.where(bad, _capi.ST_NO_SEGMENT, 0)) and np.all(s[bad] == 10000.0) and np.all(ey[bad] == 10000.0) and np.all(epsi[bad] == 10000.0)
    s8, ey8, epsi8, _ = ctx.local_position(x[:8], y[:8], psi[:8], max_ey)
    assert np.array_equal(s[~bad], s8[~bad]) and np.array_equal(ey[~bad], ey8[~bad]) and np.array_equal(epsi[~bad], epsi8[~bad])
    # max_ey = 0: 300 interior rows (off the centre line), the end-point rows, and the same interior rows put ON the centre line of the first straight
    m = np.concatenate([np.nonzero(group == 0)[0][:300], np.nonzero(group == 1)[0]])
    cx = np.linspace(0.05, 0.95, 19)
    s, ey, epsi, st = ctx.local_position(np.concatenate([x[m], cx]), np.concatenate([y[m], np.zeros(19)]), np.concatenate([psi[m], np.full(19, 0.1)]), 0.0)
    assert np.all(st[:300] == _capi.ST_NO_SEGMENT) and np.all(s[:300] == 10000.0) and not st[300:].any()
    assert np.array_equal(s[-19:], cx) and not ey[300:].any() and np.array_equal(epsi[-19:], np.full(19, 0.1))
    ang, ast = ctx.track_angle(np.array([2 * TL, np.nan, np.inf, -0.5, 1.0]), np.full(5, 0.1))
    assert np.array_equal(ast, [4, 4, 4, 4, 0]) and not ang[:4].any() and ang[4] == track_ref.track_angle(t["track"], 1.0, 0.1)[0]
    # argument checks
    a = np.zeros(4); o = np.zeros(24); sti = np.zeros(4, np.int32); p, q, si = a.ctypes.data, o.ctypes.data, sti.ctypes.data
    for n_, xp, me in ((0, p, 0.85), (-3, p, 0.85), (4, None, 0.85), (4, p, -0.1), (4, p, np.nan), (4, p, np.inf)):
        assert lib.lmpc_local_position_batch(h, n_, xp, p, p, me, q, q + 32, q + 64, si) == -1, (n_, xp, me)
    assert lib.lmpc_local_position_batch(h, 4, p, p, p, 0.85, q, q + 32, None, si) == -1 and lib.lmpc_local_position_batch(h, 4, p, p, p, 0.85, q, q + 32, q + 64, None) == -1
    assert lib.lmpc_track_angle_batch(h, 0, p, p, q, si) == -1 and lib.lmpc_track_angle_batch(h, 4, p, None, q, si) == -1 and lib.lmpc_track_angle_batch(h, 4, p, p, None, si) == -1
    for T_, B_, gp, me in ((0, 1, q, 0.85), (1, 0, q, 0.85), (1, 1, None, 0.85), (1, 1, q, -1.0), (1, 1, q, np.nan)):
        assert lib.lmpc_state_from_global_batch(h, T_, B_, gp, me, q, si) == -1, (T_, B_, gp, me)
    assert "argument check" in lib.lmpc_last_error().decode()
    # a HIP failure reported by an earlier entry point (an allocation that cannot fit) is consumed there: it does not come back as this launch's error
    import ctypes as C
    dp = C.c_void_p()
    assert lib.lmpc_dev_alloc(h, C.c_longlong(1 << 60), C.byref(dp)) == -2 and "memory" in lib.lmpc_last_error().decode()
    assert not ctx.local_position(x[:8], y[:8], psi[:8], max_ey)[3].any()
    assert lib.lmpc_local_position_batch(h, 4, p, p, p, 0.0, q, q + 32, q + 64, si) == 0 and not sti.any()      # the origin, max_ey = 0: an end point


def test_heading_unwrap_at_the_pi_edges(ctx, t):
    """np.unwrap's rule where it is decided: headings exactly pi, 3 pi, 5 pi away from the row's angle and their floating-point neighbours, both signs, at a point on the
    centre line of the first straight (row angle 0) and at the stored end point of a curved row (row angle = its psi).  unwrap is additions, subtractions and one fmod,
    all correctly rounded on both sides, so epsi must be tests/track_ref.py's (np.unwrap's) bit for bit; |epsi| never exceeds pi."""
    pt = np.array(t["track"]); max_ey = float(t["max_ey"])
    base = np.array([k * np.pi for k in (1, 3, 5, 2, 4)])
    edge = np.concatenate([base, np.nextafter(base, 0.0), np.nextafter(base, 100.0)]); edge = np.concatenate([edge, -edge, [0.0]])
    cases = [(0.5, 0.0, 0.0), (pt[1, 0], pt[1, 1], pt[1, 2]), (pt[2, 0], pt[2, 1], pt[2, 2])]
    x = np.concatenate([np.full(edge.size, c[0]) for c in cases]); y = np.concatenate([np.full(edge.size, c[1]) for c in cases])
    psi = np.concatenate([c[2] + edge for c in cases])
    s, ey, epsi, st = ctx.local_position(x, y, psi, max_ey)
    rs, rey, repsi, rst, _ = track_ref.local_position_batch(pt, x, y, psi, max_ey)
    assert not st.any() and not rst.any()
    assert np.array_equal(epsi, repsi) and np.array_equal(s, rs) and np.array_equal(ey, rey)
    assert np.abs(epsi).max() <= np.pi and np.any(epsi == np.pi) and np.any(epsi == -np.pi)
