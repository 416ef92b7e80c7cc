"""-m gpu: the counter-based noise generated on the device (csrc/lmpc_noise.hip.h): raw words against NumPy's Philox generator, normals against the NumPy restatement
(tests/noise_ref.py), shard-invariant addressing, sessions that consume exactly the draws lmpc_noise_fill returns, the source switched off, and two shards of one job
through BatchedRollouts(device_noise=True)."""
import numpy as np
import pytest

from tests import common
from tests import noise_ref

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TOL_Z = 1e-13                  # |device - NumPy restatement| per draw, absolute: see test_normals_match_the_restatement
T, T0, B, CAR0, LAP = 3, 7, 65, 2 ** 32 + 5, 3     # one car more than a wavefront, a 64-bit car index


@pytest.fixture(scope="module")
def g(built):
    return common.load_lmpc_golden()


@pytest.fixture(scope="module")
def ctx(g):
    """A context that needs only the track (no lap store): the generator entry points and PID sessions."""
    from racinglmpc_amd import _capi
    cfg, _ = common.mpc_config(g, 12, max_batch=65)
    c = _capi.Context(cfg)
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b):
    """bit for bit, signed zeros included"""
    return np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b))


def _code(f):
    from racinglmpc_amd import _capi
    with pytest.raises(_capi.LmpcError) as e:
        f()
    return int(str(e.value).split()[2].rstrip(":"))


def test_raw_words_are_numpy_philox(ctx):
    """noise_raw(seed, stream, lap = 3, t0 = 7, T = 3, car0 = 2**32 + 5, B = 65), stream 0 and 1, seed 11 and 2**64 - 1: every (t, car) row is bit-identical to
    numpy.random.Philox(counter=[t, car, lap, stream], key=[seed, 0]).random_raw(4)."""
    for seed in (11, 2 ** 64 - 1):
        for stream in (0, 1):
            w = ctx.noise_raw(seed, stream, LAP, T0, T, CAR0, B)
            assert w.shape == (T, B, 4) and w.dtype == np.uint64
            for i in range(T):
                for b in range(B):
                    want = noise_ref.numpy_words(seed, stream, LAP, T0 + i, CAR0 + b)
                    assert np.array_equal(w[i, b], want), (seed, stream, i, b, w[i, b], want)
            assert np.array_equal(w, noise_ref.raw(seed, stream, LAP, T0, T, CAR0, B))
    # t = 0 is NumPy's first block of the zero counter (the block function at word 0 = 1)
    assert np.array_equal(ctx.noise_raw(0, 0, 0, 0, 1, 0, 1)[0, 0], noise_ref.numpy_words(0, 0, 0, 0, 0))


def test_normals_match_the_restatement(ctx):
    """noise_fill at the same shape, width 3 and width 2, against noise_ref.fill: |delta| <= 1e-13 absolute on every draw.  The bound is derived, not fitted:
    r <= sqrt(2 * 53 * ln 2) = 8.6; log, sin and cos are within a few ulp on both sides; rounding of 2 pi u2 adds at most 7e-16 * r; the sum stays below 1e-14 and the
    bound allows ten times that.  Width 2 equals the first two columns of a width-3 fill of stream 1, bit for bit.  The worst value is printed."""
    worst = 0.0
    for seed in (11, 2 ** 64 - 1):
        for stream, width in ((0, 3), (1, 2), (1, 3), (0, 2)):
            z = ctx.noise_fill(seed, stream, LAP, T0, T, CAR0, B, width)
            ref = noise_ref.fill(seed, stream, LAP, T0, T, CAR0, B, width)
            assert z.shape == ref.shape == (T, B, width) and np.all(np.isfinite(z))
            d = float(np.abs(z - ref).max())
            worst = max(worst, d)
            print("noise_fill seed %d stream %d width %d: worst |device - restatement| %.3e" % (seed, stream, width, d))
            assert d <= TOL_Z, (seed, stream, width, d)
        assert _same(ctx.noise_fill(seed, 1, LAP, T0, T, CAR0, B, 2), ctx.noise_fill(seed, 1, LAP, T0, T, CAR0, B, 3)[..., :2])
    # a larger sample for the printed figure (and the moments): 400 steps x 64 cars
    z = ctx.noise_fill(5, 0, 0, 0, 400, 0, 64, 3); ref = noise_ref.fill(5, 0, 0, 0, 400, 0, 64, 3)
    d = float(np.abs(z - ref).max()); worst = max(worst, d)
    print("noise_fill 400 x 64 x 3: worst %.3e; mean %.4f, std %.4f; worst overall %.3e" % (d, z.mean(), z.std(), worst))
    assert d <= TOL_Z and abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    # argument checks of both entry points
    for bad in (dict(width=1), dict(width=4), dict(T=0), dict(B=0), dict(t0=-1), dict(car0=-1)):
        a = dict(seed=1, stream=0, lap=0, t0=0, T=2, car0=0, B=2, width=3); a.update(bad)
        assert _code(lambda: ctx.noise_fill(**a)) == -1, bad
        if "width" not in bad:
            a.pop("width")
            assert _code(lambda: ctx.noise_raw(**a)) == -1, bad


def test_addressing_is_shard_invariant(ctx):
    """Columns 32..64 of a fill with car0 = 0, B = 65 equal a fill with car0 = 32, B = 33, bit for bit; rows 2..4 of a fill from t0 = 0 equal a fill from t0 = 2; other
    seeds, laps and streams give other draws."""
    for stream, width in ((0, 3), (1, 2)):
        whole = ctx.noise_fill(11, stream, 2, 0, 5, 0, 65, width)
        assert _same(whole[:, 32:65], ctx.noise_fill(11, stream, 2, 0, 5, 32, 33, width))
        assert _same(whole[2:5], ctx.noise_fill(11, stream, 2, 2, 3, 0, 65, width))
        assert _same(whole[3:4, 64:65], ctx.noise_fill(11, stream, 2, 3, 1, 64, 1, width))
        for other in (ctx.noise_fill(12, stream, 2, 0, 5, 0, 65, width), ctx.noise_fill(11, stream, 3, 0, 5, 0, 65, width), ctx.noise_fill(11, 1 - stream, 2, 0, 5, 0, 65, width)):
            assert not np.any(other == whole)
    raw = ctx.noise_raw(11, 0, 2, 0, 5, 0, 65)
    assert np.array_equal(raw[:, 32:65], ctx.noise_raw(11, 0, 2, 0, 5, 32, 33)) and np.array_equal(raw[2:5], ctx.noise_raw(11, 0, 2, 2, 3, 0, 65))


def _lmpc_inputs(g, nb):
    x0 = np.zeros((nb, 6)); x0[:, 0] = np.linspace(0.5, 0.9, nb); x0[:, 5] = np.linspace(-0.1, 0.1, nb)[::-1]
    return x0, np.tile(g["SS0"][1:14][None], (nb, 1, 1)), np.tile(g["uSS0"][1:13][None], (nb, 1, 1))


def _fetch_all(c, t):
    out = c.rollout_fetch(0, t)
    c.rollout_end()
    return out


def test_lmpc_session_consumes_exactly_those_draws(g):
    """LMPC session on the golden N = 12 stores, B = 33 (one car more than a plant work-group's 32), T_max = 8: rollout_set_noise(True, 11, 2, 100) with noise=None
    against the source off and the host array noise_fill(11, 0, 2, 0, 8, 100, 33, 3) -- X, U, Xglob, doneAt, status (and the final states) bit-identical.  The
    source is taken when the session begins: setting another one while it runs changes nothing; a session after it does."""
    nb, Tm = 33, 8
    c, _ = common.make_lmpc_ctx(g, 4, max_batch=64)
    x0, xl, ul = _lmpc_inputs(g, nb)
    c.rollout_set_noise(True, 11, 2, 100)
    c.rollout_begin(x0, x0, xl, ul, None, T_max=Tm)
    c.rollout_set_noise(True, 12, 9, 0)                      # (reaches the next session only)
    t, _ = c.rollout_run(Tm)
    dev = _fetch_all(c, t)
    assert t == Tm
    c.rollout_begin(x0, x0, xl, ul, None, T_max=Tm)          # the next session: source (12, 9, 0)
    t, _ = c.rollout_run(Tm)
    other = _fetch_all(c, t)
    c.rollout_set_noise(False)
    nz = c.noise_fill(11, 0, 2, 0, Tm, 100, nb, 3)
    c.rollout_begin(x0, x0, xl, ul, nz)
    t, _ = c.rollout_run(Tm)
    host = _fetch_all(c, t)
    for i, (a, b) in enumerate(zip(dev, host)):
        assert _same(a, b), i
    assert np.all(np.isfinite(dev[0])) and dev[0][1:].any() and not _same(other[0], dev[0])
    # ... and with the source on a given array still wins
    c.rollout_set_noise(True, 77, 5, 3)
    c.rollout_begin(x0, x0, xl, ul, nz)
    t, _ = c.rollout_run(Tm)
    for i, (a, b) in enumerate(zip(_fetch_all(c, t), host)):
        assert _same(a, b), i
    nz2 = c.noise_fill(12, 0, 9, 0, Tm, 0, nb, 3)
    c.rollout_set_noise(False)
    c.rollout_begin(x0, x0, xl, ul, nz2)
    t, _ = c.rollout_run(Tm)
    for i, (a, b) in enumerate(zip(_fetch_all(c, t), other)):
        assert _same(a, b), i
    c.close()


def test_pid_session_consumes_both_streams(ctx):
    """rollout_pid, B = 33, T_max = 16: noise_u = noise = None with the source (11, 2, 100) against the host arrays noise_fill(.., stream 1, width 2) and
    noise_fill(.., stream 0, width 3) with the source off; also one array given and the other generated."""
    nb, Tm = 33, 16
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (nb, 1)); x0[:, 5] = np.linspace(-0.1, 0.1, nb)
    vt = 0.6 + 0.01 * np.arange(nb)
    ctx.rollout_set_noise(True, 11, 2, 100)
    t, _ = ctx.rollout_pid(x0, x0, vt, None, None, T_max=Tm)
    dev = _fetch_all(ctx, t)
    nu = ctx.noise_fill(11, 1, 2, 0, Tm, 100, nb, 2); nz = ctx.noise_fill(11, 0, 2, 0, Tm, 100, nb, 3)
    t, _ = ctx.rollout_pid(x0, x0, vt, nu, None)
    mixed_a = _fetch_all(ctx, t)
    t, _ = ctx.rollout_pid(x0, x0, vt, None, nz)
    mixed_b = _fetch_all(ctx, t)
    ctx.rollout_set_noise(False)
    t, _ = ctx.rollout_pid(x0, x0, vt, nu, nz)
    host = _fetch_all(ctx, t)
    assert t == Tm
    for i, (a, b, c, d) in enumerate(zip(dev, host, mixed_a, mixed_b)):
        assert _same(a, b) and _same(c, b) and _same(d, b), i
    # the control law sees stream 1: u_t is Utilities.PID.solve on the device's own row t with the draws of nu (the bits test_gpu_mpc_stages checks for host arrays)
    X, U = dev[0], dev[1]
    for k in range(Tm):
        u = np.stack([-0.6 * X[k, :, 5] - 0.9 * X[k, :, 3] + np.clip(nu[k, :, 0] * 0.25, -0.9, 0.9), 1.5 * (vt - X[k, :, 0]) + np.clip(nu[k, :, 1] * 0.10, -0.2, 0.2)], axis=1)
        assert _same(U[k], u), k


def test_lti_mpc_session_consumes_exactly_those_draws(g):
    """One rollout_begin_mpc LTI session, B = 33, T_max = 8: device source against the host array of noise_fill, bit-identical logs."""
    from racinglmpc_amd import _capi
    nb, Tm = 33, 8
    cfg, _ = common.mpc_config(g, 12, max_batch=nb)
    c = _capi.Context(cfg)
    laps = [(np.array(g["xPID"])[7 * b:], np.array(g["uPID"])[7 * b:]) for b in range(nb)]
    A, Bm, _, st = _capi.lti_regression_batch(laps, 1e-7)
    assert np.all(st == 0)
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (nb, 1)); x0[:, 5] = np.linspace(-0.15, 0.15, nb)
    c.rollout_set_noise(True, 11, 2, 100)
    c.rollout_begin_mpc(x0, x0, None, A=A, B=Bm, T_max=Tm)
    t, _ = c.rollout_run(Tm)
    dev = _fetch_all(c, t)
    c.rollout_set_noise(False)
    c.rollout_begin_mpc(x0, x0, c.noise_fill(11, 0, 2, 0, Tm, 100, nb, 3), A=A, B=Bm)
    t, _ = c.rollout_run(Tm)
    host = _fetch_all(c, t)
    c.close()
    assert t == Tm and np.all(np.isfinite(dev[0])) and dev[0][1:].any()
    for i, (a, b) in enumerate(zip(dev, host)):
        assert _same(a, b), i


def test_off_means_unchanged(g, ctx):
    """Source off (a new context): noise=None is the LMPC_E_ARG of a missing array in all three entry points and leaves no session behind; the same after
    set_noise(True, ...) then set_noise(False, ...); rollout_get_noise returns what was set; a negative car0 is refused and changes nothing."""
    from racinglmpc_amd import _capi
    nb, Tm = 5, 4
    lm, _ = common.make_lmpc_ctx(g, 4, max_batch=8)
    x0, xl, ul = _lmpc_inputs(g, nb)
    vt = np.full(nb, 0.8)
    A = np.tile(np.eye(6)[None], (nb, 1, 1)); Bm = np.zeros((nb, 6, 2))

    def refused():
        assert _code(lambda: lm.rollout_begin(x0, x0, xl, ul, None, T_max=Tm)) == -1
        assert _code(lambda: ctx.rollout_begin_mpc(x0, x0, None, A=A, B=Bm, T_max=Tm)) == -1
        assert _code(lambda: ctx.rollout_pid(x0, x0, vt, None, None, T_max=Tm)) == -1
        assert _code(lambda: ctx.rollout_pid(x0, x0, vt, np.zeros((Tm, nb, 2)), None)) == -1
        assert _code(lambda: ctx.rollout_pid(x0, x0, vt, None, np.zeros((Tm, nb, 3)))) == -1
        t, _ = ctx.rollout_pid(x0, x0, vt, np.zeros((Tm, nb, 2)), np.zeros((Tm, nb, 3)))     # (no session was left active by the refused calls)
        ctx.rollout_end()
        assert t == Tm
    for c in (lm, ctx):
        c.rollout_set_noise(False)
    assert lm.rollout_get_noise() == (False, 0, 0, 0)
    assert _capi.Context(common.mpc_config(g, 12, max_batch=4)[0]).rollout_get_noise() == (False, 0, 0, 0)       # the state after lmpc_create
    refused()
    for c in (lm, ctx):
        c.rollout_set_noise(True, 2 ** 64 - 1, 2 ** 63 + 1, 2 ** 40 + 3)
        assert c.rollout_get_noise() == (True, 2 ** 64 - 1, 2 ** 63 + 1, 2 ** 40 + 3)
        assert _code(lambda: c.rollout_set_noise(True, 1, 1, -1)) == -1
        assert c.rollout_get_noise() == (True, 2 ** 64 - 1, 2 ** 63 + 1, 2 ** 40 + 3)
        c.rollout_set_noise(False, 7, 8, 9)
        assert c.rollout_get_noise() == (False, 7, 8, 9)
    refused()
    lm.close()


def test_two_shards_of_one_job_see_the_draws_of_the_whole(g):
    """BatchedRollouts(device_noise=True) on two contexts with noise_shard = (0, 17, 33) and (17, 33, 33), one 8-step PID session each: the laps equal columns 0..16
    and 17..32 of one 33-car object, bit for bit -- and they would not with the shard offset ignored."""
    from racinglmpc_amd import _capi, rollout
    nb, Tm, seed = 33, 8, 2 ** 40 + 7
    track = np.array(g["track"])
    vt = 0.6 + 0.01 * np.arange(nb)
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (nb, 1)); x0[:, 5] = np.linspace(-0.1, 0.1, nb)

    def laps(lo, hi, shard):
        c = _capi.Context(rollout.mpc_stage_config(track, 12, 0.8, hi - lo))
        ro = rollout.BatchedRollouts(c, track, seed=seed, device_noise=True)
        if shard:
            ro.noise_shard = (lo, hi, nb)
        out = ro.run_pid_laps(vt[lo:hi], x0[lo:hi], max_steps=Tm, keep_invalid=True)
        assert ro.lap == 1 and c.rollout_get_noise() == (True, seed, 0, lo if shard else 0)
        ro.close(); c.close()
        return out
    whole = laps(0, nb, False)
    parts = laps(0, 17, True) + laps(17, nb, True)
    assert len(whole) == len(parts) == nb
    for b in range(nb):
        for i in range(4):
            assert _same(whole[b][i], parts[b][i]), (b, i)
        assert whole[b][4:] == parts[b][4:]
    unsharded = laps(17, nb, False)                              # (cars 17.. with the draws of cars 0..: another disturbance)
    assert not _same(unsharded[0][0], whole[17][0])
