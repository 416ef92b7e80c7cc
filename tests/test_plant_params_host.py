"""CPU: per-car vehicle constants of the plant -- the C ABI's default row, the parametrised references pinned to the existing ones, the fitness of the GPU
test's inputs for its tolerance, the row builder _capi.plant_params and the hand-over of the rows by BatchedRollouts / bootstrap."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import common
from tests import plant_params_ref as ppr
from tests import plant_ref as pr
from tests import standin_capi


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_ld(p, q):
    """The same longdouble values, NaN and the sign of zero included (the x87 format carries padding bytes: the bytes themselves cannot be compared)."""
    return bool(np.all(((p == q) | (np.isnan(p) & np.isnan(q))) & (np.signbit(p) == np.signbit(q))))


def test_default_row_version_and_exports(built):
    """lmpc_plant_params_default returns the ten values of SysModel.py:60-70 bit for bit (Df = Dr = 0.8 * m * 9.81 / 2.0 evaluated in that order), the library is
    version 102 or later and exports the three entry points."""
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 102
    for name in ("lmpc_plant_params_default", "lmpc_plant_set_params", "lmpc_plant_get_params"):
        assert name in _capi.EXPORTS and hasattr(lib, name), name
    par = np.full(10, np.nan)
    assert lib.lmpc_plant_params_default(C.c_void_p(par.ctypes.data)) == 0
    m = 1.98
    want = np.array([m, 0.125, 0.125, 0.024, 0.8 * m * 9.81 / 2.0, 1.25, 1.0, 0.8 * m * 9.81 / 2.0, 1.25, 1.0])
    assert np.array_equal(_bits(par), _bits(want)), (par, want)
    assert np.array_equal(_bits(_capi.plant_params_default()), _bits(want)) and np.array_equal(_bits(ppr.default_row()), _bits(want))
    assert lib.lmpc_plant_params_default(None) == -1
    assert _capi.PLANT_PARAM_NAMES == ppr.NAMES and _capi.PLANT_NPAR == ppr.NPAR == 10


def test_parametrised_references_are_pinned_to_the_existing_ones():
    """At the reference's constants dyn_model_ld_par gives the longdouble bits of plant_ref.dyn_model_ld on every family of plant_ref.families, and
    dyn_model_f64_par the float64 bits of oracle.dyn_model on "lmpc regime"."""
    g = common.load_lmpc_golden()
    pt = np.array(g["track"])
    fams = pr.families(g)
    assert len(fams) == 9
    for f in fams:
        par = np.tile(ppr.default_row(), (len(f), 1))
        a = pr.dyn_model_ld(pt, f.x, f.xg, f.u, f.nz)
        b = ppr.dyn_model_ld_par(pt, f.x, f.xg, f.u, f.nz, par)
        for p, q in zip(a[:2], b[:2]):
            assert p.dtype == q.dtype == np.longdouble and _same_ld(p, q), f.name
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), f.name
    f = fams[0]
    assert f.name == "lmpc regime"
    par = np.tile(ppr.default_row(), (len(f), 1))
    xn, xgn, raised = ppr.dyn_model_f64_par(pt, f.x, f.xg, f.u, f.nz, par)
    assert not raised.any()
    for b in range(len(f)):
        o = pr.oracle_step(pt, f.x[b], f.xg[b], f.u[b], f.nz[b])
        assert np.array_equal(_bits(xn[b]), _bits(o[0])) and np.array_equal(_bits(xgn[b]), _bits(o[1])), b


def test_gpu_test_inputs_are_fit_for_the_tolerance():
    """State families x parameter families of tests/test_gpu_plant_params.py: well_conditioned (float64 against longdouble, 1e-13 (1 + |ref|)) leaves out at most 10 % of
    any state family under any parameter family and at most 2 % overall; the two references raise on the same cars.  Printed: per pair the judged / left-out / raising
    counts and the worst float64-against-longdouble error of the judged rest."""
    g = common.load_lmpc_golden()
    cs = ppr.cases(g)
    assert [(c["state"], c["param"]) for c in cs] == [(s, p) for s in ppr.STATE_FAMILIES for p in ppr.PARAM_FAMILIES]
    tot = out = 0
    print()
    for c in cs:
        assert np.array_equal(c["raised"], c["fraised"]), (c["state"], c["param"], np.where(c["raised"] != c["fraised"])[0])
        live = ~c["raised"]
        left = int((live & ~c["ok"]).sum()); n = int(live.sum())
        worst = c["e64"][c["ok"]].max() if c["ok"].any() else 0.0
        print("%-15s (%s): %3d states, %3d raise, %3d judged, %2d left out (worst of them %.1e); judged rest agrees to %.1e"
              % (c["state"], c["param"], len(live), int((~live).sum()), int(c["ok"].sum()), left, c["e64"][live & ~c["ok"]].max() if left else 0.0, worst))
        assert left <= 0.10 * n, (c["state"], c["param"], left, n)
        assert worst <= ppr.WELL_TOL
        tot += n; out += left
    print("overall: %d of %d left out" % (out, tot))
    assert out <= 0.02 * tot, (out, tot)
    # every family keeps enough judged states to mean something, and the parameter families are what they are named after
    assert all(c["ok"].sum() >= 5 for c in cs)
    p = ppr.param_families(64, 1)
    d = ppr.default_row()
    assert np.all(np.abs(p["a"] / d - 1) <= 0.2) and np.all(p["a"] != d)
    assert np.all((p["b"][:, 0] >= 1.5) & (p["b"][:, 0] <= 2.5)) and np.array_equal(p["b"][:, [1, 2, 3, 5, 6, 8, 9]], np.tile(d[[1, 2, 3, 5, 6, 8, 9]], (64, 1)))
    mu = p["b"][:, [4, 7]] / (p["b"][:, :1] * 9.81 / 2.0)
    assert np.all((mu > 0.3 - 1e-12) & (mu < 1.0 + 1e-12))
    assert np.all((p["c"][:, [5, 8]] >= 1.3) & (p["c"][:, [5, 8]] <= 2.2) & (p["c"][:, [6, 9]] >= 1.0) & (p["c"][:, [6, 9]] <= 4.0))
    assert np.all(p["c"][:, 5] != p["c"][:, 8]) and np.all(p["c"][:, 6] != p["c"][:, 9])
    assert np.all((p["d"][:, 1] >= 0.09) & (p["d"][:, 1] <= 0.16)) and np.array_equal(p["d"][:, 2], 0.25 - p["d"][:, 1])


def test_plant_params_builder():
    """_capi.plant_params: the defaults are the reference's row bit for bit, scalars and (B,) arrays broadcast, D = mu * m * 9.81 / 2.0 left to right unless Df / Dr
    are given, and everything lmpc_plant_set_params would refuse is a ValueError."""
    from racinglmpc_amd import _capi
    d = ppr.default_row()
    p = _capi.plant_params(5)
    assert p.shape == (5, 10) and p.dtype == np.float64 and p.flags["C_CONTIGUOUS"]
    assert all(np.array_equal(_bits(r), _bits(d)) for r in p)
    m = np.array([1.5, 1.98, 2.5]); mu = np.array([0.3, 0.8, 1.0])
    p = _capi.plant_params(3, m=m, mu_f=mu, mu_r=0.5, lf=0.1, lr=[0.15, 0.14, 0.13], Cf=2.0, Br=3.0)
    assert np.array_equal(p[:, 0], m) and np.array_equal(p[:, 4], mu * m * 9.81 / 2.0) and np.array_equal(p[:, 7], 0.5 * m * 9.81 / 2.0)
    assert np.array_equal(p[:, 1], [0.1] * 3) and np.array_equal(p[:, 2], [0.15, 0.14, 0.13]) and np.all(p[:, 5] == 2.0) and np.all(p[:, 9] == 3.0)
    assert np.array_equal(p[:, [3, 6, 8]], np.tile(d[[3, 6, 8]], (3, 1)))
    p = _capi.plant_params(2, Df=[5.0, 6.0], Dr=7.0, mu_f=0.1, m=3.0)                   # Df / Dr given: mu is not used
    assert np.array_equal(p[:, 4], [5.0, 6.0]) and np.array_equal(p[:, 7], [7.0, 7.0]) and np.all(p[:, 0] == 3.0)
    for kw in (dict(m=0.0), dict(m=-1.0), dict(Iz=0.0), dict(Iz=[0.024, -0.1]), dict(lf=np.nan), dict(mu_f=np.inf), dict(Df=[1.0, np.nan]), dict(m=[1.0, 2.0, 3.0]),
               dict(Cf=np.ones((2, 1)))):
        with pytest.raises(ValueError):
            _capi.plant_params(2, **kw)
    with pytest.raises(ValueError):
        _capi.plant_params(0)
    for bad in (np.zeros((2, 9)), np.zeros((2, 2, 10)), np.full((1, 10), np.nan), np.r_[0.0, d[1:]][None], np.r_[d[:3], -1.0, d[4:]][None]):
        with pytest.raises(ValueError):
            _capi.check_plant_params(bad)
    assert _capi.check_plant_params(d).shape == (1, 10)


class _Ctx(standin_capi.Context):
    """The stand-in context with the session entry points the lap runners call: records the order of the calls and the rows handed over."""

    def plant_set_params(self, par):
        standin_capi._rec("plant_set_params", None if par is None else np.array(par))

    def _open(self, kind, x0, noise):
        standin_capi._rec(kind, np.asarray(x0).shape[0]); self._B = np.asarray(x0).shape[0]; self._T = np.asarray(noise).shape[0]

    def rollout_begin(self, x0, xglob0, xLin0, uLin0, noise):
        self._open("rollout_begin", x0, noise)

    def rollout_begin_mpc(self, x0, xglob0, noise, xLin0=None, uLin0=None, A=None, B=None, stop_at_line=False):
        self._open("rollout_begin_mpc", x0, noise)

    def rollout_pid(self, x0, xglob0, vt, noise_u, noise, stop_at_line=False):
        self._open("rollout_pid", x0, noise)
        return self._T, self._B

    def rollout_run(self, n):
        return self._T, self._B

    def rollout_fetch(self, t0, t1):
        B, n = self._B, t1 - t0
        return (np.zeros((n, B, 6)), np.zeros((n, B, 2)), np.zeros((n, B, 6)), np.full(B, 5, np.int32), np.zeros(B, np.int32), np.zeros((B, 6)), np.zeros((B, 6)))

    def rollout_end(self):
        standin_capi._rec("rollout_end")


def _calls(since):
    return [c for c in standin_capi.CALLS[since:] if c[0] in ("plant_set_params", "rollout_begin", "rollout_begin_mpc", "rollout_pid")]


def test_rollouts_hand_the_rows_to_the_context_before_each_stage(monkeypatch):
    """BatchedRollouts(plant_params=rows): Context.plant_set_params(rows) directly in front of rollout_begin, rollout_pid and rollout_begin_mpc, every time; without rows the
    context's parameters are not touched; a row count that is neither 1 nor the number of cars is refused before the session begins.  bootstrap(plant_params=rows) does
    the same in its three stages."""
    from racinglmpc_amd import _capi, rollout
    g = common.load_lmpc_golden()
    track = np.array(g["track"])
    B, T = 6, 30
    rows = _capi.plant_params(B, m=np.linspace(1.5, 2.5, B))
    cfg = types.SimpleNamespace(N=12, numSS_it=0, numSS_points=0, trToUse=1, par=None, track=track, trackLength=float(g["trackLength"]))
    x0 = np.zeros((B, 6))

    def drive(ro):
        n0 = len(standin_capi.CALLS)
        ro.begin(x0, np.zeros((13, 6)), np.zeros((12, 2)), max_steps=T); ro.ctx.rollout_end()
        ro.run_pid_laps(np.full(B, 0.8), max_steps=T)
        ro.run_mpc_laps(x0, A=np.zeros((B, 6, 6)), B=np.zeros((B, 6, 2)), max_steps=T)
        ro.run_mpc_laps(x0, xLin0=np.zeros((13, 6)), uLin0=np.zeros((12, 2)), max_steps=T)
        ro.close()
        return _calls(n0)
    for par in (rows, rows[:1], rows[0]):
        calls = drive(rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False, plant_params=par))
        assert [c[0] for c in calls] == ["plant_set_params", "rollout_begin", "plant_set_params", "rollout_pid", "plant_set_params", "rollout_begin_mpc",
                                         "plant_set_params", "rollout_begin_mpc"]
        assert all(np.array_equal(c[1], np.atleast_2d(par)) for c in calls[0::2])
    calls = drive(rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False))
    assert [c[0] for c in calls] == ["rollout_begin", "rollout_pid", "rollout_begin_mpc", "rollout_begin_mpc"]
    ro = rollout.BatchedRollouts(_Ctx(cfg), track, seed=1, prefetch=False, plant_params=rows[:4])
    n0 = len(standin_capi.CALLS)
    with pytest.raises(ValueError):
        ro.run_pid_laps(np.full(B, 0.8), max_steps=T)
    assert not _calls(n0)
    with pytest.raises(ValueError):
        rollout.BatchedRollouts(_Ctx(cfg), track, plant_params=np.zeros((B, 10)))           # m = 0: refused where the rows are given

    # bootstrap: the three stages on a stand-in module (the LTI regression of the stage in between is not what is looked at)
    fake = types.SimpleNamespace(Context=_Ctx, config_from=standin_capi.config_from, check_plant_params=_capi.check_plant_params, ST_INEXACT=_capi.ST_INEXACT,
                                 lti_regression_batch=lambda laps, lamb, device=0: (np.zeros((len(laps), 6, 6)), np.zeros((len(laps), 6, 2)), np.zeros((len(laps), 2, 6)),
                                                                                      np.zeros(len(laps), np.int32)))
    monkeypatch.setattr(rollout, "_capi", fake)
    n0 = len(standin_capi.CALLS)
    out = rollout.bootstrap(track, B, 12, 0.8, 3, max_steps=T, plant_params=rows)
    calls = _calls(n0)
    assert [c[0] for c in calls] == ["plant_set_params", "rollout_pid", "plant_set_params", "rollout_begin_mpc", "plant_set_params", "rollout_begin_mpc"]
    assert all(np.array_equal(c[1], rows) for c in calls[0::2]) and all(c[1] == B for c in calls[1::2])
    assert len(out["pid"]) == len(out["mpc"]) == len(out["ltvmpc"]) == B
    n0 = len(standin_capi.CALLS)
    rollout.bootstrap(track, B, 12, 0.8, 3, max_steps=T)
    assert [c[0] for c in _calls(n0)] == ["rollout_pid", "rollout_begin_mpc", "rollout_begin_mpc"]


def test_context_pool_forwards_the_setter_to_every_member():
    """ContextPool.plant_set_params reaches every member (its __getattr__ forwards store edits only, by name)."""
    from racinglmpc_amd import _capi
    seen = []
    pool = _capi.ContextPool.__new__(_capi.ContextPool)
    pool.members = [types.SimpleNamespace(plant_set_params=lambda par, i=i: seen.append((i, par)), plant_params=lambda i=i: "rows of %d" % i) for i in range(3)]
    pool._next = 0
    pool.plant_set_params("rows")
    assert seen == [(0, "rows"), (1, "rows"), (2, "rows")] and pool.plant_params() == "rows of 0"
