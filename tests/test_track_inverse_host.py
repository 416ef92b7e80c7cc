"""CPU: the inverse track map -- the NumPy restatement (tests/track_ref.py) against what the executed reference returned (tests/golden/local_position/track_local.npz:
Map.getLocalPosition, Track.py:191-290, and Map.getAngle, Track.py:312-349), the three entry points in the library, the header and the ctypes layer, and
rollout.lap_from_global / seed_lmpc(from_global=...) against the recording CPU stand-in (tests/standin_track.py)."""
import os
import re

import numpy as np
import pytest

from tests import common
from tests import track_ref

NEW = ("lmpc_local_position_batch", "lmpc_track_angle_batch", "lmpc_state_from_global_batch")
TOL = 1e-12       # absolute.  The fixture and track_ref evaluate the same NumPy calls on the same doubles; the reference's own round trip (s, ey, epsi) -> pose ->
#                   (s, ey, epsi) over population (a) is 2e-15, so this is ten thousand times the rounding at stake


def fixture():
    return np.load(os.path.join(common.GOLDEN, "local_position", "track_local.npz"))


def fixture_rows(t):
    """Every getLocalPosition row of the fixture as one table: x, y, psi, want (n, 3: s, ey, epsi), ok (n,), row (n,: the completing track row, -1 = none), group."""
    n = t["a_x"].shape[0]; k = t["d_shift"].shape[0]
    x = np.concatenate([t["a_x"], t["b_x"], t["c_x"], np.tile(t["a_x"], k)])
    y = np.concatenate([t["a_y"], t["b_y"], t["c_y"], np.tile(t["a_y"], k)])
    psi = np.concatenate([t["a_psi"], t["b_psi"], t["c_psi"], (t["a_psi"][None] + t["d_shift"][:, None]).ravel()])
    d_out = np.tile(t["a_out"], (k, 1)); d_out[:, 2] = t["d_epsi"].ravel()      # (d): s, ey and the flag are (a)'s bit for bit -- asserted by the generator
    out = np.concatenate([t["a_out"], t["b_out"], t["c_out"], d_out])
    row = np.concatenate([t["a_row"], t["b_row"], np.full(t["c_x"].shape[0], -1), np.tile(t["a_row"], k)])
    group = np.concatenate([np.full(n, 0), np.full(t["b_x"].shape[0], 1), np.full(t["c_x"].shape[0], 2), np.full(k * n, 3)])
    return x, y, psi, out[:, :3], out[:, 3].astype(int), row, group


FIXTURE_SHA256 = "397e3324ee056e466c1b5d0c2e6f85ef073706e730040f93438538ba1d91fa9b"       # content hash of the fixture, as tests/golden/manifest.py computes it
GENERATOR_BLOB = "54c100a50bcbe4ea407b885af2894637487c1dba"                                 # git blob hash of tests/golden/make_local_position_golden.py


def test_fixture_and_generator_are_the_ones_recorded_here():
    """The fixture lives in tests/golden/local_position/, which tests/golden/MANIFEST.json does not list; its staleness check is here: the content hash of the .npz
    and the blob hash of its generator, computed by the manifest tool's own functions.  A regenerated fixture or an edited generator updates the two constants."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("golden_manifest", os.path.join(common.GOLDEN, "manifest.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    assert m.content_hash(os.path.join(common.GOLDEN, "local_position", "track_local.npz")) == FIXTURE_SHA256
    assert m.git_blob_hash(os.path.join(common.GOLDEN, "make_local_position_golden.py")) == GENERATOR_BLOB
    assert m.diff() == []                            # and the manifest of the other fixtures is as it was


def test_fixture_holds_the_populations_the_issue_names():
    t = fixture()
    x, y, psi, want, ok, row, group = fixture_rows(t)
    pt = t["track"]; TL = float(t["trackLength"])
    assert float(t["max_ey"]) == 0.4 + 0.45 and pt.shape == (7, 6)          # halfWidth + slack as the reference adds them: 0.85 + 1 ulp
    n = t["a_x"].shape[0]
    assert 3900 <= n <= 4000 and np.all(ok[group == 0] == 1)
    edges = np.concatenate([pt[:, 3], [TL]])
    assert np.abs(t["a_s"][:, None] - edges[None]).min() >= 1e-3 and np.abs(t["a_ey"]).max() <= 0.8 and np.abs(t["a_epsi"]).max() <= 0.9
    assert np.abs(t["a_out"][:, :3] - np.stack([t["a_s"], t["a_ey"], t["a_epsi"]], 1)).max() < 1e-14        # the reference's own round trip
    assert t["b_x"].shape[0] >= pt.shape[0] and np.all(ok[group == 1] == 1)
    for bx, by in zip(t["b_x"], t["b_y"]):
        assert np.any((pt[:, 0] == bx) & (pt[:, 1] == by))                                                   # the stored end points, exactly
    assert 40 <= (group == 2).sum() <= 60 and np.all(ok[group == 2] == 0) and np.all(want[group == 2] == 10000.0)
    assert sorted(np.round(t["d_shift"] / (2 * np.pi)).tolist()) == [-2, -1, 1, 2] and (group == 3).sum() == 4 * n
    assert 550 <= t["e_s"].shape[0] <= 650 and t["e_s"].max() > 2 * TL and x.shape[0] % 256 != 0


def test_track_ref_reproduces_every_local_position_row_of_the_fixture():
    """tests/track_ref.py against every Map.getLocalPosition row: status and completing track row exact, s, ey, epsi within 1e-12 absolute."""
    t = fixture()
    x, y, psi, want, ok, row, group = fixture_rows(t)
    s, ey, epsi, st, got_row = track_ref.local_position_batch(t["track"], x, y, psi, float(t["max_ey"]))
    assert np.array_equal(st == 0, ok == 1) and np.all(st[ok == 0] == track_ref.ST_NO_SEGMENT)
    assert np.array_equal(got_row, row), np.nonzero(got_row != row)[0][:10]
    err = np.abs(np.stack([s, ey, epsi], 1) - want)
    for grp, name in enumerate("abcd"):
        print("(%s) worst |track_ref - reference|: s %.2e ey %.2e epsi %.2e" % ((name,) + tuple(err[group == grp].max(axis=0))))
    assert err.max() <= TOL, err.max(axis=0)


def test_track_ref_reproduces_every_angle_row_of_the_fixture():
    t = fixture()
    psi, st = track_ref.track_angle_batch(t["track"], t["e_s"], t["e_epsi"])
    assert np.all(st == 0)
    assert np.abs(psi - t["e_psi"]).max() <= TOL
    TL = float(t["trackLength"])
    for s in (2 * TL, np.nan, np.inf, -0.5):            # the wrapped s is TrackLength exactly / no s at all: no row, where the reference raises
        assert track_ref.track_angle(t["track"], s, 0.1) == (0.0, track_ref.ST_NO_SEGMENT)


def test_track_ref_status_paths():
    """Non-finite inputs and max_ey = 0: the ordinary status paths, no fixture needed."""
    t = fixture(); pt = t["track"]
    for bad in ((np.nan, 0.0, 0.0), (0.5, np.inf, 0.0), (0.5, 0.0, -np.inf)):
        assert track_ref.local_position(pt, *bad, 0.85) == (10000.0, 10000.0, 10000.0, track_ref.ST_NO_SEGMENT, -1)
    assert track_ref.local_position(pt, 0.5, 0.0, 0.1, 0.0)[:4] == (0.5, 0.0, 0.1, 0)               # on the centre line of the first straight
    assert track_ref.local_position(pt, 0.5, 1e-3, 0.1, 0.0)[3] == track_ref.ST_NO_SEGMENT          # 1 mm beside it
    assert track_ref.local_position(pt, pt[2, 0], pt[2, 1], 0.0, 0.0)[3] == 0                       # an end point needs no width


def _header_decl(name):
    header = open(os.path.join(common.ROOT, "include", "lmpc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
    return None if m is None else [" ".join(a.replace("*", " * ").split()) for a in m.group(1).split(",")]


def test_entry_points_are_exported_declared_and_bound(built):
    """liblmpc_hip.so exports the three entry points, include/lmpc_hip.h declares them with the types of the issue, _capi binds them (max_ey as a double) and Context
    has the three methods; lmpc_version() is 104; the argument checks return LMPC_E_ARG."""
    import ctypes as C
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 104
    for name in NEW:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).restype is C.c_int
    cd, d, i = "const double *", "double *", "int *"
    types = lambda name: [a.rsplit(" ", 1)[0] for a in _header_decl(name)[1:]]
    assert types("lmpc_local_position_batch") == ["int", cd, cd, cd, "double", d, d, d, i]
    assert types("lmpc_track_angle_batch") == ["int", cd, cd, d, i]
    assert types("lmpc_state_from_global_batch") == ["int", "int", cd, "double", d, i]
    assert lib.lmpc_local_position_batch.argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 4
    assert lib.lmpc_track_angle_batch.argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    assert lib.lmpc_state_from_global_batch.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    for meth in ("local_position", "track_angle", "state_from_global"):
        assert callable(getattr(_capi.Context, meth)), meth
    # no context: LMPC_E_ARG, not a crash (the checks that need a context -- n < 1, a NULL array, a bad max_ey -- run in tests/test_gpu_track_inverse.py)
    a = np.zeros(4); st = np.zeros(4, np.int32); p = a.ctypes.data
    assert lib.lmpc_local_position_batch(None, 4, p, p, p, 0.85, p, p, p, st.ctypes.data) == -1
    assert lib.lmpc_track_angle_batch(None, 4, p, p, p, st.ctypes.data) == -1
    assert lib.lmpc_state_from_global_batch(None, 1, 1, p, 0.85, p, st.ctypes.data) == -1
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "lmpc_local_position_batch" in open(os.path.join(common.ROOT, doc)).read(), doc
    assert "library version 104" in open(os.path.join(common.ROOT, "CHANGELOG.md")).read()


class _Lib:
    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        def f(*a):
            self.seen.append((name, a)); return 0
        return f


def test_context_methods_hand_over_sizes_and_max_ey():
    """Context.local_position / track_angle / state_from_global flatten their inputs, hand n (or T, B) and max_ey as a Python float to the library and return arrays of
    the input's shape; mismatched lengths and a wrong trailing dimension are refused before anything reaches the library; ContextPool forwards to member 0."""
    from racinglmpc_amd import _capi
    ctx = _capi.Context.__new__(_capi.Context)
    ctx.lib = _Lib(); ctx._h = None; ctx.N = 12; ctx._pid = -1
    s, ey, epsi, st = ctx.local_position(np.zeros((3, 5)), np.zeros(15), np.zeros(15), np.float32(0.5))
    name, a = ctx.lib.seen[-1]
    assert name == "lmpc_local_position_batch" and a[1] == 15 and a[5] == 0.5 and type(a[5]) is float
    assert s.shape == ey.shape == epsi.shape == st.shape == (15,) and st.dtype == np.int32
    psi, st = ctx.track_angle(np.zeros(7), np.zeros(7))
    name, a = ctx.lib.seen[-1]
    assert name == "lmpc_track_angle_batch" and a[1] == 7 and psi.shape == (7,) and st.dtype == np.int32
    x, st = ctx.state_from_global(np.zeros((9, 4, 6)), 0.85)
    name, a = ctx.lib.seen[-1]
    assert name == "lmpc_state_from_global_batch" and a[1:3] == (9, 4) and a[4] == 0.85 and x.shape == (9, 4, 6) and st.shape == (9, 4)
    x, st = ctx.state_from_global(np.zeros((9, 6)), 0.85)
    assert ctx.lib.seen[-1][1][1:3] == (9, 1) and x.shape == (9, 6) and st.shape == (9,)
    n = len(ctx.lib.seen)
    for call in (lambda: ctx.local_position(np.zeros(3), np.zeros(4), np.zeros(3), 0.85), lambda: ctx.track_angle(np.zeros(3), np.zeros(2)),
                 lambda: ctx.state_from_global(np.zeros((9, 5)), 0.85), lambda: ctx.state_from_global(np.zeros(6), 0.85)):
        with pytest.raises(ValueError):
            call()
    assert len(ctx.lib.seen) == n
    other = _capi.Context.__new__(_capi.Context); other.lib = _Lib(); other._h = None; other._pid = -1
    pool = _capi.ContextPool.__new__(_capi.ContextPool); pool.members = [ctx, other]; pool._next = 0
    pool.local_position(np.zeros(2), np.zeros(2), np.zeros(2), 0.85); pool.track_angle(np.zeros(2), np.zeros(2)); pool.state_from_global(np.zeros((2, 6)), 0.85)
    assert [c[0] for c in ctx.lib.seen[n:]] == list(NEW) and other.lib.seen == []


def _standin_ctx(g):
    from oracle import lmpc_oracle as orc
    from tests import standin_track
    par = orc.QPParams.lmpc_default(int(g["N"]))
    cfg = standin_track.config_from(int(g["N"]), par.Q, par.R, par.Qf, par.dR, par.Qslack, par.Fx, par.bx, par.Fu, par.bu, par.xRef, QterminalSlack=par.QterminalSlack,
                                    numSS_Points=int(g["numSS_Points"]), numSS_it=int(g["numSS_it"]), trToUse=4, track=g["track"], trackLength=float(g["trackLength"]))
    return standin_track, standin_track.Context(cfg)


def _global_lap(g, rows):
    """x_glob rows [vx, vy, wz, psi, X, Y] of the first `rows` rows of the fixture's PID lap: psi by track_ref.track_angle, (X, Y) by the oracle's getGlobalPosition."""
    from oracle import lmpc_oracle as orc
    x = g["xPID"][:rows]; pt = g["track"]
    psi, st = track_ref.track_angle_batch(pt, x[:, 4], x[:, 3])
    assert np.all(st == 0)
    xy = np.array([orc.get_global_position(pt, float(s), float(ey)) for s, ey in zip(x[:, 4], x[:, 5])])
    return np.stack([x[:, 0], x[:, 1], x[:, 2], psi, xy[:, 0], xy[:, 1]], axis=1)


@pytest.fixture(scope="module")
def n14():
    g = common.load_variant_golden("lmpc_n14")
    flow = os.path.join(common.GOLDEN, "reference_flow_laps_n14.json")
    assert os.path.exists(flow)                      # (the lap times of the executed reference's flow: the PID lap below is the lap that flow was seeded with)
    return g


def test_lap_from_global_gives_back_a_two_lap_pid_lap(n14):
    """The fixture's PID lap (lmpc_n14.npz: the lap the reference flow of reference_flow_laps_n14.json is seeded with) up to the end of its second lap, taken to the
    inertial frame and back through rollout.lap_from_global on the stand-in: the curvilinear rows return within 1e-12 (s up to 2 TrackLength = 38.5: one ulp is
    7e-15), s continuous across the line -- strictly increasing, past TrackLength --, vx, vy, wz bit for bit."""
    from racinglmpc_amd import rollout
    g = n14; TL = float(g["trackLength"])
    rows = int(np.nonzero(g["xPID"][:, 4] > 2 * TL)[0][0])                       # two full laps
    assert rows < g["xPID"].shape[0] and np.sum(np.diff(np.floor(g["xPID"][:rows, 4] / TL)) > 0) == 1
    xg = _global_lap(g, rows)
    mod, ctx = _standin_ctx(g)
    del mod.CALLS[:]
    x = rollout.lap_from_global(ctx, xg, 0.85)
    assert [c[0] for c in mod.CALLS] == ["state_from_global"] and mod.CALLS[0][1] == (rows, 6)
    want = g["xPID"][:rows]
    assert x.shape == want.shape and np.array_equal(x[:, :3], want[:, :3])
    err = np.abs(x - want).max(axis=0)
    print("lap_from_global: worst |x - fixture| per column", err)
    assert err.max() <= TOL
    assert np.all(np.diff(x[:, 4]) > 0) and x[-1, 4] > TL and x[0, 4] < TL
    raw, st = ctx.state_from_global(xg, 0.85)                                      # the rows as the map returns them: s on the first lap
    assert np.all(st == 0) and raw[:, 4].max() <= TL and np.sum(np.diff(raw[:, 4]) < -TL / 2) == 1
    x2 = rollout.lap_from_global(ctx, xg, 0.85, TL=TL)
    assert np.array_equal(x2, x)


def test_lap_from_global_names_the_first_row_off_the_track(n14):
    from racinglmpc_amd import rollout, _capi
    g = n14
    xg = _global_lap(g, 40)
    mod, ctx = _standin_ctx(g)
    xg[17, 4] += 30.0; xg[31, 5] = np.nan
    with pytest.raises(_capi.LmpcError, match=r"row 17 .*LMPC_ST_NO_SEGMENT"):
        rollout.lap_from_global(ctx, xg, 0.85)
    with pytest.raises(ValueError):
        rollout.lap_from_global(ctx, xg[:, :5], 0.85)


def test_seed_lmpc_default_path_is_unchanged_and_from_global_converts_first(n14):
    """seed_lmpc(ctx, laps) issues the calls it issued before the inverse map existed -- model_add_trajectory, ss_add_trajectory per lap, in the order given, with the
    caller's own arrays --; from_global=True converts each lap with one state_from_global call first and then issues the same sequence with the converted rows."""
    from racinglmpc_amd import rollout
    g = n14
    mod, ctx = _standin_ctx(g)
    seen = []
    for name in ("model_add_trajectory", "ss_add_trajectory"):
        def rec(x, u, name=name, inner=getattr(ctx, name)):
            seen.append((name, x, u)); inner(x, u)
        setattr(ctx, name, rec)
    laps = [(g["xPID"][:300 + 10 * i], g["uPID"][:300 + 10 * i], "extra", i) for i in range(4)]
    before = [(a.copy(), b.copy()) for a, b, _, _ in laps]
    del mod.CALLS[:]
    rollout.seed_lmpc(ctx, laps)
    assert [c[0] for c in mod.CALLS] == ["model_add_trajectory", "ss_add_trajectory"] * 4
    assert [c[1] for c in mod.CALLS] == [s for i in range(4) for s in ((300 + 10 * i, 6),) * 2]
    assert len(seen) == 8
    for i, (lap, (xb, ub)) in enumerate(zip(laps, before)):
        for name, x, u in seen[2 * i:2 * i + 2]:
            assert x is lap[0] and u is lap[1] and np.array_equal(x, xb) and np.array_equal(u, ub)        # the caller's arrays, untouched
    assert seen[0][0] == "model_add_trajectory" and seen[1][0] == "ss_add_trajectory"
    rollout.seed_lmpc(ctx, laps[:1], from_global=False, max_ey=0.85)                                        # (max_ey without from_global: ignored)
    assert [c[0] for c in mod.CALLS[8:]] == ["model_add_trajectory", "ss_add_trajectory"] and seen[-1][1] is laps[0][0]
    # from_global
    glob = [(_global_lap(g, 300 + 10 * i), g["uPID"][:300 + 10 * i]) for i in range(2)]
    del mod.CALLS[:]; del seen[:]
    rollout.seed_lmpc(ctx, glob, from_global=True, max_ey=0.85)
    assert [c[0] for c in mod.CALLS] == ["state_from_global"] * 2 + ["model_add_trajectory", "ss_add_trajectory"] * 2
    for i in range(2):
        assert np.abs(seen[2 * i][1] - g["xPID"][:300 + 10 * i]).max() <= TOL and seen[2 * i][2] is glob[i][1] and seen[2 * i + 1][1] is seen[2 * i][1]
    with pytest.raises(ValueError):
        rollout.seed_lmpc(ctx, glob, from_global=True)


def test_standin_argument_checks(n14):
    """The stand-in refuses what the C entry points refuse with LMPC_E_ARG: no points, a negative or non-finite max_ey."""
    mod, ctx = _standin_ctx(n14)
    z = np.zeros(3)
    for call in (lambda: ctx.local_position(z, z, z, -0.1), lambda: ctx.local_position(z, z, z, np.nan), lambda: ctx.local_position(z[:0], z[:0], z[:0], 0.85),
                 lambda: ctx.track_angle(z[:0], z[:0]), lambda: ctx.state_from_global(np.zeros((0, 6)), 0.85), lambda: ctx.state_from_global(np.zeros((2, 6)), np.inf)):
        with pytest.raises(mod.LmpcError, match="error -1"):
            call()
