"""-m gpu: parking (lmpc_rollout_set_parking / _parked_at, lmpc_debug_live_compact; csrc/lmpc_live.hip.h) -- finished and listed cars leave the launches of a
rollout session, the step's kernels run over the ascending list of the live cars.

Cars are independent problems, so a live car must compute what it computes in the session without parking: every float comparison is bit for bit (as int64 words,
the way tests/test_gpu_session_trace.py::_same does), and nothing here has a tolerance.
Set-up as tests/test_gpu_session_trace.py: N = 12, the lmpc_n12 golden, the PID lap four times in both stores, host-drawn noise with a fixed seed.  The golden's PID
lap first crosses the line at row 305 (checked below); car b starts at xPID[305 - k_b] and linearises about the rows behind it, so it crosses about k_b steps in.
An LMPC session begins with its terminal guess zt at s = 10 (LMPC.__init__, PredictiveControllers.py:330), so a car must start in front of s = 10 to drive the way
the controller is meant to: a car set down a few rows before the line selects a terminal set half a lap behind it and stands still (measured: with k_b = (3, 6, 10,
10, 19) only the first car crossed, carried over the line by its speed).  The cars therefore start in the first half of the lap, k_b >= 160 (s <= 9.2), and a
session takes 164 steps (the LMPC is faster than the PID lap it learns from: about 0.7 k_b + 10 steps to the line) -- some tens of milliseconds; the car that must not cross starts at row 10.
What needs no device is in tests/test_parking_host.py."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

N, T = 12, 164
T_MPC = 216                                  # the plain MPC of initMPCParams drives at the PID lap's pace: its cars need about k_b steps
LINE = 305                                   # first row of the golden's PID lap with s > TrackLength
K6 = (160, 171, 180, 180, 200, 295)                 # rows in front of the line, test 2: cars in different poll windows, two cars in one window, one car that does not cross
E_ARG, E_STATE = "error -1:", "error -4:"
NAMES = ("X", "U", "G", "doneAt", "status", "finalX", "finalG")


@pytest.fixture(scope="module")
def g(built):
    g = common.load_lmpc_golden()
    s, TL = np.array(g["xPID"])[:, 4], float(g["trackLength"])
    assert g["xPID"].shape[0] == 1000 and s[LINE] > TL >= s[LINE - 1] and int(np.argmax(s > TL)) == LINE, (s[LINE - 1:LINE + 1], TL)
    return g


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), what


def _refused(code, call):
    from racinglmpc_amd import _capi
    with pytest.raises(_capi.LmpcError) as e:
        call()
    assert code in str(e.value), str(e.value)
    return str(e.value)


def _lmpc_ctx(g, max_batch=8, runtime=False, **kw):
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=max_batch, **kw)
    ctx = _capi.Context(cfg, runtime_kernel=runtime)
    for _ in range(4):
        ctx.model_add_trajectory(g["xPID"], g["uPID"]); ctx.ss_add_trajectory(g["xPID"], g["uPID"])
    return ctx


def _inputs(g, ks, steps=T, seed=5):
    """Car b at xPID[305 - k_b], its first linearisation trajectory the rows behind that one."""
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    r0 = [LINE - int(k) for k in ks]
    x0 = np.stack([xP[r] for r in r0])
    xl = np.stack([xP[r + 1:r + N + 2] for r in r0]); ul = np.stack([uP[r + 1:r + N + 1] for r in r0])
    return x0, xl, ul, np.random.default_rng(seed).standard_normal((steps, len(ks), 3))


def _session(ctx, inp, park=None, steps=T, trace=None, commit=None):
    """One LMPC session run to `steps` in one rollout_run; park: (mode, cars) or None (parking off)."""
    x0, xl, ul, noise = inp
    ctx.rollout_set_parking(*(park if park is not None else (0, None)))
    if trace is not None:
        ctx.rollout_set_trace(trace)
    ctx.rollout_begin(x0, x0, xl, ul, noise)
    t, nd = ctx.rollout_run(steps)
    out = dict(zip(NAMES, ctx.rollout_fetch(0, t)))
    out.update(t=t, n_done=nd)
    out["parked_at"], out["n_live"] = ctx.rollout_parked_at()
    if trace is not None:
        out["trace"] = ctx.rollout_fetch_trace(0, t)
    if commit is not None:
        out["commit"] = commit(ctx, out)
    ctx.rollout_end()
    return out


def _poll_of(done, steps=T):
    """The first finished-lap poll at or after step `done` of a run of `steps`: the next multiple of 8, or the end of the run."""
    return min(-(-int(done) // 8) * 8, steps)


def _compare_cars(park, ref, cars, what, upto=None):
    """Per car: doneAt, status, finX, finG equal; the log rows [0, upto[b]) equal (upto None: every row both sessions took)."""
    for b in cars:
        for k in ("doneAt", "status", "finalX", "finalG"):
            _same(park[k][b], ref[k][b], (what, k, b))
        n = min(park["t"], ref["t"]) if upto is None else int(upto[b])
        assert n > 0, (what, b)
        for k in ("X", "U", "G"):
            _same(park[k][:n, b], ref[k][:n, b], (what, k, b, n))


# ---- 1
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_compaction_kernel_alone(g, n):
    """lmpc_debug_live_compact against NumPy: wave edge (63 / 64 / 65), chunk edge (1023 / 1024 / 1025), two carries (2049); all live, none, only the last car, every
    second car, a seeded random third, start flags and doneAt mixed, and a second call on top of the first one's parkedAt."""
    from racinglmpc_amd import _capi
    rng = np.random.default_rng(100 + n)
    F = _capi.PARK_FINISHED

    def ref(done, p0, t, mode, prev):
        parked = (prev >= 0) | (p0 != 0) | ((done >= 0) if mode & F else np.zeros(n, bool))
        return np.flatnonzero(~parked).astype(np.int32), np.where(parked & (prev < 0), t, prev).astype(np.int32)

    live_mask = dict(all=np.ones(n, bool), none=np.zeros(n, bool), last=np.arange(n) == n - 1, second=np.arange(n) % 2 == 0, third=rng.random(n) < 1 / 3)
    ctx = _lmpc_ctx(g)
    try:
        for name, lv in live_mask.items():
            for by_flag in (True, False):                       # parked through the start list / through doneAt
                p0 = (~lv).astype(np.int32) if by_flag else np.zeros(n, np.int32)
                done = np.where(lv, -1, rng.integers(1, 40, n)).astype(np.int32) if not by_flag else np.full(n, -1, np.int32)
                live, at = ctx.debug_live_compact(done, p0, 16, F)
                wl, wa = ref(done, p0, 16, F, np.full(n, -1, np.int32))
                assert live.dtype == np.int32 and np.array_equal(live, wl) and np.array_equal(at, wa), (n, name, by_flag)
                assert np.array_equal(live, np.flatnonzero(lv)), (n, name)
        # mixed: a quarter on the start list, a quarter finished; without PARK_FINISHED only the start list parks
        p0 = (rng.random(n) < 0.25).astype(np.int32); done = np.where(rng.random(n) < 0.25, rng.integers(1, 9, n), -1).astype(np.int32)
        for mode in (F, 0, F | _capi.PARK_REROUTE):
            live, at = ctx.debug_live_compact(done, p0, 0, mode)
            wl, wa = ref(done, p0, 0, mode, np.full(n, -1, np.int32))
            assert np.array_equal(live, wl) and np.array_equal(at, wa), (n, "mixed", mode)
        # a second call parks more cars on top: earlier parking steps stay, the new ones carry the new step
        live1, at1 = ctx.debug_live_compact(done, p0, 8, F)
        done2 = np.where((done < 0) & (rng.random(n) < 0.5), 13, done).astype(np.int32)
        live2, at2 = ctx.debug_live_compact(done2, p0, 16, F, parkedAt=at1)
        wl, wa = ref(done2, p0, 16, F, at1)
        assert np.array_equal(live2, wl) and np.array_equal(at2, wa), (n, "second call")
        assert set(np.unique(at2)) <= {-1, 8, 16} and np.array_equal(at2[at1 >= 0], at1[at1 >= 0]) and len(live2) <= len(live1)
    finally:
        ctx.close()


# ---- 2
@pytest.fixture(scope="module")
def six(g):
    """Test 2's pair: the un-parked reference on one context, the parking session (PARK_FINISHED, car 1 on the start list) on another; every car traced.  Read-only."""
    from racinglmpc_amd import _capi
    inp = _inputs(g, K6)
    out = []
    for park in (None, (_capi.PARK_FINISHED, [1])):
        ctx = _lmpc_ctx(g)
        try:
            out.append(_session(ctx, inp, park, trace=np.arange(6)))
        finally:
            ctx.close()
    ref, park = out
    print("un-parked doneAt", list(ref["doneAt"]), "steps", ref["t"], "| parked doneAt", list(park["doneAt"]), "parked_at", list(park["parked_at"]), "steps", park["t"], "| status", list(ref["status"]), list(park["status"]))
    return inp, ref, park


def test_parked_against_unparked_route_kept(six):
    """B = 6, 164 steps, PARK_FINISHED with car 1 on the start list, against the same session without parking on a second context."""
    inp, ref, park = six
    d = ref["doneAt"]
    # preconditions on the reference's own crossing steps: two cars in different poll windows, two in the same one, car 5 does not cross
    win = lambda b: (int(d[b]) - 1) // 8
    assert all(d[b] >= 1 for b in range(5)) and d[5] < 0, list(d)
    wins = [win(b) for b in (0, 2, 3, 4)]                                                      # (car 1 is parked from step 0 in the session under test)
    assert 2 <= len(set(wins)) < len(wins), (list(d), wins)                                    # measured: 125, 128 | 133 | 149 -> windows 15, 15, 16, 18
    assert not (ref["parked_at"] >= 0).any() and ref["n_live"] == 6
    want = [_poll_of(d[b]) if d[b] >= 0 else -1 for b in range(6)]; want[1] = 0
    assert list(park["parked_at"]) == want, (list(park["parked_at"]), want)
    assert park["n_live"] == 1
    others = [0, 2, 3, 4, 5]
    _compare_cars(park, ref, others, "parked against un-parked", upto=[d[b] if d[b] >= 0 else T for b in range(6)])
    _compare_cars(park, ref, [5], "the car that stays live")                                  # all T rows
    assert park["doneAt"][1] == -1 and park["status"][1] == 0                                  # never stepped
    # a parked car's state stands still: the rows it is stepped for after the crossing are equal too, up to its parking step
    for b in (0, 2, 3, 4):
        for k in ("X", "U", "G"):
            _same(park[k][:want[b], b], ref[k][:want[b], b], ("rows up to the parking step", k, b))
    for k, a in park["trace"].items():
        for j in others:
            n = T if want[j] < 0 else want[j]
            _same(a[:n, j], ref["trace"][k][:n, j], ("trace up to the parking step", k, j))
    # car 5 is live: the run takes all T steps, and n_done keeps its meaning -- the cars that crossed: car 1, parked from step 0, crosses in the reference only
    assert park["t"] == ref["t"] == T and park["n_done"] == ref["n_done"] - 1 == 4


def test_session_ends_when_no_car_is_live(g):
    """Without the car that does not cross, and with the listed car the slowest: the parking session returns at the poll after the last crossing of a live car, the
    reference runs on until car 1 has crossed as well."""
    from racinglmpc_amd import _capi
    inp = _inputs(g, (168, 190, 175, 175, 177))
    out = []
    for park in (None, (_capi.PARK_FINISHED, [1])):
        ctx = _lmpc_ctx(g)
        try:
            out.append(_session(ctx, inp, park))
            if park:
                # every car parked from step 0: begin succeeds, run returns at once with 0 steps
                ctx.rollout_set_parking(0, np.arange(5))
                x0, xl, ul, noise = inp
                ctx.rollout_begin(x0, x0, xl, ul, noise)
                assert ctx.rollout_run(T) == (0, 0) and ctx.rollout_parked_at()[1] == 0 and list(ctx.rollout_parked_at()[0]) == [0] * 5
                ctx.rollout_end()
        finally:
            ctx.close()
    ref, park = out
    d = ref["doneAt"]
    print("doneAt", list(d), "un-parked steps", ref["t"], "parked steps", park["t"])
    assert (d >= 1).all()
    last = max(int(d[b]) for b in (0, 2, 3, 4))
    assert park["t"] == _poll_of(last) and park["n_live"] == 0 and park["n_done"] == 4
    assert ref["t"] > park["t"] and ref["n_done"] == 5 and int(d[1]) > last
    _compare_cars(park, ref, [0, 2, 3, 4], "five cars", upto=d)


@pytest.mark.parametrize("ltv", [True, False], ids=["ltv", "lti"])
def test_plain_mpc_sessions(g, ltv):
    """lmpc_rollout_begin_mpc: the LTV form with stop_at_line and PARK_FINISHED as test 2; the LTI form (all steps: it logs its cars past the crossing) with the
    start list only, where PARK_FINISHED must not act."""
    from racinglmpc_amd import _capi
    from tests.test_gpu_mpc_stages import _mpc_setup
    x0, xl, ul, noise = _inputs(g, K6, steps=T_MPC)
    out = []
    for park in (None, (_capi.PARK_FINISHED, [1])):
        ctx, par, _, form = _mpc_setup(g, 6, ltv)
        try:
            if ltv:
                form = dict(xLin0=xl, uLin0=ul)
            ctx.rollout_set_parking(*(park or (0, None)))
            ctx.rollout_begin_mpc(x0, x0, noise, stop_at_line=ltv, **form)
            t, nd = ctx.rollout_run(T_MPC)
            r = dict(zip(NAMES, ctx.rollout_fetch(0, t))); r.update(t=t, n_done=nd)
            r["parked_at"], r["n_live"] = ctx.rollout_parked_at()
            ctx.rollout_end()
            out.append(r)
        finally:
            ctx.close()
    ref, park = out
    d = ref["doneAt"]
    print("ltv" if ltv else "lti", "doneAt", list(d), "parked_at", list(park["parked_at"]), "steps", ref["t"], park["t"])
    assert d[5] < 0 and sum(d[b] >= 1 for b in (0, 2, 3, 4)) >= 2, list(d)
    if ltv:
        want = [_poll_of(d[b], T_MPC) if d[b] >= 0 else -1 for b in range(6)]; want[1] = 0
        upto = [d[b] if d[b] >= 0 else T_MPC for b in range(6)]
    else:
        want = [-1, 0, -1, -1, -1, -1]; upto = None                   # (every row of every live car)
    assert list(park["parked_at"]) == want, (list(park["parked_at"]), want)
    assert park["t"] == ref["t"] == T_MPC
    _compare_cars(park, ref, [0, 2, 3, 4, 5], "plain MPC", upto=upto)
    _compare_cars(park, ref, [5], "the live car")


def test_ltv_session_ends_when_no_car_is_live(g):
    """Test 2's second case for the LTV form (stop_at_line, PARK_FINISHED, car 1 on the start list and the slowest): the parking session returns at the poll after
    the last crossing of a live car, the reference runs on until car 1 has crossed as well."""
    from racinglmpc_amd import _capi
    from tests.test_gpu_mpc_stages import _mpc_setup
    x0, xl, ul, noise = _inputs(g, (168, 195, 175, 175, 177), steps=T_MPC)
    out = []
    for park in (None, (_capi.PARK_FINISHED, [1])):
        ctx, par, _, form = _mpc_setup(g, 5, True)
        try:
            ctx.rollout_set_parking(*(park or (0, None)))
            ctx.rollout_begin_mpc(x0, x0, noise, stop_at_line=True, xLin0=xl, uLin0=ul)
            t, nd = ctx.rollout_run(T_MPC)
            r = dict(zip(NAMES, ctx.rollout_fetch(0, t))); r.update(t=t, n_done=nd)
            r["parked_at"], r["n_live"] = ctx.rollout_parked_at()
            ctx.rollout_end()
            out.append(r)
        finally:
            ctx.close()
    ref, park = out
    d = ref["doneAt"]
    print("ltv, five cars: doneAt", list(d), "un-parked steps", ref["t"], "parked steps", park["t"])
    assert (d >= 1).all()
    last = max(int(d[b]) for b in (0, 2, 3, 4))
    assert park["t"] == _poll_of(last, T_MPC) and park["n_live"] == 0 and park["n_done"] == 4
    assert ref["t"] > park["t"] and ref["n_done"] == 5 and int(d[1]) > last
    _compare_cars(park, ref, [0, 2, 3, 4], "ltv, five cars", upto=d)


# ---- 3
def test_a_parked_session_is_the_session_of_its_live_cars(g):
    """B = 257, all but cars (0, 100, 256) on the start list.  Without PARK_REROUTE the three cars' rows equal the un-parked B = 257 session's (two waves per QP);
    with it they equal a B = 3 session of the same three cars (four waves per QP)."""
    from racinglmpc_amd import _capi
    B, live, steps = 257, [0, 100, 256], 12
    ks = 170 + (np.arange(B) * 7) % 40
    x0, xl, ul, noise = _inputs(g, ks, steps=steps)
    listed = np.setdiff1d(np.arange(B), live)
    runs = {}
    ctx = _lmpc_ctx(g, max_batch=B)
    try:
        assert ctx.solver_waves(257) == 2 and ctx.solver_waves(3) == 4
        for name, park in (("plain", None), ("kept", (0, listed)), ("reroute", (_capi.PARK_REROUTE, listed))):
            runs[name] = _session(ctx, (x0, xl, ul, noise), park, steps=steps)
        runs["three"] = _session(ctx, (x0[live], xl[live], ul[live], np.ascontiguousarray(noise[:, live])), None, steps=steps)
    finally:
        ctx.close()
    for name in ("kept", "reroute"):
        want = np.zeros(B, np.int32); want[live] = -1
        assert np.array_equal(runs[name]["parked_at"], want) and runs[name]["n_live"] == 3 and runs[name]["t"] == steps
    assert runs["plain"]["t"] == runs["three"]["t"] == steps
    _compare_cars(runs["kept"], runs["plain"], live, "route kept against the un-parked session")
    for j, b in enumerate(live):
        for k in NAMES:
            a, r = runs["reroute"][k], runs["three"][k]
            _same(a[:, b] if a.ndim == 3 else a[b], r[:, j] if r.ndim == 3 else r[j], ("rerouted against the three-car session", k, b))
    assert np.abs(runs["kept"]["U"][:, live]).max() > 1e-3                                     # (not a comparison of zeros)


# ---- 4
def _rows_travel_by_car(g, six, sets):
    """Test 2's session with the per-car row sets named in `sets` in force, parked against un-parked; returns the un-parked run."""
    from racinglmpc_amd import _capi
    from tests import track_cases as tk, tuning_cases
    inp = _inputs(g, K6)
    tune = tuning_cases.rows(tuning_cases.SIX)
    veh = np.tile(_capi.plant_params_default(), (6, 1)); veh[:, 0] *= 1.0 + 0.02 * np.arange(6)
    lt = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 1, 2, 2], [0, 0, 0, 0], [2, 3, 0, 1], [3, 3, 3, 0]], np.int32)
    names = ["L", "L", "oval", "L", "goggle", "L"]
    out = []
    for park in (None, (_capi.PARK_FINISHED, [1])):
        ctx = _lmpc_ctx(g)
        try:
            if "tracks" in sets:
                ctx.track_set(tk.rows_of(names))
            if "tuning" in sets:
                ctx.tuning_set(tune)
            if "vehicle" in sets:
                ctx.plant_set_params(veh)
            if "laps" in sets:
                ctx.model_set_lap_table(lt); ctx.ss_set_lap_table(lt[::-1].copy(), last=np.array([3, -1, 2, 0, 1, 3], np.int32))
            out.append(_session(ctx, inp, park))
        finally:
            ctx.close()
    ref, park = out
    d = ref["doneAt"]
    print("per-car rows", sets, ": doneAt", list(d), "parked_at", list(park["parked_at"]))
    want = [_poll_of(d[b]) if d[b] >= 0 else -1 for b in range(6)]; want[1] = 0
    assert list(park["parked_at"]) == want
    assert len({w for w in want if w > 0}) >= 2 and -1 in want, want         # cars parked at two different polls, and one still live: the grid positions moved twice
    _compare_cars(park, ref, [0, 2, 3, 4, 5], "per-car rows", upto=[d[b] if d[b] >= 0 else T for b in range(6)])
    return ref


def test_per_car_rows_travel_by_car(g, six):
    """Test 2's session with per-car tuning rows, vehicle rows, a lap table, a safe-set table and three tracks in force: parked against un-parked, live cars equal."""
    ref = _rows_travel_by_car(g, six, ("tracks", "tuning", "vehicle", "laps"))
    # and the rows are in force: a car with a row of its own in every set drives differently from test 2's
    assert not np.array_equal(_bits(ref["U"][:3, 2]), _bits(six[1]["U"][:3, 2]))


@pytest.mark.parametrize("one", ["vehicle", "tracks"])
def test_per_car_rows_travel_by_car_one_set(g, six, one):
    """The same with ONE set in force -- vehicle rows only, tracks only: the parked plant kernel with one of its two row flags (the case above sets both, test 2
    neither).  Car 2 has a row of its own in either set (mass x 1.04; the oval): its first steps differ from test 2's, so the rows are in force."""
    ref = _rows_travel_by_car(g, six, (one,))
    assert not np.array_equal(_bits(ref["U"][:3, 2]), _bits(six[1]["U"][:3, 2]))


# ---- 5
def test_runtime_kernel_context(g, six):
    """Test 2's first case on a context served by the runtime-(N, S) kernel: parked against un-parked on that kernel."""
    from racinglmpc_amd import _capi
    inp = six[0]
    out = []
    for park in (None, (_capi.PARK_FINISHED, [1])):
        ctx = _lmpc_ctx(g, runtime=True)
        try:
            assert ctx.solver_kind == 2
            out.append(_session(ctx, inp, park))
        finally:
            ctx.close()
    ref, park = out
    d = ref["doneAt"]
    print("runtime kernel: doneAt", list(d), "parked_at", list(park["parked_at"]))
    want = [_poll_of(d[b]) if d[b] >= 0 else -1 for b in range(6)]; want[1] = 0
    assert list(park["parked_at"]) == want and d[5] < 0 and sum(d[b] >= 1 for b in (0, 2, 3, 4)) == 4
    _compare_cars(park, ref, [0, 2, 3, 4, 5], "runtime kernel", upto=[d[b] if d[b] >= 0 else T for b in range(6)])


# ---- 5b
@pytest.mark.parametrize("B,rpl16", [(6, True), (300, False), (300, True)], ids=["B6-rpl16", "B300", "B300-rpl16"])
def test_regression_kernel_with_the_list_in_every_build(g, B, rpl16):
    """The regression kernel's list instantiations beyond the one-group-per-CU 8-row scan every other parked session here launches: the 16-rows-per-lane scan
    (LMPC_K1_RPL16=1 at create, as tests/test_gpu_configs.py sets it) and, at B = 300 with cars 0..9 on the start list, the occupancy build -- 290 live cars are
    more work-groups than the device has CUs.  9 steps (one poll, at step 8); parked against un-parked on one context, live cars bit for bit."""
    import os
    steps = 9
    if B == 6:
        ks, listed = K6, [1]
    else:
        ks, listed = 170 + (np.arange(B) * 7) % 40, np.arange(10)
    live = np.setdiff1d(np.arange(B), listed)
    inp = _inputs(g, ks, steps=steps)
    if rpl16:
        os.environ["LMPC_K1_RPL16"] = "1"
    try:
        ctx = _lmpc_ctx(g, max_batch=B)
    finally:
        os.environ.pop("LMPC_K1_RPL16", None)
    try:
        # the device's CU count (hipGetDeviceProperties at create) is the largest batch solved with four waves per QP, and what the regression launch compares its grid with
        if B > 6 and ctx.solver_waves(len(live)) == 4:
            pytest.skip("%d live cars do not exceed the device's CUs: the occupancy build would not be launched" % len(live))
        ref = _session(ctx, inp, None, steps=steps)
        park = _session(ctx, inp, (0, listed), steps=steps)
    finally:
        ctx.close()
    want = np.full(B, -1, np.int32); want[listed] = 0
    assert np.array_equal(park["parked_at"], want) and park["n_live"] == len(live) and park["t"] == ref["t"] == steps
    _compare_cars(park, ref, live, "regression kernel with the list")
    assert np.abs(park["U"][:, live]).max() > 1e-3                                             # (not a comparison of zeros)


# ---- 6
def _stores(ctx):
    """Everything the stores hold, as the public entry points show it (as tests/test_gpu_device_commit.py does)."""
    ss = [ctx.store_read_lap(1, l) + (ctx.ss_lap_time(l), ctx.ss_lap_rows(l)) for l in range(ctx.ss_num_laps())]
    nm = ctx.model_num_laps()
    return dict(ss=ss, model=[ctx.store_read_lap(0, p)[:2] for p in range(nm)], info=[ctx.model_lap_info(k) for k in range(nm)],
                image=[ctx.debug_model_image(k) for k in range(nm)])


def _same_stores(a, b, what):
    assert len(a["ss"]) == len(b["ss"]) and len(a["model"]) == len(b["model"]) and a["info"] == b["info"], what
    for l, (p, q) in enumerate(zip(a["ss"], b["ss"])):
        for k in range(3):
            _same(p[k], q[k], (what, "safe set", l, k))
        assert p[3:] == q[3:], (what, l)
    for l, (p, q) in enumerate(zip(a["model"], b["model"])):
        _same(p[0], q[0], (what, "model x", l)); _same(p[1], q[1], (what, "model u", l))
    for l, (p, q) in enumerate(zip(a["image"], b["image"])):
        assert p[2] == q[2], (what, l)
        _same(p[0], q[0], (what, "image words", l)); _same(p[1], q[1], (what, "image parameters", l))


def test_refusals_and_snapshot(g):
    """Every refusal of lmpc_rollout_set_parking with the setting before it intact; a car >= B refused by begin, named, before any session state changes; a `set`
    during a session reaches the next one only; commit and extend beyond a parking step refused, car named; rows = None commits equal the un-parked context's."""
    from racinglmpc_amd import _capi
    F = _capi.PARK_FINISHED
    inp = _inputs(g, K6)
    x0, xl, ul, noise = inp
    ctx = _lmpc_ctx(g, max_laps=32)
    ref = _lmpc_ctx(g, max_laps=32)
    try:
        assert ctx.rollout_parking()[0] == 0 and ctx.rollout_parking()[1].size == 0           # off after create
        ctx.rollout_set_parking(F, [4, 1])
        lib, h = ctx.lib, ctx._h
        cars = lambda *a: np.array(a, np.int32)
        for mode, n, arr in ((4, 0, None), (8 | F, 1, cars(0)), (F, -1, None), (F, 2, None), (F, 2, cars(0, -1)), (F, 3, cars(2, 0, 2))):
            rc = lib.lmpc_rollout_set_parking(h, mode, n, None if arr is None else arr.ctypes.data)
            assert rc == -1, (mode, n, arr)
            mode_now, cars_now = ctx.rollout_parking()
            assert mode_now == F and list(cars_now) == [4, 1]                                  # the setting in force stays
        _refused(E_STATE, lambda: ctx.rollout_parked_at())                                     # no session
        # a listed car the session does not have
        ctx.rollout_set_parking(F, [6])
        msg = _refused(E_ARG, lambda: ctx.rollout_begin(x0, x0, xl, ul, noise))
        assert "car 6" in msg and "B = 6" in msg, msg
        _refused(E_STATE, lambda: ctx.rollout_parked_at())                                     # (no session state changed: none is active)
        # a set during a session reaches the next session only
        ctx.rollout_set_parking(F, [1])
        ctx.rollout_begin(x0, x0, xl, ul, noise)
        ctx.rollout_set_parking(0, [0, 2, 3])
        t, nd = ctx.rollout_run(T)
        at, nl = ctx.rollout_parked_at()
        X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
        assert at[1] == 0 and at[0] == _poll_of(done[0]) and at[5] == -1 and nl == 1 and t == T
        assert ctx.rollout_parking()[0] == 0 and list(ctx.rollout_parking()[1]) == [0, 2, 3]
        # commit / extend beyond a parking step: refused, car named, nothing written
        before = (ctx.ss_num_laps(), ctx.model_num_laps())
        msg = _refused(E_ARG, lambda: ctx.rollout_commit_laps([5, 0], rows=[T, int(at[0]) + 1]))
        assert "car 0" in msg and "parked at step %d" % at[0] in msg, msg
        msg = _refused(E_ARG, lambda: ctx.rollout_commit_laps([1], rows=[2]))
        assert "car 1" in msg, msg
        msg = _refused(E_ARG, lambda: ctx.rollout_extend_laps([5, 0], [0, 1], int(at[0]) + 1))
        assert "car 0" in msg, msg
        assert (ctx.ss_num_laps(), ctx.model_num_laps()) == before
        ok = ctx.rollout_extend_laps([5, 0], [0, 1], int(at[0]))                               # up to the parking step: inside
        assert ok.all()
        ctx.rollout_commit_laps([5, 4], rows=[T, int(at[4])])                                   # explicit rows up to the parking step: inside
        valid = [b for b in (0, 2, 3, 4) if done[b] >= 0]
        ctx.rollout_commit_laps(valid)                                                          # rows = None: up to doneAt, always inside
        ctx.rollout_end()
        # the un-parked context, same calls
        ref.rollout_begin(x0, x0, xl, ul, noise)
        assert ref.rollout_run(T)[0] == T
        rdone = ref.rollout_fetch(0, 0)[3]
        assert list(rdone[[0, 2, 3, 4, 5]]) == list(done[[0, 2, 3, 4, 5]])
        assert ref.rollout_extend_laps([5, 0], [0, 1], int(at[0])).all()
        ref.rollout_commit_laps([5, 4], rows=[T, int(at[4])])
        ref.rollout_commit_laps(valid)
        ref.rollout_end()
        _same_stores(_stores(ctx), _stores(ref), "stores after commits from a parking session")
        # the next session takes the setting made during the last one
        ctx.rollout_begin(x0, x0, xl, ul, noise)
        at2, nl2 = ctx.rollout_parked_at()
        assert list(at2) == [0, -1, 0, 0, -1, -1] and nl2 == 3
        ctx.rollout_end()
    finally:
        ctx.close(); ref.close()


# ---- 7
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device_commit"])
def test_per_car_lmpc_with_parking(g, dev):
    """PerCarLMPC(park=True) against park=False: 6 cars, two generations, car 3 retired in generation 0 by a tuning row that cannot finish (bu = 0 for the
    acceleration: LMPC_ST_NOT_INTERIOR at every step).  Stores, tables, `last`, lap_times and `retired` are equal; generation 1 of the parking loop takes fewer
    session steps than T_max (the loop without parking runs all of them: its retired car never crosses)."""
    from racinglmpc_amd import _capi, rollout
    track = np.array(g["track"]); T_MAX = 400
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=32, max_lap_len=1024)
    vt = np.array([0.75, 0.78, 0.8, 0.82, 0.85, 0.8])
    tune = _capi.tuning_rows(cfg, 6)
    tune[3, -4:] = 0.0                                                    # bu of car 3: u = 0 is not strictly inside Fu u <= bu
    runs = []
    for park in (False, True):
        ctx = _capi.Context(cfg)
        try:
            ro = rollout.BatchedRollouts(ctx, track, seed=5, device_noise=True)
            ro.noise_shard = (0, 6, 6)
            seeds = ro.run_pid_laps(vt, max_steps=700, keep_invalid=True)
            assert all(l[4] >= 0 and l[5] == 0 for l in seeds)
            loop = rollout.PerCarLMPC(ro, T_max=T_MAX, ext=40, device_commit=dev, tuning=tune, park=park)
            loop.seed(seeds)
            outs = [loop.run() for _ in range(2)]
            runs.append(dict(outs=outs, lap_times=[list(t) for t in loop.lap_times], retired=dict(loop.retired), last=loop.last.copy(), steps=list(loop.steps),
                             lap_table=ro.lap_table.copy(), ss_table=ro.ss_table.copy(), ss_last=ro.ss_last.copy(), stores=_stores(ctx),
                             parked_at=None if ro.last_parked_at is None else ro.last_parked_at.copy()))
        finally:
            ctx.close()
    off, on = runs
    print("lap times", off["lap_times"], "retired", off["retired"], "steps without / with parking", off["steps"], on["steps"])
    assert list(off["retired"]) == [3] and off["retired"][3][0] == 0 and off["retired"][3][1] & _capi.ST_NOT_INTERIOR
    assert on["retired"] == off["retired"] and on["lap_times"] == off["lap_times"]
    assert all(len(t) == 2 for b, t in enumerate(off["lap_times"]) if b != 3)
    for k in ("last", "lap_table", "ss_table", "ss_last"):
        assert np.array_equal(on[k], off[k]), k
    _same_stores(on["stores"], off["stores"], "stores with and without parking")
    for gen in range(2):
        for b in range(6):
            a, r = on["outs"][gen][b], off["outs"][gen][b]
            assert (a is None) == (r is None), (gen, b)
            if a is not None:
                assert a[4] == r[4] and a[5] == r[5]
                for j in (0, 1, 3) + (() if dev else (2,)):
                    _same(a[j], r[j], ("lap tuple", gen, b, j))
    assert off["steps"][1] == T_MAX and on["steps"][1] < T_MAX and off["parked_at"] is None
    assert on["parked_at"][3] == 0 and (on["parked_at"] >= 0).all()
