"""-m gpu: queued lmpc_step_batch_dev steps run the regression of step i + 1 on the context's look-ahead stream, beside the solve of step i (lmpc_capi.hip: step_dev).

The same kernels run on the same inputs whether a step is chained or not, so every comparison here is np.array_equal on every key step_dev_fetch returns, A / B / C
included: no tolerance.  The reference of a step is the same step run alone on a fresh context with a sync in front; a second reference is the whole sequence on a
context created under LMPC_K1_AHEAD=0.  Inputs: the N = 12 seed lap of tests/golden/lmpc_n12.npz, batches as bench.synth_batch builds them, another seed and another
row offset per step, so that a step that read another step's hand-over, inputs or status shows.  Shapes: B = 5 on the four-wave route, and the smallest batch that
Context.solver_waves puts on the two-wave and on the one-wave route.

Retry: no fixture raises the deferred retry flag at the default iteration limit; tests/test_gpu_queued_retry.py lowers max_iter and runs queued steps whose launches
are pending their retry pass through every form of this module, with the helpers defined here."""
import contextlib
import os

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

N = 12
N_STEPS = 4


@contextlib.contextmanager
def _knobs(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _inputs(g, B, step):
    """bench.synth_batch with the step's own seed, its rows moved along the lap by 11 rows per step."""
    import bench
    inp = bench.synth_batch(g, B + 11 * step, N, seed=100 + step)
    return {k: np.ascontiguousarray(v[11 * step:]) for k, v in inp.items()}


def _context(g, B, ahead=True, laps=None, **kw):
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=B, **kw)
    with _knobs({} if ahead else {"LMPC_K1_AHEAD": "0"}):
        ctx = _capi.Context(cfg)
    for x, u in (laps if laps is not None else [(np.array(g["xPID"]), np.array(g["uPID"]))] * 4):
        ctx.model_add_trajectory(x, u)
        ctx.ss_add_trajectory(x, u)
    return ctx


def _buffers(ctx, inps, abc):
    """One set of device buffers per step.  abc: "own" (every step its own A / B / C), "shared" (every step the A / B / C of step 0) or "none" (NULL: the
    context's hand-over alone).  Returns ([args], [allocations])."""
    args, keep = [], []
    for inp in inps:
        a, k = ctx.step_dev_buffers(inp)
        args.append(a); keep += k
    for a in args:
        if abc == "shared":
            a.A, a.Bm, a.C = args[0].A, args[0].Bm, args[0].C
        elif abc == "none":
            a.A = None; a.Bm = None; a.C = None
    return args, keep


def _free(ctx, keep):
    for p in keep:
        ctx.dev_free(p)


def _fetch_all(ctx, args, B, abc):
    """Outputs per step.  A / B / C: with shared arrays only the last step's regression is left in them, with none nothing was written: those keys are dropped
    from the steps that cannot show them."""
    outs = []
    for i, a in enumerate(args):
        out = ctx.step_dev_fetch(a, B)
        if abc == "none" or (abc == "shared" and i != len(args) - 1):
            for k in ("A", "B", "C"):
                out.pop(k)
        outs.append(out)
    return outs


def _alone(g, B, inps, laps=None, **kw):
    """Every step run alone, a sync in front, on one fresh context: the references (own A / B / C), and the counter, which must show no chained launch."""
    ctx = _context(g, B, laps=laps, **kw)
    try:
        args, keep = _buffers(ctx, inps, "own")
        outs = []
        for a in args:
            ctx.sync()
            ctx.step_batch_dev(B, a)
            outs.append(ctx.step_dev_fetch(a, B))
        assert ctx.debug_k1_ahead() == (0, len(inps))
        _free(ctx, keep)
    finally:
        ctx.close()
    return outs


def _diff(got, want):
    return [k for k in got if not np.array_equal(got[k], want[k])]


def _route_batches(g):
    """B = 5 (four waves per QP) and the smallest batches on the two-wave and the one-wave route, asked of a context large enough to hold them."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=8192)
    ctx = _capi.Context(cfg)
    try:
        waves = {B: ctx.solver_waves(B) for B in range(1, 8193)}
    finally:
        ctx.close()
    out = [(5, 4)]
    for w in (2, 1):
        Bs = [B for B, v in waves.items() if v == w]
        assert Bs, "no batch up to 8192 runs %d wave(s) per QP" % w
        out.append((min(Bs), w))
    assert waves[5] == 4
    return out


@pytest.fixture(scope="module")
def golden():
    return common.load_lmpc_golden()


@pytest.fixture(scope="module")
def routes(built, golden):
    return _route_batches(golden)


@pytest.fixture(scope="module")
def refs5(built, golden):
    """B = 5: the four steps' inputs and each step's outputs run alone.  Shared by the tests below; never modified."""
    inps = [_inputs(golden, 5, s) for s in range(N_STEPS)]
    return inps, _alone(golden, 5, inps)


@pytest.mark.parametrize("route", [0, 1, 2], ids=["four_waves", "two_waves", "one_wave"])
def test_queued_steps_equal_the_steps_run_alone(built, golden, routes, refs5, route):
    """Parity and ordering: four queued steps with different inputs, each with its own outputs; A / B / C shared by all steps, own per step, or none."""
    g = golden
    B, waves = routes[route]
    inps, alone = refs5 if B == 5 else (None, None)
    if inps is None:
        inps = [_inputs(g, B, s) for s in range(N_STEPS)]
        alone = _alone(g, B, inps)
    assert any(_diff(alone[0], alone[s]) for s in range(1, N_STEPS))           # (the steps really differ)
    fails = []
    for ahead in (True, False):
        for abc in ("shared", "own", "none"):
            ctx = _context(g, B, ahead=ahead)
            try:
                assert ctx.solver_waves(B) == waves
                args, keep = _buffers(ctx, inps, abc)
                ctx.sync()
                c0 = ctx.debug_k1_ahead()
                for a in args:
                    ctx.step_batch_dev(B, a)
                outs = _fetch_all(ctx, args, B, abc)
                c1 = ctx.debug_k1_ahead()
                _free(ctx, keep)
            finally:
                ctx.close()
            what = "B = %d (%d waves), A / B / C %s, %s" % (B, waves, abc, "queued" if ahead else "LMPC_K1_AHEAD=0")
            count = (c1[0] - c0[0], c1[1] - c0[1])
            if count != ((N_STEPS - 1, 1) if ahead else (0, N_STEPS)):
                fails.append("%s: (chained, unchained) regression launches %s" % (what, count))
            for s in range(N_STEPS):
                bad = _diff(outs[s], alone[s])
                if bad:
                    fails.append("%s: step %d: %s differ from the step run alone" % (what, s, ", ".join(bad)))
    assert not fails, "\n".join(fails)


def _break_calls(g, next_args, next_inp):
    """name -> (call on the context between two queued steps, whether it changes what the second step computes)."""
    pid = (np.array(g["xPID"]), np.array(g["uPID"]))
    lap5 = (pid[0][:-30] * np.array([1.02, 1, 1, 1, 1, 1.0]), pid[1][:-30])

    def track_rows(c):
        from racinglmpc_amd import _capi
        return c.track_set(_capi.track_rows([(np.array(g["track"]), float(g["trackLength"]))]))

    def tuning_rows(c):
        from racinglmpc_amd import _capi
        return c.tuning_set(_capi.tuning_rows(c.cfg, 1))
    x = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (2, 1))
    return {
        "model_add_trajectory": lambda c: c.model_add_trajectory(*lap5),
        "ss_add_trajectory": lambda c: c.ss_add_trajectory(*lap5),
        "model_set_lap_table": lambda c: c.model_set_lap_table(np.array([[3, 2, 1, 0]], np.int32)),
        "lmpc_track_set": track_rows,
        "lmpc_tuning_set": tuning_rows,
        "dev_upload": lambda c: c.dev_upload(next_args.xLin, np.ascontiguousarray(next_inp["xLin"])),
        "plant_step_batch": lambda c: c.plant_step_batch(x, x.copy(), np.zeros((2, 2)), np.zeros((2, 3))),
    }


BREAKS = ["model_add_trajectory", "ss_add_trajectory", "model_set_lap_table", "lmpc_track_set", "lmpc_tuning_set", "dev_upload", "plant_step_batch"]


@pytest.mark.parametrize("call", BREAKS)
def test_a_call_between_two_steps_breaks_the_chain(built, golden, refs5, call):
    """Between two queued steps, a call that queues work or edits what the regression reads: the second step runs unchained and equals the serial run -- the same
    calls in the same order with a sync in front of every step."""
    g = golden
    B = 5
    inps = refs5[0][:2]
    outs = {}
    for serial in (True, False):
        ctx = _context(g, B)
        try:
            args, keep = _buffers(ctx, inps, "own")
            if call == "dev_upload":                        # the second step's xLin arrives by the upload: until then its buffer holds the first step's
                ctx.dev_upload(args[1].xLin, np.ascontiguousarray(inps[0]["xLin"]))
            between = _break_calls(g, args[1], inps[1])[call]
            ctx.sync()
            c0 = ctx.debug_k1_ahead()
            ctx.step_batch_dev(B, args[0])
            if serial:
                ctx.sync()
            between(ctx)
            if serial:
                ctx.sync()
            ctx.step_batch_dev(B, args[1])
            outs[serial] = [ctx.step_dev_fetch(a, B) for a in args]
            c1 = ctx.debug_k1_ahead()
            _free(ctx, keep)
        finally:
            ctx.close()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, 2), (call, serial, c0, c1)
    for s in range(2):
        assert not _diff(outs[False][s], outs[True][s]), (call, s, _diff(outs[False][s], outs[True][s]))
    assert not _diff(outs[True][0], refs5[1][0])            # (the first step is the step run alone whatever follows it)


def test_regression_status_stays_with_its_step(built, golden):
    """A step holding the singular queries of tests/golden/reg_singular_capture.npz between two clean steps: its regression-status bits reach its own `status`
    only -- the per-point status goes through the hand-over set of the step, which the neighbours' solves do not read."""
    import bench
    from racinglmpc_amd import _capi
    g = golden
    d = np.load(os.path.join(common.GOLDEN, "reg_singular_capture.npz"))
    assert int(d["N"]) == N
    laps = [(d["lapx%d" % j], d["lapu%d" % j]) for j in range(4)]
    B = d["xLin"].shape[0]
    clean = [bench.synth_batch(g, B, N, seed=7 + s, lap=laps[s]) for s in (0, 1)]
    sing = dict(x0=d["xLin"][:, 0].copy(), xLin=d["xLin"], uLin=d["uLin"], uOld=d["uLin"][:, 0].copy(), zt=d["xLin"][:, N].copy(),
                timeStep=np.zeros(B, np.int32), hasPred=np.zeros(B, np.int32), xPredPrev=np.zeros((B, N + 1, 6)))
    inps = [clean[0], sing, clean[1]]
    alone = _alone(g, B, inps, laps=laps, max_lap_len=512)
    flagged = [(o["status"] & _capi.ST_REG_SINGULAR) != 0 for o in alone]
    assert flagged[1].all() and not flagged[0].any() and not flagged[2].any(), flagged
    ctx = _context(g, B, laps=laps, max_lap_len=512)
    try:
        args, keep = _buffers(ctx, inps, "own")
        ctx.sync()
        for a in args:
            ctx.step_batch_dev(B, a)
        outs = [ctx.step_dev_fetch(a, B) for a in args]
        assert ctx.debug_k1_ahead() == (2, 1)
        _free(ctx, keep)
    finally:
        ctx.close()
    for s in range(3):
        assert not _diff(outs[s], alone[s]), (s, _diff(outs[s], alone[s]))


def test_profiling_times_every_queued_regression(built, golden, refs5):
    g = golden
    inps, alone = refs5
    ctx = _context(g, 5)
    try:
        args, keep = _buffers(ctx, inps, "own")
        ctx.sync()
        ctx.reset_stats(); ctx.set_profiling(1)
        for a in args:
            ctx.step_batch_dev(5, a)
        ctx.sync()
        st = ctx.stats(); ctx.set_profiling(False)
        assert st.n_regress == N_STEPS and st.n_regress_timed == N_STEPS and st.ms_regress > 0
        assert st.n_solve_timed == N_STEPS and st.ms_solve > 0
        assert ctx.debug_k1_ahead() == (N_STEPS - 1, 1)
        for s, a in enumerate(args):
            assert not _diff(ctx.step_dev_fetch(a, 5), alone[s]), s
        _free(ctx, keep)
    finally:
        ctx.close()


def test_pool_and_rollout_after_chained_steps(built, golden, refs5):
    """ContextPool with depth 2: the steps dealt to the members in turn; each step equals the step run alone.  Then a context that ran chained steps runs a
    rollout session and closes."""
    from racinglmpc_amd import _capi
    g = golden
    inps, alone = refs5
    B = 5
    pid = (np.array(g["xPID"]), np.array(g["uPID"]))
    cfg, _ = common.lmpc_config(g, N, max_batch=B)
    pool = _capi.ContextPool(cfg, 2)
    try:
        for _ in range(4):
            pool.model_add_trajectory(*pid); pool.ss_add_trajectory(*pid)
        per_member = [_buffers(m, inps[i::2], "own") for i, m in enumerate(pool.members)]
        for s in range(N_STEPS):
            m = pool.members[s % 2]
            m.step_batch_dev(B, per_member[s % 2][0][s // 2])
        pool.sync()
        for i, m in enumerate(pool.members):
            assert m.debug_k1_ahead() == (0, 2)               # (pool members are created without the look-ahead: measured slower there)
            for j, a in enumerate(per_member[i][0]):
                assert not _diff(m.step_dev_fetch(a, B), alone[i + 2 * j]), (i, j)
            _free(m, per_member[i][1])
    finally:
        pool.close()

    ctx = _context(g, B)
    try:
        args, keep = _buffers(ctx, inps, "own")
        for a in args:
            ctx.step_batch_dev(B, a)
        x0 = inps[0]["x0"]
        ctx.rollout_begin(x0, x0.copy(), inps[0]["xLin"], inps[0]["uLin"], np.zeros((8, B, 3)))
        steps, _ = ctx.rollout_run(4)
        assert steps == 4
        ctx.rollout_end()
        assert ctx.debug_k1_ahead() == (N_STEPS - 1, 1)
        for s, a in enumerate(args):
            assert not _diff(ctx.step_dev_fetch(a, B), alone[s]), s
        _free(ctx, keep)
    finally:
        ctx.close()
