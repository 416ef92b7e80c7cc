"""-m gpu: queued lmpc_step_batch_dev steps on the plain four-wave route hold their solve for the next call, which launches it in ONE launch with its own regression
(the two-role build of lmpc_solve_kernel_mw; lmpc_capi.hip: step_dev, launch_held, ctx_enter).

Every comparison is np.array_equal on every key step_dev_fetch returns (bench.DUMP_KEYS, A / B / C, status and iters among them) against a second context created
with the merged form off (Context(k1_merge=False), LMPC_CREATE_NO_K1_MERGE) that is given the same inputs and the same calls in the same order: no tolerance.  The
per-point regression status is a hand-over array of the context's; what a caller sees of it is its OR in `status`, which is compared.

The rule the counters follow (Context.debug_k1_merge: two-role launches, held solves launched stand-alone, regressions in a kernel of their own).  A step is
eligible when the call before it was a step_dev with nothing queued or edited since, its batch runs four waves per QP at up to one QP per CU, no lap / safe-set
table, tuning or track rows are in force, it brings its own A / Bm / C, and profiling is not 1.  The first step of a chain is never eligible: regression and solve
in kernels of their own.  An eligible step with no solve held launches its regression alone and holds its solve; an eligible step with a solve held launches ONE
two-role kernel and holds its solve.  Every other entry point, and a step that is not eligible, launches a held solve stand-alone first (a flush); a step behind a
flush is the first of a new chain.  Five queued eligible steps and a sync: (3, 1, 2).

Shapes: batches 1, 2, 3; (N, S) = (12, 48), (14, 48) -- 14 queries in work-groups of 3: the last one of a problem is partial --, (8, 0) plain MPC, and the variant
library (10, 48)."""
import contextlib
import os

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

SHAPES = [(12, 48), (14, 48), (8, 0), (10, 48)]


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


def _inputs(g, N, B, step, lap=None):
    """bench.synth_batch with the step's own seed, its rows moved along the lap by 11 rows per step."""
    import bench
    inp = bench.synth_batch(g, B + 11 * step, N, seed=100 + step, lap=lap)
    return {k: np.ascontiguousarray(v[11 * step:]) for k, v in inp.items()}


def _context(g, N, S, max_batch, merge, laps=None, knobs=None, **kw):
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=max_batch, **kw) if S else common.mpc_config(g, N, max_batch=max_batch, **kw)
    with _knobs(knobs or {}):
        ctx = _capi.Context(cfg, k1_merge=merge)
    assert ctx.S == S
    for x, u in (laps if laps is not None else [(np.array(g["xPID"]), np.array(g["uPID"]))] * (4 if S else 1)):
        ctx.model_add_trajectory(x, u)
        if S:
            ctx.ss_add_trajectory(x, u)
    return ctx


def _buffers(ctx, inp):
    """step_dev_buffers with every output array set to a fixed pattern first.  The allocations come uninitialised, and a plain MPC step (S = 0) writes no sTerm: what
    a step leaves alone then compares equal between two contexts, and a step that wrote where it should not shows against the pattern."""
    from racinglmpc_amd import _capi
    a, keep = ctx.step_dev_buffers(inp)
    B = np.asarray(inp["x0"]).shape[0]
    for k, (shp, dt) in _capi.array_specs(B, ctx.N, ctx.S, ctx.cfg.numSS_it, _capi.STEP_OUT_KEYS).items():
        if int(np.prod(shp)):
            ctx.dev_upload(getattr(a, _capi._FIELD[k]), np.full(shp, -7 if np.dtype(dt).kind == "i" else -1234.5, dtype=dt))
    return a, keep


def _play(ctx, inps, script, no_abc=()):
    """Buffers for every step of `inps` (own outputs, own A / B / C; steps in no_abc: NULL A / Bm / C), a sync, then `script`: an int queues that step, a callable
    is called with (ctx, args).  Returns (outputs per step, counters since the sync, n_retry)."""
    args, keep = [], []
    for i, inp in enumerate(inps):
        a, k = _buffers(ctx, inp)
        if i in no_abc:
            a.A = None; a.Bm = None; a.C = None
        args.append(a); keep += k
    ctx.sync(); ctx.reset_stats()
    c0 = ctx.debug_k1_merge()
    for op in script:
        if callable(op):
            op(ctx, args)
        else:
            ctx.step_batch_dev(inps[op]["x0"].shape[0], args[op])
    outs = []
    for i, a in enumerate(args):
        out = ctx.step_dev_fetch(a, inps[i]["x0"].shape[0])
        if i in no_abc:
            for k in ("A", "B", "C"):
                out.pop(k)
        outs.append(out)
    c1 = ctx.debug_k1_merge()
    n_retry = ctx.stats().n_retry
    for p in keep:
        ctx.dev_free(p)
    return outs, tuple(b - a for a, b in zip(c0, c1)), n_retry


def _both(g, N, S, max_batch, inps, script, **kw):
    """`script` on a merged-form context and on one without: ((outputs, counters, n_retry) merged, the same without)."""
    no_abc = kw.pop("no_abc", ())
    res = []
    for merge in (True, False):
        ctx = _context(g, N, S, max_batch, merge, **kw)
        try:
            res.append(_play(ctx, inps, script, no_abc))
        finally:
            ctx.close()
    assert res[1][1][0] == 0 and res[1][1][1] == 0, res[1][1]          # (the reference context never holds a solve)
    return res


def _assert_same(got, want, what):
    import bench
    bad = []
    for s, (o, r) in enumerate(zip(got, want)):
        assert set(bench.DUMP_KEYS) - {"A", "B", "C"} <= set(o) and {"status", "iters"} <= set(o)
        bad += ["step %d: %s" % (s, k) for k in o if not np.array_equal(o[k], r[k])]
    assert not bad, "%s: differ from the context without the merged form: %s" % (what, ", ".join(bad))


@pytest.fixture(scope="module")
def golden():
    return common.load_lmpc_golden()


@pytest.mark.parametrize("N,S,B", [(N, S, 3) for N, S in SHAPES] + [(12, 48, 1), (12, 48, 2)], ids=lambda v: str(v))
def test_five_queued_steps(built, golden, N, S, B):
    """Five queued steps with different inputs and outputs per step, then a sync: every output of every step, and the counters of the rule above."""
    inps = [_inputs(golden, N, B, s) for s in range(5)]
    (outs, count, n_retry), (ref, rcount, _) = _both(golden, N, S, B, inps, [0, 1, 2, 3, 4])
    assert any(not np.array_equal(ref[0]["xPred"], ref[s]["xPred"]) for s in range(1, 5))           # (the steps really differ)
    assert all((o["status"] == 0).all() for o in ref)
    if S == 0:                                                               # (no terminal set: the step leaves sTerm as it found it)
        assert all((o["sTerm"] == -1234.5).all() for o in outs + ref)
    _assert_same(outs, ref, "N = %d, S = %d, B = %d" % (N, S, B))
    assert count == (3, 1, 2) and rcount == (0, 0, 5) and n_retry == 0, (count, rcount, n_retry)


def _flush_calls(g):
    """name -> call on the context between two queued steps, a solve being held when it comes."""
    pid = (np.array(g["xPID"]), np.array(g["uPID"]))
    lap5 = (pid[0][:-30] * np.array([1.02, 1, 1, 1, 1, 1.0]), pid[1][:-30])
    seen = {}

    def download(c, args):
        seen["xPred"] = c.dev_download(args[2].xPred, np.zeros((3, 13, 6)))          # the held step's own output: its solve is launched, then the drain

    def lap_table(c, args):
        c.model_set_lap_table(np.array([[3, 2, 1, 0]], np.int32)); c.model_set_lap_table(None)

    return {"sync": lambda c, a: c.sync(), "dev_download": download, "ss_add_trajectory": lambda c, a: c.ss_add_trajectory(*lap5),
            "model_add_trajectory": lambda c, a: c.model_add_trajectory(*lap5), "lap_table_set_and_cleared": lap_table,
            "set_profiling": lambda c, a: c.set_profiling(5), "flush": lambda c, a: c.flush()}, seen


@pytest.mark.parametrize("call", ["sync", "dev_download", "ss_add_trajectory", "model_add_trajectory", "lap_table_set_and_cleared", "set_profiling", "flush"])
def test_every_other_entry_point_launches_the_held_solve_first(built, golden, call):
    """Steps 0, 1, 2, the call, steps 3, 4, a sync.  Step 2's solve is held when the call comes and must have run on the stores of before it: all five steps equal
    the context without the merged form given the same calls.  One two-role launch (step 2 carrying solve 1), two flushes (the call, the final sync), four
    regressions alone (steps 0, 1 and -- a new chain -- 3, 4)."""
    g = golden
    inps = [_inputs(g, 12, 3, s) for s in range(5)]
    calls, seen = _flush_calls(g)
    between = calls[call]
    res = []
    for merge in (True, False):
        ctx = _context(g, 12, 48, 3, merge)
        try:
            res.append(_play(ctx, inps, [0, 1, 2, between, 3, 4]))
            res[-1] += (seen.get("xPred"),)
            ctx.set_profiling(False)
        finally:
            ctx.close()
    _assert_same(res[0][0], res[1][0], call)
    assert res[0][1] == (1, 2, 4) and res[1][1] == (0, 0, 5), (call, res[0][1], res[1][1])
    if call == "dev_download":
        assert np.array_equal(res[0][3], res[0][0][2]["xPred"]) and np.array_equal(res[1][3], res[0][3])
    if call in ("ss_add_trajectory", "model_add_trajectory"):
        fresh = _inputs(g, 12, 3, 2)
        assert np.array_equal(fresh["x0"], inps[2]["x0"])                  # (inputs are what they were: only the stores moved)


def test_batch_size_changes_inside_a_chain(built, golden):
    """B = 3, 2, 3, 2, 3 in one chain: a two-role launch whose solve and regression roles serve different batch sizes."""
    inps = [_inputs(golden, 12, B, s) for s, B in enumerate([3, 2, 3, 2, 3])]
    (outs, count, _), (ref, _, _) = _both(golden, 12, 48, 3, inps, [0, 1, 2, 3, 4])
    _assert_same(outs, ref, "B = 3, 2, 3, 2, 3")
    assert count == (3, 1, 2), count


def test_a_step_without_its_own_abc_drains_as_before(built, golden):
    """Step 2 hands over through the context's own A / Bm / C: not eligible.  The held solve of step 1 is launched alone, step 2 runs as the first step of a chain;
    steps 3 and 4 chain again: one two-role launch (step 4 carrying solve 3), two flushes (step 2, the final sync), four regressions alone (0, 1, 2, 3)."""
    inps = [_inputs(golden, 12, 3, s) for s in range(5)]
    (outs, count, _), (ref, _, _) = _both(golden, 12, 48, 3, inps, [0, 1, 2, 3, 4], no_abc=(2,))
    _assert_same(outs, ref, "NULL A / Bm / C at step 2")
    assert count == (1, 2, 4), count


def test_a_one_wave_batch_inside_a_chain(built, golden):
    """LMPC_MW_MAX_BATCH=2 at lmpc_create puts B = 3 on the one-wave route (tests/test_gpu_routes.py forces routes this way); B = 2, 2, 3, 2, 2: the one-wave
    step launches the held solve alone and runs as before; same counters as the step without its own A / Bm / C."""
    from racinglmpc_amd import _capi
    knobs = {"LMPC_MW_MAX_BATCH": "2"}
    inps = [_inputs(golden, 12, B, s) for s, B in enumerate([2, 2, 3, 2, 2])]
    ctx = _context(golden, 12, 48, 3, True, knobs=knobs)
    try:
        assert ctx.solver_waves(2) == 4 and ctx.solver_waves(3) == 1
    finally:
        ctx.close()
    (outs, count, _), (ref, _, _) = _both(golden, 12, 48, 3, inps, [0, 1, 2, 3, 4], knobs=knobs)
    _assert_same(outs, ref, "B = 3 on one wave per QP at step 2")
    assert count == (1, 2, 4), count
    assert "LMPC_MW_MAX_BATCH=2" in _capi.active_knobs() if hasattr(_capi, "active_knobs") else True


def test_regression_status_comes_through_a_two_role_launch(built, golden):
    """The singular queries of tests/golden/reg_singular_capture.npz at steps 1 and 3 of clean, singular, clean, singular: step 1's regression runs in a kernel of
    its own, step 3's inside a two-role launch; LMPC_ST_REG_SINGULAR reaches the status of both, and of no clean step."""
    import bench
    from racinglmpc_amd import _capi
    g = golden
    d = np.load(os.path.join(common.GOLDEN, "reg_singular_capture.npz"))
    assert int(d["N"]) == 12
    laps = [(d["lapx%d" % j], d["lapu%d" % j]) for j in range(4)]
    B = min(d["xLin"].shape[0], 2)
    xl, ul = d["xLin"][:B], d["uLin"][:B]
    sing = dict(x0=xl[:, 0].copy(), xLin=xl, uLin=ul, uOld=ul[:, 0].copy(), zt=xl[:, 12].copy(), timeStep=np.zeros(B, np.int32), hasPred=np.zeros(B, np.int32),
                xPredPrev=np.zeros((B, 13, 6)))
    inps = [bench.synth_batch(g, B, 12, seed=7, lap=laps[0]), sing, bench.synth_batch(g, B, 12, seed=8, lap=laps[1]), sing]
    (outs, count, _), (ref, _, _) = _both(g, 12, 48, B, inps, [0, 1, 2, 3], laps=laps, max_lap_len=512)
    _assert_same(outs, ref, "singular regression")
    assert count == (2, 1, 2), count
    flagged = [(o["status"] & _capi.ST_REG_SINGULAR) != 0 for o in outs]
    assert flagged[1].all() and flagged[3].all() and not flagged[0].any() and not flagged[2].any(), flagged


def test_the_same_arrays_on_every_step(built, golden):
    """The benchmark's pattern: one set of arrays, queued ten times.  The outputs equal those of the step run once; no retry pass."""
    g = golden
    inp = _inputs(g, 12, 3, 0)
    ctx = _context(g, 12, 48, 3, True)
    try:
        a, keep = _buffers(ctx, inp)
        ctx.sync(); ctx.reset_stats()
        ctx.step_batch_dev(3, a)
        once = ctx.step_dev_fetch(a, 3)
        c0 = ctx.debug_k1_merge()
        for _ in range(10):
            ctx.step_batch_dev(3, a)
        ten = ctx.step_dev_fetch(a, 3)
        c1 = ctx.debug_k1_merge()
        assert [k for k in once if not np.array_equal(once[k], ten[k])] == []
        assert tuple(y - x for x, y in zip(c0, c1)) == (8, 1, 2) and ctx.stats().n_retry == 0
        for p in keep:
            ctx.dev_free(p)
    finally:
        ctx.close()


def test_destroy_drops_a_held_solve(built, golden):
    """close() on a context that holds a solve returns (the solve is dropped, not launched; its outputs are not examined), and a fresh context works."""
    g = golden
    inps = [_inputs(g, 12, 3, s) for s in range(3)]
    ctx = _context(g, 12, 48, 3, True)
    args = [ctx.step_dev_buffers(inp)[0] for inp in inps]
    ctx.sync()
    for a in args:
        ctx.step_batch_dev(3, a)
    assert ctx.debug_k1_merge()[0] == 1                                     # (solve 2 is held now)
    ctx.close()
    (outs, count, _), (ref, _, _) = _both(g, 12, 48, 3, inps, [0, 1, 2])
    _assert_same(outs, ref, "fresh context")
    assert count == (1, 1, 2), count
