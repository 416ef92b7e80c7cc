"""-m gpu: the deferred retry pass (lmpc_capi.hip: resolve_retries) behind queued lmpc_step_batch_dev steps in every form a step can take -- the step of before
(LMPC_K1_AHEAD=0), the two-stream look-ahead (LMPC_K1_MERGE=0), the held solve and the two-role launch (step_dev, launch_solve, launch_held).  A retry pass runs at the
next drain and must run against the data of ITS launch: the parameter block of its call, the caller's A / Bm / C (not the hand-over set the first pass read, which the
step after next overwrites), the status word of its own first pass, and the lap stores as they were at the launch.

Set-up: N = 12, the seed lap of tests/golden/lmpc_n12.npz four times in both stores, max_iter = 7 (the way tests/test_gpu_retry.py makes a first pass raise the flag).
Every step has its own seed and row offset (test_gpu_k1_ahead._inputs): a retry pass that read anything of another step gives other bits.  The reference of a step
is the same step run alone on a fresh max_iter = 7 context with a sync in front (_alone_counted: test_gpu_k1_ahead._alone, which also reports whether the step's
launch asked for its retry pass -- the change of stats().n_retry over the step).  The same kernels run on the same inputs, so every comparison is np.array_equal on
every key step_dev_fetch returns, status and iters included: no tolerance.

Batch: B_MAIN = 8, found on the device from the alone runs: the smallest B <= 64 on the four-wave route at which every flagged step of the main sequence (steps
0, 1, 2 and 4) has a problem that ends with LMPC_ST_MAXITER and one that ends with status 0 (step 0 and step 2 have their first status-0 problem in row 7).
The step at position FREE_AT raises no flag at all -- its alone run launches no retry pass -- so that n_retry must count the flagged steps, not the steps.  No
seed gives such a step through _inputs as it is: a quarter of the problems converges within 7 iterations, and of the seeds 100 .. 123 none has even two such
problems in front.  So the free step keeps step 3's seed and row offset and takes, of its first 64 rows, the first eight that converge within the limit
(FREE_ROWS).  The module fixture asserts all of this, and the anchor: the status-0 problems of every alone reference agree with the same step on a default
(max_iter = 40) context -- what the oracle tests pin -- within 1e-6 on xPred (the bound of tests/test_gpu_retry.py).  The two-wave and the one-wave batch run the
steps 0 .. 4 as _inputs gives them; every one of them is flagged there.

A given, Bm and C NULL: the Python wrapper passes the pointers on as they are, so the case runs (test_every_queueing_form, "partial")."""
import os

import numpy as np
import pytest

from tests import common
from tests.test_gpu_k1_ahead import N, _buffers, _context, _diff, _fetch_all, _free, _inputs, _knobs, _route_batches

pytestmark = pytest.mark.gpu

MAX_ITER = 7
B_MAIN = 8
STEPS = (0, 1, 2, 3, 4)       # the step numbers (seed 100 + s, rows moved by 11 s) of a five-step sequence
FREE_AT = 3                   # the position of the main sequence whose step raises no flag:
FREE_ROWS = (13, 16, 19, 21, 22, 25, 32, 42)      # these rows of step 3 at B = 64, the first B_MAIN of it that converge within MAX_ITER
SING_MAX_ITER = 7             # the limit at which a problem of the singular step carries LMPC_ST_REG_SINGULAR and LMPC_ST_MAXITER together
RING = 64                     # LMPC_RETRY_RING (lmpc_capi.hip)

# how a context queues its steps: the knobs at lmpc_create, and what five queued steps with their own A / Bm / C leave in (debug_k1_ahead, debug_k1_merge) --
# the counts tests/test_gpu_k1_ahead.py and tests/test_gpu_merged_step.py assert for the same call sequences
FORMS = {"merged": {}, "two_stream": {"LMPC_K1_MERGE": "0"}, "no_ahead": {"LMPC_K1_AHEAD": "0"}}


def _counts(form, n, eligible=True):
    """((chained, unchained) regressions, (two-role launches, held solves launched alone, regressions in a kernel of their own)) after n queued steps and a drain.
    eligible: the steps may hold their solve (four waves, own A / Bm / C)."""
    if form == "no_ahead":
        return (0, n), (0, 0, n)
    if form == "merged" and eligible:
        return (n - 1, 1), (n - 2, 1, 2)
    return (n - 1, 1), (0, 0, n)


def _ctx(g, B, form="merged", laps=None, max_iter=MAX_ITER, **kw):
    with _knobs(FORMS[form]):
        return _context(g, B, laps=laps, max_iter=max_iter, **kw)


def _alone_counted(g, B, inps, laps=None, prepare=None, **kw):
    """Every step run alone, a sync in front, on one fresh context (prepare(ctx) first).  Returns ([outputs], [retry passes the step's launch asked for: 0 or 1])."""
    ctx = _ctx(g, B, laps=laps, **kw)
    try:
        if prepare is not None:
            prepare(ctx)
        args, keep = _buffers(ctx, inps, "own")
        outs, asked = [], []
        for a in args:
            ctx.sync()
            n0 = ctx.stats().n_retry
            ctx.step_batch_dev(B, a)
            outs.append(ctx.step_dev_fetch(a, B))
            asked.append(ctx.stats().n_retry - n0)
        assert ctx.debug_k1_ahead() == (0, len(inps))
        ctx.set_profiling(False)
        _free(ctx, keep)
    finally:
        ctx.close()
    return outs, asked


def _queued(ctx, B, inps, abc="own", between=None):
    """The steps queued back to back (between: {i: call(ctx, args) in front of step i}), then fetched.  abc as test_gpu_k1_ahead._buffers takes it, or "partial":
    the caller's A, Bm and C NULL.  Returns (outputs per step, change of debug_k1_ahead, of debug_k1_merge, of n_retry)."""
    args, keep = _buffers(ctx, inps, "own" if abc == "partial" else abc)
    if abc == "partial":
        for a in args:
            a.Bm = None; a.C = None
    ctx.sync()
    a0, m0, r0 = ctx.debug_k1_ahead(), ctx.debug_k1_merge(), ctx.stats().n_retry
    for i, a in enumerate(args):
        if between and i in between:
            between[i](ctx, args)
        ctx.step_batch_dev(B, a)
    outs = _fetch_all(ctx, args, B, "own" if abc == "partial" else abc)
    if abc == "partial":
        for o in outs:
            o.pop("B"); o.pop("C")
    a1, m1, r1 = ctx.debug_k1_ahead(), ctx.debug_k1_merge(), ctx.stats().n_retry
    ctx.set_profiling(False)
    _free(ctx, keep)
    return outs, tuple(y - x for x, y in zip(a0, a1)), tuple(y - x for x, y in zip(m0, m1)), r1 - r0


def _maxiter(out):
    from racinglmpc_amd import _capi
    return (out["status"] & _capi.ST_MAXITER) != 0


def _mismatches(outs, refs, what):
    return ["%s: step %d: %s differ from the step run alone" % (what, s, ", ".join(_diff(o, r))) for s, (o, r) in enumerate(zip(outs, refs)) if _diff(o, r)]


class _Refs:
    """The inputs of a sequence, every step's outputs run alone and whether its launch asked for the retry pass.  Shared by the tests; never modified."""

    def __init__(self, g, B, inps, free=None):
        self.B = B
        self.inps = inps
        steps = range(len(inps))
        self.outs, self.asked = _alone_counted(g, B, self.inps)
        default, _ = _alone_counted(g, B, self.inps, max_iter=40)
        for s, o, d, n in zip(steps, self.outs, default, self.asked):
            hit, clean = _maxiter(o), o["status"] == 0
            print("B = %d step %d: %d at the limit, %d clean, retry passes %d, iterations %d .. %d" % (B, s, hit.sum(), clean.sum(), n, o["iters"].min(), o["iters"].max()))
            if s == free:
                assert n == 0 and clean.all(), (B, s, n, o["status"])
            else:
                assert n == 1 and hit.any() and clean.any(), (B, s, n, o["status"])
            assert (d["status"] == 0).all(), (B, s, d["status"])
            err = np.abs(o["xPred"][clean] - d["xPred"][clean]).max()
            print("    clean problems against max_iter = 40: |xPred| differs by %.3e" % err)
            assert err < 1e-6, (B, s, err)
        assert any(_diff(self.outs[0], o) for o in self.outs[1:])              # (the steps really differ)


@pytest.fixture(scope="module")
def golden():
    return common.load_lmpc_golden()


@pytest.fixture(scope="module")
def main(built, golden):
    """B_MAIN: STEPS alone; the fixture assertions of the module docstring."""
    ctx = _ctx(golden, B_MAIN)
    try:
        assert ctx.solver_waves(B_MAIN) == 4
    finally:
        ctx.close()
    inps = [_inputs(golden, B_MAIN, s) for s in STEPS]
    assert len(FREE_ROWS) == B_MAIN
    inps[FREE_AT] = {k: np.ascontiguousarray(v[list(FREE_ROWS)]) for k, v in _inputs(golden, 64, STEPS[FREE_AT]).items()}
    return _Refs(golden, B_MAIN, inps, FREE_AT)


@pytest.fixture(scope="module")
def routes(built, golden):
    """(B, waves) of the smallest two-wave and the smallest one-wave batch."""
    return _route_batches(golden)[1:]


CASES = [("merged", "own", 4), ("two_stream", "own", 4), ("no_ahead", "own", 4), ("merged", "own", 2), ("merged", "own", 1), ("merged", "none", 4), ("merged", "partial", 4),
         ("two_stream", "none", 4), ("two_stream", "partial", 4)]


@pytest.mark.parametrize("form,abc,waves", CASES, ids=["%s-%s-%dw" % c for c in CASES])
def test_every_queueing_form(built, golden, main, routes, form, abc, waves):
    """Five queued steps: bit equality per step with the step run alone, n_retry grown by the number of flagged steps, and the counters of the intended form.
    "none": NULL A / Bm / C, a drain at every step.  "partial": A the caller's, Bm and C hand-over arrays -- retry_abc mixes them, shared_abc forces the drain."""
    g = golden
    B = B_MAIN if waves == 4 else dict((w, B) for B, w in routes)[waves]
    refs = main if waves == 4 else _Refs(g, B, [_inputs(g, B, s) for s in STEPS])
    ctx = _ctx(g, B, form)
    try:
        assert ctx.solver_waves(B) == waves
        outs, ahead, merge, n_retry = _queued(ctx, B, refs.inps, abc)
    finally:
        ctx.close()
    what = "%s, A / B / C %s, B = %d (%d waves)" % (form, abc, B, waves)
    print("%s: debug_k1_ahead +%s, debug_k1_merge +%s, n_retry +%d" % (what, ahead, merge, n_retry))
    keys = {"own": (), "none": ("A", "B", "C"), "partial": ("B", "C")}[abc]
    want = [{k: v for k, v in r.items() if k not in keys} for r in refs.outs]
    bad = _mismatches(outs, want, what)
    assert not bad, "\n".join(bad)
    assert n_retry == sum(refs.asked), (what, n_retry, refs.asked)
    assert (ahead, merge) == _counts(form, len(refs.inps), eligible=abc == "own" and waves == 4), (what, ahead, merge)


@pytest.mark.parametrize("form", ["merged", "two_stream"])
def test_ring_wrap_inside_a_chain(built, golden, main, form):
    """70 queued flagged steps, more than the retry ring has slots: launch_held / launch_solve resolve the pending launches in the middle of the chain.  The steps
    cycle through the four flagged input sets of the main sequence, each step with its own outputs and A / Bm / C."""
    g = golden
    sets = [i for i in range(len(STEPS)) if i != FREE_AT]
    assert len(sets) == 4 and all(main.asked[i] == 1 for i in sets)
    n = RING + 6
    order = [sets[i % 4] for i in range(n)]
    ctx = _ctx(g, B_MAIN, form)
    try:
        outs, ahead, merge, n_retry = _queued(ctx, B_MAIN, [main.inps[i] for i in order])
    finally:
        ctx.close()
    print("%s, %d steps: debug_k1_ahead +%s, debug_k1_merge +%s, n_retry +%d" % (form, n, ahead, merge, n_retry))
    bad = _mismatches(outs, [main.outs[i] for i in order], form)
    assert not bad, "\n".join(bad)
    assert n_retry == n, (form, n_retry)
    assert (ahead, merge) == _counts(form, n), (form, ahead, merge)


def _retain_laps(g):
    """Five laps for the store_retain case: lap k is the seed lap without its last 10 k rows, so lap 4 is the fastest and among the four the steps select."""
    x, u = np.array(g["xPID"]), np.array(g["uPID"])
    return [(x[:x.shape[0] - 10 * k], u[:u.shape[0] - 10 * k]) for k in range(5)]


def _between_calls(g, B, inps):
    """({name: (call(ctx, args) between steps 1 and 2, the call that brings a fresh context to the state step 2 then finds (or None), the laps of the context
    (None: the seed lap four times))}, what dev_download returned)."""
    from racinglmpc_amd import _capi
    pid = (np.array(g["xPID"]), np.array(g["uPID"]))
    lap5 = (pid[0][:-30] * np.array([1.3, 1, 1, 1, 1, 1.0]), pid[1][:-30])       # the faster fifth lap of tests/test_gpu_retry.py: would change a late retry's selection
    seen = {}

    def lap_table(c, a=None):
        c.model_set_lap_table(np.array([[3, 2, 1, 0]], np.int32)); c.model_set_lap_table(None)

    def retain(c, a=None):
        assert 4 in np.argsort([c.ss_lap_time(l) for l in range(5)], kind="stable")[:4]          # (steps 0 and 1 selected the lap that goes)
        ms, mm = c.store_retain(ss=[0, 1, 2, 3], model=[0, 1, 2, 3])
        assert ms.tolist() == [0, 1, 2, 3, -1] and mm.tolist() == [0, 1, 2, 3, -1]

    def download(c, a):
        seen["xPred"] = c.dev_download(a[1].xPred, np.zeros((B, N + 1, 6)))

    ss_add = lambda c, a=None: c.ss_add_trajectory(*lap5)
    model_add = lambda c, a=None: c.model_add_trajectory(*lap5)
    tuning = lambda c, a=None: c.tuning_set(_capi.tuning_rows(c.cfg, 1))
    track = lambda c, a=None: c.track_set(_capi.track_rows([(np.array(g["track"]), float(g["trackLength"]))]))
    profiling = lambda c, a=None: c.set_profiling(1)
    return {
        "ss_add_trajectory": (ss_add, ss_add, None),
        "model_add_trajectory": (model_add, model_add, None),
        "model_set_lap_table_set_and_cleared": (lap_table, None, None),
        "tuning_set": (tuning, tuning, None),
        "track_set": (track, track, None),
        "store_retain": (retain, retain, _retain_laps(g)),
        "dev_upload": (lambda c, a: c.dev_upload(a[1].x0, np.ascontiguousarray(inps[2]["x0"])), None, None),      # step 1's x0 overwritten with step 2's
        "dev_download": (download, None, None),
        "flush": (lambda c, a: c.flush(), None, None),
        "set_profiling_1": (profiling, profiling, None),
    }, seen


BETWEEN = ["ss_add_trajectory", "model_add_trajectory", "model_set_lap_table_set_and_cleared", "tuning_set", "track_set", "store_retain", "dev_upload", "dev_download",
           "flush", "set_profiling_1"]


@pytest.fixture(scope="module")
def after_call(built, golden, main):
    """Per call of BETWEEN: (references of steps 0 and 1 and their retry passes, reference of step 2 on a fresh context brought to the state behind the call, its
    retry passes).  Computed once, shared by the two forms."""
    cache = {}

    def get(call):
        if call not in cache:
            g = golden
            inps = main.inps[:3]
            _, state, laps = _between_calls(g, B_MAIN, inps)[0][call]
            if laps is None:
                first, asked = main.outs[:2], main.asked[:2]
            else:
                first, asked = _alone_counted(g, B_MAIN, inps[:2], laps=laps)
                assert all(_maxiter(o).any() for o in first) and asked == [1, 1], (call, asked)
            if state is None and laps is None:
                last, asked2 = main.outs[2:3], main.asked[2:3]
            else:
                last, asked2 = _alone_counted(g, B_MAIN, inps[2:3], laps=laps, prepare=state)
            cache[call] = (first, asked, last[0], asked2[0])
        return cache[call]
    return get


@pytest.mark.parametrize("form", ["merged", "two_stream"])
@pytest.mark.parametrize("call", BETWEEN)
def test_a_call_between_queued_flagged_steps(built, golden, main, after_call, call, form):
    """Step 0, step 1 (a held solve and / or pending launches are left), the call, step 2, fetch: steps 0 and 1 equal their alone references of before the call,
    step 2 a fresh context brought to the same state and stepped alone."""
    g = golden
    inps = main.inps[:3]
    assert FREE_AT > 2
    calls, seen = _between_calls(g, B_MAIN, inps)
    between, _, laps = calls[call]
    first, asked, last, asked2 = after_call(call)
    ctx = _ctx(g, B_MAIN, form, laps=laps)
    try:
        outs, _, merge, n_retry = _queued(ctx, B_MAIN, inps, between={2: between})
    finally:
        ctx.close()
    bad = _mismatches(outs, first + [last], "%s, %s" % (form, call))
    assert not bad, "\n".join(bad)
    assert n_retry == sum(asked) + asked2, (form, call, n_retry, asked, asked2)
    if form == "merged":
        assert merge[1] >= 1, merge                                          # (step 1's solve was held when the call came)
    if call == "dev_download":
        assert np.array_equal(seen["xPred"], first[1]["xPred"])


def _singular_sequence(g):
    """The singular queries of tests/golden/reg_singular_capture.npz and four clean steps on its laps (test_gpu_k1_ahead: test_regression_status_stays_with_its_step)."""
    import bench
    d = np.load(os.path.join(common.GOLDEN, "reg_singular_capture.npz"))
    assert int(d["N"]) == N
    laps = [(d["lapx%d" % j], d["lapu%d" % j]) for j in range(4)]
    B = d["xLin"].shape[0]
    clean = [bench.synth_batch(g, B, N, seed=7 + s, lap=laps[s]) for s in range(4)]
    sing = dict(x0=d["xLin"][:, 0].copy(), xLin=d["xLin"], uLin=d["uLin"], uOld=d["uLin"][:, 0].copy(), zt=d["xLin"][:, N].copy(),
                timeStep=np.zeros(B, np.int32), hasPred=np.zeros(B, np.int32), xPredPrev=np.zeros((B, N + 1, 6)))
    return B, laps, sing, clean


@pytest.fixture(scope="module")
def singular(built, golden):
    """The singular step and the four clean ones run alone at SING_MAX_ITER; some problem of the singular step carries both bits, no clean step the singular one."""
    from racinglmpc_amd import _capi
    B, laps, sing, clean = _singular_sequence(golden)
    outs, asked = _alone_counted(golden, B, [sing] + clean, laps=laps, max_lap_len=512, max_iter=SING_MAX_ITER)
    both = ((outs[0]["status"] & _capi.ST_REG_SINGULAR) != 0) & _maxiter(outs[0])
    print("singular step: status %s, retry passes asked %s" % (outs[0]["status"], asked))
    assert both.any() and asked[0] == 1, (outs[0]["status"], asked)
    assert not any(((o["status"] & _capi.ST_REG_SINGULAR) != 0).any() for o in outs[1:])
    return B, laps, [sing] + clean, outs, asked


@pytest.mark.parametrize("form", ["merged", "two_stream"])
@pytest.mark.parametrize("at", [1, 3])
def test_regression_status_through_a_retry(built, golden, singular, at, form):
    """The singular step at position `at` of five queued steps, nothing drained in between: by the time its retry pass runs, the per-point regression status of
    its hand-over set has been rewritten by clean steps.  Every step equals its alone run: the singular bits stay on their step and reach no neighbour."""
    B, laps, inps, outs, asked = singular
    order = [1, 2, 3, 4]
    order.insert(at, 0)
    ctx = _ctx(golden, B, form, laps=laps, max_lap_len=512, max_iter=SING_MAX_ITER)
    try:
        got, ahead, merge, n_retry = _queued(ctx, B, [inps[i] for i in order])
    finally:
        ctx.close()
    what = "%s, singular step at %d" % (form, at)
    bad = _mismatches(got, [outs[i] for i in order], what)
    assert not bad, "\n".join(bad)
    assert n_retry == sum(asked), (what, n_retry, asked)
    assert (ahead, merge) == _counts(form, 5), (what, ahead, merge)


def test_pool_and_rollout_after_flagged_chained_steps(built, golden, main):
    """A ContextPool whose members have just resolved flagged queued steps takes one more step each; a context that has just resolved a flagged chain runs a short
    rollout session.  Both equal the same calls on fresh contexts (test_gpu_k1_ahead: test_pool_and_rollout_after_chained_steps)."""
    from racinglmpc_amd import _capi
    g = golden
    B = B_MAIN
    pid = (np.array(g["xPID"]), np.array(g["uPID"]))
    cfg, _ = common.lmpc_config(g, N, max_batch=B, max_iter=MAX_ITER)
    pool = _capi.ContextPool(cfg, 2)
    try:
        for _ in range(4):
            pool.model_add_trajectory(*pid); pool.ss_add_trajectory(*pid)
        per_member = [_buffers(m, main.inps[i::2], "own") for i, m in enumerate(pool.members)]
        n_first = 2 * (len(main.inps) // 2)
        for s in range(n_first):
            pool.members[s % 2].step_batch_dev(B, per_member[s % 2][0][s // 2])
        pool.sync()
        for i, m in enumerate(pool.members):
            assert m.stats().n_retry == sum(main.asked[i:n_first:2]), (i, m.stats().n_retry)
        for s in range(n_first, len(main.inps)):                              # the step after the resolved ones
            pool.members[s % 2].step_batch_dev(B, per_member[s % 2][0][s // 2])
        pool.sync()
        for i, m in enumerate(pool.members):
            for j, a in enumerate(per_member[i][0]):
                assert not _diff(m.step_dev_fetch(a, B), main.outs[i + 2 * j]), (i, j)
            assert m.stats().n_retry == sum(main.asked[i::2]), (i, m.stats().n_retry)
            _free(m, per_member[i][1])
    finally:
        pool.close()

    logs = []
    for chain_first in (True, False):
        ctx = _ctx(g, B)
        try:
            if chain_first:
                outs, _, _, n_retry = _queued(ctx, B, main.inps)
                assert not _mismatches(outs, main.outs, "before the session") and n_retry == sum(main.asked)
            x0 = main.inps[0]["x0"]
            ctx.rollout_begin(x0, x0.copy(), main.inps[0]["xLin"], main.inps[0]["uLin"], np.zeros((8, B, 3)))
            steps, _ = ctx.rollout_run(4)
            assert steps == 4
            logs.append(ctx.rollout_fetch(0, 4))
            ctx.rollout_end()
        finally:
            ctx.close()
    for k, (a, b) in enumerate(zip(*logs)):
        assert np.array_equal(a, b), "rollout_fetch()[%d] after a flagged chain differs from a fresh context's" % k


@pytest.mark.parametrize("form", ["merged", "two_stream"])
def test_close_with_flagged_launches_outstanding(built, golden, main, form):
    """close() with a held flagged solve (merged) and with launches pending their retry pass (both forms) returns, and a context created afterwards gives the alone
    answers."""
    g = golden
    ctx = _ctx(g, B_MAIN, form)
    args, _ = _buffers(ctx, main.inps[:3], "own")
    ctx.sync()
    for a in args:
        ctx.step_batch_dev(B_MAIN, a)
    assert ctx.stats().n_retry == 0                                         # (nothing has drained: the launches are pending, step 2's solve is held on the merged form)
    assert ctx.debug_k1_merge()[0] == (1 if form == "merged" else 0)
    ctx.close()
    ctx = _ctx(g, B_MAIN, form)
    try:
        outs, _, _, n_retry = _queued(ctx, B_MAIN, main.inps)
    finally:
        ctx.close()
    bad = _mismatches(outs, main.outs, "%s, fresh context" % form)
    assert not bad, "\n".join(bad)
    assert n_retry == sum(main.asked)


@pytest.mark.parametrize("form", ["merged", "two_stream"])
def test_shared_abc_under_a_pending_retry_shows(built, golden, main, form):
    """The test has teeth.  The five steps with ONE set of A / Bm / C shared by all of them, which include/lmpc_hip.h forbids while a launch is pending its retry
    pass (the caller keeps a launch's arrays untouched until lmpc_dev_sync): the retry pass of step 0 then reads the last step's A / B / C.  At least one flagged
    problem of step 0 differs from the step run alone, and no clean problem does -- so the inputs discriminate, and a retry pass that read another step's
    arrays in the tests above would show.  This documents a contract; rewrite it if the library ever starts copying the arrays."""
    g = golden
    assert FREE_AT != 0
    ctx = _ctx(g, B_MAIN, form)
    try:
        outs, _, _, n_retry = _queued(ctx, B_MAIN, main.inps, "shared")
    finally:
        ctx.close()
    assert n_retry == sum(main.asked)
    got, want = outs[0], main.outs[0]
    hit, clean = _maxiter(want), want["status"] == 0
    differs = np.zeros(B_MAIN, bool)
    for k in got:
        differs |= (got[k] != want[k]).reshape(B_MAIN, -1).any(axis=1)
    print("%s: problems of step 0 that differ: %s; at the limit alone: %s" % (form, np.flatnonzero(differs), np.flatnonzero(hit)))
    assert (differs & hit).any(), (differs, hit)
    assert not (differs & clean).any(), (differs, clean)
    assert not _diff(outs[-1], main.outs[-1])                               # (the last step's arrays are its own when its retry pass runs)
