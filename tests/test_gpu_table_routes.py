"""-m gpu: the per-problem lap tables (lmpc_ss_set_lap_table, lmpc_model_set_lap_table) on every horizon, every solve route and the retry pass.

Every fixed-(N, S) solve kernel has a second instantiation for a safe-set table (TAB in lmpc_variant.hip.h / lmpc_kernels.hip.h): other code objects than the
nominal kernels, with their own dynamic-LDS size, launcher line and hipFuncSetAttribute call.  tests/test_gpu_ss_table.py and tests/test_gpu_lap_table.py run
at N = 12; here the tables run wherever production can launch them.  The method is theirs: the reference of a table row is a context holding ONLY that row's
laps (tests/ss_table_cases.py), run at the SAME batch size, and the table context must give its BITS.  Rows are not tiled with the problems' period: problem b
gets row r(b) = (b + b // 6) % 6, so that every one of the 36 (problem, row) pairs occurs in a batch and a kernel that reads the row of another block index
does not meet an identical neighbour.  Every problem of every batch is compared; no status is masked beyond LMPC_ST_INEXACT (64).

Cells (batch sizes; "-": production never runs that kernel for the horizon; knobs are set around Context() only).  The route list is
tests/test_gpu_routes._routes(N), its batches moved to the nearest multiple of six on the same side of each threshold (64 -> 66, 1100 -> 1098):

   N   S  numSS_it | 4 waves | 2 waves | 1 wave, [A|B] in LDS     | 1 wave, [A|B] global | runtime kernel | other
   8  48   4       |   66    |   300   | 1098                     |  -                   | 1098           |
  12  48   4       |   66    |   (1)   | (1)                      |  -                   | 1098           | LMPC_FUSE=1 at 1098: the two-kernel step; retry pass at 66 (4 waves)
  14  48   4       |   66    |   300   | 600                      |  -                   | 600            |
  20  48   4       |   66    |   300   | 600                      |  -                   | 600            | step_batch_dev at 66
  40  48   4       |   66    |   -     | 300; 1098 + LMPC_NO_ABG  | 1098                 | 1098           | retry pass at 66 (4 waves)
  12  48   4       | both tables: 66 | 300 | 1098                 |  -                   |  -             | both tables in a rollout session of 3 cars
  40  48   4       |   -     |   -     |  -                       | both tables: 1098    |  -             |
  12  64  32       |   -     |   -     |  -                       |  -                   | 3, 66          | sel_lap fills all of LMPC_SSTAB_LDS
  12  72   6       |   -     |   -     |  -                       |  -                   | 3, 66          |
  12  48   4       |    6    |   -     |  -                       |  -                   |  -             | LMPC_ST_WINDOW on one car only
  (1) tests/test_gpu_ss_table.py::test_every_kernel_route_serves_the_table

Per horizon the first 36 problems of the four-wave batch -- all 36 pairs -- are also held against the oracle: the selection equals oracle.terminal_components
with sortedLapTime and cur_it per car, and xPred, uPred lie within common.TOL_XU of the nearer of the oracle's two certified optima of the QP assembled from
that selection.  The oracle runs before the test makes its first HIP context (forked workers)."""
import contextlib

import numpy as np
import pytest

from tests import common
from tests import ss_table_cases as cases
from tests.test_gpu_routes import ALL_KEYS, _knobs, _routes

pytestmark = pytest.mark.gpu

STEP_KEYS = ("xPred", "uPred", "lambd", "ztNext", "ztuNext", "status", "iters", "ssSel", "qSel")
KEYS = STEP_KEYS + ("A", "B", "C")
DEV_KEYS = tuple(k for k in KEYS if k != "qSel")                      # (step_dev_buffers(diagnostics=False) leaves qSel NULL)
SEL_KEYS = ("ssSel", "qSel", "succ", "succU", "selStart")
BATCH = {64: 66, 300: 300, 600: 600, 1100: 1098}                       # the batches of _routes -> the nearest multiple of six on the same side of the threshold
ROUTES = ("4 waves", "2 waves", "1 wave", "1 wave, [A|B] in LDS", "1 wave, [A|B] global", "1 wave, [A|B] in LDS (LMPC_NO_ABG)", "runtime kernel")
ROUTES_12 = ("4 waves", "runtime kernel")                              # N = 12: the others are in tests/test_gpu_ss_table.py


def _row(B, n=6):
    """r(b) = (b + b // 6) % n for b < B."""
    b = np.arange(B)
    return (b + b // 6) % n


@pytest.fixture(scope="module")
def g(built):
    return common.load_lmpc_golden()


def _step(ctx, p):
    return ctx.step_batch(p["x0"], p["xLin"], p["uLin"], p["uOld"], p["zt"], p["xPredPrev"], p["hasPred"], p["timeStep"])


def _sel(ctx, p):
    return ctx.select_batch(p["x0"], p["zt"], p["xPredPrev"], p["hasPred"], p["timeStep"])


def _diff(a, b, keys, rows=slice(None)):
    return [k for k in keys if not np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k])[rows])]


def _fill_ss(ctx, g):
    """The six safe-set laps of the fixture, lap 2 extended (the safe-set half of cases.fill_table_context)."""
    laps, ext = cases.fixture_laps(g)
    for x, u in laps:
        ctx.ss_add_trajectory(x, u)
    ctx.ss_extend_lap(cases.EXTENDED, ext[0], ext[1])


def _fill_own_ss(own, stored, order):
    """The laps `order` of `stored` with their current rows and Q-function (the safe-set half of cases.fill_own_context)."""
    for i, l in enumerate(order):
        x, u, q, T0 = stored[l]
        own.ss_add_trajectory(x[:T0], u[:T0])
        own.ss_replace_lap(i, x, u, q)


class _Set:
    """A table context and one reference context per row.  rows / last: the safe-set rows.  model = None: the PID run four times in every regression store,
    as in tests/ss_table_cases.py; model = (laps, mrows): the table context holds all regression laps and gets model_set_lap_table, reference r holds only the
    laps of mrows[r], by ascending insertion index and with multiplicity (trToUse = all of them)."""

    def __init__(self, g, N, max_batch, rows=cases.ROWS4, last=cases.LAST4, runtime=False, knobs=None, model=None, **kw):
        from racinglmpc_amd import _capi
        self.rows, self.last, self.model = np.asarray(rows, np.int32), np.asarray(last, np.int32), model
        cfg, self.par = common.lmpc_config(g, N, max_batch=max_batch, numSS_it=self.rows.shape[1], **kw)
        self.all = []
        pid = (np.array(g["xPID"]), np.array(g["uPID"]))

        def make():
            with _knobs(knobs or {}):
                c = _capi.Context(cfg, runtime_kernel=runtime)
            self.all.append(c)
            assert c.solver_kind == (2 if runtime else 0)
            return c
        try:
            self.ctx = make()
            for x, u in (model[0] if model else [pid] * 4):
                self.ctx.model_add_trajectory(x, u)
            _fill_ss(self.ctx, g)
            self.stored = cases.read_laps(self.ctx)
            lt = [s[3] for s in self.stored]
            self.owns = []
            for r in range(self.rows.shape[0]):
                own = make()
                for k in (sorted(int(k) for k in model[1][r]) if model else range(4)):
                    own.model_add_trajectory(*(model[0][k] if model else pid))
                _fill_own_ss(own, self.stored, cases.own_order(self.rows[r], self.last[r], lt))
                self.owns.append(own)
        except Exception:
            self.close()
            raise

    def use(self, B, perm=None):
        """Row r(b) for problem b of a batch of B, in both tables; perm: row perm[r(b)] instead.  Returns r(b)."""
        rb = _row(B, self.rows.shape[0])
        idx = rb if perm is None else np.asarray(perm)[rb]
        self.ctx.ss_set_lap_table(self.rows[idx], self.last[idx])
        if self.model:
            self.ctx.model_set_lap_table(np.asarray(self.model[1], np.int32)[idx])
        return idx

    def close(self):
        for c in self.all:
            c.close()


def _cell(st, p, B, waves, what):
    """One launch of the table context on its route, and every problem against the reference context of its row at the same batch: (outputs, failures)."""
    rb = st.use(B)
    kind = st.ctx.solver_kind
    assert st.ctx.solver_waves(B) == waves and all(o.solver_waves(B) == waves and o.solver_kind == kind for o in st.owns), (what, st.ctx.solver_waves(B), waves)
    st.ctx.reset_stats()
    out = _step(st.ctx, p)
    fails = []
    if int(st.ctx.stats().n_regress) != 1:
        fails.append("%s: %d regression launches" % (what, int(st.ctx.stats().n_regress)))
    if (out["status"] & ~64).any():
        fails.append("%s: status %s" % (what, np.unique(out["status"], return_counts=True)))
    refs = [_step(own, p) for own in st.owns]
    for r, ref in enumerate(refs):
        mine = np.where(rb == r)[0]
        assert mine.size >= B // 6
        bad = _diff(out, ref, KEYS, mine)
        if bad:
            fails.append("%s, row %d: %s differ from the context holding only that row's laps" % (what, r, ", ".join(bad)))
        # (the comparison tells the rows apart: the same problems on the next row's reference select other points or other Q-values)
        assert _diff(out, refs[(r + 1) % len(refs)], ("ssSel", "qSel"), mine), (what, r)
    return out, fails


# ---- the oracle over many (problem, row) pairs, one process per core (children never touch HIP: fork, NumPy only)
_JOB = {}


def _oracle_work(i):
    from oracle import lmpc_oracle as orc
    c = _JOB; j = c["jobs"][i]; p, b, N = c["p"], j["b"], c["N"]
    SSsel, Qsel, Succ, SuccU, ok = cases.oracle_selection(c["stored"], j["order"], p, b, c["TL"], c["L"], c["ppl"], N=N)
    res = dict(b=b, SSsel=SSsel, Qsel=Qsel, ok=ok)
    if c["solve"]:
        xs, us = j["model"]
        A, Bm, Cc = orc.compute_ltv_dynamics(xs, us, list(range(len(xs))), c["pt"], p["xLin"][b], p["uLin"][b], N)
        P, q, Ao, lo, up = orc.assemble_lmpc_qp(c["par"], A, Bm, Cc, p["x0"][b], p["uOld"][b], SSsel.T, Qsel)
        ex, cert = orc.osqp_solve_exact(P, q, Ao, lo, up, want=1e-8)
        r2 = orc.dense_ipm_solve(P, q, Ao, lo, up)
        res.update(A=A, B=Bm, C=Cc, opt=ex.x, cert=cert, opt2=r2.x)
    return res


def _oracle(jobs, **common_args):
    """jobs: [dict(b, order, model=(x laps, u laps) in the store's sorted order)]; common: stored, p, N, TL, L, ppl, par, pt, solve."""
    import multiprocessing as mp
    try:
        from threadpoolctl import threadpool_limits
        lim = threadpool_limits(1)
    except Exception:                                 # noqa: BLE001
        lim = None
    _JOB.clear()
    _JOB.update(common_args, jobs=jobs)
    n = max(1, min(16, len(jobs)))
    try:
        if n == 1 or not common_args["solve"]:
            return [_oracle_work(i) for i in range(len(jobs))]
        with mp.get_context("fork").Pool(n) as pool:
            return pool.map_async(_oracle_work, range(len(jobs)), chunksize=1).get(timeout=420)
    finally:
        _JOB.clear()
        if lim is not None and hasattr(lim, "restore_original_limits"):
            lim.restore_original_limits()


def _against_oracle(out, res, N, what):
    """Selection exact, (x, u) within TOL_XU of the nearer certified optimum; A, B, C (where the caller wants them) are compared by the caller.  Worst error."""
    nxu = 6 * (N + 1) + 2 * N
    worst = 0.0
    for r in res:
        b = r["b"]
        assert r["ok"], (what, b)
        assert np.array_equal(out["ssSel"][b], r["SSsel"]) and np.array_equal(out["qSel"][b], r["Qsel"]), (what, b)
        assert r["cert"] < 1e-7, (what, b, r["cert"])
        w = np.concatenate([out["xPred"][b].ravel(), out["uPred"][b].ravel()])
        worst = max(worst, min(float((np.abs(w - o[:nxu]) / (1 + np.abs(o[:nxu]))).max()) for o in (r["opt"], r["opt2"])))
    return worst


def _pid_model(g):
    return [np.array(g["xPID"])] * 4, [np.array(g["uPID"])] * 4


@pytest.mark.parametrize("N", [8, 12, 14, 20, 40])
def test_every_route_serves_the_table_at_every_horizon(g, N):
    """ROWS4 / LAST4 on every route production takes at horizon N (N = 12: the four-wave batch of 66 and the runtime kernel with numSS_it = 4; the other routes
    are in tests/test_gpu_ss_table.py).  Per cell: the route (solver_waves, solver_kind, one regression launch), no status bit but INEXACT, and EVERY problem equal,
    bit for bit, to the context holding only its row's laps at the same batch -- the step's outputs and A, B, C.  N = 40: [A|B] in global memory and in LDS
    (LMPC_NO_ABG) agree in every output.  The first 36 problems of the four-wave batch against the oracle."""
    TL = float(g["trackLength"])
    routes = [r for r in _routes(N) if r[0] in (ROUTES_12 if N == 12 else ROUTES)]
    want = ROUTES_12 if N == 12 else tuple(n for n in ROUTES if (n == "2 waves") <= (N <= 24) and (n == "1 wave") <= (N != 40) and ("[A|B]" in n) <= (N == 40))
    assert tuple(r[0] for r in routes) == want, routes                  # (a route renamed or dropped in tests/test_gpu_routes.py must not silently drop a cell here)
    Bmax = max(BATCH[r[1]] for r in routes)
    pmax = cases.problems(g, Bmax, N)
    # the oracle first: 36 problems, all (problem, row) pairs, on the laps as the CPU stores them (compared with the context's below)
    stored_cpu = cases.cpu_stored(g)
    lt = [s[3] for s in stored_cpu]
    rb36 = _row(36)
    jobs = [dict(b=b, order=cases.own_order(cases.ROWS4[rb36[b]], cases.LAST4[rb36[b]], lt), model=_pid_model(g)) for b in range(36)]
    assert len({(b % 6, int(rb36[b])) for b in range(36)}) == 36
    from oracle import lmpc_oracle as orc
    res = _oracle(jobs, stored=stored_cpu, p=pmax, N=N, TL=TL, L=4, ppl=12, par=orc.QPParams.lmpc_default(N), pt=np.array(g["track"]), solve=True)

    sets, outs, fails, table = {}, {}, [], []
    try:
        for name, B0, waves, knobs, rt, fused in routes:
            B = BATCH[B0]
            key = (tuple(sorted(knobs.items())), rt)
            if key not in sets:
                sets[key] = _Set(g, N, Bmax, runtime=rt, knobs=knobs)
                for (xa, ua, qa, Ta), (xb, ub, qb, Tb) in zip(sets[key].stored, stored_cpu):     # the oracle's laps are the context's
                    assert Ta == Tb and np.array_equal(xa, xb) and np.array_equal(ua, ub) and np.array_equal(qa, qb)
            what = "N = %d, %s, batch %d" % (N, name, B)
            p = {k: v[:B] for k, v in pmax.items()}
            out, f = _cell(sets[key], p, B, waves, what)
            outs[name] = out; fails += f
            table.append((name, B, waves, sets[key].ctx.solver_kind, len(f)))
            if name == "4 waves":
                worst = _against_oracle(out, res, N, what)
                print("N = %d: table rows against the oracle, 36 problems: selection identical, worst |xu - z*| / (1 + |z*|) %.2e" % (N, worst))
                if not worst < common.TOL_XU:
                    fails.append("%s: oracle: %.2e" % (what, worst))
        if N == 40:
            bad = _diff(outs["1 wave, [A|B] global"], outs["1 wave, [A|B] in LDS (LMPC_NO_ABG)"], ALL_KEYS)
            if bad:
                fails.append("N = 40, batch 1098: %s differ between [A|B] in global memory and in LDS" % ", ".join(bad))
    finally:
        for s in sets.values():
            s.close()
    print("\nN = %d, S = 48, safe-set table: route, batch, waves per QP, solver kind, failures" % N)
    for row in table:
        print("  %-36s %5d %d %d %d" % row)
    assert not fails, "\n".join(fails)


def test_the_fused_step_is_not_taken_with_a_safe_set_table(g):
    """LMPC_FUSE=1 at N = 12, batch 1098 (one wave per QP), where the fused step runs without a table (no regression launch): with a safe-set table the two-kernel
    step runs -- one regression launch -- and every output equals, bit for bit, that of a context created without the knob."""
    from racinglmpc_amd import _capi
    N, B = 12, 1098
    p = cases.problems(g, B, N)
    rb = _row(B)
    cfg, _ = common.lmpc_config(g, N, max_batch=B)
    out = {}
    for fuse in (False, True):
        with _knobs({"LMPC_FUSE": "1"} if fuse else {}):
            ctx = _capi.Context(cfg)
        try:
            cases.fill_table_context(ctx, g)
            assert ctx.solver_waves(B) == 1 and ctx.solver_kind == 0
            if fuse:                                               # (the knob is in force: without a table this batch takes the fused step)
                ctx.reset_stats(); _step(ctx, p)
                assert int(ctx.stats().n_regress) == 0
            ctx.ss_set_lap_table(cases.ROWS4[rb], cases.LAST4[rb])
            ctx.reset_stats()
            out[fuse] = _step(ctx, p)
            assert int(ctx.stats().n_regress) == 1, fuse
        finally:
            ctx.close()
    assert not (out[True]["status"] & ~64).any()
    assert not _diff(out[True], out[False], ALL_KEYS + ("resid",))


def test_device_path_equals_host_path_at_another_horizon(g):
    """N = 20, batch 66, rows r(b): step_batch_dev gives the outputs of step_batch."""
    from racinglmpc_amd import _capi
    N, B = 20, 66
    p = cases.problems(g, B, N)
    rb = _row(B)
    cfg, _ = common.lmpc_config(g, N, max_batch=B)
    with _capi.Context(cfg) as ctx:
        cases.fill_table_context(ctx, g)
        ctx.ss_set_lap_table(cases.ROWS4[rb], cases.LAST4[rb])
        assert ctx.solver_waves(B) == 4 and ctx.solver_kind == 0
        host = _step(ctx, p)
        assert not (host["status"] & ~64).any()
        args, keep = ctx.step_dev_buffers(p)
        try:
            ctx.step_batch_dev(B, args)
            dev = ctx.step_dev_fetch(args, B)
        finally:
            for q in keep:
                ctx.dev_free(q)
    assert not _diff(dev, host, ALL_KEYS)


# ---- the retry pass with a table
@contextlib.contextmanager
def _retry_ctx(g, N, B, table=None):
    """A max_iter = 7 context with the fixture's stores; table = (rows, last) per problem, or None: the shared rule."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=B, max_iter=7)
    ctx = _capi.Context(cfg)
    try:
        cases.fill_table_context(ctx, g)
        if table is not None:
            ctx.ss_set_lap_table(*table)
        yield ctx
    finally:
        ctx.close()


@pytest.mark.parametrize("N", [12, 40])
def test_retry_pass_with_a_table(g, N):
    """max_iter = 7 (tests/test_gpu_retry.py), batch 66, rows r(b): some problems end at the iteration limit and some clean; the retry pass -- the EQ, TAB
    instantiation of the one-wave kernel, whose body selects again from the problem's row -- runs once on the table context and once on each reference context;
    EVERY problem, those that end at the limit after the retry included, equals its reference context bit for bit."""
    from racinglmpc_amd import _capi
    B = 66
    p = cases.problems(g, B, N)
    st = _Set(g, N, B, max_iter=7)
    try:
        rb = st.use(B)
        assert st.ctx.solver_waves(B) == 4 and st.ctx.solver_kind == 0
        st.ctx.reset_stats()
        out = _step(st.ctx, p)
        hit = (out["status"] & _capi.ST_MAXITER) != 0
        print("N = %d, max_iter = 7: %d of %d problems at the limit after the retry pass, %d clean; iterations %s" % (N, hit.sum(), B, (out["status"] == 0).sum(), np.unique(out["iters"])))
        assert st.ctx.stats().n_retry == 1 and st.ctx.stats().n_regress == 1
        fails = []
        for r, own in enumerate(st.owns):
            own.reset_stats()
            ref = _step(own, p)
            assert own.stats().n_retry == 1, r
            bad = _diff(out, ref, KEYS, np.where(rb == r)[0])
            if bad:
                fails.append("N = %d, row %d: %s differ from the context holding only that row's laps" % (N, r, ", ".join(bad)))
        assert not fails, "\n".join(fails)
        assert hit.any() and (out["status"] == 0).any()
    finally:
        st.close()


@pytest.mark.parametrize("second", ["another table", "no table"])
@pytest.mark.parametrize("N", [12, 40])
def test_deferred_retry_reads_the_table_of_its_own_launch(g, N, second):
    """Device path, max_iter = 7, batch 66: a launch with table T1 (rows r(b)) stays pending its retry pass; then the context gets T2 -- every problem's row
    changed -- or no table at all, and a second launch on other buffers; then both are fetched.  The first launch equals a context that only ever had T1, the second
    one that only ever had T2 (or never had a table): the pending retry pass read the device image of ITS launch."""
    from racinglmpc_amd import _capi
    B = 66
    p = cases.problems(g, B, N)
    rb = _row(B)
    perm = np.array([1, 2, 3, 4, 5, 0])
    T1 = (cases.ROWS4[rb], cases.LAST4[rb])
    T2 = (cases.ROWS4[perm[rb]], cases.LAST4[perm[rb]]) if second == "another table" else None
    assert T2 is None or not (T1[0] == T2[0]).all(1).any()
    with _retry_ctx(g, N, B, T1) as c:
        ref1 = _step(c, p)
        assert ((ref1["status"] & _capi.ST_MAXITER) != 0).any() and c.stats().n_retry == 1
    with _retry_ctx(g, N, B, T2) as c:
        ref2 = _step(c, p)
        assert c.stats().n_retry == 1
    assert _diff(ref1, ref2, ("ssSel",))                                   # (the two launches do select differently)
    with _retry_ctx(g, N, B, T1) as ctx:
        a1, keep1 = ctx.step_dev_buffers(p, diagnostics=False); a2, keep2 = ctx.step_dev_buffers(p, diagnostics=False)
        try:
            ctx.step_batch_dev(B, a1)
            assert ctx.stats().n_retry == 0                                # pending
            ctx.ss_set_lap_table(*T2) if T2 is not None else ctx.ss_set_lap_table(None)
            ctx.step_batch_dev(B, a2)
            if T2 is not None:
                assert ctx.stats().n_retry == 1                            # the image is about to be overwritten: launch 1 got its pass first
            out1 = ctx.step_dev_fetch(a1, B); out2 = ctx.step_dev_fetch(a2, B)
            assert ctx.stats().n_retry == 2
        finally:
            for q in keep1 + keep2:
                ctx.dev_free(q)
    bad1, bad2 = _diff(out1, ref1, DEV_KEYS), _diff(out2, ref2, DEV_KEYS)
    assert not bad1, "the pending launch's %s differ from a context that only ever had its table" % bad1
    assert not bad2, "the second launch's %s differ from a context that only ever had %s" % (bad2, second)


# ---- both tables in force
MROWS = np.array([[0, 1, 2, 3], [4, 0, 1, 5], [2, 2, 3, 4], [5, 4, 1, 0], [0, 1, 5, 4], [3, 5, 2, 1]], np.int32)
# regression laps 0..3: 400-row cuts (the 8-rows-per-lane scan), 4: 800 rows (16 rows per lane), 5: LMPC lap 4.  Rows: mixed classes; row 0 short laps only; a lap
# twice (row 2); the same laps in three orders (rows 1, 3, 4)


def _model_laps(g):
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    laps = [(xP[0:400], uP[0:400]), (xP[100:500], uP[100:500]), (xP[200:600], uP[200:600]), (xP[210:610], uP[210:610]), (xP[150:950], uP[150:950]),
            (np.array(g["lapx0"]), np.array(g["lapu0"]))]
    assert max(x.shape[0] for x, _ in laps[:4]) <= 512 < laps[4][0].shape[0] <= 1024
    return [(np.ascontiguousarray(x), np.ascontiguousarray(u)) for x, u in laps]


def _car_model(laps, row):
    """(x laps, u laps) of a regression store holding exactly the laps of `row`, as PredictiveModel.addTrajectory sorts them."""
    from oracle import lmpc_oracle as orc
    xs, us, lt = [], [], []
    for k in sorted(int(k) for k in row):
        orc.model_sorted_insert(xs, us, lt, laps[k][0], laps[k][1])
    return xs, us


def _both_problems(g, laps, B):
    """cases.problems at N = 12 with the linearisation of base problem k moved to the first start row t >= its own at which the ORACLE's float64 regression, on
    every horizon point and on the laps of model row k, is within OWN_TOL of the same fit in longdouble (tests/test_gpu_lap_table._own_error: the rule looks at the
    reference alone), so that the oracle carries the A, B, C comparison.  Returns (problems, start rows)."""
    from tests.test_gpu_lap_table import OWN_TOL, _own_error
    N = 12
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"]); TL = float(g["trackLength"])
    p = cases.problems(g, B, N)
    named = dict(enumerate(laps))
    rows = []
    for k, t0 in enumerate(cases.start_steps(N)):
        for t in range(t0, t0 + 37):
            if all(_own_error(named, tuple(sorted(int(l) for l in MROWS[k])), xP[t + 1 + i], uP[t + 1 + i]) <= OWN_TOL for i in range(N)):
                rows.append(t)
                break
        else:
            raise AssertionError("base problem %d: no start row in [%d, %d) where the oracle carries the comparison" % (k, t0, t0 + 37))
    for b in range(B):
        t = rows[b % 6]
        p["xLin"][b] = xP[t + 1:t + N + 2]; p["uLin"][b] = uP[t + 1:t + N + 1]
        if b % 6 == 5:
            p["xLin"][b, :, 4] -= TL
    return p, rows


def test_both_tables_in_force(g):
    """An LMPC context with six different regression laps and MROWS (trToUse = 4) AND the safe-set table ROWS4 / LAST4, rows r(b) for both.  The reference of car b
    holds only car b's regression laps and only its safe-set row.  step_batch at N = 12 on the four-, two- and one-wave batches and at N = 40 with [A|B] in global
    memory: every problem equals its reference bit for bit in A, B, C and the step's outputs.  The six base problems (rows 0..5) against the oracle: A, B, C within
    TOL_ABC of compute_ltv_dynamics on the car's laps, the selection exact, (x, u) within TOL_XU of the certified optimum."""
    from oracle import lmpc_oracle as orc
    TL = float(g["trackLength"])
    laps = _model_laps(g)
    p12, start = _both_problems(g, laps, 1098)
    print("linearisation start rows of the six base problems:", start, "(fixture:", cases.start_steps(12), ")")
    stored_cpu = cases.cpu_stored(g)
    lt = [s[3] for s in stored_cpu]
    jobs = [dict(b=b, order=cases.own_order(cases.ROWS4[b], cases.LAST4[b], lt), model=_car_model(laps, MROWS[b])) for b in range(6)]
    res = _oracle(jobs, stored=stored_cpu, p=p12, N=12, TL=TL, L=4, ppl=12, par=orc.QPParams.lmpc_default(12), pt=np.array(g["track"]), solve=True)
    fails = []
    for N, cells in ((12, (("4 waves", 66, 4), ("2 waves", 300, 2), ("1 wave", 1098, 1))), (40, (("1 wave, [A|B] global", 1098, 1),))):
        pmax = p12 if N == 12 else cases.problems(g, 1098, N)
        st = _Set(g, N, 1098, model=(laps, MROWS))
        try:
            for name, B, waves in cells:
                what = "both tables, N = %d, %s, batch %d" % (N, name, B)
                out, f = _cell(st, {k: v[:B] for k, v in pmax.items()}, B, waves, what)
                fails += f
                if name == "4 waves":
                    worst_abc = 0.0
                    for r in res:
                        for got, ref in ((out["A"][r["b"]], r["A"]), (out["B"][r["b"]], r["B"]), (out["C"][r["b"]], r["C"])):
                            worst_abc = max(worst_abc, float((np.abs(got - ref) / (1 + np.abs(ref))).max()))
                    worst = _against_oracle(out, res, N, what)
                    print("both tables against the oracle, 6 cars: worst relative |A, B, C - oracle| %.2e, selection identical, worst |xu - z*| / (1 + |z*|) %.2e" % (worst_abc, worst))
                    if not (worst_abc < common.TOL_ABC and worst < common.TOL_XU):
                        fails.append("%s: oracle: A, B, C %.2e, xu %.2e" % (what, worst_abc, worst))
                    assert not np.array_equal(out["A"][0], out["A"][6])     # (the same problem on model rows 0 and 1: the cars' models do differ)
        finally:
            st.close()
    assert not fails, "\n".join(fails)


def test_both_tables_in_a_rollout_session(g):
    """Three cars with three regression rows and three safe-set rows, device noise, run until every car has crossed the line (start steps and T_max of
    tests/test_gpu_ss_table.py::test_rollout_session_with_three_rows): X, U up to each car's crossing, the crossing step and the status word equal those of one-car
    sessions on contexts holding only the car's regression laps and its safe-set row, with the car's noise offset."""
    from racinglmpc_amd import _capi
    N = 12
    rows, last = np.array([[1, 1, 1, 5], [1, 1, 1, 1], [1, 1, 5, 5]], np.int32), np.array([5, -1, -1], np.int32)
    mrows = MROWS[:3]
    laps = _model_laps(g)
    cfg, _ = common.lmpc_config(g, N, max_batch=4)
    t0 = np.array([100, 104, 108])
    assert (np.array(g["all_lap"])[t0] == 4).all() and (np.array(g["all_t"])[t0] == t0).all()
    x0 = np.array(g["all_x0"])[t0]; xl = np.array(g["all_xLin"])[t0]; ul = np.array(g["all_uLin"])[t0]
    T, SEED = 200, 78
    ctx = _capi.Context(cfg)
    owns = []
    try:
        for x, u in laps:
            ctx.model_add_trajectory(x, u)
        _fill_ss(ctx, g)
        stored = cases.read_laps(ctx); lt = [s[3] for s in stored]
        ctx.model_set_lap_table(mrows)
        ctx.ss_set_lap_table(rows, last)
        ctx.rollout_set_noise(True, SEED, 0, 0)
        ctx.rollout_begin(x0, x0, xl, ul, None, T_max=T)
        t, _ = ctx.rollout_run(T)
        X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
        ctx.rollout_end()
        print("session with both tables: steps", t, "done", done, "status", st)
        assert (done >= 0).all() and not (st & ~64).any(), (done, st)
        for b in range(3):
            own = _capi.Context(cfg); owns.append(own)
            for k in sorted(int(k) for k in mrows[b]):
                own.model_add_trajectory(*laps[k])
            _fill_own_ss(own, stored, cases.own_order(rows[b], last[b], lt))
            own.rollout_set_noise(True, SEED, 0, b)
            own.rollout_begin(x0[b:b + 1], x0[b:b + 1], xl[b:b + 1], ul[b:b + 1], None, T_max=T)
            to, _ = own.rollout_run(T)
            Xo, Uo, _, done_o, st_o, _, _ = own.rollout_fetch(0, to)
            own.rollout_end()
            n = int(done[b])
            assert done_o[0] == done[b] and st_o[0] == st[b] and np.array_equal(Xo[:n, 0], X[:n, b]) and np.array_equal(Uo[:n, 0], U[:n, b]), b
        assert not np.array_equal(U[:10, 0], U[:10, 1])
    finally:
        for c in [ctx] + owns:
            c.close()


# ---- table edges on the runtime kernel
EDGE_EXTRA = 33                                            # the slowest lap, behind laps 0..32
EDGES = {
    # numSS_it = 32, two points per lap (windows of three rows), S = 64: two terminal-block columns per lane, and sel_lap fills all of LMPC_SSTAB_LDS
    "numSS_it 32, 64 points": (32, 64, [list(range(32)), list(range(1, 33)), [k // 2 for k in range(32)]], [31, 32, -1]),
    # numSS_it = 6, 72 points: the lmpc_wide_n12 shape
    "numSS_it 6, 72 points": (6, 72, [[0, 1, 2, 3, 4, 5], [10, 11, 12, 13, 14, 32], [7, 7, 8, 8, 9, 9]], [5, 32, -1]),
}


@pytest.mark.parametrize("shape", list(EDGES))
def test_runtime_kernel_serves_wide_rows(g, shape):
    """The runtime-(N, S) kernel, N = 12, with 34 safe-set laps xP[0:330 + k], k = 0..32 (distinct LapTimes) and xP[0:370] (the slowest), three rows: the first
    laps, the last laps with `last` in the row, a row with repeats and last = -1.  B = 3 (problems 0, 2, 5: no crossing, crossing, wrap) and B = 66 (row
    (b + b // 6) % 3: all 18 pairs): every problem equals the context holding only its row's laps, bit for bit, and its selection equals the oracle's."""
    from racinglmpc_amd import _capi
    N = 12
    L, S, rows, last = EDGES[shape]
    rows, last = np.array(rows, np.int32), np.array(last, np.int32)
    ppl = S // L
    TL = float(g["trackLength"])
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    laps = [(np.ascontiguousarray(xP[0:330 + k]), np.ascontiguousarray(uP[0:330 + k])) for k in range(33)] + [(np.ascontiguousarray(xP[0:370]), np.ascontiguousarray(uP[0:370]))]
    cfg, _ = common.lmpc_config(g, N, max_batch=66, numSS_it=L, numSS_Points=S)
    made = []

    def make():
        c = _capi.Context(cfg, runtime_kernel=True); made.append(c)
        assert c.solver_kind == 2
        for _ in range(4):
            c.model_add_trajectory(xP, uP)
        return c
    try:
        ctx = make()
        for x, u in laps:
            ctx.ss_add_trajectory(x, u)
        stored = cases.read_laps(ctx)
        lt = [s[3] for s in stored]
        assert len(set(lt)) == len(lt) == 34 and max(lt) == lt[EDGE_EXTRA]
        orders = [cases.own_order(rows[r], last[r], lt, extra=EDGE_EXTRA) for r in range(3)]
        owns = []
        for r in range(3):
            own = make()
            _fill_own_ss(own, stored, orders[r])
            owns.append(own)
        p6 = cases.problems(g, 6, N)
        for B in (3, 66):
            p = {k: v[[0, 2, 5]] for k, v in p6.items()} if B == 3 else cases.problems(g, B, N)
            rb = _row(B, 3)
            ctx.ss_set_lap_table(rows[rb], last[rb])
            assert ctx.solver_waves(B) == 1
            ctx.reset_stats()
            out = _step(ctx, p)
            sel = _sel(ctx, p)
            assert int(ctx.stats().n_regress) == 1
            assert not (out["status"] & ~64).any() and not sel["status"].any(), (B, out["status"], sel["status"])
            for r in range(3):
                mine = np.where(rb == r)[0]
                bad = _diff(out, _step(owns[r], p), KEYS, mine) + _diff(sel, _sel(owns[r], p), SEL_KEYS + ("ztUsed", "status"), mine)
                assert not bad, (shape, B, r, bad)
            for b in range(min(B, 18)):
                SSsel, Qsel, Succ, SuccU, ok = cases.oracle_selection(stored, orders[rb[b]], p, b, TL, L, ppl, N=N)
                assert ok, (shape, B, b)
                assert np.array_equal(sel["ssSel"][b], SSsel) and np.array_equal(sel["qSel"][b], Qsel) and np.array_equal(sel["succ"][b], Succ) and np.array_equal(sel["succU"][b], SuccU), (shape, B, b)
                assert np.array_equal(out["ssSel"][b], SSsel) and np.array_equal(out["qSel"][b], Qsel), (shape, B, b)
    finally:
        for c in made:
            c.close()


WROWS = np.array([[0, 1, 2, 4], [1, 1, 3, 4], [3, 5, 1, 0], [0, 1, 5, 3], [0, 3, 4, 1], [1, 4, 4, 5]], np.int32)      # only row 0 names lap 2, the extended lap
WLAST = np.array([4, 5, -1, -1, 4, 5], np.int32)
WPROB = [2, 0, 1, 3, 4, 5]                                 # problem 0 of the batch is base problem 2: its zt = xP[309] lies among the rows that extend lap 2


def window_cut(stored, lt, p, TL):
    """The number of rows to keep of lap 2 (LapTime <= T < its rows) so that the 13-row window of problem 0 on row 0 runs past the end of that lap, by the oracle's
    window rule: the largest such T.  Everything else must pass the rule before and after the cut."""
    x, u, q, T0 = stored[cases.EXTENDED]
    orders = [cases.own_order(WROWS[r], WLAST[r], lt) for r in range(6)]
    assert all(cases.window_ok(stored, orders[b], p, b, TL, 4, 12) for b in range(6))
    for T in range(x.shape[0] - 1, T0 - 1, -1):
        cut = list(stored); cut[cases.EXTENDED] = (x[:T], u[:T], q[:T], T0)
        if not cases.window_ok(cut, orders[0], p, 0, TL, 4, 12):
            assert all(cases.window_ok(cut, orders[b], p, b, TL, 4, 12) for b in range(1, 6))
            return T
    raise AssertionError("no cut of lap 2 puts problem 0's window past its end")


def test_window_status_on_one_car_only(g):
    """Fixed kernels, N = 12, B = 6, a table in which only row 0 names lap 2.  After ss_truncate_lap(2, T), T chosen with the oracle's window rule on the CPU, the
    13-row window around problem 0's zt runs past the end of that lap: problem 0 carries LMPC_ST_WINDOW and its ssSel, qSel, succ, succU, selStart are the bits of the
    context holding only row 0's laps (cut the same way); the other five problems are clean and unchanged from before the edit."""
    from racinglmpc_amd import _capi
    N, TL = 12, float(g["trackLength"])
    p = {k: v[WPROB] for k, v in cases.problems(g, 6, N).items()}
    stored_cpu = cases.cpu_stored(g)
    lt = [s[3] for s in stored_cpu]
    T = window_cut(stored_cpu, lt, p, TL)
    print("lap 2: %d rows stored, LapTime %d, cut to %d" % (stored_cpu[2][0].shape[0], lt[2], T))
    cfg, _ = common.lmpc_config(g, N, max_batch=6)
    with _capi.Context(cfg) as ctx:
        cases.fill_table_context(ctx, g)
        ctx.ss_set_lap_table(WROWS, WLAST)
        assert ctx.solver_waves(6) == 4 and ctx.solver_kind == 0
        sel0, out0 = _sel(ctx, p), _step(ctx, p)
        assert not sel0["status"].any() and not (out0["status"] & ~64).any()
        ctx.ss_truncate_lap(cases.EXTENDED, T)
        sel1, out1 = _sel(ctx, p), _step(ctx, p)
        stored = cases.read_laps(ctx)
        assert stored[cases.EXTENDED][0].shape[0] == T
        with _capi.Context(cfg) as own:
            cases.fill_own_context(own, g, stored, cases.own_order(WROWS[0], WLAST[0], lt))
            ref = _sel(own, p)
            ref_step = _step(own, p)
    assert sel1["status"][0] & _capi.ST_WINDOW and out1["status"][0] & _capi.ST_WINDOW and ref["status"][0] == sel1["status"][0]
    assert not _diff(sel1, ref, SEL_KEYS, 0)
    assert not _diff(out1, ref_step, ("ssSel", "qSel", "status"), 0)
    assert not sel1["status"][1:].any() and not (out1["status"][1:] & ~64).any()
    assert not _diff(sel1, sel0, SEL_KEYS + ("ztUsed", "status"), slice(1, None)) and not _diff(out1, out0, KEYS, slice(1, None))
