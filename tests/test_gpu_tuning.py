"""-m gpu: per-car controller tuning (lmpc_tuning_set) -- cost weights and bounds of every problem from its own row.

The method is the lap tables' (tests/test_gpu_table_routes.py): the reference of a row is a context created with that row as its config (an "own context"), run
at the SAME batch size on the same stores and problems, and the tuned context must give its BITS -- xPred, uPred, slack, lambd, ztNext, ztuNext, mu, status and
iters, nothing masked beyond LMPC_ST_INEXACT.  Problem b gets row SIX[(b + b // 6) % 6] (tests/tuning_cases.py), so that all 36 (problem, row) pairs occur.
Stores: the PID lap four times in both ("pid4"); problems: common.synthetic_inputs.  The rows and what the CPU says about them: tests/tuning_cases.py."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import tuning_cases as tc
from tests.test_gpu_routes import _knobs, _routes

pytestmark = pytest.mark.gpu

KEYS = ("xPred", "uPred", "slack", "lambd", "ztNext", "ztuNext", "mu", "status", "iters")
MPC_KEYS = ("xPred", "uPred", "slack", "ztNext", "ztuNext", "mu", "status", "iters")
DEV_KEYS = tuple(k for k in KEYS if k != "mu")                        # (step_dev_buffers(diagnostics=False) leaves mu NULL)
BATCH = {64: 66, 300: 300, 600: 600, 1100: 1098}                       # the batches of _routes -> multiples of six, as tests/test_gpu_table_routes.py moves them
FAR = 100 * common.TOL_XU


@pytest.fixture(scope="module")
def g(built):
    return common.load_lmpc_golden()


def _step(ctx, p):
    return ctx.step_batch(p["x0"], p["xLin"], p["uLin"], p["uOld"], zt=p["zt"] if ctx.S else None, timeStep=p["timeStep"] if ctx.S else None)


def _diff(a, b, keys, rows=slice(None)):
    return [k for k in keys if not np.array_equal(np.asarray(a[k])[rows], np.asarray(b[k])[rows])]


def _xu(out, rows=slice(None)):
    B = out["xPred"].shape[0]
    return np.concatenate([out["xPred"].reshape(B, -1), out["uPred"].reshape(B, -1)], axis=1)[rows]


def _problems(g, N, B):
    return common.synthetic_inputs(g, N, B)


class _Set:
    """A context with the default tuning as its config (the one that gets the rows) and one own context per row name, all with the same stores."""

    def __init__(self, g, N, max_batch, names=tc.SIX, runtime=False, knobs=None, **kw):
        from racinglmpc_amd import _capi
        self.names, self.all, self.owns = tuple(names), [], []
        self.table = tc.rows(self.names, N)

        def make(name):
            cfg, _ = tc.config(g, name, N, max_batch=max_batch, **kw)
            with _knobs(knobs or {}):
                c = _capi.Context(cfg, runtime_kernel=runtime)
            self.all.append(c)
            assert c.solver_kind == (2 if runtime else 0)
            tc.fill(c, g)
            return c
        try:
            self.ctx = make("R0")
            self.owns = [make(n) for n in self.names]
        except Exception:
            self.close()
            raise

    def use(self, B):
        rb = tc.row_index(B, len(self.names))
        self.ctx.tuning_set(self.table[rb])
        return rb

    def close(self):
        for c in self.all:
            c.close()


def _cell(st, p, B, waves, what, step=_step, keys=KEYS):
    """One launch of the tuned context on its route, and every problem against the own context of its row at the same batch: (outputs, failures)."""
    rb = st.use(B)
    assert st.ctx.solver_waves(B) == waves and all(o.solver_waves(B) == waves for o in st.owns), (what, st.ctx.solver_waves(B), waves)
    out = step(st.ctx, p)
    fails = []
    if (out["status"] & ~64).any():
        fails.append("%s: status %s" % (what, np.unique(out["status"], return_counts=True)))
    refs = [step(own, p) for own in st.owns]
    for r, ref in enumerate(refs):
        mine = np.where(rb == r)[0]
        bad = _diff(out, ref, keys, mine)
        if bad:
            fails.append("%s, row %s: %s differ from the context created with that row" % (what, st.names[r], ", ".join(bad)))
        # (the comparison tells the rows apart: the same problems on the next row's context end elsewhere)
        assert _diff(out, refs[(r + 1) % len(refs)], ("xPred", "uPred"), mine), (what, r)
    return out, fails


# ---- 1. defaults
def test_defaults_give_the_bits_of_the_untouched_context(g):
    """n = 0, and n = 1 with the config's own row, give the bits of a context that never saw lmpc_tuning_set, at B = 6; after set(rows); set(None) the bits return,
    and tuning() reports what set received."""
    from racinglmpc_amd import _capi
    B = 6
    p = _problems(g, 12, B)
    cfg, _ = tc.config(g, "R0", max_batch=B)
    with _capi.Context(cfg) as fresh, _capi.Context(cfg) as ctx:
        tc.fill(fresh, g); tc.fill(ctx, g)
        ref = _step(fresh, p)
        assert not (ref["status"] & ~64).any()
        assert ctx.tuning().shape == (0, 98)
        ctx.tuning_set(None)
        assert not _diff(_step(ctx, p), ref, KEYS + ("A", "B", "C", "ssSel", "qSel", "sTerm", "resid"))
        own = _capi.tuning_rows(cfg, 1)
        ctx.tuning_set(own)
        assert np.array_equal(ctx.tuning(), own)
        assert not _diff(_step(ctx, p), ref, KEYS + ("A", "B", "C", "ssSel", "qSel", "sTerm", "resid"))
        rows = tc.rows(tc.SIX)
        ctx.tuning_set(rows)
        assert np.array_equal(ctx.tuning(), rows)
        moved = _step(ctx, p)
        assert _diff(moved, ref, ("xPred",), slice(1, None)) and not _diff(moved, ref, KEYS, 0)          # (problem 0 has row R0)
        ctx.tuning_set(None)
        assert ctx.tuning().shape == (0, 98)
        assert not _diff(_step(ctx, p), ref, KEYS + ("sTerm", "resid"))


# ---- 2. own contexts on every route; 3. the oracle
_ORACLE = {}


def _oracle36(g, N=12):
    """The oracle's certified optima of the first 36 problems under the row of each (per row group: oracle_pool.oracle_batch), before any HIP context of the test."""
    from tests import oracle_pool
    if N not in _ORACLE:
        p = _problems(g, N, 36)
        rb = tc.row_index(36)
        pid = (np.array(g["xPID"]), np.array(g["uPID"]))
        res = {}
        for r, name in enumerate(tc.SIX):
            mine = [int(b) for b in np.where(rb == r)[0]]
            for rec in oracle_pool.oracle_batch(tc.params(name, N), np.array(g["track"]), float(g["trackLength"]), [pid] * 4, N, p, mine, solve_idx=mine):
                res[rec["b"]] = rec
        _ORACLE[N] = res
    return _ORACLE[N]


def _against_oracle(out, res, N, what):
    from tests import kkt_batch
    nxu = 6 * (N + 1) + 2 * N
    rb = tc.row_index(36)
    worst = 0.0
    for b, r in res.items():
        assert r["cert"] < 1e-7 and r["cert2"] < 1e-8, (what, b, r["cert"], r["cert2"])
        w = _xu(out, b)
        worst = max(worst, min(float(np.abs(w - o[:nxu]).max()) for o in (r["opt"], r["opt2"])))
    wk = 0.0
    for k, name in enumerate(tc.SIX):
        m = np.where(rb == k)[0]
        c = kkt_batch.certificate(tc.params(name, N), out["A"][m], out["B"][m], out["C"][m], out["x0_in"][m], out["uOld_in"][m], out["xPred"][m], out["uPred"][m],
                                  out["slack"][m], out["mu"][m], out["ssSel"][m], out["qSel"][m], out["lambd"][m], out["sTerm"][m])
        wk = max(wk, float(np.max(c["worst"])))
    print("%s: 36 problems against the oracle: worst |xu - z*| %.2e, worst KKT certificate %.2e" % (what, worst, wk))
    return worst, wk


CELLS = [(12, name) for name in ("4 waves", "2 waves", "1 wave", "runtime kernel")] + [(14, "4 waves"), (40, "4 waves"), (40, "1 wave, [A|B] global"), (40, "runtime kernel")]


@pytest.mark.parametrize("N,route", CELLS, ids=["N%d-%s" % (n, r.replace(" ", "_").replace(",", "").replace("[A|B]", "AB")) for n, r in CELLS])
def test_every_route_serves_the_rows(g, N, route):
    """step_batch with rows r(b) on a route of tests/test_gpu_routes._routes(N), its batch moved to a multiple of six (66, 300, 1098): every problem equals, bit for
    bit, the context created with its row.  N = 12: four of the six routes of _routes(12); the two LMPC_FUSE=1 routes are
    test_the_fused_step_is_not_taken_with_rows.  N = 12, four waves: the first 36 problems also lie within TOL_XU of the oracle's certified optimum for the QPParams of
    their row, and their KKT certificate (tests/kkt_batch.py, per row group) is below TOL_KKT."""
    name, B0, waves, knobs, rt, fused = [r for r in _routes(N) if r[0] == route][0]
    B = BATCH[B0]
    oracle = _oracle36(g, N) if (N, route) == (12, "4 waves") else None          # (forked workers: before the first HIP context of this test)
    p = _problems(g, N, B)
    st = _Set(g, N, B, runtime=rt, knobs=knobs)
    try:
        what = "N = %d, %s, batch %d" % (N, name, B)
        assert st.ctx.solver_kind == (2 if rt else 0)
        out, fails = _cell(st, p, B, waves, what)
        if oracle is not None:
            full = st.ctx.step_batch(p["x0"], p["xLin"], p["uLin"], p["uOld"], zt=p["zt"], timeStep=p["timeStep"])
            full["x0_in"], full["uOld_in"] = p["x0"], p["uOld"]
            worst, wk = _against_oracle(full, oracle, N, what)
            if not worst < common.TOL_XU:
                fails.append("%s: |xu - z*| = %.2e against the oracle" % (what, worst))
            if not wk <= common.TOL_KKT:
                fails.append("%s: KKT certificate %.2e" % (what, wk))
    finally:
        st.close()
    assert not fails, "\n".join(fails)


FUSED = ("LMPC_FUSE=1", "runtime kernel + LMPC_FUSE=1")      # the two routes of _routes(12) that CELLS leaves to the test below


@pytest.mark.parametrize("route", FUSED, ids=["fuse", "runtime_kernel_fuse"])
def test_the_fused_step_is_not_taken_with_rows(g, route):
    """The remaining routes of _routes(12): contexts created under LMPC_FUSE=1, batch 1098 (one wave per QP).  Without rows the knob is in force -- the fused step
    launches no regression kernel (the runtime kernel ignores the knob: one launch) --, with rows r(b) the two-kernel step runs (one regression launch) and every
    problem equals, bit for bit, the context created with its row and, in every output, a tuned context created without the knob; after set(None) the same context
    takes the fused step again and returns the bits it gave before."""
    from racinglmpc_amd import _capi
    name, B0, waves, knobs, rt, fused = [r for r in _routes(12) if r[0] == route][0]
    assert knobs == {"LMPC_FUSE": "1"} and fused == (not rt)
    B = BATCH[B0]
    p = _problems(g, 12, B)
    st = _Set(g, 12, B, runtime=rt, knobs=knobs)
    try:
        ctx = st.ctx
        n_reg = lambda: int(ctx.stats().n_regress)
        ctx.reset_stats(); plain = _step(ctx, p)
        assert n_reg() == (0 if fused else 1), n_reg()                    # the knob is in force on this context
        ctx.reset_stats()
        out, fails = _cell(st, p, B, waves, "N = 12, %s, batch %d" % (name, B))
        assert n_reg() == 1, n_reg()                                      # rows in force: the two-kernel step
        cfg, _ = tc.config(g, "R0", 12, max_batch=B)
        with _capi.Context(cfg, runtime_kernel=rt) as noknob:              # (created without the knob)
            tc.fill(noknob, g)
            noknob.tuning_set(st.table[tc.row_index(B)])
            bad = _diff(out, _step(noknob, p), KEYS + ("A", "B", "C", "ssSel", "qSel", "sTerm", "resid"))
        if bad:
            fails.append("%s differ from a tuned context created without LMPC_FUSE" % ", ".join(bad))
        ctx.tuning_set(None)
        ctx.reset_stats(); back = _step(ctx, p)
        assert n_reg() == (0 if fused else 1), n_reg()                    # no rows: the fused step again
        bad = _diff(back, plain, KEYS + ("sTerm", "resid"))
        if bad:
            fails.append("after set(None): %s differ from the step before the rows" % ", ".join(bad))
    finally:
        st.close()
    assert not fails, "\n".join(fails)


def test_device_path_equals_own_contexts(g):
    """step_batch_dev at 66 with rows r(b): the outputs of the own contexts' step_batch."""
    B = 66
    p = _problems(g, 12, B)
    st = _Set(g, 12, B)

    def dev(ctx, q):
        if ctx is not st.ctx:
            return _step(ctx, q)
        args, keep = ctx.step_dev_buffers(dict(q, hasPred=np.zeros(B, np.int32), xPredPrev=np.zeros((B, 13, 6))))
        try:
            ctx.step_batch_dev(B, args)
            return ctx.step_dev_fetch(args, B)
        finally:
            for a in keep:
                ctx.dev_free(a)
    try:
        out, fails = _cell(st, p, B, 4, "step_batch_dev, batch 66", step=dev)
    finally:
        st.close()
    assert not fails, "\n".join(fails)


@contextlib.contextmanager
def _retry_ctx(g, B, rows):
    """A max_iter = 7 context (tests/test_gpu_retry.py) with the stores; rows: what it is tuned with from the start."""
    from racinglmpc_amd import _capi
    cfg, _ = tc.config(g, "R0", max_batch=B, max_iter=7)
    ctx = _capi.Context(cfg)
    try:
        tc.fill(ctx, g)
        ctx.tuning_set(rows)
        yield ctx
    finally:
        ctx.close()


def test_retry_pass_and_a_set_before_the_deferred_retry(g):
    """max_iter = 7, batch 66, rows r(b): some problems end at the iteration limit, the retry pass (the EQ per-problem-rows instantiation) runs, and every problem
    equals the max_iter = 7 context created with its row.  Device path: a launch with rows T1 stays pending its retry pass, the context gets T2 (every problem's row
    changed), a second launch runs on other buffers; the first equals a context that only ever had T1, the second one that only ever had T2 -- `set` resolved the
    pending launch against the image of ITS launch before it overwrote the image."""
    from racinglmpc_amd import _capi
    B = 66
    p = _problems(g, 12, B)
    rb = tc.row_index(B)
    T1 = tc.rows(tc.SIX)[rb]; T2 = tc.rows(tc.SIX)[(rb + 1) % 6]
    st = _Set(g, 12, B, max_iter=7)
    try:
        st.use(B)
        st.ctx.reset_stats()
        ref1 = _step(st.ctx, p)
        hit = (ref1["status"] & _capi.ST_MAXITER) != 0
        print("max_iter = 7: %d of %d at the limit after the retry pass, %d clean" % (hit.sum(), B, (ref1["status"] == 0).sum()))
        assert st.ctx.stats().n_retry == 1 and hit.any() and (ref1["status"] == 0).any()
        fails = []
        for r, own in enumerate(st.owns):
            own.reset_stats()
            ref = _step(own, p)
            bad = _diff(ref1, ref, KEYS, np.where(rb == r)[0])
            if bad:
                fails.append("row %s: %s differ from the context created with that row" % (tc.SIX[r], ", ".join(bad)))
        assert not fails, "\n".join(fails)
    finally:
        st.close()
    with _retry_ctx(g, B, T2) as c:
        ref2 = _step(c, p)
    assert _diff(ref1, ref2, ("xPred",))
    zero = dict(hasPred=np.zeros(B, np.int32), xPredPrev=np.zeros((B, 13, 6)))
    with _retry_ctx(g, B, T1) as ctx:
        a1, keep1 = ctx.step_dev_buffers(dict(p, **zero), diagnostics=False); a2, keep2 = ctx.step_dev_buffers(dict(p, **zero), diagnostics=False)
        try:
            ctx.step_batch_dev(B, a1)
            assert ctx.stats().n_retry == 0                                # pending
            ctx.tuning_set(T2)
            assert ctx.stats().n_retry == 1                                # the image is about to be overwritten: launch 1 got its pass first
            ctx.step_batch_dev(B, a2)
            out1 = ctx.step_dev_fetch(a1, B); out2 = ctx.step_dev_fetch(a2, B)
            assert ctx.stats().n_retry == 2
        finally:
            for q in keep1 + keep2:
                ctx.dev_free(q)
    bad1, bad2 = _diff(out1, ref1, DEV_KEYS), _diff(out2, ref2, DEV_KEYS)
    assert not bad1, "the pending launch's %s differ from a context that only ever had its rows" % bad1
    assert not bad2, "the second launch's %s differ from a context that only ever had the second rows" % bad2


# ---- 4. every field reaches the kernel
def test_every_field_reaches_the_kernel(g):
    """B = 6, all six problems on one single-field row: equal in bits to the context created with that row, and more than 100 x TOL_XU from the output of the row it
    was derived from (R0; the Qslack rows: R5a, which has their narrow lane) on every problem."""
    B = 6
    p = _problems(g, 12, B)
    names = tuple(sorted({n for pair in tc.FIELD_ROWS.values() for n in pair}))
    st = _Set(g, 12, B, names=names)
    try:
        own = {n: _step(c, p) for n, c in zip(names, st.owns)}
        fails = []
        for field, (row, against) in tc.FIELD_ROWS.items():
            st.ctx.tuning_set(tc.rows((row,)))
            out = _step(st.ctx, p)
            if (out["status"] & ~64).any():
                fails.append("%s: status %s" % (field, out["status"]))
            bad = _diff(out, own[row], KEYS)
            if bad:
                fails.append("%s (row %s): %s differ from the context created with that row" % (field, row, ", ".join(bad)))
            d = np.abs(_xu(out) - _xu(own[against])).max(axis=1)
            print("%-10s row %-4s against %-4s: |xu - xu'| per problem %s" % (field, row, against, np.array2string(d, precision=2)))
            if not (d > FAR).all():
                fails.append("%s (row %s): within %.1e of %s on problem(s) %s" % (field, row, FAR, against, np.where(d <= FAR)[0].tolist()))
    finally:
        st.close()
    assert not fails, "\n".join(fails)


# ---- 5. explicit matrices
def test_assemble_batch_builds_problem_b_from_row_b(g):
    """lmpc_assemble_batch with six rows: P, q, A, l, u of problem b equal oracle.assemble_lmpc_qp with row b, exactly (tests/test_gpu_parity.py's tolerance)."""
    from oracle import lmpc_oracle as orc
    from racinglmpc_amd import _capi
    B = 6
    cfg, _ = tc.config(g, "R0", max_batch=B)
    data = tc.qp_data(g, "pid4", range(B))
    arr = lambda k: np.stack([d[k] for d in data])
    with _capi.Context(cfg) as ctx:
        ctx.tuning_set(tc.rows(tc.SIX))
        P, q, A, l, u = ctx.assemble_batch(arr("A"), arr("B"), arr("C"), arr("x0"), arr("uOld"), np.transpose(arr("SS"), (0, 2, 1)), arr("Qsel"))
        with pytest.raises(_capi.LmpcError):
            ctx.assemble_batch(arr("A")[:5], arr("B")[:5], arr("C")[:5], arr("x0")[:5], arr("uOld")[:5], np.transpose(arr("SS"), (0, 2, 1))[:5], arr("Qsel")[:5])
    for b, name in enumerate(tc.SIX):
        d = data[b]
        Pr, qr, Ar, lr, ur = orc.assemble_lmpc_qp(tc.params(name), d["A"], d["B"], d["C"], d["x0"], d["uOld"], d["SS"], d["Qsel"])
        for got, ref, what in ((P[b], Pr, "P"), (q[b], qr, "q"), (A[b], Ar, "A"), (l[b], lr, "l"), (u[b], ur, "u")):
            assert np.array_equal(got, np.asarray(ref)), (name, what, float(np.abs(got - np.asarray(ref)).max()))


# ---- 6. both tables and tuning
def test_both_lap_tables_and_rows_together(g):
    """ss_set_lap_table + model_set_lap_table + rows at batch 66 (the fixture of tests/ss_table_cases.py): problem b has safe-set row, regression row and tuning row
    r(b); its reference is a context created with tuning row r(b) that holds only the laps of safe-set row r(b)."""
    from racinglmpc_amd import _capi
    from tests import ss_table_cases as cases
    B, N = 66, 12
    p = cases.problems(g, B, N)
    rb = tc.row_index(B)
    cfg, _ = tc.config(g, "R0", max_batch=B)
    step = lambda c: c.step_batch(p["x0"], p["xLin"], p["uLin"], p["uOld"], p["zt"], p["xPredPrev"], p["hasPred"], p["timeStep"])
    fails = []
    with _capi.Context(cfg) as ctx:
        cases.fill_table_context(ctx, g)
        stored = cases.read_laps(ctx); lt = [s[3] for s in stored]
        ctx.ss_set_lap_table(cases.ROWS4[rb], cases.LAST4[rb])
        ctx.model_set_lap_table(np.zeros((B, 4), np.int32) + np.arange(4, dtype=np.int32)[None, :])      # (every car names the four regression laps itself)
        ctx.tuning_set(tc.rows(tc.SIX)[rb])
        out = step(ctx)
        assert not (out["status"] & ~64).any(), np.unique(out["status"])
        for r, name in enumerate(tc.SIX):
            ocfg, _ = tc.config(g, name, max_batch=B)
            with _capi.Context(ocfg) as own:
                cases.fill_own_context(own, g, stored, cases.own_order(cases.ROWS4[r], cases.LAST4[r], lt))
                bad = _diff(out, step(own), KEYS + ("ssSel", "qSel", "A", "B", "C"), np.where(rb == r)[0])
            if bad:
                fails.append("row %d / %s: %s differ from the own context" % (r, name, ", ".join(bad)))
    assert not fails, "\n".join(fails)


# ---- 7. plain MPC
def _mpc_ctx(g, gl, B, xref0=0.8, bx=2.0, slacks=True):
    from racinglmpc_amd import _capi
    cfg, par = common.mpc_config(g, 12, max_batch=B, bx=bx, slacks=slacks)
    cfg.xRef[0] = float(xref0)
    ctx = _capi.Context(cfg)
    ctx.model_add_trajectory(np.array(gl["xPID"]), np.array(gl["uPID"]))
    return ctx, cfg


def test_plain_mpc_rows(g):
    """numSS_it = 0 (the S = 0 per-problem-rows instantiations), the ltvmpc_n12 fixture, B = 6: rows with xRef[0] in {0.6, 0.8, 1.0} x bx in {2, 0.3} give the bits of
    contexts created with those values.  With slacks = 0, rows that differ only in Qslack give equal bits (the rows' Qslack is ignored)."""
    from racinglmpc_amd import _capi
    gl = common.load_ltv_golden()
    B = 6
    p = dict(x0=gl["x0"][:B], xLin=gl["xLin"][:B], uLin=gl["uLin"][:B], uOld=gl["OldInput"][:B])
    grid = [(v, w) for v in (0.6, 0.8, 1.0) for w in (2.0, 0.3)]
    ctx, cfg = _mpc_ctx(g, gl, B)
    try:
        rows = _capi.tuning_rows(cfg, B, xRef=np.array([[v, 0, 0, 0, 0, 0] for v, w in grid]), bx=np.array([[w, w] for v, w in grid]))
        ctx.tuning_set(rows)
        out = _step(ctx, p)
        assert not (out["status"] & ~64).any(), out["status"]
        refs = []
        for b, (v, w) in enumerate(grid):
            own, _ = _mpc_ctx(g, gl, B, v, w)
            try:
                refs.append(_step(own, p))
            finally:
                own.close()
            assert not _diff(out, refs[-1], MPC_KEYS, b), (b, v, w, _diff(out, refs[-1], MPC_KEYS, b))
        assert _diff(refs[0], refs[2], ("xPred",))                                                    # (the target speed moves the answer on these problems)
        print("bx = 0.3 against bx = 2 at xRef[0] = 0.6: |xPred - xPred'| = %.2e" % float(np.abs(refs[0]["xPred"] - refs[1]["xPred"]).max()))
    finally:
        ctx.close()
    hard, hcfg = _mpc_ctx(g, gl, B, slacks=False)
    try:
        ref = _step(hard, p)
        qs = np.array([[0.0, 50.0], [5.0, 25.0], [20.0, 100.0], [1.0, 0.0], [100.0, 1.0], [0.0, 0.0]])
        hard.tuning_set(_capi.tuning_rows(hcfg, B, Qslack=qs))
        assert not _diff(_step(hard, p), ref, MPC_KEYS)
    finally:
        hard.close()


# ---- 8. sessions
def test_lmpc_session_with_three_rows(g):
    """lmpc_rollout_begin with 3 cars, 3 rows, 30 steps, device noise: X, U logs, doneAt and status are bit for bit those of one-car sessions on contexts created
    with the car's row.  A `set` between two lmpc_rollout_run calls reaches the next step and not the ones already logged; a `set` with the wrong n is refused before
    any launch of the step."""
    from racinglmpc_amd import _capi
    names = ("R1", "R3", "R5"); after = ("R2", "R3", "R0")
    t0 = np.array([100, 104, 108])
    x0 = np.array(g["all_x0"])[t0]; xl = np.array(g["all_xLin"])[t0]; ul = np.array(g["all_uLin"])[t0]
    T, SEED, CUT = 30, 78, 12
    cfg, _ = tc.config(g, "R0", max_batch=4)

    def fill(c):
        model, ss = common.stores_at_lap(g, 4)
        for x, u in model:
            c.model_add_trajectory(x, u)
        for x, u, _ in ss:
            c.ss_add_trajectory(x, u)
    with _capi.Context(cfg) as ctx:
        fill(ctx)
        ctx.tuning_set(tc.rows(names))
        ctx.rollout_set_noise(True, SEED, 0, 0)
        ctx.rollout_begin(x0, x0, xl, ul, None, T_max=T)
        t, _ = ctx.rollout_run(CUT)
        assert t == CUT
        ctx.tuning_set(tc.rows(names[:2]))
        with pytest.raises(_capi.LmpcError) as e:
            ctx.rollout_run(T)
        assert "holds 2 rows" in str(e.value) and "B = 3" in str(e.value)
        ctx.tuning_set(tc.rows(after))
        t, _ = ctx.rollout_run(T)
        assert t == T                                                 # (the refused call took no step)
        X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
        ctx.rollout_end()
    assert not (st & ~64).any(), st
    for b in range(3):
        ocfg, _ = tc.config(g, names[b], max_batch=4)
        with _capi.Context(ocfg) as own:
            fill(own)
            own.rollout_set_noise(True, SEED, 0, b)
            own.rollout_begin(x0[b:b + 1], x0[b:b + 1], xl[b:b + 1], ul[b:b + 1], None, T_max=T)
            own.rollout_run(CUT)
            own.tuning_set(tc.rows(after[b:b + 1]))                   # (the own context's second half: the same row through the same entry point, n = 1)
            to, _ = own.rollout_run(T)
            Xo, Uo, _, done_o, st_o, _, _ = own.rollout_fetch(0, to)
            own.rollout_end()
        assert to == T and done_o[0] == done[b] and st_o[0] == st[b], b
        assert np.array_equal(Xo[:, 0], X[:, b]) and np.array_equal(Uo[:, 0], U[:, b]), b
        if names[b] != after[b]:
            # ... and the rows did change the drive: a one-car session that keeps the first row leaves the logged steps equal and the later ones not
            with _capi.Context(ocfg) as own:
                fill(own)
                own.rollout_set_noise(True, SEED, 0, b)
                own.rollout_begin(x0[b:b + 1], x0[b:b + 1], xl[b:b + 1], ul[b:b + 1], None, T_max=T)
                to, _ = own.rollout_run(T)
                Xk, Uk, _, _, _, _, _ = own.rollout_fetch(0, to)
                own.rollout_end()
            assert np.array_equal(Uk[:CUT, 0], U[:CUT, b]) and not np.array_equal(Uk[CUT:, 0], U[CUT:, b]), b


def test_ltv_mpc_session_with_a_target_speed_per_car(g):
    """The LTV form of lmpc_rollout_begin_mpc with 3 cars and xRef[0] = 0.6, 0.8, 1.0: logs, doneAt and status of one-car sessions on contexts created with that
    target speed."""
    from racinglmpc_amd import _capi
    gl = common.load_ltv_golden()
    B, T = 3, 20
    vs = (0.6, 0.8, 1.0)
    x0 = gl["x0"][:B]; xl = gl["xLin"][:B]; ul = gl["uLin"][:B]
    noise = np.random.default_rng(7).standard_normal((T, B, 3))
    ctx, cfg = _mpc_ctx(g, gl, B)
    try:
        ctx.tuning_set(_capi.tuning_rows(cfg, B, xRef=np.array([[v, 0, 0, 0, 0, 0] for v in vs])))
        ctx.rollout_begin_mpc(x0, x0, noise, xLin0=xl, uLin0=ul)
        t, _ = ctx.rollout_run(T)
        X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
        ctx.rollout_end()
    finally:
        ctx.close()
    assert t == T and not (st & ~64).any(), (t, st)
    for b, v in enumerate(vs):
        own, _ = _mpc_ctx(g, gl, B, v)
        try:
            own.rollout_begin_mpc(x0[b:b + 1], x0[b:b + 1], np.ascontiguousarray(noise[:, b:b + 1]), xLin0=xl[b:b + 1], uLin0=ul[b:b + 1])
            to, _ = own.rollout_run(T)
            Xo, Uo, Go, done_o, st_o, _, _ = own.rollout_fetch(0, to)
            own.rollout_end()
        finally:
            own.close()
        assert done_o[0] == done[b] and st_o[0] == st[b] and np.array_equal(Xo[:, 0], X[:, b]) and np.array_equal(Uo[:, 0], U[:, b]) and np.array_equal(Go[:, 0], G[:, b]), b
    assert not np.array_equal(U[:, 0], U[:, 1])


def test_lti_mpc_session_with_a_target_speed_per_car(g):
    """The LTI form of lmpc_rollout_begin_mpc (no regression launch: the S = 0 per-problem-rows kernels on A_lti / B_lti) with 3 cars, each its own model and
    xRef[0] = 0.6, 0.8, 1.0: logs, doneAt and status of one-car sessions on contexts created with that target speed."""
    from racinglmpc_amd import _capi
    gl = common.load_ltv_golden()
    B, T = 3, 20
    vs = (0.6, 0.8, 1.0)
    x0 = gl["x0"][:B]
    A = np.ascontiguousarray(gl["A"][:B, 0]); Bm = np.ascontiguousarray(gl["B"][:B, 0])
    noise = np.random.default_rng(8).standard_normal((T, B, 3))
    ctx, cfg = _mpc_ctx(g, gl, B)
    try:
        ctx.tuning_set(_capi.tuning_rows(cfg, B, xRef=np.array([[v, 0, 0, 0, 0, 0] for v in vs])))
        ctx.reset_stats()
        ctx.rollout_begin_mpc(x0, x0, noise, A=A, B=Bm)
        t, _ = ctx.rollout_run(T)
        assert int(ctx.stats().n_regress) == 0
        X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
        ctx.rollout_end()
    finally:
        ctx.close()
    assert t == T and not (st & ~64).any(), (t, st)
    for b, v in enumerate(vs):
        own, _ = _mpc_ctx(g, gl, B, v)
        try:
            own.rollout_begin_mpc(x0[b:b + 1], x0[b:b + 1], np.ascontiguousarray(noise[:, b:b + 1]), A=A[b:b + 1], B=Bm[b:b + 1])
            to, _ = own.rollout_run(T)
            Xo, Uo, Go, done_o, st_o, _, _ = own.rollout_fetch(0, to)
            own.rollout_end()
        finally:
            own.close()
        assert done_o[0] == done[b] and st_o[0] == st[b] and np.array_equal(Xo[:, 0], X[:, b]) and np.array_equal(Uo[:, 0], U[:, b]) and np.array_equal(Go[:, 0], G[:, b]), b
    assert not np.array_equal(U[:, 0], U[:, 2])


# ---- 9. refusals and isolation
def test_refusals_keep_the_rows_and_the_context(g):
    """B != n is LMPC_E_ARG with a message naming both numbers, and the next correct call works; every invalid row keeps the rows in force."""
    from racinglmpc_amd import _capi
    B = 6
    p = _problems(g, 12, B)
    st = _Set(g, 12, B, names=("R0", "R1"))
    try:
        ctx, lib = st.ctx, st.ctx.lib
        rows = tc.rows(tc.SIX)
        ctx.tuning_set(rows)
        p5 = {k: v[:5] for k, v in p.items()}
        with pytest.raises(_capi.LmpcError) as e:
            _step(ctx, p5)
        assert "lmpc_tuning_set holds 6 rows" in str(e.value) and "B = 5" in str(e.value)
        out = _step(ctx, p)
        assert not _diff(out, _step(st.owns[1], p), KEYS, 1)              # (problem 1 has row R1)
        sl = _capi.TUNING_FIELDS

        def bad_row(field, i, v, j=None):
            r = rows[:1].copy()
            f = r[0, sl[field]]
            f[i] = v
            if j is not None:
                f[j] = v
            return r
        nonsym = rows[:1].copy(); nonsym[0, sl["Q"]][1] = 1.0
        nonsymR = rows[:1].copy(); nonsymR[0, sl["R"]][1] = 1.0
        nonsymQf = rows[:1].copy(); nonsymQf[0, sl["Qf"]][6] = 1.0
        for n, r in ((1, bad_row("xRef", 0, np.nan)), (1, bad_row("bu", 0, np.inf)), (1, nonsym), (1, nonsymR), (1, nonsymQf), (1, bad_row("dR", 1, -1.0)),
                     (1, bad_row("Qslack", 0, -1.0)), (1, bad_row("QtermSlack", 3, 0.0)), (-1, rows[:1]), (B + 1, np.tile(rows[:1], (B + 1, 1))), (1, None)):
            rc = lib.lmpc_tuning_set(ctx._h, n, None if r is None else np.ascontiguousarray(r).ctypes.data)
            assert rc == -1 and np.array_equal(ctx.tuning(), rows), (n, r)
        n = C.c_int(-1); two = np.zeros((2, 98))
        assert lib.lmpc_tuning_get(ctx._h, C.byref(n), two.ctypes.data, 2) == 0 and n.value == 6 and np.array_equal(two, rows[:2])
        assert not _diff(_step(ctx, p), out, KEYS)
    finally:
        st.close()


def test_a_car_without_an_interior_start_is_flagged_alone(g):
    """One car with bu[0] = 0 carries LMPC_ST_NOT_INTERIOR alone; the other five keep the bits of the contexts created with their rows."""
    from racinglmpc_amd import _capi
    B = 6
    p = _problems(g, 12, B)
    st = _Set(g, 12, B)
    try:
        rows = tc.rows(tc.SIX)
        rows[2, _capi.TUNING_FIELDS["bu"]] = [0.0, 0.5, 10.0, 10.0]
        st.ctx.tuning_set(rows)
        out = _step(st.ctx, p)
        assert out["status"][2] & _capi.ST_NOT_INTERIOR and not (np.delete(out["status"], 2) & ~64).any(), out["status"]
        for b in (0, 1, 3, 4, 5):
            assert not _diff(out, _step(st.owns[b], p), KEYS, b), b
    finally:
        st.close()


def test_the_condensed_kernel_is_not_taken_with_rows(g):
    """LMPC_CD=1 with rows in force runs the ordinary kernels: the outputs equal, bit for bit, those of a context created without the knob.  Run against the opt-in
    flavour that carries the condensed kernel (liblmpc_hip_cd.so, which build() keeps current; tests/test_gpu_condensed.py runs against it too), where the knob is
    shown to be in force first: without rows the same context gives another iterate (another QP method) than the ordinary kernels.  Where that library has not been
    built the product library stands in, and the test then only shows that the knob is inert there."""
    import os
    from racinglmpc_amd import _capi
    cd_lib = os.path.join(common.ROOT, "racinglmpc_amd", "liblmpc_hip_cd.so")
    have_cd = os.path.exists(cd_lib)
    keep = (_capi.LIB_PATH, _capi._lib)
    if have_cd:
        _capi.LIB_PATH, _capi._lib = cd_lib, None
    B = 6
    p = _problems(g, 12, B)
    out, plain = {}, {}
    try:
        assert _capi.load().lmpc_version() >= 108
        cfg, _ = tc.config(g, "R0", max_batch=B)
        for cd in (False, True):
            with _knobs({"LMPC_CD": "1"} if cd else {}):
                ctx = _capi.Context(cfg)
            try:
                tc.fill(ctx, g)
                assert ctx.solver_kind == 0
                plain[cd] = _step(ctx, p)
                ctx.tuning_set(tc.rows(tc.SIX))
                out[cd] = _step(ctx, p)
            finally:
                ctx.close()
    finally:
        _capi.LIB_PATH, _capi._lib = keep
    print("condensed flavour: %s; without rows the knob changes %s" % (have_cd, _diff(plain[True], plain[False], ("xPred", "uPred", "iters", "mu"))))
    assert not (plain[True]["status"] & ~64).any() and not (out[True]["status"] & ~64).any()
    if have_cd:
        assert _diff(plain[True], plain[False], ("xPred", "uPred", "iters", "mu"))            # the knob is in force: the condensed kernel ran
    assert not _diff(out[True], out[False], KEYS + ("sTerm", "resid"))
