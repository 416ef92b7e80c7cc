"""-m gpu: laps given back from the lap stores (lmpc_store_retain; Context.store_retain; rollout.PerCarLMPC(prune=True)).

The reference of every case is a context that never held the dropped laps: a fresh one given only the kept laps, in their order, through the host path -- or the same
context before the call, where the call must change nothing that is read.  Everything is compared bit for bit (as int64 words, so that NaN rows and the sign of a zero
count): the rows of both stores, Qfun, LapTime, the regression store's sorted order, the prefilter image, and what a regression, a selection and a step compute
from them; the stores also against tests/store_ref.py after tests/retain_ref.py.  N = 12, the golden config; what needs no device is in tests/test_store_retain_host.py."""
import numpy as np
import pytest

from tests import common, retain_ref, store_ref
from tests import ss_table_cases as sc
from tests import track_cases as tk
from tests.test_gpu_device_commit import _pid, _refused, _same, _same_stores, _stores

pytestmark = pytest.mark.gpu

N = 12
E_ARG, E_STATE = "error -1:", "error -4:"


@pytest.fixture(scope="module")
def g():
    return common.load_lmpc_golden()


def _same_out(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        _same(a[k], b[k], (what, k))


def _tables(ctx):
    rows, last = ctx.ss_lap_table()
    return ctx.model_lap_table(), rows, last


def _same_tables(a, b, what):
    for p, q, k in zip(a, b, ("lap table", "safe-set table", "last")):
        assert (p is None) == (q is None) and (p is None or np.array_equal(p, q)), (what, k, p, q)


# ---- 1
def test_retain_equals_never_having_stored(built, g):
    """Seven entries into both stores of a context that grows in both directions (image rows just under, on and just over the chunk edge, the shortest lap, a tie), one
    kept safe-set lap extended past the line, then four laps of each store kept -- against a fresh context given only those laps through the host path."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=4, max_lap_len=256)
    cars, rows = [0, 1, 2, 3, 4, 4, 0], [1024, 1025, 1026, 2, 300, 300, 40]
    keep_ss, keep_m = [1, 3, 4, 6], [0, 2, 4, 5]
    vt = [0.7, 0.75, 0.8, 0.85, 0.9]
    with _capi.Context(cfg) as A, _capi.Context(cfg) as Bc:
        t = _pid(A, vt, 1100, False)
        assert A.rollout_commit_laps(cars, rows) == (0, 0)
        X, U = A.rollout_fetch(0, t)[:2]
        A.rollout_end()
        ext = (X[300:330, 4].copy(), U[300:330, 4].copy())                                          # rows past lap 4's 300: rows != LapTime
        A.ss_extend_lap(4, *ext)
        ref = store_ref.RefStores.like(cfg)
        for c, T in zip(cars, rows):
            ref.ss_add_trajectory(X[:T, c], U[:T, c]); ref.model_add_trajectory(X[:T, c], U[:T, c])
        ref.ss_extend_lap(4, *ext)
        _same_stores(_stores(A), ref.snapshot(), "before the retain against the restatement")
        ms, mm = A.store_retain(ss=keep_ss, model=keep_m)
        assert ms.dtype == np.int32 and ms.tolist() == [-1, 0, -1, 1, 2, -1, 3] and mm.dtype == np.int32 and mm.tolist() == [0, -1, 1, -1, 2, 3, -1]
        rs, rm = retain_ref.retain(ref, keep_ss, keep_m)
        assert np.array_equal(ms, rs) and np.array_equal(mm, rm)
        for l in keep_ss:
            Bc.ss_add_trajectory(X[:rows[l], cars[l]], U[:rows[l], cars[l]])
        Bc.ss_extend_lap(keep_ss.index(4), *ext)
        for l in keep_m:
            Bc.model_add_trajectory(X[:rows[l], cars[l]], U[:rows[l], cars[l]])
        sa, sb = _stores(A), _stores(Bc)
        assert A.ss_num_laps() == 4 and A.model_num_laps() == 4
        assert [s[3] for s in sa["ss"]] == [1025, 2, 300, 40] and [s[4] for s in sa["ss"]] == [1025, 2, 330, 40]
        assert sa["info"] == [(1024, 2), (1026, 3), (300, 0), (300, 1)]                             # ascending rows, the two 300s in their order
        assert [im[2] for im in sa["image"]] == [1, 2, 1, 1]
        _same_stores(sa, sb, "retain against the fresh context")
        _same_stores(sa, ref.snapshot(), "retain against the restatement")
        xq, uq = X[0:1024:16, 0].copy(), U[0:1024:16, 0].copy()
        assert xq.shape[0] == 64
        for k, (p, r) in enumerate(zip(A.regress_points(xq, uq), Bc.regress_points(xq, uq))):
            _same(p, r, ("regress_points", "ABCs"[k]))
        tb = np.array([5, 12, 20, 26])
        sel = [c.select_batch(X[tb, 0].copy(), X[tb + N + 1, 0].copy()) for c in (A, Bc)]
        for k in _capi.SELECT_OUT_KEYS:
            _same(sel[0][k], sel[1][k], ("select_batch", k))
        # a second retain on the compacted stores, a store emptied, an untouched one
        ms, mm = A.store_retain(ss=[], model=None)
        assert ms.tolist() == [-1, -1, -1, -1] and mm is None and A.ss_num_laps() == 0 and A.model_num_laps() == 4
        s2 = _stores(A)
        assert s2["ss"] == [] and s2["info"] == sa["info"]
        for p, q in zip(s2["model"], sa["model"]):
            _same(p[0], q[0], "regression store after the safe set was emptied"); _same(p[1], q[1], "regression store after the safe set was emptied")


# ---- 2
def test_capacity_comes_back_and_growth_after_a_shrink(built, g):
    """256 laps at max_lap_len = 2048 (the stores and the image compute to about 80 MB), four kept: the device's free memory rises by more than half of what the
    released lap slots compute to (the allocator's granularity and the pooled scratch take the rest of the margin).  Then five more laps: growth from the small
    capacity, contents right."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=4, max_lap_len=2048)
    vt = np.linspace(0.7, 0.9, 8)
    cars = [i % 8 for i in range(256)]; rows = [60 + i % 50 for i in range(256)]
    keep_ss, keep_m = [3, 100, 200, 255], [0, 7, 100, 254]
    with _capi.Context(cfg) as A:
        t = _pid(A, vt, 120, False)
        assert A.rollout_commit_laps(cars, rows) == (0, 0)
        X, U = A.rollout_fetch(0, t)[:2]
        A.rollout_end()
        free0 = _capi.device_memory(0)[0]
        ms, mm = A.store_retain(ss=keep_ss, model=keep_m)
        free1 = _capi.device_memory(0)[0]
        released = (256 - 4) * retain_ref.lap_bytes(2048)
        print("stores of 256 laps: %.1f MB computed; free memory rose by %.1f MB, %.1f MB computed for the released slots" % (256 * retain_ref.lap_bytes(2048) / 2**20, (free1 - free0) / 2**20, released / 2**20))
        assert 75 * 2**20 < 256 * retain_ref.lap_bytes(2048) < 85 * 2**20
        assert free1 - free0 > released // 2, (free0, free1, released)
        assert np.flatnonzero(ms >= 0).tolist() == keep_ss and np.flatnonzero(mm >= 0).tolist() == keep_m
        ref = store_ref.RefStores.like(cfg)
        for l in keep_ss:
            ref.ss_add_trajectory(X[:rows[l], cars[l]], U[:rows[l], cars[l]])
        for l in keep_m:
            ref.model_add_trajectory(X[:rows[l], cars[l]], U[:rows[l], cars[l]])
        _same_stores(_stores(A), ref.snapshot(), "four laps kept against the restatement")
        t = _pid(A, vt, 120, False, seed=12)
        more, mrows = [7, 0, 3, 3, 5], [80, 61, 100, 100, 2]
        assert A.rollout_commit_laps(more, mrows) == (4, 4)                                         # (five laps do not fit the capacity of four: growth after the shrink)
        X2, U2 = A.rollout_fetch(0, t)[:2]
        A.rollout_end()
        for c, T in zip(more, mrows):
            ref.ss_add_trajectory(X2[:T, c], U2[:T, c]); ref.model_add_trajectory(X2[:T, c], U2[:T, c])
        assert A.ss_num_laps() == 9 and A.model_num_laps() == 9
        _same_stores(_stores(A), ref.snapshot(), "five more laps against the restatement")


# ---- 3, 4: tables
ROWS = np.array([[0, 2, 3, 5], [5, 3, 2, 0], [2, 2, 5, 0], [3, 0, 5, 5], [0, 2, 3, 5], [5, 5, 2, 3], [3, 2, 0, 0], [2, 0, 3, 5]], np.int32)
LAST = np.array([5, 2, -1, 3, 2, 5, 0, -1], np.int32)
LAPS = np.array([[1, 4, 6, 9], [9, 6, 4, 3], [3, 3, 1, 6], [4, 4, 4, 4], [9, 1, 3, 6], [6, 9, 9, 1], [1, 3, 4, 6], [3, 9, 1, 4]], np.int32)
KEEP_SS, KEEP_M = [0, 2, 3, 5], [1, 3, 4, 6, 9]


def _table_context(g, max_laps=16):
    """Six safe-set laps (lap 2 extended) and ten regression laps -- four times the PID lap, then the six -- with a lap table and a safe-set table of eight rows."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=max_laps, max_lap_len=1024)
    ctx = _capi.Context(cfg)
    sc.fill_table_context(ctx, g)
    for x, u in sc.fixture_laps(g)[0]:
        ctx.model_add_trajectory(x, u)
    ctx.model_set_lap_table(LAPS); ctx.ss_set_lap_table(ROWS, LAST)
    return ctx


def test_tables_follow(built, g):
    """A lap table and a safe-set table with `last` in force: after the retain the getters return the rows through the map, and a step of 8 problems is bit-identical."""
    p = sc.problems(g, 8)
    ctx = _table_context(g)
    try:
        before = ctx.step_batch(**p)
        print("status of the eight problems:", before["status"])
        assert before["ssSel"].any() and ((before["status"] & ~64) == 0).any(), before["status"]
        ms, mm = ctx.store_retain(ss=KEEP_SS, model=KEEP_M)
        assert ms.tolist() == [0, -1, 1, 2, -1, 3] and mm.tolist() == [-1, 0, -1, 1, 2, -1, 3, -1, -1, 4]
        lt, rows, last = _tables(ctx)
        assert np.array_equal(lt, retain_ref.remap(LAPS, mm)) and np.array_equal(rows, retain_ref.remap(ROWS, ms)) and np.array_equal(last, retain_ref.remap(LAST, ms))
        assert last.tolist() == [3, 1, -1, 2, 1, 3, 0, -1]
        assert ctx.ss_num_laps() == 4 and ctx.model_num_laps() == 5
        _same_out(ctx.step_batch(**p), before, "step after the retain")
        # the laps themselves: lap 2 (extended) is lap 1 now
        assert ctx.ss_lap_rows(1) == ctx.ss_lap_time(1) + 30
    finally:
        ctx.close()


def test_a_refused_retain_changes_nothing(built, g):
    """Lists the library refuses, and a lap that a table row, a `last` entry, the override or the lap table names and the list drops: error -1 with the table, the
    row and the lap named; stores, tables and the following step as before."""
    p = sc.problems(g, 8)
    ctx = _table_context(g, max_laps=4)                   # (grown to 16 by the ten regression laps: a refused call must not shrink it either)
    try:
        before, snap, tabs = ctx.step_batch(**p), _stores(ctx), _tables(ctx)
        msg = _refused(E_ARG, lambda: ctx.store_retain(ss=[0, 2, 3], model=KEEP_M))
        assert "safe-set lap table" in msg and "row 0 names lap 5" in msg, msg
        msg = _refused(E_ARG, lambda: ctx.store_retain(ss=KEEP_SS, model=[1, 3, 4, 9]))
        assert "lap table" in msg and "row 0 names lap 6" in msg, msg
        ctx.ss_set_lap_table(ROWS, np.array([5, 2, -1, 3, 1, 5, 0, -1], np.int32))
        msg = _refused(E_ARG, lambda: ctx.store_retain(ss=KEEP_SS, model=KEEP_M))
        assert "last" in msg and "row 4 names lap 1" in msg, msg
        ctx.ss_set_lap_table(ROWS, LAST)
        ctx.ss_set_selected([0, 2, 3, 4])
        msg = _refused(E_ARG, lambda: ctx.store_retain(ss=KEEP_SS, model=KEEP_M))
        assert "selection override" in msg and "entry 3 names lap 4" in msg, msg
        ctx.ss_set_selected([])
        # lists Context.store_retain would stop in Python, handed to the library itself
        for ss in ([3, 2], [0, 0], [0, 6], [-1, 0]):
            a = np.array(ss, np.int32)
            assert ctx.lib.lmpc_store_retain(ctx._h, a.size, a.ctypes.data, -1, None, None, None) == -1, ss
        with pytest.raises(ValueError):
            ctx.store_retain(ss=[3, 2])
        assert ctx.ss_num_laps() == 6 and ctx.model_num_laps() == 10
        _same_stores(_stores(ctx), snap, "after the refusals"); _same_tables(_tables(ctx), tabs, "after the refusals")
        _same_out(ctx.step_batch(**p), before, "step after the refusals")
    finally:
        ctx.close()


# ---- 5
def _shared_context(g, laps, max_laps=8):
    """Four regression laps (the PID lap) and the listed laps of tests/ss_table_cases.py in the safe set, lap 2 with its extension; no tables."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=max_laps, max_lap_len=1024)
    ctx = _capi.Context(cfg)
    fix, ext = sc.fixture_laps(g)
    for _ in range(4):
        ctx.model_add_trajectory(g["xPID"], g["uPID"])
    for k, l in enumerate(laps):
        ctx.ss_add_trajectory(*fix[l])
        if l == sc.EXTENDED:
            ctx.ss_extend_lap(k, *ext)
    return ctx


def test_shared_safe_set_without_tables(built, g):
    """The numSS_it fastest laps plus the latest kept: the step is what it was.  Then the highest-numbered lap dropped as well: the highest kept one is the latest
    now, and the step is that of a fresh context holding the kept laps."""
    p = sc.problems(g, 8)
    ctx = _shared_context(g, range(6))
    try:
        before = ctx.step_batch(**p)
        assert before["ssSel"].any()
        times = [ctx.ss_lap_time(l) for l in range(6)]
        fastest = sorted(range(6), key=lambda l: times[l])[:4]                                     # (sorted is stable: argsort(LapTime)[0:numSS_it])
        keep = sorted(set(fastest) | {5})
        assert len(keep) == 5 and 5 not in fastest, (times, fastest)                                 # (lap 5 is the slowest: kept as the latest only)
        ms, _ = ctx.store_retain(ss=keep)
        assert ctx.ss_num_laps() == 5 and ctx.model_num_laps() == 4
        _same_out(ctx.step_batch(**p), before, "fastest laps and the latest kept")
        ctx.store_retain(ss=[0, 1, 2, 3])
        fresh = _shared_context(g, keep[:4])
        try:
            _same_stores(_stores(ctx), _stores(fresh), "the highest-numbered lap dropped")
            after = ctx.step_batch(**p)
            _same_out(after, fresh.step_batch(**p), "the highest kept lap is the latest")
            print("the step differs from the one before the latest lap was dropped:", any(not np.array_equal(after[k], before[k]) for k in after))
        finally:
            fresh.close()
    finally:
        ctx.close()


# ---- 6
def test_refused_inside_a_session(built, g):
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=4, max_lap_len=512)
    with _capi.Context(cfg) as A:
        xs, us = np.array(g["xPID"])[:100], np.array(g["uPID"])[:100]
        for T in (100, 90, 80):
            A.ss_add_trajectory(xs[:T], us[:T]); A.model_add_trajectory(xs[:T], us[:T])
        before = _stores(A)
        _pid(A, [0.8, 0.9], 30, False)
        msg = _refused(E_STATE, lambda: A.store_retain(ss=[0, 2], model=[1]))
        assert "session" in msg, msg
        A.rollout_end()
        _same_stores(_stores(A), before, "after LMPC_E_STATE")
        ms, mm = A.store_retain(ss=[0, 2], model=[1])
        assert ms.tolist() == [0, -1, 1] and mm.tolist() == [-1, 0, -1] and A.ss_num_laps() == 2 and A.model_num_laps() == 1


def _chain_inputs(g, B, step):
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    tb = 40 + 37 * np.arange(B) + 11 * step
    rng = np.random.default_rng(100 + step)
    return dict(x0=xP[tb] + rng.normal(size=(B, 6)) * np.array([.02, .01, .02, .01, 0.0, .02]), xLin=np.stack([xP[t + 1:t + N + 2] for t in tb]),
                uLin=np.stack([uP[t + 1:t + N + 1] for t in tb]), uOld=uP[tb].copy(), zt=xP[tb + N + 1].copy(), timeStep=(tb % 300).astype(np.int32))


def test_a_held_solve_runs_on_the_stores_of_before(built, g):
    """Steps 0, 1, 2 queued (step 2's solve is held), a retain that drops a lap no step reads, steps 3, 4, a sync: every output of every step equals the same chain
    on a context that is never pruned.  The retain launches the held solve first, then moves the stores."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=3, max_laps=8, max_lap_len=1024)
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    inps = [_chain_inputs(g, 3, s) for s in range(5)]
    outs, flushed = [], None
    for prune in (True, False):
        with _capi.Context(cfg) as ctx:
            for cut in (50, 50, 0, 50, 50):                           # lap 2 is slower: in neither selection, and not the latest
                T = xP.shape[0] - cut
                ctx.model_add_trajectory(xP[:T], uP[:T]); ctx.ss_add_trajectory(xP[:T], uP[:T])
            args, keep = [], []
            for inp in inps:
                a, k = ctx.step_dev_buffers(inp)
                for key, (shp, dt) in _capi.array_specs(3, ctx.N, ctx.S, ctx.cfg.numSS_it, _capi.STEP_OUT_KEYS).items():
                    if int(np.prod(shp)):
                        ctx.dev_upload(getattr(a, _capi._FIELD[key]), np.zeros(shp, dtype=dt))
                args.append(a); keep += k
            ctx.sync()
            for s in (0, 1, 2):
                ctx.step_batch_dev(3, args[s])
            if prune:
                c0 = ctx.debug_k1_merge()
                ms, mm = ctx.store_retain(ss=[0, 1, 3, 4], model=[0, 1, 3, 4])
                flushed = ctx.debug_k1_merge()[1] - c0[1]
                assert ms.tolist() == [0, 1, -1, 2, 3] and ctx.ss_num_laps() == 4
            for s in (3, 4):
                ctx.step_batch_dev(3, args[s])
            outs.append([ctx.step_dev_fetch(a, 3) for a in args])
            for q in keep:
                ctx.dev_free(q)
    assert flushed == 1                                                # (a solve was held when the retain came, and the retain launched it)
    assert all(((o["status"] & ~64) == 0).all() for o in outs[1]), [o["status"] for o in outs[1]]
    for s, (o, r) in enumerate(zip(*outs)):
        _same_out(o, r, ("queued step", s))


# ---- 7
def test_save_stores_after_a_retain(built, g, tmp_path):
    p = sc.problems(g, 8)
    ctx = _shared_context(g, range(6))
    try:
        ctx.store_retain(ss=[0, 2, 3, 4, 5], model=[0, 1, 2, 3])
        ctx.save_stores(str(tmp_path / "pruned"))
        again = _shared_context(g, [])
        try:
            assert again.ss_num_laps() == 0
            ms, mm = again.store_retain(ss=None, model=[])          # (restore_stores wants empty stores: a retain empties one)
            assert ms is None and mm.tolist() == [-1, -1, -1, -1] and again.model_num_laps() == 0
            again.restore_stores(str(tmp_path / "pruned"))
            _same_stores(_stores(again), _stores(ctx), "restored from the file written after the retain")
            _same_out(again.step_batch(**p), ctx.step_batch(**p), "step of the restored context")
        finally:
            again.close()
    finally:
        ctx.close()


# ---- 8
def _per_car_run(g, cfg, prune, vt, tracks=None, **kw):
    from racinglmpc_amd import _capi, rollout
    B = len(vt)
    ctx = _capi.Context(cfg)
    try:
        ro = rollout.BatchedRollouts(ctx, np.array(g["track"]), seed=5, device_noise=True, **({} if tracks is None else dict(tracks=tracks)))
        ro.noise_shard = (0, B, B)
        # two whole PID runs per car (equal rows: a tie): a row of four then holds both, and the third LMPC lap pushes the second one out -- the pruned stores do give laps back
        steps = 1000 if tracks is not None else 700
        slow, fast = ro.run_pid_laps(vt - 0.05, max_steps=steps, keep_invalid=True), ro.run_pid_laps(vt, max_steps=steps, keep_invalid=True)
        assert all(l[4] >= 0 and not (l[5] & ~_capi.ST_INEXACT) for l in slow + fast)
        loop = rollout.PerCarLMPC(ro, T_max=400, ext=40, prune=prune, **kw)
        loop.seed([[a, b] for a, b in zip(slow, fast)])
        gens = []
        for _ in range(3):
            out = loop.run()
            gens.append(dict(out=out, counts=(ctx.ss_num_laps(), ctx.model_num_laps()), ss_table=ro.ss_table.copy(), ss_last=ro.ss_last.copy(), lap_table=ro.lap_table.copy()))
        ss = [ctx.store_read_lap(1, l) + (ctx.ss_lap_time(l),) for l in range(ctx.ss_num_laps())]
        nm = ctx.model_num_laps()
        model = [(ctx.store_read_lap(0, ctx.model_lap_info(k)[1])[:2], ctx.debug_model_image(k)) for k in range(nm)]      # by insertion index
        return dict(gens=gens, lap_times=[list(t) for t in loop.lap_times], retired=dict(loop.retired), steps=list(loop.steps), ss=ss, model=model,
                    latest=[l[:3] for l in loop.latest])
    finally:
        ctx.close()


@pytest.mark.parametrize("case", ["device_commit", "host_adds", "park", "tracks"])
def test_per_car_lmpc_pruned_against_unpruned(built, g, case):
    """Three generations with prune=True against prune=False: lap times, retired cars, session steps and the returned tuples are identical; every lap the pruned
    context holds is bit-identical to the lap of the unpruned one that the tables name at the same place; the counts stay within B (numSS_it + 1) and B trToUse."""
    B = 4 if case == "tracks" else 6
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=8, max_lap_len=1024)
    kw = dict(device_commit=case in ("device_commit", "tracks"), park=case == "park")
    tracks = [np.array(tk.table(n)[0]) for n in tk.deal(B)] if case == "tracks" else None
    vt = np.array([0.75, 0.78, 0.8, 0.82, 0.85, 0.8])[:B]
    on, off = (_per_car_run(g, cfg, prune, vt, tracks, **kw) for prune in (True, False))
    print(case, "lap times", off["lap_times"], "retired", off["retired"], "counts pruned", [x["counts"] for x in on["gens"]], "unpruned", [x["counts"] for x in off["gens"]])
    assert on["lap_times"] == off["lap_times"] and on["retired"] == off["retired"] and on["steps"] == off["steps"]
    assert sum(len(t) for t in off["lap_times"]) >= B                                               # (the generations did add laps)
    for a, r in zip(on["latest"], off["latest"]):
        for j in range(3):
            _same(a[j], r[j], ("latest", j))
    for gen, (p, f) in enumerate(zip(on["gens"], off["gens"])):
        for b in range(B):
            a, r = p["out"][b], f["out"][b]
            assert (a is None) == (r is None), (gen, b)
            if a is not None:
                assert a[4] == r[4] and a[5] == r[5]
                for j in (0, 1, 3) + (() if kw["device_commit"] else (2,)):
                    _same(a[j], r[j], ("lap tuple", gen, b, j))
        ns, nm = p["counts"]
        assert ns <= B * (cfg.numSS_it + 1) and nm <= B * cfg.trToUse, (gen, ns, nm)
        assert f["counts"][0] >= ns and f["counts"][1] >= nm, (gen, f["counts"], p["counts"])
    assert sum(off["gens"][-1]["counts"]) > sum(on["gens"][-1]["counts"])                           # (laps were given back)
    # the tables of the last generation name the same laps under other indices: every lap the pruned context holds, against its counterpart
    p, f = on["gens"][-1], off["gens"][-1]
    seen_ss, seen_m = set(), set()
    for tab_p, tab_f in ((p["ss_table"], f["ss_table"]), (p["ss_last"][:, None], f["ss_last"][:, None])):
        for i, j in zip(tab_p.reshape(-1).tolist(), tab_f.reshape(-1).tolist()):
            assert (i < 0) == (j < 0)
            if i >= 0 and i not in seen_ss:
                seen_ss.add(i)
                for k in range(3):
                    _same(on["ss"][i][k], off["ss"][j][k], ("safe-set lap", i, j, "xuq"[k]))
                assert on["ss"][i][3] == off["ss"][j][3]
    for i, j in zip(p["lap_table"].reshape(-1).tolist(), f["lap_table"].reshape(-1).tolist()):
        if i not in seen_m:
            seen_m.add(i)
            (pa, pim), (fa, fim) = on["model"][i], off["model"][j]
            _same(pa[0], fa[0], ("regression lap", i, j, "x")); _same(pa[1], fa[1], ("regression lap", i, j, "u"))
            assert pim[2] == fim[2]
            _same(pim[0], fim[0], ("image words", i, j)); _same(pim[1], fim[1], ("image parameters", i, j))
    assert seen_ss == set(range(len(on["ss"]))) and seen_m == set(range(len(on["model"])))          # (and it holds no lap that nothing names)
