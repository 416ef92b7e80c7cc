"""-m gpu: laps of a rollout session committed to the lap stores on the device (lmpc_rollout_commit_laps, lmpc_rollout_extend_laps; rollout.PerCarLMPC(device_commit=True)).

The reference of every case is the host path on a second context: rollout_fetch of the same session's logs, then ss_add_trajectory / model_add_trajectory /
ss_extend_lap of those rows.  Everything is compared bit for bit (as int64 words, so that NaN rows and the sign of a zero count): the rows of both stores, Qfun,
LapTime, the regression store's sorted order, the prefilter image (lmpc_debug_model_image), and what a regression and a safe-set selection compute from them.
Both contexts' laps go through the same store-writing kernels (the second one's from staged host rows, one lap per launch), so every snapshot of the stores is
also compared, bit for bit, with tests/store_ref.py: the same edits restated on the host from the fetched rows.
N = 12; what needs no device is in tests/test_device_commit_host.py."""
import numpy as np
import pytest

from tests import common, store_ref

pytestmark = pytest.mark.gpu

N = 12
E_ARG, E_STATE = "error -1:", "error -4:"


@pytest.fixture(scope="module")
def g():
    return common.load_lmpc_golden()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), what


def _stores(ctx):
    """Everything the stores hold, as the public entry points show it."""
    ss = [ctx.store_read_lap(1, l) + (ctx.ss_lap_time(l), ctx.ss_lap_rows(l)) for l in range(ctx.ss_num_laps())]
    nm = ctx.model_num_laps()
    model = [ctx.store_read_lap(0, p)[:2] for p in range(nm)]
    info = [ctx.model_lap_info(k) for k in range(nm)]
    image = [ctx.debug_model_image(k) for k in range(nm)]
    return dict(ss=ss, model=model, info=info, image=image)


def _same_stores(a, b, what):
    assert len(a["ss"]) == len(b["ss"]) and len(a["model"]) == len(b["model"]), what
    for l, (p, q) in enumerate(zip(a["ss"], b["ss"])):
        for k in range(3):
            _same(p[k], q[k], (what, "safe set", l, "xuq"[k]))
        assert p[3:] == q[3:], (what, "safe set", l, p[3:], q[3:])
    for l, (p, q) in enumerate(zip(a["model"], b["model"])):
        _same(p[0], q[0], (what, "regression store", l, "x")); _same(p[1], q[1], (what, "regression store", l, "u"))
    assert a["info"] == b["info"], (what, a["info"], b["info"])
    for l, (p, q) in enumerate(zip(a["image"], b["image"])):
        assert p[2] == q[2], (what, "image chunks", l, p[2], q[2])
        _same(p[0], q[0], (what, "image words", l)); _same(p[1], q[1], (what, "image parameters", l))


def _pid(ctx, vt, T_max, stop_at_line, seed=11, x0=None):
    """One PID session on host-drawn noise (the same draws for the same seed); left active.  Returns t."""
    B = len(vt)
    rng = np.random.default_rng(seed)
    nu, nz = rng.standard_normal((T_max, B, 2)), rng.standard_normal((T_max, B, 3))
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1)) if x0 is None else x0
    t, _ = ctx.rollout_pid(x0, x0, np.asarray(vt, float), nu, nz, stop_at_line=stop_at_line)
    return t


def _refused(code, call):
    from racinglmpc_amd import _capi
    with pytest.raises(_capi.LmpcError) as e:
        call()
    assert code in str(e.value), str(e.value)
    return str(e.value)


def test_commit_equals_the_host_path_at_every_boundary(built, g):
    """Six entries into both stores of a context that has to grow in both directions inside the call: image rows (rows - 1) just under, on and just over the 1024-row
    chunk edge, the shortest lap the regression store takes, a tie in the sorted insert that is also a duplicated car; rows past the first crossing take computeCost's
    cost = 0 branch.  Against the host path on a second context: stores, LapTime, sorted order, prefilter image, one regression of 64 points, one selection."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=8, max_laps=4, max_lap_len=256)
    cars, rows = [0, 1, 2, 3, 4, 4], [1024, 1025, 1026, 2, 300, 300]
    vt = [0.7, 0.75, 0.8, 0.85, 0.9]
    with _capi.Context(cfg) as A, _capi.Context(cfg) as Bc:
        t = _pid(A, vt, 1100, False)
        assert t == 1100
        first = A.rollout_commit_laps(cars, rows)
        X, U, _, done, st, _, _ = A.rollout_fetch(0, t)
        A.rollout_end()
        assert first == (0, 0) and A.ss_num_laps() == 6 and A.model_num_laps() == 6               # no entry skipped
        assert (done[:3] >= 0).all() and (done[:3] < 1024).all(), done                             # (rows past the first crossing are part of the long laps)
        ref = store_ref.RefStores.like(cfg)
        for c, T in zip(cars, rows):
            x, u = X[:T, c].copy(), U[:T, c].copy()
            for dst in (Bc, ref):
                dst.ss_add_trajectory(x, u); dst.model_add_trajectory(x, u)
        sa, sb = _stores(A), _stores(Bc)
        _same_stores(sa, ref.snapshot(), "commit against the restatement"); _same_stores(sb, ref.snapshot(), "host laps against the restatement")
        assert [s[3] for s in sa["ss"]] == rows and [i[0] for i in sa["info"]] == rows
        assert [i[1] for i in sa["info"]] == [3, 4, 5, 0, 1, 2]                                    # ascending rows, the two 300s in listed order
        assert [im[2] for im in sa["image"]] == [1, 1, 2, 1, 1, 1]                                 # 1023 and 1024 image rows: one chunk; 1025: two
        assert sa["image"][3][0].shape == (3, 1) and sa["image"][2][0].shape == (3, 1025)
        _same_stores(sa, sb, "commit")
        for l, T in enumerate(rows):                                                               # (and against the fetched rows themselves)
            _same(sa["ss"][l][0], X[:T, cars[l]], ("rows", l)); _same(sa["ss"][l][1], U[:T, cars[l]], ("inputs", l))
        q = sa["ss"][0][2]
        # (row doneAt is the first with s > trackLength: cost 0 there and behind it, counting up towards row 0 in front of it)
        assert not q[done[0]:].any() and q[done[0] - 1] == 1.0 and q[0] == done[0], (done[0], q[:3])
        xq, uq = X[0:1024:16, 0].copy(), U[0:1024:16, 0].copy()
        assert xq.shape[0] == 64
        for k, (p, r) in enumerate(zip(A.regress_points(xq, uq), Bc.regress_points(xq, uq))):
            _same(p, r, ("regress_points", "ABCs"[k]))
        for c in (A, Bc):
            c.ss_set_selected([0, 1, 2, 4])
        tb = np.array([40, 120, 200, 260])
        sel = [c.select_batch(X[tb, 0].copy(), X[tb + N + 1, 0].copy()) for c in (A, Bc)]
        assert sel[0]["ssSel"].any()
        for k in _capi.SELECT_OUT_KEYS:
            _same(sel[0][k], sel[1][k], ("select_batch", k))


def test_rows_none_refusals_and_nothing_half_done(built, g):
    """rows=None commits up to each car's crossing step and refuses a car that has not crossed (LMPC_E_STATE, the car named); every refusal leaves both stores as
    they were."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=4, max_lap_len=512)
    with _capi.Context(cfg) as A:
        xs, us = np.array(g["xPID"])[:100], np.array(g["uPID"])[:100]
        ref = store_ref.RefStores.like(cfg)
        for dst in (A, ref):
            dst.ss_add_trajectory(xs, us); dst.model_add_trajectory(xs, us)
        before = _stores(A)
        _same_stores(before, ref.snapshot(), "one lap from the host against the restatement")
        t = _pid(A, [0.9, 0.8, 0.45], 400, True)
        X, U, _, done, st, _, _ = A.rollout_fetch(0, t)
        assert t == 400 and done[0] >= 0 and done[1] >= 0 and done[2] < 0 and done[0] != done[1], done
        B = 3
        msg = _refused(E_STATE, lambda: A.rollout_commit_laps([0, 1, 2]))
        assert "car 2" in msg, msg
        _same_stores(_stores(A), before, "after LMPC_E_STATE")
        for bad in (lambda: A.rollout_commit_laps([0, B], [10, 10]), lambda: A.rollout_commit_laps([0, 1], [10, 0]), lambda: A.rollout_commit_laps([0, 2], [10, t + 1]),
                    lambda: A.rollout_commit_laps([0, 1], [10, int(done[1]) + 1]),               # (stop_at_line: a car is logged up to its crossing step only)
                    lambda: A.rollout_commit_laps([0, 1], [10, 1]),                              # (the regression store takes no one-row lap)
                    lambda: A.rollout_commit_laps([0, 1], [10, 10], ss=False, model=False)):
            _refused(E_ARG, bad)
            assert A.ss_num_laps() == 1 and A.model_num_laps() == 1
            _same_stores(_stores(A), before, "after LMPC_E_ARG")
        assert A.rollout_commit_laps([0, 1]) == (1, 1)
        A.rollout_end()
        assert A.ss_num_laps() == 3 and A.model_num_laps() == 3
        for k, b in enumerate((0, 1)):
            x, u, q = A.store_read_lap(1, 1 + k)
            _same(x, X[:done[b], b], ("lap of car", b)); _same(u, U[:done[b], b], ("inputs of car", b))
            _same(q, np.arange(done[b] - 1, -1, -1.0), ("Qfun of car", b))
            assert A.ss_lap_time(1 + k) == done[b] and A.model_lap_info(1 + k)[0] == done[b]
        x0, u0, q0 = A.store_read_lap(1, 0)
        _same(x0, before["ss"][0][0], "the lap stored before")
        for b in (0, 1):
            ref.ss_add_trajectory(X[:done[b], b], U[:done[b], b]); ref.model_add_trajectory(X[:done[b], b], U[:done[b], b])
        _same_stores(_stores(A), ref.snapshot(), "rows=None against the restatement")


def _seeded(ctx, g):
    """Three laps; the last Qfun value of lap 2 is 1/3 (ss_replace_lap): counting down from it is not the closed form."""
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    for T in (100, 110, 120):
        ctx.ss_add_trajectory(xP[:T], uP[:T])
    ctx.ss_replace_lap(2, xP[:120], uP[:120], np.arange(119, -1, -1.0) + 1.0 / 3.0)


def test_extension_equals_the_host_path(built, g):
    """rollout_extend_laps against ss_extend_lap of the fetched rows, with a store growth inside the call; refusals change nothing."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=4, max_lap_len=128)
    cars, laps, n = [0, 1, 2], [2, 0, 1], 40
    vt = [0.7, 0.8, 0.9]
    with _capi.Context(cfg) as A, _capi.Context(cfg) as Bc:
        ref = store_ref.RefStores.like(cfg)
        for c in (A, Bc, ref):
            _seeded(c, g)
        before = _stores(A)
        _same_stores(before, ref.snapshot(), "seed laps against the restatement")
        t = _pid(A, vt, 60, False)
        _refused(E_ARG, lambda: A.rollout_extend_laps([0, 1, 2], [2, 0, 2], n))                    # the same lap twice
        _refused(E_ARG, lambda: A.rollout_extend_laps(cars, laps, t + 1))
        _refused(E_ARG, lambda: A.rollout_extend_laps(cars, [2, 0, 3], n))                         # no such lap
        _refused(E_ARG, lambda: A.rollout_extend_laps([0, 1, 3], laps, n))                         # no such car
        _same_stores(_stores(A), before, "after LMPC_E_ARG")
        ext = A.rollout_extend_laps(cars, laps, n)
        A.rollout_end()
        assert ext.dtype == bool and ext.tolist() == [True, True, True]
        assert _pid(Bc, vt, 60, False) == t
        X, U = Bc.rollout_fetch(0, t)[:2]
        Bc.rollout_end()
        for c, l in zip(cars, laps):
            Bc.ss_extend_lap(l, X[:n, c], U[:n, c]); ref.ss_extend_lap(l, X[:n, c], U[:n, c])
        assert [A.ss_lap_rows(l) for l in range(3)] == [140, 150, 160] == [Bc.ss_lap_rows(l) for l in range(3)]
        _same_stores(_stores(A), _stores(Bc), "extension")
        _same_stores(_stores(A), ref.snapshot(), "extension against the restatement")
        q = A.store_read_lap(1, 2)[2]
        want = 1.0 / 3.0
        for i in range(n):
            want -= 1.0
            assert q[120 + i] == want, i
        assert any(q[120 + i] != 1.0 / 3.0 - (i + 1) for i in range(n))                            # (the closed form is another number)
        for c in (A, Bc, ref):                                                                     # one more row on the last lap: it continues from the Qfun value the call left on the host side
            c.ss_add_point(X[0, 0], U[0, 0])
        _same_stores(_stores(A), _stores(Bc), "addPoint after the extension")
        _same_stores(_stores(A), ref.snapshot(), "addPoint after the extension against the restatement")


def test_extension_skips_a_car_with_non_finite_rows(built, g):
    """Car 1 starts with vx = NaN: its entry comes back not extended and its lap keeps its rows, the other two are extended as the host path extends them."""
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=4, max_lap_len=128)
    cars, laps, n = [0, 1, 2], [2, 0, 1], 40
    vt = [0.7, 0.8, 0.9]
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (3, 1)); x0[1, 0] = np.nan
    with _capi.Context(cfg) as A, _capi.Context(cfg) as Bc:
        ref = store_ref.RefStores.like(cfg)
        for c in (A, Bc, ref):
            _seeded(c, g)
        t = _pid(A, vt, 60, False, x0=x0)
        ext = A.rollout_extend_laps(cars, laps, n)
        X, U = A.rollout_fetch(0, t)[:2]
        A.rollout_end()
        assert not np.isfinite(X[:n, 1]).all() and np.isfinite(X[:n, [0, 2]]).all() and np.isfinite(U[:n, [0, 2]]).all()
        assert ext.tolist() == [True, False, True]
        for c, l in ((0, 2), (2, 1)):
            Bc.ss_extend_lap(l, X[:n, c], U[:n, c]); ref.ss_extend_lap(l, X[:n, c], U[:n, c])
        assert [A.ss_lap_rows(l) for l in range(3)] == [100, 150, 160]
        _same_stores(_stores(A), _stores(Bc), "extension with a skipped car")
        _same_stores(_stores(A), ref.snapshot(), "extension with a skipped car against the restatement")


def test_per_car_lmpc_with_device_commit_equals_the_host_loop(built, g):
    """PerCarLMPC, 3 cars, 2 generations (the first extends nothing: the seeds are whole PID runs; the second extends every car's first LMPC lap), once with the laps
    fetched and added by the host and once committed on the device: same lap times and tables after each generation, same stores at the end, and the device run
    returns the first N + 2 rows of the host run's laps."""
    from racinglmpc_amd import _capi, rollout
    track = np.array(g["track"])
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=16, max_lap_len=1024)
    SEED, T_MAX, EXT = 5, 400, 40
    vt = np.array([0.75, 0.8, 0.85])
    runs = []
    ctxs = [_capi.Context(cfg), _capi.Context(cfg)]
    ref = store_ref.RefStores.like(cfg)
    try:
        for name in ("ss_add_trajectory", "model_add_trajectory", "ss_extend_lap"):                # what the host loop hands to its context goes to the restatement as well
            def both(*args, _real=getattr(ctxs[0], name), _ref=getattr(ref, name)):
                _ref(*args)
                return _real(*args)
            setattr(ctxs[0], name, both)
        for ctx, dev in zip(ctxs, (False, True)):
            ro = rollout.BatchedRollouts(ctx, track, seed=SEED, device_noise=True)
            ro.noise_shard = (0, 3, 3)
            seeds = ro.run_pid_laps(vt, max_steps=700, keep_invalid=True)
            assert all(l[4] >= 0 and l[5] == 0 for l in seeds)
            loop = rollout.PerCarLMPC(ro, T_max=T_MAX, ext=EXT, device_commit=dev)
            loop.seed(seeds)
            gens = []
            for _ in range(2):
                out = loop.run()
                assert not loop.retired and all(o is not None for o in out), (dev, loop.retired, loop.last_status, loop.last_done)
                gens.append(dict(out=out, lap_times=[list(t) for t in loop.lap_times], ss_table=ro.ss_table.copy(), ss_last=ro.ss_last.copy(), lap_table=ro.lap_table.copy()))
            runs.append(gens)
        for gen, (h, d) in enumerate(zip(*runs)):
            assert h["lap_times"] == d["lap_times"], (gen, h["lap_times"], d["lap_times"])
            for k in ("ss_table", "ss_last", "lap_table"):
                assert np.array_equal(h[k], d[k]), (gen, k, h[k], d[k])
            for b in range(3):
                ho, do = h["out"][b], d["out"][b]
                assert do[0].shape == (N + 2, 6) and do[1].shape == (N + 2, 2) and do[2] is None and do[4] == ho[4] and do[5] == ho[5]
                _same(do[0], ho[0][:N + 2], (gen, b, "head x")); _same(do[1], ho[1][:N + 2], (gen, b, "head u")); _same(do[3], ho[3], (gen, b, "final state"))
        sh, sd = _stores(ctxs[0]), _stores(ctxs[1])
        assert len(sh["ss"]) == 9 and any(s[4] > s[3] for s in sh["ss"])                            # 3 seeds + 2 x 3 laps; generation 2 has extended laps
        _same_stores(sd, sh, "after generation 2")
        _same_stores(sh, ref.snapshot(), "after generation 2 against the restatement")
    finally:
        for c in ctxs:
            c.close()
