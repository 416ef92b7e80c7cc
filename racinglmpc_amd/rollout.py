"""Batched closed-loop LMPC rollouts: B independent cars share one safe set and are advanced in lock-step ON THE DEVICE
(lmpc_rollout_*: regression + solve + plant kernel + bookkeeping per simulated step, no host round trip).  Caller side of
the hot path (reference SysModel.Simulator.sim, SysModel.py:22-54; plant: Simulator.dynModel, SysModel.py:56-147).

Rank-local: each rank owns a contiguous shard of the rollouts (parallel.shard) and its own device context; after a lap the
ranks exchange their fastest VALID laps once (lmpc_rollout_exchange: device-packed records, one RCCL all-gather) and apply
identical inserts.  A lap is valid when the car crossed the finish line and no status bit other than LMPC_ST_INEXACT was
raised up to the crossing step; anything else never reaches a lap store -- neither as a new lap nor as the rows that extend a
stored lap past the finish line (the batched LMPC.addPoint): those are checked for status bits and finiteness first.

The three stages in front of the LMPC laps (main.py:61-95) run the same way: BatchedRollouts.run_pid_laps (whole PID laps in one launch), run_mpc_laps (LTI path-following
MPC / LTV-MPC sessions on a numSS_it == 0 context) and bootstrap(), which chains them -- PID laps -> batched Utilities.Regression -> LTI-MPC laps -> LTV-MPC laps.
"""
import numpy as np

from . import _capi, parallel


def _lap_metrics_rows(ctx, B, cars):
    """(B, METRICS_NCOL) of the active session: one Context.rollout_lap_metrics call over `cars`, up to their crossing steps; NaN rows for the cars not listed."""
    cars = np.asarray(cars, np.int64).reshape(-1)
    out = np.full((B, _capi.METRICS_NCOL), np.nan)
    if cars.size:
        out[cars] = ctx.rollout_lap_metrics(cars)
    return out


class BatchedRollouts:
    """B closed-loop LMPC laps against a shared safe set, or (ss_table) each car against its own (one GPU context, one rank)."""

    def __init__(self, ctx, track, seed=0, global_noise=False, prefetch=True, plant_params=None, device_noise=False, lap_table=None, ss_table=None, ss_last=None, tuning=None, tracks=None, trace=None, trace_what=None, park=None, metrics=False):
        """metrics: run_pid_laps, run_mpc_laps and run_lap_device leave the lap metrics of their session in `last_metrics` -- (B, _capi.METRICS_NCOL), columns
        _capi.METRIC_FIELDS, one Context.rollout_lap_metrics call over the cars that crossed the line, taken before the session ends; NaN rows for the others.  The
        returned tuples are what they are without it.  False: no call is made and last_metrics stays None.
        trace / trace_what: the cars of THIS object whose controller output every LMPC / MPC session records step by step, and the planes (_capi.TRACE_* bits; None:
        every plane the context can record) -- the reference's xStoredPredTraj / uStoredPredTraj / SSStoredPredTraj (PredictiveControllers.py:364-379) with the
        Q-values, the solver's words and the inertial positions beside them (Context.rollout_set_trace); handed to the context before every begin and run_mpc_laps,
        beside tuning.  run_lap_device, run_mpc_laps and PerCarLMPC.run then leave the session's trace in `last_trace`: the planes (steps, listed cars, ...) of
        Context.rollout_fetch_trace plus "cars" and "doneAt" (the crossing step of each listed car, -1: none) -- TraceView turns it into one car's history.  None:
        the context's trace is left as it is and last_trace stays None.
        tracks: the tracks of the cars of THIS object (this rank's shard) -- one PointAndTangent table for all cars or a sequence of them, one per car (tables, or
        (table, trackLength) pairs, or (n, 98) rows as _capi.track_rows builds them); handed to the context (Context.track_set) before every begin, run_pid_laps and
        run_mpc_laps, beside plant_params.  `TL` is then an array, one length per row (track_lengths(B): one per car).  None: the context's rows are left as they
        are and `TL` is the length of `track`, the table of the context's configuration.
        tuning: controller tuning of the cars of THIS object (this rank's shard), rows of _capi.TUNING_FIELDS as _capi.tuning_rows builds them -- one row for all cars
        or one per car (Context.tuning_set); handed to the context before every begin and run_mpc_laps, beside lap_table / ss_table.  The context's rows are live in a
        session, as the safe-set table is.  None: the context's rows are left as they are (the config's weights unless the caller set others).
        lap_table: per-car regression laps of the cars of THIS object, rows of trToUse insertion indices into the context's regression store -- one row for all cars
        or one per car (Context.model_set_lap_table); handed to the context before every begin and every LTV run_mpc_laps, as plant_params is.  None: the context's
        table is left as it is (no table unless the caller set one: every car regresses on the first trToUse laps of the store's sorted order).  On an LMPC context
        the safe set does not follow this table: it has its own, ss_table.
        ss_table / ss_last: per-car safe sets of the cars of THIS object, rows of numSS_it safe-set lap indices and each car's latest lap -- one row for all cars or one
        per car (Context.ss_set_lap_table); handed to the context before every begin, as lap_table and plant_params are.  The context's table is live in a session:
        a caller that changes it between two rollout_run calls reaches the next step.  None: the context's table is left as it is (the shared selection unless the
        caller set one).
        plant_params: vehicle constants of the cars of THIS object (this rank's shard), rows of _capi.PLANT_PARAM_NAMES as _capi.plant_params builds them -- one row
        for all cars or one per car; handed to the context (Context.plant_set_params) before every begin, run_pid_laps and run_mpc_laps.  None: the context's
        parameters are left as they are (the reference's vehicle unless the caller set others).
        global_noise: the plant noise of a lap is drawn for ALL rollouts of the job (same seed on every rank) and this rank keeps the columns
        of its shard (`noise_shard` = (lo, hi, total), set by LmpcGeneration) -- a rollout then sees the same draws however the job is split over
        ranks.  Default: every rank draws for its own shard only (seed per rank).
        device_noise: the disturbance is generated on the device by the counter-based generator of csrc/lmpc_noise.hip.h (Context.rollout_set_noise): the draw of
        (seed, session, step, GLOBAL car index, component) is a pure function of those numbers, so nothing is drawn or uploaded by the host and a car sees the same
        disturbance however the job is split over ranks (`noise_shard[0]` is the first global index of this rank's cars; 0 without an LmpcGeneration) -- what global_noise
        buys with a draw for the whole job on every rank.  `seed` is then an integer in [0, 2**64), the same on every rank; `rng` is never touched, no worker thread is
        started, prefetch_noise and close have nothing to do; `lap` counts the sessions begun (begin, run_pid_laps, each run_mpc_laps) and is the generator's session
        counter.  The stream is the device generator's own: it does not reproduce the draws of `rng`."""
        self.ctx, self.track = ctx, np.asarray(track, float)
        self.TL = float(self.track[-1, 3] + self.track[-1, 4])
        self.tracks = None
        if tracks is not None:
            self.set_tracks(tracks)
        self.rng = np.random.default_rng(seed)
        self.global_noise, self.noise_shard = bool(global_noise), None
        self.last_status = None
        self.last_done = None
        self.plant_params = None if plant_params is None else _capi.check_plant_params(plant_params)
        self.lap_table = None if lap_table is None else _capi.check_lap_table(lap_table, ctx.cfg.trToUse)
        self.ss_table, self.ss_last = (None, None) if ss_table is None else _capi.check_ss_table(ss_table, ctx.cfg.numSS_it, ss_last)
        if ss_table is None and ss_last is not None:
            raise ValueError("ss_last: needs ss_table")
        self.tuning = None if tuning is None else _capi.check_tuning(tuning, ctx.cfg.numSS_it)
        self.trace = None if trace is None else _capi.check_trace(trace, trace_what, ctx.cfg.numSS_it)
        self.last_trace = None
        # park: the parking of every LMPC / MPC session of this object (Context.rollout_set_parking) -- True (PARK_FINISHED: a car leaves the launches once it has
        # crossed the line, and a session that stops at the line ends when no car is live), a mode of _capi.PARK_* bits, or (mode, cars) with the cars parked from
        # step 0.  Handed to the context before every begin and run_mpc_laps, where the trace is; run_lap_device, run_mpc_laps and PerCarLMPC.run then leave the
        # session's parking steps in `last_parked_at` (Context.rollout_parked_at: -1 for a car stepped to the end; a parked car's log rows stand still from its
        # step on).  None: the context's parking is left as it is and last_parked_at stays None.
        self.park = self._check_park(park)
        self.last_parked_at = None
        self.metrics = bool(metrics)
        self.last_metrics = None
        self.device_noise = bool(device_noise)
        if self.device_noise:
            import operator
            self.seed = operator.index(seed)
            if not 0 <= self.seed < 2 ** 64:
                raise ValueError("device_noise: seed must be an integer in [0, 2**64), got %r" % (seed,))
        self.lap = 0                   # device_noise: sessions begun so far -- the `lap` word of the generator's counter for the NEXT session
        self.prefetch = bool(prefetch) # False: every array is drawn when it is asked for, no worker thread (same draws, same order: tests compare the two)
        self._pre = None               # (shape key, generator state before the draw, future): the NEXT lap's plant noise, drawn by a worker thread while this lap runs

    def _draw_noise(self, max_steps, B, prefetch_only=False, width=3):
        """Plant noise of one lap, (max_steps, B, 3) N(0, 1) draws; width = 2: the control-law noise of a PID lap, a draw of its own.
          A generation loop asks for the same shape lap after lap, and 1.2 M draws are ~15 ms of one
        host core -- a tenth of a 1024-rollout lap on the GPU: the next lap's array is drawn by a worker thread while the device runs this one (NumPy releases
        the GIL inside the fill).  The generator is consumed in exactly the order it would be without the prefetch: a prefetched array of another shape is
        discarded together with its draws (the generator state from before the draw is restored)."""
        if getattr(self, "device_noise", False):   # (the session's buffer is filled on the device: _device_noise_session)
            return None
        if self.global_noise and self.noise_shard is not None:
            lo, hi, total = self.noise_shard
            assert hi - lo == B, (lo, hi, B)
            key = (max_steps, total, lo, hi, width)
            draw = lambda: np.ascontiguousarray(self.rng.standard_normal((max_steps, total, width))[:, lo:hi])
        else:
            key = (max_steps, B, width)
            draw = lambda: self.rng.standard_normal((max_steps, B, width))
        if not getattr(self, "prefetch", True):    # (objects built without __init__ -- tests/test_host_checks.py -- prefetch)
            return None if prefetch_only else draw()
        if prefetch_only:                          # (prefetch_noise: start the draw of the FIRST lap; the generator is consumed in the same order)
            if self._pre is None:
                from concurrent.futures import ThreadPoolExecutor
                if not hasattr(self, "_pool"):
                    self._pool = ThreadPoolExecutor(max_workers=1)
                self._pre = (key, self.rng.bit_generator.state, self._pool.submit(draw))
            return None
        noise = None
        if self._pre is not None:
            pkey, state, fut = self._pre
            self._pre = None
            got = fut.result()
            if pkey == key:
                noise = got
            else:
                self.rng.bit_generator.state = state
        if noise is None:
            noise = draw()
        from concurrent.futures import ThreadPoolExecutor
        if not hasattr(self, "_pool"):
            self._pool = ThreadPoolExecutor(max_workers=1)
        self._pre = (key, self.rng.bit_generator.state, self._pool.submit(draw))
        return noise

    def close(self):
        """End of a generation loop: wait for the prefetched draw nobody will use, give its draws back (the generator state from before that draw is restored, so
        `rng` is where a run without prefetching leaves it) and shut the worker thread down.  Between begin() calls `rng` belongs to the prefetcher: the worker
        thread is drawing from it -- do not touch it from the caller's thread before close()."""
        if self._pre is not None:
            _, state, fut = self._pre
            self._pre = None
            fut.result()
            self.rng.bit_generator.state = state
        pool = self.__dict__.pop("_pool", None)
        if pool is not None:
            pool.shutdown(wait=True)

    def prefetch_noise(self, max_steps, B, wait=False):
        """Draw the plant noise of the first lap ahead of time (worker thread; same draws, same order as without the call): the synthetic disturbance is input
        data of a closed-loop run, and 1.2 M normal draws are 15-20 ms of host time that would otherwise open the first lap."""
        self._draw_noise(max_steps, B, prefetch_only=True)
        if wait and self._pre is not None:
            self._pre[2].result()

    def _device_noise_session(self, B):
        """device_noise: hand the context the source of the session about to begin -- (seed, this object's session counter, first global car index) -- and count the
        session.  Returns True when the session is to be begun with noise=None; False (host draws) leaves the context alone."""
        if not getattr(self, "device_noise", False):  # (objects built without __init__ -- tests/test_host_checks.py -- draw on the host)
            return False
        car0 = 0
        if self.noise_shard is not None:
            lo, hi, total = self.noise_shard
            assert hi - lo == B, (lo, hi, B)
            car0 = int(lo)
        self.ctx.rollout_set_noise(True, self.seed, self.lap, car0)
        self.lap += 1
        return True

    def set_tracks(self, tracks):
        """tracks as __init__ takes them; TL becomes the array of their lengths."""
        arr = tracks if isinstance(tracks, np.ndarray) else None
        if arr is not None and arr.ndim == 2 and arr.shape[1] == _capi.TRACK_NPAR:
            rows = _capi.check_tracks(arr)
        elif arr is not None and arr.ndim == 2:                       # one table for every car
            rows = _capi.track_rows([arr])
        else:
            rows = _capi.track_rows(list(tracks))
        if rows is None:
            raise ValueError("tracks: at least one track expected")
        self.tracks = rows
        self.TL = rows[:, 1].copy()

    def track_lengths(self, B):
        """TrackLength of each of B cars, (B,): the cars' own rows, or the one length every car shares."""
        TL = np.atleast_1d(np.asarray(self.TL, float))
        if TL.shape[0] not in (1, B):
            raise ValueError("tracks: one row or one per car (%d) expected, got %d" % (B, TL.shape[0]))
        return np.broadcast_to(TL, (B,)).copy()

    def track_row_of(self, b):
        """The track_row argument of the host-side lap writers for car b: b with one row per car in force, else None (the config's track, or the one row)."""
        rows = getattr(self, "tracks", None)
        return int(b) if rows is not None and rows.shape[0] > 1 else None

    # The per-car row sets this object hands to the context in front of a session: attribute -> (setter of the context, attributes that travel with the rows).
    # Tracks are refused by the context while a session is active; the vehicle rows and the lap table are snapshotted when one begins; the others are live.
    _ROW_SETS = {"tracks": ("track_set", ()), "plant_params": ("plant_set_params", ()), "lap_table": ("model_set_lap_table", ()),
                 "ss_table": ("ss_set_lap_table", ("ss_last",)), "tuning": ("tuning_set", ())}

    def _apply_rows(self, B, which):
        """The named row sets (keys of _ROW_SETS, in the order given) of this object's B cars go to the context; a set this object does not hold is left alone."""
        for name in which:
            setter, extra = self._ROW_SETS[name]
            rows = getattr(self, name, None)           # (objects built without __init__ -- tests/test_host_checks.py -- have none)
            if rows is None:
                continue
            if rows.shape[0] not in (1, B):
                raise ValueError("%s: one row or one per car (%d) expected, got %d" % (name, B, rows.shape[0]))
            getattr(self.ctx, setter)(rows, *[getattr(self, e, None) for e in extra])

    def _apply_trace(self, B):
        """The traced cars of this object go to the context in front of a session that solves."""
        tr = getattr(self, "trace", None)              # (objects built without __init__ -- tests/test_host_checks.py -- have none)
        if tr is None:
            return
        cars, what = tr
        if cars.size and int(cars.max()) >= B:
            raise ValueError("trace: car %d listed, the session has %d cars" % (int(cars.max()), B))
        self.ctx.rollout_set_trace(cars, what)

    @staticmethod
    def _check_park(park):
        if park is None:
            return None
        if isinstance(park, (tuple, list)):
            if len(park) != 2:
                raise ValueError("park: True, a mode, or (mode, cars) expected")
            return _capi.check_parking(park[0], park[1])
        return _capi.check_parking(park, None)

    def _apply_park(self, B):
        """The parking of this object goes to the context in front of a session that solves."""
        pk = getattr(self, "park", None)               # (objects built without __init__ have none)
        if pk is None:
            return
        mode, cars = pk
        if cars.size and int(cars.max()) >= B:
            raise ValueError("park: car %d listed, the session has %d cars" % (int(cars.max()), B))
        self.ctx.rollout_set_parking(mode, cars)

    def _fetch_parked(self):
        """last_parked_at of the active session, to be called before rollout_end."""
        self.last_parked_at = None if getattr(self, "park", None) is None else self.ctx.rollout_parked_at()[0]
        return self.last_parked_at

    def _fetch_metrics(self, done):
        """last_metrics of the active session, to be called before rollout_end: the cars that crossed the line, up to their crossing steps."""
        done = np.asarray(done)
        self.last_metrics = _lap_metrics_rows(self.ctx, done.shape[0], np.flatnonzero(done >= 0)) if getattr(self, "metrics", False) else None
        return self.last_metrics

    def _fetch_trace(self, t, done):
        """last_trace of the active session, to be called before rollout_end: the planes of steps [0, t) and the listed cars' crossing steps."""
        tr = getattr(self, "trace", None)
        if tr is None or tr[0].size == 0:
            self.last_trace = None
            return None
        out = self.ctx.rollout_fetch_trace(0, t)
        out["cars"] = tr[0].copy(); out["doneAt"] = np.asarray(done)[tr[0]].copy()
        self.last_trace = out
        return out

    @staticmethod
    def _per_rollout(a, B):
        a = np.asarray(a, float)
        return np.tile(a[None], (B, 1, 1)) if a.ndim == 2 else a

    def begin(self, x0, xLin0, uLin0, xglob0=None, max_steps=400):
        B = x0.shape[0]
        xl = self._per_rollout(xLin0, B); ul = self._per_rollout(uLin0, B)
        noise = self._draw_noise(max_steps, B)
        self._apply_rows(B, ("tracks", "plant_params", "lap_table", "ss_table", "tuning"))
        self._apply_trace(B)
        self._apply_park(B)
        if self._device_noise_session(B):
            self.ctx.rollout_begin(x0, x0 if xglob0 is None else xglob0, xl, ul, None, T_max=max_steps)
        else:
            self.ctx.rollout_begin(x0, x0 if xglob0 is None else xglob0, xl, ul, noise)

    def run_lap_device(self, x0, xLin0, uLin0, xglob0=None, max_steps=400, ext=0, on_ext=None, keep_invalid=False):
        """The whole lap stays on the GPU: four kernel launches per simulated step.  If ext > 0 the lap pauses after `ext` steps
        and on_ext(X, U) is called with the states/inputs logged so far (n <= ext rows, n x B x .) -- the hook that plays
        LMPC.addPoint for the stored laps.  Returns the VALID laps [(x, u, x_glob, final12, done_at, status)] (final12 = state +
        global state right after the finish line); with keep_invalid the unfinished / flagged ones are returned too, their
        done_at / status telling them apart."""
        B = x0.shape[0]
        self.begin(x0, xLin0, uLin0, xglob0, max_steps)
        if ext > 0:
            t, nd = self.ctx.rollout_run(ext)
            X, U, G, done, st, fx, fg = self.ctx.rollout_fetch(0, t)
            if on_ext is not None:
                on_ext(X, U)
        t, nd = self.ctx.rollout_run(max_steps)
        X, U, G, done, st, fx, fg = self.ctx.rollout_fetch(0, t)
        self._fetch_trace(t, done)
        self._fetch_parked()
        self._fetch_metrics(done)
        self.ctx.rollout_end()
        self.last_status, self.last_done = st, done
        laps = []
        for b in range(B):
            valid = done[b] >= 0 and (st[b] & ~_capi.ST_INEXACT) == 0
            if not (valid or keep_invalid):
                continue
            T = int(done[b]) if done[b] >= 0 else X.shape[0]
            laps.append((X[:T, b].copy(), U[:T, b].copy(), G[:T, b].copy(), np.concatenate([fx[b], fg[b]]), int(done[b]), int(st[b])))
        return laps


    def _collect(self, B, X, U, G, done, st, fx, fg, whole, keep_invalid):
        """Lap tuples (x, u, x_glob, final12, done_at, status) of a finished session: the rows up to the crossing step, or (whole: a multiLap run, main.py:57) every logged row."""
        self.last_status, self.last_done = st, done
        laps = []
        for b in range(B):
            valid = done[b] >= 0 and (st[b] & ~_capi.ST_INEXACT) == 0
            if not (valid or keep_invalid):
                continue
            T = X.shape[0] if (whole or done[b] < 0) else int(done[b])
            laps.append((X[:T, b].copy(), U[:T, b].copy(), G[:T, b].copy(), np.concatenate([fx[b], fg[b]]), int(done[b]), int(st[b])))
        return laps

    def run_pid_laps(self, vt, x0=None, max_steps=1000, stop_at_line=False, keep_invalid=False):
        """len(vt) PID laps (main.py:61-70; Utilities.PID.solve, Utilities.py:60-67), car b at target speed vt[b], the whole lap in one kernel launch (Context.rollout_pid).
        Generator consumption, in this order, with or without the prefetcher: the control-law noise (max_steps, B, 2), then the plant noise (max_steps, B, 3); step t
        of car b uses rows [t, b] of both (device_noise: no consumption -- streams 1 and 0 of one session of the device generator).  Returns the valid laps as run_lap_device does; stop_at_line = False (the reference's multiLap simulator, main.py:57) keeps
        all max_steps rows of a lap -- the rows past the finish line are what an LMPC safe set seeded from the lap needs there --, True the rows up to the crossing."""
        vt = np.atleast_1d(np.asarray(vt, float)); B = vt.shape[0]
        x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1)) if x0 is None else np.asarray(x0, float)
        noise_u = self._draw_noise(max_steps, B, width=2)
        noise = self._draw_noise(max_steps, B)
        self._apply_rows(B, ("tracks", "plant_params"))
        if self._device_noise_session(B):
            t, _ = self.ctx.rollout_pid(x0, x0, vt, None, None, stop_at_line=stop_at_line, T_max=max_steps)
        else:
            t, _ = self.ctx.rollout_pid(x0, x0, vt, noise_u, noise, stop_at_line=stop_at_line)
        out = self.ctx.rollout_fetch(0, t)
        self._fetch_metrics(out[3])
        self.ctx.rollout_end()
        return self._collect(B, *out, whole=not stop_at_line, keep_invalid=keep_invalid)

    def run_mpc_laps(self, x0, A=None, B=None, xLin0=None, uLin0=None, max_steps=1000, stop_at_line=False, keep_invalid=False):
        """x0.shape[0] closed-loop laps of the plain MPC on a numSS_it == 0 context, state resident on the device (Context.rollout_begin_mpc): with A (nb, 6, 6) / B (nb, 6, 2) the LTI
        path-following MPC of main.py:72-80 on those models, else the LTV-MPC of main.py:85-95 from xLin0 / uLin0 (one trajectory for all, or one per rollout) on the
        context's regression store.  Generator consumption: one plant-noise draw (max_steps, nb, 3) (device_noise: none, one session of the device generator).  Returns lap tuples as run_pid_laps does."""
        x0 = np.asarray(x0, float); nb = x0.shape[0]
        noise = self._draw_noise(max_steps, nb)
        self._apply_rows(nb, ("tracks", "plant_params") + (("lap_table",) if A is None else ()) + ("tuning",))      # (the LTI form runs no regression)
        self._apply_trace(nb)
        self._apply_park(nb)
        kw = dict(T_max=max_steps) if self._device_noise_session(nb) else {}       # (noise is None then: the session's buffer is filled on the device)
        if A is not None:
            self.ctx.rollout_begin_mpc(x0, x0, noise, A=A, B=B, stop_at_line=stop_at_line, **kw)
        else:
            self.ctx.rollout_begin_mpc(x0, x0, noise, xLin0=self._per_rollout(xLin0, nb), uLin0=self._per_rollout(uLin0, nb), stop_at_line=stop_at_line, **kw)
        t, _ = self.ctx.rollout_run(max_steps)
        out = self.ctx.rollout_fetch(0, t)
        self._fetch_trace(t, out[3])
        self._fetch_parked()
        self._fetch_metrics(out[3])
        self.ctx.rollout_end()
        return self._collect(nb, *out, whole=not stop_at_line, keep_invalid=keep_invalid)


LTI_LAMB = 0.0000001                   # main.py:74
BOOTSTRAP_STORE_LAPS = 4               # PID laps in the shared regression store of bootstrap()'s LTV-MPC stage (main.py:102-104 gives its LMPC model four as well)


def mpc_stage_config(track, N, vt, max_batch, trToUse=1, device=0):
    """LmpcConfig of main.py's two MPC stages: the values of initMPCParams (initControllerParameters.py:4-26), no terminal set."""
    track = np.asarray(track, float)
    Fx = np.array([[0., 0., 0., 0., 0., 1.], [0., 0., 0., 0., 0., -1.]])
    Fu = np.kron(np.eye(2), np.array([1, -1])).T
    return _capi.config_from(N, np.diag([1.0, 1.0, 1, 1, 0.0, 100.0]), np.diag([1.0, 10.0]), np.zeros((6, 6)), np.zeros(2), np.array([0., 50.]),
                             Fx, [2., 2.], Fu, [0.5, 0.5, 10.0, 10.0], np.array([float(vt), 0, 0, 0, 0, 0]), numSS_it=0, trToUse=int(trToUse), track=track,
                             trackLength=float(track[-1, 3] + track[-1, 4]), max_batch=int(max_batch), device=int(device))


def bootstrap(track, B, N, vt, seed, device=0, max_steps=1000, vt_mpc=None, plant_params=None, device_noise=False, per_car_store=False, tuning=None, tracks=None):
    """main.py:61-95 for B cars without a host round trip inside a lap: PID laps -> one LTI model per car (batched Utilities.Regression, lamb = 1e-7) -> LTI-MPC laps,
    car b on its own (A_b, B_b) -> LTV-MPC laps.  vt: the PID target speed, one value (main.py:50) or one per car; the MPC stages track vt_mpc (default: vt, or the
    mean of the per-car values).  Every stage runs max_steps steps from x0 = [0.5, 0, 0, 0, 0, 0] like the reference's multiLap simulator (main.py:45, 57).

    The LTV-MPC rollouts share ONE regression store (the context's): it holds the min(B, 4) PID laps whose target speed is nearest to vt_mpc, lowest car index
    first among equals -- the local regression weighs stored points by their distance to the linearisation point, so laps driven near the speed the MPC tracks
    are the data it uses, and four is what main.py:102-104 gives the LMPC's model.  Every rollout starts its linearisation from the first N + 1 rows of the LAST
    stored lap (MPC.__init__, PredictiveControllers.py:88-90).  With B = 1 that is the car's own single PID lap, main.py:88-89.

    per_car_store: main.py:88-95 replicated per car instead -- ALL B PID laps go into the store (trToUse = 1), in car order, and a lap table gives car b its own lap
    as its only regression data (Context.model_set_lap_table, row b = [b]); car b starts its linearisation from the first N + 1 rows of its own lap
    (PredictiveControllers.py:88-90).  Each car's LTV model is then identified from what that car's vehicle did, which is what matters with plant_params.
    store_laps lists all B cars.

    plant_params: vehicle constants (one row, or one per car; _capi.plant_params) of all three stages -- car b drives the same vehicle in its PID, LTI-MPC and LTV-MPC
    lap; None: the reference's vehicle.

    tracks: the cars' tracks in all three stages (BatchedRollouts(tracks=): one table, or one per car); None: every car on `track`.  `track` stays the table of the
    context's configuration.  With cars on different tracks use per_car_store: a lap of another track is no regression data for a car.

    tuning: controller tuning of the two MPC stages (one row, or one per car; _capi.tuning_rows on mpc_stage_config) -- e.g. a target speed xRef[0] per car; None: the
    values of mpc_stage_config for every car.

    One generator seeded with `seed` feeds all stages in the order PID control-law noise, PID plant noise, LTI-MPC plant noise, LTV-MPC plant noise.
    device_noise: the disturbances are generated on the device instead (BatchedRollouts(device_noise=True)): the three stages are sessions 0, 1 and 2 of `seed`.
    Returns dict(pid=, mpc=, ltvmpc= lists of lap tuples (x, u, x_glob, final12, done_at, status) with every car in it, flagged or not -- check `status` and
    `done_at` --, A=, B=, Error=, lti_status=, store_laps= the cars whose PID laps went into the shared store): seed_lmpc(ctx, [pid[b] for b in store_laps]) seeds an
    LMPC context with them as main.py:102-110 does with its PID lap."""
    track = np.asarray(track, float)
    vt = np.broadcast_to(np.asarray(vt, float), (B,)).copy()
    vt_mpc = float(vt.mean()) if vt_mpc is None else float(vt_mpc)
    n_store = B if per_car_store else min(B, BOOTSTRAP_STORE_LAPS)
    ctx = _capi.Context(mpc_stage_config(track, N, vt_mpc, B, trToUse=1 if per_car_store else n_store, device=device))
    try:
        ro = BatchedRollouts(ctx, track, seed=seed, plant_params=plant_params, device_noise=device_noise, tuning=tuning, tracks=tracks)
    except Exception:
        ctx.close()
        raise
    try:
        x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1))
        pid = ro.run_pid_laps(vt, x0, max_steps=max_steps, keep_invalid=True)
        A, Bm, Err, lst = _capi.lti_regression_batch([(l[0], l[1]) for l in pid], LTI_LAMB, device=device)
        mpc = ro.run_mpc_laps(x0, A=A, B=Bm, max_steps=max_steps, keep_invalid=True)
        order = list(range(B)) if per_car_store else sorted(range(B), key=lambda b: (abs(vt[b] - vt_mpc), b))[:n_store]
        for b in order:
            ctx.model_add_trajectory(pid[b][0], pid[b][1])
        if per_car_store:                           # car b: insertion index b, its own lap and nothing else; its own first N + 1 rows to linearise about
            ro.lap_table = _capi.check_lap_table(np.arange(B).reshape(B, 1), 1)
            ltv = ro.run_mpc_laps(x0, xLin0=np.stack([l[0][0:N + 1] for l in pid]), uLin0=np.stack([l[1][0:N] for l in pid]), max_steps=max_steps, keep_invalid=True)
        else:
            last = pid[order[-1]]                   # xStored[-1]: laps of equal length keep their insertion order (PredictiveModel.py:35-46)
            ltv = ro.run_mpc_laps(x0, xLin0=last[0][0:N + 1], uLin0=last[1][0:N], max_steps=max_steps, keep_invalid=True)
    finally:
        ro.close()
        ctx.close()
    return dict(pid=pid, mpc=mpc, ltvmpc=ltv, A=A, B=Bm, Error=Err, lti_status=lst, store_laps=order)


def lap_from_global(ctx, xglob, max_ey, TL=None):
    """xglob (T, B, 6): the logs of B cars at once, car b of the log on track row b of the context (Context.track_set) and s made continuous with car b's own
    TrackLength -- TL: one length or (B,), default: the rows in force on the context, else its configuration's.  Returns (T, B, 6).  xglob (T, 6):
    One lap recorded in the inertial frame -- (T, 6) rows [vx, vy, wz, psi, X, Y], the reference's x_glob -- as the (T, 6) curvilinear rows [vx, vy, wz, epsi, s, ey]
    the lap stores take (Context.state_from_global: Map.getLocalPosition per row, Track.py:191-290).  The map returns s on the first lap; here s is made continuous
    across finish-line crossings: from every row whose s drops by more than TrackLength / 2 against the row before, one more TrackLength is added, so a multi-lap
    PID lap comes back with s running past TrackLength, as seed_lmpc expects.  TL: the track length (default: the context's).  max_ey: the reference's
    halfWidth + slack.  Raises LmpcError naming the first row the map places on no segment (ST_NO_SEGMENT)."""
    xg = np.asarray(xglob, float)
    if xg.ndim not in (2, 3) or xg.shape[-1] != 6 or xg.shape[0] < 1:
        raise ValueError("lap_from_global: (T, 6) or (T, B, 6) rows [vx, vy, wz, psi, X, Y] expected, got shape %s" % (xg.shape,))
    if TL is None:
        rows = ctx.tracks() if hasattr(ctx, "tracks") else np.zeros((0, 0))
        TL = rows[:, 1] if rows.shape[0] else ctx.cfg.trackLength
    TL = np.asarray(TL, float)
    x, st = ctx.state_from_global(xg, max_ey)
    x = np.array(x, float).reshape(xg.shape); st = np.asarray(st).reshape(xg.shape[:-1])
    bad = np.argwhere(st & _capi.ST_NO_SEGMENT)
    if bad.size:
        r = tuple(int(i) for i in bad[0])
        raise _capi.LmpcError("lap_from_global: row %s (X = %r, Y = %r, psi = %r) lies on no track segment within max_ey = %r (LMPC_ST_NO_SEGMENT)"
                              % (r[0] if len(r) == 1 else r, xg[r + (4,)], xg[r + (5,)], xg[r + (3,)], float(max_ey)))
    if xg.ndim == 2:
        if TL.size != 1:
            raise ValueError("lap_from_global: one (T, 6) lap takes one TrackLength, got %d (per-car tracks: pass the (T, B, 6) log)" % TL.size)
        TL = float(TL.reshape(-1)[0])
        laps = np.concatenate([[0], np.cumsum(np.diff(x[:, 4]) < -TL / 2)])
        x[:, 4] = x[:, 4] + laps * TL
        return x
    if TL.size not in (1, xg.shape[1]):
        raise ValueError("lap_from_global: one TrackLength or one per car (%d) expected, got %d" % (xg.shape[1], TL.size))
    TLb = np.broadcast_to(TL.reshape(-1), (xg.shape[1],))
    laps = np.concatenate([np.zeros((1, xg.shape[1]), int), np.cumsum(np.diff(x[:, :, 4], axis=0) < -TLb[None] / 2, axis=0)])
    x[:, :, 4] = x[:, :, 4] + laps * TLb[None]
    return x


def seed_lmpc(ctx, laps, from_global=False, max_ey=None, track_rows=None):
    """main.py:102-110 with laps of bootstrap(): every (x, u, ...) tuple goes into the regression store (PredictiveModel.addTrajectory) and into the safe set
    (LMPC.addTrajectory) of the LMPC context `ctx`, in the order given; an LMPC context needs numSS_it / trToUse of them.  The reference passes its one PID lap four
    times; bootstrap()'s "pid" laps are such laps -- max_steps rows of a multiLap run, s running past TrackLength -- one per car.
    from_global: each lap is (x_glob, u, ...) recorded in the inertial frame (motion capture, another simulator, the reference's x_glob log) and is converted with
    lap_from_global(ctx, x_glob, max_ey) first; max_ey (the reference's halfWidth + slack) must then be given.
    track_rows: with one track row per car in force on the context (Context.track_set), the row of each lap -- the TrackLength of its Q-function; from_global then
    needs one lap per row, lap i recorded on track i (the laps, cut or padded to one length, are converted as one (T, n, 6) log)."""
    if from_global:
        if max_ey is None:
            raise ValueError("seed_lmpc(from_global=True) needs max_ey (the reference's halfWidth + slack)")
        if track_rows is None:
            laps = [(lap_from_global(ctx, lap[0], max_ey), lap[1]) for lap in laps]
        else:
            if [int(r) for r in track_rows] != list(range(len(laps))):
                raise ValueError("seed_lmpc(from_global=True, track_rows=...): lap i must be the lap of track row i")
            T = max(np.asarray(lap[0]).shape[0] for lap in laps)
            log = np.stack([np.concatenate([np.asarray(lap[0], float), np.tile(np.asarray(lap[0], float)[-1:], (T - np.asarray(lap[0]).shape[0], 1))]) for lap in laps], axis=1)
            x = lap_from_global(ctx, log, max_ey)
            laps = [(x[:np.asarray(lap[0]).shape[0], i], lap[1]) for i, lap in enumerate(laps)]
    for i, lap in enumerate(laps):
        ctx.model_add_trajectory(lap[0], lap[1])
        if track_rows is None:
            ctx.ss_add_trajectory(lap[0], lap[1])
        else:
            ctx.ss_add_trajectory(lap[0], lap[1], track_row=int(track_rows[i]))


class LmpcGeneration:
    """Iterated batched LMPC over all ranks.  Generation g: every rank runs its shard of rollouts for one lap; the K
    globally fastest valid laps are exchanged (one all-gather of device-packed records) and appended to the model store and the
    safe set of every rank in identical order.  Generation g+1 starts its rollouts from the states in which those K laps crossed
    the finish line (the reference's xF, SysModel.py:50), and the first `ext` steps of the rollout continuing lap k extend stored
    lap k past the finish line -- the batched form of LMPC.addPoint (:466-474), without which no safe-set point lies beyond the
    line and the terminal constraint would stop the cars in front of it.

    The rollouts may drive different vehicles (BatchedRollouts(plant_params=...): rows for the cars of the rank's shard).  The safe set and the regression store
    stay SHARED: a lap driven by one vehicle then serves as terminal set and as regression data for the others (BatchedRollouts(lap_table=...) can give each car
    its own regression laps and BatchedRollouts(ss_table=...) its own safe set, but this class hands out neither: PerCarLMPC below is the loop with nothing
    shared).  Whether that is wanted -- robustness of a
    learned safe set against model mismatch -- or not is the caller's decision; nothing here keeps vehicles apart."""

    def __init__(self, rollouts, total_rollouts, K=4, T_max=400, ext=40, comm=None):
        self.ro, self.total, self.K, self.T_max, self.ext = rollouts, total_rollouts, K, T_max, ext
        trk = getattr(rollouts, "tracks", None)
        if trk is not None and np.unique(trk, axis=0).shape[0] > 1:      # (one safe set for all cars: a lap of one track is no terminal set on another)
            raise ValueError("LmpcGeneration shares one safe set among its cars: they must be on one track (PerCarLMPC is the loop for cars on different tracks)")
        self.comm = comm or parallel.LocalComm()
        self.rank, self.world = self.comm.rank, self.comm.world
        self.lo, self.hi = parallel.shard(total_rollouts, self.rank, self.world)
        if self.hi <= self.lo:
            raise ValueError("every rank needs at least one rollout (total %d, world %d)" % (total_rollouts, self.world))
        rollouts.noise_shard = (self.lo, self.hi, total_rollouts)
        self.parents = None            # [(x, u, x_glob, final12, stored_lap_index)] of the previous generation
        self.last_exchange = None      # (bytes per rank, seconds) of the last all-gather
        self.last_status = self.last_done = None
        self.skipped_extensions = []   # [(k, status bits)]: stored laps NOT extended in the last generation because the continuing rollout was flagged
        self.open_laps = set()         # stored laps that end at the finish line for good (their extension was skipped): kept out of the safe-set selection
        self.step_hook = None          # developer / test hook: called as step_hook(t) after every simulated step (the lap is then advanced one step per call:
                                       # tests/test_gpu_closed_loop.py samples the session's QPs through Context.debug_rollout_qp)

    def _advance(self, n):
        """ctx.rollout_run(n) -- or, with a step hook, n single steps with the hook in between (stops when every rollout has finished, as rollout_run does)."""
        ctx = self.ro.ctx
        if self.step_hook is None:
            return ctx.rollout_run(n)
        t_end = min(self.T_max, ctx._ro_t + n)
        while True:
            t, nd = ctx.rollout_run(1)
            self.step_hook(t)
            if nd >= self.hi - self.lo or t >= t_end:
                return t, nd

    def close(self):
        """After the last run(): BatchedRollouts.close() (prefetched noise returned to the generator, worker thread ended)."""
        self.ro.close()

    def prepare(self, wait=True):
        """Optional, before the first run(): the first lap's plant noise is drawn now (BatchedRollouts.prefetch_noise) instead of inside the lap."""
        self.ro.prefetch_noise(self.T_max, self.hi - self.lo, wait=wait)

    def run(self, x0_all=None, xLin0=None, uLin0=None):
        import time
        ro, ctx, K, N = self.ro, self.ro.ctx, self.K, self.ro.ctx.N
        lo, hi = self.lo, self.hi
        gb = np.arange(lo, hi)
        if self.parents is None:
            x0 = x0_all[lo:hi]; xg0 = x0.copy()
            xl, ul = xLin0, uLin0
            ext = 0
        else:
            par = gb % K
            fin = np.stack([self.parents[k][3] for k in range(K)])
            x0 = fin[par, 0:6].copy(); x0[:, 4] -= ro.track_lengths(x0.shape[0]) if getattr(ro, "tracks", None) is not None else ro.TL   # xF = x_cl[-1] - [0,0,0,0,TrackLength,0]
            xg0 = fin[par, 6:12].copy()
            xl = np.stack([self.parents[k][0][1:N + 2] for k in par]); ul = np.stack([self.parents[k][1][1:N + 1] for k in par])
            ext = self.ext
        ro.begin(x0, xl, ul, xg0, self.T_max)
        undo = []                      # (stored lap, rows before this generation's extension): a generation completes or leaves the safe set as it found it
        open_before = set(self.open_laps)
        try:
            self._apply_selection()    # (the laps added by the previous generation take part from the first step on)
            if ext > 0:
                # the rollout with GLOBAL index k (k < K) continues stored lap k: its first ext points extend that lap on every rank.
                # Each row is taken from the rank whose shard holds rollout k, together with that rollout's accumulated status bits: a row of a
                # flagged rollout (anything but INEXACT) or a non-finite row never reaches a lap store -- decided from the gathered data, hence
                # identically on every rank.
                t, _ = self._advance(ext)
                X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
                n = min(t, ext)
                buf = np.zeros((K, ext, 9)); mask = np.zeros(K, dtype=np.int64)
                for k in range(K):
                    if lo <= k < hi:
                        buf[k, :n, 0:6] = X[:n, k - lo]; buf[k, :n, 6:8] = U[:n, k - lo]; buf[k, :, 8] = float(st[k - lo]); mask[k] = 1
                rows, owned = parallel.gather_owned_rows(buf, mask, self.comm)
                nmin = int(self.comm.allreduce_max(-float(n))[0] * -1)                 # rows every owner really logged
                self.skipped_extensions = []
                for k in range(K):
                    if not owned[k] or nmin <= 0:
                        continue                                                   # (no rows to append: the lap stays open, see below)
                    clean = (int(rows[k, 0, 8]) & ~_capi.ST_INEXACT) == 0 and bool(np.all(np.isfinite(rows[k, :nmin, 0:8])))
                    if not clean:
                        self.skipped_extensions.append((k, int(rows[k, 0, 8])))
                        continue
                    lap = self.parents[k][4]
                    undo.append((lap, ctx.ss_lap_rows(lap)))
                    ctx.ss_extend_lap(lap, rows[k, :nmin, 0:6], rows[k, :nmin, 6:8])
                # A stored lap whose extension was skipped ends AT the finish line: a car approaching the line would find its 13-row window running
                # past the lap's end (LMPC_ST_WINDOW -- the reference's IndexError, :497) on every step there.  Such a lap stays in the store (and in the
                # regression data) but is left out of the safe-set selection from now on: the numSS_it fastest laps among the others are used --
                # decided from the gathered rows, hence identically on every rank.
                self.open_laps |= {self.parents[k][4] for k, _ in self.skipped_extensions} | {self.parents[k][4] for k in range(K) if nmin <= 0 or not owned[k]}
                self._apply_selection()
            self._advance(self.T_max)
            _, _, _, self.last_done, self.last_status, _, _ = ctx.rollout_fetch(0, 0)     # per-rollout finish step / accumulated status bits
            t0 = time.perf_counter()
            # The device-packed exchange needs the context's own RCCL communicator spanning the same world as `comm` (or a single process);
            # any other communicator object (parallel.py: "any object with rank / world / allgather / ...") takes the host-packed path.
            c_rank, c_world, c_rccl = ctx.comm_info()
            if self.world > 1 and c_rccl and c_world != self.world:
                raise RuntimeError("communicator world %d does not match the context's RCCL communicator (world %d)" % (self.world, c_world))
            device_path = self.world == 1 or (c_rccl and c_world == self.world)
            recs, lens, n_valid = ctx.rollout_exchange(K, self.T_max) if device_path else self._host_exchange()
            self.last_exchange = (recs[0].nbytes + lens[0].nbytes, time.perf_counter() - t0)
            ctx.rollout_end()
            best = parallel.top_k(recs, lens, K, self.T_max)
            if len(best) < K:
                raise RuntimeError("only %d valid laps among %d rollouts (need K = %d): the others did not finish within %d steps or were flagged"
                                   % (len(best), self.total, K, self.T_max))
        except Exception:
            for lap, rows_before in undo:
                ctx.ss_truncate_lap(lap, rows_before)
            self.open_laps = open_before
            # ... and the selection as it was: the library's own argsort(LapTime) when no lap was open before, else the choice that goes with the old set
            if open_before:
                self._apply_selection()
            else:
                ctx.ss_set_selected([])
            raise
        self.parents = []
        for x, u, xg, src, T, extra in best:
            ctx.ss_add_trajectory(x, u)
            ctx.model_add_trajectory(x, u)
            self.parents.append((x, u, xg, extra[:12], ctx.ss_num_laps() - 1))
        return best

    def _apply_selection(self):
        """Safe-set selection of this generation: the library's own choice -- the numSS_it fastest stored laps, argsort(LapTime) (:395, 402) -- unless
        some stored lap never got its extension past the finish line (`open_laps`): then the numSS_it fastest of the OTHER laps, handed over explicitly."""
        ctx = self.ro.ctx
        if not self.open_laps:
            return
        L = ctx.cfg.numSS_it
        usable = [l for l in range(ctx.ss_num_laps()) if l not in self.open_laps]
        if len(usable) < L:
            raise RuntimeError("fewer than numSS_it = %d stored laps have their extension past the finish line" % L)
        usable.sort(key=lambda l: (ctx.ss_lap_time(l), l))                  # stable argsort(LapTime)
        ctx.ss_set_selected(usable[:L])

    def _host_exchange(self):
        """Same exchange with host-packed records over a caller-supplied communicator (CPU tests)."""
        ctx = self.ro.ctx
        X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, ctx._ro_t)
        valid = [b for b in range(X.shape[1]) if done[b] >= 0 and (st[b] & ~_capi.ST_INEXACT) == 0]
        laps = [(X[:done[b], b], U[:done[b], b], G[:done[b], b], np.concatenate([fx[b], fg[b]])) for b in valid]
        rec, ln = parallel.pack_laps(laps, self.K, self.T_max, ids=valid)        # (the record carries the rollout's index in the shard, as the device-packed records do)
        return self.comm.allgather(rec), self.comm.allgather(ln), len(laps)


def lap_and_exchange(rollouts, x0_all, xLin0, uLin0, K, T_max, comm=None):
    """One generation over all ranks (first generation form: explicit start states), device-resident."""
    gen = LmpcGeneration(rollouts, x0_all.shape[0], K=K, T_max=T_max, ext=0, comm=comm)
    return gen.run(x0_all, xLin0, uLin0)


class PerCarHistory:
    """What one store holds of every car, as the reference's per-object lists do (LMPC.LapTime, PredictiveModel's sorted xStored): per car the (length, index)
    entries in the order they were added, the same lap any number of times.  row(b): the `width` fastest entries of car b -- a stable argsort of the lengths over
    the car's own list, multiplicities kept -- as store indices: a row of the lap tables."""

    def __init__(self, B, width):
        self.width = int(width)
        self.entries = [[] for _ in range(int(B))]

    def add(self, b, length, index, times=1):
        self.entries[b].extend([(int(length), int(index))] * int(times))

    def row(self, b):
        e = self.entries[b]
        if len(e) < self.width:
            raise ValueError("car %d has %d history entries, %d are needed" % (b, len(e), self.width))
        return [e[i][1] for i in sorted(range(len(e)), key=lambda i: e[i][0])[:self.width]]      # (sorted is stable)

    def rows(self):
        return np.array([self.row(b) for b in range(len(self.entries))], np.int32)

    def prune(self):
        """Every car's list cut to its `width` fastest entries, in the order they were added, multiplicities kept.  row(b) is what it was, now and after any later
        add: a stable "width fastest" never takes back an entry that `width` others of the list already precede, and entries added later go behind these."""
        for b, e in enumerate(self.entries):
            keep = sorted(sorted(range(len(e)), key=lambda i: e[i][0])[:self.width])
            self.entries[b] = [e[i] for i in keep]

    def remap(self, map):
        """Store indices renumbered: entry (length, index) becomes (length, map[index]) -- the map Context.store_retain returns; every index held must be a kept one."""
        for b, e in enumerate(self.entries):
            if any(map[i] < 0 for _, i in e):
                raise ValueError("car %d's history names a lap that was not kept" % b)
            self.entries[b] = [(n, int(map[i])) for n, i in e]

    def indices(self):
        """The store indices any car's list holds, as a set."""
        return {i for e in self.entries for _, i in e}


class PerCarLMPC:
    """main.py:100-121 once per car, with nothing shared: B independent learners in one batch.  Car b regresses on its own laps (Context.model_set_lap_table) and
    takes its terminal set and terminal cost from its own laps (Context.ss_set_lap_table), with `last[b]` = its own most recent lap -- every controller object of
    the reference owns both stores (PredictiveControllers.py:395-412, PredictiveModel.py:35-46).  With BatchedRollouts(plant_params=...) each car also drives its own
    vehicle.  No collectives are needed: the cars are independent, and a rank runs its shard with `rollouts.noise_shard` set.

    seed(laps_per_car): entry b is one lap tuple (x, u, x_glob, final12, ...) as run_pid_laps / bootstrap return them, or a list of them.  Every lap is stored ONCE in
    both stores; the car's history starts as its laps, the fastest one repeated until numSS_it (safe set) and trToUse (regression) entries are there -- the
    reference's four copies of the PID lap (main.py:103-110) without the copies.
    run(): one generation.  Car b starts from its own finish state (xF, SysModel.py:50) and linearises about the first rows of its latest lap; the first `ext` steps
    of car b extend car b's own latest lap past the finish line (the batched LMPC.addPoint, :466-474; ClosedLoop's rules: never rows of a flagged rollout, never
    non-finite rows) unless that lap was stored with its rows past the line already (a multiLap PID lap); then the lap is finished, every valid lap is added to both
    stores, and row b of both tables becomes the numSS_it / trToUse fastest entries of car b's history with last[b] = the lap just added.
    A car whose lap is not valid -- not finished within T_max, flagged with anything but ST_INEXACT, or its extension skipped -- is RETIRED:
    retired[b] = (generation, status).  It keeps its slot in the batch, so that indices, noise streams and rows of the others do not move; its later laps are ignored.
    lap_times[b]: the steps of car b's laps, generation by generation.
    device_commit=True: the laps never leave the device.  The extension is one Context.rollout_extend_laps call and the adds one Context.rollout_commit_laps call
    per generation, over the same cars in the same order, so store indices, histories, tables, `last`, lap_times and `retired` come out as without it (an entry
    that comes back not extended -- a non-finite row -- retires its car with EXT_SKIPPED); only status words, crossing steps, final states and the first N + 2
    logged rows are downloaded.  The tuples run() returns, and latest[b], then carry only the first min(T, N + 2) rows of x and u -- what the next generation
    linearises about -- and None for x_glob; the full lap is in the stores (Context.store_read_lap).
    tuning: rows of _capi.tuning_rows, one for all cars or one per car -- what BatchedRollouts(tuning=) takes; car b then also runs its own controller tuning.
    trace / trace_what: what BatchedRollouts(trace=) takes; `traces` then holds one entry per generation, the session's trace (planes, "cars", "doneAt"), the same with
    and without device_commit -- TraceView(track, car, traces) is one car's history as the reference's plots read an LMPC object.
    Tracks: with BatchedRollouts(tracks=) holding one track per car, car b drives, regresses and selects on its own track; its start state is its crossing state
    shifted by its OWN TrackLength, and its laps and extensions are stored with track_row = b (Context.ss_add_trajectory / ss_extend_lap, or the device commit, which
    takes the car's row by itself).
    park=True: every generation begins with the retired cars parked from step 0 and _capi.PARK_FINISHED set (Context.rollout_set_parking), with and without
    device_commit: a retired car is no longer solved, a car that has crossed the line leaves the launches at the next poll, and the session ends when no car is
    live instead of at T_max.  Stores, histories, tables, `last`, lap_times, `retired` and the returned tuples come out as without it; `steps[g]` -- the session steps
    generation g took -- is what differs.  (A lap that crosses the line within the first `ext` steps, whose extension rows a parked car no longer logs, is refused.)
    park=_capi.PARK_REROUTE adds that bit: the solve route then follows the live count, and another route answers to the routes' bound (2e-7 in x, u), not bit for
    bit -- the laps are no longer promised equal to those without parking.  The rollouts object's own `park` is put back after every generation.
    metrics=True: `metrics[g]` is the (B, _capi.METRICS_NCOL) lap metrics of generation g (columns _capi.METRIC_FIELDS): one Context.rollout_lap_metrics call over the
    generation's valid cars, up to their crossing steps, before the session ends -- with and without device_commit, with and without park; NaN rows for cars that
    are retired or not valid.  Everything else comes out as without it.
    prune=True: the stores hold only what a car can still read.  After seed and after every generation's adds both histories are cut to their rows
    (PerCarHistory.prune) and ONE Context.store_retain call keeps, in the safe set, the union over the cars of row b and last[b], and in the regression store the union
    of the rows; histories, `last` and the tables handed over are renumbered through the maps it returns.  A lap that has dropped out of a car's row can never come
    back into it, so what run() returns, lap_times, retired, steps, latest and metrics are identical to prune=False; only store indices differ, through the maps
    (the two stores' indices no longer run in lockstep).  Retired cars keep their rows and therefore their laps.  The stores stay bounded whatever the number of
    generations: ss_num_laps() <= B (numSS_it + 1) and model_num_laps() <= B trToUse.  Works with device_commit, park, tuning, tracks, metrics and trace."""

    EXT_SKIPPED = 1 << 30          # retired[b][1] carries this bit when the car's extension was skipped (beside the status bits that caused it, if any)

    def __init__(self, rollouts, T_max=400, ext=40, device_commit=False, tuning=None, trace=None, trace_what=None, park=False, metrics=False, prune=False):
        self.ro, self.T_max, self.ext = rollouts, int(T_max), int(ext)
        self.prune = bool(prune)
        self.with_metrics = bool(metrics)
        self.metrics = []                  # one entry per generation run with metrics=True
        self.device_commit = bool(device_commit)
        self.park = bool(park)             # True, or _capi.PARK_* bits to go with PARK_FINISHED (PARK_REROUTE)
        self.park_mode = _capi.check_parking(_capi.PARK_FINISHED | (0 if park is True or not park else int(park)), None)[0]
        self.steps = []                    # session steps of each generation (T_max or the last crossing's poll without park)
        if trace is not None:              # (the cars whose predictions every generation records: what BatchedRollouts(trace=) takes)
            self.ro.trace = _capi.check_trace(trace, trace_what, self.ro.ctx.cfg.numSS_it)
        self.traces = []                   # one entry per generation run with a trace: the rollouts object's last_trace of that session
        if tuning is not None:             # (one row, or one per car: each learner its own cost weights and bounds; the rollouts object hands them to the context before every begin)
            self.ro.tuning = _capi.check_tuning(tuning, self.ro.ctx.cfg.numSS_it)
        self.B = None
        self.generation = 0
        self.retired = {}
        self.lap_times = []
        self.last_status = self.last_done = None

    def seed(self, laps_per_car):
        ctx = self.ro.ctx
        if ctx.ss_num_laps() != 0 or ctx.model_num_laps() != 0:      # (one counter below numbers the laps of both stores)
            raise ValueError("PerCarLMPC.seed needs a context with empty lap stores")
        laps_per_car = [list(l) if isinstance(l, list) else [l] for l in laps_per_car]
        B = self.B = len(laps_per_car)
        self.ro._apply_rows(B, ("tracks",))           # (per-car tracks: car b's laps are stored with the TrackLength of row b)
        self.ss_hist, self.model_hist = PerCarHistory(B, ctx.cfg.numSS_it), PerCarHistory(B, ctx.cfg.trToUse)
        self.last = np.full(B, -1, np.int32)
        self.latest = [None] * B           # (x, u, final12, ends at the line) of each car's most recent lap
        self.lap_times = [[] for _ in range(B)]
        n = 0                              # laps stored so far: the next index in both stores, which start empty (safe-set lap index, regression-store insertion index)
        for b, laps in enumerate(laps_per_car):
            if not laps:
                raise ValueError("PerCarLMPC.seed: car %d has no lap" % b)
            first = n
            for lap in laps:
                x, u = np.asarray(lap[0], float), np.asarray(lap[1], float)
                ctx.model_add_trajectory(x, u); self._ss_add(b, x, u)
                self.ss_hist.add(b, x.shape[0], n); self.model_hist.add(b, x.shape[0], n)
                n += 1
            lens = [np.asarray(l[0]).shape[0] for l in laps]
            k = int(np.argmin(lens))                       # (np.argmin: the first among equals)
            for hist in (self.ss_hist, self.model_hist):
                hist.add(b, lens[k], first + k, times=max(0, hist.width - len(laps)))
            lap = laps[-1]
            x = np.asarray(lap[0], float)
            done = int(lap[4]) if len(lap) > 4 else x.shape[0]
            self.latest[b] = (x, np.asarray(lap[1], float), np.asarray(lap[3], float), done >= x.shape[0])
            self.last[b] = n - 1
        self._hand_tables()
        self._retain()

    def _ss_add(self, b, x, u):
        """Car b's lap into the safe set, its Q-function counted with car b's own TrackLength."""
        row = self.ro.track_row_of(b)
        if row is None:
            self.ro.ctx.ss_add_trajectory(x, u)
        else:
            self.ro.ctx.ss_add_trajectory(x, u, track_row=row)

    def _hand_tables(self):
        """Rows of both tables and `last`, from the histories, to the rollouts object (it hands them to the context before the next begin)."""
        self.ro.lap_table = _capi.check_lap_table(self.model_hist.rows(), self.model_hist.width)
        self.ro.ss_table, self.ro.ss_last = _capi.check_ss_table(self.ss_hist.rows(), self.ss_hist.width, self.last.copy())

    def _retain(self):
        """prune=True: the laps no car reads any more are given back (Context.store_retain), histories, `last` and the tables renumbered.  The tables in force on the
        context are those of the session that has just ended and may name laps about to go, so the new ones go to the context first."""
        if not self.prune:
            return
        ro, ctx = self.ro, self.ro.ctx
        ctx.model_set_lap_table(ro.lap_table); ctx.ss_set_lap_table(ro.ss_table, ro.ss_last)
        self.ss_hist.prune(); self.model_hist.prune()
        keep_ss = sorted(self.ss_hist.indices() | {int(l) for l in self.last if l >= 0})
        keep_model = sorted(self.model_hist.indices())
        map_ss, map_model = ctx.store_retain(ss=keep_ss, model=keep_model)
        self.ss_hist.remap(map_ss); self.model_hist.remap(map_model)
        self.last = np.array([map_ss[l] if l >= 0 else l for l in self.last], np.int32)
        self._hand_tables()

    def close(self):
        self.ro.close()

    def run(self):
        """One generation; returns the lap tuples (x, u, x_glob, final12, done_at, status) of every car, None for a retired one."""
        if self.B is None:
            raise RuntimeError("PerCarLMPC.run before seed")
        if not self.park:
            return self._run()
        own = getattr(self.ro, "park", None)          # (the retired cars are this loop's business: other sessions of the rollouts object keep its own setting)
        try:
            return self._run()
        finally:
            self.ro.park = own

    def _take_metrics(self, valid):
        """metrics[g] of the active session, before rollout_end: the valid cars of this generation up to their crossing steps."""
        if self.with_metrics:
            self.metrics.append(_lap_metrics_rows(self.ro.ctx, self.B, valid))

    def _valid(self, done, st):
        """The cars whose lap of this session counts: not retired, across the line, flagged with nothing but ST_INEXACT."""
        return [b for b in range(self.B) if b not in self.retired and done[b] >= 0 and (int(st[b]) & ~_capi.ST_INEXACT) == 0]

    def _start_arrays(self):
        """(x0, xg0, xLin0, uLin0) of the session about to begin: every car from its own finish state, linearising about the first rows of its latest lap."""
        ro, B, N = self.ro, self.B, self.ro.ctx.N
        fin = np.stack([self.latest[b][2] for b in range(B)])
        x0 = fin[:, 0:6].copy(); x0[:, 4] -= ro.track_lengths(B) if getattr(ro, "tracks", None) is not None else ro.TL   # xF = x_cl[-1] - [0,0,0,0,TrackLength_b,0]: each car's own track
        xg0 = fin[:, 6:12].copy()
        xl = np.stack([self.latest[b][0][1:N + 2] for b in range(B)]); ul = np.stack([self.latest[b][1][1:N + 1] for b in range(B)])
        return x0, xg0, xl, ul

    def _run(self):
        ro, ctx, B, N = self.ro, self.ro.ctx, self.B, self.ro.ctx.N
        gen = self.generation
        x0, xg0, xl, ul = self._start_arrays()
        if self.park:                    # (the retired cars keep their slots and are not stepped; the rollouts object hands this to the context in begin)
            ro.park = _capi.check_parking(self.park_mode, sorted(self.retired))
        ro.begin(x0, xl, ul, xg0, self.T_max)
        if self.device_commit:
            return self._finish_on_device(gen)
        try:
            if self.ext > 0 and any(self.latest[b][3] and b not in self.retired for b in range(B)):
                t, _ = ctx.rollout_run(self.ext)
                X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
                n = min(t, self.ext)
                at = ctx.rollout_parked_at()[0] if self.park else None
                for b in range(B):
                    if b in self.retired or not self.latest[b][3]:
                        continue
                    if at is not None and 0 <= at[b] < n:      # (the device path: rollout_extend_laps refuses the same rows)
                        raise ValueError("PerCarLMPC(park=True): car %d was parked at step %d, inside the %d extension rows" % (b, int(at[b]), n))
                    clean = n > 0 and (int(st[b]) & ~_capi.ST_INEXACT) == 0 and bool(np.all(np.isfinite(X[:n, b]))) and bool(np.all(np.isfinite(U[:n, b])))
                    if not clean:
                        self.retired[b] = (gen, int(st[b]) | self.EXT_SKIPPED)
                        continue
                    if ro.track_row_of(b) is None:
                        ctx.ss_extend_lap(int(self.last[b]), X[:n, b], U[:n, b])     # (the table is live in the session: the next step selects from the longer lap)
                    else:
                        ctx.ss_extend_lap(int(self.last[b]), X[:n, b], U[:n, b], track_row=b)     # (the table is live in the session: the next step selects from the longer lap)
            t, _ = ctx.rollout_run(self.T_max)
            X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t)
            if ro._fetch_trace(t, done) is not None:
                self.traces.append(ro.last_trace)
            ro._fetch_parked()
            self._take_metrics(self._valid(done, st))
        finally:
            ctx.rollout_end()
        self.last_status, self.last_done = st, done
        self.steps.append(int(t))
        out = [None] * B
        for b in range(B):
            if b in self.retired:
                continue
            if not (done[b] >= 0 and (int(st[b]) & ~_capi.ST_INEXACT) == 0):
                self.retired[b] = (gen, int(st[b]))
                continue
            T = int(done[b])
            x, u = X[:T, b].copy(), U[:T, b].copy()
            idx, idx_model = ctx.ss_num_laps(), ctx.model_num_laps()      # (one counter per store: after a store_retain they no longer run in lockstep)
            self._ss_add(b, x, u); ctx.model_add_trajectory(x, u)
            self.ss_hist.add(b, T, idx); self.model_hist.add(b, T, idx_model)
            self.last[b] = idx
            f12 = np.concatenate([fx[b], fg[b]])
            self.latest[b] = (x, u, f12, True)
            self.lap_times[b].append(T)
            out[b] = (x, u, G[:T, b].copy(), f12, T, int(st[b]))
        self._hand_tables()
        self._retain()
        self.generation += 1
        return out

    def _finish_on_device(self, gen):
        """The rest of run() after begin with device_commit: same decisions on the same status words, the rows themselves stay on the device."""
        ro, ctx, B, N = self.ro, self.ro.ctx, self.B, self.ro.ctx.N
        try:
            if self.ext > 0 and any(self.latest[b][3] and b not in self.retired for b in range(B)):
                t, _ = ctx.rollout_run(self.ext)
                _, _, _, done, st, fx, fg = ctx.rollout_fetch(0, 0)
                n = min(t, self.ext)
                cars = []
                for b in range(B):
                    if b in self.retired or not self.latest[b][3]:
                        continue
                    if not (n > 0 and (int(st[b]) & ~_capi.ST_INEXACT) == 0):
                        self.retired[b] = (gen, int(st[b]) | self.EXT_SKIPPED)
                        continue
                    cars.append(b)
                if cars:                                    # (the table is live in the session: the next step selects from the longer laps)
                    extended = ctx.rollout_extend_laps(cars, [int(self.last[b]) for b in cars], n)
                    for b, ok in zip(cars, extended):
                        if not ok:                          # (a non-finite row: the lap is as it was)
                            self.retired[b] = (gen, int(st[b]) | self.EXT_SKIPPED)
            t, _ = ctx.rollout_run(self.T_max)
            _, _, _, done, st, fx, fg = ctx.rollout_fetch(0, 0)
            Xh, Uh = ctx.rollout_fetch(0, min(t, N + 2))[:2]
            if ro._fetch_trace(t, done) is not None:
                self.traces.append(ro.last_trace)
            ro._fetch_parked()
            valid = []
            for b in range(B):
                if b in self.retired:
                    continue
                if not (done[b] >= 0 and (int(st[b]) & ~_capi.ST_INEXACT) == 0):
                    self.retired[b] = (gen, int(st[b]))
                    continue
                valid.append(b)
            self._take_metrics(valid)
            first, first_model = ctx.rollout_commit_laps(valid) if valid else (None, None)
        finally:
            ctx.rollout_end()
        self.last_status, self.last_done = st, done
        self.steps.append(int(t))
        out = [None] * B
        for k, b in enumerate(valid):
            T, idx = int(done[b]), first + k
            x, u = Xh[:T, b].copy(), Uh[:T, b].copy()
            self.ss_hist.add(b, T, idx); self.model_hist.add(b, T, first_model + k)
            self.last[b] = idx
            f12 = np.concatenate([fx[b], fg[b]])
            self.latest[b] = (x, u, f12, True)
            self.lap_times[b].append(T)
            out[b] = (x, u, None, f12, T, int(st[b]))
        self._hand_tables()
        self._retain()
        self.generation += 1
        return out


class FreeRunningLMPC(PerCarLMPC):
    """PerCarLMPC without the shared generation: ONE session holds `laps` laps of every car, and a car starts its next lap at its own crossing
    (Context.rollout_relaunch) while the others keep driving -- the reference's car does the same, its next lap begins at the step after its crossing, from xF
    (main.py:100-121, SysModel.py:50).  Over G laps the session takes about max_b sum_g T(b, g) steps where the lockstep loop takes sum_g max_b T(b, g), with one
    begin / end where it has G.  Same seed(laps_per_car), histories, tables, `retired`, `lap_times`, `latest`, `last` as PerCarLMPC; the laps never leave the device
    (device commit is the only mode).

    run(laps=G, max_steps=None): one session with room for G (T_lap + 8) logged rows (capped by max_steps), driven in chunks that end at the next multiple of 8 --
    the session's own finished-lap poll -- or at the next step where some car is exactly `ext` steps into a lap, whichever comes first.  At a stop where the count of
    finished cars has moved, an extension is due or a car has been T_lap steps in its lap, doneAt, the status words and the crossing states are read
    (rollout_fetch(0, 0)) and, in this order:
      (a) every car exactly `ext` steps into a lap whose predecessor ended at the line extends that predecessor by the lap's first `ext` rows: PerCarLMPC's rule
          (status clean apart from ST_INEXACT, else retired with EXT_SKIPPED), one rollout_extend_laps call for all such cars, an entry that comes back not extended
          retires its car;
      (b) the cars that have crossed since the last stop, in ascending order: the valid ones (_valid) are added to both stores by one rollout_commit_laps call;
          histories, `last`, lap_times are updated and both tables handed to the context; those with laps left to do are relaunched by one rollout_relaunch call;
      (c) a car T_lap steps into a lap without a crossing, or with a bad status word at its crossing, is retired: it keeps its slot and is not relaunched.
    The session ends when no car has a lap left to do or to finish, or at max_steps; a lap unfinished then is dropped.  A car is noticed at the first stop after its
    crossing: at most 7 steps of slack per lap, stepped and thrown away.  Retired cars and cars that have done their laps keep being stepped until the session ends
    (no parking).  Afterwards the rollouts object's `lap` has advanced by the largest number of laps any car began, so later sessions draw fresh noise; prune=True
    runs the store_retain of PerCarLMPC after the session, never inside it.  Returns per car the list of its laps' tuples (head x, head u, None, final12, T, status)
    -- the first min(T, N + 2) rows, as PerCarLMPC(device_commit=True) returns them.  retired[b] = (generation + laps the car had finished in this run, status).
    `steps`: the session steps of each run; `stops`: per run (stops made, stops at which the session was read, seconds spent in them).

    Equivalence: cars are independent problems, the kernels and routes are those of the lockstep session of the same B, per-car tables name the same laps and
    the device noise of car b's k-th lap is that of lockstep generation k.  So `laps` generations of PerCarLMPC(device_commit=True).run() from the same seeds leave
    the same lap_times and retired, and bit for bit the same stored laps (rows, Qfun with its extension rows, LapTime, prefilter images) under every car's history
    -- but store indices follow CROSSING order here and generation-then-car order there: compare laps through the histories, not by index.
    Refused with ValueError: park, trace, metrics (on this object or on the rollouts object), a rollouts object without device_noise, and a lap that crosses the line
    within its first `ext` steps (the extension rows would be those of the next lap)."""

    def __init__(self, rollouts, T_lap=400, ext=40, tuning=None, prune=False, park=False, trace=None, trace_what=None, metrics=False):
        for name, on in (("park", park), ("trace", trace is not None), ("metrics", metrics),
                         ("park", getattr(rollouts, "park", None) is not None), ("trace", getattr(rollouts, "trace", None) is not None), ("metrics", getattr(rollouts, "metrics", False))):
            if on:
                raise ValueError("FreeRunningLMPC: %s is not available in a session that changes laps (Context.rollout_relaunch refuses it); use PerCarLMPC" % name)
        if not getattr(rollouts, "device_noise", False):
            raise ValueError("FreeRunningLMPC: the rollouts object must draw on the device (BatchedRollouts(device_noise=True)): a car's next lap redraws its own noise rows")
        PerCarLMPC.__init__(self, rollouts, T_max=T_lap, ext=ext, device_commit=True, tuning=tuning, prune=prune)
        self.T_lap = self.T_max
        self.stops = []

    def run(self, laps=1, max_steps=None):
        import time
        if self.B is None:
            raise RuntimeError("FreeRunningLMPC.run before seed")
        G = int(laps)
        if G < 1:
            raise ValueError("FreeRunningLMPC.run: laps = %d, at least one expected" % G)
        ro, ctx, B, N, T_lap, ext = self.ro, self.ro.ctx, self.B, self.ro.ctx.N, self.T_lap, self.ext
        for name in ("park", "trace"):
            if getattr(ro, name, None) is not None:
                raise ValueError("FreeRunningLMPC: the rollouts object has %s set" % name)
        cap = G * (T_lap + 8) if max_steps is None else min(G * (T_lap + 8), int(max_steps))
        gen0 = self.generation
        x0, xg0, xl, ul = self._start_arrays()
        ro.begin(x0, xl, ul, xg0, cap)
        start = np.zeros(B, np.int64)                      # session row each car's current lap began at
        began = np.ones(B, np.int64)                       # laps begun in this run
        stored = np.zeros(B, np.int64)                     # laps of this run in the stores
        live = np.array([b not in self.retired for b in range(B)])            # driving a lap that counts
        ext_due = np.array([bool(live[b] and ext > 0 and self.latest[b][3]) for b in range(B)])   # the current lap still has its predecessor to extend
        out = [[] for _ in range(B)]
        t, nd_known, n_stops, n_reads, t_stops = 0, 0, 0, 0, 0.0
        done = st = None
        try:
            while live.any() and t < cap:
                nxt = min((t // 8 + 1) * 8, cap)
                for b in np.flatnonzero(ext_due):
                    if t < start[b] + ext < nxt:
                        nxt = int(start[b] + ext)
                t, nd = ctx.rollout_run(nxt - t)
                tic = time.perf_counter()
                n_stops += 1
                ext_now = [int(b) for b in np.flatnonzero(ext_due) if t - start[b] == ext]
                overdue = [int(b) for b in np.flatnonzero(live) if t - start[b] >= T_lap]
                if nd != nd_known or ext_now or overdue:
                    n_reads += 1
                    _, _, _, done, st, fx, fg = ctx.rollout_fetch(0, 0)
                    gen_of = lambda b: gen0 + int(began[b]) - 1
                    # (a) extensions due
                    cars = []
                    for b in ext_now:
                        if done[b] >= 0:
                            raise ValueError("FreeRunningLMPC: car %d crossed the line %d steps into its lap, inside the %d extension rows" % (b, int(done[b] - start[b]), ext))
                        ext_due[b] = False
                        if (int(st[b]) & ~_capi.ST_INEXACT) != 0:
                            self.retired[b] = (gen_of(b), int(st[b]) | self.EXT_SKIPPED); live[b] = False
                            continue
                        cars.append(b)
                    if cars:                               # (the safe-set table is live in the session: the next step selects from the longer laps)
                        extended = ctx.rollout_extend_laps(cars, [int(self.last[b]) for b in cars], ext)
                        for b, ok in zip(cars, extended):
                            if not ok:                     # (a non-finite row: the lap is as it was)
                                self.retired[b] = (gen_of(b), int(st[b]) | self.EXT_SKIPPED); live[b] = False
                    # (b) the cars that have crossed since the last stop
                    crossed = [int(b) for b in np.flatnonzero(live) if done[b] >= 0]
                    for b in crossed:
                        if ext_due[b]:
                            raise ValueError("FreeRunningLMPC: car %d crossed the line %d steps into its lap, inside the %d extension rows" % (b, int(done[b] - start[b]), ext))
                    ok_set = set(self._valid(done, st))
                    valid = [b for b in crossed if b in ok_set and done[b] - start[b] <= T_lap]
                    again = []
                    if valid:
                        first, first_model = ctx.rollout_commit_laps(valid)
                        heads = {}                         # the first N + 2 rows behind a lap start, fetched once per distinct start (cars relaunched at one stop share theirs)
                        for k, b in enumerate(valid):
                            T, s = int(done[b] - start[b]), int(start[b])
                            if s not in heads:
                                heads[s] = ctx.rollout_fetch(s, min(s + N + 2, t))[:2]
                            x, u = heads[s][0][:min(T, N + 2), b].copy(), heads[s][1][:min(T, N + 2), b].copy()
                            self.ss_hist.add(b, T, first + k); self.model_hist.add(b, T, first_model + k)
                            self.last[b] = first + k
                            f12 = np.concatenate([fx[b], fg[b]])
                            self.latest[b] = (x, u, f12, True)
                            self.lap_times[b].append(T)
                            out[b].append((x, u, None, f12, T, int(st[b])))
                            stored[b] += 1
                            if stored[b] < G:
                                again.append(b)
                            else:
                                live[b] = False
                        for b in valid:                    # what _hand_tables makes of the histories, for the rows that have changed (a stop must not cost O(B) on the host)
                            ro.lap_table[b] = self.model_hist.row(b); ro.ss_table[b] = self.ss_hist.row(b); ro.ss_last[b] = self.last[b]
                        # (the regression row of a relaunched car is taken from the context's table at the relaunch; the safe-set table is live)
                        ctx.model_set_lap_table(ro.lap_table); ctx.ss_set_lap_table(ro.ss_table, ro.ss_last)
                    if again:
                        ctx.rollout_relaunch(again, T_lap + 8)
                        for b in again:
                            start[b] = t; began[b] += 1; ext_due[b] = ext > 0
                    # (c) overdue, or flagged at the crossing
                    for b in np.flatnonzero(live):
                        b = int(b)
                        if b in again:
                            continue
                        if done[b] >= 0 or t - start[b] >= T_lap:
                            self.retired[b] = (gen_of(b), int(st[b])); live[b] = False
                    nd_known = int((np.asarray(done) >= 0).sum()) - len(again)
                t_stops += time.perf_counter() - tic
        finally:
            ctx.rollout_end()
        ro.lap += int(began.max()) - 1                     # (begin counted one session: every further lap begun has drawn the next lap word)
        self.last_status, self.last_done = st, done
        self.steps.append(int(t))
        self.stops.append((n_stops, n_reads, t_stops))
        self._hand_tables()
        self._retain()
        self.generation += int(began.max())
        return out


def _track_angle(table, s):
    """Tangent angle of the centre line at arc length s of a PointAndTangent table (Track.py:54-133: column 2 is the angle at a row's END point); NaN on no row."""
    TL = table[-1, 3] + table[-1, 4]
    s = np.mod(np.asarray(s, float), TL)
    out = np.full(s.shape, np.nan)
    for i in range(table.shape[0]):
        on = (s >= table[i, 3]) & (s < table[i, 3] + table[i, 4])
        out[on] = table[i, 2] if table[i, 5] == 0.0 else table[i - 1, 2] + (s[on] - table[i, 3]) * table[i, 5]
    return out


class TraceView:
    """One car's history in the attribute shape the reference's plots read from an LMPC object (plot.py:50-103 plotClosedLoopLMPC, :106-175 animation_xy,
    animation_states): SS_glob, LapTime, SS, uSS, it, N, numSS_Points, xStoredPredTraj[it][i] (N + 1, 6), uStoredPredTraj[it][i] (N, 2) and SSStoredPredTraj[it][i]
    (S, 6) -- the three per-step logs of LMPC.unpackSolution (PredictiveControllers.py:364-379) -- built from session traces instead of a host loop.  Beside them
    xyPred[it][i] (N + 1, 2) and xySS[it][i] (S, 2), the inertial positions the device has already mapped (no per-point getGlobalPosition on the host), qSel, iters,
    status and mapStatus where recorded.  Every lap is cut at the car's crossing step (all recorded steps for a car that did not cross).

    track_or_map: the PointAndTangent table of the car's track, or an object that has one (the reference's Map).
    car: the car's index in its batch.
    laps: one entry per lap, in order -- a trace (an element of PerCarLMPC.traces, or BatchedRollouts.last_trace) or a pair (trace, lap) with lap the car's tuple
    (x, u, x_glob, ...) as run_lap_device returns it.  Without the tuple the lap's states and inputs are row 0 of the predictions (x_0 = x0 is an equality row of the
    QP) and SS_glob is put together from them: vx, vy, wz, the track's tangent angle + epsi, and (X, Y) of row 0 of xyPred (NaN without the XY plane)."""

    PLANES = ("xPred", "uPred", "ssSel", "qSel", "xyPred", "xySS", "iters", "status", "mapStatus")

    def __init__(self, track_or_map, car, laps):
        self.track = np.asarray(getattr(track_or_map, "PointAndTangent", track_or_map), float)
        self.TrackLength = float(self.track[-1, 3] + self.track[-1, 4])
        self.car = int(car)
        self.SS, self.uSS, self.SS_glob, self.LapTime = [], [], [], []
        self.xStoredPredTraj, self.uStoredPredTraj, self.SSStoredPredTraj = [], [], []
        self.qSel, self.xyPred, self.xySS, self.iters, self.status, self.mapStatus = [], [], [], [], [], []
        self.N = self.numSS_Points = None
        for entry in laps:
            tr, lap = entry if isinstance(entry, (tuple, list)) else (entry, None)
            where = np.flatnonzero(np.asarray(tr["cars"]) == self.car)
            if where.size != 1:
                raise ValueError("TraceView: car %d is not among the traced cars %s" % (self.car, list(np.asarray(tr["cars"]))))
            k = int(where[0])
            if "xPred" not in tr:
                raise ValueError("TraceView: the trace has no XPRED plane")
            steps = tr["xPred"].shape[0]
            done = int(tr["doneAt"][k])
            T = done if 0 <= done <= steps else steps
            cut = {key: tr[key][:T, k] for key in self.PLANES if key in tr}
            xP = cut["xPred"]
            self.N = xP.shape[1] - 1
            if "ssSel" in cut:
                self.numSS_Points = cut["ssSel"].shape[1]
            if lap is not None:
                x, u, xg = (np.asarray(a, float)[:T] for a in lap[:3])
            else:
                x = xP[:, 0, :].copy()
                u = cut["uPred"][:, 0, :].copy() if "uPred" in cut else np.full((T, 2), np.nan)
                xy = cut["xyPred"][:, 0, :] if "xyPred" in cut else np.full((T, 2), np.nan)
                xg = np.column_stack([x[:, 0:3], _track_angle(self.track, x[:, 4]) + x[:, 3], xy])
            self.SS.append(x); self.uSS.append(u); self.SS_glob.append(xg); self.LapTime.append(T)
            self.xStoredPredTraj.append(xP)
            for name, key in (("uStoredPredTraj", "uPred"), ("SSStoredPredTraj", "ssSel"), ("qSel", "qSel"), ("xyPred", "xyPred"), ("xySS", "xySS"),
                              ("iters", "iters"), ("status", "status"), ("mapStatus", "mapStatus")):
                getattr(self, name).append(cut.get(key))
        self.it = len(self.LapTime)
