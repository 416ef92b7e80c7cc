"""The three stages in front of the LMPC laps (main.py:61-95) as device sessions against the host-stepped loops that were the only way before them:

    python tools/stage_bench.py --stage pid      # lmpc_rollout_pid        vs  bench.pid_laps' loop (NumPy control law + lmpc_plant_step_batch per step)
    python tools/stage_bench.py --stage mpc      # LTI-MPC session         vs  lmpc_qp_solve_batch + lmpc_plant_step_batch per step
    python tools/stage_bench.py --stage ltvmpc   # LTV-MPC session         vs  lmpc_step_batch + lmpc_plant_step_batch + the shift in NumPy per step

One JSON line: per batch size (default 1, 256, 1024; N = 12) simulated steps/s of both ways (car-steps: B x T / seconds; for the MPC stages that is also the rate of
closed-loop QP solves) and the seconds behind them.  Wall clock around work that ends in a drained stream (the session's fetch, the host loop's last download), uploads
of start states and noise included on both sides; every shape is run once untimed first, then `--repeats` times alternating the two ways, medians reported.  Both ways
are fed the same draws, and the tool checks that their logs are equal bit for bit before it reports a time.  --out also writes the line to a file.

--plant-params: every batch size is measured a second time with per-car vehicle constants in force (Context.plant_set_params: all ten constants of every car scaled
by U(0.9, 1.1), generator seeded with 7) -- the per-car instantiations of the plant kernels beside the nominal ones; those rows carry "plant_params": true.

--tracks: every batch size is also measured with track rows in force (Context.track_set): once with ONE row, the L track's own -- the per-car-track kernels on the
geometry of the configuration, the price of reading a row at all --, and once with the cars dealt round-robin over the reference's three tracks (racinglmpc_amd.track:
L, oval, goggle); those rows carry "tracks": "one" / "three" (else "none").  Both ways of a row run with the same rows, so the bit-for-bit check holds there too.

    python tools/stage_bench.py --device-noise   # host wall clock of a session's begin: host draw + upload  vs  the noise generated on the device

--device-noise (no --stage): BatchedRollouts.begin of an LMPC session at B = 1024, T_max = 400 on the golden N = 12 stores, timed three ways in one run, alternating:
the host draw (numpy standard_normal, no prefetcher) plus the upload -- unchanged code, so it stands for the library before the device generator --, the upload alone
(the array drawn beforehand: what a prefetcher that hides the draw completely leaves), and device_noise=True (one fill launch, nothing drawn or copied).  begin returns
with the stream drained, so the wall clock covers the fill kernel.  Medians and all samples go to profiles/device_noise_begin.json (or --out).  A record, not a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

X0 = np.array([0.5, 0, 0, 0, 0, 0.0])


def pid_u(x, vt, nu):
    return np.stack([-0.6 * x[:, 5] - 0.9 * x[:, 3] + np.clip(nu[:, 0] * 0.25, -0.9, 0.9), 1.5 * (vt - x[:, 0]) + np.clip(nu[:, 1] * 0.10, -0.2, 0.2)], axis=1)


def track_rows_for(B, tracks):
    """Rows for Context.track_set: "one" -- the L track for every car; "three" -- car b on track b mod 3 of (L, oval, goggle); "none" -- no rows."""
    from racinglmpc_amd import _capi, track
    if tracks == "none":
        return None
    names = ("L",) if tracks == "one" else tuple("L oval goggle".split()[b % 3] for b in range(B))
    tabs = {n: track.table_from_spec(track.REFERENCE_SPECS[n]) for n in set(names)}
    return _capi.track_rows([tabs[n] for n in names])


def run_stage(stage, g, B, T, plant_params=False, tracks="none"):
    from racinglmpc_amd import _capi, rollout
    N = 12
    ctx = _capi.Context(rollout.mpc_stage_config(g["track"], N, 0.8, B, trToUse=1))
    ctx.track_set(track_rows_for(B, tracks))
    if plant_params:
        ctx.plant_set_params(_capi.plant_params_default()[None] * np.random.default_rng(7).uniform(0.9, 1.1, (B, _capi.PLANT_NPAR)))
    rng = np.random.default_rng(7)
    noise = rng.standard_normal((T, B, 3)); nu = rng.standard_normal((T, B, 2))
    x0 = np.tile(X0, (B, 1)); x0[:, 5] = np.linspace(-0.1, 0.1, B) if B > 1 else 0.0
    vt = 0.6 + 0.02 * (np.arange(B) % 30)
    if stage == "mpc":
        A1, B1, _, _ = _capi.lti_regression(g["xPID"], g["uPID"], 1e-7)
        A = np.tile(A1[None], (B, 1, 1)); Bm = np.tile(B1[None], (B, 1, 1))
        At = np.tile(A[:, None], (1, N, 1, 1)); Bt = np.tile(Bm[:, None], (1, N, 1, 1)); Ct = np.zeros((B, N, 6))
    if stage == "ltvmpc":
        ctx.model_add_trajectory(g["xPID"], g["uPID"])
        xl0 = np.tile(np.array(g["xPID"])[None, 0:N + 1], (B, 1, 1)); ul0 = np.tile(np.array(g["uPID"])[None, 0:N], (B, 1, 1))

    def device():
        if stage == "pid":
            t, _ = ctx.rollout_pid(x0, x0, vt, nu, noise)
        else:
            if stage == "mpc":
                ctx.rollout_begin_mpc(x0, x0, noise, A=A, B=Bm)
            else:
                ctx.rollout_begin_mpc(x0, x0, noise, xLin0=xl0, uLin0=ul0)
            t, _ = ctx.rollout_run(T)
        X, U, G = ctx.rollout_fetch(0, t)[:3]
        ctx.rollout_end()
        return X, U, G

    def host():
        x = x0.copy(); xg = x0.copy(); uOld = np.zeros((B, 2)); X, U, G = [], [], []
        if stage == "ltvmpc":
            xLin, uLin = xl0, ul0
        for t in range(T):
            if stage == "pid":
                u = pid_u(x, vt, nu[t])
            elif stage == "mpc":
                u = ctx.qp_solve_batch(At, Bt, Ct, x, uOld)["uPred"][:, 0].copy()
            else:
                o = ctx.step_batch(x, xLin, uLin, uOld)
                u = o["uPred"][:, 0].copy()
                xLin = np.concatenate([o["xPred"][:, 1:], o["xPred"][:, N:N + 1]], axis=1); uLin = np.concatenate([o["uPred"][:, 1:], o["uPred"][:, N - 1:N]], axis=1)
            X.append(x); U.append(u); G.append(xg)
            x, xg, _ = ctx.plant_step_batch(x, xg, u, noise[t])
            uOld = u
        return np.stack(X), np.stack(U), np.stack(G)
    return ctx, device, host


def device_noise_begin(g, B=1024, T=400, repeats=7):
    """Seconds of BatchedRollouts.begin (host wall clock, stream drained when it returns) with the noise drawn on the host and uploaded, uploaded only, and generated on
    the device."""
    from racinglmpc_amd import rollout
    from tests import common
    ctx, _ = common.make_lmpc_ctx(g, 4, max_batch=B)
    track = np.array(g["track"])
    x0 = np.zeros((B, 6)); x0[:, 0] = np.linspace(0.5, 0.9, B); x0[:, 5] = np.linspace(-0.1, 0.1, B)[::-1]
    xl = np.tile(g["SS0"][1:14][None], (B, 1, 1)); ul = np.tile(g["uSS0"][1:13][None], (B, 1, 1))
    host = rollout.BatchedRollouts(ctx, track, seed=7, prefetch=False)
    dev = rollout.BatchedRollouts(ctx, track, seed=7, device_noise=True)
    drawn = np.random.default_rng(7).standard_normal((T, B, 3))

    def timed(f):
        t0 = time.perf_counter(); f(); dt = time.perf_counter() - t0
        ctx.rollout_end()
        return dt
    ways = dict(host_draw_and_upload=lambda: host.begin(x0, xl, ul, max_steps=T), upload_only=lambda: ctx.rollout_begin(x0, x0, xl, ul, drawn),
                device_noise=lambda: dev.begin(x0, xl, ul, max_steps=T))
    for f in ways.values():                                            # untimed: session buffers, code objects
        timed(f)
    samples = {k: [] for k in ways}
    for _ in range(repeats):
        for k, f in ways.items():
            if k != "device_noise":
                ctx.rollout_set_noise(False)
            samples[k].append(timed(f))
    ctx.close()
    return dict(tool="stage_bench", mode="device_noise_begin", N=12, B=B, T_max=T, noise_bytes=int(drawn.nbytes), unit="seconds of host wall clock per BatchedRollouts.begin",
                median_s={k: float(np.median(v)) for k, v in samples.items()}, samples_s=samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", choices=("pid", "mpc", "ltvmpc"))
    ap.add_argument("--device-noise", action="store_true", help="time a session's begin with host-drawn and with device-generated noise (B = 1024, T_max = 400); no --stage")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256, 1024])
    ap.add_argument("--steps", type=int, default=0, help="simulated steps per lap (default: 400 for pid, 100 for the MPC stages)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plant-params", action="store_true", help="also measure every batch size with per-car vehicle constants (+-10 % around the reference's, seed 7)")
    ap.add_argument("--tracks", action="store_true", help="also measure every batch size with one track row (the L track's) and with the cars over the three reference tracks")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not args.device_noise and not args.stage:
        ap.error("--stage is required (or --device-noise)")
    import __graft_entry__ as ge
    ge.build()
    from tests import common
    g = common.load_lmpc_golden()
    if args.device_noise:
        line = device_noise_begin(g, repeats=max(args.repeats, 7))
        print(json.dumps(line))
        with open(args.out or os.path.join(ROOT, "profiles", "device_noise_begin.json"), "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")
        return
    T = args.steps or (400 if args.stage == "pid" else 100)
    rows = []
    for B, par, trk in [(B, par, trk) for B in args.batches for par in ([False, True] if args.plant_params else [False]) for trk in (("none", "one", "three") if args.tracks else ("none",))]:
        ctx, device, host = run_stage(args.stage, g, B, T, plant_params=par, tracks=trk)
        d, h = device(), host()                                        # untimed: code objects, session buffers, pooled scratch
        same = all(np.array_equal(a, b) for a, b in zip(d, h))
        td, th = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter(); device(); td.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); host(); th.append(time.perf_counter() - t0)
        ctx.close()
        sd, sh = float(np.median(td)), float(np.median(th))
        rows.append(dict(B=B, steps=T, plant_params=par, tracks=trk, device_s=sd, host_stepped_s=sh, device_steps_per_s=B * T / sd, host_stepped_steps_per_s=B * T / sh,
                         device_s_all=td, host_stepped_s_all=th, logs_bit_identical=bool(same)))
    line = dict(tool="stage_bench", stage=args.stage, N=12, unit="car-steps per second of wall time" + ("" if args.stage == "pid" else " = closed-loop QP solves per second"),
                results=rows)
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
