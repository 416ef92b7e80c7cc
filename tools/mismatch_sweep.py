"""Model mismatch in one batch: B cars on a grid of tyre-grip (mu) x mass (m) scalings of the reference's vehicle, every car with its own row of vehicle constants
(Context.plant_set_params), the controllers unchanged.

    python tools/mismatch_sweep.py [--mu 0.6 0.8 1.0 1.2] [--m 0.8 1.0 1.2] [--cars-per-cell 16] [--seed 3] [--own-model]

Two laps per car, both device-resident: one PID lap (lmpc_rollout_pid, vt = 0.8, 1000 steps as main.py:57) and one LMPC lap (lmpc_rollout_begin / _run, 400 steps) from a
safe set seeded with the four nominal PID laps of rollout.bootstrap -- the safe set and the regression store are those of the NOMINAL vehicle, so the LMPC lap shows
what a learned safe set is worth on another car.  Per grid cell: cars that finished, cars flagged (any status bit but INEXACT), lap time (steps to the line) of the
finished ones.  --own-model adds a second LMPC lap beside it ("lmpc_own_model"): the same nominal safe set, but every car's regression rows are its OWN PID lap
(Context.model_set_lap_table: the lap repeated trToUse times, as main.py:103-104 repeats its one lap), i.e. the LTV model is identified on the car that drives -- the
reference's own flow, main.py:88-89.  A car whose PID lap was flagged or holds a non-finite row keeps the nominal rows and is counted in "own_model_fallback".  Writes profiles/mismatch_sweep.json (or --out) and prints it as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cell_stats(laps, cells, ncell):
    from racinglmpc_amd import _capi
    out = []
    for c in range(ncell):
        mine = [l for l, k in zip(laps, cells) if k == c]
        fin = [l[4] for l in mine if l[4] >= 0 and (l[5] & ~_capi.ST_INEXACT) == 0]
        out.append(dict(cars=len(mine), finished=len(fin), flagged=sum(1 for l in mine if (l[5] & ~_capi.ST_INEXACT) != 0),
                        lap_steps_min=int(min(fin)) if fin else None, lap_steps_median=float(np.median(fin)) if fin else None, lap_steps_max=int(max(fin)) if fin else None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mu", type=float, nargs="+", default=[0.6, 0.8, 1.0, 1.2], help="scalings of the reference's friction coefficient 0.8, front and rear")
    ap.add_argument("--m", type=float, nargs="+", default=[0.8, 1.0, 1.2], help="scalings of the reference's mass 1.98")
    ap.add_argument("--cars-per-cell", type=int, default=16)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--own-model", action="store_true", help="also the LMPC lap with each car's regression laps taken from its own PID lap (nominal safe set)")
    ap.add_argument("--park", action="store_true", help="parking (BatchedRollouts(park=True)): a car that has crossed the line leaves the launches of the LMPC lap; same laps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mismatch_sweep.json"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from racinglmpc_amd import _capi, rollout
    from tests import common
    g = common.load_lmpc_golden()
    N = args.horizon
    grid = [(mu, m) for mu in args.mu for m in args.m]
    cells = np.repeat(np.arange(len(grid)), args.cars_per_cell)
    B = len(cells)
    mu = np.array([grid[c][0] for c in cells]); ms = np.array([grid[c][1] for c in cells])
    rows = _capi.plant_params(B, m=1.98 * ms, mu_f=0.8 * mu, mu_r=0.8 * mu)
    # the seed laps: the nominal vehicle, as main.py:61-110
    seeds = rollout.bootstrap(g["track"], 4, N, 0.8, args.seed)
    seed_laps = [seeds["pid"][b] for b in seeds["store_laps"]]
    # PID laps of the grid (any context serves: the PID stage needs the track only)
    ctx = _capi.Context(rollout.mpc_stage_config(g["track"], N, 0.8, B))
    ro = rollout.BatchedRollouts(ctx, g["track"], seed=args.seed + 1, plant_params=rows)
    pid = ro.run_pid_laps(np.full(B, 0.8), max_steps=1000, keep_invalid=True)
    ro.close(); ctx.close()
    # one LMPC lap of the grid from the nominal safe set
    cfg, _ = common.lmpc_config(g, N, max_batch=B)
    ctx = _capi.Context(cfg)
    rollout.seed_lmpc(ctx, seed_laps)
    ro = rollout.BatchedRollouts(ctx, g["track"], seed=args.seed + 2, plant_params=rows, park=True if args.park else None)
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1))
    lmpc = ro.run_lap_device(x0, seed_laps[0][0][1:N + 2], seed_laps[0][1][1:N + 1], max_steps=400, keep_invalid=True)
    ro.close(); ctx.close()
    own = None
    if args.own_model:
        ctx = _capi.Context(cfg)
        rollout.seed_lmpc(ctx, seed_laps)                              # regression laps 0 .. 3 (insertion indices) and the safe set: nominal
        L = cfg.trToUse
        assert L <= len(seed_laps)                                     # (the library's default choice: the first trToUse laps of the sorted order = the seed laps, equal in length)
        table = np.tile(np.arange(L, dtype=np.int32), (B, 1))
        fallback = 0
        for b in range(B):
            ok = (pid[b][5] & ~_capi.ST_INEXACT) == 0 and np.all(np.isfinite(pid[b][0])) and np.all(np.isfinite(pid[b][1]))
            ctx.model_add_trajectory(pid[b][0] if ok else seed_laps[0][0], pid[b][1] if ok else seed_laps[0][1])      # insertion index len(seed_laps) + b
            if ok:
                table[b] = len(seed_laps) + b
            else:
                fallback += 1
        ro = rollout.BatchedRollouts(ctx, g["track"], seed=args.seed + 2, plant_params=rows, lap_table=table, park=True if args.park else None)       # (the seed of the lap above: the same disturbance)
        own = ro.run_lap_device(x0, seed_laps[0][0][1:N + 2], seed_laps[0][1][1:N + 1], max_steps=400, keep_invalid=True)
        ro.close(); ctx.close()
    ps, ls = cell_stats(pid, cells, len(grid)), cell_stats(lmpc, cells, len(grid))
    line = dict(tool="mismatch_sweep", N=N, cars=B, cars_per_cell=args.cars_per_cell, seed=args.seed,
                note="mu, m: scalings of the reference's 0.8 and 1.98; safe set and regression store from four nominal PID laps; lap_steps: simulated steps (0.1 s) to the line",
                cells=[dict(mu_scale=grid[c][0], m_scale=grid[c][1], pid=ps[c], lmpc=ls[c]) for c in range(len(grid))])
    if own is not None:
        os_ = cell_stats(own, cells, len(grid))
        for c in range(len(grid)):
            line["cells"][c]["lmpc_own_model"] = os_[c]
        line["own_model_fallback"] = fallback
        line["note"] += "; lmpc_own_model: regression rows from each car's own PID lap (lap table), nominal safe set"
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
