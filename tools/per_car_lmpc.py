"""Independent learners in one batch: B cars on a grid of tyre-grip (mu) x mass (m) scalings of the reference's vehicle (rows of vehicle constants spread over the
cars as tools/mismatch_sweep.py spreads them), each seeded with its OWN PID lap, run for G generations of rollout.PerCarLMPC -- main.py:100-121 once per car.

    python tools/per_car_lmpc.py [--mu 0.8 1.0] [--m 0.9 1.0 1.1] [--cars-per-cell 2] [--generations 4] [--seed 3] [--device-commit] [--prune] [--free-running [--laps 4]]

Two runs from the same seed laps, same vehicles, same noise (device generator, same seed and car indices):
  "own":    every car selects its terminal set from its own laps (Context.ss_set_lap_table, last[b] = its own latest lap) -- rollout.PerCarLMPC as it is;
  "shared": the same loop with the safe-set table switched off -- the library's shared rule picks the numSS_it fastest laps of ALL cars for everybody, and the
            "current lap" is the last lap stored, whoever drove it.  The regression keeps its per-car table in both runs, so the safe set is the only difference.
Per car and generation: lap time in steps (None from the generation in which the car was retired) and, for a retired car, (generation, status bits).
Writes profiles/per_car_lmpc.json (or --out) and prints it as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mu", type=float, nargs="+", default=[0.8, 1.0], help="scalings of the reference's friction coefficient 0.8, front and rear")
    ap.add_argument("--m", type=float, nargs="+", default=[0.9, 1.0, 1.1], help="scalings of the reference's mass 1.98")
    ap.add_argument("--cars-per-cell", type=int, default=2)
    ap.add_argument("--generations", type=int, default=4)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--device-commit", action="store_true", help="laps are committed to the stores on the device (PerCarLMPC(device_commit=True)): same lap times, no log download")
    ap.add_argument("--park", action="store_true", help="parking (PerCarLMPC(park=True)): retired cars are not stepped, finished cars leave the launches, a generation ends when no car is live; same lap times")
    ap.add_argument("--metrics", action="store_true", help="lap metrics reduced on the device (PerCarLMPC(metrics=True)): t_cross, ey_absmax, lane_excess_max, input_margin_min, alat_absmax and the realised stage cost under the config's dR and Qslack, per car and generation")
    ap.add_argument("--prune", action="store_true", help="the \"own\" run gives back the laps no car reads any more after every generation (PerCarLMPC(prune=True)): same lap times, stores bounded by B (numSS_it + 1) and B trToUse laps; the \"shared\" run selects among ALL cars' laps and is never pruned")
    ap.add_argument("--free-running", action="store_true", help="the \"own\" run is ONE session of rollout.FreeRunningLMPC in which every car starts its next lap at its own crossing (--laps per car): same lap times as --device-commit, fewer session steps; not with --park or --metrics")
    ap.add_argument("--laps", type=int, default=None, help="laps per car of the --free-running session (default: --generations)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_car_lmpc.json"))
    args = ap.parse_args()
    if args.free_running and (args.park or args.metrics):
        raise SystemExit("--free-running: a session that changes laps takes neither --park nor --metrics")
    if args.laps is not None and not args.free_running:
        raise SystemExit("--laps goes with --free-running")
    import __graft_entry__ as ge
    ge.build()
    from racinglmpc_amd import _capi, rollout
    from tests import common
    g = common.load_lmpc_golden()
    N, G = args.horizon, args.generations
    grid = [(mu, m) for mu in args.mu for m in args.m]
    cells = np.repeat(np.arange(len(grid)), args.cars_per_cell)
    B = len(cells)
    mu = np.array([grid[c][0] for c in cells]); ms = np.array([grid[c][1] for c in cells])
    rows = _capi.plant_params(B, m=1.98 * ms, mu_f=0.8 * mu, mu_r=0.8 * mu)

    class SharedSafeSet(rollout.PerCarLMPC):
        """The same loop without the safe-set table: the shared selection of the library."""
        def _hand_tables(self):
            super()._hand_tables()
            self.ro.ss_table = self.ro.ss_last = None
            self.ro.ctx.ss_set_lap_table(None)

    result = dict(horizon=N, generations=G, seed=args.seed, device_commit=bool(args.device_commit), park=bool(args.park), prune=bool(args.prune), cars=[dict(car=b, mu_scale=float(mu[b]), m_scale=float(ms[b])) for b in range(B)])
    seeds = None
    for name, cls in (("own", rollout.PerCarLMPC), ("shared", SharedSafeSet)):
        cfg, _ = common.lmpc_config(g, N, max_batch=B, max_laps=max(16, B * (G + 1)), max_lap_len=1024)
        with _capi.Context(cfg) as ctx:
            ro = rollout.BatchedRollouts(ctx, g["track"], seed=args.seed, plant_params=rows, device_noise=True)
            pid = ro.run_pid_laps(np.full(B, 0.8), max_steps=1000, keep_invalid=True)           # (main.py:61-70, every car on its own vehicle)
            if seeds is None:
                seeds = [int(l[4]) for l in pid]
            free = args.free_running and name == "own"
            if free:
                loop = rollout.FreeRunningLMPC(ro, T_lap=400, ext=40, prune=args.prune)
            else:
                loop = cls(ro, T_max=400, ext=40, device_commit=args.device_commit, park=args.park, metrics=args.metrics, prune=args.prune and name == "own")
            bad = [b for b, l in enumerate(pid) if l[4] < 0 or (l[5] & ~_capi.ST_INEXACT) != 0 or not np.all(np.isfinite(l[0]))]
            if bad:
                raise SystemExit("PID lap of car(s) %s did not finish or was flagged: no seed lap" % bad)
            loop.seed(pid)
            if free:
                loop.run(laps=G if args.laps is None else args.laps)
                result["free_running"] = dict(laps=G if args.laps is None else args.laps, stops=[list(s) for s in loop.stops])
            else:
                for _ in range(G):
                    loop.run()
            stored = (ctx.ss_num_laps(), ctx.model_num_laps())
            loop.close()
            result[name] = dict(stored_laps=list(stored), session_steps=list(loop.steps), lap_steps=[t + [None] * (G - len(t)) for t in loop.lap_times], retired={str(b): list(v) for b, v in sorted(loop.retired.items())})
            if args.metrics:
                result[name]["metrics"] = _capi.metrics_report(loop.metrics, list(cfg.dR), list(cfg.Qslack))
    result["pid_lap_steps"] = seeds
    print("%-4s %-8s %-8s %-6s | %-28s | %-28s" % ("car", "mu", "m", "PID", "own safe set", "shared safe set"))
    for b in range(B):
        print("%-4d %-8.2f %-8.2f %-6d | %-28s | %-28s" % (b, mu[b], ms[b], seeds[b], result["own"]["lap_steps"][b], result["shared"]["lap_steps"][b]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
