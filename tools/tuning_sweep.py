"""Controller tuning sweep in one batch: one car per point of a grid Qslack[1] x dR[1] x QtermSlack scale (Context.tuning_set: each car's cost weights from its own
row), every car on the reference's vehicle and seeded with its own PID lap (car b has stream b of the device noise generator), run for G generations of
rollout.PerCarLMPC(device_commit=True) -- main.py:100-121 once per car, ten tunings in one launch instead of ten contexts.

    python tools/tuning_sweep.py [--qslack1 25 100] [--dr1 50 200] [--qterm 0.2 1.0] [--generations 3] [--seed 3]

Per car and generation: lap time in steps (None from the generation in which the car was retired) and the status word of the generation's session; for a retired
car, (generation, status bits).  The numbers are reported, not asserted.  Writes profiles/tuning_sweep.json (or --out) and prints it as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qslack1", type=float, nargs="+", default=[25.0, 100.0], help="linear lane-slack weight Qslack[1] (reference: 25)")
    ap.add_argument("--dr1", type=float, nargs="+", default=[50.0, 200.0], help="input-rate weight of the acceleration dR[1] (reference: 50)")
    ap.add_argument("--qterm", type=float, nargs="+", default=[0.2, 1.0], help="scalings of the reference's QterminalSlack = 500 I")
    ap.add_argument("--generations", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--park", action="store_true", help="parking (PerCarLMPC(park=True)): retired cars are not stepped, finished cars leave the launches, a generation ends when no car is live; same lap times")
    ap.add_argument("--metrics", action="store_true", help="lap metrics reduced on the device (PerCarLMPC(metrics=True)): t_cross, ey_absmax, lane_excess_max, input_margin_min, alat_absmax and the realised stage cost under each car's own dR and Qslack, per car and generation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuning_sweep.json"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from racinglmpc_amd import _capi, rollout
    from tests import common
    g = common.load_lmpc_golden()
    N, G = args.horizon, args.generations
    grid = [(a, b, c) for a in args.qslack1 for b in args.dr1 for c in args.qterm]
    B = len(grid)
    cfg, _ = common.lmpc_config(g, N, max_batch=B, max_laps=max(16, B * (G + 1)), max_lap_len=1024)
    base = _capi.tuning_rows(cfg, 1)[0]
    sl = _capi.TUNING_FIELDS
    rows = _capi.tuning_rows(cfg, B, Qslack=np.array([[base[sl["Qslack"]][0], a] for a, b, c in grid]), dR=np.array([[base[sl["dR"]][0], b] for a, b, c in grid]),
                             QtermSlack=np.array([c * base[sl["QtermSlack"]] for a, b, c in grid]))
    result = dict(horizon=N, generations=G, seed=args.seed, cars=[dict(car=i, Qslack1=a, dR1=b, QtermSlack_scale=c) for i, (a, b, c) in enumerate(grid)])
    with _capi.Context(cfg) as ctx:
        # (every car drives the reference's vehicle; the device generator gives car b its own disturbance stream of the one seed)
        ro = rollout.BatchedRollouts(ctx, g["track"], seed=args.seed, device_noise=True)
        pid = ro.run_pid_laps(np.full(B, 0.8), max_steps=1000, keep_invalid=True)               # (main.py:61-70)
        bad = [b for b, l in enumerate(pid) if l[4] < 0 or (l[5] & ~_capi.ST_INEXACT) != 0 or not np.all(np.isfinite(l[0]))]
        if bad:
            raise SystemExit("PID lap of car(s) %s did not finish or was flagged: no seed lap" % bad)
        loop = rollout.PerCarLMPC(ro, T_max=400, ext=40, device_commit=True, tuning=rows, park=args.park, metrics=args.metrics)
        loop.seed(pid)
        status = []
        for _ in range(G):
            loop.run()
            status.append([int(s) for s in np.asarray(loop.last_status).reshape(-1)] if loop.last_status is not None else None)
        assert np.array_equal(ctx.tuning(), rows)
        loop.close()
    result["pid_lap_steps"] = [int(l[4]) for l in pid]
    result["lap_steps"] = [t + [None] * (G - len(t)) for t in loop.lap_times]
    result["status_per_generation"] = status
    result["park"] = bool(args.park); result["session_steps"] = list(loop.steps)
    result["retired"] = {str(b): list(v) for b, v in sorted(loop.retired.items())}
    if args.metrics:
        result["metrics"] = _capi.metrics_report(loop.metrics, rows[:, sl["dR"]], rows[:, sl["Qslack"]])
    print("%-4s %-8s %-8s %-8s %-6s | %s" % ("car", "Qslack1", "dR1", "Qterm x", "PID", "LMPC lap steps"))
    for b, (a, d, c) in enumerate(grid):
        print("%-4d %-8g %-8g %-8g %-6d | %s" % (b, a, d, c, result["pid_lap_steps"][b], result["lap_steps"][b]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
