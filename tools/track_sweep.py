"""Several tracks in one batch: B cars dealt round-robin over the reference's three track specs (racinglmpc_amd.track.REFERENCE_SPECS: the L-shaped track it runs, and
the oval and the goggle track it carries in comments; Context.track_set: each car's track table and length from its own row).  rollout.bootstrap(tracks=) runs
main.py:61-95 per car -- PID lap, LTI-MPC lap, LTV-MPC lap, car b on its own track with its own regression lap -- and rollout.PerCarLMPC(device_commit=True), seeded
with every car's PID lap, runs G generations of main.py:100-121 per car: one context, one set of lap stores, one launch sequence for all tracks.

    python tools/track_sweep.py [--cars 12] [--generations 3] [--seed 3] [--vt 0.8]

Per track and generation: the lap times in steps of its cars (None from the generation in which a car was retired); per stage of the bootstrap the crossing steps.
The numbers are reported, not asserted.  Writes profiles/per_car_tracks.json (or --out; an existing file keeps its other keys) under the key "track_sweep" and
prints the result as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cars", type=int, default=12)
    ap.add_argument("--generations", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--vt", type=float, default=0.8, help="target speed of the PID and MPC stages (main.py:50)")
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--park", action="store_true", help="parking (PerCarLMPC(park=True)): retired cars are not stepped, finished cars leave the launches, a generation ends when no car is live; same lap times")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_car_tracks.json"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from racinglmpc_amd import _capi, rollout, track
    from tests import common
    g = common.load_lmpc_golden()
    B, N, G = args.cars, args.horizon, args.generations
    order = ("L", "oval", "goggle")
    names = [order[b % 3] for b in range(B)]
    tabs = {n: track.table_from_spec(track.REFERENCE_SPECS[n]) for n in order}
    tables = [tabs[n] for n in names]
    result = dict(horizon=N, generations=G, seed=args.seed, vt=args.vt, cars=[dict(car=b, track=names[b], trackLength=tabs[names[b]][1]) for b in range(B)])
    boot = rollout.bootstrap(np.array(g["track"]), B, N, args.vt, seed=args.seed, max_steps=1000, device_noise=True, per_car_store=True, tracks=tables)
    result["bootstrap"] = {stage: dict(crossing_steps=[int(l[4]) for l in boot[stage]], status=[int(l[5]) for l in boot[stage]]) for stage in ("pid", "mpc", "ltvmpc")}
    bad = [b for b, l in enumerate(boot["pid"]) if l[4] < 0 or (l[5] & ~_capi.ST_INEXACT) != 0 or not np.all(np.isfinite(l[0]))]
    if bad:
        raise SystemExit("PID lap of car(s) %s did not finish or was flagged: no seed lap" % bad)
    cfg, _ = common.lmpc_config(g, N, max_batch=B, max_laps=max(16, B * (G + 1)), max_lap_len=1024)
    with _capi.Context(cfg) as ctx:
        ro = rollout.BatchedRollouts(ctx, g["track"], seed=args.seed, device_noise=True, tracks=tables)
        loop = rollout.PerCarLMPC(ro, T_max=400, ext=40, device_commit=True, park=args.park)
        loop.seed(boot["pid"])
        status = []
        for _ in range(G):
            loop.run()
            status.append([int(s) for s in np.asarray(loop.last_status).reshape(-1)] if loop.last_status is not None else None)
        assert np.array_equal(ctx.tracks(), ro.tracks)
        loop.close()
    result["lap_steps"] = [t + [None] * (G - len(t)) for t in loop.lap_times]
    result["status_per_generation"] = status
    result["park"] = bool(args.park); result["session_steps"] = list(loop.steps)
    result["retired"] = {str(b): list(v) for b, v in sorted(loop.retired.items())}
    result["per_track"] = {n: dict(pid=[result["bootstrap"]["pid"]["crossing_steps"][b] for b in range(B) if names[b] == n],
                                   ltvmpc=[result["bootstrap"]["ltvmpc"]["crossing_steps"][b] for b in range(B) if names[b] == n],
                                   lmpc_generations=[[result["lap_steps"][b][k] for b in range(B) if names[b] == n] for k in range(G)]) for n in order}
    print("%-7s %-10s | %-22s | %s" % ("track", "length", "PID / LTV-MPC steps", "LMPC lap steps per generation"))
    for n in order:
        r = result["per_track"][n]
        print("%-7s %-10.4f | %-22s | %s" % (n, tabs[n][1], "%s / %s" % (r["pid"], r["ltvmpc"]), r["lmpc_generations"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["track_sweep"] = result
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
