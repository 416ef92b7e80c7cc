"""Free-running sessions (Context.rollout_relaunch, rollout.FreeRunningLMPC) measured on the GPU; writes profiles/free_running.json.

    python tools/free_run_bench.py --parent DIR [--repeats 5] [--out profiles/free_running.json]      both measurements
    python tools/free_run_bench.py --skip-ab                                                            (b) only: no parent build at hand
    python tools/free_run_bench.py --parent DIR --ab-only                                               (a) only

(a) Nothing lost when unused.  DIR is a built checkout of the parent commit.  Parent and this build alternate, `repeats` times each, every run a process of its own:
    `bench.py --gpus 1 --full --rollouts-only --no-cpu-baseline` (headline and rollout leg) and one PerCarLMPC(device_commit=True).run() at B = 256 and B = 1024, run
    with the tree's own Python package (tools/park_bench.py: leg `off`).  Rule: this build's median inside the parent's own min .. max.
(b) G = 5 laps per car at B = 256 and B = 1024 on a uniform batch, a three-track batch (track.REFERENCE_SPECS) and a batch with a spread of tuning rows (dR from half
    to twice the config's, lane bound 0.3 .. 0.5): FreeRunningLMPC.run(laps=5) against five PerCarLMPC(device_commit=True).run() generations on fresh contexts seeded
    with the same per-car PID laps, alternating, `repeats` times after one discarded warm-up.  Per case: wall time of both, session steps, laps stored per second, the
    step counts that bound the gain -- sum_g max_b T(b, g), what lockstep must take, against max_b sum_g T(b, g), what one session must take, plus the poll slack of at
    most 7 steps per lap -- and the stops the driver made, those at which it read the session, and the time spent in them.  No threshold: the figures are the result.
Host clock, every region ending in a device synchronise; median with min .. max.  Needs a GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from park_bench import spread                                                 # noqa: E402

G_LAPS, T_LAP, EXT = 5, 400, 40


def seeds_for(ctx, g, B, seed, tracks=None):
    """A rollouts object on `ctx` and per-car PID laps that end at the line (tools/park_bench.py seeds its loops the same way)."""
    from racinglmpc_amd import rollout
    kw = {} if tracks is None else dict(tracks=tracks)
    ro = rollout.BatchedRollouts(ctx, g["track"], seed=seed, device_noise=True, **kw)
    pid = ro.run_pid_laps(0.75 + 0.1 * np.arange(B) / B, max_steps=1000, stop_at_line=True, keep_invalid=True)
    bad = [b for b, l in enumerate(pid) if l[4] < 0 or l[5] != 0]
    if bad:
        raise SystemExit("PID lap of car(s) %s did not finish or was flagged: no seed lap" % bad[:8])
    return ro, pid


def one_run(g, N, B, seed, free, tuning=None, tracks=None):
    """G_LAPS laps per car on a fresh context, free-running or lockstep: (ms, lap_times, retired, session steps, stops)."""
    from racinglmpc_amd import _capi, rollout
    from tests import common
    cfg, _ = common.lmpc_config(g, N, max_batch=B, max_laps=(G_LAPS + 1) * B + 16, max_lap_len=1024)
    with _capi.Context(cfg) as ctx:
        ro, pid = seeds_for(ctx, g, B, seed, tracks)
        if free:
            loop = rollout.FreeRunningLMPC(ro, T_lap=T_LAP, ext=EXT, tuning=tuning)
        else:
            loop = rollout.PerCarLMPC(ro, T_max=T_LAP, ext=EXT, device_commit=True, tuning=tuning)
        loop.seed(pid)
        ctx.sync()
        t0 = time.perf_counter()
        if free:
            loop.run(laps=G_LAPS)
        else:
            for _ in range(G_LAPS):
                loop.run()
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        loop.close()
        return ms, [list(t) for t in loop.lap_times], {int(b): list(v) for b, v in loop.retired.items()}, [int(s) for s in loop.steps], [list(s) for s in getattr(loop, "stops", [])]


def leg(args):
    """One PerCarLMPC(device_commit=True).run() at B = 256 and 1024 on whatever tree sys.path names: one JSON line (the parent has no FreeRunningLMPC; this leg uses none)."""
    from park_bench import one_generation
    from tests import common
    g = common.load_lmpc_golden()
    out = {}
    for B in (256, 1024):
        one_generation(g, args.horizon, B, args.seed, False)                  # warm-up, discarded
        ms, laps, steps, done, retired = one_generation(g, args.horizon, B, args.seed, False)
        out[str(B)] = dict(run_ms=ms, lap_steps_sum=int(sum(t[0] for t in laps if t)), retired=len(retired))
    print(json.dumps(out))


def measure_ab(args):
    trees = [("parent", os.path.abspath(args.parent)), ("this", ROOT)]
    bench = ["bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20", "--full", "--rollouts-only", "--no-cpu-baseline"]
    runs = {name: dict(headline_solves_per_s=[], rollout_two_generations_s=[], per_car_run_ms_B256=[], per_car_run_ms_B1024=[]) for name, _ in trees}
    same = set()
    for rep in range(args.repeats):
        for name, tree in (trees if rep % 2 == 0 else trees[::-1]):
            last = lambda cmd: [l for l in subprocess.run([sys.executable] + cmd, cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout.splitlines() if l.startswith("{")][-1]
            b = json.loads(last(bench))
            runs[name]["headline_solves_per_s"].append(b["value"])
            runs[name]["rollout_two_generations_s"].append(sum(x["seconds"] for x in b["config_rollouts"]["generations"]))
            o = json.loads(last([os.path.abspath(__file__), "--leg", "--tree", tree, "--horizon", str(args.horizon), "--seed", str(args.seed)]))
            runs[name]["per_car_run_ms_B256"].append(o["256"]["run_ms"]); runs[name]["per_car_run_ms_B1024"].append(o["1024"]["run_ms"])
            same.add((tuple(tuple(x["best_lap_steps"]) for x in b["config_rollouts"]["generations"]), o["256"]["lap_steps_sum"], o["1024"]["lap_steps_sum"]))
            print("a/b run %d, %s: %s" % (rep, name, {k: round(v[-1], 4) for k, v in runs[name].items()}), file=sys.stderr, flush=True)
    figures = {}
    for k in runs["this"]:
        p, t = runs["parent"][k], runs["this"][k]
        figures[k] = dict(parent_runs=p, this_runs=t, parent_median=float(np.median(p)), parent_range=[min(p), max(p)], this_median=float(np.median(t)), this_range=[min(t), max(t)],
                          this_median_inside_parent_range=bool(min(p) <= np.median(t) <= max(p)))
    return dict(what="parent's build and this one alternating, %d runs each, every run a process of its own; no session relaunches" % args.repeats,
                rule="this build's median inside the parent's own min .. max", same_lap_steps_in_all_runs=len(same) == 1, figures=figures,
                all_inside=all(f["this_median_inside_parent_range"] for f in figures.values()))


def measure_free(args, g):
    from racinglmpc_amd import _capi, track
    from tests import common
    N = args.horizon
    names = ["L", "oval", "goggle"]
    out = []
    for B in args.batches:
        for kind in ("uniform", "three_tracks", "tuning_spread"):
            kw = {}
            if kind == "three_tracks":
                tabs = {n: track.table_from_spec(track.REFERENCE_SPECS[n]) for n in names}
                kw["tracks"] = [tabs[names[b % 3]] for b in range(B)]
            if kind == "tuning_spread":
                cfg, _ = common.lmpc_config(g, N, max_batch=B)
                kw["tuning"] = _capi.tuning_rows(cfg, B, dR=np.array(list(cfg.dR))[None, :] * np.linspace(0.5, 2.0, B)[:, None], bx=np.linspace(0.3, 0.5, B)[:, None] * np.ones((1, 2)))
            ms = {False: [], True: []}; info = {}
            for rep in range(args.repeats + 1):                               # (repeat 0: warm-up, discarded)
                for free in ((False, True) if rep % 2 == 0 else (True, False)):
                    got = one_run(g, N, B, args.seed, free, **kw)
                    if rep > 0:
                        ms[free].append(got[0])
                    info[free] = got
            lock, free = info[False], info[True]
            T = [t for t in lock[1]]
            laps_stored = sum(len(t) for t in free[1])
            sum_of_max = sum(max((t[k] for t in T if len(t) > k), default=0) for k in range(G_LAPS))
            max_of_sum = max(sum(t) for t in free[1])
            rec = dict(case="%s_B%d" % (kind, B), B=B, laps_per_car=G_LAPS, same_lap_times=lock[1] == free[1], same_retired=lock[2] == free[2], retired=len(free[2]),
                       laps_stored=laps_stored, lockstep_session_steps=lock[3], lockstep_steps_total=int(sum(lock[3])), free_running_session_steps=free[3][0],
                       bound_sum_of_max=int(sum_of_max), bound_max_of_sum=int(max_of_sum), poll_slack_at_most=7 * G_LAPS,
                       stops=free[4][0][0], stops_read=free[4][0][1], stops_ms=round(free[4][0][2] * 1e3, 3),
                       lockstep_ms=spread(ms[False]), free_running_ms=spread(ms[True]))
            rec["lockstep_laps_per_s"] = round(sum(len(t) for t in lock[1]) / (rec["lockstep_ms"]["median"] * 1e-3), 1)
            rec["free_running_laps_per_s"] = round(laps_stored / (rec["free_running_ms"]["median"] * 1e-3), 1)
            rec["time_ratio_free_over_lockstep"] = round(rec["free_running_ms"]["median"] / rec["lockstep_ms"]["median"], 4)
            rec["step_ratio_free_over_lockstep"] = round(rec["free_running_session_steps"] / max(1, rec["lockstep_steps_total"]), 4)
            out.append(rec)
            print("%-22s steps %4d -> %4d (bounds %d / %d), %.1f -> %.1f ms (ratio %.3f), %d stops, %d read, %.1f ms in them" % (rec["case"], rec["lockstep_steps_total"],
                  rec["free_running_session_steps"], sum_of_max, max_of_sum, rec["lockstep_ms"]["median"], rec["free_running_ms"]["median"], rec["time_ratio_free_over_lockstep"],
                  rec["stops"], rec["stops_read"], rec["stops_ms"]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit, for (a)")
    ap.add_argument("--skip-ab", action="store_true")
    ap.add_argument("--ab-only", action="store_true", help="(a) alone")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--leg", action="store_true", help="(internal) the per-car leg of (a), run on --tree")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "free_running.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if args.leg:
        return leg(args)
    if args.repeats < 5:
        raise SystemExit("at least five repeats")
    if not args.skip_ab and not args.parent:
        raise SystemExit("--parent DIR (a built checkout of the parent commit) or --skip-ab")
    import __graft_entry__ as ge
    ge.build()
    from racinglmpc_amd import _capi
    from tests import common
    try:
        _capi.device_memory(0)
    except _capi.LmpcError as e:
        raise SystemExit("free_run_bench needs a GPU: %s" % e)
    g = common.load_lmpc_golden()
    result = dict(horizon=args.horizon, repeats=args.repeats, laps_per_car=G_LAPS, T_lap=T_LAP, ext=EXT)
    if os.path.exists(args.out):                                              # (a run with --skip-ab keeps the A / B of an earlier one)
        with open(args.out) as f:
            result = dict(json.load(f), **result)
    if not args.ab_only:
        result["b_free_running_against_lockstep"] = measure_free(args, g)
    if not args.skip_ab:
        result["a_unused_against_parent"] = measure_ab(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
