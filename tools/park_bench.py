"""Parking (Context.rollout_set_parking, rollout.PerCarLMPC(park=True)) measured on the GPU; writes profiles/parking.json.

    python tools/park_bench.py --parent DIR [--repeats 5] [--out profiles/parking.json]      all three measurements
    python tools/park_bench.py --skip-ab                                                       (b) and (c) only: no parent build at hand
    python tools/park_bench.py --parent DIR --ab-only --ab-parked --out profiles/NAME_ab.json  (a) only, with its parked leg: a change that claims to alter nothing

(a) No regression when off.  DIR is a built checkout of the parent commit.  Parent and this build alternate, `repeats` times each, every run a process of its own:
    `bench.py --gpus 1 --full --rollouts-only --no-cpu-baseline` (headline and rollout leg) and one un-parked PerCarLMPC.run() at B = 256 and B = 1024 (leg `off`
    below, run with the tree's own Python package).  Rule: this build's median inside the parent's own min .. max.
    --ab-parked (a parent that has parking): also one parked PerCarLMPC(device_commit=True, park=True) generation at B = 256 -- host-launch bound -- and B = 4096,
    where the live count moves most (leg `parked`); lap steps and retired cars must agree in every run of both builds.
(b) Parked against un-parked on this build: one generation of PerCarLMPC(device_commit=True) on fresh contexts seeded with the same per-car PID laps, alternating,
    `repeats` times after one discarded warm-up, at B = 256, 1024 and 4096, B = 4096 with PARK_REROUTE, a three-track batch (track.REFERENCE_SPECS) and a batch in
    which 5 % of the cars carry a tuning row that cannot finish.  Beside each time the work fraction sum_t nLive(t) / (B x un-parked steps), from doneAt and the poll
    rule (a car leaves at the first multiple of 8 at or after its crossing step): what the time can at best follow.
(c) The compaction launch: lmpc_debug_live_compact timed from the host at n = 256 .. 262144 -- an UPPER bound on a rebuild, since the debug entry also allocates,
    uploads three arrays and downloads three; and the poll it rides on: a session in which no car finishes within 64 steps, with PARK_FINISHED (the kernel is launched at
    every poll and returns at once) against the start list alone (no launch), per poll.
Host clock, every region ending in a device synchronise; median with min .. max.  Needs a GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), all=[round(float(x), 4) for x in v])


def seeded_loop(ctx, g, B, seed, park, device_commit=True, tuning=None, tracks=None, reroute=False):
    """A PerCarLMPC on `ctx`, seeded with per-car PID laps that end at the line (as tools/commit_bench.py seeds it)."""
    from racinglmpc_amd import _capi, rollout
    kw = {} if tracks is None else dict(tracks=tracks)
    ro = rollout.BatchedRollouts(ctx, g["track"], seed=seed, device_noise=True, **kw)
    pid = ro.run_pid_laps(0.75 + 0.1 * np.arange(B) / B, max_steps=1000, stop_at_line=True, keep_invalid=True)
    bad = [b for b, l in enumerate(pid) if l[4] < 0 or l[5] != 0]
    if bad:
        raise SystemExit("PID lap of car(s) %s did not finish or was flagged: no seed lap" % bad[:8])
    kw = dict(park=_capi.PARK_REROUTE if reroute else True) if park else {}       # (the parent's PerCarLMPC has no such argument)
    loop = rollout.PerCarLMPC(ro, T_max=400, ext=40, device_commit=device_commit, tuning=tuning, **kw)
    loop.seed(pid)
    return loop


def one_generation(g, N, B, seed, park, **kw):
    """(run ms, lap_times, session steps, doneAt, retired) of one generation on a fresh context."""
    from racinglmpc_amd import _capi
    from tests import common
    cfg, _ = common.lmpc_config(g, N, max_batch=B, max_laps=2 * B + 16, max_lap_len=1024)
    with _capi.Context(cfg) as ctx:
        loop = seeded_loop(ctx, g, B, seed, park, **kw)
        ctx.sync()
        t0 = time.perf_counter()
        loop.run()
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        loop.close()
        return ms, [list(t) for t in loop.lap_times], int(loop.steps[-1]) if hasattr(loop, "steps") else None, np.array(loop.last_done), sorted(loop.retired)


def work_fraction(done, steps_unparked):
    """sum_t nLive(t) / (B x steps): a car is stepped up to the first multiple of 8 at or after its crossing step, an unfinished one to the end."""
    done = np.asarray(done)
    stepped = np.where(done >= 0, np.minimum(-(-done // 8) * 8, steps_unparked), steps_unparked)
    return float(stepped.sum()) / float(done.size * steps_unparked)


def leg(args, park):
    """One un-parked (B = 256, 1024) or parked (B = 256, 4096) PerCarLMPC.run() per batch size, on whatever tree sys.path names: one JSON line."""
    from tests import common
    g = common.load_lmpc_golden()
    out = {}
    for B in ((256, 4096) if park else (256, 1024)):
        one_generation(g, args.horizon, B, args.seed, park)                     # warm-up, discarded
        ms, laps, steps, done, retired = one_generation(g, args.horizon, B, args.seed, park)
        out[str(B)] = dict(run_ms=ms, lap_steps_sum=int(sum(t[0] for t in laps if t)), retired=len(retired))
    print(json.dumps(out))


def measure_ab(args):
    trees = [("parent", os.path.abspath(args.parent)), ("this", ROOT)]
    bench = ["bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20", "--full", "--rollouts-only", "--no-cpu-baseline"]
    runs = {name: dict(headline_solves_per_s=[], rollout_two_generations_s=[], per_car_run_ms_B256=[], per_car_run_ms_B1024=[]) for name, _ in trees}
    if args.ab_parked:
        for name, _ in trees:
            runs[name].update(parked_run_ms_B256=[], parked_run_ms_B4096=[])
    same = {name: set() for name, _ in trees}
    for rep in range(args.repeats):
        for name, tree in (trees if rep % 2 == 0 else trees[::-1]):
            last = lambda cmd: [l for l in subprocess.run([sys.executable] + cmd, cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout.splitlines() if l.startswith("{")][-1]
            b = json.loads(last(bench))
            runs[name]["headline_solves_per_s"].append(b["value"])
            runs[name]["rollout_two_generations_s"].append(sum(x["seconds"] for x in b["config_rollouts"]["generations"]))
            o = json.loads(last([os.path.abspath(__file__), "--leg", "off", "--tree", tree, "--horizon", str(args.horizon), "--seed", str(args.seed)]))
            runs[name]["per_car_run_ms_B256"].append(o["256"]["run_ms"]); runs[name]["per_car_run_ms_B1024"].append(o["1024"]["run_ms"])
            same[name].add((tuple(tuple(x["best_lap_steps"]) for x in b["config_rollouts"]["generations"]), o["256"]["lap_steps_sum"], o["1024"]["lap_steps_sum"]))
            if args.ab_parked:
                k = json.loads(last([os.path.abspath(__file__), "--leg", "parked", "--tree", tree, "--horizon", str(args.horizon), "--seed", str(args.seed)]))
                runs[name]["parked_run_ms_B256"].append(k["256"]["run_ms"]); runs[name]["parked_run_ms_B4096"].append(k["4096"]["run_ms"])
                same[name].add(("parked",) + tuple(k[B][f] for B in ("256", "4096") for f in ("lap_steps_sum", "retired")))
            print("a/b run %d, %s: %s" % (rep, name, {k: round(v[-1], 4) for k, v in runs[name].items()}), file=sys.stderr, flush=True)
    figures = {}
    for k in runs["this"]:
        p, t = runs["parent"][k], runs["this"][k]
        figures[k] = dict(parent_runs=p, this_runs=t, parent_median=float(np.median(p)), parent_range=[min(p), max(p)], this_median=float(np.median(t)), this_range=[min(t), max(t)],
                          this_median_inside_parent_range=bool(min(p) <= np.median(t) <= max(p)))
    return dict(what="parent's build and this one alternating, %d runs each, every run a process of its own; parking off" % args.repeats,
                rule="this build's median inside the parent's own min .. max", same_lap_steps_in_all_runs=len(same["parent"] | same["this"]) == (2 if args.ab_parked else 1), figures=figures,
                all_inside=all(f["this_median_inside_parent_range"] for f in figures.values()))


def measure_parked(args, g):
    from racinglmpc_amd import _capi, track
    from tests import common
    N = args.horizon
    names = ["L", "oval", "goggle"]
    cases = [dict(name="B256", B=256), dict(name="B1024", B=1024), dict(name="B4096", B=4096), dict(name="B4096_reroute", B=4096, reroute=True),
             dict(name="three_tracks_B255", B=255, tracks=True), dict(name="five_percent_cannot_finish_B1024", B=1024, stuck=0.05)]
    out = []
    for case in cases:
        B = case["B"]; kw = {}
        if case.get("tracks"):
            tabs = {n: track.table_from_spec(track.REFERENCE_SPECS[n]) for n in names}
            kw["tracks"] = [tabs[names[b % 3]] for b in range(B)]
        if case.get("stuck"):
            cfg, _ = common.lmpc_config(g, N, max_batch=B)
            rows = _capi.tuning_rows(cfg, B); rows[::int(round(1 / case["stuck"])), -4:] = 0.0          # bu = 0: LMPC_ST_NOT_INTERIOR at every step, the car does not finish
            kw["tuning"] = rows
        if case.get("reroute"):
            kw["reroute"] = True
        ms = {False: [], True: []}; info = {}
        for rep in range(args.repeats + 1):                       # (repeat 0: warm-up, discarded)
            for park in ((False, True) if rep % 2 == 0 else (True, False)):
                got = one_generation(g, N, B, args.seed, park, **kw)
                if rep > 0:
                    ms[park].append(got[0])
                info[park] = got
        if info[False][1] != info[True][1] or info[False][4] != info[True][4]:
            raise SystemExit("%s: parked and un-parked disagree on lap times or retired cars" % case["name"])
        done = info[False][3]; laps = [int(d) for d in done if d >= 0]
        rec = dict(case=case["name"], B=B, steps_unparked=info[False][2], steps_parked=info[True][2], finished=len(laps), lap_steps_min=min(laps), lap_steps_max=max(laps),
                   work_fraction=round(work_fraction(done, info[False][2]), 4), unparked_run_ms=spread(ms[False]), parked_run_ms=spread(ms[True]))
        rec["time_ratio_parked_over_unparked"] = round(rec["parked_run_ms"]["median"] / rec["unparked_run_ms"]["median"], 4)
        out.append(rec)
        print("%-34s steps %3d -> %3d, work fraction %.3f, run() %.1f -> %.1f ms (ratio %.3f)" % (case["name"], rec["steps_unparked"], rec["steps_parked"], rec["work_fraction"],
              rec["unparked_run_ms"]["median"], rec["parked_run_ms"]["median"], rec["time_ratio_parked_over_unparked"]), file=sys.stderr)
    return out


def measure_compaction(args, g):
    from racinglmpc_amd import _capi
    from tests import common
    cfg, _ = common.lmpc_config(g, args.horizon, max_batch=256)
    rng = np.random.default_rng(args.seed)
    out = dict(debug_entry_us=[], note="lmpc_debug_live_compact from the host: allocation, three uploads, the launch, three downloads and the drain -- an upper bound on a rebuild")
    with _capi.Context(cfg) as ctx:
        for n in (256, 4096, 65536, 262144):
            done = np.where(rng.random(n) < 0.5, 100, -1).astype(np.int32); p0 = np.zeros(n, np.int32)
            ctx.debug_live_compact(done, p0, 8, _capi.PARK_FINISHED)
            t = []
            for _ in range(20):
                t0 = time.perf_counter(); ctx.debug_live_compact(done, p0, 8, _capi.PARK_FINISHED); t.append((time.perf_counter() - t0) * 1e6)
            out["debug_entry_us"].append(dict(n=n, **spread(t)))
        # the poll: 64 steps in which nobody finishes; PARK_FINISHED launches the kernel at each of the 8 polls (it returns at once), the start list alone does not
        for _ in range(4):
            ctx.model_add_trajectory(g["xPID"], g["uPID"]); ctx.ss_add_trajectory(g["xPID"], g["uPID"])
        B = 256
        x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1)); x0[:, 5] = np.linspace(-0.1, 0.1, B)
        xl = np.tile(np.array(g["xPID"])[None, 1:args.horizon + 2], (B, 1, 1)); ul = np.tile(np.array(g["uPID"])[None, 1:args.horizon + 1], (B, 1, 1))
        noise = rng.standard_normal((64, B, 3))
        t = {0: [], _capi.PARK_FINISHED: []}
        for rep in range(2 * (args.repeats + 1)):
            for mode in ((0, _capi.PARK_FINISHED) if rep % 2 == 0 else (_capi.PARK_FINISHED, 0)):
                ctx.rollout_set_parking(mode, [B - 1])             # (one car on the start list, so that both sessions run the list kernels)
                ctx.rollout_begin(x0, x0, xl, ul, noise); ctx.sync()
                t0 = time.perf_counter(); ctx.rollout_run(64); ctx.sync(); dt = (time.perf_counter() - t0) * 1e3
                ctx.rollout_end()
                if rep > 1:
                    t[mode].append(dt)
        a, b = spread(t[0]), spread(t[_capi.PARK_FINISHED])
        out["poll_B256_64_steps_ms"] = dict(start_list_only=a, park_finished=b, per_poll_us=round((b["median"] - a["median"]) / 8 * 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit, for (a)")
    ap.add_argument("--skip-ab", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--ab-only", action="store_true", help="(a) alone")
    ap.add_argument("--ab-parked", action="store_true", help="(a) with a parked generation at B = 256 and B = 4096 (the parent must have parking)")
    ap.add_argument("--leg", choices=["off", "parked"], help="(internal) one leg of (a), run on --tree")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parking.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if args.leg:
        return leg(args, args.leg == "parked")
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
        raise SystemExit("park_bench needs a GPU: %s" % e)
    g = common.load_lmpc_golden()
    result = dict(horizon=args.horizon, repeats=args.repeats, T_max=400, ext=40)
    if os.path.exists(args.out):                                  # (a run with --skip-ab keeps the A / B of an earlier one)
        with open(args.out) as f:
            result = dict(json.load(f), **result)
    if not args.ab_only:
        result["b_parked_against_unparked"] = measure_parked(args, g)
        result["c_compaction"] = measure_compaction(args, g)
    if not args.skip_ab:
        result["a_off_against_parent"] = measure_ab(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
