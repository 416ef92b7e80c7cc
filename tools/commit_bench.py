"""What happens between two laps of rollout.PerCarLMPC, timed both ways on the GPU: the host path (the whole session log downloaded, every car's lap handed in again
through the host entry points, one add and one extension call per car per store) against the device path (Context.rollout_extend_laps / rollout_commit_laps: the laps never leave the device).

    python tools/commit_bench.py [--batches 256 1024] [--repeats 5] [--horizon 12] [--out profiles/device_commit.json]

Per batch size and repeat, two FRESH contexts are seeded with the same per-car PID laps (device noise: same seed, same cars, hence the same session data) and run one
generation of PerCarLMPC, one with device_commit=False and one with True, in alternating order.  The seed laps end at the line, so the generation extends every
car's lap after `ext` steps and adds every valid lap at the end.  Timed with the host clock, each region ending in a device synchronise:
  bookkeeping   from the return of rollout_run(ext) to the next rollout_run (fetch + extension), plus from the return of the last rollout_run to the return of
                run() (fetch + adds, the end of the session, histories and tables) -- PerCarLMPC's own code, nothing re-implemented here;
  run           the whole PerCarLMPC.run() call.
One warm-up repeat is discarded.  Reported: median, minimum and maximum over the repeats, in milliseconds.  Needs a GPU: there is nothing to measure without one.
Writes --out and prints the result as one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_generation(g, N, B, seed, device_commit):
    """(bookkeeping ms, run ms, lap_times, steps, retired cars) of one generation on a fresh context."""
    from racinglmpc_amd import _capi, rollout
    from tests import common
    cfg, _ = common.lmpc_config(g, N, max_batch=B, max_laps=2 * B + 16, max_lap_len=1024)
    with _capi.Context(cfg) as ctx:
        ro = rollout.BatchedRollouts(ctx, g["track"], seed=seed, device_noise=True)
        pid = ro.run_pid_laps(0.75 + 0.1 * np.arange(B) / B, max_steps=1000, stop_at_line=True, keep_invalid=True)
        bad = [b for b, l in enumerate(pid) if l[4] < 0 or l[5] != 0]
        if bad:
            raise SystemExit("PID lap of car(s) %s did not finish or was flagged: no seed lap" % bad[:8])
        loop = rollout.PerCarLMPC(ro, T_max=400, ext=40, device_commit=device_commit)
        loop.seed(pid)
        ctx.sync()
        book = [0.0]; mark = [None]; steps = [0]
        real_run = ctx.rollout_run

        def timed_run(n):
            if mark[0] is not None:                     # (the extension's region ends where the next run begins)
                ctx.sync(); book[0] += time.perf_counter() - mark[0]
            out = real_run(n)
            ctx.sync(); mark[0] = time.perf_counter(); steps[0] = out[0]
            return out

        ctx.rollout_run = timed_run
        try:
            t0 = time.perf_counter()
            loop.run()
            ctx.sync()
            t1 = time.perf_counter()
            run = t1 - t0; book[0] += t1 - mark[0]      # (the host path adds the laps after rollout_end: the region ends with run())
        finally:
            del ctx.rollout_run
        loop.close()
        return book[0] * 1e3, run * 1e3, [list(t) for t in loop.lap_times], steps[0], len(loop.retired)


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), all=[round(float(x), 3) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_commit.json"))
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit("at least five repeats")
    import __graft_entry__ as ge
    ge.build()
    from racinglmpc_amd import _capi
    from tests import common
    try:
        _capi.device_memory(0)
    except _capi.LmpcError as e:
        raise SystemExit("commit_bench needs a GPU: %s" % e)
    g = common.load_lmpc_golden()
    result = dict(horizon=args.horizon, repeats=args.repeats, T_max=400, ext=40, unit="ms", batches=[])
    for B in args.batches:
        book = {False: [], True: []}; run = {False: [], True: []}
        info = None
        for rep in range(args.repeats + 1):                       # (repeat 0: warm-up, discarded)
            got = {}
            for dev in ((False, True) if rep % 2 == 0 else (True, False)):
                got[dev] = one_generation(g, args.horizon, B, args.seed, dev)
                if rep > 0:
                    book[dev].append(got[dev][0]); run[dev].append(got[dev][1])
            if got[False][2:] != got[True][2:]:
                raise SystemExit("B = %d: the two paths disagree on lap times, steps or retired cars" % B)
            info = got[True]
        laps = [t[0] for t in info[2] if t]
        result["batches"].append(dict(B=B, session_steps=info[3], laps_committed=len(laps), retired=info[4], lap_steps_min=min(laps), lap_steps_max=max(laps),
                                      host_bookkeeping=spread(book[False]), device_bookkeeping=spread(book[True]), host_run=spread(run[False]), device_run=spread(run[True])))
        print("B = %4d: bookkeeping host %.2f ms (%.2f .. %.2f), device %.2f ms (%.2f .. %.2f); run() host %.1f ms, device %.1f ms" % (
            B, *[result["batches"][-1]["host_bookkeeping"][k] for k in ("median", "min", "max")], *[result["batches"][-1]["device_bookkeeping"][k] for k in ("median", "min", "max")],
            result["batches"][-1]["host_run"]["median"], result["batches"][-1]["device_run"]["median"]), file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
