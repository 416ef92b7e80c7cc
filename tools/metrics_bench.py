"""Developer tool (GPU box): what the lap metrics cost (lmpc_rollout_lap_metrics).  Writes profiles/lap_metrics.json.

    python tools/metrics_bench.py --parent DIR [--repeats 5] [--out profiles/lap_metrics.json]      both measurements
    python tools/metrics_bench.py --skip-ab                                                         (b) only: no parent build at hand

Host clock; every timed region ends in a device synchronise (both entry points drain the stream before they return); `repeats` runs per figure, medians reported
with min, max and every run.  Reported, not asserted.
(a) No regression with the feature unused.  DIR is a built checkout of the parent commit.  `python bench.py --gpus 1 --steps 200 --warmup 20` in the parent's tree and
    in this one, alternating, every run a process of its own.  Rule: this build's median inside the parent's own min .. max.
(b) The call against the download it replaces.  One PID session of B cars and T = 400 steps (device noise, not stopping at the line), finished; then, alternating:
    one rollout_lap_metrics call over all B cars with 400 rows each; rollout_fetch of the full logs (T x B x 14 doubles); and the NumPy restatement
    tests/metrics_ref.py over the fetched logs (one car at a time: the order contract, not speed, is what it is written for).  B = 256, 1024, 4096."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)), all=[round(float(x), 4) for x in v])


def measure_ab(args):
    trees = [("parent", os.path.abspath(args.parent)), ("this", ROOT)]
    bench = ["bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"]
    runs = {name: [] for name, _ in trees}
    for rep in range(args.repeats):
        for name, tree in (trees if rep % 2 == 0 else trees[::-1]):
            out = subprocess.run([sys.executable] + bench, cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout
            runs[name].append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"])
            print("a/b run %d, %s: %.1f" % (rep, name, runs[name][-1]), file=sys.stderr, flush=True)
    p, t = runs["parent"], runs["this"]
    return dict(what="python bench.py --gpus 1 --steps 200 --warmup 20: parent's build and this one alternating, %d runs each, every run a process of its own" % args.repeats,
                rule="this build's median inside the parent's own min .. max", figure="headline_solves_per_s",
                parent_runs=p, this_runs=t, parent_median=float(np.median(p)), parent_range=[min(p), max(p)], this_median=float(np.median(t)), this_range=[min(t), max(t)],
                this_median_inside_parent_range=bool(min(p) <= np.median(t) <= max(p)))


def measure_call(args, g):
    from racinglmpc_amd import _capi
    from tests import common, metrics_ref
    out = []
    T = args.steps
    for B in args.batches:
        cfg, _ = common.lmpc_config(g, args.horizon, max_batch=B, max_laps=4, max_lap_len=512)
        Fx, Fu = np.array(list(cfg.Fx)).reshape(2, 6), np.array(list(cfg.Fu)).reshape(4, 2)
        w = metrics_ref.weights_of_config(cfg)
        with _capi.Context(cfg) as ctx:
            ctx.rollout_set_noise(True, seed=args.seed)
            x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1))
            t, n_done = ctx.rollout_pid(x0, x0, np.linspace(0.7, 0.9, B), None, None, stop_at_line=False, T_max=T)
            cars, rows = np.arange(B), np.full(B, t)
            ctx.rollout_lap_metrics(cars, rows); ctx.rollout_fetch(0, t)                            # (untimed first: the pooled scratch and the host pages exist)
            call, fetch, ref = [], [], []
            ref_runs = args.repeats if B <= 1024 else 1                                             # (seconds per run at 4096 cars)
            for rep in range(args.repeats):
                t0 = time.perf_counter(); m = ctx.rollout_lap_metrics(cars, rows); call.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); X, U, G, done, st, fx, fg = ctx.rollout_fetch(0, t); fetch.append((time.perf_counter() - t0) * 1e3)
                if rep < ref_runs:
                    t0 = time.perf_counter()
                    r = metrics_ref.session_metrics(X, U, G, done, fx, cars, rows, lambda c: w, Fx, Fu, lambda c: float(cfg.trackLength))
                    ref.append((time.perf_counter() - t0) * 1e3)
            ctx.rollout_end()
        same = bool(np.array_equal(np.ascontiguousarray(m).view(np.int64), np.ascontiguousarray(r).view(np.int64)))
        out.append(dict(B=B, rows=int(t), cars_across_the_line=int(n_done), log_bytes=int(t) * B * 14 * 8, result_bytes=B * _capi.METRICS_NCOL * 8,
                        metrics_call_ms=spread(call), fetch_full_logs_ms=spread(fetch), numpy_restatement_ms=spread(ref),
                        call_over_fetch=round(float(np.median(call) / np.median(fetch)), 4), device_equals_restatement_bit_for_bit=same))
        print("b: %s" % json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit, for (a)")
    ap.add_argument("--skip-ab", action="store_true")
    ap.add_argument("--ab-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lap_metrics.json"))
    args = ap.parse_args()
    if not args.skip_ab and not args.parent:
        raise SystemExit("--parent DIR (a built checkout of the parent commit) or --skip-ab")
    import __graft_entry__ as ge
    ge.build()
    from tests import common
    result = dict(tool="tools/metrics_bench.py", repeats=args.repeats, clock="host perf_counter; every region ends in a device synchronise")
    if not args.ab_only:
        result["b_call_against_fetch"] = measure_call(args, common.load_lmpc_golden())
    if not args.skip_ab:
        result["a_unused_against_parent"] = measure_ab(args)
    result["not_measured"] = ["the kernel alone (no profiler run: the figures are whole calls, table upload and result download included)",
                              "sessions with per-car tuning rows (B weights rows in the upload instead of one)",
                              "the LMPC loop with metrics=True against metrics=False (one call per generation beside hundreds of step launches)",
                              "more than one GPU"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
