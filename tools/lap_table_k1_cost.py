"""What the per-problem lap table costs the regression kernel: K1's HIP-event time (lmpc_set_profiling, ms_regress / n_regress_timed) of lmpc_regress_batch at B = 256
and B = 4096, N = 12, for several builds of the library measured in turn in one visit to the GPU.

    python tools/lap_table_k1_cost.py [--tree NAME=DIR ...] [--lib NAME=FILE ...] [--reps 5] [--table-reps 2] [--out profiles/lap_table_k1.json]

--tree NAME=DIR   another checkout of this project with its library built (the parent commit, say): its racinglmpc_amd package is imported in a process of its own.
                  A tree without Context.model_set_lap_table gives the figures without a table only.
--lib NAME=FILE   another build of THIS tree's library (LMPC_LIB).  The "six-wave" rows of the committed file: --lib six-wave=racinglmpc_amd/liblmpc_hip_k1w6.so, the
                  flavour racinglmpc_amd.build.build_flavour("k1w6", ["LMPC_K1_TAB_WAVES8=6"]) makes -- <true, 8, true> compiled for six waves per SIMD (spills).
This tree is always measured, as "this".  Without a table: --reps processes per build, the builds alternating.  With a table (--table-reps processes per build that has
one): a table of one shared row; one own lap per car and four own laps per car out of 4096 distinct 1000-row laps (the golden PID lap + N(0, 0.01) on vx, vy, wz), car b
on laps b .. b + trToUse - 1; and the same with the first 400 rows of every lap (the 8-rows-per-lane scan).  10 warm-up + 60 timed launches per figure, microseconds."""
import argparse
import collections
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, WARM, TIMED = 12, 10, 60


def child(tree, with_table):
    sys.path.insert(0, tree)
    sys.path.append(ROOT)
    from racinglmpc_amd import _capi
    from oracle import lmpc_oracle as orc
    g = np.load(os.path.join(ROOT, "tests", "golden", "lmpc_n12.npz"))
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"])
    cases = {}
    with_table = with_table and hasattr(_capi.Context, "model_set_lap_table")

    def cfg_for(L):
        par = orc.QPParams.mpc_default(N, 0.8)
        return _capi.config_from(N, par.Q, par.R, par.Qf, par.dR, par.Qslack, par.Fx, par.bx, par.Fu, par.bu, par.xRef, numSS_it=0, trToUse=L, track=g["track"],
                                 trackLength=float(g["trackLength"]), max_batch=4096, max_laps=4096 + 8, max_lap_len=1024)

    def timed(ctx, B):
        tb = (37 * np.arange(B)) % 900
        rng = np.random.default_rng(7)
        xl = np.stack([xP[t:t + N + 1] for t in tb]) + rng.normal(scale=0.01, size=(B, N + 1, 6)) * np.array([1, 1, 1, 0, 0, 0.0])
        ul = np.stack([uP[t:t + N] for t in tb])
        ctx.set_profiling(1)
        for _ in range(WARM):
            ctx.regress_batch(xl, ul)
        ctx.reset_stats()
        for _ in range(TIMED):
            ctx.regress_batch(xl, ul)
        s = ctx.stats()
        ctx.set_profiling(0)
        return 1000.0 * s.ms_regress / s.n_regress_timed

    for rows in (1000, 400):
        for L in (1, 4):
            if rows == 400 and (L == 4 or not with_table):
                continue
            with _capi.Context(cfg_for(L)) as ctx:
                for _ in range(L):
                    ctx.model_add_trajectory(xP[:rows], uP[:rows])
                for B in (256, 4096):
                    cases["no table rows=%d trToUse=%d B=%d" % (rows, L, B)] = timed(ctx, B)
                if not with_table:
                    continue
                rng = np.random.default_rng(11)
                for b in range(4096):
                    ctx.model_add_trajectory(xP[:rows] + rng.normal(scale=0.01, size=(rows, 6)) * np.array([1, 1, 1, 0, 0, 0.0]), uP[:rows])
                for B in (256, 4096):
                    ctx.model_set_lap_table([list(range(L))])
                    cases["table, one shared row rows=%d trToUse=%d B=%d" % (rows, L, B)] = timed(ctx, B)
                    ctx.model_set_lap_table([[L + (b + j) % B for j in range(L)] for b in range(B)])
                    cases["table, own laps rows=%d trToUse=%d B=%d" % (rows, L, B)] = timed(ctx, B)
                    ctx.model_set_lap_table(None)
    print("K1COST " + json.dumps(cases), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", action="append", default=[], metavar="NAME=DIR")
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=FILE")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--table-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lap_table_k1.json"))
    ap.add_argument("--child", nargs=2, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]))
    builds = [(n, os.path.abspath(d), None) for n, d in (a.split("=", 1) for a in args.tree)] + [("this", ROOT, None)] + \
             [(n, ROOT, os.path.abspath(f)) for n, f in (a.split("=", 1) for a in args.lib)]
    agg = collections.OrderedDict()

    def one(name, tree, lib, table):
        env = dict(os.environ)
        if lib:
            env["LMPC_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, str(table)], capture_output=True, text=True, env=env, timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("K1COST ")]
        if r.returncode != 0 or not line:              # nothing more is started on the GPU after a failure
            sys.exit("%s failed (%d):\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
        for k, v in json.loads(line[0][7:]).items():
            agg.setdefault((k, name + (" (table run)" if table else "")), []).append(v)
        print(name, "table" if table else "", "ok", flush=True)

    for _ in range(args.reps):
        for name, tree, lib in builds:
            if lib is None:
                one(name, tree, None, 0)
    for _ in range(args.table_reps):
        for name, tree, lib in builds:
            if os.path.exists(os.path.join(tree, "racinglmpc_amd", "_capi.py")) and "model_set_lap_table" in open(os.path.join(tree, "racinglmpc_amd", "_capi.py")).read():
                one(name, tree, lib, 1)
    out = dict(tool="tools/lap_table_k1_cost.py " + " ".join("--tree %s=.." % n for n, _, l in builds if n != "this" and l is None) + " " + " ".join("--lib %s=.." % n for n, _, l in builds if l),
               what="K1 HIP-event time (lmpc_set_profiling, ms_regress / n_regress_timed) of lmpc_regress_batch, N = 12, one GPU, one visit, the builds in turn; "
                    "%d warm-up + %d timed launches per figure; microseconds.  bench.py's headline figure runs no lap table." % (WARM, TIMED),
               figures=[dict(case=k, build=b, runs=[round(x, 2) for x in v], mean=round(float(np.mean(v)), 2), min=round(min(v), 2), max=round(max(v), 2)) for (k, b), v in sorted(agg.items())])
    for f in out["figures"]:
        print("%-52s %-28s mean %7.2f  min %7.2f  max %7.2f  n=%d" % (f["case"], f["build"], f["mean"], f["min"], f["max"], len(f["runs"])))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
