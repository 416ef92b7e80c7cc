"""Developer tool (GPU box): one LMPC generation of B device-resident cars with chosen cars traced (BatchedRollouts(trace=), lmpc_rollout_set_trace), written as an
.npz: the trace planes (steps, listed cars, ...), `cars`, `doneAt`, and per listed car its lap lap<car>_x / _u / _xglob up to the crossing step -- what
rollout.TraceView(track, car, [(trace, lap)]) takes.

--slowest: every car is listed with the SOLVER plane (other planes only if --what names them) and the tool prints, per simulated step, which car needed the most
interior-point iterations and its status word: the slowest QP of a launch gates the launch, and this is the table of who that was.

    python tools/trace_export.py --batch 256 --cars 0,17,255 --out trace.npz
    python tools/trace_export.py --batch 256 --slowest --out slowest.npz > profiles/session_trace_slowest_B256.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench

PLANE_BITS = dict(xpred=1, upred=2, ss=4, qsel=8, solver=16, xy=32, all=63)


def parse_what(text):
    what = 0
    for name in text.split(","):
        if name.strip().lower() not in PLANE_BITS:
            raise SystemExit("--what: unknown plane %r (one of %s)" % (name, ", ".join(PLANE_BITS)))
        what |= PLANE_BITS[name.strip().lower()]
    return what


def slowest_table(iters, status, done):
    """Rows (step, car, iterations, status word, that car had crossed the line before this step, mean iterations of the launch, cars still racing)."""
    rows = []
    for t in range(iters.shape[0]):
        b = int(np.argmax(iters[t]))                      # (the first among equals)
        racing = (done < 0) | (done > t)
        rows.append((t, b, int(iters[t, b]), int(status[t, b]), bool(not racing[b]), float(iters[t].mean()), int(racing.sum())))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--cars", default="0", help="comma-separated car indices to trace (ignored with --slowest: every car)")
    ap.add_argument("--what", default=None, help="comma-separated planes: xpred, upred, ss, qsel, solver, xy, all (default: all; with --slowest: solver)")
    ap.add_argument("--steps", type=int, default=400, help="T_max of the session")
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--seed", type=int, default=100)
    ap.add_argument("--slowest", action="store_true")
    ap.add_argument("--out", default="trace.npz")
    a = ap.parse_args()
    from racinglmpc_amd import _capi, rollout
    B, N = a.batch, a.horizon
    cars = np.arange(B) if a.slowest else np.array([int(c) for c in a.cars.split(",")], np.int32)
    what = parse_what(a.what) if a.what else (_capi.TRACE_SOLVER if a.slowest else _capi.TRACE_ALL)
    if a.slowest:
        what |= _capi.TRACE_SOLVER
    g = bench.load_seed()
    ctx = bench.make_ctx(g, N, B, 0)
    print("# trace planes: %.1f MB on the device for %d cars x %d steps (what = %d)" % (ctx.rollout_trace_bytes(len(cars), what, a.steps) / 1e6, len(cars), a.steps, what))
    ro = rollout.BatchedRollouts(ctx, g["track"], seed=a.seed, trace=cars, trace_what=what)
    x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1)); x0[:, 5] = np.linspace(-0.1, 0.1, B); x0[:, 0] += np.linspace(0.0, 0.1, B)
    laps = ro.run_lap_device(x0, g["xPID"][1:N + 2], g["uPID"][1:N + 1], max_steps=a.steps, keep_invalid=True)
    tr, done, st = ro.last_trace, ro.last_done, ro.last_status
    out = dict(tr)
    for k, b in enumerate(cars if not a.slowest else []):
        x, u, xg = laps[int(b)][:3]
        out["lap%d_x" % b] = x; out["lap%d_u" % b] = u; out["lap%d_xglob" % b] = xg
    out["doneAt_all"] = done; out["status_all"] = st
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    steps = next(v.shape[0] for k, v in tr.items() if k not in ("cars", "doneAt"))
    print("# B = %d, N = %d, %d simulated steps, %d cars crossed the line, %d with a status bit other than INEXACT; planes %s -> %s" % (
        B, N, steps, int((done >= 0).sum()), int(((st & ~_capi.ST_INEXACT) != 0).sum()), sorted(k for k in tr if k not in ("cars", "doneAt")), a.out))
    if a.slowest:
        rows = slowest_table(tr["iters"], tr["status"], done)
        print("# step  car  iters  status  crossed_before  mean_iters_of_launch  cars_racing")
        for r in rows:
            print("%5d %5d %5d %6d %6d %12.2f %8d" % (r[0], r[1], r[2], r[3], int(r[4]), r[5], r[6]))
        it = tr["iters"]
        top = np.bincount(np.argmax(it, axis=1), minlength=B)
        print("# launches gated: max over steps of the slowest QP %d iterations, mean of the slowest %.2f, mean over all QPs %.2f; %d distinct cars were the slowest, car %d most often (%d of %d steps)" % (
            int(it.max()), float(it.max(axis=1).mean()), float(it.mean()), int((top > 0).sum()), int(np.argmax(top)), int(top.max()), steps))
    ro.close(); ctx.close()


if __name__ == "__main__":
    main()
