"""What giving laps back buys a long run: B independent learners (rollout.PerCarLMPC(device_commit=True)) for G generations, once with prune=True and once without,
from the same seed laps and the same noise.

    python tools/retain_bench.py [--cars 256 1024 8192] [--generations 10] [--budget 240] [--out profiles/store_retain.json]

Per B and per run: resident device memory after the last generation (free memory before the context was created minus free memory then: lmpc_device_memory), the
number of store growths, wall time per generation, and for the pruned run every Context.store_retain call: its wall time, the laps it kept, the bytes its gather read
and wrote (9 columns x rows of every kept lap, the prefilter image of the regression laps) and the bytes it zero-filled (the new allocations), with the rate next to
the 6.29 TB/s a device-to-device copy reaches on this chip -- for orientation only: a call also allocates, frees and drains.
The library has no getter for the stores' capacity: the growths are counted from the lap counts by its own rule (capacity = initial max_laps x 2^j, one growth per
commit that does not fit; a retain sets the smallest such capacity that holds the kept laps).
--budget: seconds per (B, run) after which no further generation is started (8192 cars: as many generations as fit the time); the generations run are recorded.
Recorded, not gated: the expectation is memory constant in the generation count with prune, linear without."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29         # device-to-device copy rate of the chip, TB/s (orientation)
CHUNK = 1024            # K1_CHUNK: rows of one prefilter-image chunk


def lap_slot_bytes(max_lap_len):
    return 2 * 9 * max_lap_len * 8 + 3 * max_lap_len * 4 + (max_lap_len + CHUNK - 1) // CHUNK * 48


def run(g, B, G, prune, seed, budget):
    from racinglmpc_amd import _capi, rollout
    from tests import common
    init_laps, lap_len = B, 1024
    cfg, _ = common.lmpc_config(g, 12, max_batch=B, max_laps=init_laps, max_lap_len=lap_len)
    free0 = _capi.device_memory(0)[0]
    cap = [init_laps]; growths = [0]; retains = []
    with _capi.Context(cfg) as ctx:
        def fit(n):                                        # the library's growth rule, from the lap counts
            if n > cap[0]:
                growths[0] += 1
                while cap[0] < n:
                    cap[0] *= 2
        real = ctx.store_retain

        def timed(ss=None, model=None):
            fit(max(ctx.ss_num_laps(), ctx.model_num_laps()))
            rows_ss = [ctx.ss_lap_rows(l) for l in ss]; rows_m = [ctx.model_lap_info(l)[0] for l in model]
            moved = 2 * (sum(9 * 8 * r for r in rows_ss) + sum(9 * 8 * r + 3 * 4 * (r - 1) + (r - 1 + CHUNK - 1) // CHUNK * 48 for r in rows_m))
            ctx.sync()
            t0 = time.perf_counter()
            out = real(ss=ss, model=model)
            dt = time.perf_counter() - t0
            new_cap = init_laps
            while new_cap < max(len(ss), len(model)):
                new_cap *= 2
            cap[0] = new_cap
            retains.append(dict(seconds=dt, kept_ss=len(ss), kept_model=len(model), bytes_gathered=moved, bytes_zero_filled=new_cap * lap_slot_bytes(lap_len),
                                gather_TBps_of_call=moved / dt / 1e12, copy_TBps_of_chip=COPY_TBS))
            return out
        ctx.store_retain = timed
        ro = rollout.BatchedRollouts(ctx, g["track"], seed=seed, device_noise=True)
        vt = 0.75 + 0.1 * (np.arange(B) % 16) / 15.0
        pid = ro.run_pid_laps(vt, max_steps=1000, keep_invalid=True)
        bad = [b for b, l in enumerate(pid) if l[4] < 0 or (l[5] & ~_capi.ST_INEXACT) != 0]
        if bad:
            raise SystemExit("PID lap of car(s) %s did not finish or was flagged: no seed lap" % bad[:8])
        loop = rollout.PerCarLMPC(ro, T_max=400, ext=40, device_commit=True, prune=prune)
        loop.seed(pid)
        fit(max(ctx.ss_num_laps(), ctx.model_num_laps()))
        wall, counts = [], []
        t_start = time.perf_counter()
        for _ in range(G):
            if time.perf_counter() - t_start > budget:
                break
            t0 = time.perf_counter()
            loop.run()
            ctx.sync()
            wall.append(time.perf_counter() - t0)
            if not prune:
                fit(max(ctx.ss_num_laps(), ctx.model_num_laps()))
            counts.append([ctx.ss_num_laps(), ctx.model_num_laps()])
        resident = free0 - _capi.device_memory(0)[0]
        out = dict(prune=prune, generations=len(wall), resident_bytes_after_last_generation=int(resident), store_growths=growths[0], lap_capacity=cap[0],
                   stores_bytes_at_capacity=cap[0] * lap_slot_bytes(lap_len), seconds_per_generation=wall, laps_stored=counts, retired=len(loop.retired),
                   lap_steps_mean=[float(np.mean([t[k] for t in loop.lap_times if len(t) > k])) for k in range(len(wall)) if any(len(t) > k for t in loop.lap_times)],
                   retains=retains)
        loop.close()
    return out, [list(t) for t in loop.lap_times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cars", type=int, nargs="+", default=[256, 1024, 8192])
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--budget", type=float, default=240.0, help="seconds per (B, run) after which no further generation is started")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_retain.json"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from tests import common
    g = common.load_lmpc_golden()
    result = dict(generations=args.generations, seed=args.seed, max_lap_len=1024, lap_slot_bytes=lap_slot_bytes(1024), sizes=[])
    for B in args.cars:
        pruned, lt_p = run(g, B, args.generations, True, args.seed, args.budget)
        plain, lt_f = run(g, B, args.generations, False, args.seed, args.budget)
        n = min(pruned["generations"], plain["generations"])
        same = [t[:n] for t in lt_p] == [t[:n] for t in lt_f]
        result["sizes"].append(dict(cars=B, same_lap_times=bool(same), pruned=pruned, unpruned=plain))
        print("B = %5d: resident %.1f MB pruned, %.1f MB unpruned; growths %d / %d; s per generation %.2f / %.2f; same lap times: %s" % (
            B, pruned["resident_bytes_after_last_generation"] / 2**20, plain["resident_bytes_after_last_generation"] / 2**20, pruned["store_growths"], plain["store_growths"],
            float(np.mean(pruned["seconds_per_generation"])), float(np.mean(plain["seconds_per_generation"])), same), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
