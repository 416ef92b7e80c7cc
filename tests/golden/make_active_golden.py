"""tests/golden/make_active_golden.py -- tests/golden/lmpc_active.npz: QPs with ACTIVE inequality rows at every built horizon, each with its certified optimum.

CPU only; uses oracle/ and tests/ and nothing else (no reference tree).  ~3 min on eight cores.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_active_golden.py          then   python tests/golden/manifest.py write

Stores.  The oracle's restatement of the reference flow (closed_loop.OracleFlow(g, 12, "osqp"): restated OSQP at eps = 1e-3 + polish) runs 30 laps at seed 5; lap
lengths fall from 238 to 78 steps.  The safe set then holds 34 laps, the last one in progress; of the 33 complete ones the four with the fewest rows (ties: the older
lap) are taken -- 155, 157, 161, 163 rows, each a lap plus the rows addPoint appended during the next one -- with uSS cut to the rows of SS.

Directed problems (tests/active_cases.py: HORIZONS, FAMILIES, OFFSETS, START_ROWS): per horizon, start rows on the 155-row lap x the seven offset families.
Every candidate is solved by both of the oracle's methods (osqp_solve_exact: restated ADMM + polish; dense_ipm_solve: dense interior point + active-set finish) through
tests/oracle_pool -- the call the GPU tests use -- and enters only if the two agree on (x, u) to 1e-9 (1 + |z*|) and both certificates are <= 1e-8.

Closed-loop records, N = 12 and N = 14 (N = 14: a run of its own, seed 5): the QPs of the last ten laps as OracleFlow.dump holds them, ranked by the number of lane
slacks above 1e-6 at the optimum, ties in dump order; they are solved again by both methods in that order until 32 have passed the same admission rule.  (N = 20 and N = 40 are not run in closed loop from the PID stores: the regression turns singular after 123 and 24 steps.)

The script prints the rejections and the coverage per horizon and fails if more than 10 % of a horizon's candidates (directed and closed-loop together) were rejected or a horizon holds fewer than
8 problems with an active lane slack, 8 with an input at a bound, 4 with both, 2 with neither.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import lmpc_oracle as orc  # noqa: E402
from tests import active_cases as ac, closed_loop, common  # noqa: E402

SEED, LAPS, DUMP_FROM, N_CL = 5, 30, 20, 32
K1_SAMPLE = 3            # problems per horizon whose A, B, C and selection are stored (first, middle, last)


def flow(g, N):
    f = closed_loop.OracleFlow(g, N, "osqp")
    out = closed_loop.run_laps(f, g, LAPS, seed=SEED, dump_from=DUMP_FROM)
    assert len(out) == LAPS and all("error" not in r for r in out), out[-1]
    return f, out


def stores(f):
    c = f.ctrl
    rows = [s.shape[0] for s in c.SS[:-1]]                                # (the last entry is the lap in progress)
    pick = sorted(range(len(rows)), key=lambda i: (rows[i], i))[:4]
    return [(np.array(c.SS[i]), np.array(c.uSS[i])[:rows[i]]) for i in pick]


def _cl_work(args):
    r, N = args
    par = orc.QPParams.lmpc_default(N)
    P, q, A, l, u = orc.assemble_lmpc_qp(par, r["A"], r["B"], r["C"], r["x0"], r["uOld"], r["SS"], r["Qsel"])
    ex, cert = orc.osqp_solve_exact(P, q, A, l, u)                       # (certificate 1e-9: at 1e-8 one flat closed-loop QP in eight ends 1e-8 from the other method's optimum)
    r2 = orc.dense_ipm_solve(P, q, A, l, u)
    return dict(opt=ex.x, opt2=r2.x, cert=cert, cert2=max(orc.kkt_certificate(P, q, A, l, u, r2.x, r2.y).values()))


def _cl_rank(args):
    r, N = args
    P, q, A, l, u = orc.assemble_lmpc_qp(orc.QPParams.lmpc_default(N), r["A"], r["B"], r["C"], r["x0"], r["uOld"], r["SS"], r["Qsel"])
    return ac.active_counts(orc.dense_ipm_solve(P, q, A, l, u).x, N)[0]


def closed_loop_records(dump, N):
    """32 admitted QPs of the dump, most active lane slacks AT THE OPTIMUM first (every QP of the dump is solved once by dense_ipm_solve for the ranking: the flow's
    own eps = 1e-3 answer carries slacks of 1e-4 on rows that are inactive at the optimum), ties in dump order."""
    import multiprocessing as mp
    with mp.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        nact = np.array(pool.map(_cl_rank, [(d, N) for d in dump], chunksize=8))
        order = np.argsort(-nact, kind="stable")
        keep, rejected, pos = [], 0, 0
        while len(keep) < N_CL:
            chunk = order[pos:pos + N_CL - len(keep)]; pos += len(chunk)
            assert len(chunk), "the dump ran out of QPs"
            for i, s in zip(chunk, pool.map(_cl_work, [(dump[i], N) for i in chunk], chunksize=1)):
                if ac.admitted(s, N):
                    keep.append((int(i), s))
                else:
                    rejected += 1
    keep.sort(key=lambda a: (-nact[a[0]], a[0]))
    return keep, rejected, nact


def main():
    try:
        from threadpoolctl import threadpool_limits
        threadpool_limits(1)                                               # one BLAS thread per process: the same sums on every machine
    except Exception:                                                     # noqa: BLE001
        pass
    g = common.load_lmpc_golden()
    f12, laps12 = flow(g, 12)
    print("N = 12 flow, seed %d: lap lengths %s" % (SEED, [r["steps"] for r in laps12]))
    lap_list = stores(f12)
    print("stores: %s rows, vx up to %.2f, |ey| up to %.2f" % ([x.shape[0] for x, _ in lap_list], max(x[:, 0].max() for x, _ in lap_list), max(np.abs(x[:, 5]).max() for x, _ in lap_list)))
    out = dict(horizons=np.array(ac.HORIZONS), cl_horizons=np.array(ac.CL_HORIZONS), families=np.array(ac.FAMILIES), offsets=ac.OFFSETS)
    for i, (x, u) in enumerate(lap_list):
        out["lapx%d" % i], out["lapu%d" % i] = x, u
    fails, tally = [], {}
    for N in ac.HORIZONS:
        rows = np.array(ac.START_ROWS[N])
        assert rows.min() >= 5 and rows.max() <= 113 - N
        t = np.repeat(rows, len(ac.FAMILIES)); fam = np.tile(np.arange(len(ac.FAMILIES)), len(rows))
        inp = ac.directed_inputs(lap_list, N, t, fam)
        res = ac.oracle_records(lap_list, N, inp, range(len(t)), solve=True)
        ok = np.array([ac.admitted(r, N) for r in res])
        res = [r for r, o in zip(res, ok) if o]
        K = len(res); p = "n%d_" % N
        for k in ("x0", "uOld", "zt", "timeStep"):
            out[p + k] = inp[k][ok]
        out[p + "t"], out[p + "fam"] = t[ok], fam[ok]
        z = [ac.split(r["opt"], N) for r in res]
        for j, k in enumerate(("x", "u", "slack", "lambd", "sTerm")):
            out[p + k] = np.stack([a[j] for a in z])
        out[p + "cert"] = np.array([[r["cert"], r["cert2"]] for r in res])
        cnt = np.array([ac.active_counts(r["opt"], N) for r in res])
        out[p + "nact_slack"], out[p + "nact_u"] = cnt[:, 0], cnt[:, 1]
        out[p + "lam_unique"] = np.array([ac.lambda_unique(r, N) for r in res])
        k1 = np.unique(np.linspace(0, K - 1, K1_SAMPLE).round().astype(int))
        out[p + "k1"] = k1
        for k in ("A", "B", "C", "SSsel", "Qsel", "Succ", "SuccU"):
            out[p + k] = np.stack([np.asarray(res[i][k]) for i in k1])
        s, b = cnt[:, 0] > 0, cnt[:, 1] > 0
        cov = (int(s.sum()), int(b.sum()), int((s & b).sum()), int((~s & ~b).sum()))
        print("N = %2d: %d candidates, %d rejected; active lane slack on %d problems (up to %d rows), input at a bound on %d (up to %d steps), both %d, neither %d; "
              "lambda* unique on %d; worst certificate %.1e" % (N, len(ok), int((~ok).sum()), cov[0], cnt[:, 0].max(), cov[1], cnt[:, 1].max(), cov[2], cov[3],
                                                               int(out[p + "lam_unique"].sum()), out[p + "cert"].max()))
        tally[N] = [len(ok), int((~ok).sum())]
        if not (cov[0] >= 8 and cov[1] >= 8 and cov[2] >= 4 and cov[3] >= 2):
            fails.append("N = %d: coverage (slack, bound, both, neither) = %s" % (N, cov))
    for N in ac.CL_HORIZONS:
        f, laps_n = (f12, laps12) if N == 12 else flow(g, N)
        keep, rejected, nact = closed_loop_records(f.dump, N)
        p = "cl%d_" % N
        for k in ("A", "B", "C", "x0", "uOld", "SS", "Qsel"):
            out[p + k] = np.stack([np.asarray(f.dump[i][k], float) for i, _ in keep])
        z = [ac.split(s["opt"], N) for _, s in keep]
        for j, k in enumerate(("x", "u", "slack", "lambd", "sTerm")):
            out[p + k] = np.stack([a[j] for a in z])
        out[p + "cert"] = np.array([[s["cert"], s["cert2"]] for _, s in keep])
        out[p + "dump_index"] = np.array([i for i, _ in keep])
        cnt = np.array([ac.active_counts(s["opt"], N) for _, s in keep])
        out[p + "nact_slack"], out[p + "nact_u"] = cnt[:, 0], cnt[:, 1]
        print("N = %2d closed loop (lap lengths %s): %d QPs in the last ten laps, %d rejected on the way to %d; active lane slacks %d .. %d, input-bound steps %d .. %d; worst certificate %.1e"
              % (N, [r["steps"] for r in laps_n][DUMP_FROM:], len(f.dump), rejected, len(keep), cnt[:, 0].min(), cnt[:, 0].max(), cnt[:, 1].min(), cnt[:, 1].max(), out[p + "cert"].max()))
        tally[N][0] += rejected + len(keep); tally[N][1] += rejected
    for N, (cand, rej) in tally.items():                                   # per horizon, directed candidates and closed-loop candidates together
        print("N = %2d: %d of %d candidates rejected" % (N, rej, cand))
        if rej > 0.1 * cand:
            fails.append("N = %d: %d of %d candidates rejected" % (N, rej, cand))
    assert not fails, "\n".join(fails)
    np.savez_compressed(ac.PATH, **out)
    size = os.path.getsize(ac.PATH)
    print("wrote %s: %d bytes" % (ac.PATH, size))
    assert size < 1 << 20, "a committed file stays below 1 MiB"


if __name__ == "__main__":
    main()
