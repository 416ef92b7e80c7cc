"""Test infrastructure: the oracle (oracle/lmpc_oracle.py) over many problems of a batch, one single-threaded process per host core.

The per-problem oracle work of the all-problem parity tests -- regression of N points (~1 ms each), selection, and, where asked, the QP solved
to its certified optimum (osqp_solve_exact: 0.1 s at N = 12, 0.3-1 s at N = 40) -- is minutes of one core for a 1024-problem batch; the GPU
box has a few hundred hardware threads.  Children never touch HIP (fork start method: they inherit the parent's memory, run NumPy, return arrays).
"""
import os

import numpy as np

_JOB = {}


def select_laps(xS, uS, Qf, z, ppl, xPrev, cur_it, tstep, N, TL):
    """SS_sel, Qfun_sel, Succ, SuccU of `ppl` points from each of the laps xS (oracle.terminal_components with numSS_Points = ppl len(xS)).

    An even ppl is the reference's own selection.  With an odd ppl the reference's window arithmetic (selectPoints :492-495: numPoints = ppl + 1 is even, and
    range(-numPoints / 2 + MinNorm, numPoints / 2 + MinNorm + 1) has numPoints + 1 entries) selects ppl + 1 columns per lap wherever the window is centred, one more
    than its QP has (numSS_Points = ppl numSS_it columns, :340-362): the reference cannot assemble such a step, so there is nothing of it to restate.  The library
    defines the case -- columns start .. start + ppl - 1 of the same window, successors start + 1 .. start + ppl (lmpc_solve_common.hip.h, k2_select) -- and the
    records follow that rule: the first ppl columns of the reference's window, which is the reference's selection itself for every even ppl."""
    from oracle import lmpc_oracle as orc
    L = len(xS)
    if ppl % 2 == 0:
        return orc.terminal_components(xS, uS, Qf, [x.shape[0] for x in xS], z, ppl * L, L, xPrev, cur_it, tstep, N, TL)
    SSsel = np.empty((6, 0)); Succ = np.empty((6, 0)); SuccU = np.empty((2, 0)); Qsel = np.empty(0)
    for jj in np.argsort(np.array([x.shape[0] for x in xS]))[:L]:
        P, U, Q = orc.select_points(xS[jj], uS[jj], Qf[jj], jj, z, ppl + 1, xPrev, cur_it, tstep, N, TL)
        SSsel = np.append(SSsel, P[:, :ppl], axis=1); Qsel = np.append(Qsel, Q[:ppl], axis=0)
        Succ = np.append(Succ, P[:, 1:ppl + 1], axis=1); SuccU = np.append(SuccU, U[:, 1:ppl + 1], axis=1)
    return SSsel, Qsel, Succ, SuccU


def _work(b):
    from oracle import lmpc_oracle as orc
    j = _JOB
    inp, N, TL, pt = j["inp"], j["N"], j["TL"], j["pt"]
    xM = [l[0] for l in j["laps"]]; uM = [l[1] for l in j["laps"]]
    A, B, C = orc.compute_ltv_dynamics(xM, uM, list(range(len(xM))), pt, inp["xLin"][b], inp["uLin"][b], N)
    ss = j["laps"] if j.get("ss_laps") is None else j["ss_laps"]
    xS = [l[0] for l in ss]; uS = [l[1] for l in ss]
    Qf = [orc.compute_cost(x, TL) for x in xS]
    z = inp["zt"][b].copy()
    if z[4] - inp["x0"][b][4] > TL / 2:
        z[4] = np.max([z[4] - TL, 0])
    L = len(xS)
    xPrev = inp["xPredPrev"][b] if "hasPred" in inp and inp["hasPred"][b] else None          # (the reference's `self.xPred == []` on a first step)
    SSsel, Qsel, Succ, SuccU = select_laps(xS, uS, Qf, z, j.get("ppl", 12), xPrev, L, int(inp["timeStep"][b]), N, TL)
    res = dict(b=b, A=A, B=B, C=C, SSsel=SSsel, Qsel=Qsel, Succ=Succ, SuccU=SuccU)
    if b in j["solve"]:
        P, q, Ao, l, u = orc.assemble_lmpc_qp(j["par"], A, B, C, inp["x0"][b], inp["uOld"][b], SSsel, Qsel)
        ex, cert = orc.osqp_solve_exact(P, q, Ao, l, u, want=1e-8)
        res.update(opt=ex.x, cert=cert, obj=float(0.5 * ex.x @ P @ ex.x + q @ ex.x), Pq=(np.asarray(P.todense()) if hasattr(P, "todense") else np.asarray(P), np.asarray(q)))
        # a second certified optimum by the other method (dense interior point on the explicit matrices): where the two disagree on lambda the QP has more
        # than one optimal lambda (x, u are unique, lambda is not: SURVEY 8(c)-3) and zt = Succ lambda is not a function of the QP alone
        r2 = orc.dense_ipm_solve(P, q, Ao, l, u)
        res.update(opt2=r2.x, cert2=max(orc.kkt_certificate(P, q, Ao, l, u, r2.x, r2.y).values()))
    return res


def _objf(P, q):
    return lambda z: float(0.5 * z @ P @ z + q @ z)


def oracle_batch(par, pt, TL, laps, N, inp, idx, solve_idx=(), procs=None, ss_laps=None, ppl=12):
    """Oracle results for the problems `idx` of `inp` (stores: `laps`, used both as regression store and as safe set, in the library's order):
    list of dicts b, A, B, C, SSsel (6, S), Qsel, Succ, SuccU and -- for b in solve_idx -- opt (the certified optimum z*), cert, obj.
    ss_laps: the safe set where it is not the regression store;  ppl: safe-set points per lap (numSS_Points / numSS_it; select_laps)."""
    import multiprocessing as mp
    try:
        from threadpoolctl import threadpool_limits
        lim = threadpool_limits(1)                     # (inherited by the forked children: one BLAS thread per process)
    except Exception:                                 # noqa: BLE001
        lim = None
    _JOB.clear()
    _JOB.update(par=par, pt=np.asarray(pt), TL=float(TL), laps=[(np.asarray(x), np.asarray(u)) for x, u in laps], N=int(N), inp=inp, solve=set(int(b) for b in solve_idx),
                ss_laps=None if ss_laps is None else [(np.asarray(x), np.asarray(u)) for x, u in ss_laps], ppl=int(ppl))
    idx = [int(b) for b in idx]
    n = procs or max(1, min(64, (os.cpu_count() or 2) - 2, len(idx)))
    try:
        if n == 1:
            out = [_work(b) for b in idx]
        else:
            with mp.get_context("fork").Pool(n) as pool:
                out = pool.map_async(_work, idx, chunksize=max(1, len(idx) // (4 * n))).get(timeout=420)     # (a worker that dies leaves map() waiting for ever: fail instead)
        for r in out:
            if "Pq" in r:
                r["objf"] = _objf(*r.pop("Pq"))
        return out
    finally:
        _JOB.clear()
        if lim is not None:
            lim.restore_original_limits() if hasattr(lim, "restore_original_limits") else None
