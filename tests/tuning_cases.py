"""Rows and helpers of the per-car controller tuning tests (tests/test_tuning_host.py, tests/test_gpu_tuning.py; lmpc_tuning_set).

A row is the LMPC default tuning (oracle.QPParams.lmpc_default) with the fields of ROWS[name] replaced:

  R0   none
  R1   dR = (1, 10)                                      R2   dR = (20, 200)
  R3   Q = diag(0,0,0,0,0,10), R = diag(0.1, 1), QtermSlack = 100 I
  R4   bu = (0.4, 0.4, 5, 5), QtermSlack = diag(250, 500, 500, 1000, 2000, 500), Q = diag(1,0,0,0,0,0), xRef = (1.5, 0, 0, 0, 0, 0)
  R5   bx = (0.05, 0.02), Qslack = (20, 100)             the lane narrowed below the cars' ey: with bx = 0.3 the lane is not active and Qslack tests nothing
  R5a  bx = (0.05, 0.02)                                 R5b  R5a + Qslack = (20, 25)          R5c  R5a + Qslack = (5, 100)
  RQf  Qf = diag(0, 0, 0, 0, 0, 50)                      (differs from R0 in Qf only)
  and the single-field rows of the "every field reaches the kernel" test: Rbu (bu = (0.1, 0.1, 1, 1): the bu of R4 alone is not active on these problems and leaves R0's optimum), RT (QtermSlack = 100 I), RQ (Q and xRef of R4), RR (R of R3).

The problems: the 12 problems of common.synthetic_inputs(g, 12, 12), no previous prediction, on two sets of stores --
  "lap4"  common.stores_at_lap(g, 4): the PID lap four times as regression data; safe set SS0 three times and SS3[:1000] (the CPU facts below, tests/test_tuning_host.py);
  "pid4"  the PID lap four times in both stores, as tests/test_gpu_routes.py and bench.py set a context up (the GPU tests: oracle_pool.oracle_batch takes one list of
          laps for both stores).
A, B, C and the selection do not depend on the row; every row is solved on the same 12 QP data sets.

CPU outcome (the figures of DIST_MEASURED, CERT_MEASURED and MODEL_ITERS, measured once with study() below: oracle = dense_ipm_solve + kkt_certificate on the explicit matrices; model = the
NumPy model of the kernels' iteration, tests/ipm_model.py, in both forms -- exact_nu = True, the one-wave kernel, and False, the multi-wave kernels -- with the
kernels' max_iter = 40):
  * every QP of every row on both store sets is certified to <= CERT_MEASURED, and the model ends every one of them converged inside max_iter in both forms
    (iterations per row: MODEL_ITERS) -- R5's lane-active QPs included, so no row had to be replaced by a milder one;
  * distances |(x, u) - (x, u)'|_inf between the optima of two rows, minimum over the 12 problems: DIST_MEASURED (both store sets; the smaller figure is kept).
The host test re-derives certificate and distances on 6 of the 12 problems and holds them against these figures, halved."""
import numpy as np

from tests import common

N = 12
NPROB = 12


def _diag(*v):
    return np.diag(np.array(v, float))


ROWS = {
    "R0": {},
    "R1": dict(dR=(1.0, 10.0)),
    "R2": dict(dR=(20.0, 200.0)),
    "R3": dict(Q=_diag(0, 0, 0, 0, 0, 10), R=_diag(0.1, 1.0), QterminalSlack=100.0 * np.eye(6)),
    "R4": dict(bu=(0.4, 0.4, 5.0, 5.0), QterminalSlack=_diag(250, 500, 500, 1000, 2000, 500), Q=_diag(1, 0, 0, 0, 0, 0), xRef=(1.5, 0, 0, 0, 0, 0)),
    "R5": dict(bx=(0.05, 0.02), Qslack=(20.0, 100.0)),
    "R5a": dict(bx=(0.05, 0.02)),
    "R5b": dict(bx=(0.05, 0.02), Qslack=(20.0, 25.0)),
    "R5c": dict(bx=(0.05, 0.02), Qslack=(5.0, 100.0)),
    "RQf": dict(Qf=_diag(0, 0, 0, 0, 0, 50)),
    "Rbu": dict(bu=(0.1, 0.1, 1.0, 1.0)),
    "RT": dict(QterminalSlack=100.0 * np.eye(6)),
    "RQ": dict(Q=_diag(1, 0, 0, 0, 0, 0), xRef=(1.5, 0, 0, 0, 0, 0)),
    "RR": dict(R=_diag(0.1, 1.0)),
}
SIX = ("R0", "R1", "R2", "R3", "R4", "R5")                      # the rows of the batches: problem b gets SIX[(b + b // 6) % 6]
# the single-field rows: name of the test case -> (row, the row it must differ from by more than 100 TOL_XU)
FIELD_ROWS = {"dR": ("R1", "R0"), "Qslack[0]": ("R5b", "R5a"), "Qslack[1]": ("R5c", "R5a"), "bx": ("R5a", "R0"), "bu": ("Rbu", "R0"), "Qf": ("RQf", "R0"),
              "QtermSlack": ("RT", "R0"), "Q + xRef": ("RQ", "R0"), "R": ("RR", "R0")}

# (row, against): minimum over the 12 problems of |(x, u) - (x, u)'|_inf, the smaller of the two store sets -- measured by study(), see the module docstring
DIST_MEASURED = {("R1", "R0"): 1.014e-2, ("R2", "R0"): 8.454e-3, ("R3", "R0"): 5.823e-2, ("R4", "R0"): 1.437e-1, ("R5", "R0"): 1.639e-1, ("R5a", "R0"): 1.610e-1,
                 ("R5b", "R0"): 1.609e-1, ("R5c", "R0"): 1.639e-1, ("R5", "R5a"): 9.303e-3, ("R5c", "R5a"): 9.303e-3, ("R5b", "R5a"): 1.590e-4,
                 ("RQf", "R0"): 1.644e-2, ("Rbu", "R0"): 3.625e-2, ("RT", "R0"): 1.068e-2, ("RQ", "R0"): 9.295e-2, ("RR", "R0"): 2.059e-2}
CERT_MEASURED = 4.6e-13                # (2.3e-13 without Rbu)
# iterations of the model, (min, max) over both forms, both store sets and the 12 problems
MODEL_ITERS = {"R0": (7, 10), "R1": (6, 15), "R2": (7, 10), "R3": (7, 9), "R4": (7, 10), "R5": (10, 16), "R5a": (7, 11), "R5b": (7, 14), "R5c": (9, 14),
               "RQf": (7, 13), "Rbu": (7, 10), "RT": (7, 11), "RQ": (7, 12), "RR": (6, 10)}


def params(name, N=N, slacks=True):
    """oracle.QPParams of a row."""
    from oracle import lmpc_oracle as orc
    p = orc.QPParams.lmpc_default(N)
    for k, v in ROWS[name].items():
        v = np.array(v, float)
        setattr(p, k, v if v.ndim == 2 else v.reshape(-1))
    p.slacks = bool(slacks)
    return p


def row_of(par):
    """The 98 doubles of a tuning row from a QPParams record (the order of include/lmpc_hip.h), without the library."""
    T = np.zeros((6, 6)) if par.QterminalSlack is None else np.asarray(par.QterminalSlack, float)
    return np.concatenate([np.asarray(par.Q, float).ravel(), np.asarray(par.R, float).ravel(), np.asarray(par.Qf, float).ravel(), np.asarray(par.dR, float).ravel(),
                           np.asarray(par.Qslack, float).ravel(), np.diag(T), np.asarray(par.xRef, float).ravel(), np.asarray(par.bx, float).ravel(),
                           np.asarray(par.bu, float).ravel()])


def rows(names, N=N):
    return np.stack([row_of(params(n, N)) for n in names])


def config(g, name, N=N, max_batch=64, **kw):
    """(LmpcConfig, QPParams) of a context created with the row as its config: the reference of the row (an "own context")."""
    from racinglmpc_amd import _capi
    par = params(name, N)
    cfg = _capi.config_from(N, par.Q, par.R, par.Qf, par.dR, par.Qslack, par.Fx, par.bx, par.Fu, par.bu, par.xRef, QterminalSlack=par.QterminalSlack,
                            numSS_Points=48, numSS_it=4, trToUse=4, track=g["track"], trackLength=float(g["trackLength"]), max_batch=max_batch, **kw)
    return cfg, par


def row_index(B, n=6):
    """r(b) = (b + b // 6) % n: all 36 (problem, row) pairs occur in 36 problems, and a neighbour never has the same row."""
    b = np.arange(B)
    return (b + b // 6) % n


def stores(g, which):
    """(model laps, safe-set laps [(x, u)]) of a store set ("lap4" / "pid4")."""
    if which == "lap4":
        model, ss = common.stores_at_lap(g, 4)
        return [(np.array(x), np.array(u)) for x, u in model], [(np.array(x), np.array(u)) for x, u, _ in ss]
    pid = (np.array(g["xPID"]), np.array(g["uPID"]))
    return [pid] * 4, [pid] * 4


def fill(ctx, g, which="pid4"):
    model, ss = stores(g, which)
    for x, u in model:
        ctx.model_add_trajectory(x, u)
    for x, u in ss:
        ctx.ss_add_trajectory(x, u)


_QP_CACHE = {}


def qp_data(g, which, idx=range(NPROB)):
    """What the regression and the selection hand the QP for problems idx of synthetic_inputs(g, 12, 12) on a store set: [dict(A, B, C, x0, uOld, SS (6, S), Qsel)].
    Independent of the row.  Computed once per store set and shared."""
    from oracle import lmpc_oracle as orc
    if which not in _QP_CACHE:
        _QP_CACHE[which] = {}
    inp = common.synthetic_inputs(g, N, NPROB)
    model, ss = stores(g, which)
    pt = np.array(g["track"]); TL = float(g["trackLength"])
    out = []
    for b in idx:
        if b not in _QP_CACHE[which]:
            A, B, C = orc.compute_ltv_dynamics([m[0] for m in model], [m[1] for m in model], list(range(len(model))), pt, inp["xLin"][b], inp["uLin"][b], N)
            xs = [s[0] for s in ss]; us = [s[1] for s in ss]
            Qf = [orc.compute_cost(x, TL) for x in xs]
            z = inp["zt"][b].copy()
            if z[4] - inp["x0"][b][4] > TL / 2:
                z[4] = np.max([z[4] - TL, 0])
            SS, Qsel, _, _ = orc.terminal_components(xs, us, Qf, [x.shape[0] for x in xs], z, 48, 4, None, len(xs), int(inp["timeStep"][b]), N, TL)
            _QP_CACHE[which][b] = dict(A=np.array(A), B=np.array(B), C=np.array(C), x0=inp["x0"][b], uOld=inp["uOld"][b], SS=SS, Qsel=Qsel)
        out.append(_QP_CACHE[which][b])
    return out


def oracle_solve(par, d):
    """The oracle's optimum of one QP of qp_data under `par`: ((x, u) as one vector, worst entry of kkt_certificate)."""
    from oracle import lmpc_oracle as orc
    P, q, Ao, lo, up = orc.assemble_lmpc_qp(par, d["A"], d["B"], d["C"], d["x0"], d["uOld"], d["SS"], d["Qsel"])
    r = orc.dense_ipm_solve(P, q, Ao, lo, up)
    cert = max(orc.kkt_certificate(P, q, Ao, lo, up, r.x, r.y).values())
    nxu = 6 * (par.N + 1) + 2 * par.N
    return np.array(r.x[:nxu]), float(cert)


def model_solve(par, d, exact_nu, maxit=40):
    """The NumPy model of the kernels' iteration on the same QP: (converged inside maxit, iterations)."""
    from tests import ipm_model
    qp = ipm_model.StructQP(par, d["A"], d["B"], d["C"], d["x0"], d["uOld"], d["SS"], d["Qsel"])
    with np.errstate(all="ignore"):
        r = ipm_model.ipm_solve(qp, exact_nu=exact_nu, maxit=maxit)
    ok = bool(np.isfinite(r["gap"]) and r["gap"] < 1e-11 and r["rd"] < 1e-9 * max(1.0, np.abs(d["Qsel"]).max()) and r["re"] < 1e-9 and r["iters"] < maxit - 1)
    return ok, int(r["iters"])


def dist(a, b):
    return float(np.abs(a - b).max())


def study(g, names=tuple(ROWS), which=("lap4", "pid4"), idx=range(NPROB), model=True):
    """The CPU check of the rows: per store set, every row's QPs through the oracle (and the model), and the distances of FIELD_ROWS / SIX against their partner.
    Returns dict(cert=worst certificate, iters={row: (min, max)}, not_converged=[...], dist={(row, against): minimum over the problems and store sets})."""
    cert = 0.0; iters = {}; bad = []; dmin = {}
    for w in which:
        data = qp_data(g, w, idx)
        opt = {}
        for n in names:
            par = params(n)
            sols = [oracle_solve(par, d) for d in data]
            opt[n] = [s[0] for s in sols]; cert = max(cert, max(s[1] for s in sols))
            if model:
                for ex in (True, False):
                    for b, d in zip(idx, data):
                        ok, it = model_solve(par, d, ex)
                        lo, hi = iters.get(n, (it, it)); iters[n] = (min(lo, it), max(hi, it))
                        if not ok:
                            bad.append((w, n, b, ex, it))
        pairs = [(n, "R0") for n in names if n != "R0"] + [(n, "R5a") for n in ("R5", "R5b", "R5c") if n in names and "R5a" in names]
        for a, b_ in pairs:
            if b_ in opt:
                dm = min(dist(x, y) for x, y in zip(opt[a], opt[b_]))
                dmin[(a, b_)] = min(dmin.get((a, b_), np.inf), dm)
    return dict(cert=cert, iters=iters, not_converged=bad, dist=dmin)
