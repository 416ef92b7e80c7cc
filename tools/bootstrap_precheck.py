"""CPU only: the three stages of rollout.bootstrap (main.py:61-95 for B cars) driven by the oracle alone, on the very draws bootstrap(track, B, N, vt, seed,
max_steps=...) feeds the device -- PID control-law noise (T, B, 2), PID plant noise, LTI-MPC plant noise, LTV-MPC plant noise (T, B, 3 each) from one
default_rng(seed).  Per car: oracle PID loop -> oracle.lti_regression -> LTI-MPC loop (assemble_mpc_qp + osqp_solve_exact + dyn_model) -> LTV-MPC loop on the
shared store of the min(B, 4) PID laps (compute_ltv_dynamics).  Prints, per stage, the row at which every car first has s > TrackLength and the largest |ey|:
the values of vt, seed and max_steps used by tests/test_gpu_mpc_stages.py::test_bootstrap_end_to_end were chosen with it.

    python tools/bootstrap_precheck.py --cars 16 --vt 0.8 --seed 9 --steps 1000 --sim-steps 400
"""
import argparse
import os
os.environ.setdefault("OMP_NUM_THREADS", "1"); os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")     # one thread per worker process
import json
import multiprocessing as mp
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
J = {}
X0 = np.array([0.5, 0, 0, 0, 0, 0.0])


def _pid(b):
    from oracle import lmpc_oracle as orc
    x, xg, X, U = X0.copy(), X0.copy(), [], []
    for t in range(J["T"]):
        nu = J["nu"][t, b]
        u = np.array([-0.6 * x[5] - 0.9 * x[3] + np.clip(nu[0] * 0.25, -0.9, 0.9), 1.5 * (J["vt"] - x[0]) + np.clip(nu[1] * 0.10, -0.2, 0.2)])
        X.append(x); U.append(u)
        it = iter(J["nz"][0][t, b])
        x, xg = orc.dyn_model(J["pt"], x, xg, u, lambda: next(it))
    return np.array(X), np.array(U)


def _mpc(job):
    from oracle import lmpc_oracle as orc
    b, ltv = job
    par, pt, N = J["par"], J["pt"], J["N"]
    x, xg, uOld, X, st = X0.copy(), X0.copy(), np.zeros(2), [], 0
    if ltv:
        xS = [J["pid"][i][0] for i in J["store"]]; uS = [J["pid"][i][1] for i in J["store"]]
        xLin, uLin = xS[-1][0:N + 1].copy(), uS[-1][0:N].copy()
    else:
        A, Bm, _ = orc.lti_regression(J["pid"][b][0], J["pid"][b][1], 0.0000001)
    for t in range(J["T"]):
        if ltv:
            A, Bm, C = orc.compute_ltv_dynamics(xS, uS, list(range(len(xS))), pt, xLin, uLin, N)
            P, q, Ao, lo, up = orc.assemble_mpc_qp(par, A, Bm, C, x, uOld)
        else:
            P, q, Ao, lo, up = orc.assemble_mpc_qp(par, A, Bm, None, x, uOld)
        ex, cert = orc.osqp_solve_exact(P, q, Ao, lo, up, want=1e-8)
        st += int(cert > 1e-6)
        xP = ex.x[:6 * (N + 1)].reshape(N + 1, 6); uP = ex.x[6 * (N + 1):6 * (N + 1) + 2 * N].reshape(N, 2)
        u = uP[0].copy(); X.append(x)
        it = iter(J["nz"][2 if ltv else 1][t, b])
        x, xg = orc.dyn_model(pt, x, xg, u, lambda: next(it))
        if ltv:
            xLin = np.vstack([xP[1:], xP[N]]); uLin = np.vstack([uP[1:], uP[N - 1]])
        uOld = u
    return np.array(X), st


def _report(name, laps, TL):
    done = [int(np.argmax(x[:, 4] > TL)) if np.any(x[:, 4] > TL) else -1 for x in laps]
    ey = max(float(np.abs(x[:, 5]).max()) for x in laps)
    print(json.dumps(dict(stage=name, first_row_past_the_line=done, all_finished=all(d > 0 for d in done), max_abs_ey=ey, min_vx=min(float(x[:, 0].min()) for x in laps))), flush=True)
    return all(d > 0 for d in done) and ey < 2.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cars", type=int, default=16); ap.add_argument("--vt", type=float, default=0.8); ap.add_argument("--seed", type=int, default=9)
    ap.add_argument("--steps", type=int, default=1000); ap.add_argument("--N", type=int, default=12); ap.add_argument("--procs", type=int, default=8)
    ap.add_argument("--sim-steps", type=int, default=0, help="simulate only the first n of the --steps steps (the draws stay those of --steps)")
    a = ap.parse_args()
    from oracle import lmpc_oracle as orc
    from tests import common
    orc.build_lib()
    g = common.load_lmpc_golden()
    pt = np.array(g["track"]); TL = float(g["trackLength"]); B, T = a.cars, a.steps
    rng = np.random.default_rng(a.seed)
    nu = rng.standard_normal((T, B, 2)); nz = [rng.standard_normal((T, B, 3)) for _ in range(3)]
    J.update(T=a.sim_steps or T, vt=a.vt, nu=nu, nz=nz, pt=pt, N=a.N, par=orc.QPParams.mpc_default(a.N, a.vt), store=list(range(min(B, 4))))
    with mp.get_context("fork").Pool(a.procs) as pool:
        J["pid"] = pool.map(_pid, range(B))
    ok = _report("pid", [l[0] for l in J["pid"]], TL)
    with mp.get_context("fork").Pool(a.procs) as pool:
        res = pool.map(_mpc, [(b, False) for b in range(B)] + [(b, True) for b in range(B)], chunksize=1)
    ok = _report("mpc", [r[0] for r in res[:B]], TL) and ok
    ok = _report("ltvmpc", [r[0] for r in res[B:]], TL) and ok
    print(json.dumps(dict(cars=B, vt=a.vt, seed=a.seed, steps=T, uncertified_qps=int(sum(r[1] for r in res)), ok=bool(ok))))


if __name__ == "__main__":
    main()
