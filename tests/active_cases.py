"""Test infrastructure: the hard-problem fixture tests/golden/lmpc_active.npz (made by tests/golden/make_active_golden.py) as the tests read it.

The fixture holds QPs whose optimum has ACTIVE inequality rows -- lane slacks above zero, steering at +-0.5 -- for every built horizon, with the oracle's certified
optimum next to each, so that a test on the GPU box compares every solve route with an optimum without solving anything there:

  * stores: the four fastest complete laps (fewest rows; ties by age) of the oracle's restatement of the reference flow at N = 12, seed 5, 30 laps
    (closed_loop.OracleFlow(g, 12, "osqp")): 155, 157, 161 and 163 rows, vx up to 2.9, |ey| up to 0.37.  They serve as regression store and as safe set,
    in this order (LapTime = rows, Q-function = compute_cost of the rows, as for every lap handed to addTrajectory).
  * directed problems, per horizon N in HORIZONS: x0 = row t of the 155-row lap plus the offset of a family, linearisation = the rows that follow
    (xLin = rows t + 1 .. t + N + 1, uLin = rows t + 1 .. t + N: not stored, `directed_inputs` takes them from the lap), uOld = the input of row t,
    zt = row t + N + 1, timeStep = t -- bench.synth_batch with a directed offset instead of noise.
  * closed-loop records at N = 12 and N = 14: QPs the reference flow itself met in its last ten laps, as A, B, C, x0, uOld, SS, Qsel and the optimum.

What is stored per directed problem and what is recomputed: the inputs and the optimum z* = (x, u, slack, lambda, sTerm) of every problem; the oracle's A, B, C and
selection (SSsel, Qsel, Succ, SuccU) only of the problems listed in n<N>_k1 -- no committed file may exceed 1 MiB, and regression and selection cost the oracle a
millisecond per horizon point, so the tests recompute them (`oracle_records`, the very call that made the fixture) and tests/test_oracle_golden.py pins the stored
sample, and the optimum of a handful per horizon, bit for bit.
"""
import os

import numpy as np

from tests import common

HORIZONS = (8, 12, 14, 20, 40)
CL_HORIZONS = (12, 14)
FAMILIES = ("none", "ey+", "ey-", "epsi+", "epsi-", "vx-", "vywz+")
#                     vx    vy   wz   epsi  s    ey
OFFSETS = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                    [0.0, 0.0, 0.0, 0.0, 0.0, 0.12],
                    [0.0, 0.0, 0.0, 0.0, 0.0, -0.12],
                    [0.0, 0.0, 0.0, 0.35, 0.0, 0.0],
                    [0.0, 0.0, 0.0, -0.35, 0.0, 0.0],
                    [-0.8, 0.0, 0.0, 0.0, 0.0, 0.0],
                    [0.0, 0.1, 1.0, 0.0, 0.0, 0.0]])
# Start rows on the 155-row lap, inside 5 .. 113 - N.  Chosen from a scan of every row x family with the oracle so that each horizon holds enough problems with an
# active lane slack, with an input at a bound, with both and with neither (the minima the generator asserts): rows 30..32 are where the lap runs along the lane edge
# (|ey| 0.37: an ey or epsi offset pushes the prediction over it), 57..59 and 74..79 the next two corners; at N = 40 every row but 9..11 has both kinds active.
START_ROWS = {8: (30, 31, 32, 58, 77, 105), 12: (5, 30, 31, 32, 77, 98), 14: (5, 30, 31, 57, 79, 99), 20: (5, 30, 31, 32, 58, 74), 40: (5, 10, 30, 46, 59, 73)}
ACTIVE_SLACK = 1e-6       # a lane row counts as active when its slack s* exceeds this
AT_BOUND = 1e-7            # a step counts as input-bound when |u| is within this of a bound
PATH = os.path.join(common.GOLDEN, "lmpc_active.npz")


def load():
    return dict(np.load(PATH))


def laps(f):
    return [(f["lapx%d" % i], f["lapu%d" % i]) for i in range(4)]


def directed_inputs(lap_list, N, t, fam):
    """The step inputs of the directed problems (t[i], family fam[i]) at horizon N on the query lap lap_list[0]."""
    xq, uq = lap_list[0]
    t = np.asarray(t, int); fam = np.asarray(fam, int)
    return dict(x0=xq[t] + OFFSETS[fam], xLin=np.stack([xq[a + 1:a + N + 2] for a in t]), uLin=np.stack([uq[a + 1:a + N + 1] for a in t]),
                uOld=uq[t].copy(), zt=xq[t + N + 1].copy(), timeStep=t.astype(np.int32))


def fixture_inputs(f, N):
    """directed_inputs of the fixture's problems at horizon N; x0, uOld, zt and timeStep are stored as well and must be the same bits."""
    inp = directed_inputs(laps(f), N, f["n%d_t" % N], f["n%d_fam" % N])
    for k in ("x0", "uOld", "zt", "timeStep"):
        assert np.array_equal(inp[k], f["n%d_%s" % (N, k)]), (N, k)
    return inp


def oracle_records(f_or_laps, N, inp, idx, solve=False, procs=None):
    """The oracle on problems idx of inp (tests/oracle_pool: regression, selection and, with solve, both certified optima), stores = the fixture's laps."""
    from oracle import lmpc_oracle as orc
    from tests import oracle_pool
    g = common.load_lmpc_golden()
    lap_list = laps(f_or_laps) if isinstance(f_or_laps, dict) else f_or_laps
    idx = list(idx)
    return oracle_pool.oracle_batch(orc.QPParams.lmpc_default(N), np.array(g["track"]), float(g["trackLength"]), lap_list, N, inp, idx,
                                    solve_idx=idx if solve else (), procs=procs)


def split(z, N, S=48):
    """(x (N + 1, 6), u (N, 2), slack (2N,), lambda (S,), sTerm (6,)) of a solution vector in the reference's order."""
    a = 6 * (N + 1); b = a + 2 * N; c = b + 2 * N; d = c + S
    return z[:a].reshape(N + 1, 6), z[a:b].reshape(N, 2), z[b:c], z[c:d], z[d:d + 6]


def active_counts(z, N):
    """(lane rows with s* > ACTIVE_SLACK, steps with steering or acceleration within AT_BOUND of a bound) at the optimum z."""
    _, u, s, _, _ = split(z, N)
    at = (np.abs(np.abs(u[:, 0]) - 0.5) <= AT_BOUND) | (np.abs(np.abs(u[:, 1]) - 10.0) <= AT_BOUND)
    return int((s > ACTIVE_SLACK).sum()), int(at.sum())


def xu_err(x, u, xs, us):
    """Scaled distance common.TOL_XU bounds: max |xu - z*| / (1 + |z*|)."""
    return float(max((np.abs(x - xs) / (1 + np.abs(xs))).max(), (np.abs(u - us) / (1 + np.abs(us))).max()))


def scaled_err(a, ref):
    return float((np.abs(a - ref) / (1 + np.abs(ref))).max())


def admitted(r, N):
    """The fixture's admission rule on an oracle record with both optima: the two solvers agree on (x, u) to 1e-9 (1 + |z*|), both certificates <= 1e-8."""
    n = 6 * (N + 1) + 2 * N
    return bool(scaled_err(r["opt2"][:n], r["opt"][:n]) <= 1e-9 and r["cert"] <= 1e-8 and r["cert2"] <= 1e-8)


def lambda_unique(r, N, S=48):
    """Succ lambda* is a function of the QP alone as far as the oracle can tell: its two methods agree on it to 1e-7 (common.compare_with_oracle's rule)."""
    n = 6 * (N + 1) + 4 * N
    a, b = r["opt"][n:n + S], r["opt2"][n:n + S]
    return bool(common.zt_err(r["Succ"] @ a, r["SuccU"] @ a, r["Succ"], r["SuccU"], b) < 1e-7)
