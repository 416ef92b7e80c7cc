"""tests/ss_table_cases.py -- the safe-set fixture, the problems and the references of the per-problem safe-set table tests (test infrastructure, not product).

Safe-set laps (cuts of the golden PID run that cross the finish line, and LMPC lap 4 of the golden flow):

  index  rows  what
    0    330   PID rows 0..329 (the line is crossed at row 305)
    1    345   PID rows 0..344
    2    237   LMPC lap 4, which ends at the line; extended past it by ss_extend_lap with the first 30 rows of LMPC lap 5 (267 rows stored)
    3    330   PID rows 5..334: the LapTime of lap 0
    4    320   PID rows 305..624, the second PID lap, s shifted back by TrackLength
    5    360   PID rows 0..359: slower than every other lap, the "other lap" of the references (see own_order)

Three different lengths and more, two equal LapTimes (0 and 3), one lap extended past the line (2).  The regression store of every context is the PID run four
times, as in the golden flow.

The reference of a table row is a context that holds ONLY that row's laps (with multiplicity), added in ascending index order, on which the shared rule is in
force.  Its latest lap is the last one added, so: `last` in the row -- that lap is added last instead (it must then be listed once and tie with no other lap of
the row, so that moving it does not change the stable argsort); `last` not in the row or -1 -- lap 5 is added behind the row's laps: it is the latest, it is no faster
than any of them and added last, hence never selected, and every entry takes the Qfun[it][0] branch.

Horizons.  problems(g, B, N) starts the six base problems at rows t = [100, 200, 308 - N, 311 - N, 150, 306] of the PID run (start_steps): the two problems whose
previous prediction crosses the line keep their terminal targets zt = xP[309] and xP[312] at every N, problem 5 stays the one wrap problem, and the others end
before the line at every built-in horizon (200 + 40 < 305).  tests/test_ss_table_host.py checks, for N in {8, 12, 14, 20, 40}, the crossing pattern, the single
wrap and that none of the 36 (problem, row) pairs of either row set raises LMPC_ST_WINDOW in the oracle; no horizon needed other steps.  ppl is 12 at every horizon.
"""
import numpy as np

N = 12
EXTRA = 5                       # the lap that is slower than all others
EXTENDED = 2                    # the lap that ss_extend_lap carries past the line

# six rows (numSS_it = 4): mixed lengths; a duplicate pair; the same laps in both orders (rows 2 and 3, with the tie 0 / 3); last in the row (rows 0, 2, 4, 5),
# named but not in the row (row 1), -1 (row 3)
ROWS4 = np.array([[0, 1, 2, 4], [1, 1, 3, 4], [3, 2, 1, 0], [0, 1, 2, 3], [0, 3, 4, 2], [2, 4, 4, 5]], np.int32)
LAST4 = np.array([4, 5, 2, -1, 2, 5], np.int32)
# the same for numSS_it = 2
ROWS2 = np.array([[0, 2], [1, 1], [3, 0], [0, 3], [4, 2], [2, 5]], np.int32)
LAST2 = np.array([2, 5, -1, 5, 2, 5], np.int32)


def fixture_laps(g):
    """[(x, u)] of laps 0..5 at their addTrajectory-time length, and the (x, u) rows that extend lap 2."""
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"]); TL = float(g["trackLength"])
    second = xP[305:625].copy(); second[:, 4] -= TL
    laps = [(xP[0:330], uP[0:330]), (xP[0:345], uP[0:345]), (np.array(g["lapx0"]), np.array(g["lapu0"])), (xP[5:335], uP[5:335]), (second, uP[305:625]), (xP[0:360], uP[0:360])]
    ext = (np.array(g["lapx1"])[0:30], np.array(g["lapu1"])[0:30])
    return [(np.ascontiguousarray(x), np.ascontiguousarray(u)) for x, u in laps], ext


def cpu_stored(g):
    """[(x, u, qfun, LapTime)] of the six laps as a context stores them after fill_table_context (what read_laps returns), computed by the oracle on the CPU:
    LMPC.computeCost per lap, and LMPC.addPoint for the rows that extend lap 2 (s + TrackLength, the Q-function counting down)."""
    from oracle import lmpc_oracle as orc
    TL = float(g["trackLength"])
    laps, ext = fixture_laps(g)
    stored = []
    for i, (x, u) in enumerate(laps):
        q = orc.compute_cost(x, TL); T0 = x.shape[0]
        if i == EXTENDED:
            assert x[-1, 4] <= TL
            xe = ext[0].copy(); xe[:, 4] += TL
            x = np.vstack([x, xe]); u = np.vstack([u, ext[1]]); q = np.concatenate([q, q[-1] - 1 - np.arange(xe.shape[0])])
        stored.append((x, u, q, T0))
    return stored


def fill_table_context(ctx, g):
    """Regression store and the six safe-set laps, lap 2 extended."""
    laps, ext = fixture_laps(g)
    for _ in range(4):
        ctx.model_add_trajectory(g["xPID"], g["uPID"])
    for x, u in laps:
        ctx.ss_add_trajectory(x, u)
    ctx.ss_extend_lap(EXTENDED, ext[0], ext[1])


def start_steps(N=N):
    """Start rows of the six base problems in the golden PID run at horizon N."""
    return [100, 200, 308 - N, 311 - N, 150, 306]


def problems(g, B=6, N=N):
    """B problems of horizon N (12: the arrays of the N = 12 tests), the six base problems cycled: hasPred = 1 everywhere, timeStep != 0; xPredPrev crosses the line
    for problems 2, 3 and 5 and not for 0, 1 and 4; problem 5 starts just behind the line with zt still counted in the lap before, the wrap branch (:392-394)."""
    xP, uP = np.array(g["xPID"]), np.array(g["uPID"]); TL = float(g["trackLength"])
    t = np.array(start_steps(N))[np.arange(B) % 6]
    x0 = xP[t].copy(); xLin = np.stack([xP[k + 1:k + N + 2] for k in t]); uLin = np.stack([uP[k + 1:k + N + 1] for k in t])
    zt = xP[t + N + 1].copy(); xPredPrev = np.stack([xP[k:k + N + 1] for k in t])
    wrap = t == 306
    x0[wrap, 4] -= TL; xLin[wrap, :, 4] -= TL
    return dict(x0=x0, xLin=xLin, uLin=uLin, uOld=uP[t].copy(), zt=zt, xPredPrev=xPredPrev, hasPred=np.ones(B, np.int32), timeStep=(t % 97 + 3).astype(np.int32))


def own_order(row, last, laptime, extra=EXTRA):
    """The laps of the reference context of (row, last), in the order they are added.  extra: the lap that is slower than all others (lap 5 of this fixture)."""
    row = [int(l) for l in row]; last = int(last)
    order = sorted(row)
    if last in row:
        assert row.count(last) == 1 and sum(laptime[l] == laptime[last] for l in row) == 1, (row, last)
        order.remove(last); order.append(last)
    else:
        # (lap 5 may itself be in the row: the copy added behind it ties with it, and the stable argsort selects the copies added first)
        assert all(laptime[l] <= laptime[extra] for l in row), (row, last)
        order.append(extra)
    return order


def read_laps(ctx):
    """[(x, u, qfun, LapTime)] of every safe-set lap of ctx as stored now."""
    return [ctx.store_read_lap(1, l) + (ctx.ss_lap_time(l),) for l in range(ctx.ss_num_laps())]


def fill_own_context(own, g, stored, order):
    """The regression store, and the laps `order` of `stored` (read_laps of the table context) with their current rows and Q-function, as restore_stores installs them."""
    for _ in range(4):
        own.model_add_trajectory(g["xPID"], g["uPID"])
    for i, l in enumerate(order):
        x, u, q, T0 = stored[l]
        own.ss_add_trajectory(x[:T0], u[:T0])
        own.ss_replace_lap(i, x, u, q)


def window_ok(stored, order, p, b, TL, numSS_it, ppl):
    """The oracle's window rule for problem b of `p` on the laps `order`: the ppl + 1 rows selected around zt lie inside every lap used (the reference's
    IndexError, :497; LMPC_ST_WINDOW where it does not hold)."""
    SS = [stored[l][0] for l in order]; LapTime = [stored[l][3] for l in order]
    z = p["zt"][b].copy()
    if z[4] - p["x0"][b][4] > TL / 2:
        z[4] = np.max([z[4] - TL, 0])
    srt = np.argsort(np.array(LapTime), kind="stable")
    ok = True
    for jj in srt[0:numSS_it]:
        d = SS[jj] - z[None, :]
        nrm = np.abs(d[:, 0])
        for j in range(1, 6):
            nrm = nrm + np.abs(d[:, j])
        m = int(np.argmin(nrm)); npw = ppl + 1
        start = m - npw // 2 if m - npw / 2 >= 0 else m
        ok = ok and start + npw <= SS[jj].shape[0]
    return ok


def oracle_selection(stored, order, p, b, TL, numSS_it, ppl, N=N):
    """oracle.terminal_components for problem b of `p` on the laps `order`, sortedLapTime and cur_it per car: (SSsel.T, Qsel, Succ.T, SuccU.T, window ok)."""
    from oracle import lmpc_oracle as orc
    SS = [stored[l][0] for l in order]; uSS = [stored[l][1] for l in order]; Qf = [stored[l][2] for l in order]; LapTime = [stored[l][3] for l in order]
    z = p["zt"][b].copy()
    if z[4] - p["x0"][b][4] > TL / 2:
        z[4] = np.max([z[4] - TL, 0])
    srt = np.argsort(np.array(LapTime), kind="stable")
    ok = window_ok(stored, order, p, b, TL, numSS_it, ppl)
    xPrev = p["xPredPrev"][b] if p["hasPred"][b] else None
    SSsel, Qsel, Succ, SuccU = orc.terminal_components(SS, uSS, Qf, LapTime, z, ppl * numSS_it, numSS_it, xPrev, len(order), int(p["timeStep"][b]), N, TL, sortedLapTime=srt)
    return SSsel.T, Qsel, Succ.T, SuccU.T, ok
