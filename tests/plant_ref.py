"""High-precision restatement of the plant (oracle.lmpc_oracle.dyn_model = Simulator.dynModel, SysModel.py:56-147) and the state families
the plant / track-lookup tests run on (tests/test_gpu_plant_track.py, tests/test_oracle_golden.py).

dyn_model_ld integrates every car of a batch at once in np.longdouble: the same 100 Euler sub-steps, the same curvature lookup (the wrap
`while s > TrackLength` and the segment test `c0 <= s < c0 + len` of Track.py:292-310, made in float64 on s rounded to float64 as the oracle
makes it), the same noise clipping.  Where the oracle would raise (s on no segment) or never return (its wrap loop on an infinite s) the car
is flagged and integrated on with curvature 0; its state means nothing then.  `wraps` is the largest number of wraps any sub-step of the car
needed: the device kernels bound that loop (64 laps in the plant and the regression, 4096 in the global position, see track_curvature).

Every family is built from the track table, the track length and the golden PID lap; nothing here reads a fixture of its own."""
import numpy as np

LD = np.longdouble
PLANT_WRAP_BOUND = 64            # lmpc_kernels.hip.h, track_curvature / plant_curvature
GLOBAL_WRAP_BOUND = 4096         # lmpc_kernels.hip.h, lmpc_global_position_kernel
_HANG_LAPS = 1 << 20             # beyond this the oracle's wrap loop is as good as endless (s = inf never returns)


def _substeps():
    i, deltaT, dt = 0, 0.001, 0.1
    while (i + 1) * deltaT <= dt:            # the oracle's loop condition, evaluated in float64
        i += 1
    return i


N_SUB = _substeps()


def wrap_f64(pt, s):
    """Vectorised `while s > TrackLength: s = s - TrackLength` in float64.  Returns (wrapped s, wraps needed, hang): hang marks an s the
    loop could never finish (non-finite or absurdly far)."""
    TL = pt[-1, 3] + pt[-1, 4]
    s = np.array(s, dtype=np.float64, copy=True)
    n = np.zeros(s.shape, np.int64)
    hang = ~np.isfinite(s) & (s > 0) | (s > TL * _HANG_LAPS)
    act = (s > TL) & ~hang
    while act.any():
        s[act] = s[act] - TL
        n[act] += 1
        act = (s > TL) & ~hang
    return s, n, hang


def wrap_threshold(pt, k):
    """The smallest float64 s whose wrap needs k subtractions (the float64 loop rounds: it is not k TL - TL to the last bit)."""
    TL = pt[-1, 3] + pt[-1, 4]
    lo, hi = (int(v) for v in np.array([(k - 0.5) * TL, (k + 0.5) * TL]).view(np.int64))
    while hi - lo > 1:                                  # positive floats are ordered like their bit patterns
        mid = (lo + hi) // 2
        if wrap_f64(pt, np.array([mid], np.int64).view(np.float64))[1][0] >= k:
            hi = mid
        else:
            lo = mid
    return float(np.array([hi], np.int64).view(np.float64)[0])


def segment_of(pt, s):
    """Index of the segment with c0 <= s < c0 + len (float64 comparisons), -1 where there is none."""
    c0 = pt[:, 3]; c1 = pt[:, 3] + pt[:, 4]
    hit = (s[..., None] >= c0) & (s[..., None] < c1)
    idx = np.where(hit.any(-1), hit.argmax(-1), -1)
    return idx


def curvature_lookup(pt, s):
    """Map.curvature for an array of s: (curvature, no-segment flag, wraps needed).  Decisions are the oracle's float64 ones."""
    s64 = np.asarray(s, dtype=np.float64)
    sw, n, hang = wrap_f64(pt, s64)
    idx = segment_of(pt, sw)
    bad = (idx < 0) | hang
    cur = np.where(bad, 0.0, pt[np.maximum(idx, 0), 5])
    return cur, bad, n


def dyn_model_ld(pt, x, xg, u, nz):
    """x, xg (B, 6), u (B, 2), nz (B, 3) -> (xn, xgn (B, 6) longdouble, raise (B,), wraps (B,)): raise = the oracle raises or never returns."""
    x = np.asarray(x, np.float64); xg = np.asarray(xg, np.float64); u = np.asarray(u, np.float64); nz = np.asarray(nz, np.float64)
    m = LD(1.98); lf = LD(0.125); lr = LD(0.125); Iz = LD(0.024)
    Df = LD(0.8 * 1.98 * 9.81 / 2.0); Cf = LD(1.25); Bf = LD(1.0)
    deltaT = LD(0.001)
    delta, a = u[:, 0].astype(LD), u[:, 1].astype(LD)
    sd, cd = np.sin(delta), np.cos(delta)
    vx, vy, wz, epsi, s, ey = (x[:, j].astype(LD) for j in range(6))
    psi, X, Y = (xg[:, j].astype(LD) for j in (3, 4, 5))
    raised = np.zeros(x.shape[0], bool); wraps = np.zeros(x.shape[0], np.int64)
    with np.errstate(all="ignore"):
        for _ in range(N_SUB):
            alpha_f = delta - np.arctan2(vy + lf * wz, vx)
            alpha_r = -np.arctan2(vy - lf * wz, vx)
            Fyf = Df * np.sin(Cf * np.arctan(Bf * alpha_f))
            Fyr = Df * np.sin(Cf * np.arctan(Bf * alpha_r))
            nvx = vx + deltaT * (a - 1 / m * Fyf * sd + wz * vy)
            nvy = vy + deltaT * (1 / m * (Fyf * cd + Fyr) - wz * vx)
            nwz = wz + deltaT * (1 / Iz * (lf * Fyf * cd - lr * Fyr))
            npsi = psi + deltaT * wz
            nX = X + deltaT * (vx * np.cos(psi) - vy * np.sin(psi))
            nY = Y + deltaT * (vx * np.sin(psi) + vy * np.cos(psi))
            cur, bad, n = curvature_lookup(pt, s)
            raised |= bad; wraps = np.maximum(wraps, n)
            cur = cur.astype(LD)
            q = (vx * np.cos(epsi) - vy * np.sin(epsi)) / (1 - cur * ey)
            nepsi = epsi + deltaT * (wz - q * cur)
            ns = s + deltaT * q
            ney = ey + deltaT * (vx * np.sin(epsi) + vy * np.cos(epsi))
            vx, vy, wz, epsi, s, ey, psi, X, Y = nvx, nvy, nwz, nepsi, ns, ney, npsi, nX, nY
        clip = lambda v: np.maximum(-0.05, np.minimum(v, 0.05))          # np.max([-0.05, np.min([v, 0.05])]) of the oracle
        n0, n1, n2 = clip(nz[:, 0] * 0.01), clip(nz[:, 1] * 0.01), clip(nz[:, 2] * 0.005)
        xn = np.stack([vx + LD(0.01) * n0.astype(LD), vy + LD(0.01) * n1.astype(LD), wz + LD(0.01) * n2.astype(LD), epsi, s, ey], 1)
    xgn = np.stack([vx, vy, wz, psi, X, Y], 1)
    return xn, xgn, raised, wraps


def oracle_step(pt, x, xg, u, nz):
    """orc.dyn_model on one car: (xn, xgn) or None where it raises."""
    from oracle import lmpc_oracle as orc
    it = iter(nz)
    try:
        with np.errstate(all="ignore"):
            return orc.dyn_model(pt, x, xg, u, lambda: next(it))
    except ValueError:
        return None


def scaled_err(got, ref):
    """max |got - ref| / (1 + |ref|) per car (rows), computed in longdouble; NaN / inf pairs count as equal when both are the same."""
    got = np.asarray(got, LD); ref = np.asarray(ref, LD)
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(all="ignore"):
        e = np.abs(got - ref) / (1 + np.abs(ref))
    e = np.where(same, 0, e)
    e = np.where(np.isnan(e), np.inf, e)
    return e.reshape(e.shape[0], -1).max(1).astype(np.float64)


# --------------------------------------------------------------------------------------------------------------------------
# The kernel's guard predicates (plant_step_duo), evaluated on a state as the kernel evaluates them at its first sub-step
# --------------------------------------------------------------------------------------------------------------------------
def tyre_fast(x, u):
    """(front, rear) booleans: vx > 0 && |yq| <= vx && |B alpha| <= 1 && |C atan(B alpha)| <= 1 -- the polynomial path of each tyre."""
    lf = 0.125
    vx, vy, wz = x[:, 0], x[:, 1], x[:, 2]
    out = []
    with np.errstate(all="ignore"):
        for role in (0, 1):
            yq = vy - lf * wz if role else vy + lf * wz
            at = np.arctan(yq / vx)
            alpha = -at if role else u[:, 0] - at
            xs = 1.25 * np.arctan(alpha)
            out.append((vx > 0.0) & (np.abs(yq) <= vx) & (np.abs(alpha) <= 1.0) & (np.abs(xs) <= 1.0))
    return out


def heading_fast(x, xg):
    """(psi, epsi): |angle| < 1e5 -- the Cody-Waite reduction; else the ocml sin / cos."""
    return np.abs(xg[:, 3]) < 1.0e5, np.abs(x[:, 3]) < 1.0e5


def guard_counts(x, xg, u):
    """{guard: (fast, fallback)} on the initial states."""
    f, r = tyre_fast(x, u); hp, he = heading_fast(x, xg)
    out = {"front tyre": f, "rear tyre": r, "psi": hp, "epsi": he}
    return {k: (int(v.sum()), int((~v).sum())) for k, v in out.items()}


# --------------------------------------------------------------------------------------------------------------------------
# State families
# --------------------------------------------------------------------------------------------------------------------------
class Family:
    """x, xg (n, 6), u (n, 2), nz (n, 3).  judges: which references decide ("ld": dyn_model_ld, "oracle": orc.dyn_model).  smooth: the
    longdouble reference must agree with the oracle to 1e-13 (no float64 decision or cancellation of the oracle in the way)."""

    def __init__(self, name, x, xg, u, nz, judges, smooth, note=""):
        self.name, self.x, self.xg, self.u, self.nz = name, np.asarray(x, float), np.asarray(xg, float), np.asarray(u, float), np.asarray(nz, float)
        self.judges, self.smooth, self.note = judges, smooth, note

    def __len__(self):
        return self.x.shape[0]


def den_rounding_bound(pt, x, xn):
    """What float64 may lose against the longdouble reference through 1 - cur ey alone: the product cur ey is rounded (2^-53 |cur ey|) before
    a subtraction that cancels to |den|, and the step's travel (|xn - x|, the quotient's share of it) scales with 1 / den -- per car, in the
    units of the scaled error."""
    cur = pt[np.maximum(segment_of(pt, x[:, 4]), 0), 5]
    den = 1 - cur * x[:, 5]
    with np.errstate(all="ignore"):
        rel = 2.0 ** -53 * np.abs(cur * x[:, 5]) / np.abs(den)
        return (rel * np.abs(np.asarray(xn, np.float64) - x).max(1) / (1 + np.abs(x).min(1))).astype(np.float64)


def _nb(v):
    """v and its float64 neighbours (nextafter on both sides)."""
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


def families(g, n_lmpc=300, seed=2026):
    pt = np.array(g["track"]); TL = float(g["trackLength"])
    assert TL == pt[-1, 3] + pt[-1, 4]
    xP, uP, gP = np.asarray(g["xPID"]), np.asarray(g["uPID"]), np.asarray(g["xPID_glob"])
    rng = np.random.default_rng(seed)
    c0 = pt[:, 3]; ln = pt[:, 4]; cur = pt[:, 5]
    arcs_p, arcs_n, straights = np.where(cur > 0)[0], np.where(cur < 0)[0], np.where(cur == 0)[0]
    fams = []

    def base(n, vx=0.8, s=None, ey=0.0, epsi=0.0):
        x = np.zeros((n, 6)); x[:, 0] = vx; x[:, 3] = epsi; x[:, 5] = ey
        x[:, 4] = 3.0 if s is None else s
        xg = np.zeros((n, 6)); xg[:, :3] = x[:, :3]; xg[:, 3] = 0.3; xg[:, 4] = 1.0; xg[:, 5] = -0.5
        return x, xg

    def noise(n):
        return rng.standard_normal((n, 3))

    # ---- LMPC regime: vx 0.5-3.5, |vy| <= 0.5, |wz| <= 3, |epsi| <= 0.5, |ey| <= 0.6 on straights and on arcs of both signs ----
    n = n_lmpc
    seg = np.concatenate([straights, arcs_p, arcs_n])[rng.integers(0, len(pt), n)]
    seg[: n // 3] = straights[rng.integers(0, len(straights), n // 3)]
    seg[n // 3: 2 * n // 3] = arcs_p[rng.integers(0, len(arcs_p), n // 3)]
    seg[2 * n // 3:] = arcs_n[rng.integers(0, len(arcs_n), n - 2 * (n // 3))]
    x = np.stack([rng.uniform(0.5, 3.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-3, 3, n), rng.uniform(-0.5, 0.5, n),
                  c0[seg] + ln[seg] * rng.uniform(0.02, 0.98, n) + TL * rng.integers(0, 3, n), rng.uniform(-0.6, 0.6, n)], 1)
    xg = np.concatenate([x[:, :3], (rng.uniform(-np.pi, np.pi, n) + 2 * np.pi * rng.integers(-3, 4, n))[:, None], rng.uniform(-5, 5, (n, 2))], 1)
    u = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-10, 10, n)], 1)
    fams.append(Family("lmpc regime", x, xg, u, noise(n), ("ld", "oracle"), True))

    # ---- tyre-force fallbacks ----
    rows = []                                                     # (vx, vy, wz, delta, a)
    for vy, wz in ((1.2, 0.0), (-1.2, 0.0), (0.5, 6.0), (0.3, -8.0), (0.9, 1.0), (-0.9, -1.0)):
        rows.append((1.0, vy, wz, 0.1, 1.0))                    # sliding: |vy +- lf wz| > vx
    for vx in (0.0, -0.0, -0.5, -1e-8):                          # vx <= 0, signed zeros: atan2 at its branch cut and at the origin
        for vy in (0.0, -0.0):
            for wz in (0.0, -0.0):
                rows.append((vx, vy, wz, 0.0, 0.0))
        rows.append((vx, 0.0, 0.0, 0.3, 1.0)); rows.append((vx, 0.05, -0.2, -0.3, 0.0))
    for vx in (1e-8, 3e-9, 1e-7):                                # vx around 1e-8
        rows.append((vx, 0.0, 0.0, 0.0, 1.0)); rows.append((vx, 0.0, 0.0, 0.2, 0.5)); rows.append((vx, 1e-9, 0.0, 0.0, 0.0))
    for d in (1.0, -1.0, 0.9, -0.7):                             # |delta - atan(.)| > 1, as the PID inputs reach
        rows.append((0.6, 0.0, 0.0, d, 0.5)); rows.append((0.6, 0.2, 0.5, d, -1.0))
    for v in _nb(1.0):                                           # |yq| = vx: just inside, on, just outside (both tyres: wz = 0)
        rows.append((1.0, v, 0.0, 0.0, 0.0)); rows.append((1.0, -v, 0.0, 0.0, 0.0))
        rows.append((2.0, 2 * v, 0.0, 0.0, 0.0))
    vxq, wzq = 1.0, 4.0                                          # front yq = vy + lf wz = vx, rear below it
    for v in _nb(vxq - 0.125 * wzq):
        rows.append((vxq, v, wzq, 0.0, 0.0))
    for d in _nb(1.0) + [-d for d in _nb(1.0)]:                  # |B alpha_f| = 1 (yq = 0 -> alpha_f = delta)
        rows.append((0.7, 0.0, 0.0, d, 0.0))
    r = np.array(rows, float)
    x, xg = base(len(r), s=3.0, ey=0.1)
    x[:, 0:3] = r[:, 0:3]; xg[:, 0:3] = r[:, 0:3]
    fams.append(Family("tyre fallbacks", x, xg, r[:, 3:5], noise(len(r)), ("ld", "oracle"), True))

    # ---- headings: psi / epsi at odd multiples of pi / 4 (+- 1 ulp), 2 pi k up to 40 laps, 1e3, 1e5 (+- 1 ulp), 1e7 ----
    angs = []
    for k in (1, 3, 5, 7, -1, -3, -5, -7, 9, 15, 41, -63):
        angs += _nb(k * np.pi / 4)
    angs += [2 * np.pi * k for k in (1, 2, 5, 13, 27, 40, -40)]
    angs += [1e3, -1e3] + _nb(1e5) + [-a for a in _nb(1e5)] + [1e7, -1e7]
    angs = np.array(angs)
    na = len(angs)
    x, xg = base(2 * na, vx=1.5, s=0.5, ey=0.05)
    x[:, 1] = 0.1; x[:, 2] = 0.4; xg[:, 0:3] = x[:, 0:3]
    xg[:na, 3] = angs; x[:na, 3] = 0.2                           # psi family
    x[na:, 3] = angs; xg[na:, 3] = 0.3                           # epsi family (on a straight: no curvature term)
    u = np.tile([0.05, 0.5], (2 * na, 1))
    big = np.abs(np.concatenate([angs, angs])) > 1.5e3           # float64 rounding of psi + dt wz: the longdouble state drifts off
    fams.append(Family("headings", x[~big], xg[~big], u[~big], noise(int((~big).sum())), ("ld", "oracle"), True))
    fams.append(Family("headings large", x[big], xg[big], u[big], noise(int(big.sum())), ("oracle",), False,
                       "|angle| > 1.5e3: the state rounds psi to float64 every sub-step, the oracle is the judge"))

    # ---- track position: segment starts +- 1 ulp, k TL +- 1 ulp (k = 1..5), TL, s < 0, -0.0, around the 65th wrap; forward and backward ----
    svals = []
    for c in c0[1:]:
        svals += _nb(c)
    svals += [0.0, -0.0, np.nextafter(0.0, 1.0), -1e-3, -5.0, TL]
    for k in range(1, 6):
        svals += _nb(k * TL)
    svals += [65 * TL] + _nb(wrap_threshold(pt, PLANT_WRAP_BOUND + 1)) + [64.5 * TL, 65.5 * TL]   # 64 wraps still land, 65 do not
    svals = np.array(svals)
    ns = len(svals)
    x, xg = base(2 * ns, vx=0.8, s=np.concatenate([svals, svals]), ey=0.2)
    x[ns:, 3] = np.pi                                            # epsi = pi: s decreases
    x[:, 1] = 0.02; xg[:, 1] = 0.02
    u = np.tile([0.1, 0.3], (2 * ns, 1))
    fams.append(Family("track position", x, xg, u, noise(2 * ns), ("oracle", "ld"), False))

    # ---- crossings inside one step: segment boundaries and k TL, forward at vx = 3 and backward (epsi = pi, or vx < 0) ----
    bnd = list(c0[1:]) + [k * TL for k in range(1, 6)]
    rows = []
    for b in bnd:
        rows.append((3.0, 0.0, b - 0.15)); rows.append((3.0, np.pi, b + 0.15))
    for b in (c0[2], TL, 2 * TL, 4 * TL):
        rows.append((-1.0, 0.0, b + 0.05))                      # vx < 0: backward through the fallback tyre path
    rows.append((3.0, np.pi, 0.15))                              # backward across s = 0: the oracle raises mid-step
    r = np.array(rows)
    x, xg = base(len(r), s=r[:, 2], ey=0.1)
    x[:, 0] = r[:, 0]; x[:, 3] = r[:, 1]; xg[:, 0] = r[:, 0]
    u = np.tile([0.0, 0.2], (len(r), 1))
    fams.append(Family("crossings", x, xg, u, noise(len(r)), ("oracle", "ld"), False))

    # ---- the curvilinear denominator 1 - cur ey near zero (the car creeps: vx = 1e-6, vy = wz = delta = a = 0) and exactly zero ----
    rows = []
    for i in (int(arcs_p[0]), int(arcs_n[0])):
        k = cur[i]
        for d in (1e-2, 1e-4, 1e-6, -1e-6, -1e-4):
            rows.append((1e-6, 0.0, (1 - d) / k, c0[i] + 0.3 * ln[i]))
        ey0 = 1 / k                                              # fl(1 - k ey) == 0 exactly, ey on the float64 grid
        for e in (ey0, np.nextafter(ey0, np.inf), np.nextafter(ey0, -np.inf)):
            if 1 - k * e == 0.0:
                rows.append((0.5, np.pi, e, c0[i] + 0.3 * ln[i]))   # num < 0: the oracle's s runs to -inf and it raises
    r = np.array(rows)
    x, xg = base(len(r), vx=r[:, 0], s=r[:, 3], ey=r[:, 2], epsi=r[:, 1])
    u = np.zeros((len(r), 2))
    dz = 1 - cur[segment_of(pt, r[:, 3])] * r[:, 2] == 0.0
    fams.append(Family("denominator", x[~dz], xg[~dz], u[~dz], np.zeros((int((~dz).sum()), 3)), ("oracle", "ld"), False,
                       "|1 - cur ey| down to 1e-6: float64 rounds cur ey before the subtraction (the reference and the kernel alike), 1e-10 of den"))
    fams.append(Family("denominator zero", x[dz], xg[dz], u[dz], np.zeros((int(dz.sum()), 3)), ("oracle",), False,
                       "1 - cur ey == 0 in float64: both sides non-finite / NO_SEGMENT"))

    # ---- noise at the clip points (5 for vx / vy, 10 for wz) and beyond, +- inf ----
    nzv = []
    for v in (5.0, -5.0, np.nextafter(5.0, 0), np.nextafter(5.0, 9), 4.0, np.inf, -np.inf):
        w = 2 * v
        nzv.append((v, -v, w))
    nzv = np.array(nzv)
    idx = np.arange(0, 990, 990 // len(nzv))[: len(nzv)]
    fams.append(Family("noise", xP[idx], gP[idx], uP[idx], nzv, ("ld", "oracle"), True))
    return fams
