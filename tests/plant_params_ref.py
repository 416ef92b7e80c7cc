"""The plant with per-car vehicle constants: references and inputs of tests/test_plant_params_host.py and tests/test_gpu_plant_params.py.

tests/plant_ref.py and the oracle carry the reference's ten constants (SysModel.py:60-70) inside; here they are an argument, par (B, 10) in the order
m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br.  Two restatements of Simulator.dynModel (SysModel.py:56-147):

  dyn_model_ld_par   plant_ref.dyn_model_ld with `par`: all cars at once in np.longdouble, the track decisions in float64 as the oracle makes them;
  dyn_model_f64_par  the same arithmetic in float64, one car at a time with scalar NumPy calls in the evaluation order of oracle.dyn_model.

Both keep the reference's quirk: the rear slip angle is taken with lf (SysModel.py:97), lr enters the yaw equation only (:106).  At the reference's
constants the first reproduces plant_ref.dyn_model_ld and the second oracle.dyn_model, bit for bit (tests/test_plant_params_host.py).

well_conditioned: a state is judged numerically only where the two agree to 1e-13 (1 + |ref|).  The device is held to 1e-12 (1 + |ref|) against the longdouble
form; a sliding car whose grip or yaw inertia has moved amplifies a last-bit difference of float64 by up to 1e9 within one step, and no float64 implementation can
be held to 1e-12 there.  The decision is made from the two CPU references alone, never from a device result."""
import numpy as np

from tests import plant_ref as pr
from tests.plant_ref import N_SUB, curvature_lookup, families, scaled_err       # noqa: F401  (re-exported for the tests)

LD = np.longdouble
NPAR = 10
NAMES = ("m", "lf", "lr", "Iz", "Df", "Cf", "Bf", "Dr", "Cr", "Br")
WELL_TOL = 1e-13
STATE_FAMILIES = ("lmpc regime", "tyre fallbacks", "headings", "track position", "crossings", "noise")
PARAM_FAMILIES = ("a", "b", "c", "d")
SEED = 7


def default_row():
    """SysModel.py:60-70, restated here on its own (the library's lmpc_plant_params_default is compared with it)."""
    m = 1.98; lf = 0.125; lr = 0.125; Iz = 0.024
    Df = 0.8 * m * 9.81 / 2.0; Cf = 1.25; Bf = 1.0
    Dr = 0.8 * m * 9.81 / 2.0; Cr = 1.25; Br = 1.0
    return np.array([m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br])


def dyn_model_ld_par(pt, x, xg, u, nz, par):
    """plant_ref.dyn_model_ld with par (B, 10): (xn, xgn (B, 6) longdouble, raise (B,), wraps (B,))."""
    x = np.asarray(x, np.float64); xg = np.asarray(xg, np.float64); u = np.asarray(u, np.float64); nz = np.asarray(nz, np.float64)
    par = np.asarray(par, np.float64)
    assert par.shape == (x.shape[0], NPAR), par.shape
    m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br = (par[:, j].astype(LD) for j in range(NPAR))
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
            Fyr = Dr * np.sin(Cr * np.arctan(Br * alpha_r))
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
        clip = lambda v: np.maximum(-0.05, np.minimum(v, 0.05))
        n0, n1, n2 = clip(nz[:, 0] * 0.01), clip(nz[:, 1] * 0.01), clip(nz[:, 2] * 0.005)
        xn = np.stack([vx + LD(0.01) * n0.astype(LD), vy + LD(0.01) * n1.astype(LD), wz + LD(0.01) * n2.astype(LD), epsi, s, ey], 1)
    xgn = np.stack([vx, vy, wz, psi, X, Y], 1)
    return xn, xgn, raised, wraps


def _car_f64(pt, x, x_glob, u, nz, p):
    """oracle.dyn_model with the ten constants taken from p: the same statements in the same order, float64 scalars through the same NumPy routines."""
    from oracle import lmpc_oracle as orc
    m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br = (float(v) for v in p)
    deltaT = 0.001; dt = 0.1
    x_next = np.zeros(6); cur_x_next = np.zeros(6)
    delta, a = u[0], u[1]
    psi, X, Y = x_glob[3], x_glob[4], x_glob[5]
    vx, vy, wz, epsi, s, ey = x
    i = 0
    while (i + 1) * deltaT <= dt:
        alpha_f = delta - np.arctan2(vy + lf * wz, vx)
        alpha_r = - np.arctan2(vy - lf * wz, vx)
        Fyf = Df * np.sin(Cf * np.arctan(Bf * alpha_f))
        Fyr = Dr * np.sin(Cr * np.arctan(Br * alpha_r))
        x_next[0] = vx + deltaT * (a - 1 / m * Fyf * np.sin(delta) + wz * vy)
        x_next[1] = vy + deltaT * (1 / m * (Fyf * np.cos(delta) + Fyr) - wz * vx)
        x_next[2] = wz + deltaT * (1 / Iz * (lf * Fyf * np.cos(delta) - lr * Fyr))
        x_next[3] = psi + deltaT * (wz)
        x_next[4] = X + deltaT * ((vx * np.cos(psi) - vy * np.sin(psi)))
        x_next[5] = Y + deltaT * (vx * np.sin(psi) + vy * np.cos(psi))
        cur = orc.curvature(pt, s)
        cur_x_next[0] = x_next[0]; cur_x_next[1] = x_next[1]; cur_x_next[2] = x_next[2]
        cur_x_next[3] = epsi + deltaT * (wz - (vx * np.cos(epsi) - vy * np.sin(epsi)) / (1 - cur * ey) * cur)
        cur_x_next[4] = s + deltaT * ((vx * np.cos(epsi) - vy * np.sin(epsi)) / (1 - cur * ey))
        cur_x_next[5] = ey + deltaT * (vx * np.sin(epsi) + vy * np.cos(epsi))
        psi, X, Y = x_next[3], x_next[4], x_next[5]
        vx, vy, wz, epsi, s, ey = cur_x_next
        i += 1
    noise_vx = np.max([-0.05, np.min([nz[0] * 0.01, 0.05])])
    noise_vy = np.max([-0.05, np.min([nz[1] * 0.01, 0.05])])
    noise_wz = np.max([-0.05, np.min([nz[2] * 0.005, 0.05])])
    cur_x_next[0] += 0.01 * noise_vx; cur_x_next[1] += 0.01 * noise_vy; cur_x_next[2] += 0.01 * noise_wz
    return cur_x_next.copy(), x_next.copy()


def dyn_model_f64_par(pt, x, xg, u, nz, par):
    """The float64 form, one car at a time: (xn, xgn (B, 6) float64 -- NaN rows where the reference raises --, raise (B,))."""
    x = np.asarray(x, np.float64); xg = np.asarray(xg, np.float64); u = np.asarray(u, np.float64); nz = np.asarray(nz, np.float64)
    par = np.asarray(par, np.float64)
    B = x.shape[0]
    assert par.shape == (B, NPAR), par.shape
    xn = np.full((B, 6), np.nan); xgn = np.full((B, 6), np.nan); raised = np.zeros(B, bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            try:
                xn[b], xgn[b] = _car_f64(pt, x[b], xg[b], u[b], nz[b], par[b])
            except ValueError:
                raised[b] = True
    return xn, xgn, raised


def param_families(B, seed):
    """{"a" | "b" | "c" | "d": par (B, 10)}.  (a) all ten constants scaled independently by U(0.8, 1.2); (b) mass and grip: m in [1.5, 2.5], mu_f, mu_r in
    [0.3, 1.0], D = mu m 9.81 / 2; (c) tyre curves: Cf, Cr in [1.3, 2.2], Bf, Br in [1, 4], drawn independently front and rear; (d) axle position: lf in
    [0.09, 0.16], lr = 0.25 - lf."""
    rng = np.random.default_rng(seed)
    d = default_row()
    out = {}
    out["a"] = d[None] * rng.uniform(0.8, 1.2, (B, NPAR))
    p = np.tile(d, (B, 1))
    p[:, 0] = rng.uniform(1.5, 2.5, B)
    p[:, 4] = rng.uniform(0.3, 1.0, B) * p[:, 0] * 9.81 / 2.0; p[:, 7] = rng.uniform(0.3, 1.0, B) * p[:, 0] * 9.81 / 2.0
    out["b"] = p
    p = np.tile(d, (B, 1))
    p[:, 5] = rng.uniform(1.3, 2.2, B); p[:, 8] = rng.uniform(1.3, 2.2, B); p[:, 6] = rng.uniform(1.0, 4.0, B); p[:, 9] = rng.uniform(1.0, 4.0, B)
    assert np.all(p[:, 5] != p[:, 8]) and np.all(p[:, 6] != p[:, 9])
    out["c"] = p
    p = np.tile(d, (B, 1))
    p[:, 1] = rng.uniform(0.09, 0.16, B); p[:, 2] = 0.25 - p[:, 1]
    out["d"] = p
    return out


def tyre_fast_par(x, u, par):
    """(front, rear) booleans, the guards of plant_step_duo on the initial state with the car's own constants:
    vx > 0 && |yq| <= vx && |B alpha| <= 1 && |C atan(B alpha)| <= 1; both slip angles with lf."""
    vx, vy, wz = x[:, 0], x[:, 1], x[:, 2]
    lf = par[:, 1]
    out = []
    with np.errstate(all="ignore"):
        for role in (0, 1):
            Bt, Ct = (par[:, 9], par[:, 8]) if role else (par[:, 6], par[:, 5])
            yq = vy - lf * wz if role else vy + lf * wz
            at = np.arctan(yq / vx)
            alpha = -at if role else u[:, 0] - at
            ba = Bt * alpha
            xs = Ct * np.arctan(ba)
            out.append((vx > 0.0) & (np.abs(yq) <= vx) & (np.abs(ba) <= 1.0) & (np.abs(xs) <= 1.0))
    return out


def well_conditioned(pt, x, xg, u, nz, par, ld=None):
    """(ok (B,), (xn, xgn, raise, wraps) of dyn_model_ld_par): ok where the float64 and the longdouble form agree to WELL_TOL (1 + |ref|) on the state and on the
    global state.  Cars on which a reference raises are not ok (they are judged by their status word alone)."""
    rx, rg, raised, wraps = dyn_model_ld_par(pt, x, xg, u, nz, par) if ld is None else ld
    fx, fg, fraised = dyn_model_f64_par(pt, x, xg, u, nz, par)
    e = np.maximum(scaled_err(fx, rx), scaled_err(fg, rg))
    ok = ~raised & ~fraised & (e <= WELL_TOL)
    return ok, (rx, rg, raised, wraps), e, fraised


_CASES = {}


def cases(g, seed=SEED):
    """Every (state family, parameter family) pair the tests judge: a list of dicts with the family names, the inputs x, xg, u, nz, par, the longdouble reference
    (rx, rg), raise / wraps, the well-conditioned mask `ok` and the float64-against-longdouble scaled error `e64`.  Built once per process."""
    key = (id(g), seed)
    if key not in _CASES:
        pt = np.array(g["track"])
        fams = {f.name: f for f in families(g)}
        out = []
        for i, sn in enumerate(STATE_FAMILIES):
            f = fams[sn]
            pars = param_families(len(f), seed * 1000 + i)
            for pn in PARAM_FAMILIES:
                par = pars[pn]
                ok, (rx, rg, raised, wraps), e, fraised = well_conditioned(pt, f.x, f.xg, f.u, f.nz, par)
                out.append(dict(state=sn, param=pn, x=f.x, xg=f.xg, u=f.u, nz=f.nz, par=par, rx=rx, rg=rg, raised=raised, wraps=wraps, ok=ok, e64=e, fraised=fraised))
        _CASES[key] = out
    return _CASES[key]
