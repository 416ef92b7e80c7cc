"""NumPy restatement of racinglmpc_amd/csrc/lmpc_metrics.hip.h (lmpc_rollout_lap_metrics): the same terms in the same order, the same reduction order -- thread k
folds rows k, k + 256, .. in ascending order into the identity, lanes combine at offsets 1, 2, .. 32 with the lower lane as left operand, the four waves in their
order -- so that a device result can be compared bit for bit.  NumPy rounds every elementwise operation on its own, which is what the kernel's contraction-off
arithmetic does.  Columns: racinglmpc_amd._capi.METRIC_FIELDS."""
import numpy as np

NT = 256
NCOL = 20
S_VX, S_LE, S_LE2, S_DU0, S_DU1, S_CX, S_CU, S_PATH, NS = range(9)
H_VX, H_EPSI, H_ALAT, H_LE, NH = range(5)
L_VX, L_MARGIN, NL = range(3)
QNAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]


def first_min(left, right):
    """commit_first_min: the left one stays among equals, a comparison with NaN is false."""
    return np.where(right < left, right, left)


def first_max(left, right):
    return np.where(left < right, right, left)


def weights(Q, R, xRef, bx, bu):
    return dict(Q=np.asarray(Q, float).reshape(6, 6), R=np.asarray(R, float).reshape(2, 2), xRef=np.asarray(xRef, float).reshape(6),
                bx=np.asarray(bx, float).reshape(2), bu=np.asarray(bu, float).reshape(4))


def weights_of_config(cfg):
    return weights(list(cfg.Q), list(cfg.R), list(cfg.xRef), list(cfg.bx), list(cfg.bu))


def weights_of_tuning_row(row):
    from racinglmpc_amd._capi import TUNING_FIELDS as TF
    row = np.asarray(row, float)
    return weights(row[TF["Q"]], row[TF["R"]], row[TF["xRef"]], row[TF["bx"]], row[TF["bu"]])


def identity(shape):
    return dict(sum=np.zeros(shape + (NS,)), hi=np.full(shape + (NH,), -np.inf), lo=np.full(shape + (NL,), np.inf), ey=np.full(shape, -np.inf),
                ey_row=np.full(shape, -1, np.int64), bad=np.zeros(shape, np.int64), le_rows=np.zeros(shape, np.int64))


def combine(l, r):
    """met_combine: `r` folded into `l` as the right operand."""
    take = (l["ey"] < r["ey"]) | ((l["ey"] == r["ey"]) & (r["ey_row"] < l["ey_row"]))
    return dict(sum=l["sum"] + r["sum"], hi=first_max(l["hi"], r["hi"]), lo=first_min(l["lo"], r["lo"]), ey=np.where(take, r["ey"], l["ey"]),
                ey_row=np.where(take, r["ey_row"], l["ey_row"]), bad=l["bad"] + r["bad"], le_rows=l["le_rows"] + r["le_rows"])


def row_terms(X, U, G, w, Fx, Fu):
    """met_row for rows 0 .. T-1 at once: X (T, 6), U (T, 2), G (T, 6)."""
    T = X.shape[0]
    Fx, Fu = np.asarray(Fx, float).reshape(2, 6), np.asarray(Fu, float).reshape(4, 2)
    x = [X[:, j] for j in range(6)]; u0, u1 = U[:, 0], U[:, 1]
    p = identity((T,))
    p["bad"] = (~(np.isfinite(X).all(axis=1) & np.isfinite(U).all(axis=1) & np.isfinite(G).all(axis=1))).astype(np.int64)
    p["sum"][:, S_VX] = x[0]
    p["hi"][:, H_VX] = first_max(p["hi"][:, H_VX], x[0]); p["lo"][:, L_VX] = first_min(p["lo"][:, L_VX], x[0])
    aey = np.abs(x[5]); take = p["ey"] < aey
    p["ey"] = np.where(take, aey, p["ey"]); p["ey_row"] = np.where(take, np.arange(T), p["ey_row"])
    p["hi"][:, H_EPSI] = first_max(p["hi"][:, H_EPSI], np.abs(x[3]))
    p["hi"][:, H_ALAT] = first_max(p["hi"][:, H_ALAT], np.abs(x[0] * x[2]))
    v = []
    for r in range(2):
        f = Fx[r, 0] * x[0]
        for c in range(1, 6):
            f = f + Fx[r, c] * x[c]
        d = f - w["bx"][r]
        v.append(np.where(d < 0.0, 0.0, d))
        p["hi"][:, H_LE] = first_max(p["hi"][:, H_LE], v[r])
    p["sum"][:, S_LE] = v[0] + v[1]; p["sum"][:, S_LE2] = v[0] * v[0] + v[1] * v[1]
    p["le_rows"] = ((v[0] > 0.0) | (v[1] > 0.0)).astype(np.int64)
    for r in range(4):
        p["lo"][:, L_MARGIN] = first_min(p["lo"][:, L_MARGIN], w["bu"][r] - (Fu[r, 0] * u0 + Fu[r, 1] * u1))
    if T > 1:
        d0, d1 = u0[1:] - u0[:-1], u1[1:] - u1[:-1]
        dX, dY = G[1:, 4] - G[:-1, 4], G[1:, 5] - G[:-1, 5]
        p["sum"][1:, S_DU0] = d0 * d0; p["sum"][1:, S_DU1] = d1 * d1; p["sum"][1:, S_PATH] = np.sqrt(dX * dX + dY * dY)
    e = [x[i] - w["xRef"][i] for i in range(6)]
    cx = None
    for i in range(6):
        q = w["Q"][i, 0] * e[0]
        for j in range(1, 6):
            q = q + w["Q"][i, j] * e[j]
        cx = e[0] * q if i == 0 else cx + e[i] * q
    p["sum"][:, S_CX] = cx
    R = w["R"]
    p["sum"][:, S_CU] = u0 * (R[0, 0] * u0 + R[0, 1] * u1) + u1 * (R[1, 0] * u0 + R[1, 1] * u1)
    return p


def _take(p, idx):
    return {k: a[idx] for k, a in p.items()}


def reduce_rows(p, T):
    """The kernel's reduction of T partial results (one per row): thread fold, lane tree, waves."""
    chunks = (T + NT - 1) // NT
    pad = identity((chunks * NT,))
    for k, a in p.items():
        pad[k][:T] = a
    acc = identity((NT,))
    for j in range(chunks):                                 # thread k: rows k, k + 256, .. in ascending order, each as the right operand
        acc = combine(acc, _take(pad, slice(j * NT, (j + 1) * NT)))
    acc = {k: a.reshape((NT // 64, 64) + a.shape[1:]) for k, a in acc.items()}
    off = 1
    while off < 64:                                         # lane l (left) with lane l + off (right) while l + off < 64, all lanes at once on the old values
        lo = combine(_take(acc, (slice(None), slice(0, 64 - off))), _take(acc, (slice(None), slice(off, 64))))
        for k in acc:
            acc[k] = acc[k].copy(); acc[k][:, :64 - off] = lo[k]
        off *= 2
    out = _take(acc, (0, 0))
    for wv in range(1, NT // 64):
        out = combine(out, _take(acc, (wv, 0)))
    return out


def lap_metrics(X, U, G, T, w, Fx, Fu, TL, fin_s=None):
    """One entry: rows [0, T) of one car's logs X (>= T, 6), U (>= T, 2), G (>= T, 6).  fin_s: finX_s when T is the car's crossing step (t_cross exists), else None."""
    X, U, G = (np.ascontiguousarray(np.asarray(a, float)[:T]) for a in (X, U, G))
    with np.errstate(all="ignore"):
        r = reduce_rows(row_terms(X, U, G, w, Fx, Fu), T)
        t_cross = QNAN
        if fin_s is not None:
            s = X[T - 1, 4]
            t_cross = np.float64(T - 1) + (np.float64(TL) - s) / (np.float64(fin_s) - s)
    S, H, L = r["sum"], r["hi"], r["lo"]
    return np.array([float(T), t_cross, float(r["bad"]), L[L_VX], H[H_VX], S[S_VX], r["ey"], float(r["ey_row"]), H[H_EPSI], H[H_ALAT], H[H_LE], float(r["le_rows"]),
                     S[S_LE], S[S_LE2], L[L_MARGIN], S[S_DU0], S[S_DU1], S[S_CX], S[S_CU], S[S_PATH]])


def session_metrics(X, U, G, done, finX, cars, rows, weights_of, Fx, Fu, TL_of):
    """lmpc_rollout_lap_metrics on fetched logs X (t, B, 6), U, G: entry i covers rows [0, rows[i]) of car cars[i] (rows=None: doneAt).  weights_of(car), TL_of(car)."""
    out = np.zeros((len(cars), NCOL))
    for i, c in enumerate(cars):
        T = int(done[c]) if rows is None else int(rows[i])
        out[i] = lap_metrics(X[:, c], U[:, c], G[:, c], T, weights_of(c), Fx, Fu, TL_of(c), finX[c, 4] if T == int(done[c]) else None)
    return out
