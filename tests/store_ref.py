"""What the lap stores hold after a sequence of edits, restated in NumPy / plain Python (test infrastructure): the reference of the store-writing kernels
(csrc/lmpc_commit.hip.h).  Every function computes in IEEE double with one rounding per operation (Python floats), scanning rows in their order.

  prefilter_image   the 16-bit image the regression kernel ranks rows on (the scan it serves: PredictiveModel.py:180-197)
  compute_cost      LMPC.computeCost, PredictiveControllers.py:447-464
  extend_rows       LMPC.addPoint for n rows, PredictiveControllers.py:466-474
  sorted_order      PredictiveModel.addTrajectory's sorted insert, PredictiveModel.py:35-46
  RefStores         both stores behind the method names of _capi.Context, and a snapshot in the shape the GPU tests read a context's stores in
"""
import math

import numpy as np

CHUNK = 1024          # K1_CHUNK: rows of one image chunk


def _first_min(left, right):
    """The smaller one; among equals (+0.0 == -0.0) the one met first stays."""
    return right if right < left else left


def _first_max(left, right):
    return right if left < right else left


def prefilter_image(x, u, scaling):
    """(q (3, rows - 1) uint32, par (chunks, 6), chunks) of one regression-store lap, the shape of Context.debug_model_image.

    Rows 0 .. T-2 in chunks of 1024.  Per chunk and scaled feature k of (vx, vy, wz, delta, a): lo_k / hi_k over the finite values (0 / 0 when there is none); the
    widest range over the features, each range no smaller than 1e-9 of the larger of |lo_k|, |hi_k|, and the whole no smaller than 1e-300, gives the one scale
    sc = 65535 / range.  A row's word is (feature - lo_k) * sc clamped to [0, 65535] and truncated, 0 when that is not finite; the words are packed
    (vx | vy << 16), (wz | delta << 16), (a).  par[chunk] = (lo_0 .. lo_4, sc)."""
    x, u = np.asarray(x, float), np.asarray(u, float)
    nrows = x.shape[0] - 1
    chunks = (nrows + CHUNK - 1) // CHUNK
    q = np.zeros((3, nrows), np.uint32); par = np.zeros((chunks, 6))
    sca = [float(s) for s in scaling]

    def feat(t, k):
        return float(x[t, k] if k < 3 else u[t, k - 3]) * sca[k]

    for ch in range(chunks):
        t0, t1 = ch * CHUNK, min(nrows, (ch + 1) * CHUNK)
        lo, rmax = [0.0] * 5, 0.0
        for k in range(5):
            l, h = math.inf, -math.inf
            for t in range(t0, t1):
                v = feat(t, k)
                if math.isfinite(v):
                    l = _first_min(l, v); h = _first_max(h, v)
            if not l <= h:
                l, h = 0.0, 0.0
            lo[k] = l
            floor = 1e-9 * max(abs(l), abs(h))
            rmax = max(rmax, max(h - l, floor))
        sc = 65535.0 / max(rmax, 1e-300)
        for k in range(5):
            par[ch, k] = lo[k]
            for t in range(t0, t1):
                v = (feat(t, k) - lo[k]) * sc
                w = int(min(max(v, 0.0), 65535.0)) if math.isfinite(v) else 0
                q[k >> 1, t] |= np.uint32(w << 16 if k & 1 else w)
        par[ch, 5] = sc
    return q, par, chunks


def compute_cost(x, track_length):
    """Qfun of a lap as it is added: 0 on the last row; going backwards, one more than the row behind where s < trackLength, else 0 (a NaN s is not below)."""
    x = np.asarray(x, float)
    T = x.shape[0]
    cost = np.zeros(T)
    for r in range(T - 2, -1, -1):
        cost[r] = cost[r + 1] + 1.0 if float(x[r, 4]) < track_length else 0.0
    return cost


def extend_rows(x, u, qlast, track_length):
    """(x with s + trackLength, u, Qfun) of n appended rows: Qfun counts down from qlast by REPEATED subtraction of 1.0, each rounded (qlast - (i + 1) is
    another number when qlast is no integer)."""
    x = np.array(x, float).reshape(-1, 6); u = np.array(u, float).reshape(-1, 2)
    x[:, 4] = x[:, 4] + float(track_length)
    q = np.zeros(x.shape[0]); cur = float(qlast)
    for i in range(x.shape[0]):
        cur = cur - 1.0
        q[i] = cur
    return x, u, q


def sorted_order(lengths):
    """Insertion indices of the regression laps in the store's order: ascending rows, a new lap behind the stored ones of its length (appended among equals)."""
    order = []
    for slot, T in enumerate(lengths):
        if not order or T >= lengths[order[-1]]:
            order.append(slot)
        else:
            i = 0
            while i < len(order) and not T < lengths[order[i]]:
                i += 1
            order.insert(i, slot)
    return order


class RefStores:
    """Both lap stores on the host.  The editing methods have the names and arguments of _capi.Context's, so a test can apply one sequence of calls to both."""

    def __init__(self, track_length, scaling):
        self.TL, self.scaling = float(track_length), [float(s) for s in scaling]
        self.ss = []          # [x, u, q, LapTime]
        self.model = []       # [x, u] by insertion index

    @classmethod
    def like(cls, cfg):
        return cls(cfg.trackLength, list(cfg.scaling))

    def ss_add_trajectory(self, x, u):
        x = np.array(x, float).reshape(-1, 6); u = np.array(u, float).reshape(-1, 2)
        self.ss.append([x, u, compute_cost(x, self.TL), x.shape[0]])

    def model_add_trajectory(self, x, u):
        self.model.append([np.array(x, float).reshape(-1, 6), np.array(u, float).reshape(-1, 2)])

    def model_replace_lap(self, pos, x, u):
        slot = sorted_order([m[0].shape[0] for m in self.model])[pos]
        assert np.asarray(x).shape[0] == self.model[slot][0].shape[0]
        self.model[slot] = [np.array(x, float).reshape(-1, 6), np.array(u, float).reshape(-1, 2)]

    def ss_replace_lap(self, lap, x, u, qfun):
        self.ss[lap][:3] = [np.array(x, float).reshape(-1, 6), np.array(u, float).reshape(-1, 2), np.array(qfun, float).reshape(-1)]

    def ss_extend_lap(self, lap, x, u):
        s = self.ss[lap]
        xe, ue, qe = extend_rows(x, u, s[2][-1], self.TL)
        s[:3] = [np.vstack([s[0], xe]), np.vstack([s[1], ue]), np.concatenate([s[2], qe])]

    def ss_add_point(self, x, u):
        self.ss_extend_lap(len(self.ss) - 1, np.asarray(x, float)[None], np.asarray(u, float)[None])

    def snapshot(self):
        """dict(ss, model, info, image): safe-set laps as (x, u, q, LapTime, rows); regression laps (x, u) in sorted order; (rows, sorted position) and the
        prefilter image per insertion index."""
        order = sorted_order([m[0].shape[0] for m in self.model])
        return dict(ss=[(s[0], s[1], s[2], s[3], s[0].shape[0]) for s in self.ss],
                    model=[(self.model[k][0], self.model[k][1]) for k in order],
                    info=[(m[0].shape[0], order.index(k)) for k, m in enumerate(self.model)],
                    image=[prefilter_image(m[0], m[1], self.scaling) for m in self.model])
