"""tests/standin_tracks.py -- tests/standin_track.py plus per-car tracks (test infrastructure, never product).

standin_track.Context with what racinglmpc_amd._capi.Context gained for lmpc_track_set: track_set / tracks, the track_row argument of ss_add_trajectory and
ss_extend_lap, and the inverse map of a T x B log in which car b lies on row b.  The rules are the C entry points': one row serves every element, n > 1 rows
need a call of n elements (LmpcError), a host-side lap writer without track_row is refused at n > 1.  The arithmetic is the oracle's and tests/track_ref.py's on
the table of the element's row.  It also carries scripted rollout sessions, enough for rollout.PerCarLMPC's bookkeeping: every car finishes after `done[b]` steps."""
import numpy as np

from oracle import lmpc_oracle as orc
from tests import standin_capi as base
from tests import standin_track
from tests import track_ref
from tests.standin_capi import CALLS, LmpcError, config_from  # noqa: F401  (the stand-in's module interface)

TRACK_NPAR = 98


def _table(row):
    n = int(row[0])
    return np.array(row[2:2 + 6 * n]).reshape(n, 6), float(row[1])


class Context(standin_track.Context):
    def __init__(self, cfg, done=None):
        super().__init__(cfg)
        self.trk = np.zeros((0, TRACK_NPAR))
        self.done = done                 # scripted sessions: crossing step of every car
        self.session = None
        self.begun = []                  # x0 of every session begun

    # ---- rows
    def track_set(self, rows):
        base._rec("track_set", None if rows is None else np.array(rows))
        if self.session is not None:
            raise LmpcError("liblmpc_hip error -4: lmpc_track_set: a rollout session is active")
        self.trk = np.zeros((0, TRACK_NPAR)) if rows is None or np.size(rows) == 0 else np.array(rows, float).reshape(-1, TRACK_NPAR)

    def tracks(self):
        return self.trk.copy()

    def _tl(self, track_row, who):
        n = self.trk.shape[0]
        if track_row is None:
            if n > 1:
                raise LmpcError("liblmpc_hip error -4: %s: lmpc_track_set holds %d rows and this call names no car" % (who, n))
            return self.cfg.trackLength if n == 0 else float(self.trk[0, 1])
        if not 0 <= int(track_row) < max(n, 1):
            raise LmpcError("liblmpc_hip error -1: %s: track_row %d, %d rows in force" % (who, track_row, n))
        return self.cfg.trackLength if n == 0 else float(self.trk[0 if n == 1 else int(track_row), 1])

    # ---- stores
    def ss_add_trajectory(self, x, u, track_row=None):
        base._rec("ss_add_trajectory", (np.asarray(x).shape, track_row))
        TL = self._tl(track_row, "lmpc_ss_add_trajectory")
        x = np.array(x, float)
        self.SS.append(x); self.uSS.append(np.array(u, float)); self.LapTime.append(x.shape[0])
        self.Qfun.append(orc.compute_cost(x, TL))

    def ss_extend_lap(self, lap, x, u, track_row=None):
        base._rec("ss_extend_lap", (int(lap), np.asarray(x).shape, track_row))
        TL = self._tl(track_row, "lmpc_ss_extend_lap")
        x = np.array(x, float); x[:, 4] += TL
        q = self.Qfun[lap][-1] - 1.0 - np.arange(x.shape[0])
        self.SS[lap] = np.concatenate([self.SS[lap], x]); self.uSS[lap] = np.concatenate([self.uSS[lap], np.array(u, float)]); self.Qfun[lap] = np.concatenate([self.Qfun[lap], q])

    def ss_num_laps(self):
        return len(self.SS)

    def model_num_laps(self):
        return len(self.xStored)

    def model_set_lap_table(self, rows):
        base._rec("model_set_lap_table", None)

    def ss_set_lap_table(self, rows, last=None):
        base._rec("ss_set_lap_table", None)

    # ---- the inverse map of a log: car b on row b
    def state_from_global(self, xglob, max_ey):
        xg = np.asarray(xglob, float)
        n = self.trk.shape[0]
        if n == 0:
            return super().state_from_global(xg, max_ey)
        base._rec("state_from_global", xg.shape)
        standin_track._check_max_ey(max_ey)
        log = xg if xg.ndim == 3 else xg[:, None]
        if n > 1 and log.shape[1] != n:
            raise LmpcError("liblmpc_hip error -1: track rows: B = %d elements but lmpc_track_set holds %d rows" % (log.shape[1], n))
        out = np.zeros(log.shape); st = np.zeros(log.shape[:2], np.int32)
        for b in range(log.shape[1]):
            out[:, b], st[:, b] = track_ref.state_from_global(_table(self.trk[0 if n == 1 else b])[0], log[:, b], float(max_ey))
        return (out, st) if xg.ndim == 3 else (out[:, 0], st[:, 0])

    # ---- scripted sessions
    def rollout_begin(self, x0, xglob0, xLin0, uLin0, noise):
        base._rec("rollout_begin", None)
        n = self.trk.shape[0]
        if n > 1 and np.asarray(x0).shape[0] != n:
            raise LmpcError("liblmpc_hip error -1: track rows: B = %d elements but lmpc_track_set holds %d rows" % (np.asarray(x0).shape[0], n))
        self.session = dict(B=np.asarray(x0).shape[0], t=0)
        self.begun.append(np.array(x0, float))

    def rollout_run(self, n):
        self.session["t"] = min(max(self.done) + 1, self.session["t"] + n)
        return self.session["t"], 0

    def rollout_fetch(self, t0, t1):
        B, n = self.session["B"], t1 - t0
        X = np.zeros((n, B, 6)); X[:, :, 4] = 0.1 * np.arange(t0, t1)[:, None]
        fin = np.zeros((B, 6)); fin[:, 4] = 100.0
        return X, np.zeros((n, B, 2)), np.zeros((n, B, 6)), np.array(self.done, np.int32), np.zeros(B, np.int32), fin, np.zeros((B, 6))

    def rollout_end(self):
        self.session = None
