"""tests/standin_track.py -- tests/standin_capi.py plus the inverse track map (test infrastructure, never product).

standin_capi.Context with the three methods racinglmpc_amd._capi.Context gained for the inverse map -- local_position, track_angle, state_from_global --, the
arithmetic behind them being tests/track_ref.py on the track table of the stand-in's configuration.  Calls are recorded in standin_capi.CALLS like every other
call of the stand-in; the argument checks are those of the C entry points (LMPC_E_ARG there, LmpcError here)."""
import numpy as np

from tests import standin_capi as base
from tests import track_ref
from tests.standin_capi import CALLS, LmpcError, config_from  # noqa: F401  (the stand-in's module interface)

ST_NO_SEGMENT = base.ST_NO_SEGMENT


def _check_max_ey(max_ey):
    if not (np.isfinite(max_ey) and max_ey >= 0):
        raise LmpcError("liblmpc_hip error -1: argument check failed: max_ey")


class Context(base.Context):
    def local_position(self, x, y, psi, max_ey):
        x = np.ravel(np.asarray(x, float))
        base._rec("local_position", x.shape)
        _check_max_ey(max_ey)
        if x.shape[0] < 1:
            raise LmpcError("liblmpc_hip error -1: argument check failed: n >= 1")
        s, ey, epsi, st, _ = track_ref.local_position_batch(self.cfg.track, x, y, psi, float(max_ey))
        return s, ey, epsi, st

    def track_angle(self, s, epsi):
        s = np.ravel(np.asarray(s, float))
        base._rec("track_angle", s.shape)
        if s.shape[0] < 1:
            raise LmpcError("liblmpc_hip error -1: argument check failed: n >= 1")
        return track_ref.track_angle_batch(self.cfg.track, s, epsi)

    def state_from_global(self, xglob, max_ey):
        xg = np.asarray(xglob, float)
        base._rec("state_from_global", xg.shape)
        _check_max_ey(max_ey)
        if xg.ndim not in (2, 3) or xg.shape[-1] != 6 or xg.shape[0] < 1:
            raise LmpcError("liblmpc_hip error -1: argument check failed: T >= 1 && B >= 1")
        return track_ref.state_from_global(self.cfg.track, xg, float(max_ey))
