"""tests/track_cases.py -- the tracks, rows and oracle laps the per-car-track tests share (tests/test_tracks_host.py, tests/test_gpu_tracks.py).

The three tracks are the reference's three specs (Track.py:15-48; racinglmpc_amd.track.REFERENCE_SPECS): the L-shaped one it runs, the oval (13.0 m, a closing row
of 6e-16 m) and the goggle track (11 rows).  Cars are dealt over them round-robin.  PID_ROWS pins the oracle's PID laps (vt = 0.8, seed 7, multiLap = False)."""
import functools

import numpy as np

NAMES = ("L", "oval", "goggle")
PID_ROWS = {"L": 300, "oval": 200, "goggle": 295}          # rows of oracle.pid_lap(table, 0.8, seed=7, multiLap=False), measured with the oracle
TABLE_ROWS = {"L": 7, "oval": 6, "goggle": 11}
MAX_EY = 0.85                                              # the reference's halfWidth + slack on its L track; used for all three


@functools.lru_cache(maxsize=None)
def table(name):
    from racinglmpc_amd import track
    tab, TL = track.table_from_spec(track.REFERENCE_SPECS[name])
    tab.setflags(write=False)
    return tab, TL


def deal(B, names=NAMES, perm=None):
    """Track name of each of B cars: round-robin over `names`, then permuted."""
    out = [names[b % len(names)] for b in range(B)]
    return out if perm is None else [out[i] for i in perm]


def rows_of(names):
    from racinglmpc_amd import _capi
    return _capi.track_rows([(np.array(table(n)[0]), table(n)[1]) for n in names])


def lengths_of(names):
    return np.array([table(n)[1] for n in names])


@functools.lru_cache(maxsize=None)
def pid_lap(name, steps=None, seed=7, vt=0.8):
    """oracle.pid_lap on the track: one lap up to the line (steps = None: multiLap = False), or `steps` rows of a multiLap run.  (x, u, x_glob), read-only."""
    from oracle import lmpc_oracle as orc
    pt = np.array(table(name)[0])
    if steps is None:
        out = orc.pid_lap(pt, vt, seed=seed, multiLap=False)
    else:
        out = orc.pid_lap(pt, vt, seed=seed, multiLap=True, maxSimTime=steps * 0.1 + 0.05)
    for a in out:
        a.setflags(write=False)
    return out


def global_lap(name, x):
    """x_glob rows [vx, vy, wz, psi, X, Y] of curvilinear rows x on the track: psi by track_ref.track_angle, (X, Y) by the oracle's getGlobalPosition -- the exact
    image of the rows under the forward map (the simulator's own x_glob integrates on its own and differs from it by the integration error)."""
    from oracle import lmpc_oracle as orc
    from tests import track_ref
    pt = np.array(table(name)[0])
    psi, st = track_ref.track_angle_batch(pt, x[:, 4], x[:, 3])
    assert np.all(st == 0)
    xy = np.array([orc.get_global_position(pt, float(s), float(ey)) for s, ey in zip(x[:, 4], x[:, 5])])
    return np.stack([x[:, 0], x[:, 1], x[:, 2], psi, xy[:, 0], xy[:, 1]], axis=1)
