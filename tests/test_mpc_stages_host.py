"""CPU: the entry points of the batched PID / MPC / LTV-MPC stages (main.py:61-95) are exported by the library and bound with the header's argument
types, and the noise bookkeeping of BatchedRollouts.run_pid_laps / run_mpc_laps is the documented one with and without the prefetcher."""
import ctypes as C
import os
import re

import numpy as np

from tests import common

NEW = ("lmpc_rollout_begin_mpc", "lmpc_rollout_pid", "lmpc_lti_regression_batch")


def _header_args(name):
    """C argument types of `name` as include/lmpc_hip.h declares them: a list of "ptr", "int", "double"."""
    header = open(os.path.join(common.ROOT, "include", "lmpc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
    assert m, "no declaration of %s" % name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append("ptr" if "*" in a else "double" if a.startswith("double") else "int" if a.startswith("int") else a)
    return out


def test_new_entry_points_are_exported_and_bound_with_the_header_types(built):
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 101
    for name in NEW:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
        f = getattr(lib, name)
        want = _header_args(name)
        assert f.restype is C.c_int and f.argtypes is not None and len(f.argtypes) == len(want), (name, want, f.argtypes)
        for i, (w, t) in enumerate(zip(want, f.argtypes)):
            if w == "ptr":
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, i, t)
            else:
                assert t is {"int": C.c_int, "double": C.c_double}[w], (name, i, w, t)
    assert _header_args("lmpc_rollout_pid") == ["ptr", "int", "int", "ptr", "ptr", "ptr", "ptr", "ptr", "int", "ptr", "ptr"]
    assert _header_args("lmpc_rollout_begin_mpc") == ["ptr", "int", "int"] + ["ptr"] * 7 + ["int"]
    assert _header_args("lmpc_lti_regression_batch") == ["int", "int", "ptr", "ptr", "ptr", "int", "double", "ptr", "ptr", "ptr", "ptr"]
    for meth in ("rollout_begin_mpc", "rollout_pid"):
        assert callable(getattr(_capi.Context, meth))
    assert callable(_capi.lti_regression_batch)


class _Recorder:
    """Stands where the device context stands: keeps the arrays the lap runners hand over."""
    N = 12

    def __init__(self):
        self.calls = []

    def rollout_pid(self, x0, xg, vt, noise_u, noise, stop_at_line=False):
        self.calls.append(("pid", np.array(noise_u), np.array(noise))); self.T = noise.shape[0]; self.B = x0.shape[0]
        return self.T, self.B

    def rollout_begin_mpc(self, x0, xg, noise, xLin0=None, uLin0=None, A=None, B=None, stop_at_line=False):
        self.calls.append(("lti" if A is not None else "ltv", None, np.array(noise))); self.T = noise.shape[0]; self.B = x0.shape[0]

    def rollout_run(self, n):
        return self.T, self.B

    def rollout_fetch(self, t0, t1):
        B, n = self.B, t1 - t0
        return (np.zeros((n, B, 6)), np.zeros((n, B, 2)), np.zeros((n, B, 6)), np.full(B, 5, np.int32), np.zeros(B, np.int32), np.zeros((B, 6)), np.zeros((B, 6)))

    def rollout_end(self):
        pass


def _stages(prefetch, seed=11, B=5, T=40):
    from racinglmpc_amd import rollout
    ctx = _Recorder()
    track = np.array([[0, 0, 0, 0, 10.0, 0.0]])
    ro = rollout.BatchedRollouts(ctx, track, seed=seed, prefetch=prefetch)
    x0 = np.zeros((B, 6))
    laps = ro.run_pid_laps(0.7 + 0.01 * np.arange(B), max_steps=T)
    assert len(laps) == B and laps[0][0].shape == (T, 6)                 # multiLap: every logged row
    assert ro.run_pid_laps(0.7 + 0.01 * np.arange(B), max_steps=T, stop_at_line=True)[0][0].shape == (5, 6)
    ro.run_mpc_laps(x0, A=np.zeros((B, 6, 6)), B=np.zeros((B, 6, 2)), max_steps=T)
    ro.run_mpc_laps(x0, xLin0=np.zeros((13, 6)), uLin0=np.zeros((12, 2)), max_steps=T)
    ro.run_mpc_laps(x0, xLin0=np.zeros((13, 6)), uLin0=np.zeros((12, 2)), max_steps=T + 3)
    ro.close()
    return ctx.calls, ro.rng.bit_generator.state


def test_noise_of_the_pid_and_mpc_laps_is_drawn_in_the_documented_order():
    """Same seed => same arrays with and without the prefetcher, in the order run_pid_laps / run_mpc_laps document (control-law noise (T, B, 2), then plant noise
    (T, B, 3) per PID lap; one plant draw per MPC lap), and after close() the generator is where a run without prefetching leaves it."""
    B, T = 5, 40
    ref = np.random.default_rng(11)
    want = [("pid", ref.standard_normal((T, B, 2)), ref.standard_normal((T, B, 3))), ("pid", ref.standard_normal((T, B, 2)), ref.standard_normal((T, B, 3))),
            ("lti", None, ref.standard_normal((T, B, 3))), ("ltv", None, ref.standard_normal((T, B, 3))), ("ltv", None, ref.standard_normal((T + 3, B, 3)))]
    for prefetch in (False, True):
        calls, state = _stages(prefetch)
        assert [c[0] for c in calls] == [w[0] for w in want]
        for c, w in zip(calls, want):
            assert (c[1] is None) == (w[1] is None) and (w[1] is None or np.array_equal(c[1], w[1])), (prefetch, c[0])
            assert np.array_equal(c[2], w[2]), (prefetch, c[0])
        assert state == ref.bit_generator.state, prefetch
