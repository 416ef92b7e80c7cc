"""CPU: the counter-based device noise -- the NumPy restatement of its block function against NumPy's own Philox generator, the four entry points in the library,
the header and the ctypes layer, and the bookkeeping of BatchedRollouts(device_noise=...) against a recording stand-in for the device context."""
import os
import re

import numpy as np
import pytest

from tests import common
from tests import noise_ref

NEW = ("lmpc_noise_raw", "lmpc_noise_fill", "lmpc_rollout_set_noise", "lmpc_rollout_get_noise")


def test_restated_block_function_equals_numpy_philox():
    """noise_ref.words(seed, stream, lap, t, car) == numpy.random.Philox(counter=[t, car, lap, stream], key=[seed, 0]).random_raw(4) on 300 random 64-bit tuples and on
    the corners t = 0, car = 2**32 + 5, seed = 2**64 - 1, all-ones car / lap words, t = 2**63 - 1 and 2**64 - 2 (the C ABI's steps are non-negative long long values, so
    t + 1 never carries into the car word as NumPy's 256-bit counter increment would at t = 2**64 - 1); without the + 1 on word 0 of the counter the two differ."""
    rng = np.random.default_rng(2024)
    tuples = [tuple(int(v) for v in rng.integers(0, 2 ** 64, size=5, dtype=np.uint64)) for _ in range(300)]
    tuples += [(2 ** 64 - 1, 0, 3, 0, 2 ** 32 + 5), (0, 0, 0, 0, 0), (11, 1, 2, 7, 100), (2 ** 64 - 1, 1, 2 ** 64 - 1, 2 ** 64 - 2, 2 ** 64 - 1), (5, 0, 0, 2 ** 63 - 1, 9),
               (1, 0, 0, 2 ** 32 - 1, 2 ** 32 - 1), (1, 0, 0, 2 ** 32, 2 ** 32)]
    for seed, stream, lap, t, car in tuples:
        want = noise_ref.numpy_words(seed, stream, lap, t, car)
        got = noise_ref.words(seed, stream, lap, t, car)
        assert got.dtype == np.uint64 and got.shape == (4,) and np.array_equal(got, want), (seed, stream, lap, t, car, got, want)
    # vectorised over (t, car), as the GPU tests use it
    got = noise_ref.raw(2 ** 64 - 1, 1, 3, 7, 3, 2 ** 32 + 5, 5)
    assert got.shape == (3, 5, 4)
    for i in range(3):
        for b in range(5):
            assert np.array_equal(got[i, b], noise_ref.numpy_words(2 ** 64 - 1, 1, 3, 7 + i, 2 ** 32 + 5 + b))
    # the block function on the counter as given (no increment) is NOT NumPy's first block
    plain = np.array([int(v[0]) for v in noise_ref.philox4x64_10(7, 100, 2, 1, 11, 0)], dtype=np.uint64)
    assert not np.array_equal(plain, noise_ref.numpy_words(11, 1, 2, 7, 100))
    assert np.array_equal(plain, noise_ref.numpy_words(11, 1, 2, 6, 100))


def test_restated_transform_is_box_muller_on_the_documented_uniforms():
    """u1 in (0, 1], u2 in [0, 1) at the extreme words; z0^2 + z1^2 = -2 log u1; width 2 is the first two columns of width 3; the draws look standard normal."""
    z0, z1 = noise_ref.box_muller(np.array([0, 2 ** 64 - 1], dtype=np.uint64), np.array([0, 2 ** 64 - 1], dtype=np.uint64))
    assert np.all(np.isfinite(z0)) and np.all(np.isfinite(z1))
    assert z0[0] == np.sqrt(-2.0 * np.log(2.0 ** -53)) and z1[0] == 0.0 and abs(z0[0]) < 8.6           # u1 = 2^-53, u2 = 0: the largest radius
    assert z0[1] == 0.0 and z1[1] == 0.0                                                               # u1 = 1: radius 0
    f3 = noise_ref.fill(11, 1, 2, 0, 40, 100, 33, 3); f2 = noise_ref.fill(11, 1, 2, 0, 40, 100, 33, 2)
    assert f3.shape == (40, 33, 3) and f2.shape == (40, 33, 2) and np.array_equal(f2, f3[..., :2])
    w = noise_ref.raw(11, 1, 2, 0, 40, 100, 33)
    u1 = ((w[..., 0] >> np.uint64(11)) + np.uint64(1)).astype(float) * 2.0 ** -53
    assert np.allclose(f3[..., 0] ** 2 + f3[..., 1] ** 2, -2.0 * np.log(u1), rtol=1e-12, atol=0)
    assert abs(f3.mean()) < 0.05 and abs(f3.std() - 1.0) < 0.05 and not np.array_equal(f3, noise_ref.fill(11, 0, 2, 0, 40, 100, 33, 3))


def _header_decl(name):
    header = open(os.path.join(common.ROOT, "include", "lmpc_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
    return None if m is None else [" ".join(a.replace("*", " * ").split()) for a in m.group(1).split(",")]


def test_entry_points_are_exported_declared_and_bound(built):
    """liblmpc_hip.so exports lmpc_noise_raw, lmpc_noise_fill, lmpc_rollout_set_noise and lmpc_rollout_get_noise, include/lmpc_hip.h declares them with the 64-bit
    argument types, _capi binds them with those types and Context has the four methods; the session entry points document noise = NULL."""
    import ctypes as C
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 103
    for name in NEW:
        assert name in _capi.EXPORTS and hasattr(lib, name), name
        assert _header_decl(name) is not None, name
    u64, i64 = "unsigned long long", "long long"
    d = _header_decl("lmpc_noise_raw")
    assert [a.rsplit(" ", 1)[0] for a in d[1:]] == [u64, u64, u64, i64, "int", i64, "int", u64 + " *"], d
    d = _header_decl("lmpc_noise_fill")
    assert [a.rsplit(" ", 1)[0] for a in d[1:]] == [u64, u64, u64, i64, "int", i64, "int", "int", "double *"], d
    d = _header_decl("lmpc_rollout_set_noise")
    assert [a.rsplit(" ", 1)[0] for a in d[1:]] == ["int", u64, u64, i64], d
    d = _header_decl("lmpc_rollout_get_noise")
    assert [a.rsplit(" ", 1)[0] for a in d[1:]] == ["int *", u64 + " *", u64 + " *", i64 + " *"], d
    assert lib.lmpc_noise_raw.argtypes == [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_void_p]
    assert lib.lmpc_noise_fill.argtypes == [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    assert lib.lmpc_rollout_set_noise.argtypes[1:] == [C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_longlong]
    for name in NEW:
        assert getattr(lib, name).restype is C.c_int
    for meth in ("noise_raw", "noise_fill", "rollout_set_noise", "rollout_get_noise"):
        assert callable(getattr(_capi.Context, meth)), meth
    # no context: LMPC_E_ARG, not a crash
    assert lib.lmpc_rollout_set_noise(None, 1, 0, 0, 0) == -1 and lib.lmpc_rollout_get_noise(None, None, None, None, None) == -1
    assert lib.lmpc_noise_fill(None, 0, 0, 0, 0, 1, 0, 1, 3, None) == -1 and lib.lmpc_noise_raw(None, 0, 0, 0, 0, 1, 0, 1, None) == -1


class _Recorder:
    """Stands where the device context stands (tests/standin_capi.py offers no rollout sessions): keeps what the lap runners hand over, in call order."""
    N = 12

    def __init__(self):
        self.calls = []

    def _keep(self, a):
        return None if a is None else np.array(a)

    def _shape(self, B, noise, T_max):
        self.B = B; self.T = int(T_max) if noise is None else noise.shape[0]

    def rollout_set_noise(self, on, seed=0, lap=0, car0=0):
        self.calls.append(("set_noise", on, seed, lap, car0))

    def rollout_begin(self, x0, xg, xLin0, uLin0, noise, T_max=None):
        self._shape(x0.shape[0], noise, T_max); self.calls.append(("lmpc", None, self._keep(noise), T_max))

    def rollout_pid(self, x0, xg, vt, noise_u, noise, stop_at_line=False, T_max=None):
        self._shape(x0.shape[0], noise, T_max); self.calls.append(("pid", self._keep(noise_u), self._keep(noise), T_max))
        return self.T, self.B

    def rollout_begin_mpc(self, x0, xg, noise, xLin0=None, uLin0=None, A=None, B=None, stop_at_line=False, T_max=None):
        self._shape(x0.shape[0], noise, T_max); self.calls.append(("lti" if A is not None else "ltv", None, self._keep(noise), T_max))

    def rollout_run(self, n):
        return self.T, self.B

    def rollout_fetch(self, t0, t1):
        B, n = self.B, t1 - t0
        return (np.zeros((n, B, 6)), np.zeros((n, B, 2)), np.zeros((n, B, 6)), np.full(B, 5, np.int32), np.zeros(B, np.int32), np.zeros((B, 6)), np.zeros((B, 6)))

    def rollout_end(self):
        pass


def _drive(ro, B, T):
    """begin, run_pid_laps, both forms of run_mpc_laps, begin again: five sessions."""
    x0 = np.zeros((B, 6))
    ro.begin(x0, np.zeros((13, 6)), np.zeros((12, 2)), max_steps=T)
    laps = ro.run_pid_laps(0.7 + 0.01 * np.arange(B), max_steps=T)
    assert len(laps) == B and laps[0][0].shape == (T, 6)
    ro.run_mpc_laps(x0, A=np.zeros((B, 6, 6)), B=np.zeros((B, 6, 2)), max_steps=T)
    ro.run_mpc_laps(x0, xLin0=np.zeros((13, 6)), uLin0=np.zeros((12, 2)), max_steps=T + 3)
    ro.begin(x0, np.zeros((13, 6)), np.zeros((12, 2)), max_steps=T)


@pytest.mark.parametrize("shard", [None, (17, 22, 33)])
def test_device_noise_never_draws_on_the_host_and_counts_sessions(shard):
    """BatchedRollouts(device_noise=True): rng.bit_generator.state is untouched across begin, run_pid_laps and run_mpc_laps, no worker thread exists, every session
    is begun with noise=None (run_pid_laps: noise_u=None too) and T_max = max_steps, directly after rollout_set_noise(True, seed, lap, car0) with lap = 0, 1, 2, ...
    and car0 = noise_shard[0] (0 without a shard); prefetch_noise and close do nothing."""
    import threading
    from racinglmpc_amd import rollout
    B, T, seed = 5, 40, 2 ** 63 + 11
    ctx = _Recorder()
    ro = rollout.BatchedRollouts(ctx, np.array([[0, 0, 0, 0, 10.0, 0.0]]), seed=seed, device_noise=True)
    if shard is not None:
        ro.noise_shard = shard
    state = ro.rng.bit_generator.state
    threads = threading.active_count()
    assert ro.lap == 0
    ro.prefetch_noise(T, B, wait=True)
    assert ctx.calls == [] and ro._pre is None
    _drive(ro, B, T)
    assert ro.rng.bit_generator.state == state and ro._pre is None and not hasattr(ro, "_pool") and threading.active_count() == threads
    ro.close()
    assert ro.rng.bit_generator.state == state and ro.lap == 5
    car0 = 0 if shard is None else shard[0]
    kinds = ["lmpc", "pid", "lti", "ltv", "lmpc"]
    steps = [T, T, T, T + 3, T]
    assert len(ctx.calls) == 10
    for i, (kind, n) in enumerate(zip(kinds, steps)):
        assert ctx.calls[2 * i] == ("set_noise", True, seed, i, car0), (i, ctx.calls[2 * i])
        k, nu, nz, T_max = ctx.calls[2 * i + 1]
        assert k == kind and nu is None and nz is None and T_max == n, (i, ctx.calls[2 * i + 1][0], T_max)
    with pytest.raises(ValueError):
        rollout.BatchedRollouts(ctx, np.array([[0, 0, 0, 0, 10.0, 0.0]]), seed=-1, device_noise=True)
    with pytest.raises(TypeError):
        rollout.BatchedRollouts(ctx, np.array([[0, 0, 0, 0, 10.0, 0.0]]), seed=None, device_noise=True)


@pytest.mark.parametrize("prefetch", [False, True])
def test_host_noise_is_unchanged_without_device_noise(prefetch):
    """device_noise=False (the default): the context is handed the arrays of numpy.random.default_rng(seed).standard_normal in the documented order -- one (T, B, 3) per
    begin and per MPC session, (T, B, 2) then (T, B, 3) per PID lap --, rollout_set_noise is never called, no T_max is passed, and after close() the generator is where
    a run without prefetching leaves it."""
    from racinglmpc_amd import rollout
    B, T, seed = 5, 40, 11
    ctx = _Recorder()
    ro = rollout.BatchedRollouts(ctx, np.array([[0, 0, 0, 0, 10.0, 0.0]]), seed=seed, prefetch=prefetch)
    assert ro.device_noise is False
    _drive(ro, B, T)
    ro.close()
    ref = np.random.default_rng(seed)
    want = [("lmpc", None, ref.standard_normal((T, B, 3))), ("pid", ref.standard_normal((T, B, 2)), ref.standard_normal((T, B, 3))), ("lti", None, ref.standard_normal((T, B, 3))),
            ("ltv", None, ref.standard_normal((T + 3, B, 3))), ("lmpc", None, ref.standard_normal((T, B, 3)))]
    assert [c[0] for c in ctx.calls] == [w[0] for w in want]
    for c, w in zip(ctx.calls, want):
        assert c[3] is None
        assert (c[1] is None) == (w[1] is None) and (w[1] is None or np.array_equal(c[1], w[1])), c[0]
        assert np.array_equal(c[2], w[2]), c[0]
    assert ro.rng.bit_generator.state == ref.bit_generator.state and ro.lap == 0


def test_context_methods_pass_null_and_need_a_length():
    """Context.rollout_begin / rollout_begin_mpc / rollout_pid with noise=None hand NULL and T_max to the library; without T_max there is no length to run: ValueError
    before anything reaches the library."""
    from racinglmpc_amd import _capi

    class _Lib:
        def __init__(self):
            self.seen = []

        def __getattr__(self, name):
            def f(*a):
                self.seen.append((name, a)); return 0
            return f
    ctx = _capi.Context.__new__(_capi.Context)
    ctx.lib = _Lib(); ctx._h = None; ctx.N = 12; ctx._pid = -1
    B, T = 3, 9
    x0 = np.zeros((B, 6)); xl = np.zeros((B, 13, 6)); ul = np.zeros((B, 12, 2))
    val = lambda v: getattr(v, "value", v)
    ctx.rollout_begin(x0, x0, xl, ul, None, T_max=T)
    name, a = ctx.lib.seen[-1]
    assert name == "lmpc_rollout_begin" and val(a[1]) == B and val(a[2]) == T and a[-1] is None and ctx._ro == (B, T)
    ctx.rollout_begin_mpc(x0, x0, None, xLin0=xl, uLin0=ul, T_max=T)
    name, a = ctx.lib.seen[-1]
    assert name == "lmpc_rollout_begin_mpc" and a[1] == B and a[2] == T and a[9] is None and a[10] == 0
    ctx.rollout_pid(x0, x0, 0.8, None, None, T_max=T)
    name, a = ctx.lib.seen[-1]
    assert name == "lmpc_rollout_pid" and a[1] == B and a[2] == T and a[6] is None and a[7] is None
    nz = np.zeros((T, B, 3))
    ctx.rollout_pid(x0, x0, 0.8, None, nz)                       # (one array given: it sets the length)
    name, a = ctx.lib.seen[-1]
    assert a[2] == T and a[6] is None and a[7] == nz.ctypes.data
    ctx.rollout_begin(x0, x0, xl, ul, nz)
    name, a = ctx.lib.seen[-1]
    assert val(a[2]) == T and val(a[-1]) == nz.ctypes.data
    n = len(ctx.lib.seen)
    for call in (lambda: ctx.rollout_begin(x0, x0, xl, ul, None), lambda: ctx.rollout_begin_mpc(x0, x0, None, xLin0=xl, uLin0=ul), lambda: ctx.rollout_pid(x0, x0, 0.8, None, None)):
        with pytest.raises(ValueError):
            call()
    assert len(ctx.lib.seen) == n
