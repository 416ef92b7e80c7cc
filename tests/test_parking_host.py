"""CPU: parking (lmpc_rollout_set_parking / _get_parking / _parked_at, lmpc_debug_live_compact) -- what needs no device: exports, declarations and bindings; the
argument check of the Python layer with its messages; and the hand-over by BatchedRollouts and PerCarLMPC on scripted stand-in contexts: what reaches the context
per session and per generation, and nothing at all while `park` is off.  The GPU side is tests/test_gpu_parking.py."""
import os
import re

import numpy as np
import pytest

from tests import common

NEW = ("lmpc_rollout_set_parking", "lmpc_rollout_get_parking", "lmpc_rollout_parked_at", "lmpc_debug_live_compact")


def _header():
    with open(os.path.join(common.ROOT, "include", "lmpc_hip.h")) as f:
        return f.read()


def _header_decl(name):
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
    return None if m is None else [" ".join(a.replace("*", " * ").split()) for a in m.group(1).split(",")]


def test_entry_points_are_exported_declared_and_bound(built):
    """liblmpc_hip.so is version 111 or later and exports the four entry points; include/lmpc_hip.h declares them and the two mode bits as the issue writes them;
    _capi binds them with those types and Context has the four methods.  Without a context every one is LMPC_E_ARG, not a crash."""
    import ctypes as C
    from racinglmpc_amd import _capi
    lib = _capi.load()
    assert lib.lmpc_version() >= 111
    for name in NEW:
        assert name in _capi.EXPORTS and hasattr(lib, name) and getattr(lib, name).restype is C.c_int, name
    types = lambda name: [a.rsplit(" ", 1)[0] for a in _header_decl(name)[1:]]
    assert types("lmpc_rollout_set_parking") == ["unsigned", "int", "const int *"]
    assert types("lmpc_rollout_get_parking") == ["unsigned *", "int *", "int *", "int"]
    assert types("lmpc_rollout_parked_at") == ["int *", "int *"]
    assert types("lmpc_debug_live_compact") == ["int", "const int *", "const int *", "int", "unsigned", "int *", "int *", "int *"]
    assert lib.lmpc_rollout_set_parking.argtypes == [C.c_void_p, C.c_uint, C.c_int, C.c_void_p]
    assert lib.lmpc_rollout_get_parking.argtypes == [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.c_void_p, C.c_int]
    assert lib.lmpc_rollout_parked_at.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    assert lib.lmpc_debug_live_compact.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    bits = dict(re.findall(r"#define LMPC_PARK_([A-Z]+)\s+(\d+)u", _header()))
    assert bits == dict(FINISHED="1", REROUTE="2") and (_capi.PARK_FINISHED, _capi.PARK_REROUTE) == (1, 2)
    for meth in ("rollout_set_parking", "rollout_parking", "rollout_parked_at", "debug_live_compact"):
        assert callable(getattr(_capi.Context, meth)), meth
    mode, n, nl = C.c_uint(), C.c_int(), C.c_int()
    one = np.zeros(1, np.int32)
    assert lib.lmpc_rollout_set_parking(None, 0, 0, None) == -1 and lib.lmpc_rollout_get_parking(None, C.byref(mode), C.byref(n), None, 0) == -1
    assert lib.lmpc_rollout_parked_at(None, None, C.byref(nl)) == -1
    assert lib.lmpc_debug_live_compact(None, 1, one.ctypes.data, one.ctypes.data, 0, 0, one.ctypes.data, one.ctypes.data, C.byref(nl)) == -1


def test_the_compaction_kernel_and_the_variant_revision():
    """The compaction kernel has a header of its own, and the variant libraries are asked for revision 11 (their launchers take the live list)."""
    src = os.path.join(common.ROOT, "racinglmpc_amd", "csrc")
    with open(os.path.join(src, "lmpc_live.hip.h")) as f:
        assert "lmpc_rollout_live_kernel" in f.read()
    with open(os.path.join(src, "lmpc_kernels.hip.h")) as f:
        assert re.search(r"#define LMPC_VARIANT_ABI_REV 11\b", f.read())


class _NoLibrary:
    """Stands where the loaded library stands: any call is a failure of the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def test_check_parking_raises_before_the_library_is_called():
    """check_parking and Context.rollout_set_parking: unknown mode bits, a negative or repeated car, a list that is not one-dimensional or not of integers --
    ValueError with these texts, the library untouched.  True is PARK_FINISHED; None, False and 0 are "no bits"; no cars is an empty int32 list."""
    from racinglmpc_amd import _capi
    ctx = object.__new__(_capi.Context)
    ctx.lib = _NoLibrary(); ctx._h = None; ctx._pid = -1
    for mode, cars, text in ((4, None, "parking: mode = 4 has unknown bits"), (-1, None, "parking: mode = -1 has unknown bits"), (7, [0], "parking: mode = 7 has unknown bits"),
                             (1, [0, -1], "parking: negative car index"), (1, [2, 0, 2], "parking: a car is listed twice"),
                             (1, [[0, 1]], "parking: cars must be one-dimensional"), (0, [0.5], "parking: cars must be integers")):
        with pytest.raises(ValueError) as e:
            _capi.check_parking(mode, cars)
        assert str(e.value) == text
        with pytest.raises(ValueError):
            ctx.rollout_set_parking(mode, cars)
    mode, cars = _capi.check_parking(True, [3, 0, 4])
    assert mode == _capi.PARK_FINISHED and cars.dtype == np.int32 and list(cars) == [3, 0, 4]              # (the order given is kept)
    for off in (None, False, 0):
        assert _capi.check_parking(off, None)[0] == 0
    for none in (None, [], np.zeros(0, np.int64)):
        mode, cars = _capi.check_parking(3, none)
        assert mode == 3 and cars.size == 0 and cars.dtype == np.int32


class _Recorder:
    """Stands where the device context stands for the lap runners: keeps the order of the calls and answers with scripted logs."""
    N = 12

    def __init__(self, numSS_it=4, done=(7, -1, 9)):
        self.cfg = type("cfg", (), dict(numSS_it=numSS_it, trToUse=4))()
        self.calls, self.done = [], np.array(done, np.int32)

    def rollout_set_parking(self, mode, cars):
        self.calls.append(("set_parking", int(mode), [int(c) for c in cars]))

    def rollout_parked_at(self):
        self.calls.append(("parked_at",)); return np.array([8, -1, 16], np.int32)[:self.B], 1

    def rollout_begin(self, x0, xg, xl, ul, noise, T_max=None):
        self.B = x0.shape[0]; self.calls.append(("begin",))

    def rollout_begin_mpc(self, x0, xg, noise, **kw):
        self.B = x0.shape[0]; self.calls.append(("begin_mpc",))

    def rollout_run(self, n):
        self.calls.append(("run", n)); return 10, 2

    def rollout_fetch(self, t0, t1):
        n, B = t1 - t0, self.B
        return np.zeros((n, B, 6)), np.zeros((n, B, 2)), np.zeros((n, B, 6)), self.done[:B], np.zeros(B, np.int32), np.zeros((B, 6)), np.zeros((B, 6))

    def rollout_end(self):
        self.calls.append(("end",))


def test_batched_rollouts_hand_the_parking_over():
    """BatchedRollouts(park=): True, a mode, or (mode, cars); rollout_set_parking before every begin and run_mpc_laps, where the trace goes; the parking steps are read
    before rollout_end and kept in last_parked_at; a listed car the session does not have is refused before the session begins; without park= the context is not
    touched and last_parked_at stays None."""
    from racinglmpc_amd import _capi, rollout
    x0 = np.zeros((3, 6)); xl = np.zeros((13, 6)); ul = np.zeros((12, 2)); track = np.zeros((3, 6)) + 1.0
    ctx = _Recorder()
    ro = rollout.BatchedRollouts(ctx, track, prefetch=False, park=(_capi.PARK_FINISHED | _capi.PARK_REROUTE, [2, 0]))
    assert ro.last_parked_at is None
    laps = ro.run_lap_device(x0, xl, ul, max_steps=20, keep_invalid=True)
    assert [c[0] for c in ctx.calls] == ["set_parking", "begin", "run", "parked_at", "end"] and ctx.calls[0] == ("set_parking", 3, [2, 0])
    assert len(laps) == 3 and list(ro.last_parked_at) == [8, -1, 16]
    with pytest.raises(ValueError) as e:
        ro.run_lap_device(x0[:2], xl, ul, max_steps=20)                                           # car 2 of a two-car session
    assert str(e.value) == "park: car 2 listed, the session has 2 cars" and [c[0] for c in ctx.calls].count("begin") == 1
    for park, want in ((True, (1, [])), (_capi.PARK_REROUTE, (2, [])), ((0, [1]), (0, [1]))):
        m = _Recorder(numSS_it=0)
        rm = rollout.BatchedRollouts(m, track, prefetch=False, park=park)
        rm.run_mpc_laps(x0, A=np.zeros((3, 6, 6)), B=np.zeros((3, 6, 2)), max_steps=20, keep_invalid=True)
        assert [c[0] for c in m.calls] == ["set_parking", "begin_mpc", "run", "parked_at", "end"] and m.calls[0] == ("set_parking",) + want
    for bad in ((1, [0], 2), 4, (1, [0, 0])):
        with pytest.raises(ValueError):
            rollout.BatchedRollouts(_Recorder(), track, prefetch=False, park=bad)
    plain = _Recorder()
    rp = rollout.BatchedRollouts(plain, track, prefetch=False)
    rp.run_lap_device(x0, xl, ul, max_steps=20, keep_invalid=True)
    assert [c[0] for c in plain.calls] == ["begin", "run", "end"] and rp.last_parked_at is None


def _loop(park, device_commit):
    """PerCarLMPC on the scripted context of tests/test_device_commit_host.py, which also records what parking it is handed."""
    from racinglmpc_amd import rollout
    from tests.test_device_commit_host import SCRIPT, _LoopCtx

    class Ctx(_LoopCtx):
        def __init__(self, *a):
            super().__init__(*a); self.parking = []; self.asked = 0

        def rollout_set_parking(self, mode, cars):
            self.parking.append((self.gen + 1, int(mode), [int(c) for c in cars]))

        def rollout_parked_at(self):
            self.asked += 1
            return np.full(self.B, -1, np.int32), self.B

    ctx = Ctx(3, 2, SCRIPT, ())
    ro = rollout.BatchedRollouts(ctx, np.array(common.load_lmpc_golden()["track"]), seed=1, prefetch=False)
    loop = rollout.PerCarLMPC(ro, T_max=60, ext=10, device_commit=device_commit, park=park)
    lap = lambda T, ends: (np.zeros((T, 6)), np.zeros((T, 2)), None, np.zeros(12), T if ends else T - 20, 0)
    loop.seed([lap(50, True), [lap(70, True), lap(60, True)], lap(80, False), [lap(90, False)]])
    gens = []
    for _ in range(len(SCRIPT)):
        before = sorted(loop.retired)
        out = loop.run()
        gens.append(dict(before=before, out=[None if o is None else (o[4], o[5]) for o in out], retired=dict(loop.retired), lap_times=[list(t) for t in loop.lap_times],
                         ss_table=ro.ss_table.tolist(), ss_last=ro.ss_last.tolist(), lap_table=ro.lap_table.tolist()))
    return ctx, loop, ro, gens


@pytest.mark.parametrize("device_commit", [False, True], ids=["host", "device_commit"])
def test_per_car_lmpc_parks_its_retired_cars(device_commit):
    """PerCarLMPC(park=True): before every begin the context is handed PARK_FINISHED and the cars retired so far, in ascending order; the books come out as
    without it.  park=False: the context's parking is never touched and never asked for."""
    from racinglmpc_amd import _capi
    c0, l0, r0, g0 = _loop(False, device_commit)
    c1, l1, r1, g1 = _loop(True, device_commit)
    assert c0.parking == [] and c0.asked == 0 and r0.park is None and r0.last_parked_at is None
    assert c1.parking == [(gen, _capi.PARK_FINISHED, g["before"]) for gen, g in enumerate(g1)]
    assert c1.parking[0][2] == [] and any(p[2] for p in c1.parking) and set(c1.parking[-1][2]) <= set(l1.retired)
    assert g0 == g1 and c0.ss == c1.ss and c0.model == c1.model and c0.rows == c1.rows and c0.extended == c1.extended
    assert len(l1.steps) == len(g1) and l0.steps == l1.steps                                    # (the scripted context takes the same steps either way)
    assert r1.last_parked_at is not None and c1.asked >= len(g1)
