"""ctypes binding of liblmpc_hip.so (C ABI: include/lmpc_hip.h).  NumPy in, NumPy out.

The library is the only compute path: importing this module without a built .so, or calling into it
without a working HIP device, raises -- there is no CPU fallback.
"""
import ctypes as C
import os
import subprocess
import warnings

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LMPC_LIB") or os.path.join(_HERE, "liblmpc_hip.so")      # LMPC_LIB: developer builds (build.build_flavour)

MAX_TRACK_ROWS = 16
MAX_USED_LAPS = 32
COMM_ID_BYTES = 128
E_VARIANT = -5
CREATE_RUNTIME_KERNEL, CREATE_FORCE_RUNTIME_KERNEL, CREATE_NO_K1_AHEAD, CREATE_NO_K1_MERGE = 1, 2, 4, 8

ST_MAXITER, ST_REG_SINGULAR, ST_NO_SEGMENT, ST_WINDOW, ST_NUMERIC, ST_NOT_INTERIOR, ST_INEXACT, ST_INFEASIBLE = 1, 2, 4, 8, 16, 32, 64, 128

PLANT_NPAR = 10
COMMIT_SS, COMMIT_MODEL = 1, 2         # LMPC_COMMIT_SS / LMPC_COMMIT_MODEL: the `stores` bits of lmpc_rollout_commit_laps
# One row of lap metrics (lmpc_rollout_lap_metrics): name -> column, the LMPC_MET_* enumerators of include/lmpc_hip.h in their order.
METRICS_NCOL = 20
METRIC_FIELDS = {name: k for k, name in enumerate((
    "rows", "t_cross", "nonfinite_rows", "vx_min", "vx_max", "vx_sum", "ey_absmax", "ey_absmax_row", "epsi_absmax", "alat_absmax", "lane_excess_max",
    "lane_excess_rows", "lane_excess_sum", "lane_excess_sqsum", "input_margin_min", "du0_sqsum", "du1_sqsum", "cost_state", "cost_input", "path_length"))}


def metrics_stage_cost(metrics, dR, Qslack):
    """The realised stage cost of buildCost (PredictiveControllers.py:228-257) from rows of lap metrics: cost_state + cost_input + dR . du_sqsum +
    Qslack[0] lane_excess_sqsum + Qslack[1] lane_excess_sum.  dR, Qslack: (2,) for all rows, or one pair per row -- the caller's own tuning."""
    m, F = np.asarray(metrics, float), METRIC_FIELDS
    dR, Qs = np.asarray(dR, float), np.asarray(Qslack, float)
    return (m[..., F["cost_state"]] + m[..., F["cost_input"]] + dR[..., 0] * m[..., F["du0_sqsum"]] + dR[..., 1] * m[..., F["du1_sqsum"]]
            + Qs[..., 0] * m[..., F["lane_excess_sqsum"]] + Qs[..., 1] * m[..., F["lane_excess_sum"]])


def metrics_report(per_generation, dR, Qslack, fields=("t_cross", "ey_absmax", "lane_excess_max", "input_margin_min", "alat_absmax")):
    """What the sweep tools print of PerCarLMPC(metrics=True).metrics: {name: [car][generation]} for `fields` and "stage_cost" (metrics_stage_cost under dR, Qslack:
    (2,) or one pair per car), plain floats with None where a car has no lap in that generation -- ready for json.dump."""
    m = np.stack([np.asarray(p, float) for p in per_generation], axis=1)                           # (B, G, METRICS_NCOL)
    dR, Qs = np.asarray(dR, float), np.asarray(Qslack, float)
    cost = metrics_stage_cost(m, dR[:, None, :] if dR.ndim == 2 else dR, Qs[:, None, :] if Qs.ndim == 2 else Qs)
    cols = {name: m[..., METRIC_FIELDS[name]] for name in fields}
    cols["stage_cost"] = cost
    return {name: [[None if np.isnan(v) else float(v) for v in row] for row in a] for name, a in cols.items()}
# LMPC_TRACE_*: the planes of a session trace (lmpc_rollout_set_trace), the per-step logs of LMPC.unpackSolution (PredictiveControllers.py:364-379) among them
TRACE_XPRED, TRACE_UPRED, TRACE_SS, TRACE_QSEL, TRACE_SOLVER, TRACE_XY = 1, 2, 4, 8, 16, 32
TRACE_ALL = 63
TRACE_DEFAULT = None                   # rollout_set_trace(what=TRACE_DEFAULT): every plane the context can record (no SS / QSEL without a safe set)
# LMPC_PARK_*: parking (lmpc_rollout_set_parking) -- FINISHED: a car leaves the launches of a session that stops at the line at the first poll after its crossing step;
# REROUTE: the solve-kernel route follows the live count instead of the session's B
PARK_FINISHED, PARK_REROUTE = 1, 2
PLANT_PARAM_NAMES = ("m", "lf", "lr", "Iz", "Df", "Cf", "Bf", "Dr", "Cr", "Br")       # one row of vehicle constants, the order of SysModel.py:60-70


class LmpcConfig(C.Structure):
    _fields_ = [
        ("N", C.c_int), ("numSS_it", C.c_int), ("numSS_points", C.c_int), ("trToUse", C.c_int), ("maxNumPoint", C.c_int),
        ("h", C.c_double), ("lamb", C.c_double), ("dt", C.c_double), ("scaling", C.c_double * 5),
        ("Q", C.c_double * 36), ("R", C.c_double * 4), ("Qf", C.c_double * 36), ("dR", C.c_double * 2), ("Qslack", C.c_double * 2),
        ("QtermSlack", C.c_double * 36), ("xRef", C.c_double * 6),
        ("Fx", C.c_double * 12), ("bx", C.c_double * 2), ("Fu", C.c_double * 8), ("bu", C.c_double * 4),
        ("track", C.c_double * (MAX_TRACK_ROWS * 6)), ("track_rows", C.c_int), ("trackLength", C.c_double),
        ("device", C.c_int), ("max_batch", C.c_int), ("max_laps", C.c_int), ("max_lap_len", C.c_int),
        ("tol_gap", C.c_double), ("tol_res", C.c_double), ("reg_lambda", C.c_double), ("max_iter", C.c_int), ("slacks", C.c_int),
    ]


class LmpcStats(C.Structure):
    _fields_ = [("ms_regress", C.c_double), ("ms_solve", C.c_double), ("n_regress", C.c_longlong), ("n_solve", C.c_longlong),
                ("qp_solved", C.c_longlong), ("ipm_iters", C.c_longlong), ("n_regress_timed", C.c_longlong), ("n_solve_timed", C.c_longlong), ("n_retry", C.c_longlong)]


# The per-problem arrays of a step, stated once on this side (the library's statement: csrc/lmpc_arrays.h): key of the entry points below, member of lmpc_step_dev_args (None: the
# selection's own outputs; the members come first, in the C struct's order: StepDevArgs mirrors it), dtype, role, shape for B problems (N1 = N + 1, N2 = 2 N, M = 8 N + S, L1 = max(numSS_it, 1)).
_f8, _i4 = np.float64, np.int32
ARRAYS = (
    ("x0", "x0", _f8, "in", "B 6"), ("xLin", "xLin", _f8, "in", "B N1 6"), ("uLin", "uLin", _f8, "in", "B N 2"), ("uOld", "uOld", _f8, "in", "B 2"),
    ("zt", "zt", _f8, "in", "B 6"), ("xPredPrev", "xPredPrev", _f8, "in", "B N1 6"), ("hasPred", "hasPred", _i4, "in", "B"), ("timeStep", "timeStep", _i4, "in", "B"),
    ("xPred", "xPred", _f8, "out", "B N1 6"), ("uPred", "uPred", _f8, "out", "B N 2"), ("slack", "slack", _f8, "out", "B N2"), ("lambd", "lambda_", _f8, "out", "B S"),
    ("sTerm", "sTerm", _f8, "out", "B 6"), ("ztNext", "ztNext", _f8, "out", "B 6"), ("ztuNext", "ztuNext", _f8, "out", "B 2"), ("ssSel", "ssSel", _f8, "out", "B S 6"),
    ("A", "A", _f8, "out", "B N 6 6"), ("B", "Bm", _f8, "out", "B N 6 2"), ("C", "C", _f8, "out", "B N 6"), ("mu", "mu", _f8, "out", "B M"),
    ("resid", "resid", _f8, "out", "B 3"), ("status", "status", _i4, "out", "B"), ("iters", "iters", _i4, "out", "B"), ("qSel", "qSel", _f8, "out", "B S"),
    ("succ", None, _f8, "select", "B S 6"), ("succU", None, _f8, "select", "B S 2"), ("ztUsed", None, _f8, "select", "B 6"), ("selStart", None, _i4, "select", "B L1"),
)
STEP_IN_KEYS, STEP_OUT_KEYS = (tuple(k for k, f, dt, role, shp in ARRAYS if role == r) for r in ("in", "out"))     # STEP_OUT_KEYS: what step_batch and step_dev_fetch return
QP_OUT_KEYS = ("xPred", "uPred", "slack", "lambd", "sTerm", "mu", "status", "iters", "resid")         # qp_solve_batch, in the order of its arguments
SELECT_OUT_KEYS = ("ssSel", "qSel", "succ", "succU", "ztUsed", "selStart", "status")                 # select_batch, in the order of its arguments
DIAGNOSTIC_KEYS = ("qSel", "mu", "resid")                                                             # step_dev_buffers(diagnostics=False) leaves them NULL
_FIELD = {k: f for k, f, dt, role, shp in ARRAYS}


def array_specs(B, N, S, numSS_it, keys=None):
    """{key: (shape, dtype)} of the arrays of ARRAYS (all, or `keys` in the order given) for B problems of horizon N with S safe-set points in use."""
    d = dict(B=B, N=N, N1=N + 1, N2=2 * N, S=S, M=8 * N + S, L1=max(numSS_it, 1))
    spec = {k: (tuple(d[t] if t in d else int(t) for t in shp.split()), dt) for k, f, dt, role, shp in ARRAYS}
    return spec if keys is None else {k: spec[k] for k in keys}


class StepDevArgs(C.Structure):
    _fields_ = [(f, C.c_void_p) for k, f, dt, role, shp in ARRAYS if f is not None]


class TraceOut(C.Structure):
    """lmpc_trace_out: one pointer per plane, NULL = not wanted."""
    _fields_ = [(k, C.c_void_p) for k in ("xPred", "uPred", "ssSel", "qSel", "xyPred", "xySS", "iters", "status", "mapStatus")]


def trace_planes(N, S, what):
    """The planes a session trace of `what` records at horizon N with S safe-set points in use (0 without a safe set), in the order of lmpc_trace_out:
    [(key, bit, shape per (step, car), dtype)].  XY records xyPred, mapStatus and -- with a safe set -- xySS."""
    table = (("xPred", TRACE_XPRED, (N + 1, 6), _f8), ("uPred", TRACE_UPRED, (N, 2), _f8), ("ssSel", TRACE_SS, (S, 6), _f8), ("qSel", TRACE_QSEL, (S,), _f8),
             ("xyPred", TRACE_XY, (N + 1, 2), _f8), ("xySS", TRACE_XY, (S, 2), _f8), ("iters", TRACE_SOLVER, (), _i4), ("status", TRACE_SOLVER, (), _i4),
             ("mapStatus", TRACE_XY, (), _i4))
    return [(k, bit, shp, dt) for k, bit, shp, dt in table if (what & bit) and int(np.prod(shp)) > 0]


def trace_bytes(N, S, n, what, T_max):
    """What lmpc_rollout_trace_bytes returns: T_max x n x the bytes of the recorded planes per (step, car)."""
    return int(T_max) * int(n) * sum(int(np.prod(shp)) * np.dtype(dt).itemsize for k, bit, shp, dt in trace_planes(N, S, what))


def check_trace(cars, what, numSS_it):
    """(cars as int32, what) of a rollout_set_trace call, or ValueError for what the library refuses with LMPC_E_ARG: no planes or unknown bits, a negative or repeated
    car, SS / QSEL without a safe set.  what=None: every plane the context can record.  No cars: (empty, 0), the trace is off."""
    cars = np.zeros(0, np.int32) if cars is None else np.asarray(cars)
    if cars.ndim != 1:
        raise ValueError("trace: cars must be one-dimensional")
    if cars.size and not np.issubdtype(cars.dtype, np.integer):
        raise ValueError("trace: cars must be integers")
    cars = _i32(cars)
    if cars.size == 0:
        return cars, 0
    if what is None:
        what = TRACE_ALL if numSS_it > 0 else TRACE_ALL & ~(TRACE_SS | TRACE_QSEL)
    what = int(what)
    if what <= 0 or what & ~TRACE_ALL:
        raise ValueError("trace: what = %d names no plane or an unknown one" % what)
    if (cars < 0).any():
        raise ValueError("trace: negative car index")
    if np.unique(cars).size != cars.size:
        raise ValueError("trace: a car is listed twice")
    if numSS_it == 0 and what & (TRACE_SS | TRACE_QSEL):
        raise ValueError("trace: SS / QSEL planes need a context with a safe set (numSS_it > 0)")
    return cars, what


def check_parking(mode, cars):
    """(mode, cars as int32) of a rollout_set_parking call, or ValueError for what the library refuses with LMPC_E_ARG: unknown mode bits, a negative or repeated
    car.  mode may be True (PARK_FINISHED) or False / None (0); cars None: no car parked from step 0."""
    mode = PARK_FINISHED if mode is True else 0 if mode is None or mode is False else int(mode)
    if mode < 0 or mode & ~(PARK_FINISHED | PARK_REROUTE):
        raise ValueError("parking: mode = %d has unknown bits" % mode)
    cars = np.zeros(0, np.int32) if cars is None else np.asarray(cars)
    if cars.ndim != 1:
        raise ValueError("parking: cars must be one-dimensional")
    if cars.size and not np.issubdtype(cars.dtype, np.integer):
        raise ValueError("parking: cars must be integers")
    cars = _i32(cars)
    if (cars < 0).any():
        raise ValueError("parking: negative car index")
    if np.unique(cars).size != cars.size:
        raise ValueError("parking: a car is listed twice")
    return mode, cars


def check_relaunch(cars, lap_rows):
    """(cars as int32, lap_rows) of a rollout_relaunch call, or ValueError for what the library refuses with LMPC_E_ARG whatever the session: no car, a negative or
    repeated car, lap_rows < 1.  (A car beyond the session's B, one that has not crossed the line and a lap shorter than N + 2 rows are the session's to refuse.)"""
    cars = np.asarray(cars)
    if cars.ndim == 0:
        cars = cars.reshape(1)
    if cars.ndim != 1:
        raise ValueError("relaunch: cars must be one-dimensional")
    if cars.size == 0:
        raise ValueError("relaunch: at least one car expected")
    if not np.issubdtype(cars.dtype, np.integer):
        raise ValueError("relaunch: cars must be integers")
    cars = _i32(cars)
    if (cars < 0).any():
        raise ValueError("relaunch: negative car index")
    if np.unique(cars).size != cars.size:
        raise ValueError("relaunch: a car is listed twice")
    if isinstance(lap_rows, bool) or not isinstance(lap_rows, (int, np.integer)):
        raise ValueError("relaunch: lap_rows must be an integer")
    if int(lap_rows) < 1:
        raise ValueError("relaunch: lap_rows = %d, at least one row expected" % int(lap_rows))
    return cars, int(lap_rows)


EXPORTS = [
    "lmpc_config_default", "lmpc_create", "lmpc_create_ex", "lmpc_solver_kind", "lmpc_destroy", "lmpc_last_error", "lmpc_active_knobs", "lmpc_version", "lmpc_device_memory",
    "lmpc_model_add_trajectory", "lmpc_model_num_laps", "lmpc_model_replace_lap", "lmpc_model_set_lap_table", "lmpc_model_get_lap_table", "lmpc_model_lap_info",
    "lmpc_ss_add_trajectory", "lmpc_ss_add_point", "lmpc_ss_replace_lap", "lmpc_ss_set_selected", "lmpc_ss_set_lap_table", "lmpc_ss_get_lap_table", "lmpc_ss_num_laps", "lmpc_ss_get_qfun", "lmpc_ss_get_laptime", "lmpc_store_read_lap",
    "lmpc_regress_batch", "lmpc_regress_points", "lmpc_select_batch", "lmpc_qp_solve_batch", "lmpc_step_batch", "lmpc_assemble_batch", "lmpc_qp_dims",
    "lmpc_dev_alloc", "lmpc_dev_free", "lmpc_dev_upload", "lmpc_dev_download", "lmpc_dev_sync", "lmpc_step_batch_dev",
    "lmpc_lti_regression", "lmpc_lti_regression_batch", "lmpc_comm_unique_id", "lmpc_comm_init", "lmpc_comm_destroy", "lmpc_comm_info", "lmpc_comm_allgather_dev", "lmpc_comm_allgather",
    "lmpc_comm_allreduce_max", "lmpc_comm_barrier", "lmpc_rollout_exchange",
    "lmpc_set_profiling", "lmpc_get_stats", "lmpc_reset_stats", "lmpc_selftest", "lmpc_solver_waves", "lmpc_solver_lds", "lmpc_plant_step_batch", "lmpc_plant_params_default", "lmpc_plant_set_params", "lmpc_plant_get_params", "lmpc_noise_raw", "lmpc_noise_fill", "lmpc_rollout_set_noise", "lmpc_rollout_get_noise", "lmpc_global_position_batch", "lmpc_local_position_batch", "lmpc_track_angle_batch", "lmpc_state_from_global_batch", "lmpc_rollout_begin", "lmpc_rollout_begin_mpc", "lmpc_rollout_pid", "lmpc_rollout_run", "lmpc_rollout_fetch", "lmpc_rollout_end", "lmpc_rollout_release", "lmpc_ss_extend_lap", "lmpc_ss_truncate_lap",
    "lmpc_rollout_commit_laps", "lmpc_rollout_extend_laps", "lmpc_rollout_lap_metrics", "lmpc_debug_model_image", "lmpc_tuning_from_config", "lmpc_tuning_set", "lmpc_tuning_get",
    "lmpc_track_row_from_config", "lmpc_track_set", "lmpc_track_get", "lmpc_ss_add_trajectory_on", "lmpc_ss_extend_lap_on",
    "lmpc_rollout_set_trace", "lmpc_rollout_get_trace", "lmpc_rollout_trace_bytes", "lmpc_rollout_fetch_trace",
    "lmpc_rollout_set_parking", "lmpc_rollout_get_parking", "lmpc_rollout_parked_at", "lmpc_debug_live_compact",
    "lmpc_debug_set_trace", "lmpc_debug_exec_audit", "lmpc_debug_rollout_peek", "lmpc_debug_rollout_capture", "lmpc_debug_rollout_qp",
    "lmpc_debug_k1_ahead", "lmpc_debug_k1_merge", "lmpc_dev_flush", "lmpc_store_retain",
    "lmpc_rollout_relaunch", "lmpc_rollout_lap_start",
]

_lib = None


class LmpcError(RuntimeError):
    pass


def load():
    """dlopen liblmpc_hip.so (built by racinglmpc_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LmpcError("liblmpc_hip.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`. "
                            "There is no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name in EXPORTS:
            getattr(lib, name)          # raises AttributeError if a declared symbol is missing
        lib.lmpc_last_error.restype = C.c_char_p
        lib.lmpc_active_knobs.restype = C.c_char_p
        # (declared argument types let the hot call take plain integers as addresses: no c_void_p object per array)
        lib.lmpc_step_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 24
        # (the batched stages of main.py:61-95, argument types as include/lmpc_hip.h declares them)
        lib.lmpc_rollout_begin_mpc.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int]
        lib.lmpc_rollout_pid.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.lmpc_lti_regression_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 4
        # (device noise: 64-bit seeds, laps and car indices must not pass through ctypes' default int conversion)
        lib.lmpc_noise_raw.argtypes = [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_void_p]
        lib.lmpc_noise_fill.argtypes = [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
        lib.lmpc_rollout_set_noise.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_longlong]
        lib.lmpc_rollout_get_noise.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_longlong)]
        # (inverse track map: max_ey is a double passed by value)
        lib.lmpc_local_position_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lmpc_track_angle_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lmpc_state_from_global_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        # (per-problem regression laps: rows of int32 insertion indices)
        lib.lmpc_model_set_lap_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.lmpc_model_get_lap_table.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]
        lib.lmpc_model_lap_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.lmpc_model_set_lap_table.restype = lib.lmpc_model_get_lap_table.restype = lib.lmpc_model_lap_info.restype = C.c_int
        # (per-problem safe-set laps: rows of int32 lap indices, one "latest lap" index per row)
        lib.lmpc_ss_set_lap_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.lmpc_ss_get_lap_table.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_int]
        lib.lmpc_ss_set_lap_table.restype = lib.lmpc_ss_get_lap_table.restype = C.c_int
        # (laps of a session committed on the device: int32 tables in, int32 / packed words out)
        lib.lmpc_rollout_commit_laps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.lmpc_rollout_extend_laps.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.lmpc_debug_model_image.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        lib.lmpc_rollout_commit_laps.restype = lib.lmpc_rollout_extend_laps.restype = lib.lmpc_debug_model_image.restype = C.c_int
        # (lap metrics reduced on the device: int32 tables in, rows of METRICS_NCOL doubles out)
        lib.lmpc_rollout_lap_metrics.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lmpc_rollout_lap_metrics.restype = C.c_int
        # (per-problem controller tuning: rows of TUNING_NPAR doubles)
        lib.lmpc_tuning_from_config.argtypes = [C.c_void_p, C.c_void_p]
        lib.lmpc_tuning_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.lmpc_tuning_get.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]
        lib.lmpc_tuning_from_config.restype = lib.lmpc_tuning_set.restype = lib.lmpc_tuning_get.restype = C.c_int
        # (per-car tracks: rows of TRACK_NPAR doubles)
        lib.lmpc_track_row_from_config.argtypes = [C.c_void_p, C.c_void_p]
        lib.lmpc_track_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.lmpc_track_get.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_int]
        lib.lmpc_ss_add_trajectory_on.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        lib.lmpc_ss_extend_lap_on.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        for f in (lib.lmpc_track_row_from_config, lib.lmpc_track_set, lib.lmpc_track_get, lib.lmpc_ss_add_trajectory_on, lib.lmpc_ss_extend_lap_on):
            f.restype = C.c_int
        # (session traces: an int32 car list, plane bits, a struct of plane pointers)
        lib.lmpc_rollout_set_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
        lib.lmpc_rollout_get_trace.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_uint), C.c_int]
        lib.lmpc_rollout_trace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_int, C.POINTER(C.c_longlong)]
        lib.lmpc_rollout_fetch_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(TraceOut)]
        for f in (lib.lmpc_rollout_set_trace, lib.lmpc_rollout_get_trace, lib.lmpc_rollout_trace_bytes, lib.lmpc_rollout_fetch_trace):
            f.restype = C.c_int
        # (parking: mode bits, an int32 car list; the compaction kernel between int32 host arrays)
        lib.lmpc_rollout_set_parking.argtypes = [C.c_void_p, C.c_uint, C.c_int, C.c_void_p]
        lib.lmpc_rollout_get_parking.argtypes = [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_int), C.c_void_p, C.c_int]
        lib.lmpc_rollout_parked_at.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        lib.lmpc_debug_live_compact.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        for f in (lib.lmpc_rollout_set_parking, lib.lmpc_rollout_get_parking, lib.lmpc_rollout_parked_at, lib.lmpc_debug_live_compact):
            f.restype = C.c_int
        # (laps given back: two int32 keep lists in, two int32 maps out)
        lib.lmpc_store_retain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lmpc_store_retain.restype = C.c_int
        # (free-running sessions: an int32 car list in; two int32 arrays out)
        lib.lmpc_rollout_relaunch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        lib.lmpc_rollout_lap_start.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lmpc_rollout_relaunch.restype = lib.lmpc_rollout_lap_start.restype = C.c_int
        for f in (lib.lmpc_rollout_begin_mpc, lib.lmpc_rollout_pid, lib.lmpc_lti_regression_batch, lib.lmpc_noise_raw, lib.lmpc_noise_fill, lib.lmpc_rollout_set_noise,
                  lib.lmpc_rollout_get_noise, lib.lmpc_local_position_batch, lib.lmpc_track_angle_batch, lib.lmpc_state_from_global_batch):
            f.restype = C.c_int
        _lib = lib
    return _lib


def active_knobs():
    """Developer environment variables the library has acted on in this process ([] = none): route / grid choices, results identical."""
    v = load().lmpc_active_knobs().decode()
    return v.split(";") if v else []


def device_memory(device=0):
    """(free, total) bytes of HBM on `device` (hipMemGetInfo)."""
    f, t = C.c_ulonglong(), C.c_ulonglong()
    _chk(load().lmpc_device_memory(C.c_int(device), C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def comm_unique_id():
    """ncclGetUniqueId (call on rank 0, hand the bytes to the other ranks)."""
    buf = (C.c_ubyte * COMM_ID_BYTES)()
    _chk(load().lmpc_comm_unique_id(buf))
    return bytes(buf)


def lti_regression(x, u, lamb, device=0):
    """Utilities.Regression on the GPU: returns (A (6,6), B (6,2), Error (2,6), status)."""
    x = np.ascontiguousarray(x, dtype=np.float64); u = np.ascontiguousarray(u, dtype=np.float64)
    assert x.ndim == 2 and x.shape[1] == 6 and u.shape == (x.shape[0], 2), (x.shape, u.shape)
    A = np.zeros((6, 6)); B = np.zeros((6, 2)); E = np.zeros((2, 6)); st = C.c_int()
    _chk(load().lmpc_lti_regression(C.c_int(int(device)), _d(x), _d(u), C.c_int(x.shape[0]), C.c_double(float(lamb)), _d(A), _d(B), _d(E), C.byref(st)))
    return A, B, E, st.value


def lti_regression_batch(laps, lamb, device=0):
    """Utilities.Regression for a batch of laps [(x (T_b, 6), u (T_b, 2)), ...] of any lengths in one launch (lmpc_lti_regression_batch):
    returns (A (B, 6, 6), B (B, 6, 2), Error (B, 2, 6), status (B,))."""
    laps = [(_f64(x), _f64(u)) for x, u in laps]
    n = len(laps)
    assert n >= 1 and all(x.ndim == 2 and x.shape[1] == 6 and u.shape == (x.shape[0], 2) for x, u in laps)
    T = _i32([x.shape[0] for x, _ in laps]); ld = int(T.max())
    X = np.zeros((n, ld, 6)); U = np.zeros((n, ld, 2))
    for b, (x, u) in enumerate(laps):
        X[b, :T[b]] = x; U[b, :T[b]] = u
    A = np.zeros((n, 6, 6)); Bm = np.zeros((n, 6, 2)); E = np.zeros((n, 2, 6)); st = np.zeros(n, np.int32)
    _chk(load().lmpc_lti_regression_batch(int(device), n, X.ctypes.data, U.ctypes.data, T.ctypes.data, ld, float(lamb), A.ctypes.data, Bm.ctypes.data, E.ctypes.data, st.ctypes.data))
    return A, Bm, E, st


def plant_params_default():
    """The reference's vehicle (SysModel.py:60-70) as one row of PLANT_PARAM_NAMES (lmpc_plant_params_default: needs the library, not a device)."""
    par = np.zeros(PLANT_NPAR)
    _chk(load().lmpc_plant_params_default(_d(par)))
    return par


def _check_rows(rows, width, label, allow_none, values=None):
    """What every check of float rows opens with: None for "no rows" (allow_none: None or empty), else (n, width) float64 rows, a flat row being one row; ValueError
    under `label` for another shape or a non-finite entry.  values: how the message names a row's entries (default "<width> values")."""
    if allow_none and (rows is None or np.size(rows) == 0):
        return None
    r = np.array(rows, dtype=np.float64, ndmin=2)
    if r.ndim != 2 or r.shape[1] != width:
        raise ValueError("%s: rows of %s expected, got shape %s" % (label, values or "%d values" % width, r.shape))
    if not np.all(np.isfinite(r)):
        raise ValueError("%s: non-finite entry in row(s) %s" % (label, np.where(~np.isfinite(r).all(1))[0].tolist()))
    return np.ascontiguousarray(r)


def check_plant_params(par):
    """(n, 10) float64 rows, or ValueError for what lmpc_plant_set_params refuses: a wrong shape, a non-finite entry, m <= 0 or Iz <= 0."""
    par = _check_rows(par, PLANT_NPAR, "plant parameters", False, "%d values %s" % (PLANT_NPAR, PLANT_PARAM_NAMES))
    if not (np.all(par[:, 0] > 0) and np.all(par[:, 3] > 0)):
        raise ValueError("plant parameters: m and Iz must be positive (rows %s)" % np.where(~((par[:, 0] > 0) & (par[:, 3] > 0)))[0].tolist())
    return par


def _check_lap_rows(rows, L, label, width_name):
    """The shape rule of both lap tables: (n, L) int32 rows of lap indices, or None for "no table" (None or no rows); ValueError under `label`, which calls the row
    width `width_name`.  A flat list is one row per entry when L is 1, else one row."""
    if rows is None or np.size(rows) == 0:
        return None
    L = int(L)
    a = np.asarray(rows)
    if L < 1 or not np.issubdtype(a.dtype, np.integer) or a.ndim > 2:
        raise ValueError("%s: integer rows of %s = %d lap indices expected, got dtype %s, shape %s" % (label, width_name, L, a.dtype, a.shape))
    if a.ndim < 2:
        a = a.reshape(-1, 1) if L == 1 else a.reshape(1, -1)
    if a.shape[1] != L:
        raise ValueError("%s: rows of %s = %d lap indices expected, got shape %s" % (label, width_name, L, a.shape))
    if a.min() < 0:
        raise ValueError("%s: negative lap index in row(s) %s" % (label, np.where((a < 0).any(1))[0].tolist()))
    return np.ascontiguousarray(a, dtype=np.int32)


def check_lap_table(rows, trToUse):
    """(n, trToUse) int32 rows of a per-problem lap table, or None for "no table" (None or no rows); ValueError for a shape that is not rows of trToUse entries or
    for a negative index (the library checks the upper end against the laps stored).  A flat list is one row per entry when trToUse is 1, else one row."""
    return _check_lap_rows(rows, trToUse, "lap table", "trToUse")


SS_LAST_SHARED = -2        # LMPC_SS_LAST_SHARED: lmpc_ss_get_lap_table's `last` entries when the table was set without one


def check_ss_table(rows, numSS_it, last=None):
    """(rows (n, numSS_it) int32, last (n,) int32 or None) of a per-problem safe-set lap table, or (None, None) for "no table" (rows None or empty).  The shape
    rules are check_lap_table's, with numSS_it entries per row.  last: one integer entry per row, each -1 ("none of the row's laps is the car's latest") or a lap
    index; ValueError for another shape, a non-integer dtype, an entry below -1, or a `last` given without rows (the library checks the upper ends against the
    laps stored)."""
    r = _check_lap_rows(rows, numSS_it, "safe-set lap table", "numSS_it")
    if r is None:
        if last is not None and np.size(last):
            raise ValueError("safe-set lap table: `last` given without rows")
        return None, None
    if last is None:
        return r, None
    a = np.asarray(last)
    if not np.issubdtype(a.dtype, np.integer) or a.ndim > 1 or a.size != r.shape[0]:
        raise ValueError("safe-set lap table: `last` must hold one integer per row (%d), got dtype %s, shape %s" % (r.shape[0], a.dtype, a.shape))
    a = a.reshape(-1)
    if a.min() < -1:
        raise ValueError("safe-set lap table: `last` below -1 in row(s) %s" % np.where(a < -1)[0].tolist())
    return r, np.ascontiguousarray(a, dtype=np.int32)


def check_retain(keep, stored, what):
    """The keep list of one store for Context.store_retain as an int32 array, or ValueError for what lmpc_store_retain refuses with LMPC_E_ARG: `stored` laps are in
    the store `what` names ("safe set" / "regression store"); the list holds strictly ascending lap indices in [0, stored).  An empty list empties the store."""
    a = np.asarray(keep)
    if a.ndim != 1:
        raise ValueError("store_retain: %s: a one-dimensional list of lap indices expected, got shape %s" % (what, a.shape))
    if a.size == 0:
        return np.zeros(0, np.int32)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("store_retain: %s: integer lap indices expected, got dtype %s" % (what, a.dtype))
    if a.min() < 0:
        raise ValueError("store_retain: %s: negative lap index at position(s) %s" % (what, np.where(a < 0)[0].tolist()))
    if a.max() >= int(stored):
        raise ValueError("store_retain: %s: position(s) %s name a lap that is not stored (%d laps are)" % (what, np.where(a >= int(stored))[0].tolist(), int(stored)))
    if (np.diff(a) <= 0).any():
        k = int(np.where(np.diff(a) <= 0)[0][0]) + 1
        raise ValueError("store_retain: %s: strictly ascending lap indices expected, position %d holds %d after %d" % (what, k, int(a[k]), int(a[k - 1])))
    return np.ascontiguousarray(a, dtype=np.int32)


def plant_params(B, m=1.98, lf=0.125, lr=0.125, Iz=0.024, mu_f=0.8, mu_r=0.8, Cf=1.25, Bf=1.0, Cr=1.25, Br=1.0, Df=None, Dr=None):
    """(B, 10) rows of vehicle constants for Context.plant_set_params, columns PLANT_PARAM_NAMES; needs neither the library nor a device.  Every argument is a
    scalar or a (B,) array.  The peak tyre forces are D = mu * m * 9.81 / 2.0, evaluated left to right as SysModel.py:68, 73 do (the defaults give the reference's
    bits), unless Df / Dr are given.  Raises ValueError on what lmpc_plant_set_params would refuse."""
    B = int(B)
    if B < 1:
        raise ValueError("plant_params: B must be at least 1")

    def col(name, v):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != B):
            raise ValueError("plant_params: %s must be a scalar or a (%d,) array, got shape %s" % (name, B, v.shape))
        return np.broadcast_to(v, (B,)).astype(np.float64)
    m = col("m", m)
    Df = col("mu_f", mu_f) * m * 9.81 / 2.0 if Df is None else col("Df", Df)
    Dr = col("mu_r", mu_r) * m * 9.81 / 2.0 if Dr is None else col("Dr", Dr)
    cols = [m, col("lf", lf), col("lr", lr), col("Iz", Iz), Df, col("Cf", Cf), col("Bf", Bf), Dr, col("Cr", Cr), col("Br", Br)]
    return check_plant_params(np.stack(cols, axis=1))


# One row of controller tuning (lmpc_tuning_set): name -> slice of the row, in the order of include/lmpc_hip.h.  The values of LmpcConfig; QtermSlack is the diagonal.
TUNING_NPAR = 98
TUNING_FIELDS = {"Q": slice(0, 36), "R": slice(36, 40), "Qf": slice(40, 76), "dR": slice(76, 78), "Qslack": slice(78, 80), "QtermSlack": slice(80, 86),
                 "xRef": slice(86, 92), "bx": slice(92, 94), "bu": slice(94, 98)}
_TUNING_SHAPES = {"Q": (6, 6), "R": (2, 2), "Qf": (6, 6), "dR": (2,), "Qslack": (2,), "QtermSlack": (6,), "xRef": (6,), "bx": (2,), "bu": (4,)}


def check_tuning(rows, numSS_it=0):
    """(n, 98) float64 rows, or None for "no rows" (None or empty); ValueError for what lmpc_tuning_set refuses in a row: a wrong shape, a non-finite entry, Q, R or
    Qf not exactly symmetric, a negative dR or Qslack entry, and (numSS_it > 0) a QtermSlack entry <= 0.  bu <= 0 is no error here either (LMPC_ST_NOT_INTERIOR)."""
    r = _check_rows(rows, TUNING_NPAR, "tuning", True)
    if r is None:
        return None
    for name in ("Q", "R", "Qf"):
        m = r[:, TUNING_FIELDS[name]].reshape((-1,) + _TUNING_SHAPES[name])
        if not np.array_equal(m, m.transpose(0, 2, 1)):
            raise ValueError("tuning: %s must be exactly symmetric" % name)
    for name in ("dR", "Qslack"):
        if (r[:, TUNING_FIELDS[name]] < 0).any():
            raise ValueError("tuning: negative %s entry" % name)
    if int(numSS_it) > 0 and not (r[:, TUNING_FIELDS["QtermSlack"]] > 0).all():
        raise ValueError("tuning: QtermSlack entries must be positive on a context with a terminal set")
    return r


def tuning_rows(cfg, B, **fields):
    """(B, 98) rows of controller tuning for Context.tuning_set, columns TUNING_FIELDS: the weights and bounds of `cfg` (an LmpcConfig) with the named fields replaced.
    Each keyword -- Q, R, Qf, dR, Qslack, QtermSlack (or QterminalSlack), xRef, bx, bu -- is a scalar, an array for every car (the field's own shape: Q (6, 6),
    dR (2,), ...), or an array with a leading B axis, one entry per car.  The terminal-slack weight has two keywords, so that a (6, 6) array is never ambiguous at
    B = 6: QtermSlack takes DIAGONALS -- (6,) for every car or (B, 6), one per car; QterminalSlack takes full MATRICES, the reference's name and form -- (6, 6) or
    (B, 6, 6), which must be diagonal.
    Needs neither the library nor a device.  Raises ValueError on what lmpc_tuning_set would refuse."""
    B = int(B)
    if B < 1:
        raise ValueError("tuning_rows: B must be at least 1")
    row = np.zeros(TUNING_NPAR)
    for name, sl in TUNING_FIELDS.items():
        v = np.array(getattr(cfg, name), dtype=np.float64)
        row[sl] = v.reshape(6, 6).diagonal() if name == "QtermSlack" else v
    rows = np.tile(row, (B, 1))
    for key, v in fields.items():
        name = "QtermSlack" if key == "QterminalSlack" else key
        if name not in TUNING_FIELDS:
            raise ValueError("tuning_rows: unknown field %r (one of %s)" % (key, ", ".join(TUNING_FIELDS)))
        shp = _TUNING_SHAPES[name]
        v = np.asarray(v, dtype=np.float64)
        if key == "QterminalSlack":
            if v.ndim not in (2, 3) or v.shape[-2:] != (6, 6):
                raise ValueError("tuning_rows: QterminalSlack must be a (6, 6) or a (%d, 6, 6) array of matrices, got shape %s (diagonals go by the name QtermSlack)" % (B, v.shape))
            off = v - v * np.eye(6)
            if np.any(off != 0):
                raise ValueError("tuning_rows: QterminalSlack must be diagonal")
            v = np.diagonal(v, axis1=-2, axis2=-1)
        if v.ndim == 0:
            v = np.broadcast_to(v, shp)
        if v.shape == shp:
            v = np.broadcast_to(v, (B,) + shp)
        elif v.shape != (B,) + shp:
            raise ValueError("tuning_rows: %s must be a scalar, a %s array or a (%d,) + %s array, got shape %s" % (key, shp, B, shp, v.shape))
        rows[:, TUNING_FIELDS[name]] = v.reshape(B, -1)
    return check_tuning(rows, cfg.numSS_it)


# One track row (lmpc_track_set): [0] the number of table rows, [1] trackLength, [2:98] PointAndTangent, 16 x 6 row-major, unused rows zero.
TRACK_NPAR = 2 + MAX_TRACK_ROWS * 6


def track_row(table, trackLength=None):
    """One row of TRACK_NPAR doubles from a PointAndTangent table ((rows, 6), rows <= 16) and its length (default: cumulative s + length of the last row, as
    Map.__init__ computes TrackLength, Track.py:133).  Needs neither the library nor a device."""
    t = np.asarray(table, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] != 6 or not 1 <= t.shape[0] <= MAX_TRACK_ROWS:
        raise ValueError("track_row: a (rows, 6) table with 1 <= rows <= %d expected, got shape %s" % (MAX_TRACK_ROWS, t.shape))
    row = np.zeros(TRACK_NPAR)
    row[0] = t.shape[0]
    row[1] = float(t[-1, 3] + t[-1, 4]) if trackLength is None else float(trackLength)
    row[2:2 + t.size] = t.reshape(-1)
    return row


def track_rows(tables):
    """(n, 98) rows for Context.track_set from a sequence of PointAndTangent tables, or of (table, trackLength) pairs; checked as check_tracks does."""
    rows = [track_row(*t) if isinstance(t, tuple) else track_row(t) for t in tables]
    return check_tracks(np.stack(rows)) if rows else None


def track_table(row):
    """(PointAndTangent, trackLength) of one track row: the inverse of track_row."""
    row = np.asarray(row, dtype=np.float64)
    n = int(row[0])
    return row[2:2 + 6 * n].reshape(n, 6).copy(), float(row[1])


def check_tracks(rows):
    """(n, 98) float64 rows, or None for "no rows" (None or empty); ValueError for what lmpc_track_set refuses in a row: a wrong shape, a non-finite entry, a row count
    that is not an integer in 1..16, trackLength <= 0, a negative segment length."""
    r = _check_rows(rows, TRACK_NPAR, "tracks", True)
    if r is None:
        return None
    n = r[:, 0]
    if not np.all((n >= 1) & (n <= MAX_TRACK_ROWS) & (n == np.floor(n))):
        raise ValueError("tracks: the row count must be an integer in 1..%d" % MAX_TRACK_ROWS)
    if not np.all(r[:, 1] > 0):
        raise ValueError("tracks: trackLength must be positive")
    for k in range(r.shape[0]):
        if (r[k, 2:].reshape(MAX_TRACK_ROWS, 6)[:int(n[k]), 4] < 0).any():
            raise ValueError("tracks: negative segment length in row %d" % k)
    return r


def _chk(rc):
    if rc != 0:
        raise LmpcError("liblmpc_hip error %d: %s" % (rc, load().lmpc_last_error().decode()))


def _d(a):
    # (c_void_p around the raw address: numpy's data_as goes through ctypes.cast, 3 us per array -- 25 arrays per lmpc_step_batch call)
    return None if a is None else C.c_void_p(a.ctypes.data)


def _p(p):
    """device pointer -> c_void_p (ctypes hands Structure c_void_p fields back as plain ints)."""
    return p if isinstance(p, C.c_void_p) else C.c_void_p(p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _npz_path(path):
    """The file np.savez_compressed writes for `path`: it appends .npz to a path without that extension (file objects are taken as they are)."""
    if isinstance(path, (str, os.PathLike)):
        path = os.fspath(path)
        if not path.endswith(".npz"):
            path += ".npz"
    return path


def default_config():
    cfg = LmpcConfig()
    _chk(load().lmpc_config_default(C.byref(cfg)))
    return cfg


def set_arr(field, values):
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    assert len(v) == len(field), (len(v), len(field))
    for i, x in enumerate(v):
        field[i] = float(x)


class Context:
    """One lmpc_ctx: device lap stores + batched solver for a fixed (N, safe-set size) configuration."""

    def __init__(self, cfg, runtime_kernel=False, k1_ahead=True, k1_merge=True):
        """k1_ahead=False: queued step_batch_dev steps keep their regression on the context's stream (LMPC_CREATE_NO_K1_AHEAD; ContextPool members: several batches in
        flight fill the idle CUs already, and the look-ahead's event operations only cost them).  k1_merge=False: chained steps never hold their solve for a two-role
        launch with the next step's regression (LMPC_CREATE_NO_K1_MERGE): the two-stream look-ahead serves all of them."""
        self.lib = load()
        self.cfg = cfg
        self.N = cfg.N
        self.S = cfg.numSS_points if cfg.numSS_it > 0 else 0
        self.M = 8 * self.N + self.S
        self._step_plan = {}
        self._ro_trace = None
        self._h = C.c_void_p()
        self._pid = os.getpid()         # the process that owns the device context (see close)
        base = 0 if k1_ahead and not _POOL_MEMBER else CREATE_NO_K1_AHEAD
        if not k1_merge:
            base |= CREATE_NO_K1_MERGE
        if runtime_kernel:              # (tests: the runtime-(N, S) kernel even where a fast one exists)
            rc = self.lib.lmpc_create_ex(C.byref(cfg), C.c_uint(base | CREATE_FORCE_RUNTIME_KERNEL), C.byref(self._h))
        else:
            rc = self.lib.lmpc_create_ex(C.byref(cfg), C.c_uint(base), C.byref(self._h)) if base else self.lib.lmpc_create(C.byref(cfg), C.byref(self._h))
        if rc == E_VARIANT:             # (N, numSS_points) outside the built-in set: compile its shared object once (hipcc, ~20 s), then retry ...
            from . import build
            try:
                build.build_variant(self.N, self.S)
                rc = self.lib.lmpc_create_ex(C.byref(cfg), C.c_uint(base), C.byref(self._h))
            except (OSError, RuntimeError, ValueError, subprocess.SubprocessError) as e:
                # ... and where that is not possible (no hipcc on the box, a failed build): the runtime-(N, S) kernel serves the horizon, several times slower.
                # MPCParams.N is a plain parameter in the reference (PredictiveControllers.py:63-107, main.py:43): LMPC_E_VARIANT never reaches a user.
                warnings.warn("no solve-kernel variant for N = %d, numSS_points = %d (%s): using the runtime-(N, S) kernel" % (self.N, self.S, str(e).splitlines()[0][:120]))
                rc = self.lib.lmpc_create_ex(C.byref(cfg), C.c_uint(base | CREATE_RUNTIME_KERNEL), C.byref(self._h))
        _chk(rc)
        self.solver_kind = int(self.lib.lmpc_solver_kind(self._h))      # 0 built-in, 1 variant library, 2 runtime-(N, S) kernel

    def close(self):
        # A forked child inherits this object but not a usable HIP runtime: when the child's garbage collector finalises its copy, lmpc_destroy would run HIP calls
        # in a process that must not make any (a segmentation fault in a multiprocessing worker, and a parent waiting for ever on the dead worker: it happened in the
        # worker pools of the GPU tests).  Only the creating process destroys the context.
        if self._h and getattr(self, "_pid", None) == os.getpid():
            self.lib.lmpc_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- stores
    # ---- the per-car row sets (csrc/lmpc_rows.h): every `set` and `get` of the five goes through these two
    def _rows_set(self, fn, rows, *extra):
        """rows (n, width) as its check returned them go to the setter `fn`, None as (0, NULL); extra: per-row arrays (or None) that travel with the rows."""
        if rows is None:
            _chk(fn(self._h, 0, None, *[None] * len(extra)))
        else:
            _chk(fn(self._h, rows.shape[0], _d(rows), *[_d(e) for e in extra]))

    def _rows_get(self, fn, width, dtype, *extra):
        """The rows in force behind the getter `fn`, (n, width) of dtype: the count first, then the rows.  extra: the dtypes of further (n,) outputs of the getter;
        with any, (rows, *those) is returned."""
        n = C.c_int()
        _chk(fn(self._h, C.byref(n), None, *[None] * len(extra), 0))
        out = [np.zeros((n.value, width), dtype)] + [np.zeros(n.value, t) for t in extra]
        if n.value:
            _chk(fn(self._h, C.byref(n), *[_d(a) for a in out], n.value))
        return tuple(out) if extra else out[0]

    def model_add_trajectory(self, x, u):
        x = _f64(x); u = _f64(u)
        _chk(self.lib.lmpc_model_add_trajectory(self._h, _d(x), _d(u), C.c_int(x.shape[0])))

    def model_replace_lap(self, pos, x, u):
        x = _f64(x); u = _f64(u)
        _chk(self.lib.lmpc_model_replace_lap(self._h, C.c_int(pos), _d(x), _d(u), C.c_int(x.shape[0])))

    def model_num_laps(self):
        n = C.c_int()
        _chk(self.lib.lmpc_model_num_laps(self._h, C.byref(n)))
        return n.value

    def model_set_lap_table(self, rows):
        """Per-problem regression laps (lmpc_model_set_lap_table): rows (n, trToUse) of INSERTION indices of regression-store laps (0 = the first
        model_add_trajectory; duplicates allowed, any order inside a row).  None or no rows -- the default, the first trToUse laps of the sorted order for every
        problem; one row -- every problem; n rows -- problem b of a later regress_batch / regress_points / step_batch / step_batch_dev / rollout_begin /
        LTV rollout_begin_mpc uses row b, and a call with another batch size is refused.  A session uses the table in force when it began.  On an LMPC context
        only the regression follows the table: the safe set has a table of its own, ss_set_lap_table."""
        self._rows_set(self.lib.lmpc_model_set_lap_table, check_lap_table(rows, int(self.cfg.trToUse)))

    def model_lap_info(self, lap):
        """(rows, position in the sorted order) of the regression-store lap with insertion index `lap` (lmpc_model_lap_info)."""
        T = C.c_int(); pos = C.c_int()
        _chk(self.lib.lmpc_model_lap_info(self._h, int(lap), C.byref(T), C.byref(pos)))
        return T.value, pos.value

    def model_lap_table(self):
        """The rows in force, (n, trToUse) int32 as model_set_lap_table received them; n = 0: the default (lmpc_model_get_lap_table)."""
        return self._rows_get(self.lib.lmpc_model_get_lap_table, int(self.cfg.trToUse), np.int32)

    def ss_add_trajectory(self, x, u, track_row=None):
        """LMPC.addTrajectory.  track_row: the row of track_set whose TrackLength computeCost uses (lmpc_ss_add_trajectory_on) -- needed when one row per car is in
        force, since a lap handed in by the host names no car; None: the config's TrackLength, or the one row's."""
        x = _f64(x); u = _f64(u)
        if track_row is None:
            _chk(self.lib.lmpc_ss_add_trajectory(self._h, _d(x), _d(u), C.c_int(x.shape[0])))
        else:
            _chk(self.lib.lmpc_ss_add_trajectory_on(self._h, C.c_int(int(track_row)), _d(x), _d(u), C.c_int(x.shape[0])))

    def ss_add_point(self, x, u):
        x = _f64(x); u = _f64(u)
        _chk(self.lib.lmpc_ss_add_point(self._h, _d(x), _d(u)))

    def ss_replace_lap(self, lap, x, u, qfun):
        x = _f64(x); u = _f64(u); q = _f64(qfun)
        _chk(self.lib.lmpc_ss_replace_lap(self._h, C.c_int(lap), _d(x), _d(u), _d(q), C.c_int(x.shape[0])))

    def ss_set_selected(self, laps):
        laps = _i32(laps)
        _chk(self.lib.lmpc_ss_set_selected(self._h, _d(laps), C.c_int(len(laps))))

    def ss_set_lap_table(self, rows, last=None):
        """Per-problem safe sets (lmpc_ss_set_lap_table): rows (n, numSS_it) of safe-set lap indices in ss_add_trajectory order (duplicates allowed, any order inside
        a row: each row is used in ascending LapTime, ties by index).  last (n,): the index of each car's most recent lap -- the entry of a row that equals it takes
        the "current lap" branch of the Q-function shift -- or -1 for none; None: the context-wide rule, the last lap stored.  None or no rows -- the shared
        selection; one row -- every problem; n rows -- problem b of a later select_batch / step_batch / step_batch_dev / rollout step uses row b, and a launch
        with another batch size is refused.  The table names laps, not snapshots, and is live in a rollout session: a later ss_extend_lap or a new `set` reaches
        the next step."""
        rows, last = check_ss_table(rows, int(self.cfg.numSS_it), last)
        self._rows_set(self.lib.lmpc_ss_set_lap_table, rows, last)

    def ss_lap_table(self):
        """(rows (n, numSS_it) int32, last (n,) int32 or None) in force, as ss_set_lap_table received them; n = 0: the shared selection (lmpc_ss_get_lap_table)."""
        rows, last = self._rows_get(self.lib.lmpc_ss_get_lap_table, int(self.cfg.numSS_it), np.int32, np.int32)
        return rows, (None if last.size == 0 or np.all(last == SS_LAST_SHARED) else last)

    def ss_get_qfun(self, lap):
        T = C.c_int()
        _chk(self.lib.lmpc_ss_get_qfun(self._h, C.c_int(lap), None, C.byref(T)))
        q = np.zeros(T.value)
        _chk(self.lib.lmpc_ss_get_qfun(self._h, C.c_int(lap), _d(q), C.byref(T)))
        return q

    # ---- batched compute (host buffers)
    def regress_batch(self, xLin, uLin):
        N = self.N
        xLin = _f64(xLin); uLin = _f64(uLin)
        B = xLin.shape[0]
        stride = xLin.shape[1] * 6
        A = np.zeros((B, N, 6, 6)); Bm = np.zeros((B, N, 6, 2)); Cc = np.zeros((B, N, 6)); st = np.zeros((B, N), np.int32)
        _chk(self.lib.lmpc_regress_batch(self._h, C.c_int(B), _d(xLin), C.c_int(stride), _d(uLin), _d(A), _d(Bm), _d(Cc), _d(st)))
        return A, Bm, Cc, st

    def regress_points(self, x, u):
        """PredictiveModel.regressionAndLinearization for n independent points: (A (n, 6, 6), B (n, 6, 2), C (n, 6), status (n,))."""
        x = _f64(x).reshape(-1, 6); u = _f64(u).reshape(-1, 2); n = x.shape[0]
        A = np.zeros((n, 6, 6)); Bm = np.zeros((n, 6, 2)); Cc = np.zeros((n, 6)); st = np.zeros(n, np.int32)
        _chk(self.lib.lmpc_regress_points(self._h, C.c_int(n), _d(x), _d(u), _d(A), _d(Bm), _d(Cc), _d(st)))
        return A, Bm, Cc, st

    def _zeros(self, keys, B):
        """Fresh zero arrays {key: array} for B problems, shapes and dtypes from ARRAYS."""
        return {k: np.zeros(shp, dt) for k, (shp, dt) in array_specs(B, self.N, self.S, self.cfg.numSS_it, keys).items()}

    def select_batch(self, x0, zt, xPredPrev=None, hasPred=None, timeStep=None):
        x0 = _f64(x0); zt = _f64(zt); B = x0.shape[0]
        xpp = None if xPredPrev is None else _f64(xPredPrev)
        hp = None if hasPred is None else _i32(hasPred)
        ts = None if timeStep is None else _i32(timeStep)
        out = self._zeros(SELECT_OUT_KEYS, B)
        _chk(self.lib.lmpc_select_batch(self._h, C.c_int(B), _d(x0), _d(zt), _d(xpp), _d(hp), _d(ts), *[_d(out[k]) for k in SELECT_OUT_KEYS]))
        return out

    def qp_solve_batch(self, A, Bm, Cc, x0, uOld, ssSel=None, qSel=None):
        A = _f64(A); Bm = _f64(Bm); Cc = _f64(Cc); x0 = _f64(x0); uOld = _f64(uOld); B = x0.shape[0]
        ss = None if ssSel is None else _f64(ssSel); q = None if qSel is None else _f64(qSel)
        out = self._zeros(QP_OUT_KEYS, B)
        _chk(self.lib.lmpc_qp_solve_batch(self._h, C.c_int(B), _d(A), _d(Bm), _d(Cc), _d(x0), _d(uOld), _d(ss), _d(q), *[_d(out[k]) for k in QP_OUT_KEYS]))
        return out

    def step_batch(self, x0, xLin, uLin, uOld, zt=None, xPredPrev=None, hasPred=None, timeStep=None):
        N, S = self.N, self.S
        x0 = _f64(x0); xLin = _f64(xLin); uLin = _f64(uLin); uOld = _f64(uOld); B = x0.shape[0]
        assert xLin.shape == (B, N + 1, 6) and uLin.shape == (B, N, 2), (xLin.shape, uLin.shape)
        ztc = None if zt is None else _f64(zt)
        xpp = None if xPredPrev is None else _f64(xPredPrev)
        hp = None if hasPred is None else _i32(hasPred)
        ts = None if timeStep is None else _i32(timeStep)
        # the sixteen outputs are ranges of ONE fresh float64 buffer and one int32 buffer (a drop-in LMPC.solve spends more time in sixteen
        # allocations and twenty-six address look-ups than the library spends outside its two kernels): addresses are base + offset
        plan = self._step_plan.get(B)
        if plan is None:
            offs, o = [], 0
            for k, (shp, dt) in array_specs(B, N, S, self.cfg.numSS_it, STEP_OUT_KEYS).items():
                if dt is _f8:                              # (status, iters: the int32 buffer)
                    n = int(np.prod(shp)); offs.append((k, shp, o, n)); o += n
            plan = self._step_plan[B] = (offs, o)
        offs, total = plan
        buf = np.zeros(total); ibuf = np.zeros(2 * B, np.int32)
        base = buf.ctypes.data; ibase = ibuf.ctypes.data
        out = {k: buf[o:o + n].reshape(shp) for k, shp, o, n in offs}
        out["status"] = ibuf[:B]; out["iters"] = ibuf[B:]
        adr = {k: base + 8 * o for k, shp, o, n in offs}
        pa = lambda a: None if a is None else a.ctypes.data
        _chk(self.lib.lmpc_step_batch(self._h, B, pa(x0), pa(xLin), pa(uLin), pa(uOld), pa(ztc), pa(xpp), pa(hp), pa(ts),
                                      adr["xPred"], adr["uPred"], adr["slack"], adr["lambd"], adr["sTerm"], adr["ztNext"], adr["ztuNext"], adr["ssSel"], adr["qSel"], adr["mu"],
                                      adr["A"], adr["B"], adr["C"], ibase, ibase + 4 * B, adr["resid"]))
        return out

    def qp_dims(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _chk(self.lib.lmpc_qp_dims(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def assemble_batch(self, A, Bm, Cc, x0, uOld, ssSel=None, qSel=None):
        nz, mi, me = self.qp_dims(); m = mi + me
        A = _f64(A); Bm = _f64(Bm); Cc = _f64(Cc); x0 = _f64(x0); uOld = _f64(uOld); B = x0.shape[0]
        ss = None if ssSel is None else _f64(ssSel); q = None if qSel is None else _f64(qSel)
        P = np.zeros((B, nz, nz)); qv = np.zeros((B, nz)); Ad = np.zeros((B, m, nz)); l = np.zeros((B, m)); u = np.zeros((B, m))
        _chk(self.lib.lmpc_assemble_batch(self._h, C.c_int(B), _d(A), _d(Bm), _d(Cc), _d(x0), _d(uOld), _d(ss), _d(q), _d(P), _d(qv), _d(Ad), _d(l), _d(u)))
        return P, qv, Ad, l, u

    # ---- device-resident path
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        _chk(self.lib.lmpc_dev_alloc(self._h, C.c_longlong(int(nbytes)), C.byref(p)))
        return p

    def dev_free(self, p):
        _chk(self.lib.lmpc_dev_free(self._h, _p(p)))

    def dev_upload(self, p, arr):
        arr = np.ascontiguousarray(arr)
        _chk(self.lib.lmpc_dev_upload(self._h, _p(p), _d(arr), C.c_longlong(arr.nbytes)))

    def dev_download(self, p, arr):
        assert arr.flags["C_CONTIGUOUS"]
        _chk(self.lib.lmpc_dev_download(self._h, _d(arr), _p(p), C.c_longlong(arr.nbytes)))
        return arr

    def dev_array(self, arr):
        """Allocate HBM for `arr` and upload it; returns the device pointer."""
        arr = np.ascontiguousarray(arr)
        p = self.dev_alloc(max(arr.nbytes, 8))
        if arr.nbytes:
            self.dev_upload(p, arr)
        return p

    def sync(self):
        _chk(self.lib.lmpc_dev_sync(self._h))

    def flush(self):
        """Launch the solve a queued step_batch_dev left held for the next step (lmpc_dev_flush); no drain.  For callers that queue steps and then do host work."""
        _chk(self.lib.lmpc_dev_flush(self._h))

    def step_batch_dev(self, B, args):
        _chk(self.lib.lmpc_step_batch_dev(self._h, C.c_int(B), C.byref(args)))

    def step_dev_buffers(self, inp, diagnostics=True):
        """HBM-resident inputs/outputs of lmpc_step_batch_dev for a batch given as host arrays (keys x0, xLin, uLin, uOld, zt,
        xPredPrev, hasPred, timeStep).  Returns (StepDevArgs, device pointers to free with dev_free).  diagnostics=False leaves out what
        the hot path does not need downstream (inequality multipliers mu, residual triple, Q-function values of the selection):
        those pointers stay NULL and the kernels skip the stores."""
        B = np.asarray(inp["x0"]).shape[0]
        a = StepDevArgs(); keep = []
        # (A_i / B_i / C_i, MPC.A / B / C of the reference, are the hand-over from the regression kernel to the solve kernel.  Caller-owned here, so that launches
        # can be queued back to back: a launch that used the context's own hand-over buffers is drained before the next one overwrites them)
        keys = [k for k in STEP_IN_KEYS + STEP_OUT_KEYS if diagnostics or k not in DIAGNOSTIC_KEYS]
        for k, (shp, dt) in array_specs(B, self.N, self.S, self.cfg.numSS_it, keys).items():
            if k in STEP_IN_KEYS:                          # (x0, xLin, uLin, uOld must be given; the others default to zeros)
                p = self.dev_array(np.ascontiguousarray(inp[k] if inp.get(k) is not None or k in ("x0", "xLin", "uLin", "uOld") else np.zeros(shp), dtype=dt))
            else:
                p = self.dev_alloc(max(int(np.prod(shp)) * np.dtype(dt).itemsize, 8))
            keep.append(p); setattr(a, _FIELD[k], p)
        return a, keep

    def step_dev_fetch(self, a, B):
        """Download every output of a finished lmpc_step_batch_dev call (same keys as step_batch)."""
        self.sync()
        out = self._zeros(STEP_OUT_KEYS, B)
        for k, arr in out.items():
            src = getattr(a, _FIELD[k])
            if arr.nbytes and src:                         # (diagnostic outputs that were not requested stay zero)
                self.dev_download(src, arr)
        return out

    def plant_step_batch(self, x, x_glob, u, noise):
        x = _f64(x); xg = _f64(x_glob); u = _f64(u); nz = _f64(noise); B = x.shape[0]
        xn = np.zeros((B, 6)); xgn = np.zeros((B, 6)); st = np.zeros(B, np.int32)
        _chk(self.lib.lmpc_plant_step_batch(self._h, C.c_int(B), _d(x), _d(xg), _d(u), _d(nz), _d(xn), _d(xgn), _d(st)))
        return xn, xgn, st

    def plant_set_params(self, par):
        """Vehicle constants of the plant for every later plant_step_batch / rollout_begin / rollout_begin_mpc / rollout_pid (lmpc_plant_set_params): None or no rows --
        the reference's vehicle; one row of PLANT_PARAM_NAMES -- every car; (n, 10) -- car b uses row b (n <= max_batch; a later call with more cars is refused).
        A session uses the rows in force when it began.  plant_params() builds the rows."""
        self._rows_set(self.lib.lmpc_plant_set_params, None if par is None or np.size(par) == 0 else _f64(par).reshape(-1, PLANT_NPAR))

    def tuning_set(self, rows):
        """Per-problem controller tuning (lmpc_tuning_set): None or no rows -- the config's weights and bounds; one row of TUNING_FIELDS -- every problem; (n, 98) --
        problem b uses row b, and a launch of another batch size is refused (LmpcError, the context stays usable).  The rows are live: a call between two rollout_run
        calls reaches the next step.  They apply to qp_solve_batch, step_batch, step_batch_dev, every step of a rollout session and assemble_batch.  tuning_rows()
        builds the rows."""
        self._rows_set(self.lib.lmpc_tuning_set, check_tuning(rows, int(self.cfg.numSS_it)))

    def track_set(self, rows):
        """Per-car tracks (lmpc_track_set): None or no rows -- the config's track; one row of TRACK_NPAR doubles (track_row) -- every car; (n, 98) -- element b of a
        batched call uses row b, and a call of another count is refused (LmpcError, the context stays usable).  Refused while a rollout session is active.
        track_rows() builds the rows from PointAndTangent tables."""
        self._rows_set(self.lib.lmpc_track_set, check_tracks(rows))

    def tracks(self):
        """The rows in force, (n, 98), as track_set received them; n = 0: the config's track (lmpc_track_get)."""
        return self._rows_get(self.lib.lmpc_track_get, TRACK_NPAR, np.float64)

    def tuning(self):
        """The rows in force, (n, 98), as tuning_set received them; n = 0: the config's weights (lmpc_tuning_get)."""
        return self._rows_get(self.lib.lmpc_tuning_get, TUNING_NPAR, np.float64)

    def plant_params(self):
        """The rows in force, (n, 10); n = 0: the reference's vehicle (lmpc_plant_get_params)."""
        return self._rows_get(self.lib.lmpc_plant_get_params, PLANT_NPAR, np.float64)

    # ---- counter-based noise generated on the device (lmpc_noise_*, lmpc_rollout_set_noise; csrc/lmpc_noise.hip.h)
    def noise_raw(self, seed, stream, lap, t0, T, car0, B):
        """The four raw 64-bit words of steps t0 .. t0 + T - 1 and cars car0 .. car0 + B - 1, (T, B, 4) uint64: row [t - t0, b] is what
        numpy.random.Philox(counter=[t, car0 + b, lap, stream], key=[seed, 0]).random_raw(4) returns (lmpc_noise_raw)."""
        T = int(T); B = int(B)
        out = np.zeros((max(T, 0), max(B, 0), 4), np.uint64)
        _chk(self.lib.lmpc_noise_raw(self._h, int(seed), int(stream), int(lap), int(t0), T, int(car0), B, out.ctypes.data))
        return out

    def noise_fill(self, seed, stream, lap, t0, T, car0, B, width=3):
        """The N(0, 1) draws of the same range, (T, B, width) float64 (lmpc_noise_fill): stream 0 / width 3 is the plant noise a session with the device source on sees
        at step t for global car index car0 + b, stream 1 / width 2 the control-law noise of a PID lap."""
        T = int(T); B = int(B); width = int(width)
        out = np.zeros((max(T, 0), max(B, 0), max(width, 0)))
        _chk(self.lib.lmpc_noise_fill(self._h, int(seed), int(stream), int(lap), int(t0), T, int(car0), B, width, out.ctypes.data))
        return out

    def rollout_set_noise(self, on, seed=0, lap=0, car0=0):
        """Noise source of the sessions begun after this call (lmpc_rollout_set_noise).  on: rollout_begin / rollout_begin_mpc / rollout_pid take noise=None (rollout_pid
        also noise_u=None) and the session's draws are generated on the device for steps 0 .. T_max - 1 and global car indices car0 .. car0 + B - 1 of session `lap`;
        an array given is used as it is.  off (a new context): noise=None is refused."""
        _chk(self.lib.lmpc_rollout_set_noise(self._h, 1 if on else 0, int(seed), int(lap), int(car0)))

    def rollout_get_noise(self):
        """(on, seed, lap, car0) in force (lmpc_rollout_get_noise)."""
        on = C.c_int(); seed = C.c_ulonglong(); lap = C.c_ulonglong(); car0 = C.c_longlong()
        _chk(self.lib.lmpc_rollout_get_noise(self._h, C.byref(on), C.byref(seed), C.byref(lap), C.byref(car0)))
        return bool(on.value), int(seed.value), int(lap.value), int(car0.value)

    @staticmethod
    def _session_noise(noise, nb, width, T_max):
        """(array or None, T_max) of a session's noise argument: an array (T_max, nb, width), or None with T_max given -- the device source (rollout_set_noise)."""
        if noise is None:
            if T_max is None:
                raise ValueError("noise=None (the device source, rollout_set_noise) needs T_max")
            return None, int(T_max)
        nz = _f64(noise)
        assert nz.ndim == 3 and nz.shape[1:] == (nb, width) and (T_max is None or int(T_max) == nz.shape[0]), (nz.shape, nb, width, T_max)
        return nz, nz.shape[0]

    def rollout_begin(self, x0, xglob0, xLin0, uLin0, noise, T_max=None):
        """noise: (T_max, B, 3) N(0, 1) draws, or None with T_max given: the device source (rollout_set_noise; NULL goes to the library, which refuses it while the
        source is off)."""
        x0 = _f64(x0); xg = _f64(xglob0); xl = _f64(xLin0); ul = _f64(uLin0)
        B = x0.shape[0]
        nz, T = self._session_noise(noise, B, 3, T_max)
        assert xl.shape == (B, self.N + 1, 6) and ul.shape == (B, self.N, 2)
        tr = self.rollout_trace()                 # (what the session is about to take as its snapshot of the trace)
        _chk(self.lib.lmpc_rollout_begin(self._h, C.c_int(B), C.c_int(T), _d(x0), _d(xg), _d(xl), _d(ul), _d(nz)))
        self._ro = (B, T); self._ro_t = 0; self._ro_trace = tr

    def rollout_begin_mpc(self, x0, xglob0, noise, xLin0=None, uLin0=None, A=None, B=None, stop_at_line=False, T_max=None):
        """Session of B plain-MPC laps on a numSS_it == 0 context (lmpc_rollout_begin_mpc).  A (B, 6, 6) and B (B, 6, 2) given: the LTI MPC on those models;
        else the LTV-MPC from the linearisation trajectories xLin0 (B, N + 1, 6), uLin0 (B, N, 2).  noise: (T_max, B, 3), or None with T_max given: the device
        source (rollout_set_noise)."""
        x0 = _f64(x0); xg = _f64(xglob0); nb = x0.shape[0]
        nz, T = self._session_noise(noise, nb, 3, T_max)
        assert xg.shape == x0.shape == (nb, 6)
        lti = A is not None or B is not None
        if lti:
            A = _f64(A); B = _f64(B); xl = ul = None
            assert A.shape == (nb, 6, 6) and B.shape == (nb, 6, 2), (A.shape, B.shape)
        else:
            xl = _f64(xLin0); ul = _f64(uLin0); A = B = None
            assert xl.shape == (nb, self.N + 1, 6) and ul.shape == (nb, self.N, 2), (xl.shape, ul.shape)
        pa = lambda a: None if a is None else a.ctypes.data
        tr = self.rollout_trace()
        _chk(self.lib.lmpc_rollout_begin_mpc(self._h, nb, T, pa(x0), pa(xg), pa(xl), pa(ul), pa(A), pa(B), pa(nz), 1 if stop_at_line else 0))
        self._ro = (nb, T); self._ro_t = 0; self._ro_trace = tr

    def rollout_pid(self, x0, xglob0, vt, noise_u, noise, stop_at_line=False, T_max=None):
        """B whole PID laps in one launch (lmpc_rollout_pid): vt (B,) target speeds, noise_u (T_max, B, 2) and noise (T_max, B, 3) N(0, 1) draws of the control law and
        of the plant -- either or both None with T_max given: the device source (rollout_set_noise).  Returns (steps logged, cars that crossed the line); the session
        stays open for rollout_fetch / rollout_end."""
        x0 = _f64(x0); xg = _f64(xglob0); nb = x0.shape[0]
        vt = _f64(np.broadcast_to(np.asarray(vt, float), (nb,)))
        if T_max is None:                         # (one array given: it sets the length of the other, generated one)
            T_max = next((np.shape(a)[0] for a in (noise, noise_u) if a is not None), None)
        nz, T = self._session_noise(noise, nb, 3, T_max)
        nu, T = self._session_noise(noise_u, nb, 2, T)
        assert xg.shape == x0.shape == (nb, 6)
        pa = lambda a: None if a is None else a.ctypes.data
        t = C.c_int(); nd = C.c_int()
        _chk(self.lib.lmpc_rollout_pid(self._h, nb, T, x0.ctypes.data, xg.ctypes.data, vt.ctypes.data, pa(nu), pa(nz),
                                       1 if stop_at_line else 0, C.byref(t), C.byref(nd)))
        self._ro = (nb, T); self._ro_t = t.value; self._ro_trace = None              # (a PID session records no trace)
        return t.value, nd.value

    def rollout_run(self, max_steps):
        t = C.c_int(); nd = C.c_int()
        _chk(self.lib.lmpc_rollout_run(self._h, C.c_int(int(max_steps)), C.byref(t), C.byref(nd)))
        self._ro_t = t.value                      # simulated steps so far (upper bound for rollout_fetch)
        return t.value, nd.value

    def rollout_fetch(self, t0, t1):
        B = self._ro[0]; n = t1 - t0
        X = np.zeros((n, B, 6)); U = np.zeros((n, B, 2)); G = np.zeros((n, B, 6))
        done = np.zeros(B, np.int32); st = np.zeros(B, np.int32); fx = np.zeros((B, 6)); fg = np.zeros((B, 6))
        _chk(self.lib.lmpc_rollout_fetch(self._h, C.c_int(t0), C.c_int(t1), _d(X), _d(U), _d(G), _d(done), _d(st), _d(fx), _d(fg)))
        return X, U, G, done, st, fx, fg

    def rollout_end(self):
        _chk(self.lib.lmpc_rollout_end(self._h))

    # ---- session traces (lmpc_rollout_set_trace; csrc/lmpc_trace.hip.h)
    def rollout_set_trace(self, cars, what=TRACE_DEFAULT):
        """The cars whose controller output the sessions begun after this call record at every step, and the planes (TRACE_* bits; TRACE_DEFAULT: every plane this
        context can record) -- xStoredPredTraj / uStoredPredTraj / SSStoredPredTraj of the reference (PredictiveControllers.py:364-379), Qfun_SelectedTot, the
        solver's words and the inertial positions.  None or no cars: off.  A session keeps the list it began with; rollout_pid ignores it."""
        cars, what = check_trace(cars, what, self.cfg.numSS_it)
        _chk(self.lib.lmpc_rollout_set_trace(self._h, cars.shape[0], cars.ctypes.data if cars.size else None, what))

    def rollout_trace(self):
        """(cars (n,) int32, what) in force (lmpc_rollout_get_trace); no cars and 0: off."""
        n = C.c_int(); what = C.c_uint()
        _chk(self.lib.lmpc_rollout_get_trace(self._h, C.byref(n), None, C.byref(what), 0))
        cars = np.zeros(n.value, np.int32)
        _chk(self.lib.lmpc_rollout_get_trace(self._h, C.byref(n), cars.ctypes.data, C.byref(what), cars.shape[0]))
        return cars, int(what.value)

    # ---- parking (lmpc_rollout_set_parking; csrc/lmpc_live.hip.h)
    def rollout_set_parking(self, mode=0, cars=None):
        """The parking of the sessions begun after this call: mode (PARK_* bits; True: PARK_FINISHED) and the cars parked from step 0.  A parked car leaves the
        launches of every later step; a session that stops at the line ends when no car is live.  mode 0 and no cars: off.  A session keeps the setting it began
        with; rollout_pid ignores it."""
        mode, cars = check_parking(mode, cars)
        _chk(self.lib.lmpc_rollout_set_parking(self._h, mode, cars.shape[0], cars.ctypes.data if cars.size else None))

    def rollout_parking(self):
        """(mode, cars (n,) int32) in force (lmpc_rollout_get_parking); 0 and no cars: off."""
        n = C.c_int(); mode = C.c_uint()
        _chk(self.lib.lmpc_rollout_get_parking(self._h, C.byref(mode), C.byref(n), None, 0))
        cars = np.zeros(n.value, np.int32)
        _chk(self.lib.lmpc_rollout_get_parking(self._h, C.byref(mode), C.byref(n), cars.ctypes.data if cars.size else None, cars.shape[0]))
        return int(mode.value), cars

    def rollout_parked_at(self):
        """(parked_at (B,) int32, n_live) of the active session (lmpc_rollout_parked_at): -1 for a live car, else the first step the car was not stepped -- its
        state, log rows and trace planes stand still from there."""
        ro = getattr(self, "_ro", None)           # (no session begun so far: the library says so)
        at = np.zeros(ro[0] if ro else 0, np.int32); nl = C.c_int()
        _chk(self.lib.lmpc_rollout_parked_at(self._h, at.ctypes.data if at.size else None, C.byref(nl)))
        return at, nl.value

    def debug_live_compact(self, doneAt, parked0, t, mode, parkedAt=None):
        """The sessions' compaction kernel on host arrays (lmpc_debug_live_compact): returns (live (n_live,) int32 ascending, parkedAt (n,) int32).  parkedAt given:
        the result of an earlier call, on top of which this one parks more cars."""
        done = _i32(doneAt); p0 = _i32(parked0); n = done.shape[0]
        assert done.shape == p0.shape == (n,)
        at = np.full(n, -1, np.int32) if parkedAt is None else _i32(parkedAt).copy()
        assert at.shape == (n,)
        live = np.zeros(n, np.int32); nl = C.c_int()
        _chk(self.lib.lmpc_debug_live_compact(self._h, n, done.ctypes.data, p0.ctypes.data, int(t), int(mode), live.ctypes.data, at.ctypes.data, C.byref(nl)))
        return live[:nl.value].copy(), at

    def rollout_trace_bytes(self, n, what, T_max):
        """Device memory the trace planes of a session of that shape take (lmpc_rollout_trace_bytes)."""
        b = C.c_longlong()
        _chk(self.lib.lmpc_rollout_trace_bytes(self._h, int(n), int(what), int(T_max), C.byref(b)))
        return int(b.value)

    def rollout_fetch_trace(self, t0, t1, keys=None):
        """The recorded planes of steps [t0, t1) of the active session (lmpc_rollout_fetch_trace): dict key -> array (t1 - t0, n, ...) with n the listed cars in the
        order given to rollout_set_trace -- xPred (.., N + 1, 6), uPred (.., N, 2), ssSel (.., S, 6), qSel (.., S), iters, status, xyPred (.., N + 1, 2), xySS (.., S, 2),
        mapStatus.  keys: only those planes (one the session does not record is refused by the library)."""
        if self._ro_trace is None:
            cars, what = np.zeros(0, np.int32), 0
        else:
            cars, what = self._ro_trace
        n = int(t1) - int(t0)
        if n < 0:
            raise ValueError("rollout_fetch_trace: t1 < t0")
        planes = {k: (shp, dt) for k, bit, shp, dt in trace_planes(self.N, self.S, what)}
        if keys is not None:
            full = {k: (shp, dt) for k, bit, shp, dt in trace_planes(self.N, max(self.S, 1), TRACE_ALL)}
            planes = {k: full[k] for k in keys}
        out = {k: np.zeros((n, cars.shape[0]) + tuple(shp), dt) for k, (shp, dt) in planes.items()}
        arg = TraceOut(**{k: v.ctypes.data for k, v in out.items()})
        _chk(self.lib.lmpc_rollout_fetch_trace(self._h, int(t0), int(t1), C.byref(arg)))
        return out

    # ---- checkpoint / resume of the lap stores (optional .npz dump; no reference counterpart beyond an unused `import pickle`, main.py:36) ----
    def store_read_lap(self, store, lap):
        """(x (T, 6), u (T, 2), qfun (T,) or None) of one stored lap: store 0 = regression store in its sorted order, 1 = safe set in addTrajectory order."""
        T = C.c_int()
        _chk(self.lib.lmpc_store_read_lap(self._h, C.c_int(store), C.c_int(int(lap)), None, None, None, C.byref(T)))
        x = np.zeros((T.value, 6)); u = np.zeros((T.value, 2)); q = np.zeros(T.value) if store == 1 else None
        _chk(self.lib.lmpc_store_read_lap(self._h, C.c_int(store), C.c_int(int(lap)), _d(x), _d(u), _d(q), C.byref(T)))
        return x, u, q

    def save_stores(self, path):
        """Both lap stores (and the explicit safe-set selection, if one is set by the caller: not stored -- it is per-step state of the controller) as one .npz.
        Tuning rows (tuning_set) are not saved either: they are controller parameters, not store content -- set them again on the restored context.
        Neither are track rows (track_set): the stores carry laps, not tracks -- a stored lap's Qfun and extension rows already hold what its TrackLength made of them."""
        out = {}
        nm = C.c_int(); _chk(self.lib.lmpc_model_num_laps(self._h, C.byref(nm)))
        for i in range(nm.value):
            x, u, _ = self.store_read_lap(0, i); out["model_x%d" % i] = x; out["model_u%d" % i] = u
        ns = self.ss_num_laps()
        for i in range(ns):
            x, u, q = self.store_read_lap(1, i); out["ss_x%d" % i] = x; out["ss_u%d" % i] = u; out["ss_q%d" % i] = q
            out["ss_laptime%d" % i] = np.int64(self.ss_lap_time(i))
        # The lap table names laps by insertion index; the file holds the laps in their SORTED order and restore_stores inserts them in that order, so the
        # table is written in terms of sorted positions -- the insertion indices of the restored context.  Laps of equal length keep their insertion order in
        # the sorted order, hence a row's own order (length, then index) is the same before and after.
        tab = self.model_lap_table() if nm.value else np.zeros((0, 0), np.int32)      # (no laps stored: no table can be in force)
        if tab.shape[0]:
            pos = np.array([self.model_lap_info(k)[1] for k in range(nm.value)], np.int32)      # insertion index -> sorted position
            out["model_lap_table"] = pos[tab]
        # (the safe-set table names laps by their addTrajectory index, which restore_stores keeps)
        srows, slast = self.ss_lap_table() if ns else (np.zeros((0, 0), np.int32), None)
        if srows.shape[0]:
            out["ss_lap_table"] = srows
            if slast is not None:
                out["ss_lap_last"] = slast
        np.savez_compressed(_npz_path(path), n_model=np.int64(nm.value), n_ss=np.int64(ns), N=np.int64(self.N), **out)

    def restore_stores(self, path):
        """Into a context whose stores are EMPTY: the regression laps in their sorted order (a stable sorted insert keeps it), the safe-set laps at their addTrajectory-time
        length followed by the rows addPoint had appended and their Q-function.  The restored context answers every later call bit for bit like the one that was saved.
        `path` is what save_stores was given, with or without the .npz extension."""
        with np.load(_npz_path(path)) as d:
            nm = C.c_int(); _chk(self.lib.lmpc_model_num_laps(self._h, C.byref(nm)))
            if nm.value or self.ss_num_laps():
                raise LmpcError("restore_stores needs a context with empty lap stores")
            for i in range(int(d["n_model"])):
                self.model_add_trajectory(d["model_x%d" % i], d["model_u%d" % i])
            if "model_lap_table" in d.files:                 # (per-problem regression laps, in terms of the insertion indices the loop above has just given)
                self.model_set_lap_table(d["model_lap_table"])
            for i in range(int(d["n_ss"])):
                x, u, q, T0 = d["ss_x%d" % i], d["ss_u%d" % i], d["ss_q%d" % i], int(d["ss_laptime%d" % i])
                self.ss_add_trajectory(x[:T0], u[:T0])
                self.ss_replace_lap(i, x, u, q)          # (always: the saved rows and Q-function, whatever computeCost makes of the first T0 rows)
            if "ss_lap_table" in d.files:                    # (per-problem safe-set laps; a file written without them restores to "no table")
                self.ss_set_lap_table(d["ss_lap_table"], d["ss_lap_last"] if "ss_lap_last" in d.files else None)

    def store_retain(self, ss=None, model=None):
        """Laps given back (lmpc_store_retain): the safe set keeps the laps `ss` lists (strictly ascending indices in ss_add_trajectory order), the regression store
        those `model` lists (strictly ascending insertion indices); None leaves a store untouched, an empty list empties it.  The k-th kept lap gets index k; lap
        tables, `last` and the selection override are renumbered with the stores, and a lap one of them names must be kept.  The device stores shrink to the kept laps.
        Returns (map_ss, map_model): int32 arrays over the laps stored before the call, the new index or -1 for a dropped lap; None for an untouched store."""
        ns, nm = self.ss_num_laps(), self.model_num_laps()
        ks = None if ss is None else check_retain(ss, ns, "safe set")
        km = None if model is None else check_retain(model, nm, "regression store")
        ms, mm = np.full(ns, -1, np.int32), np.full(nm, -1, np.int32)
        _chk(self.lib.lmpc_store_retain(self._h, -1 if ks is None else ks.size, None if ks is None or not ks.size else ks.ctypes.data,
                                        -1 if km is None else km.size, None if km is None or not km.size else km.ctypes.data,
                                        ms.ctypes.data if ns else None, mm.ctypes.data if nm else None))
        return (None if ks is None else ms), (None if km is None else mm)

    def rollout_release(self):
        """Free the device buffers a finished session keeps for the next lap (lmpc_rollout_release)."""
        _chk(self.lib.lmpc_rollout_release(self._h))

    def debug_rollout_capture(self, on=True):
        """Sessions begun after this call keep the selected safe-set points of every step (lmpc_debug_rollout_capture)."""
        _chk(self.lib.lmpc_debug_rollout_capture(self._h, C.c_int(1 if on else 0)))

    def debug_rollout_qp(self, b0, n, selection=True):
        """The QP of the last simulated step for rollouts b0 .. b0 + n - 1: dict(A, B, C, xPred, uPred, lam, ztNext, ztuNext, iters, status[, ssSel (n, S, 6), qSel, succ (n, S, 6),
        succU (n, S, 2)]) -- lmpc_debug_rollout_qp."""
        N, S = self.N, self.cfg.numSS_points
        o = dict(A=np.zeros((n, N, 6, 6)), B=np.zeros((n, N, 6, 2)), C=np.zeros((n, N, 6)), xPred=np.zeros((n, N + 1, 6)), uPred=np.zeros((n, N, 2)), lam=np.zeros((n, S)),
                 ztNext=np.zeros((n, 6)), ztuNext=np.zeros((n, 2)), iters=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
        if selection:
            o.update(ssSel=np.zeros((n, S, 6)), qSel=np.zeros((n, S)), succ=np.zeros((n, S, 6)), succU=np.zeros((n, S, 2)))
        g = lambda k: _d(o[k]) if k in o else None
        _chk(self.lib.lmpc_debug_rollout_qp(self._h, C.c_int(int(b0)), C.c_int(int(n)), g("A"), g("B"), g("C"), g("xPred"), g("uPred"), g("ssSel"), g("qSel"), g("succ"), g("succU"),
                                            g("lam"), g("ztNext"), g("ztuNext"), g("iters"), g("status")))
        return o

    def ss_extend_lap(self, lap, x, u, track_row=None):
        """track_row: the row of track_set whose TrackLength is added to s (lmpc_ss_extend_lap_on); None: the config's, or the one row's."""
        x = _f64(x); u = _f64(u)
        if track_row is None:
            _chk(self.lib.lmpc_ss_extend_lap(self._h, C.c_int(int(lap)), _d(x), _d(u), C.c_int(x.shape[0])))
        else:
            _chk(self.lib.lmpc_ss_extend_lap_on(self._h, C.c_int(int(track_row)), C.c_int(int(lap)), _d(x), _d(u), C.c_int(x.shape[0])))

    def rollout_commit_laps(self, cars, rows=None, ss=True, model=True):
        """Laps of the active session into the lap stores on the device (lmpc_rollout_commit_laps): entry i is rows [0, rows[i]) of car cars[i] as the session logged
        them (rows=None: up to each car's crossing step), added to the safe set (ss) and / or the regression store (model) in the order listed -- what
        ss_add_trajectory / model_add_trajectory make of the fetched rows, bit for bit, without the fetch.  Returns (first_ss, first_model): the index of the first new
        lap in each store (None for a store not written); the others follow consecutively."""
        cars = _i32(np.atleast_1d(cars))
        if cars.ndim != 1:
            raise ValueError("rollout_commit_laps: cars must be one-dimensional")
        if rows is not None:
            rows = _i32(np.atleast_1d(rows))
            if rows.shape != cars.shape:
                raise ValueError("rollout_commit_laps: one row count per listed car expected")
        fs = C.c_int(-1); fm = C.c_int(-1)
        stores = (COMMIT_SS if ss else 0) | (COMMIT_MODEL if model else 0)
        _chk(self.lib.lmpc_rollout_commit_laps(self._h, cars.shape[0], cars.ctypes.data, None if rows is None else rows.ctypes.data, stores, C.byref(fs), C.byref(fm)))
        return (fs.value if ss else None), (fm.value if model else None)

    def rollout_lap_metrics(self, cars, rows=None):
        """(n, METRICS_NCOL) lap metrics of the active session, reduced on the device (lmpc_rollout_lap_metrics): row i covers rows [0, rows[i]) of car cars[i] as the
        session logged them (rows=None: up to each car's crossing step), columns METRIC_FIELDS.  Reads only; refused like rollout_commit_laps."""
        cars = _i32(np.atleast_1d(cars))
        if cars.ndim != 1:
            raise ValueError("rollout_lap_metrics: cars must be one-dimensional")
        if rows is not None:
            rows = _i32(np.atleast_1d(rows))
            if rows.shape != cars.shape:
                raise ValueError("rollout_lap_metrics: one row count per listed car expected")
        out = np.zeros((cars.shape[0], METRICS_NCOL))
        _chk(self.lib.lmpc_rollout_lap_metrics(self._h, cars.shape[0], cars.ctypes.data, None if rows is None else rows.ctypes.data, out.ctypes.data))
        return out

    def rollout_extend_laps(self, cars, laps, n_rows):
        """The first n_rows logged rows of car cars[i] appended to safe-set lap laps[i] on the device (lmpc_rollout_extend_laps: ss_extend_lap of the fetched rows
        without the fetch).  Returns a bool array: False where a row held a non-finite value -- that lap is left as it was."""
        cars = _i32(np.atleast_1d(cars)); laps = _i32(np.atleast_1d(laps))
        if cars.ndim != 1 or laps.shape != cars.shape:
            raise ValueError("rollout_extend_laps: one safe-set lap per listed car expected")
        ext = np.zeros(cars.shape[0], np.int32)
        _chk(self.lib.lmpc_rollout_extend_laps(self._h, cars.shape[0], cars.ctypes.data, laps.ctypes.data, int(n_rows), ext.ctypes.data))
        return ext != 0

    # ---- free-running sessions (lmpc_rollout_relaunch; csrc/lmpc_relaunch.hip.h)
    def rollout_relaunch(self, cars, lap_rows):
        """The listed cars of the active session -- each has crossed the line -- start their next lap on the device, as a fresh rollout_begin would start it
        (lmpc_rollout_relaunch): state = crossing state less the car's own TrackLength, linearisation about rows 1 .. N + 1 of the lap just ended, every other array
        of the step zeroed, device noise redrawn for the next lap_rows steps, the car's lap-table row taken anew from the table in force.  Between two rollout_run
        calls; afterwards rollout_commit_laps / rollout_extend_laps count a car's rows from its lap start (rollout_lap_start)."""
        cars, lap_rows = check_relaunch(cars, lap_rows)
        _chk(self.lib.lmpc_rollout_relaunch(self._h, cars.shape[0], cars.ctypes.data, lap_rows))

    def rollout_lap_start(self):
        """(start (B,) int32, lap (B,) int32) of the active session (lmpc_rollout_lap_start): the session row each car's current lap began at and the laps it has
        begun after its first; zeros in a session without a relaunch."""
        ro = getattr(self, "_ro", None)           # (no session begun so far: the library says so)
        start = np.zeros(ro[0] if ro else 0, np.int32); lap = np.zeros_like(start)
        _chk(self.lib.lmpc_rollout_lap_start(self._h, start.ctypes.data if start.size else None, lap.ctypes.data if lap.size else None))
        return start, lap

    def debug_model_image(self, lap):
        """(q (3, rows - 1) uint32, par (chunks, 6), chunks): the prefilter image of the regression-store lap with insertion index `lap` (lmpc_debug_model_image)."""
        rows, _ = self.model_lap_info(lap)
        n = C.c_int()
        _chk(self.lib.lmpc_debug_model_image(self._h, int(lap), None, None, C.byref(n)))
        q = np.zeros((3, rows - 1), np.uint32); par = np.zeros((n.value, 6))
        _chk(self.lib.lmpc_debug_model_image(self._h, int(lap), q.ctypes.data, par.ctypes.data, C.byref(n)))
        return q, par, n.value

    def ss_truncate_lap(self, lap, T):
        _chk(self.lib.lmpc_ss_truncate_lap(self._h, C.c_int(int(lap)), C.c_int(int(T))))

    def ss_num_laps(self):
        n = C.c_int()
        _chk(self.lib.lmpc_ss_num_laps(self._h, C.byref(n)))
        return n.value

    def ss_lap_time(self, lap):
        """LMPC.LapTime[lap]: rows of the stored lap when it was added (addPoint extensions not counted)."""
        T = C.c_int()
        _chk(self.lib.lmpc_ss_get_laptime(self._h, C.c_int(int(lap)), C.byref(T)))
        return T.value

    def ss_lap_rows(self, lap):
        T = C.c_int()
        _chk(self.lib.lmpc_ss_get_qfun(self._h, C.c_int(int(lap)), None, C.byref(T)))
        return T.value

    # ---- multi-GPU exchange (RCCL behind the C ABI; see parallel.py for the rendezvous)
    def comm_init(self, id_bytes, rank, world):
        buf = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(bytes(id_bytes))
        _chk(self.lib.lmpc_comm_init(self._h, buf, C.c_int(int(rank)), C.c_int(int(world))))

    def comm_destroy(self):
        _chk(self.lib.lmpc_comm_destroy(self._h))

    def comm_info(self):
        r, w, f = C.c_int(), C.c_int(), C.c_int()
        _chk(self.lib.lmpc_comm_info(self._h, C.byref(r), C.byref(w), C.byref(f)))
        return r.value, w.value, bool(f.value)

    def comm_allgather(self, arr):
        """Every rank's `arr` (same shape / dtype everywhere), stacked along a new leading axis of length world."""
        arr = np.ascontiguousarray(arr)
        world = self.comm_info()[1]
        out = np.empty((world,) + arr.shape, dtype=arr.dtype)
        _chk(self.lib.lmpc_comm_allgather(self._h, _d(arr), _d(out), C.c_longlong(arr.nbytes)))
        return out

    def comm_allreduce_max(self, values):
        v = np.ascontiguousarray(np.atleast_1d(np.asarray(values, dtype=np.float64)))
        _chk(self.lib.lmpc_comm_allreduce_max(self._h, _d(v), C.c_int(v.shape[0])))
        return v

    def comm_barrier(self):
        _chk(self.lib.lmpc_comm_barrier(self._h))

    def rollout_exchange(self, K, T_max):
        """Per-lap exchange of the current rollout session (device-packed records, one ncclAllGather).
        Returns (records (world, K, T_max + 1, 14), lens (world, K), number of valid laps on this rank)."""
        world = self.comm_info()[1]
        rec = np.zeros((world, K, T_max + 1, 14)); ln = np.zeros((world, K), dtype=np.int64); nv = C.c_int()
        _chk(self.lib.lmpc_rollout_exchange(self._h, C.c_int(int(K)), C.c_int(int(T_max)), _d(rec), _d(ln), C.byref(nv)))
        return rec, ln, nv.value

    def solver_waves(self, B):
        return int(self.lib.lmpc_solver_waves(self._h, C.c_int(int(B))))

    def solver_lds(self):
        """dict lds_1w, lds_1w_abg, lds_mw (dynamic LDS per QP in bytes; 0: this (N, numSS_points) has no such kernel) and n_cu: what the routes are chosen from."""
        out = (C.c_ulonglong * 4)()
        _chk(self.lib.lmpc_solver_lds(self._h, out))
        return dict(lds_1w=int(out[0]), lds_1w_abg=int(out[1]), lds_mw=int(out[2]), n_cu=int(out[3]))

    def global_position_batch(self, s, ey):
        """Map.getGlobalPosition for arrays of (s, ey): returns xy (n, 2) and status (n,)."""
        s = _f64(np.ravel(s)); ey = _f64(np.ravel(ey)); n = s.shape[0]
        xy = np.zeros((n, 2)); st = np.zeros(n, np.int32)
        _chk(self.lib.lmpc_global_position_batch(self._h, C.c_int(n), _d(s), _d(ey), _d(xy), _d(st)))
        return xy, st

    def local_position(self, x, y, psi, max_ey):
        """Map.getLocalPosition (Track.py:191-290) for arrays of inertial poses (x, y, psi): returns s, ey, epsi (n,) and status (n,) -- ST_NO_SEGMENT with
        s = ey = epsi = 10000 where no track row completes or an input is not finite.  max_ey: the reference's halfWidth + slack (0.85 on its track)."""
        x = _f64(np.ravel(x)); y = _f64(np.ravel(y)); psi = _f64(np.ravel(psi)); n = x.shape[0]
        if y.shape[0] != n or psi.shape[0] != n:
            raise ValueError("local_position: x, y, psi must have the same number of elements, got %d, %d, %d" % (n, y.shape[0], psi.shape[0]))
        s = np.zeros(n); ey = np.zeros(n); epsi = np.zeros(n); st = np.zeros(n, np.int32)
        _chk(self.lib.lmpc_local_position_batch(self._h, n, x.ctypes.data, y.ctypes.data, psi.ctypes.data, float(max_ey), s.ctypes.data, ey.ctypes.data, epsi.ctypes.data, st.ctypes.data))
        return s, ey, epsi, st

    def track_angle(self, s, epsi):
        """Map.getAngle (Track.py:312-349) for arrays of (s, epsi): returns psi (n,) and status (n,) -- ST_NO_SEGMENT with psi = 0 where the reference raises."""
        s = _f64(np.ravel(s)); epsi = _f64(np.ravel(epsi)); n = s.shape[0]
        if epsi.shape[0] != n:
            raise ValueError("track_angle: s and epsi must have the same number of elements, got %d, %d" % (n, epsi.shape[0]))
        psi = np.zeros(n); st = np.zeros(n, np.int32)
        _chk(self.lib.lmpc_track_angle_batch(self._h, n, s.ctypes.data, epsi.ctypes.data, psi.ctypes.data, st.ctypes.data))
        return psi, st

    def state_from_global(self, xglob, max_ey):
        """Rows [vx, vy, wz, psi, X, Y] of a session log, (T, B, 6) or (T, 6), to rows [vx, vy, wz, epsi, s, ey] of the same shape (lmpc_state_from_global_batch):
        returns (x, status) with status (T, B) or (T,).  Every row on its own: s lies on the first lap (rollout.lap_from_global makes it continuous)."""
        xg = _f64(xglob)
        if xg.ndim not in (2, 3) or xg.shape[-1] != 6:
            raise ValueError("state_from_global: (T, B, 6) or (T, 6) rows [vx, vy, wz, psi, X, Y] expected, got shape %s" % (xg.shape,))
        T = xg.shape[0]; B = xg.shape[1] if xg.ndim == 3 else 1
        x = np.zeros(xg.shape); st = np.zeros(xg.shape[:-1], np.int32)
        _chk(self.lib.lmpc_state_from_global_batch(self._h, T, B, xg.ctypes.data, float(max_ey), x.ctypes.data, st.ctypes.data))
        return x, st

    def selftest(self):
        _chk(self.lib.lmpc_selftest(self._h))

    # ---- developer flavours only (build.build_flavour with LMPC_TRACE / LMPC_EXEC_AUDIT; the product library refuses both calls)
    TRACE_ROWS = 48

    def debug_trace_begin(self, B):
        """Device buffer for the per-iteration trace of the next solve launches of up to B problems; returns its handle for debug_trace_fetch."""
        p = self.dev_alloc(B * self.TRACE_ROWS * 6 * 8)
        self.dev_upload(p, np.full((B, self.TRACE_ROWS, 6), np.nan))
        _chk(self.lib.lmpc_debug_set_trace(self._h, _p(p)))
        return p

    def debug_trace_fetch(self, p, B):
        """(B, 48, 6) rows (gap, r_d, r_e, sigma, alpha_p, alpha_d) per iteration, NaN where no iteration ran; switches the trace off and frees the buffer."""
        out = np.zeros((B, self.TRACE_ROWS, 6))
        self.sync(); self.dev_download(p, out)
        _chk(self.lib.lmpc_debug_set_trace(self._h, None)); self.dev_free(p)
        return out

    def debug_rollout_peek(self, B):
        """(xLin (B, N+1, 6), uLin (B, N, 2), status (B,), rstatus (B, N)) of the running rollout session, see lmpc_debug_rollout_peek."""
        N = self.N
        xl = np.zeros((B, N + 1, 6)); ul = np.zeros((B, N, 2)); st = np.zeros(B, np.int32); rs = np.zeros((B, N), np.int32)
        _chk(self.lib.lmpc_debug_rollout_peek(self._h, _d(xl), _d(ul), _d(st), _d(rs)))
        return xl, ul, st, rs

    def debug_exec_audit(self, reset=True):
        """(partial[8], calls[8]) of the cross-lane primitives since the last reset (sites: csrc/lmpc_kernels.hip.h)."""
        out = (C.c_ulonglong * 16)()
        _chk(self.lib.lmpc_debug_exec_audit(self._h, out, C.c_int(1 if reset else 0)))
        v = np.array(list(out), dtype=np.uint64)
        return v[:8], v[8:]

    def debug_k1_ahead(self):
        """(chained, unchained) regression launches of step_batch_dev since the context was created: chained ones ran on the look-ahead stream beside the previous step's solve (see lmpc_debug_k1_ahead)."""
        out = (C.c_longlong * 2)()
        _chk(self.lib.lmpc_debug_k1_ahead(self._h, out))
        return int(out[0]), int(out[1])

    def debug_k1_merge(self):
        """(two-role launches, held solves launched stand-alone, regression launches of step_batch_dev in a kernel of their own) since the context was created (see lmpc_debug_k1_merge)."""
        out = (C.c_longlong * 3)()
        _chk(self.lib.lmpc_debug_k1_merge(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def set_profiling(self, every):
        """False / 0: off; True / 1: events around every kernel launch; k: around every k-th launch of each kernel (see lmpc_set_profiling)."""
        _chk(self.lib.lmpc_set_profiling(self._h, C.c_int(int(every))))

    def stats(self):
        s = LmpcStats()
        _chk(self.lib.lmpc_get_stats(self._h, C.byref(s)))
        return s

    def reset_stats(self):
        _chk(self.lib.lmpc_reset_stats(self._h))


def config_from(N, Q, R, Qf, dR, Qslack, Fx, bx, Fu, bu, xRef, QterminalSlack=None, numSS_Points=0, numSS_it=0, trToUse=0,
                track=None, trackLength=0.0, max_batch=256, max_laps=64, max_lap_len=2048, device=0, slacks=True, **solver):
    """Build an LmpcConfig from the numeric content of MPCParams / LMPC ctor args / Map."""
    cfg = default_config()
    cfg.N = int(N); cfg.numSS_it = int(numSS_it); cfg.numSS_points = int(numSS_Points) if numSS_it else 0; cfg.trToUse = int(trToUse)
    set_arr(cfg.Q, np.asarray(Q, float)); set_arr(cfg.R, np.asarray(R, float)); set_arr(cfg.Qf, np.asarray(Qf, float))
    set_arr(cfg.dR, np.asarray(dR, float)); set_arr(cfg.Qslack, np.asarray(Qslack, float)); set_arr(cfg.xRef, np.asarray(xRef, float))
    Fx = np.asarray(Fx, float); Fu = np.asarray(Fu, float)
    if Fx.shape != (2, 6) or Fu.shape != (4, 2):
        raise LmpcError("only the reference's constraint shapes are supported: Fx (2,6), Fu (4,2); got %s %s" % (Fx.shape, Fu.shape))
    set_arr(cfg.Fx, Fx); set_arr(cfg.Fu, Fu)
    set_arr(cfg.bx, np.squeeze(np.asarray(bx, float))); set_arr(cfg.bu, np.squeeze(np.asarray(bu, float)))
    if QterminalSlack is not None:
        set_arr(cfg.QtermSlack, np.asarray(QterminalSlack, float))
    if track is not None:
        track = np.asarray(track, float)
        if track.shape[0] > MAX_TRACK_ROWS:
            raise LmpcError("track table too long")
        for i, v in enumerate(track.reshape(-1)):
            cfg.track[i] = float(v)
        cfg.track_rows = track.shape[0]
    cfg.trackLength = float(trackLength)
    cfg.max_batch, cfg.max_laps, cfg.max_lap_len, cfg.device = int(max_batch), int(max_laps), int(max_lap_len), int(device)
    cfg.slacks = 1 if slacks else 0
    for k, v in solver.items():
        setattr(cfg, k, v)
    return cfg


_POOL_MEMBER = False


def _pool_member(cfg):
    """Context(cfg) as a ContextPool creates it: without the look-ahead regression (k1_ahead=False) -- several batches in flight fill the idle CUs already, and chained
    members measured 3-5 % slower (profiles/k1_ahead_ab.json, pipelined_batches).  The constructor is called as Context(cfg), the one form every stand-in of it takes."""
    global _POOL_MEMBER
    _POOL_MEMBER = True
    try:
        return Context(cfg)
    finally:
        _POOL_MEMBER = False


class ContextPool:
    """`depth` contexts on one device -- one HIP stream, one set of work buffers, one copy of the (small) lap stores each -- for callers that keep several INDEPENDENT
    batches in flight.  Inside one launch the CUs whose QP has converged idle until the slowest QP of the batch has (mean 8.6 against a maximum of 13 iterations at batch
    256); with the next batch queued on another stream its work-groups start on those CUs: 1.21 -> 1.66 M solves/s at batch 256 with three in flight, 1.84 -> 3.14 M at
    batch 512 (tools/pipelined_bench.py).  Store edits go to every member; `step_batch_dev` deals the steps to the members in turn and returns the member it used.
    A closed loop -- step t + 1 needs step t -- cannot use it; batched requests can."""

    def __init__(self, cfg, depth=2):
        if int(depth) < 1:
            raise ValueError("ContextPool: depth must be at least 1")
        self.members = []; self._next = 0
        try:
            for _ in range(int(depth)):
                self.members.append(_pool_member(cfg))
        except Exception:
            self.close()                               # (a member that failed to come up does not leave the earlier ones' device memory behind)
            raise

    def __getattr__(self, name):                       # lap-store edits (model_add_trajectory, ss_add_trajectory, ss_add_point, ss_set_selected, ...): the same call on every member
        if name in ("members", "_next"):               # (not set yet: a failed __init__ must not recurse through this hook)
            raise AttributeError(name)
        if name in ("plant_set_params", "tuning_set", "track_set") or (name.startswith(("model_", "ss_")) and not name.startswith(("ss_get", "ss_num", "ss_lap", "model_num", "model_lap"))):   # (the vehicle too: the same on every member; model_set_lap_table and ss_set_lap_table go with the store edits, the queries model_lap_table / model_lap_info / ss_lap_table to the first)
            def forward(*a, **kw):
                out = None
                for m in self.members:
                    out = getattr(m, name)(*a, **kw)
                return out
            return forward
        return getattr(self.members[0], name)

    def restore_stores(self, path):
        """Context.restore_stores into every member (step_batch_dev deals steps to all of them; save_stores may go to any one: their stores are equal)."""
        for m in self.members:
            m.restore_stores(path)

    def store_retain(self, ss=None, model=None):
        """Context.store_retain on every member (their stores are equal, so are the maps); returns the maps of the last one."""
        out = None
        for m in self.members:
            out = m.store_retain(ss=ss, model=model)
        return out

    def step_dev_buffers(self, inp, diagnostics=True):
        """One set of device buffers per member: [(args, allocations)], in member order."""
        return [m.step_dev_buffers(inp, diagnostics=diagnostics) for m in self.members]

    def step_batch_dev(self, B, args_per_member):
        i = self._next; self._next = (i + 1) % len(self.members)
        self.members[i].step_batch_dev(B, args_per_member[i][0])
        return i

    def sync(self):
        for m in self.members:
            m.sync()

    def close(self):
        for m in self.members:
            m.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
