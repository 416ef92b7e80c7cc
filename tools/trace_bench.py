"""Developer tool (GPU box): what a session trace costs.  One LMPC generation (lmpc_rollout_begin, lmpc_rollout_run to the end, lmpc_rollout_fetch of the logs,
lmpc_rollout_end) of B cars, T_max = 400, on the bench's seed lap, timed on the host clock around calls that end in a device synchronise, for

    a  parent      another build of the library without the trace (--parent-lib FILE: the parent commit's liblmpc_hip.so), same calls
    b  off         this tree, trace off
    c  8cars       this tree, 8 cars traced, all planes
    d  solver      this tree, every car traced, SOLVER plane only
    e  all         this tree, every car traced, all planes
    c' / e'        c and e with LMPC_TRACE_OWN_STREAM=1: the trace kernel on a stream of its own beside the plant (and a second event for the next solve) instead of
                   behind the plant kernel on the plant stream

    a2 / b2        a and b once more on contexts of their own, created last: what two contexts of ONE library differ by (the first variant of the list is also the first
                   context of the process)

One process, one fresh context per variant, one warm-up generation each, then --repeats rounds in which the variants alternate, the round starting one variant
further down the list each time (so that no variant always runs behind the same neighbour); median and range per variant.  The
traced variants also fetch their trace (timed apart: `fetch_trace_s`).  Every variant goes through the same ctypes calls on the C ABI, so that (a) needs nothing of
the Python layer the older library does not have.  Writes one JSON document (--out).

    python tools/trace_bench.py --parent-lib racinglmpc_amd/liblmpc_hip_parent.so --out profiles/session_trace.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench

N = 12


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Lib:
    """The C ABI of one build of the library, called without declared argument types (every argument is wrapped here)."""

    def __init__(self, path):
        self.path = path
        self.lib = C.CDLL(path)
        self.lib.lmpc_last_error.restype = C.c_char_p
        self.version = int(self.lib.lmpc_version())

    def chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s: error %d: %s" % (what, rc, self.lib.lmpc_last_error().decode()))

    def context(self, g, B):
        from racinglmpc_amd import _capi
        cfg = _capi.default_config()
        cfg.N = N; cfg.max_batch = B; cfg.device = 0
        for i, v in enumerate(g["track"].reshape(-1)):
            cfg.track[i] = float(v)
        cfg.track_rows = g["track"].shape[0]; cfg.trackLength = g["trackLength"]
        h = C.c_void_p()
        self.chk(self.lib.lmpc_create(C.byref(cfg), C.byref(h)), "lmpc_create")
        x, u = np.ascontiguousarray(g["xPID"]), np.ascontiguousarray(g["uPID"])
        for _ in range(4):
            self.chk(self.lib.lmpc_model_add_trajectory(h, _p(x), _p(u), C.c_int(x.shape[0])), "model_add_trajectory")
            self.chk(self.lib.lmpc_ss_add_trajectory(h, _p(x), _p(u), C.c_int(x.shape[0])), "ss_add_trajectory")
        return h


def generation(L, h, inp, T_max, trace):
    """One generation; returns (seconds of begin + run + fetch + end, seconds of fetch_trace, simulated steps, cars that crossed)."""
    from racinglmpc_amd import _capi
    x0, xl, ul, noise = inp
    B = x0.shape[0]
    lib = L.lib
    t = C.c_int(); nd = C.c_int()
    X = np.empty((T_max, B, 6)); U = np.empty((T_max, B, 2)); G = np.empty((T_max, B, 6))
    done = np.zeros(B, np.int32); st = np.zeros(B, np.int32); fx = np.zeros((B, 6)); fg = np.zeros((B, 6))
    planes = {}
    if trace is not None:
        cars, what = trace
        planes = {k: np.empty((T_max, len(cars)) + tuple(shp), dt) for k, bit, shp, dt in _capi.trace_planes(N, 48, what)}
    t0 = time.perf_counter()
    L.chk(lib.lmpc_rollout_begin(h, C.c_int(B), C.c_int(T_max), _p(x0), _p(x0), _p(xl), _p(ul), _p(noise)), "rollout_begin")
    L.chk(lib.lmpc_rollout_run(h, C.c_int(T_max), C.byref(t), C.byref(nd)), "rollout_run")
    L.chk(lib.lmpc_rollout_fetch(h, C.c_int(0), C.c_int(t.value), _p(X), _p(U), _p(G), _p(done), _p(st), _p(fx), _p(fg)), "rollout_fetch")
    t1 = time.perf_counter()
    if trace is not None:
        out = _capi.TraceOut(**{k: v.ctypes.data for k, v in planes.items()})
        L.chk(lib.lmpc_rollout_fetch_trace(h, C.c_int(0), C.c_int(t.value), C.byref(out)), "rollout_fetch_trace")
    t2 = time.perf_counter()
    L.chk(lib.lmpc_rollout_end(h), "rollout_end")
    t3 = time.perf_counter()
    return (t1 - t0) + (t3 - t2), t2 - t1, t.value, nd.value, (X[:t.value], U[:t.value], done, st)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="a build of the library without the trace (the parent commit's): variant a")
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--steps", type=int, default=400, help="T_max")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--this-first", action="store_true", help="create this tree's trace-off context first and the parent's second (what the place in the creation order is worth)")
    ap.add_argument("--out", default="profiles/session_trace.json")
    a = ap.parse_args()
    from racinglmpc_amd import _capi
    g = bench.load_seed()
    here = Lib(_capi.LIB_PATH)
    parent = Lib(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    doc = dict(tool="tools/trace_bench.py", creation_order="this tree first" if a.this_first else "parent first", N=N, T_max=a.steps, repeats=a.repeats, library_version=here.version, parent_version=parent.version if parent else None,
               timing="host clock around begin + run + fetch + end (each ends in a device synchronise); fetch_trace timed apart", batches={})
    for B in [int(b) for b in a.batches.split(",")]:
        x0 = np.tile(np.array([0.5, 0, 0, 0, 0, 0.0]), (B, 1)); x0[:, 5] = np.linspace(-0.1, 0.1, B); x0[:, 0] += np.linspace(0.0, 0.1, B)
        xl = np.ascontiguousarray(np.tile(g["xPID"][None, 1:N + 2], (B, 1, 1))); ul = np.ascontiguousarray(np.tile(g["uPID"][None, 1:N + 1], (B, 1, 1)))
        noise = np.random.default_rng(100).standard_normal((a.steps, B, 3))
        inp = (x0, xl, ul, noise)
        every = np.arange(B, dtype=np.int32); eight = np.ascontiguousarray(np.linspace(0, B - 1, 8).astype(np.int32))
        variants = []                    # (name, library, trace, LMPC_TRACE_OWN_STREAM)
        if parent:
            variants.append(("a_parent", parent, None, None))
        variants += [("b_off", here, None, None), ("c_8cars_all", here, (eight, _capi.TRACE_ALL), None), ("d_every_solver", here, (every, _capi.TRACE_SOLVER), None),
                     ("e_every_all", here, (every, _capi.TRACE_ALL), None), ("c_8cars_all_own_stream", here, (eight, _capi.TRACE_ALL), "1"),
                     ("e_every_all_own_stream", here, (every, _capi.TRACE_ALL), "1")]
        if parent:
            variants.append(("a2_parent_again", parent, None, None))
        variants.append(("b2_off_again", here, None, None))
        if parent and a.this_first:
            variants[0], variants[1] = variants[1], variants[0]
        ctxs, res, ref = {}, {}, None

        def one(name, L, trace, knob):
            if knob is None:
                os.environ.pop("LMPC_TRACE_OWN_STREAM", None)
            else:
                os.environ["LMPC_TRACE_OWN_STREAM"] = knob
            if trace is not None:
                L.chk(L.lib.lmpc_rollout_set_trace(ctxs[name], C.c_int(len(trace[0])), _p(trace[0]), C.c_uint(trace[1])), "rollout_set_trace")
            return generation(L, ctxs[name], inp, a.steps, trace)
        for name, L, trace, knob in variants:                       # fresh contexts, one warm-up generation each; the logs of all variants must agree
            ctxs[name] = L.context(g, B)
            s, f, steps, nd, logs = one(name, L, trace, knob)
            res[name] = dict(seconds=[], fetch_trace_s=[], steps=steps, crossed=nd,
                             trace_bytes=0 if trace is None else _capi.trace_bytes(N, 48, len(trace[0]), trace[1], a.steps))
            if ref is None:
                ref = logs
            res[name]["logs_equal_first_variant"] = bool(all(np.array_equal(p.view(np.int64) if p.dtype == np.float64 else p, q.view(np.int64) if q.dtype == np.float64 else q)
                                                             for p, q in zip(logs, ref)))
        for rnd in range(a.repeats):
            for name, L, trace, knob in variants[rnd % len(variants):] + variants[:rnd % len(variants)]:
                s, f, steps, nd, _logs = one(name, L, trace, knob)
                res[name]["seconds"].append(s); res[name]["fetch_trace_s"].append(f)
        os.environ.pop("LMPC_TRACE_OWN_STREAM", None)
        for name, L, trace, knob in variants:
            L.chk(L.lib.lmpc_destroy(ctxs[name]), "lmpc_destroy")
            r = res[name]
            r.update(median_s=statistics.median(r["seconds"]), min_s=min(r["seconds"]), max_s=max(r["seconds"]), fetch_trace_median_s=statistics.median(r["fetch_trace_s"]),
                     ms_per_step=1e3 * statistics.median(r["seconds"]) / max(r["steps"], 1))
            print("B=%5d %-22s median %.4f s (range %.4f .. %.4f), %d steps, %.3f ms/step, fetch_trace %.4f s, planes %.1f MB, logs equal: %s" % (
                B, name, r["median_s"], r["min_s"], r["max_s"], r["steps"], r["ms_per_step"], r["fetch_trace_median_s"], r["trace_bytes"] / 1e6, r["logs_equal_first_variant"]), flush=True)
        if parent:
            pa, off = res["a_parent"], res["b_off"]
            res["untraced_within_parent_range"] = bool(pa["min_s"] <= off["median_s"] <= pa["max_s"])
            both = res["a_parent"]["seconds"] + res["a2_parent_again"]["seconds"]
            res["untraced_within_range_of_both_parent_contexts"] = bool(min(both) <= off["median_s"] <= max(both))
            print("B=%5d trace off: median %.4f s against the parent's range %.4f .. %.4f -> %s" % (B, off["median_s"], pa["min_s"], pa["max_s"],
                  "inside" if res["untraced_within_parent_range"] else "OUTSIDE"), flush=True)
        doc["batches"][str(B)] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
