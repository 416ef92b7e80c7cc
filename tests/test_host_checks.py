"""CPU checks of the test infrastructure itself: the vectorised KKT certificate against the dense oracle certificate on the
reference-produced fixture, and the construction of the K1 prefilter edge case."""
import numpy as np
import pytest

from tests import common, k1_cases, kkt_batch


def _split(z, N=12, S=48):
    x = z[:, :6 * (N + 1)].reshape(-1, N + 1, 6); o = 6 * (N + 1)
    u = z[:, o:o + 2 * N].reshape(-1, N, 2); o += 2 * N
    s = z[:, o:o + 2 * N]; o += 2 * N
    return x, u, s, z[:, o:o + S], z[:, o + S:o + S + 6]


def test_batch_certificate_agrees_with_dense_oracle_certificate():
    """On the 60 recorded QPs: the certified optimum passes the banded certificate at the level of the dense one, and a
    1e-5 perturbation of one input is caught."""
    from oracle import lmpc_oracle as orc
    g = common.load_lmpc_golden()
    par = orc.QPParams.lmpc_default(12)
    x, u, s, lam, sT = _split(g["rec_sol_opt"])
    mu = g["rec_y_opt"][:, :144]
    ss = np.transpose(g["rec_SSsel"], (0, 2, 1))
    c = kkt_batch.certificate(par, g["rec_A"], g["rec_B"], g["rec_C"], g["rec_x0"], g["rec_OldInput"], x, u, s, mu, ssSel=ss, qSel=g["rec_Qsel"], lambd=lam, sTerm=sT)
    assert c["worst"].max() < 1e-8 and c["worst"].max() <= 10 * max(g["rec_cert_opt"].max(), 1e-10)
    u2 = u.copy(); u2[:, 3, 0] += 1e-5
    c2 = kkt_batch.certificate(par, g["rec_A"], g["rec_B"], g["rec_C"], g["rec_x0"], g["rec_OldInput"], x, u2, s, mu, ssSel=ss, qSel=g["rec_Qsel"], lambd=lam, sTerm=sT)
    assert c2["worst"].min() > 1e-6
    # the reference flow's eps = 1e-3 answers (polish failed) do not pass, its polished answers do
    xr, ur, sr, lr, tr = _split(g["rec_sol"])
    c3 = kkt_batch.certificate(par, g["rec_A"], g["rec_B"], g["rec_C"], g["rec_x0"], g["rec_OldInput"], xr, ur, sr, np.maximum(g["rec_y"][:, :144], 0.0),
                               ssSel=ss, qSel=g["rec_Qsel"], lambd=lr, sTerm=tr)
    ok = g["rec_polish"] == 1
    assert c3["worst"][ok].max() < 1e-6 and c3["worst"][~ok].min() > 1e-6


def test_batch_certificate_plain_mpc():
    from oracle import lmpc_oracle as orc
    gl = common.load_ltv_golden()
    par = orc.QPParams.mpc_default(12, 0.8)
    z, y = gl["sol_opt"], gl["y_opt"]
    x = z[:, :78].reshape(-1, 13, 6); u = z[:, 78:102].reshape(-1, 12, 2); s = z[:, 102:126]
    c = kkt_batch.certificate(par, gl["A"], gl["B"], gl["C"], gl["x0"], gl["OldInput"], x, u, s, y[:, :96])
    assert c["worst"].max() < 1e-8


def test_k1_slack_case_construction(monkeypatch):
    """The constructed lap really puts a row of the exact top 7 at integer distance T + 9 (so a prefilter slack of 8 drops it)."""
    from oracle import lmpc_oracle as orc
    case = k1_cases.slack_case()
    emu = k1_cases.emulate_prefilter(case)
    assert emu["T"] == case["E0"] + 6
    assert emu["e"][case["victim"]] == emu["T"] + 9
    assert [int(emu["e"][r]) for r in case["decoys"]] == [case["E0"] + i for i in range(7)]
    monkeypatch.setattr(orc, "H_BAND", case["h"]); monkeypatch.setattr(orc, "SCALING", np.ones(5))
    idx, K = orc.compute_indices(case["x"], case["u"], np.hstack([case["xq"][:3], case["uq"]]))
    assert sorted(idx) == sorted(case["decoys"][:6] + [case["victim"]])
    assert sorted(idx) == sorted(emu["exact_top"])


def test_bench_watchdog_prints_one_line_and_exits_non_zero():
    """bench.py's headline watchdog (a collective that never returns must not leave the job hanging, nor end it with rc 0): while the main thread sits in a call
    that does not come back, rank 0 prints one JSON line with `rccl_error` naming the phase, and the process ends with status 3."""
    import json
    import subprocess
    import sys
    code = ("import sys, time; sys.path.insert(0, %r); import bench; "
            "wd = bench.Watchdog(0, 2, lambda m: {'metric': 'QP solves/sec (N=12, nx=6, nu=2)', 'value': None, 'rccl_error': m}); "
            "wd.arm(0.3, 'closing barrier'); time.sleep(30)") % common.ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=60)
    assert r.returncode == 3, (r.returncode, r.stderr[-300:])
    line = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert line["value"] is None and "closing barrier did not return within 0 s on rank 0" in line["rccl_error"]
    # a single rank arms nothing (no collective to hang in)
    code1 = code.replace("bench.Watchdog(0, 2,", "bench.Watchdog(0, 1,").replace("time.sleep(30)", "time.sleep(0.6); print('alive')")
    r1 = subprocess.run([sys.executable, "-c", code1], capture_output=True, timeout=60)
    assert r1.returncode == 0 and r1.stdout.decode().strip() == "alive"


def test_noise_prefetch_keeps_the_draw_order():
    """BatchedRollouts.prefetch_noise / the per-lap prefetch of the plant noise: the generator is consumed in exactly the order it would be without them,
    a prefetched array of another shape is discarded together with its draws."""
    from racinglmpc_amd import rollout

    def mk():
        r = rollout.BatchedRollouts.__new__(rollout.BatchedRollouts)
        r.rng = np.random.default_rng(5); r._pre = None; r.global_noise = False; r.noise_shard = None
        return r
    ref = np.random.default_rng(5)
    want = [ref.standard_normal((10, 4, 3)), ref.standard_normal((10, 4, 3)), ref.standard_normal((7, 4, 3))]
    a = mk(); got = [a._draw_noise(10, 4), a._draw_noise(10, 4), a._draw_noise(7, 4)]
    assert all(np.array_equal(x, y) for x, y in zip(want, got))
    b = mk(); b.prefetch_noise(10, 4, wait=True); got = [b._draw_noise(10, 4), b._draw_noise(10, 4), b._draw_noise(7, 4)]
    assert all(np.array_equal(x, y) for x, y in zip(want, got))
    c = mk(); c.prefetch_noise(9, 4); assert np.array_equal(c._draw_noise(10, 4), want[0])          # wrong shape prefetched: discarded, state restored


def test_context_is_not_destroyed_by_a_forked_child():
    """A multiprocessing worker inherits the parent's Context objects; when its garbage collector finalises the copies, lmpc_destroy must NOT run there (HIP calls in a
    forked child: a segmentation fault in the worker and a parent waiting for ever -- it happened in the oracle pools of the GPU tests, round 6).  No GPU needed: the
    object is built around a recording stand-in for the library."""
    import ctypes as C
    import os
    from racinglmpc_amd import _capi

    class _Lib:
        def __init__(self):
            self.destroyed = 0

        def lmpc_destroy(self, h):
            self.destroyed += 1

    ctx = _capi.Context.__new__(_capi.Context)
    ctx.lib = _Lib(); ctx._h = C.c_void_p(1234); ctx._pid = os.getpid()
    r, w = os.pipe()
    pid = os.fork()
    if pid == 0:                                       # the child: finalise the inherited copy, report how often the library was called
        os.close(r)
        ctx.close()
        os.write(w, b"%d" % ctx.lib.destroyed)
        os._exit(0)
    os.close(w)
    got = os.read(r, 16); os.waitpid(pid, 0); os.close(r)
    assert got == b"0"
    assert ctx._h.value == 1234 and ctx.lib.destroyed == 0     # the parent's handle is untouched ...
    ctx.close()
    assert ctx.lib.destroyed == 1 and not ctx._h              # ... and the parent destroys it once


def test_context_pool_releases_its_members_when_one_fails(monkeypatch):
    """ContextPool: a member that fails to come up closes the ones before it and the error is the member's own (not a recursion through the pool's attribute hook);
    `with` closes every member.  No GPU needed: Context is replaced by a recording stand-in."""
    import pytest
    from racinglmpc_amd import _capi
    made = []

    class _Ctx:
        def __init__(self, cfg):
            if len(made) == 2:
                raise _capi.LmpcError("no device memory")
            self.closed = 0; self.calls = []; made.append(self)

        def close(self):
            self.closed += 1

        def ss_add_point(self, *a):
            self.calls.append(a); return len(self.calls)

        def ss_num_laps(self):
            return 7

    monkeypatch.setattr(_capi, "Context", _Ctx)
    with pytest.raises(_capi.LmpcError, match="no device memory"):
        _capi.ContextPool(None, depth=3)
    assert [m.closed for m in made] == [1, 1]
    with pytest.raises(ValueError):
        _capi.ContextPool(None, depth=0)
    del made[:]
    with _capi.ContextPool(None, depth=2) as pool:
        assert pool.ss_add_point(1.0, 2.0) == 1 and [m.calls for m in made] == [[(1.0, 2.0)]] * 2      # store edits reach every member
        assert pool.ss_num_laps() == 7                                                                    # queries go to the first
    assert [m.closed for m in made] == [1, 1]


def test_context_pool_restores_every_member(monkeypatch):
    """ContextPool.restore_stores reaches every member, not only the first (a member with empty stores answers nothing: step_batch_dev deals steps to it
    in turn).  No GPU needed: Context is replaced by a recording stand-in."""
    from racinglmpc_amd import _capi
    made = []

    class _Ctx:
        def __init__(self, cfg):
            self.restored = []; made.append(self)

        def restore_stores(self, path):
            self.restored.append(path)

        def close(self):
            pass

    monkeypatch.setattr(_capi, "Context", _Ctx)
    with _capi.ContextPool(None, depth=3) as pool:
        pool.restore_stores("laps.npz")
    assert [m.restored for m in made] == [["laps.npz"]] * 3


def test_save_and_restore_stores_take_the_same_path(tmp_path):
    """Context.save_stores / restore_stores: np.savez_compressed appends .npz to a path without it, so restore_stores with the SAME string must find that
    file.  No GPU needed: the real methods run around a stand-in library whose lap stores are empty."""
    import ctypes as C
    import os
    from racinglmpc_amd import _capi

    class _Lib:
        def lmpc_model_num_laps(self, h, n):
            n._obj.value = 0; return 0

        def lmpc_ss_num_laps(self, h, n):
            n._obj.value = 0; return 0

    ctx = _capi.Context.__new__(_capi.Context)
    ctx.lib = _Lib(); ctx._h = C.c_void_p(); ctx._pid = os.getpid(); ctx.N = 12
    base = str(tmp_path / "stores")
    ctx.save_stores(base)
    assert sorted(os.listdir(str(tmp_path))) == ["stores.npz"]
    ctx.restore_stores(base)
    ctx.restore_stores(base + ".npz")
    ctx.save_stores(base + ".npz")                     # (a path with the extension is taken as it is)
    assert sorted(os.listdir(str(tmp_path))) == ["stores.npz"]


# ---- the per-problem array table: racinglmpc_amd/csrc/lmpc_arrays.h and racinglmpc_amd._capi.ARRAYS

_LAYOUT_PROGRAM = r"""
#include "lmpc_arrays.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {                      /* N S numSS_it B */
    if (argc != 5) return 2;
    const lmpc_dims d = {(size_t)atol(argv[1]), (size_t)atol(argv[2]), (size_t)atol(argv[3])};
    size_t total[2];
    lmpc_slab_layout(d, (size_t)atol(argv[4]), 0, total, [](const char *name, auto, int slab, size_t offset, size_t bytes) {
        printf("%s %d %zu %zu\n", name, slab, offset, bytes); });
    printf("total %zu %zu\n", total[0], total[1]);
    return 0;
}
"""


def _slab_rule(N, S, L, B):
    """The work-buffer layout as lmpc_create has always made it, restated: this order, max(n, 1) elements per range, every range rounded up to 256 bytes,
    the inputs in one slab and everything else in the other.  Returns ([(name, slab, offset, bytes)], [bytes of slab 0, bytes of slab 1])."""
    M = 8 * N + S
    rows = [("x0", 0, 8, B * 6), ("xLin", 0, 8, B * (N + 1) * 6), ("uLin", 0, 8, B * N * 2), ("uOld", 0, 8, B * 2), ("zt", 0, 8, B * 6),
            ("xPredPrev", 0, 8, B * (N + 1) * 6), ("hasPred", 0, 4, B), ("timeStep", 0, 4, B),
            ("xPred", 1, 8, B * (N + 1) * 6), ("uPred", 1, 8, B * N * 2), ("slack", 1, 8, B * N * 2), ("lambda", 1, 8, B * S), ("sTerm", 1, 8, B * 6),
            ("ztNext", 1, 8, B * 6), ("ztuNext", 1, 8, B * 2), ("ssSel", 1, 8, B * S * 6), ("qSel", 1, 8, B * S), ("mu", 1, 8, B * M),
            ("A", 1, 8, B * N * 36), ("Bm", 1, 8, B * N * 12), ("C", 1, 8, B * N * 6), ("status", 1, 4, B), ("iters", 1, 4, B), ("resid", 1, 8, B * 3),
            ("succ", 1, 8, B * S * 6), ("succU", 1, 8, B * S * 2), ("ztUsed", 1, 8, B * 6), ("rstatus", 1, 4, B * N), ("selStart", 1, 4, B * max(L, 1))]
    slab = np.array([r[1] for r in rows]); item = np.array([r[2] for r in rows], np.int64); n = np.array([r[3] for r in rows], np.int64)
    nbytes = (np.maximum(n, 1) * item + 255) // 256 * 256
    offset = np.zeros(len(rows), np.int64)
    for s in (0, 1):
        offset[slab == s] = np.cumsum(nbytes[slab == s]) - nbytes[slab == s]
    return [(r[0], int(s), int(o), int(b)) for r, s, o, b in zip(rows, slab, offset, nbytes)], [int(nbytes[slab == s].sum()) for s in (0, 1)]


_LAYOUT_BIN = {}


def _layout_program(tmp_path_factory):
    """The program above, compiled once with plain g++ against the header alone (no HIP header on the include path)."""
    import os
    import subprocess
    if "exe" not in _LAYOUT_BIN:
        d = tmp_path_factory.mktemp("slab_layout")
        src = d / "layout.cpp"; src.write_text(_LAYOUT_PROGRAM)
        exe = str(d / "layout")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(common.ROOT, "racinglmpc_amd", "csrc"), str(src), "-o", exe],
                       check=True, capture_output=True, timeout=120)
        _LAYOUT_BIN["exe"] = exe
    return _LAYOUT_BIN["exe"]


@pytest.mark.parametrize("N,S,L,B", [(12, 48, 4, 1), (12, 0, 0, 1), (40, 48, 4, 3), (2, 1, 1, 1), (14, 48, 4, 16)])
def test_slab_layout_of_the_array_table(tmp_path_factory, N, S, L, B):
    """lmpc_arrays.h lays the context's two slabs out exactly as the hand-written list did: names, order, slab, offsets and sizes ((12, 0, 0, 1): every
    S-sized range at its one-element floor; (2, 1, 1, 1): the smallest legal configuration)."""
    import subprocess
    out = subprocess.run([_layout_program(tmp_path_factory)] + [str(v) for v in (N, S, L, B)], check=True, capture_output=True, timeout=30).stdout.decode().split("\n")
    got = [(f[0], int(f[1]), int(f[2]), int(f[3])) for f in (l.split() for l in out if l and not l.startswith("total"))]
    total = [int(v) for v in [l for l in out if l.startswith("total")][0].split()[1:]]
    want, want_total = _slab_rule(N, S, L, B)
    assert got == want
    assert total == want_total
    assert all(o % 256 == 0 and b % 256 == 0 and b >= 256 for _, _, o, b in got)


class _ShapeLib:
    """Stand-in library: every entry point the shape test reaches succeeds and touches nothing."""

    def __getattr__(self, name):
        return lambda *a: 0


@pytest.mark.parametrize("B,N,S,L", [(3, 12, 48, 4), (2, 12, 0, 0)])
def test_python_array_table_gives_the_shapes_the_entry_points_return(B, N, S, L):
    """racinglmpc_amd._capi.ARRAYS against the shapes and dtypes step_batch, step_dev_fetch, qp_solve_batch and select_batch have always returned, written out;
    the entry points themselves (run around a stand-in library) return exactly these, step_batch from one float64 and one int32 buffer and a plan cached per B."""
    import ctypes as C
    import os
    import types
    from racinglmpc_amd import _capi
    f8, i4 = np.float64, np.int32
    M = 8 * N + S
    step = dict(xPred=((B, N + 1, 6), f8), uPred=((B, N, 2), f8), slack=((B, 2 * N), f8), lambd=((B, S), f8), sTerm=((B, 6), f8), ztNext=((B, 6), f8),
                ztuNext=((B, 2), f8), ssSel=((B, S, 6), f8), qSel=((B, S), f8), mu=((B, M), f8), A=((B, N, 6, 6), f8), B=((B, N, 6, 2), f8), C=((B, N, 6), f8),
                status=((B,), i4), iters=((B,), i4), resid=((B, 3), f8))
    qp = {k: step[k] for k in ("xPred", "uPred", "slack", "lambd", "sTerm", "mu", "status", "iters", "resid")}
    sel = dict(ssSel=((B, S, 6), f8), qSel=((B, S), f8), succ=((B, S, 6), f8), succU=((B, S, 2), f8), ztUsed=((B, 6), f8), selStart=((B, max(L, 1)), i4),
               status=((B,), i4))
    if (B, N, S, L) == (3, 12, 48, 4):                  # (the same, as plain numbers)
        assert step["xPred"][0] == (3, 13, 6) and step["slack"][0] == (3, 24) and step["mu"][0] == (3, 144) and step["ssSel"][0] == (3, 48, 6) and sel["selStart"][0] == (3, 4)
    else:
        assert step["lambd"][0] == (2, 0) and step["mu"][0] == (2, 96) and step["ssSel"][0] == (2, 0, 6) and sel["succU"][0] == (2, 0, 2) and sel["selStart"][0] == (2, 1)

    def same(spec, want):
        return set(spec) == set(want) and all(tuple(spec[k][0]) == want[k][0] and np.dtype(spec[k][1]) == np.dtype(want[k][1]) for k in want)
    assert same(_capi.array_specs(B, N, S, L, _capi.STEP_OUT_KEYS), step)
    assert same(_capi.array_specs(B, N, S, L, _capi.QP_OUT_KEYS), qp)
    assert same(_capi.array_specs(B, N, S, L, _capi.SELECT_OUT_KEYS), sel)
    inputs = _capi.array_specs(B, N, S, L, _capi.STEP_IN_KEYS)
    assert same(inputs, dict(x0=((B, 6), f8), xLin=((B, N + 1, 6), f8), uLin=((B, N, 2), f8), uOld=((B, 2), f8), zt=((B, 6), f8),
                             xPredPrev=((B, N + 1, 6), f8), hasPred=((B,), i4), timeStep=((B,), i4)))

    ctx = _capi.Context.__new__(_capi.Context)
    ctx.lib = _ShapeLib(); ctx._h = C.c_void_p(); ctx._pid = os.getpid()
    ctx.cfg = types.SimpleNamespace(numSS_it=L, numSS_points=S, N=N); ctx.N, ctx.S, ctx.M, ctx._step_plan = N, S, M, {}
    arrs = lambda out: {k: (v.shape, v.dtype) for k, v in out.items()}
    out = ctx.step_batch(np.zeros((B, 6)), np.zeros((B, N + 1, 6)), np.zeros((B, N, 2)), np.zeros((B, 2)), zt=np.zeros((B, 6)))
    assert same(arrs(out), step)
    bases = {id(v.base) for k, v in out.items() if v.dtype == f8}
    assert len(bases) == 1 and out["status"].base is out["iters"].base and out["status"].base is not None
    plan = ctx._step_plan[B]
    ctx.step_batch(np.zeros((B, 6)), np.zeros((B, N + 1, 6)), np.zeros((B, N, 2)), np.zeros((B, 2)))
    assert list(ctx._step_plan) == [B] and ctx._step_plan[B] is plan
    assert same(arrs(ctx.step_dev_fetch(_capi.StepDevArgs(), B)), step)
    assert same(arrs(ctx.qp_solve_batch(np.zeros((B, N, 6, 6)), np.zeros((B, N, 6, 2)), np.zeros((B, N, 6)), np.zeros((B, 6)), np.zeros((B, 2)))), qp)
    assert same(arrs(ctx.select_batch(np.zeros((B, 6)), np.zeros((B, 6)))), sel)


def test_step_dev_args_mirrors_the_c_struct():
    """StepDevArgs._fields_, in order, are the members of lmpc_step_dev_args as include/lmpc_hip.h declares them (`lambda` is spelt lambda_ in Python), all pointers."""
    import ctypes as C
    import os
    import re
    from racinglmpc_amd import _capi
    text = open(os.path.join(common.ROOT, "include", "lmpc_hip.h")).read()
    end = text.index("} lmpc_step_dev_args;")
    body = re.sub(r"/\*.*?\*/", "", text[text.rindex("typedef struct {", 0, end) + len("typedef struct {"):end], flags=re.S)
    members = re.findall(r"\*\s*(\w+)", body)
    assert len(members) == 24 and members[0] == "x0" and members[-1] == "qSel"
    assert [n for n, _ in _capi.StepDevArgs._fields_] == ["lambda_" if m == "lambda" else m for m in members]
    assert all(t is C.c_void_p for _, t in _capi.StepDevArgs._fields_)
