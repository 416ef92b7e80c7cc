"""The corners of the supported range: one table of (N, numSS_it, points per lap) cases for tests/test_gpu_envelope.py and tests/test_envelope_host.py.

lmpc_create_ex takes 2 <= N <= 64, numSS_it <= 32, numSS_points <= 384 and at most 63 points per lap; the solve code changes shape at exactly these edges (EDGES
below states each as a predicate, tests/test_envelope_host.py checks that the table has a case on either side of every one).  A case says which solve kernels serve
it -- `variant`: a fixed (N, S) instantiation prepared by racinglmpc_amd.build.EXTRA_VARIANTS, else the runtime-(N, S) kernel only -- and, for a fixed one, which
class of the route rules of lmpc_capi.hip (create_body) it is in:
    abg       [A_k | B_k] in global memory for batches beyond the QPs that fit the CUs with it in LDS (lmpc_variant.hip.h: use_abg)
    mw        "full": four waves per QP up to one QP per CU, then two where `two` says so, then one;  "throughout": four waves per QP at every batch size (two QPs
              of the one-wave layout do not fit a CU);  "none": the multi-wave layout exceeds the LDS of a CU, one wave per QP at every batch size
    two       the two-wave regime reaches beyond one QP per CU (mw2_max_batch > n_cu)
    fit       abg cases: QPs per CU of the one-wave layout with [A_k | B_k] in LDS (160 KB / lds_1w); a batch of up to fit x n_cu keeps it there (launch_solve)
These classes are stated here from the layouts (solve_lds / solve_lds1) and ASSERTED against what the library reports (Context.solver_waves, solver_kind,
solver_lds): a case that silently moves to another route fails.

Problems: bench.synth_batch on the recorded PID lap, 64 problems P (seed 1234) in rows 0 .. 63 of every batch, problems of another seed behind them.
Stores: the recorded PID lap four times as regression store (plain MPC: once); numSS_it DISTINCT laps as safe set -- the PID lap's 1000 rows (three times round the
track, s unwrapped, so that every zt of P has its window inside every lap) moved by a per-lap offset and a per-row jitter, lap i of L cut to 1000 - (L - 1 - i) rows so that
no two lap times tie.  (Identical laps would make lambda, hence zt, non-unique.)"""
import collections
import functools

import numpy as np

from tests import common

P_SIZE = 64
SEED_P, SEED_FILL = 1234, 4321
N_CU = 256                      # MI355X; the GPU tests take the CU count of their device (Context.solver_lds()["n_cu"]) instead
LDS_CU = 160 * 1024

Case = collections.namedtuple("Case", "N L ppl variant abg mw two fit why")


def _c(N, L, ppl, why, variant=False, abg=False, mw="full", two=False, fit=0):
    return Case(N, L, ppl, variant, abg, mw if variant else "none", two, fit, why)


CASES = [
    _c(2, 4, 12, "16-slot sweep dump (8 N < 64); a horizon shorter than the four-wave pipeline has waves; t1 scratch with PSTW == CW", variant=True, two=True),
    _c(3, 4, 12, "16-slot sweep dump, odd horizon"),
    _c(7, 4, 12, "last horizon of the 16-slot sweep dump", variant=True, two=True),
    _c(2, 0, 0, "plain MPC at the shortest horizon", variant=True, two=True),
    _c(12, 2, 29, "58 points: the terminal block fills the wave exactly (CH = 1)"),
    _c(12, 1, 59, "59 points from one lap: one column in a second pass (CH = 2)", variant=True, two=True),
    _c(12, 6, 63, "378 points, 63 per lap (the most): six passes exactly full (CH = 6)"),
    _c(12, 32, 12, "384 points from 32 laps: a seventh pass with 6 live columns, the lap table of the kernels filled to its last entry", variant=True),
    _c(2, 32, 12, "the widest safe set on the shortest horizon"),
    _c(63, 4, 12, "[A|B] stays in LDS (use_abg off); 64 predicted rows: one pass of the crossing count", variant=True),
    _c(64, 4, 12, "use_abg on; 65 predicted rows: second pass of the crossing count with one live lane; every lane reads a regression status", variant=True, abg=True, fit=1),
    _c(64, 0, 0, "use_abg on without a terminal set; two QPs per CU keep [A|B] in LDS", variant=True, abg=True, fit=2),
    _c(64, 1, 12, "use_abg off at the longest horizon (12 points)"),
    _c(32, 32, 12, "two QPs of the one-wave layout do not fit a CU: four waves per QP at every batch size", variant=True, mw="throughout"),
    _c(40, 32, 12, "no multi-wave kernels and no runtime kernel at a horizon of the reference; the build takes the combined code-generation option (build.VARIANT_SALTS)", variant=True, mw="none"),
    _c(64, 16, 12, "the multi-wave layout (and the runtime kernel's) exceeds the LDS of a CU, the one-wave layout fits: one wave per QP at every batch size", variant=True, mw="none"),
    _c(64, 32, 12, "the far corner: no multi-wave kernels, no runtime kernel (its layout exceeds the LDS of a CU)", variant=True, mw="none"),
]
# the runtime kernel's layout (rt_layout: nothing shared between phases) exceeds the LDS of a CU and lmpc_create_ex refuses it: N = 64 beyond 146 points (168 KB at
# 192, 209 KB at 384), N = 40 beyond 366; only a fixed variant serves these
RT_REFUSED = {(64, 192), (64, 384), (40, 384)}

# every edge of "Why" as a predicate on a case: the table has cases on both sides
EDGES = {
    "8 N < 64 (16-slot sweep dump)": lambda c: 8 * c.N < 64,
    "S + 6 <= 64 (one terminal-block column per lane)": lambda c: 0 < c.L * c.ppl and c.L * c.ppl + 6 <= 64,
    "S + 6 a multiple of 64 (last pass exactly full)": lambda c: c.L > 0 and (c.L * c.ppl + 6) % 64 == 0,
    "S + 6 > 6 x 64 (seventh pass)": lambda c: c.L * c.ppl + 6 > 384,
    "N == 64": lambda c: c.N == 64,
    "63 points per lap": lambda c: c.ppl == 63,
    "numSS_it == 32": lambda c: c.L == 32,
    "no terminal set": lambda c: c.L == 0,
}


def S_of(c):
    return c.L * c.ppl


def case_id(c):
    return "N%d_L%d_ppl%d" % (c.N, c.L, c.ppl)


def compared_rows(c):
    """The problems of P compared with the oracle: 8 where N >= 41 or S >= 378, 16 otherwise."""
    return list(range(0, P_SIZE, 8 if (c.N >= 41 or S_of(c) >= 378) else 4))


def routes(c, n_cu=N_CU):
    """(name, batch, waves per QP, knobs, runtime kernel) of every route production takes for the case on a device of n_cu CUs, as tests/test_gpu_routes._routes
    derives them: P always in rows 0 .. 63.  Batches (at 256 CUs): 96 is below one QP per CU; n_cu + 44 (300) lies between one QP per CU and the end of every
    two-wave regime that exists (2 n_cu at the least); the one-wave batch is beyond the case's last multi-wave batch -- 4 n_cu + 76 (1100), 2 n_cu + 88 (600) with
    several terminal-block columns per lane, n_cu + 44 without a two-wave regime; use_abg: fit x n_cu + 44, beyond the QPs that fit the CUs with [A|B] in LDS."""
    assert n_cu >= 96, "the batch of 96 (P and 32 problems behind it) is meant to lie below one QP per CU"
    S = S_of(c)
    mid = n_cu + 44
    r = []
    if c.variant:
        if c.mw == "full":
            r.append(("4 waves", 96, 4, {}, False))
            if c.two:
                r.append(("2 waves", mid, 2, {}, False))
            one = 4 * n_cu + 76 if (c.two and S + 6 <= 64) else 2 * n_cu + 88 if c.two else mid
            if c.abg:
                one = c.fit * n_cu + 44
                if c.fit > 1:
                    r.append(("1 wave, [A|B] in LDS", mid, 1, {}, False))
                r += [("1 wave, [A|B] global", one, 1, {}, False), ("1 wave, [A|B] in LDS (LMPC_NO_ABG)", one, 1, {"LMPC_NO_ABG": "1"}, False)]
            else:
                r.append(("1 wave", one, 1, {}, False))
        elif c.mw == "throughout":
            r += [("4 waves", 96, 4, {}, False), ("4 waves, more than one QP per CU", mid, 4, {}, False)]
        else:
            r += [("1 wave, batch 96", 96, 1, {}, False), ("1 wave", mid, 1, {}, False)]
    if (c.N, S) not in RT_REFUSED:
        r.append(("runtime kernel", 96, 1, {}, True))
    return r


@functools.lru_cache(maxsize=None)
def golden():
    g = common.load_lmpc_golden()
    return dict(track=np.array(g["track"]), TL=float(g["trackLength"]), xPID=np.array(g["xPID"]), uPID=np.array(g["uPID"]), trackLength=g["trackLength"])


@functools.lru_cache(maxsize=None)
def ss_laps(L):
    """L distinct safe-set laps in the library's order (fastest first: lap i has 1000 - (L - 1 - i) rows)."""
    g = golden()
    laps = []
    for i in range(L):
        rng = np.random.default_rng(500 + i)
        T = 1000 - (L - 1 - i)
        x = g["xPID"][:T] + rng.normal(size=(1, 6)) * np.array([.02, .01, .02, .01, .02, .02]) + rng.normal(size=(T, 6)) * 1e-3
        u = g["uPID"][:T] + rng.normal(size=(T, 2)) * 1e-3
        laps.append((x, u))
    return laps


@functools.lru_cache(maxsize=None)
def problems(N, B=P_SIZE):
    """P in rows 0 .. 63, rows 64 .. B - 1 from the other seed."""
    import bench
    g = golden()
    P = bench.synth_batch(g, P_SIZE, N, seed=SEED_P)
    if B == P_SIZE:
        return P
    F = bench.synth_batch(g, B, N, seed=SEED_FILL)
    return {k: np.concatenate([P[k], F[k][P_SIZE:B]]) for k in P}


def params(c):
    from oracle import lmpc_oracle as orc
    if c.L == 0:
        return orc.QPParams.mpc_default(c.N, 0.8)
    par = orc.QPParams.lmpc_default(c.N)
    par.numSS_Points, par.numSS_it = S_of(c), c.L
    return par


@functools.lru_cache(maxsize=None)
def oracle_records(c, solve=True):
    """Oracle records of the compared problems of P (computed once per case and shared; nobody writes to them): tests/oracle_pool.oracle_batch with the case's points
    per lap, plain MPC: tests/test_gpu_routes._mpc_oracle."""
    g = golden()
    rows = compared_rows(c)
    P = problems(c.N)
    if c.L == 0:
        from tests.test_gpu_routes import _mpc_oracle
        return _mpc_oracle(g, params(c), c.N, P, rows=rows)
    from tests import oracle_pool
    pid = (g["xPID"], g["uPID"])
    return oracle_pool.oracle_batch(params(c), g["track"], g["TL"], [pid] * 4, c.N, P, rows, solve_idx=rows if solve else (), ss_laps=ss_laps(c.L), ppl=c.ppl)


def certified(res):
    """(records for the comparison, number left out of the (x, u) comparison): a record whose oracle certificate is not below 1e-8 keeps A, B, C and the selection only.
    At most one in eight may be left out, never all."""
    keep, out = [], 0
    for r in res:
        if "opt" in r and not max(r["cert"], r.get("cert2", 0.0)) < 1e-8:
            r = {k: v for k, v in r.items() if k not in ("opt", "opt2", "cert", "cert2", "obj", "objf")}
            out += 1
        keep.append(r)
    assert out <= len(res) // 8 and out < len(res), "%d of %d oracle records are not certified below 1e-8" % (out, len(res))
    return keep, out


def config(c, B, **kw):
    g = golden()
    if c.L == 0:
        return common.mpc_config(g, c.N, max_batch=B, **kw)[0]
    return common.lmpc_config(g, c.N, max_batch=B, numSS_it=c.L, numSS_Points=S_of(c), trToUse=4, max_laps=max(40, c.L + 4), max_lap_len=1024, **kw)[0]


def context(c, B, knobs=None, runtime_kernel=False):
    """A context of the case on the route that (B, knobs, runtime_kernel) select, stores filled.  The knobs are set around Context() only."""
    from racinglmpc_amd import _capi
    from tests.test_gpu_routes import _knobs
    g = golden()
    with _knobs(knobs or {}):
        ctx = _capi.Context(config(c, B), runtime_kernel=runtime_kernel)
    for _ in range(4 if c.L else 1):
        ctx.model_add_trajectory(g["xPID"], g["uPID"])
    for x, u in ss_laps(c.L):
        ctx.ss_add_trajectory(x, u)
    return ctx
