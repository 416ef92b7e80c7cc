"""No GPU: the reference side of tests/test_gpu_envelope.py stands on its own, and the case table covers the edges it is there for.

  * every case of tests/envelope_cases.CASES: the oracle selects on every compared problem without raising (every window inside its lap), the selection has
    numSS_it x points-per-lap columns, and osqp_solve_exact certifies below 1e-8 on all but at most one in eight of them;
  * the table has at least one case on each side of every edge at which the solve code changes shape (envelope_cases.EDGES), every fixed-variant case is
    prepared by build() (racinglmpc_amd.build.EXTRA_VARIANTS or built in), and the runtime-only cases are not;
  * oracle_pool.select_laps is the reference's own selection for every even number of points per lap, and for an odd one the first points-per-lap columns of the
    same window."""
import numpy as np
import pytest

from tests import envelope_cases as ec


@pytest.mark.parametrize("c", ec.CASES, ids=[ec.case_id(c) for c in ec.CASES])
def test_the_oracle_certifies_every_case(c):
    res = ec.oracle_records(c)
    rows = ec.compared_rows(c)
    assert [r["b"] for r in res] == rows and len(rows) == (8 if (c.N >= 41 or ec.S_of(c) >= 378) else 16)
    S, N = ec.S_of(c), c.N
    for r in res:
        assert np.isfinite(r["A"]).all() and np.isfinite(r["B"]).all() and np.isfinite(r["C"]).all()
        if c.L:
            assert r["SSsel"].shape == (6, S) and r["Qsel"].shape == (S,) and r["Succ"].shape == (6, S) and r["SuccU"].shape == (2, S), r["b"]
            assert np.array_equal(r["SSsel"][:, 1:c.ppl], r["Succ"][:, :c.ppl - 1])                 # the successor of column j of a lap is its column j + 1
    certs = [max(r["cert"], r.get("cert2", 0.0)) for r in res]
    keep, left_out = ec.certified(res)
    print("%s: %d problems, worst certificate %.1e, %d left out" % (ec.case_id(c), len(res), max(certs), left_out))
    assert left_out == 0          # (the recorded run leaves none out: a certificate that gets worse shows here before the one-in-eight allowance is used up)


def test_the_table_has_both_sides_of_every_edge():
    from racinglmpc_amd import build
    for name, pred in ec.EDGES.items():
        sides = {bool(pred(c)) for c in ec.CASES}
        assert sides == {True, False}, name
    prepared = set(build.BUILTIN) | set(build.EXTRA_VARIANTS)
    for c in ec.CASES:
        assert 2 <= c.N <= 64 and c.L <= 32 and ec.S_of(c) <= 384 and c.ppl <= 63
        assert ((c.N, ec.S_of(c)) in prepared) == c.variant, ec.case_id(c)
        names = [r[0] for r in ec.routes(c)]
        assert len(names) == len(set(names)) and names, ec.case_id(c)
        assert ("runtime kernel" in names) == ((c.N, ec.S_of(c)) not in ec.RT_REFUSED)
    # the classes the issue names: both sides of use_abg, a four-waves-throughout case, cases without multi-wave kernels, a two-wave regime and none
    assert {c.abg for c in ec.CASES if c.variant} == {True, False}
    assert {c.mw for c in ec.CASES if c.variant} == {"full", "throughout", "none"}
    assert {c.two for c in ec.CASES if c.variant and c.mw == "full"} == {True, False}


@pytest.mark.parametrize("ppl", [12, 29, 63])
def test_select_laps_is_the_reference_selection_cut_to_the_points_per_lap(ppl):
    from oracle import lmpc_oracle as orc
    from tests import oracle_pool
    g = ec.golden()
    L, N = 3, 12
    laps = ec.ss_laps(L)
    xS = [x for x, u in laps]; uS = [u for x, u in laps]
    Qf = [orc.compute_cost(x, g["TL"]) for x in xS]
    P = ec.problems(N)
    for b in (0, 1, 17, 40):                     # (b = 0: the window starts at row 0 of the lap or near it -- the branch without a centred window)
        z = P["zt"][b].copy() if b else xS[0][3].copy()
        got = oracle_pool.select_laps(xS, uS, Qf, z, ppl, None, L, 5, N, g["TL"])
        assert got[0].shape == (6, L * ppl) and got[1].shape == (L * ppl,) and got[2].shape == (6, L * ppl) and got[3].shape == (2, L * ppl)
        ref = orc.terminal_components(xS, uS, Qf, [x.shape[0] for x in xS], z, ppl * L, L, None, L, 5, N, g["TL"])
        w = ref[0].shape[1] // L                  # the reference's columns per lap: ppl, or ppl + 1 where ppl is odd and the window is centred
        assert w in (ppl, ppl + 1) and (ppl % 2 == 1 or w == ppl)
        for l in range(L):
            for a, r in zip(got, ref):
                assert np.array_equal(a[..., l * ppl:(l + 1) * ppl], r[..., l * w:l * w + ppl]), (ppl, b, l)
