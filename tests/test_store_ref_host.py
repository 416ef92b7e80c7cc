"""CPU: tests/store_ref.py, the host restatement the GPU tests compare the lap stores with, checked on laps whose answers are known by construction."""
import numpy as np

from tests import k1_cases, store_ref


def _words(q):
    """(rows, 5) 16-bit words out of the three packed planes."""
    return np.stack([q[0] & 0xffff, q[0] >> 16, q[1] & 0xffff, q[1] >> 16, q[2] & 0xffff], 1).astype(np.int64)


def test_image_of_the_lap_whose_scale_is_exactly_one():
    """tests/k1_cases.slack_case: every feature range is [0, 65535], so lo = +0.0, sc = 1 exactly and every word is the feature truncated."""
    case = k1_cases.slack_case()
    x, u = case["x"], case["u"]
    q, par, chunks = store_ref.prefilter_image(x, u, np.ones(5))
    assert chunks == 1 and q.shape == (3, x.shape[0] - 1) and q.dtype == np.uint32 and par.shape == (1, 6)
    assert np.array_equal(par.view(np.int64), np.array([[0.0] * 5 + [1.0]]).view(np.int64))
    F = np.hstack([x[:-1, 0:3], u[:-1]])
    assert np.array_equal(_words(q), np.floor(F).astype(np.int64))
    assert not (q[2] >> 16).any()
    # the same words as the emulation the prefilter tests rank rows with
    tq = np.hstack([case["xq"][0:3], case["uq"]]).astype(np.int64)
    assert np.array_equal(np.abs(_words(q) - tq[None]).sum(1), k1_cases.emulate_prefilter(case)["e"])


def test_image_edges():
    """Among equal minima the first one met stays (the sign of a zero minimum); a feature without a finite value; the 1e-9 and 1e-300 floors; chunks of 1024 rows."""
    T = 1030
    x = np.ones((T, 6)); u = np.ones((T, 2))
    x[:, 0] = np.linspace(1.0, 3.0, T)
    x[3, 1], x[4, 1] = 0.0, -0.0
    x[7, 2], x[6, 2] = 0.0, -0.0
    u[:1024, 0] = np.nan
    u[1024:, 0] = np.inf
    q, par, chunks = store_ref.prefilter_image(x, u, [0.5, 1, 1, 1, 1])
    assert chunks == 2 and q.shape == (3, T - 1)
    assert not np.signbit(par[0, 1]) and np.signbit(par[0, 2]) and par[0, 1] == par[0, 2] == 0.0
    assert par[0, 3] == 0.0 and par[1, 3] == 0.0 and not (q[1] >> 16).any()                     # (no finite delta anywhere: lo = 0, words 0)
    assert par[0, 0] == 0.5 and par[1, 0] == x[1024, 0] * 0.5 and par[1, 1] == 1.0               # every chunk has its own minima
    assert par[0, 5] == 65535.0 / 1.0                                                            # widest range of chunk 0: vy and wz, 0 .. 1
    assert par[1, 5] == 65535.0 / (x[1028, 0] * 0.5 - x[1024, 0] * 0.5)                          # chunk 1 holds rows 1024 .. 1028
    x = np.tile(np.array([1.5, -2.0, 0.25, 0, 0, 0]), (9, 1)); u = np.tile(np.array([0.1, 3.0]), (9, 1))
    q, par, chunks = store_ref.prefilter_image(x, u, np.ones(5))
    assert chunks == 1 and par[0, 5] == 65535.0 / (1e-9 * 3.0) and not q.any()                   # constant features: the range floor
    q, par, chunks = store_ref.prefilter_image(np.zeros((2, 6)), np.zeros((2, 2)), np.ones(5))
    assert q.shape == (3, 1) and par[0, 5] == 65535.0 / 1e-300 and not q.any()
    x[4, 0] = 1e300
    q, par, chunks = store_ref.prefilter_image(x, u, np.ones(5))
    assert _words(q)[4, 0] in (65534, 65535) and _words(q)[3, 0] == 0 and par[0, 5] == 65535.0 / (1e300 - 1.5)      # (range * (65535 / range) may round below 65535)


def test_cost_countdown_and_order():
    from oracle import lmpc_oracle as orc
    TL = 10.0
    x = np.zeros((700, 6)); x[:, 4] = np.linspace(0.0, 9.9, 700)
    x[[255, 256, 699], 4] = 10.0; x[100, 4] = np.nan
    cost = store_ref.compute_cost(x, TL)
    assert np.array_equal(cost, orc.compute_cost(x, TL))
    assert cost[699] == 0 and cost[698] == 1 and cost[257] == 699 - 257 and cost[256] == 0 and cost[255] == 0 and cost[254] == 1 and cost[100] == 0 and cost[99] == 1 and cost[0] == 100
    assert np.array_equal(store_ref.compute_cost(np.zeros((1, 6)), TL), [0.0])
    xe, ue, qe = store_ref.extend_rows(np.arange(18.0).reshape(3, 6), np.ones((3, 2)), 1.0 / 3.0, TL)
    assert np.array_equal(xe[:, 4], [14.0, 20.0, 26.0]) and xe[0, 3] == 3.0
    assert qe[0] == 1.0 / 3.0 - 1.0 and qe[2] == ((1.0 / 3.0 - 1.0) - 1.0) - 1.0 and qe[2] != 1.0 / 3.0 - 3.0
    assert store_ref.sorted_order([300, 1024, 2, 300, 2, 5000, 300]) == [2, 4, 0, 3, 6, 1, 5]


def test_ref_stores_snapshot():
    ref = store_ref.RefStores(10.0, [0.1, 1, 1, 1, 1])
    rng = np.random.default_rng(0)
    laps = [(rng.standard_normal((T, 6)), rng.standard_normal((T, 2))) for T in (5, 3, 5)]
    for x, u in laps:
        ref.ss_add_trajectory(x, u); ref.model_add_trajectory(x, u)
    ref.ss_replace_lap(1, laps[0][0], laps[0][1], np.arange(4, -1, -1.0) + 0.5)
    ref.ss_extend_lap(1, laps[1][0], laps[1][1])
    ref.ss_add_point(laps[1][0][0], laps[1][1][0])
    ref.model_replace_lap(2, laps[0][0], laps[0][1])              # sorted position 2 = insertion index 2
    s = ref.snapshot()
    assert s["info"] == [(5, 1), (3, 0), (5, 2)] and [m[0].shape[0] for m in s["model"]] == [3, 5, 5]
    assert np.array_equal(s["model"][2][0], laps[0][0]) and s["image"][2][0].shape == (3, 4)
    assert s["ss"][1][3:] == (3, 8) and np.array_equal(s["ss"][1][2], [4.5, 3.5, 2.5, 1.5, 0.5, -0.5, -1.5, -2.5])
    assert s["ss"][2][3:] == (5, 6) and s["ss"][2][0][5, 4] == laps[1][0][0, 4] + 10.0 and s["ss"][2][2][5] == -1.0
