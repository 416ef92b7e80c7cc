"""-m gpu: laps handed in from the host (model_add_trajectory, ss_add_trajectory, the two replace calls, ss_extend_lap, ss_add_point) against tests/store_ref.py,
bit for bit, at the smallest shapes at which the store-writing kernels' scans and reductions can go wrong: the 256-row pass edge of the cost scan, the
four-rows-per-thread, 256-rows-per-wave and 1024-rows-per-chunk edges of the image's min / max reduction, a one-row lap, a tie in the sorted order.  Every
context starts at max_laps = 4, max_lap_len = 256, so both stores grow inside the calls."""
import numpy as np
import pytest

from tests import common, store_ref
from tests.test_gpu_device_commit import _same_stores, _stores

pytestmark = pytest.mark.gpu

N = 12


@pytest.fixture(scope="module")
def g():
    return common.load_lmpc_golden()


class _Both:
    """One sequence of store edits applied to a context and to the host restatement."""

    def __init__(self, ctx, cfg):
        self.ctx, self.ref = ctx, store_ref.RefStores.like(cfg)

    def __getattr__(self, name):
        def call(*args):
            getattr(self.ref, name)(*args)
            return getattr(self.ctx, name)(*args)
        return call

    def check(self, what):
        got = _stores(self.ctx)
        _same_stores(got, self.ref.snapshot(), what)
        return got


def _lap(T, TL, seed, cross=0.9):
    """T rows of generic values; s rises to 1.05 trackLength, crossing the line at about cross * T."""
    rng = np.random.default_rng(seed)
    x, u = rng.standard_normal((T, 6)), rng.standard_normal((T, 2))
    x[:, 4] = np.linspace(0.0, 1.05 * TL / cross, T) if T > 1 else 0.5 * TL
    return x, u


def _open(g):
    from racinglmpc_amd import _capi
    cfg, _ = common.lmpc_config(g, N, max_batch=4, max_laps=4, max_lap_len=256)
    return _capi.Context(cfg), cfg


def test_lap_lengths(built, g):
    """1 row (safe set only), 2, the pass edge of the cost scan (256, 257), the image's chunk edge (1024 .. 1026 rows: 1023 .. 1025 image rows), two laps of 300."""
    ctx, cfg = _open(g)
    with ctx:
        b = _Both(ctx, cfg)
        b.ss_add_trajectory(*_lap(1, cfg.trackLength, 1))
        rows = [2, 256, 257, 1024, 1025, 1026, 300, 300]
        for k, T in enumerate(rows):
            x, u = _lap(T, cfg.trackLength, 10 + k)
            b.ss_add_trajectory(x, u); b.model_add_trajectory(x, u)
        got = b.check("lap lengths")
        assert [s[4] for s in got["ss"]] == [1] + rows and got["ss"][0][2].tolist() == [0.0]
        assert [i[1] for i in got["info"]] == [0, 1, 2, 5, 6, 7, 3, 4]                             # the two 300s behind one another, in front of 1024
        assert [im[2] for im in got["image"]] == [1, 1, 1, 1, 1, 2, 1, 1]
        assert all(s[2][0] > 0 and s[2][-1] == 0 and not s[2][-2:].any() for s in got["ss"][2:])   # the cost counts up to the crossing and is 0 behind it


def test_compute_cost_rows_at_the_pass_edges(built, g):
    """s >= trackLength at rows 255 and 256 (either side of the scan's last full pass) and at T - 1; one NaN s (not below trackLength: cost 0)."""
    ctx, cfg = _open(g)
    with ctx:
        b = _Both(ctx, cfg)
        TL = cfg.trackLength
        for T, at in ((600, (255, 256, 599)), (600, (255,)), (600, (256,)), (257, (256,)), (513, (255, 256, 511, 512))):
            x, u = _lap(T, TL, T + len(at))
            x[:, 4] = np.linspace(0.0, 0.99 * TL, T)
            x[list(at), 4] = [TL, TL * 1.5, np.inf, TL, TL][:len(at)]
            x[100, 4] = np.nan
            b.ss_add_trajectory(x, u)
        got = b.check("computeCost")
        q = got["ss"][0][2]
        assert q[599] == 0 and q[598] == 1 and q[257] == 342 and q[256] == 0 and q[255] == 0 and q[254] == 1 and q[100] == 0 and q[99] == 1 and q[0] == 100


def _zero_pair(col, r0, first_negative):
    col[:] = np.abs(col) + 0.25
    col[r0], col[r0 + 1] = (-0.0, 0.0) if first_negative else (0.0, -0.0)


def test_image_minima_and_floors(built, g):
    """A +0.0 / -0.0 pair as a feature's minimum across a thread edge (rows 3, 4), a wave edge (255, 256) and a chunk edge (1023, 1024), both signs first; a feature
    with no finite value in a chunk; constant features (the 1e-9 floor of a range) and all-zero ones (the 1e-300 floor); entries of 1e300 and of +-1e308."""
    ctx, cfg = _open(g)
    with ctx:
        b = _Both(ctx, cfg)
        TL = cfg.trackLength
        for neg in (False, True):
            x, u = _lap(1100, TL, 3 + neg)
            _zero_pair(x[:, 0], 3, neg); _zero_pair(x[:, 1], 255, neg); _zero_pair(x[:, 2], 1023, neg)
            u[1024:, 0] = np.nan; u[1030, 0] = np.inf                                             # delta: nothing finite in chunk 1
            u[:, 1] = 2.5
            b.model_add_trajectory(x, u)
        x = np.tile(np.array([1.5, -2.0, 0.25, 0.0, 1.0, 0.0]), (50, 1)); u = np.tile(np.array([0.1, 3.0]), (50, 1))
        b.model_add_trajectory(x, u)                                                              # every feature constant
        b.model_add_trajectory(np.zeros((9, 6)), np.zeros((9, 2)))                                # every feature zero
        x, u = _lap(40, TL, 7); x[11, 1] = 1e300; u[12, 1] = -1e300
        b.model_add_trajectory(x, u)
        x, u = _lap(40, TL, 8); x[11, 2] = 1e308; x[30, 2] = -1e308                               # (a range that is not finite: scale 0)
        b.model_add_trajectory(x, u)
        got = b.check("image")
        p0, p1 = got["image"][0][1], got["image"][1][1]
        assert got["image"][0][2] == 2 and not np.signbit(p0[0, 0:3]).any() and np.signbit(p1[0, 0:3]).all() and not (p0[0, 0:3] != 0).any()
        assert np.signbit(p0[1, 2]) and not np.signbit(p1[1, 2]) and p0[1, 2] == 0                # (row 1024 is chunk 1's own minimum)
        assert p0[1, 3] == 0 and not (got["image"][0][0][1, 1024:] >> 16).any()
        assert got["image"][2][1][0, 5] == 65535.0 / (1e-9 * 3.0) and got["image"][3][1][0, 5] == 65535.0 / 1e-300
        assert got["image"][4][1][0, 5] == 65535.0 / 1e300 and got["image"][5][1][0, 5] == 0.0


def test_replace_extend_and_add_point(built, g):
    """model_replace_lap of a stored lap; ss_replace_lap with a Qfun ending at 1/3, then 40 appended rows (counted down by repeated subtraction) and one
    ss_add_point; ss_extend_lap with a NaN row, which is appended as given."""
    ctx, cfg = _open(g)
    with ctx:
        b = _Both(ctx, cfg)
        TL = cfg.trackLength
        for k, T in enumerate((100, 120, 110)):
            x, u = _lap(T, TL, 20 + k)
            b.ss_add_trajectory(x, u); b.model_add_trajectory(x, u)
        x, u = _lap(110, TL, 30)
        b.model_replace_lap(1, x, u)                                                              # sorted position 1: the lap of 110 rows
        b.check("model_replace_lap")
        x, u = _lap(120, TL, 31)
        b.ss_replace_lap(2, x, u, np.arange(119, -1, -1.0) + 1.0 / 3.0)                           # (longer than the lap it replaces)
        xe, ue = _lap(40, TL, 32)
        b.ss_extend_lap(2, xe, ue)
        b.ss_add_point(xe[0], ue[0])
        got = b.check("ss_replace_lap, extension, addPoint")
        q = got["ss"][2][2]
        assert got["ss"][2][3:] == (110, 161) and q[119] == 1.0 / 3.0 and q[120] == 1.0 / 3.0 - 1.0
        assert any(q[120 + i] != 1.0 / 3.0 - (i + 1) for i in range(41))                           # (the closed form is another number)
        xe, ue = _lap(130, TL, 33)
        xe[5] = np.nan; ue[5] = np.nan; xe[77, 4] = np.inf
        b.ss_extend_lap(0, xe, ue)
        got = b.check("extension with a NaN row")
        assert got["ss"][0][3:] == (100, 230) and np.isnan(got["ss"][0][0][105]).all() and got["ss"][0][2][229] == -130.0
        b.ss_extend_lap(0, xe[:30], ue[:30])                                                       # (rows 230 .. 259: across the capacity of 256)
        b.check("a second extension")
