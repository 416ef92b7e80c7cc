"""CPU: the one row-set type behind the five per-car tables (vehicle constants, regression laps, safe-set laps, tuning, tracks) at its three levels.
csrc/lmpc_rows.h as a stand-alone program under AddressSanitizer and UBSan (g++ alone: the header includes no HIP header); BatchedRollouts._apply_rows on a
context that records the setter calls; Context._rows_get / _rows_set around a stand-in library; the ValueError texts of the row checks of racinglmpc_amd._capi,
written out.  What needs a context on a device is in tests/test_gpu_row_sets.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import common

# The program checks the contract for one element type and three widths and prints one line per failed check; exit status 1 if any failed.
_ROWS_PROGRAM = r"""
#include "lmpc_rows.h"
#include <cstdio>
#include <cstring>
#include <memory>

static int g_checks = 0, g_failed = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_failed++; printf("FAILED (%s, width %d) line %d: %s\n", g_type, g_width, __LINE__, #cond); } } while (0)
static const char *g_type = "?"; static int g_width = 0;

// fits(B, rule) at n in {0, 1, 3} (rows) against B in {1, 2, 3, 4} (columns), written out
static const int NS[3] = {0, 1, 3};
static const bool EXACT[3][4] = {{true, true, true, true}, {true, true, true, true}, {false, false, true, false}};
static const bool AT_LEAST[3][4] = {{true, true, true, true}, {true, true, true, true}, {true, true, true, false}};

template <class T> static T value(int r, int j) { return (T)(r * 1000 + j + 1); }
template <class T> static std::vector<T> make_rows(int n, int width) {
    std::vector<T> v((size_t)n * width);
    for (int r = 0; r < n; r++) for (int j = 0; j < width; j++) v[(size_t)r * width + j] = value<T>(r, j);
    return v;
}

template <class T> static void run(const char *type, int width) {
    g_type = type; g_width = width;
    const T sentinel = (T)-7;
    for (int in = 0; in < 3; in++) {
        const int n = NS[in];
        lmpc_row_set<T> s(width, "lmpc_some_set");
        CHECK(s.n == 0 && !s.in_force() && s.width == width && s.rows.empty());
        const std::vector<T> src = make_rows<T>(n, width);
        s.assign(n, src.data());
        CHECK(s.n == n && s.in_force() == (n > 0) && s.rows == src && s.width == width && !strcmp(s.setter, "lmpc_some_set"));
        for (int B = 1; B <= 4; B++) {
            CHECK(s.fits(B, LMPC_ROWS_EXACT) == EXACT[in][B - 1]);
            CHECK(s.fits(B, LMPC_ROWS_AT_LEAST) == AT_LEAST[in][B - 1]);
        }
        CHECK(s.stride(width) == (n == 3 ? width : 0));
        CHECK(s.stride(2 * width + 4) == (n == 3 ? 2 * width + 4 : 0));
        if (n == 1) for (int b = 0; b < 4; b++) CHECK(s.row(b) == s.rows.data());          // one row serves every problem
        if (n == 3) for (int b = 0; b < 3; b++) {
            CHECK(s.row(b) == s.rows.data() + (size_t)b * width);
            CHECK(s.row(b)[0] == value<T>(b, 0) && s.row(b)[width - 1] == value<T>(b, width - 1));
        }
        // get: the count always; min(capacity, n) rows into a buffer of exactly `capacity` rows (AddressSanitizer sees a row too many), nothing through NULL
        const int caps[3] = {0, 2, 5};
        for (int ic = 0; ic < 3; ic++) {
            const int cap = caps[ic], copied = cap < n ? cap : n;
            std::unique_ptr<T[]> out(new T[(size_t)cap * width]);
            for (int i = 0; i < cap * width; i++) out[i] = sentinel;
            int got = -1;
            s.get(&got, out.get(), cap);
            CHECK(got == n);
            bool same = true, untouched = true;
            for (int i = 0; i < copied * width; i++) same = same && out[i] == src[i];
            for (int i = copied * width; i < cap * width; i++) untouched = untouched && out[i] == sentinel;
            CHECK(same); CHECK(untouched);
        }
        { int got = -1; s.get(&got, (T *)nullptr, 5); CHECK(got == n); }
        { int got = -1; s.get(&got, (T *)nullptr, 0); CHECK(got == n); }
        // expand: one row per car -- out of the rows themselves, and out of an image of another width and element type
        if (n > 0) {
            const int B = n == 1 ? 3 : 2;                                                  // n = 1 -> B = 3: the row repeated; n = 3 -> B = 2: the first two
            std::unique_ptr<T[]> out(new T[(size_t)B * width]);
            s.expand(B, out.get(), s.rows.data(), (size_t)width);
            bool ok = true;
            for (int b = 0; b < B; b++) for (int j = 0; j < width; j++) ok = ok && out[(size_t)b * width + j] == value<T>(n == 1 ? 0 : b, j);
            CHECK(ok);
            const size_t iw = 2 * (size_t)width + 1;
            const std::vector<long long> image = make_rows<long long>(n, (int)iw);
            std::unique_ptr<long long[]> io(new long long[(size_t)B * iw]);
            s.expand(B, io.get(), image.data(), iw);
            ok = true;
            for (int b = 0; b < B; b++) for (size_t j = 0; j < iw; j++) ok = ok && io[(size_t)b * iw + j] == value<long long>(n == 1 ? 0 : b, (int)j);
            CHECK(ok);
        }
        // clear: back to "the config's value", width and setter kept, every count fits again
        s.clear();
        CHECK(s.n == 0 && !s.in_force() && s.rows.empty() && s.width == width && !strcmp(s.setter, "lmpc_some_set"));
        for (int B = 1; B <= 4; B++) CHECK(s.fits(B, LMPC_ROWS_EXACT) && s.fits(B, LMPC_ROWS_AT_LEAST));
        CHECK(s.stride(width) == 0);
        { int got = -1; T one = sentinel; s.get(&got, &one, 1); CHECK(got == 0 && one == sentinel); }
        // a second assign replaces the first
        const std::vector<T> two = make_rows<T>(2, width);
        s.assign(2, two.data());
        CHECK(s.n == 2 && s.rows == two && s.fits(2, LMPC_ROWS_EXACT) && !s.fits(3, LMPC_ROWS_EXACT) && s.fits(1, LMPC_ROWS_AT_LEAST) && !s.fits(3, LMPC_ROWS_AT_LEAST));
    }
}

int main() {
    const int widths[3] = {1, 2, 98};
    for (int w : widths) { run<int>("int", w); run<double>("double", w); }
    printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
"""


def test_row_set_header_contract_under_sanitizers(tmp_path):
    """lmpc_rows.h alone, g++ -Wall -Werror with AddressSanitizer and UBSan, T in {int, double} x width in {1, 2, 98}: fits under both rules at n in {0, 1, 3} against
    B in {1, 2, 3, 4} (all 24 cells per rule against a table written out), stride, row(b), get at capacity 0 / < n / > n / out == NULL, expand at n = 1 -> B = 3 and
    n = 3 -> B = 2, assign followed by clear."""
    src = tmp_path / "rows.cpp"; src.write_text(_ROWS_PROGRAM)
    exe = str(tmp_path / "rows")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(common.ROOT, "racinglmpc_amd", "csrc"), str(src), "-o", exe], check=True, capture_output=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()
    last = out.strip().split("\n")[-1].split()
    assert last[1] == "checks," and int(last[0]) == 642 and int(last[2]) == 0, out


# ---- rollout.py: one _apply_rows
class _RecordingContext:
    """Stands where a Context does: every row setter records (name, arguments)."""

    def __init__(self):
        self.calls = []

    def track_set(self, rows):
        self.calls.append(("track_set", rows))

    def plant_set_params(self, par):
        self.calls.append(("plant_set_params", par))

    def model_set_lap_table(self, rows):
        self.calls.append(("model_set_lap_table", rows))

    def ss_set_lap_table(self, rows, last=None):
        self.calls.append(("ss_set_lap_table", rows, last))

    def tuning_set(self, rows):
        self.calls.append(("tuning_set", rows))


_SETS = [("tracks", "track_set", 98, np.float64), ("plant_params", "plant_set_params", 10, np.float64), ("lap_table", "model_set_lap_table", 4, np.int32),
         ("ss_table", "ss_set_lap_table", 4, np.int32), ("tuning", "tuning_set", 98, np.float64)]


def _bare_rollouts():
    from racinglmpc_amd.rollout import BatchedRollouts
    ro = BatchedRollouts.__new__(BatchedRollouts)          # (no __init__: the object holds no row set at all)
    ro.ctx = _RecordingContext()
    return ro


@pytest.mark.parametrize("name,setter,width,dtype", _SETS)
def test_apply_rows_hands_each_set_to_its_setter(name, setter, width, dtype):
    B = 3
    for n in (1, B):
        ro = _bare_rollouts()
        rows = np.arange(n * width).reshape(n, width).astype(dtype)
        setattr(ro, name, rows)
        ro._apply_rows(B, (name,))
        assert len(ro.ctx.calls) == 1 and ro.ctx.calls[0][0] == setter and ro.ctx.calls[0][1] is rows
        if name == "ss_table":
            assert ro.ctx.calls[0][2] is None                  # (no ss_last on the object)
            last = np.arange(n, dtype=np.int32)
            ro.ss_last = last
            ro._apply_rows(B, (name,))
            assert ro.ctx.calls[1][0] == setter and ro.ctx.calls[1][1] is rows and ro.ctx.calls[1][2] is last
    ro = _bare_rollouts()
    setattr(ro, name, np.zeros((2, width), dtype))
    with pytest.raises(ValueError) as e:
        ro._apply_rows(B, (name,))
    assert str(e.value) == "%s: one row or one per car (3) expected, got 2" % name
    assert ro.ctx.calls == []
    ro = _bare_rollouts()                                      # the attribute missing, or None: nothing is called
    ro._apply_rows(B, (name,))
    setattr(ro, name, None)
    ro._apply_rows(B, (name,))
    assert ro.ctx.calls == []


def test_apply_rows_keeps_the_order_it_is_given_and_applies_nothing_else():
    ro = _bare_rollouts()
    for name, _, width, dtype in _SETS:
        setattr(ro, name, np.zeros((1, width), dtype))
    ro._apply_rows(5, ("tracks", "plant_params", "lap_table", "ss_table", "tuning"))
    assert [c[0] for c in ro.ctx.calls] == ["track_set", "plant_set_params", "model_set_lap_table", "ss_set_lap_table", "tuning_set"]
    ro.ctx.calls.clear()
    ro._apply_rows(5, ("tracks", "plant_params"))
    assert [c[0] for c in ro.ctx.calls] == ["track_set", "plant_set_params"]
    with pytest.raises(KeyError):
        ro._apply_rows(5, ("trace",))                          # (the traced cars are a list, not a row set: _apply_trace)


# ---- _capi.py: _rows_set / _rows_get around a stand-in library
class _RowsLib:
    """Setter and getters of one row set as the library has them: (handle, n, rows[, last]) and (handle, *n, rows[, last], capacity)."""

    def __init__(self, rows, last=None):
        self.rows, self.last, self.calls = rows, last, []

    @staticmethod
    def _fill(ptr, a, n):
        assert isinstance(ptr, C.c_void_p) and ptr.value
        C.memmove(ptr.value, a.ctypes.data, a[:n].nbytes)

    def set(self, h, n, rows, *extra):
        self.calls.append(("set", h, n, rows, extra))
        return 0

    def get(self, h, n_ref, rows, capacity):
        self.calls.append(("get", h, rows is None, capacity))
        n_ref._obj.value = self.rows.shape[0]
        if rows is not None:
            self._fill(rows, self.rows, min(capacity, self.rows.shape[0]))
        return 0

    def get2(self, h, n_ref, rows, last, capacity):
        self.calls.append(("get2", h, rows is None, last is None, capacity))
        n_ref._obj.value = self.rows.shape[0]
        if rows is not None:
            self._fill(rows, self.rows, min(capacity, self.rows.shape[0])); self._fill(last, self.last, min(capacity, self.rows.shape[0]))
        return 0


def _bare_context():
    from racinglmpc_amd import _capi
    ctx = _capi.Context.__new__(_capi.Context)
    ctx._h = C.c_void_p(77); ctx._pid = -1                     # (another process id: __del__ leaves the stand-in handle alone)
    return ctx


def test_rows_set_and_rows_get_around_a_stand_in_library():
    ctx = _bare_context()
    rows = np.arange(3 * 98, dtype=np.float64).reshape(3, 98)
    lib = _RowsLib(rows)
    ctx._rows_set(lib.set, None)
    ctx._rows_set(lib.set, rows)
    (_, h0, n0, p0, e0), (_, h1, n1, p1, e1) = lib.calls
    assert h0 is ctx._h and n0 == 0 and p0 is None and e0 == ()
    assert h1 is ctx._h and n1 == 3 and p1.value == rows.ctypes.data and e1 == ()
    lib.calls.clear()
    got = ctx._rows_get(lib.get, 98, np.float64)
    assert got.dtype == np.float64 and got.shape == (3, 98) and np.array_equal(got, rows) and got is not rows
    assert lib.calls == [("get", ctx._h, True, 0), ("get", ctx._h, False, 3)]       # the count first, then the rows
    empty = _RowsLib(np.zeros((0, 10)))
    got = ctx._rows_get(empty.get, 10, np.float64)
    assert got.shape == (0, 10) and empty.calls == [("get", ctx._h, True, 0)]       # no rows in force: one call
    # rows with a per-row array beside them (the safe-set table and its `last`)
    tab = np.array([[0, 1, 2, 3], [3, 2, 1, 0]], np.int32); last = np.array([3, -1], np.int32)
    lib = _RowsLib(tab, last)
    ctx._rows_set(lib.set, tab, last)
    ctx._rows_set(lib.set, tab, None)
    ctx._rows_set(lib.set, None, None)
    assert lib.calls[0][2] == 2 and lib.calls[0][3].value == tab.ctypes.data and lib.calls[0][4][0].value == last.ctypes.data
    assert lib.calls[1][2] == 2 and lib.calls[1][4] == (None,)
    assert lib.calls[2][2] == 0 and lib.calls[2][3] is None and lib.calls[2][4] == (None,)
    lib.calls.clear()
    r, l = ctx._rows_get(lib.get2, 4, np.int32, np.int32)
    assert r.dtype == np.int32 and np.array_equal(r, tab) and l.dtype == np.int32 and np.array_equal(l, last)
    assert lib.calls == [("get2", ctx._h, True, True, 0), ("get2", ctx._h, False, False, 2)]


def test_rows_set_and_rows_get_raise_the_library_error(monkeypatch):
    from racinglmpc_amd import _capi
    ctx = _bare_context()

    class _Err:
        @staticmethod
        def lmpc_last_error():
            return b"tuning rows: B = 2 problems but lmpc_tuning_set holds 3 rows"
    monkeypatch.setattr(_capi, "load", lambda: _Err)
    with pytest.raises(_capi.LmpcError, match="holds 3 rows"):
        ctx._rows_set(lambda *a: 2, np.zeros((1, 98)))
    with pytest.raises(_capi.LmpcError, match="holds 3 rows"):
        ctx._rows_get(lambda *a: 2, 98, np.float64)


def test_context_getters_and_setters_go_through_the_two_helpers():
    """Every public set / get of the five, on a stand-in library: the entry point it reaches and what it hands over / returns."""
    import types
    from racinglmpc_amd import _capi
    ctx = _bare_context()
    ctx.cfg = types.SimpleNamespace(trToUse=4, numSS_it=4)
    f8 = np.arange(2 * 98, dtype=np.float64).reshape(2, 98) + 1.0
    par = np.arange(20, dtype=np.float64).reshape(2, 10) + 1.0
    tab = np.array([[0, 1, 2, 3], [3, 2, 1, 0]], np.int32); last = np.array([3, -1], np.int32)
    libs = {"plant": _RowsLib(par), "lt": _RowsLib(tab), "sst": _RowsLib(tab, last), "tune": _RowsLib(f8), "trk": _RowsLib(f8)}
    ctx.lib = types.SimpleNamespace(
        lmpc_plant_set_params=libs["plant"].set, lmpc_plant_get_params=libs["plant"].get, lmpc_model_set_lap_table=libs["lt"].set, lmpc_model_get_lap_table=libs["lt"].get,
        lmpc_ss_set_lap_table=libs["sst"].set, lmpc_ss_get_lap_table=libs["sst"].get2, lmpc_tuning_set=libs["tune"].set, lmpc_tuning_get=libs["tune"].get,
        lmpc_track_set=libs["trk"].set, lmpc_track_get=libs["trk"].get)
    assert np.array_equal(ctx.plant_params(), par) and np.array_equal(ctx.model_lap_table(), tab)
    r, l = ctx.ss_lap_table()
    assert np.array_equal(r, tab) and np.array_equal(l, last)
    libs["sst"].last = np.full(2, _capi.SS_LAST_SHARED, np.int32)
    assert ctx.ss_lap_table()[1] is None                       # set without `last`
    libs["sst"].rows = np.zeros((0, 4), np.int32)
    r, l = ctx.ss_lap_table()
    assert r.shape == (0, 4) and l is None
    ctx.plant_set_params(par); ctx.plant_set_params(par[0]); ctx.plant_set_params(None); ctx.plant_set_params([])
    assert [c[2] for c in libs["plant"].calls if c[0] == "set"] == [2, 1, 0, 0]
    ctx.model_set_lap_table(tab); ctx.model_set_lap_table(None)
    assert [c[2] for c in libs["lt"].calls if c[0] == "set"] == [2, 0]
    ctx.ss_set_lap_table(tab, last); ctx.ss_set_lap_table(tab); ctx.ss_set_lap_table(None)
    sets = [c for c in libs["sst"].calls if c[0] == "set"]
    assert [c[2] for c in sets] == [2, 2, 0] and sets[0][4][0] is not None and sets[1][4] == (None,) and sets[2][4] == (None,)
    tune = np.tile(_tuning_row(), (2, 1))
    ctx.tuning_set(tune); ctx.tuning_set(None)
    assert [c[2] for c in libs["tune"].calls if c[0] == "set"] == [2, 0]
    trk = np.zeros((1, 98)); trk[0, 0] = 1; trk[0, 1] = 10.0; trk[0, 2 + 4] = 10.0
    ctx.track_set(trk); ctx.track_set(None)
    assert [c[2] for c in libs["trk"].calls if c[0] == "set"] == [1, 0]
    assert np.array_equal(ctx.tuning(), f8) and np.array_equal(ctx.tracks(), f8)


def _tuning_row():
    """One row lmpc_tuning_set accepts: identity weights, positive bounds."""
    from racinglmpc_amd import _capi
    row = np.zeros(_capi.TUNING_NPAR)
    row[_capi.TUNING_FIELDS["Q"]] = np.eye(6).reshape(-1); row[_capi.TUNING_FIELDS["Qf"]] = np.eye(6).reshape(-1); row[_capi.TUNING_FIELDS["R"]] = np.eye(2).reshape(-1)
    for k in ("dR", "Qslack", "QtermSlack", "bx", "bu"):
        row[_capi.TUNING_FIELDS[k]] = 1.0
    return row


def _nan_rows():
    t = np.zeros((2, 98)); t[1, 5] = np.nan
    return t


def _inf_plant():
    p = np.ones((3, 10)); p[2, 0] = np.inf
    return p


# (check, arguments, the text the check raised before the checks shared their opening)
_TEXTS = [
    ("check_plant_params", lambda: (np.zeros((2, 9)),), "plant parameters: rows of 10 values ('m', 'lf', 'lr', 'Iz', 'Df', 'Cf', 'Bf', 'Dr', 'Cr', 'Br') expected, got shape (2, 9)"),
    ("check_plant_params", lambda: (_inf_plant(),), "plant parameters: non-finite entry in row(s) [2]"),
    ("check_tuning", lambda: (np.zeros((1, 97)),), "tuning: rows of 98 values expected, got shape (1, 97)"),
    ("check_tuning", lambda: (_nan_rows(),), "tuning: non-finite entry in row(s) [1]"),
    ("check_tracks", lambda: (np.zeros((3, 97)),), "tracks: rows of 98 values expected, got shape (3, 97)"),
    ("check_tracks", lambda: (_nan_rows(),), "tracks: non-finite entry in row(s) [1]"),
    ("check_lap_table", lambda: ([[0, 1, 2]], 4), "lap table: rows of trToUse = 4 lap indices expected, got shape (1, 3)"),
    ("check_lap_table", lambda: ([[0.5, 1, 2, 3]], 4), "lap table: integer rows of trToUse = 4 lap indices expected, got dtype float64, shape (1, 4)"),
    ("check_lap_table", lambda: ([[0, 1, 2, 3], [0, -1, 2, 3]], 4), "lap table: negative lap index in row(s) [1]"),
    ("check_ss_table", lambda: ([[0, 1, 2]], 4), "safe-set lap table: rows of numSS_it = 4 lap indices expected, got shape (1, 3)"),
    ("check_ss_table", lambda: ([[0.5, 1, 2, 3]], 4), "safe-set lap table: integer rows of numSS_it = 4 lap indices expected, got dtype float64, shape (1, 4)"),
    ("check_ss_table", lambda: ([[0, 1, 2, 3], [0, -1, 2, 3]], 4), "safe-set lap table: negative lap index in row(s) [1]"),
]


@pytest.mark.parametrize("check,args,text", _TEXTS, ids=["%s-%d" % (t[0], i) for i, t in enumerate(_TEXTS)])
def test_row_checks_keep_their_error_texts(check, args, text):
    from racinglmpc_amd import _capi
    with pytest.raises(ValueError) as e:
        getattr(_capi, check)(*args())
    assert str(e.value) == text


def test_row_checks_keep_what_they_accept_and_return():
    from racinglmpc_amd import _capi
    assert _capi.check_tuning(None) is None and _capi.check_tuning([]) is None and _capi.check_tracks(None) is None and _capi.check_tracks(np.zeros((0, 98))) is None
    assert _capi.check_lap_table(None, 4) is None and _capi.check_ss_table(None, 4) == (None, None)
    with pytest.raises(ValueError):
        _capi.check_plant_params(None)                         # (no "no rows" form here: Context.plant_set_params handles None itself)
    flat = _tuning_row()
    r = _capi.check_tuning(flat, 4)
    assert r.shape == (1, 98) and r.dtype == np.float64 and r.flags.c_contiguous and r is not flat and np.array_equal(r[0], flat)
    p = _capi.check_plant_params(list(range(1, 11)))
    assert p.shape == (1, 10) and p.dtype == np.float64 and p.flags.c_contiguous
    t = _capi.check_lap_table([0, 1, 2, 3], 4)
    assert t.shape == (1, 4) and t.dtype == np.int32
    t = _capi.check_lap_table([0, 1, 2], 1)
    assert t.shape == (3, 1)
    r, l = _capi.check_ss_table([[0, 1, 2, 3]], 4, [2])
    assert r.shape == (1, 4) and r.dtype == np.int32 and l.dtype == np.int32 and l.tolist() == [2]
