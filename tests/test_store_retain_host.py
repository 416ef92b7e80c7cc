"""CPU: laps given back from the lap stores (lmpc_store_retain) -- what needs no device.  csrc/lmpc_retain.h, the books, as a stand-alone program under
AddressSanitizer and UBSan (g++ alone: the header includes no HIP header); the ValueError texts of _capi.check_retain, written out; rollout.PerCarHistory.prune
against the unpruned history over random add sequences; rollout.PerCarLMPC(prune=True) on a context that only counts rows.  What needs a context on a device is in
tests/test_gpu_store_retain.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import common, retain_ref
from tests.test_device_commit_host import SCRIPT, _LoopCtx

# One line per failed check; exit status 1 if any failed.
_RETAIN_PROGRAM = r"""
#include "lmpc_retain.h"
#include <cstdio>
#include <memory>

static int g_checks = 0, g_failed = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_failed++; printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)
typedef std::vector<int> vi;
#define LAST_SHARED (-2)

// a keep list in a heap block of exactly its size (AddressSanitizer sees an entry too many)
static std::unique_ptr<int[]> block(const vi &v) { std::unique_ptr<int[]> p(new int[v.size()]); for (size_t i = 0; i < v.size(); i++) p[i] = v[i]; return p; }
static int check(const vi &keep, int stored, int *why = nullptr) { auto p = block(keep); return lmpc_retain_check((int)keep.size(), p.get(), stored, why); }
static vi map_of(const vi &keep, int stored) { auto p = block(keep); return lmpc_retain_map((int)keep.size(), p.get(), stored); }
static long long dropped(const vi &idx, const vi &map) { auto p = block(idx); const long long at = lmpc_retain_first_dropped(p.get(), idx.size(), map); for (size_t i = 0; i < idx.size(); i++) CHECK(p[i] == idx[i]); return at; }
static vi remapped(const vi &idx, const vi &map) { auto p = block(idx); lmpc_retain_remap(p.get(), idx.size(), map); return vi(p.get(), p.get() + idx.size()); }

int main() {
    // identity: every lap kept
    CHECK(check({0, 1, 2, 3, 4}, 5) == -1);
    CHECK(map_of({0, 1, 2, 3, 4}, 5) == (vi{0, 1, 2, 3, 4}) && map_of({0, 1, 2, 3, 4}, 5) == lmpc_retain_identity(5));
    CHECK(lmpc_retain_keeps_all(lmpc_retain_identity(5)) && lmpc_retain_keeps_all(lmpc_retain_identity(0)) && lmpc_retain_kept(lmpc_retain_identity(5)) == 5);
    // the first, a middle and the last lap dropped
    CHECK(check({1, 2, 3, 4}, 5) == -1 && map_of({1, 2, 3, 4}, 5) == (vi{-1, 0, 1, 2, 3}));
    CHECK(check({0, 1, 3, 4}, 5) == -1 && map_of({0, 1, 3, 4}, 5) == (vi{0, 1, -1, 2, 3}));
    CHECK(check({0, 1, 2, 3}, 5) == -1 && map_of({0, 1, 2, 3}, 5) == (vi{0, 1, 2, 3, -1}));
    CHECK(!lmpc_retain_keeps_all(map_of({1, 2, 3, 4}, 5)) && !lmpc_retain_keeps_all(map_of({0, 1, 3, 4}, 5)) && !lmpc_retain_keeps_all(map_of({0, 1, 2, 3}, 5)));
    CHECK(lmpc_retain_kept(map_of({1, 3}, 5)) == 2);
    // a store emptied; an empty store
    CHECK(check({}, 5) == -1 && map_of({}, 5) == (vi{-1, -1, -1, -1, -1}) && lmpc_retain_kept(map_of({}, 5)) == 0 && !lmpc_retain_keeps_all(map_of({}, 5)));
    CHECK(check({}, 0) == -1 && map_of({}, 0).empty());
    // refused lists: the position of the first offender and why
    int why = -1;
    CHECK(check({3, 2}, 5, &why) == 1 && why == 1);                     // descending
    CHECK(check({0, 2, 2, 4}, 5, &why) == 2 && why == 1);               // duplicate
    CHECK(check({0, 5}, 5, &why) == 1 && why == 0);                     // past the end
    CHECK(check({-1, 0}, 5, &why) == 0 && why == 0);                    // negative
    CHECK(check({0}, 0, &why) == 0 && why == 0);                        // an empty store holds no lap 0
    CHECK(check({4, 1, 7}, 5) == 1);                                    // the first one only
    // per-lap vectors
    const vi map = map_of({1, 3, 4, 6}, 7);
    CHECK(map == (vi{-1, 0, -1, 1, 2, -1, 3}));
    CHECK(lmpc_retain_gather(vi{10, 11, 12, 13, 14, 15, 16}, map) == (vi{11, 13, 14, 16}));
    CHECK(lmpc_retain_gather(std::vector<double>{.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5}, map) == (std::vector<double>{1.5, 3.5, 4.5, 6.5}));
    CHECK(lmpc_retain_gather(vi{1, 2, 3}, map_of({}, 3)).empty());
    // the sorted order: lengths 30 20 30 20 10 20 30 -> order 4 1 3 5 0 2 6 (ascending rows, ties by insertion index); ties before and after
    const vi order{4, 1, 3, 5, 0, 2, 6};
    CHECK(lmpc_retain_order(order, map) == (vi{2, 0, 1, 3}));          // kept 1 3 4 6 with lengths 20 20 10 30: 4 | 1 3 | 6 under new names
    CHECK(lmpc_retain_order(order, map_of({0, 2, 5, 6}, 7)) == (vi{2, 0, 1, 3}));    // lengths 30 30 20 30: 5 | 0 2 6
    CHECK(lmpc_retain_order(order, lmpc_retain_identity(7)) == order);
    CHECK(lmpc_retain_order(order, map_of({}, 7)).empty());
    // tables: every named lap kept -> -1 and the rows under their new names, duplicates inside a row included
    const vi rows{1, 1, 3, 6, 6, 4, 3, 1};
    CHECK(dropped(rows, map) == -1 && remapped(rows, map) == (vi{0, 0, 1, 3, 3, 2, 1, 0}));
    // a table row, a `last` entry and the override naming a dropped lap: the position of the first such entry, the inputs untouched (checked inside dropped())
    CHECK(dropped({1, 3, 4, 6, 1, 2, 4, 6}, map) == 5);
    CHECK(dropped({6, -1, 5, LAST_SHARED}, map) == 2);
    CHECK(dropped({0}, map) == 0 && dropped({7}, map) == 0 && dropped({1, 99}, map) == 1);    // (an index past the store names a lap that is not kept either)
    CHECK(dropped({}, map) == -1);
    // sentinels pass through: -1 "none of the row's laps", LMPC_SS_LAST_SHARED
    CHECK(dropped({-1, LAST_SHARED, 6, -1}, map) == -1 && remapped({-1, LAST_SHARED, 6, -1}, map) == (vi{-1, LAST_SHARED, 3, -1}));
    CHECK(dropped({LAST_SHARED, LAST_SHARED}, map_of({}, 7)) == -1 && remapped({LAST_SHARED, LAST_SHARED}, map_of({}, 7)) == (vi{LAST_SHARED, LAST_SHARED}));
    // capacity: the smallest initial * 2^j that holds the laps
    CHECK(lmpc_retain_capacity(4, 0) == 4 && lmpc_retain_capacity(4, 4) == 4 && lmpc_retain_capacity(4, 5) == 8 && lmpc_retain_capacity(4, 8) == 8 && lmpc_retain_capacity(4, 9) == 16);
    CHECK(lmpc_retain_capacity(3, 7) == 12 && lmpc_retain_capacity(64, 1) == 64 && lmpc_retain_capacity(1, 1000) == 1024);
    printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
"""


def test_retain_header_contract_under_sanitizers(tmp_path):
    """lmpc_retain.h alone, g++ -Wall -Werror with AddressSanitizer and UBSan: identity; the first, a middle and the last lap dropped; a store emptied; descending,
    duplicate and out-of-range lists refused at the first offender; a table row, a `last` entry and the override naming a dropped lap refused with the inputs
    untouched; sentinels passed through; the sorted order with ties in length before and after; the capacity rule."""
    src = tmp_path / "retain.cpp"; src.write_text(_RETAIN_PROGRAM)
    exe = str(tmp_path / "retain")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(common.ROOT, "racinglmpc_amd", "csrc"), str(src), "-o", exe], check=True, capture_output=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()
    last = out.strip().split("\n")[-1].split()
    assert last[1] == "checks," and int(last[0]) >= 60 and int(last[2]) == 0, out


def test_the_restatement_agrees_with_itself_on_the_same_cases():
    """tests/retain_ref.py on the cases of the program above: the GPU tests compare a context against it."""
    assert retain_ref.check_keep([0, 1, 3, 4], 5) is None and retain_ref.check_keep([], 0) is None
    assert retain_ref.check_keep([3, 2], 5) == 1 and retain_ref.check_keep([0, 2, 2], 5) == 2 and retain_ref.check_keep([0, 5], 5) == 1 and retain_ref.check_keep([-1], 5) == 0
    m = retain_ref.keep_map([1, 3, 4, 6], 7)
    assert m.tolist() == [-1, 0, -1, 1, 2, -1, 3] and m.dtype == np.int32
    assert retain_ref.remap([[1, 1, 3, 6], [6, 4, 3, 1]], m).tolist() == [[0, 0, 1, 3], [3, 2, 1, 0]]
    assert retain_ref.remap([-1, -2, 6], m).tolist() == [-1, -2, 3]
    for bad in ([2], [7], [1, 5]):
        with pytest.raises(ValueError):
            retain_ref.remap(bad, m)
    assert [retain_ref.capacity(4, n) for n in (0, 4, 5, 8, 9)] == [4, 4, 8, 8, 16]
    assert retain_ref.lap_bytes(512) == 2 * 9 * 512 * 8 + 3 * 512 * 4 + 48 == 79920          # "about 80 KB at max_lap_len 512"
    assert retain_ref.lap_bytes(2048) == 2 * 9 * 2048 * 8 + 3 * 2048 * 4 + 2 * 48


def test_check_retain_error_texts():
    from racinglmpc_amd import _capi
    a = _capi.check_retain([0, 2, 5], 6, "safe set")
    assert a.dtype == np.int32 and a.tolist() == [0, 2, 5] and a.flags["C_CONTIGUOUS"]
    assert _capi.check_retain([], 0, "safe set").shape == (0,) and _capi.check_retain(np.zeros(0), 3, "safe set").dtype == np.int32      # an empty list empties the store
    assert _capi.check_retain(np.arange(4, dtype=np.int64), 4, "regression store").tolist() == [0, 1, 2, 3]
    cases = [
        (([[0, 1]], 3, "safe set"), "store_retain: safe set: a one-dimensional list of lap indices expected, got shape (1, 2)"),
        (([0.0, 1.0], 3, "safe set"), "store_retain: safe set: integer lap indices expected, got dtype float64"),
        (([-1, 0, -3], 3, "regression store"), "store_retain: regression store: negative lap index at position(s) [0, 2]"),
        (([0, 3], 3, "safe set"), "store_retain: safe set: position(s) [1] name a lap that is not stored (3 laps are)"),
        (([0], 0, "safe set"), "store_retain: safe set: position(s) [0] name a lap that is not stored (0 laps are)"),
        (([2, 1], 3, "safe set"), "store_retain: safe set: strictly ascending lap indices expected, position 1 holds 1 after 2"),
        (([0, 1, 1, 2], 3, "regression store"), "store_retain: regression store: strictly ascending lap indices expected, position 2 holds 1 after 1"),
    ]
    for args, text in cases:
        with pytest.raises(ValueError) as e:
            _capi.check_retain(*args)
        assert str(e.value) == text, (args, str(e.value))


def test_history_prune_is_lossless():
    """200 seeded random add sequences over 3 cars, lengths from a small range (ties) and repeated indices (add(times=...)): after every add, row(b) of a history
    that is pruned, and renumbered as a store_retain of its indices would renumber it, equals row(b) of one that never is, through the accumulated map."""
    from racinglmpc_amd import rollout
    for seed in range(200):
        rng = np.random.default_rng(seed)
        width = int(rng.integers(1, 5))
        full, cut = rollout.PerCarHistory(3, width), rollout.PerCarHistory(3, width)
        names = {}                                     # index in the unpruned numbering -> index in the pruned one
        stored = 0                                     # laps the pruned store holds
        for b in range(3):                             # (as PerCarLMPC.seed: one lap per car, repeated until the row is full)
            T = int(rng.integers(20, 26))
            full.add(b, T, b, times=width); cut.add(b, T, stored, times=width); names[b] = stored; stored += 1
        nxt = 3
        for step in range(int(rng.integers(5, 25))):
            b, T, times = int(rng.integers(0, 3)), int(rng.integers(20, 26)), int(rng.integers(1, 3))
            full.add(b, T, nxt, times=times); cut.add(b, T, stored, times=times); names[nxt] = stored; nxt += 1; stored += 1
            if rng.integers(0, 2):                     # prune now, or let a few adds pile up first
                cut.prune()
                keep = sorted(cut.indices())
                m = retain_ref.keep_map(keep, stored)
                cut.remap(m)
                names = {k: int(m[v]) for k, v in names.items() if m[v] >= 0}
                stored = len(keep)
                assert all(len(e) <= width for e in cut.entries)
            for c in range(3):
                assert [names[i] for i in full.row(c)] == cut.row(c), (seed, step, c)
    h = rollout.PerCarHistory(1, 2)
    h.add(0, 30, 0); h.add(0, 20, 1); h.add(0, 20, 2); h.add(0, 10, 3, times=1)
    h.prune()
    assert h.entries[0] == [(20, 1), (10, 3)] and h.row(0) == [3, 1]      # the first of the two 20s stays; entries keep the order they were added in
    with pytest.raises(ValueError):
        h.remap([0, 1, 2, -1])


class _RetainCtx(_LoopCtx):
    """tests/test_device_commit_host._LoopCtx with a store_retain that gathers its row counts and records the call; the tables it holds must name kept laps."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.retains = []

    def store_retain(self, ss=None, model=None):
        ms, mm = retain_ref.keep_map(ss, len(self.ss)), retain_ref.keep_map(model, len(self.model))
        assert retain_ref.check_keep(ss, len(self.ss)) is None and retain_ref.check_keep(model, len(self.model)) is None
        self._model_rows = retain_ref.remap(self._model_rows, mm)          # (raises where a table in force names a dropped lap, as the library refuses)
        self._ss_rows, self._ss_last = retain_ref.remap(self._ss_rows, ms), retain_ref.remap(self._ss_last, ms)
        self.retains.append((self.gen, list(ss), list(model), len(self.ss), len(self.model)))
        self.rows = [self.rows[k] for k in ss]; self.ss = [self.ss[k] for k in ss]; self.model = [self.model[k] for k in model]
        return ms, mm

    def rollout_commit_laps(self, cars, rows=None, ss=True, model=True):
        first_model = len(self.model)
        first, _ = super().rollout_commit_laps(cars, rows, ss, model)
        return first, first_model


def _loop(device_commit, prune):
    from racinglmpc_amd import rollout
    ctx = _RetainCtx(3, 2, SCRIPT)
    ro = rollout.BatchedRollouts(ctx, np.array(common.load_lmpc_golden()["track"]), seed=1, prefetch=False)
    loop = rollout.PerCarLMPC(ro, T_max=60, ext=10, device_commit=device_commit, prune=prune)
    lap = lambda T, ends: (np.zeros((T, 6)), np.zeros((T, 2)), None, np.zeros(12), T if ends else T - 20, 0)
    loop.seed([lap(50, True), [lap(70, True), lap(60, True)], lap(80, False), [lap(90, False)]])
    gens = []
    for _ in range(len(SCRIPT)):
        out = loop.run()
        gens.append(dict(out=out, ss_table=ro.ss_table.copy(), ss_last=ro.ss_last.copy(), lap_table=ro.lap_table.copy(), retired=dict(loop.retired),
                         lap_times=[list(t) for t in loop.lap_times], counts=(ctx.ss_num_laps(), ctx.model_num_laps()), rows=list(ctx.rows), model=list(ctx.model)))
    return ctx, loop, gens


@pytest.mark.parametrize("device_commit", [False, True], ids=["host_adds", "device_commit"])
def test_per_car_lmpc_prune_keeps_the_books(device_commit):
    """The four-generation script of tests/test_device_commit_host.py with and without prune, on a context that only counts rows: one store_retain after seed and one
    after every generation, its keep lists the union of the rows (and `last`) of all cars, retired ones included; lap times, retired cars and the returned laps as
    without it; the tables name laps of the same lengths; the two stores' counts differ (two counters) and stay within B (numSS_it + 1) and B trToUse."""
    B, numSS_it, trToUse = 4, 3, 2
    pc, pl, pg = _loop(device_commit, True)
    fc, fl, fg = _loop(device_commit, False)
    assert not fc.retains and [r[0] for r in pc.retains] == [-1, 0, 1, 2, 3]
    assert pl.retired == fl.retired and pl.lap_times == fl.lap_times and pl.steps == fl.steps
    for gen, (p, f) in enumerate(zip(pg, fg)):
        assert p["retired"] == f["retired"] and p["lap_times"] == f["lap_times"], gen
        assert [o is None for o in p["out"]] == [o is None for o in f["out"]], gen
        for po, fo in zip(p["out"], f["out"]):
            if po is not None:
                assert po[4] == fo[4] and po[5] == fo[5] and np.array_equal(po[0], fo[0]) and np.array_equal(po[1], fo[1]) and np.array_equal(po[3], fo[3])
        # the same laps under other names: rows (with the extensions) of every lap a table names
        for k, store in (("ss_table", "rows"), ("ss_last", "rows"), ("lap_table", "model")):
            assert [[p[store][i] for i in row] for row in np.atleast_2d(p[k]).tolist()] == [[f[store][i] for i in row] for row in np.atleast_2d(f[k]).tolist()], (gen, k)
        ns, nm = p["counts"]
        assert ns <= B * (numSS_it + 1) and nm <= B * trToUse, (gen, ns, nm)
        # nothing is held that no car names
        assert set(range(ns)) == set(p["ss_table"].reshape(-1).tolist()) | set(p["ss_last"].tolist()) and set(range(nm)) == set(p["lap_table"].reshape(-1).tolist())
    # Worked out by hand from the script (valid laps per generation: 4, 3, 1, 1; widths 3 and 2).  Unpruned both stores count 5, 9, 12, 13, 14.
    assert [f["counts"] for f in fg] == [(9, 9), (12, 12), (13, 13), (14, 14)]
    # The seed keeps all five laps of both stores (car 1's two laps fill its regression row of width 2, and its safe-set row of width 3 is 60, 60, 70).
    assert pc.retains[0] == (-1, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], 5, 5)
    # Generation 0 stores laps 5 .. 8 of 50, 40, 30, 45 rows.  Safe set: car 1's 70-row lap 1 leaves its row (40, 60, 60).  Regression store: lap 1 likewise (40, 60),
    # and car 0's new lap 5 of 50 rows never enters its row (50, 50: the seed lap twice, first among equals) -- it is kept in the safe set as car 0's latest only.
    assert pc.retains[1] == (0, [0, 2, 3, 4, 5, 6, 7, 8], [0, 2, 3, 4, 6, 7, 8], 9, 9)
    # From here on the two stores' indices differ.  Generation 1 (cars 0, 1, 3): safe set 8 + 3, car 0's previous latest goes; regression store 7 + 3, car 0's lap
    # again, car 1's 60-row lap (40, 40) and car 3's 90-row lap (44, 45) go.  Generation 2 (car 0, 35 rows) and 3 (car 0, 36 rows): car 0's rows fill up with its
    # own fast laps; the retired cars 1, 2, 3 keep theirs.
    assert [(r[3], r[4], len(r[1]), len(r[2])) for r in pc.retains[2:]] == [(11, 10, 10, 7), (11, 8, 10, 8), (11, 9, 11, 8)]
    assert [p["counts"] for p in pg] == [(8, 7), (10, 7), (10, 8), (11, 8)]
