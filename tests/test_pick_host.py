"""CPU: csrc/lmpc_pick.h -- run-time flags into compile-time ones -- as a stand-alone program under AddressSanitizer and UBSan (g++ alone: the header includes no
HIP header), on stand-in function templates shaped like the kernels the host launches through it."""
import os
import subprocess

from tests import common

# One line per failed check; exit status 1 if any failed.  Every stand-in logs (which template, its arguments as bits in the order of its parameter list).
_PICK_PROGRAM = r"""
#include "lmpc_pick.h"
#include <cstdio>
#include <utility>
#include <vector>

static int g_checks = 0, g_failed = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_failed++; printf("FAILED line %d (flags %d%d%d%d): %s\n", __LINE__, g_f[0], g_f[1], g_f[2], g_f[3], #cond); } } while (0)
static bool g_f[4];
static std::vector<std::pair<int, int>> g_log;          // (template, argument bits: first parameter in the highest bit)

struct list { const int *car; int n; };
template <bool A> int one() { g_log.push_back({1, A}); return 100 + A; }
template <bool PAR, bool TRK> int plant() { g_log.push_back({2, PAR * 2 + TRK}); return 200 + PAR * 2 + TRK; }                       // <bool, bool>
template <bool PAR, bool TRK, class... LIVE> int rollout_plant(LIVE... lv) {                                                           // <bool, bool, class...>
    static_assert(sizeof...(LIVE) <= 1, "empty, or one list");
    g_log.push_back({3, PAR * 4 + TRK * 2 + (int)sizeof...(LIVE)});
    int n = 0; ((n = lv.n), ...);
    return 300 + n;
}
template <bool OCC, int RPL, bool TAB, class... LIVE> int regress(LIVE... lv) {                                                        // <bool, int, bool, class...>
    static_assert(TAB || sizeof...(LIVE) == 0, "the list exists with TAB only: this combination must not be instantiated");
    static_assert(RPL == 8 || RPL == 16, "the two scans");
    g_log.push_back({4, OCC * 8 + (RPL == 8) * 4 + TAB * 2 + (int)sizeof...(LIVE)});
    int n = 0; ((n = lv.n), ...);
    return 400 + n;
}
static int g_cell = 7;

int main() {
    const list ll = {nullptr, 5};
    for (int n = 1; n <= 4; n++) for (int mask = 0; mask < (1 << n); mask++) {
        for (int i = 0; i < 4; i++) g_f[i] = i < n && ((mask >> (n - 1 - i)) & 1);          // flag i: bit n-1-i, so that `mask` reads as the flags in order
        g_log.clear();
        int ret = -1;
        if (n == 1) ret = lmpc_pick([&](auto A) { return one<A>(); }, g_f[0]);
        if (n == 2) ret = lmpc_pick([&](auto PAR, auto TRK) { return plant<PAR, TRK>(); }, g_f[0], g_f[1]);
        if (n == 3) ret = lmpc_pick([&](auto PAR, auto TRK, auto LIVE) {
            if constexpr (LIVE) return rollout_plant<PAR, TRK>(ll); else return rollout_plant<PAR, TRK>();
        }, g_f[0], g_f[1], g_f[2]);
        if (n == 4) ret = lmpc_pick([&](auto OCC, auto SMALL, auto TAB, auto LIVE) {
            constexpr bool occ = OCC, tab = TAB; constexpr int rpl = SMALL ? 8 : 16;
            auto go = [&](auto... lv) { return regress<occ, rpl, tab, decltype(lv)...>(lv...); };
            if constexpr (!LIVE) return go();
            else if constexpr (tab) return go(ll);
            else return -2;                                                                  // (list without table: no such kernel, nothing instantiated)
        }, g_f[0], g_f[1], g_f[2], g_f[3]);
        const bool excluded = n == 4 && g_f[3] && !g_f[2];
        CHECK(g_log.size() == (excluded ? 0u : 1u));                                         // exactly one instantiation, exactly once
        if (excluded) { CHECK(ret == -2); continue; }
        if (g_log.size() != 1) continue;
        CHECK(g_log[0].first == n);
        CHECK(g_log[0].second == mask);                                                      // its template arguments are the flags, in the order given
        const int listed = (n >= 3 && g_f[n - 1]) ? 5 : 0;
        CHECK(ret == (n == 1 ? 100 + mask : n == 2 ? 200 + mask : n * 100 + listed));        // the lambda's result comes back
    }
    for (int i = 0; i < 4; i++) g_f[i] = false;
    // a reference comes back as a reference, void as void
    int &cell = lmpc_pick([&](auto A, auto B) -> int & { return g_cell; }, true, false);
    CHECK(&cell == &g_cell);
    int hit = 0;
    lmpc_pick([&](auto A, auto B, auto C) { hit += A * 4 + B * 2 + C; }, true, false, true);
    CHECK(hit == 5);
    printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
"""


def test_pick_header_under_sanitizers(tmp_path):
    """lmpc_pick.h alone, g++ -Wall -Werror with AddressSanitizer and UBSan: one to four flags, all 2 + 4 + 8 + 16 combinations -- one instantiation called once, its
    template arguments the flags in order, the list-without-table combinations of the <bool, int, bool, class...> stand-in never instantiated (a static_assert in
    it), results handed through by value, by reference and as void."""
    src = tmp_path / "pick.cpp"; src.write_text(_PICK_PROGRAM)
    exe = str(tmp_path / "pick")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", os.path.join(common.ROOT, "racinglmpc_amd", "csrc"), str(src), "-o", exe], check=True, capture_output=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()
    last = out.strip().split("\n")[-1].split()
    # 30 combinations: 4 excluded (2 checks each), 26 called (4 checks each), and the two result forms
    assert last[1] == "checks," and int(last[0]) == 4 * 2 + 26 * 4 + 2 and int(last[2]) == 0, out
