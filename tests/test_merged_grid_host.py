"""CPU: csrc/lmpc_merge.h -- the grid of a two-role launch of the four-wave solve kernel (the solve of one step and the regression of the next in one launch) -- as a
stand-alone program under AddressSanitizer and UBSan (g++ alone: the header includes no HIP header).  Host and device take the work-group count and every
work-group's role, problem and first query from these functions and from nowhere else."""
import os
import subprocess

from tests import common

_GRID_PROGRAM = r"""
#include "lmpc_merge.h"
#include <cstdio>
#include <vector>

static int g_checks = 0, g_failed = 0;
#define CHECK(cond) do { g_checks++; if (!(cond)) { g_failed++; printf("FAILED line %d (Bs %d Bn %d N %d QGe %d wg %lld): %s\n", __LINE__, Bs, Bn, N, Q, wg, #cond); } } while (0)

int main() {
    const int batches[] = {1, 3}, horizons[] = {2, 12, 14, 64};
    for (int Bs : batches) for (int Bn : batches) for (int N : horizons) for (int Q = 1; Q <= 12; Q++) {
        long long wg = -1;
        const long long grid = lmpc_merged_grid(Bs, Bn, N, Q);
        const int npass = lmpc_merged_npass(N, Q);
        CHECK(npass * Q >= N && (npass - 1) * Q < N);                       // the fewest work-groups that hold N queries
        CHECK(grid == Bs + (long long)Bn * npass);
        std::vector<int> solved(Bs, 0), served((size_t)Bn * N, 0);
        int last_role = 0;
        for (wg = 0; wg < grid; wg++) {
            const lmpc_wg_role r = lmpc_merged_role(wg, Bs, Bn, N, Q);
            CHECK(r.role == 0 || r.role == 1);
            CHECK(r.role >= last_role); last_role = r.role;                  // the solves have the lowest ids
            if (r.role == 0) { CHECK(wg < Bs && r.b == (int)wg); if (r.b >= 0 && r.b < Bs) solved[r.b]++; }
            if (r.role == 1) {
                CHECK(wg >= Bs && r.b >= 0 && r.b < Bn && r.i0 >= 0 && r.i0 % Q == 0 && r.nq >= 1 && r.nq <= Q && r.i0 + r.nq <= N);
                CHECK(r.b == (int)((wg - Bs) / npass) && r.i0 == (int)((wg - Bs) % npass) * Q);
                CHECK(r.nq == Q || r.i0 + r.nq == N);                        // partial only at the end of a problem
                if (r.b >= 0 && r.b < Bn) for (int q = r.i0; q < r.i0 + r.nq && q < N; q++) served[(size_t)r.b * N + q]++;
            }
        }
        wg = -1;
        for (int b = 0; b < Bs; b++) CHECK(solved[b] == 1);                   // every problem solved exactly once
        for (size_t e = 0; e < served.size(); e++) CHECK(served[e] == 1);     // every (problem, query) served exactly once
        for (wg = grid; wg < grid + 3; wg++) CHECK(lmpc_merged_role(wg, Bs, Bn, N, Q).role == -1);      // nothing beyond the count
        wg = -1; CHECK(lmpc_merged_role(wg, Bs, Bn, N, Q).role == -1);
    }
    printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
"""


def test_merged_grid_covers_every_problem_and_query_once(tmp_path):
    """B_solve and B_next in {1, 3}, N in {2, 12, 14, 64}, every QGe from 1 to 12 (K1_QG): the count is B_solve + B_next ceil(N / QGe); the first B_solve
    work-groups solve problems 0 .. B_solve - 1; every (problem, query) of the next step is served by exactly one regression work-group, whose range is partial
    only at the end of a problem; ids beyond the count have no role."""
    src = tmp_path / "grid.cpp"; src.write_text(_GRID_PROGRAM)
    exe = str(tmp_path / "grid")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", os.path.join(common.ROOT, "racinglmpc_amd", "csrc"), str(src), "-o", exe], check=True, capture_output=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()
    last = out.strip().split("\n")[-1].split()
    assert last[1] == "checks," and int(last[0]) > 2 * 2 * 4 * 12 * 10 and int(last[2]) == 0, out
