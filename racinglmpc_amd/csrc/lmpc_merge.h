// racinglmpc_amd/csrc/lmpc_merge.h -- the grid of a two-role launch of the multi-wave solve kernel (lmpc_solve_mw.hip.h): the solve of one step and the
// regression of the next in ONE launch.  Host and device use the same arithmetic; no HIP header is needed (tests/test_merged_grid_host.py compiles it with g++).
//
//   work-groups [0, B_solve)                          solve role, work-group j solves problem j (lowest ids: placed first)
//   work-groups [B_solve, B_solve + B_next * npass)   regression role, work-group B_solve + j serves problem j / npass, queries (j % npass) * QGe .. of the N
//
// QGe: queries per regression work-group (k1_queries_per_block under the host's cap), npass = ceil(N / QGe); the last work-group of a problem may be partial.
#pragma once
#if defined(__HIPCC__)
#define LMPC_MERGE_HD __host__ __device__
#else
#define LMPC_MERGE_HD
#endif

struct lmpc_wg_role { int role, b, i0, nq; };       // role 0: solve problem b;  role 1: regression of problem b, queries i0 .. i0 + nq - 1;  role -1: beyond the grid

LMPC_MERGE_HD inline int lmpc_merged_npass(int N, int QGe) { return (N + QGe - 1) / QGe; }
LMPC_MERGE_HD inline long long lmpc_merged_grid(int B_solve, int B_next, int N, int QGe) { return (long long)B_solve + (long long)B_next * lmpc_merged_npass(N, QGe); }
LMPC_MERGE_HD inline lmpc_wg_role lmpc_merged_role(long long wg, int B_solve, int B_next, int N, int QGe) {
    lmpc_wg_role r = {-1, 0, 0, 0};
    if (wg < 0 || QGe < 1 || wg >= lmpc_merged_grid(B_solve, B_next, N, QGe)) return r;
    if (wg < B_solve) { r.role = 0; r.b = (int)wg; return r; }
    const int npass = lmpc_merged_npass(N, QGe), j = (int)(wg - B_solve);
    r.role = 1; r.b = j / npass; r.i0 = (j % npass) * QGe; r.nq = N - r.i0 < QGe ? N - r.i0 : QGe;
    return r;
}
