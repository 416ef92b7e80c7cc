// racinglmpc_amd/csrc/lmpc_live.hip.h -- parking (lmpc_rollout_set_parking): the ordered list of the cars a session still steps.
//
// A car is parked when the caller listed it before the session began (parked0), when an earlier rebuild parked it (parkedAt >= 0), or -- LMPC_PARK_FINISHED -- when
// it has crossed the line (doneAt >= 0).  One launch turns doneAt, the start flags, the previous parkedAt and the step t into
//   live[0 .. nLive)   the indices of the cars that are not parked, ASCENDING: the grid position of a car in the step's kernels is a function of the set of live
//                      cars alone, not of the order in which waves of this kernel happen to run;
//   parkedAt[b]        -1 while car b is live, else the first step it was not stepped (t of the rebuild that parked it; an earlier value stays);
//   hdr[1] = nLive, hdr[2] = hdr[0]   (hdr[0]: the session's nDone counter, which the plant kernel advances).
// force == 0: the launch returns at once while hdr[0] == hdr[2] -- nothing has crossed since the last rebuild, so the list stands (the host launches it at every
// finished-lap poll and reads nDone and nLive back in one copy).
//
// One work-group of 1024 threads walks the cars in chunks of 1024 with a carry.  Per wave: a 64-bit ballot of "live", its population count, and the lane's rank among
// the live lanes below it; the 16 wave totals meet in LDS, every thread sums those in front of its wave.  No atomics, no scratch, plain vector stores; any n >= 1.
// Included by lmpc_capi.hip only.
#pragma once
#include <hip/hip_runtime.h>

#define LMPC_LIVE_NT 1024
#define LMPC_LIVE_FINISHED 1u                  // == LMPC_PARK_FINISHED (include/lmpc_hip.h)

struct lmpc_live_args {
    int n, t; unsigned mode; int force;
    const int *doneAt, *parked0;               // n each; parked0 may be null (no start list)
    int *parkedAt, *live, *hdr;                // n, n, 3
};

__global__ __launch_bounds__(LMPC_LIVE_NT) void lmpc_rollout_live_kernel(lmpc_live_args a) {
    __shared__ int wtot[LMPC_LIVE_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nd = a.hdr[0];
    if (!a.force && nd == a.hdr[2]) return;                                   // (uniform over the work-group; hdr[2] is written only behind the barriers below)
    int carry = 0;
    for (int base = 0; base < a.n; base += LMPC_LIVE_NT) {
        const int b = base + tid;
        bool lv = false;
        if (b < a.n) {
            const int pa = a.parkedAt[b];
            const bool parked = pa >= 0 || (a.parked0 && a.parked0[b] != 0) || ((a.mode & LMPC_LIVE_FINISHED) && a.doneAt[b] >= 0);
            if (parked && pa < 0) a.parkedAt[b] = a.t;
            lv = !parked;
        }
        const unsigned long long m = __ballot(lv);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(m);
        __syncthreads();
        int off = carry, tot = 0;
        for (int w = 0; w < LMPC_LIVE_NT / 64; w++) { const int cnt = wtot[w]; off += w < wave ? cnt : 0; tot += cnt; }
        if (lv) a.live[off + rank] = b;                                       // (off + rank < number of live cars <= n)
        carry += tot;
        __syncthreads();                                                      // wtot is written again by the next chunk
    }
    if (tid == 0) { a.hdr[1] = carry; a.hdr[2] = nd; }
}
