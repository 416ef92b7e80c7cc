// racinglmpc_amd/csrc/lmpc_relaunch.hip.h -- the lap change inside a running session (lmpc_rollout_relaunch): a car that has crossed the line is put, on the device,
// into the state a fresh lmpc_rollout_begin would give it for its next lap, while the other cars of the session keep driving.  The reference runs one car, whose next
// lap begins at the step after its crossing, from xF (main.py:100-121, SysModel.py:50).
//   lmpc_rollout_relaunch_kernel     one 256-thread work-group per listed car: start state, linearisation trajectories from the car's own logged rows, every
//                                    per-problem array of the step zeroed, the finish-line books reset, the car's lap-table row replaced, its noise rows redrawn.
//   lmpc_rollout_shift_lap_kernel    the twin of lmpc_rollout_shift_kernel a session launches once it has relaunched: timeStep counts the steps of the car's LAP,
//                                    t + 1 - lapStart[b] (the Q-function shift of the selection reads it, lmpc_solve_common.hip.h).
// Nothing here is compute-heavy: what counts is that a lap change costs one launch for all listed cars, no download of the lap and no memset per array and car.
// Included by lmpc_capi.hip only, after the kernels' header (lmpc_rollout_state, LMPC_SHIFT_TPR) and lmpc_noise.hip.h (the draws).
#pragma once
#include <hip/hip_runtime.h>

#define LMPC_RELAUNCH_NT 256
#define LMPC_RELAUNCH_MAX_SPANS 40                                       // per-problem arrays a session can hold (lmpc_arrays.h lists 29; the host checks the count)

struct lmpc_relaunch_span { unsigned *p; unsigned words, pad; };        // one per-problem array of the session: problem b owns 32-bit words [b words, (b + 1) words)
struct lmpc_relaunch_entry { int car, s0, lap, pad; double TL; };       // s0: the session row the lap now ending began at; lap: the car's lap number from now on; TL: its own TrackLength
struct lmpc_relaunch_args {
    int B, N, t, T_max;                                                 // t: steps the session has taken = the first row of the new lap
    int lap_rows, n_spans, lt_stride, dev_noise;                        // lt_stride: ints per lap-table row (0: the session has no table); dev_noise: the session draws on the device
    unsigned long long seed, lap0, car0;                                // the session's snapshot of the noise source
    double *x, *xg, *xLin, *uLin, *zt, *finX, *finG, *noise;
    const double *logX, *logU;
    int *doneAt, *statusAcc, *nDone, *lapStart, *lt;
    lmpc_relaunch_span span[LMPC_RELAUNCH_MAX_SPANS];
};

// What rollout_setup does at init_state, for the car of this work-group alone.  Bounds (all checked by the host before the launch): car < B; the lap has at least
// N + 2 rows, so the rows s0 + 1 .. s0 + N + 1 read below were logged; noise rows stop at T_max.
__global__ void __launch_bounds__(LMPC_RELAUNCH_NT) lmpc_rollout_relaunch_kernel(lmpc_relaunch_args a, const lmpc_relaunch_entry *__restrict__ table, const int *__restrict__ ltRows) {
#pragma clang fp contract(off)
    const lmpc_relaunch_entry e = table[blockIdx.x];
    const int tid = threadIdx.x, N = a.N;
    const size_t b = (size_t)e.car, B = (size_t)a.B;
    // the crossing state, read before it is zeroed: x = finX with the car's own TrackLength taken off s (xF, SysModel.py:50: one FP64 subtraction), xg = finG
    double keep = 0.0;
    if (tid < 6) keep = a.finX[b * 6 + tid]; else if (tid < 12) keep = a.finG[b * 6 + (tid - 6)];
    if (tid == 4) keep = keep - e.TL;
    // every per-problem array of the step, by the table of lmpc_arrays.h: hasPred, timeStep, the solver's outputs and status words among them
    for (int k = 0; k < a.n_spans; k++) {
        const unsigned words = a.span[k].words;
        unsigned *p = a.span[k].p + b * (size_t)words;
        for (unsigned i = tid; i < words; i += LMPC_RELAUNCH_NT) p[i] = 0u;
    }
    __syncthreads();                                                    // (x0, zt, xLin and uLin are among the arrays zeroed above and are written below by other threads)
    if (tid < 6) { a.x[b * 6 + tid] = keep; a.finX[b * 6 + tid] = 0.0; a.zt[b * 6 + tid] = tid == 4 ? 10.0 : 0.0; }      // zt: LMPC.__init__ :330
    else if (tid < 12) { a.xg[b * 6 + (tid - 6)] = keep; a.finG[b * 6 + (tid - 6)] = 0.0; }
    // xLin = logged X rows s0 + 1 .. s0 + N + 1, uLin = logged U rows s0 + 1 .. s0 + N of this car (LMPC.addTrajectory :431-433)
    for (int i = tid; i < (N + 1) * 6; i += LMPC_RELAUNCH_NT) {
        const int row = i / 6, col = i - row * 6;
        a.xLin[b * (size_t)(N + 1) * 6 + i] = a.logX[((size_t)(e.s0 + 1 + row) * B + b) * 6 + col];
    }
    for (int i = tid; i < N * 2; i += LMPC_RELAUNCH_NT) {
        const int row = i >> 1, col = i & 1;
        a.uLin[b * (size_t)N * 2 + i] = a.logU[((size_t)(e.s0 + 1 + row) * B + b) * 2 + col];
    }
    if (tid == 0) { a.doneAt[b] = -1; a.statusAcc[b] = 0; a.lapStart[b] = a.t; atomicAdd(a.nDone, -1); }
    for (int i = tid; i < a.lt_stride; i += LMPC_RELAUNCH_NT) a.lt[b * (size_t)a.lt_stride + i] = ltRows[(size_t)blockIdx.x * a.lt_stride + i];
    // the plant noise of the new lap: rows [t, min(T_max, t + lap_rows)) of this car's column hold the draws (seed, stream 0, lap0 + lap, step of the lap, car0 + car)
    // -- what a fresh session of that lap number holds in rows 0 .. (lmpc_noise_fill_kernel, the same device functions)
    if (a.dev_noise) {
        const int rows = min(a.lap_rows, a.T_max - a.t);
        for (int k = tid; k < rows; k += LMPC_RELAUNCH_NT) {
            const lmpc_philox_words w = lmpc_noise_words(a.seed, 0ull, a.lap0 + (unsigned long long)e.lap, (unsigned long long)k, a.car0 + (unsigned long long)b);
            double z0, z1, z2, z3;
            lmpc_box_muller(w.w[0], w.w[1], z0, z1);
            lmpc_box_muller(w.w[2], w.w[3], z2, z3);
            double *o = a.noise + ((size_t)(a.t + k) * B + b) * 3;
            o[0] = z0; o[1] = z1; o[2] = z2;
        }
    }
}

// lmpc_rollout_shift_kernel with the one difference named above (a kernel of its own, the text once more, for the reason given at lmpc_rollout_shift_live_kernel:
// the plain kernel is what every session that never relaunches runs, and it keeps its machine code).
__global__ __launch_bounds__(256) void lmpc_rollout_shift_lap_kernel(lmpc_dev_params p, int B, int t, lmpc_rollout_state r, const int *__restrict__ lapStart) {
    const int N = p.N, tpr = LMPC_SHIFT_TPR(N);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, b = tid / tpr, e = tid - b * tpr;
    if (b >= B) return;
    const int row = e >> 3, col = e & 7;
    const double *uP = r.uPred + (size_t)b * N * 2, *xP = r.xPred + (size_t)b * (N + 1) * 6;
    double *xl = r.xLin + (size_t)b * (N + 1) * 6, *ul = r.uLin + (size_t)b * N * 2, *xpp = r.xPP + (size_t)b * (N + 1) * 6;
    if (col < 6) {
        const double v = xP[row * 6 + col];
        xpp[row * 6 + col] = v;
        if (row >= 1) xl[(row - 1) * 6 + col] = v;
        if (row == N) { const double z = r.ztNext[(size_t)b * 6 + col]; xl[N * 6 + col] = z; r.zt[(size_t)b * 6 + col] = z; }
    } else {
        const int c = col - 6;
        if (row >= 1 && row < N) ul[(row - 1) * 2 + c] = uP[row * 2 + c];
        if (row == N) ul[(N - 1) * 2 + c] = r.ztuNext[(size_t)b * 2 + c];
        if (row == 0) r.uOld[(size_t)b * 2 + c] = uP[c];
    }
    if (e == 0) { r.hasPred[b] = 1; r.timeStep[b] = t + 1 - lapStart[b]; }
}
