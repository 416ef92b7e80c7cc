// racinglmpc_amd/csrc/lmpc_trace.hip.h -- session traces: what the controller of a listed car computed at one simulated step, copied from the step's output
// buffers (which the next solve overwrites) into planes that stay for the session.  The three per-step logs LMPC.unpackSolution appends in the reference
// (PredictiveControllers.py:364-379: xStoredPredTraj, uStoredPredTraj, SSStoredPredTraj), the Q-values of the selected points (Qfun_SelectedTot, :404-412), the
// solver's iteration count and status word of the step, and the inertial (X, Y) of the predicted and selected points (Map.getGlobalPosition, Track.py:135-189: what
// plot.py:106-175 computes per point on the host).  Included by lmpc_capi.hip only, behind lmpc_kernels.hip.h (global_position_point, the track sources).
//
// One launch per simulated step of a traced session, one work-group per listed car.  Thread e moves element e of the car's row xPred | uPred | ssSel | qSel | iters,
// status: neighbouring lanes read and write neighbouring doubles (a divergent branch only where a wave straddles two planes).  For XY one thread per point, the
// N + 1 prediction rows and then the S selected points.  No LDS, no barrier: a point on no segment ORs its bit into the row's mapStatus word, which the session zeroes
// when it begins.
#pragma once
#include <hip/hip_runtime.h>

#define LMPC_TRACE_NT 256                      // threads per work-group: a row of the reference configuration (N = 12, S = 48) is 440 elements, two passes

struct lmpc_trace_args {
    const int *cars; int n, N, S;                                             // the listed cars (device), their count, horizon, safe-set points in use
    const double *xPred, *uPred, *ssSel, *qSel; const int *iters, *status;    // the step's outputs for all B cars (lmpc_arrays.h layouts)
    double *oX, *oU, *oSS, *oQ, *oXY, *oXYS; int *oIt, *oSt, *oMap;           // the planes, [T_max][n][...]; null: not recorded
    const double *trk; int trkStride;                                         // the session's track image (TRK kernels only)
};

// TRK: car cars[k] maps its points on its own track row (lmpc_track_set), as the plant kernels integrate it there.
// PARKED: empty, or (a parking session, lmpc_live.hip.h) one `const int *parkedAt` over all B cars -- a listed car with parkedAt >= 0 returns at once: its outputs are no
// longer written, and its planes keep what they held.  Empty, the kernel is the one it was (signature, argument layout, text).
template <bool TRK, class... PARKED>
__global__ __launch_bounds__(LMPC_TRACE_NT) void lmpc_rollout_trace_kernel(lmpc_dev_params p_, int t, lmpc_trace_args a, PARKED... parkedAt) {
    const int k = blockIdx.x;
    const size_t b = (size_t)a.cars[k], row = (size_t)t * (size_t)a.n + (size_t)k;
    if constexpr (sizeof...(PARKED) > 0) { if ((parkedAt[b], ...) >= 0) return; }
    const int nx = (a.N + 1) * 6, nu = a.N * 2, ns = a.S * 6, nq = a.S;
    const int e1 = a.oX ? nx : 0, e2 = e1 + (a.oU ? nu : 0), e3 = e2 + (a.oSS ? ns : 0), e4 = e3 + (a.oQ ? nq : 0), e5 = e4 + (a.oIt ? 2 : 0);
    for (int e = threadIdx.x; e < e5; e += LMPC_TRACE_NT) {
        if (e < e1) a.oX[row * nx + e] = a.xPred[b * nx + e];
        else if (e < e2) a.oU[row * nu + (e - e1)] = a.uPred[b * nu + (e - e1)];
        else if (e < e3) a.oSS[row * ns + (e - e2)] = a.ssSel[b * ns + (e - e2)];
        else if (e < e4) a.oQ[row * nq + (e - e3)] = a.qSel[b * nq + (e - e3)];
        else if (e == e4) a.oIt[row] = a.iters[b];
        else a.oSt[row] = a.status[b];
    }
    if (!a.oXY) return;
    lmpc_track_row tr_ = {nullptr, 0, 0.0}; if constexpr (TRK) tr_ = track_row_at(a.trk, (size_t)a.trkStride, b);
    const auto &tk = track_src<TRK>(p_, tr_);
    const int np = a.N + 1, npts = np + (a.oXYS ? a.S : 0);
    for (int e = threadIdx.x; e < npts; e += LMPC_TRACE_NT) {
        const double *src = e < np ? a.xPred + b * nx + (size_t)e * 6 : a.ssSel + b * ns + (size_t)(e - np) * 6;       // (s, ey): columns 4, 5 of a state row
        double *dst = e < np ? a.oXY + (row * np + e) * 2 : a.oXYS + (row * a.S + (e - np)) * 2;
        double x, y;
        const bool on = global_position_point(tk, src[4], src[5], x, y);
        dst[0] = x; dst[1] = y;
        if (!on) atomicOr(a.oMap + row, LMPC_ST_NO_SEGMENT);
    }
}
