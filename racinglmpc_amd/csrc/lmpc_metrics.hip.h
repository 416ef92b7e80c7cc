// racinglmpc_amd/csrc/lmpc_metrics.hip.h -- lap metrics of a rollout session: per listed car, the reductions over its log rows that a sweep wants back instead of the
// logs (lmpc_rollout_lap_metrics; the columns LMPC_MET_* are defined in include/lmpc_hip.h).  A reader: nothing of the session or the stores is written.
// The source is a session's logs as they are: logX (T x B x 6), logU (T x B x 2), logG (T x B x 6), row t of car b at log[(t * B + b) * width], and finX (B x 6), the
// state right after the crossing step (SysModel.py:45).  One 256-thread work-group per entry, the shape of the commit kernels (lmpc_commit.hip.h); no atomics, no
// scratch; a row's 48 + 16 + 48 bytes are fetched as seven 16-byte loads (every row starts on a multiple of 16 bytes).
//
// THE ORDER CONTRACT.  A result is reproducible on the host (tests/metrics_ref.py restates this file in NumPy), the standard the prefilter image is held to: every
// operation below is rounded on its own (no contraction into FMAs) and happens in the order written here.
//   Terms of row t (x = logX row, u = logU row, (X, Y) = logG row [4:6]; Q, R, xRef, bx, bu: the entry's weights row; Fx, Fu: the context's):
//     bad        = some of the 14 logged values is not finite
//     alat       = |x0 * x2|
//     f_r        = ((((Fx[r][0] x0 + Fx[r][1] x1) + Fx[r][2] x2) + Fx[r][3] x3) + Fx[r][4] x4) + Fx[r][5] x5,  d_r = f_r - bx_r,  v_r = d_r < 0 ? 0 : d_r   (r = 0, 1: a NaN stays)
//     le_sum     = v_0 + v_1,  le_sq = v_0 v_0 + v_1 v_1,  le_row = v_0 > 0 or v_1 > 0,  le_max = first-max(first-max(-inf, v_0), v_1)
//     margin     = first-min over r = 0, 1, 2, 3 in this order, from +inf, of bu_r - (Fu[r][0] u0 + Fu[r][1] u1)
//     du_j       = (u_j - u_j of row t-1)^2, 0 at t = 0;  path = sqrt(dX dX + dY dY) with dX = X - X of row t-1, dY likewise, 0 at t = 0
//     cost_state = sum over i = 0..5 ascending, from the i = 0 product, of e_i * (sum over j = 0..5 ascending, from the j = 0 product, of Q[i][j] e_j),  e = x - xRef
//                  (the 36 products Q[i][j] e_j, row by row; buildCost's x' Q x about xRef, PredictiveControllers.py:228-257)
//     cost_input = u0 * (R[0][0] u0 + R[0][1] u1) + u1 * (R[1][0] u0 + R[1][1] u1)
//   Combination of two partial results `left`, `right` (met_combine; a row's terms are a partial result, the identity is: sums +0.0, counts 0, maxima -inf,
//   minima +inf, argmax row -1):
//     sums left + right; counts added; minima / maxima by commit_first_min / commit_first_max (lmpc_commit.hip.h: the left one stays among equals, a comparison
//     with NaN is false, so a NaN is skipped and an entry without a comparable value keeps the identity); ey_absmax travels with its row and `right` replaces `left`
//     when left < right, or when they are equal and right's row is the lower one -- the FIRST row that attains the maximum, whatever the order.
//   Reduction order, a function of T alone: thread k folds rows k, k + 256, k + 512, .. (< T) in ascending order into the identity, each as `right`; within a
//   wave lanes combine at offsets 1, 2, 4, 8, 16, 32, lane l (left) with lane l + offset (right) while l + offset < 64; thread 0 then folds the results of waves
//   1, 2, 3, in this order, as `right` into that of wave 0.
//   t_cross = (double)(T - 1) + (TL - s) / (finX_s - s), s = x4 of row T - 1 (the crossing, SysModel.py:45, interpolated between the last logged row and finX), for an
//   entry that ends at the car's crossing step; else the quiet NaN 0x7ff8000000000000.
// Included by lmpc_capi.hip only, after lmpc_commit.hip.h (commit_first_min / commit_first_max).
#pragma once
#include <hip/hip_runtime.h>

#define LMPC_MET_NT 256
static_assert(LMPC_MET_NT % 64 == 0, "whole waves");

struct lmpc_metrics_weights { double Q[36], R[4], xRef[6], bx[2], bu[4]; };     // of one tuning row (lmpc_tuning_set), or of the config
struct lmpc_metrics_entry { int car, rows, cross, wrow; double TL; };             // cross: rows == doneAt[car] (t_cross exists); wrow: the entry's row of the weights table
struct lmpc_metrics_args {
    const double *logX, *logU, *logG, *finX; int B;                               // the session
    const lmpc_metrics_weights *weights; const lmpc_metrics_entry *table;        // uploaded by the call, one copy
    double Fx[12], Fu[8];
};

enum { MS_VX = 0, MS_LE, MS_LE2, MS_DU0, MS_DU1, MS_CX, MS_CU, MS_PATH, MS_N };  // the sums
enum { MH_VX = 0, MH_EPSI, MH_ALAT, MH_LE, MH_N };                               // the maxima without a row
enum { ML_VX = 0, ML_MARGIN, ML_N };                                             // the minima
struct met_part { double sum[MS_N], hi[MH_N], lo[ML_N], ey; int ey_row, bad, le_rows; };

__device__ __forceinline__ met_part met_identity() {
    met_part p;
#pragma unroll
    for (int k = 0; k < MS_N; k++) p.sum[k] = 0.0;
#pragma unroll
    for (int k = 0; k < MH_N; k++) p.hi[k] = -INFINITY;
#pragma unroll
    for (int k = 0; k < ML_N; k++) p.lo[k] = INFINITY;
    p.ey = -INFINITY; p.ey_row = -1; p.bad = 0; p.le_rows = 0;
    return p;
}
__device__ __forceinline__ void met_combine(met_part &l, const met_part &r) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < MS_N; k++) l.sum[k] = l.sum[k] + r.sum[k];
#pragma unroll
    for (int k = 0; k < MH_N; k++) l.hi[k] = commit_first_max(l.hi[k], r.hi[k]);
#pragma unroll
    for (int k = 0; k < ML_N; k++) l.lo[k] = commit_first_min(l.lo[k], r.lo[k]);
    if (l.ey < r.ey || (l.ey == r.ey && r.ey_row < l.ey_row)) { l.ey = r.ey; l.ey_row = r.ey_row; }
    l.bad += r.bad; l.le_rows += r.le_rows;
}

// the terms of row t of car `car`, in the order of the header
__device__ __forceinline__ met_part met_row(const lmpc_metrics_args &a, const lmpc_metrics_weights &w, int car, int t) {
#pragma clang fp contract(off)
    const size_t row = (size_t)t * a.B + car;
    const double2 *px = (const double2 *)(a.logX + row * 6), *pg = (const double2 *)(a.logG + row * 6);
    const double2 x01 = px[0], x23 = px[1], x45 = px[2], uu = *(const double2 *)(a.logU + row * 2), g01 = pg[0], g23 = pg[1], g45 = pg[2];
    const double x[6] = {x01.x, x01.y, x23.x, x23.y, x45.x, x45.y}, u[2] = {uu.x, uu.y};
    met_part p = met_identity();
    bool fin = __builtin_isfinite(g01.x) && __builtin_isfinite(g01.y) && __builtin_isfinite(g23.x) && __builtin_isfinite(g23.y) && __builtin_isfinite(g45.x) && __builtin_isfinite(g45.y) &&
               __builtin_isfinite(u[0]) && __builtin_isfinite(u[1]);
#pragma unroll
    for (int j = 0; j < 6; j++) fin = fin && __builtin_isfinite(x[j]);
    p.bad = fin ? 0 : 1;
    p.sum[MS_VX] = x[0]; p.hi[MH_VX] = commit_first_max(p.hi[MH_VX], x[0]); p.lo[ML_VX] = commit_first_min(p.lo[ML_VX], x[0]);
    const double aey = fabs(x[5]);
    if (p.ey < aey) { p.ey = aey; p.ey_row = t; }
    p.hi[MH_EPSI] = commit_first_max(p.hi[MH_EPSI], fabs(x[3]));
    p.hi[MH_ALAT] = commit_first_max(p.hi[MH_ALAT], fabs(x[0] * x[2]));
    double v[2];
#pragma unroll
    for (int r = 0; r < 2; r++) {
        double f = a.Fx[r * 6] * x[0];
#pragma unroll
        for (int c = 1; c < 6; c++) f = f + a.Fx[r * 6 + c] * x[c];
        const double d = f - w.bx[r];
        v[r] = d < 0.0 ? 0.0 : d;
        p.hi[MH_LE] = commit_first_max(p.hi[MH_LE], v[r]);
    }
    p.sum[MS_LE] = v[0] + v[1]; p.sum[MS_LE2] = v[0] * v[0] + v[1] * v[1];
    p.le_rows = (v[0] > 0.0 || v[1] > 0.0) ? 1 : 0;
#pragma unroll
    for (int r = 0; r < 4; r++) p.lo[ML_MARGIN] = commit_first_min(p.lo[ML_MARGIN], w.bu[r] - (a.Fu[r * 2] * u[0] + a.Fu[r * 2 + 1] * u[1]));
    if (t > 0) {
        const size_t prev = row - (size_t)a.B;
        const double2 up = *(const double2 *)(a.logU + prev * 2), gp = ((const double2 *)(a.logG + prev * 6))[2];
        const double d0 = u[0] - up.x, d1 = u[1] - up.y, dX = g45.x - gp.x, dY = g45.y - gp.y;
        p.sum[MS_DU0] = d0 * d0; p.sum[MS_DU1] = d1 * d1; p.sum[MS_PATH] = sqrt(dX * dX + dY * dY);
    }
    double e[6], cx = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) e[i] = x[i] - w.xRef[i];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double q = w.Q[i * 6] * e[0];
#pragma unroll
        for (int j = 1; j < 6; j++) q = q + w.Q[i * 6 + j] * e[j];
        cx = i == 0 ? e[0] * q : cx + e[i] * q;
    }
    p.sum[MS_CX] = cx;
    p.sum[MS_CU] = u[0] * (w.R[0] * u[0] + w.R[1] * u[1]) + u[1] * (w.R[2] * u[0] + w.R[3] * u[1]);
    return p;
}

__device__ __forceinline__ met_part met_shfl_down(const met_part &p, int off) {
    met_part o;
#pragma unroll
    for (int k = 0; k < MS_N; k++) o.sum[k] = __shfl_down(p.sum[k], off, 64);
#pragma unroll
    for (int k = 0; k < MH_N; k++) o.hi[k] = __shfl_down(p.hi[k], off, 64);
#pragma unroll
    for (int k = 0; k < ML_N; k++) o.lo[k] = __shfl_down(p.lo[k], off, 64);
    o.ey = __shfl_down(p.ey, off, 64); o.ey_row = __shfl_down(p.ey_row, off, 64); o.bad = __shfl_down(p.bad, off, 64); o.le_rows = __shfl_down(p.le_rows, off, 64);
    return o;
}

// out: n x LMPC_METRICS_NCOL, row blockIdx.x written whole by thread 0
__global__ void __launch_bounds__(LMPC_MET_NT) lmpc_lap_metrics_kernel(lmpc_metrics_args a, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ met_part red[LMPC_MET_NT / 64];
    const lmpc_metrics_entry e = a.table[blockIdx.x];
    const lmpc_metrics_weights &w = a.weights[e.wrow];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = e.rows;
    met_part p = met_identity();
    for (int t = tid; t < T; t += LMPC_MET_NT) met_combine(p, met_row(a, w, e.car, t));
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const met_part o = met_shfl_down(p, off);
        if (lane + off < 64) met_combine(p, o);
    }
    if (lane == 0) red[wave] = p;
    __syncthreads();
    if (tid != 0) return;
    for (int k = 1; k < LMPC_MET_NT / 64; k++) met_combine(p, red[k]);
    double *o = out + (size_t)blockIdx.x * LMPC_METRICS_NCOL;
    double t_cross = __builtin_nan("");
    if (e.cross) { const double s = a.logX[((size_t)(T - 1) * a.B + e.car) * 6 + 4]; t_cross = (double)(T - 1) + (e.TL - s) / (a.finX[(size_t)e.car * 6 + 4] - s); }
    o[LMPC_MET_ROWS] = (double)T; o[LMPC_MET_T_CROSS] = t_cross; o[LMPC_MET_NONFINITE_ROWS] = (double)p.bad;
    o[LMPC_MET_VX_MIN] = p.lo[ML_VX]; o[LMPC_MET_VX_MAX] = p.hi[MH_VX]; o[LMPC_MET_VX_SUM] = p.sum[MS_VX];
    o[LMPC_MET_EY_ABSMAX] = p.ey; o[LMPC_MET_EY_ABSMAX_ROW] = (double)p.ey_row;
    o[LMPC_MET_EPSI_ABSMAX] = p.hi[MH_EPSI]; o[LMPC_MET_ALAT_ABSMAX] = p.hi[MH_ALAT];
    o[LMPC_MET_LANE_EXCESS_MAX] = p.hi[MH_LE]; o[LMPC_MET_LANE_EXCESS_ROWS] = (double)p.le_rows;
    o[LMPC_MET_LANE_EXCESS_SUM] = p.sum[MS_LE]; o[LMPC_MET_LANE_EXCESS_SQSUM] = p.sum[MS_LE2];
    o[LMPC_MET_INPUT_MARGIN_MIN] = p.lo[ML_MARGIN];
    o[LMPC_MET_DU0_SQSUM] = p.sum[MS_DU0]; o[LMPC_MET_DU1_SQSUM] = p.sum[MS_DU1];
    o[LMPC_MET_COST_STATE] = p.sum[MS_CX]; o[LMPC_MET_COST_INPUT] = p.sum[MS_CU];
    o[LMPC_MET_PATH_LENGTH] = p.sum[MS_PATH];
}
