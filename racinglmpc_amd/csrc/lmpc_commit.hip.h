// racinglmpc_amd/csrc/lmpc_commit.hip.h -- the writer of the two lap stores ([lap][column][row], row stride max_lap_len): every lap and every batch of appended rows, from
// a rollout session's logs or from the host, enters the stores through the two kernels below, and the rules of what a stored lap holds are stated here only.
// A source is a log: logX (T x B x 6) and logU (T x B x 2), row t of car b at log[(t * B + b) * width] -- a session's logs as they are, or one lap handed in by the
// host (T x 6, T x 2, row-major: B = 1, car 0) staged on the device.
//   lmpc_commit_laps_kernel   whole laps: the transposed copy of rows [0, T) into the safe set and / or the regression store, the Q-function of the safe-set lap
//                             (LMPC.computeCost, PredictiveControllers.py:447-464) and the K1 prefilter image of the regression-store lap (the scan it serves:
//                             PredictiveModel.py:180-197).
//   lmpc_extend_laps_kernel   rows appended to safe-set laps: the batched LMPC.addPoint (PredictiveControllers.py:466-474).
// Both are one 256-thread work-group per lap: nothing here is compute-heavy, what counts is that a lap costs one launch and no per-column copy.
// Included by lmpc_capi.hip only, after the kernels' header (K1_CHUNK, LMPC_COLS).
#pragma once
#include <hip/hip_runtime.h>

#define LMPC_COMMIT_NT 256
#define LMPC_COMMIT_RPT (K1_CHUNK / LMPC_COMMIT_NT)      // rows of one prefilter chunk per thread, CONSECUTIVE ones (see commit_first_min)
static_assert(K1_CHUNK % LMPC_COMMIT_NT == 0 && LMPC_COMMIT_NT % 64 == 0, "one prefilter chunk is a whole number of rows per thread");

struct lmpc_commit_entry { int car, rows, ss_slot, m_slot; double TL; };   // slots: -1 = that store is not written; TL: the trackLength computeCost compares s with -- the
                                                                        // entry's own, since cars may be on different tracks (lmpc_track_set) and a host lap is "car 0" of a one-car source
struct lmpc_commit_args {
    const double *logX, *logU; int B;                                   // the source
    double *sstore, *mstore; unsigned *mquant; double *mqpar;           // the stores and the prefilter image (lmpc_ctx)
    int ls, mq_chunks;                                                  // row stride of every column (max_lap_len); chunks the image holds per lap
    double scaling[5];
};
struct lmpc_extend_entry { int car, lap, row0, pad; double TL; };      // row0: rows the lap holds now (the first appended row); TL: the trackLength added to s (:472), the entry's own

// The minimum / maximum of a feature over a chunk is the one a scan in row order finds when it replaces its value only by a strictly smaller / larger one: among equals
// (+0.0 and -0.0 compare equal) the value met FIRST stays, which defines the sign of a zero minimum.  "Keep the left one on a tie" is associative, so a reduction
// that combines neighbours in row order gives the bits of that sequential scan.
__device__ __forceinline__ double commit_first_min(double left, double right) { return right < left ? right : left; }
__device__ __forceinline__ double commit_first_max(double left, double right) { return left < right ? right : left; }

// lo[k] / hi[k] of this thread's rows -> of the whole group, in row order: lanes hold consecutive rows, so the tree takes offsets 1, 2, .. 32 (the left operand is
// always the lower lane), then the four waves are combined in their order by every thread.
__device__ __forceinline__ void commit_reduce_minmax(double (&lo)[5], double (&hi)[5], double (*red)[10]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; k++) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double ol = __shfl_down(lo[k], off, 64), oh = __shfl_down(hi[k], off, 64);
            if (lane + off < 64) { lo[k] = commit_first_min(lo[k], ol); hi[k] = commit_first_max(hi[k], oh); }
        }
    }
    __syncthreads();                                                    // (the previous chunk's readers are done with `red`)
    if (lane == 0) for (int k = 0; k < 5; k++) { red[wave][k] = lo[k]; red[wave][5 + k] = hi[k]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; k++) {
        double l = red[0][k], h = red[0][5 + k];
        for (int w = 1; w < LMPC_COMMIT_NT / 64; w++) { l = commit_first_min(l, red[w][k]); h = commit_first_max(h, red[w][5 + k]); }
        lo[k] = l; hi[k] = h;
    }
}

// The prefilter image of rows 0 .. T-2 of one lap (the regression reads row t with row t + 1, so the last row is no candidate), per chunk of K1_CHUNK rows.  Feature k of
// (vx, vy, wz, delta, a) is scaled by scaling[k]; lo_k / hi_k are its extremes over the chunk's finite values (0 / 0 when there is none); the chunk's one scale is
// sc = 65535 / W, W the widest hi_k - lo_k, each range taken no smaller than 1e-9 max(|lo_k|, |hi_k|) (a constant feature) and W no smaller than 1e-300 (all zero).
// A row's 16-bit word is (feature - lo_k) * sc clamped to [0, 65535] and truncated, 0 when not finite; words are packed (vx | vy << 16), (wz | delta << 16), (a), and
// the chunk's parameters are (lo_0 .. lo_4, sc).  The regression kernel ranks rows by integer L1 distances on this image and re-evaluates the survivors in FP64, so the
// image decides nothing by itself -- but it is part of what a context computes bit for bit, hence every operation is rounded on its own (no contraction).
__device__ __forceinline__ void commit_quantise(const lmpc_commit_args &a, int car, int T, int slot, double (*red)[10]) {
#pragma clang fp contract(off)
    const int nrows = T - 1, tid = threadIdx.x;
    unsigned *q = a.mquant + (size_t)slot * 3 * a.ls;
    double *par = a.mqpar + (size_t)slot * a.mq_chunks * 6;
    for (int t0 = 0, ch = 0; t0 < nrows; t0 += K1_CHUNK, ch++) {
        double f[LMPC_COMMIT_RPT][5], lo[5], hi[5];
#pragma unroll
        for (int k = 0; k < 5; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
#pragma unroll
        for (int i = 0; i < LMPC_COMMIT_RPT; i++) {
            const int t = t0 + tid * LMPC_COMMIT_RPT + i;
            if (t < nrows) {
                const double *x = a.logX + ((size_t)t * a.B + car) * 6, *u = a.logU + ((size_t)t * a.B + car) * 2;
#pragma unroll
                for (int k = 0; k < 5; k++) {
                    const double v = (k < 3 ? x[k] : u[k - 3]) * a.scaling[k];
                    f[i][k] = v;
                    if (__builtin_isfinite(v)) { lo[k] = commit_first_min(lo[k], v); hi[k] = commit_first_max(hi[k], v); }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 5; k++) f[i][k] = 0.0;
            }
        }
        commit_reduce_minmax(lo, hi, red);
        double rmax = 0.0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            if (!(lo[k] <= hi[k])) { lo[k] = 0.0; hi[k] = 0.0; }       // (no finite value of this feature in the chunk)
            const double al = fabs(lo[k]), ah = fabs(hi[k]);
            const double fl = 1e-9 * (al < ah ? ah : al), rg = hi[k] - lo[k];
            const double w = rg < fl ? fl : rg;
            rmax = rmax < w ? w : rmax;
        }
        const double sc = 65535.0 / (rmax < 1e-300 ? 1e-300 : rmax);
        if (tid < 5) par[(size_t)ch * 6 + tid] = lo[tid];
        if (tid == 5) par[(size_t)ch * 6 + 5] = sc;
#pragma unroll
        for (int i = 0; i < LMPC_COMMIT_RPT; i++) {
            const int t = t0 + tid * LMPC_COMMIT_RPT + i;
            if (t >= nrows) continue;
            unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const double v = (f[i][k] - lo[k]) * sc;
                unsigned qq = 0u;
                if (__builtin_isfinite(v)) { const double c0 = v < 0.0 ? 0.0 : v; qq = (unsigned)(65535.0 < c0 ? 65535.0 : c0); }
                w[k >> 1] |= (k & 1) ? qq << 16 : qq;
            }
            q[t] = w[0]; q[(size_t)a.ls + t] = w[1]; q[2 * (size_t)a.ls + t] = w[2];
        }
    }
    // a lap's image is written whole: zeros behind row T-2 of the three planes and in the parameters of the chunks not used (a replaced lap leaves nothing behind)
    for (int e = tid; e < 3 * (a.ls - nrows); e += LMPC_COMMIT_NT) { const int pl = e / (a.ls - nrows), t = nrows + e % (a.ls - nrows); q[(size_t)pl * a.ls + t] = 0u; }
    const int used = (nrows + K1_CHUNK - 1) / K1_CHUNK;
    for (int e = used * 6 + tid; e < a.mq_chunks * 6; e += LMPC_COMMIT_NT) par[e] = 0.0;
}

// LMPC.computeCost (PredictiveControllers.py:447-464): cost[T-1] = 0, backwards cost[r] = cost[r+1] + 1 where s[r] < trackLength, else 0 (a NaN s is not below) -- the
// distance from r to the nearest row r' >= r that is the last one or has !(s < trackLength).  Small integers: exact in any order.  256 rows per pass, from the end of
// the lap; *q0 = cost[0].
__device__ __forceinline__ void commit_cost(const lmpc_commit_args &a, int car, int T, double TL, double *qcol, double *q0, int *nearw) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = T - 1;                                                  // the nearest such row at or behind the end of the pass
    for (int base = ((T - 1) / LMPC_COMMIT_NT) * LMPC_COMMIT_NT; base >= 0; base -= LMPC_COMMIT_NT) {
        const int r = base + tid;
        int idx = 0x7fffffff;
        if (r < T && (r == T - 1 || !(a.logX[((size_t)r * a.B + car) * 6 + 4] < TL))) idx = r;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_down(idx, off, 64); if (lane + off < 64) idx = min(idx, o); }     // suffix minimum within the wave
        __syncthreads();
        if (lane == 0) nearw[wave] = idx;
        __syncthreads();
        for (int w = wave + 1; w < LMPC_COMMIT_NT / 64; w++) idx = min(idx, nearw[w]);
        idx = min(idx, carry);
        if (r < T) { const double cost = (double)(idx - r); qcol[r] = cost; if (r == 0) *q0 = cost; }
        for (int w = 0; w < LMPC_COMMIT_NT / 64; w++) carry = min(carry, nearw[w]);
    }
}

__global__ void __launch_bounds__(LMPC_COMMIT_NT) lmpc_commit_laps_kernel(lmpc_commit_args a, const lmpc_commit_entry *__restrict__ table, double *__restrict__ q0) {
    __shared__ double red[LMPC_COMMIT_NT / 64][10];
    __shared__ int nearw[LMPC_COMMIT_NT / 64];
    const lmpc_commit_entry e = table[blockIdx.x];
    const int tid = threadIdx.x, T = e.rows, ls = a.ls;
    double *sb = e.ss_slot >= 0 ? a.sstore + (size_t)e.ss_slot * LMPC_COLS * ls : nullptr;
    double *mb = e.m_slot >= 0 ? a.mstore + (size_t)e.m_slot * LMPC_COLS * ls : nullptr;
    // columns 0..7: neighbouring lanes write neighbouring rows of a column
    for (int t = tid; t < T; t += LMPC_COMMIT_NT) {
        const double *x = a.logX + ((size_t)t * a.B + e.car) * 6, *u = a.logU + ((size_t)t * a.B + e.car) * 2;
        double v[8];
#pragma unroll
        for (int j = 0; j < 6; j++) v[j] = x[j];
        v[6] = u[0]; v[7] = u[1];
#pragma unroll
        for (int j = 0; j < 8; j++) { if (sb) sb[(size_t)j * ls + t] = v[j]; if (mb) mb[(size_t)j * ls + t] = v[j]; }
    }
    if (sb) commit_cost(a, e.car, T, e.TL, sb + (size_t)8 * ls, q0 + blockIdx.x, nearw);
    if (mb) commit_quantise(a, e.car, T, e.m_slot, red);
}

// One work-group per (car, safe-set lap): rows [0, n_rows) of the car appended at row0 -- s + trackLength (:472), Qfun counting down from qlast by REPEATED subtraction
// of 1.0 (:474 once per row; row i: i + 1 subtractions, each rounded -- a closed form qlast - (i + 1) is another number when qlast is not an integer).  Thread k owns
// rows [k c, (k + 1) c), c = ceil(n_rows / 256): O(n_rows) subtractions per thread.
// flag != NULL (a session's logs, which may hold a diverged car): flag[entry] = every value of the rows is finite, and only then they are appended.
// flag == NULL (rows the host hands in): appended whatever they hold, as LMPC.addPoint does.
__global__ void __launch_bounds__(LMPC_COMMIT_NT) lmpc_extend_laps_kernel(lmpc_commit_args a, int n_rows, const lmpc_extend_entry *__restrict__ table, const double *__restrict__ qlast,
                                                                          int *__restrict__ flag) {
#pragma clang fp contract(off)
    const lmpc_extend_entry e = table[blockIdx.x];
    const int tid = threadIdx.x, ls = a.ls;
    if (flag) {                                                         // (uniform over the grid)
        int ok = 1;
        for (int i = tid; i < n_rows * 8; i += LMPC_COMMIT_NT) {
            const int t = i >> 3, j = i & 7;
            const double v = j < 6 ? a.logX[((size_t)t * a.B + e.car) * 6 + j] : a.logU[((size_t)t * a.B + e.car) * 2 + (j - 6)];
            if (!__builtin_isfinite(v)) ok = 0;
        }
        ok = __syncthreads_and(ok);
        if (tid == 0) flag[blockIdx.x] = ok ? 1 : 0;
        if (!ok) return;
    }
    double *base = a.sstore + (size_t)e.lap * LMPC_COLS * ls + e.row0;
    for (int i = tid; i < n_rows * 8; i += LMPC_COMMIT_NT) {
        const int j = i / n_rows, t = i - j * n_rows;                  // column-major: neighbouring lanes, neighbouring rows
        double v = j < 6 ? a.logX[((size_t)t * a.B + e.car) * 6 + j] : a.logU[((size_t)t * a.B + e.car) * 2 + (j - 6)];
        if (j == 4) v = v + e.TL;
        base[(size_t)j * ls + t] = v;
    }
    const int per = (n_rows + LMPC_COMMIT_NT - 1) / LMPC_COMMIT_NT, t_lo = tid * per, t_hi = min(n_rows, t_lo + per);
    if (t_lo < t_hi) {
        double q = qlast[blockIdx.x];
        for (int t = 0; t < t_lo; t++) q -= 1.0;
        for (int t = t_lo; t < t_hi; t++) { q -= 1.0; base[(size_t)8 * ls + t] = q; }
    }
}
