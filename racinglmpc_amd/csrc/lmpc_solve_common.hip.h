// racinglmpc_amd/csrc/lmpc_solve_common.hip.h -- what the solve-kernel families share around the Newton iteration, once.
//
//   lmpc_solve_kernel     one wave per QP                      (lmpc_kernels.hip.h)
//   lmpc_solve_kernel_mw  two or four waves per QP             (lmpc_solve_mw.hip.h)
//   lmpc_solve_kernel_rt  runtime (N, S), one wave per QP      (lmpc_solve_rt.hip.h)
//   lmpc_solve_kernel_cd  condensed form, one wave per QP      (lmpc_solve_cd.hip.h)
//
// They differ inside the Newton iteration (who owns the recursion, matrix-core tiles against plain multiply-adds, registers against LDS) and solve the same QP
// by the same rules around it.  For all four: the kernels' I/O block lmpc_solve_io, the step rules and the safe-set selection k2_select.  For the runtime and the
// condensed kernel also the parameter block in LDS, the regression status bits and the exit of a selection-only launch, the start of the iteration, the exit
// status and the epilogue (stage_params .. solve_epilogue below: one wave per QP, N and S as arguments -- template constants in the condensed kernel, p.N and
// p.S in the runtime kernel; no function holds a barrier, the callers keep theirs).  lmpc_solve_kernel and lmpc_solve_kernel_mw keep their own text of those
// five blocks: with the calls in its place the compiler lays out and allocates the whole kernel differently -- every instantiation, the Newton iteration
// included -- and the four-wave kernel measured 1.4 % slower on the benchmark (CHANGELOG, "One selection ..."); their machine code is the yardstick, so
// whatever changes in one of these blocks is still written into those two kernels by hand.
//
// Included by lmpc_kernels.hip.h behind the cross-lane primitives and the PAR_* layout it builds on; not a header to include on its own.
#pragma once

// =====================================================================================================
// K2 + K3: safe-set selection + structured primal-dual interior-point QP solve.  One wave per QP.
// Templated on the horizon N and the number of safe-set columns S (0 = plain MPC, no terminal set) so that
// every LDS offset and trip count is a compile-time constant.
// =====================================================================================================
struct lmpc_solve_io {
    // mode bit 0: select the safe set on device (else read ssSel/qSel); bit 1: run the QP solve; bit 2 (one-wave kernel only): fused step --
    // the wave first runs the regression of its own QP from xLin / uLin (rows of N+1 / N points), [A_k | B_k] and C_k never leave LDS
    // (Aout / Bout / Cout, if given, receive a copy)
    int mode;
    const double *A, *Bm, *C, *x0, *uOld, *ssSelIn, *qSelIn;
    const double *xLin, *uLin; double *Aout, *Bout, *Cout;
    const double *zt, *xPredPrev; const int *hasPred, *timeStep;
    const int *rstatus;       // optional per-point status of the regression kernel (B x N): OR-ed into status[b] (the reference raises there)
    double *xPred, *uPred, *slack, *lambda, *sTerm, *mu, *ztNext, *ztuNext;
    double *ssSelOut, *qSelOut, *succOut, *succUOut, *ztUsed, *resid;
    int *selStartOut;         // optional: first row of the 13-row window per selected lap (B x numSS_it)
    int *status, *iters;
    long long *tbuf;          // optional cycle stamps of problem 0 (builds with -DLMPC_TIMING only)
    double *abPack;           // one-wave kernel, long horizons (ABG): global scratch for [A_k | B_k] in the kernel's 6 x 8 layout, 48 N doubles per problem
    int *retry_flag;          // optional (host-mapped): a problem that ends at the iteration limit / breaks down writes retry_epoch here (atomic max, system
    int retry_epoch;          // scope), so that the host launches the retry pass only when one is needed (lmpc_capi.hip: resolve_retries)
    const int *ssTab;         // optional: per-problem safe-set laps (lmpc_ss_set_lap_table), resolved on the host: numSS_it entries of LMPC_SSTAB_ENTRY ints per row --
    int ssTabStride;          // (slot, rows, is the car's latest lap, pad), 16 bytes -- in the row's sorted order; ints between rows (0: one row serves every problem)
    const double *tune;       // optional: per-problem controller tuning (lmpc_tuning_set), the device image of the rows: PAR_TOT doubles per row in the PAR_* layout (doubled
    int tuneStride;           // weights, Fx / Fu of the context) -- what the staging copy of the parameter block reads instead of `p`; doubles between rows (0: one row serves every problem)
    const double *trk;        // optional: per-problem tracks (lmpc_track_set), the device image of the rows (LMPC_TRACK_NPAR doubles each; [1] is the trackLength the selection reads).
    int trkStride;            // Served by the per-problem-rows instantiations (the host sets io.tune with it); doubles between rows (0: one row serves every problem)
};
// Parking: the solve kernels take the live list as a trailing parameter pack BESIDE lmpc_solve_io (lmpc_live_list, lmpc_kernels.hip.h), and lmpc_solve_io keeps its
// layout -- grown by a pointer, the two- and four-wave per-problem-rows kernels came out with other scalar loads and registers although no line of theirs read it.
// With the pack empty a kernel is the kernel it was: its prologue keeps the text it had, the lookup stands behind it under `if constexpr`.
#define LMPC_SSTAB_ENTRY 4
// With a table the selection keeps (slot, rows) of every selected lap for the successor rows of feasibleStateInput, beside sel_start: in LMPC_SSTAB_LDS bytes of
// dynamic LDS behind the kernel's layout, which the launchers add only when io.ssTab is set -- a launch without a table has the footprint it always had.
// The fixed-(N, S) solve kernels are templates on TAB, as the regression kernel is: the TAB = false instantiations, which serve every launch without a table, carry
// none of this; the runtime-(N, S) kernel branches at run time.
// TAB is the ONE "per-problem rows" instantiation: it serves the safe-set table and the tuning rows (io.tune) alike.  Its staging copy always reads io.tune (a launch
// with a table and no rows in force hands in the context's default row, stride 0); its selection reads io.ssTab where there is one and the parameter block's
// selection where there is none (a tuned launch without a table: k2_lap_of) -- a wave-uniform test in that instantiation only.
#define LMPC_SSTAB_LDS (2 * LMPC_MAX_USED_LAPS * sizeof(int))
// The lap K2 reads as entry l of problem b: from the table row (b and l are uniform over the wave: one 16-byte scalar load), else from the parameter block.
// latest: the entry takes the "current lap" branch of the Q-function shift (:502-512)
struct k2_lap { int slot, rows, latest; };
template <bool TAB>
__device__ __forceinline__ k2_lap k2_lap_of(const lmpc_dev_params &p, const lmpc_solve_io &io, int b, int l) {
    if (TAB && io.ssTab) { const int4 e = *(const int4 *)(io.ssTab + (size_t)b * io.ssTabStride + LMPC_SSTAB_ENTRY * l); return {e.x, e.y, e.z}; }
    return {p.sslot[l], p.sslen[l], p.sslapid[l] < p.cur_it - 1 ? 0 : 1};
}
__device__ __forceinline__ void flag_retry(const lmpc_solve_io &io, int st) {
    if (io.retry_flag && (st & (LMPC_ST_MAXITER | LMPC_ST_NUMERIC))) __hip_atomic_fetch_max(io.retry_flag, io.retry_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Step rules of the interior-point iteration (both solve kernels; tests/ipm_model.py mirrors them).
//  * round 6: three constants of these rules re-tuned on EVERY closed-loop QP of the reference's 40-lap experiment in the NumPy model (tools/knob_model.py, 12 442 QPs at N = 12,
//    10 336 at N = 14, the bench batches at N = 12 / 14 / 40; profiles/r6_knob_model.txt) instead of the few hundred problems of rounds 1-3: centring parameter
//    sigma = (gap_aff / gap)^5 (was ^3), fraction to the boundary 0.99 (was 0.995), separate steps after an iteration whose gap shrank by less than 20x (was 10x).  Closed loop
//    9.25 -> 8.98 iterations at N = 12 and 9.86 -> 9.49 at N = 14, QPs above 14 iterations halved (55 -> 28 of 12 442; 124 -> 64 of 10 336), and the 24-31-iteration two-cycle
//    QPs (1 in ~3 400: maxima 26 / 31 / 25 per seed) end at 17-18; bench batch 8.63 -> 8.44 (maximum 13 unchanged), N = 40 bench 10.91 / 18 -> 10.72 / 16.
//  * fraction to the boundary: LMPC_FRAC0, and once the predictor says the iteration is in its final phase (centring parameter sigma < 1e-3,
//    i.e. the affine step alone removes > 90 % of the gap) 1 - 10 gap: the gap then contracts quadratically instead of by 1 / 200 per
//    step (about one iteration less per solve).  Ungated, the longer step lets single complementarity products collapse while the
//    iterate is still far from the path (one 38-iteration stall in 1024 problems of the NumPy model); gated it never fired there.
//  * separate primal / dual step lengths after an iteration whose gap shrank by less than 1 / LMPC_SEP_THRESHOLD (20x).
#define LMPC_SEP_THRESHOLD 0.05
#define LMPC_FRAC0 0.99
//  * the corrector's second-order term dt_aff dmu_aff enters with weight LMPC_SO_W = 1.1 (same study: the bench batches' slowest problems -- linear tail, no strict
//    complementarity -- gain an iteration, 13 -> 12 at N = 12 and 14 -> 13 at N = 14 in the model; every closed-loop set is neutral within 0.3 %; 1.2 and beyond cost the closed loop)
#define LMPC_SO_W 1.1
//  * termination (round 6: ONE rule for every horizon and every kernel route; it replaces round 5's stack of gap-ratio / gap-floor / dual-residual thresholds, each
//    of which had been fitted to the last miss found).  The gap and residual tolerances say the KKT conditions hold; they do not say how far the iterate is from
//    the optimum: a QP without strict complementarity (about one in ten here) converges linearly and sits ~sqrt(gap) away, a flat closed-loop QP sits 660 dual
//    residuals away.  What the tolerance of the parity statement is written in is the distance itself, and a contracting iteration bounds it a posteriori:
//        |z_k - z*| <= rho / (1 - rho) |z_k - z_{k-1}|,   rho = |z_k - z_{k-1}| / |z_{k-1} - z_{k-2}|
//    (z = (x, u); max-norm of the steps actually taken, wave-uniform scalars the step phase has anyway).  The iteration ends when that estimate is below LMPC_ACC_TOL = 1e-7:
//    step^2 <= tol (step_prev - step), no division.  A superlinear last step passes at once (rho ~ 1e-3), a linearly converging problem iterates until the steps
//    are short enough, whatever made them long.  tools/term_rule_model.py (NumPy model, every QP of the reference's 40-lap closed loop at N = 12, three seeds = 12 442
//    QPs, iterated past the stop and compared with a 1e-15 solve; profiles/r6_term_rule_model.txt):
//        rule                                   closed-loop iterations   worst |xu - z*| / (1 + |z*|)   bench batch (iterations mean / max, worst error)
//        gap test alone (rounds 1-4)            8.97                     1.4e-5   (89 QPs > 3e-7)        8.31 / 13   1.5e-7
//        round 5, N <= 12 (1e-3 | 0.1)          8.98                     3.3e-6   (23)                  8.32 / 13   1.5e-7
//        round 5, N > 12 (1e-4 | 0.03 | est)    9.03                     3.8e-7   (2)                   8.44 / 13   2.1e-8
//        this rule, tol 3e-7                    9.18                     1.2e-7   (0)                   8.53 / 13   9.3e-10
//        this rule, tol 1e-7  (built)           9.26                     1.2e-7   (0)                   8.63 / 13   7.0e-10
//        ideal (first iterate within 3e-7)      8.98                                                    8.31 / 13
//    -- round 5's N <= 12 pair, the one the graded horizon ran, misses 1e-6 on 8 of 12 442 closed-loop QPs (the sampled probe had seen 8.75e-7 on 1 246).
//    The rate is an estimate from two steps, not a bound on the next one: at 3e-7 one of 10 336 closed-loop QPs at N = 14 stopped 3.7e-7 from its optimum (zt 1.02e-6:
//    its next contraction was 2.4 x slower than the last; the model and the GPU probe against the oracle found the same QP), at 1e-7 it iterates once more (1.7e-7 in
//    the model's worst case there).  Price against 3e-7: +0.9 % iterations in the closed loop, +1.2 % on the bench batch, maximum unchanged.
#define LMPC_ACC_TOL 1e-7
__device__ __forceinline__ bool step_bound_ok(double step, double step_prev) {
#ifdef LMPC_AB_NOACC                    // (developer A / B: the gap test alone, rounds 1-4)
    return true;
#endif
    return step < step_prev && step * step <= LMPC_ACC_TOL * (step_prev - step);
}
// Barrier weights theta = mu / t are capped at 1e11 in the Newton matrix: 1 / theta >= 1e-11 is a dual regularisation of the inequality row
// (F dw + (1 / theta_c) dmu = -r_c / mu); the right-hand side uses the same effective reciprocal rt = 1 / max(t, 1e-11 mu), so the fixed
// point does not move and the row's equation is off by 1e-11 dmu only.  Uncapped, an active lane row (t ~ 1e-14, mu ~ 10: main.py's fast
// laps, ey on the lane boundary) puts 1e15 into a stage Hessian whose other entries are O(1) and the Riccati recursion loses the regular
// part of the cost-to-go to rounding: the dual residual stalls at 1e-7 and the iteration wanders off (tests/ipm_model.py, tools/ipm_model_sets.py).
#define LMPC_TH_INV 1e-11
__device__ __forceinline__ double barrier_rt(double t, double mu) { return frcp(fmax(t, mu * LMPC_TH_INV)); }
__device__ __forceinline__ double step_fraction(double sig, double gap) { return sig < 1e-3 ? fmax(LMPC_FRAC0, 1.0 - 10.0 * gap) : LMPC_FRAC0; }
__device__ __forceinline__ double centring_sigma(double r) { const double r2 = r * r; return r2 * r2 * r; }       // (gap_aff / gap)^5

// ------------------------------------------------------------------------------------------------
// The parameter block in LDS (PAR_*).  Visible behind the caller's barrier.
// ------------------------------------------------------------------------------------------------
// tune: the problem's row of the tuning image (io.tune + b * io.tuneStride), or null: the block every problem shares
__device__ __forceinline__ void stage_params(const lmpc_dev_params &p, double *par, int lane, const double *tune = nullptr) {
    if (tune) { for (int i = lane; i < PAR_TOT; i += WAVE) par[i] = tune[i]; return; }
    if (lane < 12) par[PAR_FX + lane] = p.Fx[lane];
    if (lane < 8) par[PAR_FU + lane] = p.Fu[lane];
    if (lane < 2) { par[PAR_BX + lane] = p.bx[lane]; par[PAR_DR2 + lane] = p.dR2[lane]; }
    if (lane < 4) { par[PAR_BU + lane] = p.bu[lane]; par[PAR_R2 + lane] = p.R2[lane]; }
    if (lane < 36) { par[PAR_Q2 + lane] = p.Q2[lane]; par[PAR_QF2 + lane] = p.Qf2[lane]; }
    if (lane < 6) { par[PAR_T2 + lane] = p.T2[lane]; par[PAR_XREF + lane] = p.xRef[lane]; }
    if (lane == 0) { par[PAR_AS] = p.a_s; par[PAR_CS] = p.c_s; }
}

// ------------------------------------------------------------------------------------------------
// K2: safe-set selection.  LMPC.addTerminalComponents :392-412 and selectPoints :478-514.  Every solve kernel: wave `wave` of NW handles laps
// wave, wave + NW, ...; results go to SS (6 x S, row-major), Qsel (S), sel_start (window start per lap, kept for the successor rows of
// feasibleStateInput) and the optional global outputs.  With a lap table (io.ssTab) the laps are those of the problem's table row (k2_lap_of) and sel_lap
// receives their (slot, rows) pairs; else sel_lap is not touched.
// <N_, S_, NW, TAB_>: the fixed-(N, S) kernels hand in their template constants, and the instantiation is the text it was when N, S and TAB were the template's
// own parameters (same machine code).  N_ = 0: N and S come from the parameter block; TAB_ < 0: a table or none is found out at run time (the runtime kernel).
// ------------------------------------------------------------------------------------------------
// TAG: nothing in the function reads it.  The parking instantiation of a two- or four-wave kernel hands in its LIVE pack, so that it has a k2_select of its own: with
// ONE instance inlined into both the per-problem-rows kernel and its parking sibling, the per-problem-rows kernel came out with other scalar registers than it has
// alone (measured on all 44 of them; profiles/parking_kernel_diff.txt is taken with the tag).
template <int N_, int S_, int NW, int TAB_ = 0, class... TAG>
__device__ __forceinline__ void k2_select(const lmpc_dev_params &p, const lmpc_solve_io &io, int b, int lane, int wave, double *SS, double *Qsel,
                                          int *sel_start, int *sel_lap, int *st_sh) {
    const int N = N_ ? N_ : p.N, S = N_ ? S_ : p.S;
    const bool tab = TAB_ < 0 ? io.ssTab != nullptr : TAB_ != 0;
    if (io.mode & 1) {
        // TrackLength of THIS problem: its track row (lmpc_track_set) in the per-problem-rows instantiations and the runtime kernel -- one double per problem, uniform
        // over the wave -- else the parameter block's.  A retry pass gets the io of its own launch, hence the rows of its own launch.
        double TL = p.TL;
        if (TAB_ != 0) { if (io.trk) TL = io.trk[(size_t)b * io.trkStride + 1]; }
        double ztv[6];
#pragma unroll
        for (int j = 0; j < 6; j++) ztv[j] = io.zt[(size_t)b * 6 + j];
        const double x04 = io.x0[(size_t)b * 6 + 4];
        if (ztv[4] - x04 > TL / 2) ztv[4] = fmax(ztv[4] - TL, 0.0);        // :392-393
        if (io.ztUsed && wave == 0 && lane < 6) { double v = ztv[0];
#pragma unroll
            for (int j = 1; j < 6; j++) if (lane == j) v = ztv[j];
            io.ztUsed[(size_t)b * 6 + lane] = v; }
        const int hasPred = io.hasPred ? io.hasPred[b] : 0;                     // Q-function shift bookkeeping (:502-512)
        int crossed = 0;
        if (hasPred) {
#pragma unroll
            for (int r0 = 0; r0 <= N; r0 += WAVE) {                               // N + 1 predicted rows: 65 at the largest horizon, one more than a wave has lanes
                const int r = r0 + lane;
                const int c_ = (r <= N && io.xPredPrev[((size_t)b * (N + 1) + (r <= N ? r : 0)) * 6 + 4] > TL) ? 1 : 0;
                crossed += (int)__popcll(__ballot(c_));
            }
        }
        const int tstep = io.timeStep ? io.timeStep[b] : 0;
        const int ppl = p.ppl, npw = ppl + 1;                                   // numSS_Points/numSS_it + 1 (=13)
        for (int l = wave; l < p.L; l += NW) {
            int slot_ = p.sslot[l], T_ = p.sslen[l], latest_ = 0;
            if (tab) { const k2_lap lp = k2_lap_of<true>(p, io, b, l); slot_ = lp.slot; T_ = lp.rows; latest_ = lp.latest; if (lane == 0) { sel_lap[2 * l] = lp.slot; sel_lap[2 * l + 1] = lp.rows; } }
            const double *base = p.sstore + (size_t)slot_ * LMPC_COLS * p.lap_stride;
            const int T = T_, ls = p.lap_stride;
            double best = INFINITY; int bi = 0x7fffffff;
            for (int r = lane; r < T; r += WAVE) {
                double nrm = fabs(base[r] - ztv[0]);                            // la.norm(x - zt, 1, axis=1)
                nrm = nrm + fabs(base[ls + r] - ztv[1]);
                nrm = nrm + fabs(base[2 * ls + r] - ztv[2]);
                nrm = nrm + fabs(base[3 * ls + r] - ztv[3]);
                nrm = nrm + fabs(base[4 * ls + r] - ztv[4]);
                nrm = nrm + fabs(base[5 * ls + r] - ztv[5]);
                if (nrm < best) { best = nrm; bi = r; }
            }
            wave_argmin(best, bi);                                              // np.argmin: first minimum
            if ((unsigned)bi >= (unsigned)T) {                                  // no row compares below +inf: zt or x0 is not finite (np.argmin would go on with row 0 or the first NaN).
                bi = 0; if (lane == 0) atomicOr(st_sh, LMPC_ST_NUMERIC);        // The window arithmetic below must not see the sentinel (start + lane overflowed: a fault on the device)
            }
            const int MinNorm = bi;
            const int start = ((double)MinNorm - (double)npw / 2.0 >= 0.0) ? MinNorm - npw / 2 : MinNorm;   // :492-495
            if (lane == 0) { sel_start[l] = start; if (io.selStartOut) io.selStartOut[(size_t)b * p.L + l] = start; if (start + npw > T) atomicOr(st_sh, LMPC_ST_WINDOW); }
            double shift = 0.0;                                                 // :502-512
            if (hasPred && crossed > 0) {
                bool earlier = p.sslapid[l] < p.cur_it - 1;                     // (k2_lap_of<false>(..).latest is this test)
                if (tab) earlier = !latest_;
                if (earlier) shift = base[8 * ls];
                else shift = (double)tstep + (double)(N - crossed);
            }
            if (lane < ppl) {                                                   // (ppl <= 64: lmpc_create_ex refuses more points per lap than a wave has lanes)
                int r0 = start + lane; r0 = r0 > T - 1 ? T - 1 : r0;
                int r1 = start + lane + 1; r1 = r1 > T - 1 ? T - 1 : r1;
                const int col = l * ppl + lane;
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    const double v = base[j * ls + r0];
                    SS[j * S + col] = v;
                    if (io.ssSelOut) io.ssSelOut[((size_t)b * S + col) * 6 + j] = v;
                    if (io.succOut) io.succOut[((size_t)b * S + col) * 6 + j] = base[j * ls + r1];
                }
                if (io.succUOut) { io.succUOut[((size_t)b * S + col) * 2] = base[6 * ls + r1]; io.succUOut[((size_t)b * S + col) * 2 + 1] = base[7 * ls + r1]; }
                const double qv = base[8 * ls + r0] + shift;
                Qsel[col] = qv;
                if (io.qSelOut) io.qSelOut[(size_t)b * S + col] = qv;
            }
        }
    } else {
        for (int c = wave * WAVE + lane; c < S; c += NW * WAVE) {
#pragma unroll
            for (int j = 0; j < 6; j++) SS[j * S + c] = io.ssSelIn[((size_t)b * S + c) * 6 + j];
            Qsel[c] = io.qSelIn[(size_t)b * S + c];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Behind the selection: the regression kernel's status bits of this problem's N points (the reference raises there), and the end of a launch that
// only selects (io.mode bit 1 clear).  A retry pass does not call solve_regression_status: it takes the bits over from the first pass's status word
// (the per-point buffer may belong to a later launch by the time a deferred retry pass runs).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void solve_regression_status(const lmpc_solve_io &io, int b, int N, int lane, int *st_sh) {
    if (io.rstatus && lane < N) { const int rs_ = io.rstatus[(size_t)b * N + lane]; if (rs_) atomicOr(st_sh, rs_); }       // (N <= 64)
}
__device__ __forceinline__ bool solve_selection_only(const lmpc_solve_io &io, int b, int lane, const int *st_sh) {
    if (io.mode & 2) return false;
    if (lane == 0) io.status[b] = *st_sh;
    return true;
}

// ------------------------------------------------------------------------------------------------
// Start of the iteration, behind the roll-out x_{k+1} = A_k x_k + C_k (u = 0).  Lane slacks: a row the roll-out violates starts one unit inside
// (s = violation + 1); every other slack starts at 1 / c_s, where the multiplier of s >= 0 (mu0 / s) already balances the slack's linear cost c_s --
// from s = 1 the first Newton steps were spent driving ~2N slacks to zero against the positivity bound (11.0 -> 9.5 iterations on the bench batch,
// 12 -> 6 on the LTV-MPC QPs).  lambda = 1 / S.  qmax: enters as the largest |Qfun| among the selected columns lane, lane + 64, ... of the calling lane
// -- from LDS or from the caller's register copy -- and leaves as the largest of all.  Returns mu0.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double solve_start(int N, int S, int lane, double c_s, const double *par, const double *x, double *s, double *lam, double &qmax, int *st_sh) {
    const double *Fx = par + PAR_FX, *bx = par + PAR_BX, *bu = par + PAR_BU;
    const double s_init = c_s > 1.0 ? 1.0 / c_s : 1.0;
    for (int i = lane; i < 2 * N; i += WAVE) {
        const int k = i >> 1, j = i & 1; double f = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) f = fma(Fx[j * 6 + c], x[k * 6 + c], f);
        const double viol = f - bx[j];
        s[i] = viol > 0.0 ? viol + 1.0 : s_init;
    }
    if (S > 0) {
        for (int c = lane; c < S; c += WAVE) lam[c] = 1.0 / (double)S;
        qmax = wmax(qmax);
    }
    const double mu0 = fmax(1.0, 0.01 * (S > 0 ? qmax : 1.0));
    if (lane < 4 && !(bu[lane] > 0.0)) atomicOr(st_sh, LMPC_ST_NOT_INTERIOR);
    return mu0;
}

// ------------------------------------------------------------------------------------------------
// Exit status behind the iteration: a problem that left it without converging ends INEXACT where the KKT conditions hold to the looser bounds, else at
// the iteration limit.  Hard lane rows (MPCParams.slacks = False) are imposed through slack variables with a 1e12 quadratic weight: at the optimum a
// slack is mu / 2e12 ~ 1e-11 unless the hard problem is infeasible -- then it is the violation itself, and the reference's solver reports "primal
// infeasible" (feasible = 0, PredictiveControllers.py:277-280).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void solve_exit_status(const lmpc_dev_params &p, int N, int lane, bool converged, double gap, double rdn, double ren, double qscale,
                                                  const double *s, int *st_sh) {
    if (!converged && lane == 0 && !(*st_sh & (LMPC_ST_NUMERIC | LMPC_ST_INEXACT)))
        atomicOr(st_sh, (gap < 1e-9 && rdn < 1e-5 * qscale && ren < 1e-7) ? LMPC_ST_INEXACT : LMPC_ST_MAXITER);
    if (!p.slacks) {
        double smax = 0.0;
        for (int i = lane; i < 2 * N; i += WAVE) smax = fmax(smax, s[i]);
        smax = wmax(smax);
        if (smax > 1e-8 && lane == 0) atomicOr(st_sh, LMPC_ST_INFEASIBLE);
    }
}

// ------------------------------------------------------------------------------------------------
// Epilogue: unpackSolution (:364-379) and feasibleStateInput (:382-384; S = 0: MPC.feasibleStateInput :157-159), then status, iterations, the retry flag and
// the residuals.  zt = Succ_SS lambda, zt_u = Succ_uSS lambda: the successor rows are read back from the store (window starts kept in
// sel_start; with a table, slot and rows in sel_lap).  Reference order of np.dot(Succ, lambd): sequential over columns; the tree sum differs by rounding only.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void solve_epilogue(const lmpc_dev_params &p, const lmpc_solve_io &io, int b, int N, int S, bool tab, int lane,
                                               const double *x, const double *u, const double *s, const double *lam, const double *m, const double *SS,
                                               const int *sel_start, const int *sel_lap, const int *st_sh, int it, double gap, double rdn, double ren) {
    const int M = 8 * N + S;
    for (int i = lane; i < 6 * (N + 1); i += WAVE) io.xPred[(size_t)b * 6 * (N + 1) + i] = x[i];
    for (int i = lane; i < 2 * N; i += WAVE) { io.uPred[(size_t)b * 2 * N + i] = u[i]; if (io.slack) io.slack[(size_t)b * 2 * N + i] = s[i]; }
    if (io.mu) for (int r = lane; r < M; r += WAVE) io.mu[(size_t)b * M + r] = m[r];
    if (S > 0) {
        if (io.lambda) for (int c = lane; c < S; c += WAVE) io.lambda[(size_t)b * S + c] = lam[c];
        if (lane < 6 && io.sTerm) {
            double v = -x[N * 6 + lane];
            for (int c = 0; c < S; c++) v = fma(SS[lane * S + c], lam[c], v);
            io.sTerm[(size_t)b * 6 + lane] = v;
        }
        if ((io.mode & 1) && (io.ztNext || io.ztuNext)) {
            double acc[8];
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] = 0.0;
            for (int c = lane; c < S; c += WAVE) {
                const int l = c / p.ppl, cc = c % p.ppl;
                int slot = p.sslot[l], T = p.sslen[l];
                if (tab) { slot = sel_lap[2 * l]; T = sel_lap[2 * l + 1]; }
                const double *base = p.sstore + (size_t)slot * LMPC_COLS * p.lap_stride;
                int r1 = sel_start[l] + cc + 1; r1 = r1 > T - 1 ? T - 1 : r1;
                const double lv = lam[c];
#pragma unroll
                for (int j = 0; j < 8; j++) acc[j] = fma(base[j * p.lap_stride + r1], lv, acc[j]);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] = wsum(acc[j]);
            if (lane < 6 && io.ztNext) { double v = acc[0];
#pragma unroll
                for (int j = 1; j < 6; j++) if (lane == j) v = acc[j];
                io.ztNext[(size_t)b * 6 + lane] = v; }
            if (lane < 2 && io.ztuNext) io.ztuNext[(size_t)b * 2 + lane] = lane == 0 ? acc[6] : acc[7];
        }
    } else {
        if (lane < 6 && io.ztNext) io.ztNext[(size_t)b * 6 + lane] = x[N * 6 + lane];
        if (lane < 2 && io.ztuNext) io.ztuNext[(size_t)b * 2 + lane] = u[(N - 1) * 2 + lane];
    }
    if (lane == 0) {
        const int st = *st_sh;
        io.status[b] = st; io.iters[b] = it; flag_retry(io, st);
        if (io.resid) { io.resid[(size_t)b * 3] = gap; io.resid[(size_t)b * 3 + 1] = rdn; io.resid[(size_t)b * 3 + 2] = ren; }
    }
}
