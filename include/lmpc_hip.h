/*
 * include/lmpc_hip.h -- C ABI of liblmpc_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the per-time-step LMPC hot path of urosolia/RacingLMPC.  The reference has
 * no FFI: its seam is Python duck typing (Simulator.sim -> Controller.solve(x0), SysModel.py:34).
 * Each entry point below replaces the reference interface cited next to it (paths under
 * /root/reference/src/fnc/controller/).  The Python side that binds these symbols with ctypes is
 * racinglmpc_amd/_capi.py; the drop-in modules are racinglmpc_amd/PredictiveControllers.py and
 * racinglmpc_amd/PredictiveModel.py.
 *
 * Conventions: extern "C"; every function returns 0 on success or a negative LMPC_E_* code and
 * never throws; plain pointers and sizes only; all matrices row-major FP64 (NumPy C-contiguous);
 * host pointers unless the name ends in _dev; caller owns every buffer; one lmpc_ctx per Python
 * controller object; calls on one ctx are serialised by the caller.
 */
#ifndef LMPC_HIP_H
#define LMPC_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define LMPC_NX 6
#define LMPC_NU 2
#define LMPC_MAX_TRACK_ROWS 16
#define LMPC_MAX_USED_LAPS 32      /* trToUse / numSS_it upper bound (the reference takes any: PredictiveControllers.py:293-311, PredictiveModel.py:31) */
#define LMPC_MAX_N 64              /* horizon: 2 <= N <= 64 */
#define LMPC_MAX_SS_POINTS 384     /* numSS_points upper bound = 32 laps x 12 points (beyond 58 the terminal block takes several columns per lane); at most 63 points per
                                      lap (the selection's window of points-per-lap + 1 rows is one row per lane).  With an odd number of points per lap the reference's
                                      window has one row more than its QP has columns and the reference cannot assemble the step; the library keeps the first
                                      points-per-lap rows of that window.
                                      The one-wave layout of every pair of the range fits a CU (at most 108 KB of LDS per QP).  The two- and four-wave kernels
                                      exist where their layout fits the 160 KB as well -- not at N = 64 from 96 points or N = 40 with 384: such a pair runs one wave per QP at
                                      every batch size (lmpc_solver_lds reports 0 for them).  The runtime-(N, S) kernel shares nothing between phases and stops earlier:
                                      N = 64 beyond 146 points (209 KB at 384) and N = 40 beyond 366 are LMPC_E_ARG there and need their fixed variant.  A fixed variant
                                      exists where its build passes the ISA check (racinglmpc_amd.build): (40, 384), (64, 192) and (64, 384) do and are tested; the other
                                      pairs beyond the runtime kernel's limit have not been compiled -- one whose build fails would be refused with LMPC_E_ARG */

/* error codes (function return values) */
#define LMPC_OK 0
#define LMPC_E_ARG (-1)            /* bad argument / unsupported configuration */
#define LMPC_E_HIP (-2)            /* a HIP runtime call failed (see lmpc_last_error) */
#define LMPC_E_CAPACITY (-3)       /* (no longer returned: the lap stores grow on demand; kept so that the numbering of the codes is stable) */
#define LMPC_E_STATE (-4)          /* call not valid in the current state (e.g. no laps stored) */
#define LMPC_E_VARIANT (-5)        /* lmpc_create: the solve kernels for this (N, numSS_points) are not part of the library and their shared object
                                      liblmpc_var_N<N>_S<S>.so (next to liblmpc_hip.so) has not been built yet; racinglmpc_amd builds it on demand */

/* per-problem status bits (status[] outputs); 0 == solved */
#define LMPC_ST_MAXITER 1          /* interior-point iteration limit hit before tolerances met */
#define LMPC_ST_REG_SINGULAR 2     /* local regression normal matrix not positive definite (reference: cvxopt raises) */
#define LMPC_ST_NO_SEGMENT 4       /* curvature(): s on no track segment (reference: int(np.where) raises, Track.py:307) */
#define LMPC_ST_WINDOW 8           /* safe-set window runs past the end of a stored lap (reference: IndexError, :497) */
#define LMPC_ST_NUMERIC 16         /* NaN / non-positive pivot inside the KKT factorisation */
#define LMPC_ST_NOT_INTERIOR 32    /* u = 0 is not strictly inside Fu u <= bu (solver start point) */
#define LMPC_ST_INFEASIBLE 128      /* lmpc_config.slacks = 0 (MPCParams.slacks = False): a hard lane row is exceeded by more than 1e-8 at the optimum of the penalised
                                    * problem, i.e. the hard problem has no feasible point (e.g. x0 already outside the lane: its k = 0 row is fixed by the
                                    * equality).  Reference: OSQP reports primal infeasible and MPC.solve sets feasible = 0 (PredictiveControllers.py:277-280). */
#define LMPC_ST_INEXACT 64         /* returned iterate is optimal to working accuracy only (gap < 1e-9, dual residual < 1e-5 rel., equality
                                      residual < 1e-7) because the factorisation broke down or the iteration limit was hit at that point;
                                      the solution is usable (the reference's own solver tolerance is 1e-3) */

typedef struct lmpc_ctx lmpc_ctx;

/* Numeric content of MPCParams (PredictiveControllers.py:24-51), of PredictiveModel.__init__
 * (PredictiveModel.py:12-32), of the LMPC constructor (PredictiveControllers.py:293-311) and of the
 * track table Map.PointAndTangent (Track.py:54-133).                                              */
typedef struct {
    int N;                      /* horizon (reference main.py:43 uses 14; BASELINE metric uses 12) */
    int numSS_it;               /* laps in the safe set per solve; 0 => plain MPC/LTV-MPC, no terminal set */
    int numSS_points;           /* total safe-set columns (reference: 12 * numSS_it = 48); any multiple of numSS_it up to LMPC_MAX_SS_POINTS, at most 63 per lap */
    int trToUse;                /* laps used by the regression (PredictiveModel usedIt) */
    int maxNumPoint;            /* 7   (PredictiveModel.py:18) */
    double h, lamb, dt;         /* 5, 0.0, 0.1 (PredictiveModel.py:19-21) */
    double scaling[5];          /* diag of PredictiveModel.py:22-26 */
    double Q[36], R[4], Qf[36], dR[2], Qslack[2], QtermSlack[36], xRef[6];
    double Fx[12], bx[2], Fu[8], bu[4];          /* 2 state rows, 4 input rows (reference shapes) */
    double track[LMPC_MAX_TRACK_ROWS * 6]; int track_rows; double trackLength;
    int device;                 /* HIP device ordinal */
    int max_batch;              /* capacity of internal work buffers */
    int max_laps, max_lap_len;  /* INITIAL lap-store capacity (rows per lap include addPoint extensions).  The reference's stores are Python lists
                                 * (PredictiveControllers.py:418-445, :466-474; PredictiveModel.py:35-46): when a lap or a row does not fit, the
                                 * device stores are reallocated at >= twice the size (lmpc_*_add_trajectory, lmpc_ss_add_point, lmpc_ss_extend_lap) */
    /* solver: structure-exploiting primal-dual interior point on the block-banded KKT system */
    double tol_gap, tol_res, reg_lambda; int max_iter;
    int slacks;                 /* MPCParams.slacks (:184-198, 218-221, 248-254): 1 = lane rows softened by slack variables (main.py always);
                                   0 = hard lane rows Fx x_k <= bx, no slack variables in the QP (plain MPC only: numSS_it = 0).  Solved with an internal
                                   quadratic slack weight of 1e12: a hard row may be exceeded by mu / 2e12 ~ 1e-11; the `slack` output holds that excess. */
} lmpc_config;

typedef struct {
    double ms_regress, ms_solve;      /* accumulated HIP-event time of the two kernels (profiling on).  A regression that ran ahead on the look-ahead stream
                                         (lmpc_step_batch_dev, queued steps) shares the chip with the previous step's solve: its time includes the wait for a free CU */
    long long n_regress, n_solve;     /* launches accumulated */
    long long qp_solved;              /* problems passed through the solve kernel */
    long long ipm_iters;              /* interior-point iterations accumulated by the host-buffer entry points (lmpc_step_batch, lmpc_qp_solve_batch) */
    long long n_regress_timed, n_solve_timed;   /* launches that carried events: ms_regress / n_regress_timed is the average kernel duration */
    long long n_retry;                /* retry passes launched on demand (a problem of the batch ended at the iteration limit / broke down; see lmpc_capi.hip) */
} lmpc_stats;

int lmpc_config_default(lmpc_config *cfg);                       /* reference defaults, N = 12 */
int lmpc_create(const lmpc_config *cfg, lmpc_ctx **out);         /* MPC/LMPC.__init__, :63-107, :293-338 */
int lmpc_create_ex(const lmpc_config *cfg, unsigned flags, lmpc_ctx **out);
        /* lmpc_create with flags.  LMPC_CREATE_RUNTIME_KERNEL: an (N, numSS_points) pair that is neither built in nor available as a variant library is served by
         * the runtime-(N, S) solve kernel (any horizon without a compiler on the box, several times slower) instead of LMPC_E_VARIANT -- MPCParams.N is a plain
         * parameter in the reference (:63-107, main.py:43).  LMPC_CREATE_FORCE_RUNTIME_KERNEL: use that kernel even where a fast one exists (tests).
         * LMPC_CREATE_NO_K1_AHEAD: no look-ahead regression -- for contexts of which several run side by side on one device (racinglmpc_amd._capi.ContextPool): their batches
         * fill each other's idle CUs already, and the look-ahead's event operations measured 3-5 % slower there */
#define LMPC_CREATE_RUNTIME_KERNEL 1u
#define LMPC_CREATE_FORCE_RUNTIME_KERNEL 2u
#define LMPC_CREATE_NO_K1_AHEAD 4u       /* queued lmpc_step_batch_dev steps keep their regression on the context's stream (see lmpc_step_batch_dev); same results */
#define LMPC_CREATE_NO_K1_MERGE 8u       /* queued steps never hold a solve for a two-role launch: the two-stream look-ahead serves every chained step (see lmpc_step_batch_dev); same results */
int lmpc_solver_kind(lmpc_ctx *);                                /* 0: built-in solve kernels, 1: variant library, 2: runtime-(N, S) kernel */
int lmpc_destroy(lmpc_ctx *ctx);
const char *lmpc_last_error(void);
const char *lmpc_active_knobs(void);                             /* developer environment variables this process has acted on ("NAME=value;..."; "" = none): LMPC_K1_QG,
                                                                    LMPC_K1_RPL16, LMPC_MW_MAX_BATCH, LMPC_MW2_MAX_BATCH, LMPC_FUSE, LMPC_CD, LMPC_NO_ABG, LMPC_TRACE_OWN_STREAM, LMPC_K1_AHEAD, LMPC_K1_AHEAD_MAX_BATCH, LMPC_K1_MERGE, LMPC_K1_MERGE_QG -- route / grid
                                                                    choices, each announced once on stderr; no reference counterpart.  Bit-identical results: LMPC_TRACE_OWN_STREAM
                                                                    (traced sessions: the trace kernel on a stream of its own instead of the plant stream), LMPC_K1_QG, LMPC_K1_RPL16
                                                                    (regression grid / scan build: A, B, C do not depend on either), LMPC_FUSE (fused one-wave step against the
                                                                    two-kernel one-wave step; ignored by the runtime-(N, S) kernel, which has no fused form), LMPC_NO_ABG
                                                                    ([A_k | B_k] in LDS instead of global memory), LMPC_K1_AHEAD (=0 at lmpc_create: queued
                                                                    lmpc_step_batch_dev steps keep their regression on the context's stream, behind the previous solve,
                                                                    instead of the look-ahead stream beside it; LMPC_K1_AHEAD_MAX_BATCH: the largest batch that chains), LMPC_K1_MERGE (=0 at lmpc_create: no held solves, no
                                                                    two-role launches; LMPC_K1_MERGE_QG: the cap of the queries per regression work-group in them).  LMPC_MW_MAX_BATCH and LMPC_MW2_MAX_BATCH move a batch to
                                                                    another solve kernel (four / two / one wave(s) per QP): A, B, C, the selection and the status word stay
                                                                    bit-identical, the QP answer agrees to the termination rule's bound (x, u within 2e-7: measured by
                                                                    tests/test_gpu_routes.py).  LMPC_CD (condensed kernel, opt-in builds only): another QP method, same optimum
                                                                    to the stated tolerances (tests/test_gpu_condensed.py) */
int lmpc_version(void);
int lmpc_device_memory(int device, unsigned long long *free_bytes, unsigned long long *total_bytes);
        /* hipMemGetInfo of `device`: what is left of the 288 GB for max_batch, the lap stores (lmpc_config: max_laps x max_points) and rollout sessions -- and what a
         * destroyed context has given back (tests/test_gpu_stores.py).  No reference counterpart (the reference holds its stores in Python lists) */

/* ---- lap stores -------------------------------------------------------------------------------
 * Two separate stores, as in the reference: the regression store (PredictiveModel.xStored/uStored)
 * and the safe set (LMPC.SS/uSS/Qfun).  Device layout: [lap][column][row], FP64, row stride
 * max_lap_len, so that a wave scanning one column of one lap reads contiguous memory.           */
int lmpc_model_add_trajectory(lmpc_ctx *, const double *x /*T x 6*/, const double *u /*T x 2*/, int T);
        /* PredictiveModel.addTrajectory, PredictiveModel.py:35-46: sorted insert, ascending T, ties append */
int lmpc_model_num_laps(lmpc_ctx *, int *n);
int lmpc_model_replace_lap(lmpc_ctx *, int pos /*position in sorted order*/, const double *x, const double *u, int T);
int lmpc_model_set_lap_table(lmpc_ctx *, int n, const int *laps /*n x trToUse insertion indices, or NULL with n = 0*/);
        /* Per-problem regression laps (one of the five per-car row sets, one contract: INTEGRATION.md section 4, "The per-car row sets"): which stored laps the regression (PredictiveModel.regressionAndLinearization) of each problem of a batch reads -- each car's
         * LTV model from its own data, main.py:88-89 per car.  An entry is the INSERTION index of a regression-store lap (0 = the first lmpc_model_add_trajectory):
         * stable under later inserts and store growth, unrelated to the lap's position in the sorted order.  Duplicates inside a row are allowed (main.py:103-104 adds
         * one lap four times).  Each row is used in the order a context holding only those laps would use them -- ascending length, ties by insertion index
         * (PredictiveModel.py:35-46) -- whatever order the caller lists them in.  n = 0: back to the context-wide default, the first trToUse laps of the sorted
         * order.  n = 1: that row serves every problem.  n > 1: problem b of a call uses row b, and a call whose batch B != n returns LMPC_E_ARG and says so in
         * lmpc_last_error (the context stays usable).  LMPC_E_ARG for an index < 0 or >= the laps stored, n < 0, NULL with n > 0, n > max_batch x N: after such an
         * argument error the table in force stays (a HIP failure while the device image is uploaded, LMPC_E_HIP, leaves the context without a table).  The table applies wherever the regression kernel runs: lmpc_regress_batch, lmpc_regress_points (point e uses row e), lmpc_step_batch,
         * lmpc_step_batch_dev, lmpc_rollout_begin and the LTV form of lmpc_rollout_begin_mpc with every step of their sessions -- a session takes a snapshot when it
         * begins, a later call reaches the next session only.  On an LMPC context (numSS_it > 0) ONLY THE REGRESSION follows the table: the safe set, its selection and
         * the terminal constraint stay shared by all problems unless the safe set is given its own table, lmpc_ss_set_lap_table.  With a table in force the fused one-wave step (LMPC_FUSE=1) is not taken: the two-kernel step runs.
         * The table lives on the device as resolved (slot, rows) pairs, uploaded here and not per launch; it is rebuilt from the indices when the stores are
         * reallocated or a lap is replaced.  As for the regression grid and scan build, A, B, C of a problem do not depend on which other rows the table holds */
int lmpc_model_get_lap_table(lmpc_ctx *, int *n, int *laps /*capacity rows x trToUse, or NULL*/, int capacity);
        /* the rows in force as lmpc_model_set_lap_table received them (n = 0: the default); laps receives min(n, capacity) rows */
int lmpc_model_lap_info(lmpc_ctx *, int lap /*insertion index*/, int *rows /*or NULL*/, int *sorted_pos /*or NULL*/);
        /* the regression-store lap with that insertion index: its rows, and its position in the sorted order -- the index lmpc_store_read_lap (store 0) and
         * lmpc_model_replace_lap take.  Needs no device.  LMPC_E_ARG for an index that names no stored lap */
int lmpc_ss_add_trajectory(lmpc_ctx *, const double *x, const double *u, int T);
        /* LMPC.addTrajectory + computeCost, PredictiveControllers.py:418-464 (it += 1) */
int lmpc_ss_add_point(lmpc_ctx *, const double *x /*6*/, const double *u /*2*/);
        /* LMPC.addPoint, :466-474: append x + [0,0,0,0,TrackLength,0] to lap it-1, Qfun[-1]-1 */
int lmpc_ss_replace_lap(lmpc_ctx *, int lap, const double *x, const double *u, const double *qfun, int T);
int lmpc_ss_set_selected(lmpc_ctx *, const int *laps, int n);
        /* override of argsort(LapTime)[0:numSS_it] (:395,402); n = 0 restores the built-in stable sort */
int lmpc_ss_set_lap_table(lmpc_ctx *, int n, const int *laps /* n x numSS_it safe-set lap indices, lmpc_ss_add_trajectory order; NULL with n = 0 */,
                          const int *last /* n, or NULL */);
        /* Per-problem safe sets (one of the five per-car row sets, one contract: INTEGRATION.md section 4, "The per-car row sets"): which stored laps the selection (LMPC.addTerminalComponents / selectPoints, :386-412, :478-514) of each problem of a batch reads -- each
         * car's terminal set and terminal cost from its own laps, as every LMPC object of the reference owns SS / uSS / Qfun / LapTime (:395-412).  Row b names the numSS_it
         * laps problem b selects from, by their index in lmpc_ss_add_trajectory order.  Duplicates are allowed (main.py:109-110 adds one lap four times), so a row may be
         * served by fewer than numSS_it stored laps.  Each row is used in the order a controller holding only those laps would use them -- ascending LapTime
         * (lmpc_ss_get_laptime), ties by lap index, a stable argsort(LapTime) -- whatever order the caller lists them in: the columns of ssSel / qSel / succ / succU /
         * lambda and selStart[b, l] follow that order.  last[b]: the index of car b's most recent lap, the reference's self.it - 1; it need not be in the row.  An entry
         * of row b takes the "current lap" branch of the Q-function shift (:502-512: timeStep + N - crossed) iff its index equals last[b], every other entry takes
         * Qfun[it][0]; last[b] = -1: none does.  last = NULL: the context-wide rule for every row -- the latest lap is index lmpc_ss_num_laps - 1 at launch time.
         * n = 0: back to the shared selection (lmpc_ss_set_selected / the built-in argsort), bit for bit.  n = 1: that row serves every problem.  n > 1: problem b of a
         * call uses row b, and a launch whose batch B != n returns LMPC_E_ARG and says so in lmpc_last_error (the context stays usable).  LMPC_E_ARG for an index < 0 or
         * >= the laps stored, last outside [-1, laps stored), n < 0, NULL laps with n > 0, n > 0 on a context with numSS_it = 0: after such an argument error the table
         * in force stays.  The table names LAPS, not snapshots of them: rows appended or removed by lmpc_ss_add_point, lmpc_ss_extend_lap, lmpc_ss_truncate_lap,
         * lmpc_ss_replace_lap, a new lmpc_ss_add_trajectory and a growth of the stores are seen by the next launch (the device image of resolved (slot, rows, latest)
         * entries is uploaded again before the next launch that reads it, after the retry passes of earlier launches have run against the image of their own launch).
         * The table applies wherever the selection runs on the device: lmpc_select_batch, lmpc_step_batch, lmpc_step_batch_dev and every step of an lmpc_rollout_begin
         * session.  It is LIVE in a session, as lmpc_ss_set_selected is -- not a snapshot taken at begin like the model table: a `set` between two lmpc_rollout_run
         * calls reaches the next step, and B is checked against n before the first launch of a step, so a refused lmpc_rollout_run leaves no half-done step.  All solve
         * kernels (one, two, four waves per QP, the runtime-(N, S) kernel, their retry passes) serve a table -- the fixed-(N, S) ones in instantiations of their own, so
         * that a launch without a table runs the kernels it ran before; the fused one-wave step (LMPC_FUSE=1) and the condensed
         * kernel (LMPC_CD=1) do not and are not taken while one is in force: the two-kernel step / the ordinary kernels run.  With a table a launch asks for 256 bytes
         * more dynamic LDS per QP (slot and rows of the selected laps for the successor rows of feasibleStateInput); without one nothing changes */
#define LMPC_SS_LAST_SHARED (-2)
int lmpc_ss_get_lap_table(lmpc_ctx *, int *n, int *laps /* capacity x numSS_it, or NULL */, int *last /* capacity, or NULL */, int capacity);
        /* the rows in force as lmpc_ss_set_lap_table received them (n = 0: the shared selection); laps / last receive min(n, capacity) rows / entries, every entry of
         * last LMPC_SS_LAST_SHARED where `set` was given last = NULL */

/* Per-problem controller tuning: the cost weights and bounds of each problem of a batch from its own row -- every controller object of the reference owns its MPCParams
 * (PredictiveControllers.py:24-51, initControllerParameters.py).  A row is LMPC_TUNING_NPAR doubles in this order: Q[36], R[4], Qf[36], dR[2], Qslack[2],
 * QtermSlack[6] (the diagonal), xRef[6], bx[2], bu[4] -- the values of lmpc_config, not the doubled ones of the device block.  Fx and Fu, the shape of the
 * constraint rows, stay context-wide. */
#define LMPC_TUNING_NPAR 98
int lmpc_tuning_from_config(const lmpc_config *, double *row /*98*/);
        /* the row a context created from that config uses by default (MPCParams, PredictiveControllers.py:24-51).  Needs no device */
int lmpc_tuning_set(lmpc_ctx *, int n, const double *rows /*n x 98, or NULL with n = 0*/);
        /* The tuning (MPCParams, PredictiveControllers.py:24-51) of every later solve on this context (one of the five per-car row sets, one contract: INTEGRATION.md section 4, "The per-car row sets").  n = 0: back to the config's weights, bit for bit (the kernels
         * that read the parameter block).  n = 1: that row serves every problem.  n > 1: problem b of a call uses row b, and a launch whose batch B != n returns
         * LMPC_E_ARG and says so in lmpc_last_error (the context stays usable) -- the lap tables' rule.  LMPC_E_ARG, with the rows in force kept, for a non-finite
         * entry, Q, R or Qf not exactly symmetric, a negative dR or Qslack entry, a QtermSlack entry <= 0 on a context with numSS_it > 0, n < 0, n > max_batch, NULL
         * rows with n > 0.  (n <= max_batch also bounds what a rollout session can use: lmpc_rollout_begin accepts more cars than max_batch, but such a session
         * cannot have one row per car -- `set` refuses the rows, and rows of another count refuse every step; it runs on n = 0 or n = 1.  Create the context with
         * max_batch >= the cars of a per-car tuned session.)  A row with bu[j] <= 0 is NOT an argument error: the kernels' own rule gives that problem LMPC_ST_NOT_INTERIOR and leaves its neighbours
         * alone.  On a context with slacks = 0 the rows' Qslack is ignored (the internal weight 1e12 and no linear term, as for the config).  The rows apply to
         * lmpc_qp_solve_batch, lmpc_step_batch, lmpc_step_batch_dev, every step of lmpc_rollout_begin and lmpc_rollout_begin_mpc sessions (LTI and LTV form) and
         * lmpc_assemble_batch (the explicit matrices of problem b from row b); lmpc_select_batch and the regression read no weights.  The rows are LIVE, as the
         * safe-set table is: a `set` between two lmpc_rollout_run calls reaches the next step, and B is checked against n before the first launch of a step, so a
         * refused step leaves nothing half done.  The device image (doubled values in the layout of the kernels' parameter block in LDS, ready for their staging copy)
         * is uploaded by `set`, not per launch; launches still waiting for their deferred retry pass are resolved and the stream is drained before it is overwritten,
         * so a retry pass reads the rows of its own launch.  All solve kernels (one, two, four waves per QP, the runtime-(N, S) kernel, their retry passes) serve rows
         * -- the fixed-(N, S) ones in the per-problem-rows instantiations that also serve the safe-set table, so that a launch without rows or table runs the kernels
         * it ran before.  While rows are in force NEITHER the fused one-wave step (LMPC_FUSE=1) NOR the condensed kernel (LMPC_CD=1, which takes Q pre-digested by
         * the host) is taken: the two-kernel step / the ordinary kernels run */
int lmpc_tuning_get(lmpc_ctx *, int *n, double *rows /*capacity x 98, or NULL*/, int capacity);
        /* the rows in force as lmpc_tuning_set received them (n = 0: the config's weights; MPCParams, PredictiveControllers.py:24-51); rows receives min(n, capacity) rows */

/* Per-car tracks: the track table and length of each element of a batch from its own row -- the reference builds one Map per spec (Track.py:13 "Modify the vector spec
 * to change the geometry of the track").  A row is LMPC_TRACK_NPAR doubles: [0] the number of table rows (an integer 1..16 as a double), [1] trackLength, [2..97]
 * PointAndTangent, 16 x 6 row-major (x, y, psi, cumulative s, segment length, curvature), unused rows zero. */
#define LMPC_TRACK_NPAR 98
int lmpc_track_row_from_config(const lmpc_config *, double *row /*98*/);
        /* the row a context created from that config uses by default (track, track_rows, trackLength).  Needs no device */
int lmpc_track_set(lmpc_ctx *, int n, const double *rows /*n x 98, or NULL with n = 0*/);
        /* Per-car tracks (one of the five per-car row sets, one contract: INTEGRATION.md section 4, "The per-car row sets").  n = 0: the config's track; every path returns the bits it returned before there were rows (the kernels that read the parameter block run).  n = 1: that row
         * serves every car.  n > 1: element b of a batched call uses row b, and a call whose count differs from n returns LMPC_E_ARG and says so in lmpc_last_error
         * (the context stays usable).  LMPC_E_ARG, with the rows in force kept, for a non-finite entry, a row count that is not an integer in 1..16, trackLength <= 0, a
         * negative segment length (a zero or rounding-sized one is a row no s lies on, e.g. the closing row of an oval: accepted), n < 0, n > max_batch, NULL rows with
         * n > 0.  LMPC_E_STATE while a rollout session is active: a lap on a track that changes under it means nothing, so rows are NOT live (unlike tuning rows).
         * Launches still waiting for their deferred retry pass are resolved and the stream is drained before the device image is overwritten, so a retry pass reads
         * the rows of its own launch.
         * "Element b": problem b of lmpc_regress_batch, lmpc_step_batch, lmpc_step_batch_dev, lmpc_select_batch, lmpc_qp_solve_batch (where it selects); point e of
         * lmpc_regress_points, lmpc_global_position_batch, lmpc_local_position_batch, lmpc_track_angle_batch; car b of lmpc_plant_step_batch, of lmpc_rollout_begin /
         * _begin_mpc / _pid sessions and every step of them, of lmpc_rollout_commit_laps / _extend_laps (computeCost and addPoint with the car's own TrackLength) and of
         * the T x B log of lmpc_state_from_global_batch.  max_ey stays one scalar per call.
         * The host-side lap writers name no car: lmpc_ss_add_trajectory, lmpc_ss_add_point and lmpc_ss_extend_lap use the config's TrackLength at n = 0 and row 0 at
         * n = 1, and return LMPC_E_STATE at n > 1 -- the _on forms below take the row.  lmpc_ss_replace_lap takes its own Qfun; lmpc_model_* reads no track.
         * While rows are in force neither the fused one-wave step (LMPC_FUSE=1) nor the condensed kernel (LMPC_CD=1) is taken, as with tuning rows; the selection reads
         * the problem's TrackLength in the per-problem-rows instantiations of the solve kernels and in the runtime-(N, S) kernel */
int lmpc_track_get(lmpc_ctx *, int *n, double *rows /*capacity x 98, or NULL*/, int capacity);
        /* the rows in force as lmpc_track_set received them (n = 0: the config's track); rows receives min(n, capacity) rows */
int lmpc_ss_add_trajectory_on(lmpc_ctx *, int track_row, const double *x, const double *u, int T);
int lmpc_ss_extend_lap_on(lmpc_ctx *, int track_row, int lap, const double *x /*n x 6*/, const double *u /*n x 2*/, int n);
        /* lmpc_ss_add_trajectory / lmpc_ss_extend_lap with the TrackLength of track row `track_row` (0 <= track_row < max(n, 1) of lmpc_track_set) in computeCost / addPoint */
int lmpc_ss_num_laps(lmpc_ctx *, int *n);
int lmpc_ss_get_qfun(lmpc_ctx *, int lap, double *qfun /*T*/, int *T);
int lmpc_store_read_lap(lmpc_ctx *, int store /*0: regression store (sorted position), 1: safe set*/, int lap, double *x /*T x 6*/, double *u /*T x 2*/, double *qfun /*T, safe set only*/, int *T);
        /* checkpoint / resume: one stored lap back on the host, safe-set laps with the rows LMPC.addPoint appended (the reference imports pickle for this and never uses it,
         * main.py:36; racinglmpc_amd._capi.Context.save_stores / restore_stores write and read an .npz).  Any of x, u, qfun may be NULL */
int lmpc_ss_get_laptime(lmpc_ctx *, int lap, int *T);
        /* LMPC.LapTime[lap] (:420): rows of the lap when it was added (without addPoint extensions) -- what argsort(LapTime) sorts */
int lmpc_store_retain(lmpc_ctx *, int n_ss, const int *keep_ss, int n_model, const int *keep_model,
                      int *map_ss /* laps stored before the call, or NULL */, int *map_model /* likewise, or NULL */);
        /* Laps given back: each store keeps the laps listed and drops the others, and the device stores shrink to what is kept.  No reference counterpart -- its lists
         * only grow (PredictiveControllers.py:418-445, PredictiveModel.py:35-46), although a controller reads only numSS_it fastest laps plus the latest one
         * (:395-412, :502-512) and trToUse fastest laps (PredictiveModel.py:31).  keep_ss: n_ss strictly ascending safe-set lap indices (lmpc_ss_add_trajectory order);
         * keep_model: n_model strictly ascending regression-store insertion indices.  n = -1 (with NULL) leaves that store untouched, n = 0 empties it.  Afterwards the
         * k-th kept lap has index k in its store; map[old] is the new index of lap `old`, -1 for a dropped one (the identity for an untouched store).  Relative order is
         * kept, so the regression store's sorted order among the kept laps (ascending rows, ties by insertion index) and the shared selection (stable argsort of LapTime)
         * are what they were.  Without a `last` column the LATEST LAP is the highest kept index: cur_it = the laps kept, as if only they had ever been added.
         * Everything that names a lap is renumbered with the stores: the rows of lmpc_model_set_lap_table, the rows and `last` of lmpc_ss_set_lap_table, the override
         * of lmpc_ss_set_selected; their device images are rebuilt.  Checked in full before anything changes -- a refused call leaves stores, books, tables and
         * capacities as they were: LMPC_E_ARG for a list that is not strictly ascending or names a lap not stored, and for a lap that a table in force, a `last`
         * entry or the override names and the list does not keep (lmpc_last_error names the table, the row and the lap); LMPC_E_STATE while a rollout session is
         * active.  Keeping fewer than numSS_it / trToUse laps without a table is no error here: the next step reports it as it always did.
         * Like every store edit it launches a held solve (lmpc_dev_flush), resolves pending retry passes against the stores of their launch and drains the context's
         * streams first.  The kept laps are gathered by one kernel launch into new zero-filled allocations -- device memory peaks at old + new during the call -- whose
         * lap capacity is the smallest (initial max_laps) x 2^j that holds both stores' kept laps; the row capacity stays, and later growth works as before.  A HIP
         * failure on the way (LMPC_E_HIP) frees the new allocations and leaves the context as it was.  A call that keeps every lap of both stores does nothing. */

/* ---- batched compute, host buffers --------------------------------------------------------- */
int lmpc_regress_batch(lmpc_ctx *, int B, const double *xLin /*B x N x 6 (first N rows used)*/, int xLinRowStride /* (N+1)*6 or N*6 */,
                       const double *uLin /*B x N x 2*/,
                       double *A /*B x N x 36*/, double *Bm /*B x N x 12*/, double *C /*B x N x 6*/, int *status /*B x N*/);
int lmpc_regress_points(lmpc_ctx *, int n, const double *x /*n x 6*/, const double *u /*n x 2*/, double *A /*n x 6 x 6*/, double *B /*n x 6 x 2*/, double *C /*n x 6*/, int *status /*n*/);
        /* PredictiveModel.regressionAndLinearization, PredictiveModel.py:48-197, for n independent points (the reference calls it with one): no horizon around them */
        /* MPC.computeLTVdynamics -> PredictiveModel.regressionAndLinearization, :140-145 / PredictiveModel.py:48-197 */

int lmpc_select_batch(lmpc_ctx *, int B, const double *x0 /*B x 6*/, const double *zt /*B x 6*/,
                      const double *xPredPrev /*B x (N+1) x 6*/, const int *hasPred /*B*/, const int *timeStep /*B*/,
                      double *ssSel /*B x S x 6*/, double *qSel /*B x S*/, double *succ /*B x S x 6*/, double *succU /*B x S x 2*/,
                      double *ztUsed /*B x 6*/, int *selStart /*B x numSS_it: first row of each lap's window, or NULL*/, int *status /*B*/);
        /* LMPC.addTerminalComponents (selection part) + selectPoints, :386-412, :478-514.  xPredPrev, hasPred, timeStep may be NULL (a first step);
         * a set hasPred[b] without xPredPrev is LMPC_E_ARG -- here, in lmpc_step_batch and (any hasPred array) in lmpc_step_batch_dev */

int lmpc_qp_solve_batch(lmpc_ctx *, int B, const double *A, const double *Bm, const double *C,
                        const double *x0 /*B x 6*/, const double *uOld /*B x 2*/,
                        const double *ssSel /*B x S x 6 or NULL*/, const double *qSel /*B x S or NULL*/,
                        double *xPred /*B x (N+1) x 6*/, double *uPred /*B x N x 2*/, double *slack /*B x 2N*/,
                        double *lambda /*B x S*/, double *sTerm /*B x 6*/, double *mu /*B x (8N+S) ineq duals, reference row order*/,
                        int *status /*B*/, int *iters /*B*/, double *resid /*B x 3: gap, dual res, eq res*/);
        /* buildCost/buildEqConstr/addSafeSet* + osqp_solve_qp + unpackSolution, :200-283, :340-379 */

int lmpc_step_batch(lmpc_ctx *, int B, const double *x0, const double *xLin /*B x (N+1) x 6*/, const double *uLin /*B x N x 2*/,
                    const double *uOld, const double *zt, const double *xPredPrev, const int *hasPred, const int *timeStep,
                    double *xPred, double *uPred, double *slack, double *lambda, double *sTerm,
                    double *ztNext /*B x 6*/, double *ztuNext /*B x 2*/, double *ssSel /*B x S x 6*/,
                    double *qSel /*B x S: Qfun_SelectedTot, :404-412, or NULL*/, double *mu /*B x (8N+S) inequality duals, reference row order, or NULL*/,
                    double *Aout /*B x N x 36 or NULL*/, double *Bout, double *Cout,
                    int *status, int *iters, double *resid);
        /* one full MPC.solve(x0) per problem, :110-137 (a3 -> a19 of SURVEY section 8).  status[b] carries the solver bits and the
         * OR of the regression kernel's per-point bits (LMPC_ST_REG_SINGULAR, LMPC_ST_NO_SEGMENT) of the problem's N points. */

int lmpc_assemble_batch(lmpc_ctx *, int B, const double *A, const double *Bm, const double *C, const double *x0, const double *uOld,
                        const double *ssSel, const double *qSel,
                        double *Pdense /*B x nz x nz*/, double *q /*B x nz*/, double *Adense /*B x m x nz*/, double *l /*B x m*/, double *u /*B x m*/);
        /* the reference's explicit OSQP-form matrices (H_FTOCP,q_FTOCP,[F;G],l,u of :259-273), for parity checks only */
int lmpc_qp_dims(lmpc_ctx *, int *nz, int *m_ineq, int *m_eq);

/* ---- device-resident path (bench / rollouts): buffers live in HBM ---------------------------- */
int lmpc_dev_alloc(lmpc_ctx *, long long bytes, void **dptr);
int lmpc_dev_free(lmpc_ctx *, void *dptr);
int lmpc_dev_upload(lmpc_ctx *, void *dptr, const void *host, long long bytes);
int lmpc_dev_download(lmpc_ctx *, void *host, const void *dptr, long long bytes);
int lmpc_dev_sync(lmpc_ctx *);
typedef struct {          /* all device pointers, layouts as in lmpc_step_batch.  Optional (NULL = not wanted): slack, lambda, sTerm, ztNext, ztuNext,
                             ssSel, A, Bm, C, mu, resid, qSel.  With LMPC_FUSE=1 in the environment, batches that run one wavefront per QP take
                             the step as ONE kernel: each wave first runs the regression (MPC.computeLTVdynamics, :140-145) of its own QP,
                             A_i / B_i / C_i stay in LDS and are copied out only if A / Bm / C are given (results bit-identical to the
                             two-kernel step on the one-wave kernel; measured slower, hence off by default; contexts served by the
                             runtime-(N, S) kernel ignore the knob). */
    const double *x0, *xLin, *uLin, *uOld, *zt, *xPredPrev; const int *hasPred, *timeStep;
    double *xPred, *uPred, *slack, *lambda, *sTerm, *ztNext, *ztuNext, *ssSel, *A, *Bm, *C, *mu, *resid;
    int *status, *iters;
    double *qSel;          /* B x S or NULL */
} lmpc_step_dev_args;
int lmpc_step_batch_dev(lmpc_ctx *, int B, const lmpc_step_dev_args *args);   /* async on the ctx stream; status as in lmpc_step_batch */
        /* Queued steps.  When the previous call on the context was also a two-kernel lmpc_step_batch_dev, this step's regression is queued on a second stream of the
         * context's and runs BESIDE the previous step's solve (it needs nothing of it); the solves themselves stay strictly one after the other, each behind its own
         * regression.  The regression writes a hand-over set of the context's, which the solve reads, and copies A / Bm / C to the caller's arrays where given: those are
         * outputs only, nothing on the device reads them except a retry pass at the next drain, so the caller keeps them (and every input: xLin / uLin of step i + 1 are
         * read while step i solves) untouched until lmpc_dev_sync, as before.  ONE set of A / Bm / C shared by several queued steps is covered only while no launch is
         * pending its retry pass: a problem that ends at the iteration limit (LMPC_ST_MAXITER, LMPC_ST_NUMERIC) is solved again at the next drain, from the arrays its
         * step was given, and finds the regression of the last queued step in shared ones -- a caller whose problems may raise that flag gives every queued step its
         * own A / Bm / C (or none).  Any other call on the context that queues work or edits what the regression reads (lap
         * stores, lap table, track / tuning rows, lmpc_dev_upload, ...) breaks the chain: the next step's regression goes behind it on the context's stream.  A drain of
         * the context (lmpc_dev_sync, lmpc_dev_download) covers both streams.  Results are bit-identical to the unchained step; LMPC_K1_AHEAD=0 turns chaining off.
         * Held solves.  On the plain four-wave route (up to one QP per CU, no lap / safe-set table, tuning or track rows in force, A / Bm / C given, not under
         * lmpc_set_profiling(1)) the solve of a chained step is not launched by its own call: the next lmpc_step_batch_dev launches it in ONE launch with its own
         * regression -- a two-role build of the solve kernel, nothing but kernels in the queue -- and EVERY other entry point of the context launches it first thing,
         * stand-alone on the context's stream, so each of them finds the order it found before.  The outputs of a queued step are defined after the next lmpc_dev_sync,
         * as they always were; new is only that the LAST queued solve starts at the next call into the context.  A caller that queues steps and then goes away to do
         * host work calls lmpc_dev_flush, which launches a held solve and returns without draining.  lmpc_destroy DROPS a held solve without launching it: the caller
         * may have freed its arrays by then, and nothing has asked for the results.  LMPC_K1_MERGE=0 at lmpc_create (or LMPC_CREATE_NO_K1_MERGE) keeps the two-stream form. */
int lmpc_dev_flush(lmpc_ctx *);            /* launches a held solve (above), if there is one; no drain.  The next lmpc_step_batch_dev starts a new chain */

/* ---- caller side of the path, next row of SURVEY 8(f): plant integrator + device-resident closed-loop laps ---- */
/* Map.getGlobalPosition (Track.py:135-189), batched: curvilinear (s, ey) -> inertial (X, Y) for n points on the track given
 * in lmpc_config.track (plotting / logging export, plot.py:50-175).  status[e] = LMPC_ST_NO_SEGMENT where the reference raises. */
int lmpc_global_position_batch(lmpc_ctx *, int n, const double *s /*n*/, const double *ey /*n*/, double *xy /*n x 2*/, int *status /*n*/);

/* The inverse of that map.  Map.getLocalPosition (Track.py:191-290), batched: inertial pose (X, Y, psi) -> curvilinear (s, ey, epsi) for n points, the reference's
 * walk over the track rows branch for branch (exact end-point tests, the two-angle test of a straight row, the arc test of a curved row; the first row that
 * completes wins).  max_ey is the reference's halfWidth + slack (0.85 on its track; the track table does not carry it): a projection further from the centre line
 * does not complete its row.  status[e] = LMPC_ST_NO_SEGMENT and s = ey = epsi = 10000.0 where no row completes (the values the reference returns after its
 * message) or an input is not finite.  psi may be any multiple of 2 pi away from the track's angle (np.unwrap against the row's angle, as the reference).
 * Map.getAngle (Track.py:312-349), batched: (s, epsi) -> psi; status[e] = LMPC_ST_NO_SEGMENT and psi = 0 where the reference raises (s on no row).
 * LMPC_E_ARG for n < 1, a NULL pointer, a non-finite or negative max_ey. */
int lmpc_local_position_batch(lmpc_ctx *, int n, const double *x /*n*/, const double *y /*n*/, const double *psi /*n*/, double max_ey,
                              double *s /*n*/, double *ey /*n*/, double *epsi /*n*/, int *status /*n*/);
int lmpc_track_angle_batch(lmpc_ctx *, int n, const double *s /*n*/, const double *epsi /*n*/, double *psi /*n*/, int *status /*n*/);
int lmpc_state_from_global_batch(lmpc_ctx *, int T, int B, const double *xglob /*T x B x 6: vx vy wz psi X Y*/, double max_ey,
                                 double *x /*T x B x 6: vx vy wz epsi s ey*/, int *status /*T x B*/);
        /* Map.getLocalPosition (Track.py:191-290) on every row of a session log in the layout of lmpc_rollout_fetch: the device function of
         * lmpc_local_position_batch per row, vx, vy, wz copied through.  Rows are independent: s lies on the first lap, it is NOT made continuous across the finish
         * line (racinglmpc_amd.rollout.lap_from_global adds the lap count on the host).  LMPC_E_ARG for T < 1, B < 1, a NULL pointer, a non-finite or negative max_ey */

int lmpc_plant_step_batch(lmpc_ctx *, int B, const double *x /*B x 6*/, const double *x_glob /*B x 6*/, const double *u /*B x 2*/,
                          const double *noise /*B x 3 N(0,1) draws*/, double *x_next, double *x_glob_next, int *status);
        /* Simulator.dynModel, fnc/simulator/SysModel.py:56-147 (100 Euler sub-steps, clipped noise) */

/* Per-car vehicle constants of the plant.  The reference's Simulator.dynModel carries one vehicle as literals (SysModel.py:60-70); a row of
 * LMPC_PLANT_NPAR doubles holds those ten values in the reference's order: m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br.  As in the reference the rear slip
 * angle is taken with lf (SysModel.py:97); lr enters the yaw equation only (:106). */
#define LMPC_PLANT_NPAR 10
int lmpc_plant_params_default(double *par /*10*/);
        /* the literals of SysModel.py:60-70: m = 1.98, lf = lr = 0.125, Iz = 0.024, Cf = Cr = 1.25, Bf = Br = 1.0, Df = Dr = 0.8 * m * 9.81 / 2.0 evaluated in that
         * order.  Needs no device */
int lmpc_plant_set_params(lmpc_ctx *, int n, const double *par /*n x 10, or NULL with n = 0*/);
        /* the vehicle(s) of every later lmpc_plant_step_batch, lmpc_rollout_begin, lmpc_rollout_begin_mpc and lmpc_rollout_pid on this context (Simulator.dynModel,
         * SysModel.py:56-147, with the constants of :60-70 replaced; one of the five per-car row sets, one contract: INTEGRATION.md section 4, "The per-car row sets").  n = 0: the reference's vehicle (the kernels that carry the literals).  n = 1: every car uses
         * that row.  n > 1: car b uses row b, n <= max_batch; a later call with B > n returns LMPC_E_ARG and says so in lmpc_last_error.  LMPC_E_ARG for a non-finite
         * entry, m <= 0 or Iz <= 0: the parameters in force stay.  A rollout session takes a snapshot when it begins: setting parameters while a session is active
         * is allowed and reaches the next session only; kept session buffers of the same shape are reused whatever the parameters */
int lmpc_plant_get_params(lmpc_ctx *, int *n, double *par /*capacity rows x 10, or NULL*/, int capacity);
        /* the rows in force (n = 0: the reference's vehicle, SysModel.py:60-70); par receives min(n, capacity) rows */

/* Counter-based N(0,1) draws generated on the device.  The reference has no counterpart beyond np.random.randn() at SysModel.py:139-141 (plant) and
 * Utilities.py:67-68 (PID control law).  The draw for (seed, stream, lap, t, car) is a pure function of those five numbers: its four 64-bit words are what
 * numpy.random.Philox(counter=[t, car, lap, stream], key=[seed, 0]).random_raw(4) returns (Philox4x64-10; NumPy increments word 0 of the counter before its first
 * block, so the block function runs on [t + 1, car, lap, stream]); Box-Muller in FP64 turns the pairs (w0, w1), (w2, w3) into z0, z1 and z2, z3:
 * u1 = ((w0 >> 11) + 1) 2^-53, u2 = (w1 >> 11) 2^-53, r = sqrt(-2 log u1), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2).  stream 0: plant noise (width 3: z0, z1, z2);
 * stream 1: control-law noise of a PID lap (width 2: z0, z1).  car: the GLOBAL rollout index; t: the simulated step; lap: a session counter the caller chooses. */
int lmpc_noise_raw(lmpc_ctx *, unsigned long long seed, unsigned long long stream, unsigned long long lap, long long t0, int T, long long car0, int B,
                   unsigned long long *words /*host, T x B x 4*/);
        /* the four raw words of steps t0 .. t0 + T - 1 and cars car0 .. car0 + B - 1 (checks of the block function and its addressing).  No reference counterpart beyond
         * np.random.randn() at SysModel.py:139-141 and Utilities.py:67-68.  LMPC_E_ARG for T < 1, B < 1, t0 < 0 or car0 < 0 */
int lmpc_noise_fill(lmpc_ctx *, unsigned long long seed, unsigned long long stream, unsigned long long lap, long long t0, int T, long long car0, int B,
                    int width /*2 or 3*/, double *out /*host, T x B x width*/);
        /* the normal draws of the same range, in the layout of the `noise` / `noise_u` arguments below: out[((t - t0) B + b) width + j].  No reference counterpart beyond
         * np.random.randn() at SysModel.py:139-141 and Utilities.py:67-68.  LMPC_E_ARG for width outside {2, 3}, T < 1, B < 1, t0 < 0 or car0 < 0 */
int lmpc_rollout_set_noise(lmpc_ctx *, int on, unsigned long long seed, unsigned long long lap, long long car0);
        /* the noise source of later sessions on this context.  No reference counterpart beyond np.random.randn() at SysModel.py:139-141 and Utilities.py:67-68.
         * on != 0: lmpc_rollout_begin, lmpc_rollout_begin_mpc and lmpc_rollout_pid accept noise = NULL (lmpc_rollout_pid also noise_u = NULL) and then fill the session's
         * buffer on the device, on the context's stream in front of the first step: steps 0 .. T_max - 1, cars car0 .. car0 + B - 1, `lap` as given, stream 0 (noise) /
         * stream 1 (noise_u) -- no host draw, no host-to-device copy of noise.  A non-NULL array is used exactly as without this call.  on == 0 (the state after
         * lmpc_create): a NULL array is LMPC_E_ARG and every path returns the bits it returned before this entry point existed.  A session takes (seed, lap, car0) when it
         * begins, as it does the vehicle rows: setting the source while a session is active reaches the next session only.  The library never advances `lap` on its own.
         * LMPC_E_ARG for car0 < 0 */
int lmpc_rollout_get_noise(lmpc_ctx *, int *on, unsigned long long *seed, unsigned long long *lap, long long *car0);
        /* what lmpc_rollout_set_noise left in force (on = 0 after lmpc_create); any pointer may be NULL.  No reference counterpart beyond np.random.randn() at
         * SysModel.py:139-141 and Utilities.py:67-68 */
int lmpc_rollout_begin(lmpc_ctx *, int B, int T_max, const double *x0 /*B x 6*/, const double *xglob0 /*B x 6*/,
                       const double *xLin0 /*B x (N+1) x 6*/, const double *uLin0 /*B x N x 2*/, const double *noise /*T_max x B x 3, or NULL: lmpc_rollout_set_noise*/);
int lmpc_rollout_begin_mpc(lmpc_ctx *, int B, int T_max, const double *x0 /*B x 6*/, const double *xglob0 /*B x 6*/,
                           const double *xLin0 /*B x (N+1) x 6 or NULL*/, const double *uLin0 /*B x N x 2 or NULL*/,
                           const double *A_lti /*B x 6 x 6 or NULL*/, const double *B_lti /*B x 6 x 2 or NULL*/, const double *noise /*T_max x B x 3, or NULL: lmpc_rollout_set_noise*/, int stop_at_line);
        /* Simulator.sim with one plain MPC per rollout (main.py:72-95; MPC.solve, PredictiveControllers.py:110-137), state resident on the device.  Valid only on a
         * context with numSS_it == 0 (lmpc_rollout_begin keeps refusing those), B <= max_batch, no session active.  A_lti / B_lti given: the LTI path-following MPC on the
         * model of Utilities.Regression (main.py:74-82) -- rollout b solves with A_b, B_b at every stage and C = 0 (buildEqConstr :216-218); xLin0 / uLin0 are not used.
         * Both NULL: the LTV-MPC (timeVarying, main.py:85-95) on the regression store -- trToUse laps must be stored (else LMPC_E_STATE, as lmpc_step_batch); per step
         * xLin <- [xPred[1:], xPred[N]], uLin <- [uPred[1:], uPred[N-1]], OldInput <- uPred[0] (:129-137, feasibleStateInput :157-159).  stop_at_line = 1:
         * Simulator(multiLap = False), lmpc_rollout_run ends once every car has crossed the line (SysModel.py:45); 0: all T_max steps (multiLap = True, main.py:57),
         * doneAt still the first crossing.  lmpc_rollout_run / _fetch / _end / _release, lmpc_debug_rollout_peek and lmpc_debug_rollout_qp (selection outputs NULL)
         * work on the session as on one of lmpc_rollout_begin */
int lmpc_rollout_pid(lmpc_ctx *, int B, int T_max, const double *x0 /*B x 6*/, const double *xglob0 /*B x 6*/, const double *vt /*B*/,
                     const double *noise_u /*T_max x B x 2 N(0,1) draws, or NULL: lmpc_rollout_set_noise*/, const double *noise /*T_max x B x 3, or NULL*/, int stop_at_line, int *steps_total, int *n_done);
        /* Simulator.sim driven by Utilities.PID (main.py:61-70; PID.solve, fnc/Utilities.py:60-67: u0 = -0.6 ey - 0.9 epsi + clip(0.25 n0, +-0.9),
         * u1 = 1.5 (vt - vx) + clip(0.10 n1, +-0.2)) for B cars, the whole lap in ONE kernel launch: begins a session, runs it to the end (all T_max steps; with
         * stop_at_line a car is logged up to its crossing step only), and leaves it active for lmpc_rollout_fetch / _end.  Needs only the track: valid on any context
         * (B <= max_batch, T_max <= 100000, no session active).  The plant step is the device function of lmpc_plant_step_batch: same state and draws, same bits */
int lmpc_rollout_run(lmpc_ctx *, int max_steps, int *steps_total, int *n_done);
int lmpc_rollout_fetch(lmpc_ctx *, int t0, int t1, double *X /*(t1-t0) x B x 6*/, double *U /*.. x B x 2*/, double *Xglob,
                       int *doneAt /*B*/, int *status /*B*/, double *finalX /*B x 6*/, double *finalXglob /*B x 6*/);
int lmpc_rollout_end(lmpc_ctx *);
        /* Simulator.sim with one LMPC controller per rollout, SysModel.py:22-54, state resident on the device.  The session's device buffers are kept for the next
         * lap of the same shape (a generation loop begins one per lap); lmpc_rollout_release or lmpc_destroy frees them */
int lmpc_rollout_release(lmpc_ctx *);
        /* give the kept session buffers back (55 MB at 1024 rollouts x 400 steps) without destroying the context; not valid between begin and end.  No reference counterpart */

/* ---- session traces (version 110; kernel: racinglmpc_amd/csrc/lmpc_trace.hip.h).  What the controller of a listed car computed at every step of a session, kept on
 * the device beside the plant's logs: the three per-step logs LMPC.unpackSolution appends (PredictiveControllers.py:364-379: xStoredPredTraj, uStoredPredTraj,
 * SSStoredPredTraj), the Q-values of the selected points, the solver's words of the step and the inertial positions of the predicted and selected points
 * (Map.getGlobalPosition, Track.py:135-189; plot.py:106-175 draws them). */
enum { LMPC_TRACE_XPRED = 1,   /* (N+1) x 6                      xStoredPredTraj[it][i]            */
       LMPC_TRACE_UPRED = 2,   /* N x 2                          uStoredPredTraj[it][i]            */
       LMPC_TRACE_SS    = 4,   /* S x 6 selected points          SSStoredPredTraj[it][i] (= SS_PointSelectedTot.T) */
       LMPC_TRACE_QSEL  = 8,   /* S  Qfun_SelectedTot                                              */
       LMPC_TRACE_SOLVER= 16,  /* int iters, int status of the step (status: the step's own word, not the accumulated one) */
       LMPC_TRACE_XY    = 32 };/* (N+1) x 2 inertial (X, Y) of the xPred rows; on a context with a safe set also S x 2 of the
                                  selected points; one int mapStatus per (step, car) */
#define LMPC_TRACE_ALL 63u
int lmpc_rollout_set_trace(lmpc_ctx *, int n, const int *cars /*n distinct car indices, any order; NULL with n = 0: off*/, unsigned what);
        /* the cars and planes later sessions of lmpc_rollout_begin and lmpc_rollout_begin_mpc (LTV and LTI form) record at every step (LMPC.unpackSolution,
         * PredictiveControllers.py:364-379).  A session takes (cars, what) as a snapshot when it begins, like the vehicle rows and the noise source: a `set` during a
         * session reaches the next session only.  Off after lmpc_create; with the trace off every path allocates, launches and returns what it did before this entry
         * point existed.  lmpc_rollout_pid ignores it (no predictions).  LMPC_E_ARG, with the trace in force kept, for n < 0, n > 0 with NULL cars, what == 0 or
         * unknown bits, a negative or repeated car, LMPC_TRACE_SS or LMPC_TRACE_QSEL on a context with numSS_it == 0.  A car >= B is refused by the `begin` that meets
         * it, before any session state changes.  Needs no device */
int lmpc_rollout_get_trace(lmpc_ctx *, int *n, int *cars /*capacity, or NULL*/, unsigned *what, int capacity);
        /* what lmpc_rollout_set_trace left in force (n = 0, what = 0: off); cars receives min(n, capacity) entries.  No reference counterpart (the reference's
         * logs are Python lists, PredictiveControllers.py:364-379) */
int lmpc_rollout_trace_bytes(lmpc_ctx *, int n, unsigned what, int T_max, long long *bytes);
        /* device memory a session of that shape allocates for its trace planes: T_max x n x the bytes of the planes per (step, car) -- XPRED (N+1) x 6 doubles, UPRED
         * N x 2, SS S x 6, QSEL S, SOLVER two ints, XY ((N+1) + S) x 2 doubles and one int; S = numSS_points on a context with a safe set, else 0.  On an LMPC context
         * SS, QSEL and XY also make the session keep the selection outputs of the last step for all B cars (B x S x 15 doubles, the buffers of
         * lmpc_debug_rollout_capture), not counted here.  No reference counterpart (Python lists, PredictiveControllers.py:364-379).  Needs no device */
typedef struct { double *xPred, *uPred, *ssSel, *qSel, *xyPred, *xySS; int *iters, *status, *mapStatus; } lmpc_trace_out;   /* any may be NULL */
int lmpc_rollout_fetch_trace(lmpc_ctx *, int t0, int t1, const lmpc_trace_out *out);   /* plane layout [t - t0][k][...], k = position in `cars` */
        /* the trace rows of steps [t0, t1) of the active session (xStoredPredTraj / uStoredPredTraj / SSStoredPredTraj of PredictiveControllers.py:364-379, per listed
         * car).  Every row t < steps taken has been written for every listed car, also for a car that has crossed the line (its lane keeps solving): cut at doneAt.
         * mapStatus[t][k]: LMPC_ST_NO_SEGMENT if a point of that row lies on no segment of the car's track (written as (0, 0), the rule of
         * lmpc_global_position_batch), else 0.  LMPC_E_STATE with no session active, on a session begun without a trace and on a lmpc_rollout_pid session;
         * LMPC_E_ARG for a non-NULL pointer of a plane the session does not record, t0 < 0, t1 < t0, t1 beyond the steps taken */
/* ---- parking (version 111; kernel: racinglmpc_amd/csrc/lmpc_live.hip.h).  A car that has crossed the line, or that the caller lists before the session begins, is taken
 * out of the launches: the kernels of a session step run over the ascending list of the cars still live, and the session ends when none is left.  Cars are independent
 * problems, so a live car computes bit for bit what it computes in the session without parking.  No reference counterpart (Simulator.sim runs one car, SysModel.py:22-54). */
#define LMPC_PARK_FINISHED 1u   /* in a session that stops at the line, a car leaves the launches at the first poll after its crossing step */
#define LMPC_PARK_REROUTE  2u   /* the solve-kernel route (4 / 2 / 1 waves per QP) follows the live count; default: the route of the session's B */
int lmpc_rollout_set_parking(lmpc_ctx *, unsigned mode, int n, const int *cars /* n distinct cars parked from step 0; NULL with n = 0 */);
        /* the parking of later sessions of lmpc_rollout_begin and lmpc_rollout_begin_mpc (LTV and LTI form); lmpc_rollout_pid ignores it, as it ignores traces.  Off
         * (mode 0, no cars) after lmpc_create, and then every path allocates, launches and returns what it did before this entry point existed.  A session takes
         * (mode, cars) as a snapshot when it begins, like the trace and the noise source: a `set` during a session reaches the next session only.  Needs no device.
         * LMPC_E_ARG, with the setting in force kept, for unknown mode bits, n < 0, n > 0 with NULL cars, a negative or repeated car.  A car >= B is refused, and
         * named, by the `begin` that meets it, before any session state changes.  LMPC_PARK_FINISHED acts only in sessions that stop at the line (lmpc_rollout_begin,
         * lmpc_rollout_begin_mpc with stop_at_line = 1); a session that logs its cars past the crossing parks the start list only.
         * The live list is built at `begin` and rebuilt at the finished-lap poll lmpc_rollout_run makes anyway (every 8 steps and at the end of a run), when nDone has
         * moved since the last rebuild: a car is stepped for up to 7 steps past its crossing.  The live count comes back in the copy that brings nDone.  A session that
         * stops at the line ends when no car is live (with a start list only: when every car not on it has crossed); n_done keeps its meaning.  With every car on the
         * start list `begin` succeeds and lmpc_rollout_run returns at once with 0 steps.
         * statusAcc, doneAt, finX and finG of a car are what they are without parking (frozen at the crossing step either way).  NOT WRITTEN for a parked car, from its
         * parking step on: its state, its log rows and its trace planes -- lmpc_rollout_fetch and lmpc_rollout_fetch_trace return what the kept buffers held there
         * (a reused session: the previous lap's rows); cut at lmpc_rollout_parked_at.  lmpc_rollout_commit_laps with explicit rows[k] beyond a parked car's parking
         * step and lmpc_rollout_extend_laps with n_rows beyond it are LMPC_E_ARG, car named; rows = NULL (up to doneAt) is always inside.
         * A parking session runs the per-problem-rows instantiations of the regression and solve kernels (the config's own row where no rows are in force) and never
         * the condensed kernel; the four-wave route needs the live count <= the four-wave batch limit on either route, which holds because it never exceeds B */
int lmpc_rollout_get_parking(lmpc_ctx *, unsigned *mode, int *n, int *cars /*capacity, or NULL*/, int capacity);
        /* what lmpc_rollout_set_parking left in force (mode 0, n 0: off); cars receives min(n, capacity) entries; any pointer may be NULL.  No reference counterpart */
int lmpc_rollout_parked_at(lmpc_ctx *, int *at /*B: -1 live, else the first step the car was not stepped*/, int *n_live);
        /* of the active session (LMPC_E_STATE without one); a session without parking answers -1 for every car and n_live = B.  Either pointer may be NULL */
int lmpc_debug_live_compact(lmpc_ctx *, int n, const int *doneAt, const int *parked0 /*n flags*/, int t, unsigned mode, int *live /*n; n_live written*/, int *parkedAt /*n, in and out: -1 = not parked so far*/, int *n_live);
        /* (every build) the session's own compaction kernel between host arrays: car b is parked if parkedAt[b] >= 0 on entry, parked0[b] != 0, or (LMPC_PARK_FINISHED)
         * doneAt[b] >= 0; a car parked by this call gets parkedAt[b] = t; live receives the others in ascending order.  Any n >= 1 */
int lmpc_ss_extend_lap(lmpc_ctx *, int lap, const double *x /*n x 6*/, const double *u /*n x 2*/, int n);
/* Undo extensions: keep the first T rows of stored lap `lap` (LapTime <= T <= current rows).  rollout.LmpcGeneration rolls a failed
 * generation back with it, so that a generation either completes or leaves the safe set as it found it.  No reference counterpart. */
int lmpc_ss_truncate_lap(lmpc_ctx *, int lap, int T);
        /* LMPC.addPoint (:466-474) applied to any stored lap: n points appended with s + TrackLength, Qfun counting down */

/* ---- laps of the active session committed to the lap stores ON THE DEVICE (version 107; kernels: racinglmpc_amd/csrc/lmpc_commit.hip.h).  The session logs lie in
 * device memory next to the stores: no log is downloaded, no lap uploaded, one launch serves every listed car. */
#define LMPC_COMMIT_SS 1u
#define LMPC_COMMIT_MODEL 2u
int lmpc_rollout_commit_laps(lmpc_ctx *, int n, const int *cars /*n*/, const int *rows /*n, or NULL: doneAt[car]*/,
                             unsigned stores, int *first_ss /*or NULL*/, int *first_model /*or NULL*/);
        /* For i = 0 .. n-1 in the order listed, the effect of fetching the logs and then lmpc_ss_add_trajectory(X[:T_i, car_i], U[:T_i, car_i], T_i) (bit LMPC_COMMIT_SS:
         * LMPC.addTrajectory + computeCost, PredictiveControllers.py:418-464) followed by lmpc_model_add_trajectory of the same rows (bit LMPC_COMMIT_MODEL:
         * PredictiveModel.addTrajectory, PredictiveModel.py:35-46; its prefilter image serves the scan of :180-197).  Afterwards store contents, Qfun, LapTime, the
         * regression store's sorted order (ties append, in listed order), its prefilter image and the safe-set table's dirty mark are bit for bit what the host path
         * leaves.  The new laps get consecutive indices; first_ss / first_model receive the first (-1 for a store not written).  A car may be listed more than
         * once: every entry gets a lap (main.py:103-110 adds one lap four times).  Valid in an active session of any kind (lmpc_rollout_begin, _begin_mpc, _pid) with
         * at least one step taken.  Everything is checked before anything changes: LMPC_E_ARG for n < 1, NULL cars, a car outside [0, B), stores 0 or with unknown
         * bits, rows[i] < 1 (< 2 with the model bit, as lmpc_model_add_trajectory), rows[i] beyond what the session logged for that car (the steps taken; for a car of
         * a stop_at_line PID session its crossing step); LMPC_E_STATE when rows == NULL and a listed car has doneAt < 0 (lmpc_last_error names the car).  One store
         * growth, one table upload, one launch, one download of n doubles; the context's bookkeeping changes only after the launch has completed */
int lmpc_rollout_extend_laps(lmpc_ctx *, int n, const int *cars /*n*/, const int *laps /*n distinct safe-set lap indices*/,
                             int n_rows, int *extended /*n: 1 appended, 0 skipped (a non-finite value)*/);
        /* lmpc_ss_extend_lap(laps[i], X[:n_rows, cars[i]], U[:n_rows, cars[i]], n_rows) -- the batched LMPC.addPoint, PredictiveControllers.py:466-474 -- for every entry
         * whose n_rows x 8 logged values are all finite; the other entries are left untouched and reported in `extended`.  Qfun continues from the lap's last value by
         * repeated subtraction of 1.0, as the host loop does.  The caller keeps deciding on status bits (it has them from lmpc_rollout_fetch with t0 = t1 = 0).
         * LMPC_E_ARG, before anything changes, for n_rows < 1 or beyond the steps taken, a lap index that names no stored lap, the same lap twice, a car out of range.
         * One store growth, one launch, one download of the flags; the live safe-set table sees the longer laps at the next step */
/* ---- free-running sessions (version 116; kernels: racinglmpc_amd/csrc/lmpc_relaunch.hip.h).  A car that has crossed the line starts its next lap inside the running
 * session, at its own crossing, while the other cars keep driving: the reference runs one car, whose next lap begins at the step after its crossing, from xF
 * (main.py:100-121, SysModel.py:50).  A session then holds G laps per car in about max_b sum_g T(b, g) steps and one begin / end. */
int lmpc_rollout_relaunch(lmpc_ctx *, int n, const int *cars /*n distinct*/, int lap_rows);
        /* Each listed car b -- it must have crossed the line, doneAt[b] >= 0 -- is put into the state a fresh lmpc_rollout_begin would give it for its next lap, on the
         * device: nothing of the lap is downloaded.  With s0 = lapStart[b] (0 until the car's first relaunch) and t = the steps the session has taken:
         * x[b] = finX[b] with the car's own TrackLength (its lmpc_track_set row, else the config's) subtracted from s, one FP64 subtraction (xF, SysModel.py:50);
         * xg[b] = finG[b]; xLin[b] = logged X rows s0 + 1 .. s0 + N + 1 and uLin[b] = logged U rows s0 + 1 .. s0 + N of the car (LMPC.addTrajectory,
         * PredictiveControllers.py:431-433); every other per-problem array of the step is zeroed for car b (the table of lmpc_arrays.h: hasPred, timeStep, the solver's
         * outputs and status words among them) and zt[b] = (0, 0, 0, 0, 10, 0) (LMPC.__init__ :330); statusAcc[b] = 0, doneAt[b] = -1, finX[b] = finG[b] = 0; the
         * session's count of finished cars goes down by one per listed car, so lmpc_rollout_run goes on and ends only when every car is done again.
         * Books: lapStart[b] = t, lapNo[b] += 1 (lmpc_rollout_lap_start).  From then on the car's timeStep counts the steps of its LAP, t + 1 - lapStart[b] (the
         * Q-function shift of the selection reads it), its lap is the session rows [lapStart[b], doneAt[b]), and doneAt[b] stays a SESSION row, one past the crossing.
         * Noise: in a session begun with noise = NULL (lmpc_rollout_set_noise) rows [t, min(T_max, t + lap_rows)) of the car's noise column are redrawn: the draws of
         * (seed, stream 0, lap0 + lapNo[b], step of the lap 0 .., car0 + b), lap0 the session's snapshot -- what a fresh session with that lap number holds in rows 0 ..
         * (lap_rows: the most steps the caller lets the lap take; beyond them the column keeps what it held).  In a session begun on a host array the car goes on
         * reading the caller's array at the SESSION step: the array is the caller's to lay out.
         * Regression laps: row b of the session's snapshot of the lap table is resolved anew from the table in force on the context now
         * (lmpc_model_set_lap_table; the other cars keep their rows; a session begun without a table, or no table in force now: no row changes).  The safe-set
         * table and the tuning rows are live in a session already.
         * Valid in an active session of lmpc_rollout_begin between two lmpc_rollout_run calls; both streams of the session are drained first.  One upload of the
         * entry table, one launch for all listed cars, one drain.  A session that never relaunches allocates, launches and returns what it did before this entry point
         * existed.  In a session that has relaunched, lmpc_rollout_commit_laps and lmpc_rollout_extend_laps count a car's rows from its lap start (rows == NULL:
         * doneAt - lapStart; rows[i] and n_rows are checked against t - lapStart[car]); lmpc_rollout_fetch is unchanged and returns session rows.
         * Everything is checked before anything changes, and lmpc_last_error names the car.  LMPC_E_ARG: n < 1, NULL cars, a car outside [0, B) or listed twice,
         * lap_rows < 1, a lap with fewer than N + 2 rows.  LMPC_E_STATE: no session active, a session of another kind (lmpc_rollout_begin_mpc, lmpc_rollout_pid), a
         * listed car with doneAt < 0, a session begun with parking or with a trace in force; and lmpc_rollout_lap_metrics after the first relaunch */
int lmpc_rollout_lap_start(lmpc_ctx *, int *start /*B, or NULL*/, int *lap /*B, or NULL*/);
        /* of the active session (LMPC_E_STATE without one): the session row each car's current lap began at, and the laps it has begun after its first.  A session
         * without a relaunch answers zeros for both.  No reference counterpart (one car, one lap at a time: main.py:100-121).  Needs no device */
/* ---- lap metrics of the active session reduced ON THE DEVICE (version 112; kernel: racinglmpc_amd/csrc/lmpc_metrics.hip.h).  What a sweep over thousands of cars
 * wants back per car and lap -- a lap time finer than one step, the distance kept from the lane edge and the input bounds, the cornering, the smoothness of the
 * inputs, the realised cost under the car's own weights -- as one row of LMPC_METRICS_NCOL doubles per listed car instead of its T x 14 logged ones. */
#define LMPC_METRICS_NCOL 20
enum { LMPC_MET_ROWS = 0,              /* T */
       LMPC_MET_T_CROSS = 1,           /* (T-1) + (TL - s_{T-1}) / (finX_s - s_{T-1}) when T == doneAt[c], else NaN: the line crossing (SysModel.py:45) interpolated
                                          between the last logged row and finX (the state right after the crossing step), in steps */
       LMPC_MET_NONFINITE_ROWS = 2,    /* rows with a non-finite value among the 14 logged ones: the entries to distrust */
       LMPC_MET_VX_MIN = 3, LMPC_MET_VX_MAX = 4, LMPC_MET_VX_SUM = 5,
       LMPC_MET_EY_ABSMAX = 6, LMPC_MET_EY_ABSMAX_ROW = 7,                 /* max |ey| and the FIRST row that attains it */
       LMPC_MET_EPSI_ABSMAX = 8,
       LMPC_MET_ALAT_ABSMAX = 9,       /* max |vx wz| */
       LMPC_MET_LANE_EXCESS_MAX = 10, LMPC_MET_LANE_EXCESS_ROWS = 11,     /* max over t, r of v; rows with some v > 0 */
       LMPC_MET_LANE_EXCESS_SUM = 12, LMPC_MET_LANE_EXCESS_SQSUM = 13,    /* sum_t sum_r v, sum_t sum_r v^2 */
       LMPC_MET_INPUT_MARGIN_MIN = 14, /* min over t and the four rows of bu_r - Fu_r u_t; negative: a bound was exceeded */
       LMPC_MET_DU0_SQSUM = 15, LMPC_MET_DU1_SQSUM = 16,                  /* sum_{t=1}^{T-1} (u_{t,j} - u_{t-1,j})^2, 0 at T = 1 */
       LMPC_MET_COST_STATE = 17,       /* sum_t (x_t - xRef)' Q (x_t - xRef) */
       LMPC_MET_COST_INPUT = 18,       /* sum_t u_t' R u_t */
       LMPC_MET_PATH_LENGTH = 19 };    /* sum_{t=1}^{T-1} sqrt((X_t - X_{t-1})^2 + (Y_t - Y_{t-1})^2) */
int lmpc_rollout_lap_metrics(lmpc_ctx *, int n, const int *cars /*n*/, const int *rows /*n, or NULL: doneAt[car]*/, double *out /*n x LMPC_METRICS_NCOL*/);
        /* Entry i covers rows t = 0 .. T-1 of car c = cars[i] as the session logged them, T = rows[i] or doneAt[c]: x_t = logX[t][c] (vx, vy, wz, epsi, s, ey),
         * u_t = logU[t][c], (X_t, Y_t) = logG[t][c][4:6] -- the arrays of lmpc_rollout_fetch.  TL is the car's own TrackLength (its lmpc_track_set row, else the
         * config's); Q, R, xRef, bx, bu come from the car's own tuning row (lmpc_tuning_set, else the config's; more than one row in force must be one per car of
         * the session, else LMPC_E_ARG); Fx, Fu are the context's; v_{t,r} = max(0, Fx_r x_t - bx_r) for the two lane rows.
         * The realised stage cost of buildCost (PredictiveControllers.py:228-257: x' Q x about xRef, u' R u, the input-rate term of dR, the slack terms of Qslack) is
         * composed by the caller, whose dR and Qslack they are:
         *     cost_state + cost_input + dR[0] du0_sqsum + dR[1] du1_sqsum + Qslack[0] lane_excess_sqsum + Qslack[1] lane_excess_sum.
         * Non-finite values: minima and maxima keep the first among equals and a comparison with NaN is false (the rule of the prefilter image,
         * lmpc_commit.hip.h), so a NaN is skipped -- an entry without a comparable value keeps -inf (maxima), +inf (minima) and row -1; counts count only true
         * comparisons; sums propagate NaN under IEEE rules; nonfinite_rows tells which entries to distrust.  A non-finite car does not affect any other entry.
         * Every term and the order of the reduction are stated in the kernel's header; the order depends on T alone, so a result can be reproduced on the host
         * bit for bit (tests/metrics_ref.py).
         * Valid in an active session of any kind (lmpc_rollout_begin, _begin_mpc, _pid) with at least one step taken; a car may be listed more than once.  The rules
         * of lmpc_rollout_commit_laps, everything checked before the launch: LMPC_E_ARG for n < 1, NULL cars or out, a car outside [0, B), rows[i] < 1, rows[i] beyond
         * what the session logged for that car (the steps taken; a parked car's parking step; for a car of a stop_at_line PID session its crossing step);
         * LMPC_E_STATE with no session active, or when rows == NULL and a listed car has doneAt < 0 (lmpc_last_error names the car).  `out` is written only on
         * success.  Reads only: no store and no session state changes.  One upload of the entry table, one launch, one download of n x LMPC_METRICS_NCOL doubles.
         * No reference counterpart beyond the lines named (the reference reports lap times in whole steps, main.py:113-121) */
int lmpc_debug_model_image(lmpc_ctx *, int lap /*insertion index*/, unsigned *q /*3 x (rows-1)*/, double *par /*chunks used x 6*/, int *chunks);
        /* the prefilter image of one regression-store lap as the regression kernel reads it (the scan of PredictiveModel.py:180-197 on 16-bit fixed point): three planes
         * of packed words (vx | vy << 16), (wz | delta << 16), (a) over rows 0 .. rows-2, and per 1024-row chunk the five minima and the common scale.  Available in every
         * build; tests compare the image of a committed lap with that of an uploaded one.  Any output may be NULL.  No reference counterpart */
int lmpc_lti_regression(int device, const double *x /*T x 6*/, const double *u /*T x 2*/, int T, double lamb,
                        double *A /*6 x 6*/, double *B /*6 x 2*/, double *Error /*2 x 6: max; min of the fit residual*/, int *status /*or NULL*/);
        /* Utilities.Regression, fnc/Utilities.py:5-28 (main.py:74-77: the LTI model of the path-following MPC); ridge least squares over one lap */

int lmpc_lti_regression_batch(int device, int B, const double *x /*B x ldT x 6*/, const double *u /*B x ldT x 2*/, const int *T /*B: rows of lap b, 3 <= T[b] <= ldT*/, int ldT,
                              double lamb, double *A /*B x 6 x 6*/, double *Bm /*B x 6 x 2*/, double *Error /*B x 2 x 6*/, int *status /*B or NULL*/);
        /* Utilities.Regression (fnc/Utilities.py:5-28) for B laps in one launch (one work-group per lap; main.py:74-77 for a batch of PID laps).  lmpc_lti_regression is
         * its B = 1 call: same bits */

/* ---- multi-GPU: one process per GPU, RCCL over xGMI.  The QPs / rollouts of a batch are independent given the
 * read-only safe set, so the data path has no collective; the ONE exchange is per lap.  The reference has no counterpart (single
 * process); what is exchanged are the arguments of LMPC.addTrajectory / PredictiveModel.addTrajectory (:418-445, PredictiveModel.py:35-46).
 * The 128-byte id is created on rank 0 and handed to the other processes by the caller (racinglmpc_amd/parallel.py). */
#define LMPC_COMM_ID_BYTES 128
int lmpc_comm_unique_id(unsigned char *id /*LMPC_COMM_ID_BYTES*/);                       /* ncclGetUniqueId */
int lmpc_comm_init(lmpc_ctx *, const unsigned char *id, int rank, int world);            /* ncclCommInitRank on the ctx's device */
int lmpc_comm_destroy(lmpc_ctx *);
int lmpc_comm_info(lmpc_ctx *, int *rank, int *world, int *is_rccl);
int lmpc_comm_allgather_dev(lmpc_ctx *, const void *send_dev, void *recv_dev /*world x bytes*/, long long bytes);   /* ncclAllGather, async on the ctx stream */
int lmpc_comm_allgather(lmpc_ctx *, const void *send_host, void *recv_host /*world x bytes*/, long long bytes);     /* same for small host-side control data */
int lmpc_comm_allreduce_max(lmpc_ctx *, double *v /*n, in/out, host*/, int n);
int lmpc_comm_barrier(lmpc_ctx *);                                                       /* stream drained on every rank */
int lmpc_rollout_exchange(lmpc_ctx *, int K, int T_max, double *records /*world x K x (T_max+1) x 14*/, long long *lens /*world x K, -1 = empty*/,
                          int *n_valid_local);
        /* per-lap exchange of the current rollout session: the rank's K fastest valid laps (finished, <= T_max steps, status clean) are
         * packed on the device from the session logs -- rows t < T: x_t | u_t | x_glob_t, row T_max: state and global state right after the
         * finish line, rollout index -- and all-gathered; every rank receives the same world x K records */

int lmpc_selftest(lmpc_ctx *);                   /* device self test of the cross-lane reduction primitives */
/* Developer switch (environment, read at lmpc_create): LMPC_MW_MAX_BATCH=<n> overrides the largest batch that runs four waves per
 * QP (default: the number of CUs; 0 forces the one-wave kernel everywhere).  Results do not depend on it beyond summation order. */
int lmpc_solver_waves(lmpc_ctx *, int B);         /* wavefronts per QP the solve kernel uses for a batch of B (4 or 2: lmpc_solve_kernel_mw, 1: lmpc_solve_kernel) */
int lmpc_solver_lds(lmpc_ctx *, unsigned long long out4[4]);
        /* what the routes of this context's (N, numSS_points) are chosen from: dynamic LDS per QP, in bytes, of the one-wave kernel with [A_k | B_k] in LDS, of the
         * one-wave kernel with [A_k | B_k] in global memory (0: this (N, numSS_points) has none) and of the multi-wave kernels (0: none -- the runtime kernel, and a
         * fixed (N, numSS_points) whose multi-wave layout exceeds the 160 KB of a CU: one wave per QP at every batch size); out4[3]: CUs of the device */
int lmpc_set_profiling(lmpc_ctx *, int every);    /* 0: off; k > 0: HIP events on the launch stream around every k-th launch of each kernel (an event
                                                     record costs ~4 us of stream time: k = 1 adds 15 us to a two-kernel step) */
int lmpc_get_stats(lmpc_ctx *, lmpc_stats *out);  /* drains pending events */
int lmpc_reset_stats(lmpc_ctx *);

/* ---- developer entry points.  They exist in every build, but only the flavours built with the named macro carry the code behind them
 *      (racinglmpc_amd.build.build_flavour); in the product library both return LMPC_E_ARG and say so in lmpc_last_error. ---- */
int lmpc_debug_set_trace(lmpc_ctx *, double *dev_rows /* max_batch x 48 x 6 doubles of device memory, or NULL */);
        /* -DLMPC_TRACE: every later solve launch records, per problem and interior-point iteration, (gap, r_d, r_e | sigma, alpha_p, alpha_d) --
         * the columns of tests/ipm_model.py's trace, for a differential comparison of kernel and model (tools/n40_model.py) */
int lmpc_debug_rollout_peek(lmpc_ctx *, double *xLin /*B x (N+1) x 6*/, double *uLin /*B x N x 2*/, int *status /*B*/, int *rstatus /*B x N*/);
        /* (every build) the rollout session's current linearisation trajectories -- the queries of the NEXT step's regression -- and the status words of the step
         * just taken; any pointer may be NULL.  tools/robustness_sweep.py captures the inputs of a flagged closed-loop regression with it */
int lmpc_debug_rollout_capture(lmpc_ctx *, int on);
        /* (every build) sessions begun after this call also keep the selected safe-set points / Q-values of the step just taken (B x S x 6, B x S): off by default,
         * the rollout step then does not write them */
int lmpc_debug_rollout_qp(lmpc_ctx *, int b0, int n, double *A, double *B, double *C, double *xPred, double *uPred, double *ssSel, double *qSel, double *succ, double *succU,
                          double *lambda, double *ztNext, double *ztuNext, int *iters, int *status);
        /* (every build) the QP the LAST simulated step solved for rollouts b0 .. b0 + n - 1: the regression's A, B, C, the kernel's answer (xPred, uPred, lambda, zt / zt_u),
         * and (capture on) the selection with its successor rows -- what tests/closed_loop_probe.py hands to the oracle; x0 / uOld are rows t - 1 / t - 2 of the
         * session's logs.  Any pointer may be NULL */
int lmpc_debug_k1_ahead(lmpc_ctx *, long long out[2]);
        /* (every build) regression launches of lmpc_step_batch_dev since lmpc_create: out[0] chained (on the look-ahead stream, beside the previous step's solve),
         * out[1] unchained (on the context's stream); the fused step launches no regression and counts as neither */
int lmpc_debug_k1_merge(lmpc_ctx *, long long out[3]);
        /* (every build) since lmpc_create: out[0] two-role launches (a held solve and the next step's regression), out[1] held solves launched stand-alone (a flush),
         * out[2] regression launches of lmpc_step_batch_dev in a kernel of their own (chained or not).  A step whose regression rode in a two-role launch still counts
         * as chained in lmpc_debug_k1_ahead */
int lmpc_debug_exec_audit(lmpc_ctx *, unsigned long long *out16, int reset);
        /* -DLMPC_EXEC_AUDIT: out16[site] = calls of a cross-lane primitive (DPP / permlane / bpermute reductions, MFMA stages) of the built-in
         * kernels that found an incomplete EXEC mask, out16[8 + site] = calls; sites are listed in csrc/lmpc_kernels.hip.h */

#ifdef __cplusplus
}
#endif
#endif /* LMPC_HIP_H */
