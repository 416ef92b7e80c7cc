// racinglmpc_amd/csrc/lmpc_capi.hip -- host side of liblmpc_hip.so: the C ABI declared in include/lmpc_hip.h.
// Owns the device lap stores, work buffers, stream and HIP-event timers; launches the kernels of
// lmpc_kernels.hip.h.  No CPU compute path exists here: if HIP fails, the call fails.
#include "lmpc_variant.hip.h"
#include "lmpc_noise.hip.h"
#include "lmpc_track.hip.h"
#include "lmpc_commit.hip.h"
#include "lmpc_retain.hip.h"
#include "lmpc_metrics.hip.h"
#include "lmpc_trace.hip.h"
#include "lmpc_live.hip.h"
#include "lmpc_relaunch.hip.h"
#include "lmpc_arrays.h"
#include "lmpc_rows.h"
#include "lmpc_pick.h"
#include "lmpc_retain.h"
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

static thread_local std::string g_err;
static int set_err(int code, const char *what, const char *detail) {
    g_err = std::string(what) + ": " + (detail ? detail : "");
    // A failed HIP call also stays behind as the thread's "last error", and the launch checks below read that with hipGetLastError(): reported here, it is consumed
    // here -- an allocation that did not fit (lmpc_create, lmpc_dev_alloc) must not come back as the result of the next entry point's kernel launch.
    if (code == LMPC_E_HIP) (void)hipGetLastError();
    return code;
}
// Developer knobs read from the environment (round 6, ADVICE r5: a stray variable must not change behaviour silently).  Every knob that is SET is recorded
// here, announced once on stderr and listed by lmpc_active_knobs(); knobs that change RESULTS (LMPC_NO_RETRY) exist in developer flavours only.
static std::mutex g_knob_mu;
static std::string g_knobs;
static const char *dev_knob(const char *name) {
    const char *e = getenv(name);
    if (e) {
        std::lock_guard<std::mutex> lk(g_knob_mu);
        const std::string item = std::string(name) + "=" + e;
        if ((";" + g_knobs + ";").find(";" + item + ";") == std::string::npos) {
            g_knobs += (g_knobs.empty() ? "" : ";") + item;
            fprintf(stderr, "liblmpc_hip: developer knob %s is active\n", item.c_str());
        }
    }
    return e;
}
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return set_err(LMPC_E_HIP, #call, hipGetErrorString(e_)); } while (0)
#define ARGCHK(cond) do { if (!(cond)) return set_err(LMPC_E_ARG, "argument check failed", #cond); } while (0)
#define RCCHK(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// ---- device allocations of a context.  Builds with -DLMPC_GUARD (the "asan" developer flavour, racinglmpc_amd.build: host code under AddressSanitizer) put a
// 256-byte guard zone filled with 0xA5 behind every allocation -- and between the work-buffer ranges of the two slabs -- and check it when the buffer is
// freed (lmpc_destroy, store growth, end of a rollout session): a kernel that wrote past a buffer's end is reported on stderr and counted
// (lmpc_debug_guard_failures).  Ordinary builds: plain hipMalloc / hipFree.
#define LMPC_GUARD_BYTES 256
static int g_guard_failures = 0;
#ifdef LMPC_GUARD
#define LMPC_SLAB_GAP LMPC_GUARD_BYTES      // (a zone behind every work-buffer range of the slabs as well, see check_slab_gaps)
#include <map>
#include <mutex>
static std::map<void *, size_t> g_guarded; static std::mutex g_guard_mu;
static int check_guard_zone(const void *zone, const char *what) {
    unsigned char h[LMPC_GUARD_BYTES];
    if (hipMemcpy(h, zone, LMPC_GUARD_BYTES, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    for (int i = 0; i < LMPC_GUARD_BYTES; i++) if (h[i] != 0xA5) {
        fprintf(stderr, "liblmpc_hip GUARD: %s: byte %d behind the buffer was overwritten (0x%02x)\n", what, i, h[i]); g_guard_failures++; return 1; }
    return 0;
}
static hipError_t g_malloc_raw(void **p, size_t bytes) {
    const size_t padded = (bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(p, padded + LMPC_GUARD_BYTES);
    if (e != hipSuccess) return e;
    e = hipMemset((char *)*p + padded, 0xA5, LMPC_GUARD_BYTES);
    std::lock_guard<std::mutex> lk(g_guard_mu); g_guarded[*p] = padded;
    return e;
}
static hipError_t g_free(void *p) {
    if (!p) return hipSuccess;
    size_t padded = 0; bool known = false;
    { std::lock_guard<std::mutex> lk(g_guard_mu); auto it = g_guarded.find(p); if (it != g_guarded.end()) { padded = it->second; known = true; g_guarded.erase(it); } }
    if (known) { (void)hipDeviceSynchronize(); check_guard_zone((char *)p + padded, "device buffer"); }
    return hipFree(p);
}
#else
#define LMPC_SLAB_GAP 0
static hipError_t g_malloc_raw(void **p, size_t bytes) { return hipMalloc(p, bytes); }
static hipError_t g_free(void *p) { return p ? hipFree(p) : hipSuccess; }
#endif
template <class T> static hipError_t g_malloc(T **p, size_t bytes) { return g_malloc_raw((void **)p, bytes); }

struct evpair { hipEvent_t a, b; int kind; };
// the device image of a row set (lmpc_rows.h), filled by image_upload; cap: the bytes allocated
struct dev_image { void *p; size_t cap; };
enum { IMG_LT = 0, IMG_SST, IMG_TUNE, IMG_TRK, IMG_COUNT };

struct lmpc_ctx {
    lmpc_config cfg;
    int init_max_laps;                       // cfg.max_laps as lmpc_create was given it (growth overwrites cfg.max_laps): the capacities lmpc_store_retain shrinks to are this times 2^j
    lmpc_dev_params dp;
    hipStream_t stream;
    double *mstore, *sstore;                 // device lap stores [lap][col][row]
    unsigned *mquant; double *mqpar; int mq_chunks;   // K1 prefilter image of the model store (lmpc_commit.hip.h: commit_quantise)
    std::vector<int> m_order, m_len;         // model: sorted position -> slot ; length per slot
    std::vector<int> s_len;                  // safe set: rows per lap (incl. addPoint extensions)
    std::vector<int> s_laptime;              // LMPC.LapTime (rows at addTrajectory time)
    std::vector<double> s_qlast, s_q0;       // last / first Qfun value per lap
    std::vector<int> s_override;             // explicit selection (lmpc_ss_set_selected)
    // Device work buffers of the host-pointer entry points, sized for max_batch: one pointer per array of lmpc_arrays.h, each a range of two device slabs
    // (inputs | outputs, laid out by lmpc_slab_layout).  Small contexts also own host-mapped mirrors of both slabs (h_in / h_out) with the same layout: hm holds
    // the host address of every range, dm the address the device sees -- a full batch of lmpc_step_batch then copies nothing, the kernels read and write the mirrors.
    lmpc_arrays w, hm, dm;
    lmpc_dims dims;                          // (N, S, numSS_it) the per-problem sizes of lmpc_arrays.h are taken at
    char *slab_in, *slab_out, *h_in, *h_out;
    lmpc_variant_api var;                    // launchers of the (N, numSS_points) instantiation of the solve kernels in use
    void *var_dl;                            // dlopen handle when that instantiation lives in its own shared object (lmpc_variant.hip)
    int mw_max_batch, mw2_max_batch, n_cu;   // largest batch served by the four-wave / the two-wave solve kernel
    bool k1_force16;                         // regression kernel: never the 8-rows-per-lane scan (launch_k1)
    int k1_qg_force;                         // (experiments, LMPC_K1_QG at lmpc_create: queries per work-group of the regression kernel; 0 = the rule of k1_grid)
    int fuse_k1;                             // fused step for one-wave batches (LMPC_FUSE=0 turns it off)
    double *ab_pack;                         // global scratch of the one-wave kernel's long-horizon variant ([A_k | B_k] per problem), max_batch x 48 N doubles
    int cd_ok, cd_hasq, cd_mode;             // condensed one-wave kernel (opt-in: libraries built with -DLMPC_WITH_CD only): usable for this configuration / state cost present / LMPC_CD=1 in the environment selects it, at every batch size
    int profiling; bool ev_open; std::vector<evpair> events; lmpc_stats stats;
    // retry pass on demand: launches since the last drain of the stream, the host-mapped ring the kernels flag themselves in, launch counter
    struct pending_solve { lmpc_solve_io io; int B; int epoch; lmpc_dev_params dp; bool shared_abc; };   // dp: the parameter block (selected laps, store pointers) of the launch
    std::vector<pending_solve> pending; int *h_retry, *d_retry; int epoch;
    size_t ab_pack_cap;                      // problems ab_pack holds
    void *scr_dev; size_t scr_bytes;         // pooled scratch of the host-buffer entry points (pooled_scratch: staged laps and launch tables of the stores, plant step, global position)
    std::vector<char *> gaps;                // guard builds: the 256-byte zones between the work-buffer ranges of the slabs
    unsigned create_flags; int solver_kind;  // lmpc_create_ex flags; which solve kernels serve this context: 0 built-in, 1 variant library, 2 the runtime-(N, S) kernel
    int dbg_capture;                         // lmpc_debug_rollout_capture: rollout sessions also keep the selected safe-set points of the last step (parity probes of the closed loop)
    double *dbg_trace;                       // developer builds (-DLMPC_TRACE): device buffer of the per-iteration side channel, see lmpc_debug_set_trace
    double tr_s[4]; long long tr_n;          // developer trace of lmpc_step_batch's one-QP path (lmpc_debug_step_trace): seconds spent staging / launching / waiting / unstaging
    struct lmpc_rollout_session *ro;
    int noise_on; unsigned long long noise_seed, noise_lap; long long noise_car0;   // lmpc_rollout_set_noise: sessions begun with noise = NULL fill their buffer on the device (lmpc_noise.hip.h); 0 after lmpc_create
    std::vector<int> trace_cars; unsigned trace_what;   // lmpc_rollout_set_trace: the cars and planes later sessions record at every step (lmpc_trace.hip.h); empty / 0 after lmpc_create
    std::vector<int> park_cars; unsigned park_mode;     // lmpc_rollout_set_parking: the cars later sessions park from step 0 and the LMPC_PARK_* bits (lmpc_live.hip.h); empty / 0 after lmpc_create
    // The per-car row sets (lmpc_rows.h: the rows as the caller gave them, 0 rows = the config's value, one row serves all, else row b for problem b) and img[], their device images.
    lmpc_row_set<double> plant{LMPC_PLANT_NPAR, "lmpc_plant_set_params"};   // vehicle constants (0 rows: the reference's vehicle, the kernels with the literals); no image: a call uploads its cars' rows
    // trToUse insertion indices per row (0 rows: the first trToUse laps of the sorted order serve every problem).  img[IMG_LT]: the same rows as resolved (slot, rows)
    // pairs in each row's sorted order, uploaded by `set` and rebuilt when the stores move or a lap is replaced (resolve_lap_table); lt_small: every lap named anywhere
    // has at most 512 rows, i.e. the 8-rows-per-lane scan serves the whole table (launch_k1)
    lmpc_row_set<int> lt{0, "lmpc_model_set_lap_table"}; bool lt_small;
    // numSS_it safe-set lap indices per row and (sst_has_last) one "latest lap" index per row.  img[IMG_SST]: the rows as the solve kernels read them (LMPC_SSTAB_ENTRY
    // ints per entry: slot, current rows, latest flag, pad; each row in ascending LapTime, ties by index).  The image names rows of laps, so every edit of the safe set
    // marks it dirty and the next launch that reads it uploads it again (ss_table_for)
    lmpc_row_set<int> sst{0, "lmpc_ss_set_lap_table"}; std::vector<int> sst_last; bool sst_has_last, sst_dirty;
    // LMPC_TUNING_NPAR doubles per row (0 rows: the config's weights serve every problem).  img[IMG_TUNE]: what the per-problem-rows instantiations of the solve kernels and
    // the assemble kernel stage from -- PAR_TOT doubles per row in the PAR_* layout, doubled weights, Fx / Fu of the config; with no rows in force it holds the config's
    // own row (what a launch with a safe-set table alone reads).  Uploaded by `set`, never per launch
    lmpc_row_set<double> tune{LMPC_TUNING_NPAR, "lmpc_tuning_set"};
    // LMPC_TRACK_NPAR doubles per row (0 rows: the config's track, read from the parameter block by the kernels that ran before there were rows).  img[IMG_TRK]: the rows, uploaded by `set`
    lmpc_row_set<double> trk{LMPC_TRACK_NPAR, "lmpc_track_set"};
    dev_image img[IMG_COUNT];
    // Look-ahead regression (step_dev).  Queued steps: the regression of step i + 1 needs nothing of step i's solve, so it runs on k1_stream beside it, ordered by
    // stream events only -- e_k1 behind a regression launch, e_front on `stream` in front of a solve launch of step_dev.  It writes the hand-over set the solve in
    // flight is NOT reading: ho[0] is the work buffers' A / Bm / C / rstatus, ho[1] a second set allocated by the first chained step; ho_cur: the set the last step used.
    // chain: the previous call on this context that could enqueue work, or edit what a regression reads, was a two-kernel step_dev (ctx_enter clears it).
    struct handover { double *A, *Bm, *C; int *rstatus; };
    hipStream_t k1_stream; hipEvent_t e_k1, e_front; handover ho[2]; int ho_cur;
    int k1_ahead, k1_ahead_max_batch; bool chain, sst_upload_broke; long long n_k1_chained, n_k1_unchained;   // k1_ahead: LMPC_K1_AHEAD=0 at lmpc_create turns it off (the step of before: one stream, the caller's A / Bm / C as the hand-over)
    // Held solve (step_dev, the merged form of the look-ahead): on a route with a two-role build of the solve kernel (lmpc_variant_api::launch_mw4_next) the solve of a
    // chained step is not launched by its own call.  The next step_dev launches it in ONE launch with its own regression (no event packet between two solves: nothing
    // but kernels in the queue); every other entry point launches it stand-alone first thing (ctx_enter), so each of them sees the order it always saw.  `held` is all
    // launch_solve would have been given plus the parameter block of the step's call; has_held: there is one.  lmpc_destroy drops it.
    struct held_solve { lmpc_solve_io io; int B; lmpc_dev_params dp; lmpc_k1_also retry_abc; };
    held_solve held; bool has_held;
    int k1_merge, k1_merge_qg;               // LMPC_K1_MERGE=0 / LMPC_CREATE_NO_K1_MERGE: the two-stream look-ahead for every chained step;  the cap of the queries per regression work-group of a two-role launch
    long long n_merged, n_held_flushed, n_k1_alone;   // two-role launches; held solves launched stand-alone; regression launches of step_dev in a kernel of their own
    void *comm; int comm_rank, comm_world;   // RCCL communicator of this rank (lmpc_comm.hip.h); null = single process
    void *comm_scr, *comm_scr_h; size_t comm_scr_bytes;   // communicator scratch: device allocation + pinned host mirror (lmpc_comm.hip.h: comm_scratch)
};

// a device-resident rollout session (lmpc_rollout_*, below the stores section, which commits a session's logs and therefore sees the struct)
struct lmpc_rollout_session {
    bool active;                                                // between lmpc_rollout_begin and lmpc_rollout_end; the buffers outlive the session (see lmpc_rollout_begin)
    int B, T_max, t;
    int kind, stop_at_line;                                     // RO_LMPC / RO_LTV / RO_LTI / RO_PID (what one simulated step launches); 0: the run does not end when every car has crossed the line
    double *d_noiseU, *d_vt;                                    // RO_PID only: controller noise T_max x B x 2, target speed per car
    unsigned long long nz_seed, nz_lap; long long nz_car0;      // the session's snapshot of the noise source (lmpc_rollout_set_noise), taken when it begins
    int *d_lt; bool has_lt, lt_small; int lt_stride;            // the session's snapshot of the lap table (resolved (slot, rows) pairs, B x trToUse x 2), taken when it begins; has_lt: the table builds of the regression kernel run
    const double *trk; int trk_stride;                          // the context's track image for this session's cars (null: the config's track); lmpc_track_set is refused while the session is active
    double *d_par; bool has_par;                                // the session's snapshot of the per-car vehicle constants (B x LMPC_PLANT_NPAR), taken when it begins; has_par: the PAR kernels run
    hipStream_t pstream; hipEvent_t e_solved, e_plant;          // plant integration runs beside the next regression (lmpc_rollout_plant_kernel)
    std::vector<void *> keep;
    // what the session shares with a step, by the names and sizes of lmpc_arrays.h (x0: the cars' states).  Never allocated: mu, ztUsed, selStart; ssSel, qSel, succ,
    // succU only with lmpc_debug_rollout_capture on (else null: the step does not write them)
    lmpc_arrays a;
    double *d_xg, *d_logX, *d_logU, *d_logG, *d_noise, *d_finX, *d_finG;
    int *d_done, *d_nDone, *d_stAcc;
    // the session's snapshot of the trace (lmpc_rollout_set_trace), taken when it begins: tr_n listed cars (0: no trace, nothing below exists), the planes recorded;
    // d_trCars: the list on the device, uploaded per begin; the planes [T_max][tr_n][...] belong to the kept set and are reused while B, T_max, tr_n, tr_what stay;
    // the trace kernel runs on the plant stream behind the plant kernel (lmpc_rollout_run); tstream / e_trace serve the measured alternative, tr_own_stream
    int tr_n; unsigned tr_what; int *d_trCars;
    double *tr_x, *tr_u, *tr_ss, *tr_q, *tr_xy, *tr_xys; int *tr_it, *tr_st, *tr_map;
    hipStream_t tstream; hipEvent_t e_trace;
    // the session's snapshot of the parking (lmpc_rollout_set_parking), taken when it begins.  parked: the step's kernels run over d_live[0 .. nLive), the ascending
    // list of the cars still stepped (lmpc_live.hip.h); pk_mode: the bits that act in this session (LMPC_PARK_FINISHED only where it stops at the line); pk_n0: cars
    // parked from step 0; nd_host: nDone as the last poll read it.  d_live / d_parkedAt / d_park0 (B ints each) are allocated by the first parking session on the
    // kept buffers; d_nDone holds four ints: nDone, nLive, nDone at the last rebuild, unused
    bool parked; unsigned pk_mode; int pk_n0, nLive, nd_host; int *d_live, *d_parkedAt, *d_park0;
    bool tr_own_stream;                                         // (developer knob LMPC_TRACE_OWN_STREAM=1, read when a traced session begins: the trace kernel on a stream of its own beside the plant, the next solve waiting for a second event -- the A / B of tools/trace_bench.py, measured slower; same bits)
    // lap changes inside the session (lmpc_rollout_relaunch; lmpc_relaunch.hip.h).  relaunched: this session has made one -- until then nothing below is read and the
    // session launches what it always did.  lapStart[b]: the session row car b's current lap began at; lapNo[b]: laps it has begun after its first (host books; the
    // shift kernel reads d_lapStart, B ints allocated on the kept buffers by the first relaunch).  nz_dev: begun with noise = NULL, the buffer is the device
    // generator's.  lt_host: the resolved rows d_lt holds, so that lt_small stays right when one row is replaced
    bool relaunched, nz_dev; int *d_lapStart; std::vector<int> lapStart, lapNo, lt_host;
};
// the session row car `car`'s current lap began at (0 in a session that has not relaunched)
static int session_lap_start(const lmpc_rollout_session *r, int car) { return r->relaunched ? r->lapStart[(size_t)car] : 0; }

enum { RO_LMPC = 0, RO_LTV = 1, RO_LTI = 2, RO_PID = 3 };

// How every entry point that enqueues on the context's stream, or edits what a regression reads (lap stores and their images, lap table, track rows, parameter
// images, a device array of the caller's), begins: the context's device, and the chain of look-ahead regressions broken -- the next step_dev runs its regression
// on the context's stream again, behind whatever this call queues.  step_dev alone sets the flag, at its end.
// A held solve (lmpc_ctx::held) is launched here, stand-alone on the context's stream, before the entry point does anything else: a store edit, an upload, a drain or a
// download then finds the stream as it would be had every step launched its own solve.  keep_held: step_dev, which decides itself what becomes of it.
static int launch_held(lmpc_ctx *c, const lmpc_k1_next *next);
static int ctx_enter(lmpc_ctx *c, bool keep_held = false) {
    c->chain = false;
    if (const hipError_t e = hipSetDevice(c->cfg.device)) return set_err(LMPC_E_HIP, "hipSetDevice(c->cfg.device)", hipGetErrorString(e));
    if (c->has_held && !keep_held) return launch_held(c, nullptr);
    return LMPC_OK;
}

#ifdef LMPC_DEV_FAST
// developer build (racinglmpc_amd.build.build_flavour("dev", ["LMPC_DEV_FAST"])): only the N = 12 variants, seconds to compile; LMPC_FORCE_NW=<1|2|4>
// picks the waves per QP at every batch size (1 = the one-wave kernel)
#ifndef LMPC_DEV_N
#define LMPC_DEV_N 12
#endif
static bool builtin_variant(lmpc_variant_api *v, int n, int s) {
    if (n == LMPC_DEV_N && s == 48) return lmpc_variant_fill<LMPC_DEV_N, 48>(v);
    return n == LMPC_DEV_N && s == 0 && lmpc_variant_fill<LMPC_DEV_N, 0>(v);
}
#else
template <int N, int S> static bool try_builtin(lmpc_variant_api *v, int n, int s) { return n == N && s == S && lmpc_variant_fill<N, S>(v); }
static bool builtin_variant(lmpc_variant_api *v, int n, int s) {    // the reference's configurations (main.py:43 N = 14, BASELINE N = 12 / 40) are part of the library
    return try_builtin<8, 0>(v, n, s) || try_builtin<12, 0>(v, n, s) || try_builtin<14, 0>(v, n, s) || try_builtin<20, 0>(v, n, s) || try_builtin<40, 0>(v, n, s) ||
           try_builtin<8, 48>(v, n, s) || try_builtin<12, 48>(v, n, s) || try_builtin<14, 48>(v, n, s) || try_builtin<20, 48>(v, n, s) || try_builtin<40, 48>(v, n, s);
}
#endif
// any other (N, numSS_points): liblmpc_var_N<N>_S<S>.so next to this library
static int load_variant(lmpc_ctx *c, int n, int s) {
    Dl_info info;
    if (!dladdr((const void *)&load_variant, &info) || !info.dli_fname) return set_err(LMPC_E_VARIANT, "variant lookup", "cannot locate liblmpc_hip.so");
    std::string dir(info.dli_fname); const size_t sl = dir.rfind('/'); dir = sl == std::string::npos ? std::string(".") : dir.substr(0, sl);
    char name[96]; snprintf(name, sizeof(name), "/liblmpc_var_N%d_S%d.so", n, s);
    const std::string path = dir + name;
    void *h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) return set_err(LMPC_E_VARIANT, "solve-kernel variant not built (racinglmpc_amd.build.build_variant(N, numSS_points) makes it)", path.c_str());
    typedef int (*get_t)(lmpc_variant_api *, int);
    get_t get = (get_t)dlsym(h, "lmpc_variant_get");
    const int rc = get ? get(&c->var, LMPC_VARIANT_ABI) : -1;
    if (rc != 0 || c->var.N != n || c->var.S != s) { dlclose(h); return set_err(rc == -2 ? LMPC_E_ARG : LMPC_E_VARIANT, rc == -2 ? "variant exceeds the LDS of a CU" : "stale or foreign variant library (rebuild it)", path.c_str()); }
    c->var_dl = h;
    return LMPC_OK;
}
static int pick_solver(lmpc_ctx *c) {
    const int n = c->cfg.N, s = c->cfg.numSS_it > 0 ? c->cfg.numSS_points : 0;
    c->solver_kind = 0;
    if (!(c->create_flags & LMPC_CREATE_FORCE_RUNTIME_KERNEL)) {
        if (builtin_variant(&c->var, n, s)) return LMPC_OK;
        c->solver_kind = 1;
        const int rc = load_variant(c, n, s);
        if (rc == LMPC_OK || !(c->create_flags & LMPC_CREATE_RUNTIME_KERNEL)) return rc;
    }
    // no built-in instantiation, no variant library (and nobody to compile one): the runtime-(N, S) kernel (lmpc_solve_rt.hip.h)
    c->solver_kind = 2;
    if (!lmpc_variant_fill_rt(&c->var, n, s)) return set_err(LMPC_E_ARG, "runtime solve kernel", "this (N, numSS_points) exceeds the LDS of a CU");
    return LMPC_OK;
}

extern "C" {

const char *lmpc_last_error(void) { return g_err.c_str(); }
const char *lmpc_active_knobs(void) { std::lock_guard<std::mutex> lk(g_knob_mu); static thread_local std::string copy; copy = g_knobs; return copy.c_str(); }
int lmpc_version(void) { return 116; }
int lmpc_device_memory(int device, unsigned long long *free_bytes, unsigned long long *total_bytes) {
    ARGCHK(free_bytes && total_bytes && device >= 0);
    size_t f = 0, t = 0;
    HIPCHK(hipSetDevice(device)); HIPCHK(hipMemGetInfo(&f, &t));
    *free_bytes = (unsigned long long)f; *total_bytes = (unsigned long long)t;
    return LMPC_OK;
}

int lmpc_config_default(lmpc_config *c) {
    if (!c) return LMPC_E_ARG;
    memset(c, 0, sizeof(*c));
    c->N = 12; c->numSS_it = 4; c->numSS_points = 48; c->trToUse = 4; c->maxNumPoint = 7;
    c->h = 5.0; c->lamb = 0.0; c->dt = 0.1;
    const double sc[5] = {0.1, 1, 1, 1, 1}; memcpy(c->scaling, sc, sizeof(sc));
    c->dR[0] = 5.0; c->dR[1] = 50.0; c->Qslack[0] = 5.0; c->Qslack[1] = 25.0;       // initControllerParameters.py:50-54
    for (int i = 0; i < 6; i++) c->QtermSlack[i * 7] = 500.0;
    c->Fx[5] = 1.0; c->Fx[11] = -1.0; c->bx[0] = c->bx[1] = 0.4;
    const double fu[8] = {1, 0, -1, 0, 0, 1, 0, -1}; memcpy(c->Fu, fu, sizeof(fu));
    c->bu[0] = c->bu[1] = 0.5; c->bu[2] = c->bu[3] = 10.0;
    c->track_rows = 0; c->trackLength = 0.0;
    c->device = 0; c->max_batch = 256; c->max_laps = 64; c->max_lap_len = 2048;
    c->tol_gap = 1e-11; c->tol_res = 1e-9; c->reg_lambda = 1e-6; c->max_iter = 40; c->slacks = 1;
    return LMPC_OK;
}

static void fill_params(lmpc_ctx *c) {
    const lmpc_config &f = c->cfg; lmpc_dev_params &p = c->dp;
    memset(&p, 0, sizeof(p));
    p.N = f.N; p.L = f.numSS_it; p.S = f.numSS_it > 0 ? f.numSS_points : 0; p.ppl = f.numSS_it > 0 ? f.numSS_points / f.numSS_it : 0;
    p.trToUse = f.trToUse; p.maxNumPoint = f.maxNumPoint; p.h = f.h; p.lamb = f.lamb; p.dt = f.dt;
    memcpy(p.scaling, f.scaling, sizeof(p.scaling));
    for (int i = 0; i < 36; i++) { p.Q2[i] = 2 * f.Q[i]; p.Qf2[i] = 2 * f.Qf[i]; }
    for (int i = 0; i < 4; i++) p.R2[i] = 2 * f.R[i];
    p.dR2[0] = 2 * f.dR[0]; p.dR2[1] = 2 * f.dR[1]; p.a_s = 2 * f.Qslack[0]; p.c_s = f.Qslack[1];
    for (int i = 0; i < 6; i++) { p.T2[i] = 2 * f.QtermSlack[i * 7]; p.xRef[i] = f.xRef[i]; }
    memcpy(p.Fx, f.Fx, sizeof(p.Fx)); memcpy(p.bx, f.bx, sizeof(p.bx)); memcpy(p.Fu, f.Fu, sizeof(p.Fu)); memcpy(p.bu, f.bu, sizeof(p.bu));
    memcpy(p.track, f.track, sizeof(double) * 6 * f.track_rows); p.track_rows = f.track_rows; p.TL = f.trackLength;
    p.tol_gap = f.tol_gap; p.tol_res = f.tol_res; p.reg = f.reg_lambda; p.max_iter = f.max_iter; p.slacks = f.slacks ? 1 : 0;
    if (!f.slacks) {
        // MPCParams.slacks = False (PredictiveControllers.py:184-198): hard lane rows.  The solve kernels keep their slack variables with a quadratic
        // weight of 1e12 and no linear term: a lane row can then be exceeded by mu / 2e12 ~ 1e-11 m, a thousand times below the solver's own tolerance,
        // and the stage Hessians stay bounded -- a hard row's barrier weight mu^2 / gap enters them directly and costs the Riccati recursion
        // the dual residual below gap ~ 1e-9 (NumPy model: |x - x*| stalls at 1e-7 .. 1e-5 on the fixture; with the penalty 2e-9 in <= 10 iterations).
        p.a_s = 2.0e12; p.c_s = 0.0;
    }
    p.lap_stride = f.max_lap_len; p.mstore = c->mstore; p.sstore = c->sstore;
    p.mquant = c->mquant; p.mqpar = c->mqpar; p.mq_chunks = c->mq_chunks;
}


// ---- controller tuning rows (lmpc_tuning_set): Q[36] R[4] Qf[36] dR[2] Qslack[2] QtermSlack[6] xRef[6] bx[2] bu[4], the values of lmpc_config
enum { TN_Q = 0, TN_R = 36, TN_QF = 40, TN_DR = 76, TN_QS = 78, TN_T = 80, TN_XREF = 86, TN_BX = 92, TN_BU = 94 };
static_assert(TN_BU + 4 == LMPC_TUNING_NPAR, "layout of a tuning row");
int lmpc_tuning_from_config(const lmpc_config *f, double *row) {
    if (!f || !row) return set_err(LMPC_E_ARG, "lmpc_tuning_from_config", "NULL argument");
    memcpy(row + TN_Q, f->Q, sizeof(f->Q)); memcpy(row + TN_R, f->R, sizeof(f->R)); memcpy(row + TN_QF, f->Qf, sizeof(f->Qf));
    memcpy(row + TN_DR, f->dR, sizeof(f->dR)); memcpy(row + TN_QS, f->Qslack, sizeof(f->Qslack));
    for (int i = 0; i < 6; i++) row[TN_T + i] = f->QtermSlack[i * 7];
    memcpy(row + TN_XREF, f->xRef, sizeof(f->xRef)); memcpy(row + TN_BX, f->bx, sizeof(f->bx)); memcpy(row + TN_BU, f->bu, sizeof(f->bu));
    return LMPC_OK;
}


// ---- track rows (lmpc_track_set): [0] rows, [1] trackLength, [2..97] PointAndTangent 16 x 6 row-major, unused rows zero
static_assert(2 + LMPC_MAX_TRACK_ROWS * 6 == LMPC_TRACK_NPAR, "layout of a track row");
int lmpc_track_row_from_config(const lmpc_config *f, double *row) {
    if (!f || !row) return set_err(LMPC_E_ARG, "lmpc_track_row_from_config", "NULL argument");
    if (f->track_rows < 0 || f->track_rows > LMPC_MAX_TRACK_ROWS) return set_err(LMPC_E_ARG, "lmpc_track_row_from_config", "track_rows out of range");
    memset(row, 0, sizeof(double) * LMPC_TRACK_NPAR);
    row[0] = (double)f->track_rows; row[1] = f->trackLength;
    memcpy(row + 2, f->track, sizeof(double) * 6 * (size_t)f->track_rows);
    return LMPC_OK;
}

}  // extern "C" (helpers)

// The track of element b of a batched call with rows in force: the device image and its stride (0: one row serves all).  No rows: dev stays null -- the kernels
// that read the parameter block run.  B against the rows is checked by track_for before anything is queued.
struct trk_src { const double *dev; int stride; };
// The one count check of the row sets: a call of B `noun` ("problems" / "elements" / "cars") against the rows in force, refused under `what` (the set's name in messages).
template <class T> static int rows_fit(const lmpc_row_set<T> &s, long long B, lmpc_row_rule rule, const char *noun, const char *what) {
    if (s.fits(B, rule)) return LMPC_OK;
    char msg[128]; snprintf(msg, sizeof(msg), "B = %lld %s but %s holds %d %srows", B, noun, s.setter, s.n, rule == LMPC_ROWS_AT_LEAST ? "per-car " : "");
    return set_err(LMPC_E_ARG, what, msg);
}
// the body of the five getters: the rows in force of set `m` of the context
template <class T> static int rows_get(lmpc_ctx *c, lmpc_row_set<T> lmpc_ctx::*m, int *n, T *out, int capacity) {
    ARGCHK(c && n && capacity >= 0);
    (c->*m).get(n, out, capacity);
    return LMPC_OK;
}
static int track_for(lmpc_ctx *c, long long B, trk_src *t) {
    t->dev = nullptr; t->stride = 0;
    if (!c->trk.in_force()) return LMPC_OK;
    RCCHK(rows_fit(c->trk, B, LMPC_ROWS_EXACT, "elements", "track rows"));
    t->dev = (const double *)c->img[IMG_TRK].p; t->stride = c->trk.stride(LMPC_TRACK_NPAR);
    return LMPC_OK;
}
// TrackLength of track row `row` (computeCost, addPoint): the config's without rows, the one row's with one
static double track_length_of(const lmpc_ctx *c, int row) {
    return c->trk.in_force() ? c->trk.row(row)[1] : c->cfg.trackLength;
}
// the host-side lap writers have no car: the config's TrackLength, or row 0 of one; with one row per car the caller must say which (the _on forms)
static int track_length_host(lmpc_ctx *c, const char *who, const char *on_form, double *TL) {
    if (c->trk.n > 1) { char msg[160]; snprintf(msg, sizeof(msg), "lmpc_track_set holds %d rows and this call names no car: use %s", c->trk.n, on_form); return set_err(LMPC_E_STATE, who, msg); }
    *TL = track_length_of(c, 0);
    return LMPC_OK;
}
static int track_length_on(lmpc_ctx *c, const char *who, int row, double *TL) {
    if (row < 0 || row >= std::max(c->trk.n, 1)) { char msg[128]; snprintf(msg, sizeof(msg), "track_row %d, %d rows in force", row, c->trk.n); return set_err(LMPC_E_ARG, who, msg); }
    *TL = track_length_of(c, row);
    return LMPC_OK;
}

// one row as the kernels stage it: the PAR_* layout of the parameter block in LDS, the values fill_params derives from a config holding this row
static void tuning_image_row(const lmpc_config &f, const double *row, double *img) {
    memcpy(img + PAR_FX, f.Fx, sizeof(f.Fx)); memcpy(img + PAR_FU, f.Fu, sizeof(f.Fu));
    memcpy(img + PAR_BX, row + TN_BX, 2 * sizeof(double)); memcpy(img + PAR_BU, row + TN_BU, 4 * sizeof(double));
    for (int i = 0; i < 36; i++) { img[PAR_Q2 + i] = 2 * row[TN_Q + i]; img[PAR_QF2 + i] = 2 * row[TN_QF + i]; }
    for (int i = 0; i < 4; i++) img[PAR_R2 + i] = 2 * row[TN_R + i];
    img[PAR_DR2] = 2 * row[TN_DR]; img[PAR_DR2 + 1] = 2 * row[TN_DR + 1];
    for (int i = 0; i < 6; i++) { img[PAR_T2 + i] = 2 * row[TN_T + i]; img[PAR_XREF + i] = row[TN_XREF + i]; }
    img[PAR_AS] = f.slacks ? 2 * row[TN_QS] : 2.0e12; img[PAR_CS] = f.slacks ? row[TN_QS + 1] : 0.0;      // (hard lane rows: the rows' Qslack is ignored, see fill_params)
}
static int tuning_upload(lmpc_ctx *c, int n, const double *rows);

#define LMPC_RETRY_RING 64
#define LMPC_SLAB_COPY_MAX ((size_t)256 * 1024)     // contexts whose output slab has at most this many bytes (batch 1 .. ~16) own host-mapped mirrors of their slabs

template <class T> static T *mut(const T *p) { return const_cast<T *>(p); }      // (a caller's input array inside an lmpc_arrays: only ever the source of a copy)
// temporaries of one call, freed when it returns on any path (not the pooled scratch: lmpc_assemble_batch wants hundreds of KB per problem, not to be kept for the context's life)
struct call_temps {
    std::vector<void *> held;
    ~call_temps() { for (void *q : held) (void)hipFree(q); }
    template <class T> hipError_t alloc(T **q, size_t bytes) { const hipError_t e = hipMalloc((void **)q, bytes); if (e == hipSuccess) held.push_back(*q); return e; }
};
// scratch of the host-buffer entry points (every one of them waits for its own work before it returns): one device allocation, grown on demand and kept (no hipMalloc / hipFree per call)
static int pooled_scratch(lmpc_ctx *c, size_t bytes, void **out) {
    if (bytes > c->scr_bytes) {
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->scr_dev) { (void)g_free(c->scr_dev); c->scr_dev = nullptr; c->scr_bytes = 0; }
        const size_t want = std::max<size_t>((bytes + 4095) & ~(size_t)4095, (size_t)64 * 1024);
        HIPCHK(g_malloc(&c->scr_dev, want)); c->scr_bytes = want;
    }
    *out = c->scr_dev;
    return LMPC_OK;
}
// `bytes` of host data become the device image `img` of a row set.  A larger image goes into a new allocation that replaces the old one only once it is filled: a HIP
// failure on the way leaves the image in force, and its capacity, as they were.  The callers have resolved the launches still pending their retry pass and drained the
// stream (those read the image of THEIR launch); nothing is drained here.  what: the copy, named in the error.
static int image_upload(dev_image *img, const void *host, size_t bytes, const char *what) {
    const bool grow = bytes > img->cap;
    void *buf = img->p;
    if (grow) HIPCHK(g_malloc(&buf, bytes));
    const hipError_t e = hipMemcpy(buf, host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { if (grow) (void)g_free(buf); return set_err(LMPC_E_HIP, what, hipGetErrorString(e)); }
    if (grow) { (void)g_free(img->p); img->p = buf; img->cap = bytes; }
    return LMPC_OK;
}
// Look-ahead regression: the largest batch whose queued steps chain.  PLACEHOLDER_RULE
#define K1_AHEAD_MAX_BATCH_RULE (1 << 30)
// Two-role launches: the cap of the queries per regression work-group (k1_queries_per_block under it).  A CU takes a regression work-group only when its QP has
// converged, so a finer split leaves a shorter tail behind the last solves -- but every work-group loads and scans the laps for itself, and that weighs more:
// measured at batch 256 (profiles/merged_step_ab.json, ms per step) 12: 0.1799, 6: 0.1805, 4: 0.1831, 3: 0.1909, 2: 0.2025, 1: 0.2511 against the parent's 0.1874.
// One work-group per problem, the whole horizon.
#define MERGE_QG_RULE 12
// everything of lmpc_create that can fail; the caller destroys the context on any error (one failure path, no leaks)
static int create_body(lmpc_ctx *c) {
    const lmpc_config *cfg = &c->cfg;
    HIPCHK(hipSetDevice(cfg->device));
    // an unsupported (N, numSS_points) pair is an ordinary user error: find that out before anything is allocated
    c->k1_force16 = dev_knob("LMPC_K1_RPL16") != nullptr;
    { const char *e = dev_knob("LMPC_K1_QG"); c->k1_qg_force = e ? atoi(e) : 0; }
    { const int rc = pick_solver(c); if (rc) return rc; }
    {   // batches that leave SIMDs idle (B <= number of CUs) run the 4-waves-per-QP kernel
        const char *e = dev_knob("LMPC_MW_MAX_BATCH"); hipDeviceProp_t prop; int cus = 256;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
        c->mw_max_batch = e ? atoi(e) : cus; c->n_cu = cus;
    }
    // a variant whose one-wave LDS footprint leaves room for ONE QP per CU only would keep three SIMDs idle at any batch size and runs four waves
    // per QP throughout.  None of the built-in horizons is in that class any more: N = 40 fits two QPs per CU with [A_k | B_k] in LDS (53.5 KB)
    // and four with it in global memory (38.2 KB, lmpc_variant.hip.h: use_abg), so N = 40 follows the ordinary rule below (one wave from batch 257)
    if (!dev_knob("LMPC_MW_MAX_BATCH") && 2 * (c->var.lds_1w_abg ? c->var.lds_1w_abg : c->var.lds_1w) > 160 * 1024) c->mw_max_batch = 1 << 30;
    // Two waves per QP between the four-wave and the one-wave regime: how far up depends on the horizon -- the longer the horizon, the
    // larger the share of the Newton step that is sequential (the helper wave only waits) and the fewer QPs of the multi-wave LDS layout fit a
    // CU.  Measured (solve kernel, ms; two waves | one wave): N=12 B=1024 0.30 | 0.40, B=2048 (two rounds | one round) 0.56 | 0.47;  N=14 B=512 0.33 | 0.42, B=1024 0.48 | 0.44;
    // N=20 B=512 0.43 | 0.56, B=1024 0.79 | 0.63;  N=40 B=512 1.35 | 1.00, B=1024 2.33 | 1.78 (and four waves: 1.18, 2.05).
    c->mw2_max_batch = c->mw_max_batch == c->n_cu ? (cfg->N <= 12 ? 4 : cfg->N <= 24 ? 2 : 0) * c->n_cu : 0;

    // safe sets wider than 58 points (several terminal-block columns per lane): the two-wave kernel is built for one wave per SIMD
    // (two QPs per CU), so its regime ends at two QPs per CU
    if (cfg->numSS_it > 0 && cfg->numSS_points + 6 > WAVE && c->mw2_max_batch > 2 * c->n_cu) c->mw2_max_batch = 2 * c->n_cu;
    // ... and never beyond what is resident at once: a second round of two-wave work-groups loses to the one-wave kernel (N = 12, batch 1024,
    // solve kernel: 0.425 ms in two rounds against 0.349 ms; round 4 found it out the hard way -- 512 bytes more static LDS, three QPs per CU instead of four)
    if (c->var.occ_mw2 > 0 && c->mw2_max_batch > c->var.occ_mw2 * c->n_cu) c->mw2_max_batch = c->var.occ_mw2 * c->n_cu;
    if (const char *e = dev_knob("LMPC_MW2_MAX_BATCH")) c->mw2_max_batch = atoi(e);        // (experiments)
    // a variant without multi-wave kernels -- the runtime kernel, and a fixed (N, S) whose multi-wave layout exceeds the LDS of a CU (lmpc_variant.hip.h: has_mw) --
    // runs one wave per QP at every batch size, whatever the rules and knobs above said (the four-waves-throughout rule included: there is no four-wave kernel)
    if (c->var.lds_mw == 0) { c->mw_max_batch = 0; c->mw2_max_batch = 0; }
    // Fused step (regression inside the one-wave solve kernel): bit-identical results, 42 MB less HBM traffic per step at batch 4096, but
    // MEASURED SLOWER -- 1.37 vs 1.01 + 0.23 ms at batch 4096, 2.48 vs 1.81 + 0.44 ms at batch 8192 with six QPs per CU; 1.92 vs 1.45 + 0.41 ms
    // at batch 8192 with eight: the regression's short dependent chains (DPP minima, 5 x 5 Cholesky, scattered L2 reads) want the four waves
    // per SIMD its own kernel gets, the solve kernel runs two.  Off unless LMPC_FUSE=1.
    { const char *e = dev_knob("LMPC_FUSE"); c->fuse_k1 = e ? atoi(e) : 0; }
    // (the runtime-(N, S) kernel has no fused form: it would take io.mode & 4 for a plain solve and read A / B / C nobody wrote -- the step runs as two kernels there)
    if (c->solver_kind == 2) c->fuse_k1 = 0;
    if (c->fuse_k1 && (size_t)(54 * cfg->N + k1_fused_doubles(cfg->N, cfg->trToUse, cfg->maxNumPoint)) * sizeof(double) > (size_t)160 * 1024) c->fuse_k1 = 0;   // (many laps: the regression's work space does not fit beside the solve)
    {   // condensed kernel (lmpc_solve_cd.hip.h): built for 2N <= 32 and one terminal-block column per lane; it takes the state cost as diagonal Q, Qf
        bool diag = true; c->cd_hasq = 0;
        for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) {
            if (i != j && (cfg->Q[i * 6 + j] != 0.0 || cfg->Qf[i * 6 + j] != 0.0)) diag = false;
            if (cfg->Q[i * 6 + j] != 0.0 || cfg->Qf[i * 6 + j] != 0.0) c->cd_hasq = 1;
            if (i == j && (cfg->Q[i * 6 + j] < 0.0 || cfg->Qf[i * 6 + j] < 0.0)) diag = false;
        }
        c->cd_ok = c->var.lds_cd > 0 && diag;
        const char *e = dev_knob("LMPC_CD"); c->cd_mode = e ? atoi(e) : 0;
    }
    HIPCHK(hipStreamCreate(&c->stream));
    // look-ahead regression: see lmpc_ctx.  (Bit-identical either way: the same kernels on the same inputs.)
    { const char *e = dev_knob("LMPC_K1_AHEAD"); c->k1_ahead = e ? atoi(e) != 0 : 1; }
    if (c->create_flags & LMPC_CREATE_NO_K1_AHEAD) c->k1_ahead = 0;
    c->k1_ahead_max_batch = K1_AHEAD_MAX_BATCH_RULE;
    if (const char *e = dev_knob("LMPC_K1_AHEAD_MAX_BATCH")) c->k1_ahead_max_batch = atoi(e);        // (experiments)
    // merged form of the look-ahead (lmpc_ctx::held): on wherever the look-ahead is; LMPC_K1_MERGE=0 / LMPC_CREATE_NO_K1_MERGE leave the two-stream form.  The cap of the
    // queries per regression work-group of a two-role launch: MERGE_QG_RULE, LMPC_K1_MERGE_QG for the sweep.  (Bit-identical either way.)
    { const char *e = dev_knob("LMPC_K1_MERGE"); c->k1_merge = c->k1_ahead && (e ? atoi(e) != 0 : 1) && !(c->create_flags & LMPC_CREATE_NO_K1_MERGE); }
    { const char *e = dev_knob("LMPC_K1_MERGE_QG"); c->k1_merge_qg = e && atoi(e) > 0 ? atoi(e) : MERGE_QG_RULE; }
    if (c->var.lds_1w_abg > 0 && !dev_knob("LMPC_NO_ABG")) { HIPCHK(g_malloc(&c->ab_pack, sizeof(double) * 48 * (size_t)cfg->N * (size_t)cfg->max_batch)); c->ab_pack_cap = (size_t)cfg->max_batch; }
    HIPCHK(hipHostMalloc(&c->h_retry, sizeof(int) * LMPC_RETRY_RING, hipHostMallocMapped));
    memset(c->h_retry, 0, sizeof(int) * LMPC_RETRY_RING);
    HIPCHK(hipHostGetDevicePointer((void **)&c->d_retry, c->h_retry, 0));
    const size_t store_elems = (size_t)cfg->max_laps * LMPC_COLS * cfg->max_lap_len;
    HIPCHK(g_malloc(&c->mstore, store_elems * sizeof(double)));
    HIPCHK(g_malloc(&c->sstore, store_elems * sizeof(double)));
    HIPCHK(hipMemset(c->mstore, 0, store_elems * sizeof(double)));
    c->mq_chunks = (cfg->max_lap_len + K1_CHUNK - 1) / K1_CHUNK;
    HIPCHK(g_malloc(&c->mquant, (size_t)cfg->max_laps * 3 * cfg->max_lap_len * sizeof(unsigned)));
    HIPCHK(g_malloc(&c->mqpar, (size_t)cfg->max_laps * c->mq_chunks * 6 * sizeof(double)));
    HIPCHK(hipMemset(c->mquant, 0, (size_t)cfg->max_laps * 3 * cfg->max_lap_len * sizeof(unsigned)));
    HIPCHK(hipMemset(c->mqpar, 0, (size_t)cfg->max_laps * c->mq_chunks * 6 * sizeof(double)));
    HIPCHK(hipMemset(c->sstore, 0, store_elems * sizeof(double)));
    c->dims = {(size_t)cfg->N, (size_t)(cfg->numSS_it > 0 ? cfg->numSS_points : 0), (size_t)cfg->numSS_it};
    const size_t gap = LMPC_SLAB_GAP;
    // two passes over the same layout: sizes first, then pointers into the slabs and their mirrors (every range 256-byte aligned)
    size_t total[2];
    lmpc_slab_layout(c->dims, (size_t)cfg->max_batch, gap, total, [](const char *, auto, int, size_t, size_t) {});
    HIPCHK(g_malloc(&c->slab_in, total[0])); HIPCHK(g_malloc(&c->slab_out, total[1]));
    HIPCHK(hipMemset(c->slab_in, 0, total[0])); HIPCHK(hipMemset(c->slab_out, 0, total[1]));
    char *mapped[2] = {nullptr, nullptr};    // device addresses of the mirrors
    if (total[1] <= LMPC_SLAB_COPY_MAX) {
        HIPCHK(hipHostMalloc(&c->h_in, total[0], hipHostMallocMapped)); HIPCHK(hipHostMalloc(&c->h_out, total[1], hipHostMallocMapped)); memset(c->h_in, 0, total[0]); memset(c->h_out, 0, total[1]);
        HIPCHK(hipHostGetDevicePointer((void **)&mapped[0], c->h_in, 0)); HIPCHK(hipHostGetDevicePointer((void **)&mapped[1], c->h_out, 0));
    }
    char *const dev[2] = {c->slab_in, c->slab_out}, *const host[2] = {c->h_in, c->h_out};
    lmpc_slab_layout(c->dims, (size_t)cfg->max_batch, gap, total, [&](const char *, auto m, int slab, size_t off, size_t bytes) {
        typedef std::remove_reference_t<decltype(c->w.*m)> ptr_t;
        c->w.*m = (ptr_t)(dev[slab] + off);
        if (host[slab]) { c->hm.*m = (ptr_t)(host[slab] + off); c->dm.*m = (ptr_t)(mapped[slab] + off); }
        if (gap) c->gaps.push_back(dev[slab] + off + bytes);
    });
    for (char *g_ : c->gaps) HIPCHK(hipMemset(g_, 0xA5, LMPC_GUARD_BYTES));
    c->ho[0] = {c->w.A, c->w.Bm, c->w.C, c->w.rstatus};
    return LMPC_OK;
}

extern "C" {
int lmpc_destroy(lmpc_ctx *c);
int lmpc_create_ex(const lmpc_config *cfg, unsigned flags, lmpc_ctx **out);
int lmpc_create(const lmpc_config *cfg, lmpc_ctx **out) { return lmpc_create_ex(cfg, 0u, out); }
int lmpc_solver_kind(lmpc_ctx *c) { return c ? c->solver_kind : LMPC_E_ARG; }
int lmpc_create_ex(const lmpc_config *cfg, unsigned flags, lmpc_ctx **out) {
    ARGCHK(cfg && out);
    ARGCHK(cfg->N >= 2 && cfg->N <= LMPC_MAX_N);
    ARGCHK(cfg->numSS_it >= 0 && cfg->numSS_it <= LMPC_MAX_USED_LAPS && cfg->trToUse >= 0 && cfg->trToUse <= LMPC_MAX_USED_LAPS);
    ARGCHK(cfg->maxNumPoint >= 1 && cfg->maxNumPoint <= 8);
    if (cfg->numSS_it > 0) {
        ARGCHK(cfg->numSS_points % cfg->numSS_it == 0 && cfg->numSS_points <= LMPC_MAX_SS_POINTS && cfg->numSS_points / cfg->numSS_it + 1 <= WAVE);
        for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) if (i != j) ARGCHK(cfg->QtermSlack[i * 6 + j] == 0.0);   // diagonal terminal-slack weight
        for (int i = 0; i < 6; i++) ARGCHK(cfg->QtermSlack[i * 7] > 0.0);
    }
    ARGCHK(cfg->track_rows >= 0 && cfg->track_rows <= LMPC_MAX_TRACK_ROWS);
    ARGCHK(cfg->slacks || cfg->numSS_it == 0);          // hard lane rows: plain MPC only (the reference's LMPC.unpackSolution mis-slices without slack variables)
    ARGCHK(cfg->max_batch >= 1 && cfg->max_laps >= 1 && cfg->max_lap_len >= 8);
    lmpc_ctx *c = new lmpc_ctx();                      // value-initialised: every pointer starts as nullptr, so lmpc_destroy is safe at any point
    c->cfg = *cfg; c->init_max_laps = cfg->max_laps; c->lt.width = cfg->trToUse; c->sst.width = cfg->numSS_it; c->create_flags = flags; c->profiling = 0; c->ro = nullptr; c->var_dl = nullptr; c->comm = nullptr; c->comm_rank = 0; c->comm_world = 1;
    memset(&c->stats, 0, sizeof(c->stats));
    int rc = create_body(c);
    if (rc != LMPC_OK) { const std::string keep = g_err; lmpc_destroy(c); g_err = keep; return rc; }
    fill_params(c);
    rc = tuning_upload(c, 0, nullptr);                 // (the config's own row: what a launch with a safe-set table and no tuning rows stages from)
    if (rc != LMPC_OK) { const std::string keep = g_err; lmpc_destroy(c); g_err = keep; return rc; }
    *out = c;
    return LMPC_OK;
}

static void rollout_free(lmpc_ctx *c);
static void check_slab_gaps(lmpc_ctx *c) {
#ifdef LMPC_GUARD
    (void)hipDeviceSynchronize();
    for (char *g_ : c->gaps) check_guard_zone(g_, "work-buffer range of a slab");
#else
    (void)c;
#endif
}
int lmpc_debug_guard_failures(void) { return g_guard_failures; }      /* guard builds (-DLMPC_GUARD): overruns found so far; 0 in ordinary builds */
int lmpc_destroy(lmpc_ctx *c) {
    if (!c) return LMPC_OK;
    (void)hipSetDevice(c->cfg.device);
    c->has_held = false;                               // a held solve is dropped, not launched: the caller may have freed its arrays, and nobody has asked for the results
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->k1_stream) (void)hipStreamSynchronize(c->k1_stream);
    rollout_free(c);
    if (c->comm) { (void)ncclCommDestroy((ncclComm_t)c->comm); c->comm = nullptr; }
    if (c->scr_dev) (void)g_free(c->scr_dev);
    if (c->comm_scr) (void)g_free(c->comm_scr);
    if (c->comm_scr_h) (void)hipHostFree(c->comm_scr_h);
    for (auto &e : c->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    void *ptrs[] = {c->mstore, c->sstore, c->mquant, c->mqpar, c->slab_in, c->slab_out, c->ab_pack, c->ho[1].A, c->ho[1].Bm, c->ho[1].C, c->ho[1].rstatus};      // (the work buffers are ranges of the two slabs)
    check_slab_gaps(c);
    for (void *q : ptrs) if (q) (void)g_free(q);
    for (dev_image &im : c->img) (void)g_free(im.p);
    if (c->h_retry) (void)hipHostFree(c->h_retry);
    if (c->h_in) (void)hipHostFree(c->h_in);
    if (c->h_out) (void)hipHostFree(c->h_out);
    if (c->e_k1) (void)hipEventDestroy(c->e_k1);
    if (c->e_front) (void)hipEventDestroy(c->e_front);
    if (c->k1_stream) (void)hipStreamDestroy(c->k1_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->var_dl) dlclose(c->var_dl);
    delete c;
    return LMPC_OK;
}

static int resolve_retries(lmpc_ctx *c);
// Every entry point that changes what a deferred retry pass would read -- the lap stores, caller-visible device buffers (lmpc_dev_upload), the
// context's A / B / C hand-over buffers (lmpc_regress_batch, lmpc_regress_points, lmpc_qp_solve_batch, lmpc_assemble_batch; a
// lmpc_step_batch_dev launch with A / Bm / C NULL hands over through them and is the only kind of launch left pending) -- or hands results to
// someone else (lmpc_comm_allgather_dev, lmpc_ss_get_qfun) first gives the launches still pending their retry pass: a flagged problem is then
// re-solved against the data of ITS launch, never against a changed safe set or overwritten inputs.  (No launch pending -- the drop-in flow,
// where lmpc_step_batch resolves before it returns -- costs nothing: no stream drain is added.)  The retry pass reads nothing else of the
// context's: not the per-point regression status (it keeps the first pass's bits), not the [A_k | B_k] scratch (it stages them in LDS).
#define RESOLVE_PENDING() RCCHK(resolve_retries(c))

// ---------------------------------------------------------------------------------------------- stores
// The reference keeps its laps in Python lists that grow without bound (PredictiveControllers.py:418-445, PredictiveModel.py:35-46; addPoint
// appends a row per closed-loop step, :466-474).  max_laps / max_lap_len of lmpc_config are therefore INITIAL capacities: when a lap or a row
// does not fit, both stores (and the K1 prefilter image) move to allocations of at least twice the size -- strided device-to-device copies,
// [lap][column][row] with the new row stride -- and the device parameter block is rebuilt.  Amortised O(1) per stored row; no kernel is in
// flight while it happens (the stream is drained first).

// Per-problem lap table (lmpc_model_set_lap_table).  The context keeps insertion indices; what the regression kernel reads are (slot, rows) pairs.  One row of `idx`
// (trToUse insertion indices, any order, duplicates allowed) in the order a context holding only those laps would use them: ascending length, ties by insertion
// index (PredictiveModel.addTrajectory, PredictiveModel.py:35-46: a sorted insert that appends among equals).  *small: no lap of the row exceeds the 8-rows-per-lane scan.
static void resolve_lap_row(const lmpc_ctx *c, const int *idx, int *pairs, bool *small) {
    const int L = c->cfg.trToUse;
    std::vector<int> o(idx, idx + L);
    std::sort(o.begin(), o.end(), [&](int a, int b) { return c->m_len[a] != c->m_len[b] ? c->m_len[a] < c->m_len[b] : a < b; });
    for (int i = 0; i < L; i++) { pairs[2 * i] = o[i]; pairs[2 * i + 1] = c->m_len[o[i]]; if (c->m_len[o[i]] - 1 > 8 * WAVE) *small = false; }   // (insertion index == slot)
}
// the whole table, resolved: rows x trToUse x 2 ints
static std::vector<int> resolve_lap_rows(const lmpc_ctx *c, bool *small) {
    const size_t L = (size_t)c->cfg.trToUse;
    std::vector<int> pairs((size_t)c->lt.n * L * 2);
    *small = true;
    for (int r = 0; r < c->lt.n; r++) resolve_lap_row(c, &c->lt.rows[(size_t)r * L], &pairs[(size_t)r * L * 2], small);
    return pairs;
}
// (re)build the device image from the indices the context keeps: after `set`, after the stores moved, after a lap was replaced.  No kernel is in flight (callers drain the stream).
static int resolve_lap_table(lmpc_ctx *c) {
    if (!c->lt.in_force()) return LMPC_OK;
    const std::vector<int> pairs = resolve_lap_rows(c, &c->lt_small);
    return image_upload(&c->img[IMG_LT], pairs.data(), pairs.size() * sizeof(int), "hipMemcpy (lap-table image)");
}

static int grow_stores(lmpc_ctx *c, int need_laps, int need_len) {
    const int old_laps = c->cfg.max_laps, old_len = c->cfg.max_lap_len;
    int new_laps = old_laps, new_len = old_len;
    while (new_laps < need_laps) new_laps *= 2;
    while (new_len < need_len) new_len *= 2;
    if (new_laps == old_laps && new_len == old_len) return LMPC_OK;
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    const int old_chunks = c->mq_chunks, new_chunks = (new_len + K1_CHUNK - 1) / K1_CHUNK;
    const size_t elems = (size_t)new_laps * LMPC_COLS * new_len;
    double *nm = nullptr, *ns = nullptr, *np_ = nullptr; unsigned *nq = nullptr;
    auto fail = [&](int rc) { if (nm) (void)g_free(nm); if (ns) (void)g_free(ns); if (nq) (void)g_free(nq); if (np_) (void)g_free(np_); return rc; };
#define GROWCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(set_err(LMPC_E_HIP, #call, hipGetErrorString(e_))); } while (0)
    GROWCHK(g_malloc(&nm, elems * sizeof(double))); GROWCHK(g_malloc(&ns, elems * sizeof(double)));
    GROWCHK(g_malloc(&nq, (size_t)new_laps * 3 * new_len * sizeof(unsigned))); GROWCHK(g_malloc(&np_, (size_t)new_laps * new_chunks * 6 * sizeof(double)));
    GROWCHK(hipMemset(nm, 0, elems * sizeof(double))); GROWCHK(hipMemset(ns, 0, elems * sizeof(double)));
    GROWCHK(hipMemset(nq, 0, (size_t)new_laps * 3 * new_len * sizeof(unsigned))); GROWCHK(hipMemset(np_, 0, (size_t)new_laps * new_chunks * 6 * sizeof(double)));
    const size_t nml = c->m_len.size(), nsl = c->s_len.size();
    if (nml) {
        GROWCHK(hipMemcpy2D(nm, (size_t)new_len * 8, c->mstore, (size_t)old_len * 8, (size_t)old_len * 8, nml * LMPC_COLS, hipMemcpyDeviceToDevice));
        GROWCHK(hipMemcpy2D(nq, (size_t)new_len * 4, c->mquant, (size_t)old_len * 4, (size_t)old_len * 4, nml * 3, hipMemcpyDeviceToDevice));
        GROWCHK(hipMemcpy2D(np_, (size_t)new_chunks * 48, c->mqpar, (size_t)old_chunks * 48, (size_t)old_chunks * 48, nml, hipMemcpyDeviceToDevice));
    }
    if (nsl) GROWCHK(hipMemcpy2D(ns, (size_t)new_len * 8, c->sstore, (size_t)old_len * 8, (size_t)old_len * 8, nsl * LMPC_COLS, hipMemcpyDeviceToDevice));
#undef GROWCHK
    (void)g_free(c->mstore); (void)g_free(c->sstore); (void)g_free(c->mquant); (void)g_free(c->mqpar);
    c->mstore = nm; c->sstore = ns; c->mquant = nq; c->mqpar = np_; c->mq_chunks = new_chunks;
    c->cfg.max_laps = new_laps; c->cfg.max_lap_len = new_len;
    const lmpc_dev_params keep = c->dp;
    fill_params(c);
    // (per-launch parts of the parameter block survive: selected slots / lengths are refreshed by every launch anyway)
    memcpy(c->dp.mslot, keep.mslot, sizeof(keep.mslot)); memcpy(c->dp.mlen, keep.mlen, sizeof(keep.mlen));
    memcpy(c->dp.sslot, keep.sslot, sizeof(keep.sslot)); memcpy(c->dp.sslen, keep.sslen, sizeof(keep.sslen)); memcpy(c->dp.sslapid, keep.sslapid, sizeof(keep.sslapid));
    c->dp.cur_it = keep.cur_it;
    return resolve_lap_table(c);
}

// ---- the one writer of the stores (lmpc_commit.hip.h).  Its kernels read rows as log[(t * B + car) * width], the layout of a session's logs; a lap the host hands in
// (x: T x 6, u: T x 2, row-major) is that layout with B = 1, car = 0, so it is staged at the head of the pooled scratch and written by the same launch.
struct store_rows { const double *logX, *logU; int B; void *tail; };   // tail: pooled scratch behind the staged rows, for the launch's table and results
static int staged_rows(lmpc_ctx *c, const double *x, const double *u, int T, size_t tail_bytes, store_rows *s) {
    void *scr; RCCHK(pooled_scratch(c, sizeof(double) * 8 * (size_t)T + tail_bytes, &scr));
    double *dx = (double *)scr, *du = dx + 6 * (size_t)T;
    HIPCHK(hipMemcpyAsync(dx, x, sizeof(double) * 6 * (size_t)T, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(du, u, sizeof(double) * 2 * (size_t)T, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                          // (x and u are the caller's pageable memory: read before anything below can fail and return)
    *s = {dx, du, 1, du + 2 * (size_t)T};
    return LMPC_OK;
}
// both streams of the session drained (the logs are complete up to step t and no launch reads the stores), then its logs as the source
static int session_rows(lmpc_ctx *c, size_t tail_bytes, store_rows *s) {
    RCCHK(ctx_enter(c)); RESOLVE_PENDING();
    if (c->ro->pstream) HIPCHK(hipStreamSynchronize(c->ro->pstream));
    HIPCHK(hipStreamSynchronize(c->stream));
    void *scr; RCCHK(pooled_scratch(c, tail_bytes, &scr));
    *s = {c->ro->d_logX, c->ro->d_logU, c->ro->B, scr};
    return LMPC_OK;
}
static lmpc_commit_args commit_args(const lmpc_ctx *c, const store_rows &s) {
    lmpc_commit_args a; a.logX = s.logX; a.logU = s.logU; a.B = s.B; a.sstore = c->sstore; a.mstore = c->mstore; a.mquant = c->mquant; a.mqpar = c->mqpar;
    a.ls = c->cfg.max_lap_len; a.mq_chunks = c->mq_chunks; memcpy(a.scaling, c->cfg.scaling, sizeof(a.scaling));
    return a;
}
#define LMPC_COMMIT_TAIL(n) ((sizeof(double) + sizeof(lmpc_commit_entry)) * (size_t)(n))
#define LMPC_EXTEND_TAIL(n) ((sizeof(double) + sizeof(lmpc_extend_entry) + sizeof(int)) * (size_t)(n))

// Whole laps: entry i of `tab` is rows [0, rows) of car `car` of the source, written to the slots it names.  One growth of the stores, one table upload, one launch, one
// download of q0 (the Qfun of every entry's first row), then the stream is drained: on return the source has been read.  The context's vectors are not touched.
static int commit_laps(lmpc_ctx *c, const store_rows &s, const std::vector<lmpc_commit_entry> &tab, std::vector<double> &q0) {
    const size_t n = tab.size();
    int laps = 0, rows = 0;
    for (const lmpc_commit_entry &t : tab) { laps = std::max(laps, std::max(t.ss_slot, t.m_slot) + 1); rows = std::max(rows, t.rows); }
    RCCHK(grow_stores(c, laps, rows));
    double *d_q0 = (double *)s.tail; lmpc_commit_entry *d_tab = (lmpc_commit_entry *)(d_q0 + n);
    q0.assign(n, 0.0);
    hipError_t e = hipMemcpyAsync(d_tab, tab.data(), sizeof(lmpc_commit_entry) * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { hipLaunchKernelGGL(lmpc_commit_laps_kernel, dim3((unsigned)n), dim3(LMPC_COMMIT_NT), 0, c->stream, commit_args(c, s), (const lmpc_commit_entry *)d_tab, d_q0); e = hipGetLastError(); }
    if (e == hipSuccess && tab[0].ss_slot >= 0) e = hipMemcpyAsync(q0.data(), d_q0, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream);      // (every entry of a call names the same stores)
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(LMPC_E_HIP, "lmpc_commit_laps_kernel", hipGetErrorString(e));
    return LMPC_OK;
}
// The context's vectors after commit_laps has written NEW laps (consecutive slots behind the stored ones): LMPC.addTrajectory's lists (PredictiveControllers.py:418-445;
// the last row's cost is 0, :447-464) and PredictiveModel.addTrajectory's sorted insert (PredictiveModel.py:35-46: append if empty or T >= the longest, else in front
// of the first longer lap -- a new lap goes behind the stored ones of its length).
static void commit_book(lmpc_ctx *c, const std::vector<lmpc_commit_entry> &tab, const std::vector<double> &q0) {
    for (size_t i = 0; i < tab.size(); i++) {
        const int T = tab[i].rows;
        if (tab[i].ss_slot >= 0) { c->s_len.push_back(T); c->s_laptime.push_back(T); c->s_qlast.push_back(0.0); c->s_q0.push_back(q0[i]); c->sst_dirty = true; }   // (last = NULL: which lap is the latest has changed)
        if (tab[i].m_slot >= 0) {
            c->m_len.push_back(T);                                   // (regression store: insertion index == slot)
            if (c->m_order.empty() || T >= c->m_len[c->m_order.back()]) c->m_order.push_back(tab[i].m_slot);
            else { size_t k = 0; while (k < c->m_order.size() && !(T < c->m_len[c->m_order[k]])) k++; c->m_order.insert(c->m_order.begin() + k, tab[i].m_slot); }
        }
    }
}
// one lap handed in by the host: staged, written to the slots named (-1: that store is not written) and, a new lap, entered in the books.  Blocking: x and u are pageable memory
static int commit_host_lap(lmpc_ctx *c, const double *x, const double *u, int T, int ss_slot, int m_slot, bool new_lap, double TL) {
    store_rows s; RCCHK(staged_rows(c, x, u, T, LMPC_COMMIT_TAIL(1), &s));
    const std::vector<lmpc_commit_entry> tab{{0, T, ss_slot, m_slot, TL}}; std::vector<double> q0;
    RCCHK(commit_laps(c, s, tab, q0));
    if (new_lap) commit_book(c, tab, q0);
    return LMPC_OK;
}

// Appended rows, the batched LMPC.addPoint (PredictiveControllers.py:466-474): rows [0, n_rows) of car cars[i] of the source behind the rows of safe-set lap laps[i].  One
// growth, one upload of the table and of every lap's last Qfun value, one launch, one download of the flags, a drained stream, then the books of every lap
// extended.  extended == NULL: the rows are appended whatever they hold; else an entry with a non-finite value is left as it is and reported as 0.
// track_row < 0: entry i adds the TrackLength of car cars[i]'s track (a session); else that of the row named (a host lap)
// src != NULL: the index entry i hands the kernel in place of cars[i] (session_source_index: a lap that does not begin at session row 0)
static int extend_laps(lmpc_ctx *c, const store_rows &s, int n, const int *cars, const int *laps, int n_rows, int *extended, int track_row = -1, const int *src = nullptr) {
    int longest = 0;
    for (int i = 0; i < n; i++) longest = std::max(longest, c->s_len[laps[i]] + n_rows);
    RCCHK(grow_stores(c, c->cfg.max_laps, longest));
    std::vector<lmpc_extend_entry> tab((size_t)n); std::vector<double> ql((size_t)n);
    for (int i = 0; i < n; i++) { tab[(size_t)i] = {src ? src[i] : cars[i], laps[i], c->s_len[laps[i]], 0, track_length_of(c, track_row < 0 ? cars[i] : track_row)}; ql[(size_t)i] = c->s_qlast[laps[i]]; }
    double *d_ql = (double *)s.tail; lmpc_extend_entry *d_tab = (lmpc_extend_entry *)(d_ql + n); int *d_flag = extended ? (int *)(d_tab + n) : nullptr;
    hipError_t e = hipMemcpyAsync(d_ql, ql.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab, tab.data(), sizeof(lmpc_extend_entry) * (size_t)n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { hipLaunchKernelGGL(lmpc_extend_laps_kernel, dim3(n), dim3(LMPC_COMMIT_NT), 0, c->stream, commit_args(c, s), n_rows, (const lmpc_extend_entry *)d_tab, (const double *)d_ql, d_flag); e = hipGetLastError(); }
    if (e == hipSuccess && extended) e = hipMemcpyAsync(extended, d_flag, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(LMPC_E_HIP, "lmpc_extend_laps_kernel", hipGetErrorString(e));
    for (int i = 0; i < n; i++) {
        if (extended && !extended[i]) continue;
        double q = c->s_qlast[laps[i]];
        for (int k = 0; k < n_rows; k++) q -= 1.0;                     // :474, one subtraction per appended row, each rounded: what the kernel left in the last row
        c->s_len[laps[i]] += n_rows; c->s_qlast[laps[i]] = q; c->sst_dirty = true;
    }
    return LMPC_OK;
}

int lmpc_model_add_trajectory(lmpc_ctx *c, const double *x, const double *u, int T) {
    ARGCHK(c && x && u && T >= 2);
    RCCHK(ctx_enter(c));
    RESOLVE_PENDING();
    HIPCHK(hipStreamSynchronize(c->stream));
    return commit_host_lap(c, x, u, T, -1, (int)c->m_len.size(), true, 0.0);                  // PredictiveModel.addTrajectory (PredictiveModel.py:35-46); the regression store holds no cost: no TrackLength is read
}
int lmpc_model_num_laps(lmpc_ctx *c, int *n) { ARGCHK(c && n); *n = (int)c->m_order.size(); return LMPC_OK; }
int lmpc_model_replace_lap(lmpc_ctx *c, int pos, const double *x, const double *u, int T) {
    ARGCHK(c && x && u && pos >= 0 && pos < (int)c->m_order.size());
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    ARGCHK(T == c->m_len[c->m_order[pos]]);
    RCCHK(commit_host_lap(c, x, u, T, -1, c->m_order[pos], false, 0.0));
    return resolve_lap_table(c);
}

int lmpc_model_set_lap_table(lmpc_ctx *c, int n, const int *laps) {
    // checked in full before anything is changed: a refused table leaves the one in force
    ARGCHK(c && n >= 0 && (n == 0 || laps));
    if (n == 0) { c->lt.clear(); return LMPC_OK; }
    const int L = c->cfg.trToUse, stored = (int)c->m_len.size();
    ARGCHK(L >= 1 && (long long)n <= (long long)c->cfg.max_batch * c->cfg.N);         // (lmpc_regress_points serves up to max_batch x N points)
    for (size_t i = 0; i < (size_t)n * L; i++)
        if (laps[i] < 0 || laps[i] >= stored) {
            char msg[128]; snprintf(msg, sizeof(msg), "row %d names lap %d, %d laps are stored", (int)(i / L), laps[i], stored);
            return set_err(LMPC_E_ARG, "lap table", msg);
        }
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));   // (a regression still in flight reads the image about to be overwritten)
    c->lt.assign(n, laps);
    const int rc = resolve_lap_table(c);
    if (rc) c->lt.clear();
    return rc;
}
int lmpc_model_lap_info(lmpc_ctx *c, int lap, int *rows, int *sorted_pos) {
    // the lap with insertion index `lap`: its rows and its position in the sorted order (what lmpc_store_read_lap and lmpc_model_replace_lap address laps by)
    ARGCHK(c && lap >= 0 && lap < (int)c->m_len.size());
    if (rows) *rows = c->m_len[lap];
    if (sorted_pos) *sorted_pos = (int)(std::find(c->m_order.begin(), c->m_order.end(), lap) - c->m_order.begin());
    return LMPC_OK;
}
int lmpc_model_get_lap_table(lmpc_ctx *c, int *n, int *laps, int capacity) { return rows_get(c, &lmpc_ctx::lt, n, laps, capacity); }

static int ss_add_trajectory_tl(lmpc_ctx *c, const double *x, const double *u, int T, double TL) {
    RCCHK(ctx_enter(c));
    RESOLVE_PENDING();
    HIPCHK(hipStreamSynchronize(c->stream));
    return commit_host_lap(c, x, u, T, (int)c->s_len.size(), -1, true, TL);
}
int lmpc_ss_add_trajectory_on(lmpc_ctx *c, int track_row, const double *x, const double *u, int T) {
    ARGCHK(c && x && u && T >= 1);
    double TL; RCCHK(track_length_on(c, "lmpc_ss_add_trajectory_on", track_row, &TL));
    return ss_add_trajectory_tl(c, x, u, T, TL);
}
int lmpc_ss_add_trajectory(lmpc_ctx *c, const double *x, const double *u, int T) {
    ARGCHK(c && x && u && T >= 1);
    double TL; RCCHK(track_length_host(c, "lmpc_ss_add_trajectory", "lmpc_ss_add_trajectory_on", &TL));
    return ss_add_trajectory_tl(c, x, u, T, TL);                        // LMPC.addTrajectory + computeCost (PredictiveControllers.py:418-464)
}

__global__ void lmpc_store_row_kernel(double *base, int stride, int row, double v0, double v1, double v2, double v3, double v4, double v5, double v6, double v7, double v8) {
    const double v[9] = {v0, v1, v2, v3, v4, v5, v6, v7, v8};
    if (threadIdx.x < LMPC_COLS) base[(size_t)threadIdx.x * stride + row] = v[threadIdx.x];
}

int lmpc_ss_add_point(lmpc_ctx *c, const double *x, const double *u) {
    ARGCHK(c && x && u);
    if (c->s_len.empty()) return set_err(LMPC_E_STATE, "addPoint before any addTrajectory", "");
    double TL; RCCHK(track_length_host(c, "lmpc_ss_add_point", "lmpc_ss_extend_lap_on", &TL));
    RCCHK(ctx_enter(c));
    RESOLVE_PENDING();
    const int lap = (int)c->s_len.size() - 1, row = c->s_len[lap];
    if (row >= c->cfg.max_lap_len) { const int rc = grow_stores(c, c->cfg.max_laps, row + 1); if (rc) return rc; }
    const double q = c->s_qlast[lap] - 1.0;                        // :474
    double *base = c->sstore + (size_t)lap * LMPC_COLS * c->cfg.max_lap_len;
    hipLaunchKernelGGL(lmpc_store_row_kernel, dim3(1), dim3(64), 0, c->stream, base, c->cfg.max_lap_len, row,
                       x[0], x[1], x[2], x[3], x[4] + TL, x[5], u[0], u[1], q);   // :472-473
    HIPCHK(hipGetLastError());
    c->s_len[lap] = row + 1; c->s_qlast[lap] = q; c->sst_dirty = true;
    return LMPC_OK;
}
int lmpc_ss_replace_lap(lmpc_ctx *c, int lap, const double *x, const double *u, const double *qfun, int T) {
    ARGCHK(c && x && u && qfun && lap >= 0 && lap < (int)c->s_len.size() && T >= 1);
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    RCCHK(commit_host_lap(c, x, u, T, lap, -1, false, track_length_of(c, 0)));     // (the cost the kernel writes is replaced below: the caller's Qfun stands)
    // the caller's Q-function over the cost the kernel wrote: column 8 of a lap is contiguous ([lap][column][row]; the stores may have moved above)
    HIPCHK(hipMemcpy(c->sstore + ((size_t)lap * LMPC_COLS + 8) * c->cfg.max_lap_len, qfun, sizeof(double) * (size_t)T, hipMemcpyHostToDevice));
    c->s_len[lap] = T; c->s_qlast[lap] = qfun[T - 1]; c->s_q0[lap] = qfun[0]; c->sst_dirty = true;
    return LMPC_OK;
}
int lmpc_ss_set_selected(lmpc_ctx *c, const int *laps, int n) {
    ARGCHK(c && n >= 0 && n <= LMPC_MAX_USED_LAPS && (n == 0 || laps));
    if (n == 0) c->s_override.clear(); else c->s_override.assign(laps, laps + n);
    return LMPC_OK;
}
int lmpc_ss_set_lap_table(lmpc_ctx *c, int n, const int *laps, const int *last) {
    // checked in full before anything is changed: a refused table leaves the one in force.  Nothing is uploaded here: the image is built by the next launch that reads it
    ARGCHK(c && n >= 0 && (n == 0 || laps));
    if (n == 0) { c->sst.clear(); c->sst_last.clear(); c->sst_has_last = false; return LMPC_OK; }
    const int L = c->cfg.numSS_it, stored = (int)c->s_len.size();
    ARGCHK(L >= 1);
    char msg[128];
    for (size_t i = 0; i < (size_t)n * L; i++)
        if (laps[i] < 0 || laps[i] >= stored) {
            snprintf(msg, sizeof(msg), "row %d names lap %d, %d laps are stored", (int)(i / L), laps[i], stored);
            return set_err(LMPC_E_ARG, "safe-set lap table", msg);
        }
    for (int r = 0; last && r < n; r++)
        if (last[r] < -1 || last[r] >= stored) {
            snprintf(msg, sizeof(msg), "last[%d] = %d, %d laps are stored", r, last[r], stored);
            return set_err(LMPC_E_ARG, "safe-set lap table", msg);
        }
    c->sst.assign(n, laps); c->sst_has_last = last != nullptr;
    if (last) c->sst_last.assign(last, last + n); else c->sst_last.clear();
    c->sst_dirty = true;
    return LMPC_OK;
}
int lmpc_ss_get_lap_table(lmpc_ctx *c, int *n, int *laps, int *last, int capacity) {
    RCCHK(rows_get(c, &lmpc_ctx::sst, n, laps, capacity));
    const size_t rows = (size_t)std::min(capacity, c->sst.n);
    for (size_t r = 0; last && r < rows; r++) last[r] = c->sst_has_last ? c->sst_last[r] : LMPC_SS_LAST_SHARED;
    return LMPC_OK;
}
int lmpc_ss_num_laps(lmpc_ctx *c, int *n) { ARGCHK(c && n); *n = (int)c->s_len.size(); return LMPC_OK; }
int lmpc_ss_get_qfun(lmpc_ctx *c, int lap, double *qfun, int *T) {
    ARGCHK(c && T && lap >= 0 && lap < (int)c->s_len.size());
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    *T = c->s_len[lap];
    if (qfun) HIPCHK(hipMemcpy(qfun, c->sstore + ((size_t)lap * LMPC_COLS + 8) * c->cfg.max_lap_len, sizeof(double) * c->s_len[lap], hipMemcpyDeviceToHost));
    return LMPC_OK;
}

int lmpc_store_read_lap(lmpc_ctx *c, int store, int lap, double *x, double *u, double *qfun, int *T) {
    // checkpoint / resume ("optional: dump lap stores as .npz"; the reference imports pickle for it and never uses it, main.py:36): rows of one stored lap back on
    // the host.  store 0: regression store, `lap` = position in its sorted order (PredictiveModel.xStored[lap]); store 1: safe set, `lap` = index in addTrajectory order, with
    // the rows LMPC.addPoint appended and the Q-function.  T is always set; x (T x 6), u (T x 2), qfun (T) may be NULL.
    ARGCHK(c && T && (store == 0 || store == 1));
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    int slot, rows; const double *base;
    if (store == 0) { ARGCHK(lap >= 0 && lap < (int)c->m_order.size()); slot = c->m_order[lap]; rows = c->m_len[slot]; base = c->mstore; }
    else { ARGCHK(lap >= 0 && lap < (int)c->s_len.size()); slot = lap; rows = c->s_len[lap]; base = c->sstore; }
    *T = rows;
    if (!x && !u && !qfun) return LMPC_OK;
    const size_t ls = c->cfg.max_lap_len;
    std::vector<double> col(rows);
    for (int j = 0; j < LMPC_COLS; j++) {
        if ((j < 6 && !x) || (j >= 6 && j < 8 && !u) || (j == 8 && (!qfun || store == 0))) continue;
        HIPCHK(hipMemcpy(col.data(), base + ((size_t)slot * LMPC_COLS + j) * ls, sizeof(double) * rows, hipMemcpyDeviceToHost));
        for (int r = 0; r < rows; r++) { if (j < 6) x[(size_t)r * 6 + j] = col[r]; else if (j < 8) u[(size_t)r * 2 + (j - 6)] = col[r]; else qfun[r] = col[r]; }
    }
    return LMPC_OK;
}

int lmpc_ss_get_laptime(lmpc_ctx *c, int lap, int *T) { ARGCHK(c && T && lap >= 0 && lap < (int)c->s_laptime.size()); *T = c->s_laptime[lap]; return LMPC_OK; }

static int ss_extend_lap_row(lmpc_ctx *c, int track_row, int lap, const double *x, const double *u, int n);
int lmpc_ss_extend_lap_on(lmpc_ctx *c, int track_row, int lap, const double *x, const double *u, int n) {
    ARGCHK(c && lap >= 0 && lap < (int)c->s_len.size() && n >= 0 && (n == 0 || (x && u)));
    double TL; RCCHK(track_length_on(c, "lmpc_ss_extend_lap_on", track_row, &TL));
    return ss_extend_lap_row(c, track_row, lap, x, u, n);
}
int lmpc_ss_extend_lap(lmpc_ctx *c, int lap, const double *x, const double *u, int n) {
    // batched-mode form of LMPC.addPoint (:466-474) for ANY stored lap: append n points shifted by TrackLength in s,
    // Q-function continuing to count down.  (In the reference the points of lap j extend lap j-1 one by one.)  The rows are appended as given, finite or not.
    ARGCHK(c && lap >= 0 && lap < (int)c->s_len.size() && n >= 0 && (n == 0 || (x && u)));
    double TL; RCCHK(track_length_host(c, "lmpc_ss_extend_lap", "lmpc_ss_extend_lap_on", &TL));
    return ss_extend_lap_row(c, 0, lap, x, u, n);
}
static int ss_extend_lap_row(lmpc_ctx *c, int track_row, int lap, const double *x, const double *u, int n) {
    if (n == 0) return LMPC_OK;
    RCCHK(ctx_enter(c));
    RESOLVE_PENDING();
    store_rows s; RCCHK(staged_rows(c, x, u, n, LMPC_EXTEND_TAIL(1), &s));
    const int car = 0;
    return extend_laps(c, s, 1, &car, &lap, n, nullptr, track_row);
}

int lmpc_ss_truncate_lap(lmpc_ctx *c, int lap, int T) {
    ARGCHK(c && lap >= 0 && lap < (int)c->s_len.size() && T >= c->s_laptime[lap] && T <= c->s_len[lap]);
    if (T == c->s_len[lap]) return LMPC_OK;
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    double q = 0.0;                                                  // Qfun of the new last row (addPoint counts on from it, :474)
    HIPCHK(hipMemcpy(&q, c->sstore + ((size_t)lap * LMPC_COLS + 8) * c->cfg.max_lap_len + (T - 1), sizeof(double), hipMemcpyDeviceToHost));
    c->s_len[lap] = T; c->s_qlast[lap] = q; c->sst_dirty = true;
    return LMPC_OK;
}

int lmpc_debug_model_image(lmpc_ctx *c, int lap, unsigned *q, double *par, int *chunks) {
    // the K1 prefilter image of the regression-store lap with insertion index `lap` (lmpc_commit.hip.h: commit_quantise; the scan it serves: PredictiveModel.py:180-197): the
    // three planes of packed words over rows 0 .. rows-2 (3 x (rows-1)), the six parameters of every chunk in use, and their number.  Any output may be NULL.
    ARGCHK(c && lap >= 0 && lap < (int)c->m_len.size());
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    const int nrows = c->m_len[lap] - 1, used = (nrows + K1_CHUNK - 1) / K1_CHUNK; const size_t ls = (size_t)c->cfg.max_lap_len;
    if (chunks) *chunks = used;
    if (q) HIPCHK(hipMemcpy2D(q, (size_t)nrows * sizeof(unsigned), c->mquant + (size_t)lap * 3 * ls, ls * sizeof(unsigned), (size_t)nrows * sizeof(unsigned), 3, hipMemcpyDeviceToHost));
    if (par && used) HIPCHK(hipMemcpy(par, c->mqpar + (size_t)lap * c->mq_chunks * 6, sizeof(double) * 6 * (size_t)used, hipMemcpyDeviceToHost));
    return LMPC_OK;
}

// ---- laps given back (lmpc_retain.h: the books; lmpc_retain.hip.h: the gather).  The only entry point after which a store holds fewer laps than before.
// a lap that something still names is not dropped: `what` names the table, `per_row` entries make a row (0: the position is the row)
static int retain_refuse_named(const char *what, long long pos, int per_row, int lap) {
    char msg[160];
    if (per_row > 0) snprintf(msg, sizeof(msg), "%s: row %lld names lap %d, which is not kept", what, pos / per_row, lap);
    else snprintf(msg, sizeof(msg), "%s: entry %lld names lap %d, which is not kept", what, pos, lap);
    return set_err(LMPC_E_ARG, "lmpc_store_retain", msg);
}
static int retain_check_list(const char *store, int n, const int *keep, int stored) {
    int why = 0; const int k = lmpc_retain_check(n, keep, stored, &why);
    if (k < 0) return LMPC_OK;
    char msg[160];
    if (why == 0) snprintf(msg, sizeof(msg), "%s: entry %d names lap %d, %d laps are stored", store, k, keep[k], stored);
    else snprintf(msg, sizeof(msg), "%s: entry %d (lap %d) is not above entry %d (lap %d): strictly ascending indices expected", store, k, keep[k], k - 1, keep[k - 1]);
    return set_err(LMPC_E_ARG, "lmpc_store_retain", msg);
}
int lmpc_store_retain(lmpc_ctx *c, int n_ss, const int *keep_ss, int n_model, const int *keep_model, int *map_ss, int *map_model) {
    ARGCHK(c && n_ss >= -1 && n_model >= -1 && (n_ss <= 0 || keep_ss) && (n_model <= 0 || keep_model));
    if (c->ro && c->ro->active) return set_err(LMPC_E_STATE, "lmpc_store_retain", "a rollout session is active: its steps read the laps by the indices they had when it began (lmpc_rollout_end first)");
    // checked in full before anything changes: the lists, then everything that names a lap
    const int ns0 = (int)c->s_len.size(), nm0 = (int)c->m_len.size();
    if (n_ss >= 0) RCCHK(retain_check_list("safe set", n_ss, keep_ss, ns0));
    if (n_model >= 0) RCCHK(retain_check_list("regression store", n_model, keep_model, nm0));
    const std::vector<int> smap = n_ss >= 0 ? lmpc_retain_map(n_ss, keep_ss, ns0) : lmpc_retain_identity(ns0);
    const std::vector<int> mmap = n_model >= 0 ? lmpc_retain_map(n_model, keep_model, nm0) : lmpc_retain_identity(nm0);
    long long at;
    if (c->lt.in_force() && (at = lmpc_retain_first_dropped(c->lt.rows.data(), c->lt.rows.size(), mmap)) >= 0) return retain_refuse_named("lap table (lmpc_model_set_lap_table)", at, c->cfg.trToUse, c->lt.rows[(size_t)at]);
    if (c->sst.in_force() && (at = lmpc_retain_first_dropped(c->sst.rows.data(), c->sst.rows.size(), smap)) >= 0) return retain_refuse_named("safe-set lap table (lmpc_ss_set_lap_table)", at, c->cfg.numSS_it, c->sst.rows[(size_t)at]);
    if (c->sst.in_force() && c->sst_has_last && (at = lmpc_retain_first_dropped(c->sst_last.data(), c->sst_last.size(), smap)) >= 0) return retain_refuse_named("last of the safe-set lap table (lmpc_ss_set_lap_table)", at, 1, c->sst_last[(size_t)at]);
    if ((at = lmpc_retain_first_dropped(c->s_override.data(), c->s_override.size(), smap)) >= 0) return retain_refuse_named("selection override (lmpc_ss_set_selected)", at, 0, c->s_override[(size_t)at]);
    if (map_ss) std::copy(smap.begin(), smap.end(), map_ss);
    if (map_model) std::copy(mmap.begin(), mmap.end(), map_model);
    if (lmpc_retain_keeps_all(smap) && lmpc_retain_keeps_all(mmap)) return LMPC_OK;
    // like every other store edit: a held solve launched, the pending retries resolved against the stores of their launch, both streams drained before the stores move
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    if (c->k1_stream) HIPCHK(hipStreamSynchronize(c->k1_stream));
    const int ks = lmpc_retain_kept(smap), km = lmpc_retain_kept(mmap);
    const int new_laps = lmpc_retain_capacity(c->init_max_laps, std::max(ks, km)), ls = c->cfg.max_lap_len;
    std::vector<lmpc_retain_entry> tab;
    for (int old = 0; old < nm0; old++) if (mmap[(size_t)old] >= 0) tab.push_back({0, old, mmap[(size_t)old], c->m_len[(size_t)old]});
    for (int old = 0; old < ns0; old++) if (smap[(size_t)old] >= 0) tab.push_back({1, old, smap[(size_t)old], c->s_len[(size_t)old]});
    void *d_tab = nullptr;
    if (!tab.empty()) RCCHK(pooled_scratch(c, sizeof(lmpc_retain_entry) * tab.size(), &d_tab));
    const size_t elems = (size_t)new_laps * LMPC_COLS * ls, qwords = (size_t)new_laps * 3 * ls, pdoubles = (size_t)new_laps * c->mq_chunks * 6;
    double *nm = nullptr, *ns = nullptr, *np_ = nullptr; unsigned *nq = nullptr;
    auto fail = [&](int rc) { if (nm) (void)g_free(nm); if (ns) (void)g_free(ns); if (nq) (void)g_free(nq); if (np_) (void)g_free(np_); return rc; };
#define RETAINCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(set_err(LMPC_E_HIP, #call, hipGetErrorString(e_))); } while (0)
    RETAINCHK(g_malloc(&nm, elems * sizeof(double))); RETAINCHK(g_malloc(&ns, elems * sizeof(double)));
    RETAINCHK(g_malloc(&nq, qwords * sizeof(unsigned))); RETAINCHK(g_malloc(&np_, pdoubles * sizeof(double)));
    RETAINCHK(hipMemsetAsync(nm, 0, elems * sizeof(double), c->stream)); RETAINCHK(hipMemsetAsync(ns, 0, elems * sizeof(double), c->stream));
    RETAINCHK(hipMemsetAsync(nq, 0, qwords * sizeof(unsigned), c->stream)); RETAINCHK(hipMemsetAsync(np_, 0, pdoubles * sizeof(double), c->stream));
    if (!tab.empty()) {
        lmpc_retain_args a;
        a.src_store[0] = c->mstore; a.src_store[1] = c->sstore; a.dst_store[0] = nm; a.dst_store[1] = ns;
        a.src_quant = c->mquant; a.dst_quant = nq; a.src_qpar = c->mqpar; a.dst_qpar = np_; a.ls = ls; a.mq_chunks = c->mq_chunks;
        RETAINCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(lmpc_retain_entry) * tab.size(), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(lmpc_retain_laps_kernel, dim3((unsigned)tab.size()), dim3(LMPC_RETAIN_NT), 0, c->stream, a, (const lmpc_retain_entry *)d_tab);
        RETAINCHK(hipGetLastError());
    }
    RETAINCHK(hipStreamSynchronize(c->stream));                          // (the table is a local: read before this call returns on any path)
#undef RETAINCHK
    (void)g_free(c->mstore); (void)g_free(c->sstore); (void)g_free(c->mquant); (void)g_free(c->mqpar);
    c->mstore = nm; c->sstore = ns; c->mquant = nq; c->mqpar = np_;
    c->cfg.max_laps = new_laps;
    // the books and everything that names a lap, renumbered here and nowhere else
    c->m_order = lmpc_retain_order(c->m_order, mmap); c->m_len = lmpc_retain_gather(c->m_len, mmap);
    c->s_len = lmpc_retain_gather(c->s_len, smap); c->s_laptime = lmpc_retain_gather(c->s_laptime, smap);
    c->s_qlast = lmpc_retain_gather(c->s_qlast, smap); c->s_q0 = lmpc_retain_gather(c->s_q0, smap);
    lmpc_retain_remap(c->lt.rows.data(), c->lt.rows.size(), mmap);
    lmpc_retain_remap(c->sst.rows.data(), c->sst.rows.size(), smap);
    lmpc_retain_remap(c->sst_last.data(), c->sst_last.size(), smap);
    lmpc_retain_remap(c->s_override.data(), c->s_override.size(), smap);
    c->sst_dirty = true;
    fill_params(c);                                                      // (the per-launch parts -- selected slots, lengths, cur_it -- are written by every launch that reads them)
    return resolve_lap_table(c);
}

// ---- laps of the active session straight into the stores: no log leaves the device
// Parking sessions: the step each car was parked at (-1: live), for the row checks below; empty for a session without parking
static int session_parked_at(lmpc_rollout_session *r, std::vector<int> &at) {
    at.clear();
    if (!r->parked) return LMPC_OK;
    at.resize((size_t)r->B);
    HIPCHK(hipMemcpy(at.data(), r->d_parkedAt, sizeof(int) * (size_t)r->B, hipMemcpyDeviceToHost));
    return LMPC_OK;
}
// Entry i of a call that lists (car, rows) of the active session -- lmpc_rollout_commit_laps, lmpc_rollout_lap_metrics: *T = rows[i], or doneAt[car] with rows == NULL, checked
// against what the session logged for the car (done: doneAt of every car; pat: session_parked_at; least: the fewest rows the call takes).  Refusals are reported under `who`.
static int session_entry_rows(const lmpc_rollout_session *r, const char *who, int i, int car, const int *rows, const std::vector<int> &done, const std::vector<int> &pat, int least, int *T_out) {
    const int s0 = session_lap_start(r, car);                           // (a session that has relaunched counts a car's rows from its lap start; else 0)
    const int T = rows ? rows[i] : done[(size_t)car] - s0;
    char msg[160];
    // (a parked car is not logged from its parking step on; rows = NULL stops at doneAt, which lies inside)
    if (rows && !pat.empty() && pat[(size_t)car] >= 0 && T > pat[(size_t)car]) { snprintf(msg, sizeof(msg), "entry %d: %d rows of car %d, which was parked at step %d (lmpc_rollout_parked_at)", i, T, car, pat[(size_t)car]); return set_err(LMPC_E_ARG, who, msg); }
    if (!rows && done[(size_t)car] < 0) { snprintf(msg, sizeof(msg), "car %d has not crossed the line (doneAt < 0) and no row count was given", car); return set_err(LMPC_E_STATE, who, msg); }
    // rows the session logged for this car: every step logs every car, except that a stop_at_line PID lap is logged up to the crossing step only
    const int logged = (r->kind == RO_PID && r->stop_at_line && done[(size_t)car] >= 0) ? done[(size_t)car] : r->t - s0;
    if (T < least || T > logged) { snprintf(msg, sizeof(msg), "entry %d: %d rows of car %d, %d are logged (at least %d needed)", i, T, car, logged, least); return set_err(LMPC_E_ARG, who, msg); }
    *T_out = T;
    return LMPC_OK;
}
// The commit kernels address row t of an entry's car as log[(t * B + car) * width].  In a session that has relaunched, the rows of a car count from its lap start s0:
// the entry hands the kernels s0 * B + car in place of the car, so that the entry's row 0 is the lap's first -- no new kernel argument.  Refused where that index does
// not fit the int of the entry tables.  With s0 == 0 the index is the car: the tables built and the launches made are those of a session that never relaunched.
static int session_source_index(const lmpc_rollout_session *r, const char *who, int i, int car, int *out) {
    const long long at = (long long)session_lap_start(r, car) * r->B + car;
    if (at > 0x7fffffffLL) { char msg[160]; snprintf(msg, sizeof(msg), "entry %d: the lap of car %d begins at session row %d, beyond what the entry table addresses with B = %d", i, car, session_lap_start(r, car), r->B); return set_err(LMPC_E_ARG, who, msg); }
    *out = (int)at;
    return LMPC_OK;
}
int lmpc_rollout_commit_laps(lmpc_ctx *c, int n, const int *cars, const int *rows, unsigned stores, int *first_ss, int *first_model) {
    // For i = 0 .. n-1 in the order listed: lmpc_ss_add_trajectory (LMPC.addTrajectory + computeCost, PredictiveControllers.py:418-464) and lmpc_model_add_trajectory
    // (PredictiveModel.addTrajectory, PredictiveModel.py:35-46) of rows [0, rows[i]) of car cars[i] as the session logged them, all in one commit_laps.
    // Checked in full before anything changes; the host vectors are touched only after the launch has completed.
    ARGCHK(c && c->ro && c->ro->active && c->ro->t >= 1 && n >= 1 && cars && stores != 0u && !(stores & ~(LMPC_COMMIT_SS | LMPC_COMMIT_MODEL)));
    lmpc_rollout_session *r = c->ro; const int B = r->B;
    const bool ss = (stores & LMPC_COMMIT_SS) != 0, model = (stores & LMPC_COMMIT_MODEL) != 0;
    for (int i = 0; i < n; i++) ARGCHK(cars[i] >= 0 && cars[i] < B);
    store_rows s; RCCHK(session_rows(c, LMPC_COMMIT_TAIL(n), &s));
    std::vector<int> done((size_t)B);
    HIPCHK(hipMemcpy(done.data(), r->d_done, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
    const int ns0 = (int)c->s_len.size(), nm0 = (int)c->m_len.size();
    std::vector<lmpc_commit_entry> tab((size_t)n);
    std::vector<int> pat; RCCHK(session_parked_at(r, pat));
    for (int i = 0; i < n; i++) {
        const int car = cars[i]; int T;
        RCCHK(session_entry_rows(r, "lmpc_rollout_commit_laps", i, car, rows, done, pat, model ? 2 : 1, &T));
        int src; RCCHK(session_source_index(r, "lmpc_rollout_commit_laps", i, car, &src));
        tab[(size_t)i] = {src, T, ss ? ns0 + i : -1, model ? nm0 + i : -1, track_length_of(c, car)};
    }
    std::vector<double> q0;
    RCCHK(commit_laps(c, s, tab, q0));
    commit_book(c, tab, q0);
    if (first_ss) *first_ss = ss ? ns0 : -1;
    if (first_model) *first_model = model ? nm0 : -1;
    return LMPC_OK;
}

int lmpc_rollout_extend_laps(lmpc_ctx *c, int n, const int *cars, const int *laps, int n_rows, int *extended) {
    // lmpc_ss_extend_lap of rows [0, n_rows) of car cars[i] onto safe-set lap laps[i], for every entry whose rows are all finite; the others are left as they are and
    // reported, all in one extend_laps.
    ARGCHK(c && c->ro && c->ro->active && n >= 1 && cars && laps && extended && n_rows >= 1 && n_rows <= c->ro->t);
    const int stored = (int)c->s_len.size();
    std::vector<char> seen((size_t)stored, 0);
    for (int i = 0; i < n; i++) {
        ARGCHK(cars[i] >= 0 && cars[i] < c->ro->B && laps[i] >= 0 && laps[i] < stored);
        if (seen[(size_t)laps[i]]) { char msg[96]; snprintf(msg, sizeof(msg), "lap %d is listed twice", laps[i]); return set_err(LMPC_E_ARG, "lmpc_rollout_extend_laps", msg); }
        seen[(size_t)laps[i]] = 1;
    }
    { std::vector<int> pat; RCCHK(session_parked_at(c->ro, pat));
      if (!pat.empty()) for (int i = 0; i < n; i++) if (pat[(size_t)cars[i]] >= 0 && n_rows > pat[(size_t)cars[i]]) {
          char msg[160]; snprintf(msg, sizeof(msg), "entry %d: %d rows of car %d, which was parked at step %d (lmpc_rollout_parked_at)", i, n_rows, cars[i], pat[(size_t)cars[i]]);
          return set_err(LMPC_E_ARG, "lmpc_rollout_extend_laps", msg); } }
    // a session that has relaunched: rows [0, n_rows) of a car are those of its current lap, checked against what the lap has logged
    std::vector<int> src;
    if (c->ro->relaunched) {
        src.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            const int logged = c->ro->t - session_lap_start(c->ro, cars[i]);
            if (n_rows > logged) { char msg[160]; snprintf(msg, sizeof(msg), "entry %d: %d rows of car %d, whose lap has logged %d", i, n_rows, cars[i], logged); return set_err(LMPC_E_ARG, "lmpc_rollout_extend_laps", msg); }
            RCCHK(session_source_index(c->ro, "lmpc_rollout_extend_laps", i, cars[i], &src[(size_t)i]));
        }
    }
    store_rows s; RCCHK(session_rows(c, LMPC_EXTEND_TAIL(n), &s));
    return extend_laps(c, s, n, cars, laps, n_rows, extended, -1, src.empty() ? nullptr : src.data());
}

int lmpc_rollout_lap_metrics(lmpc_ctx *c, int n, const int *cars, const int *rows, double *out) {
    // Per entry the reductions of lmpc_metrics.hip.h over rows [0, rows[i]) of car cars[i] as the session logged them, under the row checks of
    // lmpc_rollout_commit_laps; all checked before the launch, nothing of the context or the session is written.  The upload is one buffer: the weights rows the
    // entries name (one for all cars, or one per car: Q, R, xRef, bx, bu of the tuning rows in force, else of the config), then the entry table.
    if (!c) return set_err(LMPC_E_ARG, "lmpc_rollout_lap_metrics", "null context");
    if (!(c->ro && c->ro->active)) return set_err(LMPC_E_STATE, "lmpc_rollout_lap_metrics", "no rollout session is active");
    if (c->ro->relaunched) return set_err(LMPC_E_STATE, "lmpc_rollout_lap_metrics", "the session has relaunched a car (lmpc_rollout_relaunch): its rows no longer count from the session's first");
    ARGCHK(c->ro->t >= 1 && n >= 1 && cars && out);
    lmpc_rollout_session *r = c->ro; const int B = r->B;
    for (int i = 0; i < n; i++) ARGCHK(cars[i] >= 0 && cars[i] < B);
    RCCHK(rows_fit(c->tune, B, LMPC_ROWS_EXACT, "cars", "lmpc_rollout_lap_metrics"));
    const int nw = c->tune.n > 1 ? B : 1;
    const size_t wbytes = sizeof(lmpc_metrics_weights) * (size_t)nw, obytes = sizeof(double) * LMPC_METRICS_NCOL * (size_t)n;
    store_rows s; RCCHK(session_rows(c, obytes + wbytes + sizeof(lmpc_metrics_entry) * (size_t)n, &s));
    std::vector<int> done((size_t)B);
    HIPCHK(hipMemcpy(done.data(), r->d_done, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
    std::vector<int> pat; RCCHK(session_parked_at(r, pat));
    std::vector<char> up(wbytes + sizeof(lmpc_metrics_entry) * (size_t)n);
    lmpc_metrics_weights *w = (lmpc_metrics_weights *)up.data(); lmpc_metrics_entry *tab = (lmpc_metrics_entry *)(up.data() + wbytes);
    double cfg_row[LMPC_TUNING_NPAR]; RCCHK(lmpc_tuning_from_config(&c->cfg, cfg_row));
    for (int b = 0; b < nw; b++) {
        const double *row = c->tune.in_force() ? c->tune.row(b) : cfg_row;
        memcpy(w[b].Q, row + TN_Q, sizeof(w[b].Q)); memcpy(w[b].R, row + TN_R, sizeof(w[b].R)); memcpy(w[b].xRef, row + TN_XREF, sizeof(w[b].xRef));
        memcpy(w[b].bx, row + TN_BX, sizeof(w[b].bx)); memcpy(w[b].bu, row + TN_BU, sizeof(w[b].bu));
    }
    for (int i = 0; i < n; i++) {
        const int car = cars[i]; int T;
        RCCHK(session_entry_rows(r, "lmpc_rollout_lap_metrics", i, car, rows, done, pat, 1, &T));
        tab[i] = {car, T, T == done[(size_t)car] ? 1 : 0, nw > 1 ? car : 0, track_length_of(c, car)};
    }
    double *d_out = (double *)s.tail; char *d_up = (char *)(d_out + LMPC_METRICS_NCOL * (size_t)n);
    lmpc_metrics_args a; a.logX = r->d_logX; a.logU = r->d_logU; a.logG = r->d_logG; a.finX = r->d_finX; a.B = B;
    a.weights = (const lmpc_metrics_weights *)d_up; a.table = (const lmpc_metrics_entry *)(d_up + wbytes);
    memcpy(a.Fx, c->cfg.Fx, sizeof(a.Fx)); memcpy(a.Fu, c->cfg.Fu, sizeof(a.Fu));
    std::vector<double> res(LMPC_METRICS_NCOL * (size_t)n);            // (`out` is the caller's: written only once everything has succeeded)
    hipError_t e = hipMemcpyAsync(d_up, up.data(), up.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { hipLaunchKernelGGL(lmpc_lap_metrics_kernel, dim3((unsigned)n), dim3(LMPC_MET_NT), 0, c->stream, a, d_out); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(res.data(), d_out, obytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return set_err(LMPC_E_HIP, "lmpc_lap_metrics_kernel", hipGetErrorString(e));
    memcpy(out, res.data(), obytes);
    return LMPC_OK;
}

// refresh the per-launch part of the device parameter block
// model_from_table: the regression launch this refresh is for reads a lap table (the context's, or a session's snapshot), whose rows `set` has checked -- the
// sorted-order laps of the block are then not needed.  They are refreshed whenever they exist all the same: what decides is what the LAUNCH reads, and a session
// begun without a table keeps reading the block whatever table the context has been given since.
// ss_from_table: likewise for a solve launch that selects from the safe-set lap table (ss_table_for), whose rows `set` has checked: the block's selection is not
// read and not refreshed -- a row may name one lap numSS_it times, so fewer than numSS_it stored laps are no error then.
static int refresh_params(lmpc_ctx *c, bool need_model, bool need_ss, bool model_from_table = false, bool ss_from_table = false) {
    lmpc_dev_params &p = c->dp;
    if (need_model) {
        const bool have = (int)c->m_order.size() >= c->cfg.trToUse && c->cfg.trToUse >= 1;
        if (!have && !model_from_table) return set_err(LMPC_E_STATE, "regression needs trToUse stored laps", "");
        if (have) for (int i = 0; i < c->cfg.trToUse; i++) { p.mslot[i] = c->m_order[i]; p.mlen[i] = c->m_len[c->m_order[i]]; }   // usedIt = range(trToUse), PredictiveModel.py:31
    }
    if (need_ss && !ss_from_table) {
        const int L = c->cfg.numSS_it, nl = (int)c->s_len.size();
        if (nl < L) return set_err(LMPC_E_STATE, "safe set holds fewer than numSS_it laps", "");
        std::vector<int> sel;
        if (!c->s_override.empty()) { sel = c->s_override; if ((int)sel.size() != L) return set_err(LMPC_E_ARG, "selection override must list numSS_it laps", ""); }
        else {   // argsort(LapTime)[0:numSS_it] (:395,402), stable
            std::vector<int> idx(nl); for (int i = 0; i < nl; i++) idx[i] = i;
            std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return c->s_laptime[a] < c->s_laptime[b]; });
            sel.assign(idx.begin(), idx.begin() + L);
        }
        for (int i = 0; i < L; i++) { if (sel[i] < 0 || sel[i] >= nl) return set_err(LMPC_E_ARG, "selected lap out of range", ""); p.sslot[i] = sel[i]; p.sslapid[i] = sel[i]; p.sslen[i] = c->s_len[sel[i]]; }
        p.cur_it = nl;
    }
    return LMPC_OK;
}

// HIP events around a kernel launch (profiling on).  An event record costs ~4 us on the launch stream -- 15 us per step for the two kernels,
// 5 % of a batch-256 step -- so profiling = k times every k-th launch of a kind only: the average duration is sampled over the run.
static void ev_begin(lmpc_ctx *c, int kind, hipStream_t on) {
    c->ev_open = false;
    if (!c->profiling) return;
    const long long idx = kind == 0 ? c->stats.n_regress : c->stats.n_solve;
    if (idx % c->profiling) return;
    evpair e; hipEventCreate(&e.a); hipEventCreate(&e.b); e.kind = kind; hipEventRecord(e.a, on); c->events.push_back(e); c->ev_open = true;
}
static void ev_end(lmpc_ctx *c, hipStream_t on) { if (c->ev_open) hipEventRecord(c->events.back().b, on); c->ev_open = false; }

// K1 launch shape: queries per work-group shrink (12 -> 6 -> 4 -> ... -> 1) until the grid covers the chip (one work-group per CU is resident)
static void k1_grid(lmpc_ctx *c, int B, int *qg, int *nblk) {
    const int N = c->cfg.N, cands[] = {12, 6, 4, 3, 2, 1};
    int q = 1, np = N;
    for (int k = 0; k < 6; k++) {
        q = k1_queries_per_block(cands[k], c->cfg.trToUse, c->cfg.maxNumPoint); np = (N + q - 1) / q;
        if (c->k1_qg_force > 0) { if (cands[k] <= c->k1_qg_force) break; else continue; }
        if ((long long)B * np >= (long long)c->n_cu) break;      // (two or more groups per CU measured no faster: round 2 26-35 us against 27 us at batch 256; round 5, LMPC_K1_QG = 6 / 4 / 3 / 2: 20 / 27 / 29 / 39 us against 22)
    }
    *qg = q; *nblk = B * np;
}
// The regression kernel in the build that fits the launch: the occupancy build when the grid exceeds one work-group per CU, and the
// 8-rows-per-lane scan when every lap in use lies inside its first quantisation chunk half (<= 512 rows; k1_scan_lap).
// The lap table a regression launch reads: the context's (k1_table_for) or a rollout session's snapshot.  dev == nullptr: none, the laps of the parameter block.
// trk / trkStride: the per-problem tracks of the same launch (lmpc_track_set; null: the parameter block's track)
// ll: parking -- the launch covers the B entries of that list (table builds only: a parking session without a lap table hands in the block's own laps as a one-row table)
struct k1_table { const int *dev; int stride; bool small; const double *trk; int trkStride; lmpc_live_list ll; };      // ll.car != null needs dev != null
// the context's table for a call of B problems (B points for lmpc_regress_points): one row serves all, else row b belongs to problem b and the counts must agree
static int k1_table_for(lmpc_ctx *c, int B, k1_table *t) {
    t->dev = nullptr; t->stride = 0; t->small = true; t->ll = {};
    { trk_src ts; const int rc = track_for(c, B, &ts); if (rc) return rc; t->trk = ts.dev; t->trkStride = ts.stride; }
    if (!c->lt.in_force()) return LMPC_OK;
    RCCHK(rows_fit(c->lt, B, LMPC_ROWS_EXACT, "problems", "lap table"));
    t->dev = (const int *)c->img[IMG_LT].p; t->stride = c->lt.stride(2 * c->cfg.trToUse); t->small = c->lt_small;
    return LMPC_OK;
}
// on: the stream (null: the context's); also: a second copy of A / Bm / C, each pointer or null (step_dev: the caller's arrays beside the hand-over set) -- all null:
// the builds without it, whose text is what it was before there was a second copy
typedef lmpc_k1_also k1_also;
static void launch_k1(lmpc_ctx *c, int nblk, int B, int qg, const double *xLin, int xstride, const double *uLin, double *dA, double *dB, double *dC, int *dst, const k1_table &t,
                      hipStream_t on = nullptr, k1_also also = {}) {
    if (!on) on = c->stream;
    bool small = true;
    if (t.dev) small = t.small;                                          // (every lap named anywhere in the table)
    else for (int i = 0; i < c->cfg.trToUse; i++) small = small && c->dp.mlen[i] - 1 <= 8 * WAVE;
    if (c->k1_force16) small = false;                                    // (LMPC_K1_RPL16 at lmpc_create: A / B of the two scan builds, tests/test_gpu_configs.py)
    const bool occ = nblk > c->n_cu;
    const bool live = t.dev && t.ll.car;
    lmpc_pick([&](auto OCC, auto SMALL, auto TAB, auto LIVE, auto ALSO) {
        constexpr bool o = OCC, tab = TAB; constexpr int rpl = SMALL ? 8 : K1_RPL;
        auto go = [&](auto... lv) { hipLaunchKernelGGL((lmpc_regress_kernel<o, rpl, tab, decltype(lv)...>), dim3(nblk), dim3(K1_NT), 0, on, c->dp, B, qg, xLin, xstride, uLin,
                                                       dA, dB, dC, dst, t.dev, t.stride, t.trk, t.trkStride, lv...); };
        if constexpr (LIVE) { if constexpr (tab && !ALSO) go(t.ll); }   // a parking session: the table builds with the live list (its B entries); never with a second copy
        else if constexpr (ALSO) go(also);
        else go();
    }, occ, small, t.dev != nullptr, live, !live && (also.A || also.Bm || also.C));
}
static int launch_regress(lmpc_ctx *c, int B, const double *d_xLin, int xstride, const double *d_uLin, double *dA, double *dB, double *dC, int *dst,
                          hipStream_t on = nullptr, k1_also also = {}) {
    if (!on) on = c->stream;
    int rc = refresh_params(c, true, false, c->lt.in_force()); if (rc) return rc;
    k1_table tab; rc = k1_table_for(c, B, &tab); if (rc) return rc;
    ev_begin(c, 0, on);                                       // (a look-ahead launch: its events lie on that stream, and the time between them includes its wait for a free CU)
    int qg, nblk; k1_grid(c, B, &qg, &nblk);
    launch_k1(c, nblk, B, qg, d_xLin, xstride, d_uLin, dA, dB, dC, dst, tab, on, also);
    ev_end(c, on);
    HIPCHK(hipGetLastError());
    c->stats.n_regress++;
    return LMPC_OK;
}
extern "C" int lmpc_solver_waves(lmpc_ctx *c, int B);
// Retry pass on demand.  The adaptive equal / separate step rule can fall into a two-cycle (a separate step feeds (alpha_p - alpha_d) H dw into
// the dual residual, the next equal step is blocked): a few problems per million ended at the iteration limit that way in round 1, and most
// of them converge in 10-12 iterations from the start point with equal steps only (lmpc_solve_kernel<N, S, true>).  Rounds 1-2 launched that
// retry kernel behind EVERY solve -- 4.4 us per step in which all work-groups return at once (1.9 % of a batch-256 step, 3 % at batch 1).  Now a
// problem that needs it says so itself: it writes the launch's epoch into a host-mapped ring (flag_retry, system-scope atomic), and the host
// looks at the ring at its next drain of the stream, before any result of the launch can be read: lmpc_step_batch / lmpc_qp_solve_batch
// right after the solve, the device-resident path in lmpc_dev_sync / lmpc_dev_download / lmpc_dev_free.  The retry kernel skips problems
// whose CURRENT status word is clean, so a flagged launch whose buffers a later launch reused is handled correctly.  Closed-loop rollouts
// (lmpc_rollout_run), where the plant consumes uPred without a host round trip, keep the unconditional launch (immediate = true).
static int resolve_retries(lmpc_ctx *c) {
    if (c->pending.empty()) return LMPC_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    int rc = LMPC_OK, launched = 0;
#if defined(LMPC_DEV_FAST) || defined(LMPC_TRACE) || defined(LMPC_TIMING)
    static const bool no_retry = dev_knob("LMPC_NO_RETRY") != nullptr;     // (developer probe, developer flavours only: leave the first pass's output as it is, tools/n40_probe.py)
#else
    const bool no_retry = false;
#endif
    for (auto &pe : c->pending) {
        if (no_retry || c->h_retry[pe.epoch % LMPC_RETRY_RING] != pe.epoch) continue;
        pe.io.retry_flag = nullptr;
        // the retry runs against the parameter block of ITS launch (selected laps, lap lengths, cur_it), not the context's current one
        rc = c->var.launch_retry(c->stream, pe.dp, pe.B, pe.io, nullptr); if (rc) break;
        if (hipGetLastError() != hipSuccess) { rc = set_err(LMPC_E_HIP, "retry launch", ""); break; }
        c->stats.n_retry++; launched++;
    }
    c->pending.clear();
    // nothing is in flight that could still write the ring: start the epochs over (they never grow past the ring size, so the signed
    // counter cannot overflow and `epoch % ring` stays a valid slot)
    if (rc == LMPC_OK && launched && hipStreamSynchronize(c->stream) != hipSuccess) rc = set_err(LMPC_E_HIP, "hipStreamSynchronize", "retry pass");
    c->epoch = 0; memset(c->h_retry, 0, sizeof(int) * LMPC_RETRY_RING);
    return rc;
}
// Per-problem safe-set laps (lmpc_ss_set_lap_table) for a launch of B problems that selects on the device: B against the rows, the device image brought up to date,
// io.ssTab / io.ssTabStride set.  No table: io stays as it is (the selection of the parameter block).  Called before the first launch of a step (step_dev,
// lmpc_rollout_run), so that a refused batch leaves nothing half done, and by launch_solve for every other caller.
// The image is rebuilt from the indices whenever the safe set has been edited since the last upload: an entry holds the lap's CURRENT rows, and with last = NULL
// the latest lap is the last one stored at launch time.  Launches still pending their retry pass read the image of THEIR launch: they are resolved, and the
// stream is drained, before it is overwritten.
static int ss_table_for(lmpc_ctx *c, int B, lmpc_solve_io *io) {
    if (!c->sst.in_force() || c->cfg.numSS_it == 0 || !(io->mode & 1)) return LMPC_OK;
    RCCHK(rows_fit(c->sst, B, LMPC_ROWS_EXACT, "problems", "safe-set lap table"));
    const int L = c->cfg.numSS_it;
    if (c->sst_dirty) {
        RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
        const int latest_shared = (int)c->s_len.size() - 1;
        std::vector<int> img((size_t)c->sst.n * L * LMPC_SSTAB_ENTRY, 0), o((size_t)L);
        for (int r = 0; r < c->sst.n; r++) {
            // the order a controller holding only these laps would use them: argsort(LapTime), stable (:395, :402) -- ascending LapTime, ties by lap index
            std::copy(c->sst.row(r), c->sst.row(r) + L, o.begin());
            std::sort(o.begin(), o.end(), [&](int a, int b) { return c->s_laptime[a] != c->s_laptime[b] ? c->s_laptime[a] < c->s_laptime[b] : a < b; });
            const int latest = c->sst_has_last ? c->sst_last[r] : latest_shared;
            for (int l = 0; l < L; l++) {
                int *e = &img[((size_t)r * L + l) * LMPC_SSTAB_ENTRY];
                e[0] = o[l]; e[1] = c->s_len[o[l]]; e[2] = o[l] == latest ? 1 : 0;       // (safe-set lap index == slot)
            }
        }
        RCCHK(image_upload(&c->img[IMG_SST], img.data(), img.size() * sizeof(int), "hipMemcpy (safe-set table image)"));
        c->sst_dirty = false; c->sst_upload_broke = true;      // (a step with something to upload runs unchained, step_dev)
    }
    io->ssTab = (const int *)c->img[IMG_SST].p; io->ssTabStride = c->sst.stride(L * LMPC_SSTAB_ENTRY);
    return LMPC_OK;
}
// Per-problem controller tuning (lmpc_tuning_set) for a launch of B problems that solves: B against the rows, io.tune / io.tuneStride set.  No rows in force, or a
// launch that only selects (the selection reads no weights): io stays as it is.  Called where ss_table_for is, before the first launch of a step.
static int tuning_for(lmpc_ctx *c, int B, lmpc_solve_io *io) {
    if (!c->tune.in_force() || !(io->mode & 2)) return LMPC_OK;
    RCCHK(rows_fit(c->tune, B, LMPC_ROWS_EXACT, "problems", "tuning rows"));
    io->tune = (const double *)c->img[IMG_TUNE].p; io->tuneStride = c->tune.stride(PAR_TOT);
    return LMPC_OK;
}
// The device image of n rows (n = 0: the config's own row).  Launches still pending their retry pass read the image of THEIR launch: they are resolved, and the stream
// is drained, before it is overwritten (as ss_table_for does for the safe-set table).
static int tuning_upload(lmpc_ctx *c, int n, const double *rows) {
    double own[LMPC_TUNING_NPAR];
    if (n == 0) { lmpc_tuning_from_config(&c->cfg, own); rows = own; }
    const int nr = n == 0 ? 1 : n;
    std::vector<double> img((size_t)nr * PAR_TOT);
    for (int r = 0; r < nr; r++) tuning_image_row(c->cfg, rows + (size_t)r * LMPC_TUNING_NPAR, &img[(size_t)r * PAR_TOT]);
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    return image_upload(&c->img[IMG_TUNE], img.data(), img.size() * sizeof(double), "hipMemcpy (tuning image)");
}
// ll (parking sessions; ll.car null: none): the live list and its entries -- what the kernels are launched over; B stays the session's batch, which the per-car rows are
// checked against and the abPack scratch is sized for.  reroute (LMPC_PARK_REROUTE): the route (waves per QP) follows ll.n instead of B.  The choice between [A_k | B_k] in
// LDS and in the abPack scratch (long horizons) stays with B on either route: a rerouted one-wave launch at N = 40 may take the global-memory build where a session of
// nLive cars would not -- same QP answer to the routes' bound, not the same kernel
static int launch_solve(lmpc_ctx *c, int B, const lmpc_solve_io &io_in, bool immediate = false, lmpc_live_list ll = {}, bool reroute = false, const k1_also *retry_abc = nullptr) {
    lmpc_solve_io io = io_in;
    const int Bl = ll.car ? ll.n : B, Br = (ll.car && reroute) ? ll.n : B;      // problems launched; the batch the route is chosen for
    if (!io.ssTab) { const int rc = ss_table_for(c, B, &io); if (rc) return rc; }
    if (!io.tune) { const int rc = tuning_for(c, B, &io); if (rc) return rc; }
    // (per-problem tracks, lmpc_track_set: the selection reads the problem's TrackLength; B against the rows)
    if (!io.trk && (io.mode & 1)) { trk_src ts; const int rc = track_for(c, B, &ts); if (rc) return rc; io.trk = ts.dev; io.trkStride = ts.stride; }
    if ((io.ssTab || io.trk || ll.car) && !io.tune) { io.tune = (const double *)c->img[IMG_TUNE].p; io.tuneStride = 0; }      // (a table or tracks alone: the per-problem-rows kernels stage the config's own row -- or, selecting only, read none)
    // [A_k | B_k] from global memory only when the batch does not fit the CUs with it in LDS (N = 40: more than two QPs per CU); a batch that
    // fits runs 3 % faster from LDS (measured at N = 40, batch 512: 0.997 vs 1.030 ms)
    io.abPack = nullptr;
    if (c->ab_pack && (long long)B > (long long)(160 * 1024 / c->var.lds_1w) * c->n_cu) {
        if ((size_t)B > c->ab_pack_cap) {                   // rollout sessions may run more problems than max_batch: the scratch follows
            int rc = resolve_retries(c); if (rc) return rc;
            HIPCHK(hipStreamSynchronize(c->stream));
            (void)g_free(c->ab_pack); c->ab_pack = nullptr; c->ab_pack_cap = 0;
            HIPCHK(g_malloc(&c->ab_pack, sizeof(double) * 48 * (size_t)c->cfg.N * (size_t)B)); c->ab_pack_cap = (size_t)B;
        }
        io.abPack = c->ab_pack;
    }
    const bool deferred = (io.mode & 2) && !immediate && !io.tbuf;       // (the retry pass of a traced launch would overwrite the trace rows: traced builds still defer, the rows of a retried problem are its retry's)
    if (deferred) {
        if ((int)c->pending.size() >= LMPC_RETRY_RING - 1) { int rc = resolve_retries(c); if (rc) return rc; }
        c->epoch++; io.retry_epoch = c->epoch; io.retry_flag = c->d_retry + (c->epoch % LMPC_RETRY_RING);
    }
    const bool term = c->cfg.numSS_it > 0;
    int rc = refresh_params(c, false, term && (io.mode & 1), false, io.ssTab != nullptr); if (rc) return rc;
    const bool timing_buf = io.tbuf != nullptr;              // (the cycle-stamp build pins the kernel route; the trace build below must not)
#ifdef LMPC_TRACE
    if (!io.tbuf && c->dbg_trace && (io.mode & 2)) io.tbuf = (long long *)c->dbg_trace;
#endif
    ev_begin(c, 1, c->stream);
    // waves per QP: 4 up to one QP per CU, 2 up to mw2_max_batch (four QPs per CU at N <= 12, see create_body), beyond that the one-wave
    // kernel, whose slim LDS layout keeps eight QPs resident per CU at N = 12
#ifdef LMPC_DEV_FAST
    if (const char *f = dev_knob("LMPC_FORCE_NW")) {
        const int nw = atoi(f);
        rc = nw == 4 ? c->var.launch_mw4(c->stream, c->dp, Bl, io, ll.car) : nw == 2 ? c->var.launch_mw2(c->stream, c->dp, Bl, io, ll.car) : c->var.launch_1w(c->stream, c->dp, Bl, io, ll.car);
    } else
#endif
    // (a safe-set lap table, tuning rows: the condensed kernel has no per-problem lookup -- it takes Q pre-digested by the host, cd_hasq -- and is not taken: the kernels below serve them)
    // (parking: the list comes with io.tune, so the condensed kernel is not taken; Br <= B, so the four-wave launch has nLive <= mw_max_batch on either route)
    rc = (c->cd_ok && c->cd_mode == 1 && !(io.mode & 4) && !io.tune && !c->trk.in_force()) ? c->var.launch_cd(c->stream, c->dp, Bl, io, c->cd_hasq)
       : (io.mode & 4) ? c->var.launch_1w(c->stream, c->dp, Bl, io, ll.car)        // fused step: the one-wave kernel runs the regression itself
       : (Br <= c->mw_max_batch && (!timing_buf || dev_knob("LMPC_TIMING_MW"))) ? c->var.launch_mw4(c->stream, c->dp, Bl, io, ll.car)
       : (lmpc_solver_waves(c, Br) == 2 && !timing_buf) ? c->var.launch_mw2(c->stream, c->dp, Bl, io, ll.car) : c->var.launch_1w(c->stream, c->dp, Bl, io, ll.car);
    ev_end(c, c->stream);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    c->stats.n_solve++; if (io.mode & 2) c->stats.qp_solved += Bl;
    if (deferred) {
        // the retry pass reads what the CALLER holds for this launch where there is such a thing (retry_abc: the caller's arrays, which it keeps until lmpc_dev_sync), not
        // the hand-over set the first pass read, which a later step's regression overwrites; shared_abc: some of it still is a hand-over set of the context's
        lmpc_solve_io pio = io;
        if (retry_abc) { pio.A = retry_abc->A; pio.Bm = retry_abc->Bm; pio.C = retry_abc->C; }
        bool shared = false;
        for (const auto &h : c->ho) shared = shared || (h.A && (pio.A == h.A || pio.Bm == h.Bm || pio.C == h.C));
        c->pending.push_back({pio, Bl, io.retry_epoch, c->dp, shared});
    }
    else if (io.mode & 2) {
        rc = c->var.launch_retry(c->stream, c->dp, Bl, io, ll.car);
        if (rc) return rc;
        HIPCHK(hipGetLastError());
    }
    return LMPC_OK;
}
// The held solve of the context (lmpc_ctx::held), launched: stand-alone (next null: a flush -- ctx_enter, or a step that cannot carry it) or as the solve role of a
// two-role launch whose other work-groups run the regression *next.  What launch_solve keeps of a launch is kept here, when the launch happens: the retry ring and the
// pending entry, the counters, and the profiling events -- around the whole launch, a solve's; a regression inside a two-role launch is counted, not timed.
static int launch_held(lmpc_ctx *c, const lmpc_k1_next *next) {
    const lmpc_ctx::held_solve h = c->held; c->has_held = false;
    lmpc_solve_io io = h.io;
    if ((int)c->pending.size() >= LMPC_RETRY_RING - 1) RESOLVE_PENDING();
    c->epoch++; io.retry_epoch = c->epoch; io.retry_flag = c->d_retry + (c->epoch % LMPC_RETRY_RING);
    ev_begin(c, 1, c->stream);
    const int rc = next ? c->var.launch_mw4_next(c->stream, h.dp, h.B, io, *next) : c->var.launch_mw4(c->stream, h.dp, h.B, io, nullptr);
    ev_end(c, c->stream);
    if (rc) return set_err(LMPC_E_STATE, "held solve", "no launcher");
    HIPCHK(hipGetLastError());
    c->stats.n_solve++; c->stats.qp_solved += h.B;
    if (next) { c->stats.n_regress++; c->n_merged++; } else c->n_held_flushed++;
    lmpc_solve_io pio = io; pio.A = h.retry_abc.A; pio.Bm = h.retry_abc.Bm; pio.C = h.retry_abc.C;      // (the caller's arrays: a step is held only where it gave all three)
    c->pending.push_back({pio, h.B, io.retry_epoch, h.dp, false});
    return LMPC_OK;
}
// Which steps take the merged form of the look-ahead: the plain four-wave solve at up to one QP per CU (the only kernel with a two-role build), nothing per problem in
// force (lap table, safe-set table, tuning rows, track rows: other instantiations), the caller's own A / Bm / C (the retry pass of a held solve reads them), and not
// lmpc_set_profiling(1), which asks for the duration of EVERY kernel of a kind: a regression inside a two-role launch has none of its own.
static bool k1_merge_ok(const lmpc_ctx *c, int B, const lmpc_arrays &a) {
    if (!c->k1_merge || !c->var.launch_mw4_next || B > c->mw_max_batch || B > c->n_cu || !(a.A && a.Bm && a.C) || c->profiling == 1) return false;
    if ((c->cd_ok && c->cd_mode == 1) || c->dbg_trace) return false;
#ifdef LMPC_DEV_FAST
    if (getenv("LMPC_FORCE_NW")) return false;
#endif
    return !c->lt.in_force() && !c->sst.in_force() && !c->tune.in_force() && !c->trk.in_force();
}

#define H2D(dst, src, n) HIPCHK(hipMemcpyAsync(dst, src, sizeof(*(dst)) * (size_t)(n), hipMemcpyHostToDevice, c->stream))
#define D2H(dst, src, n) do { if (dst) HIPCHK(hipMemcpyAsync(dst, src, sizeof(*(src)) * (size_t)(n), hipMemcpyDeviceToHost, c->stream)); } while (0)

// For B problems, copy every array that both sides name: a NULL pointer on either side skips the array, and so does an array without elements (S = 0).
// src_first: the first problem on the source side.  hipMemcpyHostToHost: the host-mapped mirrors, a plain memcpy; else asynchronous on the context's stream.
static int copy_arrays(lmpc_ctx *c, size_t B, const lmpc_dims &d, const lmpc_arrays &dst, const lmpc_arrays &src, hipMemcpyKind kind, size_t src_first = 0) {
    hipError_t e = hipSuccess;
    lmpc_arrays_each(d, [&](const char *, auto m, size_t elem, size_t n, int) {
        if (!(dst.*m) || !(src.*m) || !n || e != hipSuccess) return;
        if (kind == hipMemcpyHostToHost) memcpy(dst.*m, src.*m + src_first * n, elem * n * B);
        else e = hipMemcpyAsync(dst.*m, src.*m + src_first * n, elem * n * B, kind, c->stream);
    });
    return e == hipSuccess ? LMPC_OK : set_err(LMPC_E_HIP, "hipMemcpyAsync", hipGetErrorString(e));
}
// hasPred / timeStep a caller did not give are zeros in the work buffers
static int zero_absent_flags(lmpc_ctx *c, int B, const lmpc_arrays &in) {
    if (!in.hasPred) HIPCHK(hipMemsetAsync(c->w.hasPred, 0, sizeof(int) * B, c->stream));
    if (!in.timeStep) HIPCHK(hipMemsetAsync(c->w.timeStep, 0, sizeof(int) * B, c->stream));
    return LMPC_OK;
}
// What a solve launch reads and writes, from a set of arrays.  mode bit 0 (selection on the device): the selection's inputs and its outputs, else ssSel / qSel are
// inputs; bit 1 (QP solve): the QP's data and its answer.  An array the caller does not want written it leaves NULL in `a`; what is special to one caller
// (rstatus, tbuf, the fused step's xLin / uLin / Aout / Bout / Cout) it sets itself.
static lmpc_solve_io solve_io(int mode, const lmpc_arrays &a) {
    lmpc_solve_io io; memset(&io, 0, sizeof(io));
    io.mode = mode; io.x0 = a.x0; io.status = a.status; io.iters = a.iters;
    if (mode & 1) {
        io.zt = a.zt; io.xPredPrev = a.xPredPrev; io.hasPred = a.hasPred; io.timeStep = a.timeStep;
        io.ssSelOut = a.ssSel; io.qSelOut = a.qSel; io.succOut = a.succ; io.succUOut = a.succU; io.ztUsed = a.ztUsed; io.selStartOut = a.selStart;
    } else { io.ssSelIn = a.ssSel; io.qSelIn = a.qSel; }
    if (mode & 2) {
        io.A = a.A; io.Bm = a.Bm; io.C = a.C; io.uOld = a.uOld;
        io.xPred = a.xPred; io.uPred = a.uPred; io.slack = a.slack; io.lambda = a.lambda; io.sTerm = a.sTerm; io.mu = a.mu;
        io.ztNext = a.ztNext; io.ztuNext = a.ztuNext; io.resid = a.resid;
    }
    return io;
}

// iteration counts of the batch just solved into the work buffers: copied to the caller (if asked) and added to lmpc_stats.ipm_iters; synchronises the stream.  mirror: they
// are on the host already (host-mapped route of lmpc_step_batch) and only added.  (host-buffer entry points only: the device-resident path leaves them in the caller's buffer)
static int fetch_iters(lmpc_ctx *c, int B, int *iters, const int *mirror = nullptr) {
    std::vector<int> tmp;
    if (!mirror) {
        if (!iters) { tmp.resize((size_t)B); iters = tmp.data(); }
        HIPCHK(hipMemcpyAsync(iters, c->w.iters, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        mirror = iters;
    }
    for (int b = 0; b < B; b++) c->stats.ipm_iters += mirror[b];
    return LMPC_OK;
}

int lmpc_regress_batch(lmpc_ctx *c, int B, const double *xLin, int xLinRowStride, const double *uLin, double *A, double *Bm, double *C, int *status) {
    ARGCHK(c && xLin && uLin && A && Bm && C && B >= 1 && B <= c->cfg.max_batch);
    const int N = c->cfg.N;
    ARGCHK(xLinRowStride == N * 6 || xLinRowStride == (N + 1) * 6);
    RCCHK(ctx_enter(c)); RESOLVE_PENDING();          // (a pending launch may hand its A / B / C over through the work buffers: its retry pass first)
    { k1_table tab; const int rc = k1_table_for(c, B, &tab); if (rc) return rc; }      // (B against the lap table's rows: refused before anything is queued)
    lmpc_arrays in = {}, out = {}; in.uLin = mut(uLin); out.A = A; out.Bm = Bm; out.C = C; out.rstatus = status;
    H2D(c->w.xLin, xLin, (size_t)B * xLinRowStride);                 // (rows of N or N + 1 points: the caller's stride, not the table's size)
    RCCHK(copy_arrays(c, B, c->dims, c->w, in, hipMemcpyHostToDevice));
    RCCHK(launch_regress(c, B, c->w.xLin, xLinRowStride, c->w.uLin, c->w.A, c->w.Bm, c->w.C, c->w.rstatus));
    RCCHK(copy_arrays(c, B, c->dims, out, c->w, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

// hasPred without xPredPrev: the selection's Q-function shift (:502-512) would read predictions nobody supplied -- stale rows of the work buffer through the host entry
// points, a null pointer on the device through lmpc_step_batch_dev.  Host arrays are scanned (an all-zero hasPred is what callers pass on a first step); device arrays cannot be.
static bool pred_args_ok(int B, const double *xPredPrev, const int *hasPred) {
    if (!hasPred || xPredPrev) return true;
    for (int i = 0; i < B; i++) if (hasPred[i]) return false;
    return true;
}
int lmpc_regress_points(lmpc_ctx *c, int n, const double *x, const double *u, double *A, double *Bm, double *C, int *status) {
    // PredictiveModel.regressionAndLinearization (PredictiveModel.py:48-197) for n independent linearisation points (x (n x 6), u (n x 2)): the reference's own call
    // shape -- one point per call -- without a horizon around it.  The regression kernel runs with a parameter block whose horizon is 1: one query per work-group.
    ARGCHK(c && x && u && A && Bm && C && n >= 1 && (long long)n <= (long long)c->cfg.max_batch * c->cfg.N);
    RCCHK(ctx_enter(c)); RESOLVE_PENDING();          // (see lmpc_regress_batch)
    k1_table tab; { const int rc = k1_table_for(c, n, &tab); if (rc) return rc; }      // (point e uses row e)
    const lmpc_dims one = {1, c->dims.S, c->dims.L};                 // n problems of horizon 1: the table's sizes of uLin, A, Bm, C, rstatus
    lmpc_arrays in = {}, out = {}; in.uLin = mut(u); out.A = A; out.Bm = Bm; out.C = C; out.rstatus = status;
    H2D(c->w.xLin, x, (size_t)n * 6);                                // (one row per point, not the two of a horizon-1 trajectory)
    RCCHK(copy_arrays(c, n, one, c->w, in, hipMemcpyHostToDevice));
    int rc = refresh_params(c, true, false, tab.dev != nullptr); if (rc) return rc;
    {
        const lmpc_dev_params keep = c->dp;
        c->dp.N = 1;                                                     // (launch_k1 passes c->dp by value)
        ev_begin(c, 0, c->stream);
        launch_k1(c, n, n, 1, c->w.xLin, 6, c->w.uLin, c->w.A, c->w.Bm, c->w.C, c->w.rstatus, tab);
        ev_end(c, c->stream);
        c->dp = keep;
    }
    HIPCHK(hipGetLastError());
    c->stats.n_regress++;
    RCCHK(copy_arrays(c, n, one, out, c->w, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_select_batch(lmpc_ctx *c, int B, const double *x0, const double *zt, const double *xPredPrev, const int *hasPred, const int *timeStep,
                      double *ssSel, double *qSel, double *succ, double *succU, double *ztUsed, int *selStart, int *status) {
    ARGCHK(c && x0 && zt && B >= 1 && B <= c->cfg.max_batch && c->cfg.numSS_it > 0);
    ARGCHK(pred_args_ok(B, xPredPrev, hasPred));
    RCCHK(ctx_enter(c));
    lmpc_arrays in = {}, out = {};
    in.x0 = mut(x0); in.zt = mut(zt); in.xPredPrev = mut(xPredPrev); in.hasPred = mut(hasPred); in.timeStep = mut(timeStep);
    out.ssSel = ssSel; out.qSel = qSel; out.succ = succ; out.succU = succU; out.ztUsed = ztUsed; out.selStart = selStart; out.status = status;
    RCCHK(copy_arrays(c, B, c->dims, c->w, in, hipMemcpyHostToDevice)); RCCHK(zero_absent_flags(c, B, in));
    RCCHK(launch_solve(c, B, solve_io(1, c->w)));
    RCCHK(copy_arrays(c, B, c->dims, out, c->w, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

// the data of a batch of QPs given as host arrays (lmpc_qp_solve_batch, lmpc_assemble_batch, lmpc_debug_timing) into the work buffers
static int upload_qp(lmpc_ctx *c, int B, const double *A, const double *Bm, const double *C, const double *x0, const double *uOld, const double *ssSel, const double *qSel) {
    lmpc_arrays in = {}; in.A = mut(A); in.Bm = mut(Bm); in.C = mut(C); in.x0 = mut(x0); in.uOld = mut(uOld); in.ssSel = mut(ssSel); in.qSel = mut(qSel);
    return copy_arrays(c, B, c->dims, c->w, in, hipMemcpyHostToDevice);
}
// the arrays a plain solve of such a batch works on: everything but ztNext / ztuNext, which these entry points do not return
static lmpc_arrays qp_arrays(const lmpc_ctx *c) { lmpc_arrays a = c->w; a.ztNext = a.ztuNext = nullptr; return a; }

int lmpc_qp_solve_batch(lmpc_ctx *c, int B, const double *A, const double *Bm, const double *C, const double *x0, const double *uOld,
                        const double *ssSel, const double *qSel, double *xPred, double *uPred, double *slack, double *lambda, double *sTerm,
                        double *mu, int *status, int *iters, double *resid) {
    ARGCHK(c && A && Bm && C && x0 && uOld && xPred && uPred && B >= 1 && B <= c->cfg.max_batch);
    const bool term = c->dims.S > 0;
    if (term) ARGCHK(ssSel && qSel);
    RCCHK(ctx_enter(c)); RESOLVE_PENDING();          // (see lmpc_regress_batch: the copies below overwrite the A / B / C work buffers)
    RCCHK(upload_qp(c, B, A, Bm, C, x0, uOld, ssSel, qSel));
    RCCHK(launch_solve(c, B, solve_io(2, qp_arrays(c))));
    RCCHK(resolve_retries(c));                           // drains the stream; a flagged problem gets its retry pass before anything is copied out
    lmpc_arrays out = {};
    out.xPred = xPred; out.uPred = uPred; out.slack = slack; out.mu = mu; out.status = status; out.resid = resid;
    if (term) { out.lambda = lambda; out.sTerm = sTerm; }
    RCCHK(copy_arrays(c, B, c->dims, out, c->w, hipMemcpyDeviceToHost));
    return fetch_iters(c, B, iters);                     // synchronises the stream
}

// The look-ahead stream, its two events and the second hand-over set: made by the first chained step of a context, so that contexts that never queue steps (the
// drop-in classes, LMPC_K1_AHEAD=0) hold what they held before.
// The stream gets the LOWEST stream priority.  The runtime deals its few hardware queues to streams per priority class: two streams of one class can share a
// queue, and a look-ahead stream that shared the context's queue ran every regression BEHIND the solve it was meant to run beside (measured with one other
// context alive in the process: 210 us per batch-256 step against 192 unchained, 185 with queues of their own).  A class of its own cannot collide with `stream`;
// and when a solve and the next regression become ready together the solve's work-groups are placed first, which is the order that measured well.
// (hipEventReleaseToDevice on both events: measured, the same 13 us between two solves.)
static int k1_ahead_setup(lmpc_ctx *c) {
    // (each piece only if it is missing: a failure half way leaves what exists to lmpc_destroy, and the next chained step makes the rest)
    if (!c->k1_stream) { int least = 0, greatest = 0; HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest)); HIPCHK(hipStreamCreateWithPriority(&c->k1_stream, hipStreamDefault, least)); }
    if (!c->e_k1) HIPCHK(hipEventCreateWithFlags(&c->e_k1, hipEventDisableTiming));
    if (!c->e_front) HIPCHK(hipEventCreateWithFlags(&c->e_front, hipEventDisableTiming));
    const size_t nb = (size_t)c->cfg.max_batch * (size_t)c->cfg.N;
    lmpc_ctx::handover &h = c->ho[1];
    if (!h.A) HIPCHK(g_malloc(&h.A, sizeof(double) * 36 * nb));
    if (!h.Bm) HIPCHK(g_malloc(&h.Bm, sizeof(double) * 12 * nb));
    if (!h.C) HIPCHK(g_malloc(&h.C, sizeof(double) * 6 * nb));
    if (!h.rstatus) HIPCHK(g_malloc(&h.rstatus, sizeof(int) * nb));      // (the last piece: what step_dev looks at)
    return LMPC_OK;
}
// Which batches chain: up to k1_ahead_max_batch problems (create_body: the rule, and LMPC_K1_AHEAD_MAX_BATCH for experiments)
static bool k1_ahead_pays(const lmpc_ctx *c, int B) { return B <= c->k1_ahead_max_batch; }
// one step on device arrays: the body of lmpc_step_batch_dev, which lmpc_step_batch runs on the work buffers or their host-mapped mirrors
static int step_dev(lmpc_ctx *c, int B, const lmpc_arrays &a) {
    ARGCHK(B >= 1 && a.x0 && a.xLin && a.uLin && a.uOld && a.xPred && a.uPred && a.status && a.iters);
    const int N = c->cfg.N; const bool term = c->cfg.numSS_it > 0;
    if (term) ARGCHK(a.zt != nullptr);
    ARGCHK(!a.hasPred || a.xPredPrev);                   // (device arrays: a set hasPred[b] would dereference the missing predictions inside the kernel)
    bool was_chain = c->chain;                           // (the previous call was a two-kernel step_dev and nothing has been queued or edited since)
    RCCHK(ctx_enter(c, true));                           // (a held solve stays held: launched below, with this step's regression or in front of this step)
    ARGCHK(B <= c->cfg.max_batch);                      // the work buffers (per-point regression status, A, B, C hand-over) are sized for max_batch
    // Regression kernel, then the solve kernel; A, Bm, C are optional outputs (the hand-over then uses the context's work buffers).
    // With LMPC_FUSE=1 batches that run one wave per QP take the fused step instead: every wave runs the regression of its own QP in
    // front of the solve and [A_k | B_k], C_k never leave LDS (see lmpc_create for the measurement that keeps it off by default).
    { k1_table tab; const int rc = k1_table_for(c, B, &tab); if (rc) return rc; }      // (B against the lap table's rows: refused before anything is queued)
    // (a lap table in force: the fused form reads the laps of the parameter block -- it lives in the variant libraries -- so the two-kernel step runs)
    // (likewise a safe-set lap table, lmpc_ss_set_lap_table: the fused form's LDS layout has no room behind it for the selected laps)
    // (likewise tuning rows, lmpc_tuning_set: the fused form has no per-problem-rows instantiation)
    const bool fused = c->fuse_k1 && lmpc_solver_waves(c, B) == 1 && !c->lt.in_force() && !(term && c->sst.in_force()) && !c->tune.in_force() && !c->trk.in_force();      // (likewise track rows, lmpc_track_set)
    lmpc_solve_io io = solve_io((fused ? 4 : 0) | (term ? 3 : 2), a);
    // The merged form of the look-ahead (lmpc_ctx::held): a chained step on a route with a two-role build.  Its regression is launched now -- in one launch with the solve
    // held by the step before, or in a kernel of its own behind everything queued where none is held (the second step of a chain) -- and its own solve is held.
    // Any other step first launches a held solve stand-alone and then runs unchained: such a solve lies behind no e_front record a look-ahead regression could wait for.
    const bool merged = was_chain && !c->sst_upload_broke && !fused && c->k1_ahead && k1_ahead_pays(c, B) && k1_merge_ok(c, B, a);
    if (c->has_held && !merged) { RCCHK(launch_held(c, nullptr)); was_chain = false; }
    if (fused || !c->k1_ahead || !k1_ahead_pays(c, B)) {      // the step of before: one stream, the caller's A / Bm / C as the hand-over where given; it starts no chain
        double *dA = a.A ? a.A : c->w.A, *dB = a.Bm ? a.Bm : c->w.Bm, *dC = a.C ? a.C : c->w.C;
        // A, Bm, C not given: the hand-over goes through the context's own buffers, which this launch's regression overwrites -- a launch still
        // pending its retry pass that used them is resolved first (a stream drain).  Callers that queue launches back to back pass their own
        // A / Bm / C (racinglmpc_amd._capi.Context.step_dev_buffers does) and keep every buffer of a launch untouched until lmpc_dev_sync.
        if (dA == c->w.A || dB == c->w.Bm || dC == c->w.C) for (const auto &pe : c->pending) if (pe.shared_abc) { RESOLVE_PENDING(); break; }
        RCCHK(ss_table_for(c, B, &io));                       // (B against the safe-set lap table's rows: refused before the regression is queued)
        RCCHK(tuning_for(c, B, &io));                         // (and against the tuning rows)
        io.A = dA; io.Bm = dB; io.C = dC;
        // (io.rstatus / the fused regression: a singular regression or an off-track linearisation point marks status[b]; the reference raises there)
        if (fused) { io.xLin = a.xLin; io.uLin = a.uLin; io.Aout = a.A; io.Bout = a.Bm; io.Cout = a.C; RCCHK(refresh_params(c, true, false)); }
        else { RCCHK(launch_regress(c, B, a.xLin, (N + 1) * 6, a.uLin, dA, dB, dC, c->w.rstatus)); io.rstatus = c->w.rstatus; c->n_k1_unchained++; c->n_k1_alone++; }
        return launch_solve(c, B, io);
    }
    // The look-ahead form.  The regression writes one of the context's two hand-over sets -- and the caller's A / Bm / C beside it, where given -- and the solve's
    // first pass reads that set, never the caller's arrays: the regression of the NEXT queued step may then run beside this solve, since it writes the other set (and
    // the caller's arrays, which nothing on the device reads any more).  A step that is not chained takes set 0 with its regression on the context's stream, as
    // before; a chained step i + 1 takes the other set than step i, on k1_stream:
    //     k1_stream waits for e_front(i) | K1(i + 1) | e_k1 | stream waits for e_k1 | e_front(i + 1) on stream | K3(i + 1)
    // e_front(i) lies on `stream` behind the wait for K1(i) and in front of K3(i): K1(i + 1) is ordered behind K3(i - 1), the last first-pass reader of its set, and
    // behind K1(i) (the caller's arrays are written in step order) -- not behind K3(i).  Every K3 waits for its K1, so a drain of `stream` leaves k1_stream idle.
    RCCHK(ss_table_for(c, B, &io));                           // (B against the safe-set lap table's rows: refused before the regression is queued; an upload drains and breaks the chain)
    RCCHK(tuning_for(c, B, &io));                             // (and against the tuning rows)
    const bool chained = was_chain && !c->sst_upload_broke;
    c->sst_upload_broke = false;
    if (chained && !c->ho[1].rstatus) {                       // the first chained step of the context
        RCCHK(k1_ahead_setup(c));
        // (the step before ran when there was no event to record: this one's regression waits for a record BEHIND that step's solve -- ordered, once without the overlap)
        HIPCHK(hipEventRecord(c->e_front, c->stream));
    }
    const int set = chained ? 1 - c->ho_cur : 0;
    const lmpc_ctx::handover &h = c->ho[set];
    // the retry pass of an earlier launch reads the caller's A / Bm / C where the caller gave them, else the hand-over set of ITS launch: such a launch is resolved
    // (a stream drain) before the next step is queued, as it always was -- whichever set that step writes: a caller without arrays of its own drains at every step
    // and gains nothing here (tests/test_gpu_retry.py counts on the pass having run by then)
    for (const auto &pe : c->pending) if (pe.shared_abc) { RESOLVE_PENDING(); break; }
    const k1_also also = {a.A, a.Bm, a.C};
    if (merged && chained) {
        // one queue, kernels only: [solve(i - 1) | K1(i)] of this call lies behind [solve(i - 2) | K1(i - 1)], the last reader of the set K1(i) writes and the writer of
        // the set solve(i - 1) reads.  The regression role reads the lap stores through the held step's parameter block: the chain is unbroken, so they are the ones of now.
        if (c->has_held) { const lmpc_k1_next nx = {B, c->k1_merge_qg, a.xLin, (N + 1) * 6, a.uLin, h.A, h.Bm, h.C, h.rstatus, also}; RCCHK(launch_held(c, &nx)); }
        else { RCCHK(launch_regress(c, B, a.xLin, (N + 1) * 6, a.uLin, h.A, h.Bm, h.C, h.rstatus, c->stream, also)); c->n_k1_alone++; }
        c->n_k1_chained++;
        c->ho_cur = set;
        io.A = h.A; io.Bm = h.Bm; io.C = h.C; io.rstatus = h.rstatus;
        RCCHK(refresh_params(c, false, term, false, false));      // (what launch_solve would do now: the held launch takes the selection of ITS call)
        c->held.io = io; c->held.B = B; c->held.dp = c->dp; c->held.retry_abc = {a.A, a.Bm, a.C}; c->has_held = true;
        c->chain = true;
        return LMPC_OK;
    }
    if (chained) {
        HIPCHK(hipStreamWaitEvent(c->k1_stream, c->e_front, 0));
        RCCHK(launch_regress(c, B, a.xLin, (N + 1) * 6, a.uLin, h.A, h.Bm, h.C, h.rstatus, c->k1_stream, also));
        HIPCHK(hipEventRecord(c->e_k1, c->k1_stream));
        HIPCHK(hipStreamWaitEvent(c->stream, c->e_k1, 0));
        c->n_k1_chained++; c->n_k1_alone++;
    } else {
        RCCHK(launch_regress(c, B, a.xLin, (N + 1) * 6, a.uLin, h.A, h.Bm, h.C, h.rstatus, c->stream, also));
        c->n_k1_unchained++; c->n_k1_alone++;
    }
    c->ho_cur = set;
    io.A = h.A; io.Bm = h.Bm; io.C = h.C; io.rstatus = h.rstatus;
    if (c->e_front) HIPCHK(hipEventRecord(c->e_front, c->stream));      // (no event yet: no step has chained, and the first one that does records its own)
    const k1_also retry_abc = {a.A ? a.A : h.A, a.Bm ? a.Bm : h.Bm, a.C ? a.C : h.C};
    RCCHK(launch_solve(c, B, io, false, {}, false, &retry_abc));
    c->chain = true;
    return LMPC_OK;
}
int lmpc_step_batch_dev(lmpc_ctx *c, int B, const lmpc_step_dev_args *a) { ARGCHK(c && a); return step_dev(c, B, lmpc_step_arrays(*a)); }

int lmpc_step_batch(lmpc_ctx *c, int B, const double *x0, const double *xLin, const double *uLin, const double *uOld, const double *zt,
                    const double *xPredPrev, const int *hasPred, const int *timeStep, double *xPred, double *uPred, double *slack, double *lambda,
                    double *sTerm, double *ztNext, double *ztuNext, double *ssSel, double *qSel, double *mu, double *Aout, double *Bout, double *Cout,
                    int *status, int *iters, double *resid) {
    ARGCHK(c && x0 && xLin && uLin && uOld && xPred && uPred && B >= 1 && B <= c->cfg.max_batch);
    ARGCHK(pred_args_ok(B, xPredPrev, hasPred));
    const bool term = c->cfg.numSS_it > 0;
    if (term) ARGCHK(zt != nullptr);
    RCCHK(ctx_enter(c));
    { k1_table tab; const int rc = k1_table_for(c, B, &tab); if (rc) return rc; }      // (B against the lap table's rows)
    // the caller's arrays by the table's names (a NULL output is not wanted).  Plain MPC: the S = 0 kernels read no zt / xPredPrev / hasPred / timeStep and write no
    // lambda / sTerm / ssSel / qSel.  hasPred counts only with the predictions it speaks of; it and timeStep are zeros when not given.
    lmpc_arrays in = {}, out = {};
    in.x0 = mut(x0); in.xLin = mut(xLin); in.uLin = mut(uLin); in.uOld = mut(uOld);
    if (term) { in.zt = mut(zt); in.xPredPrev = mut(xPredPrev); in.hasPred = mut(xPredPrev ? hasPred : nullptr); in.timeStep = mut(timeStep); }
    out.xPred = xPred; out.uPred = uPred; out.slack = slack; out.mu = mu; out.ztNext = ztNext; out.ztuNext = ztuNext; out.A = Aout; out.Bm = Bout; out.C = Cout;
    out.status = status; out.iters = iters; out.resid = resid; if (term) { out.lambda = lambda; out.sTerm = sTerm; out.ssSel = ssSel; out.qSel = qSel; }
    // Two routes.  A full batch of a small context (the drop-in classes: max_batch = 1) runs on the HOST-MAPPED mirrors of the slabs: the kernels read the inputs from and
    // write the outputs to host memory -- no hipMemcpyAsync in either direction and ONE drain of the stream per call (two copies and two drains were ~25 us of a 0.24 ms
    // LMPC.solve); a few KB cross the host link inside the kernels instead.  Any other call copies array by array to and from the work buffers.
    const bool mapped = c->h_in && B == c->cfg.max_batch;
    const auto tr0 = std::chrono::steady_clock::now();
    lmpc_arrays a = lmpc_step_arrays(mapped ? c->dm : c->w);
    if (mapped) {
        memset(c->hm.hasPred, 0, sizeof(int) * B); memset(c->hm.timeStep, 0, sizeof(int) * B);
        RCCHK(copy_arrays(c, B, c->dims, c->hm, in, hipMemcpyHostToHost));
        // (A, B, C asked for: the regression writes them to the host, the solve reads them back at its start; else they stay on the device)
        if (!Aout && !Bout && !Cout) { a.A = c->w.A; a.Bm = c->w.Bm; a.C = c->w.C; }
    } else {
        RCCHK(copy_arrays(c, B, c->dims, c->w, in, hipMemcpyHostToDevice));
        if (term) RCCHK(zero_absent_flags(c, B, in));
    }
    const auto tr1 = std::chrono::steady_clock::now();
    RCCHK(step_dev(c, B, a));
    c->chain = false;                                    // (this call drains before it returns: its step starts no chain)
    const auto tr2 = std::chrono::steady_clock::now();
    RCCHK(resolve_retries(c));                           // drains the stream; a flagged problem gets its retry pass before anything is copied out
    const auto tr3 = std::chrono::steady_clock::now();
    if (!mapped) {
        out.iters = nullptr;                             // (fetch_iters copies them)
        RCCHK(copy_arrays(c, B, c->dims, out, c->w, hipMemcpyDeviceToHost));
        return fetch_iters(c, B, iters);                 // synchronises the stream
    }
    RCCHK(copy_arrays(c, B, c->dims, out, c->hm, hipMemcpyHostToHost));
    RCCHK(fetch_iters(c, B, nullptr, c->hm.iters));
    const auto tr4 = std::chrono::steady_clock::now();
    c->tr_s[0] += std::chrono::duration<double>(tr1 - tr0).count(); c->tr_s[1] += std::chrono::duration<double>(tr2 - tr1).count();
    c->tr_s[2] += std::chrono::duration<double>(tr3 - tr2).count(); c->tr_s[3] += std::chrono::duration<double>(tr4 - tr3).count(); c->tr_n++;
    return LMPC_OK;
}

int lmpc_qp_dims(lmpc_ctx *c, int *nz, int *m_ineq, int *m_eq) {
    ARGCHK(c);
    const int N = c->cfg.N, S = c->cfg.numSS_it > 0 ? c->cfg.numSS_points : 0;
    const int ns = c->cfg.slacks ? 2 * N : 0;
    if (nz) *nz = 6 * (N + 1) + 2 * N + ns + (S > 0 ? S + 6 : 0);
    if (m_ineq) *m_ineq = 6 * N + ns + S;
    if (m_eq) *m_eq = 6 * (N + 1) + (S > 0 ? 7 : 0);
    return LMPC_OK;
}

int lmpc_assemble_batch(lmpc_ctx *c, int B, const double *A, const double *Bm, const double *C, const double *x0, const double *uOld,
                        const double *ssSel, const double *qSel, double *Pdense, double *q, double *Adense, double *l, double *u) {
    ARGCHK(c && A && Bm && C && x0 && uOld && Pdense && q && Adense && l && u && B >= 1 && B <= c->cfg.max_batch);
    int nz, mi, me; lmpc_qp_dims(c, &nz, &mi, &me); const int mm = mi + me;
    if (c->dims.S > 0) ARGCHK(ssSel && qSel);
    RCCHK(rows_fit(c->tune, B, LMPC_ROWS_EXACT, "problems", "tuning rows"));
    RCCHK(ctx_enter(c)); RESOLVE_PENDING();          // (see lmpc_regress_batch)
    call_temps tmp; double *dP, *dq, *dA, *dl, *du;
    HIPCHK(tmp.alloc(&dP, sizeof(double) * (size_t)B * nz * nz)); HIPCHK(tmp.alloc(&dq, sizeof(double) * (size_t)B * nz));
    HIPCHK(tmp.alloc(&dA, sizeof(double) * (size_t)B * mm * nz)); HIPCHK(tmp.alloc(&dl, sizeof(double) * (size_t)B * mm)); HIPCHK(tmp.alloc(&du, sizeof(double) * (size_t)B * mm));
    RCCHK(upload_qp(c, B, A, Bm, C, x0, uOld, ssSel, qSel));
    // (the matrices of problem b from tuning row b; no rows in force: the image holds the config's own row)
    hipLaunchKernelGGL(lmpc_assemble_kernel, dim3(B), dim3(256), 0, c->stream, c->dp, B, c->w.A, c->w.Bm, c->w.C, c->w.x0, c->w.uOld, c->w.ssSel, c->w.qSel, dP, dq, dA, dl, du,
                       (const double *)c->img[IMG_TUNE].p, c->tune.stride(PAR_TOT));
    HIPCHK(hipGetLastError());
    D2H(Pdense, dP, (size_t)B * nz * nz); D2H(q, dq, (size_t)B * nz); D2H(Adense, dA, (size_t)B * mm * nz); D2H(l, dl, (size_t)B * mm); D2H(u, du, (size_t)B * mm);
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

// ---------------------------------------------------------------------------------------------- controller tuning rows
int lmpc_tuning_set(lmpc_ctx *c, int n, const double *rows) {
    ARGCHK(c && n >= 0 && n <= c->cfg.max_batch && (rows || n == 0));
    char msg[160];
    for (int r = 0; r < n; r++) {
        const double *w = rows + (size_t)r * LMPC_TUNING_NPAR; const char *bad = nullptr;
        for (int i = 0; i < LMPC_TUNING_NPAR && !bad; i++) if (!std::isfinite(w[i])) bad = "a non-finite entry";
        for (int i = 0; i < 6 && !bad; i++) for (int j = 0; j < i; j++) if (w[TN_Q + i * 6 + j] != w[TN_Q + j * 6 + i] || w[TN_QF + i * 6 + j] != w[TN_QF + j * 6 + i]) bad = "Q or Qf not symmetric";
        if (!bad && w[TN_R + 1] != w[TN_R + 2]) bad = "R not symmetric";
        if (!bad && (w[TN_DR] < 0.0 || w[TN_DR + 1] < 0.0)) bad = "a negative dR entry";
        if (!bad && (w[TN_QS] < 0.0 || w[TN_QS + 1] < 0.0)) bad = "a negative Qslack entry";
        if (!bad && c->cfg.numSS_it > 0) for (int i = 0; i < 6; i++) if (!(w[TN_T + i] > 0.0)) bad = "a QtermSlack entry <= 0";
        if (bad) { snprintf(msg, sizeof(msg), "row %d: %s (the rows in force stay)", r, bad); return set_err(LMPC_E_ARG, "lmpc_tuning_set", msg); }
    }
    RCCHK(tuning_upload(c, n, rows));
    c->tune.assign(n, rows);
    return LMPC_OK;
}
int lmpc_tuning_get(lmpc_ctx *c, int *n, double *rows, int capacity) { return rows_get(c, &lmpc_ctx::tune, n, rows, capacity); }

// ---------------------------------------------------------------------------------------------- track rows
int lmpc_track_set(lmpc_ctx *c, int n, const double *rows) {
    ARGCHK(c && n >= 0 && n <= c->cfg.max_batch && (rows || n == 0));
    if (c->ro && c->ro->active) return set_err(LMPC_E_STATE, "lmpc_track_set", "a rollout session is active: a lap on a track that changes under it means nothing (lmpc_rollout_end first)");
    char msg[160];
    for (int r = 0; r < n; r++) {
        const double *w = rows + (size_t)r * LMPC_TRACK_NPAR; const char *bad = nullptr;
        for (int i = 0; i < LMPC_TRACK_NPAR && !bad; i++) if (!std::isfinite(w[i])) bad = "a non-finite entry";
        if (!bad && !(w[0] >= 1.0 && w[0] <= (double)LMPC_MAX_TRACK_ROWS && w[0] == std::floor(w[0]))) bad = "the row count is not an integer in 1..16";
        if (!bad && !(w[1] > 0.0)) bad = "trackLength <= 0";
        for (int i = 0; !bad && i < (int)w[0]; i++) if (w[2 + i * 6 + 4] < 0.0) bad = "a negative segment length";
        if (bad) { snprintf(msg, sizeof(msg), "row %d: %s (the rows in force stay)", r, bad); return set_err(LMPC_E_ARG, "lmpc_track_set", msg); }
    }
    // launches still pending their retry pass read the image of THEIR launch: they are resolved, and the stream is drained, before it is overwritten (as for tuning)
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    if (n > 0) RCCHK(image_upload(&c->img[IMG_TRK], rows, sizeof(double) * LMPC_TRACK_NPAR * (size_t)n, "hipMemcpy (track image)"));
    c->trk.assign(n, rows);
    return LMPC_OK;
}
int lmpc_track_get(lmpc_ctx *c, int *n, double *rows, int capacity) { return rows_get(c, &lmpc_ctx::trk, n, rows, capacity); }

// ---------------------------------------------------------------------------------------------- device buffers
int lmpc_dev_alloc(lmpc_ctx *c, long long bytes, void **dptr) { ARGCHK(c && dptr && bytes > 0); RCCHK(ctx_enter(c)); HIPCHK(hipMalloc(dptr, (size_t)bytes)); return LMPC_OK; }
int lmpc_dev_free(lmpc_ctx *c, void *dptr) { ARGCHK(c); RCCHK(ctx_enter(c)); { int rc = resolve_retries(c); if (rc) return rc; } HIPCHK(hipFree(dptr)); return LMPC_OK; }
int lmpc_dev_upload(lmpc_ctx *c, void *dptr, const void *host, long long bytes) { ARGCHK(c && dptr && host); RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipMemcpyAsync(dptr, host, (size_t)bytes, hipMemcpyHostToDevice, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return LMPC_OK; }
int lmpc_dev_download(lmpc_ctx *c, void *host, const void *dptr, long long bytes) { ARGCHK(c && dptr && host); RCCHK(ctx_enter(c)); { int rc = resolve_retries(c); if (rc) return rc; } HIPCHK(hipMemcpyAsync(host, dptr, (size_t)bytes, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return LMPC_OK; }
int lmpc_debug_k1_ahead(lmpc_ctx *c, long long out[2]) { ARGCHK(c && out); out[0] = c->n_k1_chained; out[1] = c->n_k1_unchained; return LMPC_OK; }
int lmpc_debug_k1_merge(lmpc_ctx *c, long long out[3]) { ARGCHK(c && out); out[0] = c->n_merged; out[1] = c->n_held_flushed; out[2] = c->n_k1_alone; return LMPC_OK; }
int lmpc_dev_flush(lmpc_ctx *c) { ARGCHK(c); return ctx_enter(c); }
int lmpc_dev_sync(lmpc_ctx *c) { ARGCHK(c); RCCHK(ctx_enter(c)); { int rc = resolve_retries(c); if (rc) return rc; } HIPCHK(hipStreamSynchronize(c->stream)); return LMPC_OK; }

// developer trace: host-side seconds of the one-QP path of lmpc_step_batch since the context was made -- out[0..3] = staging the inputs, launching the
// two kernels, waiting for the stream, reading the outputs back; out[4] = calls (tools/dropin_time.py)
int lmpc_debug_step_trace(lmpc_ctx *c, double *out5) { ARGCHK(c && out5); for (int i = 0; i < 4; i++) out5[i] = c->tr_s[i]; out5[4] = (double)c->tr_n; return LMPC_OK; }

// timing build only: one solve of problem 0 of a host batch with cycle stamps (tools/phase_timing.py)
int lmpc_debug_timing(lmpc_ctx *c, const double *A, const double *Bm, const double *C, const double *x0, const double *uOld,
                      const double *ssSel, const double *qSel, long long *tbuf_host, int nt) {
    ARGCHK(c && tbuf_host && nt >= 2);
    RCCHK(ctx_enter(c)); RESOLVE_PENDING();
    RCCHK(upload_qp(c, 1, A, Bm, C, x0, uOld, ssSel, qSel));
    call_temps tmp; long long *dt;
    HIPCHK(tmp.alloc(&dt, sizeof(long long) * nt)); HIPCHK(hipMemsetAsync(dt, 0, sizeof(long long) * nt, c->stream));
    lmpc_solve_io io = solve_io(2, qp_arrays(c));
    io.tbuf = dt; io.abPack = c->ab_pack;      // (long horizons: the route a large batch takes, [A_k | B_k] in global memory; LMPC_NO_ABG=1 for the other)
    RCCHK(launch_solve(c, 1, io));
    HIPCHK(hipMemcpyAsync(tbuf_host, dt, sizeof(long long) * nt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

#ifdef LMPC_TIMING
// (developer build only) phase stamps of work-group 0 of one regression launch: tbuf_host[0..7] = cycle counter at K1STAMP(id)
int lmpc_debug_k1_timing(lmpc_ctx *c, int B, const double *xLin, const double *uLin, long long *tbuf_host) {
    ARGCHK(c && xLin && uLin && tbuf_host && B >= 1 && B <= c->cfg.max_batch);
    const int N = c->cfg.N;
    RCCHK(ctx_enter(c)); RESOLVE_PENDING();
    lmpc_arrays in = {}; in.xLin = mut(xLin); in.uLin = mut(uLin);
    RCCHK(copy_arrays(c, B, c->dims, c->w, in, hipMemcpyHostToDevice));
    // on any way out: the stream is drained, the kernels' stamp pointer is null again, then the buffer goes
    struct stamp_buffer : call_temps { hipStream_t s; ~stamp_buffer() { long long *nul = nullptr; (void)hipStreamSynchronize(s); (void)hipMemcpyToSymbol(HIP_SYMBOL(g_k1_tbuf), &nul, sizeof(nul)); } } tmp;
    tmp.s = c->stream;
    long long *dt; HIPCHK(tmp.alloc(&dt, sizeof(long long) * 24)); HIPCHK(hipMemsetAsync(dt, 0, sizeof(long long) * 24, c->stream));
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_k1_tbuf), &dt, sizeof(dt)));
    for (int rep = 0; rep < 2; rep++) RCCHK(launch_regress(c, B, c->w.xLin, (N + 1) * 6, c->w.uLin, c->w.A, c->w.Bm, c->w.C, c->w.rstatus));
    HIPCHK(hipMemcpyAsync(tbuf_host, dt, sizeof(long long) * 24, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}
#endif

// ---------------------------------------------------------------------------------------------- plant / rollouts
}  // extern "C"
// Per-car vehicle constants (lmpc_plant_set_params).  The rows in force for a call of B cars, one per car: the single row repeated, or the first B of the n rows.
static int plant_rows_for(lmpc_ctx *c, int B, std::vector<double> &rows) {
    RCCHK(rows_fit(c->plant, B, LMPC_ROWS_AT_LEAST, "cars", "plant parameters"));
    rows.resize((size_t)B * LMPC_PLANT_NPAR);
    c->plant.expand(B, rows.data(), c->plant.rows.data(), LMPC_PLANT_NPAR);
    return LMPC_OK;
}
extern "C" {
int lmpc_plant_params_default(double *par) {
    // the literals of Simulator.dynModel, SysModel.py:60-70, in the order the reference lists them
    if (!par) return set_err(LMPC_E_ARG, "argument check failed", "par");
    const double m = 1.98, lf = 0.125, lr = 0.125, Iz = 0.024;
    const double Df = 0.8 * m * 9.81 / 2.0, Cf = 1.25, Bf = 1.0;
    const double Dr = 0.8 * m * 9.81 / 2.0, Cr = 1.25, Br = 1.0;
    const double v[LMPC_PLANT_NPAR] = {m, lf, lr, Iz, Df, Cf, Bf, Dr, Cr, Br};
    memcpy(par, v, sizeof(v));
    return LMPC_OK;
}

int lmpc_plant_set_params(lmpc_ctx *c, int n, const double *par) {
    // the constants of Simulator.dynModel (SysModel.py:60-70) per car; n = 0 returns to the reference's vehicle.  Checked in full before anything is changed.
    ARGCHK(c && n >= 0 && (n == 0 || par) && n <= c->cfg.max_batch);
    for (int b = 0; b < n; b++) {
        const double *q = par + (size_t)b * LMPC_PLANT_NPAR;
        for (int j = 0; j < LMPC_PLANT_NPAR; j++)
            if (!std::isfinite(q[j])) { char msg[96]; snprintf(msg, sizeof(msg), "row %d, entry %d is not finite", b, j); return set_err(LMPC_E_ARG, "plant parameters", msg); }
        if (!(q[0] > 0.0) || !(q[3] > 0.0)) { char msg[96]; snprintf(msg, sizeof(msg), "row %d: m and Iz must be positive", b); return set_err(LMPC_E_ARG, "plant parameters", msg); }
    }
    c->plant.assign(n, par);
    return LMPC_OK;
}

// the rows lmpc_plant_set_params left in force (n = 0: the literals of SysModel.py:60-70, see lmpc_plant_params_default)
int lmpc_plant_get_params(lmpc_ctx *c, int *n, double *par, int capacity) { return rows_get(c, &lmpc_ctx::plant, n, par, capacity); }

// ---- counter-based noise (lmpc_noise.hip.h).  No reference counterpart beyond np.random.randn() at SysModel.py:139-141 and Utilities.py:67-68.
#define NOISE_RANGE_CHK() do { ARGCHK(T >= 1 && B >= 1 && t0 >= 0 && car0 >= 0); ARGCHK(((unsigned long long)T * (unsigned long long)B + LMPC_NOISE_NT - 1) / LMPC_NOISE_NT <= 0x7fffffffull); } while (0)
int lmpc_noise_raw(lmpc_ctx *c, unsigned long long seed, unsigned long long stream, unsigned long long lap, long long t0, int T, long long car0, int B, unsigned long long *words) {
    // the four Philox4x64-10 words of every (t, car) of the range: what numpy.random.Philox(counter=[t, car, lap, stream], key=[seed, 0]).random_raw(4) returns
    ARGCHK(c && words); NOISE_RANGE_CHK();
    RCCHK(ctx_enter(c));
    const size_t total = (size_t)T * (size_t)B;
    unsigned long long *d; { void *q; const int rc = pooled_scratch(c, sizeof(unsigned long long) * total * 4, &q); if (rc) return rc; d = (unsigned long long *)q; }
    hipLaunchKernelGGL(lmpc_noise_raw_kernel, dim3((unsigned)((total + LMPC_NOISE_NT - 1) / LMPC_NOISE_NT)), dim3(LMPC_NOISE_NT), 0, c->stream, seed, stream, lap,
                       (unsigned long long)t0, T, (unsigned long long)car0, B, d);
    HIPCHK(hipGetLastError());
    D2H(words, d, total * 4);
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_noise_fill(lmpc_ctx *c, unsigned long long seed, unsigned long long stream, unsigned long long lap, long long t0, int T, long long car0, int B, int width, double *out) {
    // the N(0, 1) draws of the range, T x B x width, by the kernel that fills a session's buffer (lmpc_rollout_set_noise): same launch, same bits
    ARGCHK(c && out && (width == 2 || width == 3)); NOISE_RANGE_CHK();
    RCCHK(ctx_enter(c));
    const size_t total = (size_t)T * (size_t)B;
    double *d; { void *q; const int rc = pooled_scratch(c, sizeof(double) * total * (size_t)width, &q); if (rc) return rc; d = (double *)q; }
    lmpc_noise_fill_launch(c->stream, seed, stream, lap, t0, T, car0, B, width, d);
    HIPCHK(hipGetLastError());
    D2H(out, d, total * (size_t)width);
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_rollout_set_noise(lmpc_ctx *c, int on, unsigned long long seed, unsigned long long lap, long long car0) {
    // the noise source of the sessions begun after this call (an active session keeps the snapshot it took); needs no device
    ARGCHK(c && car0 >= 0);
    c->noise_on = on ? 1 : 0; c->noise_seed = seed; c->noise_lap = lap; c->noise_car0 = car0;
    return LMPC_OK;
}

int lmpc_rollout_get_noise(lmpc_ctx *c, int *on, unsigned long long *seed, unsigned long long *lap, long long *car0) {
    ARGCHK(c);
    if (on) *on = c->noise_on;
    if (seed) *seed = c->noise_seed;
    if (lap) *lap = c->noise_lap;
    if (car0) *car0 = c->noise_car0;
    return LMPC_OK;
}

int lmpc_plant_step_batch(lmpc_ctx *c, int B, const double *x, const double *xg, const double *u, const double *noise, double *xn, double *xgn, int *status) {
    ARGCHK(c && x && xg && u && noise && xn && xgn && B >= 1);
    RCCHK(ctx_enter(c));
    const bool par = c->plant.in_force();
    std::vector<double> rows;
    if (par) { const int rc = plant_rows_for(c, B, rows); if (rc) return rc; }
    trk_src ts; { const int rc = track_for(c, B, &ts); if (rc) return rc; }      // (car b on track row b)
    double *d; { void *q; const int rc = pooled_scratch(c, sizeof(double) * (size_t)B * (29 + LMPC_PLANT_NPAR) + sizeof(int) * (size_t)B, &q); if (rc) return rc; d = (double *)q; }
    double *dp = d + (size_t)B * 29;
    int *ds = (int *)(d + (size_t)B * (29 + LMPC_PLANT_NPAR));
    double *dx = d, *dg = d + (size_t)B * 6, *du = d + (size_t)B * 12, *dn = d + (size_t)B * 14, *dxn = d + (size_t)B * 17, *dgn = d + (size_t)B * 23;
    H2D(dx, x, (size_t)B * 6); H2D(dg, xg, (size_t)B * 6); H2D(du, u, (size_t)B * 2); H2D(dn, noise, (size_t)B * 3);
    const dim3 grid((B + PLANT_CARS - 1) / PLANT_CARS);
    if (par) {
        H2D(dp, rows.data(), rows.size());                            // (`rows` lives until the stream is drained below)
    }
    const double *kp = par ? dp : nullptr;
    lmpc_pick([&](auto PAR, auto TRK) { hipLaunchKernelGGL((lmpc_plant_kernel<PAR, TRK>), grid, dim3(PLANT_NT), 0, c->stream, c->dp, B, dx, dg, du, dn, dxn, dgn, ds, kp, ts.dev, ts.stride); },
              par, ts.dev != nullptr);
    HIPCHK(hipGetLastError());
    D2H(xn, dxn, (size_t)B * 6); D2H(xgn, dgn, (size_t)B * 6); D2H(status, ds, B);
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_global_position_batch(lmpc_ctx *c, int n, const double *s, const double *ey, double *xy, int *status) {
    ARGCHK(c && s && ey && xy && status && n >= 1);
    RCCHK(ctx_enter(c));
    int rc = refresh_params(c, false, false); if (rc) return rc;
    trk_src ts; rc = track_for(c, n, &ts); if (rc) return rc;         // (point e on track row e)
    double *d; { void *q; const int rc2 = pooled_scratch(c, sizeof(double) * (size_t)n * 4 + sizeof(int) * (size_t)n, &q); if (rc2) return rc2; d = (double *)q; }
    int *ds = (int *)(d + (size_t)n * 4);
    H2D(d, s, (size_t)n); H2D(d + n, ey, (size_t)n);
    hipLaunchKernelGGL(ts.dev ? lmpc_global_position_kernel<true> : lmpc_global_position_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->dp, n,
                       (const double *)d, (const double *)(d + n), d + 2 * (size_t)n, ds, ts.dev, ts.stride);
    HIPCHK(hipGetLastError());
    D2H(xy, d + 2 * (size_t)n, (size_t)n * 2); D2H(status, ds, (size_t)n);
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

// ---- the inverse track map (lmpc_track.hip.h): Map.getLocalPosition, Track.py:191-290, and Map.getAngle, Track.py:312-349, batched.  max_ey is the reference's
// halfWidth + slack (0.85 on its track), which the track table in lmpc_config does not carry.
int lmpc_local_position_batch(lmpc_ctx *c, int n, const double *x, const double *y, const double *psi, double max_ey, double *s, double *ey, double *epsi, int *status) {
    ARGCHK(c && x && y && psi && s && ey && epsi && status && n >= 1 && std::isfinite(max_ey) && max_ey >= 0.0);
    RCCHK(ctx_enter(c));
    int rc = refresh_params(c, false, false); if (rc) return rc;
    trk_src ts; rc = track_for(c, n, &ts); if (rc) return rc;         // (point e on track row e)
    const size_t m = (size_t)n;
    double *d; { void *q; const int rc2 = pooled_scratch(c, sizeof(double) * m * 6 + sizeof(int) * m, &q); if (rc2) return rc2; d = (double *)q; }
    int *ds = (int *)(d + m * 6);
    H2D(d, x, m); H2D(d + m, y, m); H2D(d + 2 * m, psi, m);
    hipLaunchKernelGGL(ts.dev ? lmpc_local_position_kernel<true> : lmpc_local_position_kernel<false>, dim3(lmpc_track_grid(m)), dim3(LMPC_TRACK_NT), 0, c->stream, c->dp, m,
                       (const double *)d, (const double *)(d + m), (const double *)(d + 2 * m), (size_t)1, max_ey, d + 3 * m, d + 4 * m, d + 5 * m, (size_t)1, ds,
                       (const double *)nullptr, (double *)nullptr, ts.dev, ts.stride, (size_t)0);
    HIPCHK(hipGetLastError());
    D2H(s, d + 3 * m, m); D2H(ey, d + 4 * m, m); D2H(epsi, d + 5 * m, m); D2H(status, ds, m);
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_track_angle_batch(lmpc_ctx *c, int n, const double *s, const double *epsi, double *psi, int *status) {
    ARGCHK(c && s && epsi && psi && status && n >= 1);
    RCCHK(ctx_enter(c));
    int rc = refresh_params(c, false, false); if (rc) return rc;
    trk_src ts; rc = track_for(c, n, &ts); if (rc) return rc;         // (point e on track row e)
    const size_t m = (size_t)n;
    double *d; { void *q; const int rc2 = pooled_scratch(c, sizeof(double) * m * 3 + sizeof(int) * m, &q); if (rc2) return rc2; d = (double *)q; }
    int *ds = (int *)(d + m * 3);
    H2D(d, s, m); H2D(d + m, epsi, m);
    hipLaunchKernelGGL(ts.dev ? lmpc_track_angle_kernel<true> : lmpc_track_angle_kernel<false>, dim3(lmpc_track_grid(m)), dim3(LMPC_TRACK_NT), 0, c->stream, c->dp, m,
                       (const double *)d, (const double *)(d + m), d + 2 * m, ds, ts.dev, ts.stride);
    HIPCHK(hipGetLastError());
    D2H(psi, d + 2 * m, m); D2H(status, ds, m);
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_state_from_global_batch(lmpc_ctx *c, int T, int B, const double *xglob, double max_ey, double *x, int *status) {
    // rows of a session log (lmpc_rollout_fetch): x_glob = [vx vy wz psi X Y] -> x = [vx vy wz epsi s ey], one thread per row by the device function of
    // lmpc_local_position_batch.  Rows are independent: s is NOT made continuous across the finish line here (rollout.lap_from_global adds the lap count on the host)
    ARGCHK(c && xglob && x && status && T >= 1 && B >= 1 && std::isfinite(max_ey) && max_ey >= 0.0);
    ARGCHK(((unsigned long long)T * (unsigned long long)B + LMPC_TRACK_NT - 1) / LMPC_TRACK_NT <= 0x7fffffffull);
    RCCHK(ctx_enter(c));
    int rc = refresh_params(c, false, false); if (rc) return rc;
    trk_src ts; rc = track_for(c, B, &ts); if (rc) return rc;         // (car b of the T x B log on track row b)
    const size_t m = (size_t)T * (size_t)B;
    double *d; { void *q; const int rc2 = pooled_scratch(c, sizeof(double) * m * 12 + sizeof(int) * m, &q); if (rc2) return rc2; d = (double *)q; }
    double *dx = d + m * 6; int *ds = (int *)(d + m * 12);
    H2D(d, xglob, m * 6);
    hipLaunchKernelGGL(ts.dev ? lmpc_local_position_kernel<true> : lmpc_local_position_kernel<false>, dim3(lmpc_track_grid(m)), dim3(LMPC_TRACK_NT), 0, c->stream, c->dp, m,
                       (const double *)(d + 4), (const double *)(d + 5), (const double *)(d + 3), (size_t)6, max_ey, dx + 4, dx + 5, dx + 3, (size_t)6, ds, (const double *)d, dx,
                       ts.dev, ts.stride, (size_t)B);
    HIPCHK(hipGetLastError());
    D2H(x, dx, m * 6); D2H(status, ds, m);
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

#define LMPC_PID_MAX_STEPS 100000                             // host bound on the one launch that holds a whole lap (the reference simulates 1000 steps, main.py:57): ~seconds of kernel at most

static void rollout_free(lmpc_ctx *c) {
    if (!c->ro) return;
    for (void *q : c->ro->keep) (void)g_free(q);
    if (c->ro->pstream) { (void)hipStreamDestroy(c->ro->pstream); (void)hipEventDestroy(c->ro->e_solved); (void)hipEventDestroy(c->ro->e_plant); }
    if (c->ro->tstream) { (void)hipStreamDestroy(c->ro->tstream); (void)hipEventDestroy(c->ro->e_trace); }
    delete c->ro; c->ro = nullptr;
}

}  // extern "C"
// Session traces (lmpc_rollout_set_trace): bytes per (step, car) of each plane in the order xPred, uPred, ssSel, qSel, iters, status, xyPred, xySS, mapStatus; 0: not recorded.
#define LMPC_TRACE_PLANES 9
static void trace_plane_bytes(const lmpc_ctx *c, unsigned what, size_t pb[LMPC_TRACE_PLANES]) {
    const size_t N = c->dims.N, S = c->dims.S, d = sizeof(double);
    pb[0] = (what & LMPC_TRACE_XPRED) ? (N + 1) * 6 * d : 0; pb[1] = (what & LMPC_TRACE_UPRED) ? N * 2 * d : 0;
    pb[2] = (what & LMPC_TRACE_SS) ? S * 6 * d : 0; pb[3] = (what & LMPC_TRACE_QSEL) ? S * d : 0;
    pb[4] = pb[5] = (what & LMPC_TRACE_SOLVER) ? sizeof(int) : 0;
    pb[6] = (what & LMPC_TRACE_XY) ? (N + 1) * 2 * d : 0; pb[7] = (what & LMPC_TRACE_XY) ? S * 2 * d : 0; pb[8] = (what & LMPC_TRACE_XY) ? sizeof(int) : 0;
}
// Session set-up shared by lmpc_rollout_begin (kind RO_LMPC), lmpc_rollout_begin_mpc (RO_LTV / RO_LTI) and lmpc_rollout_pid (RO_PID): buffers, initial state, noise.
// xLin0 / uLin0 may be NULL (RO_LTI, RO_PID: no linearisation trajectory; the buffers are zeroed).
static int rollout_setup(lmpc_ctx *c, int kind, int stop_at_line, int B, int T_max, const double *x0, const double *xg0, const double *xLin0, const double *uLin0, const double *noise) {
    RCCHK(ctx_enter(c));
    const size_t S = c->dims.S, Bz = B;
    trk_src trk; { const int rc = track_for(c, B, &trk); if (rc) return rc; }      // (car b on track row b: refused before any session state changes)
    std::vector<double> par_rows;                               // refused before any session state changes (B beyond the per-car rows)
    if (c->plant.in_force()) RCCHK(plant_rows_for(c, B, par_rows));
    // the trace in force (lmpc_rollout_set_trace; a PID session has no predictions and records none): a listed car the session does not have is refused here
    const int tn = kind == RO_PID ? 0 : (int)c->trace_cars.size(); const unsigned tw = tn ? c->trace_what : 0u;
    for (int k = 0; k < tn; k++) if (c->trace_cars[(size_t)k] >= B) {
        char msg[128]; snprintf(msg, sizeof(msg), "traced car %d (entry %d of lmpc_rollout_set_trace) but the session has B = %d cars", c->trace_cars[(size_t)k], k, B);
        return set_err(LMPC_E_ARG, "session trace", msg);
    }
    // the parking in force (lmpc_rollout_set_parking; a PID session is one launch and ignores it): a listed car the session does not have is refused here
    const bool park = kind != RO_PID && (c->park_mode != 0u || !c->park_cars.empty());
    if (park) for (size_t k = 0; k < c->park_cars.size(); k++) if (c->park_cars[k] >= B) {
        char msg[128]; snprintf(msg, sizeof(msg), "parked car %d (entry %d of lmpc_rollout_set_parking) but the session has B = %d cars", c->park_cars[k], (int)k, B);
        return set_err(LMPC_E_ARG, "session parking", msg);
    }
    // SS, QSEL and XY of an LMPC session read the selection outputs the step writes only into the capture buffers: a traced session has them, capture or not
    const bool need_sel = c->dbg_capture != 0 || (tn > 0 && S > 0 && (tw & (LMPC_TRACE_SS | LMPC_TRACE_QSEL | LMPC_TRACE_XY)) != 0);
    std::vector<int> lt_rows; bool lt_small = true;             // sessions that run the regression: the lap table in force, one resolved row per car (refused here as well when B is not its row count)
    if ((kind == RO_LMPC || kind == RO_LTV) && c->lt.in_force()) {
        k1_table tab; RCCHK(k1_table_for(c, B, &tab));
        const std::vector<int> pairs = resolve_lap_rows(c, &lt_small);
        const size_t rowlen = (size_t)c->cfg.trToUse * 2;
        lt_rows.resize((size_t)B * rowlen);
        c->lt.expand(B, lt_rows.data(), pairs.data(), rowlen);
    }
    // A generation loop begins a session of the same shape every lap: its ~35 device buffers (55 MB of logs at 1024 rollouts x 400 steps), the plant stream and
    // the two events are kept from one session to the next (round 5: allocating and freeing them was ~5 ms of every generation) and released by
    // lmpc_destroy or by a session of another shape.
    if (c->ro && !c->ro->active && c->ro->B == B && c->ro->T_max == T_max && (c->ro->a.ssSel != nullptr) == need_sel && c->ro->tr_n == tn && c->ro->tr_what == tw) {
        lmpc_rollout_session *r = c->ro; r->t = 0; r->active = true; r->kind = kind; r->stop_at_line = stop_at_line;
        goto init_state;
    }
    rollout_free(c);
    {
    lmpc_rollout_session *r = new lmpc_rollout_session(); c->ro = r; r->B = B; r->T_max = T_max; r->t = 0; r->pstream = nullptr; r->active = true; r->kind = kind; r->stop_at_line = stop_at_line;
    r->tr_n = tn; r->tr_what = tw; r->tstream = nullptr; r->d_live = nullptr;
    if (tn) { HIPCHK(hipStreamCreate(&r->tstream)); HIPCHK(hipEventCreateWithFlags(&r->e_trace, hipEventDisableTiming)); }
    HIPCHK(hipStreamCreate(&r->pstream)); HIPCHK(hipEventCreateWithFlags(&r->e_solved, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&r->e_plant, hipEventDisableTiming));
    bool ok = true;
    auto dalloc = [&](size_t bytes) -> void * { void *q = nullptr; if (g_malloc(&q, std::max<size_t>(bytes, 8)) != hipSuccess) { ok = false; return nullptr; } r->keep.push_back(q); return q; };
#define DA(type, name, n) r->name = (type *)dalloc(sizeof(type) * (size_t)(n));
    lmpc_arrays_each(c->dims, [&](const char *, auto m, size_t elem, size_t n, int role) {
        typedef lmpc_arrays A;
        // (mu, ztUsed, selStart: no session asks for them; ssSel, qSel and the selection's successors: capture buffers, listed below)
        const bool shared = role == LMPC_ARR_SEL ? lmpc_is(m, &A::rstatus) : !lmpc_is(m, &A::ssSel) && !lmpc_is(m, &A::qSel) && !lmpc_is(m, &A::mu);
        if (shared)
            r->a.*m = (std::remove_reference_t<decltype(r->a.*m)>)dalloc(elem * n * Bz);
    });
    DA(double, d_xg, Bz * 6) DA(int, d_done, Bz) DA(int, d_nDone, 4) DA(int, d_stAcc, Bz) DA(double, d_finX, Bz * 6) DA(double, d_finG, Bz * 6)
    DA(double, d_par, Bz * LMPC_PLANT_NPAR) DA(int, d_lt, Bz * (size_t)std::max(c->cfg.trToUse, 1) * 2)
    if (need_sel) { DA(double, a.ssSel, Bz * S * 6) DA(double, a.qSel, Bz * S) DA(double, a.succ, Bz * S * 6) DA(double, a.succU, Bz * S * 2) }
    DA(double, d_logX, (size_t)T_max * Bz * 6) DA(double, d_logU, (size_t)T_max * Bz * 2) DA(double, d_logG, (size_t)T_max * Bz * 6) DA(double, d_noise, (size_t)T_max * Bz * 3)
    if (tn) {                                                   // only the planes asked for (trace_plane_bytes: bytes per step and car)
        size_t pb[LMPC_TRACE_PLANES]; trace_plane_bytes(c, tw, pb);
        const size_t rows = (size_t)T_max * (size_t)tn;
        DA(int, d_trCars, tn)
        void **pl[LMPC_TRACE_PLANES] = {(void **)&r->tr_x, (void **)&r->tr_u, (void **)&r->tr_ss, (void **)&r->tr_q, (void **)&r->tr_it, (void **)&r->tr_st, (void **)&r->tr_xy, (void **)&r->tr_xys, (void **)&r->tr_map};
        for (int i = 0; i < LMPC_TRACE_PLANES; i++) *pl[i] = pb[i] ? dalloc(rows * pb[i]) : nullptr;
    }
    r->d_noiseU = nullptr; r->d_vt = nullptr;                   // (allocated by the first lmpc_rollout_pid on the session's buffers, kept with them)
#undef DA
    if (!ok) { rollout_free(c); return set_err(LMPC_E_HIP, "hipMalloc", "rollout buffers"); }
    }
init_state:
    lmpc_rollout_session *r = c->ro;
    std::vector<double> ztv((size_t)B * 6, 0.0);
    for (int b = 0; b < B; b++) ztv[(size_t)b * 6 + 4] = 10.0;                                   // LMPC.__init__ :330
    std::vector<int> neg((size_t)B, -1);
    // the step's arrays: the initial state, zt and (if given) the first linearisation trajectories are uploaded, every other one is zeroed -- a reused session is
    // indistinguishable from a fresh one: what the previous lap left in the solver's outputs and status words goes too
    lmpc_arrays first = {}; first.x0 = mut(x0); first.zt = ztv.data(); first.xLin = mut(xLin0); first.uLin = mut(uLin0);
    RCCHK(copy_arrays(c, Bz, c->dims, r->a, first, hipMemcpyHostToDevice));
    {
        hipError_t e = hipSuccess;
        lmpc_arrays_each(c->dims, [&](const char *, auto m, size_t elem, size_t n, int) {
            if (r->a.*m && !(first.*m) && e == hipSuccess) e = hipMemsetAsync(r->a.*m, 0, elem * n * Bz, c->stream); });
        HIPCHK(e);
    }
    H2D(r->d_xg, xg0, Bz * 6); H2D(r->d_done, neg.data(), Bz);
    // the snapshot of the noise source: lmpc_rollout_set_noise during the session reaches the next one only.  noise == NULL (the callers have checked that the source
    // is on): the buffer the plant kernels read is written by one launch on the context's stream, in front of the first step -- no host draw, no upload
    r->nz_seed = c->noise_seed; r->nz_lap = c->noise_lap; r->nz_car0 = c->noise_car0;
    if (noise) H2D(r->d_noise, noise, (size_t)T_max * Bz * 3);
    else { lmpc_noise_fill_launch(c->stream, r->nz_seed, 0ull, r->nz_lap, 0, T_max, r->nz_car0, B, 3, r->d_noise); HIPCHK(hipGetLastError()); }
    r->nz_dev = noise == nullptr; r->relaunched = false; r->lapStart.clear(); r->lapNo.clear();      // (every car's first lap begins at row 0; the books exist from the first lmpc_rollout_relaunch on)
    r->trk = trk.dev; r->trk_stride = trk.stride;
    if (r->tr_n) { const char *e = dev_knob("LMPC_TRACE_OWN_STREAM"); r->tr_own_stream = e && atoi(e) != 0; }
    r->has_par = !par_rows.empty();                             // the snapshot: lmpc_plant_set_params during the session reaches the next one only
    if (r->has_par) H2D(r->d_par, par_rows.data(), par_rows.size());
    r->has_lt = !lt_rows.empty(); r->lt_small = lt_small; r->lt_stride = 2 * c->cfg.trToUse;   // the snapshot: lmpc_model_set_lap_table during the session reaches the next one only
    if (r->has_lt) H2D(r->d_lt, lt_rows.data(), lt_rows.size());
    r->lt_host = lt_rows;                                       // (read by lmpc_rollout_relaunch, which replaces single rows)
    if (r->tr_n) {                                           // the car list may differ from the kept session's; mapStatus is ORed into, so it starts at zero
        H2D(r->d_trCars, c->trace_cars.data(), (size_t)r->tr_n);
        if (r->tr_map) HIPCHK(hipMemsetAsync(r->tr_map, 0, sizeof(int) * (size_t)T_max * (size_t)r->tr_n, c->stream));
    }
    HIPCHK(hipMemsetAsync(r->d_nDone, 0, sizeof(int) * 4, c->stream)); HIPCHK(hipMemsetAsync(r->d_stAcc, 0, sizeof(int) * Bz, c->stream));
    HIPCHK(hipMemsetAsync(r->d_finX, 0, sizeof(double) * Bz * 6, c->stream)); HIPCHK(hipMemsetAsync(r->d_finG, 0, sizeof(double) * Bz * 6, c->stream));
    // the snapshot of the parking: lmpc_rollout_set_parking during the session reaches the next one only.  The first live list -- every car but the start list -- is
    // built by the session's compaction kernel behind the uploads above; its length comes back before the drain that ends the set-up anyway
    r->parked = park; r->pk_mode = 0u; r->pk_n0 = 0; r->nLive = B; r->nd_host = 0;
    std::vector<int> flags; int hdr[2] = {0, B};
    if (park) {
        r->pk_mode = c->park_mode & (stop_at_line ? ~0u : ~(unsigned)LMPC_PARK_FINISHED);      // (a session that logs its cars past the crossing parks the start list only)
        r->pk_n0 = (int)c->park_cars.size();
        if (!r->d_live) {                   // beside the kept set, as the PID noise is: sessions of the same shape reuse the buffers whatever their parking
            void *q = nullptr;
            if (g_malloc(&q, sizeof(int) * 3 * Bz) != hipSuccess) { r->active = false; return set_err(LMPC_E_HIP, "hipMalloc", "live list"); }
            r->keep.push_back(q); r->d_live = (int *)q; r->d_parkedAt = r->d_live + Bz; r->d_park0 = r->d_parkedAt + Bz;
        }
        flags.assign(Bz, 0); for (int car : c->park_cars) flags[(size_t)car] = 1;
        H2D(r->d_park0, flags.data(), Bz);
        HIPCHK(hipMemsetAsync(r->d_parkedAt, 0xff, sizeof(int) * Bz, c->stream));              // -1: live
        const lmpc_live_args la = {B, 0, r->pk_mode, 1, r->d_done, r->d_park0, r->d_parkedAt, r->d_live, r->d_nDone};
        hipLaunchKernelGGL(lmpc_rollout_live_kernel, dim3(1), dim3(LMPC_LIVE_NT), 0, c->stream, la);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hdr, r->d_nDone, sizeof(hdr), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (park) r->nLive = hdr[1];
    return LMPC_OK;
}
static void rollout_state(lmpc_rollout_session *r, lmpc_rollout_state &st) {
    const lmpc_arrays &a = r->a; st.x = a.x0; st.xg = r->d_xg; st.xLin = a.xLin; st.uLin = a.uLin; st.uOld = a.uOld; st.zt = a.zt; st.xPP = a.xPredPrev;
    st.hasPred = a.hasPred; st.timeStep = a.timeStep; st.doneAt = r->d_done; st.xPred = a.xPred; st.uPred = a.uPred; st.ztNext = a.ztNext; st.ztuNext = a.ztuNext;
    st.status = a.status; st.logX = r->d_logX; st.logU = r->d_logU; st.logG = r->d_logG; st.noise = r->d_noise; st.nDone = r->d_nDone; st.statusAcc = r->d_stAcc;
    st.finX = r->d_finX; st.finG = r->d_finG; st.plantPar = r->d_par; st.trk = r->trk; st.trkStride = r->trk_stride;
}
extern "C" {
int lmpc_rollout_begin(lmpc_ctx *c, int B, int T_max, const double *x0, const double *xg0, const double *xLin0, const double *uLin0, const double *noise) {
    // B closed-loop LMPC laps, state resident on the device.  xLin0 / uLin0: per-rollout first linearisation trajectories
    // (B x (N+1) x 6, B x N x 2) -- LMPC.addTrajectory :431-433.  noise: T_max x B x 3 N(0,1) draws.
    // noise == NULL with lmpc_rollout_set_noise on: the draws are generated on the device (steps 0 .. T_max - 1, cars car0 .. car0 + B - 1, stream 0).
    ARGCHK(c && x0 && xg0 && xLin0 && uLin0 && B >= 1 && T_max >= 1 && c->cfg.numSS_it > 0);
    ARGCHK(noise || c->noise_on);                                                           // (no array and no device source)
    return rollout_setup(c, RO_LMPC, 1, B, T_max, x0, xg0, xLin0, uLin0, noise);
}

int lmpc_rollout_begin_mpc(lmpc_ctx *c, int B, int T_max, const double *x0, const double *xg0, const double *xLin0, const double *uLin0,
                           const double *A_lti, const double *B_lti, const double *noise, int stop_at_line) {
    // B closed-loop laps of the plain MPC (numSS_it == 0: no terminal set), main.py:72-95.  A_lti / B_lti given (B x 6 x 6, B x 6 x 2): the LTI path-following MPC
    // on the model of Utilities.Regression -- every stage of rollout b uses A_b, B_b and C = 0 (MPC.buildEqConstr, PredictiveControllers.py:216-218), expanded here
    // once; xLin0 / uLin0 are not used.  Both NULL: the LTV-MPC (timeVarying, :110-145) on the regression store, first linearisation trajectories xLin0 / uLin0.
    ARGCHK(c && x0 && xg0 && B >= 1 && T_max >= 1 && c->cfg.numSS_it == 0);
    ARGCHK(noise || c->noise_on);                                                           // (no array and no device source: lmpc_rollout_set_noise)
    ARGCHK((A_lti != nullptr) == (B_lti != nullptr) && (A_lti || (xLin0 && uLin0)));
    ARGCHK(B <= c->cfg.max_batch);
    ARGCHK(!(c->ro && c->ro->active));                                                      // (a session is already active: end it first)
    RCCHK(ctx_enter(c));
    const bool lti = A_lti != nullptr;
    if (!lti) { const int rc = refresh_params(c, true, false, c->lt.in_force()); if (rc) return rc; }       // LMPC_E_STATE without trToUse stored laps, as lmpc_step_batch
    RESOLVE_PENDING();
    int rc = rollout_setup(c, lti ? RO_LTI : RO_LTV, stop_at_line ? 1 : 0, B, T_max, x0, xg0, lti ? nullptr : xLin0, lti ? nullptr : uLin0, noise);
    if (rc) return rc;
    if (lti) {
        lmpc_rollout_session *r = c->ro; const size_t N = c->cfg.N, Bz = B;
        std::vector<double> eA(Bz * N * 36), eB(Bz * N * 12);
        for (size_t b = 0; b < Bz; b++) for (size_t k = 0; k < N; k++) {
            memcpy(&eA[(b * N + k) * 36], A_lti + b * 36, sizeof(double) * 36); memcpy(&eB[(b * N + k) * 12], B_lti + b * 12, sizeof(double) * 12);
        }
        hipError_t e = hipMemcpyAsync(r->a.A, eA.data(), sizeof(double) * eA.size(), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(r->a.Bm, eB.data(), sizeof(double) * eB.size(), hipMemcpyHostToDevice, c->stream);   // (C = 0: rollout_setup has zeroed it)
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);                      // (the pageable host arrays must outlive the copies)
        if (e != hipSuccess) { r->active = false; return set_err(LMPC_E_HIP, "lmpc_rollout_begin_mpc", hipGetErrorString(e)); }
    }
    return LMPC_OK;
}

int lmpc_rollout_pid(lmpc_ctx *c, int B, int T_max, const double *x0, const double *xg0, const double *vt, const double *noise_u, const double *noise,
                     int stop_at_line, int *steps_total, int *n_done) {
    // B PID laps (main.py:61-70: Simulator.sim with Utilities.PID, Utilities.py:42-68), the whole lap in ONE launch (lmpc_pid_rollout_kernel).  vt: target speed per
    // car (B); noise_u: T_max x B x 2 N(0,1) draws of the control law; noise: T_max x B x 3 of the plant.  Needs only the track: valid on any context.  Leaves an
    // active session whose logs lmpc_rollout_fetch returns; lmpc_rollout_run has nothing left to do on it.  steps_total: rows the logs hold (T_max, or with
    // stop_at_line the last crossing step if every car crossed).
    // noise / noise_u == NULL with lmpc_rollout_set_noise on: generated on the device, stream 0 into the plant's buffer and stream 1 into the control law's.
    ARGCHK(c && x0 && xg0 && vt && B >= 1 && T_max >= 1 && T_max <= LMPC_PID_MAX_STEPS);
    ARGCHK((noise_u && noise) || c->noise_on);                                              // (an array missing and no device source: lmpc_rollout_set_noise)
    ARGCHK(B <= c->cfg.max_batch);
    ARGCHK(!(c->ro && c->ro->active));                                                      // (a session is already active: end it first)
    RCCHK(ctx_enter(c));
    RESOLVE_PENDING();
    int rc = rollout_setup(c, RO_PID, stop_at_line ? 1 : 0, B, T_max, x0, xg0, nullptr, nullptr, noise);
    if (rc) return rc;
    lmpc_rollout_session *r = c->ro; const size_t Bz = B;
    auto fail = [&](int code) { r->active = false; return code; };
    if (!r->d_noiseU) {                     // beside the kept set: sessions of the same shape reuse the buffers whatever their kind
        void *q = nullptr;
        if (g_malloc(&q, sizeof(double) * ((size_t)T_max * Bz * 2 + Bz)) != hipSuccess) return fail(set_err(LMPC_E_HIP, "hipMalloc", "control-law noise"));
        r->keep.push_back(q); r->d_noiseU = (double *)q; r->d_vt = r->d_noiseU + (size_t)T_max * Bz * 2;
    }
    hipError_t e = hipSuccess;
    if (noise_u) e = hipMemcpyAsync(r->d_noiseU, noise_u, sizeof(double) * (size_t)T_max * Bz * 2, hipMemcpyHostToDevice, c->stream);
    else { lmpc_noise_fill_launch(c->stream, r->nz_seed, 1ull, r->nz_lap, 0, T_max, r->nz_car0, B, 2, r->d_noiseU); e = hipGetLastError(); }   // (the session's snapshot, as d_noise)
    if (e == hipSuccess) e = hipMemcpyAsync(r->d_vt, vt, sizeof(double) * Bz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && stop_at_line) {      // rows behind a car's crossing step are not written: a reused session must not show the previous lap's there
        e = hipMemsetAsync(r->d_logX, 0, sizeof(double) * (size_t)T_max * Bz * 6, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(r->d_logU, 0, sizeof(double) * (size_t)T_max * Bz * 2, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(r->d_logG, 0, sizeof(double) * (size_t)T_max * Bz * 6, c->stream);
    }
    if (e != hipSuccess) return fail(set_err(LMPC_E_HIP, "lmpc_rollout_pid", hipGetErrorString(e)));
    lmpc_rollout_state st; rollout_state(r, st);
    const dim3 grid((B + PLANT_CARS - 1) / PLANT_CARS);
    lmpc_pick([&](auto PAR, auto TRK) {
        hipLaunchKernelGGL((lmpc_pid_rollout_kernel<PAR, TRK>), grid, dim3(PLANT_NT), 0, c->stream, c->dp, B, T_max, stop_at_line ? 1 : 0, (const double *)r->d_vt, (const double *)r->d_noiseU, st);
    }, r->has_par, r->trk != nullptr);
    e = hipGetLastError();
    std::vector<int> done(Bz);
    if (e == hipSuccess) e = hipMemcpyAsync(done.data(), r->d_done, sizeof(int) * Bz, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(set_err(LMPC_E_HIP, "lmpc_rollout_pid", hipGetErrorString(e)));
    int nd = 0, last = 0;
    for (int b = 0; b < B; b++) if (done[b] >= 0) { nd++; last = std::max(last, done[b]); }
    r->t = (stop_at_line && nd == B) ? last : T_max;
    if (steps_total) *steps_total = r->t;
    if (n_done) *n_done = nd;
    return LMPC_OK;
}

// The launches of a session step over the live list ll.  ll.car == nullptr: a session without parking -- the grids cover ll.n = B cars, the kernels are the ones without a list
static void launch_rollout_plant(lmpc_ctx *c, lmpc_rollout_session *r, const lmpc_rollout_state &st, lmpc_live_list ll) {
    const dim3 grid((ll.n + PLANT_CARS - 1) / PLANT_CARS);
    lmpc_pick([&](auto PAR, auto TRK, auto LIVE) {
        constexpr bool par = PAR, trk = TRK;
        auto go = [&](auto... lv) { hipLaunchKernelGGL((lmpc_rollout_plant_kernel<par, trk, decltype(lv)...>), grid, dim3(PLANT_NT), 0, r->pstream, c->dp, r->B, r->t, st, lv...); };
        if constexpr (LIVE) go(ll); else go();
    }, r->has_par, r->trk != nullptr, ll.car != nullptr);
}
static void launch_rollout_trace(lmpc_ctx *c, lmpc_rollout_session *r, hipStream_t on, lmpc_live_list ll) {      // (a parking session hands in parkedAt: a parked car's planes keep what they held)
    lmpc_trace_args ta = {r->d_trCars, r->tr_n, c->cfg.N, (int)c->dims.S, r->a.xPred, r->a.uPred, r->a.ssSel, r->a.qSel, r->a.iters, r->a.status,
                          r->tr_x, r->tr_u, r->tr_ss, r->tr_q, r->tr_xy, r->tr_xys, r->tr_it, r->tr_st, r->tr_map, r->trk, r->trk_stride};
    lmpc_pick([&](auto TRK, auto PARKED) {
        constexpr bool trk = TRK;
        auto go = [&](auto... at) { hipLaunchKernelGGL((lmpc_rollout_trace_kernel<trk, decltype(at)...>), dim3(r->tr_n), dim3(LMPC_TRACE_NT), 0, on, c->dp, r->t, ta, at...); };
        if constexpr (PARKED) go((const int *)r->d_parkedAt); else go();
    }, r->trk != nullptr, ll.car != nullptr);
}
// (the shift and old-input kernels keep a parking twin each: DESIGN.md, "Shipped kernels keep their machine code")
static void launch_rollout_shift(lmpc_ctx *c, lmpc_rollout_session *r, const lmpc_rollout_state &st, lmpc_live_list ll) {
    const dim3 grid((ll.n * LMPC_SHIFT_TPR(c->cfg.N) + 255) / 256);
    if (ll.car) hipLaunchKernelGGL(lmpc_rollout_shift_live_kernel, grid, dim3(256), 0, c->stream, c->dp, r->t, st, ll);
    else if (r->relaunched) hipLaunchKernelGGL(lmpc_rollout_shift_lap_kernel, grid, dim3(256), 0, c->stream, c->dp, r->B, r->t, st, (const int *)r->d_lapStart);      // (timeStep counts the steps of each car's lap; a parking session never relaunches)
    else hipLaunchKernelGGL(lmpc_rollout_shift_kernel, grid, dim3(256), 0, c->stream, c->dp, r->B, r->t, st);
}
static void launch_rollout_oldinput(lmpc_ctx *c, lmpc_rollout_session *r, lmpc_live_list ll) {
    const dim3 grid((ll.n * 2 + 255) / 256);
    if (ll.car) hipLaunchKernelGGL(lmpc_rollout_oldinput_live_kernel, grid, dim3(256), 0, c->stream, c->cfg.N, (const double *)r->a.uPred, r->a.uOld, ll);
    else hipLaunchKernelGGL(lmpc_rollout_oldinput_kernel, grid, dim3(256), 0, c->stream, r->B, c->cfg.N, (const double *)r->a.uPred, r->a.uOld);
}

int lmpc_rollout_run(lmpc_ctx *c, int max_steps, int *steps_total, int *n_done) {
    // advance every rollout by up to max_steps simulated steps (four launches per step on two streams, no host round trip except a
    // finished-lap poll every 8 steps); stops early once every rollout has crossed the finish line
    // Sessions of lmpc_rollout_begin_mpc run the same chain without the safe-set selection (io.mode 2: the S = 0 solve kernels write ztNext = xPred[N],
    // ztuNext = uPred[N - 1], MPC.feasibleStateInput :157-159, which the shift kernel appends to xLin / uLin); the LTI form has no regression launch and no
    // linearisation trajectory to shift, only OldInput.  A session of lmpc_rollout_pid has run to its end already.
    ARGCHK(c && c->ro && c->ro->active && max_steps >= 1 && c->ro->kind != RO_PID);
    lmpc_rollout_session *r = c->ro;
    const int B = r->B; const size_t N = c->cfg.N;
    const bool lmpc = r->kind == RO_LMPC, lti = r->kind == RO_LTI;
    RCCHK(ctx_enter(c));
    lmpc_rollout_state st; rollout_state(r, st);
    int nd = 0, rc = LMPC_OK;
    const int t_end = std::min(r->T_max, r->t + max_steps);
    // Parking (lmpc_rollout_set_parking): every launch of a step covers the nL entries of the live list instead of the B cars; the list is rebuilt at the
    // finished-lap poll below.  No live car: nothing to step
    const bool park = r->parked, reroute = park && (r->pk_mode & LMPC_PARK_REROUTE) != 0;
    if (park && r->nLive == 0) { if (steps_total) *steps_total = r->t; if (n_done) *n_done = r->nd_host; return LMPC_OK; }
    if (park) nd = r->nd_host;
    if (park && !lti && !r->has_lt) {
        // the regression kernel reads the live list in its table builds: a session without a lap table hands them the block's own laps as ONE row for every car
        rc = refresh_params(c, true, lmpc, false, false); if (rc) return rc;
        std::vector<int> row((size_t)c->cfg.trToUse * 2); bool small = true;
        for (int i = 0; i < c->cfg.trToUse; i++) { row[(size_t)2 * i] = c->dp.mslot[i]; row[(size_t)2 * i + 1] = c->dp.mlen[i]; small = small && c->dp.mlen[i] - 1 <= 8 * WAVE; }
        HIPCHK(hipMemcpyAsync(r->d_lt, row.data(), sizeof(int) * row.size(), hipMemcpyHostToDevice, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
        r->lt_small = small;
    }
    lmpc_live_list ll = {park ? r->d_live : nullptr, r->nLive};      // (a session without parking: nLive = B)
    while (r->t < t_end) {
        lmpc_solve_io io = solve_io(lmpc ? 3 : 2, r->a);
        // the safe-set lap table is live in a session (as lmpc_ss_set_selected is): B against its rows before the first launch of the step
        if (lmpc) { rc = ss_table_for(c, B, &io); if (rc) return rc; }
        rc = tuning_for(c, B, &io); if (rc) return rc;       // (the tuning rows are live in the same way: a lmpc_tuning_set between two runs reaches the next step)
        if (!lti) {
        rc = refresh_params(c, true, lmpc, r->has_lt, io.ssTab != nullptr); if (rc) return rc;      // (what this session's launch reads: its snapshot, or -- begun without a table -- the block, whatever table the context has been given since)
        ev_begin(c, 0, c->stream);
        { int qg, nblk; k1_grid(c, ll.n, &qg, &nblk);
          const k1_table tab = {(r->has_lt || ll.car) ? r->d_lt : nullptr, r->has_lt ? r->lt_stride : 0, r->lt_small, r->trk, r->trk_stride, ll};
          launch_k1(c, nblk, ll.n, qg, (const double *)r->a.xLin, (int)(N + 1) * 6, (const double *)r->a.uLin, r->a.A, r->a.Bm, r->a.C, r->a.rstatus, tab); }
        ev_end(c, c->stream); c->stats.n_regress++;
        }
        io.rstatus = lti ? nullptr : r->a.rstatus;
        if (r->t > 0) HIPCHK(hipStreamWaitEvent(c->stream, r->e_plant, 0));          // the solve needs the plant's new state
        if (r->t > 0 && r->tr_n && r->tr_own_stream) HIPCHK(hipStreamWaitEvent(c->stream, r->e_trace, 0));   // (traced sessions: and must not overwrite outputs the trace kernel of the last step still reads)
        rc = launch_solve(c, B, io, true, ll, reroute); if (rc) return rc;      // (the plant consumes uPred without a host round trip: unconditional retry pass)
        HIPCHK(hipEventRecord(r->e_solved, c->stream));
        HIPCHK(hipStreamWaitEvent(r->pstream, r->e_solved, 0));
        // the trace of this step: behind the plant kernel on the plant stream, in front of e_plant -- off the solve -> shift -> regression chain of the context's
        // stream, and the one event the next solve waits for anyway covers it.  (LMPC_TRACE_OWN_STREAM=1: on a stream of its own beside the plant, with an event of its
        // own for the next solve -- measured slower, DESIGN.md "Session traces")
        if (r->tr_n && r->tr_own_stream) {
            HIPCHK(hipStreamWaitEvent(r->tstream, r->e_solved, 0));
            launch_rollout_trace(c, r, r->tstream, ll);
            HIPCHK(hipEventRecord(r->e_trace, r->tstream));
        }
        launch_rollout_plant(c, r, st, ll);
        if (r->tr_n && !r->tr_own_stream) launch_rollout_trace(c, r, r->pstream, ll);
        HIPCHK(hipEventRecord(r->e_plant, r->pstream));
        if (lti) launch_rollout_oldinput(c, r, ll); else launch_rollout_shift(c, r, st, ll);      // then the next step's regression
        HIPCHK(hipGetLastError());
        r->t++;
        if ((r->t & 7) == 0 || r->t == t_end) {
            HIPCHK(hipStreamSynchronize(r->pstream));
            if (r->tr_n) HIPCHK(hipStreamSynchronize(r->tstream));
            // Parking: the plant stream is idle, so doneAt and nDone stand; the compaction kernel (which returns at once unless nDone has moved since the last rebuild)
            // goes behind the shift on the context's stream, and nLive comes back in the copy that brings nDone: no drain of its own
            if (park && (r->pk_mode & LMPC_PARK_FINISHED)) {
                const lmpc_live_args la = {B, r->t, r->pk_mode, 0, r->d_done, r->d_park0, r->d_parkedAt, r->d_live, r->d_nDone};
                hipLaunchKernelGGL(lmpc_rollout_live_kernel, dim3(1), dim3(LMPC_LIVE_NT), 0, c->stream, la);
                HIPCHK(hipGetLastError());
            }
            int hd[2] = {0, 0};                                        // nDone, nLive (the second: parking sessions only)
            HIPCHK(hipMemcpyAsync(hd, r->d_nDone, sizeof(hd), hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
            nd = hd[0]; r->nd_host = nd;
            if (park) ll.n = r->nLive = hd[1];
            if (r->nLive == 0 || (r->stop_at_line && nd >= B - r->pk_n0)) break;      // (with a start list only: every car not on it has crossed; pk_n0 = 0 without parking)
        }
    }
    if (steps_total) *steps_total = r->t;
    if (n_done) *n_done = nd;
    return LMPC_OK;
}

int lmpc_rollout_relaunch(lmpc_ctx *c, int n, const int *cars, int lap_rows) {
    // The lap change of the listed cars inside the running session (lmpc_relaunch.hip.h): each is put, on the device, into the state a fresh lmpc_rollout_begin would
    // give it for its next lap -- main.py:100-121 runs one car, whose next lap begins at the step after its crossing, from xF (SysModel.py:50).  Everything is
    // checked before anything changes; then one upload of the entry table (with the cars' new lap-table rows), one launch, one drain.
    if (!c) return set_err(LMPC_E_ARG, "lmpc_rollout_relaunch", "null context");
    if (!(c->ro && c->ro->active)) return set_err(LMPC_E_STATE, "lmpc_rollout_relaunch", "no rollout session is active");
    lmpc_rollout_session *r = c->ro; const int B = r->B, N = c->cfg.N;
    if (r->kind != RO_LMPC) return set_err(LMPC_E_STATE, "lmpc_rollout_relaunch", "only a session of lmpc_rollout_begin changes laps (this one is of lmpc_rollout_begin_mpc or lmpc_rollout_pid)");
    if (r->parked) return set_err(LMPC_E_STATE, "lmpc_rollout_relaunch", "the session was begun with parking in force (lmpc_rollout_set_parking)");
    if (r->tr_n) return set_err(LMPC_E_STATE, "lmpc_rollout_relaunch", "the session was begun with a trace in force (lmpc_rollout_set_trace)");
    char msg[192];
    if (n < 1 || !cars) return set_err(LMPC_E_ARG, "lmpc_rollout_relaunch", "n < 1 or no car list");
    if (lap_rows < 1) { snprintf(msg, sizeof(msg), "lap_rows = %d: at least one row of noise per lap expected", lap_rows); return set_err(LMPC_E_ARG, "lmpc_rollout_relaunch", msg); }
    std::vector<char> seen((size_t)B, 0);
    for (int i = 0; i < n; i++) {
        if (cars[i] < 0 || cars[i] >= B) { snprintf(msg, sizeof(msg), "entry %d: car %d, the session has B = %d cars", i, cars[i], B); return set_err(LMPC_E_ARG, "lmpc_rollout_relaunch", msg); }
        if (seen[(size_t)cars[i]]) { snprintf(msg, sizeof(msg), "car %d is listed twice", cars[i]); return set_err(LMPC_E_ARG, "lmpc_rollout_relaunch", msg); }
        seen[(size_t)cars[i]] = 1;
    }
    const bool lt = r->has_lt && c->lt.in_force();                    // (a session begun without a table has no row to replace; with none in force now the cars keep their rows)
    if (lt) RCCHK(rows_fit(c->lt, B, LMPC_ROWS_EXACT, "cars", "lmpc_rollout_relaunch"));
    size_t n_spans = 0;
    lmpc_arrays_each(c->dims, [&](const char *, auto m, size_t, size_t cnt, int) { if (r->a.*m && cnt) n_spans++; });
    if (n_spans > LMPC_RELAUNCH_MAX_SPANS) return set_err(LMPC_E_ARG, "lmpc_rollout_relaunch", "more per-problem arrays than LMPC_RELAUNCH_MAX_SPANS (lmpc_relaunch.hip.h)");
    // both streams of the session drained: the logs are complete up to step t, doneAt and finX stand, no launch reads what the kernel writes
    RCCHK(ctx_enter(c)); RESOLVE_PENDING();
    HIPCHK(hipStreamSynchronize(r->pstream)); HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<int> done((size_t)B);
    HIPCHK(hipMemcpy(done.data(), r->d_done, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        const int car = cars[i], s0 = session_lap_start(r, car);
        if (done[(size_t)car] < 0) { snprintf(msg, sizeof(msg), "car %d has not crossed the line (doneAt < 0)", car); return set_err(LMPC_E_STATE, "lmpc_rollout_relaunch", msg); }
        if (done[(size_t)car] - s0 < N + 2) { snprintf(msg, sizeof(msg), "the lap of car %d has %d rows, the next lap linearises about rows 1 .. N + 1 = %d of it", car, done[(size_t)car] - s0, N + 1); return set_err(LMPC_E_ARG, "lmpc_rollout_relaunch", msg); }
    }
    // ---- nothing is refused from here on
    const size_t Bz = (size_t)B, stride = lt ? (size_t)r->lt_stride : 0;
    if (!r->d_lapStart) {                                             // beside the kept set, as the live list is: later sessions on these buffers reuse it
        void *q = nullptr;
        if (g_malloc(&q, sizeof(int) * Bz) != hipSuccess) return set_err(LMPC_E_HIP, "hipMalloc", "lap starts");
        r->keep.push_back(q); r->d_lapStart = (int *)q;
    }
    const bool first = !r->relaunched;
    if (first) { HIPCHK(hipMemsetAsync(r->d_lapStart, 0, sizeof(int) * Bz, c->stream)); r->lapStart.assign(Bz, 0); r->lapNo.assign(Bz, 0); }
    // one upload: the entry table, behind it the cars' rows of the lap table in force, resolved against the stores as they are now
    std::vector<char> up(sizeof(lmpc_relaunch_entry) * (size_t)n + sizeof(int) * stride * (size_t)n);
    lmpc_relaunch_entry *tab = (lmpc_relaunch_entry *)up.data(); int *rows = (int *)(up.data() + sizeof(lmpc_relaunch_entry) * (size_t)n);
    for (int i = 0; i < n; i++) {
        const int car = cars[i];
        tab[i] = {car, r->lapStart[(size_t)car], r->lapNo[(size_t)car] + 1, 0, track_length_of(c, car)};
        if (lt) { bool small = true; resolve_lap_row(c, c->lt.row(car), rows + (size_t)i * stride, &small); }
    }
    void *scr; RCCHK(pooled_scratch(c, up.size(), &scr));
    HIPCHK(hipMemcpyAsync(scr, up.data(), up.size(), hipMemcpyHostToDevice, c->stream));
    lmpc_relaunch_args a = {};
    a.B = B; a.N = N; a.t = r->t; a.T_max = r->T_max; a.lap_rows = lap_rows; a.lt_stride = (int)stride; a.dev_noise = r->nz_dev ? 1 : 0;
    a.seed = r->nz_seed; a.lap0 = r->nz_lap; a.car0 = (unsigned long long)r->nz_car0;
    a.x = r->a.x0; a.xg = r->d_xg; a.xLin = r->a.xLin; a.uLin = r->a.uLin; a.zt = r->a.zt; a.finX = r->d_finX; a.finG = r->d_finG; a.noise = r->d_noise;
    a.logX = r->d_logX; a.logU = r->d_logU; a.doneAt = r->d_done; a.statusAcc = r->d_stAcc; a.nDone = r->d_nDone; a.lapStart = r->d_lapStart; a.lt = r->d_lt;
    lmpc_arrays_each(c->dims, [&](const char *, auto m, size_t elem, size_t cnt, int) {      // (every array the session holds, by the table: a later array is covered)
        if (r->a.*m && cnt) a.span[a.n_spans++] = {(unsigned *)(r->a.*m), (unsigned)(elem * cnt / sizeof(unsigned)), 0u}; });
    hipLaunchKernelGGL(lmpc_rollout_relaunch_kernel, dim3((unsigned)n), dim3(LMPC_RELAUNCH_NT), 0, c->stream, a, (const lmpc_relaunch_entry *)scr,
                       (const int *)((const char *)scr + sizeof(lmpc_relaunch_entry) * (size_t)n));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));                          // (`up` is a local; and the next lmpc_rollout_run finds the session as a begin leaves it)
    // the books, once the launch has completed
    r->relaunched = true;
    for (int i = 0; i < n; i++) {
        const size_t car = (size_t)cars[i];
        r->lapStart[car] = r->t; r->lapNo[car] += 1;
        if (lt) std::copy(rows + (size_t)i * stride, rows + (size_t)(i + 1) * stride, r->lt_host.begin() + car * stride);
    }
    if (lt) { bool small = true; for (size_t k = 1; k < r->lt_host.size(); k += 2) small = small && r->lt_host[k] - 1 <= 8 * WAVE; r->lt_small = small; }
    return LMPC_OK;
}

int lmpc_rollout_lap_start(lmpc_ctx *c, int *start, int *lap) {
    // of the active session: the session row each car's current lap began at and the laps it has begun after its first; zeros in a session that has not relaunched
    ARGCHK(c);
    if (!(c->ro && c->ro->active)) return set_err(LMPC_E_STATE, "lmpc_rollout_lap_start", "no rollout session is active");
    const lmpc_rollout_session *r = c->ro;
    for (int b = 0; b < r->B; b++) {
        if (start) start[b] = r->relaunched ? r->lapStart[(size_t)b] : 0;
        if (lap) lap[b] = r->relaunched ? r->lapNo[(size_t)b] : 0;
    }
    return LMPC_OK;
}

int lmpc_rollout_fetch(lmpc_ctx *c, int t0, int t1, double *X, double *U, double *G, int *doneAt, int *status, double *finalX, double *finalG) {
    // logs of steps [t0, t1): X/G (t1-t0) x B x 6, U (t1-t0) x B x 2; doneAt: steps until s > TrackLength (-1: not yet);
    // finalX / finalG: state right after the crossing step (the reference's xF before the TrackLength shift, SysModel.py:50)
    ARGCHK(c && c->ro && c->ro->active && t0 >= 0 && t1 >= t0 && t1 <= c->ro->t);
    lmpc_rollout_session *r = c->ro; const size_t Bz = r->B, n = (size_t)(t1 - t0);
    RCCHK(ctx_enter(c));
    if (n) { D2H(X, r->d_logX + (size_t)t0 * Bz * 6, n * Bz * 6); D2H(U, r->d_logU + (size_t)t0 * Bz * 2, n * Bz * 2); D2H(G, r->d_logG + (size_t)t0 * Bz * 6, n * Bz * 6); }
    D2H(doneAt, r->d_done, Bz); D2H(status, r->d_stAcc, Bz); D2H(finalX, r->d_finX, Bz * 6); D2H(finalG, r->d_finG, Bz * 6);
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_rollout_set_trace(lmpc_ctx *c, int n, const int *cars, unsigned what) {
    // the cars and planes of the sessions begun after this call (an active session keeps its snapshot); checked in full before anything changes; needs no device.
    // A car >= B can only be judged by the begin that meets it (rollout_setup)
    ARGCHK(c && n >= 0 && (n == 0 || cars));
    if (n > 0) {
        ARGCHK(what != 0 && (what & ~LMPC_TRACE_ALL) == 0);
        if (c->cfg.numSS_it == 0 && (what & (LMPC_TRACE_SS | LMPC_TRACE_QSEL)))
            return set_err(LMPC_E_ARG, "lmpc_rollout_set_trace", "LMPC_TRACE_SS / LMPC_TRACE_QSEL on a context without a safe set (numSS_it == 0)");
        std::vector<int> sorted(cars, cars + n); std::sort(sorted.begin(), sorted.end());
        if (sorted[0] < 0) { char msg[64]; snprintf(msg, sizeof(msg), "car %d is negative", sorted[0]); return set_err(LMPC_E_ARG, "lmpc_rollout_set_trace", msg); }
        for (int k = 1; k < n; k++) if (sorted[(size_t)k] == sorted[(size_t)k - 1]) { char msg[64]; snprintf(msg, sizeof(msg), "car %d is listed twice", sorted[(size_t)k]); return set_err(LMPC_E_ARG, "lmpc_rollout_set_trace", msg); }
    }
    c->trace_cars.assign(cars, cars + n); c->trace_what = n ? what : 0u;
    return LMPC_OK;
}

int lmpc_rollout_set_parking(lmpc_ctx *c, unsigned mode, int n, const int *cars) {
    // the cars later sessions park from step 0 and the LMPC_PARK_* bits; everything is checked before anything changes, no device needed.
    // A car >= B can only be judged by the begin that meets it (rollout_setup)
    if (!c) return set_err(LMPC_E_ARG, "lmpc_rollout_set_parking", "null context");
    if (mode & ~(unsigned)(LMPC_PARK_FINISHED | LMPC_PARK_REROUTE)) return set_err(LMPC_E_ARG, "lmpc_rollout_set_parking", "unknown mode bits");
    if (n < 0 || (n > 0 && !cars)) return set_err(LMPC_E_ARG, "lmpc_rollout_set_parking", n < 0 ? "n is negative" : "n > 0 with NULL cars");
    if (n > 0) {
        std::vector<int> sorted(cars, cars + n); std::sort(sorted.begin(), sorted.end());
        if (sorted[0] < 0) { char msg[64]; snprintf(msg, sizeof(msg), "car %d is negative", sorted[0]); return set_err(LMPC_E_ARG, "lmpc_rollout_set_parking", msg); }
        for (int k = 1; k < n; k++) if (sorted[(size_t)k] == sorted[(size_t)k - 1]) { char msg[64]; snprintf(msg, sizeof(msg), "car %d is listed twice", sorted[(size_t)k]); return set_err(LMPC_E_ARG, "lmpc_rollout_set_parking", msg); }
    }
    if (n > 0) c->park_cars.assign(cars, cars + n); else c->park_cars.clear();
    c->park_mode = mode;
    return LMPC_OK;
}

int lmpc_rollout_get_parking(lmpc_ctx *c, unsigned *mode, int *n, int *cars, int capacity) {
    ARGCHK(c && capacity >= 0);
    if (mode) *mode = c->park_mode;
    if (n) *n = (int)c->park_cars.size();
    if (cars) for (int k = 0; k < capacity && k < (int)c->park_cars.size(); k++) cars[k] = c->park_cars[(size_t)k];
    return LMPC_OK;
}

int lmpc_rollout_parked_at(lmpc_ctx *c, int *at, int *n_live) {
    // per car of the active session: -1 while it is live, else the first step it was not stepped (its state, log rows and trace planes stand still from there)
    ARGCHK(c);
    if (!(c->ro && c->ro->active)) return set_err(LMPC_E_STATE, "lmpc_rollout_parked_at", "no rollout session is active");
    lmpc_rollout_session *r = c->ro;
    if (n_live) *n_live = r->parked ? r->nLive : r->B;
    if (at) {
        if (r->parked) { RCCHK(ctx_enter(c)); HIPCHK(hipMemcpy(at, r->d_parkedAt, sizeof(int) * (size_t)r->B, hipMemcpyDeviceToHost)); }
        else for (int b = 0; b < r->B; b++) at[b] = -1;
    }
    return LMPC_OK;
}

int lmpc_debug_live_compact(lmpc_ctx *c, int n, const int *doneAt, const int *parked0, int t, unsigned mode, int *live, int *parkedAt, int *n_live) {
    // (every build) the sessions' compaction kernel on host arrays: doneAt, parked0 (n flags) in; parkedAt (n) in and out -- -1 for a car not parked so far;
    // live (n: the first n_live entries are written) and n_live out.  One launch, as a session makes it
    ARGCHK(c && n >= 1 && doneAt && parked0 && live && parkedAt && n_live && t >= 0 && !(mode & ~(unsigned)(LMPC_PARK_FINISHED | LMPC_PARK_REROUTE)));
    RCCHK(ctx_enter(c));
    const size_t nz = (size_t)n;
    int *d = nullptr; HIPCHK(g_malloc((void **)&d, sizeof(int) * (4 * nz + 4)));
    int *d_done = d, *d_p0 = d + nz, *d_at = d + 2 * nz, *d_live = d + 3 * nz, *d_hdr = d + 4 * nz;
    int hdr[4] = {0, 0, 0, 0};
    hipError_t e = hipMemcpyAsync(d_done, doneAt, sizeof(int) * nz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_p0, parked0, sizeof(int) * nz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_at, parkedAt, sizeof(int) * nz, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_live, 0xff, sizeof(int) * nz, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_hdr, 0, sizeof(int) * 4, c->stream);
    if (e == hipSuccess) {
        const lmpc_live_args la = {n, t, mode, 1, d_done, d_p0, d_at, d_live, d_hdr};
        hipLaunchKernelGGL(lmpc_rollout_live_kernel, dim3(1), dim3(LMPC_LIVE_NT), 0, c->stream, la);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(live, d_live, sizeof(int) * nz, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(parkedAt, d_at, sizeof(int) * nz, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hdr, d_hdr, sizeof(int) * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)g_free(d);
    if (e != hipSuccess) return set_err(LMPC_E_HIP, "lmpc_debug_live_compact", hipGetErrorString(e));
    *n_live = hdr[1];
    return LMPC_OK;
}

int lmpc_rollout_get_trace(lmpc_ctx *c, int *n, int *cars, unsigned *what, int capacity) {
    ARGCHK(c && n && capacity >= 0);
    *n = (int)c->trace_cars.size();
    if (what) *what = c->trace_what;
    if (cars) memcpy(cars, c->trace_cars.data(), sizeof(int) * (size_t)std::min(capacity, *n));
    return LMPC_OK;
}

int lmpc_rollout_trace_bytes(lmpc_ctx *c, int n, unsigned what, int T_max, long long *bytes) {
    ARGCHK(c && bytes && n >= 0 && T_max >= 0 && (what & ~LMPC_TRACE_ALL) == 0);
    size_t pb[LMPC_TRACE_PLANES], per = 0; trace_plane_bytes(c, what, pb);
    for (int i = 0; i < LMPC_TRACE_PLANES; i++) per += pb[i];
    *bytes = (long long)per * (long long)n * (long long)T_max;
    return LMPC_OK;
}

int lmpc_rollout_fetch_trace(lmpc_ctx *c, int t0, int t1, const lmpc_trace_out *out) {
    // trace rows of steps [t0, t1), every plane [t - t0][k][...] with k the position in the session's car list; a NULL pointer skips its plane
    ARGCHK(c && out);
    if (!(c->ro && c->ro->active)) return set_err(LMPC_E_STATE, "lmpc_rollout_fetch_trace", "no rollout session is active");
    lmpc_rollout_session *r = c->ro;
    if (r->kind == RO_PID || r->tr_n == 0) return set_err(LMPC_E_STATE, "lmpc_rollout_fetch_trace", r->kind == RO_PID ? "a PID session records no trace" : "the session was begun without a trace (lmpc_rollout_set_trace)");
    ARGCHK(t0 >= 0 && t1 >= t0 && t1 <= r->t);
    ARGCHK((!out->xPred || r->tr_x) && (!out->uPred || r->tr_u) && (!out->ssSel || r->tr_ss) && (!out->qSel || r->tr_q) && (!out->xyPred || r->tr_xy) &&
           (!out->xySS || r->tr_xys) && (!out->iters || r->tr_it) && (!out->status || r->tr_st) && (!out->mapStatus || r->tr_map));     // (a plane the session does not record)
    RCCHK(ctx_enter(c)); HIPCHK(hipStreamSynchronize(r->tstream)); HIPCHK(hipStreamSynchronize(r->pstream));
    size_t pb[LMPC_TRACE_PLANES]; trace_plane_bytes(c, r->tr_what, pb);
    const size_t first = (size_t)t0 * (size_t)r->tr_n, rows = (size_t)(t1 - t0) * (size_t)r->tr_n;
    void *dst[LMPC_TRACE_PLANES] = {out->xPred, out->uPred, out->ssSel, out->qSel, out->iters, out->status, out->xyPred, out->xySS, out->mapStatus};
    const void *src[LMPC_TRACE_PLANES] = {r->tr_x, r->tr_u, r->tr_ss, r->tr_q, r->tr_it, r->tr_st, r->tr_xy, r->tr_xys, r->tr_map};
    for (int i = 0; i < LMPC_TRACE_PLANES; i++)
        if (dst[i] && rows && pb[i]) HIPCHK(hipMemcpyAsync(dst[i], (const char *)src[i] + first * pb[i], rows * pb[i], hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_debug_rollout_peek(lmpc_ctx *c, double *xLin, double *uLin, int *status, int *rstatus) {
    // developer entry point: the rollout session's current linearisation trajectories (B x (N+1) x 6, B x N x 2 -- what the NEXT step's regression will be asked) and the
    // status words of the step just taken (per rollout: B; per horizon point of its regression: B x N).  tools/robustness_sweep.py steps a generation one step at a
    // time with it to capture the inputs of a flagged regression.  Any pointer may be NULL.
    ARGCHK(c && c->ro && c->ro->active);
    lmpc_rollout_session *r = c->ro;
    RCCHK(ctx_enter(c)); HIPCHK(hipStreamSynchronize(r->pstream)); HIPCHK(hipStreamSynchronize(c->stream));
    lmpc_arrays out = {}; out.xLin = xLin; out.uLin = uLin; out.status = status; out.rstatus = rstatus;
    RCCHK(copy_arrays(c, r->B, c->dims, out, r->a, hipMemcpyDeviceToHost));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_debug_rollout_capture(lmpc_ctx *c, int on) {
    // developer entry point: rollout sessions begun after this call also write the selected safe-set points / Q-values of every step (B x S x 6, B x S) so that
    // lmpc_debug_rollout_qp can hand a closed-loop QP to the oracle.  Off (the default) the step does not write them.
    ARGCHK(c && !(c->ro && c->ro->active));
    c->dbg_capture = on ? 1 : 0;
    return LMPC_OK;
}

int lmpc_debug_rollout_qp(lmpc_ctx *c, int b0, int n, double *A, double *Bm, double *Cm, double *xPred, double *uPred, double *ssSel, double *qSel, double *succ, double *succU,
                          double *lambda, double *ztNext, double *ztuNext, int *iters, int *status) {
    // developer entry point: the QP the LAST simulated step solved for rollouts b0 .. b0 + n - 1 -- the regression's A, B, C (n x N x 36 / 12 / 6), the kernel's
    // answer (n x (N+1) x 6, n x N x 2, n x S; zt / zt_u of feasibleStateInput: n x 6, n x 2), iterations and status, and (capture on) the selected safe-set points, their
    // Q-values and successors (n x S x 6, n x S, n x S x 6, n x S x 2).  Its x0 / uOld are rows t - 1 / t - 2 of the session's logs (lmpc_rollout_fetch).  Meant to be
    // called between lmpc_rollout_run(ctx, 1, ..) calls; any pointer may be NULL.
    ARGCHK(c && c->ro && c->ro->active && c->ro->t >= 1 && b0 >= 0 && n >= 1 && b0 + n <= c->ro->B && ((!ssSel && !qSel && !succ && !succU) || c->ro->a.ssSel));
    lmpc_rollout_session *r = c->ro;
    RCCHK(ctx_enter(c)); HIPCHK(hipStreamSynchronize(r->pstream)); HIPCHK(hipStreamSynchronize(c->stream));
    lmpc_arrays out = {};
    out.A = A; out.Bm = Bm; out.C = Cm; out.xPred = xPred; out.uPred = uPred; out.lambda = lambda; out.ztNext = ztNext; out.ztuNext = ztuNext;
    out.ssSel = ssSel; out.qSel = qSel; out.succ = succ; out.succU = succU; out.iters = iters; out.status = status;
    RCCHK(copy_arrays(c, n, c->dims, out, r->a, hipMemcpyDeviceToHost, b0));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LMPC_OK;
}

int lmpc_rollout_end(lmpc_ctx *c) {
    ARGCHK(c); RCCHK(ctx_enter(c)); HIPCHK(hipStreamSynchronize(c->stream));
    if (c->ro) {
        if (c->ro->pstream) HIPCHK(hipStreamSynchronize(c->ro->pstream));
        if (c->ro->tstream) HIPCHK(hipStreamSynchronize(c->ro->tstream));
#ifdef LMPC_GUARD
        rollout_free(c);                                   // (guard builds check the zone behind every buffer when it is freed: keep doing that per session)
#else
        c->ro->active = false;
#endif
    }
    return LMPC_OK;
}

int lmpc_rollout_release(lmpc_ctx *c) {
    // lmpc_rollout_end keeps the session's device buffers (~35 allocations, 55 MB at 1024 rollouts x 400 steps), its stream and events for the next lap of the same
    // shape; this gives them back without destroying the context.  Not valid inside a session.
    ARGCHK(c && !(c->ro && c->ro->active));
    RCCHK(ctx_enter(c)); HIPCHK(hipStreamSynchronize(c->stream));
    rollout_free(c);
    return LMPC_OK;
}

int lmpc_lti_regression_batch(int device, int B, const double *x, const double *u, const int *T, int ldT, double lamb, double *A, double *Bm, double *Error, int *status) {
    // Utilities.Regression (fnc/Utilities.py:5-28) for B laps in one launch, one work-group per lap: lap b has T[b] rows at x + b * ldT * 6 (u + b * ldT * 2), rows beyond
    // T[b] are not read.  A: B x 6 x 6, Bm: B x 6 x 2, Error: B x 2 x 6, status: B or NULL.  No context needed (main.py:74-77 runs before any controller exists).
    ARGCHK(x && u && T && A && Bm && Error && B >= 1 && ldT >= 3);
    for (int b = 0; b < B; b++) ARGCHK(T[b] >= 3 && T[b] <= ldT);
    HIPCHK(hipSetDevice(device));
    const size_t Bz = B, rows = Bz * (size_t)ldT;
    double *d; HIPCHK(hipMalloc(&d, sizeof(double) * (rows * 8 + Bz * 60) + sizeof(int) * 2 * Bz));
    double *dx = d, *du = d + rows * 6, *dout = du + rows * 2; int *dst = (int *)(dout + Bz * 60), *dT = dst + Bz;
    hipError_t e = hipMemcpy(dx, x, sizeof(double) * rows * 6, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(du, u, sizeof(double) * rows * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dT, T, sizeof(int) * Bz, hipMemcpyHostToDevice);
    std::vector<double> hout(Bz * 60); std::vector<int> hst(Bz, 0);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(lmpc_lti_regress_kernel, dim3(B), dim3(LTI_NT), 0, 0, (const double *)dx, (const double *)du, (const int *)dT, ldT, lamb, dout, dst);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(hout.data(), dout, sizeof(double) * hout.size(), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(hst.data(), dst, sizeof(int) * Bz, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return set_err(LMPC_E_HIP, "lmpc_lti_regression_batch", hipGetErrorString(e));
    for (size_t b = 0; b < Bz; b++) {
        memcpy(A + b * 36, &hout[b * 60], sizeof(double) * 36); memcpy(Bm + b * 12, &hout[b * 60 + 36], sizeof(double) * 12); memcpy(Error + b * 12, &hout[b * 60 + 48], sizeof(double) * 12);
        if (status) status[b] = hst[b];
    }
    return LMPC_OK;
}

int lmpc_lti_regression(int device, const double *x, const double *u, int T, double lamb, double *A, double *B, double *Error, int *status) {
    // Utilities.Regression (fnc/Utilities.py:5-28), called by main.py:74-77 before any controller exists: no context needed.  The one-lap call of the batched form.
    ARGCHK(x && u && A && B && Error && T >= 3);
    return lmpc_lti_regression_batch(device, 1, x, u, &T, T, lamb, A, B, Error, status);
}

int lmpc_selftest(lmpc_ctx *c) {
    // cross-lane primitives (DPP + v_permlane16/32_swap reductions) against closed-form values
    ARGCHK(c);
    RCCHK(ctx_enter(c));
    double *d; HIPCHK(hipMalloc(&d, sizeof(double) * 192));
    hipLaunchKernelGGL(lmpc_selftest_kernel, dim3(1), dim3(WAVE), 0, c->stream, d);
    double hbuf[192]; HIPCHK(hipMemcpyAsync(hbuf, d, sizeof(hbuf), hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); hipFree(d);
    double s = 0, mx = -1e300, mn = 1e300;
    for (int l = 0; l < 64; l++) { const double v = 1.0 + 0.25 * l + ((l * 37) % 11) * 1e-3; s += v; mx = v > mx ? v : mx; mn = v < mn ? v : mn; }
    for (int l = 0; l < 64; l++) {
        if (fabs(hbuf[l] - s) > 1e-9 * s || hbuf[64 + l] != mx || hbuf[128 + l] != mn) return set_err(LMPC_E_HIP, "wave reduction self test failed", "");
    }
    return LMPC_OK;
}

int lmpc_debug_set_trace(lmpc_ctx *c, double *dev_rows) {
    // developer builds (-DLMPC_TRACE): every later solve launch writes LMPC_TRACE_ROWS x 6 doubles per problem into dev_rows (caller-owned device memory, at least
    // max_batch x 48 x 6 doubles; NULL switches it off): per iteration (gap, r_d, r_e | sigma, alpha_p, alpha_d).  Ordinary builds carry no such code: LMPC_E_ARG.
    ARGCHK(c);
#ifdef LMPC_TRACE
    RCCHK(ctx_enter(c)); RESOLVE_PENDING(); HIPCHK(hipStreamSynchronize(c->stream));
    c->dbg_trace = dev_rows;
    return LMPC_OK;
#else
    (void)dev_rows;
    return set_err(LMPC_E_ARG, "lmpc_debug_set_trace", "this library was built without -DLMPC_TRACE (racinglmpc_amd.build.build_flavour)");
#endif
}

int lmpc_debug_exec_audit(lmpc_ctx *c, unsigned long long *out16, int reset) {
    // developer builds (-DLMPC_EXEC_AUDIT): out16[site] = calls of a cross-lane primitive that found an incomplete EXEC mask, out16[8 + site] = calls, since
    // the last reset (sites: lmpc_kernels.hip.h, EXEC_AUDIT); built-in variants only (a liblmpc_var_*.so carries counters of its own).  Ordinary builds: LMPC_E_ARG.
    ARGCHK(c && out16);
#ifdef LMPC_EXEC_AUDIT
    RCCHK(ctx_enter(c)); HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_exec_audit), sizeof(unsigned long long) * 2 * LMPC_AUDIT_SITES));
    if (reset) { unsigned long long z[2 * LMPC_AUDIT_SITES] = {0}; HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_exec_audit), z, sizeof(z))); }
    return LMPC_OK;
#else
    (void)reset;
    return set_err(LMPC_E_ARG, "lmpc_debug_exec_audit", "this library was built without -DLMPC_EXEC_AUDIT (racinglmpc_amd.build.build_flavour)");
#endif
}

int lmpc_solver_waves(lmpc_ctx *c, int B) {
    if (!c) return LMPC_E_ARG;
    if (B <= c->mw_max_batch) return 4;
    if (B <= c->mw2_max_batch) return 2;
    return 1;
}

int lmpc_solver_lds(lmpc_ctx *c, unsigned long long out4[4]) {
    ARGCHK(c && out4);
    out4[0] = c->var.lds_1w; out4[1] = c->var.lds_1w_abg; out4[2] = c->var.lds_mw; out4[3] = (unsigned long long)c->n_cu;
    return LMPC_OK;
}

int lmpc_set_profiling(lmpc_ctx *c, int every) { ARGCHK(c); RCCHK(ctx_enter(c)); c->profiling = every > 0 ? every : 0; return LMPC_OK; }      // (a held solve is launched under the setting of its step)
static int drain_events(lmpc_ctx *c) {
    RCCHK(ctx_enter(c)); HIPCHK(hipStreamSynchronize(c->stream));
    for (auto &e : c->events) {
        float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, e.a, e.b));
        if (e.kind == 0) { c->stats.ms_regress += ms; c->stats.n_regress_timed++; } else { c->stats.ms_solve += ms; c->stats.n_solve_timed++; }
        hipEventDestroy(e.a); hipEventDestroy(e.b);
    }
    c->events.clear();
    return LMPC_OK;
}
int lmpc_get_stats(lmpc_ctx *c, lmpc_stats *out) { ARGCHK(c && out); int rc = drain_events(c); if (rc) return rc; *out = c->stats; return LMPC_OK; }
int lmpc_reset_stats(lmpc_ctx *c) { ARGCHK(c); int rc = drain_events(c); if (rc) return rc; memset(&c->stats, 0, sizeof(c->stats)); return LMPC_OK; }

}  // extern "C"

#include "lmpc_comm.hip.h"
