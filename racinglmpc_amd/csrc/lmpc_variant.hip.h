// racinglmpc_amd/csrc/lmpc_variant.hip.h -- one (N, numSS_points) instantiation of the solve kernels behind a small table of launchers.
//
// The solve kernels are templates on the horizon N and the number of safe-set columns S (every LDS offset, trip count and register array
// is a compile-time constant).  The library carries the reference's configurations built in (lmpc_capi.hip: N in {8,12,14,20,40} x S in
// {0,48}); any other pair -- the reference takes any N (main.py:43) and numSS_Points = 12 numSS_it (initControllerParameters.py:43-44) -- is
// a shared object of its own, liblmpc_var_N<N>_S<S>.so next to the library (racinglmpc_amd/csrc/lmpc_variant.hip compiled with
// -DLMPC_VAR_N / -DLMPC_VAR_S; racinglmpc_amd.build.build_variant), loaded by lmpc_create on demand.
#pragma once
#include "lmpc_kernels.hip.h"
#include "lmpc_solve_mw.hip.h"
#ifndef LMPC_VARIANT_TU
#include "lmpc_solve_rt.hip.h"       // the runtime-(N, S) fallback kernel lives in the library only
#endif
#ifdef LMPC_WITH_CD                  // the condensed kernel is a measured alternative (not faster), kept out of the default build: racinglmpc_amd.build.build_flavour("cd", ["LMPC_WITH_CD"])
#include "lmpc_solve_cd.hip.h"
#endif

struct lmpc_variant_api {
    int N, S;
    size_t lds_mw, lds_1w;                    // dynamic LDS per QP: multi-wave kernels / one-wave kernels
    int (*launch_1w)(hipStream_t, const lmpc_dev_params &, int B, const lmpc_solve_io &, const int *live);      // lmpc_solve_kernel<N,S>
    int (*launch_retry)(hipStream_t, const lmpc_dev_params &, int B, const lmpc_solve_io &, const int *live);   // lmpc_solve_kernel<N,S,true>
    int (*launch_mw4)(hipStream_t, const lmpc_dev_params &, int B, const lmpc_solve_io &, const int *live);     // lmpc_solve_kernel_mw<N,S,4>
    int (*launch_mw2)(hipStream_t, const lmpc_dev_params &, int B, const lmpc_solve_io &, const int *live);     // lmpc_solve_kernel_mw<N,S,2>
    size_t lds_1w_abg;                        // one-wave kernel with [A_k | B_k] in global memory (long horizons): dynamic LDS per QP; 0 = not used for this (N, S)
    size_t lds_cd;                            // condensed one-wave kernel (lmpc_solve_cd.hip.h): dynamic LDS per QP without the state-cost block; 0 = not built for this (N, S)
    size_t lds_cd_q;                          //   ... with it (Q or Qf non-zero)
    int (*launch_cd)(hipStream_t, const lmpc_dev_params &, int B, const lmpc_solve_io &, int hasQ);   // lmpc_solve_kernel_cd<N,S>
    int occ_mw2;                              // work-groups of the two-wave kernel the runtime keeps resident per CU (asked, not assumed: 0 = unknown)
    // lmpc_solve_kernel_mw<N,S,4,false,lmpc_k1_next>: the plain four-wave solve of B problems and, in the same launch, the regression of the next step (lmpc_merge.h);
    // null where the (N, S) has no multi-wave kernels
    int (*launch_mw4_next)(hipStream_t, const lmpc_dev_params &, int B, const lmpc_solve_io &, const lmpc_k1_next &);
};

// What lmpc_create asks a variant library for (lmpc_variant_get): the revision and the sizes of the three structures that cross the boundary by value or
// by layout.  A liblmpc_var_*.so built against another layout of the parameter block answers -1 and is rebuilt (racinglmpc_amd._capi: E_VARIANT).
constexpr int LMPC_VARIANT_ABI = LMPC_VARIANT_ABI_REV * 0x1000000 + (int)((sizeof(lmpc_dev_params) * 31u + sizeof(lmpc_solve_io) * 7u + sizeof(lmpc_variant_api)) & 0xffffffu);
static_assert(sizeof(lmpc_dev_params) < 4096 && sizeof(lmpc_solve_io) < 1024, "by-value kernel arguments: keep them inside the kernarg segment's preload range");

// One solve family of an (N, S) -- a kernel with its plain, its TAB and its list instantiation -- described once; the launchers, the dynamic-LDS limits and the occupancy
// query read this.  A launch with per-problem rows -- safe-set laps (io.ssTab), controller tuning (lmpc_tuning_set), or both; the host sets io.tune for every such launch
// (lmpc_capi.hip, launch_solve) -- takes `tab`, with LMPC_SSTAB_LDS bytes behind the launch's LDS for the (slot, rows) of the selected laps.  (S = 0 has the TAB
// instantiations for the tuning rows alone: no table there, lmpc_capi.hip, ss_table_for.)
// list: the parking instantiation of the same kernel, which takes the list beside io (B entries; per-problem rows as well, the host sets io.tune with the list) --
// an instantiation of its own, so that `plain` and `tab` are the kernels they were for every launch outside a parking session.
// lds: the dynamic LDS of a plain launch;  lim / lim_tab: the limit of `plain` and that of `tab` and `list`.
template <class K, class KL> struct lmpc_solve_family { K plain, tab; KL list; int threads; size_t lds, lim, lim_tab; };
template <class K, class KL> lmpc_solve_family(K, K, KL, int, size_t, size_t, size_t) -> lmpc_solve_family<K, KL>;
// (`live`: the last argument of the launchers of lmpc_variant_api, null outside a parking session)
template <class K, class KL> static int lmpc_launch_pair(const lmpc_solve_family<K, KL> &f, hipStream_t st, const lmpc_dev_params &p, int B, const lmpc_solve_io &io, const int *live) {
    if (live) hipLaunchKernelGGL(f.list, dim3(B), dim3(f.threads), f.lds + LMPC_SSTAB_LDS, st, p, B, io, lmpc_live_list{live, B});
    else hipLaunchKernelGGL(io.tune ? f.tab : f.plain, dim3(B), dim3(f.threads), f.lds + (io.tune ? LMPC_SSTAB_LDS : 0), st, p, B, io);
    return 0;
}
static bool lmpc_raise_lds_limit(const void *fn, size_t lds) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess; }
template <class K, class KL> static bool lmpc_raise_lds_limits(const lmpc_solve_family<K, KL> &f) {
    return lmpc_raise_lds_limit((const void *)f.plain, f.lim) && lmpc_raise_lds_limit((const void *)f.tab, f.lim_tab) && lmpc_raise_lds_limit((const void *)f.list, f.lim_tab);
}

template <int N, int S> struct lmpc_variant_launchers {
    // (every supported S has the multi-wave kernels where their layout fits: wave 0 carries ceil((S + 6) / 64) terminal-block columns per lane)
    static constexpr size_t lds1 = (size_t)solve_lds1<N, S>::tot * sizeof(double), ldsm = (size_t)solve_lds<N, S>::tot * sizeof(double);
    // The multi-wave layout shares nothing between phases and outgrows the 160 KB of a CU long before the one-wave layout does (N = 64 from 96 safe-set
    // points, N = 40 at 384).  Such an (N, S) has no multi-wave kernels -- they are not instantiated -- and runs one wave per QP at every batch size (lds_mw = 0:
    // lmpc_capi.hip, create_body).  mw_static: an upper bound of the multi-wave kernel's static LDS (red, phi_sh, gs0, ss_rowsum, sel_start, two words), which
    // counts against the same 160 KB.
    static constexpr size_t mw_static = (size_t)(8 * N + 160) * sizeof(double);
    static constexpr bool has_mw = ldsm + LMPC_SSTAB_LDS + mw_static <= (size_t)160 * 1024;
    // fused step (io.mode & 4): the regression's work space sits behind [A_k | B_k], C_k; it fits the solve's footprint at the reference's
    // settings (4 laps x 7 points) and grows it a little beyond
    static size_t lds_for(const lmpc_dev_params &p, const lmpc_solve_io &io) {
        const size_t f = (io.mode & 4) ? (size_t)(54 * N + k1_fused_doubles(N, p.trToUse, p.maxNumPoint)) * sizeof(double) : 0;
        return f > lds1 ? f : lds1;
    }
    static constexpr size_t lds1_max() { const size_t f = (size_t)(54 * N + k1_fused_doubles(N, LMPC_MAX_USED_LAPS, 8)) * sizeof(double); return (f > lds1 ? f : lds1) + LMPC_SSTAB_LDS; }
    // long horizons: [A_k | B_k] in global memory where that lets more QPs share a CU than the 160 KB of LDS otherwise hold and fewer than four do (idle SIMDs)
    static constexpr size_t lds1g = (size_t)solve_lds1<N, S, true>::tot * sizeof(double);
    // (measured, solve kernel, ms at batch 1024 / 4096: N = 40 LDS 1.467 / 4.073, global 1.092 / 3.398 -- two -> four QPs per CU;  N = 20 LDS 0.655 / 1.571,
    //  global 0.725 / 1.554 -- five -> seven per CU, but every SIMD was busy already and the variant spills: only where fewer than four QPs fit)
    static constexpr bool use_abg = (160 * 1024 / lds1) < 4 && (160 * 1024 / lds1g) > (160 * 1024 / lds1) && solve_lds1<N, S>::CH == 1;
#ifdef LMPC_WITH_CD
    static constexpr bool has_cd = 2 * N <= 32 && S + 6 <= WAVE;          // condensed kernel: short horizons, one terminal-block column per lane
#else
    static constexpr bool has_cd = false;
#endif
    static constexpr size_t lds_cd(bool hasQ) {
#ifdef LMPC_WITH_CD
        if constexpr (has_cd) return (size_t)(hasQ ? solve_ldsc<N, S>::tot_q : solve_ldsc<N, S>::tot) * sizeof(double);
#endif
        return 0; }

    // The families of this (N, S), each instantiation named here and nowhere else (per-problem rows, io.ssTab / io.tune: every (N, S) has the TAB instantiations -- S = 0 for the tuning rows).
    // one-wave (EQ: its retry pass): a launch says what it takes (lds_for), the limit is lds1_max;  ABG: [A_k | B_k] in global memory, instantiated only where use_abg
    template <bool EQ, bool ABG = false> static auto one_wave(size_t lds = ABG ? lds1g : lds1) {
        return lmpc_solve_family{lmpc_solve_kernel<N, S, EQ, ABG>, lmpc_solve_kernel<N, S, EQ, ABG, true>, lmpc_solve_kernel<N, S, EQ, ABG, true, lmpc_live_list>, WAVE,
                                 lds, ABG ? lds1g : lds1_max(), ABG ? lds1g + LMPC_SSTAB_LDS : lds1_max()}; }
    template <int NW> static auto multi_wave() {
        return lmpc_solve_family{lmpc_solve_kernel_mw<N, S, NW>, lmpc_solve_kernel_mw<N, S, NW, true>, lmpc_solve_kernel_mw<N, S, NW, true, lmpc_live_list>, WAVE * NW,
                                 ldsm, ldsm, ldsm + LMPC_SSTAB_LDS}; }

    // the two-role build of the plain four-wave kernel: the larger of the solve's layout and the regression's work space (k1_smem_carve)
    static constexpr size_t lds_next = ldsm > (size_t)k1_smem_doubles<4>() * sizeof(double) ? ldsm : (size_t)k1_smem_doubles<4>() * sizeof(double);
    static constexpr auto mw4_next() { return lmpc_solve_kernel_mw<N, S, 4, false, lmpc_k1_next>; }

    static bool raise_limits() {
        if constexpr (has_mw) { if (!lmpc_raise_lds_limit((const void *)mw4_next(), lds_next)) return false; }
        if constexpr (use_abg) { if (!lmpc_raise_lds_limits(one_wave<false, true>())) return false; }
#ifdef LMPC_WITH_CD
        if constexpr (has_cd) { if (!lmpc_raise_lds_limit((const void *)lmpc_solve_kernel_cd<N, S>, lds_cd(true))) return false; }
#endif
        if constexpr (has_mw) { if (!(lmpc_raise_lds_limits(multi_wave<4>()) && lmpc_raise_lds_limits(multi_wave<2>()))) return false; }
        return lmpc_raise_lds_limits(one_wave<false>()) && lmpc_raise_lds_limits(one_wave<true>());
    }

    static int l1(hipStream_t st, const lmpc_dev_params &p, int B, const lmpc_solve_io &io, const int *live) {
        if constexpr (use_abg) { if (!(io.mode & 4) && io.abPack) return lmpc_launch_pair(one_wave<false, true>(), st, p, B, io, live); }
        return lmpc_launch_pair(one_wave<false>(lds_for(p, io)), st, p, B, io, live); }
    static int lr(hipStream_t st, const lmpc_dev_params &p, int B, const lmpc_solve_io &io, const int *live) { return lmpc_launch_pair(one_wave<true>(lds_for(p, io)), st, p, B, io, live); }
    static int l4(hipStream_t st, const lmpc_dev_params &p, int B, const lmpc_solve_io &io, const int *live) { return lmpc_launch_pair(multi_wave<4>(), st, p, B, io, live); }
    static int l2(hipStream_t st, const lmpc_dev_params &p, int B, const lmpc_solve_io &io, const int *live) { return lmpc_launch_pair(multi_wave<2>(), st, p, B, io, live); }
    static int l4n(hipStream_t st, const lmpc_dev_params &p, int B, const lmpc_solve_io &io, const lmpc_k1_next &nx) {
        const long long grid = lmpc_merged_grid(B, nx.B, p.N, k1_queries_per_block(nx.qg, p.trToUse, p.maxNumPoint));
        if constexpr (has_mw) { hipLaunchKernelGGL(mw4_next(), dim3((unsigned)grid), dim3(WAVE * 4), lds_next, st, p, B, io, nx); return 0; }
        return -1;
    }
    static int lc(hipStream_t st, const lmpc_dev_params &p, int B, const lmpc_solve_io &io, int hasQ) {
#ifdef LMPC_WITH_CD
        if constexpr (has_cd) { hipLaunchKernelGGL((lmpc_solve_kernel_cd<N, S>), dim3(B), dim3(WAVE), lds_cd(hasQ), st, p, B, io, hasQ); return 0; }
#endif
        (void)hasQ; return l1(st, p, B, io, nullptr);
    }
};

// fills the table and raises the kernels' dynamic-LDS limit; false if the device refuses (a one-wave footprint beyond 160 KB -- no supported (N, S) has one:
// the largest, N = 64 with 384 safe-set points, takes 108 KB).  An (N, S) whose multi-wave layout does not fit a CU (has_mw) gets lds_mw = 0 and the one-wave
// launcher in the multi-wave slots.
template <int N, int S> static bool lmpc_variant_fill(lmpc_variant_api *v) {
    static_assert(N >= 2 && N <= LMPC_MAX_N && S >= 0 && S <= LMPC_MAX_SS_POINTS, "unsupported variant");
    using L = lmpc_variant_launchers<N, S>;
    if (!L::raise_limits()) return false;
    v->N = N; v->S = S;
    v->lds_1w = L::lds1; v->lds_1w_abg = L::use_abg ? L::lds1g : 0; v->lds_cd = L::lds_cd(false); v->lds_cd_q = L::lds_cd(true);
    v->launch_1w = &L::l1; v->launch_retry = &L::lr; v->launch_cd = &L::lc;
    if constexpr (L::has_mw) {
        v->lds_mw = L::ldsm; v->launch_mw4 = &L::l4; v->launch_mw2 = &L::l2; v->launch_mw4_next = &L::l4n;
        int nb = 0; const auto m2 = L::template multi_wave<2>();
        v->occ_mw2 = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)m2.plain, m2.threads, m2.lds) == hipSuccess ? nb : 0;
    } else {
        v->lds_mw = 0; v->launch_mw4 = &L::l1; v->launch_mw2 = &L::l1; v->occ_mw2 = 0; v->launch_mw4_next = nullptr;
    }
    return true;
}

#ifndef LMPC_VARIANT_TU
// The runtime-(N, S) kernel behind the same table (lmpc_solve_rt.hip.h): one wave per QP whatever the batch size, no multi-wave / condensed / fused forms.
// false if the footprint of this (N, S) exceeds the LDS of a CU: N = 64 beyond 146 safe-set points (209 KB at 384), N = 40 beyond 366 -- only a fixed variant serves those.
static bool lmpc_variant_fill_rt(lmpc_variant_api *v, int N, int S) {
    if (N < 2 || N > LMPC_MAX_N || S < 0 || S > LMPC_MAX_SS_POINTS) return false;
    const size_t lds = (size_t)rt_layout(N, S).tot * sizeof(double);
    if (lds + 1024 > (size_t)160 * 1024) return false;
    for (const void *k : {(const void *)lmpc_rt_family<false>::plain, (const void *)lmpc_rt_family<false>::list, (const void *)lmpc_rt_family<true>::plain, (const void *)lmpc_rt_family<true>::list})
        if (!lmpc_raise_lds_limit(k, lds + LMPC_SSTAB_LDS)) return false;
    v->N = N; v->S = S; v->lds_mw = 0; v->lds_1w = lds; v->lds_1w_abg = 0; v->lds_cd = 0; v->lds_cd_q = 0; v->occ_mw2 = 0;
    v->launch_1w = &lmpc_rt_launch<false>; v->launch_retry = &lmpc_rt_launch<true>; v->launch_mw4 = &lmpc_rt_launch<false>; v->launch_mw2 = &lmpc_rt_launch<false>; v->launch_cd = &lmpc_rt_launch_cd; v->launch_mw4_next = nullptr;
    return true;
}
#endif
