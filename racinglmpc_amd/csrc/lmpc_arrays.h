// racinglmpc_amd/csrc/lmpc_arrays.h -- the per-problem arrays one step moves, stated once: name, element type, elements per problem, role.
// Host side only (lmpc_capi.hip) and plain C++: no HIP header is needed, tests/test_host_checks.py compiles the slab layout with g++.
// Everything that allocates, copies, zeroes or hands these arrays to a kernel walks this list (lmpc_arrays_each) instead of naming them again.
#pragma once
#include <cstddef>

enum { LMPC_ARR_IN = 0, LMPC_ARR_OUT = 1, LMPC_ARR_SEL = 2 };     // step input | step output | output of the selection alone (lmpc_select_batch, regression status)

// X(name, type, elements per problem, role).  N: horizon; S: safe-set points in use (0 when numSS_it == 0); L: numSS_it; M = 8 N + S inequality rows.
// The order is the order of the ranges in the context's two slabs (inputs | everything else); the first 24 names are the members of lmpc_step_dev_args.
#define LMPC_STEP_ARRAYS(X) \
    X(x0, double, 6, IN) X(xLin, double, (N + 1) * 6, IN) X(uLin, double, N * 2, IN) X(uOld, double, 2, IN) \
    X(zt, double, 6, IN) X(xPredPrev, double, (N + 1) * 6, IN) X(hasPred, int, 1, IN) X(timeStep, int, 1, IN) \
    X(xPred, double, (N + 1) * 6, OUT) X(uPred, double, N * 2, OUT) X(slack, double, N * 2, OUT) X(lambda, double, S, OUT) \
    X(sTerm, double, 6, OUT) X(ztNext, double, 6, OUT) X(ztuNext, double, 2, OUT) X(ssSel, double, S * 6, OUT) \
    X(qSel, double, S, OUT) X(mu, double, M, OUT) X(A, double, N * 36, OUT) X(Bm, double, N * 12, OUT) \
    X(C, double, N * 6, OUT) X(status, int, 1, OUT) X(iters, int, 1, OUT) X(resid, double, 3, OUT)
#define LMPC_SELECT_ARRAYS(X) \
    X(succ, double, S * 6, SEL) X(succU, double, S * 2, SEL) X(ztUsed, double, 6, SEL) X(rstatus, int, N, SEL) X(selStart, int, (L > 0 ? L : 1), SEL)
#define LMPC_ARRAYS(X) LMPC_STEP_ARRAYS(X) LMPC_SELECT_ARRAYS(X)

// one pointer per array: the context's work buffers, their host-mapped mirrors, a caller's host arrays, a rollout session's buffers
struct lmpc_arrays {
#define X(name, type, count, role) type *name;
    LMPC_ARRAYS(X)
#undef X
};
struct lmpc_dims { size_t N, S, L; };                              // S as the context defines it: numSS_it > 0 ? numSS_points : 0
// the 24 arrays of a step out of `s` (an lmpc_arrays, or the lmpc_step_dev_args of include/lmpc_hip.h: same member names); the selection-only arrays stay NULL, a step does not write them
template <class T> inline lmpc_arrays lmpc_step_arrays(const T &s) {
    lmpc_arrays a = {};
#define X(name, type, count, role) a.name = (type *)s.name;
    LMPC_STEP_ARRAYS(X)
#undef X
    return a;
}

// f(name, &lmpc_arrays::member, bytes per element, elements per problem, role) for every array, in slab order; expanded at compile time, no table is read at run time
template <class F> inline void lmpc_arrays_each(const lmpc_dims &d, F &&f) {
    const size_t N = d.N, S = d.S, L = d.L, M = 8 * N + S;
    (void)L; (void)M;
#define X(name, type, count, role) f(#name, &lmpc_arrays::name, sizeof(type), (size_t)(count), (int)LMPC_ARR_##role);
    LMPC_ARRAYS(X)
#undef X
}
// is `m` (as lmpc_arrays_each hands it out) this member?  Members of another element type compare unequal instead of failing to compile.
template <class A, class B> inline bool lmpc_is(A, B) { return false; }
template <class A> inline bool lmpc_is(A m, A member) { return m == member; }

// Slab layout of a context of B problems: f(name, member, slab (0 inputs, 1 outputs), byte offset, bytes) per array; total[slab] = bytes of the slab.
// Every range holds at least one element and is rounded up to 256 bytes; `gap` bytes follow every range (the guard zones of -DLMPC_GUARD builds, else 0).
template <class F> inline void lmpc_slab_layout(const lmpc_dims &d, size_t B, size_t gap, size_t total[2], F &&f) {
    total[0] = total[1] = 0;
    lmpc_arrays_each(d, [&](const char *name, auto m, size_t elem, size_t n, int role) {
        const int slab = role == LMPC_ARR_IN ? 0 : 1;
        const size_t elems = B * n > 1 ? B * n : 1, bytes = (elems * elem + 255) & ~(size_t)255;
        f(name, m, slab, total[slab], bytes);
        total[slab] += bytes + gap;
    });
}
