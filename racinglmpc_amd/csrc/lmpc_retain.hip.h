// racinglmpc_amd/csrc/lmpc_retain.hip.h -- the device side of lmpc_store_retain: the kept laps of both stores gathered into fresh allocations.
// Out of place: the destination buffers are new, zero-filled allocations of the new lap capacity (the same row stride), so the peak is OLD + NEW device memory until
// the old buffers are freed, and a failure on the way leaves the old ones in force.  One launch covers both stores: one 256-thread work-group per (store, kept lap),
// driven by an uploaded table.  A safe-set lap is its 9 columns x rows; a regression-store lap also its prefilter image, 3 planes x (rows - 1) words and 6 parameters
// per chunk in use (lmpc_commit.hip.h: commit_quantise).  Behind a lap's rows the destination stays zero, as in a store the lap was committed to directly.
// Everything is copied as integer words: every bit survives, NaN payloads and the sign of a zero included.
// The copy is memory-bound and contiguous per column; a lane moves 16 bytes per access where source and destination are both 16-byte aligned -- a column starts at
// (lap * 9 + column) * max_lap_len doubles, so with an odd max_lap_len only every other column is -- 8 bytes where both are 8-byte aligned, else 4.
// Included by lmpc_capi.hip only, after the kernels' header (K1_CHUNK, LMPC_COLS).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define LMPC_RETAIN_NT 256

struct lmpc_retain_entry { int store, src, dst, rows; };                 // store: 0 regression store (with its image), 1 safe set; src / dst: lap slots; rows the lap holds
struct lmpc_retain_args {
    const double *src_store[2]; double *dst_store[2];                   // [0] regression store, [1] safe set
    const unsigned *src_quant; unsigned *dst_quant; const double *src_qpar; double *dst_qpar;
    int ls, mq_chunks;                                                  // row stride of every column (max_lap_len) and chunks the image holds per lap: the same on both sides
};

// n 32-bit words from src to dst by the whole work-group, in the widest access both addresses allow; the tail of a wide pass (at most 3 words) goes word by word
__device__ __forceinline__ void retain_copy_words(unsigned *__restrict__ dst, const unsigned *__restrict__ src, size_t n) {
    const uintptr_t both = (uintptr_t)dst | (uintptr_t)src;
    const size_t tid = threadIdx.x;
    size_t done = 0;
    if ((both & 15) == 0) {
        const uint4 *s = (const uint4 *)src; uint4 *d = (uint4 *)dst;
        for (size_t i = tid; i < n / 4; i += LMPC_RETAIN_NT) d[i] = s[i];
        done = n / 4 * 4;
    } else if ((both & 7) == 0) {
        const uint2 *s = (const uint2 *)src; uint2 *d = (uint2 *)dst;
        for (size_t i = tid; i < n / 2; i += LMPC_RETAIN_NT) d[i] = s[i];
        done = n / 2 * 2;
    }
    for (size_t i = done + tid; i < n; i += LMPC_RETAIN_NT) dst[i] = src[i];
}

__global__ void __launch_bounds__(LMPC_RETAIN_NT) lmpc_retain_laps_kernel(lmpc_retain_args a, const lmpc_retain_entry *__restrict__ table) {
    const lmpc_retain_entry e = table[blockIdx.x];
    const size_t ls = (size_t)a.ls;
    const double *sb = a.src_store[e.store] + (size_t)e.src * LMPC_COLS * ls;
    double *db = a.dst_store[e.store] + (size_t)e.dst * LMPC_COLS * ls;
    for (int j = 0; j < LMPC_COLS; j++)
        retain_copy_words((unsigned *)(db + (size_t)j * ls), (const unsigned *)(sb + (size_t)j * ls), 2 * (size_t)e.rows);
    if (e.store != 0) return;
    const int nrows = e.rows - 1, used = (nrows + K1_CHUNK - 1) / K1_CHUNK;      // (a regression-store lap has at least two rows)
    if (nrows <= 0) return;
    for (int pl = 0; pl < 3; pl++)
        retain_copy_words(a.dst_quant + ((size_t)e.dst * 3 + pl) * ls, a.src_quant + ((size_t)e.src * 3 + pl) * ls, (size_t)nrows);
    retain_copy_words((unsigned *)(a.dst_qpar + (size_t)e.dst * a.mq_chunks * 6), (const unsigned *)(a.src_qpar + (size_t)e.src * a.mq_chunks * 6), 2 * 6 * (size_t)used);
}
