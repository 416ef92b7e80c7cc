// racinglmpc_amd/csrc/lmpc_rows.h -- the per-car row sets of a context (vehicle constants, regression laps, safe-set laps, tuning, tracks), their contract stated once.
// A set keeps n rows of a fixed width as the caller gave them.  0 rows: the config's value.  One row serves every problem (device stride 0).  n rows: problem b reads row b,
// and a call of another count is refused before anything is queued (fits; lmpc_capi.hip: rows_fit).  Plain C++ like lmpc_arrays.h: tests/test_row_sets_host.py compiles it with g++.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

// B against n rows.  EXACT: B == n (lap table, safe-set table, tuning, tracks).  AT_LEAST: B <= n, "the first B of the n rows" (the plant rows).
enum lmpc_row_rule { LMPC_ROWS_EXACT = 0, LMPC_ROWS_AT_LEAST = 1 };

template <class T> struct lmpc_row_set {
    std::vector<T> rows; int n, width; const char *setter;          // setter: the entry point that fills the set, named in refusals
    explicit lmpc_row_set(int width_ = 0, const char *setter_ = "") : n(0), width(width_), setter(setter_) {}
    bool in_force() const { return n > 0; }
    const T *row(int b) const { return rows.data() + (size_t)(n == 1 ? 0 : b) * (size_t)width; }
    int stride(int image_width) const { return n <= 1 ? 0 : image_width; }      // of a device image of image_width elements per row
    bool fits(long long B, lmpc_row_rule rule) const { return n <= 1 || (rule == LMPC_ROWS_EXACT ? B == n : B <= n); }
    void assign(int n_, const T *src) { rows.assign(src, src + (size_t)n_ * (size_t)width); n = n_; }
    void clear() { rows.clear(); n = 0; }
    // the rows in force: *n_out rows exist, the first min(capacity, n) of them go to `out` (NULL: the count alone)
    void get(int *n_out, T *out, int capacity) const {
        *n_out = n;
        if (out && n > 0 && capacity > 0) std::copy(rows.begin(), rows.begin() + (size_t)std::min(capacity, n) * (size_t)width, out);
    }
    // one row per car out of an image of this set (image_width elements per row; the rows themselves: rows.data(), width): the single row repeated, else row b for car b
    template <class U> void expand(int B, U *out, const U *image, size_t image_width) const {
        for (int b = 0; b < B; b++) { const U *src = image + (size_t)(n == 1 ? 0 : b) * image_width; std::copy(src, src + image_width, out + (size_t)b * image_width); }
    }
};
