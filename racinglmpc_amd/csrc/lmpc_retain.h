// racinglmpc_amd/csrc/lmpc_retain.h -- the books of lmpc_store_retain (a lap store cut down to the laps its caller still reads), stated once: what a keep list must
// look like, the map from old to new lap indices, and what becomes of everything that names a lap by its index -- the per-lap vectors, the regression store's sorted
// order, the rows of a lap table, a `last` column, the selection override.  The k-th kept lap gets index k, so the map is monotone: relative order, and with it every
// "ties by index" rule, survives.  Plain C++ like lmpc_rows.h: tests/test_store_retain_host.py compiles it with g++.
#pragma once
#include <cstddef>
#include <vector>

// A keep list of a store that holds `stored` laps: n >= 0 strictly ascending indices in [0, stored).  Returns -1 for a good list, else the position of the first
// entry that breaks the rule; *why (if given): 0 out of range, 1 not above its predecessor.
inline int lmpc_retain_check(int n, const int *keep, int stored, int *why = nullptr) {
    for (int k = 0; k < n; k++) {
        if (keep[k] < 0 || keep[k] >= stored) { if (why) *why = 0; return k; }
        if (k > 0 && keep[k] <= keep[k - 1]) { if (why) *why = 1; return k; }
    }
    return -1;
}
// map[old] = the new index of lap `old`, -1 for a dropped one (the list has passed lmpc_retain_check)
inline std::vector<int> lmpc_retain_map(int n, const int *keep, int stored) {
    std::vector<int> map((size_t)stored, -1);
    for (int k = 0; k < n; k++) map[(size_t)keep[k]] = k;
    return map;
}
// the map of a store that is left untouched
inline std::vector<int> lmpc_retain_identity(int stored) {
    std::vector<int> map((size_t)stored);
    for (int k = 0; k < stored; k++) map[(size_t)k] = k;
    return map;
}
inline bool lmpc_retain_keeps_all(const std::vector<int> &map) { return map.empty() || map.back() == (int)map.size() - 1; }   // (monotone: the last lap is at its place only if every lap is)
inline int lmpc_retain_kept(const std::vector<int> &map) { int n = 0; for (int m : map) n += m >= 0; return n; }
// a per-lap vector of the kept laps, in their new order
template <class T> std::vector<T> lmpc_retain_gather(const std::vector<T> &v, const std::vector<int> &map) {
    std::vector<T> out;
    for (size_t old = 0; old < map.size(); old++) if (map[old] >= 0) out.push_back(v[old]);
    return out;
}
// the regression store's sorted order (sorted position -> lap) among the kept laps, under their new indices: the positions keep their relative order
inline std::vector<int> lmpc_retain_order(const std::vector<int> &order, const std::vector<int> &map) {
    std::vector<int> out;
    for (int lap : order) if (map[(size_t)lap] >= 0) out.push_back(map[(size_t)lap]);
    return out;
}
// Indices that name laps -- rows of a table, a `last` column, the override.  A negative entry is a sentinel ("none", LMPC_SS_LAST_SHARED) and names no lap.
// Returns -1 when every lap named is kept, else the position of the first entry whose lap is not (an index beyond the store names a lap that is not kept either).
inline long long lmpc_retain_first_dropped(const int *idx, size_t count, const std::vector<int> &map) {
    for (size_t i = 0; i < count; i++)
        if (idx[i] >= 0 && (idx[i] >= (int)map.size() || map[(size_t)idx[i]] < 0)) return (long long)i;
    return -1;
}
// the same indices under the new numbering, sentinels passed through (lmpc_retain_first_dropped has returned -1 for them)
inline void lmpc_retain_remap(int *idx, size_t count, const std::vector<int> &map) {
    for (size_t i = 0; i < count; i++) if (idx[i] >= 0) idx[i] = map[(size_t)idx[i]];
}
// the lap capacity after a retain: the smallest initial * 2^j (j >= 0) that holds `need` laps -- what growth from the initial capacity would have reached
inline int lmpc_retain_capacity(int initial, int need) {
    long long cap = initial;
    while (cap < need) cap *= 2;
    return (int)cap;
}
