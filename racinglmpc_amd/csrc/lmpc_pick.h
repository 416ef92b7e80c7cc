// racinglmpc_amd/csrc/lmpc_pick.h -- run-time flags into compile-time ones, for the host side of a kernel launch: lmpc_pick(f, a, b, ...) calls f with one std::bool_constant
// per flag, in order, and hands f's result through.  f names the kernel template once and leaves out (`if constexpr`) a combination that has no kernel.  Plain C++ like lmpc_rows.h.
#pragma once
#include <type_traits>

template <class F, class... Rest> decltype(auto) lmpc_pick(F &&f, bool a, Rest... rest) {
    if constexpr (sizeof...(Rest) == 0) { if (a) return f(std::true_type{}); else return f(std::false_type{}); }
    else if (a) return lmpc_pick([&](auto... c) -> decltype(auto) { return f(std::true_type{}, c...); }, rest...);
    else return lmpc_pick([&](auto... c) -> decltype(auto) { return f(std::false_type{}, c...); }, rest...);
}
