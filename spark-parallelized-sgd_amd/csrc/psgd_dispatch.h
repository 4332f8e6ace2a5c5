// psgd_dispatch.h -- a runtime value to a compile-time one over a listed set: how every chain
// launcher (launch_<family>) maps the fields of its ChainPlan to a template instance. The lists
// are the set of built instances: a value outside them is an error, never another kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace psgd {

// f(std::integral_constant<int, V>{}) for the first listed value that equals v; f returns int.
// hipErrorInvalidValue when v is not listed. The instances are emitted into the code object in
// list order, outer lists first: the launchers list f32 before f64 and nest as their kernels'
// template parameters do, which keeps each object's kernels in a stable order.
template <int V, int... Vs, typename F>
int dispatch_int(int v, F&& f) {
    if (v == V) return f(std::integral_constant<int, V>{});
    if constexpr (sizeof...(Vs) > 0) return dispatch_int<Vs...>(v, f);
    else return (int)hipErrorInvalidValue;
}

// f(std::true_type{}) or f(std::false_type{}).
template <typename F>
int dispatch_bool(bool v, F&& f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}

// Row storage / arithmetic type of the code 0 = f64, 1 = f32 (psgd_internal.h).
template <int CODE>
using FloatOf = std::conditional_t<CODE == 1, float, double>;

}  // namespace psgd
