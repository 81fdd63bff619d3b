// typed_dispatch.hpp — a run-time value to a compile-time one (plain C++17, no HIP): what the plans' typed dispatches
// (spo_plan.hpp dispatch_pass, deom_plan.hpp dispatch_stage / dispatch_band) are built from.
#pragma once

#include <type_traits>

namespace qd {

// f(std::integral_constant<int, V>{}) for the V of the list that equals v; false when v is not in the list or f
// returns false (a miss is the caller's internal error, never a silent no-op).
template <int... Vs, typename F>
bool dispatch_int(int v, F&& f) {
  return ((v == Vs && f(std::integral_constant<int, Vs>{})) || ...);
}
template <int V>
using int_c = std::integral_constant<int, V>;

}  // namespace qd
