// Host build of pyqed_amd/csrc/deom_plan.hpp for tests/test_deom_plan_host.py: the plans as C functions.
#include "../../pyqed_amd/csrc/deom_plan.hpp"

using namespace qd;

extern "C" {
void plan_deom_stage(int B, int nmax, int K, int ns, int nmod, int bminor, int horner, StagePlan* out) {
  *out = deom_stage_plan(B, nmax, K, ns, nmod, bminor, horner);
}
void plan_deom_band(int ns, int K, int nmod, int max_own, int max_loc, BandPlan* out) {
  *out = deom_band_plan(ns, K, nmod, max_own, max_loc);
}
// 1 when the typed dispatch reaches a kernel for the plan; out[7] / out[5] then hold the compile-time values it
// reached (kind, G, KMAX, NS2, UNI, HM, NM / G, KMAX, NS2, TPB, FAST), which the caller compares with the plan's.
int plan_deom_stage_hits(const StagePlan* p, int* out) {
  return dispatch_stage(*p, [&](auto k) {
    using T = decltype(k);
    const int v[7] = {T::kind, T::G, T::KMAX, T::NS2, T::UNI, T::HM, T::NM};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
    return true;
  });
}
int plan_deom_band_hits(const BandPlan* p, int* out) {
  return dispatch_band(*p, [&](auto k) {
    using T = decltype(k);
    const int v[5] = {T::G, T::KMAX, T::NS2, T::TPB, T::FAST};
    for (int i = 0; i < 5; ++i) out[i] = v[i];
    return true;
  });
}
}
