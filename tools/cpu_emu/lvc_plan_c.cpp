// Host build of pyqed_amd/csrc/lvc_plan.hpp for tests/test_lvc_plan_host.py and the GPU tests: the plan as C functions.
#include "../../pyqed_amd/csrc/lvc_plan.hpp"

using namespace qd;

extern "C" {
// LVC_MAX_NEL, LVC_MAX_MODES, LVC_TILE, LVC_RES_TPB, LVC_RESIDENT_MAX_D, LVC_OBS_MAX_GRID, LVC_OBS_NV,
// LVC_GRID_YZ_MAX, LVC_LDS_MAX, LVC_FLAT_GRID_MAX
void plan_lvc_constants(long* out) {
  const long c[] = {LVC_MAX_NEL,      LVC_MAX_MODES, LVC_TILE,        LVC_RES_TPB,       LVC_RESIDENT_MAX_D,
                    LVC_OBS_MAX_GRID, LVC_OBS_NV,    LVC_GRID_YZ_MAX, (long)LVC_LDS_MAX, LVC_FLAT_GRID_MAX};
  std::copy(c, c + 10, out);
}
void plan_lvc(const char* fn, long B, int nel, int M, const int* dims, int path, int nsteps, int save_every,
              int want_obs, LvcPlan* out) {
  *out = lvc_plan(fn, B, nel, M, dims, path, nsteps, save_every, want_obs != 0);
}
// the NEL the typed dispatch reaches, -1 when it reaches none
int plan_lvc_dispatch(int nel) {
  int hit = -1;
  dispatch_lvc_nel(nel, [&](auto N) {
    hit = decltype(N)::value;
    return true;
  });
  return hit;
}
}
