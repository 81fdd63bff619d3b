// Host build of the pair part of pyqed_amd/csrc/lvc_plan.hpp for tests/test_lvc_pair_plan_host.py and the GPU tests:
// the plan of qd_lvc_pair_observe and qd_lvc_pair_rk4 as C functions.
#include "../../pyqed_amd/csrc/lvc_plan.hpp"

using namespace qd;

extern "C" {
// LVC_PAIR_MAX, LVC_PAIR_RESIDENT_MAX_D, LVC_LDS_MAX, LVC_TILE, LVC_RES_TPB, LVC_PAIR_NV_MAX, LVC_PAIR_REG_NEL,
// LVC_OBS_MAX_GRID, sizeof(LvcPlan), sizeof(LvcPairPlan)
void plan_lvc_pair_constants(long* out) {
  const long c[] = {LVC_PAIR_MAX,     LVC_PAIR_RESIDENT_MAX_D, (long)LVC_LDS_MAX,     LVC_TILE,
                    LVC_RES_TPB,      LVC_PAIR_NV_MAX,         LVC_PAIR_REG_NEL,      LVC_OBS_MAX_GRID,
                    (long)sizeof(LvcPlan), (long)sizeof(LvcPairPlan)};
  std::copy(c, c + 10, out);
}
void plan_lvc_pair(const char* fn, long P, int nel, int M, const int* dims, int nblk, const int* blocks, int path,
                   int nsteps, int save_every, LvcPairPlan* out) {
  *out = lvc_pair_plan(fn, P, nel, M, dims, nblk, blocks, path, nsteps, save_every);
}
// the resident limit of a model with M modes
long plan_lvc_pair_limit(int M) { return lvc_pair_resident_limit(M); }
}
