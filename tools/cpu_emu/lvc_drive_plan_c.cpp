// Host build of the driven part of pyqed_amd/csrc/lvc_plan.hpp for tests/test_lvc_drive_plan_host.py and the GPU tests:
// the plan of qd_lvc_driven_rk4 as C functions.
#include "../../pyqed_amd/csrc/lvc_plan.hpp"

using namespace qd;

extern "C" {
// LVC_MAX_DRIVES, LVC_DRIVE_RESIDENT_MAX_D, LVC_DRIVE_LDS_MAX, LVC_TILE, LVC_RES_TPB, LVC_OBS_NV, sizeof(LvcPlan)
void plan_lvc_drive_constants(long* out) {
  const long c[] = {LVC_MAX_DRIVES, LVC_DRIVE_RESIDENT_MAX_D, (long)LVC_DRIVE_LDS_MAX, LVC_TILE,
                    LVC_RES_TPB,    LVC_OBS_NV,               (long)sizeof(LvcPlan)};
  std::copy(c, c + 7, out);
}
void plan_lvc_drive(const char* fn, long B, int nel, int M, const int* dims, int nd, const int* drive_mode, int sample,
                    int hold, long nf, int path, int nsteps, int save_every, int want_obs, LvcDrivePlan* out) {
  *out = lvc_drive_plan(fn, B, nel, M, dims, nd, drive_mode, sample, hold, nf, path, nsteps, save_every, want_obs != 0);
}
// the resident limit of a model with M modes
long plan_lvc_drive_limit(int M) { return lvc_drive_resident_limit(M); }
long plan_lvc_drive_row(int sample, int hold, long s, int stage) { return lvc_drive_row(sample, hold, s, stage); }
}
