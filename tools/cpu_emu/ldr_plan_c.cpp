// Host build of pyqed_amd/csrc/ldr_plan.hpp for tests/test_ldr_plan_host.py and the GPU tests: the plan as C functions.
#include "../../pyqed_amd/csrc/ldr_plan.hpp"

using namespace qd;

extern "C" {
// LDR_MAX_DIM, LDR_MAX_M, LDR_MAX_N, LDR_WAVES, LDR_TPB, LDR_SUB, LDR_RT, LDR_NSUB, LDR_CT, LDR_KT, LDR_BS_STRIDE,
// LDR_DS_STRIDE, LDR_FUSE_MIN_COLS, LDR_POINT_GRID_MAX, LDR_INDEX_MAX, LDR_LDS_MAX
void plan_ldr_constants(long* out) {
  const long c[] = {LDR_MAX_DIM, LDR_MAX_M,     LDR_MAX_N,     LDR_WAVES,         LDR_TPB,            LDR_SUB,
                    LDR_RT,      LDR_NSUB,      LDR_CT,        LDR_KT,            LDR_BS_STRIDE,      LDR_DS_STRIDE,
                    LDR_FUSE_MIN_COLS, LDR_POINT_GRID_MAX, LDR_INDEX_MAX, (long)LDR_LDS_MAX};
  std::copy(c, c + 16, out);
}
void plan_ldr(const char* fn, long B, int ndim, const int* dims, int M, int ns, int nsteps, int nout, int path,
              LdrPlan* out) {
  *out = ldr_plan(fn, B, ndim, dims, M, ns, nsteps, nout, path);
}
int plan_ldr_fusable(int M) { return M >= 1 && ldr_fusable(M) ? ldr_fused_cols(M) : 0; }
// qd_ldr_jacobi_run's plan (tests/test_ldr_jacobi_plan_host.py)
void plan_ldr_jacobi(const char* fn, long B, int ndim, const int* dims, int M, int ns, int nsteps, int nout, int path,
                     LdrJacobiPlan* out) {
  *out = ldr_jacobi_plan(fn, B, ndim, dims, M, ns, nsteps, nout, path);
}
int plan_ldr_jacobi_max_pass() { return LDR_JACOBI_MAX_PASS; }
}
