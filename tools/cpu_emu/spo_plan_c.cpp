// Host build of pyqed_amd/csrc/spo_plan.hpp for tests/test_spo_plan_host.py: the plans as C functions.  Each returns
// whether the specialised kernels take the shape and fills `out` with the planned passes.
#include "../../pyqed_amd/csrc/spo_plan.hpp"

using namespace qd;

extern "C" {
int plan_spo2(int nx, int ny, int ns, int jacobi, Pass* out /*[3]: row, row with k_y, column*/) {
  const SpoPlan p = spo2_plan(nx, ny, ns, jacobi != 0);
  if (p.special) out[0] = p.row[0], out[1] = p.row[1], out[2] = p.col;
  return p.special;
}
int plan_spo2_batch(int nx, int ny, int ns, int B, int jacobi, int observed, Pass* out /*[2]: row, column*/) {
  const SpoPlan p = spo2_batch_plan(nx, ny, ns, B, jacobi != 0, observed != 0);
  if (p.special) out[0] = p.row[0], out[1] = p.col;
  return p.special;
}
int plan_spo3(int nx, int ny, int nz, int ns, Pass* out /*[3]: row, mid, column*/) {
  const SpoPlan p = spo3_plan(nx, ny, nz, ns);
  if (p.special) out[0] = p.row[0], out[1] = p.mid, out[2] = p.col;
  return p.special;
}
int plan_spo1d(int nx, int B, Pass* out) { return spo1d_plan(nx, B, out); }
// 1 when dispatch_pass reaches a kernel for the pass
int plan_dispatch_hits(const Pass* p) {
  return dispatch_pass(*p, [](auto, auto, auto, auto) { return true; });
}
void plan_pass_name(const Pass* p, const char* prefix, char* buf, int n) { pass_name(*p, prefix, buf, (size_t)n); }
}
