// Host build of pyqed_amd/csrc/fft_plan.hpp for tests/test_fft_plan_host.py: the plans as C functions.
#include "../../pyqed_amd/csrc/fft_plan.hpp"

using namespace qd::spog;

extern "C" {
void plan_fft_axis(int L, AxisPlan* out) { *out = axis_plan(L); }
int plan_fourstep_split(int L, int allow_bluestein) { return fourstep_split(L, allow_bluestein != 0); }
void plan_fft_lines(long O, int L, long I, LinesPlan* out) { *out = fft_lines_plan(O, L, I); }
void plan_fft_pass(const AxisPlan* ax, long O, long I, int ns, int rows, PassPlan* out) {
  *out = pass_plan(*ax, O, I, ns, rows != 0);
}
void plan_nd_layout(const int* n, int D, int ns, int nsteps, NdLayout* out) {
  AxisPlan ax[3];
  for (int d = 0; d < D; ++d) ax[d] = axis_plan(n[d]);
  *out = nd_layout(ax, D, n, ns, nsteps);
}
// The passes of a run in order, at most cap of them written; returns their number.
int plan_step_sequence(int D, int nsteps, int nout, int snaps, int merged, int ky, StepPass* out, int cap) {
  int k = 0;
  step_sequence(D, nsteps, nout, snaps != 0, merged != 0, ky != 0, [&](const StepPass& s) {
    if (k < cap) out[k] = s;
    ++k;
    return 0;
  });
  return k;
}
// out[i] = fdiv(x[i], make_fdiv(d))
void plan_fdiv(unsigned d, const unsigned* x, int n, unsigned* out) {
  const FDiv D = make_fdiv(d);
  for (int i = 0; i < n; ++i) out[i] = fdiv(x[i], D);
}
}
