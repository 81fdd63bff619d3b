// ldr.hip — conical-intersection dynamics in the local diabatic representation, matrix-free: qd_ldr_run.
//
// Replaces LDR2.run and LDRN.run of pyqed/ldr/ldr.py:1564-1611, 579-625, which materialise the electronic overlap
// A = U^+ U and exp_T = A * expKx * expKy as dense (npts ns)^2 arrays, by the factorisation of ldr_plan.hpp: expand
// with U, one dense mode product per axis, project with U^+.  This file is the host side only: pointer checks, the
// plan (ldr_plan.hpp decides what is admitted, the path, every grid and the scratch layout), scratch from the arena,
// and the launches.  Everything is stream-ordered and reads no host memory after the call returns.
//
// qd_ldr_jacobi_run is the same for LDR2_Jacobi (ldr.py:1779-1987), whose last-axis propagator differs for every row
// of the grid: two real-matrix passes along the last axis around a phase table (ldr_jacobi_plan).
#include "ldr_kernels.hpp"

namespace qd {
namespace {

dim3 grid_of(const LdrLaunch& l) { return dim3(l.gx, l.gy, l.gz); }

struct LdrArgs {
  const c128 *U, *expV, *K[LDR_MAX_DIM];
};

int ldr_axis(const LdrPlan& p, int d, const LdrArgs& t, const c128* in, c128* out, c128* snap, size_t snap_bstride,
             hipStream_t st) {
  const LdrAxis& a = p.axis[d];
  LdrPass k{};
  k.in = in;
  k.out = out;
  k.K = t.K[d];
  k.U = t.U;
  k.expV = t.expV;
  k.snap = snap;
  k.snap_bstride = snap_bstride;
  k.C = a.C;
  k.st = a.st;
  k.s = a.s;
  k.outer = a.outer;
  k.npts = (unsigned)p.npts;
  k.n = a.n;
  k.M = p.M;
  k.ns = p.ns;
  k.cu = a.cu;
  const dim3 g = grid_of(a.launch), b(a.launch.tpb);
  if (a.expand && a.project)
    hipLaunchKernelGGL((ldr_axis_kernel<true, true>), g, b, a.launch.lds, st, k);
  else if (a.expand)
    hipLaunchKernelGGL((ldr_axis_kernel<true, false>), g, b, a.launch.lds, st, k);
  else if (a.project)
    hipLaunchKernelGGL((ldr_axis_kernel<false, true>), g, b, a.launch.lds, st, k);
  else
    hipLaunchKernelGGL((ldr_axis_kernel<false, false>), g, b, a.launch.lds, st, k);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// The step loop of both entry points: the opening half step, then per step the expand kernel (split path), the plan's
// passes, launched by passes(buf, snapshot of the step or null, snap_bstride), and the project kernel (split path).
template <class Plan, class Passes>
int ldr_steps(const Plan& p, const c128* U, const c128* expV, const c128* psi, const c128* expVh, c128* snap,
              hipStream_t st, Passes passes) {
  void* w = nullptr;
  QD_TRY(workspace(WS_MISC, p.ws_total, &w, st));
  c128* state[2] = {(c128*)((char*)w + p.ws_psi0), (c128*)((char*)w + p.ws_psi1)};
  c128* work[2] = {(c128*)((char*)w + p.ws_w0), (c128*)((char*)w + p.ws_w1)};
  const size_t per = (size_t)p.npts * p.ns, npsi = (size_t)p.B * per, nchi = (size_t)p.B * p.npts * p.M;
  const size_t snap_bstride = (size_t)p.nsnap * per;
  const int nout = p.nrun / p.nsnap;
  hipLaunchKernelGGL(ldr_open_kernel, grid_of(p.open), dim3(p.open.tpb), 0, st, psi, expVh, state[0], per, npsi);
  QD_HIP(hipGetLastError());
  for (int s = 0; s < p.nrun; ++s) {
    const c128* cur = state[s & 1];
    c128* nxt = state[(s + 1) & 1];
    c128* sn = (s + 1) % nout == 0 ? snap + (size_t)((s + 1) / nout - 1) * per : nullptr;
    auto buf = [&](int b, bool dst) -> c128* {
      return b == LDR_BUF_PSI ? (dst ? nxt : (c128*)cur) : work[b - LDR_BUF_W0];
    };
    if (p.path == LDR_SPLIT) {
      hipLaunchKernelGGL(ldr_expand_kernel, grid_of(p.expand), dim3(p.expand.tpb), 0, st, cur, U,
                         buf(p.expand_dst, true), (size_t)p.npts, p.M, p.ns, nchi);
      QD_HIP(hipGetLastError());
    }
    QD_TRY(passes(buf, sn, snap_bstride));
    if (p.path == LDR_SPLIT) {
      hipLaunchKernelGGL(ldr_project_kernel, grid_of(p.project), dim3(p.project.tpb), 0, st,
                         (const c128*)buf(p.project_src, false), U, expV, nxt, sn, snap_bstride, (size_t)p.npts, p.M,
                         p.ns, npsi);
      QD_HIP(hipGetLastError());
    }
  }
  return QD_OK;
}

int ldr_run(const LdrPlan& p, const LdrArgs& t, const c128* psi, const c128* expVh, c128* snap, hipStream_t st) {
  return ldr_steps(p, t.U, t.expV, psi, expVh, snap, st, [&](auto buf, c128* sn, size_t snap_bstride) -> int {
    for (int d = 0; d < p.ndim; ++d)
      QD_TRY(ldr_axis(p, d, t, buf(p.axis[d].src, false), buf(p.axis[d].dst, true), sn, snap_bstride, st));
    return QD_OK;
  });
}

// ---- qd_ldr_jacobi_run: forward real pass (* ph), plain passes, back real pass (ldr_jacobi_plan)
struct LdrJacobiArgs {
  const c128 *U, *expV, *ph, *K[LDR_MAX_DIM];
  const double *F, *Fb;
};

int ldr_jacobi_pass(const LdrJacobiPlan& p, int i, const LdrJacobiArgs& t, const c128* in, c128* out, c128* snap,
                    size_t snap_bstride, hipStream_t st) {
  const LdrJacobiPass& a = p.pass[i];
  const dim3 g = grid_of(a.launch), b(a.launch.tpb);
  if (!a.real) {
    LdrPass k{};
    k.in = in;
    k.out = out;
    k.K = t.K[a.axis];
    k.C = a.C;
    k.st = a.st;
    k.s = a.s;
    k.outer = a.outer;
    k.npts = (unsigned)p.npts;
    k.n = a.n;
    k.M = p.M;
    k.ns = p.ns;
    k.cu = a.cu;
    hipLaunchKernelGGL((ldr_axis_kernel<false, false>), g, b, a.launch.lds, st, k);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
  LdrRealPass k{};
  k.in = in;
  k.out = out;
  k.F = a.phase ? t.F : t.Fb;
  k.ph = a.phase ? t.ph : nullptr;
  k.U = t.U;
  k.expV = t.expV;
  k.snap = snap;
  k.snap_bstride = snap_bstride;
  k.C = a.C;
  k.outer = a.outer;
  k.npts = (unsigned)p.npts;
  k.n = a.n;
  k.M = p.M;
  k.ns = p.ns;
  k.cu = a.cu;
  if (a.phase && a.expand)
    hipLaunchKernelGGL((ldr_real_axis_kernel<true, true, false>), g, b, a.launch.lds, st, k);
  else if (a.phase)
    hipLaunchKernelGGL((ldr_real_axis_kernel<false, true, false>), g, b, a.launch.lds, st, k);
  else if (a.project)
    hipLaunchKernelGGL((ldr_real_axis_kernel<false, false, true>), g, b, a.launch.lds, st, k);
  else
    hipLaunchKernelGGL((ldr_real_axis_kernel<false, false, false>), g, b, a.launch.lds, st, k);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

int ldr_jacobi_run(const LdrJacobiPlan& p, const LdrJacobiArgs& t, const c128* psi, const c128* expVh, c128* snap,
                   hipStream_t st) {
  return ldr_steps(p, t.U, t.expV, psi, expVh, snap, st, [&](auto buf, c128* sn, size_t snap_bstride) -> int {
    for (int i = 0; i < p.npass; ++i)
      QD_TRY(ldr_jacobi_pass(p, i, t, buf(p.pass[i].src, false), buf(p.pass[i].dst, true), sn, snap_bstride, st));
    return QD_OK;
  });
}

}  // namespace
}  // namespace qd

using namespace qd;

extern "C" int qd_ldr_jacobi_run(const qd_c128* psi, int B, int ndim, const int* dims, int M, int ns, const qd_c128* U,
                                 const qd_c128* expV, const qd_c128* expVh, const double* F, const double* Fb,
                                 const qd_c128* ph, const qd_c128* K0, const qd_c128* K1, int nsteps, int nout,
                                 qd_c128* snap, int path, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  const LdrJacobiPlan p = ldr_jacobi_plan("qd_ldr_jacobi_run", B, ndim, dims, M, ns, nsteps, nout, path);
  if (p.refused) {
    set_error("%s", p.msg);
    return QD_EINVAL;
  }
  QD_CHECK_ARG(psi && U && expV && expVh, "qd_ldr_jacobi_run: null psi, U, expV or expVh");
  QD_CHECK_ARG(F && Fb && ph, "qd_ldr_jacobi_run: null F, Fb or ph");
  LdrJacobiArgs t{(const c128*)U, (const c128*)expV, (const c128*)ph, {(const c128*)K0, (const c128*)K1, nullptr},
                  F, Fb};
  for (int d = 0; d < ndim - 1; ++d) QD_CHECK_ARG(t.K[d], "qd_ldr_jacobi_run: null K%d with ndim=%d", d, ndim);
  // no snapshot is due: nothing is launched and no path is noted, as in qd_ldr_run
  if (p.nsnap == 0) return QD_OK;
  QD_CHECK_ARG(snap, "qd_ldr_jacobi_run: null snap with %d snapshots due", p.nsnap);
  note_path(p.path == LDR_FUSED ? "ldr_jacobi_fused" : "ldr_jacobi_split");
  return ldr_jacobi_run(p, t, (const c128*)psi, (const c128*)expVh, (c128*)snap, st);
}

extern "C" int qd_ldr_run(const qd_c128* psi, int B, int ndim, const int* dims, int M, int ns, const qd_c128* U,
                          const qd_c128* expV, const qd_c128* expVh, const qd_c128* K0, const qd_c128* K1,
                          const qd_c128* K2, int nsteps, int nout, qd_c128* snap, int path, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  const LdrPlan p = ldr_plan("qd_ldr_run", B, ndim, dims, M, ns, nsteps, nout, path);
  if (p.refused) {
    set_error("%s", p.msg);
    return QD_EINVAL;
  }
  QD_CHECK_ARG(psi && U && expV && expVh, "qd_ldr_run: null psi, U, expV or expVh");
  LdrArgs t{(const c128*)U, (const c128*)expV, {(const c128*)K0, (const c128*)K1, (const c128*)K2}};
  for (int d = 0; d < ndim; ++d) QD_CHECK_ARG(t.K[d], "qd_ldr_run: null K%d with ndim=%d", d, ndim);
  // no snapshot is due: the reference computes nothing it keeps.  Nothing is launched, so no path is noted either
  if (p.nsnap == 0) return QD_OK;
  QD_CHECK_ARG(snap, "qd_ldr_run: null snap with %d snapshots due", p.nsnap);
  note_path(p.path == LDR_FUSED ? "ldr_axes_fused" : "ldr_axes_split");
  return ldr_run(p, t, (const c128*)psi, (const c128*)expVh, (c128*)snap, st);
}
