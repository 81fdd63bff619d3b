// response.hip — Liouville-space response functions on the (t1, t2, t3) grid.
//
// Eigen (sum-over-states) form of the reference's SOS propagator
// (pyqed/oqs.py:160-214: eig(R), U = U1 diag(e^{lam t}) U1^-1, G = -iU) and of
// correlation_4op_3t (oqs.py:268-357):
//   S[i,j,k] = <<I| a G(tau_i) b G(tau_j) c G(tau_k) d |rho0>>
//            = (-i)^3 sum_pqr alpha_p e^{lam_p tau_i} B_pq e^{lam_q tau_j} C_qr e^{lam_r tau_k} beta_r
// with alpha = I^T a U1, B = U1^-1 b U1, C = U1^-1 c U1, beta = U1^-1 d rho0
// (host-side setup, like the reference's eig).  Kernels:
//   qd_sos_propagator     U[a][b][k]                  (oqs.py:210 contraction)
//   qd_response_cube      S[i][j][k], full n^3 cube   (oqs.py:339-357 tensordots)
//   qd_response2d_ensemble  sum over M disorder members of the (t3, t1) slice at
//                         fixed t2 — one complex GEMM
//                           S = X [n3 x K] * Z [K x n1],  K = M * nL,
//                           X[i][m*nL+p] = i * alpha_mp e^{lam_mp t3_i}
//                           Z[m*nL+p][k] = sum_q Mt_mpq beta_mq e^{lam_mq t1_k},
//                           Mt_m = B_m diag(e^{lam_m t2}) C_m  (host)
//                         run split-K over workgroups on the MFMA block engine
//                         with a deterministic slab reduction.
// This file is the host side: argument checks, scratch, and the launches that response_plan.hpp lists.  The kernels
// are in response_kernels.hpp and ens_kernels.hpp.
#include "ens_kernels.hpp"

namespace qd {
namespace {

static_assert(ENS_KT == CG_KT && ENS_GEMM_TPB == CG_WG, "response_plan.hpp plans for the block engine's K-tile and workgroup");

// What the operand builds of a plan read and write.  The fixed-t2 ensemble fills the X and Z sides; the scan's
// operands fill the P side and the Z side (Q = C_m Y_m is the uniform Z build with Mt := C and no X blocks).
struct BuildArgs {
  EnsDims d;
  int M;
  // X side: nL eigen indices per member, t3 an array or t3_0 + i dt3; tables: coarse at X, then fine
  const c128 *alpha, *lam;
  int nL;
  const double* t3;
  double t3_0, dt3;
  int n3;
  c128 *X, *fine;
  // Z side: Mt [M][nL][nz], t1 an array or t1_0 + k dt1
  const c128 *Mt, *beta, *lamz;
  int nz;
  const double* t1;
  double t1_0, dt1;
  int n1;
  c128* Z;
  // P side: P_m = X_m B_m over np x nr indices (nr is the Z side's nL)
  const c128 *palpha, *Bm, *lamp;
  int np;
  double p_0, dp;
  c128* P;
};

// One operand-build launch of a plan.
int launch_build(const RespLaunch& l, const BuildArgs& a, hipStream_t st) {
  const EnsDims& d = a.d;
  const dim3 g(l.gx, l.gy), b(ENS_TPB);
  if (l.note) note_path(l.note);
  switch (l.kernel) {
    case RK_XTAB:
      hipLaunchKernelGGL(ens_xtab_kernel, g, b, 0, st, a.alpha, a.lam, d.K, d.Kp, a.t3_0, a.dt3, a.n3, d.n3p, a.X,
                         a.fine);
      break;
    case RK_Z_UNIFORM:
      hipLaunchKernelGGL(ens_z_uniform_kernel, g, b, l.lds, st, a.Mt, a.beta, a.lamz, l.M, a.nL, a.nz, l.G, a.t1_0,
                         a.dt1, a.n1, d.n1p, a.Z, a.alpha, a.lam, d.K, d.Kp, a.t3_0, a.dt3, a.n3, d.n3p, l.xbx, a.X);
      break;
    case RK_X_UNIFORM:
      hipLaunchKernelGGL(ens_x_uniform_kernel, g, b, 0, st, a.alpha, a.lam, d.K, d.Kp, a.t3_0, a.dt3, a.n3, d.n3p,
                         l.xbx, a.X);
      break;
    case RK_Z_PAD:
      hipLaunchKernelGGL(ens_z_pad_kernel, g, b, 0, st, d.K, d.Kp, d.n1p, a.Z);
      break;
    case RK_XZ:
      hipLaunchKernelGGL(ens_xz_kernel, g, b, 0, st, a.Mt, a.beta, a.lam, l.M, a.nL, a.t1, a.n1, d.n1p, d.Kp, a.Z,
                         a.alpha, a.t3, a.n3, d.n3p, l.xrows, d.K, a.X, a.nz, a.lamz);
      break;
    case RK_Z_GENERIC:
      hipLaunchKernelGGL(ens_z_generic_kernel, g, b, 0, st, a.Mt, a.beta, a.lamz, a.M, a.nL, a.t1, a.n1, d.n1p, d.Kp,
                         a.Z, a.nz);
      break;
    case RK_P_UNIFORM:
      hipLaunchKernelGGL(ens_p_uniform_kernel, g, b, 0, st, a.palpha, a.Bm, a.lamp, a.M, a.np, a.nL, a.p_0, a.dp,
                         a.n3, d.n3p, d.Kp, a.P);
      break;
    case RK_P_PAD:
      hipLaunchKernelGGL(ens_p_pad_kernel, g, b, 0, st, d.K, d.Kp, d.n3p, a.P);
      break;
    default:
      QD_CHECK_ARG(false, "response: internal: kernel %d is no operand build", l.kernel);
  }
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// slabs[s] = A [Mp][Kp] * B [Kp][Np] over K-tile range s of S, on the planned ens_gemm_kernel.  fine != nullptr: A is
// the coarse table of ens_xtab_kernel (generated A operand).
int launch_ens_gemm(const GemmPlan& pl, const c128* A, int Kp, const c128* B, int Mp, int Np, c128* slabs,
                    hipStream_t st, const c128* fine = nullptr) {
  note_path(pl.name);
  const bool hit = dispatch_ens_gemm(pl, [&](auto k) {
    using T = decltype(k);
    hipLaunchKernelGGL((ens_gemm_kernel<T::BT, T::XTAB, T::DEPTH>), dim3(pl.gx, pl.gy, pl.gz), dim3(CG_WG), 0, st, A,
                       Kp, B, Np, Kp / CG_KT, pl.S, slabs, Mp, fine);
    return true;
  });
  QD_CHECK_ARG(hit, "response: internal: no ens_gemm_kernel for BT=%d XTAB=%d DEPTH=%d", pl.bt, pl.xtab, pl.depth);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// out (+)= the slabs summed in order, plain (n3 x n1) or transposed (n1 x n3)
int launch_reduce(const RespLaunch& l, const c128* slabs, int S, int n3, int n1, int n3p, int n1p, c128* out,
                  int accumulate, hipStream_t st) {
  if (l.kernel == RK_REDUCE_TRANS)
    hipLaunchKernelGGL(ens_reduce_trans_kernel, dim3(l.gx, l.gy), dim3(ENS_TPB), 0, st, slabs, S, n3, n1, n3p, n1p, out,
                       accumulate);
  else
    hipLaunchKernelGGL(ens_reduce_kernel, dim3(l.gx), dim3(ENS_TPB), 0, st, slabs, S, n3, n1, n3p, n1p, out,
                       accumulate);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

}  // namespace
}  // namespace qd

using namespace qd;

extern "C" int qd_sos_propagator(const qd_c128* U1, const qd_c128* U2, const qd_c128* lam, int nL, const double* t,
                                 int nt, qd_c128* U, void* stream) {
  QD_CHECK_ARG(U1 && U2 && lam && t && U, "qd_sos_propagator: null pointer");
  QD_CHECK_ARG(nL >= 1 && nt >= 1, "qd_sos_propagator: nL=%d nt=%d must be >= 1", nL, nt);
  const size_t tot = (size_t)nL * nL * nt;
  hipLaunchKernelGGL(sos_propagator_kernel, dim3(flat_grid(tot)), dim3(256), 0, (hipStream_t)stream,
                     (const c128*)U1, (const c128*)U2, (const c128*)lam, nL, t, nt, (c128*)U);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

extern "C" int qd_response_cube(const qd_c128* alpha, const qd_c128* B, const qd_c128* C, const qd_c128* beta,
                                const qd_c128* lam, int nL, const double* t3, int n3, const double* t2, int n2,
                                const double* t1, int n1, qd_c128* out, void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(alpha && B && C && beta && lam && t3 && t2 && t1 && out, "qd_response_cube: null pointer");
  QD_CHECK_ARG(nL >= 1 && nL <= 4096 && n3 >= 1 && n2 >= 1 && n1 >= 1, "qd_response_cube: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  void* w = nullptr;
  const size_t ny = (size_t)n1 * nL, nw = (size_t)n2 * nL * n1;
  int rc = workspace(WS_2DES, (ny + nw) * sizeof(c128), &w, st);
  if (rc) return rc;
  c128* Y = (c128*)w;
  c128* W = Y + ny;
  hipLaunchKernelGGL(cube_y_kernel, dim3(flat_grid(ny)), dim3(256), 0, st, (const c128*)C, (const c128*)beta,
                     (const c128*)lam, nL, t1, n1, Y);
  QD_HIP(hipGetLastError());
  hipLaunchKernelGGL(cube_w_kernel, dim3(flat_grid(nw)), dim3(256), 0, st, (const c128*)B, Y, (const c128*)lam,
                     nL, t2, n2, n1, W);
  QD_HIP(hipGetLastError());
  QD_CHECK_ARG((size_t)n3 * n2 < (1u << 31), "qd_response_cube: n3*n2 too large");
  hipLaunchKernelGGL(cube_out_kernel, dim3(n3 * n2), dim3(256), nL * sizeof(c128), st, (const c128*)alpha,
                     (const c128*)lam, W, nL, t3, n3, n2, n1, (c128*)out);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

namespace {
// Shared driver.  Time grids are either device arrays (t3 / t1) or uniform (t0 + j dt, when the
// array pointer is null): the uniform form builds the GEMM operands from exponential tables.
// nL / lam: the t3 (X, GEMM K) side; nz / lamz: the t1 side (Mt is [M][nL][nz]).  trans != 0 writes
// out[k][i] = S[i][k] (the host's swapped form, which puts the smaller pruned index set on K).
int ens_run(const char* fn, const qd_c128* alpha, const qd_c128* Mt, const qd_c128* beta, const qd_c128* lam, int M,
            int nL, const double* t3, double t3_0, double dt3, int n3, const double* t1, double t1_0, double dt1,
            int n1, qd_c128* out, int accumulate, void* stream, int nz = 0, const qd_c128* lamz_ = nullptr,
            int trans = 0) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  if (nz == 0) nz = nL;
  QD_CHECK_ARG(alpha && Mt && beta && lam && out, "%s: null pointer", fn);
  QD_CHECK_ARG(M >= 1 && nL >= 1 && nz >= 1 && n3 >= 1 && n1 >= 1, "%s: bad sizes", fn);
  QD_CHECK_ARG(ens_sizes_ok(M, nL), "%s: M*nL too large", fn);
  hipStream_t st = (hipStream_t)stream;
  const EnsPlan pl = ens_plan(fn, M, nL, nz, n3, n1, !t3, !t1, trans != 0);
  // a shape too large for the arena reports that before a refusal of its plan
  void* w = nullptr;
  int rc = workspace(WS_2DES, pl.total * sizeof(c128), &w, st);
  if (rc) return rc;
  QD_CHECK_ARG(!pl.refused, "%s", pl.msg);
  BuildArgs a{};
  a.d = pl.d;
  a.M = M;
  a.alpha = (const c128*)alpha;
  a.lam = (const c128*)lam;
  a.nL = nL;
  a.t3 = t3, a.t3_0 = t3_0, a.dt3 = dt3, a.n3 = n3;
  a.X = (c128*)w + pl.offX;
  a.fine = (c128*)w + pl.offFine;
  a.Mt = (const c128*)Mt;
  a.beta = (const c128*)beta;
  a.lamz = (const c128*)(lamz_ ? lamz_ : lam);
  a.nz = nz;
  a.t1 = t1, a.t1_0 = t1_0, a.dt1 = dt1, a.n1 = n1;
  a.Z = (c128*)w + pl.offZ;
  c128* slabs = (c128*)w + pl.offSlabs;
  for (int i = 0; i < pl.nbuild; ++i) QD_TRY(launch_build(pl.build[i], a, st));
  QD_TRY(launch_ens_gemm(pl.gemm, a.X, pl.d.Kp, a.Z, pl.d.n3p, pl.d.n1p, slabs, st, pl.xtab ? a.fine : nullptr));
  return launch_reduce(pl.reduce, slabs, pl.gemm.S, n3, n1, pl.d.n3p, pl.d.n1p, (c128*)out, accumulate, st);
}
}  // namespace

extern "C" int qd_response2d_ensemble(const qd_c128* alpha, const qd_c128* Mt, const qd_c128* beta,
                                      const qd_c128* lam, int M, int nL, const double* t3, int n3, const double* t1,
                                      int n1, qd_c128* out, int accumulate, void* stream) {
  QD_CHECK_ARG(t3 && t1, "qd_response2d_ensemble: null time grid");
  return ens_run("qd_response2d_ensemble", alpha, Mt, beta, lam, M, nL, t3, 0, 0, n3, t1, 0, 0, n1, out, accumulate,
                 stream);
}

extern "C" int qd_response2d_ensemble_uniform(const qd_c128* alpha, const qd_c128* Mt, const qd_c128* beta,
                                              const qd_c128* lam, int M, int nL, double t3_0, double dt3, int n3,
                                              double t1_0, double dt1, int n1, qd_c128* out, int accumulate,
                                              void* stream) {
  QD_CHECK_ARG(nL <= ZMAX && n1 <= 16 * UNI_MAXC, "qd_response2d_ensemble_uniform: nL=%d (<= %d), n1=%d (<= %d)", nL,
               ZMAX, n1, 16 * UNI_MAXC);
  return ens_run("qd_response2d_ensemble_uniform", alpha, Mt, beta, lam, M, nL, nullptr, t3_0, dt3, n3, nullptr, t1_0,
                 dt1, n1, out, accumulate, stream);
}

extern "C" int qd_response2d_ensemble_rect(const qd_c128* alpha, const qd_c128* lamx, int nx, const qd_c128* Mt,
                                           const qd_c128* beta, const qd_c128* lamz, int nz, int M, const double* t3,
                                           double t3_0, double dt3, int n3, const double* t1, double t1_0, double dt1,
                                           int n1, int transpose_out, qd_c128* out, int accumulate, void* stream) {
  QD_CHECK_ARG(lamz, "qd_response2d_ensemble_rect: null pointer");
  QD_CHECK_ARG(t1 || (nz <= ZMAX && nx <= ZMAX && n1 <= 16 * UNI_MAXC),
               "qd_response2d_ensemble_rect: uniform t1 needs nx, nz <= %d and n1 <= %d", ZMAX, 16 * UNI_MAXC);
  return ens_run("qd_response2d_ensemble_rect", alpha, Mt, beta, lamx, M, nx, t3, t3_0, dt3, n3, t1, t1_0, dt1, n1, out,
                 accumulate, stream, nz, lamz, transpose_out ? 1 : 0);
}

extern "C" int qd_response2d_t2_dims(int M, int nL, int n3, int n1, int* n3p, int* n1p, int* Kp) {
  QD_CHECK_ARG(n3p && n1p && Kp, "qd_response2d_t2_dims: null pointer");
  QD_CHECK_ARG(M >= 1 && nL >= 1 && n3 >= 1 && n1 >= 1, "qd_response2d_t2_dims: bad sizes");
  const EnsDims d = ens_dims(M, nL, n3, n1);
  *n3p = d.n3p;
  *n1p = d.n1p;
  *Kp = d.Kp;
  return QD_OK;
}

extern "C" int qd_response2d_t2_operands_rect(const qd_c128* alpha, const qd_c128* lamp, int np,
                                              const qd_c128* Bm, const qd_c128* lamr, int nr, const qd_c128* Cm,
                                              const qd_c128* beta, const qd_c128* lamq, int nq, int M, double t3_0,
                                              double dt3, int n3, double t1_0, double dt1, int n1, qd_c128* P_,
                                              qd_c128* Q_, void* stream) {
  const char* fn = "qd_response2d_t2_operands_rect";
  QD_CHECK_ARG(alpha && lamp && Bm && lamr && Cm && beta && lamq && P_ && Q_, "%s: null pointer", fn);
  QD_CHECK_ARG(M >= 1 && np >= 1 && nr >= 1 && nq >= 1 && n3 >= 1 && n1 >= 1, "%s: bad sizes", fn);
  const T2OpsPlan pl = t2ops_plan(fn, M, np, nr, nq, n3, n1);
  QD_CHECK_ARG(!pl.refused, "%s", pl.msg);
  BuildArgs a{};
  a.d = pl.d;
  a.M = M;
  a.n3 = n3;
  a.palpha = (const c128*)alpha;
  a.Bm = (const c128*)Bm;
  a.lamp = (const c128*)lamp;
  a.np = np;
  a.p_0 = t3_0, a.dp = dt3;
  a.P = (c128*)P_;
  // Q = C_m Y_m: the uniform Z build with Mt := C [M][nr][nq] (Z rows only)
  a.Mt = (const c128*)Cm;
  a.beta = (const c128*)beta;
  a.lamz = (const c128*)lamq;
  a.nL = nr;
  a.nz = nq;
  a.t1_0 = t1_0, a.dt1 = dt1, a.n1 = n1;
  a.Z = (c128*)Q_;
  for (int i = 0; i < pl.nbuild; ++i) QD_TRY(launch_build(pl.build[i], a, (hipStream_t)stream));
  return QD_OK;
}

extern "C" int qd_response2d_t2_operands(const qd_c128* alpha, const qd_c128* Bm, const qd_c128* Cm,
                                         const qd_c128* beta, const qd_c128* lam, int M, int nL, double t3_0,
                                         double dt3, int n3, double t1_0, double dt1, int n1, qd_c128* P_,
                                         qd_c128* Q_, void* stream) {
  return qd_response2d_t2_operands_rect(alpha, lam, nL, Bm, lam, nL, Cm, beta, lam, nL, M, t3_0, dt3, n3, t1_0, dt1,
                                        n1, P_, Q_, stream);
}

extern "C" int qd_response2d_t2_apply(const qd_c128* P, const qd_c128* Q, const qd_c128* lam, int M, int nL, int n3,
                                      int n1, const double* t2, int n2, qd_c128* out, int accumulate, void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  const char* fn = "qd_response2d_t2_apply";
  QD_CHECK_ARG(P && Q && lam && t2 && out, "%s: null pointer", fn);
  QD_CHECK_ARG(M >= 1 && nL >= 1 && n3 >= 1 && n1 >= 1 && n2 >= 1 && n2 <= GRID_YZ_MAX, "%s: bad sizes", fn);
  hipStream_t st = (hipStream_t)stream;
  const T2ApplyPlan pl = t2apply_plan(fn, M, nL, n3, n1, n2);
  QD_CHECK_ARG(!pl.refused, "%s", pl.msg);
  const EnsDims& d = pl.d;
  void* w = nullptr;
  int rc = workspace(WS_2DES, pl.total * sizeof(c128), &w, st);
  if (rc) return rc;
  c128* E = (c128*)w + pl.offE;
  c128* slabs = (c128*)w + pl.offSlabs;
  hipLaunchKernelGGL(ens_e_kernel, dim3(pl.e.gx), dim3(ENS_TPB), 0, st, (const c128*)lam, d.K, d.Kp, t2, n2, E);
  QD_HIP(hipGetLastError());
  hipLaunchKernelGGL(ens_t2_gemm_kernel, dim3(pl.gx, pl.gy, pl.gz), dim3(CG_WG), 0, st, (const c128*)P, d.Kp,
                     (const c128*)Q, d.n1p, (const c128*)E, d.tiles, pl.S, slabs, d.n3p, (int)pl.ldz);
  QD_HIP(hipGetLastError());
  hipLaunchKernelGGL(ens_reduce_t2_kernel, dim3(pl.reduce.gx), dim3(ENS_TPB), 0, st, slabs, pl.S, n2, n3, n1, d.n3p,
                     d.n1p, (c128*)out, accumulate);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

extern "C" int qd_response2d_t2scan(const qd_c128* alpha, const qd_c128* Bm, const qd_c128* Cm, const qd_c128* beta,
                                    const qd_c128* lam, int M, int nL, double t3_0, double dt3, int n3,
                                    const double* t2, int n2, double t1_0, double dt1, int n1, qd_c128* out,
                                    int accumulate, void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  const char* fn = "qd_response2d_t2scan";
  QD_CHECK_ARG(alpha && Bm && Cm && beta && lam && t2 && out, "%s: null pointer", fn);
  QD_CHECK_ARG(M >= 1 && nL >= 1 && n3 >= 1 && n1 >= 1 && n2 >= 1, "%s: bad sizes", fn);
  const EnsDims d = ens_dims(M, nL, n3, n1);
  void* w = nullptr;
  int rc = workspace(WS_2DES_OPS, ((size_t)d.n3p * d.Kp + (size_t)d.Kp * d.n1p) * sizeof(c128), &w, (hipStream_t)stream);
  if (rc) return rc;
  qd_c128* P = (qd_c128*)w;
  qd_c128* Q = P + (size_t)d.n3p * d.Kp;
  if ((rc = qd_response2d_t2_operands(alpha, Bm, Cm, beta, lam, M, nL, t3_0, dt3, n3, t1_0, dt1, n1, P, Q, stream)))
    return rc;
  return qd_response2d_t2_apply(P, Q, lam, M, nL, n3, n1, t2, n2, out, accumulate, stream);
}

// Split-K complex GEMM for other translation units (TDSE batches): partial products of A [Mp][Kp] * B [Kp][Np]
// (row-major, Mp and Np multiples of 128, Kp of 16) into S slabs [S][Mp][Np]; S is returned through *S_out
// (<= max_S).  The caller sums the slabs in order s = 0 .. S-1.
int qd::cgemm_splitk_slabs(const c128* A, const c128* B, int Mp, int Kp, int Np, c128* slabs, int max_S, int* S_out,
                           hipStream_t st) {
  const SplitKPlan pl = splitk_plan(Mp, Kp, Np, max_S);
  QD_CHECK_ARG(!pl.refused, "%s", pl.msg);
  QD_TRY(launch_ens_gemm(pl.gemm, A, Kp, B, Mp, Np, slabs, st));
  *S_out = pl.gemm.S;
  return QD_OK;
}

extern "C" int qd_resolvent_grid2d(const qd_c128* a, const qd_c128* M, const qd_c128* v, const qd_c128* lam, int n,
                                   const double* wx, int nx, const double* wy, int ny, qd_c128* out, void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  const char* fn = "qd_resolvent_grid2d";
  QD_CHECK_ARG(a && M && v && lam && wx && wy && out, "%s: null pointer", fn);
  QD_CHECK_ARG(n >= 1 && nx >= 1 && ny >= 1 && n <= 65536 && nx <= 65536 && ny <= 65536, "%s: bad sizes", fn);
  hipStream_t st = (hipStream_t)stream;
  const ResolventPlan pl = resolvent_plan(n, nx, ny);
  void* w = nullptr;
  int rc = workspace(WS_2DES, pl.total * sizeof(c128), &w, st);
  if (rc) return rc;
  c128* Mp = (c128*)w + pl.offM;
  c128* Z = (c128*)w + pl.offZ;
  c128* W = (c128*)w + pl.offW;
  c128* X = (c128*)w + pl.offX;
  c128* slabs = (c128*)w + pl.offSlabs;
  hipLaunchKernelGGL(pad_square_kernel, dim3(pl.pad.gx), dim3(ENS_TPB), 0, st, (const c128*)M, n, pl.np, pl.np, Mp);
  QD_HIP(hipGetLastError());
  auto operand = [&](const RespLaunch& l, const qd_c128* coef, const double* wg, int nw, int rows_w, int R, int C,
                     c128* o) {
    hipLaunchKernelGGL(resolvent_operand_kernel, dim3(l.gx), dim3(ENS_TPB), 0, st, (const c128*)coef, (const c128*)lam,
                       n, wg, nw, rows_w, R, C, o);
    return hipGetLastError();
  };
  QD_HIP(operand(pl.zop, v, wy, ny, 0, pl.np, pl.nyp, Z));
  QD_HIP(operand(pl.xop, a, wx, nx, 1, pl.nxp, pl.np, X));
  // W = M Z (padded), then out = X W
  QD_TRY(launch_ens_gemm(pl.gemm1, Mp, pl.np, Z, pl.np, pl.nyp, slabs, st));
  QD_TRY(launch_reduce(pl.reduce1, slabs, pl.gemm1.S, pl.np, pl.nyp, pl.np, pl.nyp, W, 0, st));
  QD_TRY(launch_ens_gemm(pl.gemm2, X, pl.np, W, pl.nxp, pl.nyp, slabs, st));
  return launch_reduce(pl.reduce2, slabs, pl.gemm2.S, nx, ny, pl.nxp, pl.nyp, (c128*)out, 0, st);
}

extern "C" int qd_resolvent_sum(const qd_c128* coeff, const qd_c128* lam, int n, const double* w, int nw,
                                qd_c128* out, void* stream) {
  QD_CHECK_ARG(coeff && lam && w && out, "qd_resolvent_sum: null pointer");
  QD_CHECK_ARG(n >= 1 && nw >= 1, "qd_resolvent_sum: bad sizes");
  hipLaunchKernelGGL(resolvent_sum_kernel, dim3(flat_grid(nw)), dim3(256), 0, (hipStream_t)stream,
                     (const c128*)coeff, (const c128*)lam, n, w, nw, (c128*)out);
  QD_HIP(hipGetLastError());
  return QD_OK;
}
