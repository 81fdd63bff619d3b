// wp_gmat3.hip — wavepacket dynamics in three curvilinear coordinates: the 3 x 3 G-matrix kinetic operator and its RK4
// run (extension; the reference's SPO3 stores a metric and never reads it).
//
// K psi = 1/2 sum_rs p_r G_rs(x, y, z) p_s psi with a position-dependent real 3 x 3 metric, all nine entries read;
// i dpsi_a/dt = K psi_a + sum_b V_ab psi_b integrated with RK4 in Horner form (qd_common.hpp), y_0 = psi,
// y_{s+1} = psi - i c_s H y_s.  psi [B][ns][nx][ny][nz], the states as planes as in wp_gmat.hip, so every pass runs on
// B ns members and only the pass that adds sum_b V_ab y_b knows ns.  Kernels and formulas: wp_gmat3_kernels.hpp.
//
//   wp3_gmat_pow2   every axis a power of two in [16, 256].  A stage is four launches:
//                     X   (y, D_y y, D_z y, G) -> u = D_x phi_x, phi_y, phi_z
//                     Y   u += D_y phi_y
//                     Z   y' = psi - i c (1/2 (u + D_z phi_z) + V y), the snapshot, and D_z y' in the same launch
//                     Y'  D_y y'
//                   A call starts with two launches that form D_z psi and D_y psi; a step is 16 launches.  Six
//                   state-sized scratch arrays per call (y, D_y y, D_z y, u, phi_y, phi_z), seven for ns > 1: Z reads
//                   the planes b != a of y, which other workgroups of the launch write, so the stages ping-pong y
//                   between two arrays as gmat_rk4 does in wp_gmat.hip.
//   wp3_gmat_any    every other shape, an axis of length 1 included: fft_lines along each axis of the views
//                   x [M][nx][ny nz], y [M nx][ny][nz], z [M nx ny][nz][1], a 3 x 3 point-wise product and a combine
//                   kernel; where fft_lines leaves four-step order the k table is applied through that order.
// No atomics; a member's result is a function of the shape alone.  The coupled entry points note wp3_gmat_ms beside
// the path; the single-surface ones are the ns = 1 case of the same code.
#include "spo_plan.hpp"
#include "wp_gmat3_kernels.hpp"

namespace qd {
namespace {

struct Gmat3Args {
  int B, ns, nx, ny, nz;
  const double* G;       // [nx][ny][nz][3][3]
  const c128* v;         // [ns][ns][nx][ny][nz] or null
  const double *kx, *ky, *kz;
  hipStream_t st;
  long npts() const { return (long)nx * ny * nz; }
  long members() const { return (long)B * ns; }
  long total() const { return members() * npts(); }
};

int check_args3(const char* who, const void* psi, int B, int ns, const void* G, const void* kx, const void* ky,
                const void* kz, int nx, int ny, int nz) {
  QD_CHECK_ARG(psi && G && kx && ky && kz, "%s: null pointer (psi, G, kx, ky and kz must be non-null)", who);
  QD_CHECK_ARG(B >= 1 && ns >= 1 && nx >= 1 && ny >= 1 && nz >= 1, "%s: B=%d ns=%d nx=%d ny=%d nz=%d must be >= 1", who,
               B, ns, nx, ny, nz);
  const double pts = (double)nx * ny * nz;
  QD_CHECK_ARG((double)B * ns * pts < 2147483648.0 && (double)ns * ns * pts < 2147483648.0,
               "%s: B ns nx ny nz = %.0f, ns ns nx ny nz = %.0f points, must be < 2^31", who, (double)B * ns * pts,
               (double)ns * ns * pts);
  return QD_OK;
}

int grid_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 16384)); }

bool pow2_grid3(int nx, int ny, int nz) { return wpg3_pow2(nx) && wpg3_pow2(ny) && wpg3_pow2(nz); }

// ---------------------------------------------------------------- power-of-two grids
struct Pow2x3 {
  Gmat3Args a;
  c128* tw[3];
  double* ks[3];

  int prepare() {
    const int len[3] = {a.nx, a.ny, a.nz};
    const double* k[3] = {a.kx, a.ky, a.kz};
    void* w = nullptr;
    QD_TRY(workspace(WS_SPO, (size_t)(a.nx + a.ny + a.nz) * (sizeof(c128) + sizeof(double)), &w, a.st));
    tw[0] = (c128*)w;
    tw[1] = tw[0] + a.nx;
    tw[2] = tw[1] + a.ny;
    ks[0] = (double*)(tw[2] + a.nz);
    ks[1] = ks[0] + a.nx;
    ks[2] = ks[1] + a.ny;
    for (int d = 0; d < 3; ++d) {
      hipLaunchKernelGGL(twiddle_kernel, dim3((len[d] + 255) / 256), dim3(256), 0, a.st, len[d], tw[d]);
      hipLaunchKernelGGL(wpg_ktable_kernel, dim3((len[d] + 255) / 256), dim3(256), 0, a.st, k[d], len[d], ks[d]);
    }
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // (y, dy, dz) -> (u, phy, phz)
  int xpass(const c128* y, const c128* dy, const c128* dz, c128* u, c128* phy, c128* phz) const {
    const long I = (long)a.ny * a.nz;
    const bool hit = dispatch_int<16, 32, 64, 128, 256>(a.nx, [&](auto L_) {
      constexpr int L = decltype(L_)::value, C = wpg3_c(L);
      hipLaunchKernelGGL((wp3_gmat_x_kernel<L>), dim3((unsigned)(a.members() * (I / C))), dim3(C * L / 4), 0, a.st, y,
                         dy, dz, a.G, (const c128*)tw[0], (const double*)ks[0], I, u, phy, phz);
      return true;
    });
    QD_CHECK_ARG(hit, "wp3_gmat: internal: no x kernel for nx = %d", a.nx);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // acc: dst += D_y src; else dst = D_y src
  int ypass(bool acc, const c128* src, c128* dst) const {
    const bool hit = dispatch_int<16, 32, 64, 128, 256>(a.ny, [&](auto L_) {
      constexpr int L = decltype(L_)::value, C = wpg3_c(L);
      const dim3 grid((unsigned)(a.members() * a.nx * (a.nz / C))), block(C * L / 4);
      if (acc)
        hipLaunchKernelGGL((wp3_gmat_y_kernel<L, true>), grid, block, 0, a.st, src, (const c128*)tw[1],
                           (const double*)ks[1], a.nz, dst);
      else
        hipLaunchKernelGGL((wp3_gmat_y_kernel<L, false>), grid, block, 0, a.st, src, (const c128*)tw[1],
                           (const double*)ks[1], a.nz, dst);
      return true;
    });
    QD_CHECK_ARG(hit, "wp3_gmat: internal: no y kernel for ny = %d", a.ny);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // the 2-D row kernel on the nx ny lines of nz points of every plane
  int zpass(int mode, const c128* phz, const c128* u, const c128* ys, const c128* psi, double coef, c128* ynew,
            c128* dz, c128* snap, size_t sstride) const {
    const int rows = a.nx * a.ny;
    const bool hit = dispatch_int<16, 32, 64, 128, 256>(a.nz, [&](auto L_) {
      return dispatch_int<WPG_PRO, WPG_APPLY, WPG_STAGE>(mode, [&](auto M_) {
        constexpr int L = decltype(L_)::value, R = wpg_row_r(L);
        hipLaunchKernelGGL((wp2_gmat_row_kernel<L, decltype(M_)::value>), dim3((unsigned)(a.members() * (rows / R))),
                           dim3(R * L / 4), 0, a.st, phz, u, ys, psi, a.v, (const c128*)tw[2], (const double*)ks[2],
                           rows, a.ns, coef, ynew, dz, snap, sstride);
        return true;
      });
    });
    QD_CHECK_ARG(hit, "wp3_gmat: internal: no z kernel for nz = %d, mode %d", a.nz, mode);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // dz = D_z psi, dy = D_y psi
  int prologue(const c128* psi, c128* dy, c128* dz) const {
    QD_TRY(zpass(WPG_PRO, nullptr, nullptr, psi, nullptr, 0.0, nullptr, dz, nullptr, 0));
    return ypass(false, psi, dy);
  }
};

// ---------------------------------------------------------------- any grid
struct AnyGrid3 {
  Gmat3Args a;
  double* ks[3];
  c128 *t1, *t2;   // transform scratch, one state each

  int prepare() {
    const int len[3] = {a.nx, a.ny, a.nz};
    const double* k[3] = {a.kx, a.ky, a.kz};
    void* w = nullptr;
    const size_t n = (size_t)a.total();
    QD_TRY(workspace(WS_SPO, 2 * n * sizeof(c128) + (size_t)(a.nx + a.ny + a.nz) * sizeof(double), &w, a.st));
    t1 = (c128*)w;
    t2 = t1 + n;
    ks[0] = (double*)(t2 + n);
    ks[1] = ks[0] + a.nx;
    ks[2] = ks[1] + a.ny;
    for (int d = 0; d < 3; ++d)
      hipLaunchKernelGGL(wpg_ktable_kernel, dim3((len[d] + 255) / 256), dim3(256), 0, a.st, k[d], len[d], ks[d]);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // dst = D_axis src (axis 0: x, 1: y, 2: z); dst may be src
  int deriv(const c128* src, int axis, c128* dst) const {
    const long n = a.total(), M = a.members();
    const long O = axis == 0 ? M : axis == 1 ? M * a.nx : M * a.nx * a.ny;
    const long I = axis == 0 ? (long)a.ny * a.nz : axis == 1 ? a.nz : 1;
    const int L = axis == 0 ? a.nx : axis == 1 ? a.ny : a.nz;
    QD_TRY(copy_device(t1, src, (size_t)n * sizeof(c128), a.st));
    int l2 = 0;
    {
      WsScope plan(a.st);   // fft_lines' tables go back to the arena with each call
      QD_TRY(fft_lines(t1, O, L, I, false, a.st, &l2));
    }
    hipLaunchKernelGGL(wpg_pick_kernel, dim3(grid_for(n)), dim3(256), 0, a.st, (const c128*)t1, t2,
                       (const double*)ks[axis], n, L, I, l2);
    QD_HIP(hipGetLastError());
    {
      WsScope plan(a.st);
      QD_TRY(fft_lines(t2, O, L, I, true, a.st, &l2));
    }
    hipLaunchKernelGGL(wpg_pick_kernel, dim3(grid_for(n)), dim3(256), 0, a.st, (const c128*)t2, dst,
                       (const double*)nullptr, n, L, I, l2);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // ynew = (K + v) ys (psi null) or psi - i coef (K + v) ys; b0..b2: three state-sized buffers; ynew may be ys for
  // ns = 1 alone
  int stage(const c128* ys, const c128* psi, double coef, c128* ynew, c128* snap, size_t sstride, c128* b0, c128* b1,
            c128* b2) const {
    const long n = a.total();
    c128* b[3] = {b0, b1, b2};
    for (int d = 0; d < 3; ++d) QD_TRY(deriv(ys, d, b[d]));
    hipLaunchKernelGGL(wpg3_gprod_kernel, dim3(grid_for(n)), dim3(256), 0, a.st, b0, b1, b2, a.G, n, a.npts());
    QD_HIP(hipGetLastError());
    for (int d = 0; d < 3; ++d) QD_TRY(deriv(b[d], d, b[d]));
    hipLaunchKernelGGL(wpg3_combine_kernel, dim3(grid_for(n)), dim3(256), 0, a.st, (const c128*)b0, (const c128*)b1,
                       (const c128*)b2, ys, psi, a.v, n, a.npts(), a.ns, coef, ynew, snap, sstride);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
};

// out = (K + V) psi; the caller has checked the arguments and holds the call's WsScope
int gmat3_apply(const Gmat3Args& a, const c128* psi, c128* out) {
  const bool pow2 = pow2_grid3(a.nx, a.ny, a.nz);
  note_path(pow2 ? "wp3_gmat_pow2" : "wp3_gmat_any");
  void* w = nullptr;
  const size_t n = (size_t)a.total();
  if (pow2) {
    Pow2x3 p{a};
    QD_TRY(p.prepare());
    QD_TRY(workspace(WS_SPO, 5 * n * sizeof(c128), &w, a.st));
    c128 *dy = (c128*)w, *dz = dy + n, *u = dz + n, *phy = u + n, *phz = phy + n;
    QD_TRY(p.prologue(psi, dy, dz));
    QD_TRY(p.xpass(psi, dy, dz, u, phy, phz));
    QD_TRY(p.ypass(true, phy, u));
    return p.zpass(WPG_APPLY, phz, u, psi, nullptr, 0.0, out, nullptr, nullptr, 0);
  }
  AnyGrid3 g{a};
  QD_TRY(g.prepare());
  QD_TRY(workspace(WS_SPO, 3 * n * sizeof(c128), &w, a.st));
  c128* b = (c128*)w;
  return g.stage(psi, nullptr, 0.0, out, nullptr, 0, b, b + n, b + 2 * n);
}

// nsteps >= 1 Horner-RK4 steps of psi in place, snapshots [B][nsteps / nout][ns][nx][ny][nz]
int gmat3_rk4(const Gmat3Args& a, c128* psi, double dt, int nsteps, int nout, c128* snap) {
  hipStream_t st = a.st;
  const size_t n = (size_t)a.total(), mpts = (size_t)a.ns * a.npts();   // points of the batch, of one member
  const size_t sstride = (size_t)(nsteps / nout) * mpts;                // between the members' snapshot blocks
  const double coef[4] = {dt * 0.25, dt / 3.0, dt * 0.5, dt};   // rk4_horner_coef
  const bool pow2 = pow2_grid3(a.nx, a.ny, a.nz);
  note_path(pow2 ? "wp3_gmat_pow2" : "wp3_gmat_any");
  const bool pingpong = a.ns > 1;   // a stage reads y across planes: it must not write the array it reads
  const int nbuf = (pow2 ? 5 : 3) + 1 + (pingpong ? 1 : 0);
  void* w = nullptr;
  QD_TRY(workspace(WS_SPO, (size_t)nbuf * n * sizeof(c128), &w, st));
  c128* s[7];
  for (int i = 0; i < nbuf; ++i) s[i] = (c128*)w + (size_t)i * n;
  c128 *y = s[nbuf - 1 - (pingpong ? 1 : 0)], *y2 = pingpong ? s[nbuf - 1] : y;
  Pow2x3 p{a};
  AnyGrid3 g{a};
  if (pow2) {
    QD_TRY(p.prepare());
    QD_TRY(p.prologue(psi, s[0], s[1]));   // s[0] = D_y psi, s[1] = D_z psi
  } else {
    QD_TRY(g.prepare());
  }
  const c128* srcs[4] = {psi, y, y2, y};   // psi -> y -> y2 -> y -> psi
  c128* dsts[4] = {y, y2, y, psi};
  for (int step = 1; step <= nsteps; ++step) {
    for (int k = 0; k < 4; ++k) {
      const c128* src = srcs[k];
      c128* dst = dsts[k];
      c128* sp = (k == 3 && snap && step % nout == 0) ? snap + (size_t)(step / nout - 1) * mpts : nullptr;
      if (pow2) {
        QD_TRY(p.xpass(src, s[0], s[1], s[2], s[3], s[4]));                                // u, phi_y, phi_z
        QD_TRY(p.ypass(true, s[3], s[2]));                                                 // u += D_y phi_y
        QD_TRY(p.zpass(WPG_STAGE, s[4], s[2], src, psi, coef[k], dst, s[1], sp, sstride));   // s[1] = D_z y_{k+1}
        QD_TRY(p.ypass(false, dst, s[0]));                                                 // s[0] = D_y y_{k+1}
      } else {
        QD_TRY(g.stage(src, psi, coef[k], dst, sp, sstride, s[0], s[1], s[2]));
      }
    }
  }
  return QD_OK;
}

}  // namespace
}  // namespace qd

using namespace qd;

extern "C" int qd_wp3_gmat_ms_apply(const qd_c128* psi, int B, int ns, const double* G, const qd_c128* V,
                                    const double* kx, const double* ky, const double* kz, int nx, int ny, int nz,
                                    qd_c128* out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args3("qd_wp3_gmat_ms_apply", psi, B, ns, G, kx, ky, kz, nx, ny, nz));
  QD_CHECK_ARG(out, "qd_wp3_gmat_ms_apply: null pointer (out must be non-null)");
  QD_CHECK_ARG((const void*)out != (const void*)psi, "qd_wp3_gmat_ms_apply: out must not alias psi");
  note_path("wp3_gmat_ms");
  return gmat3_apply(Gmat3Args{B, ns, nx, ny, nz, G, (const c128*)V, kx, ky, kz, st}, (const c128*)psi, (c128*)out);
}

extern "C" int qd_wp3_gmat_ms_rk4(qd_c128* psi, int B, int ns, const double* G, const qd_c128* V, const double* kx,
                                  const double* ky, const double* kz, int nx, int ny, int nz, double dt, int nsteps,
                                  int nout, qd_c128* snap, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args3("qd_wp3_gmat_ms_rk4", psi, B, ns, G, kx, ky, kz, nx, ny, nz));
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "qd_wp3_gmat_ms_rk4: nsteps=%d must be >= 0 and nout=%d >= 1", nsteps, nout);
  if (nsteps == 0) return QD_OK;
  note_path("wp3_gmat_ms");
  return gmat3_rk4(Gmat3Args{B, ns, nx, ny, nz, G, (const c128*)V, kx, ky, kz, st}, (c128*)psi, dt, nsteps, nout,
                   (c128*)snap);
}

extern "C" int qd_wp3_gmat_apply(const qd_c128* psi, int B, const double* G, const qd_c128* v, const double* kx,
                                 const double* ky, const double* kz, int nx, int ny, int nz, qd_c128* out,
                                 void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args3("qd_wp3_gmat_apply", psi, B, 1, G, kx, ky, kz, nx, ny, nz));
  QD_CHECK_ARG(out, "qd_wp3_gmat_apply: null pointer (out must be non-null)");
  QD_CHECK_ARG((const void*)out != (const void*)psi, "qd_wp3_gmat_apply: out must not alias psi");
  return gmat3_apply(Gmat3Args{B, 1, nx, ny, nz, G, (const c128*)v, kx, ky, kz, st}, (const c128*)psi, (c128*)out);
}

extern "C" int qd_wp3_gmat_rk4(qd_c128* psi, int B, const double* G, const qd_c128* v, const double* kx,
                               const double* ky, const double* kz, int nx, int ny, int nz, double dt, int nsteps,
                               int nout, qd_c128* snap, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args3("qd_wp3_gmat_rk4", psi, B, 1, G, kx, ky, kz, nx, ny, nz));
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "qd_wp3_gmat_rk4: nsteps=%d must be >= 0 and nout=%d >= 1", nsteps, nout);
  if (nsteps == 0) return QD_OK;
  return gmat3_rk4(Gmat3Args{B, 1, nx, ny, nz, G, (const c128*)v, kx, ky, kz, st}, (c128*)psi, dt, nsteps, nout,
                   (c128*)snap);
}
