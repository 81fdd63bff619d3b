// wp_gmat.hip — wavepacket dynamics in curvilinear coordinates: the G-matrix kinetic operator and its RK4 run.
//
// Replaces the curvilinear branch of pyqed/wpd.py:
//   KEO / PEO / hpsi (wpd.py:1861-1940)                        -> qd_wp2_gmat_apply
//   adiabatic_2d(coords='curvilinear') (wpd.py:1783-1859)       -> qd_wp2_gmat_rk4
// K psi = 1/2 sum_rs p_r G_rs(x, y) p_s psi with a position-dependent 2 x 2 metric G, so exp(-i K dt) is not diagonal
// in k and the split-operator classes do not apply; the reference integrates i dpsi/dt = (K + v) psi with RK4.
//
// The reference's ifft2(kx fft2(psi)) is the one-dimensional D_x psi = IFFT_x(kx FFT_x psi) (the transform along the
// other axis cancels), so an application of H is 8 line transforms where the reference makes 12 (kernels and formulas:
// wp_gmat_kernels.hpp).  RK4 in Horner form (qd_common.hpp), y_0 = psi, y_{s+1} = psi - i c_s H y_s.
//
//   wp2_gmat_pow2   nx, ny powers of two in [16, 1024]: two launches per stage.  The column pass turns (y_s, D_y y_s)
//                   into (u, phi_y); the row pass finishes H y_s, makes y_{s+1} and, in the same launch, D_y y_{s+1}
//                   for the next column pass.  One prologue row pass per call forms D_y psi: 8 launches per step, four
//                   state-sized scratch arrays per member (y, D_y y, u, phi_y).  The batch is part of the grid.  The
//                   column tile has a narrow and (nx >= 512) a wide form, chosen from the number of workgroups and
//                   noted beside the path as wp2_gmat_col_narrow / wp2_gmat_col_wide.
//   wp2_gmat_any    every other shape: fft_lines along each axis and element-wise kernels between; where fft_lines
//                   leaves four-step order the k table is applied through that order.
// No atomics; a member's result is a function of the shape alone.
//
// Coupled surfaces (qd_wp2_gmat_ms_apply / qd_wp2_gmat_ms_rk4, noted as wp2_gmat_ms): i dpsi_a/dt = K psi_a +
// sum_b V_ab psi_b, K the same on every state.  The states are planes, psi [B][ns][nx][ny], so both paths above run
// unchanged on B ns members (the tile rule counts B ns) and only the last kernel of a stage, which adds
// sum_b V_ab y_b, knows ns.  That kernel reads the planes b != a of y, which other workgroups of the same launch
// write when y is updated in place, so for ns > 1 the stages ping-pong between two y arrays (psi -> y -> y' -> y ->
// psi: five state-sized scratch arrays instead of four).  The alternative, one workgroup owning all ns planes of its
// rows, would tie the row tile and its LDS to ns; the extra array costs memory only.  The single-surface entry
// points are the ns = 1 case of the same code.
#include <atomic>

#include "spo_plan.hpp"
#include "wp_gmat_kernels.hpp"

namespace qd {
namespace {

struct GmatArgs {
  int B, ns, nx, ny;   // B ns members: the states of a coupled system are planes [B][ns][nx][ny]
  const double* G;
  const c128* v;       // [ns][ns][nx][ny]
  const double *kx, *ky;
  hipStream_t st;
  long npts() const { return (long)nx * ny; }
  long members() const { return (long)B * ns; }
  long total() const { return members() * nx * ny; }
};

int check_args(const char* who, const void* psi, int B, const void* G, const void* kx, const void* ky, int nx, int ny) {
  QD_CHECK_ARG(psi && G && kx && ky, "%s: null pointer (psi, G, kx and ky must be non-null)", who);
  QD_CHECK_ARG(B >= 1 && nx >= 1 && ny >= 1, "%s: B=%d nx=%d ny=%d must be >= 1", who, B, nx, ny);
  QD_CHECK_ARG((double)B * nx * ny < 2147483648.0, "%s: B nx ny = %.0f points, must be < 2^31", who,
               (double)B * nx * ny);
  return QD_OK;
}

int check_args_ms(const char* who, const void* psi, int B, int ns, const void* G, const void* kx, const void* ky,
                  int nx, int ny) {
  QD_CHECK_ARG(psi && G && kx && ky, "%s: null pointer (psi, G, kx and ky must be non-null)", who);
  QD_CHECK_ARG(B >= 1 && ns >= 1 && nx >= 1 && ny >= 1, "%s: B=%d ns=%d nx=%d ny=%d must be >= 1", who, B, ns, nx, ny);
  QD_CHECK_ARG((double)B * ns * nx * ny < 2147483648.0 && (double)ns * ns * nx * ny < 2147483648.0,
               "%s: B ns nx ny = %.0f, ns ns nx ny = %.0f points, must be < 2^31", who, (double)B * ns * nx * ny,
               (double)ns * ns * nx * ny);
  return QD_OK;
}

int grid_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 16384)); }

// ---------------------------------------------------------------- power-of-two grids
// Compute units of the current device: one lookup per thread and device.
int device_cus(int* cus) {
  static thread_local int last_dev = -1, last_cus = 0;
  int dev = 0;
  QD_HIP(hipGetDevice(&dev));
  if (dev != last_dev) {
    QD_HIP(hipDeviceGetAttribute(&last_cus, hipDeviceAttributeMultiprocessorCount, dev));
    last_dev = dev;
  }
  *cus = last_cus;
  return QD_OK;
}

// The wide column tile of nx = L needs more dynamic LDS than the 64 KB a kernel gets unasked: raise the kernel's limit,
// once per device.
template <int L>
int col_wide_ready() {
  static std::atomic<unsigned long long> ready{0};   // bit d: done on device d
  int dev = 0;
  QD_HIP(hipGetDevice(&dev));
  const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0;
  if (ready.load() & bit) return QD_OK;
  QD_HIP(hipFuncSetAttribute((const void*)wp2_gmat_col_kernel<L, wpg_col_wide(L)>,
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)wpg_col_lds(L, wpg_col_wide(L))));
  ready.fetch_or(bit);
  return QD_OK;
}

struct Pow2 {
  GmatArgs a;
  c128 *twx, *twy;
  double *kxs, *kys;
  bool wide;   // the column tile of this call

  // The wide tile (nx >= 512) when it leaves a workgroup for every compute unit of the device, else the narrow one.
  int pick_tile() {
    wide = false;
    if (a.nx >= WPG_WIDE_MIN_NX) {
      int cus = 0;
      QD_TRY(device_cus(&cus));
      wide = a.members() * (a.ny / WPG_WIDE_C) >= cus;
    }
    if (wide) QD_TRY(a.nx == 512 ? col_wide_ready<512>() : col_wide_ready<1024>());
    note_path(wide ? "wp2_gmat_col_wide" : "wp2_gmat_col_narrow");
    return QD_OK;
  }

  int prepare() {
    QD_TRY(pick_tile());
    void* w = nullptr;
    QD_TRY(workspace(WS_SPO, (size_t)(a.nx + a.ny) * (sizeof(c128) + sizeof(double)), &w, a.st));
    twx = (c128*)w;
    twy = twx + a.nx;
    kxs = (double*)(twy + a.ny);
    kys = kxs + a.nx;
    const int len[2] = {a.nx, a.ny};
    c128* tw[2] = {twx, twy};
    const double* k[2] = {a.kx, a.ky};
    double* ks[2] = {kxs, kys};
    for (int d = 0; d < 2; ++d) {
      hipLaunchKernelGGL(twiddle_kernel, dim3((len[d] + 255) / 256), dim3(256), 0, a.st, len[d], tw[d]);
      hipLaunchKernelGGL(wpg_ktable_kernel, dim3((len[d] + 255) / 256), dim3(256), 0, a.st, k[d], len[d], ks[d]);
    }
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // (y, dy) -> (u, phy)
  int col(const c128* y, const c128* dy, c128* u, c128* phy) const {
    const bool hit = dispatch_int<16, 32, 64, 128, 256, 512, 1024>(a.nx, [&](auto L_) {
      constexpr int L = decltype(L_)::value;
      auto launch = [&](auto C_) {
        constexpr int C = decltype(C_)::value;
        constexpr size_t lds = wpg_col_lds(L, C);
        hipLaunchKernelGGL((wp2_gmat_col_kernel<L, C>), dim3((unsigned)(a.members() * (a.ny / C))), dim3(C * L / 4), lds,
                           a.st, y, dy, a.G, (const c128*)twx, (const double*)kxs, a.ny, u, phy);
      };
      if (wide) launch(int_c<wpg_col_wide(L)>{});
      else launch(int_c<wpg_col_c(L)>{});
      return true;
    });
    QD_CHECK_ARG(hit, "wp2_gmat: internal: no column kernel for nx = %d", a.nx);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  int row(int mode, const c128* phy, const c128* u, const c128* ys, const c128* psi, double coef, c128* ynew, c128* dy,
          c128* snap, size_t sstride) const {
    const bool hit = dispatch_int<16, 32, 64, 128, 256, 512, 1024>(a.ny, [&](auto L_) {
      return dispatch_int<WPG_PRO, WPG_APPLY, WPG_STAGE>(mode, [&](auto M_) {
        constexpr int L = decltype(L_)::value, R = wpg_row_r(L);
        hipLaunchKernelGGL((wp2_gmat_row_kernel<L, decltype(M_)::value>), dim3((unsigned)(a.members() * (a.nx / R))),
                           dim3(R * L / 4), 0, a.st, phy, u, ys, psi, a.v, (const c128*)twy, (const double*)kys, a.nx,
                           a.ns, coef, ynew, dy, snap, sstride);
        return true;
      });
    });
    QD_CHECK_ARG(hit, "wp2_gmat: internal: no row kernel for ny = %d, mode %d", a.ny, mode);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
};

int pow2_apply(const GmatArgs& a, const c128* psi, c128* out) {
  Pow2 p{a};
  QD_TRY(p.prepare());
  void* w = nullptr;
  const size_t n = (size_t)a.total();
  QD_TRY(workspace(WS_SPO, 3 * n * sizeof(c128), &w, a.st));
  c128 *dy = (c128*)w, *u = dy + n, *phy = u + n;
  QD_TRY(p.row(WPG_PRO, nullptr, nullptr, psi, nullptr, 0.0, nullptr, dy, nullptr, 0));
  QD_TRY(p.col(psi, dy, u, phy));
  return p.row(WPG_APPLY, phy, u, psi, nullptr, 0.0, out, nullptr, nullptr, 0);
}

// ---------------------------------------------------------------- any grid
struct AnyGrid {
  GmatArgs a;
  double *kxs, *kys;
  c128 *t1, *t2;   // transform scratch, one state each

  int prepare() {
    void* w = nullptr;
    const size_t n = (size_t)a.total();
    QD_TRY(workspace(WS_SPO, 2 * n * sizeof(c128) + (size_t)(a.nx + a.ny) * sizeof(double), &w, a.st));
    t1 = (c128*)w;
    t2 = t1 + n;
    kxs = (double*)(t2 + n);
    kys = kxs + a.nx;
    hipLaunchKernelGGL(wpg_ktable_kernel, dim3((a.nx + 255) / 256), dim3(256), 0, a.st, a.kx, a.nx, kxs);
    hipLaunchKernelGGL(wpg_ktable_kernel, dim3((a.ny + 255) / 256), dim3(256), 0, a.st, a.ky, a.ny, kys);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // dst = D_axis src (axis 0: x, 1: y); dst may be src
  int deriv(const c128* src, int axis, c128* dst) const {
    const long n = a.total();
    const long O = axis ? a.members() * a.nx : a.members(), I = axis ? 1 : a.ny;
    const int L = axis ? a.ny : a.nx;
    const double* ks = axis ? kys : kxs;
    QD_TRY(copy_device(t1, src, (size_t)n * sizeof(c128), a.st));
    int l2 = 0;
    {
      WsScope plan(a.st);   // fft_lines' tables go back to the arena with each call
      QD_TRY(fft_lines(t1, O, L, I, false, a.st, &l2));
    }
    hipLaunchKernelGGL(wpg_pick_kernel, dim3(grid_for(n)), dim3(256), 0, a.st, (const c128*)t1, t2, ks, n, L, I, l2);
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
    QD_TRY(deriv(ys, 0, b0));
    QD_TRY(deriv(ys, 1, b1));
    hipLaunchKernelGGL(wpg_gprod_kernel, dim3(grid_for(n)), dim3(256), 0, a.st, b0, b1, a.G, n, a.npts());
    QD_HIP(hipGetLastError());
    QD_TRY(deriv(b0, 0, b2));
    QD_TRY(deriv(b1, 1, b0));
    hipLaunchKernelGGL(wpg_combine_kernel, dim3(grid_for(n)), dim3(256), 0, a.st, (const c128*)b2, (const c128*)b0, ys,
                       psi, a.v, n, a.npts(), a.ns, coef, ynew, snap, sstride);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
};

bool pow2_grid(int nx, int ny) { return pow2_in_range(nx) && pow2_in_range(ny); }

// out = (K + V) psi; the caller has checked the arguments and holds the call's WsScope
int gmat_apply(const GmatArgs& a, const c128* psi, c128* out) {
  const bool pow2 = pow2_grid(a.nx, a.ny);
  note_path(pow2 ? "wp2_gmat_pow2" : "wp2_gmat_any");
  if (pow2) return pow2_apply(a, psi, out);
  AnyGrid g{a};
  QD_TRY(g.prepare());
  void* w = nullptr;
  const size_t n = (size_t)a.total();
  QD_TRY(workspace(WS_SPO, 3 * n * sizeof(c128), &w, a.st));
  c128* b = (c128*)w;
  return g.stage(psi, nullptr, 0.0, out, nullptr, 0, b, b + n, b + 2 * n);
}

// nsteps >= 1 Horner-RK4 steps of psi in place, snapshots [B][nsteps / nout][ns][nx][ny]
int gmat_rk4(const GmatArgs& a, c128* psi, double dt, int nsteps, int nout, c128* snap) {
  hipStream_t st = a.st;
  const size_t n = (size_t)a.total(), mpts = (size_t)a.ns * a.npts();   // points of the batch, of one member
  const size_t sstride = (size_t)(nsteps / nout) * mpts;                // between the members' snapshot blocks
  const double coef[4] = {dt * 0.25, dt / 3.0, dt * 0.5, dt};   // rk4_horner_coef
  const bool pow2 = pow2_grid(a.nx, a.ny);
  note_path(pow2 ? "wp2_gmat_pow2" : "wp2_gmat_any");
  const bool pingpong = a.ns > 1;   // a stage reads y across planes: it must not write the array it reads
  void* w = nullptr;
  QD_TRY(workspace(WS_SPO, (pingpong ? 5 : 4) * n * sizeof(c128), &w, st));
  c128 *y = (c128*)w, *s1 = y + n, *s2 = s1 + n, *s3 = s2 + n, *y2 = pingpong ? s3 + n : y;
  Pow2 p{a};
  AnyGrid g{a};
  if (pow2) {
    QD_TRY(p.prepare());
    QD_TRY(p.row(WPG_PRO, nullptr, nullptr, psi, nullptr, 0.0, nullptr, s1, nullptr, 0));   // s1 = D_y psi
  } else {
    QD_TRY(g.prepare());
  }
  const c128* srcs[4] = {psi, y, y2, y};   // psi -> y -> y2 -> y -> psi
  c128* dsts[4] = {y, y2, y, psi};
  for (int step = 1; step <= nsteps; ++step) {
    for (int s = 0; s < 4; ++s) {
      const c128* src = srcs[s];
      c128* dst = dsts[s];
      c128* sp = (s == 3 && snap && step % nout == 0) ? snap + (size_t)(step / nout - 1) * mpts : nullptr;
      if (pow2) {
        QD_TRY(p.col(src, s1, s2, s3));                                            // s2 = u, s3 = phi_y
        QD_TRY(p.row(WPG_STAGE, s3, s2, src, psi, coef[s], dst, s1, sp, sstride));   // s1 = D_y y_{s+1}
      } else {
        QD_TRY(g.stage(src, psi, coef[s], dst, sp, sstride, s1, s2, s3));
      }
    }
  }
  return QD_OK;
}

}  // namespace
}  // namespace qd

using namespace qd;

extern "C" int qd_wp2_gmat_apply(const qd_c128* psi, int B, const double* G, const qd_c128* v, const double* kx,
                                 const double* ky, int nx, int ny, qd_c128* out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args("qd_wp2_gmat_apply", psi, B, G, kx, ky, nx, ny));
  QD_CHECK_ARG(out, "qd_wp2_gmat_apply: null pointer (out must be non-null)");
  QD_CHECK_ARG((const void*)out != (const void*)psi, "qd_wp2_gmat_apply: out must not alias psi");
  return gmat_apply(GmatArgs{B, 1, nx, ny, G, (const c128*)v, kx, ky, st}, (const c128*)psi, (c128*)out);
}

extern "C" int qd_wp2_gmat_rk4(qd_c128* psi, int B, const double* G, const qd_c128* v, const double* kx,
                               const double* ky, int nx, int ny, double dt, int nsteps, int nout, qd_c128* snap,
                               void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args("qd_wp2_gmat_rk4", psi, B, G, kx, ky, nx, ny));
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "qd_wp2_gmat_rk4: nsteps=%d must be >= 0 and nout=%d >= 1", nsteps, nout);
  if (nsteps == 0) return QD_OK;
  return gmat_rk4(GmatArgs{B, 1, nx, ny, G, (const c128*)v, kx, ky, st}, (c128*)psi, dt, nsteps, nout, (c128*)snap);
}

extern "C" int qd_wp2_gmat_ms_apply(const qd_c128* psi, int B, int ns, const double* G, const qd_c128* V,
                                    const double* kx, const double* ky, int nx, int ny, qd_c128* out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args_ms("qd_wp2_gmat_ms_apply", psi, B, ns, G, kx, ky, nx, ny));
  QD_CHECK_ARG(out, "qd_wp2_gmat_ms_apply: null pointer (out must be non-null)");
  QD_CHECK_ARG((const void*)out != (const void*)psi, "qd_wp2_gmat_ms_apply: out must not alias psi");
  note_path("wp2_gmat_ms");
  return gmat_apply(GmatArgs{B, ns, nx, ny, G, (const c128*)V, kx, ky, st}, (const c128*)psi, (c128*)out);
}

extern "C" int qd_wp2_gmat_ms_rk4(qd_c128* psi, int B, int ns, const double* G, const qd_c128* V, const double* kx,
                                  const double* ky, int nx, int ny, double dt, int nsteps, int nout, qd_c128* snap,
                                  void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args_ms("qd_wp2_gmat_ms_rk4", psi, B, ns, G, kx, ky, nx, ny));
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "qd_wp2_gmat_ms_rk4: nsteps=%d must be >= 0 and nout=%d >= 1", nsteps, nout);
  if (nsteps == 0) return QD_OK;
  note_path("wp2_gmat_ms");
  return gmat_rk4(GmatArgs{B, ns, nx, ny, G, (const c128*)V, kx, ky, st}, (c128*)psi, dt, nsteps, nout, (c128*)snap);
}
