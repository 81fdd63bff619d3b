// wp_gmat.hip — wavepacket dynamics in two and three curvilinear coordinates: the G-matrix kinetic operator and its
// RK4 run.
//
// Replaces the curvilinear branch of pyqed/wpd.py:
//   KEO / PEO / hpsi (wpd.py:1861-1940)                        -> qd_wp2_gmat_apply
//   adiabatic_2d(coords='curvilinear') (wpd.py:1783-1859)       -> qd_wp2_gmat_rk4
// and extends it to three coordinates (qd_wp3_gmat_*; the reference's SPO3 stores a metric and never reads it).
// K psi = 1/2 sum_rs p_r G_rs p_s psi with a position-dependent real D x D metric G, every entry read, so exp(-i K dt)
// is not diagonal in k and the split-operator classes do not apply; the reference integrates i dpsi/dt = (K + v) psi
// with RK4.
//
// The reference's ifft2(kx fft2(psi)) is the one-dimensional D_x psi = IFFT_x(kx FFT_x psi) (the transform along the
// other axis cancels), so an application of H in two coordinates is 8 line transforms where the reference makes 12
// (kernels and formulas: wp_gmat_kernels.hpp).  RK4 in Horner form (qd_common.hpp), y_0 = psi,
// y_{s+1} = psi - i c_s H y_s.
//
// One argument struct, one check, one apply driver and one RK4 driver serve both dimensions; they are written against
// a stepper (prepare, nscratch, prologue, stage), of which there are three:
//   Fused2 (wp2_gmat_pow2)   nx, ny powers of two in [16, 1024]: two launches per stage.  The column pass turns
//                   (y_s, D_y y_s) into (u, phi_y); the row pass finishes H y_s, makes y_{s+1} and, in the same launch,
//                   D_y y_{s+1} for the next column pass.  One prologue row pass per call forms D_y psi: 8 launches per
//                   step, four state-sized scratch arrays per member (y, D_y y, u, phi_y).  The batch is part of the
//                   grid.  The column tile has a narrow and (nx >= 512) a wide form, chosen from the number of
//                   workgroups and noted beside the path as wp2_gmat_col_narrow / wp2_gmat_col_wide.
//   Fused3 (wp3_gmat_pow2)   every axis a power of two in [16, 256].  A stage is four launches:
//                     X   (y, D_y y, D_z y, G) -> u = D_x phi_x, phi_y, phi_z
//                     Y   u += D_y phi_y
//                     Z   y' = psi - i c (1/2 (u + D_z phi_z) + V y), the snapshot, and D_z y' in the same launch
//                     Y'  D_y y'
//                   A call starts with two launches that form D_z psi and D_y psi; a step is 16 launches.  Six
//                   state-sized scratch arrays per call (y, D_y y, D_z y, u, phi_y, phi_z).  Z is the row pass of
//                   Fused2 on the nx ny lines of nz points: both steppers take their tables and that launch from
//                   Pow2Lines.
//   AnyGrid<D> (wp2_gmat_any, wp3_gmat_any)   every other shape, an axis of length 1 included: fft_lines along each
//                   axis a of the view [members prod n[< a]][n[a]][prod n[> a]], a D x D point-wise product and a
//                   combine kernel; where fft_lines leaves four-step order the k table is applied through that order.
// No atomics; a member's result is a function of the shape alone.
//
// Coupled surfaces (qd_wp{2,3}_gmat_ms_apply / _ms_rk4, noted as wp2_gmat_ms / wp3_gmat_ms beside the path):
// i dpsi_a/dt = K psi_a + sum_b V_ab psi_b, K the same on every state.  The states are planes, psi [B][ns][grid], so
// every stepper runs unchanged on B ns members (the tile rule counts B ns) and only the last kernel of a stage, which
// adds sum_b V_ab y_b, knows ns.  That kernel reads the planes b != a of y, which other workgroups of the same launch
// write when y is updated in place, so for ns > 1 the stages ping-pong between two y arrays (psi -> y -> y' -> y ->
// psi: one more state-sized scratch array).  The alternative, one workgroup owning all ns planes of its rows, would
// tie the row tile and its LDS to ns; the extra array costs memory only.  The single-surface entry points are the
// ns = 1 case of the same code.
#include <atomic>

#include "spo_plan.hpp"
#include "wp_gmat_kernels.hpp"

namespace qd {
namespace {

struct GmatArgs {
  int B, ns, D, n[3];   // B ns members: the states of a coupled system are planes [B][ns][grid]; n[2] = 1 for D = 2
  const double* G;      // [grid][D][D]
  const c128* v;        // [ns][ns][grid] or null
  const double* k[3];   // k[2] unused for D = 2
  hipStream_t st;
  long npts() const { return (long)n[0] * n[1] * n[2]; }
  long members() const { return (long)B * ns; }
  long total() const { return members() * npts(); }
};

int check_args(const char* who, const void* psi, const GmatArgs& a) {
  QD_CHECK_ARG(psi && a.G && a.k[0] && a.k[1] && (a.D == 2 || a.k[2]),
               "%s: null pointer (psi, G and every k vector must be non-null)", who);
  QD_CHECK_ARG(a.B >= 1 && a.ns >= 1 && a.n[0] >= 1 && a.n[1] >= 1 && a.n[2] >= 1,
               "%s: B=%d ns=%d and the %d extents (%d, %d, %d) must be >= 1", who, a.B, a.ns, a.D, a.n[0], a.n[1],
               a.n[2]);
  const double pts = (double)a.n[0] * a.n[1] * a.n[2];
  QD_CHECK_ARG((double)a.B * a.ns * pts < 2147483648.0 && (double)a.ns * a.ns * pts < 2147483648.0,
               "%s: B ns points = %.0f, ns ns points = %.0f, must be < 2^31", who, (double)a.B * a.ns * pts,
               (double)a.ns * a.ns * pts);
  return QD_OK;
}

int grid_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 16384)); }

// `count` state-sized scratch arrays of the call
int states(const GmatArgs& a, int count, c128** s) {
  void* w = nullptr;
  const size_t n = (size_t)a.total();
  QD_TRY(workspace(WS_SPO, (size_t)count * n * sizeof(c128), &w, a.st));
  for (int i = 0; i < count; ++i) s[i] = (c128*)w + (size_t)i * n;
  return QD_OK;
}

// ---------------------------------------------------------------- power-of-two grids
// What the two fused steppers share: the twiddles and k / n tables of every axis, and the row kernel on the lines of
// the last axis (the row pass in two coordinates, the Z pass in three).
struct Pow2Lines {
  GmatArgs a;
  c128* tw[3];
  double* ks[3];

  int prepare() {
    void* w = nullptr;
    const int sum = a.n[0] + a.n[1] + (a.D == 3 ? a.n[2] : 0);
    QD_TRY(workspace(WS_SPO, (size_t)sum * (sizeof(c128) + sizeof(double)), &w, a.st));
    c128* t = (c128*)w;
    double* k = (double*)(t + sum);
    for (int d = 0; d < a.D; ++d) {
      const int len = a.n[d];
      tw[d] = t;
      ks[d] = k;
      t += len;
      k += len;
      hipLaunchKernelGGL(twiddle_kernel, dim3((len + 255) / 256), dim3(256), 0, a.st, len, tw[d]);
      hipLaunchKernelGGL(wpg_ktable_kernel, dim3((len + 255) / 256), dim3(256), 0, a.st, a.k[d], len, ks[d]);
    }
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // (phi, u, ys) of the last axis -> ynew and its derivative d along that axis, by `mode` (wp2_gmat_row_kernel)
  int row(int mode, const c128* phi, const c128* u, const c128* ys, const c128* psi, double coef, c128* ynew, c128* d,
          c128* snap, size_t sstride) const {
    const int len = a.n[a.D - 1], rows = (int)(a.npts() / len);
    const bool hit = dispatch_int<16, 32, 64, 128, 256, 512, 1024>(len, [&](auto L_) {
      return dispatch_int<WPG_PRO, WPG_APPLY, WPG_STAGE>(mode, [&](auto M_) {
        constexpr int L = decltype(L_)::value, R = wpg_row_r(L);
        hipLaunchKernelGGL((wp2_gmat_row_kernel<L, decltype(M_)::value>), dim3((unsigned)(a.members() * (rows / R))),
                           dim3(R * L / 4), 0, a.st, phi, u, ys, psi, a.v, (const c128*)tw[a.D - 1],
                           (const double*)ks[a.D - 1], rows, a.ns, coef, ynew, d, snap, sstride);
        return true;
      });
    });
    QD_CHECK_ARG(hit, "wp_gmat: internal: no row kernel for lines of %d points, mode %d", len, mode);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
};

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

// Scratch s: D_y y, u, phi_y
struct Fused2 : Pow2Lines {
  bool wide = false;   // the column tile of this call
  explicit Fused2(const GmatArgs& args) : Pow2Lines{args} {}
  static bool fits(const GmatArgs& a) { return pow2_in_range(a.n[0]) && pow2_in_range(a.n[1]); }
  static const char* name() { return "wp2_gmat_pow2"; }
  int nscratch() const { return 3; }

  // The wide tile (nx >= 512) when it leaves a workgroup for every compute unit of the device, else the narrow one.
  int pick_tile() {
    wide = false;
    if (a.n[0] >= WPG_WIDE_MIN_NX) {
      int cus = 0;
      QD_TRY(device_cus(&cus));
      wide = a.members() * (a.n[1] / WPG_WIDE_C) >= cus;
    }
    if (wide) QD_TRY(a.n[0] == 512 ? col_wide_ready<512>() : col_wide_ready<1024>());
    note_path(wide ? "wp2_gmat_col_wide" : "wp2_gmat_col_narrow");
    return QD_OK;
  }

  int prepare() {
    QD_TRY(pick_tile());
    return Pow2Lines::prepare();
  }

  // (y, dy) -> (u, phy)
  int col(const c128* y, const c128* dy, c128* u, c128* phy) const {
    const int ny = a.n[1];
    const bool hit = dispatch_int<16, 32, 64, 128, 256, 512, 1024>(a.n[0], [&](auto L_) {
      constexpr int L = decltype(L_)::value;
      auto launch = [&](auto C_) {
        constexpr int C = decltype(C_)::value;
        constexpr size_t lds = wpg_col_lds(L, C);
        hipLaunchKernelGGL((wp2_gmat_col_kernel<L, C>), dim3((unsigned)(a.members() * (ny / C))), dim3(C * L / 4), lds,
                           a.st, y, dy, a.G, (const c128*)tw[0], (const double*)ks[0], ny, u, phy);
      };
      if (wide) launch(int_c<wpg_col_wide(L)>{});
      else launch(int_c<wpg_col_c(L)>{});
      return true;
    });
    QD_CHECK_ARG(hit, "wp2_gmat: internal: no column kernel for nx = %d", a.n[0]);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // s[0] = D_y psi
  int prologue(const c128* psi, c128* const* s) const {
    return row(WPG_PRO, nullptr, nullptr, psi, nullptr, 0.0, nullptr, s[0], nullptr, 0);
  }

  // ynew = (K + v) ys (psi null) or psi - i coef (K + v) ys with s[0] = D_y ynew; s[0] = D_y ys on entry
  int stage(const c128* ys, const c128* psi, double coef, c128* ynew, c128* snap, size_t sstride,
            c128* const* s) const {
    QD_TRY(col(ys, s[0], s[1], s[2]));
    return row(psi ? WPG_STAGE : WPG_APPLY, s[2], s[1], ys, psi, coef, ynew, s[0], snap, sstride);
  }
};

// Scratch s: D_y y, D_z y, u, phi_y, phi_z
struct Fused3 : Pow2Lines {
  explicit Fused3(const GmatArgs& args) : Pow2Lines{args} {}
  static bool fits(const GmatArgs& a) { return wpg3_pow2(a.n[0]) && wpg3_pow2(a.n[1]) && wpg3_pow2(a.n[2]); }
  static const char* name() { return "wp3_gmat_pow2"; }
  int nscratch() const { return 5; }

  // (y, dy, dz) -> (u, phy, phz)
  int xpass(const c128* y, const c128* dy, const c128* dz, c128* u, c128* phy, c128* phz) const {
    const long I = (long)a.n[1] * a.n[2];
    const bool hit = dispatch_int<16, 32, 64, 128, 256>(a.n[0], [&](auto L_) {
      constexpr int L = decltype(L_)::value, C = wpg3_c(L);
      hipLaunchKernelGGL((wp3_gmat_x_kernel<L>), dim3((unsigned)(a.members() * (I / C))), dim3(C * L / 4), 0, a.st, y,
                         dy, dz, a.G, (const c128*)tw[0], (const double*)ks[0], I, u, phy, phz);
      return true;
    });
    QD_CHECK_ARG(hit, "wp3_gmat: internal: no x kernel for nx = %d", a.n[0]);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // acc: dst += D_y src; else dst = D_y src
  int ypass(bool acc, const c128* src, c128* dst) const {
    const int nz = a.n[2];
    const bool hit = dispatch_int<16, 32, 64, 128, 256>(a.n[1], [&](auto L_) {
      constexpr int L = decltype(L_)::value, C = wpg3_c(L);
      const dim3 grid((unsigned)(a.members() * a.n[0] * (nz / C))), block(C * L / 4);
      if (acc)
        hipLaunchKernelGGL((wp3_gmat_y_kernel<L, true>), grid, block, 0, a.st, src, (const c128*)tw[1],
                           (const double*)ks[1], nz, dst);
      else
        hipLaunchKernelGGL((wp3_gmat_y_kernel<L, false>), grid, block, 0, a.st, src, (const c128*)tw[1],
                           (const double*)ks[1], nz, dst);
      return true;
    });
    QD_CHECK_ARG(hit, "wp3_gmat: internal: no y kernel for ny = %d", a.n[1]);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // s[1] = D_z psi, s[0] = D_y psi
  int prologue(const c128* psi, c128* const* s) const {
    QD_TRY(row(WPG_PRO, nullptr, nullptr, psi, nullptr, 0.0, nullptr, s[1], nullptr, 0));
    return ypass(false, psi, s[0]);
  }

  // as Fused2::stage, with s[0] = D_y and s[1] = D_z of ys on entry and of ynew behind a Horner stage
  int stage(const c128* ys, const c128* psi, double coef, c128* ynew, c128* snap, size_t sstride,
            c128* const* s) const {
    QD_TRY(xpass(ys, s[0], s[1], s[2], s[3], s[4]));   // u, phi_y, phi_z
    QD_TRY(ypass(true, s[3], s[2]));                   // u += D_y phi_y
    QD_TRY(row(psi ? WPG_STAGE : WPG_APPLY, s[4], s[2], ys, psi, coef, ynew, s[1], snap, sstride));
    return psi ? ypass(false, ynew, s[0]) : QD_OK;
  }
};

// ---------------------------------------------------------------- any grid
// Scratch s: one array per coordinate (D_a ys, then phi_a, then D_a phi_a, each in place)
template <int D>
struct AnyGrid {
  GmatArgs a;
  double* ks[D];
  c128 *t1, *t2;   // transform scratch, one state each
  explicit AnyGrid(const GmatArgs& args) : a(args) {}
  static const char* name() { return D == 2 ? "wp2_gmat_any" : "wp3_gmat_any"; }
  int nscratch() const { return D; }

  int prepare() {
    void* w = nullptr;
    const size_t n = (size_t)a.total();
    int sum = 0;
    for (int d = 0; d < D; ++d) sum += a.n[d];
    QD_TRY(workspace(WS_SPO, 2 * n * sizeof(c128) + (size_t)sum * sizeof(double), &w, a.st));
    t1 = (c128*)w;
    t2 = t1 + n;
    double* k = (double*)(t2 + n);
    for (int d = 0; d < D; ++d) {
      ks[d] = k;
      k += a.n[d];
      hipLaunchKernelGGL(wpg_ktable_kernel, dim3((a.n[d] + 255) / 256), dim3(256), 0, a.st, a.k[d], a.n[d], ks[d]);
    }
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // dst = D_axis src on the view [O][L][I] = [members prod n[< axis]][n[axis]][prod n[> axis]]; dst may be src
  int deriv(const c128* src, int axis, c128* dst) const {
    const long n = a.total();
    long O = a.members(), I = 1;
    for (int d = 0; d < axis; ++d) O *= a.n[d];
    for (int d = axis + 1; d < D; ++d) I *= a.n[d];
    const int L = a.n[axis];
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

  int prologue(const c128*, c128* const*) const { return QD_OK; }

  // ynew = (K + v) ys (psi null) or psi - i coef (K + v) ys; ynew may be ys for ns = 1 alone
  int stage(const c128* ys, const c128* psi, double coef, c128* ynew, c128* snap, size_t sstride,
            c128* const* s) const {
    const long n = a.total();
    WpgVec<D> b;
    for (int d = 0; d < D; ++d) b.p[d] = s[d];
    for (int d = 0; d < D; ++d) QD_TRY(deriv(ys, d, b.p[d]));
    hipLaunchKernelGGL(wpg_gprod_kernel<D>, dim3(grid_for(n)), dim3(256), 0, a.st, b, a.G, n, a.npts());
    QD_HIP(hipGetLastError());
    for (int d = 0; d < D; ++d) QD_TRY(deriv(b.p[d], d, b.p[d]));
    hipLaunchKernelGGL(wpg_combine_kernel<D>, dim3(grid_for(n)), dim3(256), 0, a.st, b, ys, psi, a.v, n, a.npts(),
                       a.ns, coef, ynew, snap, sstride);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
};

// ---------------------------------------------------------------- drivers
constexpr int MAX_SCRATCH = 5;   // Fused3

// out = (K + V) psi
template <class S>
int apply_with(S s, const c128* psi, c128* out) {
  note_path(S::name());
  QD_TRY(s.prepare());
  c128* b[MAX_SCRATCH];
  QD_TRY(states(s.a, s.nscratch(), b));
  QD_TRY(s.prologue(psi, b));
  return s.stage(psi, nullptr, 0.0, out, nullptr, 0, b);
}

// nsteps >= 1 Horner-RK4 steps of psi in place, snapshots [B][nsteps / nout][ns][grid]
template <class S>
int rk4_with(S s, c128* psi, double dt, int nsteps, int nout, c128* snap) {
  const GmatArgs& a = s.a;
  const size_t mpts = (size_t)a.ns * a.npts();             // points of one member
  const size_t sstride = (size_t)(nsteps / nout) * mpts;   // between the members' snapshot blocks
  const double coef[4] = {dt * 0.25, dt / 3.0, dt * 0.5, dt};   // rk4_horner_coef
  note_path(S::name());
  const bool pingpong = a.ns > 1;   // a stage reads y across planes: it must not write the array it reads
  const int nb = s.nscratch();
  c128* b[MAX_SCRATCH + 2];
  QD_TRY(states(a, nb + 1 + (pingpong ? 1 : 0), b));
  c128 *y = b[nb], *y2 = pingpong ? b[nb + 1] : y;
  QD_TRY(s.prepare());
  QD_TRY(s.prologue(psi, b));
  const c128* srcs[4] = {psi, y, y2, y};   // psi -> y -> y2 -> y -> psi
  c128* dsts[4] = {y, y2, y, psi};
  for (int step = 1; step <= nsteps; ++step) {
    for (int k = 0; k < 4; ++k) {
      c128* sp = (k == 3 && snap && step % nout == 0) ? snap + (size_t)(step / nout - 1) * mpts : nullptr;
      QD_TRY(s.stage(srcs[k], psi, coef[k], dsts[k], sp, sstride, b));
    }
  }
  return QD_OK;
}

// f(the stepper of this shape)
template <class F>
int with_stepper(const GmatArgs& a, F&& f) {
  if (a.D == 2) return Fused2::fits(a) ? f(Fused2(a)) : f(AnyGrid<2>(a));
  return Fused3::fits(a) ? f(Fused3(a)) : f(AnyGrid<3>(a));
}

// The bodies of the entry points.  `ms`: the note of a coupled-surface entry point, else null.
int apply_entry(const char* who, const char* ms, const GmatArgs& a, const qd_c128* psi, qd_c128* out) {
  WsScope wss_(a.st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args(who, psi, a));
  QD_CHECK_ARG(out, "%s: null pointer (out must be non-null)", who);
  QD_CHECK_ARG((const void*)out != (const void*)psi, "%s: out must not alias psi", who);
  if (ms) note_path(ms);
  return with_stepper(a, [&](auto s) { return apply_with(s, (const c128*)psi, (c128*)out); });
}

int rk4_entry(const char* who, const char* ms, const GmatArgs& a, qd_c128* psi, double dt, int nsteps, int nout,
              qd_c128* snap) {
  WsScope wss_(a.st);  // call-scoped scratch (qd_runtime.hip)
  QD_TRY(check_args(who, psi, a));
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "%s: nsteps=%d must be >= 0 and nout=%d >= 1", who, nsteps, nout);
  if (nsteps == 0) return QD_OK;
  if (ms) note_path(ms);
  return with_stepper(a, [&](auto s) { return rk4_with(s, (c128*)psi, dt, nsteps, nout, (c128*)snap); });
}

GmatArgs args2(int B, int ns, const double* G, const qd_c128* v, const double* kx, const double* ky, int nx, int ny,
               void* stream) {
  return GmatArgs{B, ns, 2, {nx, ny, 1}, G, (const c128*)v, {kx, ky, nullptr}, (hipStream_t)stream};
}

GmatArgs args3(int B, int ns, const double* G, const qd_c128* v, const double* kx, const double* ky, const double* kz,
               int nx, int ny, int nz, void* stream) {
  return GmatArgs{B, ns, 3, {nx, ny, nz}, G, (const c128*)v, {kx, ky, kz}, (hipStream_t)stream};
}

}  // namespace
}  // namespace qd

using namespace qd;

extern "C" int qd_wp2_gmat_apply(const qd_c128* psi, int B, const double* G, const qd_c128* v, const double* kx,
                                 const double* ky, int nx, int ny, qd_c128* out, void* stream) {
  return apply_entry("qd_wp2_gmat_apply", nullptr, args2(B, 1, G, v, kx, ky, nx, ny, stream), psi, out);
}

extern "C" int qd_wp2_gmat_rk4(qd_c128* psi, int B, const double* G, const qd_c128* v, const double* kx,
                               const double* ky, int nx, int ny, double dt, int nsteps, int nout, qd_c128* snap,
                               void* stream) {
  return rk4_entry("qd_wp2_gmat_rk4", nullptr, args2(B, 1, G, v, kx, ky, nx, ny, stream), psi, dt, nsteps, nout, snap);
}

extern "C" int qd_wp2_gmat_ms_apply(const qd_c128* psi, int B, int ns, const double* G, const qd_c128* V,
                                    const double* kx, const double* ky, int nx, int ny, qd_c128* out, void* stream) {
  return apply_entry("qd_wp2_gmat_ms_apply", "wp2_gmat_ms", args2(B, ns, G, V, kx, ky, nx, ny, stream), psi, out);
}

extern "C" int qd_wp2_gmat_ms_rk4(qd_c128* psi, int B, int ns, const double* G, const qd_c128* V, const double* kx,
                                  const double* ky, int nx, int ny, double dt, int nsteps, int nout, qd_c128* snap,
                                  void* stream) {
  return rk4_entry("qd_wp2_gmat_ms_rk4", "wp2_gmat_ms", args2(B, ns, G, V, kx, ky, nx, ny, stream), psi, dt, nsteps,
                   nout, snap);
}

extern "C" int qd_wp3_gmat_apply(const qd_c128* psi, int B, const double* G, const qd_c128* v, const double* kx,
                                 const double* ky, const double* kz, int nx, int ny, int nz, qd_c128* out,
                                 void* stream) {
  return apply_entry("qd_wp3_gmat_apply", nullptr, args3(B, 1, G, v, kx, ky, kz, nx, ny, nz, stream), psi, out);
}

extern "C" int qd_wp3_gmat_rk4(qd_c128* psi, int B, const double* G, const qd_c128* v, const double* kx,
                               const double* ky, const double* kz, int nx, int ny, int nz, double dt, int nsteps,
                               int nout, qd_c128* snap, void* stream) {
  return rk4_entry("qd_wp3_gmat_rk4", nullptr, args3(B, 1, G, v, kx, ky, kz, nx, ny, nz, stream), psi, dt, nsteps,
                   nout, snap);
}

extern "C" int qd_wp3_gmat_ms_apply(const qd_c128* psi, int B, int ns, const double* G, const qd_c128* V,
                                    const double* kx, const double* ky, const double* kz, int nx, int ny, int nz,
                                    qd_c128* out, void* stream) {
  return apply_entry("qd_wp3_gmat_ms_apply", "wp3_gmat_ms", args3(B, ns, G, V, kx, ky, kz, nx, ny, nz, stream), psi,
                     out);
}

extern "C" int qd_wp3_gmat_ms_rk4(qd_c128* psi, int B, int ns, const double* G, const qd_c128* V, const double* kx,
                                  const double* ky, const double* kz, int nx, int ny, int nz, double dt, int nsteps,
                                  int nout, qd_c128* snap, void* stream) {
  return rk4_entry("qd_wp3_gmat_ms_rk4", "wp3_gmat_ms", args3(B, ns, G, V, kx, ky, kz, nx, ny, nz, stream), psi, dt,
                   nsteps, nout, snap);
}
