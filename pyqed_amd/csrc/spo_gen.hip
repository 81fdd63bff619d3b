// spo_gen.hip — split-operator propagation on ANY grid (every size the reference's SPO classes accept): the host
// side.  The decisions are fft_plan.hpp's (plain C++, enumerated on the host by tests/test_fft_plan_host.py), the
// device code is in fft_lds.hpp and spo_gen_kernels.hpp; this file builds the tables and executes the plans.
//
// The reference transforms with scipy.fftpack / numpy.fft (pocketfft), which take every length
// (wpd.py:225-273 SPO, :692-758 SPO2, :1349-1411 SPO3).  spo.hip's register / Stockham kernels cover
// powers of two in [16, 1024]; this file serves every other grid with the same pass structure:
//
//   an axis plan per grid axis (axis_plan: mixed radix, Bluestein or direct DFT, by its length)
//
//   one fused LDS pass per axis (spo_axis_kernel): a tile of G outer rows x C consecutive inner columns
//   (C * 16 B contiguous per line element, the whole [L][ns] row when C == ns) is loaded once, then
//     [IFFT] -> [U1 point op] -> [snapshot] -> [U2 point op] -> [FFT] -> [k_y phase] -> [FFT * K * IFFT]
//   run on it in LDS and it is stored once.  Point operators (exp(-i V dt/2) per grid point, any ns)
//   need every state of a point, i.e. the last (contiguous) axis with C == ns; KMUL (exp_K / N) is the
//   outermost axis's FFT -> multiply -> IFFT.  The step sequence is spo.hip's (qd_spo2_run_ex /
//   qd_spo3_run): both V/2 halves of every Strang step applied, as the reference's return_states=True
//   arithmetic (wpd.py:723-730), or the merged V structure (wpd.py:736-755).
//   A pass that does not fit the LDS budget (DIRECT axes, ns * M too large for a fused row) runs
//   unfused: axis transforms, a point-operator kernel (thread per (point, state), any ns) and a
//   k-space multiply, with one grid-sized scratch buffer.
//
//   2D grids alternate two layouts between the passes (nd_layout): the row pass reads [x][y][s] rows and writes
//   [y][x][s], the kinetic pass reads those x lines contiguously (exp_K / N transposed to match) and writes [x][y][s]
//   back, so every pass loads whole contiguous lines and only the stores are strided (fire-and-forget, off the
//   dependent chain): 200^2 x 2 24.3 -> 22.5 us per step, 1000^2 x 2 143 -> 134 (profiles/r04/spo/spo_xpose_ab.txt).
//   3D grids could rotate their layouts the same way but lose at 96^3 and above (see nd_layout).
//
//   SPO (1D, wpd.py:225-273): one persistent workgroup per wavepacket, all steps in LDS when the line
//   fits; otherwise one launch sequence per step.
#include "fft_lines.hpp"
#include "spo_gen_kernels.hpp"

namespace qd {
namespace spog {

inline int grid_for(long n) { return (int)std::max<long>(1, std::min<long>((n + 255) / 256, 8192)); }

// The kernels' view of a planned axis, its tables built in the ax.slots slots at tab.
int make_fft(const AxisPlan& ax, c128* tab, Fft& f, hipStream_t st) {
  const int L = ax.L, M = ax.M;
  f.L = L;
  f.M = M;
  f.kind = ax.kind;
  f.nst = ax.nst;
  std::copy(ax.R, ax.R + MAX_ST, f.R);
  std::copy(ax.Ns, ax.Ns + MAX_ST, f.Ns);
  std::copy(ax.dnb, ax.dnb + MAX_ST, f.dnb);
  std::copy(ax.dns, ax.dns + MAX_ST, f.dns);
  f.dM = ax.dM;
  f.tw = tab + ax.tw;
  f.chirp = f.bhat = nullptr;
  hipLaunchKernelGGL(twiddle_table_kernel, dim3((M + 255) / 256), dim3(256), 0, st, M, tab + ax.tw);
  QD_HIP(hipGetLastError());
  if (ax.refused) {
    set_error("spo: FFT plan of length %d needs %d stages (max %d)", M, ax.nst, MAX_ST);
    return QD_EINVAL;
  }
  if (ax.kind == BLUESTEIN) {
    c128* chirp = tab + ax.chirp;
    c128* b = tab + ax.b;
    c128* bhat = tab + ax.bhat;
    hipLaunchKernelGGL(chirp_kernel, dim3((M + 255) / 256), dim3(256), 0, st, L, M, chirp, b);
    hipLaunchKernelGGL(bhat_kernel, dim3((M + 255) / 256), dim3(256), 0, st, M, (const c128*)b, (const c128*)f.tw, bhat);
    QD_HIP(hipGetLastError());
    f.chirp = chirp;
    f.bhat = bhat;
  }
  return QD_OK;
}

// ---------------------------------------------------------------- executor
struct Exec {
  int D = 0;
  int n[3] = {1, 1, 1};
  int ns = 1;
  long npts = 0;
  AxisPlan ax[3];
  Fft f[3];
  hipStream_t st = nullptr;
  c128* psi = nullptr;
  c128* tmp = nullptr;     // grid-sized scratch (unfused passes)
  const c128* Ks = nullptr;   // exp_K / N
  const c128* KsT = nullptr;  // exp_K / N in the kinetic pass's input layout (xpose): [n1][n0]
  const c128* Ky = nullptr;   // Jacobi k_y phase [n0][n1] (D == 2)
  NdLayout lay{};             // 2D: alternating layouts (file header); psi [n0][n1][ns] <-> tmp [n1][n0][ns]

  long outer(int d) const { long o = 1; for (int k = 0; k < d; ++k) o *= n[k]; return o; }
  long inner(int d) const { long i = ns; for (int k = d + 1; k < D; ++k) i *= n[k]; return i; }

  int set_axis(int d, const AxisPlan& a, c128* tab) {
    ax[d] = a;
    return make_fft(a, tab, f[d], st);
  }

  struct Store {   // F_XOUT map (see Flags)
    long nlo, sh, sl, se;
  };
  // one spo_axis_kernel pass with plan p, tiled as t, over the [O][p.L][I] grid at src, stored to dst ([p.L][O][I]
  // with F_XOUT)
  int launch_tile(const Fft& p, const PassPlan& t, long O, long I, int flags, const c128* U1, const c128* U2,
                  c128* snap, c128* src, c128* dst, const c128* K, Store sm = {1, 0, 0, 0}) {
    AxisArgs a;
    a.psi = src;
    a.out = dst;
    a.sh = sm.sh;
    a.sl = sm.sl;
    a.se = sm.se;
    a.dlo = make_fdiv((unsigned)sm.nlo);
    a.O = (int)O;
    a.L = p.L;
    a.I = (int)I;
    a.C = t.C;
    a.dLC = t.dLC;
    a.dC = t.dC;
    a.dLns = t.dLns;
    a.dns = t.dns;
    a.G = t.G;
    a.flags = flags;
    a.ns = ns;
    a.U1 = U1;
    a.U2 = U2;
    a.snap = snap;
    a.K = K;
    a.Ky = Ky;
    a.twl = t.twl;
    // (round 4 tried staging the pass's operators in LDS with the tile: 500^2 x 2 50.3 vs 43.8 us per step, the larger
    // tile lowering the workgroups per CU; profiles/r04/spo/spo_any_aux_*.txt)
    (void)hipFuncSetAttribute((const void*)spo_axis_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
    hipLaunchKernelGGL(spo_axis_kernel, dim3((unsigned)t.gx, (unsigned)t.gy), dim3(256), t.lds, st, p, a);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // xpose passes (D == 2): the row pass over psi ([n0][n1][ns] rows), stored transposed into tmp when xout; the
  // kinetic pass over tmp's x lines ([n1][n0][ns]) with exp_K / N transposed, stored transposed back into psi
  int row_pass(int flags, const c128* U1, const c128* U2, c128* snap, bool xout) {
    return launch_tile(f[1], lay.row, n[0], ns, flags | (xout ? F_XOUT : 0), U1, U2, snap, psi, xout ? tmp : psi, Ks,
                       Store{n[0], 0, ns, (long)n[0] * ns});
  }
  int kin_pass() {
    return launch_tile(f[0], lay.kin, n[1], ns, F_KMUL | F_KROW | F_XOUT, nullptr, nullptr, nullptr, tmp, psi, KsT,
                       Store{n[1], 0, ns, (long)n[1] * ns});
  }

  int transform(int d, bool inv) {
    const long O = outer(d), I = inner(d);
    const PassPlan t = pass_plan(ax[d], O, I, ns, false);
    if (t.fused) return launch_tile(f[d], t, O, I, inv ? F_INV : F_FWD, nullptr, nullptr, nullptr, psi, psi, Ks);
    // direct DFT from HBM into the scratch grid, then back
    const int L = n[d];
    const long lines = O * I;
    const dim3 grid((L + 255) / 256, (unsigned)std::min<long>(lines, 65535));
    if (inv)
      hipLaunchKernelGGL(dft_axis_kernel<true>, grid, dim3(256), 0, st, (const c128*)psi, tmp, O, L, I, f[d].tw);
    else
      hipLaunchKernelGGL(dft_axis_kernel<false>, grid, dim3(256), 0, st, (const c128*)psi, tmp, O, L, I, f[d].tw);
    QD_HIP(hipGetLastError());
    QD_TRY(copy_device(psi, tmp, (size_t)npts * ns * sizeof(c128), st));
    return QD_OK;
  }

  int pointop(const c128* U) {
    hipLaunchKernelGGL(pointop_kernel, dim3(grid_for(npts * ns)), dim3(256), 0, st, (const c128*)psi, tmp, U, npts, ns);
    QD_HIP(hipGetLastError());
    QD_TRY(copy_device(psi, tmp, (size_t)npts * ns * sizeof(c128), st));
    return QD_OK;
  }

  int kmul(const c128* K) {
    hipLaunchKernelGGL(kmul_kernel, dim3(grid_for(npts * ns)), dim3(256), 0, st, psi, K, npts * ns, ns);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }

  // One pass over axis d with the ops of `flags` (F_PT*, F_SNAP, F_KY: last axis; F_KMUL: axis 0).
  int pass(int d, int flags, const c128* U1, const c128* U2, c128* snap) {
    const bool pt = flags & (F_PT1 | F_PT2 | F_SNAP | F_KY);
    const PassPlan t = pass_plan(ax[d], outer(d), inner(d), ns, pt);
    if (t.fused) return launch_tile(f[d], t, outer(d), inner(d), flags, U1, U2, snap, psi, psi, Ks);
    int rc;
    if ((flags & F_INV) && (rc = transform(d, true))) return rc;
    if ((flags & F_PT1) && (rc = pointop(U1))) return rc;
    if (flags & F_SNAP)
      QD_TRY(copy_device(snap, psi, (size_t)npts * ns * sizeof(c128), st));
    if ((flags & F_PT2) && (rc = pointop(U2))) return rc;
    if ((flags & F_FWD) && (rc = transform(d, false))) return rc;
    if ((flags & F_KY) && (rc = kmul(Ky))) return rc;
    if (flags & F_KMUL) {
      if ((rc = transform(d, false))) return rc;
      if ((rc = kmul(Ks))) return rc;
      if ((rc = transform(d, true))) return rc;
    }
    return QD_OK;
  }
};

// step_sequence on x: with alternating layouts (D == 2) the last-axis passes are row passes that store into the other
// layout exactly when they end in a forward transform, and the kinetic pass is the one over that layout.
int run_nd(Exec& x, const c128* Uh, const c128* Ufull, int nsteps, int nout, const SnapSink& snap, bool ky) {
  const c128* U[3] = {nullptr, Uh, Ufull};   // PointOp
  return step_sequence(x.D, nsteps, nout, (bool)snap, Ufull != nullptr, ky, [&](const StepPass& s) -> int {
    c128* sp = s.rec >= 0 ? snap.at(s.rec) : nullptr;
    int rc;
    if (!x.lay.xpose) rc = x.pass(s.axis, s.flags, U[s.u1], U[s.u2], sp);
    else if (s.axis == 0) rc = x.kin_pass();
    else rc = x.row_pass(s.flags, U[s.u1], U[s.u2], sp, (s.flags & F_FWD) != 0);
    if (rc) return rc;
    return s.rec >= 0 ? snap.taken(s.rec, x.st) : QD_OK;
  });
}

// The kinetic step of the 1D run on lines beyond the LDS plans, psi [B][nx].
struct Line1d {
  Exec x;            // four-step: the [B][L1][L2] view
  c128* psi;
  c128* tmp;
  const c128* ks;    // exp_K / nx (four-step: in the four-step's k order)
  const c128* tw;    // exp(-2 pi i m / nx)
  long total;
  int nx, B, L1, L2;
  hipStream_t st;

  // Smooth lengths L = L1 L2 with both factors LDS-plannable run the four-step FFT: the line viewed as [L1][L2]
  // (n = L2 n1 + n2), FFT_L1 over n1 (stride L2), twiddle w_L^(n2 k1), FFT_L2 over n2 (contiguous) leaves
  // X[k1 + L1 k2] at L2 k1 + k2; the kinetic factor is applied in that order (exp_K permuted once) and the inverse
  // runs the same passes backwards, so no transpose is ever made.
  int kstep_fourstep() {
    int r;
    if ((r = x.pass(1, F_FWD, nullptr, nullptr, nullptr))) return r;
    hipLaunchKernelGGL(fourstep_twiddle_kernel, dim3(grid_for(total)), dim3(256), 0, st, psi, total, L1, L2, tw, 0);
    if ((r = x.pass(2, F_FWD, nullptr, nullptr, nullptr))) return r;
    hipLaunchKernelGGL(bcast_mul_kernel, dim3(grid_for(total)), dim3(256), 0, st, psi, ks, total, nx);
    if ((r = x.pass(2, F_INV, nullptr, nullptr, nullptr))) return r;
    hipLaunchKernelGGL(fourstep_twiddle_kernel, dim3(grid_for(total)), dim3(256), 0, st, psi, total, L1, L2, tw, 1);
    if ((r = x.pass(1, F_INV, nullptr, nullptr, nullptr))) return r;
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
  // Other lengths: direct DFT lines, one launch sequence per step on the [B][nx] grid
  int kstep_direct() {
    const dim3 grid((nx + 255) / 256, (unsigned)std::min<long>(B, 65535));
    hipLaunchKernelGGL(dft_axis_kernel<false>, grid, dim3(256), 0, st, (const c128*)psi, tmp, (long)B, nx, 1L, tw);
    hipLaunchKernelGGL(bcast_mul_kernel, dim3(grid_for(total)), dim3(256), 0, st, tmp, ks, total, nx);
    hipLaunchKernelGGL(dft_axis_kernel<true>, grid, dim3(256), 0, st, (const c128*)tmp, psi, (long)B, nx, 1L, tw);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
  int kstep() { return L1 ? kstep_fourstep() : kstep_direct(); }
};

}  // namespace spog

// Unnormalised DFT along the middle axis of the [O][L][I] grid x, in place (inv: the conjugate kernel), for pyqed.fft's
// any-length transforms (fft.hip).  Lengths the LDS plans take (mixed radix <= 5120, Bluestein with M <= 5120) run one
// spo_axis_kernel pass; longer lengths that split as L1 L2 with both factors LDS-plannable run the four-step FFT and
// leave X[k1 + L1 k2] at slot L2 k1 + k2 (p.l2 = L2; p.l2 = 0: natural order); anything else a direct DFT.
int fft_lines_run(const LinesPlan& p, c128* x, bool inv, hipStream_t st) {
  using namespace spog;
  const long total = p.O * p.L * p.I;
  Exec e;
  e.st = st;
  e.psi = x;
  e.ns = (int)p.I;
  e.n[0] = (int)p.O;
  e.npts = p.O * p.L;
  int rc;
  void* w = nullptr;
  if ((rc = workspace(WS_MISC, (p.slots + (p.scratch ? (size_t)total : 0)) * sizeof(c128), &w, st))) return rc;
  c128* tab = (c128*)w;
  if (p.L1) {
    c128* twL = tab + p.tw_l;
    e.D = 3;
    e.n[1] = p.L1;
    e.n[2] = p.L2;
    if ((rc = e.set_axis(1, p.ax[0], tab))) return rc;
    if ((rc = e.set_axis(2, p.ax[1], tab + p.ax[0].slots))) return rc;
    hipLaunchKernelGGL(twiddle_table_kernel, dim3((p.L + 255) / 256), dim3(256), 0, st, p.L, twL);
    QD_HIP(hipGetLastError());
    if ((rc = e.transform(1, inv))) return rc;
    hipLaunchKernelGGL(fourstep_twiddle_inner_kernel, dim3(grid_for(total)), dim3(256), 0, st, x, total, p.L1, p.L2,
                       p.I, (const c128*)twL, inv ? 1 : 0);
    QD_HIP(hipGetLastError());
    return e.transform(2, inv);
  }
  e.D = 2;
  e.n[1] = p.L;
  e.tmp = tab + p.slots;
  if ((rc = e.set_axis(1, p.ax[0], tab))) return rc;
  return e.transform(1, inv);
}

int fft_lines(c128* x, long O, int L, long I, bool inv, hipStream_t st, int* l2) {
  const LinesPlan p = fft_lines_plan(O, L, I);
  *l2 = p.l2;
  return fft_lines_run(p, x, inv, st);
}

// Generic SPO2 / SPO3 run (any grid, any ns).  dims = {nx, ny} or {nx, ny, nz}; expK [dims] unscaled;
// expKy [nx][ny] (2D Jacobi) or null; expV (merged V structure) or null.
int spo_generic_run(c128* psi, const c128* expVh, const c128* expV, const c128* expK, const c128* expKy,
                    const int* dims, int D, int ns, int nsteps, int nout, const SnapSink& snap, hipStream_t st) {
  using namespace spog;
  WsScope wss_(st);
  Exec x;
  x.D = D;
  x.ns = ns;
  x.st = st;
  x.psi = psi;
  x.npts = 1;
  size_t tabs = 0;
  for (int d = 0; d < D; ++d) {
    x.n[d] = dims[d];
    x.npts *= dims[d];
    x.ax[d] = axis_plan(dims[d]);
    tabs += x.ax[d].slots;
  }
  const size_t slots = (size_t)x.npts * ns + 2 * x.npts + tabs;   // tmp grid + exp_K / N (+ transposed) + tables
  void* w = nullptr;
  int rc = workspace(WS_SPO, slots * sizeof(c128), &w, st);
  if (rc) return rc;
  x.tmp = (c128*)w;
  c128* ks = x.tmp + (size_t)x.npts * ns;
  c128* tab = ks + x.npts;
  for (int d = 0; d < D; ++d) {
    if ((rc = make_fft(x.ax[d], tab, x.f[d], st))) return rc;
    tab += x.ax[d].slots;
  }
  hipLaunchKernelGGL(scale_copy_kernel, dim3(grid_for(x.npts)), dim3(256), 0, st, expK, ks, x.npts,
                     1.0 / (double)x.npts);
  QD_HIP(hipGetLastError());
  x.Ks = ks;
  x.Ky = expKy;
  x.lay = nd_layout(x.ax, D, x.n, ns, nsteps);
  for (int d = 0; d < D; ++d)
    note_path(x.f[d].kind == DIRECT ? "spo_axis_direct" : x.f[d].kind == BLUESTEIN ? "spo_axis_bluestein"
                                                                                    : "spo_axis_mixed");
  note_path(x.lay.xpose ? "spo_layout_alternating" : "spo_layout_in_place");
  if (x.lay.xpose) {
    c128* kt = tab;   // behind the plan tables
    hipLaunchKernelGGL(scale_transpose_kernel, dim3(grid_for(x.npts)), dim3(256), 0, st, expK, kt, dims[0], dims[1],
                       1.0 / (double)x.npts);
    QD_HIP(hipGetLastError());
    x.KsT = kt;
  }
#ifdef QD_PHASE_TIMING
  {
    unsigned long long z[2][6] = {};
    QD_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_spo_tim), z, sizeof(z), 0, hipMemcpyHostToDevice, st));
    rc = run_nd(x, expVh, expV, nsteps, nout, snap, expKy != nullptr);
    QD_HIP(hipStreamSynchronize(st));
    QD_HIP(hipMemcpyFromSymbol(z, HIP_SYMBOL(g_spo_tim), sizeof(z)));
    const char* nm[5] = {"load", "inv_fft", "point_ops", "fwd_fft_or_kin", "store"};
    for (int k = 0; k < 2; ++k) {
      if (!z[k][5]) continue;
      fprintf(stderr, "[spo_axis phase timing] %s pass, us per block:", k ? "kinetic" : "row");
      for (int q = 0; q < 5; ++q) fprintf(stderr, " %s %.3f", nm[q], (double)z[k][q] / z[k][5] / 100.0);
      fprintf(stderr, " (%llu blocks)\n", z[k][5]);
    }
    return rc;
  }
#else
  return run_nd(x, expVh, expV, nsteps, nout, snap, expKy != nullptr);
#endif
}

// Generic 1D SPO.run (any nx), B wavepackets [B][nx].
int spo1d_generic_run(c128* psi, const c128* expV, const c128* expVh, const c128* expK, int nx, int B, int nt,
                      int nout, c128* snap, hipStream_t st) {
  using namespace spog;
  WsScope wss_(st);
  const long n = (long)nx * B;
  const AxisPlan ax = axis_plan(nx);
  const size_t slots = ax.slots + (size_t)2 * n + nx;
  void* w = nullptr;
  int rc = workspace(WS_MISC, slots * sizeof(c128), &w, st);
  if (rc) return rc;
  c128* tab = (c128*)w;
  c128* tmp = tab + ax.slots;
  c128* ks = tmp + 2 * n;
  Fft f;
  if ((rc = make_fft(ax, tab, f, st))) return rc;
  note_path(f.kind == DIRECT ? "spo1d_long" : f.kind == BLUESTEIN ? "spo1d_bluestein" : "spo1d_mixed");
  if (f.kind != DIRECT) {
    int twl;
    const size_t lds = tile_lds(f.M, 1, &twl);
    (void)hipFuncSetAttribute((const void*)spo1d_gen_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
    hipLaunchKernelGGL(spo1d_gen_kernel, dim3(B), dim3(256), lds, st, f, psi, expV, expVh, expK, nt, nout, snap, twl);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
  // Lines beyond the LDS plans: the four-step FFT where the length splits into two mixed-radix factors, else the
  // direct DFT (Line1d).
  Line1d k;
  k.psi = psi;
  k.tmp = tmp;
  k.ks = ks;
  k.tw = f.tw;
  k.total = n;
  k.nx = nx;
  k.B = B;
  k.L1 = fourstep_split(nx, false);
  k.L2 = k.L1 ? nx / k.L1 : 0;
  k.st = st;
  note_path(k.L1 ? "spo1d_fourstep" : "spo1d_direct");
  const long total = n;
  auto vmul = [&](const c128* V) -> int {   // psi[b][k] *= V[k]
    hipLaunchKernelGGL(bcast_mul_kernel, dim3(grid_for(total)), dim3(256), 0, st, psi, V, total, nx);
    QD_HIP(hipGetLastError());
    return QD_OK;
  };
  if (k.L1) {
    const AxisPlan a1 = axis_plan(k.L1), a2 = axis_plan(k.L2);
    void* w2 = nullptr;
    if ((rc = workspace(WS_MISC, (a1.slots + a2.slots) * sizeof(c128), &w2, st))) return rc;
    c128* tab2 = (c128*)w2;
    Exec& x = k.x;
    x.D = 3;
    x.n[0] = B;
    x.n[1] = k.L1;
    x.n[2] = k.L2;
    x.ns = 1;
    x.npts = total;
    x.st = st;
    x.psi = psi;
    x.tmp = tmp;
    if ((rc = x.set_axis(1, a1, tab2))) return rc;
    if ((rc = x.set_axis(2, a2, tab2 + a1.slots))) return rc;
    hipLaunchKernelGGL(fourstep_kperm_kernel, dim3(grid_for(nx)), dim3(256), 0, st, expK, ks, k.L1, k.L2, 1.0 / nx);
    QD_HIP(hipGetLastError());
  } else {
    hipLaunchKernelGGL(scale_copy_kernel, dim3(grid_for(nx)), dim3(256), 0, st, expK, ks, (long)nx, 1.0 / nx);
    QD_HIP(hipGetLastError());
  }
  if ((rc = vmul(expVh))) return rc;
  const int nblk = nt / nout;
  const int nsnap = nblk > 0 ? nblk - 1 : 0;
  for (int blk = 1; blk < nblk; ++blk) {
    for (int s = 0; s < nout; ++s) {
      if ((rc = k.kstep())) return rc;
      if ((rc = vmul(expV))) return rc;
    }
    if (snap)
      for (int b = 0; b < B; ++b)
        QD_TRY(copy_device(snap + ((size_t)b * nsnap + (blk - 1)) * nx, psi + (size_t)b * nx, nx * sizeof(c128), st));
  }
  if ((rc = k.kstep())) return rc;
  return vmul(expVh);
}

}  // namespace qd
