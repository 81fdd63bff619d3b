// spo.hip — split-operator wavepacket propagation on power-of-two grids, 1D, 2D and 3D, multi-state.
//
// Replaces the Strang loops of pyqed/wpd.py:
//   SPO.run   (wpd.py:225-273, 1D single surface)             -> qd_spo1d_run
//   SPO2.run  (wpd.py:692-758; _KEO_linear wpd.py:837-848, Jacobi 850-887) -> qd_spo2_run[_ex], qd_spo2_run_batch
//   SPO3.run  (wpd.py:1418-1432, FFT kinetic step)            -> qd_spo3_run; 64^3 separable: spo3_sep64_run
// Every other grid runs the any-size engine (spo_gen.hip); this file is the host side of the specialised path:
//   spo_plan.hpp       which shapes the specialised kernels take, each pass's kernel family, template values and
//                      launch geometry (plain C++, enumerated by tests/test_spo_plan_host.py), the typed dispatch
//   spo_fft_pow2.hpp   twiddles, Stockham LDS FFT, 256-point and 64-point register transforms (shared with fft.hip)
//   spo_kernels.hpp    row / column passes (LDS, latency-shaped, 256-point, batch), the 1D kernel, spo_expv_kernel
//   spo_kernels_3d.hpp mid-axis passes, 64-point passes along every axis, axis_factor_kernel
//
// Step layout (psi [nx][ny]([nz])[ns], state index fastest, as the reference):
//   row pass    (contiguous axis): [IFFT] -> V/2 -> [snapshot] -> [V/2] -> [FFT] (-> k_y phase, Jacobi)
//   mid pass    (3D, y):           FFT or IFFT
//   column pass (x):               FFT_x -> * exp_K / points -> IFFT_x
// A run of n Strang steps V/2 K V/2 is: row(V/2, FFT) [mid], then n x {col [mid^-1], row [mid]}, the last row pass
// without the trailing V/2 + FFT.  Both V/2 are applied separately (no V/2 V/2 -> V merge) so every step is the
// reference's return_states=True arithmetic; expV selects the merged structure of return_states=False.  psi is read
// and written once per kernel; exp_V_half (ns^2 per point) once per row pass, exp_K once per column pass.
// Each pass family a run takes is noted once (note_path) as <spo2|spo3>_<family>[_c<tile width>].
#include "spo_plan.hpp"
#include "spo_kernels_3d.hpp"

namespace qd {
namespace {

int twiddles(int L, hipStream_t st, c128* tw) {
  hipLaunchKernelGGL(twiddle_kernel, dim3((L + 255) / 256), dim3(256), 0, st, L, tw);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// After a typed dispatch: a pass with no kernel is an internal error of the plan, never a silent no-op.
int launched(bool hit, const Pass& p) {
  QD_CHECK_ARG(hit, "spo: internal: no kernel for pass kind %d L=%d C=%d NS=%d", p.kind, p.L, p.C, p.NS);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

void note_pass(const char* prefix, const Pass& p) {
  char name[48];
  note_path(pass_name(p, prefix, name, sizeof name));
}

// Row pass p over psi: `U` the point operator of this pass, `flags` its RowFlags.  Batches (B members, blockIdx.y):
// psi / snap offset by wstride / sstride per member.
int launch_row(const Pass& p, c128* psi, const c128* U, const c128* tw, int ns, int flags, c128* snap,
               const c128* expKy, hipStream_t st, int B = 1, size_t wstride = 0, size_t sstride = 0) {
  const dim3 g(p.gx, p.gy, p.gz), b(p.block);
  return launched(dispatch_pass(p, [&](auto K, auto L_, auto, auto NS_) {
    constexpr int k = decltype(K)::value, L = decltype(L_)::value, NS = decltype(NS_)::value;
    if constexpr (k == ROW_Q16)
      hipLaunchKernelGGL((p.ky ? spo2_row_q16_kernel<NS, true> : spo2_row_q16_kernel<NS, false>), g, b, 0, st, psi, U,
                         tw, flags, snap, expKy, wstride, sstride);
    else if constexpr (k == ROW_64) hipLaunchKernelGGL(spo_row64_kernel<NS>, g, b, 0, st, psi, U, tw, flags, snap);
    else if constexpr (k == ROW_FAST)
      hipLaunchKernelGGL((spo2_row_fast_kernel<L, NS>), g, b, p.lds, st, psi, U, tw, flags, snap, expKy);
    else if constexpr (k == ROW_LDS)
      hipLaunchKernelGGL(spo2_row_kernel<L>, g, b, p.lds, st, psi, U, tw, L, ns, flags, snap, expKy);
    else if constexpr (k == ROW_WAVE)
      hipLaunchKernelGGL(spo2_row_wave_kernel<4>, g, b, 0, st, psi, U, tw, flags, snap, B, wstride, sstride);
    return k == ROW_Q16 || k == ROW_64 || k == ROW_FAST || k == ROW_LDS || k == ROW_WAVE;
  }), p);
}

// Column pass p: `pitch` = points per row of psi (the number of columns).
int launch_col(const Pass& p, c128* psi, const c128* expKT, const c128* tw, int pitch, int ns, hipStream_t st,
               size_t wstride = 0) {
  const dim3 g(p.gx, p.gy, p.gz), b(p.block);
  return launched(dispatch_pass(p, [&](auto K, auto L_, auto C_, auto NS_) {
    constexpr int k = decltype(K)::value, L = decltype(L_)::value, C = decltype(C_)::value, NS = decltype(NS_)::value;
    if constexpr (k == COL_Q16)
      hipLaunchKernelGGL(spo2_col_q16_kernel<NS>, g, b, 0, st, psi, expKT, tw, p.gx, pitch, wstride);
    else if constexpr (k == COL_64) hipLaunchKernelGGL((spo_col64_kernel<C, NS>), g, b, 0, st, psi, expKT, tw, pitch);
    else if constexpr (k == COL_FAST)
      hipLaunchKernelGGL((spo2_col_fast_kernel<L, C, NS>), g, b, p.lds, st, psi, expKT, tw, pitch);
    else if constexpr (k == COL_LDS)
      hipLaunchKernelGGL((spo2_col_kernel<L, C>), g, b, p.lds, st, psi, expKT, tw, pitch, ns);
    else if constexpr (k == COL_TILE)
      hipLaunchKernelGGL(spo2_col_tile8_kernel<8>, g, b, 0, st, psi, expKT, tw, wstride);
    return k == COL_Q16 || k == COL_64 || k == COL_FAST || k == COL_LDS || k == COL_TILE;
  }), p);
}

// Mid pass p of a 3D grid: forward or inverse transform along y, `inner` = nz ns.
int launch_mid(const Pass& p, c128* psi, const c128* tw, int inner, bool inv, hipStream_t st) {
  const dim3 g(p.gx), b(p.block);
  return launched(dispatch_pass(p, [&](auto K, auto L_, auto C_, auto) {
    constexpr int k = decltype(K)::value, L = decltype(L_)::value, C = decltype(C_)::value;
    return dispatch_int<0, 1>(inv, [&](auto I) {
      constexpr bool INV = decltype(I)::value != 0;
      if constexpr (k == MID_64) hipLaunchKernelGGL((spo_mid64_kernel<C, INV>), g, b, 0, st, psi, tw, inner);
      else if constexpr (k == MID_FAST)
        hipLaunchKernelGGL((spo_mid_fast_kernel<L, C, INV>), g, b, 0, st, psi, tw, inner);
      else if constexpr (k == MID_LDS) hipLaunchKernelGGL((spo_mid_kernel<L, C, INV>), g, b, 0, st, psi, tw, inner);
      return k == MID_64 || k == MID_FAST || k == MID_LDS;
    });
  }), p);
}

// The prologue of a power-of-two run, queued on the stream: scratch for exp_K transposed to [columns][nx] and scaled by
// 1 / points (the FFT normalisation), and the twiddle table of every axis.
struct Pow2Tables { c128 *expKT, *tw[3]; };
int pow2_prologue(const c128* expK, const int* dims, int D, hipStream_t st, Pow2Tables* t) {
  size_t cols = 1, ntw = 0;
  for (int a = 0; a < D; ++a) {
    if (a) cols *= dims[a];
    ntw += dims[a];
  }
  const size_t nk = dims[0] * cols;
  void* w = nullptr;
  QD_TRY(workspace(WS_SPO, (nk + ntw) * sizeof(c128), &w, st));
  t->expKT = (c128*)w;
  c128* tw = t->expKT + nk;
  for (int a = 0; a < D; tw += dims[a++]) {
    t->tw[a] = tw;
    QD_TRY(twiddles(dims[a], st, tw));
  }
  hipLaunchKernelGGL(transpose_scale_kernel, dim3((int)std::min<size_t>((nk + 255) / 256, 4096)), dim3(256), 0, st,
                     expK, dims[0], (int)cols, 1.0 / (double)nk, t->expKT);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// The Strang loop of the power-of-two runs.  row(flags, snapshot, point operator) is the row pass, kin() the kinetic
// passes in front of it (column; 3D: column, inverse mid), fwd() what follows a row pass that ends on its forward
// transform (3D: forward mid).  expV: the merged structure (IFFT -> V -> [snapshot] -> FFT per step, then the tail
// K, V/2 of wpd.py:752-755); else both halves, IFFT -> V/2 -> [snapshot] -> V/2 -> FFT, and the last step stops
// after its first half.  ky: ROW_KY on the passes that end on a forward transform (Jacobi).
template <typename Row, typename Kin, typename Fwd>
int strang_loop(int nsteps, int nout, const SnapSink& snap, hipStream_t st, const c128* expVh, const c128* expV, int ky,
                Row&& row, Kin&& kin, Fwd&& fwd) {
  QD_TRY(row(ROW_VH1 | ROW_FWD | ky, nullptr, expVh));
  QD_TRY(fwd());
  for (int s = 1; s <= nsteps; ++s) {
    QD_TRY(kin());
    const bool take = snap && (s % nout == 0);
    int flags = ROW_INV | ROW_VH1 | (take ? ROW_SNAP : 0);
    if (expV) flags |= ROW_FWD | ky;
    else if (s < nsteps) flags |= ROW_VH2 | ROW_FWD | ky;
    QD_TRY(row(flags, take ? snap.at(s / nout - 1) : nullptr, expV ? expV : expVh));
    if (take) QD_TRY(snap.taken(s / nout - 1, st));
    if (flags & ROW_FWD) QD_TRY(fwd());
  }
  if (expV) {
    QD_TRY(kin());
    QD_TRY(row(ROW_INV | ROW_VH1, nullptr, expVh));
  }
  return QD_OK;
}
int no_pass() { return QD_OK; }

SnapSink plain_sink(qd_c128* snap, size_t grid_elems) {
  SnapSink k;
  k.snap = (c128*)snap;
  k.grid_elems = grid_elems;
  return k;
}

// The observer of an observed run; nrec: records per member (the strides between the members of a batch)
SpoObserver make_observer(const int* dims, int ndim, const double* const x[3], int ns, int B, const qd_c128* basis,
                          double weight, qd_c128* rdm, double* mom, size_t nrec) {
  SpoObserver o;
  o.ndim = ndim;
  for (int d = 0; d < ndim; ++d) {
    o.dims[d] = dims[d];
    o.x[d] = x[d];
  }
  o.ns = ns;
  o.B = B;
  o.basis = (const c128*)basis;
  o.weight = weight;
  o.rdm = (c128*)rdm;
  o.mom = mom;
  o.rdm_bstride = nrec * ns * ns;
  o.mom_bstride = nrec * ndim * ns;
  return o;
}

}  // namespace

// SPO3 on a 64 x 64 x 64 grid with a separable kinetic propagator (qd_spo3_run_axes): three passes per step, each the
// whole axis propagator F^-1 diag(e_a / n) F on its lines with the 64-point register transforms -- z (contiguous,
// with the point operators: the previous step's closing half, the snapshot, this step's opening half), y (mid axis),
// x (columns) -- where the non-separable path needs four (the x pass multiplies the 3-D exp_K between the y and z
// transforms, so both are undone in passes of their own).
int spo3_sep64_run(c128* psi, const c128* Vh, const c128* const m[3], int ns, int nsteps, int nout,
                   const SnapSink& snap, hipStream_t st) {
  void* w = nullptr;
  QD_TRY(workspace(WS_SPO, (size_t)4 * 64 * sizeof(c128), &w, st));
  c128* tw = (c128*)w;
  c128* d = tw + 64;
  QD_TRY(twiddles(64, st, tw));
  hipLaunchKernelGGL(axis_factor_kernel, dim3(3), dim3(64), 0, st, m[0], m[1], m[2], 64, d);
  QD_HIP(hipGetLastError());
  const int rows = 64 * 64, nyz = 64 * 64, inner = 64 * ns;
  // one launch per pass with NS = ns states compiled in (1 or 2: spo3_axes_sink); the y pass tiles 4 ns inner indices
  auto pass = [&](auto&& launch) -> int {
    QD_CHECK_ARG((dispatch_int<1, 2>(ns, launch)), "spo3_sep64_run: internal: no kernel for ns = %d", ns);
    QD_HIP(hipGetLastError());
    return QD_OK;
  };
  for (int s = 0; s <= nsteps; ++s) {
    // step s's z pass closes step s - 1 (its snapshot) and opens step s; the pass after the last step only closes
    const bool take = snap && s > 0 && s % nout == 0;
    int flags = (s > 0 ? ROW_VH1 : 0) | (take ? ROW_SNAP : 0);
    if (s < nsteps) flags |= ROW_VH2 | ROW_FWD | ROW_KZ;
    c128* sp = take ? snap.at(s / nout - 1) : nullptr;
    QD_TRY(pass([&](auto NS) {
      hipLaunchKernelGGL(spo_row64_kernel<decltype(NS)::value>, dim3(rows / 16), dim3(256), 0, st, psi, Vh, tw, flags,
                         sp, d + 128);
      return true;
    }));
    if (take) QD_TRY(snap.taken(s / nout - 1, st));
    if (s == nsteps) break;
    QD_TRY(pass([&](auto NS) {
      constexpr int N = decltype(NS)::value, C = 4 * N;
      hipLaunchKernelGGL((spo_mid64_kernel<C, false, true>), dim3(64 * (inner / C)), dim3(16 * C), 0, st, psi, tw,
                         inner, d + 64);
      hipLaunchKernelGGL((spo_col64_kernel<4, N>), dim3(nyz / 4), dim3(64 * N), 0, st, psi, (const c128*)d, tw, nyz, 0);
      return true;
    }));
  }
  return QD_OK;
}

}  // namespace qd

using namespace qd;

// qd_spo2_run_ex with its snapshot store behind a sink (qd_common.hpp): the plain entry points pass the caller's
// pointer and no observer, qd_spo2_run_observed the observer and, without snapshots, its scratch slot.
static int spo2_run_sink(qd_c128* psi_, const qd_c128* expVh_, const qd_c128* expV_, const qd_c128* expK_,
                         const qd_c128* expKy_, int nx, int ny, int ns, int nsteps, int nout, const SnapSink& snap,
                         void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi_ && expVh_ && expK_, "qd_spo2_run_ex: null pointer");
  QD_CHECK_ARG(nx >= 1 && ny >= 1 && ns >= 1, "qd_spo2_run_ex: nx=%d ny=%d ns=%d", nx, ny, ns);
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "qd_spo2_run_ex: nsteps=%d nout=%d", nsteps, nout);
  if (nsteps == 0 && !expV_) return QD_OK;
  c128* psi = (c128*)psi_;
  const c128* expKy = (const c128*)expKy_;
  const int dims[2] = {nx, ny};
  const SpoPlan p = spo2_plan(nx, ny, ns, expKy != nullptr);
  note_path(p.special ? "spo2_pow2" : "spo_any");
  if (!p.special)
    return spo_generic_run(psi, (const c128*)expVh_, (const c128*)expV_, (const c128*)expK_, expKy, dims, 2, ns, nsteps,
                           nout, snap, st);
  note_pass("spo2", p.row[0]);
  if (p.row[1].kind != p.row[0].kind) note_pass("spo2", p.row[1]);
  note_pass("spo2", p.col);
  Pow2Tables t;
  QD_TRY(pow2_prologue((const c128*)expK_, dims, 2, st, &t));
  auto row = [&](int flags, c128* sp, const c128* U) {
    return launch_row(p.row[(flags & ROW_KY) != 0], psi, U, t.tw[1], ns, flags, sp, expKy, st);
  };
  auto col = [&]() { return launch_col(p.col, psi, t.expKT, t.tw[0], ny, ns, st); };
  return strang_loop(nsteps, nout, snap, st, (const c128*)expVh_, (const c128*)expV_, expKy ? ROW_KY : 0, row, col,
                     no_pass);
}

extern "C" int qd_spo2_run_ex(qd_c128* psi_, const qd_c128* expVh_, const qd_c128* expV_, const qd_c128* expK_,
                              const qd_c128* expKy_, int nx, int ny, int ns, int nsteps, int nout, qd_c128* snap_,
                              void* stream) {
  return spo2_run_sink(psi_, expVh_, expV_, expK_, expKy_, nx, ny, ns, nsteps, nout,
                       plain_sink(snap_, (size_t)nx * ny * ns), stream);
}

extern "C" int qd_spo2_run(qd_c128* psi_, const qd_c128* expVh_, const qd_c128* expK_, int nx, int ny, int ns,
                           int nsteps, int nout, qd_c128* snap_, void* stream) {
  return qd_spo2_run_ex(psi_, expVh_, nullptr, expK_, nullptr, nx, ny, ns, nsteps, nout, snap_, stream);
}

// qd_spo2_run_batch behind a sink; obs (or null) carries the outputs of all B members, and the members that run one
// at a time observe through a copy of it that points at their own rows.
static int spo2_batch_sink(qd_c128* psi_, int B, const qd_c128* expVh_, const qd_c128* expK_, const qd_c128* expKy_,
                           int nx, int ny, int ns, int nsteps, int nout, qd_c128* snap_, SpoObserver* obs,
                           void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi_ && expVh_ && expK_, "qd_spo2_run_batch: null pointer");
  QD_CHECK_ARG(B >= 1 && B <= 65535, "qd_spo2_run_batch: B=%d outside [1, 65535]", B);
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "qd_spo2_run_batch: nsteps=%d nout=%d", nsteps, nout);
  const size_t grid_elems = (size_t)nx * ny * ns;
  const int nsave = nsteps / nout;
  hipStream_t st = (hipStream_t)stream;
  SnapSink snap = plain_sink(snap_, grid_elems);
  const SpoPlan p = spo2_batch_plan(nx, ny, ns, B, expKy_ != nullptr, obs != nullptr);
  if (obs && nsave) {
    if (!snap_) {   // one reused state: per member in the batch loop, for all of them in turn otherwise
      void* slot = nullptr;
      QD_TRY(workspace(WS_SPO, (size_t)(p.special ? B : 1) * grid_elems * sizeof(c128), &slot, st));
      snap.slot = (c128*)slot;
    }
    snap.bstride = snap_ ? (size_t)nsave * grid_elems : grid_elems;
    QD_TRY(obs->prepare(st));
    snap.obs = obs;
  }
  if (!p.special) {
    // other shapes: one member at a time on the single-wavefunction path
    SpoObserver one;
    if (snap.obs) {
      one = *obs;
      one.B = 1;
    }
    for (int w = 0; w < B; ++w) {
      SnapSink k = plain_sink(snap_ ? snap_ + (size_t)w * nsave * grid_elems : nullptr, grid_elems);
      if (snap.obs) {
        one.rdm = obs->rdm + (size_t)w * obs->rdm_bstride;
        one.mom = obs->mom ? obs->mom + (size_t)w * obs->mom_bstride : nullptr;
        k.slot = snap.slot;   // member w's snapshots are observed before member w + 1 starts
        k.obs = &one;
      }
      QD_TRY(spo2_run_sink(psi_ + w * grid_elems, expVh_, nullptr, expK_, expKy_, nx, ny, ns, nsteps, nout, k, stream));
    }
    return QD_OK;
  }
  if (nsteps == 0) return QD_OK;
  c128* psi = (c128*)psi_;
  const int dims[2] = {nx, ny};
  Pow2Tables t;
  QD_TRY(pow2_prologue((const c128*)expK_, dims, 2, st, &t));
  const size_t sstride = snap.slot ? grid_elems : (size_t)nsave * grid_elems;
  note_path("spo2_batch256");
  note_pass("spo2", p.row[0]);
  note_pass("spo2", p.col);
  // the Strang step sequence of qd_spo2_run_ex (both V/2 halves, wpd.py:723-730)
  auto row = [&](int flags, c128* sp, const c128* U) {
    return launch_row(p.row[0], psi, U, t.tw[1], ns, flags, sp, nullptr, st, B, grid_elems, sstride);
  };
  auto col = [&]() { return launch_col(p.col, psi, t.expKT, t.tw[0], ny, ns, st, grid_elems); };
  return strang_loop(nsteps, nout, snap, st, (const c128*)expVh_, nullptr, 0, row, col, no_pass);
}

extern "C" int qd_spo2_run_batch(qd_c128* psi_, int B, const qd_c128* expVh_, const qd_c128* expK_, int nx, int ny,
                                 int ns, int nsteps, int nout, qd_c128* snap_, void* stream) {
  return spo2_batch_sink(psi_, B, expVh_, expK_, nullptr, nx, ny, ns, nsteps, nout, snap_, nullptr, stream);
}

extern "C" int qd_spo2_run_observed(qd_c128* psi, int B, const qd_c128* expVh, const qd_c128* expK,
                                    const qd_c128* expKy, int nx, int ny, int ns, int nsteps, int nout, qd_c128* snap,
                                    const qd_c128* basis, const double* x, const double* y, double weight,
                                    qd_c128* rdm, double* mom, void* stream) {
  QD_CHECK_ARG(psi && expVh && expK, "qd_spo2_run_observed: null pointer");
  QD_CHECK_ARG(nx >= 1 && ny >= 1, "qd_spo2_run_observed: nx=%d ny=%d", nx, ny);
  const int dims[2] = {nx, ny};
  const double* const ax[3] = {x, y, nullptr};
  QD_TRY(spo_observer_check("qd_spo2_run_observed", dims, 2, ns, B, ax, rdm, mom));
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "qd_spo2_run_observed: nsteps=%d nout=%d", nsteps, nout);
  SpoObserver o = make_observer(dims, 2, ax, ns, B, basis, weight, rdm, mom, (size_t)(nsteps / nout));
  return spo2_batch_sink(psi, B, expVh, expK, expKy, nx, ny, ns, nsteps, nout, snap, &o, stream);
}

extern "C" int qd_spo1d_run(qd_c128* psi_, const qd_c128* expV_, const qd_c128* expVh_, const qd_c128* expK_, int nx,
                            int B, int nt, int nout, qd_c128* snap_, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi_ && expV_ && expVh_ && expK_, "qd_spo1d_run: null pointer");
  QD_CHECK_ARG(nx >= 1 && B >= 1 && nt >= 0 && nout >= 1, "qd_spo1d_run: nx=%d B=%d nt=%d nout=%d", nx, B, nt, nout);
  Pass p;
  const bool special = spo1d_plan(nx, B, &p);
  note_path(special ? "spo1d_pow2" : "spo_any");
  if (!special)
    return spo1d_generic_run((c128*)psi_, (const c128*)expV_, (const c128*)expVh_, (const c128*)expK_, nx, B, nt, nout,
                             (c128*)snap_, st);
  void* w = nullptr;
  QD_TRY(workspace(WS_MISC, nx * sizeof(c128), &w, st));
  QD_TRY(twiddles(nx, st, (c128*)w));
  return launched(dispatch_pass(p, [&](auto K, auto L, auto, auto) {
    if constexpr (decltype(K)::value == SPO_1D)
      hipLaunchKernelGGL(spo1d_kernel<decltype(L)::value>, dim3(p.gx), dim3(p.block), 0, st, (c128*)psi_,
                         (const c128*)expV_, (const c128*)expVh_, (const c128*)expK_, (const c128*)w, nt, nout,
                         (c128*)snap_);
    return decltype(K)::value == SPO_1D;
  }), p);
}

static int spo3_run_sink(qd_c128* psi_, const qd_c128* expVh_, const qd_c128* expK_, int nx, int ny, int nz, int ns,
                         int nsteps, int nout, const SnapSink& snap, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi_ && expVh_ && expK_, "qd_spo3_run: null pointer");
  QD_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && ns >= 1, "qd_spo3_run: nx=%d ny=%d nz=%d ns=%d", nx, ny, nz, ns);
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "qd_spo3_run: nsteps=%d nout=%d", nsteps, nout);
  if (nsteps == 0) return QD_OK;
  c128* psi = (c128*)psi_;
  const int dims[3] = {nx, ny, nz};
  const SpoPlan p = spo3_plan(nx, ny, nz, ns);
  note_path(p.special ? "spo3_pow2" : "spo_any");
  if (!p.special)
    return spo_generic_run(psi, (const c128*)expVh_, nullptr, (const c128*)expK_, nullptr, dims, 3, ns, nsteps, nout,
                           snap, st);
  for (const Pass* q : {&p.row[0], &p.mid, &p.col}) note_pass("spo3", *q);
  Pow2Tables t;
  QD_TRY(pow2_prologue((const c128*)expK_, dims, 3, st, &t));
  const int inner = nz * ns;
  auto row = [&](int flags, c128* sp, const c128* U) {
    return launch_row(p.row[0], psi, U, t.tw[2], ns, flags, sp, nullptr, st);
  };
  auto kin = [&]() -> int {
    QD_TRY(launch_col(p.col, psi, t.expKT, t.tw[0], ny * nz, ns, st));
    return launch_mid(p.mid, psi, t.tw[1], inner, true, st);
  };
  auto fwd = [&]() { return launch_mid(p.mid, psi, t.tw[1], inner, false, st); };
  return strang_loop(nsteps, nout, snap, st, (const c128*)expVh_, nullptr, 0, row, kin, fwd);
}

extern "C" int qd_spo3_run(qd_c128* psi_, const qd_c128* expVh_, const qd_c128* expK_, int nx, int ny, int nz, int ns,
                           int nsteps, int nout, qd_c128* snap_, void* stream) {
  return spo3_run_sink(psi_, expVh_, expK_, nx, ny, nz, ns, nsteps, nout,
                       plain_sink(snap_, (size_t)nx * ny * nz * ns), stream);
}

extern "C" int qd_spo3_run_observed(qd_c128* psi, const qd_c128* expVh, const qd_c128* expK, const qd_c128* mx,
                                    const qd_c128* my, const qd_c128* mz, int nx, int ny, int nz, int ns, int nsteps,
                                    int nout, qd_c128* snap, const qd_c128* basis, const double* x, const double* y,
                                    const double* z, double weight, qd_c128* rdm, double* mom, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip): the observer's partial rows and the snapshot slot
  QD_CHECK_ARG(psi && expVh, "qd_spo3_run_observed: null pointer");
  const bool axes = mx && my && mz;
  QD_CHECK_ARG((expK != nullptr) != (mx || my || mz) && (expK || axes),
               "qd_spo3_run_observed: exactly one of expK and (mx, my, mz) selects the kinetic step");
  QD_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1, "qd_spo3_run_observed: nx=%d ny=%d nz=%d", nx, ny, nz);
  const int dims[3] = {nx, ny, nz};
  const double* const ax[3] = {x, y, z};
  QD_TRY(spo_observer_check("qd_spo3_run_observed", dims, 3, ns, 1, ax, rdm, mom));
  QD_CHECK_ARG(nsteps >= 0 && nout >= 1, "qd_spo3_run_observed: nsteps=%d nout=%d", nsteps, nout);
  const size_t grid_elems = (size_t)nx * ny * nz * ns;
  SpoObserver o = make_observer(dims, 3, ax, ns, 1, basis, weight, rdm, mom, 0);
  SnapSink k = plain_sink(snap, grid_elems);
  if (nsteps / nout) {
    if (!snap) {
      void* slot = nullptr;
      QD_TRY(workspace(WS_SPO, grid_elems * sizeof(c128), &slot, st));
      k.slot = (c128*)slot;
    }
    QD_TRY(o.prepare(st));
    k.obs = &o;
  }
  if (axes)
    return spo3_axes_sink((c128*)psi, (const c128*)expVh, (const c128*)mx, (const c128*)my, (const c128*)mz, nx, ny,
                          nz, ns, nsteps, nout, k, st);
  return spo3_run_sink(psi, expVh, expK, nx, ny, nz, ns, nsteps, nout, k, stream);
}

extern "C" int qd_spo_expv(const void* v, int v_complex, long npts, int ns, double dt, qd_c128* expV_,
                           qd_c128* expVh_, void* stream) {
  QD_CHECK_ARG(v && expVh_, "qd_spo_expv: null pointer");
  QD_CHECK_ARG(ns >= 1 && ns <= 1024, "qd_spo_expv: ns=%d outside [1, 1024]", ns);
  QD_CHECK_ARG(npts >= 0, "qd_spo_expv: npts=%ld", npts);
  if (npts == 0) return QD_OK;
  if (ns > 2)   // scaling-and-squaring Taylor exponential of the Hermitian matrix eigh reads (spo_expm.hip)
    return spo_expm_run(v, v_complex, 1, npts, ns, dt, (c128*)expV_, (c128*)expVh_, (hipStream_t)stream);
  const int grid = (int)std::min<long>((npts + 255) / 256, 8192);
  if (v_complex)
    hipLaunchKernelGGL(spo_expv_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, v, npts, ns, dt,
                       (c128*)expV_, (c128*)expVh_);
  else
    hipLaunchKernelGGL(spo_expv_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, v, npts, ns, dt,
                       (c128*)expV_, (c128*)expVh_);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

extern "C" int qd_spo_expm(const qd_c128* v, int hermitian, long npts, int ns, double dt, qd_c128* expV_,
                           qd_c128* expVh_, void* stream) {
  QD_CHECK_ARG(v && expVh_, "qd_spo_expm: null pointer");
  QD_CHECK_ARG(ns >= 1 && ns <= 1024, "qd_spo_expm: ns=%d outside [1, 1024]", ns);
  QD_CHECK_ARG(npts >= 0, "qd_spo_expm: npts=%ld", npts);
  if (npts == 0) return QD_OK;
  return spo_expm_run(v, 1, hermitian ? 1 : 0, npts, ns, dt, (c128*)expV_, (c128*)expVh_, (hipStream_t)stream);
}
