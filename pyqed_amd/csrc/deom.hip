// deom.hip — DEOM / HEOM auxiliary-density-operator (ADO) hierarchy, RK4.
//
// Replaces DEOMSolver.run's loop (pyqed/heom/deom.py:1107-1113) over rk4
// (deom.py:725-766) whose RHS is rem_cal / generate_dot_element
// (deom.py:641-673) with the time-dependent H(t), Q(t) of generate_time
// (deom.py:676-688).  Per ADO n with index vector key_n:
//   d rho_n = damp_n rho_n - i[H(t), rho_n]
//           + sum_{k: n_k>0} ( cL_nk Q_m rho_{n-e_k} + cR_nk rho_{n-e_k} Q_m )
//           + sum_{k: tier<L} cP_nk [Q_m, rho_{n+e_k}]
// with damp_n = -sum_k n_k expn_k, cL = -i sqrt(n_k)/sqrt(etaa_k) etal_k,
// cR = +i sqrt(n_k)/sqrt(etaa_k) etar_k, cP = -i sqrt(n_k+1) sqrt(etaa_k),
// m = mode[k].  The host builds the bit-exact neighbour tables minus/plus
// (hash of key -/+ e_k, -1 when absent) and the coefficient tables once.
//
// One launch per RK4 stage (the stage needs every ADO of the previous stage); H(t)/Q(t) are assembled in LDS
// per workgroup from H + f_sys(t) Hdip, Q + f_coup(t) Qdip.  The fused
// epilogue does the RK4 bookkeeping (deom_rk4_next: the classic acc form for
// driven runs, the accumulator-free Horner form when the generator is constant
// over the step) and records rho_0 (the system density matrix) after every step.
//
// This file is the host side and one translation unit; its device code sits in the headers it includes:
//   deom_plan.hpp         which kernel runs a stage (deom_stage_plan) or the banded launch (deom_band_plan), with its
//                         template values, launch geometry, DeomParams layout values and noted name (plain C++,
//                         enumerated by tests/test_deom_plan_host.py), and the typed dispatch
//   deom_kernels.hpp      DeomParams, deom_rk4_next; the element, lane-group, pipelined and 16 x 16 MFMA stage kernels;
//                         snapshot, trace, Euler chain and row-gather kernels
//   deom_tile_kernels.hpp the any-ns / any-mode tile kernels (VALU and MFMA)
//   deom_band_kernel.hpp  the persistent banded kernel, its per-call preparation and its stream-ordered fallback
#include "deom_band_kernel.hpp"
#include "deom_tile_kernels.hpp"

#include <cstdlib>
#include <vector>

using namespace qd;

namespace {

// The table and operator part of DeomParams: what the hierarchy and its generator fix.  The state pointers, stage,
// step, nsteps, pulse values, layout and RK4 form are the caller's.
DeomParams deom_params(int B, int nmax, int K, int ns, int nmod, const int32_t* minus, const int32_t* plus,
                       const qd_c128* coef, const qd_c128* damp, const int32_t* mode, const qd_c128* H,
                       const qd_c128* Hdip, const qd_c128* Q, const qd_c128* Qdip, double dt) {
  DeomParams p{};
  p.minus = minus;
  p.plus = plus;
  p.coef = (const c128*)coef;
  p.damp = (const c128*)damp;
  p.mode = mode;
  p.H = (const c128*)H;
  p.Hdip = (const c128*)Hdip;
  p.Q = (const c128*)Q;
  p.Qdip = (const c128*)Qdip;
  p.B = B;
  p.nmax = nmax;
  p.K = K;
  p.ns = ns;
  p.nmod = nmod;
  p.dt = dt;
  return p;
}

// The plan of p's shape (deom_plan.hpp), its layout values written into p; a shape no kernel takes is the caller's
// argument error.
int deom_plan_stage(DeomParams& p, StagePlan& pl) {
  pl = deom_stage_plan(p.B, p.nmax, p.K, p.ns, p.nmod, p.bminor, p.horner);
  QD_CHECK_ARG(pl.refusal == STAGE_OK, "%s", pl.msg);
  p.xsplit = pl.xsplit;
  p.ntst = pl.ntst;
  p.bchunk = pl.bchunk;
  return QD_OK;
}

// Workgroups of the pipelined kernel `fn` per block class: what one XCD's CUs hold at once (every wave persistent, no
// tail generation).
int pipe_blocks_per_class(const void* fn, size_t lds) {
  static thread_local const void* last_fn = nullptr;   // one lookup per kernel / LDS size / device
  static thread_local size_t last_lds = 0;
  static thread_local int last_dev = -1, last_bpc = 1;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (fn != last_fn || lds != last_lds || dev != last_dev) {
    int per_cu = 0, cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, DEOM_TPB, lds);
    last_fn = fn;
    last_lds = lds;
    last_dev = dev;
    last_bpc = std::max(1, per_cu) * std::max(1, cus / 8);
  }
  return last_bpc;
}

// Launch one RK4 stage of the hierarchy described by p on the kernel of its plan pl (deom_plan_stage).
int deom_launch_stage(const StagePlan& pl, const DeomParams& p, hipStream_t st) {
  if (p.step == 0 && p.stage == 0) note_path(pl.name);   // dispatch notes once per run (qd_take_path)
  const bool hit = dispatch_stage(pl, [&](auto k) {
    using T = decltype(k);
    auto go = [&](auto kern, long grid) {
      hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(pl.tpb), pl.lds, st, p);
      return true;
    };
    if constexpr (T::kind == ST_ELEMENT) return go(deom_stage_kernel, pl.grid);
    else if constexpr (T::kind == ST_TILE) return go(deom_stage_tile_kernel, pl.grid);
    else if constexpr (T::kind == ST_TMFMA) return go(deom_stage_tmfma_kernel, pl.grid);
    else if constexpr (T::kind == ST_MFMA16) return go(deom_stage_mfma16_kernel<T::NM>, pl.grid);
    else if constexpr (T::kind == ST_PIPE)
      return go(deom_stage_pipe_kernel<T::KMAX>,
                pl.grid * pipe_blocks_per_class((const void*)deom_stage_pipe_kernel<T::KMAX>, pl.lds));
    else if constexpr (T::kind == ST_GROUP_W5)
      return go(deom_stage_grp_w5_kernel<T::G, T::KMAX, T::NS2, T::UNI, T::HM>, pl.grid);
    else return go(deom_stage_grp_kernel<T::G, T::KMAX, T::NS2, T::UNI, T::HM>, pl.grid);
  });
  QD_CHECK_ARG(hit, "deom: internal: no kernel for stage kind %d G=%d KMAX=%d UNI=%d HM=%d NM=%d", pl.kind, pl.G,
               pl.KMAX, pl.UNI, pl.HM, pl.NM);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// obs[b][s][m] = Tr(E_m rho_0(s)) over the B x nsnap snapshots of snap (deom_trace_kernel)
int launch_trace(const c128* snap, const qd_c128* E, int ne, int B, int ns, int nsnap, qd_c128* obs, hipStream_t st) {
  const int n = B * nsnap * ne;
  hipLaunchKernelGGL(deom_trace_kernel, dim3(std::max(1, std::min(1024, (n + 255) / 256))), dim3(256), 0, st, snap,
                     (const c128*)E, ne, B, ns, nsnap, (c128*)obs);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

int deom_run(qd_c128* ados, int B, int nmax, int K, int ns, const int32_t* minus, const int32_t* plus,
             const qd_c128* coef, const qd_c128* damp, const int32_t* mode, int nmod, const qd_c128* H,
             const qd_c128* Hdip, const qd_c128* Q, const qd_c128* Qdip, const qd_c128* fsys, const qd_c128* fcoup,
             double dt, int nsteps, qd_c128* rho_sys, const qd_c128* E, int ne, qd_c128* trace, void* stream,
             int bminor) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(ados && minus && plus && coef && damp && mode && H && Q, "qd_deom_rk4: null pointer");
  QD_CHECK_ARG(B >= 1 && nmax >= 1 && K >= 1 && nsteps >= 0, "qd_deom_rk4: bad sizes B=%d nmax=%d K=%d", B, nmax, K);
  QD_CHECK_ARG(ns >= 1 && nmod >= 1, "qd_deom_rk4: ns=%d nmod=%d", ns, nmod);
  QD_CHECK_ARG(!Hdip || fsys, "qd_deom_rk4: Hdip given without fsys");
  QD_CHECK_ARG(!Qdip || fcoup, "qd_deom_rk4: Qdip given without fcoup");
  QD_CHECK_ARG(!trace || (E && ne >= 1), "qd_deom_rk4: trace requested without observables");
  hipStream_t st = (hipStream_t)stream;
  const size_t ns2 = (size_t)ns * ns;
  const size_t tot = (size_t)B * nmax * ns2;
  const bool need_snap = rho_sys || trace;
  const size_t snap_elems = need_snap && !rho_sys ? (size_t)B * (nsteps + 1) * ns2 : 0;
  void* w = nullptr;
  int rc = workspace(WS_DEOM, (3 * tot + snap_elems) * sizeof(c128), &w, st);
  if (rc) return rc;
  c128* acc = (c128*)w;
  c128* xs[2] = {acc + tot, acc + 2 * tot};
  c128* snap = rho_sys ? (c128*)rho_sys : (need_snap ? acc + 3 * tot : nullptr);
  // fsys/fcoup are host arrays [nsteps][3] (values at t, t+dt/2, t+dt): kernel args per stage
  const qd_c128* fs_h = fsys;
  const qd_c128* fc_h = fcoup;
  if (snap) {
    hipLaunchKernelGGL(deom_snap0_kernel, dim3(std::max(1, std::min(1024, (int)((B * ns2 + 255) / 256)))), dim3(256),
                       0, st, (const c128*)ados, snap, B, nmax, ns, nsteps, bminor);
    QD_HIP(hipGetLastError());
  }
  DeomParams p = deom_params(B, nmax, K, ns, nmod, minus, plus, coef, damp, mode, H, Hdip, Q, Qdip, dt);
  p.rho = (const c128*)ados;
  p.rho_out = (c128*)ados;
  p.acc = acc;
  p.snap = snap;
  p.nsteps = nsteps;
  p.bminor = bminor;
  // Horner-form RK4 unless the run is driven
  p.horner = !Hdip && !Qdip;
  // the shape is the run's: one plan for its 4 nsteps stage launches
  StagePlan pl;
  QD_TRY(deom_plan_stage(p, pl));
  static const int stage_time[4] = {0, 1, 1, 2};
  for (int s = 0; s < nsteps; ++s) {
    p.step = s;
    for (int stage = 0; stage < 4; ++stage) {
      p.stage = stage;
      p.xin = stage == 0 ? (const c128*)ados : xs[(stage - 1) & 1];
      p.xout = xs[stage & 1];
      const int ti = s * 3 + stage_time[stage];
      p.fs = fs_h ? cmk(fs_h[ti].re, fs_h[ti].im) : cmk(0, 0);
      p.fc = fc_h ? cmk(fc_h[ti].re, fc_h[ti].im) : cmk(0, 0);
      QD_TRY(deom_launch_stage(pl, p, st));
    }
  }
  if (trace) QD_TRY(launch_trace(snap, E, ne, B, ns, nsteps + 1, trace, st));
  return QD_OK;
}

}  // namespace

extern "C" int qd_deom_rk4(qd_c128* ados, int B, int nmax, int K, int ns, const int32_t* minus, const int32_t* plus,
                           const qd_c128* coef, const qd_c128* damp, const int32_t* mode, int nmod, const qd_c128* H,
                           const qd_c128* Hdip, const qd_c128* Q, const qd_c128* Qdip, const qd_c128* fsys,
                           const qd_c128* fcoup, double dt, int nsteps, qd_c128* rho_sys, const qd_c128* E, int ne,
                           qd_c128* trace, void* stream) {
  return deom_run(ados, B, nmax, K, ns, minus, plus, coef, damp, mode, nmod, H, Hdip, Q, Qdip, fsys, fcoup, dt, nsteps,
                  rho_sys, E, ne, trace, stream, 0);
}

extern "C" int qd_deom_rk4_ado_major(qd_c128* ados, int B, int nmax, int K, int ns, const int32_t* minus,
                                     const int32_t* plus, const qd_c128* coef, const qd_c128* damp,
                                     const int32_t* mode, int nmod, const qd_c128* H, const qd_c128* Hdip,
                                     const qd_c128* Q, const qd_c128* Qdip, const qd_c128* fsys,
                                     const qd_c128* fcoup, double dt, int nsteps, qd_c128* rho_sys, const qd_c128* E,
                                     int ne, qd_c128* trace, void* stream) {
  return deom_run(ados, B, nmax, K, ns, minus, plus, coef, damp, mode, nmod, H, Hdip, Q, Qdip, fsys, fcoup, dt, nsteps,
                  rho_sys, E, ne, trace, stream, 1);
}

// One RK4 stage over a band of ADOs (tier-banded sharding of one hierarchy): rows [0, n_own) of
// rho / xin / xout are this band's ADOs, rows [n_own, n_loc) of xin the halo copies of the neighbours other bands
// own; minus / plus [n_own][K] hold LOCAL row indices (-1 = absent).  Stage s reads xin (s = 0: rho), writes the
// owned rows of xout (s < 3) and acc, and at s = 3 the owned rows of rho; snap (band owning ADO 0 only) receives
// rho_0 after the step.  Same kernels and arithmetic as qd_deom_rk4: acc = null selects the Horner-form stages
// (what qd_deom_rk4 runs without a pulse; then stage s writes rho + dt / (4 - s) L x), a non-null acc the classic
// RK4 bookkeeping (required for driven stages).
extern "C" int qd_deom_stage(qd_c128* rho, const qd_c128* xin, qd_c128* xout, qd_c128* acc, int n_own, int K, int ns,
                             const int32_t* minus, const int32_t* plus, const qd_c128* coef, const qd_c128* damp,
                             const int32_t* mode, int nmod, const qd_c128* H, const qd_c128* Hdip, const qd_c128* Q,
                             const qd_c128* Qdip, double fs_re, double fs_im, double fc_re, double fc_im, int stage,
                             double dt, qd_c128* snap, int step, int nsteps, void* stream) {
  QD_CHECK_ARG(rho && xin && minus && plus && coef && damp && mode && H && Q, "qd_deom_stage: null pointer");
  QD_CHECK_ARG(acc || (!Hdip && !Qdip), "qd_deom_stage: a driven stage needs the RK4 accumulator acc");
  QD_CHECK_ARG(stage >= 0 && stage <= 3 && (stage == 3 || xout), "qd_deom_stage: bad stage %d / null xout", stage);
  QD_CHECK_ARG(n_own >= 1 && K >= 1, "qd_deom_stage: bad sizes n_own=%d K=%d", n_own, K);
  QD_CHECK_ARG(ns >= 1 && nmod >= 1, "qd_deom_stage: ns=%d nmod=%d", ns, nmod);
  QD_CHECK_ARG(!snap || (step >= 0 && step < nsteps), "qd_deom_stage: snapshot step %d outside [0, %d)", step, nsteps);
  DeomParams p = deom_params(1, n_own, K, ns, nmod, minus, plus, coef, damp, mode, H, Hdip, Q, Qdip, dt);
  p.rho = (const c128*)rho;
  p.rho_out = (c128*)rho;
  p.xin = (const c128*)xin;
  p.xout = (c128*)xout;
  p.acc = (c128*)acc;
  p.fs = cmk(fs_re, fs_im);
  p.fc = cmk(fc_re, fc_im);
  p.snap = (c128*)snap;
  p.stage = stage;
  p.step = step;
  p.nsteps = nsteps;
  p.bminor = 0;
  p.horner = acc == nullptr;   // no accumulator: Horner-form stages (constant generator over the step)
  StagePlan pl;
  QD_TRY(deom_plan_stage(p, pl));
  return deom_launch_stage(pl, p, (hipStream_t)stream);
}

// y = alpha P x for B ADO vectors (the generator of generate_dot_element, heom/deom.py:641-664, as an operator; the
// Krylov form of DEOMSolver.correlation_4op_3t applies it and its transpose, pyqed_amd/deom_krylov.py).  One stage
// launch of the stage kernels: Horner stage 2 (s_3 = rho + dt / 2 L s_2) with rho = 0 (a null rho: nothing is read
// for it) and dt = 2 alpha, so the coefficient is alpha exactly and the kernel reads its input only from xin.
extern "C" int qd_deom_apply(const qd_c128* x, qd_c128* y, const qd_c128* x0, int B, int nmax, int K, int ns,
                             const int32_t* minus,
                             const int32_t* plus, const qd_c128* coef, const qd_c128* damp, const int32_t* mode,
                             int nmod, const qd_c128* H, const qd_c128* Q, double alpha, int ado_major, void* stream) {
  QD_CHECK_ARG(x && y && minus && plus && coef && damp && mode && H && Q, "qd_deom_apply: null pointer");
  QD_CHECK_ARG(x != y && x0 != y, "qd_deom_apply: y must alias neither x nor x0");
  QD_CHECK_ARG(B >= 1 && nmax >= 1 && K >= 1 && ns >= 1 && nmod >= 1, "qd_deom_apply: bad sizes B=%d nmax=%d K=%d ns=%d",
               B, nmax, K, ns);
  // the Horner stage-2 form y = rho + (dt / 2) L x with rho = x0 and dt = 2 alpha; rho == nullptr (x0 NULL): the stage
  // kernels take rho = 0 without a zeroed buffer to read; stage 2 never writes rho_out
  DeomParams p = deom_params(B, nmax, K, ns, nmod, minus, plus, coef, damp, mode, H, nullptr, Q, nullptr, 2.0 * alpha);
  p.rho = (const c128*)x0;
  p.xin = (const c128*)x;
  p.xout = (c128*)y;
  p.stage = 2;
  p.step = 1;   // not a run's first stage: no dispatch notes from the launcher
  p.nsteps = 2;
  p.bminor = ado_major ? 1 : 0;
  p.horner = 1;
  note_path("deom_apply");
  StagePlan pl;
  QD_TRY(deom_plan_stage(p, pl));
  return deom_launch_stage(pl, p, (hipStream_t)stream);
}

// dst[i][:] = src[idx[i]][:] for i < n, rows of `row_elems` complex (packs a band's halo rows for the exchange);
// src holds nsrc rows.  check != 0: synchronise and return QD_EINVAL if an index was out of range.
extern "C" int qd_gather_rows(const qd_c128* src, int nsrc, const int32_t* idx, int n, int row_elems, qd_c128* dst,
                              int check, void* stream) {
  QD_CHECK_ARG(n >= 0 && row_elems >= 1 && nsrc >= 0, "qd_gather_rows: bad sizes n=%d row=%d nsrc=%d", n, row_elems,
               nsrc);
  if (n == 0) return QD_OK;
  QD_CHECK_ARG(src && idx && dst, "qd_gather_rows: null pointer");
  WsScope wss_((hipStream_t)stream);
  void* w = nullptr;   // the bad-index flag, only when the caller asks for the check
  if (check) {
    int rc = workspace(WS_MISC, sizeof(int), &w, (hipStream_t)stream);
    if (rc) return rc;
    QD_TRY(fill_bytes(w, 0, sizeof(int), (hipStream_t)stream));
  }
  const size_t tot = (size_t)n * row_elems;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((int)std::min<size_t>((tot + 255) / 256, 8192)), dim3(256), 0,
                     (hipStream_t)stream, (const c128*)src, nsrc, idx, n, row_elems, (c128*)dst, (int*)w);
  QD_HIP(hipGetLastError());
  if (check) {
    int h = 0;
    QD_HIP(hipMemcpyAsync(&h, w, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    QD_HIP(hipStreamSynchronize((hipStream_t)stream));
    QD_CHECK_ARG(h == 0, "qd_gather_rows: a row index outside [0, %d)", nsrc);
  }
  return QD_OK;
}

// obs[s][m] = Tr(E_m rho_0(s)) for s < nsnap (DEOMSolver.run's Tr(p1 rho_0), heom/deom.py:1100,1113)
extern "C" int qd_deom_trace(const qd_c128* snap, const qd_c128* E, int ne, int nsnap, int ns, qd_c128* obs,
                             void* stream) {
  QD_CHECK_ARG(snap && E && obs && ne >= 1 && nsnap >= 1 && ns >= 1, "qd_deom_trace: bad arguments");
  return launch_trace((const c128*)snap, E, ne, 1, ns, nsnap, obs, (hipStream_t)stream);
}

extern "C" int qd_heom_chain_euler(qd_c128* ados, int B, int nado, int ns, const qd_c128* H, const qd_c128* Q,
                                   double gamma, double D0_re, double D0_im, double dt, int nsteps, qd_c128* rho_sys,
                                   const qd_c128* E, int ne, qd_c128* obs, void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(ados && H && Q, "qd_heom_chain_euler: null pointer");
  QD_CHECK_ARG(B >= 1 && nado >= 2 && nsteps >= 0, "qd_heom_chain_euler: bad sizes B=%d nado=%d", B, nado);
  QD_CHECK_ARG(ns >= 1, "qd_heom_chain_euler: ns=%d", ns);
  QD_CHECK_ARG(!obs || (E && ne >= 1), "qd_heom_chain_euler: obs requested without observables");
  hipStream_t st = (hipStream_t)stream;
  const size_t ns2 = (size_t)ns * ns;
  c128* snap = (c128*)rho_sys;
  const size_t snap_elems = (!snap && obs) ? (size_t)B * (nsteps + 1) * ns2 : 0;
  void* w = nullptr;
  int rc = workspace(WS_DEOM, (snap_elems + (size_t)B * ns2) * sizeof(c128), &w, st);
  if (rc) return rc;
  c128* tmp = (c128*)w;
  if (snap_elems) snap = tmp + (size_t)B * ns2;
  hipLaunchKernelGGL(heom_chain_sweep_kernel, dim3(B), dim3(256), 0, st, (c128*)ados, nado, ns, (const c128*)H,
                     (const c128*)Q, gamma, cmk(D0_re, D0_im), dt, nsteps, snap, tmp);
  QD_HIP(hipGetLastError());
  if (obs) QD_TRY(launch_trace(snap, E, ne, B, ns, nsteps + 1, obs, st));
  return QD_OK;
}

namespace {

// The bands spin on each other's epochs, so all of them must be resident at once.  The launch is cooperative
// (hipLaunchCooperativeKernel checks the grid against the occupancy of the kernel and refuses an oversize one with
// hipErrorCooperativeLaunchTooLarge instead of stranding bands; +15-19 us once per run, MI355X_MICROARCH.md row
// coop-launch).  Work queued on other streams can still delay a band's start; the bounded spin then sets *status and
// the caller re-runs on the stage launches (DEOMSolver.run).  QD_OPT_COOP_LAUNCH = 0: plain launch (profiling).
template <typename Kern>
hipError_t band_launch_one(Kern kern, BandParams p, int nbands, int tpb, size_t lds, hipStream_t st) {
  if (!option(QD_OPT_COOP_LAUNCH)) {
    hipLaunchKernelGGL(kern, dim3(nbands), dim3(tpb), lds, st, p);
    return hipGetLastError();
  }
  void* args[] = {(void*)&p};
  return hipLaunchCooperativeKernel((const void*)kern, dim3(nbands), dim3(tpb), args, (unsigned)lds, st);
}

}  // namespace

// One hierarchy (B = 1) as one persistent launch over `nbands` tier bands (deom_band_kernel.hpp).  The band
// tables come from deom_shard.make_plans: band_lo [nbands + 1], halo_off / halo_idx (global halo rows per band),
// src_off / src (bands owning them), lminus / lplus [nmax][K] local rows; max_own / max_loc the largest band's
// owned / owned + halo row counts.  ns^2 <= 16 (ns <= 4), K <= 8, max_own ns'^2 <= 1024 lanes (ns' = 2 or 4),
// every band's rows in LDS (deom_band_plan).  status (device int, or null): 1 after the run if a hand-off timed out
// (the caller re-runs); with null the call stays asynchronous and queues a stream-ordered fallback that re-runs the
// propagation on one workgroup when (and only when) a hand-off timed out (deom_banded_fallback_kernel).
extern "C" int qd_deom_rk4_banded(qd_c128* ados, int nmax, int K, int ns, const int32_t* lminus, const int32_t* lplus,
                                  const int32_t* band_lo, const int32_t* halo_off, const int32_t* halo_idx,
                                  const int32_t* src_off, const int32_t* src, int nbands, int max_own, int max_loc,
                                  const qd_c128* coef, const qd_c128* damp, const int32_t* mode, int nmod,
                                  const qd_c128* H, const qd_c128* Hdip, const qd_c128* Q, const qd_c128* Qdip,
                                  const qd_c128* fsys, const qd_c128* fcoup, double dt, int nsteps, qd_c128* rho_sys,
                                  const qd_c128* E, int ne, qd_c128* trace, int32_t* status, void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(ados && lminus && lplus && band_lo && halo_off && src_off && coef && damp && mode && H && Q,
               "qd_deom_rk4_banded: null pointer");
  QD_CHECK_ARG(nmax >= 1 && K >= 1 && K <= 8 && nsteps >= 0 && nmod >= 1,
               "qd_deom_rk4_banded: bad sizes nmax=%d K=%d nmod=%d (K <= 8)", nmax, K, nmod);
  QD_CHECK_ARG(nbands >= 1 && max_own >= 1 && max_loc >= max_own,
               "qd_deom_rk4_banded: bad band sizes nbands=%d max_own=%d max_loc=%d", nbands, max_own, max_loc);
  {  // the bands wait on each other: every band's workgroup must be resident at once (one per CU suffices)
    int dev = 0, cus = 0;
    QD_HIP(hipGetDevice(&dev));
    QD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    QD_CHECK_ARG(nbands <= cus, "qd_deom_rk4_banded: %d bands exceed the %d CUs (bands must be co-resident)", nbands,
                 cus);
  }
  QD_CHECK_ARG(!Hdip || fsys, "qd_deom_rk4_banded: Hdip given without fsys");
  QD_CHECK_ARG(!Qdip || fcoup, "qd_deom_rk4_banded: Qdip given without fcoup");
  QD_CHECK_ARG(!trace || (E && ne >= 1), "qd_deom_rk4_banded: trace requested without observables");
  const BandPlan bp = deom_band_plan(ns, K, nmod, max_own, max_loc);
  QD_CHECK_ARG(bp.refusal == BAND_OK, "%s", bp.msg);
  const int tpb = bp.tpb;
  const size_t lds = bp.lds;
  const size_t ns2 = (size_t)ns * ns;
  hipStream_t st = (hipStream_t)stream;
  const size_t tot = (size_t)nmax * ns2;
  QD_CHECK_ARG(tot * sizeof(c128) < ((size_t)1 << 31), "qd_deom_rk4_banded: %zu ADO elements exceed 32-bit offsets",
               tot);
  const bool need_snap = rho_sys || trace;
  const size_t snap_elems = need_snap && !rho_sys ? (size_t)(nsteps + 1) * ns2 : 0;
  const size_t nf = fsys ? (size_t)nsteps * 3 : 0, nc = fcoup ? (size_t)nsteps * 3 : 0;
  const size_t flag_bytes = 16;   // the status word, 16-B padded
  // without a caller status word the call stays asynchronous: the initial ADOs are saved (and, for driven runs, an
  // accumulator kept) for a stream-ordered fallback launch that re-runs the propagation only if a hand-off timed out
  const bool guard = !status && nsteps > 0;
  const size_t gtab_elems = ((size_t)2 * nmax * K * sizeof(int32_t) + sizeof(c128) - 1) / sizeof(c128);
  const size_t fb_elems = guard ? (Hdip || Qdip ? 2 : 1) * tot + gtab_elems : 0;
  void* w = nullptr;
  int rc = workspace(WS_DEOM, (2 * tot + snap_elems + nf + nc + fb_elems) * sizeof(c128) + flag_bytes, &w, st);
  if (rc) return rc;
  c128* buf = (c128*)w;
  c128* snap = rho_sys ? (c128*)rho_sys : (need_snap ? buf + 2 * tot : nullptr);
  c128* fsv = nf ? buf + 2 * tot + snap_elems : nullptr;
  c128* fcv = nc ? buf + 2 * tot + snap_elems + nf : nullptr;
  c128* saved = guard ? buf + 2 * tot + snap_elems + nf + nc : nullptr;
  c128* fb_acc = guard && (Hdip || Qdip) ? saved + tot : nullptr;
  int* gtab = guard ? (int*)(saved + (Hdip || Qdip ? 2 : 1) * tot) : nullptr;
  int* stat_ws = (int*)(buf + 2 * tot + snap_elems + nf + nc + fb_elems);
  int* stat = status ? (int*)status : stat_ws;
  if (fsv) QD_TRY(upload(fsv, fsys, nf * sizeof(c128), st));
  if (fcv) QD_TRY(upload(fcv, fcoup, nc * sizeof(c128), st));
  // both hand-off buffers preset to parity 1 in every double (stages 0 and 1, their first writers, carry parity 0),
  // the status words zeroed, snapshot row 0 written: one kernel
  {
    const long nwords = (long)(2 * tot * sizeof(c128) / 8);
    hipLaunchKernelGGL(deom_band_prep_kernel, dim3((int)std::min<long>((nwords + 255) / 256, 1024)), dim3(256), 0, st,
                       (unsigned long long*)buf, nwords, stat_ws, status ? (int*)status : nullptr,
                       (const c128*)ados, snap, (int)ns2, saved, (long)tot);
    QD_HIP(hipGetLastError());
  }
  if (nsteps > 0) {
    BandParams p;
    p.ados = (const c128*)ados;
    p.buf = buf;
    p.status = stat;
    p.band_lo = band_lo;
    p.halo_off = halo_off;
    p.halo_idx = halo_idx;
    p.src_off = src_off;
    p.src = src;
    p.lminus = lminus;
    p.lplus = lplus;
    p.coef = (const c128*)coef;
    p.damp = (const c128*)damp;
    p.mode = mode;
    p.H = (const c128*)H;
    p.Hdip = (const c128*)Hdip;
    p.Q = (const c128*)Q;
    p.Qdip = (const c128*)Qdip;
    p.fsv = fsv;
    p.fcv = fcv;
    p.snap = snap;
    p.tim = nullptr;
#ifdef QD_PHASE_TIMING
    void* tw = nullptr;
    if (int rc2 = workspace(WS_MISC, (size_t)nbands * 4 * sizeof(unsigned long long), &tw, st)) return rc2;
    p.tim = (unsigned long long*)tw;
#endif
    p.nmax = nmax;
    p.K = K;
    p.ns = ns;
    p.nmod = nmod;
    p.nsteps = nsteps;
    p.max_loc = max_loc;
    p.dt = dt;
    note_path(bp.name);
    hipError_t le = hipSuccess;
    const bool hit = dispatch_band(bp, [&](auto k) {
      using T = decltype(k);
      le = band_launch_one(deom_band_kernel<T::G, T::KMAX, T::NS2, T::TPB, T::FAST>, p, nbands, tpb, lds, st);
      return true;
    });
    QD_CHECK_ARG(hit, "qd_deom_rk4_banded: internal: no kernel for G=%d KMAX=%d FAST=%d TPB=%d", bp.G, bp.KMAX, bp.FAST,
                 bp.TPB);
    if (le == hipErrorCooperativeLaunchTooLarge) {
      (void)hipGetLastError();
      set_error("qd_deom_rk4_banded: %d bands of %d threads / %zu B LDS cannot all be co-resident "
                "(hipErrorCooperativeLaunchTooLarge); use fewer bands or the stage launches", nbands, tpb, lds);
      return QD_EBUSY;
    }
    QD_HIP(le);
    if (option(QD_OPT_FAKE_TIMEOUT))   // tests: report a hand-off timeout after the run
      QD_TRY(fill_bytes(stat, 1, 1, st));
#ifdef QD_PHASE_TIMING
    {   // per-phase wall-clock (100 MHz ticks) summed over the stages: mean and max over bands, per stage, in us
      std::vector<unsigned long long> h((size_t)nbands * 4);
      QD_HIP(hipMemcpyAsync(h.data(), p.tim, h.size() * 8, hipMemcpyDeviceToHost, st));
      QD_HIP(hipStreamSynchronize(st));
      const char* nm[4] = {"wait", "halo", "compute", "publish"};
      for (int k = 0; k < 4; ++k) {
        double sm = 0, mx = 0;
        for (int b = 0; b < nbands; ++b) {
          sm += (double)h[(size_t)b * 4 + k];
          mx = std::max(mx, (double)h[(size_t)b * 4 + k]);
        }
        fprintf(stderr, "band phase %-8s mean %.3f us max %.3f us per stage\n", nm[k], sm / nbands / 100.0 / (4.0 * nsteps),
                mx / 100.0 / (4.0 * nsteps));
      }
    }
#endif
    // the last stage 3 wrote the final rho straight into ados (deom_band_kernel)
    if (guard) {   // stream-ordered fallback: a no-op unless the banded launch reported a hand-off timeout
      DeomParams f = deom_params(1, nmax, K, ns, nmod, nullptr, nullptr, coef, damp, mode, H, Hdip, Q, Qdip, dt);
      f.acc = fb_acc;
      f.snap = snap;
      f.nsteps = nsteps;
      f.horner = !Hdip && !Qdip;
      note_path("deom_banded_guarded");
      hipLaunchKernelGGL(deom_banded_fallback_kernel, dim3(1), dim3(1024), 0, st, f, (const int*)stat,
                         (const c128*)saved, (c128*)ados, buf, buf + tot, (const c128*)fsv, (const c128*)fcv,
                         lminus, lplus, band_lo, halo_off, halo_idx, nbands, gtab, gtab + (size_t)nmax * K);
      QD_HIP(hipGetLastError());
    }
  }
  if (trace) QD_TRY(launch_trace(snap, E, ne, 1, ns, nsteps + 1, trace, st));
  return QD_OK;
}
