// lvc.hip — linear vibronic coupling in Fock space, matrix-free: qd_lvc_apply, qd_lvc_rk4, qd_lvc_observe, the
// laser-driven qd_lvc_driven_rk4, and the pair record and its run, qd_lvc_pair_observe and qd_lvc_pair_rk4.
//
// Replaces LVC.buildH + SESolver.run of pyqed/mol.py:959-1262 on a dense or sparse H by the stencil of
// lvc_kernels.hpp.  This file is the host side only: pointer checks, the plan (lvc_plan.hpp decides what is admitted,
// the path, every grid and the scratch layout), scratch from the arena, and the launches.  dims and omega are host
// arrays read at call time into kernel arguments, so the calls are asynchronous and a capture holds their values.
#include "lvc_pair_kernels.hpp"

namespace qd {
namespace {

int lvc_refused(const LvcPlan& p) {
  set_error("%s", p.msg);
  return QD_EINVAL;
}

LvcDev lvc_dev(const LvcPlan& p, const double* omega) {
  LvcDev m = p.dev;
  for (int j = 0; j < m.M; ++j) m.omega[j] = omega[j];
  return m;
}

dim3 grid_of(const LvcLaunch& l) { return dim3(l.gx, l.gy, l.gz); }

// out = base + coef (-iH) v, or out = H v (base null)
int lvc_stage(const LvcPlan& p, const LvcDev& m, const c128* Hel, const c128* W, const c128* v, const c128* base,
              c128* out, double coef, hipStream_t st) {
  const bool hit = dispatch_lvc_nel(m.nel, [&](auto N) {
    hipLaunchKernelGGL((lvc_stage_kernel<decltype(N)::value>), grid_of(p.stage), dim3(p.stage.tpb), p.stage.lds, st, m,
                       Hel, W, v, base, out, coef);
    return true;
  });
  QD_CHECK_ARG(hit, "lvc: no stage kernel for nel=%d", m.nel);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// the record of B states psi (members bstride apart) into obs + b * obs_bstride (complex values)
int lvc_observe(const LvcPlan& p, const LvcDev& m, const c128* psi, size_t bstride, double* part, c128* obs,
                size_t obs_bstride, hipStream_t st) {
  hipLaunchKernelGGL(lvc_obs_part_kernel, grid_of(p.obs_part), dim3(p.obs_part.tpb), 0, st, m, psi, bstride, part);
  QD_HIP(hipGetLastError());
  hipLaunchKernelGGL(lvc_obs_final_kernel, grid_of(p.obs_final), dim3(p.obs_final.tpb), 0, st, m.nel, m.M, p.G,
                     (const double*)part, (double*)obs, 2 * obs_bstride);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

int lvc_run_staged(const LvcPlan& p, const LvcDev& m, const c128* Hel, const c128* W, c128* psi, int B, double dt,
                   int nsteps, int save_every, int nsave, c128* snap, c128* obs, hipStream_t st) {
  void* w = nullptr;
  QD_TRY(workspace(WS_MISC, p.ws_total, &w, st));
  c128* x0 = (c128*)((char*)w + p.ws_x0);
  c128* x1 = (c128*)((char*)w + p.ws_x1);
  double* part = (double*)((char*)w + p.ws_part);
  const size_t rec_b = (size_t)(nsave + 1) * p.nobs;
  if (obs) QD_TRY(lvc_observe(p, m, psi, m.D, part, obs, rec_b, st));
  const double c[4] = {dt * 0.25, dt / 3.0, dt * 0.5, dt};   // rk4_horner_coef
  for (int s = 0; s < nsteps; ++s) {
    QD_TRY(lvc_stage(p, m, Hel, W, psi, psi, x0, c[0], st));
    QD_TRY(lvc_stage(p, m, Hel, W, x0, psi, x1, c[1], st));
    QD_TRY(lvc_stage(p, m, Hel, W, x1, psi, x0, c[2], st));
    QD_TRY(lvc_stage(p, m, Hel, W, x0, psi, psi, c[3], st));
    if (save_every > 0 && (s + 1) % save_every == 0) {
      const int idx = (s + 1) / save_every;
      if (snap) {
        hipLaunchKernelGGL(lvc_snap_kernel, grid_of(p.snap), dim3(p.snap.tpb), 0, st, (const c128*)psi, B, m.D, nsave,
                           idx, snap);
        QD_HIP(hipGetLastError());
      }
      if (obs) QD_TRY(lvc_observe(p, m, psi, m.D, part, obs + (size_t)idx * p.nobs, rec_b, st));
    }
  }
  return QD_OK;
}

template <int NEL>
int lvc_launch_resident(const LvcPlan& p, const LvcDev& m, const c128* Hel, const c128* W, c128* psi, double dt,
                        int nsteps, int save_every, int nsave, c128* snap, c128* obs, hipStream_t st) {
  static const hipError_t attr = hipFuncSetAttribute((const void*)lvc_resident_kernel<NEL>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)LVC_LDS_MAX);
  QD_HIP(attr);
  const LvcLds L{(unsigned)p.lds_vec1, (unsigned)p.lds_tab, (unsigned)p.lds_wave, (unsigned)p.lds_tile,
                 (unsigned)p.lds_nbar};
  hipLaunchKernelGGL((lvc_resident_kernel<NEL>), grid_of(p.resident), dim3(p.resident.tpb), p.resident.lds, st, m, L,
                     Hel, W, psi, dt, nsteps, save_every, nsave, snap, (double*)obs, p.nobs);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// ---------------------------------------------------------------- laser-driven runs
// the tables a driven launch takes besides the model
struct LvcDriveArgs {
  const c128 *Hel, *W, *A, *fvals;
};

const c128* lvc_row(const LvcDrivePlan& p, const LvcDriveArgs& t, int s, int stage) {
  return p.drive.nd ? t.fvals + (size_t)lvc_drive_row(p.sample, p.hold, s, stage) * p.drive.nd : nullptr;
}

int lvc_run_driven_staged(const LvcDrivePlan& dp, const LvcDev& m, const LvcDriveArgs& t, c128* psi, int B, double dt,
                          int nsteps, int save_every, int nsave, c128* snap, c128* obs, hipStream_t st) {
  const LvcPlan& p = dp.base;
  void* w = nullptr;
  QD_TRY(workspace(WS_MISC, dp.ws_total, &w, st));
  c128* x0 = (c128*)((char*)w + p.ws_x0);
  c128* x1 = (c128*)((char*)w + p.ws_x1);
  c128* x2 = (c128*)((char*)w + dp.ws_acc);   // stage mode only
  double* part = (double*)((char*)w + p.ws_part);
  const size_t rec_b = (size_t)(nsave + 1) * p.nobs;
  if (obs) QD_TRY(lvc_observe(p, m, psi, m.D, part, obs, rec_b, st));
  // out = base + c_out (-iH_f v) with the row of (s, stage); acc = acc_in + c_acc (-iH_f v) in stage mode
  auto stage = [&](int s, int stg, const c128* v, c128* out, double c_out, const c128* acc_in, c128* acc,
                   double c_acc) -> int {
    const c128* f = lvc_row(dp, t, s, stg);
    const bool hit = dispatch_lvc_nel(m.nel, [&](auto N) {
      constexpr int NEL = decltype(N)::value;
      if (dp.sample == LVC_STAGE)
        hipLaunchKernelGGL((lvc_stage_rk4_kernel<NEL>), grid_of(p.stage), dim3(p.stage.tpb), p.stage.lds, st, m,
                           dp.drive, t.Hel, t.W, t.A, f, v, (const c128*)psi, acc_in, out, acc, c_out, c_acc);
      else
        hipLaunchKernelGGL((lvc_stage_driven_kernel<NEL>), grid_of(p.stage), dim3(p.stage.tpb), p.stage.lds, st, m,
                           dp.drive, t.Hel, t.W, t.A, f, v, (const c128*)psi, out, c_out);
      return true;
    });
    QD_CHECK_ARG(hit, "qd_lvc_driven_rk4: no stage kernel for nel=%d", m.nel);
    QD_HIP(hipGetLastError());
    return QD_OK;
  };
  const double c[4] = {dt * 0.25, dt / 3.0, dt * 0.5, dt};   // rk4_horner_coef
  for (int s = 0; s < nsteps; ++s) {
    if (dp.sample == LVC_STAGE) {
      QD_TRY(stage(s, 0, psi, x0, dt * 0.5, psi, x2, dt / 6.0));
      QD_TRY(stage(s, 1, x0, x1, dt * 0.5, x2, x2, dt / 3.0));
      QD_TRY(stage(s, 2, x1, x0, dt, x2, x2, dt / 3.0));
      QD_TRY(stage(s, 3, x0, nullptr, 0.0, x2, psi, dt / 6.0));
    } else {
      QD_TRY(stage(s, 0, psi, x0, c[0], nullptr, nullptr, 0.0));
      QD_TRY(stage(s, 1, x0, x1, c[1], nullptr, nullptr, 0.0));
      QD_TRY(stage(s, 2, x1, x0, c[2], nullptr, nullptr, 0.0));
      QD_TRY(stage(s, 3, x0, psi, c[3], nullptr, nullptr, 0.0));
    }
    if (save_every > 0 && (s + 1) % save_every == 0) {
      const int idx = (s + 1) / save_every;
      if (snap) {
        hipLaunchKernelGGL(lvc_snap_kernel, grid_of(p.snap), dim3(p.snap.tpb), 0, st, (const c128*)psi, B, m.D, nsave,
                           idx, snap);
        QD_HIP(hipGetLastError());
      }
      if (obs) QD_TRY(lvc_observe(p, m, psi, m.D, part, obs + (size_t)idx * p.nobs, rec_b, st));
    }
  }
  return QD_OK;
}

template <int NEL, int SAMPLE>
int lvc_launch_resident_driven(const LvcDrivePlan& dp, const LvcDev& m, const LvcDriveArgs& t, c128* psi, double dt,
                               int nsteps, int save_every, int nsave, c128* snap, c128* obs, hipStream_t st) {
  static const hipError_t attr =
      hipFuncSetAttribute((const void*)lvc_resident_driven_kernel<NEL, SAMPLE>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)LVC_DRIVE_LDS_MAX);
  QD_HIP(attr);
  const LvcDriveLds L{(unsigned)dp.lds_vec1, (unsigned)dp.lds_tab,  (unsigned)dp.lds_eff, (unsigned)dp.lds_drv,
                      (unsigned)dp.lds_wave, (unsigned)dp.lds_tile, (unsigned)dp.lds_nbar};
  hipLaunchKernelGGL((lvc_resident_driven_kernel<NEL, SAMPLE>), grid_of(dp.resident), dim3(dp.resident.tpb),
                     dp.resident.lds, st, m, dp.drive, L, t.Hel, t.W, t.A, t.fvals, dp.hold, psi, dt, nsteps,
                     save_every, nsave, snap, (double*)obs, dp.base.nobs);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// ---------------------------------------------------------------- pair records
int lvc_pair_refused(const LvcPairPlan& p) {
  set_error("%s", p.msg);
  return QD_EINVAL;
}

// the records of the P pairs psi [P][2][D] into rec + p * rec_pstride (complex values)
int lvc_pair_record(const LvcPairPlan& pp, const LvcDev& m, const c128* psi, double* part, c128* rec,
                    size_t rec_pstride, hipStream_t st) {
  const bool hit = dispatch_lvc_nel(m.nel, [&](auto N) {
    hipLaunchKernelGGL((lvc_pair_part_kernel<decltype(N)::value>), grid_of(pp.part), dim3(pp.part.tpb), 0, st, m,
                       pp.blocks, psi, part);
    return true;
  });
  QD_CHECK_ARG(hit, "lvc: no pair kernel for nel=%d", m.nel);
  QD_HIP(hipGetLastError());
  hipLaunchKernelGGL(lvc_pair_final_kernel, grid_of(pp.fin), dim3(pp.fin.tpb), 0, st, m.nel, pp.blocks.nblk, pp.rows,
                     pp.base.G, (const double*)part, (double*)rec, 2 * rec_pstride);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

int lvc_run_pair_staged(const LvcPairPlan& pp, const LvcDev& m, const c128* Hel, const c128* W, c128* psi, double dt,
                        int nsteps, int save_every, int nsave, c128* rec, hipStream_t st) {
  const LvcPlan& p = pp.base;
  void* w = nullptr;
  QD_TRY(workspace(WS_MISC, pp.ws_total, &w, st));
  c128* x0 = (c128*)((char*)w + p.ws_x0);
  c128* x1 = (c128*)((char*)w + p.ws_x1);
  double* part = (double*)((char*)w + pp.ws_part);
  const size_t rec_p = (size_t)(nsave + 1) * pp.nrec;
  QD_TRY(lvc_pair_record(pp, m, psi, part, rec, rec_p, st));
  const double c[4] = {dt * 0.25, dt / 3.0, dt * 0.5, dt};   // rk4_horner_coef
  for (int s = 0; s < nsteps; ++s) {
    QD_TRY(lvc_stage(p, m, Hel, W, psi, psi, x0, c[0], st));
    QD_TRY(lvc_stage(p, m, Hel, W, x0, psi, x1, c[1], st));
    QD_TRY(lvc_stage(p, m, Hel, W, x1, psi, x0, c[2], st));
    QD_TRY(lvc_stage(p, m, Hel, W, x0, psi, psi, c[3], st));
    if ((s + 1) % save_every == 0)
      QD_TRY(lvc_pair_record(pp, m, psi, part, rec + (size_t)((s + 1) / save_every) * pp.nrec, rec_p, st));
  }
  return QD_OK;
}

template <int NEL>
int lvc_launch_resident_pair(const LvcPairPlan& pp, const LvcDev& m, const c128* Hel, const c128* W, c128* psi,
                             double dt, int nsteps, int save_every, int nsave, c128* rec, hipStream_t st) {
  static const hipError_t attr = hipFuncSetAttribute((const void*)lvc_resident_pair_kernel<NEL>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)LVC_LDS_MAX);
  QD_HIP(attr);
  const LvcPairLds L{(unsigned)pp.lds_ket1, (unsigned)pp.lds_bra0, (unsigned)pp.lds_bra1,
                     (unsigned)pp.lds_tab,  (unsigned)pp.lds_wave, (unsigned)pp.lds_tile};
  hipLaunchKernelGGL((lvc_resident_pair_kernel<NEL>), grid_of(pp.resident), dim3(pp.resident.tpb), pp.resident.lds,
                     st, m, pp.blocks, L, Hel, W, psi, dt, nsteps, save_every, nsave, (double*)rec, pp.nrec);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

}  // namespace
}  // namespace qd

using namespace qd;

extern "C" int qd_lvc_apply(const qd_c128* psi, qd_c128* out, int B, int nel, int M, const int* dims,
                            const double* omega, const qd_c128* Hel, const qd_c128* W, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  QD_CHECK_ARG(psi && out && omega && Hel && W, "qd_lvc_apply: null pointer");
  QD_CHECK_ARG(psi != out, "qd_lvc_apply: out must not be psi");
  const LvcPlan p = lvc_plan("qd_lvc_apply", B, nel, M, dims);
  if (p.refused) return lvc_refused(p);
  return lvc_stage(p, lvc_dev(p, omega), (const c128*)Hel, (const c128*)W, (const c128*)psi, nullptr, (c128*)out, 0.0,
                   st);
}

extern "C" int qd_lvc_rk4(qd_c128* psi, int B, int nel, int M, const int* dims, const double* omega,
                          const qd_c128* Hel, const qd_c128* W, double dt, int nsteps, int save_every, qd_c128* snap,
                          qd_c128* obs, int path, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi && omega && Hel && W, "qd_lvc_rk4: null pointer");
  const LvcPlan p = lvc_plan("qd_lvc_rk4", B, nel, M, dims, path, nsteps, save_every, obs != nullptr);
  if (p.refused) return lvc_refused(p);
  const LvcDev m = lvc_dev(p, omega);
  const int nsave = save_every > 0 ? nsteps / save_every : 0;
  if (p.path == LVC_RESIDENT) {
    note_path("lvc_resident");
    int rc = QD_OK;
    const bool hit = dispatch_lvc_nel(nel, [&](auto N) {
      rc = lvc_launch_resident<decltype(N)::value>(p, m, (const c128*)Hel, (const c128*)W, (c128*)psi, dt, nsteps,
                                                   save_every, nsave, (c128*)snap, (c128*)obs, st);
      return true;
    });
    QD_CHECK_ARG(hit, "qd_lvc_rk4: no resident kernel for nel=%d", nel);
    return rc;
  }
  note_path("lvc_staged");
  return lvc_run_staged(p, m, (const c128*)Hel, (const c128*)W, (c128*)psi, B, dt, nsteps, save_every, nsave,
                        (c128*)snap, (c128*)obs, st);
}

extern "C" int qd_lvc_observe(const qd_c128* psi, int B, int nel, int M, const int* dims, qd_c128* obs, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi && obs, "qd_lvc_observe: null pointer");
  const LvcPlan p = lvc_plan("qd_lvc_observe", B, nel, M, dims);
  if (p.refused) return lvc_refused(p);
  void* w = nullptr;
  QD_TRY(workspace(WS_MISC, p.ws_part_bytes, &w, st));
  return lvc_observe(p, p.dev, (const c128*)psi, p.dev.D, (double*)w, (c128*)obs, p.nobs, st);
}

extern "C" int qd_lvc_driven_rk4(qd_c128* psi, int B, int nel, int M, const int* dims, const double* omega,
                                 const qd_c128* Hel, const qd_c128* W, int nd, const qd_c128* A, const int* drive_mode,
                                 const qd_c128* fvals, int nf, int sample, int hold, double dt, int nsteps,
                                 int save_every, qd_c128* snap, qd_c128* obs, int path, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi && omega && Hel && W, "qd_lvc_driven_rk4: null pointer");
  const LvcDrivePlan dp = lvc_drive_plan("qd_lvc_driven_rk4", B, nel, M, dims, nd, drive_mode, sample, hold, nf, path,
                                         nsteps, save_every, obs != nullptr);
  if (dp.refused) {
    set_error("%s", dp.msg);
    return QD_EINVAL;
  }
  // a call that reads no row (no steps) needs no fvals: an empty [0][nd] array may be null
  QD_CHECK_ARG(nd == 0 || (A && (fvals || dp.rows_needed == 0)), "qd_lvc_driven_rk4: null A or fvals with nd=%d", nd);
  const LvcDev m = lvc_dev(dp.base, omega);
  const LvcDriveArgs t{(const c128*)Hel, (const c128*)W, (const c128*)A, (const c128*)fvals};
  const int nsave = save_every > 0 ? nsteps / save_every : 0;
  if (dp.base.path == LVC_RESIDENT) {
    note_path("lvc_driven_resident");
    int rc = QD_OK;
    const bool hit = dispatch_lvc_nel(nel, [&](auto N) {
      constexpr int NEL = decltype(N)::value;
      rc = sample == LVC_STAGE
               ? lvc_launch_resident_driven<NEL, 1>(dp, m, t, (c128*)psi, dt, nsteps, save_every, nsave, (c128*)snap,
                                                    (c128*)obs, st)
               : lvc_launch_resident_driven<NEL, 0>(dp, m, t, (c128*)psi, dt, nsteps, save_every, nsave, (c128*)snap,
                                                    (c128*)obs, st);
      return true;
    });
    QD_CHECK_ARG(hit, "qd_lvc_driven_rk4: no resident kernel for nel=%d", nel);
    return rc;
  }
  note_path("lvc_driven_staged");
  return lvc_run_driven_staged(dp, m, t, (c128*)psi, B, dt, nsteps, save_every, nsave, (c128*)snap, (c128*)obs, st);
}

extern "C" int qd_lvc_pair_observe(const qd_c128* psi, int P, int nel, int M, const int* dims, int nblk,
                                   const int* blocks, qd_c128* rec, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi && rec, "qd_lvc_pair_observe: null pointer");
  const LvcPairPlan pp = lvc_pair_plan("qd_lvc_pair_observe", P, nel, M, dims, nblk, blocks);
  if (pp.refused) return lvc_pair_refused(pp);
  void* w = nullptr;
  QD_TRY(workspace(WS_MISC, pp.ws_part_bytes, &w, st));
  return lvc_pair_record(pp, pp.base.dev, (const c128*)psi, (double*)w, (c128*)rec, pp.nrec, st);
}

extern "C" int qd_lvc_pair_rk4(qd_c128* psi, int P, int nel, int M, const int* dims, const double* omega,
                               const qd_c128* Hel, const qd_c128* W, double dt, int nsteps, int save_every, int nblk,
                               const int* blocks, qd_c128* rec, int path, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi && omega && Hel && W && rec, "qd_lvc_pair_rk4: null pointer");
  const LvcPairPlan pp = lvc_pair_plan("qd_lvc_pair_rk4", P, nel, M, dims, nblk, blocks, path, nsteps, save_every);
  if (pp.refused) return lvc_pair_refused(pp);
  const LvcDev m = lvc_dev(pp.base, omega);
  const int nsave = save_every > 0 ? nsteps / save_every : 0;
  if (pp.base.path == LVC_RESIDENT) {
    note_path("lvc_pair_resident");
    int rc = QD_OK;
    const bool hit = dispatch_lvc_nel(nel, [&](auto N) {
      rc = lvc_launch_resident_pair<decltype(N)::value>(pp, m, (const c128*)Hel, (const c128*)W, (c128*)psi, dt, nsteps,
                                                        save_every, nsave, (c128*)rec, st);
      return true;
    });
    QD_CHECK_ARG(hit, "qd_lvc_pair_rk4: no resident kernel for nel=%d", nel);
    return rc;
  }
  note_path("lvc_pair_staged");
  return lvc_run_pair_staged(pp, m, (const c128*)Hel, (const c128*)W, (c128*)psi, dt, nsteps, save_every, nsave,
                             (c128*)rec, st);
}
