// glf_eig.hip — qd_lindblad_rk4_eig: Hermitian Lindblad batches at N_p = 128 propagated in the eigenbasis of
// A = -iH - 1/2 sum_c C_c^+ C_c (lindblad_eig_kernel, glf_eig_kernel.hpp; the host plan that diagonalises A and guards
// its conditioning is pyqed_amd/oqs.py).  A translation unit of its own: next to the kernels of glf.hip the kernel
// changed the batch kernel's register allocation.
#include "glf_eig_kernel.hpp"

#include <algorithm>

using namespace qd;

namespace {

// The daggers and E~^T of qd_lindblad_rk4_eig's operands (all padded to 128 by the caller).
__global__ void eig_prep_kernel(const c128* V, const c128* Vi, const c128* Ct, int nc, const c128* Et, int ne, c128* Vd,
                                c128* Vid, c128* Ctd, c128* eT) {
  constexpr int Np = EIG_NP;
  constexpr size_t NN = (size_t)Np * Np;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < NN; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / Np), j = (int)(e % Np);
    const size_t t = (size_t)j * Np + i;
    Vd[t] = cconj(V[e]);
    Vid[t] = cconj(Vi[e]);
    for (int c = 0; c < nc; ++c) Ctd[c * NN + t] = cconj(Ct[c * NN + e]);
    for (int m = 0; m < ne; ++m) eT[m * NN + t] = Et[m * NN + e];
  }
}

}  // namespace

extern "C" int qd_lindblad_rk4_eig(const qd_c128* lam, const qd_c128* V, const qd_c128* Vinv, const qd_c128* Ct, int nc,
                                   qd_c128* rho, int B, int N, double dt, int nsteps, const qd_c128* Et, int ne,
                                   qd_c128* obs, void* stream) {
  QD_CHECK_ARG(lam && V && Vinv && Ct && rho, "qd_lindblad_rk4_eig: lam, V, Vinv, Ct and rho must be non-null");
  QD_CHECK_ARG(N > 64 && N <= EIG_NP, "qd_lindblad_rk4_eig: N=%d outside (64, 128]", N);
  QD_CHECK_ARG(nc >= 1 && nc <= MAX_NC, "qd_lindblad_rk4_eig: nc=%d outside [1, %d]", nc, MAX_NC);
  QD_CHECK_ARG(B >= 1 && nsteps >= 0 && ne >= 0, "qd_lindblad_rk4_eig: bad sizes B=%d nsteps=%d ne=%d", B, nsteps, ne);
  QD_CHECK_ARG(ne == 0 || (Et && obs), "qd_lindblad_rk4_eig: Et/obs null but ne=%d", ne);
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  constexpr int Np = EIG_NP;
  constexpr size_t NN = (size_t)Np * Np;
  int rc;
  void* wops = nullptr;
  if ((rc = workspace(WS_LINDBLAD_OPS, (size_t)(2 + nc + ne) * NN * sizeof(c128), &wops, st))) return rc;
  c128* Vd = (c128*)wops;
  c128* Vid = Vd + NN;
  c128* Ctd = Vid + NN;
  c128* eT = Ctd + (size_t)nc * NN;
  const bool pad = Np != N;
  const size_t per = (size_t)(1 + nc) * NN;   // stage buffer, Y_c
  void* wst = nullptr;
  if ((rc = workspace(WS_LINDBLAD, ((size_t)B * per + (pad ? (size_t)B * NN : 0)) * sizeof(c128), &wst, st))) return rc;
  c128* scratch = (c128*)wst;
  c128* rho_p = pad ? scratch + (size_t)B * per : (c128*)rho;
  hipLaunchKernelGGL(eig_prep_kernel, dim3((int)(NN / 256)), dim3(256), 0, st, (const c128*)V, (const c128*)Vinv,
                     (const c128*)Ct, nc, (const c128*)Et, ne, Vd, Vid, Ctd, eT);
  QD_HIP(hipGetLastError());
  if (pad && (rc = glf_pad((const c128*)rho, rho_p, B, N, Np, st))) return rc;
  LindbladEigParams p{};
  p.Ct = (const c128*)Ct;
  p.Ctd = Ctd;
  p.V = (const c128*)V;
  p.Vd = Vd;
  p.Vi = (const c128*)Vinv;
  p.Vid = Vid;
  p.lam = (const c128*)lam;
  p.eT = eT;
  p.rho = rho_p;
  p.ws = scratch;
  p.obs = (c128*)obs;
  p.nc = nc;
  p.ne = ne;
  p.nsteps = nsteps;
  p.dt = dt;
  p.tbuf = nullptr;
#ifdef QD_PHASE_TIMING
  QD_HIP(hipMalloc(&p.tbuf, (size_t)B * QD_TSTRIDE * sizeof(unsigned long long)));
  QD_HIP(hipMemsetAsync(p.tbuf, 0, (size_t)B * QD_TSTRIDE * sizeof(unsigned long long), st));
#endif
  note_path("glf_eig");
  hipLaunchKernelGGL(lindblad_eig_kernel, dim3(B), dim3(CG_WG), 0, st, p);
  QD_HIP(hipGetLastError());
  if (pad && (rc = glf_unpad(rho_p, (c128*)rho, B, N, Np, st))) return rc;
#ifdef QD_PHASE_TIMING
  {   // diagnostics build: per-phase clocks to stderr (waits on the host)
    std::vector<unsigned long long> t((size_t)B * QD_TSTRIDE);
    QD_HIP(hipStreamSynchronize(st));
    QD_HIP(hipMemcpy(t.data(), p.tbuf, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    (void)hipFree(p.tbuf);
    int dev = 0, khz = 100000;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
    const char* names[6] = {"ygemm", "ystore", "xgemm", "epilogue", "obs", "basis-changes"};
    std::fprintf(stderr, "[qd phase timing] eig N=%d B=%d nsteps=%d, us per step (basis-changes: per call; mean over "
                 "workgroups):", N, B, nsteps);
    for (int q = 0; q < 6; ++q) {
      double s = 0;
      for (int b = 0; b < B; ++b) s += (double)t[(size_t)b * QD_TSTRIDE + q];
      std::fprintf(stderr, " %s %.2f", names[q], s / B / (khz * 1e-3) / (q == 5 ? 1 : std::max(1, nsteps)));
    }
    double cyc = 0, wt = 0;
    for (int b = 0; b < B; ++b) {
      cyc += (double)t[(size_t)b * QD_TSTRIDE + QD_TCLK];
      wt += (double)t[(size_t)b * QD_TSTRIDE + QD_TWALL];
    }
    const double mhz = wt > 0 ? cyc / (wt / (khz * 1e3)) / 1e6 : 0.0;
    std::fprintf(stderr, " | shader clock %.0f MHz\n", mhz);
    // the K loops' per-wave stamps (shader cycles, no barrier in front; the basis changes' two phases included)
    const char* knames[6] = {"y-head", "y-ksteps", "y-wait", "x-head", "x-ksteps", "x-wait"};
    for (int w = 0; w < 2; ++w) {
      std::fprintf(stderr, "[qd phase timing] eig K loops, wave %d, us per step:", 4 * w);
      for (int q = 0; q < 6; ++q) {
        double s = 0;
        for (int b = 0; b < B; ++b) s += (double)t[(size_t)b * QD_TSTRIDE + QD_TKLOOP + 6 * w + q];
        std::fprintf(stderr, " %s %.2f", knames[q], mhz > 0 ? s / B / mhz / std::max(1, nsteps) : 0.0);
      }
      std::fprintf(stderr, "\n");
    }
  }
#endif
  return QD_OK;
}
