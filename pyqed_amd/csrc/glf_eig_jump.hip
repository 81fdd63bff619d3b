// glf_eig_jump.hip — qd_lindblad_rk4_eig_jump: Hermitian Lindblad batches at N_p = 128 with one collapse operator,
// propagated in the eigenbasis of that operator C = W diag(mu) W^-1 (lindblad_eig_jump_kernel,
// glf_eig_jump_kernel.hpp; the host plan that diagonalises C and guards its conditioning is pyqed_amd/oqs.py).  A
// translation unit of its own: lindblad_eig_kernel and the kernels of glf.hip keep their register allocation.
#include "glf_eig_jump_kernel.hpp"

#include <algorithm>

using namespace qd;

namespace {

// The halved daggers and E~^T of qd_lindblad_rk4_eig_jump's operands (all padded to 128 by the caller).
__global__ void eig_jump_prep_kernel(const c128* W, const c128* Wi, const c128* Et, int ne, c128* Wdh, c128* Widh,
                                     c128* eT) {
  constexpr int Np = JUMP_NP;
  constexpr size_t NN = (size_t)Np * Np;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < NN; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / Np), j = (int)(e % Np);
    const size_t t = (size_t)j * Np + i;
    Wdh[t] = cscale(cconj(W[e]), 0.5);
    Widh[t] = cscale(cconj(Wi[e]), 0.5);
    for (int m = 0; m < ne; ++m) eT[m * NN + t] = Et[m * NN + e];
  }
}

}  // namespace

extern "C" int qd_lindblad_rk4_eig_jump(const qd_c128* mu, const qd_c128* At, const qd_c128* W, const qd_c128* Winv,
                                        qd_c128* rho, int B, int N, double dt, int nsteps, const qd_c128* Et, int ne,
                                        qd_c128* obs, void* stream) {
  QD_CHECK_ARG(mu && At && W && Winv && rho, "qd_lindblad_rk4_eig_jump: mu, At, W, Winv and rho must be non-null");
  QD_CHECK_ARG(N > 64 && N <= JUMP_NP, "qd_lindblad_rk4_eig_jump: N=%d outside (64, 128]", N);
  QD_CHECK_ARG(B >= 1 && nsteps >= 0 && ne >= 0, "qd_lindblad_rk4_eig_jump: bad sizes B=%d nsteps=%d ne=%d", B, nsteps,
               ne);
  QD_CHECK_ARG(ne == 0 || (Et && obs), "qd_lindblad_rk4_eig_jump: Et/obs null but ne=%d", ne);
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  constexpr int Np = JUMP_NP;
  constexpr size_t NN = (size_t)Np * Np;
  int rc;
  void* wops = nullptr;
  if ((rc = workspace(WS_LINDBLAD_OPS, (size_t)(2 + ne) * NN * sizeof(c128), &wops, st))) return rc;
  c128* Wdh = (c128*)wops;
  c128* Widh = Wdh + NN;
  c128* eT = Widh + NN;
  const bool pad = Np != N;
  const size_t per = 2 * NN;   // the two stage buffers
  void* wst = nullptr;
  if ((rc = workspace(WS_LINDBLAD, ((size_t)B * per + (pad ? (size_t)B * NN : 0)) * sizeof(c128), &wst, st))) return rc;
  c128* scratch = (c128*)wst;
  c128* rho_p = pad ? scratch + (size_t)B * per : (c128*)rho;
  hipLaunchKernelGGL(eig_jump_prep_kernel, dim3((int)(NN / 256)), dim3(256), 0, st, (const c128*)W, (const c128*)Winv,
                     (const c128*)Et, ne, Wdh, Widh, eT);
  QD_HIP(hipGetLastError());
  if (pad && (rc = glf_pad((const c128*)rho, rho_p, B, N, Np, st))) return rc;
  LindbladJumpParams p{};
  p.At = (const c128*)At;
  p.W = (const c128*)W;
  p.Wi = (const c128*)Winv;
  p.Wdh = Wdh;
  p.Widh = Widh;
  p.mu = (const c128*)mu;
  p.eT = eT;
  p.rho = rho_p;
  p.ws = scratch;
  p.obs = (c128*)obs;
  p.ne = ne;
  p.nsteps = nsteps;
  p.dt = dt;
  p.tbuf = nullptr;
#ifdef QD_PHASE_TIMING
  QD_HIP(hipMalloc(&p.tbuf, (size_t)B * QD_TSTRIDE * sizeof(unsigned long long)));
  QD_HIP(hipMemsetAsync(p.tbuf, 0, (size_t)B * QD_TSTRIDE * sizeof(unsigned long long), st));
#endif
  note_path("glf_eig_jump");
  hipLaunchKernelGGL(lindblad_eig_jump_kernel, dim3(B), dim3(CG_WG), 0, st, p);
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
    // the kernel's slots: 0 the four passes of the two basis changes, 2 the stages' GEMM (both sums of every tile),
    // 3 the tail (dagger, update, the next stage's M o v, hand-over and the pass-end barrier), 4 the observables;
    // slots 1 and 5 are not used
    const char* names[6] = {"basis-changes", nullptr, "gemm", "tail", "obs", nullptr};
    std::fprintf(stderr, "[qd phase timing] eig_jump N=%d B=%d nsteps=%d, us per step (basis-changes: per call; mean "
                 "over workgroups):", N, B, nsteps);
    for (int q = 0; q < 6; ++q) {
      if (!names[q]) continue;
      double s = 0;
      for (int b = 0; b < B; ++b) s += (double)t[(size_t)b * QD_TSTRIDE + q];
      std::fprintf(stderr, " %s %.2f", names[q], s / B / (khz * 1e-3) / (q == 0 ? 1 : std::max(1, nsteps)));
    }
    double cyc = 0, wt = 0;
    for (int b = 0; b < B; ++b) {
      cyc += (double)t[(size_t)b * QD_TSTRIDE + QD_TCLK];
      wt += (double)t[(size_t)b * QD_TSTRIDE + QD_TWALL];
    }
    std::fprintf(stderr, " | shader clock %.0f MHz\n", wt > 0 ? cyc / (wt / (khz * 1e3)) / 1e6 : 0.0);
  }
#endif
  return QD_OK;
}
