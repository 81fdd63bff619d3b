// spo_expm.hip — the point propagators exp(-i V dt/2), exp(-i V dt) of the split-operator build for any number of
// states (qd_spo_expm; spo.hip evaluates ns <= 2 in closed form).
#include "qd_common.hpp"

#include "fft_plan.hpp"   // LDS_MAX

namespace qd {
namespace spog {

// ---------------------------------------------------------------- point propagators, any ns
// exp(-i V tau) per grid point for the SPO build (wpd.py:585-623 SPO2, :1290-1330 SPO3: eigh -> U e^{-iw tau} U^+;
// wpd.py:960-985 SPO2NH: eig -> U_R e^{-iw tau} U_R^-1).  Both are the matrix exponential; here it is evaluated
// directly, by scaling and squaring a degree-18 Taylor polynomial (||X|| <= 1/2 after scaling: truncation
// < 1e-22), so no eigenvectors are needed on the device.  exp(-i V dt) = exp(-i V dt/2)^2 (one more product).
// herm: the Hermitian matrix LAPACK's eigh sees (lower triangle, real diagonal); otherwise the full matrix.
// One workgroup per grid point (grid-stride), lane e = i ns + j owns element (i, j).  GLB = false: the four ns x ns
// matrices live in LDS (ns <= 50: 160 KB at ns = 50); GLB = true (50 < ns <= 1024): in a per-workgroup slice of a
// global scratch buffer (64 ns^2 bytes, L2-resident up to ns ~ 90), with the same code -- the workgroup barrier
// orders its global stores and loads as it does LDS ones.
template <bool CPLX, bool GLB>
__global__ __launch_bounds__(1024) void spo_expm_kernel(const void* v_, int herm, long npts, int ns, double dt,
                                                        c128* expV, c128* expVh, c128* work) {
  extern __shared__ c128 sm[];
  const int ns2 = ns * ns;
  c128* X = GLB ? work + (size_t)blockIdx.x * 4 * ns2 : sm;
  c128* T = X + ns2;
  c128* S = T + ns2;
  c128* W = S + ns2;
  __shared__ int sh_s;
  const int t0 = threadIdx.x, nt = blockDim.x;
  auto vat = [&](long p, int r, int c) {
    const size_t o = (size_t)p * ns2 + (size_t)r * ns + c;
    return CPLX ? ((const c128*)v_)[o] : cmk(((const double*)v_)[o], 0.0);
  };
  auto matmul = [&](const c128* A, const c128* B, c128* C, double scale) {   // C = scale A B (C distinct from A, B)
    __syncthreads();
    for (int e = t0; e < ns2; e += nt) {
      const int i = e / ns, j = e - i * ns;
      c128 acc = cmk(0.0, 0.0);
      for (int l = 0; l < ns; ++l) acc = cadd(acc, cmul(A[i * ns + l], B[l * ns + j]));
      C[e] = cscale(acc, scale);
    }
    __syncthreads();
  };
  for (long p = blockIdx.x; p < npts; p += gridDim.x) {
    // ||V tau||_inf (max row sum), tau = dt / 2; H (the matrix eigh / eig would see) staged in X
    const double tau = 0.5 * dt;
    for (int e = t0; e < ns2; e += nt) {
      const int i = e / ns, j = e - i * ns;
      c128 h;
      if (herm) {
        if (i == j) h = cmk(vat(p, i, i).re, 0.0);
        else h = i > j ? vat(p, i, j) : cconj(vat(p, j, i));
      } else {
        h = vat(p, i, j);
      }
      X[e] = h;
      W[e] = cmk(sqrt(h.re * h.re + h.im * h.im), 0.0);
    }
    __syncthreads();
    for (int e = t0; e < ns; e += nt) {
      double r = 0.0;
      for (int l = 0; l < ns; ++l) r += W[e * ns + l].re;
      T[e] = cmk(r, 0.0);
    }
    __syncthreads();
    if (t0 == 0) {
      double nrm = 0.0;
      for (int l = 0; l < ns; ++l) nrm = fmax(nrm, T[l].re);
      nrm *= fabs(tau);
      int sq = 0;
      if (!(nrm <= 1.7976931348623157e308)) {
        sq = -1;   // inf / NaN in V: no exponential (the host raises LinAlgError first, as eigh does)
      } else {
        while (nrm > 0.5 && sq < 1100) {   // a finite norm needs at most ~1025 halvings: the loop always ends
          nrm *= 0.5;
          ++sq;
        }
      }
      sh_s = sq;
    }
    __syncthreads();
    const int sq = sh_s;
    if (sq < 0) {
      const c128 nan = cmk(__builtin_nan(""), __builtin_nan(""));
      for (int e = t0; e < ns2; e += nt) {
        expVh[(size_t)p * ns2 + e] = nan;
        if (expV) expV[(size_t)p * ns2 + e] = nan;
      }
      __syncthreads();
      continue;
    }
    const double sc = ldexp(tau, -sq);   // tau / 2^sq without an integer shift (sq may exceed 63)
    // X = -i V tau / 2^sq ; S = I + X ; T = X
    for (int e = t0; e < ns2; e += nt) {
      const int i = e / ns, j = e - i * ns;
      const c128 x = cmulmi(cscale(X[e], sc));
      X[e] = x;
      T[e] = x;
      S[e] = cadd(x, cmk(i == j ? 1.0 : 0.0, 0.0));
    }
    for (int k = 2; k <= 18; ++k) {
      matmul(T, X, W, 1.0 / k);   // W = T X / k
      for (int e = t0; e < ns2; e += nt) {
        T[e] = W[e];
        S[e] = cadd(S[e], W[e]);
      }
    }
    for (int q = 0; q < sq; ++q) {
      matmul(S, S, W, 1.0);
      for (int e = t0; e < ns2; e += nt) S[e] = W[e];
    }
    __syncthreads();
    for (int e = t0; e < ns2; e += nt) expVh[(size_t)p * ns2 + e] = S[e];
    if (expV) {
      matmul(S, S, W, 1.0);
      for (int e = t0; e < ns2; e += nt) expV[(size_t)p * ns2 + e] = W[e];
    }
    __syncthreads();
  }
}

}  // namespace spog

// exp(-i V dt/2), exp(-i V dt) per point for any ns <= SPO_EXPM_MAX_NS (spo_expm_kernel): LDS-resident matrices up to
// ns = 50, a global scratch slice per workgroup above (grid bounded by a 512 MB slab).
int spo_expm_run(const void* v, int v_complex, int herm, long npts, int ns, double dt, c128* expV, c128* expVh,
                 hipStream_t st) {
  using namespace spog;
  if (npts == 0) return QD_OK;
  const int threads = std::min(1024, std::max(64, ((ns * ns + 63) / 64) * 64));
  if (ns <= 50) {
    const size_t lds = (size_t)4 * ns * ns * sizeof(c128);
    (void)hipFuncSetAttribute((const void*)spo_expm_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(LDS_MAX - 64));
    (void)hipFuncSetAttribute((const void*)spo_expm_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(LDS_MAX - 64));
    const int grid = (int)std::min<long>(npts, 16384);
    if (v_complex)
      hipLaunchKernelGGL((spo_expm_kernel<true, false>), dim3(grid), dim3(threads), lds, st, v, herm, npts, ns, dt,
                         expV, expVh, nullptr);
    else
      hipLaunchKernelGGL((spo_expm_kernel<false, false>), dim3(grid), dim3(threads), lds, st, v, herm, npts, ns, dt,
                         expV, expVh, nullptr);
    note_path("spo_expm_lds");
  } else {
    const size_t per = (size_t)4 * ns * ns * sizeof(c128);
    const int grid = (int)std::max<long>(1, std::min<long>({npts, 1024, (long)((512ull << 20) / per)}));
    WsScope wss_(st);
    void* work = nullptr;
    const int rc = workspace(WS_SPO, per * grid, &work, st);
    if (rc) return rc;
    if (v_complex)
      hipLaunchKernelGGL((spo_expm_kernel<true, true>), dim3(grid), dim3(threads), 0, st, v, herm, npts, ns, dt, expV,
                         expVh, (c128*)work);
    else
      hipLaunchKernelGGL((spo_expm_kernel<false, true>), dim3(grid), dim3(threads), 0, st, v, herm, npts, ns, dt,
                         expV, expVh, (c128*)work);
    note_path("spo_expm_global");
  }
  QD_HIP(hipGetLastError());
  return QD_OK;
}

}  // namespace qd
