// response_kernels.hpp — device code of response.hip outside the ensemble GEMMs: the exponential every response kernel
// takes (cexp_t), the SOS propagator, the three kernels of the full (t3, t2, t1) cube, and the frequency-domain
// resolvent kernels with the zero-padding copy of their GEMM operand.
#pragma once

#include "cgemm_block.hpp"

namespace qd {
namespace {

__device__ __forceinline__ c128 cexp_t(c128 lam, double t) {
  // exp(lam * t) for real t, numpy's formula exp(re)*(cos im, sin im)
  const double er = exp(lam.re * t);
  double s, c;
  sincos(lam.im * t, &s, &c);
  return cmk(er * c, er * s);
}

__global__ void sos_propagator_kernel(const c128* U1, const c128* U2, const c128* lam, int nL, const double* t, int nt,
                                      c128* U) {
  const size_t tot = (size_t)nL * nL * nt;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % nt);
    const int b = (int)((e / nt) % nL);
    const int a = (int)(e / ((size_t)nt * nL));
    const double tk = t[k];
    c128 s = cmk(0, 0);
    for (int j = 0; j < nL; ++j) s = cadd(s, cmul(cmul(U1[(size_t)a * nL + j], cexp_t(lam[j], tk)), U2[(size_t)j * nL + b]));
    U[e] = s;
  }
}

// Y[k][q] = sum_r C[q][r] e^{lam_r t1_k} beta_r
__global__ void cube_y_kernel(const c128* C, const c128* beta, const c128* lam, int nL, const double* t1, int n1,
                              c128* Y) {
  const size_t tot = (size_t)n1 * nL;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int q = (int)(e % nL), k = (int)(e / nL);
    c128 s = cmk(0, 0);
    for (int r = 0; r < nL; ++r) s = cadd(s, cmul(C[(size_t)q * nL + r], cmul(cexp_t(lam[r], t1[k]), beta[r])));
    Y[e] = s;
  }
}

// W[j][p][k] = sum_q B[p][q] e^{lam_q t2_j} Y[k][q]
__global__ void cube_w_kernel(const c128* B, const c128* Y, const c128* lam, int nL, const double* t2, int n2, int n1,
                              c128* W) {
  const size_t tot = (size_t)n2 * nL * n1;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % n1);
    const int p = (int)((e / n1) % nL);
    const int j = (int)(e / ((size_t)n1 * nL));
    c128 s = cmk(0, 0);
    for (int q = 0; q < nL; ++q)
      s = cadd(s, cmul(cmul(B[(size_t)p * nL + q], cexp_t(lam[q], t2[j])), Y[(size_t)k * nL + q]));
    W[e] = s;
  }
}

// out[i][j][k] = i * sum_p alpha_p e^{lam_p t3_i} W[j][p][k]      ((-i)^3 = i)
// One block per (i, j) row; the p-loop coefficients are staged in LDS.
__global__ void cube_out_kernel(const c128* alpha, const c128* lam, const c128* W, int nL, const double* t3, int n3,
                                int n2, int n1, c128* out) {
  extern __shared__ c128 xs[];
  const int ij = blockIdx.x;
  const int i = ij / n2, j = ij % n2;
  for (int p = threadIdx.x; p < nL; p += blockDim.x) xs[p] = cmuli(cmul(alpha[p], cexp_t(lam[p], t3[i])));
  __syncthreads();
  const c128* Wj = W + (size_t)j * nL * n1;
  c128* o = out + ((size_t)i * n2 + j) * n1;
  for (int k = threadIdx.x; k < n1; k += blockDim.x) {
    c128 s = cmk(0, 0);
    for (int p = 0; p < nL; ++p) s = cadd(s, cmul(xs[p], Wj[(size_t)p * n1 + k]));
    o[k] = s;
  }
}

// ---- frequency-domain bilinear grids (DEOMSolver.correlation_4op_3t, heom/deom.py:1127-1209):
//   out[i][j] = sum_pq x_p(wx_i) M_pq z_q(wy_j),  x_p(w) = a_p / (-lam_p - i w),  z_q(w) = v_q / (-lam_q - i w)
// as two split-K MFMA GEMMs: W = M Z (n x n x ny), out = X W (nx x n x ny).
__device__ __forceinline__ c128 cdiv(c128 a, c128 b) {
  // Smith's algorithm (scaled, as numpy's complex division)
  if (fabs(b.re) >= fabs(b.im)) {
    const double r = b.im / b.re, d = b.re + b.im * r;
    return cmk((a.re + a.im * r) / d, (a.im - a.re * r) / d);
  }
  const double r = b.re / b.im, d = b.im + b.re * r;
  return cmk((a.re * r + a.im) / d, (a.im * r - a.re) / d);
}

// rows_w = 1: out[i][p] (ld = Kp) = coef_p / (-lam_p - i w_i) for i < nw, p < n, zero padding up to [rows][Kp]
// rows_w = 0: out[q][j] (ld = nwp) = coef_q / (-lam_q - i w_j), [Kp][nwp]
__global__ void resolvent_operand_kernel(const c128* coef, const c128* lam, int n, const double* w, int nw, int rows_w,
                                         int R, int C, c128* out) {
  const size_t tot = (size_t)R * C;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / C), c = (int)(e % C);
    const int iw = rows_w ? r : c, p = rows_w ? c : r;
    c128 v = cmk(0, 0);
    if (iw < nw && p < n) v = cdiv(coef[p], cmk(-lam[p].re, -lam[p].im - w[iw]));
    out[e] = v;
  }
}

// dst [R][C] = src [n][n] zero-padded
__global__ void pad_square_kernel(const c128* src, int n, int R, int C, c128* dst) {
  const size_t tot = (size_t)R * C;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / C), c = (int)(e % C);
    dst[e] = (r < n && c < n) ? src[(size_t)r * n + c] : cmk(0, 0);
  }
}

// out[i] = sum_n -c_n / (lam_n + i w_i)   (Lindblad_solver.correlation_*_1w, superoperator.py:603-700)
__global__ void resolvent_sum_kernel(const c128* c, const c128* lam, int n, const double* w, int nw, c128* out) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += gridDim.x * blockDim.x) {
    c128 s = cmk(0, 0);
    for (int k = 0; k < n; ++k) {
      const c128 den = cmk(lam[k].re, lam[k].im + w[i]);
      const double d2 = den.re * den.re + den.im * den.im;
      const c128 inv = cmk(den.re / d2, -den.im / d2);
      s = csub(s, cmul(c[k], inv));
    }
    out[i] = s;
  }
}

}  // namespace
}  // namespace qd
