// fft.hip — physical-unit Fourier transforms of pyqed/fft.py on the GPU.
//
//   qd_fft_axis : FFT / inverse FFT along one axis of a contiguous array viewed as
//                 [outer][n][inner], fused with fftshift, a scale factor and the
//                 phase exp(-/+ i freq x0) of pyqed.fft.fft / ifft (fft.py:11-102)
//                 and fft2 (fft.py:104-126).  Any n (numpy.fft takes every length):
//                 powers of two in [16, 1024] run one Stockham LDS kernel (spo_fft_pow2.hpp) with the
//                 epilogue fused; every other n runs the any-size engine of the SPO
//                 grids (spo_gen.hip fft_lines: mixed radix 2/3/4/5/p <= 61 in LDS,
//                 Bluestein, four-step for long smooth lengths, direct DFT for the
//                 rest) on a copy, then one shift / scale / phase pass back.
//   qd_dft2     : DFT at arbitrary momenta (fft.py:128-160 dft / dft2).
#include "spo_fft_pow2.hpp"
#include "spo_plan.hpp"

#include <cstdlib>

namespace qd {
namespace {

// post-processing of one transformed row X (natural order) into data
__device__ __forceinline__ void fft_store(const c128* X, c128* base, long stride, int n, int shift, double scale,
                                          const double* freq, double x0, int sign) {
  for (int kp = threadIdx.x; kp < n; kp += blockDim.x) {
    const int k = shift ? ((kp - n / 2) % n + n) % n : kp;
    c128 v = cscale(X[k], scale);
    if (freq) {
      double s, c;
      sincos(sign * freq[kp] * x0, &s, &c);
      v = cmul(v, cmk(c, s));
    }
    base[(long)kp * stride] = v;
  }
}

template <int L>
__global__ void fft_pow2_kernel(c128* data, int inner, int inverse, int shift, double scale, const double* freq,
                                double x0, const c128* twg) {
  __shared__ c128 tw[L], A[L], B[L];
  const long b = blockIdx.x;
  const long o = b / inner, i = b % inner;
  c128* base = data + o * (long)L * inner + i;
  for (int k = threadIdx.x; k < L; k += blockDim.x) {
    tw[k] = twg[k];
    A[k] = base[(long)k * inner];
  }
  __syncthreads();
  const int t = threadIdx.x;
  c128* X = inverse ? fft_lds<L, true>(A, B, tw, t, t < L / 4) : fft_lds<L, false>(A, B, tw, t, t < L / 4);
  fft_store(X, base, inner, L, shift, scale, freq, x0, inverse ? 1 : -1);
}

// out[o][kp][i] = scale X[o][pos(k)][i] exp(sign i freq[kp] x0), k = fftshift source of kp; pos = the slot of X[k]
// in fft_lines' output (four-step order when l2 != 0)
__global__ void fft_post_kernel(const c128* __restrict__ X, c128* __restrict__ out, long O, int n, long I, int shift,
                                double scale, const double* __restrict__ freq, double x0, int sign, int l2) {
  const long tot = O * n * I;
  const int l1 = l2 ? n / l2 : 1;
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < tot; f += (long)gridDim.x * blockDim.x) {
    const long o = f / ((long)n * I), r = f - o * n * I;
    const int kp = (int)(r / I);
    const long i = r - (long)kp * I;
    const int k = shift ? ((kp - n / 2) % n + n) % n : kp;
    const int pos = l2 ? (k % l1) * l2 + k / l1 : k;
    c128 v = cscale(X[((size_t)o * n + pos) * I + i], scale);
    if (freq) {
      double sn, c;
      sincos(sign * freq[kp] * x0, &sn, &c);
      v = cmul(v, cmk(c, sn));
    }
    out[f] = v;
  }
}

// out[i][j] = sum_{a,b} f[a][b] exp(-i (kx_i x_b + ky_j y_a)) * w    (ny == 1 / y == 0 gives 1D dft)
__global__ void dft2_kernel(const double* x, int nx, const double* y, int ny, const c128* f, const double* kx, int nkx,
                            const double* ky, int nky, double w, c128* out) {
  const int tot = nkx * nky;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += gridDim.x * blockDim.x) {
    const int i = e / nky, j = e % nky;
    c128 acc = cmk(0, 0);
    for (int a = 0; a < ny; ++a)
      for (int bb = 0; bb < nx; ++bb) {
        double s, c;
        sincos(-(kx[i] * x[bb] + ky[j] * y[a]), &s, &c);
        acc = cadd(acc, cmul(f[(long)a * nx + bb], cmk(c, s)));
      }
    out[e] = cscale(acc, w);
  }
}

}  // namespace
}  // namespace qd

using namespace qd;

extern "C" int qd_fft_axis(qd_c128* data, int outer, int n, int inner, int inverse, int shift, double scale,
                           const double* freq, double x0, void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(data, "qd_fft_axis: null pointer");
  QD_CHECK_ARG(outer >= 1 && inner >= 1 && n >= 1, "qd_fft_axis: bad sizes");
  QD_CHECK_ARG((long)outer * n * inner < (1L << 31), "qd_fft_axis: array too large (%ld elements)",
               (long)outer * n * inner);
  hipStream_t st = (hipStream_t)stream;
  const int batch = outer * inner;
  const bool pow2 = pow2_in_range(n);
  note_path(pow2 ? "fft_pow2" : "fft_any");
  if (pow2) {
    void* w = nullptr;
    int rc = workspace(WS_MISC, n * sizeof(c128), &w, st);
    if (rc) return rc;
    hipLaunchKernelGGL(twiddle_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, (c128*)w);
    QD_HIP(hipGetLastError());
    const int threads = std::max(64, n / 4);
    const bool hit = dispatch_int<16, 32, 64, 128, 256, 512, 1024>(n, [&](auto L) {
      hipLaunchKernelGGL(fft_pow2_kernel<decltype(L)::value>, dim3(batch), dim3(threads), 0, st, (c128*)data, inner,
                         inverse, shift, scale, freq, x0, (const c128*)w);
      return true;
    });
    QD_CHECK_ARG(hit, "qd_fft_axis: internal: no kernel for n = %d", n);
    QD_HIP(hipGetLastError());
    return QD_OK;
  }
  // any other length: transform a copy with the any-size engine, then shift / scale / phase back into data
  const long tot = (long)outer * n * inner;
  void* w = nullptr;
  int rc = workspace(WS_MISC, (size_t)tot * sizeof(c128), &w, st);
  if (rc) return rc;
  c128* X = (c128*)w;
  QD_TRY(copy_device(X, data, (size_t)tot * sizeof(c128), st));
  int l2 = 0;
  if ((rc = fft_lines(X, outer, n, inner, inverse != 0, st, &l2))) return rc;
  const int grid = (int)std::max<long>(1, std::min<long>((tot + 255) / 256, 16384));
  hipLaunchKernelGGL(fft_post_kernel, dim3(grid), dim3(256), 0, st, (const c128*)X, (c128*)data, (long)outer, n,
                     (long)inner, shift, scale, freq, x0, inverse ? 1 : -1, l2);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

extern "C" int qd_dft2(const double* x, int nx, const double* y, int ny, const qd_c128* f, const double* kx, int nkx,
                       const double* ky, int nky, double weight, qd_c128* out, void* stream) {
  QD_CHECK_ARG(x && y && f && kx && ky && out, "qd_dft2: null pointer");
  QD_CHECK_ARG(nx >= 1 && ny >= 1 && nkx >= 1 && nky >= 1, "qd_dft2: bad sizes");
  const int tot = nkx * nky;
  hipLaunchKernelGGL(dft2_kernel, dim3(std::min(16384, (tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, nx, y,
                     ny, (const c128*)f, kx, nkx, ky, nky, weight, (c128*)out);
  QD_HIP(hipGetLastError());
  return QD_OK;
}
