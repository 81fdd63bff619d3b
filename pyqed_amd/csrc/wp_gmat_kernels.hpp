// wp_gmat_kernels.hpp — kernels of the curvilinear (G-matrix) wavepacket propagator (wp_gmat.hip), psi [B][nx][ny].
//
//   D_x f = IFFT_x(kx FFT_x f)     D_y f = IFFT_y(ky FFT_y f)      (1/n folded into the k tables)
//   phi_x = Gxx D_x y + Gxy D_y y   phi_y = Gyx D_x y + Gyy D_y y
//   H y   = 1/2 (D_x phi_x + D_y phi_y) + v y
//
// Power-of-two grids: two fused passes per application of H, every transform on LDS (fft_lds<L, INV>).
//   column pass (x, strided axis): a tile of C columns, each tile row one C x 16 B segment; y and D_y y in,
//                                  u = D_x phi_x and phi_y out
//   row pass (y, contiguous axis): R whole rows; D_y phi_y, H y, the Horner update, and D_y of the new state
// Any other grid: element-wise kernels around fft_lines (qd_common.hpp).
#pragma once

#include "spo_fft_pow2.hpp"

namespace qd {
namespace {

// Rows per row-pass workgroup and columns per column-pass workgroup: 4 points per thread.  The column tile has two
// widths: the narrow one keeps two buffers within 33 KB of LDS and 256 threads; the wide one (nx >= 512: 4 columns,
// 64 B per tile row where the narrow tile has 32 or 16) takes 512 or 1024 threads and 78 or 152 KB, and is used when
// it still leaves a workgroup for every CU (wp_gmat.hip).  Same arithmetic per line, so the same bits.
constexpr int wpg_row_r(int L) { return L <= 256 ? 256 / L : 1; }
constexpr int wpg_col_c(int L) { return L <= 64 ? 16 : 1024 / L; }
constexpr int WPG_WIDE_MIN_NX = 512, WPG_WIDE_C = 4;
constexpr int wpg_col_wide(int L) { return L >= WPG_WIDE_MIN_NX ? WPG_WIDE_C : wpg_col_c(L); }
constexpr size_t wpg_col_lds(int L, int C) { return (size_t)(L + 2 * C * (L + 1)) * sizeof(c128) + L * sizeof(double); }

// ks[k] = k[k] / n: the multiplier of a forward / inverse transform pair
__global__ void wpg_ktable_kernel(const double* k, int n, double* ks) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) ks[e] = k[e] / (double)n;
}

// D of NL lines of length L held in LDS at cur + line * LP (4 NL L / 4 threads, thread tid: line tid / (L / 4)):
// forward transform, * ks, inverse transform.  The caller has a barrier behind its writes to cur; returns the buffer
// that holds the result (the same one for every line), behind a barrier.
template <int L, int LP, int NL>
__device__ __forceinline__ c128* wpg_deriv(c128* cur, c128* oth, const c128* tw, const double* ks, int tid) {
  constexpr int T = L / 4, BD = NL * T;
  const int fo = (tid / T) * LP, t = tid % T;
  c128* r = fft_lds<L, false>(cur + fo, oth + fo, tw, t, true);
  if (r != cur + fo) {
    c128* tmp = cur;
    cur = oth;
    oth = tmp;
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD, a = (e / L) * LP + e % L;
    cur[a] = cscale(cur[a], ks[e % L]);
  }
  __syncthreads();
  r = fft_lds<L, true>(cur + fo, oth + fo, tw, t, true);
  return r == cur + fo ? cur : oth;
}

// Column pass over columns j0 .. j0 + C - 1 of member m (blockIdx.x = m (ny / C) + j0 / C), L = nx; line stride L + 1
// in LDS (the transposing stores of a tile row would otherwise all land in one bank).
template <int L, int C>
__global__ __launch_bounds__(C * L / 4) void wp2_gmat_col_kernel(const c128* y, const c128* dy, const double* G,
                                                                 const c128* twx, const double* kxs, int ny, c128* u,
                                                                 c128* phy) {
  constexpr int LP = L + 1, BD = C * L / 4;
  extern __shared__ c128 sm[];   // wpg_col_lds(L, C) bytes
  c128 *tw = sm, *A = sm + L, *Bf = A + C * LP;
  double* ks = (double*)(Bf + C * LP);
  const int tid = threadIdx.x, nblk = ny / C;
  const int m = blockIdx.x / nblk, j0 = (blockIdx.x % nblk) * C;
  const size_t mo = (size_t)m * L * ny;
  c128 yv[4], dv[4];
  double g[4][4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {   // element e: tile row e / C, column e % C
    const int e = tid + n * BD;
    const size_t p = (size_t)(e / C) * ny + j0 + e % C;
    yv[n] = y[mo + p];
    dv[n] = dy[mo + p];
#pragma unroll
    for (int q = 0; q < 4; ++q) g[n][q] = G[4 * p + q];
  }
  for (int k = tid; k < L; k += BD) {
    tw[k] = twx[k];
    ks[k] = kxs[k];
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD;
    A[(e % C) * LP + e / C] = yv[n];
  }
  __syncthreads();
  c128* cur = wpg_deriv<L, LP, C>(A, Bf, tw, ks, tid);
#pragma unroll
  for (int n = 0; n < 4; ++n) {   // every thread rewrites the slots it reads: no barrier between
    const int e = tid + n * BD, a = (e % C) * LP + e / C;
    const size_t p = (size_t)(e / C) * ny + j0 + e % C;
    const c128 dx = cur[a];
    phy[mo + p] = cadd(cscale(dx, g[n][2]), cscale(dv[n], g[n][3]));
    cur[a] = cadd(cscale(dx, g[n][0]), cscale(dv[n], g[n][1]));
  }
  __syncthreads();
  cur = wpg_deriv<L, LP, C>(cur, cur == A ? Bf : A, tw, ks, tid);
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD;
    u[mo + (size_t)(e / C) * ny + j0 + e % C] = cur[(e % C) * LP + e / C];
  }
}

// Row pass over rows r0 .. r0 + R - 1 of member m (blockIdx.x = m (nx / R) + r0 / R), L = ny.
//   WPG_PRO:   dy = D_y ys
//   WPG_APPLY: ynew = 1/2 (u + D_y phy) + v ys                                  (v null: no potential)
//   WPG_STAGE: ynew = psi - i coef (1/2 (u + D_y phy) + v ys), also to snap when given; dy = D_y ynew
// ynew may be ys or psi: a thread reads the points it writes before it writes them.
enum WpgRowMode { WPG_PRO = 0, WPG_APPLY = 1, WPG_STAGE = 2 };

template <int L, int MODE>
__global__ __launch_bounds__(wpg_row_r(L) * L / 4) void wp2_gmat_row_kernel(const c128* phy, const c128* u,
                                                                            const c128* ys, const c128* psi,
                                                                            const c128* v, const c128* twy,
                                                                            const double* kys, int nx, double coef,
                                                                            c128* ynew, c128* dy, c128* snap,
                                                                            size_t sstride) {
  constexpr int R = wpg_row_r(L), BD = R * L / 4;
  __shared__ c128 tw[L], A[R * L], Bf[R * L];
  __shared__ double ks[L];
  const int tid = threadIdx.x, nblk = nx / R;
  const int m = blockIdx.x / nblk;
  const size_t vo = (size_t)(blockIdx.x % nblk) * R * L;   // the tile is R L contiguous points
  const size_t po = (size_t)m * nx * L + vo;
  c128 yv[4], ph[4], uv[4], vv[4], ps[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD;
    yv[n] = ys[po + e];
    ph[n] = MODE != WPG_PRO ? phy[po + e] : cmk(0, 0);
    uv[n] = MODE != WPG_PRO ? u[po + e] : cmk(0, 0);
    vv[n] = MODE != WPG_PRO && v ? v[vo + e] : cmk(0, 0);
    ps[n] = MODE == WPG_STAGE ? psi[po + e] : cmk(0, 0);
  }
  for (int k = tid; k < L; k += BD) {
    tw[k] = twy[k];
    ks[k] = kys[k];
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) A[tid + n * BD] = MODE == WPG_PRO ? yv[n] : ph[n];
  __syncthreads();
  c128* cur = wpg_deriv<L, L, R>(A, Bf, tw, ks, tid);
  if (MODE == WPG_PRO) {
#pragma unroll
    for (int n = 0; n < 4; ++n) dy[po + tid + n * BD] = cur[tid + n * BD];
    return;
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD;
    const c128 h = cadd(cscale(cadd(uv[n], cur[e]), 0.5), cmul(vv[n], yv[n]));
    if (MODE == WPG_APPLY) {
      ynew[po + e] = h;
    } else {
      const c128 yn = cadd(ps[n], cscale(cmulmi(h), coef));
      ynew[po + e] = yn;
      if (snap) snap[(size_t)m * sstride + vo + e] = yn;
      cur[e] = yn;   // the slot this thread read
    }
  }
  if (MODE == WPG_APPLY) return;
  __syncthreads();
  cur = wpg_deriv<L, L, R>(cur, cur == A ? Bf : A, tw, ks, tid);
#pragma unroll
  for (int n = 0; n < 4; ++n) dy[po + tid + n * BD] = cur[tid + n * BD];
}

// ---------------------------------------------------------------- any grid: element-wise kernels around fft_lines
// dst[o][k][i] = s[k] src[o][pos(k)][i] over the [O][L][I] grid of n points: pos(k) the slot of bin k in fft_lines'
// output (four-step order when l2 != 0, else k itself); s null: the reordering alone.
__global__ void wpg_pick_kernel(const c128* __restrict__ src, c128* __restrict__ dst, const double* __restrict__ s,
                                long n, int L, long I, int l2) {
  const int l1 = l2 ? L / l2 : 1;
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    const long o = f / ((long)L * I), r = f - o * L * I;
    const int k = (int)(r / I);
    const long i = r - (long)k * I;
    const int pos = l2 ? (k % l1) * l2 + k / l1 : k;
    const c128 z = src[((size_t)o * L + pos) * I + i];
    dst[f] = s ? cscale(z, s[k]) : z;
  }
}

// (a, b) <- (Gxx a + Gxy b, Gyx a + Gyy b) per point of every member (npts points per member)
__global__ void wpg_gprod_kernel(c128* a, c128* b, const double* __restrict__ G, long n, long npts) {
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    const double* g = G + 4 * (f % npts);
    const c128 dx = a[f], dv = b[f];
    a[f] = cadd(cscale(dx, g[0]), cscale(dv, g[1]));
    b[f] = cadd(cscale(dx, g[2]), cscale(dv, g[3]));
  }
}

// h = 1/2 (u + w) + v ys;  psi null: ynew = h;  else ynew = psi - i coef h (also to snap when given)
__global__ void wpg_combine_kernel(const c128* u, const c128* w, const c128* ys, const c128* psi, const c128* v,
                                   long n, long npts, double coef, c128* ynew, c128* snap, size_t sstride) {
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    const long m = f / npts, p = f - m * npts;
    const c128 yv = ys[f];
    const c128 h = cadd(cscale(cadd(u[f], w[f]), 0.5), cmul(v ? v[p] : cmk(0, 0), yv));
    if (!psi) {
      ynew[f] = h;
      continue;
    }
    const c128 yn = cadd(psi[f], cscale(cmulmi(h), coef));
    ynew[f] = yn;
    if (snap) snap[(size_t)m * sstride + p] = yn;
  }
}

}  // namespace
}  // namespace qd
