// wp_gmat3_kernels.hpp — kernels of the three-dimensional curvilinear (G-matrix) wavepacket propagator (wp_gmat3.hip),
// psi [B][ns][nx][ny][nz], the states as planes as in wp_gmat_kernels.hpp.
//
//   D_a f   = IFFT_a(k_a FFT_a f)                                  (1/n folded into the k tables)
//   phi_r   = G_rx D_x y + G_ry D_y y + G_rz D_z y                 (summed in that order)
//   (H y)_a = 1/2 ((D_x phi_x + D_y phi_y) + D_z phi_z)_a + sum_b V_ab y_b
//
// Powers of two in [16, 256] on every axis: every transform on LDS (wpg_deriv), every pass a kernel over an
// [O][L][I] view of the grid.
//   X  (L = nx, I = ny nz)   y, D_y y, D_z y and the nine metric entries in; D_x y, then phi_x, formed in LDS;
//                            u = D_x phi_x, phi_y, phi_z out
//   Y  (L = ny, I = nz)      u += D_y phi_y in place (ACC), or dst = D_y src (the prologue and the pass behind Z)
//   Z  (L = nz, I = 1)       whole lines: the 2-D row kernel wp2_gmat_row_kernel over nx ny rows of nz points, which is
//                            the same arithmetic (D phi, H y, the Horner update, D of the new state)
// X and Y take strided tiles of C = min(16, 1024 / L) consecutive inner indices, 4 points per thread, LDS lines padded
// to L + 1 (the stores transpose).  L <= 256 keeps C >= 4: a tile row is at least one 64 B segment.
// Any other grid: element-wise kernels around fft_lines, with wpg_pick_kernel for the k multiply.
#pragma once

#include "wp_gmat_kernels.hpp"

namespace qd {
namespace {

constexpr int wpg3_c(int L) { return L <= 64 ? 16 : 1024 / L; }
constexpr bool wpg3_pow2(int n) { return n >= 16 && n <= 256 && (n & (n - 1)) == 0; }

// X pass over the tile of C inner indices i0 .. i0 + C - 1 of member m (blockIdx.x = m (I / C) + i0 / C), L = nx,
// I = ny nz (a multiple of C).  The metric is indexed by the point within the member.
template <int L>
__global__ __launch_bounds__(wpg3_c(L) * L / 4) void wp3_gmat_x_kernel(const c128* y, const c128* dy, const c128* dz,
                                                                       const double* G, const c128* twx,
                                                                       const double* kxs, long I, c128* u, c128* phy,
                                                                       c128* phz) {
  constexpr int C = wpg3_c(L), LP = L + 1, BD = C * L / 4;
  __shared__ c128 tw[L], A[C * LP], Bf[C * LP];
  __shared__ double ks[L];
  const int tid = threadIdx.x;
  const long nblk = I / C;
  const long m = blockIdx.x / nblk, i0 = (blockIdx.x % nblk) * C;
  const size_t mo = (size_t)m * L * I;
  c128 yv[4], dyv[4], dzv[4];
  double g[4][9];
#pragma unroll
  for (int n = 0; n < 4; ++n) {   // element e: tile row e / C, inner index e % C
    const int e = tid + n * BD;
    const size_t p = (size_t)(e / C) * I + i0 + e % C;
    yv[n] = y[mo + p];
    dyv[n] = dy[mo + p];
    dzv[n] = dz[mo + p];
#pragma unroll
    for (int q = 0; q < 9; ++q) g[n][q] = G[9 * p + q];
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
    const size_t p = (size_t)(e / C) * I + i0 + e % C;
    const c128 dx = cur[a];
    phy[mo + p] = cadd(cadd(cscale(dx, g[n][3]), cscale(dyv[n], g[n][4])), cscale(dzv[n], g[n][5]));
    phz[mo + p] = cadd(cadd(cscale(dx, g[n][6]), cscale(dyv[n], g[n][7])), cscale(dzv[n], g[n][8]));
    cur[a] = cadd(cadd(cscale(dx, g[n][0]), cscale(dyv[n], g[n][1])), cscale(dzv[n], g[n][2]));
  }
  __syncthreads();
  cur = wpg_deriv<L, LP, C>(cur, cur == A ? Bf : A, tw, ks, tid);
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD;
    u[mo + (size_t)(e / C) * I + i0 + e % C] = cur[(e % C) * LP + e / C];
  }
}

// Y pass over the tile of C inner indices of outer index o (blockIdx.x = o (I / C) + i0 / C) of the [O][L][I] view,
// L = ny, I = nz:  ACC: dst += D src (a thread reads the slots of dst it writes before it writes them);  else
// dst = D src.
template <int L, bool ACC>
__global__ __launch_bounds__(wpg3_c(L) * L / 4) void wp3_gmat_y_kernel(const c128* src, const c128* twy,
                                                                       const double* kys, int I, c128* dst) {
  constexpr int C = wpg3_c(L), LP = L + 1, BD = C * L / 4;
  __shared__ c128 tw[L], A[C * LP], Bf[C * LP];
  __shared__ double ks[L];
  const int tid = threadIdx.x, nblk = I / C;
  const size_t oo = (size_t)(blockIdx.x / nblk) * L * I + (size_t)(blockIdx.x % nblk) * C;
  c128 sv[4], uv[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD;
    const size_t p = oo + (size_t)(e / C) * I + e % C;
    sv[n] = src[p];
    uv[n] = ACC ? dst[p] : cmk(0, 0);
  }
  for (int k = tid; k < L; k += BD) {
    tw[k] = twy[k];
    ks[k] = kys[k];
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD;
    A[(e % C) * LP + e / C] = sv[n];
  }
  __syncthreads();
  const c128* cur = wpg_deriv<L, LP, C>(A, Bf, tw, ks, tid);
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD;
    const c128 d = cur[(e % C) * LP + e / C];
    dst[oo + (size_t)(e / C) * I + e % C] = ACC ? cadd(uv[n], d) : d;
  }
}

// ---------------------------------------------------------------- any grid: element-wise kernels around fft_lines
// (a, b, c) <- G (a, b, c) per point of every member (npts points per member), each row summed from its x term
__global__ void wpg3_gprod_kernel(c128* a, c128* b, c128* c, const double* __restrict__ G, long n, long npts) {
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    const double* g = G + 9 * (f % npts);
    const c128 dx = a[f], dy = b[f], dz = c[f];
    a[f] = cadd(cadd(cscale(dx, g[0]), cscale(dy, g[1])), cscale(dz, g[2]));
    b[f] = cadd(cadd(cscale(dx, g[3]), cscale(dy, g[4])), cscale(dz, g[5]));
    c[f] = cadd(cadd(cscale(dx, g[6]), cscale(dy, g[7])), cscale(dz, g[8]));
  }
}

// h = 1/2 ((ux + uy) + uz) + sum_b V_ab ys_b over the [B ns] planes of npts points (plane f / npts = m ns + a; v null:
// no potential);  psi null: ynew = h;  else ynew = psi - i coef h (also to snap when given).  ynew may be ys for
// ns = 1 alone.
__global__ void wpg3_combine_kernel(const c128* ux, const c128* uy, const c128* uz, const c128* ys, const c128* psi,
                                    const c128* v, long n, long npts, int ns, double coef, c128* ynew, c128* snap,
                                    size_t sstride) {
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    const long mp = f / npts, p = f - mp * npts;
    const int sa = (int)(mp % ns);
    c128 vy = cmk(0, 0);
    if (v) {
      const c128* yb = ys + (size_t)(mp - sa) * npts + p;
      const c128* vb = v + (size_t)sa * ns * npts + p;
      vy = wpg_vy_any(vb[0], yb[0]);
      for (int b = 1; b < ns; ++b) vy = cadd(vy, wpg_vy_any(vb[(size_t)b * npts], yb[(size_t)b * npts]));
    }
    const c128 h = cadd(cscale(cadd(cadd(ux[f], uy[f]), uz[f]), 0.5), vy);
    if (!psi) {
      ynew[f] = h;
      continue;
    }
    const c128 yn = cadd(psi[f], cscale(cmulmi(h), coef));
    ynew[f] = yn;
    if (snap) snap[(size_t)(mp / ns) * sstride + (size_t)sa * npts + p] = yn;
  }
}

}  // namespace
}  // namespace qd
