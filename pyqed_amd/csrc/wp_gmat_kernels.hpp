// wp_gmat_kernels.hpp — kernels of the curvilinear (G-matrix) wavepacket propagator (wp_gmat.hip) in two and three
// coordinates, psi [B][nx][ny] or [B][nx][ny][nz] (on coupled surfaces [B][ns][...], below).
//
//   D_a f   = IFFT_a(k_a FFT_a f)                                  (1/n folded into the k tables)
//   phi_r   = sum_s G_rs D_s y                                     (summed from the x term, s ascending)
//   H y     = 1/2 (D_x phi_x + D_y phi_y) + v y                    in two coordinates,
//             1/2 ((D_x phi_x + D_y phi_y) + D_z phi_z) + v y      in three
//
// Two coordinates, power-of-two grids: two fused passes per application of H, every transform on LDS
// (fft_lds<L, INV>).
//   column pass (x, strided axis): a tile of C columns, each tile row one C x 16 B segment; y and D_y y in,
//                                  u = D_x phi_x and phi_y out
//   row pass (y, contiguous axis): R whole rows; D_y phi_y, H y, the Horner update, and D_y of the new state
// Three coordinates, powers of two in [16, 256] on every axis: every pass a kernel over an [O][L][I] view of the grid.
//   X  (L = nx, I = ny nz)   y, D_y y, D_z y and the nine metric entries in; D_x y, then phi_x, formed in LDS;
//                            u = D_x phi_x, phi_y, phi_z out
//   Y  (L = ny, I = nz)      u += D_y phi_y in place (ACC), or dst = D_y src (the prologue and the pass behind Z)
//   Z  (L = nz, I = 1)       whole lines: the row pass over nx ny rows of nz points, which is the same arithmetic
//                            (D phi, H y, the Horner update, D of the new state)
// X and Y take strided tiles of C = min(16, 1024 / L) consecutive inner indices, 4 points per thread, LDS lines padded
// to L + 1 (the stores transpose).  L <= 256 keeps C >= 4: a tile row is at least one 64 B segment.
// Any other grid: element-wise kernels, templates on the number of coordinates, around fft_lines (qd_common.hpp).
//
// Coupled surfaces: psi [B][ns][nx][ny], the states as planes, so every pass sees B ns members; the potential
// V [ns][ns][nx][ny], and v y of plane a becomes sum_b V_ab y_b (b ascending from V_a0 y_0, added to the kinetic half
// last).  The sum reads every plane of the member at the thread's own points: with ns > 1 the array a stage writes
// must not be the one it reads there (wp_gmat.hip ping-pongs y).  ns = 1 is the single-surface arithmetic.
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

// V y with its fused multiply-adds written out.  The single-surface kernels formed this product with cmul and took the
// compiler's contraction of it, which chose the fused product of the imaginary part differently in the row pass and in
// the any-grid kernel; both choices are spelled here so that those entry points keep their bits whatever a compiler
// contracts around a loop over states.
__device__ __forceinline__ c128 wpg_vy_row(c128 v, c128 y) {
  return cmk(fma(v.re, y.re, -(v.im * y.im)), fma(v.im, y.re, v.re * y.im));
}
__device__ __forceinline__ c128 wpg_vy_any(c128 v, c128 y) {
  return cmk(fma(v.re, y.re, -(v.im * y.im)), fma(v.re, y.im, v.im * y.re));
}

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

// Row pass over rows r0 .. r0 + R - 1 of plane a of member m (blockIdx.x = (m ns + a) (nx / R) + r0 / R), L = ny.
//   WPG_PRO:   dy = D_y ys
//   WPG_APPLY: ynew = 1/2 (u + D_y phy) + sum_b V_ab ys_b                        (v null: no potential)
//   WPG_STAGE: ynew = psi - i coef (1/2 (u + D_y phy) + sum_b V_ab ys_b), also to snap when given; dy = D_y ynew
// ynew may be psi (read at the thread's own plane and points only).  ynew may be ys for ns = 1 alone: a thread reads
// the points it writes before it writes them, but the planes b != a of ys belong to other workgroups.
// In three coordinates this kernel is the Z pass, over nx ny rows of nz points: a change here changes those bits too.
enum WpgRowMode { WPG_PRO = 0, WPG_APPLY = 1, WPG_STAGE = 2 };

template <int L, int MODE>
__global__ __launch_bounds__(wpg_row_r(L) * L / 4) void wp2_gmat_row_kernel(const c128* phy, const c128* u,
                                                                            const c128* ys, const c128* psi,
                                                                            const c128* v, const c128* twy,
                                                                            const double* kys, int nx, int ns,
                                                                            double coef, c128* ynew, c128* dy,
                                                                            c128* snap, size_t sstride) {
  constexpr int R = wpg_row_r(L), BD = R * L / 4;
  __shared__ c128 tw[L], A[R * L], Bf[R * L];
  __shared__ double ks[L];
  const int tid = threadIdx.x, nblk = nx / R;
  const int mp = blockIdx.x / nblk, sa = mp % ns;            // plane mp = m ns + sa
  const size_t npts = (size_t)nx * L;
  const size_t vo = (size_t)(blockIdx.x % nblk) * R * L;   // the tile is R L contiguous points
  const size_t po = (size_t)mp * npts + vo;
  c128 ph[4], uv[4], vy[4], ps[4];   // ph: phy, or ys itself in WPG_PRO; vy: sum_b V_ab ys_b
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + n * BD;
    ph[n] = MODE != WPG_PRO ? phy[po + e] : ys[po + e];
    uv[n] = MODE != WPG_PRO ? u[po + e] : cmk(0, 0);
    ps[n] = MODE == WPG_STAGE ? psi[po + e] : cmk(0, 0);
    vy[n] = cmk(0, 0);
  }
  if (MODE != WPG_PRO && v) {
    const c128* yb = ys + (size_t)(mp - sa) * npts + vo;   // plane 0 of this member
    const c128* vb = v + (size_t)sa * ns * npts + vo;      // V_a0
#pragma unroll
    for (int n = 0; n < 4; ++n) vy[n] = wpg_vy_row(vb[tid + n * BD], yb[tid + n * BD]);
    for (int b = 1; b < ns; ++b) {
      yb += npts;
      vb += npts;
#pragma unroll
      for (int n = 0; n < 4; ++n) vy[n] = cadd(vy[n], wpg_vy_row(vb[tid + n * BD], yb[tid + n * BD]));
    }
  }
  for (int k = tid; k < L; k += BD) {
    tw[k] = twy[k];
    ks[k] = kys[k];
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) A[tid + n * BD] = ph[n];
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
    const c128 h = cadd(cscale(cadd(uv[n], cur[e]), 0.5), vy[n]);
    if (MODE == WPG_APPLY) {
      ynew[po + e] = h;
    } else {
      const c128 yn = cadd(ps[n], cscale(cmulmi(h), coef));
      ynew[po + e] = yn;
      if (snap) snap[(size_t)(mp / ns) * sstride + (size_t)sa * npts + vo + e] = yn;
      cur[e] = yn;   // the slot this thread read
    }
  }
  if (MODE == WPG_APPLY) return;
  __syncthreads();
  cur = wpg_deriv<L, L, R>(cur, cur == A ? Bf : A, tw, ks, tid);
#pragma unroll
  for (int n = 0; n < 4; ++n) dy[po + tid + n * BD] = cur[tid + n * BD];
}

// ---------------------------------------------------------------- three coordinates: the X and Y passes
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

// One state-sized array per coordinate
template <int D>
struct WpgVec {
  c128* p[D];
};

// d <- G d per point of every member (npts points per member), G [npts][D][D], each row summed from its x term
template <int D>
__global__ void wpg_gprod_kernel(WpgVec<D> d, const double* __restrict__ G, long n, long npts) {
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    const double* g = G + D * D * (f % npts);
    c128 in[D];
#pragma unroll
    for (int s = 0; s < D; ++s) in[s] = d.p[s][f];
#pragma unroll
    for (int r = 0; r < D; ++r) {
      c128 phi = cadd(cscale(in[0], g[D * r]), cscale(in[1], g[D * r + 1]));
#pragma unroll
      for (int s = 2; s < D; ++s) phi = cadd(phi, cscale(in[s], g[D * r + s]));
      d.p[r][f] = phi;
    }
  }
}

// h = 1/2 (u_x + u_y (+ u_z)) + sum_b V_ab ys_b, the kinetic terms summed from u_x, over the [B ns] planes of npts
// points (plane f / npts = m ns + a; v null: no potential);  psi null: ynew = h;  else ynew = psi - i coef h (also to
// snap when given).  ynew may be ys for ns = 1 alone.
template <int D>
__global__ void wpg_combine_kernel(WpgVec<D> u, const c128* ys, const c128* psi, const c128* v, long n, long npts,
                                   int ns, double coef, c128* ynew, c128* snap, size_t sstride) {
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
    c128 k = cadd(u.p[0][f], u.p[1][f]);
#pragma unroll
    for (int s = 2; s < D; ++s) k = cadd(k, u.p[s][f]);
    const c128 h = cadd(cscale(k, 0.5), vy);
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
