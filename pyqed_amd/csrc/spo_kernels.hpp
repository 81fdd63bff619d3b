// spo_kernels.hpp — row and column passes of the 2D split-operator step (spo.hip), psi [nx][ny][ns] with the
// state index fastest: the LDS kernels (any ns), the latency-shaped kernels (ns <= 2), the 256-point register
// kernels and the batch kernels of qd_spo2_run_batch (SPO3 runs the same row and column kernels on its z and x axes);
// the persistent 1D kernel and the point propagators exp(-i V tau).
#pragma once

#include "spo_fft_pow2.hpp"

namespace qd {
namespace {

// psi_point <- U psi_point for each grid point of one row held in LDS (buf[a][j]).
// out[a][j] = sum_b U[j][a][b] in[b][j] for the n points j of a row ([state][point] LDS layout, row
// stride `stride`).  Reads one LDS buffer and writes the other (no per-thread state arrays, which
// would be indexed at run time and land in scratch).
__device__ __forceinline__ void apply_point_op(const c128* in, c128* out, int stride, const c128* U /*[n][ns][ns]*/,
                                               int n, int ns) {
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const c128* u = U + (size_t)j * ns * ns;
    for (int a = 0; a < ns; ++a) {
      c128 s = cmk(0, 0);
      for (int b = 0; b < ns; ++b) s = cadd(s, cmul(u[a * ns + b], in[b * stride + j]));
      out[a * stride + j] = s;
    }
  }
}

enum RowFlags { ROW_INV = 1, ROW_VH1 = 2, ROW_SNAP = 4, ROW_VH2 = 8, ROW_FWD = 16, ROW_KY = 32, ROW_KZ = 64 };

// One row i of psi [nx][ny][ns]; FFTs along y (length L = ny) for each state.
// ROW_KY (Jacobi KEO, wpd.py:850-887): after FFT_y multiply by expKy[i][ky] (row i's k_y factor).
// `expVh` is the point operator of this pass (exp_V_half, or exp_V on merged passes).
template <int L>
__global__ __launch_bounds__(256) void spo2_row_kernel(c128* psi, const c128* expVh, const c128* twy, int ny, int ns,
                                                       int flags, c128* snap, const c128* expKy) {
  extern __shared__ c128 sm[];
  c128* tw = sm;            // L
  c128* A = sm + L;         // ns * L
  c128* Bf = A + ns * L;    // ns * L
  const int i = blockIdx.x;
  const size_t rowoff = (size_t)i * L * ns;
  for (int k = threadIdx.x; k < L; k += blockDim.x) tw[k] = twy[k];
  for (int e = threadIdx.x; e < L * ns; e += blockDim.x) A[(e % ns) * L + e / ns] = psi[rowoff + e];
  __syncthreads();
  const int T = L / 4;
  const int f = threadIdx.x / T, t = threadIdx.x % T;
  const bool active = f < ns;
  c128* cur = A;
  c128* oth = Bf;
  if (flags & ROW_INV) {
    c128* r = fft_lds<L, true>(A + (active ? f : 0) * L, Bf + (active ? f : 0) * L, tw, t, active);
    const bool inA = (r == A + (active ? f : 0) * L);
    cur = inA ? A : Bf;
    oth = inA ? Bf : A;
  }
  const c128* Ui = expVh + (size_t)i * L * ns * ns;
  if (flags & ROW_VH1) {
    apply_point_op(cur, oth, L, Ui, L, ns);
    c128* tmp = cur;
    cur = oth;
    oth = tmp;
    __syncthreads();
  }
  if (flags & ROW_SNAP) {
    for (int e = threadIdx.x; e < L * ns; e += blockDim.x) snap[rowoff + e] = cur[(e % ns) * L + e / ns];
    __syncthreads();
  }
  if (flags & ROW_VH2) {
    apply_point_op(cur, oth, L, Ui, L, ns);
    c128* tmp = cur;
    cur = oth;
    oth = tmp;
    __syncthreads();
  }
  if (flags & ROW_FWD) {
    c128* r = fft_lds<L, false>(cur + (active ? f : 0) * L, oth + (active ? f : 0) * L, tw, t, active);
    cur = (r == cur + (active ? f : 0) * L) ? cur : oth;
  }
  if (flags & ROW_KY) {
    const c128* ky = expKy + (size_t)i * L;
    for (int e = threadIdx.x; e < L * ns; e += blockDim.x) cur[e] = cmul(ky[e % L], cur[e]);
    __syncthreads();
  }
  for (int e = threadIdx.x; e < L * ns; e += blockDim.x) psi[rowoff + e] = cur[(e % ns) * L + e / ns];
}

// C columns j0..j0+C-1 of psi [nx][ny][ns]; FFT along x (length L = nx), multiply
// by expKT[j][i] (exp_K transposed and pre-scaled by 1/(nx ny)), inverse FFT.
template <int L, int C>
__global__ __launch_bounds__(256) void spo2_col_kernel(c128* psi, const c128* expKT, const c128* twx, int ny, int ns) {
  extern __shared__ c128 sm[];
  c128* tw = sm;                 // L
  c128* A = sm + L;              // C * ns * L   (layout [c][a][i])
  c128* Bf = A + C * ns * L;
  const int j0 = blockIdx.x * C;
  const int W = C * ns;  // transforms in this workgroup
  for (int k = threadIdx.x; k < L; k += blockDim.x) tw[k] = twx[k];
  for (int e = threadIdx.x; e < L * W; e += blockDim.x) {
    const int ca = e % W, i = e / W;
    A[ca * L + i] = psi[((size_t)i * ny + j0) * ns + ca];  // (j0 + c) * ns + a == j0*ns + ca
  }
  __syncthreads();
  const int T = L / 4;
  const int f = threadIdx.x / T, t = threadIdx.x % T;
  const bool active = f < W;
  const int fo = (active ? f : 0) * L;
  c128* r = fft_lds<L, false>(A + fo, Bf + fo, tw, t, active);
  c128* cur = (r == A + fo) ? A : Bf;
  c128* oth = (cur == A) ? Bf : A;
  for (int e = threadIdx.x; e < L * W; e += blockDim.x) {
    const int ca = e / L, i = e % L;
    const int c = ca / ns;
    cur[ca * L + i] = cmul(cur[ca * L + i], expKT[(size_t)(j0 + c) * L + i]);
  }
  __syncthreads();
  r = fft_lds<L, true>(cur + fo, oth + fo, tw, t, active);
  cur = (r == cur + fo) ? cur : oth;
  for (int e = threadIdx.x; e < L * W; e += blockDim.x) {
    const int ca = e % W, i = e / W;
    psi[((size_t)i * ny + j0) * ns + ca] = cur[ca * L + i];
  }
}

// ---------------------------------------------------------------- latency-shaped 2D passes (ns <= 2)
// At 256 x 256 x 2 a pass moves 8-16 KB per workgroup, so its time is the chain of dependent
// memory round trips, not bandwidth.  These variants issue EVERY global load of the pass (psi,
// the point operator, exp_Ky / exp_K, twiddles) before the first wait, keep the point-local work
// (V/2, snapshot, V/2, k_y phase) in registers, and touch LDS only for the FFT exchanges: one
// load round trip + one store drain per pass.  Same arithmetic, same order as the generic kernels.

// Row pass, thread j owns grid point j of row i (blockDim = max(L, 64)).
template <int L, int NS>
__global__ __launch_bounds__(L < 64 ? 64 : L) void spo2_row_fast_kernel(c128* psi, const c128* U, const c128* twy,
                                                                        int flags, c128* snap, const c128* expKy) {
  extern __shared__ c128 sm[];
  c128* tw = sm;          // L
  c128* A = sm + L;       // NS * L   ([state][point])
  c128* Bf = A + NS * L;  // NS * L
  const int i = blockIdx.x, j = threadIdx.x;
  const bool own = j < L;
  const size_t pt = (size_t)i * L + j;
  c128 p[NS], u[NS * NS], ky = cmk(1, 0);
  if (own) {
#pragma unroll
    for (int a = 0; a < NS; ++a) p[a] = psi[pt * NS + a];
    if (flags & (ROW_VH1 | ROW_VH2)) {
#pragma unroll
      for (int e = 0; e < NS * NS; ++e) u[e] = U[pt * NS * NS + e];
    }
    if (flags & ROW_KY) ky = expKy[pt];
    tw[j] = twy[j];
  }
  constexpr int T = L / 4;
  const int f = j / T, t = j % T;
  const bool active = f < NS;
  auto fft = [&](auto inv_tag) {
    constexpr bool INV = decltype(inv_tag)::value;
    if (own) {
#pragma unroll
      for (int a = 0; a < NS; ++a) A[a * L + j] = p[a];
    }
    __syncthreads();
    c128* r = fft_lds<L, INV>(A + (active ? f : 0) * L, Bf + (active ? f : 0) * L, tw, t, active);
    // fft_lds ends on a barrier; the result buffer is the same for every transform
    c128* res = (r == A + (active ? f : 0) * L) ? A : Bf;
    if (own) {
#pragma unroll
      for (int a = 0; a < NS; ++a) p[a] = res[a * L + j];
    }
    __syncthreads();  // the next FFT overwrites A
  };
  auto point_op = [&]() {
    c128 q[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      c128 s = cmk(0, 0);
#pragma unroll
      for (int b = 0; b < NS; ++b) s = cadd(s, cmul(u[a * NS + b], p[b]));
      q[a] = s;
    }
#pragma unroll
    for (int a = 0; a < NS; ++a) p[a] = q[a];
  };
  if (flags & ROW_INV) fft(std::true_type{});  // (fft's first barrier also publishes tw)
  if (flags & ROW_VH1) point_op();
  if ((flags & ROW_SNAP) && own) {
#pragma unroll
    for (int a = 0; a < NS; ++a) snap[pt * NS + a] = p[a];
  }
  if (flags & ROW_VH2) point_op();
  if (flags & ROW_FWD) fft(std::false_type{});
  if (flags & ROW_KY) {
#pragma unroll
    for (int a = 0; a < NS; ++a) p[a] = cmul(ky, p[a]);
  }
  if (own) {
#pragma unroll
    for (int a = 0; a < NS; ++a) psi[pt * NS + a] = p[a];
  }
}

// Column pass over C columns j0..j0+C-1 (W = C*NS transforms, blockDim = W*L/4): exp_K for the
// pass is loaded with psi, before the forward FFT.
template <int L, int C, int NS>
__global__ __launch_bounds__(C * NS * L / 4 < 64 ? 64 : C * NS * L / 4) void spo2_col_fast_kernel(
    c128* psi, const c128* expKT, const c128* twx, int ny) {
  constexpr int W = C * NS;
  constexpr int BD = W * L / 4 < 64 ? 64 : W * L / 4;
  constexpr int IT = (L * W + BD - 1) / BD;
  extern __shared__ c128 sm[];
  c128* tw = sm;           // L
  c128* A = sm + L;        // W * L  ([c][a][i])
  c128* Bf = A + W * L;
  const int j0 = blockIdx.x * C;
  const int tid = threadIdx.x;
  constexpr bool FULL = (L * W) % BD == 0;
  c128 v[IT], kf[IT];
#pragma unroll
  for (int n = 0; n < IT; ++n) {
    const int e = tid + n * BD;  // load order: row i = e / W, transform ca = e % W (coalesced);
    v[n] = cmk(0, 0);            // multiply order: transform ca = e / L, row i = e % L
    kf[n] = cmk(0, 0);
    if (FULL || e < L * W) {
      v[n] = psi[((size_t)(e / W) * ny + j0) * NS + e % W];
      kf[n] = expKT[(size_t)(j0 + (e / L) / NS) * L + e % L];
    }
  }
  for (int k = tid; k < L; k += BD) tw[k] = twx[k];
#pragma unroll
  for (int n = 0; n < IT; ++n) {
    const int e = tid + n * BD;
    if (FULL || e < L * W) A[(e % W) * L + e / W] = v[n];
  }
  __syncthreads();
  constexpr int T = L / 4;
  const int f = tid / T, t = tid % T;
  const bool active = f < W;
  const int fo = (active ? f : 0) * L;
  c128* r = fft_lds<L, false>(A + fo, Bf + fo, tw, t, active);
  c128* cur = (r == A + fo) ? A : Bf;
  c128* oth = (cur == A) ? Bf : A;
#pragma unroll
  for (int n = 0; n < IT; ++n) {
    const int e = tid + n * BD;
    if (FULL || e < L * W) cur[e] = cmul(cur[e], kf[n]);
  }
  __syncthreads();
  r = fft_lds<L, true>(cur + fo, oth + fo, tw, t, active);
  cur = (r == cur + fo) ? cur : oth;
#pragma unroll
  for (int n = 0; n < IT; ++n) {
    const int e = tid + n * BD;
    if (FULL || e < L * W) psi[((size_t)(e / W) * ny + j0) * NS + e % W] = cur[(e % W) * L + e / W];
  }
}

// expKT[j][i] = expK[i][j] * scale
__global__ void transpose_scale_kernel(const c128* expK, int nx, int ny, double scale, c128* expKT) {
  const size_t tot = (size_t)nx * ny;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / ny), j = (int)(e % ny);
    expKT[(size_t)j * nx + i] = cscale(expK[e], scale);
  }
}

// Row pass of spo2_row_fast_kernel for L = 256: one workgroup per row, wave c = state c (its 256-point
// transforms run on 4 values per lane).  The point operators mix the states of a point, whose values
// sit in the same lane of every wave: they are exchanged through LDS (one workgroup barrier per point
// operator).  Same flags and arithmetic order of the point work as the LDS kernels:
// [IFFT_y] -> V/2 -> [snapshot] -> [V/2] -> [FFT_y] -> [k_y phase].
// Batches of wavefunctions (qd_spo2_run_batch): blockIdx.y = member w, psi / snap offset by w * wstride /
// w * sstride (the point operators are shared).
// KY: the Jacobi k_y factor is compiled in only where used (its 4 per-lane values would otherwise hold 16 VGPRs
// through the whole pass: 142 -> under 128 VGPRs, 3 -> 4 waves per SIMD for the linear case).
template <int NS, bool KY>
__global__ __launch_bounds__(64 * NS) void spo2_row_q16_kernel(c128* psi, const c128* U, const c128* twy, int flags,
                                                               c128* snap, const c128* expKy, size_t wstride = 0,
                                                               size_t sstride = 0) {
  __shared__ c128 S[NS * 272];
  __shared__ c128 Xs[NS * 256];   // point-operator exchange: [state][lane * 4 + a]
  const int i = blockIdx.x, c = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 2, s = lane & 3;
  psi += blockIdx.y * wstride;
  if (snap) snap += blockIdx.y * sstride;
  c128 x[1][4], u[4][NS], ky[4];
  const size_t row = (size_t)i * 256;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const size_t pt = row + 64 * a + 16 * s + g;
    x[0][a] = psi[pt * NS + c];
    if (flags & (ROW_VH1 | ROW_VH2)) {
#pragma unroll
      for (int b = 0; b < NS; ++b) u[a][b] = U[(pt * NS + c) * NS + b];   // row c of the point's operator
    }
    if constexpr (KY) ky[a] = expKy[pt];
  }
  const Q16Tw t = q16_twiddles(twy, g, s);
  c128* Sw = S + c * 272;
  auto point_op = [&]() {
    if (NS > 1) {
#pragma unroll
      for (int a = 0; a < 4; ++a) Xs[c * 256 + lane * 4 + a] = x[0][a];
      __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      c128 acc = cmk(0, 0);
#pragma unroll
      for (int b = 0; b < NS; ++b) acc = cadd(acc, cmul(u[a][b], NS > 1 ? Xs[b * 256 + lane * 4 + a] : x[0][a]));
      x[0][a] = acc;
    }
    if (NS > 1) __syncthreads();   // Xs is rewritten by the next operator
  };
  if (flags & ROW_INV) fft256_wave<true, 1>(x, t, Sw, g, s);
  if (flags & ROW_VH1) point_op();
  if (flags & ROW_SNAP) {
#pragma unroll
    for (int a = 0; a < 4; ++a) snap[(row + 64 * a + 16 * s + g) * NS + c] = x[0][a];
  }
  if (flags & ROW_VH2) point_op();
  if (flags & ROW_FWD) fft256_wave<false, 1>(x, t, Sw, g, s);
  if constexpr (KY) {
    if (flags & ROW_KY) {
#pragma unroll
      for (int a = 0; a < 4; ++a) x[0][a] = cmul(ky[a], x[0][a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) psi[(row + 64 * a + 16 * s + g) * NS + c] = x[0][a];
}

// Row pass for batches, one wave per (row i, member): the wave holds both states of its points (x[c][a] =
// psi[64 a + 16 s + g][c]), so the point operators are lane-local (no state exchange through LDS, no workgroup
// barrier but the one after the operator staging) and every lane loads 32 contiguous bytes per point.  The MB
// waves of a workgroup are MB members of one row and share the row's point operators, staged in LDS once.  The
// two states' 256-point transforms run one after the other through one 272-entry exchange buffer per wave (LDS
// per workgroup 16 KB + MB x 4.25 KB: four workgroups of MB = 4 per CU).  Same arithmetic and order as
// spo2_row_q16_kernel<2, false>, so the results are bit-identical.
template <int MB>
__global__ __launch_bounds__(64 * MB) void spo2_row_wave_kernel(c128* psi, const c128* U, const c128* twy, int flags,
                                                                c128* snap, int B, size_t wstride, size_t sstride) {
  __shared__ c128 Us[256 * 4];          // [point][row c][col b]
  __shared__ c128 S[MB * 272];          // per-wave FFT exchange
  const int i = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 2, s = lane & 3;
  const int member = blockIdx.y * MB + w;
  const bool live = member < B;          // uniform per wave; dead waves still join the staging barrier
  c128* ps = psi + (size_t)(live ? member : 0) * wstride;
  const size_t row = (size_t)i * 256;
  c128 x[2][4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const size_t pt = row + 64 * a + 16 * s + g;
    x[0][a] = ps[pt * 2];
    x[1][a] = ps[pt * 2 + 1];
  }
  const bool vh = flags & (ROW_VH1 | ROW_VH2);
  if (vh) {
#pragma unroll
    for (int q = 0; q < 1024 / (64 * MB); ++q) {
      const int e = threadIdx.x + 64 * MB * q;
      Us[e] = U[row * 4 + e];
    }
  }
  const Q16Tw t = q16_twiddles(twy, g, s);
  c128* Sw = S + w * 272;
  auto line = [&](int c) -> c128 (&)[1][4] { return *reinterpret_cast<c128(*)[1][4]>(&x[c][0]); };
  if (vh) __syncthreads();
  if (!live) return;
  auto point_op = [&]() {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int pt = 64 * a + 16 * s + g;
      c128 y[2];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        c128 acc = cmk(0, 0);
#pragma unroll
        for (int b = 0; b < 2; ++b) acc = cadd(acc, cmul(Us[pt * 4 + c * 2 + b], x[b][a]));
        y[c] = acc;
      }
      x[0][a] = y[0];
      x[1][a] = y[1];
    }
  };
  if (flags & ROW_INV) {
    fft256_wave<true, 1>(line(0), t, Sw, g, s);
    fft256_wave<true, 1>(line(1), t, Sw, g, s);
  }
  if (flags & ROW_VH1) point_op();
  if (flags & ROW_SNAP) {
    c128* sn = snap + (size_t)member * sstride;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const size_t pt = row + 64 * a + 16 * s + g;
      sn[pt * 2] = x[0][a];
      sn[pt * 2 + 1] = x[1][a];
    }
  }
  if (flags & ROW_VH2) point_op();
  if (flags & ROW_FWD) {
    fft256_wave<false, 1>(line(0), t, Sw, g, s);
    fft256_wave<false, 1>(line(1), t, Sw, g, s);
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const size_t pt = row + 64 * a + 16 * s + g;
    ps[pt * 2] = x[0][a];
    ps[pt * 2 + 1] = x[1][a];
  }
}

// Column pass of spo2_col_fast_kernel for L = nx = 256: one 64-lane workgroup per (column j, state c)
// (no state mixing in this pass): FFT_x -> * exp_K / (nx ny) -> IFFT_x.  Blocks of one XCD (blockIdx.x
// % 8) take a contiguous run of columns, so the pieces that adjacent columns read from one row share
// that XCD's L2 lines.
template <int NS>
__global__ __launch_bounds__(64) void spo2_col_q16_kernel(c128* psi, const c128* expKT, const c128* twx, int ncols,
                                                          int pitch, size_t wstride = 0) {
  __shared__ c128 S[272];
  const int b = blockIdx.x, c = blockIdx.y;
  psi += blockIdx.z * wstride;
  const int j = (ncols % 8 == 0) ? (b % 8) * (ncols / 8) + b / 8 : b;
  const int lane = threadIdx.x, g = lane >> 2, s = lane & 3;
  c128 x[1][4], kf[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int p = 64 * a + 16 * s + g;
    x[0][a] = psi[((size_t)p * pitch + j) * NS + c];
    kf[a] = expKT[(size_t)j * 256 + p];
  }
  const Q16Tw t = q16_twiddles(twx, g, s);
  fft256_wave<false, 1>(x, t, S, g, s);
#pragma unroll
  for (int a = 0; a < 4; ++a) x[0][a] = cmul(x[0][a], kf[a]);
  fft256_wave<true, 1>(x, t, S, g, s);
#pragma unroll
  for (int a = 0; a < 4; ++a) psi[((size_t)(64 * a + 16 * s + g) * pitch + j) * NS + c] = x[0][a];
}

// Column pass for batches with NC adjacent columns per 64 NC-thread workgroup and one wave per column holding
// both states (x[c][a], c = state): the 256 x NC x 2 tile is read and written as NC x 32-B contiguous row pieces
// (256 B at NC = 8), and the waves' FFT exchange buffers live inside the tile (it is dead between the line reads
// and the write-back), so the workgroup's LDS is the tile alone (NC = 8: 68 KB, two workgroups per CU as the
// round-3 4-column kernel).  Same arithmetic per line as spo2_col_q16_kernel.  NS = 2, nx = ny = 256.
template <int NC>
__global__ __launch_bounds__(64 * NC) void spo2_col_tile8_kernel(c128* psi, const c128* expKT, const c128* twx,
                                                                 size_t wstride) {
  constexpr int TW = 2 * NC + 1;     // tile row stride: 2 NC lines + 1 pad
  __shared__ c128 T[256 * TW];       // [row][lines]; per-wave FFT exchange T + w * 272 in between
  psi += blockIdx.y * wstride;
  const int j0 = blockIdx.x * NC;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, g = lane >> 2, s = lane & 3;
  const int j = j0 + w;
  {
    c128 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {    // element e = row * 2 NC + (column - j0) * 2 + state
      const int e = tid + 64 * NC * q, r = e / (2 * NC), cs = e % (2 * NC);
      v[q] = psi[((size_t)r * 256 + j0) * 2 + cs];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + 64 * NC * q;
      T[(e / (2 * NC)) * TW + e % (2 * NC)] = v[q];
    }
  }
  c128 kf[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) kf[a] = expKT[(size_t)j * 256 + 64 * a + 16 * s + g];
  __syncthreads();
  c128 x[2][4];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int a = 0; a < 4; ++a) x[c][a] = T[(64 * a + 16 * s + g) * TW + 2 * w + c];
  const Q16Tw t = q16_twiddles(twx, g, s);
  __syncthreads();                   // every wave has its lines: the tile becomes the FFT exchange
  c128* Sw = T + w * 272;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    c128(&xl)[1][4] = *reinterpret_cast<c128(*)[1][4]>(&x[c][0]);
    fft256_wave<false, 1>(xl, t, Sw, g, s);
#pragma unroll
    for (int a = 0; a < 4; ++a) x[c][a] = cmul(x[c][a], kf[a]);
    fft256_wave<true, 1>(xl, t, Sw, g, s);
  }
  __syncthreads();                   // every wave is done with its exchange region
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int a = 0; a < 4; ++a) T[(64 * a + 16 * s + g) * TW + 2 * w + c] = x[c][a];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int e = tid + 64 * NC * q, r = e / (2 * NC), cs = e % (2 * NC);
    psi[((size_t)r * 256 + j0) * 2 + cs] = T[r * TW + cs];
  }
}

// ---------------------------------------------------------------- 1D persistent SPO
// SPO.run structure (wpd.py:250-270): V/2 ; for i in 1..nt//nout-1: nout x [K, V], snapshot ;
// then K, V/2.  One workgroup per wavepacket, all steps in LDS.
template <int L>
__global__ __launch_bounds__(256) void spo1d_kernel(c128* psi, const c128* expV, const c128* expVh, const c128* expK,
                                                    const c128* twg, int nt, int nout, c128* snap) {
  __shared__ c128 tw[L], A[L], Bf[L], eV[L], eK[L];
  const int b = blockIdx.x;
  c128* p = psi + (size_t)b * L;
  for (int k = threadIdx.x; k < L; k += blockDim.x) {
    tw[k] = twg[k];
    eV[k] = expV[k];
    eK[k] = cscale(expK[k], 1.0 / L);
    A[k] = cmul(expVh[k], p[k]);
  }
  __syncthreads();
  const int T = L / 4;
  const int t = threadIdx.x;
  const bool active = t < T;
  c128* cur = A;
  c128* oth = Bf;
  const int nblk = nt / nout;
  const int nsnap = nblk > 0 ? nblk - 1 : 0;
  auto kstep = [&]() {
    c128* r = fft_lds<L, false>(cur, oth, tw, t, active);
    if (r != cur) { oth = cur; cur = r; }
    for (int k = threadIdx.x; k < L; k += blockDim.x) cur[k] = cmul(cur[k], eK[k]);
    __syncthreads();
    r = fft_lds<L, true>(cur, oth, tw, t, active);
    if (r != cur) { oth = cur; cur = r; }
  };
  for (int blk = 1; blk < nblk; ++blk) {
    for (int s = 0; s < nout; ++s) {
      kstep();
      for (int k = threadIdx.x; k < L; k += blockDim.x) cur[k] = cmul(eV[k], cur[k]);
      __syncthreads();
    }
    if (snap)
      for (int k = threadIdx.x; k < L; k += blockDim.x) snap[((size_t)b * nsnap + (blk - 1)) * L + k] = cur[k];
  }
  kstep();
  for (int k = threadIdx.x; k < L; k += blockDim.x) p[k] = cmul(expVh[k], cur[k]);
}

// ---------------------------------------------------------------- point propagators (SPO build)
// exp(-i V tau) per grid point for tau = dt and dt/2 (wpd.py:585-623: eigh -> U e^{-i w tau} U^+).
// LAPACK's eigh reads the lower triangle and ignores Im of the diagonal; so does this: a = Re V00,
// d = Re V11, b = conj(V10).  For ns = 2 the exponential is closed form,
//   exp(-i H tau) = e^{-i m tau} [cos(r tau) I - i (sin(r tau)/r) (H - m I)],
//   m = (a + d)/2, delta = (a - d)/2, r = sqrt(delta^2 + |b|^2)   (sin(r tau)/r -> tau at r = 0),
// identical to the eigen form in exact arithmetic and independent of the eigenvector phases.
__device__ __forceinline__ void expv2(double a, double d, c128 b, double tau, c128* E) {
  const double m = 0.5 * (a + d), de = 0.5 * (a - d);
  const double r = sqrt(de * de + b.re * b.re + b.im * b.im);
  double sn, cs, ph_s, ph_c;
  sincos(r * tau, &sn, &cs);
  const double sr = r > 0.0 ? sn / r : tau;
  sincos(-m * tau, &ph_s, &ph_c);
  const c128 ph = cmk(ph_c, ph_s);
  E[0] = cmul(ph, cmk(cs, -sr * de));                 // c - i s delta
  E[3] = cmul(ph, cmk(cs, sr * de));                  // c + i s delta
  E[1] = cmul(ph, cmulmi(cscale(b, sr)));             // -i s b
  E[2] = cmul(ph, cmulmi(cscale(cconj(b), sr)));      // -i s b*
}

template <bool CPLX>
__global__ void spo_expv_kernel(const void* v_, long npts, int ns, double dt, c128* expV, c128* expVh) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < npts; e += (long)gridDim.x * blockDim.x) {
    if (ns == 1) {
      const double a = CPLX ? ((const c128*)v_)[e].re : ((const double*)v_)[e];
      double sn, cs;
      sincos(-a * dt, &sn, &cs);
      if (expV) expV[e] = cmk(cs, sn);
      sincos(-a * 0.5 * dt, &sn, &cs);
      expVh[e] = cmk(cs, sn);
      continue;
    }
    double a, d;
    c128 b;
    if (CPLX) {
      const c128* v = (const c128*)v_ + e * 4;
      a = v[0].re;
      d = v[3].re;
      b = cconj(v[2]);
    } else {
      const double* v = (const double*)v_ + e * 4;
      a = v[0];
      d = v[3];
      b = cmk(v[2], 0.0);
    }
    c128 E[4];
    if (expV) {
      expv2(a, d, b, dt, E);
#pragma unroll
      for (int q = 0; q < 4; ++q) expV[e * 4 + q] = E[q];
    }
    expv2(a, d, b, 0.5 * dt, E);
#pragma unroll
    for (int q = 0; q < 4; ++q) expVh[e * 4 + q] = E[q];
  }
}

}  // namespace
}  // namespace qd
