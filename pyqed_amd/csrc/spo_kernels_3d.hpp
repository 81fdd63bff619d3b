// spo_kernels_3d.hpp — the passes only 3D grids take (spo.hip), psi [nx][ny][nz][ns]: the middle-axis (y) passes and
// the 64-point register passes along every axis, which also carry the separable propagator of spo3_sep64_run.
#pragma once

#include "spo_kernels.hpp"

namespace qd {
namespace {

// Middle-axis pass of a 3D grid psi [nx][ny][nz][ns] viewed as [outer][L][inner]
// (inner = nz*ns): each workgroup transforms C consecutive inner indices of one
// outer index i along the L axis (chunks of C*16 B per row: coalesced).
template <int L, int C, bool INV>
__global__ __launch_bounds__(256) void spo_mid_kernel(c128* psi, const c128* tw_g, int inner) {
  __shared__ c128 tw[L];
  __shared__ c128 A[C * L], Bf[C * L];  // layout [c][j]; LDS sized to the C transforms of this block
  const int chunks = inner / C;
  const int i = blockIdx.x / chunks, c0 = (blockIdx.x % chunks) * C;
  c128* base = psi + (size_t)i * L * inner + c0;
  for (int k = threadIdx.x; k < L; k += blockDim.x) tw[k] = tw_g[k];
  for (int e = threadIdx.x; e < L * C; e += blockDim.x) {
    const int c = e % C, j = e / C;
    A[c * L + j] = base[(size_t)j * inner + c];
  }
  __syncthreads();
  const int T = L / 4;
  const int f = threadIdx.x / T, t = threadIdx.x % T;
  const bool active = f < C;
  const int fo = (active ? f : 0) * L;
  c128* r = fft_lds<L, INV>(A + fo, Bf + fo, tw, t, active);
  c128* cur = (r == A + fo) ? A : Bf;
  for (int e = threadIdx.x; e < L * C; e += blockDim.x) {
    const int c = e % C, j = e / C;
    base[(size_t)j * inner + c] = cur[c * L + j];
  }
}

// Latency-shaped middle-axis pass (same transforms and arithmetic as spo_mid_kernel): the block size is fixed at
// compile time (BD = C L / 4 threads, IT = 4 elements per thread), so every global load of the pass (the C
// columns of 16-B pieces and the twiddles) is issued before the first wait and every store after the transform:
// one load round trip + one store drain per pass instead of IT dependent load / LDS-store iterations.
template <int L, int C, bool INV>
__global__ __launch_bounds__(C * L / 4 < 64 ? 64 : C * L / 4) void spo_mid_fast_kernel(c128* psi, const c128* tw_g,
                                                                                       int inner) {
  constexpr int BD = C * L / 4 < 64 ? 64 : C * L / 4;
  constexpr int IT = (L * C + BD - 1) / BD;
  constexpr bool FULL = (L * C) % BD == 0;
  __shared__ c128 tw[L];
  __shared__ c128 A[C * L], Bf[C * L];  // layout [c][j]
  const int chunks = inner / C;
  const int i = blockIdx.x / chunks, c0 = (blockIdx.x % chunks) * C;
  c128* base = psi + (size_t)i * L * inner + c0;
  const int tid = threadIdx.x;
  c128 v[IT];
#pragma unroll
  for (int n = 0; n < IT; ++n) {
    const int e = tid + n * BD;  // c = e % C fastest: C * 16 B contiguous per row j
    v[n] = (FULL || e < L * C) ? base[(size_t)(e / C) * inner + e % C] : cmk(0, 0);
  }
  static_assert(L <= BD, "one twiddle per thread");
  const c128 twv = tid < L ? tw_g[tid] : cmk(0, 0);
  if (tid < L) tw[tid] = twv;
#pragma unroll
  for (int n = 0; n < IT; ++n) {
    const int e = tid + n * BD;
    if (FULL || e < L * C) A[(e % C) * L + e / C] = v[n];
  }
  __syncthreads();
  constexpr int T = L / 4;
  const int f = tid / T, t = tid % T;
  const bool active = f < C;
  const int fo = (active ? f : 0) * L;
  c128* r = fft_lds<L, INV>(A + fo, Bf + fo, tw, t, active);
  const c128* cur = (r == A + fo) ? A : Bf;
#pragma unroll
  for (int n = 0; n < IT; ++n) {
    const int e = tid + n * BD;
    if (FULL || e < L * C) base[(size_t)(e / C) * inner + e % C] = cur[(e % C) * L + e / C];
  }
}

// Middle-axis pass at L = 64 with the register transform (same tiles and loads as spo_mid_fast_kernel<64, C>):
// the C columns (C x 16 B per row) are staged in LDS, each 16-lane group transforms one column line in place
// (fft64_group, wave barriers only), and the tile is stored back.
// KD: the whole separable axis propagator F^-1 diag(d) F on each line (forward transform, * d[k], inverse; d holds
// e_y / ny), natural order in and out (qd_spo3_run_axes on power-of-two 64-point axes)
template <int C, bool INV, bool KD = false>
__global__ __launch_bounds__(16 * C) void spo_mid64_kernel(c128* psi, const c128* tw_g, int inner,
                                                           const c128* dk = nullptr) {
  constexpr int BD = 16 * C, LS = 65;  // line stride (padded)
  __shared__ c128 A[C * LS];
  __shared__ c128 tw[64];
  const int chunks = inner / C;
  const int i = blockIdx.x / chunks, c0 = (blockIdx.x % chunks) * C;
  c128* base = psi + (size_t)i * 64 * inner + c0;
  const int tid = threadIdx.x, g = tid >> 4, lane16 = tid & 15, qq = lane16 >> 2, s = lane16 & 3;
  c128 v[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + BD * n;
    v[n] = base[(size_t)(e / C) * inner + e % C];
  }
  if (tid < 64) tw[tid] = tw_g[tid];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + BD * n;
    A[(e % C) * LS + e / C] = v[n];
  }
  __syncthreads();
  const Q16Tw t = q64_twiddles(tw, qq, s);
  c128* line = A + g * LS;
  fft64_group<INV>(line, 1, t, qq, s, v);
  if constexpr (KD) {
#pragma unroll
    for (int k = 0; k < 4; ++k) line[lane16 + 16 * k] = cmul(v[k], dk[lane16 + 16 * k]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    fft64_group<true>(line, 1, t, qq, s, v);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) line[lane16 + 16 * k] = v[k];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + BD * n;
    base[(size_t)(e / C) * inner + e % C] = A[(e % C) * LS + e / C];
  }
}

// Column (x) pass at L = nx = 64 with the register transform (same tiles and loads as spo2_col_fast_kernel<64, C,
// NS>): W = C NS lines (column-major over states) staged in LDS, each 16-lane group runs FFT_x -> * exp_K /
// (nx ny nz) -> IFFT_x on one line in registers (natural order between the transforms).
template <int C, int NS>
__global__ __launch_bounds__(16 * C * NS) void spo_col64_kernel(c128* psi, const c128* expKT, const c128* tw_g,
                                                                int ny, int kstride = 64) {
  constexpr int W = C * NS, BD = 16 * W, LS = 65;
  __shared__ c128 A[W * LS];
  __shared__ c128 tw[64];
  const int j0 = blockIdx.x * C;
  const int tid = threadIdx.x, g = tid >> 4, lane16 = tid & 15, qq = lane16 >> 2, s = lane16 & 3;
  c128 v[4], kf[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + BD * n;   // row i = e / W, line w = e % W (coalesced W x 16 B per row)
    v[n] = psi[((size_t)(e / W) * ny + j0) * NS + e % W];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) kf[k] = expKT[(size_t)(j0 + g / NS) * kstride + lane16 + 16 * k];   // 0: one factor
  if (tid < 64) tw[tid] = tw_g[tid];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + BD * n;
    A[(e % W) * LS + e / W] = v[n];
  }
  __syncthreads();
  const Q16Tw t = q64_twiddles(tw, qq, s);
  c128* line = A + g * LS;
  fft64_group<false>(line, 1, t, qq, s, v);
#pragma unroll
  for (int k = 0; k < 4; ++k) line[lane16 + 16 * k] = cmul(v[k], kf[k]);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  fft64_group<true>(line, 1, t, qq, s, v);
#pragma unroll
  for (int k = 0; k < 4; ++k) line[lane16 + 16 * k] = v[k];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int e = tid + BD * n;
    psi[((size_t)(e / W) * ny + j0) * NS + e % W] = A[(e % W) * LS + e / W];
  }
}

// Row pass along a 64-point contiguous axis (SPO3's z lines, psi [rows][64][NS]) with the register transform:
// one 16-lane group per row holding every state of its points, so the point operators are lane-local; 16 rows
// per 256-thread workgroup, each with NS x 64 entries of LDS exchange space.  The row's values come straight
// from global memory in the transform's input layout (lane l = 4 qq + s: points 16 a + 4 s + qq, NS x 16 B
// contiguous per point) and leave in natural order (points l + 16 k).  Same flags as spo2_row_kernel:
// [IFFT] -> V/2 -> [snapshot] -> [V/2] -> [FFT].
template <int NS>
__global__ __launch_bounds__(256) void spo_row64_kernel(c128* psi, const c128* U, const c128* tw_g, int flags,
                                                        c128* snap, const c128* dz = nullptr) {
  __shared__ c128 E[16 * NS * 64];      // per row: [state][64]
  __shared__ c128 tw[64];
  const int tid = threadIdx.x, grp = tid >> 4, lane16 = tid & 15, qq = lane16 >> 2, s = lane16 & 3;
  const size_t row = (size_t)blockIdx.x * 16 + grp;
  c128* pr = psi + row * 64 * NS;
  c128* ex = E + grp * NS * 64;
  c128 x[NS][4];
  const bool inv = flags & ROW_INV;
  // input layout: points 16 a + 4 s + qq (transform input) when the pass starts with the IFFT, else natural
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int p = inv ? 16 * a + 4 * s + qq : lane16 + 16 * a;
#pragma unroll
    for (int c = 0; c < NS; ++c) x[c][a] = pr[p * NS + c];
  }
  if (tid < 64) tw[tid] = tw_g[tid];
  __syncthreads();
  const Q16Tw t = q64_twiddles(tw, qq, s);
  if (inv) {
#pragma unroll
    for (int c = 0; c < NS; ++c) fft64_regs<true>(ex + c * 64, 1, t, qq, s, x[c]);
  }
  // from here the lane holds the points lane16 + 16 k
  if (flags & (ROW_VH1 | ROW_VH2 | ROW_SNAP)) {
    c128 u[4][NS * NS];
    if (flags & (ROW_VH1 | ROW_VH2)) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < NS * NS; ++e) u[k][e] = U[((row * 64) + lane16 + 16 * k) * NS * NS + e];
    }
    auto point_op = [&]() {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        c128 q[NS];
#pragma unroll
        for (int a = 0; a < NS; ++a) {
          c128 acc = cmk(0, 0);
#pragma unroll
          for (int b = 0; b < NS; ++b) acc = cadd(acc, cmul(u[k][a * NS + b], x[b][k]));
          q[a] = acc;
        }
#pragma unroll
        for (int a = 0; a < NS; ++a) x[a][k] = q[a];
      }
    };
    if (flags & ROW_VH1) point_op();
    if (flags & ROW_SNAP) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < NS; ++c) snap[(row * 64 + lane16 + 16 * k) * NS + c] = x[c][k];
    }
    if (flags & ROW_VH2) point_op();
  }
  if (flags & ROW_FWD) {
    // natural -> transform input layout through the row's exchange space, then the forward transform
#pragma unroll
    for (int c = 0; c < NS; ++c) {
#pragma unroll
      for (int k = 0; k < 4; ++k) ex[c * 64 + lane16 + 16 * k] = x[c][k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int c = 0; c < NS; ++c) fft64_group<false>(ex + c * 64, 1, t, qq, s, x[c]);
    if (flags & ROW_KZ) {   // * e_z / nz, inverse transform: the separable z propagator, natural order out
#pragma unroll
      for (int c = 0; c < NS; ++c) {
#pragma unroll
        for (int k = 0; k < 4; ++k) ex[c * 64 + lane16 + 16 * k] = cmul(x[c][k], dz[lane16 + 16 * k]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
      for (int c = 0; c < NS; ++c) fft64_group<true>(ex + c * 64, 1, t, qq, s, x[c]);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < NS; ++c) pr[(lane16 + 16 * k) * NS + c] = x[c][k];
}

}  // namespace

// d[a][k] = fft(m_a)[k] / n (the axis factor e_a / n of a circulant axis propagator given by its first column)
__global__ void axis_factor_kernel(const c128* m0, const c128* m1, const c128* m2, int n, c128* d) {
  const c128* m = blockIdx.x == 0 ? m0 : blockIdx.x == 1 ? m1 : m2;
  const int k = threadIdx.x;
  if (k >= n) return;
  c128 acc = cmk(0.0, 0.0);
  for (int j = 0; j < n; ++j) {
    double sn, cs;
    sincospi(-2.0 * (double)((j * k) % n) / n, &sn, &cs);
    acc = cadd(acc, cmul(m[j], cmk(cs, sn)));
  }
  d[blockIdx.x * n + k] = cmk(acc.re / n, acc.im / n);
}
}  // namespace qd
