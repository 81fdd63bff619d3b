// spo_gen_kernels.hpp — the device code of the any-size engine (spo_gen.hip): the fused LDS pass over one axis
// (spo_axis_kernel), the unfused kernels of the passes that do not fit the LDS (direct DFT, point operator, k-space
// multiplies, four-step twiddles), the plan tables, and the persistent 1D run (spo1d_gen_kernel).
#pragma once

#include "fft_lds.hpp"

namespace qd {
namespace spog {

// ---------------------------------------------------------------- fused axis pass
#ifdef QD_PHASE_TIMING
// diagnostics build: per-pass phase wall clock summed over blocks (thread 0's view after each barrier)
// [0] load, [1] inverse FFT, [2] point ops / snapshot / k_y, [3] forward FFT / kinetic step, [4] store, [5] blocks
__device__ unsigned long long g_spo_tim[2][6];
#define SPO_MARK(k)                                   \
  if (threadIdx.x == 0) {                             \
    const unsigned long long now_ = wall_clock64();   \
    atomicAdd(&g_spo_tim[a.flags & F_KMUL ? 1 : 0][k], now_ - tl_); \
    tl_ = now_;                                       \
  }
#else
#define SPO_MARK(k)
#endif
__global__ __launch_bounds__(256) void spo_axis_kernel(Fft p, AxisArgs a) {
  extern __shared__ c128 sm[];
#ifdef QD_PHASE_TIMING
  unsigned long long tl_ = wall_clock64();
  if (threadIdx.x == 0) atomicAdd(&g_spo_tim[a.flags & F_KMUL ? 1 : 0][5], 1ull);
#endif
  const int M = p.M, L = a.L, C = a.C, G = a.G, I = a.I;
  const int nl = G * C;
  c128* cur = sm;
  c128* oth = sm + (size_t)nl * M;
  // twiddles: staged in LDS behind the two line buffers when the host reserved room (a.twl), else read from HBM/L2
  const c128* tw = p.tw;
  if (a.twl) {
    c128* stw = oth + (size_t)nl * M;
    for (int m = threadIdx.x; m < M; m += blockDim.x) stw[m] = p.tw[m];
    tw = stw;
  }
  const int o0 = blockIdx.x * G, i0 = blockIdx.y * C;
  const int gv = min(G, a.O - o0), cv = min(C, I - i0);
  const int tot = G * L * C;
  const int ns = a.ns;
  const int pts = I / ns;
  for (int f = threadIdx.x; f < tot; f += blockDim.x) {
    const int g = (int)fdiv((unsigned)f, a.dLC), r = f - g * (L * C), e = (int)fdiv((unsigned)r, a.dC), c = r - e * C;
    cur[(g * C + c) * M + e] =
        (g < gv && c < cv) ? a.psi[((size_t)(o0 + g) * L + e) * I + i0 + c] : cmk(0.0, 0.0);
  }
  __syncthreads();
  SPO_MARK(0)
  if (a.flags & F_INV) lds_fft<true>(p, tw, cur, oth, nl);
  SPO_MARK(1)
  auto point_op = [&](const c128* U) {   // C == I == ns: line g * ns + s holds state s of row g
    const int n = G * L * ns;
    const int row0 = o0;
    for (int f = threadIdx.x; f < n; f += blockDim.x) {
      const int g = (int)fdiv((unsigned)f, a.dLns), r = f - g * (L * ns), e = (int)fdiv((unsigned)r, a.dns),
                s = r - e * ns;
      if (g >= gv) continue;
      const c128* u = U + (((size_t)(row0 + g) * L + e) * ns + s) * ns;
      c128 acc = cmk(0.0, 0.0);
      for (int b = 0; b < ns; ++b) acc = cadd(acc, cmul(u[b], cur[(g * ns + b) * M + e]));
      oth[(g * ns + s) * M + e] = acc;
    }
    __syncthreads();
    c128* t = cur;
    cur = oth;
    oth = t;
  };
  if (a.flags & F_PT1) point_op(a.U1);
  if (a.flags & F_SNAP) {
    for (int f = threadIdx.x; f < tot; f += blockDim.x) {
      const int g = (int)fdiv((unsigned)f, a.dLC), r = f - g * (L * C), e = (int)fdiv((unsigned)r, a.dC), c = r - e * C;
      if (g < gv && c < cv) a.snap[((size_t)(o0 + g) * L + e) * I + i0 + c] = cur[(g * C + c) * M + e];
    }
  }
  if (a.flags & F_PT2) point_op(a.U2);
  SPO_MARK(2)
  if (a.flags & F_FWD) lds_fft<false>(p, tw, cur, oth, nl);
  if (a.flags & F_KY) {
    for (int f = threadIdx.x; f < tot; f += blockDim.x) {
      const int g = (int)fdiv((unsigned)f, a.dLC), r = f - g * (L * C), e = (int)fdiv((unsigned)r, a.dC), c = r - e * C;
      if (g < gv) cur[(g * C + c) * M + e] = cmul(a.Ky[(size_t)(o0 + g) * L + e], cur[(g * C + c) * M + e]);
    }
    __syncthreads();
  }
  if (a.flags & F_KMUL) {   // outermost axis (O == 1): FFT -> * exp_K / N -> IFFT
    lds_fft<false>(p, tw, cur, oth, nl);
    for (int f = threadIdx.x; f < tot; f += blockDim.x) {
      const int r = f - (int)fdiv((unsigned)f, a.dLC) * (L * C), e = (int)fdiv((unsigned)r, a.dC), c = r - e * C;
        if (a.flags & F_KROW) {
        const int g = (int)fdiv((unsigned)f, a.dLC);
        if (g < gv) cur[(g * C + c) * M + e] = cmul(cur[(g * C + c) * M + e], a.K[(size_t)(o0 + g) * L + e]);
      } else if (c < cv) {
        cur[c * M + e] = cmul(cur[c * M + e], a.K[(size_t)e * pts + (int)fdiv((unsigned)(i0 + c), a.dns)]);
      }
    }
    __syncthreads();
    lds_fft<true>(p, tw, cur, oth, nl);
  }
  SPO_MARK(3)
  for (int f = threadIdx.x; f < tot; f += blockDim.x) {
    const int g = (int)fdiv((unsigned)f, a.dLC), r = f - g * (L * C), e = (int)fdiv((unsigned)r, a.dC), c = r - e * C;
    if (g < gv && c < cv) {
      size_t o;
      if (a.flags & F_XOUT) {
        const unsigned og = (unsigned)(o0 + g), hi = fdiv(og, a.dlo), lo = og - hi * a.dlo.d;
        o = (size_t)hi * a.sh + (size_t)lo * a.sl + (size_t)e * a.se + i0 + c;
      } else {
        o = ((size_t)(o0 + g) * L + e) * I + i0 + c;
      }
      a.out[o] = cur[(g * C + c) * M + e];
    }
  }
#ifdef QD_PHASE_TIMING
  __syncthreads();
#endif
  SPO_MARK(4)
}

// ---------------------------------------------------------------- unfused kernels
// Direct DFT along one axis, out of place: dst[o][k][i] = sum_n src[o][n][i] w^(n k) (w = exp(-+2 pi i / L)).
// Block (x, y): outputs k in [256 x, 256 x + 256) of lines y, y + gridDim.y, ...; input staged 256 points at a
// time in LDS, per-output accumulators in LDS (flat loops: any blockDim).
template <bool INV>
__global__ __launch_bounds__(256) void dft_axis_kernel(const c128* __restrict__ src, c128* __restrict__ dst, long O,
                                                       int L, long I, const c128* __restrict__ tw) {
  __shared__ c128 xs[256];
  __shared__ c128 acc[256];
  const long nlines = O * I;
  const int k0 = blockIdx.x * 256;
  const int nk = min(256, L - k0);
  for (long line = blockIdx.y; line < nlines; line += gridDim.y) {
    const long o = line / I, i = line - o * I;
    const c128* s = src + (size_t)o * L * I + i;
    for (int t = threadIdx.x; t < 256; t += blockDim.x) acc[t] = cmk(0.0, 0.0);
    for (int n0 = 0; n0 < L; n0 += 256) {
      const int cnt = min(256, L - n0);
      __syncthreads();
      for (int t = threadIdx.x; t < cnt; t += blockDim.x) xs[t] = s[(size_t)(n0 + t) * I];
      __syncthreads();
      for (int kk = threadIdx.x; kk < nk; kk += blockDim.x) {
        const long k = k0 + kk;
        long e = ((long)n0 * k) % L;
        c128 a = acc[kk];
        for (int t = 0; t < cnt; ++t) {
          c128 w = tw[e];
          if (INV) w = cconj(w);
          a = cadd(a, cmul(xs[t], w));
          e += k;
          if (e >= L) e -= L;
        }
        acc[kk] = a;
      }
    }
    __syncthreads();
    for (int kk = threadIdx.x; kk < nk; kk += blockDim.x) dst[(size_t)o * L * I + (size_t)(k0 + kk) * I + i] = acc[kk];
    __syncthreads();
  }
}

// dst[p][s] = sum_b U[p][s][b] src[p][b], one thread per (point, state), any ns
__global__ void pointop_kernel(const c128* __restrict__ src, c128* __restrict__ dst, const c128* __restrict__ U,
                               long npts, int ns) {
  const long n = npts * ns;
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    const long pt = f / ns;
    const c128* u = U + (size_t)f * ns;
    const c128* x = src + (size_t)pt * ns;
    c128 acc = cmk(0.0, 0.0);
    for (int b = 0; b < ns; ++b) acc = cadd(acc, cmul(u[b], x[b]));
    dst[f] = acc;
  }
}

// psi[p][s] *= K[p]: one factor per point for all its states (exp_K / N on the whole grid, and the Jacobi k_y phase
// per (row, k_y))
__global__ void kmul_kernel(c128* psi, const c128* __restrict__ K, long n, int ns) {
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x)
    psi[f] = cmul(psi[f], K[f / ns]);
}

// dst[j][i] = s src[i][j] (src [r][c]): the kinetic table of the xpose passes
__global__ void scale_transpose_kernel(const c128* __restrict__ src, c128* __restrict__ dst, int r, int c, double s) {
  const long n = (long)r * c;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const int i = (int)(e / c), j = (int)(e % c);
    dst[(size_t)j * r + i] = cscale(src[e], s);
  }
}
__global__ void scale_copy_kernel(const c128* __restrict__ src, c128* __restrict__ dst, long n, double s) {
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x)
    dst[f] = cscale(src[f], s);
}

// psi[f] *= K[f % L] (one factor per line position, every line of the batch)
__global__ void bcast_mul_kernel(c128* psi, const c128* __restrict__ K, long n, int L) {
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x)
    psi[f] = cmul(psi[f], K[f % L]);
}

// Four-step twiddle of a line viewed as [L1][L2]: element (k1, n2) *= w_L^(+-n2 k1) (index (n2 k1) mod L exact)
__global__ void fourstep_twiddle_kernel(c128* psi, long n, int L1, int L2, const c128* __restrict__ twL, int inv) {
  const long L = (long)L1 * L2;
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    const long r = f % L;
    const long k1 = r / L2, n2 = r - k1 * L2;
    c128 w = twL[(n2 * k1) % L];
    if (inv) w = cconj(w);
    psi[f] = cmul(psi[f], w);
  }
}

// exp_K in the four-step's k order: Kp[k1 L2 + k2] = scale * K[k1 + L1 k2]
__global__ void fourstep_kperm_kernel(const c128* __restrict__ K, c128* Kp, int L1, int L2, double scale) {
  const long L = (long)L1 * L2;
  for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < L; r += (long)gridDim.x * blockDim.x) {
    const long k1 = r / L2, k2 = r - k1 * L2;
    Kp[r] = cscale(K[k1 + (long)L1 * k2], scale);
  }
}

// Four-step twiddle of lines viewed as [L1][L2] inside a [O][L][I] grid: element (o, k1, n2, i) *= w_L^(+-n2 k1)
__global__ void fourstep_twiddle_inner_kernel(c128* psi, long n, int L1, int L2, long I, const c128* __restrict__ twL,
                                              int inv) {
  const long L = (long)L1 * L2;
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    const long r = (f / I) % L;
    const long k1 = r / L2, n2 = r - k1 * L2;
    c128 w = twL[(n2 * k1) % L];
    if (inv) w = cconj(w);
    psi[f] = cmul(psi[f], w);
  }
}

// ---------------------------------------------------------------- plan tables
__global__ void twiddle_table_kernel(int M, c128* tw) {
  for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) {
    double s, c;
    sincospi(-2.0 * (double)m / (double)M, &s, &c);
    tw[m] = cmk(c, s);
  }
}

// c_n = exp(-pi i n^2 / L) with n^2 mod 2L exact; b_m = conj(c_|m|) wrapped into M slots
__global__ void chirp_kernel(int L, int M, c128* chirp, c128* b) {
  for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < M; m += gridDim.x * blockDim.x) {
    const int n = m < L ? m : (M - m < L ? M - m : -1);
    c128 v = cmk(0.0, 0.0);
    if (n >= 0) {
      const long q = ((long)n * n) % (2L * L);
      double s, c;
      sincospi(-(double)q / (double)L, &s, &c);
      if (m < L) chirp[m] = cmk(c, s);
      v = cmk(c, -s);
    }
    b[m] = v;
  }
}

// bhat[k] = (1/M) sum_m b[m] exp(-2 pi i m k / M) (direct, exact index (m k) mod M)
__global__ void bhat_kernel(int M, const c128* __restrict__ b, const c128* __restrict__ tw, c128* bhat) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < M; k += gridDim.x * blockDim.x) {
    c128 acc = cmk(0.0, 0.0);
    long e = 0;
    for (int m = 0; m < M; ++m) {
      acc = cadd(acc, cmul(b[m], tw[e]));
      e += k;
      if (e >= M) e -= M;
    }
    bhat[k] = cscale(acc, 1.0 / M);
  }
}

// ---------------------------------------------------------------- 1D persistent SPO
// SPO.run (wpd.py:250-270): V/2; for blk in 1..nt//nout-1: nout x [K, V], snapshot; K; V/2.
// One workgroup per wavepacket, the line resident in LDS for the whole run.
__global__ __launch_bounds__(256) void spo1d_gen_kernel(Fft p, c128* psi, const c128* eV, const c128* eVh,
                                                        const c128* eK, int nt, int nout, c128* snap, int twl) {
  extern __shared__ c128 sm[];
  const int L = p.L, M = p.M;
  c128* cur = sm;
  c128* oth = sm + M;
  const c128* tw = p.tw;
  if (twl) {
    c128* stw = sm + 2 * M;
    for (int m = threadIdx.x; m < M; m += blockDim.x) stw[m] = p.tw[m];
    tw = stw;
  }
  const int b = blockIdx.x;
  c128* x = psi + (size_t)b * L;
  const double inv = 1.0 / L;
  for (int k = threadIdx.x; k < L; k += blockDim.x) cur[k] = cmul(eVh[k], x[k]);
  __syncthreads();
  const int nblk = nt / nout;
  const int nsnap = nblk > 0 ? nblk - 1 : 0;
  auto kstep = [&]() {
    lds_fft<false>(p, tw, cur, oth, 1);
    for (int k = threadIdx.x; k < L; k += blockDim.x) cur[k] = cmul(cur[k], cscale(eK[k], inv));
    __syncthreads();
    lds_fft<true>(p, tw, cur, oth, 1);
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
  for (int k = threadIdx.x; k < L; k += blockDim.x) x[k] = cmul(eVh[k], cur[k]);
}

}  // namespace spog
}  // namespace qd
