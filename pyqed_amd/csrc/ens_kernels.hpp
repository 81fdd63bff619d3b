// ens_kernels.hpp — device code of the 2DES ensemble on the (t3, t1) grid (response.hip): the operand builds of
//   S = X [n3 x K] * Z [K x n1]  (fixed t2)  and  S_j = P diag(E_j) Q  (t2 scan),
// the staging policies that feed them to the MFMA block engine, the split-K GEMMs and the slab reductions.  The sizes
// the kernels are written around (ZMAX, UNI_ROWS, XU_ROWS, UNI_MAXC, ENS_BT) live with the launch plan in
// response_plan.hpp.
#pragma once

#include "response_kernels.hpp"
#include "response_plan.hpp"

namespace qd {
namespace {

// ---------------------------------------------------------------- ensemble 2D slice
// One launch builds both GEMM operands (two bandwidth-bound writes of n x K c128 overlap):
//   blockIdx.y <  M : Z rows of member m (below)
//   blockIdx.y >= M : X [n3p][Kp], X[i][m*nL+p] = i * alpha_mp e^{lam_mp t3_i} (zero in the padding),
//                     grid-strided over the (blockIdx.y - M, blockIdx.x) blocks
// Z [Kp][n1p]: Z[m*nL+p][k] = sum_q Mt[m][p][q] y_q(k),  y_q(k) = beta[m][q] e^{lamz_mq t1_k}
// one thread per t1 point computes the nz exponentials once (registers, nz <= ZMAX) and emits the
// nL outputs of its column; Mt_m (nL x nz, rectangular when structurally zero alpha / beta columns
// were pruned on the host) staged in LDS.
__global__ __launch_bounds__(256) void ens_xz_kernel(const c128* Mt, const c128* beta, const c128* lam, int M, int nL,
                                                     const double* t1, int n1, int n1p, int Kp, c128* Z,
                                                     const c128* alpha, const double* t3, int n3, int n3p, int xrows,
                                                     int K, c128* X, int nz, const c128* lamz) {
  __shared__ c128 sM[ZMAX * ZMAX];
  if ((int)blockIdx.y >= M) {
    const size_t tot = (size_t)n3p * Kp;
    const size_t nthr = (size_t)xrows * gridDim.x * blockDim.x;
    for (size_t e = ((size_t)(blockIdx.y - M) * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x; e < tot;
         e += nthr) {
      const int kk = (int)(e % Kp), i = (int)(e / Kp);
      c128 v = cmk(0, 0);
      if (i < n3 && kk < K) v = cmuli(cmul(alpha[kk], cexp_t(lam[kk], t3[i])));
      X[e] = v;
    }
    return;
  }
  const int m = blockIdx.y;
  const int k = blockIdx.x * 256 + threadIdx.x;
  for (int e = threadIdx.x; e < nL * nz; e += 256) sM[e] = Mt[(size_t)m * nL * nz + e];
  __syncthreads();
  if (k >= n1p) return;
  c128 y[ZMAX];
  const double tk = k < n1 ? t1[k] : 0.0;
#pragma unroll
  for (int q = 0; q < ZMAX; ++q)
    y[q] = (q < nz && k < n1) ? cmul(beta[(size_t)m * nz + q], cexp_t(lamz[(size_t)m * nz + q], tk)) : cmk(0, 0);
  for (int p = 0; p < nL; ++p) {
    c128 v = cmk(0, 0);
#pragma unroll
    for (int q = 0; q < ZMAX; ++q)
      if (q < nz) v = cadd(v, cmul(sM[p * nz + q], y[q]));
    Z[((size_t)m * nL + p) * n1p + k] = v;
  }
}

// ---- uniform time grids (t = t0 + j dt): exponentials from two-level tables,
// e^{lam (t0 + (16 l + j) dt)} = e^{lam (t0 + 16 l dt)} * e^{lam j dt}; the coarse factor is a direct
// exponential, the fine table a product chain of e^{lam dt} (<= 15 products).  A handful of
// transcendentals per 16-64 outputs instead of one per output; relative error ~1e-14.
__device__ __forceinline__ void ens_x_uniform_block(int bx, int by, const c128* alpha, const c128* lam, int K, int Kp,
                                                    double t0, double dt, int n3, int n3p, c128* X) {
  const int kk = bx * 256 + threadIdx.x;
  const int i0 = by * XU_ROWS;
  if (kk >= Kp) return;
  const bool col = kk < K;
  const c128 l = col ? lam[kk] : cmk(0, 0);
  const c128 a = col ? cmuli(alpha[kk]) : cmk(0, 0);
  c128 T1[16];
  T1[0] = cmk(1, 0);
  const c128 st = cexp_t(l, dt);
#pragma unroll
  for (int j = 1; j < 16; ++j) T1[j] = cmul(T1[j - 1], st);
  for (int g = 0; g < XU_ROWS / 16; ++g) {
    const int ib = i0 + 16 * g;
    const c128 base = cmul(a, cexp_t(l, t0 + (double)ib * dt));
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int i = ib + j;
      if (i >= n3p) break;
      X[(size_t)i * Kp + kk] = (col && i < n3) ? cmul(base, T1[j]) : cmk(0, 0);
    }
  }
}

// Materialised uniform X in a launch of its own: block blockIdx.x of the (Kp/256) x (n3p/XU_ROWS) tiling.  The block
// index runs along x, whose extent is not bound by the 65,535 of a grid's y.
__global__ __launch_bounds__(256) void ens_x_uniform_kernel(const c128* alpha, const c128* lam, int K, int Kp,
                                                            double t3_0, double dt3, int n3, int n3p, int xbx,
                                                            c128* X) {
  ens_x_uniform_block(blockIdx.x % xbx, blockIdx.x / xbx, alpha, lam, K, Kp, t3_0, dt3, n3, n3p, X);
}

// Z rows of G members per block (uniform t1), tables in dynamic LDS: per member Mt_m (nL x nz), the fine
// table e^{lamz_q j dt} (nz x 16) and the coarse one beta_q e^{lamz_q (t0 + 16 l dt)} (nz x nC).  Every
// wave takes part in the table phase (G nz (16 + nC) exponentials per block instead of nz (16 + nC) per
// 256-thread block), and a block then streams G nL full Z rows.  Blocks blockIdx.y >= ceil(M / G) build
// X blocks instead (materialised uniform X, when the A operand is not generated in the GEMM).
__global__ __launch_bounds__(256) void ens_z_uniform_kernel(const c128* Mt, const c128* beta, const c128* lamz, int M,
                                                            int nL, int nz, int G, double t0, double dt, int n1,
                                                            int n1p, c128* Z, const c128* alpha, const c128* lamx,
                                                            int K, int Kp, double t3_0, double dt3, int n3, int n3p,
                                                            int xbx, c128* X) {
  extern __shared__ c128 zs[];
  const int nMB = (M + G - 1) / G;
  if ((int)blockIdx.y >= nMB) {
    if (blockIdx.x != 0) return;
    const int xb = blockIdx.y - nMB;
    ens_x_uniform_block(xb % xbx, xb / xbx, alpha, lamx, K, Kp, t3_0, dt3, n3, n3p, X);
    return;
  }
  const int nC = n1p / 16;
  const int per = nL * nz + nz * (16 + nC);
  const int m0 = blockIdx.y * G;
  const int g = min(G, M - m0);
  // round 1: every input of the block's members (Mt, lamz, beta) in one parallel load round into LDS
  c128* sLam = zs + G * per;
  c128* sBeta = sLam + G * nz;
  for (int e = threadIdx.x; e < g * nL * nz; e += 256)
    zs[(e / (nL * nz)) * per + e % (nL * nz)] = Mt[(size_t)m0 * nL * nz + e];
  for (int e = threadIdx.x; e < g * nz; e += 256) {
    sLam[e] = lamz[(size_t)m0 * nz + e];
    sBeta[e] = beta[(size_t)m0 * nz + e];
  }
  __syncthreads();
  // round 2: the exponential tables from LDS operands (no global latency inside the loop)
  // one thread per (member, q): fine[j] = e^{lam j dt} as powers of e^{lam dt}, coarse[l] = beta e^{lam t0} times
  // powers of e^{16 lam dt} (3 exponentials instead of 16 + nC; relative error ~1e-14)
  for (int e = threadIdx.x; e < g * nz; e += 256) {
    const int gi = e / nz, q = e - gi * nz;
    const c128 l = sLam[gi * nz + q];
    c128* fine = zs + gi * per + nL * nz + q * 16;
    c128* coarse = zs + gi * per + nL * nz + nz * 16 + q * nC;
    const c128 e1 = cexp_t(l, dt);
    c128 f = cmk(1.0, 0.0);
    fine[0] = f;
    for (int j = 1; j < 16; ++j) {
      f = cmul(f, e1);
      fine[j] = f;
    }
    const c128 e16 = cexp_t(l, 16.0 * dt);
    c128 c = cmul(sBeta[gi * nz + q], cexp_t(l, t0));
    for (int u = 0; u < nC; ++u) {
      coarse[u] = c;
      c = cmul(c, e16);
    }
  }
  __syncthreads();
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n1p) return;
  for (int gi = 0; gi < g; ++gi) {
    const c128* sM = zs + gi * per;
    const c128* sF = sM + nL * nz;
    const c128* sC = sF + nz * 16;
    c128 y[ZMAX];
#pragma unroll
    for (int q = 0; q < ZMAX; ++q)
      y[q] = (q < nz && k < n1) ? cmul(sC[q * nC + (k >> 4)], sF[q * 16 + (k & 15)]) : cmk(0, 0);
    for (int p = 0; p < nL; ++p) {
      c128 v = cmk(0, 0);
#pragma unroll
      for (int q = 0; q < ZMAX; ++q)
        if (q < nz) v = cadd(v, cmul(sM[p * nz + q], y[q]));
      Z[((size_t)(m0 + gi) * nL + p) * n1p + k] = v;
    }
  }
}

// rows K..Kp-1 of Z are padding
__global__ void ens_z_pad_kernel(int K, int Kp, int n1p, c128* Z) {
  const size_t tot = (size_t)(Kp - K) * n1p;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x)
    Z[(size_t)K * n1p + e] = cmk(0, 0);
}

// Generic fallback for nL > ZMAX (one thread per output element).
__global__ void ens_z_generic_kernel(const c128* Mt, const c128* beta, const c128* lam, int M, int nL,
                                     const double* t1, int n1, int n1p, int Kp, c128* Z, int nz) {
  const size_t tot = (size_t)Kp * n1p;
  const int K = M * nL;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % n1p), row = (int)(e / n1p);
    c128 v = cmk(0, 0);
    if (row < K && k < n1) {
      const int m = row / nL, p = row % nL;
      const c128* Mr = Mt + ((size_t)m * nL + p) * nz;
      for (int q = 0; q < nz; ++q)
        v = cadd(v, cmul(Mr[q], cmul(beta[(size_t)m * nz + q], cexp_t(lam[(size_t)m * nz + q], t1[k]))));
    }
    Z[e] = v;
  }
}

// Uniform t3 without materialising X: X[i][kk] = coarse[i >> 4][kk] * fine[i & 15][kk] with
//   coarse[c][kk] = i alpha_kk e^{lam_kk (t0 + 16 c dt)},  fine[j][kk] = (e^{lam_kk dt})^j (product chain),
// the same factors (and roundings) ens_x_uniform_block multiplies, formed by the GEMM's A staging instead
// (tables: (n3p/16 + 16) x Kp, 1/8 of X at n3p = 256).  Columns kk >= K are zero; rows past n3 inside the
// last 16-row group are finite and only reach output rows the reduction never reads.
__global__ __launch_bounds__(256) void ens_xtab_kernel(const c128* alpha, const c128* lam, int K, int Kp, double t0,
                                                       double dt, int n3, int n3p, c128* coarse, c128* fine) {
  const int kk = blockIdx.x * 256 + threadIdx.x;
  if (kk >= Kp) return;
  const bool col = kk < K;
  const c128 l = col ? lam[kk] : cmk(0, 0);
  const c128 a = col ? cmuli(alpha[kk]) : cmk(0, 0);
  const c128 st = cexp_t(l, dt);
  c128 f = cmk(1, 0);
  for (int j = 0; j < 16; ++j) {
    fine[(size_t)j * Kp + kk] = f;
    f = cmul(f, st);
  }
  for (int c = 0; c < n3p / 16; ++c)
    coarse[(size_t)c * Kp + kk] = (col && 16 * c < n3) ? cmul(a, cexp_t(l, t0 + (double)(16 * c) * dt)) : cmk(0, 0);
}

#ifndef ENS_PIPE
#define ENS_PIPE false  // fragment double-buffering (PIPE) fits (250 VGPRs, no scratch) but measured neutral here
#endif

// A operand X [n3p][Kp] (materialised by ens_xz_kernel), streamed one tile ahead.
struct EnsXA {
  using Raw = cg_v2;
  const c128* X;
  int Kp, row0, k0;
  __device__ __forceinline__ Raw fetch(int t, int e, int) const {
    return cg_ld(X + (size_t)(row0 + (e >> 4)) * Kp + k0 + t * CG_KT + (e & 15));
  }
  __device__ __forceinline__ cg_v2 finish(const Raw& r, int, int, int) const { return r; }
};

struct EnsXTab {
  struct Raw {
    cg_v2 c, f;
  };
  const c128* coarse;
  const c128* fine;
  int Kp, row0, k0;
  __device__ __forceinline__ Raw fetch(int t, int e, int) const {
    const int row = row0 + (e >> 4);
    const size_t kk = (size_t)k0 + t * CG_KT + (e & 15);
    return Raw{cg_ld(coarse + (size_t)(row >> 4) * Kp + kk), cg_ld(fine + (size_t)(row & 15) * Kp + kk)};
  }
  __device__ __forceinline__ cg_v2 finish(const Raw& r, int, int, int) const {
    const c128 v = cmul(cmk(r.c.x, r.c.y), cmk(r.f.x, r.f.y));
    return cg_v2{v.re, v.im};
  }
};

template <int BT = ENS_BT>
struct EnsZB {
  using Raw = cg_v2;
  const c128* Z;
  int n1p, col0, k0;
  __device__ __forceinline__ Raw fetch(int t, int e, int) const {
    return cg_ld(Z + (size_t)(k0 + t * CG_KT + e / BT) * n1p + col0 + (e % BT));
  }
  __device__ __forceinline__ cg_v2 finish(const Raw& r, int, int, int) const { return r; }
};

// XCD-aware tile order for the split-K GEMMs (speed only: any placement computes the same tiles).
// Workgroups are dealt round-robin over the 8 XCDs, so linear id L runs on XCD L % 8.  Tile u (column
// block fastest, then row block, then K split) is given to L with u = (L % 8) * (T / 8) + L / 8: each
// XCD owns a contiguous run of tiles, i.e. whole rows of column blocks that share one A (P / X) K-range
// and neighbouring row blocks that share B (Q / Z) tiles, in its own L2.  Identity when T % 8 != 0.
__device__ __forceinline__ void ens_tile(int& bn, int& bm, int& s) {
  const int NX = gridDim.x, NY = gridDim.y, T = NX * NY * gridDim.z;
  const int L = blockIdx.x + NX * (blockIdx.y + NY * blockIdx.z);
  const int u = (T % 8 == 0) ? (L % 8) * (T / 8) + L / 8 : L;
  bn = u % NX;
  bm = (u / NX) % NY;
  s = u / (NX * NY);
}

// grid: (n1p/BT) x (n3p/BT) x S ; each workgroup accumulates K-tiles [t0, t1) of its block.  BT = 64 for
// problems whose 128-blocks cannot fill the chip with >= 4 K-tiles per workgroup (4x the blocks, 1/4 the
// split-K slabs to write and reduce).
template <int BT, bool XTAB, int DEPTH = 1>
__global__ __launch_bounds__(CG_WG) void ens_gemm_kernel(const c128* X, int Kp, const c128* Z, int n1p, int tiles,
                                                         int S, c128* slabs, int n3p, const c128* fine) {
  __shared__ CgLds<BT> L;
  int bn, bm, s;
  ens_tile(bn, bm, s);
  const int t0 = (int)((long)tiles * s / S), t1 = (int)((long)tiles * (s + 1) / S);
  CgAcc<BT> A;
  c128* slab = slabs + (size_t)s * n3p * n1p;
  if (t1 > t0) {
    EnsZB<BT> pb{Z, n1p, bn * BT, t0 * CG_KT};
    if constexpr (XTAB) {
      EnsXTab pa{X, fine, Kp, bm * BT, t0 * CG_KT};  // X = the coarse table
      cg_block_gemm_gen<BT, ENS_PIPE>(t1 - t0, pa, pb, L, A);
    } else {
      EnsXA pa{X, Kp, bm * BT, t0 * CG_KT};
      if constexpr (DEPTH == 2)   // fragment double-buffering for the 64-blocks (shard: 0.1630 vs 0.1653 ms per grid;
                                  // the 128-blocks slow down with it, 1.53 vs 1.19 ms: profiles/r06/2des/knobs_ab.txt)
        cg_block_gemm_gen2<BT, ENS_PIPE || BT == 64>(t1 - t0, pa, pb, L, A);
      else
        cg_block_gemm_gen<BT, ENS_PIPE>(t1 - t0, pa, pb, L, A);
    }
    cg_epilogue<BT>(A, [&](int row, int col, c128 v) {
      slab[(size_t)(bm * BT + row) * n1p + bn * BT + col] = v;
    });
  } else {
    for (int e = threadIdx.x; e < BT * BT; e += CG_WG)
      slab[(size_t)(bm * BT + e / BT) * n1p + bn * BT + e % BT] = cmk(0, 0);
  }
}

// out[i][k] (+)= sum_s slab[s][i][k], fixed order -> deterministic
__global__ void ens_reduce_kernel(const c128* slabs, int S, int n3, int n1, int n3p, int n1p, c128* out,
                                  int accumulate) {
  const size_t tot = (size_t)n3 * n1;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / n1), k = (int)(e % n1);
    c128 v = accumulate ? out[e] : cmk(0, 0);
    v = slab_sum(v, 0, S, [&](int s) { return slabs[((size_t)s * n3p + i) * n1p + k]; });
    out[e] = v;
  }
}

// out[k][i] (+)= sum_s slab[s][i][k] (out is n1 x n3): 16 x 16 tiles through LDS, coalesced on both sides
__global__ __launch_bounds__(256) void ens_reduce_trans_kernel(const c128* slabs, int S, int n3, int n1, int n3p,
                                                               int n1p, c128* out, int accumulate) {
  __shared__ c128 tile[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int k0 = blockIdx.x * 16, i0 = blockIdx.y * 16;
  {
    const int i = i0 + ty, k = k0 + tx;
    c128 v = cmk(0, 0);
    if (i < n3 && k < n1) v = slab_sum(v, 0, S, [&](int s) { return slabs[((size_t)s * n3p + i) * n1p + k]; });
    tile[ty][tx] = v;
  }
  __syncthreads();
  const int k = k0 + ty, i = i0 + tx;
  if (i < n3 && k < n1) {
    const size_t e = (size_t)k * n3 + i;
    const c128 v = tile[tx][ty];
    out[e] = accumulate ? cadd(out[e], v) : v;
  }
}

// out[j][i][k] (+)= sum_s slab[s][i][j*n1p + k]   (slab leading dimension ldz = n2*n1p), fixed order
__global__ void ens_reduce_t2_kernel(const c128* slabs, int S, int n2, int n3, int n1, int n3p, int n1p, c128* out,
                                     int accumulate) {
  const size_t tot = (size_t)n2 * n3 * n1;
  const size_t ldz = (size_t)n2 * n1p;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % n1);
    const int i = (int)((e / n1) % n3);
    const int j = (int)(e / ((size_t)n1 * n3));
    c128 v = accumulate ? out[e] : cmk(0, 0);
    v = slab_sum(v, 0, S, [&](int s) { return slabs[((size_t)s * n3p + i) * ldz + (size_t)j * n1p + k]; });
    out[e] = v;
  }
}

// ---- t2 scan without a per-t2 operand: with P_m = X_m B_m and Q_m = C_m Y_m,
//   S_j = sum_m P_m diag(e^{lam_m t2_j}) Q_m = P * diag(E_j) * Q,   E_j[(m,r)] = e^{lam_mr t2_j},
// so P [n3p][Kp] and Q [Kp][n1p] are built once per scan and the GEMM's B operand for waiting time j is
// Q with its rows scaled by E_j, formed in the staging step (one complex multiply per staged element).
// P block: MB = floor(256 / max(np, nr)) members; thread c < MB np computes x_{m p}(t) for (m, p) =
// (m0 + c / np, c % np), the X values of a 16-row group go through LDS, and output thread c < MB nr,
// (m, r) = (m0 + c / nr, c % nr), contracts its member's np values with B_m[:, r] (registers).
// np = nr = nL and lamp = lam in the unpruned form; the host passes the compact index sets otherwise.
__global__ __launch_bounds__(256) void ens_p_uniform_kernel(const c128* alpha, const c128* Bm, const c128* lamp, int M,
                                                            int np, int nr, double t0, double dt, int n3, int n3p,
                                                            int Kp, c128* P) {
  __shared__ c128 sX[16 * 256];
  const int MB = 256 / (np > nr ? np : nr);
  const int m0 = blockIdx.x * MB;
  const int c = threadIdx.x;
  // X part: x_{m p}(t) = i alpha_mp e^{lamp_mp t} for (m, p) = (m0 + c / np, c % np)
  const int mx = m0 + c / np, px = c % np;
  const bool xcol = c < MB * np && mx < M;
  const int kx = mx * np + px;
  const c128 l = xcol ? lamp[kx] : cmk(0, 0);
  const c128 a = xcol ? cmuli(alpha[kx]) : cmk(0, 0);
  // output column (m, r) = (m0 + c / nr, c % nr), P column kk = m nr + r
  const int m = m0 + c / nr, r = c % nr;
  const bool col = c < MB * nr && m < M;
  const int kk = m * nr + r;
  c128 T1[16];
  T1[0] = cmk(1, 0);
  const c128 st = cexp_t(l, dt);
#pragma unroll
  for (int j = 1; j < 16; ++j) T1[j] = cmul(T1[j - 1], st);
  c128 b[ZMAX];
#pragma unroll
  for (int p = 0; p < ZMAX; ++p) b[p] = (col && p < np) ? Bm[((size_t)m * np + p) * nr + r] : cmk(0, 0);
  const int mc0 = (c / nr) * np;             // first sX column of this output thread's member
  for (int g = 0; g < UNI_ROWS / 16; ++g) {
    const int ib = (int)blockIdx.y * UNI_ROWS + 16 * g;
    const c128 base = cmul(a, cexp_t(l, t0 + (double)ib * dt));
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) sX[j * 256 + c] = cmul(base, T1[j]);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int i = ib + j;
      if (i >= n3p) break;
      c128 v = cmk(0, 0);
      if (col && i < n3) {
#pragma unroll
        for (int p = 0; p < ZMAX; ++p)
          if (p < np) v = cadd(v, cmul(sX[j * 256 + mc0 + p], b[p]));
      }
      if (col && kk < Kp) P[(size_t)i * Kp + kk] = v;
    }
  }
}

// columns K..Kp-1 of P are padding (the member blocks cover columns < K only)
__global__ void ens_p_pad_kernel(int K, int Kp, int n3p, c128* P) {
  const int w = Kp - K;
  const size_t tot = (size_t)n3p * w;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x)
    P[(e / w) * Kp + K + e % w] = cmk(0, 0);
}

// E [n2][Kp]: e^{lam_kk t2_j}, zero in the padding
__global__ void ens_e_kernel(const c128* lam, int K, int Kp, const double* t2, int n2, c128* E) {
  const size_t tot = (size_t)n2 * Kp;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int kk = (int)(e % Kp), j = (int)(e / Kp);
    E[e] = kk < K ? cexp_t(lam[kk], t2[j]) : cmk(0, 0);
  }
}

struct EnsQEB {
  struct Raw { cg_v2 q, e; };
  const c128* Q;
  const c128* Ej;   // E row of this column block's waiting time
  int n1p, col0, k0;
  __device__ __forceinline__ Raw fetch(int t, int e, int) const {
    const int row = k0 + t * CG_KT + e / ENS_BT;
    return Raw{cg_ld(Q + (size_t)row * n1p + col0 + (e % ENS_BT)), cg_ld(Ej + row)};
  }
  __device__ __forceinline__ cg_v2 finish(const Raw& r, int, int, int) const {
    const c128 v = cmul(cmk(r.e.x, r.e.y), cmk(r.q.x, r.q.y));
    return cg_v2{v.re, v.im};
  }
};

// grid: (n2 * n1p / BT) x (n3p / BT) x S; column block bn is waiting time (bn * BT) / n1p
__global__ __launch_bounds__(CG_WG) void ens_t2_gemm_kernel(const c128* P, int Kp, const c128* Q, int n1p,
                                                            const c128* E, int tiles, int S, c128* slabs, int n3p,
                                                            int ldz) {
  __shared__ CgLds<ENS_BT> L;
  int bn, bm, s;
  ens_tile(bn, bm, s);
  const int t0 = (int)((long)tiles * s / S), t1 = (int)((long)tiles * (s + 1) / S);
  const int j = (bn * ENS_BT) / n1p, colq = (bn * ENS_BT) % n1p;
  CgAcc<ENS_BT> A;
  c128* slab = slabs + (size_t)s * n3p * ldz;
  if (t1 > t0) {
    EnsXA pa{P, Kp, bm * ENS_BT, t0 * CG_KT};
    EnsQEB pb{Q, E + (size_t)j * Kp, n1p, colq, t0 * CG_KT};
    cg_block_gemm_gen<ENS_BT>(t1 - t0, pa, pb, L, A);
    cg_epilogue<ENS_BT>(A, [&](int row, int col, c128 v) {
      slab[(size_t)(bm * ENS_BT + row) * ldz + bn * ENS_BT + col] = v;
    });
  } else {
    for (int e = threadIdx.x; e < ENS_BT * ENS_BT; e += CG_WG)
      slab[(size_t)(bm * ENS_BT + e / ENS_BT) * ldz + bn * ENS_BT + e % ENS_BT] = cmk(0, 0);
  }
}

}  // namespace
}  // namespace qd
