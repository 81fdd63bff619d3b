// ldr_kernels.hpp — the kernels of qd_ldr_run (ldr.hip): the K-tiled axis mode product on the f64 MFMAs with the two
// point rotations of the local diabatic representation fused into its first load and last store, and the point kernels
// of the split path; and the real-matrix pass of qd_ldr_jacobi_run (ldr_real_axis_kernel, below).  Geometry and layouts
// are ldr_plan.hpp's; nothing here decides a shape.
//
// ldr_axis_kernel<EXPAND, PROJECT>: out[o, i, in] = sum_k K[i, k] in[o, k, in] for one axis.  Workgroup (bx, by) owns
// rows by * LDR_RT .. + LDR_RT (wave w the 16 from 16 w on) and the sub-tiles bx * LDR_NSUB + j of `cu` columns.  Per
// K-tile every lane loads its A fragments K[row][k] from global memory (the rows of a wave are its own), the workgroup
// stages the B tile [LDR_KT][LDR_CT] in LDS once (thread t owns column t % LDR_CT and the k-rows t / LDR_CT + 8 i), and
// each wave runs the 4-product complex form on v_mfma_f64_16x16x4_f64 for its LDR_NSUB accumulator pairs.  Rows,
// columns and K past the end are loaded as zeros and never stored.
//   EXPAND:  the staged element is chi[q, mu] = sum_b U[q, mu, b] psi[q, b], formed from psi [B, npts, ns] on load.
//   PROJECT: the axis is the last one (s = 1, column = (o, mu)): a wave parks its finished 16 x 16 tile in LDS and
//            stores psi'[p, a] = expV[p, a] sum_mu conj(U[p, mu, a]) tile[row, q M + mu] for the cu / M points q of the
//            sub-tile, into the next state and, on a snapshot step, into the snapshot.
#pragma once

#include "ldr_plan.hpp"
#include "qd_common.hpp"

namespace qd {
namespace {

struct LdrPass {
  const c128* in;     // chi [B npts M]; psi [B npts ns] when EXPAND
  c128* out;          // chi; psi' [B npts ns] when PROJECT
  const c128* K;      // [n][n]
  const c128* U;      // [npts][M][ns]
  const c128* expV;   // [npts][ns] (PROJECT)
  c128* snap;         // PROJECT: member 0's snapshot of this step, or null
  size_t snap_bstride;   // elements between the members' snapshots
  unsigned C, st, s, outer, npts;
  int n, M, ns, cu;
};

template <bool EXPAND, bool PROJECT>
__global__ __launch_bounds__(LDR_TPB) void ldr_axis_kernel(LdrPass p) {
  extern __shared__ c128 ldr_lds[];
  c128* Bs = ldr_lds;                                   // [LDR_KT][LDR_BS_STRIDE]
  c128* Ds = ldr_lds + LDR_KT * LDR_BS_STRIDE;          // [LDR_WAVES][LDR_SUB][LDR_DS_STRIDE] (PROJECT)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int n = p.n, M = p.M, ns = p.ns;
  const int row0 = (int)blockIdx.y * LDR_RT + LDR_SUB * w;
  const bool wave_live = row0 < n;

  // the column this thread stages
  const int lc = t % LDR_CT, lk = t / LDR_CT;
  const unsigned c = (blockIdx.x * LDR_NSUB + (unsigned)(lc / LDR_SUB)) * (unsigned)p.cu + (unsigned)(lc % LDR_SUB);
  const bool clive = (lc % LDR_SUB) < p.cu && c < p.C;
  const unsigned o = clive ? c / p.st : 0, inner = clive ? c - o * p.st : 0;
  const c128* colp = p.in + (size_t)o * n * p.st + inner;   // plain: element k at colp[k * st]
  unsigned pg0 = 0, pl0 = 0, mu = 0;                        // EXPAND: the point of k = 0, in the batch and in its member
  if constexpr (EXPAND) {
    const unsigned ip = inner / (unsigned)M;
    mu = inner - ip * (unsigned)M;
    pg0 = o * (unsigned)n * p.s + ip;
    pl0 = pg0 - (o / p.outer) * p.npts;
  }

  const int arow = row0 + l15;
  const c128* Arow = p.K + (size_t)(arow < n ? arow : 0) * n;
  d4 accr[LDR_NSUB], acci[LDR_NSUB];
#pragma unroll
  for (int j = 0; j < LDR_NSUB; ++j) accr[j] = acci[j] = d4{0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < n; k0 += LDR_KT) {
    const int nq = min(LDR_KT / 4, (n - k0 + 3) >> 2);
    c128 a[LDR_KT / 4];
#pragma unroll
    for (int q = 0; q < LDR_KT / 4; ++q) {
      const int k = k0 + 4 * q + l4;
      a[q] = (q < nq && arow < n && k < n) ? Arow[k] : cmk(0.0, 0.0);
    }
    __syncthreads();   // the previous tile has been consumed
#pragma unroll
    for (int i = 0; i < LDR_KT * LDR_CT / LDR_TPB; ++i) {
      const int kk = lk + (LDR_TPB / LDR_CT) * i, k = k0 + kk;
      c128 v = cmk(0.0, 0.0);
      if (clive && k < n) {
        if constexpr (EXPAND) {
          const size_t pg = pg0 + (size_t)k * p.s, pl = pl0 + (size_t)k * p.s;
          const c128* u = p.U + (pl * M + mu) * ns;
          const c128* x = p.in + pg * ns;
          for (int b = 0; b < ns; ++b) v = cadd(v, cmul(u[b], x[b]));
        } else {
          v = colp[(size_t)k * p.st];
        }
      }
      Bs[kk * LDR_BS_STRIDE + lc] = v;
    }
    __syncthreads();
    if (wave_live) {
#pragma unroll
      for (int q = 0; q < LDR_KT / 4; ++q) {
        if (q < nq) {   // uniform
#pragma unroll
          for (int j = 0; j < LDR_NSUB; ++j) {
            const c128 b = Bs[(4 * q + l4) * LDR_BS_STRIDE + j * LDR_SUB + l15];
            accr[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q].re, b.re, accr[j], 0, 0, 0);
            acci[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q].re, b.im, acci[j], 0, 0, 0);
            accr[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[q].im, b.im, accr[j], 0, 0, 0);
            acci[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q].im, b.re, acci[j], 0, 0, 0);
          }
        }
      }
    }
  }

  // D: the lane holds rows row0 + lane / 16 + 4 r of column lane % 16 of each sub-tile
  if constexpr (!PROJECT) {
    if (!wave_live) return;
#pragma unroll
    for (int j = 0; j < LDR_NSUB; ++j) {
      const unsigned cj = (blockIdx.x * LDR_NSUB + j) * (unsigned)p.cu + l15;
      if (!(l15 < p.cu && cj < p.C)) continue;
      const unsigned oj = cj / p.st, ij = cj - oj * p.st;
      c128* dst = p.out + (size_t)oj * n * p.st + ij;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = row0 + l4 + 4 * r;
        if (i < n) dst[(size_t)i * p.st] = cmk(accr[j][r], acci[j][r]);
      }
    }
  } else {
    c128* D = Ds + w * LDR_SUB * LDR_DS_STRIDE;
    const int np = p.cu / M, total = LDR_SUB * np * ns;
#pragma unroll
    for (int j = 0; j < LDR_NSUB; ++j) {
      // D is this wave's own, so wave-level ordering of its LDS writes and reads would do; the workgroup barriers
      // are what the compiler is sure to honour, every thread reaches them (the loop bounds are uniform), and their
      // cost next to the K loop has not been measured apart
      __syncthreads();   // the tile of the previous sub-tile has been read
#pragma unroll
      for (int r = 0; r < 4; ++r) D[(l4 + 4 * r) * LDR_DS_STRIDE + l15] = cmk(accr[j][r], acci[j][r]);
      __syncthreads();
      for (int idx = lane; idx < total; idx += 64) {
        const int a = idx % ns, q = (idx / ns) % np, r = idx / (ns * np);
        const int i = row0 + r;
        const unsigned cb = (blockIdx.x * LDR_NSUB + j) * (unsigned)p.cu + (unsigned)(q * M);
        if (!(i < n && cb < p.C)) continue;
        const size_t pg = (size_t)(cb / (unsigned)M) * n + i;   // s = 1: column (o, mu), point o n + i
        const size_t b = pg / p.npts, pl = pg - b * p.npts;
        const c128* u = p.U + pl * M * ns + a;
        const c128* x = D + r * LDR_DS_STRIDE + q * M;
        c128 acc = cmk(0.0, 0.0);
        for (int m = 0; m < M; ++m) acc = cadd(acc, cmul(cconj(u[(size_t)m * ns]), x[m]));
        const c128 v = cmul(p.expV[pl * ns + a], acc);
        p.out[pg * ns + a] = v;
        if (p.snap) p.snap[b * p.snap_bstride + pl * ns + a] = v;
      }
    }
  }
}

// ldr_real_axis_kernel<EXPAND, PHASE, PROJECT>: the pass of ldr_axis_kernel along the last axis (s = 1, st = M, column
// = (o, mu)) with a real matrix F [n][n], for qd_ldr_jacobi_run (ldr_jacobi_plan).  Geometry, staging and the D layout
// are ldr_axis_kernel's; the A fragments are doubles and a k-step is two MFMAs, one into the real and one into the
// imaginary accumulator.
//   EXPAND:  as in ldr_axis_kernel.
//   PHASE:   the stored element is ph[(o mod outer) n + i] acc: ph [npts] has the grid's shape with the row index of
//            the pass in the last axis' place, and o mod outer takes the member out of the column's block index.
//   PROJECT: as in ldr_axis_kernel.
struct LdrRealPass {
  const c128* in;     // chi [B npts M]; psi [B npts ns] when EXPAND
  c128* out;          // chi; psi' [B npts ns] when PROJECT
  const double* F;    // [n][n]
  const c128* ph;     // [npts] (PHASE)
  const c128* U;      // [npts][M][ns]
  const c128* expV;   // [npts][ns] (PROJECT)
  c128* snap;         // PROJECT: member 0's snapshot of this step, or null
  size_t snap_bstride;
  unsigned C, outer, npts;
  int n, M, ns, cu;
};

template <bool EXPAND, bool PHASE, bool PROJECT>
__global__ __launch_bounds__(LDR_TPB) void ldr_real_axis_kernel(LdrRealPass p) {
  static_assert(!(PHASE && PROJECT), "the forward pass multiplies the table, the back pass projects");
  extern __shared__ c128 ldr_lds[];
  c128* Bs = ldr_lds;                                   // [LDR_KT][LDR_BS_STRIDE]
  c128* Ds = ldr_lds + LDR_KT * LDR_BS_STRIDE;          // [LDR_WAVES][LDR_SUB][LDR_DS_STRIDE] (PROJECT)
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int n = p.n, M = p.M, ns = p.ns;
  const unsigned st = (unsigned)M;
  const int row0 = (int)blockIdx.y * LDR_RT + LDR_SUB * w;
  const bool wave_live = row0 < n;

  // the column this thread stages: c = o M + mu, element k at (o n + k) M + mu
  const int lc = t % LDR_CT, lk = t / LDR_CT;
  const unsigned c = (blockIdx.x * LDR_NSUB + (unsigned)(lc / LDR_SUB)) * (unsigned)p.cu + (unsigned)(lc % LDR_SUB);
  const bool clive = (lc % LDR_SUB) < p.cu && c < p.C;
  const unsigned o = clive ? c / st : 0, mu = clive ? c - o * st : 0;
  const c128* colp = p.in + (size_t)o * n * st + mu;
  const unsigned pg0 = o * (unsigned)n;                     // EXPAND: the point of k = 0 in the batch ...
  const unsigned pl0 = pg0 - (o / p.outer) * p.npts;        // ... and in its member

  const int arow = row0 + l15;
  const double* Arow = p.F + (size_t)(arow < n ? arow : 0) * n;
  d4 accr[LDR_NSUB], acci[LDR_NSUB];
#pragma unroll
  for (int j = 0; j < LDR_NSUB; ++j) accr[j] = acci[j] = d4{0.0, 0.0, 0.0, 0.0};

  for (int k0 = 0; k0 < n; k0 += LDR_KT) {
    const int nq = min(LDR_KT / 4, (n - k0 + 3) >> 2);
    double a[LDR_KT / 4];
#pragma unroll
    for (int q = 0; q < LDR_KT / 4; ++q) {
      const int k = k0 + 4 * q + l4;
      a[q] = (q < nq && arow < n && k < n) ? Arow[k] : 0.0;
    }
    __syncthreads();   // the previous tile has been consumed
#pragma unroll
    for (int i = 0; i < LDR_KT * LDR_CT / LDR_TPB; ++i) {
      const int kk = lk + (LDR_TPB / LDR_CT) * i, k = k0 + kk;
      c128 v = cmk(0.0, 0.0);
      if (clive && k < n) {
        if constexpr (EXPAND) {
          const size_t pg = (size_t)pg0 + k, pl = (size_t)pl0 + k;
          const c128* u = p.U + (pl * M + mu) * ns;
          const c128* x = p.in + pg * ns;
          for (int b = 0; b < ns; ++b) v = cadd(v, cmul(u[b], x[b]));
        } else {
          v = colp[(size_t)k * st];
        }
      }
      Bs[kk * LDR_BS_STRIDE + lc] = v;
    }
    __syncthreads();
    if (wave_live) {
#pragma unroll
      for (int q = 0; q < LDR_KT / 4; ++q) {
        if (q < nq) {   // uniform
#pragma unroll
          for (int j = 0; j < LDR_NSUB; ++j) {
            const c128 b = Bs[(4 * q + l4) * LDR_BS_STRIDE + j * LDR_SUB + l15];
            accr[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b.re, accr[j], 0, 0, 0);
            acci[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b.im, acci[j], 0, 0, 0);
          }
        }
      }
    }
  }

  // D: the lane holds rows row0 + lane / 16 + 4 r of column lane % 16 of each sub-tile
  if constexpr (!PROJECT) {
    if (!wave_live) return;
#pragma unroll
    for (int j = 0; j < LDR_NSUB; ++j) {
      const unsigned cj = (blockIdx.x * LDR_NSUB + j) * (unsigned)p.cu + l15;
      if (!(l15 < p.cu && cj < p.C)) continue;
      const unsigned oj = cj / st, ij = cj - oj * st;
      c128* dst = p.out + (size_t)oj * n * st + ij;
      const c128* phr = PHASE ? p.ph + (size_t)(oj % p.outer) * n : nullptr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = row0 + l4 + 4 * r;
        if (i < n) {
          c128 v = cmk(accr[j][r], acci[j][r]);
          if constexpr (PHASE) v = cmul(phr[i], v);
          dst[(size_t)i * st] = v;
        }
      }
    }
  } else {
    c128* D = Ds + w * LDR_SUB * LDR_DS_STRIDE;
    const int np = p.cu / M, total = LDR_SUB * np * ns;
#pragma unroll
    for (int j = 0; j < LDR_NSUB; ++j) {
      // workgroup barriers as in ldr_axis_kernel: every thread reaches them (the loop bounds are uniform)
      __syncthreads();   // the tile of the previous sub-tile has been read
#pragma unroll
      for (int r = 0; r < 4; ++r) D[(l4 + 4 * r) * LDR_DS_STRIDE + l15] = cmk(accr[j][r], acci[j][r]);
      __syncthreads();
      for (int idx = lane; idx < total; idx += 64) {
        const int a = idx % ns, q = (idx / ns) % np, r = idx / (ns * np);
        const int i = row0 + r;
        const unsigned cb = (blockIdx.x * LDR_NSUB + j) * (unsigned)p.cu + (unsigned)(q * M);
        if (!(i < n && cb < p.C)) continue;
        const size_t pg = (size_t)(cb / (unsigned)M) * n + i;   // column (o, mu), point o n + i
        const size_t b = pg / p.npts, pl = pg - b * p.npts;
        const c128* u = p.U + pl * M * ns + a;
        const c128* x = D + r * LDR_DS_STRIDE + q * M;
        c128 acc = cmk(0.0, 0.0);
        for (int m = 0; m < M; ++m) acc = cadd(acc, cmul(cconj(u[(size_t)m * ns]), x[m]));
        const c128 v = cmul(p.expV[pl * ns + a], acc);
        p.out[pg * ns + a] = v;
        if (p.snap) p.snap[b * p.snap_bstride + pl * ns + a] = v;
      }
    }
  }
}

// out[b, p, a] = f[p, a] psi[b, p, a] (the opening half step), per = npts ns
__global__ void ldr_open_kernel(const c128* psi, const c128* f, c128* out, size_t per, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    out[i] = cmul(f[i % per], psi[i]);
}

// chi[b, p, mu] = sum_a U[p, mu, a] psi[b, p, a] (split path)
__global__ void ldr_expand_kernel(const c128* psi, const c128* U, c128* chi, size_t npts, int M, int ns, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pg = i / M, pl = pg % npts;
    const int mu = (int)(i - pg * M);
    const c128* u = U + (pl * M + mu) * ns;
    const c128* x = psi + pg * ns;
    c128 v = cmk(0.0, 0.0);
    for (int b = 0; b < ns; ++b) v = cadd(v, cmul(u[b], x[b]));
    chi[i] = v;
  }
}

// psi'[b, p, a] = expV[p, a] sum_mu conj(U[p, mu, a]) chi[b, p, mu], and the snapshot (split path)
__global__ void ldr_project_kernel(const c128* chi, const c128* U, const c128* expV, c128* out, c128* snap,
                                   size_t snap_bstride, size_t npts, int M, int ns, size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pg = i / ns, b = pg / npts, pl = pg - b * npts;
    const int a = (int)(i - pg * ns);
    const c128* u = U + pl * M * ns + a;
    const c128* x = chi + pg * M;
    c128 acc = cmk(0.0, 0.0);
    for (int m = 0; m < M; ++m) acc = cadd(acc, cmul(cconj(u[(size_t)m * ns]), x[m]));
    const c128 v = cmul(expV[pl * ns + a], acc);
    out[i] = v;
    if (snap) snap[b * snap_bstride + pl * ns + a] = v;
  }
}

}  // namespace
}  // namespace qd
