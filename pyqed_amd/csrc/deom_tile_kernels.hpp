// deom_tile_kernels.hpp — the DEOM stage kernels for any ns and any number of modes (deom.hip): the VALU tile kernel
// and its MFMA form.
#pragma once

#include "deom_kernels.hpp"

namespace qd {
namespace {

// ---------------------------------------------------------------- any ns, any number of modes
// Tiled stage kernel for hierarchies the register / MFMA-16 kernels do not cover (ns > 16, more than
// DEOM_MAX_NMOD coupling operators, or K beyond their tables).  Grouping the stencil by mode m,
//   d_n = damp_n x_n + [-i H(t) | Q_1 .. Q_M] [x_n ; Y_1 .. Y_M] + [x_n | Z_1 .. Z_M] [i H(t) ; Q_1 .. Q_M],
//   Y_m = sum_{k: mode k = m} cL_nk x_{n-e_k} + cP_nk x_{n+e_k},   Z_m = sum_{k: mode k = m} cR_nk x_{n-e_k} - cP_nk x_{n+e_k},
// i.e. one complex GEMM of inner dimension 2 (1 + M) ns per ADO.  One workgroup per 16 x 16 output tile of one
// ADO (256 threads, one element each); the A / B operand tiles (16 x 16) are staged in LDS chunk by chunk, the
// neighbour combinations Y_m / Z_m formed while loading (no scratch), H(t) = H + f_s Hdip, Q(t) = Q + f_c Qdip
// likewise.  Same RK4 epilogue as deom_stage_kernel.  Flat-loop form (tools/cpu_emu runs it on the host).
__global__ __launch_bounds__(256) void deom_stage_tile_kernel(DeomParams p) {
  __shared__ c128 sA[DEOM_TT][DEOM_TT + 1];
  __shared__ c128 sB[DEOM_TT][DEOM_TT + 1];
  __shared__ c128 sacc[DEOM_TT * DEOM_TT];
  const int ns = p.ns, ns2 = ns * ns, K = p.K;
  const int nt = (ns + DEOM_TT - 1) / DEOM_TT;
  const long tile = blockIdx.x;
  const int tj = (int)(tile % nt), ti = (int)((tile / nt) % nt);
  const long bn = tile / ((long)nt * nt);
  const int n = (int)(bn % p.nmax);
  const size_t bbase = (size_t)(bn - n) * ns2;
  const c128* X = p.xin + bbase;
  const c128* xn = X + (size_t)n * ns2;
  const int* mi = p.minus + (size_t)n * K;
  const int* pl = p.plus + (size_t)n * K;
  const c128* cf = p.coef + (size_t)n * K * 3;
  const int i0 = ti * DEOM_TT, j0 = tj * DEOM_TT;
  auto hq = [&](int seg, int r, int c) {   // segment 0: H(t), segment m + 1: Q_m(t)
    if (seg == 0) return p.Hdip ? cadd(p.H[r * ns + c], cmul(p.Hdip[r * ns + c], p.fs)) : p.H[r * ns + c];
    const size_t o = (size_t)(seg - 1) * ns2 + r * ns + c;
    return p.Qdip ? cadd(p.Q[o], cmul(p.Qdip[o], p.fc)) : p.Q[o];
  };
  auto mix = [&](int m, int r, int c, bool right) {   // Y_m (left) / Z_m (right) element (r, c)
    c128 v = cmk(0.0, 0.0);
    for (int k = 0; k < K; ++k) {
      if (p.mode[k] != m) continue;
      const int a = mi[k], b = pl[k];
      if (a >= 0) v = cadd(v, cmul(cf[3 * k + (right ? 1 : 0)], X[(size_t)a * ns2 + r * ns + c]));
      if (b >= 0) {
        const c128 t = cmul(cf[3 * k + 2], X[(size_t)b * ns2 + r * ns + c]);
        v = right ? csub(v, t) : cadd(v, t);
      }
    }
    return v;
  };
  for (int f = threadIdx.x; f < DEOM_TT * DEOM_TT; f += blockDim.x) sacc[f] = cmk(0.0, 0.0);
  for (int side = 0; side < 2; ++side) {
    for (int seg = 0; seg <= p.nmod; ++seg) {
      for (int l0 = 0; l0 < ns; l0 += DEOM_TT) {
        __syncthreads();
        for (int f = threadIdx.x; f < DEOM_TT * DEOM_TT; f += blockDim.x) {
          const int r = f / DEOM_TT, c = f % DEOM_TT;
          const int ia = i0 + r, la = l0 + c;     // A[ia][la]
          const int lb = l0 + r, jb = j0 + c;     // B[lb][jb]
          c128 a = cmk(0.0, 0.0), b = cmk(0.0, 0.0);
          if (side == 0) {           // [-i H | Q_m] x [x_n ; Y_m]
            if (ia < ns && la < ns) a = seg == 0 ? cmulmi(hq(0, ia, la)) : hq(seg, ia, la);
            if (lb < ns && jb < ns) b = seg == 0 ? xn[lb * ns + jb] : mix(seg - 1, lb, jb, false);
          } else {                   // [x_n | Z_m] x [i H ; Q_m]
            if (ia < ns && la < ns) a = seg == 0 ? xn[ia * ns + la] : mix(seg - 1, ia, la, true);
            if (lb < ns && jb < ns) b = seg == 0 ? cmuli(hq(0, lb, jb)) : hq(seg, lb, jb);
          }
          sA[r][c] = a;
          sB[r][c] = b;
        }
        __syncthreads();
        for (int f = threadIdx.x; f < DEOM_TT * DEOM_TT; f += blockDim.x) {
          const int r = f / DEOM_TT, c = f % DEOM_TT;
          c128 s = sacc[f];
          for (int kk = 0; kk < DEOM_TT; ++kk) s = cadd(s, cmul(sA[r][kk], sB[kk][c]));
          sacc[f] = s;
        }
      }
    }
  }
  __syncthreads();
  const double dt = p.dt;
  for (int f = threadIdx.x; f < DEOM_TT * DEOM_TT; f += blockDim.x) {
    const int i = i0 + f / DEOM_TT, j = j0 + f % DEOM_TT;
    if (i >= ns || j >= ns) continue;
    const size_t e = bbase + (size_t)n * ns2 + (size_t)i * ns + j;
    const c128 d = cadd(sacc[f], cmul(p.damp[n], xn[i * ns + j]));
    const c128 r0 = p.rho ? p.rho[e] : cmk(0, 0);   // rho == nullptr: qd_deom_apply
    c128 a = (p.stage > 0 && !p.horner) ? p.acc[e] : cmk(0, 0);
    const c128 v = deom_rk4_next(p.stage, p.horner, dt, r0, a, d);
    if (p.stage < 3) {
      if (!p.horner) p.acc[e] = a;
      p.xout[e] = v;
    } else {
      p.rho_out[e] = v;
      if (p.snap && n == 0) {
        const size_t b = bn / p.nmax;
        p.snap[(b * (p.nsteps + 1) + p.step + 1) * ns2 + i * ns + j] = v;
      }
    }
  }
}

// MFMA form of the tiled kernel (same regrouping, same epilogue) for ns >= 17: one wave per 16 x 16 output tile,
// the four waves of a workgroup on a 2 x 2 block of tiles of one ADO (their A / B strips meet in the CU's L1).  Each
// 16-wide chunk of the inner dimension is 4 v_mfma_f64_16x16x4_f64 k-steps x 4 real products; lane l holds
// A[i0 + (l & 15)][l0 + 4q + (l >> 4)] and B[l0 + 4q + (l >> 4)][j0 + (l & 15)] (the layouts of
// deom_stage_mfma16_kernel), D rows (l >> 4) + 4r, column l & 15.  Y_m / Z_m elements are formed from the
// neighbours while loading (wave-uniform k loop, scalar table loads).
__global__ __launch_bounds__(256) void deom_stage_tmfma_kernel(DeomParams p) {
  const int ns = p.ns, ns2 = ns * ns, K = p.K;
  const int nt = (ns + 15) / 16, nbk = (nt + 1) / 2;
  const long blk = blockIdx.x;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int bj = (int)(blk % nbk), bi = (int)((blk / nbk) % nbk);
  const long bn = __builtin_amdgcn_readfirstlane((int)(blk / ((long)nbk * nbk)));
  const int ti = 2 * bi + (wv >> 1), tj = 2 * bj + (wv & 1);
  if (ti >= nt || tj >= nt) return;          // wave-uniform; no workgroup barrier below
  const int n = (int)(bn % p.nmax);
  const size_t bbase = (size_t)(bn - n) * ns2;
  const c128* X = p.xin + bbase;
  const c128* xn = X + (size_t)n * ns2;
  const int* mi = p.minus + (size_t)n * K;
  const int* pl = p.plus + (size_t)n * K;
  const c128* cf = p.coef + (size_t)n * K * 3;
  const int i0 = ti * 16, j0 = tj * 16;
  const int lr = lane & 15, rq = lane >> 4;
  auto hq = [&](int seg, int r, int c) -> c128 {
    if (r >= ns || c >= ns) return cmk(0.0, 0.0);
    if (seg == 0) return p.Hdip ? cadd(p.H[r * ns + c], cmul(p.Hdip[r * ns + c], p.fs)) : p.H[r * ns + c];
    const size_t o = (size_t)(seg - 1) * ns2 + r * ns + c;
    return p.Qdip ? cadd(p.Q[o], cmul(p.Qdip[o], p.fc)) : p.Q[o];
  };
  auto xat = [&](int r, int c) -> c128 { return (r < ns && c < ns) ? xn[r * ns + c] : cmk(0.0, 0.0); };
  auto mix = [&](int m, int r, int c, bool right) -> c128 {
    c128 v = cmk(0.0, 0.0);
    if (r >= ns || c >= ns) return v;
    for (int k = 0; k < K; ++k) {
      if (p.mode[k] != m) continue;
      const int a = mi[k], b = pl[k];
      if (a >= 0) v = cadd(v, cmul(cf[3 * k + (right ? 1 : 0)], X[(size_t)a * ns2 + r * ns + c]));
      if (b >= 0) {
        const c128 t = cmul(cf[3 * k + 2], X[(size_t)b * ns2 + r * ns + c]);
        v = right ? csub(v, t) : cadd(v, t);
      }
    }
    return v;
  };
  d4 Dre = d4{0.0, 0.0, 0.0, 0.0}, Dim = d4{0.0, 0.0, 0.0, 0.0};
  auto cmfma = [&](c128 a, c128 b) {
    Dre = __builtin_amdgcn_mfma_f64_16x16x4f64(a.re, b.re, Dre, 0, 0, 0);
    Dim = __builtin_amdgcn_mfma_f64_16x16x4f64(a.re, b.im, Dim, 0, 0, 0);
    Dre = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.im, b.im, Dre, 0, 0, 0);
    Dim = __builtin_amdgcn_mfma_f64_16x16x4f64(a.im, b.re, Dim, 0, 0, 0);
  };
  for (int seg = 0; seg <= p.nmod; ++seg) {
    for (int l0 = 0; l0 < ns; l0 += 16) {
      c128 a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {   // left: [-iH | Q_m] x [x_n ; Y_m]
        const int l = l0 + 4 * q + rq;
        a[q] = seg == 0 ? cmulmi(hq(0, i0 + lr, l)) : hq(seg, i0 + lr, l);
        b[q] = seg == 0 ? xat(l, j0 + lr) : mix(seg - 1, l, j0 + lr, false);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) cmfma(a[q], b[q]);
#pragma unroll
      for (int q = 0; q < 4; ++q) {   // right: [x_n | Z_m] x [iH ; Q_m]
        const int l = l0 + 4 * q + rq;
        a[q] = seg == 0 ? xat(i0 + lr, l) : mix(seg - 1, i0 + lr, l, true);
        b[q] = seg == 0 ? cmuli(hq(0, l, j0 + lr)) : hq(seg, l, j0 + lr);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) cmfma(a[q], b[q]);
    }
  }
  const double dt = p.dt;
  const c128 dmp = p.damp[n];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + rq + 4 * r, j = j0 + lr;
    if (i >= ns || j >= ns) continue;
    const size_t e = bbase + (size_t)n * ns2 + (size_t)i * ns + j;
    const c128 d = cadd(cmk(Dre[r], Dim[r]), cmul(dmp, xn[i * ns + j]));
    const c128 r0 = p.rho ? p.rho[e] : cmk(0, 0);   // rho == nullptr: qd_deom_apply
    c128 a = (p.stage > 0 && !p.horner) ? p.acc[e] : cmk(0, 0);
    const c128 v = deom_rk4_next(p.stage, p.horner, dt, r0, a, d);
    if (p.stage < 3) {
      if (!p.horner) p.acc[e] = a;
      p.xout[e] = v;
    } else {
      p.rho_out[e] = v;
      if (p.snap && n == 0) {
        const size_t b = bn / p.nmax;
        p.snap[(b * (p.nsteps + 1) + p.step + 1) * ns2 + i * ns + j] = v;
      }
    }
  }
}

}  // namespace
}  // namespace qd
