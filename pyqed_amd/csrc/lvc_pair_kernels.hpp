// lvc_pair_kernels.hpp — the pair record of the LVC model and the run that takes it (gfx950): qd_lvc_pair_observe and
// qd_lvc_pair_rk4 of lvc.hip, launched as LvcPairPlan (lvc_plan.hpp) says.
//
// A pair is a ket and a bra of one model, psi [P][2][D].  Block r of its record is
//   R_r[a][b] = sum_n L_r[a, n] conj(bra[b, n]),   L_0 = ket,  L_{j+1} = x_j ket,
// so that <bra| A (x) 1 |ket> = tr(A R_0) and <bra| A (x) x_j |ket> = tr(A R_{j+1}): a correlation function
// <bra(t)| b |ket(t)> needs the one block of its middle operator.  Nothing is derived by conjugation except the bra
// factor of the sum itself.
//
// Partial kernel: a thread owns the vibrational point n, as in lvc_point.  Up to NEL = LVC_PAIR_REG_NEL it holds the
// NEL bra amplitudes and accumulates all NEL^2 complex sums of the block in one pass: every element of the pair is
// read once, the +-1 neighbours of the ket from the neighbouring lanes' loads or L1 / L2.  Past that one pass takes
// one row a (2 NEL accumulators), as lvc_obs_part_kernel does.  Every sum (r, a, b) has the order of the observable
// record's: thread t of partial workgroup g adds its points of the tiles g, g + G, ..., the 64 lanes by a butterfly,
// the four waves in wave order, the G partial rows in index order, without contraction and without atomics.  So
// identical calls agree bit for bit, a block does not depend on which other blocks are asked for, and with bra = ket
// block r is the rho / X[r - 1] part of qd_lvc_observe's record bit for bit.
//
// Staged run: the existing lvc_stage_kernel on the 2 P contiguous states (four launches per step for all pairs), the
// partial and final launches where a record is due.  Resident run (D <= LVC_PAIR_RESIDENT_MAX_D):
// lvc_resident_pair_kernel, one workgroup per pair for the whole call, four stage vectors in LDS, both base states in
// registers, the record taken from LDS by the same point and tile-sum functions, so the in-run records equal
// qd_lvc_pair_observe of the same states bit for bit on either path.
#pragma once

#include "lvc_kernels.hpp"

namespace qd {

// byte offsets of the pair resident kernel's LDS regions (LvcPairPlan::lds_*)
struct LvcPairLds {
  unsigned ket1, bra0, bra1, tab, wave, tile;
};

// rows of a block one pass accumulates, and the doubles of its partial row (LvcPairPlan::rows, nv)
template <int NEL>
struct LvcPairShape {
  static constexpr int ROWS = NEL <= LVC_PAIR_REG_NEL ? NEL : 1;
  static constexpr int PASSES = NEL / ROWS;
  static constexpr int NV = 2 * NEL * ROWS;
};

// What point n adds to the rows a0 .. a0 + ROWS - 1 of block r: acc[2 (i NEL + b)], acc[2 (i NEL + b) + 1] +=
// left_i conj(bra[b, n]) with left_i = ket[a0 + i, n] (r = 0) or (x_j ket)[a0 + i, n] (r = j + 1): the arithmetic of
// lvc_obs_point.  ldk(a, idx) and ldb(b, idx) return the ket's and the bra's elements.
template <int NEL, int ROWS, typename LdK, typename LdB>
__device__ __forceinline__ void lvc_pair_point(const LvcDev& m, int r, int a0, int n, LdK&& ldk, LdB&& ldb,
                                               double (&acc)[2 * NEL * ROWS]) {
#pragma clang fp contract(off)
  c128 p[NEL];
#pragma unroll
  for (int b = 0; b < NEL; ++b) p[b] = ldb(b, n);
  int s = 0;
  bool lo = false, hi = false;
  double cm = 0.0, cp = 0.0;
  if (r > 0) {
    const int j = r - 1, N = m.dims[j];
    s = m.stride[j];
    const int nj = (n / s) % N;
    cm = sqrt(0.5 * nj);
    cp = sqrt(0.5 * (nj + 1));
    lo = nj > 0;
    hi = nj + 1 < N;
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int a = a0 + i;
    c128 left;
    if (r > 0) {
      const c128 um = lo ? ldk(a, n - s) : cmk(0, 0), up = hi ? ldk(a, n + s) : cmk(0, 0);
      left = cmk(cm * um.re + cp * up.re, cm * um.im + cp * up.im);
    } else {
      left = ldk(a, n);
    }
#pragma unroll
    for (int b = 0; b < NEL; ++b) {
      acc[2 * (i * NEL + b)] += left.re * p[b].re + left.im * p[b].im;
      acc[2 * (i * NEL + b) + 1] += left.im * p[b].re - left.re * p[b].im;
    }
  }
}

// lvc_obs_tile_sum for NV values: the sum of acc over a group of LVC_TILE threads, butterflies, then the group's wave
// rows of `sh` ([4][NV]) in wave order.  Every thread of the workgroup calls it (two __syncthreads); thread t < NV of
// the group returns the sum of value t.
template <int NV>
__device__ __forceinline__ double lvc_pair_tile_sum(double (&acc)[NV], double* sh) {
#pragma clang fp contract(off)
  static_assert(NV <= LVC_TILE, "one thread per value");
  const int t = threadIdx.x % LVC_TILE, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    double s = acc[v];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) sh[wave * NV + v] = s;
  }
  __syncthreads();
  double s = 0.0;
  if (t < NV) s = ((sh[t] + sh[NV + t]) + sh[2 * NV + t]) + sh[3 * NV + t];
  __syncthreads();
  return s;
}

// part[p][k][pass][g][.] of the pairs psi [P][2][D]: grid (G, nblk PASSES, P), LVC_TILE threads
template <int NEL>
__global__ __launch_bounds__(LVC_TILE) void lvc_pair_part_kernel(LvcDev m, LvcPairBlocks bl,
                                                                 const c128* __restrict__ psi_g,
                                                                 double* __restrict__ part) {
  constexpr int ROWS = LvcPairShape<NEL>::ROWS, PASSES = LvcPairShape<NEL>::PASSES, NV = LvcPairShape<NEL>::NV;
  __shared__ double sh[4 * NV];
  const int k = blockIdx.y / PASSES, a0 = (blockIdx.y % PASSES) * ROWS, r = bl.r[k];
  const c128* ket = psi_g + (size_t)blockIdx.z * 2 * m.D;
  const c128* bra = ket + m.D;
  const size_t nvib = m.nvib;
  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
  const int tiles = (m.nvib + LVC_TILE - 1) / LVC_TILE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int n = tile * LVC_TILE + threadIdx.x;
    if (n < m.nvib)
      lvc_pair_point<NEL, ROWS>(
          m, r, a0, n, [&](int a, int idx) { return ket[a * nvib + idx]; },
          [&](int b, int idx) { return bra[b * nvib + idx]; }, acc);
  }
  const double s = lvc_pair_tile_sum<NV>(acc, sh);
  if (threadIdx.x < NV)
    part[(((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * NV + threadIdx.x] = s;
}

// The G partial rows of every value of pair blockIdx.x summed in index order into its record [nblk][nel][nel]; grid
// (P), LVC_TILE threads.  rec_pstride: doubles from one pair's record to the next pair's.
__global__ __launch_bounds__(LVC_TILE) void lvc_pair_final_kernel(int nel, int nblk, int rows, int G,
                                                                  const double* __restrict__ part,
                                                                  double* __restrict__ rec, size_t rec_pstride) {
#pragma clang fp contract(off)
  const int passes = nel / rows, nv = 2 * nel * rows, nblock = 2 * nel * nel;
  const double* pb = part + (size_t)blockIdx.x * nblk * passes * G * nv;
  double* out = rec + blockIdx.x * rec_pstride;
  for (int o = threadIdx.x; o < nblk * nblock; o += LVC_TILE) {
    const int k = o / nblock, w = o % nblock, q = w / nv, v = w % nv;   // row a = w / (2 nel) is row a % rows of pass q
    const double* row = pb + ((size_t)(k * passes + q) * G) * nv + v;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += row[(size_t)g * nv];
    out[o] = s;
  }
}

// The record of the pair in LDS (resident kernel, LVC_RES_TPB threads, every thread calls it): group q of LVC_TILE
// threads plays the partial workgroups q, q + 2, ... of lvc_pair_part_kernel (one tile each: nvib <=
// LVC_PAIR_RESIDENT_MAX_D keeps G = tiles), then the tile partials are summed as lvc_pair_final_kernel sums them.
template <int NEL>
__device__ __forceinline__ void lvc_pair_obs_resident(const LvcDev& m, const LvcPairBlocks& bl, const c128* ket,
                                                      const c128* bra, double* sh_wave, double* sh_tile, double* rec) {
#pragma clang fp contract(off)
  constexpr int ROWS = LvcPairShape<NEL>::ROWS, PASSES = LvcPairShape<NEL>::PASSES, NV = LvcPairShape<NEL>::NV;
  constexpr int GROUPS = LVC_RES_TPB / LVC_TILE;
  const int q = threadIdx.x / LVC_TILE, t = threadIdx.x % LVC_TILE;
  const int G = (m.nvib + LVC_TILE - 1) / LVC_TILE;
  const size_t nvib = m.nvib;
  for (int k = 0; k < bl.nblk; ++k) {
    const int r = bl.r[k];
    for (int pass = 0; pass < PASSES; ++pass) {
      const int a0 = pass * ROWS;
      for (int g0 = 0; g0 < G; g0 += GROUPS) {
        const int g = g0 + q, n = g * LVC_TILE + t;
        double acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = 0.0;
        if (g < G && n < m.nvib)
          lvc_pair_point<NEL, ROWS>(
              m, r, a0, n, [&](int a, int idx) { return ket[a * nvib + idx]; },
              [&](int b, int idx) { return bra[b * nvib + idx]; }, acc);
        const double s = lvc_pair_tile_sum<NV>(acc, sh_wave + q * 4 * NV);
        if (g < G && t < NV) sh_tile[g * NV + t] = s;
      }
      __syncthreads();
      if ((int)threadIdx.x < NV) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += sh_tile[g * NV + threadIdx.x];
        rec[2 * ((k * NEL + a0) * NEL) + threadIdx.x] = s;
      }
      __syncthreads();
    }
  }
}

// The whole qd_lvc_pair_rk4 call of pair blockIdx.x: grid (P), LVC_RES_TPB threads, dynamic LDS as LvcPairPlan::lds_*
// lay it out.  lvc_resident_kernel for two states at once: thread t owns the vibrational points t, t + LVC_RES_TPB,
// ... (at most KP) of the ket and of the bra, each state's stage vectors ping-pong between its A and B (A -> B -> A
// -> B -> A), so both new states are in their A vectors (and in the registers) when the step ends and the record is
// read from there.  rec [P][nsave + 1][nrec] complex, one record at t0 and one after every save_every steps.
template <int NEL>
__global__ __launch_bounds__(LVC_RES_TPB) void lvc_resident_pair_kernel(LvcDev m, LvcPairBlocks bl, LvcPairLds L,
                                                                        const c128* __restrict__ Hel,
                                                                        const c128* __restrict__ W, c128* psi_g,
                                                                        double dt, int nsteps, int save_every,
                                                                        int nsave, double* __restrict__ rec,
                                                                        int nrec) {
  constexpr int KP = (int)((((LVC_PAIR_RESIDENT_MAX_D + NEL - 1) / NEL) + LVC_RES_TPB - 1) / LVC_RES_TPB);
  extern __shared__ __attribute__((aligned(16))) char lvc_smem[];
  c128* const A[2] = {(c128*)lvc_smem, (c128*)(lvc_smem + L.bra0)};
  c128* const Bv[2] = {(c128*)(lvc_smem + L.ket1), (c128*)(lvc_smem + L.bra1)};
  c128* tab = (c128*)(lvc_smem + L.tab);
  double* sh_wave = (double*)(lvc_smem + L.wave);
  double* sh_tile = (double*)(lvc_smem + L.tile);
  const size_t nvib = m.nvib;
  c128* psi = psi_g + (size_t)blockIdx.x * 2 * m.D;
  double* orec = rec + (size_t)blockIdx.x * (nsave + 1) * nrec * 2;
  lvc_load_tables(tab, Hel, W, NEL, m.M);
  c128 base[2][KP][NEL];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int n = threadIdx.x + k * LVC_RES_TPB;
#pragma unroll
      for (int a = 0; a < NEL; ++a) {
        base[w][k][a] = n < m.nvib ? psi[(size_t)w * m.D + a * nvib + n] : cmk(0, 0);
        if (n < m.nvib) A[w][a * nvib + n] = base[w][k][a];
      }
    }
  }
  __syncthreads();
  lvc_pair_obs_resident<NEL>(m, bl, A[0], A[1], sh_wave, sh_tile, orec);
  for (int s = 0; s < nsteps; ++s) {
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
      const double coef = rk4_horner_coef(dt, stage);
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const c128* src = (stage & 1) ? Bv[w] : A[w];
        c128* dst = (stage & 1) ? A[w] : Bv[w];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          const int n = threadIdx.x + k * LVC_RES_TPB;
          if (n < m.nvib) {
            c128 v[NEL], y[NEL];
            lvc_point<NEL>(m, tab, n, [&](int b, int idx) { return src[b * nvib + idx]; }, v, y);
#pragma unroll
            for (int a = 0; a < NEL; ++a) {
              const c128 o = cadd(base[w][k][a], cscale(cmulmi(y[a]), coef));
              dst[a * nvib + n] = o;
              if (stage == 3) base[w][k][a] = o;
            }
          }
        }
      }
      __syncthreads();
    }
    if ((s + 1) % save_every == 0)
      lvc_pair_obs_resident<NEL>(m, bl, A[0], A[1], sh_wave, sh_tile,
                                 orec + (size_t)((s + 1) / save_every) * nrec * 2);
  }
#pragma unroll
  for (int w = 0; w < 2; ++w) {
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const int n = threadIdx.x + k * LVC_RES_TPB;
      if (n < m.nvib) {
#pragma unroll
        for (int a = 0; a < NEL; ++a) psi[(size_t)w * m.D + a * nvib + n] = base[w][k][a];
      }
    }
  }
}

}  // namespace qd
