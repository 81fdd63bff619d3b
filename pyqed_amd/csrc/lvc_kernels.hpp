// lvc_kernels.hpp — the kernels of the linear-vibronic-coupling model in Fock space (gfx950); lvc.hip launches them as
// lvc_plan.hpp says.
//
//   (H psi)[a, n] = sum_b Hel[a][b] psi[b, n] + (sum_j omega_j n_j) psi[a, n]
//                 + sum_j sum_b W[j][a][b] ( sqrt(n_j / 2) psi[b, n - e_j] + sqrt((n_j + 1) / 2) psi[b, n + e_j] )
//
// with the terms that would leave 0 <= n_j < N_j dropped.  A thread owns one vibrational multi-index n and all NEL
// amplitudes psi[., n] in registers (lvc_point): the +-1 neighbours along the fastest axis are the neighbouring lanes'
// own 16-byte loads, those along a slower axis coalesced 16-byte loads at the axis stride, served from L1 / L2.  Hel
// and W sit in LDS and are read at wave-uniform addresses (broadcasts); the dimensions, strides and frequencies are
// kernel arguments.  Nothing is derived by conjugation: Hel and W may be any complex matrices.
//
// Staged path (any D): lvc_stage_kernel, one launch per Horner stage, out = psi + c (-iH) v.  Resident path
// (D <= LVC_RESIDENT_MAX_D): lvc_resident_kernel, one workgroup per batch member runs the whole call; the two stage
// vectors ping-pong in LDS, the step's base state stays in the owning threads' registers, and snapshots and
// observables are written from inside the loop.
//
// Observables, one record of nobs = nel^2 (1 + M) + M complex values:
//   rho[a][b] = sum_n psi[a,n] conj(psi[b,n]),  X[j][a][b] = sum_n (x_j psi)[a,n] conj(psi[b,n]),
//   nbar[j] = sum_{a,n} n_j |psi[a,n]|^2.
// Row (r, a) of the record (r = 0: rho, r = j + 1: X[j]) is summed in an order the shape alone fixes: thread t of
// partial workgroup g adds its points of the tiles g, g + G, ... (lvc_obs_point), the 64 lanes of a wave are summed by a
// butterfly, the four waves in wave order, and the G partial rows in index order (lvc_obs_tile_sum, then a serial sum).
// The resident kernel plays the partial workgroups with its two groups of LVC_TILE threads and runs the same
// functions on its LDS copy of the state, with floating-point contraction off in both, so its in-run records equal
// qd_lvc_observe of the stored snapshot bit for bit.  No atomics anywhere.
//
// Laser-driven runs (qd_lvc_driven_rk4, at the end of this file): the same stencil with tables rebuilt from a field row
// in device memory (lvc_load_tables_driven); lvc_stage_driven_kernel and lvc_stage_rk4_kernel on the staged path,
// lvc_resident_driven_kernel on the resident one.
#pragma once

#include "lvc_plan.hpp"
#include "qd_common.hpp"

namespace qd {

// byte offsets of the resident kernel's LDS regions (LvcPlan::lds_*)
struct LvcLds {
  unsigned vec1, tab, wave, tile, nbar;
};

// Hel [NEL][NEL] then W [M][NEL][NEL] into LDS (the caller synchronises)
__device__ __forceinline__ void lvc_load_tables(c128* tab, const c128* __restrict__ Hel, const c128* __restrict__ W,
                                                int nel, int M) {
  const int nn = nel * nel;
  for (int e = threadIdx.x; e < (1 + M) * nn; e += blockDim.x) tab[e] = e < nn ? Hel[e] : W[e - nn];
}

// y = (H v)[., n] for the vibrational point n < nvib; ld(b, idx) returns v[b, idx]
template <int NEL, typename Load>
__device__ __forceinline__ void lvc_point(const LvcDev& m, const c128* tab, int n, Load&& ld, c128 (&v)[NEL],
                                          c128 (&y)[NEL]) {
#pragma unroll
  for (int b = 0; b < NEL; ++b) v[b] = ld(b, n);
#pragma unroll
  for (int a = 0; a < NEL; ++a) {
    c128 s = cmul(tab[a * NEL], v[0]);
#pragma unroll
    for (int b = 1; b < NEL; ++b) s = cadd(s, cmul(tab[a * NEL + b], v[b]));
    y[a] = s;
  }
  double diag = 0.0;
  for (int j = 0; j < m.M; ++j) {
    const int s = m.stride[j], N = m.dims[j];
    const int nj = (n / s) % N;
    diag += m.omega[j] * nj;
    const bool lo = nj > 0, hi = nj + 1 < N;
    if (!(lo || hi)) continue;
    const double cm = sqrt(0.5 * nj), cp = sqrt(0.5 * (nj + 1));
    c128 t[NEL];
#pragma unroll
    for (int b = 0; b < NEL; ++b) {
      const c128 um = lo ? ld(b, n - s) : cmk(0, 0), up = hi ? ld(b, n + s) : cmk(0, 0);
      t[b] = cmk(cm * um.re + cp * up.re, cm * um.im + cp * up.im);
    }
    const c128* Wj = tab + (1 + j) * NEL * NEL;
#pragma unroll
    for (int a = 0; a < NEL; ++a) {
#pragma unroll
      for (int b = 0; b < NEL; ++b) y[a] = cadd(y[a], cmul(Wj[a * NEL + b], t[b]));
    }
  }
#pragma unroll
  for (int a = 0; a < NEL; ++a) y[a] = cadd(y[a], cscale(v[a], diag));
}

// One Horner stage out = base + coef (-iH) v of B states, or out = H v when base is null (qd_lvc_apply).
// grid (ceil(nvib / LVC_TILE), B), LVC_TILE threads, dynamic LDS (1 + M) NEL^2 c128.  out may be base (stage 3 writes
// psi in place: every thread reads and writes its own elements of it); v must be neither.
template <int NEL>
__global__ __launch_bounds__(LVC_TILE) void lvc_stage_kernel(LvcDev m, const c128* __restrict__ Hel,
                                                             const c128* __restrict__ W, const c128* v_g,
                                                             const c128* base_g, c128* out_g, double coef) {
  extern __shared__ __attribute__((aligned(16))) char lvc_smem[];
  c128* tab = (c128*)lvc_smem;
  lvc_load_tables(tab, Hel, W, NEL, m.M);
  __syncthreads();
  const int n = blockIdx.x * LVC_TILE + threadIdx.x;
  if (n >= m.nvib) return;
  const size_t off = (size_t)blockIdx.y * m.D;
  const c128* vin = v_g + off;
  const size_t nvib = m.nvib;
  c128 v[NEL], y[NEL];
  lvc_point<NEL>(m, tab, n, [&](int b, int idx) { return vin[b * nvib + idx]; }, v, y);
#pragma unroll
  for (int a = 0; a < NEL; ++a) {
    const size_t e = off + a * nvib + n;
    out_g[e] = base_g ? cadd(base_g[e], cscale(cmulmi(y[a]), coef)) : y[a];
  }
}

// snap[b][idx - 1][.] = psi[b][.] for B states of D elements (grid-strided)
__global__ void lvc_snap_kernel(const c128* __restrict__ psi, int B, int D, int nsave, int idx, c128* __restrict__ snap) {
  const size_t tot = (size_t)B * D;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x)
    snap[((e / D) * nsave + idx - 1) * D + e % D] = psi[e];
}

// ---------------------------------------------------------------- observables
// What point n adds to row (r, a): acc[2 b], acc[2 b + 1] += left conj(psi[b, n]) with left = psi[a, n] (r = 0) or
// (x_j psi)[a, n] (r = j + 1); acc[2 LVC_MAX_NEL] += n_j |psi[a, n]|^2 (r >= 1).
template <typename Load>
__device__ __forceinline__ void lvc_obs_point(const LvcDev& m, int r, int a, int n, Load&& ld,
                                              double (&acc)[LVC_OBS_NV]) {
#pragma clang fp contract(off)
  const c128 c = ld(a, n);
  c128 left = c;
  if (r > 0) {
    const int j = r - 1, s = m.stride[j], N = m.dims[j];
    const int nj = (n / s) % N;
    const double cm = sqrt(0.5 * nj), cp = sqrt(0.5 * (nj + 1));
    const c128 um = nj > 0 ? ld(a, n - s) : cmk(0, 0), up = nj + 1 < N ? ld(a, n + s) : cmk(0, 0);
    left = cmk(cm * um.re + cp * up.re, cm * um.im + cp * up.im);
    acc[2 * LVC_MAX_NEL] += nj * (c.re * c.re + c.im * c.im);
  }
#pragma unroll
  for (int b = 0; b < LVC_MAX_NEL; ++b) {
    if (b < m.nel) {
      const c128 p = ld(b, n);
      acc[2 * b] += left.re * p.re + left.im * p.im;
      acc[2 * b + 1] += left.im * p.re - left.re * p.im;
    }
  }
}

// The sum of acc over a group of LVC_TILE threads (four whole waves): butterflies, then the group's wave rows of `sh`
// ([4][LVC_OBS_NV]) in wave order.  Every thread of the workgroup calls it (two __syncthreads); thread t < LVC_OBS_NV
// of the group returns the sum of value t.
__device__ __forceinline__ double lvc_obs_tile_sum(double (&acc)[LVC_OBS_NV], double* sh) {
#pragma clang fp contract(off)
  const int t = threadIdx.x % LVC_TILE, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int v = 0; v < LVC_OBS_NV; ++v) {
    double s = acc[v];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) sh[wave * LVC_OBS_NV + v] = s;
  }
  __syncthreads();
  double s = 0.0;
  if (t < LVC_OBS_NV) s = ((sh[t] + sh[LVC_OBS_NV + t]) + sh[2 * LVC_OBS_NV + t]) + sh[3 * LVC_OBS_NV + t];
  __syncthreads();
  return s;
}

// Where value v of row (r, a) goes in a record: the double slot of rec, or -1 for the nbar part (summed over a after)
__device__ __forceinline__ int lvc_obs_slot(int nel, int r, int a, int v) {
  return v < 2 * nel ? 2 * ((r * nel + a) * nel + (v >> 1)) + (v & 1) : -1;
}

// part[b][row][g][.] of states psi [B][D]: grid (G, rows, B), LVC_TILE threads
__global__ __launch_bounds__(LVC_TILE) void lvc_obs_part_kernel(LvcDev m, const c128* __restrict__ psi_g, size_t bstride,
                                                                double* __restrict__ part) {
  __shared__ double sh[4 * LVC_OBS_NV];
  const int row = blockIdx.y, r = row / m.nel, a = row % m.nel;
  const c128* psi = psi_g + (size_t)blockIdx.z * bstride;
  const size_t nvib = m.nvib;
  double acc[LVC_OBS_NV];
#pragma unroll
  for (int v = 0; v < LVC_OBS_NV; ++v) acc[v] = 0.0;
  const int tiles = (m.nvib + LVC_TILE - 1) / LVC_TILE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int n = tile * LVC_TILE + threadIdx.x;
    if (n < m.nvib) lvc_obs_point(m, r, a, n, [&](int b, int idx) { return psi[b * nvib + idx]; }, acc);
  }
  const double s = lvc_obs_tile_sum(acc, sh);
  if (threadIdx.x < LVC_OBS_NV)
    part[(((size_t)blockIdx.z * gridDim.y + row) * gridDim.x + blockIdx.x) * LVC_OBS_NV + threadIdx.x] = s;
}

// The G partial rows of every (row, value) of member blockIdx.x summed in index order into its record; nbar[j] adds the
// rows' parts in the order a = 0, 1, ...  grid (B), LVC_TILE threads.
__global__ __launch_bounds__(LVC_TILE) void lvc_obs_final_kernel(int nel, int M, int G, const double* __restrict__ part,
                                                                 double* __restrict__ obs, size_t obs_bstride) {
#pragma clang fp contract(off)
  __shared__ double nb[LVC_MAX_MODES * LVC_MAX_NEL];
  const int rows = (1 + M) * nel;
  const double* pb = part + (size_t)blockIdx.x * rows * G * LVC_OBS_NV;
  double* rec = obs + blockIdx.x * obs_bstride;
  for (int o = threadIdx.x; o < rows * LVC_OBS_NV; o += LVC_TILE) {
    const int row = o / LVC_OBS_NV, v = o % LVC_OBS_NV, r = row / nel, a = row % nel;
    const bool nbar = v == 2 * LVC_MAX_NEL && r > 0;
    if (!(v < 2 * nel || nbar)) continue;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += pb[((size_t)row * G + g) * LVC_OBS_NV + v];
    if (nbar) nb[(r - 1) * nel + a] = s;
    else rec[lvc_obs_slot(nel, r, a, v)] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < M) {
    double s = 0.0;
    for (int a = 0; a < nel; ++a) s += nb[threadIdx.x * nel + a];
    rec[2 * (nel * nel * (1 + M) + threadIdx.x)] = s;
    rec[2 * (nel * nel * (1 + M) + threadIdx.x) + 1] = 0.0;
  }
}

// The record of the state in LDS (resident kernel, LVC_RES_TPB threads, every thread calls it): group q of LVC_TILE
// threads plays the partial workgroups q, q + 2, ... of lvc_obs_part_kernel (one tile each: nvib <= LVC_RESIDENT_MAX_D
// keeps G = tiles), then the tile partials are summed as lvc_obs_final_kernel sums them.
__device__ __forceinline__ void lvc_obs_resident(const LvcDev& m, const c128* st, double* sh_wave, double* sh_tile,
                                                 double* sh_nb, double* rec) {
#pragma clang fp contract(off)
  constexpr int GROUPS = LVC_RES_TPB / LVC_TILE;
  const int q = threadIdx.x / LVC_TILE, t = threadIdx.x % LVC_TILE;
  const int G = (m.nvib + LVC_TILE - 1) / LVC_TILE, rows = (1 + m.M) * m.nel;
  const size_t nvib = m.nvib;
  for (int row = 0; row < rows; ++row) {
    const int r = row / m.nel, a = row % m.nel;
    for (int g0 = 0; g0 < G; g0 += GROUPS) {
      const int g = g0 + q, n = g * LVC_TILE + t;
      double acc[LVC_OBS_NV];
#pragma unroll
      for (int v = 0; v < LVC_OBS_NV; ++v) acc[v] = 0.0;
      if (g < G && n < m.nvib) lvc_obs_point(m, r, a, n, [&](int b, int idx) { return st[b * nvib + idx]; }, acc);
      const double s = lvc_obs_tile_sum(acc, sh_wave + q * 4 * LVC_OBS_NV);
      if (g < G && t < LVC_OBS_NV) sh_tile[g * LVC_OBS_NV + t] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < LVC_OBS_NV) {
      const int v = threadIdx.x;
      const bool nbar = v == 2 * LVC_MAX_NEL && r > 0;
      if (v < 2 * m.nel || nbar) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += sh_tile[g * LVC_OBS_NV + v];
        if (nbar) sh_nb[(r - 1) * m.nel + a] = s;
        else rec[lvc_obs_slot(m.nel, r, a, v)] = s;
      }
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < m.M) {
    double s = 0.0;
    for (int a = 0; a < m.nel; ++a) s += sh_nb[threadIdx.x * m.nel + a];
    rec[2 * (m.nel * m.nel * (1 + m.M) + threadIdx.x)] = s;
    rec[2 * (m.nel * m.nel * (1 + m.M) + threadIdx.x) + 1] = 0.0;
  }
}

// ---------------------------------------------------------------- resident path
// The whole qd_lvc_rk4 call of member blockIdx.x: grid (B), LVC_RES_TPB threads, dynamic LDS as LvcPlan::lds_* lay it
// out.  Thread t owns the vibrational points t, t + LVC_RES_TPB, ... (at most KP, nvib <= LVC_RESIDENT_MAX_D / NEL).
// Stage s reads one LDS vector and writes the other: psi in A, stage 0 A -> B, 1 B -> A, 2 A -> B, 3 B -> A, so the
// new state is in A (and in the registers) when the step ends.
template <int NEL>
__global__ __launch_bounds__(LVC_RES_TPB) void lvc_resident_kernel(LvcDev m, LvcLds L, const c128* __restrict__ Hel,
                                                                   const c128* __restrict__ W, c128* psi_g, double dt,
                                                                   int nsteps, int save_every, int nsave,
                                                                   c128* __restrict__ snap, double* __restrict__ obs,
                                                                   int nobs) {
  constexpr int KP = (int)((((LVC_RESIDENT_MAX_D + NEL - 1) / NEL) + LVC_RES_TPB - 1) / LVC_RES_TPB);
  extern __shared__ __attribute__((aligned(16))) char lvc_smem[];
  c128* A = (c128*)lvc_smem;
  c128* Bv = (c128*)(lvc_smem + L.vec1);
  c128* tab = (c128*)(lvc_smem + L.tab);
  double* sh_wave = (double*)(lvc_smem + L.wave);
  double* sh_tile = (double*)(lvc_smem + L.tile);
  double* sh_nb = (double*)(lvc_smem + L.nbar);
  const size_t nvib = m.nvib;
  c128* psi = psi_g + (size_t)blockIdx.x * m.D;
  double* orec = obs ? obs + (size_t)blockIdx.x * (nsave + 1) * nobs * 2 : nullptr;
  lvc_load_tables(tab, Hel, W, NEL, m.M);
  c128 base[KP][NEL];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int n = threadIdx.x + k * LVC_RES_TPB;
#pragma unroll
    for (int a = 0; a < NEL; ++a) {
      base[k][a] = n < m.nvib ? psi[a * nvib + n] : cmk(0, 0);
      if (n < m.nvib) A[a * nvib + n] = base[k][a];
    }
  }
  __syncthreads();
  if (orec) lvc_obs_resident(m, A, sh_wave, sh_tile, sh_nb, orec);
  for (int s = 0; s < nsteps; ++s) {
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
      const c128* src = (stage & 1) ? Bv : A;
      c128* dst = (stage & 1) ? A : Bv;
      const double coef = rk4_horner_coef(dt, stage);
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const int n = threadIdx.x + k * LVC_RES_TPB;
        if (n < m.nvib) {
          c128 v[NEL], y[NEL];
          lvc_point<NEL>(m, tab, n, [&](int b, int idx) { return src[b * nvib + idx]; }, v, y);
#pragma unroll
          for (int a = 0; a < NEL; ++a) {
            const c128 o = cadd(base[k][a], cscale(cmulmi(y[a]), coef));
            dst[a * nvib + n] = o;
            if (stage == 3) base[k][a] = o;
          }
        }
      }
      __syncthreads();
    }
    if (save_every > 0 && (s + 1) % save_every == 0) {
      const int idx = (s + 1) / save_every;
      if (snap) {
        c128* out = snap + ((size_t)blockIdx.x * nsave + idx - 1) * m.D;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          const int n = threadIdx.x + k * LVC_RES_TPB;
          if (n < m.nvib) {
#pragma unroll
            for (int a = 0; a < NEL; ++a) out[a * nvib + n] = base[k][a];
          }
        }
      }
      if (orec) lvc_obs_resident(m, A, sh_wave, sh_tile, sh_nb, orec + (size_t)idx * nobs * 2);
    }
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int n = threadIdx.x + k * LVC_RES_TPB;
    if (n < m.nvib) {
#pragma unroll
      for (int a = 0; a < NEL; ++a) psi[a * nvib + n] = base[k][a];
    }
  }
}

// ---------------------------------------------------------------- laser-driven runs (qd_lvc_driven_rk4)
// H(t) = H0 - sum_d f_d(t) mu_d, mu_d = A_d (x) 1 or A_d (x) x_j, is the same stencil with the tables
//   Hel(t) = Hel - sum_{d: mode -1} f_d A_d,   W[j](t) = W[j] - sum_{d: mode j} f_d A_d,
// so every kernel below is its undriven counterpart with lvc_load_tables_driven in place of lvc_load_tables and the
// same lvc_point.  f is one row of fvals in device memory, read when the kernel runs.

// byte offsets of the driven resident kernel's LDS regions (LvcDrivePlan::lds_*)
struct LvcDriveLds {
  unsigned vec1, tab, eff, drv, wave, tile, nbar;
};

// The effective tables of one field row into LDS (the caller synchronises): entry e of table r = e / nel^2 is
// base[e] - sum_{d: mode[d] == r - 1} f[d] A[d][e % nel^2], the drives subtracted in the order d = 0, 1, ... without
// contraction.  base is Hel then W ([(1 + M) nel^2], global or LDS), A [nd][nel^2] (global or LDS).  A thread builds
// the entries e = t, t + blockDim.x, ...; dr.mode and f[d] are wave-uniform reads (kernel argument, scalar load).
__device__ __forceinline__ void lvc_load_tables_driven(c128* tab, const c128* base_hel, const c128* base_w,
                                                       const c128* A, const LvcDrive& dr, const c128* __restrict__ f,
                                                       int nel, int M) {
#pragma clang fp contract(off)
  const int nn = nel * nel;
  for (int e = threadIdx.x; e < (1 + M) * nn; e += blockDim.x) {
    const int r = e / nn, q = e - r * nn;
    c128 s = r == 0 ? base_hel[q] : base_w[e - nn];
    for (int d = 0; d < dr.nd; ++d) {
      if (dr.mode[d] != r - 1) continue;
      const c128 fd = f[d], a = A[d * nn + q];
      const double pr = fd.re * a.re - fd.im * a.im, pi = fd.re * a.im + fd.im * a.re;
      s.re = s.re - pr;
      s.im = s.im - pi;
    }
    tab[e] = s;
  }
}

// lvc_stage_kernel with the tables of the field row f: one Horner stage out = base + coef (-iH_f) v of B states.
// grid (ceil(nvib / LVC_TILE), B), LVC_TILE threads, dynamic LDS (1 + M) NEL^2 c128.  Aliasing as lvc_stage_kernel.
template <int NEL>
__global__ __launch_bounds__(LVC_TILE) void lvc_stage_driven_kernel(LvcDev m, LvcDrive dr, const c128* __restrict__ Hel,
                                                                    const c128* __restrict__ W,
                                                                    const c128* __restrict__ A,
                                                                    const c128* __restrict__ f, const c128* v_g,
                                                                    const c128* base_g, c128* out_g, double coef) {
  extern __shared__ __attribute__((aligned(16))) char lvc_smem[];
  c128* tab = (c128*)lvc_smem;
  lvc_load_tables_driven(tab, Hel, W, A, dr, f, NEL, m.M);
  __syncthreads();
  const int n = blockIdx.x * LVC_TILE + threadIdx.x;
  if (n >= m.nvib) return;
  const size_t off = (size_t)blockIdx.y * m.D;
  const c128* vin = v_g + off;
  const size_t nvib = m.nvib;
  c128 v[NEL], y[NEL];
  lvc_point<NEL>(m, tab, n, [&](int b, int idx) { return vin[b * nvib + idx]; }, v, y);
#pragma unroll
  for (int a = 0; a < NEL; ++a) {
    const size_t e = off + a * nvib + n;
    out_g[e] = cadd(base_g[e], cscale(cmulmi(y[a]), coef));
  }
}

// One classical RK4 stage with the tables of the field row f: k = -iH_f v, out = base + c_out k (skipped when out is
// null: the last stage), acc = acc_in + c_acc k.  acc_in is base in stage 0; acc may be acc_in, and in the last stage
// acc is psi itself: a thread reads and writes only its own elements of an aliased buffer.  v is aliased with nothing
// that is written.  Grid and LDS as lvc_stage_driven_kernel.
template <int NEL>
__global__ __launch_bounds__(LVC_TILE) void lvc_stage_rk4_kernel(LvcDev m, LvcDrive dr, const c128* __restrict__ Hel,
                                                                 const c128* __restrict__ W, const c128* __restrict__ A,
                                                                 const c128* __restrict__ f, const c128* v_g,
                                                                 const c128* base_g, const c128* acc_in_g, c128* out_g,
                                                                 c128* acc_g, double c_out, double c_acc) {
  extern __shared__ __attribute__((aligned(16))) char lvc_smem[];
  c128* tab = (c128*)lvc_smem;
  lvc_load_tables_driven(tab, Hel, W, A, dr, f, NEL, m.M);
  __syncthreads();
  const int n = blockIdx.x * LVC_TILE + threadIdx.x;
  if (n >= m.nvib) return;
  const size_t off = (size_t)blockIdx.y * m.D;
  const c128* vin = v_g + off;
  const size_t nvib = m.nvib;
  c128 v[NEL], y[NEL];
  lvc_point<NEL>(m, tab, n, [&](int b, int idx) { return vin[b * nvib + idx]; }, v, y);
#pragma unroll
  for (int a = 0; a < NEL; ++a) {
    const size_t e = off + a * nvib + n;
    const c128 k = cmulmi(y[a]);
    const c128 ai = acc_in_g[e];
    if (out_g) out_g[e] = cadd(base_g[e], cscale(k, c_out));
    acc_g[e] = cadd(ai, cscale(k, c_acc));
  }
}

// The whole qd_lvc_driven_rk4 call of member blockIdx.x: lvc_resident_kernel with the tables rebuilt in LDS from the
// base tables and the drive matrices (both copied to LDS once) whenever the field row changes, a barrier on each side
// of every rebuild.  grid (B), LVC_RES_TPB threads, dynamic LDS as LvcDrivePlan::lds_* lay it out.
//   SAMPLE 0 (hold): step s takes row s / hold (rebuilt when s % hold == 0); the Horner step of lvc_resident_kernel.
//   SAMPLE 1 (stage): classical RK4, the stages of step s take rows 2s, 2s + 1, 2s + 1, 2s + 2: rebuilt before stage 1
//   and before stage 3 (whose row is the next step's first), and once before the first step.  The stage vectors
//   ping-pong as in the Horner step (A -> B -> A -> B -> A); k1 .. k4 are summed into registers next to base:
//   acc = base + dt/6 k1 + dt/3 k2 + dt/3 k3, psi' = acc + dt/6 k4.
template <int NEL, int SAMPLE>
__global__ __launch_bounds__(LVC_RES_TPB) void lvc_resident_driven_kernel(
    LvcDev m, LvcDrive dr, LvcDriveLds L, const c128* __restrict__ Hel, const c128* __restrict__ W,
    const c128* __restrict__ Adrv, const c128* __restrict__ fvals, int hold, c128* psi_g, double dt, int nsteps,
    int save_every, int nsave, c128* __restrict__ snap, double* __restrict__ obs, int nobs) {
  constexpr int KP = (int)((((LVC_DRIVE_RESIDENT_MAX_D + NEL - 1) / NEL) + LVC_RES_TPB - 1) / LVC_RES_TPB);
  extern __shared__ __attribute__((aligned(16))) char lvc_smem[];
  c128* A = (c128*)lvc_smem;
  c128* Bv = (c128*)(lvc_smem + L.vec1);
  c128* tab0 = (c128*)(lvc_smem + L.tab);
  c128* tab = (c128*)(lvc_smem + L.eff);
  c128* drv = (c128*)(lvc_smem + L.drv);
  double* sh_wave = (double*)(lvc_smem + L.wave);
  double* sh_tile = (double*)(lvc_smem + L.tile);
  double* sh_nb = (double*)(lvc_smem + L.nbar);
  const size_t nvib = m.nvib;
  constexpr int NN = NEL * NEL;
  c128* psi = psi_g + (size_t)blockIdx.x * m.D;
  double* orec = obs ? obs + (size_t)blockIdx.x * (nsave + 1) * nobs * 2 : nullptr;
  lvc_load_tables(tab0, Hel, W, NEL, m.M);
  for (int e = threadIdx.x; e < dr.nd * NN; e += blockDim.x) drv[e] = Adrv[e];
  // the tables of row `row`; every thread calls it
  auto rebuild = [&](int row) {
    __syncthreads();
    lvc_load_tables_driven(tab, tab0, tab0 + NN, drv, dr, fvals + (size_t)row * dr.nd, NEL, m.M);
    __syncthreads();
  };
  c128 base[KP][NEL];
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int n = threadIdx.x + k * LVC_RES_TPB;
#pragma unroll
    for (int a = 0; a < NEL; ++a) {
      base[k][a] = n < m.nvib ? psi[a * nvib + n] : cmk(0, 0);
      if (n < m.nvib) A[a * nvib + n] = base[k][a];
    }
  }
  __syncthreads();
  if (orec) lvc_obs_resident(m, A, sh_wave, sh_tile, sh_nb, orec);
  if (SAMPLE == 1 && nsteps > 0) rebuild(0);
  for (int s = 0; s < nsteps; ++s) {
    if (SAMPLE == 0 && s % hold == 0) rebuild(s / hold);
    c128 acc[SAMPLE == 1 ? KP : 1][NEL];
#pragma unroll
    for (int stage = 0; stage < 4; ++stage) {
      if (SAMPLE == 1 && (stage & 1)) rebuild(2 * s + (stage + 1) / 2);
      const c128* src = (stage & 1) ? Bv : A;
      c128* dst = (stage & 1) ? A : Bv;
      const double coef = SAMPLE == 1 ? (stage == 2 ? dt : stage == 3 ? dt / 6.0 : dt * 0.5) : rk4_horner_coef(dt, stage);
      const double cacc = stage == 0 ? dt / 6.0 : dt / 3.0;
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const int n = threadIdx.x + k * LVC_RES_TPB;
        if (n < m.nvib) {
          c128 v[NEL], y[NEL];
          lvc_point<NEL>(m, tab, n, [&](int b, int idx) { return src[b * nvib + idx]; }, v, y);
#pragma unroll
          for (int a = 0; a < NEL; ++a) {
            if constexpr (SAMPLE == 1) {
              const c128 kk = cmulmi(y[a]);
              const c128 o = cadd(stage == 3 ? acc[k][a] : base[k][a], cscale(kk, coef));
              if (stage < 3) acc[k][a] = cadd(stage == 0 ? base[k][a] : acc[k][a], cscale(kk, cacc));
              dst[a * nvib + n] = o;
              if (stage == 3) base[k][a] = o;
            } else {
              const c128 o = cadd(base[k][a], cscale(cmulmi(y[a]), coef));
              dst[a * nvib + n] = o;
              if (stage == 3) base[k][a] = o;
            }
          }
        }
      }
      __syncthreads();
    }
    if (save_every > 0 && (s + 1) % save_every == 0) {
      const int idx = (s + 1) / save_every;
      if (snap) {
        c128* out = snap + ((size_t)blockIdx.x * nsave + idx - 1) * m.D;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          const int n = threadIdx.x + k * LVC_RES_TPB;
          if (n < m.nvib) {
#pragma unroll
            for (int a = 0; a < NEL; ++a) out[a * nvib + n] = base[k][a];
          }
        }
      }
      if (orec) lvc_obs_resident(m, A, sh_wave, sh_tile, sh_nb, orec + (size_t)idx * nobs * 2);
    }
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) {
    const int n = threadIdx.x + k * LVC_RES_TPB;
    if (n < m.nvib) {
#pragma unroll
      for (int a = 0; a < NEL; ++a) psi[a * nvib + n] = base[k][a];
    }
  }
}

}  // namespace qd
