// glf_herm_k.hpp — the stage epilogue of the persistent Hermitian kernels at Np = 128 on the Hermitian tile layout
// (cgemm_dma128.hpp): k = X + X^+ formed in the registers of the wave that owns the upper element, with one trip of
// the lower elements through LDS and one barrier ahead of the Horner update (HermKL, herm_k_publish, herm_k_update),
// and the workgroup's observables without a VGPR held across the K loops.  The Lindblad batch kernel
// (glf_batch_kernel.hpp) uses all of it; lindblad_eig_jump_kernel (glf_eig_jump_kernel.hpp), which forms k inside its
// GEMM, takes wave_uniform and the observables.  Each in a translation unit of its own.
#pragma once
#include "cgemm_dma128.hpp"
#include "glf_kernel.hpp"

namespace qd {
namespace {

// A double every lane holds alike, moved to scalar registers.
__device__ __forceinline__ double wave_uniform(double v) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// wg_observables (glf_kernel.hpp) for this kernel: the same per-thread partials, wave butterfly and 8-wave sum, bit
// for bit, with the butterfly's partner taken from the laundered thread index.  __shfl_xor's own lane id is hoisted
// out of the step loop and then holds a VGPR across every K loop, and this kernel has none to spare.
__device__ __forceinline__ double lane_xor(double v, int lane, int off) {
  const int a = (lane ^ off) << 2;
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_ds_bpermute(a, (int)(unsigned)u);
  const unsigned hi = __builtin_amdgcn_ds_bpermute(a, (int)(unsigned)(u >> 32));
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void wg_observables_batch(const c128* rho, const c128* eT, int ne, size_t NN, c128* out,
                                                     c128* sred) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, wave = tid >> 6;
  for (int m = 0; m < ne; ++m) {
    const c128* e = eT + (size_t)m * NN;
    double sr = 0.0, si = 0.0;
    for (size_t i = tid; i < NN; i += CG_WG) {
      c128 r = rho[i], x = e[i];
      sr += r.re * x.re - r.im * x.im;
      si += r.re * x.im + r.im * x.re;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sr += lane_xor(sr, lane, off);
      si += lane_xor(si, lane, off);
    }
    if (lane == 0) sred[wave] = cmk(sr, si);
    __syncthreads();
    if (tid == 0) {
      c128 s = sred[0];
      for (int w = 1; w < CG_WG / 64; ++w) s = cadd(s, sred[w]);
      out[m] = s;
    }
    __syncthreads();
  }
}

// Tiles whose rho a wave loads ahead of the publishing barrier.  A wave owns four or five tiles on and above the
// diagonal: a fifth tile's rho is loaded behind the first tile's update, into the registers that tile frees (five
// tiles' rho next to five tiles' accumulators spilled).
constexpr int HERM_K_NPRE = 4;

// The LDS image of conj(X) below the diagonal, stored at the mirror position: what the owner of an upper element
// (i, j), i < j, adds to its own X_ij for k = X + X^+.  The 28 16 x 16 tiles above the diagonal take 256 slots each,
// element (ra, cc) at ra * 16 + (cc ^ ra): the XOR spreads the writer's 16 lanes (one column, rows 16 B * 16 apart)
// over 16 distinct 16-byte slots, and the reader's 16 lanes (one row) stay inside one 256-byte run.  The 8 diagonal
// tiles take 128 slots each, rows ra and 15 - ra of the strict upper triangle folded into one run of 16: slot
// 16 ra + cc for ra < 8, its complement in 255 for the rows below.
struct HermKL {
  static constexpr int DIAG0 = 28 * 256, SIZE = DIAG0 + 8 * 128;
  static constexpr int tile(int R, int C) { return (R * 8 - R * (R + 1) / 2 + (C - R - 1)) * 256; }   // R < C
  static __device__ __forceinline__ int slot(int ra, int cc) { return ra * 16 + (cc ^ ra); }
  static __device__ __forceinline__ int dslot(int ra, int cc) {                                       // ra < cc
    const int s = ra * 16 + cc;
    return s ^ (ra < 8 ? 0 : 255);
  }
};

// Wave W of the Hermitian tile layout (cgemm_dma128.hpp) publishes its accumulator elements below the diagonal into
// the HermKL image: whole tiles with R > C (the lower-left quadrant among them) and the ra > cc elements of diagonal
// tiles.  The wave's tile roles are compile-time constants: no per-element index arithmetic or branches outside the
// diagonal tiles.  The accumulators of the tiles below the diagonal die here.
template <int W>
__device__ __forceinline__ void herm_k_publish(const CgAcc<128>& A, c128* KL, int lane) {
  const int lr = lane >> 4, lc = lane & 15;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (W >> 1) : 7 - (W >> 1), C = cg_herm_ctile(W, nj);   // constants after unrolling
      if (R < C) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const c128 v = cmk(A.re[mi][nj][r], A.im[mi][nj][r]);
        const int ra = lr + 4 * r;
        if (R > C) KL[HermKL::tile(C, R) + HermKL::slot(lc, ra)] = cconj(v);
        else if (ra > lc) KL[HermKL::DIAG0 + R * 128 + HermKL::dslot(lc, ra)] = cconj(v);
      }
    }
}

// rho on the elements of wave W's tiles on and above the diagonal, in MFMA layout (q[mi * 4 + nj][r]; the entries of
// the tiles below the diagonal are never touched and take no registers).  Diagonal tiles load all 256 elements: no
// load sits in a branch, the values below the diagonal are discarded.  Every address is the matrix's base (scalar
// registers) plus a 32-bit byte offset, the lane's own plus a uniform one: no 64-bit address pair per element.
template <int W>
__device__ __forceinline__ void herm_k_rho_loads(const c128* rho, int Np, int lane, c128 (&q)[8][4], int N0, int N1) {
  const unsigned vu = (unsigned)((lane >> 4) * Np + (lane & 15)) * (unsigned)sizeof(c128);
  int n = 0;   // ordinal of the tile among the wave's tiles on and above the diagonal
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (W >> 1) : 7 - (W >> 1), C = cg_herm_ctile(W, nj);
      if (R > C) continue;
      if (n < N0 || n >= N1) { ++n; continue; }
      ++n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned su = (unsigned)((16 * R + 4 * r) * Np) * (unsigned)sizeof(c128);   // uniform
        q[mi * 4 + nj][r] = *reinterpret_cast<const c128*>(reinterpret_cast<const char*>(rho + 16 * C) + (vu + su));
      }
    }
}

// Behind the barrier that publishes the HermKL image: wave W reads the mirror's conjugate of each element of its
// tiles on and above the diagonal (a tile's four reads first, straight-line), forms k = X_ij + conj(X_ji) (v + conj(v)
// on the diagonal) and runs the Horner update rn_ij = rho_ij + hc k, writing the mirror rn_ji as the conjugate.
// Addresses as in herm_k_rho_loads: uniform bases, one per-lane offset for the elements and one for the mirrors.
template <int W, int NPRE>
__device__ __forceinline__ void herm_k_update(const CgAcc<128>& A, const c128* KL, int lane, c128 (&q)[8][4],
                                              const c128* rho, c128* rn, int Np, double hc) {
  const int lr = lane >> 4, lc = lane & 15;
  const unsigned vu = (unsigned)(lr * Np + lc) * (unsigned)sizeof(c128);
  const unsigned vm = (unsigned)(lc * Np + lr) * (unsigned)sizeof(c128);
  int n = 0;   // ordinal of the tile among the wave's tiles on and above the diagonal
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (W >> 1) : 7 - (W >> 1), C = cg_herm_ctile(W, nj);
      if (R > C) continue;
      if (n >= 1) {   // rho of tile n - 1 + NPRE into the registers tile n - 1 has just freed, used NPRE - 1 tiles on
        cg_sched_fence();
        herm_k_rho_loads<W>(rho, Np, lane, q, n - 1 + NPRE, n + NPRE);
        cg_sched_fence();
      }
      ++n;
      c128 m[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ra = lr + 4 * r;
        if (R < C) m[r] = KL[HermKL::tile(R, C) + HermKL::slot(ra, lc)];
        else m[r] = KL[HermKL::DIAG0 + R * 128 + HermKL::dslot(ra, lc)];   // ra >= lc: some slot of the tile, discarded
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const c128 x = cmk(A.re[mi][nj][r], A.im[mi][nj][r]);
        const int ra = lr + 4 * r;
        const c128 k = cadd(x, R == C && ra == lc ? cconj(x) : m[r]);
        const c128 v = cadd(q[mi * 4 + nj][r], cscale(k, hc));
        const unsigned su = (unsigned)((16 * R + 4 * r) * Np) * (unsigned)sizeof(c128);   // uniform, as sm
        const unsigned sm = (unsigned)(16 * C * Np) * (unsigned)sizeof(c128);
        char* u = reinterpret_cast<char*>(rn + 16 * C) + (vu + su);
        char* t = reinterpret_cast<char*>(rn + 16 * R + 4 * r) + (vm + sm);
        if (R < C || ra <= lc) *reinterpret_cast<c128*>(u) = v;
        if (R < C || ra < lc) *reinterpret_cast<c128*>(t) = cconj(v);
      }
    }
}

}  // namespace
}  // namespace qd
