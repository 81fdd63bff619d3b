// cgemm_block.hpp — workgroup-level complex-fp64 GEMM engine on
// v_mfma_f64_16x16x4_f64 (gfx950), used by the density-matrix kernels.
//
// One 512-thread workgroup (8 waves, 2 per SIMD) computes a BT x BT complex
// output block as a sum of "segments"  sum_s A_s[BT x K] * B_s[K x BT],
// with A_s, B_s row-major complex128 in global memory (L2/MALL resident).
//
// Data path per K-tile of 16 complex columns:
//   global --(16-B coalesced loads, register prefetch of tile t+1)--> LDS
//   (A tile row stride 18 complex: conflict-free ds_write_b128 staging and
//    ds_read_b128 fragment reads; B tile stride BT: natural and conflict-free)
//   LDS --(one complex = one ds_read_b128 per lane)--> MFMA fragments.
// (The Lindblad batch kernel's GEMMs stage with global_load_lds instead and use 3-product complex MACs:
// cgemm_dma128.hpp.)
// A complex 16x16x4 MAC is 4 real f64 MFMAs:
//   Cr += Ar*Br ; Cr += (-Ai)*Bi ; Ci += Ar*Bi ; Ci += Ai*Br
// f64 MFMA operand / result maps (cdna_hip_programming.md §3):
//   A: lane l holds A[l&15][k=l>>4];  B: lane l holds B[k=l>>4][l&15]
//   D: 4 regs/lane, reg r = D[row=(l>>4)+4r][col=l&15]
#pragma once
#include "qd_common.hpp"

namespace qd {

constexpr int CG_WG = 512;       // threads per workgroup
constexpr int CG_KT = 16;        // complex K per LDS stage
constexpr int CG_SA = CG_KT + 2; // padded A-tile row stride (complex)

template <int BT> struct CgCfg;
// BT x BT block; wave grid WR x WC; each wave owns MW x NW MFMA tiles (16x16).
template <> struct CgCfg<128> { static constexpr int MW = 2, NW = 4, WR = 4, WC = 2; };
template <> struct CgCfg<64>  { static constexpr int MW = 1, NW = 2, WR = 4, WC = 2; };
template <> struct CgCfg<32>  { static constexpr int MW = 1, NW = 1, WR = 2, WC = 2; };

struct CgSeg {
  const c128* A;  // points at A[block_row0][0], leading dim lda
  const c128* B;  // points at B[0][block_col0], leading dim ldb
};

template <int BT>
struct CgLds {
  c128 a[2][BT * CG_SA];
  c128 b[2][CG_KT * BT];
};

template <int BT>
struct CgAcc {
  static constexpr int MW = CgCfg<BT>::MW, NW = CgCfg<BT>::NW;
  d4 re[MW][NW];
  d4 im[MW][NW];
};

// Number of complex elements per thread for one A (or B) tile.
template <int BT> constexpr int cg_nld() { return (BT * CG_KT) / CG_WG; }

// Staging registers are plain 16-B vectors and the loads go through an explicit
// global (address space 1) pointer: global_load_dwordx4 that stay in flight
// across the MFMA work of the current tile (no flat loads, no scratch round trip).
typedef double cg_v2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) cg_v2 cg_gv2;

__device__ __forceinline__ cg_v2 cg_ld(const c128* p) {
  return *(cg_gv2*)(p);  // generic -> global address-space cast (the pointer is a global buffer)
}
__device__ __forceinline__ void cg_st_lds(c128* p, cg_v2 v) { *reinterpret_cast<cg_v2*>(p) = v; }

#ifndef CG_STAGE_AT
#define CG_STAGE_AT 3  // k-step (of 4) before which the next tile's LDS stores are issued (4 = after compute)
#endif

__device__ __forceinline__ void cg_sched_fence() { __builtin_amdgcn_sched_barrier(0); }   // nothing moves across it

template <int BT>
__device__ __forceinline__ void cg_zero(CgAcc<BT>& acc) {
#pragma unroll
  for (int mi = 0; mi < CgAcc<BT>::MW; ++mi)
#pragma unroll
    for (int nj = 0; nj < CgAcc<BT>::NW; ++nj) {
      acc.re[mi][nj] = d4{0.0, 0.0, 0.0, 0.0};
      acc.im[mi][nj] = d4{0.0, 0.0, 0.0, 0.0};
    }
}

struct CgNoMid {
  __device__ __forceinline__ void operator()() const {}
};

// One K-tile of MFMA work from LDS buffer `buf`.  `mid()` runs before k-step CG_STAGE_AT: the caller puts
// the next tile's LDS stores there, so they issue while this tile's MFMAs are still in the pipe instead
// of between the last MFMA and the barrier (the double buffer keeps the two tiles apart).
// PIPE: the fragments of k-step q+1 are read from LDS into a second register set before the MFMAs
// of k-step q issue, so only the tile's first k-step waits on LDS latency (without it every k-step's
// first MFMA waits for its ds_read_b128s: the reads reuse the registers the previous MFMAs consume).
template <int BT, bool PIPE = false, typename Mid = CgNoMid>
__device__ __forceinline__ void cg_compute_tile(const CgLds<BT>& L, int buf, CgAcc<BT>& acc, int wr0, int wc0,
                                                Mid mid = Mid()) {
  constexpr int MW = CgCfg<BT>::MW, NW = CgCfg<BT>::NW;
  constexpr int NQ = CG_KT / 4;
  const int lane = threadIdx.x & 63;
  const int lr = lane & 15, lk = lane >> 4;
  constexpr int NS = PIPE ? 2 : 1;
  c128 a[NS][MW], b[NS][NW];
  auto frag = [&](int q, int slot) {
    const int kk = 4 * q;
#pragma unroll
    for (int mi = 0; mi < MW; ++mi) a[slot][mi] = L.a[buf][(wr0 + mi * 16 + lr) * CG_SA + kk + lk];
#pragma unroll
    for (int nj = 0; nj < NW; ++nj) b[slot][nj] = L.b[buf][(kk + lk) * BT + wc0 + nj * 16 + lr];
  };
  if (PIPE) frag(0, 0);
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (q == CG_STAGE_AT) {
      // keep the staging stores (and the vmcnt wait for their data) behind the MFMAs already issued:
      // without the fence the scheduler hoists them above the tile's MFMAs
      cg_sched_fence();
      mid();
      cg_sched_fence();
    }
    const int cs = PIPE ? (q & 1) : 0;
    if (PIPE) {
      if (q + 1 < NQ) frag(q + 1, (q + 1) & 1);
    } else {
      frag(q, 0);
    }
#pragma unroll
    for (int mi = 0; mi < MW; ++mi)
#pragma unroll
      for (int nj = 0; nj < NW; ++nj) {
        acc.re[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cs][mi].re, b[cs][nj].re, acc.re[mi][nj], 0, 0, 0);
        acc.im[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cs][mi].re, b[cs][nj].im, acc.im[mi][nj], 0, 0, 0);
      }
#pragma unroll
    for (int mi = 0; mi < MW; ++mi)
#pragma unroll
      for (int nj = 0; nj < NW; ++nj) {
        acc.re[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[cs][mi].im, b[cs][nj].im, acc.re[mi][nj], 0, 0, 0);
        acc.im[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[cs][mi].im, b[cs][nj].re, acc.im[mi][nj], 0, 0, 0);
      }
  }
  if (CG_STAGE_AT >= NQ) {
    cg_sched_fence();
    mid();
  }
}

// Generic engine: T K-tiles; the operand tiles come from two policies with
//   Raw fetch(int t, int e, int q)           issued one tile ahead (global loads in flight during MFMA)
//   cg_v2 finish(const Raw&, int t, int e, int q)  run just before the LDS store (after the MFMA work)
// where e = tid + CG_WG*q is the element of the tile this thread stages (A: row e>>4, col e&15;
// B: row e/BT, col e%BT) and q < cg_nld<BT>() its compile-time slot.  A policy may fetch inputs and compute the operand in finish (generated operands).
// All threads of the workgroup must call it.  Ends with a workgroup barrier.
// zero = false accumulates onto acc (segment lists longer than an LDS table, run in chunks).
template <int BT, bool PIPE = false, typename APol, typename BPol>
__device__ __forceinline__ void cg_block_gemm_gen(int T, APol& pa, BPol& pb, CgLds<BT>& L, CgAcc<BT>& acc,
                                                  bool zero = true) {
  constexpr int MW = CgCfg<BT>::MW, NW = CgCfg<BT>::NW, WC = CgCfg<BT>::WC, WR = CgCfg<BT>::WR;
  const int wave = threadIdx.x >> 6;
  const bool active = wave < WR * WC;
  const int wr0 = (wave / WC) * (MW * 16);
  const int wc0 = (wave % WC) * (NW * 16);
  if (zero) cg_zero(acc);
  constexpr int NLD = cg_nld<BT>();
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // staging address math stays per call (see cg_epilogue)
  typename APol::Raw ra[NLD];
  typename BPol::Raw rb[NLD];
  auto load = [&](int t) {
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = tid + CG_WG * q;
      ra[q] = pa.fetch(t, e, q);
      rb[q] = pb.fetch(t, e, q);
    }
  };
  auto store = [&](int t, int buf) {
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = tid + CG_WG * q;
      cg_st_lds(&L.a[buf][(e >> 4) * CG_SA + (e & 15)], pa.finish(ra[q], t, e, q));
      cg_st_lds(&L.b[buf][e], pb.finish(rb[q], t, e, q));
    }
  };
  load(0);
  store(0, 0);
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const bool more = (t + 1) < T;
    if (more) load(t + 1);
    auto mid = [&]() {
      if (more) store(t + 1, (t + 1) & 1);
    };
    if (active) {
      cg_compute_tile<BT, PIPE>(L, t & 1, acc, wr0, wc0, mid);
    } else {
      mid();
    }
    __syncthreads();
  }
}

// The same engine with the global loads issued two K-tiles ahead (two register sets, loop unrolled by two so
// the set index is a compile-time constant): a tile's loads have two tiles of MFMA work to arrive instead of
// three k-steps, for blocks whose MFMA time per K-tile is short (BT = 64: 1.9 us per tile per SIMD) next to
// the fabric latency of operands served from the Infinity Cache.  Same results as cg_block_gemm_gen
// (identical MFMA order).
template <int BT, bool PIPE = false, typename APol, typename BPol>
__device__ __forceinline__ void cg_block_gemm_gen2(int T, APol& pa, BPol& pb, CgLds<BT>& L, CgAcc<BT>& acc) {
  constexpr int MW = CgCfg<BT>::MW, NW = CgCfg<BT>::NW, WC = CgCfg<BT>::WC, WR = CgCfg<BT>::WR;
  const int wave = threadIdx.x >> 6;
  const bool active = wave < WR * WC;
  const int wr0 = (wave / WC) * (MW * 16);
  const int wc0 = (wave % WC) * (NW * 16);
  // cg_zero(acc), written out: through the helper the split kernels and the 2DES 64-block GEMM schedule a few
  // instructions in another order (tools/isa_diff.py against the build before)
#pragma unroll
  for (int mi = 0; mi < MW; ++mi)
#pragma unroll
    for (int nj = 0; nj < NW; ++nj) {
      acc.re[mi][nj] = d4{0.0, 0.0, 0.0, 0.0};
      acc.im[mi][nj] = d4{0.0, 0.0, 0.0, 0.0};
    }
  constexpr int NLD = cg_nld<BT>();
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  typename APol::Raw ra[2][NLD];
  typename BPol::Raw rb[2][NLD];
  auto load = [&](int t, auto slot) {
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = tid + CG_WG * q;
      ra[slot()][q] = pa.fetch(t, e, q);
      rb[slot()][q] = pb.fetch(t, e, q);
    }
  };
  auto store = [&](int t, int buf, auto slot) {
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = tid + CG_WG * q;
      cg_st_lds(&L.a[buf][(e >> 4) * CG_SA + (e & 15)], pa.finish(ra[slot()][q], t, e, q));
      cg_st_lds(&L.b[buf][e], pb.finish(rb[slot()][q], t, e, q));
    }
  };
  struct S0 { constexpr int operator()() const { return 0; } };
  struct S1 { constexpr int operator()() const { return 1; } };
  load(0, S0{});
  if (T > 1) load(1, S1{});
  store(0, 0, S0{});
  __syncthreads();
  // iteration t: tile t+1 sits in register set (t+1)&1 and goes to LDS during tile t's MFMAs; tile t+2 is
  // loaded into set t&1 (tile t left it at iteration t-1)
  auto step = [&](int t, auto cur, auto nxt) {
    if (t + 2 < T) load(t + 2, cur);
    const bool more = (t + 1) < T;
    auto mid = [&]() {
      if (more) store(t + 1, (t + 1) & 1, nxt);
    };
    if (active) {
      cg_compute_tile<BT, PIPE>(L, t & 1, acc, wr0, wc0, mid);
    } else {
      mid();
    }
    __syncthreads();
  };
  int t = 0;
  for (; t + 1 < T; t += 2) {
    step(t, S0{}, S1{});
    step(t + 1, S1{}, S0{});
  }
  if (t < T) step(t, S0{}, S1{});
}

// Policies that read row-major complex tiles from memory through segment tables in LDS.
template <int BT>
struct CgSegA {
  using Raw = cg_v2;
  const CgSeg* segs;
  int tps, lda;
  __device__ __forceinline__ Raw fetch(int t, int e, int) const {
    const CgSeg sg = segs[t / tps];
    return cg_ld(sg.A + (size_t)(e >> 4) * lda + (t % tps) * CG_KT + (e & 15));
  }
  __device__ __forceinline__ cg_v2 finish(const Raw& r, int, int, int) const { return r; }
};
template <int BT>
struct CgSegB {
  using Raw = cg_v2;
  const CgSeg* segs;
  int tps, ldb;
  __device__ __forceinline__ Raw fetch(int t, int e, int) const {
    const CgSeg sg = segs[t / tps];
    return cg_ld(sg.B + (size_t)((t % tps) * CG_KT + e / BT) * ldb + (e % BT));
  }
  __device__ __forceinline__ cg_v2 finish(const Raw& r, int, int, int) const { return r; }
};

// Accumulate sum_s A_s * B_s over nseg segments of depth K (K % 16 == 0) into
// a zero-initialised accumulator.  All threads of the workgroup must call it.
// `segs` should live in LDS (or be uniform): it is indexed at run time, and a
// private array indexed at run time would be placed in scratch memory.
// Ends with a workgroup barrier, so LDS may be reused immediately after.
template <int BT, bool PIPE = false>
__device__ __forceinline__ void cg_block_gemm(const CgSeg* segs, int nseg, int K, int lda, int ldb, CgLds<BT>& L,
                                              CgAcc<BT>& acc, bool zero = true) {
  const int tps = K / CG_KT;
  CgSegA<BT> pa{segs, tps, lda};
  CgSegB<BT> pb{segs, tps, ldb};
  cg_block_gemm_gen<BT, PIPE>(nseg * tps, pa, pb, L, acc, zero);
}

// ---------------------------------------------------------------- X GEMM of the Hermitian 128-kernel, quadrant layout
// The plain X GEMM (every tile takes every segment) of the register-staged Hermitian kernel at BT = 128
// (glf_kernel.hpp: Redfield's GLF operands, and the CHUNK kernels).  Arithmetic and K-tile pipeline of
// cg_block_gemm<128> on another tile -> wave map: wave w owns row tiles i and 4 + i and column tiles
// {2h, 2h+1, 4+2h, 5+2h}, i = w / 2, h = w % 2, two 16 x 16 tiles in each 64 x 64 quadrant of the block.
struct CgQuadLayout {
  static __device__ __forceinline__ int row0(int wave, int mi) { return mi * 64 + (wave >> 1) * 16; }
  static __device__ __forceinline__ int col0(int wave, int nj) { return (nj >> 1) * 64 + (2 * (wave & 1) + (nj & 1)) * 16; }
};

// cg_compute_tile<128> on the quadrant layout
template <typename Mid>
__device__ __forceinline__ void cg_quad_compute_tile(const CgLds<128>& L, int buf, CgAcc<128>& acc, int wave, Mid mid) {
  constexpr int BT = 128, MW = 2, NW = 4, NQ = CG_KT / 4;
  const int lane = threadIdx.x & 63;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (q == CG_STAGE_AT) {
      cg_sched_fence();
      mid();
      cg_sched_fence();
    }
    const int kk = 4 * q;
    c128 a[MW], b[NW];
#pragma unroll
    for (int mi = 0; mi < MW; ++mi) a[mi] = L.a[buf][(CgQuadLayout::row0(wave, mi) + lr) * CG_SA + kk + lk];
#pragma unroll
    for (int nj = 0; nj < NW; ++nj) b[nj] = L.b[buf][(kk + lk) * BT + CgQuadLayout::col0(wave, nj) + lr];
#pragma unroll
    for (int mi = 0; mi < MW; ++mi)
#pragma unroll
      for (int nj = 0; nj < NW; ++nj) {
        acc.re[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi].re, b[nj].re, acc.re[mi][nj], 0, 0, 0);
        acc.im[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi].re, b[nj].im, acc.im[mi][nj], 0, 0, 0);
      }
#pragma unroll
    for (int mi = 0; mi < MW; ++mi)
#pragma unroll
      for (int nj = 0; nj < NW; ++nj) {
        acc.re[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[mi].im, b[nj].im, acc.re[mi][nj], 0, 0, 0);
        acc.im[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi].im, b[nj].re, acc.im[mi][nj], 0, 0, 0);
      }
  }
  if (CG_STAGE_AT >= NQ) {
    cg_sched_fence();
    mid();
  }
}

// cg_block_gemm<128> on the quadrant layout: sum_s A_s B_s over nseg segments of depth K (tps = K / 16 K-tiles per
// segment); zero = false accumulates onto acc (chunked segment lists).  All threads call it; ends with a workgroup
// barrier.  Visit the result with cg_quad_epilogue.
__device__ __forceinline__ void cg_quad_x_gemm(const CgSeg* segs, int nseg, int K, int lda, int ldb, CgLds<128>& L,
                                               CgAcc<128>& acc, bool zero = true) {
  constexpr int BT = 128;
  const int wave = threadIdx.x >> 6;
  if (zero) cg_zero(acc);
  const int tps = K / CG_KT, T = nseg * tps;
  CgSegA<BT> pa{segs, tps, lda};
  CgSegB<BT> pb{segs, tps, ldb};
  constexpr int NLD = cg_nld<BT>();
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  cg_v2 ra[NLD], rb[NLD];
  auto load = [&](int t) {
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = tid + CG_WG * q;
      ra[q] = pa.fetch(t, e, q);
      rb[q] = pb.fetch(t, e, q);
    }
  };
  auto store = [&](int t, int buf) {
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int e = tid + CG_WG * q;
      cg_st_lds(&L.a[buf][(e >> 4) * CG_SA + (e & 15)], ra[q]);
      cg_st_lds(&L.b[buf][e], rb[q]);
    }
  };
  load(0);
  store(0, 0);
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const bool more = (t + 1) < T;
    if (more) load(t + 1);
    auto mid = [&]() {
      if (more) store(t + 1, (t + 1) & 1);
    };
    cg_quad_compute_tile(L, t & 1, acc, wave, mid);
    __syncthreads();
  }
}

template <typename F>
__device__ __forceinline__ void cg_quad_epilogue(const CgAcc<128>& acc, F&& f) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int nj = 0; nj < 4; ++nj) {
        const int row = CgQuadLayout::row0(wave, mi) + (lane >> 4) + 4 * r;
        const int col = CgQuadLayout::col0(wave, nj) + (lane & 15);
        f(row, col, cmk(acc.re[mi][nj][r], acc.im[mi][nj][r]));
      }
}

// Visit every accumulator element: f(row, col, value) with row/col inside the block.
template <int BT, typename F>
__device__ __forceinline__ void cg_epilogue(const CgAcc<BT>& acc, F&& f) {
  constexpr int MW = CgCfg<BT>::MW, NW = CgCfg<BT>::NW, WC = CgCfg<BT>::WC, WR = CgCfg<BT>::WR;
  // The thread index goes through an empty asm so the compiler cannot hoist the per-element
  // address math of an epilogue out of a persistent kernel's step loop (it would spill it).
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int wave = tid >> 6;
  if (wave >= WR * WC) return;
  const int lane = tid & 63;
  const int wr0 = (wave / WC) * (MW * 16);
  const int wc0 = (wave % WC) * (NW * 16);
#pragma unroll
  for (int mi = 0; mi < MW; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int nj = 0; nj < NW; ++nj) {
        const int row = wr0 + mi * 16 + (lane >> 4) + 4 * r;
        const int col = wc0 + nj * 16 + (lane & 15);
        f(row, col, cmk(acc.re[mi][nj][r], acc.im[mi][nj][r]));
      }
}

}  // namespace qd
