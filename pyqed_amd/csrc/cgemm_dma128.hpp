// cgemm_dma128.hpp — the Lindblad batch kernels' GEMM engine (glf_batch_kernel.hpp, glf_eig_kernel.hpp): 128-blocks staged
// by 16-byte global_load_lds (no staging registers, no ds_write pass), 3-product complex MACs.
// An LDS-DMA load writes lane-linearly (wave base + lane * 16 B), so the A tile is [128 rows][16 k] without padding and
// the k index is XOR-ed with row & 15 on the per-lane SOURCE address and again in the fragment read: the 16 lanes of one
// ds_read_b128 group (rows r0 .. r0 + 15, one k) hit 16 distinct 16-byte slots.  The B tile keeps the [16 k][128] image.
// Tile t + 1's loads are issued at the top of tile t into the other buffer (the batch kernel's engines) or two at a time
// under tile t's first four half k-steps (glf_eig_kernel.hpp's engines: CgDmaStageHook); the __syncthreads() that ends
// a tile waits for them (vmcnt(0)).  A GEMM's last K-tile stages tile 0 of its follower (lookahead), whole or its B half
// alone; an A tile may instead come from a wave's registers in the same image (cg_dma_a_slot, the hand-overs at the end
// of this file), and so may a B tile (cg_dma_b_slot).  The 3-product MAC (3 MFMAs per complex k-step for the 4 of cg_compute_tile):
//   P1 += ar br ; P2 += ai bi ; P3 += (ar + ai)(br + bi) ;  re = P1 - P2, im = P3 - P1 - P2
// with P1 / P2 in the tile's re / im registers until cg_dma_finalise.
// Hermitian X GEMM: X = A r + sum_c B_c W_c (segment 0; segments >= 1, W = C^+ / 2) for k = X + X^+.  Only k on the
// upper triangle is used and B W (= C r C^+ / 2) is itself Hermitian, so the segments >= 1 skip the 16 x 16 tiles below
// the diagonal (there X = A r alone) and each tile above it takes the full C r C^+ instead of its half:
// k_ij = (A r)_ij + conj((A r)_ji) + (C r C^+)_ij for i < j; diagonal tiles keep the half in both triangles.  Tile
// layout (16-tiles R, C in 0..7): wave w = 2 i + h owns row tiles {i, 7 - i} and the column tiles cg_herm_ctile(w, .),
// placed so that each SIMD's two waves (w, w + 4) hold 9 of the 36 tiles with R <= C.
#pragma once
#include "cgemm_block.hpp"

namespace qd {

// Column tile nj of wave w, and the wave's tiles (bit mi * 4 + nj) below the diagonal (skipped in the Hermitian
// segments) / above it (which take those segments twice).
constexpr int cg_herm_ctile(int w, int nj) {
  constexpr unsigned short cols[8] = {0x3210, 0x7654, 0x7610, 0x5432, 0x7432, 0x6510, 0x5410, 0x7632};
  return (cols[w] >> (nj * 4)) & 15;
}
constexpr unsigned cg_herm_mask(int w, bool below) {
  unsigned m = 0;
  for (int mi = 0; mi < 2; ++mi)
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (w >> 1) : 7 - (w >> 1), C = cg_herm_ctile(w, nj);
      if (below ? R > C : R < C) m |= 1u << (mi * 4 + nj);
    }
  return m;
}

// CgAcc<128> with the third accumulator set of the 3-product form (tile index mi * 4 + nj)
struct CgAcc3 : CgAcc<128> { d4 p3[8]; };

typedef const __attribute__((address_space(1))) void cg_gvoid;
typedef __attribute__((address_space(3))) void cg_lvoid;

// A pointer every lane of the wave holds alike, as a scalar (the DMA loads then take an SGPR base + 32-bit lane offset).
__device__ __forceinline__ const char* cg_uniform(const void* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
}

// The A-tile image, written once: element (row, k) of a [128][16] K-tile, row = r0 + lr with r0 the row's 16-tile and
// lr = row & 15, sits at 16-byte slot row * 16 + (k ^ lr).  Its three users are the DMA source address (slot (row, s)
// is loaded from column cg_dma_a_kslot(lr, s): the XOR is its own inverse), the fragment read of cg_dma_ksteps, and a
// wave that writes an accumulator tile into the image from registers (cg_dma_a_tile_write).
constexpr int cg_dma_a_kslot(int lr, int k) { return k ^ lr; }
constexpr int cg_dma_a_slot(int r0, int lr, int k) { return (r0 + lr) * CG_KT + cg_dma_a_kslot(lr, k); }
constexpr bool cg_dma_a_slot_bijective() {   // 128 x 16 onto 0 .. 2047, and the source map undoes the slot map
  bool seen[128 * CG_KT] = {};
  for (int row = 0; row < 128; ++row)
    for (int k = 0; k < CG_KT; ++k) {
      const int s = cg_dma_a_slot(row & ~15, row & 15, k);
      if (s < 0 || s >= 128 * CG_KT || seen[s]) return false;
      if (cg_dma_a_kslot(row & 15, cg_dma_a_kslot(row & 15, k)) != k) return false;
      seen[s] = true;
    }
  return true;
}
constexpr bool cg_dma_a_slot_conflict_free() {   // the 16 lanes of one ds_read_b128 group (rows r0 .. r0 + 15, one k):
  for (int r0 = 0; r0 < 128; r0 += 16)           // 16 distinct slots, one in each 16-byte column of the 256-byte bank row
    for (int k = 0; k < CG_KT; ++k) {
      unsigned cols = 0;
      for (int lr = 0; lr < 16; ++lr) {
        const int s = cg_dma_a_slot(r0, lr, k);
        for (int l2 = 0; l2 < lr; ++l2)
          if (cg_dma_a_slot(r0, l2, k) == s) return false;
        cols |= 1u << (s & 15);
      }
      if (cols != 0xffffu) return false;
    }
  return true;
}
static_assert(cg_dma_a_slot_bijective(), "A-tile image: slots");
static_assert(cg_dma_a_slot_conflict_free(), "A-tile image: fragment read groups");

// The B-tile image, written once: element (k, col) of a [16][128] K-tile sits at 16-byte slot k * 128 + col, row-major
// as in memory.  Its users are the DMA (element e = tid + 512 q lands lane-linearly at slot e and is loaded from
// B[e / 128][e % 128]: cg_dma_b_k, cg_dma_b_col), the fragment read of cg_dma_ksteps, and a wave that writes rows of a
// result into the image from registers (eig_tail, glf_eig_kernel.hpp).
constexpr int cg_dma_b_slot(int k, int col) { return k * 128 + col; }
constexpr int cg_dma_b_k(int e) { return e >> 7; }
constexpr int cg_dma_b_col(int e) { return e & 127; }
constexpr bool cg_dma_b_slot_bijective() {   // 16 x 128 onto 0 .. 2047, and the DMA's source map undoes the slot map
  bool seen[128 * CG_KT] = {};
  for (int k = 0; k < CG_KT; ++k)
    for (int col = 0; col < 128; ++col) {
      const int s = cg_dma_b_slot(k, col);
      if (s < 0 || s >= 128 * CG_KT || seen[s]) return false;
      if (cg_dma_b_k(s) != k || cg_dma_b_col(s) != col) return false;
      seen[s] = true;
    }
  return true;
}
static_assert(cg_dma_b_slot_bijective(), "B-tile image: slots");

// Per-thread part of the staging addresses (bytes) and the wave's first element of each 512-element load round.
struct CgDmaStage {
  const CgSeg* segs;
  int tps, lda, ldb;
  unsigned offA, offB;
  int wbase;
  __device__ __forceinline__ CgDmaStage(const CgSeg* s, int tps_, int lda_, int ldb_) : segs(s), tps(tps_), lda(lda_), ldb(ldb_) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));  // staging address math stays per call (see cg_epilogue)
    // A: element e = tid + 512 q sits at LDS slot (row e >> 4, k-slot e & 15) and holds A[row][(e & 15) ^ (row & 15)]
    // (row & 15 = (tid >> 4) & 15 for every q);  B: element e -> B[e / 128][e % 128]
    const int row = tid >> 4;
    offA = (unsigned)(row * lda + cg_dma_a_kslot(row & 15, tid & 15)) * (unsigned)sizeof(c128);
    offB = (unsigned)(cg_dma_b_k(tid) * ldb + cg_dma_b_col(tid)) * (unsigned)sizeof(c128);
    wbase = __builtin_amdgcn_readfirstlane(tid & ~63);
  }
  // K-tile t of the segment list -> LDS buffer buf (4 + 4 loads of 16 B per thread)
  __device__ __forceinline__ void issue(int t, CgLds<128>& L, int buf) const {
    const CgSeg sg = segs[t / tps];
    issue_at(sg.A, sg.B, (t % tps) * CG_KT, L, buf);
  }
  // the K-tile at depth kt of the operand pair (A, B), named directly (no segment-table read)
  __device__ __forceinline__ void issue_at(const c128* A, const c128* B, int kt, CgLds<128>& L, int buf) const {
    const char* ga = cg_uniform(A + kt);
    const char* gb = cg_uniform(B + (size_t)kt * ldb);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      __builtin_amdgcn_global_load_lds((cg_gvoid*)(ga + (size_t)q * 32 * lda * sizeof(c128) + offA),
                                       (cg_lvoid*)(&L.a[buf][wbase + CG_WG * q]), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((cg_gvoid*)(gb + (size_t)q * 4 * ldb * sizeof(c128) + offB),
                                       (cg_lvoid*)(&L.b[buf][wbase + CG_WG * q]), 16, 0, 0);
    }
  }
  // piece i (0 .. 7) of a K-tile's eight loads per thread: A round i (i < 4) or B round i - 4 of issue_at, from the tile's
  // uniform bases ga = A + kt and gb = B + kt ldb (cg_uniform)
  __device__ __forceinline__ void piece(const char* ga, const char* gb, int i, CgLds<128>& L, int buf) const {
    const int q = i & 3;
    if (i >= 4)
      __builtin_amdgcn_global_load_lds((cg_gvoid*)(gb + (size_t)q * 4 * ldb * sizeof(c128) + offB),
                                       (cg_lvoid*)(&L.b[buf][wbase + CG_WG * q]), 16, 0, 0);
    else
      __builtin_amdgcn_global_load_lds((cg_gvoid*)(ga + (size_t)q * 32 * lda * sizeof(c128) + offA),
                                       (cg_lvoid*)(&L.a[buf][wbase + CG_WG * q]), 16, 0, 0);
  }
  // one half of issue_at: the B tile at depth kt of B alone (4 loads per thread), for a K-tile whose A half reaches LDS
  // from registers (glf_eig_kernel.hpp)
  __device__ __forceinline__ void issue_b_at(const c128* B, int kt, CgLds<128>& L, int buf) const {
    const char* gb = cg_uniform(B + (size_t)kt * ldb);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      __builtin_amdgcn_global_load_lds((cg_gvoid*)(gb + (size_t)q * 4 * ldb * sizeof(c128) + offB),
                                       (cg_lvoid*)(&L.b[buf][wbase + CG_WG * q]), 16, 0, 0);
  }
};

// The hook of cg_dma_ksteps: hook(p) runs at point p = 2 q + h / 2 of the stream (0 .. 7 for a whole K-tile), behind the
// fragment reads of half k-step (q, h) and ahead of its MFMAs.  The default does nothing and leaves no instruction: the
// batch kernel's instantiations are the ones they were.
struct CgNoHook {
  __device__ __forceinline__ void operator()(int) const {}
};

// Staging under the k-steps (glf_eig_kernel.hpp's two engines): the eight pieces of the K-tile (ga, gb) -> buffer buf go
// out two at the points 0 .. 3, the A rounds at points 0 and 1 and the B rounds at 2 and 3, each pair behind a half
// k-step's fragment reads and under its 12 MFMAs, so that no wave opens a K-tile with eight loads in front of its first
// fragment.  ga == nullptr: the B half alone (points 2 and 3); gb == nullptr: the A half alone (points 0 and 1); both:
// nothing.  A point holds one half's pieces only, so each takes one test.  The tests are uniform
// branches, and they also keep the loads in basic blocks of their own: hipcc's waitcnt pass puts s_waitcnt vmcnt(0)
// in front of an LDS read that follows LDS-DMA loads in the SAME block when it cannot tell their buffers apart (a
// run-time buffer index), which makes the read wait for the whole DMA it was meant to run under.  tools/dma_waits.py
// finds such waits in the listing; there must be none.
constexpr int CG_STAGE_PER = 2;   // pieces per point
struct CgDmaStageHook {
  const CgDmaStage& st;
  CgLds<128>& L;
  const char* ga;
  const char* gb;
  int buf;
  __device__ __forceinline__ void operator()(int p) const {
    static_assert(4 % CG_STAGE_PER == 0, "a point's pieces belong to one half");
    if (p * CG_STAGE_PER >= 8) return;
    if (p * CG_STAGE_PER < 4 ? !ga : !gb) return;
#pragma unroll
    for (int i = p * CG_STAGE_PER; i < (p + 1) * CG_STAGE_PER; ++i) st.piece(ga, gb, i, L, buf);
  }
};

// QD_PHASE_TIMING builds: the two engines of glf_eig_kernel.hpp stamp each K-tile per wave with the shader clock and no
// barrier in front: tk[o] the head (tile-end barrier released -> the first fragment reads and whatever the hook issues at
// point 0 are out), tk[o + 1] the k-steps (-> the last MFMA is issued), tk[o + 2] the tile-end wait and barrier.
#ifdef QD_PHASE_TIMING
#define CG_KSTAMP_PARAM , unsigned long long (&tk)[6], int tko
#define CG_KSTAMP_ARG(a, o) , a, o
#define CG_KSTAMP_TOP unsigned long long ks0_ = clock64(), ks1_ = ks0_;
#define CG_KSTAMP_END                  \
  cg_sched_fence();                    \
  const unsigned long long ks2_ = clock64(); \
  cg_sched_fence();
#define CG_KSTAMP_BAR                              \
  {                                                \
    const unsigned long long ks3_ = clock64();     \
    tk[tko] += ks1_ - ks0_;                        \
    tk[tko + 1] += ks2_ - ks1_;                    \
    tk[tko + 2] += ks3_ - ks2_;                    \
    ks0_ = ks3_;                                   \
  }
// hook H, then the clock at point 0
template <class H>
struct CgStampHook {
  const H& h;
  unsigned long long& at;
  __device__ __forceinline__ void operator()(int p) const {
    h(p);
    if (p == 0) {
      cg_sched_fence();
      at = clock64();
      cg_sched_fence();
    }
  }
};
#define CG_KSTAMP_HOOK(h) CgStampHook<decltype(h)>{h, ks1_}
#else
#define CG_KSTAMP_PARAM
#define CG_KSTAMP_ARG(a, o)
#define CG_KSTAMP_TOP
#define CG_KSTAMP_END
#define CG_KSTAMP_BAR
#define CG_KSTAMP_HOOK(h) h
#endif

// k-steps [Q0, Q1) of one K-tile for a wave with row tiles at r0[], column tiles at c0[] and the tiles SK skipped (the
// Hermitian segments' tiles below the diagonal; 0 elsewhere).  The B fragments are read and consumed two at a time and
// each operand sum is formed where its fragment is read: the third accumulator set takes the registers that a
// 4-product k-step spends on holding all four B fragments at once.
template <unsigned SK, int Q0, int Q1, class Hook = CgNoHook>
__device__ __forceinline__ void cg_dma_ksteps(const CgLds<128>& L, int buf, CgAcc3& acc, const int (&r0)[2],
                                              const int (&c0)[4], const Hook& hook = Hook()) {
  constexpr int BT = 128, MW = 2, NW = 4;
  constexpr unsigned LIVE = 0xffu & ~SK;   // the tiles this range computes
  const int lane = threadIdx.x & 63;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int q = Q0; q < Q1; ++q) {
    const int kk = 4 * q;
    c128 a[MW];
    double sa[MW];
#pragma unroll
    for (int mi = 0; mi < MW; ++mi) {
      a[mi] = L.a[buf][cg_dma_a_slot(r0[mi], lr, kk + lk)];
      if ((LIVE >> (mi * 4)) & 15u) sa[mi] = a[mi].re + a[mi].im;
    }
#pragma unroll
    for (int h = 0; h < NW; h += 2) {
      c128 b[2];
      double sb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nj = h + j;
        if (((LIVE >> nj) | (LIVE >> (4 + nj))) & 1u) {
          b[j] = L.b[buf][cg_dma_b_slot(kk + lk, c0[nj] + lr)];
          sb[j] = b[j].re + b[j].im;
        }
      }
      hook(2 * q + h / 2);
#pragma unroll
      for (int mi = 0; mi < MW; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int nj = h + j;
          if (SK & (1u << (mi * 4 + nj))) continue;   // below the diagonal: no Hermitian part
          acc.re[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi].re, b[j].re, acc.re[mi][nj], 0, 0, 0);
        }
#pragma unroll
      for (int mi = 0; mi < MW; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int nj = h + j;
          if (SK & (1u << (mi * 4 + nj))) continue;
          acc.im[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi].im, b[j].im, acc.im[mi][nj], 0, 0, 0);
          acc.p3[mi * 4 + nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(sa[mi], sb[j], acc.p3[mi * 4 + nj], 0, 0, 0);
        }
    }
  }
}

// The tiles of mask M scaled by the power of two S (exact): all three accumulator sets.
__device__ __forceinline__ void cg_dma_scale(CgAcc3& acc, unsigned M, double S) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj)
      if (M & (1u << (mi * 4 + nj))) {
        acc.re[mi][nj] *= S;
        acc.im[mi][nj] *= S;
        acc.p3[mi * 4 + nj] *= S;
      }
}

__device__ __forceinline__ void cg_dma_zero(CgAcc3& acc) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      acc.re[mi][nj] = d4{0.0, 0.0, 0.0, 0.0};
      acc.im[mi][nj] = d4{0.0, 0.0, 0.0, 0.0};
      acc.p3[mi * 4 + nj] = d4{0.0, 0.0, 0.0, 0.0};
    }
}

// (P1, P2, P3) -> (re, im); the accumulator then reads like a CgAcc<128>.
__device__ __forceinline__ void cg_dma_finalise(CgAcc3& acc) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const d4 p1 = acc.re[mi][nj], p2 = acc.im[mi][nj];
      acc.re[mi][nj] = p1 - p2;
      acc.im[mi][nj] = (acc.p3[mi * 4 + nj] - p1) - p2;
      // pinned tile by tile ahead of whatever follows the GEMM (the empty asm keeps the compiler from sinking the
      // subtractions into the epilogue): each p3 dies here instead of staying live next to the epilogue's loads
      asm volatile("" : "+v"(acc.re[mi][nj]), "+v"(acc.im[mi][nj]));
    }
}

// One link of a stage's K-tile stream: A B of depth K on the CgCfg<128> tiles, the operands named directly, with
// tile 0 of the GEMM that follows, (nA, nB), issued at the top of this GEMM's last K-tile into the buffer that tile
// leaves free.  K / 16 must be even: the last tile then computes from buffer 1, buffer 0 was last read one barrier
// earlier, and the follower finds its tile 0 where its own prologue would have put it.  The barrier that ends the last
// tile waits for that load (vmcnt(0)), so the follower starts without issue(0) and without a prologue barrier
// (cg_dma_block_gemm_stream with first = false, or cg_dma_herm_x_gemm with pre = true).  first: this GEMM heads the
// stream and stages its own tile 0.  All threads call it; ends with a workgroup barrier.  Visit the result with
// cg_epilogue<128>.
__device__ __forceinline__ void cg_dma_block_gemm_stream(const c128* A, const c128* B, const c128* nA, const c128* nB,
                                                         bool first, int K, int lda, int ldb, CgLds<128>& L,
                                                         CgAcc3& acc) {
  constexpr int MW = CgCfg<128>::MW, NW = CgCfg<128>::NW, WC = CgCfg<128>::WC, NQ = CG_KT / 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr0 = (wave / WC) * (MW * 16), wc0 = (wave % WC) * (NW * 16);
  const int r0[2] = {wr0, wr0 + 16}, c0[4] = {wc0, wc0 + 16, wc0 + 32, wc0 + 48};
  cg_dma_zero(acc);
  const int T = K / CG_KT;
  const CgDmaStage st(nullptr, T, lda, ldb);
  if (first) {
    st.issue_at(A, B, 0, L, 0);
    __syncthreads();
  }
  for (int t = 0; t < T; ++t) {
    if (t + 1 < T) st.issue_at(A, B, (t + 1) * CG_KT, L, (t + 1) & 1);
    else st.issue_at(nA, nB, 0, L, 0);
    cg_sched_fence();
    cg_dma_ksteps<0u, 0, NQ>(L, t & 1, acc, r0, c0);
    __syncthreads();
  }
  cg_dma_finalise(acc);
}

// K-tiles [t0, t1) of the X GEMM (of T in all) for wave W with the skipped tiles SK fixed at compile time.
template <int W, unsigned SK>
__device__ __forceinline__ void cg_dma_herm_x_range(int t0, int t1, int T, const CgDmaStage& st, CgLds<128>& L,
                                                    CgAcc3& acc) {
  constexpr int NQ = CG_KT / 4, R0 = 16 * (W >> 1), R1 = 16 * (7 - (W >> 1));
  const int r0[2] = {R0, R1};
  const int c0[4] = {16 * cg_herm_ctile(W, 0), 16 * cg_herm_ctile(W, 1), 16 * cg_herm_ctile(W, 2),
                     16 * cg_herm_ctile(W, 3)};
  for (int t = t0; t < t1; ++t) {
    if (t + 1 < T) st.issue(t + 1, L, (t + 1) & 1);
    cg_sched_fence();
    cg_dma_ksteps<SK, 0, NQ>(L, t & 1, acc, r0, c0);
    __syncthreads();
  }
}

// The Hermitian X GEMM of the file header (successor of the register-staged cg_herm_x_gemm: same segments, tile layout
// and roles).  segs[0] = (A, r), segs[1..nseg-1] = (B_c, W_c) with sum_c B_c W_c Hermitian; K = the common depth
// (tps = K / 16 K-tiles per segment).  Each wave runs the Hermitian segments on a code path of its own with compile-time
// tile roles: no selects or branches in the MFMA stream.  All threads call it; ends with a workgroup barrier.
// pre: tile 0 already sits in buffer 0, staged and waited for by the GEMM before it (cg_dma_block_gemm_stream).
__device__ __forceinline__ void cg_dma_herm_x_gemm(const CgSeg* segs, int nseg, int K, int lda, int ldb, CgLds<128>& L,
                                                   CgAcc3& acc, bool pre = false) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  cg_dma_zero(acc);
  const int tps = K / CG_KT, T = nseg * tps;
  const CgDmaStage st(segs, tps, lda, ldb);
  if (!pre) {
    st.issue(0, L, 0);
    __syncthreads();
  }
  auto run = [&](auto wc) {
    constexpr int W = decltype(wc)::value;
    // the tiles above the diagonal take the Hermitian segments twice: their segment-0 sums are halved, the Hermitian
    // segments run on the plain fragments and the result is doubled, 2 (A r / 2 + B W).  Powers of two commute with
    // every rounding, so the bits are those of A r + 2 B W and no wave holds a doubled copy of its A fragments.
    cg_dma_herm_x_range<W, 0u>(0, tps, T, st, L, acc);
    cg_dma_scale(acc, cg_herm_mask(W, false), 0.5);
    cg_dma_herm_x_range<W, cg_herm_mask(W, true)>(tps, T, T, st, L, acc);
    cg_dma_scale(acc, cg_herm_mask(W, false), 2.0);
  };
#define QD_HT(w) \
  case w: run(std::integral_constant<int, w>{}); break;
  switch (wave) {
    QD_HT(0) QD_HT(1) QD_HT(2) QD_HT(3) QD_HT(4) QD_HT(5) QD_HT(6) default: QD_HT(7)
  }
#undef QD_HT
  cg_dma_finalise(acc);
}

// (P1, P2, P3) -> (re, im) on the tiles of mask M only (cg_dma_finalise on a wave's live tiles).
template <unsigned M>
__device__ __forceinline__ void cg_dma_finalise_live(CgAcc3& acc) {
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      if (!(M & (1u << (mi * 4 + nj)))) continue;
      const d4 p1 = acc.re[mi][nj], p2 = acc.im[mi][nj];
      acc.re[mi][nj] = p1 - p2;
      acc.im[mi][nj] = (acc.p3[mi * 4 + nj] - p1) - p2;
      asm volatile("" : "+v"(acc.re[mi][nj]), "+v"(acc.im[mi][nj]));
    }
}

// ---------------------------------------------------------------- hand-overs through LDS (glf_eig_kernel.hpp)
// The two GEMMs of a stage whose operands are each other's results hand the first K-tiles over in LDS instead of
// through memory and a cold prologue.  These are cg_dma_block_gemm_stream and the Hermitian segments of
// cg_dma_herm_x_gemm with the lookahead and the prologue made selectable.  Every tile-end barrier is written as s_waitcnt
// vmcnt(0) + __syncthreads(): the hand-overs' arguments count on the drain, so it is spelled out instead of left to
// the fence the compiler puts in front of a barrier with a DMA in flight.
// Both engines stage the next K-tile from inside the k-steps (CgDmaStageHook: two pieces at each of the points 0 .. 3)
// instead of ahead of them.  Issuing later is safe by construction: the target buffer has been free since the tile-end
// barrier before (WAR), and the issuing wave's tile-end s_waitcnt vmcnt(0) followed by the barrier still covers every
// piece ahead of any wave's read of it (RAW): nothing else orders another wave's ds_read behind an LDS-DMA load.  The
// last piece goes out under k-step 1, with half the tile's MFMAs (two k-steps of both waves of the SIMD) behind it.

// cg_dma_block_gemm_stream whose follower may take the A half of its tile 0 from registers: nA == nullptr makes the
// lookahead the B half alone (tile 0 of nB -> L.b[0]) and leaves L.a[0] and, behind the closing barrier, all of
// buffer 1 to the caller.  L.a[0] was last read at tile T - 2, one barrier before the closing one.
// How the GEMM finds its first K-tiles:
//   CG_START_COLD   it heads a stream and stages its own tile 0 (a prologue: DMA round trip and barrier);
//   CG_START_TILE0  tile 0 sits in buffer 0, staged and waited for by the GEMM before it (an ordinary lookahead);
//   CG_START_TWO    tile 0 AND the B half of tile 1 are the caller's: tile 0 complete in buffer 0 and rows 16 .. 31 of
//                   B complete in L.b[1] behind a barrier, B in memory possibly still being stored by any wave.  Tile
//                   0's hook stages the A half of tile 1 alone (points 0 and 1), so no B is read from memory under
//                   it; its closing s_waitcnt vmcnt(0) + barrier retire that DMA, complete every wave's stores of B
//                   and make B workgroup-visible ahead of its first DMA read, tile 2, issued under tile 1.  No DMA is
//                   in flight when the loop is entered, so tile 0 stays in the loop with its run-time buffer index: the
//                   compiler has no LDS-DMA load to order its fragment reads behind, and the stores in flight do not
//                   concern an LDS read (a peeled tile 0 with the A half of tile 1 in flight across the caller's
//                   barrier was built and measured slower).
enum CgStart { CG_START_COLD, CG_START_TILE0, CG_START_TWO };
__device__ __forceinline__ void cg_dma_block_gemm_stream_h(const c128* A, const c128* B, const c128* nA, const c128* nB,
                                                           CgStart start, int K, int lda, int ldb, CgLds<128>& L,
                                                           CgAcc3& acc CG_KSTAMP_PARAM) {
  constexpr int MW = CgCfg<128>::MW, NW = CgCfg<128>::NW, WC = CgCfg<128>::WC, NQ = CG_KT / 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr0 = (wave / WC) * (MW * 16), wc0 = (wave % WC) * (NW * 16);
  const int r0[2] = {wr0, wr0 + 16}, c0[4] = {wc0, wc0 + 16, wc0 + 32, wc0 + 48};
  cg_dma_zero(acc);
  const int T = K / CG_KT;
  const CgDmaStage st(nullptr, T, lda, ldb);
  if (start == CG_START_COLD) {
    st.issue_at(A, B, 0, L, 0);
    __syncthreads();
  }
  CG_KSTAMP_TOP
  for (int t = 0; t < T; ++t) {
    // the tile staged under this one: tile t + 1 (under tile 0 of CG_START_TWO its A half alone), or at the last tile
    // the follower's tile 0, whole or its B half alone
    const bool more = t + 1 < T;
    const char* ga = more ? cg_uniform(A + (t + 1) * CG_KT) : nA ? cg_uniform(nA) : nullptr;
    const char* gb = cg_uniform(more ? B + (size_t)(t + 1) * CG_KT * ldb : nB);
    if (start == CG_START_TWO && t == 0) gb = nullptr;   // L.b[1] is the caller's: the A half of tile 1 alone
    const CgDmaStageHook hook{st, L, ga, gb, more ? (t + 1) & 1 : 0};
    cg_sched_fence();
    cg_dma_ksteps<0u, 0, NQ>(L, t & 1, acc, r0, c0, CG_KSTAMP_HOOK(hook));
    CG_KSTAMP_END
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    CG_KSTAMP_BAR
  }
  cg_dma_finalise(acc);
}

// Accumulator tile (mi, nj) of the CgCfg<128> layout (finalised: re / im) written into the A-tile image of buffer buf
// as the 16 columns [16 kt0 .. 16 kt0 + 15] of the rows the wave owns: the MFMA result map (register e of lane l =
// element ((l >> 4) + 4 e, l & 15)) through cg_dma_a_slot.  One ds_write_b128 per register; the 64 lanes of one cover
// four whole 256-byte rows of the image.
__device__ __forceinline__ void cg_dma_a_tile_write(const CgAcc3& acc, int mi, int nj, int row0 /* % 16 == 0 */, int lane,
                                                    CgLds<128>& L, int buf) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    L.a[buf][cg_dma_a_slot(row0, (lane >> 4) + 4 * e, lane & 15)] = cmk(acc.re[mi][nj][e], acc.im[mi][nj][e]);
}

// The Hermitian sum D = sum_c B_c W_c on its own (no segment 0, no halving): wave W's part on the tiles on and above the
// diagonal of the Hermitian tile layout, from a zeroed accumulator over every segment (segs[c] = (B_c, W_c), W_c in
// full).  The tiles below the diagonal are never touched: with W fixed at compile time they take no registers, so a
// wave holds at most 5 live tiles.  Called from a per-wave code path (switch on the wave index) by all threads; ends
// with a workgroup barrier; the caller finishes with cg_dma_finalise_live on the live tiles.  No prologue of its own.
// two = false: tile 0 sits in buffer 0, staged and waited for by the GEMM before it (an ordinary lookahead).  two = true: tiles 0 AND 1 are the caller's: tile 0 complete in buffer 0
// behind a barrier, the A half of tile 1 complete in L.a[1] behind the same barrier, the B half of tile 1 in flight to
// L.b[1] as this wave's own DMA.  Tile 0 then issues nothing (no hook) and its closing wait and barrier cover that DMA;
// the stream from memory starts with tile 2, issued inside tile 1.  The last tile reads buffer 1 (T is even) and its
// hook stages the A half alone of tile 0 of nA -> L.a[0], last read one barrier earlier, for a follower whose B half
// comes from the caller's registers; nA == nullptr: it issues nothing.  The closing wait and barrier cover that DMA.
template <int W>
__device__ __forceinline__ void cg_dma_herm_d_gemm_h(const CgSeg* segs, const c128* nA, int nseg, int K, int lda,
                                                     int ldb, CgLds<128>& L, CgAcc3& acc, bool two CG_KSTAMP_PARAM) {
  constexpr unsigned SK = cg_herm_mask(W, true);
  constexpr int NQ = CG_KT / 4, R0 = 16 * (W >> 1), R1 = 16 * (7 - (W >> 1));
  const int r0[2] = {R0, R1};
  const int c0[4] = {16 * cg_herm_ctile(W, 0), 16 * cg_herm_ctile(W, 1), 16 * cg_herm_ctile(W, 2),
                     16 * cg_herm_ctile(W, 3)};
  cg_dma_zero(acc);
  const int tps = K / CG_KT, T = nseg * tps;
  const CgDmaStage st(segs, tps, lda, ldb);
  int t = 0;
  CG_KSTAMP_TOP
  if (two) {   // both buffers named by literals: the fragment reads of buffer 0 do not wait for the DMA into buffer 1
    cg_sched_fence();
    const CgNoHook none;
    cg_dma_ksteps<SK, 0, NQ>(L, 0, acc, r0, c0, CG_KSTAMP_HOOK(none));
    CG_KSTAMP_END
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    CG_KSTAMP_BAR
    t = 1;
  }
  for (; t < T; ++t) {
    const char *ga = nullptr, *gb = nullptr;
    if (t + 1 == T) {   // the follower's tile 0, A half alone, or nothing
      if (nA) ga = cg_uniform(nA);
    } else {
      const CgSeg sg = segs[(t + 1) / tps];
      const int kt = ((t + 1) % tps) * CG_KT;
      ga = cg_uniform(sg.A + kt);
      gb = cg_uniform(sg.B + (size_t)kt * ldb);
    }
    const CgDmaStageHook hook{st, L, ga, gb, (t + 1) & 1};   // T even: the last tile stages into buffer 0
    cg_sched_fence();
    cg_dma_ksteps<SK, 0, NQ>(L, t & 1, acc, r0, c0, CG_KSTAMP_HOOK(hook));
    CG_KSTAMP_END
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    CG_KSTAMP_BAR
  }
}

// ---------------------------------------------------------------- k = A B + (A B)^+ in the accumulators (glf_eig_jump_kernel.hpp)
// For a tile (R, C) above the diagonal,
//   k_RC = sum_k A[R, k] B[k, C]  +  conj( sum_k B[k, R] A[C, k] )
// and the second sum is the same K-tile read with the roles swapped: its MFMA A fragment (m = lane & 15, k = lane >> 4)
// is B[kt + k][R0 + m], the B-image read of cg_dma_ksteps with the column tile set to R0, and its B fragment is
// A[C0 + n][kt + k], the A-image read with the row tile set to C0.  Both keep the images' conflict-free patterns, and
// nothing new is staged.  The conjugation is free in the 3-product form: P1 += ar br and P2 += ai bi are the same for
// conj(a) conj(b), and P3 takes (ar - ai)(br - bi) instead of the sums; cg_dma_finalise is unchanged.
// Masks over the wave's tiles (bit mi * 4 + nj): FS the tiles that run the first sum, SW (a subset) those that also
// run the swapped, conjugated sum, DG the tiles of FS on the diagonal (c0[nj] == r0[mi]): a diagonal tile's fragments
// are its row's, so they are read once.
constexpr unsigned cg_xh_row(unsigned m, int mi) { return (m >> (mi * 4)) & 15u; }
constexpr unsigned cg_xh_col(unsigned m, int nj) { return ((m >> nj) | (m >> (4 + nj))) & 1u; }
constexpr int cg_xh_diag_row(unsigned dg, int nj) { return (dg >> nj) & 1u ? 0 : (dg >> (4 + nj)) & 1u ? 1 : -1; }

// k-steps [Q0, Q1) of one K-tile: cg_dma_ksteps' order (row fragments, then the column fragments two at a time, the
// hook behind each pair's reads and ahead of its MFMAs), each tile's swapped sum issued behind the pair's first sums so
// that no MFMA follows the one it depends on.
template <unsigned FS, unsigned SW, unsigned DG, int Q0, int Q1, class Hook = CgNoHook>
__device__ __forceinline__ void cg_dma_ksteps_xh(const CgLds<128>& L, int buf, CgAcc3& acc, const int (&r0)[2],
                                                 const int (&c0)[4], const Hook& hook = Hook()) {
  static_assert((SW & ~FS) == 0u && (DG & ~FS) == 0u && (DG & SW) == 0u, "SW and DG are disjoint subsets of FS");
  constexpr int MW = 2, NW = 4;
  const int lane = threadIdx.x & 63;
  const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int q = Q0; q < Q1; ++q) {
    const int kk = 4 * q;
    c128 a[MW], br[MW];
    double sa[MW], sbr[MW], dbr[MW];
#pragma unroll
    for (int mi = 0; mi < MW; ++mi) {
      if (cg_xh_row(FS, mi)) {
        a[mi] = L.a[buf][cg_dma_a_slot(r0[mi], lr, kk + lk)];
        sa[mi] = a[mi].re + a[mi].im;
      }
      if (cg_xh_row(SW, mi)) {   // the swapped sums' A fragment: B on the wave's row tile
        br[mi] = L.b[buf][cg_dma_b_slot(kk + lk, r0[mi] + lr)];
        dbr[mi] = br[mi].re - br[mi].im;
        if (cg_xh_row(DG, mi)) sbr[mi] = br[mi].re + br[mi].im;
      }
    }
#pragma unroll
    for (int h = 0; h < NW; h += 2) {
      c128 b[2], ac[2];
      double sb[2], dac[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nj = h + j, dm = cg_xh_diag_row(DG, nj);
        if (cg_xh_col(FS, nj)) {
          if (dm >= 0 && cg_xh_row(SW, dm)) {
            b[j] = br[dm];
            sb[j] = sbr[dm];
          } else {
            b[j] = L.b[buf][cg_dma_b_slot(kk + lk, c0[nj] + lr)];
            sb[j] = b[j].re + b[j].im;
          }
        }
        if (cg_xh_col(SW, nj)) {   // the swapped sums' B fragment: A on the column tile
          if (dm >= 0) ac[j] = a[dm];
          else ac[j] = L.a[buf][cg_dma_a_slot(c0[nj], lr, kk + lk)];
          dac[j] = ac[j].re - ac[j].im;
        }
      }
      hook(2 * q + h / 2);
#pragma unroll
      for (int mi = 0; mi < MW; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int nj = h + j;
          if (!(FS & (1u << (mi * 4 + nj)))) continue;
          acc.re[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi].re, b[j].re, acc.re[mi][nj], 0, 0, 0);
        }
#pragma unroll
      for (int mi = 0; mi < MW; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int nj = h + j;
          if (!(FS & (1u << (mi * 4 + nj)))) continue;
          acc.im[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi].im, b[j].im, acc.im[mi][nj], 0, 0, 0);
          acc.p3[mi * 4 + nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(sa[mi], sb[j], acc.p3[mi * 4 + nj], 0, 0, 0);
        }
#pragma unroll
      for (int mi = 0; mi < MW; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int nj = h + j;
          if (!(SW & (1u << (mi * 4 + nj)))) continue;
          acc.re[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(br[mi].re, ac[j].re, acc.re[mi][nj], 0, 0, 0);
        }
#pragma unroll
      for (int mi = 0; mi < MW; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int nj = h + j;
          if (!(SW & (1u << (mi * 4 + nj)))) continue;
          acc.im[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(br[mi].im, ac[j].im, acc.im[mi][nj], 0, 0, 0);
          acc.p3[mi * 4 + nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(dbr[mi], dac[j], acc.p3[mi * 4 + nj], 0, 0, 0);
        }
    }
  }
}

}  // namespace qd
