// glf_eig_kernel.hpp — lindblad_eig_kernel: the Lindblad batch at Np = 128 propagated in the eigenbasis of the
// effective Hamiltonian's generator A = -iH - 1/2 sum_c C_c^+ C_c = V Lam V^-1 (host plan: pyqed_amd/oqs.py).  With
// rho~ = V^-1 rho V^-+ and C~_c = V^-1 C_c V the equation of motion is
//     d rho~/dt = Lam~ o rho~ + sum_c C~_c rho~ C~_c^+ ,   Lam~_ij = lam_i + conj(lam_j)
// so the A term is an elementwise multiply in the stage epilogue and only the dissipator is a GEMM.  The dissipator
// of a Hermitian rho~ is Hermitian on its own: the second GEMM runs on the 36 16 x 16 tiles on and above the diagonal
// (cg_dma_herm_d_gemm_h), each upper element's owner writes its mirror as the conjugate, and no X + X^+ pass through
// LDS exists.  Per stage (64 + 36) nc tile-GEMMs for the 64 + (64 + 36) nc of glf_batch_kernel.hpp (nc = 1: 9,600
// against 15,744 3-product MFMAs).  One persistent workgroup per matrix.  Only glf_eig.hip includes this header: next
// to the kernels of glf.hip it changed the batch kernel's register allocation (3 spilled VGPRs).
// One routine serves the two basis changes and the stages:
//     rn = a base + hc (g Lam~ o r + sum_c (M_c r) W_c)
// with a = g = 0, hc = 1 for a basis change (M = V^-1, W = V^-+ and M = V, W = V^+; the multiplications by zero are
// exact on finite data) and a = g = 1, hc the Horner coefficient of the stage (glf_horner_coef) otherwise.
// Every result is exactly Hermitian with an exactly real diagonal by construction.  RK4 of a linear equation commutes
// with the fixed change of variables, so in exact arithmetic the back-transformed state is the persistent kernel's;
// in floating point it differs from it in rounding, scaled by cond(V) (guarded on the host).
// A phase is one K-tile stream: every GEMM but its first finds its first K-tile in LDS buffer 0, put there under the
// GEMM before it, every K-tile is staged from inside the k-steps of the tile before it (CgDmaStageHook), and between the Y GEMM and the second GEMM at n_c = 1 the first two K-tiles of Y go from the
// accumulators into the staging buffers (eig_y_handover) instead of through memory, a drain and a cold prologue.  A
// phase hands the next one its first K-tiles in the same way: rows 0 .. 31 of its result go from eig_tail's registers into
// L.b[0] and L.b[1], the next M's K-tile 0 arrives by DMA under the second GEMM's last K-tile, and the barrier between
// the phases drains nothing.  The
// hand-overs and the waits and barriers each one rests on are listed in the kernel's phase loop.
// Register budget: the second GEMM holds at most 5 live tiles (120 accumulator VGPRs); 0 spilled VGPRs, 0 B scratch
// (tools/isa_diff.py).
#pragma once
#include "cgemm_dma128.hpp"
#include "glf_kernel.hpp"

namespace qd {

struct LindbladEigParams {
  const c128* Ct;    // [nc][128][128]  C~_c
  const c128* Ctd;   // [nc][128][128]  C~_c^+
  const c128* V;     // [128][128]      V (identity on the padding), Vd = V^+, Vi = V^-1, Vid = V^-+
  const c128* Vd;
  const c128* Vi;
  const c128* Vid;
  const c128* lam;   // [128]           eigenvalues of A (zero on the padding)
  const c128* eT;    // [ne][128][128]  (V^+ E_m V)^T
  c128* rho;         // [B][128][128]   state (in/out, original basis)
  c128* ws;          // [B][1 + nc][128][128]  stage buffer, Y_c
  c128* obs;         // [B][nsteps+1][ne]
  int nc, ne, nsteps;
  double dt;
  unsigned long long* tbuf;  // [B][QD_TSTRIDE] per-phase ticks and K-loop stamps (QD_PHASE_TIMING diagnostics) or null
};

namespace {

constexpr int EIG_NP = 128;

// A double every lane holds alike, moved to scalar registers.
__device__ __forceinline__ double eig_uniform(double v) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// m on the elements of wave W's tiles on and above the diagonal, in MFMA layout (q[mi * 4 + nj][e]; diagonal tiles load
// all 256 elements, the values below the diagonal are discarded).  Every address is the matrix's base (scalar
// registers) plus a 32-bit byte offset, the lane's own plus a uniform one.
template <int W>
__device__ __forceinline__ void eig_tile_loads(const c128* m, int lane, c128 (&q)[8][4]) {
  const unsigned vu = (unsigned)((lane >> 4) * EIG_NP + (lane & 15)) * (unsigned)sizeof(c128);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (W >> 1) : 7 - (W >> 1), C = cg_herm_ctile(W, nj);
      if (R > C) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned su = (unsigned)((16 * R + 4 * e) * EIG_NP) * (unsigned)sizeof(c128);   // uniform
        q[mi * 4 + nj][e] = *reinterpret_cast<const c128*>(reinterpret_cast<const char*>(m + 16 * C) + (vu + su));
      }
    }
}

// Behind the second GEMM: wave W, on its tiles with R <= C, forms k_ij = D_ij + g Lam~_ij r_ij and rn_ij = a base_ij +
// hc k_ij and writes rn_ji as the conjugate.  Diagonal tiles use ra <= lc only; on the diagonal Lam~_ii and r_ii are
// real, so the accumulator's imaginary part is dropped and rn_ii is real.  Each upper element is read (r, base) and
// written by one thread, loads first, so rn may be r or base.  The loads of r are issued behind the (P1, P2, P3) ->
// (re, im) arithmetic and those of base once r is consumed: either set of five tiles next to all three accumulator
// sets, or both next to two, spilled.
// Rows 0 .. 31 of rn are the B halves of K-tiles 0 and 1 of the next phase's Y GEMM.  Besides going to memory as every
// other row they are written into L.b[0] (rows 0 .. 15) and L.b[1] (rows 16 .. 31) in the engine's B-tile image
// (cg_dma_b_slot), the same values from the same registers, by the roles of eig_rn_lds_upper / eig_rn_lds_mirror: compile-time
// facts of W like every other tile role here.  The last phase of a call writes them too and nobody reads them.
constexpr bool eig_rn_lds_upper(int R, int C, int ra, int lc) { return R < 2 && (R < C || ra <= lc); }
constexpr bool eig_rn_lds_mirror(int R, int C, int ra, int lc) { return C < 2 && (R < C || ra < lc); }
// Every slot of the two images has exactly one writer: rows 0 .. 15 come from waves 0 and 1 (row tile 0, all eight column
// tiles), rows 16 .. 31 from waves 2 and 3 (row tile 1, C >= 1), tile (1, 0) from wave 0 as the conjugate transpose of its
// tile (0, 1), and the lower triangles of (0, 0) and (1, 1) from their owners as conjugates.
constexpr bool eig_rn_lds_one_to_one() {
  unsigned char n[2][CG_KT * EIG_NP] = {};
  for (int w = 0; w < 8; ++w)
    for (int mi = 0; mi < 2; ++mi)
      for (int nj = 0; nj < 4; ++nj) {
        const int R = mi == 0 ? (w >> 1) : 7 - (w >> 1), C = cg_herm_ctile(w, nj);
        if (R > C) continue;
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 4; ++e) {
            const int ra = (lane >> 4) + 4 * e, lc = lane & 15;
            if (eig_rn_lds_upper(R, C, ra, lc)) ++n[R][cg_dma_b_slot(ra, 16 * C + lc)];    // rn[16 R + ra][16 C + lc]
            if (eig_rn_lds_mirror(R, C, ra, lc)) ++n[C][cg_dma_b_slot(lc, 16 * R + ra)];   // rn[16 C + lc][16 R + ra]
          }
      }
  for (int t = 0; t < 2; ++t)
    for (int s = 0; s < CG_KT * EIG_NP; ++s)
      if (n[t][s] != 1) return false;
  return true;
}
static_assert(eig_rn_lds_one_to_one(), "rows 0 .. 31 of rn onto L.b[0], L.b[1]: one writer per slot");
template <int W>
__device__ __forceinline__ void eig_tail(CgAcc3& A, const c128* r, const c128* base, c128* rn, const c128* lamS,
                                         CgLds<128>& L, int lane, double a, double g, double hc) {
  constexpr unsigned LIVE = 0xffu & ~cg_herm_mask(W, true);
  const int lr = lane >> 4, lc = lane & 15;
  const unsigned vu = (unsigned)(lr * EIG_NP + lc) * (unsigned)sizeof(c128);
  const unsigned vm = (unsigned)(lc * EIG_NP + lr) * (unsigned)sizeof(c128);
  c128 q[8][4];
  cg_dma_finalise_live<LIVE>(A);
  cg_sched_fence();   // the loads of r go into the registers the third accumulator set has left
  eig_tile_loads<W>(r, lane, q);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (W >> 1) : 7 - (W >> 1), C = cg_herm_ctile(W, nj);
      if (R > C) continue;
      const c128 lj = lamS[16 * C + lc];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const c128 li = lamS[16 * R + lr + 4 * e], x = q[mi * 4 + nj][e];
        const double gre = g * (li.re + lj.re), gim = g * (li.im - lj.im);   // g (lam_i + conj(lam_j))
        A.re[mi][nj][e] += gre * x.re - gim * x.im;
        A.im[mi][nj][e] += gre * x.im + gim * x.re;
      }
      // pinned tile by tile, as in cg_dma_finalise: sunk to the stores, the sums kept r live next to base
      asm volatile("" : "+v"(A.re[mi][nj]), "+v"(A.im[mi][nj]));
    }
  cg_sched_fence();   // the loads of base go into the registers r has left
  eig_tile_loads<W>(base, lane, q);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (W >> 1) : 7 - (W >> 1), C = cg_herm_ctile(W, nj);
      if (R > C) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ra = lr + 4 * e;
        const c128 k = cmk(A.re[mi][nj][e], A.im[mi][nj][e]);
        c128 v = cadd(cscale(q[mi * 4 + nj][e], a), cscale(k, hc));
        if (R == C && ra == lc) v.im = 0.0;
        const unsigned su = (unsigned)((16 * R + 4 * e) * EIG_NP) * (unsigned)sizeof(c128);   // uniform, as sm
        const unsigned sm = (unsigned)(16 * C * EIG_NP) * (unsigned)sizeof(c128);
        char* u = reinterpret_cast<char*>(rn + 16 * C) + (vu + su);
        char* t = reinterpret_cast<char*>(rn + 16 * R + 4 * e) + (vm + sm);
        if (R < C || ra <= lc) *reinterpret_cast<c128*>(u) = v;
        if (R < C || ra < lc) *reinterpret_cast<c128*>(t) = cconj(v);
        if constexpr (W < 4) {   // row tiles 0 and 1 (mi == 0 of waves 0 .. 3); the buffers are named by literals
          if (R < 2 && eig_rn_lds_upper(R, C, ra, lc)) L.b[R & 1][cg_dma_b_slot(ra, 16 * C + lc)] = v;
          if (R < 2 && C < 2 && eig_rn_lds_mirror(R, C, ra, lc)) L.b[C & 1][cg_dma_b_slot(lc, 16 * R + ra)] = cconj(v);
        }
      }
    }
}

// Y = M r of an n_c = 1 phase handed to the second GEMM: columns 0 .. 31 are K-tiles 0 and 1 of its A operand and sit,
// finalised, in the accumulators of the four waves with wc0 == 0 (column tiles nj = 0, 1 of both row tiles).  Those go
// into L.a[0] and L.a[1] from the registers and never to memory; every other column is stored to Y as before and
// streamed back from tile 2 on.
__device__ __forceinline__ void eig_y_handover(const CgAcc3& A, c128* Y, CgLds<128>& L) {
  constexpr int MW = CgCfg<128>::MW, NW = CgCfg<128>::NW, WC = CgCfg<128>::WC;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));   // as in cg_epilogue
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int wr0 = (wave / WC) * (MW * 16), wc0 = (wave % WC) * (NW * 16);
  if (wc0 == 0) {
#pragma unroll
    for (int mi = 0; mi < MW; ++mi) {
      cg_dma_a_tile_write(A, mi, 0, wr0 + mi * 16, lane, L, 0);
      cg_dma_a_tile_write(A, mi, 1, wr0 + mi * 16, lane, L, 1);
    }
  }
#pragma unroll
  for (int mi = 0; mi < MW; ++mi)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int nj = 0; nj < NW; ++nj) {
        if (nj < 2 && wc0 == 0) continue;
        const int row = wr0 + mi * 16 + (lane >> 4) + 4 * e, col = wc0 + nj * 16 + (lane & 15);
        Y[(size_t)row * EIG_NP + col] = cmk(A.re[mi][nj][e], A.im[mi][nj][e]);
      }
}

__global__ __launch_bounds__(CG_WG) void lindblad_eig_kernel(LindbladEigParams p) {
  constexpr int BT = EIG_NP, Np = EIG_NP;
  constexpr size_t NN = (size_t)Np * Np;
  __shared__ CgLds<BT> L;
  __shared__ c128 sred[CG_WG / 64];
  __shared__ CgSeg segs[MAX_NC];   // the second GEMM's segment table (Y_c, W_c)
  __shared__ c128 lamS[Np];

  const int b = blockIdx.x;
  c128* rho = p.rho + (size_t)b * NN;
  c128* ws = p.ws + (size_t)b * (1 + p.nc) * NN;
  c128* Y = ws + NN;
  c128* obs = p.obs ? p.obs + (size_t)b * (p.nsteps + 1) * p.ne : nullptr;
  if (threadIdx.x < Np) lamS[threadIdx.x] = p.lam[threadIdx.x];
  __syncthreads();

  CgAcc3 A;
  QD_TIMING_DECL
#ifdef QD_PHASE_TIMING
  unsigned long long txf = 0;   // the basis changes' ticks, charged to slot 5 instead of the stages' slots
#endif

  // Phase ph of the call: 0 the change to the eigenbasis, 1 .. 4 nsteps the Horner stages, then the change back.
  const int nph = 4 * p.nsteps + 2;
  for (int ph = 0; ph < nph; ++ph) {
    const bool xf = ph == 0 || ph == nph - 1;
    const int stage = (ph - 1) & 3;
    // Horner stages (glf_horner_coef): rho~ -> s1 -> s2 -> s3 -> rho~, s_m in place in ws; a basis change in place
    const c128* r = (xf || stage == 0) ? rho : ws;
    c128* rn = (xf || stage == 3) ? rho : ws;
    const c128* M = ph == 0 ? p.Vi : xf ? p.V : p.Ct;
    const c128* Wm = ph == 0 ? p.Vid : xf ? p.Vd : p.Ctd;
    int n = xf ? 1 : p.nc;
    double dts = p.dt;
    asm volatile("" : "+s"(dts), "+s"(n));   // per phase: no coefficient or flag register held across the K loops
    const double hc = eig_uniform(xf ? 1.0 : glf_horner_coef(dts, stage)), ag = xf ? 0.0 : 1.0;
#ifdef QD_PHASE_TIMING
    unsigned long long tkeep[4] = {tacc[0], tacc[1], tacc[2], tacc[3]};
#endif
    // One K-tile stream per phase: every GEMM but the phase's first finds its tile 0 in LDS buffer 0, and no barrier,
    // drain or prologue stands between a GEMM and its follower.  The segment table is written ahead of the Y GEMMs'
    // barriers; its last reader in the phase before is separated from these writes by that phase's closing barrier.
    // T = 8 n is even: every GEMM's last K-tile reads buffer 1 and buffer 0 was last read one
    // barrier earlier.  Every tile-end barrier of the two engines used here is s_waitcnt vmcnt(0) + barrier.
    // Staging: a K-tile's eight DMA pieces per thread are issued inside the k-steps of the tile before it, two behind
    // the fragment reads of each of its first four half k-steps (CgDmaStageHook, cgemm_dma128.hpp), not at its top.
    // "Issued under tile t" below means there.  What every placement rests on: WAR, the tile-end barrier of tile t - 1,
    // behind which no wave reads the target buffer again; RAW, the issuing wave's s_waitcnt vmcnt(0) at the end of
    // tile t and the barrier behind it, the only thing that orders another wave's ds_read behind an LDS-DMA load.
    // The special cases:
    //   a GEMM's last tile, whole lookahead (n >= 2, and Y_c -> Y_{c+1}): the follower's tile 0 -> buffer 0 under tile
    //     T - 1, which reads buffer 1; buffer 0 was last read at tile T - 2.
    //   the Y GEMM's last tile at n = 1, B half alone: points 0 and 1 issue nothing, W tile 0 -> L.b[0] at points 2, 3.
    //   tile 0 of the second GEMM with `two`: no hook at all; the only DMA in flight is the one issued behind the Y
    //     GEMM's closing barrier (below), covered by tile 0's closing wait and barrier.
    //   tile 2 of Y (second GEMM, n = 1): first issued under tile 1, behind tile 0's closing wait and barrier, which
    //     complete and publish the Y stores (see (2)).
    //   the second GEMM's last tile, A half alone: the next phase's M tile 0 -> L.a[0] at points 0 and 1, nothing at 2
    //     and 3; behind the call's last phase nothing is issued (see (6)).
    //   tile 0 of a phase's first Y GEMM behind a hand-over (CG_START_TWO), A half alone: M tile 1 -> L.a[1] at points 0
    //     and 1; the B halves of tiles 0 and 1 are in LDS already and rn is not read from memory before tile 2 (see (6)).
    //   issue_b_at behind the Y GEMM's closing barrier (n = 1): stays where it was, every wave its four pieces, ahead
    //     of the raw barrier; it is no part of a K loop.
    // Invariants (keep ALL of these when editing):
    //  (1) Y_c -> Y_{c+1} (n >= 2): the lookahead of cg_dma_block_gemm_stream_h, (M_{c+1}, r) tile 0.
    //  (2) last Y GEMM -> second GEMM, n = 1.  Tiles 0 and 1 of the second GEMM's A operand are columns 0 .. 31 of Y
    //      and go from the accumulators into L.a[0] and L.a[1] (eig_y_handover); the B halves are DMA: W tile 0 ->
    //      L.b[0] as the Y GEMM's lookahead, W tile 1 -> L.b[1] behind its closing barrier.
    //      WAR: L.a[0] and L.b[0] were last read at Y tile 6 and L.a[1], L.b[1] at Y tile 7; the lookahead is issued
    //      behind tile 6's barrier (under tile 7), the ds_writes and the second DMA behind tile 7's (the closing one).
    //      RAW: L.b[0]: the closing barrier's vmcnt(0).  L.a[0], L.a[1]: each writer's s_waitcnt lgkmcnt(0), then the
    //      raw s_barrier below, ahead of tile 0's fragment reads.  That barrier must not be a __syncthreads(): with
    //      the DMA and the Y stores in flight it would drain both.  L.b[1]: in flight across it; tile 0 reads buffer
    //      0 only and its closing s_waitcnt vmcnt(0) + barrier retire the DMA ahead of tile 1's reads.
    //      Y in memory: vmcnt counts stores, so the same tile-0 wait completes every wave's Y stores and the barrier
    //      makes all of Y (columns 32 .. 127) workgroup-visible (one CU, write-through L1) ahead of the first DMA read
    //      of it, tile 2, issued under tile 1.  Nothing is issued under tile 0.
    //  (3) last Y GEMM -> second GEMM, n >= 2: an ordinary lookahead of (Y_0, W_0) tile 0.  Y_0 was stored ahead of
    //      Y GEMM 1, whose seven drained tile-end barriers precede the first such lookahead; Y_{n-1} is first read at
    //      tile 8 (n - 1) - 1 of the second GEMM, behind at least seven of its drained barriers.
    //  (4) nothing between a hand-over and its reader touches the staging buffers: the Y epilogue and eig_tail store
    //      from registers.
    //  (5) no compiler-made s_waitcnt vmcnt between a K loop's DMA pieces and a fragment read (tools/dma_waits.py on
    //      the listing): the pieces sit behind uniform branches in blocks of their own (CgDmaStageHook).
    //  (6) phase -> next phase (every phase but the call's last; the call's first phase keeps its cold prologue).  K-tiles
    //      0 and 1 of the next Y GEMM (c = 0): the B halves are rows 0 .. 31 of rn and go from eig_tail's registers into
    //      L.b[0] and L.b[1] (and to memory as before: later K-tiles, the epilogue and the caller read them there); the A
    //      halves are DMA: the next M's tile 0 -> L.a[0] under the second GEMM's last tile, tile 1 -> L.a[1] under the Y
    //      GEMM's tile 0.
    //      WAR: L.a[0] was last read at the second GEMM's tile T - 2, one barrier ahead of the hook that issues into it;
    //      L.b[0] at T - 2 and L.b[1] at T - 1, both ahead of the second GEMM's closing barrier, behind which eig_tail
    //      writes; L.a[1] at T - 1, and its DMA is issued behind that barrier and the one below.
    //      RAW: L.a[0]: the second GEMM's closing s_waitcnt vmcnt(0) + barrier.  L.b[0], L.b[1]: each writer's s_waitcnt
    //      lgkmcnt(0), then the raw s_barrier below, ahead of tile 0's fragment reads.  That barrier must not wait for
    //      vmcnt and must not be a __syncthreads(): it would drain the rn stores in front of tile 0 instead of under it.
    //      L.a[1]: the Y GEMM's tile-0 wait and barrier, as for any staged tile.
    //      rn in memory: the same tile-0 wait completes every wave's rn stores and the barrier makes rn workgroup-visible
    //      ahead of the first DMA read of it, tile 2 (rows 32 .. 47), issued under tile 1; under tile 0 only M is read.
    //      These are (2)'s arguments moved one GEMM later.
    //      In place: rn may be r (basis changes, stages 1 and 2) or base (basis changes, stage 3).  Every element of r and
    //      base is loaded by its owner before the owner stores it and its mirror (eig_tail), the Y GEMMs' DMA reads of r
    //      were retired by their tile-end waits, and the second GEMM reads Y and W alone; the raw barrier changes none
    //      of this, and the next phase reads rn from memory behind the drain of its tile 0 only.
    //      The segment table: its readers (the second GEMM's hooks up to tile T - 2) are done ahead of the closing
    //      barrier of tile T - 1, and thread 0 writes it behind the raw barrier.
    //      Observables (ne > 0, behind the first basis change and behind every step): wg_observables reads rho from
    //      memory, so there the phase ends in a full __syncthreads() (drain and publish); it touches sred alone, the
    //      staged tiles stay by (4), and the next phase starts as behind any other.
    int tid0 = threadIdx.x;
    asm volatile("" : "+v"(tid0));
    if (tid0 == 0)
      for (int c = 0; c < n; ++c) {
        segs[c].A = Y + (size_t)c * NN;
        segs[c].B = Wm + (size_t)c * NN;
      }
    const bool hand = n == 1;
    for (int c = 0; c < n; ++c) {
      const c128* Mc = M + (size_t)c * NN;
      const bool last = c + 1 == n;
      // the call's first phase stages its own tile 0; every later one finds tile 0 and L.b[1] handed on by the phase before (6)
      const CgStart start = c > 0 ? CG_START_TILE0 : ph == 0 ? CG_START_COLD : CG_START_TWO;
      cg_dma_block_gemm_stream_h(Mc, r, last ? (hand ? nullptr : Y) : Mc + NN, last ? Wm : r, start, Np, Np,
                                 Np, L, A CG_KSTAMP_ARG(tk, 0));
      QD_TMARK(0);
      c128* Yc = Y + (size_t)c * NN;
      if (hand) {
        eig_y_handover(A, Yc, L);
        const CgDmaStage st(nullptr, Np / CG_KT, Np, Np);
        st.issue_b_at(Wm, CG_KT, L, 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's ds_writes; NOT vmcnt: see (2)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      } else {
        cg_epilogue<BT>(A, [&](int row, int col, c128 v) { Yc[(size_t)row * Np + col] = v; });
      }
      QD_TMARK(1);
    }
    {
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));   // the per-element index math stays inside the phase
      const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = tid & 63;
      // the next phase's M (c = 0): a stage's C~, V ahead of the change back, nothing behind the last phase
      const c128* nM = ph + 1 == nph ? nullptr : ph + 2 == nph ? p.V : p.Ct;
      auto tail = [&](auto wc) {
        constexpr int W = decltype(wc)::value;
        cg_dma_herm_d_gemm_h<W>(segs, nM, n, Np, Np, Np, L, A, hand CG_KSTAMP_ARG(tk, 3));
        QD_TMARK(2);
        eig_tail<W>(A, r, rho, rn, lamS, L, lane, ag, ag, hc);
      };
#define QD_EW(w) \
  case w: tail(std::integral_constant<int, w>{}); break;
      switch (wave) { QD_EW(0) QD_EW(1) QD_EW(2) QD_EW(3) QD_EW(4) QD_EW(5) QD_EW(6) default: QD_EW(7) }
#undef QD_EW
    }
    const bool watch = (ph == 0 || (!xf && stage == 3)) && p.ne > 0;   // observables on rho~: t0 and the end of every step
    if (watch) {
      __syncthreads();   // wg_observables reads rho from memory: the stores drained and published
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's ds_writes of rows 0 .. 31; NOT vmcnt: see (6)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    QD_TMARK(3);
#ifdef QD_PHASE_TIMING
    if (xf)
      for (int q = 0; q < 4; ++q) {
        txf += tacc[q] - tkeep[q];
        tacc[q] = tkeep[q];
      }
#endif
    if (watch) {   // touches sred alone: the staged tiles stay (4)
      wg_observables(rho, p.eT, p.ne, NN, obs + (size_t)(ph / 4) * p.ne, sred);
      __syncthreads();
      QD_TMARK(4);
    }
  }
#ifdef QD_PHASE_TIMING
  tacc[5] += txf;
#endif
  QD_TIMING_FLUSH
}

}  // namespace
}  // namespace qd
