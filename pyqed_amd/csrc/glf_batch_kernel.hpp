// glf_batch_kernel.hpp — the Lindblad batch kernel lindblad_rk4_kernel<128, true, true, false> (the headline one):
// the persistent Hermitian kernel at Np = 128 for Lindblad operands (sum_c C_c r C_c^+ / 2 Hermitian), an explicit
// specialization of glf_kernel.hpp's template on an engine of its own (cgemm_dma128.hpp).  Only glf.hip includes it:
// its register allocation sits on the 256-VGPR wall (0 spilled, 0 B scratch) and has changed with its neighbours in
// the translation unit and with statements moved into helpers.  After any edit compare assembly and resource figures
// with tools/isa_diff.py; a build that spills a VGPR or uses scratch is not a candidate.
// What the allocator gives up first are loop invariants held across every K loop, so the kernel keeps none it can form
// where it is used: the thread index, dt, n_c and Np each go through an empty asm at their point of use (the Horner
// coefficient, the n_c tests, the epilogue's row offsets and the observables' lane index are then made per stage or
// per call), and the epilogue's addresses are the matrix base in scalar registers plus one 32-bit offset.
// Stage epilogue: k = X + X^+ is formed in the registers of the wave that owns the upper element, with one trip of the
// lower elements through LDS and one barrier ahead of the Horner update (HermKL, herm_k_publish, herm_k_update:
// glf_herm_k.hpp, shared with lindblad_eig_jump_kernel in its own translation unit; the text moved there unchanged
// and this kernel's instructions with it, tools/isa_diff.py).
#pragma once
#include "glf_herm_k.hpp"

namespace qd {
namespace {

template <>
__global__ __launch_bounds__(CG_WG) void lindblad_rk4_kernel<128, true, true, false>(LindbladParams p) {
  constexpr int BT = 128;
  if (p.guard && __hip_atomic_load(p.guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  __shared__ CgLds<BT> L;
  __shared__ c128 sred[CG_WG / 64];
  __shared__ CgSeg segs[2 + MAX_NC];   // segment table in LDS (no scratch)

  const int b = blockIdx.x;
  const int Np = p.Np;
  const size_t NN = (size_t)Np * Np;
  c128* rho = p.rho + (size_t)b * NN;
  // single block: always true here (launched at Np == 128 only), tested at run time as in glf_kernel.hpp's template
  const bool single = (Np / BT) == 1;
  c128* ws = p.ws + (size_t)b * glf_slots(Np, p.nc) * NN;
  c128* rbuf1 = single ? ws : ws + NN;
  c128* Y = single ? ws + NN : ws + 2 * NN;
  c128* obs = p.obs ? p.obs + (size_t)b * (p.total_steps + 1) * p.ne : nullptr;

  if (p.ne > 0 && p.step0 == 0) wg_observables_batch(rho, p.eT, p.ne, NN, obs, sred);
  __syncthreads();

  const double dt = p.dt;
  CgAcc3 A;
  QD_TIMING_DECL

  for (int step = 0; step < p.nsteps; ++step) {
    for (int stage = 0; stage < 4; ++stage) {
      // Horner stages (glf_horner_coef): rho -> s1 -> s2 -> s3 -> rho; single block: s_m in place in ws
      const c128* r = stage == 0 ? rho : ((stage - 1) & 1) ? rbuf1 : ws;
      c128* rn = stage == 3 ? rho : (stage & 1) ? rbuf1 : ws;
      // the stages' coefficients stay out of the VGPRs: formed per stage from a dt the compiler cannot see through
      // (hoisted out of the step loop, dt / 3 and dt / 2 sat in four VGPRs across every K loop), then scalar
      double dts = dt;
      asm volatile("" : "+s"(dts));
      const double hc = wave_uniform(glf_horner_coef(dts, stage));
      // Hermitian rho: L[rho] = X + X^+ with X = (-iK) r + sum_c (C_c r)(C_c^+ / 2)   (single block; p.Cd holds
      // C_c^+ / 2 on this path).  phase 1: Y_c = C_c r
      // One K-tile stream per stage: Y_0 .. Y_{nc-1}, then X.  The X GEMM's segment table is written here, once;
      // the Y GEMMs name their operands directly and never read it.  The last K-tile of each GEMM stages tile 0 of
      // the next one (Y_{c+1}: (C_{c+1}, r); after the last c the X GEMM's (mK, r)), both known before the stage
      // starts, so only the stage's first GEMM pays a cold tile.
      // Invariants (keep ALL of these when editing):
      //  (1) the table's first reader is the X GEMM's issue(1) at the top of its tile 0, at least Np / 16 tile-end
      //      barriers after thread 0's writes (nc = 0: the barrier below); its last reader in the stage before is
      //      separated from these writes by the two barriers of the k epilogue;
      //  (2) Np / 16 is even (Np = 128 here), so a GEMM's last tile reads buffer 1 and the lookahead goes to
      //      buffer 0, last read one barrier earlier;
      //  (3) no barrier follows the Y stores.  Every tile-end __syncthreads() of the X GEMM has an LDS-DMA load in
      //      flight and is therefore s_waitcnt vmcnt(0) + s_barrier; vmcnt counts stores as well, so each wave's
      //      Y stores are complete when it arrives at the barrier that ends X tile 0, and all of Y is complete and
      //      workgroup-visible (one CU, write-through L1) once that barrier releases.  Segment 0 (tiles 0 ..
      //      Np/16 - 1) reads (mK, r) only; the first load of a Y_c is issued at the top of tile Np/16 - 1, behind
      //      the barrier that ends tile Np/16 - 2: six barriers later at Np = 128.  The Y stores drain under
      //      segment 0's first MFMAs.  A GEMM loop whose tile-end barrier no longer drains vmcnt (counted waits, a
      //      raw s_barrier) needs an explicit s_waitcnt vmcnt(0) ahead of one of segment 0's barriers.
      //  (4) nothing between a lookahead and its consumer touches LDS buffer 0 (cg_epilogue stores from registers).
      int tid0 = threadIdx.x, nc = p.nc;
      asm volatile("" : "+v"(tid0), "+s"(nc));   // tests made per stage: no flag register held across the K loops
      if (tid0 == 0) {
        segs[0].A = p.mK;
        segs[0].B = r;
        for (int c = 0; c < nc; ++c) {
          segs[1 + c].A = Y + (size_t)c * NN;
          segs[1 + c].B = p.Cd + (size_t)c * NN;
        }
      }
      if (nc == 0) __syncthreads();   // no Y GEMM to hide the X prologue under
      for (int c = 0; c < nc; ++c) {
        const c128* nA = c + 1 < nc ? p.Cop + (size_t)(c + 1) * NN : p.mK;
        cg_dma_block_gemm_stream(p.Cop + (size_t)c * NN, r, nA, r, c == 0, Np, Np, Np, L, A);
        QD_TMARK(0);
        c128* Yc = Y + (size_t)c * NN;
        cg_epilogue<BT>(A, [&](int row, int col, c128 v) { Yc[(size_t)row * Np + col] = v; });
        QD_TMARK(1);
      }
      // phase 2: X in registers (one accumulator over 1 + nc segments), fused k and RK4 epilogue
      cg_dma_herm_x_gemm(segs, 1 + nc, Np, Np, Np, L, A, nc > 0);
      QD_TMARK(2);
      // k = X + X^+ formed in the registers of the wave that owns the upper element: every wave publishes conj(X) of its
      // elements below the diagonal at the mirror slot of the HermKL image (herm_k_publish; those accumulators die),
      // loads rho on its tiles on and above the diagonal into the freed registers, and behind ONE barrier adds the
      // mirror from LDS to its own X_ij and runs the Horner update on (i, j) and, as the conjugate, on (j, i)
      // (herm_k_update).  Each k is the same two operands in the same addition as X_ij + conj(X_ji) formed in LDS.
      // The rho loads sit before the barrier: one load latency per stage, most of it under the barrier.  At stage 3
      // (rn == rho) every element and its mirror are read and written by one thread, loads first.  The closing barrier
      // keeps the next stage's LDS-DMA out of the image and makes rn complete for it.
      {
        static_assert(HermKL::SIZE * sizeof(c128) <= sizeof(CgLds<BT>), "LDS k image");
        c128* KL = reinterpret_cast<c128*>(&L);
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));  // keep the per-element index math inside the stage loop (no LICM + spill)
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = tid & 63;
        int Npe = Np;
        asm volatile("" : "+s"(Npe));   // likewise the uniform row offsets: per stage, not in scalar registers for the run
        auto tail = [&](auto wc) {
          constexpr int W = decltype(wc)::value;
          c128 q[8][4];
          herm_k_publish<W>(A, KL, lane);
          cg_sched_fence();   // the loads go into the registers the publishing frees: none may be scheduled ahead of it
          herm_k_rho_loads<W>(rho, Npe, lane, q, 0, HERM_K_NPRE);
          __syncthreads();
          QD_TMARK(5);
          herm_k_update<W, HERM_K_NPRE>(A, KL, lane, q, rho, rn, Npe, hc);
        };
#define QD_KW(w) \
  case w: tail(std::integral_constant<int, w>{}); break;
        switch (wave) { QD_KW(0) QD_KW(1) QD_KW(2) QD_KW(3) QD_KW(4) QD_KW(5) QD_KW(6) default: QD_KW(7) }
#undef QD_KW
        __syncthreads();
      }
      QD_TMARK(3);
    }
    const int gs = p.step0 + step + 1;  // global step count after this step
    if (p.ne > 0) wg_observables_batch(rho, p.eT, p.ne, NN, obs + (size_t)gs * p.ne, sred);
    if (p.snap && p.save_every > 0 && (gs % p.save_every) == 0) {
      const int s = gs / p.save_every - 1;
      if (s < p.nsave) {
        const int N = p.N;
        c128* out = p.snap + ((size_t)b * p.nsave + s) * N * N;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));  // as in wg_observables
        for (size_t i = tid; i < (size_t)N * N; i += CG_WG) {
          const int ii = (int)(i / N), jj = (int)(i % N);
          out[i] = rho[(size_t)ii * Np + jj];
        }
      }
    }
    __syncthreads();
    QD_TMARK(4);
  }
  QD_TIMING_FLUSH
}

}  // namespace
}  // namespace qd
