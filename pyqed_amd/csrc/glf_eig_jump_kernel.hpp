// glf_eig_jump_kernel.hpp — lindblad_eig_jump_kernel: the Lindblad batch at Np = 128 with ONE collapse operator,
// propagated in the eigenbasis of that operator, C = W diag(mu) W^-1 (host plan: pyqed_amd/oqs.py, EigJumpPlan).  With
// rho~ = W^-1 rho W^-+ and A~ = W^-1 A W, A = -iH - 1/2 C^+ C, the equation of motion is
//     d rho~/dt = X + X^+ + M o rho~ ,   X = A~ rho~ ,   M_ij = mu_i conj(mu_j)
// so the dissipator is elementwise and the A term is ONE full GEMM: 64 tile-GEMMs per stage (6,144 3-product MFMAs)
// for the 100 (9,600) of lindblad_eig_kernel, which diagonalises A and pays two GEMMs for the dissipator.  One
// persistent workgroup per matrix.
// A stage is the batch kernel's pipeline at n_c = 0 (glf_batch_kernel.hpp): the full GEMM on the Hermitian tile layout
// (cgemm_dma128.hpp), k = X + X^+ through herm_k_publish and the HermKL image, and the Horner update
//     rn_ij = a base_ij + hc k_ij
// on the elements on and above the diagonal, the mirror written as the conjugate and the diagonal's imaginary part
// dropped: every stage result is exactly Hermitian with an exactly real diagonal.  The elementwise term rides in the
// GEMM's accumulators: instead of from zero they start from T = M o r / 2 on all 64 tiles (jump_init_mr), so that
// X = T + A~ r and k_ij = X_ij + conj(X_ji) carries T_ij + conj(T_ji) = M_ij r_ij.  T is loaded straight into the
// registers the accumulators occupy anyway, under the DMA of the GEMM's first K-tile: the epilogue holds no r next to
// the accumulators and the base (five tiles of each spilled), and is the batch kernel's with a and the diagonal rule.
// The K loop stages each K-tile from inside the k-steps of the tile before (CgDmaStageHook), as lindblad_eig_kernel's
// engines do, with the operands named directly: no segment table.
// The same pass runs the two basis changes, rho~ = W^-1 rho W^-+ at the head and rho = W rho~ W^+ at the tail, each
// as Y = M r (64 tiles, stored) and X = Y (M^+ / 2) (64 tiles) with a = 0, T = 0, hc = 1: k = (Z + Z^+) / 2 for
// Z = M r M^+, Hermitian by construction; the multiplication by zero is exact on finite data.  128 tile-GEMMs per
// change, 4 % of a 20-step call.
// Only glf_eig_jump.hip includes this header: the neighbours' register allocation has changed with what shares their
// translation unit.  0 spilled VGPRs, 0 B scratch (tools/isa_diff.py).
#pragma once
#include "glf_herm_k.hpp"

namespace qd {

struct LindbladJumpParams {
  const c128* At;    // [128][128]      A~ = W^-1 A W (zero on the padding)
  const c128* W;     // [128][128]      W (identity on the padding), Wi = W^-1
  const c128* Wi;
  const c128* Wdh;   // [128][128]      W^+ / 2, Widh = W^-+ / 2
  const c128* Widh;
  const c128* mu;    // [128]           eigenvalues of C (zero on the padding)
  const c128* eT;    // [ne][128][128]  (W^+ E_m W)^T
  c128* rho;         // [B][128][128]   state (in/out, original basis)
  c128* ws;          // [B][2][128][128]  the Horner stages' two buffers; the first holds Y during a basis change
  c128* obs;         // [B][nsteps+1][ne]
  int ne, nsteps;
  double dt;
  unsigned long long* tbuf;  // [B][QD_TSTRIDE] per-phase ticks (QD_PHASE_TIMING diagnostics) or null
};

namespace {

constexpr int JUMP_NP = 128;
constexpr int JUMP_NPRE = 3;   // tiles whose base a wave loads ahead of the publishing barrier (HERM_K_NPRE: 4 spilled here)

// The accumulators of wave W's eight tiles set to T = M o r / 2, M_ij = mu_i conj(mu_j), in the 3-product form
// (P1, P2, P3) = (T_re, 0, T_re + T_im), which cg_dma_finalise turns into (T_re, T_im) plus the GEMM's sums.
// jump_r_loads: r on the wave's tiles in MFMA layout (addresses as in herm_k_rho_loads); jump_mu_reads: mu on the
// wave's column and row indices, out of LDS.
template <int W>
__device__ __forceinline__ void jump_r_loads(const c128* r, int Np, int lane, c128 (&rq)[8][4]) {
  const unsigned vu = (unsigned)((lane >> 4) * Np + (lane & 15)) * (unsigned)sizeof(c128);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (W >> 1) : 7 - (W >> 1), C = cg_herm_ctile(W, nj);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned su = (unsigned)((16 * R + 4 * e) * Np) * (unsigned)sizeof(c128);   // uniform
        rq[mi * 4 + nj][e] = *reinterpret_cast<const c128*>(reinterpret_cast<const char*>(r + 16 * C) + (vu + su));
      }
    }
}
template <int W>
__device__ __forceinline__ void jump_mu_reads(const c128* muS, int lane, c128 (&mj)[4], c128 (&mi_)[2][4]) {
#pragma unroll
  for (int nj = 0; nj < 4; ++nj) mj[nj] = muS[16 * cg_herm_ctile(W, nj) + (lane & 15)];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int e = 0; e < 4; ++e) mi_[mi][e] = muS[16 * (mi == 0 ? (W >> 1) : 7 - (W >> 1)) + (lane >> 4) + 4 * e];
}
__device__ __forceinline__ void jump_init_mr(CgAcc3& acc, c128 (&rq)[8][4], const c128 (&mj)[4],
                                             const c128 (&mi_)[2][4]) {
  // T in place of r first, tile by tile and pinned, then the three sets from it: formed in one sweep, the sets (192
  // VGPRs) grow next to r (128) and mu (48) and the sweep spills
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const c128 a = mi_[mi][e], b = mj[nj], x = rq[mi * 4 + nj][e];
        const double mre = 0.5 * (a.re * b.re + a.im * b.im), mim = 0.5 * (a.im * b.re - a.re * b.im);
        rq[mi * 4 + nj][e] = cmk(mre * x.re - mim * x.im, mre * x.im + mim * x.re);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(rq[mi * 4 + nj][e].re), "+v"(rq[mi * 4 + nj][e].im));
    }
  cg_sched_fence();
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const c128 t = rq[mi * 4 + nj][e];
        acc.re[mi][nj][e] = t.re;
        acc.im[mi][nj][e] = 0.0;
        acc.p3[mi * 4 + nj][e] = t.re + t.im;
      }
}

// One pass's GEMM for wave W: X = T + A B of depth Np on all 64 tiles of the Hermitian tile layout, T = M o r / 2 (mr)
// or zero.  Cold start: K-tile 0 by DMA and a barrier; every later K-tile is staged from inside the k-steps of the
// tile before it (CgDmaStageHook), and every tile-end barrier is s_waitcnt vmcnt(0) + barrier, as in
// cg_dma_herm_d_gemm_h.  WAR: the target buffer has been free since the tile-end barrier before; RAW: the issuing
// wave's tile-end wait, then the barrier.
// Order inside the prologue: r to registers and mu out of LDS FIRST, then the DMA of K-tile 0, then the arithmetic
// under it -- an LDS read issued behind an LDS-DMA load gets the compiler's s_waitcnt vmcnt(0) in front of it
// (tools/dma_waits.py), the global loads in front do not mind.  Called from a per-wave code path by all threads; ends
// with a workgroup barrier; the accumulators are finalised.
template <int W>
__device__ __forceinline__ void jump_gemm(const c128* A, const c128* B, const c128* r, bool mr, const c128* muS, int Np,
                                          int lane, CgLds<128>& L, CgAcc3& acc) {
  constexpr int NQ = CG_KT / 4, R0 = 16 * (W >> 1), R1 = 16 * (7 - (W >> 1));
  const int r0[2] = {R0, R1};
  const int c0[4] = {16 * cg_herm_ctile(W, 0), 16 * cg_herm_ctile(W, 1), 16 * cg_herm_ctile(W, 2),
                     16 * cg_herm_ctile(W, 3)};
  const int T = Np / CG_KT;
  const CgDmaStage st(nullptr, T, Np, Np);
  if (mr) {
    c128 rq[8][4], mj[4], mi_[2][4];
    jump_r_loads<W>(r, Np, lane, rq);
    jump_mu_reads<W>(muS, lane, mj, mi_);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // mu is out of LDS ahead of the DMA
    cg_sched_fence();
    st.issue_at(A, B, 0, L, 0);
    cg_sched_fence();
    jump_init_mr(acc, rq, mj, mi_);
  } else {
    st.issue_at(A, B, 0, L, 0);
    cg_dma_zero(acc);
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const bool more = t + 1 < T;
    const char* ga = more ? cg_uniform(A + (t + 1) * CG_KT) : nullptr;
    const char* gb = more ? cg_uniform(B + (size_t)(t + 1) * CG_KT * Np) : nullptr;
    const CgDmaStageHook hook{st, L, ga, gb, (t + 1) & 1};
    cg_sched_fence();
    cg_dma_ksteps<0u, 0, NQ>(L, t & 1, acc, r0, c0, hook);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  cg_dma_finalise(acc);
}

// herm_k_update (glf_herm_k.hpp) with the base scaled by a and the diagonal's imaginary part dropped:
// rn_ij = a base_ij + hc k_ij, k_ij = X_ij + conj(X_ji) from the HermKL image, rn_ji the conjugate.  The same
// addresses and the same order of loads and stores; the base of the tiles beyond the first NPRE is loaded behind the
// update of the tile that frees their registers, as there.
template <int W, int NPRE>
__device__ __forceinline__ void jump_update(const CgAcc<128>& A, const c128* KL, int lane, c128 (&q)[8][4],
                                            const c128* base, c128* rn, int Np, double a, double hc) {
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
      if (n >= 1) {
        cg_sched_fence();
        herm_k_rho_loads<W>(base, Np, lane, q, n - 1 + NPRE, n + NPRE);
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
        c128 v = cadd(cscale(q[mi * 4 + nj][r], a), cscale(k, hc));
        if (R == C && ra == lc) v.im = 0.0;
        const unsigned su = (unsigned)((16 * R + 4 * r) * Np) * (unsigned)sizeof(c128);   // uniform, as sm
        const unsigned sm = (unsigned)(16 * C * Np) * (unsigned)sizeof(c128);
        char* u = reinterpret_cast<char*>(rn + 16 * C) + (vu + su);
        char* t = reinterpret_cast<char*>(rn + 16 * R + 4 * r) + (vm + sm);
        if (R < C || ra <= lc) *reinterpret_cast<c128*>(u) = v;
        if (R < C || ra < lc) *reinterpret_cast<c128*>(t) = cconj(v);
      }
    }
}

// Y = M r of a basis change: wave W stores all eight of its tiles (addresses as in herm_k_rho_loads).
template <int W>
__device__ __forceinline__ void jump_store_y(const CgAcc<128>& A, c128* Y, int Np, int lane) {
  const unsigned vu = (unsigned)((lane >> 4) * Np + (lane & 15)) * (unsigned)sizeof(c128);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (W >> 1) : 7 - (W >> 1), C = cg_herm_ctile(W, nj);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned su = (unsigned)((16 * R + 4 * e) * Np) * (unsigned)sizeof(c128);   // uniform
        *reinterpret_cast<c128*>(reinterpret_cast<char*>(Y + 16 * C) + (vu + su)) = cmk(A.re[mi][nj][e], A.im[mi][nj][e]);
      }
    }
}

__global__ __launch_bounds__(CG_WG) void lindblad_eig_jump_kernel(LindbladJumpParams p) {
  constexpr int BT = JUMP_NP;
  constexpr size_t NN = (size_t)JUMP_NP * JUMP_NP;
  // the dimension as a run-time value, as in the batch kernel: with a constant the K loop is unrolled, and the
  // compiler then orders each tile's fragment reads behind the LDS-DMA loads of the tile before (tools/dma_waits.py)
  int Np = JUMP_NP;
  asm volatile("" : "+s"(Np));
  __shared__ CgLds<BT> L;
  __shared__ c128 sred[CG_WG / 64];
  __shared__ c128 muS[JUMP_NP];

  const int b = blockIdx.x;
  c128* rho = p.rho + (size_t)b * NN;
  c128* ws = p.ws + (size_t)b * 2 * NN;
  c128* rbuf1 = ws + NN;
  c128* obs = p.obs ? p.obs + (size_t)b * (p.nsteps + 1) * p.ne : nullptr;
  if (threadIdx.x < JUMP_NP) muS[threadIdx.x] = p.mu[threadIdx.x];
  __syncthreads();

  CgAcc3 A;
  QD_TIMING_DECL
#ifdef QD_PHASE_TIMING
  unsigned long long txf = 0;   // the basis changes' ticks, charged to slot 0 instead of the stages' slots
#endif

  // Pass `it` of the call, each ONE full GEMM on the Hermitian tile layout and one tail, on one per-wave code path:
  //   0              Y = W^-1 rho -> ws                  4 nsteps + 2   Y = W rho~ -> ws
  //   1              rho~ = sym(Y W^-+) -> rho           4 nsteps + 3   rho = sym(Y W^+) -> rho
  //   2 .. 4 nsteps + 1   the Horner stages (glf_horner_coef), stage = (it - 2) & 3: rho~ -> s1 -> s2 -> s3 -> rho~ over
  //                  ws and rbuf1 as in the batch kernel, so a stage never writes the buffer its GEMM and its
  //                  elementwise term read
  // sym(Z) = (Z + Z^+) / 2 is a stage with a = 0, T = 0, hc = 1 and the halved dagger as the B operand.
  const int nit = 4 * p.nsteps + 4;
  for (int it = 0; it < nit; ++it) {
    const bool xf = it < 2 || it >= nit - 2, ypass = it == 0 || it == nit - 2;
    const int stage = (it - 2) & 3;
    const c128* r = (xf || stage == 0) ? rho : ((stage - 1) & 1) ? rbuf1 : ws;
    c128* rn = (xf || stage == 3) ? rho : (stage & 1) ? rbuf1 : ws;
    const c128* oa = it == 0 ? p.Wi : it == nit - 2 ? p.W : xf ? ws : p.At;
    const c128* ob = it == 1 ? p.Widh : it == nit - 1 ? p.Wdh : r;
    double dts = p.dt;
    asm volatile("" : "+s"(dts));   // per pass: no coefficient register held across the K loop
    const double hc = wave_uniform(xf ? 1.0 : glf_horner_coef(dts, stage)), ab = wave_uniform(xf ? 0.0 : 1.0);
#ifdef QD_PHASE_TIMING
    unsigned long long tkeep[6] = {tacc[0], tacc[1], tacc[2], tacc[3], tacc[4], tacc[5]};
#endif
    // k = X + X^+ as in the batch kernel: conj(X) below the diagonal published at the mirror slot of the HermKL image,
    // the base of the update loaded into the registers the publishing freed, ONE barrier, then the update on the
    // elements on and above the diagonal.  rn is never r; at stage 3 and in a basis change rn == base == rho
    // and every element and its mirror are read and written by one thread, loads first.  The closing barrier keeps the
    // next pass's LDS-DMA out of the image and makes rn (or Y) complete for it and for the observables.
    {
      static_assert(HermKL::SIZE * sizeof(c128) <= sizeof(CgLds<BT>), "LDS k image");
      c128* KL = reinterpret_cast<c128*>(&L);
      const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
      auto pass = [&](auto wc) {
        constexpr int W = decltype(wc)::value;
        {
          int tid = threadIdx.x;
          asm volatile("" : "+v"(tid));   // the prologue's index math stays inside the pass (no LICM + spill) ...
          jump_gemm<W>(oa, ob, r, !xf, muS, Np, tid & 63, L, A);
        }
        QD_TMARK(2);
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));   // ... and the tail's is made behind the K loop, not held across it
        const int lane = tid & 63;
        int Npe = Np;
        asm volatile("" : "+s"(Npe));   // the uniform row offsets are made here, not held across the K loop
        if (ypass) {
          jump_store_y<W>(A, ws, Npe, lane);
          return;
        }
        c128 q[8][4];
        herm_k_publish<W>(A, KL, lane);
        cg_sched_fence();   // the loads go into the registers the publishing frees
        herm_k_rho_loads<W>(rho, Npe, lane, q, 0, JUMP_NPRE);
        __syncthreads();
        QD_TMARK(5);
        jump_update<W, JUMP_NPRE>(A, KL, lane, q, rho, rn, Npe, ab, hc);
      };
#define QD_JW(w) \
  case w: pass(std::integral_constant<int, w>{}); break;
      switch (wave) { QD_JW(0) QD_JW(1) QD_JW(2) QD_JW(3) QD_JW(4) QD_JW(5) QD_JW(6) default: QD_JW(7) }
#undef QD_JW
      __syncthreads();
    }
    QD_TMARK(3);
#ifdef QD_PHASE_TIMING
    if (xf)
      for (int q = 0; q < 6; ++q) {
        txf += tacc[q] - tkeep[q];
        tacc[q] = tkeep[q];
      }
#endif
    // observables on rho~: t0 behind the first change and the end of every step (behind the closing barrier above)
    if (p.ne > 0 && (it == 1 || (!xf && stage == 3))) {
      wg_observables_batch(rho, p.eT, p.ne, NN, obs + (size_t)((it - 1) / 4) * p.ne, sred);
      QD_TMARK(4);
    }
  }
#ifdef QD_PHASE_TIMING
  tacc[0] += txf;
#endif
  QD_TIMING_FLUSH
}

}  // namespace
}  // namespace qd
