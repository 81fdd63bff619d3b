// glf_batch_kernel.hpp — the Lindblad batch kernel lindblad_rk4_kernel<128, true, true, false> (the headline one):
// the persistent Hermitian kernel at Np = 128 for Lindblad operands (sum_c C_c r C_c^+ / 2 Hermitian), an explicit
// specialization of glf_kernel.hpp's template on an engine of its own (cgemm_dma128.hpp).  Only glf.hip includes it:
// its register allocation sits on the 256-VGPR wall (0 spilled, 0 B scratch) and has changed with its neighbours in
// the translation unit and with statements moved into helpers.  After any edit compare assembly and resource figures
// with tools/isa_diff.py; a build that spills a VGPR or uses scratch is not a candidate.
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

// Pass A (PB = false) / pass B (PB = true) of k = X + X^+ into the LDS k buffers (see the kernel) for wave W of the
// Hermitian tile layout (cgemm_dma128.hpp).  Tile (R, C) of 16 x 16 lies in 64 x 64 quadrant (R / 4, C / 4); only the
// diagonal 16 x 16 tiles need per-element tests, every other tile is wholly upper (pass A stores), wholly lower (pass B
// adds the conjugate at the mirror slot) or in the lower-left quadrant (pass B into T01 transposed).  The wave's tile
// roles are compile-time constants: no per-element index arithmetic or branches.
template <int W, bool PB, typename Slot>
__device__ __forceinline__ void herm_k_pass(const CgAcc<128>& A, c128* T01, c128* Tt, int lane, Slot&& slot) {
  constexpr int LD = HermK<64>::LD, TRI = HermK<64>::TRI;
  const int lr = lane >> 4, lc = lane & 15;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = mi == 0 ? (W >> 1) : 7 - (W >> 1), C = cg_herm_ctile(W, nj);   // constants after unrolling
      const int QR = R >> 2, QC = C >> 2, rr = (R & 3) * 16, c0 = (C & 3) * 16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const c128 v = cmk(A.re[mi][nj][r], A.im[mi][nj][r]);
        const int ra = rr + lr + 4 * r, cc = c0 + lc;
        if (QR < QC) {
          if (!PB) T01[ra * LD + cc] = v;
        } else if (QR > QC) {
          if (PB) {
            c128* t = &T01[cc * LD + ra];
            *t = cadd(*t, cconj(v));
          }
        } else if ((R & 3) < (C & 3)) {
          if (!PB) Tt[QR * TRI + slot(ra, cc)] = v;
        } else if ((R & 3) > (C & 3)) {
          if (PB) {
            c128* t = &Tt[QR * TRI + slot(cc, ra)];
            *t = cadd(*t, cconj(v));
          }
        } else if (!PB) {
          if (ra < cc) Tt[QR * TRI + slot(ra, cc)] = v;
          else if (ra == cc) Tt[QR * TRI + slot(ra, cc)] = cadd(v, cconj(v));
        } else if (ra > cc) {
          c128* t = &Tt[QR * TRI + slot(cc, ra)];
          *t = cadd(*t, cconj(v));
        }
      }
    }
}

template <>
__global__ __launch_bounds__(CG_WG) void lindblad_rk4_kernel<128, true, true, false>(LindbladParams p) {
  constexpr int BT = 128;
  if (p.guard && __hip_atomic_load(p.guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  __shared__ CgLds<BT> L;
  __shared__ c128 sred[CG_WG / 64];
  __shared__ CgSeg segs[2 + MAX_NC];   // segment table in LDS (no scratch)

  const int b = blockIdx.x;
  const int Np = p.Np, nc = p.nc;
  const size_t NN = (size_t)Np * Np;
  c128* rho = p.rho + (size_t)b * NN;
  // single block: always true here (launched at Np == 128 only), tested at run time as in glf_kernel.hpp's template
  const bool single = (Np / BT) == 1;
  c128* ws = p.ws + (size_t)b * glf_slots(Np, nc) * NN;
  c128* rbuf1 = single ? ws : ws + NN;
  c128* Y = single ? ws + NN : ws + 2 * NN;
  c128* obs = p.obs ? p.obs + (size_t)b * (p.total_steps + 1) * p.ne : nullptr;

  if (p.ne > 0 && p.step0 == 0) wg_observables(rho, p.eT, p.ne, NN, obs, sred);
  __syncthreads();

  const double dt = p.dt;
  CgAcc3 A;
  QD_TIMING_DECL

  for (int step = 0; step < p.nsteps; ++step) {
    for (int stage = 0; stage < 4; ++stage) {
      // Horner stages (glf_horner_coef): rho -> s1 -> s2 -> s3 -> rho; single block: s_m in place in ws
      const c128* r = stage == 0 ? rho : ((stage - 1) & 1) ? rbuf1 : ws;
      c128* rn = stage == 3 ? rho : (stage & 1) ? rbuf1 : ws;
      const double hc = wave_uniform(glf_horner_coef(dt, stage));   // the stages' coefficients stay out of the VGPRs
      // Hermitian rho: L[rho] = X + X^+ with X = (-iK) r + sum_c (C_c r)(C_c^+ / 2)   (single block; p.Cd holds
      // C_c^+ / 2 on this path).  phase 1: Y_c = C_c r
      // One K-tile stream per stage: Y_0 .. Y_{nc-1}, then X.  The X GEMM's segment table is written here, once;
      // the Y GEMMs name their operands directly and never read it.  The last K-tile of each GEMM stages tile 0 of
      // the next one (Y_{c+1}: (C_{c+1}, r); after the last c the X GEMM's (mK, r)), both known before the stage
      // starts, so only the stage's first GEMM pays a cold tile.
      // Invariants (keep ALL of these when editing):
      //  (1) the table's first reader is the X GEMM's issue(1) at the top of its tile 0, at least Np / 16 tile-end
      //      barriers after thread 0's writes (nc = 0: the barrier below); its last reader in the stage before is
      //      separated from these writes by the barriers of the k passes;
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
      if (threadIdx.x == 0) {
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
      // k = X + X^+ formed in the LDS k buffers on the upper triangle only, as in the register-staged Hermitian kernel
      // (glf_kernel.hpp): pass A stores the accumulator's upper elements, pass B adds the conjugate of every lower one
      // at its mirror slot (herm_k_pass); the Horner update reads rho on the upper triangle and writes both triangles.
      {
        using KB = HermK<BT / 2>;
        constexpr int TS = BT / 2, LD = KB::LD, TRI = KB::TRI;
        static_assert((TS * LD + 2 * TRI) * sizeof(c128) <= sizeof(CgLds<BT>), "LDS k buffers");
        c128* T01 = reinterpret_cast<c128*>(&L);
        c128* Tt = T01 + TS * LD;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));  // keep the per-element index math inside the stage loop (no LICM + spill)
        auto slot = [&](int ra, int cc) { return KB::slot(ra, cc); };
        // Every rho element the thread updates (8 of tile (0, 1), 9 of the folded triangles) is loaded once its
        // accumulator is dead, before the barrier that publishes pass B: one load latency per stage, most of it under
        // that barrier, instead of one per chunk behind it.  At stage 3 (rn == rho) every element and its mirror are
        // read and written by one thread, loads first.
        constexpr int NP0 = TS * TS / CG_WG, NP1 = (2 * TRI + CG_WG - 1) / CG_WG;
        static_assert(TS * TS % CG_WG == 0, "tile (0, 1) in whole rounds of the workgroup");
        c128 q0[NP0], q1[NP1];
        auto rho_prefetch = [&]() {
#pragma unroll
          for (int q = 0; q < NP0; ++q) {
            const int e = tid + CG_WG * q;
            q0[q] = rho[(e / TS) * Np + TS + e % TS];
          }
#pragma unroll
          for (int q = 0; q < NP1; ++q) {   // the last round is partial: clamped, so that no load sits in a branch
            int gi, gj;
            KB::place<1>(T01, Tt, min(tid + CG_WG * q, 2 * TRI - 1), gi, gj);
            q1[q] = rho[gi * Np + gj];
          }
        };
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = tid & 63;
        auto pass = [&](auto pbc) {
          constexpr bool PB = decltype(pbc)::value;
#define QD_KW(w) \
  case w: herm_k_pass<w, PB>(A, T01, Tt, lane, slot); break;
          switch (wave) { QD_KW(0) QD_KW(1) QD_KW(2) QD_KW(3) QD_KW(4) QD_KW(5) QD_KW(6) default: QD_KW(7) }
#undef QD_KW
        };
        pass(std::false_type{});
        __syncthreads();
        pass(std::true_type{});
        rho_prefetch();
        __syncthreads();
        QD_TMARK(5);
        // Horner update of one upper element (i, j) with k, writing the mirror (j, i) as the conjugate; one chunk per
        // round, its rho values loaded already
        auto update = [&](int gi, int gj, c128 k, c128 r0v) {
          const int id = gi * Np + gj, mid = gj * Np + gi;
          const c128 v = cadd(r0v, cscale(k, hc));
          rn[id] = v;
          if (gi != gj) rn[mid] = cconj(v);
        };
        auto round = [&](auto rdc) {
          constexpr int rd = decltype(rdc)::value;
          constexpr int NE = rd == 0 ? TS * TS : 2 * TRI;
          constexpr int NPER = (NE + CG_WG - 1) / CG_WG;
#pragma unroll
          for (int q = 0; q < NPER; ++q) {
            const int e = tid + CG_WG * q;
            if (NE % CG_WG != 0 && e >= NE) continue;
            int gi, gj;
            const c128 k = *KB::place<rd>(T01, Tt, e, gi, gj);
            if constexpr (rd == 0) update(gi, gj, k, q0[q]);
            else update(gi, gj, k, q1[q]);
          }
        };
        round(std::integral_constant<int, 0>{});
        round(std::integral_constant<int, 1>{});
        __syncthreads();
      }
      QD_TMARK(3);
    }
    const int gs = p.step0 + step + 1;  // global step count after this step
    if (p.ne > 0) wg_observables(rho, p.eT, p.ne, NN, obs + (size_t)gs * p.ne, sred);
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
