// glf_kernel.hpp — the persistent GLF / Lindblad RK4 kernel (lindblad_rk4_kernel) and its parameter block,
// shared by glf.hip (every nc <= MAX_NC instantiation) and glf_chunk.hip (the CHUNK instantiations for longer
// collapse-operator lists).  The CHUNK kernels live in their own translation unit: instantiated next to the
// headline kernel they changed its register allocation (12 B per lane of scratch instead of 0).
// This header holds the general kernel and the register-staged Hermitian kernel; the Lindblad batch kernel
// <128, true, true, false> is an explicit specialization in glf_batch_kernel.hpp (glf.hip only).  Algorithm: glf.hip.
#pragma once
#include "cgemm_block.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace qd {

struct LindbladParams {
  const c128* Cop;  // [nc][Np][Np]  L_c   (Lindblad: C_c)
  const c128* mK;   // [Np][Np]      P     (Lindblad: -iK)
  const c128* iKd;  // [Np][Np]      Q     (Lindblad: iH - S/2)
  const c128* Cd;   // [nc][Np][Np]  R_c   (Lindblad: C_c^+)
  const c128* eT;   // [ne][Np][Np]  E_m^T
  c128* rho;        // [B][Np][Np]   state (in/out)
  c128* ws;         // [B][3+nc][Np][Np] scratch
  c128* obs;        // [B][nsteps+1][ne]
  c128* snap;       // [B][nsave][N][N]
  int N, Np, nc, ne, nsteps, save_every, nsave;
  int step0, total_steps;  // this launch runs global steps step0 .. step0+nsteps-1 of total_steps
  int herm;                // Hermitian fast path (Lindblad, rho exactly Hermitian, single block)
  int hseg;                // Hermitian path: sum_c L_c r W_c is itself Hermitian (Lindblad C r C^+ / 2; not Redfield's
                           // sum A r Lam^+), so its redundant tiles below the diagonal may be skipped (cg_dma_herm_x_gemm)
  double dt;
  unsigned long long* tbuf;  // [B][QD_TSTRIDE] per-phase wall-clock ticks (QD_PHASE_TIMING diagnostics) or null
  int stage, rin, rout;        // split path: RK4 stage; stage input / output buffer (0 = rho, 1/2 = scratch 0/1)
  int ks, ys;                  // split path: K-splits of the k / Y phases (1 = none)
  c128* kslab;                 // [B][nb^2][ks][BT^2] partial k blocks
  c128* yslab;                 // [B][nc][nb^2][ys][BT^2] partial Y blocks
  unsigned* ticket;            // [B][1 + nc][nb^2] arrival counters (zero between launches)
  const int* guard;            // persistent kernel: run only if *guard != 0 (the single launch's fallback), or null
};

namespace {

constexpr int MAX_NC = 256;  // collapse-operator / GLF pair segments held in the kernels' LDS segment tables (4 KB);
                             // longer lists run the persistent kernels' CHUNK instantiations (chunks of MAX_NC)

// Per-matrix scratch slots of Np x Np: stage buffer(s), Y_c.
__host__ __device__ inline int glf_slots(int Np, int nc) { return (Np <= 128 ? 1 : 2) + nc; }

// Horner coefficient of RK4 stage m (0..3): s_{m+1} = rho + dt / (4 - m) L s_m  (see the file header)
__device__ __forceinline__ double glf_horner_coef(double dt, int stage) { return rk4_horner_coef(dt, stage); }

// A workgroup's row of tbuf: 6 phase slots (wall-clock ticks between barrier marks), 12 K-loop slots (shader cycles
// between per-wave stamps, no barrier in front: lindblad_eig_kernel, 6 of wave 0 then 6 of wave 4), shader and wall clock.
constexpr int QD_TSTRIDE = 24, QD_TKLOOP = 6, QD_TCLK = 22, QD_TWALL = 23;

#ifdef QD_PHASE_TIMING
// Diagnostics only (p.tbuf != null): barrier, then thread 0 charges the ticks since the last mark to `slot`.
#define QD_TMARK(slot)                                   \
  if (p.tbuf) {                                          \
    __syncthreads();                                     \
    if (threadIdx.x == 0) {                              \
      const unsigned long long now_ = wall_clock64();    \
      tacc[slot] += now_ - tlast;                        \
      tlast = now_;                                      \
    }                                                    \
  }
#define QD_TIMING_DECL                                                                \
  unsigned long long tacc[6] = {0, 0, 0, 0, 0, 0}, tlast = p.tbuf ? wall_clock64() : 0; \
  unsigned long long tk[6] = {0, 0, 0, 0, 0, 0};   /* this wave's K-loop stamps (cgemm_dma128.hpp) */ \
  const unsigned long long t0w_ = tlast, t0c_ = clock64();
#define QD_TIMING_FLUSH                                                                       \
  if (p.tbuf && (threadIdx.x & 255) == 0)                                                     \
    for (int q = 0; q < 6; ++q) p.tbuf[(size_t)b * QD_TSTRIDE + QD_TKLOOP + (threadIdx.x >> 8) * 6 + q] += tk[q]; \
  if (p.tbuf && threadIdx.x == 0) {                                                           \
    for (int q = 0; q < 6; ++q) p.tbuf[(size_t)b * QD_TSTRIDE + q] += tacc[q];               \
    p.tbuf[(size_t)b * QD_TSTRIDE + QD_TCLK] += clock64() - t0c_;                             \
    p.tbuf[(size_t)b * QD_TSTRIDE + QD_TWALL] += wall_clock64() - t0w_;                       \
  }
#else
#define QD_TMARK(slot)
#define QD_TIMING_DECL
#define QD_TIMING_FLUSH
#endif

// Tr(E_m rho) = sum_ij rho_ij E_m[j][i] = sum_ij rho_ij eT_m[i][j]; fixed
// reduction order (per-thread strided partials, wave butterfly, 8-wave sum).
__device__ void wg_observables(const c128* rho, const c128* eT, int ne, size_t NN, c128* out, c128* sred) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // per call: the per-thread addresses are not kept in registers across a step's GEMMs
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
      sr += __shfl_xor(sr, off, 64);
      si += __shfl_xor(si, off, 64);
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

// LDS k buffers of the Hermitian kernels (TS = BT / 2): T01 [TS][TS + 1] holds tile (0, 1) of k = X + X^+, Tt the upper
// triangles of the two diagonal tiles, packed and folded (rows u and TS - 1 - u of a tile share one run of TS + 1 slots).
template <int TS>
struct HermK {
  static constexpr int LD = TS + 1, TRI = TS * (TS + 1) / 2;
  // folded packed slot of (ra, cc), ra <= cc, within a diagonal tile
  static __device__ __forceinline__ int slot(int ra, int cc) {
    const bool top = ra < TS / 2;
    const int u = top ? ra : TS - 1 - ra;
    return u * (TS + 1) + (top ? 0 : TS - u) + (cc - ra);
  }
  // Element e of update round RD: its place (gi, gj) in rho, returning where its k lies.  Round 0: tile (0, 1),
  // e -> (e / TS, TS + e % TS), k in T01; round 1: the two folded diagonal triangles, k at Tt[e]
  template <int RD>
  static __device__ __forceinline__ const c128* place(const c128* T01, const c128* Tt, int e, int& gi, int& gj) {
    if (RD == 0) {
      gi = e / TS;
      gj = TS + e % TS;
      return &T01[gi * LD + e % TS];
    }
    const int ts = e / TRI, ff = e % TRI, u = ff / (TS + 1), v = ff % (TS + 1);
    const bool lo = v < TS - u;
    const int ra = lo ? u : TS - 1 - u;
    gi = ts * TS + ra;
    gj = ts * TS + (lo ? u + v : ra + v - (TS - u));
    return &Tt[e];
  }
};

// HERM: rho exactly Hermitian (single block, Np == BT), L[rho] = X + X^+; else the general form.
// HSEG (Hermitian, BT = 128, not CHUNK): sum_c L_c r W_c is itself Hermitian (Lindblad C r C^+ / 2), so the X GEMM
// skips its tiles below the diagonal: the Lindblad batch kernel, a specialization of its own (glf_batch_kernel.hpp).
// Without it (Redfield's GLF operands, the CHUNK kernels) the Hermitian kernel runs the plain X GEMM.
// CHUNK (nc > MAX_NC only; the nc <= MAX_NC instantiations are compiled without it): the segment lists of the X / k
// GEMMs run in chunks of MAX_NC collapse-operator segments through the LDS table, accumulating in registers.
template <int BT, bool HERM, bool HSEG = false, bool CHUNK = false>
__global__ __launch_bounds__(CG_WG) void lindblad_rk4_kernel(LindbladParams p) {
  static_assert(!HSEG, "HSEG exists as <128, true, true, false> only: glf_batch_kernel.hpp, included by glf.hip");
  if (p.guard && __hip_atomic_load(p.guard, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  __shared__ CgLds<BT> L;
  __shared__ c128 sred[CG_WG / 64];
  __shared__ CgSeg segs[2 + MAX_NC];   // segment table in LDS (no scratch)

  const int b = blockIdx.x;
  const int Np = p.Np, nc = p.nc;
  const size_t NN = (size_t)Np * Np;
  c128* rho = p.rho + (size_t)b * NN;
  // single block (Np <= 128): every stage input is fully consumed by the GEMMs before the epilogue
  // overwrites it, so one stage buffer is updated in place; else two alternate.
  const bool single = (Np / BT) == 1;
  c128* ws = p.ws + (size_t)b * glf_slots(Np, nc) * NN;
  c128* rbuf1 = single ? ws : ws + NN;
  c128* Y = single ? ws + NN : ws + 2 * NN;
  c128* obs = p.obs ? p.obs + (size_t)b * (p.total_steps + 1) * p.ne : nullptr;

  if (p.ne > 0 && p.step0 == 0) wg_observables(rho, p.eT, p.ne, NN, obs, sred);
  __syncthreads();

  const int nb = Np / BT;
  const double dt = p.dt;
  CgAcc<BT> A;
  QD_TIMING_DECL

  for (int step = 0; step < p.nsteps; ++step) {
    for (int stage = 0; stage < 4; ++stage) {
      // Horner stages (glf_horner_coef): rho -> s1 -> s2 -> s3 -> rho; single block: s_m in place in ws
      const c128* r = stage == 0 ? rho : ((stage - 1) & 1) ? rbuf1 : ws;
      c128* rn = stage == 3 ? rho : (stage & 1) ? rbuf1 : ws;
      double hc = glf_horner_coef(dt, stage);
      auto rk4_update = [&](size_t idx, c128 k) { rn[idx] = cadd(rho[idx], cscale(k, hc)); };
      if constexpr (HERM) {
        // Hermitian rho: L[rho] = X + X^+ with X = (-iK) r + sum_c (C_c r)(C_c^+ / 2)   (single block, nb == 1;
        // p.Cd holds C_c^+ / 2 on this path).  phase 1: Y_c = C_c r
        for (int c = 0; c < nc; ++c) {
          if (threadIdx.x == 0) {
            segs[0].A = p.Cop + (size_t)c * NN;
            segs[0].B = r;
          }
          __syncthreads();
          cg_block_gemm<BT>(segs, 1, Np, Np, Np, L, A);
          QD_TMARK(0);
          c128* Yc = Y + (size_t)c * NN;
          cg_epilogue<BT>(A, [&](int row, int col, c128 v) { Yc[(size_t)row * Np + col] = v; });
          QD_TMARK(1);
        }
        __syncthreads();
        // phase 2: X in registers (one accumulator over 1 + nc segments); k_ij = X_ij + conj(X_ji) is
        // formed from the accumulator and an LDS transpose: exactly Hermitian, fused RK4 epilogue
        constexpr bool QUAD = BT == 128;   // the X GEMM on the quadrant layout (cgemm_block.hpp)
        if constexpr (!CHUNK) {
          if (threadIdx.x == 0) {
            segs[0].A = p.mK;
            segs[0].B = r;
            for (int c = 0; c < nc; ++c) {
              segs[1 + c].A = Y + (size_t)c * NN;
              segs[1 + c].B = p.Cd + (size_t)c * NN;
            }
          }
          __syncthreads();
          if constexpr (QUAD) cg_quad_x_gemm(segs, 1 + nc, Np, Np, Np, L, A);
          else cg_block_gemm<BT>(segs, 1 + nc, Np, Np, Np, L, A);
        } else {
          for (int c0 = 0; c0 < nc; c0 += MAX_NC) {   // (P r) + the first MAX_NC segments, then MAX_NC at a time
            const int first = c0 == 0 ? 1 : 0, cn = min(MAX_NC, nc - c0);
            if (threadIdx.x == 0) {
              segs[0].A = p.mK;
              segs[0].B = r;
              for (int c = 0; c < cn; ++c) {
                segs[first + c].A = Y + (size_t)(c0 + c) * NN;
                segs[first + c].B = p.Cd + (size_t)(c0 + c) * NN;
              }
            }
            __syncthreads();
            if constexpr (QUAD) cg_quad_x_gemm(segs, first + cn, Np, Np, Np, L, A, first);
            else cg_block_gemm<BT>(segs, first + cn, Np, Np, Np, L, A, first);
          }
        }
        auto visit = [&](auto&& f) {
          if constexpr (QUAD) cg_quad_epilogue(A, f);
          else cg_epilogue<BT>(A, f);
        };
        QD_TMARK(2);
        // k = X + X^+ formed in LDS on the upper triangle only (TS = BT/2; the GEMM staging buffers are free).
        // Every stage quantity is exactly Hermitian (k_ji = conj(k_ij) bit for bit, and the RK4 updates are
        // elementwise with real coefficients), so each (i, j), i <= j, is computed once and its mirror written as
        // the conjugate.  Pass A stores the accumulator's upper elements into the k buffers (HermK: T01, Tt);
        // pass B adds the conjugate of every lower element at its mirror slot.  The accumulator
        // stays in registers through both passes (no global round trip of the diagonal tiles).  The Horner update then
        // reads rho on the upper triangle only and writes the next stage input (rho at stage 3) in full (the GEMMs,
        // observables and the caller read it).
        {
          using KB = HermK<BT / 2>;
          constexpr int TS = BT / 2, LD = KB::LD, TRI = KB::TRI;
          static_assert((TS * LD + 2 * TRI) * sizeof(c128) <= sizeof(CgLds<BT>), "LDS k buffers");
          constexpr int EPI_PRE = 4;   // rho loads of round 0's first chunk issued before the LDS passes
          constexpr int EPI_CH = 8;    // rho loads in flight per chunk of the Horner update (r06 epilogue_knobs.txt)
          c128* T01 = reinterpret_cast<c128*>(&L);
          c128* Tt = T01 + TS * LD;
          int tid = threadIdx.x;
          asm volatile("" : "+v"(tid));  // keep the per-element index math inside the stage loop (no LICM + spill)
          constexpr int NPER0 = (TS * TS + CG_WG - 1) / CG_WG;
          constexpr int CH0 = NPER0 < EPI_CH ? NPER0 : EPI_CH;
          constexpr int NPRE = EPI_PRE < CH0 ? EPI_PRE : CH0;   // prefetched elements per thread
          c128 pre[NPRE];
#pragma unroll
          for (int q = 0; q < NPRE; ++q) {   // round 0's first chunk (tile (0, 1): e -> (e / TS, TS + e % TS))
            const int e = tid + CG_WG * q;
            if (e < TS * TS) pre[q] = rho[(e / TS) * Np + TS + e % TS];
          }
          visit([&](int row, int col, c128 v) {
            const int ti = row / TS, tj = col / TS, ra = row - ti * TS, cc = col - tj * TS;
            if (ti < tj) T01[ra * LD + cc] = v;
            else if (ti == tj && ra < cc) Tt[ti * TRI + KB::slot(ra, cc)] = v;
            else if (ti == tj && ra == cc) Tt[ti * TRI + KB::slot(ra, cc)] = cadd(v, cconj(v));
          });
          __syncthreads();
          visit([&](int row, int col, c128 v) {
            const int ti = row / TS, tj = col / TS, ra = row - ti * TS, cc = col - tj * TS;
            c128* t = ti > tj ? &T01[cc * LD + ra] : (ti == tj && ra > cc) ? &Tt[ti * TRI + KB::slot(cc, ra)] : nullptr;
            if (t) *t = cadd(*t, cconj(v));
          });
          __syncthreads();
          QD_TMARK(5);
          // Horner update of one upper element (i, j) with k, writing the mirror (j, i) as the conjugate
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
            constexpr int CH = NPER < EPI_CH ? NPER : EPI_CH;
            for (int qb = 0; qb < NPER; qb += CH) {
              c128 r0[CH];
#pragma unroll
              for (int q = 0; q < CH; ++q) {
                const int e = tid + CG_WG * (qb + q);
                if (qb + q < NPER && (NE % CG_WG == 0 || e < NE)) {
                  int gi, gj;
                  KB::template place<rd>(T01, Tt, e, gi, gj);
                  if (rd == 0 && qb == 0 && q < NPRE) r0[q] = pre[q < NPRE ? q : 0];
                  else r0[q] = rho[gi * Np + gj];
                }
              }
#pragma unroll
              for (int q = 0; q < CH; ++q) {
                const int e = tid + CG_WG * (qb + q);
                if (qb + q >= NPER || (NE % CG_WG != 0 && e >= NE)) continue;
                int gi, gj;
                const c128 k = *KB::template place<rd>(T01, Tt, e, gi, gj);
                update(gi, gj, k, r0[q]);
              }
            }
          };
          round(std::integral_constant<int, 0>{});
          round(std::integral_constant<int, 1>{});
          __syncthreads();
        }
        QD_TMARK(3);
        continue;
      } else {
      // ---- phase 1: Y_c = C_c r
      for (int c = 0; c < nc; ++c) {
        for (int bm = 0; bm < nb; ++bm)
          for (int bn = 0; bn < nb; ++bn) {
            if (threadIdx.x == 0) {
              segs[0].A = p.Cop + (size_t)c * NN + (size_t)bm * BT * Np;
              segs[0].B = r + bn * BT;
            }
            __syncthreads();
            cg_block_gemm<BT>(segs, 1, Np, Np, Np, L, A);
            QD_TMARK(0);
            c128* Yc = Y + (size_t)c * NN;
            cg_epilogue<BT>(A, [&](int row, int col, c128 v) {
              Yc[(size_t)(bm * BT + row) * Np + bn * BT + col] = v;
            });
            QD_TMARK(1);
          }
      }
      __syncthreads();
      // ---- phase 2: k = (-iK) r + r (iK^+) + sum_c Y_c C_c^+ ; RK4 epilogue
      for (int bm = 0; bm < nb; ++bm)
        for (int bn = 0; bn < nb; ++bn) {
          if constexpr (!CHUNK) {
            if (threadIdx.x == 0) {
              segs[0].A = p.mK + (size_t)bm * BT * Np;
              segs[0].B = r + bn * BT;
              segs[1].A = r + (size_t)bm * BT * Np;
              segs[1].B = p.iKd + bn * BT;
              for (int c = 0; c < nc; ++c) {
                segs[2 + c].A = Y + (size_t)c * NN + (size_t)bm * BT * Np;
                segs[2 + c].B = p.Cd + (size_t)c * NN + bn * BT;
              }
            }
            __syncthreads();
            cg_block_gemm<BT>(segs, 2 + nc, Np, Np, Np, L, A);
          } else {
            for (int c0 = 0; c0 < nc; c0 += MAX_NC) {   // (P r, r Q) + the first MAX_NC pairs, then MAX_NC at a time
              const int first = c0 == 0 ? 2 : 0, cn = min(MAX_NC, nc - c0);
              if (threadIdx.x == 0) {
                segs[0].A = p.mK + (size_t)bm * BT * Np;
                segs[0].B = r + bn * BT;
                segs[1].A = r + (size_t)bm * BT * Np;
                segs[1].B = p.iKd + bn * BT;
                for (int c = 0; c < cn; ++c) {
                  segs[first + c].A = Y + (size_t)(c0 + c) * NN + (size_t)bm * BT * Np;
                  segs[first + c].B = p.Cd + (size_t)(c0 + c) * NN + bn * BT;
                }
              }
              __syncthreads();
              cg_block_gemm<BT>(segs, first + cn, Np, Np, Np, L, A, first != 0);
            }
          }
          QD_TMARK(2);
          cg_epilogue<BT>(A, [&](int row, int col, c128 k) {
            rk4_update((size_t)(bm * BT + row) * Np + bn * BT + col, k);
          });
          QD_TMARK(3);
        }
      __syncthreads();
      }
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

namespace qd {
// The CHUNK instantiations of lindblad_rk4_kernel (nc > MAX_NC), one workgroup per matrix (glf_chunk.hip).
int glf_launch_chunk(const LindbladParams& p, int B, hipStream_t st);
// Zero-padded copy [B][N][N] -> [B][Np][Np] and back (glf.hip).
int glf_pad(const c128* src, c128* dst, int B, int N, int Np, hipStream_t st);
int glf_unpad(const c128* src, c128* dst, int B, int N, int Np, hipStream_t st);
// Few matrices as one persistent launch, a workgroup per 16 x 16 output tile (glf_single.hip).
int glf_single_max_batch(int Np, int nc, int herm = 0);
int glf_single_run(const c128* P, const c128* Q, const c128* Lop, const c128* Rop, int nc, const c128* eT, int ne,
                   c128* rho, int B, int N, int Np, double dt, int nsteps, c128* obs, c128* snap, int save_every,
                   const int** status_out, hipStream_t st, int herm = 0);
}  // namespace qd
