// glf_eig_jump_kernel.hpp — lindblad_eig_jump_kernel: the Lindblad batch at Np = 128 with ONE collapse operator,
// propagated in the eigenbasis of that operator, C = W diag(mu) W^-1 (host plan: pyqed_amd/oqs.py, EigJumpPlan).  With
// rho~ = W^-1 rho W^-+ and A~ = W^-1 A W, A = -iH - 1/2 C^+ C, the equation of motion is
//     d rho~/dt = X + X^+ + M o rho~ ,   X = A~ rho~ ,   M_ij = mu_i conj(mu_j)
// so the dissipator is elementwise and the A term is ONE full GEMM: 6,144 3-product MFMAs per stage for the 9,600 of
// lindblad_eig_kernel, which diagonalises A and pays two GEMMs for the dissipator.  One persistent workgroup per
// matrix.
// k = X + X^+ is formed inside the GEMM, on the 36 16 x 16 tiles on and above the diagonal only (cg_dma_ksteps_xh,
// cgemm_dma128.hpp): a tile (R, C) above the diagonal takes sum_k A~[R,k] r[k,C] and, from the same K-tile with the
// fragment roles swapped, conj(sum_k r[k,R] A~[C,k]) = conj(X_CR); a diagonal tile takes the first sum alone and adds
// its own dagger inside the owning wave, through a wave-private 4 KB LDS patch.  28 * 2 + 8 = 64 tile-GEMMs, the count
// of the full product, with no X^+ image in LDS, no publishing barrier, and at most 5 live tiles per wave (120
// accumulator VGPRs).  Off-diagonal tiles cost two units and diagonal ones one; jump_ctile places them so that each
// SIMD's two waves (w, w + 4) hold two diagonal and seven off-diagonal tiles, 16 units.
// The tail (jump_tail) is lindblad_eig_kernel's eig_tail with one load round: rn_ij = a base_ij + hc k_ij on the upper
// elements, the mirror written as the conjugate and the diagonal's imaginary part dropped: every stage result is
// exactly Hermitian with an exactly real diagonal.  The elementwise term takes no load of r: the tail has v = rn in
// registers on exactly the tiles whose accumulators the wave owns and leaves T = M o v in them, in the 3-product form,
// for the next stage's GEMM to accumulate onto (half of it on a diagonal tile, whose dagger doubles it).  So each wave
// runs the whole call on a code path of its own (jump_run): its accumulators live from pass to pass and are the
// registers of its own tiles alone.  Rows 0 .. 31 of rn also go from the tail's registers into L.b[0] and
// L.b[1], the next pass's A operand sends its K-tile 0 into L.a[0] by DMA under this pass's last K-tile, and the next
// pass starts as CG_START_TWO: no stage starts cold, and the barrier between two passes drains nothing.
// The same engine runs the second half of the two basis changes, rho~ = W^-1 rho W^-+ at the head and
// rho = W rho~ W^+ at the tail: Y = M r on all 64 tiles (first sums alone, stored), then k = X + X^+ for X = Y (M^+ / 2)
// with a = 0, no T, hc = 1: (Z + Z^+) / 2 for Z = M r M^+, Hermitian by construction; the multiplications by zero are
// exact on finite data.  128 tile-GEMMs per change, 4 % of a 20-step call.
// Only glf_eig_jump.hip includes this header: the neighbours' register allocation has changed with what shares their
// translation unit.  0 spilled VGPRs, 0 B scratch in the normal build (tools/isa_diff.py); the
// QD_PHASE_TIMING build, whose marks sit between a pass's GEMM and its tail, spills.
#pragma once
#include "glf_herm_k.hpp"   // wave_uniform, wg_observables_batch

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

// This kernel's tile table: wave w keeps the row tiles {w >> 1, 7 - (w >> 1)} of the Hermitian tile layout
// (cgemm_dma128.hpp) and takes the column tiles jump_ctile(w, .).  A tile above the diagonal is two units of MFMA
// work (both sums) and a diagonal tile one; cg_herm_ctile, which balances tile COUNTS, would give the four SIMDs 16,
// 16, 15 and 17 units.  The batch and A-basis kernels keep cg_herm_ctile.
constexpr int jump_ctile(int w, int nj) {
  constexpr unsigned short cols[8] = {0x3210, 0x7654, 0x4321, 0x7650, 0x7432, 0x6510, 0x7632, 0x5410};
  return (cols[w] >> (nj * 4)) & 15;
}
constexpr int jump_rtile(int w, int mi) { return mi == 0 ? (w >> 1) : 7 - (w >> 1); }
enum JumpTiles { JUMP_UPPER, JUMP_ABOVE, JUMP_DIAG };   // R <= C, R < C, R == C
constexpr unsigned jump_mask(int w, JumpTiles kind) {
  unsigned m = 0;
  for (int mi = 0; mi < 2; ++mi)
    for (int nj = 0; nj < 4; ++nj) {
      const int R = jump_rtile(w, mi), C = jump_ctile(w, nj);
      if (kind == JUMP_UPPER ? R <= C : kind == JUMP_ABOVE ? R < C : R == C) m |= 1u << (mi * 4 + nj);
    }
  return m;
}
constexpr bool jump_tiles_partition() {   // every one of the 64 tiles has exactly one owner
  int n[8][8] = {};
  for (int w = 0; w < 8; ++w)
    for (int mi = 0; mi < 2; ++mi)
      for (int nj = 0; nj < 4; ++nj) ++n[jump_rtile(w, mi)][jump_ctile(w, nj)];
  for (int R = 0; R < 8; ++R)
    for (int C = 0; C < 8; ++C)
      if (n[R][C] != 1) return false;
  return true;
}
constexpr bool jump_tiles_balanced() {   // each SIMD's waves (w, w + 4): two diagonal and seven off-diagonal tiles
  for (int s = 0; s < 4; ++s) {
    int d = 0, o = 0;
    for (int w = s; w < 8; w += 4)
      for (int t = 0; t < 8; ++t) {
        d += (jump_mask(w, JUMP_DIAG) >> t) & 1u;
        o += (jump_mask(w, JUMP_ABOVE) >> t) & 1u;
      }
    if (d != 2 || o != 7) return false;
  }
  return true;
}
static_assert(jump_tiles_partition(), "jump_ctile: a partition of the 64 tiles");
static_assert(jump_tiles_balanced(), "jump_ctile: 2 diagonal + 7 off-diagonal tiles per SIMD");

// Rows 0 .. 31 of rn are the B halves of K-tiles 0 and 1 of the next pass's GEMM and go into L.b[0] (rows 0 .. 15) and
// L.b[1] (rows 16 .. 31) in the engine's B-tile image, by the roles of eig_tail (glf_eig_kernel.hpp) restated for this
// table: an upper element of a tile in row tile 0 or 1, and the mirror of one in column tile 0 or 1.
constexpr bool jump_rn_lds_upper(int R, int C, int ra, int lc) { return R < 2 && (R < C || ra <= lc); }
constexpr bool jump_rn_lds_mirror(int R, int C, int ra, int lc) { return C < 2 && (R < C || ra < lc); }
constexpr bool jump_rn_lds_one_to_one() {
  unsigned char n[2][CG_KT * JUMP_NP] = {};
  for (int w = 0; w < 8; ++w)
    for (int mi = 0; mi < 2; ++mi)
      for (int nj = 0; nj < 4; ++nj) {
        const int R = jump_rtile(w, mi), C = jump_ctile(w, nj);
        if (R > C) continue;
        if ((R < 2 || C < 2) && !(w < 4 && mi == 0)) return false;   // the writers are mi == 0 of waves 0 .. 3 (jump_tail)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 4; ++e) {
            const int ra = (lane >> 4) + 4 * e, lc = lane & 15;
            if (jump_rn_lds_upper(R, C, ra, lc)) ++n[R][cg_dma_b_slot(ra, 16 * C + lc)];    // rn[16 R + ra][16 C + lc]
            if (jump_rn_lds_mirror(R, C, ra, lc)) ++n[C][cg_dma_b_slot(lc, 16 * R + ra)];   // rn[16 C + lc][16 R + ra]
          }
      }
  for (int t = 0; t < 2; ++t)
    for (int s = 0; s < CG_KT * JUMP_NP; ++s)
      if (n[t][s] != 1) return false;
  return true;
}
static_assert(jump_rn_lds_one_to_one(), "rows 0 .. 31 of rn onto L.b[0], L.b[1]: one writer per slot");

// The diagonal tiles' dagger: a wave-private patch of 256 slots in L.a[1], free behind the GEMM's closing barrier.
// Element (ra, cc) sits at ra * 16 + (cc ^ ra) (HermKL's pattern): the writer's 64 lanes cover four whole 256-byte rows,
// and the 16 lanes of one read group (one column, rows 256 B apart) hit 16 distinct 16-byte slots.
constexpr int jump_patch_slot(int ra, int cc) { return ra * 16 + (cc ^ ra); }
static_assert(8 * 256 <= JUMP_NP * CG_SA, "the eight patches fit L.a[1]");

// One pass's GEMM for wave W, depth Np, every K-tile staged from inside the k-steps of the tile before
// (CgDmaStageHook) and every tile-end written as s_waitcnt vmcnt(0) + barrier, as in cg_dma_herm_d_gemm_h.
//   FULL = false: k = A B + (A B)^+ on the wave's tiles on and above the diagonal (cg_dma_ksteps_xh);
//   FULL = true:  Y = A B on all eight tiles (cg_dma_ksteps).
// start: CG_START_COLD stages its own tile 0 (DMA round trip and barrier).  CG_START_TWO finds tile 0 complete in
// buffer 0 (its A half by the lookahead of the pass before, its B half from that pass's tail) and rows 16 .. 31 of B
// in L.b[1]; tile 0's hook then stages the A half of tile 1 alone, and B is first read from memory for tile 2, issued
// under tile 1, behind tile 0's closing wait and barrier, which complete and publish every wave's stores of it.
// The last tile (T even: it reads buffer 1) stages the A half of tile 0 of nA -> L.a[0], last read one barrier
// earlier; nA == nullptr: nothing.  Called from a per-wave code path by all threads; ends with a workgroup barrier;
// the accumulators are NOT finalised.  A Y pass zeroes them; a k pass accumulates onto what it finds.
template <int W, bool FULL>
__device__ __forceinline__ void jump_gemm(const c128* A, const c128* B, const c128* nA, CgStart start, int Np,
                                          CgLds<128>& L, CgAcc3& acc) {
  constexpr int NQ = CG_KT / 4;
  constexpr unsigned FS = jump_mask(W, JUMP_UPPER), SW = jump_mask(W, JUMP_ABOVE), DG = jump_mask(W, JUMP_DIAG);
  const int r0[2] = {16 * jump_rtile(W, 0), 16 * jump_rtile(W, 1)};
  const int c0[4] = {16 * jump_ctile(W, 0), 16 * jump_ctile(W, 1), 16 * jump_ctile(W, 2), 16 * jump_ctile(W, 3)};
  const int T = Np / CG_KT;
  const CgDmaStage st(nullptr, T, Np, Np);
  if constexpr (FULL) cg_dma_zero(acc);   // a k pass starts from what the pass before left: T (jump_tail) or zero
  if (start == CG_START_COLD) {
    st.issue_at(A, B, 0, L, 0);
    __syncthreads();
  }
  for (int t = 0; t < T; ++t) {
    const bool more = t + 1 < T;
    const char* ga = more ? cg_uniform(A + (t + 1) * CG_KT) : nA ? cg_uniform(nA) : nullptr;
    const char* gb = more ? cg_uniform(B + (size_t)(t + 1) * CG_KT * Np) : nullptr;
    if (start == CG_START_TWO && t == 0) gb = nullptr;   // L.b[1] is the tail's: the A half of tile 1 alone
    const CgDmaStageHook hook{st, L, ga, gb, more ? (t + 1) & 1 : 0};
    cg_sched_fence();
    if constexpr (FULL) cg_dma_ksteps<0u, 0, NQ>(L, t & 1, acc, r0, c0, hook);
    else cg_dma_ksteps_xh<FS, SW, DG, 0, NQ>(L, t & 1, acc, r0, c0, hook);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

// m on the elements of wave W's tiles on and above the diagonal, in MFMA layout (eig_tile_loads on this table).
template <int W>
__device__ __forceinline__ void jump_tile_loads(const c128* m, int lane, c128 (&q)[8][4]) {
  const unsigned vu = (unsigned)((lane >> 4) * JUMP_NP + (lane & 15)) * (unsigned)sizeof(c128);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = jump_rtile(W, mi), C = jump_ctile(W, nj);
      if (R > C) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned su = (unsigned)((16 * R + 4 * e) * JUMP_NP) * (unsigned)sizeof(c128);   // uniform
        q[mi * 4 + nj][e] = *reinterpret_cast<const c128*>(reinterpret_cast<const char*>(m + 16 * C) + (vu + su));
      }
    }
}

// Behind the GEMM: wave W finalises its live tiles, adds each diagonal tile's dagger through its patch under the loads
// of base, forms rn_ij = a base_ij + hc k_ij on the upper elements and writes rn_ji as the conjugate.  Diagonal tiles
// store ra <= lc only, and rn_ii is real.  Each upper element is read (base) and written by one thread, loads first, so
// rn may be base.
// The elementwise term never takes a load of r: v = rn is in registers on exactly the tiles whose accumulators the wave
// owns, so the tail leaves T = gn M o v there for the NEXT pass, M_ij = mu_i conj(mu_j), in the 3-product form
// (P1, P2, P3) = (T_re, 0, T_re + T_im), which cg_dma_finalise turns into (T_re, T_im) plus the GEMM's sums.  A
// diagonal tile gets T / 2: its dagger adds conj(T_ji) / 2 from the lane that holds the mirror, whose v is the
// conjugate bit for bit (k_ji = x_ji + conj(x_ij), and base is exactly Hermitian), so k carries (T_ij + conj(T_ji)) / 2,
// which is T_ij up to the rounding of mu_i conj(mu_j).  gn = 1 ahead of a stage and 0 ahead of a basis change, where
// the next k pass must find zero (exact on finite data).
template <int W>
__device__ __forceinline__ void jump_tail(CgAcc3& A, const c128* base, c128* rn, const c128* muS, CgLds<128>& L,
                                          int lane, double a, double hc, double gn) {
  constexpr unsigned LIVE = jump_mask(W, JUMP_UPPER);
  const int lr = lane >> 4, lc = lane & 15;
  const unsigned vu = (unsigned)(lr * JUMP_NP + lc) * (unsigned)sizeof(c128);
  const unsigned vm = (unsigned)(lc * JUMP_NP + lr) * (unsigned)sizeof(c128);
  c128 q[8][4];
  cg_dma_finalise_live<LIVE>(A);
  cg_sched_fence();   // the loads of base go into the registers the third accumulator set has left
  jump_tile_loads<W>(base, lane, q);
  c128* P = &L.a[1][256 * W];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = jump_rtile(W, mi), C = jump_ctile(W, nj);
      if (R != C) continue;
      // k_RR = X_RR + X_RR^+: LDS operations of one wave run in order, no barrier
#pragma unroll
      for (int e = 0; e < 4; ++e) P[jump_patch_slot(lr + 4 * e, lc)] = cmk(A.re[mi][nj][e], A.im[mi][nj][e]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const c128 m = P[jump_patch_slot(lc, lr + 4 * e)];
        A.re[mi][nj][e] += m.re;
        A.im[mi][nj][e] -= m.im;
      }
    }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = jump_rtile(W, mi), C = jump_ctile(W, nj);
      if (R > C) continue;
      const c128 mj = muS[16 * C + lc];
      const double gs = R == C ? 0.5 * gn : gn;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ra = lr + 4 * e;
        const c128 k = cmk(A.re[mi][nj][e], A.im[mi][nj][e]);
        c128 v = cadd(cscale(q[mi * 4 + nj][e], a), cscale(k, hc));
        if (R == C && ra == lc) v.im = 0.0;
        const unsigned su = (unsigned)((16 * R + 4 * e) * JUMP_NP) * (unsigned)sizeof(c128);   // uniform, as sm
        const unsigned sm = (unsigned)(16 * C * JUMP_NP) * (unsigned)sizeof(c128);
        char* u = reinterpret_cast<char*>(rn + 16 * C) + (vu + su);
        char* t = reinterpret_cast<char*>(rn + 16 * R + 4 * e) + (vm + sm);
        if (R < C || ra <= lc) *reinterpret_cast<c128*>(u) = v;
        if (R < C || ra < lc) *reinterpret_cast<c128*>(t) = cconj(v);
        if constexpr (W < 4) {   // row tiles 0 and 1 (mi == 0 of waves 0 .. 3); the buffers are named by literals
          if (R < 2 && jump_rn_lds_upper(R, C, ra, lc)) L.b[R & 1][cg_dma_b_slot(ra, 16 * C + lc)] = v;
          if (R < 2 && C < 2 && jump_rn_lds_mirror(R, C, ra, lc)) L.b[C & 1][cg_dma_b_slot(lc, 16 * R + ra)] = cconj(v);
        }
        const c128 mi_ = muS[16 * R + ra];
        const double gre = gs * (mi_.re * mj.re + mi_.im * mj.im), gim = gs * (mi_.im * mj.re - mi_.re * mj.im);
        const double tre = gre * v.re - gim * v.im, tim = gre * v.im + gim * v.re;
        A.re[mi][nj][e] = tre;
        A.im[mi][nj][e] = 0.0;
        A.p3[mi * 4 + nj][e] = tre + tim;
      }
    }
}

// Y = M r of a basis change: wave W stores all eight of its tiles.
template <int W>
__device__ __forceinline__ void jump_store_y(const CgAcc<128>& A, c128* Y, int lane) {
  const unsigned vu = (unsigned)((lane >> 4) * JUMP_NP + (lane & 15)) * (unsigned)sizeof(c128);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int R = jump_rtile(W, mi), C = jump_ctile(W, nj);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned su = (unsigned)((16 * R + 4 * e) * JUMP_NP) * (unsigned)sizeof(c128);   // uniform
        *reinterpret_cast<c128*>(reinterpret_cast<char*>(Y + 16 * C) + (vu + su)) = cmk(A.re[mi][nj][e], A.im[mi][nj][e]);
      }
    }
}

// What a wave's code path needs of the call, by value: scalars of its own, nothing read through the parameter block.
struct JumpCall {
  const c128 *At, *W, *Wi, *Wdh, *Widh, *eT;
  c128 *rho, *ws, *rbuf1, *obs;
  int ne, nit;
  double dt;
};

#ifdef QD_PHASE_TIMING
#define JUMP_TIMING_PARAM , const LindbladJumpParams& p, unsigned long long (&tacc)[6], unsigned long long& tlast, unsigned long long& txf
#define JUMP_TIMING_ARG , p, tacc, tlast, txf
#else
#define JUMP_TIMING_PARAM
#define JUMP_TIMING_ARG
#endif

// The whole call for wave W (the pass table and the hand-overs are listed in the kernel).
template <int W>
__device__ __forceinline__ void jump_run(const JumpCall o, int Np, CgLds<128>& L, c128* sred, const c128* muS JUMP_TIMING_PARAM) {
  const int nit = o.nit;
  CgAcc3 A;
  for (int it = 0; it < nit; ++it) {
    const bool xf = it < 2 || it >= nit - 2, ypass = it == 0 || it == nit - 2;
    const int stage = (it - 2) & 3;
    const c128* r = (xf || stage == 0) ? o.rho : ((stage - 1) & 1) ? o.rbuf1 : o.ws;
    c128* rn = (xf || stage == 3) ? o.rho : (stage & 1) ? o.rbuf1 : o.ws;
    const c128* oa = it == 0 ? o.Wi : it == nit - 2 ? o.W : xf ? o.ws : o.At;
    const c128* ob = it == 1 ? o.Widh : it == nit - 1 ? o.Wdh : r;
    // the next pass's A operand where this pass hands over: W ahead of the change back, A~ ahead of a stage
    const c128* na = (ypass || it == nit - 1) ? nullptr : it + 1 == nit - 2 ? o.W : o.At;
    const CgStart start = (it == 0 || it == 1 || it == nit - 1) ? CG_START_COLD : CG_START_TWO;
    double dts = o.dt;
    asm volatile("" : "+s"(dts));   // per pass: no coefficient register held across the K loop
    const double hc = wave_uniform(xf ? 1.0 : glf_horner_coef(dts, stage)), ab = wave_uniform(xf ? 0.0 : 1.0);
    const double gn = wave_uniform(it >= 1 && it + 1 < nit - 2 ? 1.0 : 0.0);   // the next pass is a stage
    const bool watch = o.ne > 0 && (it == 1 || (!xf && stage == 3));   // observables on rho~: t0 and the end of every step
#ifdef QD_PHASE_TIMING
    unsigned long long tkeep[6] = {tacc[0], tacc[1], tacc[2], tacc[3], tacc[4], tacc[5]};
#endif
    if (ypass) {
      jump_gemm<W, true>(oa, ob, na, start, Np, L, A);
      cg_dma_finalise(A);
      QD_TMARK(2);
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));   // the tail's index math is made behind the K loop, not held across it
      jump_store_y<W>(A, o.ws, tid & 63);
      cg_dma_zero(A);   // the k pass behind a Y pass carries no T
    } else {
      jump_gemm<W, false>(oa, ob, na, start, Np, L, A);
      QD_TMARK(2);
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));
      jump_tail<W>(A, o.rho, rn, muS, L, tid & 63, ab, hc, gn);
    }
    if (ypass || watch || it == nit - 1) {
      __syncthreads();   // Y, or rho for the observables, read from memory next: the stores drained and published
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's ds_writes of rows 0 .. 31 and its patch reads; NOT vmcnt
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    QD_TMARK(3);
#ifdef QD_PHASE_TIMING
    if (xf)
      for (int q = 0; q < 6; ++q) {
        txf += tacc[q] - tkeep[q];
        tacc[q] = tkeep[q];
      }
#endif
    if (watch) {   // touches sred alone: the staged tiles stay
      wg_observables_batch(o.rho, o.eT, o.ne, JUMP_NP * (size_t)JUMP_NP, o.obs + (size_t)((it - 1) / 4) * o.ne, sred);
      QD_TMARK(4);
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

  QD_TIMING_DECL
#ifdef QD_PHASE_TIMING
  unsigned long long txf = 0;   // the basis changes' ticks, charged to slot 0 instead of the stages' slots
#endif

  // Each wave runs the whole call on a code path of its own (the switch at the bottom): its accumulators, which carry T
  // from a pass's tail into the next pass's GEMM, are then the registers of its own tiles alone; with the switch inside
  // the pass loop all eight tiles of every wave's table would live across it.  The workgroup barriers pair up across the
  // paths: every path runs the same passes.
  // Pass `it` of the call, each one GEMM and one tail:
  //   0              Y = W^-1 rho -> ws                  4 nsteps + 2   Y = W rho~ -> ws
  //   1              rho~ = sym(Y W^-+) -> rho           4 nsteps + 3   rho = sym(Y W^+) -> rho
  //   2 .. 4 nsteps + 1   the Horner stages (glf_horner_coef), stage = (it - 2) & 3: rho~ -> s1 -> s2 -> s3 -> rho~ over
  //                  ws and rbuf1 as in the batch kernel, so a stage never writes the buffer its GEMM reads
  // sym(Z) = (Z + Z^+) / 2 is a stage with a = 0, hc = 1, no T, Y as the A operand and the halved dagger as the B operand.
  // The elementwise term M o r of a stage is the T its predecessor's tail left in the accumulators (jump_tail): pass 1
  // leaves it for the first stage, the last stage leaves zero, and a Y pass zeroes the accumulators behind its stores.
  // From pass to pass (every pass but a Y pass and the call's last hands over; invariant (6) of lindblad_eig_kernel's
  // phase loop, glf_eig_kernel.hpp, with one GEMM per pass):
  //   B halves of the next K-tiles 0 and 1: rows 0 .. 31 of rn, from jump_tail's registers into L.b[0] and L.b[1] (and
  //     to memory as every other row).  WAR: L.b[0] was last read at tile T - 2 and L.b[1] at T - 1, both ahead of the
  //     GEMM's closing barrier.  RAW: each writer's s_waitcnt lgkmcnt(0), then the raw s_barrier that ends the pass.
  //     That barrier does not wait for vmcnt: the rn stores drain under the next tile 0, whose closing
  //     s_waitcnt vmcnt(0) + barrier complete and publish them ahead of the first DMA read of rn, tile 2.
  //   A half of the next K-tile 0: DMA into L.a[0] under this GEMM's last K-tile (L.a[0] last read at T - 2), retired
  //     by that tile's wait and barrier.  A half of K-tile 1: DMA into L.a[1] under the next tile 0, issued behind the
  //     pass-end barrier, so behind every wave's patch reads (each wave waits lgkmcnt(0) ahead of that barrier).
  //   The diagonal patches live in L.a[1], last read as a staging buffer at tile T - 1, ahead of the closing barrier.
  //   A Y pass ends in a full __syncthreads(): Y is read by the next pass's cold prologue.  So do a pass whose result
  //   the observables read from memory and the call's last pass.  The observables touch sred alone, so the staged
  //   tiles stay and the pass behind them starts as behind any other.
  const int nit = 4 * p.nsteps + 4;
  const JumpCall o{p.At, p.W, p.Wi, p.Wdh, p.Widh, p.eT, rho, ws, rbuf1, obs, p.ne, nit, p.dt};
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#define QD_JW(w) \
  case w: jump_run<w>(o, Np, L, sred, muS JUMP_TIMING_ARG); break;
  switch (wave) { QD_JW(0) QD_JW(1) QD_JW(2) QD_JW(3) QD_JW(4) QD_JW(5) QD_JW(6) default: QD_JW(7) }
#undef QD_JW
#ifdef QD_PHASE_TIMING
  tacc[0] += txf;
#endif
  QD_TIMING_FLUSH
}

}  // namespace
}  // namespace qd
