// deom_band_kernel.hpp — one hierarchy as one persistent launch over tier bands (qd_deom_rk4_banded, deom.hip): the
// band kernel with its hand-off helpers, the kernel that prepares a call and the stream-ordered single-workgroup
// fallback.
#pragma once

#include "deom_kernels.hpp"

namespace qd {
namespace {

// Stream-ordered fallback of qd_deom_rk4_banded called without a status word: queued behind the banded launch, it
// returns at once unless that launch reported a hand-off timeout in *stat; then ONE workgroup restores the saved
// initial ADOs and runs the whole propagation on deom_stage_element (the stage launches' arithmetic), stage by stage
// with a device-scope fence and a workgroup barrier between stages (slow -- one CU -- but no host wait: the banded
// entry point stays asynchronous).  x0 / x1: stage buffers, acc: the classic-form accumulator (driven runs).
// The band tables' local neighbour rows (lminus / lplus: a band's own rows first, then its halo rows) are mapped back
// to global ADO rows into gminus / gplus first.
__global__ __launch_bounds__(1024) void deom_banded_fallback_kernel(DeomParams p, const int* stat, const c128* saved,
                                                                     c128* ados, c128* x0, c128* x1,
                                                                     const c128* fsv, const c128* fcv,
                                                                     const int* lminus, const int* lplus,
                                                                     const int* band_lo, const int* halo_off,
                                                                     const int* halo_idx, int nbands, int* gminus,
                                                                     int* gplus) {
  if (__hip_atomic_load(stat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  __shared__ c128 sH[DEOM_MAX_NS * DEOM_MAX_NS];
  __shared__ c128 sQ[DEOM_MAX_NMOD * DEOM_MAX_NS * DEOM_MAX_NS];
  const size_t tot = (size_t)p.nmax * p.ns * p.ns;
  for (size_t e = threadIdx.x; e < tot; e += blockDim.x) ados[e] = saved[e];
  for (int e = threadIdx.x; e < p.nmax * p.K; e += blockDim.x) {
    const int n = e / p.K;
    int lo = 0, hi = nbands;   // band b with band_lo[b] <= n < band_lo[b + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) / 2;
      if (band_lo[mid] <= n) lo = mid;
      else hi = mid;
    }
    const int own = band_lo[lo + 1] - band_lo[lo];
    auto glob = [&](int r) { return r < 0 ? -1 : r < own ? band_lo[lo] + r : halo_idx[halo_off[lo] + r - own]; };
    gminus[e] = glob(lminus[e]);
    gplus[e] = glob(lplus[e]);
  }
  __threadfence();
  __syncthreads();
  p.minus = gminus;
  p.plus = gplus;
  p.rho = ados;
  p.rho_out = ados;
  for (int s = 0; s < p.nsteps; ++s) {
    p.step = s;
    for (int stage = 0; stage < 4; ++stage) {
      p.stage = stage;
      p.xin = stage == 0 ? (const c128*)ados : ((stage - 1) & 1 ? x1 : x0);
      p.xout = stage & 1 ? x1 : x0;
      const int ti = s * 3 + (stage + 1) / 2;   // pulse values at t, t + dt/2, t + dt
      p.fs = fsv ? fsv[ti] : cmk(0, 0);
      p.fc = fcv ? fcv[ti] : cmk(0, 0);
      deom_stage_ops(p, sH, sQ);
      __syncthreads();
      for (size_t e = threadIdx.x; e < tot; e += blockDim.x) deom_stage_element(p, e, sH, sQ);
      __threadfence();   // agent-scope release / acquire: the next stage's loads see these stores, not stale L1 lines
      __syncthreads();
    }
  }
}

// Per-call setup of the banded launch in one kernel (instead of three memsets and a copy): both hand-off buffers to
// parity 1 in every double (bytes 0x01), the status words to 0, row 0 of the snapshots from the initial ADO 0.
__global__ void deom_band_prep_kernel(unsigned long long* buf, long nwords, int* stat, int* stat2, const c128* ados,
                                      c128* snap, int ns2, c128* saved, long tot) {
  const long i0 = blockIdx.x * (long)blockDim.x + threadIdx.x, st = (long)gridDim.x * blockDim.x;
  for (long i = i0; i < nwords; i += st) buf[i] = 0x0101010101010101ull;
  if (saved)   // the initial ADOs for the stream-ordered fallback
    for (long i = i0; i < tot; i += st) saved[i] = ados[i];
  if (i0 == 0) {
    *stat = 0;
    if (stat2) *stat2 = 0;
  }
  if (snap && i0 < ns2) snap[i0] = ados[i0];
}

}  // namespace
}  // namespace qd

using namespace qd;   // as deom.hip: the band kernel keeps its file-local symbols

namespace {

// ---------------------------------------------------------------------------------------------------------------
// One hierarchy as ONE persistent launch over a handful of tier bands (qd_deom_rk4_banded).
//
// The unbanded path runs one launch per RK4 stage: at the bench hierarchy (6188 ADOs, 396 KB of state) a stage is
// two dependent memory round trips plus the ~1.5 us kernel boundary, 4.8 us in all.  Here workgroup w owns the
// contiguous ADO band [band_lo[w], band_lo[w+1]) of the partition deom_shard.make_plans builds (the keys are tier
// ordered, so a band's outside neighbours sit in tiers l -/+ 1 of it).  Its LDS holds the stage input of its owned
// rows followed by its halo rows (local rows: lminus / lplus), its registers hold rho and the RK4 accumulator of
// its owned elements for the whole run.  Per stage a workgroup
//   1. loads its halo rows of the previous stage's output with sc1 (L1-bypassing) 16-B loads into LDS, re-loading
//      every element whose doubles do not yet carry that stage's parity in their lowest mantissa bit (the data is
//      the flag, cdna_hip_programming.md Guideline 16 R2; s_sleep between sweeps, bounded spin);
//   2. evaluates the stencil of the group kernel (same arithmetic, same operand order) from LDS and runs the RK4
//      epilogue in registers;
//   3. writes the next stage input to its LDS rows (exact) and, write-through (sc1 stores) with its parity in every
//      double's lowest bit, to buf[g & 1]; no drain, no barrier, no epoch word.
// A halo value is thus off by at most one unit in its last place; it reaches the result only through dt x stencil
// (never a band's own state, which stays exact in registers and LDS; the last stage stores untagged): within 1e-13 of
// the stage launches, bit-identical with one band.  Against the epoch-word form (drain, barrier, flag; one wave
// polls, barrier, loads) 100-104k -> 115k steps/s at 6188 ADOs, 73.6k -> 85.2k at 18,564
// (profiles/r05/deom/band_r2_handoff_ab.txt).  Reuse of buf[g & 1] is safe: a band overwrites its rows at stage g
// after it loaded stage g - 1's rows of every source, which each stored only after loading its halo of stage g - 2
// (its halo loads complete before its stencil's barrier), and the neighbour relation is symmetric (sources ==
// consumers).  Both buffers are preset to parity 1 (stages 0 and 1, their first writers, carry 0).
// Stage 0 of step 0 reads the caller's ados (written before the launch); the last stage 3 writes the final rho
// straight into ados.  A spin that exceeds its bound (bands not co-resident)
// sets *status = 1 and every band leaves its loop (results then invalid; the host reports it).
constexpr unsigned BAND_SPIN_LIMIT = 1u << 21;  // sweeps (one round trip each): ~1 s

struct BandParams {
  const c128* ados;      // [nmax][ns2] rho at t = 0 (read at stage 0 of step 0 only)
  c128* buf;             // [2][nmax][ns2] stage outputs (hand-off buffers)
  int* status;           // [1] 0 = ok, 1 = a hand-off timed out
  const int* band_lo;    // [nbands + 1]
  const int* halo_off;   // [nbands + 1]
  const int* halo_idx;   // global ADO rows of each band's halo
  const int* src_off;    // [nbands + 1]
  const int* src;        // bands owning each band's halo rows
  const int* lminus;     // [nmax][K] local rows (owned first, then halo), -1 absent
  const int* lplus;
  const c128* coef;      // [nmax][K][3] cL, cR, cP
  const c128* damp;      // [nmax]
  const int* mode;       // [K]
  const c128* H;
  const c128* Hdip;      // or null
  const c128* Q;
  const c128* Qdip;      // or null
  const c128* fsv;       // [nsteps][3] pulse values (t, t + dt/2, t + dt) or null
  const c128* fcv;
  c128* snap;            // [nsteps + 1][ns2] rho_0 after each step, or null
  unsigned long long* tim;   // QD_PHASE_TIMING builds: [nbands][4] wall-clock ticks per phase
  int nmax, K, ns, nmod, nsteps, max_loc;
  double dt;
};

constexpr int BAND_HM = 8;   // halo elements per thread held as precomputed offsets (one batched load per stage)
#ifndef DEOM_BAND_EARLY
#define DEOM_BAND_EARLY 1   // undriven runs: the next stage's damping + coherent part computed before the poll (A/B: 0)
#endif
__device__ __forceinline__ c128 ld_sc1(const c128* q) {
  return cmk(__hip_atomic_load(&q->re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
             __hip_atomic_load(&q->im, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_sc1(c128* q, c128 v) {
  __hip_atomic_store(&q->re, v.re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&q->im, v.im, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// R2 hand-off granules (cdna_hip_programming.md Guideline 16: the data is the flag): the parity of the producing
// stage in the lowest mantissa bit of both halves of a handed-off element (at most one unit in the last place; it
// reaches the result only through dt times the stencil of a neighbour, never a band's own state)
__device__ __forceinline__ c128 band_tag(c128 v, unsigned t) {
  const unsigned long long x = __builtin_bit_cast(unsigned long long, v.re);
  const unsigned long long y = __builtin_bit_cast(unsigned long long, v.im);
  return cmk(__builtin_bit_cast(double, (x & ~1ull) | t), __builtin_bit_cast(double, (y & ~1ull) | t));
}
__device__ __forceinline__ bool band_has(c128 v, unsigned t) {
  const unsigned x = (unsigned)__builtin_bit_cast(unsigned long long, v.re);
  const unsigned y = (unsigned)__builtin_bit_cast(unsigned long long, v.im);
  return (((x ^ t) | (y ^ t)) & 1u) == 0;
}
// every 256 sweeps: has another band reported a timeout?
__device__ __forceinline__ bool band_abort_seen(const int* status, unsigned spins) {
  return (spins & 255) == 0 && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// FAST (ns = 2, K == KMAX, one bath mode): the mode loop, the K bound and H / Q fold to constants and registers.
template <int G, int KMAX, bool NS2, int TPB, bool FAST>
__global__ __launch_bounds__(TPB) void deom_band_kernel(BandParams p) {
  static_assert(!FAST || NS2, "FAST is the ns = 2 specialisation");
  extern __shared__ c128 deom_lds[];
  __shared__ int sAbort[2];   // a band's timed-out sweep in stage g sets sAbort[g & 1]
  const int ns = NS2 ? 2 : p.ns, ns2 = ns * ns, K = FAST ? KMAX : p.K;
  c128* sH = deom_lds;
  c128* sQ = deom_lds + ns2;
  c128* sX = deom_lds + (size_t)(1 + p.nmod) * ns2;   // [n_own + n_halo][ns2], then one zero row (absent neighbours)
  const int w = blockIdx.x;
  const int lo = p.band_lo[w], no = p.band_lo[w + 1] - lo;
  const int hoff = p.halo_off[w], nh = p.halo_off[w + 1] - hoff;
  const int soff = p.src_off[w], nsrc = p.src_off[w + 1] - soff;
  const int tid = threadIdx.x;
  const int a = tid / G, e = tid % G;
  const bool live = a < no;                  // uniform within a group
  const bool valid = live && e < ns2;
  const int ee = e < ns2 ? e : 0;            // padding lanes shadow element 0
  const int al = live ? a : 0;
  const int n = lo + al;
  const int base = (tid & 63) & ~(G - 1);
  auto shfl = [&](c128 v, int s) { return cmk(__shfl(v.re, base + s, 64), __shfl(v.im, base + s, 64)); };
  auto bc = [&](c128 v, int s) -> c128 {
    if constexpr (G == 4) {
      switch (s) {
        case 0: return dpp_qc<0x00>(v);
        case 1: return dpp_qc<0x55>(v);
        case 2: return dpp_qc<0xAA>(v);
        default: return dpp_qc<0xFF>(v);
      }
    } else {
      return shfl(v, s);
    }
  };
  auto bci = [&](int v, int s) -> int {
    if constexpr (G == 4) {
      switch (s) {
        case 0: return dpp_qi<0x00>(v);
        case 1: return dpp_qi<0x55>(v);
        case 2: return dpp_qi<0xAA>(v);
        default: return dpp_qi<0xFF>(v);
      }
    } else {
      return __shfl(v, base + s, 64);
    }
  };

  // tables of the owned ADO, once per launch: local neighbour rows broadcast into every lane of the group, the
  // 3K prefactors kept split over the group's lanes (broadcast per stage, as the group kernel)
  constexpr int NI = (KMAX + G - 1) / G;
  constexpr int NC = (3 * KMAX + G - 1) / G;
  int lm[NI], lp[NI];
  c128 lc[NC];
#pragma unroll
  for (int q = 0; q < NI; ++q) {
    const int k = e + G * q;
    lm[q] = (live && k < K) ? p.lminus[(size_t)n * K + k] : -1;
    lp[q] = (live && k < K) ? p.lplus[(size_t)n * K + k] : -1;
  }
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const int c = e + G * q;
    lc[q] = (live && c < 3 * K) ? p.coef[(size_t)n * K * 3 + c] : cmk(0, 0);
  }
  const c128 dmp = live ? p.damp[n] : cmk(0, 0);
  int im[KMAX], ip[KMAX], md[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    im[k] = bci(lm[k / G], k % G);
    ip[k] = bci(lp[k / G], k % G);
    md[k] = FAST ? 0 : (k < K ? __builtin_amdgcn_readfirstlane(p.mode[k]) : -1);
  }
  // up to 512 threads (<= 2 waves per SIMD, 256 VGPRs) the prefactors are broadcast once into every lane of the
  // group instead of once per stage
  constexpr bool FULLC = TPB <= 512;
  c128 cf[FULLC ? 3 * KMAX : 1];
  if constexpr (FULLC) {
#pragma unroll
    for (int c = 0; c < 3 * KMAX; ++c) cf[c] = bc(lc[c / G], c % G);
  }
  const bool pulsed = p.Hdip || p.Qdip;
  if (!pulsed) {
    for (int q = tid; q < ns2; q += blockDim.x) sH[q] = p.H[q];
    for (int q = tid; q < p.nmod * ns2; q += blockDim.x) sQ[q] = p.Q[q];
  }
  c128 r0 = valid ? p.ados[(size_t)n * ns2 + e] : cmk(0, 0);
  c128 acc = cmk(0, 0);
  if (valid) sX[(size_t)a * ns2 + e] = r0;
  if (tid < 2) sAbort[tid] = 0;
  // LDS element index of the own and neighbour elements this lane reads every stage; absent neighbours read the
  // zero row after the band's rows (the host sizes LDS for max_loc + 1 rows; halo writes never reach it)
  const int zrow = p.max_loc;
  for (int q = tid; q < ns2; q += blockDim.x) sX[(size_t)zrow * ns2 + q] = cmk(0, 0);
  const int oown = al * ns2 + ee;
  int om[KMAX], op[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    om[k] = ((k < K && im[k] >= 0) ? im[k] : zrow) * ns2 + ee;
    op[k] = ((k < K && ip[k] >= 0) ? ip[k] : zrow) * ns2 + ee;
  }

  const int i = ee / ns, j = ee % ns;
  auto colv = [&](c128 v, int l) -> c128 {
    if constexpr (NS2) return l == 0 ? dpp_qc<0x44>(v) : dpp_qc<0xEE>(v);
    else return shfl(v, l * ns + j);
  };
  auto rowv = [&](c128 v, int l) -> c128 {
    if constexpr (NS2) return l == 0 ? dpp_qc<0xA0>(v) : dpp_qc<0xF5>(v);
    else return shfl(v, i * ns + l);
  };
  auto for_l = [&](auto&& f) {
    if constexpr (NS2) {
      f(0);
      f(1);
    } else {
      for (int l = 0; l < ns; ++l) f(l);
    }
  };
  // H(t) / Q(t) entries this lane multiplies: H[i][l], H[l][j] (FAST: the two of each; read once for the run when
  // undriven, per stage when driven)
  c128 hil[2], hlj[2], qil[2], qlj[2];
  auto read_hq = [&]() {
    if constexpr (FAST) {
#pragma unroll
      for (int l = 0; l < 2; ++l) {
        hil[l] = sH[i * 2 + l];
        hlj[l] = sH[l * 2 + j];
        qil[l] = sQ[i * 2 + l];
        qlj[l] = sQ[l * 2 + j];
      }
    }
  };
  // damping + coherent part of the stencil, damp_n x - i[H, x], from the lane group's own elements only
  auto dlocal = [&](c128 own) -> c128 {
    c128 d = cmul(dmp, own);
    c128 comm = cmk(0, 0);
    for_l([&](int l) {
      if constexpr (FAST)
        comm = cadd(comm, csub(cmul(hil[l], colv(own, l)), cmul(rowv(own, l), hlj[l])));
      else
        comm = cadd(comm, csub(cmul(sH[i * ns + l], colv(own, l)), cmul(rowv(own, l), sH[l * ns + j])));
    });
    return cadd(d, cmulmi(comm));
  };
  // Undriven runs (H fixed): that part of stage g + 1 depends on the lane group's own rows only, so it is evaluated
  // right after stage g is published, while the source bands publish theirs (the same operations in the same
  // order: bit-identical to the stage launches)
  const bool early = DEOM_BAND_EARLY && !pulsed;
  __syncthreads();   // sH / sQ and the band's rows written above
  if (!pulsed) read_hq();
  c128 dpre = early ? dlocal(sX[oown]) : cmk(0, 0);
  static constexpr int stage_time[4] = {0, 1, 1, 2};
  const double dt = p.dt;
  const size_t slab = (size_t)p.nmax * ns2;
  const int G4 = 4 * p.nsteps;
  // this thread's halo elements q = tid + i blockDim (i < BAND_HM): byte offsets in a stage buffer, fixed for the
  // launch, so a stage issues all its halo loads back to back (one round trip); -1 = none (then element 0 is
  // loaded and dropped: branch-free).  Elements beyond BAND_HM blockDim take the generic loop below.
  const int nhe = nh * ns2;
  int hsrc[BAND_HM];
#pragma unroll
  for (int h = 0; h < BAND_HM; ++h) {
    const int q = tid + h * (int)blockDim.x;
    hsrc[h] = q < nhe ? (p.halo_idx[hoff + q / ns2] * ns2 + q % ns2) * 16 : -1;
  }
  const int slab_bytes = __builtin_amdgcn_readfirstlane((int)(slab * sizeof(c128)));
#ifdef QD_PHASE_TIMING
  unsigned long long tph[4] = {0, 0, 0, 0};
#endif

  for (int g = 0; g < G4; ++g) {
    const int step = g >> 2, stage = g & 3;
    const c128* in = g == 0 ? p.ados : p.buf + (size_t)((g - 1) & 1) * slab;
    const __amdgpu_buffer_rsrc_t rin = sc1_rsrc(in, slab_bytes);
    // the last stage's rows go straight to the caller's ados (every read of ados, stage 0's, is long done: a band
    // at stage >= 2 has loaded its sources' stage-1 rows, made after their stage-0 reads)
    const __amdgpu_buffer_rsrc_t rout =
        sc1_rsrc(g + 1 < G4 ? p.buf + (size_t)(g & 1) * slab : (c128*)p.ados, slab_bytes);
#ifdef QD_PHASE_TIMING
    const unsigned long long t0 = wall_clock64();
#endif
    // H(t), Q(t) of this stage (driven runs; every read of the previous stage's values is behind the barrier that
    // closed its stencil)
    if (pulsed) {
      const int ti = step * 3 + stage_time[stage];
      const c128 fs = p.fsv ? p.fsv[ti] : cmk(0, 0), fc = p.fcv ? p.fcv[ti] : cmk(0, 0);
      for (int q = tid; q < ns2; q += blockDim.x) sH[q] = p.Hdip ? cadd(p.H[q], cmul(p.Hdip[q], fs)) : p.H[q];
      for (int q = tid; q < p.nmod * ns2; q += blockDim.x)
        sQ[q] = p.Qdip ? cadd(p.Q[q], cmul(p.Qdip[q], fc)) : p.Q[q];
    }
#ifdef QD_PHASE_TIMING
    const unsigned long long t1 = wall_clock64();
#endif
    // 1-2. halo rows of the stage input -> LDS: sc1 loads re-issued for the granules whose lowest bits do not yet
    // hold stage g - 1's parity (the data is the flag; stage 0 of step 0 reads the caller's ados)
    {
      const unsigned tg = (unsigned)((g - 1) >> 1) & 1u;
      bool good = true;
      c128 hv[BAND_HM];
      // the first pass ~256 clocks after the publish (sooner only adds traffic; 116k -> 119k steps/s at 6188 ADOs,
      // 8 or 16 units were no better, 32 slower: profiles/r05/deom/band_first_sweep.txt)
      if (g > 0) __builtin_amdgcn_s_sleep(4);
#pragma unroll
      for (int h = 0; h < BAND_HM; ++h) hv[h] = ld16_sc1(rin, hsrc[h] < 0 ? 0 : hsrc[h]);
      if (g > 0) {
        for (unsigned spins = 0;;) {
          bool okh[BAND_HM], ok = true;
#pragma unroll
          for (int h = 0; h < BAND_HM; ++h) {
            okh[h] = hsrc[h] < 0 || band_has(hv[h], tg);
            ok &= okh[h];
          }
          if (__all(ok)) break;
          if (++spins > BAND_SPIN_LIMIT || band_abort_seen(p.status, spins)) {
            good = false;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
          asm volatile("" ::: "memory");   // the granules change under us: re-load, never reuse the value
#pragma unroll
          for (int h = 0; h < BAND_HM; ++h)
            if (!okh[h]) hv[h] = ld16_sc1(rin, hsrc[h]);
        }
      }
#pragma unroll
      for (int h = 0; h < BAND_HM; ++h)
        if (hsrc[h] >= 0) sX[(size_t)no * ns2 + tid + h * blockDim.x] = hv[h];
      for (int q = tid + BAND_HM * (int)blockDim.x; q < nhe && good; q += blockDim.x) {
        const int r = q / ns2, c = q - r * ns2, off = (p.halo_idx[hoff + r] * ns2 + c) * 16;
        c128 v = ld16_sc1(rin, off);
        for (unsigned spins = 0; g > 0 && !band_has(v, tg);) {
          if (++spins > BAND_SPIN_LIMIT || band_abort_seen(p.status, spins)) {
            good = false;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
          asm volatile("" ::: "memory");
          v = ld16_sc1(rin, off);
        }
        sX[(size_t)(no + r) * ns2 + c] = v;
      }
      if (!good) {
        sAbort[g & 1] = 1;
        __hip_atomic_store(p.status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
    if (sAbort[g & 1]) break;   // uniform: written before this barrier, rewritten (slot g & 1) only after the next
#ifdef QD_PHASE_TIMING
    const unsigned long long t2 = wall_clock64();
#endif

    // 3. stencil (group-kernel arithmetic and order) from LDS
    const c128 own = sX[oown];
    c128 ym[KMAX], yp[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      ym[k] = sX[om[k]];
      yp[k] = sX[op[k]];
    }
    if (pulsed) read_hq();
    c128 d = early ? dpre : dlocal(own);
    c128 SL = cmk(0, 0), SR = cmk(0, 0);
    auto flush = [&](int m) {
      const c128* Qm = sQ + m * ns2;
      c128 t = cmk(0, 0);
      for_l([&](int l) {
        if constexpr (FAST)
          t = cadd(t, cadd(cmul(qil[l], colv(SL, l)), cmul(rowv(SR, l), qlj[l])));
        else
          t = cadd(t, cadd(cmul(Qm[i * ns + l], colv(SL, l)), cmul(rowv(SR, l), Qm[l * ns + j])));
      });
      d = cadd(d, t);
    };
    int mcur = md[0];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k >= K) break;
      const int m = md[k];
      if (m != mcur) {
        flush(mcur);
        SL = SR = cmk(0, 0);
        mcur = m;
      }
      c128 cL, cR, cP;
      if constexpr (FULLC) {
        cL = cf[3 * k];
        cR = cf[3 * k + 1];
        cP = cf[3 * k + 2];
      } else {
        cL = bc(lc[(3 * k) / G], (3 * k) % G);
        cR = bc(lc[(3 * k + 1) / G], (3 * k + 1) % G);
        cP = bc(lc[(3 * k + 2) / G], (3 * k + 2) % G);
      }
      const c128 py = cmul(cP, yp[k]);
      SL = cadd(SL, cadd(cmul(cL, ym[k]), py));
      SR = cadd(SR, csub(cmul(cR, ym[k]), py));
    }
    flush(mcur);
    // RK4 epilogue (deom_rk4_next, as the stage kernels: Horner form unless driven)
    const c128 xo = deom_rk4_next(stage, !pulsed, dt, r0, acc, d);
    if (stage == 3) r0 = xo;
    // 4. publish: the global row write-through with stage g's parity in every double's lowest bit (the last stage's
    // rows, read by no band, carry the exact final state the host copies out) -- ahead of the barrier, which only
    // guards the band's LDS rows -- then the LDS row
    if (valid) st16_sc1(rout, (n * ns2 + e) * 16, g + 1 < G4 ? band_tag(xo, (unsigned)(g >> 1) & 1u) : xo);
    __syncthreads();   // every read of sX done
#ifdef QD_PHASE_TIMING
    const unsigned long long t3 = wall_clock64();
#endif
    if (valid) {
      sX[(size_t)a * ns2 + e] = xo;
      if (stage == 3 && p.snap && n == 0) p.snap[(size_t)(step + 1) * ns2 + e] = r0;
    }
    if (early) dpre = dlocal(xo);   // next stage's own element is xo (a padding lane's is never read)
#ifdef QD_PHASE_TIMING
    const unsigned long long t4 = wall_clock64();
    tph[0] += t1 - t0;
    tph[1] += t2 - t1;
    tph[2] += t3 - t2;
    tph[3] += t4 - t3;
#endif
  }
#ifdef QD_PHASE_TIMING
  if (tid == 0 && p.tim)
    for (int h = 0; h < 4; ++h) p.tim[w * 4 + h] = tph[h];
#endif
}

}  // namespace
