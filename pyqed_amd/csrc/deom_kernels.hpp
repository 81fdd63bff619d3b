// deom_kernels.hpp — the stage kernels of the DEOM hierarchy (deom.hip) for the shapes with a kernel of their own:
// DeomParams and the RK4 epilogue every DEOM kernel shares (deom_rk4_next), the element kernel (any B, ns <= 16,
// nmod <= 8), the lane-group kernel (ns^2 <= 64, K <= 8) with its five-waves twin, its software-pipelined persistent
// form (undriven ns = 2 ADO-major batches) and the 16 x 16 MFMA kernel (9 <= ns <= 16); the snapshot / trace kernels,
// the Euler chain of oqs._heom and the row gather.  Which of them runs a shape: deom_plan.hpp.
#pragma once

#include "deom_plan.hpp"
#include "handoff.hpp"
#include "qd_common.hpp"

namespace qd {
namespace {

struct DeomParams {
  const c128* rho;     // [B][nmax][ns][ns]   state at step start (stage 0 input)
  c128* rho_out;       // same buffer as rho (written at stage 3 only)
  const c128* xin;     // stage input (stage 0: rho)
  c128* xout;          // next-stage input
  c128* acc;           // RK4 accumulator
  const int* minus;    // [nmax][K]
  const int* plus;     // [nmax][K]
  const c128* coef;    // [nmax][K][3] : cL, cR, cP
  const c128* damp;    // [nmax]
  const int* mode;     // [K]
  const c128* H;       // [ns][ns]
  const c128* Hdip;    // [ns][ns] or null
  const c128* Q;       // [nmod][ns][ns]
  const c128* Qdip;    // [nmod][ns][ns] or null
  c128 fs, fc;         // pulse values at this stage's time
  c128* snap;          // [B][nsteps+1][ns][ns] (rho_0 after each step) or null
  int B, nmax, K, ns, nmod, stage, step, nsteps;
  double dt;
  int bminor;  // ADO-major layout [nmax][B][ns][ns] (hierarchy index fastest; group kernel only)
  int xsplit;  // group kernel: 0 = flat lane numbering; X in {1, 2, 4, 8} = hierarchies dealt to X block classes
  int ntst;    // group kernel: non-temporal rho / acc accesses (host: state beyond the Infinity Cache's share)
  int bchunk;  // group kernel, ADO-major: hierarchies of a class walked in chunks of bchunk (0 = all at once)
  int horner;  // RK4 in Horner form (no pulse: the generator is constant over the step; acc unused)
};

// RK4 stage epilogue: returns the next stage input (stage < 3) or the new rho (stage 3); `acc` is the lane's RK4
// accumulator (in: its value after the previous stage, out: after this one).
//   classic (driven runs, H(t) / Q(t) at t, t + dt/2, t + dt): deom.py:735-766's order, ddos1 = k1; += 2 k2;
//     += 2 k3; += k4; ddos += ddos1 dt / 6, each stage input rho + c k;
//   Horner (no pulse): for a generator L constant over the step RK4 is exactly the degree-4 Taylor polynomial,
//     rho' = rho + dt L(rho + dt/2 L(rho + dt/3 L(rho + dt/4 L rho))), so stage m writes rho + dt / (4 - m) L s_m
//     and needs no accumulator (glf.hip header): one state row less read and written per stage.
__device__ __forceinline__ c128 deom_rk4_next(int stage, bool horner, double dt, c128 r0, c128& acc, c128 d) {
  if (horner) {   // explicit fma: the same rounding in every kernel whatever the compiler contracts around it
    const double c = rk4_horner_coef(dt, stage);
    return cmk(__builtin_fma(d.re, c, r0.re), __builtin_fma(d.im, c, r0.im));
  }
  if (stage == 0) {
    acc = d;
    return cadd(r0, cscale(d, dt / 2));
  }
  if (stage < 3) {
    acc = cadd(acc, cscale(d, 2.0));
    return cadd(r0, cscale(d, stage == 1 ? dt / 2 : dt));
  }
  return cadd(r0, cscale(cscale(cadd(acc, d), dt), 1.0 / 6.0));
}


// One element e of a stage (any B, ns <= DEOM_MAX_NS, nmod <= DEOM_MAX_NMOD, driven or not) with H(t), Q(t) of the
// stage in sH / sQ: the generic stage kernel and the banded launch's stream-ordered fallback run this.
__device__ __forceinline__ void deom_stage_element(const DeomParams& p, size_t e, const c128* sH, const c128* sQ) {
  const int ns = p.ns, ns2 = ns * ns;
  const int j = (int)(e % ns), i = (int)((e / ns) % ns);
  const size_t bn = e / ns2;                  // b * nmax + n
  const int n = (int)(bn % p.nmax);
  const size_t bbase = (bn - n) * ns2;        // start of batch member b
  const c128* X = p.xin + bbase;
  const c128* xn = X + (size_t)n * ns2;

  // damping + coherent part: damp_n x - i (H x - x H)
  c128 d = cmul(p.damp[n], xn[i * ns + j]);
  c128 comm = cmk(0, 0);
  for (int l = 0; l < ns; ++l)
    comm = cadd(comm, csub(cmul(sH[i * ns + l], xn[l * ns + j]), cmul(xn[i * ns + l], sH[l * ns + j])));
  d = cadd(d, cmulmi(comm));

  const int* mi = p.minus + (size_t)n * p.K;
  const int* pl = p.plus + (size_t)n * p.K;
  const c128* cf = p.coef + (size_t)n * p.K * 3;
  for (int k = 0; k < p.K; ++k) {
    const c128* Qm = sQ + p.mode[k] * ns2;
    const int nm = mi[k];
    if (nm >= 0) {
      const c128* y = X + (size_t)nm * ns2;
      c128 qy = cmk(0, 0), yq = cmk(0, 0);
      for (int l = 0; l < ns; ++l) {
        qy = cadd(qy, cmul(Qm[i * ns + l], y[l * ns + j]));
        yq = cadd(yq, cmul(y[i * ns + l], Qm[l * ns + j]));
      }
      d = cadd(d, cadd(cmul(cf[3 * k + 0], qy), cmul(cf[3 * k + 1], yq)));
    }
    const int np = pl[k];
    if (np >= 0) {
      const c128* y = X + (size_t)np * ns2;
      c128 c = cmk(0, 0);
      for (int l = 0; l < ns; ++l)
        c = cadd(c, csub(cmul(Qm[i * ns + l], y[l * ns + j]), cmul(y[i * ns + l], Qm[l * ns + j])));
      d = cadd(d, cmul(cf[3 * k + 2], c));
    }
  }

  // RK4 bookkeeping (deom_rk4_next)
  const c128 r0 = p.rho ? p.rho[e] : cmk(0, 0);   // rho == nullptr: qd_deom_apply
  c128 a = (p.stage > 0 && !p.horner) ? p.acc[e] : cmk(0, 0);
  const c128 v = deom_rk4_next(p.stage, p.horner, p.dt, r0, a, d);
  if (p.stage < 3) {
    if (!p.horner) p.acc[e] = a;
    p.xout[e] = v;
  } else {
    p.rho_out[e] = v;
    if (p.snap && n == 0) {
      const size_t b = bn / p.nmax;
      p.snap[(b * (p.nsteps + 1) + p.step + 1) * ns2 + i * ns + j] = v;
    }
  }
}

__device__ __forceinline__ void deom_stage_ops(const DeomParams& p, c128* sH, c128* sQ) {
  const int ns2 = p.ns * p.ns;
  for (int e = threadIdx.x; e < ns2; e += blockDim.x)
    sH[e] = p.Hdip ? cadd(p.H[e], cmul(p.Hdip[e], p.fs)) : p.H[e];
  for (int e = threadIdx.x; e < p.nmod * ns2; e += blockDim.x)
    sQ[e] = p.Qdip ? cadd(p.Q[e], cmul(p.Qdip[e], p.fc)) : p.Q[e];
}

__global__ __launch_bounds__(DEOM_TPB) void deom_stage_kernel(DeomParams p) {
  __shared__ c128 sH[DEOM_MAX_NS * DEOM_MAX_NS];
  __shared__ c128 sQ[DEOM_MAX_NMOD * DEOM_MAX_NS * DEOM_MAX_NS];
  deom_stage_ops(p, sH, sQ);
  __syncthreads();
  const size_t tot = (size_t)p.B * p.nmax * p.ns * p.ns;
  const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (e < tot) deom_stage_element(p, e, sH, sQ);
}

// Group kernel: G = next pow2 >= ns^2 lanes per ADO, one lane per matrix element, so every
// neighbour ADO is read once per group as one coalesced ns^2 x 16-B row (not once per row/column
// it touches).  The ADO's neighbour indices and prefactors are loaded ONCE per group: lane e loads
// entries e, e + G, ... of the ADO's rows (contiguous across the group) and the group broadcasts them
// (quad DPP for G = 4, lane shuffles otherwise), so a lane issues ~2K/G + 3K/G of these loads instead
// of 5K.  All of them are issued together with the lane's own element and RK4 state (round trip 1),
// then every neighbour element (round trip 2).  NS2: ns = 2 (G = 4) with every exchange of the
// 2 x 2 products a quad DPP move.  Every lane of a group follows the same branches (they share the
// ADO), so no exchange reads an inactive lane.  H(t), Q(t) go to dynamic LDS ((1 + nmod) ns^2).
typedef double deom_d2 __attribute__((ext_vector_type(2)));
// The RK4 state rho / acc is read and written once per stage by its own lane.  p.ntst: non-temporal accesses for
// those streams, so that they do not evict the stage input rows the 2K neighbour reads hit in the caches (set by
// the host for batches whose state outgrows the Infinity Cache; below that the plain accesses keep acc resident
// there from one stage to the next).
__device__ __forceinline__ c128 ld_once(const c128* q, bool nt) {
  if (nt) {
    const deom_d2 v = __builtin_nontemporal_load((const deom_d2*)q);
    return cmk(v.x, v.y);
  }
  return *q;
}
__device__ __forceinline__ void st_once(c128* q, c128 v, bool nt) {
  if (nt) __builtin_nontemporal_store(deom_d2{v.re, v.im}, (deom_d2*)q);
  else *q = v;
}

// a load through the constant address space: wave-uniform addresses become scalar loads (s_load) of tables the
// stage kernels never write
template <typename T>
__device__ __forceinline__ T ld_uniform(const T* q) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(4))) T*)q;
#else
  return *q;   // host pass of the device function only (never executed)
#endif
}

// UNI: every wave holds lanes of ONE ADO (ADO-major layout, B / xsplit a multiple of 64 / G), so the ADO's
// neighbour indices, prefactors and damping are wave-uniform scalar loads instead of per-group vector loads
// broadcast by DPP moves.
// HM: 1 = Horner-form stages fixed at compile time (no accumulator registers or code; the undriven ns = 2 launches),
// 0 = p.horner at run time.
template <int G, int KMAX, bool NS2, bool UNI = false, int HM = 0>
__device__ __forceinline__ void deom_stage_grp_body(const DeomParams& p) {
  const bool horner = HM ? true : (bool)p.horner;
  extern __shared__ c128 deom_lds[];
  c128* sH = deom_lds;
  c128* sQ = deom_lds + p.ns * p.ns;
  const int ns = NS2 ? 2 : p.ns, ns2 = ns * ns, K = p.K;
  // [B][nmax] layout: an ADO's neighbours are rows of its own hierarchy;
  // [nmax][B] layout (bminor): a wave holds one ADO of up to 64 / G hierarchies, so its index / prefactor loads
  // are one request per wave and each neighbour read is one contiguous run of 64-B rows.
  // xsplit = X > 0: block class c = blockIdx % 8 < X owns hierarchies [c B/X, (c+1) B/X) for every ADO, classes
  // >= X exit at once.  Blocks b and b + 8 share an XCD (round-robin dispatch, MI355X_MICROARCH.md "Workgroup
  // dispatch"), so one XCD reads only its own hierarchies' rows and the 2K neighbour reads of an ADO hit that
  // XCD's L2 instead of coming from the Infinity Cache eight times over.  Placement is a speed matter only.
  // 32-bit lane arithmetic (the host checks B nmax G < 2^31): one integer division per lane
  unsigned cls = 0, u;
  if (p.xsplit > 0) {
    cls = blockIdx.x & 7;
    if (cls >= (unsigned)p.xsplit) return;  // whole block exits before any barrier
    u = (blockIdx.x >> 3) * blockDim.x + threadIdx.x;
  } else {
    u = blockIdx.x * blockDim.x + threadIdx.x;
  }
  const unsigned Bx = p.xsplit > 0 ? (unsigned)(p.B / p.xsplit) : (unsigned)p.B;
  const unsigned lgrp = u / G;              // b nmax + n, or n B + b (bminor), within the class
  const int e = (int)(u % G);
  const bool live = lgrp < Bx * (unsigned)p.nmax;   // uniform within a group
  // bchunk = C > 0 (ADO-major): the class's hierarchies are walked in chunks of C, every ADO of one chunk before
  // the next chunk, so the neighbour rows the resident waves read (tiers l - 1 .. l + 1 of C hierarchies) stay
  // within the XCD's L2 instead of spanning all Bx hierarchies of the class
  unsigned lch = lgrp, boff = 0;
  if (p.bminor && p.bchunk > 0) {
    const unsigned per = (unsigned)p.bchunk * (unsigned)p.nmax;
    const unsigned ch = lgrp / per;
    lch = lgrp - ch * per;
    boff = ch * (unsigned)p.bchunk;
  }
  const unsigned q = p.bminor ? (p.bchunk > 0 ? (unsigned)p.bchunk : Bx) : (unsigned)p.nmax;
  const unsigned hi = lch / q, lo = lch - hi * q;
  const int n = live ? (int)(p.bminor ? hi : lo) : 0;
  const size_t hb = (size_t)cls * Bx + (live ? (p.bminor ? boff + lo : hi) : 0);   // hierarchy b
  const size_t grp = p.bminor ? (size_t)n * p.B + hb : hb * p.nmax + n;     // flat row of rho / acc / xout
  const bool valid = live && e < ns2;
  const size_t rs = p.bminor ? (size_t)p.B * ns2 : (size_t)ns2;         // ADO row stride
  const int ee = e < ns2 ? e : 0;           // padding lanes shadow element 0
  const c128* X = p.xin + (p.bminor ? hb * ns2 : hb * p.nmax * ns2);
  const int base = (int)(threadIdx.x & 63) & ~(G - 1);
  auto shfl = [&](c128 v, int src) { return cmk(__shfl(v.re, base + src, 64), __shfl(v.im, base + src, 64)); };
  // value of v held by lane `src` of this group (src is a compile-time constant after unrolling)
  auto bc = [&](c128 v, int src) -> c128 {
    if constexpr (G == 4) {
      switch (src) {
        case 0: return dpp_qc<0x00>(v);
        case 1: return dpp_qc<0x55>(v);
        case 2: return dpp_qc<0xAA>(v);
        default: return dpp_qc<0xFF>(v);
      }
    } else {
      return shfl(v, src);
    }
  };
  auto bci = [&](int v, int src) -> int {
    if constexpr (G == 4) {
      switch (src) {
        case 0: return dpp_qi<0x00>(v);
        case 1: return dpp_qi<0x55>(v);
        case 2: return dpp_qi<0xAA>(v);
        default: return dpp_qi<0xFF>(v);
      }
    } else {
      return __shfl(v, base + src, 64);
    }
  };

  // round trip 1: this lane's share of the indices and prefactors, own element, RK4 state, H/Q -> LDS
  constexpr int NI = UNI ? 1 : (KMAX + G - 1) / G;
  constexpr int NC = UNI ? 1 : (3 * KMAX + G - 1) / G;
  const int nu = UNI ? __builtin_amdgcn_readfirstlane(n) : n;
  int lm[NI], lp[NI];
  c128 lc[NC];
  if constexpr (!UNI) {
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      const int k = e + G * q;
      lm[q] = (live && k < K) ? p.minus[(size_t)n * K + k] : -1;
      lp[q] = (live && k < K) ? p.plus[(size_t)n * K + k] : -1;
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const int c = e + G * q;
      lc[q] = (live && c < 3 * K) ? p.coef[(size_t)n * K * 3 + c] : cmk(0, 0);
    }
  }
  const c128 own = live ? X[(size_t)n * rs + ee] : cmk(0, 0);
  const c128 dmp = UNI ? ld_uniform(p.damp + nu) : (live ? p.damp[n] : cmk(0, 0));
  const size_t idx = grp * ns2 + e;
  // stage 0 of the Horner form: the stage input is rho itself (own == rho[idx] for a valid lane)
  const c128 r0 = !valid ? cmk(0, 0) : (horner && p.stage == 0) ? own : p.rho ? ld_once(p.rho + idx, p.ntst) : cmk(0, 0);
  c128 a0 = (valid && p.stage > 0 && !horner) ? ld_once(p.acc + idx, p.ntst) : cmk(0, 0);
  for (int q = threadIdx.x; q < ns2; q += blockDim.x)
    sH[q] = p.Hdip ? cadd(p.H[q], cmul(p.Hdip[q], p.fs)) : p.H[q];
  for (int q = threadIdx.x; q < p.nmod * ns2; q += blockDim.x)
    sQ[q] = p.Qdip ? cadd(p.Q[q], cmul(p.Qdip[q], p.fc)) : p.Q[q];
  int im[KMAX], ip[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if constexpr (UNI) {
      im[k] = k < K ? ld_uniform(p.minus + (size_t)nu * K + k) : -1;
      ip[k] = k < K ? ld_uniform(p.plus + (size_t)nu * K + k) : -1;
    } else {
      im[k] = bci(lm[k / G], k % G);
      ip[k] = bci(lp[k / G], k % G);
    }
  }

  // round trip 2: every neighbour element this lane owns
  c128 ym[KMAX], yp[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    ym[k] = (k < K && im[k] >= 0) ? X[(size_t)im[k] * rs + ee] : cmk(0, 0);
    yp[k] = (k < K && ip[k] >= 0) ? X[(size_t)ip[k] * rs + ee] : cmk(0, 0);
  }
  __syncthreads();

  const int i = ee / ns, j = ee % ns;
  // v[l][j] and v[i][l] of this lane's group (v[i][j] held by lane i ns + j)
  auto colv = [&](c128 v, int l) -> c128 {
    if constexpr (NS2) return l == 0 ? dpp_qc<0x44>(v) : dpp_qc<0xEE>(v);   // lanes (0,1,0,1) / (2,3,2,3)
    else return shfl(v, l * ns + j);
  };
  auto rowv = [&](c128 v, int l) -> c128 {
    if constexpr (NS2) return l == 0 ? dpp_qc<0xA0>(v) : dpp_qc<0xF5>(v);   // lanes (0,0,2,2) / (1,1,3,3)
    else return shfl(v, i * ns + l);
  };
  auto for_l = [&](auto&& f) {   // l = 0 .. ns-1 (two literal calls for ns = 2)
    if constexpr (NS2) {
      f(0);
      f(1);
    } else {
      for (int l = 0; l < ns; ++l) f(l);
    }
  };

  // damping + coherent part: damp_n x - i (H x - x H)
  c128 d = cmul(dmp, own);
  c128 comm = cmk(0, 0);
  for_l([&](int l) {
    comm = cadd(comm, csub(cmul(sH[i * ns + l], colv(own, l)), cmul(rowv(own, l), sH[l * ns + j])));
  });
  d = cadd(d, cmulmi(comm));
  // Dissipaton terms regrouped by bath mode m (as the MFMA tile kernel below):
  //   sum_{k: mode m} cL y_- Q.. = Q_m SL_m + SR_m Q_m,  SL_m = sum_k (cL_k y_{n-e_k} + cP_k y_{n+e_k}),
  //   SR_m = sum_k (cR_k y_{n-e_k} - cP_k y_{n+e_k}),
  // so a lane scales its own neighbour elements per k (absent neighbours were loaded as 0) and the 2 x 2 ... ns x ns
  // products and their lane exchanges run once per run of equal modes instead of three times per k.
  c128 SL = cmk(0, 0), SR = cmk(0, 0);
  auto flush = [&](int m) {
    const c128* Qm = sQ + m * ns2;
    c128 t = cmk(0, 0);
    for_l([&](int l) { t = cadd(t, cadd(cmul(Qm[i * ns + l], colv(SL, l)), cmul(rowv(SR, l), Qm[l * ns + j]))); });
    d = cadd(d, t);
  };
  int mcur = p.mode[0];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    if (k >= K) break;
    const int m = p.mode[k];
    if (m != mcur) {   // wave-uniform
      flush(mcur);
      SL = SR = cmk(0, 0);
      mcur = m;
    }
    c128 cL, cR, cP;
    if constexpr (UNI) {
      const c128* cf = p.coef + ((size_t)nu * K + k) * 3;
      cL = ld_uniform(cf);
      cR = ld_uniform(cf + 1);
      cP = ld_uniform(cf + 2);
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
  if (!valid) return;

  const c128 v = deom_rk4_next(p.stage, horner, p.dt, r0, a0, d);
  if (p.stage < 3) {
    if (!horner) st_once(p.acc + idx, a0, p.ntst);
    p.xout[idx] = v;
  } else {
    p.rho_out[idx] = v;
    if (p.snap && n == 0) p.snap[(hb * (p.nsteps + 1) + p.step + 1) * ns2 + e] = v;
  }
}

template <int G, int KMAX, bool NS2, bool UNI = false, int HM = 0>
__global__ __launch_bounds__(DEOM_TPB) void deom_stage_grp_kernel(DeomParams p) {
  deom_stage_grp_body<G, KMAX, NS2, UNI, HM>(p);
}
// The same body held to five waves per SIMD (96 VGPRs, 12 B of spill at K = 5): the undriven ns = 2 batches of >= 64
// hierarchies whose XCD classes are not wave-uniform (64 hierarchies: 30.5 -> 29.8 us per stage; at 16 hierarchies
// it is slower, 11.2 vs 10.3: profiles/r03/deom/horner_compile_time_ab.txt)
template <int G, int KMAX, bool NS2, bool UNI, int HM>
__global__ __launch_bounds__(DEOM_TPB) __attribute__((amdgpu_waves_per_eu(5))) void deom_stage_grp_w5_kernel(DeomParams p) {
  deom_stage_grp_body<G, KMAX, NS2, UNI, HM>(p);
}

// Software-pipelined persistent form of the ns = 2 group kernel for undriven ADO-major batches (Horner stages, XCD
// classes of B / 8 hierarchies, no hierarchy chunks): a fixed grid whose waves walk the class's lane groups with a
// stride, and while one group's neighbour rows are in flight the NEXT group's neighbour indices, own element and
// stage state are loaded.  The stage kernels above spend two dependent memory round trips per wave (tables + own
// rows, then the neighbour rows the tables point at), once per wave generation; here a wave pays about one per group
// after the first.  Same per-element arithmetic in the same order as deom_stage_grp_body<4, KMAX, true, false, 1>,
// so the result is bit-identical (tests/test_deom_gpu.py); H / Q go to LDS once per workgroup.  Every gather and the
// state accesses are buffer loads / stores at 32-bit byte offsets, a dead lane's at BUF_OOB (zeros / dropped), and the
// lane-group coordinates advance by a carry step: against 64-bit global addresses with a branch around each
// conditional load and a division per group, 64 hierarchies 28.9 -> 26.0 us per stage
// (profiles/r04/deom/deom_buf_ab.txt, deom_buf2_ab.txt).
template <int KMAX>
__global__ __launch_bounds__(DEOM_TPB) void deom_stage_pipe_kernel(DeomParams p) {
  constexpr int G = 4, NI = (KMAX + G - 1) / G, NC = (3 * KMAX + G - 1) / G;
  extern __shared__ c128 deom_lds[];
  c128* sH = deom_lds;
  c128* sQ = deom_lds + 4;
  for (int q = threadIdx.x; q < 4; q += blockDim.x) sH[q] = p.H[q];
  for (int q = threadIdx.x; q < p.nmod * 4; q += blockDim.x) sQ[q] = p.Q[q];
  __syncthreads();
  const int K = p.K;
  const unsigned cls = blockIdx.x & 7;
  const unsigned Bx = (unsigned)(p.B / p.xsplit);
  const unsigned per = Bx * (unsigned)p.nmax * G;            // lanes of this class
  const unsigned stride = (gridDim.x >> 3) * blockDim.x;
  const unsigned lane = threadIdx.x & 63;
  const int e = (int)(threadIdx.x & 3);
  const int base = (int)lane & ~(G - 1);
  const int i = e >> 1, j = e & 1;
  auto bc = [&](c128 v, int src) -> c128 {
    switch (src) {
      case 0: return dpp_qc<0x00>(v);
      case 1: return dpp_qc<0x55>(v);
      case 2: return dpp_qc<0xAA>(v);
      default: return dpp_qc<0xFF>(v);
    }
  };
  auto bci = [&](int v, int src) -> int {
    switch (src) {
      case 0: return dpp_qi<0x00>(v);
      case 1: return dpp_qi<0x55>(v);
      case 2: return dpp_qi<0xAA>(v);
      default: return dpp_qi<0xFF>(v);
    }
  };
  auto colv = [&](c128 v, int l) -> c128 { return l == 0 ? dpp_qc<0x44>(v) : dpp_qc<0xEE>(v); };
  auto rowv = [&](c128 v, int l) -> c128 { return l == 0 ? dpp_qc<0xA0>(v) : dpp_qc<0xF5>(v); };
  // the part of a group's inputs that addresses nothing else: its neighbour indices and own element
  struct Head {
    int lm[NI], lp[NI];
    c128 own;
    int n;
    unsigned hb, off;   // off: byte offset of this lane's element of the ADO row (BUF_OOB for a dead lane)
    bool live;
  };
  // every gather is a buffer load at a 32-bit byte offset (the host keeps every table below 2^31 bytes and the
  // factors of the __umul24 products below 2^24); a dead load takes BUF_OOB and returns zeros, the value the plain
  // form selects (no 64-bit address arithmetic, no branch around the loads)
  const unsigned nx = (unsigned)p.nmax;
  const __amdgpu_buffer_rsrc_t rX = buf_rsrc(p.xin, (int)(nx * (unsigned)p.B * 64u));
  const __amdgpu_buffer_rsrc_t rCo = buf_rsrc(p.coef, (int)(nx * (unsigned)K * 48u));
  const __amdgpu_buffer_rsrc_t rDa = buf_rsrc(p.damp, (int)(nx * 16u));
  const __amdgpu_buffer_rsrc_t rMi = buf_rsrc(p.minus, (int)(nx * (unsigned)K * 4u));
  const __amdgpu_buffer_rsrc_t rPl = buf_rsrc(p.plus, (int)(nx * (unsigned)K * 4u));
  const unsigned rsb = (unsigned)p.B * 64u;                 // ADO row stride in bytes
  const int xbytes = (int)(nx * (unsigned)p.B * 64u);
  const __amdgpu_buffer_rsrc_t rR = buf_rsrc(p.rho, p.rho ? xbytes : 0), rXo = buf_rsrc(p.xout, xbytes);
  const __amdgpu_buffer_rsrc_t rRo = buf_rsrc(p.rho_out, xbytes);
  // lane group lgrp = u / G of the class is (ADO hi, hierarchy lo) with lgrp = hi Bx + lo; a wave's next group is
  // stride / G further on, so (hi, lo) advance by a constant carry step instead of a division per group
  auto head = [&](unsigned uu, unsigned hi, unsigned lo, Head& h) {
    h.live = uu < per;
    h.n = h.live ? (int)hi : 0;
    h.hb = cls * Bx + (h.live ? lo : 0);
    const unsigned nk = __umul24((unsigned)h.n, (unsigned)K);
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      const int k = e + G * q;
      const bool ok = h.live && k < K;
      const int vm = ld4_buf(rMi, ok ? (nk + (unsigned)k) * 4u : BUF_OOB);
      const int vp = ld4_buf(rPl, ok ? (nk + (unsigned)k) * 4u : BUF_OOB);
      h.lm[q] = ok ? vm : -1;
      h.lp[q] = ok ? vp : -1;
    }
    h.off = h.live ? __umul24((unsigned)h.n, rsb) + h.hb * 64u + (unsigned)e * 16u : BUF_OOB;
    h.own = ld16_buf(rX, h.off);
  };
  unsigned u = (blockIdx.x >> 3) * blockDim.x + threadIdx.x;
  const unsigned sg = stride / G, sg_hi = sg / Bx, sg_lo = sg - sg_hi * Bx;
  unsigned ghi = (u / G) / Bx, glo = (u / G) - ghi * Bx;
  Head cur;
  head(u, ghi, glo, cur);
  // the modes of the K directions, once (scalar loads): the per-group mode tests are then uniform branches that wait
  // on no memory
  int modek[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) modek[k] = k < K ? ld_uniform(p.mode + k) : 0;
  while (__builtin_amdgcn_readfirstlane(u - lane) < per) {   // wave-uniform trip count (DPP needs whole quads)
    // this group's prefactors, damping and neighbour rows
    c128 lc[NC];
    const unsigned n3k = __umul24((unsigned)cur.n, 3u * (unsigned)K);
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const int c = e + G * q;
      lc[q] = ld16_buf(rCo, (cur.live && c < 3 * K) ? (n3k + (unsigned)c) * 16u : BUF_OOB);
    }
    const c128 dmp = ld16_buf(rDa, cur.live ? (unsigned)cur.n * 16u : BUF_OOB);
    // r0: the own element at stage 0, else rho's (zero on a dead lane: its offset is out of range)
    const c128 r0 = p.stage == 0 ? cur.own : p.ntst ? ld16_buf_nt(rR, cur.off) : ld16_buf(rR, cur.off);
    c128 ym[KMAX], yp[KMAX];
    const unsigned xb = cur.hb * 64u + (unsigned)e * 16u;   // this lane's element within a row
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int im = bci(cur.lm[k / G], k % G), ip = bci(cur.lp[k / G], k % G);
      ym[k] = ld16_buf(rX, (k < K && im >= 0) ? __umul24((unsigned)im, rsb) + xb : BUF_OOB);
      yp[k] = ld16_buf(rX, (k < K && ip >= 0) ? __umul24((unsigned)ip, rsb) + xb : BUF_OOB);
    }
    // the next group's head, in flight with the rows above
    const unsigned un = u + stride;
    unsigned nlo = glo + sg_lo, nhi = ghi + sg_hi;
    if (nlo >= Bx) {
      nlo -= Bx;
      ++nhi;
    }
    Head nxt;
    head(un, nhi, nlo, nxt);
    // stencil: deom_stage_grp_body's ns = 2 arithmetic, operation for operation
    c128 d = cmul(dmp, cur.own);
    c128 comm = cmk(0, 0);
#pragma unroll
    for (int l = 0; l < 2; ++l)
      comm = cadd(comm, csub(cmul(sH[i * 2 + l], colv(cur.own, l)), cmul(rowv(cur.own, l), sH[l * 2 + j])));
    d = cadd(d, cmulmi(comm));
    c128 SL = cmk(0, 0), SR = cmk(0, 0);
    auto flush = [&](int m) {
      const c128* Qm = sQ + m * 4;
      c128 t = cmk(0, 0);
#pragma unroll
      for (int l = 0; l < 2; ++l) t = cadd(t, cadd(cmul(Qm[i * 2 + l], colv(SL, l)), cmul(rowv(SR, l), Qm[l * 2 + j])));
      d = cadd(d, t);
    };
    int mcur = modek[0];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k >= K) break;
      const int m = modek[k];
      if (m != mcur) {
        flush(mcur);
        SL = SR = cmk(0, 0);
        mcur = m;
      }
      const c128 cL = bc(lc[(3 * k) / G], (3 * k) % G);
      const c128 cR = bc(lc[(3 * k + 1) / G], (3 * k + 1) % G);
      const c128 cP = bc(lc[(3 * k + 2) / G], (3 * k + 2) % G);
      const c128 py = cmul(cP, yp[k]);
      SL = cadd(SL, cadd(cmul(cL, ym[k]), py));
      SR = cadd(SR, csub(cmul(cR, ym[k]), py));
    }
    flush(mcur);
    {   // a dead lane's store goes to an out-of-range offset (dropped)
      c128 a0 = cmk(0, 0);
      const c128 v = deom_rk4_next(p.stage, true, p.dt, r0, a0, d);
      if (p.stage < 3) {
        st16_buf(rXo, cur.off, v);
      } else {
        st16_buf(rRo, cur.off, v);
        if (p.snap && cur.live && cur.n == 0) p.snap[((size_t)cur.hb * (p.nsteps + 1) + p.step + 1) * 4 + e] = v;
      }
    }
    cur = nxt;
    u = un;
    ghi = nhi;
    glo = nlo;
  }
}

// MFMA tile kernel for 9 <= ns <= 16 (zero-padded to 16 in registers), NM <= 2 bath modes, K <= 21: one wave per
// ADO.  The stencil regrouped by mode m:
//   d rho_n = damp_n x - iH x + x iH + sum_m (Q_m SL_m + SR_m Q_m),
//   SL_m = sum_{k: mode k = m} (cL_k x_{n-e_k} + cP_k x_{n+e_k}),  SR_m = sum_k (cR_k x_{n-e_k} - cP_k x_{n+e_k}),
// i.e. two complex 16 x 16(1+NM) x 16 GEMMs per ADO on v_mfma_f64_16x16x4_f64:
//   D  = [-iH | Q_1 .. Q_NM] [x; SL_1 ..]   (B operand = the D-register layout of x and SL: no data movement)
//   D += [x | SR_1 ..] [iH; Q_1 ..]          (A operand = the transposed layout: one 16 x 17 LDS transpose per block)
// Every matrix is loaded once in the MFMA D layout (lane l: rows (l>>4) + 4r, column l&15; 4 x 256-B row pieces
// per load instruction); neighbour loads are branch-free (absent neighbours read the ADO's own row with a zero
// coefficient) so the compiler can issue them ahead.  The RK4 epilogue is the group kernel's.
template <int NM>
__global__ __launch_bounds__(256) void deom_stage_mfma16_kernel(DeomParams p) {
  extern __shared__ c128 deom_lds[];
  c128* sH = deom_lds;                            // [16][16] H(t), zero padded
  c128* sQ = deom_lds + 256;                      // [NM][16][16] Q_m(t)
  c128* sT = deom_lds + 256 * (1 + NM) + (threadIdx.x >> 6) * (16 * 17);   // this wave's transpose tile
  const int ns = p.ns, ns2 = ns * ns, K = p.K;
  for (int e = threadIdx.x; e < 256 * (1 + NM); e += 256) {
    const int mtx = e >> 8, i = (e >> 4) & 15, j = e & 15;
    c128 v = cmk(0, 0);
    if (i < ns && j < ns) {
      const int q = i * ns + j;
      if (mtx == 0) v = p.Hdip ? cadd(p.H[q], cmul(p.Hdip[q], p.fs)) : p.H[q];
      else v = p.Qdip ? cadd(p.Q[(mtx - 1) * ns2 + q], cmul(p.Qdip[(mtx - 1) * ns2 + q], p.fc)) : p.Q[(mtx - 1) * ns2 + q];
    }
    deom_lds[e] = v;
  }
  const long total = (long)p.B * p.nmax;
  const long g0 = blockIdx.x * 4L + (threadIdx.x >> 6);
  const bool valid = g0 < total;                  // out-of-range waves compute a copy and store nothing
  const long grp = valid ? g0 : total - 1;
  const int n = (int)(grp % p.nmax);
  const long hb = grp / p.nmax;
  const c128* X = p.xin + hb * p.nmax * ns2;
  const int lane = threadIdx.x & 63, col = lane & 15, rq = lane >> 4;
  const bool colv = col < ns;
  auto ld = [&](const c128* M, int r) -> c128 {
    const int i = rq + 4 * r;
    return (colv && i < ns) ? M[i * ns + col] : cmk(0, 0);
  };
  int myidx = -1;
  c128 mycf = cmk(0, 0);
  if (lane < 2 * K) myidx = lane < K ? p.minus[(size_t)n * K + lane] : p.plus[(size_t)n * K + lane - K];
  if (lane < 3 * K) mycf = p.coef[(size_t)n * K * 3 + lane];
  const size_t own = (size_t)grp * ns2;
  c128 x[4], r0[4], a0[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    x[r] = ld(X + (size_t)n * ns2, r);
    r0[r] = p.rho ? ld(p.rho + own, r) : cmk(0, 0);
    a0[r] = (p.stage > 0 && !p.horner) ? ld(p.acc + own, r) : cmk(0, 0);
  }
  const c128 dmp = p.damp[n];
  c128 SL[NM][4], SR[NM][4];
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) SL[m][r] = SR[m][r] = cmk(0, 0);
  auto shc = [&](c128 v, int src) { return cmk(__shfl(v.re, src, 64), __shfl(v.im, src, 64)); };
#pragma unroll 2
  for (int k = 0; k < K; ++k) {
    const int m = NM == 1 ? 0 : p.mode[k];
    const int im = __shfl(myidx, k, 64), ip = __shfl(myidx, K + k, 64);
    const c128 cL = im >= 0 ? shc(mycf, 3 * k) : cmk(0, 0);
    const c128 cR = im >= 0 ? shc(mycf, 3 * k + 1) : cmk(0, 0);
    const c128 cP = ip >= 0 ? shc(mycf, 3 * k + 2) : cmk(0, 0);
    const c128* ym = X + (size_t)(im >= 0 ? im : n) * ns2;
    const c128* yp = X + (size_t)(ip >= 0 ? ip : n) * ns2;
    c128 vm[4], vp[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      vm[r] = ld(ym, r);
      vp[r] = ld(yp, r);
    }
#pragma unroll
    for (int mm = 0; mm < NM; ++mm) {
      if (mm != m) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        SL[mm][r] = cadd(SL[mm][r], cadd(cmul(cL, vm[r]), cmul(cP, vp[r])));
        SR[mm][r] = cadd(SR[mm][r], csub(cmul(cR, vm[r]), cmul(cP, vp[r])));
      }
    }
  }
  __syncthreads();  // H(t) / Q(t) in LDS
  d4 Dre = d4{0.0, 0.0, 0.0, 0.0}, Dim = d4{0.0, 0.0, 0.0, 0.0};
  auto cmfma = [&](c128 a, c128 b) {  // D += a b (complex, one 16x16x4 k-step)
    Dre = __builtin_amdgcn_mfma_f64_16x16x4f64(a.re, b.re, Dre, 0, 0, 0);
    Dim = __builtin_amdgcn_mfma_f64_16x16x4f64(a.re, b.im, Dim, 0, 0, 0);
    Dre = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.im, b.im, Dre, 0, 0, 0);
    Dim = __builtin_amdgcn_mfma_f64_16x16x4f64(a.im, b.re, Dim, 0, 0, 0);
  };
  // GEMM 1: A = [-iH | Q_m] (lane: row l&15, column 4q + (l>>4)), B = [x; SL_m] in D layout (register q)
#pragma unroll
  for (int q = 0; q < 4; ++q) cmfma(cmulmi(sH[(lane & 15) * 16 + 4 * q + rq]), x[q]);
#pragma unroll
  for (int m = 0; m < NM; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) cmfma(sQ[m * 256 + (lane & 15) * 16 + 4 * q + rq], SL[m][q]);
  // GEMM 2: A = [x | SR_m] transposed through LDS, B = [iH; Q_m] (lane: row 4q + (l>>4), column l&15)
  auto gemm2_block = [&](const c128* Y, const c128* Bm, bool iH) {
#pragma unroll
    for (int r = 0; r < 4; ++r) sT[(rq + 4 * r) * 17 + col] = Y[r];
    __syncthreads();
    c128 a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = sT[(lane & 15) * 17 + 4 * q + rq];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const c128 b = Bm[(4 * q + rq) * 16 + col];
      cmfma(a[q], iH ? cmuli(b) : b);
    }
  };
  gemm2_block(x, sH, true);
#pragma unroll
  for (int m = 0; m < NM; ++m) gemm2_block(SR[m], sQ + m * 256, false);

  const double dt = p.dt;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = rq + 4 * r;
    if (!(valid && colv && i < ns)) continue;
    const c128 d = cadd(cmk(Dre[r], Dim[r]), cmul(dmp, x[r]));
    const size_t idx = own + (size_t)i * ns + col;
    c128 a = a0[r];
    const c128 v = deom_rk4_next(p.stage, p.horner, dt, r0[r], a, d);
    if (p.stage < 3) {
      if (!p.horner) p.acc[idx] = a;
      p.xout[idx] = v;
    } else {
      p.rho_out[idx] = v;
      if (p.snap && n == 0) p.snap[(hb * (p.nsteps + 1) + p.step + 1) * ns2 + (size_t)i * ns + col] = v;
    }
  }
}

__global__ void deom_snap0_kernel(const c128* rho, c128* snap, int B, int nmax, int ns, int nsteps, int bminor) {
  const int ns2 = ns * ns;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B * ns2; e += gridDim.x * blockDim.x) {
    const int b = e / ns2, ij = e % ns2;
    snap[(size_t)b * (nsteps + 1) * ns2 + ij] = rho[(size_t)b * (bminor ? 1 : nmax) * ns2 + ij];
  }
}

// obs[b][s][m] = Tr(E_m rho_0(s)) = sum_ij E_m[j][i] rho[i][j]   (deom.py:1100,1113)
__global__ void deom_trace_kernel(const c128* snap, const c128* E, int ne, int B, int ns, int nsnap, c128* obs) {
  const int ns2 = ns * ns;
  const int tot = B * nsnap * ne;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += gridDim.x * blockDim.x) {
    const int m = e % ne, bs = e / ne;
    const c128* r = snap + (size_t)bs * ns2;
    const c128* Em = E + (size_t)m * ns2;
    c128 s = cmk(0, 0);
    for (int i = 0; i < ns; ++i)
      for (int j = 0; j < ns; ++j) s = cadd(s, cmul(Em[j * ns + i], r[i * ns + j]));
    obs[e] = s;
  }
}

// oqs._heom (pyqed/oqs.py:1808-1875): single-exponential chain, explicit in-place sweep per
// step (ADO n uses the already-updated n-1, the old n and n+1; ADO nado-1 is never updated).
// One workgroup per hierarchy, threads loop over the ns^2 matrix elements (any ns); the new ADO n is
// staged in `tmp` (ns^2 per hierarchy) and copied in behind a barrier.
__global__ __launch_bounds__(256) void heom_chain_sweep_kernel(c128* ados, int nado, int ns, const c128* H,
                                                               const c128* Q, double gamma, c128 D0, double dt,
                                                               int nsteps, c128* snap, c128* tmp_all) {
  const int ns2 = ns * ns;
  c128* A = ados + (size_t)blockIdx.x * nado * ns2;
  c128* tmp = tmp_all + (size_t)blockIdx.x * ns2;
  auto comm = [&](const c128* X, const c128* Y, int ii, int jj) {  // (X Y - Y X)[ii][jj]
    c128 s = cmk(0, 0);
    for (int l = 0; l < ns; ++l) s = cadd(s, csub(cmul(X[ii * ns + l], Y[l * ns + jj]), cmul(Y[ii * ns + l], X[l * ns + jj])));
    return s;
  };
  auto acomm = [&](const c128* X, const c128* Y, int ii, int jj) {
    c128 s = cmk(0, 0);
    for (int l = 0; l < ns; ++l) s = cadd(s, cadd(cmul(X[ii * ns + l], Y[l * ns + jj]), cmul(Y[ii * ns + l], X[l * ns + jj])));
    return s;
  };
  if (snap)
    for (int t = threadIdx.x; t < ns2; t += blockDim.x) snap[(size_t)blockIdx.x * (nsteps + 1) * ns2 + t] = A[t];
  for (int s = 0; s < nsteps; ++s) {
    for (int n = 0; n < nado - 1; ++n) {
      for (int t = threadIdx.x; t < ns2; t += blockDim.x) {
        const int i = t / ns, j = t % ns;
        const c128* xn = A + (size_t)n * ns2;
        const c128* xp = A + (size_t)(n + 1) * ns2;
        const c128 x = xn[t];
        c128 v;
        if (n == 0) {
          v = csub(csub(x, cscale(cmuli(comm(H, xn, i, j)), dt)), cscale(comm(Q, xp, i, j), dt));
        } else {
          const c128* xm = A + (size_t)(n - 1) * ns2;
          const c128 coh = cscale(cmulmi(comm(H, xn, i, j)), dt);
          c128 inner = csub(cscale(comm(Q, xp, i, j), -1.0), cscale(x, n * gamma));
          const c128 mix = cadd(cscale(comm(Q, xm, i, j), D0.re), cmuli(cscale(acomm(Q, xm, i, j), D0.im)));
          inner = cadd(inner, cscale(mix, (double)n));
          v = cadd(x, cadd(coh, cscale(inner, dt)));
        }
        tmp[t] = v;
      }
      __syncthreads();
      for (int t = threadIdx.x; t < ns2; t += blockDim.x) A[(size_t)n * ns2 + t] = tmp[t];
      __syncthreads();
    }
    if (snap)
      for (int t = threadIdx.x; t < ns2; t += blockDim.x)
        snap[((size_t)blockIdx.x * (nsteps + 1) + s + 1) * ns2 + t] = A[t];
  }
}

}  // namespace
}  // namespace qd

using namespace qd;   // as deom.hip: the kernel below keeps its file-local symbol

namespace {
// Bounds-checked (the round-3 kernel trusted idx): a row index outside [0, nsrc) reads
// nothing, writes NaN and raises *bad, which the host entry point reports.
__global__ void gather_rows_kernel(const c128* src, int nsrc, const int32_t* idx, int n, int row, c128* dst,
                                   int* bad) {
  const size_t tot = (size_t)n * row;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
    const int r = idx[e / row];
    if (r >= 0 && r < nsrc) {
      dst[e] = src[(size_t)r * row + e % row];
    } else {
      dst[e] = cmk(__builtin_nan(""), __builtin_nan(""));
      if (bad) *bad = 1;   // vector store (global_store): benign race, every writer stores 1
    }
  }
}
}  // namespace
