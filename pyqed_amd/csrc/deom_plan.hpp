// deom_plan.hpp — the shape decisions of the DEOM launches (deom.hip) in plain C++17, no HIP, so that a host build can
// enumerate them (tools/cpu_emu/deom_plan_c.cpp, tests/test_deom_plan_host.py).  deom_stage_plan says which kernel
// runs one RK4 stage of a batch of hierarchies, with its template values, launch geometry, the layout values the
// launcher writes into DeomParams and the name the run is noted under; deom_band_plan does the same for the
// one-hierarchy banded launch.  A shape no kernel takes is refused with the entry point's message.  dispatch_stage /
// dispatch_band turn a plan into compile-time values; their lists are the DEOM kernels that exist.
#pragma once

#include <cstddef>
#include <cstdio>

#include "typed_dispatch.hpp"

namespace qd {

constexpr int DEOM_MAX_NS = 16;
constexpr int DEOM_MAX_NMOD = 8;
constexpr int DEOM_TPB = 256;
constexpr int DEOM_TT = 16;   // tile edge of the any-ns kernels (deom_tile_kernels.hpp)
constexpr size_t DEOM_LDS_MAX = 160 * 1024;

// ---------------------------------------------------------------- one RK4 stage (qd_deom_rk4, qd_deom_stage, ...)
// Kernel families: deom_stage_kernel, deom_stage_grp_kernel, deom_stage_grp_w5_kernel, deom_stage_pipe_kernel,
// deom_stage_mfma16_kernel, deom_stage_tile_kernel, deom_stage_tmfma_kernel.
enum StageKind { ST_ELEMENT, ST_GROUP, ST_GROUP_W5, ST_PIPE, ST_MFMA16, ST_TILE, ST_TMFMA, STAGE_KINDS };
enum StageRefusal { STAGE_OK, STAGE_NEEDS_GROUP, STAGE_LANE_RANGE };

struct StagePlan {
  int kind;                        // StageKind
  int G, KMAX, NS2, UNI, HM, NM;   // the family's template values (0 where it has none)
  int tpb, max_tpb;                // threads per workgroup, and the kernel's launch bound
  int resident;   // ST_PIPE: `grid` counts the 8 block classes only; the launcher multiplies it by the workgroups of a
                  // class that one XCD holds at once (the occupancy query, at run time)
  long grid;      // workgroups
  size_t lds;     // dynamic LDS bytes
  int xsplit, ntst, bchunk;        // DeomParams values (see there)
  int refusal;                     // StageRefusal; then only msg is set
  const char* name;                // note_path
  char msg[112];
};

inline StagePlan deom_stage_plan(int B, int nmax, int K, int ns, int nmod, int bminor, int horner) {
  StagePlan pl{};
  pl.name = "";
  const size_t ns2 = (size_t)ns * ns;
  const size_t tot = (size_t)B * nmax * ns2;
  // group kernel when ns^2 <= 64 lanes and K <= 8; MFMA tile kernel for 9 <= ns <= 16 (nmod <= 2, K <= 21); the
  // tiled kernels for what the element kernel's LDS tables (ns <= 16, nmod <= 8) do not hold; else the element kernel
  int G = 1;
  while (G < (int)ns2) G *= 2;
  const bool grp = G <= 64 && K <= 8;
  const bool mfma = !grp && !bminor && ns >= 9 && ns <= 16 && nmod <= 2 && K <= 21;
  if (bminor && !grp) {
    pl.refusal = STAGE_NEEDS_GROUP;
    std::snprintf(pl.msg, sizeof pl.msg, "qd_deom_rk4_ado_major: needs ns^2 <= 64 and K <= 8 (group kernel)");
    return pl;
  }
  if (grp && !((size_t)B * nmax * G < (1u << 31))) {
    pl.refusal = STAGE_LANE_RANGE;
    std::snprintf(pl.msg, sizeof pl.msg, "qd_deom_rk4: B nmax = %zu ADO rows exceed the 32-bit lane range",
                  (size_t)B * nmax);
    return pl;
  }
  const size_t nthreads = grp ? (size_t)B * nmax * G : tot;
  // A small hierarchy (one at L = 12, K = 5: 24.8k lanes) as 256-thread blocks would occupy ~100 of the
  // 256 CUs, each CU then issuing the loads of 4 waves; 64-thread blocks spread the same lanes over every CU.
  int tpb = (nthreads + DEOM_TPB - 1) / DEOM_TPB < 1024 ? 64 : DEOM_TPB;
  if (!grp) tpb = DEOM_TPB;
  long grid = (long)((nthreads + tpb - 1) / tpb);
  // XCD classes for the group kernel (p.xsplit, see the kernel): batches of 8k hierarchies are dealt over the
  // 8 block classes
  pl.xsplit = 0;
  if (grp && B >= 8 && B % 8 == 0) {
    pl.xsplit = 8;
    const size_t per = (size_t)(B / 8) * nmax * G;   // lanes per class
    grid = 8 * (long)((per + tpb - 1) / tpb);
  }
  // non-temporal rho / acc from 64 MB of state per buffer (four buffers of 25 MB at 64 hierarchies of the bench
  // hierarchy stay in the 256 MB Infinity Cache: 32.7 vs 34.2 us per stage plain / non-temporal; at 256, 101 MB
  // each: 127 vs 116 us, profiles/r02/deom/nontemporal_state_ab.txt)
  pl.ntst = tot * 16 >= ((size_t)64 << 20);
  const size_t lds = (size_t)(1 + nmod) * ns2 * 16;   // H(t), Q(t) of the group kernel
  // the software-pipelined persistent form (undriven ns = 2 ADO-major batches of >= 64 hierarchies in 8 XCD classes,
  // no hierarchy chunks).  Its buffer loads take 32-bit byte offsets: every table below 2^31 - 2^20 bytes, __umul24
  // factors below 2^24.
  const bool small_tables = (size_t)nmax * B * 64 < ((size_t)1 << 31) - ((size_t)1 << 20) && nmax < (1 << 24) &&
                            (size_t)B * 64 < ((size_t)1 << 24);
  const bool pipe_ok = grp && G == 4 && horner && bminor && pl.xsplit == 8 && B >= 64 && K <= 6 &&
                       tpb == DEOM_TPB && small_tables;
  // hierarchy chunks of 16 in classes of more (ADO-major) for the stage kernels: 256 hierarchies = 8 classes of 32,
  // see the kernel; not for the pipelined form (256 hierarchies: 97.0 us per stage unchunked vs 102.7-103.3 for the
  // chunked stage kernel, profiles/r04/deom/deom_bchunk_pipe_ab.txt)
  pl.bchunk = 0;
  if (grp && bminor && pl.xsplit > 0) {
    const int Bx = B / pl.xsplit;
    pl.bchunk = (!pipe_ok && Bx > 16 && Bx % 16 == 0) ? 16 : 0;
  }
  // wave-uniform ADO (scalar tables): ADO-major, classes (chunks) of a multiple of 64 / G hierarchies, 64-multiple
  // blocks
  const int wb = pl.bchunk > 0 ? pl.bchunk : (pl.xsplit > 0 ? B / pl.xsplit : 0);
  const bool uni = grp && G == 4 && bminor && pl.xsplit > 0 && wb % (64 / G) == 0 && tpb % 64 == 0;
  const bool tiled = !bminor && !grp && !mfma && (ns > DEOM_MAX_NS || nmod > DEOM_MAX_NMOD);

  auto set = [&](StageKind kind, const char* name, long g, int t, size_t l) {
    pl.kind = kind;
    pl.name = name;
    pl.grid = g;
    pl.tpb = t;
    pl.max_tpb = DEOM_TPB;   // every stage kernel is bounded to 256 threads
    pl.lds = l;
  };
  if (tiled) {
    pl.xsplit = 0;
    if (ns >= 17) {   // MFMA tiles: a wave per 16 x 16 tile, 2 x 2 tiles per workgroup
      const int nt = (ns + 15) / 16, nbk = (nt + 1) / 2;
      set(ST_TMFMA, "deom_tmfma", (long)B * nmax * nbk * nbk, 256, 0);
    } else {          // a workgroup per 16 x 16 tile
      const int nt = (ns + DEOM_TT - 1) / DEOM_TT;
      set(ST_TILE, "deom_tile", (long)B * nmax * nt * nt, 256, 0);
    }
  } else if (mfma) {   // a wave per ADO; H(t), Q(t) padded to 16 x 16 and a transpose tile per wave
    set(ST_MFMA16, "deom_mfma16", ((long)B * nmax + 3) / 4, 256, (size_t)(256 * (1 + nmod) + 4 * 16 * 17) * 16);
    pl.NM = nmod == 1 ? 1 : 2;
  } else if (!grp) {
    set(ST_ELEMENT, "deom_element", grid, tpb, 0);
  } else if (pipe_ok && pl.bchunk == 0) {
    // workgroups per class: what one XCD's CUs hold at once (every wave persistent, no tail generation)
    pl.KMAX = K == 5 ? 5 : K <= 4 ? 4 : 6;
    set(ST_PIPE, pl.KMAX == 5 ? "deom_pipe_k5" : pl.KMAX == 4 ? "deom_pipe_k4" : "deom_pipe_k6", 8, DEOM_TPB, lds);
    pl.G = 4;
    pl.resident = 1;
  } else if (G == 4) {
    // ns = 2; registers sized to K (ym/yp/indices scale with KMAX); K = 5 (the bench bath, Pade npsd = 4):
    // 104 instead of 116 VGPRs, same speed (profiles/r02/deom/kmax5_ab.txt); undriven runs take the
    // compile-time Horner instantiations (HM = 1)
    pl.HM = horner ? 1 : 0;
    const bool w5 = !uni && K == 5 && pl.HM && B >= 64;   // deom_stage_grp_w5_kernel, see there
    set(w5 ? ST_GROUP_W5 : ST_GROUP, uni ? "deom_grp4_uniform" : w5 ? "deom_grp4_w5" : "deom_grp4", grid, tpb, lds);
    pl.G = 4;
    pl.KMAX = K <= 4 ? 4 : K == 5 ? 5 : K <= 6 ? 6 : 8;
    pl.NS2 = 1;
    pl.UNI = uni;
  } else {
    set(ST_GROUP, "deom_grp", grid, tpb, lds);
    pl.G = G;
    pl.KMAX = 8;
  }
  return pl;
}

// A stage kernel's compile-time values (0 / false where the family has none).
template <int KIND, int G_ = 0, int KMAX_ = 0, bool NS2_ = false, bool UNI_ = false, int HM_ = 0, int NM_ = 0>
struct StageKernel {
  static constexpr int kind = KIND, G = G_, KMAX = KMAX_, HM = HM_, NM = NM_;
  static constexpr bool NS2 = NS2_, UNI = UNI_;
};

// f(StageKernel<...>{}) for the planned kernel; false when the plan's values are in no list (the caller's internal
// error) or f returns false.  The lists are the stage kernels deom.hip instantiates
// (tests/test_deom_plan_host.py holds the set).
template <typename F>
bool dispatch_stage(const StagePlan& p, F&& f) {
  switch (p.kind) {
    case ST_ELEMENT: return f(StageKernel<ST_ELEMENT>{});
    case ST_TILE: return f(StageKernel<ST_TILE>{});
    case ST_TMFMA: return f(StageKernel<ST_TMFMA>{});
    case ST_MFMA16:
      return dispatch_int<1, 2>(p.NM, [&](auto NM) {
        return f(StageKernel<ST_MFMA16, 0, 0, false, false, 0, decltype(NM)::value>{});
      });
    case ST_PIPE:
      return p.G == 4 && dispatch_int<4, 5, 6>(p.KMAX, [&](auto KM) {
        return f(StageKernel<ST_PIPE, 4, decltype(KM)::value>{});
      });
    case ST_GROUP_W5:
      return p.G == 4 && p.KMAX == 5 && p.NS2 && !p.UNI && p.HM == 1 &&
             f(StageKernel<ST_GROUP_W5, 4, 5, true, false, 1>{});
    case ST_GROUP:
      if (p.G != 4)   // ns = 1, 3 .. 8: the run-time Horner switch, K to 8
        return p.KMAX == 8 && !p.NS2 && !p.UNI && !p.HM && dispatch_int<1, 16, 32, 64>(p.G, [&](auto G) {
          return f(StageKernel<ST_GROUP, decltype(G)::value, 8>{});
        });
      return p.NS2 && dispatch_int<4, 5, 6, 8>(p.KMAX, [&](auto KM) {
        return dispatch_int<0, 1>(p.UNI, [&](auto U) {
          return dispatch_int<0, 1>(p.HM, [&](auto HM) {
            return f(StageKernel<ST_GROUP, 4, decltype(KM)::value, true, decltype(U)::value != 0,
                                 decltype(HM)::value>{});
          });
        });
      });
    default: return false;
  }
}

// ---------------------------------------------------------------- one hierarchy, banded (qd_deom_rk4_banded)
enum BandRefusal { BAND_OK, BAND_NS, BAND_K, BAND_LANES, BAND_LDS };

struct BandPlan {
  int G, KMAX, NS2, FAST;   // deom_band_kernel's template values ...
  int TPB;                  // ... and its launch-bound class: 256, 512 or 1024
  int tpb;                  // threads per workgroup
  size_t lds;               // dynamic LDS bytes
  int refusal;              // BandRefusal; then only msg is set
  const char* name;         // note_path
  char msg[112];
};

// max_own / max_loc: the largest band's owned / owned + halo rows.  G lanes per owned ADO in ONE workgroup per band,
// every band's rows (and a zero row for absent neighbours) in LDS beside H(t), Q(t).  The entry point checks K <= 8
// with its other sizes before it plans; the device-dependent checks (bands <= CUs, the cooperative launch) stay
// there too.
inline BandPlan deom_band_plan(int ns, int K, int nmod, int max_own, int max_loc) {
  BandPlan pl{};
  pl.name = "";
  auto refuse = [&](BandRefusal why) {
    pl.refusal = why;
    return pl;
  };
  if (!(ns >= 2 && ns <= 4)) {
    std::snprintf(pl.msg, sizeof pl.msg, "qd_deom_rk4_banded: ns=%d outside [2, 4]", ns);
    return refuse(BAND_NS);
  }
  if (K > 8) {
    std::snprintf(pl.msg, sizeof pl.msg, "qd_deom_rk4_banded: bad sizes K=%d (K <= 8)", K);
    return refuse(BAND_K);
  }
  const int G = ns == 2 ? 4 : 16;
  const int tpb = (max_own * G + 63) / 64 * 64;
  if (tpb > 1024) {
    std::snprintf(pl.msg, sizeof pl.msg,
                  "qd_deom_rk4_banded: %d owned rows x %d lanes exceed one 1024-thread workgroup", max_own, G);
    return refuse(BAND_LANES);
  }
  const size_t ns2 = (size_t)ns * ns;
  const size_t lds = ((size_t)(1 + nmod) + (size_t)max_loc + 1) * ns2 * 16;   // + the zero row
  if (lds > DEOM_LDS_MAX) {
    std::snprintf(pl.msg, sizeof pl.msg,
                  "qd_deom_rk4_banded: %zu B of band rows exceed the 160 KB LDS (more bands)", lds);
    return refuse(BAND_LDS);
  }
  pl.G = G;
  pl.tpb = tpb;
  pl.TPB = tpb <= 256 ? 256 : tpb <= 512 ? 512 : 1024;
  pl.lds = lds;
  if (G == 4) {
    // FAST: one bath mode and K == KMAX, for the bench bath (K = 5) and its stretch (npsd 5: K = 6)
    pl.FAST = nmod == 1 && (K == 5 || K == 6);
    pl.KMAX = pl.FAST ? K : K <= 5 ? 5 : 8;
    pl.NS2 = 1;
    pl.name = pl.FAST ? "deom_banded_fast" : "deom_banded";
  } else {
    pl.KMAX = 8;
    pl.name = "deom_banded_g16";
  }
  return pl;
}

template <int G_, int KMAX_, bool NS2_, int TPB_, bool FAST_>
struct BandKernel {
  static constexpr int G = G_, KMAX = KMAX_, TPB = TPB_;
  static constexpr bool NS2 = NS2_, FAST = FAST_;
};

// f(BandKernel<...>{}) for the planned kernel, as dispatch_stage: the lists are the deom_band_kernel instantiations.
template <typename F>
bool dispatch_band(const BandPlan& p, F&& f) {
  return dispatch_int<256, 512, 1024>(p.TPB, [&](auto T) {
    constexpr int TPB = decltype(T)::value;
    if (p.G == 16) return p.KMAX == 8 && !p.NS2 && !p.FAST && f(BandKernel<16, 8, false, TPB, false>{});
    if (p.G != 4 || !p.NS2) return false;
    if (p.FAST)
      return dispatch_int<5, 6>(p.KMAX, [&](auto KM) { return f(BandKernel<4, decltype(KM)::value, true, TPB, true>{}); });
    return dispatch_int<5, 8>(p.KMAX, [&](auto KM) { return f(BandKernel<4, decltype(KM)::value, true, TPB, false>{}); });
  });
}

}  // namespace qd
