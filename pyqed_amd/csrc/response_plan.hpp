// response_plan.hpp — the shape decisions of the 2DES response launches (response.hip) in plain C++17, no HIP, so that
// a host build can enumerate them (tools/cpu_emu/response_plan_c.cpp, tests/test_response_plan_host.py): the padded
// dimensions (ens_dims), the split-K count (split_count) and block size (split_plan), the member groups of the uniform
// Z build (z_group, z_lds), and per entry point a plan that is either a refusal with the entry point's message or the
// workspace layout and the launches in order: ens_plan (qd_response2d_ensemble*), t2ops_plan
// (qd_response2d_t2_operands*), t2apply_plan (qd_response2d_t2_apply), resolvent_plan (qd_resolvent_grid2d) and
// splitk_plan (cgemm_splitk_slabs).  dispatch_ens_gemm turns a GEMM plan into compile-time values; its list is the
// ens_gemm_kernel instantiations that exist.  response.hip executes what these return and decides nothing itself.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdio>

#include "typed_dispatch.hpp"

namespace qd {

constexpr int ENS_BT = 128;          // padding of the grid sides, and the block of the scan's GEMM
constexpr int ENS_KT = 16;           // complex K per GEMM stage (cgemm_block.hpp's CG_KT)
constexpr int ZMAX = 16;             // eigen indices a thread of the Z / P builds holds in registers
constexpr int UNI_ROWS = 64;         // P rows per block (t2 scan)
constexpr int XU_ROWS = 16;          // materialised uniform X: rows per block (one 16-row group: more, shorter blocks)
constexpr int UNI_MAXC = 1024 / 16;  // coarse-table entries of a uniform t1 grid (n1p <= 1024)
#ifndef ENS_MIN_TILES128
#define ENS_MIN_TILES128 32          // K-tiles per workgroup below which 128-blocks give way to 64-blocks
#endif
constexpr int GRID_YZ_MAX = 65535;   // the largest y or z extent of a grid
constexpr int ENS_TPB = 256;         // threads of every operand build and reduction
constexpr int ENS_GEMM_TPB = 512;    // threads of the GEMMs (CG_WG)
constexpr int FLAT_GRID_MAX = 16384; // blocks of a grid-strided element kernel
constexpr int PAD_GRID = 64;         // blocks of the padding kernels
constexpr int XZ_XROWS = 4096;       // block rows the X half of ens_xz_kernel gets at most

inline int resp_ceil(long a, long b) { return (int)((a + b - 1) / b); }
inline unsigned flat_grid(size_t n) { return (unsigned)std::min<size_t>((n + ENS_TPB - 1) / ENS_TPB, FLAT_GRID_MAX); }

// ---------------------------------------------------------------- padded dimensions
// Grid sides to multiples of ENS_BT, K = M nL to whole K-tiles.
struct EnsDims {
  int n3p, n1p, K, tiles, Kp;
};
inline EnsDims ens_dims(int M, int nL, int n3, int n1) {
  EnsDims d;
  d.n3p = resp_ceil(n3, ENS_BT) * ENS_BT;
  d.n1p = resp_ceil(n1, ENS_BT) * ENS_BT;
  d.K = M * nL;
  d.tiles = resp_ceil(d.K, ENS_KT);
  d.Kp = d.tiles * ENS_KT;
  return d;
}
// what the ensemble entry points admit of M and nL (K below 2^30, M below the 2^26 of the member index)
inline bool ens_sizes_ok(long M, long nL) { return M * nL < (1L << 30) && M < 65536 * 1024; }

// ---------------------------------------------------------------- split-K
// Splits of a GEMM whose `blocks` output blocks run over `tiles` K-tiles: enough to put `target` workgroups on the
// chip, but no fewer than `min_tiles` K-tiles per split.
inline int split_count(int target, int blocks, int tiles, int min_tiles) {
  return std::max(1, std::min(resp_ceil(target, blocks), std::max(1, tiles / min_tiles)));
}
// Square blocks of bt: >= 4 K-tiles per workgroup.  64-blocks: two workgroups per CU (69.6 KB of LDS each), 512 in all
// (8,192-member shard: 0.169-0.170 vs 0.172-0.173 ms per grid at 256; 384 and 768 slower,
// profiles/r05/2des/wg64_splits_ab.txt); 128-blocks hold one per CU.  The fixed-t2 GEMM, the scan's GEMM and the two
// resolvent GEMMs all take this one rule (the last three with bt = 128).
inline int ens_splits(int bt, int blocks, int tiles) { return split_count(bt == 64 ? 512 : 256, blocks, tiles, 4); }
// 64-wide column blocks of a skinny B (a batch of <= 64 vectors, cgemm_splitk_slabs): >= 512 workgroups, >= 8
// K-tiles each
inline int skinny_splits(int blocks, int tiles) { return split_count(512, blocks, tiles, 8); }

// (BT, S) for a split-K GEMM of Mp x Np (multiples of 128) over `tiles` K-tiles: 128-blocks with enough
// splits to cover the 256 CUs once at >= 4 K-tiles per workgroup; 64-blocks when that leaves the chip
// under-filled or gives a workgroup fewer than 32 K-tiles (the S partial slabs to write and reduce then
// cost more than the 64-block's lower operand reuse; measured on the 256 x 256 2DES grid: 64-blocks
// win at K <= 8k, 128-blocks from K = 32k).
struct SplitPlan {
  int bt, S;
};
inline SplitPlan split_plan(int Mp, int Np, int tiles) {
  const int S128 = ens_splits(128, (Mp / 128) * (Np / 128), tiles);
  const bool small = (Mp / 128) * (Np / 128) * S128 < 256 || tiles / S128 < ENS_MIN_TILES128;
  const int bt = small ? 64 : 128;
  return {bt, ens_splits(bt, (Mp / bt) * (Np / bt), tiles)};
}

// ---------------------------------------------------------------- member groups of ens_z_uniform_kernel
// c128 values of one member in the block's LDS: Mt_m (nL x nz), the fine (nz x 16) and coarse (nz x n1p / 16) tables,
// lamz and beta
inline int z_per_member(int nL, int nz, int n1p) { return nL * nz + nz * (16 + n1p / 16) + 2 * nz; }
// members per block: tables of <= 32 KB LDS, at most 32 members and at least 1024 member blocks when M allows
// (M = 4096: 0.128 -> 0.116 ms per 256 x 256 grid; no change at M = 32k, where the LDS cap binds)
inline int z_group(int nL, int nz, int n1p, int M) {
  const int G = std::max(1, std::min(32, 2048 / z_per_member(nL, nz, n1p)));
  return std::max(1, std::min(G, M / 1024));
}
// its dynamic LDS bytes
inline size_t z_lds(int G, int nL, int nz, int n1p) { return (size_t)G * z_per_member(nL, nz, n1p) * 16; }

// ---------------------------------------------------------------- launches
enum RespKernel {
  RK_XTAB,        // ens_xtab_kernel: the coarse and fine tables of a uniform t3 (A operand generated in the GEMM)
  RK_Z_UNIFORM,   // ens_z_uniform_kernel: Z of a uniform t1, G members per block; block rows past ceil(M / G) build X
  RK_X_UNIFORM,   // ens_x_uniform_kernel: materialised uniform X in a launch of its own, blocks along x
  RK_Z_PAD,       // ens_z_pad_kernel: rows K .. Kp - 1 of Z
  RK_XZ,          // ens_xz_kernel: Z of an array t1 in block rows < M, X of an array t3 in the xrows after them
  RK_Z_GENERIC,   // ens_z_generic_kernel: all Kp rows of Z, any nL
  RK_P_UNIFORM,   // ens_p_uniform_kernel
  RK_P_PAD,       // ens_p_pad_kernel
  RK_E,           // ens_e_kernel
  RK_REDUCE,      // ens_reduce_kernel
  RK_REDUCE_TRANS,   // ens_reduce_trans_kernel
  RK_REDUCE_T2,   // ens_reduce_t2_kernel
  RK_PAD_SQUARE,  // pad_square_kernel
  RK_RESOLVENT_OPERAND   // resolvent_operand_kernel
};

// One launch of ENS_TPB threads.  M, xrows, xbx and G are the argument values that differ between a kernel's uses:
// RK_XZ takes M = 0 and xrows = XZ_XROWS when it builds X only; RK_Z_UNIFORM's block rows past the member groups
// build X blocks (xbx column blocks per row group), or none ride along and xbx is 1.
struct RespLaunch {
  int kernel;         // RespKernel
  unsigned gx, gy;
  int M, xrows, xbx, G;
  size_t lds;         // dynamic LDS bytes
  const char* note;   // note_path ahead of the launch, or null
};
inline RespLaunch resp_launch(RespKernel k, long gx, long gy = 1, const char* note = nullptr) {
  return RespLaunch{k, (unsigned)gx, (unsigned)gy, 0, 0, 1, 1, 0, note};
}

// The split-K GEMM ens_gemm_kernel<bt, xtab, depth> on grid (Np / bt) x (Mp / bt) x S.  The 64-block kernel keeps two
// K-tiles of global loads in flight (4,096-member shard: 0.111 ms per grid at 2 vs 0.113 at 1,
// profiles/r02/ensdepth_ab.txt).
struct GemmPlan {
  int bt, xtab, depth, S;
  unsigned gx, gy, gz;
  const char* name;   // note_path
};
inline GemmPlan gemm_plan(SplitPlan pl, int Mp, int Np, bool xtab) {
  // 64-blocks with a generated A operand have no kernel and no name: dispatch_ens_gemm misses such a plan
  return GemmPlan{pl.bt, xtab, pl.bt == 64 ? 2 : 1, pl.S, (unsigned)(Np / pl.bt), (unsigned)(Mp / pl.bt),
                  (unsigned)pl.S, pl.bt == 64 ? (xtab ? "" : "ens_gemm64") : (xtab ? "ens_gemm128_xtab" : "ens_gemm128")};
}

template <int BT_, bool XTAB_, int DEPTH_>
struct EnsGemmKernel {
  static constexpr int BT = BT_, DEPTH = DEPTH_;
  static constexpr bool XTAB = XTAB_;
};
// f(EnsGemmKernel<...>{}) for the planned kernel; false when the plan's values are in no list (the caller's internal
// error) or f returns false.  The list is the ens_gemm_kernel instantiations: <64, false, 2>, <128, true, 1> and
// <128, false, 1> (64-blocks are load-bound in the staging already and never generate their A operand).
template <typename F>
bool dispatch_ens_gemm(const GemmPlan& p, F&& f) {
  if (p.bt == 64) return !p.xtab && p.depth == 2 && f(EnsGemmKernel<64, false, 2>{});
  return p.bt == 128 && p.depth == 1 && dispatch_int<0, 1>(p.xtab, [&](auto X) {
    return f(EnsGemmKernel<128, decltype(X)::value != 0, 1>{});
  });
}

// ---------------------------------------------------------------- fixed-t2 ensemble (ens_run)
constexpr int ENS_MAX_BUILDS = 4;
struct EnsPlan {
  int refused;      // then only msg is set
  EnsDims d;
  int xtab;         // the X part holds the tables: coarse [n3p / 16][Kp] at offX, fine [16][Kp] at offFine
  int nbuild;
  // workspace in c128 values: X (or the tables) | Z | slabs
  size_t nX, nZ, nslabs, offX, offFine, offZ, offSlabs, total;
  RespLaunch build[ENS_MAX_BUILDS];   // the operand builds in order
  GemmPlan gemm;
  RespLaunch reduce;
  char msg[192];
};

// nL: the t3 (X, GEMM K) side; nz: the t1 side (Mt is [M][nL][nz]).  A uniform grid is t0 + j dt, and its operand comes
// from exponential tables; an array grid takes one exponential per element.
inline EnsPlan ens_plan(const char* fn, int M, int nL, int nz, int n3, int n1, bool t3_uniform, bool t1_uniform,
                        bool trans) {
  EnsPlan p{};
  const EnsDims d = p.d = ens_dims(M, nL, n3, n1);
  const SplitPlan sp = split_plan(d.n3p, d.n1p, d.tiles);
  p.nX = (size_t)d.n3p * d.Kp;
  p.nZ = (size_t)d.Kp * d.n1p;
  p.nslabs = (size_t)sp.S * d.n3p * d.n1p;
  p.offX = 0;
  p.offZ = p.nX;
  p.offSlabs = p.nX + p.nZ;
  p.total = p.nX + p.nZ + p.nslabs;
  const long zbx = resp_ceil(d.n1p, 256);
  const bool zfast = nL <= ZMAX && nz <= ZMAX && M <= GRID_YZ_MAX - XZ_XROWS;
  const long xbx = resp_ceil(d.Kp, 256), xblocks = xbx * (d.n3p / XU_ROWS);
  // uniform t3 on 128-blocks: the A operand is generated in the GEMM staging from (n3p/16 + 16) x Kp tables held in
  // the X buffer; 64-blocks are already load-bound in the staging
  p.xtab = t3_uniform && sp.bt == 128;
  p.offFine = (size_t)(d.n3p / 16) * d.Kp;
  auto add = [&](RespLaunch l) -> RespLaunch& { return p.build[p.nbuild++] = l; };
  // X of an array t3 from the X half of the combined kernel alone
  auto x_only = [&](const char* note) {
    RespLaunch& l = add(resp_launch(RK_XZ, zbx, XZ_XROWS, note));
    l.M = 0;
    l.xrows = XZ_XROWS;
  };
  auto x_uniform_own = [&](const char* note) { add(resp_launch(RK_X_UNIFORM, xblocks, 1, note)).xbx = (int)xbx; };
  auto z_pad = [&] {
    if (d.Kp > d.K) add(resp_launch(RK_Z_PAD, PAD_GRID));
  };
  if (p.xtab) add(resp_launch(RK_XTAB, xbx));
  const int G = z_group(nL, nz, d.n1p, M);
  const int nMB = resp_ceil(M, G);
  const bool xin = t3_uniform && !p.xtab;  // uniform t3, X materialised
  if (t1_uniform && nL <= ZMAX && nz <= ZMAX && d.n1p <= 16 * UNI_MAXC && nMB <= GRID_YZ_MAX) {
    // Z (uniform t1), G members per block; a materialised uniform X in the same launch while the grid's y extent
    // holds both, else in a launch of its own
    const bool xsame = xin && (long)nMB + xblocks <= GRID_YZ_MAX;
    RespLaunch& z = add(resp_launch(RK_Z_UNIFORM, zbx, nMB + (xsame ? xblocks : 0), "ens_z_uniform"));
    z.M = M;
    z.G = G;
    z.xbx = (int)xbx;
    z.lds = z_lds(G, nL, nz, d.n1p);
    if (xin && !xsame) x_uniform_own("ens_x_uniform_own");
    z_pad();
    if (!t3_uniform) x_only(nullptr);
  } else {
    if (t1_uniform) {
      p.refused = 1;
      std::snprintf(p.msg, sizeof p.msg,
                    "%s: uniform t1 needs nL <= %d, n1 <= %d and at most 65535 member groups (M = %d makes %d)", fn,
                    ZMAX, 16 * UNI_MAXC, M, nMB);
      return p;
    }
    if (xin) x_uniform_own(nullptr);  // uniform t3 with an array t1: X blocks only
    if (zfast) {
      // X (when from an array) gets as many block rows as Z has (capped): one launch, both writes
      const int xrows = !t3_uniform ? std::max(1, std::min(M, XZ_XROWS)) : 0;
      RespLaunch& l = add(resp_launch(RK_XZ, zbx, M + xrows, "ens_z_array"));
      l.M = M;
      l.xrows = xrows;
      z_pad();
    } else {
      if (!t3_uniform) x_only("ens_z_generic");
      add(resp_launch(RK_Z_GENERIC, flat_grid(p.nZ), 1, t3_uniform ? "ens_z_generic" : nullptr));
    }
  }
  p.gemm = gemm_plan(sp, d.n3p, d.n1p, p.xtab);
  p.reduce = trans ? resp_launch(RK_REDUCE_TRANS, resp_ceil(n1, 16), resp_ceil(n3, 16))
                   : resp_launch(RK_REDUCE, flat_grid((size_t)n3 * n1));
  return p;
}

// ---------------------------------------------------------------- t2 scan: P and Q (qd_response2d_t2_operands_rect)
struct T2OpsPlan {
  int refused;
  EnsDims d;          // K = M nr
  int nbuild;
  RespLaunch build[4];   // P build, P pad, Q build (the uniform Z build with Mt := C, Z rows only), Q pad
  char msg[192];
};
inline T2OpsPlan t2ops_plan(const char* fn, int M, int np, int nr, int nq, int n3, int n1) {
  T2OpsPlan p{};
  p.refused = 1;
  if (!(np <= ZMAX && nr <= ZMAX && nq <= ZMAX && n1 <= 16 * UNI_MAXC)) {
    std::snprintf(p.msg, sizeof p.msg, "%s: np=%d nr=%d nq=%d (<= %d), n1=%d (<= %d)", fn, np, nr, nq, ZMAX, n1,
                  16 * UNI_MAXC);
    return p;
  }
  auto too_large = [&] {
    std::snprintf(p.msg, sizeof p.msg, "%s: M=%d too large", fn, M);
    return p;
  };
  if (!((long)M * nr < (1L << 30))) return too_large();
  const EnsDims d = ens_dims(M, nr, n3, n1);
  const int G = z_group(nr, nq, d.n1p, M);
  // the Z-build grid's y extent is the number of member groups
  if (!(resp_ceil(M, G) <= GRID_YZ_MAX)) return too_large();
  p.refused = 0;
  p.d = d;
  const int MB = 256 / std::max(np, nr);   // members per block of the P build
  p.build[p.nbuild++] = resp_launch(RK_P_UNIFORM, resp_ceil(M, MB), d.n3p / UNI_ROWS);
  if (d.Kp > d.K) p.build[p.nbuild++] = resp_launch(RK_P_PAD, PAD_GRID);
  RespLaunch& z = p.build[p.nbuild++] = resp_launch(RK_Z_UNIFORM, resp_ceil(d.n1p, 256), resp_ceil(M, G));
  z.M = M;
  z.G = G;
  z.lds = z_lds(G, nr, nq, d.n1p);
  if (d.Kp > d.K) p.build[p.nbuild++] = resp_launch(RK_Z_PAD, PAD_GRID);
  return p;
}

// ---------------------------------------------------------------- t2 scan: the waiting times (qd_response2d_t2_apply)
// ens_t2_gemm_kernel on grid (n2 n1p / ENS_BT) x (n3p / ENS_BT) x S: column block bn is waiting time bn ENS_BT / n1p.
struct T2ApplyPlan {
  int refused;
  EnsDims d;
  int S;
  unsigned gx, gy, gz;   // the GEMM's grid
  long ldz;              // n2 n1p, the slabs' leading dimension
  size_t nE, nslabs, offE, offSlabs, total;   // workspace in c128 values: E [n2][Kp] | slabs
  RespLaunch e, reduce;
  char msg[96];
};
inline T2ApplyPlan t2apply_plan(const char* fn, int M, int nL, int n3, int n1, int n2) {
  T2ApplyPlan p{};
  const EnsDims d = p.d = ens_dims(M, nL, n3, n1);
  p.ldz = (long)n2 * d.n1p;
  if (!(p.ldz / ENS_BT <= GRID_YZ_MAX)) {
    p.refused = 1;
    std::snprintf(p.msg, sizeof p.msg, "%s: n2*n1 too large", fn);
    return p;
  }
  const int blocks2d = (int)((d.n3p / ENS_BT) * (p.ldz / ENS_BT));
  p.S = ens_splits(ENS_BT, blocks2d, d.tiles);
  p.gx = (unsigned)(p.ldz / ENS_BT);
  p.gy = (unsigned)(d.n3p / ENS_BT);
  p.gz = (unsigned)p.S;
  p.nE = (size_t)n2 * d.Kp;
  p.nslabs = (size_t)p.S * d.n3p * p.ldz;
  p.offE = 0;
  p.offSlabs = p.nE;
  p.total = p.nE + p.nslabs;
  p.e = resp_launch(RK_E, flat_grid(p.nE));
  p.reduce = resp_launch(RK_REDUCE_T2, flat_grid((size_t)n2 * n3 * n1));
  return p;
}

// ---------------------------------------------------------------- resolvent grid (qd_resolvent_grid2d)
// W = M Z (np x np x nyp), then out = X W (nxp x np x nyp), both on 128-blocks; the slabs serve both.
struct ResolventPlan {
  int np, nxp, nyp;   // n as a row / column block dimension and as K (a multiple of 16 too), and the padded grid
  // workspace in c128 values: M padded | Z | W | X | slabs
  size_t nM, nZ, nW, nX, nslabs, offM, offZ, offW, offX, offSlabs, total;
  RespLaunch pad, zop, xop;
  GemmPlan gemm1, gemm2;
  RespLaunch reduce1, reduce2;
};
inline ResolventPlan resolvent_plan(int n, int nx, int ny) {
  ResolventPlan p{};
  const int BT = ENS_BT;
  p.np = resp_ceil(n, BT) * BT;
  p.nxp = resp_ceil(nx, BT) * BT;
  p.nyp = resp_ceil(ny, BT) * BT;
  const int tiles = p.np / ENS_KT;
  const int S1 = ens_splits(BT, (p.np / BT) * (p.nyp / BT), tiles), S2 = ens_splits(BT, (p.nxp / BT) * (p.nyp / BT), tiles);
  p.nM = (size_t)p.np * p.np;
  p.nZ = p.nW = (size_t)p.np * p.nyp;
  p.nX = (size_t)p.nxp * p.np;
  p.nslabs = std::max((size_t)S1 * p.np * p.nyp, (size_t)S2 * p.nxp * p.nyp);
  p.offM = 0;
  p.offZ = p.nM;
  p.offW = p.offZ + p.nZ;
  p.offX = p.offW + p.nW;
  p.offSlabs = p.offX + p.nX;
  p.total = p.offSlabs + p.nslabs;
  p.pad = resp_launch(RK_PAD_SQUARE, flat_grid(p.nM));
  p.zop = resp_launch(RK_RESOLVENT_OPERAND, flat_grid(p.nZ));
  p.xop = resp_launch(RK_RESOLVENT_OPERAND, flat_grid(p.nX));
  p.gemm1 = gemm_plan(SplitPlan{BT, S1}, p.np, p.nyp, false);
  p.gemm2 = gemm_plan(SplitPlan{BT, S2}, p.nxp, p.nyp, false);
  p.reduce1 = resp_launch(RK_REDUCE, flat_grid((size_t)p.np * p.nyp));   // W keeps its padding
  p.reduce2 = resp_launch(RK_REDUCE, flat_grid((size_t)nx * ny));
  return p;
}

// ---------------------------------------------------------------- cgemm_splitk_slabs
struct SplitKPlan {
  int refused;
  GemmPlan gemm;
  char msg[48];
};
inline SplitKPlan splitk_plan(int Mp, int Kp, int Np, int max_S) {
  SplitKPlan p{};
  if (!(Mp % 128 == 0 && Np % 64 == 0 && Kp % ENS_KT == 0)) {
    p.refused = 1;
    std::snprintf(p.msg, sizeof p.msg, "cgemm_splitk_slabs: bad padding");
    return p;
  }
  const int tiles = Kp / ENS_KT;
  SplitPlan pl = Np % 128 == 0 ? split_plan(Mp, Np, tiles) : SplitPlan{64, skinny_splits((Mp / 64) * (Np / 64), tiles)};
  pl.S = std::min(pl.S, max_S);
  p.gemm = gemm_plan(pl, Mp, Np, false);
  return p;
}

}  // namespace qd
