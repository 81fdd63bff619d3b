// spo_plan.hpp — the shape decisions of the power-of-two split-operator path (spo.hip) in plain C++17, no HIP, so
// that a host build can enumerate them (tools/cpu_emu/spo_plan_c.cpp, tests/test_spo_plan_host.py).  A plan says
// whether the specialised kernels take the shape (`special`, LDS bounds included; spo_gen.hip runs every other grid)
// and, per pass, the kernel family, its template values and the launch geometry.  dispatch_pass turns a planned pass
// into compile-time values; its lists are the kernels that exist.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdio>

#include "typed_dispatch.hpp"

namespace qd {

constexpr int SPO_MAX_NS = 8;
constexpr size_t SPO_LDS_MAX = 160 * 1024;

// Kernel families.  Row passes run along the contiguous axis (with the point operators), column passes along x (with
// exp_K), mid passes along y of a 3D grid.
enum PassKind {
  ROW_Q16, ROW_64, ROW_FAST, ROW_LDS, ROW_WAVE, MID_64, MID_FAST, MID_LDS, COL_Q16, COL_64, COL_FAST, COL_LDS,
  COL_TILE, SPO_1D, PASS_KINDS
};
constexpr const char* PASS_NAMES[PASS_KINDS] = {"row_q16",  "row64",   "row_fast", "row_lds", "row_wave",
                                                "mid64",    "mid_fast", "mid_lds", "col_q16", "col64",
                                                "col_fast", "col_lds", "col_tile", "lds"};

struct Pass {
  int kind;              // PassKind
  int L, C, NS;          // template values: transform length, lines per workgroup (0: no tile), states (0: run time)
  int ky;                // ROW_Q16: the Jacobi k_y factor is compiled in
  int gx, gy, gz;        // grid
  int block, max_block;  // threads per workgroup, and the kernel's launch bound
  size_t lds;            // dynamic LDS bytes
};
// The name a pass is noted under (note_path): <prefix>_<family>[_c<tile width>], e.g. spo3_mid64_c8.
inline const char* pass_name(const Pass& p, const char* prefix, char* buf, size_t n) {
  if (p.C) std::snprintf(buf, n, "%s_%s_c%d", prefix, PASS_NAMES[p.kind], p.C);
  else std::snprintf(buf, n, "%s_%s", prefix, PASS_NAMES[p.kind]);
  return buf;
}

constexpr bool pow2_in_range(int n) { return n >= 16 && n <= 1024 && (n & (n - 1)) == 0; }
constexpr int round64(int t) { return std::max(64, (t + 63) / 64 * 64); }
// LDS bytes of a pass that stages W transforms of length L in two buffers beside the twiddles
constexpr size_t lds_bytes(int L, int W) { return (size_t)(L + 2 * W * L) * 16; }
inline Pass make_pass(PassKind kind, int L, int C, int NS, int gx, int block, int max_block, size_t lds = 0) {
  return Pass{kind, L, C, NS, 0, gx, 1, 1, block, max_block, lds};
}

// Row pass over `rows` rows of length L.  fast (ns <= 2): the latency-shaped kernels -- 256 points on one wave per
// state, 64 points on 16 lanes per row (not with the Jacobi k_y factor `ky`), else one thread per point; otherwise
// the LDS kernel with ns transforms of L / 4 threads.
inline Pass row_pass(int L, int ns, int rows, bool fast, bool ky) {
  if (fast && L == 256) {
    Pass p = make_pass(ROW_Q16, L, 0, ns, rows, 64 * ns, 64 * ns);
    p.ky = ky;
    return p;
  }
  if (fast && L == 64 && rows % 16 == 0 && !ky) return make_pass(ROW_64, L, 0, ns, rows / 16, 256, 256);
  if (fast) return make_pass(ROW_FAST, L, 0, ns, rows, std::max(64, L), std::max(64, L), lds_bytes(L, ns));
  return make_pass(ROW_LDS, L, 0, 0, rows, round64(ns * (L / 4)), 256, lds_bytes(L, ns));
}

// Column pass over `cols` columns of length L, C per workgroup.  fast: 256 points on one wave per (column, state), 64
// points on 16 lanes per line (tiles of the 3D x pass only: C3), else the latency-shaped kernel; otherwise the LDS
// kernel with C ns transforms of L / 4 threads.
inline Pass col_pass(int L, int ns, int cols, int C, bool fast, bool C3 = false) {
  if (fast && L == 256) {
    Pass p = make_pass(COL_Q16, L, 0, ns, cols, 64, 64);
    p.gy = ns;
    return p;
  }
  if (fast && C3 && L == 64) return make_pass(COL_64, L, C, ns, cols / C, 16 * C * ns, 16 * C * ns);
  const int t = C * ns * (L / 4);
  if (fast) return make_pass(COL_FAST, L, C, ns, cols / C, std::max(64, t), std::max(64, t), lds_bytes(L, C * ns));
  return make_pass(COL_LDS, L, C, 0, cols / C, round64(t), 256, lds_bytes(L, C * ns));
}

struct SpoPlan {
  bool special;
  Pass row[2];   // 2D: [the pass carries the Jacobi k_y factor]; else row[0]
  Pass mid, col;
};

// qd_spo2_run_ex: L in [16, 1024], ns <= 8, one transform set per workgroup, both passes within the LDS
inline SpoPlan spo2_plan(int nx, int ny, int ns, bool jacobi) {
  SpoPlan p{};
  p.special = pow2_in_range(nx) && pow2_in_range(ny) && ns >= 1 && ns <= SPO_MAX_NS && ns * (ny / 4) <= 256 &&
              ns * (nx / 4) <= 256 && lds_bytes(ny, ns) <= SPO_LDS_MAX && lds_bytes(nx, 2 * ns) <= SPO_LDS_MAX;
  if (!p.special) return p;
  // column tiling: C columns per workgroup so that C*ns transforms of nx/4 threads fit 256 threads
  int C = std::max(1, 256 / (ns * (nx / 4)));
  while (C > 1 && ny % C) C >>= 1;
  C = std::min(C, 2);  // keep >= ny/2 workgroups in flight
  const bool fast = ns <= 2 && C == 2;
  p.row[0] = row_pass(ny, ns, nx, fast, false);
  p.row[1] = row_pass(ny, ns, nx, fast, jacobi);
  p.col = col_pass(nx, ns, ny, C, fast);
  return p;
}

// The 256 x 256 batch loop of qd_spo2_run_batch (`special`; else one member at a time through spo2_plan); an observed
// single wavefunction keeps qd_spo2_run_ex's dispatch, as SPO2.run does.  ns = 2: a wave per member, 4 members per
// workgroup sharing the staged point operators (64 wavepackets: 476k wavepacket-steps/s against 428k for 2-member
// groups of the single-row kernel); the column pass in tiles of 8 columns (503k against 477k for 4).
inline SpoPlan spo2_batch_plan(int nx, int ny, int ns, int B, bool jacobi, bool observed) {
  SpoPlan p{};
  p.special = nx == 256 && ny == 256 && ns >= 1 && ns <= 2 && !jacobi && (!observed || B > 1);
  if (!p.special) return p;
  p.row[0] = ns == 1 ? make_pass(ROW_Q16, 256, 0, 1, nx, 64, 64) : make_pass(ROW_WAVE, 256, 4, 2, nx, 256, 256);
  p.row[0].gy = ns == 1 ? B : (B + 3) / 4;
  p.col = ns == 1 ? make_pass(COL_Q16, 256, 0, 1, ny, 64, 64) : make_pass(COL_TILE, 256, 8, 2, ny / 8, 512, 512);
  (ns == 1 ? p.col.gz : p.col.gy) = B;
  return p;
}

constexpr PassKind mid_kind(int L, int C) {
  return L == 64 ? MID_64 : C * L / 4 <= 256 && L <= 64 ? MID_FAST : MID_LDS;
}

// qd_spo3_run: the z pass over nx ny rows of length nz (contiguous, fused V/2), the y pass over tiles of the inner
// index (nz ns), the x pass over ny nz columns.  The x pass takes at least two columns per workgroup, so 2 ns
// transforms of nx / 4 threads must fit its 256 threads.
inline SpoPlan spo3_plan(int nx, int ny, int nz, int ns) {
  SpoPlan p{};
  p.special = pow2_in_range(nx) && pow2_in_range(ny) && pow2_in_range(nz) && nx <= 256 && ny <= 256 && nz <= 256 &&
              ns >= 1 && ns <= SPO_MAX_NS && ns * (nz / 4) <= 256 && 2 * ns * (nx / 4) <= 256 &&
              lds_bytes(nz, ns) <= SPO_LDS_MAX && lds_bytes(nx, 2 * ns) <= SPO_LDS_MAX;
  if (!p.special) return p;
  const int nyz = ny * nz, inner = nz * ns;
  const size_t nk = (size_t)nx * nyz;
  const bool fast = ns <= 2;
  p.row[0] = row_pass(nz, ns, nx * ny, fast, false);
  // Mid pass: C consecutive inner indices (C * 16 B per row read) per block. C is the largest of
  // 16 / 8 / 4 that still gives >= 4 blocks per CU (on its own worth ~1% at 64^3 x 2: 512 -> 1024
  // blocks; C = 4 costs 13% at 128^3; tools/spo3_midc_sweep.sh).
  int midC = 4;
  for (int c : {16, 8}) {
    if (c * ny <= 1024 && inner % c == 0 && (size_t)nx * (inner / c) >= 1024) { midC = c; break; }
  }
  while (midC > 1 && inner % midC) midC >>= 1;  // inner = nz * ns >= 16 keeps midC >= 4
  const PassKind mk = mid_kind(ny, midC);
  const int mt = mk == MID_64 ? 16 * midC : std::max(64, midC * (ny / 4));
  p.mid = make_pass(mk, ny, midC, 0, nx * (inner / midC), mt, mk == MID_LDS ? 256 : mt);
  // x pass: the latency-shaped two-column kernel (colC = 0), or the LDS-staged kernel over colC
  // columns x ns states per block (colC * ns * 16 B contiguous per row).
  // Default: at <= 64^3 x 2 points and midC >= 8 the LDS-staged kernel with the mid pass's row width
  // (colC * ns == midC, 128 B rows at 64^3 x 2: 41.1 -> 33.4 us per step); above that the
  // two-column kernel (128^3 x 2: 142 us either way, 146 us with colC * ns == midC).
  int colC = 0;
  // (nx <= 64: the LDS-staged x kernels are instantiated for 16 / 32 / 64-point columns)
  if (nk * ns <= (size_t)1 << 19 && midC >= 8 && midC % ns == 0 && nx <= 64) {  // 32^3 x 2 (midC = 4): 15.4 vs 16.6 us
    const int c = midC / ns;
    if ((c == 2 || c == 4 || c == 8) && nyz % c == 0 && c * ns * (nx / 4) <= 256) colC = c;
  }
  p.col = col_pass(nx, ns, nyz, colC ? colC : 2, fast, colC != 0);
  return p;
}

// qd_spo1d_run: one workgroup per wavepacket, all steps in LDS
inline bool spo1d_plan(int nx, int B, Pass* p) {
  if (pow2_in_range(nx)) *p = make_pass(SPO_1D, nx, 0, 0, B, std::max(64, nx / 4), 256);
  return pow2_in_range(nx);
}

// ---------------------------------------------------------------- typed dispatch (dispatch_int: typed_dispatch.hpp)
// A 3D column tile has colC ns == midC in {8, 16} lines on nx <= 64, and midC's nx (nz ns / midC) >= 1024 blocks with
// nz <= 256 need nx >= 4 colC.
constexpr bool col_tile_ok(int L, int C, int NS) { return (C * NS == 8 || C * NS == 16) && L <= 64 && L >= 4 * C; }

// f(kind, L, C, NS) with the pass's template values as integral constants.  The lists and the `if constexpr` bounds
// admit exactly the combinations the plans above return (tests/test_spo_plan_host.py holds the set), so these are
// the kernels spo.hip instantiates.
template <typename F>
bool dispatch_pass(const Pass& p, F&& f) {
  using Z = int_c<0>;
  auto ns12 = [&](auto K, auto L, auto C) { return dispatch_int<1, 2>(p.NS, [&](auto NS) { return f(K, L, C, NS); }); };
  switch (p.kind) {
    case ROW_Q16: return ns12(int_c<ROW_Q16>{}, int_c<256>{}, Z{});
    case ROW_64: return ns12(int_c<ROW_64>{}, int_c<64>{}, Z{});
    case ROW_WAVE: return p.C == 4 && p.NS == 2 && f(int_c<ROW_WAVE>{}, int_c<256>{}, int_c<4>{}, int_c<2>{});
    case COL_Q16: return ns12(int_c<COL_Q16>{}, int_c<256>{}, Z{});
    case COL_TILE: return p.C == 8 && p.NS == 2 && f(int_c<COL_TILE>{}, int_c<256>{}, int_c<8>{}, int_c<2>{});
    case ROW_FAST:   // 256 points run ROW_Q16; `special` keeps ns transforms of L / 4 threads within 256
      return dispatch_int<16, 32, 64, 128, 512, 1024>(p.L, [&](auto L) {
        constexpr int l = decltype(L)::value;
        return dispatch_int<1, 2>(p.NS, [&](auto NS) {
          if constexpr (decltype(NS)::value * (l / 4) <= 256) return f(int_c<ROW_FAST>{}, int_c<l>{}, Z{}, NS);
          return false;
        });
      });
    case ROW_LDS:
    case SPO_1D:
      return dispatch_int<16, 32, 64, 128, 256, 512, 1024>(p.L, [&](auto L) {
        return p.kind == ROW_LDS ? f(int_c<ROW_LDS>{}, L, Z{}, Z{}) : f(int_c<SPO_1D>{}, L, Z{}, Z{});
      });
    case MID_64:
    case MID_FAST:
    case MID_LDS:   // the family follows from (L, C); C transforms of L / 4 threads within 256 (spo_mid_kernel's LDS)
      return dispatch_int<16, 32, 64, 128, 256>(p.L, [&](auto L) {
        constexpr int l = decltype(L)::value;
        return dispatch_int<4, 8, 16>(p.C, [&](auto C) {
          constexpr int c = decltype(C)::value, k = mid_kind(l, c);
          if constexpr (c * l <= 1024) return p.kind == k && f(int_c<k>{}, int_c<l>{}, C, Z{});
          return false;
        });
      });
    case COL_64:
    case COL_FAST:   // two columns: C NS transforms of L / 4 threads within 256 (256 points run COL_Q16); or a 3D tile,
                     // on 64 points with the register transform
      return dispatch_int<16, 32, 64, 128, 512>(p.L, [&](auto L) {
        constexpr int l = decltype(L)::value;
        return dispatch_int<2, 4, 8>(p.C, [&](auto C) {
          constexpr int c = decltype(C)::value, k = c != 2 && l == 64 ? COL_64 : COL_FAST;
          return dispatch_int<1, 2>(p.NS, [&](auto NS) {
            if constexpr (c == 2 ? c * decltype(NS)::value * (l / 4) <= 256 : col_tile_ok(l, c, decltype(NS)::value))
              return p.kind == k && f(int_c<k>{}, int_c<l>{}, int_c<c>{}, NS);
            return false;
          });
        });
      });
    case COL_LDS:   // ns >= 3 states when C > 1 (else the pass is fast): C ns transforms of L / 4 threads within 256
      return dispatch_int<16, 32, 64, 128, 256, 512, 1024>(p.L, [&](auto L) {
        constexpr int l = decltype(L)::value;
        return dispatch_int<1, 2, 4>(p.C, [&](auto C) {
          if constexpr (decltype(C)::value == 1 || decltype(C)::value * 3 * (l / 4) <= 256)
            return f(int_c<COL_LDS>{}, int_c<l>{}, C, Z{});
          return false;
        });
      });
    default: return false;
  }
}

}  // namespace qd
