// fft_plan.hpp — the shape decisions of the any-size FFT engine (spo_gen.hip) in plain C++17, no HIP, so that a host
// build can enumerate them (tools/cpu_emu/fft_plan_c.cpp, tests/test_fft_plan_host.py): the plan of one axis
// (axis_plan), the four-step split of a long line (fourstep_split), the plan of one fft_lines call (fft_lines_plan),
// the tile of one fused LDS pass (pass_plan), the layout of a D-dimensional run (nd_layout) and the Strang / merged
// pass sequence (step_sequence).  spo_gen.hip executes what these return and decides nothing itself.
#pragma once

#include <algorithm>
#include <cstddef>

#ifdef __HIPCC__   // fdiv also runs in the kernels; a host build sees no HIP header
#include <hip/hip_runtime.h>
#define QD_FFT_HD __host__ __device__ __forceinline__
#else
#define QD_FFT_HD inline
#endif

namespace qd {
namespace spog {

constexpr int MAX_ST = 32;
constexpr size_t LDS_MAX = 163840;            // one workgroup may hold all 160 KiB on gfx950
constexpr size_t LDS_SOFT = 65536;            // tile target: two or more workgroups per CU
constexpr int GEN_MAXP = 61;                  // largest prime run as a direct radix stage
constexpr size_t ELEM = 16;                   // bytes of one complex fp64 value
constexpr int MAX_LDS_M = (int)(LDS_MAX / (2 * ELEM));   // 5120

enum Kind { MIXED = 0, BLUESTEIN = 1, DIRECT = 2 };

// Division by a launch-invariant divisor d >= 1 as a multiply-high (Granlund-Montgomery / Hacker's Delight 10-8,
// exact for every 32-bit x): l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1, t = umulhi(x, m),
// x / d = (t + ((x - t) >> 1)) >> (l - 1); d = 1 is x itself.  The element loops of the LDS passes divide their
// flat index by runtime lengths several times per element; a 32-bit udiv is ~25 VALU instructions, this is 5.
struct FDiv {
  unsigned d, m, s;
};
inline FDiv make_fdiv(unsigned d) {
  FDiv r{d, 0u, 0u};
  if (d > 1) {
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    r.m = (unsigned)((((unsigned long long)1 << 32) * ((1ull << l) - d)) / d + 1);
    r.s = l - 1;
  }
  return r;
}
QD_FFT_HD unsigned fdiv(unsigned x, FDiv D) {
  if (D.d == 1) return x;
  const unsigned t = (unsigned)(((unsigned long long)x * D.m) >> 32);
  return (t + ((x - t) >> 1)) >> D.s;
}

enum Flags { F_INV = 1, F_PT1 = 2, F_SNAP = 4, F_PT2 = 8, F_FWD = 16, F_KY = 32, F_KMUL = 64,
             F_XOUT = 128,    // store into another layout: element (o, e, i) of [O][L][I], o = hi nlo + lo, to
                              // out[hi sh + lo sl + e se + i] (2D: [L][O][I])
             F_KROW = 256 };  // KMUL on whole rows (C == I == ns): factor K[o][e] of the [O][L] table

// ---------------------------------------------------------------- one axis
//   MIXED      mixed-radix Stockham autosort in LDS: radix 8, 4, 2, 3, 5 butterflies in closed form, any
//              other prime p <= 61 as a direct p-point DFT stage; natural-order output, fp64 twiddles
//              exp(-2 pi i m / L) from sincospi, L <= 5120 (two LDS lines of L complex values)
//   BLUESTEIN  lengths with a prime factor > 61: chirp-z, X_k = c_k sum_n (x_n c_n) conj(c_{k-n}),
//              c_n = exp(-pi i n^2 / L) (n^2 mod 2L exact in integers), the convolution as an M-point
//              mixed-radix FFT pair in LDS, M = the smallest 2^a 3^b 5^c >= 2L - 1 (M <= 5120)
//   DIRECT     everything longer: O(L^2) DFT straight from HBM / L2, twiddle index (n k) mod L exact
struct AxisPlan {
  int L, M, kind;
  int nst;             // Stockham stages of the M-point transform (DIRECT: 0)
  int R[MAX_ST];       // radix of stage s
  int Ns[MAX_ST];      // product of the radices before stage s
  FDiv dnb[MAX_ST];    // M / R[s]
  FDiv dns[MAX_ST];    // Ns[s]
  FDiv dM;             // M
  size_t slots;        // complex table slots: tw [M]; BLUESTEIN also chirp [L], b [M], bhat [M]
  size_t tw, chirp, b, bhat;   // offsets of the tables inside the slots (BLUESTEIN only: the last three)
  bool refused;        // more than MAX_ST stages: R / Ns hold the first MAX_ST only, no kernel may run the plan
};

inline bool all_factors_small(int n, int maxp) {
  for (int p = 2; (long)p * p <= n; ++p)
    while (n % p == 0) {
      if (p > maxp) return false;
      n /= p;
    }
  return n <= maxp;
}

inline int next_smooth(int n) {  // smallest 2^a 3^b 5^c >= n
  for (int m = n;; ++m) {
    int r = m;
    for (int p : {2, 3, 5})
      while (r % p == 0) r /= p;
    if (r == 1) return m;
  }
}

// Kind of an axis of length L and the length M of its LDS transform.
inline Kind axis_kind(int L, int* M) {
  *M = L;
  if (L <= MAX_LDS_M && all_factors_small(L, GEN_MAXP)) return MIXED;
  const int m = next_smooth(2 * L - 1);
  if (L >= 2 && m <= MAX_LDS_M) {
    *M = m;
    return BLUESTEIN;
  }
  return DIRECT;
}

inline void factor_stages(int M, AxisPlan& f) {
  f.nst = 0;
  int ns = 1, n = M;
  auto push = [&](int r) {
    if (f.nst < MAX_ST) {
      f.R[f.nst] = r;
      f.Ns[f.nst] = ns;
      f.dnb[f.nst] = make_fdiv((unsigned)(M / r));
      f.dns[f.nst] = make_fdiv((unsigned)ns);
    }
    ++f.nst;
    ns *= r;
    n /= r;
  };
  // radix 8 first (one LDS stage and barrier instead of a radix-4 and a radix-2 one: 200 = 8 5 5 in three stages
  // instead of four)
  {
    // 8s as long as no single 2 would be left over unpaired with a 4 (16 = 8 2 would take as many stages as 4 4)
    int twos = 0;
    for (int m = n; m % 2 == 0; m /= 2) ++twos;
    for (int k = 0; k < twos / 3 && twos % 3 != 1; ++k) push(8);
    if (twos % 3 == 1 && twos >= 4) {   // 2^(3j+1): 8^(j-1) 4 4 is as short as 8^j 2 and has no radix-2 stage
      for (int k = 0; k < (twos - 4) / 3; ++k) push(8);
    }
  }
  while (n % 4 == 0) push(4);
  while (n % 2 == 0) push(2);
  while (n % 3 == 0) push(3);
  while (n % 5 == 0) push(5);
  int p = 7;
  while (n > 1) {
    while (n % p == 0) push(p);
    p += 2;
  }
}

inline AxisPlan axis_plan(int L) {
  AxisPlan a{};
  a.L = L;
  a.kind = axis_kind(L, &a.M);
  a.dM = make_fdiv((unsigned)a.M);
  if (a.kind != DIRECT) factor_stages(a.M, a);
  a.refused = a.nst > MAX_ST;
  a.slots = (size_t)a.M;
  if (a.kind == BLUESTEIN) {
    a.chirp = (size_t)a.M;
    a.b = a.chirp + L;
    a.bhat = a.b + a.M;
    a.slots = a.bhat + a.M;
  }
  return a;
}

// ---------------------------------------------------------------- four-step split
// L1 of the split L = L1 L2 of a line no LDS plan takes: the largest divisor <= sqrt(L) (the most balanced split)
// such that both factors are LDS plans; 0: none.  fft_lines allows Bluestein factors, the 1D split-operator run wants
// both factors mixed-radix, so 5121 = 9 x 569 splits in the first and runs the direct DFT in the second.
inline int fourstep_split(int L, bool allow_bluestein) {
  auto ok = [&](int n) {
    int M;
    const Kind k = axis_kind(n, &M);
    return allow_bluestein ? k != DIRECT : k == MIXED;
  };
  int L1 = 0;
  for (int a = 2; (long)a * a <= L; ++a)
    if (L % a == 0 && ok(a) && ok(L / a)) L1 = a;
  return L1;
}

// ---------------------------------------------------------------- one fft_lines call
// Transform along the middle axis of [O][L][I].  An LDS plan of L itself runs one pass; a DIRECT length that splits
// runs the four-step FFT on the [O][L1][L2][I] view (ax[0] over L1, ax[1] over L2, and a twiddle table of L slots
// behind theirs) and leaves X[k1 + L1 k2] at slot L2 k1 + k2; any other the direct DFT through a grid-sized scratch.
struct LinesPlan {
  long O, I;
  int L, kind;       // kind of L itself
  int L1, L2;        // the four-step split, or 0, 0
  int l2;            // what the call reports: L2, or 0 for natural order
  AxisPlan ax[2];    // ax[0]: L, or L1; ax[1]: L2
  size_t slots;      // complex table slots in all
  size_t tw_l;       // four-step: offset of exp(-2 pi i m / L), m < L
  bool scratch;      // O L I more slots behind the tables (direct DFT)
};

inline LinesPlan fft_lines_plan(long O, int L, long I) {
  LinesPlan p{};
  p.O = O;
  p.L = L;
  p.I = I;
  p.ax[0] = axis_plan(L);
  p.kind = p.ax[0].kind;
  p.slots = p.ax[0].slots;
  if (p.kind == DIRECT) p.L1 = fourstep_split(L, true);
  if (p.L1) {
    p.L2 = p.l2 = L / p.L1;
    p.ax[0] = axis_plan(p.L1);
    p.ax[1] = axis_plan(p.L2);
    p.tw_l = p.ax[0].slots + p.ax[1].slots;
    p.slots = p.tw_l + (size_t)L;
  }
  p.scratch = p.kind == DIRECT && !p.L1;
  return p;
}

// ---------------------------------------------------------------- one fused LDS pass
// A workgroup of spo_axis_kernel holds a tile of G outer rows x C consecutive inner columns of the [O][L][I] grid in
// two LDS buffers of M slots per line, and the twiddles behind them where M more slots fit.
struct PassPlan {
  bool fused;         // false: the pass runs unfused (a DIRECT axis, or the whole row does not fit the LDS)
  int C, G, twl;
  size_t lds;         // dynamic LDS bytes
  long gx, gy;        // grid: ceil(O / G), ceil(I / C)
  FDiv dLC, dC, dLns, dns;   // L C, C, L ns, ns
};

// c lines of the axis in LDS at once
inline bool lines_fit(const AxisPlan& ax, long c) {
  return ax.kind != DIRECT && (size_t)c * 2 * ax.M * ELEM <= LDS_MAX;
}
// dynamic LDS bytes of `lines` lines of M slots, *twl = 1 with the twiddles staged behind them
inline size_t tile_lds(int M, long lines, int* twl) {
  size_t lds = (size_t)2 * lines * M * ELEM;
  *twl = lds + (size_t)M * ELEM <= LDS_MAX;
  if (*twl) lds += (size_t)M * ELEM;
  return lds;
}
// rows per tile of a whole-row pass (C == I) over O rows of length L: stack short rows (< 256 elements per
// tile) while >= 256 tiles remain
inline int stack_rows(long O, int L, int c, int M) {
  const size_t line = (size_t)2 * M * ELEM;
  int g = 1;
  while (g < O && (long)g * c * L < 256 && O / (2 * g) >= 256 && (size_t)(2 * g) * c * line <= LDS_SOFT) g *= 2;
  return (int)std::min<long>(g, O);
}

// Tile of a pass with plan ax over [O][ax.L][I], ns states per point; rows: the pass needs whole rows (C == I: point
// operators, snapshot, k_y phase).
inline PassPlan pass_plan(const AxisPlan& ax, long O, long I, int ns, bool rows) {
  PassPlan p{};
  const size_t line = (size_t)2 * ax.M * ELEM;
  int c;
  if (rows) {
    c = (int)I;
  } else {   // 8 consecutive columns (128-B rows) when that still leaves >= 256 tiles, else fewer
    c = (int)std::min<long>(I, 8);
    while (c > 1 && ((size_t)c * line > LDS_SOFT || ((I + c - 1) / c) * O < 256)) c >>= 1;
  }
  if (!lines_fit(ax, c)) return p;
  p.fused = true;
  p.C = c;
  p.G = c == I ? stack_rows(O, ax.L, c, ax.M) : 1;   // whole rows
  p.lds = tile_lds(ax.M, (long)p.G * c, &p.twl);
  p.gx = (O + p.G - 1) / p.G;
  p.gy = (I + c - 1) / c;
  p.dLC = make_fdiv((unsigned)(ax.L * c));
  p.dC = make_fdiv((unsigned)c);
  p.dLns = make_fdiv((unsigned)(ax.L * ns));
  p.dns = make_fdiv((unsigned)ns);
  return p;
}

// ---------------------------------------------------------------- layout of a D-dimensional run
// 2D grids alternate two layouts between the passes when every axis is an LDS plan whose whole row of ns states fits:
// the row pass reads [n0][n1][ns] rows and stores [n1][n0][ns], the kinetic pass reads those x lines contiguously and
// stores [n0][n1][ns] back.  (The same rotation for 3D grids: 60^3 x 2 55.4 -> 54.4 us per step, but 96^3 126.5 ->
// 143.4 and 100^3 140.7 -> 161.7, the scattered 32-B stores at large strides costing more than the strided loads
// removed; profiles/r04/spo/spo_xpose_ab.txt.)
struct NdLayout {
  bool xpose;
  PassPlan row, kin;   // xpose: the row pass over the n0 rows [n1][ns], the kinetic pass over the n1 lines [n0][ns]
};
inline NdLayout nd_layout(const AxisPlan* ax, int D, const int* n, int ns, int nsteps) {
  NdLayout l{};
  l.xpose = nsteps >= 1 && D == 2;
  for (int d = 0; d < D && l.xpose; ++d) l.xpose = lines_fit(ax[d], ns);   // every axis a whole-row LDS pass (C == ns)
  if (l.xpose) {
    l.row = pass_plan(ax[1], n[0], ns, ns, true);
    l.kin = pass_plan(ax[0], n[1], ns, ns, true);
  }
  return l;
}

// ---------------------------------------------------------------- step sequence
// One pass of a run: axis, Flags, which point operator F_PT1 / F_PT2 apply, and the snapshot record of F_SNAP.
enum PointOp { U_NONE = 0, U_HALF = 1, U_FULL = 2 };   // none, exp(-i V dt/2), exp(-i V dt)
struct StepPass {
  int axis, flags, u1, u2;
  int rec;   // F_SNAP: the record the pass stores, else -1
};

// The Strang / merged sequence of qd_spo2_run_ex / qd_spo3_run on a D-dimensional grid (D = 2, 3), handed pass by pass
// to ex(const StepPass&) -> int (nonzero stops the run and is returned).  Strang: both V/2 halves of every step, as
// the reference's return_states=True arithmetic (wpd.py:723-730); merged: V/2, nsteps x [K, V], K, V/2 (wpd.py:
// 736-755).  The state is recorded after every nout-th step when snaps.  F_KY rides on every forward transform of the
// last axis.  The entry points return before planning a Strang run of no steps; so does this.
template <class Ex>
inline int step_sequence(int D, int nsteps, int nout, bool snaps, bool merged, bool ky, Ex&& ex) {
  if (!merged && nsteps == 0) return 0;
  const int last = D - 1;
  const int kyf = ky ? F_KY : 0;
  int rc;
  auto fwd_mid = [&]() {
    for (int d = last - 1; d >= 1; --d)
      if ((rc = ex(StepPass{d, F_FWD, U_NONE, U_NONE, -1}))) return rc;
    return 0;
  };
  auto kinetic = [&]() {   // K on axis 0, then back along the middle axes
    if ((rc = ex(StepPass{0, F_KMUL, U_NONE, U_NONE, -1}))) return rc;
    for (int d = 1; d < last; ++d)
      if ((rc = ex(StepPass{d, F_INV, U_NONE, U_NONE, -1}))) return rc;
    return 0;
  };
  if ((rc = ex(StepPass{last, F_PT1 | F_FWD | kyf, U_HALF, U_NONE, -1}))) return rc;
  if ((rc = fwd_mid())) return rc;
  for (int s = 1; s <= nsteps; ++s) {
    if ((rc = kinetic())) return rc;
    const bool take = snaps && (s % nout == 0);
    int flags = F_INV | F_PT1 | (take ? F_SNAP : 0);
    if (merged) flags |= F_FWD | kyf;
    else if (s < nsteps) flags |= F_PT2 | F_FWD | kyf;
    if ((rc = ex(StepPass{last, flags, merged ? U_FULL : U_HALF, U_HALF, take ? s / nout - 1 : -1}))) return rc;
    if ((flags & F_FWD) && (rc = fwd_mid())) return rc;
  }
  if (merged) {   // merged tail (wpd.py:752-755): K, then V/2
    if ((rc = kinetic())) return rc;
    if ((rc = ex(StepPass{last, F_INV | F_PT1, U_HALF, U_NONE, -1}))) return rc;
  }
  return 0;
}

}  // namespace spog
}  // namespace qd
