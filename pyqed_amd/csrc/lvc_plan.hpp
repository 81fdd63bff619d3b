// lvc_plan.hpp — the shape decisions of the linear-vibronic-coupling entry points (lvc.hip: qd_lvc_apply, qd_lvc_rk4,
// qd_lvc_observe, qd_lvc_driven_rk4 in the second part: LvcDrivePlan, and qd_lvc_pair_observe / qd_lvc_pair_rk4 in the
// third: LvcPairPlan) in plain C++17, no HIP, so that a host build can enumerate them (tools/cpu_emu/lvc_plan_c.cpp,
// lvc_drive_plan_c.cpp, lvc_pair_plan_c.cpp, tests/test_lvc_plan_host.py, test_lvc_drive_plan_host.py,
// test_lvc_pair_plan_host.py): what a call admits and every refusal with its message, the path (resident or staged),
// the tile, the grids, the LDS bytes and layout of the resident kernel, the scratch layout, and the layout of the
// observable partials.  lvc.hip executes what lvc_plan returns and decides nothing itself; lvc_kernels.hpp reads the
// same constants.
//
// State psi[a][n_1]..[n_M], row-major, electronic index slowest: element (a, n) at a * nvib + n, with n the flat
// vibrational index (last mode fastest, stride[j] = prod_{k > j} dims[k]).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdio>

#include "typed_dispatch.hpp"

namespace qd {

constexpr int LVC_MAX_NEL = 8;              // electronic states a thread holds in registers
constexpr int LVC_MAX_MODES = 6;
constexpr int LVC_TILE = 256;               // vibrational points per workgroup of the staged, apply and partial kernels
constexpr int LVC_RES_TPB = 512;            // threads of the resident kernel: two groups of LVC_TILE
// Resident up to the measured crossover, not wherever the LDS would fit (D = 4096): a resident step costs one CU's
// time, linear in D and growing with M, a staged step four launches, 14-28 us flat below D = 5000.  nel = 3, us per
// step resident / staged (tools/bench_lvc.py, profiles/lvc/): M = 1: 7.3 / 14.5 at D = 2049, 14.3 / 14.8 at 4095;
// M = 2: 11.4 / 16.8 at 2028, 15.6 / 16.1 at 3072, 23.3 / 17.5 at 3996; M = 3: 16.0 / 19.7 at 2187, 22.2 / 18.7 at
// 3000; M = 4: 20.3 / 22.4 at 1875, 42.7 / 22.1 at 3888; M = 6: 29.1 / 27.6 at 2187.  The smallest crossover is
// M = 6's, just under 2187.
constexpr long LVC_RESIDENT_MAX_D = 2048;
constexpr int LVC_OBS_MAX_GRID = 1024;      // partial rows per (member, observable row) at most
constexpr int LVC_OBS_NV = 2 * LVC_MAX_NEL + 1;   // doubles of one partial row: nel complex sums, then the nbar part
constexpr int LVC_GRID_YZ_MAX = 65535;      // the largest y or z extent of a grid
constexpr size_t LVC_LDS_MAX = 80 * 1024;   // what the resident kernel may ask for, all dynamic (a CU has 160 KiB)
constexpr int LVC_FLAT_GRID_MAX = 4096;     // blocks of the grid-strided snapshot copy

enum LvcPath { LVC_AUTO = 0, LVC_STAGED = 1, LVC_RESIDENT = 2 };

// The model as the kernels take it (a kernel argument by value: nothing of it lives in device memory).
struct LvcDev {
  int nel, M, nvib, D;
  int dims[LVC_MAX_MODES];
  int stride[LVC_MAX_MODES];
  double omega[LVC_MAX_MODES];
};

struct LvcLaunch {
  unsigned gx, gy, gz;
  int tpb;
  size_t lds;   // dynamic LDS bytes
};

struct LvcPlan {
  int refused;   // then only msg is set
  int path;      // LVC_STAGED or LVC_RESIDENT (qd_lvc_rk4 only)
  LvcDev dev;    // omega left zero: the caller's values go in at call time
  int nobs;      // complex values of one observable record: nel^2 (1 + M) + M
  int rows;      // observable rows (r, a): r = 0 rho, r = j + 1 X[j]; (1 + M) nel of them
  int G;         // partial rows per (member, observable row): workgroup g sums the tiles g, g + G, ...
  int kp;        // vibrational points a thread of the resident kernel owns at most
  LvcLaunch stage;      // one Horner stage, or H psi: grid (tiles, B)
  LvcLaunch resident;   // the whole call: grid (B)
  LvcLaunch obs_part;   // grid (G, rows, B)
  LvcLaunch obs_final;  // grid (B)
  LvcLaunch snap;       // grid-strided copy of B states
  // resident LDS in bytes from the 16-byte aligned base: two stage vectors | Hel and W | wave partials | tile partials |
  // the nbar parts of the rows
  size_t lds_vec1, lds_tab, lds_wave, lds_tile, lds_nbar;
  // scratch in bytes: two stage vectors of B states | partial rows [B][rows][G][LVC_OBS_NV] doubles
  size_t ws_x0, ws_x1, ws_part, ws_part_bytes, ws_total;   // qd_lvc_observe takes ws_part_bytes alone
  char msg[160];
};

inline long lvc_ceil(long a, long b) { return (a + b - 1) / b; }
inline size_t lvc_align16(size_t n) { return (n + 15) & ~(size_t)15; }

// What the three entry points admit of a model, and the launches of a call on B states.  `fn` names the entry point in
// the messages.  path_req, nsteps, save_every and want_obs matter to qd_lvc_rk4 only (the others pass LVC_AUTO, 0, 0 and
// false; staged launches are what they execute).
inline LvcPlan lvc_plan(const char* fn, long B, int nel, int M, const int* dims, int path_req = LVC_AUTO,
                        int nsteps = 0, int save_every = 0, bool want_obs = false) {
  LvcPlan p{};
  p.refused = 1;
  auto refuse = [&](auto... a) {
    std::snprintf(p.msg, sizeof p.msg, a...);
    return p;
  };
  if (!(nel >= 1 && nel <= LVC_MAX_NEL)) return refuse("%s: nel=%d outside [1, %d]", fn, nel, LVC_MAX_NEL);
  if (!(M >= 1 && M <= LVC_MAX_MODES)) return refuse("%s: M=%d outside [1, %d]", fn, M, LVC_MAX_MODES);
  if (!dims) return refuse("%s: null dims", fn);
  long D = nel;
  for (int j = 0; j < M; ++j) {
    if (!(dims[j] >= 1)) return refuse("%s: dims[%d]=%d must be at least 1", fn, j, dims[j]);
    if (D > ((1L << 31) - 1) / dims[j]) return refuse("%s: D = nel * prod(dims) must stay below 2^31", fn);
    D *= dims[j];
  }
  if (!(B >= 1 && B <= LVC_GRID_YZ_MAX)) return refuse("%s: B=%ld outside [1, %d]", fn, B, LVC_GRID_YZ_MAX);
  if (!(path_req >= LVC_AUTO && path_req <= LVC_RESIDENT)) return refuse("%s: path=%d outside [0, 2]", fn, path_req);
  if (!(nsteps >= 0 && save_every >= 0))
    return refuse("%s: nsteps=%d and save_every=%d must not be negative", fn, nsteps, save_every);
  if (want_obs && !(save_every > 0 || nsteps == 0)) return refuse("%s: observables need save_every > 0", fn);
  const bool fits = D <= LVC_RESIDENT_MAX_D;
  if (path_req == LVC_RESIDENT && !fits)
    return refuse("%s: the resident path needs D <= %ld (D = %ld)", fn, LVC_RESIDENT_MAX_D, D);
  p.refused = 0;
  p.path = path_req == LVC_AUTO ? (fits ? LVC_RESIDENT : LVC_STAGED) : path_req;

  LvcDev& d = p.dev;
  d.nel = nel;
  d.M = M;
  d.D = (int)D;
  d.nvib = (int)(D / nel);
  for (int j = M - 1, s = 1; j >= 0; --j) {
    d.dims[j] = dims[j];
    d.stride[j] = s;
    s *= dims[j];
  }
  for (int j = M; j < LVC_MAX_MODES; ++j) d.dims[j] = d.stride[j] = 1;
  p.nobs = nel * nel * (1 + M) + M;
  p.rows = (1 + M) * nel;
  const long tiles = lvc_ceil(d.nvib, LVC_TILE);
  p.G = (int)std::min<long>(tiles, LVC_OBS_MAX_GRID);
  p.kp = (int)lvc_ceil(lvc_ceil(LVC_RESIDENT_MAX_D, nel), LVC_RES_TPB);

  p.stage = LvcLaunch{(unsigned)tiles, (unsigned)B, 1, LVC_TILE, (size_t)(1 + M) * nel * nel * 16};
  p.obs_part = LvcLaunch{(unsigned)p.G, (unsigned)p.rows, (unsigned)B, LVC_TILE, 0};
  p.obs_final = LvcLaunch{(unsigned)B, 1, 1, LVC_TILE, 0};
  p.snap = LvcLaunch{(unsigned)std::min<long>(lvc_ceil((long)B * D, LVC_TILE), LVC_FLAT_GRID_MAX), 1, 1, LVC_TILE, 0};

  if (fits) {
    p.lds_vec1 = (size_t)D * 16;
    p.lds_tab = 2 * p.lds_vec1;
    p.lds_wave = p.lds_tab + (size_t)(1 + M) * nel * nel * 16;
    p.lds_tile = p.lds_wave + lvc_align16((size_t)(LVC_RES_TPB / 64) * LVC_OBS_NV * 8);
    p.lds_nbar = p.lds_tile + lvc_align16((size_t)lvc_ceil(LVC_RESIDENT_MAX_D, LVC_TILE) * LVC_OBS_NV * 8);
    p.resident = LvcLaunch{(unsigned)B, 1, 1, LVC_RES_TPB, p.lds_nbar + lvc_align16((size_t)M * nel * 8)};
  }

  p.ws_x0 = 0;
  p.ws_x1 = (size_t)B * D * 16;
  p.ws_part = 2 * p.ws_x1;
  p.ws_part_bytes = lvc_align16((size_t)B * p.rows * p.G * LVC_OBS_NV * 8);
  p.ws_total = p.ws_part + p.ws_part_bytes;
  return p;
}

// ---------------------------------------------------------------- laser-driven runs (qd_lvc_driven_rk4)
// H(t) = H0 - sum_d f_d(t) mu_d with mu_d = A_d (x) 1 (drive_mode -1) or A_d (x) x_j (drive_mode j) is an LVC
// Hamiltonian with the tables Hel - sum f_d A_d and W[j] - sum f_d A_d: the kernels rebuild their tables from one row
// of fvals [nf][nd] and run the same stencil.  sample 0 (hold): step s takes row s / hold, the generator is constant
// within a step and the step is the Horner form of qd_lvc_rk4.  sample 1 (stage): classical RK4, row h holds
// f(t0 + h dt / 2), the stages of step s take the rows 2s, 2s + 1, 2s + 1, 2s + 2.
constexpr int LVC_MAX_DRIVES = 8;
// The driven resident kernel is sized for D <= 2048 (registers: LVC_DRIVE_RESIDENT_MAX_D / NEL / LVC_RES_TPB points per
// thread; LDS below), and up to there it wins in one to five modes.  nel = 3, one electronic drive, us per step
// resident / staged in hold mode (tools/bench_lvc.py --driven --scan, profiles/lvc/crossover_scan_driven*.jsonl):
// M = 1: 7.6 / 14.8 at D = 2046; M = 2: 11.8 / 17.2 at 2028; M = 3: 16.4 / 19.2 at 1944; M = 4: 20.6 / 22.9 at 1875;
// M = 5: 18.0 / 23.9 at 1536, then a tie within 4 % (25.0 / 25.5 at 1620, 25.1 / 24.4 at 1944; stage mode 25.4 / 27.0).
// In six modes the step from one to two points per thread (nvib > 512) costs more than the staged launches:
// 21.0 / 26.5 at 1536, 29.3 / 28.4 at 1584, 29.0 / 27.6 at 1728, 29.3 / 26.9 at 1944, so the limit there is 1536.
constexpr long LVC_DRIVE_RESIDENT_MAX_D = 2048;
constexpr long LVC_DRIVE_RESIDENT_MAX_D_M6 = 1536;
constexpr long lvc_drive_resident_limit(int M) {
  return M >= 6 ? LVC_DRIVE_RESIDENT_MAX_D_M6 : LVC_DRIVE_RESIDENT_MAX_D;
}
// What the driven resident kernel may ask for: two state vectors of 32 KiB at the limit, the base tables, the effective
// tables and the drive matrices (7 + 7 + 8 KiB at nel = 8, M = 6), the partials.  One workgroup per CU either way.
constexpr size_t LVC_DRIVE_LDS_MAX = 96 * 1024;

enum LvcSample { LVC_HOLD = 0, LVC_STAGE = 1 };

// The drives as the kernels take them (a kernel argument by value, as LvcDev)
struct LvcDrive {
  int nd;
  int mode[LVC_MAX_DRIVES];   // -1: the table Hel, j: the table W[j]
};

struct LvcDrivePlan {
  int refused;   // then only msg is set
  LvcPlan base;  // lvc_plan() of the same shape with the driven limit's path: dev, the stage, observable and snapshot
                 // launches, and the scratch of the two stage vectors and the partials
  LvcDrive drive;
  int sample, hold;
  int rows_needed;      // rows of fvals the call reads: ceil(nsteps / hold), or 2 nsteps + 1; 0 when nd = 0
  LvcLaunch resident;   // the driven resident kernel: grid (B)
  // its LDS in bytes from the 16-byte aligned base: two stage vectors | base Hel and W | effective Hel and W |
  // drive matrices | wave partials | tile partials | the nbar parts of the rows
  size_t lds_vec1, lds_tab, lds_eff, lds_drv, lds_wave, lds_tile, lds_nbar;
  // scratch in bytes: base.ws_total, then in stage mode the accumulator of B states
  size_t ws_acc, ws_total;
  char msg[200];
};

// The row of fvals that stage `stage` of step `s` reads
inline long lvc_drive_row(int sample, int hold, long s, int stage) {
  return sample == LVC_STAGE ? 2 * s + (stage + 1) / 2 : s / hold;
}

// What qd_lvc_driven_rk4 admits beyond lvc_plan(), and what it launches.  nf is the number of rows fvals holds.
inline LvcDrivePlan lvc_drive_plan(const char* fn, long B, int nel, int M, const int* dims, int nd,
                                   const int* drive_mode, int sample, int hold, long nf, int path_req, int nsteps,
                                   int save_every, bool want_obs) {
  LvcDrivePlan p{};
  p.refused = 1;
  auto refuse = [&](auto... a) {
    std::snprintf(p.msg, sizeof p.msg, a...);
    return p;
  };
  // the shape, with the path left open: the driven limit decides it below
  p.base = lvc_plan(fn, B, nel, M, dims, path_req == LVC_RESIDENT ? LVC_AUTO : path_req, nsteps, save_every, want_obs);
  if (p.base.refused) return refuse("%s", p.base.msg);
  if (!(nd >= 0 && nd <= LVC_MAX_DRIVES)) return refuse("%s: nd=%d outside [0, %d]", fn, nd, LVC_MAX_DRIVES);
  if (nd > 0 && !drive_mode) return refuse("%s: null drive_mode", fn);
  for (int d = 0; d < nd; ++d)
    if (!(drive_mode[d] >= -1 && drive_mode[d] < M))
      return refuse("%s: drive_mode[%d]=%d outside [-1, %d)", fn, d, drive_mode[d], M);
  if (!(sample == LVC_HOLD || sample == LVC_STAGE)) return refuse("%s: sample=%d outside {0, 1}", fn, sample);
  if (sample == LVC_HOLD && !(hold >= 1)) return refuse("%s: hold=%d must be at least 1", fn, hold);
  const long need = nd == 0 || nsteps == 0 ? 0 : sample == LVC_STAGE ? 2L * nsteps + 1 : lvc_ceil(nsteps, hold);
  if (nf < need)
    return refuse("%s: fvals holds %ld rows, %ld are needed (%s)", fn, nf, need,
                  sample == LVC_STAGE ? "2 nsteps + 1" : "ceil(nsteps / hold)");
  const long D = p.base.dev.D;
  const long limit = lvc_drive_resident_limit(M);
  const bool fits = D <= limit;
  if (path_req == LVC_RESIDENT && !fits)
    return refuse("%s: the resident path needs D <= %ld with %d modes (D = %ld)", fn, limit, M, D);
  p.refused = 0;
  p.base.path = path_req == LVC_AUTO ? (fits ? LVC_RESIDENT : LVC_STAGED) : path_req;
  p.drive.nd = nd;
  for (int d = 0; d < LVC_MAX_DRIVES; ++d) p.drive.mode[d] = d < nd ? drive_mode[d] : -1;
  p.sample = sample;
  p.hold = sample == LVC_HOLD ? hold : 1;
  p.rows_needed = (int)need;

  if (fits) {
    const size_t tab = (size_t)(1 + M) * nel * nel * 16;
    p.lds_vec1 = (size_t)D * 16;
    p.lds_tab = 2 * p.lds_vec1;
    p.lds_eff = p.lds_tab + tab;
    p.lds_drv = p.lds_eff + tab;
    p.lds_wave = p.lds_drv + (size_t)nd * nel * nel * 16;
    p.lds_tile = p.lds_wave + lvc_align16((size_t)(LVC_RES_TPB / 64) * LVC_OBS_NV * 8);
    p.lds_nbar = p.lds_tile + lvc_align16((size_t)lvc_ceil(LVC_DRIVE_RESIDENT_MAX_D, LVC_TILE) * LVC_OBS_NV * 8);
    p.resident = LvcLaunch{(unsigned)B, 1, 1, LVC_RES_TPB, p.lds_nbar + lvc_align16((size_t)M * nel * 8)};
  }
  p.ws_acc = p.base.ws_total;
  p.ws_total = p.ws_acc + (sample == LVC_STAGE ? (size_t)B * D * 16 : 0);
  return p;
}

// ---------------------------------------------------------------- pair records (qd_lvc_pair_observe, qd_lvc_pair_rk4)
// P pairs (ket, bra) of one model, psi [P][2][D]: the 2P states are the batch of the stage kernel, and block r of a
// pair's record is R_r[a][b] = sum_n L_r[a, n] conj(bra[b, n]) with L_0 = ket, L_{j+1} = x_j ket.  A call names the
// blocks it wants (blocks [nblk], entries in [0, M]); every block is summed on its own, in the order of the
// observable record's row (r, a), so a subset of blocks has the bits of the all-block call.
constexpr int LVC_PAIR_MAX = 32767;       // pairs of one call: 2 P states stay within LVC_GRID_YZ_MAX
constexpr int LVC_PAIR_REG_NEL = 4;       // up to here a thread accumulates all nel^2 sums of a block in one pass
constexpr int LVC_PAIR_NV_MAX = 2 * LVC_PAIR_REG_NEL * LVC_PAIR_REG_NEL;   // doubles of one partial row at most
// The pair resident kernel holds four stage vectors (ket A/B, bra A/B) where the single-state one holds two, so it
// starts at half that kernel's limit: four vectors of 16 KiB, inside LVC_LDS_MAX with the tables and partials (74
// KiB at nel = 8, M = 6), and 2 ceil(1024 / nel / LVC_RES_TPB) base points per thread, no more registers than the
// single-state kernel's.  That is what the kernel is built for; the plan goes resident up to the measured crossover of
// the mode count, as the driven plan does.  nel = 3, one pair, one block, a record every step, us per step resident /
// staged (tools/bench_lvc.py --pair --scan, profiles/lvc_pair/): M = 1: 12.8 / 21.2 at D = 510, 15.3 / 22.7 at 1023;
// M = 2: 17.7 / 23.0 at 768, 21.5 / 24.9 at 972; M = 3: 22.2 / 26.5 at 756, 28.1 / 27.2 at 840, 27.8 / 27.7 at 882;
// M = 4: 26.3 / 28.0 at 768, 33.9 / 29.3 at 960; M = 5: 30.9 / 31.1 at 729, 40.8 / 33.3 at 972; M = 6: 33.9 / 31.3 at
// 192, 36.6 / 33.1 at 288, 35.5 / 32.6 at 480, 46.6 / 35.6 at 972.  From three modes on the step from one to two
// points per thread of the record's tile (nvib > 256, D > 768 at nel = 3) is where staged takes over; in six modes the
// one workgroup never catches the staged launches, so the plan never chooses it there (a forced call is refused).
constexpr long LVC_PAIR_RESIDENT_MAX_D = LVC_RESIDENT_MAX_D / 2;
constexpr long LVC_PAIR_RESIDENT_MAX_D_M345 = 768;
constexpr long lvc_pair_resident_limit(int M) {
  return M <= 2 ? LVC_PAIR_RESIDENT_MAX_D : M <= 5 ? LVC_PAIR_RESIDENT_MAX_D_M345 : 0;
}

// The blocks of a call as the kernels take them (a kernel argument by value, as LvcDev)
struct LvcPairBlocks {
  int nblk;
  int r[1 + LVC_MAX_MODES];   // 0: ket, j + 1: x_j ket
};

struct LvcPairPlan {
  int refused;   // then only msg is set
  LvcPlan base;  // lvc_plan() of the 2 P states with the pair limit's path: dev, the stage launch, the two stage vectors
  int P;
  LvcPairBlocks blocks;
  int rows;      // rows a of a block that one pass accumulates: nel (nel <= LVC_PAIR_REG_NEL) or 1
  int passes;    // nel / rows
  int nv;        // doubles of one partial row: 2 nel rows (value v: row v / (2 nel), column (v / 2) % nel, re | im)
  int nrec;      // complex values of one record: nblk nel^2
  LvcLaunch part;       // grid (base.G, nblk passes, P)
  LvcLaunch fin;        // grid (P)
  LvcLaunch resident;   // the whole call: grid (P)
  // resident LDS in bytes from the 16-byte aligned base: ket A | ket B | bra A | bra B | Hel and W | wave partials |
  // tile partials
  size_t lds_ket1, lds_bra0, lds_bra1, lds_tab, lds_wave, lds_tile;
  // scratch in bytes: the two stage vectors of the 2 P states (base.ws_x0, base.ws_x1), then the partial rows
  // [P][nblk][passes][G][nv] doubles in the place of the observable partials, which a pair call never takes
  size_t ws_part, ws_part_bytes, ws_total;   // qd_lvc_pair_observe takes ws_part_bytes alone
  char msg[200];
};

// What qd_lvc_pair_observe and qd_lvc_pair_rk4 admit, and what they launch.  path_req, nsteps and save_every matter to
// qd_lvc_pair_rk4 only (qd_lvc_pair_observe passes LVC_AUTO, 0, 0).
inline LvcPairPlan lvc_pair_plan(const char* fn, long P, int nel, int M, const int* dims, int nblk, const int* blocks,
                                 int path_req = LVC_AUTO, int nsteps = 0, int save_every = 0) {
  LvcPairPlan p{};
  p.refused = 1;
  auto refuse = [&](auto... a) {
    std::snprintf(p.msg, sizeof p.msg, a...);
    return p;
  };
  if (!(P >= 1 && P <= LVC_PAIR_MAX)) return refuse("%s: P=%ld outside [1, %d]", fn, P, LVC_PAIR_MAX);
  // the shape, with the path left open (the pair limit decides it below); a run records, so save_every >= 1
  p.base = lvc_plan(fn, 2 * P, nel, M, dims, path_req == LVC_RESIDENT ? LVC_AUTO : path_req, nsteps, save_every, true);
  if (p.base.refused) return refuse("%s", p.base.msg);
  if (!blocks) return refuse("%s: null blocks", fn);
  if (!(nblk >= 1 && nblk <= 1 + M)) return refuse("%s: nblk=%d outside [1, %d]", fn, nblk, 1 + M);
  for (int k = 0; k < nblk; ++k)
    if (!(blocks[k] >= 0 && blocks[k] <= M)) return refuse("%s: blocks[%d]=%d outside [0, %d]", fn, k, blocks[k], M);
  const long D = p.base.dev.D;
  const long limit = lvc_pair_resident_limit(M);
  const bool fits = D <= limit;
  if (path_req == LVC_RESIDENT && !fits)
    return refuse("%s: the pair resident path needs D <= %ld with %d modes (D = %ld)", fn, limit, M, D);
  p.refused = 0;
  p.base.path = path_req == LVC_AUTO ? (fits ? LVC_RESIDENT : LVC_STAGED) : path_req;
  p.P = (int)P;
  p.blocks.nblk = nblk;
  for (int k = 0; k <= LVC_MAX_MODES; ++k) p.blocks.r[k] = k < nblk ? blocks[k] : 0;
  p.rows = nel <= LVC_PAIR_REG_NEL ? nel : 1;
  p.passes = nel / p.rows;
  p.nv = 2 * nel * p.rows;
  p.nrec = nblk * nel * nel;
  p.part = LvcLaunch{(unsigned)p.base.G, (unsigned)(nblk * p.passes), (unsigned)P, LVC_TILE, 0};
  p.fin = LvcLaunch{(unsigned)P, 1, 1, LVC_TILE, 0};
  if (fits) {
    const size_t vec = (size_t)D * 16;
    p.lds_ket1 = vec;
    p.lds_bra0 = 2 * vec;
    p.lds_bra1 = 3 * vec;
    p.lds_tab = 4 * vec;
    p.lds_wave = p.lds_tab + (size_t)(1 + M) * nel * nel * 16;
    p.lds_tile = p.lds_wave + lvc_align16((size_t)(LVC_RES_TPB / 64) * LVC_PAIR_NV_MAX * 8);
    p.resident = LvcLaunch{(unsigned)P, 1, 1, LVC_RES_TPB,
                           p.lds_tile + lvc_align16((size_t)lvc_ceil(LVC_PAIR_RESIDENT_MAX_D, LVC_TILE) *
                                                    LVC_PAIR_NV_MAX * 8)};
  }
  p.ws_part = p.base.ws_part;
  p.ws_part_bytes = lvc_align16((size_t)P * nblk * p.passes * p.base.G * p.nv * 8);
  p.ws_total = p.ws_part + p.ws_part_bytes;
  return p;
}

// f(int_c<NEL>{}) for the plan's nel: the kernels are instantiated for 1 .. LVC_MAX_NEL
template <typename F>
bool dispatch_lvc_nel(int nel, F&& f) {
  return dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(nel, f);
}

}  // namespace qd
