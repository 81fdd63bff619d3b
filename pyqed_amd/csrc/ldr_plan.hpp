// ldr_plan.hpp — the shape decisions of qd_ldr_run (ldr.hip) in plain C++17, no HIP, so that a host build can enumerate
// them (tools/cpu_emu/ldr_plan_c.cpp, tests/test_ldr_plan_host.py): what a call admits and every refusal with its
// message, the path (rotations fused into the first and last axis pass, or point kernels of their own), the launch of
// every axis pass with its tiling, the LDS bytes and the scratch layout.  ldr.hip executes what ldr_plan returns and
// decides nothing itself; ldr_kernels.hpp reads the same constants.
//
// One kinetic step of the local diabatic representation (pyqed/ldr/ldr.py:1564-1611, 579-625) is
//     psi'[p, a] = expV[p, a] sum_{q, b} (U(p)^+ U(q))[a, b] prod_d K_d[p_d, q_d] psi[q, b]
// and factorises over the M basis states the kept states U(p) [M, ns] are expanded in:
//     chi[q, mu]  = sum_b U[q, mu, b] psi[q, b]                      expand, per point
//     chi        <- (K_0 (x) K_1 (x) K_2) chi                        one dense mode product per axis
//     psi'[p, a]  = expV[p, a] sum_mu conj(U[p, mu, a]) chi[p, mu]   project and phase, per point
// chi is [B, npts, M] row-major (point index p = (p_0 n_1 + p_1) n_2 + p_2, last axis fastest, mu fastest of all).
//
// An axis pass out[o, i, in] = sum_k K[i, k] in[o, k, in] sees chi as C = B npts M / n columns of length n, `st`
// elements apart: column c = o * st + in, st = s * M with s the axis' stride in points.  A workgroup of LDR_WAVES waves
// owns LDR_RT rows and LDR_NSUB sub-tiles of LDR_SUB columns; sub-tile t of the pass covers the `cu` columns from
// t * cu on.  cu = LDR_SUB except in a projecting pass, where cu = (LDR_SUB / M) M keeps the M values of a point inside
// one sub-tile.  K is consumed in tiles of LDR_KT.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdio>

namespace qd {

constexpr int LDR_MAX_DIM = 3;
constexpr int LDR_MAX_M = 32;               // basis states per point; 1 <= ns <= M
constexpr int LDR_MAX_N = 4096;             // the longest axis (K_d is n x n: 256 MiB at the limit)
constexpr int LDR_WAVES = 4;
constexpr int LDR_TPB = 64 * LDR_WAVES;
constexpr int LDR_SUB = 16;                 // rows and columns of one MFMA tile (v_mfma_f64_16x16x4_f64)
constexpr int LDR_RT = LDR_SUB * LDR_WAVES; // rows per workgroup: one MFMA row tile per wave
constexpr int LDR_NSUB = 2;                 // column sub-tiles per workgroup: every A fragment is used twice
constexpr int LDR_CT = LDR_SUB * LDR_NSUB;  // columns the workgroup stages per K-tile
constexpr int LDR_KT = 32;                  // K-tile
constexpr int LDR_BS_STRIDE = LDR_CT + 1;   // elements between the k-rows of the staged B tile
constexpr int LDR_DS_STRIDE = LDR_SUB + 1;  // elements between the rows of a wave's finished tile (projecting pass)
// A projecting pass leaves LDR_SUB - (LDR_SUB / M) M columns of every sub-tile idle.  Fused when at most a quarter is.
constexpr int LDR_FUSE_MIN_COLS = 12;
constexpr int LDR_POINT_GRID_MAX = 4096;    // blocks of the grid-strided point kernels
constexpr long LDR_INDEX_MAX = (1L << 31) - 1;
constexpr size_t LDR_LDS_MAX = 64 * 1024;

enum LdrPath { LDR_AUTO = 0, LDR_FUSED = 1, LDR_SPLIT = 2 };
enum LdrBuf { LDR_BUF_PSI = 0, LDR_BUF_W0 = 1, LDR_BUF_W1 = 2 };   // psi: the step's input (src) or output (dst) state

struct LdrLaunch {
  unsigned gx, gy, gz;
  int tpb;
  size_t lds;   // dynamic LDS bytes
};

struct LdrAxis {
  int n;            // axis length
  int ktiles;       // K-tiles of LDR_KT
  int cu;           // columns used of every sub-tile
  int expand;       // the pass reads psi and U and forms chi as it stages its B tile
  int project;      // the pass projects with conj(U), multiplies expV and stores psi' (and the snapshot)
  int src, dst;     // LdrBuf
  unsigned s;       // axis stride in points
  unsigned st;      // axis stride in elements of chi: s * M
  unsigned outer;   // points-blocks of n * s per member: npts / (n * s)
  unsigned C;       // columns: B * npts * M / n
  LdrLaunch launch; // grid (column tiles, row tiles)
};

struct LdrPlan {
  int refused;      // then only msg is set
  int path;         // LDR_FUSED or LDR_SPLIT
  int ndim, M, ns, B;
  int n[LDR_MAX_DIM];
  long npts;
  int nsnap;        // snapshots: nsteps / nout
  int nrun;         // steps run: nsnap * nout (the reference drops what follows the last snapshot)
  LdrAxis axis[LDR_MAX_DIM];
  int expand_dst, project_src;   // split path: LdrBuf the expand kernel writes and the project kernel reads
  LdrLaunch open;       // psi0 * expVh, B npts ns elements
  LdrLaunch expand;     // B npts M elements (split)
  LdrLaunch project;    // B npts ns elements (split)
  // scratch in bytes: two states [B, npts, ns] | two work arrays [B, npts, M]
  size_t ws_psi0, ws_psi1, ws_w0, ws_w1, ws_total;
  char msg[200];
};

inline long ldr_ceil(long a, long b) { return (a + b - 1) / b; }
inline size_t ldr_align256(size_t n) { return (n + 255) & ~(size_t)255; }
inline int ldr_fused_cols(int M) { return M <= LDR_SUB ? (LDR_SUB / M) * M : 0; }
inline bool ldr_fusable(int M) { return ldr_fused_cols(M) >= LDR_FUSE_MIN_COLS; }

inline LdrLaunch ldr_point_launch(long elems) {
  return LdrLaunch{(unsigned)std::min<long>(std::max<long>(ldr_ceil(elems, LDR_TPB), 1), LDR_POINT_GRID_MAX), 1, 1,
                   LDR_TPB, 0};
}

inline LdrPlan ldr_plan(const char* fn, long B, int ndim, const int* dims, int M, int ns, int nsteps, int nout,
                        int path_req = LDR_AUTO) {
  LdrPlan p{};
  p.refused = 1;
  auto refuse = [&](auto... a) {
    std::snprintf(p.msg, sizeof p.msg, a...);
    return p;
  };
  if (!(ndim >= 1 && ndim <= LDR_MAX_DIM)) return refuse("%s: ndim=%d outside [1, %d]", fn, ndim, LDR_MAX_DIM);
  if (!dims) return refuse("%s: null dims", fn);
  if (!(ns >= 1 && ns <= M && M <= LDR_MAX_M))
    return refuse("%s: ns=%d, M=%d outside 1 <= ns <= M <= %d", fn, ns, M, LDR_MAX_M);
  if (!(B >= 1)) return refuse("%s: B=%ld must be at least 1", fn, B);
  if (B > LDR_INDEX_MAX / M) return refuse("%s: B * npts * M must stay below 2^31", fn);
  long tot = B * M;   // elements of chi
  long npts = 1;
  for (int d = 0; d < ndim; ++d) {
    if (!(dims[d] >= 1 && dims[d] <= LDR_MAX_N))
      return refuse("%s: dims[%d]=%d outside [1, %d]", fn, d, dims[d], LDR_MAX_N);
    if (tot > LDR_INDEX_MAX / dims[d]) return refuse("%s: B * npts * M must stay below 2^31", fn);
    tot *= dims[d];
    npts *= dims[d];
  }
  if (!(nsteps >= 0 && nout >= 1))
    return refuse("%s: nsteps=%d must not be negative and nout=%d at least 1", fn, nsteps, nout);
  if (!(path_req >= LDR_AUTO && path_req <= LDR_SPLIT)) return refuse("%s: path=%d outside [0, 2]", fn, path_req);
  if (path_req == LDR_FUSED && !ldr_fusable(M))
    return refuse("%s: the fused path needs (%d / M) * M >= %d columns of a tile (M = %d)", fn, LDR_SUB,
                  LDR_FUSE_MIN_COLS, M);
  p.refused = 0;
  p.path = path_req == LDR_AUTO ? (ldr_fusable(M) ? LDR_FUSED : LDR_SPLIT) : path_req;
  p.ndim = ndim;
  p.M = M;
  p.ns = ns;
  p.B = (int)B;
  p.npts = npts;
  p.nsnap = nsteps / nout;
  p.nrun = p.nsnap * nout;
  const bool fused = p.path == LDR_FUSED;

  long s = npts;
  for (int d = 0; d < ndim; ++d) {
    LdrAxis& a = p.axis[d];
    p.n[d] = a.n = dims[d];
    s /= dims[d];
    a.s = (unsigned)s;
    a.st = (unsigned)(s * M);
    a.outer = (unsigned)(npts / (dims[d] * s));
    a.C = (unsigned)(tot / dims[d]);
    a.ktiles = (int)ldr_ceil(a.n, LDR_KT);
    a.expand = fused && d == 0;
    a.project = fused && d == ndim - 1;
    a.cu = a.project ? ldr_fused_cols(M) : LDR_SUB;
    // fused: psi -> W0 -> W1 -> ... -> psi; split: W0 -> W1 -> W0 ...
    a.src = a.expand ? LDR_BUF_PSI : (fused ? LDR_BUF_W0 + (d - 1) % 2 : LDR_BUF_W0 + d % 2);
    a.dst = a.project ? LDR_BUF_PSI : (fused ? LDR_BUF_W0 + d % 2 : LDR_BUF_W0 + (d + 1) % 2);
    const size_t lds = (size_t)LDR_KT * LDR_BS_STRIDE * 16 +
                       (a.project ? (size_t)LDR_WAVES * LDR_SUB * LDR_DS_STRIDE * 16 : 0);
    a.launch = LdrLaunch{(unsigned)ldr_ceil(a.C, (long)LDR_NSUB * a.cu), (unsigned)ldr_ceil(a.n, LDR_RT), 1, LDR_TPB,
                         lds};
  }
  for (int d = ndim; d < LDR_MAX_DIM; ++d) p.n[d] = 1;
  p.expand_dst = LDR_BUF_W0;
  p.project_src = LDR_BUF_W0 + ndim % 2;
  p.open = ldr_point_launch(B * npts * ns);
  p.expand = ldr_point_launch(tot);
  p.project = ldr_point_launch(B * npts * ns);

  const size_t psi_b = ldr_align256((size_t)B * npts * ns * 16), w_b = ldr_align256((size_t)tot * 16);
  p.ws_psi0 = 0;
  p.ws_psi1 = psi_b;
  p.ws_w0 = 2 * psi_b;
  p.ws_w1 = p.ws_w0 + w_b;
  p.ws_total = p.ws_w1 + w_b;
  return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// qd_ldr_jacobi_run: the kinetic factor of LDR2_Jacobi (pyqed/ldr/ldr.py:1870-1936), whose propagator along the last
// axis differs for every row of the grid, expTy[i] = S diag(exp(-i E_m dt / I(x_i))) S.  Every row's matrix has the
// same eigenvectors, so the last axis is passed twice with a real matrix and the rows differ in a table only:
//     chi  = expand(psi) with U
//     chi <- F along the last axis, then chi[p] *= ph[p]      real matrix; ph has the grid's shape, mode index last
//     chi <- K_d along every axis d < ndim - 1                the plain complex pass of ldr_plan
//     chi <- Fb along the last axis                           real matrix
//     psi' = expV project(chi) with U^+
// The pass list is forward (axis ndim - 1), plain (axes 0 .. ndim - 2), back (axis ndim - 1): ndim + 1 passes.  A real
// pass has the geometry of a plain one (the B tile staged in LDS is complex either way); its A fragments are doubles
// and it issues two MFMAs per k-step where the plain pass issues four.  Fused path: the forward pass expands on load and
// multiplies ph on store, the back pass projects on store.  Split path: the point kernels of ldr_plan around the same
// passes, the forward one still multiplying ph.  What is admitted, every refusal and the scratch layout are ldr_plan's.
constexpr int LDR_JACOBI_MAX_PASS = LDR_MAX_DIM + 1;

struct LdrJacobiPass {
  int axis;         // the axis the pass runs along
  int real;         // the matrix is real (F or Fb): forward and back; 0: the plain ldr_axis_kernel with K[axis]
  int expand;       // forms chi from psi and U on load (forward, fused)
  int phase;        // multiplies ph[point block in its member, row] on store (forward)
  int project;      // projects with conj(U), multiplies expV and stores psi' (back, fused)
  int n, ktiles, cu;
  int src, dst;     // LdrBuf
  unsigned s, st, outer, C;
  LdrLaunch launch;
};

struct LdrJacobiPlan {
  int refused;      // then only msg is set
  int path;         // LDR_FUSED or LDR_SPLIT
  int ndim, M, ns, B;
  int n[LDR_MAX_DIM];
  long npts;
  int nsnap, nrun;
  int npass;        // ndim + 1
  LdrJacobiPass pass[LDR_JACOBI_MAX_PASS];
  int expand_dst, project_src;   // split path
  LdrLaunch open, expand, project;
  size_t ws_psi0, ws_psi1, ws_w0, ws_w1, ws_total;
  char msg[200];
};

inline LdrJacobiPlan ldr_jacobi_plan(const char* fn, long B, int ndim, const int* dims, int M, int ns, int nsteps,
                                     int nout, int path_req = LDR_AUTO) {
  LdrJacobiPlan p{};
  const LdrPlan b = ldr_plan(fn, B, ndim, dims, M, ns, nsteps, nout, path_req);
  if (b.refused) {
    p.refused = 1;
    std::copy(b.msg, b.msg + sizeof b.msg, p.msg);
    return p;
  }
  p.path = b.path;
  p.ndim = ndim;
  p.M = M;
  p.ns = ns;
  p.B = b.B;
  p.npts = b.npts;
  p.nsnap = b.nsnap;
  p.nrun = b.nrun;
  for (int d = 0; d < LDR_MAX_DIM; ++d) p.n[d] = b.n[d];
  const bool fused = p.path == LDR_FUSED;
  p.npass = ndim + 1;
  for (int i = 0; i < p.npass; ++i) {
    LdrJacobiPass& a = p.pass[i];
    const bool fwd = i == 0, back = i == p.npass - 1;
    a.axis = fwd || back ? ndim - 1 : i - 1;
    const LdrAxis& g = b.axis[a.axis];
    a.real = fwd || back;
    a.expand = fused && fwd;
    a.phase = fwd;
    a.project = fused && back;
    a.n = g.n;
    a.ktiles = g.ktiles;
    a.s = g.s;
    a.st = g.st;
    a.outer = g.outer;
    a.C = g.C;
    a.cu = a.project ? ldr_fused_cols(M) : LDR_SUB;
    // fused: psi -> W0 -> W1 -> ... -> psi; split: W0 -> W1 -> W0 ...
    a.src = a.expand ? LDR_BUF_PSI : (fused ? LDR_BUF_W0 + (i - 1) % 2 : LDR_BUF_W0 + i % 2);
    a.dst = a.project ? LDR_BUF_PSI : (fused ? LDR_BUF_W0 + i % 2 : LDR_BUF_W0 + (i + 1) % 2);
    const size_t lds = (size_t)LDR_KT * LDR_BS_STRIDE * 16 +
                       (a.project ? (size_t)LDR_WAVES * LDR_SUB * LDR_DS_STRIDE * 16 : 0);
    a.launch = LdrLaunch{(unsigned)ldr_ceil(a.C, (long)LDR_NSUB * a.cu), (unsigned)ldr_ceil(a.n, LDR_RT), 1, LDR_TPB,
                         lds};
  }
  p.expand_dst = LDR_BUF_W0;
  p.project_src = LDR_BUF_W0 + p.npass % 2;
  p.open = b.open;
  p.expand = b.expand;
  p.project = b.project;
  p.ws_psi0 = b.ws_psi0;
  p.ws_psi1 = b.ws_psi1;
  p.ws_w0 = b.ws_w0;
  p.ws_w1 = b.ws_w1;
  p.ws_total = b.ws_total;
  return p;
}

}  // namespace qd
