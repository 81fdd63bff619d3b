// sos_signals.hip — the sum-over-states signals of pyqed/signal/sos.py beyond photon_echo, in factorised form.
//
// Every third-order pathway there is a sum over three state indices of four dipoles times three factors: two Green's
// functions 1 / (w - z), each along one grid axis, and one fixed-delay exponential.  Summing the index that only the
// delay factor and the dipoles see leaves
//   S(i, j) = sum_p 1 / (x_i - zx[p]) * sum_q W[p][q] / (y_j - zy[p][q]),     z = (E_u - E_v) - i Gamma_uv,
// which three kernels evaluate (qd_sos_polesum):
//   build  (pathways only)  zx, zy, W from E, dip, gamma and the index lists; one thread per (p, q), which sums the
//          third index (exp / sincos in double, as sos.hip)
//   inner  T[p][j] = sum_q W[p][q] / (y_j - zy[p][q]): one reciprocal per (p, q, j); a workgroup owns one p and
//          SOS_THREADS values of j and stages row p of (zy, W) through LDS
//   outer  S(i, j) = sum_p 1 / (x_i - zx[p]) T[p][j]: SOS_TILE x SOS_TILE tiles; per round of SOS_PCHUNK poles one
//          reciprocal per (i, p), shared by the tile's j through LDS, next to the staged T rows
// Work per grid point is O(P); the sums run in index order in every kernel (no atomics), so a call repeats bit for bit.
// TPA (qd_sos_tpa) is not of that form: one thread per grid point at O(nf ne) is its minimal work.
#include "qd_common.hpp"
#include "sos_signals_tiles.hpp"

namespace qd {
namespace {

__device__ __forceinline__ c128 cinv(c128 z) {
  const double d = z.re * z.re + z.im * z.im;
  return cmk(z.re / d, -z.im / d);
}

// ------------------------------------------------------------------------------------------------ the pole sum
// T[p][j] = fd(j, p) * sum_q W[p][q] * fy(j, p, q); fd = 1 / (y_j - zx[p]) when the x factor is diagonal, else 1.
// Workgroup b: p = b / njt, j = (b % njt) * SOS_THREADS + thread.
__global__ __launch_bounds__(SOS_THREADS) void sos_inner_kernel(const c128* __restrict__ zx,
                                                                 const c128* __restrict__ zy,
                                                                 const c128* __restrict__ W, int Q,
                                                                 const double* __restrict__ y, int n1, int njt,
                                                                 int xdiag, int ypole, c128* __restrict__ T) {
  __shared__ c128 sz[SOS_QCHUNK];
  __shared__ c128 sw[SOS_QCHUNK];
  const int p = blockIdx.x / njt;
  const int j = (blockIdx.x % njt) * SOS_THREADS + threadIdx.x;
  const bool live = j < n1;
  const double yj = (live && (ypole || xdiag)) ? y[j] : 0.0;
  const size_t row = (size_t)p * Q;
  c128 acc = cmk(0, 0);
  for (int q0 = 0; q0 < Q; q0 += SOS_QCHUNK) {
    const int q = q0 + threadIdx.x;
    if (q < Q) {
      sw[threadIdx.x] = W[row + q];
      if (ypole) sz[threadIdx.x] = zy[row + q];
    }
    __syncthreads();
    const int nq = min(SOS_QCHUNK, Q - q0);
    if (live) {
      if (ypole) {
        for (int k = 0; k < nq; ++k) {
          const c128 z = sz[k];
          acc = cadd(acc, cmul(sw[k], cinv(cmk(yj - z.re, -z.im))));
        }
      } else {
        for (int k = 0; k < nq; ++k) acc = cadd(acc, sw[k]);
      }
    }
    __syncthreads();
  }
  if (live) {
    if (xdiag) {
      const c128 z = zx[p];
      acc = cmul(acc, cinv(cmk(yj - z.re, -z.im)));
    }
    T[(size_t)p * n1 + j] = acc;
  }
}

// S(i, j) = sum_p fx(i, p) T[p][j]; fx = 1 / (x_i - zx[p]) (xpole) or 1.  Tile b: rows (b / ntj) * SOS_TILE ...,
// columns (b % ntj) * SOS_TILE ...; IFAST: neighbouring threads run along i (the axis with stride 1), else along j.
template <bool IFAST>
__global__ __launch_bounds__(SOS_THREADS) void sos_outer_kernel(const c128* __restrict__ zx,
                                                                 const c128* __restrict__ T, int P,
                                                                 const double* __restrict__ x, int n0, int n1, int ntj,
                                                                 int xpole, c128* __restrict__ S, long si, long sj,
                                                                 int accumulate) {
  __shared__ c128 sg[SOS_PCHUNK][SOS_TILE];   // fx(i, p) of the round
  __shared__ c128 st[SOS_PCHUNK][SOS_TILE];   // T[p][j] of the round
  const int i0 = (blockIdx.x / ntj) * SOS_TILE, j0 = (blockIdx.x % ntj) * SOS_TILE;
  const int tid = threadIdx.x;
  const int ti = IFAST ? tid % SOS_TILE : tid / SOS_TILE;
  const int tj = IFAST ? tid / SOS_TILE : tid % SOS_TILE;
  // the staging thread's column of the tile: its x_i and its column of T do not change between rounds
  const int sc = tid % SOS_TILE, sr = tid / SOS_TILE;
  const bool xlive = i0 + sc < n0, tlive = j0 + sc < n1;
  const double xi = (xpole && xlive) ? x[i0 + sc] : 0.0;
  c128 acc = cmk(0, 0);
  for (int p0 = 0; p0 < P; p0 += SOS_PCHUNK) {
#pragma unroll
    for (int r = sr; r < SOS_PCHUNK; r += SOS_THREADS / SOS_TILE) {
      const int p = p0 + r;
      c128 g = cmk(0, 0), t = cmk(0, 0);
      if (p < P) {
        if (xlive) {
          if (xpole) {
            const c128 z = zx[p];
            g = cinv(cmk(xi - z.re, -z.im));
          } else {
            g = cmk(1, 0);
          }
        }
        if (tlive) t = T[(size_t)p * n1 + j0 + sc];
      }
      sg[r][sc] = g;
      st[r][sc] = t;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < SOS_PCHUNK; ++r) acc = cadd(acc, cmul(sg[r][ti], st[r][tj]));
    __syncthreads();
  }
  const int i = i0 + ti, j = j0 + tj;
  if (i < n0 && j < n1) {
    c128* o = S + (size_t)i * si + (size_t)j * sj;
    *o = accumulate ? cadd(*o, acc) : acc;
  }
}

int polesum_check(const char* who, int P, int Q, int n0, int n1) {
  QD_CHECK_ARG(P >= 0 && Q >= 0 && n0 >= 1 && n1 >= 1, "%s: bad sizes P=%d Q=%d n0=%d n1=%d", who, P, Q, n0, n1);
  QD_CHECK_ARG((size_t)P * (size_t)Q < ((size_t)1 << 31) && (size_t)P * (size_t)n1 < ((size_t)1 << 31),
               "%s: P*Q and P*n1 must stay below 2^31 (P=%d Q=%d n1=%d)", who, P, Q, n1);
  const size_t blocks_in = (size_t)P * ceil_div(n1, SOS_THREADS);
  const size_t blocks_out = (size_t)ceil_div(n0, SOS_TILE) * ceil_div(n1, SOS_TILE);
  QD_CHECK_ARG(blocks_in < ((size_t)1 << 31) && blocks_out < ((size_t)1 << 31), "%s: grid too large (n0=%d n1=%d)",
               who, n0, n1);
  return QD_OK;
}

// The two passes on scratch T [P][n1].  Arguments are checked by the callers.
int polesum_run(const c128* zx, const c128* zy, const c128* W, int P, int Q, const double* x, int n0, const double* y,
                int n1, int xkind, int ykind, c128* S, long si, long sj, int accumulate, c128* T, hipStream_t st) {
  if (accumulate && (P == 0 || Q == 0)) {
    note_path("sos_polesum_empty");
    return QD_OK;
  }
  if (Q == 0) P = 0;   // an empty inner sum: zeros, and no pole table is read
  if (P > 0) {
    const int njt = ceil_div(n1, SOS_THREADS);
    hipLaunchKernelGGL(sos_inner_kernel, dim3((unsigned)P * njt), dim3(SOS_THREADS), 0, st, zx, zy, W, Q, y, n1, njt,
                       (int)(xkind == QD_SOS_DIAG), (int)(ykind == QD_SOS_POLE), T);
    QD_HIP(hipGetLastError());
  }
  const int nti = ceil_div(n0, SOS_TILE), ntj = ceil_div(n1, SOS_TILE);
  const int xpole = xkind == QD_SOS_POLE;
  if (si == 1 && sj != 1) {
    note_path("sos_polesum_ifast");
    hipLaunchKernelGGL(sos_outer_kernel<true>, dim3((unsigned)nti * ntj), dim3(SOS_THREADS), 0, st, zx, T, P, x, n0, n1,
                       ntj, xpole, S, si, sj, accumulate);
  } else {
    note_path("sos_polesum_jfast");
    hipLaunchKernelGGL(sos_outer_kernel<false>, dim3((unsigned)nti * ntj), dim3(SOS_THREADS), 0, st, zx, T, P, x, n0,
                       n1, ntj, xpole, S, si, sj, accumulate);
  }
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// ------------------------------------------------------------------------------------------------ the pathways
struct SosModel {
  const c128* E;
  const c128* dip;
  const double* gam;
  int N;
  double deph;
  const int *gi, *ei, *fi;
  int ng, ne, nf;
  double t;
};

// Gamma_uv = (gamma_u + gamma_v) / 2 + pure dephasing off the diagonal
__device__ __forceinline__ double linewidth(const SosModel& m, int u, int v) {
  return 0.5 * (m.gam[u] + m.gam[v]) + (u != v ? m.deph : 0.0);
}
// z_uv of G_uv(w) = 1 / (w - (E_u - E_v) + i Gamma_uv) = 1 / (w - z_uv)
__device__ __forceinline__ c128 pole(const SosModel& m, int u, int v) {
  const c128 dE = csub(m.E[u], m.E[v]);
  return cmk(dE.re, dE.im - linewidth(m, u, v));
}
// exp(-i (E_u - E_v) t - Gamma_uv t)
__device__ __forceinline__ c128 delay_exp(const SosModel& m, int u, int v) {
  const c128 dE = csub(m.E[u], m.E[v]);
  double sn, cs;
  sincos(-dE.re * m.t, &sn, &cs);
  const double mag = exp(dE.im * m.t - linewidth(m, u, v) * m.t);
  return cmk(mag * cs, mag * sn);
}
// U_uv = -i exp(...), the retarded propagator of the reference
__device__ __forceinline__ c128 delay_u(const SosModel& m, int u, int v) { return cmulmi(delay_exp(m, u, v)); }
__device__ __forceinline__ c128 dp(const SosModel& m, int r, int c) { return m.dip[(size_t)r * m.N + c]; }
__device__ __forceinline__ c128 cmul3(c128 a, c128 b, c128 c) { return cmul(cmul(a, b), c); }

// One thread per (p, q): zx[p] (by the q == 0 thread), zy[p][q], W[p][q].  The dipole index order is the reference's.
__global__ __launch_bounds__(SOS_THREADS) void sos_build_kernel(int path, SosModel m, int P, int Q,
                                                                 c128* __restrict__ zx, c128* __restrict__ zy,
                                                                 c128* __restrict__ W) {
  const size_t e = (size_t)blockIdx.x * SOS_THREADS + threadIdx.x;
  if (e >= (size_t)P * Q) return;
  const int p = (int)(e / Q), q = (int)(e % Q);
  const int a = 0;
  c128 x, y, w, s = cmk(0, 0);
  switch (path) {
    case QD_SOS_GSB: {  // gg -> ge -> gg -> e'g -> gg; c = a
      const int b = m.ei[p], d = m.ei[q];
      x = pole(m, a, b);
      y = pole(m, d, a);
      w = cmul(cmul(dp(m, a, b), dp(m, b, a)), cmul(dp(m, a, d), dp(m, d, a)));
      break;
    }
    case QD_SOS_SE: {  // q = (c, d), d in g
      const int b = m.ei[p], c = m.ei[q / m.ng], d = m.gi[q % m.ng];
      x = pole(m, a, b);
      y = pole(m, c, d);
      w = cmul(cmul(cmul(dp(m, a, b), dp(m, c, a)), cmul(dp(m, d, c), dp(m, b, d))), delay_u(m, c, b));
      break;
    }
    case QD_SOS_ESA: {
      const int b = m.ei[p], d = m.fi[q];
      x = pole(m, a, b);
      y = pole(m, d, b);
      for (int k = 0; k < m.ne; ++k) {
        const int c = m.ei[k];
        s = cadd(s, cmul3(dp(m, c, a), dp(m, d, c), delay_u(m, c, b)));
      }
      w = cscale(cmul3(dp(m, b, a), dp(m, b, d), s), -1.0);
      break;
    }
    case QD_SOS_SE_T3: {
      const int b = m.ei[p], c = m.ei[q];
      x = pole(m, a, b);
      y = pole(m, c, b);
      for (int k = 0; k < m.ng; ++k) {
        const int d = m.gi[k];
        s = cadd(s, cmul3(dp(m, d, c), dp(m, b, d), delay_u(m, c, d)));
      }
      w = cmul3(dp(m, a, b), dp(m, c, a), s);
      break;
    }
    case QD_SOS_ESA_T3: {
      const int b = m.ei[p], c = m.ei[q];
      x = pole(m, a, b);
      y = pole(m, c, b);
      for (int k = 0; k < m.nf; ++k) {
        const int d = m.fi[k];
        s = cadd(s, cmul3(dp(m, d, c), dp(m, b, d), delay_u(m, d, b)));
      }
      w = cscale(cmul3(dp(m, b, a), dp(m, c, a), s), -1.0);
      break;
    }
    case QD_SOS_DQC_R1_T3: {  // both Green's functions at the second grid (the x factor is diagonal)
      const int b = m.ei[p], c = m.fi[q];
      x = pole(m, b, a);
      y = pole(m, c, a);
      for (int k = 0; k < m.ne; ++k) {
        const int d = m.ei[k];
        s = cadd(s, cmul3(dp(m, d, a), dp(m, d, c), delay_u(m, c, d)));
      }
      w = cscale(cmul3(dp(m, b, a), dp(m, c, b), s), -1.0);
      break;
    }
    case QD_SOS_DQC_R1_T1: {
      const int c = m.fi[p], d = m.ei[q];
      x = pole(m, c, a);
      y = pole(m, c, d);
      for (int k = 0; k < m.ne; ++k) {
        const int b = m.ei[k];
        s = cadd(s, cmul3(dp(m, b, a), dp(m, c, b), delay_u(m, b, a)));
      }
      w = cscale(cmul3(dp(m, d, a), dp(m, d, c), s), -1.0);
      break;
    }
    case QD_SOS_DQC_R2_T3: {
      const int b = m.ei[p], c = m.fi[q];
      x = pole(m, b, a);
      y = pole(m, c, a);
      for (int k = 0; k < m.ne; ++k) {
        const int d = m.ei[k];
        s = cadd(s, cmul3(dp(m, d, c), dp(m, a, d), delay_u(m, d, a)));
      }
      w = cmul3(dp(m, b, a), dp(m, c, b), s);
      break;
    }
    case QD_SOS_DQC_R2_T1: {  // the reference's delay factor carries no -i here
      const int c = m.fi[p], d = m.ei[q];
      x = pole(m, c, a);
      y = pole(m, d, a);
      for (int k = 0; k < m.ne; ++k) {
        const int b = m.ei[k];
        s = cadd(s, cmul3(dp(m, b, a), dp(m, c, b), delay_exp(m, b, a)));
      }
      w = cmul3(dp(m, d, c), dp(m, a, d), s);
      break;
    }
    default: {  // QD_SOS_CARS: p -> a, the omega1 pole; q -> (b, sign), the two poles of the Lorentzian in the shift:
      // L(s - w_ba; G) = (1 / 2 pi i) [1 / (s - w_ba - i G) - 1 / (s - w_ba + i G)]
      const int u = p + 1, b = q / 2 + 1, minus = q % 2;
      x = pole(m, u, a);
      if (b == u) {   // alpha_ba = 0 on the diagonal; a pole away from the real axis keeps 0 * fy finite
        y = cmk(0, 1);
        w = cmk(0, 0);
      } else {
        const c128 dE = csub(m.E[b], m.E[u]);
        const double G = linewidth(m, b, u);
        y = cmk(dE.re, dE.im + (minus ? -G : G));
        const double c = (minus ? -1.0 : 1.0) / (2.0 * 3.14159265358979323846);
        w = cmulmi(cscale(cmul(dp(m, b, a), dp(m, u, a)), c));
      }
      break;
    }
  }
  if (q == 0) zx[p] = x;
  zy[e] = y;
  W[e] = w;
}

// ------------------------------------------------------------------------------------------------ TPA
__global__ __launch_bounds__(SOS_THREADS) void sos_tpa_kernel(const double* __restrict__ E,
                                                               const c128* __restrict__ dip,
                                                               const double* __restrict__ gam, int N,
                                                               const int* __restrict__ ei, int ne,
                                                               const int* __restrict__ fi, int nf,
                                                               const double* __restrict__ wp, int np,
                                                               const double* __restrict__ w1s, int n1, int second,
                                                               double* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * SOS_THREADS + threadIdx.x;
  if (e >= (size_t)np * n1) return;
  const int i = (int)(e / n1), j = (int)(e % n1);
  const double w = wp[i];
  const double w1 = w1s ? w1s[j] : 0.5 * w;
  const double w2 = w - w1;
  const double E0 = E[0];
  double sig = 0.0;
  for (int kf = 0; kf < nf; ++kf) {
    const int f = fi[kf];
    c128 amp = cmk(0, 0);
    for (int km = 0; km < ne; ++km) {
      const int mm = ei[km];
      const double em = E[mm] - E0, g = gam[mm];
      c128 r = cinv(cmk(w1 - em, g));
      if (second) r = cadd(r, cinv(cmk(w2 - em, g)));
      amp = cadd(amp, cmul(cmul(dip[(size_t)f * N + mm], dip[(size_t)mm * N]), r));
    }
    const double gf = gam[f], xf = w - E[f] + E0;
    sig += (amp.re * amp.re + amp.im * amp.im) * (gf / (3.14159265358979323846 * (gf * gf + xf * xf)));
  }
  out[e] = sig;
}

}  // namespace
}  // namespace qd

using namespace qd;

extern "C" int qd_sos_polesum(const qd_c128* zx, const qd_c128* zy, const qd_c128* W, int P, int Q, const double* x,
                              int n0, const double* y, int n1, int xkind, int ykind, qd_c128* S, long stride_i,
                              long stride_j, int accumulate, void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(xkind >= QD_SOS_POLE && xkind <= QD_SOS_DIAG && (ykind == QD_SOS_POLE || ykind == QD_SOS_UNITY),
               "qd_sos_polesum: xkind=%d ykind=%d", xkind, ykind);
  QD_TRY(polesum_check("qd_sos_polesum", P, Q, n0, n1));
  QD_CHECK_ARG(S && (W || P == 0 || Q == 0), "qd_sos_polesum: null pointer (S, W)");
  QD_CHECK_ARG(P == 0 || Q == 0 || ((xkind == QD_SOS_UNITY || zx) && (ykind == QD_SOS_UNITY || zy)),
               "qd_sos_polesum: null pole table");
  QD_CHECK_ARG((xkind != QD_SOS_POLE || x) && ((ykind == QD_SOS_UNITY && xkind != QD_SOS_DIAG) || y),
               "qd_sos_polesum: null grid");
  QD_CHECK_ARG((stride_j == 1 && stride_i >= n1) || (stride_i == 1 && stride_j >= n0),
               "qd_sos_polesum: strides (%ld, %ld) do not address %d x %d distinct elements", stride_i, stride_j, n0,
               n1);
  hipStream_t st = (hipStream_t)stream;
  void* w = nullptr;
  QD_TRY(workspace(WS_MISC, (size_t)P * n1 * sizeof(c128), &w, st));
  return polesum_run((const c128*)zx, (const c128*)zy, (const c128*)W, P, Q, x, n0, y, n1, xkind, ykind, (c128*)S,
                     stride_i, stride_j, accumulate, (c128*)w, st);
}

extern "C" int qd_sos_pathway(int pathway, const qd_c128* E, const qd_c128* dip, const double* gamma, int N,
                              double dephasing, const int32_t* g_idx, int ng, const int32_t* e_idx, int ne,
                              const int32_t* f_idx, int nf, double delay, const double* wa, int na, const double* wb,
                              int nb, qd_c128* S, int accumulate, void* stream) {
  WsScope wss_((hipStream_t)stream);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(pathway >= 0 && pathway < QD_SOS_NPATHWAYS, "qd_sos_pathway: unknown pathway %d", pathway);
  QD_CHECK_ARG(E && dip && gamma && wa && wb && S, "qd_sos_pathway: null pointer");
  QD_CHECK_ARG(N >= 1 && N <= 32768 && na >= 1 && nb >= 1 && ng >= 0 && ne >= 0 && nf >= 0 && ng <= N && ne <= N &&
                   nf <= N,
               "qd_sos_pathway: bad sizes N=%d na=%d nb=%d ng=%d ne=%d nf=%d", N, na, nb, ng, ne, nf);
  QD_CHECK_ARG((g_idx || !ng) && (e_idx || !ne) && (f_idx || !nf), "qd_sos_pathway: null index list");
  // the axis paired with p (x) and the one paired with (p, q) (y); S(i, j) at S[i * si + j * sj]
  int P = 0, Q = 0, xkind = QD_SOS_POLE;
  bool x_is_a = true, out_ab = true;   // x is the first grid; S is laid [na][nb]
  const char* name = "";
  switch (pathway) {
    case QD_SOS_GSB: P = ne, Q = ne, out_ab = false, name = "sos_gsb"; break;
    case QD_SOS_SE: P = ne, Q = ne * ng, out_ab = false, name = "sos_se"; break;   // ne, ng <= N <= 2^15
    case QD_SOS_ESA: P = ne, Q = nf, out_ab = false, name = "sos_esa"; break;
    case QD_SOS_SE_T3: P = ne, Q = ne, out_ab = false, name = "sos_se_t3"; break;
    case QD_SOS_ESA_T3: P = ne, Q = ne, out_ab = false, name = "sos_esa_t3"; break;
    case QD_SOS_DQC_R1_T3: P = ne, Q = nf, xkind = QD_SOS_DIAG, name = "sos_dqc_r1_t3"; break;
    case QD_SOS_DQC_R1_T1: P = nf, Q = ne, name = "sos_dqc_r1_t1"; break;
    case QD_SOS_DQC_R2_T3: P = ne, Q = nf, name = "sos_dqc_r2_t3"; break;
    case QD_SOS_DQC_R2_T1: P = nf, Q = ne, name = "sos_dqc_r2_t1"; break;
    default: P = N - 1, Q = 2 * (N - 1), x_is_a = false, name = "sos_cars"; break;
  }
  const double* x = x_is_a ? wa : wb;
  const double* y = x_is_a ? wb : wa;
  const int n0 = x_is_a ? na : nb, n1 = x_is_a ? nb : na;
  QD_TRY(polesum_check("qd_sos_pathway", P, Q, n0, n1));
  // [na][nb] with x = wa: (nb, 1); [nb][na] with x = wa: (1, na); [na][nb] with x = wb (CARS): (1, nb)
  const long si = (x_is_a && out_ab) ? nb : 1;
  const long sj = (x_is_a && out_ab) ? 1 : (x_is_a ? na : nb);
  hipStream_t st = (hipStream_t)stream;
  const size_t nPQ = (size_t)P * Q, nT = (size_t)P * n1;
  void* w = nullptr;
  QD_TRY(workspace(WS_MISC, ((size_t)P + 2 * nPQ + nT) * sizeof(c128), &w, st));
  c128* zx = (c128*)w;
  c128* zy = zx + P;
  c128* Wt = zy + nPQ;
  c128* T = Wt + nPQ;
  note_path(name);
  if (nPQ) {
    const SosModel m = {(const c128*)E, (const c128*)dip, gamma, N, dephasing, g_idx, e_idx, f_idx, ng, ne, nf, delay};
    hipLaunchKernelGGL(sos_build_kernel, dim3((unsigned)ceil_div((long)nPQ, SOS_THREADS)), dim3(SOS_THREADS), 0, st,
                       pathway, m, P, Q, zx, zy, Wt);
    QD_HIP(hipGetLastError());
  }
  return polesum_run(zx, zy, Wt, P, Q, x, n0, y, n1, xkind, QD_SOS_POLE, (c128*)S, si, sj, accumulate, T, st);
}

extern "C" int qd_sos_tpa(const double* E, const qd_c128* dip, const double* gamma, int N, const int32_t* e_idx, int ne,
                          const int32_t* f_idx, int nf, const double* wp, int np, const double* w1, int n1,
                          int second_order, double* signal, void* stream) {
  QD_CHECK_ARG(E && dip && gamma && wp && signal, "qd_sos_tpa: null pointer");
  QD_CHECK_ARG(N >= 1 && np >= 1 && n1 >= 1 && ne >= 0 && nf >= 0 && (w1 || n1 == 1),
               "qd_sos_tpa: bad sizes N=%d np=%d n1=%d ne=%d nf=%d (n1 = 1 without w1)", N, np, n1, ne, nf);
  QD_CHECK_ARG((e_idx || !ne) && (f_idx || !nf), "qd_sos_tpa: null index list");
  const size_t tot = (size_t)np * n1;
  QD_CHECK_ARG(tot / SOS_THREADS < ((size_t)1 << 31) - 1, "qd_sos_tpa: grid too large");
  note_path("sos_tpa");
  hipLaunchKernelGGL(sos_tpa_kernel, dim3((unsigned)ceil_div((long)tot, SOS_THREADS)), dim3(SOS_THREADS), 0,
                     (hipStream_t)stream, E, (const c128*)dip, gamma, N, e_idx, ne, f_idx, nf, wp, np, w1, n1,
                     second_order, signal);
  QD_HIP(hipGetLastError());
  return QD_OK;
}
