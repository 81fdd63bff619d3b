// Stand-alone walk over pyqed_amd/csrc/ldr_plan.hpp for a sanitizer build of the host code (no GPU, no Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/cpu_emu/ldr_plan_main.cpp -o ldr_plan_san && ./ldr_plan_san
// Plans every axis length 1 .. 130 and around the longest on every axis of one to three dimensions, the whole
// 1 <= ns <= M <= 32 square, B in {1, 3, 64, 2^31 - 1}, every path request and out-of-range arguments, and checks what
// a reader of the plan relies on: tiles cover rows, K and columns, the buffers chain, the scratch parts are disjoint.
// Every call is planned by ldr_jacobi_plan as well (forward, plain and back passes of qd_ldr_jacobi_run).
#include <cstdlib>
#include <cstring>

#include "../../pyqed_amd/csrc/ldr_plan.hpp"

using namespace qd;

static long plans = 0, refusals = 0;

static void fail(const char* what, const LdrPlan& p) {
  std::fprintf(stderr, "ldr_plan_main: %s (ndim=%d M=%d ns=%d B=%d n=%d,%d,%d)\n", what, p.ndim, p.M, p.ns, p.B,
               p.n[0], p.n[1], p.n[2]);
  std::exit(1);
}

static void walk_jacobi(long B, int ndim, const int* dims, int M, int ns, int nsteps, int nout, int path,
                        const LdrPlan& base) {
  const LdrJacobiPlan p = ldr_jacobi_plan("ldr_plan_main", B, ndim, dims, M, ns, nsteps, nout, path);
  if (p.refused != base.refused || std::strcmp(p.msg, base.msg)) fail("jacobi: refusal differs from ldr_plan's", base);
  if (p.refused) return;
  const bool fused = p.path == LDR_FUSED;
  if (p.npass != p.ndim + 1 || p.npass > LDR_JACOBI_MAX_PASS) fail("jacobi: pass count", base);
  int prev = fused ? (int)LDR_BUF_PSI : p.expand_dst;
  for (int i = 0; i < p.npass; ++i) {
    const LdrJacobiPass& a = p.pass[i];
    const bool end = i == 0 || i == p.npass - 1;
    if (a.axis != (end ? p.ndim - 1 : i - 1) || a.real != end || a.phase != (i == 0)) fail("jacobi: pass order", base);
    if (a.real && (a.s != 1 || a.st != (unsigned)p.M || (long)a.outer * a.n != p.npts)) fail("jacobi: real axis", base);
    if ((long)a.launch.gy * LDR_RT < a.n || (long)(a.launch.gy - 1) * LDR_RT >= a.n) fail("jacobi: row tiles", base);
    if ((long)a.ktiles * LDR_KT < a.n || (long)(a.ktiles - 1) * LDR_KT >= a.n) fail("jacobi: K-tiles", base);
    const long per = (long)LDR_NSUB * a.cu;
    if ((long)a.launch.gx * per < (long)a.C || (long)(a.launch.gx - 1) * per >= (long)a.C)
      fail("jacobi: column tiles", base);
    if (a.project && (a.cu % p.M || a.C % p.M)) fail("jacobi: a point straddles sub-tiles", base);
    if (a.launch.lds > LDR_LDS_MAX) fail("jacobi: LDS", base);
    if (a.src != prev || a.src == a.dst) fail("jacobi: buffer chain", base);
    prev = a.dst;
  }
  if (prev != (fused ? (int)LDR_BUF_PSI : p.project_src)) fail("jacobi: buffer chain end", base);
  if (p.ws_psi1 != base.ws_psi1 || p.ws_w0 != base.ws_w0 || p.ws_w1 != base.ws_w1 || p.ws_total != base.ws_total)
    fail("jacobi: scratch layout differs from ldr_plan's", base);
}

static void walk(long B, int ndim, const int* dims, int M, int ns, int nsteps, int nout, int path) {
  const LdrPlan p = ldr_plan("ldr_plan_main", B, ndim, dims, M, ns, nsteps, nout, path);
  walk_jacobi(B, ndim, dims, M, ns, nsteps, nout, path, p);
  if (p.refused) {
    if (std::strlen(p.msg) == 0 || std::strlen(p.msg) >= sizeof p.msg - 1) fail("refusal without a whole message", p);
    ++refusals;
    return;
  }
  ++plans;
  const bool fused = p.path == LDR_FUSED;
  int prev = fused ? (int)LDR_BUF_PSI : p.expand_dst;
  for (int d = 0; d < p.ndim; ++d) {
    const LdrAxis& a = p.axis[d];
    if ((long)a.launch.gy * LDR_RT < a.n || (long)(a.launch.gy - 1) * LDR_RT >= a.n) fail("row tiles", p);
    if ((long)a.ktiles * LDR_KT < a.n || (long)(a.ktiles - 1) * LDR_KT >= a.n) fail("K-tiles", p);
    const long per = (long)LDR_NSUB * a.cu;
    if ((long)a.launch.gx * per < (long)a.C || (long)(a.launch.gx - 1) * per >= (long)a.C) fail("column tiles", p);
    if (a.project && (a.cu % p.M || a.C % p.M || a.s != 1)) fail("a point straddles sub-tiles", p);
    if (a.launch.lds > LDR_LDS_MAX) fail("LDS", p);
    if (a.src != prev || (a.src == a.dst && a.src != LDR_BUF_PSI)) fail("buffer chain", p);
    prev = a.dst;
  }
  if (prev != (fused ? (int)LDR_BUF_PSI : p.project_src)) fail("buffer chain end", p);
  const size_t psi_b = (size_t)p.B * p.npts * p.ns * 16, w_b = (size_t)p.B * p.npts * p.M * 16;
  if (p.ws_psi1 - p.ws_psi0 < psi_b || p.ws_w0 - p.ws_psi1 < psi_b || p.ws_w1 - p.ws_w0 < w_b ||
      p.ws_total - p.ws_w1 < w_b)
    fail("scratch overlap", p);
}

int main() {
  const long Bs[] = {1, 3, 64, LDR_INDEX_MAX, 0, -1, 1L << 40};
  for (int n = 1; n <= 130; ++n)
    for (int M = 1; M <= LDR_MAX_M; M += (n % 7 == 0 ? 1 : 5))
      for (int ns = 1; ns <= M; ns += 3)
        for (long B : Bs)
          for (int path = -1; path <= 3; ++path) {
            const int shapes[][3] = {{n, 1, 1}, {n, 3, 1}, {3, n, 1}, {n, 3, 4}, {3, n, 4}, {3, 4, n}};
            const int nd[] = {1, 2, 2, 3, 3, 3};
            for (int k = 0; k < 6; ++k) walk(B, nd[k], shapes[k], M, ns, 5, 2, path);
          }
  for (int M = 0; M <= LDR_MAX_M + 1; ++M)
    for (int ns = 0; ns <= M + 1; ++ns)
      for (int n : {1, LDR_KT, LDR_RT + 1, LDR_MAX_N - 1, LDR_MAX_N, LDR_MAX_N + 1, 0, -5}) {
        const int d3[3] = {n, LDR_MAX_N, 2};
        for (int ndim = 0; ndim <= 4; ++ndim)
          for (int nout = 0; nout <= 2; ++nout) walk(1, ndim, d3, M, ns, 7, nout, LDR_AUTO);
      }
  walk(1, 2, nullptr, 2, 2, 1, 1, LDR_AUTO);
  std::printf("ldr_plan_main: %ld plans, %ld refusals, all consistent\n", plans, refusals);
  return plans > 100000 && refusals > 10000 ? 0 : 1;
}
