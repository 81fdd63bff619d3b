// Host build of pyqed_amd/csrc/response_plan.hpp for tests/test_response_plan_host.py: the plans as C functions.
#include "../../pyqed_amd/csrc/response_plan.hpp"

using namespace qd;

extern "C" {
// ENS_BT, ENS_KT, ZMAX, UNI_ROWS, XU_ROWS, UNI_MAXC, ENS_MIN_TILES128, GRID_YZ_MAX, XZ_XROWS
void plan_resp_constants(int* out) {
  const int c[] = {ENS_BT, ENS_KT, ZMAX, UNI_ROWS, XU_ROWS, UNI_MAXC, ENS_MIN_TILES128, GRID_YZ_MAX, XZ_XROWS};
  std::copy(c, c + 9, out);
}
void plan_ens_dims(int M, int nL, int n3, int n1, EnsDims* out) { *out = ens_dims(M, nL, n3, n1); }
int plan_ens_sizes_ok(long M, long nL) { return ens_sizes_ok(M, nL); }
int plan_z_group(int nL, int nz, int n1p, int M) { return z_group(nL, nz, n1p, M); }
size_t plan_z_lds(int G, int nL, int nz, int n1p) { return z_lds(G, nL, nz, n1p); }
void plan_ens(const char* fn, int M, int nL, int nz, int n3, int n1, int t3_uniform, int t1_uniform, int trans,
              EnsPlan* out) {
  *out = ens_plan(fn, M, nL, nz, n3, n1, t3_uniform != 0, t1_uniform != 0, trans != 0);
}
void plan_t2ops(const char* fn, int M, int np, int nr, int nq, int n3, int n1, T2OpsPlan* out) {
  *out = t2ops_plan(fn, M, np, nr, nq, n3, n1);
}
void plan_t2apply(const char* fn, int M, int nL, int n3, int n1, int n2, T2ApplyPlan* out) {
  *out = t2apply_plan(fn, M, nL, n3, n1, n2);
}
void plan_resolvent(int n, int nx, int ny, ResolventPlan* out) { *out = resolvent_plan(n, nx, ny); }
void plan_splitk(int Mp, int Kp, int Np, int max_S, SplitKPlan* out) { *out = splitk_plan(Mp, Kp, Np, max_S); }
// 100 BT + 10 XTAB + DEPTH of the kernel the typed dispatch reaches, -1 when it reaches none
int plan_gemm_dispatch(const GemmPlan* g) {
  int hit = -1;
  dispatch_ens_gemm(*g, [&](auto k) {
    using T = decltype(k);
    hit = 100 * T::BT + 10 * T::XTAB + T::DEPTH;
    return true;
  });
  return hit;
}
}
