// spo_observe.hip — observables of split-operator states on the device (gfx950).
//
// For B states psi [npts][ns] (npts = n0 n1 n2 in C order, state index fastest: the layout of psi and snap everywhere
// in the SPO code) and chi(p) = M(p) psi(p) (chi_a = sum_b M[p][a][b] psi_b; M null: chi = psi):
//   rdm[a][b] = w sum_p conj(chi_a(p)) chi_b(p)         electronic reduced density matrix (populations on the diagonal)
//   mom[d][a] = w sum_p x_d(p) |chi_a(p)|^2             first moments per state along axis d
// (SPO2.population / rdm_el, ResultSPO2.get_population / position of pyqed/wpd.py:104-160, 627-689, which reduce every
// state on the host).
//
// Summation order is fixed by the shape: per-thread register accumulators over a grid-stride loop, a shuffle
// reduction inside each wave, the waves of a workgroup summed in wave order through LDS, one partial row per workgroup
// in call-scoped scratch, and a second kernel that sums the rows in index order (contiguous chunks in order, then the
// chunks in order).  No float atomics and no counters, so results are bit-identical from run to run and under graph
// replay, and nothing has to be re-zeroed between launches.
//
// Register path (ns <= 4): the upper triangle (<= 10 complex) and the moments (<= 12 real) stay in registers, psi is
// read once with 16-byte loads and the basis is applied in registers.  Generic path (ns > 4): one block row per
// (a <= b) pair, each re-reading its two components of chi -- ns (ns + 1) / 2 passes over the state instead of one,
// accepted because this path exists for coverage of every ns the run entry points take, not for speed; with a basis a
// pre-pass writes chi to scratch first so that the pairs do not each redo the ns x ns product.
#include "qd_common.hpp"

namespace qd {
namespace {

constexpr int OBS_BLOCK = 256;       // 4 waves
constexpr int OBS_MAX_GRID = 1024;   // partial rows per state
constexpr int OBS_GEN_GRID = 64;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;   // lane 0 holds the wave's sum
}

// Partial row of a workgroup: [2 t], [2 t + 1] = Re, Im of pair t = (a <= b) in row-major upper-triangle order, then
// (MOM) [2 NP + d ns + a] for d = 0..2.
template <int NS, bool BASIS, bool MOM>
__global__ __launch_bounds__(OBS_BLOCK) void spo_obs_reg_kernel(const c128* __restrict__ psi, size_t bstride,
                                                                const c128* __restrict__ basis, unsigned npts,
                                                                unsigned n1, unsigned n2, const double* __restrict__ x0,
                                                                const double* __restrict__ x1,
                                                                const double* __restrict__ x2, double* __restrict__ part) {
  constexpr int NP = NS * (NS + 1) / 2, NV = 2 * NP + (MOM ? 3 * NS : 0);
  const c128* ps = psi + (size_t)blockIdx.y * bstride;
  double acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = 0.0;
  const unsigned stride = gridDim.x * OBS_BLOCK;
  for (unsigned p = blockIdx.x * OBS_BLOCK + threadIdx.x; p < npts; p += stride) {
    c128 u[NS], c[NS];
#pragma unroll
    for (int a = 0; a < NS; ++a) u[a] = ps[(size_t)p * NS + a];
    if constexpr (BASIS) {
      const c128* M = basis + (size_t)p * NS * NS;
#pragma unroll
      for (int a = 0; a < NS; ++a) {
        c[a] = cmul(M[a * NS], u[0]);
#pragma unroll
        for (int b = 1; b < NS; ++b) c[a] = cadd(c[a], cmul(M[a * NS + b], u[b]));
      }
    } else {
#pragma unroll
      for (int a = 0; a < NS; ++a) c[a] = u[a];
    }
    double xs[3];
    if constexpr (MOM) {
      const unsigned q = p / n2;
      xs[2] = x2[p - q * n2];
      const unsigned i = q / n1;
      xs[1] = x1[q - i * n1];
      xs[0] = x0[i];
    }
    int t = 0;
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      const double pa = c[a].re * c[a].re + c[a].im * c[a].im;
      acc[2 * t] += pa;
      ++t;
      if constexpr (MOM) {
#pragma unroll
        for (int d = 0; d < 3; ++d) acc[2 * NP + d * NS + a] += xs[d] * pa;
      }
#pragma unroll
      for (int b = a + 1; b < NS; ++b) {
        acc[2 * t] += c[a].re * c[b].re + c[a].im * c[b].im;
        acc[2 * t + 1] += c[a].re * c[b].im - c[a].im * c[b].re;
        ++t;
      }
    }
  }
  __shared__ double sh[OBS_BLOCK / 64][NV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const double s = wave_sum(acc[v]);
    if (lane == 0) sh[wave][v] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < OBS_BLOCK / 64; ++w) s += sh[w][threadIdx.x];
    part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NV + threadIdx.x] = s;
  }
}

// chi = M psi for any ns: one thread per component
__global__ void spo_obs_chi_kernel(const c128* __restrict__ psi, size_t bstride, const c128* __restrict__ basis,
                                   size_t nel, int ns, c128* __restrict__ chi) {
  const c128* ps = psi + (size_t)blockIdx.y * bstride;
  c128* out = chi + (size_t)blockIdx.y * nel;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nel; e += (size_t)gridDim.x * blockDim.x) {
    const size_t p = e / ns;
    const c128* M = basis + e * ns;   // row a = e - p ns of the point's matrix
    const c128* u = ps + p * ns;
    c128 acc = cmul(M[0], u[0]);
    for (int b = 1; b < ns; ++b) acc = cadd(acc, cmul(M[b], u[b]));
    out[e] = acc;
  }
}

// Generic path: blockIdx.y = pair t = (a <= b), blockIdx.z = member; the same partial-row layout as the register path.
__global__ __launch_bounds__(OBS_BLOCK) void spo_obs_gen_kernel(const c128* __restrict__ chi, size_t bstride,
                                                                unsigned npts, int ns, unsigned n1, unsigned n2,
                                                                const double* __restrict__ x0,
                                                                const double* __restrict__ x1,
                                                                const double* __restrict__ x2, int mom_on,
                                                                double* __restrict__ part, int NV) {
  int a = 0, b = (int)blockIdx.y;
  while (b >= ns - a) {
    b -= ns - a;
    ++a;
  }
  b += a;
  const bool diag_mom = mom_on && a == b;
  const c128* ps = chi + (size_t)blockIdx.z * bstride;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const unsigned stride = gridDim.x * OBS_BLOCK;
  for (unsigned p = blockIdx.x * OBS_BLOCK + threadIdx.x; p < npts; p += stride) {
    const c128 ca = ps[(size_t)p * ns + a], cb = ps[(size_t)p * ns + b];
    const double re = ca.re * cb.re + ca.im * cb.im;
    acc[0] += re;
    acc[1] += ca.re * cb.im - ca.im * cb.re;
    if (diag_mom) {
      const unsigned q = p / n2, i = q / n1;
      acc[2] += x0[i] * re;
      acc[3] += x1[q - i * n1] * re;
      acc[4] += x2[p - q * n2] * re;
    }
  }
  __shared__ double sh[OBS_BLOCK / 64][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < 5; ++v) {
    const double s = wave_sum(acc[v]);
    if (lane == 0) sh[wave][v] = s;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    double s = sh[0][threadIdx.x];
    for (int w = 1; w < OBS_BLOCK / 64; ++w) s += sh[w][threadIdx.x];
    double* row = part + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * NV;
    const int NP = ns * (ns + 1) / 2;
    if (threadIdx.x < 2) row[2 * blockIdx.y + threadIdx.x] = s;
    else if (diag_mom) row[2 * NP + (threadIdx.x - 2) * ns + a] = s;
  }
}

// Sums the G partial rows of member blockIdx.x in index order and writes its outputs: 256 / NV groups of threads each
// sum a contiguous chunk of rows in order, then the chunk sums are added in chunk order (NV >= 256: one group).
__global__ __launch_bounds__(OBS_BLOCK) void spo_obs_final_kernel(const double* __restrict__ part, int G, int NV,
                                                                  int ns, int ndim, double w, double* __restrict__ rdm,
                                                                  size_t rdm_bstride, double* __restrict__ mom,
                                                                  size_t mom_bstride) {
  __shared__ double sh[OBS_BLOCK];
  const double* rows = part + (size_t)blockIdx.x * G * NV;
  const int groups = NV < OBS_BLOCK ? OBS_BLOCK / NV : 1;
  const int chunk = (G + groups - 1) / groups;
  const int g = groups > 1 ? (int)threadIdx.x / NV : 0;
  const int NP = ns * (ns + 1) / 2;
  double* R = rdm + 2 * (size_t)blockIdx.x * rdm_bstride;
  double* Mo = mom ? mom + (size_t)blockIdx.x * mom_bstride : nullptr;
  for (int v = groups > 1 ? (int)threadIdx.x % NV : (int)threadIdx.x; v < NV; v += OBS_BLOCK) {
    double s = 0.0;
    if (g < groups) {
      const int r1 = min(G, (g + 1) * chunk);
      for (int r = g * chunk; r < r1; ++r) s += rows[(size_t)r * NV + v];
    }
    if (groups > 1) {   // uniform over the block: the loop body runs once for every thread
      sh[threadIdx.x] = s;
      __syncthreads();
      if (g != 0) break;
      for (int k = 1; k < groups; ++k) s += sh[k * NV + v];
    }
    s *= w;
    if (v < 2 * NP) {
      int a = 0, b = v >> 1;
      while (b >= ns - a) {
        b -= ns - a;
        ++a;
      }
      b += a;
      if (!(v & 1)) {
        R[2 * (a * ns + b)] = s;
        if (a != b) R[2 * (b * ns + a)] = s;
      } else if (a == b) {
        R[2 * (a * ns + a) + 1] = 0.0;
      } else {
        R[2 * (a * ns + b) + 1] = s;
        R[2 * (b * ns + a) + 1] = -s;
      }
    } else if (Mo) {
      const int m = v - 2 * NP;   // d ns + a
      if (m < ndim * ns) Mo[m] = s;
    }
  }
}

template <int NS>
void launch_reg(bool basis, bool mom, dim3 grid, hipStream_t st, const c128* psi, size_t bstride, const c128* M,
                unsigned npts, unsigned n1, unsigned n2, const double* x0, const double* x1, const double* x2,
                double* part) {
  if (basis && mom)
    hipLaunchKernelGGL((spo_obs_reg_kernel<NS, true, true>), grid, dim3(OBS_BLOCK), 0, st, psi, bstride, M, npts, n1, n2,
                       x0, x1, x2, part);
  else if (basis)
    hipLaunchKernelGGL((spo_obs_reg_kernel<NS, true, false>), grid, dim3(OBS_BLOCK), 0, st, psi, bstride, M, npts, n1,
                       n2, x0, x1, x2, part);
  else if (mom)
    hipLaunchKernelGGL((spo_obs_reg_kernel<NS, false, true>), grid, dim3(OBS_BLOCK), 0, st, psi, bstride, M, npts, n1,
                       n2, x0, x1, x2, part);
  else
    hipLaunchKernelGGL((spo_obs_reg_kernel<NS, false, false>), grid, dim3(OBS_BLOCK), 0, st, psi, bstride, M, npts, n1,
                       n2, x0, x1, x2, part);
}

}  // namespace

int SpoObserver::prepare(hipStream_t st) {
  npts = 1;
  for (int d = 0; d < ndim; ++d) npts *= dims[d];
  const bool reg = ns <= 4;
  note_path(reg ? "spo_obs_reg" : "spo_obs_gen");
  G = (int)std::max<long>(1, std::min<long>((npts + OBS_BLOCK - 1) / OBS_BLOCK, reg ? OBS_MAX_GRID : OBS_GEN_GRID));
  NV = ns * (ns + 1) + (mom ? 3 * ns : 0);
  const size_t part_bytes = ((size_t)B * G * NV * sizeof(double) + 15) & ~(size_t)15;
  const size_t chi_bytes = (!reg && basis) ? (size_t)B * npts * ns * sizeof(c128) : 0;
  void* w = nullptr;
  QD_TRY(workspace(WS_SPO, part_bytes + chi_bytes, &w, st));
  part = (double*)w;
  chi = chi_bytes ? (c128*)((char*)w + part_bytes) : nullptr;
  return QD_OK;
}

int SpoObserver::launch(const c128* psi, size_t psi_bstride, int rec, hipStream_t st) const {
  // axes past ndim have one point: any valid pointer serves, and the final pass drops their columns
  const unsigned n1 = ndim >= 2 ? dims[1] : 1, n2 = ndim >= 3 ? dims[2] : 1;
  const double* x0 = x[0];
  const double* x1 = ndim >= 2 ? x[1] : x[0];
  const double* x2 = ndim >= 3 ? x[2] : x[0];
  if (ns <= 4) {
    const dim3 grid(G, B);
#define OBS_REG(NS) \
  launch_reg<NS>(basis != nullptr, mom != nullptr, grid, st, psi, psi_bstride, basis, (unsigned)npts, n1, n2, x0, x1, x2, part)
    if (ns == 1) OBS_REG(1);
    else if (ns == 2) OBS_REG(2);
    else if (ns == 3) OBS_REG(3);
    else OBS_REG(4);
#undef OBS_REG
  } else {
    const c128* src = psi;
    size_t bs = psi_bstride;
    if (basis) {
      const size_t nel = (size_t)npts * ns;
      hipLaunchKernelGGL(spo_obs_chi_kernel, dim3((unsigned)std::min<size_t>((nel + 255) / 256, 4096), B), dim3(256), 0,
                         st, psi, psi_bstride, basis, nel, ns, chi);
      QD_HIP(hipGetLastError());
      src = chi;
      bs = nel;
    }
    hipLaunchKernelGGL(spo_obs_gen_kernel, dim3(G, ns * (ns + 1) / 2, B), dim3(OBS_BLOCK), 0, st, src, bs,
                       (unsigned)npts, ns, n1, n2, x0, x1, x2, mom ? 1 : 0, part, NV);
  }
  QD_HIP(hipGetLastError());
  hipLaunchKernelGGL(spo_obs_final_kernel, dim3(B), dim3(OBS_BLOCK), 0, st, (const double*)part, G, NV, ns, ndim, weight,
                     (double*)(rdm + (size_t)rec * ns * ns), rdm_bstride,
                     mom ? mom + (size_t)rec * ndim * ns : (double*)nullptr, mom_bstride);
  QD_HIP(hipGetLastError());
  return QD_OK;
}

// Argument checks shared by qd_spo_observe and the observed runs (before any HIP call)
int spo_observer_check(const char* who, const int* dims, int ndim, int ns, long B, const double* const x[3],
                       const void* rdm, const void* mom) {
  QD_CHECK_ARG(rdm, "%s: null rdm", who);
  QD_CHECK_ARG(ndim >= 1 && ndim <= 3, "%s: ndim=%d outside [1, 3]", who, ndim);
  QD_CHECK_ARG(dims, "%s: null dims", who);
  QD_CHECK_ARG(ns >= 1 && ns <= 1024, "%s: ns=%d outside [1, 1024]", who, ns);
  QD_CHECK_ARG(B >= 1 && B <= 65535, "%s: B=%ld outside [1, 65535]", who, B);
  long npts = 1;
  for (int d = 0; d < ndim; ++d) {
    QD_CHECK_ARG(dims[d] >= 1, "%s: dims[%d]=%d", who, d, dims[d]);
    QD_CHECK_ARG(npts <= ((long)1 << 31) / dims[d], "%s: more than 2^31 grid points", who);
    npts *= dims[d];
  }
  QD_CHECK_ARG(npts < ((long)1 << 31), "%s: more than 2^31 - 1 grid points", who);
  QD_CHECK_ARG((long)ns * (ns + 1) / 2 <= 65535, "%s: ns=%d has too many state pairs", who, ns);
  if (mom)
    for (int d = 0; d < ndim; ++d) QD_CHECK_ARG(x[d], "%s: mom needs the axis of dimension %d (null)", who, d);
  return QD_OK;
}

}  // namespace qd

using namespace qd;

extern "C" int qd_spo_observe(const qd_c128* psi, long B, const int* dims, int ndim, int ns, const qd_c128* basis,
                              const double* x0, const double* x1, const double* x2, double weight, qd_c128* rdm,
                              double* mom, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  WsScope wss_(st);  // call-scoped scratch (qd_runtime.hip)
  QD_CHECK_ARG(psi, "qd_spo_observe: null psi");
  const double* const x[3] = {x0, x1, x2};
  QD_TRY(spo_observer_check("qd_spo_observe", dims, ndim, ns, B, x, rdm, mom));
  SpoObserver o;
  o.ndim = ndim;
  for (int d = 0; d < ndim; ++d) {
    o.dims[d] = dims[d];
    o.x[d] = x[d];
  }
  o.ns = ns;
  o.B = (int)B;
  o.basis = (const c128*)basis;
  o.weight = weight;
  o.rdm = (c128*)rdm;
  o.mom = mom;
  o.rdm_bstride = (size_t)ns * ns;
  o.mom_bstride = (size_t)ndim * ns;
  QD_TRY(o.prepare(st));
  return o.launch((const c128*)psi, (size_t)o.npts * ns, 0, st);
}
