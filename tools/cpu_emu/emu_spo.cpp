// Host build of spo_gen.hip (with fft_plan.hpp, fft_lds.hpp and spo_gen_kernels.hpp) through the flat-loop emulation
// shim (tools/cpu_emu/hip/hip_runtime.h), for tests/test_fft_engine_host.py, tests/test_spo_gen_host.py and
// tools/cpu_emu/emu_bits.py.
#include <vector>
#include <cstdarg>
#include "hip/hip_runtime.h"
thread_local emu_dim3 threadIdx, blockIdx, blockDim, gridDim;
#include "../../pyqed_amd/csrc/spo_gen.hip"

namespace qd {
static thread_local std::vector<void*> g_bufs;
void set_error(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fprintf(stderr, "\n");
}
WsScope::WsScope(hipStream_t s) : st(s), mark(g_bufs.size()) {}
WsScope::~WsScope() { while (g_bufs.size() > mark) { free(g_bufs.back()); g_bufs.pop_back(); } }
int workspace(WsSlot, size_t bytes, void** ptr, hipStream_t) { *ptr = calloc(1, bytes + 16); g_bufs.push_back(*ptr); return 0; }
void note_path(const char*) {}
int copy_device(void* dst, const void* src, size_t n, hipStream_t) { memmove(dst, src, n); return 0; }
int SpoObserver::launch(const c128*, size_t, int, hipStream_t) const { return 0; }   // no observer in the emulation
}
namespace qd { namespace spog { c128 sm[163840 / 16]; } }
extern "C" {
int emu_spo_nd(void* psi, const void* Uh, const void* Uf, const void* K, const void* Ky, const int* dims, int D, int ns,
               int nsteps, int nout, void* snap) {
  qd::SnapSink sink;   // the caller's snapshots, no observer: what the plain entry points pass
  sink.snap = (qd::c128*)snap;
  sink.grid_elems = (size_t)ns;
  for (int d = 0; d < D; ++d) sink.grid_elems *= (size_t)dims[d];
  return qd::spo_generic_run((qd::c128*)psi, (const qd::c128*)Uh, (const qd::c128*)Uf, (const qd::c128*)K,
                             (const qd::c128*)Ky, dims, D, ns, nsteps, nout, sink, nullptr);
}
int emu_spo1d(void* psi, const void* eV, const void* eVh, const void* eK, int nx, int B, int nt, int nout, void* snap) {
  return qd::spo1d_generic_run((qd::c128*)psi, (const qd::c128*)eV, (const qd::c128*)eVh, (const qd::c128*)eK, nx, B,
                               nt, nout, (qd::c128*)snap, nullptr);
}
// fft_lines on the [O][L][I] array x in place (call-scoped scratch as qd_fft_axis opens it); *l2 != 0: four-step slot
// order, X[k] at (k % L1) * L2 + k / L1 with L1 = L / L2
int emu_fft_lines(void* x, long O, int L, long I, int inv, int* l2) {
  qd::WsScope wss_(nullptr);
  return qd::fft_lines((qd::c128*)x, O, L, I, inv != 0, nullptr, l2);
}
}
