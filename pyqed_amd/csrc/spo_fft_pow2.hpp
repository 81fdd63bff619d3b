// spo_fft_pow2.hpp — the power-of-two transforms shared by spo.hip and fft.hip (device code, included into each
// translation unit): the twiddle table exp(-2 pi i k/L), the Stockham autosort FFT on LDS (radix-4 stages + one
// radix-2 stage when log2 L is odd, L in [16, 1024], natural-order output), the 256-point transform on one wave
// (16 x 16 in registers) and the 64-point transform on 16 lanes.  Unnormalised; INV conjugates the twiddles.
#pragma once

#include "qd_common.hpp"

namespace qd {
namespace {

__global__ void twiddle_kernel(int L, c128* tw) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < L; k += gridDim.x * blockDim.x) {
    double s, c;
    sincospi(-2.0 * (double)k / (double)L, &s, &c);
    tw[k] = cmk(c, s);
  }
}

// Stockham FFT of length L on LDS buffers a/b (one transform), T = L/4 threads,
// thread index t in [0, T).  All threads of the workgroup must call it (barriers).
// Returns the buffer holding the result.  INV: conjugated twiddles, no scaling.
template <int L, bool INV>
__device__ __forceinline__ c128* fft_lds(c128* a, c128* b, const c128* tw, int t, bool active) {
#pragma unroll
  for (int Ns = 1; Ns * 4 <= L; Ns *= 4) {
    if (active) {
      const int j = t;
      const int k = j % Ns;
      const int base = k * (L / (4 * Ns));
      c128 w1 = tw[base], w2 = tw[2 * base], w3 = tw[3 * base];
      if (INV) {
        w1 = cconj(w1);
        w2 = cconj(w2);
        w3 = cconj(w3);
      }
      const c128 v0 = a[j];
      const c128 v1 = cmul(a[j + L / 4], w1);
      const c128 v2 = cmul(a[j + L / 2], w2);
      const c128 v3 = cmul(a[j + 3 * L / 4], w3);
      const c128 a0 = cadd(v0, v2), a1 = csub(v0, v2), b0 = cadd(v1, v3), b1 = csub(v1, v3);
      const c128 ib1 = INV ? cmuli(b1) : cmulmi(b1);  // (+i or -i) * b1
      const int d = (j / Ns) * Ns * 4 + k;
      b[d] = cadd(a0, b0);
      b[d + Ns] = cadd(a1, ib1);
      b[d + 2 * Ns] = csub(a0, b0);
      b[d + 3 * Ns] = csub(a1, ib1);
    }
    __syncthreads();
    c128* tmp = a;
    a = b;
    b = tmp;
  }
  constexpr int lg = __builtin_ctz(L);
  if (lg & 1) {  // final radix-2 stage, Ns = L/2
    if (active) {
      constexpr int Ns = L / 2;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = t + h * (L / 4);
        const int k = j % Ns;
        c128 w = tw[k];
        if (INV) w = cconj(w);
        const c128 v0 = a[j], v1 = cmul(a[j + L / 2], w);
        const int d = (j / Ns) * Ns * 2 + k;
        b[d] = cadd(v0, v1);
        b[d + Ns] = csub(v0, v1);
      }
    }
    __syncthreads();
    c128* tmp = a;
    a = b;
    b = tmp;
  }
  return a;
}

// ---------------------------------------------------------------- 256-point passes in registers
// L = 256 = 16 x 16 (Cooley-Tukey, n = 16 n1 + n2, k = k1 + 16 k2):
//   X[k1 + 16 k2] = sum_n2 w16^(n2 k2) w256^(n2 k1) sum_n1 x[16 n1 + n2] w16^(n1 k1)
// ONE wave per transform set.  Lane (g, s) = (lane >> 2, lane & 3) holds the points
// p_a = 64 a + 16 s + g (a = 0..3) of its line, before and after every transform: an inverse FFT,
// point-local work and a forward FFT chain with no data movement.  Each 16-point DFT runs inside
// a quad (4 x 4: DFT4 in registers, three quad-DPP rotations, DFT4); the two 16-point steps
// exchange through LDS once.  Per pass: one global load round trip, two wave-local LDS
// transposes per FFT, no workgroup-wide barrier (the Stockham LDS FFT takes 4 barrier stages per
// transform plus the staging).  w = exp(-2 pi i / L) forward, its conjugate inverse; no scaling.
template <bool ZPOS>  // y[r] = sum_a x[a] z^(a r), z = +i (ZPOS) or -i
__device__ __forceinline__ void dft4(c128 (&x)[4]) {
  const c128 s02 = cadd(x[0], x[2]), d02 = csub(x[0], x[2]);
  const c128 s13 = cadd(x[1], x[3]), d13 = csub(x[1], x[3]);
  const c128 zd = ZPOS ? cmuli(d13) : cmulmi(d13);
  x[0] = cadd(s02, s13);
  x[1] = cadd(d02, zd);
  x[2] = csub(s02, s13);
  x[3] = csub(d02, zd);
}

struct Q16Tw {
  c128 a[4];  // w4^(a s)            (pre-rotation of the inputs, also the final w4^(s d))
  c128 b[4];  // w16^(s ((s - r) & 3))  (inner twiddle of the sent element r)
  c128 d[4];  // w256^(g (s + 4 d))  (inter-step twiddle of output k1 = s + 4 d)
};

__device__ __forceinline__ Q16Tw q16_twiddles(const c128* tw, int g, int s) {
  Q16Tw t;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    t.a[q] = tw[64 * ((q * s) & 3)];
    t.b[q] = tw[16 * ((s * ((s - q) & 3)) & 15)];
    t.d[q] = tw[(g * (s + 4 * q)) & 255];
  }
  return t;
}

__device__ __forceinline__ c128 twmul(c128 v, c128 w, bool inv) { return cmul(v, inv ? cconj(w) : w); }

// 16-point DFT of the quad: lane s holds v[a] = x[4 a + s]; on return lane s holds X[s + 4 d] in v[d].
template <bool INV>
__device__ __forceinline__ void dft16_quad(c128 (&v)[4], const Q16Tw& t) {
  // U_s[(s - r) & 3] = sum_a (v[a] w4^(a s)) w4^(-a r): pre-rotate, DFT4 with root w4^-1
#pragma unroll
  for (int a = 1; a < 4; ++a) v[a] = twmul(v[a], t.a[a], INV);
  dft4<!INV>(v);
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = twmul(v[r], t.b[r], INV);
  // lane l receives element r of lane (l + r) & 3: R_r = U_b[l] w16^(b l), b = (l + r) & 3
  v[1] = dpp_qc<0x39>(v[1]);
  v[2] = dpp_qc<0x4E>(v[2]);
  v[3] = dpp_qc<0x93>(v[3]);
  // X[l + 4 d] = w4^(l d) sum_r w4^(r d) R_r
  dft4<INV>(v);
#pragma unroll
  for (int d = 1; d < 4; ++d) v[d] = twmul(v[d], t.a[d], INV);
}

// 256-point FFT of NS lines held in the wave's layout; S: NS x 16 x 17 c128 of LDS (this wave's).
template <bool INV, int NS>
__device__ __forceinline__ void fft256_wave(c128 (&x)[NS][4], const Q16Tw& t, c128* S, int g, int s) {
#pragma unroll
  for (int c = 0; c < NS; ++c) {
    dft16_quad<INV>(x[c], t);
#pragma unroll
    for (int d = 0; d < 4; ++d) S[c * 272 + (s + 4 * d) * 17 + g] = twmul(x[c][d], t.d[d], INV);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int c = 0; c < NS; ++c) {
#pragma unroll
    for (int a = 0; a < 4; ++a) x[c][a] = S[c * 272 + g * 17 + 4 * a + s];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int c = 0; c < NS; ++c) dft16_quad<INV>(x[c], t);
}

// ---------------------------------------------------------------- 64-point transforms on 16 lanes
// L = 64 = 4 x 16 (n = 4 m + q, k = k1 + 16 k2):
//   X[k1 + 16 k2] = sum_q w4^(q k2) [w64^(q k1) X_q[k1]],  X_q = 16-point DFT of x[4 m + q]
// A group of 16 lanes (lane l = 4 qq + s of the group) transforms one line held in LDS (any stride):
// quad qq runs the 16-point DFT of x[4 m + qq] (dft16_quad: lane s loads x[16 a + 4 s + qq]), scales output
// k1 = s + 4 d by w64^(qq k1), the 64 values are exchanged through the line's own storage (slot 4 k1 + q),
// and lane l finishes X[l + 16 k2] (k2 = 0..3) with one register DFT4.  Returns the result in v (natural order
// X[l + 16 k2] in v[k2]); the line's storage holds exchange values afterwards.  Twiddles t = q64_twiddles of the
// 64-entry table w64^k (they depend on the lane only).  INV: conjugated twiddles, no scaling.
__device__ __forceinline__ Q16Tw q64_twiddles(const c128* tw, int qq, int s) {
  Q16Tw t;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    t.a[q] = tw[16 * ((q * s) & 3)];
    t.b[q] = tw[4 * ((s * ((s - q) & 3)) & 15)];
    t.d[q] = tw[(qq * (s + 4 * q)) & 63];
  }
  return t;
}

// The transform from registers already in the input layout (v[a] = x[16 a + 4 s + qq]); `line` is exchange space.
template <bool INV>
__device__ __forceinline__ void fft64_regs(c128* line, int stride, const Q16Tw& t, int qq, int s, c128 (&v)[4]) {
  dft16_quad<INV>(v, t);
#pragma unroll
  for (int d = 0; d < 4; ++d) v[d] = twmul(v[d], t.d[d], INV);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int d = 0; d < 4; ++d) line[(4 * (s + 4 * d) + qq) * stride] = v[d];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int l = 4 * qq + s;
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = line[(4 * l + q) * stride];
  dft4<INV>(v);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool INV>
__device__ __forceinline__ void fft64_group(c128* line, int stride, const Q16Tw& t, int qq, int s, c128 (&v)[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) v[a] = line[(16 * a + 4 * s + qq) * stride];
  fft64_regs<INV>(line, stride, t, qq, s, v);
}

}  // namespace
}  // namespace qd
