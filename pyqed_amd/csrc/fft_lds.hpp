// fft_lds.hpp — the any-length transform of the any-size engine on lines held in LDS (spo_gen_kernels.hpp): the plan
// of one axis as the kernels take it by value (Fft, filled from fft_plan.hpp's AxisPlan and the table pointer), the
// arguments of one fused pass (AxisArgs), the mixed-radix Stockham stages and the Bluestein wrapper around them.
#pragma once

#include "fft_plan.hpp"
#include "qd_common.hpp"

namespace qd {
namespace spog {

struct Fft {           // device-side plan of one axis, passed by value
  int L, M, kind, nst;
  int R[MAX_ST];
  int Ns[MAX_ST];
  FDiv dnb[MAX_ST];    // M / R[s]
  FDiv dns[MAX_ST];    // Ns[s]
  FDiv dM;             // M
  const c128* tw;      // exp(-2 pi i m / M), m < M (DIRECT: M = L)
  const c128* chirp;   // BLUESTEIN: exp(-pi i n^2 / L), n < L
  const c128* bhat;    // BLUESTEIN: (1/M) FFT_M(b), b_m = conj(c_|m|) wrapped
};

struct AxisArgs {
  c128* psi;           // tile source
  c128* out;           // tile destination (psi: in place; F_XOUT: the other layout's buffer)
  long sh, sl, se;     // F_XOUT strides of hi, lo, e
  FDiv dlo;            // F_XOUT: division by nlo
  int O, L, I, C, G, flags, ns;
  FDiv dLC, dC, dLns, dns;   // L C, C, L ns, ns
  int twl;             // 1: twiddles staged in LDS (M more c128 of dynamic LDS)
  const c128* U1;      // [points][ns][ns] (F_PT1)
  const c128* U2;      // (F_PT2)
  c128* snap;          // (F_SNAP) same layout as psi
  const c128* K;       // (F_KMUL) exp_K / N over the grid points, [L][I / ns]
  const c128* Ky;      // (F_KY) [O][L]
};

// ---------------------------------------------------------------- device FFT
// One Stockham stage over nl lines of length M: butterfly j of a line reads src[j + r M/R] (r < R) times
// tw^(r k M/(Ns R)), k = j mod Ns, and writes the R-point DFT to dst[(j / Ns) Ns R + k + q Ns].
template <bool INV, int R0>   // R0 = 2, 3, 4, 5, 8: closed-form butterflies; 0: any prime R <= GEN_MAXP
__device__ __forceinline__ void stage(const c128* __restrict__ src, c128* __restrict__ dst, int nl, int M, int Rr,
                                      int Ns, FDiv dnb, FDiv dns, const c128* __restrict__ tw) {
  const int R = R0 ? R0 : Rr;
  const int nb = M / R;
  const int tot = nl * nb;
  const int tstep = M / (Ns * R);
  for (int f = threadIdx.x; f < tot; f += blockDim.x) {
    const int l = (int)fdiv((unsigned)f, dnb), j = f - l * nb;
    const c128* s = src + (size_t)l * M;
    c128* d = dst + (size_t)l * M;
    const int jq = (int)fdiv((unsigned)j, dns);
    const int k = j - jq * Ns;
    const int db = jq * Ns * R + k;
    auto ld = [&](int r) {
      const c128 x = s[j + r * nb];
      if (r == 0 || k == 0) return x;
      c128 w = tw[r * k * tstep];
      if (INV) w = cconj(w);
      return cmul(x, w);
    };
    if constexpr (R0 == 8) {   // DFT8 = DFT4 of the even and of the odd inputs, combined with w8^k
      const c128 x0 = ld(0), x1 = ld(1), x2 = ld(2), x3 = ld(3), x4 = ld(4), x5 = ld(5), x6 = ld(6), x7 = ld(7);
      auto mj = [](c128 v) { return INV ? cmuli(v) : cmulmi(v); };   // times -+ i
      const c128 a0 = cadd(x0, x4), a1 = csub(x0, x4), a2 = cadd(x2, x6), a3 = mj(csub(x2, x6));
      const c128 b0 = cadd(x1, x5), b1 = csub(x1, x5), b2 = cadd(x3, x7), b3 = mj(csub(x3, x7));
      const c128 e0 = cadd(a0, a2), e2 = csub(a0, a2), e1 = cadd(a1, a3), e3 = csub(a1, a3);
      c128 o0 = cadd(b0, b2), o2 = csub(b0, b2), o1 = cadd(b1, b3), o3 = csub(b1, b3);
      const double h = 0.70710678118654752440;   // 1 / sqrt(2)
      // o1 w8, o2 w8^2 = -+ i, o3 w8^3 with w8 = (1 -+ i) / sqrt(2)
      o1 = INV ? cmk((o1.re - o1.im) * h, (o1.re + o1.im) * h) : cmk((o1.re + o1.im) * h, (o1.im - o1.re) * h);
      o2 = mj(o2);
      o3 = INV ? cmk(-(o3.re + o3.im) * h, (o3.re - o3.im) * h) : cmk((o3.im - o3.re) * h, -(o3.re + o3.im) * h);
      d[db] = cadd(e0, o0);
      d[db + Ns] = cadd(e1, o1);
      d[db + 2 * Ns] = cadd(e2, o2);
      d[db + 3 * Ns] = cadd(e3, o3);
      d[db + 4 * Ns] = csub(e0, o0);
      d[db + 5 * Ns] = csub(e1, o1);
      d[db + 6 * Ns] = csub(e2, o2);
      d[db + 7 * Ns] = csub(e3, o3);
    } else if constexpr (R0 == 4) {
      const c128 x0 = ld(0), x1 = ld(1), x2 = ld(2), x3 = ld(3);
      const c128 a0 = cadd(x0, x2), a1 = csub(x0, x2), b0 = cadd(x1, x3), b1 = csub(x1, x3);
      const c128 ib1 = INV ? cmuli(b1) : cmulmi(b1);
      d[db] = cadd(a0, b0);
      d[db + Ns] = cadd(a1, ib1);
      d[db + 2 * Ns] = csub(a0, b0);
      d[db + 3 * Ns] = csub(a1, ib1);
    } else if constexpr (R0 == 2) {
      const c128 x0 = ld(0), x1 = ld(1);
      d[db] = cadd(x0, x1);
      d[db + Ns] = csub(x0, x1);
    } else if constexpr (R0 == 3) {
      const double c = -0.5, sn = 0.86602540378443864676;   // cos, sin(2 pi / 3)
      const c128 x0 = ld(0), x1 = ld(1), x2 = ld(2);
      const c128 t = cadd(x1, x2), u = csub(x1, x2);
      const c128 a = cadd(x0, cscale(t, c));
      const c128 b = INV ? cmuli(cscale(u, sn)) : cmulmi(cscale(u, sn));   // -+ i s (x1 - x2)
      d[db] = cadd(x0, t);
      d[db + Ns] = cadd(a, b);
      d[db + 2 * Ns] = csub(a, b);
    } else if constexpr (R0 == 5) {
      const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;   // cos(2 pi/5), cos(4 pi/5)
      const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;    // sin(2 pi/5), sin(4 pi/5)
      const c128 x0 = ld(0), x1 = ld(1), x2 = ld(2), x3 = ld(3), x4 = ld(4);
      const c128 t1 = cadd(x1, x4), t2 = cadd(x2, x3), t3 = csub(x1, x4), t4 = csub(x2, x3);
      const c128 a1 = cadd(x0, cadd(cscale(t1, c1), cscale(t2, c2)));
      const c128 a2 = cadd(x0, cadd(cscale(t1, c2), cscale(t2, c1)));
      const c128 b1r = cadd(cscale(t3, s1), cscale(t4, s2));
      const c128 b2r = csub(cscale(t3, s2), cscale(t4, s1));
      const c128 b1 = INV ? cmuli(b1r) : cmulmi(b1r), b2 = INV ? cmuli(b2r) : cmulmi(b2r);
      d[db] = cadd(x0, cadd(t1, t2));
      d[db + Ns] = cadd(a1, b1);
      d[db + 4 * Ns] = csub(a1, b1);
      d[db + 2 * Ns] = cadd(a2, b2);
      d[db + 3 * Ns] = csub(a2, b2);
    } else {  // any prime R <= GEN_MAXP: y_q = sum_r x_r w_R^(r q), w_R^m = tw[m M/R]
      for (int q = 0; q < R; ++q) {
        c128 acc = cmk(0.0, 0.0);
        int e = 0;  // r q mod R
        for (int r = 0; r < R; ++r) {
          c128 w = tw[e * nb];
          if (INV) w = cconj(w);
          acc = cadd(acc, cmul(ld(r), w));
          e += q;
          if (e >= R) e -= R;
        }
        d[db + q * Ns] = acc;
      }
    }
  }
}
template <bool INV>
__device__ __forceinline__ void stockham(const Fft& p, const c128* tw, c128*& cur, c128*& oth, int nl, int M) {
  for (int s = 0; s < p.nst; ++s) {
    const int R = p.R[s], Ns = p.Ns[s];
    const FDiv dnb = p.dnb[s], dns = p.dns[s];   // copies: a reference would put the plan in scratch
    switch (R) {   // wave-uniform: one branch-free element loop per radix
      case 8: stage<INV, 8>(cur, oth, nl, M, 8, Ns, dnb, dns, tw); break;
      case 4: stage<INV, 4>(cur, oth, nl, M, 4, Ns, dnb, dns, tw); break;
      case 2: stage<INV, 2>(cur, oth, nl, M, 2, Ns, dnb, dns, tw); break;
      case 3: stage<INV, 3>(cur, oth, nl, M, 3, Ns, dnb, dns, tw); break;
      case 5: stage<INV, 5>(cur, oth, nl, M, 5, Ns, dnb, dns, tw); break;
      default: stage<INV, 0>(cur, oth, nl, M, R, Ns, dnb, dns, tw); break;
    }
    __syncthreads();
    c128* t = cur;
    cur = oth;
    oth = t;
  }
}

// Length-L DFT (INV: conjugate kernel, no scaling) of nl lines held in the first L slots of each M-slot
// line of cur.  Result in cur (first L slots).
template <bool INV>
__device__ __forceinline__ void lds_fft(const Fft& p, const c128* tw, c128*& cur, c128*& oth, int nl) {
  const int M = p.M, L = p.L;
  if (p.kind == BLUESTEIN) {
    const int tot = nl * M;
    for (int f = threadIdx.x; f < tot; f += blockDim.x) {
      const int n = f - (int)fdiv((unsigned)f, p.dM) * M;
      c128 v = cmk(0.0, 0.0);
      if (n < L) {
        c128 ch = p.chirp[n];
        if (INV) ch = cconj(ch);
        v = cmul(cur[f], ch);
      }
      cur[f] = v;
    }
    __syncthreads();
    stockham<false>(p, tw, cur, oth, nl, M);
    for (int f = threadIdx.x; f < tot; f += blockDim.x) {
      c128 b = p.bhat[f - (int)fdiv((unsigned)f, p.dM) * M];
      if (INV) b = cconj(b);
      cur[f] = cmul(cur[f], b);
    }
    __syncthreads();
    stockham<true>(p, tw, cur, oth, nl, M);
    for (int f = threadIdx.x; f < tot; f += blockDim.x) {
      const int n = f - (int)fdiv((unsigned)f, p.dM) * M;
      if (n < L) {
        c128 ch = p.chirp[n];
        if (INV) ch = cconj(ch);
        cur[f] = cmul(cur[f], ch);
      }
    }
    __syncthreads();
  } else {
    stockham<INV>(p, tw, cur, oth, nl, M);
  }
}

}  // namespace spog
}  // namespace qd
