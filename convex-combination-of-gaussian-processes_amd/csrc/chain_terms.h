// The log-posterior terms of one transformed parameter vector -- logpost_terms of capi.hip -- restated so that the host and
// the device compute THE SAME BITS: the Metropolis chain that runs inside small_reg_kernel<.., CHAIN> forms them in the
// kernel, and its host twin (ccgp_chain_logpost_sets, ccgp_chain_terms) must reproduce every accept / reject decision.
// glibc's exp and log have no device counterpart with their bits, so exp and log are written here from operations IEEE 754
// defines exactly -- add, multiply, divide (see below), explicit fma, and bit assembly -- with contraction off inside every
// function (the pragma is function-local: a file-scope one would change the kernels of whatever includes this).
//   chain_exp: x = (256 m + j) ln 2 / 256 + r, |r| <= ln 2 / 512; exp(x) = 2^m (hi_j + (lo_j + hi_j (e^r - 1))) with
//     hi_j + lo_j = 2^(j/256) to 2^-106 (exp_table.h, chain_exp_lo.h) and a degree-5 polynomial for e^r - 1 (truncation
//     r^6 / 720 < 1e-20): one rounding of the final sum, 0.5 ulp + 0.003.  NaN stays NaN, x > 1000 (+Inf) gives +Inf,
//     x < -1000 (-Inf) gives 0, and the scaling by 2^m is two multiplications by powers of two, so overflow and the
//     subnormal range round as IEEE multiplication does.
//   chain_log: fdlibm's e_log.c (argument reduced to [sqrt 1/2, sqrt 2), s = f / (2 + f), degree-14 even polynomial), < 1 ulp.
// The sums keep logpost_terms' order of operations, divisions included (1 / theta, 4 / lambda, 1 / (1 + e^-phi)), and
// chain_log divides once (s = f / (2 + f)).  fp64 division is an exactly rounded operation on the host and, under this
// project's flags, on the device (the div_scale / div_fmas / div_fixup sequence): the Makefile compiles without -ffast-math
// and without -fno-honor-*; a build that relaxes division (fast math, -freciprocal-math) would break the host / device
// agreement, and tests/test_gpu_chains.py would show it.  Plain C++ apart from the __host__ __device__ marks.
#pragma once

#include "../../include/ccgp.h"
#include "chain_exp_lo.h"
#include "exp_table.h"

#if defined(__HIPCC__)
#define CCGP_CHAIN_HD __host__ __device__
#else
#define CCGP_CHAIN_HD
#endif

namespace ccgp {

constexpr int kChainTable = 256;   // entries of each of the two tables (hi, lo)

CCGP_CHAIN_HD inline double chain_from_bits(unsigned long long b) {
  double v;
  __builtin_memcpy(&v, &b, sizeof v);
  return v;
}
CCGP_CHAIN_HD inline unsigned long long chain_bits(double v) {
  unsigned long long b;
  __builtin_memcpy(&b, &v, sizeof b);
  return b;
}

// thi / tlo: the two tables as doubles (the kernel keeps them in LDS, the host in a static array)
CCGP_CHAIN_HD inline double chain_exp(double x, const double* thi, const double* tlo) {
#pragma clang fp contract(off)
  if (x > 1000.0) return chain_from_bits(0x7ff0000000000000ULL);
  if (x < -1000.0) return 0.0;
  const double kScale = chain_from_bits(0x40771547652b82feULL);     // 256 / ln 2
  const double kNegCHi = chain_from_bits(0xbf662e42fe000000ULL);    // -(ln 2 / 256), 24 trailing zero bits: n * hi is exact
  const double kNegCLo = chain_from_bits(0xbd9f473de6af278fULL);
  const double kMagic = 6755399441055744.0;                         // 1.5 * 2^52: the low dword of t holds n
  const double c5 = chain_from_bits(0x3f81111111111111ULL), c4 = chain_from_bits(0x3fa5555555555555ULL),
               c3 = chain_from_bits(0x3fc5555555555555ULL);
  const double t = __builtin_fma(x, kScale, kMagic);
  const double nf = t - kMagic;
  const int n = (int)(unsigned)(chain_bits(t) & 0xffffffffULL);     // a NaN leaves any n: every path below keeps the NaN
  double r = __builtin_fma(kNegCHi, nf, x);
  r = __builtin_fma(kNegCLo, nf, r);
  double p = __builtin_fma(r, c5, c4);
  p = __builtin_fma(r, p, c3);
  p = __builtin_fma(r, p, 0.5);
  p = __builtin_fma(r, p, 1.0);
  const double q = r * p;                                           // e^r - 1
  const int j = n & 255, m = n >> 8;                                // |m| <= 1443
  const double v = thi[j] + __builtin_fma(thi[j], q, tlo[j]);
  const int m1 = m / 2, m2 = m - m1;                                // 2^m1 and 2^m2 are normal numbers; v 2^m1 is exact
  const double s1 = chain_from_bits((unsigned long long)(1023 + m1) << 52);
  const double s2 = chain_from_bits((unsigned long long)(1023 + m2) << 52);
  return (v * s1) * s2;
}

CCGP_CHAIN_HD inline double chain_log(double x) {
#pragma clang fp contract(off)
  const double ln2_hi = chain_from_bits(0x3fe62e42fee00000ULL), ln2_lo = chain_from_bits(0x3dea39ef35793c76ULL);
  const double Lg1 = chain_from_bits(0x3fe5555555555593ULL), Lg2 = chain_from_bits(0x3fd999999997fa04ULL),
               Lg3 = chain_from_bits(0x3fd2492494229359ULL), Lg4 = chain_from_bits(0x3fcc71c51d8e78afULL),
               Lg5 = chain_from_bits(0x3fc7466496cb03deULL), Lg6 = chain_from_bits(0x3fc39a09d078c69fULL),
               Lg7 = chain_from_bits(0x3fc2f112df3e5244ULL);
  if (!(x > 0.0)) return x == 0.0 ? chain_from_bits(0xfff0000000000000ULL) : chain_from_bits(0x7ff8000000000000ULL);
  if (x == chain_from_bits(0x7ff0000000000000ULL)) return x;
  int k = 0;
  if (x < chain_from_bits(0x0010000000000000ULL)) { x = x * 18014398509481984.0; k = -54; }   // subnormal: scale by 2^54
  unsigned long long b = chain_bits(x);
  unsigned hx = (unsigned)(b >> 32);
  hx += 0x3ff00000u - 0x3fe6a09eu;
  k += (int)(hx >> 20) - 0x3ff;
  hx = (hx & 0x000fffffu) + 0x3fe6a09eu;
  b = ((unsigned long long)hx << 32) | (b & 0xffffffffULL);
  const double f = chain_from_bits(b) - 1.0;
  const double hfsq = 0.5 * f * f;
  const double s = f / (2.0 + f);
  const double z = s * s, w = z * z;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  const double R = t2 + t1, dk = k;
  return s * (hfsq + R) + dk * ln2_lo - hfsq + f + dk * ln2_hi;
}

// what logpost_terms gives for one vector theta (psi1, psi2, phi[, zeta]): the mixing weights w0 = p, w1 = 1 - p, the rates of
// the two components -- t[0], t[1] for component 1 and t[2], t[3] for component 2 in the anisotropic script (d = 2), else
// t[0] for every dimension of component 1 and t[2] of component 2 (t[1] = t[0], t[3] = t[2]) -- log-Jacobian and log-prior
struct ChainTerms {
  double w0, w1, t[4], lj, lp;
};
CCGP_CHAIN_HD inline ChainTerms chain_terms(int prior_id, const double* theta, const double* prior_pars, const double* thi,
                                            const double* tlo) {
#pragma clang fp contract(off)
  ChainTerms o;
  const double psi1 = theta[0], psi2 = theta[1], phi = theta[2];
  const double theta1 = chain_exp(psi1, thi, tlo), theta2 = chain_exp(psi2, thi, tlo);
  const double en = chain_exp(-phi, thi, tlo);
  const double p = 1.0 / (1.0 + en);
  o.w0 = p;
  o.w1 = 1.0 - p;
  double lj = -phi - 2.0 * chain_log(1.0 + en) + psi1 + psi2;
  double lp = 0.0;
  if (prior_id == CCGP_PRIOR_ANI) {
    const double zeta = theta[3], lambda = chain_exp(zeta, thi, tlo);
    o.t[0] = theta1; o.t[1] = theta2;
    o.t[2] = (1.0 + lambda) * theta1; o.t[3] = (1.0 + lambda) * theta2;
    lj += zeta;
    lp = -psi1 - psi1 * psi1 / 2.0 - psi2 - psi2 * psi2 / 2.0 - 4.0 * zeta - 4.0 / lambda;
  } else {
    o.t[0] = o.t[1] = theta1;
    o.t[2] = o.t[3] = theta2;
    if (prior_id == CCGP_PRIOR_INVGAMMA)
      lp = -(prior_pars[0] + 1.0) * psi1 - prior_pars[1] / theta1 -
           (prior_pars[2] + 1.0) * psi2 - prior_pars[3] / theta2;
    else if (prior_id == CCGP_PRIOR_GV)
      lp = -4.0 * psi1 - 1.0 / theta1 - 6.0 * psi2 - 75.0 / theta2;
    else
      lp = -4.0 * psi1 - 2.0 / theta1 - 6.0 * psi2 - 16.0 / theta2;
  }
  o.lj = lj;
  o.lp = lp;
  return o;
}
// the rate of component q (0, 1) in dimension k of a d-dimensional design, from the four values above
CCGP_CHAIN_HD inline double chain_rate(const ChainTerms& o, int prior_id, int q, int k) {
  return o.t[2 * q + (prior_id == CCGP_PRIOR_ANI ? k : 0)];
}
// val = ll + ljac + lprior in logpost_rows' order; every NaN is the one quiet NaN, so that the host twin and the kernel agree
// in the bits of a failed proposal too (which NaN an addition of two NaNs returns is the hardware's choice)
CCGP_CHAIN_HD inline double chain_value(double ll, double lj, double lp) {
#pragma clang fp contract(off)
  const double v = ll + lj + lp;
  return v == v ? v : chain_from_bits(0x7ff8000000000000ULL);
}

}  // namespace ccgp
