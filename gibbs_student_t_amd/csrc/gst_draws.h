// The sampler's variate maps and the draw laws that its kernels share: plain scalar functions of
// their arguments for the persistent kernel (gst_kernel.hpp), the large path (gst_large.hpp) and
// the simulator (gst_sim.hpp).  No lane intrinsics, no LDS, no kernel state and no HIP: a plain
// C++ compiler can include this header (tools/draws_dump.cpp and its CPU test do).  A law is
// here when every kernel that calls it compiles to the instructions it had with the arithmetic
// written in place (DESIGN.md 4d.2c lists the ones that stayed in their kernels).
#pragma once
#include <math.h>
#include <stdint.h>

#include "gst_model.h"
#include "philox.hpp"

#if defined(__HIPCC__)
#define GST_DEV __device__   // a device function of its own, not inlined by force (gamma_mt)
#else
#define GST_DEV inline
#endif

namespace gst {

constexpr double LN10 = 2.302585092994045684;

// 10^(2 v): Q = 10^(2 log10_equad), and the factor 10^(2 delta) an equad move rescales it by
GST_HD double pow10_2(double v) { return exp(2.0 * v * LN10); }

// The jump (xi * sigma) * scale exactly as numpy evaluates it (gibbs.py:97,130): no FMA
// contraction, so x + jump matches the reference bit for bit.
GST_HD double mh_step(double xi, double sig, double scale) {
#pragma clang fp contract(off)
  return (xi * sig) * scale;
}

// numpy legacy binomial(1, p) given its uniform (inversion branch, random_binomial).
GST_HD int bern_legacy(double p, double u) {
  if (p == 0.0) return 0;
  if (p <= 0.5) return u > exp(log(1.0 - p)) ? 1 : 0;
  const double qq = 1.0 - p;
  return u > exp(log(1.0 - qq)) ? 0 : 1;
}

// cos(2 pi u) for u in [0, 1): folded to a quarter turn, then the Taylor series of cos or
// sin on [0, pi/4] (truncation < 1e-16), chosen by select.  Lighter than OCML's cospi
// (fewer live registers inside the per-TOA gamma loops).
GST_HD double cos2pi(double u) {
  double x = u < 0.5 ? u : 1.0 - u;            // cos(2 pi (1 - u)) = cos(2 pi u)
  const double sg = x > 0.25 ? -1.0 : 1.0;     // cos(2 pi (1/2 - x)) = -cos(2 pi x)
  x = x > 0.25 ? 0.5 - x : x;                  // x in [0, 1/4]
  const bool sn = x > 0.125;                   // cos(2 pi x) = sin(2 pi (1/4 - x))
  const double t = (sn ? 0.25 - x : x) * 6.283185307179586477;   // t in [0, pi/4]
  const double t2 = t * t;
  double c = 1.0 / 20922789888000.0;           // 1/16!
  c = fma(c, t2, -1.0 / 87178291200.0);
  c = fma(c, t2, 1.0 / 479001600.0);
  c = fma(c, t2, -1.0 / 3628800.0);
  c = fma(c, t2, 1.0 / 40320.0);
  c = fma(c, t2, -1.0 / 720.0);
  c = fma(c, t2, 1.0 / 24.0);
  c = fma(c, t2, -0.5);
  c = fma(c, t2, 1.0);
  double sv = 1.0 / 355687428096000.0;         // 1/17!
  sv = fma(sv, t2, -1.0 / 1307674368000.0);
  sv = fma(sv, t2, 1.0 / 6227020800.0);
  sv = fma(sv, t2, -1.0 / 39916800.0);
  sv = fma(sv, t2, 1.0 / 362880.0);
  sv = fma(sv, t2, -1.0 / 5040.0);
  sv = fma(sv, t2, 1.0 / 120.0);
  sv = fma(sv, t2, -1.0 / 6.0);
  sv = fma(sv, t2, 1.0) * t;
  return sg * (sn ? sv : c);
}

// sin(2 pi u) = cos(2 pi (u - 1/4)), the argument wrapped back into [0, 1)
GST_HD double sin2pi(double u) {
  return cos2pi(u < 0.25 ? u + 0.75 : u - 0.25);
}

// Box-Muller normal from one Philox draw (its cosine half).
GST_HD double normal_from(const Rng& rng, uint32_t index, uint32_t tag) {
  double a, b;
  rng.uniform2(index, tag, a, b);
  return sqrt(-2.0 * log(1.0 - a)) * cos2pi(b);
}

// Both Box-Muller normals of one Philox draw: normals 2k and 2k + 1 of a stream.
GST_HD void normal_pair(const Rng& rng, uint32_t k, uint32_t tag,
                                            double& n0, double& n1) {
  double a, b;
  rng.uniform2(k, tag, a, b);
  const double r = sqrt(-2.0 * log(1.0 - a));
  n0 = r * cos2pi(b);
  n1 = r * sin2pi(b);
}

// Normal j of a stream (one element of normal_pair(j / 2)).
GST_HD double normal_k(const Rng& rng, uint32_t j, uint32_t tag) {
  double n0, n1;
  normal_pair(rng, j >> 1, tag, n0, n1);
  return (j & 1u) ? n1 : n0;
}

// Marsaglia-Tsang Gamma(a, 1); a < 1 via the a+1 boost.  Attempts go in pairs: one Philox
// draw gives both Box-Muller normals, a second the two acceptance uniforms.  Bounded.
GST_DEV double gamma_mt(double a, const Rng& rng, uint32_t index, uint32_t tag) {
  double boost = 1.0;
  if (a < 1.0) {
    double ub, unused;
    rng.uniform2(index, tag | 0xFFFFFFu, ub, unused);
    boost = exp(log(1.0 - ub) / a);
    a += 1.0;
  }
  const double d = a - 1.0 / 3.0;
  const double cc = 1.0 / sqrt(9.0 * d);
#pragma unroll 1
  for (uint32_t att = 0; att < 128u; ++att) {
    double u1, u2, ua, ub;
    rng.uniform2(index, tag | (2u * att), u1, u2);
    rng.uniform2(index, tag | (2u * att + 1u), ua, ub);
    const double r = sqrt(-2.0 * log(1.0 - u1));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double xn = r * (h == 0 ? cos2pi(u2) : sin2pi(u2));
      const double u3 = h == 0 ? ua : ub;
      double v = 1.0 + cc * xn;
      if (v <= 0.0) continue;
      v = v * v * v;
      const double x2 = xn * xn;
      if (u3 < 1.0 - 0.0331 * x2 * x2) return d * v * boost;
      if (log(u3) < 0.5 * x2 + d * (1.0 - v + log(v))) return d * v * boost;
    }
  }
  return d * boost;
}

// gamma_mt for NS draws at once -- draw s with shape a[s] and Philox index index0 + 64 s,
// for the slots in `active` -- in one rejection loop, so the independent draws' dependency
// chains interleave.  Every draw consumes exactly gamma_mt's variates in gamma_mt's order,
// hence returns bitwise gamma_mt(a[s], rng, index0 + 64 s, tag).
template <int NS>
GST_HD void gamma_mt_slots(const double (&a)[NS], unsigned active,
                                               const Rng& rng, uint32_t index0, uint32_t tag,
                                               double (&out)[NS]) {
  double d[NS], cc[NS], boost[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    double as = a[s];
    boost[s] = 1.0;
    if (((active >> s) & 1u) && as < 1.0) {
      double ub, unused;
      rng.uniform2(index0 + 64u * s, tag | 0xFFFFFFu, ub, unused);
      boost[s] = exp(log(1.0 - ub) / as);
      as += 1.0;
    }
    d[s] = as - 1.0 / 3.0;
    cc[s] = 1.0 / sqrt(9.0 * d[s]);
    out[s] = d[s] * boost[s];                 // gamma_mt's value after 256 failed attempts
  }
  unsigned pend = active;
#pragma unroll 1
  for (uint32_t att = 0; att < 128u && pend; ++att) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (!((pend >> s) & 1u)) continue;
      double u1, u2, ua, ub;
      rng.uniform2(index0 + 64u * s, tag | (2u * att), u1, u2);
      rng.uniform2(index0 + 64u * s, tag | (2u * att + 1u), ua, ub);
      const double r = sqrt(-2.0 * log(1.0 - u1));
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (!((pend >> s) & 1u)) break;
        const double xn = r * (h == 0 ? cos2pi(u2) : sin2pi(u2));
        const double u3 = h == 0 ? ua : ub;
        double v = 1.0 + cc[s] * xn;
        if (v <= 0.0) continue;
        v = v * v * v;
        const double x2 = xn * xn;
        if (u3 < 1.0 - 0.0331 * x2 * x2 || log(u3) < 0.5 * x2 + d[s] * (1.0 - v + log(v))) {
          out[s] = d[s] * v * boost[s];
          pend &= ~(1u << s);
        }
      }
    }
  }
}

// ---- MH variates (gibbs.py:95-104, 128-137) ----------------------------------------------
// The variates of global step gs (0..19 white, 20..29 hyper): out4 = parameter index, jump,
// log(u_accept), 10^(2 jump).  tp: the chain's tape row (the reference's recorded u_scale,
// parameter, normal, u_accept) or null for Philox.
GST_HD void mh_variate(const DevModel& md, const Rng& rng, const double* tp, int gs,
                       double* out4) {
  const bool white = gs < NWHITE;
  const int step = white ? gs : gs - NWHITE;
  double us, par, xi, la;
  if (tp) {
    const double* e = tp + (white ? TP_WHITE : TP_HYPER) + 4 * step;
    us = e[0];
    par = e[1];
    xi = e[2];
    la = log(e[3]);
  } else {
    const uint32_t tag = white ? TAG_WHITE : TAG_HYPER;
    double ua, ub, uidx, unused;
    rng.uniform2(0u, tag | (uint32_t)(3 * step), ua, ub);
    us = ua;
    la = log(ub);
    xi = normal_from(rng, 0u, tag | (uint32_t)(3 * step + 1));
    const int nind = white ? md.nw : md.nh;
    rng.uniform2(0u, tag | (uint32_t)(3 * step + 2), uidx, unused);
    int k = (int)(uidx * nind);
    k = k < nind - 1 ? k : nind - 1;
    const int* ind = white ? md.wind : md.hind;   // ind[k] as a select chain: no indexed load
    int pk = ind[0];
#pragma unroll
    for (int j = 1; j < PMAX; ++j) pk = (k == j) ? ind[j] : pk;
    par = (double)pk;
  }
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) cnt += (md.mh_cdf[i] <= us) ? 1 : 0;
  cnt = cnt < 4 ? cnt : 4;
  const double scale = md.mh_size[0] * (cnt == 0) + md.mh_size[1] * (cnt == 1) +
                       md.mh_size[2] * (cnt == 2) + md.mh_size[3] * (cnt == 3) +
                       md.mh_size[4] * (cnt == 4);
  const double delta = mh_step(xi, white ? md.sig_w : md.sig_h, scale);
  out4[0] = par;
  out4[1] = delta;
  out4[2] = la;
  out4[3] = exp(2.0 * delta * LN10);
}

// ---- the prior side of the b-marginalised likelihood (gibbs.py:288-329) --------------------
// log phi_k = lc - g log f_k + log df_k with the power law's coefficient
// lc = 2 lA ln10 - log(12 pi^2) + (g - 3) log fyr
GST_HD double powerlaw_lc(double lA, double g, double log_12pi2, double log_fyr) {
  return 2.0 * lA * LN10 - log_12pi2 + (g - 3.0) * log_fyr;
}
// phi^-1 of a Fourier column, of an ECORR column (phi = 10^(2 log10_ecorr)); + the b draw's
// SVD noise floor f (0 outside the floor pass)
GST_HD double phi_inv_fourier(double lc, double g, double lfreq, double ldf, double fsh) {
  return exp(-(lc - g * lfreq + ldf)) + fsh;
}
GST_HD double phi_inv_ecorr(double lec, double fsh) { return exp(-2.0 * lec * LN10) + fsh; }
// log|phi| in closed form: the nf Fourier columns and the timing model's constant, then
// count ECORR columns of one backend
GST_HD double logdet_phi_fourier(int nf, double lc, double g, double sum_lfreq, double sum_ldf,
                                 double logdet_phi_tm) {
  return ((double)nf * lc - g * sum_lfreq + sum_ldf) + logdet_phi_tm;
}
// several power-law processes in the Fourier block: the closed form of one process over its own
// ncol columns; log|phi| = sum over the processes + the timing model's constant (+ ECORR)
GST_HD double logdet_phi_process(int ncol, double lc, double g, double sum_lfreq,
                                 double sum_ldf) {
  return (double)ncol * lc - g * sum_lfreq + sum_ldf;
}
GST_HD double logdet_phi_ecorr(double count, double lec) { return count * (2.0 * lec * LN10); }
// lnL = -0.5 (log|N| + r^T N^-1 r) + 0.5 (d^T Sigma^-1 d - log|Sigma| - log|phi|)
GST_HD double marginal_ll(double logdetN, double rNr, double quad, double ld_sigma,
                          double logdet_phi) {
  double ll = -0.5 * (logdetN + rNr);
  ll += 0.5 * (quad - ld_sigma - logdet_phi);
  return ll;
}

}  // namespace gst
