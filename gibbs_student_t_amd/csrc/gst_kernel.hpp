// Persistent per-chain Gibbs sweep kernel for gfx950 (MI355X, CDNA4).
//
// One 64-lane wavefront owns one chain for a whole launch of `nsweeps` sweeps of the
// reference sampler (/root/reference/gibbs.py, Gibbs.sample loop gibbs.py:354-380).
// Chains are independent, so waves never synchronise with each other: there is no
// __syncthreads, only in-order same-wave LDS traffic (except in the two-waves-per-chain
// build, PAIR below, whose two waves exchange MH likelihoods once per round).
//
// Matrix layout ("8x8 cyclic"): lane = 8p + q owns elements (8r+p, 8s+q) of the symmetric
// system matrix, r >= s, in registers L[SL(r,s)].  Internal column order is
//     [ timing model (ntm) | pad to 8*K0 | Fourier (nf) | r (augmented row) | pad ]
// so that (i) the timing-model block, whose prior never changes inside a sweep, is
// eliminated once per sweep (its Schur complement S0 is kept in registers) and (ii) the
// residual column rides along as an augmented row whose elimination yields L^-1 d, i.e.
// d^T Sigma^-1 d, for free.  Every MH step of the red-noise hyper block only refactors the
// (nf+1)-row Fourier block S0 + diag(phi^-1).
//
// Stages per sweep (gibbs.py stage order, semantically binding):
//   white MH (20 steps)      gibbs.py:114-143, lnL gibbs.py:262-284
//   Gram T^T N^-1 [T|r]       gibbs.py:302-304  -- fp64 MFMA 16x16x4, T shared by all chains
//   hyper MH (10 steps)      gibbs.py:80-111,  lnL gibbs.py:288-329
//   b draw (quirk :373)       gibbs.py:145-182  -- Cholesky draw mu + L^-T eta
//   theta, z, alpha, nu       gibbs.py:185-259
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "gst_chol.hpp"
#include "gst_draws.h"
#include "gst_model.h"
#include "gst_wave.hpp"
#include "philox.hpp"

namespace gst {

// WPB = chains (waves) per workgroup (4 = one per SIMD; the host picks 2 or 1 when the
// launch has fewer chains than CUs x 4, so the chains spread over every CU).  OCC = chains
// per SIMD the kernel is compiled for: 2 caps it at 256 registers per lane (VGPR + AGPR)
// so that two workgroups share a CU and each SIMD interleaves two chains' dependency
// chains (the kernel is latency-bound per wave).
// PAIR (with WPB = 2): the two waves of a workgroup run ONE chain, for launches with at most
// one chain per two SIMDs (config 3's 512 chains).  Both waves run every stage on identical
// state and variates; in the hyper block they evaluate different MH points per round -- the
// next proposal, and the one after it on the branch the chain's acceptance history predicts
// -- and exchange the lnL values through LDS, so that a round settles one or two MH steps
// (DESIGN.md section 8).
// GEN: the general white-noise model (per-backend efac / equad, ECORR epoch columns in the
// hyper block, up to 8 parameters; gibbs.py:64-77); pair mode too since round 6.
// ACC: the instances that keep the posterior sums (gst_set_accum), launched only while the
// sums are set.  Instances of their own because the sweep kernel sits at the register limit
// (most instances spill): the same code behind a run-time test moved the allocation of the
// whole kernel (J1713 two-chains-per-SIMD instance: scratch 340 -> 372 B/lane), while a
// template parameter leaves every other instance's code, and so its registers, as they were.
template <int MT, int NS, int K0, int RA, bool TAPE, int WPB = 4, int OCC = 1, bool PAIR = false,
          bool GEN = false, bool ACC = false>
__global__ void __launch_bounds__(64 * WPB, OCC)
    gst_sweep_kernel(const DevModel* __restrict__ mds, const DevState st, const DevRec rec, const DevTape tape,
                     int C, int nsweeps, long long sweep0, int record_every, unsigned mask,
                     unsigned long long seed, long long chain0, int eval_only, double* out_w,
                     double* out_h) {
  static_assert(!PAIR || (WPB == 2 && !TAPE), "pair mode: one chain per 2-wave workgroup");
  constexpr int PX = GEN ? 8 : 4;     // parameters held in registers
  constexpr int NSL = SL(MT, 0);
  constexpr int NT = MT / 2;          // 16-wide MFMA tiles
  constexpr int NTT = NT * (NT + 1) / 2;
  constexpr int MP = 8 * MT;
  constexpr int NTMS = NSL - SL(MT - K0, 0);  // timing-model factor slots (s < K0)
  constexpr int TB_LD = 17;
  constexpr int S0RD = s0r_doubles(MT, K0);
  static_assert(s0r_need(MT, NS) <= S0RD, "S0 region too small for the stage scratch");
  __shared__ double smem[WPB][lds_doubles(MT, K0)];
  __shared__ double xchg[PAIR ? 2 : 1][2][2];  // pair mode: [round parity][wave] {lnL, failed}
  __shared__ int xdrew[PAIR ? 1 : 1];          // pair mode: the b draw happened this sweep
  __shared__ double xfloor[1];                 // pair mode: the owner's floor_shift
  // pair mode: z / pout and alpha of the TOA slots the other wave drew (slot s belongs to
  // wave s & 1), exchanged after each stage
  __shared__ double xpo[PAIR ? NS : 1][PAIR ? 64 : 1], xal[PAIR ? NS : 1][PAIR ? 64 : 1];
  __shared__ double xyv[PAIR ? NS : 1][PAIR ? 64 : 1];   // pair mode: the drawer's y = r - T b
  __shared__ unsigned long long xzm[PAIR ? NS : 1];
  __shared__ unsigned gcnt[WPB][2];            // Grams by path (gst_gram_counts)

  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = PAIR ? (int)blockIdx.x : (int)blockIdx.x * WPB + wv;
  const int role = PAIR ? wv : 0;   // pair mode: which of the chain's two waves
  if (c >= C) return;
  // the chain's dataset (run_sims grids batch many datasets x models per launch): every
  // field of md is wave-uniform, so it is read with scalar loads
  const int ds = st.dataset ? __builtin_amdgcn_readfirstlane(st.dataset[c]) : 0;
  if ((unsigned)ds >= (unsigned)st.nd) {  // bad index: flag the chain, touch nothing else
    if (lane == 0 && st.status) st.status[c] |= 4;
    return;
  }
  const DevModel& md = mds[ds];
  const int nst = st.nst;
  const int p = lane >> 3, q = lane & 7;
  Fair fair{OCC == 2 ? wave_slot_parity() : 0u, -1};
  unsigned long long prog_ret = 0ull;  // lane 0: this sweep's ticket from st.prog
  GST_STAMP_DECL

  double* S0R = smem[wv];             // S0 during the hyper block, else stage scratch
  double* colq = S0R + S0RD;          // [8][MT] the published column
  double* mhh = colq + 8 * MT;        // [10][4] hyper MH variates
  double* phbuf = mhh + 4 * NHYPER;   // phi^-1 by internal index; eliminations' junk rows
  double* colq2 = phbuf + 8 * MT;     // [8][PW] paired tail: the odd published column
  double* S0 = S0R + lane;            // S0[64 * slot]
  // scratch inside S0R (S0 is dead outside the hyper block):
  double* mhw = S0R;                  // [20][4] white MH variates (sweep start .. white block)
  double* vbuf = S0R;                 // Gram weights, 64*NS
  double* tbuf = S0R + 64 * NS;       // 16 x TB_LD Gram tile transpose
  double* zraw = S0R;                 // b draw: a_{raug,k}
  double* apiv = zraw + MP;           //   pivots a_kk
  double* wvec = apiv + MP;           //   back-substitution rhs
  double* xbuf = wvec + MP;           //   Delta, solution (internal order)
  double* yinv = xbuf + MP;           //   1/sqrt(a_kk)
  double* bsc = yinv + MP;            //   b in reference order (T b input)
  double* tdg = bsc + MP;             //   8 x 8 diagonal-block transposes
  double* dfbuf = S0R;                // nu grid: weights [32], probabilities [32]
  // the TM factor slots (s < K0) wait in global scratch while the hyper block runs
  // per-chain rows of the state arrays: wave-uniform base pointers (SGPRs), so every
  // per-lane access is base + 32-bit lane offset
  const LaneRows tmf =
      lane_rows(st.tmfac + ((size_t)c * (PAIR ? 2 : 1) + role) * NTMS * 64, NTMS * 64, lane);
  double* const xrow = st.x + (size_t)c * md.P;
  double* const brow = st.b + (size_t)c * md.m;
  double* const zrow = st.z + (size_t)c * nst;
  double* const arow = st.alpha + (size_t)c * nst;
  double* const prow = st.pout + (size_t)c * nst;

  static_assert(RA >= 8 * K0 + 1 && RA < 8 * MT, "augmented row out of range");
  const int n = md.n, m = md.m, P = md.P;
  constexpr int raug = RA;
  const int npad = md.npad;
  const long long gch = chain0 + c;

  Rng rng;
  rng.k0 = (uint32_t)(seed & 0xffffffffull);
  rng.k1 = (uint32_t)(seed >> 32);
  rng.chain = (uint32_t)gch;
  rng.sweep = 0;

  // ---------------- load chain state ----------------
  double xv[PX] = {};
#pragma unroll
  for (int j = 0; j < PX; ++j)
    if (j < P) xv[j] = xrow[j];
  double theta = st.theta[c];
  double nu = st.nu[c];
  for (int j = lane; j < MP; j += 64) bsc[j] = (j < m) ? brow[j] : 0.0;
  for (int j = lane; j < MP; j += 64) phbuf[j] = 0.0;

  // per-TOA chain state in registers: alpha, y = r - T b, pout and the z bits; the data
  // (r, sigma^2, noise class) is re-read from the dataset's L2-resident arrays where used
  double al[NS], yv[NS], po[NS];
  double wcls = 0.0;  // lane u < ncls: W_u of the current white block
  unsigned zb = 0u, vmask = 0u;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int t = 64 * s + lane;
    const bool ok = t < n;
    vmask |= ok ? (1u << s) : 0u;
    al[s] = ok ? arow[t] : 1.0;
    po[s] = ok ? prow[t] : 0.0;
    const double zz = ok ? zrow[t] : 0.0;
    zb |= (zz != 0.0) ? (1u << s) : 0u;
    yv[s] = 0.0;
  }
  double rrr[OCC == 1 ? NS : 1];   // one-wave-per-SIMD builds: the lanes' residuals, as s2r
  if constexpr (OCC == 1) {
#pragma unroll
    for (int s = 0; s < NS; ++s) rrr[s] = ((vmask >> s) & 1u) ? md.resid[64 * s + lane] : 0.0;
  }
  auto RR = [&](int s) __attribute__((always_inline)) -> double {
    if constexpr (OCC == 1)
      return rrr[s];
    else
      return md.resid[64 * s + lane];
  };
  // one-wave-per-SIMD builds: sigma^2 of the lane's TOAs in registers for the launch (the
  // per-TOA white likelihood reads it 21 times a sweep, each a pointer load, a global load
  // and a wait without machine LICM); the two-chains-per-SIMD build has no registers to spare
  double s2r[OCC == 1 ? NS : 1];
  if constexpr (OCC == 1) {
#pragma unroll
    for (int s = 0; s < NS; ++s) s2r[s] = ((vmask >> s) & 1u) ? md.sig2[64 * s + lane] : 0.0;
  }
  auto S2 = [&](int s) __attribute__((always_inline)) -> double {
    if constexpr (OCC == 1)
      return s2r[s];
    else
      return md.sig2[64 * s + lane];
  };
  int status = 0, nfloor = 0;   // nfloor: b draws at the SVD noise floor in this launch
  // Grams computed in this launch by path (gst_gram_counts): low-rank (class Grams + rank-1
  // updates on the VALU) and n-TOA fp64 MFMA, counted in LDS (registers held across the sweep
  // loop raised the two-chains-per-SIMD build's spill by 32 B/lane)
  if (lane == 0) {
    gcnt[wv][0] = 0u;
    gcnt[wv][1] = 0u;
  }
  lds_order();

  // y = r - T b (gibbs.py:213,237,272): 8 columns x NS TOA slots of loads in flight
  auto compute_Tb = [&]() __attribute__((always_inline)) {
    double tb[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) tb[s] = 0.0;
    const int nsl = md.nslot_toa;
    const double* tc = md.Tcol;
    int j = 0;
#pragma unroll 1
    for (; j + 8 <= m; j += 8) {   // (16 columns per round: 2% slower, spills)
      double tv[8][NS], bj[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
#pragma unroll
        for (int s = 0; s < NS; ++s)
          tv[u][s] = tc[(j + u) * npad + 64 * (s < nsl ? s : nsl - 1) + lane];
        bj[u] = bsc[j + u];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int s = 0; s < NS; ++s) tb[s] = fma(tv[u][s], bj[u], tb[s]);
    }
#pragma unroll 1
    for (; j < m; ++j) {
      const double bjj = bsc[j];
#pragma unroll
      for (int s = 0; s < NS; ++s)
        tb[s] = fma(tc[j * npad + 64 * (s < nsl ? s : nsl - 1) + lane], bjj, tb[s]);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) yv[s] = (s < nsl) ? RR(s) - tb[s] : 0.0;
  };

  // sum of log-priors (gibbs.py:337-339): every prior is uniform, so the sum is the
  // host-evaluated constant (Python sum order) when all parameters are in bounds, else -inf
  // one-wave-per-SIMD builds (registers to spare): the prior bounds and efac choice held in
  // registers for the launch instead of re-read from the model descriptor at every call
  // (no machine LICM in this build: each read was a load and a wait)
  double hpmin[PX], hpmax[PX], hlp = 0.0, hefc = 1.0;
  int hief = -1;
  if constexpr (OCC == 1) {
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      hpmin[j] = j < P ? md.pmin[j] : 0.0;
      hpmax[j] = j < P ? md.pmax[j] : 0.0;
    }
    hlp = md.lp_sum;
    hief = md.idx_efac;
    hefc = md.efac_const;
  }
  auto lnprior = [&](const double (&xq)[PX]) __attribute__((always_inline)) -> double {
    // Branch-free, and every bound read before the first compare: the short-circuit form
    // compiled to a cascade of branches in which each bound's scalar load was issued and
    // waited for (with every LDS access in flight) in turn, up to 2 P + 1 round trips per call
    // (pmin / pmax have PMAX >= PX entries: the ones past P are read and ignored)
    double lo[PX], hi[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      lo[j] = OCC == 1 ? hpmin[j] : md.pmin[j];
      hi[j] = OCC == 1 ? hpmax[j] : md.pmax[j];
    }
    const double lp = OCC == 1 ? hlp : md.lp_sum;
    bool in = true;
#pragma unroll
    for (int j = 0; j < PX; ++j) in = in & ((j >= P) | ((xq[j] >= lo[j]) & (xq[j] <= hi[j])));
    return in ? lp : -INFINITY;
  };

  auto efac2_of = [&](const double (&xq)[PX]) __attribute__((always_inline)) -> double {
    const double ef = OCC == 1 ? (hief >= 0 ? pget(xq, hief) : hefc)
                               : (md.idx_efac >= 0 ? pget(xq, md.idx_efac) : md.efac_const);
    return ef * ef;
  };

  // GEN: N0 = efac_b^2 sigma^2 + 10^(2 equad_b) of the TOA's backend b (gibbs.py:262-284 with
  // the enterprise white-noise signal per backend).  The parameter indices of each of the
  // lane's TOA slots and of its noise class (lane u < ncls) are held for the launch.
  int gef[GEN ? NS : 1], geq[GEN ? NS : 1], gcef = -1, gceq = 0;
  if constexpr (GEN) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int b = ((vmask >> s) & 1u) && md.bk ? md.bk[64 * s + lane] : 0;
      gef[s] = md.efac_b[b];
      geq[s] = md.equad_b[b];
    }
    const int cb = lane < md.ncls ? md.cls_b[lane] : 0;
    gcef = md.efac_b[cb];
    gceq = md.equad_b[cb];
  }
  auto gen_n0 = [&](const double (&xq)[PX], double s2, int ie, int iq)
      __attribute__((always_inline)) -> double {
    const double ef = ie >= 0 ? pget(xq, ie) : md.efac_const;
    return ef * ef * s2 + pow10_2(pget(xq, iq));
  };
  // N0 of noise class k (wave-uniform k)
  auto cls_n0 = [&](const double (&xq)[PX], int k) __attribute__((always_inline)) -> double {
    const int b = md.cls_b[k];
    return gen_n0(xq, md.csig2[k], md.efac_b[b], md.equad_b[b]);
  };

  // white-noise conditional likelihood (gibbs.py:262-284).  Class path: TOAs with equal
  // sigma share N0 = efac^2 sigma^2 + Q, so with a_t = alpha_t^z_t
  //   sum_t log N_t = sum_t log a_t + sum_u c_u log N0_u,
  //   sum_t y_t^2 / N_t = sum_u W_u / N0_u,   W_u = sum_{t in u} y_t^2 / a_t,
  // where sum log a_t and W_u are fixed for the whole white block (b, alpha, z fixed).
  const int hncls = md.ncls, hieq = md.idx_equad;   // read once for the launch (scalars)
  double wcls_la = 0.0;   // sum_t log a_t
  auto white_prep = [&]() __attribute__((always_inline)) {
    if (md.ncls == 0) return;
    double la = 0.0;
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if ((vmask >> s) & 1u) la += ((zb >> s) & 1u) ? log(al[s]) : 0.0;
    wcls_la = wave_sum(la);
    // only the TOA slots of this chain's dataset: a ragged batch's shorter datasets have
    // fewer than 64 NS entries of cidx
    int cls[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) cls[s] = ((vmask >> s) & 1u) ? md.cidx[64 * s + lane] : -1;
    for (int u = 0; u < md.ncls; ++u) {
      double w = 0.0;
#pragma unroll
      for (int s = 0; s < NS; ++s)
        if (((vmask >> s) & 1u) && cls[s] == u)
          w += yv[s] * yv[s] / (((zb >> s) & 1u) ? al[s] : 1.0);
      w = wave_sum(w);
      if (lane == u) wcls = w;
    }
  };
  // Q = 10^(2 equad) is passed in: the MH steps carry it (Q_q = Q_x * 10^(2 delta)).
  auto lnl_white = [&](const double (&xq)[PX], double Q) __attribute__((always_inline)) -> double {
    const double ef2 = efac2_of(xq);
    if (hncls == 1) {  // uniform: no reduction
      double N0;
      if constexpr (GEN)
        N0 = cls_n0(xq, 0);
      else
        N0 = ef2 * md.csig2[0] + Q;
      return -0.5 * ((wcls_la + md.ccount[0] * log(N0)) + rdlane(wcls, 0) / N0);
    }
    double sl = 0.0, sq = 0.0;
    if (hncls > 1) {
      if (lane < md.ncls) {
        const double N0 = GEN ? gen_n0(xq, md.csig2[lane], gcef, gceq) : ef2 * md.csig2[lane] + Q;
        sl = md.ccount[lane] * log(N0);
        sq = wcls / N0;
      }
      sl = wave_sum(sl) + wcls_la;
      sq = wave_sum(sq);
      return -0.5 * (sl + sq);
    }
    LogProd lp;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (vmask & (1u << s)) {
        double N0;
        if constexpr (GEN)
          N0 = gen_n0(xq, S2(s), gef[s], geq[s]);
        else
          N0 = ef2 * S2(s) + Q;
        const double N = ((zb >> s) & 1u ? al[s] : 1.0) * N0;
        lp.mul(N);
        sq += div_pos(yv[s] * yv[s], N);
      }
    }
    sl = wave_sum(lp.log_sum());
    sq = wave_sum(sq);
    return -0.5 * (sl + sq);
  };

  // MH variates of one sweep (30 steps: 20 white then 10 hyper), produced in parallel by
  // lanes 0..29: u_scale, parameter index, jump normal, log(u_accept) (gibbs.py:95-104,
  // 128-137).  Tape mode copies the reference's recorded values instead.
  // (the large path draws the same numbers with gst_draws.h mh_variate)
  auto mh_variates = [&](const double* tp) __attribute__((always_inline)) {
    if (lane < NWHITE + NHYPER) {
      const bool white = lane < NWHITE;
      const int step = white ? lane : lane - NWHITE;
      double us, par, xi, la;
      if (TAPE) {
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
        par = (double)(white ? iget<PX>(md.wind, k) : iget<PX>(md.hind, k));
      }
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < 5; ++i) cnt += (md.mh_cdf[i] <= us) ? 1 : 0;
      cnt = cnt < 4 ? cnt : 4;
      const double scale = md.mh_size[0] * (cnt == 0) + md.mh_size[1] * (cnt == 1) +
                           md.mh_size[2] * (cnt == 2) + md.mh_size[3] * (cnt == 3) +
                           md.mh_size[4] * (cnt == 4);
      const double delta = mh_step(xi, white ? md.sig_w : md.sig_h, scale);
      double* e = white ? mhw + 4 * step : mhh + 4 * step;
      e[0] = par;
      e[1] = delta;
      e[2] = la;
      e[3] = exp(2.0 * delta * LN10);
    }
    lds_order();
  };

  // MH proposal of global step gs (gibbs.py:90-97 / 123-130): q = x with q[par] += delta;
  // returns log(u_accept).  E receives 10^(2 delta) (equad moves rescale Q by it).
  auto propose = [&](const double (&xq)[PX], double (&qv)[PX], int gs, double& E, int& par)
      __attribute__((always_inline)) -> double {
    const double* e = gs < NWHITE ? mhw + 4 * gs : mhh + 4 * (gs - NWHITE);
    par = (int)e[0];
    const double delta = e[1];
    E = e[3];
#pragma unroll
    for (int j = 0; j < PX; ++j) qv[j] = (j == par) ? xq[j] + delta : xq[j];
    return e[2];
  };

  // ---------------- matrix state ----------------
  double L[NSL];
  double ld_tm_m = 1.0, quad_tm = 0.0, logdetN = 0.0, rNr = 0.0;
  double tm_apr = 1.0, tm_zr = 0.0;       // timing-model columns' pivots / aug entries
  double f_apr[2] = {1.0, 1.0}, f_zr[2] = {0.0, 0.0};  // last factorisation's
  int ld_tm_e = 0, fail_tm = 0;

  // SVD noise floor f of this sweep's b draw (floor_shift; 0 except on the floor redo)
  double fshift = 0.0;
  // the low-rank Gram's descriptor pointers, read once for the launch (wave-uniform: scalar
  // registers) like lnl_hyper's scalars below, not at every class and flagged TOA
  const double* const hgcls = md.Gcls;
  const double* const hcsig2 = md.csig2;
  const int* const hcidx = md.cidx;
  const GDouble* const htrow = (const GDouble*)md.Trow;
  // Gram: G = T_aug^T diag(1/N) T_aug on fp64 MFMA, then TM elimination -> S0.
  auto gram_and_tm = [&](const double (&xq)[PX]) __attribute__((always_inline)) {
    const double ef2 = efac2_of(xq);
    const double Q = pow10_2(pget(xq, md.idx_equad));
    double sr = 0.0;
    double wlane[NS];   // the lane's weights w_t = 1 / N_t (the low-rank Gram reads them by lane)
    LogProd lp;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int t = 64 * s + lane;
      double w = 0.0;
      if (vmask & (1u << s)) {
        double N0;
        if constexpr (GEN)
          N0 = gen_n0(xq, S2(s), gef[s], geq[s]);
        else
          N0 = ef2 * S2(s) + Q;
        const double N = ((zb >> s) & 1u ? al[s] : 1.0) * N0;
        lp.mul(N);
        const double rs = RR(s);
        sr += rs * rs / N;
        w = 1.0 / N;
      }
      vbuf[t] = w;
      wlane[s] = w;
    }
    logdetN = wave_sum(lp.log_sum());
    rNr = wave_sum(sr);
    lds_order();
    GST_SUB_BEGIN
    // Low-rank Gram (one backend, <= 8 noise classes, at most LR_MAX flagged TOAs): the
    // weights are c_k (1 / alpha_t)^z_t with c_k = 1 / N0 of the TOA's noise class, so
    //   G = sum_k c_k G_k + sum_{t: z_t = 1} c_k(t) (1 / alpha_t - 1) [T|r]_t [T|r]_t^T
    // with the per-class Grams G_k of the dataset (DevModel::Gcls) -- the same T^T N^-1 [T|r]
    // (gibbs.py:302-304) at a cost of the class terms plus one rank-1 update per flagged TOA
    // instead of the MFMA Gram over all n TOAs (config 2: ~7 flagged of 130).
    // Taken only while every flagged TOA's alpha is at most LR_ALPHA_MAX: the rank-1 terms
    // subtract c_k (1 - 1 / alpha_t) of a class Gram's share, so a direction fixed by flagged
    // TOAs alone keeps an absolute error ~eps c_k |row|^2 against its true c_k |row|^2 / alpha_t
    // (relative ~eps alpha_t); past the bound (vvh17's fixed alpha = 1e10) the MFMA Gram runs.
    int nout = 0;
    bool big = false;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      nout += __popcll(__ballot(((zb & vmask) >> s) & 1u));
      big = big || ((((zb & vmask) >> s) & 1u) && al[s] > LR_ALPHA_MAX);
    }
    if (hgcls && nout <= LR_MAX && !(st.debug & DEBUG_MFMA_GRAM) && __ballot(big) == 0ull) {
      __hip_atomic_fetch_add(&gcnt[wv][0], lane == 0 ? 1u : 0u, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WAVEFRONT);
      // Every load of a class Gram is issued before the first is waited for, and class 0's land
      // in L itself (in source order load, FMA, load, FMA each of the 55 loads was a memory
      // round trip of its own: the compiler keeps that order).  The reciprocals c_k = 1 / N0_k
      // are formed once per Gram, class u by lane u as in lnl_white, while class 0 is in
      // flight; both loops below read them by lane.  Each operation and its operands are the
      // serial form's (an FMA with a zero addend for class 0, the explicit fma of N0 that the
      // serial form contracted to), so the chains are bitwise unchanged.
      // The class arrays are read as lane rows (a buffer resource in scalar registers + the
      // lane's byte offset): as 64-bit per-lane pointers they were one address pair per load
      // in flight (or per launch-invariant address), spilled and reloaded one by one.  Reads
      // past an array's end (lanes >= ncls, a ragged batch's missing TOA slots) return zero.
      const LaneRows gcls = lane_rows(hgcls, hncls * NSL * 64, lane);
      const LaneRows csr = lane_rows(hcsig2, hncls, lane);
      const double cs2 = lr_load(csr, 0);
#pragma unroll
      for (int i = 0; i < NSL; ++i) L[i] = lr_load(gcls, 512 * i);
      __builtin_amdgcn_sched_barrier(0);
      const double cinv = 1.0 / (GEN ? gen_n0(xq, cs2, gcef, gceq) : fma(ef2, cs2, Q));
      const double c0 = rdlane(cinv, 0);
#pragma unroll
      for (int i = 0; i < NSL; ++i) L[i] = fma(c0, L[i], 0.0);
      if (hncls > 1) {
        const __amdgpu_buffer_rsrc_t cir =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<int*>(hcidx), 0, npad * 4, 0x00020000);
        int cls[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s)
          cls[s] = __builtin_amdgcn_raw_buffer_load_b32(cir, 4 * lane, 256 * s, 0);
#pragma unroll 1
        for (int k = 1; k < hncls; ++k) {
          const double ck = rdlane(cinv, k);
          const int gk = k * NSL * 512;   // class k's byte offset
          // MT loads in flight per round: the temporaries stay below the flagged loop's rows
#pragma unroll
          for (int i0 = 0; i0 < NSL; i0 += MT) {
            double g[MT];
#pragma unroll
            for (int i = i0; i < i0 + MT && i < NSL; ++i) g[i - i0] = lr_load(gcls, gk + 512 * i);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = i0; i < i0 + MT && i < NSL; ++i) L[i] = fma(ck, g[i - i0], L[i]);
          }
        }
        // w_t - c_k(t) of the lane's own TOAs
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          double ck = c0;
#pragma unroll
          for (int u = 1; u < 8; ++u) ck = cls[s] == u ? rdlane(cinv, u) : ck;
          wlane[s] = wlane[s] - ck;
        }
      } else {
#pragma unroll
        for (int s = 0; s < NS; ++s) wlane[s] = wlane[s] - c0;
      }
      // flagged TOAs, one rank-1 update each: c_k (1 / alpha_t - 1) = w_t - c_k, formed above
      // by the lane that holds the TOA's weight w_t = 1 / N_t.  Between two TOAs' row loads
      // there is address arithmetic only: no load of the class, no division, no LDS read
#pragma unroll 1
      for (int s = 0; s < NS; ++s) {
        unsigned long long bm = __ballot(((zb & vmask) >> s) & 1u);
        int sv = s;   // a per-lane value: selects, not a cascade of scalar branches
        asm("" : "+v"(sv));
        double vs = wlane[0];
#pragma unroll
        for (int s2 = 1; s2 < NS; ++s2) vs = sv == s2 ? wlane[s2] : vs;
#pragma unroll 1
        while (bm) {
          const int tl = __builtin_ctzll(bm);
          const int t = 64 * s + tl;
          bm &= bm - 1;
          // [T|r]_t at internal columns 8 r + p (row side) and 8 r + q (column side): each
          // lane's MT entries are contiguous in Trow ([t][i % 8][i / 8]), 128-bit loads
          typedef double v2_t __attribute__((ext_vector_type(2)));
          const GDouble* tr = htrow + (size_t)t * 8 * MT;
          const __attribute__((address_space(1))) v2_t* trp =
              (const __attribute__((address_space(1))) v2_t*)(tr + MT * p);
          const __attribute__((address_space(1))) v2_t* trq =
              (const __attribute__((address_space(1))) v2_t*)(tr + MT * q);
          double tp_[MT], tq_[MT];
#pragma unroll
          for (int r = 0; r < MT; r += 2) {
            const v2_t a = trp[r / 2], b = trq[r / 2];
            tp_[r] = a[0];
            tp_[r + 1] = a[1];
            tq_[r] = b[0];
            tq_[r + 1] = b[1];
          }
          const double v = rdlane(vs, tl);
#pragma unroll
          for (int r = 0; r < MT; ++r) {
            const double vr = v * tp_[r];
#pragma unroll
            for (int s2 = 0; s2 <= r; ++s2) L[SL(r, s2)] = fma(vr, tq_[s2], L[SL(r, s2)]);
          }
        }
      }
      GST_SUB_END(9)
    } else {
    __hip_atomic_fetch_add(&gcnt[wv][1], lane == 0 ? 1u : 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WAVEFRONT);
    if constexpr (PAIR) {
    // Two waves per chain (PAIR): wave 0 computes the
    // even Gram tiles, wave 1 the odd ones (each its own MFMA pipe), then the tiles are swapped
    // through the two waves' stage-scratch regions (4 tiles per wave per round, 2 rounds)
    // and both waves hold the whole Gram, bitwise the single wave's (same MFMA sequence per
    // tile).
    auto gram_tiles = [&](auto own_c) __attribute__((always_inline)) {
      constexpr int OWN = decltype(own_c)::value;
      auto mine = [](int T) { return OWN == 0 || (T & 1) == OWN - 1; };
      v4d acc[NTT];
#pragma unroll
      for (int i = 0; i < NTT; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
      const int tl = lane >> 4;
      // two k-steps in flight: each operand set is reloaded (for k-step ks + 2) right after
      // its MFMAs have issued, so a T load has two k-steps (30 MFMAs) to arrive from L2
      double ta[NT], tb[NT], wa, wb;
      auto tload = [&](double (&t)[NT], double& w, int ks) __attribute__((always_inline)) {
        const GDouble* src = (const GDouble*)md.Tmf + (size_t)ks * NT * 64;
#pragma unroll
        for (int X = 0; X < NT; ++X) t[X] = src[X * 64 + lane];
        w = vbuf[4 * ks + tl];
      };
      auto kstep = [&](const double (&t)[NT], const double wt) __attribute__((always_inline)) {
#pragma unroll
        for (int I = 0; I < NT; ++I) {
          const double av = t[I] * wt;
#pragma unroll
          for (int J = 0; J <= I; ++J) {
            const int T = I * (I + 1) / 2 + J;
            if (mine(T)) acc[T] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, t[J], acc[T], 0, 0, 0);
          }
        }
      };
      // an even number of k-steps (Tmf and the weights are zero past n: a padding k-step
      // adds exact zeros), so the loop body has no conditional load and the wait before a
      // set's MFMAs covers only that set (a branch in the body made the compiler wait for
      // both sets at the top of every iteration); the scheduling barriers keep the order
      const int nksp = (md.nks + 1) & ~1;
      tload(ta, wa, 0);
      tload(tb, wb, 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
      for (int ks = 0; ks + 2 < nksp; ks += 2) {
        kstep(ta, wa);
        tload(ta, wa, ks + 2);
        __builtin_amdgcn_sched_barrier(0);
        kstep(tb, wb);
        tload(tb, wb, ks + 3);
        __builtin_amdgcn_sched_barrier(0);
      }
      kstep(ta, wa);
      kstep(tb, wb);
      GST_SUB_END(9)
      // MFMA C layout (col = lane&15, row = lane>>4 + 4 reg) -> cyclic register layout
      if constexpr (OWN == 0) {
#pragma unroll
        for (int I = 0; I < NT; ++I) {
#pragma unroll
          for (int J = 0; J <= I; ++J) {
            const v4d a = acc[I * (I + 1) / 2 + J];
#pragma unroll
            for (int g = 0; g < 4; ++g) tbuf[(tl + 4 * g) * TB_LD + (lane & 15)] = a[g];
            lds_order();
#pragma unroll
            for (int dr = 0; dr < 2; ++dr)
#pragma unroll
              for (int ds = 0; ds < 2; ++ds) {
                const int r = 2 * I + dr, s = 2 * J + ds;
                if (r >= s) L[SL(r, s)] = tbuf[(8 * dr + p) * TB_LD + 8 * ds + q];
              }
            lds_order();
          }
        }
      } else {
        constexpr int TS = 16 * TB_LD;  // one padded tile
        static_assert(4 * TS <= s0r_doubles(MT, K0), "tile swap exceeds the stage scratch");
#pragma unroll
        for (int rnd = 0; rnd < 2; ++rnd) {
#pragma unroll
          for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int J = 0; J <= I; ++J) {
              const int T = I * (I + 1) / 2 + J;
              if ((T >> 3) == rnd && mine(T)) {
                double* dst = smem[OWN - 1] + ((T >> 1) & 3) * TS;
#pragma unroll
                for (int g = 0; g < 4; ++g) dst[(tl + 4 * g) * TB_LD + (lane & 15)] = acc[T][g];
              }
            }
          __syncthreads();
#pragma unroll
          for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int J = 0; J <= I; ++J) {
              const int T = I * (I + 1) / 2 + J;
              if ((T >> 3) != rnd) continue;
              const double* src = smem[T & 1] + ((T >> 1) & 3) * TS;
#pragma unroll
              for (int dr = 0; dr < 2; ++dr)
#pragma unroll
                for (int ds = 0; ds < 2; ++ds) {
                  const int r = 2 * I + dr, s = 2 * J + ds;
                  if (r >= s) L[SL(r, s)] = src[(8 * dr + p) * TB_LD + 8 * ds + q];
                }
            }
          __syncthreads();
        }
      }
    };
      if (role == 0)
        gram_tiles(std::integral_constant<int, 1>{});
      else
        gram_tiles(std::integral_constant<int, 2>{});
    } else {
    v4d acc[NTT];
#pragma unroll
    for (int i = 0; i < NTT; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int tl = lane >> 4;
    // two k-steps in flight: each operand set is reloaded (for k-step ks + 2) right after
    // its MFMAs have issued, so a T load has two k-steps (30 MFMAs) to arrive from L2
    double ta[NT], tb[NT], wa, wb;
    auto tload = [&](double (&t)[NT], double& w, int ks) __attribute__((always_inline)) {
      const GDouble* src = (const GDouble*)md.Tmf + (size_t)ks * NT * 64;
#pragma unroll
      for (int X = 0; X < NT; ++X) t[X] = src[X * 64 + lane];
      w = vbuf[4 * ks + tl];
    };
    auto kstep = [&](const double (&t)[NT], const double wt) __attribute__((always_inline)) {
#pragma unroll
      for (int I = 0; I < NT; ++I) {
        const double av = t[I] * wt;
#pragma unroll
        for (int J = 0; J <= I; ++J) {
          acc[I * (I + 1) / 2 + J] =
              __builtin_amdgcn_mfma_f64_16x16x4f64(av, t[J], acc[I * (I + 1) / 2 + J], 0, 0, 0);
        }
      }
    };
    // an even number of k-steps (Tmf and the weights are zero past n: a padding k-step
    // adds exact zeros), so the loop body has no conditional load and the wait before a
    // set's MFMAs covers only that set (a branch in the body made the compiler wait for
    // both sets at the top of every iteration); the scheduling barriers keep the order
    const int nksp = (md.nks + 1) & ~1;
    tload(ta, wa, 0);
    tload(tb, wb, 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
    for (int ks = 0; ks + 2 < nksp; ks += 2) {
      kstep(ta, wa);
      tload(ta, wa, ks + 2);
      __builtin_amdgcn_sched_barrier(0);
      kstep(tb, wb);
      tload(tb, wb, ks + 3);
      __builtin_amdgcn_sched_barrier(0);
    }
    kstep(ta, wa);
    kstep(tb, wb);
    GST_SUB_END(9)
    // MFMA C layout (col = lane&15, row = lane>>4 + 4 reg) -> cyclic register layout
#pragma unroll
    for (int I = 0; I < NT; ++I) {
#pragma unroll
      for (int J = 0; J <= I; ++J) {
        const v4d a = acc[I * (I + 1) / 2 + J];
#pragma unroll
        for (int g = 0; g < 4; ++g) tbuf[(tl + 4 * g) * TB_LD + (lane & 15)] = a[g];
        lds_order();
#pragma unroll
        for (int dr = 0; dr < 2; ++dr)
#pragma unroll
          for (int ds = 0; ds < 2; ++ds) {
            const int r = 2 * I + dr, s = 2 * J + ds;
            if (r >= s) L[SL(r, s)] = tbuf[(8 * dr + p) * TB_LD + 8 * ds + q];
          }
        lds_order();
      }
    }
    }
    }
    // timing-model prior (1/tm_weight) on its diagonal; unit pivots on the pad columns
#pragma unroll
    for (int s = 0; s < K0; ++s) {
      const int j = 8 * s + q;
      if (p == q) L[SL(s, s)] = (j < md.ntm) ? (L[SL(s, s)] + md.tm_phiinv) + fshift : 1.0;
    }
    CholCtx cc{colq, phbuf, colq2, lane, p, q, raug, 1.0, 0.0, 0, 0, {1.0, 1.0}, {0.0, 0.0}};
    GST_SUB_END(10)
    chol_range_lean<MT, 0, 8 * K0>(L, cc);
    chol_harvest<MT, 0, 8 * K0, RA>(L, cc);
    chol_stats<0, 8 * K0>(cc);
    GST_SUB_END(11)
    tm_apr = cc.apr[0];
    tm_zr = cc.zr[0];
    ld_tm_m = cc.mant;
    ld_tm_e = cc.expo;
    quad_tm = cc.quad;
    fail_tm = cc.fail;
#pragma unroll
    for (int r = K0; r < MT; ++r)
#pragma unroll
      for (int s = K0; s <= r; ++s) S0[64 * SL(r - K0, s - K0)] = L[SL(r, s)];
    // the frozen timing-model columns: parked in global scratch until the b draw
#pragma unroll
    for (int s = 0; s < K0; ++s)
#pragma unroll
      for (int r = s; r < MT; ++r) lr_store(tmf, 512 * tm_slot(MT, r, s), L[SL(r, s)]);
  };

  // log f_k and log df_k of this lane's Fourier column (f = lane; every instance has
  // RA - ntm_pad <= 64), held for the launch: loaded from global memory inside every
  // likelihood they put an L2 round trip in front of each MH step's phi computation
  static_assert(RA - 8 * K0 <= 64, "one Fourier column per lane");
  const bool f_live = lane < RA - md.ntm_pad && lane < md.nf;
  double lfreq_l = f_live ? md.lfreq[lane] : 0.0;
  double ldf_l = f_live ? md.ldf[lane] : 0.0;
  // OCC 2 (256 registers, no AGPRs): held across the sweep the two were spilled and each
  // likelihood reloaded them from scratch right in front of its exp, a memory round trip with
  // nothing behind it.  That build fetches them anew at the top of every MH step instead,
  // ahead of the proposal and the prior, through bounded buffer resources (lanes that are not
  // f_live read past the end and get the 0.0 they held before): hyper_lane_consts
  const int hnlive = max(min(md.nf, RA - md.ntm_pad), 0);
  auto hyper_lane_consts = [&]() __attribute__((always_inline)) {
    if constexpr (OCC == 2) {
      const double *plf = md.lfreq, *pldf = md.ldf;
      asm volatile("" : "+s"(plf), "+s"(pldf));   // per step: not hoisted (and spilled) again
      lfreq_l = lr_load(lane_rows(plf, hnlive, lane), 0);
      ldf_l = lr_load(lane_rows(pldf, hnlive, lane), 0);
    }
  };
  // GEN: the ECORR epoch columns follow the Fourier block (lanes nf .. nf + nec - 1); the
  // lane's ecorr parameter index, or -1
  int geci = -1;
  if constexpr (GEN) {
    const int e = lane - md.nf;
    if (e >= 0 && e < md.nec && lane < RA - md.ntm_pad) geci = md.ecorr_b[md.ecb[e]];
  }

  // GEN: the Fourier block may hold several power-law processes (DevModel::nproc: red | dm |
  // chrom), each over its own run of columns.  The lane's own (log10_A, gamma) indices, fixed
  // for the launch as geci is: lc and g of lnl_hyper are then per-lane values with no select
  // inside the MH loop (lanes past the Fourier block keep process 0's)
  int lane_iA = md.idx_logA, lane_ig = md.idx_gamma;
  if constexpr (GEN) {
    for (int pp = 1; pp < md.nproc; ++pp)
      if (lane >= md.pcol[pp]) {
        lane_iA = md.pidxA[pp];
        lane_ig = md.pidxG[pp];
      }
  }

  // b-marginalised likelihood at xq (gibbs.py:288-329); factor left in L.
  // the descriptor scalars of lnl_hyper, read once for the launch (wave-uniform: scalar
  // registers), not at each of the ~11 calls per sweep
  const int hidxA = md.idx_logA, hidxg = md.idx_gamma, hntmp = md.ntm_pad, hnf = md.nf;
  const double hl12 = md.log_12pi2, hlfyr = md.log_fyr, hslf = md.sum_lfreq,
               hsldf = md.sum_ldf, hldtm = md.logdet_phi_tm;
  const int hnproc = GEN ? md.nproc : 1;
  auto lnl_hyper = [&](const double (&xq)[PX], int& failed) __attribute__((always_inline)) -> double {
    GST_COUNT(16)
    GST_SUB_BEGIN
    // the parameter indices as per-lane values: over a wave-uniform index pget's selects
    // compiled to a cascade of scalar branches in front of every factorisation
    int iA = hidxA, ig = hidxg;
    if constexpr (GEN) {
      iA = lane_iA;
      ig = lane_ig;
    }
    asm("" : "+v"(iA), "+v"(ig));
    const double lA = pget_lane(xq, iA);
    const double g = pget_lane(xq, ig);
    // log phi_k = 2 lA ln10 - log(12 pi^2) + (g-3) log fyr - g log f_k + log df_k
    const double lc = powerlaw_lc(lA, g, hl12, hlfyr);
    // S0 first: its 36 LDS loads are in flight while phi^-1 is computed (exp)
#pragma unroll
    for (int r = K0; r < MT; ++r)
#pragma unroll
      for (int s = K0; s <= r; ++s) L[SL(r, s)] = S0[64 * SL(r - K0, s - K0)];
    // Fourier columns, then the unit-prior dummies that pad a smaller model up to this
    // instance's RA (zero Gram rows: each is eliminated as an exact no-op)
    if constexpr (GEN) {
      // ECORR column of backend b: phi = 10^(2 ecorr_b) (as the large path, gst_large.hpp)
      if (lane < RA - hntmp)
        phbuf[hntmp + lane] =
            f_live ? exp(-(lc - g * lfreq_l + ldf_l)) + fshift
                   : (geci >= 0 ? exp(-2.0 * pget_lane(xq, geci) * LN10) + fshift : 1.0);
    } else {
      // every lane takes the exp (it sat in an exec-masked region of its own; the dummy
      // columns' lanes drop the value)
      const double e = phi_inv_fourier(lc, g, lfreq_l, ldf_l, fshift);
      if (lane < RA - hntmp) phbuf[hntmp + lane] = f_live ? e : 1.0;
    }
    // phbuf doubles as the eliminations' junk rows: restore the one other entry read
    // below, the augmented row's (no prior on the residual column)
    if (lane == 63) phbuf[raug] = 0.0;
    // sum_k log phi_k in closed form (no reduction on the critical path).  nf is converted
    // to double here, from its scalar register: hoisted out of the sweep loop the converted
    // value was spilled, and reloaded from scratch between the statistics and the verdict
    int nfv = hnf;
    asm volatile("" : "+s"(nfv));
    double logdet_phi = logdet_phi_fourier(nfv, lc, g, hslf, hsldf, hldtm);
    if constexpr (GEN) {
      if (hnproc > 1) {
        // several processes: one wave-uniform term each, lc and g read from the first lane of
        // the process's columns
        double ldp = 0.0;
        for (int pp = 0; pp < hnproc; ++pp) {
          const int l0 = md.pcol[pp];
          ldp += logdet_phi_process(md.pcol[pp + 1] - l0, rdlane(lc, l0), rdlane(g, l0),
                                    md.psum_lfreq[pp], md.psum_ldf[pp]);
        }
        logdet_phi = ldp + hldtm;
      }
      for (int b = 0; b < md.nb; ++b)   // log 10^(2 ecorr_b) per ECORR column of backend b
        if (md.ec_count[b] > 0.0)
          logdet_phi += logdet_phi_ecorr(md.ec_count[b], pget(xq, md.ecorr_b[b]));
    }
    lds_order();
    // the prior on the diagonal: every lane reads its row's value (all loads in flight
    // together) and the diagonal lanes keep the sum -- selects, not an exec-masked block of
    // loads each waited for in turn
    double phd[MT - K0];
#pragma unroll
    for (int r = K0; r < MT; ++r) phd[r - K0] = phbuf[8 * r + p];
    // (opaque: a select fed directly by a load is turned back into a branch around the load)
#pragma unroll
    for (int r = K0; r < MT; ++r) asm("" : "+v"(phd[r - K0]));
#pragma unroll
    for (int r = K0; r < MT; ++r) L[SL(r, r)] = (p == q) ? L[SL(r, r)] + phd[r - K0] : L[SL(r, r)];
    CholCtx cc{colq, phbuf, colq2, lane, p, q, raug, 1.0, 0.0, 0, 0, {1.0, 1.0}, {0.0, 0.0}};
    GST_SUB_END(7)
    chol_range<MT, K0, RA, kp_for(OCC)>(L, cc);
    GST_SUB_END(8)
    // the statistics where the elimination left them (no harvest: harvest_factor, once per
    // sweep).  The augmented row's diagonal element before the elimination comes from S0 again,
    // through the lane's own S0 address: held in a register across the elimination it would
    // add to the spill of the two-chains-per-SIMD build
    chol_stats_diag<MT, 8 * K0, RA, RA>(
        L, cc, rdlane(S0[64 * SL(RA / 8 - K0, RA / 8 - K0)], 9 * (RA % 8)));
    GST_SUB_END(19)
    const double mant = cc.mant, quad = cc.quad;
    const int expo = cc.expo;
    failed = cc.fail | fail_tm;
    if (failed) return -INFINITY;
    // log|Sigma| = sum log a_kk (pivots of the LDL^T-scaled elimination)
    const double ld_sigma = log(ld_tm_m * mant) + (double)(ld_tm_e + expo) * LN2;
    return marginal_ll(logdetN, rNr, quad_tm + quad, ld_sigma, logdet_phi);
  };
  // The pivots and augmented-row entries of the factor lnl_hyper left in L, gathered onto
  // lane k % 64 behind the timing-model columns' for floor_shift and the b draw: once per
  // sweep (and floor pass) at the final x, where they are consumed, not per likelihood
  auto harvest_factor = [&]() __attribute__((always_inline)) {
    CholCtx cc{colq, phbuf, colq2, lane, p, q, raug, 1.0, 0.0, 0, 0, {tm_apr, 1.0}, {tm_zr, 0.0}};
    chol_harvest<MT, 8 * K0, RA, RA>(L, cc);
    f_apr[0] = cc.apr[0];
    f_apr[1] = cc.apr[1];
    f_zr[0] = cc.zr[0];
    f_zr[1] = cc.zr[1];
  };

  // pair mode: both waves write the records (identical state): b and the TOA slots split
  const bool rec_on = record_every > 0 && !eval_only && (PAIR || role == 0);
  int hacc = 0, hrej = 0;   // pair mode: hyper-MH acceptance history (branch prediction)
  GST_STAMP_START
  compute_Tb();
  if (eval_only) nsweeps = 1;

#pragma unroll 1
  for (int it = 0; it < nsweeps; ++it) {
    if (OCC == 2 && st.prog) {
      // last sweep's ticket (arrived long ago): behind if fewer sweeps than the average
      if (it > 0) {
        const unsigned long long g = __builtin_amdgcn_readfirstlane((unsigned)prog_ret) |
                                     ((unsigned long long)__builtin_amdgcn_readfirstlane(
                                          (unsigned)(prog_ret >> 32)) << 32);
        fair.behind = (unsigned long long)(it - 1) * (unsigned long long)C < g ? 1 : 0;
      }
      // (this sweep's ticket is taken after its Gram, gram_and_tm's caller below)
    }
    fair_prio<OCC>(fair);
    rng.sweep = (uint32_t)(sweep0 + it);
    const double* tp = TAPE ? tape.data + ((size_t)c * nsweeps + it) * tape.stride : nullptr;
    if (st.debug & 1) {
      // GST_DEBUG_POISON: between two sweeps a chain's state is exactly what the records
      // hold (x, b, z, alpha, pout, theta, nu; y = r - T b and the z bits in registers are
      // functions of it), so every LDS word of the chain and its parked timing-model factor
      // are dead here.  Overwrite them with a NaN pattern: a sweep that read any of them
      // before writing it would carry the NaN into its draws, and the chains would no longer
      // be bitwise those of an ordinary launch (tests/test_gpu_invariants.py).
      const double poison = __longlong_as_double(0x7ff4dead7ff4deadll);
      for (int j = lane; j < lds_doubles(MT, K0); j += 64) smem[wv][j] = poison;
      for (int j = 0; j < NTMS; ++j) lr_store(tmf, 512 * j, poison);
      lds_order();
    }

    // ---- record the state at the start of the sweep (gibbs.py:355-361)
    if (rec_on && (it % record_every) == 0) {
      const int ri = it / record_every;
      if (ri < rec.nrec) {
        const size_t base = (size_t)c * rec.nrec + ri;
        if (rec.x && lane < P && role == 0) rec.x[base * P + lane] = pget(xv, lane);
        // from the state row, not bsc: bsc shares S0R with S0 and is stale after a sweep
        // that skipped the b draw (gibbs.py:373)
        if (rec.b)
          for (int j = lane + 64 * role; j < m; j += (PAIR ? 128 : 64)) rec.b[base * m + j] = brow[j];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const int t = 64 * s + lane;
          if ((vmask & (1u << s)) && (!PAIR || (s & 1) == role)) {
            if (rec.z) rec.z[base * nst + t] = (double)((zb >> s) & 1u);
            if (rec.alpha) rec.alpha[base * nst + t] = al[s];
            if (rec.pout) rec.pout[base * nst + t] = po[s];
          }
        }
        if (lane == 0 && role == 0) {
          if (rec.theta) rec.theta[base] = theta;
          if (rec.nu) rec.nu[base] = nu;
        }
      }
    }

    // ---- posterior sums (gst_set_accum): the same state, added into the caller's running
    // sums on every sweep from from_sweep on.  Each element has one owner (the records' split:
    // pair mode divides the b columns and the TOA slots by role) and is a plain read-modify-
    // write in sweep order, so a sum is bitwise the sequential sum of the records.  The host
    // launches an ACC instance only while sums are set (never eval_only or GST_STAGE_GRAM).
    if constexpr (ACC) {
      // the descriptor is read here with scalar loads each sweep, not kept in registers
      // across the sweep: the asm keeps the loads from being hoisted out of the loop
      const DevAccum* ap = accum_desc(st.gram_cnt);
      asm volatile("" : "+s"(ap));
      const __attribute__((address_space(4))) DevAccum& A =
          *(const __attribute__((address_space(4))) DevAccum*)ap;
      if (sweep0 + it >= A.from_sweep) {
        if (double* const sb = A.b_sum)
          for (int j = lane + 64 * role; j < m; j += (PAIR ? 128 : 64)) sb[(size_t)c * m + j] += brow[j];
        if (double* const sq = A.b_sq)
          for (int j = lane + 64 * role; j < m; j += (PAIR ? 128 : 64)) {
            const double v = brow[j];
            sq[(size_t)c * m + j] += v * v;
          }
        double* const sz = A.z_sum;
        double* const sa = A.alpha_sum;
        double* const sp = A.pout_sum;
        // gst_set_accum_toa: exceedance counts of pout at A.nthr thresholds (strict compare,
        // a plane of A.gt_plane doubles per threshold) and the sums of y = r - T b and y^2;
        // yv is the y of the b the sums above read (compute_Tb follows every b draw)
        double* const sg = A.pout_gt;
        double* const sy = A.resid_sum;
        double* const sy2 = A.resid_sq;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const size_t e = (size_t)c * nst + 64 * s + lane;
          if ((vmask & (1u << s)) && (!PAIR || (s & 1) == role)) {
            if (sz) sz[e] += (double)((zb >> s) & 1u);
            if (sa) sa[e] += al[s];
            if (sp) sp[e] += po[s];
            if (sg) {
#pragma unroll 1
              for (int k = 0; k < A.nthr; ++k)
                sg[(size_t)k * A.gt_plane + e] += po[s] > A.thr[k] ? 1.0 : 0.0;
            }
            if (sy) sy[e] += yv[s];
            if (sy2) sy2[e] += yv[s] * yv[s];
          }
        }
        if (lane == 0 && role == 0)
          if (long long* const cnt = A.count) cnt[c] += 1;
        // gst_set_accum_block: the packed lower triangle of b b^T over the columns
        // [bb_col0, bb_col0 + bb_ncol) of the state row.  Row i belongs to one wave (pair mode:
        // role i & 1), element (i, j) to lane j & 63: a lane holds its one or two b_j for the
        // whole pass (m <= MP <= 128) and reads the wave-uniform b_i from the owning lane.  The
        // read-modify-writes of BBG rows are in flight together, one wait per group, and the
        // group loop stays rolled: the instances are at the register limit.
        if (double* const bo = A.bb) {
          static_assert(MP <= 128, "a lane holds two columns of the block");
          constexpr int BBG = 8;
          constexpr int RSTEP = PAIR ? 2 : 1;
          const int c0 = A.bb_col0, K = A.bb_ncol;
          double* const tri = bo + (size_t)c * (size_t)(K * (K + 1) / 2);
          const double bj0 = lane < K ? brow[c0 + lane] : 0.0;
          const double bj1 = lane + 64 < K ? brow[c0 + 64 + lane] : 0.0;
          // columns j = lane of every row
#pragma unroll 1
          for (int i0 = role; i0 < K; i0 += BBG * RSTEP) {
            double v[BBG];
#pragma unroll
            for (int g = 0; g < BBG; ++g) {
              const int i = i0 + g * RSTEP;
              v[g] = (i < K && lane <= i) ? tri[i * (i + 1) / 2 + lane] : 0.0;
            }
#pragma unroll
            for (int g = 0; g < BBG; ++g) {
              const int i = i0 + g * RSTEP;
              if (i < K) {
                const double bi = rdlane(i < 64 ? bj0 : bj1, i & 63);
                if (lane <= i) tri[i * (i + 1) / 2 + lane] = v[g] + bi * bj0;
              }
            }
          }
          // columns j = 64 + lane of the rows i >= 64
#pragma unroll 1
          for (int i0 = 64 + role; i0 < K; i0 += BBG * RSTEP) {
            double v[BBG];
#pragma unroll
            for (int g = 0; g < BBG; ++g) {
              const int i = i0 + g * RSTEP;
              v[g] = (i < K && lane + 64 <= i) ? tri[i * (i + 1) / 2 + 64 + lane] : 0.0;
            }
#pragma unroll
            for (int g = 0; g < BBG; ++g) {
              const int i = i0 + g * RSTEP;
              if (i < K) {
                const double bi = rdlane(bj1, i & 63);
                if (lane + 64 <= i) tri[i * (i + 1) / 2 + 64 + lane] = v[g] + bi * bj1;
              }
            }
          }
        }
      }
    }

    const double x_last0 = pget(xv, P - 1);  // chain[ii, -1]
    GST_SUB_BEGIN
    if (!eval_only) mh_variates(tp);
    GST_SUB_END(20)
    GST_STAMP(0)

    // ---- white-noise MH block (gibbs.py:114-143); step -1 = the initial lnlike0
    if ((mask & 1u) && !eval_only && !GEN && md.ncls > 0) {
      // Noise-class path: a likelihood is a few scalar ops (no TOA reduction), so the
      // block is a serial chain of log/divide latencies.  Evaluate it speculatively:
      // for the next D steps, lane 2^j - 1 + b evaluates step s0+j's proposal on the
      // accept/reject path b (bit i = step s0+i accepted); the decisions are then read
      // back lane by lane.  Every value is computed with the sequential code's exact
      // operation order, so the decisions and the final state are bitwise identical.
      GST_SUB_BEGIN
      white_prep();
      GST_SUB_END(21)
      constexpr int D = 6;
      double Wu[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) Wu[u] = (u < md.ncls) ? rdlane(wcls, u) : 0.0;
      auto lnl_lane = [&](const double (&xq)[PX], double Q) __attribute__((always_inline)) -> double {
        const double ef2 = efac2_of(xq);
        if (md.ncls == 1) {
          const double N0 = ef2 * md.csig2[0] + Q;
          return -0.5 * ((wcls_la + md.ccount[0] * log(N0)) + Wu[0] / N0);
        }
        double sl = 0.0, sq = 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (u < md.ncls) {
            const double N0 = ef2 * md.csig2[u] + Q;
            sl += md.ccount[u] * log(N0);
            sq += Wu[u] / N0;
          }
        }
        return -0.5 * ((sl + wcls_la) + sq);
      };
      const int ieq = md.idx_equad;
      double Qx = pow10_2(pget(xv, ieq));
      double l0 = lnl_lane(xv, Qx), p0 = lnprior(xv);
      // this lane's node: level j, path b
      const int node = lane + 1;
      const int j = 31 - __builtin_clz(node);          // node in [2^j, 2^(j+1))
      const int b = node - (1 << j);
#pragma unroll 1
      for (int s0 = 0; s0 < NWHITE; s0 += D) {
        const int nd = (NWHITE - s0) < D ? (NWHITE - s0) : D;
        GST_SUB_BEGIN
        // the round's D steps (parameter, delta, log u, 10^(2 delta)) in registers: every
        // LDS load issues up front, and each lane's walk down its path is straight-line
        // selects instead of a divergent loop of dependent loads
        int pr[D];
        double dl[D], lu[D], ev[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const int gs = (s0 + i) < NWHITE ? s0 + i : NWHITE - 1;
          pr[i] = (int)mhw[4 * gs + 0];
          dl[i] = mhw[4 * gs + 1];
          lu[i] = mhw[4 * gs + 2];
          ev[i] = mhw[4 * gs + 3];
        }
        double xq[PX], Q = Qx;
#pragma unroll
        for (int t = 0; t < PX; ++t) xq[t] = xv[t];
#pragma unroll
        for (int i = 0; i < D - 1; ++i) {
          const bool on = i < j && ((b >> i) & 1);
#pragma unroll
          for (int t = 0; t < PX; ++t) xq[t] = (on && t == pr[i]) ? xq[t] + dl[i] : xq[t];
          Q = (on && pr[i] == ieq) ? Q * ev[i] : Q;
        }
        // the proposal of step s0 + j from the node's state (propose(): q[par] += delta)
        int par = pr[0];
        double delta = dl[0], E = ev[0];
#pragma unroll
        for (int i = 1; i < D; ++i) {
          par = j == i ? pr[i] : par;
          delta = j == i ? dl[i] : delta;
          E = j == i ? ev[i] : E;
        }
        double qv[PX];
#pragma unroll
        for (int t = 0; t < PX; ++t) qv[t] = (t == par) ? xq[t] + delta : xq[t];
        double p1 = -INFINITY, l1 = 0.0;
        if (j < nd) {
          const double Qq = (par == ieq) ? Q * E : Q;
          p1 = lnprior(qv);
          if (p1 != -INFINITY) l1 = lnl_lane(qv, Qq);
        }
        GST_SUB_END(22)
        int path = 0;
#pragma unroll
        for (int jj = 0; jj < D; ++jj) {
          if (jj < nd) {
            const int L = (1 << jj) - 1 + path;
            const double pl = rdlane(p1, L);
            const double ll = rdlane(l1, L);
            if (pl != -INFINITY && (ll + pl) - (l0 + p0) > lu[jj]) {
              l0 = ll;
              p0 = pl;
              path |= 1 << jj;
            }
          }
        }
        GST_SUB_END(15)
        // apply the accepted moves in order (the sequential code's xv = qv, Qx = Qq)
#pragma unroll
        for (int i = 0; i < D; ++i) {
          const bool on = i < nd && ((path >> i) & 1);
#pragma unroll
          for (int t = 0; t < PX; ++t) xv[t] = (on && t == pr[i]) ? xv[t] + dl[i] : xv[t];
          Qx = (on && pr[i] == ieq) ? Qx * ev[i] : Qx;
        }
      }
    } else if ((mask & 1u) || eval_only) {
      white_prep();
      double l0 = 0.0, p0 = 0.0;
      double Qx = pow10_2(pget(xv, hieq));
#pragma unroll 1
      for (int step = -1; step < NWHITE; ++step) {
        if ((step & 3) == 0) fair_prio<OCC>(fair);
        double qv[PX], luacc = 0.0, Qq = Qx;
        if (step < 0) {
#pragma unroll
          for (int j = 0; j < PX; ++j) qv[j] = xv[j];
        } else {
          double E;
          int par;
          luacc = propose(xv, qv, step, E, par);
          if (par == hieq) Qq = Qx * E;
        }
        const double p1 = lnprior(qv);
        // out-of-prior: (l1 + -inf) - (l0 + p0) is -inf or NaN, never > log(u): skip lnL
        if (step >= 0 && p1 == -INFINITY) continue;
        GST_SUB_BEGIN
        const double l1 = lnl_white(qv, Qq);
        GST_SUB_END(15)
        if (step < 0) {
          l0 = l1;
          p0 = p1;
          if (eval_only) {
            if (lane == 0) out_w[c] = l1;
            break;
          }
          continue;
        }
        if ((l1 + p1) - (l0 + p0) > luacc) {
#pragma unroll
          for (int j = 0; j < PX; ++j) xv[j] = qv[j];
          l0 = l1;
          p0 = p1;
          Qx = Qq;
        }
      }
    }

    GST_STAMP(1)
    // ---- Gram + red-noise hyper MH block (gibbs.py:80-111, 288-329) + b draw (145-182)
    // step -1: initial lnlike0; steps 0..9: proposals; step NHYPER: refactor at the final
    // x for the b draw when the factor left in registers belongs to a rejected proposal.
    bool redraw = false;
    int fb = 0;
    int owner = 0;   // the wave whose registers hold the factor at the final x (pair mode)
    if constexpr (PAIR) {
      if (mask & 6u) {
        double l0 = 0.0, p0 = 0.0;
        owner = -1;
        bool init = (mask & 2u) != 0;
        int j = init ? 0 : NHYPER, rp = 0;
        // first step >= s whose proposal from xb is inside the prior (the others are
        // rejected without a likelihood, gibbs.py:100-104 with lnprior = -inf)
        auto next_in = [&](const double (&xb)[PX], int s) __attribute__((always_inline)) -> int {
          for (; s < NHYPER; ++s) {
            double qv[PX], E;
            int par;
            (void)propose(xb, qv, NWHITE + s, E, par);
            if (lnprior(qv) != -INFINITY) break;
          }
          return s;
        };
        // one sequential MH step (gibbs.py:99-110) at step s with the lnL of its point
        auto decide = [&](int s, double l1, bool f1, int who) __attribute__((always_inline)) {
          if (f1) status |= 1;
          double qv[PX], E;
          int par;
          const double luacc = propose(xv, qv, NWHITE + s, E, par);
          const double p1 = lnprior(qv);
          if ((l1 + p1) - (l0 + p0) > luacc) {
            GST_COUNT(18)
#pragma unroll
            for (int t = 0; t < PX; ++t) xv[t] = qv[t];
            l0 = l1;
            p0 = p1;
            owner = who;
            ++hacc;
            return true;
          }
          owner = -1;
          ++hrej;
          return false;
        };
        // pass 1 (rare): the b draw's factor at the SVD noise floor, Sigma + f I (floor_shift)
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
        gram_and_tm(xv);   // both waves: identical S0 in each wave's own LDS region
        if (fail_tm) status |= 1;
        GST_STAMP(2)
        // Each round wave 0 evaluates the next point the sequential sampler needs (the
        // initial x, then the next in-prior proposal sa) and wave 1 a speculative one: the
        // step after sa on the branch (accept / reject) the chain's acceptance history
        // predicts, else on the other branch, else -- no proposal left -- the current x
        // (the reject branch's final state, for the b draw).  A last round refactors the
        // final x when no wave holds its factor and the b draw needs it.
#pragma unroll 1
        while (true) {
          const int sa = init ? -1 : next_in(xv, j);
          bool fin = false;
          if (sa >= NHYPER) {
            if (!(mask & 4u)) break;
            redraw = true;
#pragma unroll
            for (int t = 0; t < PX; ++t)
              if (t < P) redraw = redraw && (xv[t] != x_last0);      // gibbs.py:373
            if (mask & 128u) redraw = true;
            if (!redraw || owner >= 0) break;
            fin = true;
          }
          double qa[PX];
#pragma unroll
          for (int t = 0; t < PX; ++t) qa[t] = xv[t];
          int kind = 0, sb = NHYPER;   // wave 1: 0 idle, 1 accept branch, 2 reject branch, 3 x
          if (!fin) {
            if (!init) {
              double E;
              int par;
              (void)propose(xv, qa, NWHITE + sa, E, par);
            }
            const int sbR = next_in(xv, sa + 1);
            const int sbA = init ? NHYPER : next_in(qa, sa + 1);
            if (!init && hacc >= hrej && sbA < NHYPER) {
              kind = 1;
              sb = sbA;
            } else if (sbR < NHYPER) {
              kind = 2;
              sb = sbR;
            } else if (!init && (mask & 4u) && owner != 1) {
              kind = 3;
            }
          }
          hyper_lane_consts();
          double xq[PX];
#pragma unroll
          for (int t = 0; t < PX; ++t) xq[t] = role == 0 ? qa[t] : xv[t];
          if (role == 1 && (kind == 1 || kind == 2)) {
            double E;
            int par;
            (void)propose(kind == 1 ? qa : xv, xq, NWHITE + sb, E, par);
          }
          GST_COUNT(17)
          double lm = 0.0;
          int fm = 0;
          if (role == 0 || kind != 0) lm = lnl_hyper(xq, fm);
          if (lane == 0) {
            xchg[rp][role][0] = lm;
            xchg[rp][role][1] = (double)fm;
          }
          __syncthreads();
          const double lA = xchg[rp][0][0], lB = xchg[rp][1][0];
          const bool fA = xchg[rp][0][1] != 0.0, fB = xchg[rp][1][1] != 0.0;
          rp ^= 1;   // the next round writes the other buffer: no second barrier needed
          if (fin) {
            fb = fA;
            owner = 0;
            break;
          }
          const int prev = owner;
          if (init) {
            if (fA) status |= 1;
            l0 = lA;
            p0 = lnprior(xv);
            owner = fA ? -1 : 0;
            init = false;
            j = NHYPER;
            if (kind == 2) {
              decide(sb, lB, fB, 1);
              j = sb + 1;
            }
          } else if (decide(sa, lA, fA, 0)) {
            j = sa + 1;
            if (kind == 1) {
              decide(sb, lB, fB, 1);
              j = sb + 1;
            }
          } else {
            j = sa + 1;
            if (kind == 2) {
              decide(sb, lB, fB, 1);
              j = sb + 1;
            } else if (kind == 3) {
              owner = fB ? -1 : 1;
            } else if (kind == 0 && prev == 1) {
              owner = 1;   // wave 1 sat out: its factor of x is intact
            }
          }
        }
        if (redraw && !fb && role == owner) harvest_factor();
        if (pass == 1 || !redraw || fb || (st.debug & DEBUG_EXACT_BDRAW)) break;
        // the owner wave holds the factor at the final x; both waves take its floor decision
        const double fs =
            role == owner ? floor_shift(f_apr, lane, md.ntm, md.ntm_pad, md.ntm_pad + md.nf + (GEN ? md.nec : 0)) : 0.0;
        if (role == owner && lane == 0) xfloor[0] = fs;
        __syncthreads();
        fshift = xfloor[0];
        __syncthreads();
        if (fshift == 0.0) break;
        status |= STATUS_FLOOR;
        ++nfloor;
        owner = -1;   // a final round refactors x (the MH decisions stand)
        init = false;
        j = NHYPER;
        }
        fshift = 0.0;
      }
    } else if ((mask & (6u | 256u)) || eval_only) {
      bool Lvalid = false;
      double l0 = 0.0, p0 = 0.0;
      // GST_STAGE_GRAM (256, timing diagnostic): the Gram and the timing-model elimination only
      const int first = (mask & 256u) ? NHYPER + 1 : (((mask & 2u) || eval_only) ? -1 : NHYPER);
      // pass 1 (rare): the registers hold the factor at the final x and Sigma is beyond fp64
      // resolution -- refactor x's Sigma + f I for the b draw (floor_shift; the MH decisions
      // stand).  One copy of the Gram / hyper-block code serves both passes (an inlined
      // second copy of it raised the 256-register build's spill)
#pragma unroll 1
      for (int pass = 0; pass < 2; ++pass) {
      gram_and_tm(xv);
      // the sweep's progress ticket (fair_prio), issued where only LDS and register work
      // follows (the hyper MH) and its value is used at the next sweep's start (taken at the
      // sweep's start, the atomic's latency stalled the record / MH-variate stage; round-5
      // A/B: 20-sweep line +1%, 500 sweeps unchanged).  In the OCC 2 build the return is still
      // waited for here, once per sweep: the ticket is spilled, and the spill store needs it
      // 
      if (OCC == 2 && st.prog && pass == 0 && lane == 0)
        prog_ret = __hip_atomic_fetch_add(st.prog, 1ull, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
      if (fail_tm) status |= 1;
      GST_STAMP(2)
      GST_SUB_BEGIN
#pragma unroll 1
      for (int step = pass ? NHYPER : first; step <= NHYPER; ++step) {
        fair_prio<OCC>(fair);
        hyper_lane_consts();
        double qv[PX], luacc = 0.0;
        if (step == NHYPER) {
          if (eval_only || !(mask & 4u)) break;
          redraw = true;
#pragma unroll
          for (int j = 0; j < PX; ++j)
            if (j < P) redraw = redraw && (xv[j] != x_last0);   // gibbs.py:373
          if (mask & 128u) redraw = true;                        // direct update_b call
          if (!redraw || Lvalid) break;
        }
        if (step < 0 || step == NHYPER) {
#pragma unroll
          for (int j = 0; j < PX; ++j) qv[j] = xv[j];
        } else {
          double E;
          int par;
          luacc = propose(xv, qv, NWHITE + step, E, par);
        }
        const double p1 = lnprior(qv);
        if (step >= 0 && step < NHYPER && p1 == -INFINITY) continue;
        int f1 = 0;
        GST_SUB_END(27)
        const double l1 = lnl_hyper(qv, f1);
        if (step == NHYPER) {
          fb = f1;
          break;
        }
        if (f1) status |= 1;
        if (step < 0) {
          l0 = l1;
          p0 = p1;
          // a failed initial factorisation is no factor to draw b from: if every proposal
          // is then skipped, step NHYPER refactors (and flags status 2) instead
          Lvalid = !f1;
          if (eval_only) {
            if (lane == 0) out_h[c] = l1;
            break;
          }
          continue;
        }
        if ((l1 + p1) - (l0 + p0) > luacc) {
          GST_COUNT(18)
#pragma unroll
          for (int j = 0; j < PX; ++j) xv[j] = qv[j];
          l0 = l1;
          p0 = p1;
          Lvalid = true;
        } else {
          Lvalid = false;
        }
        GST_SUB_END(26)
      }
      // the factor in L is the accepted last step's or step NHYPER's: at the final x
      if (!eval_only && redraw && !fb) harvest_factor();
      if (pass == 1 || eval_only || !redraw || fb || (st.debug & DEBUG_EXACT_BDRAW)) break;
      fshift = floor_shift(f_apr, lane, md.ntm, md.ntm_pad, md.ntm_pad + md.nf + (GEN ? md.nec : 0));
      if (__builtin_expect(fshift == 0.0, 1)) break;
      status |= STATUS_FLOOR;
      ++nfloor;
      Lvalid = false;
      }
      fshift = 0.0;
    }
    if (eval_only) return;
    GST_STAMP(3)

    bool drew = false;
    if (redraw && role == owner) {
      if (fb) {
        status |= 2;
      } else {
        drew = true;
        GST_SUB_BEGIN
#pragma unroll
        for (int s = 0; s < K0; ++s)
#pragma unroll
          for (int r = s; r < MT; ++r) L[SL(r, s)] = lr_load(tmf, 512 * tm_slot(MT, r, s));
        // y_k = 1/sqrt(a_kk); z = L^-1 d has z_k = zraw_k * y_k; L_ik = a_ik * y_k
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          const int j = 64 * sl + lane;
          if (j < MP) {
            apiv[j] = f_apr[sl];
            zraw[j] = f_zr[sl];
          }
        }
        lds_order();
        for (int j = lane; j < raug; j += 64) yinv[j] = rsqrt_nr(apiv[j]);
        lds_order();
        // rhs w = z + eta
        if (TAPE) {
          // eta = L^T Delta, so that L^-T eta equals the reference's U S^-1/2 xi
          for (int j = lane; j < MP; j += 64) xbuf[j] = 0.0;
          lds_order();
          for (int j = lane; j < m; j += 64) xbuf[md.ref2int[j]] = tp[TP_DELTA + j];
          lds_order();
#pragma unroll
          for (int s = 0; s < MT; ++s) {
            double part = 0.0;
            const int j = 8 * s + q;
#pragma unroll
            for (int r = s; r < MT; ++r) {
              const int i = 8 * r + p;
              part += (i >= j && i < raug) ? L[SL(r, s)] * xbuf[i] : 0.0;
            }
            part += __shfl_xor(part, 8, 64);
            part += __shfl_xor(part, 16, 64);
            part += __shfl_xor(part, 32, 64);
            if (p == 0 && j < raug) wvec[j] = (zraw[j] + part) * yinv[j];
          }
        } else {
          // normals 2l and 2l + 1 of the b-draw stream from lane l's one Philox draw
          if (2 * lane < raug) {
            double n0, n1;
            normal_pair(rng, (uint32_t)lane, TAG_BDRAW, n0, n1);
            const int j0 = 2 * lane, j1 = 2 * lane + 1;
            wvec[j0] = zraw[j0] * yinv[j0] + n0;
            if (j1 < raug) wvec[j1] = zraw[j1] * yinv[j1] + n1;
          }
        }
        lds_order();
        GST_SUB_END(12)
        // back substitution L^T v = w, descending columns:
        // v_k = (w_k - y_k * sum_{i>k} a_ik v_i) * y_k
        double vr[MT];
#pragma unroll
        for (int r = 0; r < MT; ++r) vr[r] = 0.0;
#pragma unroll
        for (int K = MT - 1; K >= 0; --K) {
          // rows of the slots below K are solved: their part of every column 8K+q is one
          // per-lane sum, reduced over p once per slot column (every lane (p, q) gets the
          // sum of column 8K+q); the 8 in-slot columns are then solved with uniform values
          double pe = 0.0, po2 = 0.0;
#pragma unroll
          for (int r = K + 1; r < MT; r += 2) {
            pe = fma(L[SL(r, K)], vr[r], pe);
            if (r + 1 < MT) po2 = fma(L[SL(r + 1, K)], vr[r + 1], po2);
          }
          double acc = pe + po2;
          acc += dpp<DPP_ROR8>(acc);  // (l + 8) mod 16 == l ^ 8: p and p ^ 1
          acc += __shfl_xor(acc, 16, 64);
          acc += __shfl_xor(acc, 32, 64);
          // diagonal block, transposed through LDS: dcol[i] = a_{8K+i, 8K+q}
          tdg[8 * q + p] = L[SL(K, K)];
          lds_order();
          double dcol[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) dcol[i] = tdg[8 * q + i];
          const int kq = 8 * K + q;
          const double wq = wvec[kq], yq = yinv[kq];
          lds_order();
          double vmine = 0.0;
#pragma unroll
          for (int kk = 7; kk >= 0; --kk) {
            if (8 * K + kk >= raug) continue;
            // lanes q == kk now hold sum_{i>k} a_ik v_i of column k = 8K + kk
            const double vq = (wq - yq * acc) * yq;
            const double vk = rdlane(vq, kk);
            vmine = (q == kk) ? vk : vmine;
            acc = fma(dcol[kk], vk, acc);  // row k's term of the columns q < kk
          }
          xbuf[kq] = vmine;  // zero for the pad columns k >= raug
          lds_order();
          vr[K] = xbuf[8 * K + p];
        }
        lds_order();
        GST_SUB_END(13)
        for (int j = lane; j < m; j += 64) {
          const double bj = xbuf[md.ref2int[j]];
          bsc[j] = bj;
          brow[j] = bj;                   // the state array is the chain's b
        }
        lds_order();
        compute_Tb();
        GST_SUB_END(14)
      }
    }
    if constexpr (PAIR) {
      // hand the new b to the other wave: its copy of bsc, then its own y = r - T b
      if (mask & 6u) {
        if (drew) {
          double* pb = smem[role ^ 1] + (bsc - smem[role]);
          for (int j = lane; j < m; j += 64) pb[j] = bsc[j];
          // and its y = r - T b (compute_Tb's values: the partner copies them instead of
          // repeating the T b product)
          if (owner >= 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) xyv[s][lane] = yv[s];
          }
        }
        if (role == (owner >= 0 ? owner : 0) && lane == 0) xdrew[0] = drew ? 1 : 0;
        __syncthreads();
        const bool got = xdrew[0] != 0;
        if (got && role != owner) {
          if (owner >= 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) yv[s] = xyv[s][lane];
          } else {
            compute_Tb();
          }
        }
        __syncthreads();   // xdrew and xyv are rewritten next sweep
      }
    }

    GST_STAMP(4)
    fair_prio<OCC>(fair);
    GST_SUB_BEGIN
    // ---- outlier block: theta (gibbs.py:185-198)
    const double ef2 = efac2_of(xv);
    const double Q = pow10_2(pget(xv, md.idx_equad));
    const bool mix = (md.model == 2) || (md.model == 3);
    if ((mask & 8u) && mix) {
      int zs = 0;
#pragma unroll
      for (int s = 0; s < NS; ++s) zs += __popcll(__ballot(((zb & vmask) >> s) & 1u));
      const double a = (double)zs + md.mk;
      const double b = ((double)n - (double)zs) + md.k1mm;
      if (TAPE) {
        theta = tp[TP_DELTA + m];
      } else {
        // Gamma(a) on lane 0, Gamma(b) on lane 1 (and its copies), side by side
        const double g = gamma_mt(lane == 0 ? a : b, rng, lane == 0 ? 0u : 1u, TAG_THETA);
        const double ga = rdlane(g, 0), gb = rdlane(g, 1);
        theta = ga / (ga + gb);
      }
    }
    fair_prio<OCC>(fair);
    GST_SUB_END(23)
    // ---- z (gibbs.py:201-226)
    // pair mode: each wave draws z and alpha for its half of the TOA slots (Philox is keyed
    // by TOA, so every draw is the one the single-wave kernel makes) and takes the other
    // half from its partner through LDS
    const unsigned mine = PAIR ? (vmask & (role ? 0xAAAAAAAAu : 0x55555555u)) : vmask;
    if ((mask & 16u) && mix) {
      const double SQ2PI = 2.5066282746310002;  // np.sqrt(2*np.pi)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (mine & (1u << s)) {
          const int t = 64 * s + lane;
          double N0;
          if constexpr (GEN)
            N0 = gen_n0(xv, S2(s), gef[s], geq[s]);
          else
            N0 = ef2 * S2(s) + Q;
          const double Nv = al[s] * N0;
          const double y = yv[s];
          const double sd1 = sqrt(Nv);
          const double x1 = y / sd1;
          double top = theta * (exp(-(x1 * x1) / 2.0) / SQ2PI / sd1);
          if (md.model == 3) top = theta / md.pspin;
          const double sd0 = sqrt(N0);
          const double x0 = y / sd0;
          const double bot = top + (1.0 - theta) * (exp(-(x0 * x0) / 2.0) / SQ2PI / sd0);
          double qz = top / bot;
          if (isnan(qz)) qz = 1.0;
          po[s] = qz;
          const double pz = qz < 1.0 ? qz : 1.0;
          double u;
          if (TAPE) {
            u = tp[TP_DELTA + m + 1 + t];
          } else {
            double unused;
            rng.uniform2((uint32_t)t, TAG_Z, u, unused);
          }
          const int zz = bern_legacy(pz, u);
          zb = (zb & ~(1u << s)) | ((unsigned)zz << s);
        }
      }
      if constexpr (PAIR) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const unsigned long long bm = __ballot((zb >> s) & 1u);
          if ((s & 1) == role) {
            xpo[s][lane] = po[s];
            if (lane == 0) xzm[s] = bm;
          }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if ((s & 1) != role) {
            po[s] = xpo[s][lane];
            zb = (zb & ~(1u << s)) | ((unsigned)((xzm[s] >> lane) & 1ull) << s);
          }
        }
        // the partner's reads complete before either wave can overwrite its slots again
        // (a later sweep's z stage; a launch's stage mask need not hold a barrier between)
        __syncthreads();
      }
    }
    fair_prio<OCC>(fair);
    GST_SUB_END(24)
    // ---- alpha (gibbs.py:229-242)
    if ((mask & 32u) && md.vary_alpha) {
      int zs = 0;
#pragma unroll
      for (int s = 0; s < NS; ++s) zs += __popcll(__ballot(((zb & vmask) >> s) & 1u));
      if (zs >= 1) {
        double G[NS];
        if (TAPE) {
#pragma unroll
          for (int s = 0; s < NS; ++s) G[s] = tp[TP_DELTA + m + 1 + nst + 64 * s + lane];
        } else {
          // all of the lane's TOAs in one rejection loop (independent draws, so their
          // Philox / log / sqrt chains interleave); each TOA's variates and acceptance
          // sequence are exactly gamma_mt's (the large path draws them that way)
          double sh[NS];
#pragma unroll
          for (int s = 0; s < NS; ++s) sh[s] = ((double)((zb >> s) & 1u) + nu) / 2.0;
          gamma_mt_slots<NS>(sh, mine, rng, (uint32_t)lane, TAG_ALPHA, G);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (mine & (1u << s)) {
            const double zf = (double)((zb >> s) & 1u);
            double N0;
            if constexpr (GEN)
              N0 = gen_n0(xv, S2(s), gef[s], geq[s]);
            else
              N0 = ef2 * S2(s) + Q;
            const double top = ((yv[s] * yv[s]) * zf / N0 + nu) / 2.0;
            al[s] = top / G[s];
          }
        }
        if constexpr (PAIR) {
#pragma unroll
          for (int s = 0; s < NS; ++s)
            if ((s & 1) == role) xal[s][lane] = al[s];
          __syncthreads();
#pragma unroll
          for (int s = 0; s < NS; ++s)
            if ((s & 1) != role) al[s] = xal[s][lane];
          __syncthreads();   // as for z: reads done before the next write of these slots
        }
      }
    }
    GST_SUB_END(25)
    GST_STAMP(5)
    // ---- nu (gibbs.py:244-259, 331-335)
    if ((mask & 64u) && md.vary_df) {
      double sa = 0.0;
#pragma unroll
      for (int s = 0; s < NS; ++s)
        if (vmask & (1u << s)) sa += log(al[s]) + 1.0 / al[s];
      const double S = wave_sum(sa);
      double ll = -INFINITY;
      if (lane < 30) {
        const double h = (double)(lane + 1) / 2.0;
        ll = -h * S + md.dfA[lane] - md.dfB[lane];
      }
      const double mx = wave_max(ll);
      if (lane < 30) dfbuf[lane] = exp(ll - mx);
      lds_order();
      double u;
      if (TAPE) {
        u = tp[TP_DELTA + m + 1 + 2 * nst];
      } else {
        double unused;
        rng.uniform2(0u, TAG_DF, u, unused);
      }
      // numpy pairwise sum of 30 (8 accumulators), normalise, sequential cumsum, choice
      double acc8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc8[j] = dfbuf[j];
#pragma unroll
      for (int i = 8; i < 24; i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc8[j] += dfbuf[i + j];
      double tot = ((acc8[0] + acc8[1]) + (acc8[2] + acc8[3])) +
                   ((acc8[4] + acc8[5]) + (acc8[6] + acc8[7]));
#pragma unroll
      for (int i = 24; i < 30; ++i) tot += dfbuf[i];
      // p_i = e_i / tot on lane i (one division per lane, not 30 per lane), the cumsum in
      // numpy's sequential order over the published p's (each lane keeps its own prefix),
      // then lane i tests cdf_i / cdf_29 <= u and the ballot counts (searchsorted 'right')
      const double pl = lane < 30 ? dfbuf[lane] / tot : 0.0;
      if (lane < 30) dfbuf[32 + lane] = pl;
      lds_order();
      double cs = 0.0, mine = 0.0;
#pragma unroll
      for (int i = 0; i < 30; ++i) {
        cs += dfbuf[32 + i];
        mine = (i == lane) ? cs : mine;
      }
      int cnt = __popcll(__ballot(lane < 30 && mine / cs <= u));
      cnt = cnt < 29 ? cnt : 29;
      nu = (double)(cnt + 1);
      lds_order();
    }
  }

  GST_STAMP(6)
  if (role != 0) return;   // pair mode: wave 0 writes the chain's state
  GST_STAMP_FLUSH
  // ---------------- write back ----------------
  if (lane < P) xrow[lane] = pget(xv, lane);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int t = 64 * s + lane;
    if (vmask & (1u << s)) {
      zrow[t] = (double)((zb >> s) & 1u);
      arow[t] = al[s];
      prow[t] = po[s];
    }
  }
  lds_order();   // the Gram counters' LDS adds precede their read
  if (lane == 0) {
    st.theta[c] = theta;
    st.nu[c] = nu;
    if (st.status) st.status[c] = (st.status[c] | status) + nfloor * STATUS_FLOOR_COUNT;
    if (st.gram_cnt) {
      __hip_atomic_fetch_add(st.gram_cnt, (unsigned long long)gcnt[wv][0], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(st.gram_cnt + 1, (unsigned long long)gcnt[wv][1],
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace gst
