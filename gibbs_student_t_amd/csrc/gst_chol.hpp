// The persistent kernel's elimination: the right-looking LDL^T-scaled Cholesky on the 8x8-cyclic
// register layout (one-column steps, the paired tail, the lean variant), the harvest of pivots
// and augmented-row entries, their statistics, and the SVD noise floor of the b draw.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "gst_model.h"
#include "gst_wave.hpp"

namespace gst {

// The published column: colq[p][r] = row 8r+p of the column being eliminated, r fastest, so
// a lane's row-side (p) and column-side (q) reads are contiguous in r and go as 128-bit LDS
// loads; the 8 owner lanes (q == column residue) write it.  Row stride MT = 10 doubles puts
// the 8 p-rows of a 128-bit read in distinct bank groups (80 B apart).

// ---- SVD noise floor of the b draw (include/gst.h gst_sweep; oracle Oracle.floor_shift) ----
// The reference draws b through sl.svd(Sigma) (gibbs.py:169-171).  When Sigma's smallest
// eigenvalues lie below ~eps ||Sigma|| (vvh17's all-outlier start, alpha = 1e10: cond ~ 1e22,
// while Sigma diagonally scaled is well conditioned) LAPACK returns them at its own rounding
// floor, ~0.3-2 x 2^-52 s_max, so its draw is in effect one from Sigma + f I -- which is what
// lets the reference's chains leave that state within ~100 sweeps (the exact draw stays there
// for thousands).  The b draw reproduces it: when the smallest pivot of
// the factor over the real columns is below FLOOR_GATE = 2^-52 x the largest (the pivot ratio
// below which LAPACK's SVD resolves those eigenvalues no longer: above it the reference's SVD
// mean agrees with the exact mean to ~1e-6), b is drawn exactly from
// Sigma + f I with f = FLOOR_C 2^-52 x the largest pivot; every other draw is the exact one.
// Each floor draw sets status bit 4 and adds 1 to the floor-draw count in bits 8..30.
constexpr double FLOOR_GATE = 0x1p-52;
#ifndef GST_FLOOR_C
#define GST_FLOOR_C 0.75  // oracle/gibbs_oracle.py FLOOR_C (tools/vvh17_escape.py calibrates it)
#endif
constexpr double FLOOR_C = GST_FLOOR_C;
constexpr int STATUS_FLOOR = 16;
constexpr int STATUS_FLOOR_COUNT = 256;   // one floor draw, counted in bits 8..30

// Smallest / largest pivot over the real columns of a factor whose pivot of internal column
// j = 64 sl + lane is apr[sl]; real columns are [0, ntm) and [f0, f1) (the rest are unit-prior
// pads).  Wave-uniform.
__device__ __forceinline__ void pivot_range(const double (&apr)[2], int lane, int ntm, int f0,
                                            int f1, double& mn, double& mx) {
  mx = 0.0;
  mn = INFINITY;
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
    const int j = 64 * sl + lane;
    const bool real = j < ntm || (j >= f0 && j < f1);
    mx = real ? fmax(mx, apr[sl]) : mx;
    mn = real ? fmin(mn, apr[sl]) : mn;
  }
  mx = wave_max(mx);
  mn = -wave_max(-mn);
}
__device__ __forceinline__ double floor_of(double mn, double mx) {
  return mn < FLOOR_GATE * mx ? FLOOR_C * 0x1p-52 * mx : 0.0;
}
__device__ __forceinline__ double floor_shift(const double (&apr)[2], int lane, int ntm, int f0,
                                              int f1) {
  double mn, mx;
  pivot_range(apr, lane, ntm, f0, f1, mn, mx);
  return floor_of(mn, mx);
}

// Right-looking LDL^T-scaled Cholesky on the cyclic register layout.
//
// Registers keep RAW columns: after column k is eliminated, slot values hold
// a_ik = L_ik * sqrt(a_kk) (the a_kk are the pivots), so L_ik = a_ik / sqrt(a_kk) is never
// formed inside the factorisation; the rank-1 update is a_ij -= (a_ik / a_kk) * a_jk.
// After each step every lane publishes its slot column that holds the next column into
// its own LDS column buffer colq[q][.] (no owner test, no selects); step k reads the
// buffer of q = k % 8.  Rows <= k are masked on the reading side (only slot K can hold
// them).  The slot column holding column k+1 is updated first so its publication (the
// step-to-step dependency through LDS) is issued before the rest of the trailing update.
// Outputs per column: the pivot a_kk and the augmented-row entry a_{raug,k}.  Nothing is
// captured per step (the step is VALU-issue-bound): an eliminated column is frozen in the
// registers (the column-side mask zeroes every later update to it), so chol_harvest reads
// both from L after the elimination; chol_stats then gives sum log a_kk (= log|Sigma| over
// these columns, as mantissa product + exponent sum), sum a_{raug,k}^2 / a_kk (= the
// d^T Sigma^-1 d contribution) and the failure flag.  The hyper MH's likelihoods take the same
// statistics straight from the diagonal lanes (chol_stats_diag) and harvest once per sweep,
// in front of the b draw.
struct CholCtx {
  double* colq;   // [8][MT] the published column (paired tail: the even column, [8][PW])
  double* junk;   // [8][MT] where the other lanes' publishing stores land (see chol_publish)
  double* colq2;  // [8][MT - KP] paired tail: the odd column (rows >= KP)
  int lane, p, q, raug;
  double mant, quad;
  int expo, fail;
  // pivots a_kk and augmented-row entries a_{raug,k}: column k kept by lane k % 64 in
  // slot k / 64 (filled by chol_harvest)
  double apr[2], zr[2];
};

// Publish column 8s + QQ: its owner lanes (q == QQ) write their slot column s, rows >= s.
// Every lane stores ("pad, don't mask"): the others' stores go to the junk rows, so the
// elimination stays free of lane-divergent control flow, which at this register pressure
// makes the allocator spill kilobytes per lane.
// The published column carries zeros in its rows <= its own index (slot row s, p <= QQ: the
// frozen rows and the pivot row), so the readers' row- and column-side multipliers come out
// masked without a select of their own (one select here instead of two per reader side).
template <int MT, int QQ>
__device__ __forceinline__ void chol_publish(const double (&L)[SL(MT, 0)], CholCtx& cc, int s) {
  double* dst = (cc.q == QQ ? cc.colq : cc.junk) + MT * cc.p;
  const bool live = cc.p > QQ;
#pragma unroll
  for (int r2 = 0; r2 < MT; r2 += 2) {          // rows (r2, r2+1)
    if (r2 >= s) {  // one ds_write_b128 per row pair (16-byte aligned: MT, r2 even)
      typedef double v2_t __attribute__((ext_vector_type(2)));
      const double v0 = (r2 == s) ? (live ? L[SL(r2, s)] : 0.0) : L[SL(r2, s)];
      *(v2_t*)(dst + r2) = (v2_t){v0, L[SL(r2 + 1, s)]};
    } else if (r2 + 1 >= s)
      dst[r2 + 1] = live ? L[SL(r2 + 1, s)] : 0.0;
  }
}

// Raw column k as seen by this lane: rows 8r+p (lr), rows 8r+q (lc), the augmented row
// entry, the pivot and its reciprocal.
template <int MT>
struct ColView {
  double lr[MT], lc[MT];
  double akk;
  double y0, e;  // rcp estimate of 1/a_kk and its Newton residual 1 - a_kk y0
};

// 1/a_kk in two halves: the estimate and residual start the step's two dependent chains
// (the critical factor below and the trailing-update reciprocal y0 + y0 e).
template <int MT>
__device__ __forceinline__ void pivot_rcp(ColView<MT>& c) {
  c.y0 = __builtin_amdgcn_rcp(c.akk);
  c.e = fma(-c.akk, c.y0, 1.0);
}

// Rows >= K of a published column [8][STRIDE] whose first stored row is R0 (the one-column
// steps: colq, stride MT, R0 = 0; the paired tail: colq / colq2, stride MT - KP, R0 = KP).
template <int MT, int K, int STRIDE = MT, int R0 = 0>
__device__ __forceinline__ void chol_load(const double* buf, const CholCtx& cc, ColView<MT>& c) {
  static_assert(MT % 2 == 0 && STRIDE % 2 == 0 && R0 % 2 == 0 && K >= R0,
                "128-bit column loads need 16-byte alignment");
  const double* cr = buf + STRIDE * cc.p - R0;
  const double* cq = buf + STRIDE * cc.q - R0;
#pragma unroll
  for (int r2 = 0; r2 < MT; r2 += 2) {          // rows (r2, r2+1)
    if (r2 >= K) {  // 128-bit loads (16-byte aligned: MT, r2 even)
      typedef double v2_t __attribute__((ext_vector_type(2)));
      const v2_t a = *(const v2_t*)(cr + r2);
      const v2_t b = *(const v2_t*)(cq + r2);
      c.lr[r2] = a[0];
      c.lr[r2 + 1] = a[1];
      c.lc[r2] = b[0];
      c.lc[r2 + 1] = b[1];
    } else if (r2 + 1 >= K) {
      c.lr[r2 + 1] = cr[r2 + 1];
      c.lc[r2 + 1] = cq[r2 + 1];
    }
  }
}

// ---- Paired tail: two columns per LDS hand-off ------------------------------------------
// From slot column KP on, columns k and k+1 (k even, both in slot column KB) are
// published together, column k+1 still RAW with respect to column k.  Every lane applies
// column k's update to its own copy of column k+1 (one FMA per loaded row, the multiplier
// tk = a(k+1,k) / a_kk a wave-uniform scalar from the owner lanes' registers), so a hand-off
// serves two columns: the tail of the elimination is latency-bound on the ~140-cycle
// write -> read hand-off, and this halves the number of hand-offs.
// Every matrix element still receives the one-column steps' FMAs, with the same operands, in
// the same order (including which slot column takes the column-scaled form), and the
// corrected copy of column k+1 is the expression its owner lanes evaluate in the one-column
// step: the factor is bitwise that of chol_step alone.
template <int MT, int QQ, int KP>
__device__ __forceinline__ void chol_publish_pair(const double (&L)[SL(MT, 0)], CholCtx& cc,
                                                  int s) {
  constexpr int PW = MT - KP;
  const bool even = cc.q == QQ, odd = cc.q == QQ + 1;
  double* dst = (even ? cc.colq : (odd ? cc.colq2 : cc.junk)) + PW * cc.p - KP;
  const bool live = cc.p > (odd ? QQ + 1 : QQ);   // zero rows <= the column's own index
#pragma unroll
  for (int r2 = KP; r2 < MT; r2 += 2) {
    if (r2 >= s) {
      typedef double v2_t __attribute__((ext_vector_type(2)));
      const double v0 = (r2 == s) ? (live ? L[SL(r2, s)] : 0.0) : L[SL(r2, s)];
      *(v2_t*)(dst + r2) = (v2_t){v0, L[SL(r2 + 1, s)]};
    } else if (r2 + 1 >= s)
      dst[r2 + 1] = live ? L[SL(r2 + 1, s)] : 0.0;
  }
}

// Publish columns 8KB + QQ and 8KB + QQ + 1 (slot column KB already updated by every earlier
// column), load both, and turn the odd one into its value after the even column's update.
// Returns nothing; n0 / n1 are ready for chol_pair (pivots and reciprocals set).
template <int MT, int KB, int QQ, int KP>
__device__ __forceinline__ void pair_handoff(double (&L)[SL(MT, 0)], CholCtx& cc,
                                             ColView<MT>& n0, ColView<MT>& n1) {
  constexpr int PW = MT - KP;
  static_assert(QQ % 2 == 0 && KB >= KP && KP % 2 == 0 && KP >= KP_MIN,
                "pairs start at even columns of the paired tail");
  lds_order();                       // the previous pair's loads precede the overwrite
  chol_publish_pair<MT, QQ, KP>(L, cc, KB);
  const double a22 = rdlane(L[SL(KB, KB)], 9 * QQ);       // a(k, k)
  const double a32 = rdlane(L[SL(KB, KB)], 9 * QQ + 8);   // a(k+1, k)
  const double a33 = rdlane(L[SL(KB, KB)], 9 * QQ + 9);   // a(k+1, k+1), before column k
  lds_order();
  ColView<MT> raw;
  chol_load<MT, KB, PW, KP>(cc.colq, cc, n0);
  chol_load<MT, KB, PW, KP>(cc.colq2, cc, raw);
  n0.akk = a22;
  pivot_rcp<MT>(n0);
  // the one-column step's factor of column k+1's owner lanes (lc[K1] y0 refined)
  const double t = a32 * n0.y0;
  const double tk = fma(t, n0.e, t);
  n1.akk = fma(-a32, tk, a33);
  pivot_rcp<MT>(n1);
#pragma unroll
  for (int r = KB; r < MT; ++r) {
    n1.lr[r] = fma(-n0.lr[r], tk, raw.lr[r]);
    n1.lc[r] = fma(-n0.lc[r], tk, raw.lc[r]);
  }
  // rows <= k+1 of slot KB: frozen / pivot rows of column k+1, as its publication would carry
  n1.lr[KB] = (cc.p > QQ + 1) ? n1.lr[KB] : 0.0;
  n1.lc[KB] = (cc.q > QQ + 1) ? n1.lc[KB] : 0.0;
}

// Columns k = 8K + KK and k+1 (KK even); c0 / c1 as pair_handoff leaves them.
template <int MT, int K, int KK, int KEND, int KP>
__device__ __forceinline__ void chol_pair(double (&L)[SL(MT, 0)], CholCtx& cc, ColView<MT>& c0,
                                          ColView<MT>& c1) {
  static_assert(KK % 2 == 0, "pairs start at even columns");
  constexpr int k = 8 * K + KK;
  constexpr int KB = (KK == 6) ? K + 1 : K;   // slot column of columns k+2, k+3
  constexpr int QB = (KK + 2) & 7;
  constexpr bool NEXT = k + 2 < KEND;
  static_assert(k + 2 <= KEND, "the paired tail covers an even number of columns");
  // column k's column-scaled factor (its "critical" slot column is K, which holds k+1)
  const double t0 = c0.lc[K] * c0.y0;
  const double tk0 = fma(t0, c0.e, t0);
  const double sk0 = fma(c0.y0, c0.e, c0.y0);
  // column k+1's (its critical slot column is KB, which holds k+2)
  const double t1 = c1.lc[KB < MT ? KB : K] * c1.y0;
  const double tk1 = fma(t1, c1.e, t1);
  const double sk1 = fma(c1.y0, c1.e, c1.y0);
  ColView<MT> n0, n1;
  if constexpr (KB < MT) {
    // critical path: slot column KB (columns k+2, k+3) by column k, then by column k+1
#pragma unroll
    for (int r = KB; r < MT; ++r) {
      double v = L[SL(r, KB)];
      if constexpr (KB == K)
        v = fma(-c0.lr[r], tk0, v);
      else
        v = fma(-(c0.lr[r] * sk0), c0.lc[KB], v);
      L[SL(r, KB)] = fma(-c1.lr[r], tk1, v);
    }
    if constexpr (NEXT) pair_handoff<MT, KB, QB, KP>(L, cc, n0, n1);
  }
  // the rest of the two columns' trailing update (row-scaled, as the one-column steps)
  double lrs0[MT], lrs1[MT];
#pragma unroll
  for (int r = K; r < MT; ++r) {
    lrs0[r] = c0.lr[r] * sk0;
    lrs1[r] = c1.lr[r] * sk1;
  }
#pragma unroll
  for (int s = K; s < MT; ++s) {
    if (s == KB) continue;
#pragma unroll
    for (int r = s; r < MT; ++r) {
      if (s == K) {
        // KK == 6: slot column K is column k's critical one (it holds k+1); column k+1 (the
        // slot's last) leaves it alone
        L[SL(r, s)] = fma(-c0.lr[r], tk0, L[SL(r, s)]);
      } else {
        const double v = fma(-lrs0[r], c0.lc[s], L[SL(r, s)]);
        L[SL(r, s)] = fma(-lrs1[r], c1.lc[s], v);
      }
    }
  }
  if constexpr (NEXT) chol_pair<MT, KB, QB, KEND, KP>(L, cc, n0, n1);
}

// Step k = 8K + KK, software-pipelined: the slot column holding column k+1 is updated
// and published first, column k+1's loads and pivot reciprocal are issued, and only then
// does the rest of step k's trailing update run (covering their latency).
template <int MT, int K, int KK, int KEND, int KP>
__device__ __forceinline__ void chol_step(double (&L)[SL(MT, 0)], CholCtx& cc,
                                          ColView<MT>& cur) {
  constexpr int k = 8 * K + KK;
  constexpr int K1 = (KK == 7) ? K + 1 : K;  // slot column of column k+1
  constexpr int KK1 = (KK + 1) & 7;
  constexpr bool NEXT = k + 1 < KEND;
  // rows <= k of slot K arrive as zeros (chol_publish): frozen entries stay untouched
  // column k+1 starts the paired tail: publish it together with k+2 (pair_handoff)
  constexpr bool TOPAIR = NEXT && K1 >= KP;
  static_assert(!TOPAIR || KK1 == 0, "the paired tail starts at a slot column");
  ColView<MT> nxt, nxt2;
  if constexpr (K1 < MT) {
    // critical path: slot column K1 (holds column k+1).  Its factor a_{8K1+q,k} / a_kk is
    // one value per lane (lc y0 refined by the Newton term), so the published column
    // feeds this FMA directly: LDS load -> FMA and rcp -> mul -> FMA -> FMA are the two
    // step-to-step chains (the row-scaled lrs below stay off them).
    const double t0 = cur.lc[K1] * cur.y0;
    const double tk = fma(t0, cur.e, t0);
#pragma unroll
    for (int r = K1; r < MT; ++r) L[SL(r, K1)] = fma(-cur.lr[r], tk, L[SL(r, K1)]);
    if constexpr (TOPAIR) {
      pair_handoff<MT, K1, 0, KP>(L, cc, nxt, nxt2);
    } else if constexpr (NEXT) {
      lds_order();                   // column k's loads precede its overwrite
      chol_publish<MT, KK1>(L, cc, K1);
      nxt.akk = rdlane(L[SL(K1, K1)], 9 * KK1);
      lds_order();
      chol_load<MT, K1>(cc.colq, cc, nxt);
      pivot_rcp<MT>(nxt);
    }
  }
  // lrs = a_ik / a_kk for the rest of the trailing update (one multiply per row, then one
  // FMA per element)
  const double sk = fma(cur.y0, cur.e, cur.y0);
  double lrs[MT];
#pragma unroll
  for (int r = K; r < MT; ++r) lrs[r] = cur.lr[r] * sk;
  // off the critical path: the rest of the trailing update
#pragma unroll
  for (int s = K; s < MT; ++s) {
    if (s == K1 || (KK == 7 && s == K)) continue;  // slot column K is done when KK == 7
#pragma unroll
    for (int r = s; r < MT; ++r) L[SL(r, s)] = fma(-lrs[r], cur.lc[s], L[SL(r, s)]);
  }
  if constexpr (TOPAIR)
    chol_pair<MT, K1, 0, KEND, KP>(L, cc, nxt, nxt2);
  else if constexpr (NEXT)
    chol_step<MT, K1, KK1, KEND, KP>(L, cc, nxt);
}

// Eliminate columns [8*KLO, KEND) (compile-time: no branch between steps), updating the
// trailing slots.
template <int MT, int KLO, int KEND, int KP>
__device__ __forceinline__ void chol_range(double (&L)[SL(MT, 0)], CholCtx& cc) {
  static_assert(KEND > 8 * KLO && KEND <= 8 * MT, "bad elimination range");
  if constexpr (KLO >= KP) {
    ColView<MT> c0, c1;
    pair_handoff<MT, KLO, 0, KP>(L, cc, c0, c1);
    chol_pair<MT, KLO, 0, KEND, KP>(L, cc, c0, c1);
  } else {
    chol_publish<MT, 0>(L, cc, KLO);
    ColView<MT> c;
    c.akk = rdlane(L[SL(KLO, KLO)], 0);
    lds_order();
    chol_load<MT, KLO>(cc.colq, cc, c);
    pivot_rcp<MT>(c);
    chol_step<MT, KLO, 0, KEND, KP>(L, cc, c);
  }
  lds_order();
}

// The same elimination without the next column's prefetch (one ColView live instead of
// two): used for the timing-model columns, where every slot of L is still live and the
// register budget of two chains per SIMD has no room for the double buffer.
template <int MT, int K, int KK, int KEND>
__device__ __forceinline__ void chol_step_lean(double (&L)[SL(MT, 0)], CholCtx& cc) {
  constexpr int k = 8 * K + KK;
  constexpr int K1 = (KK == 7) ? K + 1 : K;
  constexpr int KK1 = (KK + 1) & 7;
  ColView<MT> cur;
  lds_order();                       // the previous step's loads precede this publication
  chol_publish<MT, KK>(L, cc, K);
  cur.akk = rdlane(L[SL(K, K)], 9 * KK);
  lds_order();
  chol_load<MT, K>(cc.colq, cc, cur);
  pivot_rcp<MT>(cur);
  // rows <= k of slot K arrive as zeros (chol_publish): frozen entries stay untouched
  const double sk = fma(cur.y0, cur.e, cur.y0);
#pragma unroll
  for (int s = K; s < MT; ++s) {
    if (KK == 7 && s == K) continue;   // slot column K is complete
#pragma unroll
    for (int r = s; r < MT; ++r) L[SL(r, s)] = fma(-(cur.lr[r] * sk), cur.lc[s], L[SL(r, s)]);
  }
  if constexpr (k + 1 < KEND) chol_step_lean<MT, K1, KK1, KEND>(L, cc);
}

template <int MT, int KLO, int KEND>
__device__ __forceinline__ void chol_range_lean(double (&L)[SL(MT, 0)], CholCtx& cc) {
  static_assert(KEND > 8 * KLO && KEND <= 8 * MT, "bad elimination range");
  chol_step_lean<MT, KLO, 0, KEND>(L, cc);
  lds_order();
}

// After an elimination over columns [KLO, KEND): the pivot of column j = 8K+q is frozen in
// lane (q,q) slot (K,K) and its augmented-row entry in lane (RA%8, q) slot (RA/8, K); lane
// j % 64 of apr / zr[j / 64] fetches both (one lane permute per slot column, no branch).
template <int MT, int KLO, int KEND, int RA>
__device__ __forceinline__ void chol_harvest(const double (&L)[SL(MT, 0)], CholCtx& cc) {
  constexpr int R = RA / 8, PA = RA % 8;
  static_assert(KEND <= RA && RA < 8 * MT, "augmented row below the eliminated columns");
#pragma unroll
  for (int K = KLO / 8; K <= (KEND - 1) / 8; ++K) {
    const double vd = bperm(L[SL(K, K)], 9 * cc.q);
    const double vz = bperm(L[SL(R, K)], 8 * PA + cc.q);
    const int j = 8 * K + cc.q;
    const bool in = (j >= KLO) && (j < KEND);
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
      const bool mine = in && (8 * sl + cc.p == K);
      cc.apr[sl] = mine ? vd : cc.apr[sl];
      cc.zr[sl] = mine ? vz : cc.zr[sl];
    }
  }
}

// Lane-parallel statistics of an elimination over columns [KLO, KEND) from the per-lane
// pivots / aug entries (lane k % 64 of apr[k / 64], zr[k / 64]): prod a_kk as mantissa
// product + exponent sum (log taken once by the caller), sum a_{raug,k}^2 / a_kk and the
// failure flag, all wave-uniform.  Branch-free on purpose: a lane-divergent region here,
// inside the register-critical hyper block, makes the allocator spill ~1.4 KB per lane.
template <int KLO, int KEND>
__device__ __forceinline__ void chol_stats(CholCtx& cc) {
  double mm = 1.0, qd = 0.0;
  int ee = 0, f = 0;
#pragma unroll
  for (int sl = 0; sl < 2; ++sl) {
    const int j = 64 * sl + cc.lane;
    const bool in = (j >= KLO) && (j < KEND);
    const double a = in ? cc.apr[sl] : 1.0, z = in ? cc.zr[sl] : 0.0;
    f |= !(a > 0.0) ? 1 : 0;
    int e;
    mm *= frexp(a, &e);
    ee += e;
    qd = fma(z * z, rcp_nr1(a), qd);
  }
  mm *= dpp<DPP_XOR1>(mm);
  mm *= dpp<DPP_XOR2>(mm);
  mm *= dpp<DPP_ROR4>(mm);
  mm *= dpp<DPP_ROR8>(mm);
  cc.mant = (rdlane(mm, 0) * rdlane(mm, 16)) * (rdlane(mm, 32) * rdlane(mm, 48));
  cc.expo = wave_sum_i(ee);
  cc.quad = wave_sum(qd);
  cc.fail = __ballot(f) != 0ull ? 1 : 0;
}

// The same three statistics of an elimination over columns [KLO, KEND = RA) read where the
// elimination leaves them, with no harvest in front (the hyper MH's likelihoods: an MH step
// needs only these wave-uniform numbers, the gathered pivots and entries only the b draw).
//  * The pivot of column 8K + q is frozen in slot (K, K) of the diagonal lane 9q: each diagonal
//    lane multiplies the mantissas and adds the exponents of its own residue class over the
//    slot columns, then chol_stats' product and sum over the lanes combine the eight classes.
//    An entry outside the range counts as mantissa 1, exponent 0 (only the last slot column can
//    hold one), and so does every other lane: selects, no exec-masked region.  A dummy pad
//    column (pivot 1) gives mantissa 1/2, exponent 1 as in chol_stats: exact.
//  * The failure flag is !(a > 0) of the in-range pivots on the diagonal lanes (NaN fails).
//  * The augmented row's own diagonal element, slot (RA / 8, RA / 8) of lane 9 (RA % 8), has
//    received -= a_{RA,k}^2 / a_kk at every step: s0rr (its value before the elimination) minus
//    what it holds now is sum a_{RA,k}^2 / a_kk.  No prior is added to that element.
// The sums differ from chol_stats' in their last bits (another order of the same terms; the
// quadratic form by one subtraction of two accumulated numbers: tests/test_hyper_diag_stats_cpu.py
// bounds both against a long-double elimination).
template <int MT, int KLO, int KEND, int RA>
__device__ __forceinline__ void chol_stats_diag(const double (&L)[SL(MT, 0)], CholCtx& cc,
                                                double s0rr) {
  static_assert(KEND == RA && RA < 8 * MT, "the corner follows the last eliminated column");
  static_assert(KLO % 8 == 0 && KLO < KEND, "the range starts at a slot column");
  constexpr int R = RA / 8, PA = RA % 8;
  const bool dg = cc.p == cc.q;
  double mm = 1.0;
  int ee = 0, f = 0;
#pragma unroll
  for (int K = KLO / 8; K <= (KEND - 1) / 8; ++K) {
    const double a = L[SL(K, K)];
    int e;
    double mk = frexp(a, &e);
    int fk = !(a > 0.0) ? 1 : 0;
    if (8 * K + 8 > KEND) {   // the partial last slot column
      const bool in = cc.q < KEND - 8 * K;
      mk = in ? mk : 1.0;
      e = in ? e : 0;
      fk = in ? fk : 0;
    }
    mm *= mk;
    ee += e;
    f |= fk;
  }
  mm = dg ? mm : 1.0;
  ee = dg ? ee : 0;
  f = dg ? f : 0;
  mm *= dpp<DPP_XOR1>(mm);
  mm *= dpp<DPP_XOR2>(mm);
  mm *= dpp<DPP_ROR4>(mm);
  mm *= dpp<DPP_ROR8>(mm);
  cc.mant = (rdlane(mm, 0) * rdlane(mm, 16)) * (rdlane(mm, 32) * rdlane(mm, 48));
  cc.expo = wave_sum_i(ee);
  cc.quad = s0rr - rdlane(L[SL(R, R)], 9 * PA);
  cc.fail = __ballot(f) != 0ull ? 1 : 0;
}

}  // namespace gst
