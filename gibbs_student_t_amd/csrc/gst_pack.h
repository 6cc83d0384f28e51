// Packing of one dataset's constants (a validated gst_model_desc) into the layouts the kernels
// read (gst_model.h DevModel).  No HIP in here: pack_dataset fills host vectors and the
// DevModel's scalars; gst.hip uploads the vectors and sets the pointers.  Tested on a CPU
// (tools/pack_dump.cpp, tests/test_pack.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "gst.h"
#include "gst_model.h"

namespace gst {

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// Each vector is the DevModel array of the same name; an empty one stays a null pointer.
struct PackedModel {
  DevModel md{};   // scalars and small arrays filled, every pointer null
  std::vector<double> Tmf, Tcol, resid, sig2, lfreq, ldf, dfA, dfB, csig2, ccount, Gcls, Trow, Tx, Xe;
  std::vector<int> ref2int, cidx, bk, ecb, ekl, eblk;
};

// ECORR epochs are disjoint when no TOA has a nonzero entry in two of the last n_ecorr
// columns of T (the epochs-first elimination and the structured Gram take the ECORR block of
// T^T N^-1 T as diagonal)
inline bool ecorr_disjoint(const gst_model_desc* d) {
  const int m = d->m, nec = d->n_ecorr;
  for (int t = 0; t < d->n; ++t) {
    int nz = 0;
    for (int j = m - nec; j < m; ++j) nz += d->T[(size_t)t * m + j] != 0.0;
    if (nz > 1) return false;
  }
  return true;
}

// The MFMA operand layout of Tmf and Tx: [k-step][tile X][lane l], lane l holding TOA
// 4 ks + l / 16, column 16 X + l % 16; k-steps padded with zeros to whole 64-TOA chunks (the
// large path's Gram stages 16).  val(t, column) gives the entries of the n real TOAs.
template <class F>
std::vector<double> mfma_tiles(int n, int npad, int NT, F val) {
  std::vector<double> out((size_t)(npad / 4) * NT * 64, 0.0);
  for (int ks = 0; ks < round_up(n, 4) / 4; ++ks)
    for (int X = 0; X < NT; ++X)
      for (int l = 0; l < 64; ++l) {
        const int t = 4 * ks + (l >> 4);
        if (t < n) out[((size_t)ks * NT + X) * 64 + l] = val(t, 16 * X + (l & 15));
      }
  return out;
}

// Entry i (internal column order [TM | pad | Fourier | ECORR | r | pad]) of TOA t's augmented
// row [T|r]; int2ref: internal column -> reference column, -1 for pads
struct AugRow {
  const gst_model_desc* d;
  std::vector<int> int2ref;
  int raug;
  double operator()(int t, int i) const {
    if (i == raug) return d->residuals[t];
    return i < (int)int2ref.size() && int2ref[i] >= 0 ? d->T[(size_t)t * d->m + int2ref[i]] : 0.0;
  }
};

// The Fourier block of a descriptor without gst_model_procs: the red noise alone
inline gst_model_procs one_process(const gst_model_desc* d) {
  gst_model_procs pr{};
  pr.nproc = 1;
  pr.ncol[0] = d->nfourier;
  pr.idx_log10_A[0] = d->idx_log10_A;
  pr.idx_gamma[0] = d->idx_gamma;
  return pr;
}

// Common arrays: column maps, T in both layouts, residuals, variances, spectrum pieces
inline AugRow pack_common(const gst_model_desc* d, const gst_model_procs& pr, PackedModel& p,
                          int ntm_pad, int raug) {
  const int n = d->n, m = d->m, nf = d->nfourier, ntm = d->ntm, nec = d->n_ecorr;
  const int mpad = round_up(raug + 1, 16), npad = 64 * ((n + 63) / 64);
  // internal column order: [TM | pad | Fourier | ECORR | r | pad]; reference order
  // [Fourier | TM | ECORR]
  AugRow row{d, std::vector<int>(mpad, -1), raug};
  p.ref2int.resize(m);
  for (int j = 0; j < nf; ++j) p.ref2int[j] = ntm_pad + j;
  for (int j = 0; j < ntm; ++j) p.ref2int[nf + j] = j;
  for (int j = 0; j < nec; ++j) p.ref2int[nf + ntm + j] = ntm_pad + nf + j;
  for (int j = 0; j < m; ++j) row.int2ref[p.ref2int[j]] = j;
  p.Tmf = mfma_tiles(n, npad, mpad / 16, row);
  p.Tcol.assign((size_t)m * npad, 0.0);
  p.resid.assign(npad, 0.0);
  p.sig2.assign(npad, 0.0);
  for (int t = 0; t < n; ++t) {
    for (int j = 0; j < m; ++j) p.Tcol[(size_t)j * npad + t] = d->T[(size_t)t * m + j];
    p.resid[t] = d->residuals[t];
    p.sig2[t] = d->toaerrs[t] * d->toaerrs[t];
  }
  // spectrum pieces: log f_k and log df_k (df from f[::2], enterprise powerlaw), process by
  // process: each has its own ladder, so df restarts at its first pair (f_1 - 0)
  p.lfreq.resize(nf);
  p.ldf.resize(nf);
  p.md.sum_lfreq = p.md.sum_ldf = 0.0;
  p.md.nproc = pr.nproc;
  for (int q = 0, k0 = 0; q < NPROC_MAX; ++q) {
    const int nc = q < pr.nproc ? pr.ncol[q] : 0;
    p.md.pcol[q] = k0;
    p.md.pcol[q + 1] = k0 + nc;
    p.md.pidxA[q] = q < pr.nproc ? pr.idx_log10_A[q] : pr.idx_log10_A[0];
    p.md.pidxG[q] = q < pr.nproc ? pr.idx_gamma[q] : pr.idx_gamma[0];
    p.md.psum_lfreq[q] = p.md.psum_ldf[q] = 0.0;
    const double* ff = d->ffreqs + k0;
    for (int k = 0; k < nc; ++k) {
      p.lfreq[k0 + k] = std::log(ff[k]);
      const int pair = k / 2;
      const double prev = pair == 0 ? 0.0 : ff[2 * (pair - 1)];
      p.ldf[k0 + k] = std::log(ff[2 * pair] - prev);
    }
    for (int k = k0; k < k0 + nc; ++k) {
      p.md.psum_lfreq[q] += p.lfreq[k];
      p.md.psum_ldf[q] += p.ldf[k];
    }
    k0 += nc;
  }
  for (int k = 0; k < nf; ++k) {
    p.md.sum_lfreq += p.lfreq[k];
    p.md.sum_ldf += p.ldf[k];
  }
  p.dfA.assign(32, 0.0);
  p.dfB.assign(32, 0.0);
  for (int k = 0; k < 30; ++k) {
    p.dfA[k] = d->df_A[k];
    p.dfB[k] = d->df_B[k];
  }
  p.md.n = n;
  p.md.m = m;
  p.md.mp = mpad;
  p.md.nf = nf;
  p.md.ntm = ntm;
  p.md.ntm_pad = ntm_pad;
  p.md.raug = raug;
  p.md.nks = round_up(n, 4) / 4;
  p.md.npad = npad;
  p.md.nslot_toa = npad / 64;
  return row;
}

// Noise classes: TOAs with bit-identical sigma share N0 in the white likelihood (and equal
// backend: N0 = efac_b^2 sigma^2 + 10^(2 equad_b) depends on both).  More than 8: ncls = 0,
// the per-TOA path, and no class arrays.
inline void pack_classes(const gst_model_desc* d, PackedModel& p) {
  const int n = d->n;
  std::vector<int> cback;
  p.cidx.assign(p.md.npad, -1);
  int t = 0;
  for (; t < n; ++t) {
    const double v = d->toaerrs[t] * d->toaerrs[t];
    const int bt = (d->nbackend > 1 && d->backend) ? d->backend[t] : 0;
    int u = 0;
    while (u < (int)p.csig2.size() && (p.csig2[u] != v || cback[u] != bt)) ++u;
    if (u == (int)p.csig2.size()) {
      if (p.csig2.size() >= 8) break;
      p.csig2.push_back(v);
      p.ccount.push_back(0.0);
      cback.push_back(bt);
    }
    p.cidx[t] = u;
    p.ccount[u] += 1.0;
  }
  if (t < n) {
    p.cidx.clear();
    p.csig2.clear();
    p.ccount.clear();
  }
  p.md.ncls = (int)p.csig2.size();
  for (int u = 0; u < 8; ++u) p.md.cls_b[u] = u < p.md.ncls ? cback[u] : 0;
}

// Persistent kernel, <= 8 noise classes: the Gram of the augmented basis per
// class, G_k = sum_{t in class k} [T|r]_t [T|r]_t^T (long double, rounded once), in the
// kernel's 8x8-cyclic register layout [k][slot][lane], and the augmented rows
// [T|r]_t in internal order, stored [t][i % 8][i / 8] (a lane's row entries 8 r + p,
// r = 0 .. MT-1, are contiguous: 128-bit loads).  With them a sweep's Gram T^T N^-1 [T|r] is
//   sum_k c_k G_k + sum_{t: z_t = 1} c_k(t) (1 / alpha_t - 1) [T|r]_t [T|r]_t^T,
// c_k = 1 / (efac_b^2 sigma_k^2 + 10^(2 equad_b)): N_t = alpha_t^z_t N0_k(t) (gibbs.py:154,
// 297-304), a rank-(outlier count) update instead of the n-TOA MFMA Gram (gst_kernel.hpp
// gram_and_tm; the kernel takes it while at most LR_MAX TOAs are flagged).
inline void pack_class_grams(const AugRow& row, PackedModel& p, int MT) {
  const int n = p.md.n, ncls = p.md.ncls;
  const int W = 8 * MT, NSL = MT * (MT + 1) / 2;
  p.Trow.assign((size_t)p.md.npad * W, 0.0);
  for (int t = 0; t < n; ++t)
    for (int i = 0; i < W; ++i) p.Trow[(size_t)t * W + (i & 7) * MT + (i >> 3)] = row(t, i);
  std::vector<long double> acc((size_t)ncls * W * W, 0.0L);
  for (int t = 0; t < n; ++t) {
    long double* a = acc.data() + (size_t)p.cidx[t] * W * W;
    const double* tr = p.Trow.data() + (size_t)t * W;
    auto at = [&](int i) { return tr[(i & 7) * MT + (i >> 3)]; };
    for (int i = 0; i < W; ++i) {
      const double ri = at(i);
      if (ri == 0.0) continue;
      for (int j = 0; j <= i; ++j) a[(size_t)i * W + j] += (long double)ri * at(j);
    }
  }
  p.Gcls.assign((size_t)ncls * NSL * 64, 0.0);
  for (int k = 0; k < ncls; ++k)
    for (int r = 0; r < MT; ++r)
      for (int sl = 0; sl <= r; ++sl)
        for (int l = 0; l < 64; ++l) {
          const int i = 8 * r + (l >> 3), j = 8 * sl + (l & 7);
          const long double v = i >= j ? acc[((size_t)k * W + i) * W + j]
                                       : acc[((size_t)k * W + j) * W + i];
          p.Gcls[((size_t)k * NSL + SL(r, sl)) * 64 + l] = (double)v;
        }
}

// Large path, disjoint ECORR epochs: the structured Gram's operands (gst_large.hpp
// lg_gram_ec), when [timing model | Fourier | r | 1] fits four 16-column tiles
inline void pack_ecorr_gram(const AugRow& row, PackedModel& p) {
  const gst_model_desc* d = row.d;
  const int n = d->n, m = d->m, nf = d->nfourier, ntm = d->ntm, nec = d->n_ecorr;
  const int Q = p.md.ntm_pad + nf;
  if (Q + 2 > 64) return;
  const int NX = (Q + 2 + 15) / 16;
  // compact [X | r | 1] row q of TOA t (the ones column stays zero here: lg_gram_ec's G_xx
  // does not use it)
  auto xval = [&](int t, int q) -> double {
    if (q < Q) return row.int2ref[q] >= 0 ? d->T[(size_t)t * m + row.int2ref[q]] : 0.0;
    return q == Q ? d->residuals[t] : 0.0;
  };
  p.Tx = mfma_tiles(n, p.md.npad, NX, xval);
  // the epochs' TOAs (ascending), 16 epochs per block, each block padded to whole k-steps
  std::vector<std::vector<int>> etoa(nec);
  for (int t = 0; t < n; ++t)
    for (int e = 0; e < nec; ++e)
      if (d->T[(size_t)t * m + nf + ntm + e] != 0.0) etoa[e].push_back(t);
  const int neblk = (nec + 15) / 16;
  std::vector<int> ent_t, ent_e;
  p.eblk.assign(neblk + 1, 0);
  for (int b = 0; b < neblk; ++b) {
    p.eblk[b] = (int)ent_t.size() / 4;
    for (int e = 16 * b; e < std::min(nec, 16 * b + 16); ++e)
      for (int t : etoa[e]) {
        ent_t.push_back(t);
        ent_e.push_back(e - 16 * b);
      }
    while (ent_t.size() % 4) {
      ent_t.push_back(-1);
      ent_e.push_back(-1);
    }
  }
  p.eblk[neblk] = (int)ent_t.size() / 4;
  const int nkse = std::max(16, round_up(p.eblk[neblk], 16));
  ent_t.resize((size_t)nkse * 4, -1);
  ent_e.resize((size_t)nkse * 4, -1);
  p.Xe.assign((size_t)nkse * NX * 64, 0.0);
  p.ekl.assign((size_t)nkse * 8, -1);
  for (int q = 0; q < 4 * nkse; ++q) {
    p.ekl[2 * q] = ent_t[q];
    p.ekl[2 * q + 1] = ent_e[q];
  }
  for (int b = 0; b < neblk; ++b)
    for (int q = 4 * p.eblk[b]; q < 4 * p.eblk[b + 1]; ++q) {
      const int t = ent_t[q];
      if (t < 0) continue;
      const double u = d->T[(size_t)t * m + nf + ntm + 16 * b + ent_e[q]];
      for (int c = 0; c < 16 * NX; ++c)
        p.Xe[((size_t)(q / 4) * NX + c / 16) * 64 + 16 * (q % 4) + c % 16] =
            c == Q + 1 ? u * u : u * xval(t, c);
    }
  p.md.gx_nt = NX;
  p.md.nkse = nkse;
  p.md.neblk = neblk;
}

// Parameters, priors, backends and the outlier model: the DevModel's scalars
inline void pack_params(const gst_model_desc* d, PackedModel& p) {
  DevModel& md = p.md;
  const int n = d->n, P = d->nparams, nec = d->n_ecorr;
  md.P = P;
  md.idx_efac = d->idx_efac;
  md.idx_equad = d->idx_equad;
  md.idx_logA = d->idx_log10_A;
  md.idx_gamma = d->idx_gamma;
  md.efac_const = d->efac_const;
  for (int j = 0; j < PMAX; ++j) {
    md.pmin[j] = j < P ? d->pmin[j] : 0.0;
    md.pmax[j] = j < P ? d->pmax[j] : 0.0;
    md.lp_in[j] = j < P ? -std::log(d->pmax[j] - d->pmin[j]) : 0.0;
    md.hind[j] = j < d->n_hyper ? d->hyper_idx[j] : d->hyper_idx[0];
    md.wind[j] = j < d->n_white ? d->white_idx[j] : d->white_idx[0];
  }
  // general white noise: per-backend parameter indices, per-TOA backend, ECORR columns
  const int nb = d->nbackend > 0 ? d->nbackend : 1;
  md.nb = nb;
  for (int b = 0; b < NBMAX; ++b) {
    md.efac_b[b] = b < nb ? (d->efac_idx ? d->efac_idx[b] : d->idx_efac) : -1;
    md.equad_b[b] = b < nb ? (d->equad_idx ? d->equad_idx[b] : d->idx_equad) : d->idx_equad;
    md.ecorr_b[b] = b < nb && d->ecorr_idx ? d->ecorr_idx[b] : -1;
    md.ec_count[b] = 0.0;
  }
  md.nec = nec;
  if (nb > 1) {
    p.bk.assign(md.npad, 0);
    for (int t = 0; t < n; ++t) p.bk[t] = d->backend ? d->backend[t] : 0;
  }
  p.ecb.resize(nec);
  for (int e = 0; e < nec; ++e) {
    p.ecb[e] = d->ecorr_backend ? d->ecorr_backend[e] : 0;
    md.ec_count[p.ecb[e]] += 1.0;
  }
  md.lp_sum = 0.0;  // Python sum() order (gibbs.py:339)
  for (int j = 0; j < P; ++j) md.lp_sum += md.lp_in[j];
  md.nh = d->n_hyper;
  md.nw = d->n_white;
  md.sig_h = 0.05 * d->n_hyper;
  md.sig_w = 0.05 * d->n_white;
  const double probs[5] = {0.1, 0.15, 0.5, 0.15, 0.1};
  const double sizes[5] = {0.1, 0.5, 1.0, 3.0, 10.0};
  double cs = 0.0, cdf[5];
  for (int i = 0; i < 5; ++i) {
    cs += probs[i];
    cdf[i] = cs;
  }
  for (int i = 0; i < 5; ++i) {
    md.mh_cdf[i] = cdf[i] / cdf[4];
    md.mh_size[i] = sizes[i];
  }
  md.model = d->model;
  md.vary_df = d->vary_df;
  md.vary_alpha = d->vary_alpha;
  if (d->theta_prior_beta) {
    md.mk = n * d->mprior;
    md.k1mm = n * (1.0 - d->mprior);
  } else {
    md.mk = 1.0;
    md.k1mm = 1.0;
  }
  md.pspin = d->pspin;
  md.tm_phiinv = 1.0 / d->tm_weight;
  md.logdet_phi_tm = d->ntm * std::log(d->tm_weight);
  md.log_fyr = std::log(1.0 / (365.25 * 86400.0));
  md.log_12pi2 = std::log(12.0) + 2.0 * std::log(M_PI);
}

// ntm_pad / raug: the internal positions of the first Fourier column and of the residual
// row; a persistent-kernel instance larger than the model leaves unit-prior dummy columns
// between the Fourier block and the residual row.  MT: the persistent
// kernel's matrix slots, 0 on the large path.  batch_disjoint: ecorr_disjoint of every
// dataset of the batch (one hyper class per batch structure).  procs: the batch's power-law
// processes (validated, gst.hip check_procs), or null for the red noise alone.
inline PackedModel pack_dataset(const gst_model_desc* d, int ntm_pad, int raug, int MT,
                                bool batch_disjoint, const gst_model_procs* procs = nullptr) {
  PackedModel p;
  const AugRow row = pack_common(d, procs ? *procs : one_process(d), p, ntm_pad, raug);
  pack_classes(d, p);
  if (MT > 0 && p.md.ncls > 0) pack_class_grams(row, p, MT);
  pack_params(d, p);
  if (MT == 0 && d->n_ecorr > 0 && ecorr_disjoint(d)) pack_ecorr_gram(row, p);
  p.md.ec_disjoint = batch_disjoint ? 1 : 0;
  return p;
}

}  // namespace gst
