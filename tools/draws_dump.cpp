// Stand-alone driver of the shared draw laws (csrc/gst_draws.h) for tests/test_draws_host.py:
//   draws_dump <input file> <output file>
// It includes nothing but gst_draws.h and philox.hpp: building it with a plain C++ compiler is
// the proof that the laws' header is free of HIP.
// The input file is doubles only:
//   header[10]: seed low word, seed high word, chains, sweeps, nw, nh, sig_w, sig_h, NH
//               (power-law cases), nf
//   wind[8], hind[8], mh_cdf[5], mh_size[5]
//   log_12pi2, log_fyr, fsh, lfreq[nf], ldf[nf],
//   per power-law case (log10_A, gamma, log10_ecorr)                  [NH][3]
// The output is, per result, a text line "name f8 count" followed by the raw doubles.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gst_draws.h"
#include "philox.hpp"

using gst::Rng;

static std::vector<double> get(FILE* f, size_t n) {
  std::vector<double> v(n);
  if (n && std::fread(v.data(), 8, n, f) != n) {
    std::fprintf(stderr, "draws_dump: short input file\n");
    std::exit(2);
  }
  return v;
}
static void put(FILE* f, const char* name, const std::vector<double>& v) {
  std::fprintf(f, "%s f8 %zu\n", name, v.size());
  if (!v.empty()) std::fwrite(v.data(), 8, v.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const auto h = get(f, 10);
  const int C = (int)h[2], S = (int)h[3], NH = (int)h[8], nf = (int)h[9];
  gst::DevModel md{};
  md.nw = (int)h[4], md.nh = (int)h[5], md.sig_w = h[6], md.sig_h = h[7];
  const auto wind = get(f, 8), hind = get(f, 8), cdf = get(f, 5), size = get(f, 5);
  for (int j = 0; j < 8; ++j) md.wind[j] = (int)wind[j], md.hind[j] = (int)hind[j];
  for (int j = 0; j < 5; ++j) md.mh_cdf[j] = cdf[j], md.mh_size[j] = size[j];
  const auto pl = get(f, 3), lfreq = get(f, nf), ldf = get(f, nf), plc = get(f, (size_t)NH * 3);
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;

  // the MH variates of every (chain, sweep, step): the three uniforms, the normal,
  // mh_variate's four entries, and its entries from a tape row made of those same variates
  std::vector<double> mu, mxi, mout, mtape;
  Rng rng;
  rng.k0 = (uint32_t)h[0], rng.k1 = (uint32_t)h[1];
  for (int c = 0; c < C; ++c)
    for (int s = 0; s < S; ++s)
      for (int gs = 0; gs < gst::NWHITE + gst::NHYPER; ++gs) {
        rng.chain = (uint32_t)c, rng.sweep = (uint32_t)s;
        const bool white = gs < gst::NWHITE;
        const uint32_t tag = white ? gst::TAG_WHITE : gst::TAG_HYPER;
        const int step = white ? gs : gs - gst::NWHITE;
        double ua, ub, uidx, unused, out4[4];
        rng.uniform2(0u, tag | (uint32_t)(3 * step), ua, ub);
        rng.uniform2(0u, tag | (uint32_t)(3 * step + 2), uidx, unused);
        mu.insert(mu.end(), {ua, ub, uidx});
        mxi.push_back(gst::normal_from(rng, 0u, tag | (uint32_t)(3 * step + 1)));
        gst::mh_variate(md, rng, nullptr, gs, out4);
        mout.insert(mout.end(), out4, out4 + 4);
        double row[gst::TP_DELTA] = {0.0}, t4[4];
        double* e = row + (white ? gst::TP_WHITE : gst::TP_HYPER) + 4 * step;
        e[0] = ua, e[1] = out4[0], e[2] = mxi.back(), e[3] = ub;
        gst::mh_variate(md, rng, row, gs, t4);
        mtape.insert(mtape.end(), t4, t4 + 4);
      }
  put(o, "mh_u", mu), put(o, "mh_xi", mxi), put(o, "mh_out", mout), put(o, "mh_tape", mtape);

  // the prior side: lc, phi^-1 of every Fourier column and of an ECORR column, log|phi|, lnL
  std::vector<double> lcv, phf, phe, ldp, mll;
  for (int k = 0; k < NH; ++k) {
    const double lA = plc[3 * k], g = plc[3 * k + 1], lec = plc[3 * k + 2];
    const double lc = gst::powerlaw_lc(lA, g, pl[0], pl[1]);
    lcv.push_back(lc);
    double slf = 0.0, sldf = 0.0;
    for (int j = 0; j < nf; ++j) {
      phf.push_back(gst::phi_inv_fourier(lc, g, lfreq[j], ldf[j], pl[2]));
      slf += lfreq[j], sldf += ldf[j];
    }
    phe.push_back(gst::phi_inv_ecorr(lec, pl[2]));
    const double ld = gst::logdet_phi_fourier(nf, lc, g, slf, sldf, 0.0) +
                      gst::logdet_phi_ecorr(3.0, lec);
    ldp.push_back(ld);
    mll.push_back(gst::marginal_ll(lA, g, lec, lc, ld));
  }
  put(o, "lc", lcv), put(o, "phi_inv", phf), put(o, "phi_inv_ecorr", phe);
  put(o, "logdet_phi", ldp), put(o, "marginal_ll", mll);
  std::fclose(o);
  return 0;
}
