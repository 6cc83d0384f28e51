// Stand-alone driver of the host packer (csrc/gst_pack.h) for tests/test_pack.py:
//   pack_dump <descriptor file> <output file>
// The descriptor file is 16 int32 (n, m, nfourier, ntm, n_ecorr, nbackend, nparams, n_hyper,
// n_white, ntm_pad, raug, MT, batch_disjoint, idx_log10_A, idx_gamma, nproc), then doubles
// T[n m], residuals[n], toaerrs[n], ffreqs[nfourier], pmin[P], pmax[P], df_A[30], df_B[30],
// then int32 backend[n], ecorr_backend[n_ecorr], ecorr_idx[nb], efac_idx[nb], equad_idx[nb],
// hyper_idx[n_hyper], white_idx[n_white], and for nproc > 0 the gst_model_procs arrays
// ncol[3], idx_log10_A[3], idx_gamma[3] (nproc = 0: the legacy packing without procs).  The
// output is, per buffer, a text line
// "name f8|i4 count" followed by the raw values.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gst_pack.h"

template <class T>
static std::vector<T> get(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
    std::fprintf(stderr, "pack_dump: short descriptor file\n");
    std::exit(2);
  }
  return v;
}
static void put(FILE* f, const char* name, const std::vector<double>& v) {
  std::fprintf(f, "%s f8 %zu\n", name, v.size());
  if (!v.empty()) std::fwrite(v.data(), 8, v.size(), f);
}
static void put(FILE* f, const char* name, const std::vector<int>& v) {
  std::fprintf(f, "%s i4 %zu\n", name, v.size());
  if (!v.empty()) std::fwrite(v.data(), 4, v.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int> h = get<int>(f, 16);
  gst_model_desc d{};
  d.n = h[0], d.m = h[1], d.nfourier = h[2], d.ntm = h[3], d.n_ecorr = h[4], d.nbackend = h[5];
  d.nparams = h[6], d.n_hyper = h[7], d.n_white = h[8];
  d.idx_log10_A = h[13], d.idx_gamma = h[14];
  const auto T = get<double>(f, (size_t)d.n * d.m), r = get<double>(f, d.n);
  const auto err = get<double>(f, d.n), ff = get<double>(f, d.nfourier);
  const auto pmin = get<double>(f, d.nparams), pmax = get<double>(f, d.nparams);
  const auto dfA = get<double>(f, 30), dfB = get<double>(f, 30);
  const auto bk = get<int>(f, d.n), ecb = get<int>(f, d.n_ecorr), eci = get<int>(f, d.nbackend);
  const auto efi = get<int>(f, d.nbackend), eqi = get<int>(f, d.nbackend);
  const auto hi = get<int>(f, d.n_hyper), wi = get<int>(f, d.n_white);
  gst_model_procs pr{};
  pr.nproc = h[15];
  if (pr.nproc > 0) {
    const auto pv = get<int>(f, 9);
    for (int q = 0; q < 3; ++q)
      pr.ncol[q] = pv[q], pr.idx_log10_A[q] = pv[3 + q], pr.idx_gamma[q] = pv[6 + q];
  }
  std::fclose(f);
  d.T = T.data(), d.residuals = r.data(), d.toaerrs = err.data(), d.ffreqs = ff.data();
  d.pmin = pmin.data(), d.pmax = pmax.data(), d.df_A = dfA.data(), d.df_B = dfB.data();
  d.backend = bk.data(), d.ecorr_backend = ecb.data(), d.ecorr_idx = eci.data();
  d.efac_idx = efi.data(), d.equad_idx = eqi.data(), d.hyper_idx = hi.data();
  d.white_idx = wi.data();
  d.idx_efac = efi[0], d.idx_equad = eqi[0];
  d.tm_weight = 1e40, d.efac_const = 1.0, d.mprior = 0.01, d.theta_prior_beta = 1;

  const gst::PackedModel p =
      gst::pack_dataset(&d, h[9], h[10], h[11], h[12] != 0, pr.nproc > 0 ? &pr : nullptr);
  const gst::DevModel& md = p.md;
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  put(o, "Tmf", p.Tmf), put(o, "Tcol", p.Tcol), put(o, "resid", p.resid), put(o, "sig2", p.sig2);
  put(o, "ref2int", p.ref2int), put(o, "cidx", p.cidx), put(o, "csig2", p.csig2);
  put(o, "ccount", p.ccount), put(o, "Trow", p.Trow), put(o, "Gcls", p.Gcls), put(o, "Tx", p.Tx);
  put(o, "Xe", p.Xe), put(o, "ekl", p.ekl), put(o, "eblk", p.eblk), put(o, "bk", p.bk);
  put(o, "ecb", p.ecb);
  put(o, "cls_b", std::vector<int>(md.cls_b, md.cls_b + 8));
  put(o, "ec_count", std::vector<double>(md.ec_count, md.ec_count + gst::NBMAX));
  put(o, "lp_sum", std::vector<double>{md.lp_sum});
  put(o, "ints", std::vector<int>{md.nks, md.npad, md.mp, md.gx_nt, md.nkse, md.neblk, md.ncls,
                                  md.ec_disjoint, md.n, md.m, md.nf, md.ntm, md.ntm_pad, md.raug,
                                  md.nslot_toa, md.nec, md.nb});
  // the spectrum pieces, process by process
  put(o, "lfreq", p.lfreq), put(o, "ldf", p.ldf);
  put(o, "sums", std::vector<double>{md.sum_lfreq, md.sum_ldf});
  put(o, "psum_lfreq", std::vector<double>(md.psum_lfreq, md.psum_lfreq + gst::NPROC_MAX));
  put(o, "psum_ldf", std::vector<double>(md.psum_ldf, md.psum_ldf + gst::NPROC_MAX));
  put(o, "nproc", std::vector<int>{md.nproc});
  put(o, "pcol", std::vector<int>(md.pcol, md.pcol + gst::NPROC_MAX + 1));
  put(o, "pidxA", std::vector<int>(md.pidxA, md.pidxA + gst::NPROC_MAX));
  put(o, "pidxG", std::vector<int>(md.pidxG, md.pidxG + gst::NPROC_MAX));
  put(o, "idx_red", std::vector<int>{md.idx_logA, md.idx_gamma});
  return std::fclose(o) ? 1 : 0;
}
