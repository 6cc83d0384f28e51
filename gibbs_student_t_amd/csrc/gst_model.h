// The model, state, record and tape structs that host and kernels share, with the constants
// and shape helpers they need.  No HIP in here: a plain C++ compiler can include this header
// (the packer gst_pack.h, the launch planner gst_plan.h and their CPU tests do).
#pragma once

#ifdef __HIPCC__
#define GST_HOST_DEVICE __host__ __device__
#else
#define GST_HOST_DEVICE
#endif

namespace gst {

constexpr int NWHITE = 20;
constexpr int NHYPER = 10;
constexpr int PMAX = 16;   // sampled parameters (large path; the persistent kernel takes <= 4,
                           // its general-white-noise (GEN) instances <= 8)
constexpr int NBMAX = 8;   // backends with their own white-noise / ECORR parameters
constexpr int NPROC_MAX = 3;   // power-law processes of the Fourier block (GST_NPROC_MAX)
GST_HOST_DEVICE constexpr int SL(int r, int s) { return r * (r + 1) / 2 + s; }

// LDS of one CU (gfx950), the most one workgroup's static + dynamic LDS can take
constexpr int LDS_LIMIT = 160 * 1024;

// Per-chain LDS (doubles), laid out so that two chains fit per SIMD (8 per CU, 20 KB each
// at J1713 sizes):
//   S0R   [64 * SL(MT-K0, 0)]  the Schur complement S0 during the hyper block, [slot][lane];
//                              outside it, scratch of the other stages (white MH variates,
//                              Gram weights + tile transposes, b-draw vectors, nu grid)
//   colq  [8 * MT]             the one published column of the elimination, [p][r]
//   mhh   [4 * NHYPER]         hyper-MH variates of the sweep
//   phbuf [8 * MT]             phi^-1 by internal column
//   colq2 [8 * (MT - KP_MIN)]  the second published column of the paired tail (rows >= KP)
// Slot column KP from which the elimination runs in column pairs (chol_pair): two columns
// per LDS hand-off.  The pair buffers hold rows r >= KP only, at row stride MT - KP (even,
// for 128-bit accesses); LDS is sized for the earliest start, KP_MIN, which keeps the extra
// LDS within two chains per SIMD (8 per CU).  kp_for: the one-chain-per-SIMD builds pair
// from KP_MIN; the 256-register two-chains-per-SIMD build only over its last slot columns
// (pairing earlier spills there, and its second wave already covers much of the hand-off
// latency).
constexpr int KP_MIN = 4;
// gram_and_tm's low-rank Gram takes sweeps with at most LR_MAX flagged TOAs (z = 1): past
// that the n-TOA MFMA Gram is cheaper, and the class Grams' share that cancels grows
constexpr int LR_MAX = 32;
constexpr double LR_ALPHA_MAX = 0x1p20;   // ... and alpha_t <= 2^20 on every flagged TOA
// the largest TOA-slot count whose two-chains-per-SIMD build the host picks (wider shapes
// run one chain per SIMD)
#ifndef GST_OCC2_NS_MAX
#define GST_OCC2_NS_MAX 8   // A/B builds override it (GST_EXTRA_CFLAGS=-DGST_OCC2_NS_MAX=16)
#endif
constexpr int OCC2_NS_MAX = GST_OCC2_NS_MAX;
GST_HOST_DEVICE constexpr int pair_pw(int MT) { return MT - KP_MIN; }
#ifndef GST_KP_OCC2
#define GST_KP_OCC2 6   // A/B builds override it (GST_EXTRA_CFLAGS=-DGST_KP_OCC2=...)
#endif
GST_HOST_DEVICE constexpr int kp_for(int OCC) { return OCC == 2 ? GST_KP_OCC2 : KP_MIN; }
// index of slot (r, s), s < K0, among the timing-model factor slots (column-major)
GST_HOST_DEVICE constexpr int tm_slot(int MT, int r, int s) {
  return s * MT - s * (s - 1) / 2 + (r - s);
}
GST_HOST_DEVICE constexpr int s0r_doubles(int MT, int K0) { return 64 * SL(MT - K0, 0); }
GST_HOST_DEVICE constexpr int lds_doubles(int MT, int K0) {
  return s0r_doubles(MT, K0) + 8 * MT + 4 * NHYPER + 8 * MT + 8 * pair_pw(MT);
}
// chains (waves) per SIMD the LDS allows with 4-chain workgroups: 2 when two workgroups
// (8 chains) fit a CU's LDS
GST_HOST_DEVICE constexpr int occ_for(int MT, int K0) {
  return lds_doubles(MT, K0) * 8 * 4 * 2 <= LDS_LIMIT ? 2 : 1;
}
// scratch aliases inside S0R (offsets in doubles), each live only while S0 is dead
GST_HOST_DEVICE constexpr int s0r_need(int MT, int NS) {
  return (4 * NWHITE > 64 * NS + 16 * 17 ? 4 * NWHITE : 64 * NS + 16 * 17) > 7 * 8 * MT + 64
             ? (4 * NWHITE > 64 * NS + 16 * 17 ? 4 * NWHITE : 64 * NS + 16 * 17)
             : 7 * 8 * MT + 64;
}
struct DevModel {
  const double* Tmf;     // [nks][NT][64]: MFMA-packed augmented T, internal column order
  const double* Tcol;    // [m][npad]: T column-major, reference column order, zero padded
  const double* resid;   // [npad]
  const double* sig2;    // [npad]  toaerrs**2
  const double* lfreq;   // [nf]    log(Ffreqs)
  const double* ldf;     // [nf]    log(repeat(df, 2))
  const double* dfA;     // [32]    n*(nu/2)*log(nu/2)
  const double* dfB;     // [32]    n*gammaln(nu/2)
  const int* ref2int;    // [m]     reference column -> internal index
  const int* cidx;       // [npad]  noise class of each TOA (TOAs with equal sigma), or null
  const double* csig2;   // [ncls]  sigma^2 of each class
  const double* ccount;  // [ncls]  TOAs per class
  int ncls;              // 0 = per-TOA white likelihood; 1..8 = class path
  // persistent kernel, ncls > 0 (else null): per-class Grams of [T|r] in the 8x8-cyclic
  // register layout [ncls][SL(MT,0)][64] and the augmented rows [npad][8 MT] (internal
  // order), for the low-rank Gram (gram_and_tm)
  const double* Gcls;
  const double* Trow;
  int n, m, mp, nf, ntm, ntm_pad, raug, nks, npad, nslot_toa;
  int P;
  int idx_efac, idx_equad, idx_logA, idx_gamma;
  double efac_const;
  double pmin[PMAX], pmax[PMAX], lp_in[PMAX], lp_sum;
  int hind[PMAX], nh, wind[PMAX], nw;
  // general white noise (large path; the persistent kernel's GEN instances):
  // per-backend efac / log10_equad / log10_ecorr parameter indices (-1: constant / none),
  // the backend of every TOA, and the ECORR epoch columns (internal columns
  // ntm_pad + nf .. ntm_pad + nf + nec - 1, between the Fourier block and the residual row)
  int nb;
  int cls_b[8];             // backend of each noise class (classes: equal sigma AND backend)
  const int* bk;            // [npad] backend of each TOA (null when nb == 1)
  int efac_b[NBMAX], equad_b[NBMAX], ecorr_b[NBMAX];
  int nec;
  int ec_disjoint;          // every TOA in at most one ECORR column (the batch's datasets all)
  const int* ecb;           // [nec] backend of each ECORR column
  double ec_count[NBMAX];   // ECORR columns per backend
  // large path, disjoint ECORR epochs (gst_large.hpp lg_gram_ec; gx_nt = 0: not built): the
  // Gram's X part (timing model + Fourier + r + a ones column, gx_nt 16-column tiles) packed
  // as Tmf, and the epochs' TOAs in epoch order, 16 epochs per block, each block padded to
  // whole k-steps of 4: their X rows times the ECORR basis value ([nkse][gx_nt][64]), TOA
  // index and block-local epoch of each entry ([nkse * 4][2], -1 padding), block k-step starts
  const double* Tx;
  const double* Xe;
  const int* ekl;
  const int* eblk;          // [neblk + 1]
  int gx_nt, nkse, neblk;
  double sig_h, sig_w;
  double mh_cdf[5], mh_size[5];
  int model, vary_df, vary_alpha;
  double mk, k1mm, pspin;
  double tm_phiinv, logdet_phi_tm;
  double sum_lfreq, sum_ldf;  // sum_k log f_k, sum_k log df_k (closed-form log|phi|)
  double log_fyr, log_12pi2;
  unsigned long long* stamps;  // diagnostic build only (GST_STAMPS): [C][GST_NSTAMP]
  // power-law processes of the Fourier block (gst.h gst_model_procs: red | dm | chrom), behind
  // every earlier field so that none moves.  Process p owns the Fourier columns
  // [pcol[p], pcol[p + 1]), pcol[nproc] = nf, with its log10_A / gamma parameter indices and
  // the sums of log f_k and log df_k over its own columns (lfreq / ldf hold each process's
  // ladder; sum_lfreq / sum_ldf above stay the sums over the whole block, which one process
  // reads).  Entries p >= nproc repeat process 0's indices with no columns and zero sums.
  int nproc;
  int pcol[NPROC_MAX + 1];
  int pidxA[NPROC_MAX], pidxG[NPROC_MAX];
  double psum_lfreq[NPROC_MAX], psum_ldf[NPROC_MAX];
};

// gst_accum (posterior sums, gst_set_accum): the context's device copy, which the accumulating
// kernels (the sweep kernel's ACC instances, lg_accum) read with scalar loads.  It lies behind
// the two Gram counters of DevState::gram_cnt (accum_desc below) and not in DevState, whose
// layout -- the kernels' argument layout -- stays as it is: the sweep kernel sits at the
// register limit, and one more pointer in DevState alone moved the allocation of 81 instances.
struct DevAccum {
  double *z_sum, *pout_sum, *alpha_sum, *b_sum, *b_sq;
  long long* count;
  long long from_sweep;
  // gst_accum_toa (gst_set_accum_toa), all null / 0 when unset: exceedance counts of pout at
  // nthr thresholds ([nthr] planes of gt_plane = C * nst doubles, C the launch's chains, which
  // the host fills in per launch) and the sums of y = r - T b and y^2
  double *pout_gt, *resid_sum, *resid_sq;
  double thr[4];
  long long gt_plane;
  int nthr;
  // gst_accum_block (gst_set_accum_block), null / 0 when unset: the packed lower triangle of
  // b b^T over the columns [bb_col0, bb_col0 + bb_ncol) of b, bb_ncol (bb_ncol + 1) / 2 doubles
  // per chain
  int bb_col0, bb_ncol;
  double* bb;
};
struct DevState {
  double *x, *b, *z, *alpha, *pout, *theta, *nu;
  int* status;
  const int* dataset;  // [C] dataset of each chain (null: every chain uses dataset 0)
  int nst;             // row stride of the per-TOA arrays (max n over the datasets)
  int nd;              // number of datasets
  double* tmfac;       // [C][timing-model factor slots][64] scratch (persistent path)
  unsigned long long* prog;  // chain-sweeps started in this launch (two chains per SIMD), or
                             // null: see fair_prio
  int debug;                 // GST_DEBUG_* flags (gst_set_debug)
  unsigned long long* gram_cnt;  // [2] Grams computed: low-rank, MFMA (gst_gram_counts), or null;
                                 // then the DevAccum of an accumulating launch
};
GST_HOST_DEVICE inline DevAccum* accum_desc(unsigned long long* gram_cnt) {
  return reinterpret_cast<DevAccum*>(gram_cnt + 2);
}
struct DevRec {
  double *x, *b, *z, *alpha, *pout, *theta, *nu;
  int nrec;
};
struct DevTape {
  const double* data;
  int stride;
};

// GST_DEBUG_* flags the kernels and the launch planner read (DevState::debug)
constexpr int DEBUG_LARGE_GRAM = 2;    // large path: dense super-tile Gram (lg_gram) forced
constexpr int DEBUG_EXACT_BDRAW = 8;
constexpr int DEBUG_MFMA_GRAM = 16;   // persistent kernel: no low-rank Gram (tests, A/B)
constexpr int DEBUG_EPOCHS_LDS = 32;  // large path: ECORR-epochs-first chains on lg_hyper<2>

// tape layout offsets (see gst.h)
constexpr int TP_WHITE = 0, TP_HYPER = 80, TP_DELTA = 120;

}  // namespace gst
