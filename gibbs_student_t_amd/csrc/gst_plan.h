// Launch planning of both paths: the large path's kernel classes, the LDS layouts of its
// kernels with dynamic LDS, and the ordered list of launches of a call (plan_large); the
// persistent path's launch shape (plan_persistent).  No HIP in here: pure functions of the
// model's integers, tested on a CPU (tools/plan_dump.cpp, tests/test_plan.py).  The kernels
// are in gst_large.hpp / gst_kernel.hpp; gst.hip maps a kernel id to its function.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "gst.h"
#include "gst_model.h"

namespace gst {

constexpr int LBLK = 256;      // threads of the per-chain kernels (4 waves)
// threads per chain of the per-TOA passes (lg_white, lg_toa): 16 waves per chain for the
// 100k-TOA datasets; 4 for datasets of up to TBLK_SMALL_NPAD TOAs, where a pass is a few
// TOAs per thread and a 16-wave chain spent it in barriers and reductions with one chain per
// CU.  The block size sets the reduction order, so it is chosen PER DATASET (kernel classes
// below), never from the launch's other datasets or its chain count: a dataset's chains are
// the same launched alone, batched with any others, or split over launches and ranks.
constexpr int TBLK = 1024;
constexpr int TBLK_SMALL = 256;
constexpr int TBLK_SMALL_NPAD = 32768;
// lg_white only: one wave per chain up to 8k TOAs (its 21 likelihood passes are then a few
// loads and one wave reduction each, with no workgroup barrier)
constexpr int TBLK_WAVE = 64;
constexpr int TBLK_WAVE_NPAD = 8192;
// Kernel classes of a dataset (the host launches one kernel per class present in a batch;
// a chain whose dataset is of another class returns at once):
//   lg_white: 0 = one wave (npad <= TBLK_WAVE_NPAD), 1 = TBLK_SMALL, 2 = TBLK threads;
//   lg_toa:   0 = TBLK_SMALL, 1 = TBLK threads;
//   hyper:    8 / 16 = lg_hyper_reg<8 / 16> (hyper block of <= 62 / 126 columns), 0 = lg_hyper
//             (LDS-resident block, <= HYPER_LDS_MAX columns), 1 = lg_hyper<1> (larger blocks:
//             blocked elimination in global memory), 2 = lg_hyper<2> (larger blocks made of
//             ECORR epochs -- hundreds of them -- around a small timing-model + Fourier block:
//             the epochs eliminated first, see lg_hyper).
GST_HOST_DEVICE constexpr int white_class(int npad) {
  return npad <= TBLK_WAVE_NPAD ? 0 : (npad <= TBLK_SMALL_NPAD ? 1 : 2);
}
GST_HOST_DEVICE constexpr int toa_class(int npad) { return npad <= TBLK_SMALL_NPAD ? 0 : 1; }
// hyper class from the dataset's own hyper block nf + nec: lg_hyper_reg<MT> takes up to
// HR<MT>::RA = 8 MT - 2 columns (62 / 126)
constexpr int HYPER_LDS_MAX = 138;   // lg_hyper<0>'s LDS block (HyperLds<0> below fits LDS_LIMIT)
// lg_hyper<2>: the timing-model + Fourier + augmented-row block X it factors per likelihood
// (qx = ntm + nfourier + 1 rows) is at most EC_QX_MAX (its lower 16x16 tiles, at most
// EC_TPW per wave, accumulate in MFMA registers); the epochs' couplings stream through LDS
// EC_ECH epochs at a time
constexpr int EC_QX_MAX = 76;
constexpr int EC_TPW = 4;
constexpr int EC_ECH = 32;
static_assert(((EC_QX_MAX + 15) / 16) * ((EC_QX_MAX + 15) / 16 + 1) / 2 <= EC_TPW * (LBLK / 64),
              "lg_hyper<2> tiles per wave");
// (force_lds: GST_DEBUG_LARGE_HYPER, the generic kernels: class 0, or 1 past HYPER_LDS_MAX)
// Class 2 (epochs first) for every block past HYPER_LDS_MAX it can take, and for blocks past
// lg_hyper_reg<8>'s 62 columns whose ECORR epochs outnumber X's rows (measured: mb, 20
// Fourier + 60 epochs, 1.8-2.1x over lg_hyper_reg<16>; ecb, 20 + 24, 0.54-0.85x of
// lg_hyper_reg<8>)
// Class 2 needs disjoint epochs (each TOA in at most one ECORR column: the ECORR block of
// T^T N^-1 T is then diagonal, which its elimination assumes); gst_model_set checks the basis
// (DevModel::ec_disjoint) and other ECORR bases take class 1 / the register kernels.
GST_HOST_DEVICE constexpr int hyper_class(int hcols, int force_lds, int nec, int qx, int disjoint = 1) {
  return (nec > 0 && disjoint && qx <= EC_QX_MAX && !force_lds &&
          (hcols > HYPER_LDS_MAX || (hcols > 8 * 8 - 2 && nec >= qx)))
             ? 2
         : hcols > HYPER_LDS_MAX ? 1
                                 : (force_lds ? 0 : (hcols <= 8 * 8 - 2 ? 8 : (hcols <= 8 * 16 - 2 ? 16 : 0)));
}
GST_HOST_DEVICE inline int hyper_class_of(const DevModel& md, int force_lds) {
  return hyper_class(md.nf + md.nec, force_lds, md.nec, md.ntm + md.nf + 1, md.ec_disjoint);
}
// Epochs-first chains (class 2) whose timing model has <= 16 columns and whose Fourier block
// fits the register layout run lg_hyper_ecr<MT, RA> (one wave per chain, MT = 6 / 8: Fourier
// blocks of <= 30 / 46 columns) instead of lg_hyper<2>; 0: lg_hyper<2> (also under
// GST_DEBUG_EPOCHS_LDS or GST_DEBUG_LARGE_HYPER)
// (instance id: 1 = <6, 46>, 2 = <8, 62>: (MT, augmented row); an instance <6, 38> for
// Fourier blocks of <= 22 columns, cutting eight pad steps, spilled 148 B/lane and measured
// no faster on ebig / mb)
// (and at most EC_REG_MAX epochs: their pivots and augmented-row entries live in registers)
constexpr int EC_REG_MAX = 192;
GST_HOST_DEVICE constexpr int ec_reg_mt(int hclass, int ntm, int nf, int nec, int debug) {
  return (hclass != 2 || ntm > 16 || nec > EC_REG_MAX || (debug & DEBUG_EPOCHS_LDS)) ? 0
         : (16 + nf <= 46 ? 1 : (16 + nf <= 62 ? 2 : 0));
}
GST_HOST_DEVICE inline int ec_reg_mt_of(const DevModel& md, int force_lds, int debug) {
  return ec_reg_mt(hyper_class_of(md, force_lds), md.ntm, md.nf, md.nec, debug);
}
// Chains whose dataset has disjoint ECORR epochs and runs them epochs first (class 2) take the
// structured Gram lg_gram_ec (DevModel::gx_nt > 0), which computes only the blocks class 2 reads:
// G_xx (X = timing model, Fourier, r), the epochs' diagonal and their couplings to X.  The
// dense Grams (lg_gram, lg_gram_small) skip these chains.  GST_DEBUG_LARGE_GRAM: dense.
GST_HOST_DEVICE inline bool gram_ec_of(const DevModel& md, int force_lds, int debug) {
  return md.gx_nt > 0 && !(debug & DEBUG_LARGE_GRAM) && hyper_class_of(md, force_lds) == 2;
}
constexpr int GRAM_WAVES = 8;  // chains per gram workgroup
constexpr int GRAM_KC = 16;    // lg_gram: k-steps (of 4 TOAs) per staged chunk
constexpr int GRAM_LDS = 2 * GRAM_KC * 8 * 64 + 2 * GRAM_WAVES * 64;   // doubles
constexpr int GS_NTMAX = 6;    // lg_gram_small<NT>: Grams of at most GS_NTMAX 16-column tiles
constexpr int GS_WPB = 4;      // ... chains (waves) per workgroup
constexpr int GEC_CPB = GS_WPB / 2;   // chains per lg_gram_ec workgroup
constexpr int TB_CG = 4;       // lg_tb: 16-chain groups per wave (chains per wave: 64)
// chains (waves) per workgroup of lg_hyper_reg<MT> and lg_hyper_ecr<MT, RA>
GST_HOST_DEVICE constexpr int hr_wpb(int MT) { return MT <= 8 ? 4 : 2; }
GST_HOST_DEVICE constexpr int he_wpb(int MT) { return MT <= 6 ? 4 : 2; }
#ifndef GST_TM_PW
#define GST_TM_PW 16   // A/B builds override it (32: config-5 tmelim 1.75 -> 2.95 ms, ebig -20%)
#endif
constexpr int TM_PW = GST_TM_PW;   // panel width of the blocked eliminations (panel_ldl)
#ifndef GST_TM_TILES
#define GST_TM_TILES 4   // (8: measured no faster on config 5, round 6)
#endif
constexpr int TM_TILES = GST_TM_TILES;   // trailing-update tiles per wave per round (panel_ldl)

// ------------------------------------------------------------------------------------
// Dynamic-LDS layouts (offsets and total in doubles): gst_model_set_batch refuses a model
// whose layout does not fit and sizes the launches from it (the host has no other source).
// lg_btm carves its LDS from its layout; lg_hyper's carve is written out in the kernel, in
// this order (from the offsets its blocked mode ran 1.0-1.7% slower): keep the two together.
// ------------------------------------------------------------------------------------
// lg_tmelim: the 16-column panel of all mp rows, [mp][TM_PW + 1]
struct TmelimLds {
  int total;
  GST_HOST_DEVICE constexpr explicit TmelimLds(int mp) : total(mp * (TM_PW + 1)) {}
};
// lg_btm: acc, wk, vt [K0] each (K0 = ntm_pad), then Delta [raug] (tape mode)
struct BtmLds {
  int wk, vt, dl, total;
  GST_HOST_DEVICE constexpr BtmLds(int K0, int raug) : wk(K0), vt(2 * K0), dl(3 * K0), total(3 * K0 + raug) {}
};
// lg_hyper<MODE>.  MODE 0: S [ms][ms + 1], ms = nf + nec + 1.  MODE 1: the panel
// [mp][TM_PW + 1] and 1 / a_kk [TM_PW] instead (S is in global memory).  MODE 2: X [qx][qx + 1]
// and its epochs-eliminated base XB, qx = ntm + nf + 1.  Then phi^-1 [nf + nec] and the
// back-substitution accumulators vv and right-hand side wv [ms] (MODE 2: [mp]); MODE 2 only:
// the epoch pivots aE [nec], two chunks of couplings Ech [2][EC_ECH][qxp] with their 1 / a_e
// einv [2][EC_ECH], the tape's Delta dl [mp] and the b draw vfull [mp], internal order.
template <int MODE>
struct HyperLds {
  int hcols, ms, qx, qxp, SS, vlen, ainv, XB, ph, vv, wv, aE, Ech, einv, dl, vfull, total;
  GST_HOST_DEVICE constexpr HyperLds(int nf, int nec, int ntm, int mp)
      : hcols(nf + nec), ms(hcols + 1), qx(ntm + nf + 1), qxp((qx + 15) & ~15),
        SS(MODE == 1 ? mp : (MODE == 2 ? qx + 1 : ms + 1)), vlen(MODE == 2 ? mp : ms),
        ainv(mp * (TM_PW + 1)), XB(qx * SS),
        ph(MODE == 1 ? ainv + TM_PW : (MODE == 2 ? 2 * qx : ms) * SS), vv(ph + hcols),
        wv(vv + vlen), aE(wv + vlen), Ech(aE + nec), einv(Ech + 2 * EC_ECH * qxp),
        dl(einv + 2 * EC_ECH), vfull(dl + mp), total(MODE == 2 ? vfull + mp : aE) {}
};
// lg_hyper's static __shared__ arrays (eck, ecs, red3, ecvalid, red, mhv, bc, hst), doubles
constexpr int HYPER_STATIC_LDS = NBMAX + 3 + 12 + 1 + 4 + 4 * NHYPER + 4 + 3;
static_assert((HyperLds<0>(HYPER_LDS_MAX, 0, 0, 0).total + HYPER_STATIC_LDS) * 8 <= LDS_LIMIT,
              "lg_hyper<0> at HYPER_LDS_MAX columns fits the LDS");
// (what does not grow with the epochs: X, XB, phi^-1 of the Fourier block, the coupling chunks)
static_assert((HyperLds<2>(EC_QX_MAX - 1, 0, 0, 0).total + HYPER_STATIC_LDS) * 8 <= LDS_LIMIT,
              "lg_hyper<2> at EC_QX_MAX rows of X fits the LDS");

// ------------------------------------------------------------------------------------
// plan_large: the launches of one gst_sweep / gst_eval_lnlike call on the large path
// ------------------------------------------------------------------------------------
// Kernel ids, in launch order within their stage (gst.hip: id -> function)
enum LargeKernel : int {
  LK_TB, LK_RECORD,
  LK_WHITE_WAVE, LK_WHITE_SMALL, LK_WHITE,            // white_class 0, 1, 2
  LK_GRAM_EC1, LK_GRAM_EC2, LK_GRAM_EC3, LK_GRAM_EC4, // lg_gram_ec<gx_nt>
  LK_GRAM_SMALL1, LK_GRAM_SMALL2, LK_GRAM_SMALL3, LK_GRAM_SMALL4, LK_GRAM_SMALL5,
  LK_GRAM_SMALL6, LK_GRAM,                            // lg_gram_small<mp / 16>, lg_gram
  LK_TMELIM,
  LK_HYPER_REG8, LK_HYPER_REG16, LK_HYPER0, LK_HYPER1, LK_HYPER2, LK_HYPER_ECR6, LK_HYPER_ECR8,
  LK_BTM,
  LK_TOA_SMALL, LK_TOA,                               // toa_class 0, 1
  LK_ACCUM,                                           // lg_accum (launched after lg_record's place)
  LK_COUNT
};
// The hyper kernel of a dataset: the one place that maps its class to a kernel
inline int hyper_kernel_of(const DevModel& md, int force_lds, int debug) {
  switch (hyper_class_of(md, force_lds)) {
    case 8: return LK_HYPER_REG8;
    case 16: return LK_HYPER_REG16;
    case 0: return LK_HYPER0;
    case 1: return LK_HYPER1;
    default: break;
  }
  const int emt = ec_reg_mt_of(md, force_lds, debug);
  return emt == 1 ? LK_HYPER_ECR6 : (emt == 2 ? LK_HYPER_ECR8 : LK_HYPER2);
}

enum : int { EV_BEGIN = 1, EV_END = 2 };
struct Launch {
  int kernel;      // LargeKernel
  int kind;        // GST_K_*: the timing kind (gst_kernel_times)
  int gx, gy, block;
  size_t lds;      // dynamic LDS, bytes
  int kclass;      // LArgs::kclass for lg_white / lg_toa (the only kernels that read it), else -1
  int floor_pass;  // LArgs::floor_pass
  int ev;          // EV_BEGIN: a timing event before the launch, EV_END: one after it
  bool record;     // lg_record: launched only on sweeps it % record_every == 0
};
struct LargePlan {
  std::vector<Launch> prologue, sweep;   // once per call; once per sweep
  int ys = 0;            // row stride of the per-TOA scratch: the batch's largest npad
  int nsb = 0, npairs = 0;   // lg_gram: super-tile rows and lower super-tiles
  int hyper_lds = 0;     // LArgs::hyper_lds
  bool need_g3 = false;  // a dataset runs lg_hyper<1>: the scratch needs G3
  std::string error;     // not empty: the call is refused
};

// mds: the batch's datasets (their integers only); debug: GST_DEBUG_*; rec_on: records are
// written (record_every > 0, not eval_only).  eval_only: one pass up to the hyper launches.
// acc_on: posterior sums are set (gst_set_accum; never with eval_only or GST_STAGE_GRAM):
// lg_accum follows lg_record's place; the host skips it on sweeps before from_sweep.
inline LargePlan plan_large(const DevModel* mds, int nd, int debug, int C, unsigned mask,
                            bool eval_only, bool rec_on, bool acc_on = false) {
  LargePlan p;
  const DevModel& h = mds[0];
  const int force = (debug & GST_DEBUG_LARGE_HYPER) ? 1 : 0;
  p.hyper_lds = force;
  // kernels present among the batch's datasets: one launch per class, each chain runs in
  // its own dataset's class, so its arithmetic never depends on the other datasets
  bool on[LK_COUNT] = {};
  int gram_small = h.mp / 16;   // one tile count per batch, else the super-tile Gram
  int gram_ec_nt = 0;
  bool gram_dense = false, tm_needed = false;
  for (int i = 0; i < nd; ++i) {
    const DevModel& md = mds[i];
    p.ys = std::max(p.ys, md.npad);
    on[LK_WHITE_WAVE + white_class(md.npad)] = true;
    on[LK_TOA_SMALL + toa_class(md.npad)] = true;
    on[hyper_kernel_of(md, force, debug)] = true;
    if (md.mp != h.mp) gram_small = 0;
    // lg_tmelim and lg_btm return at once for class-2 chains (the epochs-first kernels factor
    // the timing model and draw all of b): a batch of class-2 datasets does not launch them
    tm_needed = tm_needed || hyper_class_of(md, force) != 2;
    // the structured Gram for the datasets it takes, the dense one for the rest
    if (gram_ec_of(md, force, debug)) gram_ec_nt = md.gx_nt;
    else gram_dense = true;
  }
  if (gram_small > GS_NTMAX || (debug & GST_DEBUG_LARGE_GRAM)) gram_small = 0;
  if (gram_ec_nt) on[LK_GRAM_EC1 + gram_ec_nt - 1] = true;
  if (gram_dense) on[gram_small ? LK_GRAM_SMALL1 + gram_small - 1 : LK_GRAM] = true;
  p.need_g3 = on[LK_HYPER1];
  p.nsb = (h.mp / 16 + 3) / 4;
  p.npairs = p.nsb * (p.nsb + 1) / 2;
  const size_t lds_tm = (size_t)TmelimLds(h.mp).total * 8;
  const size_t lds_btm = (size_t)BtmLds(h.ntm_pad, h.raug).total * 8;
  const size_t lds_h0 = (size_t)HyperLds<0>(h.nf, h.nec, h.ntm, h.mp).total * 8;
  const size_t lds_h1 = (size_t)HyperLds<1>(h.nf, h.nec, h.ntm, h.mp).total * 8;
  const size_t lds_h2 = (size_t)HyperLds<2>(h.nf, h.nec, h.ntm, h.mp).total * 8;
  // (a class-2 model forced to lg_hyper<1> by GST_DEBUG_LARGE_HYPER may have a block whose
  // panel does not fit the LDS: refuse it rather than fail at launch)
  if (on[LK_HYPER1] && lds_h1 > (size_t)LDS_LIMIT)
    p.error = "gst: GST_DEBUG_LARGE_HYPER: this model's red-noise / ECORR block is too "
              "large for the blocked elimination's LDS panel (lg_hyper<1>)";
  auto chains = [&](int wpb) { return (C + wpb - 1) / wpb; };
  auto add = [&](std::vector<Launch>& v, int k, int floor_pass = 0, int ev = EV_BEGIN | EV_END) {
    Launch l{k, GST_K_HYPER, C, 1, LBLK, 0, -1, floor_pass, ev, false};
    if (k == LK_TB) {
      l.kind = GST_K_TB, l.gx = p.ys / 64, l.gy = chains(64 * TB_CG);
    } else if (k == LK_RECORD) {
      l.kind = GST_K_RECORD, l.record = true;
    } else if (k == LK_ACCUM) {
      l.kind = GST_K_ACCUM;
    } else if (k <= LK_WHITE) {
      l.kind = GST_K_WHITE, l.kclass = k - LK_WHITE_WAVE;
      l.block = k == LK_WHITE_WAVE ? TBLK_WAVE : (k == LK_WHITE_SMALL ? TBLK_SMALL : TBLK);
    } else if (k <= LK_GRAM_EC4) {
      l.kind = GST_K_GRAM, l.gx = chains(GEC_CPB), l.block = 64 * GS_WPB;
    } else if (k <= LK_GRAM_SMALL6) {
      l.kind = GST_K_GRAM, l.gx = chains(GS_WPB), l.block = 64 * GS_WPB;
    } else if (k == LK_GRAM) {
      l.kind = GST_K_GRAM, l.gx = p.npairs * chains(GRAM_WAVES), l.block = 64 * GRAM_WAVES;
      l.lds = (size_t)GRAM_LDS * 8;
    } else if (k == LK_TMELIM) {
      l.kind = GST_K_TMELIM, l.lds = lds_tm;
    } else if (k == LK_HYPER_REG8 || k == LK_HYPER_REG16) {
      const int w = hr_wpb(k == LK_HYPER_REG8 ? 8 : 16);
      l.gx = chains(w), l.block = 64 * w;
    } else if (k == LK_HYPER_ECR6 || k == LK_HYPER_ECR8) {
      const int w = he_wpb(k == LK_HYPER_ECR6 ? 6 : 8);
      l.gx = chains(w), l.block = 64 * w;
    } else if (k <= LK_HYPER2) {
      l.lds = k == LK_HYPER0 ? lds_h0 : (k == LK_HYPER1 ? lds_h1 : lds_h2);
    } else if (k == LK_BTM) {
      l.kind = GST_K_BTM, l.lds = lds_btm;
    } else {
      l.kind = GST_K_TOA, l.kclass = k - LK_TOA_SMALL;
      l.block = k == LK_TOA_SMALL ? TBLK_SMALL : TBLK;
    }
    v.push_back(l);
  };
  auto add_range = [&](int k0, int k1, int floor_pass = 0) {
    for (int k = k0; k <= k1; ++k)
      if (on[k]) add(p.sweep, k, floor_pass);
  };
  // One sweep = record, accum, white, gram, tmelim, hyper, btm, tb, toa launches (gst_large.hpp)
  add(p.prologue, LK_TB);   // y = r - T b for the current b
  if (rec_on) add(p.sweep, LK_RECORD);
  if (acc_on) add(p.sweep, LK_ACCUM);
  add_range(LK_WHITE_WAVE, LK_WHITE);
  if ((mask & (6u | GST_STAGE_GRAM)) || eval_only) {
    // one event pair around the Gram launches (each kernel skips the other's chains)
    const size_t g0 = p.sweep.size();
    add_range(LK_GRAM_EC1, LK_GRAM);
    for (size_t i = g0; i < p.sweep.size(); ++i)
      p.sweep[i].ev = (i == g0 ? EV_BEGIN : 0) | (i + 1 == p.sweep.size() ? EV_END : 0);
    if (tm_needed) add(p.sweep, LK_TMELIM);
    if (!(mask & GST_STAGE_GRAM)) {   // (with it: timing diagnostic, Gram + TM elimination only)
      add_range(LK_HYPER_REG8, LK_HYPER_ECR8);
      if (eval_only) return p;
      if ((mask & 4u) && !(debug & GST_DEBUG_EXACT_BDRAW)) {
        // the b draw's floor pass (include/gst.h gst_sweep): chains whose Sigma is beyond
        // fp64 resolution re-eliminate G with Sigma + f I and draw there; every other chain
        // returns at once (SC_FLOOR == 0)
        if (tm_needed) add(p.sweep, LK_TMELIM, 1);
        add_range(LK_HYPER_REG8, LK_HYPER_ECR8, 1);
      }
      if (mask & 4u) {
        if (tm_needed) add(p.sweep, LK_BTM);
        add(p.sweep, LK_TB);
      }
    }
  }
  if (!eval_only && (mask & 0x78u)) add_range(LK_TOA_SMALL, LK_TOA);
  return p;
}

// ------------------------------------------------------------------------------------
// plan_persistent: the launch shape of the register-resident kernel
// ------------------------------------------------------------------------------------
struct PersistPlan {
  int wpb;         // chains per workgroup: the fewest (1, 2, 4) that still fit one workgroup
                   // per CU; tape-mode (parity) launches always use 4
  bool pair;       // two waves per chain when every chain would otherwise leave a SIMD idle
                   // (GST_WAVES_AUTO: C <= 2 ncu) or on request (GST_WAVES_TWO); never in tape
                   // mode, eval_only or GST_STAGE_GRAM launches, which run one wave per chain
  bool occ2;       // the two-chains-per-SIMD build: more chains than SIMDs, NS <= OCC2_NS_MAX
  bool use_prog;   // fair_prio's launch-wide sweep counter
  int grid, block;
  size_t tmfac_bytes;   // timing-model factor scratch [C][waves per chain][slots s < K0][64]
};
inline PersistPlan plan_persistent(int ncu, int C, bool tape, bool eval_only, unsigned mask,
                                   int waves, int NS, int MT, int K0) {
  PersistPlan p;
  p.wpb = tape ? 4 : (C <= ncu ? 1 : (C <= 2 * ncu ? 2 : 4));
  p.pair = !tape && !eval_only && !(mask & GST_STAGE_GRAM) &&
           (waves == GST_WAVES_TWO || (waves == GST_WAVES_AUTO && C <= 2 * ncu));
  p.occ2 = C > 4 * ncu && NS <= OCC2_NS_MAX;
  // two chains per SIMD: the progress rule of fair_prio (with more chains than resident
  // slots, the later workgroups count as behind and the launch's tail shortens: config 4
  // 8.24 -> 8.32 M chain-sweeps/s).  Only in launches that run the red-noise block: the
  // counter's same-address atomics serialise at ~12 ns each across the XCDs, which a full
  // sweep hides but a stage-masked launch of a few microseconds per sweep would be timing
  p.use_prog = !tape && !p.pair && C > 4 * ncu && (mask & GST_STAGE_HYPER);
  p.grid = p.pair ? C : (C + p.wpb - 1) / p.wpb;
  p.block = p.pair ? 128 : 64 * p.wpb;
  const int ntms = MT * (MT + 1) / 2 - (MT - K0) * (MT - K0 + 1) / 2;
  p.tmfac_bytes = (size_t)C * (p.pair ? 2 : 1) * ntms * 64 * sizeof(double);
  return p;
}

}  // namespace gst
