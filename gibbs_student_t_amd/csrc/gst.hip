// C ABI of libgst.so (declared in include/gst.h): context, model upload, sweep launch.
//
// The host side only packs model constants into the layouts the kernel wants and picks
// the template instance (matrix slots MT, TOA slots NS, timing-model panels K0, tape or
// Philox variates).  All chain state lives in caller-owned device buffers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gst.h"
#include "gst_kernel.hpp"
#include "gst_shapes.h"
#include "gst_large.hpp"
#include "gst_pack.h"
#include "gst_plan.h"
#include "gst_sim.hpp"

namespace {

thread_local std::string g_err;

int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}

#define HIP_OK(expr)                                                              \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess)                                                         \
      return fail(std::string(#expr) + ": " + hipGetErrorString(e_));             \
  } while (0)

struct Ctx {
  int device = 0;
  bool has_model = false;
  std::vector<gst::DevModel> hmd;  // host copies, one per dataset
  gst::DevModel* dmd = nullptr;    // device array [nd] (in allocs)
  int nd = 0, nmax = 0, m = 0, raug = 0;
  int MT = 0, NS = 0, K0 = 0;
  bool gen = false;                // persistent path: the general white-noise instances
  int ncu = 256;                   // compute units of the device (workgroup sizing)
  double* tmfac = nullptr;         // persistent path: timing-model factor scratch
  unsigned long long* prog = nullptr;  // persistent path: launch-wide sweep counter (fair_prio)
  size_t tmfac_bytes = 0;
  int path_req = GST_PATH_AUTO;    // gst_set_path
  int path = GST_PATH_PERSISTENT;  // chosen by gst_model_set
  int waves = GST_WAVES_AUTO;      // gst_set_waves
  int debug = 0;                   // gst_set_debug
  unsigned long long* gram_cnt = nullptr;  // persistent path: [2] Grams by path (gst_gram_counts)
  unsigned long long gram_large = 0;       // large path: chain Grams launched (lg_gram*)
  // posterior sums (gst_set_accum): the caller's descriptor and whether its device copy
  // (behind gram_cnt's two counters, gst::accum_desc) is behind: the next accumulating launch
  // rewrites it in stream order
  gst_accum acc{};
  bool acc_on = false, acc_dirty = false;
  // gst_set_accum_toa: the caller's descriptor (zero when unset; it rides in the same device
  // copy) and the chain count its plane stride was last written for
  gst_accum_toa acc_toa{};
  int acc_C = 0;
  // gst_set_accum_block: the caller's descriptor (zero when unset; same device copy)
  gst_accum_block acc_blk{};
  std::vector<void*> allocs;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  // large path: scratch sized for scratch_C chains, per-kernel timing events
  gst::LScratch ls{};
  int scratch_C = 0;
  bool timing = false;
  std::vector<hipEvent_t> evpool;
  std::vector<int> evkind;  // kind of event pair i (events 2i, 2i+1)
  size_t evused = 0;
};

// Scratch that grows inside a launch call is allocated and freed stream-ordered
// (hipMallocAsync / hipFreeAsync on the launch's stream): no device synchronisation inside
// gst_sweep, and a buffer is released only after the work queued before it on that stream.
void free_scratch(Ctx* cx, hipStream_t st) {
  for (double* p : {cx->ls.G, cx->ls.G2, cx->ls.y, cx->ls.w, cx->ls.sc, cx->ls.v, cx->ls.G3})
    if (p) (void)hipFreeAsync(p, st);
  cx->ls = gst::LScratch{};
  cx->scratch_C = 0;
}

int upload(Ctx* cx, const void* host, size_t bytes, void** dev) {
  void* p = nullptr;
  HIP_OK(hipMalloc(&p, bytes > 0 ? bytes : 16));
  if (bytes) HIP_OK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
  cx->allocs.push_back(p);
  *dev = p;
  return 0;
}

void free_tmfac(Ctx* cx, hipStream_t st) {
  if (cx->tmfac) (void)hipFreeAsync(cx->tmfac, st);
  cx->tmfac = nullptr;
  cx->tmfac_bytes = 0;
}

// Model replacement / context teardown (outside any launch): wait for the device, then
// release everything.
void free_model(Ctx* cx) {
  (void)hipDeviceSynchronize();
  for (void* p : cx->allocs) (void)hipFree(p);
  cx->allocs.clear();
  cx->hmd.clear();
  cx->dmd = nullptr;
  cx->nd = 0;
  cx->has_model = false;
  free_scratch(cx, nullptr);
  free_tmfac(cx, nullptr);
  (void)hipDeviceSynchronize();
}

using gst::kfn_t;

// The instance for a shape (gst_shapes.h; each shape's instances live in their own
// translation unit, gst_inst.hip).  wpb: chains per workgroup (4, or 2 / 1 for sampling
// launches with fewer chains than fill every SIMD; tape-mode parity launches always use 4).
// occ2: the two-chains-per-SIMD build (256 registers per lane), picked when the launch has
// more chains than SIMDs; with at most one chain per SIMD the uncapped build keeps more of
// each chain in registers.  pair: two waves per chain (gst_set_waves).
// gen: the general white-noise model's instances (GEN shapes).  acc: the instance that keeps
// the posterior sums (gst_set_accum).
kfn_t pick(int MT, int NS, int K0, int RA, bool gen, bool tape, int wpb, bool occ2,
           bool pair = false, bool acc = false) {
#define GST_CASE(mt, ns, k0, ra, g)                                              \
  if (MT == mt && NS == ns && K0 == k0 && RA == ra && (gen ? 1 : 0) == g)        \
    return gst::GST_PICK_NAME(mt, ns, k0, ra, g)(tape, wpb, occ2, pair, acc);
  GST_SHAPES(GST_CASE)
#undef GST_CASE
  return nullptr;
}

// Register-resident shapes (MT, K0, RA), smallest first: a model with nf Fourier and ntm
// timing-model columns runs in the first with 8 K0 >= ntm and RA - 8 K0 >= nf, padded.
// General white-noise models (GEN) have their own shapes; nf counts the Fourier and the ECORR
// columns there (both sit in the hyper block).
struct Shape {
  int MT, K0, RA;
};
const Shape kShapes[] = {{8, 2, 56}, {10, 2, 76}, {10, 3, 76}};
const Shape kShapesGen[] = {{8, 2, 62}, {10, 2, 76}};

const Shape* shape_for(int nf, int ntm, bool gen = false) {
  const Shape* tab = gen ? kShapesGen : kShapes;
  const int nt = gen ? (int)(sizeof kShapesGen / sizeof(Shape)) : (int)(sizeof kShapes / sizeof(Shape));
  for (int i = 0; i < nt; ++i)
    if (8 * tab[i].K0 >= (ntm > 0 ? ntm : 1) && tab[i].RA - 8 * tab[i].K0 >= nf) return &tab[i];
  return nullptr;
}

using gst::round_up;

// Upload one packed dataset (gst_pack.h) into device buffers owned by cx; md: its DevModel
// with the pointers set (an empty vector stays a null pointer).
template <class T>
int upload_vec(Ctx* cx, const std::vector<T>& v, const T** dev) {
  void* ptr;
  if (v.empty()) return 0;
  if (upload(cx, v.data(), v.size() * sizeof(T), &ptr)) return -1;
  *dev = (const T*)ptr;
  return 0;
}
int upload_dataset(Ctx* cx, const gst::PackedModel& p, gst::DevModel& md) {
  md = p.md;
  return upload_vec(cx, p.Tmf, &md.Tmf) || upload_vec(cx, p.Tcol, &md.Tcol) ||
         upload_vec(cx, p.resid, &md.resid) || upload_vec(cx, p.sig2, &md.sig2) ||
         upload_vec(cx, p.lfreq, &md.lfreq) || upload_vec(cx, p.ldf, &md.ldf) ||
         upload_vec(cx, p.dfA, &md.dfA) || upload_vec(cx, p.dfB, &md.dfB) ||
         upload_vec(cx, p.ref2int, &md.ref2int) || upload_vec(cx, p.cidx, &md.cidx) ||
         upload_vec(cx, p.csig2, &md.csig2) || upload_vec(cx, p.ccount, &md.ccount) ||
         upload_vec(cx, p.Trow, &md.Trow) || upload_vec(cx, p.Gcls, &md.Gcls) ||
         upload_vec(cx, p.bk, &md.bk) || upload_vec(cx, p.ecb, &md.ecb) ||
         upload_vec(cx, p.Tx, &md.Tx) || upload_vec(cx, p.Xe, &md.Xe) ||
         upload_vec(cx, p.ekl, &md.ekl) || upload_vec(cx, p.eblk, &md.eblk)
             ? -1 : 0;
}

// gst_debug_variates: the kernel's own samplers, one draw (kind 0, 1) or four (kind 2) per
// thread, Philox keyed by (seed, chain 0xFFFFFFF0, sweep = call, index, TAG_DEBUG).
constexpr uint32_t TAG_DEBUG = 14u << 24;
__global__ void __launch_bounds__(256) debug_variates_kernel(int kind, double a, double b,
                                                             long long n, unsigned long long seed,
                                                             unsigned call, double* out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  gst::Rng rng;
  rng.k0 = (uint32_t)(seed & 0xffffffffull);
  rng.k1 = (uint32_t)(seed >> 32);
  rng.chain = 0xFFFFFFF0u;
  rng.sweep = call;
  if (kind == 0) {              // gamma_mt(a): the theta stage's Gamma
    if (i < n) out[i] = gst::gamma_mt(a, rng, (uint32_t)i, TAG_DEBUG);
  } else if (kind == 1) {       // the theta stage's Beta(a, b) = Ga / (Ga + Gb)
    if (i < n) {
      const double ga = gst::gamma_mt(a, rng, (uint32_t)(2 * i), TAG_DEBUG);
      const double gb = gst::gamma_mt(b, rng, (uint32_t)(2 * i + 1), TAG_DEBUG);
      out[i] = ga / (ga + gb);
    }
  } else {                      // gamma_mt_slots<4>: the alpha stage's interleaved Gammas
    const long long w = i >> 6, l = i & 63;
    if (256 * w < n) {
      const double sh[4] = {a, a, a, a};
      double g[4];
      gst::gamma_mt_slots<4>(sh, 0xFu, rng, (uint32_t)(256 * w + l), TAG_DEBUG, g);
#pragma unroll
      for (int s = 0; s < 4; ++s) out[256 * w + 64 * s + l] = g[s];
    }
  }
}

}  // namespace

extern "C" {

int gst_version(void) { return GST_ABI_VERSION; }

int gst_tape_stride(int n, int m) { return gst::TP_DELTA + m + 2 + 2 * n; }

int gst_last_error(char* buf, size_t len) {
  if (!buf || !len) return -1;
  std::snprintf(buf, len, "%s", g_err.c_str());
  return 0;
}

int gst_ctx_create(int device, void** ctx) {
  if (!ctx) return fail("gst_ctx_create: null ctx");
  int ndev = 0;
  HIP_OK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail("gst_ctx_create: bad device index");
  HIP_OK(hipSetDevice(device));
  Ctx* cx = new Ctx();
  cx->device = device;
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, device));
  cx->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIP_OK(hipEventCreate(&cx->ev0));
  HIP_OK(hipEventCreate(&cx->ev1));
  HIP_OK(hipMalloc(&cx->prog, 256));   // fair_prio's launch-wide sweep counter
  const size_t cnt_bytes = 2 * sizeof(unsigned long long) + sizeof(gst::DevAccum);
  HIP_OK(hipMalloc(&cx->gram_cnt, cnt_bytes));
  HIP_OK(hipMemset(cx->gram_cnt, 0, cnt_bytes));
  *ctx = cx;
  return 0;
}

int gst_ctx_destroy(void* ctx) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx) return 0;
  (void)hipSetDevice(cx->device);
  free_model(cx);
  if (cx->prog) (void)hipFree(cx->prog);
  if (cx->gram_cnt) (void)hipFree(cx->gram_cnt);
  for (hipEvent_t e : cx->evpool) (void)hipEventDestroy(e);
  if (cx->ev0) (void)hipEventDestroy(cx->ev0);
  if (cx->ev1) (void)hipEventDestroy(cx->ev1);
  delete cx;
  return 0;
}

static int check_desc(const gst_model_desc* d) {
  const int n = d->n, m = d->m, nf = d->nfourier, ntm = d->ntm, P = d->nparams;
  const int nec = d->n_ecorr, nb = d->nbackend > 0 ? d->nbackend : 1;
  if (n <= 0 || nec < 0 || m != nf + ntm + nec || nf <= 0 || ntm < 0)
    return fail("gst_model_set: bad sizes");
  if (P < 1 || P > gst::PMAX) return fail("gst_model_set: nparams must be 1..16");
  if (nb > gst::NBMAX) return fail("gst_model_set: at most 8 backends");
  if (d->idx_equad < 0 || d->idx_log10_A < 0 || d->idx_gamma < 0)
    return fail("gst_model_set: equad, log10_A and gamma parameters are required");
  if (d->n_hyper < 1 || d->n_hyper > P || d->n_white < 1 || d->n_white > P)
    return fail("gst_model_set: bad hyper/white index sets");
  if (!d->T || !d->residuals || !d->toaerrs || !d->ffreqs || !d->pmin || !d->pmax ||
      !d->hyper_idx || !d->white_idx || !d->df_A || !d->df_B)
    return fail("gst_model_set: null array in model descriptor");
  if ((nb > 1 && !d->backend) || (nec > 0 && (!d->ecorr_backend || !d->ecorr_idx)))
    return fail("gst_model_set: backend / ECORR arrays missing");
  for (int t = 0; nb > 1 && t < n; ++t)
    if (d->backend[t] < 0 || d->backend[t] >= nb) return fail("gst_model_set: bad backend index");
  for (int b = 0; b < nb; ++b) {
    const int ef = d->efac_idx ? d->efac_idx[b] : d->idx_efac;
    const int eq = d->equad_idx ? d->equad_idx[b] : d->idx_equad;
    const int ec = d->ecorr_idx ? d->ecorr_idx[b] : -1;
    if (ef >= P || eq < 0 || eq >= P || ec >= P) return fail("gst_model_set: bad parameter index");
  }
  for (int e = 0; e < nec; ++e) {
    const int b = d->ecorr_backend[e];
    if (b < 0 || b >= nb || d->ecorr_idx[b] < 0)
      return fail("gst_model_set: ECORR column without an ecorr parameter");
  }
  return 0;
}

// The classic model of the register-resident kernel: one backend, no ECORR, P <= 4.
static bool classic(const gst_model_desc* d) {
  return (d->nbackend <= 1) && d->n_ecorr == 0 && d->nparams <= 4 && d->n_hyper <= 4 &&
         d->n_white <= 4;
}
// The general white-noise model its GEN instances take: per-backend efac / equad (<= 8
// backends), ECORR epoch columns in the hyper block, up to 8 parameters.
static bool general_fits(const gst_model_desc* d) {
  return d->nparams <= 8 && d->n_hyper <= 8 && d->n_white <= 8 &&
         (d->nbackend > 0 ? d->nbackend : 1) <= gst::NBMAX;
}

// Datasets of one batch share the sampler structure: basis shape, parameter roles and the
// MH index sets.  n (ragged run_sims datasets), the data and the outlier model may differ.
static int same_structure(const gst_model_desc* a, const gst_model_desc* b) {
  if (a->m != b->m || a->nfourier != b->nfourier || a->ntm != b->ntm ||
      a->nparams != b->nparams || a->idx_efac != b->idx_efac || a->idx_equad != b->idx_equad ||
      a->idx_log10_A != b->idx_log10_A || a->idx_gamma != b->idx_gamma ||
      a->n_hyper != b->n_hyper || a->n_white != b->n_white || a->n_ecorr != b->n_ecorr ||
      (a->nbackend > 1 ? a->nbackend : 1) != (b->nbackend > 1 ? b->nbackend : 1))
    return 0;
  for (int j = 0; j < a->n_hyper; ++j)
    if (a->hyper_idx[j] != b->hyper_idx[j]) return 0;
  for (int j = 0; j < a->n_white; ++j)
    if (a->white_idx[j] != b->white_idx[j]) return 0;
  return 1;
}

// The power-law processes of the Fourier block against the descriptor they split
static int check_procs(const gst_model_desc* d, const gst_model_procs* pr) {
  if (pr->nproc < 1 || pr->nproc > GST_NPROC_MAX)
    return fail("gst_model_set_procs: nproc must be 1..3");
  int sum = 0;
  for (int p = 0; p < pr->nproc; ++p) {
    if (pr->ncol[p] <= 0 || pr->ncol[p] % 2)
      return fail("gst_model_set_procs: every ncol must be even and positive");
    sum += pr->ncol[p];
    bool hasA = false, hasG = false;
    for (int j = 0; j < d->n_hyper; ++j) {
      hasA = hasA || d->hyper_idx[j] == pr->idx_log10_A[p];
      hasG = hasG || d->hyper_idx[j] == pr->idx_gamma[p];
    }
    if (!hasA || !hasG || pr->idx_log10_A[p] < 0 || pr->idx_log10_A[p] >= d->nparams ||
        pr->idx_gamma[p] < 0 || pr->idx_gamma[p] >= d->nparams)
      return fail("gst_model_set_procs: a process's log10_A / gamma index is not a hyper "
                  "parameter");
  }
  if (sum != d->nfourier) return fail("gst_model_set_procs: the ncol do not sum to nfourier");
  if (pr->idx_log10_A[0] != d->idx_log10_A || pr->idx_gamma[0] != d->idx_gamma)
    return fail("gst_model_set_procs: process 0 must be the descriptor's log10_A / gamma");
  return 0;
}

// gst_model_set_batch / gst_model_set_procs: procs null is the red noise alone
static int model_set(void* ctx, const gst_model_desc* descs, const gst_model_procs* procs,
                     int nd) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx || !descs || nd <= 0) return fail("gst_model_set_batch: null argument");
  HIP_OK(hipSetDevice(cx->device));
  // 1. validate
  int nmax = 0;
  for (int i = 0; i < nd; ++i) {
    if (check_desc(&descs[i])) return -1;
    if (procs && check_procs(&descs[i], procs)) return -1;
    if (!same_structure(&descs[0], &descs[i]))
      return fail("gst_model_set_batch: datasets differ in basis shape, parameters or MH "
                  "index sets (dataset " + std::to_string(i) + ")");
    nmax = std::max(nmax, descs[i].n);
  }
  // 2. shape and path
  const gst_model_desc* d = &descs[0];
  const int nf = d->nfourier, ntm = d->ntm, m = d->m, nec = d->n_ecorr;
  bool disjoint = true;   // the batch's datasets all: one hyper class per batch structure
  for (int i = 0; i < nd && nec > 0; ++i) disjoint = disjoint && gst::ecorr_disjoint(&descs[i]);
  const bool gen = !classic(d) && general_fits(d);
  const Shape* sh = shape_for(nf + (gen ? nec : 0), ntm, gen);
  const int MT = sh ? sh->MT : 0, K0 = sh ? sh->K0 : 0;
  const int raug = sh ? sh->RA : 0;
  const int nsl = (nmax + 63) / 64;
  // TOA slots of 64 held in registers: 2, 3, 4 (J1713-sized), 6, 8 (mid-size, n <= 512),
  // 12, 16 (wide mid-size, n <= 1024: the run_sims model's shape only; these keep one chain
  // per SIMD, their two-chains-per-SIMD builds would spill kilobytes per lane)
  // (the general white-noise model: 2, 3 (MT = 10 only), 4, 8); the smallest instantiated
  // slot count that holds n
  static const int kSlots[] = {2, 3, 4, 6, 8, 12, 16};
  int NS = 16;
  for (int ns : kSlots)
    if (ns >= nsl && sh && pick(MT, ns, K0, raug, gen, false, 4, false)) { NS = ns; break; }
  const bool fits = sh && (classic(d) || gen) && round_up(nmax, 4) <= 64 * NS &&
                    pick(MT, NS, K0, raug, gen, false, 4, false);
  int path = cx->path_req;
  if (path == GST_PATH_AUTO) path = fits ? GST_PATH_PERSISTENT : GST_PATH_LARGE;
  if (path == GST_PATH_PERSISTENT && !fits) {
    char b[220];
    std::snprintf(b, sizeof b,
                  "gst_model_set: no persistent-kernel instance for MT=%d NS=%d K0=%d RA=%d "
                  "GEN=%d (n=%d m=%d nfourier=%d ntm=%d n_ecorr=%d); use the large path", MT, NS,
                  K0, raug, gen ? 1 : 0, nmax, m, nf, ntm, nec);
    return fail(b);
  }
  const bool large = path == GST_PATH_LARGE;
  // large path: timing-model block padded to whole 16-column MFMA tiles, no dummies
  const int ntm_pad = large ? round_up(ntm > 0 ? ntm : 1, 16) : 8 * K0;
  const int raug_pack = large ? ntm_pad + nf + nec : raug;
  // 3. large path: the LDS layouts of its kernels (gst_plan.h), from the descriptor's
  // integers.  Hyper blocks past HYPER_LDS_MAX columns: ECORR epochs around a small
  // timing-model + Fourier block are eliminated first (lg_hyper<2>), other blocks are factored
  // in global memory (lg_hyper<1>), whose LDS holds a 16-column panel of all mp rows
  const int mpl = round_up(raug_pack + 1, 16);
  const size_t limit = gst::LDS_LIMIT;
  const size_t lds_h0 = (size_t)gst::HyperLds<0>(nf, nec, ntm, mpl).total * 8;
  const size_t lds_h1 = (size_t)gst::HyperLds<1>(nf, nec, ntm, mpl).total * 8;
  const size_t lds_h2 = (size_t)gst::HyperLds<2>(nf, nec, ntm, mpl).total * 8;
  const int hc = gst::hyper_class(nf + nec, 0, nec, ntm + nf + 1, disjoint ? 1 : 0);
  if (large && hc == 1 && lds_h1 > limit)
    return fail("gst_model_set: large path: basis too large for the LDS panel of the "
                "red-noise / ECORR block elimination");
  if (large && hc == 2 && lds_h2 > limit)   // its LDS vectors span the basis
    return fail("gst_model_set: large path: too many ECORR epochs for the LDS of their "
                "elimination");
  // 4. pack and upload
  free_model(cx);
  std::vector<gst::DevModel> hmd(nd);
  for (int i = 0; i < nd; ++i)
    if (upload_dataset(cx, gst::pack_dataset(&descs[i], ntm_pad, raug_pack, large ? 0 : MT, disjoint,
                                             procs),
                       hmd[i])) {
      free_model(cx);
      return -1;
    }
  void* ptr;
  if (upload(cx, hmd.data(), hmd.size() * sizeof(gst::DevModel), &ptr)) return -1;
  cx->dmd = (gst::DevModel*)ptr;
  cx->hmd = hmd;
  cx->nd = nd;
  cx->nmax = nmax;
  cx->MT = MT;
  cx->NS = NS;
  cx->K0 = K0;
  cx->raug = raug_pack;
  cx->m = m;
  cx->gen = !large && gen;
  cx->path = path;
  if (large) {
    auto set_lds = [](const void* kern, size_t bytes) {
      return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    };
    HIP_OK(set_lds((const void*)gst::lg_gram, gst::GRAM_LDS * 8));
    HIP_OK(set_lds((const void*)gst::lg_tmelim, (size_t)gst::TmelimLds(mpl).total * 8));
    HIP_OK(set_lds((const void*)gst::lg_btm, (size_t)gst::BtmLds(ntm_pad, raug_pack).total * 8));
    // lg_hyper<0>: class 0, and smaller blocks under GST_DEBUG_LARGE_HYPER; lg_hyper<1>: class
    // 1, and class 2 under GST_DEBUG_LARGE_HYPER when its panel fits (plan_large refuses else)
    if (nf + nec <= gst::HYPER_LDS_MAX) HIP_OK(set_lds((const void*)gst::lg_hyper<0>, lds_h0));
    if (nf + nec > gst::HYPER_LDS_MAX && lds_h1 <= limit)
      HIP_OK(set_lds((const void*)gst::lg_hyper<1>, lds_h1));
    if (hc == 2) HIP_OK(set_lds((const void*)gst::lg_hyper<2>, lds_h2));
  }
  cx->has_model = true;
  // a block's column range belongs to the model it was checked against
  cx->acc_blk = gst_accum_block{};
  cx->acc_dirty = cx->acc_on;
  return 0;
}


int gst_model_set_batch(void* ctx, const gst_model_desc* descs, int nd) {
  return model_set(ctx, descs, nullptr, nd);
}

int gst_model_set_procs(void* ctx, const gst_model_desc* descs, const gst_model_procs* procs,
                        int nd) {
  return model_set(ctx, descs, procs, nd);
}

int gst_model_set(void* ctx, const gst_model_desc* d) { return model_set(ctx, d, nullptr, 1); }

int gst_model_info(void* ctx, int* ndatasets, int* nmax, int* tape_stride) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx || !cx->has_model) return fail("gst_model_info: no model set");
  if (ndatasets) *ndatasets = cx->nd;
  if (nmax) *nmax = cx->nmax;
  if (tape_stride) *tape_stride = gst_tape_stride(cx->nmax, cx->m);
  return 0;
}

// timing events (gst_set_timing): pair i brackets one launch of kernel kind evkind[i]
static int ev_mark(Ctx* cx, int kind, hipStream_t st, bool begin) {
  if (!cx->timing) return 0;
  if (begin) {
    if (2 * cx->evused + 2 > cx->evpool.size()) {
      hipEvent_t e0, e1;
      HIP_OK(hipEventCreate(&e0));
      HIP_OK(hipEventCreate(&e1));
      cx->evpool.push_back(e0);
      cx->evpool.push_back(e1);
      cx->evkind.push_back(0);
    }
    cx->evkind[cx->evused] = kind;
    HIP_OK(hipEventRecord(cx->evpool[2 * cx->evused], st));
  } else {
    HIP_OK(hipEventRecord(cx->evpool[2 * cx->evused + 1], st));
    ++cx->evused;
  }
  return 0;
}

// npad: the per-TOA scratch row stride (the batch's largest npad); need_g3: lg_hyper<1> runs
// (class-1 models, and class-2 ones under GST_DEBUG_LARGE_HYPER)
static int ensure_scratch(Ctx* cx, int C, size_t npad, bool need_g3, hipStream_t st) {
  if (C <= cx->scratch_C && (!need_g3 || cx->ls.G3)) return 0;
  if (C <= cx->scratch_C) {
    const size_t mp = cx->hmd[0].mp;
    HIP_OK(hipMallocAsync((void**)&cx->ls.G3, (size_t)cx->scratch_C * mp * mp * 8, st));
    HIP_OK(hipMemsetAsync(cx->ls.G3, 0, (size_t)cx->scratch_C * mp * mp * 8, st));
    return 0;
  }
  free_scratch(cx, st);
  const gst::DevModel& h = cx->hmd[0];
  const size_t mp = h.mp;
  HIP_OK(hipMallocAsync((void**)&cx->ls.G, (size_t)C * mp * mp * 8, st));
  HIP_OK(hipMallocAsync((void**)&cx->ls.G2, (size_t)C * mp * mp * 8, st));
  HIP_OK(hipMallocAsync((void**)&cx->ls.y, (size_t)C * npad * 8, st));
  HIP_OK(hipMallocAsync((void**)&cx->ls.w, (size_t)C * npad * 8, st));
  HIP_OK(hipMallocAsync((void**)&cx->ls.sc, (size_t)C * 16 * 8, st));
  HIP_OK(hipMallocAsync((void**)&cx->ls.v, (size_t)C * mp * 8, st));
  HIP_OK(hipMemsetAsync(cx->ls.G, 0, (size_t)C * mp * mp * 8, st));
  HIP_OK(hipMemsetAsync(cx->ls.G2, 0, (size_t)C * mp * mp * 8, st));
  HIP_OK(hipMemsetAsync(cx->ls.sc, 0, (size_t)C * 16 * 8, st));
  HIP_OK(hipMemsetAsync(cx->ls.v, 0, (size_t)C * mp * 8, st));
  if (need_g3) {   // lg_hyper<1>'s factor of the red-noise / ECORR block
    HIP_OK(hipMallocAsync((void**)&cx->ls.G3, (size_t)C * mp * mp * 8, st));
    HIP_OK(hipMemsetAsync(cx->ls.G3, 0, (size_t)C * mp * mp * 8, st));
  }
  cx->scratch_C = C;
  return 0;
}

// The large path's kernels by id (gst_plan.h LargeKernel); lg_gram takes two more arguments
using lkfn_t = void (*)(const gst::DevModel*, gst::LArgs);
static const lkfn_t kLargeKernels[gst::LK_COUNT] = {
    gst::lg_tb, gst::lg_record,
    gst::lg_white<gst::TBLK_WAVE>, gst::lg_white<gst::TBLK_SMALL>, gst::lg_white<gst::TBLK>,
    gst::lg_gram_ec<1>, gst::lg_gram_ec<2>, gst::lg_gram_ec<3>, gst::lg_gram_ec<4>,
    gst::lg_gram_small<1>, gst::lg_gram_small<2>, gst::lg_gram_small<3>, gst::lg_gram_small<4>,
    gst::lg_gram_small<5>, gst::lg_gram_small<6>, nullptr /* lg_gram */,
    gst::lg_tmelim,
    gst::lg_hyper_reg<8>, gst::lg_hyper_reg<16>, gst::lg_hyper<0>, gst::lg_hyper<1>,
    gst::lg_hyper<2>, gst::lg_hyper_ecr<6, 46>, gst::lg_hyper_ecr<8, 62>,
    gst::lg_btm,
    gst::lg_toa<gst::TBLK_SMALL>, gst::lg_toa<gst::TBLK>, gst::lg_accum};

static int run_launch(Ctx* cx, const gst::LargePlan& p, const gst::Launch& l, gst::LArgs& a,
                      hipStream_t st) {
  if (l.kclass >= 0) a.kclass = l.kclass;
  a.floor_pass = l.floor_pass;
  if ((l.ev & gst::EV_BEGIN) && ev_mark(cx, l.kind, st, true)) return -1;
  const dim3 grid(l.gx, l.gy), block(l.block);
  if (l.kernel == gst::LK_GRAM)
    hipLaunchKernelGGL(gst::lg_gram, grid, block, l.lds, st, cx->dmd, a, p.nsb, p.npairs);
  else
    hipLaunchKernelGGL(kLargeKernels[l.kernel], grid, block, l.lds, st, cx->dmd, a);
  HIP_OK(hipGetLastError());
  if ((l.ev & gst::EV_END) && ev_mark(cx, l.kind, st, false)) return -1;
  // one count per chain per Gram stage (gst_gram_counts)
  if ((l.ev & gst::EV_END) && l.kind == GST_K_GRAM && !a.eval_only)
    cx->gram_large += (unsigned long long)a.C;
  return 0;
}

// The plan (gst_plan.h plan_large) is built once per call; its sweep list runs nsweeps times.
static int launch_large(Ctx* cx, const gst::DevState& ds, const gst::DevRec& dr,
                        const gst::DevTape& dt, int C, int nsweeps, long long sweep0,
                        int record_every, unsigned mask, unsigned long long seed,
                        long long chain0, int eval_only, bool acc_on, double* ow, double* oh,
                        hipStream_t st) {
  const gst::LargePlan p = gst::plan_large(cx->hmd.data(), cx->nd, cx->debug, C, mask,
                                           eval_only != 0, record_every > 0 && !eval_only,
                                           acc_on);
  if (!p.error.empty()) return fail(p.error);
  if (ensure_scratch(cx, C, p.ys, p.need_g3, st)) return -1;
  gst::LArgs a{ds, dr, dt, cx->ls, p.ys, C, nsweeps, 0, record_every, mask, seed, sweep0, chain0,
               eval_only, ow, oh};
  a.hyper_lds = p.hyper_lds;
  cx->evused = 0;
  HIP_OK(hipEventRecord(cx->ev0, st));
  for (const gst::Launch& l : p.prologue)
    if (run_launch(cx, p, l, a, st)) return -1;
  const int nit = eval_only ? 1 : nsweeps;
  for (int it = 0; it < nit; ++it) {
    a.it = it;
    for (const gst::Launch& l : p.sweep) {
      if (l.record && it % record_every) continue;
      if (l.kernel == gst::LK_ACCUM && sweep0 + it < cx->acc.from_sweep) continue;
      if (run_launch(cx, p, l, a, st)) return -1;
    }
  }
  HIP_OK(hipEventRecord(cx->ev1, st));
  cx->timed = true;
  return 0;
}

// The context's device copy of the accumulator descriptor is written by a kernel, so that it
// is ordered on the stream with the launches that read it
static __global__ void set_accum_kernel(gst::DevAccum* dst, gst::DevAccum v) { *dst = v; }

static int launch(Ctx* cx, const gst_state* s, const gst_records* r, const gst_tape* tp,
                  int C, int nsweeps, long long sweep0, int record_every, unsigned mask,
                  unsigned long long seed, long long chain0, int eval_only, double* ow,
                  double* oh, void* stream) {
  if (!cx || !cx->has_model) return fail("gst: no model set");
  if (!s || !s->x || !s->b || !s->z || !s->alpha || !s->pout || !s->theta || !s->nu)
    return fail("gst: state pointers must all be set");
  if (C <= 0) return 0;
  HIP_OK(hipSetDevice(cx->device));
  const bool tape = tp && tp->data;
  if (!s->dataset && cx->nd > 1)
    return fail("gst: the model has several datasets: state.dataset must be set");
  gst::DevState ds{s->x,     s->b,  s->z,      s->alpha,   s->pout, s->theta,
                   s->nu,    s->status, s->dataset, cx->nmax, cx->nd, nullptr, nullptr,
                   cx->debug, eval_only ? nullptr : cx->gram_cnt};
  // posterior sums: sampling launches that reach from_sweep (never eval_only / GST_STAGE_GRAM)
  const bool acc_on = cx->acc_on && !eval_only && !(mask & GST_STAGE_GRAM) &&
                      sweep0 + nsweeps > cx->acc.from_sweep;
  // (pout_gt's plane stride is the launch's chain count times nmax)
  if (acc_on && (cx->acc_dirty || (cx->acc_toa.pout_gt && C != cx->acc_C))) {
    const gst_accum& h = cx->acc;
    const gst_accum_toa& t = cx->acc_toa;
    const gst_accum_block& k = cx->acc_blk;
    hipLaunchKernelGGL(set_accum_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream,
                       gst::accum_desc(cx->gram_cnt),
                       gst::DevAccum{h.z_sum, h.pout_sum, h.alpha_sum, h.b_sum, h.b_sq, h.count,
                                     h.from_sweep, t.pout_gt, t.resid_sum, t.resid_sq,
                                     {t.thr[0], t.thr[1], t.thr[2], t.thr[3]},
                                     (long long)C * cx->nmax, t.pout_gt ? t.nthr : 0,
                                     k.col0, k.ncol, k.bb});
    HIP_OK(hipGetLastError());
    cx->acc_dirty = false;
    cx->acc_C = C;
  }
  gst::DevRec dr{};
  if (r) dr = gst::DevRec{r->x, r->b, r->z, r->alpha, r->pout, r->theta, r->nu, r->nrec};
  else record_every = 0;
  if (tape && tp->stride != gst_tape_stride(cx->nmax, cx->m))
    return fail("gst: tape stride mismatch");
  gst::DevTape dt{tape ? tp->data : nullptr, tape ? tp->stride : 0};
  if (cx->path == GST_PATH_LARGE)
    return launch_large(cx, ds, dr, dt, C, nsweeps, sweep0, record_every, mask, seed, chain0,
                        eval_only, acc_on, ow, oh, (hipStream_t)stream);
  const gst::PersistPlan p = gst::plan_persistent(cx->ncu, C, tape, eval_only != 0, mask, cx->waves,
                                                  cx->NS, cx->MT, cx->K0);
  kfn_t k = pick(cx->MT, cx->NS, cx->K0, cx->raug, cx->gen, tape, p.wpb, p.occ2, p.pair,
                 acc_on);
  if (!k) return fail("gst: no kernel instance");
  hipStream_t st = (hipStream_t)stream;
  if (p.tmfac_bytes > cx->tmfac_bytes) {
    free_tmfac(cx, st);
    HIP_OK(hipMallocAsync((void**)&cx->tmfac, p.tmfac_bytes, st));
    cx->tmfac_bytes = p.tmfac_bytes;
  }
  ds.tmfac = cx->tmfac;
  if (p.use_prog) {
    HIP_OK(hipMemsetAsync(cx->prog, 0, sizeof(unsigned long long), st));
    ds.prog = cx->prog;
  }
  HIP_OK(hipEventRecord(cx->ev0, st));
  hipLaunchKernelGGL(k, dim3(p.grid), dim3(p.block), 0, st, cx->dmd, ds, dr, dt, C, nsweeps, sweep0,
                     record_every, mask, seed, chain0, eval_only, ow, oh);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(cx->ev1, st));
  cx->timed = true;
  return 0;
}

int gst_sweep(void* ctx, const gst_state* state, const gst_records* rec, const gst_tape* tape,
              int nchains, int nsweeps, long long sweep0, int record_every,
              unsigned stage_mask, unsigned long long seed, long long chain0, void* stream) {
  if (nsweeps < 0) return fail("gst_sweep: nsweeps < 0");
  if (rec && record_every > 0 && rec->nrec < (nsweeps + record_every - 1) / record_every)
    return fail("gst_sweep: record buffer too small");
  return launch(static_cast<Ctx*>(ctx), state, rec, tape, nchains, nsweeps, sweep0,
                record_every, stage_mask, seed, chain0, 0, nullptr, nullptr, stream);
}

int gst_eval_lnlike(void* ctx, const gst_state* state, int nchains, double* out_white,
                    double* out_hyper, void* stream) {
  if (!out_white || !out_hyper) return fail("gst_eval_lnlike: null outputs");
  return launch(static_cast<Ctx*>(ctx), state, nullptr, nullptr, nchains, 0, 0, 0, 0u, 0ull,
                0, 1, out_white, out_hyper, stream);
}

int gst_set_accum(void* ctx, const gst_accum* acc) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx) return fail("gst_set_accum: null ctx");
  cx->acc_on = acc != nullptr;
  cx->acc = acc ? *acc : gst_accum{};
  cx->acc_dirty = cx->acc_on;
  return 0;
}

int gst_set_accum_toa(void* ctx, const gst_accum_toa* a) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx) return fail("gst_set_accum_toa: null ctx");
  if (a) {
    if (a->nthr < 0 || a->nthr > 4) return fail("gst_set_accum_toa: nthr must be 0..4");
    for (int k = 0; k < a->nthr; ++k)
      if (!(a->thr[k] > 0.0 && a->thr[k] < 1.0) || (k > 0 && !(a->thr[k] > a->thr[k - 1])))
        return fail("gst_set_accum_toa: thresholds must be strictly increasing in (0, 1)");
  }
  cx->acc_toa = a ? *a : gst_accum_toa{};
  if (cx->acc_toa.nthr == 0) cx->acc_toa.pout_gt = nullptr;
  for (int k = cx->acc_toa.nthr; k < 4; ++k) cx->acc_toa.thr[k] = 0.0;
  cx->acc_dirty = cx->acc_on;
  return 0;
}

int gst_set_accum_block(void* ctx, const gst_accum_block* blk) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx) return fail("gst_set_accum_block: null ctx");
  if (blk) {
    if (!cx->has_model) return fail("gst_set_accum_block: no model set");
    if (blk->col0 < 0) return fail("gst_set_accum_block: col0 must be >= 0");
    if (blk->ncol < 1 || blk->ncol > GST_BLOCK_MAX)
      return fail("gst_set_accum_block: ncol must be 1.." + std::to_string(GST_BLOCK_MAX));
    if (blk->col0 > cx->m - blk->ncol)
      return fail("gst_set_accum_block: col0 + ncol exceeds the model's " +
                  std::to_string(cx->m) + " columns");
  }
  cx->acc_blk = blk && blk->bb ? *blk : gst_accum_block{};
  cx->acc_dirty = cx->acc_on;
  return 0;
}

int gst_debug_stamps(void* ctx, unsigned long long* dev_buf) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx || !cx->has_model) return fail("gst_debug_stamps: no model");
#ifdef GST_STAMPS
  for (auto& h : cx->hmd) h.stamps = dev_buf;
  HIP_OK(hipMemcpy(cx->dmd, cx->hmd.data(), cx->hmd.size() * sizeof(gst::DevModel),
                   hipMemcpyHostToDevice));
  return 0;
#else
  (void)dev_buf;
  return fail("gst_debug_stamps: library built without GST_STAMPS");
#endif
}

int gst_sync(void* ctx, void* stream) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (cx) HIP_OK(hipSetDevice(cx->device));
  HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int gst_set_path(void* ctx, int path) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx) return fail("gst_set_path: null ctx");
  if (path < GST_PATH_AUTO || path > GST_PATH_LARGE) return fail("gst_set_path: bad path");
  cx->path_req = path;
  return 0;
}

int gst_set_waves(void* ctx, int waves) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx) return fail("gst_set_waves: null ctx");
  if (waves < GST_WAVES_AUTO || waves > GST_WAVES_TWO) return fail("gst_set_waves: bad value");
  cx->waves = waves;
  return 0;
}

int gst_set_debug(void* ctx, int flags) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx) return fail("gst_set_debug: null ctx");
  if (flags & ~(GST_DEBUG_POISON | GST_DEBUG_LARGE_GRAM | GST_DEBUG_LARGE_HYPER |
                GST_DEBUG_EXACT_BDRAW | GST_DEBUG_MFMA_GRAM | GST_DEBUG_EPOCHS_LDS))
    return fail("gst_set_debug: unknown flag");
  cx->debug = flags;
  return 0;
}

int gst_get_path(void* ctx, int* path) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx || !path) return fail("gst_get_path: null argument");
  if (!cx->has_model) return fail("gst_get_path: no model set");
  *path = cx->path;
  return 0;
}

int gst_set_timing(void* ctx, int on) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx) return fail("gst_set_timing: null ctx");
  cx->timing = on != 0;
  return 0;
}

int gst_kernel_times(void* ctx, double* ms, int* launches, int nkinds) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx || !ms || !launches) return fail("gst_kernel_times: null argument");
  for (int k = 0; k < nkinds; ++k) {
    ms[k] = 0.0;
    launches[k] = 0;
  }
  for (size_t i = 0; i < cx->evused; ++i) {
    const int k = cx->evkind[i];
    if (k < 0 || k >= nkinds) continue;
    HIP_OK(hipEventSynchronize(cx->evpool[2 * i + 1]));
    float f = 0.f;
    HIP_OK(hipEventElapsedTime(&f, cx->evpool[2 * i], cx->evpool[2 * i + 1]));
    ms[k] += f;
    launches[k] += 1;
  }
  return 0;
}

int gst_simulate(const gst_sim_desc* d, void* stream) {
  if (!d) return fail("gst_simulate: null descriptor");
  if (d->n <= 0 || d->ndatasets < 0 || d->ntm < 0 || d->nfourier < 0)
    return fail("gst_simulate: bad sizes");
  if (d->ndatasets == 0) return 0;
  if (d->nfourier > gst::SIM_MAX_NF || d->ntm > gst::SIM_MAX_NF)
    return fail("gst_simulate: nfourier and ntm must be <= 512");
  if (d->residuals_clean && d->ntm > gst::SIM_MAX_TM_CLEAN)
    return fail("gst_simulate: the clean twin needs ntm <= 64");
  if (!d->red && (!d->F || !d->log_f || !d->log_df) && d->nfourier > 0)
    return fail("gst_simulate: power-law red noise needs F, log_f and log_df");
  if ((d->ntm > 0 && !d->U) || !d->theta || !d->sigma_out || !d->dof ||
      (!d->red && (!d->log10_A || !d->gamma)) || !d->residuals || !d->toaerrs_out || !d->z)
    return fail("gst_simulate: missing pointer");
  gst::SimArgs a{};
  a.n = d->n;
  a.nf = d->red ? 0 : d->nfourier;
  a.ntm = d->ntm;
  a.D = d->ndatasets;
  a.F = d->F;
  a.lf = d->log_f;
  a.ldf = d->log_df;
  a.log_fyr = d->log_fyr;
  a.log_12pi2 = std::log(12.0) + 2.0 * std::log(M_PI);
  a.U = d->U;
  a.red = d->red;
  a.err_in = d->toaerrs;
  a.theta = d->theta;
  a.sigma_out = d->sigma_out;
  a.log10_A = d->log10_A;
  a.gamma = d->gamma;
  a.dof = d->dof;
  a.k0 = (uint32_t)(d->seed & 0xffffffffull);
  a.k1 = (uint32_t)(d->seed >> 32);
  a.ds0 = d->dataset0;
  a.r = d->residuals;
  a.err = d->toaerrs_out;
  a.z = d->z;
  a.r_clean = d->residuals_clean;
  hipLaunchKernelGGL(gst::gst_simulate_kernel, dim3(d->ndatasets), dim3(gst::SIM_BLOCK), 0,
                     (hipStream_t)stream, a);
  HIP_OK(hipGetLastError());
  return 0;
}

int gst_gram_counts(void* ctx, long long* counts, int reset) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx || !counts) return fail("gst_gram_counts: null argument");
  HIP_OK(hipSetDevice(cx->device));
  HIP_OK(hipDeviceSynchronize());
  unsigned long long h[2] = {0ull, 0ull};
  HIP_OK(hipMemcpy(h, cx->gram_cnt, sizeof h, hipMemcpyDeviceToHost));
  counts[0] = (long long)h[0];
  counts[1] = (long long)h[1];
  counts[2] = (long long)cx->gram_large;
  if (reset) {
    HIP_OK(hipMemset(cx->gram_cnt, 0, sizeof h));
    cx->gram_large = 0;
  }
  return 0;
}

int gst_debug_variates(int kind, double a, double b, long long n, unsigned long long seed,
                       unsigned call, double* out, void* stream) {
  if (!out || n < 0) return fail("gst_debug_variates: bad argument");
  if (kind < 0 || kind > 2) return fail("gst_debug_variates: kind must be 0, 1 or 2");
  if (!(a > 0.0) || (kind == 1 && !(b > 0.0))) return fail("gst_debug_variates: shapes must be > 0");
  if ((kind == 2 && n % 256) || n > (1ll << 31))
    return fail("gst_debug_variates: n must be <= 2^31 (kind 2: a multiple of 256)");
  if (n == 0) return 0;
  const long long threads = kind == 2 ? n / 4 : n;
  hipLaunchKernelGGL(debug_variates_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, kind, a, b, n, seed, call, out);
  HIP_OK(hipGetLastError());
  return 0;
}

int gst_last_sweep_ms(void* ctx, double* ms) {
  Ctx* cx = static_cast<Ctx*>(ctx);
  if (!cx || !ms) return fail("gst_last_sweep_ms: null argument");
  if (!cx->timed) return fail("gst_last_sweep_ms: nothing launched");
  HIP_OK(hipEventSynchronize(cx->ev1));
  float f = 0.f;
  HIP_OK(hipEventElapsedTime(&f, cx->ev0, cx->ev1));
  *ms = f;
  return 0;
}

}  // extern "C"
