/*
 * gst.h -- C ABI of the MI355X-native batched Gibbs sampler (libgst.so).
 *
 * Drop-in boundary for the reference's Python sampler `Gibbs` (/root/reference/gibbs.py).
 * The reference has no FFI: its "interface" is the Python class.  These entry points are
 * what a ctypes (or cgo/JNI) binding of that class binds; INTEGRATION.md shows the
 * ctypes stub.  Each entry point names the reference code it replaces.
 *
 * Conventions
 *  - every function returns int: 0 = ok, < 0 = error; gst_last_error() gives the message
 *    (thread-local).  No C++ exception crosses the ABI.
 *  - all chain buffers are DEVICE pointers owned by the caller (PyTorch-ROCm tensors'
 *    data_ptr()), fp64, laid out chain-major (struct-of-arrays); the library owns only the
 *    model constants it uploads in gst_model_set and its own scratch.
 *  - `stream` is a hipStream_t (may be NULL = default stream).  No host synchronisation
 *    happens inside gst_sweep; gst_sync() waits for the stream.
 *  - one ctx per device; not re-entrant across threads, and used from one stream at a
 *    time: its scratch (the persistent path's parked timing-model factors and sweep
 *    counter, the large path's per-chain buffers) is shared by all of its launches and
 *    indexed by launch-local chain, so two concurrent gst_sweep calls on different streams
 *    would race on it.  Scratch grows with stream-ordered allocation (hipMallocAsync /
 *    hipFreeAsync on the launch's stream), never with a device-synchronising hipFree.
 */
#ifndef GST_H_
#define GST_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GST_ABI_VERSION 7

/* Outlier model kind: Gibbs(model=...) (gibbs.py:9,32,187-226). */
enum gst_outlier_model {
  GST_MODEL_GAUSSIAN = 0,
  GST_MODEL_T = 1,
  GST_MODEL_MIXTURE = 2,
  GST_MODEL_VVH17 = 3
};

/* Stage mask for gst_sweep (the per-sweep stage order of gibbs.py:363-380). */
enum gst_stage {
  GST_STAGE_WHITE = 1u << 0, /* update_white_params  gibbs.py:114-143 */
  GST_STAGE_HYPER = 1u << 1, /* update_hyper_params  gibbs.py:80-111 */
  GST_STAGE_B = 1u << 2,     /* update_b             gibbs.py:145-182 (+ quirk :373) */
  GST_STAGE_THETA = 1u << 3, /* update_theta         gibbs.py:185-198 */
  GST_STAGE_Z = 1u << 4,     /* update_z             gibbs.py:201-226 */
  GST_STAGE_ALPHA = 1u << 5, /* update_alpha         gibbs.py:229-242 */
  GST_STAGE_DF = 1u << 6,    /* update_df            gibbs.py:244-259 */
  GST_STAGE_ALL = 0x7fu,
  GST_STAGE_B_FORCE = 1u << 7, /* draw b regardless of the gibbs.py:373 test (direct call) */
  /* Timing diagnostic, not a reference stage: compute the Gram T^T N^-1 [T|r] and eliminate
   * the timing-model columns (the first half of update_hyper_params' first likelihood,
   * gibbs.py:302-304,321) and nothing else of the red-noise block; the chain state is not
   * changed by it.  bench.py times it to report the Gram stage's fp64 utilisation.  Always
   * runs one wave per chain. */
  GST_STAGE_GRAM = 1u << 8
};

/* Model + sampler configuration.  Host pointers; copied by gst_model_set.
 * Replaces: the pta protocol calls (gibbs.py:29,35,154-158,209-210,268-269,297-301,339)
 * and the Gibbs constructor options (gibbs.py:9-51). */
typedef struct gst_model_desc {
  int n;           /* TOAs */
  int m;           /* basis columns = nfourier + ntm (reference order [Fourier | TM]) */
  int nfourier;    /* 2 * components */
  int ntm;         /* timing-model columns */
  int nparams;     /* P <= 4, sorted by name as enterprise does */
  const double* T;         /* n x m, row-major, reference column order */
  const double* residuals; /* n, seconds */
  const double* toaerrs;   /* n, seconds */
  const double* ffreqs;    /* nfourier (= repeat(f, 2)) */
  double tm_weight;        /* timing-model prior variance (1e40, run_sims.py:27-29) */
  /* parameter roles: index into the P-vector or -1 */
  int idx_efac, idx_equad, idx_log10_A, idx_gamma;
  double efac_const;       /* used when idx_efac < 0 */
  const double* pmin;      /* P uniform prior bounds */
  const double* pmax;
  const int* hyper_idx;    /* hyper parameter indices (gibbs.py:64-69) */
  int n_hyper;
  const int* white_idx;    /* white parameter indices (gibbs.py:72-77) */
  int n_white;
  /* outlier model (Gibbs kwargs) */
  int model;               /* enum gst_outlier_model */
  int vary_df;
  int vary_alpha;
  int theta_prior_beta;    /* theta_prior == 'beta' */
  double mprior;           /* m (a-priori outlier probability) */
  double pspin;            /* vvh17 only */
  const double* df_A;      /* 30: n*(nu/2)*log(nu/2) for nu=1..30 (gibbs.py:333-334) */
  const double* df_B;      /* 30: n*gammaln(nu/2) */
  /* General white noise (ABI 3; all zero / NULL = the classic single-backend model above).
   * The reference treats any efac / equad parameter as white and any ecorr parameter as
   * hyper (gibbs.py:64-77), e.g. the notebook's J1643-1224 model (efac, equad and an ECORR
   * basis, gibbs_likelihood.ipynb cell 2) or per-backend selections.  Such models run on
   * the large path (GST_PATH_LARGE; AUTO picks it); nparams may then be up to 16. */
  int nbackend;            /* backends with their own parameters, 1..8 (0 = 1) */
  const int* backend;      /* n: backend of each TOA (NULL: all 0) */
  const int* efac_idx;     /* nbackend: parameter index of each backend's efac, -1 =
                              efac_const (NULL: idx_efac for every backend) */
  const int* equad_idx;    /* nbackend: each backend's log10_equad (NULL: idx_equad) */
  const int* ecorr_idx;    /* nbackend: each backend's log10_ecorr, -1 = none (NULL: none) */
  int n_ecorr;             /* ECORR basis columns: the LAST n_ecorr columns of T, prior
                              variance 10^(2 log10_ecorr) of their backend; m = nfourier +
                              ntm + n_ecorr.  Epochs are normally disjoint (each TOA in at
                              most one ECORR column, enterprise's quantised basis); the large
                              path then eliminates them first, and only then:
                              gst_model_set checks the basis, and a batch with any TOA in two
                              ECORR columns takes the general elimination (ABI 6) */
  const int* ecorr_backend;/* n_ecorr: backend of each ECORR column */
} gst_model_desc;

/* Power-law processes of the Fourier block (additive to ABI 7: callers find
 * gst_model_set_procs by symbol lookup).  Beside the achromatic red noise a multi-frequency
 * analysis carries dispersion-measure variations, a second power law whose basis scales as
 * nu^-2, and often a nu^-4 scattering process (enterprise: s = ef + eq + rn + dm + tm + ec; the
 * reference sampler treats every log10_A / gamma parameter as hyper, gibbs.py:64-69).  The
 * Fourier block of T is then [red | dm | chrom]: process p owns ncol[p] contiguous columns,
 * in this order, with its own log10_A / gamma parameters and its own frequency ladder --
 * ffreqs holds each process's repeat(f, 2) one after the other, and df restarts at each
 * process's first pair (df_1 = f_1 - 0).  The chromatic weights (1400 MHz / nu_t)^chi are
 * part of T: nothing past the prior phi looks at what a Fourier column means.
 *   phi_k = A_p^2 / (12 pi^2) fyr^(gamma_p - 3) f_k^-gamma_p df_k      (column k of process p)
 *   log|phi| = sum_p (ncol_p lc_p - gamma_p sum log f + sum log df) + timing model + ECORR
 * One gst_model_procs is shared by the batch and is part of the structure its datasets must
 * agree in.  Every ncol is even and positive, their sum is nfourier, every index is one of
 * hyper_idx, and idx_log10_A[0] / idx_gamma[0] equal the descriptor's idx_log10_A / idx_gamma.
 * Routing: such models have nparams >= 5, so they run on the persistent kernel's general
 * (GEN) instances -- up to 8 parameters, 60 Fourier + ECORR columns -- or on the large path,
 * where every hyper kernel takes them (lg_hyper_reg, lg_hyper<0/1/2>, lg_hyper_ecr): a model
 * that routes somewhere with one process routes to the same kernel with two or three. */
#define GST_NPROC_MAX 3
typedef struct gst_model_procs {
  int nproc;            /* 1..3 power-law processes in the Fourier block */
  int ncol[3];          /* Fourier columns of each, in basis order; sum = nfourier */
  int idx_log10_A[3];   /* parameter indices; [0] must equal the descriptor's */
  int idx_gamma[3];
} gst_model_procs;

/* Per-chain state, device pointers, chain-major.  x[C*P], b[C*m], z/alpha/pout[C*nmax]
 * (nmax = largest n of the model's datasets; TOAs t >= n of a chain's dataset are never
 * touched), theta/nu[C]; status[C] may be NULL, else flags are OR-ed into it:
 *   status & 1 (bit 0)  a Cholesky failure was seen in the hyper block (lnL = -inf);
 *   status & 2 (bit 1)  the b-draw factorisation failed and b was kept;
 *   status & 4 (bit 2)  dataset index out of range: the persistent path does not run the
 *                       chain, the large path runs it on dataset 0;
 *   status & 8 (bit 3)  large path: the chain's aligned 16-chain group mixes datasets;
 *   status & 16 (bit 4) informational: a b draw ran at the SVD noise floor (Sigma beyond
 *                       fp64 resolution, e.g. vvh17's all-outlier start; see gst_sweep);
 *   status >> 8 (ABI 5) the number of b draws made at the SVD noise floor (each adds 256), so
 *                       that a caller who zeroes status can count them over any window.
 * dataset[C] gives each chain's dataset index into the batch passed to
 * gst_model_set_batch; it may be NULL when there is one dataset. */
typedef struct gst_state {
  double* x;
  double* b;
  double* z;
  double* alpha;
  double* pout;
  double* theta;
  double* nu;
  int* status;
  const int* dataset;
} gst_state;

/* Chain records (Gibbs.sample's chain/bchain/zchain/... arrays, gibbs.py:344-361):
 * device pointers shaped [C][nrec][...] (per-TOA arrays [C][nrec][nmax]); any pointer may
 * be NULL to skip that array.
 * Sweep i of a launch is stored at record (i / record_every) when i % record_every == 0,
 * holding the state at the START of the sweep, as the reference does (gibbs.py:355-361). */
typedef struct gst_records {
  double* x;
  double* b;
  double* z;
  double* alpha;
  double* pout;
  double* theta;
  double* nu;
  int nrec;
} gst_records;

/* Injected-variate tape (parity mode), device pointer [C][nsweeps][stride] fp64 with
 * stride = gst_tape_stride(nmax, m) (n = nmax below).  Per chain-sweep layout:
 *   [0,80)   white MH step s: u_scale, param index, jump normal, accept uniform
 *   [80,120) hyper MH step s: same
 *   [120,120+m)  b draw term Delta = U S^-1/2 xi in reference order
 *   then: beta value; n binomial uniforms; n gamma values; dof-choice uniform. */
typedef struct gst_tape {
  const double* data;
  int stride;
} gst_tape;

/* Posterior sums kept on the device (ABI 7): running sums of the per-TOA state and of b over
 * the sweeps of every gst_sweep call, so that the products a long run ends in -- the outlier
 * probabilities mean(z_t), mean(pout_t), mean(alpha_t) and the signal T mean(b)
 * (gibbs_likelihood.ipynb: zchain.mean(axis=0) > 0.9, poutchain / alphachain means,
 * T @ bchain) -- need no per-TOA chain records.  DEVICE pointers owned by the caller, fp64
 * (count: 64-bit integers), indexed by launch-local chain like gst_state, row stride nmax for
 * the per-TOA sums; the caller zeroes them.  Any pointer may be NULL to skip that sum.
 * While set, every sweep i of every gst_sweep call with sweep0 + i >= from_sweep adds the
 * state at the START of the sweep -- the values a record of that sweep holds -- and
 * increments count[c], on every sweep whatever record_every is; sums carry over from one
 * launch to the next.  Each element is added by one owner in sweep order as a plain
 * sum = sum + v (b_sq: sum + v * v, which may be fused), so sum[c][t] is bitwise the
 * sequential sum of the records.  Entries t >= n of a chain's dataset are never touched;
 * chains that a path does not run (status bit 2 on the persistent path) keep count 0.
 * gst_eval_lnlike and GST_STAGE_GRAM launches never accumulate. */
typedef struct gst_accum {
  double* z_sum;      /* [C][nmax]  sum of z_t over counted sweeps */
  double* pout_sum;   /* [C][nmax]  sum of pout_t */
  double* alpha_sum;  /* [C][nmax]  sum of alpha_t */
  double* b_sum;      /* [C][m]     sum of b_j */
  double* b_sq;       /* [C][m]     sum of b_j^2 */
  long long* count;   /* [C]        counted sweeps */
  long long from_sweep; /* global sweep index (sweep0 + i) of the first counted sweep */
} gst_accum;

/* Per-TOA posterior sums that no mean gives (additive to ABI 7: callers find
 * gst_set_accum_toa by symbol lookup).  The notebook's outlier rule is a median,
 * np.median(poutchain, axis=0) > tau, and median(pout_t) > tau is decided by how many sweeps
 * had pout_t > tau: plane k of pout_gt counts the sweeps with pout_t > thr[k] (strict compare,
 * counts held as doubles like z_sum: exact below 2^53).  resid_sum / resid_sq are the sums of
 * y_t = (r - T b)_t and y_t * y_t of the sweep's start-of-sweep b: r is constant, so
 * E[T b] = r - E[y] and Var[T b] = Var[y] at every TOA -- the waveform band of
 * np.dot(Tmat, bchain[ind, :]).  DEVICE pointers, caller-owned and caller-zeroed, indexed by
 * launch-local chain with row stride nmax; plane k of pout_gt starts at k * nchains * nmax
 * (nchains of the gst_sweep call).  Any pointer may be NULL.  thr must be strictly increasing
 * with every value in (0, 1), nthr in [0, 4].
 * The semantics are gst_accum's and there is no second from_sweep or count: the sums are kept
 * only while gst_set_accum is set, from its from_sweep on, on every counted sweep whatever
 * record_every is, one owner per element as a plain sum = sum + v in sweep order (resid_sq:
 * sum + y * y, which may be fused); entries t >= n are never touched; gst_eval_lnlike and
 * GST_STAGE_GRAM launches never add.  With gst_set_accum unset nothing is written. */
typedef struct gst_accum_toa {
  int nthr;           /* thresholds in use, 0..4 */
  double thr[4];      /* strictly increasing, each in (0, 1) */
  double* pout_gt;    /* [nthr][C][nmax]  sweeps with pout_t > thr[k] */
  double* resid_sum;  /* [C][nmax]  sum of y_t = (r - T b)_t */
  double* resid_sq;   /* [C][nmax]  sum of y_t^2 */
} gst_accum_toa;

/* Block second moment of b (additive to ABI 7: callers find gst_set_accum_block by symbol
 * lookup).  b_sq is only the diagonal of sum_i b b^T; the spread of a process's waveform
 * T_p b_p needs the covariance of b inside the process, whose columns are strongly correlated
 * (sin / cos pairs, steep spectra).  bb keeps the lower triangle of sum_i b b^T over the
 * columns [col0, col0 + ncol) of b (reference column order, as gst_state.b and b_sum hold it):
 * element (i, j), i >= j both relative to col0, of launch-local chain c lies at
 * bb[c * ncol (ncol + 1) / 2 + i (i + 1) / 2 + j].  With b_sum and count it gives the
 * posterior covariance of the block's coefficients, hence mean and variance of B b for any
 * design matrix B (the process basis at the TOAs or on a dense grid).  A DEVICE pointer,
 * caller-owned and caller-zeroed; bb NULL switches the block off.  col0 >= 0,
 * 1 <= ncol <= GST_BLOCK_MAX and col0 + ncol <= m of the model set (setting a block before
 * gst_model_set* is an error; a later gst_model_set* switches it off).
 * The semantics are gst_accum's and there is no second from_sweep or count: the sums are kept
 * only while gst_set_accum is set, from its from_sweep on, on every counted sweep whatever
 * record_every is, one owner per element as a plain sum = sum + b_i * b_j (which may be
 * fused) of the start-of-sweep b in sweep order; gst_eval_lnlike and GST_STAGE_GRAM launches
 * never add; a chain the persistent path does not run (status bit 2) is left untouched.  With
 * gst_set_accum unset nothing is written. */
#define GST_BLOCK_MAX 256
typedef struct gst_accum_block {
  int col0, ncol;     /* columns [col0, col0 + ncol) of b, reference column order */
  double* bb;         /* [C][ncol (ncol + 1) / 2] packed lower triangle, or NULL */
} gst_accum_block;

int gst_version(void);
int gst_tape_stride(int n, int m);
int gst_last_error(char* buf, size_t len);

int gst_ctx_create(int device, void** ctx);
int gst_ctx_destroy(void* ctx);

/* Upload model constants (replaces the pta object, gibbs.py:29-35). */
int gst_model_set(void* ctx, const gst_model_desc* desc);

/* Upload a batch of `ndatasets` models at once (one Gibbs object per dataset x outlier
 * model in run_sims.py:80-113, e.g. the outlier / no_outlier pair of simulate_data.py at
 * several thetas, each under the five outlier models).  The descriptors must agree in
 * m, nfourier, ntm, nparams, parameter roles and hyper/white index sets; n, the data,
 * priors and the outlier-model options may differ.  Chains pick their dataset through
 * gst_state.dataset.  On the large path every aligned group of 16 chains must share one
 * dataset (its Gram and T b kernels stage one dataset's T per group); a chain whose group
 * mixes datasets is flagged with status & 8 (bit 3). */
int gst_model_set_batch(void* ctx, const gst_model_desc* descs, int ndatasets);

/* gst_model_set_batch for a Fourier block of several power-law processes (gst_model_procs
 * above; *procs is copied).  procs NULL or nproc = 1 is gst_model_set_batch itself. */
int gst_model_set_procs(void* ctx, const gst_model_desc* descs,
                        const gst_model_procs* procs, int ndatasets);

/* Number of datasets, largest n (row stride of per-TOA state/records) and tape stride. */
int gst_model_info(void* ctx, int* ndatasets, int* nmax, int* tape_stride);

/* Run `nsweeps` Gibbs sweeps for chains [0, nchains) (Gibbs.sample's loop body,
 * gibbs.py:354-380).  `tape` NULL or tape->data NULL -> on-device Philox4x32-10 variates
 * keyed by (seed, chain0 + c), counters by (sweep0 + i, stage, index): results do not
 * depend on how chains are sharded over launches or GPUs.
 * b draw (gibbs.py:145-182): exact Cholesky draw b = Sigma^-1 d + L^-T eta, except where
 * Sigma is beyond fp64 resolution -- its smallest LDL^T pivot (timing-model-first order, real
 * columns) below 2^-52 of its largest, p_max.  There the reference's sl.svd returns the small
 * eigenvalues at LAPACK's rounding floor (~0.3-2 x 2^-52 x s_max) and its draw is in effect
 * that of Sigma + f I; this path draws from Sigma + f I with f = 0.75 x 2^-52 p_max (flags
 * status & 16 and counts the draw in status >> 8), which reproduces the reference's escape
 * from vvh17's all-outlier start.  ABI 4 gated at 1e-14.
 * GST_DEBUG_EXACT_BDRAW turns the floor off. */
int gst_sweep(void* ctx, const gst_state* state, const gst_records* rec,
              const gst_tape* tape, int nchains, int nsweeps, long long sweep0,
              int record_every, unsigned stage_mask, unsigned long long seed,
              long long chain0, void* stream);

/* Evaluate the two likelihoods for K (state, x) pairs without sampling:
 *   out_white[k] = get_lnlikelihood_white(x_k)  (gibbs.py:262-284)
 *   out_hyper[k] = get_lnlikelihood(x_k)        (gibbs.py:288-329)
 * using chain k's b, z, alpha from `state` (x from state->x). */
int gst_eval_lnlike(void* ctx, const gst_state* state, int nchains, double* out_white,
                    double* out_hyper, void* stream);

/* Posterior sums (gst_accum above): *acc is copied; NULL switches accumulation off.  Takes
 * effect from the next gst_sweep call, in stream order with it. */
int gst_set_accum(void* ctx, const gst_accum* acc);

/* Exceedance counts and residual sums (gst_accum_toa above): *a is copied; NULL switches them
 * off.  Kept only while gst_set_accum is set; takes effect from the next gst_sweep call. */
int gst_set_accum_toa(void* ctx, const gst_accum_toa* a);

/* Block second moment of b (gst_accum_block above): *blk is copied; NULL switches it off.
 * Kept only while gst_set_accum is set; takes effect from the next gst_sweep call, in stream
 * order with it.  Errors (< 0, gst_last_error) leave the block as it was. */
int gst_set_accum_block(void* ctx, const gst_accum_block* blk);

int gst_sync(void* ctx, void* stream);

/* Execution path.  The persistent path keeps a whole chain in one wavefront for all of a
 * launch's sweeps (n <= 512 and up to 30 red-noise components with <= 16 timing-model
 * columns, 26 with <= 24, n <= 1024 for the 30-component / 16-column shape; smaller models
 * run padded with unit-prior dummy columns; the general white-noise model -- per-backend
 * efac / equad, ECORR columns, up to 8 parameters -- with <= 16 timing-model columns, up to
 * 60 Fourier + ECORR columns and n <= 512); the
 * large path runs
 * each sweep as a pipeline of kernels (fp64-MFMA Gram shared by all chains, blocked
 * timing-model elimination, LDS-resident red-noise MH, MFMA T b, per-TOA passes) for
 * large n and m (BASELINE config 5).  AUTO (default) picks persistent when it fits.
 * gst_set_path must precede gst_model_set. */
enum gst_path { GST_PATH_AUTO = 0, GST_PATH_PERSISTENT = 1, GST_PATH_LARGE = 2 };
int gst_set_path(void* ctx, int path);
int gst_get_path(void* ctx, int* path);

/* Waves per chain on the persistent path.  A sampling launch with at most one chain per two
 * SIMDs (C <= 2 x CUs, e.g. BASELINE config 3's 512 chains) runs each chain on two waves
 * that split the red-noise MH block's likelihood evaluations (AUTO, the default); the
 * chain's draws are bitwise those of the one-wave kernel.  GST_WAVES_ONE / GST_WAVES_TWO
 * force either kernel for every sampling launch (tape-mode and gst_eval_lnlike launches
 * always run one wave per chain).  Since round 6 the general white-noise model (per-backend
 * white noise, ECORR columns) has the two-wave kernel too. */
enum gst_waves { GST_WAVES_AUTO = 0, GST_WAVES_ONE = 1, GST_WAVES_TWO = 2 };
int gst_set_waves(void* ctx, int waves);

/* Diagnostics of the persistent path.  GST_DEBUG_POISON: at the start of every sweep each
 * chain overwrites all of its LDS and its parked timing-model factor scratch with a NaN
 * pattern; since a chain carries no state between sweeps beyond its state arrays, a launch
 * with this flag must give bitwise the same chains as one without (a read of any stale word
 * would surface as NaN / different draws).  Costs time; never set in production. */
/* Large path: GST_DEBUG_LARGE_GRAM forces the 64x64 super-tile Gram (lg_gram) where the
 * one-wave-per-chain Gram (lg_gram_small) would run; the two give bitwise the same G.  It also
 * turns off the structured ECORR Gram (lg_gram_ec, round 6: disjoint ECORR epochs eliminated
 * first -- only G_xx, the epochs' diagonal and their couplings, by MFMA), whose G blocks agree
 * with the dense Gram's to rounding (summation order).
 * GST_DEBUG_LARGE_HYPER forces the LDS-resident hyper kernel (lg_hyper) where the register-
 * resident one (lg_hyper_reg) would run: same variates and decisions, likelihoods within
 * rounding; and the blocked global-memory elimination (lg_hyper<1>) where the ECORR-epochs-
 * first one (lg_hyper<2>) would run: likelihoods within rounding, b draws of the same law.
 * Test switches (the defaults are the faster kernels). */
/* GST_DEBUG_EXACT_BDRAW: every b draw is the exact draw from Sigma, also beyond fp64
 * resolution (no SVD noise floor, see gst_sweep). */
/* The floor gate's pivot order: the timing-model-first LDL^T (real columns) on the
 * persistent path and the large path's classes 0 / 1 and register kernels; the large path's
 * class 2 (ECORR epochs eliminated first, lg_hyper<2>) gates on the pivots of its own order
 * [ECORR | TM | Fourier].  Pivot ratios depend on the order, so near the 2^-52 gate the two
 * orders can decide a draw differently (both draw exactly from Sigma or Sigma + f I). */
/* GST_DEBUG_MFMA_GRAM (ABI 5): the persistent kernel computes every Gram on the MFMA path,
 * never the low-rank one (datasets of <= 8 noise classes, at most 32 flagged TOAs: the
 * per-class Grams plus one rank-1 update per flagged TOA); the two agree
 * to rounding. */
/* GST_DEBUG_EPOCHS_LDS (ABI 6): large-path chains whose ECORR epochs are eliminated first run
 * the 256-thread LDS kernel lg_hyper<2> instead of the one-wave register kernel
 * lg_hyper_ecr (timing model <= 16 columns, Fourier block <= 46 columns); same elimination
 * order, likelihoods and b draws equal to rounding.  A/B and test switch. */
enum gst_debug {
  GST_DEBUG_POISON = 1,
  GST_DEBUG_LARGE_GRAM = 2,
  GST_DEBUG_LARGE_HYPER = 4,
  GST_DEBUG_EXACT_BDRAW = 8,
  GST_DEBUG_MFMA_GRAM = 16,
  GST_DEBUG_EPOCHS_LDS = 32
};
int gst_set_debug(void* ctx, int flags);

/* Per-kernel timing of the large path (HIP events around every launch of the next
 * gst_sweep / gst_eval_lnlike calls while enabled).  gst_kernel_times fills ms[k] (summed
 * milliseconds) and launches[k] for kernel kinds k < nkinds (enum gst_kernel_kind). */
enum gst_kernel_kind {
  GST_K_RECORD = 0, GST_K_WHITE = 1, GST_K_GRAM = 2, GST_K_TMELIM = 3,
  GST_K_HYPER = 4, GST_K_BTM = 5, GST_K_TB = 6, GST_K_TOA = 7,
  GST_K_ACCUM = 8, /* lg_accum: the posterior sums (ABI 7) */
  GST_K_COUNT = 9
};
int gst_set_timing(void* ctx, int on);
int gst_kernel_times(void* ctx, double* ms, int* launches, int nkinds);

/* Diagnostic builds (-DGST_STAMPS) only: per-chain per-stage s_memtime cycle sums (slots
 * 0-15 and 19-23) and event counts (16: red-noise likelihoods, 17: two-wave rounds, 18:
 * accepted red-noise proposals) are accumulated into dev_buf[C][24]; returns an error in
 * production builds. */
int gst_debug_stamps(void* ctx, unsigned long long* dev_buf);

/* Kernel-level timing of the last gst_sweep on its stream (hipEvents), milliseconds. */
int gst_last_sweep_ms(void* ctx, double* ms);

/* Grams T^T N^-1 [T|r] (gibbs.py:302-304) computed since the last reset, by path (ABI 6):
 *   counts[0]  persistent kernel, low-rank: the dataset's per-class Grams plus one rank-1
 *              update per flagged TOA, on the VALU (<= 8 noise classes, <= 32 flagged TOAs,
 *              every flagged alpha <= 2^20);
 *   counts[1]  persistent kernel, the n-TOA fp64 MFMA Gram;
 *   counts[2]  large path: the launch's chain count per Gram stage of a sweep, whichever
 *              kernels ran it (lg_gram, lg_gram_small, lg_gram_ec), chains that a kernel
 *              skipped included.  The b draw's floor pass re-eliminates the same Gram: it is
 *              not computed, and not counted, again.
 * counts[0] and counts[1]: one count per chain per Gram computed.  Synchronises the device.
 * reset != 0 zeroes the counters after reading them. */
int gst_gram_counts(void* ctx, long long* counts, int reset);

/* Test hook (ABI 6): n draws of the kernel's own samplers into the DEVICE array out, Philox
 * keyed by (seed, call), for distribution tests of the samplers themselves:
 *   kind 0  gamma_mt(a): Marsaglia-Tsang Gamma(a, 1), a < 1 by the a + 1 boost (the theta
 *           stage's Gammas);
 *   kind 1  Beta(a, b) = Ga / (Ga + Gb) from two gamma_mt draws (update_theta, gibbs.py:196);
 *   kind 2  gamma_mt_slots<4>, the alpha stage's interleaved Gamma(a) draws (gibbs.py:239);
 *           n a multiple of 256.
 * n <= 2^31.  Needs no context; runs on the current device. */
int gst_debug_variates(int kind, double a, double b, long long n, unsigned long long seed,
                       unsigned call, double* out, void* stream);

/* Batched synthetic pulsars on the current device: the simulate_data.py:10-39 recipe for
 * `ndatasets` datasets in one launch (one workgroup per dataset), Philox variates keyed by
 * (seed, dataset0 + d).  Replaces simulate_data() + the par/tim round trip through
 * libstempo (simulate_data.py:12-37, run_sims.py:41-51).  All pointers are DEVICE pointers;
 * per-dataset outputs are [ndatasets][n].
 *   error bars   toaerrs[n] if given, else 10^(-7 + 0.2 N(0,1)) s         (:15)
 *   red noise    red[n] if given (e.g. red.txt), else F (sqrt(phi) N(0,1)) with the power
 *                law phi_k = A^2/(12 pi^2) fyr^(gamma-3) f_k^-gamma df_k        (:21)
 *   outliers     z_t ~ Bernoulli(theta)                                   (:24)
 *   residuals    red + ((1 - z) err + z sigma_out) xi, xi ~ N(0,1) or Student-t(dof) for
 *                dof > 0, then the timing model refit out: r - U (U^T r)  (:26)
 *   clean twin   (residuals_clean may be NULL) the no_outlier dataset (:35-37): outlier
 *                TOAs deleted (their entries set to 0) and the timing model refit on the
 *                kept TOAs (needs ntm <= 64).
 * Limits: nfourier <= 512, ntm <= 512. */
typedef struct gst_sim_desc {
  int n, nfourier, ntm, ndatasets;
  const double* F;        /* [n][nfourier] Fourier basis (may be NULL when red is given) */
  const double* log_f;    /* [nfourier] log f_k (Hz) */
  const double* log_df;   /* [nfourier] log df_k */
  double log_fyr;         /* log(1 / yr in Hz) */
  const double* U;        /* [n][ntm] orthonormal timing-model basis (SVD of M) */
  const double* red;      /* [n] fixed red-noise realisation (s) or NULL */
  const double* toaerrs;  /* [n] fixed error bars (s) or NULL */
  const double* theta;    /* [ndatasets] outlier fraction */
  const double* sigma_out;/* [ndatasets] outlier scatter (s) */
  const double* log10_A;  /* [ndatasets] red-noise amplitude (power-law draw) */
  const double* gamma;    /* [ndatasets] red-noise spectral index */
  const double* dof;      /* [ndatasets] Student-t dof of the white noise, <= 0: Gaussian */
  unsigned long long seed;
  long long dataset0;     /* global index of dataset 0 (shards give the same datasets) */
  double* residuals;      /* out [ndatasets][n] */
  double* toaerrs_out;    /* out [ndatasets][n] */
  double* z;              /* out [ndatasets][n] injected outlier flags (0 / 1) */
  double* residuals_clean;/* out [ndatasets][n] or NULL */
} gst_sim_desc;
int gst_simulate(const gst_sim_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* GST_H_ */
