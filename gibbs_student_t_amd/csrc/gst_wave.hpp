// Lane, DPP and LDS primitives of the gfx950 kernels: cross-lane moves and reductions, per-lane
// global rows, the LDS hand-off fence, register-array selects, the issue-priority turns of the
// two-chains-per-SIMD build, the reciprocal / log-product helpers and the diagnostic stamps.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace gst {

typedef double v4d __attribute__((ext_vector_type(4)));
// a global-memory double: loads through it are global_load (a generic pointer read out of
// DevModel compiles to flat_load, which also waits on the LDS counter)
typedef __attribute__((address_space(1))) double GDouble;

// diagnostic builds: slots 0-15, 19-27 cycle sums (tools/stage_profile.py), 16-18 event counts
// (26 / 27, one-wave hyper loop: end of chol_stats -> MH verdict, verdict -> next lnl_hyper)
constexpr int GST_NSTAMP = 28;
#ifdef GST_STAMPS
#define GST_STAMP_DECL \
  unsigned long long st_acc[GST_NSTAMP] = {0}, st_t0 = 0, st_s0 = 0;
#define GST_SUB_BEGIN st_s0 = __builtin_amdgcn_s_memtime();
#define GST_COUNT(i) st_acc[i] += 1;
#define GST_SUB_END(i)                                            \
  {                                                               \
    const unsigned long long t1_ = __builtin_amdgcn_s_memtime(); \
    st_acc[i] += t1_ - st_s0;                                     \
    st_s0 = t1_;                                                  \
  }
#define GST_STAMP_START st_t0 = __builtin_amdgcn_s_memtime();
#define GST_STAMP(i)                                              \
  {                                                               \
    const unsigned long long t1_ = __builtin_amdgcn_s_memtime(); \
    st_acc[i] += t1_ - st_t0;                                     \
    st_t0 = t1_;                                                  \
  }
#define GST_STAMP_FLUSH                                             \
  if (md.stamps && lane == 0)                                       \
    for (int i_ = 0; i_ < GST_NSTAMP; ++i_) md.stamps[(size_t)c * GST_NSTAMP + i_] += st_acc[i_];
#else
#define GST_SUB_BEGIN
#define GST_COUNT(i)
#define GST_SUB_END(i)
#define GST_STAMP_DECL
#define GST_STAMP_START
#define GST_STAMP(i)
#define GST_STAMP_FLUSH
#endif

__device__ __forceinline__ double rdlane(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Two chains share each SIMD in the OCC = 2 build, and the SIMD's arbiter issues the older
// wave first: the chain that arrived second ran ~27% slower per sweep than its partner and
// every launch ended with it (tools/chain_pairs.py).  Priority turns fix that:
//  * progress rule (the host passes st.prog): each chain counts its sweep into a
//    launch-wide counter (one atomic per chain-sweep, its return value consumed a sweep
//    later); a chain that has done fewer sweeps than the launch average holds the higher
//    issue priority;
//  * the first sweep of a launch, and launches without st.prog: time slices of 2^15 clocks
//    by wave-slot parity (slot-parity-1 waves hold the higher priority kPrioShare / 8
//    of the time).
// Checked at the sweep, MH-step and stage boundaries (the clock read waits only there).
constexpr unsigned kPrioShare = 5;  // 4: 8.50 M, 5: 8.65 M, 6: 8.38 M chain-sweeps/s (age favours the older wave)
__device__ __forceinline__ unsigned wave_slot_parity() {
  return __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4) & 1u;  // HW_REG_HW_ID.WAVE_ID
}
struct Fair {
  unsigned slot;            // wave-slot parity
  int behind;               // progress rule: 1 = behind the launch average, -1 = no rule
};
template <int OCC>
__device__ __forceinline__ void fair_prio(const Fair& f) {
  if constexpr (OCC == 2) {
    bool high;
    if (f.behind >= 0) {
      high = f.behind != 0;
    } else {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      high = ((((unsigned)(t >> 15)) & 7u) < kPrioShare) == (f.slot != 0u);
    }
    if (high)
      __builtin_amdgcn_s_setprio(1);
    else
      __builtin_amdgcn_s_setprio(0);
  }
}

// Per-lane fp64 rows in global memory addressed as (wave-uniform buffer resource, this
// lane's byte offset, a constant byte offset in an SGPR): every access needs only the one
// lane-offset VGPR, where 64-bit per-lane pointers (base + lane + 4 KB multiples) would each
// hold two VGPRs across the sweep loop -- and get spilled, then reloaded one after another.
struct LaneRows {
  __amdgpu_buffer_rsrc_t rs;
  int vo;
};
__device__ __forceinline__ LaneRows lane_rows(const double* base, int doubles, int lane) {
  return {__builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(base), 0, doubles * 8, 0x00020000),
          lane * 8};
}
__device__ __forceinline__ double lr_load(const LaneRows& b, int byte_off) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(b.rs, b.vo, byte_off, 0));
}
__device__ __forceinline__ void lr_store(const LaneRows& b, int byte_off, double v) {
  typedef unsigned int u2 __attribute__((ext_vector_type(2)));
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), b.rs, b.vo, byte_off, 0);
}

// Cross-lane moves within a 16-lane row by DPP (VALU speed, no LDS traffic).
template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_ROR4 = 0x124, DPP_ROR8 = 0x128;

// Sum over the wave: quad butterflies + row rotations give every lane its 16-lane row sum,
// then the four row sums are combined in a fixed order from lanes 0/16/32/48, so the result
// is bitwise identical (uniform) in every lane.
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp<DPP_XOR1>(v);
  v += dpp<DPP_XOR2>(v);
  v += dpp<DPP_ROR4>(v);
  v += dpp<DPP_ROR8>(v);
  return (rdlane(v, 0) + rdlane(v, 16)) + (rdlane(v, 32) + rdlane(v, 48));
}

// The same for an int (exact in any order): the DPP adds, then the four row sums.
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ int wave_sum_i(int v) {
  v += dpp_i<DPP_XOR1>(v);
  v += dpp_i<DPP_XOR2>(v);
  v += dpp_i<DPP_ROR4>(v);
  v += dpp_i<DPP_ROR8>(v);
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
         (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, dpp<DPP_XOR1>(v));
  v = fmax(v, dpp<DPP_XOR2>(v));
  v = fmax(v, dpp<DPP_ROR4>(v));
  v = fmax(v, dpp<DPP_ROR8>(v));
  return fmax(fmax(rdlane(v, 0), rdlane(v, 16)), fmax(rdlane(v, 32), rdlane(v, 48)));
}

// Sum over p (lane bits 3..5) of the lanes with q == qq (lane = 8p + q), uniform result.
__device__ __forceinline__ double col_sum(double v, int qq) {
  v += dpp<DPP_ROR8>(v);  // (l + 8) mod 16 == l ^ 8
  return (rdlane(v, qq) + rdlane(v, qq + 16)) + (rdlane(v, qq + 32) + rdlane(v, qq + 48));
}

// 1/sqrt(a): hardware estimate + two Newton steps (full double accuracy to ~1 ulp).
__device__ __forceinline__ double rsqrt_nr(double a) {
  double y = __builtin_amdgcn_rsq(a);
  y = y * fma(-0.5 * a * y, y, 1.5);
  y = y * fma(-0.5 * a * y, y, 1.5);
  return y;
}

// Hand-off point between lanes of one wave through LDS.  LDS instructions of a wave execute
// in issue order, so no hardware wait is needed; what must not happen is the COMPILER moving
// a load that reads another lane's data above the store that wrote it (from one lane's
// point of view the two addresses differ, so a single-thread fence does not forbid it).  A
// wavefront-scope fence is the construct that orders memory accesses across the lanes of
// the wave; it emits no instruction.
__device__ __forceinline__ void lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// x[i] as a select chain over register values.  The empty asm makes each element an opaque
// register value: without it InstCombine turns the select of array loads into a load from a
// selected address, which keeps the whole parameter array in scratch memory (reloaded in
// every MH step of the 2-chains-per-SIMD build).
__device__ __forceinline__ double pget(const double (&x)[4], int i) {
  double a = x[0], b = x[1], c = x[2], d = x[3];
  asm("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
  return i == 0 ? a : (i == 1 ? b : (i == 2 ? c : d));
}
// the general-white-noise instances (GEN): up to 8 parameters
__device__ __forceinline__ double pget(const double (&x)[8], int i) {
  double v[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    v[k] = x[k];
    asm("" : "+v"(v[k]));
  }
  double r = v[7];
#pragma unroll
  for (int k = 6; k >= 0; --k) r = (i == k) ? v[k] : r;
  return r;
}

// x[i] over a PER-LANE index (a VGPR), as one v_cmp + v_cndmask pair per candidate.  The
// candidates are compared against opaque per-lane constants: over literal ones the compare
// chain is recognised as a switch on i, and a switch on a divergent value is lowered to a
// cascade of exec-mask regions (a saveexec and a branch per case, ~25 instructions a read in
// front of every factorisation of the hyper MH).
template <int N>
__device__ __forceinline__ double pget_lane(const double (&x)[N], int i) {
  double v[N];
  int k[N - 1];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    v[j] = x[j];
    asm("" : "+v"(v[j]));
  }
#pragma unroll
  for (int j = 0; j < N - 1; ++j) {
    k[j] = j;
    asm("" : "+v"(k[j]));
  }
  double r = v[N - 1];
#pragma unroll
  for (int j = N - 2; j >= 0; --j) r = (i == k[j]) ? v[j] : r;
  return r;
}

__device__ __forceinline__ int iget4(const int* a, int i) {   // a[i], i < 4
  return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : a[3]));
}
template <int N>
__device__ __forceinline__ int iget(const int* a, int i) {   // a[i], i < N (4 or 8)
  if constexpr (N == 4) {
    return iget4(a, i);
  } else {
    int r = a[N - 1];
#pragma unroll
    for (int k = N - 2; k >= 0; --k) r = (i == k) ? a[k] : r;
    return r;
  }
}

// 1/a: hardware estimate (~2^-24) + one Newton step (~2e-15 relative, measured on
// MI355X by tools/ubench/rcp_acc.hip); on every column step's critical path.
__device__ __forceinline__ double rcp_nr1(double a) {
  const double y = __builtin_amdgcn_rcp(a);
  return fma(y, fma(-a, y, 1.0), y);
}

constexpr double LN2 = 0.693147180559945309417;
// log(mant 2^expo) of a product kept as mantissa product + exponent sum
__device__ __forceinline__ double log_mant_exp(double mant, int expo) {
  return log(mant) + (double)expo * LN2;
}

// Per-thread sum of logs as a running product: mantissa product + exponent sum (v_frexp),
// one log per thread at the end instead of one per TOA (the per-TOA log dominated the white
// block's 21 likelihood rescans; both paths).  The mantissa product is renormalised every 128 factors
// (each factor >= 1/2, so it stays far above the fp64 underflow threshold).
struct LogProd {
  double mp = 1.0;
  int ex = 0, k = 0;
  __device__ __forceinline__ void mul(double v) {
    int e;
    mp *= frexp(v, &e);
    ex += e;
    if ((++k & 127) == 0) {
      mp = frexp(mp, &e);
      ex += e;
    }
  }
  __device__ __forceinline__ double log_sum() const {
    return log_mant_exp(mp, ex);
  }
};

// a / b for positive normal operands without the IEEE division sequence (v_div_scale /
// v_div_fmas / v_div_fixup): reciprocal estimate, one Newton step, then one residual
// correction of the quotient (within 1 ulp of the rounded quotient).
__device__ __forceinline__ double div_pos(double a, double b) {
  const double y = rcp_nr1(b);
  const double q0 = a * y;
  return fma(fma(-b, q0, a), y, q0);
}

// A lane permute of a double (ds_bpermute: any source lane per lane, through the LDS crossbar).
__device__ __forceinline__ double bperm(double v, int src_lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_ds_bpermute(4 * src_lane, (int)(b & 0xffffffffll));
  const int hi = __builtin_amdgcn_ds_bpermute(4 * src_lane, (int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

}  // namespace gst
