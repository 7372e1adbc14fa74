// Shared helpers for the gfx950 N-body backend: error plumbing, (dtype, dim) dispatch and the pair
// kernel math.  Device code here is written for CDNA4 only (wave64, no portability layer).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/nbody_hip.h"
#include "device_buffers.hpp"

namespace nbody {

// ---- error plumbing -----------------------------------------------------------------------------
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define NB_HIP(call)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) return ::nbody::hip_fail(e_, #call, __FILE__, __LINE__);     \
  } while (0)

#define NB_ARG(cond, ...)                \
  do {                                   \
    if (!(cond)) {                       \
      ::nbody::set_error(__VA_ARGS__);   \
      return NBODY_ERR_ARG;              \
    }                                    \
  } while (0)

// ---- devices --------------------------------------------------------------------------------------
// One host thread may drive several GPUs (the CLI's --gpus N, ncclCommInitAll): every entry point runs on the device its
// handle or stream belongs to and puts the caller's current device back when it returns.
struct device_guard {
  int prev     = -1;
  bool changed = false;
  explicit device_guard(int dev) {
    if (dev >= 0 && hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
  }
  ~device_guard() {
    if (changed) (void)hipSetDevice(prev);
  }
  device_guard(const device_guard&)            = delete;
  device_guard& operator=(const device_guard&) = delete;
};

inline int current_device() {
  int d = -1;
  return hipGetDevice(&d) == hipSuccess ? d : -1;
}

// 0 unless `st` is recording (nbody_graph_begin): then the capture's id
inline unsigned long long capture_id(hipStream_t st) {
  if (st == nullptr) return 0;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long id     = 0;
  if (hipStreamGetCaptureInfo(st, &cs, &id) != hipSuccess || cs != hipStreamCaptureStatusActive) return 0;
  return id ? id : ~0ull;
}

// context.hip: captures begun with nbody_graph_begin on the calling thread and not yet ended (they are thread-local captures): an
// entry that allocates and has no stream to ask refuses while this is not 0
int captures_on_this_thread();

// device a stream was created on; the NULL stream belongs to whatever device is current
inline int stream_device(hipStream_t st) {
  if (st == nullptr) return current_device();
  hipDevice_t d = -1;
  return hipStreamGetDevice(st, &d) == hipSuccess ? int(d) : current_device();
}

// a handle (context, tree, communicator) is used on the device it was created on: its buffers live there
inline int check_same_device(int handle_device, hipStream_t st, const char* what) {
  const int sd = stream_device(st);
  NB_ARG(handle_device == sd, "%s was created on device %d but the call's stream belongs to device %d", what, handle_device, sd);
  return NBODY_OK;
}

// ---- handles: create and destroy -------------------------------------------------------------------------------------------------
// Every nbody_*_create: create_check_args, the call's own argument checks if it has any (kNN's k and method), create_check_device,
// device_guard, `new`, the allocations through the handle's device_buffers, create_finish.  Every nbody_*_destroy: NULL check,
// device_guard, what is not memory, `delete` — the owner frees.
// The arguments every handle takes, in the header's order.  n_text: the whole message for n outside [n_min, n_max]; it may print n
// with one %u.
template <typename H>
inline int create_check_args(H** out, int dtype, int dim, uint32_t n, uint32_t n_min, uint32_t n_max, const char* n_text) {
  NB_ARG(out != nullptr, "out is NULL");
  *out = nullptr;
  NB_ARG(dtype == NBODY_F32 || dtype == NBODY_F64, "bad dtype %d", dtype);
  NB_ARG(dim == 2 || dim == 3, "bad dim %d", dim);
  NB_ARG(n >= n_min && n <= n_max, n_text, n);
  return NBODY_OK;
}

// After all argument checks: that no capture is open on this thread, then the device; resolves *device (-1: the current one, unless
// !default_to_current: nbody_create takes no -1).
// refuse_in_capture is false for nbody_create, nbody_bvh_create_on and nbody_octree_create_on: they allocate like the others but
// have never refused between nbody_graph_begin and nbody_graph_end, and that is kept as it is here, not judged right.
inline int create_check_device(int* device, const char* api, bool refuse_in_capture, bool default_to_current = true) {
  if (refuse_in_capture && captures_on_this_thread() != 0) {
    set_error("nbody_%s_create allocates: it cannot be called between nbody_graph_begin and nbody_graph_end", api);
    return NBODY_ERR_STATE;
  }
  int ndev = 0;
  NB_HIP(hipGetDeviceCount(&ndev));
  if (*device < 0 && default_to_current) *device = current_device();
  NB_ARG(*device >= 0 && *device < ndev, "device %d out of range (%d HIP devices visible)", *device, ndev);
  return NBODY_OK;
}

// The end of a create call.  e: the handle's device_buffers::error(), or the error of another runtime call, named by `what`.  On an
// error the half-made handle is destroyed and *out stays NULL.
template <typename H>
inline int create_finish(H** out, H* h, void (*destroy)(H*), hipError_t e, const char* what, const char* file = __builtin_FILE(),
                         int line = __builtin_LINE()) {
  if (e != hipSuccess) {
    const int r = hip_fail(e, what, file, line);
    destroy(h);
    return r;
  }
  *out = h;
  return NBODY_OK;
}

// Experiment switches (tools/README.md) exist only in the build made with -DNBODY_EXPERIMENTS (`make experiments`:
// libnbody_hip_exp.so); the shipped library never reads the environment — the launch shape is what nbody_all_pairs_describe
// states and what the ABI setters select.
#ifdef NBODY_EXPERIMENTS
inline const char* experiment_env(const char* name) { return getenv(name); }
#else
constexpr const char* experiment_env(const char*) { return nullptr; }
#endif

inline int check_tuning(int split, int tpt, int path);

// all_arrays = false: a call that reads only (m, x) — v, a and ao may be NULL
inline int check_state(const nbody_state* s, bool all_arrays = true) {
  NB_ARG(s != nullptr, "nbody_state is NULL");
  NB_ARG(s->dtype == NBODY_F32 || s->dtype == NBODY_F64, "bad dtype %d", s->dtype);
  NB_ARG(s->dim == 2 || s->dim == 3, "bad dim %d (must be 2 or 3)", s->dim);
  if (all_arrays) NB_ARG(s->m && s->x && s->v && s->a && s->ao, "nbody_state has a NULL array pointer");
  NB_ARG(s->m && s->x, "nbody_state has a NULL array pointer (m, x)");
  NB_ARG(uint64_t(s->first) + uint64_t(s->count) <= uint64_t(s->sz), "shard [%u, %u+%u) exceeds sz=%u", s->first, s->first,
         s->count, s->sz);
  // tuning is 0 or a value NBODY_TUNING() made: a hand-built state that was not zero-initialised is refused, not obeyed
  if (s->tuning != 0) {
    NB_ARG((s->tuning & ~0x1ffu) == 0 && (s->tuning & 0x100u) != 0, "nbody_state.tuning = 0x%x is not 0 or an NBODY_TUNING(...) value",
           s->tuning);
    if (int r = check_tuning(int(s->tuning & 15u), int((s->tuning >> 4) & 3u), int((s->tuning >> 6) & 3u))) return r;
  }
  return NBODY_OK;
}

// Runtime (dtype, dim) -> compile-time <T, D>.  F is a generic lambda taking (T tag, integral_constant D).
template <typename T, int D>
struct tag {
  using type = T;
  static constexpr int dim = D;
};

template <typename F>
inline int dispatch(int dtype, int dim, F&& f) {
  if (dtype == NBODY_F32 && dim == 2) return f(tag<float, 2>{});
  if (dtype == NBODY_F32 && dim == 3) return f(tag<float, 3>{});
  if (dtype == NBODY_F64 && dim == 2) return f(tag<double, 2>{});
  if (dtype == NBODY_F64 && dim == 3) return f(tag<double, 3>{});
  set_error("unsupported (dtype=%d, dim=%d)", dtype, dim);
  return NBODY_ERR_ARG;
}

// ---- pair math -----------------------------------------------------------------------------------
// The reference pair term (src/all_pairs.h:23, src/bvh.h:297,308; dist3 at src/vec.h:249-252) is
//     m_j * (x_j - x_i) / (pow(r2, 3/2) + eps)
// i.e. one pow, one add and D divisions per pair.  On gfx950 FP64 transcendentals run at quarter rate and do not overlap
// the FMA pipe (profiles/r01_valu_rates_microbench.txt), and an IEEE divide is a ~10-instruction sequence, so the kernels
// evaluate the weight   w = m_j / (r2*sqrt(r2) + eps)   once per pair and then D FMAs.  What is shipped (f64):
//   * r2 >= 4        weight_far<false>: w = (m y^3)(1 + e(3/2 + 15/8 e)), y = v_rsq_f64(r2), e = 1 - r2 y^2 — no reciprocal,
//                    and the `+ eps` dropped: eps/r^3 <= 2^-55 there, an eighth of an ulp.   7 ops + 1 transcendental
//   * 2^-16 <= r2 < 4  weight_far<true>: the same with the first-order term of the eps expansion, - eps y^3.   8 ops + 1
//   * r2 < 2^-16     weight<3>(): the guarded reciprocal form (the self pair, coincident and very close bodies), <= 2 ulp.
// Which form a pair takes depends on ITS OWN r2 alone (never on the other lanes of the wave), so a target's sum is bitwise
// independent of the shard window.  Every form is within 2.5 ulp of the exact term with no bias
// (tests/test_gpu_all_pairs.py::test_pair_term_accuracy, test_pair_term_two_body_ulps, test_pair_math_adversarial_separations).
// K1 (both twins, both source paths) takes the two weight_far forms with the source's mass folded into the polynomial's constants
// — weight_far_folded below: 6 and 7 ops + 1 — K2, the energies, Hermite and the tree walks weight_far as it stands.
// weight() with NBODY_PAIR_POLISH = 2 is what round 1 shipped everywhere and what the compiler-scheduled tree walks still use.
//
// r2 must be > 0: callers fold TINY into the first FMA of r2 (r2 = fma(dx,dx,TINY)), which makes the
// self term and coincident bodies evaluate to exactly 0 * (finite) = 0 — the value the reference
// gets from `(m*0)/eps` (self term skipped by `if (i == j) continue`) — with no branch
// and no select (a v_cmp + 2 v_cndmask select costs ~5 FMA slots on this chip).
template <typename T>
struct pair_math;

// NBODY_PAIR_POLISH: order of the polish applied to the two 2^-24 FP64 seeds of weight() as the tree walks (K9, octree)
// use it.  K1 uses weight() only for pairs closer than 2^-8 (see weight_far below) and takes the third-order form there.
//   2 (default): Newton steps  s = h + h*e/2,  w = zm + zm*e2        17 full-rate ops + 2 transcendentals per pair.
//      Per-term error bound: +3/8*e^2 (e <= 2^-23.2) - e2^2 (e2 <= 2^-24.4)  =>  within [-2e-15, +4.1e-15] relative.
//   3: third-order steps (+2 FMA): <= 2 ulp per term.
#ifndef NBODY_PAIR_POLISH
  #define NBODY_PAIR_POLISH 2
#endif

template <>
struct pair_math<double> {
  static constexpr double tiny = 1e-300;
  // returns mj / (r2 * sqrt(r2) + DBL_EPSILON); POLISH = order of the steps on the two seeds
  template <int POLISH = NBODY_PAIR_POLISH>
  __device__ static __forceinline__ double weight(double r2, double mj) {
    double y0 = __builtin_amdgcn_rsq(r2);     // ~2^-24 relative
    double h  = r2 * y0;                      // ~sqrt(r2)
    double e  = __builtin_fma(-h, y0, 1.0);   // 1 - r2*y0^2
    double s;
    if constexpr (POLISH >= 3) {
      double p = __builtin_fma(e, 0.375, 0.5);
      s        = __builtin_fma(h * e, p, h);   // sqrt(r2)*(1 + O(e^3))
    } else {
      s = __builtin_fma(h * 0.5, e, h);        // sqrt(r2)*(1 - 3/8 e^2)
    }
    double d3 = __builtin_fma(r2, s, DBL_EPSILON);
    double z0 = __builtin_amdgcn_rcp(d3);     // ~2^-24 relative
    double e2 = __builtin_fma(-d3, z0, 1.0);
    double zm = z0 * mj;
    if constexpr (POLISH >= 3) {
      double q = __builtin_fma(e2, e2, e2);   // e2 + e2^2
      return __builtin_fma(zm, q, zm);        // mj/d3 * (1 + O(e2^3))
    } else {
      return __builtin_fma(zm, e2, zm);       // mj/d3 * (1 - e2^2)
    }
  }

  // The same quantity without the reciprocal, for r2 >= 2^-16 (K1's fast path).  With u = r2^(-3/2):
  //     mj / (r2^(3/2) + eps) = mj * u / (1 + eps*u) = mj * u * (1 - eps*u + (eps*u)^2 - ...)
  // and eps*u <= 2^-52 * 2^24 = 2^-28 there, so dropping (eps*u)^2 <= 2^-56 is below half an ulp.  u comes from the
  // 2^-24 v_rsq_f64 seed y by one THIRD-order step on the cube:  y^3 * (1 - e)^(-3/2) = y^3 * (1 + 3/2 e + 15/8 e^2 + O(e^3)),
  // e = 1 - r2*y^2 <= 2^-23 (truncation 35/16 e^3 < 3e-21).  Both corrections share one FMA:
  //     w = (mj*y^3) * (1 + g),  g = e*(3/2 + 15/8 e) - eps*y^3          (the cross term of the two is < 2^-50 * 2^-28)
  // 8 full-rate ops + 1 transcendental = 48 issue cycles per wave-pair instead of 12 + 2 = 80 for weight(), and only
  // rounding error is left: a = fl(y*y) perturbs e by <= 2^-53 (x 3/2 in w), then y^3, mj*y^3 and the final FMA round once
  // each: <= 2.5 ulp per term, no bias (measured in tests/test_gpu_all_pairs.py::test_pair_term_accuracy).
  static constexpr uint32_t near_hi = 0x3EF00000u;  // high word of 2^-16: r2 below this takes weight()
  // r2 >= 4: eps*u <= 2^-52 / 8 = 2^-55, an eighth of an ulp of the weight — the term is dropped (weight_far<false>), which
  // saves the eps*y^3 multiply: 7 full-rate ops + 1 transcendental.  K1 takes that form when EVERY pair of a batch is that far
  // (one more compare on the minimum it already tracks); in a mixed batch each lane selects eps or 0 by its own r2 (the high
  // word of DBL_EPSILON is all there is to select: its low word is 0), and fma(p, e, -0) == p * e bit for bit, so a pair's
  // weight never depends on which other pairs share the batch.
  static constexpr uint32_t far_hi = 0x40100000u;   // high word of 4.0
  // k15 = 1.5 in a VGPR pair and k1875 = 1.875 in an SGPR pair, held by the caller (pair_consts): neither is an inline
  // constant, and left to itself hipcc feeds a VOP2 v_fmac with the literal and re-creates 1.5 in its accumulator
  // operand with a v_mov per pair.
  template <bool EPS = true>
  __device__ static __forceinline__ double weight_far(double r2, double mj, double k15, double k1875, double eps = DBL_EPSILON) {
    double y  = __builtin_amdgcn_rsq(r2);
    double a  = y * y;
    double e  = __builtin_fma(-r2, a, 1.0);
    double y3 = a * y;
    double p  = __builtin_fma(e, k1875, k15);
    double g;
    if constexpr (EPS) g = __builtin_fma(p, e, -(eps * y3));  // eps: DBL_EPSILON, or a lane's own choice of DBL_EPSILON / 0
    else g = p * e;
    double my = mj * y3;
    return __builtin_fma(my, g, my);
  }

  // K1's form of the same series (f64, both K1 twins, LDS tiles and scalar stream alike) with the source's mass folded into
  // the polynomial's constants.  `my = mj*y3` above exists only because the mass multiplies a polynomial whose constants are
  // global; with M15 = fl(1.5 mj) and M1875 = fl(1.875 mj) made ONCE per source (src_cst below: plain multiplies, by the
  // pre-pass or per lane after the ds_read) the polynomial delivers mj (1 + e(3/2 + 15/8 e)) directly:
  //     t = fma(e, M1875, M15);  s = fma(t, e, mj);  w = y3 * s                  6 full-rate ops + 1 transcendental (was 7)
  // The eps term, where a pair takes it, goes into e instead of into the sum: r^3 + eps = (r2 + 2/3 eps y + O(eps^2))^(3/2), so
  //     e' = 1 - (r2 + 2/3 eps y) y^2 = fma(-2/3 eps, y3, e)                     7 + 1 (was 8)
  // and the SAME polynomial in e' carries both corrections, their cross term included (weight_far adds -eps y^3 beside
  // e(3/2 + 15/8 e) and leaves the cross term 3 e eps y^3 out: up to 2^-21.6 * 2^-28, +-8 ulp at r2 = 2^-16); what is left out
  // here is (eps u)^2 / 6 < 2^-58.  No per-source quantity is needed for it: 2/3 eps is one scalar constant (pair_consts).
  // The rounding budget is that of weight_far: a and y3, ONE rounding at mass scale (M15 and M1875 are rounded, but they multiply
  // e <= 2^-23: 2^-76 of the weight), the last product (tests/test_folded_weight.py emulates old and new in exact arithmetic).
  // Bits change, accuracy does not.
  // Operands: a VOP3 instruction of this chip reads ONE scalar value, and t has two per-source operands — so in the scalar
  // stream M1875 arrives in SGPRs like the record itself, while M15 must be in a VGPR pair WITHOUT a VALU instruction having
  // put it there (two v_mov per source would give back half of the op saved): all 64 lanes load the same 16 bytes
  // (M15 of the batch's two sources) with one vector-memory instruction, requested a batch ahead (k1_sgpr_body.inc).
  // fma(-0, y3, e) == e bit for bit (y3 > 0: the product is -0, and e + (-0) == e also for e == +-0), so a lane that selects
  // 0 instead of 2/3 eps for a far pair of a MIXED batch gets the bits of the all-far batch's form: a pair's weight depends on
  // that pair alone.  A zero-mass padding record has M15 = M1875 = 0 and w = y3 * 0 = 0.
  // SMASS (mj is in SGPRs and this is its only use: the softened twin at one target per lane): s is written as the VOP3
  // instruction it should be — hipcc otherwise copies mj into a VGPR pair with two v_mov per source to make it the tied
  // accumulator of a v_fmac, which costs more than the multiply saved.
  static constexpr double eps23 = 2.0 / 3.0 * DBL_EPSILON;
  template <bool EPS, bool SMASS = false>
  __device__ static __forceinline__ double weight_far_folded(double r2, double mj, double m15, double m1875, double keps = eps23) {
    double y  = __builtin_amdgcn_rsq(r2);
    double a  = y * y;
    double e  = __builtin_fma(-r2, a, 1.0);
    double y3 = a * y;
    if constexpr (EPS) e = __builtin_fma(-keps, y3, e);  // keps: 2/3 eps (pair_consts), or a lane's own choice of that / 0
    double t = __builtin_fma(e, m1875, m15);
    double s;
    if constexpr (SMASS) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(s) : "v"(t), "v"(e), "s"(mj));
    else s = __builtin_fma(t, e, mj);
    return y3 * s;
  }
};

template <>
struct pair_math<float> {
  static constexpr float tiny = 1e-37f;
  // returns mj / (r2 * sqrt(r2) + FLT_EPSILON).  v_rsq_f32 / v_rcp_f32 are 1-ulp instructions, so no polish:
  // the term is within ~4 ulp (5e-7) of the exact expression, below the spread between the reference's own
  // float builds (its powf/divide chain is not reproducible at this level) and far below the
  // float parity tolerance (2e-5).  3 full-rate ops + 2 transcendentals.
  __device__ static __forceinline__ float weight(float r2, float mj) {
    float y0 = __builtin_amdgcn_rsqf(r2);
    float d3 = __builtin_fmaf(r2, r2 * y0, FLT_EPSILON);
    return __builtin_amdgcn_rcpf(d3) * mj;
  }
  // Sparse systems (ap_far_mode): a pair at r2 >= 4 takes m y^3 — eps u <= 2^-26 there, an eighth of an ulp.  Measured with it
  // and not kept (round 3, profiles/r03/f32_pair_forms.txt): the reciprocal-free series m u (1 - q + q^2) for every far pair —
  // v_rcp_f32 costs ~3 FMA slots on this chip, the series 2-3 FMAs plus a near check: slower wherever the check is taken.
  static constexpr uint32_t far_bits = 0x40800000u;  // 4.0f
};

// LDS source record: (x[0..D-1], m) padded to a power-of-two size so one or two ds_read_b128 fetch it.
template <typename T, int D>
struct alignas(sizeof(T) * 4) src_rec {
  T p[3];  // D used
  T m;
};

// Per-source constants of K1's f64 pair form (pair_math<double>::weight_far_folded): M15 = fl(1.5 m), M1875 = fl(1.875 m), by
// plain multiplies wherever they are made, so that every producer rounds the same — the pre-pass of the scalar stream (cst_batch
// below) and the LDS-tile form, per lane after its ds_read.  Float has none.
template <typename T>
struct src_cst {
  __device__ __forceinline__ static src_cst of(T) { return {}; }
};
template <>
struct src_cst<double> {
  double m15, m1875;
  __device__ __forceinline__ static src_cst of(double m) { return {1.5 * m, 1.875 * m}; }
};
// What the scalar stream reads beside a 64-byte batch of two f64 records (sources 2b and 2b + 1): M15 of both in the first 16
// bytes — ONE wave-uniform global_load_dwordx4 puts them into VGPRs — and M1875 of both in the second — one s_load_dwordx4.
struct alignas(32) cst_batch {
  double m15[2], m1875[2];
};

// acc += w * (xj - xi) with r2 built by FMAs starting from TINY.
template <typename T, int D>
__device__ __forceinline__ void pair_accumulate(T (&acc)[D], const T (&xi)[D], const src_rec<T, D>& s) {
  T d[D];
#pragma unroll
  for (int k = 0; k < D; ++k) d[k] = s.p[k] - xi[k];
  T r2 = pair_math<T>::tiny;
#pragma unroll
  for (int k = 0; k < D; ++k) r2 = __builtin_elementwise_fma(d[k], d[k], r2);
  T w = pair_math<T>::weight(r2, s.m);
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = __builtin_elementwise_fma(w, d[k], acc[k]);
}

// NB sources against one target, written stage by stage (all differences, all r2, all weights, then the accumulation)
// so that NB independent dependency chains are in flight: under register pressure hipcc otherwise emits one pair after
// the other through the same temporaries, each transcendental followed by a wait state (K2: 446 s_nop per 256 pairs).
template <typename T, int D, int NB>
__device__ __forceinline__ void pair_accumulate_multi(T (&acc)[D], const T (&xi)[D], const src_rec<T, D>* s) {
  T d[NB][D], r2[NB], w[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int k = 0; k < D; ++k) d[b][k] = s[b].p[k] - xi[k];
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    r2[b] = pair_math<T>::tiny;
#pragma unroll
    for (int k = 0; k < D; ++k) r2[b] = __builtin_elementwise_fma(d[b][k], d[b][k], r2[b]);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) w[b] = pair_math<T>::weight(r2[b], s[b].m);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] = __builtin_elementwise_fma(w[b], d[b][k], acc[k]);
  }
}

// K2 in f64: the same pairs with K1's reciprocal-free weight and NO per-chain branch (a near-pair branch in every chain makes
// hipcc keep all chains' temporaries alive: 350 VGPRs).  The caller tracks the smallest high word of r2 it has seen and, if a
// block of pairs held one below 2^-16 (a self pair, a very close body), discards that block's sums and recomputes them with the
// guarded form (pair_accumulate_multi) — the far results of such a block may be inf/NaN and are never used.
template <int D, int NB>
__device__ __forceinline__ void pair_accumulate_far(double (&acc)[D], const double (&xi)[D], const src_rec<double, D>* s,
                                                    uint32_t& lowest, double k15, double k1875) {
  double d[NB][D], r2[NB], w[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int k = 0; k < D; ++k) d[b][k] = s[b].p[k] - xi[k];
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    r2[b] = pair_math<double>::tiny;
#pragma unroll
    for (int k = 0; k < D; ++k) r2[b] = __builtin_elementwise_fma(d[b][k], d[b][k], r2[b]);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    w[b]              = pair_math<double>::weight_far(r2[b], s[b].m, k15, k1875);
    const uint32_t hi = uint32_t(__builtin_bit_cast(unsigned long long, r2[b]) >> 32);
    lowest            = hi < lowest ? hi : lowest;
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] = __builtin_elementwise_fma(w[b], d[b][k], acc[k]);
  }
}

// Loop-invariant operands of pair_batch that must stay in registers (made opaque to the optimiser once, outside the loop).
template <typename T>
struct pair_consts {
  __device__ __forceinline__ pair_consts() {}
};
template <>
struct pair_consts<double> {
  double k15, k1875;
  double keps;  // 2/3 eps of K1's folded form (weight_far_folded), in an SGPR pair; no instruction where it is not used
  __device__ __forceinline__ pair_consts() : k15(1.5), k1875(1.875), keps(pair_math<double>::eps23) {
    asm volatile("" : "+v"(k15));
    asm volatile("" : "+s"(k1875));
    asm("" : "+s"(keps));
  }
};

// K1's unit of work: U source records against the R targets of a lane.  acc[r] += w * (x_j - x_i) in source order.
// `ffar` is a property of the LAUNCH, compiled as two copies of the kernels' source loops — inside ONE loop hipcc hoists the
// common head of the two rules above the branch and interleaves the f32 pair chains, which costs 15 % (24.4 against 21.2 ms at
// config 3) — (ap_far_mode: the variances of ALL positions say that few batches can hold a pair closer than 2 — k1_rule below;
// every rank and every shard window of one system computes the same bits) and selects the per-pair rule:
//   dense (ffar false): f64 weight_far_folded<true> for r2 >= 2^-16, weight<3>() below; f32 weight().
//   sparse (ffar true): f64 weight_far_folded<false> for r2 >= 4, weight_far_folded<true> in [2^-16, 4), weight<3>() below;
//                       f32 m y^3 for r2 >= 4, weight() below.
// f64 takes the sources' constants kc (src_cst: M15, M1875) beside the records.
// The smallest r2 of the batch (one v_min3_u32 per two pairs on the high words) decides with one wave-uniform branch which code
// runs; in a mixed batch each lane keeps, pair by pair, what its own r2 asks for.  Under a given rule a pair's term depends on
// that pair alone, never on which other targets share the wave: results stay bitwise independent of the shard window.
// (In the dense regime the sparse rule would put every batch on the mixed path: measured 3.20 against 2.62 ms at config 2.)
template <typename T, int D, int R, int U, bool ffar>
__device__ __forceinline__ void pair_batch(T (&acc)[R][D], const T (&xi)[R][D], const src_rec<T, D> (&s)[U],
                                           const src_cst<T> (&kc)[U], const pair_consts<T>& pc) {
  if constexpr (sizeof(T) == 4) {
    if constexpr (!ffar) {
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) pair_accumulate<T, D>(acc[r], xi[r], s[u]);
    } else {
      // sparse system (ap_far_mode): a pair at r2 >= 4 takes m y^3 — eps u <= 2^-26 there, an eighth of an ulp — and every other
      // pair the guarded form above, by ITS OWN r2; a batch whose pairs are all that far never issues the reciprocal
      T d[U][R][D], r2[U][R], w[U][R];
      uint32_t lowest = 0xffffffffu;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
          for (int k = 0; k < D; ++k) d[u][r][k] = s[u].p[k] - xi[r][k];
          T q = pair_math<T>::tiny;
#pragma unroll
          for (int k = 0; k < D; ++k) q = __builtin_elementwise_fma(d[u][r][k], d[u][r][k], q);
          r2[u][r]            = q;
          const uint32_t bits = __builtin_bit_cast(uint32_t, q);
          lowest              = bits < lowest ? bits : lowest;
        }
      T y[U][R];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          y[u][r] = __builtin_amdgcn_rsqf(r2[u][r]);
          w[u][r] = s[u].m * ((y[u][r] * y[u][r]) * y[u][r]);
        }
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(lowest < pair_math<T>::far_bits) != 0ull, 0)) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const T d3 = __builtin_fmaf(r2[u][r], r2[u][r] * y[u][r], FLT_EPSILON);  // == pair_math<float>::weight
            const T wn = __builtin_amdgcn_rcpf(d3) * s[u].m;
            w[u][r]    = __builtin_bit_cast(uint32_t, r2[u][r]) < pair_math<T>::far_bits ? wn : w[u][r];
          }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int k = 0; k < D; ++k) acc[r][k] = __builtin_elementwise_fma(w[u][r], d[u][r][k], acc[r][k]);
    }
  } else {
    T d[U][R][D], r2[U][R], w[U][R];
    uint32_t lowest = 0xffffffffu;
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int k = 0; k < D; ++k) d[u][r][k] = s[u].p[k] - xi[r][k];
        T q = pair_math<T>::tiny;
#pragma unroll
        for (int k = 0; k < D; ++k) q = __builtin_elementwise_fma(d[u][r][k], d[u][r][k], q);
        r2[u][r] = q;
        const uint32_t hi = uint32_t(__builtin_bit_cast(unsigned long long, q) >> 32);
        lowest            = hi < lowest ? hi : lowest;
      }
    if constexpr (!ffar) {
      // dense system: every pair takes the eps form unless some lane holds one below 2^-16
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r)
          w[u][r] = pair_math<T>::template weight_far_folded<true>(r2[u][r], s[u].m, kc[u].m15, kc[u].m1875, pc.keps);
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(lowest < pair_math<T>::near_hi) != 0ull, 0)) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const uint32_t hi = uint32_t(__builtin_bit_cast(unsigned long long, r2[u][r]) >> 32);
            const T wn        = pair_math<T>::template weight<3>(r2[u][r], s[u].m);  // rare: take the <= 2 ulp form
            w[u][r]           = hi < pair_math<T>::near_hi ? wn : w[u][r];
          }
      }
    } else if (__builtin_expect(__builtin_amdgcn_ballot_w64(lowest < pair_math<T>::far_hi) == 0ull, 1)) {
      // sparse system, every pair of the batch at r2 >= 4: no eps term at all
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) w[u][r] = pair_math<T>::template weight_far_folded<false>(r2[u][r], s[u].m, kc[u].m15, kc[u].m1875);
    } else {
      // sparse system, some pair is closer: every lane keeps, pair by pair, what ITS r2 asks for — 2/3 eps or 0 in the far form
      // (fma(-0, y3, e) == e: a far pair gets the bits of the all-far batch above) ...
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint32_t hi = uint32_t(__builtin_bit_cast(unsigned long long, r2[u][r]) >> 32);
          const T mine      = hi < pair_math<T>::far_hi ? pc.keps : T(0);
          w[u][r]           = pair_math<T>::template weight_far_folded<true>(r2[u][r], s[u].m, kc[u].m15, kc[u].m1875, mine);
        }
      // ... and the guarded reciprocal form below 2^-16 (the self pair, coincident or very close bodies)
      if (__builtin_expect(__builtin_amdgcn_ballot_w64(lowest < pair_math<T>::near_hi) != 0ull, 0)) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const uint32_t hi = uint32_t(__builtin_bit_cast(unsigned long long, r2[u][r]) >> 32);
            const T wn        = pair_math<T>::template weight<3>(r2[u][r], s[u].m);
            w[u][r]           = hi < pair_math<T>::near_hi ? wn : w[u][r];
          }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) acc[r][k] = __builtin_elementwise_fma(w[u][r], d[u][r][k], acc[r][k]);
  }
}

// K1's unit of work in a block whose bounding boxes prove every pair far (k1_sgpr_body.inc: the certificate; f64, sparse rule; the records are in SGPRs).
// Operation for operation what an all-far batch of pair_batch<ffar = true> executes — the same differences, the same r2 chain
// seeded with `tiny`, weight_far_folded<false>, the same accumulations in the same order — without the smallest high word, the
// compare and the branch: a target's sum has the same bits whether or not its blocks were certified.
template <typename T, int D, int R, int U>
__device__ __forceinline__ void pair_batch_far(T (&acc)[R][D], const T (&xi)[R][D], const src_rec<T, D> (&s)[U], const src_cst<T> (&kc)[U]) {
  static_assert(sizeof(T) == 8, "the certified copy exists in f64 only");
  T d[U][R][D], r2[U][R], w[U][R];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int k = 0; k < D; ++k) d[u][r][k] = s[u].p[k] - xi[r][k];
      T q = pair_math<T>::tiny;
#pragma unroll
      for (int k = 0; k < D; ++k) q = __builtin_elementwise_fma(d[u][r][k], d[u][r][k], q);
      r2[u][r] = q;
    }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < R; ++r)  // (SMASS at one target per lane, as in the softened twin: the same operation, no v_mov of the mass)
      w[u][r] = pair_math<T>::template weight_far_folded<false, R == 1>(r2[u][r], s[u].m, kc[u].m15, kc[u].m1875);
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < D; ++k) acc[r][k] = __builtin_elementwise_fma(w[u][r], d[u][r][k], acc[r][k]);
}

// float has no per-source constants: the form K2's compiler-scheduled kernel calls
template <typename T, int D, int R, int U, bool ffar>
__device__ __forceinline__ void pair_batch(T (&acc)[R][D], const T (&xi)[R][D], const src_rec<T, D> (&s)[U], const pair_consts<T>& pc) {
  static_assert(sizeof(T) == 4, "f64 callers pass the sources' constants (src_cst)");
  const src_cst<T> none[U] = {};
  pair_batch<T, D, R, U, ffar>(acc, xi, s, none, pc);
}

// ---- softened pairs (ABI 2.4: nbody_all_pairs_softened_force, the softened octree walk and energies) -----------------------
// Plummer softening: the pair term is  m_j * (x_j - x_i) / (r2 + e2)^(3/2),  e2 = fl_T(eps * eps) > 0, with r2 + e2 built by the
// same FMA chain the unsoftened kernels use, seeded with e2 where they seed `tiny`.  q = r2 + e2 >= e2 never reaches 0, so there is
// no eps term, no near-pair branch and no pair rule: the self pair and coincident bodies add w * 0 = 0 because their difference is 0.
//   f64: weight_far<false> above, (m y^3)(1 + e(3/2 + 15/8 e)), y = v_rsq_f64(q): 7 full-rate ops + 1 transcendental, <= 2.5 ulp
//        (soft_weight: the octree walk, Hermite); K1's twin takes the same series as weight_far_folded<false>: 6 + 1.
//   f32: m y^3 from the 1-ulp v_rsq_f32: 3 ops + 1 transcendental, <= ~3 ulp.
// y^3 = q^(-3/2) must stay finite for q = e2, which bounds e2 from below (check_softening: kSoftMinE2).
template <typename T>
__device__ __forceinline__ T soft_weight(T q, T mj, const pair_consts<T>& pc) {
  if constexpr (sizeof(T) == 8) {
    return pair_math<double>::template weight_far<false>(q, mj, pc.k15, pc.k1875);
  } else {
    const T y = __builtin_amdgcn_rsqf(q);
    return mj * ((y * y) * y);
  }
}

// K1's unit of work in the softened form: U source records against the R targets of a lane, stage by stage like pair_batch.
// SSRC: the records are in SGPRs (the scalar stream).
template <typename T, int D, int R, int U, bool SSRC = false>
__device__ __forceinline__ void pair_batch_soft(T (&acc)[R][D], const T (&xi)[R][D], const src_rec<T, D> (&s)[U],
                                                const src_cst<T> (&kc)[U], const pair_consts<T>& pc, T e2) {
  T d[U][R][D], q[U][R], w[U][R];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int k = 0; k < D; ++k) d[u][r][k] = s[u].p[k] - xi[r][k];
      T t = e2;
#pragma unroll
      for (int k = 0; k < D; ++k) t = __builtin_elementwise_fma(d[u][r][k], d[u][r][k], t);
      q[u][r] = t;
    }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (sizeof(T) == 8)
        w[u][r] = pair_math<T>::template weight_far_folded<false, SSRC && R == 1>(q[u][r], s[u].m, kc[u].m15, kc[u].m1875);
      else w[u][r] = soft_weight<T>(q[u][r], s[u].m, pc);
    }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < D; ++k) acc[r][k] = __builtin_elementwise_fma(w[u][r], d[u][r][k], acc[r][k]);
}

// The smallest e2 a softened call accepts: e2^(-3/2) <= 2^126 (f32) / 2^1020 (f64), so that y^3 (and the potential's y) of the
// closest possible pair is finite and a coincident pair adds 0 * finite = 0.  eps >= 1.5e-13 in float, >= 1.4e-103 in double.
template <typename T>
constexpr T kSoftMinE2 = sizeof(T) == 4 ? T(0x1p-84f) : T(0x1p-680);

// eps of a softened call -> e2 = fl_T(T(eps) * T(eps)); NBODY_ERR_ARG (no GPU needed) unless eps is finite and > 0 and e2 is a
// normal number of T no smaller than kSoftMinE2<T>.
template <typename T>
inline int check_softening(double eps, T* e2_out) {
  NB_ARG(eps > 0.0 && eps <= DBL_MAX, "softening length eps = %g must be finite and > 0", eps);
  const T te = T(eps);
  const T e2 = te * te;
  NB_ARG(e2 >= kSoftMinE2<T> && e2 <= (sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)),
         "softening length eps = %g: eps^2 = %g in %s is outside [%g, max]: its square must be a normal number whose ^(-3/2) is finite",
         eps, double(e2), sizeof(T) == 4 ? "float" : "double", double(kSoftMinE2<T>));
  *e2_out = e2;
  return NBODY_OK;
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---- which per-pair rule a launch takes: ap_far_mode ---------------------------------------------------------------------
// Sparse iff a batch of 256 pairs rarely holds one closer than 2.  For bodies spread with density rho (normalised) the chance that a
// random pair is that close is (32 pi / 3) * integral(rho^2); for a uniformly filled box that integral is 1 / V, and the rule asks
// for 256 * (4/3 pi 8) / V < 0.05 (256 * 4 pi / A in 2D).  V is NOT the bounding box (rounds 3-4): one escaper inflates that at will
// — config 2 as written (the uniform cube, dt = 0.1) ejects a few bodies at ten times the bulk's speed, after 35 steps the box says
// "sparse" while 98 % of the bodies sit in a cube of side 7 and EVERY batch holds a close pair, and the sparse rule's mixed path
// made the last 65 of its 100 steps 8.5 % slower (profiles/r05/config2_state_probe.txt).  V is the volume of the uniformly
// filled box with the positions' VARIANCES: side_k = sqrt(12 var_k) — the same number for a uniform box, 0.94 of the Gaussian's
// 1 / integral(rho^2), and a few escapers move it by their share of the mass, not by their distance.  Real systems are clumpier
// than their variances (the galaxy's two discs: 6 % of the batches hold a close pair at V = 3e6) — the rule only has to tell a
// cube from a galaxy.  The moments are summed in double in a FIXED order (per block of 256 bodies, then over the blocks in index
// order by the last block to finish), from all sz positions whatever the shard window: every rank, every window and every run
// computes the same bits, so the rule — which fixes the rounding of every pair — is a function of the state alone.
struct k1_rule {
  double volume;    // prod_k sqrt(12 var_k)
  uint32_t sparse;  // volume >= threshold
  uint32_t ticket;  // blocks of the running prepare launch that have delivered their partial sums (0 between launches)
};
constexpr uint32_t kFarMinBodies = 32768;  // below this the rule is "dense" by definition (from sz alone: nothing is measured)
template <int D>
constexpr double kFarMinVolume = D == 3 ? 1.7e5 : 6.4e4;
__device__ __forceinline__ bool ap_far_mode(const k1_rule* __restrict__ rule) {
  if (rule == nullptr) return false;
  return __builtin_amdgcn_readfirstlane(int(rule->sparse)) != 0;
}

// ---- the far certificate of a K1 block (f64 scalar stream, sparse rule) ---------------------------------------------------
// The sparse rule asks every pair whether its computed r2 is >= 4.  For a block — one target group against one source chunk —
// one comparison of two bounding boxes often answers for all of its pairs: if on some axis the boxes are kFarGap = 3 apart, every
// pair's true separation is >= 3, r2 >= 9, and the three roundings of the r2 chain cannot bring the computed value below 4 (the
// slack of 1 in the gap is there so that no rounding analysis is needed).  Such a block runs pair_batch_far.  The chunk's box
// comes from the pre-pass (all_pairs.hip: k1_prepare_kernel; it covers every record of the chunk, padding included, and is the
// whole line on every axis if a record is not finite); the targets' side is taken per lane, which is the group's box exactly:
// fl(t - hi) is monotone in t, so "every lane's gap >= 3" is "the gap from the group's minimum >= 3".  An infinite gap — a target
// that is not finite — does not count, and a comparison with NaN is false: non-finite positions never certify.  (A defence only:
// the variances of such a system are NaN, the rule is dense and no certificate is attempted in the first place.)
constexpr double kFarGap = 3.0;
// chunk_box: lo[D], hi[D] of the block's source chunk, wave-uniform, through the constant address space — the pre-pass wrote the
// boxes, nothing writes them while K1 runs, and the loads are scalar ones like those of the records
template <typename T, int D, int R>
__device__ __forceinline__ bool k1_block_is_far(const T (&xi)[R][D], const T __attribute__((address_space(4))) * chunk_box) {
  bool far = false, finite = true;  // a group that holds a target with a coordinate that is not finite certifies on no axis
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int k = 0; k < D; ++k) finite = finite & ((xi[r][k] - xi[r][k]) == T(0));
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const T lo = chunk_box[k], hi = chunk_box[D + k];
    bool above = true, below = true;  // this lane's targets lie above (below) the chunk on axis k, by the gap
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const T ga = xi[r][k] - hi, gb = lo - xi[r][k];
      above = above & (ga >= T(kFarGap));  // (finite targets against a finite box or the whole line: the gap is finite or -inf)
      below = below & (gb >= T(kFarGap));
    }
    far = far | (__builtin_amdgcn_ballot_w64(!above) == 0ull) | (__builtin_amdgcn_ballot_w64(!below) == 0ull);
  }
  return far & (__builtin_amdgcn_ballot_w64(!finite) == 0ull);
}

// ---- scalar-stream helpers (K1's default form, the energies) ------------------------------------------------
constexpr int kTileJ = 512;  // source records per tile (fixed: the rounding order of K1 depends on it)

typedef uint32_t sgpr16 __attribute__((ext_vector_type(16)));
// `tie` is a VGPR value the surrounding arithmetic reads (sload16) or produces (swait): the statements carry no
// instruction for it, it only pins them in program order relative to that arithmetic (inline asm is otherwise free to
// drift across pure FP code during instruction selection).
template <typename V>
__device__ __forceinline__ sgpr16 sload16(const void* p, V& tie) {  // p wave-uniform, 4-byte aligned
  sgpr16 r;
  asm volatile("s_load_dwordx16 %0, %2, 0x0" : "=s"(r), "+v"(tie) : "s"(p));
  return r;
}
template <typename V>
__device__ __forceinline__ void swait(sgpr16& v, V& tie) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v), "+v"(tie));
}

// The constants of a batch of two f64 sources (cst_batch) on their way into registers, beside the batch's records: m15 by a
// wave-uniform vector load (every lane reads the same 16 bytes: one cache line, one instruction on the VMEM pipe, no VALU),
// m1875 by a scalar load.  Requested with the records, a compute phase ahead; completed by cswait, which is swait with vmcnt(0)
// added — vector loads return in order, and when a batch is waited for the NEXT one has not been requested yet, so 0 is the
// exact count.  hipcc does not count these loads; its own waits can only become stricter by them (a wait on vmcnt(n) for one of
// its loads allows n NEWER loads in flight, and there are at least as many as it knows of).
typedef uint32_t reg4 __attribute__((ext_vector_type(4)));
struct cst_regs {
  reg4 v, s;
};
template <typename V>
__device__ __forceinline__ cst_regs cload(const void* p, uint32_t vzero, V& tie) {  // p wave-uniform, 16-byte aligned; vzero: 0 in a VGPR
  cst_regs r;
  asm volatile("global_load_dwordx4 %0, %3, %4\n\ts_load_dwordx4 %1, %4, 0x10" : "=&v"(r.v), "=&s"(r.s), "+v"(tie) : "v"(vzero), "s"(p));
  return r;
}
template <typename V>
__device__ __forceinline__ void cswait(sgpr16& v, cst_regs& c, V& tie) {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+s"(v), "+v"(c.v), "+s"(c.s), "+v"(tie));
}
__device__ __forceinline__ void cst_unpack(const cst_regs& c, src_cst<double> (&kc)[2]) {
  struct pair_t {
    double d[2];
  };
  const pair_t v = __builtin_bit_cast(pair_t, c.v), s = __builtin_bit_cast(pair_t, c.s);
  kc[0] = {v.d[0], s.d[0]};
  kc[1] = {v.d[1], s.d[1]};
}

// K1 launch shape: validation shared by the process-wide default and the per-context setting
inline int check_tuning(int split, int tpt, int path) {
  NB_ARG(split == 0 || split == 1 || split == 2 || split == 4 || split == 8, "split must be 0, 1, 2, 4 or 8 (got %d)", split);
  NB_ARG(tpt >= 0 && tpt <= 2, "targets_per_thread must be 0, 1 or 2 (got %d)", tpt);
  NB_ARG(path >= 0 && path <= 2, "source path must be 0 (auto), 1 (LDS tiles) or 2 (scalar stream), got %d", path);
  return NBODY_OK;
}

// all_pairs.hip: per-(device, stream) packed-source scratch of the scalar-stream K1 (reserved by nbody_create, freed by nbody_destroy)
int ap_scratch_reserve(hipStream_t st, const nbody_state* view);
void ap_scratch_release(hipStream_t st);
int ap_scratch_get(hipStream_t st, int which, size_t bytes, void** out);  // which: 0 packed sources, 1 K1 turn words, 2 energies, 3 the pair rule (k1_rule + the blocks' partial moments), 4 K1 hand-off status, 5 K1 chunk sums of small launches, 6 the packed sources' f64 pair constants
void ap_status_mark(hipStream_t st);  // a recorded step is being replayed on st: it may hold a turn-passing K1
int ap_status_read(hipStream_t st, unsigned long long out[6], bool clear);  // waits for the stream; NBODY_ERR_STATE while a K1 hand-off failure is recorded
int ap_pack_sources(const nbody_state* s, hipStream_t st, void** packed_out);
void ap_auto_chunks(uint32_t sz, uint32_t* chunks, uint32_t* tiles_per_chunk);
// energy.hip: nbody_calc_energies' reduction over per-body sums S_i that `fill` writes (T[sz], on st) into the buffer it is handed:
// kinetic = 1/2 sum_i m_i |v_i|^2 (the same launch: the same bits), potential = -c/2 sum_i m_i S_i.  Blocking; host outputs of one T.
int energies_from_sums(const nbody_state* s, hipStream_t st, int (*fill)(void* sums, void* ctx), void* ctx, void* ke_out, void* pe_out);

}  // namespace nbody
