// The schedule of block (individual) time steps, shared by the three integrators that take them: hermite_block.inc (order 4),
// hermite6_block.inc (order 6) and octree_block.inc (the octree leapfrog).  Every body i has a level l_i (its step is dtmax 2^-l_i,
// step_of(l_i, L) ticks of dtmax 2^-L) and the time tau_i of its last update in ticks.  A block step begins with four launches:
//   min        tau_next = min_i(tau_i + step_i): strips of kSchedStrip bodies, wave and block minimum, one atomicMin of an unsigned
//              integer per block (a minimum does not depend on the order it is taken in);
//   count      due bodies (tau_i + step_i == tau_next) per strip of POSITIONS of an order: the body order (sidx == NULL) or another
//              (sidx = a permutation of the body indices, such as the octree's key order);
//   scan       ONE block: exclusive scan of the strips' counts; the body-order pass publishes (n_act, tau_next) to the schedule words
//              and to pinned host memory and re-arms the minimum;
//   compact    the due bodies of the order, order kept: the strip's offset + the counts of the earlier rows and waves of the strip +
//              the lane's rank in its wave's ballot.  No atomics: a slot follows from lev and tau alone.
// Each integrator ends its step with a kernel of its own that gives every active body its new level (block_next_level) and tau.
// The kernels are static, like radix_sort.hpp's: every translation unit that includes this header carries its own copy.
#pragma once
#include "common.hpp"

namespace nbody {

constexpr int kSchedBlock      = 256;
constexpr int kSchedWaves      = kSchedBlock / 64;
constexpr int kSchedItems      = 16;                         // rows of kSchedBlock positions per schedule strip
constexpr uint32_t kSchedStrip = kSchedBlock * kSchedItems;  // 4096 positions per schedule block
constexpr uint32_t kSchedNoTime = 0xffffffffu;

// sched[0]: the running minimum (kSchedNoTime between steps), sched[1]: n_act, sched[2]: tau_next of the step in flight
enum { kSchedMin = 0, kSchedCount = 1, kSchedNext = 2, kSchedWords = 4 };

__device__ __forceinline__ uint32_t step_of(int32_t lev, int32_t L) { return 1u << (L - lev); }

// ---- schedule ------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(kSchedBlock) void block_sched_min_kernel(const int32_t* __restrict__ lev, const uint32_t* __restrict__ tau,
                                                                             uint32_t* __restrict__ sched, uint32_t n, int32_t L) {
  __shared__ uint32_t wmin[kSchedWaves];
  uint32_t mn = kSchedNoTime;
#pragma unroll
  for (int k = 0; k < kSchedItems; ++k) {
    const uint32_t i = blockIdx.x * kSchedStrip + k * kSchedBlock + threadIdx.x;
    if (i < n) {
      const uint32_t due = tau[i] + step_of(lev[i], L);
      mn                 = due < mn ? due : mn;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = __shfl_xor(mn, off);
    mn               = o < mn ? o : mn;
  }
  if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kSchedWaves; ++w) mn = wmin[w] < mn ? wmin[w] : mn;
    atomicMin(&sched[kSchedMin], mn);
  }
}

// position p of the order -> its body (sidx == NULL: the body order itself); true when that body is due at `next`
__device__ __forceinline__ bool block_due(const int32_t* lev, const uint32_t* tau, const uint32_t* sidx, uint32_t p, uint32_t n, int32_t L,
                                          uint32_t next, uint32_t* body) {
  if (p >= n) return false;
  const uint32_t i = sidx ? sidx[p] : p;
  *body            = i;
  return i < n && tau[i] + step_of(lev[i], L) == next;  // (i < n always: sidx is a permutation)
}

// `word`: the schedule word that holds tau_next — kSchedMin before the body-order scan has published it, kSchedNext after
static __global__ __launch_bounds__(kSchedBlock) void block_sched_count_kernel(const int32_t* __restrict__ lev, const uint32_t* __restrict__ tau,
                                                                               const uint32_t* __restrict__ sidx,
                                                                               const uint32_t* __restrict__ sched, int word,
                                                                               uint32_t* __restrict__ bcount, uint32_t n, int32_t L) {
  __shared__ uint32_t wcnt[kSchedWaves];
  const uint32_t next = sched[word];
  uint32_t c = 0, body = 0;
#pragma unroll
  for (int k = 0; k < kSchedItems; ++k) {
    const uint32_t p = blockIdx.x * kSchedStrip + k * kSchedBlock + threadIdx.x;
    c += uint32_t(__popcll(__ballot(block_due(lev, tau, sidx, p, n, L, next, &body))));
  }
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kSchedWaves; ++w) c += wcnt[w];
    bcount[blockIdx.x] = c;
  }
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

// one block: bcount[0 .. nb) -> its exclusive scan in place.  publish: the total to sched[kSchedCount] and the host, tau_next to
// sched[kSchedNext], and the running minimum re-armed for the next step (its readers of this step have finished: stream order)
static __global__ __launch_bounds__(kSchedBlock) void block_sched_scan_kernel(uint32_t* __restrict__ bcount, uint32_t* __restrict__ sched,
                                                                              uint32_t* __restrict__ host_pair, uint32_t nb, int publish) {
  __shared__ uint32_t wsum[kSchedWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t running = 0;
  for (uint32_t base = 0; base < nb; base += kSchedBlock) {
    const uint32_t j   = base + threadIdx.x;
    const uint32_t v   = j < nb ? bcount[j] : 0u;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    __syncthreads();  // the previous round's wsum has been read
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSchedWaves; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (j < nb) bcount[j] = running + before + inc - v;
    running += total;
  }
  if (publish && threadIdx.x == 0) {
    const uint32_t next = sched[kSchedMin];
    sched[kSchedCount]  = running;
    sched[kSchedNext]   = next;
    sched[kSchedMin]    = kSchedNoTime;
    host_pair[0]        = running;  // pinned host memory: read by the host after it has synchronised with the stream
    host_pair[1]        = next;
  }
}

static __global__ __launch_bounds__(kSchedBlock) void block_sched_compact_kernel(const int32_t* __restrict__ lev, const uint32_t* __restrict__ tau,
                                                                                 const uint32_t* __restrict__ sidx,
                                                                                 const uint32_t* __restrict__ sched,
                                                                                 const uint32_t* __restrict__ boff, uint32_t* __restrict__ out,
                                                                                 uint32_t n, int32_t L) {
  __shared__ uint32_t cnt[kSchedItems * kSchedWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t next = sched[kSchedNext];
  uint64_t ballot[kSchedItems];
  uint32_t body[kSchedItems];
#pragma unroll
  for (int k = 0; k < kSchedItems; ++k) {
    const uint32_t p = blockIdx.x * kSchedStrip + k * kSchedBlock + threadIdx.x;
    body[k]          = 0u;
    ballot[k]        = __ballot(block_due(lev, tau, sidx, p, n, L, next, &body[k]));
    if (lane == 0) cnt[k * kSchedWaves + wave] = uint32_t(__popcll(ballot[k]));
  }
  __syncthreads();
  if (wave == 0) {  // exclusive scan of the 64 (row, wave) counts, in position order
    const uint32_t v = cnt[lane];
    cnt[lane]        = wave_inclusive_scan(v, lane) - v;
  }
  __syncthreads();
  const uint32_t base  = boff[blockIdx.x];
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < kSchedItems; ++k) {
    if ((ballot[k] >> lane) & 1ull) {
      const uint32_t slot = base + cnt[k * kSchedWaves + wave] + uint32_t(__popcll(ballot[k] & below));
      if (slot < n) out[slot] = body[k];  // slot < n always: n_act <= n
    }
  }
}

// ---- levels ----------------------------------------------------------------------------------------------------------------------
// start: the smallest level whose step dtmax 2^-l is <= want, at most L
template <typename T>
__device__ __forceinline__ int32_t block_first_level(T want, T dtmax, int32_t L) {
  int32_t l = 0;
  T hs      = dtmax;
  while (l < L && hs > want) {
    hs *= T(0.5);
    ++l;
  }
  return l;
}

// The level of an active body after its step h = step * tick at level l, which ends at tick `next`; want: the step its integrator's
// criterion asks for (!limited: the criterion sets no limit, want is not read).  want < h: the smallest level deeper than l whose step
// is <= want, at most L; want >= 2 h, l > 0 and `next` on the coarser level's grid: l - 1, one doubling at most; else l.  Comparisons
// and exact halvings only.
template <typename T>
__device__ __forceinline__ int32_t block_next_level(T want, bool limited, T h, int32_t l, int32_t L, uint32_t step, uint32_t next) {
  int32_t nl = l;
  if (limited) {
    if (want < h) {
      T hs = T(0.5) * h;
      nl   = l + 1;
      while (nl < L && hs > want) {
        hs *= T(0.5);
        ++nl;
      }
      if (nl > L) nl = L;
    } else if (want >= T(2) * h && l > 0 && (next & (2u * step - 1u)) == 0u) {
      nl = l - 1;
    }
  } else if (l > 0 && (next & (2u * step - 1u)) == 0u) {
    nl = l - 1;
  }
  return nl;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct block_schedule {
  int32_t* lev      = nullptr;  // level l_i, [n]
  uint32_t* tau     = nullptr;  // last update time tau_i in ticks, [n]
  uint32_t* act     = nullptr;  // active list of the last block step, ascending body order, [n]
  uint32_t* bcount  = nullptr;  // due bodies per schedule strip, then its exclusive scan, [strips]
  uint32_t* sched   = nullptr;  // {running minimum, n_act, tau_next, -}
  uint32_t* pin     = nullptr;  // pinned, mapped host memory: {n_act, tau_next}, written by the schedule
  uint32_t* pin_dev = nullptr;  // its device address
  uint32_t n = 0, strips = 0;
  uint32_t last = 0;  // n_act of the last block step
  int levels    = 0;  // max_level of the last start
  double dt     = 0.0;  // its s->dt
};

// Nothing is cleared: block_schedule_start and the start kernel of the integrator write lev, tau and the schedule words, and every
// block step writes the lists before it reads them.  mem: the owner of the part of the handle the schedule belongs to; on an error the
// caller releases it or destroys the handle.
inline hipError_t block_schedule_alloc(block_schedule* b, uint32_t n, device_buffers& mem) {
  b->n      = n;
  b->strips = uint32_t((size_t(n) + kSchedStrip - 1) / kSchedStrip);
  mem.alloc(&b->lev, sizeof(int32_t) * size_t(n));
  mem.alloc(&b->tau, sizeof(uint32_t) * size_t(n));
  mem.alloc(&b->act, sizeof(uint32_t) * size_t(n));
  mem.alloc(&b->bcount, sizeof(uint32_t) * b->strips);
  mem.alloc(&b->sched, sizeof(uint32_t) * kSchedWords);
  mem.alloc_pinned(&b->pin, sizeof(uint32_t) * 2, hipHostMallocMapped);
  hipError_t e = mem.error();
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&b->pin_dev), b->pin, 0);
  return e;
}

// mem: the owner block_schedule_alloc was given, with whatever else of that part it holds
inline void block_schedule_free(block_schedule* b, device_buffers& mem) {
  mem.release();
  *b = block_schedule{};
}

// the end of a start call, behind the integrator's kernel that writes lev and tau: the schedule words armed, the run's constants kept
inline int block_schedule_start(block_schedule* b, int L, double dt, hipStream_t st) {
  NB_HIP(hipMemsetAsync(b->sched, 0xff, sizeof(uint32_t) * kSchedWords, st));
  b->levels = L;
  b->dt     = dt;
  b->last   = 0;
  return NBODY_OK;
}

// count, scan, compact of the due bodies over one order into `out`; word: where tau_next is while `count` runs
inline int block_schedule_list(const block_schedule* b, const uint32_t* sidx, uint32_t* out, int word, bool publish, hipStream_t st) {
  const int32_t L = b->levels;
  hipLaunchKernelGGL(block_sched_count_kernel, dim3(b->strips), dim3(kSchedBlock), 0, st, b->lev, b->tau, sidx, b->sched, word, b->bcount,
                     b->n, L);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(block_sched_scan_kernel, dim3(1), dim3(kSchedBlock), 0, st, b->bcount, b->sched, b->pin_dev, b->strips, publish ? 1 : 0);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(block_sched_compact_kernel, dim3(b->strips), dim3(kSchedBlock), 0, st, b->lev, b->tau, sidx, b->sched, b->bcount, out,
                     b->n, L);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// the head of a block step: tau_next, then the active list in body order; (n_act, tau_next) go to the schedule words and to `pin`
inline int block_schedule_active(const block_schedule* b, hipStream_t st) {
  hipLaunchKernelGGL(block_sched_min_kernel, dim3(b->strips), dim3(kSchedBlock), 0, st, b->lev, b->tau, b->sched, b->n, int32_t(b->levels));
  NB_HIP(hipGetLastError());
  return block_schedule_list(b, nullptr, b->act, kSchedMin, true, st);
}

// The refusal of a step whose schedule cannot be this handle's.  api: "nbody_hermite", "nbody_hermite6" or "nbody_octree"; hint: the
// Hermite integrators name the likely cause.  The caller takes the handle out of its run of block steps.
inline int block_schedule_refuse(const block_schedule* b, const char* api, bool hint, uint32_t n_act, uint32_t next) {
  set_error("%s_block_step: the schedule on the device is not one of this handle (n_act = %u of %u, tau_next = %u of %u)%s%s%s", api,
            n_act, b->n, next, 1u << b->levels, hint ? ": were x, v, a rewritten without " : "", hint ? api : "",
            hint ? "_block_start?" : "");
  return NBODY_ERR_STATE;
}

// (n_act, tau_next) as the schedule published them, after the host has synchronised with the stream; refused unless
// 1 <= n_act <= n and 1 <= tau_next <= 2^L
inline int block_schedule_pair(const block_schedule* b, const char* api, bool hint, uint32_t* n_act, uint32_t* next) {
  *n_act = b->pin[0];
  *next  = b->pin[1];
  if (*n_act < 1u || *n_act > b->n || *next < 1u || *next > (1u << b->levels)) return block_schedule_refuse(b, api, hint, *n_act, *next);
  return NBODY_OK;
}

// what = 0 (levels), 1 (tau), 2 (the active list of the last block step): the array and its size in bytes
inline const void* block_schedule_array(const block_schedule* b, int what, size_t* bytes) {
  *bytes = 4 * size_t(what == 2 ? b->last : b->n);
  return what == 0 ? static_cast<const void*>(b->lev) : what == 1 ? static_cast<const void*>(b->tau) : b->act;
}

// The tail of nbody_<api>_block_read of the Hermite integrators, after the NULL checks and the range of `what`: refused while
// recording and unless `on` (the block start has run), then the copy-out.  type: "nbody_hermite" or "nbody_hermite6".
inline int block_schedule_read(const block_schedule* b, int device, bool on, const char* type, int what, void* host_out, size_t bytes,
                               hipStream_t st) {
  if (int r = check_same_device(device, st, type)) return r;
  device_guard guard(device);
  if (capture_id(st) != 0) {
    set_error("%s_block_read is blocking: it cannot be recorded (call it outside nbody_graph_begin/end)", type);
    return NBODY_ERR_STATE;
  }
  if (!on) {
    set_error("%s_block_read before %s_block_start on this handle", type, type);
    return NBODY_ERR_STATE;
  }
  size_t need;
  const void* src = block_schedule_array(b, what, &need);
  NB_ARG(bytes == need, "%s_block_read(what = %d) needs %zu bytes, got %zu", type, what, need, bytes);
  if (need) NB_HIP(hipMemcpyAsync(host_out, src, need, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}

// step (steps == nullptr): one block step; advance (steps: {block steps, body steps}): block steps until every body is at dtmax.
// step(&n_act, &tau_next) runs one block step and writes both on success.
template <typename Step>
inline int block_schedule_run(const block_schedule* b, Step&& step, uint32_t* n_active, uint32_t* tau, uint64_t* steps) {
  uint32_t na = 0, tn = 0;
  uint64_t nsteps = 0, nbody = 0;
  do {
    if (int r = step(&na, &tn)) return r;
    ++nsteps;
    nbody += na;
  } while (steps && tn != (1u << b->levels));
  if (n_active) *n_active = na;
  if (tau) *tau = tn;
  if (steps) {
    steps[0] = nsteps;
    steps[1] = nbody;
  }
  return NBODY_OK;
}

}  // namespace nbody
