// Block (individual) time steps for the Hermite integrator: nbody_hermite_block_* of include/nbody_hip.h.  Included by hermite.hip
// after struct nbody_hermite; the scheme (levels, ticks, the Aarseth criterion) is stated in the header.
//
// One block step is seven or eight launches on the caller's stream and one 8-byte read-back:
//   schedule   min        tau_next = min_i(tau_i + step_i): strips of kSStrip bodies, wave and block minimum, one atomicMin of an
//                         unsigned integer per block (a minimum does not depend on the order it is taken in);
//              count      active bodies (tau_i + step_i == tau_next) per strip;
//              scan       ONE block: exclusive scan of the strips' counts, n_act; publishes tau_next and re-arms the minimum;
//              compact    the active indices in ascending body order: the strip's offset + the counts of the earlier rows and
//                         waves of the strip + the lane's rank in its wave's ballot.  No atomics: a slot follows from the levels alone;
//   predict    ALL bodies to tau_next, h_i = T(tau_next - tau_i) * tick, the packed record of hermite_predict_kernel;
//   force+jerk the active targets, gathered through the list, against all N records: hermite_tile_sum (hermite_tile.hpp) as it is,
//              launched in the shape of hermite_block_plan_for(sz, n_act);
//   reduce     only where the active set is cut into more than kSerialChunks chunks (fewer than 2048 active bodies of a large system):
//              one wave per (slot, component) adds the chunks' sums, each lane a run of consecutive chunks in chunk order, the
//              runs in lane order — 2048 chunks added by one lane, as `correct` adds them, cost 1.1 ms at N = 2^20;
//   correct    one lane per active body: chunk sums in chunk order, the corrector with h = step_i * tick, the new level.
// `scan` writes (n_act, tau_next) into pinned host memory; the host synchronises after `predict` and sizes the last launches from it.

namespace nbody {

constexpr int kSItems      = 16;                  // rows of kHBlock bodies per schedule strip
constexpr uint32_t kSStrip = kHBlock * kSItems;   // 4096 bodies per schedule block
constexpr uint32_t kNoTime = 0xffffffffu;
constexpr uint32_t kSerialChunks = 64;  // up to here `correct` adds the chunks itself, one after the other (hermite_plan_for's most)

// sched[0]: the running minimum (kNoTime between steps), sched[1]: n_act, sched[2]: tau_next of the step in flight
enum { kSchedMin = 0, kSchedCount = 1, kSchedNext = 2, kSchedWords = 4 };

// Launch shape of the active-set force + jerk, from (sz, n_act) alone.  hermite_plan_for's rule with the blocks counted over the
// ACTIVE targets and no cap of 64 on the chunks: as n_act shrinks the tiles are cut finer over grid.y, down to one tile per chunk,
// so that about 2048 blocks are in flight whatever n_act is.  With n_act == sz it IS hermite_plan_for(sz, 1) (its cap of 64 binds
// below 2048 targets only, where a system has fewer than 8 tiles).
inline hermite_plan hermite_block_plan_for(uint32_t sz, uint32_t n_act) {
  hermite_plan p;
  p.R      = n_act >= 65536u ? 2u : 1u;
  p.blocks = (n_act + 64u * p.R - 1u) / (64u * p.R);
  p.ntiles = (sz + kHTile - 1u) / kHTile;
  uint32_t want = (2048u + p.blocks - 1u) / p.blocks;
  if (want > p.ntiles) want = p.ntiles;
  if (want < 1u) want = 1u;
  p.tiles_per_chunk = (p.ntiles + want - 1u) / want;
  p.chunks          = (p.ntiles + p.tiles_per_chunk - 1u) / p.tiles_per_chunk;
  return p;
}

// Slots (one slot = 2 D values) the partial sums of any n_act in [1, sz] can need: chunks * n_act.
// chunks <= ntiles gives ntiles * sz.  chunks <= ceil(2048 / blocks) and n_act <= 64 R blocks give
// chunks * n_act <= (2048 / blocks + 1) * 64 R blocks = 131072 R + 64 R blocks <= 262144 + n_act + 127.
// More than kSerialChunks chunks means fewer than 32 blocks, n_act < 2048: their reduced sums take 2048 slots behind the chunks'.
inline uint64_t hermite_block_part_slots(uint32_t sz) {
  const uint64_t a = uint64_t((sz + kHTile - 1u) / kHTile) * sz, b = 262144ull + sz + 128ull;
  return (a < b ? a : b) + 2048ull;
}

__device__ __forceinline__ uint32_t step_of(int32_t lev, int32_t L) { return 1u << (L - lev); }

// ---- schedule ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kHBlock) void hermite_sched_min_kernel(const int32_t* __restrict__ lev, const uint32_t* __restrict__ tau,
                                                                    uint32_t* __restrict__ sched, uint32_t n, int32_t L) {
  __shared__ uint32_t wmin[kHWaves];
  uint32_t mn = kNoTime;
#pragma unroll
  for (int k = 0; k < kSItems; ++k) {
    const uint32_t i = blockIdx.x * kSStrip + k * kHBlock + threadIdx.x;
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
    for (int w = 1; w < kHWaves; ++w) mn = wmin[w] < mn ? wmin[w] : mn;
    atomicMin(&sched[kSchedMin], mn);
  }
}

// the strip's rows one after the other, a ballot per wave: cnt[row * kHWaves + wave]
__device__ __forceinline__ bool sched_active(const int32_t* lev, const uint32_t* tau, uint32_t i, uint32_t n, int32_t L, uint32_t next) {
  return i < n && tau[i] + step_of(lev[i], L) == next;
}

__global__ __launch_bounds__(kHBlock) void hermite_sched_count_kernel(const int32_t* __restrict__ lev, const uint32_t* __restrict__ tau,
                                                                      const uint32_t* __restrict__ sched, uint32_t* __restrict__ bcount,
                                                                      uint32_t n, int32_t L) {
  __shared__ uint32_t wcnt[kHWaves];
  const uint32_t next = sched[kSchedMin];
  uint32_t c          = 0;
#pragma unroll
  for (int k = 0; k < kSItems; ++k) {
    const uint32_t i = blockIdx.x * kSStrip + k * kHBlock + threadIdx.x;
    c += uint32_t(__popcll(__ballot(sched_active(lev, tau, i, n, L, next))));
  }
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kHWaves; ++w) c += wcnt[w];
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

// one block: bcount[0 .. nb) -> its exclusive scan in place, the total to sched[kSchedCount] (and the host); tau_next moves to sched[kSchedNext]
// and the running minimum is re-armed for the next step (every reader of sched[kSchedMin] of this step has finished: stream order)
__global__ __launch_bounds__(kHBlock) void hermite_sched_scan_kernel(uint32_t* __restrict__ bcount, uint32_t* __restrict__ sched,
                                                                     uint32_t* __restrict__ host_pair, uint32_t nb) {
  __shared__ uint32_t wsum[kHWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t running = 0;
  for (uint32_t base = 0; base < nb; base += kHBlock) {
    const uint32_t j   = base + threadIdx.x;
    const uint32_t v   = j < nb ? bcount[j] : 0u;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    __syncthreads();  // the previous round's wsum has been read
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kHWaves; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (j < nb) bcount[j] = running + before + inc - v;
    running += total;
  }
  if (threadIdx.x == 0) {
    const uint32_t next = sched[kSchedMin];
    sched[kSchedCount]  = running;
    sched[kSchedNext]   = next;
    sched[kSchedMin]    = kNoTime;
    host_pair[0]        = running;  // pinned host memory: read by the host after it has synchronised with the stream
    host_pair[1]        = next;
  }
}

__global__ __launch_bounds__(kHBlock) void hermite_sched_compact_kernel(const int32_t* __restrict__ lev, const uint32_t* __restrict__ tau,
                                                                        const uint32_t* __restrict__ sched, const uint32_t* __restrict__ boff,
                                                                        uint32_t* __restrict__ act, uint32_t n, int32_t L) {
  __shared__ uint32_t cnt[kSItems * kHWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t next = sched[kSchedNext];
  uint64_t ballot[kSItems];
#pragma unroll
  for (int k = 0; k < kSItems; ++k) {
    const uint32_t i = blockIdx.x * kSStrip + k * kHBlock + threadIdx.x;
    ballot[k]        = __ballot(sched_active(lev, tau, i, n, L, next));
    if (lane == 0) cnt[k * kHWaves + wave] = uint32_t(__popcll(ballot[k]));
  }
  __syncthreads();
  if (wave == 0) {  // exclusive scan of the 64 (row, wave) counts, in body order
    const uint32_t v = cnt[lane];
    cnt[lane]        = wave_inclusive_scan(v, lane) - v;
  }
  __syncthreads();
  const uint32_t base = boff[blockIdx.x];
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < kSItems; ++k) {
    if ((ballot[k] >> lane) & 1ull) {
      const uint32_t slot = base + cnt[k * kHWaves + wave] + uint32_t(__popcll(ballot[k] & below));
      if (slot < n) act[slot] = blockIdx.x * kSStrip + k * kHBlock + threadIdx.x;  // slot < n always: n_act <= n
    }
  }
}

// ---- start: the first levels -----------------------------------------------------------------------------------------------------
// want = eta_start |a| / |j| (|j| = 0: level 0); the smallest level whose step dtmax 2^-l is <= want, at most L.  tau = 0.
template <typename T, int D>
__global__ __launch_bounds__(kHBlock) void hermite_block_init_kernel(const T* __restrict__ a, const T* __restrict__ jerk,
                                                                     int32_t* __restrict__ lev, uint32_t* __restrict__ tau, T eta_start,
                                                                     T dtmax, uint32_t n, int32_t L) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= n) return;
  T a2 = T(0), j2 = T(0);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const T ak = a[uint64_t(i) * D + k], jk = jerk[uint64_t(i) * D + k];
    a2 = __builtin_elementwise_fma(ak, ak, a2);
    j2 = __builtin_elementwise_fma(jk, jk, j2);
  }
  int32_t l = 0;
  if (j2 > T(0)) {
    const T want = eta_start * __builtin_elementwise_sqrt(a2) / __builtin_elementwise_sqrt(j2);
    T hs         = dtmax;
    while (l < L && hs > want) {
      hs *= T(0.5);
      ++l;
    }
  }
  lev[i] = l;
  tau[i] = 0u;
}

// ---- predict with per-body h -------------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ __launch_bounds__(kHBlock) void hermite_block_predict_kernel(const T* __restrict__ m, const T* __restrict__ x, const T* __restrict__ v,
                                                                        const T* __restrict__ a, const T* __restrict__ jerk,
                                                                        const uint32_t* __restrict__ tau, const uint32_t* __restrict__ sched,
                                                                        hsrc_rec<T>* __restrict__ recs, T tick, uint32_t n, uint32_t padded) {
  const uint32_t i = blockIdx.x * kHBlock + threadIdx.x;
  if (i >= padded) return;
  hsrc_rec<T> r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r.g[kRecP][k] = r.g[kRecV][k] = T(0);
  if (i < n) {
    const T dt = T(sched[kSchedNext] - tau[i]) * tick;
    r.g[kRecP][kRecM] = m[i];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const uint64_t e = uint64_t(i) * D + k;
      const T a0 = a[e], j0 = jerk[e], v0 = v[e];
      r.g[kRecP][k] =
          __builtin_elementwise_fma(dt, __builtin_elementwise_fma(dt * T(0.5), __builtin_elementwise_fma(dt * T(1.0 / 3.0), j0, a0), v0), x[e]);
      r.g[kRecV][k] = __builtin_elementwise_fma(dt, __builtin_elementwise_fma(dt * T(0.5), j0, a0), v0);
    }
  }
  recs[i] = r;
}

// ---- force + jerk of the active set ----------------------------------------------------------------------------------------------
// grid (blocks of 64 R active slots, chunks).  part: [chunk][2 D][n_act] raw sums over the slots.
template <typename T, int D, int R>
__global__ __launch_bounds__(kHBlock) void hermite_block_active_kernel(const hsrc_rec<T>* __restrict__ recs, T* __restrict__ part, T e2,
                                                                       uint32_t n_act, uint32_t ntiles, uint32_t tiles_per_chunk,
                                                                       const uint32_t* __restrict__ act) {
  hermite_tile_sum<T, D, R, 2, true>(reinterpret_cast<const T*>(recs), part, e2, n_act, ntiles, tiles_per_chunk, act);
}

// ---- chunk sums of a small active set ----------------------------------------------------------------------------------------------
// part [chunk][rows][n_act] -> out [rows][n_act], rows = 2 D.  One wave per (row, slot): lane l adds the chunks [l per_lane, (l + 1)
// per_lane) in chunk order, then the lanes' sums are added in lane order.  The order follows from `chunks` alone.
template <typename T>
__global__ __launch_bounds__(kHBlock) void hermite_block_reduce_kernel(const T* __restrict__ part, T* __restrict__ out, uint32_t n_act,
                                                                       uint32_t rows, uint32_t chunks, uint32_t per_lane) {
  const uint32_t w = blockIdx.x * kHWaves + (threadIdx.x >> 6);  // wave-uniform
  if (w >= rows * n_act) return;
  const uint32_t lane = threadIdx.x & 63, row = w / n_act, s = w - row * n_act;
  const uint32_t c0 = lane * per_lane, c1 = c0 + per_lane < chunks ? c0 + per_lane : chunks;
  T sum = T(0);
  if (c0 < chunks) {
    sum = part[(uint64_t(c0) * rows + row) * n_act + s];
    for (uint32_t ch = c0 + 1; ch < c1; ++ch) sum += part[(uint64_t(ch) * rows + row) * n_act + s];
  }
  const uint32_t runs = (chunks + per_lane - 1u) / per_lane;  // <= 64
  T total             = __shfl(sum, 0);
  for (uint32_t l = 1; l < runs; ++l) total += __shfl(sum, int(l));
  if (lane == 0) out[uint64_t(row) * n_act + s] = total;
}

// ---- correct + new level ---------------------------------------------------------------------------------------------------------
// hermite_correct_kernel's corrector with h = step_i * tick, then from a0, j0 (old) and a1, j1 (new)
//   a2 = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2,  a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3,  a2 <- a2 + h a3
//   want = sqrt(eta (|a1| |a2| + |j1|^2) / (|j1| |a3| + |a2|^2))       (denominator 0: no limit)
// 1 / h = 2^l / dtmax is idt * 2^l, an exact scaling of the host's idt = 1 / T(dtmax); the candidate steps h / 2, h / 4, ... are exact too.
template <typename T, int D>
__global__ __launch_bounds__(kHBlock) void hermite_block_correct_kernel(const T* __restrict__ part, const uint32_t* __restrict__ act,
                                                                        const uint32_t* __restrict__ sched, T* __restrict__ x, T* __restrict__ v,
                                                                        T* __restrict__ a, T* __restrict__ jerk, int32_t* __restrict__ lev,
                                                                        uint32_t* __restrict__ tau, T c, T tick, T idt, T eta, uint32_t n_act,
                                                                        uint32_t chunks, int32_t L) {
  const uint32_t s = blockIdx.x * kHBlock + threadIdx.x;
  if (s >= n_act) return;
  const uint32_t i    = act[s];
  const uint32_t next = sched[kSchedNext];
  const int32_t l     = lev[i];
  const uint32_t step = step_of(l, L);
  const T dt = T(step) * tick, ih = idt * T(1u << l);
  const T hdt = T(0.5) * dt, dt12 = (dt * dt) * T(1.0 / 12.0), ih2 = ih * ih, ih3 = ih2 * ih;
  T n_a1 = T(0), n_j1 = T(0), n_a2 = T(0), n_a3 = T(0);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    T sa = part[uint64_t(k) * n_act + s], sj = part[uint64_t(D + k) * n_act + s];
    for (uint32_t ch = 1; ch < chunks; ++ch) {
      sa += part[(uint64_t(ch) * (2 * D) + k) * n_act + s];
      sj += part[(uint64_t(ch) * (2 * D) + D + k) * n_act + s];
    }
    const T a1 = c * sa, j1 = c * sj;
    const uint64_t e = uint64_t(i) * D + k;
    const T a0 = a[e], j0 = jerk[e], v0 = v[e];
    const T v1 = v0 + __builtin_elementwise_fma(hdt, a0 + a1, dt12 * (j0 - j1));
    x[e]       = x[e] + __builtin_elementwise_fma(hdt, v0 + v1, dt12 * (a0 - a1));
    v[e]       = v1;
    a[e]       = a1;
    jerk[e]    = j1;
    const T da = a0 - a1;
    const T a3 = (T(12) * da + T(6) * dt * (j0 + j1)) * ih3;
    const T a2 = (T(-6) * da - dt * (T(4) * j0 + T(2) * j1)) * ih2 + dt * a3;
    n_a1 = __builtin_elementwise_fma(a1, a1, n_a1);
    n_j1 = __builtin_elementwise_fma(j1, j1, n_j1);
    n_a2 = __builtin_elementwise_fma(a2, a2, n_a2);
    n_a3 = __builtin_elementwise_fma(a3, a3, n_a3);
  }
  // |j1|^2 and |a2|^2 are the sums themselves
  const T num = __builtin_elementwise_fma(__builtin_elementwise_sqrt(n_a1), __builtin_elementwise_sqrt(n_a2), n_j1);
  const T den = __builtin_elementwise_fma(__builtin_elementwise_sqrt(n_j1), __builtin_elementwise_sqrt(n_a3), n_a2);
  int32_t nl  = l;
  if (den > T(0)) {
    const T want = __builtin_elementwise_sqrt(eta * num / den);
    if (want < dt) {  // the smallest level deeper than l whose step is <= want, at most L
      T hs = hdt;
      nl   = l + 1;
      while (nl < L && hs > want) {
        hs *= T(0.5);
        ++nl;
      }
      if (nl > L) nl = L;
    } else if (want >= T(2) * dt && l > 0 && (next & (2u * step - 1u)) == 0u) {
      nl = l - 1;  // one doubling at most, and only onto the coarser level's grid
    }
  } else if (l > 0 && (next & (2u * step - 1u)) == 0u) {
    nl = l - 1;  // no limit
  }
  lev[i] = nl;
  tau[i] = next == (1u << L) ? 0u : next;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
inline void hermite_block_free(nbody_hermite* h) {
  (void)hipFree(h->blev);
  (void)hipFree(h->btau);
  (void)hipFree(h->bact);
  (void)hipFree(h->bcount);
  (void)hipFree(h->bsched);
  (void)hipFree(h->bpart);
  if (h->bpin) (void)hipHostFree(h->bpin);
  h->blev = nullptr;
  h->btau = h->bact = h->bcount = h->bsched = h->bpin = h->bpin_dev = nullptr;
  h->bpart = nullptr;
}

static int hermite_block_alloc(nbody_hermite* h) {
  if (h->bpin) return NBODY_OK;
  const size_t n  = h->n;
  h->bstrips      = uint32_t((n + kSStrip - 1) / kSStrip);
  h->bslots       = hermite_block_part_slots(h->n);
  hipError_t e    = hipMalloc(reinterpret_cast<void**>(&h->blev), sizeof(int32_t) * n);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->btau), sizeof(uint32_t) * n);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->bact), sizeof(uint32_t) * n);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->bcount), sizeof(uint32_t) * h->bstrips);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->bsched), sizeof(uint32_t) * kSchedWords);
  if (e == hipSuccess) e = hipMalloc(&h->bpart, h->tsz * 2 * size_t(h->dim) * size_t(h->bslots));
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&h->bpin), sizeof(uint32_t) * 2, hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&h->bpin_dev), h->bpin, 0);
  if (e != hipSuccess) {
    hermite_block_free(h);
    return hip_fail(e, "nbody_hermite_block_start allocation", __FILE__, __LINE__);
  }
  return NBODY_OK;
}

template <typename T>
struct block_consts {
  T e2, eta, tick, dtmax, idt;
};

// The common head of block_start and block_step: every argument error before the device is touched, in the header's order; then the
// two call-sequence refusals.  A step takes the level count of the handle, not max_level.
template <typename T>
static int hermite_block_check(nbody_hermite* h, const nbody_state* s, double eps, double eta, bool is_start, int max_level,
                               hipStream_t st, const char* who, block_consts<T>* out) {
  const char* eta_name = is_start ? "eta_start" : "eta";
  if (int r = check_softening<T>(eps, &out->e2)) return r;
  NB_ARG(eta > 0.0 && eta <= DBL_MAX && T(eta) > T(0), "%s: %s = %g must be finite and > 0", who, eta_name, eta);
  if (is_start) NB_ARG(max_level >= 0 && max_level <= 20, "%s: max_level = %d must be in 0 .. 20", who, max_level);
  NB_ARG(h != nullptr, "nbody_hermite is NULL");
  NB_ARG(h->dtype == s->dtype && h->dim == s->dim && h->n == s->sz,
         "nbody_hermite was created for (dtype %d, dim %d, n %u), the state is (dtype %d, dim %d, sz %u)", h->dtype, h->dim, h->n,
         s->dtype, s->dim, s->sz);
  const int L = is_start ? max_level : h->blevels;
  out->eta    = T(eta);
  out->dtmax  = T(s->dt);
  out->tick   = out->dtmax;
  for (int k = 0; k < L; ++k) out->tick *= T(0.5);
  out->idt = T(1) / out->dtmax;
  NB_ARG(s->dt > 0.0 && s->dt <= DBL_MAX && out->tick >= (sizeof(T) == 4 ? T(FLT_MIN) : T(DBL_MIN)) && out->idt > T(0) &&
             out->idt <= (sizeof(T) == 4 ? T(FLT_MAX) : T(DBL_MAX)),
         "%s: dt = %g must be finite and > 0, and dt / 2^%d and 1 / dt normal numbers", who, s->dt, L);
  if (int r = check_same_device(h->device, st, "nbody_hermite")) return r;
  if (capture_id(st) != 0 || (is_start && captures_on_this_thread() != 0)) {
    set_error("%s %s: it cannot be called between nbody_graph_begin and nbody_graph_end", who,
              is_start ? "allocates on first use" : "is blocking (it reads the size of the active set back)");
    return NBODY_ERR_STATE;
  }
  if (!is_start) {
    if (!h->block_on) {
      set_error("%s before nbody_hermite_block_start on this handle (or after a later nbody_hermite_force_jerk)", who);
      return NBODY_ERR_STATE;
    }
    NB_ARG(s->dt == h->bdt, "%s: the state's dt = %g is not the dt = %g nbody_hermite_block_start was called with", who, s->dt, h->bdt);
  }
  return NBODY_OK;
}

template <typename T, int D>
static int hermite_block_start_launch(nbody_hermite* h, const nbody_state* s, const block_consts<T>& bc, T eta_start, int L, hipStream_t st) {
  if (int r = hermite_block_alloc(h)) return r;
  const int r = h->plan.R == 2 ? hermite_launch<T, D, 2, true>(h, s, bc.e2, st) : hermite_launch<T, D, 1, true>(h, s, bc.e2, st);
  if (r != NBODY_OK) return r;
  h->started = true;
  hipLaunchKernelGGL((hermite_block_init_kernel<T, D>), dim3((h->n + kHBlock - 1) / kHBlock), dim3(kHBlock), 0, st,
                     static_cast<const T*>(s->a), static_cast<const T*>(h->jerk), h->blev, h->btau, eta_start, bc.dtmax, h->n, int32_t(L));
  NB_HIP(hipGetLastError());
  NB_HIP(hipMemsetAsync(h->bsched, 0xff, sizeof(uint32_t) * kSchedWords, st));
  h->blevels  = L;
  h->bdt      = s->dt;
  h->blast    = 0;
  h->block_on = true;
  return NBODY_OK;
}

// one block step; *n_active and *tau_next are always written on success
template <typename T, int D>
static int hermite_block_step_launch(nbody_hermite* h, const nbody_state* s, const block_consts<T>& bc, hipStream_t st, uint32_t* n_active,
                                     uint32_t* tau_next) {
  const int32_t L = h->blevels;
  const uint32_t n = h->n;
  T* jerk = static_cast<T*>(h->jerk);
  auto* recs = static_cast<hsrc_rec<T>*>(h->recs);
  T* part    = static_cast<T*>(h->bpart);
  hipLaunchKernelGGL(hermite_sched_min_kernel, dim3(h->bstrips), dim3(kHBlock), 0, st, h->blev, h->btau, h->bsched, n, L);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(hermite_sched_count_kernel, dim3(h->bstrips), dim3(kHBlock), 0, st, h->blev, h->btau, h->bsched, h->bcount, n, L);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(hermite_sched_scan_kernel, dim3(1), dim3(kHBlock), 0, st, h->bcount, h->bsched, h->bpin_dev, h->bstrips);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL(hermite_sched_compact_kernel, dim3(h->bstrips), dim3(kHBlock), 0, st, h->blev, h->btau, h->bsched, h->bcount, h->bact, n, L);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((hermite_block_predict_kernel<T, D>), dim3(h->padded / kHBlock), dim3(kHBlock), 0, st, static_cast<const T*>(s->m),
                     static_cast<const T*>(s->x), static_cast<const T*>(s->v), static_cast<const T*>(s->a), jerk, h->btau, h->bsched, recs,
                     bc.tick, n, h->padded);
  NB_HIP(hipGetLastError());
  NB_HIP(hipStreamSynchronize(st));
  const uint32_t n_act = h->bpin[0], next = h->bpin[1];
  const hermite_plan p = hermite_block_plan_for(n, n_act ? n_act : 1u);
  const bool reduce = p.chunks > kSerialChunks;
  if (n_act < 1u || n_act > n || next < 1u || next > (1u << L) || uint64_t(p.chunks) * n_act + (reduce ? n_act : 0u) > h->bslots) {
    h->block_on = false;
    set_error("nbody_hermite_block_step: the schedule on the device is not one of this handle (n_act = %u of %u, tau_next = %u of %u): "
              "were x, v, a rewritten without nbody_hermite_block_start?", n_act, n, next, 1u << L);
    return NBODY_ERR_STATE;
  }
  if (p.R == 2)
    hipLaunchKernelGGL((hermite_block_active_kernel<T, D, 2>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part, bc.e2, n_act,
                       p.ntiles, p.tiles_per_chunk, h->bact);
  else
    hipLaunchKernelGGL((hermite_block_active_kernel<T, D, 1>), dim3(p.blocks, p.chunks), dim3(kHBlock), 0, st, recs, part, bc.e2, n_act,
                       p.ntiles, p.tiles_per_chunk, h->bact);
  NB_HIP(hipGetLastError());
  uint32_t chunks = p.chunks;
  if (reduce) {
    T* out = part + uint64_t(p.chunks) * (2 * D) * n_act;
    hipLaunchKernelGGL((hermite_block_reduce_kernel<T>), dim3((2 * D * n_act + kHWaves - 1) / kHWaves), dim3(kHBlock), 0, st, part, out, n_act,
                       uint32_t(2 * D), p.chunks, (p.chunks + 63u) / 64u);
    NB_HIP(hipGetLastError());
    part   = out;
    chunks = 1;
  }
  hipLaunchKernelGGL((hermite_block_correct_kernel<T, D>), dim3((n_act + kHBlock - 1) / kHBlock), dim3(kHBlock), 0, st, part, h->bact,
                     h->bsched, static_cast<T*>(s->x), static_cast<T*>(s->v), static_cast<T*>(s->a), jerk, h->blev, h->btau,
                     static_cast<T>(s->c), bc.tick, bc.idt, bc.eta, n_act, chunks, L);
  NB_HIP(hipGetLastError());
  h->blast  = n_act;
  *n_active = n_act;
  *tau_next = next;
  return NBODY_OK;
}

// block_start (is_start) | block_step (steps == nullptr) | block_advance (steps: {block steps, body steps})
static int hermite_block_call(nbody_hermite* h, const nbody_state* s, double eps, double eta, bool is_start, int max_level, void* stream,
                              const char* who, uint32_t* n_active, uint32_t* tau, uint64_t* steps) {
  if (int r = check_state(s)) return r;
  NB_ARG(s->first == 0 && s->count == s->sz, "%s needs the whole system (first = 0, count = sz), got [%u, %u+%u) of %u", who, s->first,
         s->first, s->count, s->sz);
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    block_consts<T> bc;
    hipStream_t st = as_stream(stream);
    if (int r = hermite_block_check<T>(h, s, eps, eta, is_start, max_level, st, who, &bc)) return r;
    device_guard guard(h->device);
    if (is_start) return hermite_block_start_launch<T, D>(h, s, bc, T(eta), max_level, st);
    uint32_t na = 0, tn = 0;
    uint64_t nsteps = 0, nbody = 0;
    do {
      if (int r = hermite_block_step_launch<T, D>(h, s, bc, st, &na, &tn)) return r;
      ++nsteps;
      nbody += na;
    } while (steps && tn != (1u << h->blevels));
    if (n_active) *n_active = na;
    if (tau) *tau = tn;
    if (steps) {
      steps[0] = nsteps;
      steps[1] = nbody;
    }
    return int(NBODY_OK);
  });
}

}  // namespace nbody

extern "C" int nbody_hermite_block_start(nbody_hermite* h, const nbody_state* s, double eps, double eta_start, int max_level, void* stream) {
  return nbody::hermite_block_call(h, s, eps, eta_start, true, max_level, stream, "nbody_hermite_block_start", nullptr, nullptr, nullptr);
}

extern "C" int nbody_hermite_block_step(nbody_hermite* h, const nbody_state* s, double eps, double eta, void* stream, uint32_t* n_active,
                                        uint32_t* tau) {
  return nbody::hermite_block_call(h, s, eps, eta, false, 0, stream, "nbody_hermite_block_step", n_active, tau, nullptr);
}

extern "C" int nbody_hermite_block_advance(nbody_hermite* h, const nbody_state* s, double eps, double eta, void* stream, uint64_t* block_steps,
                                           uint64_t* body_steps) {
  uint64_t steps[2] = {0, 0};
  const int r = nbody::hermite_block_call(h, s, eps, eta, false, 0, stream, "nbody_hermite_block_advance", nullptr, nullptr, steps);
  if (r == NBODY_OK) {
    if (block_steps) *block_steps = steps[0];
    if (body_steps) *body_steps = steps[1];
  }
  return r;
}

extern "C" int nbody_hermite_block_read(nbody_hermite* h, int what, void* host_out, size_t bytes, void* stream) {
  NB_ARG(h != nullptr, "nbody_hermite is NULL");
  NB_ARG(host_out != nullptr, "host_out is NULL");
  NB_ARG(what >= 0 && what <= 2, "what must be 0 (levels), 1 (tau) or 2 (the active list of the last block step), got %d", what);
  if (int r = check_same_device(h->device, as_stream(stream), "nbody_hermite")) return r;
  device_guard guard(h->device);
  hipStream_t st = as_stream(stream);
  if (capture_id(st) != 0) {
    set_error("nbody_hermite_block_read is blocking: it cannot be recorded (call it outside nbody_graph_begin/end)");
    return NBODY_ERR_STATE;
  }
  if (!h->block_on) {
    set_error("nbody_hermite_block_read before nbody_hermite_block_start on this handle");
    return NBODY_ERR_STATE;
  }
  const size_t need = 4 * size_t(what == 2 ? h->blast : h->n);
  NB_ARG(bytes == need, "nbody_hermite_block_read(what = %d) needs %zu bytes, got %zu", what, need, bytes);
  const void* src = what == 0 ? static_cast<const void*>(h->blev) : what == 1 ? static_cast<const void*>(h->btau) : h->bact;
  if (need) NB_HIP(hipMemcpyAsync(host_out, src, need, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  return NBODY_OK;
}
