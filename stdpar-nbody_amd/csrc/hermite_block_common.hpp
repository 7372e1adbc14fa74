// What the block time steps of the two Hermite integrators (hermite_block.inc: order 4, hermite6_block.inc: order 6) share beyond the
// schedule of block_schedule.hpp: the launch shape (hermite_block_plan.hpp), the block-step part of the two handles, the kernel that
// gives the first levels and the kernel that adds the chunks' sums of a small active set.  G is hermite_tile.hpp's: 2 or 3.
#pragma once
#include "block_schedule.hpp"
#include "hermite_block_plan.hpp"

namespace nbody {

// ---- start: the first levels -----------------------------------------------------------------------------------------------------
// want = eta_start |a| / |j| (|j| = 0: level 0); the smallest level whose step dtmax 2^-l is <= want, at most L.  tau = 0.
template <typename T, int D>
static __global__ __launch_bounds__(kHBlock) void hermite_block_init_kernel(const T* __restrict__ a, const T* __restrict__ jerk,
                                                                            int32_t* __restrict__ lev, uint32_t* __restrict__ tau,
                                                                            T eta_start, T dtmax, uint32_t n, int32_t L) {
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
  if (j2 > T(0)) l = block_first_level(eta_start * __builtin_elementwise_sqrt(a2) / __builtin_elementwise_sqrt(j2), dtmax, L);
  lev[i] = l;
  tau[i] = 0u;
}

// ---- chunk sums of a small active set ----------------------------------------------------------------------------------------------
// part [chunk][rows][n_act] -> out [rows][n_act], rows = G D.  One wave per (row, slot): lane l adds the chunks [l per_lane, (l + 1)
// per_lane) in chunk order, then the lanes' sums are added in lane order.  The order follows from `chunks` alone.  (2048 chunks
// added by one lane, as `correct` adds them, cost 1.1 ms at N = 2^20.)
template <typename T>
static __global__ __launch_bounds__(kHBlock) void hermite_block_reduce_kernel(const T* __restrict__ part, T* __restrict__ out, uint32_t n_act,
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

// ---- host ----------------------------------------------------------------------------------------------------------------------
// The block-step part of struct nbody_hermite and struct nbody_hermite6: allocated by the first block start of the handle.
struct hermite_block {
  block_schedule sched;
  void* bpart     = nullptr;  // T[bslots][G D]: partial sums of the active set, sized for the worst n_act
  uint64_t bslots = 0;
  bool block_on   = false;  // the block start has run and no fixed-step start since
  device_buffers mem;       // owns bpart and the schedule's arrays: a part of its own, apart from the handle's
};

inline void hermite_block_free(hermite_block* b) {
  block_schedule_free(&b->sched, b->mem);
  b->bpart = nullptr;
}

// what: "nbody_hermite_block_start allocation" or its sixth-order twin, for the error
inline int hermite_block_alloc(hermite_block* b, const hermite_handle* h, int G, uint32_t min_chunks, const char* what) {
  if (b->sched.pin) return NBODY_OK;
  b->bslots = hermite_block_part_slots(h->n, min_chunks);
  b->mem.alloc(&b->bpart, h->tsz * G * size_t(h->dim) * size_t(b->bslots));
  const hipError_t e = block_schedule_alloc(&b->sched, h->n, b->mem);
  if (e != hipSuccess) {
    hermite_block_free(b);
    return hip_fail(e, what, __FILE__, __LINE__);
  }
  return NBODY_OK;
}

// The launch shape of a block step's pair sum from what the schedule published, and whether its chunks go through
// hermite_block_reduce_kernel; refused (with the handle taken out of its run of block steps) unless (n_act, tau_next) and the partial
// sums' slots can be this handle's.  type: "nbody_hermite" or "nbody_hermite6".
inline int hermite_block_shape(hermite_block* b, const char* type, uint32_t min_chunks, uint32_t* n_act, uint32_t* next, hermite_plan* p,
                               bool* reduce) {
  int r = block_schedule_pair(&b->sched, type, true, n_act, next);
  if (r == NBODY_OK) {
    *p      = hermite_block_plan_for(b->sched.n, *n_act, min_chunks);
    *reduce = p->chunks > kSerialChunks;
    if (uint64_t(p->chunks) * *n_act + (*reduce ? *n_act : 0u) > b->bslots) r = block_schedule_refuse(&b->sched, type, true, *n_act, *next);
  }
  if (r != NBODY_OK) b->block_on = false;
  return r;
}

// nbody_<type>_block_read
inline int hermite_block_read(const hermite_handle* h, const hermite_block* b, const char* type, int what, void* host_out, size_t bytes,
                              void* stream) {
  NB_ARG(h != nullptr, "%s is NULL", type);
  NB_ARG(host_out != nullptr, "host_out is NULL");
  NB_ARG(what >= 0 && what <= 2, "what must be 0 (levels), 1 (tau) or 2 (the active list of the last block step), got %d", what);
  return block_schedule_read(&b->sched, h->device, b->block_on, type, what, host_out, bytes, as_stream(stream));
}

}  // namespace nbody
