// K1 all-pairs force, K2 all-pairs-collapsed force, K3 leapfrog step — hand-written for gfx950.
//
// K1 (replaces src/all_pairs.h:14-27).  Bound: FP64/FP32 VALU issue (no MFMA: the inner body is
// sub/FMA/rsq, not a contraction).  Structure:
//   * one lane per target body (R targets per lane), targets of a block held in VGPRs;
//   * sources are packed (x, m) records visited in tiles of 512; every tile is cut into JS slices, one per wave of the
//     block that shares a target group, and the tile sequence into source chunks over grid.y — both from sz alone, so a
//     shard window (N/8 targets on one GPU) sums exactly as the whole system does and still fills the chip;
//   * slice partials are combined through LDS in wave order, chunk sums added in chunk order — c * (((s_0 + s_1) + s_2) + ...) — by
//     the chunks' blocks themselves: passed from block to block in `a` (a turn word per target group; a failure is loud: k1_status), or,
//     where the whole grid is resident at once (<= 2048 blocks), collected by whichever chunk arrives last.  Deterministic, the same
//     bits either way, and independent of how bodies are sharded over GPUs.
//   Two ways of bringing a source record to the 64 lanes that all need the same one (bitwise the same result):
//   - LDS tiles (all_pairs_force_kernel): tiles staged in LDS by all 256 lanes with a register prefetch of the
//     next tile; the inner loop reads each record as an LDS broadcast (ds_read_b128) into VGPRs;
//   - scalar stream (all_pairs_force_sgpr_kernel, default from 2048 bodies): the record is wave-uniform, so it belongs in
//     SGPRs: ONE pre-pass launch per call (k1_prepare_kernel) packs the records (32 B x N; in f64 also the sources' pair constants
//     M15 = 1.5 m, M1875 = 1.875 m, 16 B x N), sums the positions' moments for the pair rule and resets the turn words; every wave
//     streams its slice with s_load_dwordx16 two batches deep (inline asm) and the VALU instructions take their source operands
//     from SGPRs — in f64 all but M15, which a wave-uniform global_load_dwordx4 per batch puts into VGPRs without a VALU
//     instruction (a VOP3 instruction reads one scalar value; common.hpp: weight_far_folded, cload).  No staging loads, no LDS
//     traffic, no barriers in the loop, half the VGPRs.
//   Pair rule (common.hpp, pair_batch): f64 is reciprocal-free with the source's mass folded into the polynomial — 15 full-rate
//   ops + v_rsq_f64 per pair on sparse systems (the launch-level far mode: the positions' variances, common.hpp k1_rule, say that
//   few batches can hold a pair closer than 2), 16 + 1 on dense ones; pairs below 2^-16 take the guarded reciprocal form.
//   Measured: N = 2^20 galaxy 602-633 ms per pass by the clock the box sustains = 44-46.5 % of the 78.6 TF FP64 vector peak with
//   the 16 + rsq form (profiles/r05/bench_n1.json; VALU 98 % busy: 97 % of what 16 + rsq allow); the folded form against it,
//   alternating on one box: profiles/r07/time_folded_weight.txt.
//   Space order (f64 scalar stream from 262 144 bodies on; see k1_order_wanted below): the packed sources and the window's targets
//   are sorted by a Morton key of their cells before K1 runs, so that source chunks and target groups are compact in space and
//   most blocks take the far certificate; K1 itself is the same code.  profiles/r09/time_space_order.txt.
//
// K2 (replaces src/all_pairs.h:29-50, intended semantics).  Lanes run along the SOURCE axis (one
// ordered pair per lane and step), each wave owns 64 targets whose positions it broadcasts with
// v_readlane; the partial sums of 16 (f32) / 8 (f64) targets stay in registers over a whole 2048- / 1024-record tile and are
// reduced together by a transposed DPP butterfly (transpose_reduce), lane t keeps target t's sum, and after its tiles each
// wave issues D coalesced atomic adds.  grid.y splits the source range so small N still fills the chip.
// Config 3 (f32, N = 262 144): 23.9 ms = 36.5 % of the FP32 vector peak.
//
// K3 (replaces src/system.h:52-60).  Pure HBM stream (7*D*sizeof(T) bytes/body), flat elementwise
// over count*D scalars, FP contraction off so it is bit-identical to the reference's x86 -O2 build.
#include "common.hpp"
#include "k1_order_key.hpp"
#include "radix_sort.hpp"

#include <atomic>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <vector>

namespace nbody {

constexpr int kBlock = 256;  // 4 waves
constexpr int kWaves = kBlock / 64;

struct ap_config {
  int split = 0;  // 0 = auto
  int tpt   = 0;  // targets per thread, 0 = auto
  int path  = 0;  // source path: 0 = auto (scalar stream), 1 = LDS tiles, 2 = scalar stream
};
// process-wide default in NBODY_TUNING encoding (0 = all auto); a view with a non-zero `tuning` overrides it
static std::atomic<uint32_t> g_ap_default{0};

static ap_config ap_config_of(const nbody_state* s) {
  const uint32_t t = s->tuning ? s->tuning : g_ap_default.load(std::memory_order_relaxed);
  ap_config c;
  c.split = int(t & 15u);
  c.tpt   = int((t >> 4) & 3u);
  c.path  = int((t >> 6) & 3u);
  return c;
}

// ------------------------------------------------------------------------------------------------
// K1
// ------------------------------------------------------------------------------------------------
template <typename T, int D, int R, int JS>
__global__ __launch_bounds__(kBlock) void all_pairs_force_kernel(const T* __restrict__ m, const T* __restrict__ x,
                                                                 T* __restrict__ a, T c, uint32_t sz, uint32_t first,
                                                                 uint32_t count, const k1_rule* __restrict__ rule) {
  [[maybe_unused]] constexpr T e2 = T(0);
#define K1_SOFT false
#include "k1_tile_body.inc"
#undef K1_SOFT
}
template <typename T, int D, int R, int JS>
__global__ __launch_bounds__(kBlock) void all_pairs_softened_kernel(const T* __restrict__ m, const T* __restrict__ x,
                                                                    T* __restrict__ a, T c, uint32_t sz, uint32_t first,
                                                                    uint32_t count, T e2) {
  const k1_rule* const rule = nullptr;
#define K1_SOFT true
#include "k1_tile_body.inc"
#undef K1_SOFT
}

// Scalar-stream form: pre-pass that packs (x, m) into aligned records, zero-mass padding up to a whole tile.
// (Measured and not kept, round 4: laying the records out in the order a wave reads them — one contiguous run per (chunk, slice),
// so that the stream's next address is `+ 64 bytes` instead of ten scalar operations on the record number.  Bitwise the same
// results, half the scalar instructions in the loop, and SLOWER: f32 N = 262 144 21.8 -> 22.5 ms dense, 19.3 -> 19.7 sparse — the
// eight slices' streams of a block then start 128 KB apart and fall into the same sets of the 16 KB scalar cache.)
template <typename T, int D>
__global__ __launch_bounds__(kBlock) void pack_sources_kernel(const T* __restrict__ m, const T* __restrict__ x,
                                                              src_rec<T, D>* __restrict__ out, uint32_t sz, uint32_t padded) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= padded) return;
  src_rec<T, D> r;
#pragma unroll
  for (int k = 0; k < 3; ++k) r.p[k] = (k < D && j < sz) ? x[uint64_t(j) * D + (k < D ? k : 0)] : T(0);
  r.m    = j < sz ? m[j] : T(0);
  out[j] = r;
}

// What a K1 launch needs done first, in ONE launch (rounds 2-4: a memset, the extent kernel, the pack kernel and another memset —
// four dependent launches, 20 us of a 73 us call at n = 8192):
//   PACK     the (x, m) records of the scalar-stream form, as pack_sources_kernel above, and in f64 the sources' constants
//            M15 = 1.5 m and M1875 = 1.875 m of K1's pair form beside them (common.hpp: src_cst, cst_batch; 16 bytes per source);
//   MOMENTS  the first and second moments of all sz positions, relative to body 0 (so that a system far from the origin does not
//            cancel), summed per block in a fixed order; the LAST block to deliver (a ticket) adds the blocks' sums in index order
//            and writes the rule (common.hpp: k1_rule) — the same bits whichever block comes last;
//   BOX      (f64 with PACK and MOMENTS, where the launch asks for it: bpc != 0) the bounding box of every source chunk of the
//            launch, for K1's far certificate (common.hpp: k1_block_is_far).  A chunk is a whole number of prepare blocks (bpc of
//            them), so every block stores the box of its 256 records — padding records, at the origin, included; the whole line
//            on every axis if one of them is not finite, so that nothing K1 compares with such a chunk certifies — and the last
//            block reduces each chunk's boxes.  Min and max are order-free: the same bits on every rank, whatever the order;
//   and the last block also hands the turn of every target group back to chunk 0 (the words K1's chunks pass around).
// One block per 256 bodies of the padded set; the ticket returns to 0, so a recorded launch can be replayed.
// The kernel's last argument.  Only f64 has boxes, and the f32 kernels keep the argument block (and so the code) they had.
template <typename T>
struct k1_prepare_tail {
  uint32_t turn_words;
};
template <>
struct k1_prepare_tail<double> {
  uint32_t turn_words;
  uint32_t bpc;   // prepare blocks per source chunk; 0: no boxes
  double* cbox;   // [chunk][lo[D], hi[D]]
  double* pbox;   // the same per prepare block
};
template <typename T, int D, bool PACK, bool MOMENTS>
__global__ __launch_bounds__(kBlock) void k1_prepare_kernel(const T* __restrict__ m, const T* __restrict__ x, src_rec<T, D>* __restrict__ out,
                                                            cst_batch* __restrict__ cst, uint32_t sz, uint32_t padded, k1_rule* rule, double* partial,
                                                            uint32_t* turn, k1_prepare_tail<T> tail) {
  constexpr bool BOX        = PACK && MOMENTS && sizeof(T) == 8;
  const uint32_t turn_words = tail.turn_words;
  [[maybe_unused]] uint32_t bpc = 0;
  [[maybe_unused]] T *cbox = nullptr, *pbox = nullptr;
  if constexpr (BOX) bpc = tail.bpc, cbox = tail.cbox, pbox = tail.pbox;
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  T p[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = j < sz ? x[uint64_t(j) * D + k] : T(0);
  if constexpr (PACK) {
    if (j < padded) {
      src_rec<T, D> r;
#pragma unroll
      for (int k = 0; k < 3; ++k) r.p[k] = k < D ? p[k < D ? k : 0] : T(0);
      r.m    = j < sz ? m[j] : T(0);
      out[j] = r;
      if constexpr (sizeof(T) == 8) {  // (a zero-mass padding record: constants 0)
        const src_cst<T> k  = src_cst<T>::of(r.m);
        cst[j / 2].m15[j % 2]   = k.m15;
        cst[j / 2].m1875[j % 2] = k.m1875;
      }
    }
  }
  __shared__ double red[2 * D][kWaves];
  __shared__ T bred[BOX ? 2 * D : 1][kWaves];
  __shared__ bool last_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if constexpr (MOMENTS) {
    double s1[D], s2[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double d = j < sz ? double(p[k]) - double(x[k]) : 0.0;  // relative to body 0 (sz >= 1)
      s1[k] = d;
      s2[k] = d * d;
    }
#pragma unroll
    for (int k = 0; k < D; ++k)
      for (int off = 32; off > 0; off >>= 1) {  // butterfly: every lane ends with the same sum, formed in the same order
        s1[k] += __shfl_xor(s1[k], off, 64);
        s2[k] += __shfl_xor(s2[k], off, 64);
      }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < D; ++k) {
        red[k][wave]     = s1[k];
        red[D + k][wave] = s2[k];
      }
    }
    if constexpr (BOX) {
      if (bpc != 0) {  // the box of this block's records as they are packed: p is 0 for a padding record
        bool finite = true;
#pragma unroll
        for (int k = 0; k < D; ++k) finite = finite && (p[k] - p[k]) == T(0);
        T lo[D], hi[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
          lo[k] = finite ? p[k] : -T(__builtin_inf());
          hi[k] = finite ? p[k] : T(__builtin_inf());
        }
#pragma unroll
        for (int k = 0; k < D; ++k)
          for (int off = 32; off > 0; off >>= 1) {
            lo[k] = __builtin_fmin(lo[k], __shfl_xor(lo[k], off, 64));
            hi[k] = __builtin_fmax(hi[k], __shfl_xor(hi[k], off, 64));
          }
        if (lane == 0) {
#pragma unroll
          for (int k = 0; k < D; ++k) {
            bred[k][wave]     = lo[k];
            bred[D + k][wave] = hi[k];
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < 2 * D) {
      double v = red[threadIdx.x][0];
      for (int w = 1; w < kWaves; ++w) v += red[threadIdx.x][w];
      __hip_atomic_store(partial + size_t(blockIdx.x) * (2 * D) + threadIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (BOX) {
      if (bpc != 0 && threadIdx.x >= 64 && threadIdx.x < 64 + 2 * D) {  // (wave 1: wave 0 stores the moments)
        const int q = int(threadIdx.x) - 64;
        T v         = bred[q][0];
        for (int w = 1; w < kWaves; ++w) v = q < D ? __builtin_fmin(v, bred[q][w]) : __builtin_fmax(v, bred[q][w]);
        __hip_atomic_store(pbox + size_t(blockIdx.x) * (2 * D) + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  // The ticket: the block that draws the last number knows that every other block's partial sums are out.  No __threadfence():
  // an agent-scope fence writes back and invalidates the XCD's whole L2 — which holds the records this kernel has just packed —
  // and 4096 of them made this launch 430 us at N = 2^20.  The partial sums are agent-scope stores (written through), the wave that
  // issued them waits for their acknowledgement (s_waitcnt 0) before its lane 0 draws the ticket, and the last block reads them
  // with agent-scope loads; everything else this kernel writes is read by the NEXT kernel only.
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) last_s = __hip_atomic_fetch_add(&rule->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
  __syncthreads();
  if (!last_s) return;
  if constexpr (MOMENTS) {
    // thread t: moment q = t % (2 D) of the blocks g, g + G, g + 2 G, ... in ascending order (g = t / (2 D), G groups); eight
    // loads in flight at a time (one after the other this loop was 50 us of latency at N = 262 144), added in index order
    double acc = 0.0;
    constexpr int G = kBlock / (2 * D), U = 8;
    const int q = threadIdx.x % (2 * D), g = threadIdx.x / (2 * D);
    if (g < G) {
      for (uint32_t b0 = uint32_t(g); b0 < gridDim.x; b0 += G * U) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const uint32_t b = b0 + uint32_t(u) * G;
          v[u] = b < gridDim.x ? __hip_atomic_load(partial + size_t(b) * (2 * D) + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc += v[u];  // (+ 0.0 past the end: no change)
      }
    }
    __shared__ double fin[kBlock];
    fin[threadIdx.x] = g < G ? acc : 0.0;
    __syncthreads();
    if (threadIdx.x < 2 * D) {  // thread q: the G group sums of moment q in index order
      double tot = 0.0;
#pragma unroll 6
      for (int gg = 0; gg < G; ++gg) tot += fin[gg * (2 * D) + threadIdx.x];
      fin[threadIdx.x] = tot;   // (row 0 of fin: its values have been read by exactly this thread)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double vol = 1.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double mean = fin[k] / double(sz), var = fin[D + k] / double(sz) - mean * mean;
        vol *= var > 0.0 ? __builtin_sqrt(12.0 * var) : 0.0;
      }
      rule->volume = vol;
      rule->sparse = vol >= kFarMinVolume<D> ? 1u : 0u;
    }
  }
  if constexpr (BOX) {
    if (bpc != 0) {
      // sixteen chunks at a time, sixteen neighbouring lanes per chunk: lane `sub` takes the chunk's blocks sub, sub + 16, ...
      // (four rows of loads in flight), the sixteen meet by a butterfly inside their group of lanes, lane 0 of the group stores
      const uint32_t nchunks = (gridDim.x + bpc - 1) / bpc;
      const uint32_t sub     = threadIdx.x & 15u;
      for (uint32_t c0 = 0; c0 < nchunks; c0 += kBlock / 16) {
        const uint32_t c  = c0 + (threadIdx.x >> 4);
        const uint32_t b1 = c < nchunks ? min(gridDim.x, (c + 1u) * bpc) : 0u;
        T lo[D], hi[D];
#pragma unroll
        for (int k = 0; k < D; ++k) lo[k] = T(__builtin_inf()), hi[k] = -T(__builtin_inf());
        for (uint32_t b0 = c * bpc + sub; b0 < b1; b0 += 16u * 4u) {
          T v[4][2 * D];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const uint32_t b = b0 + 16u * uint32_t(u);
#pragma unroll
            for (int q = 0; q < 2 * D; ++q)
              v[u][q] = b < b1 ? __hip_atomic_load(pbox + size_t(b) * (2 * D) + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                               : (q < D ? T(__builtin_inf()) : -T(__builtin_inf()));
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < D; ++k) {
              lo[k] = __builtin_fmin(lo[k], v[u][k]);
              hi[k] = __builtin_fmax(hi[k], v[u][D + k]);
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k)
          for (int off = 8; off > 0; off >>= 1) {
            lo[k] = __builtin_fmin(lo[k], __shfl_xor(lo[k], off, 64));
            hi[k] = __builtin_fmax(hi[k], __shfl_xor(hi[k], off, 64));
          }
        if (c < nchunks && sub == 0) {
#pragma unroll
          for (int k = 0; k < D; ++k) {
            cbox[size_t(c) * (2 * D) + k]     = lo[k];
            cbox[size_t(c) * (2 * D) + D + k] = hi[k];
          }
        }
      }
    }
  }
  for (uint32_t w = threadIdx.x; w < turn_words; w += kBlock) turn[w] = 0u;  // chunk 0 holds every turn
  if (threadIdx.x == 0) __hip_atomic_store(&rule->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int JS>
constexpr int kSgprWaves = JS > kWaves ? JS : kWaves;  // waves per block of the scalar-stream form

// Scalar-stream form.  grid = (target blocks, source chunks): block (b, y) sums chunk y's tiles for target block b — its JS slices'
// sums added in slice order through LDS — and adds that sum s_y to the target's running total IN CHUNK ORDER:
//     a = c * (((s_0 + s_1) + s_2) + ...),
// the total living in `a` itself.  Block (b, y) waits until turn[b] == y (block (b, y - 1) has added its sum), adds, and passes the
// turn on; the last chunk applies c.  No chunk-sum scratch (403 MB at N = 2^20 until round 3) and no combine launch.
//
// Progress rests on ONE assumption that is a property of the dispatcher, not of the ISA: a block waits only for blocks of smaller
// linear index, and the workgroups of a grid are started in linear index order (dealt to the XCDs round-robin, in order on each),
// so the unfinished block of smallest index is always running and never waits.  In practice nobody waits at all — block (b, y - 1)
// finished a whole round of blocks earlier (k1_status.waits counts the waves that did poll, .polls their polls).
//
// If the assumption ever fails, the failure is LOUD (k1_status, nbody_all_pairs_status, nbody_stream_sync, nbody_download):
//   * a wave that has polled h.spins times (kTurnSpins: minutes) gives up: it swaps kTurnPoison into the turn word, records
//     (block, group, chunk) in the stream's sticky status block and overwrites the group's total with NaN;
//   * every wave that finds kTurnPoison while polling overwrites the total with NaN and leaves;
//   * a turn is passed on with a compare-and-swap y -> y + 1; a holder that finds the poison instead writes NaN over what it has
//     just added.
//   EVERY wave that meets the poison writes NaN (round 6; the writes are idempotent), so the order in which they come does not
//   matter: the last store to the group's rows is a NaN in every interleaving — a holder that was in the middle of its add when
//   the poison arrived stores its finite sum, then fails its compare-and-swap and stores NaN behind it; a predecessor that had
//   not even begun to poll when its successors gave up (the case this protocol exists for: a block started late or out of order)
//   finds the poison at its first poll.  Until round 6 only the wave that lost the compare-and-swap wrote NaN, and that late
//   predecessor left a finite partial sum s_0 + ... + s_{y'-1} behind, reported by the status word alone.
//   So a poisoned group ends as NaN (never as a finite partial sum), and the host call that waits for the stream returns
//   NBODY_ERR_STATE naming the block and the chunk.
// The running total is read and written with agent-scope accesses (it changes hands between CUs and XCDs): the predecessor's
// stores are acknowledged (s_waitcnt 0) before its turn store is issued, the successor issues its loads after it has seen the turn.
// What fixes the ROUNDING is unchanged from rounds 2-3, so every shard window still sums exactly as the whole system does.
constexpr uint32_t kTurnSpins  = 1u << 26;
constexpr uint32_t kTurnPoison = 0xffffffffu;
struct k1_status {  // one per (device, stream), device memory, zeroed when allocated; sticky until nbody_all_pairs_status(..., clear)
  uint32_t err, block, group, chunk;
  unsigned long long polls, waits;
};
struct k1_handoff {
  void* sums;         // small launches (k1_collect): every chunk's sum of every target, [chunk][target block][group][r][k][lane]; else nullptr
  uint32_t* turn;     // one word per (target block, target group): the chunk whose sum is added next, or kTurnPoison
                      // (k1_collect: the number of chunks that have delivered their sums)
  k1_status* status;
  uint32_t spins;     // polls before a waiting wave gives up (kTurnSpins; lowered only by the experiments build's tests)
  uint32_t delay;     // s_sleep(127) rounds before a turn is passed on (0; the experiments build's tests make successors wait)
  uint32_t late;      // s_sleep(127) rounds before chunk 1's waves look at the turn word at all (0; experiments: a block started late)
};
// `box` (f64 launches that may take the sparse rule; else nullptr): the source chunks' bounding boxes of the pre-pass, lo[D], hi[D]
// per chunk, for the far certificate (common.hpp: k1_block_is_far) — a block whose boxes prove every pair far streams its chunk
// through a third copy of the loop that has no near/far test (pair_batch_far: the bits of an all-far batch).
constexpr size_t kBoxHeaderBytes = 64;  // in front of the boxes (experiments build: the count of certified blocks)
// The kernel's last argument: the rule, and in f64 the boxes — the f32 kernels keep the argument block (and so the code) they had.
template <typename T>
struct k1_rule_arg {
  const k1_rule* rule;
};
template <>
struct k1_rule_arg<double> {
  const k1_rule* rule;
  const double* box;
};
template <typename T, int D, int R, int JS, int RULE = 0>
__global__ __launch_bounds__(64 * kSgprWaves<JS>) void all_pairs_force_sgpr_kernel(const src_rec<T, D>* __restrict__ packed,
                                                                                   const cst_batch* __restrict__ cst,
                                                                                   const T* __restrict__ x, T* a, T c, uint32_t sz,
                                                                                   uint32_t first, uint32_t count,
                                                                                   uint32_t tiles_per_chunk, k1_handoff h,
                                                                                   k1_rule_arg<T> ra) {
  [[maybe_unused]] constexpr T e2 = T(0);
  const k1_rule* __restrict__ const rule = ra.rule;
  [[maybe_unused]] const T* __restrict__ box = nullptr;
  if constexpr (sizeof(T) == 8) box = ra.box;
#define K1_SOFT false
#include "k1_sgpr_body.inc"
#undef K1_SOFT
}
// Softened K1 (nbody_all_pairs_softened_force): a name of its own, so that the instantiations of the unsoftened kernel stay what
// they were (tools/check_k1_handoff.py holds this one to the same hand-off rules with KERNEL set to its name).
template <typename T, int D, int R, int JS>
__global__ __launch_bounds__(64 * kSgprWaves<JS>) void all_pairs_softened_sgpr_kernel(const src_rec<T, D>* __restrict__ packed,
                                                                                      const cst_batch* __restrict__ cst,
                                                                                      const T* __restrict__ x, T* a, T c, uint32_t sz,
                                                                                      uint32_t first, uint32_t count,
                                                                                      uint32_t tiles_per_chunk, k1_handoff h, T e2) {
  constexpr int RULE = 0;
  const k1_rule* const rule = nullptr;
  [[maybe_unused]] const T* const box = nullptr;  // no pair rule, no test to save: no certificate
#define K1_SOFT true
#include "k1_sgpr_body.inc"
#undef K1_SOFT
}

// Scratch (packed sources; per-chunk sums), one slot per (device, stream) that has called the scalar-stream form (grow-only).  A context
// reserves its buffer when it is created (nbody_create), so that a step recorded with nbody_graph_begin never has to
// allocate; other callers get theirs on the first call, which therefore must not be inside a capture.  A buffer that is
// outgrown is retired, not freed: a recorded graph or a launch another host thread is about to make may still name it.
// Retired buffers go when the slot is released (nbody_destroy) — at most log2(growth) of them, the largest last.
namespace {
struct scratch_buf {
  void* ptr  = nullptr;
  size_t cap = 0;
};
struct packed_slot {
  int device;
  hipStream_t stream;
  scratch_buf buf[9];  // 0: packed sources, 1: K1 turn words, 2: energies work area, 3: the pair rule + partial moments, 4: K1 hand-off status (k1_status), 5: K1 chunk sums of small launches, 6: the packed sources' f64 pair constants (cst_batch), 7: the source chunks' boxes of the far certificate, 8: the space order's work area (k1_order_layout)
  std::vector<void*> retired;
  bool k1_dirty  = false;  // a K1 that passes turns (or a recorded step, which may hold one) has been queued since the status was last read
  bool k1_failed = false;  // the last read found the sticky error set
};
std::mutex g_packed_mu;
std::vector<packed_slot> g_packed_slots;
}  // namespace

int ap_scratch_get(hipStream_t st, int which, size_t bytes, void** out) {
  const int dev = stream_device(st);
  std::lock_guard<std::mutex> lock(g_packed_mu);
  packed_slot* slot = nullptr;
  for (auto& sl : g_packed_slots)
    if (sl.stream == st && sl.device == dev) slot = &sl;
  if (slot && slot->buf[which].cap >= bytes) {
    *out = slot->buf[which].ptr;
    return NBODY_OK;
  }
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (st != nullptr) (void)hipStreamIsCapturing(st, &cs);
  if (cs != hipStreamCaptureStatusNone) {
    set_error("all-pairs: the scratch buffers of this stream must exist before a step is recorded "
              "(call nbody_all_pairs_force once outside nbody_graph_begin/end, or use a context from nbody_create)");
    return NBODY_ERR_STATE;
  }
  if (!slot) {
    g_packed_slots.push_back({dev, st, {}, {}});
    slot = &g_packed_slots.back();
  }
  void* fresh = nullptr;
  NB_HIP(hipMalloc(&fresh, bytes));  // on the stream's device: the caller holds a device_guard
  if (which == 4 || which == 3 || which == 7) {  // the status block and the rule's ticket start at zero (buffer 7: only for the experiments build's count in its header): ordered on the stream that will use
    // them (every launch that reads them is queued on `st` behind this call) — a synchronous memset would go through the legacy
    // stream, which has no defined order with a non-blocking `st` and would invalidate another thread's global-mode capture
    if (hipError_t e = hipMemsetAsync(fresh, 0, bytes, st); e != hipSuccess) {
      (void)hipFree(fresh);
      return hip_fail(e, "hipMemsetAsync(K1 scratch)", __FILE__, __LINE__);
    }
  }
  if (slot->buf[which].ptr) slot->retired.push_back(slot->buf[which].ptr);
  slot->buf[which].ptr = fresh;
  slot->buf[which].cap = bytes;
  *out                 = fresh;
  return NBODY_OK;
}

void ap_scratch_release(hipStream_t st) {
  const int dev = stream_device(st);
  std::lock_guard<std::mutex> lock(g_packed_mu);
  for (size_t i = 0; i < g_packed_slots.size(); ++i) {
    if (g_packed_slots[i].stream == st && g_packed_slots[i].device == dev) {
      for (auto& b : g_packed_slots[i].buf) (void)hipFree(b.ptr);
      for (void* p : g_packed_slots[i].retired) (void)hipFree(p);
      g_packed_slots.erase(g_packed_slots.begin() + long(i));
      return;
    }
  }
}

// ---- launch plan -----------------------------------------------------------------------------------------------
// What fixes the ROUNDING ORDER of a target's sum is derived from sz alone — never from first/count — so every shard
// of a multi-GPU run sums exactly as the single-GPU run does:
//   * split  (JS): the 512-record tile is cut into JS slices, one per wave of a target group; 8 slices (512-thread
//     blocks, scalar-stream form only) once sz >= 2048, else 4;
//   * chunks (Y):  the tile sequence is cut into Y runs, one per grid.y, each run summed by its own block and the Y
//     sums combined in run order by a second kernel.  Equal-sized blocks that start together finish together, so a
//     launch costs ceil(blocks / resident slots) block times: 1563 blocks on 1024 slots (N = 10^5) ran at 31 % of peak
//     against 39 % for N = 2^20.  Y makes the blocks short and many (>= 16 rounds for the whole system, >= 8 for a
//     1/8 shard) whatever N is; co-resident blocks then also share one 128 KB..1 MB run of source records in L2.
// What does NOT touch the order may depend on the window: targets per lane (R) and the LDS / scalar-stream choice.
struct k1_plan {
  bool scalar = false;
  int r = 1, js = 4;
  uint32_t chunks = 1, tiles_per_chunk = 0;
};

static int auto_split(uint32_t sz) { return sz >= 2048u ? 8 : 4; }

// Chunks from sz alone: 16, or more where 16 would leave a chunk above 65 536 records (up to 64), and never more than tiles.
//   * at least 16: every size runs >= 16 rounds of short blocks and small systems get the waves the scalar stream needs.
//     Measured (profiles/r02/k1_chunks_tuning.txt, k1_small_n_tuning.txt; f64, ms per pass, chunks 1 / 16): N = 4096: 0.070 /
//     0.023, 10^4: 0.166 / 0.083, 3*10^4: 0.66 / 0.57, 65 536: 2.64 / 2.50, 10^5: 7.45 / 5.81; more change nothing (N = 10^5:
//     64 chunks 5.87 ms).
//   * chunks of at most 65 536 records (2 MB in f64): blocks are dispatched x-fastest, so the blocks in flight on an XCD stream
//     the SAME chunk, and a chunk of half the XCD's 4 MiB L2 stays there.  N = 2^20 (rocprofv3 FETCH_SIZE per launch, kernel
//     time unchanged within 0.2 %): 4 chunks of 8 MB 8.4 GB, 8 chunks 4.7 GB, 16 chunks of 2 MB 0.46 GB.
void ap_auto_chunks(uint32_t sz, uint32_t* chunks, uint32_t* tiles_per_chunk) {
  const uint32_t ntiles = (sz + kTileJ - 1) / kTileJ;
  uint32_t y = 16;
  while (y < 64 && uint64_t(y) * 65536u < sz) y *= 2;
  if (y > ntiles) y = ntiles ? ntiles : 1;
  uint32_t tpc = ntiles ? (ntiles + y - 1) / y : 1;
  *tiles_per_chunk = tpc;
  *chunks          = ntiles ? (ntiles + tpc - 1) / tpc : 1;
}

template <typename T>
static int plan_all_pairs(const nbody_state* s, k1_plan* out) {
  const ap_config cfg = ap_config_of(s);
  k1_plan p;
  p.js = cfg.split ? cfg.split : auto_split(s->sz);
  p.r  = cfg.tpt;
  // Source path (bitwise identical results at equal split and chunks).  The scalar stream pays an SMEM round trip per
  // 64-byte batch, which needs several waves per SIMD to hide — the source chunks supply them at every size (N = 10^4,
  // f64: LDS tiles 0.19 ms, scalar stream unchunked 0.17-0.33 ms, with 16 chunks 0.083 ms), so the automatic choice is the
  // scalar stream wherever the 8-slice split applies; the LDS-tile form remains for tiny systems and on request.
  const uint64_t waves_r1 = (uint64_t(s->count) + 63) / 64 * uint64_t(p.js);
  p.scalar                = p.js == 8 || cfg.path == 2 || (cfg.path == 0 && waves_r1 >= 4096);
  if (p.js == 8 && cfg.path == 1) {
    set_error("all-pairs: the LDS-tile form has at most 4 source slices; sz = %u uses 8 (nbody_all_pairs_configure(4, ...) to force 4)",
              s->sz);
    return NBODY_ERR_ARG;
  }
  // source chunks: only where the split is the automatic one of large systems (so every explicit configuration keeps
  // its single-chunk order) and only in the scalar-stream form
  p.tiles_per_chunk = (s->sz + kTileJ - 1) / kTileJ;
  if (p.scalar && cfg.split == 0 && p.js == 8) ap_auto_chunks(s->sz, &p.chunks, &p.tiles_per_chunk);
  if (const char* e = experiment_env("NBODY_K1_CHUNKS"); e && p.scalar) {  // -DNBODY_EXPERIMENTS builds only (tools/tune_chunks.py): changes the rounding order
    const uint32_t ntiles = (s->sz + kTileJ - 1) / kTileJ;
    uint32_t y            = uint32_t(atoi(e));
    if (y >= 1 && y <= ntiles) {
      p.tiles_per_chunk = (ntiles + y - 1) / y;
      p.chunks          = (ntiles + p.tiles_per_chunk - 1) / p.tiles_per_chunk;
    }
  }
  if (p.r == 0) {
    // R = 2 halves the scalar-cache traffic per pair and the block count; it pays once the grid is many rounds deep.
    const uint64_t blocks_r2 = (uint64_t(s->count) + 127) / 128 * p.chunks;
    if (p.scalar) p.r = (sizeof(T) == 8 && blocks_r2 >= 4096) ? 2 : 1;
    else p.r = blocks_r2 * uint64_t(p.js) >= 8192 ? 2 : 1;
  }
  *out = p;
  return NBODY_OK;
}

// packs (x, m) of all sz bodies into this stream's record buffer (stream-ordered); used by K1 and by the energies
int ap_pack_sources(const nbody_state* s, hipStream_t st, void** packed_out) {
  const uint32_t padded = (s->sz + kTileJ - 1) / kTileJ * kTileJ;
  const size_t tsz      = s->dtype == NBODY_F32 ? 4 : 8;
  void* scratch         = nullptr;
  if (int r = ap_scratch_get(st, 0, 4 * tsz * size_t(padded), &scratch)) return r;
  int rc = dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    hipLaunchKernelGGL((pack_sources_kernel<T, D>), dim3((padded + kBlock - 1) / kBlock), dim3(kBlock), 0, st,
                       static_cast<const T*>(s->m), static_cast<const T*>(s->x), static_cast<src_rec<T, D>*>(scratch), s->sz, padded);
    NB_HIP(hipGetLastError());
    return int(NBODY_OK);
  });
  *packed_out = scratch;
  return rc;
}

// Bytes of scratch buffer 6 for `padded` packed records (f64 only): one cst_batch per two of them.
static size_t ap_cst_bytes(size_t padded) { return sizeof(cst_batch) * (padded / 2); }

// Bytes of scratch buffer 3 for a system of sz bodies: the rule, then one row of 2 D partial sums per prepare block.
static size_t ap_rule_bytes(uint32_t sz, int dim) {
  const size_t padded = (size_t(sz) + kTileJ - 1) / kTileJ * kTileJ;
  return 32 + sizeof(double) * 2 * size_t(dim) * (padded / kBlock);
}

// Bytes of scratch buffer 7 for a system of sz bodies: a header, a box (lo[dim], hi[dim] in double) per source chunk — there are
// never more chunks than tiles — then one per prepare block.
static size_t ap_box_bytes(uint32_t sz, int dim) {
  const size_t ntiles = (size_t(sz) + kTileJ - 1) / kTileJ;
  return kBoxHeaderBytes + sizeof(double) * 2 * size_t(dim) * (ntiles + ntiles * (kTileJ / kBlock));
}
// The far certificate is attempted by f64 scalar-stream launches that may take the sparse rule and cut their sources into chunks
// (an explicit split has one chunk, whose box is the whole system: nothing to certify, nothing paid).  The automatic launch has
// its chunks from sz alone, so this is a function of sz.  Measured, parent against new, at the shortest chunks the sparse rule
// can meet (N = 32 768: 2048 sources) and at 65 536: profiles/r08/time_far_certificate.txt.
static bool k1_box_wanted(uint32_t sz, uint32_t chunks) { return sz >= kFarMinBodies && chunks > 1; }

// ---- space order (f64, unsoftened, scalar stream, sz >= kOrderMinBodies) ------------------------------------------------------------
// What the far certificate can prove depends on the ORDER of the bodies, not on physics: a source chunk is a run of consecutive
// records and a target group a run of consecutive targets, and where a generator lays the bodies of a disc out in random order
// every chunk's box is the whole disc — only blocks that set one disc against the other certify (half of the flagship's), and
// in the rest 12 % of the batches hold a close pair although 0.05 % of the pairs are close.  An ordered launch therefore sorts
// the packed sources, and the window's own targets, by a space key (k1_order_key.hpp: the Morton code of the body's cell on a
// fixed grid of side 1) before K1 runs:
//   1. k1_prepare_kernel as ever (records, constants, the rule, the turn words; no boxes);
//   2. k1_order_key_kernel: the key of every body — 0 for all of them on the DENSE rule (known on the device only), so that the
//      order below is the identity and a dense launch sums bit for bit as it did unordered;
//   3. radix_sort_pairs: bodies by (key, index) — a total order, so the permutation is a function of the sz positions alone and
//      every rank, window and run has the same one;
//   4. k1_order_gather_kernel: records and constants into that order (padding records stay at the end; huge coordinates
//      clamped, see kOrderSafe), the box of every 256 of
//      them, and — for a window that is the whole system — the targets' positions, which are the records';
//      k1_order_box_kernel: the chunks' boxes from those;
//   5. for any other window: its own bodies' keys, their sort, k1_order_targets_kernel (positions into window order);
//   6. K1 itself, unchanged, on the ordered records with the ordered targets as its `x` (first = 0) and a contiguous scratch
//      array as its `a` — the hand-off reads and writes that array exactly as it did `a`;
//   7. k1_order_scatter_kernel: row k of the scratch array to a[perm[k]] (bit copies: the NaN of a failed hand-off passes).
// A target's sum runs over the sources in key order: other last bits than the natural order gives, the same on every shard.
// The gate is a function of sz and the launch kind, so every rank and window takes it alike.  Measured: profiles/r09/time_space_order.txt.
// Huge coordinates.  K1's pair form is not made for a squared distance that overflows: r2 = +inf, v_rsq_f64 gives 0 and the polish
// 1 - r2 y^2 is inf * 0 = NaN — in EVERY target's sum, since every target meets that source.  A system with such a body has
// infinite variances, which the rule reads as "sparse", so it is ordered; the ordered copies that K1 reads (records and targets,
// never the caller's x) therefore hold every coordinate clamped to +-kOrderSafe = 1e150: no difference of two of them squares
// beyond 1.2e301, and a pair of a body that far out with one of the bulk gets the weight y^3 <= 1e-450 = 0 — its true term is
// below 1.3e-300 m for any body within 1e149 of the origin, so 0 is what the sum would have kept of it anyway (bodies that lie
// beyond 1e150 AND near each other are moved relative to each other: not a system this library serves).  NaN stays NaN (a comparison with it is false), and nothing is clamped on the dense
// rule, where the launch must keep the bits of the unordered one.  No coordinate of an ordinary system is touched.
constexpr double kOrderSafe = 1e150;
__device__ __forceinline__ double k1_order_safe(double p, bool on) { return on && p > kOrderSafe ? kOrderSafe : (on && p < -kOrderSafe ? -kOrderSafe : p); }
constexpr uint32_t kOrderMinBodies = 262144;
static bool k1_order_wanted(uint32_t sz, uint32_t chunks) {
  if (const char* e = experiment_env("NBODY_K1_NO_ORDER"); e && e[0] == '1') return false;  // -DNBODY_EXPERIMENTS builds only
  uint32_t least = kOrderMinBodies;
  if (const char* e = experiment_env("NBODY_K1_ORDER_MIN")) least = uint32_t(strtoul(e, nullptr, 10));  // -DNBODY_EXPERIMENTS builds only (tests)
  return k1_box_wanted(sz, chunks) && sz >= least;
}

// Scratch buffer 8 of an ordered launch of `count` targets out of sz bodies, D-dimensional: byte offsets, 256-byte aligned.
struct k1_order_layout {
  size_t recs, cst, keys[2], idx[2], hist, xs, as, bytes;
};
static k1_order_layout k1_order_layout_of(uint32_t sz, uint32_t count, int dim) {
  const size_t padded = (size_t(sz) + kTileJ - 1) / kTileJ * kTileJ;
  size_t at           = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += (bytes + 255) / 256 * 256;
    return here;
  };
  k1_order_layout l;
  l.recs = take(32 * padded);
  l.cst  = take(ap_cst_bytes(padded));
  for (int b = 0; b < 2; ++b) l.keys[b] = take(sizeof(uint64_t) * sz);
  for (int b = 0; b < 2; ++b) l.idx[b] = take(sizeof(uint32_t) * sz);
  const size_t words = radix_sort_scratch_words(sz) > radix_sort_scratch_words(count) ? radix_sort_scratch_words(sz) : radix_sort_scratch_words(count);
  l.hist  = take(sizeof(uint32_t) * words);
  l.xs    = take(sizeof(double) * size_t(dim) * count);
  l.as    = take(sizeof(double) * size_t(dim) * count);
  l.bytes = at;
  return l;
}

template <int D>
__global__ __launch_bounds__(kBlock) void k1_order_key_kernel(const double* __restrict__ x, uint32_t first, uint32_t n,
                                                              const k1_rule* __restrict__ rule, uint64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double p[D];
#pragma unroll
  for (int k = 0; k < D; ++k) p[k] = x[(uint64_t(first) + i) * D + k];
  keys[i] = rule->sparse ? k1_order_key<D>(p) : 0ull;
}

// One thread per packed record (grid: padded / 256 blocks).  pbox: [block][lo[D], hi[D]], as k1_prepare_kernel makes them.
template <int D>
__global__ __launch_bounds__(kBlock) void k1_order_gather_kernel(const src_rec<double, D>* __restrict__ in, const cst_batch* __restrict__ cin,
                                                                 const uint32_t* __restrict__ perm, src_rec<double, D>* __restrict__ out,
                                                                 cst_batch* __restrict__ cout, uint32_t sz, double* __restrict__ pbox,
                                                                 double* __restrict__ xs, const k1_rule* __restrict__ rule) {
  const uint32_t j   = blockIdx.x * kBlock + threadIdx.x;  // < padded
  const uint32_t src = j < sz ? perm[j] : j;               // (a padding record stays where it is)
  const bool safe    = rule->sparse != 0u;
  src_rec<double, D> r = in[src];
#pragma unroll
  for (int k = 0; k < D; ++k) r.p[k] = k1_order_safe(r.p[k], safe);
  out[j] = r;
  cout[j / 2].m15[j % 2]     = cin[src / 2].m15[src % 2];
  cout[j / 2].m1875[j % 2]   = cin[src / 2].m1875[src % 2];
  if (xs != nullptr && j < sz) {
#pragma unroll
    for (int k = 0; k < D; ++k) xs[uint64_t(j) * D + k] = r.p[k];
  }
  bool finite = true;
#pragma unroll
  for (int k = 0; k < D; ++k) finite = finite && (r.p[k] - r.p[k]) == 0.0;
  double lo[D], hi[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    lo[k] = finite ? r.p[k] : -__builtin_inf();
    hi[k] = finite ? r.p[k] : __builtin_inf();
  }
#pragma unroll
  for (int k = 0; k < D; ++k)
    for (int off = 32; off > 0; off >>= 1) {
      lo[k] = __builtin_fmin(lo[k], __shfl_xor(lo[k], off, 64));
      hi[k] = __builtin_fmax(hi[k], __shfl_xor(hi[k], off, 64));
    }
  __shared__ double bred[2 * D][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      bred[k][wave]     = lo[k];
      bred[D + k][wave] = hi[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * D) {
    const int q = int(threadIdx.x);
    double v    = bred[q][0];
    for (int w = 1; w < kWaves; ++w) v = q < D ? __builtin_fmin(v, bred[q][w]) : __builtin_fmax(v, bred[q][w]);
    pbox[size_t(blockIdx.x) * (2 * D) + q] = v;
  }
}

// One block per source chunk: the chunk's box from the boxes of its bpc gather blocks (the last chunk may have fewer).
template <int D>
__global__ __launch_bounds__(kBlock) void k1_order_box_kernel(const double* __restrict__ pbox, uint32_t nblk, uint32_t bpc, double* __restrict__ cbox) {
  const uint32_t b0 = blockIdx.x * bpc, b1 = min(nblk, b0 + bpc);
  double lo[D], hi[D];
#pragma unroll
  for (int k = 0; k < D; ++k) lo[k] = __builtin_inf(), hi[k] = -__builtin_inf();
  for (uint32_t b = b0 + threadIdx.x; b < b1; b += kBlock) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      lo[k] = __builtin_fmin(lo[k], pbox[size_t(b) * (2 * D) + k]);
      hi[k] = __builtin_fmax(hi[k], pbox[size_t(b) * (2 * D) + D + k]);
    }
  }
#pragma unroll
  for (int k = 0; k < D; ++k)
    for (int off = 32; off > 0; off >>= 1) {
      lo[k] = __builtin_fmin(lo[k], __shfl_xor(lo[k], off, 64));
      hi[k] = __builtin_fmax(hi[k], __shfl_xor(hi[k], off, 64));
    }
  __shared__ double bred[2 * D][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
      bred[k][wave]     = lo[k];
      bred[D + k][wave] = hi[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * D) {
    const int q = int(threadIdx.x);
    double v    = bred[q][0];
    for (int w = 1; w < kWaves; ++w) v = q < D ? __builtin_fmin(v, bred[q][w]) : __builtin_fmax(v, bred[q][w]);
    cbox[size_t(blockIdx.x) * (2 * D) + q] = v;
  }
}

// xs[k] = x[first + perm[k]], k < count (a window that is not the whole system)
template <int D>
__global__ __launch_bounds__(kBlock) void k1_order_targets_kernel(const double* __restrict__ x, uint32_t first, uint32_t count,
                                                                  const uint32_t* __restrict__ perm, double* __restrict__ xs,
                                                                  const k1_rule* __restrict__ rule) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= count) return;
  const uint64_t i = uint64_t(first) + perm[k];
  const bool safe  = rule->sparse != 0u;
#pragma unroll
  for (int d = 0; d < D; ++d) xs[uint64_t(k) * D + d] = k1_order_safe(x[i * D + d], safe);
}

// a[perm[k]] = as[k], k < count, as 64-bit words: whatever K1 left there — a NaN of a failed hand-off too — arrives bit for bit
template <int D>
__global__ __launch_bounds__(kBlock) void k1_order_scatter_kernel(const uint64_t* __restrict__ as, uint32_t count, const uint32_t* __restrict__ perm,
                                                                  uint64_t* __restrict__ a) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= count) return;
  const uint64_t i = perm[k];
#pragma unroll
  for (int d = 0; d < D; ++d) a[i * D + d] = as[uint64_t(k) * D + d];
}

// What an ordered launch hands to K1 in place of the packed records, the boxes, x and a.
template <int D>
struct k1_ordered {
  src_rec<double, D>* packed;
  const cst_batch* cst;
  const double* box;
  const double* xs;
  double* as;
  const uint32_t* tperm;  // the window's targets in launch order, as indices into the window
};

// Steps 2 to 5 above, queued behind the pre-pass.  `packed`, `cst`, `rule`: what ap_prepare made; tpc: tiles per source chunk.
template <int D>
static int k1_order_queue(const nbody_state* s, hipStream_t st, const src_rec<double, D>* packed, const cst_batch* cst, const k1_rule* rule,
                          uint32_t tpc, k1_ordered<D>* out) {
  const uint32_t padded = (s->sz + kTileJ - 1) / kTileJ * kTileJ, nblk = padded / kBlock, bpc = tpc * (kTileJ / kBlock);
  const k1_order_layout l = k1_order_layout_of(s->sz, s->count, D);
  void *w = nullptr, *b = nullptr;
  if (int r = ap_scratch_get(st, 8, l.bytes, &w)) return r;
  if (int r = ap_scratch_get(st, 7, ap_box_bytes(s->sz, D), &b)) return r;
  char* base = static_cast<char*>(w);
  uint64_t* keys[2] = {reinterpret_cast<uint64_t*>(base + l.keys[0]), reinterpret_cast<uint64_t*>(base + l.keys[1])};
  uint32_t* idx[2]  = {reinterpret_cast<uint32_t*>(base + l.idx[0]), reinterpret_cast<uint32_t*>(base + l.idx[1])};
  uint32_t* hist    = reinterpret_cast<uint32_t*>(base + l.hist);
  auto* recs        = reinterpret_cast<src_rec<double, D>*>(base + l.recs);
  auto* csts        = reinterpret_cast<cst_batch*>(base + l.cst);
  double* xs        = reinterpret_cast<double*>(base + l.xs);
  double* cbox      = reinterpret_cast<double*>(static_cast<char*>(b) + kBoxHeaderBytes);
  double* pbox      = cbox + size_t(2 * D) * (padded / kTileJ);
  const double* x   = static_cast<const double*>(s->x);
  const bool whole  = s->first == 0 && s->count == s->sz;
  int fin           = 0;
  hipLaunchKernelGGL((k1_order_key_kernel<D>), dim3((s->sz + kBlock - 1) / kBlock), dim3(kBlock), 0, st, x, 0u, s->sz, rule, keys[0]);
  NB_HIP(hipGetLastError());
  if (int r = radix_sort_pairs(keys, idx, s->sz, kOrderKeyBits, hist, st, &fin)) return r;
  hipLaunchKernelGGL((k1_order_gather_kernel<D>), dim3(nblk), dim3(kBlock), 0, st, packed, cst, idx[fin], recs, csts, s->sz, pbox,
                     whole ? xs : static_cast<double*>(nullptr), rule);
  NB_HIP(hipGetLastError());
  hipLaunchKernelGGL((k1_order_box_kernel<D>), dim3((nblk + bpc - 1) / bpc), dim3(kBlock), 0, st, pbox, nblk, bpc, cbox);
  NB_HIP(hipGetLastError());
  if (!whole) {  // the window's own order (the sources' permutation is spent: its buffers are reused)
    hipLaunchKernelGGL((k1_order_key_kernel<D>), dim3((s->count + kBlock - 1) / kBlock), dim3(kBlock), 0, st, x, s->first, s->count, rule, keys[0]);
    NB_HIP(hipGetLastError());
    if (int r = radix_sort_pairs(keys, idx, s->count, kOrderKeyBits, hist, st, &fin)) return r;
    hipLaunchKernelGGL((k1_order_targets_kernel<D>), dim3((s->count + kBlock - 1) / kBlock), dim3(kBlock), 0, st, x, s->first, s->count, idx[fin], xs, rule);
    NB_HIP(hipGetLastError());
  }
  *out = {recs, csts, cbox, xs, reinterpret_cast<double*>(base + l.as), idx[fin]};
  return NBODY_OK;
}

// Everything a K1 launch needs done first, queued as ONE launch (k1_prepare_kernel): the packed records (pack: the scalar-stream
// form), the pair rule of the whole system (sz >= kFarMinBodies; nullptr = "dense" below) and the turn words handed back to chunk 0.
// The softened K1 has no pair rule (with_rule false): no moments are summed.  box_tpc != 0 (f64, pack): the launch's tiles per
// source chunk — the chunks' boxes are made too (*box_out; nullptr where the rule is dense by definition).
template <typename T, int D>
static int ap_prepare(const nbody_state* s, hipStream_t st, bool pack, src_rec<T, D>** packed_out, const cst_batch** cst_out,
                      const k1_rule** rule_out, uint32_t* turn, size_t turn_words, bool with_rule = true, uint32_t box_tpc = 0,
                      const T** box_out = nullptr) {
  const uint32_t padded = (s->sz + kTileJ - 1) / kTileJ * kTileJ;
  const bool moments    = with_rule && s->sz >= kFarMinBodies;
  void* scratch         = nullptr;
  void* consts          = nullptr;
  if (pack) {
    if (int r = ap_scratch_get(st, 0, 4 * sizeof(T) * size_t(padded), &scratch)) return r;
    if (sizeof(T) == 8)
      if (int r = ap_scratch_get(st, 6, ap_cst_bytes(padded), &consts)) return r;
  }
  void* q = nullptr;
  if (int r = ap_scratch_get(st, 3, ap_rule_bytes(s->sz, D), &q)) return r;  // (the ticket lives there even without moments)
  auto* rule    = static_cast<k1_rule*>(q);
  auto* partial = reinterpret_cast<double*>(static_cast<char*>(q) + 32);
  auto* out     = static_cast<src_rec<T, D>*>(scratch);
  auto* cst     = static_cast<cst_batch*>(consts);
  T *cbox = nullptr, *pbox = nullptr;
  uint32_t bpc = 0;  // prepare blocks per source chunk
  if (sizeof(T) == 8 && pack && moments && box_tpc != 0) {
    void* b = nullptr;
    if (int r = ap_scratch_get(st, 7, ap_box_bytes(s->sz, D), &b)) return r;
    cbox = reinterpret_cast<T*>(static_cast<char*>(b) + kBoxHeaderBytes);
    pbox = cbox + size_t(2 * D) * (padded / kTileJ);
    bpc  = box_tpc * (kTileJ / kBlock);
  }
  const dim3 grid(padded / kBlock), block(kBlock);
  const T *m = static_cast<const T*>(s->m), *x = static_cast<const T*>(s->x);
  const uint32_t words = uint32_t(turn_words);
  k1_prepare_tail<T> tail{};
  tail.turn_words = words;
  if constexpr (sizeof(T) == 8) tail.bpc = bpc, tail.cbox = cbox, tail.pbox = pbox;
  if (pack && moments) hipLaunchKernelGGL((k1_prepare_kernel<T, D, true, true>), grid, block, 0, st, m, x, out, cst, s->sz, padded, rule, partial, turn, tail);
  else if (pack) hipLaunchKernelGGL((k1_prepare_kernel<T, D, true, false>), grid, block, 0, st, m, x, out, cst, s->sz, padded, rule, partial, turn, tail);
  else if (moments) hipLaunchKernelGGL((k1_prepare_kernel<T, D, false, true>), grid, block, 0, st, m, x, out, cst, s->sz, padded, rule, partial, turn, tail);
  NB_HIP(hipGetLastError());
  if (box_out) *box_out = cbox;
  if (packed_out) *packed_out = out;
  if (cst_out) *cst_out = cst;
  *rule_out = moments ? rule : nullptr;
  return NBODY_OK;
}

// How the chunks' sums of a launch meet (bitwise the same either way): collected by the last chunk to arrive when the whole grid is
// resident within two rounds (<= 2048 blocks: up to 3 MB of sums), passed from chunk to chunk in `a` otherwise (no scratch).
// Measured (profiles/r05/k1_handoff_cost.txt; f64, us per launch, collected / turns / no protocol at all): N = 2048 16.2 / 23.5 / 15.1,
// 4096 23 / 41 / 20, 8192 55 / 70 / 51, f32 8192 34 / 76 / 29 — and at 4096 blocks (N = 16 384) 176 / 172 / 172: turns from there on.
constexpr uint32_t kCollectMaxBlocks = 2048;
static bool k1_collect(uint32_t target_blocks, uint32_t chunks) {
  uint32_t limit = kCollectMaxBlocks;
  if (const char* e = experiment_env("NBODY_K1_COLLECT_MAX")) limit = uint32_t(atoi(e));  // -DNBODY_EXPERIMENTS builds only (tools/tune_small_k1.py)
  return chunks > 1 && uint64_t(target_blocks) * chunks <= limit;
}
template <typename T, int D, int R, int JS>
static size_t k1_collect_bytes(uint32_t target_blocks, uint32_t chunks) {
  constexpr int TG = kSgprWaves<JS> / JS;
  return sizeof(T) * size_t(chunks) * target_blocks * TG * R * D * 64;
}

// words of the turn array for a launch of `blocks` target blocks (one per target group of a block)
template <int R, int JS>
static size_t sgpr_turn_words(uint32_t count) {
  constexpr int TG = kSgprWaves<JS> / JS, TB = TG * 64 * R;
  return size_t((count + TB - 1) / TB) * TG;
}

template <typename T, int D, int R, int JS, bool SOFT>
static int launch_all_pairs_sgpr(const nbody_state* s, const k1_plan& plan, hipStream_t st, T e2) {
  constexpr int TB = (kSgprWaves<JS> / JS) * 64 * R;
  uint32_t blocks  = (s->count + TB - 1) / TB;
  if (blocks == 0) return NBODY_OK;
  k1_handoff h{nullptr, nullptr, nullptr, kTurnSpins, 0u, 0u};
  if (plan.chunks > 1) {  // before anything is queued: a failed reservation leaves the stream untouched
    void* q = nullptr;
    if (int r = ap_scratch_get(st, 1, sizeof(uint32_t) * sgpr_turn_words<R, JS>(s->count), &q)) return r;
    h.turn = static_cast<uint32_t*>(q);
    if (k1_collect(blocks, plan.chunks)) {
      if (int r = ap_scratch_get(st, 5, k1_collect_bytes<T, D, R, JS>(blocks, plan.chunks), &q)) return r;
      h.sums = q;
    }
    if (int r = ap_scratch_get(st, 4, sizeof(k1_status), &q)) return r;
    h.status = static_cast<k1_status*>(q);
    // -DNBODY_EXPERIMENTS builds only (tests/test_gpu_all_pairs.py: the hand-off made to wait, and made to fail)
    if (const char* e = experiment_env("NBODY_K1_TURN_SPINS")) h.spins = uint32_t(strtoul(e, nullptr, 10));
    if (const char* e = experiment_env("NBODY_K1_HANDOFF_DELAY")) h.delay = uint32_t(strtoul(e, nullptr, 10));
    if (const char* e = experiment_env("NBODY_K1_HANDOFF_LATE")) h.late = uint32_t(strtoul(e, nullptr, 10));
    // timing experiment only (WRONG sums): no turn words — every chunk's block adds to whatever `a` holds without waiting
    if (const char* e = experiment_env("NBODY_K1_NO_HANDOFF"); e && e[0] == '1') h.turn = nullptr, h.sums = nullptr;
    if (const char* e = experiment_env("NBODY_K1_COLLECT"); e && e[0] == '0') h.sums = nullptr;  // experiments: turns at every size
  }
  src_rec<T, D>* packed = nullptr;
  const cst_batch* cst  = nullptr;  // f64 only
  const k1_rule* rule   = nullptr;
  const T* box          = nullptr;  // f64, unsoftened, from kFarMinBodies on: the chunks' boxes of the far certificate
  bool certify          = !SOFT && sizeof(T) == 8 && k1_box_wanted(s->sz, plan.chunks);
  if (const char* e = experiment_env("NBODY_K1_NO_CERT"); e && e[0] == '1') certify = false;  // -DNBODY_EXPERIMENTS builds only
  // the space order (see k1_order_wanted): the boxes are then made from the ordered records, not by the pre-pass
  [[maybe_unused]] const bool ordered = certify && plan.chunks > 1 && k1_order_wanted(s->sz, plan.chunks);
  if (int r = ap_prepare<T, D>(s, st, true, &packed, &cst, &rule, h.turn, h.turn ? sgpr_turn_words<R, JS>(s->count) : 0, !SOFT,
                               certify && !ordered ? plan.tiles_per_chunk : 0u, &box))
    return r;
  if constexpr (SOFT) {
    hipLaunchKernelGGL((all_pairs_softened_sgpr_kernel<T, D, R, JS>), dim3(blocks, plan.chunks), dim3(64 * kSgprWaves<JS>), 0, st,
                       packed, cst, static_cast<const T*>(s->x), static_cast<T*>(s->a), static_cast<T>(s->c), s->sz, s->first, s->count,
                       plan.tiles_per_chunk, h, e2);
    NB_HIP(hipGetLastError());
    if (h.turn != nullptr && h.sums == nullptr) ap_status_mark(st);
    return NBODY_OK;
  }
  k1_rule_arg<T> ra{};
  ra.rule = rule;
  if constexpr (sizeof(T) == 8) ra.box = box;
#ifdef NBODY_EXPERIMENTS
  if (const char* e = getenv("NBODY_K1_RULE_FORCE"); e && JS == 8 && D == 3) {  // timing experiment: one rule per instantiation
    if (e[0] == '1')
      hipLaunchKernelGGL((all_pairs_force_sgpr_kernel<T, D, R, JS, 1>), dim3(blocks, plan.chunks), dim3(64 * kSgprWaves<JS>), 0, st,
                         packed, cst, static_cast<const T*>(s->x), static_cast<T*>(s->a), static_cast<T>(s->c), s->sz, s->first, s->count,
                         plan.tiles_per_chunk, h, ra);
    else
      hipLaunchKernelGGL((all_pairs_force_sgpr_kernel<T, D, R, JS, 2>), dim3(blocks, plan.chunks), dim3(64 * kSgprWaves<JS>), 0, st,
                         packed, cst, static_cast<const T*>(s->x), static_cast<T*>(s->a), static_cast<T>(s->c), s->sz, s->first, s->count,
                         plan.tiles_per_chunk, h, ra);
    NB_HIP(hipGetLastError());
    return NBODY_OK;
  }
#endif
  if constexpr (sizeof(T) == 8) {
    if (ordered) {
      k1_ordered<D> o{};
      if (int r = k1_order_queue<D>(s, st, packed, cst, rule, plan.tiles_per_chunk, &o)) return r;
      ra.box = o.box;
      hipLaunchKernelGGL((all_pairs_force_sgpr_kernel<T, D, R, JS>), dim3(blocks, plan.chunks), dim3(64 * kSgprWaves<JS>), 0, st,
                         o.packed, o.cst, o.xs, o.as, static_cast<T>(s->c), s->sz, 0u, s->count, plan.tiles_per_chunk, h, ra);
      NB_HIP(hipGetLastError());
      hipLaunchKernelGGL((k1_order_scatter_kernel<D>), dim3((s->count + kBlock - 1) / kBlock), dim3(kBlock), 0, st,
                         reinterpret_cast<const uint64_t*>(o.as), s->count, o.tperm, static_cast<uint64_t*>(s->a));
      NB_HIP(hipGetLastError());
      if (h.turn != nullptr && h.sums == nullptr) ap_status_mark(st);
      return NBODY_OK;
    }
  }
  hipLaunchKernelGGL((all_pairs_force_sgpr_kernel<T, D, R, JS>), dim3(blocks, plan.chunks), dim3(64 * kSgprWaves<JS>), 0, st,
                     packed, cst, static_cast<const T*>(s->x), static_cast<T*>(s->a), static_cast<T>(s->c), s->sz, s->first, s->count,
                     plan.tiles_per_chunk, h, ra);
  NB_HIP(hipGetLastError());
  if (h.turn != nullptr && h.sums == nullptr) ap_status_mark(st);  // turns were passed: the next wait for this stream reads the status
  return NBODY_OK;
}

template <typename T, int D, int R, int JS, bool SOFT>
static int launch_all_pairs(const nbody_state* s, hipStream_t st, T e2) {
  constexpr int TB = (kWaves / JS) * 64 * R;
  uint32_t blocks  = (s->count + TB - 1) / TB;
  if (blocks == 0) return NBODY_OK;
  if constexpr (SOFT) {  // nothing to prepare: no packed records, no pair rule
    hipLaunchKernelGGL((all_pairs_softened_kernel<T, D, R, JS>), dim3(blocks), dim3(kBlock), 0, st, static_cast<const T*>(s->m),
                       static_cast<const T*>(s->x), static_cast<T*>(s->a), static_cast<T>(s->c), s->sz, s->first, s->count, e2);
    NB_HIP(hipGetLastError());
    return NBODY_OK;
  }
  const k1_rule* rule = nullptr;  // the same per-pair rule as the scalar-stream form (bitwise the same result)
  if (int r = ap_prepare<T, D>(s, st, false, nullptr, nullptr, &rule, nullptr, 0)) return r;
  hipLaunchKernelGGL((all_pairs_force_kernel<T, D, R, JS>), dim3(blocks), dim3(kBlock), 0, st, static_cast<const T*>(s->m),
                     static_cast<const T*>(s->x), static_cast<T*>(s->a), static_cast<T>(s->c), s->sz, s->first, s->count, rule);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// calls fn(R, JS) as integral constants for the instantiation a plan names; false if there is none
template <typename F>
static bool with_k1_instance(const k1_plan& p, F&& fn) {
#define NB_CASE(RR, JJ)                                                                       \
  if (p.r == RR && p.js == JJ) {                                                              \
    fn(std::integral_constant<int, RR>{}, std::integral_constant<int, JJ>{});                 \
    return true;                                                                              \
  }
  NB_CASE(1, 1);
  NB_CASE(1, 2);
  NB_CASE(1, 4);
  NB_CASE(2, 1);
  NB_CASE(2, 2);
  NB_CASE(2, 4);
  if (p.scalar) {
    NB_CASE(1, 8);
    NB_CASE(2, 8);
  }
#undef NB_CASE
  return false;
}

// SOFT: the softened K1 (e2 > 0) on the same launch plan — the same slices, chunks and hand-off, so the same rounding structure
template <typename T, int D, bool SOFT = false>
static int all_pairs_dispatch(const nbody_state* s, hipStream_t st, T e2 = T(0)) {
  k1_plan p;
  if (int rc = plan_all_pairs<T>(s, &p)) return rc;
  int rc = NBODY_OK;
  const bool found = with_k1_instance(p, [&](auto r, auto js) {
    constexpr int R = decltype(r)::value, JS = decltype(js)::value;
    rc = p.scalar ? launch_all_pairs_sgpr<T, D, R, JS, SOFT>(s, p, st, e2)
                  : (JS <= kWaves ? launch_all_pairs<T, D, R, (JS <= kWaves ? JS : 1), SOFT>(s, st, e2) : int(NBODY_ERR_ARG));
  });
  if (!found) {
    set_error("all-pairs: unsupported config split=%d targets_per_thread=%d", p.js, p.r);
    return NBODY_ERR_ARG;
  }
  return rc;
}

template <typename T, int D>
static int all_pairs_describe(const nbody_state* s, char* out, size_t len) {
  k1_plan p;
  if (int rc = plan_all_pairs<T>(s, &p)) return rc;
  const char* t = sizeof(T) == 8 ? "double" : "float";
  const char* pair = sizeof(T) == 4 ? (s->sz >= kFarMinBodies ? "rsq+rcp[m y^3 at r2 >= 4 if sparse]" : "rsq+rcp")
                                    : s->sz >= kFarMinBodies ? "far3m[-eps if sparse]/near3" : "far3m/near3";
  if (p.scalar) {
    bool collect = false;
    with_k1_instance(p, [&](auto r, auto js) {
      constexpr int TB = (kSgprWaves<decltype(js)::value> / decltype(js)::value) * 64 * decltype(r)::value;
      collect = k1_collect((s->count + TB - 1) / TB, p.chunks);
    });
    snprintf(out, len, "all_pairs_force_sgpr_kernel<%s,%d,R=%d,JS=%d> tile=%d chunks=%u%s pair=%s%s", t, D, p.r, p.js, kTileJ, p.chunks,
             p.chunks > 1 ? (collect ? "(summed in chunk order by the last to arrive)" : "(summed in turn into a)") : "", pair,
             sizeof(T) == 8 && k1_box_wanted(s->sz, p.chunks)
                 ? (k1_order_wanted(s->sz, p.chunks) ? " cert=box-gap>=3[if sparse: blocks proven far skip the r2 test] order=morton30[if sparse]"
                                                    : " cert=box-gap>=3[if sparse: blocks proven far skip the r2 test]")
                 : "");
  }
  else
    snprintf(out, len, "all_pairs_force_kernel<%s,%d,R=%d,JS=%d> tile=%d chunks=1 pair=%s", t, D, p.r, p.js, kTileJ, pair);
  return NBODY_OK;
}

// Everything the K1 launch for this view needs from the stream's scratch slot, reserved ahead (nbody_create,
// nbody_ctx_set_shard, nbody_ctx_configure_all_pairs) so that a recorded step never allocates: the packed records (in f64 their
// pair constants too), the extent keys and the turn words (one per target group: 32 KB at N = 2^20; this slot held 403 MB of chunk sums until round 3).
int ap_scratch_reserve(hipStream_t st, const nbody_state* s) {
  void* q             = nullptr;
  const size_t tsz    = s->dtype == NBODY_F32 ? 4 : 8;
  const size_t padded = (size_t(s->sz) + 2 * kTileJ - 1) / (2 * kTileJ) * (2 * kTileJ);  // K1 needs whole tiles, the streamed K2 pairs of them
  if (int r = ap_scratch_get(st, 0, 4 * tsz * padded, &q)) return r;
  if (s->dtype == NBODY_F64)
    if (int r = ap_scratch_get(st, 6, ap_cst_bytes(padded), &q)) return r;
  if (int r = ap_scratch_get(st, 3, ap_rule_bytes(s->sz, s->dim), &q)) return r;
  if (s->dtype == NBODY_F64 && s->sz >= kFarMinBodies)  // (whatever the launch shape turns out to be)
    if (int r = ap_scratch_get(st, 7, ap_box_bytes(s->sz, s->dim), &q)) return r;
  if (s->dtype == NBODY_F64) {  // the space order's work area, where this view's launch is an ordered one
    k1_plan p;
    if (int rc = plan_all_pairs<double>(s, &p)) return rc;
    if (p.scalar && k1_order_wanted(s->sz, p.chunks))
      if (int r = ap_scratch_get(st, 8, k1_order_layout_of(s->sz, s->count, s->dim).bytes, &q)) return r;
  }
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T = typename decltype(tg)::type;
    k1_plan p;
    if (int rc = plan_all_pairs<T>(s, &p)) return rc;
    if (!p.scalar || p.chunks <= 1) return int(NBODY_OK);
    size_t words = 0;
    with_k1_instance(p, [&](auto r, auto js) { words = sgpr_turn_words<decltype(r)::value, decltype(js)::value>(s->count); });
    if (!words) return int(NBODY_OK);
    if (int rc = ap_scratch_get(st, 1, sizeof(uint32_t) * words, &q)) return rc;
    size_t sums = 0;
    with_k1_instance(p, [&](auto r, auto js) {
      constexpr int RR = decltype(r)::value, JJ = decltype(js)::value;
      const uint32_t blocks = (s->count + (kSgprWaves<JJ> / JJ) * 64 * RR - 1) / ((kSgprWaves<JJ> / JJ) * 64 * RR);
      if (k1_collect(blocks, p.chunks)) sums = k1_collect_bytes<T, decltype(tg)::dim, RR, JJ>(blocks, p.chunks);
    });
    if (sums)
      if (int rc = ap_scratch_get(st, 5, sums, &q)) return rc;
    return ap_scratch_get(st, 4, sizeof(k1_status), &q);
  });
}

// The hand-off status of a stream's K1 launches (see all_pairs_force_sgpr_kernel).  Waits for the stream.  out (may be NULL):
// {err, block, group, chunk, polls, waits}.  Returns NBODY_ERR_STATE (and the message) while the sticky error word is set.
void ap_status_mark(hipStream_t st) {
  const int dev = stream_device(st);
  std::lock_guard<std::mutex> lock(g_packed_mu);
  for (auto& sl : g_packed_slots)
    if (sl.stream == st && sl.device == dev) sl.k1_dirty = true;
}

int ap_status_read(hipStream_t st, unsigned long long out[6], bool clear) {
  const int dev = stream_device(st);
  k1_status* dptr = nullptr;
  {
    // the 32-byte copy is made only when it can say something new: an explicit query, a turn-passing K1 or a recorded step queued
    // since the last read, or an error already seen (a tree run in --csv-detailed mode waits for the stream six times per step)
    std::lock_guard<std::mutex> lock(g_packed_mu);
    for (auto& sl : g_packed_slots)
      if (sl.stream == st && sl.device == dev && (out != nullptr || sl.k1_dirty || sl.k1_failed)) dptr = static_cast<k1_status*>(sl.buf[4].ptr);
  }
  k1_status h{};
  if (dptr) NB_HIP(hipMemcpyAsync(&h, dptr, sizeof h, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  if (dptr && clear && (h.err || h.polls || h.waits)) {
    NB_HIP(hipMemsetAsync(dptr, 0, sizeof h, st));
    NB_HIP(hipStreamSynchronize(st));
  }
  if (out) {
    out[0] = h.err, out[1] = h.block, out[2] = h.group, out[3] = h.chunk;
    out[4] = h.polls, out[5] = h.waits;
  }
  if (dptr) {
    std::lock_guard<std::mutex> lock(g_packed_mu);
    for (auto& sl : g_packed_slots)
      if (sl.stream == st && sl.device == dev) sl.k1_dirty = false, sl.k1_failed = h.err != 0 && !clear;
  }
  if (h.err) {
    set_error("all-pairs: the chunk hand-off of target block %u (group %u) failed at source chunk %u: the block of chunk %u never passed "
              "the turn on within the poll budget (workgroups not started in index order?).  `a` of that launch is not valid (the "
              "group's rows are NaN).  The flag is sticky for this stream until nbody_all_pairs_status(stream, out, 1)",
              h.block, h.group, h.chunk, h.chunk - 1u);
    return NBODY_ERR_STATE;
  }
  return NBODY_OK;
}

// ------------------------------------------------------------------------------------------------
// K2
// ------------------------------------------------------------------------------------------------
// sources per LDS tile: 32 per lane in f32 (32 KB), 16 per lane in f64 (32 KB): the cross-lane reduction and the target
// broadcasts are paid once per (NT targets x tile), so the tile is as long as the LDS budget of 3-4 blocks per CU allows
template <typename T>
constexpr int kColTileJ = sizeof(T) == 4 ? 2048 : 1024;

template <typename T, int D>
__global__ __launch_bounds__(kBlock) void collapsed_reset_kernel(T* __restrict__ a, const T* __restrict__ ao, uint64_t n) {
  // diagonal pairs of the reference (src/all_pairs.h:35-40): a[i] -= ao[i]
  uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (e < n) a[e] = a[e] - ao[e];
}

// Wavefront sum over 64 lanes with DPP cross-lane adds (VALU data path; __shfl_xor compiles to ds_bpermute_b32,
// which goes through the LDS crossbar at ~21 cycles each when every SIMD does it).  Quad swaps and row mirrors give
// every lane of a 16-lane row the row sum; row_bcast:15 / row_bcast:31 (GFX9 DPP, present on gfx950) chain the four
// rows so that lane 63 holds the total, which is returned wave-uniform through v_readlane.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);  // disabled/invalid lanes read 0
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_get(float v) {
  return __builtin_bit_cast(float, dpp_i32<CTRL, ROW_MASK>(__builtin_bit_cast(int, v)));
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_get(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = dpp_i32<CTRL, ROW_MASK>(int(b)), hi = dpp_i32<CTRL, ROW_MASK>(int(b >> 32));
  return __builtin_bit_cast(double, (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

template <typename T>
__device__ __forceinline__ T lane_bcast(T v, int src) {  // src is wave-uniform
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
  } else {
    long long b = __builtin_bit_cast(long long, v);
    int lo      = __builtin_amdgcn_readlane(int(b), src);
    int hi      = __builtin_amdgcn_readlane(int(b >> 32), src);
    return __builtin_bit_cast(T, (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
  }
}

// Transposed wavefront reduction.  Every lane holds NT partial sums p[0..NT-1] (one per target of a group); on return
// lane l holds, in p[0], the sum over ALL 64 lanes of partial number (l % NT).  One halving stage pairs each lane with a
// partner on the other side of one lane-index bit (row_mirror: l^15, row_half_mirror: l^7, quad_perm: l^2, l^1 — all
// plain DPP row operations on the VALU data path); a lane passes the half of its partials the partner keeps and adds
// what it receives to the half it keeps, so a stage over 2m partials costs m DPP adds + 2m selects and the whole row
// part NT - 1 DPP adds — against 6 DPP adds + a v_readlane PER partial for one wave_sum each (the form this replaces:
// 96 vs 15 cross-lane adds per 16 targets and component).  The remaining factor 64 / NT is summed with full-wave
// exchanges (lane ^ 8 by row_ror:8, lane ^ 16 and ^ 32 through ds_bpermute: 2-3 per group).
template <typename T>
__device__ __forceinline__ T xor_lane_add(T v, int mask) {  // v + v of lane (l ^ mask), mask in {16, 32}
  return v + __shfl_xor(v, mask, 64);
}

template <typename T, int NT>
__device__ __forceinline__ T transpose_reduce(T (&p)[NT], int lane) {
  static_assert(NT == 16 || NT == 8, "groups of 16 (f32) or 8 (f64) targets");
  if constexpr (NT == 16) {
    const bool up = (lane & 8) != 0;  // row_mirror: l <-> 15 - l
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const T send = up ? p[i] : p[i + 8], keep = up ? p[i + 8] : p[i];
      p[i]         = keep + dpp_get<0x140>(send);
    }
  }
  {
    const bool up = (lane & 4) != 0;  // row_half_mirror: l <-> l ^ 7
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const T send = up ? p[i] : p[i + 4], keep = up ? p[i + 4] : p[i];
      p[i]         = keep + dpp_get<0x141>(send);
    }
  }
  {
    const bool up = (lane & 2) != 0;  // quad_perm:[2,3,0,1]: l <-> l ^ 2
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const T send = up ? p[i] : p[i + 2], keep = up ? p[i + 2] : p[i];
      p[i]         = keep + dpp_get<0x4E>(send);
    }
  }
  {
    const bool up = (lane & 1) != 0;  // quad_perm:[1,0,3,2]: l <-> l ^ 1
    const T send  = up ? p[0] : p[1], keep = up ? p[1] : p[0];
    p[0]          = keep + dpp_get<0xB1>(send);
  }
  T v = p[0];  // sum over the lane's NT-lane group of partial (lane % NT)
  if constexpr (NT == 8) v += dpp_get<0x128>(v);  // row_ror:8: l <-> l ^ 8
  v = xor_lane_add(v, 16);
  v = xor_lane_add(v, 32);
  return v;
}

// K2's float pair (3D), scheduled by hand (round 6).  hipcc emits the pair as ONE dependent chain — sub, fma, fma, fma, rsq,
// s_nop, mul, fma, rcp, s_nop, mul, fma x 3: every instruction waits for the one before it and each transcendental is followed
// by a wait state (239 s_nop per 128 pairs) — and its own interleavings of two or four chains put v_rsq_f32 and v_rcp_f32 back
// to back and lost (28.7 against 24.05 ms at config 3, rounds 2 and 5).  Here pair p's head (differences, r^2, rsq) is
// interleaved with pair p - 1's tail (r^2 y, + eps, rcp, x m, three accumulations): the same fourteen instructions, the same
// operations on the same operands in the same order per accumulator (bitwise what pair_math<float>::weight gives), no wait
// state, every transcendental at least three instructions ahead of its consumer and seven behind the other one.
// The carried state (the last pair's differences, r^2 and rsq) lives in VGPRs between the blocks.
struct k2_carry {
  float dx, dy, dz, r2, y;
};
__device__ __forceinline__ k2_carry k2_pair_head(const src_rec<float, 3>& s, const float (&xg)[3]) {
  k2_carry n;
  asm volatile(
      "v_subrev_f32 %[dx], %[X], %[sx]\n\t"
      "v_subrev_f32 %[dy], %[Y], %[sy]\n\t"
      "v_subrev_f32 %[dz], %[Z], %[sz]\n\t"
      "v_fmaak_f32 %[r2], %[dx], %[dx], 0x2081cea\n\t"   // pair_math<float>::tiny
      "v_fmac_f32 %[r2], %[dy], %[dy]\n\t"
      "v_fmac_f32 %[r2], %[dz], %[dz]\n\t"
      "v_rsq_f32 %[y], %[r2]\n\t"
      "s_nop 0"   // the consumer may be the very next instruction (the tail of a block of one pair)
      : [dx] "=&v"(n.dx), [dy] "=&v"(n.dy), [dz] "=&v"(n.dz), [r2] "=&v"(n.r2), [y] "=&v"(n.y)
      : [sx] "v"(s.p[0]), [sy] "v"(s.p[1]), [sz] "v"(s.p[2]), [X] "s"(xg[0]), [Y] "s"(xg[1]), [Z] "s"(xg[2]));
  return n;
}
// head of the pair (s, xg) + tail of the carried pair: its weight r2 -> m / (r2 * (r2 * y) + eps), accumulated into (ax, ay, az)
__device__ __forceinline__ k2_carry k2_pair_step(const src_rec<float, 3>& s, const float (&xg)[3], float mp, const k2_carry& c,
                                                 float& ax, float& ay, float& az) {
  k2_carry n;
  float t;
  asm volatile(
      "v_mul_f32 %[t], %[r2p], %[yp]\n\t"
      "v_subrev_f32 %[dx], %[X], %[sx]\n\t"
      "v_fmaak_f32 %[t], %[r2p], %[t], 0x34000000\n\t"   // FLT_EPSILON
      "v_subrev_f32 %[dy], %[Y], %[sy]\n\t"
      "v_subrev_f32 %[dz], %[Z], %[sz]\n\t"
      "v_rcp_f32 %[t], %[t]\n\t"
      "v_fmaak_f32 %[r2], %[dx], %[dx], 0x2081cea\n\t"
      "v_fmac_f32 %[r2], %[dy], %[dy]\n\t"
      "v_fmac_f32 %[r2], %[dz], %[dz]\n\t"
      "v_mul_f32 %[t], %[mp], %[t]\n\t"
      "v_rsq_f32 %[y], %[r2]\n\t"
      "v_fmac_f32 %[ax], %[t], %[dxp]\n\t"
      "v_fmac_f32 %[ay], %[t], %[dyp]\n\t"
      "v_fmac_f32 %[az], %[t], %[dzp]"
      : [dx] "=&v"(n.dx), [dy] "=&v"(n.dy), [dz] "=&v"(n.dz), [r2] "=&v"(n.r2), [y] "=&v"(n.y), [t] "=&v"(t), [ax] "+v"(ax),
        [ay] "+v"(ay), [az] "+v"(az)
      : [sx] "v"(s.p[0]), [sy] "v"(s.p[1]), [sz] "v"(s.p[2]), [X] "s"(xg[0]), [Y] "s"(xg[1]), [Z] "s"(xg[2]), [mp] "v"(mp),
        [r2p] "v"(c.r2), [yp] "v"(c.y), [dxp] "v"(c.dx), [dyp] "v"(c.dy), [dzp] "v"(c.dz));
  return n;
}
__device__ __forceinline__ void k2_pair_tail(float mp, const k2_carry& c, float& ax, float& ay, float& az) {
  float t;
  asm volatile(
      "v_mul_f32 %[t], %[r2p], %[yp]\n\t"
      "v_fmaak_f32 %[t], %[r2p], %[t], 0x34000000\n\t"
      "v_rcp_f32 %[t], %[t]\n\t"
      "s_nop 0\n\t"
      "v_mul_f32 %[t], %[mp], %[t]\n\t"
      "v_fmac_f32 %[ax], %[t], %[dxp]\n\t"
      "v_fmac_f32 %[ay], %[t], %[dyp]\n\t"
      "v_fmac_f32 %[az], %[t], %[dzp]"
      : [t] "=&v"(t), [ax] "+v"(ax), [ay] "+v"(ay), [az] "+v"(az)
      : [mp] "v"(mp), [r2p] "v"(c.r2), [yp] "v"(c.y), [dxp] "v"(c.dx), [dyp] "v"(c.dy), [dzp] "v"(c.dz));
}

// NT: targets reduced together (NT * D partial sums live per lane); KS: source records per lane held in registers at a
// time; NB: independent pair chains in flight
// (NB = 0: float 3D only — the pair scheduled by hand, k2_pair_step above; the form that ships for config 3)
template <typename T, int D, int NT, int KS, int NB>
__global__ __launch_bounds__(kBlock) void all_pairs_collapsed_kernel(const T* __restrict__ m, const T* __restrict__ x,
                                                                     T* __restrict__ a, T c, uint32_t sz,
                                                                     uint32_t tiles_per_block) {
  using rec_t = src_rec<T, D>;
  constexpr int TJ = kColTileJ<T>;
  constexpr int KJ = TJ / 64;
  __shared__ rec_t tile[TJ];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const pair_consts<T> pc;

  // 64 targets per wave: lane l owns target i0 + l
  const uint32_t i0   = (blockIdx.x * kWaves + wave) * 64;
  const uint32_t imy  = i0 + lane;
  const bool ivalid   = imy < sz;
  T xt[D], mine[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    xt[k]   = x[uint64_t(ivalid ? imy : 0u) * D + k];  // lanes past the end hold body 0's position: computed, never stored
    mine[k] = T(0);
  }
  const int ngroups = (i0 < sz) ? int((min(64u, sz - i0) + NT - 1) / NT) : 0;  // wave-uniform

  const uint32_t ntiles = (sz + TJ - 1) / TJ;
  const uint32_t t0     = blockIdx.y * tiles_per_block;
  const uint32_t t1     = min(ntiles, t0 + tiles_per_block);

  for (uint32_t t = t0; t < t1; ++t) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TJ / kBlock; ++q) {
      uint32_t slot = q * kBlock + threadIdx.x;
      uint64_t j    = uint64_t(t) * TJ + slot;
      rec_t r;
      if (j < sz) {
#pragma unroll
        for (int k = 0; k < D; ++k) r.p[k] = x[j * D + k];
        r.m = m[j];
      } else {
#pragma unroll
        for (int k = 0; k < D; ++k) r.p[k] = T(0);
        r.m = T(0);
      }
      if (D == 2) r.p[2] = T(0);
      tile[slot] = r;
    }
    __syncthreads();

    // Per group of NT targets: the lane's KJ sources of the tile pass through registers in SUBS batches of KS (re-read from
    // LDS per group: 64 VGPRs of sources at once left no room for independent pair chains), the NT * D partial sums
    // stay in registers over the whole tile and are reduced across the wavefront once per (group, tile).
    constexpr int SUBS = KJ / KS;
    for (int g = 0; g < ngroups; ++g) {
      T xg[NT][D];  // wave-uniform: the group's target positions, broadcast into SGPRs once per tile
#pragma unroll
      for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int k = 0; k < D; ++k) xg[tt][k] = lane_bcast(xt[k], g * NT + tt);
      T part[D][NT];
      // f64: first with the reciprocal-free weight and no near-pair handling at all; a (group, tile) block that held a pair
      // closer than 2^-8 — the tile with the group's own bodies, a very close pair — is recomputed with the guarded form
      bool guarded = sizeof(T) == 4;
      for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int k = 0; k < D; ++k)
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) part[k][tt] = T(0);
        uint32_t lowest = 0xffffffffu;
#pragma unroll 1
        for (int sub = 0; sub < SUBS; ++sub) {
          rec_t src[KS];
#pragma unroll
          for (int q = 0; q < KS; ++q) src[q] = tile[(sub * KS + q) * 64 + lane];
          if constexpr (NB == 0) {
            static_assert(NB != 0 || (sizeof(T) == 4 && D == 3), "the hand-scheduled pair is float 3D");
            // the NT * KS pairs of this batch as one software pipeline: pair p = (target p / KS, source p % KS)
            k2_carry cy = k2_pair_head(src[0], xg[0]);
#pragma unroll
            for (int p = 1; p < NT * KS; ++p) {
              const int tp = (p - 1) / KS;
              cy = k2_pair_step(src[p % KS], xg[p / KS], src[(p - 1) % KS].m, cy, part[0][tp], part[1][tp], part[2][tp]);
            }
            k2_pair_tail(src[KS - 1].m, cy, part[0][NT - 1], part[1][NT - 1], part[2][NT - 1]);
          } else
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) {
            T pt[D];
#pragma unroll
            for (int k = 0; k < D; ++k) pt[k] = part[k][tt];
            if constexpr (sizeof(T) == 8) {
              if (guarded) {
#pragma unroll
                for (int q = 0; q < KS; q += NB) pair_accumulate_multi<T, D, NB>(pt, xg[tt], &src[q]);
              } else {
#pragma unroll
                for (int q = 0; q < KS; q += NB) pair_accumulate_far<D, NB>(pt, xg[tt], &src[q], lowest, pc.k15, pc.k1875);
              }
            } else {
#pragma unroll
              for (int q = 0; q < KS; q += NB) pair_accumulate_multi<T, D, NB>(pt, xg[tt], &src[q]);
            }
#pragma unroll
            for (int k = 0; k < D; ++k) part[k][tt] = pt[k];
          }
        }
        if (guarded || __builtin_amdgcn_ballot_w64(lowest < pair_math<double>::near_hi) == 0ull) break;
        guarded = true;  // wave-uniform
      }
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const T tot = transpose_reduce<T, NT>(part[k], lane);  // lane l: target g*NT + l % NT, summed over the wave
        mine[k] += (lane / NT == g) ? tot : T(0);
      }
    }
  }

  if (ivalid && t0 < t1) {
#pragma unroll
    for (int k = 0; k < D; ++k) atomicAdd(&a[uint64_t(imy) * D + k], c * mine[k]);
  }
}

// ---- K2, float 3D: the streamed form (round 6; what ships for config 3) ---------------------------------------------------
// The tile form above pays per (group of 16 targets, tile of 2048 sources) for 48 v_readlane (the targets into SGPRs), 48 zeroed
// partial sums and a transposed reduction (~150 instructions), i.e. 0.5 instructions per pair on top of the pair's fourteen,
// plus the staging of every tile through LDS behind two block barriers.  Here a WAVE owns one group of 16 targets for its whole
// source chunk: the targets go into SGPRs once, the 48 partial sums live in registers until the chunk is through, and the wave
// reduces and adds atomically once.  Sources are the packed (x, y, z, m) records (one coalesced global_load_dwordx4 per 64 sources
// and 16 pairs per lane, straight from L2 — the 4 MB of config 3 fit every XCD's L2 —: no LDS, no barrier), two batches of KS
// records per lane in registers, the next one in flight while this one is consumed; the pairs of the whole chunk form ONE
// software pipeline of k2_pair_step blocks (head of pair p with the tail of pair p - 1, above).  Lanes run along the sources and
// the wavefront reduction stays what north_star asks of the collapsed variant.
template <typename T, int D>
__global__ __launch_bounds__(kBlock) void collapsed_reset_pack_kernel(T* __restrict__ a, const T* __restrict__ ao, uint64_t nelem,
                                                                      const T* __restrict__ m, const T* __restrict__ x,
                                                                      src_rec<T, D>* __restrict__ packed, uint32_t sz, uint32_t padded) {
  const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (e < nelem) a[e] = a[e] - ao[e];  // diagonal pairs of the reference (src/all_pairs.h:35-40): a[i] -= ao[i]
  if (e < padded) {                    // records past the end carry mass 0 at the origin: their pairs add exactly 0
    src_rec<T, D> r;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.p[k] = (k < D && e < sz) ? x[e * D + k] : T(0);
    r.m       = e < sz ? m[e] : T(0);
    packed[e] = r;
  }
}

constexpr int kK2Group = 16;  // targets per wave of the streamed form
template <int KS>
__global__ __launch_bounds__(kBlock) void all_pairs_collapsed_stream_kernel(const src_rec<float, 3>* __restrict__ packed,
                                                                            const float* __restrict__ x, float* __restrict__ a, float c,
                                                                            uint32_t sz, uint32_t batches_per_chunk, uint32_t nbatches) {
  using rec_t       = src_rec<float, 3>;
  constexpr int NT  = kK2Group;
  const int lane    = threadIdx.x & 63;
  const uint32_t g  = (blockIdx.x * kWaves + (threadIdx.x >> 6));  // this wave's group of 16 targets
  const uint32_t i0 = g * NT;
  if (i0 >= sz) return;  // wave-uniform (no barrier in this kernel)
  // the group's positions: lane l < 16 loads target i0 + l (body 0's for targets past the end: computed, never stored), then SGPRs
  float xt[3];
  {
    const uint32_t i = (lane < NT && i0 + lane < sz) ? i0 + lane : 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) xt[k] = x[uint64_t(i) * 3 + k];
  }
  float xg[NT][3];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt)
#pragma unroll
    for (int k = 0; k < 3; ++k) xg[tt][k] = lane_bcast(xt[k], tt);
  const uint32_t b0 = blockIdx.y * batches_per_chunk, b1 = min(nbatches, b0 + batches_per_chunk);
  if (b0 >= b1) return;
  float part[3][NT];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) part[k][tt] = 0.0f;
  // batch b = records [b * 64 * KS, (b + 1) * 64 * KS): lane l holds records b * 64 * KS + q * 64 + l, q < KS
  auto fetch = [&](rec_t (&dst)[KS], uint32_t b) {
    const rec_t* base = packed + (uint64_t(b) * (64 * KS) + lane);
#pragma unroll
    for (int q = 0; q < KS; ++q) dst[q] = base[q * 64];
  };
  rec_t cur[KS], nxt[KS];
  fetch(cur, b0);
  k2_carry cy = k2_pair_head(cur[0], xg[0]);
  float mp    = cur[0].m;
  // one batch against the 16 targets; its first pair's head has been issued already (by the prologue or by the batch before).
  // (Macros, not lambdas over array references: a pointer to a buffer makes hipcc keep both buffers in scratch memory.)
#define K2S_CONSUME(SRC)                                                                                       \
  _Pragma("unroll") for (int p = 1; p < NT * KS; ++p) {                                                        \
    const int tp = (p - 1) / KS;                                                                               \
    cy           = k2_pair_step(SRC[p % KS], xg[p / KS], mp, cy, part[0][tp], part[1][tp], part[2][tp]);       \
    mp           = SRC[p % KS].m;                                                                              \
  }
  // the last pair's tail rides on the head of the next batch's first pair
#define K2S_BRIDGE(NEXT)                                                                                       \
  cy = k2_pair_step(NEXT[0], xg[0], mp, cy, part[0][NT - 1], part[1][NT - 1], part[2][NT - 1]);                \
  mp = NEXT[0].m;
  // two batches per trip so that the two register buffers swap without copies; a chunk is an even number of batches (the host
  // pads the record array with zero-mass records to that), and the last trip fetches its own second batch again instead of one
  // past the chunk: the head that rides on the last bridge belongs to no pair and is dropped with the wave
  for (uint32_t b = b0; b < b1; b += 2) {
    fetch(nxt, b + 1);
    K2S_CONSUME(cur)
    K2S_BRIDGE(nxt)
    fetch(cur, b + 2 < b1 ? b + 2 : b + 1);
    K2S_CONSUME(nxt)
    K2S_BRIDGE(cur)
  }
#undef K2S_CONSUME
#undef K2S_BRIDGE
  float tot[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) tot[k] = transpose_reduce<float, NT>(part[k], lane);  // lane l: target i0 + l % 16, summed over the wave
  if (lane < NT && i0 + lane < sz) {
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&a[uint64_t(i0 + lane) * 3 + k], c * tot[k]);
  }
}

// The same shape with the pair left to the compiler (K1's pair_batch: one target from SGPRs against U per-lane sources, the dense
// rule — K2 has no rule pre-pass): float 2D, and float 3D as the A/B of the hand-scheduled pair.
template <typename T, int D, int KS>
__global__ __launch_bounds__(kBlock) void all_pairs_collapsed_stream_cxx_kernel(const src_rec<T, D>* __restrict__ packed,
                                                                                const T* __restrict__ x, T* __restrict__ a, T c, uint32_t sz,
                                                                                uint32_t batches_per_chunk, uint32_t nbatches) {
  using rec_t      = src_rec<T, D>;
  constexpr int NT = sizeof(T) == 4 ? 16 : 8;
  constexpr int U  = 64 / int(sizeof(rec_t));  // records per pair_batch call: 4 in float, 2 in double
  static_assert(KS % U == 0, "whole pair batches");
  static_assert(sizeof(T) == 4, "float only: see collapsed_dispatch");
  const int lane    = threadIdx.x & 63;
  const uint32_t g  = (blockIdx.x * kWaves + (threadIdx.x >> 6));
  const uint32_t i0 = g * NT;
  if (i0 >= sz) return;  // wave-uniform (no barrier in this kernel)
  T xt[D];
  {
    const uint32_t i = (lane < NT && i0 + lane < sz) ? i0 + lane : 0u;
#pragma unroll
    for (int k = 0; k < D; ++k) xt[k] = x[uint64_t(i) * D + k];
  }
  T xg[NT][D];
#pragma unroll
  for (int tt = 0; tt < NT; ++tt)
#pragma unroll
    for (int k = 0; k < D; ++k) xg[tt][k] = lane_bcast(xt[k], tt);
  const uint32_t b0 = blockIdx.y * batches_per_chunk, b1 = min(nbatches, b0 + batches_per_chunk);
  if (b0 >= b1) return;
  const pair_consts<T> pc;
  T part[D][NT];
#pragma unroll
  for (int k = 0; k < D; ++k)
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) part[k][tt] = T(0);
  rec_t cur[KS], nxt[KS];
#define K2S_FETCH(DST, B)                                                       \
  {                                                                             \
    const rec_t* base = packed + (uint64_t(B) * (64 * KS) + lane);              \
    _Pragma("unroll") for (int q = 0; q < KS; ++q) DST[q] = base[q * 64];       \
  }
#define K2S_CONSUME(SRC)                                                                              \
  _Pragma("unroll") for (int tt = 0; tt < NT; ++tt) {                                                 \
    T acc1[1][D], xi1[1][D];                                                                          \
    _Pragma("unroll") for (int k = 0; k < D; ++k) acc1[0][k] = part[k][tt], xi1[0][k] = xg[tt][k];    \
    _Pragma("unroll") for (int q = 0; q < KS; q += U) {                                               \
      rec_t su[U];                                                                                    \
      _Pragma("unroll") for (int u = 0; u < U; ++u) su[u] = SRC[q + u];                               \
      pair_batch<T, D, 1, U, false>(acc1, xi1, su, pc);                                               \
    }                                                                                                 \
    _Pragma("unroll") for (int k = 0; k < D; ++k) part[k][tt] = acc1[0][k];                           \
  }
  K2S_FETCH(cur, b0)
  for (uint32_t b = b0; b < b1; b += 2) {  // an even number of batches per chunk (see the float 3D kernel)
    K2S_FETCH(nxt, b + 1)
    K2S_CONSUME(cur)
    K2S_FETCH(cur, (b + 2 < b1 ? b + 2 : b + 1))
    K2S_CONSUME(nxt)
  }
#undef K2S_FETCH
#undef K2S_CONSUME
  T tot[D];
#pragma unroll
  for (int k = 0; k < D; ++k) tot[k] = transpose_reduce<T, NT>(part[k], lane);  // lane l: target i0 + l % NT, summed over the wave
  if (lane < NT && i0 + lane < sz) {
#pragma unroll
    for (int k = 0; k < D; ++k) atomicAdd(&a[uint64_t(i0 + lane) * D + k], c * tot[k]);
  }
}

// K2's launch as a function of (T, D, sz) and — in -DNBODY_EXPERIMENTS builds — of the two switches the dispatch reads: everything
// the launches below take from here and nothing else, and what nbody_all_pairs_collapsed_describe prints (the pattern of k1_plan).
//   form: 20 = float 3D streamed with the hand-scheduled pair, 8 records per lane and batch (21: 4); 22 / 23 / 24 = the streamed
//   compiler-scheduled kernel with 8 / 4 / 2 records per lane and batch (never fewer than one pair_batch call: 4 in float); any
//   other value names a tile shape (NT, KS, NB), see below.  What ships: float 3D 20, float 2D 23, double the tile shape 5.
struct k2_plan {
  bool stream = false, hand = false;
  // streamed form: records per lane and batch, the padded record count, its batches of 64 * ks, source chunks (grid.y) and batches
  // per chunk (even: the kernel takes two per trip)
  int ks = 0;
  uint32_t padded = 0, nbatches = 0, chunks = 0, bpc = 0, groups = 0;
  // tile form: blocks of 256 targets (grid.x), source tiles of kColTileJ, block rows (grid.y) of tpb tiles each
  int nt = 0, nb = 0;  // with ks: the kernel's (NT, KS, NB)
  uint32_t iblocks = 0, ntiles = 0, ysplit = 0, tpb = 0;
};

template <typename T, int D>
constexpr int k2_shipped_form() {
  return sizeof(T) == 4 ? (D == 3 ? 20 : 23) : 5;
}

template <typename T, int D>
static void plan_collapsed(uint32_t sz, int form, uint32_t want_chunks, k2_plan* out) {
  k2_plan p;
  // (float only: in double the per-batch near-pair branch of pair_batch under the full unroll over targets x sources makes hipcc keep
  // every chain's temporaries alive — 264 ... 512 VGPRs and scratch for <double, 3, 2 ... 8> —; double keeps the tile form)
  p.stream = sizeof(T) == 4 && ((form >= 22 && form <= 24) || (D == 3 && (form == 20 || form == 21)));
  if (p.stream) {
    using rec_t      = src_rec<T, D>;
    constexpr int NT = sizeof(T) == 4 ? 16 : 8;
    constexpr int U  = 64 / int(sizeof(rec_t));
    p.hand           = form == 20 || form == 21;
    p.ks             = form == 20 || form == 22 ? 8 : (form == 24 ? 2 : 4);
    if (p.ks < U) p.ks = U;
    const uint32_t pair_of_batches = 2u * 64u * uint32_t(p.ks);  // at most 1024 records: what ap_scratch_reserve pads a context's buffer to
    p.padded   = (sz + pair_of_batches - 1) / pair_of_batches * pair_of_batches;
    p.groups   = (sz + NT - 1) / NT;
    p.nbatches = p.padded / uint32_t(64 * p.ks);
    // chunks: enough waves for >= 16 rounds of the chip's 4096 wave slots where the system allows, whole batches per chunk
    uint32_t chunks = want_chunks ? want_chunks : (p.groups ? (16u * 4096u + p.groups - 1) / p.groups : 1u);
    chunks          = std::max(1u, std::min({chunks, p.nbatches, 65535u}));
    p.bpc           = (p.nbatches + chunks - 1) / chunks;
    p.bpc += p.bpc & 1u;  // an even number of batches per chunk (nbatches is even)
    p.chunks = p.bpc ? (p.nbatches + p.bpc - 1) / p.bpc : 0;
    *out     = p;
    return;
  }
  p.iblocks = (sz + kWaves * 64 - 1) / (kWaves * 64);
  p.ntiles  = (sz + kColTileJ<T> - 1) / kColTileJ<T>;
  // aim for >= 4096 blocks (16 per CU) while keeping >= 1 tile per block
  uint32_t ysplit = p.iblocks ? (4096 + p.iblocks - 1) / p.iblocks : 1;
  if (ysplit > p.ntiles) ysplit = p.ntiles;
  if (ysplit < 1) ysplit = 1;
  if (ysplit > 65535) ysplit = 65535;
  p.tpb    = (p.ntiles + ysplit - 1) / ysplit;
  p.ysplit = p.tpb ? (p.ntiles + p.tpb - 1) / p.tpb : 1;
  // Measured at config 3 (f32, N = 262 144) and on the reference's matrix size (f64, N = 10^5), gpurun_out/r02/k2_times*.txt:
  // every variant with ONE pair chain per lane in flight runs at 24.05 ms (36.3 % of the FP32 vector peak) whatever NT, KS
  // and the occupancy (3 to 6 waves per SIMD); every variant that interleaves 2 or 4 chains runs at 28.7 ms — the interleaved
  // order puts v_rsq_f32 and v_rcp_f32 back to back.  Round 5, same box, cfg (16, 8, 1) 23.87 ms: the next tile's records prefetched
  // into registers while this one is consumed 23.85 (the staging is not what stalls); the target's eight chains software-pipelined with
  // sched_group_barrier (6 VALU, 1 transcendental, ...; one scheduling region per target: over the whole block of 128 pairs hipcc did
  // not finish in 30 minutes) 27.8 — independent chains side by side are SLOWER than one chain with its two wait states, again.
  // f64 (N = 10^5, ms): with the guarded rsq+rcp weight everywhere (8, 4, 4) was
  // the fastest at 7.47; with the reciprocal-free weight and a guarded second pass only for the blocks that held a near pair
  // (see the kernel) (8, 8, 1) 6.79, (8, 4, 1) 6.95, (8, 4, 2) 7.00, (8, 2, 2) 7.01, (8, 2, 1) 7.26, (16, 8, 1) 8.03, (8, 4, 4) 9.96.
  const int cfg = form >= 20 ? (sizeof(T) == 4 ? 0 : 5) : form;  // a streamed form this (T, D) does not have: the tile form as shipped
  auto shape    = [&](int nt, int ks, int nb) { p.nt = nt, p.ks = ks, p.nb = nb; };
  shape(16, 8, 4);
  if (sizeof(T) == 4 && D == 3 && (cfg == 0 || (cfg >= 10 && cfg <= 12))) {
    // NB = 0, the pair scheduled by hand (k2_pair_step): the tile form of float 3D
    if (cfg == 0) shape(16, 8, 0);
    if (cfg == 10) shape(16, 4, 0);
    if (cfg == 11) shape(8, 8, 0);
    if (cfg == 12) shape(8, 4, 0);
  } else if (cfg == 0 || (sizeof(T) == 4 && D == 3 && cfg == 8)) {
    shape(16, 8, 1);  // (float 3D, 8: the compiler-scheduled cross-check of the hand-scheduled form)
  } else {
    if (cfg == 1) shape(8, 4, 4);
    if (cfg == 2) shape(8, 4, 1);
    if (cfg == 4) shape(8, 4, 2);
    if (cfg == 5) shape(8, 8, 1);
    if (cfg == 6) shape(8, 2, 1);
    if (cfg == 7) shape(8, 2, 2);
  }
  *out = p;
}

template <typename T, int D>
static int collapsed_stream_launch(const nbody_state* s, hipStream_t st, const k2_plan& p) {
  using rec_t = src_rec<T, D>;
  void* q     = nullptr;
  if (int r = ap_scratch_get(st, 0, sizeof(rec_t) * size_t(p.padded), &q)) return r;
  rec_t* packed        = static_cast<rec_t*>(q);
  const uint64_t nelem = uint64_t(s->sz) * D;
  const uint64_t work  = nelem > p.padded ? nelem : p.padded;
  hipLaunchKernelGGL((collapsed_reset_pack_kernel<T, D>), dim3((work + kBlock - 1) / kBlock), dim3(kBlock), 0, st,
                     static_cast<T*>(s->a), static_cast<const T*>(s->ao), nelem, static_cast<const T*>(s->m),
                     static_cast<const T*>(s->x), packed, s->sz, p.padded);
  NB_HIP(hipGetLastError());
  const uint32_t blocks = (p.groups + kWaves - 1) / kWaves;
  const dim3 grid(blocks, p.chunks), block(kBlock);
  const T* x = static_cast<const T*>(s->x);
  T* a       = static_cast<T*>(s->a);
  const T c  = static_cast<T>(s->c);
  if constexpr (sizeof(T) == 4 && D == 3) {
    if (p.hand && p.ks == 8) hipLaunchKernelGGL((all_pairs_collapsed_stream_kernel<8>), grid, block, 0, st, packed, x, a, c, s->sz, p.bpc, p.nbatches);
    if (p.hand && p.ks == 4) hipLaunchKernelGGL((all_pairs_collapsed_stream_kernel<4>), grid, block, 0, st, packed, x, a, c, s->sz, p.bpc, p.nbatches);
  }
  if (!p.hand) {
    constexpr int U = 64 / int(sizeof(rec_t));
    if (p.ks == 8) hipLaunchKernelGGL((all_pairs_collapsed_stream_cxx_kernel<T, D, 8>), grid, block, 0, st, packed, x, a, c, s->sz, p.bpc, p.nbatches);
    else if (p.ks == 4) hipLaunchKernelGGL((all_pairs_collapsed_stream_cxx_kernel<T, D, 4>), grid, block, 0, st, packed, x, a, c, s->sz, p.bpc, p.nbatches);
    else hipLaunchKernelGGL((all_pairs_collapsed_stream_cxx_kernel<T, D, (U <= 2 ? 2 : 4)>), grid, block, 0, st, packed, x, a, c, s->sz, p.bpc, p.nbatches);
  }
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

template <typename T, int D>
static int collapsed_tile_launch(const nbody_state* s, hipStream_t st, const k2_plan& p) {
  uint64_t nelem = uint64_t(s->sz) * D;
  hipLaunchKernelGGL((collapsed_reset_kernel<T, D>), dim3((nelem + kBlock - 1) / kBlock), dim3(kBlock), 0, st,
                     static_cast<T*>(s->a), static_cast<const T*>(s->ao), nelem);
  NB_HIP(hipGetLastError());
  bool found = false;
#define NB_K2(NT, KS, NBC)                                                                                                 \
  if (!found && p.nt == NT && p.ks == KS && p.nb == NBC) {                                                                 \
    found = true;                                                                                                          \
    hipLaunchKernelGGL((all_pairs_collapsed_kernel<T, D, NT, KS, NBC>), dim3(p.iblocks, p.ysplit), dim3(kBlock), 0, st,     \
                       static_cast<const T*>(s->m), static_cast<const T*>(s->x), static_cast<T*>(s->a), static_cast<T>(s->c), \
                       s->sz, p.tpb);                                                                                      \
  }
  if constexpr (sizeof(T) == 4 && D == 3) {  // the pair scheduled by hand (k2_pair_step)
    NB_K2(16, 8, 0)
    NB_K2(16, 4, 0)
    NB_K2(8, 8, 0)
    NB_K2(8, 4, 0)
  }
  NB_K2(16, 8, 1)
  NB_K2(8, 4, 4)
  NB_K2(8, 4, 1)
  NB_K2(8, 4, 2)
  NB_K2(8, 8, 1)
  NB_K2(8, 2, 1)
  NB_K2(8, 2, 2)
  NB_K2(16, 8, 4)
#undef NB_K2
  if (!found) {
    set_error("all-pairs-collapsed: no kernel for the tile shape (%d, %d, %d)", p.nt, p.ks, p.nb);
    return NBODY_ERR_ARG;
  }
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

// The plan of this build for a state: the shipped form, or in -DNBODY_EXPERIMENTS builds what the two switches select
// (tools/time_collapsed.py).  float: the streamed form — 3D (config 3) with the hand-scheduled pair, 2D with the compiled one, 4 records
// per lane and batch (N = 10^4 2D: 0.043 ms against the tile form's 0.060, profiles/r06/k2_streamed_form_2.txt); double: the tile form.
template <typename T, int D>
static k2_plan collapsed_plan_of(const nbody_state* s) {
  int form        = k2_shipped_form<T, D>();
  uint32_t chunks = 0;
  if (const char* e = experiment_env("NBODY_K2_CFG")) form = atoi(e);  // -DNBODY_EXPERIMENTS builds only
  if (const char* e = experiment_env("NBODY_K2_CHUNKS")) chunks = uint32_t(atoi(e));
  k2_plan p;
  plan_collapsed<T, D>(s->sz, form, chunks, &p);
  return p;
}

template <typename T, int D>
static int collapsed_dispatch(const nbody_state* s, hipStream_t st) {
  NB_ARG(s->first == 0 && s->count == s->sz, "all-pairs-collapsed is single-GPU: needs first=0, count=sz");
  if (s->sz == 0) return NBODY_OK;
  const k2_plan p = collapsed_plan_of<T, D>(s);
  if constexpr (sizeof(T) == 4)
    if (p.stream) return collapsed_stream_launch<T, D>(s, st, p);
  return collapsed_tile_launch<T, D>(s, st, p);
}

template <typename T, int D>
static int collapsed_describe(const nbody_state* s, char* out, size_t len) {
  NB_ARG(s->first == 0 && s->count == s->sz, "all-pairs-collapsed is single-GPU: needs first=0, count=sz");
  const char* t = sizeof(T) == 8 ? "double" : "float";
  if (s->sz == 0) {
    snprintf(out, len, "all-pairs-collapsed %s %d: no bodies, no launch", t, D);
    return NBODY_OK;
  }
  const k2_plan p = collapsed_plan_of<T, D>(s);
  if (p.stream && p.hand)
    snprintf(out, len, "all_pairs_collapsed_stream_kernel<%d> hand %s %d padded=%u nbatches=%u bpc=%u chunks=%u", p.ks, t, D, p.padded,
             p.nbatches, p.bpc, p.chunks);
  else if (p.stream)
    snprintf(out, len, "all_pairs_collapsed_stream_cxx_kernel<%s,%d,%d> compiled %s %d padded=%u nbatches=%u bpc=%u chunks=%u", t, D, p.ks, t,
             D, p.padded, p.nbatches, p.bpc, p.chunks);
  else
    snprintf(out, len, "all_pairs_collapsed_kernel<%s,%d,NT=%d,KS=%d,NB=%d> tile=%d iblocks=%u ntiles=%u tpb=%u ysplit=%u", t, D, p.nt, p.ks,
             p.nb, kColTileJ<T>, p.iblocks, p.ntiles, p.tpb, p.ysplit);
  return NBODY_OK;
}

// ------------------------------------------------------------------------------------------------
// K3
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void accelerate_step_kernel(T* __restrict__ x, T* __restrict__ v, const T* __restrict__ a,
                                                                 T* __restrict__ ao, T dt, uint64_t n) {
#pragma clang fp contract(off)
  const T hdt   = T(0.5) * dt;
  const T hdtdt = hdt * dt;
  for (uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x; e < n; e += uint64_t(gridDim.x) * kBlock) {
    T ae = a[e], aoe = ao[e], ve = v[e];
    T t1 = dt * ve;
    T t2 = hdtdt * aoe;
    x[e] = x[e] + (t1 + t2);
    v[e] = ve + hdt * (ae + aoe);
    ao[e] = ae;
  }
}

template <typename T, int D>
static int accelerate_dispatch(const nbody_state* s, hipStream_t st) {
  uint64_t n = uint64_t(s->count) * D;
  if (n == 0) return NBODY_OK;
  uint64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride the rest
  T* xloc = static_cast<T*>(s->x) + uint64_t(s->first) * D;
  hipLaunchKernelGGL((accelerate_step_kernel<T>), dim3(uint32_t(blocks)), dim3(kBlock), 0, st, xloc, static_cast<T*>(s->v),
                     static_cast<const T*>(s->a), static_cast<T*>(s->ao), static_cast<T>(s->dt), n);
  NB_HIP(hipGetLastError());
  return NBODY_OK;
}

}  // namespace nbody

// ---- C ABI ------------------------------------------------------------------------------------------
using namespace nbody;

extern "C" int nbody_all_pairs_configure(int split, int targets_per_thread) {
  const uint32_t cur = g_ap_default.load(std::memory_order_relaxed);
  if (int r = check_tuning(split, targets_per_thread, int((cur >> 6) & 3u))) return r;
  uint32_t want = (cur & (3u << 6)) | uint32_t(split & 15) | (uint32_t(targets_per_thread & 3) << 4);
  g_ap_default.store(want, std::memory_order_relaxed);
  return NBODY_OK;
}

extern "C" int nbody_all_pairs_source_path(int mode) {
  if (int r = check_tuning(0, 0, mode)) return r;
  uint32_t cur = g_ap_default.load(std::memory_order_relaxed);
  while (!g_ap_default.compare_exchange_weak(cur, (cur & ~(3u << 6)) | (uint32_t(mode) << 6), std::memory_order_relaxed)) {
  }
  return NBODY_OK;
}

extern "C" int nbody_all_pairs_describe(const nbody_state* s, char* out, size_t len) {
  NB_ARG(out != nullptr && len > 0, "out is NULL");
  if (int r = check_state(s)) return r;
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using TG = decltype(tg);
    return all_pairs_describe<typename TG::type, TG::dim>(s, out, len);
  });
}

extern "C" int nbody_all_pairs_pair_rule(const nbody_state* s, void* stream, int* sparse_out, double* volume_out) {
  NB_ARG(sparse_out != nullptr, "sparse_out is NULL");
  if (int r = check_state(s)) return r;
  device_guard guard(stream_device(as_stream(stream)));
  *sparse_out = 0;
  if (volume_out) *volume_out = 0.0;
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using T         = typename decltype(tg)::type;
    constexpr int D = decltype(tg)::dim;
    const k1_rule* rule = nullptr;
    if (int r = ap_prepare<T, D>(s, as_stream(stream), false, nullptr, nullptr, &rule, nullptr, 0)) return r;
    if (rule == nullptr) return int(NBODY_OK);  // below kFarMinBodies: the dense rule by definition
    k1_rule host;
    NB_HIP(hipMemcpyAsync(&host, rule, sizeof host, hipMemcpyDeviceToHost, as_stream(stream)));
    NB_HIP(hipStreamSynchronize(as_stream(stream)));
    *sparse_out = host.sparse ? 1 : 0;
    if (volume_out) *volume_out = host.volume;
    return int(NBODY_OK);
  });
}

extern "C" int nbody_all_pairs_force(const nbody_state* s, void* stream) {
  if (int r = check_state(s)) return r;
  device_guard guard(stream_device(as_stream(stream)));
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using TG = decltype(tg);
    return all_pairs_dispatch<typename TG::type, TG::dim>(s, as_stream(stream));
  });
}

extern "C" int nbody_all_pairs_softened_force(const nbody_state* s, double eps, void* stream) {
  if (int r = check_state(s)) return r;
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using TG = decltype(tg);
    using T  = typename TG::type;
    T e2;
    if (int r = check_softening<T>(eps, &e2)) return r;
    device_guard guard(stream_device(as_stream(stream)));
    return all_pairs_dispatch<T, TG::dim, true>(s, as_stream(stream), e2);
  });
}

extern "C" int nbody_all_pairs_status(void* stream, uint64_t out[6], int clear) {
  device_guard guard(stream_device(as_stream(stream)));
  unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
  const int rc = ap_status_read(as_stream(stream), v, clear != 0);
  if (out)
    for (int i = 0; i < 6; ++i) out[i] = v[i];
  return rc;
}

#ifdef NBODY_EXPERIMENTS
// Experiments build only (tests/test_gpu_far_certificate.py): the number of (target group, source chunk) blocks that K1 launches of
// this stream have certified far since the count was last cleared.  Waits for the stream.
extern "C" int nbody_exp_k1_certified(void* stream, uint64_t* out, int clear) {
  NB_ARG(out != nullptr, "out is NULL");
  hipStream_t st = as_stream(stream);
  const int dev  = stream_device(st);
  device_guard guard(dev);
  void* dptr = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_packed_mu);
    for (auto& sl : g_packed_slots)
      if (sl.stream == st && sl.device == dev) dptr = sl.buf[7].ptr;
  }
  unsigned long long v = 0;
  if (dptr) NB_HIP(hipMemcpyAsync(&v, dptr, sizeof v, hipMemcpyDeviceToHost, st));
  NB_HIP(hipStreamSynchronize(st));
  if (dptr && clear) {
    NB_HIP(hipMemsetAsync(dptr, 0, sizeof v, st));
    NB_HIP(hipStreamSynchronize(st));
  }
  *out = v;
  return NBODY_OK;
}
#endif

extern "C" int nbody_all_pairs_collapsed_force(const nbody_state* s, void* stream) {
  if (int r = check_state(s)) return r;
  device_guard guard(stream_device(as_stream(stream)));
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using TG = decltype(tg);
    return collapsed_dispatch<typename TG::type, TG::dim>(s, as_stream(stream));
  });
}

extern "C" int nbody_all_pairs_collapsed_describe(const nbody_state* s, char* out, size_t len) {
  NB_ARG(out != nullptr && len > 0, "out is NULL");
  if (int r = check_state(s)) return r;
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using TG = decltype(tg);
    return collapsed_describe<typename TG::type, TG::dim>(s, out, len);
  });
}

extern "C" int nbody_accelerate_step(const nbody_state* s, void* stream) {
  if (int r = check_state(s)) return r;
  device_guard guard(stream_device(as_stream(stream)));
  return dispatch(s->dtype, s->dim, [&](auto tg) {
    using TG = decltype(tg);
    return accelerate_dispatch<typename TG::type, TG::dim>(s, as_stream(stream));
  });
}
