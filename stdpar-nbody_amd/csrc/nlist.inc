// Exact fixed-radius neighbour lists on the neighbour tree: nbody_nlist_* of include/nbody_hip.h.  No reference counterpart.  Included
// from knn.hip, inside namespace nbody, after fof.inc; it uses nntree.inc's structure (sorted records, buckets, boxes,
// nntree_structure_launch), bound and successor rule as they are, and nlist_plan.hpp's launch shapes.
// As in fof.inc no kernel here names nntree_rec / nntree_box in its parameters (tests count kernels by `nntree_`, `knn_` and `fof_`
// anywhere in the demangled signature): the sorted records and the boxes arrive as `const void* __restrict__` and are cast in the
// first lines; the head of fof.inc says why a by-value struct of typed pointers was not kept.
//
// Definitions (T the state's type, D its dimension):
//   neighbour  j is a neighbour of i iff j != i and d2_ij <= r2_i, d2 pair_d2's chain (pair_sweep.hpp).
//   r2_i       scalar radius: T(r) * T(r), rounded once on the host; per-body radii: v_i * v_i (or v_i, squared = 1), one multiply in T
//              on the host when the radii are set, kept as T[n] on the device.
//   count      uint32[n], |L_i| in body order; offset uint64[n + 1], its exclusive prefix sum; list uint32[total], L_i at
//              [offset[i], offset[i + 1]) in ascending ORIGINAL index; summary uint64[4]: total, the largest count, the lowest index
//              that has it, status (1: total > capacity, 2: the largest count > kNlMaxPerBody; either: no list this compute).
// Everything is an integer with one correct answer, and nothing below depends on scheduling, the body order or the keys:
//   walk       nlist_walk<T, D, Fill>, ONE function for the count and the fill pass, so the two cannot disagree on a bit.  One target
//              per lane, the 64 targets of a wave consecutive SORTED positions; no LDS, no barrier.  The cap is the lane's own r2_i,
//              loaded once through the record's original index; lanes past n carry -inf and never ask for anything.  A node is
//              skipped iff bound > r2_i in EVERY lane — strict, so a record at exactly r2_i is met; exact for the reason at the head
//              of nntree.inc (the bound is monotone in pair_d2's own chain: no epsilon).  The walk is FULL, every q != p on both
//              sides (a gather with per-body radii is not symmetric), and ends at the root or the first dead node.  The self pair
//              is out by sorted position, padding by q < n.  No divide, root or reciprocal.
//              Count: the lane's hits go to count[j], j the lane's original index.  Fill: the lane writes the original index of each
//              hit at its own cursor from offset[j] into scratch; a cursor stops at min(offset[j + 1], capacity) whatever happens.
//   scan       count -> offset by strips of kNlBlock bodies: a sum and a max of (count << 32) | ~index per strip, one block that
//              scans the strip sums in place and writes offset[n] and the summary — so the status is in memory BEFORE the fill is
//              launched —, and one pass that adds the in-strip prefix.  No decoupled look-back, no spin.
//   order      the fill leaves a segment in ascending sorted position.  One wave per body stages its segment in LDS (at most
//              kNlMaxPerBody entries, 16 KB) and places entry e at list[offset + rank(e)], rank(e) the number of the segment's
//              entries below e: the indices of a segment are distinct, so the ranks are 0 .. len - 1, each once.  A rank is < len
//              whatever the entries are, so no store leaves the segment.  len^2 / 64 compare steps per wave, 4 per LDS read.
//   The fill and the ordering read the status first and return at once if it is not 0.
// Why every loop ends: the walks visit nodes in strictly increasing successor order and stop at the root or a dead node; every other
// loop has a trip count fixed by n or by a count <= kNlMaxPerBody.  NO loop waits for another lane, wave or block.
// No atomics at all, nothing read back, nothing allocated after create: two computes give the same bits and a compute may be recorded.

constexpr uint32_t kNlStatusCapacity = 1u, kNlStatusPerBody = 2u;
// the plan's block is the tree's, and its padding (n rounded up to whole blocks) the packed records' (whole tiles of kHTile)
static_assert(kNlBlock == uint32_t(kNtBlock) && kNlBlock == uint32_t(kHTile) && kNlWave == 64u, "the plan's block is the tree's");

// ---- the walk ------------------------------------------------------------------------------------------------------------------
template <typename T, int D, bool Fill>
__device__ __forceinline__ void nlist_walk(const void* __restrict__ srt_, const void* __restrict__ boxes_, const T* __restrict__ radii, T r2,
                                           uint32_t n, uint32_t levels, uint32_t* __restrict__ count, const uint64_t* __restrict__ offset,
                                           uint32_t* __restrict__ scratch, uint64_t capacity) {
  const auto* srt     = static_cast<const nntree_rec<T>*>(srt_);
  const auto* boxes   = static_cast<const nntree_box<T>*>(boxes_);
  constexpr int U     = sizeof(T) == 8 ? 2 : 4;  // records a batch
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(blockIdx.x * (kNtBlock / 64) + (threadIdx.x >> 6))));
  if (wave * 64u >= n) return;             // wave-uniform
  const uint32_t tp = wave * 64u + lane;   // < padded: the sorted records are padded to whole blocks
  const bool live   = tp < n;

  T xi[D];
#pragma unroll
  for (int c = 0; c < D; ++c) xi[c] = srt[tp].p[c];
  const uint32_t self = live ? uint32_t(srt[tp].j) : 0u;      // the lane's original index
  const T cap         = live ? (radii ? radii[self] : r2) : -pair_inf<T>();  // r2_i; a dead lane never asks for a node or a record
  uint32_t hits       = 0u;
  uint64_t cur = 0ull, end = 0ull;
  if constexpr (Fill) {
    if (live) {
      cur = offset[self];
      end = offset[self + 1u];
      end = end < capacity ? end : capacity;  // no store at or beyond capacity, whatever the offsets hold
    }
  }

  uint32_t node = 1u;
#pragma unroll 1
  for (;;) {
    const uint32_t depth = 31u - uint32_t(__builtin_clz(node));
    const uint32_t sh    = levels - depth;
    const uint32_t first = (node - (1u << depth)) << sh;  // the node's first leaf
    const uint32_t q0    = first * uint32_t(kNtB);        // ... and its first sorted position
    if (q0 >= n) break;                                   // dead, and so is every node after it
    const T bound = nntree_bound<T, D>(boxes[node], xi);
    if (__builtin_amdgcn_ballot_w64(!(bound > cap)) != 0ull) {  // some lane needs the node
      if (sh != 0u) {
        node = 2u * node;
        continue;
      }
      const nntree_rec<T>* src = srt + size_t(first) * kNtB;
#pragma unroll 1
      for (int jj = 0; jj < kNtB; jj += U) {
#pragma unroll
        for (int b = 0; b < U; ++b) {
          T s[D];
#pragma unroll
          for (int c = 0; c < D; ++c) s[c] = src[jj + b].p[c];
          const T d2       = pair_d2<T, D>(s, xi);
          const uint32_t q = q0 + uint32_t(jj + b);
          const bool hit   = live && q < n && q != tp && d2 <= cap;  // padding and the self pair are out by position
          if constexpr (Fill) {
            if (hit && cur < end) {
              scratch[cur] = uint32_t(src[jj + b].j);
              ++cur;
            }
          } else {
            hits += hit ? 1u : 0u;
          }
        }
      }
    }
    node = (node + 1u) >> __builtin_ctz(node + 1u);  // skipped or finished: the same move
    if (node == 1u) break;
  }
  if constexpr (!Fill) {
    if (live) count[self] = hits;
  }
}

// grid: padded / kNtBlock blocks; every wave on its own.  radii: T[n] of r2_i in body order, or NULL for the scalar r2.
template <typename T, int D>
static __global__ __launch_bounds__(kNtBlock) void nlist_count_kernel(const void* __restrict__ srt_, const void* __restrict__ boxes_,
                                                                      const T* __restrict__ radii, T r2, uint32_t n, uint32_t levels,
                                                                      uint32_t* __restrict__ count) {
  nlist_walk<T, D, false>(srt_, boxes_, radii, r2, n, levels, count, nullptr, nullptr, 0ull);
}

template <typename T, int D>
static __global__ __launch_bounds__(kNtBlock) void nlist_fill_kernel(const void* __restrict__ srt_, const void* __restrict__ boxes_,
                                                                     const T* __restrict__ radii, T r2, uint32_t n, uint32_t levels,
                                                                     const uint64_t* __restrict__ offset, const uint64_t* __restrict__ summary,
                                                                     uint32_t* __restrict__ scratch, uint64_t capacity) {
  if (summary[3] != 0ull) return;  // the list does not fit: nothing is written
  nlist_walk<T, D, true>(srt_, boxes_, radii, r2, n, levels, nullptr, offset, scratch, capacity);
}

// ---- count -> offset, and the summary ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t nlist_wave_scan(uint64_t v, int lane) {  // inclusive, over the 64 lanes
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// grid: strips of kNtBlock bodies.  ssum[strip]: the strip's counts added; smax[strip]: its max of (count << 32) | ~index.
static __global__ __launch_bounds__(kNtBlock) void nlist_strip_kernel(const uint32_t* __restrict__ count, uint32_t n, uint64_t* __restrict__ ssum,
                                                                      uint64_t* __restrict__ smax) {
  __shared__ uint64_t ws[kNtBlock / 64], wm[kNtBlock / 64];
  const uint32_t i = blockIdx.x * kNtBlock + threadIdx.x;
  const uint32_t c = i < n ? count[i] : 0u;
  uint64_t s = c, m = i < n ? ((uint64_t(c) << 32) | uint64_t(~i)) : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, 64);
    const uint64_t o = __shfl_xor(m, off, 64);
    m                = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0) {
    ws[threadIdx.x >> 6] = s;
    wm[threadIdx.x >> 6] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kNtBlock / 64; ++w) {
      s += ws[w];
      m = wm[w] > m ? wm[w] : m;
    }
    ssum[blockIdx.x] = s;
    smax[blockIdx.x] = m;
  }
}

// one block: ssum[0 .. strips) -> its exclusive scan in place, `trips` rounds of kNlScanBlock; then offset[n] = the total and the
// summary: total, the largest count, the lowest index that has it, the status for this capacity.
static __global__ __launch_bounds__(kNlScanBlock) void nlist_scan_kernel(uint64_t* __restrict__ ssum, const uint64_t* __restrict__ smax,
                                                                         uint32_t strips, uint32_t trips, uint64_t capacity,
                                                                         uint64_t* __restrict__ offset_n, uint64_t* __restrict__ summary) {
  __shared__ uint64_t wsum[kNlScanBlock / 64], wbest[kNlScanBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t running = 0ull, best = 0ull;
  for (uint32_t trip = 0; trip < trips; ++trip) {
    const uint32_t j   = trip * kNlScanBlock + threadIdx.x;
    const uint64_t v   = j < strips ? ssum[j] : 0ull;
    const uint64_t m   = j < strips ? smax[j] : 0ull;
    best               = m > best ? m : best;
    const uint64_t inc = nlist_wave_scan(v, lane);
    __syncthreads();  // the previous round's wsum has been read
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint64_t before = 0ull, total = 0ull;
#pragma unroll
    for (int w = 0; w < int(kNlScanBlock / 64); ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (j < strips) ssum[j] = running + before + inc - v;
    running += total;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(best, off, 64);
    best             = o > best ? o : best;
  }
  if (lane == 0) wbest[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < int(kNlScanBlock / 64); ++w) best = wbest[w] > best ? wbest[w] : best;
    const uint64_t most = best >> 32;
    *offset_n           = running;
    summary[0]          = running;
    summary[1]          = most;
    summary[2]          = uint64_t(~uint32_t(best));
    summary[3]          = (running > capacity ? uint64_t(kNlStatusCapacity) : 0ull) | (most > uint64_t(kNlMaxPerBody) ? uint64_t(kNlStatusPerBody) : 0ull);
  }
}

// grid: the strips again.  soff: the scanned strip sums.
static __global__ __launch_bounds__(kNtBlock) void nlist_offsets_kernel(const uint32_t* __restrict__ count, const uint64_t* __restrict__ soff,
                                                                        uint32_t n, uint64_t* __restrict__ offset) {
  __shared__ uint64_t wsum[kNtBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i   = blockIdx.x * kNtBlock + threadIdx.x;
  const uint64_t c   = i < n ? uint64_t(count[i]) : 0ull;
  const uint64_t inc = nlist_wave_scan(c, lane);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint64_t before = soff[blockIdx.x];
  for (int w = 0; w < wave; ++w) before += wsum[w];
  if (i < n) offset[i] = before + inc - c;
}

// ---- segment order -------------------------------------------------------------------------------------------------------------
// grid: n blocks of one wave, body blockIdx.x.  scratch: the segments in ascending sorted position; list: in ascending index.
static __global__ __launch_bounds__(kNlWave) void nlist_order_kernel(const uint32_t* __restrict__ count, const uint64_t* __restrict__ offset,
                                                                     const uint64_t* __restrict__ summary, const uint32_t* __restrict__ scratch,
                                                                     uint32_t* __restrict__ list, uint64_t capacity) {
  __shared__ __attribute__((aligned(16))) uint32_t seg[kNlMaxPerBody];
  if (summary[3] != 0ull) return;  // the list does not fit: nothing is written
  const uint32_t lane = threadIdx.x;
  const uint32_t len  = count[blockIdx.x];
  const uint64_t beg  = offset[blockIdx.x];
  if (len == 0u || len > kNlMaxPerBody || beg + uint64_t(len) > capacity) return;  // block-uniform; the last two never with status 0
  const uint32_t len4 = (len + 3u) & ~3u;  // whole reads of four; the tail holds what is below no index
  for (uint32_t k = lane; k < len4; k += kNlWave) seg[k] = k < len ? scratch[beg + k] : kNoNeighbour;
  __syncthreads();
  const uint4* seg4 = reinterpret_cast<const uint4*>(seg);
  for (uint32_t base = 0; base < len; base += kNlWave) {
    const uint32_t e = base + lane;
    const uint32_t v = e < len ? seg[e] : 0u;
    uint32_t rank    = 0u;
    for (uint32_t k = 0; k < len4 / 4u; ++k) {  // one address for the whole wave: a broadcast
      const uint4 u = seg4[k];
      rank += (u.x < v ? 1u : 0u) + (u.y < v ? 1u : 0u) + (u.z < v ? 1u : 0u) + (u.w < v ? 1u : 0u);
    }
    if (e < len) list[beg + rank] = v;  // rank < len: inside the segment
  }
}
