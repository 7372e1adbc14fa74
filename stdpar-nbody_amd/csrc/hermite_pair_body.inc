// The body of the force + jerk kernels of hermite.hip, included into each with HFJ_GATHER defined (the idiom of k1_tile_body.inc):
//   0  hermite_force_jerk_kernel: the n targets are the bodies 0 .. n;
//   1  hermite_block_active_kernel (block time steps): the n targets are the bodies act[0 .. n), slot by slot, and part is
//      [chunk][2 D][n] over the slots.
// In scope: recs, part, e2, n, ntiles, tiles_per_chunk (and act), the template parameters T, D, R.
  using rec_t       = hsrc_rec<T>;
  constexpr int SUB = kHTile / kHWaves;         // records of a tile one wave takes
  constexpr int U   = (sizeof(T) == 8 ? 2 : 4) / R;  // records a batch: 2 pairs in flight per lane in double, 4 in float
  constexpr int NP  = (kHWaves - 1) * R * 2 * D * 64;  // the other waves' sums, handed over through LDS
  constexpr size_t kTileBytes = sizeof(rec_t) * kHTile, kPartBytes = sizeof(T) * NP;
  __shared__ __attribute__((aligned(64))) unsigned char smem[kTileBytes > kPartBytes ? kTileBytes : kPartBytes];
  rec_t* tile = reinterpret_cast<rec_t*>(smem);
  T* hand     = reinterpret_cast<T*>(smem);  // after the last tile has been consumed

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  T xi[R][D], vi[R][D], acc[R][D], jacc[R][D];
  uint32_t ti[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ti[r]            = blockIdx.x * (64 * R) + r * 64 + lane;
#if HFJ_GATHER
    const uint32_t i = act[ti[r] < n ? ti[r] : 0u];  // clamp: out-of-range lanes compute, never store
#else
    const uint32_t i = ti[r] < n ? ti[r] : 0u;  // clamp: out-of-range lanes compute, never store
#endif
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xi[r][k]   = recs[i].p[k];
      vi[r][k]   = recs[i].v[k];
      acc[r][k]  = T(0);
      jacc[r][k] = T(0);
    }
  }

  const uint32_t t0 = blockIdx.y * tiles_per_chunk;
  const uint32_t t1 = t0 + tiles_per_chunk < ntiles ? t0 + tiles_per_chunk : ntiles;
  const pair_consts<T> pc;

  // one record per lane, as 8 values: a 64-byte struct copy is left in private memory (scratch) by the compiler
  const T* flat = reinterpret_cast<const T*>(recs);
  T* tflat      = reinterpret_cast<T*>(smem);
  T stage[8];
  auto stage_load = [&](uint32_t t) {  // the record array is padded to whole tiles
#pragma unroll
    for (int k = 0; k < 8; ++k) stage[k] = flat[(uint64_t(t) * kHTile + threadIdx.x) * 8 + k];
  };
  stage_load(t0);
  for (uint32_t t = t0; t < t1; ++t) {
    __syncthreads();  // every wave is done reading the previous tile
#pragma unroll
    for (int k = 0; k < 8; ++k) tflat[threadIdx.x * 8 + k] = stage[k];
    __syncthreads();
    if (t + 1 < t1) stage_load(t + 1);  // in flight while this tile is consumed

    const rec_t* src = &tile[wave * SUB];
#pragma unroll 1
    for (int jj = 0; jj < SUB; jj += U) {
      rec_t s[U];  // field by field: a 64-byte struct copy is left in private memory (scratch) by the compiler
#pragma unroll
      for (int b = 0; b < U; ++b) {  // wave-uniform address: LDS broadcast
#pragma unroll
        for (int k = 0; k < D; ++k) {
          s[b].p[k] = src[jj + b].p[k];
          s[b].v[k] = src[jj + b].v[k];
        }
        s[b].m = src[jj + b].m;
      }
      pair_batch_hermite<T, D, R, U>(acc, jacc, xi, vi, s, pc, e2);
    }
  }

  // the four slices in wave order
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < D; ++k) {
        hand[((((wave - 1) * R + r) * 2 * D) + k) * 64 + lane]     = acc[r][k];
        hand[((((wave - 1) * R + r) * 2 * D) + D + k) * 64 + lane] = jacc[r][k];
      }
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int p = 1; p < kHWaves; ++p)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) {
          acc[r][k] += hand[((((p - 1) * R + r) * 2 * D) + k) * 64 + lane];
          jacc[r][k] += hand[((((p - 1) * R + r) * 2 * D) + D + k) * 64 + lane];
        }
    T* out = part + uint64_t(blockIdx.y) * (2 * D) * n;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (ti[r] < n) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          out[uint64_t(k) * n + ti[r]]     = acc[r][k];
          out[uint64_t(D + k) * n + ti[r]] = jacc[r][k];
        }
      }
    }
  }
