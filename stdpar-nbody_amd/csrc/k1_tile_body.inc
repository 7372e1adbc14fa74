// Body of K1's LDS-tile form, included by all_pairs_force_kernel (K1_SOFT false) and by its softened twin all_pairs_softened_kernel
// (K1_SOFT true: pair_batch_soft with e2, no pair rule; everything that fixes the rounding order is this same text).  Included
// rather than inlined for the reason k1_sgpr_body.inc gives.  In scope: T, D, R, JS, m, x, a, c, sz, first, count, rule, e2.
  using rec_t = src_rec<T, D>;
  constexpr int TG  = kWaves / JS;    // target groups per block
  constexpr int TB  = TG * 64 * R;    // targets per block
  constexpr int LPT = kTileJ / kBlock;  // source records each lane stages per tile
  constexpr int SUB = kTileJ / JS;    // sources of a tile handled by one wave

  __shared__ rec_t tile[kTileJ];
  __shared__ T partial[(JS > 1) ? (JS - 1) * TG * 64 * R * D : 1];

  const int lane   = threadIdx.x & 63;
  const int wave   = threadIdx.x >> 6;
  const int tgroup = wave / JS;
  const int jpart  = wave % JS;

  // targets of this lane
  T xi[R][D], acc[R][D];
  uint32_t ti[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint32_t local = blockIdx.x * TB + tgroup * (64 * R) + r * 64 + lane;
    ti[r]          = local;
    uint64_t i     = uint64_t(first) + (local < count ? local : 0u);  // clamp: out-of-range lanes compute, never store
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xi[r][k]  = x[i * D + k];
      acc[r][k] = T(0);
    }
  }

  const uint32_t ntiles = (sz + kTileJ - 1) / kTileJ;
  const pair_consts<T> pc;
  const bool ffar = !K1_SOFT && ap_far_mode(rule);

  // register staging of one tile: LPT records per lane
  rec_t stage[LPT];
  auto stage_load = [&](uint32_t t) {
#pragma unroll
    for (int q = 0; q < LPT; ++q) {
      uint64_t j = uint64_t(t) * kTileJ + q * kBlock + threadIdx.x;
      if (j < sz) {
#pragma unroll
        for (int k = 0; k < D; ++k) stage[q].p[k] = x[j * D + k];
        stage[q].m = m[j];
      } else {  // padding: zero mass contributes exactly 0
#pragma unroll
        for (int k = 0; k < D; ++k) stage[q].p[k] = T(0);
        stage[q].m = T(0);
      }
      if (D == 2) stage[q].p[2] = T(0);
    }
  };

  stage_load(0);
  auto run = [&](auto ff) {  // the tile loop, once per pair rule (pair_batch)
    constexpr bool FF = decltype(ff)::value;
    for (uint32_t t = 0; t < ntiles; ++t) {
      __syncthreads();  // every wave is done reading the previous tile
#pragma unroll
      for (int q = 0; q < LPT; ++q) tile[q * kBlock + threadIdx.x] = stage[q];
      __syncthreads();
      if (t + 1 < ntiles) stage_load(t + 1);  // in flight while this tile is consumed

      const rec_t* src = &tile[jpart * SUB];
      constexpr int U  = 64 / int(sizeof(rec_t));  // the scalar-stream form's batch: 2 records in f64, 4 in f32
#pragma unroll 2
      for (int jj = 0; jj < SUB; jj += U) {
        rec_t s[U];
        src_cst<T> kc[U];  // f64: the sources' constants, the multiplies the scalar stream's pre-pass makes (bitwise the same pair)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          s[u]  = src[jj + u];  // wave-uniform address: LDS broadcast
          kc[u] = src_cst<T>::of(s[u].m);
        }
        if constexpr (K1_SOFT) pair_batch_soft<T, D, R, U>(acc, xi, s, kc, pc, e2);
        else pair_batch<T, D, R, U, FF>(acc, xi, s, kc, pc);
      }
    }
  };
  if constexpr (K1_SOFT) run(std::false_type{});
  else if (ffar) run(std::true_type{});
  else run(std::false_type{});

  // combine the JS source-split partials in wave order, then a = c * sum
  if constexpr (JS > 1) {
    __syncthreads();
    if (jpart > 0) {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) partial[((((jpart - 1) * TG + tgroup) * R + r) * D + k) * 64 + lane] = acc[r][k];
    }
    __syncthreads();
    if (jpart == 0) {
#pragma unroll
      for (int p = 1; p < JS; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int k = 0; k < D; ++k) acc[r][k] += partial[((((p - 1) * TG + tgroup) * R + r) * D + k) * 64 + lane];
    }
  }
  if (jpart == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (ti[r] < count) {
#pragma unroll
        for (int k = 0; k < D; ++k) a[uint64_t(ti[r]) * D + k] = c * acc[r][k];
      }
    }
  }
