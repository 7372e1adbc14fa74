// Body of the potential's scalar-stream kernel, included by potential_sgpr_kernel (POT_SOFT false) and by
// softened_potential_sgpr_kernel (POT_SOFT true: pot_batch_soft with e2).  Included rather than inlined for the reason
// k1_sgpr_body.inc gives.  In scope: T, D, R, packed, x, sums, sz, tiles_per_chunk, e2.
  using rec_t       = src_rec<T, D>;
  constexpr int TB  = 64 * R;
  constexpr int SUB = kTileJ / kPotJS;
  __shared__ T partial[(kPotJS - 1) * 64 * R];
  const int lane  = threadIdx.x & 63;
  const int jpart = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  T xi[R][D], acc[R];
  uint32_t tg[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    tg[r]            = blockIdx.x * TB + r * 64 + lane;
    const uint64_t i = tg[r] < sz ? tg[r] : 0u;  // clamp: out-of-range lanes compute, never store
#pragma unroll
    for (int k = 0; k < D; ++k) xi[r][k] = x[i * D + k];
    acc[r] = T(0);
  }
  // f32: a tile's 64 terms are summed by themselves and the tile sums added up (`done`).  In ONE chain over the chunk a term the size
  // of the whole sum — the other galaxy's centre seen from a centre — swallows every later term below half its ulp: 575 of them at
  // N = 65 537 (9 tiles per chunk), 8.4e-6 of the potential.  f64 keeps its single chain (and its bits): its ulp is 2^-29 of float's.
  [[maybe_unused]] T done[R];
#pragma unroll
  for (int r = 0; r < R; ++r) done[r] = T(0);
  const uint32_t ntiles = (sz + kTileJ - 1) / kTileJ;
  const uint32_t t0     = blockIdx.y * tiles_per_chunk;
  const uint32_t t1     = min(ntiles, t0 + tiles_per_chunk);
  const pot_consts<T> pc;
  const uint32_t nsteps = (t1 - t0) * SUB;
  constexpr int U       = 64 / int(sizeof(rec_t));
  struct batch_t {
    rec_t r[U];
  };
  auto index = [&](uint32_t k) { return (t0 + k / SUB) * uint32_t(kTileJ) + uint32_t(jpart) * SUB + (k % SUB); };
  auto batch = [&](uint32_t k) { return packed + uint64_t(index(k)); };
  // the same two-deep SMEM pipeline as all_pairs_force_sgpr_kernel (see there)
  sgpr16 A = sload16(batch(0), xi[0][0]), B;
  for (uint32_t k = 0; k < nsteps; k += 2 * U) {
    swait(A, acc[0]);
    B = sload16(batch(k + U), xi[0][0]);
    {
      const batch_t ba = __builtin_bit_cast(batch_t, A);
      if constexpr (POT_SOFT) pot_batch_soft<T, D, R, U>(acc, xi, tg, ba.r, index(k), pc, e2);
      else pot_batch<T, D, R, U>(acc, xi, tg, ba.r, index(k), pc);
    }
    swait(B, acc[0]);
    A = sload16(batch(k + 2 * U < nsteps ? k + 2 * U : k), xi[0][0]);
    {
      const batch_t bb = __builtin_bit_cast(batch_t, B);
      if constexpr (POT_SOFT) pot_batch_soft<T, D, R, U>(acc, xi, tg, bb.r, index(k + U), pc, e2);
      else pot_batch<T, D, R, U>(acc, xi, tg, bb.r, index(k + U), pc);
    }
    if constexpr (sizeof(T) == 4) {
      if ((k + 2 * U) % SUB == 0) {  // wave-uniform: the tile's slice is through
#pragma unroll
        for (int r = 0; r < R; ++r) {
          done[r] += acc[r];
          acc[r] = T(0);
        }
      }
    }
  }
  swait(A, acc[0]);
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] += done[r];
  }
  if (jpart > 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) partial[((jpart - 1) * R + r) * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (jpart == 0) {
#pragma unroll
    for (int p = 1; p < kPotJS; ++p)
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] += partial[((p - 1) * R + r) * 64 + lane];
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (tg[r] < sz) sums[uint64_t(blockIdx.y) * sz + tg[r]] = acc[r];
  }
