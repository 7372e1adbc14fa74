// Body of K1's scalar-stream form, included by all_pairs_force_sgpr_kernel (K1_SOFT false) and by its softened twin
// all_pairs_softened_sgpr_kernel (K1_SOFT true: pair_batch_soft with e2, no pair rule; slices, chunks, the hand-off and the
// collect path are this same text).  Included in the kernels' own bodies rather than called as an inlined device function:
// inlining reorders hipcc's output for the unsoftened kernel, whose loop is checked instruction by instruction
// (tools/check_smem_pipeline.py, tools/check_k1_cst_loads.py).
// In scope: T, D, R, JS, RULE, packed, cst, x, a, c, sz, first, count, tiles_per_chunk, h, rule, e2, box.
  using rec_t = src_rec<T, D>;
  constexpr int TG  = kSgprWaves<JS> / JS;
  constexpr int TB  = TG * 64 * R;
  constexpr int SUB = kTileJ / JS;
  __shared__ T partial[(JS > 1) ? (JS - 1) * TG * 64 * R * D : 1];
  const int lane   = threadIdx.x & 63;
  const int wave   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tgroup = wave / JS;
  const int jpart  = wave % JS;
  T xi[R][D], acc[R][D];
  uint32_t ti[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint32_t local = blockIdx.x * TB + tgroup * (64 * R) + r * 64 + lane;
    ti[r]          = local;
    uint64_t i     = uint64_t(first) + (local < count ? local : 0u);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xi[r][k]  = x[i * D + k];
      acc[r][k] = T(0);
    }
  }
  // source chunk of this block (grid.y): tiles [t0, t1) of the padded source set; one chunk = everything when grid.y == 1
  const uint32_t ntiles = (sz + kTileJ - 1) / kTileJ;
  const uint32_t t0     = blockIdx.y * tiles_per_chunk;
  const uint32_t t1     = min(ntiles, t0 + tiles_per_chunk);
  const pair_consts<T> pc;
  const bool ffar       = !K1_SOFT && ap_far_mode(rule);
  const uint32_t nsteps = (t1 - t0) * SUB;  // sources this wave visits: its SUB-record slice of every tile, in tile order
  constexpr int U = 64 / int(sizeof(rec_t));  // records per 64-byte batch (2 in f64, 4 in f32); SUB % (2 * U) == 0
  struct batch_t {
    rec_t r[U];
  };
  auto batch = [&](uint32_t k) { return packed + (uint64_t(t0 + k / SUB) * kTileJ + uint32_t(jpart) * SUB + (k % SUB)); };
  // f64: the constants of the batch's two sources (cst_batch, 32 bytes beside every 64 bytes of records) travel with it
  constexpr bool CST = sizeof(T) == 8;
  auto cbatch = [&](uint32_t k) { return cst + (uint64_t(t0 + k / SUB) * kTileJ + uint32_t(jpart) * SUB + (k % SUB)) / U; };
  [[maybe_unused]] uint32_t vzero = 0;  // the vector load's lane offset
  if constexpr (CST) {
    asm volatile("" : "+v"(vzero));
    // the targets' positions have landed BEFORE the loop: hipcc otherwise waits for them at their first use inside it, with
    // vmcnt(0) on every trip — free while the loop held no vector load, a wait for the constants just requested now
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < D; ++k) asm volatile("" : "+v"(xi[r][k]));
  }
  // Two SGPR buffers, each requested (s_load_dwordx16) one compute phase before it is consumed.  Written with inline
  // asm: hipcc folds a loop-carried load from read-only memory back into a load at the loop top and waits for it there.
  // SMEM returns out of order, so the only usable wait is lgkmcnt(0): wait for X, request Y, consume X.  In f64 every request
  // is preceded by the request for the batch's constants (cload: M15 into four VGPRs by a wave-uniform vector load, M1875 into
  // four SGPRs) and every wait also waits for them (cswait: vmcnt(0), exact for the same reason) — a phase is ~340 VALU cycles
  // of this wave alone, so neither wait stalls in the steady state.  The records' request comes LAST: the hand-off tail begins
  // behind the last s_load_dwordx16 of the program (tools/check_k1_handoff.py).
  // The far certificate (common.hpp: k1_block_is_far), once per block and wave, f64 launches on the sparse rule only: this
  // wave's targets against the box of the block's source chunk.  Wave-uniform; the waves of a target group decide alike.
  [[maybe_unused]] bool cfar = false;
  if constexpr (!K1_SOFT && CST && RULE == 0) {
    if (ffar && box != nullptr) {
      cfar = k1_block_is_far<T, D, R>(xi, (const T __attribute__((address_space(4)))*)(box + size_t(blockIdx.y) * (2 * D)));
#ifdef NBODY_EXPERIMENTS
      if (cfar && jpart == 0 && lane == 0)  // certified (target group, chunk) blocks, in the header of the box buffer
        atomicAdd(reinterpret_cast<unsigned long long*>(const_cast<T*>(box)) - kBoxHeaderBytes / 8, 1ull);
#endif
    }
  }
  auto run = [&](auto ff) {  // the source stream, once per pair rule (pair_batch: 0 dense, 1 sparse) and once certified far (2)
    constexpr int FF = int(decltype(ff)::value);
    sgpr16 A, B;
    [[maybe_unused]] cst_regs CA, CB;
    auto request = [&](sgpr16& S, cst_regs& C, uint32_t k) {
      if constexpr (CST) C = cload(cbatch(k), vzero, xi[0][0]);
      S = sload16(batch(k), xi[0][0]);
    };
    auto wait = [&](sgpr16& S, cst_regs& C) {
      if constexpr (CST) cswait(S, C, acc[0][0]);
      else swait(S, acc[0][0]);
    };
    auto consume = [&](const sgpr16& S, const cst_regs& C) {
      const batch_t b = __builtin_bit_cast(batch_t, S);
      src_cst<T> kc[U];
      if constexpr (CST) cst_unpack(C, kc);
      if constexpr (K1_SOFT) pair_batch_soft<T, D, R, U, true>(acc, xi, b.r, kc, pc, e2);
      else if constexpr (FF == 2) pair_batch_far<T, D, R, U>(acc, xi, b.r, kc);
      else pair_batch<T, D, R, U, FF != 0>(acc, xi, b.r, kc, pc);
    };
    request(A, CA, 0);
    for (uint32_t k = 0; k < nsteps; k += 2 * U) {
      wait(A, CA);
      request(B, CB, k + U);
      consume(A, CA);
      wait(B, CB);
      request(A, CA, k + 2 * U < nsteps ? k + 2 * U : k);  // the last iteration re-requests its own batch
      consume(B, CB);
    }
    wait(A, CA);  // nothing in flight when the wave goes on
  };
  if constexpr (K1_SOFT) run(std::false_type{});           // one pair form: no rule to choose
  else if constexpr (RULE == 1) run(std::false_type{});  // (experiments: one rule per instantiation, forced from the host)
  else if constexpr (RULE == 2) run(std::true_type{});
  else if (ffar) {  // two copies of the loop: inside ONE loop hipcc hoists the rules' common head above the branch
    if constexpr (CST) {
      if (cfar) run(std::integral_constant<int, 2>{});  // and a third: no pair of this block needs the near/far test
      else run(std::true_type{});
    } else run(std::true_type{});
  } else run(std::false_type{});
  if constexpr (JS > 1) {
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
  if (jpart != 0) return;
  const uint32_t y = blockIdx.y, last = gridDim.y - 1u;
  uint32_t* const tw = h.turn + blockIdx.x * TG + tgroup;  // nullptr + ... when there is one chunk: never dereferenced (y == last == 0)
  if (h.sums != nullptr) {
    // Small launches (all blocks resident within a few rounds: the blocks of one target group's sixteen chunks finish TOGETHER, and
    // a chain of turns is fifteen dependent round trips through memory — 18 of 41 us at N = 4096, 42 of 76 us in float at 8192):
    // every chunk's wave stores its sum, then draws a ticket; whoever draws the last one — whichever chunk it is — adds the
    // sums IN CHUNK ORDER, ((s_0 + s_1) + s_2) + ..., applies c and writes `a`: the same bits as the turns give, no waiting, no
    // failure mode.  The sums are agent-scope stores acknowledged (s_waitcnt 0) before the ticket is drawn.
    const size_t group_scalars = size_t(R) * D * 64;
    T* const all  = static_cast<T*>(h.sums);
    T* const mine = all + ((size_t(y) * gridDim.x + blockIdx.x) * TG + tgroup) * group_scalars;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < D; ++k) __hip_atomic_store(mine + (r * D + k) * 64 + lane, acc[r][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    uint32_t drawn = 0;
    if (lane == 0) drawn = __hip_atomic_fetch_add(tw, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (uint32_t(__builtin_amdgcn_readfirstlane(int(drawn))) != last) return;
    T tot[R][D];
    for (uint32_t yy = 0; yy <= last; ++yy) {
      const T* src = all + ((size_t(yy) * gridDim.x + blockIdx.x) * TG + tgroup) * group_scalars;
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const T v = __hip_atomic_load(src + (r * D + k) * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          tot[r][k] = yy == 0 ? v : tot[r][k] + v;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (ti[r] < count) {
#pragma unroll
        for (int k = 0; k < D; ++k) a[uint64_t(ti[r]) * D + k] = c * tot[r][k];
      }
    return;
  }
  bool poisoned = false;
  if (y > 0 && h.turn != nullptr) {  // my turn?  (wave-uniform address: every lane reads the same value)
    uint32_t spins = 0, seen;
    if (y == 1)
      for (uint32_t d = 0; d < h.late; ++d) __builtin_amdgcn_s_sleep(127);  // 0 rounds, except in the hand-off tests of the experiments build
    while ((seen = __hip_atomic_load(tw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != y) {
      if (seen == kTurnPoison) {  // somebody gave up on this group: nobody will add to its total again, NaN goes over it
        poisoned = true;
        break;
      }
      if (++spins > h.spins) {  // give up (see above)
        if (lane == 0) {
          __hip_atomic_exchange(tw, kTurnPoison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (atomicCAS(&h.status->err, 0u, 1u) == 0u) {
            h.status->block = blockIdx.x;
            h.status->group = uint32_t(tgroup);
            h.status->chunk = y;
          }
        }
        poisoned = true;  // whatever the word held — this wave's own number (the turn came between the last poll and the swap), a
        break;            // predecessor's that has yet to come, or poison already — the group's total is overwritten with NaN
      }
      __builtin_amdgcn_s_sleep(8);
    }
    // The loads of the running total below must be ISSUED after the poll that saw the turn.  The accesses are relaxed agent-scope
    // atomics (sc1: they bypass this XCD's L2), so nothing has to be invalidated; what is needed is that the compiler keeps them
    // behind the loop — a wavefront-scope acquire fence says so and emits no instruction (tools/check_k1_handoff.py verifies in the
    // built code object that every load of the total carries sc1 and follows the last poll).
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (spins && lane == 0) {
      atomicAdd(&h.status->polls, (unsigned long long)spins);
      atomicAdd(&h.status->waits, 1ull);
    }
  }
  // The total's R * D * 64 scalars of this target group are contiguous in `a`: through LDS (the slices' partials are spent) every
  // lane takes scalars e = q * 64 + lane, so each access is one full-width coalesced instruction — per component the lanes would
  // touch every line three times (measured: 3.2 GB of traffic per launch at N = 2^20 instead of 1.3).
  const uint32_t gbase = blockIdx.x * TB + tgroup * (64 * R);  // first target of the group
  auto add_sum = [&](bool nan) {  // nan: overwrite the group's total with NaN instead
    if constexpr (JS > 1) {
      T* stage = partial + size_t(tgroup) * R * D * 64;  // [(jpart - 1 = 0) * TG + tgroup] block of the partials: read above, free now
      if (!nan) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int k = 0; k < D; ++k) stage[(r * 64 + lane) * D + k] = acc[r][k];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int q = 0; q < R * D; ++q) {
        const uint32_t e = uint32_t(q) * 64u + uint32_t(lane);
        if (gbase + e / D < count) {
          T* slot = a + uint64_t(gbase) * D + e;
          T t     = nan ? T(__builtin_nan("")) : stage[e];
          if (!nan && y > 0) t = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + t;  // ((s_0 + s_1) + ...) + s_y
          if (!nan && y == last) t = c * t;
          __hip_atomic_store(slot, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (ti[r] < count) {
#pragma unroll
          for (int k = 0; k < D; ++k) {
            T* slot = a + uint64_t(ti[r]) * D + k;
            T t     = nan ? T(__builtin_nan("")) : acc[r][k];
            if (!nan && y > 0) t = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + t;
            if (!nan && y == last) t = c * t;
            __hip_atomic_store(slot, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    }
  };
  add_sum(poisoned);
  if (y < last && !poisoned && h.turn != nullptr) {  // pass the turn on once the stores above have been acknowledged
    for (uint32_t d = 0; d < h.delay; ++d) __builtin_amdgcn_s_sleep(127);  // 0 rounds, except in the hand-off tests of the experiments build
    __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) expcnt(0) lgkmcnt(0): this wave's stores are at the agent's coherence point
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // and the compiler keeps them above the hand-over (no instruction)
    __builtin_amdgcn_wave_barrier();
    uint32_t held = y;
    if (lane == 0) {
      __hip_atomic_compare_exchange_strong(tw, &held, y + 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    held = __builtin_amdgcn_readfirstlane(held);  // what the word held: y, or kTurnPoison left by a successor that gave up
    if (held != y) add_sum(true);
  }
