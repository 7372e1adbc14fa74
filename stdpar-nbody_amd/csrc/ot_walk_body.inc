// Body of the compiler-scheduled octree walk (walk form 1), included by ot_force_kernel (OT_SOFT false) and by
// ot_force_softened_kernel (OT_SOFT true: the same tests in the same order, the accepted term ot_accumulate_soft).  Included
// rather than inlined for the reason k1_sgpr_body.inc gives.
// ot_force_quadrupole_kernel defines OT_QUAD as well: every accepted cell also adds its quadrupole term (ot_accumulate_quad); the
// kernels that leave it undefined are the same text as before it existed.
// The potential walks (ot_potential_kernel, ot_potential_softened_kernel, ot_potential_quadrupole_kernel) define OT_POT: the same
// tests in the same order, one scalar sum S per lane instead of acc[D] (ot_potential_term, ot_potential_soft, ot_potential_quad),
// phi[body - first] = scale * S.
// In scope: T, D, COUNT, rootrec, groups, list, nlist, x, a, c, first, theta, capacity, root, flags, counters, e2 (and quad);
// with OT_POT, phi and scale instead of a and c.
  constexpr uint32_t NCH   = 1u << D;
  constexpr uint32_t GPW   = 64u / NCH;                         // bodies per wave
  constexpr uint32_t DEPTH = (NCH - 1u) * kMaxLevels<D> + NCH;  // a pop frees one slot, an open adds <= 2^D
  __shared__ uint32_t stack[GPW][DEPTH];
  const uint32_t g = threadIdx.x / NCH, cc = threadIdx.x % NCH;
  // `list`: the owned bodies in key order (neighbours share most of their walk: cache); XCD-contiguous blocks
  const uint32_t t    = ot_xcd_contiguous_block(blockIdx.x, gridDim.x) * GPW + g;
  const bool valid    = t < nlist;
  const uint32_t body = valid ? list[t] : first;
  const ot_theta<T> th(theta);
  const pair_consts<T> pc;
  const T root_side = root[D];
#ifdef OT_POT
  T xi[D], pot = T(0);
#pragma unroll
  for (int k = 0; k < D; ++k) xi[k] = valid ? x[uint64_t(body) * D + k] : T(0);
#else
  T xi[D], acc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    xi[k]  = valid ? x[uint64_t(body) * D + k] : T(0);
    acc[k] = T(0);
  }
#endif
  uint32_t c_nodes = 0, c_terms = 0;
  uint32_t cur = 0, sp = 0;
  bool more = false;
  if (valid) {  // the root is examined alone (by every lane of the group; lane 0 keeps the result)
    const ot_node<T> nd = *rootrec;
    T di[D];
#pragma unroll
    for (int k = 0; k < D; ++k) di[k] = nd.p[k] - xi[k];
    const T d2f     = ot_dist2_fused<T, D>(di);
    const T y0      = ot_rsq(d2f);
    const bool leaf = nd.fc >= kOtBody;  // kOtBody or kOtEmpty
    const bool take = leaf || ot_accept<T, D>(!leaf, root_side, di, y0, th);
    {
      const bool on0 = take && cc == 0;  // the root is examined by every lane of the group; lane 0 keeps the result
      const uint64_t m0 = __builtin_amdgcn_ballot_w64(on0);
#ifdef OT_POT
      if constexpr (OT_SOFT) {
        if (m0 != 0ull) ot_potential_soft<T, D>(on0, pot, di, nd.m, e2);
      } else {
        if (m0 != 0ull) ot_potential_term<T, D>(on0, m0, pot, di, nd.m, d2f, y0);
      }
#else
      if constexpr (OT_SOFT) {
        if (m0 != 0ull) ot_accumulate_soft<T, D>(on0, acc, di, nd.m, e2, pc);
      } else {
        if (m0 != 0ull) ot_accumulate<T, D>(on0, m0, acc, di, nd.m, d2f, y0, pc);
      }
#endif
#ifdef OT_QUAD
      const bool q0 = on0 && !leaf;  // an accepted root cell: its quadrupole is node 0's slot
#ifdef OT_POT
      if (__builtin_amdgcn_ballot_w64(q0) != 0ull) ot_potential_quad<T, D>(q0, pot, di, d2f, y0, quad);
#else
      if (__builtin_amdgcn_ballot_w64(q0) != 0ull) ot_accumulate_quad<T, D>(q0, acc, di, d2f, y0, quad);
#endif
#endif
    }
    if (COUNT && cc == 0) {
      c_nodes = 1;
      c_terms = take;
    }
    more = !take;
    cur  = nd.fc;  // the root's stored fc is already a sibling-group number, like every fl[][0] below
  }
  uint32_t guard = capacity;  // a well-formed tree is left after < capacity steps; never spin on a damaged one
  while (more && guard-- != 0u) {  // the lanes of a group leave together
    const ot_node<T> nd = groups[cur].load(cc);  // this lane's child: two or three 16-/8-byte loads
    T di[D];
#pragma unroll
    for (int k = 0; k < D; ++k) di[k] = nd.p[k] - xi[k];
    const T d2f     = ot_dist2_fused<T, D>(di);
    const T y0      = ot_rsq(d2f);
    const bool leaf = nd.fc >= kOtBody;
    const bool take = leaf || ot_accept<T, D>(!leaf, ot_ldexp(root_side, -int(nd.lvl)), di, y0, th);
    if (COUNT) {
      ++c_nodes;
      c_terms += take;
    }
    const uint64_t take_mask = __builtin_amdgcn_ballot_w64(take);
#ifdef OT_POT
    if constexpr (OT_SOFT) {
      if (take_mask != 0ull) ot_potential_soft<T, D>(take, pot, di, nd.m, e2);
    } else {
      if (take_mask != 0ull) ot_potential_term<T, D>(take, take_mask, pot, di, nd.m, d2f, y0);
    }
#else
    if constexpr (OT_SOFT) {
      if (take_mask != 0ull) ot_accumulate_soft<T, D>(take, acc, di, nd.m, e2, pc);
    } else {
      if (take_mask != 0ull) ot_accumulate<T, D>(take, take_mask, acc, di, nd.m, d2f, y0, pc);
    }
#endif
#ifdef OT_QUAD
    {  // leaves (bodies, empty slots) have no quadrupole: a round that accepts none loads nothing more
      const bool qon = take && !leaf;
#ifdef OT_POT
      if (__builtin_amdgcn_ballot_w64(qon) != 0ull)
        ot_potential_quad<T, D>(qon, pot, di, d2f, y0, quad + (uint64_t(1u + cur * NCH + cc) * uint32_t(kOtQS<D>)));
#else
      if (__builtin_amdgcn_ballot_w64(qon) != 0ull)
        ot_accumulate_quad<T, D>(qon, acc, di, d2f, y0, quad + (uint64_t(1u + cur * NCH + cc) * uint32_t(kOtQS<D>)));
#endif
    }
#endif
    const uint32_t open_mask = uint32_t((__ballot(!take) >> (g * NCH)) & ((1ull << NCH) - 1ull));
    if (sp + uint32_t(__builtin_popcount(open_mask)) > DEPTH) {  // only below the key depth can a walk hold this many
      if (cc == 0) atomicOr(flags, kFlagStack);                  // pending nodes; reported by nbody_octree_info
      break;
    }
    if (!take) stack[g][sp + uint32_t(__builtin_popcount(open_mask >> (cc + 1u)))] = nd.fc;  // reverse child order
    sp += uint32_t(__builtin_popcount(open_mask));
    if (sp == 0u) break;
    __builtin_amdgcn_wave_barrier();  // one lane pushed, all lanes of the group pop: keep the LDS write before the read
    cur = stack[g][--sp];
    __builtin_amdgcn_wave_barrier();  // ... and this read before the next round's push into the same slot
  }
  if (more && guard == 0xffffffffu && cc == 0) atomicOr(flags, kFlagWalk);  // step budget spent: the tree is damaged
  // combine the 2^D partial sums of a body (fixed order)
#pragma unroll
  for (uint32_t off = NCH / 2; off > 0; off >>= 1) {
#ifdef OT_POT
    pot += __shfl_xor(pot, int(off), 64);
#else
#pragma unroll
    for (int k = 0; k < D; ++k) acc[k] += __shfl_xor(acc[k], int(off), 64);
#endif
    if (COUNT) {
      c_nodes += __shfl_xor(c_nodes, int(off), 64);
      c_terms += __shfl_xor(c_terms, int(off), 64);
    }
  }
  if (valid && cc == 0) {
#ifdef OT_POT
    phi[uint64_t(body - first)] = scale * pot;
#else
#pragma unroll
    for (int k = 0; k < D; ++k) a[uint64_t(body - first) * D + k] = c * acc[k];
#endif
    if (COUNT) {
      counters[uint64_t(body) * 2 + 0] = c_nodes;
      counters[uint64_t(body) * 2 + 1] = c_terms;
    }
  }
