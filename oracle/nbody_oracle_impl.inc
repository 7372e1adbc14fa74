/*
 * TEST INFRASTRUCTURE — NOT PRODUCT CODE.
 *
 * Type-generic body of the CPU oracle: a plain-C restatement of the reference's hot-path
 * algorithms (UoB-HPC/stdpar-nbody @ 2025-01-03).  Included four times by nbody_oracle.c with
 *   T   = float | double          D   = 2 | 3          SFX = f2 | f3 | d2 | d3
 * Every function cites the reference file:line it follows.  Arithmetic is written in the same
 * operation order as the reference so that a -O2 -ffp-contract=off build is bit-identical to the
 * reference compiled at -O2 (checked against oracle/_ref by tests/test_oracle_golden.py).
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use this file.
 */

#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)
#define FN(name) CAT(CAT(name, _), SFX)

#if IS_F32
  #define T_EPS FLT_EPSILON
  #define T_POW powf
  #define T_SQRT sqrtf
  #define T_FMIN fminf
  #define T_FMAX fmaxf
  #define T_SIN sinf
  #define T_COS cosf
  #define T_ACOS acosf
  #define W double /* the wider type of the *_wide references below */
  #define W_SQRT sqrt
  #define W_FABS fabs
#else
  #define W long double
  #define W_SQRT sqrtl
  #define W_FABS fabsl
  #define T_EPS DBL_EPSILON
  #define T_POW pow
  #define T_SQRT sqrt
  #define T_FMIN fmin
  #define T_FMAX fmax
  #define T_SIN sin
  #define T_COS cos
  #define T_ACOS acos
#endif

/* vec.h:232-240  dist2(a,b): tmp = 0; for i: di = a[i]-b[i]; tmp += di*di */
static inline T FN(dist2)(const T* a, const T* b) {
  T tmp = (T)0.;
  for (int i = 0; i < D; ++i) {
    T di = a[i] - b[i];
    tmp += di * di;
  }
  return tmp;
}

/* vec.h:243-246  dist = sqrt(dist2) + eps */
static inline T FN(dist)(const T* a, const T* b) { return T_SQRT(FN(dist2)(a, b)) + T_EPS; }

/* vec.h:249-252  dist3 = pow(dist2, 3/2) + eps */
static inline T FN(dist3)(const T* a, const T* b) { return T_POW(FN(dist2)(a, b), (T)3. / (T)2.) + T_EPS; }

/* The pair term shared by all_pairs.h:23 and bvh.h:297,308:
 *   acc += m_j * (x_j - x_i) / dist3(x_i, x_j)
 * operator order: (x_j - x_i) component-wise (vec.h:67-70), scalar*vec = per-component multiply
 * (vec.h:79-88), vec/scalar = per-component DIVISION (vec.h:96-110), then += (vec.h:55-58). */
static inline void FN(pair_term)(T* acc, T mj, const T* xi, const T* xj) {
  T d3 = FN(dist3)(xi, xj);
  for (int k = 0; k < D; ++k) {
    T d = xj[k] - xi[k];
    d   = d * mj;
    d   = d / d3;
    acc[k] += d;
  }
}

/* all_pairs.h:14-27  one target per logical thread, sources in ascending j, skip j == i, a[i] = c*ai */
static void FN(all_pairs_force)(const T* m, const T* x, T* a, T c, uint32_t sz, uint32_t first, uint32_t count) {
#pragma omp parallel for schedule(static)
  for (int64_t ii = 0; ii < (int64_t)count; ++ii) {
    uint64_t i = (uint64_t)first + (uint64_t)ii;
    T ai[D];
    T pi[D];
    for (int k = 0; k < D; ++k) { ai[k] = (T)0; pi[k] = x[i * D + k]; }
    for (uint32_t j = 0; j < sz; ++j) {
      if (i == j) continue;
      FN(pair_term)(ai, m[j], pi, &x[(uint64_t)j * D]);
    }
    for (int k = 0; k < D; ++k) a[i * D + k] = c * ai[k];
  }
}

/* all_pairs.h:29-50  one logical thread per ordered pair p; j = p / sz, i = p % sz.
 * mode 0 = as written in the reference: pair count is uint32*uint32 (wraps, system.h:13-14 +
 *          all_pairs.h:32) and only components [0],[1] are accumulated (all_pairs.h:37-38,47-48).
 * mode 1 = intended semantics: 64-bit pair count, all D components.
 * Sequential p order (what the serial PSTL backend executes). Term: c * m_j * (x_j - x_i) / dist3. */
static void FN(all_pairs_collapsed_force)(const T* m, const T* x, T* a, const T* ao, T c, uint32_t sz, int mode) {
  uint64_t npairs = mode == 0 ? (uint64_t)(uint32_t)(sz * sz) : (uint64_t)sz * (uint64_t)sz;
  int ncomp       = mode == 0 ? 2 : D;
  for (uint64_t p = 0; p < npairs; ++p) {
    uint64_t j = p / sz, i = p % sz;
    if (i == j) {
      for (int k = 0; k < ncomp; ++k) a[i * D + k] -= ao[i * D + k];
      continue;
    }
    const T* pi = &x[i * D];
    const T* pj = &x[j * D];
    T d3        = FN(dist3)(pi, pj);
    T cm        = c * m[j];
    for (int k = 0; k < ncomp; ++k) {
      T d = pj[k] - pi[k];
      d   = d * cm;
      d   = d / d3;
      a[i * D + k] += d;
    }
  }
}

/* system.h:52-60  x += dt*v + ((0.5*dt)*dt)*ao ; v += (0.5*dt)*(a+ao) ; ao = a */
static void FN(accelerate_step)(T* x, T* v, const T* a, T* ao, T dt, uint32_t count) {
  T hdt   = (T)0.5 * dt;
  T hdtdt = hdt * dt;
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < (int64_t)count; ++i) {
    for (int k = 0; k < D; ++k) {
      uint64_t e = (uint64_t)i * D + k;
      T t1 = dt * v[e];
      T t2 = hdtdt * ao[e];
      x[e] += t1 + t2;
      v[e] += hdt * (a[e] + ao[e]);
      ao[e] = a[e];
    }
  }
}

/* system.h:62-79  KE = 0.5*sum m|v|^2 ; PE = -0.5*c*sum_i sum_{j!=i} m_i*m_j/dist(x_i,x_j)
 * (sequential left-to-right sums, the order the serial backend produces). */
static void FN(calc_energies)(const T* m, const T* x, const T* v, T c, uint32_t sz, T* ke_out, T* pe_out) {
  T ke = (T)0;
  for (uint32_t i = 0; i < sz; ++i) {
    T n2 = (T)0.;
    for (int k = 0; k < D; ++k) n2 += v[(uint64_t)i * D + k] * v[(uint64_t)i * D + k];
    ke = ke + m[i] * n2;
  }
  T pe = (T)0;
  for (uint32_t i = 0; i < sz; ++i) {
    T total = 0;
    T mi    = m[i];
    for (uint32_t j = 0; j < sz; ++j)
      if (j != i) total += mi * m[j] / FN(dist)(&x[(uint64_t)i * D], &x[(uint64_t)j * D]);
    pe = pe + total;
  }
  *ke_out = (T)0.5 * ke;
  *pe_out = -(T)0.5 * c * pe;
}

/* system.h:62-79 with every term formed exactly as above (in T) but both sums carried in long double: the yardstick for a float
 * system, whose single float accumulator (what the serial backend produces, calc_energies above) drifts by itself — 3e-5 over
 * 3.6e7 terms — while a tree-shaped sum of the same terms does not; in double the sums add nothing to the terms' own rounding. */
static void FN(calc_energies_wide)(const T* m, const T* x, const T* v, T c, uint32_t sz, double* ke_out, double* pe_out) {
  long double ke = 0.L;
  for (uint32_t i = 0; i < sz; ++i) {
    T n2 = (T)0.;
    for (int k = 0; k < D; ++k) n2 += v[(uint64_t)i * D + k] * v[(uint64_t)i * D + k];
    ke += (long double)(m[i] * n2);
  }
  long double pe = 0.L;
#pragma omp parallel for schedule(static) reduction(+ : pe)
  for (int64_t i_ = 0; i_ < (int64_t)sz; ++i_) {
    uint32_t i        = (uint32_t)i_;
    long double total = 0.L;
    T mi              = m[i];
    for (uint32_t j = 0; j < sz; ++j)
      if (j != i) total += (long double)(mi * m[j] / FN(dist)(&x[(uint64_t)i * D], &x[(uint64_t)j * D]));
    pe += total;
  }
  *ke_out = (double)(0.5L * ke);
  *pe_out = (double)(-0.5L * (long double)c * pe);
}

/* The all-pairs force of include/nbody_hip.h restated with every operation in the wider type W (double for T = float, long double
 * for T = double) on the T inputs, the reference's eps(T) kept:
 *   a_i = c * sum_{j != i} m_j d / (r2 * sqrt(r2) + eps(T)),  d = x_j - x_i,  r2 = |d|^2
 * (a coincident pair adds d = 0, as src/all_pairs.h does), and beside it the sum of the terms' magnitudes
 *   scale_i = c * sum_{j != i} |m_j| r / (r^3 + eps(T)),
 * the yardstick a rounding error of target i is measured against.  targets[nt]: the bodies evaluated; outputs converted to double. */
static void FN(all_pairs_force_wide)(const T* m, const T* x, T c, uint32_t sz, const uint32_t* targets, uint32_t nt, double* a_out,
                                     double* scale_out) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t t = 0; t < (int64_t)nt; ++t) {
    const uint32_t i = targets[t];
    W xi[D], acc[D], sc = 0;
    for (int k = 0; k < D; ++k) { xi[k] = (W)x[(uint64_t)i * D + k]; acc[k] = 0; }
    for (uint32_t j = 0; j < sz; ++j) {
      if (j == i) continue;
      W d[D], r2 = 0;
      for (int k = 0; k < D; ++k) {
        d[k] = (W)x[(uint64_t)j * D + k] - xi[k];
        r2 += d[k] * d[k];
      }
      const W r = W_SQRT(r2);
      const W w = (W)m[j] / (r2 * r + (W)T_EPS);
      for (int k = 0; k < D; ++k) acc[k] += w * d[k];
      sc += W_FABS(w) * r;
    }
    for (int k = 0; k < D; ++k) a_out[(uint64_t)t * D + k] = (double)((W)c * acc[k]);
    scale_out[t] = (double)(W_FABS((W)c) * sc);
  }
}

/* The potential of include/nbody_hip.h with the terms formed in W as well: -c/2 sum_i sum_{j != i} m_i m_j / (sqrt(r2) + eps(T)),
 * self pair excluded by index, summed in long double.  The term is symmetric in (i, j), so each unordered pair is formed once. */
static void FN(potential_wide)(const T* m, const T* x, T c, uint32_t sz, double* pe_out) {
  long double pe = 0.L;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : pe)
  for (int64_t i_ = 0; i_ < (int64_t)sz; ++i_) {
    const uint32_t i = (uint32_t)i_;
    W xi[D], total = 0;
    for (int k = 0; k < D; ++k) xi[k] = (W)x[(uint64_t)i * D + k];
    for (uint32_t j = i + 1; j < sz; ++j) {
      W r2 = 0;
      for (int k = 0; k < D; ++k) {
        const W d = (W)x[(uint64_t)j * D + k] - xi[k];
        r2 += d * d;
      }
      total += (W)m[j] / (W_SQRT(r2) + (W)T_EPS);
    }
    pe += (long double)((W)m[i] * total);
  }
  *pe_out = (double)(-(long double)c * pe);
}

/* bvh.h:17-22 + vec.h:382-405  bounding box: init = AABB of the origin (+-10 eps), each point padded
 * by +-10 eps (tol computed in double then converted: `epsilon() * 10.`), merge = fmin/fmax. */
static void FN(bounding_box)(const T* x, uint32_t sz, T* xmin, T* xmax) {
  const T tol = (T)((double)T_EPS * 10.);
  for (int k = 0; k < D; ++k) { xmin[k] = (T)0. - tol; xmax[k] = (T)0. + tol; }
  for (uint32_t i = 0; i < sz; ++i)
    for (int k = 0; k < D; ++k) {
      T p = x[(uint64_t)i * D + k];
      xmin[k] = T_FMIN(xmin[k], p - tol);
      xmax[k] = T_FMAX(xmax[k], p + tol);
    }
}

/* vec.h:266-293 interleave_bits */
static inline uint64_t FN(interleave_bits)(const uint32_t* c) {
#if D == 2
  #define BS2(v, out)                                       \
    {                                                       \
      uint64_t q = (v);                                     \
      q = (q | q << 16) & UINT64_C(0xffff0000ffff);         \
      q = (q | q << 8) & UINT64_C(0xff00ff00ff00ff);        \
      q = (q | q << 4) & UINT64_C(0xf0f0f0f0f0f0f0f);       \
      q = (q | q << 2) & UINT64_C(0x3333333333333333);      \
      q = (q | q << 1) & UINT64_C(0x5555555555555555);      \
      out = q;                                              \
    }
  uint64_t a, b;
  BS2(c[1], a);
  BS2(c[0], b);
  return a | (b << 1);
  #undef BS2
#else
  #define BS3(v, out)                                       \
    {                                                       \
      uint64_t q = (v);                                     \
      q &= UINT64_C(0x1fffff);                              \
      q = (q | q << 32) & UINT64_C(0x1f00000000ffff);       \
      q = (q | q << 16) & UINT64_C(0x1f0000ff0000ff);       \
      q = (q | q << 8) & UINT64_C(0x100f00f00f00f00f);      \
      q = (q | q << 4) & UINT64_C(0x10c30c30c30c30c3);      \
      q = (q | q << 2) & UINT64_C(0x1249249249249249);      \
      out = q;                                              \
    }
  uint64_t a, b, e;
  BS3(c[2], a);
  BS3(c[1], b);
  BS3(c[0], e);
  return a | (b << 1) | (e << 2);
  #undef BS3
#endif
}

/* vec.h:299-356 hilbert<N>: Skilling transform. NB the 3D branch transforms only dims 0,1
 * (n = 2, bits = 21; vec.h:328) and interleaves dim 2 raw. */
static inline uint64_t FN(hilbert)(const uint32_t* cell) {
  uint32_t xx[D];
  for (int k = 0; k < D; ++k) xx[k] = cell[k];
  const uint32_t n = 2;
#if D == 2
  const uint32_t M = 1U << (32 - 1);
#else
  const uint32_t M = 1U << (21 - 1);
#endif
  for (uint32_t Q = M; Q > 1; Q >>= 1) {
    uint32_t P = Q - 1;
    for (uint32_t i = 0; i < n; ++i) {
      if ((xx[i] & Q) != 0) {
        xx[0] ^= P;
      } else {
        uint32_t t = (xx[0] ^ xx[i]) & P;
        xx[0] ^= t;
        xx[i] ^= t;
      }
    }
  }
  for (uint32_t i = 1; i < n; ++i) xx[i] ^= xx[i - 1];
  uint32_t t = 0;
  for (uint32_t Q = M; Q > 1; Q >>= 1)
    if ((xx[n - 1] & Q) != 0) t ^= Q - 1;
  for (uint32_t i = 0; i < n; ++i) xx[i] ^= t;
  return FN(interleave_bits)(xx);
}

/* bvh.h:33-45  key per body. cast<uint32_t> of an out-of-range value is UB in C++; the x86-64
 * reference build converts through a 64-bit cvttss2si/cvttsd2si and keeps the low 32 bits, which
 * `(uint32_t)(int64_t)` reproduces. */
static void FN(hilbert_keys)(const T* x, uint32_t sz, const T* xmin, const T* xmax, uint64_t* keys) {
  uint32_t cells = (D == 2) ? 0xffffffffu : 0x1fffffu;
  T cs[D];
  for (int k = 0; k < D; ++k) cs[k] = (xmax[k] - xmin[k]) / (T)cells;
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < (int64_t)sz; ++i) {
    uint32_t cell[D];
    for (int k = 0; k < D; ++k) {
      T q     = (x[(uint64_t)i * D + k] - xmin[k]) / cs[k];
      cell[k] = (uint32_t)(int64_t)q;
    }
    keys[i] = FN(hilbert)(cell);
  }
}

/* bvh.h:47-95  reorder (x,m,v,a,ao) ascending by key. The reference sort is UNSTABLE (tie order
 * unspecified); the oracle breaks ties by original index (= any stable sort). perm[new] = old. */
static void FN(apply_perm)(T* m, T* x, T* v, T* a, T* ao, uint32_t sz, const uint32_t* perm) {
  T* tmp = (T*)malloc(sizeof(T) * (size_t)sz * D);
  T* arrs[4] = {x, v, a, ao};
  for (int q = 0; q < 4; ++q) {
    memcpy(tmp, arrs[q], sizeof(T) * (size_t)sz * D);
    for (uint32_t i = 0; i < sz; ++i)
      for (int k = 0; k < D; ++k) arrs[q][(uint64_t)i * D + k] = tmp[(uint64_t)perm[i] * D + k];
  }
  memcpy(tmp, m, sizeof(T) * sz);
  for (uint32_t i = 0; i < sz; ++i) m[i] = tmp[perm[i]];
  free(tmp);
}

/* bvh.h:98-172 implicit complete binary tree. Node arrays: nm = monopole (D coords + mass,
 * monopole.h:7-23), nb = aabb (xmin[D], xmax[D]), nbw = width. */
typedef struct {
  uint32_t last_level, nnodes;
  T* nm;  /* nnodes * (D+1): x..., mass */
  T* nb;  /* nnodes * 2D */
  T* nbw; /* nnodes */
} FN(bvh_t);

static inline T FN(node_width)(const T* b) { /* bvh.h:140-144 std::max of side lengths */
  T w = b[D + 0] - b[0];
  for (int k = 1; k < D; ++k) {
    T l = b[D + k] - b[k];
    w   = (w < l) ? l : w;
  }
  return w;
}

/* bvh.h:175-244 build_tree */
static void FN(bvh_build)(FN(bvh_t) * t, const T* m, const T* x, uint32_t nbodies) {
  const T tol      = (T)((double)T_EPS * 10.);
  uint32_t ll      = t->last_level;
  uint32_t first   = (1u << ll) - 1u;
  uint32_t count   = 1u << ll;
#pragma omp parallel for schedule(static)
  for (int64_t li_ = 0; li_ < (int64_t)count; ++li_) {
    uint32_t li = (uint32_t)li_, i = first + li;
    uint32_t bl = li * 2, br = bl + 1;
    T* nm = &t->nm[(uint64_t)i * (D + 1)];
    T* nb = &t->nb[(uint64_t)i * 2 * D];
    if (bl >= nbodies) { /* dead node: mass 0 (bvh.h:185-188); b/bw left untouched by the reference */
      for (int k = 0; k <= D; ++k) nm[k] = (T)0;
      for (int k = 0; k < 2 * D; ++k) nb[k] = (T)0;
      t->nbw[i] = (T)0;
      continue;
    }
    if (br >= nbodies) { /* bvh.h:190-194 */
      for (int k = 0; k < D; ++k) nm[k] = x[(uint64_t)bl * D + k];
      nm[D] = m[bl];
      for (int k = 0; k < D; ++k) { nb[k] = x[(uint64_t)bl * D + k] - tol; nb[D + k] = x[(uint64_t)bl * D + k] + tol; }
      t->nbw[i] = FN(node_width)(nb);
    } else { /* bvh.h:195-205 */
      T mass = m[bl] + m[br];
      for (int k = 0; k < D; ++k) {
        T com = m[bl] * x[(uint64_t)bl * D + k] + m[br] * x[(uint64_t)br * D + k];
        nm[k] = com / mass;
      }
      nm[D] = mass;
      for (int k = 0; k < D; ++k) {
        T p0 = x[(uint64_t)bl * D + k], p1 = x[(uint64_t)br * D + k];
        nb[k]     = T_FMIN(p0, p1) - tol;
        nb[D + k] = T_FMAX(p0, p1) + tol;
      }
      t->nbw[i] = FN(node_width)(nb);
    }
  }
  for (int32_t l = (int32_t)ll - 1; l >= 0; --l) { /* bvh.h:210-243 */
    uint32_t f = (1u << l) - 1u, cnt = 1u << l;
#pragma omp parallel for schedule(static)
    for (int64_t li_ = 0; li_ < (int64_t)cnt; ++li_) {
      uint32_t li = (uint32_t)li_, i = f + li;
      uint32_t bl = li * 2 + f + cnt, br = bl + 1;
      const T* ml = &t->nm[(uint64_t)bl * (D + 1)];
      const T* mr = &t->nm[(uint64_t)br * (D + 1)];
      T* nm = &t->nm[(uint64_t)i * (D + 1)];
      T* nb = &t->nb[(uint64_t)i * 2 * D];
      int ibl = ml[D] != 0., ibr = mr[D] != 0.;
      if (!ibl) { /* bvh.h:225-228: copies the (dead) left monopole; b/bw untouched -> oracle writes 0 */
        for (int k = 0; k <= D; ++k) nm[k] = ml[k];
        for (int k = 0; k < 2 * D; ++k) nb[k] = (T)0;
        t->nbw[i] = (T)0;
        continue;
      }
      if (!ibr) { /* bvh.h:230-233 */
        for (int k = 0; k <= D; ++k) nm[k] = ml[k];
        for (int k = 0; k < 2 * D; ++k) nb[k] = t->nb[(uint64_t)bl * 2 * D + k];
        t->nbw[i] = t->nbw[bl];
      } else { /* bvh.h:234-241 */
        T mass = ml[D] + mr[D];
        for (int k = 0; k < D; ++k) nm[k] = (ml[D] * ml[k] + mr[D] * mr[k]) / mass;
        nm[D] = mass;
        for (int k = 0; k < D; ++k) {
          nb[k]     = T_FMIN(t->nb[(uint64_t)bl * 2 * D + k], t->nb[(uint64_t)br * 2 * D + k]);
          nb[D + k] = T_FMAX(t->nb[(uint64_t)bl * 2 * D + D + k], t->nb[(uint64_t)br * 2 * D + D + k]);
        }
        t->nbw[i] = FN(node_width)(nb);
      }
    }
  }
}

/* bvh.h:246-324 compute_force: stackless traversal, opening test bw^2 < theta^2 * dist2(xs,xj).
 * counts (optional): per body {internal-node tests, leaf-pair visits, monopole terms, body terms}. */
static void FN(bvh_force)(const FN(bvh_t) * t, const T* m, const T* x, T* a, T c, uint32_t sz, T theta, uint32_t* counts) {
  T theta2            = theta * theta;
  uint32_t last_level = t->last_level;
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t i_ = 0; i_ < (int64_t)sz; ++i_) {
    uint32_t i = (uint32_t)i_;
    T xs[D], acc[D];
    for (int k = 0; k < D; ++k) { xs[k] = x[(uint64_t)i * D + k]; acc[k] = (T)0; }
    uint32_t tree_index = 0, level = 0;
    uint32_t leaf_level = last_level + 1, nlevels = last_level + 1;
    uint64_t covered = 0;
    uint32_t c_nodes = 0, c_leaf = 0, c_mono = 0, c_body = 0;
    while (covered < sz) {
      uint32_t next_index = 0, next_level = level;
      if (level == leaf_level) { /* bvh.h:288-303 */
        uint32_t bidx = tree_index - ((1u << leaf_level) - 1u);
        for (int k = 0; k < 2; ++k) {
          if (bidx < sz && bidx != i) {
            FN(pair_term)(acc, m[bidx], xs, &x[(uint64_t)bidx * D]);
            ++c_body;
          }
          ++bidx;
        }
        covered += 2;
        ++c_leaf;
        /* force_ascend_right: parent(tree_index, level) + 1, level - 1 (bvh.h:272-275, :115-120) */
        next_index = (level == 0) ? 0u : (((1u << (level - 1)) - 1u) + (tree_index - ((1u << level) - 1u)) / 2u);
        next_index += 1;
        next_level = level - 1;
      } else {
        const T* nm = &t->nm[(uint64_t)tree_index * (D + 1)];
        T bw        = t->nbw[tree_index];
        ++c_nodes;
        if (bw * bw < theta2 * FN(dist2)(xs, nm)) { /* bvh.h:246-248,306-311 */
          FN(pair_term)(acc, nm[D], xs, nm);
          ++c_mono;
          covered += (uint64_t)(1 << (nlevels - level));
          if ((tree_index - 1) % 2) { /* right child -> parent + 1 (bvh.h:277-281) */
            next_index = (level == 0) ? 0u : (((1u << (level - 1)) - 1u) + (tree_index - ((1u << level) - 1u)) / 2u);
            next_index += 1;
            next_level = level - 1;
          } else {
            next_index = tree_index + 1;
          }
        } else { /* descend: left_child (bvh.h:126-130,283-286) */
          uint32_t f = (1u << level) - 1u, cnt = 1u << level;
          next_index = (tree_index - f) * 2 + f + cnt;
          next_level = level + 1;
        }
      }
      level      = next_level;
      tree_index = next_index;
    }
    for (int k = 0; k < D; ++k) a[(uint64_t)i * D + k] = c * acc[k];
    if (counts) {
      counts[(uint64_t)i * 4 + 0] = c_nodes;
      counts[(uint64_t)i * 4 + 1] = c_leaf;
      counts[(uint64_t)i * 4 + 2] = c_mono;
      counts[(uint64_t)i * 4 + 3] = c_body;
    }
  }
}

/* ---- the wide BVH walk: the per-body yardstick of the traversal (K9) of include/nbody_hip.h -----------------------------------------
 * bvh_force's loop above for the bodies in targets[nt], on the same T tree: the opening test bw * bw < theta2 * dist2 in T with the
 * reference's unfused dist2, the same order of visits, the same counters.  What a body accumulates from the entries it accepts (node
 * monopoles and bodies alike) is formed and summed in W, the pair form all_pairs_force_wide's with the reference's eps(T) kept:
 *   a_i = c sum m d / (r2 * r + eps(T))        scale_i = |c| sum |m| r / (r2 * r + eps(T)),    d = p - x_i, r2 = |d|^2, r = sqrt(r2)
 * near_nodes[t]: the accepted NODES whose dist2 (in T) is below 2^-16, the distance at which the product's double term changes form.
 * Written here from the formulas of include/nbody_hip.h; no reference counterpart. */
static void FN(bvh_walk_wide)(const FN(bvh_t) * t, const T* m, const T* x, T c, uint32_t sz, T theta, const uint32_t* targets,
                              uint32_t nt, double* a_out, double* scale_out, uint32_t* counts, uint32_t* near_nodes) {
  const T theta2            = theta * theta;
  const T near2             = (T)(1.0 / 65536.0);
  const uint32_t last_level = t->last_level;
  const W eps               = (W)T_EPS;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t tt = 0; tt < (int64_t)nt; ++tt) {
    const uint32_t i = targets[tt];
    T xs[D];
    W xw[D], acc[D], sc = 0;
    for (int k = 0; k < D; ++k) { xs[k] = x[(uint64_t)i * D + k]; xw[k] = (W)xs[k]; acc[k] = 0; }
    uint32_t tree_index = 0, level = 0;
    uint32_t leaf_level = last_level + 1, nlevels = last_level + 1;
    uint64_t covered = 0;
    uint32_t c_nodes = 0, c_leaf = 0, c_mono = 0, c_body = 0, c_near = 0;
    while (covered < sz) {
      uint32_t next_index = 0, next_level = level;
      const T* p = NULL; /* the accepted entry, if any: D coordinates in T */
      T mass     = (T)0;
      if (level == leaf_level) {
        uint32_t bidx = tree_index - ((1u << leaf_level) - 1u);
        for (int q = 0; q < 2; ++q) {
          if (bidx < sz && bidx != i) {
            const T* pb = &x[(uint64_t)bidx * D];
            W d[D], r2 = 0;
            for (int k = 0; k < D; ++k) { d[k] = (W)pb[k] - xw[k]; r2 += d[k] * d[k]; }
            const W r = W_SQRT(r2), w = (W)m[bidx] / (r2 * r + eps);
            for (int k = 0; k < D; ++k) acc[k] += w * d[k];
            sc += W_FABS(w) * r;
            ++c_body;
          }
          ++bidx;
        }
        covered += 2;
        ++c_leaf;
        next_index = (level == 0) ? 0u : (((1u << (level - 1)) - 1u) + (tree_index - ((1u << level) - 1u)) / 2u);
        next_index += 1;
        next_level = level - 1;
      } else {
        const T* nm = &t->nm[(uint64_t)tree_index * (D + 1)];
        T bw        = t->nbw[tree_index];
        ++c_nodes;
        const T d2t = FN(dist2)(xs, nm);
        if (bw * bw < theta2 * d2t) {
          p    = nm;
          mass = nm[D];
          ++c_mono;
          if (d2t < near2) ++c_near;
          covered += (uint64_t)(1 << (nlevels - level));
          if ((tree_index - 1) % 2) {
            next_index = (level == 0) ? 0u : (((1u << (level - 1)) - 1u) + (tree_index - ((1u << level) - 1u)) / 2u);
            next_index += 1;
            next_level = level - 1;
          } else {
            next_index = tree_index + 1;
          }
        } else {
          uint32_t f = (1u << level) - 1u, cnt = 1u << level;
          next_index = (tree_index - f) * 2 + f + cnt;
          next_level = level + 1;
        }
      }
      if (p) {
        W d[D], r2 = 0;
        for (int k = 0; k < D; ++k) { d[k] = (W)p[k] - xw[k]; r2 += d[k] * d[k]; }
        const W r = W_SQRT(r2), w = (W)mass / (r2 * r + eps);
        for (int k = 0; k < D; ++k) acc[k] += w * d[k];
        sc += W_FABS(w) * r;
      }
      level      = next_level;
      tree_index = next_index;
    }
    for (int k = 0; k < D; ++k) a_out[(uint64_t)tt * D + k] = (double)((W)c * acc[k]);
    scale_out[tt] = (double)(W_FABS((W)c) * sc);
    counts[(uint64_t)tt * 4 + 0] = c_nodes;
    counts[(uint64_t)tt * 4 + 1] = c_leaf;
    counts[(uint64_t)tt * 4 + 2] = c_mono;
    counts[(uint64_t)tt * 4 + 3] = c_body;
    near_nodes[tt] = c_near;
  }
}

/* ---- octree Barnes-Hut (octree.h) ------------------------------------------------------------- */
/* Serial restatement of the lock-based concurrent tree (what the serial PSTL backend executes: bodies are
 * inserted in index order).  Node numbering depends on insertion order; forces, visit counts, tree size and
 * the root monopole do not (cells split iff they hold >= 2 bodies, children are visited in hyperant order). */
#define OT_EMPTY 0xffffffffu
#define OT_BODY 0xfffffffeu
#define OT_CHILDREN (1u << D)

typedef struct {
  uint32_t capacity, next_free;
  T root_side;
  T root_x[D];
  uint32_t* first_child; /* capacity */
  uint32_t* parent;      /* 1 + capacity / 2^D */
  T* m;                  /* capacity * (D+1): x..., mass */
} FN(octree_t);

/* octree.h:93-112 compute_bounds: scalar min/max over ALL components of all bodies, init (0,0), +-1 */
static void FN(octree_bounds)(FN(octree_t) * t, const T* x, uint32_t sz) {
  T mn = (T)0, mx = (T)0;
  for (uint64_t e = 0; e < (uint64_t)sz * D; ++e) {
    mn = T_FMIN(mn, x[e]);
    mx = T_FMAX(mx, x[e]);
  }
  mx += 1;
  mn -= 1;
  T divide = (mx + mn) / (T)2;
  t->root_side = mx - mn;
  for (int k = 0; k < D; ++k) t->root_x[k] = divide;
}

/* octree.h:114-174 insert (no contention: every CAS succeeds) */
static int FN(octree_insert)(FN(octree_t) * t, T mass, const T* pos) {
  uint32_t idx = 0;
  T divide[D];
  for (int k = 0; k < D; ++k) divide[k] = t->root_x[k];
  T side = t->root_side;
  for (;;) {
    uint32_t status = t->first_child[idx];
    if (status != OT_EMPTY && status != OT_BODY) {
      T half = side / (T)4;
      uint32_t child_pos = 0, level = 1;
      for (int k = 0; k < D; ++k) {
        int gt = pos[k] > divide[k];
        child_pos += level * (uint32_t)gt;
        level *= 2;
        divide[k] += (T)(2 * gt - 1) * half;
      }
      idx = status + child_pos;
      side /= (T)2;
      continue;
    } else if (status == OT_EMPTY) {
      for (int k = 0; k < D; ++k) t->m[(uint64_t)idx * (D + 1) + k] = pos[k];
      t->m[(uint64_t)idx * (D + 1) + D] = mass;
      t->first_child[idx] = OT_BODY;
      return 0;
    } else { /* body: split */
      uint32_t fc = t->next_free;
      t->next_free += OT_CHILDREN;
      if (t->next_free > t->capacity) return -1; /* the reference would write out of bounds here */
      t->parent[(fc - 1) / OT_CHILDREN] = idx;
      const T* pm = &t->m[(uint64_t)idx * (D + 1)];
      uint32_t child_pos = 0, level = 1;
      for (int k = 0; k < D; ++k) {
        child_pos += level * (uint32_t)(pm[k] > divide[k]);
        level *= 2;
      }
      uint32_t ev = fc + child_pos;
      for (int k = 0; k <= D; ++k) t->m[(uint64_t)ev * (D + 1) + k] = pm[k];
      t->first_child[ev] = OT_BODY;
      t->first_child[idx] = fc;
      continue;
    }
  }
}

/* octree.h:183-224 compute_tree: every internal node = sum of its 2^D children in child order, then x /= m.
 * (Evaluated children-first here; the reference's latch makes the last arriving child do the same sum.) */
static void FN(octree_multipoles)(FN(octree_t) * t) {
  /* children are always allocated after their parent, so a descending index sweep sees children first */
  for (int64_t i = (int64_t)t->next_free - 1; i >= 0; --i) {
    uint32_t fc = t->first_child[i];
    if (fc == OT_EMPTY || fc == OT_BODY) continue;
    T mass = 0, xx[D];
    for (int k = 0; k < D; ++k) xx[k] = 0;
    for (uint32_t c = 0; c < OT_CHILDREN; ++c) {
      const T* cm = &t->m[(uint64_t)(fc + c) * (D + 1)];
      mass += cm[D];
      for (int k = 0; k < D; ++k) xx[k] += cm[D] * cm[k];
    }
    for (int k = 0; k < D; ++k) t->m[(uint64_t)i * (D + 1) + k] = xx[k] / mass;
    t->m[(uint64_t)i * (D + 1) + D] = mass;
  }
}

/* octree.h:226-263 compute_force; counts (optional): per body {nodes examined, terms accumulated} */
static void FN(octree_force)(const FN(octree_t) * t, const T* x, T* a, T c, uint32_t sz, T theta, uint32_t* counts) {
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t i_ = 0; i_ < (int64_t)sz; ++i_) {
    const T* xi = &x[(uint64_t)i_ * D];
    uint32_t idx = 0;
    T side = t->root_side;
    T acc[D];
    for (int k = 0; k < D; ++k) acc[k] = 0;
    int fwd = 1;
    uint32_t c_nodes = 0, c_terms = 0;
    while (idx != OT_EMPTY) {
      /* next_node (octree.h:63-71) */
      uint32_t next;
      if (idx == 0) next = OT_EMPTY;
      else {
        uint32_t sg = (idx - 1) / OT_CHILDREN, cp = (idx - 1) % OT_CHILDREN;
        next = cp == (OT_CHILDREN - 1) ? t->parent[sg] : idx + 1;
      }
      if (fwd) {
        const T* mj = &t->m[(uint64_t)idx * (D + 1)];
        uint32_t fc = t->first_child[idx];
        T dx = FN(dist)(xi, mj);
        ++c_nodes;
        if (fc == OT_EMPTY || fc == OT_BODY || side / dx < theta) {
          T d3 = dx * dx * dx;
          for (int k = 0; k < D; ++k) {
            T d = mj[k] - xi[k];
            d   = d * mj[D];
            d   = d / d3;
            acc[k] += d;
          }
          ++c_terms;
        } else {
          next = fc;
          side /= (T)2;
        }
      }
      fwd = next > idx;
      side *= fwd ? (T)1 : (T)2;
      idx = next;
    }
    for (int k = 0; k < D; ++k) a[(uint64_t)i_ * D + k] = c * acc[k];
    if (counts) {
      counts[(uint64_t)i_ * 2 + 0] = c_nodes;
      counts[(uint64_t)i_ * 2 + 1] = c_terms;
    }
  }
}

/* clear, bounds, insert, multipoles (octree.h:321-325) into a freshly allocated tree; <0 on overflow (the tree is freed). */
static int FN(octree_build)(FN(octree_t) * t, const T* m, const T* x, uint32_t sz) {
  size_t cap = (size_t)OT_CHILDREN * sz;
  if (cap < 1000) cap = 1000; /* system.h:30 max_tree_node_size */
  t->capacity    = (uint32_t)cap;
  t->first_child = (uint32_t*)malloc(sizeof(uint32_t) * cap);
  t->parent      = (uint32_t*)malloc(sizeof(uint32_t) * (1 + cap / OT_CHILDREN));
  t->m           = (T*)calloc(cap * (D + 1), sizeof(T));
  for (size_t i = 0; i < cap; ++i) t->first_child[i] = OT_EMPTY;
  for (size_t i = 0; i < 1 + cap / OT_CHILDREN; ++i) t->parent[i] = OT_EMPTY;
  t->next_free = 1;
  FN(octree_bounds)(t, x, sz);
  int rc = 0;
  for (uint32_t i = 0; i < sz && rc == 0; ++i) rc = FN(octree_insert)(t, m[i], &x[(uint64_t)i * D]);
  if (rc == 0) FN(octree_multipoles)(t);
  return rc;
}

static void FN(octree_free)(FN(octree_t) * t) {
  free(t->first_child);
  free(t->parent);
  free(t->m);
}

/* One force phase of run_octree (octree.h:321-326): clear, bounds, insert, multipoles, force.
 * info[0] = tree size (next_free_child_group), root monopole mass written to *root_mass. Returns <0 on overflow. */
static int FN(octree_step_force)(const T* m, const T* x, T* a, T c, uint32_t sz, T theta, uint32_t* counts, uint32_t* tree_size,
                                 T* root_mass) {
  FN(octree_t) t;
  int rc = FN(octree_build)(&t, m, x, sz);
  if (rc == 0) {
    FN(octree_force)(&t, x, a, c, sz, theta, counts);
    if (tree_size) *tree_size = t.next_free;
    if (root_mass) *root_mass = t.m[D];
  }
  FN(octree_free)(&t);
  return rc;
}

/* ---- the wide octree walk: the yardstick of the softened, quadrupole and potential walks of include/nbody_hip.h ----------------
 * The tree, its monopoles (T) and every opening decision are the ones above, operation for operation; what a body accumulates from
 * the nodes it accepts is formed and summed in W.  Written here from the formulas of include/nbody_hip.h; no reference counterpart. */
#define OT_NQ (D == 3 ? 6 : 3)

/* Q of every cell straight from the bodies it holds: Q = sum_b m_b (3 s s^T - |s|^2 I), s = x_b - p_cell (p_cell the T monopole,
 * widened), components xx, xy, (xz,) yy(, yz, zz).  Every body leaf walks up its parent chain and adds itself to each ancestor; no
 * child-to-parent shift is used.  Body leaves and empty slots keep Q = 0. */
static W* FN(octree_quadrupoles_wide)(const FN(octree_t) * t) {
  W* quad = (W*)calloc((size_t)t->next_free * OT_NQ, sizeof(W));
  for (uint32_t i = 1; i < t->next_free; ++i) {
    if (t->first_child[i] != OT_BODY) continue;
    const T* b = &t->m[(uint64_t)i * (D + 1)];
    const W mb = (W)b[D];
    uint32_t idx = i;
    while (idx != 0) {
      idx = t->parent[(idx - 1) / OT_CHILDREN];
      const T* p = &t->m[(uint64_t)idx * (D + 1)];
      W s[D], s2 = 0;
      for (int k = 0; k < D; ++k) {
        s[k] = (W)b[k] - (W)p[k];
        s2 += s[k] * s[k];
      }
      W* q  = &quad[(uint64_t)idx * OT_NQ];
      int e = 0;
      for (int u = 0; u < D; ++u)
        for (int v = u; v < D; ++v) q[e++] += mb * ((W)3 * s[u] * s[v] - (u == v ? s2 : (W)0));
    }
  }
  return quad;
}

/* compute_force's loop (octree.h:226-263, octree_force above) for the bodies in targets[nt], the accepted terms in W.  With
 * d = p - x_i, r = sqrt(|d|^2), eps = eps(T), e2 a number of T (both widened), per accepted node (cell or leaf):
 *   a_mono += m d / (r + eps)^3            s_mono += m / (r + eps)
 *   a_soft += m d / (|d|^2 + e2)^(3/2)     s_soft += m / sqrt(|d|^2 + e2)               (soft != 0 only)
 * and per accepted CELL, Q from octree_quadrupoles_wide:
 *   a_quad += -(Q d) / r^5 + 5/2 (d^T Q d) d / r^7     s_quad += 1/2 (d^T Q d) / r^5
 * a_quad_deep: the share of the cells at depth >= split_level (the root is depth 0) in that quadrupole term.  The s sums leave out
 * the body's own leaf (d == 0 in every coordinate).  Outputs: a_* = c * (a_mono, a_soft, a_mono + a_quad, a_quad_deep), s_* =
 * (s_mono, s_soft, s_mono + s_quad), and beside each of the six sums the sum of the magnitudes of its terms (|c| included for the
 * forces), scales[t][6] = {a_mono, a_soft, a_quad, s_mono, s_soft, s_quad}; counts[t][2] as octree_force's. */
static void FN(octree_walk_wide)(const FN(octree_t) * t, const W* quad, const T* x, T c, T theta, int soft, T e2t, uint32_t split_level,
                                 const uint32_t* targets, uint32_t nt, const oracle_wide_out* o) {
  const W eps = (W)T_EPS, e2 = (W)e2t, cw = (W)c, ca = W_FABS((W)c);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t tt = 0; tt < (int64_t)nt; ++tt) {
    const T* xi  = &x[(uint64_t)targets[tt] * D];
    uint32_t idx = 0, depth = 0;
    T side = t->root_side;
    W am[D], as[D], aq[D], aqd[D];
    W sm = 0, ss = 0, sq = 0, k_am = 0, k_as = 0, k_aq = 0, k_sm = 0, k_ss = 0, k_sq = 0;
    for (int k = 0; k < D; ++k) am[k] = as[k] = aq[k] = aqd[k] = 0;
    int fwd = 1;
    uint32_t c_nodes = 0, c_terms = 0;
    while (idx != OT_EMPTY) {
      uint32_t next;
      if (idx == 0) next = OT_EMPTY;
      else {
        uint32_t sg = (idx - 1) / OT_CHILDREN, cp = (idx - 1) % OT_CHILDREN;
        next = cp == (OT_CHILDREN - 1) ? t->parent[sg] : idx + 1;
      }
      if (fwd) {
        const T* mj = &t->m[(uint64_t)idx * (D + 1)];
        uint32_t fc = t->first_child[idx];
        T dx = FN(dist)(xi, mj); /* the decision, in T, on the unsoftened distance */
        ++c_nodes;
        const int leaf = fc == OT_EMPTY || fc == OT_BODY;
        if (leaf || side / dx < theta) {
          W d[D], r2 = 0;
          int self = 1;
          for (int k = 0; k < D; ++k) {
            d[k] = (W)mj[k] - (W)xi[k];
            r2 += d[k] * d[k];
            self = self && d[k] == (W)0;
          }
          const W r = W_SQRT(r2), mass = (W)mj[D], re = r + eps;
          const W w = mass / (re * re * re);
          for (int k = 0; k < D; ++k) am[k] += w * d[k];
          k_am += W_FABS(w) * r;
          if (!self) {
            sm += mass / re;
            k_sm += W_FABS(mass) / re;
          }
          if (soft) {
            const W q = r2 + e2, rq = W_SQRT(q);
            const W ws = mass / (q * rq);
            for (int k = 0; k < D; ++k) as[k] += ws * d[k];
            k_as += W_FABS(ws) * r;
            if (!self) {
              ss += mass / rq;
              k_ss += W_FABS(mass) / rq;
            }
          }
          if (!leaf) {
            const W* qq = &quad[(uint64_t)idx * OT_NQ];
            W Q[D][D], qd[D], dqd = 0, tn = 0;
            int e = 0;
            for (int u = 0; u < D; ++u)
              for (int v = u; v < D; ++v) Q[u][v] = Q[v][u] = qq[e++];
            for (int u = 0; u < D; ++u) {
              qd[u] = 0;
              for (int v = 0; v < D; ++v) qd[u] += Q[u][v] * d[v];
              dqd += d[u] * qd[u];
            }
            const W r5 = r2 * r2 * r, r7 = r5 * r2;
            for (int k = 0; k < D; ++k) {
              const W term = -qd[k] / r5 + (W)2.5 * dqd * d[k] / r7;
              aq[k] += term;
              if (depth >= split_level) aqd[k] += term;
              tn += term * term;
            }
            k_aq += W_SQRT(tn);
            const W st = (W)0.5 * dqd / r5;
            sq += st;
            k_sq += W_FABS(st);
          }
          ++c_terms;
        } else {
          next = fc;
          side /= (T)2;
          ++depth;
        }
      }
      fwd = next > idx;
      side *= fwd ? (T)1 : (T)2;
      depth -= fwd ? 0u : 1u;
      idx = next;
    }
    for (int k = 0; k < D; ++k) {
      const uint64_t e = (uint64_t)tt * D + k;
      if (o->a_mono) o->a_mono[e] = (double)(cw * am[k]);
      if (o->a_soft) o->a_soft[e] = (double)(cw * as[k]);
      if (o->a_quad) o->a_quad[e] = (double)(cw * (am[k] + aq[k]));
      if (o->a_quad_deep) o->a_quad_deep[e] = (double)(cw * aqd[k]);
    }
    if (o->s_mono) o->s_mono[tt] = (double)sm;
    if (o->s_soft) o->s_soft[tt] = (double)ss;
    if (o->s_quad) o->s_quad[tt] = (double)(sm + sq);
    if (o->scales) {
      double* sc = &o->scales[(uint64_t)tt * 6];
      sc[0] = (double)(ca * k_am);
      sc[1] = (double)(ca * k_as);
      sc[2] = (double)(ca * (k_am + k_aq));
      sc[3] = (double)k_sm;
      sc[4] = (double)k_ss;
      sc[5] = (double)(k_sm + k_sq);
    }
    if (o->counts) {
      o->counts[(uint64_t)tt * 2 + 0] = c_nodes;
      o->counts[(uint64_t)tt * 2 + 1] = c_terms;
    }
  }
}

/* The tree of octree_step_force, then the wide walk.  softening > 0: e2 = fl_T(T(softening) * T(softening)); root_q (optional): the
 * root's OT_NQ values of Q as double.  Returns <0 on overflow. */
static int FN(octree_step_walk_wide)(const T* m, const T* x, T c, uint32_t sz, T theta, double softening, uint32_t split_level,
                                     const uint32_t* targets, uint32_t nt, const oracle_wide_out* o) {
  FN(octree_t) t;
  int rc = FN(octree_build)(&t, m, x, sz);
  if (rc == 0) {
    const T e   = (T)softening;
    const T e2t = e * e;
    W* quad     = FN(octree_quadrupoles_wide)(&t);
    FN(octree_walk_wide)(&t, quad, x, c, theta, softening > 0.0, e2t, split_level, targets, nt, o);
    if (o->root_q)
      for (int k = 0; k < OT_NQ; ++k) o->root_q[k] = (double)quad[k];
    free(quad);
  }
  FN(octree_free)(&t);
  return rc;
}

#undef OT_NQ
#undef OT_EMPTY
#undef OT_BODY
#undef OT_CHILDREN

/* ---- workload generators (models.h) -------------------------------------------------------- */

/* models.h:12-28 uniform: m = 1.0/(T)n (double division), pos[i], vel[i] interleaved from sym_dis; dt=0.1, G=1 */
static void FN(model_uniform)(uint32_t n, T* m, T* x, T* v, double* dt, double* c) {
  oracle_rng g;
  oracle_rng_seed(&g, 42u);
  for (uint32_t b = 0; b < n; ++b) {
    m[b] = (T)(1.0 / (T)n);
    for (int k = 0; k < D; ++k) {
      x[(uint64_t)b * D + k] = (T)oracle_uniform(&g, -1.0, 1.0);
      v[(uint64_t)b * D + k] = (T)oracle_uniform(&g, -1.0, 1.0);
    }
  }
  *dt = (T)1e-1;
  *c  = (T)1;
}

#if D == 3
/* models.h:73-79 rotate_vec */
static inline void FN(rotate)(const T mat[3][3], T* vv) {
  T r[3] = {0, 0, 0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[i] += mat[i][j] * vv[j];
  for (int i = 0; i < 3; ++i) vv[i] = r[i];
}
#endif

/* models.h:81-110 create_circular_orbit */
static uint32_t FN(circular_orbit)(oracle_rng* g, uint32_t next, size_t npart, T constant, T total_mass, T orbit_mass,
                                   const T* centre, T* m, T* x, T* v) {
  for (size_t q = 0; q < npart; ++q) {
    T mass   = orbit_mass / (T)npart;
    T radius = (T)(30 + 20 * oracle_uniform(g, 0.0, 1.0));
    T angle  = (T)oracle_uniform(g, 0.0, 2 * 3.141592653589793238462643383279502884);
    T pos[D], vel[D];
    for (int k = 0; k < D; ++k) { pos[k] = 0; vel[k] = 0; }
    pos[0] = radius * T_SIN(angle);
    pos[1] = radius * T_COS(angle);
    T vnorm = T_SQRT(constant * total_mass / (radius + T_EPS));
    T n2    = (T)0.;
    for (int k = 0; k < D; ++k) n2 += pos[k] * pos[k];
    T s    = vnorm / (T_SQRT(n2) + T_EPS);
    vel[0] = s * (-pos[1]);
    vel[1] = s * pos[0];
#if D == 3
    pos[2] = (T)(10 * oracle_uniform(g, -1.0, 1.0));
    vel[2] = (T)(0.00001 * oracle_uniform(g, -1.0, 1.0));
    const T mat[3][3] = {{(T)0.0, (T)-1.0, (T)0.0}, {(T)0.9, (T)0.0, (T)0.5}, {(T)0.5, (T)0.0, (T)0.9}};
    FN(rotate)(mat, pos);
    FN(rotate)(mat, vel);
#endif
    m[next] = mass;
    for (int k = 0; k < D; ++k) { x[(uint64_t)next * D + k] = pos[k] + centre[k]; v[(uint64_t)next * D + k] = vel[k]; }
    ++next;
  }
  return next;
}

/* models.h:112-136 galaxy: system size = 2*(size/2.0) truncated; dt = 10, G = 1e-4. Returns the system size. */
static uint32_t FN(model_galaxy)(uint32_t n_arg, T* m, T* x, T* v, double* dt, double* c) {
  double gnp    = n_arg / 2.0;
  uint32_t size = (uint32_t)(2 * gnp);
  for (uint64_t e = 0; e < (uint64_t)size * D; ++e) { x[e] = 0; v[e] = 0; }
  for (uint32_t b = 0; b < size; ++b) m[b] = 0;
  oracle_rng g;
  oracle_rng_seed(&g, 42u);
  T constant    = (T)1e-4;
  T centre_mass = (T)1e4;
  T offset      = (T)100.0;
  T off[D];
  uint32_t next = 0;
  for (int k = 0; k < D; ++k) off[k] = 0;
  off[0] = offset * (T)-1;
  off[1] = offset * (T)(1 / 2.0);
  m[next] = centre_mass;
  for (int k = 0; k < D; ++k) { x[(uint64_t)next * D + k] = off[k]; v[(uint64_t)next * D + k] = 0; }
  ++next;
  next = FN(circular_orbit)(&g, next, (size_t)(gnp - 1), constant, centre_mass + 1, (T)1, off, m, x, v);
  centre_mass /= 10;
  off[0] = offset * (T)1;
  off[1] = offset * (T)(-1 / 2.0);
  m[next] = centre_mass;
  for (int k = 0; k < D; ++k) { x[(uint64_t)next * D + k] = off[k]; v[(uint64_t)next * D + k] = 0; }
  ++next;
  next = FN(circular_orbit)(&g, next, (size_t)(gnp - 1), constant, centre_mass + 1, (T)1, off, m, x, v);
  (void)next;
  *dt = (T)1e1;
  *c  = (T)1e-4;
  return size;
}

#if D == 3
/* models.h:30-66 plummer (3D only): dt = 1, G = 6.674e-11 */
static void FN(model_plummer)(uint32_t n, T* m, T* x, T* v, double* dt, double* c) {
  oracle_rng g;
  oracle_rng_seed(&g, 42u);
  for (uint32_t b = 0; b < n; ++b) {
    T mass    = (T)(1.0 / (T)n);
    T radius  = (T)(1.0 / sqrt(pow(oracle_uniform(&g, 0.0, 1.0), -2.0 / 3.0) - 1));
    T p_theta = (T)acos(oracle_uniform(&g, -1.0, 1.0));
    T p_phi   = (T)oracle_uniform(&g, 0.0, 2 * 3.141592653589793238462643383279502884);
    T pos[3]  = {radius * (T_SIN(p_theta) * T_COS(p_phi)), radius * (T_SIN(p_theta) * T_SIN(p_phi)), radius * T_COS(p_theta)};
    T q = (T)0.0, gg = (T)0.1;
    while (gg > q * q * pow(1.0 - q * q, 3.5)) {
      q  = (T)oracle_uniform(&g, 0.0, 1.0);
      gg = (T)(0.1 * oracle_uniform(&g, 0.0, 1.0));
    }
    T vnorm   = (T)(q * 1.41421356237309504880168872420969808 * pow(radius * radius + 1, -0.25));
    T v_theta = (T)acos(oracle_uniform(&g, -1.0, 1.0));
    T v_phi   = (T)oracle_uniform(&g, 0.0, 2 * 3.141592653589793238462643383279502884);
    T vel[3]  = {vnorm * (T_SIN(v_theta) * T_COS(v_phi)), vnorm * (T_SIN(v_theta) * T_SIN(v_phi)), vnorm * T_COS(v_theta)};
    m[b] = mass;
    for (int k = 0; k < 3; ++k) { x[(uint64_t)b * 3 + k] = pos[k]; v[(uint64_t)b * 3 + k] = vel[k]; }
  }
  *dt = (T)1;
  *c  = (T)6.674e-11;
}
#endif

#undef T_EPS
#undef T_POW
#undef T_SQRT
#undef T_FMIN
#undef T_FMAX
#undef T_SIN
#undef T_COS
#undef T_ACOS
#undef W
#undef W_SQRT
#undef W_FABS
#undef FN
#undef CAT
#undef CAT_
