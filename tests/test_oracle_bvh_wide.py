"""CPU: the oracle's wide BVH walk (oracle.bvh_walk_wide: the T tree, the opening decisions and the order of visits of bvh_force,
everything a body accumulates formed and summed in double for float inputs and in long double for double inputs) against what is
already pinned, using the oracle alone.  tests/test_gpu_bvh_wide.py measures every form of the GPU's traversal (K9) against it per
body, so it is held here first: its counters to bvh_force's bit for bit, the T walk to it within the bound the GPU will be held to,
theta = 0 to oracle.all_pairs_force_wide, and the `pairs` system's sensitivity to the eps term of a close pair.

The measure is per body and component against the body's own sum of term magnitudes, |a - a_wide| <= tol * scale_i: the global
max|a - a_ref| / max|a_ref| of tests/test_gpu_bvh.py is set by the closest pair of the system and lets a typical body be wrong by
1e-5 of its own force.

This module also owns the systems both files run (CASES, state_of, sorted_of, wide_of).  Every system is sorted with
oracle.sort_keys (ties by index, as the product's stable sort resolves them) before it is walked.

The figures of a run are in profiles/tests_bvh_wide/new_tests_figures.txt."""
import functools

import numpy as np
import pytest

import oracle as O

FORCE_TOL = {1: 1e-12, 0: 2e-5}   # the project's force bound (tests/test_gpu_bvh.py), here per body against the body's own scale
THETAS = (0.5, 1.0)
NEAR2 = 2.0 ** -16                # d2 below which the product's double term takes the guarded form (pair_math<double>::near_hi)
LDS_BYTES = 144 << 10             # csrc/bvh_plan.hpp: kTreeLdsBytes

# (name, n, dims).  2047, 2048: the last float trees the auto form walks from LDS, 2049 the first past it (test_lds_sizes)
CASES = [("uniform", 2, (3, 2)), ("uniform", 3, (3, 2)), ("uniform", 5, (3, 2)), ("uniform", 257, (3, 2)), ("uniform", 2047, (3, 2)),
         ("uniform", 2048, (3, 2)), ("uniform", 2049, (3, 2)), ("galaxy", 1000, (3, 2)), ("galaxy", 4099, (3, 2)),
         ("plummer", 4099, (3,)), ("pairs", 257, (3, 2)), ("pairs", 4099, (3, 2)), ("clusters", 4099, (3, 2))]
CASE_DIMS = [(name, n, dim) for name, n, dims in CASES for dim in dims]
CASE_IDS = [f"{name}{n}-{dim}D" for name, n, dim in CASE_DIMS]
# the smallest galaxies that reach the sweep's other launch shapes (count -> groups of 64 -> shape; 4099 -> 65 -> 8 lane ranges per
# group is among CASES): 20545 -> 322 -> 4 ranges; 41001 -> 641 -> 1 range, with work items.  Pinned in tools/bvh_plan_check.cpp.
SHAPE_CASES = [("galaxy", 20545, 3), ("galaxy", 41001, 3), ("galaxy", 41001, 2)]
SHAPE_IDS = [f"{name}{n}-{dim}D" for name, n, dim in SHAPE_CASES]


def thetas_of(name, n):
    """The opening angles of a case: 0.5 and 1.0; the clusters also at 1.4, where nodes are accepted from inside 2^-8; the
    power-of-two uniform system also at 3.0, where bodies accept the root; the launch-shape galaxies at 0.5 alone."""
    if (name, n) in [(c[0], c[1]) for c in SHAPE_CASES]:
        return (0.5,)
    return THETAS + ((1.4,) if name == "clusters" else ()) + ((3.0,) if (name, n) == ("uniform", 2048) else ())


def lds_fits(dtype, n):
    """csrc/bvh_plan.hpp's k9_lds_fits on the tree of n bodies."""
    return dtype == 0 and ((2 << O.bvh_nlevels(n)) - 1) * 32 <= LDS_BYTES


def make_state(dtype, dim, x, m, c=1.0, dt=0.01):
    s = O.State(dtype, dim, len(m))
    t = O.np_dtype(dtype)
    s.m[:], s.x[:] = np.asarray(m, t), np.asarray(x, t)
    s.c, s.dt = c, dt
    return s


PAIR_SEPS = np.array([2.0 ** -9, 0.999 * 2.0 ** -8, 1.001 * 2.0 ** -8, 2.0 ** -7, 2.0 ** -18, 0.0])


@functools.lru_cache(maxsize=None)
def pairs_system(dtype, dim, n):
    """n uniform bodies in (-1, 1)^D, 300 of 4099 (18 of 257) given a partner along a random direction at 2^-8 x {0.5, 0.999, 1.001,
    2}, at 2^-18 or at 0 (a coincident pair), class k = pair index mod 6: d2 on both sides of 2^-16, where the product's double
    term changes form, by 0.2 % and by a factor of 4, deep inside, and d = 0.  Masses span three decades.  The partner is placed
    from the position already rounded to T.  Returns (state, a, b, class): body b[k] is the partner of body a[k]."""
    rng = np.random.default_rng(1000 * dim + n)
    t = O.np_dtype(dtype)
    x = rng.uniform(-1.0, 1.0, (n, dim)).astype(t).astype(np.float64)
    npair = max(12, 300 * n // 4099)
    idx = rng.permutation(n)[:2 * npair]
    a, b = idx[:npair], idx[npair:]
    u = rng.standard_normal((npair, dim))
    u /= np.sqrt((u * u).sum(1))[:, None]
    cls = np.arange(npair) % len(PAIR_SEPS)
    x[b] = x[a] + PAIR_SEPS[cls][:, None] * u
    m = 10.0 ** rng.uniform(-3, 0, n) / n
    return make_state(dtype, dim, x, m), a, b, cls


def clusters_state(dtype, dim, n, sigma=1e-3):
    """tests/test_gpu_bvh.py::test_traversal_forms_fuzz's kind 4: n / 16 centres in (-1, 1)^D, every body within sigma (normal) of
    one of them, body 0 an escaper at 50 that makes the box 25 times the system."""
    rng = np.random.default_rng(40 + dim)
    centres = rng.uniform(-1, 1, (max(1, n // 16), dim))
    x = centres[rng.integers(0, len(centres), n)] + rng.normal(0, sigma, (n, dim))
    x[0] = 50.0
    return make_state(dtype, dim, x, rng.uniform(0.5, 1.5, n), dt=1e-3)


@functools.lru_cache(maxsize=None)
def state_of(name, n, dtype, dim):
    """The system of a case as the product receives it, unsorted (shared: do not modify)."""
    if name == "pairs":
        return pairs_system(dtype, dim, n)[0]
    if name == "clusters":
        return clusters_state(dtype, dim, n)
    return O.build_model(dtype, dim, name, n)


@functools.lru_cache(maxsize=None)
def sorted_of(name, n, dtype, dim):
    """(state in key order, its tree, perm) with perm[new] = old (shared: do not modify)."""
    s = state_of(name, n, dtype, dim).copy()
    lo, hi = O.bounding_box(s)
    perm = O.sort_keys(O.hilbert_keys(s, lo, hi))
    O.apply_perm(s, perm)
    return s, O.bvh_build(s), perm


@functools.lru_cache(maxsize=None)
def wide_of(name, n, dtype, dim, theta):
    """The wide walk of a case, rows in key order, computed once (shared: do not modify)."""
    s, tr, _ = sorted_of(name, n, dtype, dim)
    return O.bvh_walk_wide(s, tr, theta)


@functools.lru_cache(maxsize=None)
def t_walk_of(name, n, dtype, dim, theta):
    """(a, counts) of bvh_force, the reference's walk in T, rows in key order (shared: do not modify)."""
    s, tr, _ = sorted_of(name, n, dtype, dim)
    s = s.copy()
    cnt = O.bvh_force(s, tr, theta, want_counts=True)
    return s.a, cnt


def per_body(got, want, scale):
    """max over bodies (and components) of |got - want| / scale_i."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    err = err.max(axis=1) if err.ndim == 2 else err
    return float((err / scale).max())


def unfused_d2(xa, xb):
    """dist2 of the reference on T arrays: differences, then products and sums one rounding each, ascending component."""
    d = xa - xb
    d2 = d[:, 0] * d[:, 0]
    for k in range(1, d.shape[1]):
        d2 = d2 + d[:, k] * d[:, k]
    return d2


# ---- counters and the T walk against the wide walk ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("name, n, dim", CASE_DIMS + SHAPE_CASES, ids=CASE_IDS + SHAPE_IDS)
def test_counters_and_force_equal_the_t_walk(oracle, name, n, dim, dtype):
    """counts is bvh_force's bit for bit; |a_T - a_wide| <= FORCE_TOL * scale per body and component: the reference's own walk
    stays inside the bound the GPU is held to.  Measured, max over CASES and their angles: 3.9e-15 of scale in double and
    1.9e-6 in float (both galaxy 4099 3D, theta 0.5); over the launch-shape galaxies 6.4e-15 and 3.5e-6 (galaxy 41001 3D) — the
    figures a wider float bound for a case would have to be justified with (at most 4 x the case's own).  clusters 4099 at theta
    1.4 in double: near_nodes is nonzero for 3523 bodies in 3D and 3843 in 2D (3784 and 3988 at theta 0.5): nodes, not bodies,
    accepted from inside 2^-8.  uniform 2048 at theta 3.0: bodies accept the root."""
    s, tr, _ = sorted_of(name, n, dtype, dim)
    for theta in thetas_of(name, n):
        a_t, cnt = t_walk_of(name, n, dtype, dim, theta)
        w = wide_of(name, n, dtype, dim, theta)
        assert w.counts.dtype == np.uint32 and np.array_equal(w.counts, cnt), theta
        assert w.a.shape == (s.n, dim) and w.scale.shape == (s.n,) and w.near_nodes.shape == (s.n,)
        assert w.a.dtype == np.float64 and np.isfinite(w.a).all() and np.isfinite(w.scale).all()
        assert (w.scale > 0).all()
        assert (np.abs(w.a).max(axis=1) <= w.scale * (1 + 1e-12)).all()  # a sum never exceeds the sum of its terms' magnitudes
        assert (w.near_nodes <= w.counts[:, 2]).all()
        err = per_body(a_t, w.a, w.scale)
        print(f"T walk vs wide {name} {n} {dim}D dtype {dtype} theta {theta}: max err_i {err:.3g}, "
              f"{int((w.near_nodes > 0).sum())} bodies with near nodes")
        assert err <= FORCE_TOL[dtype], (theta, err)
        if name == "clusters" and dtype == 1 and theta == 1.4:
            assert (w.near_nodes > 0).any()
        if theta == 3.0:
            assert n & (n - 1) == 0 and (w.counts[:, 0] == 1).any() and not w.counts[w.counts[:, 0] == 1, 3].any()


def test_lds_sizes(oracle):
    """Which side of k9_lds_fits the sizes around 2048 fall on, from the tree's levels: float trees of 2047 and 2048 bodies (11
    levels, 4095 records of 32 bytes) fit, 2049 (12 levels) does not, and no double tree does."""
    assert [oracle.bvh_nlevels(n) for n in (2047, 2048, 2049)] == [11, 11, 12]
    assert [lds_fits(0, n) for n in (2, 257, 2047, 2048, 2049, 4099)] == [True, True, True, True, False, False]
    assert not any(lds_fits(1, n) for n in (2, 257, 2047, 2048, 2049))


# ---- the pairs system --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [257, 4099])
def test_pairs_straddle_the_near_threshold(oracle, n, dim, dtype):
    """After rounding to T the reference's unfused d2 of every partner pair lies on the side of 2^-16 its class was placed on:
    0.5 and 0.999 x 2^-8 and 2^-18 below (the last above 0), 1.001 and 2 x 2^-8 at or above, the coincident pairs at exactly 0."""
    s, a, b, cls = pairs_system(dtype, dim, n)
    d2 = unfused_d2(s.x[a], s.x[b])
    assert d2.dtype == O.np_dtype(dtype)
    for k in range(len(PAIR_SEPS)):
        assert (cls == k).sum() >= 2
    assert (d2[(cls == 0) | (cls == 1) | (cls == 4)] < NEAR2).all() and (d2[cls == 4] > 0).all()
    assert (d2[(cls == 2) | (cls == 3)] >= NEAR2).all()
    assert (d2[cls == 5] == 0).all()
    m = s.m.astype(np.float64)
    assert m.max() / m.min() >= 500  # three decades, up to the draw


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [257, 4099])
def test_pairs_are_sensitive_to_the_eps_term(oracle, n, dim, dtype):
    """What keeps the GPU comparison honest about eps(T) in the denominator: for some body, eps(T) / r^3 of its partner's term (the
    relative change of that term if eps were dropped) times the term's share of the body's scale reaches 100 x FORCE_TOL, at every
    angle.  In double only partners at d2 >= 2^-16 count: the far form with its first-order eps term, - eps y^3, is what could lose
    it (below, the guarded form divides by r^3 + eps).  Measured, max over bodies at theta 0.5 / 1.0, n = 4099, double: 3.7e-9 / 4.3e-8 in
    3D, 3.5e-9 / 3.5e-9 in 2D (eps / r^3 = 3.7e-9 at 2^-8, the partner nearly all of the scale); n = 257: 3.7e-9 / 3.4e-9 and
    3.7e-9 / 1.6e-8.  In float eps(T) = 1.2e-7 outweighs r^3 of every class (5.9e-8 at 2^-8): at least 1.6e7."""
    s, a, b, cls = pairs_system(dtype, dim, n)
    _, _, perm = sorted_of("pairs", n, dtype, dim)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    eps = float(np.finfo(O.np_dtype(dtype)).eps)
    x, m = s.x.astype(np.float64), s.m.astype(np.float64)
    far = unfused_d2(s.x[a], s.x[b]) >= NEAR2 if dtype == 1 else cls != 5
    for theta in THETAS:
        w = wide_of("pairs", n, dtype, dim, theta)
        best = 0.0
        for p, q in ((a[far], b[far]), (b[far], a[far])):
            r = np.sqrt(((x[p] - x[q]) ** 2).sum(1))
            term = abs(s.c) * m[q] * r / (r ** 3 + eps)
            best = max(best, float((eps / r ** 3 * term / w.scale[inv[p]]).max()))
        print(f"pairs {n} {dim}D dtype {dtype} theta {theta}: max eps / r^3 x share of scale {best:.3g}")
        assert best >= 100 * FORCE_TOL[dtype], (theta, best)


# ---- theta = 0 ---------------------------------------------------------------------------------------------------------------------
THETA0_CASES = [(name, n, dim, dtype) for name, n, dim in CASE_DIMS for dtype in (1, 0) if dtype == 1 or n <= 257]


@pytest.mark.parametrize("name, n, dim, dtype", THETA0_CASES, ids=[f"{c[0]}{c[1]}-{c[2]}D-{c[3]}" for c in THETA0_CASES])
def test_theta0_is_the_all_pairs_sum(oracle, name, n, dim, dtype):
    """theta = 0 opens every node, so the walk adds every other body once, in the tree's order: a and scale equal
    oracle.all_pairs_force_wide's (the same pair form, index order) on the state in key order to 1e-12 of scale.  Measured: 0 for both in
    every case (the leaves are visited in index order, so the sums agree term for term).  The T walk at theta = 0 against it:
    1.3e-14 of scale in double (galaxy 4099 3D), 6.7e-7 in float (uniform 257 2D).  In float only up to n = 257: the reference's
    own sequential float sum of 4098 terms measured 2.5e-5 of scale (galaxy 4099, 3D), outside FORCE_TOL — and FORCE_TOL is not
    widened to admit the larger size."""
    s, tr, _ = sorted_of(name, n, dtype, dim)
    w = oracle.bvh_walk_wide(s, tr, 0.0)
    a, sc = oracle.all_pairs_force_wide(s)
    assert np.array_equal(w.counts[:, 3], np.full(s.n, s.n - 1)) and not w.counts[:, 2].any() and not w.near_nodes.any()
    fa, fs = per_body(w.a, a, sc), per_body(w.scale, sc, sc)
    t = s.copy()
    oracle.bvh_force(t, tr, 0.0)
    ft = per_body(t.a, w.a, w.scale)
    print(f"theta 0 vs all_pairs_force_wide {name} {n} {dim}D dtype {dtype}: a {fa:.3g} scale {fs:.3g}; T walk vs wide {ft:.3g}")
    assert fa <= 1e-12 and fs <= 1e-12, (fa, fs)
    assert ft <= FORCE_TOL[dtype], ft


# ---- the front-end -----------------------------------------------------------------------------------------------------------------
def test_targets_select_rows(oracle):
    s, tr, _ = sorted_of("galaxy", 1000, 1, 3)
    w = wide_of("galaxy", 1000, 1, 3, 0.5)
    t = np.array([s.n - 1, 0, 7, 7])
    p = oracle.bvh_walk_wide(s, tr, 0.5, targets=t)
    for k in ("a", "scale", "counts", "near_nodes"):
        assert np.array_equal(getattr(p, k), getattr(w, k)[t]), k
    e = oracle.bvh_walk_wide(s, tr, 0.5, targets=np.zeros(0, np.uint32))
    assert e.a.shape == (0, 3) and e.counts.shape == (0, 4)
    with pytest.raises(AssertionError):
        oracle.bvh_walk_wide(s, tr, 0.5, targets=np.array([s.n]))


def test_a_library_without_the_symbol_is_refused(oracle, monkeypatch):
    real = oracle.lib()

    class Stale:
        def __getattr__(self, name):
            if name == "oracle_bvh_walk_wide":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(oracle, "_lib", Stale())
    s, tr, _ = sorted_of("uniform", 3, 1, 3)
    with pytest.raises(RuntimeError, match="older than oracle/nbody_oracle.c"):
        oracle.bvh_walk_wide(s, tr, 0.5)
