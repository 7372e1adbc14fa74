"""CPU: the oracle's wide octree walk (oracle.octree_walk_wide: the tree, the T monopoles and the opening decisions of
octree_step_force, everything a body accumulates formed and summed in double for float inputs and in long double for double inputs)
against what is already pinned, using the oracle alone.  tests/test_gpu_octree_wide.py measures the softened, quadrupole and
potential walks of the GPU against it per body, so it is held here first: its counters to octree_step_force's bit for bit, its
monopole force to the T walk, theta = 0 to direct sums, the root's Q and one accepted cell to NumPy longdouble, and the deep
system's sensitivity to the cells below the key depth.

This module also owns the systems both files run (CASES, state_of, wide_of).

The figures of a run are in profiles/tests_octree_wide/new_tests_figures.txt."""
import functools

import numpy as np
import pytest

import oracle as O

LD = np.longdouble
FORCE_TOL = {1: 1e-12, 0: 2e-5}    # the project's force bound (tests/test_gpu_octree.py), here per body against the body's own scale
THETA0_TOL = {1: 1e-13, 0: 3e-5}   # tests/test_gpu_tree_energy.py
SOFTENING = 0.05
THETAS = (0.5, 1.0)

# (name, n, dims); "clustered" is the 1300-body system of test_octree_small_systems_one_block_step, "deep" deep_state below
CASES = [("uniform", 2, (3, 2)), ("uniform", 3, (3, 2)), ("galaxy", 10, (3, 2)), ("uniform", 257, (3, 2)), ("galaxy", 1000, (3, 2)),
         ("uniform", 1024, (3, 2)), ("uniform", 1025, (3, 2)), ("clustered", 1300, (3,)), ("galaxy", 4099, (3, 2)),
         ("plummer", 4099, (3,)), ("galaxy", 20000, (3, 2)), ("deep", 2000, (3, 2))]
CASE_DIMS = [(name, n, dim) for name, n, dims in CASES for dim in dims]
CASE_IDS = [f"{name}{n}-{dim}D" for name, n, dim in CASE_DIMS]


def make_state(dtype, dim, x, m, c=1.0, dt=0.01):
    s = O.State(dtype, dim, len(m))
    t = O.np_dtype(dtype)
    s.m[:], s.x[:] = np.asarray(m, t), np.asarray(x, t)
    s.c, s.dt = c, dt
    return s


def deep_state(dtype, dim):
    """tests/test_gpu_octree.py's below-the-key-depth system — two escapers at +-9000 inflate the root cube to a side of 18 002, a
    core of 100 bodies (sigma 2e-4) lies below the 21 key levels of 3D (cells of 8.6e-3 there), and in double six close pairs are split
    35 - 45 levels down — with one change so that every dimension and dtype accepts cells below its key depth: in 2D, whose 32 key
    levels end at cells of 4.2e-6, bodies 400 .. 599 form a second core of sigma 1e-5 around 2^-10 (where float still resolves
    1.2e-10).  Its cells of depth 32 and more are accepted from 8e-6 or further, 70 eps(float): far enough that the reference's
    dist + eps(T) does not let a body accept a cell it sits in."""
    rng = np.random.default_rng(11 + dim)
    n = 2000
    x = rng.uniform(-1.0, 1.0, (n, dim))
    x[0] = 9000.0
    x[1] = -9000.0
    x[100:200] = 0.25 + 2e-4 * rng.standard_normal((100, dim))
    if dtype == 1:
        for k in range(6):
            x[300 + 2 * k + 1] = x[300 + 2 * k] + 10.0 ** (-7 - k // 2)
    m = rng.uniform(0.5, 2.0, n)
    if dim == 2:
        x[400:600] = 2.0 ** -10 + 1e-5 * rng.standard_normal((200, dim))
    return make_state(dtype, dim, x, m)


def clustered_state(dtype, dim):
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (1300, 3)).astype(np.float32)
    x[1:600:2] = x[0:600:2] + np.float32(2.0 ** -7)
    return make_state(dtype, dim, x[:, :dim], np.ones(1300), dt=1e-3)


@functools.lru_cache(maxsize=None)
def state_of(name, n, dtype, dim):
    """The system of a case (shared: do not modify)."""
    if name == "deep":
        return deep_state(dtype, dim)
    if name == "clustered":
        return clustered_state(dtype, dim)
    return O.build_model(dtype, dim, name, n)


@functools.lru_cache(maxsize=None)
def wide_of(name, n, dtype, dim, theta):
    """The wide walk of a case at softening 0.05, computed once (shared: do not modify)."""
    return O.octree_walk_wide(state_of(name, n, dtype, dim), theta, SOFTENING)


def direct_sums(s, e2=None, form="walk"):
    """NumPy longdouble direct sums over j != i (by index) on the T arrays of s: (a / c, S) with the walk's unsoftened pair
    m d / (r + eps(T))^3 and m / (r + eps(T)), or, with e2, the softened m d / (r^2 + e2)^(3/2) and m / sqrt(r^2 + e2)."""
    m, x = s.m.astype(LD), s.x.astype(LD)
    eps = LD(np.finfo(O.np_dtype(s.dtype)).eps)
    a, S = np.zeros((s.n, s.dim), LD), np.zeros(s.n, LD)
    for lo in range(0, s.n, 256):
        d = x[None, :, :] - x[lo:lo + 256][:, None, :]
        r2 = (d * d).sum(-1)
        if e2 is None:
            r = np.sqrt(r2) + eps
            w3, w1 = m[None, :] / (r * r * r), m[None, :] / r
        else:
            q = r2 + LD(e2)
            w3, w1 = m[None, :] / (q * np.sqrt(q)), m[None, :] / np.sqrt(q)
        own = (np.arange(d.shape[0]), np.arange(lo, lo + d.shape[0]))
        w1[own] = 0
        a[lo:lo + 256] = (w3[:, :, None] * d).sum(1)
        S[lo:lo + 256] = w1.sum(1)
    return a, S


def per_body(got, want, scale):
    """max over bodies (and components) of |got - want| / scale_i."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    err = err.max(axis=1) if err.ndim == 2 else err
    return float((err / scale).max())


# ---- 1, 2: counters and the monopole force against the T walk ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("name, n, dim", CASE_DIMS, ids=CASE_IDS)
def test_counters_and_monopole_force_equal_the_t_walk(oracle, name, n, dim, dtype):
    """counts is octree_step_force's bit for bit; |a_T - a_mono| <= FORCE_TOL * scale_a_mono per body and component, the bound the GPU
    is held to.  Measured over all cases: 3.2e-15 of scale in double, 1.7e-6 in float (galaxy 20000, theta 0.5) — the figure a
    widening of the float bound would have to be justified with (at most 4 x that)."""
    for theta in THETAS:
        s = state_of(name, n, dtype, dim).copy()
        cnt, _, _ = oracle.octree_step_force(s, theta, want_counts=True)
        w = wide_of(name, n, dtype, dim, theta)
        assert np.array_equal(w.counts, cnt), theta
        for k in ("a_mono", "a_soft", "a_quad", "a_quad_deep", "s_mono", "s_soft", "s_quad", "scale_a_mono", "scale_a_soft",
                  "scale_a_quad", "scale_s_mono", "scale_s_soft", "scale_s_quad"):
            v = getattr(w, k)
            assert v.dtype == np.float64 and len(v) == s.n and np.isfinite(v).all(), k
        assert (w.scale_a_mono > 0).all() and (w.scale_a_quad >= w.scale_a_mono).all() and (w.scale_s_quad >= w.scale_s_mono).all()
        for a, sc in ((w.a_mono, w.scale_a_mono), (w.a_soft, w.scale_a_soft), (w.a_quad, w.scale_a_quad)):
            assert (np.abs(a).max(axis=1) <= sc * (1 + 1e-12)).all()  # a sum never exceeds the sum of its terms' magnitudes
        err = per_body(s.a, w.a_mono, w.scale_a_mono)
        print(f"T walk vs wide {name} {n} {dim}D dtype {dtype} theta {theta}: max err_i {err:.3g}")
        assert err <= FORCE_TOL[dtype], (theta, err)


def test_targets_select_rows_and_softening_is_optional(oracle):
    s = state_of("galaxy", 1000, 1, 3)
    w = wide_of("galaxy", 1000, 1, 3, 0.5)
    t = np.array([s.n - 1, 0, 7, 7])
    p = oracle.octree_walk_wide(s, 0.5, SOFTENING, targets=t)
    for k in ("a_mono", "a_soft", "a_quad", "s_mono", "s_soft", "s_quad", "scale_a_quad", "scale_s_soft", "counts"):
        assert np.array_equal(getattr(p, k), getattr(w, k)[t]), k
    assert np.array_equal(p.root_q, w.root_q)
    u = oracle.octree_walk_wide(s, 0.5)
    assert u.a_soft is None and u.s_soft is None and u.scale_a_soft is None and u.scale_s_soft is None
    assert np.array_equal(u.a_quad, w.a_quad) and np.array_equal(u.s_mono, w.s_mono)
    # split_level: 0 puts every accepted cell's term into a_quad_deep, a level no cell reaches none
    assert np.allclose(oracle.octree_walk_wide(s, 0.5, split_level=0).a_quad_deep, w.a_quad - w.a_mono, rtol=0, atol=1e-18)
    assert not oracle.octree_walk_wide(s, 0.5, split_level=200).a_quad_deep.any()
    with pytest.raises(AssertionError):
        oracle.octree_walk_wide(s, 0.5, targets=np.array([s.n]))


def test_a_library_without_the_symbol_is_refused(oracle, monkeypatch):
    real = oracle.lib()

    class Stale:
        def __getattr__(self, name):
            if name == "oracle_octree_walk_wide":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(oracle, "_lib", Stale())
    with pytest.raises(RuntimeError, match="older than oracle/nbody_oracle.c"):
        oracle.octree_walk_wide(state_of("uniform", 3, 1, 3), 0.5)


# ---- 3: theta = 0 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_theta0_is_the_direct_sum(oracle, dtype, dim):
    """theta = 0 opens every cell, so each sum is a direct sum over the other bodies and a_quad, s_quad are the monopole sums.
    Against NumPy longdouble sums of the same pair forms, uniform n = 1000: 1e-12 of scale for the forces, 1e-13 for the potentials
    (measured: at most 2.2e-16 — for float inputs too: their wide type is double).
    Against oracle.all_pairs_force_wide the pair forms differ in where eps(T) enters, m d / (r + eps)^3 here and m d / (r^3 + eps)
    there: a relative eps / r^3 - 3 eps / r per pair.  Measured on uniform systems, max over bodies of |difference| / scale: n = 16
    (closest pair 0.17) 1.9e-14 in double and 1.0e-5 in float; n = 100 (0.086 / 0.0076 in 3D / 2D) 1.5e-13 / 4.1e-10 and
    7.8e-5 / 0.17; n = 1000 1.1e-10 / 5.9e-8 and 0.05 / 0.9.  So that comparison is made at n = 16, under the force bounds."""
    s = state_of("uniform", 1000, dtype, dim)
    w = oracle.octree_walk_wide(s, 0.0, SOFTENING)
    t = O.np_dtype(dtype)
    e2 = t(t(SOFTENING) * t(SOFTENING))
    am, sm = direct_sums(s)
    asf, ssf = direct_sums(s, e2)
    c = LD(s.c)
    figs = {"a_mono": per_body(w.a_mono, c * am, w.scale_a_mono), "a_soft": per_body(w.a_soft, c * asf, w.scale_a_soft),
            "s_mono": per_body(w.s_mono, sm, w.scale_s_mono), "s_soft": per_body(w.s_soft, ssf, w.scale_s_soft)}
    print(f"theta 0 vs longdouble direct sums, uniform 1000 {dim}D dtype {dtype}: " + " ".join(f"{k} {v:.3g}" for k, v in figs.items()))
    assert figs["a_mono"] <= 1e-12 and figs["a_soft"] <= 1e-12, figs
    assert figs["s_mono"] <= 1e-13 and figs["s_soft"] <= 1e-13, figs
    assert np.array_equal(w.a_quad, w.a_mono) and np.array_equal(w.s_quad, w.s_mono) and not w.a_quad_deep.any()
    assert np.array_equal(w.counts[:, 1], np.full(s.n, w.counts[0, 1]))  # every body accepts every leaf
    s16 = state_of("uniform", 16, dtype, dim)
    w16 = oracle.octree_walk_wide(s16, 0.0)
    a16, sc16 = oracle.all_pairs_force_wide(s16)
    gap = per_body(w16.a_mono, a16, w16.scale_a_mono)
    print(f"theta 0 vs all_pairs_force_wide, uniform 16 {dim}D dtype {dtype}: a_mono {gap:.3g}")
    assert gap <= FORCE_TOL[dtype], gap
    assert np.abs(sc16 / w16.scale_a_mono - 1).max() <= 2 * FORCE_TOL[dtype]


# ---- 4: Q ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("name, n, dim", [c for c in CASE_DIMS if c[1] >= 1000], ids=[i for c, i in zip(CASE_DIMS, CASE_IDS) if c[1] >= 1000])
def test_root_quadrupole_against_numpy(oracle, name, n, dim, dtype):
    """The root's Q against tests/test_gpu_quadrupole.py's quad_ref in longdouble, relative to its largest component: 1e-15 in
    double.  (Q is taken about the root's T centre of mass, quad_ref's about the longdouble one, a distance delta apart: the
    dipole about the centre of mass is 0, so the two differ by M (3 delta delta^T - |delta|^2 I), second order.)  In float delta is
    at most (tree depth) eps(float) of the extent, (64 x 1.2e-7)^2 = 5.9e-11 of Q: 1e-10."""
    from test_gpu_quadrupole import quad_ref
    s = state_of(name, n, dtype, dim)
    want, _ = quad_ref(s.m, s.x)
    got = wide_of(name, n, dtype, dim, 0.5).root_q
    err = float(np.abs(got.astype(LD) - want).max() / np.abs(want).max())
    print(f"root Q {name} {n} {dim}D dtype {dtype}: {err:.3g}")
    assert err <= (1e-15 if dtype == 1 else 1e-10), err


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_one_cluster_one_probe(oracle, dtype, dim):
    """test_gpu_quadrupole.py's geometry: the probe opens the root and accepts the ball's cell as one node, so its a_quad and s_quad
    are that file's and test_gpu_tree_energy.py's longdouble expansions of the ball about its centre of mass (with the ball's
    longdouble centre of mass for the cell's T one: 1e-14 in double, 1e-6 in float, of the value)."""
    from test_gpu_quadrupole import expansion
    from test_gpu_tree_energy import expansion_s
    rng = np.random.default_rng(5 + dim)
    k = 40
    ball = 1.0 + 0.3 * rng.uniform(-1, 1, (k, dim)) / np.sqrt(dim)
    x = np.vstack([ball, -3.0 * np.ones((1, dim))])
    m = np.concatenate([rng.uniform(0.5, 1.5, k) / k, [1e-3]])
    s = make_state(dtype, dim, x, m, c=0.75)
    eps = float(np.finfo(O.np_dtype(dtype)).eps)
    w = oracle.octree_walk_wide(s, 0.7, SOFTENING, targets=[k])
    assert list(w.counts[0]) == [1 + (1 << dim), 1 << dim]
    mono, quad = expansion(s.m[:k], s.x[:k], s.x[k], s.c, eps=eps)
    smono, squad = expansion_s(s.m[:k], s.x[:k], s.x[k], eps)
    tol = 1e-14 if dtype == 1 else 1e-6
    assert np.abs(w.a_mono[0] - mono).max() <= tol * np.abs(mono).max()
    assert np.abs(w.a_quad[0] - quad).max() <= tol * np.abs(quad).max()
    assert abs(w.s_mono[0] - smono) <= tol * abs(smono) and abs(w.s_quad[0] - squad) <= tol * abs(squad)
    assert np.abs(w.a_quad[0] - w.a_mono[0]).max() > 100 * tol * np.abs(mono).max()  # the term is there (2.6e-4 of the monopole)
    assert not w.a_quad_deep.any()


# ---- 5: the deep system feels the cells below the key depth -----------------------------------------------------------------------
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_deep_system_is_sensitive_to_the_deep_cells(oracle, dtype, dim, theta):
    """What keeps the GPU comparison honest about the quadrupoles of cells below the key depth (21 levels in 3D, 32 in 2D): the
    quadrupole terms of accepted cells at those depths must reach 100 x the force tolerance of some body's scale, or a wrong Q
    there would pass.  Measured, max_i |a_quad_deep_i| / scale_a_quad_i at theta 0.5 / 1.0: 3D 1.6e-2 / 4.6e-2 in both dtypes (100
    bodies over the mark in double, 53 / 99 in float); 2D 1.7e-2 / 8.0e-2 in double, 2.5e-2 / 9.0e-2 in float."""
    w = wide_of("deep", 2000, dtype, dim, theta)
    assert oracle.KEY_LEVELS == {3: 21, 2: 32}
    sens = np.abs(w.a_quad_deep).max(axis=1) / w.scale_a_quad
    print(f"deep system {dim}D dtype {dtype} theta {theta}: max |a_quad_deep| / scale {sens.max():.3g}, "
          f"{int((sens >= 100 * FORCE_TOL[dtype]).sum())} bodies over 100 x tol")
    assert sens.max() >= 100 * FORCE_TOL[dtype], sens.max()
    # the cells are accepted as cells, not from inside: no body's quadrupole terms outweigh its monopole terms many times over
    assert (w.scale_a_quad <= 2 * w.scale_a_mono).all()
