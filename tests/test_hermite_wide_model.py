"""CPU: the wide reference of tests/hermite_wide_model.py against mpmath, and the per-body criteria of tests/test_gpu_hermite_wide.py
applied to a plain same-precision NumPy evaluation: they must be reachable (an honest evaluation passes them) and have teeth (a seeded
arithmetic fault that the older global criterion lets through fails them).

Measured here (worst over the cases of each test; figures in profiles/tests_hermite_wide/figures.txt):
  mpmath     longdouble sums within 2^-58 S: worst 0.027 of that; scales within 1e-15: worst 1.5e-19.
  reachable  worst E of a / jerk / snap up to 5889 bodies 36.9 / 19.1 / 4.05 in float64 and 29.6 / 8.62 / 2.17 in float32, at 65537
             bodies 232 / 178 and 291 / 55.3 (a chain of n additions; bounds P_g + n).
  pairs      honest NumPy pair terms: worst E 2.40 / 2.30 / 2.35 (float64), 1.97 / 1.65 / 1.45 (float32) under bounds 4 / 6.5 / 8.5 and
             6 / 10 / 13.5.
  teeth      w (1 + 2^-44): global 5.8e-14 (passes 1e-12), pair E_a 256 (bound 4); w (1 + 2^-18): global 3.9e-6 (passes 2e-5), pair
             E_a 33 (bound 6); c twice on the snap: no change at c = 1, worst per-body E_s 2.2e15 / 3.5e6 at c = 0.37 (bounds 264 / 269)."""
import mpmath
import numpy as np
import pytest

import hermite_wide_model as W
from hermite_wide_model import LD, P


def test_longdouble_is_wide():
    """A platform whose long double is the 64-bit double must fail here, loudly: every bound of the wide tests assumes the reference's
    own rounding (2^-63 per operation) is far below eps_T."""
    assert np.finfo(np.longdouble).eps < 2e-19


def to_mp(z):
    """A longdouble (or narrower) number as an mpf, exactly: its 64-bit significand fits two doubles."""
    z = LD(z)
    hi = float(z)
    return mpmath.mpf(hi) + mpmath.mpf(float(z - LD(hi)))


def mp_sums(m, x, v, acc, c, e2, i):
    """The three sums and scales of body i in mpmath (components as lists)."""
    mp = mpmath.mpf
    n, D = x.shape
    c, e2 = mp(float(c)), mp(float(e2))
    a, j, s = ([mp(0)] * D for _ in range(3))
    S = [mp(0)] * 3
    for k in range(n):
        d = [mp(float(x[k, t])) - mp(float(x[i, t])) for t in range(D)]
        u = [mp(float(v[k, t])) - mp(float(v[i, t])) for t in range(D)]
        b = [mp(float(acc[k, t])) - mp(float(acc[i, t])) for t in range(D)]
        dd, uu, bb = (sum(p * p for p in z) for z in (d, u, b))
        q = dd + e2
        w = mp(float(m[k])) / (q * mpmath.sqrt(q))
        al = sum(p * r for p, r in zip(d, u)) / q
        ga = (uu + sum(p * r for p, r in zip(d, b))) / q
        nd, nu, nb = mpmath.sqrt(dd), mpmath.sqrt(uu), mpmath.sqrt(bb)
        a = [a[t] + w * d[t] for t in range(D)]
        j = [j[t] + w * (u[t] - 3 * al * d[t]) for t in range(D)]
        s = [s[t] + w * (b[t] - 6 * al * u[t] + (15 * al * al - 3 * ga) * d[t]) for t in range(D)]
        S[0] += abs(w) * nd
        S[1] += abs(w) * (nu + 3 * dd * nu / q)
        S[2] += abs(w) * (nb + 6 * nd * uu / q + (15 * dd * uu / (q * q) + 3 * (uu + nd * nb) / q) * nd)
    return [[c * z for z in g] for g in (a, j, s)], [abs(c) * z for z in S]


@pytest.mark.parametrize("dim", [3, 2])
def test_wide_against_mpmath(dim):
    """n = 8 with a coincident pair (different velocities) and a zero mass, c = 0.37, eps = 0.05, mpmath at 40 digits: every longdouble
    sum within 2^-58 S of mpmath's, every scale within 1e-15 relative.  Measured: 0.027 x 2^-58 S and 1.5e-19."""
    mpmath.mp.dps = 40
    rng = np.random.default_rng(dim)
    n = 8
    m, x, v = rng.uniform(0.5, 1.5, n), rng.normal(0, 1, (n, dim)), rng.normal(0, 1, (n, dim))
    acc = rng.normal(0, 1, (n, dim))
    x[5] = x[2]
    m[6] = 0
    e2 = W.e2_of(np.float64, 0.05)
    (a, j, s), scales = W.wide(m, x, v, acc, W.C, e2)
    worst_sum = worst_scale = 0
    for i in range(n):
        refs, rscales = mp_sums(m, x, v, acc, W.C, e2, i)
        for got, ref, S in zip((a, j, s), refs, rscales):
            for k in range(dim):
                worst_sum = max(worst_sum, abs(to_mp(got[i, k]) - ref[k]) / (mpmath.mpf(2) ** -58 * S))
        for got, S in zip(scales, rscales):
            worst_scale = max(worst_scale, abs(to_mp(got[i]) - S) / S)
    print(f"dim={dim}: sums {float(worst_sum):.3g} of 2^-58 S, scales {float(worst_scale):.3g}")
    assert worst_sum <= 1 and worst_scale <= 1e-15


def plain_start(T, m, x, v, c, e2, targets, order, **fault):
    """What the start of either order computes, in plain NumPy of type T: order 4 a and the jerk; order 6 a of ALL bodies first, then a,
    jerk and snap with those accelerations.  Returns the sums of the targets and the acc used (None for order 4)."""
    if order == 4:
        return W.pair_sums(T, m, x, v, None, c, e2, targets, **fault)[0], None
    acc = W.pair_sums(T, m, x, v, None, c, e2, None, **fault)[0][0]
    return W.pair_sums(T, m, x, v, acc, c, e2, targets, **fault)[0], acc


def worst_units(T, got, m, x, v, acc, c, e2, targets):
    """Worst E_g over the targets for each quantity of `got` against the wide reference, and the reference's largest magnitude."""
    refs, scales = W.wide(m, x, v, acc, c, e2, targets)
    big = max(float(np.abs(z).max()) for z in refs + scales if z is not None)
    return [float(W.err_units(g, r, S, T).max()) for g, r, S in zip(got, refs, scales) if r is not None], big


@pytest.mark.parametrize("n", [65, 257, 1000, 5889, 65537])
@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("dim", [3, 2])
def test_bound_is_reachable(T, dim, n):
    """The adversarial systems of the GPU tests, evaluated in plain NumPy of type T (sources added one after the other: L = n): every
    evaluated body within P_g + n, everything finite, every reference value and scale below W.adv_limit.  At n = 65537 a and the jerk only:
    the accelerations of all bodies, which the snap needs as input, cost 4e9 NumPy pairs (on the GPU the library makes them).
    Measured: worst E 36.9 / 19.1 / 4.05 in float64 and 29.6 / 8.62 / 2.17 in float32 up to 5889 bodies, 232 / 178 and 291 / 55.3 at
    65537."""
    m, x, v, planted = W.adversarial(T, dim, n)
    e2 = W.e2_of(T, W.ADV_EPS[T])
    t = W.targets_for(n, planted)
    got, acc = plain_start(T, m, x, v, W.C, e2, t, 6 if n < 65537 else 4)
    assert all(g.dtype == T and np.isfinite(g).all() for g in got if g is not None)
    worst, big = worst_units(T, got, m, x, v, acc, W.C, e2, t)
    print(f"T={T.__name__} dim={dim} n={n}: E " + " ".join(f"{w:.3g}" for w in worst) + f" bounds P + {n}; largest |ref| or scale {big:.3g}")
    assert big < W.adv_limit(T, n)
    assert all(w <= p + n for w, p in zip(worst, P[T])), worst


def pair_units(T, dim, eps, **fault):
    """Worst E_a, E_j, E_s over 64 isolated pairs evaluated in plain NumPy of type T (order 6's start)."""
    m, x, v = W.isolated_pairs(T, dim, 64, eps, seed=1)
    e2 = W.e2_of(T, eps)
    worst = np.zeros(3)
    for p in range(len(m)):
        got, acc = plain_start(T, m[p], x[p], v[p], W.C, e2, None, 6, **fault)
        worst = np.maximum(worst, worst_units(T, got, m[p], x[p], v[p], acc, W.C, e2, None)[0])
    return worst


@pytest.mark.parametrize("T,eps", [(np.float64, 0.05), (np.float64, 1e-9), (np.float32, 0.05), (np.float32, 1e-4)])
@pytest.mark.parametrize("dim", [3, 2])
def test_pair_bound_is_reachable(T, dim, eps):
    """64 isolated pairs in plain NumPy (fewer roundings than the kernels' pair: one division where they take a reciprocal square root
    and a series): within P_g + 1.5.  Measured: worst 2.40 / 2.30 / 2.35 in float64, 1.97 / 1.65 / 1.45 in float32."""
    worst = pair_units(T, dim, eps)
    print(f"T={T.__name__} dim={dim} eps={eps}: E " + " ".join(f"{w:.3g}" for w in worst))
    assert all(w <= p + W.PAIR_EXTRA for w, p in zip(worst, P[T])), worst


@pytest.mark.parametrize("T,factor", [(np.float64, 1 + 2.0 ** -44), (np.float32, 1 + 2.0 ** -18)])
def test_teeth_pair_weight(T, factor):
    """w scaled by (1 + 2^-44) in double, (1 + 2^-18) in float: on the Gaussian cluster of the older tests (n = 300, c = 1, eps = 0.05)
    a, jerk and snap stay within the global TOL; on the isolated pairs E_a exceeds P_a + 1.5.  Measured: global 5.8e-14 / 3.9e-6, pair
    E_a 256 / 33 against 4 / 6."""
    m, x, v = W.gaussian_cluster(T, 3, 300, seed=7)
    e2 = W.e2_of(T, 0.05)
    got, acc = plain_start(T, m, x, v, 1.0, e2, None, 6, w_factor=factor)
    refs, _ = W.wide(m, x, v, acc, 1.0, e2)
    glob = max(W.maxrel(g, r) for g, r in zip(got, refs))
    worst = pair_units(T, 3, 0.05, w_factor=factor)
    print(f"T={T.__name__}: global {glob:.3g} (TOL {W.TOL[T]:g}); pair E " + " ".join(f"{w:.3g}" for w in worst))
    assert glob <= W.TOL[T]
    assert worst[0] > P[T][0] + W.PAIR_EXTRA


@pytest.mark.parametrize("T", [np.float64, np.float32])
def test_teeth_c_twice_on_the_snap(T):
    """c applied twice to the snap: nothing at c = 1 (the older tests' only value), far outside P_s + n on the adversarial system
    (n = 257) at c = 0.37, where a and the jerk still pass.  Measured: worst E_s 2.2e15 (float64), 3.5e6 (float32) against 264 / 269."""
    m, x, v = W.gaussian_cluster(T, 3, 300, seed=7)
    e2 = W.e2_of(T, 0.05)
    got, acc = plain_start(T, m, x, v, 1.0, e2, None, 6, snap_c_twice=True)
    refs, _ = W.wide(m, x, v, acc, 1.0, e2)
    assert max(W.maxrel(g, r) for g, r in zip(got, refs)) <= W.TOL[T]
    n = 257
    m, x, v, _ = W.adversarial(T, 3, n)
    e2 = W.e2_of(T, W.ADV_EPS[T])
    got, acc = plain_start(T, m, x, v, W.C, e2, None, 6, snap_c_twice=True)
    worst, _ = worst_units(T, got, m, x, v, acc, W.C, e2, None)
    print(f"T={T.__name__}: E " + " ".join(f"{w:.3g}" for w in worst))
    assert worst[0] <= P[T][0] + n and worst[1] <= P[T][1] + n
    assert worst[2] > P[T][2] + n


def test_plans_and_chain_lengths():
    """plan_for restates hermite_plan_for: the boundaries the comment of csrc/hermite_tile.hpp and the older tests name."""
    assert W.plan_for(2, 1) == (1, 1, 1, 1, 1) and W.plan_for(257, 1)[3:] == (2, 1) and W.plan_for(257, 2)[3:] == (2, 1)
    assert W.plan_for(5888, 1)[3:] == (23, 1) and W.plan_for(5889, 1)[3:] == (12, 2)
    assert W.plan_for(5888, 2)[3:] == (23, 1) and W.plan_for(5889, 2)[3:] == (12, 2)
    assert W.plan_for(65535, 1)[0] == 1 and W.plan_for(65537, 1)[0] == 2
    assert W.block_plan_for(20000, 20000, 2) == W.plan_for(20000, 2) and W.block_plan_for(20000, 64, 2)[3:] == (79, 1)
    assert W.chain_length(W.plan_for(2, 1)) == 68 and W.chain_length(W.plan_for(5889, 2)) == 128 + 3 + 11 + 1
