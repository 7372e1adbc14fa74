"""CPU: the oracle's wide references (oracle.all_pairs_force_wide, oracle.potential_wide: every operation in double for float
inputs and in long double for double inputs, the reference's eps(T) kept) against the oracle's own T arithmetic.  The GPU tests of
the float K1 above 32 768 bodies and of the energies measure the kernels against these, so they are held to the restatement of the
reference first."""
import numpy as np
import pytest


def _system(oracle, dtype, dim, wl, n):
    s = oracle.build_model(dtype, dim, wl, n)
    return s


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [300, 1000])
def test_oracle_force_within_rounding_of_the_wide_one(oracle, dtype, dim, n):
    """|a_T - a_wide| <= tol * scale_i per target, scale_i the sum of the magnitudes of the target's terms: 1e-13 in double (n
    terms of a few ulp of 1.1e-16 each in one chain), 1e-4 in float (6e-8 each)."""
    tol = 1e-13 if dtype == 1 else 1e-4
    for wl in ("galaxy", "uniform"):
        s = _system(oracle, dtype, dim, wl, n)
        oracle.all_pairs_force(s)
        a, scale = oracle.all_pairs_force_wide(s)
        assert a.shape == (s.n, dim) and scale.shape == (s.n,) and a.dtype == np.float64 and scale.dtype == np.float64
        assert np.isfinite(a).all() and np.isfinite(scale).all() and (scale > 0).all()
        assert (np.abs(a).max(axis=1) <= scale * (1 + 1e-12)).all()     # a sum never exceeds the sum of its terms' magnitudes
        err = np.abs(s.a.astype(np.float64) - a).max(axis=1) / scale
        assert err.max() <= tol, (wl, err.max())


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [300, 1000])
def test_targets_select_rows_of_the_full_call(oracle, dtype, dim, n):
    s = _system(oracle, dtype, dim, "galaxy", n)
    a, scale = oracle.all_pairs_force_wide(s)
    rng = np.random.default_rng(5 + n)
    for t in (np.array([0]), np.array([s.n - 1, 0, 7, 7]), rng.permutation(s.n)[: n // 3], np.arange(s.n, dtype=np.int64)):
        at, st = oracle.all_pairs_force_wide(s, t)
        assert np.array_equal(at, a[t]) and np.array_equal(st, scale[t])
    at, st = oracle.all_pairs_force_wide(s, np.array([], dtype=np.uint32))
    assert at.shape == (0, dim) and st.shape == (0,)


def test_wide_force_of_hand_made_pairs(oracle):
    """Two bodies at distance r: a = c m_j / (r^2 + eps(T) / r) towards the other body, scale = |a|; a coincident pair of distinct
    bodies and a zero-mass partner add exactly 0; eps(T) is the float one for float inputs (r^3 = 1e-9 << 1.19e-7)."""
    for dtype, eps in ((0, np.finfo(np.float32).eps), (1, np.finfo(np.float64).eps)):
        for r in (3.0, 2.0 ** -10, 1e-3):
            s = oracle.State(dtype, 3, 4)
            s.m[:] = [2.0, 3.0, 5.0, 0.0]
            s.x[:] = [[1, 2, 3], [1, 2, 3], [1, 2, 3], [1, 2, 3.5]]
            s.x[1, 1] += r
            s.x[2] = s.x[1]                      # body 2 coincides with body 1
            s.c = 0.25
            rr = float(s.x[1, 1]) - 2.0          # the separation the T arrays hold
            a, scale = oracle.all_pairs_force_wide(s)
            want0 = 0.25 * (3.0 + 5.0) * rr / (rr ** 3 + float(eps))
            assert abs(a[0, 1] - want0) <= 1e-14 * want0 and a[0, 0] == 0 and a[0, 2] == 0
            assert abs(scale[0] - want0) <= 1e-14 * want0
            want1 = -0.25 * 2.0 * rr / (rr ** 3 + float(eps))
            assert abs(a[1, 1] - want1) <= 1e-14 * abs(want1) and np.array_equal(a[1], a[2])


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [300, 1000])
def test_potential_wide_equals_the_t_terms_in_double(oracle, dim, n):
    """In double the terms formed in T and in long double differ by an ulp each: 1e-12 on the sum.  In float the T terms carry 6e-8
    each, with no common sign: 1e-6."""
    for wl in ("galaxy", "uniform"):
        s = _system(oracle, 1, dim, wl, n)
        _, pe = oracle.calc_energies_wide(s)
        pw = oracle.potential_wide(s)
        assert np.isfinite(pw) and pw < 0 and abs(pw - pe) <= 1e-12 * abs(pe), (wl, pw, pe)
        f = _system(oracle, 0, dim, wl, n)
        _, pe = oracle.calc_energies_wide(f)
        pw = oracle.potential_wide(f)
        assert abs(pw - pe) <= 1e-6 * abs(pe), (wl, pw, pe)


def test_calc_energies_wide_kinetic_is_the_long_double_sum(oracle):
    s = _system(oracle, 1, 3, "galaxy", 1000)
    ke, _ = oracle.calc_energies_wide(s)
    ld = np.longdouble
    want = ld(0.5) * (s.m.astype(ld) * (s.v.astype(ld) ** 2).sum(axis=1)).sum()
    assert abs(ke - float(want)) <= 1e-15 * float(want)
