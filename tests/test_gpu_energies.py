"""GPU: the energies (K10/K11, csrc/energy.hip) beyond what one global sum at n <= 6000 shows.
  1. The pair term m_j / (r + eps(T)) alone, on both sides of its near/far switch (pot_math::far / near: r2 = 2^-48 in f64, 2^-20 in
     f32) and softened, in ulps of T: a system whose masses are 0 except for one pair has PE = -c m_i m_j / (r + eps) exactly.
  2. Dense systems on both sides of n = 8192, where ap_auto_chunks starts to give a source chunk more than one tile, and at
     65 537, against oracle.potential_wide (terms and sums formed wide) and a long double kinetic sum.
  3. n > 262 144 (the second trip of energy_partial_kernel's grid-stride loop: energies_blocks caps at 1024 blocks of 256) and
     n > 2^20 (32 source chunks): the CPU cannot sum these densely, so all masses are 0 except about 3000 bodies placed at every
     edge the kernels have; PE and KE are then the sums over those bodies alone."""
import numpy as np
import pytest

from test_gpu_softening import e2_of, ref_potential

pytestmark = pytest.mark.gpu

LD = np.longdouble
T_OF = {0: np.float32, 1: np.float64}
SOFT = 0.05
# the project's tolerances: tests/test_gpu_all_pairs.py (test_near_pairs_in_another_source_tile: 1e-12 in double, 2e-6 in float
# against the wide sum) and tests/test_gpu_softening.py (test_softened_energies: 1e-13 / 1e-5)
PE_TOL = {1: 1e-12, 0: 2e-6}
PE_SOFT_TOL = {1: 1e-13, 0: 1e-5}
# KE against the long double sum: 1e-12 in double as everywhere; in float the worst case of the kernel's own sum — D + 1 roundings
# in a term, then a chain of at most 5 + 6 + 3 (thread, wave, block) + 4 + 6 + 3 (final kernel) additions of positive numbers:
# 31 * 2^-24 = 1.9e-6.
KE_TOL = {1: 1e-12, 0: 2e-6}

# Pair term, largest |PE_gpu - PE_ref| in ulps of T over every separation and pair of indices, measured on an MI355X
# (run with -s: every case prints its figure before it asserts):
#                       f64 3D   f64 2D   f32 3D   f32 2D
#   unsoftened           1.67     1.59     2.50     2.63
#   softened (0.05)      1.86     1.59     1.98     1.72
#   far form, mean signed error (ulp)   +0.013   -0.032   -0.114   -0.065
# PAIR_ULPS = 4 x the largest of the type, rounded up to a whole ulp, never above 16 (the term's own analysis in csrc/energy.hip
# gives about 3): 4 x 1.86 = 7.4 -> 8 in f64; 4 x 2.63 = 10.5 -> 11 in f32.
PAIR_ULPS = {1: 8.0, 0: 11.0}
assert max(PAIR_ULPS.values()) <= 16.0
# BIAS_ULPS bounds the MEAN signed error of the f64 far form over a case's ~300 separations, by the same rule: 4 x 0.032 = 0.13.
# The form's series is cut after the third order (what is left is below 2^-70) and every other step rounds to nearest, so its
# error has no sign of its own; a wrong series coefficient errs to ONE side and shows in the mean long before it reaches PAIR_ULPS
# (0.5 for 0.375 in pot_math<double>::far: largest error 4.4 ulp, mean +0.25 / +0.20).
BIAS_ULPS = 0.13


def auto_chunks(n):
    """ap_auto_chunks (csrc/all_pairs.hip) restated: 16 chunks, doubling while chunks * 65 536 < n, up to 64, never more than
    tiles; (chunks, tiles of 512 records per chunk)."""
    ntiles = (n + 511) // 512
    y = 16
    while y < 64 and y * 65536 < n:
        y *= 2
    y = max(1, min(y, ntiles))
    tpc = (ntiles + y - 1) // y
    return (ntiles + tpc - 1) // tpc, tpc


def test_auto_chunks_restated():
    assert auto_chunks(8191) == (16, 1) and auto_chunks(8193) == (9, 2) and auto_chunks(65537) == (15, 9)
    assert auto_chunks(262145) == (16, 33) and auto_chunks((1 << 20) + 513) == (32, 65)


def ke_ref(m, v):
    return float(LD(0.5) * (m.astype(LD) * (v.astype(LD) ** 2).sum(axis=1)).sum())


def as_oracle_state(oracle, hs):
    ref = oracle.State(hs.dtype, hs.dim, hs.n)
    ref.m[:], ref.x[:], ref.v[:], ref.c, ref.dt = hs.m, hs.x, hs.v, hs.c, hs.dt
    return ref


# ---- 1. the pair term ----------------------------------------------------------------------------------------------------

def separations(dtype, rng):
    """About 150 separations: log-uniform over the range, 32 within +-1e-6 relative of the switch r (r2 = near_bits), and the
    switch itself with its two neighbours in T."""
    t = T_OF[dtype]
    lo, hi, sw = (-40, 20, 2.0 ** -24) if dtype == 1 else (-16, 12, 2.0 ** -10)
    r = np.concatenate([2.0 ** rng.uniform(lo, hi, 115), sw * (1 + rng.uniform(-1e-6, 1e-6, 32))])
    exact = np.array([np.nextafter(t(sw), t(0)), t(sw), np.nextafter(t(sw), t(1))], np.float64)
    return r, exact


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_pair_term_on_both_sides_of_the_switch(nb, dtype, dim):
    """n = 1030 (three tiles, the last padded), every mass 0 except the pair (i, j): in one record batch, in different tiles, and
    with j in the padded last tile.  The fillers sit in a box far from the pair and m_i m_j = 0 makes every one of their terms
    exactly 0, so PE = -c m_i m_j / (r + eps(T)), softened / sqrt(r^2 + e2), with r what the T arrays hold.  Body i sits at the
    origin, so that x_j is the separation vector and separations a millionth apart stay distinct in float."""
    t = T_OF[dtype]
    n = 1030
    rng = np.random.default_rng(900 + 10 * dtype + dim)
    hs = nb.HostSystem(dtype, dim, n)
    fill = rng.uniform(3.0e6, 4.0e6, (n, dim)).astype(t)
    hs.v[:] = rng.standard_normal((n, dim)).astype(t)
    hs.c, hs.dt = 1.0, 0.01
    eps_t, e2 = LD(np.finfo(t).eps), LD(e2_of(dtype, SOFT))
    dev = nb.DeviceSystem.from_host(hs)
    worst = {False: 0.0, True: 0.0}
    signed = []                          # unsoftened far form: (|PE_gpu| - |PE_ref|) in ulps, sign kept
    for i, j in ((0, 1), (3, 517), (600, 1029)):
        mi, mj = t(1.37), t(0.73)
        hs.m[:] = 0
        hs.m[i], hs.m[j] = mi, mj
        want_ke = ke_ref(hs.m[[i, j]], hs.v[[i, j]])
        r, exact = separations(dtype, rng)
        dirs = rng.standard_normal((r.size, dim))
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        vecs = np.concatenate([dirs * r[:, None], np.eye(dim)[[0, 1 % dim, dim - 1]] * exact[:, None]]).astype(t)
        seen = set()
        for vec in vecs:
            hs.x[:] = fill
            hs.x[i] = 0
            hs.x[j] = vec
            dev.upload(hs)
            d = hs.x[j].astype(LD) - hs.x[i].astype(LD)
            r2 = (d * d).sum()
            near = float(t((hs.x[j] * hs.x[j]).sum(dtype=t))) < (2.0 ** -48 if dtype == 1 else 2.0 ** -20)
            seen.add(near)
            for soft in (False, True):
                ke, pe = dev.calc_energies(softening=SOFT if soft else 0.0)
                want = -LD(mi) * LD(mj) / (np.sqrt(r2 + e2) if soft else np.sqrt(r2) + eps_t)
                assert np.isfinite(pe) and abs(float(ke) - want_ke) <= KE_TOL[dtype] * want_ke
                ulps = float(abs(LD(pe) - want) / LD(np.spacing(t(abs(want)))))
                worst[soft] = max(worst[soft], ulps)
                if not soft and not near:
                    signed.append(float((abs(LD(pe)) - abs(want)) / LD(np.spacing(t(abs(want))))))
                assert ulps <= PAIR_ULPS[dtype], (i, j, vec, soft, pe, want, ulps)
        assert seen == {False, True}     # both forms were taken
    dev.close()
    bias = float(np.mean(signed))
    print(f"pair term dtype={dtype} dim={dim}: unsoftened {worst[False]:.2f} ulp, softened {worst[True]:.2f} ulp, "
          f"far form's mean signed error {bias:+.3f} ulp over {len(signed)}")
    if dtype == 1:
        assert len(signed) >= 250 and abs(bias) <= BIAS_ULPS, bias


# ---- 2. dense sizes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,dim,n", [(dt, d, n) for n in (8191, 8193) for dt in (1, 0) for d in (3, 2)]
                         + [(1, 3, 65537), (0, 2, 65537)])
def test_dense_energies_against_the_wide_potential(nb, oracle, dtype, dim, n):
    """galaxy on both sides of n = 8192 (one tile per source chunk / two, the last chunk short) and at 65 537 (9 tiles per chunk):
    PE against oracle.potential_wide, KE against the long double sum; at 8193 the softened potential too.
    Measured (PE, relative): double 0 ... 4e-16; float 6.3e-7 ... 8.5e-7 at 8191 / 8193 and 8.9e-7 at 65 537 in 2D.  The last case
    found a fault: with a lane's terms of a whole chunk in ONE float chain it was 8.4e-6 — seen from a galaxy's centre the other
    centre's term (4.5, half an ulp 2.4e-7) swallowed the 575 terms of 1.4e-7 after it — and csrc/potential_body.inc now sums a
    tile's 64 terms by themselves in float."""
    hs = nb.build_model(dtype, dim, "galaxy", n)
    assert hs.n == n and auto_chunks(n)[1] == {8191: 1, 8193: 2, 65537: 9}[n]
    dev = nb.DeviceSystem.from_host(hs)
    assert f"chunks={auto_chunks(n)[0]}(" in nb.describe_all_pairs(dev.state())   # the library's own ap_auto_chunks (K1 shares it)
    ke, pe = dev.calc_energies()
    want_pe = oracle.potential_wide(as_oracle_state(oracle, hs))
    want_ke = ke_ref(hs.m, hs.v)
    print(f"dense n={n} dtype={dtype} dim={dim}: PE rel {abs(float(pe) - want_pe) / abs(want_pe):.3g} "
          f"KE rel {abs(float(ke) - want_ke) / want_ke:.3g}")
    assert np.isfinite(pe) and abs(float(pe) - want_pe) <= PE_TOL[dtype] * abs(want_pe), (pe, want_pe)
    assert abs(float(ke) - want_ke) <= KE_TOL[dtype] * want_ke, (ke, want_ke)
    if n == 8193:
        ke_s, pe_s = dev.calc_energies(softening=SOFT)
        # (float inputs: float64 is the wide type, and NumPy's long double takes 9 s here)
        want = float(ref_potential(hs.m, hs.x, hs.c, e2_of(dtype, SOFT), dt=LD if dtype == 1 else np.float64))
        print(f"dense n={n} dtype={dtype} dim={dim} softened: PE rel {abs(float(pe_s) - want) / abs(want):.3g}")
        assert ke_s == ke
        assert np.isfinite(pe_s) and abs(float(pe_s) - want) <= PE_SOFT_TOL[dtype] * abs(want), (pe_s, want)
    dev.close()


# ---- 3. beyond one trip of the reduction ---------------------------------------------------------------------------------

def massive_bodies(n, rng):
    """8-index windows at index 0, at the last 8 indices, on both sides of every multiple of 262 144 (where a thread of
    energy_partial_kernel starts its next trip) and of every source-chunk edge, plus 2000 random indices."""
    chunks, tpc = auto_chunks(n)
    edges = [k * 262144 for k in range(1, n // 262144 + 1)] + [c * tpc * 512 for c in range(1, chunks)]
    idx = [np.arange(8), np.arange(n - 8, n), rng.choice(n, 2000, replace=False)]
    idx += [np.arange(e - 8, e + 8) for e in edges]
    idx = np.unique(np.concatenate(idx))
    return idx[(idx >= 0) & (idx < n)]


def sparse_mass_potential(m, x, c, e2, eps_t):
    """-c/2 sum_i sum_{j != i} m_i m_j / (r + eps_t), or / sqrt(r^2 + e2) where e2 is given, over K bodies in long double."""
    m, x = m.astype(LD), x.astype(LD)
    tot = LD(0)
    for s in range(0, len(m), 256):
        d = x[None, :, :] - x[s:s + 256][:, None, :]
        q = (d * d).sum(-1)
        inv = 1 / (np.sqrt(q) + LD(eps_t)) if e2 is None else 1 / np.sqrt(q + LD(e2))
        inv[np.arange(inv.shape[0]), np.arange(s, s + inv.shape[0])] = 0  # self term, by index
        tot += (m[s:s + 256] * (inv * m[None, :]).sum(1)).sum()
    return float(-LD(0.5) * LD(c) * tot)


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("n", [262145, (1 << 20) + 513])
def test_energies_beyond_one_trip_of_the_reduction(nb, dtype, n):
    """3D, random finite positions and velocities for every body, mass on about 3000 of them: every other body's terms are exactly
    0 (0 * finite), so PE and KE equal the sums over the massive bodies alone — wherever the kernels drop, repeat or misplace a
    body at one of their edges, a massive body sits there.  A second launch with every mass non-zero checks KE alone."""
    t = T_OF[dtype]
    chunks, tpc = auto_chunks(n)
    assert (chunks, tpc) == ((16, 33) if n == 262145 else (32, 65)) and n > 1024 * 256
    rng = np.random.default_rng(n % 1000 + dtype)
    hs = nb.HostSystem(dtype, 3, n)
    hs.x[:] = rng.uniform(-50.0, 50.0, (n, 3)).astype(t)
    hs.v[:] = rng.standard_normal((n, 3)).astype(t)
    k = massive_bodies(n, rng)
    assert 2000 <= k.size <= 3500 and {0, n - 1, 262143, 262144, tpc * 512 - 1, tpc * 512, (chunks - 1) * tpc * 512} <= set(k.tolist())
    hs.m[k] = rng.uniform(0.5, 2.0, k.size).astype(t)
    hs.c, hs.dt = 1.0, 0.01
    dev = nb.DeviceSystem.from_host(hs)
    # the library's own ap_auto_chunks, which K1's automatic launch shares: the windows of massive_bodies sit on ITS chunk edges
    assert f"chunks={chunks}(" in nb.describe_all_pairs(dev.state()) and "tile=512" in nb.describe_all_pairs(dev.state())
    want_ke = ke_ref(hs.m[k], hs.v[k])
    for soft in (False, True):
        ke, pe = dev.calc_energies(softening=SOFT if soft else 0.0)
        want = sparse_mass_potential(hs.m[k], hs.x[k], hs.c, e2_of(dtype, SOFT) if soft else None, np.finfo(t).eps)
        tol = (PE_SOFT_TOL if soft else PE_TOL)[dtype]
        print(f"n={n} dtype={dtype} soft={soft}: PE rel {abs(float(pe) - want) / abs(want):.3g} KE rel {abs(float(ke) - want_ke) / want_ke:.3g}")
        assert np.isfinite(pe) and abs(float(pe) - want) <= tol * abs(want), (soft, pe, want)
        assert abs(float(ke) - want_ke) <= KE_TOL[dtype] * want_ke, (soft, ke, want_ke)
    hs.m[:] = rng.uniform(0.5, 2.0, n).astype(t)
    dev.upload(hs)
    ke, pe = dev.calc_energies()
    want_ke = ke_ref(hs.m, hs.v)
    print(f"n={n} dtype={dtype} every mass non-zero: KE rel {abs(float(ke) - want_ke) / want_ke:.3g}")
    assert np.isfinite(pe) and abs(float(ke) - want_ke) <= KE_TOL[dtype] * want_ke, (ke, want_ke)
    dev.close()
