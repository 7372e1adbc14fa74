"""GPU: all-pairs k nearest neighbours, local densities and the density centre (nbody_knn_*) against NumPy longdouble written here from
the T-typed inputs (the reference project has no counterpart, so there are no fixtures).  The random systems and the choice of targets
are those of tests/test_gpu_neighbours.py (seed 100 + n; all bodies up to 4097, a fixed subset above, bodies 0 and n - 1 included).

Launch-shape boundaries of the sweep (knn_plan_for(sz) of csrc/knn.hip), each with a size on either side: one LDS tile of 256 records
and one chunk | two tiles, two chunks (256 / 257); one tile per chunk | several (5888 / 5889); the plan never goes back to one chunk
and has one target per lane at every size.  Beside them the wave's slice of 64 records (63 / 64 / 65), a last tile that is nearly all
padding (257, 513, 4097, 5889, 65537), the sizes 1, 2, 3 and k, k + 1 for every k (a list that is not full | just full), and the list
capacities 4 | 8 | 16 from either side (k = 4 / 5, 8 / 9).

Bounds, with D2 exact (longdouble) and eps_T the machine epsilon of T — those derived in tests/test_gpu_neighbours.py: each difference
rounds once, the D squares and adds round once each, all terms are positive, so a computed d2 is within (D + 2) u = 2.5 eps_T of the
exact one and two compared values within 5 eps_T.  Hence per slot s: |d2_s - D2(i, idx_s)| <= 4 eps_T D2 and D2(i, idx_s) <= (s-th
smallest exact D2)(1 + 8 eps_T).  A slot's index must be the exact one where its exact order statistic is clear of BOTH its
neighbours in the order (s - 1 and s + 1, the latter up to k + 1) by more than a factor 1 + 8 eps_T: a slot may legitimately change
places with either.  The share of slots without such a clear gap may be at most 1e-3 per case, else the test fails.
Density: relative error <= 32 eps_T against longdouble from the GPU's own idx (M has <= 14 roundings of positive terms, d2_k is within
2.5 eps_T and raised to 3/2, sqrt, two products and the divide round once each: <= 22 eps_T at k = 16).  Summary: TOL = {f64: 1e-12,
f32: 2e-5}, the project's bound for a summed quantity, against longdouble from the GPU's own rho.

Measured on an MI355X, worst over all sizes, k, 2D and 3D (192 cases per type): |d2 - D2| / D2 1.74 eps_T in double, 1.91 in float;
slots without a clear gap 0 of 430 614 in double, 4 in float (all in one case: 3D, n = 4097, k = 16), every other slot the exact neighbour; rho 4.76 eps_T
in double, 4.52 in float; x_dc 1.95e-16 / 3.67e-8, r_c 1.82e-16 / 5.76e-8, rho_c 4.51e-16 / 5.58e-8; the sanity case: |x_dc - shift| =
0.0169 against r_c = 0.987 and |com - shift| = 0.434.  The figures per case, as the tests print them (-s), are in
profiles/knn/gpu_test_suite.txt."""
import ctypes
import functools
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TOL = {1: 1e-12, 0: 2e-5}  # the project's bound for a summed quantity against NumPy
LD = np.longdouble
NONE = 0xFFFFFFFF
KS = [1, 2, 6, 16]
KS_CAPACITY = [4, 5, 8, 9]  # either side of the list capacities, at one mid size
MID = 1000
SIZES = [1, 2, 3, 4, 6, 7, 16, 17, 63, 64, 65, 255, 256, 257, 513, 1000, 4097, 5888, 5889, 20000, 65535, 65536, 65537]
NREF = 17  # exact order statistics kept per target: k + 1 at k = 16


def npt(dtype):
    return np.float32 if dtype == 0 else np.float64


def eps_t(dtype):
    return float(np.finfo(npt(dtype)).eps)


def random_system(nb, dtype, dim, n, seed, c=1.0):
    rng = np.random.default_rng(seed)
    t = npt(dtype)
    hs = nb.HostSystem(dtype, dim, n)
    hs.m[:] = rng.uniform(0.5, 1.5, n).astype(t) / n
    hs.x[:] = rng.normal(0, 1, (n, dim)).astype(t)
    hs.v[:] = rng.normal(0, 0.3, (n, dim)).astype(t)
    hs.dt, hs.c = 0.01, c
    return hs


def targets_of(n):
    if n <= 4097:
        return np.arange(n)
    k = 256 if n <= 20000 else 64
    rng = np.random.default_rng(7 + n)
    t = rng.choice(n, k, replace=False)
    t[0], t[1] = 0, n - 1
    return np.unique(t)


def exact_d2_rows(x, targets):
    """Yields (slice of targets, D2 rows in longdouble with the self pair at +inf)."""
    x = np.asarray(x, LD)
    n = len(x)
    step = max(1, min(256, (1 << 21) // max(n, 1)))
    for s in range(0, len(targets), step):
        t = targets[s:s + step]
        d = x[None, :, :] - x[t][:, None, :]
        D2 = (d * d).sum(-1)
        D2[np.arange(len(t)), t] = np.inf
        yield slice(s, s + len(t)), D2


@functools.lru_cache(maxsize=None)
def case(dtype, dim, n):
    """One random system per (dtype, dim, n) and, for its targets in longdouble from the T-typed inputs, the NREF smallest exact D2 in
    ascending order with their indices (+inf, NONE where a body has fewer) — computed once, shared by every k, never changed."""
    from conftest import load_package
    nb = load_package()
    hs = random_system(nb, dtype, dim, n, seed=100 + n)
    t = targets_of(n)
    m = min(NREF, n - 1)
    val = np.full((len(t), NREF), np.inf, LD)
    arg = np.full((len(t), NREF), NONE, np.int64)
    if m > 0:
        for sl, D2 in exact_d2_rows(hs.x, t):
            part = np.sort(np.argpartition(D2, m - 1, axis=1)[:, :m], axis=1) if m < n else np.tile(np.arange(n), (D2.shape[0], 1))
            v = np.take_along_axis(D2, part, 1)
            o = np.argsort(v, axis=1, kind="stable")  # part ascends by index: ties to the lowest index
            val[sl, :m] = np.take_along_axis(v, o, 1)
            arg[sl, :m] = np.take_along_axis(part, o, 1)
    val.setflags(write=False)
    arg.setflags(write=False)
    return hs, t, val, arg


def gather_d2(x, targets, idx):
    """Exact D2(t, idx[t, s]) in longdouble, +inf where idx is NONE."""
    x = np.asarray(x, LD)
    j = np.where(idx == NONE, 0, idx).astype(np.int64)
    d = x[j] - x[targets][:, None, :]
    D2 = (d * d).sum(-1)
    D2[idx == NONE] = np.inf
    return D2


def reference_rho(m, x, idx, k, dim):
    """rho of every body in longdouble from the given neighbour lists."""
    n = len(m)
    if k == 1 or n <= k:
        return np.zeros(n, LD)
    M = np.asarray(m, LD)[idx[:, :k - 1].astype(np.int64)].sum(1)
    d2k = gather_d2(x, np.arange(n), idx[:, k - 1:k])[:, 0]
    pi = LD("3.14159265358979323846264338327950288")
    with np.errstate(divide="ignore"):
        return M / (pi * 4 / 3 * d2k * np.sqrt(d2k)) if dim == 3 else M / (pi * d2k)


def reference_summary(rho, x):
    rho, x = np.asarray(rho, LD), np.asarray(x, LD)
    s1, s2 = rho.sum(), (rho * rho).sum()
    xdc = (rho[:, None] * x).sum(0) / s1
    rc = np.sqrt((rho * rho * ((x - xdc) ** 2).sum(1)).sum() / s2)
    return xdc, rc, s2 / s1, (rho[:, None] * np.abs(x)).sum(0) / s1


def gpu_all(dev, k):
    h = dev.knn_handle(k)
    h.compute(dev.state(), dev.stream)
    return h.read(0, dev.stream), h.read(1, dev.stream), h.read(2, dev.stream), h.density_centre(dev.stream)


def summary_bytes(s):
    return s[0].tobytes() + np.asarray(s[1]).tobytes() + np.asarray(s[2]).tobytes()


def check_lists(hs, dtype, dim, n, k, t, val, arg, idx, d2):
    """The per-target properties of the module docstring; returns (ambiguous slots, slots, worst |d2 - D2| / D2 in eps_T)."""
    T = npt(dtype)
    et = LD(eps_t(dtype))
    assert idx.shape == (n, k) and idx.dtype == np.uint32 and d2.shape == (n, k) and d2.dtype == T
    have = min(k, n - 1)
    assert (idx[:, have:] == NONE).all() and np.isposinf(d2[:, have:]).all(), "unused slots must hold (0xffffffff, +inf)"
    if have == 0:
        return 0, 0, 0.0
    used, ud2 = idx[:, :have].astype(np.int64), d2[:, :have]
    assert (used < n).all(), "a padding record or an empty slot in a list that should be full"
    assert (used != np.arange(n)[:, None]).all(), "the self pair"
    srt = np.sort(used, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), "an index twice in one list"
    assert np.isfinite(ud2).all()
    asc = (ud2[:, 1:] > ud2[:, :-1]) | ((ud2[:, 1:] == ud2[:, :-1]) & (used[:, 1:] > used[:, :-1]))
    assert asc.all(), "rows must ascend in (d2, idx)"
    D2 = gather_d2(hs.x, t, idx[t][:, :have])
    err = np.abs(ud2[t].astype(LD) - D2) / np.where(D2 > 0, D2, 1)
    assert (np.abs(ud2[t].astype(LD) - D2) <= 4 * et * D2).all(), float(err.max() / et)
    assert (D2 <= val[:, :have] * (1 + 8 * et)).all(), float((D2 / val[:, :have]).max())
    up = val[:, 1:have + 1] > val[:, :have] * (1 + 8 * et)  # clear of the next order statistic (k + 1 included)
    clear = up.copy()
    clear[:, 1:] &= up[:, :-1]  # ... and of the previous one
    assert (used[t][clear] == arg[:, :have][clear]).all(), "a neighbour with a clear gap on both sides is not the exact one"
    amb = int((~clear).sum())
    assert amb <= 1e-3 * clear.size, (amb, clear.size)
    return amb, int(clear.size), float(err.max() / et)


# ---- 1. lists, densities and the summary on random data -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_knn_density_and_summary_against_numpy_longdouble(nb, dtype, dim, n):
    """Every k of KS (and of KS_CAPACITY at n = 1000) on one device system: the list properties per target, rho of every body within
    32 eps_T of longdouble from the GPU's own idx, the summary within TOL of longdouble from the GPU's own rho; rho = 0 and a NaN summary
    for k = 1 and n <= k."""
    hs, t, val, arg = case(dtype, dim, n)
    et = eps_t(dtype)
    dev = nb.DeviceSystem.from_host(hs)
    try:
        for k in KS + (KS_CAPACITY if n == MID else []):
            idx, d2, rho, (xdc, rc, rhoc) = gpu_all(dev, k)
            amb, slots, derr = check_lists(hs, dtype, dim, n, k, t, val, arg, idx, d2)
            assert rho.shape == (n,) and rho.dtype == npt(dtype) and xdc.shape == (dim,) and xdc.dtype == npt(dtype)
            if k == 1 or n <= k:
                assert (rho == 0).all()
                assert np.isnan(xdc).all() and np.isnan(rc) and np.isnan(rhoc)
                print(f"knn dtype={dtype} dim={dim} n={n} k={k}: {amb} of {slots} slots without a clear gap, worst d2 error "
                      f"{derr:.3g} eps; rho = 0, summary NaN")
                continue
            ref = reference_rho(hs.m, hs.x, idx, k, dim)
            assert np.isfinite(rho).all() and (rho > 0).all()
            rerr = float((np.abs(rho.astype(LD) - ref) / ref).max())
            rx, rrc, rrhoc, scale = reference_summary(rho, hs.x)
            xerr = float((np.abs(xdc.astype(LD) - rx) / scale).max())
            cerr, derr2 = float(abs(LD(rc) - rrc) / rrc), float(abs(LD(rhoc) - rrhoc) / rrhoc)
            print(f"knn dtype={dtype} dim={dim} n={n} k={k}: {amb} of {slots} slots without a clear gap, worst d2 error {derr:.3g} eps, "
                  f"rho {rerr / et:.3g} eps (bound 32), x_dc {xerr:.3g} r_c {cerr:.3g} rho_c {derr2:.3g} (bound {TOL[dtype]:g})")
            assert rerr <= 32 * et, rerr / et
            assert xerr <= TOL[dtype] and cerr <= TOL[dtype] and derr2 <= TOL[dtype]
    finally:
        dev.close()


# ---- 2. exact ties ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(side):
    """Integer coordinates of the shuffled lattice with its 32 duplicates, masses in double, and per body the 16 smallest (d2, index)
    in integers — computed once per side, shared by both dtypes, never changed."""
    n0 = side ** 3
    rng = np.random.default_rng(4000 + n0)
    coords = np.stack(np.unravel_index(rng.permutation(n0), (side,) * 3), -1).astype(np.int64)
    coords = np.concatenate([coords, coords[rng.choice(n0, 32, replace=False)]])
    coords = coords[rng.permutation(len(coords))]
    n = len(coords)
    mass = rng.uniform(0.5, 1.5, n) / n
    want_j, want_d = np.empty((n, 16), np.int64), np.empty((n, 16), np.int64)
    for s in range(0, n, 512):
        d = coords[None, :, :] - coords[s:s + 512, None, :]
        D2 = (d * d).sum(-1)
        D2[np.arange(len(D2)), np.arange(s, s + len(D2))] = 1 << 40  # the self pair is out by index
        for r in range(len(D2)):
            o = np.lexsort((np.arange(n), D2[r]))[:16]
            want_j[s + r], want_d[s + r] = o, D2[r][o]
    for a in (coords, mass, want_j, want_d):
        a.setflags(write=False)
    return coords, mass, want_j, want_d


@pytest.mark.parametrize("side", [9, 17])
@pytest.mark.parametrize("dtype", [1, 0])
def test_exact_ties_on_a_shuffled_lattice_with_duplicates(nb, dtype, side):
    """Bodies on an integer lattice (9^3 = 729 and 17^3 = 4913 points, order shuffled by a fixed seed) plus 32 exact duplicates of
    existing points: every d2 is exact in float and double, so idx and d2 must equal NumPy's lexsort on (index, exact d2) in every slot,
    k = 6 and 16 — the insertion's strict `<` and the lexicographic wave and chunk merges."""
    coords, mass, want_j, want_d = lattice(side)
    n = len(coords)
    t = npt(dtype)
    hs = nb.HostSystem(dtype, 3, n)
    hs.m[:] = mass.astype(t)
    hs.x[:] = coords.astype(t)
    hs.dt, hs.c = 0.01, 1.0
    assert (want_d[:, 0] == 0).sum() == 64 and (want_d[:, 1:] == want_d[:, :-1]).any(1).all()  # duplicates, and ties in every row
    dev = nb.DeviceSystem.from_host(hs)
    try:
        for k in (6, 16):
            idx, d2 = dev.knn(k)
            assert np.array_equal(idx.astype(np.int64), want_j[:, :k]), k
            assert np.array_equal(d2, want_d[:, :k].astype(t)), k
    finally:
        dev.close()


# ---- 3. bitwise cross-checks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 257, 1000, 5889, 65537])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_column_0_is_the_nearest_neighbour_and_lists_do_not_depend_on_the_capacity(nb, dtype, dim, n):
    hs, *_ = case(dtype, dim, n)
    dev = nb.DeviceSystem.from_host(hs)
    try:
        _, nn, nnd2 = dev.neighbours(0.05)
        got = {k: dev.knn(k) for k in (1, 4, 6, 8, 16)}
    finally:
        dev.close()
    for k, (idx, d2) in got.items():
        assert np.array_equal(idx[:, 0], nn) and d2[:, 0].tobytes() == nnd2.tobytes(), k
    for small, big in ((4, 16), (6, 8), (1, 4), (8, 16)):
        assert np.array_equal(got[small][0], got[big][0][:, :small]), (small, big)
        assert got[small][1].tobytes() == np.ascontiguousarray(got[big][1][:, :small]).tobytes(), (small, big)


@pytest.mark.parametrize("n,k", [(1000, 6), (5889, 16), (65537, 6)])
@pytest.mark.parametrize("dtype", [1, 0])
def test_bitwise_repeatable_eager_replayed_and_new_handle(nb, dtype, n, k):
    hs = random_system(nb, dtype, 3, n, seed=80 + n)
    dev = nb.DeviceSystem.from_host(hs)

    def outputs():
        h = dev.knn_handle(k)
        return tuple(h.read(w, dev.stream).tobytes() for w in range(3)) + (summary_bytes(h.density_centre(dev.stream)),)

    dev.knn_compute(k)
    first = outputs()
    dev.knn_compute(k)
    assert outputs() == first
    # a handle destroyed and made again
    dev._knn.pop(k).close()
    dev.knn_compute(k)
    assert outputs() == first
    # recorded and replayed; the handle's arrays are overwritten in between so that the replay has to produce them
    g = nb.StepGraph(dev, lambda: dev.knn_compute(k))
    other = random_system(nb, dtype, 3, n, seed=81 + n)
    dev2 = nb.DeviceSystem.from_host(other)
    dev.knn_handle(k).compute(dev2.state(), dev2.stream)
    dev2.sync()
    assert all(a != b for a, b in zip(outputs(), first))
    g.launch()
    assert outputs() == first
    g.launch()
    assert outputs() == first
    g.close()
    dev2.close()
    dev.close()


# ---- 4. coincident bodies ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_a_duplicated_body_at_k_2_gives_infinite_density_and_a_nan_summary(nb, dtype, dim):
    n = 1000
    hs = random_system(nb, dtype, dim, n, seed=55)
    hs.x[900] = hs.x[5]  # in different tiles
    dev = nb.DeviceSystem.from_host(hs)
    try:
        # k = 2: the k-th neighbour is the second, so a pair alone keeps d2_k > 0 ...
        idx, d2, rho, (xdc, rc, rhoc) = gpu_all(dev, 2)
        assert idx[5, 0] == 900 and idx[900, 0] == 5 and d2[5, 0] == 0 and d2[900, 0] == 0
        assert np.isfinite(rho).all() and np.isfinite(xdc).all()
        # ... and a triple makes it 0 for its three bodies: rho = +inf there, finite elsewhere, and every summary output NaN
        hs.x[300] = hs.x[5]
        dev.upload(hs)
        idx, d2, rho, (xdc, rc, rhoc) = gpu_all(dev, 2)
        same = [5, 300, 900]
        assert [list(idx[i]) for i in same] == [[300, 900], [5, 900], [5, 300]] and (d2[same] == 0).all()
        assert np.isposinf(rho[same]).all()
        rest = np.delete(np.arange(n), same)
        assert np.isfinite(rho[rest]).all() and (rho[rest] > 0).all()
        assert np.isnan(xdc).all() and np.isnan(rc) and np.isnan(rhoc)
    finally:
        dev.close()


def test_a_duplicated_pair_at_k_2_in_a_system_of_pairs(nb):
    """Two bodies on one point at k = 2: the k-th distance is the one to the SECOND neighbour, a third body, so d2_k > 0 and the density
    is finite — rho_i = m_j / (V d2_k^(3/2)) with the duplicate's mass, by the header's definition.  (d2_k = 0 takes k coincident
    neighbours: the triple of the test above.)"""
    n = 300
    hs = random_system(nb, 1, 3, n, seed=56)
    hs.x[200] = hs.x[7]
    dev = nb.DeviceSystem.from_host(hs)
    try:
        idx, d2, rho, _ = gpu_all(dev, 2)
    finally:
        dev.close()
    assert idx[7, 0] == 200 and idx[200, 0] == 7 and idx[7, 1] == idx[200, 1] and d2[7, 1] == d2[200, 1]
    for i, j in ((7, 200), (200, 7)):
        want = LD(hs.m[j]) / (LD(4) / 3 * LD(np.pi) * LD(d2[i, 1]) ** LD(1.5))
        assert abs(LD(rho[i]) - want) <= 1e-14 * want


# ---- 5. a physical sanity case ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
def test_density_centre_finds_the_cluster_where_the_centre_of_mass_does_not(nb, dtype):
    """A normal blob of 4096 bodies shifted by (3, -2, 1) and 64 far outliers at distance 50 on one side: density_centre(6) lies within
    r_c of the shift; the mass-weighted mean of x is farther from the shift than x_dc is."""
    rng = np.random.default_rng(2024)
    t = npt(dtype)
    shift = np.array([3.0, -2.0, 1.0])
    blob = rng.normal(0, 1, (4096, 3))
    out = rng.normal(0, 1, (64, 3))
    out[:, 0] = np.abs(out[:, 0])
    out = 50.0 * out / np.linalg.norm(out, axis=1)[:, None]
    x = np.concatenate([blob, out]) + shift
    x = x[rng.permutation(len(x))]
    n = len(x)
    hs = nb.HostSystem(dtype, 3, n)
    hs.m[:] = t(1.0 / n)
    hs.x[:] = x.astype(t)
    hs.dt, hs.c = 0.01, 1.0
    dev = nb.DeviceSystem.from_host(hs)
    try:
        xdc, rc, rhoc = dev.density_centre()
        rho = dev.local_density()
    finally:
        dev.close()
    com = (hs.m[:, None].astype(np.float64) * hs.x.astype(np.float64)).sum(0) / hs.m.astype(np.float64).sum()
    off_dc, off_com = np.linalg.norm(xdc.astype(np.float64) - shift), np.linalg.norm(com - shift)
    print(f"sanity dtype={dtype}: |x_dc - shift| = {off_dc:.3g}, r_c = {float(rc):.3g}, rho_c = {float(rhoc):.3g}, |com - shift| = {off_com:.3g}")
    assert rho.shape == (n,) and (rho > 0).all()
    assert 0 < rc < 2 and off_dc < rc
    assert off_com > off_dc


# ---- 6. call sequence -----------------------------------------------------------------------------------------------------------------------
def test_call_sequence_errors(nb):
    L = nb.lib()
    hs = random_system(nb, 1, 3, 300, seed=1)
    dev = nb.DeviceSystem.from_host(hs)
    st = dev.state()
    stream = ctypes.c_void_p(dev.stream)
    err = lambda: L.nbody_last_error()

    def rc_of(call):
        try:
            call()
        except nb.NbodyError as e:
            return int(re.match(r"nbody backend error (\d+)", str(e)).group(1)), str(e)
        return 0, ""

    def outputs(h):
        return tuple(h.read(w, dev.stream).tobytes() for w in range(3)) + (summary_bytes(h.density_centre(dev.stream)),)

    h = nb.Knn(1, 3, 300, 6, dev.device)
    assert rc_of(lambda: h.read(0, dev.stream))[0] == 3  # before the first compute
    assert rc_of(lambda: h.density_centre(dev.stream))[0] == 3
    # a handle made for another n, dtype or dim
    for other in (nb.Knn(1, 3, 301, 6, dev.device), nb.Knn(0, 3, 300, 6, dev.device), nb.Knn(1, 2, 300, 6, dev.device)):
        rc, msg = rc_of(lambda: other.compute(st, dev.stream))
        assert rc == 1 and "was created for" in msg
        other.close()
    # v, a, ao are not read
    bare = nb.nbody_state()
    ctypes.memmove(ctypes.byref(bare), ctypes.byref(st), ctypes.sizeof(st))
    bare.v = bare.a = bare.ao = None
    h.compute(bare, dev.stream)
    want = outputs(h)
    h.compute(st, dev.stream)
    assert outputs(h) == want
    # density_centre: any output may be NULL
    one = ctypes.c_double()
    assert L.nbody_knn_density_centre(h.h, None, None, None, stream) == 0
    assert L.nbody_knn_density_centre(h.h, None, ctypes.byref(one), None, stream) == 0
    assert one.value == float(h.density_centre(dev.stream)[1])
    # read: bytes must match
    buf = np.zeros(300 * 6 + 1)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.nbody_knn_read(h.h, 0, p, 300 * 6 * 8, stream) == 1 and b"bytes" in err()
    assert L.nbody_knn_read(h.h, 0, p, 300 * 6 * 4, stream) == 0
    assert L.nbody_knn_read(h.h, 1, p, 300 * 8, stream) == 1 and b"bytes" in err()
    assert L.nbody_knn_read(h.h, 1, p, 300 * 6 * 8, stream) == 0
    assert L.nbody_knn_read(h.h, 2, p, 300 * 6 * 8, stream) == 1 and b"bytes" in err()
    assert L.nbody_knn_read(h.h, 2, p, 300 * 8, stream) == 0
    assert L.nbody_knn_read(h.h, 3, p, 300 * 8, stream) == 1 and b"what" in err()
    # under capture: create, read and density_centre are refused, and the capture goes on to record a compute that replays
    assert L.nbody_graph_begin(stream) == 0
    try:
        made = ctypes.c_void_p()
        rc_create = L.nbody_knn_create(ctypes.byref(made), 1, 3, 300, 6)
        rc_read = L.nbody_knn_read(h.h, 2, p, 300 * 8, stream)
        rc_centre = L.nbody_knn_density_centre(h.h, None, None, None, stream)
        h.compute(st, dev.stream)
    finally:
        g = ctypes.c_void_p()
        rc_end = L.nbody_graph_end(stream, ctypes.byref(g))
    assert (rc_create, rc_read, rc_centre, rc_end) == (3, 3, 3, 0) and not made.value
    assert L.nbody_graph_launch(g, stream) == 0 and L.nbody_graph_launch(g, stream) == 0
    dev.sync()  # the stream is out of capture and works
    assert outputs(h) == want
    L.nbody_graph_destroy(g)
    # the state is untouched
    out = dev.download()
    assert np.array_equal(out.x, hs.x) and np.array_equal(out.m, hs.m) and np.array_equal(out.v, hs.v)
    h2 = nb.Knn(1, 3, 300, 16, dev.device)  # create works again after the capture
    h2.close()
    h.close()
    # the system's handles are cached per k and closed with it
    dev.knn(6)
    dev.knn(16)
    assert sorted(dev._knn) == [6, 16] and dev.knn_handle(6) is dev.knn_handle(6)
    dev.close()
    assert dev._knn == {}


# ---- 7. CLI -------------------------------------------------------------------------------------------------------------------------------------
def cli(dim, args, cwd):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", f"nbody_hip_d{dim}")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


CLI_CASES = [("double", ["--algorithm", "all-pairs"]), ("float", ["--algorithm", "all-pairs"]), ("double", []), ("float", [])]


@pytest.mark.parametrize("prec,extra", CLI_CASES, ids=[p + "-" + ("_".join(a.strip("-") for a in e) or "default_octree") for p, e in CLI_CASES])
def test_cli_save_density(nb, prec, extra):
    """-n 1000 -s 4 --save-density 6 --save pos, no --softening: density.bin has the stated header and size, its last frame equals
    DeviceSystem's result on the saved last positions bit for bit, and positions.bin is byte-identical to a run without the flag."""
    dtype = 1 if prec == "double" else 0
    n, dim, k, tsz = 1000, 3, 6, 4 if dtype == 0 else 8
    base = ["-n", n, "-s", 4, "--precision", prec, "--save", "pos"] + extra
    with tempfile.TemporaryDirectory() as d, tempfile.TemporaryDirectory() as d0:
        r = cli(dim, base + ["--save-density", k], d)
        assert r.returncode == 0, r.stderr
        r0 = cli(dim, base, d0)
        assert r0.returncode == 0, r0.stderr
        praw = open(os.path.join(d, "positions.bin"), "rb").read()
        assert praw == open(os.path.join(d0, "positions.bin"), "rb").read()
        assert not os.path.exists(os.path.join(d0, "density.bin"))
        raw = open(os.path.join(d, "density.bin"), "rb").read()
    assert struct.unpack("<5I", raw[:20]) == (n, 4, tsz, dim, k)
    frame = (n + dim + 2) * tsz
    nframes = (len(praw) - 16) // (n * dim * tsz)
    assert nframes >= 1 and len(raw) == 20 + nframes * frame
    last = np.frombuffer(raw, npt(dtype), n + dim + 2, len(raw) - frame)
    hs = nb.build_model(dtype, dim, "uniform", n)
    hs.x[:] = np.frombuffer(praw, npt(dtype), n * dim, len(praw) - n * dim * tsz).reshape(n, dim)
    dev = nb.DeviceSystem.from_host(hs)
    try:
        rho = dev.local_density(k)
        xdc, rc, rhoc = dev.density_centre(k)
    finally:
        dev.close()
    assert last[:n].tobytes() == rho.tobytes()
    assert last[n:].tobytes() == summary_bytes((xdc, rc, rhoc))
    assert np.isfinite(last).all() and (last[:n] > 0).all()
