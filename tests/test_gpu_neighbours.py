"""GPU: all-pairs per-body potentials, nearest neighbours and the closest pair (nbody_neighbours_*) against NumPy longdouble written here
from the T-typed inputs (the reference project has no counterpart, so there are no fixtures).

Launch-shape boundaries of the sweep (hermite_plan_for(sz, 2) of csrc/hermite_tile.hpp, the sixth order's plan), each with a size on
either side: one LDS tile of 256 records and one chunk | two tiles, two chunks (256 / 257); one tile per chunk | several (5888 / 5889);
one target per lane | two (65535 / 65536, and 65537 for the ragged last block); the plan never goes back to one chunk.  Beside them
the wave's slice of 64 records (63 / 64 / 65), a last tile that is nearly all padding (257, 513, 4097, 5889, 65537) and the sizes
1, 2, 3.  Sizes above 4097 compare a fixed subset of targets (bodies 0 and n - 1 included) against all sources.

Bounds.  Potential: the project's bound for a summed quantity against NumPy, TOL = {f64: 1e-12, f32: 2e-5} (tests/test_gpu_softening.py,
tests/test_gpu_hermite.py), per body — every term of S_i is positive.  Neighbours, with D2 exact (longdouble) and eps_T the machine
epsilon of T: D2(i, nn_i) <= min_j D2(i, j) (1 + 8 eps_T) and |nnd2_i - D2(i, nn_i)| <= 4 eps_T D2(i, nn_i): each difference rounds once,
the D squares and adds round once each, all terms are positive, so a computed d2 is within (D + 2) u = 2.5 eps_T of the exact one and two
compared values within 5 eps_T.

Measured on an MI355X (worst per-body |phi - ref| / |ref| over the sizes): 4.67e-16 in double, 2.49e-7 in float; 0.5 sum m_i phi_i against
calc_energies(softening) within 1.98e-16 and 1.28e-7; the octree's softened potential at theta = 0 within 4.91e-16 and 2.86e-7 per body;
every target of every random system had a clear runner-up and the exact neighbour.  The figures per size, as the tests print them
(-s), are in profiles/neighbours/gpu_test_suite.txt."""
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
EPS = 0.05

SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 513, 1000, 4097, 5888, 5889, 20000, 65535, 65536, 65537]


def npt(dtype):
    return np.float32 if dtype == 0 else np.float64


def eps_t(dtype):
    return float(np.finfo(npt(dtype)).eps)


def e2_of(dtype, eps):
    t = npt(dtype)
    return t(t(eps) * t(eps))


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


def reference(m, x, c, e2, targets, nn):
    """For the targets t, in longdouble from the T-typed inputs: phi_t = -c sum_{j != t} m_j / sqrt(D2(t, j) + e2); the smallest
    D2(t, j), j != t, its lowest index, the second smallest; and D2(t, nn_t) for the given nn (inf where nn is 0xffffffff)."""
    m, x = np.asarray(m, LD), np.asarray(x, LD)
    n = len(m)
    phi, dmin, amin, dsec, dnn = (np.zeros(len(targets), LD), np.full(len(targets), np.inf, LD), np.full(len(targets), NONE, np.int64),
                                  np.full(len(targets), np.inf, LD), np.full(len(targets), np.inf, LD))
    step = max(1, min(256, (1 << 21) // max(n, 1)))
    for s in range(0, len(targets), step):
        t = targets[s:s + step]
        rows = np.arange(len(t))
        d = x[None, :, :] - x[t][:, None, :]
        D2 = (d * d).sum(-1)
        w = m[None, :] / np.sqrt(D2 + LD(e2))
        w[rows, t] = 0
        phi[s:s + step] = -LD(c) * w.sum(1)
        ok = nn[s:s + step] != NONE
        dnn[s:s + step][ok] = D2[rows[ok], nn[s:s + step][ok].astype(np.int64)]
        D2[rows, t] = np.inf
        if n > 1:
            amin[s:s + step] = D2.argmin(1)
            dmin[s:s + step] = D2[rows, amin[s:s + step]]
            D2[rows, amin[s:s + step]] = np.inf
            dsec[s:s + step] = D2.min(1)
    return phi, dmin, amin, dsec, dnn


def gpu_outputs(nb, hs, eps=EPS):
    dev = nb.DeviceSystem.from_host(hs)
    phi, nn, nnd2 = dev.neighbours(eps)
    cp = dev.neighbours_handle.closest_pair(dev.stream)
    dev.close()
    return phi, nn, nnd2, cp


@functools.lru_cache(maxsize=None)
def case(dtype, dim, n):
    """One random system per (dtype, dim, n): the GPU's outputs and the longdouble reference of its targets, computed once and shared."""
    from conftest import load_package
    nb = load_package()
    hs = random_system(nb, dtype, dim, n, seed=100 + n)
    phi, nn, nnd2, cp = gpu_outputs(nb, hs)
    t = targets_of(n)
    ref = reference(hs.m, hs.x, hs.c, e2_of(dtype, EPS), t, nn[t])
    return hs, (phi, nn, nnd2, cp), t, ref


# ---- 1. potential -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_potential_against_numpy_longdouble(nb, dtype, dim, n):
    """Per body |phi - ref| <= TOL |ref|.  Measured on an MI355X, worst over all sizes and bodies: 4.67e-16 in double (2D, N = 4097; at most
    3.3e-16 from 65 535 bodies on) and 2.49e-7 in float (3D, N = 4097; at most 1.8e-7 from 65 535 on); per size in
    profiles/neighbours/gpu_test_suite.txt."""
    hs, (phi, nn, nnd2, cp), t, (rphi, *_) = case(dtype, dim, n)
    assert phi.shape == (n,) and phi.dtype == npt(dtype) and np.isfinite(phi).all()
    if n == 1:
        assert phi[0] == 0
        return
    err = np.abs(phi[t].astype(LD) - rphi) / np.abs(rphi)
    print(f"potential dtype={dtype} dim={dim} n={n}: worst per-body error {float(err.max()):.3g} (bound {TOL[dtype]:g})")
    assert (phi < 0).all()
    assert err.max() <= TOL[dtype], (n, float(err.max()))


# ---- 2. energy cross-checks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 4097, 20000])
@pytest.mark.parametrize("dtype", [1, 0])
def test_energy_from_phi_equals_calc_energies(nb, dtype, n):
    hs, (phi, *_), _, _ = case(dtype, 3, n)
    # PE = -c/2 sum_i m_i S_i = 1/2 sum_i m_i phi_i (phi_i = -c S_i carries the sign), accumulated in float64
    pe_phi = 0.5 * float((hs.m.astype(np.float64) * phi.astype(np.float64)).sum())
    dev = nb.DeviceSystem.from_host(hs)
    _, pe = dev.calc_energies(softening=EPS)
    dev.close()
    print(f"energy dtype={dtype} n={n}: from phi {pe_phi:.17g}, calc_energies {float(pe):.17g}, rel {abs(pe_phi - float(pe)) / abs(float(pe)):.3g}")
    assert abs(pe_phi - float(pe)) <= TOL[dtype] * abs(float(pe))


@pytest.mark.parametrize("dtype", [1, 0])
def test_octree_softened_potential_at_theta_0_agrees_per_body(nb, dtype):
    hs, (phi, *_), _, _ = case(dtype, 3, 1000)
    dev = nb.DeviceSystem.from_host(hs)
    tree_phi = dev.octree_potential(0.0, softening=EPS)
    dev.close()
    err = np.abs(tree_phi.astype(np.float64) - phi.astype(np.float64)) / np.abs(phi.astype(np.float64))
    print(f"octree theta=0 dtype={dtype}: worst per-body difference {err.max():.3g}")
    assert err.max() <= TOL[dtype]


# ---- 3. neighbours, random data -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_nearest_neighbour_against_numpy_longdouble(nb, dtype, dim, n):
    hs, (phi, nn, nnd2, cp), t, (_, dmin, amin, dsec, dnn) = case(dtype, dim, n)
    assert nn.shape == (n,) and nn.dtype == np.uint32 and nnd2.shape == (n,) and nnd2.dtype == npt(dtype)
    if n == 1:
        assert nn[0] == NONE and np.isposinf(nnd2[0]) and phi[0] == 0
        assert cp[0] == NONE and cp[1] == NONE and np.isposinf(cp[2])
        return
    assert (nn < n).all(), "a body was skipped or took a padding record"  # no body skipped, no padding
    assert (nn != np.arange(n)).all()
    et = LD(eps_t(dtype))
    assert (dnn <= dmin * (1 + 8 * et)).all(), float((dnn / dmin).max())
    assert (np.abs(nnd2[t].astype(LD) - dnn) <= 4 * et * dnn).all()
    clear = dsec > dmin * (1 + 10 * et)  # where the runner-up is clearly farther, the index is the exact one
    assert (nn[t][clear] == amin[clear]).all()
    print(f"neighbours dtype={dtype} dim={dim} n={n}: {int(clear.sum())} of {len(t)} targets with a clear runner-up, all exact")


# ---- 4. exact ties ----------------------------------------------------------------------------------------------------------------------
LATTICES = [(2, 16), (3, 7), (3, 17), (3, 41)]  # 41^3 = 68 921 bodies: above the two-targets-per-lane size


@pytest.mark.parametrize("dim,side", LATTICES)
@pytest.mark.parametrize("dtype", [1, 0])
def test_exact_ties_on_a_shuffled_lattice(nb, dtype, dim, side):
    """Integer lattice of spacing 1, bodies in a fixed shuffled order: every d2 is an exact integer, every body has 2 to 6 neighbours at
    d2 == 1 scattered over waves, tiles and chunks; nn must be the LOWEST index among them (from the grid, in integers)."""
    n = side ** dim
    rng = np.random.default_rng(4000 + n)
    order = rng.permutation(n)  # body i sits at lattice site order[i]
    index_of = np.empty(n, np.int64)
    index_of[order] = np.arange(n)
    coords = np.stack(np.unravel_index(order, (side,) * dim), -1)
    want = np.full(n, n, np.int64)
    grid = index_of.reshape((side,) * dim)
    for ax in range(dim):
        for sh in (-1, 1):
            c2 = coords.copy()
            c2[:, ax] += sh
            ok = (c2[:, ax] >= 0) & (c2[:, ax] < side)
            cand = np.full(n, n, np.int64)
            cand[ok] = grid[tuple(c2[ok].T)]
            want = np.minimum(want, cand)
    t = npt(dtype)
    hs = nb.HostSystem(dtype, dim, n)
    hs.m[:] = rng.uniform(0.5, 1.5, n).astype(t) / n
    hs.x[:] = coords.astype(t)
    hs.dt, hs.c = 0.01, 1.0
    phi, nn, nnd2, cp = gpu_outputs(nb, hs, eps=0.25)
    assert np.array_equal(nn.astype(np.int64), want)
    assert (nnd2 == t(1.0)).all()
    assert cp[0] == 0 and cp[1] == want[0] and cp[2] == t(1.0)
    assert np.isfinite(phi).all() and (phi < 0).all()


# ---- 5. coincident bodies and padding -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_coincident_bodies(nb, dtype, dim):
    """Three bodies at one point, at indices in different tiles: each reports the lowest-index other one at nnd2 == 0 exactly, and its phi
    holds m_j / eps for both others."""
    n, same = 1000, [5, 300, 900]
    hs = random_system(nb, dtype, dim, n, seed=55)
    hs.x[same] = hs.x[same[0]]
    phi, nn, nnd2, cp = gpu_outputs(nb, hs)
    assert list(nn[same]) == [300, 5, 5] and (nnd2[same] == 0).all()
    assert cp[0] == 5 and cp[1] == 300 and cp[2] == 0
    t = np.arange(n)
    rphi, *_ = reference(hs.m, hs.x, hs.c, e2_of(dtype, EPS), t, nn)
    err = np.abs(phi.astype(LD) - rphi) / np.abs(rphi)
    assert err.max() <= TOL[dtype], float(err.max())
    m = hs.m.astype(LD)
    assert abs(rphi[5]) > (m[300] + m[900]) / LD(EPS) * LD(0.99)  # the coincident terms are in the reference


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_one_and_two_bodies_and_a_padded_tile(nb, dtype, dim):
    t = npt(dtype)
    hs = random_system(nb, dtype, dim, 1, seed=3)
    phi, nn, nnd2, cp = gpu_outputs(nb, hs)
    assert phi[0] == 0 and nn[0] == NONE and np.isposinf(nnd2[0])
    assert cp[0] == NONE and cp[1] == NONE and np.isposinf(cp[2])
    hs = random_system(nb, dtype, dim, 2, seed=4, c=2.0)
    phi, nn, nnd2, cp = gpu_outputs(nb, hs)
    d = hs.x[1].astype(LD) - hs.x[0].astype(LD)
    D2 = (d * d).sum()
    assert list(nn) == [1, 0] and nnd2[0] == nnd2[1]  # d2 is bitwise symmetric
    assert abs(LD(nnd2[0]) - D2) <= 4 * LD(eps_t(dtype)) * D2
    assert cp[0] == 0 and cp[1] == 1 and cp[2] == nnd2[0]
    for i in (0, 1):
        ref = -LD(2.0) * LD(hs.m[1 - i]) / np.sqrt(D2 + LD(e2_of(dtype, EPS)))
        assert abs(LD(phi[i]) - ref) <= TOL[dtype] * abs(ref)
    # n = 257: the second tile holds one body and 255 padding records at the origin; put the bodies far from it
    hs = random_system(nb, dtype, dim, 257, seed=5)
    hs.x[:] += t(40.0)
    phi, nn, nnd2, cp = gpu_outputs(nb, hs)
    assert (nn < 257).all() and (nnd2 < 100).all() and cp[1] < 257


# ---- 6. invariances -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 5889])
@pytest.mark.parametrize("dtype", [1, 0])
def test_nn_does_not_depend_on_eps(nb, dtype, n):
    hs = random_system(nb, dtype, 3, n, seed=60 + n)
    a, b = gpu_outputs(nb, hs, eps=0.05), gpu_outputs(nb, hs, eps=0.5)
    assert np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()
    assert a[3] == b[3]
    assert not np.array_equal(a[0], b[0])


@pytest.mark.parametrize("n", [1000, 5889])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_nn_under_a_permutation_of_the_bodies(nb, dtype, dim, n):
    """Body i of the first system is body p(i) of the second: nn'[p(i)] == p(nn[i]) and nnd2 has the same bits (d2 does not depend on
    where a body stands).  Needs data without ties, which the test asserts of its seed."""
    hs = random_system(nb, dtype, dim, n, seed=70 + n)
    p = np.random.default_rng(71 + n).permutation(n)
    hp = nb.HostSystem(dtype, dim, n)
    hp.m[p], hp.x[p] = hs.m, hs.x
    hp.dt, hp.c = hs.dt, hs.c
    _, nn, nnd2, cp = gpu_outputs(nb, hs)
    _, nn2, nnd22, cp2 = gpu_outputs(nb, hp)
    # no ties: every body's runner-up is farther by 1e-5 relatively (100 eps_T in float, far more in double), in float64 arithmetic
    # whose own error is 1e-15 — all bodies are needed here, and longdouble would take seconds at 5889
    x = hs.x.astype(np.float64)
    for s in range(0, n, 512):
        d = x[None, :, :] - x[s:s + 512, None, :]
        D2 = (d * d).sum(-1)
        D2[np.arange(len(D2)), np.arange(s, s + len(D2))] = np.inf
        two = np.partition(D2, 1, axis=1)[:, :2]
        assert (two[:, 1] > two[:, 0] * (1 + 1e-5)).all(), "this seed has a near tie: choose another"
    assert np.array_equal(nn2[p], p[nn])
    assert nnd22[p].tobytes() == nnd2.tobytes()
    assert cp2[2] == cp[2] and {int(cp2[0]), int(cp2[1])} == {int(p[cp[0]]), int(p[cp[1]])}


# ---- 7. determinism, call sequence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 5889, 65537])
@pytest.mark.parametrize("dtype", [1, 0])
def test_bitwise_repeatable_eager_replayed_and_new_handle(nb, dtype, n):
    hs = random_system(nb, dtype, 3, n, seed=80 + n)
    dev = nb.DeviceSystem.from_host(hs)

    def outputs():
        h = dev.neighbours_handle
        return tuple(h.read(k, dev.stream).tobytes() for k in range(3)) + (h.closest_pair(dev.stream),)

    dev.neighbours_compute(EPS)
    first = outputs()
    dev.neighbours_compute(EPS)
    assert outputs() == first
    # a handle destroyed and made again
    dev._neighbours.close()
    dev._neighbours = None
    dev.neighbours_compute(EPS)
    assert outputs() == first
    # recorded and replayed; the handle's arrays are overwritten in between so that the replay has to produce them
    g = nb.StepGraph(dev, lambda: dev.neighbours_compute(EPS))
    other = random_system(nb, dtype, 3, n, seed=81 + n)
    dev2 = nb.DeviceSystem.from_host(other)
    dev.neighbours_handle.compute(dev2.state(), 0.5, dev2.stream)
    dev2.sync()
    assert outputs() != first
    g.launch()
    assert outputs() == first
    g.launch()
    assert outputs() == first
    g.close()
    dev2.close()
    dev.close()


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

    h = nb.Neighbours(1, 3, 300, dev.device)
    assert rc_of(lambda: h.read(0, dev.stream))[0] == 3  # before the first compute
    assert rc_of(lambda: h.closest_pair(dev.stream))[0] == 3
    # a handle made for another n, dtype or dim: after eps, before the device
    for other in (nb.Neighbours(1, 3, 301, dev.device), nb.Neighbours(0, 3, 300, dev.device), nb.Neighbours(1, 2, 300, dev.device)):
        rc, msg = rc_of(lambda: other.compute(st, 0.05, dev.stream))
        assert rc == 1 and "was created for" in msg
        rc, msg = rc_of(lambda: other.compute(st, 0.0, dev.stream))
        assert rc == 1 and "softening" in msg  # eps comes first
        other.close()
    # v, a, ao are not read
    bare = nb.nbody_state()
    ctypes.memmove(ctypes.byref(bare), ctypes.byref(st), ctypes.sizeof(st))
    bare.v = bare.a = bare.ao = None
    h.compute(bare, 0.05, dev.stream)
    want = tuple(h.read(k, dev.stream).tobytes() for k in range(3)) + (h.closest_pair(dev.stream),)
    h.compute(st, 0.05, dev.stream)
    assert tuple(h.read(k, dev.stream).tobytes() for k in range(3)) + (h.closest_pair(dev.stream),) == want
    # closest_pair: any output may be NULL
    i = ctypes.c_uint32()
    assert L.nbody_neighbours_closest_pair(h.h, None, None, None, stream) == 0
    assert L.nbody_neighbours_closest_pair(h.h, ctypes.byref(i), None, None, stream) == 0 and i.value == want[3][0]
    # read: bytes must match
    buf = np.zeros(301)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.nbody_neighbours_read(h.h, 0, p, 301 * 8, stream) == 1 and b"bytes" in err()
    assert L.nbody_neighbours_read(h.h, 1, p, 300 * 8, stream) == 1 and b"bytes" in err()
    assert L.nbody_neighbours_read(h.h, 1, p, 300 * 4, stream) == 0
    assert L.nbody_neighbours_read(h.h, 3, p, 300 * 8, stream) == 1 and b"what" in err()
    # under capture: create, read and closest_pair are refused, and the capture goes on to record a compute that replays
    assert L.nbody_graph_begin(stream) == 0
    try:
        made = ctypes.c_void_p()
        rc_create = L.nbody_neighbours_create(ctypes.byref(made), 1, 3, 300)
        rc_read = L.nbody_neighbours_read(h.h, 0, p, 300 * 8, stream)
        rc_pair = L.nbody_neighbours_closest_pair(h.h, None, None, None, stream)
        h.compute(st, 0.05, dev.stream)
    finally:
        g = ctypes.c_void_p()
        rc_end = L.nbody_graph_end(stream, ctypes.byref(g))
    assert (rc_create, rc_read, rc_pair, rc_end) == (3, 3, 3, 0) and not made.value
    assert L.nbody_graph_launch(g, stream) == 0 and L.nbody_graph_launch(g, stream) == 0
    dev.sync()  # the stream is out of capture and works
    assert tuple(h.read(k, dev.stream).tobytes() for k in range(3)) + (h.closest_pair(dev.stream),) == want
    L.nbody_graph_destroy(g)
    # the state is untouched
    out = dev.download()
    assert np.array_equal(out.x, hs.x) and np.array_equal(out.m, hs.m) and np.array_equal(out.v, hs.v)
    h2 = nb.Neighbours(1, 3, 300, dev.device)  # create works again after the capture
    h2.close()
    h.close()
    dev.close()


# ---- 8. closest pair ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 257, 1000, 4097])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_closest_pair_is_the_argmin(nb, dtype, dim, n):
    hs, (phi, nn, nnd2, cp), t, (_, dmin, amin, dsec, dnn) = case(dtype, dim, n)
    assert len(t) == n
    i = int(np.argmin(dmin))
    j = int(amin[i])
    i, j = min(i, j), max(i, j)
    # the runner-up among the PAIRS: the smallest D2 of any pair other than (i, j)
    rest = dmin.copy()
    rest[[i, j]] = np.minimum(dsec[i], dsec[j])
    gap = rest.min() / dmin[i] - 1
    assert gap > 10 * eps_t(dtype), "this seed's two closest pairs nearly tie: choose another"
    assert (cp[0], cp[1]) == (i, j), (cp, i, j)
    assert cp[2] == nnd2[i] == nnd2[j]
    assert cp[2] == nnd2.min()


# ---- 9. CLI -------------------------------------------------------------------------------------------------------------------------------------
def cli(dim, args, cwd):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", f"nbody_hip_d{dim}")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def read_positions(path):
    raw = open(path, "rb").read()
    n, steps, tsz, dim = struct.unpack("<4I", raw[:16])
    data = np.frombuffer(raw[16:], dtype=np.float32 if tsz == 4 else np.float64)
    assert data.size % (n * dim) == 0
    return (n, steps, tsz, dim), data.reshape(-1, n, dim)


def read_neighbours(path):
    raw = open(path, "rb").read()
    n, steps, tsz, dim = struct.unpack("<4I", raw[:16])
    t = np.float32 if tsz == 4 else np.float64
    frame = n * (2 * tsz + 4)
    assert (len(raw) - 16) % frame == 0
    out = []
    for k in range((len(raw) - 16) // frame):
        o = 16 + k * frame
        out.append((np.frombuffer(raw, t, n, o), np.frombuffer(raw, np.uint32, n, o + n * tsz), np.frombuffer(raw, t, n, o + n * (tsz + 4))))
    return (n, steps, tsz, dim), out


CLI_CASES = [
    ("double", 3, ["--algorithm", "all-pairs"]),
    ("float", 2, ["--algorithm", "all-pairs"]),
    ("double", 3, ["--algorithm", "all-pairs", "--csv-detailed"]),  # a frame per step
    ("double", 3, ["--algorithm", "all-pairs", "--integrator", "hermite", "--hermite-eta", "0.02", "--csv-detailed"]),
    ("double", 3, ["--algorithm", "all-pairs", "--integrator", "hermite", "--hermite-eta", "0.02"]),
    ("double", 3, ["--algorithm", "octree", "--csv-detailed"]),
    ("double", 3, ["--algorithm", "octree"]),
]


@pytest.mark.parametrize("prec,dim,extra", CLI_CASES, ids=[f"{p}-{d}D-" + "_".join(a.strip("-") for a in e) for p, d, e in CLI_CASES])
def test_cli_save_neighbours(nb, prec, dim, extra):
    """Every frame of neighbours.bin holds phi within TOL and neighbours within the bounds of test 3 of the same frame of positions.bin
    (masses from build_model); without the flag the same command writes the same positions.bin byte for byte and no neighbours.bin."""
    dtype = 1 if prec == "double" else 0
    base = ["-n", 300, "-s", 12, "--precision", prec, "--softening", 0.05, "--save", "pos"] + extra
    with tempfile.TemporaryDirectory() as d, tempfile.TemporaryDirectory() as d0:
        r = cli(dim, base + ["--save-neighbours"], d)
        assert r.returncode == 0, r.stderr
        r0 = cli(dim, base, d0)
        assert r0.returncode == 0, r0.stderr
        assert open(os.path.join(d, "positions.bin"), "rb").read() == open(os.path.join(d0, "positions.bin"), "rb").read()
        assert not os.path.exists(os.path.join(d0, "neighbours.bin"))
        head, pos = read_positions(os.path.join(d, "positions.bin"))
        nhead, frames = read_neighbours(os.path.join(d, "neighbours.bin"))
    assert nhead == head == (300, 12, 4 if dtype == 0 else 8, dim)
    assert len(frames) == len(pos) == (13 if "--csv-detailed" in extra else 1)
    hs = nb.build_model(dtype, dim, "uniform", 300)
    t = np.arange(300)
    et = LD(eps_t(dtype))
    for k, (phi, nn, nnd2) in enumerate(frames):
        assert pos[k].dtype == npt(dtype)
        rphi, dmin, amin, dsec, dnn = reference(hs.m, pos[k], hs.c, e2_of(dtype, 0.05), t, nn)
        assert (np.abs(phi.astype(LD) - rphi) <= TOL[dtype] * np.abs(rphi)).all(), k
        assert (nn < 300).all() and (nn != t).all()
        assert (dnn <= dmin * (1 + 8 * et)).all() and (np.abs(nnd2.astype(LD) - dnn) <= 4 * et * dnn).all(), k
    if len(pos) > 1:
        assert not np.array_equal(pos[0], pos[-1])
