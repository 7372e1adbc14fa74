"""GPU: every form of the BVH traversal (K9) per body against the oracle's wide walk (oracle.bvh_walk_wide, validated on the CPU by
tests/test_oracle_bvh_wide.py, which also owns the systems): the per-lane walk over global memory (traversal 1), the per-lane walk
over a copy of the tree in LDS (auto, float trees of up to 2048 bodies) and the sweep written as ISA (traversal 5; auto from 4096
bodies in double) in each of its launch shapes — 8 and 4 lane ranges per group, work items, plain index order — in float and double,
2D and 3D, with the per-body counters on AND off: the plain instantiation, the one every run uses, is a different program in the sweep.

The oracle makes the reference's opening decisions and the GPU's counters are held to them bit for bit, so body i of the GPU and
of the wide walk accumulate the same entries.  Bound, per body and component, against the body's own sum of term magnitudes:
|a - a_wide| <= FORCE_TOL * scale_i (the project's force bound: 1e-12 double, 2e-5 float).  The plain run must equal the counting
run bit for bit, and every form every other.

The figures an MI355X gave are in profiles/tests_bvh_wide/new_tests_figures.txt."""
import numpy as np
import pytest

from test_oracle_bvh_wide import (CASE_DIMS, CASE_IDS, FORCE_TOL, SHAPE_CASES, SHAPE_IDS, per_body, sorted_of, state_of, thetas_of,
                                  wide_of)

pytestmark = pytest.mark.gpu


def host_of(nb, s):
    hs = nb.HostSystem(s.dtype, s.dim, s.n)
    hs.m[:], hs.x[:], hs.v[:] = s.m, s.x, s.v
    hs.c, hs.dt = s.c, s.dt
    return hs


def built(nb, name, n, dtype, dim):
    """bounding_box -> hilbert_sort -> build_tree on the unsorted system of a case; the permutation must be the oracle's.  Returns
    the device system with its bodies in key order."""
    dev = nb.DeviceSystem.from_host(host_of(nb, state_of(name, n, dtype, dim)))
    st, t = dev.state(), dev.bvh
    t.bounding_box(st, dev.stream)
    t.hilbert_sort(st, dev.stream)
    assert np.array_equal(t.read(1, dev.stream), sorted_of(name, n, dtype, dim)[2]), "permutation"
    t.build_tree(st, dev.stream)
    return dev


def zero_a(dev):
    hs = dev.download()
    hs.a[:] = 0
    dev.upload(hs)


def force(dev, theta, mode, order=0, counters=False, windows=None):
    """One traversal into a zeroed `a`: (a, counters or None)."""
    t = dev.bvh
    t.set_traversal(mode)
    t.set_launch_order(order)
    t.enable_counters(counters)
    zero_a(dev)
    for first, count in windows or ((0, None),):
        t.compute_force(dev.state(first, count), theta, dev.stream)
    dev.sync()
    a = dev.download().a.copy()
    cnt = t.read(5, dev.stream) if counters else None
    t.set_launch_order(0)
    return a, cnt


def check_forms(nb, name, n, dtype, dim, forms):
    """Every (traversal, launch order) of `forms` at every angle of the case: counting run against the wide walk, plain run
    bitwise equal to it, every form bitwise equal to the first.  Prints one figure per form and angle."""
    dev = built(nb, name, n, dtype, dim)
    for theta in thetas_of(name, n):
        w = wide_of(name, n, dtype, dim, theta)
        first = None
        for mode, order in forms:
            a, cnt = force(dev, theta, mode, order, counters=True)
            assert np.array_equal(cnt, w.counts), (theta, mode, order, "counters")
            assert np.isfinite(a).all(), (theta, mode, order)
            err = per_body(a, w.a, w.scale)
            print(f"gpu vs wide {name} {n} {dim}D dtype {dtype} theta {theta} traversal {mode} order {order}: max err_i {err:.3g}")
            assert err <= FORCE_TOL[dtype], (theta, mode, order, err)
            plain, _ = force(dev, theta, mode, order, counters=False)
            assert np.array_equal(plain, a), (theta, mode, order, "counters off")
            if first is None:
                first = a
            assert np.array_equal(a, first), (theta, mode, order, "forms differ")
    dev.close()


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("name, n, dim", CASE_DIMS, ids=CASE_IDS)
def test_traversal_forms_against_the_wide_walk(nb, oracle, name, n, dim, dtype):
    """Every case of tests/test_oracle_bvh_wide.py at its angles through traversal 1 (per-lane, global memory), 5 (the sweep) and 0
    (auto: the LDS walk for float trees of up to 2048 bodies, the sweep for double from 4096, else the per-lane walk), counters on
    and off.  Where auto is the LDS walk (test_oracle_bvh_wide.py::test_lds_sizes: float up to 2048 bodies, 2049 is past it) it is
    thereby compared bitwise with traversal 1.
    measured on an MI355X, max over cases, angles and forms of the per-body figure: 3.6e-15 of scale in double and 1.8e-6 in float
    (both galaxy 4099 3D, theta 0.5; the three forms agree bit for bit, so they share every figure); the reference's own T walk
    gives 3.9e-15 and 1.9e-6 on the same cases.  Nothing was over the bound, so csrc/bvh.hip is unchanged.  With the - eps y^3
    term of weight_far dropped in tree_accumulate (a scratch build) pairs 257 / 4099 in double give 2.8e-9 / 3.5e-9 in 3D and
    3.7e-9 / 3.4e-9 in 2D at traversal 1, and clusters 4099 fails as well."""
    check_forms(nb, name, n, dtype, dim, ((1, 0), (5, 0), (0, 0)))


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("name, n, dim", SHAPE_CASES, ids=SHAPE_IDS)
def test_sweep_launch_shapes_against_the_wide_walk(nb, oracle, name, n, dim, dtype):
    """The sweep's launch shapes at the smallest galaxies that reach them, count -> groups of 64 -> shape (tools/bvh_plan_check.cpp
    pins the four plans): 4099 -> 65 -> 8 lane ranges per group (galaxy 4099 of the test above, 3D and 2D); 20545 -> 322 -> 4
    ranges; 41001 -> 641 -> 1 range with work items (above 2048 pairs the sort ends in its starting buffer, so the sorted keys are
    where bvh_items_kernel reads them), 3D and 2D, and 41001 in plain index order (launch order 1: no items).  Double on auto,
    float on traversal 5 (auto takes the sweep from 180 000 bodies on in float), theta 0.5, all rows of the wide walk.
    measured on an MI355X: 4.3e-15 (20545), 6.1e-15 (41001 3D) and 3.9e-15 (41001 2D) of scale in double, 3.0e-6, 3.5e-6 and
    2.0e-6 in float, items and index order bit for bit the same; the reference's T walk gives 4.1e-15, 6.4e-15, 3.9e-15 and
    3.0e-6, 3.5e-6, 2.0e-6."""
    mode = 0 if dtype == 1 else 5
    check_forms(nb, name, n, dtype, dim, ((mode, 0),) + (((mode, 1),) if n == 41001 else ()))


@pytest.mark.parametrize("dtype, dim", [(0, 3), (1, 2)])
def test_shard_windows_that_start_inside_a_group(nb, oracle, dtype, dim):
    """galaxy 4099, float 3D and double 2D, traversal 1 and 5, counters off: windows (0, 1000), (1000, 2001), (3001, 1098) — none of
    the inner edges a multiple of 64 — into a zeroed `a` give the full traversal bit for bit, which is within the per-body bound."""
    name, n, theta = "galaxy", 4099, 0.5
    dev = built(nb, name, n, dtype, dim)
    w = wide_of(name, n, dtype, dim, theta)
    for mode in (1, 5):
        full, _ = force(dev, theta, mode)
        part, _ = force(dev, theta, mode, windows=((0, 1000), (1000, 2001), (3001, 1098)))
        assert np.array_equal(part, full), mode
        err = per_body(full, w.a, w.scale)
        print(f"gpu vs wide windows galaxy {n} {dim}D dtype {dtype} theta {theta} traversal {mode}: max err_i {err:.3g}")
        assert np.isfinite(full).all() and err <= FORCE_TOL[dtype], (mode, err)
    dev.close()
