"""GPU: the tree-pruned exact kNN (NBODY_KNN_TREE, csrc/nntree.inc) against the all-pairs method of the same handle type, BIT FOR BIT.
The tie rule of include/nbody_hip.h is exact, so the k neighbours are a set with one correct answer and no tolerance is involved:
every case computes idx, d2, rho and the summary (x_dc, r_c, rho_c) with a TREE and an ALL_PAIRS handle on the same DeviceSystem and
compares the raw bits (NaN summaries included).  Where the input allows an exact integer reference (lattices) both are also held to
it, and three sizes are held to the NumPy-longdouble criteria of tests/test_gpu_knn.py, whose systems, references and checks are
imported, not copied.

Sizes: B = 32 records a bucket, 64 targets a wave (two buckets), the hierarchy padded to a power of two of buckets — so B - 1, B,
B + 1, the wave (63, 64, 65), bucket counts on either side of a power of two (4 | 5 buckets: 128 | 129, 8 | 9: 256 | 257), the sort's
forms (one block up to 2048 | splitters up to 1 572 864 | radix passes beyond), and the sizes 1, 2, 3 and k, k + 1 of a list that is
not full."""
import functools
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_knn import KS, KS_CAPACITY, LD, MID, NONE, case, check_lists, eps_t, npt, random_system, reference_rho, summary_bytes

pytestmark = pytest.mark.gpu

B = 32
SIZES = [1, 2, 3, 4, 6, 7, 16, 17, B - 1, B, B + 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 4097, 65537]
SPLITTER_MAX_N = 768 * 2048  # kSplitterMaxN of csrc/radix_sort.hpp


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def outputs(dev, k, method):
    """(idx, d2, rho, x_dc, r_c, rho_c) of one compute with the system's handle for (k, method)."""
    h = dev.knn_handle(k, method)
    assert h.method == method
    h.compute(dev.state(), dev.stream)
    xdc, rc, rhoc = h.density_centre(dev.stream)
    return h.read(0, dev.stream), h.read(1, dev.stream), h.read(2, dev.stream), xdc, np.asarray(rc), np.asarray(rhoc)


NAMES = ("idx", "d2", "rho", "x_dc", "r_c", "rho_c")


def assert_identical(dev, k, what=""):
    tree, full = outputs(dev, k, "tree"), outputs(dev, k, "all-pairs")
    for name, a, b in zip(NAMES, tree, full):
        if not same(a, b):
            bad = np.argwhere(np.atleast_1d(a != b) | np.atleast_1d(np.isnan(a) != np.isnan(b)))
            raise AssertionError(f"{what} k={k}: {name} differs from all-pairs at {len(bad)} places, first {bad[:4].tolist()}")
    return tree


def system_of(nb, dtype, x, m=None):
    n, dim = x.shape
    hs = nb.HostSystem(dtype, dim, n)
    hs.x[:] = x.astype(npt(dtype))
    hs.m[:] = (np.random.default_rng(n).uniform(0.5, 1.5, n) / n if m is None else m).astype(npt(dtype))
    hs.dt, hs.c = 0.01, 1.0
    return hs


# ---- 1. random systems -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_random_systems_are_identical_to_all_pairs(nb, dtype, dim, n):
    hs = random_system(nb, dtype, dim, n, seed=100 + n)
    dev = nb.DeviceSystem.from_host(hs)
    try:
        for k in KS:
            idx, d2, rho, *_ = assert_identical(dev, k, f"dtype={dtype} dim={dim} n={n}")
            have = min(k, n - 1)
            assert (idx[:, have:] == NONE).all() and np.isposinf(d2[:, have:]).all() and (idx[:, :have] < n).all()
            if k == 1 or n <= k:
                assert (rho == 0).all()
    finally:
        dev.close()


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_list_capacities_from_either_side(nb, dtype, dim):
    hs = random_system(nb, dtype, dim, MID, seed=100 + MID)
    dev = nb.DeviceSystem.from_host(hs)
    try:
        for k in KS_CAPACITY:
            assert_identical(dev, k, f"dtype={dtype} dim={dim} n={MID}")
    finally:
        dev.close()


# ---- 2. the radix form of the sort -------------------------------------------------------------------------------------------------------
def test_the_radix_form_of_the_sort_once(nb):
    n = SPLITTER_MAX_N + 1
    hs = random_system(nb, 0, 3, n, seed=100 + n)
    dev = nb.DeviceSystem.from_host(hs)
    try:
        assert_identical(dev, 6, f"float 3D n={n}")
    finally:
        dev.close()


# ---- 3. ties -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(dim):
    """The shuffled 8 x 8 x 8 (3D) or 64 x 64 (2D) integer lattice and per body the 16 smallest (d2, index) in int64 — the exact
    reference, computed once, shared by both types, never changed, and not involving the code under test."""
    shape = (8, 8, 8) if dim == 3 else (64, 64)
    n = int(np.prod(shape))
    rng = np.random.default_rng(4500 + n)
    coords = np.stack(np.unravel_index(rng.permutation(n), shape), -1).astype(np.int64)
    want_j, want_d = np.empty((n, 16), np.int64), np.empty((n, 16), np.int64)
    order = np.arange(n)
    for i in range(n):
        d = coords - coords[i]
        D2 = (d * d).sum(-1)
        D2[i] = 1 << 40  # the self pair is out by index
        o = np.lexsort((order, D2))[:16]
        want_j[i], want_d[i] = o, D2[o]
    for a in (coords, want_j, want_d):
        a.setflags(write=False)
    return coords, want_j, want_d


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_exact_ties_on_shuffled_lattices(nb, dtype, dim):
    coords, want_j, want_d = lattice(dim)
    assert (want_d[:, 1:] == want_d[:, :-1]).any(1).all()  # ties in every row
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, coords))
    try:
        for k in (6, 16):
            idx, d2, *_ = assert_identical(dev, k, f"lattice dtype={dtype} dim={dim}")
            assert np.array_equal(idx.astype(np.int64), want_j[:, :k]), k
            assert np.array_equal(d2, want_d[:, :k].astype(npt(dtype))), k
    finally:
        dev.close()


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_coincident_and_duplicated_bodies_and_a_constant_axis(nb, dtype, dim):
    rng = np.random.default_rng(77 + dim)
    five = np.full((5, dim), 0.375)
    half = rng.normal(0, 1, (700, dim))
    twice = np.concatenate([half, half])[rng.permutation(1400)]
    flat = rng.normal(0, 1, (1500, dim))
    flat[:, 1] = 0.25
    for name, x, ks in (("five at one point", five, (1, 2, 4, 6)), ("every body twice", twice, (2, 6, 16)), ("one axis constant", flat, (6, 16))):
        dev = nb.DeviceSystem.from_host(system_of(nb, dtype, x))
        try:
            for k in ks:
                idx, d2, rho, *_ = assert_identical(dev, k, f"{name} dtype={dtype} dim={dim}")
                if name == "five at one point":
                    assert [list(r[:4]) for r in idx[:, :min(k, 4)].tolist()] == [[j for j in range(5) if j != i][:k] for i in range(5)]
                    assert (d2[:, :min(k, 4)] == 0).all() and (idx[:, 4:] == NONE).all()
                if name == "every body twice":
                    assert (d2[:, 0] == 0).all()
        finally:
            dev.close()


# ---- 4. adverse geometry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
def test_a_tight_cluster_and_one_body_far_away(nb, dtype):
    """4097 bodies within 1e-3 and one at 1e6: the bounds are 1e6 wide, so nearly all keys are equal and the order is by index."""
    x = np.random.default_rng(12).normal(0, 1, (4098, 3)) * 1e-3 / 4
    x[2500] = (1e6, 0.0, 0.0)
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, x))
    try:
        for k in (1, 6, 16):
            assert_identical(dev, k, f"cluster dtype={dtype}")
    finally:
        dev.close()


@pytest.mark.parametrize("model", ["plummer", "galaxy"])
@pytest.mark.parametrize("dtype", [1, 0])
def test_the_models_of_the_cli(nb, dtype, model):
    dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, model, 20000))
    try:
        for k in (6, 16):
            assert_identical(dev, k, f"{model} dtype={dtype}")
    finally:
        dev.close()


# ---- 5. the order of the bodies does not matter --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
def test_order_independence_and_an_untouched_state(nb, dtype):
    """The same 4097 bodies as generated, shuffled and reversed: per body the same d2 row bit for bit and the same neighbour SET after
    mapping the indices (rows whose k-th and (k + 1)-th d2 are equal are compared on d2 only: there the tie rule, which is by index,
    may pick another body).  The state's arrays are bit-identical after a tree compute."""
    n, k = 4097, 6
    hs = random_system(nb, dtype, 3, n, seed=100 + n)
    rng = np.random.default_rng(3)
    got = {}
    for name, p in (("as generated", np.arange(n)), ("shuffled", rng.permutation(n)), ("reversed", np.arange(n)[::-1].copy())):
        sys = nb.HostSystem(dtype, 3, n)
        sys.m[:], sys.x[:], sys.v[:] = hs.m[p], hs.x[p], hs.v[p]
        sys.dt, sys.c = hs.dt, hs.c
        dev = nb.DeviceSystem.from_host(sys)
        try:
            idx, d2 = dev.knn(k + 1, method="tree")
            after = dev.download()
            assert same(after.x, sys.x) and same(after.m, sys.m) and same(after.v, sys.v), name
        finally:
            dev.close()
        inv = np.empty(n, np.int64)
        inv[p] = np.arange(n)
        got[name] = (p[idx.astype(np.int64)][inv], d2[inv])  # rows and indices in the generated order
    base_j, base_d = got["as generated"]
    clear = base_d[:, k] > base_d[:, k - 1]
    assert clear.sum() > 0.99 * n
    for name in ("shuffled", "reversed"):
        j, d = got[name]
        assert same(d, base_d), name
        assert np.array_equal(np.sort(j[clear, :k], 1), np.sort(base_j[clear, :k], 1)), name


# ---- 6. an independent reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 4097, 65537])
@pytest.mark.parametrize("dtype", [1, 0])
def test_against_numpy_longdouble(nb, dtype, n):
    """The criteria of tests/test_gpu_knn.py (its case, bounds and check_lists, the cap of 1e-3 slots without a clear gap included) on
    the TREE method alone, k = 16, 3D; rho within 32 eps_T of longdouble from the method's own idx."""
    dim, k = 3, 16
    hs, t, val, arg = case(dtype, dim, n)
    dev = nb.DeviceSystem.from_host(hs)
    try:
        idx, d2, rho, *_ = outputs(dev, k, "tree")
    finally:
        dev.close()
    amb, slots, derr = check_lists(hs, dtype, dim, n, k, t, val, arg, idx, d2)
    ref = reference_rho(hs.m, hs.x, idx, k, dim)
    rerr = float((np.abs(rho.astype(LD) - ref) / ref).max()) / eps_t(dtype)
    print(f"nntree dtype={dtype} n={n} k={k}: {amb} of {slots} slots without a clear gap, worst d2 error {derr:.3g} eps, rho {rerr:.3g} eps (bound 32)")
    assert rerr <= 32


# ---- 7. handle behaviour --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(1000, 6), (5889, 16), (65537, 6)])
@pytest.mark.parametrize("dtype", [1, 0])
def test_bitwise_repeatable_eager_replayed_and_new_handle(nb, dtype, n, k):
    hs = random_system(nb, dtype, 3, n, seed=80 + n)
    dev = nb.DeviceSystem.from_host(hs)

    def read_all():
        h = dev.knn_handle(k, "tree")
        return tuple(h.read(w, dev.stream).tobytes() for w in range(3)) + (summary_bytes(h.density_centre(dev.stream)),)

    dev.knn_compute(k, "tree")
    first = read_all()
    dev.knn_compute(k, "tree")
    assert read_all() == first
    dev._knn_other.pop((k, "tree")).close()  # a handle destroyed and made again
    dev.knn_compute(k, "tree")
    assert read_all() == first
    # recorded and replayed; the handle's arrays are overwritten in between so that the replay has to produce them
    g = nb.StepGraph(dev, lambda: dev.knn_compute(k, "tree"))
    dev2 = nb.DeviceSystem.from_host(random_system(nb, dtype, 3, n, seed=81 + n))
    dev.knn_handle(k, "tree").compute(dev2.state(), dev2.stream)
    dev2.sync()
    assert all(a != b for a, b in zip(read_all(), first))
    g.launch()
    assert read_all() == first
    g.launch()
    assert read_all() == first
    g.close()
    dev2.close()
    dev.close()


def test_call_sequence_and_method(nb):
    L = nb.lib()
    hs = random_system(nb, 1, 3, 300, seed=1)
    dev = nb.DeviceSystem.from_host(hs)
    st = dev.state()

    def rc_of(call):
        try:
            call()
        except nb.NbodyError as e:
            return int(re.match(r"nbody backend error (\d+)", str(e)).group(1)), str(e)
        return 0, ""

    h = nb.Knn(1, 3, 300, 6, dev.device, "tree")
    plain = nb.Knn(1, 3, 300, 6, dev.device)
    assert h.method == "tree" and L.nbody_knn_method(h.h) == 1
    assert plain.method == "all-pairs" and L.nbody_knn_method(plain.h) == 0
    plain.close()
    assert rc_of(lambda: h.read(0, dev.stream))[0] == 3  # NBODY_ERR_STATE before the first compute
    assert rc_of(lambda: h.density_centre(dev.stream))[0] == 3
    for other in (nb.Knn(1, 3, 301, 6, dev.device, "tree"), nb.Knn(0, 3, 300, 6, dev.device, "tree"), nb.Knn(1, 2, 300, 6, dev.device, "tree")):
        rc, msg = rc_of(lambda: other.compute(st, dev.stream))
        assert rc == 1 and "was created for" in msg
        other.close()
    h.compute(st, dev.stream)
    assert h.read(0, dev.stream).shape == (300, 6)
    h.close()
    # the system keeps one handle per (k, method) and closes them all
    dev.knn(6)
    dev.knn(6, method="tree")
    assert dev.knn_handle(6, "tree") is dev.knn_handle(6, "tree") and dev.knn_handle(6, "tree") is not dev.knn_handle(6)
    assert sorted(dev._knn) == [6] and sorted(dev._knn_other) == [(6, "tree")]
    dev.close()
    assert dev._knn == {} and dev._knn_other == {}


# ---- 8. CLI ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--algorithm", "octree"], ["--algorithm", "bvh", "--precision", "double"]],
                         ids=["default", "octree", "bvh_double"])
def test_cli_density_tree_writes_the_same_bytes(nb, extra):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")
    base = [exe, "-n", "3000", "-s", "20", "--workload", "plummer", "--csv-detailed", "--save-density", "6"] + extra
    with tempfile.TemporaryDirectory() as d0, tempfile.TemporaryDirectory() as d1:
        r0 = subprocess.run(base, cwd=d0, capture_output=True, text=True, timeout=600)
        assert r0.returncode == 0, r0.stderr
        r1 = subprocess.run(base + ["--density-tree"], cwd=d1, capture_output=True, text=True, timeout=600)
        assert r1.returncode == 0, r1.stderr
        a, b = open(os.path.join(d0, "density.bin"), "rb").read(), open(os.path.join(d1, "density.bin"), "rb").read()
    tsz = 8 if "double" in extra else 4
    assert struct.unpack("<5I", a[:20]) == (3000, 20, tsz, 3, 6) and len(a) > 20 + (3000 + 5) * tsz
    assert a == b
