"""CPU: the NumPy model of the tree-pruned exact kNN (tests/nntree_model.py, a restatement of csrc/nntree.inc in T arithmetic) against
brute force sorted by (d2 by pair_d2's chain in T, index) — EXACTLY, every slot, float32 and float64.  What a GPU-less machine can
prove of the method: that the boxes, the strict prune, the `<=` gate with the lexicographic insert, the skipped masked records, the
cap at the k-th entry and the seed lose no neighbour and store none twice.  The shipped kernels are held to the all-pairs method bit
for bit by tests/test_gpu_nntree.py."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import nntree_model as M

B = M.B
TYPES = [np.float64, np.float32]


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check(x, ks):
    for k in ks:
        want_j, want_d = M.brute(x, k)
        idx, d2, tree = M.knn_tree(x, k)
        assert same(idx, want_j), (x.dtype, x.shape, k)
        assert same(d2, want_d), (x.dtype, x.shape, k)
    return tree


def test_fma_emulation_is_libm_fma():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fma.restype, libm.fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    libm.fmaf.restype, libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    rng = np.random.default_rng(5)
    for t, f in ((np.float64, libm.fma), (np.float32, libm.fmaf)):
        a = (rng.normal(0, 1, 4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(t)
        b = a.copy()  # the chain squares
        c = (np.abs(rng.normal(0, 1, 4000)) * 10.0 ** rng.integers(-14, 12, 4000)).astype(t)
        # near-cancelling and half-way cases: c = -(a b) rounded, and products that land on a rounding boundary of the sum
        a2 = rng.integers(1, 1 << 12, 2000).astype(t)
        c2 = (rng.integers(1, 1 << 24, 2000) * 2.0 ** rng.integers(20, 60, 2000)).astype(t)
        for x, y, z in ((a, b, c), (a, rng.permutation(a), -(a * a)), (a2, a2, c2), (a2, a2 + t(0.5), c2)):
            got = M.fma(x, y, z)
            want = np.array([f(float(p), float(q), float(r)) for p, q, r in zip(x, y, z)], t)
            assert same(got, want)


@pytest.mark.parametrize("k", [1, 6, 16])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_random_systems(t, dim, k):
    for n in sorted({1, 2, 3, k, k + 1, B - 1, B, B + 1, 63, 64, 65, 2 * B + 1, 1000}):
        x = np.random.default_rng(100 + n).normal(0, 1, (n, dim)).astype(t)
        check(x, [k])


def test_the_walk_prunes():
    """Not a contract, a sanity check of the structure: at n = 4000 a lane meets fewer than half of the records (the seed and the
    left-to-right walk together; about 1400 when this was written, growing slowly with n: about 1800 at n = 16000)."""
    x = np.random.default_rng(1).normal(0, 1, (4000, 3)).astype(np.float32)
    tree = check(x, [6])
    assert tree.pairs / 64 / ((4000 + 63) // 64) < 2000


@pytest.mark.parametrize("t", TYPES)
def test_shuffled_integer_lattice_ties_everywhere(t):
    rng = np.random.default_rng(4512)
    x = np.stack(np.unravel_index(rng.permutation(512), (8, 8, 8)), -1).astype(t)
    want_j, want_d = M.brute(x, 16)
    assert (want_d[:, 1:] == want_d[:, :-1]).any(1).all() and (want_d == np.round(want_d)).all()
    check(x, [1, 6, 16])


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_five_bodies_at_one_point(t, dim):
    x = np.full((5, dim), 0.375, t)
    check(x, [1, 2, 4, 6])
    idx, d2, _ = M.knn_tree(x, 6)
    assert (d2[:, :4] == 0).all() and (idx[:, 4:] == M.NONE).all() and np.isposinf(d2[:, 4:]).all()
    assert [list(r[:4]) for r in idx] == [[j for j in range(5) if j != i] for i in range(5)]


@pytest.mark.parametrize("t", TYPES)
def test_one_axis_constant(t):
    x = np.random.default_rng(9).normal(0, 1, (300, 3)).astype(t)
    x[:, 1] = t(0.25)
    check(x, [6, 16])


@pytest.mark.parametrize("t", TYPES)
def test_tight_cluster_and_one_body_far_away(t):
    x = (np.random.default_rng(11).normal(0, 1, (200, 3)) * 1e-3).astype(t)
    x[137] = t(1e6)
    check(x, [1, 6, 16])


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_the_bound_is_below_the_d2_of_every_point_in_the_box(t, dim):
    """10^4 (box, inside point, target) triples: computed bound <= computed d2, with targets outside, inside and on the faces, boxes
    of zero extent on an axis, and points on the faces and corners of the box."""
    rng = np.random.default_rng(23 + dim)
    n = 10000
    a, b = rng.normal(0, 1, (n, dim)), rng.normal(0, 1, (n, dim))
    lo, hi = np.minimum(a, b).astype(t), np.maximum(a, b).astype(t)
    hi[::7, 0] = lo[::7, 0]  # flat boxes
    u = rng.uniform(0, 1, (n, dim))
    u[rng.uniform(0, 1, (n, dim)) < 0.2] = 0.0  # on a face
    u[rng.uniform(0, 1, (n, dim)) < 0.2] = 1.0
    y = np.clip((lo + (hi - lo) * u.astype(t)).astype(t), lo, hi)
    x = rng.normal(0, 2, (n, dim)).astype(t)  # mostly outside
    inside = np.clip((lo + (hi - lo) * rng.uniform(0, 1, (n, dim)).astype(t)).astype(t), lo, hi)
    x[1::3] = inside[1::3]  # inside
    x[2::9, 0] = lo[2::9, 0]  # on a face
    x[5::9, 1] = hi[5::9, 1]
    x[8::90] *= t(1e4)  # far away: the bound is a large number with few low bits to spare
    bound, d2 = M.box_bound(lo, hi, x), M.pair_d2(y, x)
    assert (bound <= d2).all(), int((bound > d2).sum())
    kind = ((x >= lo) & (x <= hi)).all(1)
    assert kind.sum() > 2000 and (~kind).sum() > 4000 and (bound[kind] == 0).all() and (bound[~kind] > 0).any()
    assert ((x == lo) | (x == hi)).any(1).sum() > 1000
