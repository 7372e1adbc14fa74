"""CPU: the NumPy model of the friends-of-friends link walk (tests/fof_model.py, a restatement of csrc/fof.inc in T arithmetic) against
the brute-force O(n^2) component search over the same emulated chain — partitions, labels and sizes EXACTLY, float32 and float64, 2D
and 3D.  What a GPU-less machine can prove of the method: that the strict prune against b2, linking only to q < p and the early end
of the walk lose no friend, on ties included.  The shipped kernels are held to the same reference in tests/test_gpu_fof.py."""
import numpy as np
import pytest

import fof_model as M

TYPES = [np.float64, np.float32]
SIZES = [1, 2, 33, 65, 257, 1000]


def check(x, b):
    want_l, want_s = M.brute(x, b)
    label, size, tree = M.fof_tree(x, b)
    assert label.dtype == np.uint32 and np.array_equal(label, want_l), (x.dtype, x.shape, b)
    assert np.array_equal(size, want_s), (x.dtype, x.shape, b)
    n = len(x)
    assert (label <= np.arange(n)).all() and (label[label] == label).all()
    assert np.array_equal(np.bincount(label, minlength=n)[label], size)
    return label, size, tree


def lattice(n, dim, t):
    """The first n points (raster order) of an integer lattice, shuffled: every d2 and b2 = 1 are exact, so b = 1 is a tie of every
    bond, and every point but the first has a neighbour at distance exactly 1."""
    side = int(np.ceil(n ** (1.0 / dim)))
    g = np.stack(np.meshgrid(*([np.arange(side)] * dim), indexing="ij"), -1).reshape(-1, dim)[:n]
    return g[np.random.default_rng(7 + n).permutation(n)].astype(t)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_random_points_at_three_linking_lengths(t, dim, n):
    x = np.random.default_rng(300 + n).random((n, dim)).astype(t)
    groups = []
    for c in (0.5, 0.9, 1.4):  # mostly singletons, many mid-sized groups, a percolating one
        label, _, _ = check(x, c * n ** (-1.0 / dim))
        groups.append(len(np.unique(label)))
    assert groups[0] >= groups[1] >= groups[2]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_lattice_on_a_tie_and_one_ulp_below(t, dim, n):
    x = lattice(n, dim, t)
    on, _, _ = check(x, 1.0)
    below, size, _ = check(x, float(np.nextafter(t(1), t(0))))
    assert (size == 1).all() and np.array_equal(below, np.arange(n))  # one ulp below the bond length: nothing links
    assert (on == 0).all()  # on the tie every bond is met, and a raster prefix of the lattice is connected


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_coincident_points(t, dim, n):
    """Every body on one of at most three sites: b = 0 links exactly the bodies of a site (d2 = 0 <= 0)."""
    rng = np.random.default_rng(11 + n)
    sites = rng.random((3, dim)).astype(t)
    site = rng.integers(0, 3, n)
    x = sites[site]
    label, size, _ = check(x, 0.0)
    for s in range(3):
        mem = np.nonzero(site == s)[0]
        if len(mem):
            assert (label[mem] == mem[0]).all() and (size[mem] == len(mem)).all()


def test_the_walk_prunes_and_meets_each_pair_once():
    """Not a contract, a sanity check: a lane only meets records at earlier positions (whole batches of its wave's buckets aside), so
    the mean over the lanes stays below n / 2 whatever the linking length; at n = 4000 and b = 0.9 n^(-1/3) it was about 520 when
    this was written — the boxes of 32 records are several b wide there, so a wave's 64 lanes ask for many buckets."""
    x = np.random.default_rng(3).random((4000, 3)).astype(np.float32)
    _, _, tree = check(x, 0.9 * 4000 ** (-1.0 / 3))
    per_lane = tree.pairs / 4000
    print(f"pairs a lane: {per_lane:.1f}")
    assert per_lane < 4000 / 2, per_lane


def test_union_find_rules():
    parent = list(range(8))
    assert M.hook(parent, 5, 3) and parent[5] == 3  # the larger root is pointed at the smaller
    assert M.hook(parent, 7, 5) and parent[7] == 3
    assert not M.hook(parent, 7, 3)
    assert M.hook(parent, 3, 1) and parent[3] == 1
    assert all(parent[i] <= i for i in range(8))
    assert M.find(parent, 7) == 1 and parent[7] in (1, 3)  # halving only ever stores an ancestor
    edges_i, edges_j = [5, 7, 3], [3, 5, 1]
    label, size = M.labels_from_edges(8, edges_i, edges_j)
    assert list(label) == [0, 1, 2, 1, 4, 1, 6, 1] and list(size) == [1, 4, 1, 4, 1, 4, 1, 4]
