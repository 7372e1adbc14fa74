"""CPU: the NumPy model of the fixed-radius neighbour-list walk (tests/nlist_model.py, a restatement of csrc/nlist.inc in T
arithmetic) against the definition by brute force over the same emulated chain — count, offset and list EXACTLY, scalar and per-body
radii, float32 and float64, 2D and 3D, n over the bucket (32) and wave (64) boundaries.  What a GPU-less machine can prove of the
method: that the strict prune against a cap PER LANE loses no neighbour, on ties included, and that placing by rank orders a
segment.  The shipped kernels are held to the same references in tests/test_gpu_nlist.py."""
import numpy as np
import pytest

import nlist_model as M

TYPES = [np.float64, np.float32]
SIZES = [1, 2, 31, 33, 63, 65, 129, 257, 1000]


def check(x, **radius):
    want = M.brute(x, **radius)
    count, offset, idx, tree = M.walk(x, **radius)
    n = len(x)
    assert count.dtype == np.uint32 and offset.dtype == np.uint64 and idx.dtype == np.uint32
    assert np.array_equal(count, want[0]) and np.array_equal(offset, want[1]) and np.array_equal(idx, want[2]), (x.dtype, x.shape, radius)
    assert offset[0] == 0 and offset[n] == len(idx) and np.array_equal(np.diff(offset), count)
    for i in range(n):
        seg = idx[int(offset[i]):int(offset[i + 1])].astype(np.int64)
        assert (np.diff(seg) > 0).all() and i not in seg
    return count, offset, idx, tree


def lattice(n, dim, t):
    """The first n points (raster order) of an integer lattice, shuffled: every d2 and r2 = 1 are exact, so r = 1 is a tie of every
    bond."""
    side = int(np.ceil(n ** (1.0 / dim)))
    g = np.stack(np.meshgrid(*([np.arange(side)] * dim), indexing="ij"), -1).reshape(-1, dim)[:n]
    return g[np.random.default_rng(7 + n).permutation(n)].astype(t), side


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_random_points_at_three_scalar_radii(t, dim, n):
    x = np.random.default_rng(300 + n).random((n, dim)).astype(t)
    totals = []
    for c in (0.5, 1.4, 2.5):
        count, offset, idx, _ = check(x, r=c * n ** (-1.0 / dim))
        totals.append(len(idx))
        # symmetric: (i, j) is listed iff (j, i) is
        i = np.repeat(np.arange(n), count)
        assert set(zip(i.tolist(), idx.tolist())) == set(zip(idx.tolist(), i.tolist())) and len(idx) % 2 == 0
    assert totals[0] <= totals[1] <= totals[2]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_per_body_radii_are_a_gather(t, dim, n):
    rng = np.random.default_rng(900 + n)
    x = rng.random((n, dim)).astype(t)
    v = (rng.random(n) * 3.0 * n ** (-1.0 / dim)).astype(t)
    v[rng.random(n) < 0.2] = 0  # some bodies list nothing (nothing is coincident here)
    count, _, _, _ = check(x, radii=v)
    assert (count[v == 0] == 0).all()
    check(x, radii=(v * v).astype(t), squared=True)  # the same r2_i, given squared
    got = M.walk(x, radii=(v * v).astype(t), squared=True)[:3]
    assert all(np.array_equal(a, b) for a, b in zip(got, M.walk(x, radii=v)[:3]))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_lattice_on_a_tie_and_one_ulp_below(t, dim, n):
    x, side = lattice(n, dim, t)
    count, _, _, _ = check(x, r=1.0)
    below = check(x, r=float(np.nextafter(t(1), t(0))))
    assert (below[0] == 0).all() and len(below[2]) == 0  # one ulp below the bond length: nobody is within it
    # on the tie every bond is met: the bonds of a raster prefix, counted in integers
    g = x.astype(np.int64)
    occupied = {tuple(p) for p in g.tolist()}
    want = [sum(tuple(p + s * e) in occupied for e in np.eye(dim, dtype=np.int64) for s in (-1, 1)) for p in g]
    assert count.tolist() == want


@pytest.mark.parametrize("n", [1, 33, 257])
@pytest.mark.parametrize("t", TYPES)
def test_coincident_points_at_radius_zero(t, n):
    """Every body on one of at most three sites: r = 0 lists exactly the other bodies of the site (d2 = 0 <= 0)."""
    rng = np.random.default_rng(11 + n)
    site = rng.integers(0, 3, n)
    x = rng.random((3, 3)).astype(t)[site]
    count, offset, idx, _ = check(x, r=0.0)
    for i in range(n):
        mates = np.nonzero((site == site[i]) & (np.arange(n) != i))[0]
        assert np.array_equal(idx[int(offset[i]):int(offset[i + 1])], mates)


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("t", TYPES)
def test_the_cell_list_is_the_definition(t, dim):
    n = 1500
    x = np.random.default_rng(5).random((n, dim)).astype(t)
    r = 1.4 * n ** (-1.0 / dim)
    want = M.brute(x, r=r)
    got = M.cell_list(x, r)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert np.array_equal(M.summary(got[0]), [len(got[2]), got[0].max(), np.argmax(got[0]), 0])


def test_rank_order_and_summary():
    seg = np.random.default_rng(1).permutation(5000)[:777]
    assert np.array_equal(M.rank_order(seg), np.sort(seg)) and len(M.rank_order([])) == 0
    count = np.array([3, 7, 0, 7, 1], np.uint32)
    assert M.summary(count).tolist() == [18, 7, 1, 0]  # the lowest index among the largest
    assert M.summary(count, 17).tolist() == [18, 7, 1, M.OVER_CAPACITY] and M.summary(count, 18)[3] == 0
    big = np.array([M.MAX_PER_BODY + 1, 2], np.uint32)
    assert M.summary(big, 10)[3] == M.OVER_CAPACITY | M.OVER_PER_BODY and M.summary(big)[3] == M.OVER_PER_BODY
    assert M.summary(np.zeros(1, np.uint32)).tolist() == [0, 0, 0, 0]


def test_the_walk_prunes():
    """Not a contract, a sanity check: a lane meets far fewer than the n - 1 records of an all-pairs sweep."""
    n = 4000
    x = np.random.default_rng(3).random((n, 3)).astype(np.float32)
    _, _, _, tree = check(x, r=1.4 * n ** (-1.0 / 3))
    per_lane = tree.pairs / n
    print(f"pairs a lane: {per_lane:.1f}")
    assert per_lane < n / 2, per_lane
