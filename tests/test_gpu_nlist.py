"""GPU: exact fixed-radius neighbour lists (nbody_nlist_*, csrc/nlist.inc) against references in the same T arithmetic, EXACTLY.  count,
offset, list and summary are integers with one correct answer — the test is d2 <= r2_i on pair_d2's own chain, which
tests/nlist_model.py emulates bit for bit — so no tolerance is involved anywhere.  Every test computes the reference's total first and
makes the handle with exactly that capacity.

Sizes: 32 records a bucket, 64 targets a wave, 256 lanes a block and a strip, the hierarchy padded to a power of two of buckets — so
31 | 32 | 33, 63 | 64 | 65, 127 .. 129, 255 .. 257, the sort's one-block form up to 2048 and the splitter form beyond (2047, 2049,
4097, 65 537); segment lengths around the ordering's 64 entries a round and its limit of 4096."""
import functools
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import nlist_model as M
from conftest import ROOT
from fof_model import b2_of, labels_from_edges
from nntree_model import pair_d2

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025, 2047, 2049, 4097]
CS = (0.5, 1.4, 2.5)  # r = c n^(-1/D): in 3D about 0.5, 11 and 65 neighbours a body
BIG = 65537


def npt(dtype):
    return np.float64 if dtype == 1 else np.float32


def system_of(nb, dtype, x):
    n, dim = x.shape
    hs = nb.HostSystem(dtype, dim, n)
    hs.x[:] = x.astype(npt(dtype))
    hs.m[:] = (np.random.default_rng(n).uniform(0.5, 1.5, n) / n).astype(npt(dtype))
    hs.dt, hs.c = 0.01, 1.0
    return hs


@functools.lru_cache(maxsize=None)
def uniform(dtype, dim, n):
    x = np.random.default_rng(500 + n).random((n, dim)).astype(npt(dtype))
    x.setflags(write=False)
    return x


def radii_of(dim, n):
    return [c * n ** (-1.0 / dim) for c in CS]


@functools.lru_cache(maxsize=None)
def reference(dtype, dim, n):
    """[(count, offset, idx)] of uniform(dtype, dim, n) at the three radii: brute force, computed once and shared."""
    return M.brute_many(uniform(dtype, dim, n), radii_of(dim, n))


def rc_of(nb, call):
    try:
        call()
    except nb.NbodyError as e:
        return int(re.match(r"nbody backend error (\d+)", str(e)).group(1)), str(e)
    return 0, ""


def run(dev, capacity, r=None, radii=None, squared=False):
    """(count, offset, idx, summary) of the state as it is, on the system's handle for `capacity`."""
    h = dev.nlist_handle(capacity)
    dev._nlist_run(h, r, radii, squared)
    return (*h.lists(dev.stream), h.summary(dev.stream))


def assert_exact(got, want, capacity, what=""):
    count, offset, idx, summary = got
    wc, wo, wi = want
    assert count.dtype == np.uint32 and offset.dtype == np.uint64 and idx.dtype == np.uint32 and summary.dtype == np.uint64
    bad = np.nonzero(count != wc)[0]
    assert len(bad) == 0, f"{what}: count differs at {len(bad)} bodies, first {bad[:4].tolist()}: {count[bad[:4]].tolist()} != {wc[bad[:4]].tolist()}"
    assert np.array_equal(offset, wo), f"{what}: offset differs"
    assert len(idx) == len(wi), (what, len(idx), len(wi))
    bad = np.nonzero(idx != wi)[0]
    assert len(bad) == 0, f"{what}: list differs at {len(bad)} entries, first {bad[:4].tolist()}: {idx[bad[:4]].tolist()} != {wi[bad[:4]].tolist()}"
    assert np.array_equal(summary, M.summary(wc, capacity)), (what, summary, M.summary(wc, capacity))
    # every segment strictly ascending: a step down or a repeat only where the next segment starts
    starts = np.zeros(len(idx) + 1, bool)
    starts[offset[:-1].astype(np.int64)] = True
    assert ((np.diff(idx.astype(np.int64)) > 0) | starts[1:len(idx)]).all(), what


def pairs_of(count, idx):
    return np.repeat(np.arange(len(count), dtype=np.int64), count), idx.astype(np.int64)


# ---- 1. random uniform systems ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_random_systems_equal_brute_force(nb, dtype, dim, n):
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, uniform(dtype, dim, n)))
    try:
        for r, want in zip(radii_of(dim, n), reference(dtype, dim, n)):
            total = len(want[2])
            got = run(dev, total, r)
            assert_exact(got, want, total, what=f"dtype={dtype} dim={dim} n={n} r={r}")
            i, j = pairs_of(got[0], got[2])  # the scalar radius is symmetric: (i, j) is listed iff (j, i) is
            assert total % 2 == 0 and np.array_equal(np.sort(i * n + j), np.sort(j * n + i))
    finally:
        dev.close()


# ---- 2. one large random size (the splitter sort; a cell-list reference) ----------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim", [(0, 3), (1, 3), (0, 2), (1, 2)])
def test_one_large_size_equals_the_cell_list(nb, dtype, dim):
    x = uniform(dtype, dim, BIG)
    r = 1.4 * BIG ** (-1.0 / dim)
    want = M.cell_list(x, r)
    total = len(want[2])
    assert total > 4 * BIG
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, x))
    try:
        assert_exact(run(dev, total, r), want, total, what=f"dtype={dtype} dim={dim} n={BIG}")
    finally:
        dev.close()


# ---- 3. an integer lattice with gaps: r2 and every d2 are exact ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(dim):
    side = 16 if dim == 3 else 64
    g = np.stack(np.meshgrid(*([np.arange(side)] * dim), indexing="ij"), -1).reshape(-1, dim)
    g = g[g[:, 0] % 5 != 4]  # every fifth plane removed
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def lattice_pairs(dim, r2):
    """Integer arithmetic: the directed pairs (i, j) of lattice points whose integer squared distance is <= r2, j != i."""
    g = lattice(dim)
    side = int(g.max()) + 1
    index = -np.ones((side + 4,) * dim, np.int64)
    index[tuple((g + 2).T)] = np.arange(len(g))
    reach = int(np.floor(np.sqrt(r2)))
    offs = np.stack(np.meshgrid(*([np.arange(-reach, reach + 1)] * dim), indexing="ij"), -1).reshape(-1, dim)
    offs = offs[((offs**2).sum(1) <= r2) & ((offs**2).sum(1) > 0)]
    ei, ej = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for off in offs:
        j = index[tuple((g + 2 + off).T)]
        ok = j >= 0
        ei.append(np.nonzero(ok)[0])
        ej.append(j[ok])
    return np.concatenate(ei), np.concatenate(ej)


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_lattice_in_three_orders(nb, dtype, dim):
    t = npt(dtype)
    g = lattice(dim)
    n = len(g)
    orders = [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(4).permutation(n)]
    rs = [1.0, float(t(np.sqrt(2.0))), 2.0, float(np.nextafter(t(1), t(0)))]
    r2ints = [int(np.floor(float(b2_of(r, t)))) for r in rs]  # an integer d2 is <= r2 iff it is <= floor(r2)
    assert r2ints[0] == 1 and r2ints[2] == 4 and r2ints[3] == 0 and r2ints[1] in (1, 2)  # sqrt(2) rounded, squared: below or above 2
    for order in orders:  # body k of this system is lattice point order[k]
        inv = np.empty(n, np.int64)
        inv[order] = np.arange(n)
        dev = nb.DeviceSystem.from_host(system_of(nb, dtype, g[order].astype(t)))
        try:
            for r, r2 in zip(rs, r2ints):
                ci, cj = lattice_pairs(dim, r2)
                want = M.from_pairs(n, inv[ci], inv[cj])  # the same lists after the renaming
                total = len(want[2])
                assert_exact(run(dev, total, r), want, total, what=f"dtype={dtype} dim={dim} r={r}")
        finally:
            dev.close()
    assert len(lattice_pairs(dim, 0)[0]) == 0 and len(lattice_pairs(dim, 1)[0]) < len(lattice_pairs(dim, 2)[0]) < len(lattice_pairs(dim, 4)[0])


# ---- 4. segment lengths ---------------------------------------------------------------------------------------------------------------------
def cluster_system(dtype, dim, L, r):
    """L + 1 bodies inside a ball of radius r / 4 and 33 far bodies more than r apart from everything, indices shuffled.  Returns (x,
    the cluster's indices ascending)."""
    t = npt(dtype)
    rng = np.random.default_rng(70 + L)
    u = rng.normal(size=(L + 1, dim))
    u *= (0.25 * r * rng.random(L + 1) ** (1.0 / dim) / np.linalg.norm(u, axis=1))[:, None]
    far = np.zeros((33, dim))
    far[:, 0] = 10.0 * r * (1 + np.arange(33))
    x = np.concatenate([u + 3.0, far + 3.0]).astype(t)
    perm = rng.permutation(len(x))
    out = np.empty_like(x)
    out[perm] = x
    return out, np.sort(perm[:L + 1])


def cluster_want(n, members):
    lists = [np.zeros(0, np.int64)] * n
    for i in members:
        lists[i] = members[members != i]
    return M.pack(lists)


@pytest.mark.parametrize("L", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096])
@pytest.mark.parametrize("dtype,dim", [(1, 3), (0, 2)])
def test_segment_lengths(nb, dtype, dim, L):
    r = 0.5
    x, members = cluster_system(dtype, dim, L, r)
    n = len(x)
    want = cluster_want(n, members)
    total = L * (L + 1)
    assert len(want[2]) == total
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, x))
    try:
        got = run(dev, total, r)
        assert_exact(got, want, total, what=f"dtype={dtype} dim={dim} L={L}")
        assert got[3][1] == L and got[3][2] == (members[0] if L else 0)
    finally:
        dev.close()


@pytest.mark.parametrize("dtype,dim", [(1, 3), (0, 2)])
def test_a_segment_beyond_the_limit_sets_the_status_and_the_handle_recovers(nb, dtype, dim):
    L, r = 4097, 0.5
    x, members = cluster_system(dtype, dim, L, r)
    n = len(x)
    want = cluster_want(n, members)
    total = L * (L + 1)
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, x))
    try:
        h = dev.nlist_handle(total)
        h.compute(dev.state(), r, dev.stream)
        summary = h.summary(dev.stream)
        assert summary.tolist() == [total, L, int(members[0]), nb.NeighbourLists.OVER_PER_BODY] and np.array_equal(summary, M.summary(want[0], total))
        assert np.array_equal(h.read(0, dev.stream), want[0]) and np.array_equal(h.read(1, dev.stream), want[1])
        rc, msg = rc_of(nb, lambda: h.read(2, dev.stream))
        assert rc == 3 and "4097" in msg and "NBODY_NLIST_MAX_PER_BODY" in msg, msg
        small = 0.03  # a following compute at a smaller radius on the same handle
        sw = M.brute(x, r=small)
        assert 0 < sw[0].max() <= nb.NeighbourLists.MAX_PER_BODY and len(sw[2]) <= total
        assert_exact(run(dev, total, small), sw, total, what="after the overflow")
    finally:
        dev.close()


# ---- 5. capacity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim", [(1, 3), (0, 2)])
def test_capacity(nb, dtype, dim):
    n = 2049
    rs = radii_of(dim, n)
    refs = reference(dtype, dim, n)
    want, total = refs[1], len(refs[1][2])
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, uniform(dtype, dim, n)))
    try:
        assert_exact(run(dev, total, rs[1]), want, total, what="exactly total")
        h = dev.nlist_handle(total - 1)
        h.compute(dev.state(), rs[1], dev.stream)
        summary = h.summary(dev.stream)
        assert np.array_equal(summary, M.summary(want[0], total - 1)) and summary[3] == nb.NeighbourLists.OVER_CAPACITY
        assert np.array_equal(h.read(0, dev.stream), want[0]) and np.array_equal(h.read(1, dev.stream), want[1])
        rc, msg = rc_of(nb, lambda: h.read(2, dev.stream))
        assert rc == 3 and str(total) in msg and str(total - 1) in msg and "capacity" in msg, msg
        assert_exact(run(dev, total - 1, rs[0]), refs[0], total - 1, what="a smaller radius then fits")  # the status is cleared
        h0 = dev.nlist_handle(0)  # counts only
        h0.compute(dev.state(), rs[1], dev.stream)
        assert np.array_equal(h0.read(0, dev.stream), want[0]) and np.array_equal(h0.read(1, dev.stream), want[1])
        assert np.array_equal(h0.summary(dev.stream), M.summary(want[0], 0))
        assert rc_of(nb, lambda: h0.read(2, dev.stream))[0] == 3
        assert np.array_equal(dev.radius_counts(rs[2]), refs[2][0])
        offset, idx = dev.radius_neighbours(rs[2])  # capacity=None: sized from the counts
        assert np.array_equal(offset, refs[2][1]) and np.array_equal(idx, refs[2][2]) and len(refs[2][2]) in dev._nlist
    finally:
        dev.close()
    assert dev._nlist == {}


# ---- 6. per-body radii ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_per_body_radii_equal_brute_force(nb, dtype, dim, n):
    t = npt(dtype)
    rng = np.random.default_rng(40 + n)
    x = uniform(dtype, dim, n)
    v = (rng.random(n) * 3.0 * n ** (-1.0 / dim)).astype(t)
    v[rng.random(n) < 0.2] = 0
    want = M.brute(x, radii=v)
    total = len(want[2])
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, x))
    try:
        got = run(dev, total, radii=v)
        assert_exact(got, want, total, what=f"radii dtype={dtype} dim={dim} n={n}")
        assert (got[0][v == 0] == 0).all()
        i, j = pairs_of(got[0], got[2])
        assert not np.array_equal(np.sort(i * n + j), np.sort(j * n + i))  # a gather: not symmetric
        assert_exact(run(dev, total, radii=(v * v).astype(t), squared=True), want, total, what="squared")
        # clear_radii: the scalar behaviour again, bit for bit; r is ignored while radii are set
        h = dev.nlist_handle(total)
        h.set_radii(v, False, dev.stream)
        h.compute(dev.state(), 123.0, dev.stream)
        assert all(np.array_equal(a, b) for a, b in zip(h.lists(dev.stream), want))
        r = radii_of(dim, n)[0]
        scalar = M.brute(x, r=r)
        assert len(scalar[2]) <= total
        assert_exact(run(dev, total, r), scalar, total, what="after clear_radii")
        fresh = nb.NeighbourLists(dtype, dim, n, total, dev.device)
        fresh.compute(dev.state(), r, dev.stream)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(fresh.lists(dev.stream), dev.nlist_handle(total).lists(dev.stream)))
        # a bad value is refused, names its index, and leaves the handle as it was (scalar)
        for bad_value, at in ((-1.0, 5), (float("nan"), n - 1), (float("inf"), 0)):
            bad = v.copy()
            bad[at] = bad_value
            rc, msg = rc_of(nb, lambda: fresh.set_radii(bad, False, dev.stream))
            assert rc == 1 and f"index {at}" in msg, msg
        bad = v.copy()
        bad[7] = -0.5
        rc, msg = rc_of(nb, lambda: fresh.set_radii(bad, True, dev.stream))
        assert rc == 1 and "index 7" in msg, msg
        assert rc_of(nb, lambda: fresh.set_radii(v[:-1], False, dev.stream))[0] == 1  # n - 1 values
        fresh.compute(dev.state(), r, dev.stream)
        assert all(np.array_equal(a, b) for a, b in zip(fresh.lists(dev.stream), scalar))
        fresh.close()
    finally:
        dev.close()


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("dtype,dim", [(1, 3), (0, 3), (0, 2)])
def test_squared_radii_from_the_kth_neighbour(nb, dtype, dim, k):
    """r2_i = body i's own k-th squared distance from the tree kNN: L_i is exactly {j : d2_ij <= d2_ik}, and holds row i of the kNN
    index array (more only where a distance ties with the k-th)."""
    n = 2049
    x = uniform(dtype, dim, n)
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, x))
    try:
        kidx, kd2 = dev.knn(k, method="tree")
        r2 = np.ascontiguousarray(kd2[:, k - 1])
        want = M.brute(x, radii=r2, squared=True)
        total = len(want[2])
        got = run(dev, total, radii=r2, squared=True)
        assert_exact(got, want, total, what=f"kNN radii dtype={dtype} dim={dim} k={k}")
        count, offset, idx, _ = got
        assert (count >= k).all()
        for i in range(n):
            seg = idx[int(offset[i]):int(offset[i + 1])]
            assert np.isin(kidx[i], seg).all(), i
            assert (pair_d2(x[seg], x[i]) <= r2[i]).all()
        assert np.array_equal(dev.radius_counts(radii=r2, squared=True), count)
    finally:
        dev.close()


# ---- 7. against friends-of-friends ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, BIG])
@pytest.mark.parametrize("dtype,dim", [(1, 3), (0, 2)])
def test_the_components_of_the_list_graph_are_the_fof_groups(nb, dtype, dim, n):
    r = 0.9 * n ** (-1.0 / dim)
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, uniform(dtype, dim, n)))
    try:
        want = M.cell_list(uniform(dtype, dim, n), r)
        total = len(want[2])
        count, offset, idx, _ = got = run(dev, total, r)
        assert_exact(got, want, total, what=f"dtype={dtype} dim={dim} n={n}")
        label, size = labels_from_edges(n, *pairs_of(count, idx))
        flabel, fsize = dev.fof(r)
        assert np.array_equal(label, flabel) and np.array_equal(size, fsize)
        assert 1 < len(np.unique(label)) < n
    finally:
        dev.close()


# ---- 8. degenerate inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_degenerate_inputs(nb, dtype, dim):
    t = npt(dtype)
    rng = np.random.default_rng(21)
    sites = rng.random((40, dim)).astype(t)
    site = rng.integers(0, 40, 700)
    x = sites[site]  # coincident and duplicated bodies, r = 0: exactly the other bodies of a site
    flat = rng.random((700, dim)).astype(t)
    flat[:, dim - 1] = t(0.25)  # a constant axis: zero key bits on it, boxes of zero extent
    blob = np.concatenate([rng.normal(0, 0.01, (300, dim)), np.full((1, dim), 1000.0)]).astype(t)  # a cluster with one far body
    blob = blob[rng.permutation(len(blob))]
    for name, pts, rs in (("coincident", x, [0.0]), ("constant axis", flat, [0.05, 0.0]), ("cluster and a far body", blob, [0.01, 2000.0])):
        dev = nb.DeviceSystem.from_host(system_of(nb, dtype, pts))
        try:
            for r, want in zip(rs, M.brute_many(pts, rs)):
                total = len(want[2])
                got = run(dev, total, r)
                assert_exact(got, want, total, what=f"{name} dtype={dtype} dim={dim} r={r}")
                if name == "coincident":
                    assert np.array_equal(got[0], np.bincount(site, minlength=40)[site] - 1)
                if name == "cluster and a far body" and r == 2000.0:
                    assert (got[0] == len(blob) - 1).all()
        finally:
            dev.close()


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_one_body(nb, dtype, dim):
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, np.full((1, dim), 0.5)))
    try:
        for capacity in (0, 7):
            count, offset, idx, summary = run(dev, capacity, 1.0)
            assert count.tolist() == [0] and offset.tolist() == [0, 0] and len(idx) == 0 and summary.tolist() == [0, 0, 0, 0]
            L = nb.lib()
            assert L.nbody_nlist_read(dev.nlist_handle(capacity).h, 2, None, 0, dev.stream) == 0  # bytes = 0: host_out may be NULL
            assert L.nbody_nlist_read(dev.nlist_handle(capacity).h, 2, None, 4, dev.stream) == 1 and b"needs 0 bytes" in L.nbody_last_error()
    finally:
        dev.close()


# ---- 9. repeats, handles, a replayed graph, the call sequence -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
def test_repeats_handles_and_a_replayed_graph_give_the_same_bits(nb, dtype):
    n, dim = 4097, 3
    r = radii_of(dim, n)[1]
    want = reference(dtype, dim, n)[1]
    total = len(want[2])
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, uniform(dtype, dim, n)))

    def read_all(capacity=total):
        h = dev.nlist_handle(capacity)
        return tuple(a.tobytes() for a in h.lists(dev.stream)) + (h.summary(dev.stream).tobytes(),)

    dev.nlist_compute(r, total)
    first = read_all()
    assert first[:3] == tuple(a.tobytes() for a in want)
    dev.nlist_compute(r, total)  # a repeated compute
    assert read_all() == first
    dev._nlist.pop(total).close()  # a new handle on the same system
    dev.nlist_compute(r, total)
    assert read_all() == first
    dev.nlist_compute(r, total + 100)  # two handles alive at once
    assert read_all(total + 100) == first and read_all() == first
    assert dev.nlist_handle(total) is not dev.nlist_handle(total + 100) and sorted(dev._nlist) == [total, total + 100]
    # recorded and replayed; the handle's arrays are overwritten in between so that the replay has to produce them
    g = nb.StepGraph(dev, lambda: dev.nlist_compute(r, total))
    dev.nlist_handle(total).compute(dev.state(), 0.0, dev.stream)
    assert read_all() != first
    g.launch()
    assert read_all() == first
    g.launch()
    assert read_all() == first
    g.close()
    dev.close()
    assert dev._nlist == {}


def test_call_sequence(nb):
    dev = nb.DeviceSystem.from_host(system_of(nb, 1, uniform(1, 3, 257)))
    st = dev.state()
    h = nb.NeighbourLists(1, 3, 257, 1000, dev.device)
    for what in range(3):
        assert rc_of(nb, lambda: h.read(what, dev.stream))[0] == 3  # NBODY_ERR_STATE before the first compute
    assert rc_of(nb, lambda: h.summary(dev.stream))[0] == 3
    for other in (nb.NeighbourLists(1, 3, 258, 0, dev.device), nb.NeighbourLists(0, 3, 257, 0, dev.device), nb.NeighbourLists(1, 2, 257, 0, dev.device)):
        rc, msg = rc_of(nb, lambda: other.compute(st, 0.1, dev.stream))
        assert rc == 1 and "was created for" in msg
        other.close()
    for bad in (-1.0, float("nan"), float("inf"), 1e200):
        rc, msg = rc_of(nb, lambda: h.compute(st, bad, dev.stream))
        assert rc == 1 and "radius" in msg, (bad, msg)
    h.set_radii(np.full(257, 0.1), False, dev.stream)  # before the first compute; r is then ignored, whatever it is
    h.compute(st, float("nan"), dev.stream)
    want = M.brute(uniform(1, 3, 257), r=0.1)
    assert all(np.array_equal(a, b) for a, b in zip(h.lists(dev.stream), want))
    h.clear_radii(dev.stream)
    h.compute(st, 0.0, dev.stream)  # legal: nothing is coincident here
    assert (h.read(0, dev.stream) == 0).all() and h.summary(dev.stream).tolist() == [0, 0, 0, 0] and len(h.read(2, dev.stream)) == 0
    L = nb.lib()
    buf = np.zeros(600, np.uint32)
    assert L.nbody_nlist_read(h.h, 0, buf.ctypes.data, 4 * 256, dev.stream) == 1 and b"needs 1028 bytes" in L.nbody_last_error()
    assert L.nbody_nlist_read(h.h, 1, buf.ctypes.data, 8 * 257, dev.stream) == 1 and b"needs 2064 bytes" in L.nbody_last_error()
    assert L.nbody_nlist_read(h.h, 2, buf.ctypes.data, 4, dev.stream) == 1 and b"0 entries" in L.nbody_last_error()
    # between graph begin and end the blocking calls are refused and the capture stays usable
    seen = []

    def record():
        dev.nlist_compute(0.1, 1000)
        hh = dev.nlist_handle(1000)
        seen.append(rc_of(nb, lambda: hh.summary(dev.stream))[0])
        seen.append(rc_of(nb, lambda: hh.read(0, dev.stream))[0])
        seen.append(rc_of(nb, lambda: hh.set_radii(np.full(257, 0.1), False, dev.stream))[0])
        seen.append(rc_of(nb, lambda: nb.NeighbourLists(1, 3, 257, 0, dev.device))[0])

    dev.nlist_handle(1000)  # made before the recording
    g = nb.StepGraph(dev, record)
    assert seen == [3, 3, 3, 3]
    g.launch()
    assert all(np.array_equal(a, b) for a, b in zip(dev.nlist_handle(1000).lists(dev.stream), want))
    g.close()
    h.close()
    dev.close()


# ---- 10. the product's models ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["plummer", "galaxy"])
@pytest.mark.parametrize("dtype", [1, 0])
def test_plummer_and_galaxy_equal_the_cell_list(nb, dtype, model):
    n = 8192
    hs = nb.build_model(dtype, 3, model, n)
    x = np.array(hs.x)
    dev = nb.DeviceSystem.from_host(hs)
    try:
        _, d2 = dev.knn(6, method="tree")
        r = float(np.median(np.sqrt(d2[:, 5].astype(np.float64))))  # the median distance to the sixth neighbour
        want = M.cell_list(x, r)
        total = len(want[2])
        assert 3 * n <= total and want[0].max() <= nb.NeighbourLists.MAX_PER_BODY
        assert_exact(run(dev, total, r), want, total, what=f"{model} dtype={dtype}")
    finally:
        dev.close()


# ---- 11. CLI --------------------------------------------------------------------------------------------------------------------------------
def cli(dim, args, cwd):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", f"nbody_hip_d{dim}")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("prec,extra", [("double", ["--algorithm", "all-pairs"]), ("float", [])], ids=["double-all_pairs", "float-default_octree"])
def test_cli_save_lists(nb, prec, extra):
    """-n 1000 -s 1 --csv-detailed --save pos --save-lists R: two frames; lists.bin has the stated header, every frame equals the
    binding's outputs on that frame's saved positions byte for byte, and positions.bin is what a run without the flag writes.  A
    second run with --lists-capacity one below the larger frame's total: that frame has the status set and no list."""
    dtype = 1 if prec == "double" else 0
    n, dim, tsz = 1000, 3, 4 if dtype == 0 else 8
    base = ["-n", n, "-s", 1, "--csv-detailed", "--precision", prec, "--save", "pos"] + extra
    with tempfile.TemporaryDirectory() as d, tempfile.TemporaryDirectory() as d0, tempfile.TemporaryDirectory() as d1:
        r0 = cli(dim, base, d0)
        assert r0.returncode == 0, r0.stderr
        praw = open(os.path.join(d0, "positions.bin"), "rb").read()
        nframes = (len(praw) - 16) // (n * dim * tsz)
        assert nframes == 2
        frames = np.frombuffer(praw, npt(dtype), nframes * n * dim, 16).reshape(nframes, n, dim)
        r = 1.5 * float(np.prod(frames[0].max(0) - frames[0].min(0)) / n) ** (1.0 / dim)  # 1.5 times the mean spacing of the first frame
        run1 = cli(dim, base + ["--save-lists", repr(r)], d)
        assert run1.returncode == 0, run1.stderr
        assert open(os.path.join(d, "positions.bin"), "rb").read() == praw
        assert not os.path.exists(os.path.join(d0, "lists.bin"))
        raw = open(os.path.join(d, "lists.bin"), "rb").read()
        hs = nb.build_model(dtype, dim, "uniform", n)

        def expect(capacity):
            want, totals = struct.pack("<4IdQ", n, 1, tsz, dim, r, capacity), []
            for f in range(nframes):
                hs.x[:] = frames[f]
                dev = nb.DeviceSystem.from_host(hs)
                try:
                    h = dev.nlist_handle(capacity)
                    h.compute(dev.state(), r, dev.stream)
                    summary = h.summary(dev.stream)
                    want += summary.tobytes() + h.read(0, dev.stream).tobytes()
                    if summary[3] == 0:
                        want += h.read(2, dev.stream).tobytes()
                    totals.append((int(summary[0]), int(summary[3])))
                finally:
                    dev.close()
            return want, totals

        want, totals = expect(64 * n)
        assert raw == want and all(t > n and s == 0 for t, s in totals), totals
        tight = max(t for t, _ in totals) - 1
        run2 = cli(dim, base + ["--save-lists", repr(r), "--lists-capacity", tight], d1)
        assert run2.returncode == 0, run2.stderr
        want2, totals2 = expect(tight)
        assert open(os.path.join(d1, "lists.bin"), "rb").read() == want2
        assert any(s == nb.NeighbourLists.OVER_CAPACITY for _, s in totals2), totals2
