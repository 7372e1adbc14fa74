"""GPU: every handle class is created, used once so that its buffers are touched, and closed twice; the parts allocated after create
(block steps of the Hermite integrators, counters, the quadrupole pool) go the same way; a DeviceSystem closes every handle it cached.
The buffers of a handle are owned by a device_buffers (csrc/device_buffers.hpp) whose bookkeeping is proved on the CPU
(tests/test_device_buffers.py); what runs here shows that the handles hand it every buffer they use and survive their own teardown.
Small on purpose: n = 64, k = 4."""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K = 64, 4
THETA, EPS, ETA = 0.5, 0.05, 0.02
CASES = [(1, 3), (0, 2)]  # (dtype, dim): double 3D, float 2D
IDS = ["f64-3d", "f32-2d"]


def system(nb, dtype, dim, n=N, seed=7):
    rng = np.random.default_rng(seed + n)
    t = nb.np_dtype(dtype)
    hs = nb.HostSystem(dtype, dim, n)
    hs.m[:] = rng.uniform(0.5, 1.5, n).astype(t) / n
    hs.x[:] = rng.normal(0, 1, (n, dim)).astype(t)
    hs.v[:] = rng.normal(0, 0.3, (n, dim)).astype(t)
    hs.dt, hs.c = 0.01, 1.0
    return nb.DeviceSystem.from_host(hs)


def closed_twice(h):
    assert h.h
    h.close()
    assert not h.h
    h.close()
    assert not h.h


def finite_accelerations(dev):
    a = dev.download().a
    assert np.isfinite(a).all() and np.abs(a).max() > 0


def use_bvh(nb, dev, late):
    b = nb.Bvh(dev.dtype, dev.dim, dev.n, dev.device)
    st = dev.state()
    if late:
        b.enable_counters()
    b.bounding_box(st, dev.stream)
    b.hilbert_sort(st, dev.stream)
    b.build_tree(st, dev.stream)
    b.compute_force(st, THETA, dev.stream)
    finite_accelerations(dev)
    if late:
        assert b.read(5, dev.stream).sum() > 0  # the walk counted into the handle's array
    return [b]


def use_octree(nb, dev, late):
    t = nb.Octree(dev.dtype, dev.dim, dev.n, dev.device)
    st = dev.state()
    if late:
        t.enable_counters()
    t.clear(dev.stream)
    t.compute_bounds(st, dev.stream)
    t.insert(st, dev.stream)
    t.compute_tree(dev.stream)
    t.compute_force(st, THETA, dev.stream)
    finite_accelerations(dev)
    if late:
        assert t.read_counters(dev.stream).sum() > 0  # the walk counted into the handle's array
        t.compute_quadrupoles(dev.stream)
        t.compute_quadrupoles(dev.stream)  # the pool is there: nothing is allocated twice
        t.compute_quadrupole_force(st, THETA, dev.stream)
        finite_accelerations(dev)
        assert np.isfinite(t.read_root_quadrupole(dev.stream)).all()
    return [t]


def use_hermite(nb, dev, late):
    h = nb.Hermite(dev.dtype, dev.dim, dev.n, dev.device)
    h.force_jerk(dev.state(), EPS, dev.stream)
    if late:
        h.block_start(dev.state(), EPS, 0.01, 6, dev.stream)
        h.block_start(dev.state(), EPS, 0.01, 6, dev.stream)  # the block part is there: nothing is allocated twice
        n_act, tau = h.block_step(dev.state(), EPS, ETA, dev.stream)
        assert 1 <= n_act <= dev.n and tau >= 1
    finite_accelerations(dev)
    assert np.isfinite(h.read(0, dev.stream)).all()
    return [h]


def use_hermite6(nb, dev, late):
    h = nb.Hermite6(dev.dtype, dev.dim, dev.n, dev.device)
    h.start(dev.state(), EPS, dev.stream)
    if late:  # double only
        h.block_start(dev.state(), EPS, 0.01, 6, dev.stream)
        n_act, tau = h.block_step(dev.state(), EPS, ETA, dev.stream)
        assert 1 <= n_act <= dev.n and tau >= 1
    finite_accelerations(dev)
    assert np.isfinite(h.read(1, dev.stream)).all()
    return [h]


def use_neighbours(nb, dev, late):
    h = nb.Neighbours(dev.dtype, dev.dim, dev.n, dev.device)
    h.compute(dev.state(), EPS, dev.stream)
    assert (h.read(1, dev.stream) < dev.n).all()
    i, j, d2 = h.closest_pair(dev.stream)
    assert i < j < dev.n and d2 > 0
    return [h]


def use_knn(method):
    def use(nb, dev, late):
        h = nb.Knn(dev.dtype, dev.dim, dev.n, K, dev.device, method)
        assert h.method == method
        h.compute(dev.state(), dev.stream)
        assert (h.read(0, dev.stream) < dev.n).all() and (h.read(2, dev.stream) > 0).all()
        return [h]
    return use


def use_octree_block(nb, dev, late):
    t = nb.Octree(dev.dtype, dev.dim, dev.n, dev.device)
    h = nb.OctreeBlock(dev.dtype, dev.dim, dev.n, dev.device)
    h.start(t, dev.state(), THETA, EPS, ETA, 6, dev.stream)
    n_act, tau = h.step(t, dev.state(), THETA, EPS, ETA, dev.stream)
    assert 1 <= n_act <= dev.n and tau >= 1
    finite_accelerations(dev)
    return [h, t]


def use_step_graph(nb, dev, late):
    dev.all_pairs_force()  # outside the recording first: a recorded step never allocates
    g = nb.StepGraph(dev, dev.all_pairs_force)
    g.launch()
    finite_accelerations(dev)
    return [g]


USES = {"bvh": use_bvh, "octree": use_octree, "hermite": use_hermite, "hermite6": use_hermite6, "neighbours": use_neighbours,
        "knn-all-pairs": use_knn("all-pairs"), "knn-tree": use_knn("tree"), "octree-block": use_octree_block, "step-graph": use_step_graph}
LATE = {"bvh": CASES, "octree": CASES, "hermite": CASES, "hermite6": CASES[:1]}  # the handles with a part allocated after create


@pytest.mark.parametrize("dtype, dim", CASES, ids=IDS)
@pytest.mark.parametrize("what", sorted(USES))
def test_create_use_close_twice(nb, what, dtype, dim):
    dev = system(nb, dtype, dim)
    handles = USES[what](nb, dev, False)
    dev.sync()
    for h in handles:
        closed_twice(h)
    dev.all_pairs_force()  # the context is unharmed by its neighbours' teardown
    finite_accelerations(dev)
    closed_twice(dev)


@pytest.mark.parametrize("what, dtype, dim", [(w, *c) for w in sorted(LATE) for c in LATE[w]])
def test_parts_allocated_after_create_close_with_the_handle(nb, what, dtype, dim):
    dev = system(nb, dtype, dim)
    handles = USES[what](nb, dev, True)
    dev.sync()
    for h in handles:
        closed_twice(h)
    closed_twice(dev)


@pytest.mark.parametrize("dtype, dim", CASES, ids=IDS)
def test_device_system_closes_every_cached_handle(nb, dtype, dim):
    dev = system(nb, dtype, dim)
    dev.bvh_force(THETA)
    dev.octree_force(THETA)
    dev.hermite_start(EPS)
    dev.neighbours(EPS)
    for method in ("all-pairs", "tree"):
        idx, d2 = dev.knn(K, method)
        assert idx.shape == (N, K) and (idx < N).all()
    cached = [dev.bvh, dev.octree, dev.hermite, dev.neighbours_handle, dev.knn_handle(K), dev.knn_handle(K, "tree")]
    assert all(h.h for h in cached) and dev.h
    for _ in range(2):
        dev.close()
        assert not dev.h
        assert all(not h.h for h in cached)
        assert all(getattr(dev, a) is None for a in dev._CACHED) and dev._knn == {} and dev._knn_other == {}


def test_two_hundred_tree_knn_handles_come_and_go(nb):
    """A leak large enough to matter would end this in an allocation error; the results after it are those from before it."""
    n = 4096
    dev = system(nb, 1, 3, n)
    before = nb.Knn(1, 3, n, K, dev.device, "tree")
    before.compute(dev.state(), dev.stream)
    want = [before.read(w, dev.stream) for w in (0, 1, 2)]
    for _ in range(200):
        nb.Knn(1, 3, n, K, dev.device, "tree").close()
    after = nb.Knn(1, 3, n, K, dev.device, "tree")
    after.compute(dev.state(), dev.stream)
    for w in (0, 1, 2):
        got = after.read(w, dev.stream)
        assert got.tobytes() == want[w].tobytes(), w
        assert before.read(w, dev.stream).tobytes() == want[w].tobytes(), w  # the old handle's buffers were nobody else's
    for h in (before, after, dev):
        closed_twice(h)


@pytest.mark.parametrize("api", ["nbody_bvh_create_on", "nbody_octree_create_on", "nbody_create"])
def test_tree_and_context_create_check_the_device_last(nb, api):
    """After out, dtype, dim and n: the device, which needs the runtime.  The context takes no -1 for "the current device"."""
    L = nb.lib()
    create = getattr(L, api)
    err = lambda: L.nbody_last_error().decode()
    visible = r" out of range \(\d+ HIP devices visible\)"
    h = ctypes.c_void_p(0x1000)
    assert create(ctypes.byref(h), nb.F64, 3, ctypes.c_uint32(N), 99) == 1
    assert re.fullmatch("device 99" + visible, err()) and h.value is None
    assert create(ctypes.byref(h), nb.F64, 4, ctypes.c_uint32(N), 99) == 1 and err() == "bad dim 4"  # an argument error wins
    if api == "nbody_create":
        assert create(ctypes.byref(h), nb.F64, 3, ctypes.c_uint32(N), -1) == 1
        assert re.fullmatch("device -1" + visible, err()) and h.value is None
