"""GPU: friends-of-friends groups (nbody_fof_*, csrc/fof.inc) against references in the same T arithmetic, EXACTLY.  label and size are
integers with one correct answer — the friend test is d2 <= b2 on pair_d2's own chain, which tests/fof_model.py emulates bit for bit —
so no tolerance is involved anywhere but in the catalogue's mass and centre of mass, whose bound is derived below.

Sizes: 32 records a bucket, 64 targets a wave, 256 lanes a block, the hierarchy padded to a power of two of buckets — so 31 | 32 | 33,
63 | 64 | 65, 127 .. 129, 255 .. 257, the sort's one-block form up to 2048 and the splitter form beyond (2047, 2049, 4097, 65 537)."""
import functools
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import fof_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025, 2047, 2049, 4097]
CS = (0.5, 0.9, 1.4)  # b = c n^(-1/D): mostly singletons, many mid-sized groups, a percolating group
BIG = 65537
LD = np.longdouble


def npt(dtype):
    return np.float64 if dtype == 1 else np.float32


def system_of(nb, dtype, x, m=None):
    n, dim = x.shape
    hs = nb.HostSystem(dtype, dim, n)
    hs.x[:] = x.astype(npt(dtype))
    hs.m[:] = (np.random.default_rng(n).uniform(0.5, 1.5, n) / n if m is None else m).astype(npt(dtype))
    hs.dt, hs.c = 0.01, 1.0
    return hs


@functools.lru_cache(maxsize=None)
def uniform(dtype, dim, n):
    x = np.random.default_rng(500 + n).random((n, dim)).astype(npt(dtype))
    x.setflags(write=False)
    return x


def linking_lengths(dim, n):
    return [c * n ** (-1.0 / dim) for c in CS]


@functools.lru_cache(maxsize=None)
def reference(dtype, dim, n):
    """[(label, size)] of uniform(dtype, dim, n) at the three linking lengths: brute force, computed once and shared."""
    return M.brute_many(uniform(dtype, dim, n), linking_lengths(dim, n))


def run(dev, b, min_members=1):
    h = dev.fof_handle(min_members)
    h.compute(dev.state(), b, dev.stream)
    return h.read(0, dev.stream), h.read(1, dev.stream), h.summary(dev.stream)


def assert_exact(got, want_label, want_size, min_members=1, what=""):
    label, size, summary = got
    assert label.dtype == np.uint32 and size.dtype == np.uint32 and summary.dtype == np.uint32
    bad = np.nonzero(label != want_label)[0]
    assert len(bad) == 0, f"{what}: label differs at {len(bad)} bodies, first {bad[:4].tolist()}: {label[bad[:4]].tolist()} != {want_label[bad[:4]].tolist()}"
    bad = np.nonzero(size != want_size)[0]
    assert len(bad) == 0, f"{what}: size differs at {len(bad)} bodies, first {bad[:4].tolist()}"
    assert np.array_equal(summary, M.summary(want_label, want_size, min_members)), (what, summary)


# ---- 1. random uniform systems ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_random_systems_equal_brute_force(nb, dtype, dim, n):
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, uniform(dtype, dim, n)))
    try:
        for b, (want_label, want_size) in zip(linking_lengths(dim, n), reference(dtype, dim, n)):
            assert_exact(run(dev, b), want_label, want_size, what=f"dtype={dtype} dim={dim} n={n} b={b}")
    finally:
        dev.close()


# ---- 2. one large random size (the splitter sort; a cell-list reference) ----------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim", [(0, 3), (1, 3), (0, 2), (1, 2)])
def test_one_large_size_equals_the_cell_list(nb, dtype, dim):
    x = uniform(dtype, dim, BIG)
    b = 0.9 * BIG ** (-1.0 / dim)
    want_label, want_size = M.cell_list(x, b)
    assert 1 < len(np.unique(want_label)) < BIG and want_size.max() > 20
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, x))
    try:
        assert_exact(run(dev, b), want_label, want_size, what=f"dtype={dtype} dim={dim} n={BIG}")
    finally:
        dev.close()


# ---- 3. a chain: the deepest case for hooking and path halving ------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_chain(nb, dtype, dim):
    t = npt(dtype)
    n = BIG
    x = np.zeros((n, dim), t)
    x[:, 0] = np.random.default_rng(9).permutation(n)  # spacing exactly 1, indices shuffled: every d2 of neighbours is exactly 1
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, x))
    try:
        label, size, summary = run(dev, 1.0)
        assert (label == 0).all() and (size == n).all() and list(summary) == [1, 1, n, 0]
        label, size, summary = run(dev, float(np.nextafter(t(1), t(0))))  # one ulp of T below: T(b) is that value, b2 < 1
        assert np.array_equal(label, np.arange(n)) and (size == 1).all() and list(summary) == [n, n, 1, 0]
    finally:
        dev.close()


# ---- 4. an integer lattice with gaps: b2 and every d2 are exact ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(dim):
    side = 16 if dim == 3 else 64
    g = np.stack(np.meshgrid(*([np.arange(side)] * dim), indexing="ij"), -1).reshape(-1, dim)
    g = g[g[:, 0] % 5 != 4]  # every fifth plane removed: b = 1 leaves slabs, b = 2 bridges the gaps
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def lattice_reference(dim, r2):
    """Integer grid union-find: bodies whose integer squared distance is <= r2 are friends."""
    g = lattice(dim)
    side = int(g.max()) + 1
    index = -np.ones((side + 4,) * dim, np.int64)
    index[tuple((g + 2).T)] = np.arange(len(g))
    reach = int(np.floor(np.sqrt(r2)))
    offs = np.stack(np.meshgrid(*([np.arange(-reach, reach + 1)] * dim), indexing="ij"), -1).reshape(-1, dim)
    offs = offs[((offs**2).sum(1) <= r2) & ((offs**2).sum(1) > 0)]
    ei, ej = [], []
    for off in offs:
        j = index[tuple((g + 2 + off).T)]
        ok = j >= 0
        ei.append(np.nonzero(ok)[0])
        ej.append(j[ok])
    return M.labels_from_edges(len(g), np.concatenate(ei) if ei else [], np.concatenate(ej) if ej else [])


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_lattice_in_three_orders(nb, dtype, dim):
    t = npt(dtype)
    g = lattice(dim)
    n = len(g)
    orders = [np.arange(n), np.arange(n)[::-1].copy(), np.random.default_rng(4).permutation(n)]
    cases = [(1.0, 1), (2.0, 4), (float(np.nextafter(t(1), t(0))), 0)]
    for order in orders:  # body k of this system is lattice point order[k]
        dev = nb.DeviceSystem.from_host(system_of(nb, dtype, g[order].astype(t)))
        try:
            for b, r2 in cases:
                canon_label, canon_size = lattice_reference(dim, r2)
                lowest = np.full(n, n, np.int64)  # per canonical group: the lowest index its members have in THIS order
                np.minimum.at(lowest, canon_label[order], np.arange(n))
                want_label = lowest[canon_label[order]].astype(np.uint32)
                assert_exact(run(dev, b), want_label, canon_size[order], what=f"dtype={dtype} dim={dim} b={b}")
        finally:
            dev.close()
    groups = len(np.unique(lattice_reference(dim, 1)[0]))
    assert groups == (4 if dim == 3 else 13) and len(np.unique(lattice_reference(dim, 4)[0])) == 1  # slabs, then one bridged group


# ---- 5. degenerate inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_degenerate_inputs(nb, dtype, dim):
    t = npt(dtype)
    rng = np.random.default_rng(21)
    # coincident and duplicated bodies, b = 0: exactly the bodies of a site are a group
    sites = rng.random((40, dim)).astype(t)
    site = rng.integers(0, 40, 700)
    x = sites[site]
    # a constant axis: zero key bits on it, boxes of zero extent
    flat = rng.random((700, dim)).astype(t)
    flat[:, dim - 1] = t(0.25)
    # two blobs and one far body
    blobs = np.concatenate([rng.normal(0, 0.01, (300, dim)), rng.normal(0, 0.01, (300, dim)) + 10.0, np.full((1, dim), 1000.0)]).astype(t)
    blobs = blobs[rng.permutation(len(blobs))]
    for name, pts, bs in (("coincident", x, [0.0]), ("constant axis", flat, [0.9 * 700 ** (-1.0 / (dim - 1)) if dim == 3 else 1e-3, 0.0]),
                          ("blobs", blobs, [1.0]), ("one group", flat, [10.0])):
        dev = nb.DeviceSystem.from_host(system_of(nb, dtype, pts))
        try:
            for b, (want_label, want_size) in zip(bs, M.brute_many(pts, bs)):
                got = run(dev, b)
                assert_exact(got, want_label, want_size, what=f"{name} dtype={dtype} dim={dim} b={b}")
                if name == "coincident":
                    assert got[2][0] == len(np.unique(site))
                if name == "blobs":
                    assert list(np.sort(np.unique(got[1]))) == [1, 300] and got[2][0] == 3
                if name == "one group":
                    assert (got[0] == 0).all() and list(got[2]) == [1, 1, 700, 0]
        finally:
            dev.close()


# ---- 6. the catalogue -----------------------------------------------------------------------------------------------------------------------
def gamma(k):
    """k u / (1 - k u), u = 2^-53: the relative error bound of k roundings in double (Higham)."""
    u = LD(2.0) ** -53
    return k * u / (1 - k * u)


@pytest.mark.parametrize("min_members", [1, 2, 20])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [1, 0])
def test_catalogue(nb, dtype, dim, min_members):
    """Entries, their order and c exactly.  Mass and centre of mass against NumPy longdouble: the kernel adds `size` terms in double in
    SOME fixed order and every product m x is rounded once, so sum(m x) is within gamma(size + 1) sum|m x| of the exact value and
    sum(m) within gamma(size) sum(m) (the masses are positive); the quotient adds one rounding, and sum|m x| / sum(m) >= |com|, so
    |com - ref| <= 3 gamma(size + 2) sum|m x| / sum(m), plus one rounding to T (u_T |com|).  Nothing here is tuned."""
    n = 4097
    t = npt(dtype)
    x = uniform(dtype, dim, n)
    hs = system_of(nb, dtype, x)
    m = np.array(hs.m, t)
    u_t = LD(2.0) ** (-53 if dtype == 1 else -24)
    dev = nb.DeviceSystem.from_host(hs)
    try:
        for b, (want_label, want_size) in zip(linking_lengths(dim, n), reference(dtype, dim, n)):
            want = M.catalogue(want_label, want_size, m, x, min_members)
            cat, summary = dev.fof_groups(b, min_members)
            assert np.array_equal(summary, M.summary(want_label, want_size, min_members))
            c = int(summary[1])
            assert c == len(want["label"]) and (min_members > 1 or c == summary[0])
            assert cat["label"].dtype == np.uint32 and np.array_equal(cat["label"], want["label"])
            assert cat["size"].dtype == np.uint32 and np.array_equal(cat["size"], want["size"])
            assert (np.diff(cat["label"].astype(np.int64)) > 0).all()
            assert cat["mass"].shape == (c,) and cat["com"].shape == (c, dim) and cat["mass"].dtype == t and cat["com"].dtype == t
            s = want["size"].astype(LD)
            mass_tol = (gamma(s) + u_t) * want["mass"]
            com_tol = 3 * gamma(s + 2)[:, None] * want["sum_abs_mx"] / want["mass"][:, None] + u_t * np.abs(want["com"])
            mass_err, com_err = np.abs(cat["mass"].astype(LD) - want["mass"]), np.abs(cat["com"].astype(LD) - want["com"])
            print(f"dtype={dtype} dim={dim} min={min_members} b={b:.4g}: c={c}, worst mass err / tol {float((mass_err / mass_tol).max()) if c else 0:.3f}, "
                  f"worst com err / tol {float((com_err / com_tol).max()) if c else 0:.3f}")
            assert (mass_err <= mass_tol).all() and (com_err <= com_tol).all()
            again, _ = dev.fof_groups(b, min_members)  # the bits of a second compute
            for k in ("label", "size", "mass", "com"):
                assert again[k].tobytes() == cat[k].tobytes(), k
    finally:
        dev.close()


# ---- 7. repeats and handles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
def test_repeats_handles_and_a_replayed_graph_give_the_same_bits(nb, dtype):
    n, dim = 4097, 3
    b = linking_lengths(dim, n)[1]
    want_label, want_size = reference(dtype, dim, n)[1]
    dev = nb.DeviceSystem.from_host(system_of(nb, dtype, uniform(dtype, dim, n)))

    def read_all(min_members=1):
        h = dev.fof_handle(min_members)
        return h.read(0, dev.stream).tobytes(), h.read(1, dev.stream).tobytes()

    dev.fof_compute(b)
    first = read_all()
    assert first == (want_label.tobytes(), want_size.tobytes())
    dev.fof_compute(b)  # a repeated compute
    assert read_all() == first
    dev._fof.pop(1).close()  # a new handle on the same system
    dev.fof_compute(b)
    assert read_all() == first
    dev.fof_compute(b, 20)  # two handles with different min_members on one system
    assert read_all(20) == first and read_all() == first
    assert dev.fof_handle(20) is not dev.fof_handle(1) and sorted(dev._fof) == [1, 20]
    summary1, summary20 = dev.fof_handle(1).summary(dev.stream), dev.fof_handle(20).summary(dev.stream)
    assert summary1[0] == summary20[0] and summary1[1] == summary1[0] and summary20[1] == (want_size[want_label == np.arange(n)] >= 20).sum()
    # recorded and replayed; the handle's arrays are overwritten in between so that the replay has to produce them
    g = nb.StepGraph(dev, lambda: dev.fof_compute(b))
    dev.fof_handle(1).compute(dev.state(), 0.0, dev.stream)
    assert read_all() != first
    g.launch()
    assert read_all() == first
    g.launch()
    assert read_all() == first and np.array_equal(dev.fof_handle(1).summary(dev.stream), summary1)
    g.close()
    dev.close()
    assert dev._fof == {}


def test_call_sequence(nb):
    import re
    hs = system_of(nb, 1, uniform(1, 3, 257))
    dev = nb.DeviceSystem.from_host(hs)
    st = dev.state()

    def rc_of(call):
        try:
            call()
        except nb.NbodyError as e:
            return int(re.match(r"nbody backend error (\d+)", str(e)).group(1)), str(e)
        return 0, ""

    h = nb.Fof(1, 3, 257, 2, dev.device)
    for what in range(2):
        assert rc_of(lambda: h.read(what, dev.stream))[0] == 3  # NBODY_ERR_STATE before the first compute
    assert rc_of(lambda: h.summary(dev.stream))[0] == 3
    for other in (nb.Fof(1, 3, 258, 1, dev.device), nb.Fof(0, 3, 257, 1, dev.device), nb.Fof(1, 2, 257, 1, dev.device)):
        rc, msg = rc_of(lambda: other.compute(st, 0.1, dev.stream))
        assert rc == 1 and "was created for" in msg
        other.close()
    for bad in (-1.0, float("nan"), float("inf"), 1e200):
        rc, msg = rc_of(lambda: h.compute(st, bad, dev.stream))
        assert rc == 1 and "linking length" in msg, (bad, msg)
    hf = nb.Fof(0, 3, 257, 1, dev.device)  # a float handle: b beyond float's range, and b whose square is (1e200, 1e30)
    devf = nb.DeviceSystem.from_host(system_of(nb, 0, uniform(0, 3, 257)))
    for bad in (1e200, 1e39, 1e30, -0.5):
        rc, msg = rc_of(lambda: hf.compute(devf.state(), bad, devf.stream))
        assert rc == 1 and "linking length" in msg, (bad, msg)
    hf.compute(devf.state(), 1e19, devf.stream)  # b2 = 1e38 is finite in float: one group
    assert (hf.read(0, devf.stream) == 0).all()
    hf.close()
    devf.close()
    h.compute(st, 0.0, dev.stream)  # legal: nothing is coincident here
    assert (h.read(1, dev.stream) == 1).all() and list(h.summary(dev.stream)) == [257, 0, 1, 0]
    assert all(len(v) == 0 for v in h.catalogue(dev.stream).values())  # an empty catalogue reads as empty arrays
    L = nb.lib()
    buf = np.zeros(300, np.uint32)
    assert L.nbody_fof_read(h.h, 0, buf.ctypes.data, 4 * 256, dev.stream) == 1 and b"needs 1028 bytes" in L.nbody_last_error()
    assert L.nbody_fof_read(h.h, 2, buf.ctypes.data, 4, dev.stream) == 1 and b"0 catalogued groups" in L.nbody_last_error()
    h.close()
    dev.close()


# ---- 8. CLI ---------------------------------------------------------------------------------------------------------------------------------
def cli(dim, args, cwd):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", f"nbody_hip_d{dim}")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


CLI_CASES = [("double", ["--algorithm", "all-pairs"], 20), ("float", [], 3)]


@pytest.mark.parametrize("prec,extra,min_members", CLI_CASES, ids=["double-all_pairs-default_min", "float-default_octree-min3"])
def test_cli_save_groups(nb, prec, extra, min_members):
    """-n 1000 -s 1 --csv-detailed --save pos --save-groups B: two frames; groups.bin has the stated header, every frame equals the
    binding's outputs on that frame's saved positions byte for byte, and positions.bin is what a run without the flag writes."""
    dtype = 1 if prec == "double" else 0
    n, dim, tsz = 1000, 3, 4 if dtype == 0 else 8
    base = ["-n", n, "-s", 1, "--csv-detailed", "--precision", prec, "--save", "pos"] + extra
    with tempfile.TemporaryDirectory() as d, tempfile.TemporaryDirectory() as d0:
        r0 = cli(dim, base, d0)
        assert r0.returncode == 0, r0.stderr
        praw = open(os.path.join(d0, "positions.bin"), "rb").read()
        nframes = (len(praw) - 16) // (n * dim * tsz)
        assert nframes == 2
        frames = np.frombuffer(praw, npt(dtype), nframes * n * dim, 16).reshape(nframes, n, dim)
        # a linking length that gives groups of every kind here: 1.2 times the mean spacing of the first frame's bounding box
        b = 1.2 * float(np.prod(frames[0].max(0) - frames[0].min(0)) / n) ** (1.0 / dim)
        flags = ["--save-groups", repr(b)] + ([] if min_members == 20 else ["--groups-min", min_members])
        r = cli(dim, base + flags, d)
        assert r.returncode == 0, r.stderr
        assert open(os.path.join(d, "positions.bin"), "rb").read() == praw
        assert not os.path.exists(os.path.join(d0, "groups.bin"))
        raw = open(os.path.join(d, "groups.bin"), "rb").read()
    assert struct.unpack("<4IdI", raw[:28]) == (n, 1, tsz, dim, b, min_members)
    hs = nb.build_model(dtype, dim, "uniform", n)
    want = raw[:28]
    for f in range(nframes):
        hs.x[:] = frames[f]
        dev = nb.DeviceSystem.from_host(hs)
        try:
            h = dev.fof_handle(min_members)
            h.compute(dev.state(), b, dev.stream)
            summary, cat = h.summary(dev.stream), h.catalogue(dev.stream)
            want += summary.tobytes() + h.read(0, dev.stream).tobytes() + h.read(1, dev.stream).tobytes()
            for e in range(int(summary[1])):
                want += cat["label"][e].tobytes() + cat["size"][e].tobytes() + cat["mass"][e].tobytes() + cat["com"][e].tobytes()
            assert 1 < summary[0] < n and summary[2] > 1, summary  # groups of more than one kind
        finally:
            dev.close()
    assert raw == want
