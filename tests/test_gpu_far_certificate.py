"""K1's far certificate (csrc/common.hpp: k1_block_is_far; f64 scalar stream, sparse rule): a block — one target group against
one source chunk — whose bounding boxes are >= 3 apart on some axis streams its chunk through a loop without the near/far test.
The certificate must not change a bit, so every check here is an equality.

References.  The LDS-tile form never certifies, but it has no source chunks (one chunk, at most four slices), so it sums in another
order than the chunked launch and can only bound the result (TILE_RTOL below), not reproduce it.  The bitwise references are
  * the same launch with the certificate switched off (NBODY_K1_NO_CERT=1, experiments build: the same code object, only the
    box pointer is withheld) and the count of certified blocks that build keeps, against a NumPy restatement of the certificate;
  * in the shipped library, shard windows: a window's target groups hold other bodies than the whole launch's, so its blocks are
    certified differently — a window across the cluster boundary is not certified at all — and the rows must still be equal.
N = 32 768 is the smallest system that can take the sparse rule (kFarMinBodies): 16 chunks of 2048 sources, a launch well under
a millisecond."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N = 32768
GAP = 3.0
# tile form against the chunked scalar stream: two orders of one sum of N terms.  The terms of a component do not all have one
# sign, so the bound is on the scale of the largest row: N^(1/2) * 2^-53 * (sum of |terms|) stays far below 1e-12 of it
# (the same figure the smoke run allows against the oracle).
TILE_RTOL = 1e-12


@pytest.fixture(scope="module")
def nbx():
    """A second instance of the binding, bound to libnbody_hip_exp.so (the build that reads the switches and counts)."""
    name = "stdpar_nbody_amd_exp"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "stdpar-nbody_amd", "__init__.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mod.LIB_PATH = os.path.join(ROOT, "stdpar-nbody_amd", "libnbody_hip_exp.so")
        assert os.path.exists(mod.LIB_PATH), "libnbody_hip_exp.so is not built (make -C stdpar-nbody_amd experiments)"
    return sys.modules[name]


def system(nb, x, seed=1):
    n = len(x)
    hs = nb.HostSystem(nb.F64, 3, n)
    hs.m[:] = np.random.default_rng(seed).uniform(0.5, 1.5, n)
    hs.x[:] = x
    hs.dt, hs.c = 1e-3, 1.0
    return hs


def cube(rng, n, centre, side):
    return np.asarray(centre, np.float64) + rng.uniform(-0.5, 0.5, (n, 3)) * np.asarray(side, np.float64)


def two_clusters(n=N, split=N // 2, seed=7):
    rng = np.random.default_rng(seed)
    return np.concatenate([cube(rng, split, (-100.0, 50.0, 0.0), 40.0), cube(rng, n - split, (100.0, -50.0, 0.0), 40.0)])


def launch_shape(nb, dev, sparse=True):
    """(targets per lane, chunks) of the launch, and that it is the scalar stream on the sparse (dense) rule."""
    desc = nb.describe_all_pairs(dev.state())
    assert desc.startswith("all_pairs_force_sgpr_kernel<double,3,") and "JS=8" in desc and "cert=box-gap>=3" in desc, desc
    rule, volume = nb.all_pairs_pair_rule(dev.state(), dev.stream)
    assert rule == sparse, volume
    return int(re.search(r"R=(\d)", desc).group(1)), int(re.search(r"chunks=(\d+)", desc).group(1))


def model(x, r, chunks, first=0, count=None):
    """The certificate restated: -> (number of certified blocks, chunk boxes lo, hi).  Chunks as ap_auto_chunks cuts them, boxes
    over the padded records (padding lies at the origin; a chunk with a non-finite record is the whole line), target groups of
    64 r lanes whose lanes past `count` hold body `first`, gaps formed as the kernel forms them."""
    n = len(x)
    count = n - first if count is None else count
    ntiles = (n + 511) // 512
    tpc = (ntiles + 15) // 16
    assert (ntiles + tpc - 1) // tpc == chunks
    xp = np.zeros((ntiles * 512, 3))
    xp[:n] = x
    lo, hi = np.empty((chunks, 3)), np.empty((chunks, 3))
    for c in range(chunks):
        rec = xp[c * tpc * 512:(c + 1) * tpc * 512]
        ok = np.isfinite(rec).all()
        lo[c] = rec.min(axis=0) if ok else -np.inf
        hi[c] = rec.max(axis=0) if ok else np.inf
    g = 64 * r
    certified = 0
    with np.errstate(invalid="ignore"):
        for t0 in range(0, count, g):
            local = np.arange(t0, t0 + g)
            t = x[first + np.where(local < count, local, 0)]
            tmin, tmax = t.min(axis=0), t.max(axis=0)
            if not np.isfinite(t).all():
                continue
            for c in range(chunks):
                above, below = tmin - hi[c], lo[c] - tmax
                certified += bool((((above >= GAP) & np.isfinite(above)) | ((below >= GAP) & np.isfinite(below))).any())
    return certified, lo, hi


def force(nb, hs, first=0, count=None, path=0):
    dev = nb.DeviceSystem.from_host(hs)
    if path:
        dev.configure_all_pairs(4, 0, path)
    dev.all_pairs_force(first, count)
    a = dev.download().a.copy()
    dev.close()
    return a


def certified_blocks(nbx, stream, clear=False):
    """nbody_exp_k1_certified (experiments build only): the (target group, source chunk) blocks K1 has certified on this stream."""
    out = ctypes.c_uint64()
    assert nbx.lib().nbody_exp_k1_certified(ctypes.c_void_p(stream), ctypes.byref(out), 1 if clear else 0) == 0
    return int(out.value)


def counted(nbx, hs, certify=True):
    """-> (a, certified blocks) of one launch of the experiments build, with or without the certificate."""
    os.environ.pop("NBODY_K1_NO_CERT", None)
    if not certify:
        os.environ["NBODY_K1_NO_CERT"] = "1"
    try:
        dev = nbx.DeviceSystem.from_host(hs)
        certified_blocks(nbx, dev.stream, clear=True)
        dev.all_pairs_force()
        a = dev.download().a.copy()
        blocks = certified_blocks(nbx, dev.stream)
        dev.close()
    finally:
        os.environ.pop("NBODY_K1_NO_CERT", None)
    return a, blocks


def check(nb, nbx, x, expect=None, hs=None, sparse=True):
    """One system through every reference: shipped == experiments with and without the certificate (bitwise), the tile form
    (within its bound), and the count of certified blocks == the model (== expect when given).  -> (a, count)."""
    hs = hs or system(nb, x)
    dev = nb.DeviceSystem.from_host(hs)
    r, chunks = launch_shape(nb, dev, sparse)
    dev.all_pairs_force()
    a = dev.download().a.copy()
    dev.close()
    want, lo, hi = model(x, r, chunks)
    want = want if sparse else 0  # the dense rule has no test to save: the certificate is not attempted
    on, blocks = counted(nbx, hs)
    off, none = counted(nbx, hs, certify=False)
    print(f"n={len(x)} R={r} chunks={chunks}: certified {blocks}, model {want}, switched off {none}")
    assert none == 0
    assert blocks == want
    assert expect is None or want == expect, (want, expect)
    assert np.array_equal(a.view(np.int64), off.view(np.int64)) and np.array_equal(on.view(np.int64), off.view(np.int64))
    if np.isfinite(x).all():
        tile = force(nb, hs, path=1)
        err = np.abs(a - tile).max() / np.abs(tile).max()
        print(f"  against the tile form: {err:.3g} of the largest component")
        assert err <= TILE_RTOL
    return a, blocks, (lo, hi)


def test_aligned_clusters_certify_half_of_the_blocks(nb, nbx):
    """Cluster one in the first half of the indices, cluster two in the second: every cross-cluster block is certified, no other."""
    _, blocks, _ = check(nb, nbx, two_clusters(), expect=(N // 128) * 16 // 2)
    assert blocks == 2048
    rng = np.random.default_rng(3)
    check(nb, nbx, cube(rng, N, (0.0, 0.0, 0.0), 100.0), expect=0)  # a uniform cube on the sparse rule: every box is the cube


def test_padding_and_an_unaligned_boundary(nb, nbx):
    """N no multiple of the tile and clusters split inside a group and a chunk: the chunk across the boundary certifies against
    nobody, and the last chunk's box holds its padding records (the origin, which no body of either cluster is near)."""
    n, split = N + 37, N // 2 + 5
    x = two_clusters(n, split)
    _, blocks, (lo, hi) = check(nb, nbx, x)
    assert blocks > 0
    assert lo[-1, 0] == 0.0 and hi[-1, 1] == 0.0  # cluster two lies at x > 0, y < 0: the padding is the box's corner
    ntiles = (n + 511) // 512
    c = split // (((ntiles + 15) // 16) * 512)  # the chunk across the boundary spans both clusters on every axis
    assert lo[c, 0] < -80 and hi[c, 0] > 80


@pytest.mark.parametrize("gap", [np.nextafter(3.0, 0.0), 3.0, 2.5])
def test_at_the_threshold(nb, nbx, gap):
    """Two slabs that overlap in y and z, cluster one ending at x = 0 exactly and cluster two beginning at x = gap exactly in
    EVERY target group (so in every chunk): all cross-cluster blocks certify at 3.0, none just below."""
    rng = np.random.default_rng(11)
    half = N // 2
    one = cube(rng, half, (-20.0, 0.0, 0.0), (40.0, 60.0, 60.0))
    two = cube(rng, half, (20.0, 0.0, 0.0), (40.0, 60.0, 60.0))
    one[:, 0] = np.minimum(one[:, 0], -1e-3)
    two[:, 0] = np.maximum(two[:, 0], 1e-3) + gap
    one[::64, 0] = 0.0
    two[::64, 0] = gap
    check(nb, nbx, np.concatenate([one, two]), expect=2048 if gap >= 3.0 else 0)


def test_intruders(nb, nbx):
    """A body stored among cluster one's indices that lies inside cluster two: its chunk certifies against no group of cluster two,
    its target group against no chunk of cluster two — 128 + 8 blocks fewer."""
    x = two_clusters()
    x[5000] = (101.0, -49.0, 1.0)
    check(nb, nbx, x, expect=2048 - 128 - 8)


def test_shard_windows(nb):
    """Shipped library: a window's groups are cut elsewhere, so its blocks are certified differently; [16320, 16448) is one group
    across the cluster boundary, which nothing certifies.  The rows equal the whole launch's."""
    hs = system(nb, two_clusters())
    full = force(nb, hs)
    for first, count in ((1000, 3000), (N // 2 - 64, 128), (N // 2 - 700, 1500)):
        dev = nb.DeviceSystem.from_host(hs)
        dev.all_pairs_force(first, count)
        rows = dev.download().a[first:first + count]
        dev.close()
        assert np.array_equal(rows, full[first:first + count]), (first, count)


def test_non_finite_positions_never_certify(nb, nbx):
    """One NaN and one infinite source position.  The variances of such a system are NaN, so the launch takes the dense rule and
    attempts no certificate at all; were it attempted, the boxes would refuse (a chunk with such a record is the whole line, a gap
    that is not finite does not count: the model, which does not look at the rule, certifies neither their chunks nor their
    groups).  No block is certified and every bit is that of the launch without the certificate."""
    x = two_clusters()
    x[3000, 1] = np.nan
    x[20000, 0] = np.inf
    assert model(x, 2, 16)[0] == 2048 - 2 * (128 + 8) + 2  # (two blocks lie in a refused chunk AND a refused group)
    _, blocks, _ = check(nb, nbx, x, expect=0, sparse=False)
    assert blocks == 0


def test_replay_rebuilds_the_boxes(nb):
    """A recorded step (K1 + K3) replayed three times equals three eager steps: nothing is allocated, and the boxes follow the bodies."""
    hs = system(nb, two_clusters())
    hs.v[:] = np.random.default_rng(5).normal(0.0, 300.0, hs.v.shape)  # 0.3 per step: bodies cross their boxes' faces
    d1, d2 = nb.DeviceSystem.from_host(hs), nb.DeviceSystem.from_host(hs)
    for _ in range(3):
        d1.all_pairs_force()
        d1.accelerate_step()
    g = nb.StepGraph(d2, lambda: (d2.all_pairs_force(), d2.accelerate_step()))
    for _ in range(3):
        g.launch()
    a, b = d1.download(), d2.download()
    g.close()
    d1.close()
    d2.close()
    assert np.array_equal(a.x, b.x) and np.array_equal(a.v, b.v) and np.array_equal(a.a, b.a)
    assert not np.array_equal(a.x, hs.x)


def test_the_flagship_shape_in_small(nb, nbx):
    """The product's galaxy at N = 32 768: two discs, one per half of the indices."""
    hs = nb.build_model(nb.F64, 3, "galaxy", N)
    assert hs.n == N
    _, blocks, _ = check(nb, nbx, hs.x.copy(), hs=hs)
    assert blocks > 0
