"""K1's space order (csrc/all_pairs.hip: k1_order_wanted; f64, unsoftened, scalar stream): sources and targets sorted by the
space key (csrc/k1_order_key.hpp) so that more blocks take the far certificate.  The shipped gate is kOrderMinBodies; the
experiments build lowers it with NBODY_K1_ORDER_MIN=32768 — the smallest system that can take the sparse rule — and withholds the
order with NBODY_K1_NO_ORDER=1, so every check here runs at N = 32 768 and N = 32 768 + 37 (padding records, a last partial group).

Bounds.  An ordered launch sums a target's terms in key order, the unordered one in index order: two orders of one sum of N
terms, so the rows agree within 1e-12 of the largest row's norm and no tighter (the argument of test_gpu_far_certificate.py:
N^(1/2) * 2^-53 * (sum of |terms|) is far below it); against the wide oracle the ordered rows are held to the 1e-12 of the largest
component that test_gpu_all_pairs.py asks of the unordered ones.  Everything else is an equality: shard windows, repeated runs,
a replayed step, the dense rule (identity order) and the count of certified blocks against the NumPy restatement
(tools/k1_order_model.py) on the restated order."""
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
ORDER_TOL = 1e-12   # ordered against unordered rows, of the largest row's norm
FORCE_TOL = 1e-12   # against the wide oracle, of the largest component (tests/test_gpu_all_pairs.py: FORCE_TOL[1])


@pytest.fixture(scope="module")
def nbx():
    """The binding bound to libnbody_hip_exp.so (the build that reads the switches and counts certified blocks)."""
    name = "stdpar_nbody_amd_exp"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "stdpar-nbody_amd", "__init__.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mod.LIB_PATH = os.path.join(ROOT, "stdpar-nbody_amd", "libnbody_hip_exp.so")
        assert os.path.exists(mod.LIB_PATH), "libnbody_hip_exp.so is not built (make -C stdpar-nbody_amd experiments)"
    return sys.modules[name]


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("k1_order_model", os.path.join(ROOT, "tools", "k1_order_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class switches:
    """The experiments build's environment for the launches inside: the gate at N, the order withheld or not."""

    def __init__(self, order=True):
        self.order = order

    def __enter__(self):
        os.environ["NBODY_K1_ORDER_MIN"] = str(N)
        os.environ.pop("NBODY_K1_NO_ORDER", None)
        if not self.order:
            os.environ["NBODY_K1_NO_ORDER"] = "1"

    def __exit__(self, *exc):
        os.environ.pop("NBODY_K1_ORDER_MIN", None)
        os.environ.pop("NBODY_K1_NO_ORDER", None)


def system(nb, x, seed=1):
    n, dim = x.shape
    hs = nb.HostSystem(nb.F64, dim, n)
    hs.m[:] = np.random.default_rng(seed).uniform(0.5, 1.5, n)
    hs.x[:] = x
    hs.dt, hs.c = 1e-3, 1.0
    return hs


def cube(rng, n, centre, side):
    centre = np.asarray(centre, np.float64)
    return centre + rng.uniform(-0.5, 0.5, (n, len(centre))) * np.asarray(side, np.float64)


def two_clusters(n, dim, seed=7):
    rng = np.random.default_rng(seed)
    one, two = cube(rng, n // 2, (-100.0, 80.0, 0.0)[:dim], 40.0), cube(rng, n - n // 2, (100.0, -80.0, 0.0)[:dim], 40.0)
    x = np.concatenate([one, two])
    return x[rng.permutation(n)]  # the clusters' bodies interleaved: in index order no block certifies


_galaxy = {}


def galaxy(nb, n, dim):
    """The generator's galaxy at N bodies; the 37 extra bodies of the odd size are copies of the first ones, moved a little."""
    if dim not in _galaxy:
        hs = nb.build_model(nb.F64, dim, "galaxy", N)
        assert hs.n == N
        _galaxy[dim] = np.array(hs.x, np.float64).reshape(N, dim)
    x = _galaxy[dim]
    return x if n == N else np.concatenate([x, x[:n - N] + 0.25])


def layout(nb, name, n, dim):
    return galaxy(nb, n, dim) if name == "galaxy" else two_clusters(n, dim)


def certified_blocks(nbx, stream, clear=False):
    out = ctypes.c_uint64()
    assert nbx.lib().nbody_exp_k1_certified(ctypes.c_void_p(stream), ctypes.byref(out), 1 if clear else 0) == 0
    return int(out.value)


def launch(nbx, hs, order=True, tpt=0, windows=None, expect_order=True, sparse=True):
    """-> (a, certified blocks) of the experiments build; `windows`: [(first, count)] launched one after the other into one `a`."""
    with switches(order):
        dev = nbx.DeviceSystem.from_host(hs)
        if tpt:
            dev.configure_all_pairs(0, tpt, 0)
        desc = nbx.describe_all_pairs(dev.state())
        assert desc.startswith(f"all_pairs_force_sgpr_kernel<double,{hs.dim},") and "JS=8" in desc, desc
        assert ("order=" in desc) == (order and expect_order), desc
        assert not tpt or f"R={tpt}" in desc, desc
        rule, volume = nbx.all_pairs_pair_rule(dev.state(), dev.stream)
        assert sparse is None or bool(rule) == sparse, volume
        certified_blocks(nbx, dev.stream, clear=True)
        for first, count in windows or [(0, None)]:
            dev.all_pairs_force(first, count)
        a = dev.download().a.copy()
        blocks = certified_blocks(nbx, dev.stream)
        status = nbx.all_pairs_status(dev.stream)
        dev.close()
    assert not status["failed"], status
    return a, blocks, int(re.search(r"R=(\d)", desc).group(1))


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


_wide = {}


def wide_sample(oracle, hs, tag):
    """Rows of the wide oracle for a fixed sample of targets, computed once per system."""
    if tag not in _wide:
        ref = oracle.State(1, hs.dim, hs.n)
        ref.m[:], ref.x[:], ref.c = hs.m, hs.x, hs.c
        picks = np.unique(np.concatenate([np.random.default_rng(11).integers(0, hs.n, 96), [0, hs.n // 2, hs.n - 1]]))
        _wide[tag] = (picks, oracle.all_pairs_force_wide(ref, picks)[0])
    return _wide[tag]


@pytest.mark.parametrize("n", [N, N + 37])
@pytest.mark.parametrize("tpt", [1, 2])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("name", ["galaxy", "clusters"])
def test_ordered_against_unordered_and_the_oracle(nbx, oracle, model, name, dim, tpt, n):
    x = layout(nbx, name, n, dim)
    hs = system(nbx, x)
    on, blocks_on, r = launch(nbx, hs, tpt=tpt)
    off, blocks_off, _ = launch(nbx, hs, order=False, tpt=tpt)
    assert r == tpt
    scale = np.linalg.norm(off, axis=1).max()
    err = np.linalg.norm(on - off, axis=1).max() / scale
    picks, ref = wide_sample(oracle, hs, (name, dim, n))
    werr = np.abs(on[picks] - ref).max() / np.abs(ref).max()
    perm = model.space_order(x)
    want = model.certified(x[perm], x[perm], r)[0]
    natural = model.certified(x, x, r)[0]
    print(f"{name} D={dim} R={r} n={n}: ordered - unordered {err:.3g} of the largest row, ordered - wide {werr:.3g} of the largest "
          f"component; certified {blocks_on} (model {want}), unordered {blocks_off} (model {natural})")
    assert np.isfinite(on).all()
    assert err <= ORDER_TOL
    assert werr <= FORCE_TOL
    assert blocks_on == want and blocks_off == natural
    assert blocks_on > blocks_off


def test_twice_the_same_bits(nbx):
    hs = system(nbx, two_clusters(N + 37, 3))
    a, blocks, _ = launch(nbx, hs)
    b, again, _ = launch(nbx, hs)
    assert same_bits(a, b) and blocks == again
    with switches():
        dev = nbx.DeviceSystem.from_host(hs)
        dev.all_pairs_force()
        dev.all_pairs_force()   # the same context again: the scratch of the first call is reused
        c = dev.download().a.copy()
        dev.close()
    assert same_bits(a, c)


@pytest.mark.parametrize("name,n", [("clusters", N + 37), ("galaxy", N)])
def test_shard_windows(nbx, name, n):
    """The ordered whole launch against ordered windows: every window sorts ALL sources alike and its own targets; equal rows."""
    hs = system(nbx, layout(nbx, name, n, 3))
    full, _, _ = launch(nbx, hs)
    rows, _, _ = launch(nbx, hs, windows=[(1000, 2049)])
    assert same_bits(rows[1000:3049], full[1000:3049]) and not rows[:1000].any() and not rows[3049:].any()
    for parts in (2, 8, 70):
        cuts = [nbx.shard_range(n, k, parts) for k in range(parts)]
        got, _, _ = launch(nbx, hs, windows=[(f, e - f) for f, e in cuts])
        assert same_bits(got, full), parts
    # the two clusters' bodies alternate in index order, so every window straddles them; one more across the middle of the galaxy
    rows, _, _ = launch(nbx, hs, windows=[(n // 2 - 700, 1500)])
    assert same_bits(rows[n // 2 - 700:n // 2 + 800], full[n // 2 - 700:n // 2 + 800])


def test_dense_cube_keeps_its_bits(nbx):
    """A cube of the same size on the dense rule: the keys are all 0, the order is the identity, nothing certifies."""
    rng = np.random.default_rng(3)
    hs = system(nbx, cube(rng, N + 37, (0.0, 0.0, 0.0), 40.0))
    on, blocks_on, _ = launch(nbx, hs, sparse=False)
    off, blocks_off, _ = launch(nbx, hs, order=False, sparse=False)
    assert same_bits(on, off) and np.isfinite(on).all()
    assert blocks_on == 0 and blocks_off == 0


def test_escaper_at_1e6(nbx, oracle, model):
    """One body at 1e6: its cell is clamped to the grid's outermost one, the rule stays sparse, the launch is ordered."""
    x = two_clusters(N, 3)
    x[77] = (1e6, 3.0, -2.0)
    hs = system(nbx, x)
    on, blocks_on, r = launch(nbx, hs)
    off, _, _ = launch(nbx, hs, order=False)
    scale = np.linalg.norm(off, axis=1).max()
    picks, ref = wide_sample(oracle, hs, "escaper")
    perm = model.space_order(x)
    print(f"escaper at 1e6: ordered - unordered {np.linalg.norm(on - off, axis=1).max() / scale:.3g}, certified {blocks_on}")
    assert np.isfinite(on).all()
    assert np.linalg.norm(on - off, axis=1).max() <= ORDER_TOL * scale
    assert np.abs(on[picks] - ref).max() <= FORCE_TOL * np.abs(ref).max()
    assert blocks_on == model.certified(x[perm], x[perm], r)[0] and blocks_on > 0


def test_escapers_at_1e6_and_minus_1e300(nbx, oracle, model):
    """One body at 1e6 and one at -1e300: both cells are clamped, so the order stays total, and the result stays finite and within
    tolerance.  The variances of this system are +inf, which the rule reads as sparse: the launch is ordered, and the ordered copies
    K1 reads hold the far body at -1e150 (all_pairs.hip: kOrderSafe), so no squared distance overflows; its pairs weigh 0, as they
    do in the wide oracle once rounded to double.  The reference is the wide oracle at the tolerance of every other case: the
    UNORDERED launch cannot serve here — K1's pair form turns the overflowing squared distance into NaN (inf * 0 in the polish) in
    every row, below the gate as before the order existed — so it is held to the ordered one only on rows where it is finite."""
    x = two_clusters(N, 3)
    x[77] = (1e6, 3.0, -2.0)
    x[20000] = (-1e300, 0.0, 0.0)
    hs = system(nbx, x)
    on, blocks_on, r = launch(nbx, hs, sparse=None)
    off, blocks_off, _ = launch(nbx, hs, order=False, sparse=None)
    perm = model.space_order(x)
    xs = model.launch_positions(x[perm])
    want = model.certified(xs, xs, r)[0]
    ref = oracle.State(1, 3, N)
    ref.m[:], ref.x[:], ref.c = hs.m, hs.x, hs.c
    picks = np.unique(np.concatenate([np.random.default_rng(11).integers(0, N, 96), [0, 77, 20000, N - 1]]))
    wide = oracle.all_pairs_force_wide(ref, picks)[0]
    ok = np.isfinite(off).all(axis=1)
    print(f"escapers at 1e6 and -1e300: rows that are not finite: ordered {int((~np.isfinite(on)).any(axis=1).sum())}, unordered "
          f"{int((~ok).sum())} of {N}; ordered - wide {np.abs(on[picks] - wide).max() / np.abs(wide).max():.3g} of the largest component; "
          f"certified {blocks_on} (model {want}), unordered {blocks_off}")
    assert np.isfinite(wide).all() and not wide[picks == 20000].any()      # the far body feels nothing that a double can hold
    assert np.isfinite(on).all()
    assert np.abs(on[picks] - wide).max() <= FORCE_TOL * np.abs(wide).max()
    assert not on[20000].any()
    if ok.any():
        assert np.linalg.norm(on[ok] - off[ok], axis=1).max() <= ORDER_TOL * np.linalg.norm(off[ok], axis=1).max()
    assert blocks_on == want and blocks_on > 0


def test_nan_position_orders_nothing(nbx):
    """A NaN position: the variances are NaN, the rule is dense, the order is the identity — the behaviour of the unordered launch."""
    x = two_clusters(N, 3)
    x[3000, 1] = np.nan
    hs = system(nbx, x)
    on, blocks_on, _ = launch(nbx, hs, sparse=False)
    off, blocks_off, _ = launch(nbx, hs, order=False, sparse=False)
    assert same_bits(on, off) and blocks_on == 0 and blocks_off == 0


def test_capture_and_replay(nbx):
    """A recorded step (the ordering passes, K1, the scatter, K3) replayed three times equals three eager steps: nothing is
    allocated while recording, and keys, order and boxes follow the bodies."""
    hs = system(nbx, two_clusters(N + 37, 3))
    hs.v[:] = np.random.default_rng(5).normal(0.0, 300.0, hs.v.shape)  # 0.3 per step: bodies change cells
    with switches():
        d1, d2 = nbx.DeviceSystem.from_host(hs), nbx.DeviceSystem.from_host(hs)
        assert "order=" in nbx.describe_all_pairs(d1.state())
        for _ in range(3):
            d1.all_pairs_force()
            d1.accelerate_step()
        g = nbx.StepGraph(d2, lambda: (d2.all_pairs_force(), d2.accelerate_step()))
        for _ in range(3):
            g.launch()
        a, b = d1.download(), d2.download()
        g.close()
        d1.close()
        d2.close()
    assert same_bits(a.x, b.x) and same_bits(a.v, b.v) and same_bits(a.a, b.a)
    assert not np.array_equal(a.x, hs.x)


def test_shipped_gate(nb, oracle):
    """The shipped library reads no switch: ordered from kOrderMinBodies = 262 144 on, not below.  One ordered launch of the
    shipped build at the gate: within the oracle's bound on a sample, and a rank's window equal to the whole launch's rows."""
    n = 262144
    small = nb.DeviceSystem.from_host(nb.build_model(nb.F64, 3, "galaxy", n // 2))
    assert "order=" not in nb.describe_all_pairs(small.state())
    small.close()
    hs = nb.build_model(nb.F64, 3, "galaxy", n)
    assert hs.n == n
    dev = nb.DeviceSystem.from_host(hs)
    assert "order=morton30" in nb.describe_all_pairs(dev.state())
    dev.all_pairs_force()
    full = dev.download().a.copy()
    dev.close()
    ref = oracle.State(1, 3, n)
    ref.m[:], ref.x[:], ref.c = hs.m, hs.x, hs.c
    picks = np.unique(np.concatenate([np.random.default_rng(11).integers(0, n, 24), [0, n - 1]]))
    want = oracle.all_pairs_force_wide(ref, picks)[0]
    assert np.abs(full[picks] - want).max() <= FORCE_TOL * np.abs(want).max()
    f, e = nb.shard_range(n, 3, 8)
    dev = nb.DeviceSystem.from_host(hs)
    dev.all_pairs_force(f, e - f)
    got = dev.download().a
    dev.close()
    assert np.array_equal(got[f:e], full[f:e]) and not got[:f].any() and not got[e:].any()
