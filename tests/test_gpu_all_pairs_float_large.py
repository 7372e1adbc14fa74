"""GPU: K1 in float from kFarMinBodies = 32 768 bodies on, where the launch measures the positions' moments and takes one of two
compiled copies of its source loop (csrc/common.hpp, pair_batch, `sizeof(T) == 4 && ffar`): under the sparse rule a pair at
r2 >= 4 takes m y^3 and a closer one, per lane, the guarded rcp(r2 * r2*y + eps) form.  Both rules, the production input (galaxy)
and the last size below the threshold, against oracle.all_pairs_force_wide — the reference's formula with every operation in
double on the float inputs and the reference's FLT_EPSILON kept — and the launch shapes of one system against each other bit for
bit.

Error measure, used everywhere in this file: per target err_i = max_k |a_gpu - a_wide|_k / scale_i, scale_i = c sum_j |m_j| r /
(r^3 + eps) the sum of the magnitudes of the target's terms.  Every case asserts the rule it means to test."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Largest err_i per case, measured on an MI355X (run with -s: every case prints its figure before it asserts):
#   planted sparse, automatic launch     3D 1.22e-6   2D 2.24e-6
#   planted sparse, split 4 (both paths) 3D 1.11e-5   2D 5.72e-5
#   dense at 32 768 (uniform, planted)   3D 1.22e-7   2D 2.17e-7
#   galaxy 32 768 (sparse)               3D 4.30e-6   2D 3.65e-6
#   32 767 bodies (dense by definition)  3D 5.65e-7   2D 1.08e-6
# The rule is MAX_ERR = 4 x the largest, rounded up to one digit, never above 1.5e-4 — what the reference's own float arithmetic
# shows on these inputs (float oracle against a float64 sum with FLT_EPSILON on the planted systems: 4.3e-5 in 3D, 1.4e-4 in 2D).
# 4 x 5.72e-5 is above that, so the cap it is: a margin of 2.6 over the largest figure.  The
# largest figures are the explicit split 4, which has ONE source chunk: a lane adds 8250 terms in one float chain where the
# automatic launch (8 slices, 13 chunks) adds 320, and in the 2D box (|d| up to 3500, terms of one sign on a side) the chain's
# rounding grows with its length.  That is the cost of the shape asked for, not of the pair rule: both source paths give the same
# bits there.
MAX_ERR = 1.5e-4
assert MAX_ERR <= 1.5e-4
# The automatic launches (every case but the explicit split 4) are held to their own, tighter constant by the same rule:
# 4 x 4.30e-6 = 1.7e-5 -> 2e-5.
MAX_ERR_AUTO = 2e-5

N = 33001                                # 65 tiles of 512, the last padded; 13 source chunks
SIDE = {3: 63.0, 2: 1250.0}              # half side of the sparse box, as tests/test_gpu_all_pairs.py's double system
F = np.float32
GAPS = [F(2.0), np.nextafter(F(2.0), F(3.0)), np.nextafter(F(2.0), F(1.0)), F(1.5), F(0.3), F(2.0 ** -8), F(3e-3), F(1e-4), F(1e-6)]
WINDOWS = ((0, N // 8), (N // 8, N // 8), (N - 5000, 5000), (12345, 7777))


def as_oracle_state(oracle, hs):
    ref = oracle.State(hs.dtype, hs.dim, hs.n)
    ref.m[:], ref.x[:], ref.v[:], ref.c, ref.dt = hs.m, hs.x, hs.v, hs.c, hs.dt
    return ref


def first_bodies(nb, hs, n):
    h = nb.HostSystem(hs.dtype, hs.dim, n)
    h.m[:], h.x[:], h.v[:], h.c, h.dt = hs.m[:n], hs.x[:n], hs.v[:n], hs.c, hs.dt
    return h


def sample_targets(n, planted, seed=1):
    """Every planted body, every target of the first and the last two blocks of 64, and 2000 random targets."""
    rng = np.random.default_rng(seed)
    tail = ((n - 1) // 64 - 1) * 64
    return np.unique(np.concatenate([np.asarray(planted, np.int64), np.arange(128), np.arange(tail, n),
                                     rng.choice(n, 2000, replace=False)])).astype(np.uint32)


def worst_err(a, targets, ref):
    ra, scale = ref
    return (np.abs(a[targets].astype(np.float64) - ra).max(axis=1) / scale).max()


@functools.lru_cache(maxsize=None)
def _planted_sparse(dim):
    """(m, x, planted, r2 of the planted gaps in float32): N bodies uniform in +-SIDE, masses in 0.5 ... 2, partners >= 4099 indices
    from their targets.  A target's coordinate on the gap axis is exactly 0 and its others are whole numbers, so the partner's
    coordinate IS the gap and fl(r2) is the rounded square of the gap and nothing else."""
    rng = np.random.default_rng(177 + dim)
    x = rng.uniform(-SIDE[dim], SIDE[dim], (N, dim)).astype(F)
    m = rng.uniform(0.5, 2.0, N).astype(F)
    planted, r2 = [], []
    for k, gap in enumerate(GAPS):
        i, j = 101 + 977 * k, 101 + 977 * k + 4099 + 1033 * k   # another source tile, another slice, usually another chunk
        x[i] = np.round(x[i])
        x[i, k % dim] = 0
        x[j] = x[i]
        x[j, k % dim] = gap
        d = x[j] - x[i]
        r2.append((d * d).sum(dtype=F))
        planted += [i, j]
    x[300] = x[29000]                        # coincident, distinct bodies
    x[400] = 0
    x[400, 1] = 7                            # not at the origin, where the zero-mass padding records sit
    x[31000] = x[400]
    x[31000, 0] = F(1e-22)                   # r2 = 1e-44: denormal in float
    x[500] = x[24000]
    x[500, dim - 1] += F(1e-3)
    m[500] = 0                               # zero-mass partner of a near pair
    planted += [300, 29000, 400, 31000, 500, 24000]
    x.setflags(write=False)
    m.setflags(write=False)
    return m, x, np.array(planted), np.array(r2, F)


def planted_sparse_host(nb, dim):
    m, x, planted, r2 = _planted_sparse(dim)
    hs = nb.HostSystem(0, dim, N)
    hs.m[:], hs.x[:] = m, x
    hs.c, hs.dt = 1.0, 0.01
    return hs, planted, r2


_REFS = {}


def reference(oracle, key, hs, targets):
    """oracle.all_pairs_force_wide of `hs` on `targets`, computed once per key and shared (never modified)."""
    if key not in _REFS:
        ra, scale = oracle.all_pairs_force_wide(as_oracle_state(oracle, hs), targets)
        assert np.isfinite(ra).all() and (scale > 0).all()
        ra.setflags(write=False)
        scale.setflags(write=False)
        _REFS[key] = (ra, scale)
    return _REFS[key]


def launch(dev, first=0, count=None):
    dev.all_pairs_force(first, count)
    dev.sync()
    return dev.download().a.copy()


@pytest.mark.parametrize("dim", [3, 2])
def test_sparse_rule_with_planted_pairs(nb, oracle, dim):
    """The sparse rule on 33 001 bodies with partners planted tiles apart: r2 exactly 4 and one float ulp to either side (the m y^3
    / guarded switch), gaps from 1.5 down to 1e-6, a coincident pair, a zero-mass partner and a denormal r2.  EVERY target against
    the wide reference (1.1e9 pairs in double: about 2 s on 16 threads)."""
    hs, planted, r2 = planted_sparse_host(nb, dim)
    four = F(4.0)
    assert r2[0] == four and r2[1] > four and r2[2] < four and len({float(r2[0]), float(r2[1]), float(r2[2])}) == 3, r2[:3]
    # the squares of 2 + ulp and 2 - ulp: two float steps above 4 (4.000001) and two below (3.9999995), nothing between counts
    assert r2[1] == F(4.0 + 2.0 ** -20) and r2[2] == F(4.0 - 2.0 ** -21), r2[:3]
    assert r2[3] == F(2.25) and r2[4] == F(0.3) * F(0.3) and r2[5] == F(2.0 ** -16)
    dev = nb.DeviceSystem.from_host(hs)
    sparse, vol = nb.all_pairs_pair_rule(dev.state(), dev.stream)
    assert sparse is True and vol >= (1.7e5 if dim == 3 else 6.4e4), (sparse, vol)
    assert nb.all_pairs_pair_rule(dev.state(100, 5000), dev.stream) == (sparse, vol)
    desc = nb.describe_all_pairs(dev.state())
    assert "m y^3" in desc and "all_pairs_force_sgpr_kernel<float" in desc and "chunks=13" in desc, desc
    a = launch(dev)
    dev.close()
    assert np.isfinite(a).all()
    targets = np.arange(N, dtype=np.uint32)
    ref = reference(oracle, ("sparse", dim), hs, targets)
    err = np.abs(a.astype(np.float64) - ref[0]).max(axis=1) / ref[1]
    print(f"planted sparse dim={dim}: max err_i {err.max():.3g} (planted {err[planted].max():.3g})")
    bad = np.where(err > MAX_ERR_AUTO)[0]
    assert bad.size == 0, (bad[:6], err[bad[:6]])


@pytest.mark.parametrize("dim", [3, 2])
def test_launch_shapes_of_the_sparse_system_agree_bit_for_bit(nb, oracle, dim):
    """Shard windows equal the rows of the whole launch; one and two targets per lane give the same bits ("no effect on the
    result", include/nbody_hip.h); at the explicit split 4 the LDS-tile form and the scalar stream give the same bits under the
    sparse rule, and that result (another summation order: 4 slices, one chunk) is within MAX_ERR too."""
    hs, planted, _ = planted_sparse_host(nb, dim)
    dev = nb.DeviceSystem.from_host(hs)
    assert nb.all_pairs_pair_rule(dev.state(), dev.stream)[0] is True
    full = launch(dev)
    assert np.isfinite(full).all()
    for first, count in WINDOWS:
        assert nb.all_pairs_pair_rule(dev.state(first, count), dev.stream)[0] is True
        w = launch(dev, first, count)
        assert np.array_equal(w[first:first + count], full[first:first + count]), (first, count)
    dev.close()
    for tpt in (1, 2):
        d2 = nb.DeviceSystem.from_host(hs)
        d2.configure_all_pairs(0, tpt, 0)
        assert f"R={tpt}" in nb.describe_all_pairs(d2.state()) and "m y^3" in nb.describe_all_pairs(d2.state())
        assert np.array_equal(launch(d2), full), tpt
        d2.close()
    res = []
    for path, kernel in ((1, "all_pairs_force_kernel<float"), (2, "all_pairs_force_sgpr_kernel<float")):
        d2 = nb.DeviceSystem.from_host(hs)
        d2.configure_all_pairs(4, 0, path)
        desc = nb.describe_all_pairs(d2.state())
        assert desc.startswith(kernel) and "JS=4" in desc and "chunks=1 " in desc and "m y^3" in desc, desc
        assert nb.all_pairs_pair_rule(d2.state(), d2.stream)[0] is True
        res.append(launch(d2))
        d2.close()
    assert np.isfinite(res[0]).all() and np.array_equal(res[0], res[1])
    targets = np.arange(N, dtype=np.uint32)
    err = worst_err(res[0], targets, reference(oracle, ("sparse", dim), hs, targets))
    print(f"planted sparse dim={dim}, split 4: max err_i {err:.3g}")
    assert err <= MAX_ERR, err


@pytest.mark.parametrize("dim", [3, 2])
def test_far_pair_has_the_same_bits_in_an_all_far_batch_and_in_a_mixed_one(nb, dim):
    """Float twin of the test of this name in tests/test_gpu_folded_weight.py.  Two sparse systems that differ in the POSITION of
    one massless body p.  In the first, every target of p's block is farther than 3 from all eight records of two consecutive
    batches (a batch is 4 records in float): those waves take the batches through the m y^3 form alone.  In the second, p sits at
    distance 1 from the first of these records: the same wave takes the same batch through the mixed form, in which every other
    lane keeps m y^3.  p has no mass, so as a source it adds exactly 0 in both systems, and every acceleration except p's own must
    be bit for bit the same.  What this can catch is narrow: in float m y^3 is formed BEFORE the wave-uniform branch and only
    selected after it, so a far pair's bits can differ between the two batches only if that select or the branch is broken; a
    wrong weight on either side of r2 = 4 is the business of the reference tests above, not of this one."""
    m, x, _, _ = _planted_sparse(dim)
    group = np.arange(128 * 57, 128 * 58)       # covers whole blocks at one and at two targets per lane
    p = int(group[5])
    j = None
    for cand in range(20000, N - 8, 8):
        d = x[group][:, None, :].astype(np.float64) - x[cand:cand + 8][None, :, :]
        if (d * d).sum(-1).min() >= 9.0:
            j = cand
            break
    assert j is not None
    out = []
    for moved in (False, True):
        hs = nb.HostSystem(0, dim, N)
        hs.m[:], hs.x[:] = m, x
        hs.m[p] = 0
        hs.c, hs.dt = 1.0, 0.01
        if moved:
            hs.x[p] = hs.x[j]
            hs.x[p, 0] += F(1.0)                # r2 = 1: below 4 (the guarded form), for this lane alone
        dev = nb.DeviceSystem.from_host(hs)
        assert nb.all_pairs_pair_rule(dev.state(), dev.stream)[0] is True
        assert "m y^3" in nb.describe_all_pairs(dev.state())
        out.append(launch(dev))
        dev.close()
    others = np.arange(N) != p
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    assert np.array_equal(out[0][others], out[1][others])
    assert not np.array_equal(out[0][p], out[1][p])   # (p itself moved: its own sum is another one)


@pytest.mark.parametrize("dim", [3, 2])
def test_dense_rule_at_the_threshold(nb, oracle, dim):
    """uniform at n = 32 768, the first size whose rule is measured: the unit cube is dense, every pair takes the guarded form.
    Near pairs (gaps 2^-8, 1e-4, 1e-6 as the float arrays hold them) and one coincidence planted in another source tile."""
    n = 32768
    hs = nb.build_model(0, dim, "uniform", n)
    assert hs.n == n
    planted = []
    for k, gap in enumerate([2.0 ** -8, 1e-4, 1e-6]):
        i, j = 101 + 977 * k, 101 + 977 * k + 4099 + 1033 * k
        hs.x[j] = hs.x[i]
        hs.x[j, k % dim] += F(gap)
        assert hs.x[j, k % dim] != hs.x[i, k % dim]
        planted += [i, j]
    hs.x[300] = hs.x[29000]
    planted += [300, 29000]
    dev = nb.DeviceSystem.from_host(hs)
    sparse, vol = nb.all_pairs_pair_rule(dev.state(), dev.stream)
    assert sparse is False and 0 < vol < (1.7e5 if dim == 3 else 6.4e4), (sparse, vol)
    assert "all_pairs_force_sgpr_kernel<float" in nb.describe_all_pairs(dev.state())
    a = launch(dev)
    dev.close()
    assert np.isfinite(a).all()
    targets = sample_targets(n, planted)
    err = worst_err(a, targets, reference(oracle, ("dense", dim), hs, targets))
    print(f"dense uniform n={n} dim={dim}: max err_i {err:.3g}")
    assert err <= MAX_ERR_AUTO, err


@pytest.mark.parametrize("dim", [3, 2])
def test_galaxy_at_the_threshold_takes_the_sparse_rule(nb, oracle, dim):
    """The production input: `--precision float --workload galaxy --algorithm all-pairs -n 32768` measures prod sqrt(12 var_k) =
    3.7e6 (3D) / 7.2e4 (2D), above the thresholds 1.7e5 / 6.4e4: the sparse rule in both dimensions."""
    n = 32768
    hs = nb.build_model(0, dim, "galaxy", n)
    assert hs.n == n
    dev = nb.DeviceSystem.from_host(hs)
    sparse, vol = nb.all_pairs_pair_rule(dev.state(), dev.stream)
    assert sparse is True and vol >= (1.7e5 if dim == 3 else 6.4e4), (sparse, vol)
    assert "m y^3" in nb.describe_all_pairs(dev.state())
    a = launch(dev)
    dev.close()
    assert np.isfinite(a).all()
    targets = sample_targets(n, [0, n // 2, n // 2 - 1, n - 1])     # the two centre masses and their neighbours in index
    err = worst_err(a, targets, reference(oracle, ("galaxy", dim), hs, targets))
    print(f"galaxy n={n} dim={dim}: vol {vol:.3g} max err_i {err:.3g}")
    assert err <= MAX_ERR_AUTO, err


@pytest.mark.parametrize("dim", [3, 2])
def test_one_body_below_the_threshold_is_dense_by_definition(nb, oracle, dim):
    """The first 32 767 bodies of the planted sparse system: the same box, but below kFarMinBodies nothing is measured and every
    pair, the ones at r2 >= 4 included, takes the guarded form."""
    n = 32767
    full, planted, _ = planted_sparse_host(nb, dim)
    hs = first_bodies(nb, full, n)
    assert planted.max() < n
    dev = nb.DeviceSystem.from_host(hs)
    assert nb.all_pairs_pair_rule(dev.state(), dev.stream)[0] is False
    assert nb.all_pairs_pair_rule(dev.state(100, 5000), dev.stream)[0] is False
    assert "m y^3" not in nb.describe_all_pairs(dev.state())
    a = launch(dev)
    dev.close()
    assert np.isfinite(a).all()
    targets = sample_targets(n, planted)
    err = worst_err(a, targets, reference(oracle, ("below", dim), hs, targets))
    print(f"planted n={n} dim={dim} (dense by definition): max err_i {err:.3g}")
    assert err <= MAX_ERR_AUTO, err
