"""GPU: K1's f64 pair form with the source's mass folded into the polynomial (csrc/common.hpp: weight_far_folded; the constants
M15, M1875 beside the packed records, read by wave-uniform loads in the scalar stream and derived per lane in the LDS-tile form).
2D and 3D, both pair rules (40 000 bodies in a box on either side of kFarMinVolume), batches that mix far and close pairs,
unsoftened against the oracle and softened against a NumPy direct sum within the suite's f64 force tolerance, both source paths
bit for bit, shard windows bit for bit, and one far pair with identical bits in an all-far batch and in a mixed one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FORCE_TOL = 1e-12   # tests/test_gpu_all_pairs.py: FORCE_TOL[1]
N = 40000           # >= kFarMinBodies (32 768): the pair rule is measured, not "dense" by definition
BOX = {("sparse", 3): 63.0, ("sparse", 2): 1250.0,   # half side: volume 2.0e6 / area 6.3e6, above kFarMinVolume (1.7e5 / 6.4e4)
       ("dense", 3): 20.0, ("dense", 2): 100.0}      # volume 6.4e4 / area 4.0e4, below it
WINDOWS = ((0, N // 8), (N // 8, N // 8), (N - 5000, 5000), (12345, 7777))


def system(nb, dim, rule, seed=0):
    """Uniform box with partners planted tiles apart from their targets: gaps on both sides of r = 2 (the sparse rule's switch; on
    the sparse box these make mixed batches), down to the guarded form's range, and a zero-mass partner."""
    rng = np.random.default_rng(1000 + 10 * dim + seed)
    hs = nb.HostSystem(1, dim, N)
    side = BOX[(rule, dim)]
    hs.x[:] = rng.uniform(-side, side, (N, dim))
    hs.m[:] = 10.0 ** rng.uniform(-1, 1, N)
    hs.v[:] = 0
    for k, gap in enumerate([2.0, np.nextafter(2.0, 1.0), 1.5, 0.3, 3e-2, 2.0 ** -8, 3e-3, 1e-6]):
        i, j = 211 + 977 * k, 211 + 977 * k + 4099 + 1033 * k
        d = np.zeros(dim)
        d[k % dim] = gap
        hs.x[i] = np.round(hs.x[i])
        hs.x[j] = hs.x[i] + d
    hs.x[500] = hs.x[24000]
    hs.x[500, dim - 1] += 1.25
    hs.m[500] = 0
    hs.c, hs.dt = 1.0, 0.01
    return hs


def per_target_err(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    mag = np.abs(ref).max(axis=1)
    return (np.abs(a - ref).max(axis=1) / np.maximum(mag, np.median(mag))).max(), np.abs(a - ref).max() / np.abs(ref).max()


def softened_ref(m, x, c, e2, targets):
    """c * sum_j m_j (x_j - x_i) / (|x_j - x_i|^2 + e2)^(3/2) for the sampled targets, in long double."""
    dt = np.longdouble
    m, x = np.asarray(m, dt), np.asarray(x, dt)
    out = np.zeros((len(targets), x.shape[1]), dt)
    for s in range(0, len(targets), 64):
        t = targets[s:s + 64]
        d = x[None, :, :] - x[t][:, None, :]
        q = (d * d).sum(-1) + dt(e2)
        out[s:s + 64] = ((m[None, :] / (q * np.sqrt(q)))[:, :, None] * d).sum(1)
    return dt(c) * out


@pytest.mark.parametrize("rule", ["sparse", "dense"])
@pytest.mark.parametrize("dim", [3, 2])
def test_folded_k1_against_the_oracle(nb, oracle, dim, rule):
    """Unsoftened: the automatic launch (8 slices, chunks, R = 2) against the oracle, per target and overall, within FORCE_TOL;
    shard windows bit for bit; the LDS-tile form and the scalar stream at the same split bit for bit."""
    hs = system(nb, dim, rule)
    dev = nb.DeviceSystem.from_host(hs)
    sparse, vol = nb.all_pairs_pair_rule(dev.state(), dev.stream)
    assert sparse is (rule == "sparse"), (sparse, vol)
    desc = nb.describe_all_pairs(dev.state())
    assert "all_pairs_force_sgpr_kernel<double" in desc and "R=2" in desc and "JS=8" in desc and "far3m" in desc, desc
    ref = oracle.State(1, dim, N)
    ref.m[:], ref.x[:], ref.v[:], ref.c, ref.dt = hs.m, hs.x, hs.v, hs.c, hs.dt
    oracle.all_pairs_force(ref)
    dev.all_pairs_force()
    dev.sync()
    a = dev.download().a.copy()
    assert np.all(np.isfinite(a))
    worst, overall = per_target_err(a, ref.a)
    print(f"dim={dim} {rule}: per-target {worst:.3g} overall {overall:.3g}")
    assert worst <= FORCE_TOL and overall <= FORCE_TOL, (worst, overall)
    for first, count in WINDOWS:
        dev.all_pairs_force(first, count)
        dev.sync()
        assert np.array_equal(dev.download().a[first:first + count], a[first:first + count]), (first, count)
    dev.close()
    try:
        for tpt in (1, 2):
            res = []
            for path in (1, 2):
                nb.configure_all_pairs(4, tpt, source_path=path)
                d2 = nb.DeviceSystem.from_host(hs)
                d2.all_pairs_force()
                d2.sync()
                res.append(d2.download().a.copy())
                d2.close()
            assert np.array_equal(res[0], res[1]), tpt
            worst, overall = per_target_err(res[0], ref.a)
            assert worst <= FORCE_TOL and overall <= FORCE_TOL, (tpt, worst, overall)
    finally:
        nb.configure_all_pairs(0, 0, source_path=0)


@pytest.mark.parametrize("rule", ["sparse", "dense"])
@pytest.mark.parametrize("dim", [3, 2])
def test_folded_softened_k1(nb, dim, rule):
    """The softened twin on the same systems (it has no pair rule: the boxes only change the separations): against the direct sum
    on 384 sampled targets, the planted ones among them; shard windows and both source paths bit for bit."""
    hs = system(nb, dim, rule)
    eps = 0.05
    e2 = np.float64(eps) * np.float64(eps)
    rng = np.random.default_rng(3)
    t = np.unique(np.concatenate([rng.choice(N, 368, replace=False), 211 + 977 * np.arange(8), [500, 24000]]))
    ref = softened_ref(hs.m, hs.x, hs.c, e2, t)
    dev = nb.DeviceSystem.from_host(hs)
    dev.all_pairs_softened_force(eps)
    dev.sync()
    a = dev.download().a.copy()
    assert np.all(np.isfinite(a))
    worst, overall = per_target_err(a[t], ref)
    print(f"dim={dim} {rule} softened: per-target {worst:.3g} overall {overall:.3g}")
    assert worst <= FORCE_TOL and overall <= FORCE_TOL, (worst, overall)
    for first, count in WINDOWS:
        dev.all_pairs_softened_force(eps, first, count)
        dev.sync()
        assert np.array_equal(dev.download().a[first:first + count], a[first:first + count]), (first, count)
    dev.close()
    try:
        for tpt in (1, 2):
            res = []
            for path in (1, 2):
                nb.configure_all_pairs(4, tpt, source_path=path)
                d2 = nb.DeviceSystem.from_host(hs)
                d2.all_pairs_softened_force(eps)
                d2.sync()
                res.append(d2.download().a.copy())
                d2.close()
            assert np.array_equal(res[0], res[1]), tpt
            worst, overall = per_target_err(res[0][t], ref)
            assert worst <= FORCE_TOL and overall <= FORCE_TOL, (tpt, worst, overall)
    finally:
        nb.configure_all_pairs(0, 0, source_path=0)


@pytest.mark.parametrize("dim", [3, 2])
def test_far_pair_has_the_same_bits_in_an_all_far_batch_and_in_a_mixed_one(nb, dim):
    """Two sparse systems that differ in the POSITION of one massless body p.  In the first, every target of p's wave (the 128
    targets of its block: R = 2) is farther than 2 from both sources of one batch (j, j + 1): the wave takes the batch through the
    all-far form.  In the second, p sits at distance 1 from source j: the same wave takes the same batch through the mixed form, in
    which every other lane selects 0 for the eps term.  p has no mass, so as a source it adds exactly 0 in both systems, and every
    acceleration except p's own must be bit for bit the same."""
    rng = np.random.default_rng(50 + dim)
    hs = nb.HostSystem(1, dim, N)
    side = BOX[("sparse", dim)]
    hs.x[:] = rng.uniform(-side, side, (N, dim))
    hs.m[:] = 10.0 ** rng.uniform(-1, 1, N)
    hs.v[:] = 0
    hs.c, hs.dt = 1.0, 0.01
    group = np.arange(128 * 57, 128 * 58)       # one block's targets: they share every wave of the block
    p = int(group[5])
    hs.m[p] = 0
    j = None
    for cand in range(20000, N - 2, 2):         # a batch (two consecutive records, even first) far from the whole group
        d = hs.x[group][:, None, :] - hs.x[cand:cand + 2][None, :, :]
        if (d * d).sum(-1).min() >= 9.0:
            j = cand
            break
    assert j is not None
    out = []
    for moved in (False, True):
        h2 = nb.HostSystem(1, dim, N)
        h2.x[:], h2.m[:], h2.v[:], h2.c, h2.dt = hs.x, hs.m, hs.v, hs.c, hs.dt
        if moved:
            h2.x[p] = hs.x[j]
            h2.x[p, 0] += 1.0                   # r^2 = 1: below 4 (the mixed form), far above 2^-16 (not the guarded one)
        dev = nb.DeviceSystem.from_host(h2)
        assert nb.all_pairs_pair_rule(dev.state(), dev.stream)[0] is True
        assert "R=2" in nb.describe_all_pairs(dev.state())
        dev.all_pairs_force()
        dev.sync()
        out.append(dev.download().a.copy())
        dev.close()
    others = np.arange(N) != p
    assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
    assert np.array_equal(out[0][others], out[1][others])
    assert not np.array_equal(out[0][p], out[1][p])   # (p itself moved: its own sum is another one)
