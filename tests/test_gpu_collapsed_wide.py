"""GPU: K2 (nbody_all_pairs_collapsed_force) per body against the wide reference, at every launch shape its plan has.

Reference: oracle.all_pairs_force_wide — the reference's formula with every operation in double for float inputs and in long double
for double inputs, eps(T) kept (tests/test_oracle_wide.py validates it).  Error measure, used everywhere in this file: per target
err_i = max_k |a_gpu - a_wide|_k / scale_i, scale_i = c sum_j |m_j| r / (r^3 + eps) the sum of the magnitudes of the target's terms.
Bound: the project's force bound per body, FORCE_TOL = 1e-12 double / 2e-5 float, as tests/test_gpu_octree_wide.py uses it, in every
case: none needed more.  (For comparison, the reference's own arithmetic in T, oracle.all_pairs_force against the same wide sums on
the same targets, measured on the CPU: double at most 2.9e-14; float 2.5e-4 on galaxy at 33 001 bodies, 4.4e-5 / 1.5e-4 on the planted
system in 3D / 2D, 4.8e-6 on uniform — one chain of n terms where K2's chains hold at most 32.)

Every case asserts the launch shape it means to test from nbody_all_pairs_collapsed_describe (tests/test_collapsed_plan.py pins the
arithmetic) and prints its figure before it asserts (-s).  The figures an MI355X gave are in
profiles/tests_k2_wide/new_tests_figures.txt and in the docstrings."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401
from test_collapsed_plan import experiment_forms, fields, k2_switches
from test_gpu_all_pairs import _planted_system
from test_gpu_all_pairs_float_large import as_oracle_state, planted_sparse_host, sample_targets
from test_gpu_space_order import nbx  # noqa: F401  (the binding bound to libnbody_hip_exp.so; asserts that it is built)
from test_oracle_octree_wide import FORCE_TOL

pytestmark = pytest.mark.gpu

F32, F64 = 0, 1
N = 33001
SIZES = {F64: (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049),                    # group 8, wave 64, block 256, tile 1024
         F32: (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 5000)}  # group 16, block 64, batches 512 / 256
NP_T = {F32: np.float32, F64: np.float64}


def reference(oracle, hs, targets=None):
    ra, scale = oracle.all_pairs_force_wide(as_oracle_state(oracle, hs), targets)
    assert np.isfinite(ra).all() and np.isfinite(scale).all()
    ra.setflags(write=False)
    scale.setflags(write=False)
    return ra, scale


_REFS = {}


def cached_reference(oracle, key, hs, targets):
    """The wide reference of a system, computed once per key and shared (never modified)."""
    if key not in _REFS:
        _REFS[key] = reference(oracle, hs, targets)
    return _REFS[key]


def per_body(got, want, scale):
    """err_i; a body whose terms are all zero (a single body) must be exact."""
    diff = np.abs(np.asarray(got, np.float64) - want).max(axis=1)
    assert np.all(diff[scale == 0] == 0)
    return np.where(scale > 0, diff / np.where(scale > 0, scale, 1.0), 0.0)


def k2(nb, dev):
    dev.all_pairs_collapsed_force()
    dev.sync()
    return dev.download().a.copy()


def steady(hs, seed):
    """The driver's steady state: a random, ao == a, so that the reset leaves exactly 0."""
    hs.a[:] = np.random.default_rng(seed).standard_normal(hs.a.shape)
    hs.ao[:] = hs.a


# ---- (a) every target at the shape boundaries ----------------------------------------------------------------------------------------

def boundary_system(nb, dtype, dim, n):
    hs = nb.build_model(dtype, dim, "uniform", n)
    assert hs.n == n
    if n >= 17:
        t = NP_T[dtype]
        hs.x[5] = hs.x[11]                   # coincident, distinct bodies: the pair adds exactly 0
        hs.x[7] = hs.x[3]
        hs.x[7, 0] += t(1e-4)                # r^3 = 1e-12 << eps(float): the `+ eps` dominates the denominator
        assert hs.x[7, 0] != hs.x[3, 0]
        hs.x[13] = 0                         # at the origin, where the streamed form's zero-mass padding records sit
    steady(hs, n)
    return hs


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_every_target_at_the_shape_boundaries(nb, oracle, dtype, dim):
    """uniform at sizes on both sides of every boundary of the launch shape — a group of 8 / 16 targets, a wave, a block, one and two
    batches, one and two tiles, the padding — with a coincident pair, a pair at 1e-4 and a body at the origin from 17 bodies on, from
    the driver's steady state (ao == a).  EVERY target against the wide reference.
    MI355X, largest err_i over the sizes: double 3D 1.51e-15, 2D 1.65e-15; float 3D 1.82e-7, 2D 2.19e-7."""
    worst = {}
    for n in SIZES[dtype]:
        hs = boundary_system(nb, dtype, dim, n)
        dev = nb.DeviceSystem.from_host(hs)
        a = k2(nb, dev)
        dev.close()
        assert np.isfinite(a).all(), n
        if n == 1:
            assert not a.any()
            continue
        ref = reference(oracle, hs)
        err = per_body(a, *ref)
        worst[n] = err.max()
        print(f"boundaries dtype={dtype} dim={dim} n={n}: max err_i {err.max():.3g} (body {err.argmax()})")
        bad = np.where(err > FORCE_TOL[dtype])[0]
        assert bad.size == 0, (n, bad[:6], err[bad[:6]])
    print(f"boundaries dtype={dtype} dim={dim}: max err_i {max(worst.values()):.3g} (n={max(worst, key=worst.get)})")


# ---- (b) the production shapes at 33 001 bodies ---------------------------------------------------------------------------------------

SHAPE = {(F32, 3): ("all_pairs_collapsed_stream_kernel<8> hand float 3 ", dict(padded=33792, nbatches=66, bpc=4, chunks=17)),
         (F32, 2): ("all_pairs_collapsed_stream_cxx_kernel<float,2,4> compiled float 2 ", dict(padded=33280, nbatches=130, bpc=6, chunks=22)),
         (F64, 3): ("all_pairs_collapsed_kernel<double,3,NT=8,KS=8,NB=1> tile=1024 ", dict(iblocks=129, ntiles=33, tpb=2, ysplit=17)),
         (F64, 2): ("all_pairs_collapsed_kernel<double,2,NT=8,KS=8,NB=1> tile=1024 ", dict(iblocks=129, ntiles=33, tpb=2, ysplit=17))}
D_GAPS = [2.0 ** -8, np.nextafter(2.0 ** -8, 0.0), np.nextafter(2.0 ** -8, 1.0), 1e-3, 1e-6, 1e-9, 1e-12]
D_SIDE = {3: 63.0, 2: 1250.0}


def high_word(v):
    return int(np.float64(v).view(np.uint64)) >> 32


def planted_double_host(nb, dim):
    """(hs, planted, r2 of the planted gaps in double), built as test_gpu_all_pairs_float_large.py builds its float system: N bodies
    uniform in +-D_SIDE, masses in 0.5 ... 2, partners >= 4099 indices from their targets (another tile of 1024 and, at two tiles per
    block row, another block row).  A target's coordinate on the gap axis is exactly 0 and its others are whole numbers, so the
    partner's coordinate IS the gap and fl(r2) is the rounded square of the gap and nothing else."""
    rng = np.random.default_rng(277 + dim)
    hs = nb.HostSystem(F64, dim, N)
    x = rng.uniform(-D_SIDE[dim], D_SIDE[dim], (N, dim))
    m = rng.uniform(0.5, 2.0, N)
    planted, r2 = [], []
    for k, gap in enumerate(D_GAPS):
        i, j = 101 + 977 * k, 101 + 977 * k + 4099 + 1033 * k
        x[i] = np.round(x[i])
        x[i, k % dim] = 0
        x[j] = x[i]
        x[j, k % dim] = gap
        d = x[j] - x[i]
        r2.append((d * d).sum())
        planted += [i, j]
    x[300] = x[29000]                        # coincident, distinct bodies
    x[400] = 0                               # a body at the origin ...
    x[31000] = 0
    x[31000, 0] = 1e-160                     # ... and its partner at r2 = 1e-320: denormal in double
    x[500] = x[24000]
    x[500, dim - 1] += 1e-3
    m[500] = 0                               # zero-mass partner of a near pair
    planted += [300, 29000, 400, 31000, 500, 24000]
    hs.m[:], hs.x[:] = m, x
    hs.c, hs.dt = 1.0, 0.01
    return hs, np.array(planted), np.array(r2)


def production_system(nb, dtype, dim, kind):
    """(hs, planted bodies) of one of the three systems of the 33 001-body cases."""
    if kind == "planted":
        if dtype == F32:
            hs, planted, r2 = planted_sparse_host(nb, dim)
            f = np.float32
            assert r2[5] == f(2.0 ** -16) and r2[7] == f(1e-4) * f(1e-4) and r2[8] == f(1e-6) * f(1e-6), r2
        else:
            hs, planted, r2 = planted_double_host(nb, dim)
            near = 2.0 ** -16
            # 2^-8 squares to 2^-16 exactly, whose high word is near_hi itself (0x3EF00000): not below it, the far form; one ulp
            # less squares to a value below 2^-16 (guarded); one ulp more stays far
            assert r2[0] == near and r2[1] < near < r2[2] and high_word(r2[0]) == 0x3EF00000, r2[:3]
            assert high_word(r2[1]) < 0x3EF00000 <= high_word(r2[2]), [hex(high_word(v)) for v in r2[:3]]
            assert r2[1] == near * (1 - 2.0 ** -52) and r2[2] == near * (1 + 2.0 ** -51), r2[:3]
            assert np.array_equal(r2[3:], np.array(D_GAPS[3:]) * np.array(D_GAPS[3:])), r2
            assert 0 < hs.x[31000, 0] ** 2 < np.finfo(np.float64).tiny and not hs.x[400].any()
        return hs, planted
    hs = nb.build_model(dtype, dim, kind, N)
    assert hs.n in (N, N - 1)                # (galaxy makes an even number of bodies)
    return hs, np.array([0, hs.n // 2, hs.n // 2 - 1, hs.n - 1])


def production_targets(n, planted):
    """sample_targets plus the whole 64-aligned run of targets around every planted body: the near-pair decision is per group of
    targets, so a planted pair changes the path of its group-mates."""
    runs = [np.arange(p // 64 * 64, min(n, p // 64 * 64 + 64)) for p in planted]
    return np.unique(np.concatenate([sample_targets(n, planted)] + runs)).astype(np.uint32)


@pytest.mark.parametrize("kind", ["galaxy", "uniform", "planted"])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_production_shapes_at_33001_bodies(nb, oracle, dtype, dim, kind):
    """The shapes production sizes take and no smaller size reaches.  Float: four (3D) / six (2D) batches per chunk — two and three
    trips with the hand-over between them and the clamped prefetch of the last — and a last chunk of two / four batches.  Double: two
    tiles per block row, the last row with one.  The planted systems put near pairs tiles and block rows apart from their targets;
    the double one tries the two-pass near-pair decision at its threshold r2 = 2^-16, one ulp to either side of the gap, down to
    1e-12, a coincident pair, a zero-mass partner and a denormal r2.
    MI355X, largest err_i (galaxy / uniform / planted): double 3D 2.45e-15 / 2.62e-16 / 4.88e-16, 2D 1.32e-15 / 9.98e-16 / 7.11e-16;
    float 3D 7.39e-7 / 1.10e-7 / 1.91e-7, 2D 8.97e-7 / 1.12e-7 / 3.31e-7."""
    hs, planted = production_system(nb, dtype, dim, kind)
    dev = nb.DeviceSystem.from_host(hs)
    line = nb.describe_all_pairs_collapsed(dev.state())
    prefix, shape = SHAPE[dtype, dim]
    got = fields(line)
    assert line.startswith(prefix) and {k: got[k] for k in shape} == shape, line
    a = k2(nb, dev)
    dev.close()
    assert np.isfinite(a).all()
    targets = production_targets(hs.n, planted)
    key = ("production", dtype, dim, kind)
    ref = cached_reference(oracle, key, hs, targets)
    err = per_body(a[targets], *ref)
    bound = FORCE_TOL[dtype]
    on_planted = err[np.isin(targets, planted)].max()
    print(f"production {kind} dtype={dtype} dim={dim} n={hs.n}: max err_i {err.max():.3g} (planted {on_planted:.3g}) bound {bound:.3g}")
    bad = np.where(err > bound)[0]
    assert bad.size == 0, (targets[bad[:6]], err[bad[:6]])


# ---- (c) the reset ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_reset_with_independent_a_and_ao(nb, oracle, dtype, dim, n):
    """K2 computes a = (a - ao) + sum (the diagonal pairs of the reference).  a0 and ao0 random and independent: the first call must
    give fl_T(a0 - ao0) + a_wide per body within FORCE_TOL (scale_i + max_k |a0 - ao0|_k); a second call with ao untouched subtracts
    ao0 and adds the sum once more, within the same bound doubled.
    MI355X, largest error / bound over the cases: first call double 1.4e-3, float 1.0e-2; second call (of the doubled bound) double
    1.4e-3, float 1.0e-2."""
    t = NP_T[dtype]
    hs = nb.build_model(dtype, dim, "uniform", n)
    rng = np.random.default_rng(1000 * dim + n)
    hs.a[:] = rng.standard_normal(hs.a.shape)
    hs.ao[:] = rng.standard_normal(hs.a.shape)
    a0, ao0 = hs.a.copy(), hs.ao.copy()
    dev = nb.DeviceSystem.from_host(hs)
    a1 = k2(nb, dev)
    a2 = k2(nb, dev)
    assert np.array_equal(dev.download().ao, ao0)
    dev.close()
    assert np.isfinite(a1).all() and np.isfinite(a2).all()
    wide, scale = cached_reference(oracle, ("reset", dtype, dim, n), hs, None)
    reset = (a0 - ao0).astype(t)                              # fl_T(a0 - ao0)
    bound = FORCE_TOL[dtype] * (scale + np.abs(reset.astype(np.float64)).max(axis=1))
    want1 = reset.astype(np.float64) + wide
    e1 = (np.abs(a1.astype(np.float64) - want1).max(axis=1) / bound).max()
    want2 = (want1.astype(t) - ao0).astype(np.float64) + wide
    e2 = (np.abs(a2.astype(np.float64) - want2).max(axis=1) / (2 * bound)).max()
    print(f"reset dtype={dtype} dim={dim} n={n}: error / bound first call {e1:.3g}, second call {e2:.3g}")
    assert e1 <= 1.0 and e2 <= 1.0, (e1, e2)


# ---- (d) one partial sum per target means the same bits --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [257, 1024])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_one_partial_sum_per_target_gives_the_same_bits(nb, dtype, dim, n):
    """Where the plan has one block row (double) or one source chunk (float), every target receives ONE atomic add onto the reset
    value and two calls from the same uploaded state must agree bit for bit.  That holds up to 1024 bodies, except in float 2D, whose
    batches are 256 records: one chunk up to 512 bodies (tests/test_collapsed_plan.py pins both), so that case runs at 512 in place of
    1024.  Nothing is asserted about bits where several chunks add atomically."""
    if (dtype, dim, n) == (F32, 2, 1024):
        n = 512
    hs = nb.build_model(dtype, dim, "uniform", n)
    rng = np.random.default_rng(n)
    hs.a[:] = rng.standard_normal(hs.a.shape)
    hs.ao[:] = rng.standard_normal(hs.a.shape)
    dev = nb.DeviceSystem.from_host(hs)
    f = fields(nb.describe_all_pairs_collapsed(dev.state()))
    assert (f["ysplit"] if dtype == F64 else f["chunks"]) == 1, f
    first = k2(nb, dev)
    dev.upload(hs)
    second = k2(nb, dev)
    dev.close()
    assert np.isfinite(first).all() and first.any()
    assert np.array_equal(first, second)


# ---- (e) the experiment forms ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_experiment_forms(nbx, oracle, dtype, dim):  # noqa: F811
    """The forms NBODY_K2_CFG and NBODY_K2_CHUNKS select in libnbody_hip_exp.so — the A/B baseline of every K2 optimisation, the
    compiled pair that cross-checks the hand-scheduled one among them — on the 6000 bodies of tests/test_gpu_all_pairs.py's planted
    system (near pairs tiles apart, coincidences, a zero-mass partner, a denormal r2), every target.  Each form's describe line is
    asserted first, so that a value that silently fell through to the default would be caught; the streamed forms also run as one
    chunk (every batch in one chain of trips) and with an odd chunk count.
    MI355X, largest err_i over the forms: double 3D 1.19e-15, 2D 9.81e-16; float 3D 2.50e-7, 2D 6.69e-7."""
    hs, planted = _planted_system(nbx, dtype, dim, True)
    steady(hs, 6000 + dim)
    ref = cached_reference(oracle, ("forms", dtype, dim), hs, None)
    bound = FORCE_TOL[dtype]
    dev = nbx.DeviceSystem.from_host(hs)
    seen, worst = set(), 0.0
    for cfg, chunks, prefix in experiment_forms(dtype, dim):
        with k2_switches(cfg, chunks):
            line = nbx.describe_all_pairs_collapsed(dev.state())
            assert line.startswith(prefix), (cfg, chunks, line)
            if chunks is not None:
                assert fields(line)["chunks"] == chunks, line
            dev.upload(hs)
            a = k2(nbx, dev)
        seen.add(line)
        assert np.isfinite(a).all(), line
        err = per_body(a, *ref)
        worst = max(worst, err.max())
        print(f"form cfg={cfg} chunks={chunks} dtype={dtype} dim={dim}: max err_i {err.max():.3g} (planted {err[planted].max():.3g})  {line}")
        bad = np.where(err > bound)[0]
        assert bad.size == 0, (line, bad[:6], err[bad[:6]])
    dev.close()
    assert len(seen) >= (7 if dtype == F64 else 8 if dim == 2 else 17), seen   # the forms are distinct launches (24 = 23 in float)
    print(f"forms dtype={dtype} dim={dim}: max err_i {worst:.3g} bound {bound:.3g}")
