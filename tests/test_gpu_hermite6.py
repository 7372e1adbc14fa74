"""GPU: the sixth-order Hermite integrator for all-pairs (nbody_hermite6_*) against a NumPy restatement of the scheme written here
(ref_ajs, ref_step6, ref_run6; the reference has no Hermite, so there are no fixtures): np.longdouble for single evaluations, float64 for
runs.  Conventions (maxrel, e2_of, random_system, cluster, TOL) are those of tests/test_gpu_hermite.py, restated.

Launch-shape boundaries of the sixth order (hermite_plan_for(sz, 2) of csrc/hermite_tile.hpp), each with a size on either side: one LDS tile of 256 records and one
chunk | two tiles, two chunks (256 / 257); one tile per chunk | several (5888 / 5889); one target per lane | two (65535 / 65536, and
65537: a ragged last tile in that regime).  Inside a regime the chunk count varies with the size, but the code path does not (a loop
over the chunk's tiles, a ragged last chunk: 4097, 5889 and 65537 have one), and the plan never goes back to one chunk.

Cost of the NumPy side: longdouble arithmetic runs at some 10 ns per operation, so all targets are compared up to 1000 bodies, a fixed
subset of 256 (first body, the whole last block of 64, random others) up to 20 000 and of 64 (first, last, random others) above.

Measured on an MI355X (max|got - ref| / max|ref|, worst over the sizes): a 1.8e-15, jerk 3.7e-15, snap 5.2e-15 in double; a 9.8e-7,
jerk 2.6e-6, snap 4.3e-6 in float; two steps within 5e-15 except the crackle, 6.9e-14 at dt = 0.05; two-body errors 6.71e-5 / 1.033e-6 /
1.572e-8 / 2.417e-10 (ratios 65.0, 65.7, 65.1), equal to NumPy's to the printed digits; |dE / E| 1.29e-8 and 4.83e-9 (NumPy the same)
against the fourth order's 5.6e-6 and 1.77e-7; the float trajectory at 0.72 x its yardstick (7.07e-7, GPU 5.08e-7).

Per-body bounds in ulps against a wide reference, c != 1 and the ends of the softening range are in tests/test_gpu_hermite_wide.py."""
import ctypes
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TOL = {1: 1e-12, 0: 2e-5}  # the project's bound for a summed force against NumPy (tests/test_gpu_softening.py), reused for jerk and snap
LD = np.longdouble


def maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def npt(dtype):
    return np.float32 if dtype == 0 else np.float64


def e2_of(dtype, eps):
    t = npt(dtype)
    return t(t(eps) * t(eps))


def ref_ajs(m, x, v, acc, c, e2, dt=LD, targets=None, reverse=False):
    """a_i = c sum_j w d, j_i = c sum_j w (u - 3 alpha d), s_i = c sum_j w (b - 6 alpha u + (15 alpha^2 - 3 gamma) d) with d = x_j - x_i,
    u = v_j - v_i, b = acc_j - acc_i, q = |d|^2 + e2, w = m_j q^(-3/2), alpha = d.u / q, gamma = (|u|^2 + d.b) / q, in `dt`.  The self
    pair adds 0 because d = u = b = 0.  reverse: sources summed in reversed order.  (Component-first arrays: long inner loops.)"""
    m, x, v, acc = np.asarray(m, dt), np.asarray(x, dt), np.asarray(v, dt), np.asarray(acc, dt)
    ms, xs, vs, bs = (m[::-1], x[::-1], v[::-1], acc[::-1]) if reverse else (m, x, v, acc)
    xs, vs, bs = xs.T[:, None, :], vs.T[:, None, :], bs.T[:, None, :]
    idx = np.arange(len(m)) if targets is None else np.asarray(targets)
    a, j, s = (np.zeros((x.shape[1], len(idx)), dt) for _ in range(3))
    step = max(1, min(256, (1 << 18) // len(m)))
    for o in range(0, len(idx), step):
        t = idx[o:o + step]
        d, u, b = xs - x[t].T[:, :, None], vs - v[t].T[:, :, None], bs - acc[t].T[:, :, None]
        q = (d * d).sum(0) + dt(e2)
        al = (d * u).sum(0) / q
        ga = ((u * u).sum(0) + (d * b).sum(0)) / q
        w = ms[None, :] / (q * np.sqrt(q))
        a[:, o:o + step] = (w * d).sum(2)
        j[:, o:o + step] = (w * (u - dt(3) * al * d)).sum(2)
        s[:, o:o + step] = (w * (b - dt(6) * al * u + (dt(15) * al * al - dt(3) * ga) * d)).sum(2)
    return dt(c) * a.T, dt(c) * j.T, dt(c) * s.T


def ref_step6(m, x, v, a0, j0, s0, k0, h, c, e2, dt=LD, reverse=False, targets=None):
    """One P(EC)^1 sixth-order step in `dt`; returns x1, v1, a1, j1, s1, k1, xp, vp, ap (rows `targets` only, if given: the predictor
    runs for all bodies, they are the sources)."""
    x, v, a0, j0, s0, k0 = (np.asarray(z, dt) for z in (x, v, a0, j0, s0, k0))
    h = dt(h)
    xp = x + h * (v + h / dt(2) * (a0 + h / dt(3) * (j0 + h / dt(4) * (s0 + h / dt(5) * k0))))
    vp = v + h * (a0 + h / dt(2) * (j0 + h / dt(3) * (s0 + h / dt(4) * k0)))
    ap = a0 + h * (j0 + h / dt(2) * (s0 + h / dt(3) * k0))
    a1, j1, s1 = ref_ajs(m, xp, vp, ap, c, e2, dt, targets=targets, reverse=reverse)
    if targets is not None:
        x, v, a0, j0, s0, xp, vp, ap = (z[targets] for z in (x, v, a0, j0, s0, xp, vp, ap))
    v1 = v + h / dt(2) * (a0 + a1) + h * h / dt(10) * (j0 - j1) + h * h * h / dt(120) * (s0 + s1)
    x1 = x + h / dt(2) * (v + v1) + h * h / dt(10) * (a0 - a1) + h * h * h / dt(120) * (j0 + j1)
    k1 = (dt(60) * (a1 - a0) - h * (dt(24) * j0 + dt(36) * j1) + h * h * (dt(9) * s1 - dt(3) * s0)) / (h * h * h)
    return x1, v1, a1, j1, s1, k1, xp, vp, ap


def ref_start6(m, x, v, c, e2, dt=LD, reverse=False):
    """The two evaluations of the start: a with ap = 0, then a, jerk and snap at (x, v, a)."""
    a, _, _ = ref_ajs(m, x, v, np.zeros(np.shape(x), dt), c, e2, dt, reverse=reverse)
    return ref_ajs(m, x, v, a, c, e2, dt, reverse=reverse)


def ref_run6(m, x, v, h, c, e2, nsteps, dt=np.float64, reverse=False, each=None):
    m, x, v = np.asarray(m, dt), np.asarray(x, dt).copy(), np.asarray(v, dt).copy()
    a, j, s = ref_start6(m, x, v, c, e2, dt, reverse)
    k = np.zeros_like(a)
    for i in range(nsteps):
        x, v, a, j, s, k, _, _, _ = ref_step6(m, x, v, a, j, s, k, h, c, e2, dt, reverse)
        if each:
            each(i + 1, x, v)
    return x, v, a, j, s, k


def ref_energy(m, x, v, c, e2):
    m, x, v = np.asarray(m, np.float64), np.asarray(x, np.float64), np.asarray(v, np.float64)
    d = x[None] - x[:, None]
    inv = 1 / np.sqrt((d * d).sum(-1) + np.float64(e2))
    np.fill_diagonal(inv, 0)
    return 0.5 * (m * (v * v).sum(-1)).sum() - 0.5 * c * (m[:, None] * m[None, :] * inv).sum()


def random_system(nb, dtype, dim, n, seed, c=1.0, dt=0.01):
    rng = np.random.default_rng(seed)
    t = npt(dtype)
    hs = nb.HostSystem(dtype, dim, n)
    hs.m[:] = rng.uniform(0.5, 1.5, n).astype(t) / n
    hs.x[:] = rng.normal(0, 1, (n, dim)).astype(t)
    hs.v[:] = rng.normal(0, 0.3, (n, dim)).astype(t)
    hs.dt, hs.c = dt, c
    return hs


def cluster(nb, dtype, n, seed=2024, dt=0.01):
    """The Gaussian cluster of the energy and trajectory tests: sigma_x = 1, sigma_v = 0.3, m = 1 / N, c = 1."""
    rng = np.random.default_rng(seed)
    t = npt(dtype)
    hs = nb.HostSystem(dtype, 3, n)
    hs.m[:] = t(1.0 / n)
    hs.x[:] = rng.normal(0, 1, (n, 3)).astype(t)
    hs.v[:] = rng.normal(0, 0.3, (n, 3)).astype(t)
    hs.dt, hs.c = dt, 1.0
    return hs


def start(nb, hs, eps):
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite6_start(eps)
    return dev


def targets_of(n):
    """None: all bodies.  Otherwise the fixed subset the NumPy side can afford (module docstring), first and last body included."""
    if n <= 1000:
        return None
    rng = np.random.default_rng(5)
    if n <= 20000:
        tail = np.arange(n - 64, n)
        return np.concatenate(([0], tail, rng.choice(np.arange(1, n - 64), 256 - 65, replace=False)))
    return np.concatenate(([0, n - 1], rng.choice(np.arange(1, n - 1), 62, replace=False)))


def derivs(dev):
    """(a, jerk, snap, crackle) on the device."""
    return dev.download().a, dev.hermite6_read(0), dev.hermite6_read(1), dev.hermite6_read(2)


SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 1000, 4097, 5888, 5889, 65535, 65536, 65537]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_start_against_numpy_longdouble(nb, dtype, dim, n):
    """a, jerk and snap after start; the reference snap is computed from the a the GPU made (its own a is within TOL of that one).
    xp, vp, ap read back as the state that was evaluated, and the crackle as 0."""
    eps = 0.05
    hs = random_system(nb, dtype, dim, n, seed=100 + n)
    dev = start(nb, hs, eps)
    a, j, s, k = derivs(dev)
    xp, vp, ap = (dev.hermite6_read(w) for w in (3, 4, 5))
    dev.close()
    assert all(np.isfinite(z).all() for z in (a, j, s))
    assert np.array_equal(xp, hs.x) and np.array_equal(vp, hs.v) and np.array_equal(ap, a) and not k.any()
    t = targets_of(n)
    ra, rj, rs = ref_ajs(hs.m, hs.x, hs.v, a, hs.c, e2_of(dtype, eps), targets=t)
    pick = (lambda z: z) if t is None else (lambda z: z[t])
    got = [maxrel(pick(g), r) for g, r in ((a, ra), (j, rj), (s, rs))]
    print(f"dtype={dtype} dim={dim} n={n}: a {got[0]:.3g} jerk {got[1]:.3g} snap {got[2]:.3g}")
    assert max(got) <= TOL[dtype], (n, got)


@pytest.mark.parametrize("dtype", [1, 0])
def test_degenerate_inputs(nb, dtype):
    t, eps = npt(dtype), 0.05
    e2 = e2_of(dtype, eps)

    def check(hs, what):
        dev = start(nb, hs, eps)
        a, j, s, _ = derivs(dev)
        dev.close()
        assert all(np.isfinite(z).all() for z in (a, j, s)), what
        refs = ref_ajs(hs.m, hs.x, hs.v, a, hs.c, e2)
        for name, got, ref in zip(("a", "jerk", "snap"), (a, j, s), refs):
            if np.abs(np.asarray(ref, np.float64)).max() == 0:
                assert np.array_equal(got, np.zeros_like(got)), (what, name)
            else:
                assert maxrel(got, ref) <= TOL[dtype], (what, name, maxrel(got, ref))
        return a, j, s

    for n in (3, 300):
        hs = random_system(nb, dtype, 3, n, seed=n)
        hs.x[1] = hs.x[0]  # coincident, different velocities
        check(hs, f"coincident n={n}")
        hs = random_system(nb, dtype, 3, n, seed=n + 1)
        hs.x[2] = hs.x[0] + t(1e-3 * eps) * np.array([1, 0, 0], t)  # a pair at 1e-3 eps
        check(hs, f"close pair n={n}")
        hs = random_system(nb, dtype, 3, n, seed=n + 2)
        hs.x[:] = t(0.25)  # all bodies at one point: a = 0, so b = 0 and the snap is 0 too; the jerk is the velocities' m / eps^3 sum
        a, _, s = check(hs, f"one point n={n}")
        assert np.array_equal(a, np.zeros_like(a)) and np.array_equal(s, np.zeros_like(s))
        hs = random_system(nb, dtype, 3, n, seed=n + 3)
        hs.v[:] = 0  # all velocities zero: the jerk is exactly 0, the snap is the w b and d.b terms only
        a, j, s = check(hs, f"zero velocities n={n}")
        assert np.array_equal(j, np.zeros_like(j))
        m, x, al = np.asarray(hs.m, LD), np.asarray(hs.x, LD), np.asarray(a, LD)
        d, b = x[None] - x[:, None], al[None] - al[:, None]
        q = (d * d).sum(-1) + LD(e2)
        w = m[None] / (q * np.sqrt(q))
        only = LD(hs.c) * (w[:, :, None] * (b - (LD(3) * (d * b).sum(-1) / q)[:, :, None] * d)).sum(1)
        assert maxrel(s, only) <= TOL[dtype], (n, maxrel(s, only))


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [257, 4097])
def test_two_steps_against_numpy_longdouble(nb, n, dim):
    """Two steps in double, each against a longdouble ref_step6 from the state the GPU had before it (downloaded: x, v, a, jerk, snap,
    crackle), so the second step carries a non-zero crackle through the predictor.  ao comes back bit for bit.
    dt = 0.05: the crackle formula divides 60 (a1 - a0) by h^3, so an error delta in a1 becomes 60 delta / h^3 in k1.  A summed a
    carries about 5e-15 max|a| (this file's first test; NumPy's own float64 sum the same), max|k| / max|a| is about 1e4 .. 1e5 for
    these systems, so the bound 1e-12 max|k| needs 60 x 5e-15 / h^3 <= 1e-12 x 1e4, i.e. h >= 0.03: at h = 0.01 a float64 NumPy step is
    itself 4e-12 .. 1.5e-11 away from the longdouble one, at h = 0.05 3e-14 .. 8e-14.  That is the crackle's conditioning in the number
    format, not an allowance: every other quantity is held to the same bound, which they meet at any h."""
    eps = 0.05
    hs = random_system(nb, 1, dim, n, seed=n + dim, dt=0.05)
    hs.ao[:] = np.random.default_rng(3).normal(0, 1, (n, dim))  # must come back bit for bit
    e2 = e2_of(1, eps)
    t = targets_of(n)
    pick = (lambda z: z) if t is None else (lambda z: z[t])
    dev = start(nb, hs, eps)
    for step in (1, 2):
        before = dev.download()
        _, j0, s0, k0 = derivs(dev)
        assert (step == 1) == (not k0.any())
        dev.hermite6_step(eps)
        out = dev.download()
        got = (out.x, out.v, out.a) + tuple(dev.hermite6_read(w) for w in range(6))
        ref = ref_step6(hs.m, before.x, before.v, before.a, j0, s0, k0, hs.dt, hs.c, e2, targets=t)
        for name, g, r in zip(("x", "v", "a", "jerk", "snap", "crackle", "xp", "vp", "ap"), got, ref):
            e = maxrel(pick(g), r)
            print(f"n={n} dim={dim} step {step} {name}: {e:.3g}")
            assert e <= TOL[1], (step, name, e)
        assert np.array_equal(out.ao, hs.ao)
    dev.close()


def two_body(nb, nsteps):
    """Two unit masses on a circular orbit of separation 1, eps = 0.1, c = 1: a rotation with w^2 = 2 c / (1 + e2)^(3/2)
    (tests/test_gpu_hermite.py's two_body)."""
    eps = 0.1
    e2 = e2_of(1, eps)
    w = np.sqrt(2.0 / (1.0 + e2) ** 1.5)
    hs = nb.HostSystem(1, 3, 2)
    hs.m[:] = 1.0
    hs.x[:] = [[0.5, 0, 0], [-0.5, 0, 0]]
    hs.v[:] = [[0, 0.5 * w, 0], [0, -0.5 * w, 0]]
    hs.c, hs.dt = 1.0, 2 * (2 * np.pi / w) / nsteps
    return hs, eps, e2, w


def exact_two_body(w, t):
    p = 0.5 * np.array([np.cos(w * t), np.sin(w * t), 0.0])
    return np.array([p, -p])


def test_order_of_convergence(nb):
    """Max position error over two periods with 50 .. 400 steps: successive ratios in [56, 72] (sixth order: 64; without the crackle
    term of the predictor the scheme is fifth order and gives 32), and up to 200 steps the GPU's error within 1 % of the NumPy float64
    scheme's (6.71e-5, 1.03e-6, 1.57e-8, 2.42e-10 there; at 400 steps rounding is a visible part of 2.4e-10)."""
    errs_gpu, errs_np = [], []
    for nsteps in (50, 100, 200, 400):
        hs, eps, e2, w = two_body(nb, nsteps)
        dev = start(nb, hs, eps)
        eg = 0.0
        for k in range(nsteps):
            dev.hermite6_step(eps)
            eg = max(eg, np.abs(dev.download().x - exact_two_body(w, (k + 1) * hs.dt)).max())
        dev.close()
        en = [0.0]

        def each(k, x, v):
            en[0] = max(en[0], np.abs(x - exact_two_body(w, k * hs.dt)).max())

        ref_run6(hs.m, hs.x, hs.v, hs.dt, hs.c, e2, nsteps, each=each)
        errs_gpu.append(eg)
        errs_np.append(en[0])
        print(f"n={nsteps}: gpu {eg:.4g} numpy {en[0]:.4g}")
        if nsteps <= 200:
            assert abs(eg - en[0]) <= 0.01 * en[0], (nsteps, eg, en[0])
    ratios = [errs_gpu[i] / errs_gpu[i + 1] for i in range(3)]
    print("ratios", ratios)
    assert all(56 <= r <= 72 for r in ratios), ratios


def test_energy_conservation(nb):
    """N = 256 cluster, eps = 0.05, to t = 2: |dE / E| of the GPU's sixth-order run within a factor 2 of ref_run6's (1.29e-8 at dt = 0.02,
    4.83e-9 at 0.01) and below a tenth of the GPU's fourth-order Hermite's at the same dt (NumPy's pair of schemes: 1 / 435 and 1 / 37)."""
    eps = 0.05
    e2 = e2_of(1, eps)
    for dt in (0.02, 0.01):
        nsteps = int(round(2.0 / dt))
        hs = cluster(nb, 1, 256, dt=dt)
        e0 = ref_energy(hs.m, hs.x, hs.v, hs.c, e2)
        x, v = ref_run6(hs.m, hs.x, hs.v, hs.dt, hs.c, e2, nsteps)[:2]
        de_np = abs((ref_energy(hs.m, x, v, hs.c, e2) - e0) / e0)

        dev = start(nb, hs, eps)
        k0, p0 = dev.calc_energies(softening=eps)
        assert abs((k0 + p0) - e0) <= 1e-12 * abs(e0)
        for _ in range(nsteps):
            dev.hermite6_step(eps)
        k1, p1 = dev.calc_energies(softening=eps)
        dev.close()
        de_gpu = abs(((k1 + p1) - (k0 + p0)) / (k0 + p0))

        dev = nb.DeviceSystem.from_host(hs)
        dev.hermite_start(eps)
        for _ in range(nsteps):
            dev.hermite_step(eps)
        k2, p2 = dev.calc_energies(softening=eps)
        dev.close()
        de_4 = abs(((k2 + p2) - (k0 + p0)) / (k0 + p0))
        print(f"dt={dt}: sixth order gpu {de_gpu:.3g} numpy {de_np:.3g} fourth order gpu {de_4:.3g}")
        assert de_np / 2 <= de_gpu <= 2 * de_np, (dt, de_gpu, de_np)
        assert de_gpu < 0.1 * de_4, (dt, de_gpu, de_4)


def test_float_trajectory(nb):
    """N = 1000 cluster, eps = 0.05, dt = 0.01, 100 steps in float.  Yardstick (tests/test_gpu_hermite.py's construction): the distance
    (max|dx| / max|x|) between a NumPy float32 sixth-order run and the float64 one, the larger of forward and reversed source order; the
    GPU float run must be within 4 x of the float64 NumPy run.  Measured on an MI355X: 0.72 x (yardstick 7.07e-7, GPU 5.08e-7), the
fourth-order run's figures: the rounding of the position update sets both."""
    eps, nsteps = 0.05, 100
    hs32 = cluster(nb, 0, 1000)
    m, x, v = hs32.m.astype(np.float64), hs32.x.astype(np.float64), hs32.v.astype(np.float64)  # the same start, exactly
    x64 = ref_run6(m, x, v, np.float64(np.float32(hs32.dt)), hs32.c, e2_of(0, eps), nsteps, np.float64)[0]
    yard = 0.0
    for rev in (False, True):
        xf = ref_run6(hs32.m, hs32.x, hs32.v, hs32.dt, hs32.c, e2_of(0, eps), nsteps, np.float32, reverse=rev)[0]
        assert xf.dtype == np.float32
        yard = max(yard, maxrel(xf, x64))
    dev = start(nb, hs32, eps)
    for _ in range(nsteps):
        dev.hermite6_step(eps)
    got = dev.download().x
    dev.close()
    dist = maxrel(got, x64)
    print(f"yardstick {yard:.3g} gpu {dist:.3g} multiple {dist / yard:.2f}")
    assert dist <= 4 * yard, (dist, yard)


def everything(dev):
    out = dev.download()
    return (out.x, out.v, out.a) + tuple(dev.hermite6_read(w) for w in range(6))


def run_eager(nb, hs, eps, nsteps):
    dev = start(nb, hs, eps)
    for _ in range(nsteps):
        dev.hermite6_step(eps)
    got = everything(dev)
    dev.close()
    return got


def same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("dtype,dim,n", [(1, 3, 4097), (0, 3, 1000), (1, 2, 300), (1, 3, 70001)])
def test_bitwise_repeatable(nb, dtype, dim, n):
    """The same start run twice; start called twice; 20 eager steps against 20 replays of one recorded step; a handle destroyed and made
    again.  70001: two targets per lane."""
    eps, nsteps = 0.05, 20 if n < 70000 else 3
    hs = random_system(nb, dtype, dim, n, seed=n)
    first, second = run_eager(nb, hs, eps, nsteps), run_eager(nb, hs, eps, nsteps)
    assert same(first, second)
    # start twice: the second reads the a of the first, which does not enter a
    dev = start(nb, hs, eps)
    once = everything(dev)
    dev.hermite6_start(eps)
    assert same(once, everything(dev))
    # replays of one recorded step
    g = nb.StepGraph(dev, lambda: dev.hermite6_step(eps))
    for _ in range(nsteps):
        g.launch()
    replayed = everything(dev)
    g.close()
    dev.close()
    assert same(first, replayed)
    # the handle destroyed after the run and made again: restart from the state on the device
    dev = start(nb, hs, eps)
    for _ in range(nsteps):
        dev.hermite6_step(eps)
    mid = everything(dev)
    dev._hermite6.close()
    dev._hermite6 = None
    dev.hermite6_start(eps)  # a, jerk and snap at the corrected state
    again = everything(dev)
    dev._hermite6.close()
    dev._hermite6 = None
    dev.hermite6_start(eps)
    assert same(again, everything(dev))
    dev.close()
    assert same(first, mid)


def test_call_sequence_errors(nb):
    L = nb.lib()
    hs = random_system(nb, 1, 3, 300, seed=1)
    dev = nb.DeviceSystem.from_host(hs)
    st = dev.state()
    stream = ctypes.c_void_p(dev.stream)

    def rc_of(call):
        try:
            call()
        except nb.NbodyError as e:
            return int(re.match(r"nbody backend error (\d+)", str(e)).group(1)), str(e)
        return 0, ""

    h = nb.Hermite6(1, 3, 300, dev.device)
    assert rc_of(lambda: h.step(st, 0.05, dev.stream))[0] == 3  # step before start
    assert rc_of(lambda: h.read(0, dev.stream))[0] == 3
    for other in (nb.Hermite6(1, 3, 301, dev.device), nb.Hermite6(0, 3, 300, dev.device), nb.Hermite6(1, 2, 300, dev.device)):
        assert rc_of(lambda: other.start(st, 0.05, dev.stream))[0] == 1
        assert rc_of(lambda: other.step(st, 0.05, dev.stream))[0] == 1
        other.close()
    window = dev.state(first=10, count=100)
    for call in (h.start, h.step):
        rc, msg = rc_of(lambda: call(window, 0.05, dev.stream))
        assert rc == 1 and "whole system" in msg
        rc, msg = rc_of(lambda: call(st, 0.0, dev.stream))
        assert rc == 1 and "softening" in msg
    h.start(st, 0.05, dev.stream)
    assert rc_of(lambda: h.step(st, 0.0, dev.stream))[0] == 1
    buf = np.zeros(300 * 3 + 1)
    assert L.nbody_hermite6_read(h.h, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, stream) == 1
    assert L.nbody_hermite6_read(h.h, 6, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes - 8, stream) == 1
    assert L.nbody_hermite6_read(h.h, -1, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes - 8, stream) == 1
    # under capture: create and read are refused, and the capture goes on to record a step that replays
    want = run_eager(nb, hs, 0.05, 2)
    assert L.nbody_graph_begin(stream) == 0
    try:
        made = ctypes.c_void_p()
        rc_create = L.nbody_hermite6_create(ctypes.byref(made), 1, 3, 300)
        rc_read = L.nbody_hermite6_read(h.h, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes - 8, stream)
        h.step(st, 0.05, dev.stream)
    finally:
        g = ctypes.c_void_p()
        rc_end = L.nbody_graph_end(stream, ctypes.byref(g))
    assert (rc_create, rc_read, rc_end) == (3, 3, 0) and not made.value
    assert L.nbody_graph_launch(g, stream) == 0 and L.nbody_graph_launch(g, stream) == 0
    dev.sync()  # the stream is out of capture and works
    out = dev.download()
    got = (out.x, out.v, out.a) + tuple(h.read(w, dev.stream) for w in range(6))
    L.nbody_graph_destroy(g)
    assert same(want, got)
    status = nb.all_pairs_status(dev.stream, check=False)
    assert status["rc"] == 0 and not status["failed"]
    # create works again after the capture
    h2 = nb.Hermite6(1, 3, 300, dev.device)
    h2.close()
    h.close()
    dev.close()


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def cli(args, cwd=None):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


HERMITE = ["-n", 1000, "--precision", "double", "--algorithm", "all-pairs", "--workload", "galaxy", "--softening", 0.05, "--integrator",
           "hermite"]
SIXTH = HERMITE + ["--hermite-order", 6]


def read_positions(path):
    raw = open(path, "rb").read()
    n, steps, tsz, dim = struct.unpack("<4I", raw[:16])
    data = np.frombuffer(raw[16:], dtype=np.float32 if tsz == 4 else np.float64)
    return data[: data.size // (n * dim) * n * dim].reshape(-1, n, dim)


def read_energies(path):
    raw = open(path, "rb").read()
    steps, tsz = struct.unpack("<2I", raw[:8])
    return np.frombuffer(raw[8:], dtype=np.float32 if tsz == 4 else np.float64).reshape(-1, 2)


def state_rows(hs):
    """The CLI's --print-state rows (host/system.hpp: components 0 and 1, % .3e)."""
    f = lambda v: "% .3e" % float(v)
    return [f"{i:02d}: m={f(hs.m[i])}, p=({f(hs.x[i][0])}, {f(hs.x[i][1])}), v=({f(hs.v[i][0])}, {f(hs.v[i][1])}), "
            f"f=({f(hs.a[i][0])}, {f(hs.a[i][1])})" for i in range(hs.n)]


def test_cli_sixth_order_is_the_binding_run(nb):
    """-s 20 --csv-detailed --save all with --hermite-order 6: the 21 frames and energy rows are those of hermite6_start and 20
    hermite6_step calls through the binding, bit for bit (the same library calls); the CSV row has the fourth-order run's columns.  -s 20
    --print-state replays one recorded step: the same final rows as 20 eager steps.  --csv-total prints its two lines."""
    hs = nb.build_model(1, 3, "galaxy", 1000)
    dev = nb.DeviceSystem.from_host(hs)
    frames, energies = [dev.download().x.copy()], [dev.calc_energies(softening=0.05)]
    dev.hermite6_start(0.05)
    for _ in range(20):
        dev.hermite6_step(0.05)
        frames.append(dev.download().x.copy())
        energies.append(dev.calc_energies(softening=0.05))
    final = dev.download()
    dev.close()
    with tempfile.TemporaryDirectory() as d:
        r = cli(SIXTH + ["-s", 20, "--csv-detailed", "--save", "all"], cwd=d)
        assert r.returncode == 0, r.stderr
        pos, en = read_positions(os.path.join(d, "positions.bin")), read_energies(os.path.join(d, "energy.bin"))
    assert pos.shape == (21, 1000, 3) and en.shape == (21, 2)
    assert np.array_equal(pos, np.array(frames))
    assert np.array_equal(en, np.array(energies, np.float64))
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("all-pairs,")]
    assert len(rows) == 1 and re.fullmatch(r"all-pairs,3,64,20,1000,\d+\.\d\d,\d+\.\d\d,0\.00", rows[0]), r.stdout
    # the recorded step
    r = cli(SIXTH + ["-s", 20, "--print-state"])
    assert r.returncode == 0, r.stderr
    rows6 = r.stdout.split("Final state:")[1].strip().splitlines()[:hs.n]
    assert rows6 == state_rows(final)
    r = cli(SIXTH + ["-s", 30, "--csv-total"])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "algorithm,dim,precision,nsteps,nbodies,total [s]"
    assert len(lines) == 2 and re.fullmatch(r"all-pairs,3,64,20,1000,\d+\.\d\d", lines[1]), r.stdout


def test_cli_order_four_is_the_run_without_the_flag(nb):
    outs = []
    for extra in (["--hermite-order", 4], [], ["--hermite-order", 6]):
        with tempfile.TemporaryDirectory() as d:
            r = cli(HERMITE + extra + ["-s", 20, "--csv-detailed", "--save", "all"], cwd=d)
            assert r.returncode == 0, r.stderr
            files = (open(os.path.join(d, "positions.bin"), "rb").read(), open(os.path.join(d, "energy.bin"), "rb").read())
        p = cli(HERMITE + extra + ["-s", 20, "--print-state"])
        assert p.returncode == 0, p.stderr
        outs.append(files + (re.sub(r"Total time: .*", "", p.stdout),))
    assert outs[0] == outs[1]
    assert outs[2][0] != outs[0][0] and outs[2][2] != outs[0][2]
