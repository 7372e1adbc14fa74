"""GPU: the fourth-order Hermite integrator for all-pairs (nbody_hermite_*) against a NumPy Hermite written here (the reference has no
Hermite, so there are no fixtures): np.longdouble for single evaluations, float64 for runs.

Launch-shape boundaries of the fourth order (hermite_plan_for(sz, 1) of csrc/hermite_tile.hpp) crossed by the sizes below: the LDS tile of 256 records (255 / 256 / 257: one tile, then two
tiles and two chunks), two targets per lane from 65536 bodies on (65535 / 65536 / 65537), one chunk from 2048 blocks of 128 targets on
(262016: two chunks, 262017: one).

Measured on an MI355X (max|got - ref| / max|ref|, worst over the sizes): a 8.2e-15 and jerk 6.1e-15 in double, a 4.0e-6 and jerk 4.5e-6 in
float (all at N = 262 017); against the softened K1 1.0e-6 in float; one step within 7.4e-15; two-body errors 1.613e-5 / 9.798e-7 /
6.04e-8 / 3.749e-9, equal to NumPy's to the printed digits; |dE / E| 5.6e-6 and 1.77e-7 (NumPy the same) against the leapfrog's 1.36e-2
and 6.87e-3; the float trajectory at 0.72 x its yardstick (7.1e-7).

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

TOL = {1: 1e-12, 0: 2e-5}  # the project's bound for a summed force against NumPy (tests/test_gpu_softening.py), reused for the jerk
LD = np.longdouble


def maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def npt(dtype):
    return np.float32 if dtype == 0 else np.float64


def e2_of(dtype, eps):
    t = npt(dtype)
    return t(t(eps) * t(eps))


def ref_force_jerk(m, x, v, c, e2, dt=LD, targets=None, reverse=False):
    """a_i = c sum_j m_j d q^(-3/2), j_i = c sum_j m_j (u - 3 (d.u)/q d) q^(-3/2); d = x_j - x_i, u = v_j - v_i, q = |d|^2 + e2, in `dt`.
    The self pair adds 0 because d = u = 0.  reverse: sources summed in reversed order."""
    m, x, v = np.asarray(m, dt), np.asarray(x, dt), np.asarray(v, dt)
    if reverse:
        ms, xs, vs = m[::-1], x[::-1], v[::-1]
    else:
        ms, xs, vs = m, x, v
    idx = np.arange(len(m)) if targets is None else np.asarray(targets)
    a, j = np.zeros((len(idx), x.shape[1]), dt), np.zeros((len(idx), x.shape[1]), dt)
    step = max(1, min(256, (1 << 21) // len(m)))
    for s in range(0, len(idx), step):
        t = idx[s:s + step]
        d = xs[None, :, :] - x[t][:, None, :]
        u = vs[None, :, :] - v[t][:, None, :]
        q = (d * d).sum(-1) + dt(e2)
        du = (d * u).sum(-1)
        w = ms[None, :] / (q * np.sqrt(q))
        a[s:s + step] = (w[:, :, None] * d).sum(1)
        j[s:s + step] = (w[:, :, None] * (u - (dt(3) * du / q)[:, :, None] * d)).sum(1)
    return dt(c) * a, dt(c) * j


def ref_step(m, x, v, a0, j0, h, c, e2, dt=LD, reverse=False):
    """One P(EC)^1 Hermite step in `dt`; returns x1, v1, a1, j1, xp, vp."""
    x, v, a0, j0, h = np.asarray(x, dt), np.asarray(v, dt), np.asarray(a0, dt), np.asarray(j0, dt), dt(h)
    xp = x + h * v + h * h / dt(2) * a0 + h * h * h / dt(6) * j0
    vp = v + h * a0 + h * h / dt(2) * j0
    a1, j1 = ref_force_jerk(m, xp, vp, c, e2, dt, reverse=reverse)
    v1 = v + h / dt(2) * (a0 + a1) + h * h / dt(12) * (j0 - j1)
    x1 = x + h / dt(2) * (v + v1) + h * h / dt(12) * (a0 - a1)
    return x1, v1, a1, j1, xp, vp


def ref_run(m, x, v, h, c, e2, nsteps, dt=np.float64, reverse=False, each=None):
    m, x, v = np.asarray(m, dt), np.asarray(x, dt).copy(), np.asarray(v, dt).copy()
    a, j = ref_force_jerk(m, x, v, c, e2, dt, reverse=reverse)
    for k in range(nsteps):
        x, v, a, j, _, _ = ref_step(m, x, v, a, j, h, c, e2, dt, reverse)
        if each:
            each(k + 1, x, v)
    return x, v, a, j


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
    dev.hermite_start(eps)
    return dev


SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 513, 1000, 4097, 20000, 65535, 65536, 65537, 262016, 262017]


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_force_jerk_against_numpy_longdouble(nb, dtype, dim):
    eps, worst = 0.05, {}
    for n in SIZES:
        hs = random_system(nb, dtype, dim, n, seed=100 + n)
        dev = start(nb, hs, eps)
        a, j = dev.download().a, dev.hermite_jerk()
        dev.close()
        assert np.isfinite(a).all() and np.isfinite(j).all()
        if n < 20000:
            t = None
        else:  # a fixed random subset of targets (first and last body included) keeps the CPU side in seconds
            k = 256 if n == 20000 else 64
            t = np.concatenate(([0, n - 1], np.random.default_rng(5).choice(np.arange(1, n - 1), k - 2, replace=False)))
        ra, rj = ref_force_jerk(hs.m, hs.x, hs.v, hs.c, e2_of(dtype, eps), targets=t)
        ga, gj = (a, j) if t is None else (a[t], j[t])
        worst[n] = (maxrel(ga, ra), maxrel(gj, rj))
        print(f"dtype={dtype} dim={dim} n={n}: a {worst[n][0]:.3g} jerk {worst[n][1]:.3g}")
        assert worst[n][0] <= TOL[dtype] and worst[n][1] <= TOL[dtype], (n, worst[n])


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_acceleration_agrees_with_the_softened_k1(nb, dtype, dim):
    """Two roundings of the same sum (other slices, other chunks): within TOL, bitwise equality is not asked."""
    for n in (65, 1000, 4097, 70001):
        hs = random_system(nb, dtype, dim, n, seed=7 + n)
        dev = start(nb, hs, 0.05)
        a = dev.download().a
        dev.all_pairs_softened_force(0.05)
        k1 = dev.download().a
        dev.close()
        r = maxrel(a, k1)
        print(f"dtype={dtype} dim={dim} n={n}: {r:.3g}")
        assert r <= TOL[dtype], (n, r)


@pytest.mark.parametrize("dtype", [1, 0])
def test_degenerate_inputs(nb, dtype):
    t, eps = npt(dtype), 0.05
    e2 = e2_of(dtype, eps)

    def check(hs, what):
        dev = start(nb, hs, eps)
        a, j = dev.download().a, dev.hermite_jerk()
        dev.close()
        assert np.isfinite(a).all() and np.isfinite(j).all(), what
        ra, rj = ref_force_jerk(hs.m, hs.x, hs.v, hs.c, e2)
        for got, ref in ((a, ra), (j, rj)):
            if np.abs(np.asarray(ref, np.float64)).max() == 0:
                assert np.array_equal(got, np.zeros_like(got)), what
            else:
                assert maxrel(got, ref) <= TOL[dtype], (what, maxrel(got, ref))
        return a, j

    for n in (3, 300, 4099):
        hs = random_system(nb, dtype, 3, n, seed=n)
        hs.x[1] = hs.x[0]  # coincident, different velocities
        check(hs, f"coincident n={n}")
        hs = random_system(nb, dtype, 3, n, seed=n + 1)
        hs.x[2] = hs.x[0] + t(1e-3 * eps) * np.array([1, 0, 0], t)  # a pair at 1e-3 eps
        check(hs, f"close pair n={n}")
        hs = random_system(nb, dtype, 3, n, seed=n + 2)
        hs.x[:] = t(0.25)  # all bodies at one point: a = 0, the jerk is the velocities' m / eps^3 sum
        a, _ = check(hs, f"one point n={n}")
        assert np.array_equal(a, np.zeros_like(a))
        hs = random_system(nb, dtype, 3, n, seed=n + 3)
        hs.v[:] = 0  # all velocities zero: jerk exactly 0 in every component
        _, j = check(hs, f"zero velocities n={n}")
        assert np.array_equal(j, np.zeros_like(j))


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("n", [257, 4097])
def test_one_step_against_numpy_longdouble(nb, n, dim):
    eps = 0.05
    hs = random_system(nb, 1, dim, n, seed=n + dim, dt=0.01)
    hs.ao[:] = np.random.default_rng(3).normal(0, 1, (n, dim))  # must come back bit for bit
    e2 = e2_of(1, eps)
    dev = start(nb, hs, eps)
    dev.hermite_step(eps)
    out, jerk = dev.download(), dev.hermite_jerk()
    xp, vp = dev.hermite.read(1, dev.stream), dev.hermite.read(2, dev.stream)
    dev.close()
    a0, j0 = ref_force_jerk(hs.m, hs.x, hs.v, hs.c, e2)
    x1, v1, a1, j1, rxp, rvp = ref_step(hs.m, hs.x, hs.v, a0, j0, hs.dt, hs.c, e2)
    for name, got, ref in (("x", out.x, x1), ("v", out.v, v1), ("a", out.a, a1), ("jerk", jerk, j1), ("xp", xp, rxp), ("vp", vp, rvp)):
        r = maxrel(got, ref)
        print(f"n={n} dim={dim} {name}: {r:.3g}")
        assert r <= TOL[1], (name, r)
    assert np.array_equal(out.ao, hs.ao)


def two_body(nb, nsteps):
    """Two unit masses on a circular orbit of separation 1, eps = 0.1, c = 1: a rotation with w^2 = 2 c / (1 + e2)^(3/2)."""
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
    """Max position error over two periods with n = 200 .. 1600 steps: the GPU's within 1 % of the NumPy float64 Hermite's, successive
    ratios in [14, 18] (fourth order: 16; a second-order scheme gives 4)."""
    errs_gpu, errs_np = [], []
    for nsteps in (200, 400, 800, 1600):
        hs, eps, e2, w = two_body(nb, nsteps)
        dev = start(nb, hs, eps)
        eg = 0.0
        for k in range(nsteps):
            dev.hermite_step(eps)
            eg = max(eg, np.abs(dev.download().x - exact_two_body(w, (k + 1) * hs.dt)).max())
        dev.close()
        en = [0.0]

        def each(k, x, v):
            en[0] = max(en[0], np.abs(x - exact_two_body(w, k * hs.dt)).max())

        ref_run(hs.m, hs.x, hs.v, hs.dt, hs.c, e2, nsteps, each=each)
        errs_gpu.append(eg)
        errs_np.append(en[0])
        print(f"n={nsteps}: gpu {eg:.4g} numpy {en[0]:.4g}")
        assert abs(eg - en[0]) <= 0.01 * en[0], (nsteps, eg, en[0])
    ratios = [errs_gpu[i] / errs_gpu[i + 1] for i in range(3)]
    print("ratios", ratios)
    assert all(14 <= r <= 18 for r in ratios), ratios


def test_energy_conservation(nb):
    """N = 256 cluster, eps = 0.05, to t = 2: |dE / E| of the GPU Hermite within a factor 2 of the NumPy Hermite's and below a tenth of
    the GPU leapfrog's (softened K1 + K3, ao = 0 at the first step) at the same dt."""
    eps = 0.05
    e2 = e2_of(1, eps)
    for dt in (0.02, 0.01):
        nsteps = int(round(2.0 / dt))
        hs = cluster(nb, 1, 256, dt=dt)
        e0 = ref_energy(hs.m, hs.x, hs.v, hs.c, e2)
        x, v, _, _ = ref_run(hs.m, hs.x, hs.v, hs.dt, hs.c, e2, nsteps)
        de_np = abs((ref_energy(hs.m, x, v, hs.c, e2) - e0) / e0)

        dev = start(nb, hs, eps)
        k0, p0 = dev.calc_energies(softening=eps)
        assert abs((k0 + p0) - e0) <= 1e-12 * abs(e0)
        for _ in range(nsteps):
            dev.hermite_step(eps)
        k1, p1 = dev.calc_energies(softening=eps)
        dev.close()
        de_gpu = abs(((k1 + p1) - (k0 + p0)) / (k0 + p0))

        dev = nb.DeviceSystem.from_host(hs)
        for _ in range(nsteps):
            dev.all_pairs_softened_force(eps)
            dev.accelerate_step()
        k2, p2 = dev.calc_energies(softening=eps)
        dev.close()
        de_leap = abs(((k2 + p2) - (k0 + p0)) / (k0 + p0))
        print(f"dt={dt}: hermite gpu {de_gpu:.3g} numpy {de_np:.3g} leapfrog gpu {de_leap:.3g}")
        assert de_np / 2 <= de_gpu <= 2 * de_np, (dt, de_gpu, de_np)
        assert de_gpu < 0.1 * de_leap, (dt, de_gpu, de_leap)


def test_float_trajectory(nb):
    """N = 1000 cluster, eps = 0.05, dt = 0.01, 100 steps in float.  Yardstick: the distance (max|dx| / max|x|) between a NumPy float32
    Hermite run and the float64 one, the larger of forward and reversed source order; the GPU float run must be within 4 x of the
    float64 NumPy run.  Measured on an MI355X: 0.72 x (yardstick 7.1e-7, GPU 5.08e-7): the rounding of the position update sets it."""
    eps, nsteps = 0.05, 100
    hs32 = cluster(nb, 0, 1000)
    m, x, v = hs32.m.astype(np.float64), hs32.x.astype(np.float64), hs32.v.astype(np.float64)  # the same start, exactly
    x64, _, _, _ = ref_run(m, x, v, np.float64(np.float32(hs32.dt)), hs32.c, e2_of(0, eps), nsteps, np.float64)
    yard = 0.0
    for rev in (False, True):
        xf, _, _, _ = ref_run(hs32.m, hs32.x, hs32.v, hs32.dt, hs32.c, e2_of(0, eps), nsteps, np.float32, reverse=rev)
        yard = max(yard, maxrel(xf, x64))
    dev = start(nb, hs32, eps)
    for _ in range(nsteps):
        dev.hermite_step(eps)
    got = dev.download().x
    dev.close()
    dist = maxrel(got, x64)
    print(f"yardstick {yard:.3g} gpu {dist:.3g} multiple {dist / yard:.2f}")
    assert dist <= 4 * yard, (dist, yard)


def run_eager(nb, hs, eps, nsteps):
    dev = start(nb, hs, eps)
    for _ in range(nsteps):
        dev.hermite_step(eps)
    out, j = dev.download(), dev.hermite_jerk()
    dev.close()
    return out, j


def same(a, b):
    return all(np.array_equal(getattr(a[0], k), getattr(b[0], k)) for k in ("x", "v", "a")) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype,dim,n", [(1, 3, 4097), (0, 3, 1000), (1, 2, 300), (1, 3, 70001)])
def test_bitwise_repeatable(nb, dtype, dim, n):
    """The same start run twice; 20 eager steps against 20 replays of one recorded step; a handle destroyed and made again."""
    eps, nsteps = 0.05, 20 if n < 70000 else 3
    hs = random_system(nb, dtype, dim, n, seed=n)
    first, second = run_eager(nb, hs, eps, nsteps), run_eager(nb, hs, eps, nsteps)
    assert same(first, second)
    # replays of one recorded step
    dev = start(nb, hs, eps)
    g = nb.StepGraph(dev, lambda: dev.hermite_step(eps))
    for _ in range(nsteps):
        g.launch()
    replayed = (dev.download(), dev.hermite_jerk())
    g.close()
    dev.close()
    assert same(first, replayed)
    # the handle destroyed half way and made again: restart from the state on the device
    dev = start(nb, hs, eps)
    for _ in range(nsteps):
        dev.hermite_step(eps)
    mid = (dev.download(), dev.hermite_jerk())
    dev._hermite.close()
    dev._hermite = None
    dev.hermite_start(eps)  # a and the jerk at the corrected state
    again_a, again_j = dev.download().a, dev.hermite_jerk()
    dev._hermite.close()
    dev._hermite = None
    dev.hermite_start(eps)
    assert np.array_equal(dev.download().a, again_a) and np.array_equal(dev.hermite_jerk(), again_j)
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

    h = nb.Hermite(1, 3, 300, dev.device)
    assert rc_of(lambda: h.step(st, 0.05, dev.stream))[0] == 3  # step before force_jerk
    assert rc_of(lambda: h.read(0, dev.stream))[0] == 3
    for other in (nb.Hermite(1, 3, 301, dev.device), nb.Hermite(0, 3, 300, dev.device), nb.Hermite(1, 2, 300, dev.device)):
        assert rc_of(lambda: other.force_jerk(st, 0.05, dev.stream))[0] == 1
        assert rc_of(lambda: other.step(st, 0.05, dev.stream))[0] == 1
        other.close()
    h.force_jerk(st, 0.05, dev.stream)
    buf = np.zeros(300 * 3 + 1)
    assert L.nbody_hermite_read(h.h, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, stream) == 1
    assert L.nbody_hermite_read(h.h, 3, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes - 8, stream) == 1
    # under capture: create and read are refused, and the capture goes on to record a step that replays
    want = run_eager(nb, hs, 0.05, 2)
    assert L.nbody_graph_begin(stream) == 0
    try:
        made = ctypes.c_void_p()
        rc_create = L.nbody_hermite_create(ctypes.byref(made), 1, 3, 300)
        rc_read = L.nbody_hermite_read(h.h, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes - 8, stream)
        h.step(st, 0.05, dev.stream)
    finally:
        g = ctypes.c_void_p()
        rc_end = L.nbody_graph_end(stream, ctypes.byref(g))
    assert (rc_create, rc_read, rc_end) == (3, 3, 0) and not made.value
    assert L.nbody_graph_launch(g, stream) == 0 and L.nbody_graph_launch(g, stream) == 0
    dev.sync()  # the stream is out of capture and works
    got = (dev.download(), h.read(0, dev.stream))
    L.nbody_graph_destroy(g)
    assert same(want, got)
    status = nb.all_pairs_status(dev.stream, check=False)
    assert status["rc"] == 0 and not status["failed"]
    # create works again after the capture
    h2 = nb.Hermite(1, 3, 300, dev.device)
    h2.close()
    h.close()
    dev.close()


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------
def cli(args, cwd=None):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


BASE = ["-n", 1000, "--precision", "double", "--algorithm", "all-pairs", "--workload", "galaxy", "--softening", 0.05]
HERMITE = BASE + ["--integrator", "hermite"]


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


def test_cli_detailed_frames_and_energies(nb):
    """-s 20 --csv-detailed --save all: 21 frames within TOL x 100 of a NumPy float64 Hermite run from the same model (20 steps of
    accumulated rounding: the allowance tests/test_gpu_softening.py gives its 100-step run), the energy rows within 1e-7 of
    calc_energies(softening) on the NumPy run's (x, v).  Extent of the galaxy at n = 1000: max|x| = 150 (printed); the frames came out within 1.9e-15 of the NumPy run, so a pair term at the
    softening length moves by 150 x 1.9e-15 / 0.05 = 6e-12 relative, far inside 1e-7."""
    hs = nb.build_model(1, 3, "galaxy", 1000)
    assert hs.n == 1000
    print("extent max|x| =", np.abs(hs.x).max())
    e2 = e2_of(1, 0.05)
    frames, states = [hs.x.astype(np.float64).copy()], [(hs.x.copy(), hs.v.copy())]
    ref_run(hs.m, hs.x, hs.v, hs.dt, hs.c, e2, 20, each=lambda k, x, v: (frames.append(x.copy()), states.append((x.copy(), v.copy()))))
    with tempfile.TemporaryDirectory() as d:
        r = cli(HERMITE + ["-s", 20, "--csv-detailed", "--save", "all"], cwd=d)
        assert r.returncode == 0, r.stderr
        pos, en = read_positions(os.path.join(d, "positions.bin")), read_energies(os.path.join(d, "energy.bin"))
    assert pos.shape == (21, 1000, 3) and en.shape == (21, 2)
    worst = max(maxrel(pos[k], frames[k]) for k in range(21))
    print(f"worst frame {worst:.3g}")
    assert worst <= TOL[1] * 100
    for k in (0, 1, 10, 20):
        scratch = nb.HostSystem(1, 3, 1000)
        scratch.m[:], scratch.x[:], scratch.v[:] = hs.m, states[k][0], states[k][1]
        scratch.dt, scratch.c = hs.dt, hs.c
        dev = nb.DeviceSystem.from_host(scratch)
        ke, pe = dev.calc_energies(softening=0.05)
        dev.close()
        assert abs(en[k][0] - ke) <= 1e-7 * abs(ke) and abs(en[k][1] - pe) <= 1e-7 * abs(pe), (k, en[k], ke, pe)
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("all-pairs,")]
    assert len(rows) == 1 and re.fullmatch(r"all-pairs,3,64,20,1000,\d+\.\d\d,\d+\.\d\d,0\.00", rows[0]), r.stdout


def test_cli_recorded_step(nb):
    """-s 20 --print-state replays one recorded step: the final rows are those of 20 eager steps through the binding."""
    r = cli(HERMITE + ["-s", 20, "--print-state"])
    assert r.returncode == 0, r.stderr
    hs = nb.build_model(1, 3, "galaxy", 1000)
    out, _ = run_eager(nb, hs, 0.05, nb.executed_steps(20, False))
    final = r.stdout.split("Final state:")[1].strip().splitlines()[:hs.n]
    assert final == state_rows(out)
    leap = cli(BASE + ["-s", 20, "--print-state"])
    assert leap.returncode == 0 and leap.stdout.split("Final state:")[1].strip().splitlines()[:hs.n] != final


def test_cli_csv_total(nb):
    r = cli(HERMITE + ["-s", 30, "--csv-total"])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "algorithm,dim,precision,nsteps,nbodies,total [s]"
    assert len(lines) == 2 and re.fullmatch(r"all-pairs,3,64,20,1000,\d+\.\d\d", lines[1]), r.stdout


def test_cli_default_integrator_is_the_leapfrog(nb):
    outs = []
    for extra in (["--integrator", "leapfrog"], []):
        with tempfile.TemporaryDirectory() as d:
            r = cli(BASE + extra + ["-s", 20, "--csv-detailed", "--save", "all"], cwd=d)
            assert r.returncode == 0, r.stderr
            outs.append((open(os.path.join(d, "positions.bin"), "rb").read(), open(os.path.join(d, "energy.bin"), "rb").read()))
    assert outs[0] == outs[1]
    with tempfile.TemporaryDirectory() as d:
        r = cli(HERMITE + ["-s", 20, "--csv-detailed", "--save", "all"], cwd=d)
        assert r.returncode == 0, r.stderr
        assert open(os.path.join(d, "positions.bin"), "rb").read() != outs[0][0]
