"""GPU: octree quadrupole moments — the pass against the tensor summed directly in NumPy, the quadrupole walk against the expansion
and against a NumPy direct sum written here, its invariants against the monopole walk (counters; theta so small that only bodies are
accepted), its bitwise invariances (shard windows, build forms, recorded steps, repeated calls), its phase-order errors and the
CLI's --quadrupole."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ROOT_TOL = {1: 1e-11, 0: 1e-4}
PROBE_TOL = {1: 1e-12, 0: 1e-5}


def np_t(dtype):
    return np.float64 if dtype == 1 else np.float32


def quad_ref(m, x, dt=np.longdouble):
    """sum m (3 d d^T - |d|^2 I) about the centre of mass, d over the system's own dimensions: the NQ stored components."""
    m, x = np.asarray(m, dt), np.asarray(x, dt)
    p = (m[:, None] * x).sum(0) / m.sum()
    d = x - p
    r2 = (d * d).sum(1)
    dim = x.shape[1]
    out = []
    for u in range(dim):
        for v in range(u, dim):
            e = 3 * d[:, u] * d[:, v] - (r2 if u == v else 0)
            out.append((m * e).sum())
    return np.array(out, dt), p


def expansion(m, x, probe, c, dt=np.longdouble, eps=0.0):
    """Monopole and monopole + quadrupole acceleration at `probe` from the bodies (m, x), expanded about their centre of mass.
    eps: the walk's monopole term is the reference's m d / (|d| + eps)^3 (eps = the machine epsilon of T); the quadrupole term has none."""
    q, p = quad_ref(m, x, dt)
    dim = x.shape[1]
    Q = np.zeros((dim, dim), dt)
    k = 0
    for u in range(dim):
        for v in range(u, dim):
            Q[u, v] = Q[v, u] = q[k]
            k += 1
    d = p - np.asarray(probe, dt)
    y = 1 / np.sqrt((d * d).sum())
    mono = np.asarray(m, dt).sum() * d / (np.sqrt((d * d).sum()) + dt(eps)) ** 3
    qd = Q @ d
    return dt(c) * mono, dt(c) * (mono - qd * y ** 5 + dt(2.5) * (d @ qd) * d * y ** 7)


def direct(m, x, c, targets=None):
    """c * sum_{j != i} m_j (x_j - x_i) / |x_j - x_i|^3 in float64."""
    m, x = np.asarray(m, np.float64), np.asarray(x, np.float64)
    idx = np.arange(len(m)) if targets is None else np.asarray(targets)
    out = np.zeros((len(idx), x.shape[1]))
    for s in range(0, len(idx), 256):
        t = idx[s:s + 256]
        d = x[None, :, :] - x[t][:, None, :]
        r2 = (d * d).sum(-1)
        r2[r2 == 0] = np.inf
        out[s:s + 256] = ((m[None, :] / (r2 * np.sqrt(r2)))[:, :, None] * d).sum(1)
    return c * out


def rel_errors(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)


def system(nb, dtype, dim, x, m, c=1.0, dt=0.01):
    hs = nb.HostSystem(dtype, dim, len(m))
    hs.m[:], hs.x[:] = np.asarray(m, np_t(dtype)), np.asarray(x, np_t(dtype))
    hs.c, hs.dt = c, dt
    return hs


def quad_force(nb, dev, theta):
    dev.octree_force(theta, quadrupole=True)
    return dev.download().a.copy()


def mono_force(nb, dev, theta):
    dev.octree_force(theta)
    return dev.download().a.copy()


def workloads(dim):
    return ("galaxy", "plummer", "uniform") if dim == 3 else ("galaxy", "uniform")  # (the Plummer sphere is a 3D model)


def deep_system(nb, dtype, dim):
    """test_gpu_octree.py's below-the-key-depth case: escapers inflate the root cube, a core lies far below the key resolution, and in
    double close pairs are split 35 - 45 levels down."""
    rng = np.random.default_rng(11 + dim)
    n = 2000
    x = rng.uniform(-1.0, 1.0, (n, dim))
    x[0] = 9000.0
    x[1] = -9000.0
    x[100:200] = 0.25 + 2e-4 * rng.standard_normal((100, dim))
    if dtype == 1:
        for k in range(6):
            x[300 + 2 * k + 1] = x[300 + 2 * k] + 10.0 ** (-7 - k // 2)
    m = rng.uniform(0.5, 2.0, n)
    return system(nb, dtype, dim, x, m)


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_root_quadrupole_against_numpy(nb, dtype, dim):
    cases = [nb.build_model(dtype, dim, wl, n) for wl in workloads(dim) for n in (1000, 5000)]
    cases.append(deep_system(nb, dtype, dim))
    for form in (3, 1):
        for hs in cases:
            dev = nb.DeviceSystem.from_host(hs)
            dev.octree.set_build(form)
            dev.octree_force(0.5, quadrupole=True)
            got = dev.octree.read_root_quadrupole(dev.stream)
            dev.octree.info(dev.stream)
            dev.close()
            want, _ = quad_ref(hs.m, hs.x)
            err = np.abs(got.astype(np.longdouble) - want).max() / np.abs(want).max()
            assert err <= ROOT_TOL[dtype], (form, hs.n, float(err))


@pytest.mark.parametrize("dtype", [1, 0])
def test_root_quadrupole_of_tiny_systems(nb, dtype):
    """One body: the root is a leaf, Q = 0.  Two bodies: Q of the pair about its centre of mass."""
    for dim in (3, 2):
        hs = system(nb, dtype, dim, [[0.5] * dim], [2.0])
        dev = nb.DeviceSystem.from_host(hs)
        dev.octree_force(0.5, quadrupole=True)
        assert not dev.octree.read_root_quadrupole(dev.stream).any()
        dev.close()
        hs = system(nb, dtype, dim, [[0.5] * dim, [-0.25] + [0.125] * (dim - 1)], [2.0, 1.0])
        dev = nb.DeviceSystem.from_host(hs)
        dev.octree_force(0.5, quadrupole=True)
        got = dev.octree.read_root_quadrupole(dev.stream)
        want, _ = quad_ref(hs.m, hs.x)
        assert np.abs(got - want).max() <= ROOT_TOL[dtype] * np.abs(want).max()
        dev.close()


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_one_cluster_one_probe(nb, dtype, dim):
    """A compact ball around (1, ..., 1) and one light probe at (-3, ..., -3): the root is opened, the ball's cell is accepted as
    one node (the probe's counters: the root and the 2^dim children examined, 2^dim terms), so the probe's acceleration is the
    expansion of the ball about its centre of mass."""
    rng = np.random.default_rng(5 + dim)
    k = 40
    ball = 1.0 + 0.3 * rng.uniform(-1, 1, (k, dim)) / np.sqrt(dim)
    x = np.vstack([ball, -3.0 * np.ones((1, dim))])
    m = np.concatenate([rng.uniform(0.5, 1.5, k) / k, [1e-3]])
    hs = system(nb, dtype, dim, x, m)
    xs, ms = hs.x.astype(np.float64), hs.m.astype(np.float64)  # the values the device holds
    dev = nb.DeviceSystem.from_host(hs)
    dev.octree.enable_counters(True)
    theta = 0.7
    aq = quad_force(nb, dev, theta)[k]
    cnt = dev.octree.read_counters(dev.stream)[k]
    assert list(cnt) == [1 + (1 << dim), 1 << dim], cnt
    am = mono_force(nb, dev, theta)[k]
    dev.close()
    mono, want = expansion(ms[:k], xs[:k], xs[k], hs.c)
    assert np.abs(aq - want).max() <= PROBE_TOL[dtype] * np.abs(want).max(), (aq, want)
    assert np.abs(am - mono).max() <= PROBE_TOL[dtype] * np.abs(mono).max()
    exact = direct(ms, xs, hs.c, [k])[0]
    eq, em = np.linalg.norm(aq - exact), np.linalg.norm(am - exact)
    assert eq < 0.2 * em, (eq, em)


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_one_cluster_one_probe_at_large_and_small_scales(nb, dtype, dim):
    """The term stays finite and right where f32's y^5 or y^7 alone would not be (|d| ~ 2e-6 and ~ 7e6).
    Large: test_one_cluster_one_probe's geometry times 1e6, at theta 0.5 (the root cube's +-1 margin no longer counts, so the root
    is 0.6 of its distance to the probe, not 0.9; the ball's cell 0.3).  Small, theta 0.7: the root cube always contains the origin and +-1, so a tiny system
    sits deep in the tree; a massless anchor at (1, -1, ...) makes the root exactly [-2, 2]^dim, the ball fills [1.2u, 1.8u]^dim,
    u = 2^-22, and the probe sits at (-3u, ...): the cell [0, 4u]^dim, which holds the ball and nothing else, is accepted."""
    rng = np.random.default_rng(15 + dim)
    k = 40
    eps = float(np.finfo(np_t(dtype)).eps)
    for scale in (1e6, 2.0 ** -22):
        theta = 0.5 if scale > 1 else 0.7
        if scale > 1:
            ball = scale * (1.0 + 0.3 * rng.uniform(-1, 1, (k, dim)) / np.sqrt(dim))
            extra = [-3.0 * scale * np.ones(dim)]
            m = np.concatenate([rng.uniform(0.5, 1.5, k) / k, [1e-3]])
        else:
            ball = scale * rng.uniform(1.2, 1.8, (k, dim))
            extra = [-3.0 * scale * np.ones(dim), np.array([1.0] + [-1.0] * (dim - 1))]
            m = np.concatenate([rng.uniform(0.5, 1.5, k) / k, [1e-3, 0.0]])
        hs = system(nb, dtype, dim, np.vstack([ball] + [e[None, :] for e in extra]), m)
        xs, ms = hs.x.astype(np.float64), hs.m.astype(np.float64)
        dev = nb.DeviceSystem.from_host(hs)
        dev.octree.enable_counters(True)
        aq = quad_force(nb, dev, theta)
        cnt = dev.octree.read_counters(dev.stream)[k]
        am = mono_force(nb, dev, theta)[k]
        dev.octree.info(dev.stream)
        dev.close()
        assert np.isfinite(aq).all(), scale
        aq = aq[k]
        if scale > 1:
            assert list(cnt) == [1 + (1 << dim), 1 << dim], cnt
        mono, want = expansion(ms[:k], xs[:k], xs[k], hs.c, eps=eps)
        assert np.abs(aq - want).max() <= PROBE_TOL[dtype] * np.abs(want).max(), (scale, aq, want)
        assert np.abs(am - mono).max() <= PROBE_TOL[dtype] * np.abs(mono).max(), (scale, am, mono)
        if scale > 1:  # (at the small scale the walk's eps term, the reference's, is larger than either expansion's error)
            exact = direct(ms, xs, hs.c, [k])[0]
            assert np.linalg.norm(aq - exact) < 0.2 * np.linalg.norm(am - exact)


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_invariants_against_the_monopole_walk(nb, dtype, dim):
    hs = nb.build_model(dtype, dim, "galaxy", 4096)
    dev = nb.DeviceSystem.from_host(hs)
    t = dev.octree
    t.enable_counters(True)
    mono_force(nb, dev, 0.5)
    plain = t.read_counters(dev.stream).copy()
    quad_force(nb, dev, 0.5)
    assert np.array_equal(t.read_counters(dev.stream), plain)
    # theta so small that no cell is accepted: only bodies, and the walk is the monopole walk's bit for bit
    a0 = mono_force(nb, dev, 1e-9)
    a1 = quad_force(nb, dev, 1e-9)
    assert np.array_equal(a0, a1)
    dev.close()


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim, workload", [(3, "galaxy"), (3, "plummer"), (3, "uniform"), (2, "galaxy"), (2, "uniform")])
def test_accuracy_against_the_direct_sum(nb, dtype, dim, workload):
    hs = nb.build_model(dtype, dim, workload, 4096)
    exact = direct(hs.m, hs.x, hs.c)
    dev = nb.DeviceSystem.from_host(hs)
    for theta, ratio in ((0.5, 0.4), (0.7, 0.5)):
        em = rel_errors(mono_force(nb, dev, theta), exact)
        eq = rel_errors(quad_force(nb, dev, theta), exact)
        rms_m, rms_q = np.sqrt((em ** 2).mean()), np.sqrt((eq ** 2).mean())
        print(f"{workload} {dim}D dtype {dtype} theta {theta}: rms {rms_m:.3g} -> {rms_q:.3g}, "
              f"p99 {np.percentile(em, 99):.3g} -> {np.percentile(eq, 99):.3g}")
        assert rms_q <= ratio * rms_m, (theta, rms_q, rms_m)
        assert np.percentile(eq, 99) <= np.percentile(em, 99), theta
    dev.close()


@pytest.mark.parametrize("dtype", [1, 0])
def test_bitwise_invariances(nb, dtype):
    for dim in (3, 2):
        hs = nb.build_model(dtype, dim, "plummer" if dim == 3 else "uniform", 9000)
        dev = nb.DeviceSystem.from_host(hs)
        t = dev.octree
        whole = quad_force(nb, dev, 0.5)
        assert np.array_equal(quad_force(nb, dev, 0.5), whole)  # repeated calls
        for parts in (2, 7):
            dev.upload(hs)
            for p in range(parts):
                f, e = nb.shard_range(hs.n, p, parts)
                t.compute_quadrupole_force(dev.state(f, e - f), 0.5, dev.stream)
            assert np.array_equal(dev.download().a, whole), parts
        q3 = t.read_root_quadrupole(dev.stream)
        t.set_build(1)
        assert np.array_equal(quad_force(nb, dev, 0.5), whole)
        assert np.array_equal(t.read_root_quadrupole(dev.stream), q3)
        t.info(dev.stream)
        t.set_build(0)
        dev.close()
    # build forms 1 and 3 below the key depth
    hs = deep_system(nb, dtype, 3)
    out = []
    for form in (1, 3):
        dev = nb.DeviceSystem.from_host(hs)
        dev.octree.set_build(form)
        out.append((quad_force(nb, dev, 0.5), dev.octree.read_root_quadrupole(dev.stream)))
        dev.octree.info(dev.stream)
        dev.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_recorded_step_replays_the_eager_result(nb):
    n = 9000
    d1 = nb.DeviceSystem.from_host(nb.build_model(1, 3, "galaxy", n))
    for _ in range(3):
        d1.octree_force(0.5, quadrupole=True)
        d1.accelerate_step()
    d1.sync()
    d2 = nb.DeviceSystem.from_host(nb.build_model(1, 3, "galaxy", n))
    d2.octree_force(0.5, quadrupole=True)  # the quadrupole array is allocated outside the capture
    d2.upload(nb.build_model(1, 3, "galaxy", n))
    g = nb.StepGraph(d2, lambda: (d2.octree_force(0.5, quadrupole=True), d2.accelerate_step()))
    for _ in range(3):
        g.launch()
    d2.sync()
    a, b = d1.download(), d2.download()
    assert np.array_equal(a.x, b.x) and np.array_equal(a.a, b.a)
    g.close()
    d1.close()
    d2.close()


def test_first_pass_under_capture_is_refused(nb):
    dev = nb.DeviceSystem.from_host(nb.build_model(1, 3, "galaxy", 2000))
    t, st = dev.octree, dev.state()
    t.clear(dev.stream)
    t.compute_bounds(st, dev.stream)
    t.insert(st, dev.stream)
    t.compute_tree(dev.stream)
    with pytest.raises(nb.NbodyError, match="call once before capture"):
        nb.StepGraph(dev, lambda: t.compute_quadrupoles(dev.stream))
    dev.close()


def test_phase_order_and_walk_form_errors(nb):
    dev = nb.DeviceSystem.from_host(nb.build_model(1, 3, "galaxy", 3000))
    t, st = dev.octree, dev.state()
    with pytest.raises(nb.NbodyError, match="before nbody_octree_compute_tree"):
        t.compute_quadrupoles(dev.stream)
    dev.octree_force(0.5)  # a tree, no quadrupoles
    with pytest.raises(nb.NbodyError, match="before nbody_octree_compute_quadrupoles"):
        t.compute_quadrupole_force(st, 0.5, dev.stream)
    with pytest.raises(nb.NbodyError, match="before nbody_octree_compute_quadrupoles"):
        t.read_root_quadrupole(dev.stream)
    t.compute_quadrupoles(dev.stream)
    t.compute_quadrupole_force(st, 0.5, dev.stream)
    t.read_root_quadrupole(dev.stream)
    t.compute_tree(dev.stream)  # a fresh multipole pass: the quadrupoles are stale
    with pytest.raises(nb.NbodyError, match="before nbody_octree_compute_quadrupoles"):
        t.compute_quadrupole_force(st, 0.5, dev.stream)
    with pytest.raises(nb.NbodyError, match="before nbody_octree_compute_quadrupoles"):
        t.read_root_quadrupole(dev.stream)
    t.compute_quadrupoles(dev.stream)
    t.clear(dev.stream)
    with pytest.raises(nb.NbodyError, match="before nbody_octree_compute_quadrupoles"):
        t.read_root_quadrupole(dev.stream)
    dev.octree_force(0.5, quadrupole=True)
    t.set_walk(2)
    with pytest.raises(nb.NbodyError, match="quadrupole walk"):
        t.compute_quadrupole_force(st, 0.5, dev.stream)
    t.set_walk(0)
    # argument errors that need a tree: a state of another dtype or dim than the tree's, a NULL output
    import ctypes
    L = nb.lib()
    for dtype, dim in ((0, 3), (1, 2)):
        other = nb.DeviceSystem.from_host(nb.build_model(dtype, dim, "galaxy", 3000))
        assert L.nbody_octree_compute_quadrupole_force(t.h, ctypes.byref(other.state()), ctypes.c_double(0.5), ctypes.c_void_p(dev.stream)) == 1
        assert b"octree was created for" in L.nbody_last_error()
        other.close()
    assert L.nbody_octree_read_root_quadrupole(t.h, None, ctypes.c_void_p(dev.stream)) == 1
    assert b"NULL argument" in L.nbody_last_error()
    t.info(dev.stream)
    dev.close()


def cli(dim, args, cwd=None):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", f"nbody_hip_d{dim}")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def read_positions(path):
    raw = open(path, "rb").read()
    n, steps, tsz, dim = struct.unpack("<4I", raw[:16])
    data = np.frombuffer(raw[16:], dtype=np.float32 if tsz == 4 else np.float64)
    return data[: data.size // (n * dim) * n * dim].reshape(-1, n, dim)


def test_cli_quadrupole_positions(nb):
    n = 4096
    base = ["-n", n, "-s", 3, "--algorithm", "octree", "--workload", "galaxy", "--quadrupole", "--save", "pos"]
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
        r1, r2 = cli(3, base, cwd=d1), cli(3, base + ["--csv-detailed"], cwd=d2)
        assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
        plain = read_positions(os.path.join(d1, "positions.bin"))
        detailed = read_positions(os.path.join(d2, "positions.bin"))
    assert len(detailed) == 4, len(detailed)
    dev = nb.DeviceSystem.from_host(nb.build_model(0, 3, "galaxy", n))  # the CLI's default precision: float
    want = [dev.download().x.copy()]
    for _ in range(3):
        dev.octree_force(0.5, quadrupole=True)
        dev.accelerate_step()
        want.append(dev.download().x.copy())
    dev.close()
    assert np.array_equal(detailed, np.stack(want))
    assert len(plain) >= 1 and all(np.array_equal(f, want[k]) for k, f in enumerate(plain))


def state_rows(hs):
    """The CLI's --print-state rows (host/system.hpp: components 0 and 1, % .3e)."""
    f = lambda v: "% .3e" % float(v)
    return [f"{i:02d}: m={f(hs.m[i])}, p=({f(hs.x[i][0])}, {f(hs.x[i][1])}), v=({f(hs.v[i][0])}, {f(hs.v[i][1])}), "
            f"f=({f(hs.a[i][0])}, {f(hs.a[i][1])})" for i in range(hs.n)]


def test_cli_quadrupole_recorded_step(nb):
    """Without --csv-detailed the CLI records one step and replays it (the path users get by default): its final state equals the
    same steps driven through the binding.  theta 1 on a uniform cube, where the quadrupole term shows in the printed digits."""
    n = 2000
    args = ["-n", n, "-s", 3, "--algorithm", "octree", "--workload", "uniform", "--theta", 1.0, "--print-state"]
    quad, mono = cli(3, args + ["--quadrupole"]), cli(3, args)
    assert quad.returncode == 0 and mono.returncode == 0, (quad.stderr, mono.stderr)
    final = lambda out: out.split("Final state:")[1].strip().splitlines()[:n]
    dev = nb.DeviceSystem.from_host(nb.build_model(0, 3, "uniform", n))  # the CLI's default precision: float
    for _ in range(nb.executed_steps(3, False)):
        dev.octree_force(1.0, quadrupole=True)
        dev.accelerate_step()
    want = state_rows(dev.download())
    dev.close()
    assert final(quad.stdout) == want
    assert final(mono.stdout) != want


def test_cli_quadrupole_csv_rows_keep_their_format():
    args = ["-n", 3000, "-s", 3, "--algorithm", "octree", "--workload", "plummer", "--precision", "double"]

    def shape(out):
        lines = [ln for ln in out.splitlines() if ln.startswith("algorithm,") or ln.startswith("octree,")]
        return [re.sub(r"\d+\.\d+", "F", ln) for ln in lines]

    for flag in ("--csv-total", "--csv-detailed"):
        plain, quad = cli(3, args + [flag]), cli(3, args + [flag, "--quadrupole"])
        assert plain.returncode == 0 and quad.returncode == 0, quad.stderr
        assert len(shape(quad.stdout)) == 2 and shape(quad.stdout) == shape(plain.stdout), (quad.stdout, plain.stdout)
    info = cli(3, args + ["--quadrupole", "--print-info", "--csv-detailed"])
    assert info.returncode == 0 and "Tree size:" in info.stdout, info.stderr
