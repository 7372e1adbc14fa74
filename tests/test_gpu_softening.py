"""GPU: Plummer softening (ABI 2.4) — the softened K1 (both source paths), the softened potential and the softened octree walk
against a NumPy direct sum written here (the reference has no softening, so there are no fixtures), their bitwise invariances
(shard windows, source paths, recorded steps, opening decisions) and the CLI's --softening."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TOL = {1: 1e-12, 0: 2e-5}


def maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def e2_of(dtype, eps):
    t = np.float32 if dtype == 0 else np.float64
    return t(t(eps) * t(eps))


def ref_force(m, x, c, e2, targets=None, dt=np.longdouble):
    """c * sum_{j != i} m_j (x_j - x_i) / (|x_j - x_i|^2 + e2)^(3/2) in `dt` (the self term is 0: its difference is 0)."""
    m, x = np.asarray(m, dt), np.asarray(x, dt)
    idx = np.arange(len(m)) if targets is None else np.asarray(targets)
    out = np.zeros((len(idx), x.shape[1]), dt)
    for s in range(0, len(idx), 256):
        t = idx[s:s + 256]
        d = x[None, :, :] - x[t][:, None, :]
        q = (d * d).sum(-1) + dt(e2)
        w = m[None, :] / (q * np.sqrt(q))
        out[s:s + 256] = (w[:, :, None] * d).sum(1)
    return dt(c) * out


def ref_potential(m, x, c, e2, dt=np.longdouble):
    m, x = np.asarray(m, dt), np.asarray(x, dt)
    tot = dt(0)
    for s in range(0, len(m), 256):
        d = x[None, :, :] - x[s:s + 256][:, None, :]
        q = (d * d).sum(-1) + dt(e2)
        inv = 1 / np.sqrt(q)
        inv[np.arange(inv.shape[0]), np.arange(s, s + inv.shape[0])] = 0  # self term, by index
        tot += (m[s:s + 256] * (inv * m[None, :]).sum(1)).sum()
    return -dt(0.5) * dt(c) * tot


def device(nb, hs):
    return nb.DeviceSystem.from_host(hs)


SIZES = [1, 2, 3, 65, 2047, 2048, 4099, 8192, 8193, 70001]
EPS = [0.01, 0.1, 1.0]


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_softened_k1_against_numpy(nb, dtype, dim):
    """Sizes across the tile form, the collect path, the turn hand-off and the scalar-stream form; every eps on galaxy and uniform."""
    rng = np.random.default_rng(7)
    worst = {}
    for k, n in enumerate(SIZES):
        for wl in ("galaxy", "uniform") if n > 1 else ("uniform",):  # (the galaxy needs two bodies)
            eps = EPS[(k + (wl == "uniform")) % 3]
            hs = nb.build_model(dtype, dim, wl, n)
            dev = device(nb, hs)
            dev.all_pairs_softened_force(eps)
            a = dev.download().a
            dev.close()
            assert np.isfinite(a).all()
            e2 = e2_of(dtype, eps)
            if hs.n <= 4099:
                ref, got = ref_force(hs.m, hs.x, hs.c, e2), a
            elif hs.n <= 8193:
                t = rng.choice(hs.n, 1024, replace=False)
                ref, got = ref_force(hs.m, hs.x, hs.c, e2, t), a[t]
            else:
                t = rng.choice(hs.n, 512, replace=False)
                ref, got = ref_force(hs.m, hs.x, hs.c, e2, t, np.float64), a[t]
            if hs.n == 1:
                assert np.array_equal(a, np.zeros_like(a))
                continue
            worst[(hs.n, wl, eps)] = r = maxrel(got, ref)
            assert r <= TOL[dtype], (hs.n, wl, eps, r)
    print(f"dtype={dtype} dim={dim} max maxrel {max(worst.values()):.3g}")


@pytest.mark.parametrize("dtype", [1, 0])
def test_softened_k1_adversarial_inputs(nb, dtype):
    """Coincident bodies, a body at 1e-3 eps from another, all bodies at one point: finite, as NumPy says; a coincident pair adds 0."""
    t = np.float32 if dtype == 0 else np.float64
    eps = 0.1
    for n in (3, 4099):
        hs = nb.build_model(dtype, 3, "uniform", n)
        hs.x[1] = hs.x[0]                                     # coincident
        hs.x[2] = hs.x[0] + t(1e-3 * eps) * np.array([1, 0, 0], t)  # at 1e-3 eps
        dev = device(nb, hs)
        dev.all_pairs_softened_force(eps)
        a = dev.download().a
        dev.close()
        assert np.isfinite(a).all()
        assert maxrel(a, ref_force(hs.m, hs.x, hs.c, e2_of(dtype, eps))) <= TOL[dtype]
    for n in (2, 3, 2048):   # a coincident pair alone, and everything at one point: exactly 0
        hs = nb.HostSystem(dtype, 3, n)
        hs.m[:] = 1.0
        hs.x[:] = t(0.25)
        hs.dt, hs.c = 0.1, 1.0
        dev = device(nb, hs)
        dev.all_pairs_softened_force(eps)
        a = dev.download().a
        dev.close()
        assert np.array_equal(a, np.zeros_like(a)), n


def test_softened_k1_tends_to_the_unsoftened_one(nb):
    """eps = 1e-30 on a jittered lattice agrees with nbody_all_pairs_force.  (Spacing 1: the unsoftened term carries the reference's
    + eps(T) in r^3 + eps, a relative change of eps(T) / r^3 — 1.8e-12 at r = 0.05, 2.2e-16 at r = 1.)"""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(*[np.arange(10.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    hs = nb.HostSystem(1, 3, len(g))
    hs.x[:] = g + rng.uniform(-0.2, 0.2, g.shape)
    hs.m[:] = rng.uniform(0.5, 1.5, len(g))
    hs.dt, hs.c = 0.1, 1.0
    dev = device(nb, hs)
    dev.all_pairs_softened_force(1e-30)
    soft = dev.download().a.copy()
    dev.all_pairs_force()
    plain = dev.download().a
    dev.close()
    assert maxrel(soft, plain) <= 1e-14


@pytest.mark.parametrize("dtype", [1, 0])
def test_softened_k1_bitwise_invariances(nb, dtype):
    """Shard windows (2, 7, 8, 70 parts) equal the whole launch; LDS tiles equal the scalar stream; a recorded step equals direct calls."""
    eps = 0.1
    for n in (4099, 70001):
        hs = nb.build_model(dtype, 3, "galaxy", n)
        dev = device(nb, hs)
        dev.all_pairs_softened_force(eps)
        whole = dev.download().a.copy()
        for parts in (2, 7, 8, 70):
            dev.upload(hs)
            for p in range(parts):
                f, e = nb.shard_range(hs.n, p, parts)
                dev.all_pairs_softened_force(eps, f, e - f)
            assert np.array_equal(dev.download().a, whole), (n, parts)
        got = {}
        for path in (1, 2):
            dev.configure_all_pairs(4, 0, path)
            dev.all_pairs_softened_force(eps)
            got[path] = dev.download().a.copy()
        assert np.array_equal(got[1], got[2]), n
        dev.close()
    hs = nb.build_model(dtype, 3, "galaxy", 4099)
    d1, d2 = device(nb, hs), device(nb, hs)
    for _ in range(3):
        d1.all_pairs_softened_force(eps)
        d1.accelerate_step()
    g = nb.StepGraph(d2, lambda: (d2.all_pairs_softened_force(eps), d2.accelerate_step()))
    for _ in range(3):
        g.launch()
    a, b = d1.download(), d2.download()
    g.close()
    d1.close()
    d2.close()
    assert np.array_equal(a.x, b.x) and np.array_equal(a.v, b.v) and np.array_equal(a.a, b.a)


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_softened_energies(nb, dtype, dim):
    eps = 0.1
    for n in (100, 3000):
        hs = nb.build_model(dtype, dim, "galaxy", n)
        dev = device(nb, hs)
        ke0, pe0 = dev.calc_energies()
        ke, pe = dev.calc_energies(softening=eps)
        dev.close()
        assert ke == ke0  # the kinetic part is the unsoftened call's
        ref = ref_potential(hs.m, hs.x, hs.c, e2_of(dtype, eps))
        assert abs(float(pe) - float(ref)) <= (1e-13 if dtype == 1 else 1e-5) * abs(float(ref)), (n, pe, ref)
    # the self term is excluded: one body has no potential; two coincident ones have -c m0 m1 / eps
    t = np.float32 if dtype == 0 else np.float64
    for n, want in ((1, 0.0), (2, None)):
        hs = nb.HostSystem(dtype, dim, n)
        hs.m[:] = [0.75, 1.25][:n]
        hs.x[:] = t(0.5)
        hs.dt, hs.c = 0.1, 2.0
        dev = device(nb, hs)
        ke, pe = dev.calc_energies(softening=eps)
        dev.close()
        if want is not None:
            assert pe == 0.0
        else:
            exact = -2.0 * 0.75 * 1.25 / float(np.sqrt(e2_of(dtype, eps)))
            assert abs(float(pe) - exact) <= (1e-15 if dtype == 1 else 1e-6) * abs(exact), (pe, exact)


# measured on MI355X: max |x_gpu - x_numpy| / max |x| after 100 steps = 9.52e-15; the bound is >= 10x that
MEASURED_TRAJ = 9.52e-15
TRAJ_BOUND = 1e-13


def test_softened_trajectory_against_numpy_leapfrog(nb):
    """N = 512 galaxy, double, eps = 0.1: 100 steps of softened K1 + K3 against a NumPy leapfrog with the same softened forces
    (K3 as nbody_hip.h states it: x += dt v + ((dt/2) dt) ao; v += (dt/2)(a + ao); ao = a)."""
    eps = 0.1
    hs = nb.build_model(1, 3, "galaxy", 512)
    dev = device(nb, hs)
    x, v, ao = hs.x.astype(np.float64).copy(), hs.v.astype(np.float64).copy(), hs.ao.astype(np.float64).copy()
    dt, e2 = np.float64(hs.dt), e2_of(1, eps)
    for _ in range(100):
        dev.all_pairs_softened_force(eps)
        dev.accelerate_step()
        a = ref_force(hs.m, x, hs.c, e2, dt=np.float64)
        x = x + dt * v + ((0.5 * dt) * dt) * ao
        v = v + (0.5 * dt) * (a + ao)
        ao = a
    got = dev.download().x
    dev.close()
    err = np.abs(got - x).max() / np.abs(x).max()
    print(f"trajectory: max |dx| / max |x| = {err:.3g}")
    assert err <= TRAJ_BOUND, err


@pytest.mark.parametrize("dtype", [1, 0])
def test_softened_octree(nb, oracle, dtype):
    eps = 0.1
    for dim in (3, 2):
        hs = nb.build_model(dtype, dim, "galaxy", 3000)
        dev = device(nb, hs)
        # theta so small that every cell opens: the walk is the direct sum
        dev.octree_force(1e-9, softening=eps)
        a = dev.download().a.copy()
        assert maxrel(a, ref_force(hs.m, hs.x, hs.c, e2_of(dtype, eps))) <= TOL[dtype], dim
        # theta 0.5: the softened walk makes the unsoftened walk's decisions, body by body
        t = dev.octree
        t.enable_counters(True)
        dev.octree_force(0.5)
        plain = t.read_counters(dev.stream).copy()
        dev.octree_force(0.5, softening=eps)
        soft = t.read_counters(dev.stream)
        assert np.array_equal(plain, soft)
        whole = dev.download().a.copy()
        # its value: per body against the oracle's wide walk (the same decisions: the counters are the oracle's, test_gpu_octree.py)
        ref = oracle.State(dtype, dim, hs.n)
        ref.m[:], ref.x[:], ref.c, ref.dt = hs.m, hs.x, hs.c, hs.dt
        w = oracle.octree_walk_wide(ref, 0.5, eps)
        assert np.array_equal(soft, w.counts), dim
        err = (np.abs(whole.astype(np.float64) - w.a_soft).max(axis=1) / w.scale_a_soft).max()
        print(f"softened octree {dim}D dtype {dtype}: max err_i {err:.3g}")
        assert err <= TOL[dtype], (dim, err)
        for parts in (2, 7):
            for p in range(parts):
                f, e = nb.shard_range(hs.n, p, parts)
                t.compute_softened_force(dev.state(f, e - f), 0.5, eps, dev.stream)
            assert np.array_equal(dev.download().a, whole), parts
        t.set_walk(2)
        with pytest.raises(nb.NbodyError, match="softened walk"):
            t.compute_softened_force(dev.state(), 0.5, eps, dev.stream)
        t.set_walk(0)
        t.info(dev.stream)
        dev.close()


def cli(dim, args, cwd=None):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", f"nbody_hip_d{dim}")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def test_cli_softening(nb, oracle):
    strip = lambda out: re.sub(r"Total time: .*", "", out)
    base = ["-n", 300, "-s", 12, "--precision", "double", "--algorithm", "all-pairs", "--workload", "galaxy", "--print-state"]
    plain, zero = cli(3, base), cli(3, base + ["--softening", 0])
    assert plain.returncode == 0 and zero.returncode == 0, zero.stderr
    assert strip(plain.stdout) == strip(zero.stdout)
    # the softened run against the same run driven from Python (12 steps: -s 12 is past the 10 warm-up steps)
    soft = cli(3, base + ["--softening", 0.1])
    assert soft.returncode == 0, soft.stderr
    assert strip(soft.stdout) != strip(plain.stdout)
    hs = nb.build_model(1, 3, "galaxy", 300)
    dev = device(nb, hs)
    for _ in range(12):
        dev.all_pairs_softened_force(0.1)
        dev.accelerate_step()
    out = dev.download()
    dev.close()
    assert oracle.parse_print_state(soft.stdout)[1] == oracle.format_state_rows(out)
    forced = cli(3, base + ["--softening", 0.1, "--gpus", 1])
    assert forced.returncode == 0, forced.stderr
    assert strip(forced.stdout) == strip(soft.stdout)
    # positions.bin (bitwise against Python, and with --gpus 1) and energy.bin (calc_energies(softening=...))
    args = ["-n", 500, "-s", 4, "--precision", "double", "--algorithm", "all-pairs", "--workload", "galaxy", "--csv-detailed",
            "--softening", 0.1]
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2, tempfile.TemporaryDirectory() as d3:
        r1, r2 = cli(3, args + ["--save", "pos"], cwd=d1), cli(3, args + ["--save", "pos", "--gpus", 1], cwd=d2)
        r3 = cli(3, args + ["--save", "energy"], cwd=d3)
        assert r1.returncode == 0 and r2.returncode == 0 and r3.returncode == 0, (r1.stderr, r2.stderr, r3.stderr)
        p1 = open(os.path.join(d1, "positions.bin"), "rb").read()
        assert p1 == open(os.path.join(d2, "positions.bin"), "rb").read()
        frames, _ = oracle.read_positions_bin(os.path.join(d1, "positions.bin"))
        en, _ = oracle.read_energy_bin(os.path.join(d3, "energy.bin"))
    hs = nb.build_model(1, 3, "galaxy", 500)
    dev = device(nb, hs)
    want_x, want_e = [dev.download().x.copy()], [dev.calc_energies(softening=0.1)]
    for _ in range(4):
        dev.all_pairs_softened_force(0.1)
        dev.accelerate_step()
        want_x.append(dev.download().x.copy())
        want_e.append(dev.calc_energies(softening=0.1))
    dev.close()
    assert np.array_equal(frames, np.stack(want_x))
    assert np.array_equal(np.asarray(en).reshape(-1, 2), np.array(want_e))
    # the default algorithm (octree, float) takes the softened walk
    r = cli(3, ["-n", 2000, "-s", 3, "--workload", "galaxy", "--softening", 0.05, "--print-state"])
    assert r.returncode == 0, r.stderr
    final = oracle.parse_print_state(r.stdout)[1]
    assert len(final) == 2000 and not any("nan" in row or "inf" in row for row in final)
