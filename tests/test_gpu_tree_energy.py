"""GPU: octree potentials and energies — per-body phi against a float64 NumPy direct sum written here (theta = 0, where every cell is
opened, and theta 0.5 / 0.7), the energies against nbody_calc_energies, one probe against the monopole and quadrupole expansions,
the walks' invariants (counters, shard windows, build forms, repeated calls, a recorded call), their errors, and the CLI's
--tree-energy."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PROBE_TOL = {1: 1e-12, 0: 1e-5}
# theta = 0: largest per-body relative phi error against the float64 direct sum (also the bound on PE against the float exact path).
# Measured on one MI355X: f64 4.0e-15, f32 1.33e-5 (galaxy 2D; 3D at most 4.4e-6).
THETA0_TOL = {1: 1e-13, 0: 3e-5}
# theta 0.5 / 0.7, N = 4096, the worst workload of each dimension: rms per-body relative phi error and |PE - exact| / |PE| of the
# monopole walk, both dtypes (the quadrupole walk must also halve the rms).  Measured: 3D (plummer) rms 3.25e-4 / 7.1e-4, PE 1.03e-4 /
# 1.6e-4; 2D (uniform) rms 4.9e-3 / 1.03e-2, PE 4.9e-3 / 1.01e-2.  2D is worse by design: the plane's tensor is not traceless, a filled
# square cell has Q ~ q I, so every accepted cell misses the same-signed 1/2 q / r^3 (the quadrupole walk: rms 1.2e-4 at 0.5).
RMS_TOL = {(3, 0.5): 1e-3, (3, 0.7): 2e-3, (2, 0.5): 1.2e-2, (2, 0.7): 2.5e-2}
PE_TOL = {(3, 0.5): 3e-4, (3, 0.7): 4e-4, (2, 0.5): 1.2e-2, (2, 0.7): 2.5e-2}


def np_t(dtype):
    return np.float64 if dtype == 1 else np.float32


def direct_s(m, x, eps_t=0.0, soft=None, targets=None):
    """S_i = sum_{j != i} m_j / (|x_j - x_i| + eps_t), or m_j / sqrt(|x_j - x_i|^2 + soft^2), in float64."""
    m, x = np.asarray(m, np.float64), np.asarray(x, np.float64)
    idx = np.arange(len(m)) if targets is None else np.asarray(targets)
    out = np.zeros(len(idx))
    for s in range(0, len(idx), 512):
        t = idx[s:s + 512]
        d = x[None, :, :] - x[t][:, None, :]
        r2 = (d * d).sum(-1)
        w = 1.0 / (np.sqrt(r2 + soft * soft) if soft else np.sqrt(r2) + eps_t)
        w[np.arange(len(t)), t] = 0.0
        out[s:s + 512] = (w * m[None, :]).sum(1)
    return out


def system(nb, dtype, dim, x, m, c=1.0, dt=0.01):
    hs = nb.HostSystem(dtype, dim, len(m))
    hs.m[:], hs.x[:] = np.asarray(m, np_t(dtype)), np.asarray(x, np_t(dtype))
    hs.c, hs.dt = c, dt
    return hs


def cases():
    return [(dtype, dim, wl) for dtype in (1, 0) for dim, wl in ((3, "galaxy"), (3, "uniform"), (3, "plummer"), (2, "galaxy"),
                                                                  (2, "uniform"))]


def torch_buf(nb, dev):
    """A zeroed device buffer of n values of T, ready before anything is queued on the context's stream."""
    import torch
    buf = torch.zeros(dev.n, dtype=torch.float64 if dev.dtype == 1 else torch.float32, device=f"cuda:{dev.device}")
    torch.cuda.synchronize(dev.device)
    return buf


def tree_built(dev, quadrupole=False):
    return dev._octree_build(quadrupole)


@pytest.mark.parametrize("dtype, dim, workload", cases())
def test_theta0_against_the_direct_sum(nb, dtype, dim, workload):
    """theta = 0 opens every cell: phi is the direct sum of the reference's term m / (r + eps(T)) (and of the softened term), and the
    quadrupole walk, which then accepts no cell, is the monopole walk bit for bit."""
    hs = nb.build_model(dtype, dim, workload, 4096)
    xs, ms = hs.x.astype(np.float64), hs.m.astype(np.float64)
    eps_t = float(np.finfo(np_t(dtype)).eps)
    dev = nb.DeviceSystem.from_host(hs)
    for soft in (None, 0.05):
        phi = dev.octree_potential(0.0, softening=soft or 0.0).astype(np.float64)
        want = -hs.c * direct_s(ms, xs, eps_t, soft)
        err = np.abs(phi - want) / np.abs(want)
        print(f"{workload} {dim}D dtype {dtype} soft {soft}: max rel {err.max():.3g}")
        assert err.max() <= THETA0_TOL[dtype], (soft, float(err.max()))
    mono = dev.octree_potential(0.0)
    quad = dev.octree_potential(0.0, quadrupole=True)
    assert np.array_equal(mono, quad)
    dev.close()


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_energies_against_the_exact_path(nb, dtype, dim):
    hs = nb.build_model(dtype, dim, "plummer" if dim == 3 else "galaxy", 4096)
    dev = nb.DeviceSystem.from_host(hs)
    for soft in (0.0, 0.05):
        ke, pe = dev.calc_energies(soft)
        for theta, quad in ((0.0, False), (0.5, False), (0.0, soft == 0.0), (0.5, soft == 0.0)):
            tk, tp = dev.octree_energies(theta, softening=soft, quadrupole=quad)
            assert tk.tobytes() == ke.tobytes(), (soft, theta, quad)
            rel = abs(float(tp) - float(pe)) / abs(float(pe))
            print(f"{dim}D dtype {dtype} soft {soft} theta {theta} quad {quad}: PE rel {rel:.3g}")
            assert rel <= (THETA0_TOL[dtype] if theta == 0.0 else PE_TOL[dim, 0.5]), (soft, theta, quad, rel)
    dev.octree.info(dev.stream)
    dev.close()


def expansion_s(m, x, probe, eps=0.0):
    """S at `probe` from the bodies (m, x) expanded about their centre of mass: M / (|d| + eps) and M / |d| + 1/2 d^T Q d / |d|^5."""
    dt = np.longdouble
    m, x = np.asarray(m, dt), np.asarray(x, dt)
    p = (m[:, None] * x).sum(0) / m.sum()
    s = x - p
    r2 = (s * s).sum(1)
    dim = x.shape[1]
    Q = np.zeros((dim, dim), dt)
    for u in range(dim):
        for v in range(dim):
            Q[u, v] = (m * (3 * s[:, u] * s[:, v] - (r2 if u == v else 0))).sum()
    d = p - np.asarray(probe, dt)
    r = np.sqrt((d * d).sum())
    return m.sum() / (r + dt(eps)), m.sum() / (r + dt(eps)) + dt(0.5) * (d @ Q @ d) / r ** 5


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_one_cluster_one_probe(nb, dtype, dim):
    """test_gpu_quadrupole.py's geometry: the probe's walk opens the root and accepts the ball's cell as one node, so its phi is the
    expansion of the ball about its centre of mass — at unit scale, times 1e6 and at 2^-22 (where float's y^5 alone would overflow)."""
    eps = float(np.finfo(np_t(dtype)).eps)
    for scale, seed in ((1.0, 5), (1e6, 15), (2.0 ** -22, 15)):
        rng = np.random.default_rng(seed + dim)
        k = 40
        theta = 0.5 if scale > 1 else 0.7
        if scale >= 1:
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
        pm = dev.octree_potential(theta)
        pq = dev.octree_potential(theta, quadrupole=True)
        dev.octree.info(dev.stream)
        dev.close()
        assert np.isfinite(pm).all() and np.isfinite(pq).all(), scale
        mono, quad = expansion_s(ms[:k], xs[:k], xs[k], eps)
        assert abs(pm[k] + hs.c * mono) <= PROBE_TOL[dtype] * abs(mono), (scale, pm[k], mono)
        assert abs(pq[k] + hs.c * quad) <= PROBE_TOL[dtype] * abs(quad), (scale, pq[k], quad)
        if scale == 1.0:  # (the 1e6 ball's draw is nearly isotropic: there the octupole is not much below the quadrupole)
            exact = direct_s(ms, xs, eps, targets=[k])[0]
            assert abs(quad - exact) < 0.2 * abs(mono - exact), (abs(quad - exact), abs(mono - exact))


@pytest.mark.parametrize("dtype, dim, workload", cases())
def test_accuracy_against_the_direct_sum(nb, dtype, dim, workload):
    hs = nb.build_model(dtype, dim, workload, 4096)
    xs, ms = hs.x.astype(np.float64), hs.m.astype(np.float64)
    s = direct_s(ms, xs, float(np.finfo(np_t(dtype)).eps))
    want_phi, want_pe = -hs.c * s, -0.5 * hs.c * (ms * s).sum()
    dev = nb.DeviceSystem.from_host(hs)
    for theta in (0.5, 0.7):
        rms = {}
        for quad in (False, True):
            err = (dev.octree_potential(theta, quadrupole=quad).astype(np.float64) - want_phi) / np.abs(want_phi)
            rms[quad] = np.sqrt((err ** 2).mean())
            pe = float(dev.octree_energies(theta, quadrupole=quad)[1])
            pe_err = abs(pe - want_pe) / abs(want_pe)
            print(f"{workload} {dim}D dtype {dtype} theta {theta} quad {quad}: rms {rms[quad]:.3g} "
                  f"p99 {np.percentile(np.abs(err), 99):.3g} PE {pe_err:.3g}")
            assert pe_err <= PE_TOL[dim, theta], (theta, quad, pe_err)
        assert rms[False] <= RMS_TOL[dim, theta], (theta, rms)
        assert rms[True] <= 0.5 * rms[False], (theta, rms)
    dev.close()


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_counters_equal_the_force_walks(nb, dtype, dim):
    hs = nb.build_model(dtype, dim, "galaxy", 4096)
    dev = nb.DeviceSystem.from_host(hs)
    t = dev.octree
    t.enable_counters(True)
    dev.octree_force(0.5)
    want = t.read_counters(dev.stream).copy()
    for soft, quad in ((0.0, False), (0.05, False), (0.0, True)):
        dev.octree_potential(0.5, softening=soft, quadrupole=quad)
        assert np.array_equal(t.read_counters(dev.stream), want), (soft, quad)
    dev.close()


@pytest.mark.parametrize("dtype", [1, 0])
def test_bitwise_invariances(nb, dtype):
    """Shard windows, build forms 1 and 3 and repeated calls give the same phi bit for bit."""
    tsz = 8 if dtype == 1 else 4
    for dim in (3, 2):
        hs = nb.build_model(dtype, dim, "plummer" if dim == 3 else "uniform", 9000)
        dev = nb.DeviceSystem.from_host(hs)
        t = dev.octree
        for soft, quad in ((0.0, False), (0.05, False), (0.0, True)):
            whole = dev.octree_potential(0.5, softening=soft, quadrupole=quad)
            assert np.array_equal(dev.octree_potential(0.5, softening=soft, quadrupole=quad), whole)
            for parts in (2, 7):
                buf = torch_buf(nb, dev)
                for p in range(parts):
                    f, e = nb.shard_range(hs.n, p, parts)
                    st, ptr = dev.state(f, e - f), buf.data_ptr() + f * tsz
                    if quad:
                        t.compute_quadrupole_potential(st, 0.5, ptr, dev.stream)
                    elif soft:
                        t.compute_softened_potential(st, 0.5, soft, ptr, dev.stream)
                    else:
                        t.compute_potential(st, 0.5, ptr, dev.stream)
                dev.sync()
                assert np.array_equal(buf.cpu().numpy(), whole), (soft, quad, parts)
            t.set_build(1)
            assert np.array_equal(dev.octree_potential(0.5, softening=soft, quadrupole=quad), whole), (soft, quad)
            t.info(dev.stream)
            t.set_build(0)
        dev.close()


def test_recorded_potential_replays_the_eager_result(nb):
    hs = nb.build_model(1, 3, "galaxy", 9000)
    dev = nb.DeviceSystem.from_host(hs)
    eager = dev.octree_potential(0.5)
    buf = torch_buf(nb, dev)
    t = dev.octree

    def record():
        st, _ = tree_built(dev)
        t.compute_potential(st, 0.5, buf.data_ptr(), dev.stream)

    g = nb.StepGraph(dev, record)
    g.launch()
    g.launch()
    dev.sync()
    assert np.array_equal(buf.cpu().numpy(), eager)
    g.close()
    dev.close()


def test_walk_form_and_phase_errors(nb):
    dev = nb.DeviceSystem.from_host(nb.build_model(1, 3, "galaxy", 3000))
    t = dev.octree
    L = nb.lib()
    buf = torch_buf(nb, dev)
    ke, pe = ctypes.c_double(), ctypes.c_double()
    st = dev.state()
    assert L.nbody_octree_compute_potential(t.h, ctypes.byref(st), 0.5, buf.data_ptr(), dev.stream) == 3
    assert b"before nbody_octree_compute_tree" in L.nbody_last_error()
    dev.octree_force(0.5)  # a tree, no quadrupoles
    assert L.nbody_octree_compute_quadrupole_potential(t.h, ctypes.byref(st), 0.5, buf.data_ptr(), dev.stream) == 3
    assert b"before nbody_octree_compute_quadrupoles" in L.nbody_last_error()
    assert L.nbody_octree_calc_energies(t.h, ctypes.byref(st), 0.5, 0.0, 1, ctypes.byref(ke), ctypes.byref(pe), dev.stream) == 3
    assert b"before nbody_octree_compute_quadrupoles" in L.nbody_last_error()
    t.set_walk(2)
    for call in (lambda: t.compute_potential(st, 0.5, buf.data_ptr(), dev.stream),
                 lambda: t.compute_softened_potential(st, 0.5, 0.05, buf.data_ptr(), dev.stream),
                 lambda: t.calc_energies(st, 0.5, stream=dev.stream)):
        with pytest.raises(nb.NbodyError, match="potential walk"):
            call()
    assert L.nbody_octree_compute_potential(t.h, ctypes.byref(st), 0.5, buf.data_ptr(), dev.stream) == 1
    t.set_walk(0)
    t.compute_potential(st, 0.5, buf.data_ptr(), dev.stream)
    # blocking: refused under capture
    with pytest.raises(nb.NbodyError, match="cannot be recorded"):
        nb.StepGraph(dev, lambda: t.calc_energies(st, 0.5, stream=dev.stream))
    t.info(dev.stream)
    dev.close()


def cli(args, cwd):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")
    return subprocess.run([exe] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def cli_pair(args):
    """(positions.bin bytes, energy.bin records) of the run without and with --tree-energy."""
    out = []
    for extra in ([], ["--tree-energy"]):
        with tempfile.TemporaryDirectory() as d:
            r = cli(args + extra, d)
            assert r.returncode == 0, (args + extra, r.stderr)
            import oracle as O
            energy, _ = O.read_energy_bin(os.path.join(d, "energy.bin"))
            out.append((open(os.path.join(d, "positions.bin"), "rb").read(), energy.copy()))
    return out


def test_cli_tree_energy():
    base = ["-n", 4096, "-s", 5, "--algorithm", "octree", "--workload", "plummer", "--save", "all"]
    # the detailed path at the default theta, in the default precision: the dynamics are untouched
    (pos0, e0), (pos1, e1) = cli_pair(base + ["--csv-detailed"])
    assert pos0 == pos1
    assert len(e0) == len(e1) == 6
    assert e0[:, 0].tobytes() == e1[:, 0].tobytes()
    assert not np.array_equal(e0[:, 1], e1[:, 1])  # the tree's potential
    # theta 0, double: the tree's potential is the exact one to rounding level, for the three walks
    for extra in ([], ["--softening", 0.05], ["--quadrupole"]):
        (pos0, e0), (pos1, e1) = cli_pair(base + ["--csv-detailed", "--precision", "double", "--theta", 0] + extra)
        assert pos0 == pos1, extra
        assert e0[:, 0].tobytes() == e1[:, 0].tobytes(), extra
        rel = np.abs(e1[:, 1] - e0[:, 1]) / np.abs(e0[:, 1])
        assert rel.max() <= 1e-12, (extra, rel.max())
    # the recorded path: one record, the initial state
    (pos0, e0), (pos1, e1) = cli_pair(base + ["--precision", "double"])
    assert pos0 == pos1
    assert len(e0) == len(e1) == 1
    assert e0[:, 0].tobytes() == e1[:, 0].tobytes()
    assert abs(e1[0, 1] - e0[0, 1]) <= PE_TOL[3, 0.5] * abs(e0[0, 1])
