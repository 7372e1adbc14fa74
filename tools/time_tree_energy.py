"""Octree potentials and energies against the force walk and the exact energy path, A/B in ONE process (boxes of the pool differ by
several percent: only an interleaved comparison in one session says anything).  Times are HIP events recorded on the context's own
stream, the two calls alternated, median of the rounds.
    python tools/time_tree_energy.py [--quick]
1. N = 10^6 galaxy, 3D, double and float, one tree: the potential walk (nbody_octree_compute_potential) next to the monopole force
   walk at theta 0.5 and 0.7, the force walk in form 1 (the same compiler-scheduled walk) and in the shipped auto form.
2. One DeviceSystem.octree_energies (tree build + potential walk + reduction, blocking) next to one nbody_calc_energies.
3. Error: PE against nbody_calc_energies on a double copy of the positions and masses; per-body phi on a fixed sample of 4096 bodies
   against a float64 direct sum over all N (torch on the device), rms and 99th percentile; monopole and quadrupole walks,
   theta 0.3, 0.5, 0.7, 0.9.
4. The CLI, `-n 1000000 -s 10 --algorithm octree --workload galaxy --precision double --csv-detailed --save energy`, with and
   without --tree-energy: the `total [s]` column."""
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402


def timed(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(stream, fa, fb, reps=5, rounds=5):
    fa(), fb()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(stream, fa, reps))
        b.append(timed(stream, fb, reps))
    return statistics.median(a), statistics.median(b)


def sample_s(m, x, idx, eps_t):
    """S_i = sum_{j != i} m_j / (|x_j - x_i| + eps_t) for the bodies idx, float64 on the device."""
    mt = torch.as_tensor(np.asarray(m, np.float64), device="cuda")
    xt = torch.as_tensor(np.asarray(x, np.float64), device="cuda")
    out = np.zeros(len(idx))
    for s in range(0, len(idx), 16):
        t = torch.as_tensor(idx[s:s + 16], device="cuda")
        r = torch.sqrt(((xt[None, :, :] - xt[t][:, None, :]) ** 2).sum(-1)) + eps_t
        w = mt[None, :] / r
        w[torch.arange(len(t), device="cuda"), t] = 0.0
        out[s:s + 16] = w.sum(1).cpu().numpy()
    return out


def cli_total(n, tree_energy):
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")
    args = [exe, "-n", str(n), "-s", "10", "--algorithm", "octree", "--workload", "galaxy", "--precision", "double", "--csv-detailed",
            "--save", "energy"] + (["--tree-energy"] if tree_energy else [])
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(args, cwd=d, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    row = [ln for ln in r.stdout.splitlines() if ln.startswith("octree,")][0].split(",")
    return float(row[5]), float(row[6])


def main():
    quick = "--quick" in sys.argv
    nb = load_package()
    n = 62500 if quick else 1000000
    for tname, dtype in (("f64", nb.F64), ("f32", nb.F32)):
        hs = nb.build_model(dtype, 3, "galaxy", n)
        dev = nb.DeviceSystem.from_host(hs)
        t, st = dev.octree, dev.state()
        dev.octree_force(0.5, quadrupole=True)  # one tree, its monopoles and quadrupoles; the walks below reuse it
        dev.sync()
        phi = torch.empty(n, dtype=torch.float64 if dtype == nb.F64 else torch.float32, device="cuda")
        torch.cuda.synchronize()
        # 1. the potential walk against the force walk on the same tree
        for theta in (0.5, 0.7):
            pot = lambda: t.compute_potential(st, theta, phi.data_ptr(), dev.stream)
            force = lambda: t.compute_force(st, theta, dev.stream)
            t.set_walk(1)
            f1, p1 = ab(dev.stream, force, pot)
            t.set_walk(0)
            fa, pa = ab(dev.stream, force, pot)
            print(f"{tname} 3D galaxy N={n}: walk theta={theta} force (form 1) {f1:8.3f} ms   potential {p1:8.3f} ms   ratio {p1 / f1:.3f}"
                  f"   | force (auto) {fa:8.3f} ms   potential {pa:8.3f} ms   ratio {pa / fa:.3f}", flush=True)
        # 2. one tree-energy evaluation against one exact one
        ex, tr = ab(dev.stream, lambda: dev.calc_energies(), lambda: dev.octree_energies(0.5), reps=1, rounds=5)
        print(f"{tname} 3D galaxy N={n}: energies  nbody_calc_energies {ex:9.3f} ms   octree_energies(theta 0.5, with its tree build) "
              f"{tr:8.3f} ms   speed-up {ex / tr:.1f}x", flush=True)
        # 3. accuracy against the exact double sums
        ref_hs = nb.HostSystem(nb.F64, 3, n)
        ref_hs.m[:], ref_hs.x[:], ref_hs.v[:], ref_hs.c, ref_hs.dt = hs.m, hs.x, hs.v, hs.c, hs.dt
        ref = nb.DeviceSystem.from_host(ref_hs)
        exact_pe = float(ref.calc_energies()[1])
        ref.close()
        idx = np.random.default_rng(7).choice(n, 4096, replace=False)
        eps_t = float(np.finfo(np.float64 if dtype == nb.F64 else np.float32).eps)
        want_phi = -hs.c * sample_s(hs.m, hs.x, idx, eps_t)
        print(f"{tname} 3D galaxy N={n}: error against the double direct sum (PE over all bodies; phi on 4096 sampled bodies)")
        print(f"    {'theta':>5s} {'walk':>11s} {'PE rel err':>11s} {'phi rms':>10s} {'phi p99':>10s}")
        for theta in (0.3, 0.5, 0.7, 0.9):
            for quad in (False, True):
                pe = float(dev.octree_energies(theta, quadrupole=quad)[1])
                e = np.abs(dev.octree_potential(theta, quadrupole=quad)[idx].astype(np.float64) - want_phi) / np.abs(want_phi)
                print(f"    {theta:5.1f} {'quadrupole' if quad else 'monopole':>11s} {abs(pe - exact_pe) / abs(exact_pe):11.3e} "
                      f"{np.sqrt((e * e).mean()):10.3e} {np.percentile(e, 99):10.3e}", flush=True)
        t.info(dev.stream)
        dev.close()
    # 4. the CLI
    for te in (False, True):
        total, force = cli_total(n, te)
        print(f"CLI d3 -n {n} -s 10 octree galaxy double --csv-detailed --save energy{' --tree-energy' if te else ''}: "
              f"total [s] {total:.2f}   force [s] {force:.2f}", flush=True)


if __name__ == "__main__":
    main()
