"""Quadrupole pass and walk against the monopole ones, A/B in ONE process (boxes of the pool differ by several percent: only an
interleaved comparison in one session says anything).  Times are HIP events recorded on the context's own stream around `reps`
back-to-back calls, the two forms alternated, median of the rounds.
    python tools/time_quadrupole.py [--quick]
1. N = 10^6 galaxy, 3D, double and float, one tree: the quadrupole pass (nbody_octree_compute_quadrupoles) next to the monopole pass
   (nbody_octree_compute_tree), and the quadrupole walk next to the monopole walk in the same form (walk form 1) at theta 0.5.
2. Error against time: theta 0.5, 0.7, 0.9; the monopole walk (form 1 and the shipped auto form) and the quadrupole walk (+ its
   pass); per-body relative force error |a - a_K1| / |a_K1| against K1's direct sum on the same state, in double also for the float
   system (K1 on a double copy of its positions and masses: a float K1 would measure its own rounding), RMS and 99th percentile."""
import os
import statistics
import sys

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


def errors(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    e = np.linalg.norm(a - ref, axis=1) / np.linalg.norm(ref, axis=1)
    return np.sqrt((e * e).mean()), np.percentile(e, 99)


def main():
    quick = "--quick" in sys.argv
    nb = load_package()
    n = 62500 if quick else 1000000
    for tname, dtype in (("f64", nb.F64), ("f32", nb.F32)):
        hs = nb.build_model(dtype, 3, "galaxy", n)
        dev = nb.DeviceSystem.from_host(hs)
        t, st = dev.octree, dev.state()
        dev.octree_force(0.5, quadrupole=True)  # one tree, its monopoles and quadrupoles; everything below reuses it
        dev.sync()
        mp, qp = ab(dev.stream, lambda: t.compute_tree(dev.stream), lambda: t.compute_quadrupoles(dev.stream))
        print(f"{tname} 3D galaxy N={n}: pass   monopole (compute_tree) {mp:8.3f} ms   quadrupole {qp:8.3f} ms   ratio {qp / mp:.3f}",
              flush=True)
        t.set_walk(1)
        mw, qw = ab(dev.stream, lambda: t.compute_force(st, 0.5, dev.stream), lambda: t.compute_quadrupole_force(st, 0.5, dev.stream))
        print(f"{tname} 3D galaxy N={n}: walk theta=0.5 monopole (form 1) {mw:8.3f} ms   quadrupole {qw:8.3f} ms   ratio {qw / mw:.3f}",
              flush=True)
        t.set_walk(0)
        # error against time: K1's direct sum on the same state, in double
        ref_hs = nb.HostSystem(nb.F64, 3, n)
        ref_hs.m[:], ref_hs.x[:], ref_hs.c, ref_hs.dt = hs.m, hs.x, hs.c, hs.dt
        ref = nb.DeviceSystem.from_host(ref_hs)
        ref.all_pairs_force()
        exact = ref.download().a.copy()
        ref.close()
        print(f"{tname} 3D galaxy N={n}: error against K1, times per call (walks on the same tree; the quadrupole pass {qp:.3f} ms "
              f"comes on top of the quadrupole walk)")
        print(f"    {'theta':>5s} {'walk':>14s} {'ms':>8s} {'rms err':>10s} {'p99 err':>10s}")
        for theta in (0.5, 0.7, 0.9):
            rows = []
            for name, walk, call in (("monopole f1", 1, lambda: t.compute_force(st, theta, dev.stream)),
                                     ("monopole auto", 0, lambda: t.compute_force(st, theta, dev.stream)),
                                     ("quadrupole", 0, lambda: t.compute_quadrupole_force(st, theta, dev.stream))):
                t.set_walk(walk)
                ms, _ = ab(dev.stream, call, call, reps=3, rounds=3)
                call()
                rms, p99 = errors(dev.download().a, exact)
                rows.append((name, ms, rms, p99))
            t.set_walk(0)
            for name, ms, rms, p99 in rows:
                print(f"    {theta:5.1f} {name:>14s} {ms:8.3f} {rms:10.3e} {p99:10.3e}", flush=True)
        t.info(dev.stream)
        dev.close()


if __name__ == "__main__":
    main()
