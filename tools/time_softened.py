"""Softened against unsoftened force phases, A/B in ONE process (boxes of the pool differ by several percent: only an interleaved
comparison in one session says anything about the pair form).  Times are HIP events recorded on the context's own stream around
`reps` back-to-back calls, the two forms alternated, median of the rounds.
    python tools/time_softened.py [--quick]
Cases: K1 at the headline shape (3D double galaxy, N = 2^20) and at config 3's size in float (N = 262 144); the octree walk alone
(walk form 1 against the softened walk, the same tree) at N = 10^6 galaxy in double and float.  Then the relative energy drift of
a softened (eps = 0.1) and an unsoftened galaxy run, N = 1024, double, 1000 steps of K1 + K3 (a measurement, not a bound)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

EPS = 0.1


def timed(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(name, stream, plain, soft, reps, rounds):
    plain(), soft()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(stream, plain, reps))
        b.append(timed(stream, soft, reps))
    ma, mb = statistics.median(a), statistics.median(b)
    print(f"{name:44s} unsoftened {ma:9.3f} ms  softened {mb:9.3f} ms  ratio {mb / ma:.4f}", flush=True)


def main():
    quick = "--quick" in sys.argv
    nb = load_package()
    for tname, dtype, n in (("f64", nb.F64, 1 << 20), ("f32", nb.F32, 262144)):
        n = n // 16 if quick else n
        dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, "galaxy", n))
        ab(f"K1 {tname} 3D galaxy N={n}", dev.stream, dev.all_pairs_force, lambda: dev.all_pairs_softened_force(EPS),
           reps=2 if n > 500000 else 5, rounds=5)
        print("   ", nb.describe_all_pairs(dev.state()))
        dev.close()
    for tname, dtype in (("f64", nb.F64), ("f32", nb.F32)):
        n = 62500 if quick else 1000000
        dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, "galaxy", n))
        dev.octree_force(0.5)  # builds the tree once; the A/B walks it
        t, st = dev.octree, dev.state()
        t.set_walk(1)
        ab(f"octree walk {tname} 3D galaxy N={n} theta=0.5", dev.stream, lambda: t.compute_force(st, 0.5, dev.stream),
           lambda: t.compute_softened_force(st, 0.5, EPS, dev.stream), reps=5, rounds=5)
        dev.close()
    steps = 100 if quick else 1000
    for eps in (0.0, EPS):
        hs = nb.build_model(nb.F64, 3, "galaxy", 1024)
        dev = nb.DeviceSystem.from_host(hs)
        k0, p0 = dev.calc_energies(softening=eps)
        for _ in range(steps):
            dev.all_pairs_softened_force(eps) if eps else dev.all_pairs_force()
            dev.accelerate_step()
        k1, p1 = dev.calc_energies(softening=eps)
        dev.close()
        e0, e1 = float(k0 + p0), float(k1 + p1)
        print(f"energy drift N=1024 f64 galaxy {steps} steps eps={eps}: E0 {e0:.12g} E {e1:.12g} |dE/E0| {abs(e1 - e0) / abs(e0):.3e}",
              flush=True)


if __name__ == "__main__":
    main()
