"""nbody_knn_compute by the tree-pruned method (NBODY_KNN_TREE) against the all-pairs method on the same input, in ONE process (boxes
of the pool differ by several percent: only an interleaved comparison in one session says anything).  Times are HIP events recorded
on the context's own stream around `reps` back-to-back calls, the methods alternated, median of the rounds.
    python tools/time_knn_tree.py [--quick]
1. all-pairs vs tree at the two cases of tools/time_knn.py (3D galaxy, N = 65 536 in double, N = 262 144 in float), k = 6 and 16;
2. the crossover: both methods at k = 6 on a ladder of N (3D galaxy, both types), to read off where the tree becomes the faster one;
3. tree only at N = 10^6, k = 6: galaxy and plummer, float and double, and the same galaxy with its bodies shuffled (the sort must
   make the order of the state irrelevant to speed).
A compute's split into sort / boxes / walk comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python
tools/time_knn_tree.py --quick, a run of its own): the launches of a compute are separate kernels there."""
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


def medians(dev, forms, reps, rounds):
    for f in forms:
        f()
    torch.cuda.synchronize()
    ms = [[] for _ in forms]
    for _ in range(rounds):
        for q, f in enumerate(forms):
            ms[q].append(timed(dev.stream, f, reps))
    return [statistics.median(v) for v in ms]


def shuffled(nb, hs):
    p = np.random.default_rng(17).permutation(hs.n)
    out = nb.HostSystem(hs.dtype, hs.dim, hs.n)
    out.m[:], out.x[:], out.v[:] = hs.m[p], hs.x[p], hs.v[p]
    out.dt, out.c = hs.dt, hs.c
    return out


def main():
    quick = "--quick" in sys.argv
    nb = load_package()
    types = (("f64", nb.F64), ("f32", nb.F32))

    print("1. all-pairs vs tree, 3D galaxy (ms per compute; ratio = tree / all-pairs)")
    for tname, dtype, n in (("f64", nb.F64, 65536), ("f32", nb.F32, 262144)):
        n = n // 8 if quick else n
        dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, "galaxy", n))
        for k in (6, 16):
            a, t = medians(dev, (lambda: dev.knn_compute(k), lambda: dev.knn_compute(k, "tree")), 10, 5)
            print(f"  {tname} N={n:<8d} k={k:<3d} all-pairs {a:9.3f}   tree {t:9.3f}   ratio {t / a:.4f}", flush=True)
        dev.close()

    print("2. the crossover, 3D galaxy, k = 6 (ms per compute)")
    for tname, dtype in types:
        for n in (1024, 2048, 4096, 8192, 16384, 32768) if not quick else (2048, 8192):
            dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, "galaxy", n))
            a, t = medians(dev, (lambda: dev.knn_compute(6), lambda: dev.knn_compute(6, "tree")), 20, 5)
            print(f"  {tname} N={n:<8d} all-pairs {a:9.4f}   tree {t:9.4f}   ratio {t / a:.4f}", flush=True)
            dev.close()

    print("3. tree only, k = 6 (ms per compute)")
    big = 1000000 // 8 if quick else 1000000
    for tname, dtype in types:
        for model in ("galaxy", "plummer", "galaxy shuffled"):
            hs = nb.build_model(dtype, 3, model.split()[0], big)
            if model.endswith("shuffled"):
                hs = shuffled(nb, hs)
            dev = nb.DeviceSystem.from_host(hs)
            (t,) = medians(dev, (lambda: dev.knn_compute(6, "tree"),), 5, 5)
            print(f"  {tname} N={big:<8d} {model:16s} tree {t:9.3f}", flush=True)
            dev.close()


if __name__ == "__main__":
    main()
