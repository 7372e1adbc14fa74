"""nbody_knn_compute (k nearest neighbours, local densities, density centre) at k = 6 and k = 16 against nbody_neighbours_compute on
the same input, in ONE process (boxes of the pool differ by several percent: only an interleaved comparison in one session says
anything).  Times are HIP events recorded on the context's own stream around `reps` back-to-back calls, the three forms alternated,
median of the rounds.
    python tools/time_knn.py [--quick]
Cases, 3D galaxy: N = 65 536 in double, N = 262 144 in float.  Columns: nbody_neighbours_compute (pack + sweep + finish + closest) and
nbody_knn_compute (pack + sweep + finish + summary) at k = 6 (list capacity 8) and k = 16 (capacity 16).  The sweeps alone come from
a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/time_knn.py): the launches of a compute are separate
kernels there.
Flop model behind the achieved / peak column of the kNN sweep's plain batch, counted instruction by instruction with FMA = 2: 3
subtractions (3), mul + 2 FMA for d2 (5), min / compare (1): 9 per pair in both types; the insertions are not counted, so the column
says how far the insertions and the occupancy keep the sweep from the plain batch's bound.  The neighbours sweep: 20 per pair in
double, 12 in float (tools/time_neighbours.py)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

EPS = 0.05
PEAK = {"f64": 78.6e12, "f32": 157.3e12}  # vector peak of the MI355X, FLOP/s
FLOPS = {"f64": (20, 9), "f32": (12, 9)}  # per pair: the neighbour sweep, the kNN sweep's plain batch


def timed(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    quick = "--quick" in sys.argv
    nb = load_package()
    print(f"{'case':34s} {'neighbours':>11s} {'knn k=6':>11s} {'knn k=16':>11s}   ratio to neighbours (6, 16)   achieved / peak (neighbours, 6, 16)")
    for tname, dtype, n in (("f64", nb.F64, 65536), ("f32", nb.F32, 262144)):
        n = n // 8 if quick else n
        hs = nb.build_model(dtype, 3, "galaxy", n)
        dev = nb.DeviceSystem.from_host(hs)
        forms = (lambda: dev.neighbours_compute(EPS), lambda: dev.knn_compute(6), lambda: dev.knn_compute(16))
        for f in forms:
            f()
        torch.cuda.synchronize()
        reps, rounds = 10, 5
        ms = [[] for _ in forms]
        for _ in range(rounds):
            for k, f in enumerate(forms):
                ms[k].append(timed(dev.stream, f, reps))
        med = [statistics.median(v) for v in ms]
        pairs = float(hs.n) ** 2
        fn, fk = FLOPS[tname]
        print(f"{tname} 3D galaxy N={hs.n:<16d} {med[0]:8.3f} ms {med[1]:8.3f} ms {med[2]:8.3f} ms   {med[1] / med[0]:.3f}, {med[2] / med[0]:.3f}"
              f"                 {pairs * fn / (med[0] * 1e-3) / PEAK[tname]:.3f}, {pairs * fk / (med[1] * 1e-3) / PEAK[tname]:.3f}, "
              f"{pairs * fk / (med[2] * 1e-3) / PEAK[tname]:.3f}", flush=True)
        dev.close()


if __name__ == "__main__":
    main()
