"""nbody_neighbours_compute (per-body potentials, nearest neighbours, closest pair) against the softened K1 and the fourth-order
Hermite force + jerk, in ONE process (boxes of the pool differ by several percent: only an interleaved comparison in one session says
anything).  Times are HIP events recorded on the context's own stream around `reps` back-to-back calls, the three forms alternated,
median of the rounds.
    python tools/time_neighbours.py [--quick]
Cases, 3D galaxy: N = 65 536 in double, N = 262 144 in float.  Columns: nbody_all_pairs_softened_force on auto, nbody_hermite_force_jerk
(records + pair kernel + scale: the same skeleton with about twice the arithmetic per pair) and nbody_neighbours_compute (pack +
sweep + finish + closest).  The sweep alone comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python
tools/time_neighbours.py): the four launches of a compute are separate kernels there.
Flop model behind the achieved / peak column of the sweep, counted instruction by instruction with FMA = 2 and the reciprocal square
root not counted: 3 subtractions (3), mul + 2 FMA for d2 (5), + e2 (1), the weight (double: y y, fma, fma, m y, p e, fma = 9; float:
m y = 1), the add into the slice sum (1), min / compare (1): 20 per pair in double, 12 in float.  force + jerk: 46 and 42
(tools/time_hermite.py)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

EPS = 0.05
PEAK = {"f64": 78.6e12, "f32": 157.3e12}  # vector peak of the MI355X, FLOP/s
FLOPS = {"f64": (46, 20), "f32": (42, 12)}  # per pair: force + jerk, the neighbour sweep


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
    print(f"{'case':34s} {'K1 soft auto':>13s} {'force_jerk':>11s} {'neighbours':>11s}   ratio to force_jerk   achieved / peak (force_jerk, neighbours)")
    for tname, dtype, n in (("f64", nb.F64, 65536), ("f32", nb.F32, 262144)):
        n = n // 8 if quick else n
        hs = nb.build_model(dtype, 3, "galaxy", n)
        k1, herm, nbr = nb.DeviceSystem.from_host(hs), nb.DeviceSystem.from_host(hs), nb.DeviceSystem.from_host(hs)
        forms = (lambda: k1.all_pairs_softened_force(EPS), lambda: herm.hermite_start(EPS), lambda: nbr.neighbours_compute(EPS))
        devs = (k1, herm, nbr)
        for f in forms:
            f()
        torch.cuda.synchronize()
        reps, rounds = 10, 5
        ms = [[] for _ in forms]
        for _ in range(rounds):
            for k, f in enumerate(forms):
                ms[k].append(timed(devs[k].stream, f, reps))
        med = [statistics.median(v) for v in ms]
        pairs = float(hs.n) ** 2
        fh, fn = FLOPS[tname]
        print(f"{tname} 3D galaxy N={hs.n:<16d} {med[0]:10.3f} ms {med[1]:8.3f} ms {med[2]:8.3f} ms   {med[2] / med[1]:.3f}                 "
              f"{pairs * fh / (med[1] * 1e-3) / PEAK[tname]:.3f}, {pairs * fn / (med[2] * 1e-3) / PEAK[tname]:.3f}", flush=True)
        print("   ", nb.describe_all_pairs(k1.state()))
        for d in devs:
            d.close()


if __name__ == "__main__":
    main()
