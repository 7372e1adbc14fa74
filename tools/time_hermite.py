"""The Hermite force + jerk phase and step against the softened K1 in both its forms, in ONE process (boxes of the pool differ by
several percent: only an interleaved comparison in one session says anything).  Times are HIP events recorded on the context's own
stream around `reps` back-to-back calls, the four forms alternated, median of the rounds.
    python tools/time_hermite.py [--quick]
Cases, 3D galaxy: N = 65 536 and 2^20 in double, N = 262 144 in float.  Columns: nbody_all_pairs_softened_force as LDS tiles
(source_path = 1 with 4 source slices, its most: the yardstick — the same launch structure with about half the arithmetic) and on auto; nbody_hermite_force_jerk
(records of the state as it is + pair kernel + scale) and nbody_hermite_step (predict + pair kernel + correct).  The pair kernel
alone, and predict + correct beside it, come from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python
tools/time_hermite.py): the three launches of a step are separate kernels there.
Flop model behind the achieved / peak columns: the project's nominal 20 per ordered pair for the force plus what the
jerk adds, counted instruction by instruction with FMA = 2: 3 subtractions for u, 1 mul + 2 FMA for d.u (5), alpha (double: -3 A,
fma(e, e, e), fma, mul = 6; float: two mul = 2), 3 FMA for t (6), 3 FMA to accumulate (6): 26 in double, 22 in float; 46 and 42
per pair."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

EPS = 0.05
PEAK = {"f64": 78.6e12, "f32": 157.3e12}  # vector peak of the MI355X, FLOP/s
FLOPS = {"f64": (20, 46), "f32": (20, 42)}  # per pair: softened force, force + jerk


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
    print(f"{'case':34s} {'K1 soft tile':>13s} {'K1 soft auto':>13s} {'force_jerk':>11s} {'step':>9s}   ratio to tile   achieved / peak (K1 tile, force_jerk)")
    for tname, dtype, n in (("f64", nb.F64, 65536), ("f64", nb.F64, 1 << 20), ("f32", nb.F32, 262144)):
        n = n // 8 if quick else n
        hs = nb.build_model(dtype, 3, "galaxy", n)
        tile, auto = nb.DeviceSystem.from_host(hs), nb.DeviceSystem.from_host(hs)
        tile.configure_all_pairs(split=4, source_path=1)  # the tile form has at most 4 source slices
        herm = nb.DeviceSystem.from_host(hs)
        herm.hermite_start(EPS)
        forms = (lambda: tile.all_pairs_softened_force(EPS), lambda: auto.all_pairs_softened_force(EPS),
                 lambda: herm.hermite_start(EPS), lambda: herm.hermite_step(EPS))
        devs = (tile, auto, herm, herm)
        for f in forms:
            f()
        torch.cuda.synchronize()
        reps, rounds = (2 if n > 500000 else 10), 5
        ms = [[] for _ in forms]
        for _ in range(rounds):
            for k, f in enumerate(forms):
                ms[k].append(timed(devs[k].stream, f, reps))
        med = [statistics.median(v) for v in ms]
        pairs = float(hs.n) ** 2
        fk1, fh = FLOPS[tname]
        print(f"{tname} 3D galaxy N={hs.n:<16d} {med[0]:10.3f} ms {med[1]:10.3f} ms {med[2]:8.3f} ms {med[3]:6.3f} ms   "
              f"{med[2] / med[0]:.3f} / {med[3] / med[0]:.3f}   "
              f"{pairs * fk1 / (med[0] * 1e-3) / PEAK[tname]:.3f}, {pairs * fh / (med[2] * 1e-3) / PEAK[tname]:.3f}", flush=True)
        print("   ", nb.describe_all_pairs(tile.state()), "|", nb.describe_all_pairs(auto.state()))
        for d in (tile, auto, herm):
            d.close()


if __name__ == "__main__":
    main()
