"""The sixth-order Hermite step (nbody_hermite6_step: predict + force, jerk and snap + correct) against the fourth-order one
(nbody_hermite_step) in ONE process (boxes of the pool differ by several percent: only an interleaved comparison in one session says
anything).  Times are HIP events recorded on the context's own stream around `reps` back-to-back calls, the two forms alternated,
median of the rounds; the shader clock is sampled with rocm-smi while a case is timed (bench.Telemetry).
    python tools/time_hermite6.py [--quick]
Cases, 3D galaxy, eps = 0.05: N = 4096, 65 536 and 262 144 in double, N = 262 144 in float.
VALU fraction: vector instructions of the pair loop per ordered pair, read from the code object (f64: 33 + the rsq for the fourth
order, 55 + the rsq for the sixth; f32: 27 + 1 and 49 + 1), times N^2 pairs, over what the CUs can issue in the measured time at the
sampled clock: 64 lanes per CU and clock in double, 128 in float (the chip's 78.6 / 157.3 TFLOP/s vector peaks at 2.4 GHz, FMA = 2).
At 2400 MHz nominal when rocm-smi gave no sample.  Padding pairs (zero-mass records up to a whole tile of 256, lanes past the last
body) are issued too and not counted: at N = 4096 and above they are below 2 %."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from conftest import load_package  # noqa: E402
import bench  # noqa: E402

EPS = 0.05
INSTR = {"f64": (34, 56), "f32": (28, 50)}  # per pair, the rsq included: fourth order, sixth order
LANES = {"f64": 64, "f32": 128}  # per CU and clock


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
    arch, cus = nb.device_info(0)
    print(f"{arch}, {cus} CUs")
    print(f"{'case':28s} {'4th step':>11s} {'6th step':>11s} {'6th start':>11s}  ratio   sclk MHz (min .. max)   VALU fraction 4th, 6th")
    for tname, dtype, n in (("f64", nb.F64, 4096), ("f64", nb.F64, 65536), ("f64", nb.F64, 262144), ("f32", nb.F32, 262144)):
        n = n // 8 if quick else n
        hs = nb.build_model(dtype, 3, "galaxy", n)
        h4, h6 = nb.DeviceSystem.from_host(hs), nb.DeviceSystem.from_host(hs)
        h4.hermite_start(EPS)
        h6.hermite6_start(EPS)
        forms = (lambda: h4.hermite_step(EPS), lambda: h6.hermite6_step(EPS), lambda: h6.hermite6_start(EPS))
        devs = (h4, h6, h6)
        for f in forms:
            f()
        torch.cuda.synchronize()
        reps, rounds = (3 if n > 100000 else 20 if n > 10000 else 200), 5
        ms = [[] for _ in forms]
        tele = bench.Telemetry(0)
        with tele:
            for _ in range(rounds):
                for k, f in enumerate(forms):
                    ms[k].append(timed(devs[k].stream, f, reps))
        med = [statistics.median(v) for v in ms]
        s = tele.summary() or {}
        clk = s.get("sclk_mhz_mean") or 2400.0
        frac = [float(hs.n) ** 2 * INSTR[tname][k] / (med[k] * 1e-3 * cus * LANES[tname] * clk * 1e6) for k in (0, 1)]
        span = f"{clk:.0f} ({s['sclk_mhz_min']:.0f} .. {s['sclk_mhz_max']:.0f}, {s['samples']} samples)" if s else "not sampled: 2400 nominal"
        print(f"{tname} 3D galaxy N={hs.n:<10d} {med[0]:8.3f} ms {med[1]:8.3f} ms {med[2]:8.3f} ms  {med[1] / med[0]:.3f}   {span}   "
              f"{frac[0]:.3f}, {frac[1]:.3f}", flush=True)
        for d in (h4, h6):
            d.close()


if __name__ == "__main__":
    main()
