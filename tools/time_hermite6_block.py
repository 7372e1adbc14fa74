"""Block time steps of the sixth-order Hermite integrator (nbody_hermite6_block_*, double), timed in ONE process per table (boxes of
the pool differ by several percent: only an interleaved comparison in one session says anything).
    python tools/time_hermite6_block.py [--quick] [--parent-lib PATH] [a] [b] [c]     the three tables below (default: all), profiler off
    python tools/time_hermite6_block.py --trace N                  the block steps of table (b) for N bodies, nothing timed: run it as
        rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_hermite6_block.py --trace N
    python tools/time_hermite6_block.py --summarize DIR            the split of a block step into its launches from that trace
(a) a block step with every body active (max_level = 0) against nbody_hermite6_step, 3D galaxy, eps = 0.05, N = 65 536 and 2^20.  HIP
    events around `reps` calls, the forms alternated, median and min .. max of the rounds.  With --parent-lib the fixed step of a
    libnbody_hip.so built from the parent commit is a third form in the same rounds (its own handle, the same device arrays): the
    comparison the record wants is against the code before the block steps, not against the new build's fixed step.
(b) time per block step against n_act in {1, 64, 1024, 16 384, N}, N = 65 536 and 2^20: HIP events around every single call (first
    launch of the schedule .. corrector, the read-back in between included) and the host clock around call + synchronise.  The active
    sets are those of tools/time_hermite_block.py table (b), made by construction: massless tracers fast enough to sit at the
    deepest of max_level = 4 levels, every other body at level 0.  A row is void unless every timed step had the n_act it was built for.
(c) the binary in a cluster of tests/test_gpu_hermite6_block.py (N = 512, to t = 0.5, dt_max = 1/16, max_level = 12): wall time,
    counts and |dE / E| of the sixth-order block steps (eta = 0.3 and 0.2), of the fourth-order block steps (eta = 0.02 and 0.01) and of
    the sixth-order fixed step."""
import collections
import csv
import ctypes
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from conftest import load_package  # noqa: E402
import time_hermite_block as B  # noqa: E402  (events, timed, spread, the tracer systems, the binaries)

EPS, ETA_START, TRACER_LEVELS = B.EPS, B.ETA_START, B.TRACER_LEVELS
# The step criterion's eta in table (b).  A tracer starts with eta_start |a| / |j| = tick / 4 and must keep want < 2 ticks; every other
# body starts with >= 4 dt_max and must keep want >= dt_max, but eta (num / den)^(1/6) is a shorter time than eta |a| / |j| (with
# eta = eta_start the galaxy's bodies went deeper after the first interval and the rows were void): 4 x eta_start sits between.
ETA_STEP = 4 * ETA_START


class ParentStep:
    """nbody_hermite6_step of another build of the library on the arrays of a DeviceSystem of this one."""

    def __init__(self, path, dev):
        vp, d = ctypes.c_void_p, ctypes.c_double
        self.L = ctypes.CDLL(path)
        self.L.nbody_hermite6_create_on.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]
        self.L.nbody_hermite6_start.argtypes = self.L.nbody_hermite6_step.argtypes = [vp, vp, d, vp]
        self.L.nbody_hermite6_destroy.argtypes = [vp]
        self.L.nbody_hermite6_destroy.restype = None
        self.L.nbody_last_error.restype = ctypes.c_char_p
        self.h, self.dev = vp(), dev
        self.check(self.L.nbody_hermite6_create_on(ctypes.byref(self.h), dev.dtype, dev.dim, dev.n, dev.device))
        st = dev.state()
        self.check(self.L.nbody_hermite6_start(self.h, ctypes.byref(st), EPS, dev.stream))

    def check(self, rc):
        if rc:
            raise RuntimeError(self.L.nbody_last_error().decode())

    def step(self):
        st = self.dev.state()
        self.check(self.L.nbody_hermite6_step(self.h, ctypes.byref(st), EPS, self.dev.stream))

    def close(self):
        self.L.nbody_hermite6_destroy(self.h)


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------
def table_a(nb, quick, parent_lib):
    print("(a) every body active: nbody_hermite6_block_step with max_level = 0 against nbody_hermite6_step"
          + (" of this build and of the parent commit's" if parent_lib else "") + "; median (min .. max) of the rounds")
    for n in (65536, 1 << 20):
        n = n // 8 if quick else n
        hs = nb.build_model(nb.F64, 3, "galaxy", n)
        fixed, block = nb.DeviceSystem.from_host(hs), nb.DeviceSystem.from_host(hs)
        fixed.hermite6_start(EPS)
        block.hermite6_block_start(EPS, 0.3, 0)
        forms = [("step", fixed, lambda: fixed.hermite6_step(EPS)), ("block step", block, lambda: block.hermite6_block_step(EPS, 0.4))]
        pdev = parent = None
        if parent_lib:
            pdev = nb.DeviceSystem.from_host(hs)
            parent = ParentStep(parent_lib, pdev)
            forms.insert(0, ("parent's step", pdev, parent.step))
        for _, _, f in forms:
            f()
        fixed.sync()
        reps, rounds = (2 if n > 500000 else 20), (4 if n > 500000 else 7)
        ms = [[] for _ in forms]
        for _ in range(rounds):
            for k, (_, d, f) in enumerate(forms):
                ms[k].append(B.timed(d.stream, f, reps))
        base = statistics.median(ms[0])
        print(f"f64 3D galaxy N={hs.n:<8d} " + "   ".join(f"{name} {B.spread(v)}" for (name, _, _), v in zip(forms, ms))
              + f"   block step / {forms[0][0]} {statistics.median(ms[-1]) / base:.4f}", flush=True)
        if parent:
            parent.close()
            pdev.close()
        fixed.close()
        block.close()


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------
def table_b(nb, quick, trace_n=None):
    if trace_n is None:
        print("(b) time per block step against n_act (double, 3D galaxy, eps = 0.05): HIP events around one call | host clock around call + sync;"
              " medians")
    for n in ((65536, 1 << 20) if trace_n is None else (trace_n,)):
        n = n // 8 if quick else n
        hs, cand, speed = B.tracer_case(nb, n)
        all_active = []
        for k in (k for k in (1, 64, 1024, 16384) if k <= len(cand)):
            dev = nb.DeviceSystem.from_host(B.tracer_system(nb, hs, cand, speed, k))
            dev.hermite6_block_start(EPS, ETA_START, TRACER_LEVELS)
            dev.sync()
            s, e0, e1 = B.events(dev.stream)
            ev, wall, ok = [], [], True
            for interval in range(1 if trace_n else 3):
                for step in range(1 << 20):  # until the interval is complete
                    t0 = time.perf_counter()
                    e0.record(s)
                    n_act, tau = dev.hermite6_block_step(EPS, ETA_STEP)
                    e1.record(s)
                    e1.synchronize()
                    w = (time.perf_counter() - t0) * 1e3
                    last = tau == 1 << TRACER_LEVELS
                    ok = ok and n_act == (n if last else k)
                    if last:
                        all_active.append((e0.elapsed_time(e1), w))
                        break
                    if interval or step:  # the very first step loads the code objects
                        ev.append(e0.elapsed_time(e1))
                        wall.append(w)
            dev.close()
            if trace_n is None:
                print(f"N={n:<8d} n_act={k:<8d} {statistics.median(ev) * 1e3:10.1f} us | {statistics.median(wall) * 1e3:10.1f} us"
                      + ("" if ok else "   (NOT the active sets it was built for: row void)"), flush=True)
        if trace_n is None:
            print(f"N={n:<8d} n_act={n:<8d} {statistics.median(q[0] for q in all_active) * 1e3:10.1f} us | "
                  f"{statistics.median(q[1] for q in all_active) * 1e3:10.1f} us", flush=True)


def summarize(d):
    """Per class of block step (the grid of its force + jerk + snap launch), per launch: median kernel time and median idle time before it."""
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    name = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "").replace("nbody::", "").split("<")[0]
    rows = [r for r in rows if name(r).startswith(("block_sched_", "hermite6_block_", "hermite_block_"))]
    steps, cur = [], []
    for r in rows:
        if name(r) == "hermite_block_init_kernel":
            cur = []
            continue
        cur.append(r)
        if name(r) == "hermite6_block_correct_kernel":
            steps.append(cur)
            cur = []
    head = ("block_sched_min_kernel", "block_sched_count_kernel", "block_sched_scan_kernel", "block_sched_compact_kernel",
            "hermite6_block_predict_kernel", "hermite6_block_active_kernel")
    classes = collections.defaultdict(list)
    for s in steps:  # with or without hermite_block_reduce_kernel in front of the corrector
        if tuple(name(r) for r in s[:6]) == head and len(s) in (7, 8):
            a = s[5]
            wg = int(a.get("Workgroup_Size_X", 256) or 256)
            classes[(int(a["Grid_Size_X"]) // wg, int(a["Grid_Size_Y"]))].append(s)
    for (bx, by), ss in sorted(classes.items()):
        shape = tuple(name(r) for r in ss[0])
        ss = [s for s in ss if len(s) == len(shape)]
        phase = ("schedule", "schedule", "schedule", "schedule", "predict", "force + jerk + snap") + ("correct",) * (len(shape) - 6)
        print(f"force + jerk + snap grid {bx} x {by} blocks: {len(ss)} block steps ({os.path.basename(f)})")
        print(f"  {'launch':32s} {'kernel us':>10s} {'idle before us':>15s}")
        tot = collections.OrderedDict()
        for j in range(len(shape)):
            dur = statistics.median((int(s[j]["End_Timestamp"]) - int(s[j]["Start_Timestamp"])) / 1e3 for s in ss)
            gap = statistics.median((int(s[j]["Start_Timestamp"]) - int(s[j - 1]["End_Timestamp"])) / 1e3 for s in ss) if j else 0.0
            print(f"  {shape[j]:32s} {dur:10.2f} {gap:15.2f}")
            # the wait in front of the pair sum is the read-back: synchronise, 8 bytes, plan, launch
            key = "read-back" if j == 5 else phase[j]
            tot[key] = tot.get(key, 0.0) + gap
            tot[phase[j]] = tot.get(phase[j], 0.0) + dur
        span = statistics.median((int(s[-1]["End_Timestamp"]) - int(s[0]["Start_Timestamp"])) / 1e3 for s in ss)
        print("  " + "  ".join(f"{k} {v:.1f}" for k, v in tot.items()) + f"  | first launch .. corrector {span:.1f} us (device clock)")


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------
def table_c(nb, quick):
    print("(c) N = 512, 1 binary of separation 0.004, eps 0.002, to t = 0.5, double; dt_max = 1/16, max_level = 12, eta_start = 0.01;"
          " wall time (host clock, synchronised) and |dE / E|")
    n, sep, eps, nint = 512, 0.004, 0.002, 8

    def run(label, start, advance, steps):
        hs = B.binaries(nb, n, 1, sep, eps, 1.0 / 16 / steps)
        dev = nb.DeviceSystem.from_host(hs)
        k0, p0 = dev.calc_energies(softening=eps)
        start(dev)
        dev.sync()
        t0, bs, bod = time.perf_counter(), 0, 0
        for _ in range(nint * steps):
            s, b = advance(dev)
            bs, bod = bs + s, bod + b
        dev.sync()
        w = time.perf_counter() - t0
        k1, p1 = dev.calc_energies(softening=eps)
        dev.close()
        print(f"  {label:32s} {w * 1e3:10.1f} ms  {bs} block steps, {bod} body steps ({bod / n:.1f} N)  "
              f"|dE/E| {abs((k1 + p1 - k0 - p0) / (k0 + p0)):.3g}", flush=True)

    for eta in (0.3, 0.2):
        run(f"order 6 block steps eta={eta}", lambda d: d.hermite6_block_start(eps, 0.01, 12), lambda d: d.hermite6_block_advance(eps, eta), 1)
    for eta in (0.02, 0.01):
        run(f"order 4 block steps eta={eta}", lambda d: d.hermite_block_start(eps, 0.01, 12), lambda d: d.hermite_block_advance(eps, eta), 1)
    for sub in (4, 6, 8):
        run(f"order 6 fixed step dt_max/2^{sub}", lambda d: d.hermite6_start(eps), lambda d: (d.hermite6_step(eps), (1, n))[1], 1 << sub)


def main():
    args = sys.argv[1:]
    if "--summarize" in args:
        return summarize(args[args.index("--summarize") + 1])
    nb = load_package()
    quick = "--quick" in args
    if "--trace" in args:
        return table_b(nb, quick, int(args[args.index("--trace") + 1]))
    parent_lib = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
    which = [a for a in args if a in ("a", "b", "c")] or ["a", "b", "c"]
    for w in which:
        if w == "a":
            table_a(nb, quick, parent_lib)
        else:
            {"b": table_b, "c": table_c}[w](nb, quick)


if __name__ == "__main__":
    main()
