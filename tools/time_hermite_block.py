"""Block time steps of the Hermite integrator (nbody_hermite_block_*), timed in ONE process per table (boxes of the pool differ by
several percent: only an interleaved comparison in one session says anything).
    python tools/time_hermite_block.py [--quick] [a] [b] [c]      the three tables below (default: all), profiler off
    python tools/time_hermite_block.py --trace N                   the block steps of table (b) for N bodies, nothing timed: run it as
        rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_hermite_block.py --trace N
    python tools/time_hermite_block.py --summarize DIR             the split of a block step into its launches from that trace
(a) a block step with every body active (max_level = 0) against nbody_hermite_step, 3D galaxy, eps = 0.05: N = 65 536 and 2^20 in
    double, 262 144 in float.  HIP events around `reps` calls, the two forms alternated, median and min .. max of the rounds.  The pair
    loop and its launch shape are the same, so the difference is the schedule (4 launches), the gather and the 8-byte read-back.
(b) time per block step against n_act in {1, 64, 1024, 16 384, N}, N = 65 536 and 2^20 in double: HIP events around every single call
    (first launch of the schedule .. corrector, the read-back in between included) and the host clock around call + synchronise.
    The active sets are made by construction: 16 384 evenly spaced bodies of the galaxy lose their mass, and n_act of them get a
    velocity so large that eta_start |a| / |j| lies below the smallest step; with max_level = 4 fifteen of sixteen block steps then
    have exactly those n_act bodies active and the sixteenth all N.  dt is chosen so that every other body stays at level 0.  A
    row is printed only if every timed step had the n_act it was built for.
(c) wall time to t = 0.5 of the binary-in-a-cluster case of tests/test_gpu_hermite_block.py (N = 512) and to t = 0.125 of an
    N = 65 536 cluster with 64 such binaries, block steps against fixed steps, with the |dE / E| each reaches."""
import collections
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

EPS = 0.05
ETA_START, TRACER_LEVELS, CANDIDATES = 3e-3, 4, 16384


def events(stream):
    import torch
    s = torch.cuda.ExternalStream(stream)
    return s, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(stream, fn, reps):
    s, e0, e1 = events(stream)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(v):
    return f"{statistics.median(v):10.3f} ms ({min(v):.3f} .. {max(v):.3f})"


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------
def table_a(nb, quick):
    print("(a) every body active: nbody_hermite_block_step with max_level = 0 against nbody_hermite_step; median (min .. max) of the rounds")
    for tname, dtype, n in (("f64", nb.F64, 65536), ("f64", nb.F64, 1 << 20), ("f32", nb.F32, 262144)):
        n = n // 8 if quick else n
        hs = nb.build_model(dtype, 3, "galaxy", n)
        fixed, block = nb.DeviceSystem.from_host(hs), nb.DeviceSystem.from_host(hs)
        fixed.hermite_start(EPS)
        block.hermite_block_start(EPS, 0.01, 0)
        forms = ((fixed, lambda: fixed.hermite_step(EPS)), (block, lambda: block.hermite_block_step(EPS, 0.02)))
        for _, f in forms:
            f()
        fixed.sync()
        reps, rounds = (2 if n > 500000 else 20), (4 if n > 500000 else 7)
        ms = [[], []]
        for _ in range(rounds):
            for k, (d, f) in enumerate(forms):
                ms[k].append(timed(d.stream, f, reps))
        ratio = statistics.median(ms[1]) / statistics.median(ms[0])
        print(f"{tname} 3D galaxy N={hs.n:<8d} step {spread(ms[0])}   block step {spread(ms[1])}   ratio {ratio:.4f}", flush=True)
        fixed.close()
        block.close()


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------
def tracer_case(nb, n):
    """The galaxy with CANDIDATES massless bodies; returns (hs, candidate indices, speed) with hs.dt set so that every body is at level
    0 unless it is given `speed`."""
    hs = nb.build_model(nb.F64, 3, "galaxy", n)
    light = np.nonzero(hs.m <= 10 * np.median(hs.m))[0]  # not the central mass of a disc
    ncand = min(CANDIDATES, n // 4)
    cand = light[:: len(light) // ncand][:ncand]
    hs.m[cand] = 0.0
    nrm = lambda q: np.sqrt((q * q).sum(-1))
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite_start(EPS)
    r = nrm(dev.download().a) / nrm(dev.hermite_jerk())
    hs.dt = float(ETA_START * r.min() / 4)  # every body as it is: want >= 4 dt
    trial = 1e3 * np.abs(hs.v).max()
    fast = nb.HostSystem(hs.dtype, 3, n)
    for k in ("m", "x", "v", "a", "ao"):
        getattr(fast, k)[:] = getattr(hs, k)
    fast.dt, fast.c = hs.dt, hs.c
    fast.v[cand] = [trial, 0.0, 0.0]
    dev.upload(fast)
    dev.hermite_start(EPS)
    rt = (nrm(dev.download().a) / nrm(dev.hermite_jerk()))[cand]  # ~ 1 / speed
    dev.close()
    tick = hs.dt / 2 ** TRACER_LEVELS
    speed = trial * ETA_START * rt.max() / (tick / 4)  # the slowest-changing tracer: want = tick / 4
    return hs, cand, float(speed)


def tracer_system(nb, hs, cand, speed, k):
    out = nb.HostSystem(hs.dtype, 3, hs.n)
    for f in ("m", "x", "v", "a", "ao"):
        getattr(out, f)[:] = getattr(hs, f)
    out.dt, out.c = hs.dt, hs.c
    out.v[cand[:: len(cand) // k][:k]] = [speed, 0.0, 0.0]
    return out


def table_b(nb, quick, trace_n=None):
    if trace_n is None:
        print("(b) time per block step against n_act (double, 3D galaxy, eps = 0.05): HIP events around one call | host clock around call + sync;"
              " medians")
    for n in ((65536, 1 << 20) if trace_n is None else (trace_n,)):
        n = n // 8 if quick else n
        hs, cand, speed = tracer_case(nb, n)
        eta, all_active = ETA_START ** 2, []
        for k in (k for k in (1, 64, 1024, 16384) if k <= len(cand)):
            dev = nb.DeviceSystem.from_host(tracer_system(nb, hs, cand, speed, k))
            dev.hermite_block_start(EPS, ETA_START, TRACER_LEVELS)
            dev.sync()
            s, e0, e1 = events(dev.stream)
            ev, wall, ok = [], [], True
            for interval in range(1 if trace_n else 3):
                for step in range(1 << 20):  # until the interval is complete
                    t0 = time.perf_counter()
                    e0.record(s)
                    n_act, tau = dev.hermite_block_step(EPS, eta)
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
    """Per class of block step (the grid of its force + jerk launch), per launch: median kernel time and median idle time before it."""
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    name = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "").replace("nbody::", "").split("<")[0]
    rows = [r for r in rows if name(r).startswith(("block_sched_", "hermite_block_"))]
    steps, cur = [], []
    for r in rows:
        if name(r) == "hermite_block_init_kernel":
            cur = []
            continue
        cur.append(r)
        if name(r) == "hermite_block_correct_kernel":
            steps.append(cur)
            cur = []
    head = ("block_sched_min_kernel", "block_sched_count_kernel", "block_sched_scan_kernel", "block_sched_compact_kernel",
            "hermite_block_predict_kernel", "hermite_block_active_kernel")
    classes = collections.defaultdict(list)
    for s in steps:  # with or without hermite_block_reduce_kernel in front of the corrector
        if tuple(name(r) for r in s[:6]) == head and len(s) in (7, 8):
            a = s[5]
            wg = int(a.get("Workgroup_Size_X", 256) or 256)
            classes[(int(a["Grid_Size_X"]) // wg, int(a["Grid_Size_Y"]))].append(s)
    for (bx, by), ss in sorted(classes.items()):
        shape = tuple(name(r) for r in ss[0])
        ss = [s for s in ss if len(s) == len(shape)]
        phase = ("schedule", "schedule", "schedule", "schedule", "predict", "force + jerk") + ("correct",) * (len(shape) - 6)
        print(f"force + jerk grid {bx} x {by} blocks: {len(ss)} block steps ({os.path.basename(f)})")
        print(f"  {'launch':32s} {'kernel us':>10s} {'idle before us':>15s}")
        tot = collections.OrderedDict()
        for j in range(len(shape)):
            dur = statistics.median((int(s[j]["End_Timestamp"]) - int(s[j]["Start_Timestamp"])) / 1e3 for s in ss)
            gap = statistics.median((int(s[j]["Start_Timestamp"]) - int(s[j - 1]["End_Timestamp"])) / 1e3 for s in ss) if j else 0.0
            print(f"  {shape[j]:32s} {dur:10.2f} {gap:15.2f}")
            # the wait in front of the force + jerk is the read-back: synchronise, 8 bytes, plan, launch
            key = "read-back" if j == 5 else phase[j]
            tot[key] = tot.get(key, 0.0) + gap
            tot[phase[j]] = tot.get(phase[j], 0.0) + dur
        span = statistics.median((int(s[-1]["End_Timestamp"]) - int(s[0]["Start_Timestamp"])) / 1e3 for s in ss)
        print("  " + "  ".join(f"{k} {v:.1f}" for k, v in tot.items()) + f"  | first launch .. corrector {span:.1f} us (device clock)")


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------
def binaries(nb, n, nbin, sep, eps, dt, seed=2024):
    rng = np.random.default_rng(seed)
    m = np.full(n, 1.0 / n)
    x, v = rng.normal(0, 1, (n, 3)), rng.normal(0, 0.3, (n, 3))
    vc = np.sqrt(2.0 / n / sep) * (sep * sep / (sep * sep + eps * eps)) ** 0.75
    for b in range(nbin):
        x[2 * b + 1] = x[2 * b] + [sep, 0, 0]
        v[2 * b + 1] = v[2 * b] + [0, vc, 0]
    hs = nb.HostSystem(nb.F64, 3, n)
    hs.m[:], hs.x[:], hs.v[:] = m, x, v
    hs.dt, hs.c = dt, 1.0
    return hs


def table_c(nb, quick):
    print("(c) wall time (host clock, synchronised) and |dE / E|, double; dt_max = 1/16, max_level = 12, eta_start = 0.01")
    cases = (("1 binary of separation 0.004, eps 0.002, to t = 0.5", 512, 1, 0.004, 0.002, 8),
             ("64 binaries of separation 8e-4, eps 4e-4, to t = 0.125", 65536 // (8 if quick else 1), 64, 8e-4, 4e-4, 2))
    for label, n, nbin, sep, eps, nint in cases:
        print(f"N={n}, {label}")
        for eta in (0.02, 0.01):
            hs = binaries(nb, n, nbin, sep, eps, 1.0 / 16)
            dev = nb.DeviceSystem.from_host(hs)
            k0, p0 = dev.calc_energies(softening=eps)
            dev.hermite_block_start(eps, 0.01, 12)
            dev.sync()
            t0, bs, bod = time.perf_counter(), 0, 0
            for _ in range(nint):
                s, b = dev.hermite_block_advance(eps, eta)
                bs, bod = bs + s, bod + b
            dev.sync()
            w = time.perf_counter() - t0
            k1, p1 = dev.calc_energies(softening=eps)
            dev.close()
            print(f"  block steps eta={eta}: {w * 1e3:10.1f} ms  {bs} block steps, {bod} body steps ({bod / n:.1f} N)  "
                  f"|dE/E| {abs((k1 + p1 - k0 - p0) / (k0 + p0)):.3g}", flush=True)
        for sub in (4, 6, 8):
            hs = binaries(nb, n, nbin, sep, eps, 1.0 / 16 / 2 ** sub)
            dev = nb.DeviceSystem.from_host(hs)
            k0, p0 = dev.calc_energies(softening=eps)
            dev.hermite_start(eps)
            dev.sync()
            t0 = time.perf_counter()
            for _ in range(nint << sub):
                dev.hermite_step(eps)
            dev.sync()
            w = time.perf_counter() - t0
            k1, p1 = dev.calc_energies(softening=eps)
            dev.close()
            print(f"  fixed step dt_max/2^{sub}:  {w * 1e3:10.1f} ms  {nint << sub} steps  |dE/E| {abs((k1 + p1 - k0 - p0) / (k0 + p0)):.3g}", flush=True)


def main():
    args = sys.argv[1:]
    if "--summarize" in args:
        return summarize(args[args.index("--summarize") + 1])
    nb = load_package()
    quick = "--quick" in args
    if "--trace" in args:
        return table_b(nb, quick, int(args[args.index("--trace") + 1]))
    which = [a for a in args if a in ("a", "b", "c")] or ["a", "b", "c"]
    for w in which:
        {"a": table_a, "b": table_b, "c": table_c}[w](nb, quick)


if __name__ == "__main__":
    main()
